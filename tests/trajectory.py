"""Teacher-forced checks of the training step (test_cpu_trajectory.py, test_gpu_trajectory.py).

The tests of engine.TrainStep compare its modes with each other; a fault in the code the modes share
passes all of them.  A free-running comparison of trained weights with an independent trainer is no
help either: AdamW's first updates are about lr sign(g), one gradient element near zero flips an
update by 2 lr and the trajectories part.  So every step is judged on its own, from the product's
OWN state before it:

  gradient    the CPU oracle (oracle.gpt1_oracle.loss_and_grads, fp32) at the product's weights
              of step k, the product's batch, seed = the model's dropout seed, call = the dropout
              counter read before the step: loss and every named parameter's gradient.
              fp32 path: loss within 1e-5, per parameter max|got - ref| / max|ref| < 1e-4 (the bars of
              test_gpu_model.py::test_dropout_model_matches_oracle_fp32).  bf16 path: the rule of
              test_c2_full_size_bf16_step_matches_oracle as test_gpu_grad_targets.py applies it, per
              parameter by norm e_c < max(2e-2, 1.25 e_t) with cosine > 0.999, e_t the error of the
              oracle's forward under torch.autocast(bfloat16) on the same GPU from the same state;
              loss within 1 %.
  adamw       numerics.adamw_numpy (bit-equal to csrc/adamw.h) from the before-state, the product's
              own gradient, lr_k (the constant, or the schedule at the iteration the DRIVER counted),
              t = step count before + 1 and gscale = the clip coefficient: the after-state master, m
              and v bit for bit.  With clipping: opt.grad_norm within 2^-22 of the fp64 norm of the
              p.grads (which also shows they were left unscaled), coef = max_norm / (norm + 1e-6) to
              1e-6 when clipping, exactly 1 when not.
  counters    the dropout counter and the step count against the driver's own count: +1 per
              training-mode forward with p > 0 (backward or not), +0 per eval forward, +1 step per step.
  shadow      bf16 models: the bf16 shadow the next forward reads equals the master rounded to
              nearest-even, bit for bit, region by region.

`Checker` takes any trainer with the small observable interface below, so the CPU stand-in of
test_cpu_trajectory.py (the oracle itself, with faults planted) drives it as the product does.

TRAINER INTERFACE
  attributes   dtype ("fp32" | "bf16"), ocfg (oracle.OracleConfig), seed_base (dropout seed of rank 0),
               world, rank, hyper (b1, b2, eps, wd), max_norm (None: no clipping), lr_of(k)
  snapshot()   -> State(master, m, v: {name: float32 numpy}, step, counter)
  train_step() -> Obs(x, y, loss, grads {name: float32 numpy}, lr, norm, coef, shards)
                  shards: data parallel only, [(x, y)] per rank, derived from the generator state and
                  the CPU token stream, not from the rank's own buffers
  shadow()     -> [(region, master float32 numpy, shadow int16 numpy)] or None
  eval_loss(split) -> (x, y, loss);  probe() -> (x, y, loss): a training-mode forward, no backward
  resume(path) -> a fresh trainer that loaded the checkpoint this one saved

Not a conftest and no fixtures: plain helpers, as tests/numerics.py and tests/footprint.py.
"""
import collections
import hashlib
import math

import numpy as np
import torch

import numerics as nm
from oracle import gpt1_oracle as O

Record = collections.namedtuple("Record", "step what name measured bound ok")
State = collections.namedtuple("State", "master m v step counter")
Obs = collections.namedtuple("Obs", "x y loss grads lr norm coef shards")
Obs.__new__.__defaults__ = (None, None, None)

LR = 1e-3
DROPOUT = 0.2
RANK_KEY_STRIDE = 7919     # model.set_dropout_rank: rank r draws key base + 7919 r
FP32_LOSS, FP32_GRAD = 1e-5, 1e-4
BF16_LOSS, BF16_FLOOR, BF16_SLACK, BF16_COS = 1e-2, 2e-2, 1.25, 0.999
# The sampler's generator seed (both trainers).  The bf16 rule needs a seed at which torch's own bf16 path is
# inside it on all six steps, which at E's 1024 tokens it is for 17 of the 71 seeds 9 .. 79 (the HIP path
# for 19; DESIGN section 2, "Trajectory"): 38 is the first such seed for every mode at the constant
# learning rate, CLIP_DATA_SEED for the two clip + schedule modes, whose states differ.  A seed that stops
# being fair fails the "torch-bf16" records and is replaced; the bars are not.  The fp32 bars hold at any
# seed (RELU_LEVEL below: seeds 58 and 63, where the fp32 HIP path and the oracle decide one ReLU each way).
DATA_SEED = 38
CLIP_DATA_SEED = 72
# max_norm of the clip + schedule modes over the first step's measured norm: at seed 72 steps 0, 1, 3, 4
# clip and steps 2, 5 do not (asserted: both happen)
CLIP_OF_FIRST_NORM = 0.97
PLAN = (3, 1, 2)           # training steps before the evals, before the checkpoint, after the resume


def schedule(it):
    """warm-up, peak and four points of the cosine: a different learning rate on each of 6 steps."""
    from replicatinggpt_amd.schedule import warmup_cosine
    return warmup_cosine(2 * it, LR, 3, 13, 1e-4)


# ---------------------------------------------------------------------------------------
# the cached oracle
# ---------------------------------------------------------------------------------------
_CACHE = {}
CACHE_STATS = {"hit": 0, "miss": 0}


def _key(kind, master, x, y, ocfg, train, seed, call):
    h = hashlib.sha1()
    for name in sorted(master):
        h.update(np.ascontiguousarray(master[name]).tobytes())
    h.update(np.ascontiguousarray(x.numpy()).tobytes())
    h.update(np.ascontiguousarray(y.numpy()).tobytes())
    h.update(repr((kind, ocfg.block_size, ocfg.n_embd, ocfg.n_head, ocfg.n_layers, ocfg.dropout, bool(train),
                   int(seed), int(call), tuple(x.shape))).encode())
    return h.hexdigest()


def _cached(kind, fn, master, x, y, ocfg, train, seed, call):
    k = _key(kind, master, x, y, ocfg, train, seed, call)
    if k in _CACHE:
        CACHE_STATS["hit"] += 1
    else:
        CACHE_STATS["miss"] += 1
        _CACHE[k] = fn()
    return _CACHE[k]


def _params(master, dtype=torch.float32, device="cpu"):
    return {k: torch.from_numpy(np.array(v)).to(device=device, dtype=dtype) for k, v in master.items()}


def _oracle_run(P, x, y, ocfg, seed, call, toggles=(), backward=True):
    """O.loss_and_grads with the FeedForward ReLUs observed: (loss, grads, [pre-activation z per layer]).
    ``toggles``: (layer, flat index) hidden units whose ReLU takes the other decision -- relu(z) is
    computed as z * mask, the same values and derivative as torch.relu wherever the mask is z > 0."""
    zs, real = [], torch.relu
    by_layer = {}
    for l, i in toggles:
        by_layer.setdefault(l, []).append(i)

    def relu(z):
        l = len(zs)
        zs.append(z.detach())
        if l not in by_layer:
            return real(z)
        mask = z.detach() > 0
        idx = torch.tensor(by_layer[l])
        mask.view(-1)[idx] = ~mask.view(-1)[idx]
        return z * mask.to(z.dtype)
    torch.relu = relu
    try:
        if backward:
            _, loss, g = O.loss_and_grads(P, x, y, ocfg, train=True, seed=seed, call=call)
        else:
            with torch.no_grad():
                loss, g = O.forward(P, x, ocfg, y, True, seed, call)[1], None
    finally:
        torch.relu = real
    return loss, g, zs


def oracle_grads(master, x, y, ocfg, seed, call, dtype=torch.float32, toggles=()):
    """(loss, {name: gradient as float64 numpy}) of the CPU oracle's training forward / backward at
    ``master`` -- shared by key (weights, batch, call, seed) among the modes that are bit-identical."""
    def run():
        loss, g, _ = _oracle_run(_params(master, dtype), x, y, ocfg, seed, call, toggles)
        return float(loss), {k: v.double().numpy() for k, v in g.items()}
    return _cached(("grads", str(dtype), tuple(toggles)), run, master, x, y, ocfg, True, seed, call)


# A hidden unit whose pre-activation z is zero to within fp32 rounding has no ReLU decision that an
# fp32 evaluation could be held to: z > 0 in one correct evaluation, z <= 0 in another (another
# summation order, another machine's BLAS), and the unit's whole backward term switches with it -- 1e-3
# to 5e-2 of a gradient's maximum from one unit in 10^6, seen between the fp32 and the fp64 oracle
# (sampler seeds 25, 46, 62), between two machines' fp32 oracles, and between the oracle and the fp32
# HIP path (seed 63, step 0: z = -1.5e-8 / -2.6e-8 in the fp32 / fp64 oracle).  The rounding level is
# measured, from the reference alone: E_l = max |z_fp32 - z_fp64| over layer l's units at this state.
# A unit with |z_fp64| <= RELU_LEVEL * E_l is UNDECIDED.  Where a gradient misses the bar against the
# oracle as it decided, the oracle with undecided units decided the other way is as valid an fp32
# reference, and the SAME bar is applied against each such reference: one unit decided the other way,
# then two (about 10 units of 10^6 are undecided at a state; with more than MAX_UNDECIDED per shard, or
# none, the miss stands; pairs are tried up to MAX_UNDECIDED units in all).  Every use is a "relu-decision" record.
RELU_LEVEL = 4.0
MAX_UNDECIDED = 16
MAX_DECIDED_OTHERWISE = 2


def undecided_units(master, x, y, ocfg, seed, call):
    """[(layer, flat index)] of the hidden units undecided at fp32 rounding level, and the level per layer."""
    z32 = _oracle_run(_params(master), x, y, ocfg, seed, call, backward=False)[2]
    z64 = _oracle_run(_params(master, torch.float64), x, y, ocfg, seed, call, backward=False)[2]
    units, levels = [], []
    for l, (a, b) in enumerate(zip(z32, z64)):
        level = float((a.double() - b).abs().max())
        levels.append(level)
        units += [(l, int(i)) for i in torch.nonzero(b.abs().reshape(-1) <= RELU_LEVEL * level).reshape(-1)]
    return units, levels


def oracle_loss(master, x, y, ocfg, train, seed=0, call=0):
    def run():
        with torch.no_grad():
            return float(O.forward(_params(master), x, ocfg, y, train, seed, call)[1])
    return _cached("loss", run, master, x, y, ocfg, train, seed, call)


def torch_bf16_grads(master, x, y, ocfg, seed, call, device="cuda"):
    """The same from the oracle's functional forward under autocast(bfloat16) on the GPU: the
    calibration e_t of the bf16 bar."""
    def run():
        P = _params(master, device=device)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            _, loss, g = O.loss_and_grads(P, x.to(device), y.to(device), ocfg, train=True, seed=seed, call=call)
        return float(loss), {k: v.double().cpu().numpy() for k, v in g.items()}
    return _cached("bf16", run, master, x, y, ocfg, True, seed, call)


# ---------------------------------------------------------------------------------------
# the per-step checker
# ---------------------------------------------------------------------------------------
def grad_norm64(grads):
    return math.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads.values()))


class Checker:
    """Judges what a trainer shows; every check appends a Record(step, what, name, measured, bound, ok).
    ``fp64``: also hold the fp32 oracle itself to an fp64 run of the same oracle at every visited
    state, at the fp32 bars (the control: the reference alone stays inside them on this data)."""

    def __init__(self, trainer, fp64=False, device="cuda"):
        self.records = []
        self.fp64 = fp64
        self.device = device
        self.k = 0                                  # training steps taken, counted here
        st = trainer.snapshot()
        self.counter = st.counter                   # dropout calls, counted here from the first state
        self.step0 = st.step
        self.names = sorted(st.master)

    def add(self, step, what, name, measured, bound, ok):
        self.records.append(Record(step, what, name, float(measured), float(bound), bool(ok)))

    def failures(self):
        return [r for r in self.records if not r.ok]

    # -- gradients -----------------------------------------------------------------------------
    def _reference(self, fn, tr, before, obs, **kw):
        """Loss of this rank's shard and the gradient the step must have applied: one rank: the
        oracle's; data parallel: the mean over the ranks' shards, rank r at key base + 7919 r."""
        if tr.world == 1:
            return fn(before.master, obs.x, obs.y, tr.ocfg, tr.seed_base, before.counter, **kw)
        per = [fn(before.master, sx, sy, tr.ocfg, tr.seed_base + RANK_KEY_STRIDE * r, before.counter, **kw)
               for r, (sx, sy) in enumerate(obs.shards)]
        mean = {n: sum(g[n] for _, g in per) / tr.world for n in per[0][1]}
        return per[tr.rank][0], mean

    def check_grads(self, tag, tr, before, obs):
        ref_loss, ref = self._reference(oracle_grads, tr, before, obs)
        assert set(obs.grads) == set(ref) == set(self.names)
        if tr.world > 1:
            want = obs.shards[tr.rank]
            same = torch.equal(obs.x, want[0]) and torch.equal(obs.y, want[1])
            self.add(tag, "batch", "rank shard of the global draw", 0.0 if same else 1.0, 0.0, same)
        dl = abs(obs.loss - ref_loss)
        if tr.dtype == "fp32":
            self.add(tag, "loss", "loss", dl, FP32_LOSS, dl < FP32_LOSS)
            got = {n: obs.grads[n].astype(np.float64) for n in self.names}
            for n, e in self._fp32_errors(tag, "grad", tr, before, obs, got, ref, torch.float32).items():
                self.add(tag, "grad", n, e, FP32_GRAD, e < FP32_GRAD)
        else:
            self.add(tag, "loss", "loss", dl, BF16_LOSS * ref_loss, dl < BF16_LOSS * ref_loss)
            _, ref_t = self._reference(torch_bf16_grads, tr, before, obs, device=self.device)
            for n in self.names:
                a, b = obs.grads[n].astype(np.float64).ravel(), ref[n].ravel()
                nb = np.linalg.norm(b)
                e_c = float(np.linalg.norm(a - b) / nb)
                e_t = float(np.linalg.norm(ref_t[n].ravel() - b) / nb)
                cos = float(a @ b / (np.linalg.norm(a) * nb))
                bound = max(BF16_FLOOR, BF16_SLACK * e_t)
                self.add(tag, "grad", n, e_c, bound, e_c < bound)
                self.add(tag, "cosine", n, 1.0 - cos, 1.0 - BF16_COS, cos > BF16_COS)
                # the calibration itself must be inside the rule: where torch's own bf16 path is not, the
                # batch is no fair test of anyone's (test_gpu_grad_targets.py's header) -- another seed, never the bar
                t = ref_t[n].ravel()
                cos_t = float(t @ b / (np.linalg.norm(t) * nb))
                self.add(tag, "torch-bf16", n, 1.0 - cos_t, 1.0 - BF16_COS, cos_t > BF16_COS)
        if self.fp64:
            l64, g64 = self._reference(oracle_grads, tr, before, obs, dtype=torch.float64)
            l32, g32 = self._reference(oracle_grads, tr, before, obs)
            self.add(tag, "oracle64", "loss", abs(l32 - l64), FP32_LOSS, abs(l32 - l64) < FP32_LOSS)
            for n, e in self._fp32_errors(tag, "oracle64", tr, before, obs, g32, g64, torch.float64).items():
                self.add(tag, "oracle64", n, e, FP32_GRAD, e < FP32_GRAD)

    def _fp32_errors(self, tag, what, tr, before, obs, got, ref, dtype):
        """{name: max|got - ref| / max|ref|} against the oracle (run in ``dtype``) as it decided its ReLUs
        or, where that misses the bar, against the first reference with undecided units decided the
        other way that meets it (the comment at RELU_LEVEL); the errors against ``ref`` if none does."""
        def errors(r):
            return {n: float(np.abs(got[n] - r[n]).max() / (np.abs(r[n]).max() + 1e-30)) for n in self.names}
        errs = errors(ref)
        if max(errs.values()) < FP32_GRAD:
            return errs
        shards = [(obs.x, obs.y)] if tr.world == 1 else obs.shards
        keys = [tr.seed_base + RANK_KEY_STRIDE * r for r in range(len(shards))]
        units = []
        for r, (sx, sy) in enumerate(shards):
            u, levels = undecided_units(before.master, sx, sy, tr.ocfg, keys[r], before.counter)
            units += [(r,) + t for t in u]
        if not 0 < len(units) <= MAX_UNDECIDED * len(shards):
            self.add(tag, "relu-decision", f"{what}: {len(units)} undecided units, the miss stands", len(units),
                     MAX_UNDECIDED, True)
            return errs
        import itertools
        most = MAX_DECIDED_OTHERWISE if len(units) <= MAX_UNDECIDED else 1     # pairs: 120 references at the most
        for chosen in itertools.chain.from_iterable(itertools.combinations(units, k) for k in range(1, most + 1)):
            per = [oracle_grads(before.master, sx, sy, tr.ocfg, keys[r], before.counter, dtype=dtype,
                                toggles=tuple((l, i) for rr, l, i in chosen if rr == r))[1]
                   for r, (sx, sy) in enumerate(shards)]
            alt = errors({n: sum(g[n] for g in per) / len(per) for n in self.names})
            if max(alt.values()) < FP32_GRAD:
                self.add(tag, "relu-decision", f"{what}: (shard, layer, unit) {list(chosen)} of {len(units)} undecided at "
                         f"|z| <= {RELU_LEVEL:g} x {max(levels):.1e}, decided the other way", len(chosen), MAX_UNDECIDED, True)
                return alt
        self.add(tag, "relu-decision", f"{what}: no decision of the {len(units)} undecided units meets the bar",
                 len(units), MAX_UNDECIDED, True)
        return errs

    # -- optimizer transition -----------------------------------------------------------------
    def check_adamw(self, tag, tr, before, obs, after):
        lr = tr.lr_of(self.k)
        self.add(tag, "lr", "lr", abs(obs.lr - lr), 0.0, obs.lr == lr)
        gscale = None
        if tr.max_norm is not None:
            n64 = grad_norm64(obs.grads)
            d = abs(obs.norm - n64)
            self.add(tag, "norm", "opt.grad_norm vs the p.grads (left unscaled)", d, 2.0 ** -22 * n64,
                     d <= 2.0 ** -22 * n64)
            if n64 + 1e-6 > tr.max_norm:
                want = tr.max_norm / (obs.norm + 1e-6)
                self.add(tag, "coef", "clipping", abs(obs.coef - want), 1e-6 * want,
                         obs.coef < 1.0 and abs(obs.coef - want) <= 1e-6 * want)
            else:
                self.add(tag, "coef", "not clipping", abs(obs.coef - 1.0), 0.0, obs.coef == 1.0)
            gscale = obs.coef
        b1, b2, eps, wd = tr.hyper
        t = before.step + 1
        for n in self.names:
            P, M, V = nm.adamw_numpy(before.master[n].ravel(), obs.grads[n].ravel(), before.m[n].ravel(),
                                     before.v[n].ravel(), lr, b1, b2, eps, wd, t, gscale)
            for what, want, got in (("master", P, after.master[n]), ("m", M, after.m[n]), ("v", V, after.v[n])):
                bad = int((want.view(np.uint32) != got.ravel().view(np.uint32)).sum())
                self.add(tag, "adamw", f"{n} [{what}]", bad, 0, bad == 0)

    def check_shadow(self, tag, tr):
        sh = tr.shadow()
        if sh is None:
            assert tr.dtype == "fp32"
            return
        for region, master, bits in sh:
            bad = int((nm.bf16_bits_of(master) != bits).sum())
            self.add(tag, "shadow", region, bad, 0, bad == 0)

    def _count(self, tag, st, name):
        self.add(tag, "counter", name, st.counter - self.counter, 0, st.counter == self.counter)
        self.add(tag, "step-count", name, st.step - (self.step0 + self.k), 0, st.step == self.step0 + self.k)

    # -- the events of the scenario ---------------------------------------------------------------
    def train_step(self, tr):
        tag = f"step {self.k}"
        before = tr.snapshot()          # before step(): early AdamW advances the count when the backward starts
        self._count(tag, before, "before the step")
        obs = tr.train_step()
        after = tr.snapshot()
        self.check_grads(tag, tr, before, obs)
        self.check_adamw(tag, tr, before, obs, after)
        self.k += 1
        self.counter += 1
        self._count(tag, after, "after the step")
        self.check_shadow(tag, tr)
        return obs

    def eval_loss(self, tr, split):
        tag = f"eval {split} after step {self.k - 1}"
        st = tr.snapshot()
        x, y, loss = tr.eval_loss(split)
        ref = oracle_loss(st.master, x, y, tr.ocfg, False)
        bar = FP32_LOSS if tr.dtype == "fp32" else BF16_LOSS * ref
        self.add(tag, "loss", "eval loss", abs(loss - ref), bar, abs(loss - ref) < bar)
        self._count(tag, tr.snapshot(), "after an eval forward")

    def probe(self, tr):
        tag = f"probe after step {self.k - 1}"
        st = tr.snapshot()
        x, y, loss = tr.probe()
        ref = oracle_loss(st.master, x, y, tr.ocfg, True, tr.seed_base + RANK_KEY_STRIDE * tr.rank, st.counter)
        bar = FP32_LOSS if tr.dtype == "fp32" else BF16_LOSS * ref
        self.add(tag, "loss", "training-mode loss", abs(loss - ref), bar, abs(loss - ref) < bar)
        self.counter += 1
        self._count(tag, tr.snapshot(), "after a training-mode forward without backward")


def run_scenario(tr, path, plan=PLAN, fp64=False, device="cuda", on_step=None):
    """plan[0] training steps; the two eval losses; a training-mode forward without backward; plan[1]
    steps; checkpoint, resume into fresh objects; plan[2] steps.  plan = (n, 0, 0) runs the n steps
    alone.  Returns (checker, the trainer that finished)."""
    ck = Checker(tr, fp64, device)

    def steps(n):
        for _ in range(n):
            obs = ck.train_step(tr)
            if on_step is not None:
                on_step(tr, ck, obs)
    steps(plan[0])
    if plan[1] or plan[2]:
        ck.eval_loss(tr, "train")
        ck.eval_loss(tr, "val")
        ck.probe(tr)
        steps(plan[1])
        tr = tr.resume(path)
        steps(plan[2])
    return ck, tr


def worst(records):
    """The record closest to (or furthest past) its bound; bitwise checks count their mismatches."""
    def ratio(r):
        if r.bound > 0:
            return r.measured / r.bound
        return math.inf if not r.ok else 0.0
    return max(records, key=ratio)


def summary(mode, ck):
    """One line per kind of check: how many, and the worst (step, name, measured, bound)."""
    lines = []
    for what in sorted({r.what for r in ck.records}):
        rs = [r for r in ck.records if r.what == what]
        w = worst(rs)
        lines.append(f"[trajectory {mode}] {what:10s} {len(rs):4d} checks, {sum(not r.ok for r in rs)} failed; worst "
                     f"{w.step}: {w.name}: {w.measured:.3e} (bound {w.bound:.3e})")
    return lines


# ---------------------------------------------------------------------------------------
# the CPU stand-in: the oracle as a trainer, with faults to plant
# ---------------------------------------------------------------------------------------
def synthetic_stream(device=None):
    from replicatinggpt_amd.data import TokenStream
    return TokenStream.synthetic(n_tokens=1 << 16, device=device)


def draw_windows(stream, gen, split, T, B, world):
    """BatchSampler.draw_ix and the windows it gathers, on the CPU: [(x, y)] per rank."""
    data = stream.train_cpu if split == "train" else stream.val_cpu
    ix = torch.randint(len(data) - T, (B * world,), generator=gen)
    return [O.windows(data, ix[r * B:(r + 1) * B], T) for r in range(world)]


class OracleTrainer:
    """The product's observable behaviour restated on the CPU: the fp32 oracle for the gradients
    (every rank's, under data parallelism), numerics.adamw_numpy for the update, a bf16 shadow of the
    master, the dropout counter, the step count, the iteration and checkpoint / resume.  ``fault``
    names one deliberate deviation (FAULTS); ``fault_at`` the training step it first shows at."""
    dtype = "fp32"
    hyper = (0.9, 0.999, 1e-8, 1e-2)

    def __init__(self, ocfg, B, init_seed=1337, data_seed=None, world=1, rank=0, clip=None, sched=None, fault=None,
                 fault_at=1, stale="blocks.0.ln2.weight"):
        self.ocfg, self.B, self.world, self.rank = ocfg, B, world, rank
        self.seed_base = 0x1337
        self.max_norm, self.sched = clip, sched
        self.fault, self.fault_at, self.stale = fault, fault_at, stale
        torch.manual_seed(init_seed)
        self.P = {k: v.numpy().copy() for k, v in O.init_params(ocfg).items()}
        self.m = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.P.items()}
        self.step = self.counter = self.it = 0
        self.stream = synthetic_stream()
        self.gen = torch.Generator().manual_seed(DATA_SEED if data_seed is None else data_seed)
        self.prev = {k: v.copy() for k, v in self.P.items()}     # the weights one step ago
        self.prev_norm = None
        self.prev_grads = None
        self.bits = {k: nm.bf16_bits_of(v) for k, v in self.P.items()}

    def lr_of(self, k):
        return self.sched(k) if self.sched is not None else LR

    def on(self, name):
        return self.fault == name and self.it >= self.fault_at

    def snapshot(self):
        cp = lambda d: {k: v.copy() for k, v in d.items()}
        return State(cp(self.P), cp(self.m), cp(self.v), self.step, self.counter)

    def shadow(self):
        return [(k, self.P[k].copy(), self.bits[k].copy()) for k in sorted(self.P)]

    def _batch(self, split):
        return draw_windows(self.stream, self.gen, split, self.ocfg.block_size, self.B, self.world)

    def _weights(self):
        """What the forward reads: the master, or with the stale-shadow fault one tensor a step old."""
        W = dict(self.P)
        if self.on("stale_shadow"):
            W[self.stale] = self.prev[self.stale]
        return W

    def _grads(self, W, x, y, seed, call):
        if not self.on("update_before_last_read"):
            return oracle_grads(W, x, y, self.ocfg, seed, call)
        # the matrix takes its AdamW update as soon as its own gradient is final -- before the dgrad
        # that still reads it: the forward sees W_k, the backward's saved copy is W_k+1
        name = self.stale
        W = dict(self.P)
        _, g0 = oracle_grads(W, x, y, self.ocfg, seed, call)   # its own gradient does not depend on the matrix
        b1, b2, eps, wd = self.hyper
        new, _, _ = nm.adamw_numpy(self.P[name].ravel(), g0[name].astype(np.float32).ravel(), self.m[name].ravel(),
                                   self.v[name].ravel(), self.lr_of(self.it), b1, b2, eps, wd, self.step + 1)
        new = torch.from_numpy(new.reshape(self.P[name].shape))
        leaf = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in W.items()}
        ptr = leaf[name].data_ptr()

        def pack(t):
            if t.data_ptr() == ptr and t.numel() == new.numel():
                return ("swap", t.shape == new.shape)
            return ("keep", t)

        def unpack(p):
            if p[0] == "keep":
                return p[1]
            return new if p[1] else new.t()
        with torch.autograd.graph.saved_tensors_hooks(pack, unpack):
            _, loss = O.forward(leaf, x, self.ocfg, y, True, seed, call)
        loss.backward()
        return float(loss.detach()), {k: v.grad.double().numpy() for k, v in leaf.items()}

    def train_step(self):
        shards = self._batch("train")
        call = self.counter - 1 if self.on("reuse_masks") else self.counter
        W = self._weights()
        order = list(range(self.world))
        if self.on("dp_swapped_shards"):
            order = order[::-1]
        per = []
        for r in range(self.world):
            key = self.seed_base + (0 if self.on("dp_shared_key") else RANK_KEY_STRIDE * r)
            per.append(self._grads(W, *shards[order[r]], key, call))
        div = 1 if self.on("dp_sum") else self.world
        grads = {k: (sum(g[k] for _, g in per) / div).astype(np.float32) for k in per[0][1]}
        if self.on("missed_zero") and self.prev_grads is not None:
            grads[self.stale] = grads[self.stale] + self.prev_grads[self.stale]
        lr = self.lr_of(max(self.it - 1, 0)) if self.on("late_schedule") else self.lr_of(self.it)
        norm = coef = None
        if self.max_norm is not None:
            norm = float(np.float32(grad_norm64(grads)))
            basis = self.prev_norm if (self.on("stale_clip_norm") and self.prev_norm is not None) else norm
            coef = float(np.float32(min(1.0, self.max_norm / (basis + 1e-6))))
            self.prev_norm = norm
        self.prev = {k: v.copy() for k, v in self.P.items()}
        self.prev_grads = grads
        b1, b2, eps, wd = self.hyper
        t = self.step + 1
        for k in self.P:
            P, M, V = nm.adamw_numpy(self.P[k].ravel(), grads[k].ravel(), self.m[k].ravel(), self.v[k].ravel(), lr,
                                     b1, b2, eps, wd, t, coef)
            self.P[k], self.m[k], self.v[k] = (a.reshape(self.P[k].shape) for a in (P, M, V))
            if not (self.on("stale_shadow") and k == self.stale):
                self.bits[k] = nm.bf16_bits_of(self.P[k])
        shown = grads
        if self.on("scaled_in_place") and coef is not None:
            shown = {k: (g * np.float32(coef)).astype(np.float32) for k, g in grads.items()}
        self.step += 1
        self.counter += 1
        self.it += 1
        x, y = shards[order[self.rank]]
        return Obs(x, y, per[self.rank][0], shown, lr, norm, coef, shards if self.world > 1 else None)

    def eval_loss(self, split):
        x, y = self._batch(split)[self.rank]
        if self.fault == "eval_consumes_call":
            self.counter += 1
        return x, y, oracle_loss(self.P, x, y, self.ocfg, False)

    def probe(self):
        x, y = self._batch("train")[self.rank]
        loss = oracle_loss(self.P, x, y, self.ocfg, True, self.seed_base + RANK_KEY_STRIDE * self.rank, self.counter)
        if self.fault != "probe_consumes_none":
            self.counter += 1
        return x, y, loss

    def resume(self, path):
        torch.save({"P": self.P, "m": self.m, "v": self.v, "step": self.step, "counter": self.counter, "it": self.it,
                    "rng": self.gen.get_state()}, path)
        new = OracleTrainer(self.ocfg, self.B, init_seed=99, data_seed=12345, world=self.world, rank=self.rank,
                            clip=self.max_norm, sched=self.sched, fault=self.fault, fault_at=self.fault_at,
                            stale=self.stale)
        ck = torch.load(path, weights_only=False)
        new.P, new.m, new.v = ck["P"], ck["m"], ck["v"]
        new.prev = {k: v.copy() for k, v in new.P.items()}
        new.bits = {k: nm.bf16_bits_of(v) for k, v in new.P.items()}
        new.counter, new.it = ck["counter"], ck["it"]
        new.step = 0 if self.fault == "step_not_restored" else ck["step"]
        new.gen.set_state(ck["rng"])
        return new


# fault -> (trainer arguments, the step it must be reported at, the checks of which one must report it)
FAULTS = {
    "reuse_masks": ({}, "step 1", ("loss", "grad")),
    "eval_consumes_call": ({}, "eval train after step 2", ("counter",)),
    "probe_consumes_none": ({}, "probe after step 2", ("counter",)),
    "stale_shadow:position_embedding_table.weight": ({}, "step 1", ("grad", "loss", "shadow")),
    "stale_shadow:blocks.0.ln2.weight": ({}, "step 1", ("grad", "loss", "shadow")),
    "update_before_last_read:blocks.1.ffwd.net.0.weight": ({}, "step 1", ("grad",)),
    "step_not_restored": ({}, "step 4", ("step-count",)),
    "late_schedule": ({"sched": True}, "step 1", ("lr", "adamw")),
    "stale_clip_norm": ({"clip": True}, "step 1", ("coef",)),
    "scaled_in_place": ({"clip": True}, "step 1", ("norm", "grad")),
    "missed_zero:blocks.1.sa_heads.proj.bias": ({}, "step 1", ("grad",)),
    "dp_shared_key": ({"world": 2}, "step 1", ("grad",)),
    "dp_sum": ({"world": 2}, "step 1", ("grad",)),
    "dp_swapped_shards": ({"world": 2}, "step 1", ("batch", "grad")),
}


# ---------------------------------------------------------------------------------------
# the product as a trainer
# ---------------------------------------------------------------------------------------
class ProductTrainer:
    """engine.TrainStep (or GPT1.py's loop written by hand: ``hand``) behind the trainer interface.
    ``build(seed)`` -> (model, optimizer): fresh objects, so resume() can make its own."""

    def __init__(self, gpt_cfg, B, hand=False, graph=True, segmented=False, clip=None, sched=None, world=1, rank=0,
                 init_seed=1337, data_seed=None, _resumed_from=None):
        from replicatinggpt_amd import AdamW, BigramLanguageModel
        from replicatinggpt_amd.data import BatchSampler
        from replicatinggpt_amd.engine import Evaluator, GradReducer, TrainStep
        self.args = dict(gpt_cfg=gpt_cfg, B=B, hand=hand, graph=graph, segmented=segmented, clip=clip, sched=sched,
                         world=world, rank=rank)
        self.data_seed = data_seed
        self.cfg, self.B, self.hand, self.world, self.rank = gpt_cfg, B, hand, world, rank
        self.dtype = gpt_cfg.dtype
        self.ocfg = O.OracleConfig(block_size=gpt_cfg.block_size, n_embd=gpt_cfg.n_embd, n_head=gpt_cfg.n_head,
                                   n_layers=gpt_cfg.n_layers, dropout=gpt_cfg.dropout)
        self.seed_base = gpt_cfg.dropout_seed
        self.max_norm, self.sched = clip, sched
        torch.manual_seed(init_seed)
        self.model = BigramLanguageModel(gpt_cfg).to("cuda")
        assert self.model.training
        kw = {}
        if clip is not None:
            kw["max_grad_norm"] = clip
        if sched is not None or clip is not None:
            kw["dynamic_lr"] = True
        self.opt = AdamW(self.model.parameters(), lr=LR, **kw).attach(self.model)
        grp = self.opt.param_groups[0]
        self.hyper = (grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"])
        self.stream = synthetic_stream("cuda")
        self.gen = torch.Generator().manual_seed(DATA_SEED if data_seed is None else data_seed)
        if _resumed_from is None:
            it = 0
        else:
            from replicatinggpt_amd import checkpoint
            torch.randint(10, (17,), generator=self.gen)     # a scrambled generator, a different init: all loaded
            it = checkpoint.load_checkpoint(_resumed_from, self.model, self.opt, generator=self.gen)
        self.sampler = BatchSampler(self.stream, gpt_cfg.block_size, B, world_size=world, rank=rank,
                                    generator=self.gen)
        self.evaluator = Evaluator(self.model, self.sampler)
        self.step = None
        self.it = it
        if not hand:
            red = None
            if world > 1:
                red = GradReducer(self.model.flat.grad, bucket_bytes=64 << 10)
            elif segmented:
                red = GradReducer(self.model.flat.grad)      # world size 1: the segmentation only
            self.step = TrainStep(self.model, self.opt, self.sampler, red, use_graph=graph,
                                  overlap=True if segmented else None, seg_layers=1, lr_schedule=sched)
            self.step.it = it
            self.step.capture(restore=True)
        self.named = dict(self.model.named_parameters())
        self.offs = {id(p): off for _, p, off in self.opt._param_slices()}

    def lr_of(self, k):
        return self.sched(k) if self.sched is not None else LR

    def snapshot(self):
        torch.cuda.synchronize()
        opt = self.opt
        opt._ensure()
        assert opt._psteps is None
        m_all, v_all = opt._m.cpu().numpy(), opt._v.cpu().numpy()
        master, m, v = {}, {}, {}
        for n, p in self.named.items():
            off, k = self.offs[id(p)], p.numel()
            master[n] = p.detach().cpu().numpy().copy()
            m[n] = m_all[off:off + k].reshape(p.shape).copy()
            v[n] = v_all[off:off + k].reshape(p.shape).copy()
        return State(master, m, v, int(opt._step_t.item()), int(self.model._rng_counter.item()))

    def shadow(self):
        if self.dtype != "bf16":
            return None
        if self.step is None or self.step.g_fb is None and not self.step.g_seg:
            self.model._sync_shadow()     # eager: the host-side check the next forward runs; a replay cannot
        torch.cuda.synchronize()
        st = self.model.flat
        master, bits = st.master.detach().cpu().numpy(), st.shadow.view(torch.int16).cpu().numpy()
        return [(key, master[o:o + n].copy(), bits[o:o + n].copy()) for key, (o, n) in st.offsets.items()]

    def train_step(self):
        gstate = self.gen.get_state()
        if self.step is not None:
            loss = self.step.step()
            x, y = self.step.x, self.step.y
        else:
            x, y = self.sampler.get_batch("train")
            _, loss = self.model(x, y)
            self.opt.zero_grad(set_to_none=True)
            loss.backward()
            self.opt.step()
        self.it += 1
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().cpu().numpy().copy() for n, p in self.named.items()}
        norm = coef = None
        if self.max_norm is not None:
            norm, coef = float(self.opt.grad_norm), float(self.opt.clip_coef)
        shards = None
        if self.world > 1:   # every rank's shard, from the generator state and the CPU copy of the tokens
            g = torch.Generator()
            g.set_state(gstate)
            shards = draw_windows(self.stream, g, "train", self.cfg.block_size, self.B, self.world)
        return Obs(x.cpu().clone(), y.cpu().clone(), float(loss.detach()), grads, self.opt.param_groups[0]["lr"], norm,
                   coef, shards)

    def eval_loss(self, split):
        self.model.eval()
        try:
            loss = float(self.evaluator.loss(split))
        finally:
            self.model.train()
        return self.evaluator.x.cpu().clone(), self.evaluator.y.cpu().clone(), loss

    def probe(self):
        x, y = self.sampler.get_batch("train")
        _, loss = self.model(x, y)
        return x.cpu().clone(), y.cpu().clone(), float(loss.detach())

    def resume(self, path):
        from replicatinggpt_amd import checkpoint
        torch.cuda.synchronize()
        it = self.step.it if self.step is not None else self.it
        checkpoint.save_checkpoint(path, self.model, self.opt, it, generator=self.gen)
        return ProductTrainer(**self.args, init_seed=99, data_seed=12345, _resumed_from=path)
