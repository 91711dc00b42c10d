"""Shapes off the bf16 training path's fast branches, and the two comparators that judge them
(test_cpu_twins.py, test_gpu_bf16_offpath.py).

ROW-PADDED TWINS.  A batch of B_r rows whose token count is off the fast path (the "ragged" batch)
and its twin: the same rows followed by B_a - B_r filler rows whose targets are all ignore_index,
with B_a chosen so that every fast-path predicate holds.  The loss is the mean over the same valid
tokens, attention never crosses rows, and the Philox element indices (((b H + h) T + q) T + k for the
attention, the flat [B T, C] index for the FeedForward) do not depend on B: with dropout on, both
runs compute the same function of the same operands with the same rounding points.  Only the kernels
(generic against persistent / MFMA / fused) and the fp32 summation orders differ, so the two runs are
held to conftest.bf16_close element by element (twin_records).

SHAPES WITH NO TWIN.  Width, head size, vocabulary and sequence length are the model's and cannot be
padded away; those shapes are held to the fp32 oracle by a rule relative to the oracle's own forward
under torch.autocast(bfloat16) (rule_records): per parameter, by norm,
    e_c < max(2e-2, 1.25 e_t)   and   1 - cos_c < max(2e-4, 1.5625 (1 - cos_t)),
the second line being the first one's 1.25 margin carried to the cosine (1 - cos ~ e^2 / 2), with every
e_t <= 6e-2 so that a noisy reference cannot hide a failure.

Plain helpers, no fixtures; everything here runs on CPU tensors."""
import torch
import torch.nn.functional as F

from conftest import bf16_close
from oracle import gpt1_oracle as O
from test_cpu_grad_targets import CASES, DATA_SEED, DROPOUT, INIT_SEED, N_LAYERS, micro_batches

IGNORE = -100

# every pair runs on this model (head size 64)
PAIR_MODEL = dict(block_size=64, n_embd=128, n_head=2, vocab_size=65)
# T: sequence length; B_r rows in the ragged batch; B_a rows in the twin
PAIRS = {
    "T1": dict(T=64, B_r=3, B_a=4),      # 192 tokens: M % 128 != 0, generic forward / dgrad GEMMs
    "T2": dict(T=64, B_r=9, B_a=10),     # 576 tokens: the same, grouped weight gradients at an uneven split (5 + 4)
    "T3": dict(T=48, B_r=3, B_a=8),      # 144 tokens: tokens % 64 != 0, every GEMM generic; generic attention in both
    "T4": dict(T=37, B_r=3, B_a=128),    # 111 tokens: tokens % 16 != 0, the plain bf16 head against the fused one
}

# T: one sequence length per micro-batch (the model's dropout calls 0, 1, ...)
SHAPES = {
    "X1": dict(B=8, T=(64,), block_size=64, n_embd=192, n_head=3, vocab_size=65),
    "X2": dict(B=4, T=(64,), block_size=64, n_embd=128, n_head=4, vocab_size=65),
    "X3": dict(B=CASES["O"]["B"], T=CASES["O"]["T"], block_size=CASES["O"]["block_size"],
               n_embd=CASES["O"]["n_embd"], n_head=CASES["O"]["n_head"], vocab_size=65),
    "X4": dict(B=4, T=(64,), block_size=64, n_embd=128, n_head=2, vocab_size=200),
    "X5": dict(B=2, T=(320,), block_size=320, n_embd=128, n_head=2, vocab_size=65),
}


def spec_of(name):
    """Model dimensions, B and T of pair or shape ``name`` (a pair: B is the ragged batch's)."""
    if name in PAIRS:
        p = PAIRS[name]
        return dict(PAIR_MODEL, B=p["B_r"], T=(p["T"],))
    return dict(SHAPES[name])


def oracle_config(spec):
    return O.OracleConfig(vocab_size=spec["vocab_size"], block_size=spec["block_size"], n_embd=spec["n_embd"],
                          n_head=spec["n_head"], n_layers=N_LAYERS, dropout=DROPOUT)


def oracle_params(spec, dtype=torch.float32):
    torch.manual_seed(INIT_SEED)
    return {k: v.to(dtype) for k, v in O.init_params(oracle_config(spec)).items()}


def make_pair(pair):
    """(ragged batch, twin batch) of CPU (idx, targets): one torch.Generator(DATA_SEED) draws the
    twin's idx and targets, the filler rows' targets are then all IGNORE, and the ragged batch is the
    twin's first B_r rows."""
    p = PAIRS[pair]
    gen = torch.Generator().manual_seed(DATA_SEED)
    V = PAIR_MODEL["vocab_size"]
    idx = torch.randint(0, V, (p["B_a"], p["T"]), generator=gen)
    tgt = torch.randint(0, V, (p["B_a"], p["T"]), generator=gen)
    ragged = (idx[:p["B_r"]].clone(), tgt[:p["B_r"]].clone())
    tgt[p["B_r"]:] = IGNORE
    return ragged, (idx, tgt)


def shape_batches(name):
    """[(idx, targets)] of shape ``name``, one per micro-batch, from one torch.Generator(DATA_SEED);
    X3 is CASES["O"]'s micro-batches A and B themselves."""
    if name == "X3":
        return micro_batches("O")
    s = SHAPES[name]
    gen = torch.Generator().manual_seed(DATA_SEED)
    out = []
    for T in s["T"]:
        idx = torch.randint(0, s["vocab_size"], (s["B"], T), generator=gen)
        tgt = torch.randint(0, s["vocab_size"], (s["B"], T), generator=gen)
        out.append((idx, tgt))
    return out


def oracle_step(P, idx, tgt, cfg, seed, call=0, ignore_index=None):
    """(logits [B T, V], loss, {name: grad}) of the oracle in training mode: O.forward without targets,
    then F.cross_entropy -- with ``ignore_index`` when given, else the plain mean of GPT1.py:192."""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    logits, _ = O.forward(leaf, idx, cfg, None, True, seed, call)
    logits = logits.reshape(-1, logits.shape[-1])
    kw = {} if ignore_index is None else {"ignore_index": ignore_index}
    loss = F.cross_entropy(logits, tgt.reshape(-1), **kw)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in leaf.items()}


# ---------------------------------------------------------------------------------------
# the twin comparator: conftest.bf16_close with its defaults, element by element
# ---------------------------------------------------------------------------------------
def loss_close(a, b):
    """The project's bf16 loss bar: within 1 % (test_gpu_grad_targets.check_loss)."""
    return abs(float(a) - float(b)) < 1e-2 * abs(float(b))


def twin_records(got, ref, rows=None):
    """``got`` and ``ref``: (loss, logits, {name: grad}); ``rows``: compare the first ``rows`` rows of
    the logits (the ragged run's B_r T), all when None.  Returns [(name, ok, stats)] with the loss as
    "loss" (stats: its absolute and relative difference) and the logits as "logits"."""
    (lg, zg, gg), (lr, zr, gr) = got, ref
    recs = [("loss", loss_close(lg, lr), dict(diff=abs(float(lg) - float(lr)),
                                              rel=abs(float(lg) - float(lr)) / abs(float(lr))))]
    n = zg.shape[0] if rows is None else rows
    recs.append(("logits", *bf16_close(zg[:n], zr[:n])))
    assert set(gg) == set(gr), sorted(set(gg) ^ set(gr))
    for name in gg:
        assert gg[name].shape == gr[name].shape, name
        recs.append((name, *bf16_close(gg[name], gr[name])))
    return recs


def twin_report(label, recs):
    """Prints the loss difference and the worst tensor of ``recs``; returns the failing records."""
    loss = recs[0][2]
    tens = recs[1:]
    worst = max(tens, key=lambda r: max(r[2]["worst_elem_ratio"], r[2]["maxrel"] / 2e-2, r[2]["normrel"] / 1e-2))
    print(f"[{label}] loss diff {loss['diff']:.3e} (rel {loss['rel']:.3e}); worst (name, worst_elem_ratio, maxrel, "
          f"normrel) = ({worst[0]}, {worst[2]['worst_elem_ratio']:.3e}, {worst[2]['maxrel']:.3e}, "
          f"{worst[2]['normrel']:.3e}); largest normrel {max(r[2]['normrel'] for r in tens):.3e}; logits maxrel "
          f"{tens[0][2]['maxrel']:.3e}")
    return [r for r in recs if not r[1]]


# ---------------------------------------------------------------------------------------
# the reference-relative rule against the fp32 oracle
# ---------------------------------------------------------------------------------------
E_FLOOR, E_MARGIN, COS_FLOOR, E_T_CAP = 2e-2, 1.25, 2e-4, 6e-2


def _err_cos(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / b.norm()), float(F.cosine_similarity(a, b, dim=0))


def rule_records(got, ref, ref_t):
    """Per parameter (name, e_c, e_t, cos_c, cos_t, ok): ``got`` the gradients under test, ``ref`` the
    fp32 oracle's, ``ref_t`` those of the oracle's forward under autocast(bfloat16)."""
    assert set(got) == set(ref) == set(ref_t)
    recs = []
    for name in got:
        e_c, cos_c = _err_cos(got[name], ref[name])
        e_t, cos_t = _err_cos(ref_t[name], ref[name])
        ok = e_c < max(E_FLOOR, E_MARGIN * e_t) and 1 - cos_c < max(COS_FLOOR, E_MARGIN ** 2 * (1 - cos_t))
        recs.append((name, e_c, e_t, cos_c, cos_t, ok))
    return recs


def rule_report(label, recs):
    """Prints the worst parameter of ``recs`` by each line of the rule and torch's own largest error;
    returns (failing records, records whose e_t is above the cap -- the "torch-bf16" record)."""
    we = max(recs, key=lambda r: r[1] / max(E_FLOOR, E_MARGIN * r[2]))
    wc = max(recs, key=lambda r: (1 - r[3]) / max(COS_FLOOR, E_MARGIN ** 2 * (1 - r[4])))
    wt = max(recs, key=lambda r: r[2])
    for tag, r in (("by error", we), ("by cosine", wc)):
        print(f"[{label}] worst {tag} (name, e_c, e_t, cos_c, cos_t) = ({r[0]}, {r[1]:.3e}, {r[2]:.3e}, {r[3]:.6f}, "
              f"{r[4]:.6f}); e_c / e_t = {r[1] / max(r[2], 1e-30):.3f}")
    print(f"[{label}] torch-bf16 largest e_t = {wt[2]:.3e} ({wt[0]}), cap {E_T_CAP:.0e}")
    return [r for r in recs if not r[5]], [r for r in recs if not r[2] <= E_T_CAP]
