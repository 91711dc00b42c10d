"""The control of tests/trajectory.py, as test_cpu_numerics.py and test_cpu_footprint.py are of their
checkers: a CPU stand-in trainer with the product's observable interface (trajectory.OracleTrainer:
the fp32 oracle, numerics.adamw_numpy, oracle/philox.py) runs the scenario of test_gpu_trajectory.py.

Unfaulted it passes every check -- among them the fp32 oracle against an fp64 run of the same oracle
at every visited state, which shows that the reference alone stays inside the fp32 bars on this data
(shape E with the GPU test's init seed, token stream and sampler seed: the states the fp32 GPU modes
visit, to their 1e-6).  That comparison depends on the machine: the fp32 oracle's summation order
follows its BLAS and thread count, and a hidden unit whose pre-activation is zero to rounding is then
decided one way here and the other way there (3.7e-4 .. 3e-2 of a gradient's maximum).  The checker
meets it as trajectory.RELU_LEVEL says, and test_undecided_relu_unit_is_resolved_and_a_decided_one_is_not
makes the case happen on every machine.  Then each fault of trajectory.FAULTS is planted and the checker must report
it: first at the step the fault first acts, and there under one of the checks named for it.  Run with
-s for the factor by which each fault fails."""
import functools

import numpy as np
import pytest

import numerics as nm
import trajectory as tj
from test_cpu_grad_targets import CASES, oracle_config

CLIP_ALWAYS = 0.05    # far below these models' gradient norm at initialisation (asserted: every step clips)


def _trainer(shape, fault=None, world=1, rank=0, clip=None, sched=None):
    name, _, tensor = (fault or "").partition(":")
    kw = {"stale": tensor} if tensor else {}
    return tj.OracleTrainer(oracle_config(shape), CASES[shape]["B"], world=world, rank=rank, clip=clip,
                            sched=tj.schedule if sched else None, fault=name or None, **kw)


def _report(mode, ck):
    for line in tj.summary(mode, ck):
        print(line)


def test_fma32_selection_equals_the_exhaustive_one():
    """numerics.fma32 fixes up only the elements whose float64 sum is a float32 midpoint; the result
    is the one of fixing up every inexact element -- on the edge state of the AdamW tests (subnormals,
    overflow) and on ties built by hand: 1 + 2^-24 + a product far below (the float64 sum is the
    midpoint itself; the exact value lies just above or below it)."""
    p, g, m, v = nm.adamw_edge_state()
    w1, b2, omb2 = np.float32(0.1), np.float32(0.999), np.float32(1 - 0.999)
    for a, b, c in ((w1, (g - m).astype(np.float32), m), ((omb2 * g).astype(np.float32), g, (v * b2).astype(np.float32)),
                    (p, g, m)):
        assert np.array_equal(nm.fma32(a, b, c).view(np.uint32), nm.fma32(a, b, c, every=True).view(np.uint32))
    # c = 1 + 2^-23 (odd last bit) and a b = +-2^-24 (1 - 2^-46): the exact sum lies 2^-70 inside the
    # midpoint 1 + 3 2^-24, float64 rounds it ONTO the midpoint, and ties-to-even from there would give
    # 1 + 2^-22 -- the exactly rounded result is c itself
    f = np.float32
    a = f([1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 1.0 + 2.0 ** -23])
    b = f([2.0 ** -24 * (1.0 - 2.0 ** -23), 2.0 ** -24 * (1.0 - 2.0 ** -23), 2.0 ** -24])
    c = f([1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 1.0])
    got = nm.fma32(a, b, c)
    assert np.array_equal(got.view(np.uint32), nm.fma32(a, b, c, every=True).view(np.uint32))
    assert got[0] == c[0] and got[1] == c[1] and got[2] == f(1.0 + 2.0 ** -23)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    assert naive[0] != got[0] and naive[1] != got[1]      # the cases are real: plain double rounding misses them


def test_undecided_relu_unit_is_resolved_and_a_decided_one_is_not():
    """The comment at trajectory.RELU_LEVEL, made to happen: at the first state of shape E the hidden unit
    whose fp64 pre-activation is nearest zero is decided the other way in the "product's" gradient.
    Against the oracle as it decided that misses the 1e-4 bar; the checker finds the unit among the
    undecided ones, meets the bar against the reference that decides it likewise, and says so in a
    relu-decision record.  The same with the unit FURTHEST from zero is a fault and stays one."""
    import torch
    tr = _trainer("E")
    ck = tj.Checker(tr, device="cpu")
    before = tr.snapshot()
    obs = tr.train_step()
    args = (before.master, obs.x, obs.y, tr.ocfg, tr.seed_base, before.counter)
    units, levels = tj.undecided_units(*args)
    z64 = tj._oracle_run(tj._params(before.master, torch.float64), *args[1:], backward=False)[2]
    layer = min(range(len(z64)), key=lambda l: float(z64[l].abs().min()))
    near = (layer, int(z64[layer].abs().reshape(-1).argmin()))
    far = (layer, int(z64[layer].abs().reshape(-1).argmax()))
    print(f"{len(units)} undecided units at levels {levels}; nearest zero {near}: z = {float(z64[layer].reshape(-1)[near[1]]):.3e}")
    assert near in units and far not in units and len(units) <= tj.MAX_UNDECIDED
    ref = tj.oracle_grads(*args)[1]

    def direct(got):
        return max(float(np.abs(got[n] - ref[n]).max() / np.abs(ref[n]).max()) for n in ref)
    got = tj.oracle_grads(*args, toggles=(near,))[1]
    print(f"decided the other way: {direct(got):.3e} of the gradient's maximum against the oracle as it decided")
    assert direct(got) > tj.FP32_GRAD
    errs = ck._fp32_errors("state 0", "grad", tr, before, obs, got, ref, torch.float32)
    assert max(errs.values()) < tj.FP32_GRAD
    notes = [r.name for r in ck.records if r.what == "relu-decision"]
    assert len(notes) == 1 and str(near[1]) in notes[0] and "decided the other way" in notes[0], notes
    bad = tj.oracle_grads(*args, toggles=(far,))[1]
    errs = ck._fp32_errors("state 0", "grad", tr, before, obs, bad, ref, torch.float32)
    print(f"a decided unit switched: {max(errs.values()):.3e}")
    assert max(errs.values()) > tj.FP32_GRAD and "no decision" in ck.records[-1].name


@functools.lru_cache(maxsize=None)
def _clean(shape, world=1, rank=0, clip=None, sched=False, fp64=False, tmp=None, data_seed=None):
    tr = _trainer(shape, None, world, rank, clip, sched)
    if data_seed is not None:
        tr.gen.manual_seed(data_seed)
    return tj.run_scenario(tr, tmp, fp64=fp64, device="cpu")


@pytest.mark.parametrize("recipe", [False, True], ids=["constant-lr", "clip-schedule"])
def test_unfaulted_stand_in_passes_and_the_oracle_is_stable(tmp_path, recipe):
    """Shape E with the GPU test's init seed, token stream and sampler seeds (trajectory.DATA_SEED; for
    the clip + schedule modes CLIP_DATA_SEED, max_norm 0.97 of the first norm, some steps clipping and
    some not): every check passes, and the fp32 oracle is within the fp32 bars of its own fp64 run at
    all 6 visited states (margin printed)."""
    kw = {}
    if recipe:
        first = _trainer("E", clip=1e30)
        first.gen.manual_seed(tj.CLIP_DATA_SEED)
        kw = dict(clip=tj.CLIP_OF_FIRST_NORM * first.train_step().norm, sched=True, data_seed=tj.CLIP_DATA_SEED)
    ck, tr = _clean("E", fp64=True, tmp=str(tmp_path / "ck.pt"), **kw)
    _report("cpu E-fp32" + ("-clip-schedule" if recipe else ""), ck)
    assert not ck.failures(), ck.failures()[:5]
    o64 = [r for r in ck.records if r.what == "oracle64"]
    names = len(ck.names)
    assert len(o64) == sum(tj.PLAN) * (names + 1)
    w = tj.worst(o64)
    print(f"fp32 oracle vs fp64 oracle over {sum(tj.PLAN)} states: worst {w.step} {w.name} {w.measured:.3e}, "
          f"bar {w.bound:.0e}: margin {w.bound / w.measured:.0f}x")
    assert tr.step == tr.counter - 1 == sum(tj.PLAN)     # 6 steps, 7 training-mode forwards
    if recipe:
        coefs = {r.name for r in ck.records if r.what == "coef"}
        assert coefs == {"clipping", "not clipping"}, coefs
    # every named parameter on every training step, under both the gradient and the AdamW check
    for k in range(sum(tj.PLAN)):
        for what, per in (("grad", 1), ("adamw", 3)):
            got = [r for r in ck.records if r.step == f"step {k}" and r.what == what]
            assert len(got) == per * names, (k, what, len(got))


@pytest.mark.parametrize("variant", ["O", "O-clip-schedule", "O-dp-rank0", "O-dp-rank1"])
def test_unfaulted_variants_pass(tmp_path, variant):
    """Shape O: plain; clipping on every step under the schedule; both ranks of a two-rank run."""
    kw = {"O": {}, "O-clip-schedule": dict(clip=CLIP_ALWAYS, sched=True), "O-dp-rank0": dict(world=2, rank=0),
          "O-dp-rank1": dict(world=2, rank=1)}[variant]
    ck, _ = _clean("O", tmp=str(tmp_path / "ck.pt"), **kw)
    _report("cpu " + variant, ck)
    assert not ck.failures(), ck.failures()[:5]
    if "clip" in variant:
        coefs = [r for r in ck.records if r.what == "coef"]
        assert len(coefs) == sum(tj.PLAN) and all(r.name == "clipping" for r in coefs)
        assert len({tj.schedule(k) for k in range(sum(tj.PLAN))}) == sum(tj.PLAN)


def test_data_parallel_replicas_agree(tmp_path):
    a, ta = _clean("O", world=2, rank=0, tmp=str(tmp_path / "a.pt"))
    b, tb = _clean("O", world=2, rank=1, tmp=str(tmp_path / "b.pt"))
    assert all(np.array_equal(ta.P[k], tb.P[k]) for k in ta.P)


@pytest.mark.parametrize("fault", sorted(tj.FAULTS))
def test_planted_fault_is_reported(tmp_path, fault):
    kw, where, whats = tj.FAULTS[fault]
    kw = dict(kw)
    if kw.pop("clip", False):
        kw["clip"] = CLIP_ALWAYS
    ck, _ = tj.run_scenario(_trainer("O", fault, **kw), str(tmp_path / "ck.pt"), device="cpu")
    bad = ck.failures()
    assert bad, f"no check reports the planted fault {fault}"
    first = bad[0].step
    here = [r for r in bad if r.step == first]
    by_what = {}
    for r in here:
        cur = by_what.get(r.what)
        factor = r.measured / r.bound if r.bound > 0 else float("inf")
        if cur is None or factor > cur[0]:
            by_what[r.what] = (factor, r)
    for what, (factor, r) in sorted(by_what.items()):
        f = "bitwise / exact" if factor == float("inf") else f"{factor:.3g}x its bound"
        print(f"[fault {fault}] first reported at {first!r} by {what}: {r.name}: {r.measured:.3e} vs {r.bound:.3e} ({f})")
    for what, (factor, r) in sorted(by_what.items()):
        if what == "grad" and r.measured < tj.BF16_FLOOR:
            print(f"[fault {fault}] the bf16 rule's floor {tj.BF16_FLOOR:.0e} would pass this gradient error ({r.measured:.2e}, "
                  f"here by max-norm): on a bf16 model the fault is left to {sorted(set(by_what) - {'grad', 'loss'})}")
        if what == "loss" and r.measured < tj.BF16_LOSS:
            print(f"[fault {fault}] the bf16 loss bar (1 % of ~4.2) would pass this loss error ({r.measured:.2e})")
    passed = sorted(set(whats) - set(by_what))
    if passed:
        print(f"[fault {fault}] NOT reported there by: {passed} (moves those by less than their bar)")
    assert first == where, (fault, first, where, bad[0])
    assert set(by_what) & set(whats), (fault, sorted(by_what), whats)
