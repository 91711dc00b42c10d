"""The instruments of tests/test_gpu_bf16_offpath.py on CPU tensors: the twin builder, the identity
the row-padded twins rest on (on the fp64 oracle, dropout on), and controls for the two comparators
of tests/twins.py -- fed the oracle's own results they pass, with planted faults they fail."""
import functools

import pytest
import torch
import torch.nn.functional as F

import twins as TW
from oracle import gpt1_oracle as O
from replicatinggpt_amd import GPTConfig

SEED = GPTConfig().dropout_seed


# ---------------------------------------------------------------------------------------
# the twin builder
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(TW.PAIRS))
def test_make_pair(pair):
    p = TW.PAIRS[pair]
    (ri, rt), (ti, tt) = TW.make_pair(pair)
    assert ri.shape == rt.shape == (p["B_r"], p["T"]) and ti.shape == tt.shape == (p["B_a"], p["T"])
    assert ri.dtype == rt.dtype == ti.dtype == tt.dtype == torch.int64
    assert torch.equal(ti[:p["B_r"]], ri) and torch.equal(tt[:p["B_r"]], rt)
    assert bool((tt[p["B_r"]:] == TW.IGNORE).all()) and not bool((rt == TW.IGNORE).any())
    V = TW.PAIR_MODEL["vocab_size"]
    assert 0 <= int(ti.min()) and int(ti.max()) < V and 0 <= int(rt.min()) and int(rt.max()) < V
    again = TW.make_pair(pair)
    assert all(torch.equal(a, b) for a, b in zip((ri, rt, ti, tt), (*again[0], *again[1])))
    # the token counts the pairs are about: the ragged one off a fast-path predicate, the twin on all of them
    n_r, n_a = p["B_r"] * p["T"], p["B_a"] * p["T"]
    assert n_a % 128 == 0 and n_r % 128 != 0
    assert (n_r % 64 == 0) == (pair in ("T1", "T2")) and (n_r % 16 == 0) == (pair != "T4")


def test_shapes_table():
    """The shapes with no twin, as the GPU file reads them; X3 is CASES["O"] itself."""
    for name, s in TW.SHAPES.items():
        bs = TW.shape_batches(name)
        assert len(bs) == len(s["T"])
        for (idx, tgt), T in zip(bs, s["T"]):
            assert idx.shape == tgt.shape == (s["B"], T) and T <= s["block_size"]
            assert int(idx.max()) < s["vocab_size"] and int(tgt.max()) < s["vocab_size"]
        assert s["n_embd"] % s["n_head"] == 0
    assert [tuple(i.shape) for i, _ in TW.shape_batches("X3")] == [(3, 37), (3, 29)]
    assert TW.SHAPES["X3"]["n_embd"] * 2 % 16 != 0   # bf16 rows of 252 bytes


# ---------------------------------------------------------------------------------------
# the identity, on the fp64 oracle
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle64(pair, which, unmask_filler=False):
    spec = TW.spec_of(pair)
    P = TW.oracle_params(spec, torch.float64)
    ragged, twin = TW.make_pair(pair)
    if which == "ragged":
        return TW.oracle_step(P, *ragged, TW.oracle_config(spec), SEED)
    idx, tgt = twin
    if unmask_filler:   # the fault "filler rows' targets not ignored"
        tgt = torch.where(tgt == TW.IGNORE, idx, tgt)
    return TW.oracle_step(P, idx, tgt, TW.oracle_config(spec), SEED, ignore_index=TW.IGNORE)


@pytest.mark.parametrize("pair", sorted(TW.PAIRS))
def test_twin_identity_fp64(pair):
    """Ragged batch and twin on the fp64 oracle with dropout 0.2: the same loss and logits, every
    gradient within 1e-12 of its maximum.  oracle_step is O.forward without targets followed by
    F.cross_entropy(..., ignore_index=-100); without ignore_index it is O.forward's own loss."""
    n = TW.PAIRS[pair]["B_r"] * TW.PAIRS[pair]["T"]
    zr, lr, gr = oracle64(pair, "ragged")
    zt, lt, gt = oracle64(pair, "twin")
    assert lr.dtype == torch.float64
    dl, dz = abs(float(lr) - float(lt)), float((zr - zt[:n]).abs().max())
    worst = max(float((gr[k] - gt[k]).abs().max() / gt[k].abs().max()) for k in gr)
    print(f"[{pair}] fp64 oracle, ragged vs twin: loss diff {dl:.1e}, logits diff {dz:.1e}, worst gradient diff "
          f"{worst:.1e} of the maximum")
    assert dl < 1e-13 and dz < 1e-12 and worst < 1e-12
    spec = TW.spec_of(pair)
    idx, tgt = TW.make_pair(pair)[0]
    z0, l0 = O.forward(TW.oracle_params(spec, torch.float64), idx, TW.oracle_config(spec), tgt, True, SEED, 0)
    assert torch.equal(z0, zr) and float(l0) == float(lr)
    # the twin's loss really is the mean over the valid tokens only
    ttgt = TW.make_pair(pair)[1][1].reshape(-1)
    rows = F.cross_entropy(zt, ttgt.clamp(min=0), reduction="none")
    assert abs(float(rows[ttgt != TW.IGNORE].mean()) - float(lt)) < 1e-13 and int((ttgt != TW.IGNORE).sum()) == n


# ---------------------------------------------------------------------------------------
# controls for the comparators
# ---------------------------------------------------------------------------------------
def _as_run(step):
    z, l, g = step
    return float(l), z, {k: v.clone() for k, v in g.items()}


def _twin_fails(got, ref, rows):
    return {r[0] for r in TW.twin_records(got, ref, rows) if not r[1]}


def _rule_fails(got, ref):
    # the oracle as its own bf16 reference: e_t = 0, so the floors of the rule are what is tested
    return {r[0] for r in TW.rule_records(got, ref, ref) if not r[5]}


@pytest.mark.parametrize("pair", ["T1", "T3"])
def test_comparators_pass_clean_and_catch_planted_faults(pair):
    p = TW.PAIRS[pair]
    T, n = p["T"], p["B_r"] * p["T"]
    ragged, twin = _as_run(oracle64(pair, "ragged")), _as_run(oracle64(pair, "twin"))
    assert _twin_fails(ragged, twin, n) == set()
    assert _rule_fails(ragged[2], twin[2]) == set()

    def planted(name, fn):
        g = {k: v.clone() for k, v in ragged[2].items()}
        g[name] = fn(g[name])
        return (ragged[0], ragged[1], g)

    def caught(name, fn, by_rule=True):
        bad = planted(name, fn)
        assert _twin_fails(bad, twin, n) == {name}, name
        if by_rule:
            assert _rule_fails(bad[2], twin[2]) == {name}, name

    # one parameter's gradient scaled by 1.03
    caught("blocks.1.ffwd.net.0.weight", lambda g: g * 1.03)
    # a gradient accumulated twice
    caught("blocks.0.sa_heads.proj.weight", lambda g: g + g)
    # one row's contribution missing from a bias gradient: lm_head.bias' is the column sum of
    # (softmax(logits) - onehot(target)) / n over the rows
    idx, tgt = TW.make_pair(pair)[0]
    row = n - 1
    contrib = (torch.softmax(ragged[1][row], dim=-1) - F.one_hot(tgt.reshape(-1)[row], ragged[1].shape[1])) / n
    full = ((torch.softmax(ragged[1], dim=-1) - F.one_hot(tgt.reshape(-1), ragged[1].shape[1])) / n).sum(0)
    assert torch.allclose(full, ragged[2]["lm_head.bias"], rtol=1e-9, atol=1e-12)   # the formula is the gradient
    caught("lm_head.bias", lambda g: g - contrib)
    # wpe rows past T left nonzero (a stale slot where the overwriting backward owes zeros)
    wpe = "position_embedding_table.weight"
    if T < TW.PAIR_MODEL["block_size"]:
        assert not bool(ragged[2][wpe][T:].any()) and not bool(twin[2][wpe][T:].any())

        def stale(g):
            g[T:] = g[:g.shape[0] - T]
            return g
        # (by norm the 16 stale rows of 64 are caught as well)
        caught(wpe, stale)
    # the filler rows' targets not ignored: every gradient and the loss move
    loose = _as_run(oracle64(pair, "twin", True))
    bad = _twin_fails(ragged, loose, n)
    print(f"[{pair}] filler targets not ignored: {len(bad)} of {len(ragged[2]) + 2} records fail")
    assert set(ragged[2]) <= bad
    assert _rule_fails(ragged[2], loose[2]) == set(ragged[2])
    # the logits rows and the loss gate on their own
    z = ragged[1].clone()
    z[n // 2] += 0.05 * float(z.abs().max())
    assert _twin_fails((ragged[0], z, ragged[2]), twin, n) == {"logits"}
    assert _twin_fails((ragged[0] * 1.011, ragged[1], ragged[2]), twin, n) == {"loss"}


def test_rule_is_relative_and_capped():
    """The rule follows the reference's own error with the 1.25 margin on both lines, keeps the project's
    2e-2 floor, and the cap on e_t is reported on its own."""
    gen = torch.Generator().manual_seed(0)
    ref = {"w": torch.randn(4096, generator=gen, dtype=torch.float64)}
    noise = torch.randn(4096, generator=gen, dtype=torch.float64)
    noise -= ref["w"] * (noise @ ref["w"]) / (ref["w"] @ ref["w"])   # orthogonal: 1 - cos = e^2 / 2 to first order
    noise *= ref["w"].norm() / noise.norm()

    def at(e):
        return {"w": ref["w"] + e * noise}
    ok = lambda e_c, e_t: TW.rule_records(at(e_c), ref, at(e_t))[0][5]   # noqa: E731
    assert ok(1.9e-2, 0.0) and not ok(2.1e-2, 0.0)
    assert ok(1.2 * 4.5e-2, 4.5e-2) and not ok(1.3 * 4.5e-2, 4.5e-2)
    # the cosine line on its own: a gradient of the right direction error but shrunk by 4 % passes the
    # cosine and fails the norm; one turned by 6e-2 and rescaled onto the reference's norm error fails the cosine
    shrunk = TW.rule_records({"w": 0.96 * ref["w"]}, ref, at(1e-2))[0]
    assert shrunk[3] > 1 - 1e-12 and not shrunk[5]
    turned = ref["w"] + 6e-2 * noise
    turned = {"w": turned * (ref["w"] @ turned) / (turned @ turned)}   # the closest point of that direction
    r = TW.rule_records(turned, ref, at(4.5e-2))[0]
    assert r[1] < 1.25 * 6e-2 and 1 - r[3] > 1.5625 * (1 - r[4]) and not r[5]
    _, capped = TW.rule_report("control", TW.rule_records(at(5e-2), ref, at(6.5e-2)))
    assert [c[0] for c in capped] == ["w"]
    _, capped = TW.rule_report("control", TW.rule_records(at(5e-2), ref, at(5.9e-2)))
    assert capped == []
