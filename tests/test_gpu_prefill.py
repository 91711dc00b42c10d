"""The one-pass prompt prefill on the MI355X (decode.py _prefill_pass, csrc/decode.hip
k_decode_prefill_attn / k_decode_logprob_rows).

The bar is bitwise: a prefill by one pass leaves the K/V caches, the tokens and the log-probabilities that
a prefill by per-token steps leaves, so every comparison between the two is torch.equal.  Against the fp64
oracle the bounds are the ones the per-token engine is held to (test_gpu_model.py, test_gpu_complete.py)."""
import ctypes

import pytest
import torch

from footprint import Box
from test_gpu_complete import (FP32_BAR, LOGPROB_ABS, PAD, V, case, check_rows_against, make_model, oracle_stream,
                               teacher_logprobs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------
# 1. the attention kernel
# ---------------------------------------------------------------------------------------
ATTN_CASES = [(3, 2, 24, 1, 16), (2, 4, 8, 63, 70), (2, 2, 32, 64, 64), (2, 3, 21, 65, 80), (1, 1, 64, 130, 130)]


def _attn_boxes(B, H, D, P, Tmax, seed):
    """q in a box of its own and k | v side by side in another (two row strides, both padded), the caches
    dense [B, H, Tmax, D] between guards and full of a sentinel, o poisoned."""
    g = torch.Generator().manual_seed(seed)
    HD = H * D
    qb = Box(B * P, HD, torch.float32, ld=HD + 3, device=DEV).fill(torch.randn(B * P, HD, generator=g)).snapshot()
    kvb = Box(B * P, 2 * HD, torch.float32, ld=2 * HD + 5, device=DEV).fill(torch.randn(B * P, 2 * HD, generator=g))
    kvb.snapshot()
    ob = Box(B * P, HD, torch.float32, ld=HD + 2, device=DEV)
    kcb = Box(B * H * Tmax, D, torch.float32, device=DEV).fill(torch.full((B * H * Tmax, D), SENTINEL))
    vcb = Box(B * H * Tmax, D, torch.float32, device=DEV).fill(torch.full((B * H * Tmax, D), SENTINEL))
    return qb, kvb, ob, kcb, vcb


def _check_caches(kcb, vcb, kvb, B, H, D, P, Tmax):
    HD = H * D
    kc, vc = kcb.view.view(B, H, Tmax, D), vcb.view.view(B, H, Tmax, D)
    for cache, box, cols, name in ((kc, kcb, kvb.view[:, :HD], "k"), (vc, vcb, kvb.view[:, HD:], "v")):
        want = cols.reshape(B, P, H, D).permute(0, 2, 1, 3)
        assert torch.equal(cache[:, :, :P], want), f"{name} cache rows < P are not the {name} columns"
        assert bool((cache[:, :, P:] == SENTINEL).all()), f"{name} cache rows >= P were written"
        box.assert_clean(f"{name}cache")


@pytest.mark.parametrize("B,H,D,P,Tmax", ATTN_CASES)
def test_prefill_attn_is_decode_attn_per_position(B, H, D, P, Tmax):
    """o[b P + t] is ops.decode_attn's output for nkeys = t + 1 on the cache the call wrote, bit for bit, and
    within the 1e-5 relative bar of an fp64 causal softmax; the cache rows < P are the K / V columns, rows
    >= P, the operands and every guard band are untouched; the q = o = None form writes the same caches."""
    from replicatinggpt_amd import ops
    HD = H * D
    scale = float(HD) ** -0.5
    qb, kvb, ob, kcb, vcb = _attn_boxes(B, H, D, P, Tmax, 100 * P + D)
    q, k, v = qb.view, kvb.view[:, :HD], kvb.view[:, HD:]
    kc, vc = kcb.view.view(B, H, Tmax, D), vcb.view.view(B, H, Tmax, D)
    ops.decode_prefill_attn(q, k, v, P, scale, kc, vc, ob.view)
    torch.cuda.synchronize()
    qb.assert_unchanged("q")
    kvb.assert_unchanged("kv")
    ob.assert_clean("o")
    _check_caches(kcb, vcb, kvb, B, H, D, P, Tmax)
    got = ob.view.reshape(B, P, HD)
    assert not bool(torch.isnan(got).any()), "an element of o was not written"
    # per position: the decode kernel on that cache, its query rows b P + t read in place
    want = torch.empty_like(got)
    for t in range(P):
        o_t = torch.empty((B, HD), device=DEV)
        ops.decode_attn(q[t:], P * q.stride(0), kc, 0, vc, 0, H * Tmax * D, Tmax * D, D, B, H, D, None, t + 1, scale, o_t)
        want[:, t] = o_t
    torch.cuda.synchronize()
    diff = (_bits(got) != _bits(want)).nonzero()
    assert diff.numel() == 0, f"{diff.shape[0]} element(s) differ from decode_attn, first (b, t, c) = {diff[0].tolist()}"
    # fp64 causal softmax
    q64 = q.double().reshape(B, P, H, D).permute(0, 2, 1, 3)
    k64 = k.double().reshape(B, P, H, D).permute(0, 2, 1, 3)
    v64 = v.double().reshape(B, P, H, D).permute(0, 2, 1, 3)
    s = (q64 @ k64.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(P, P, device=DEV).triu(1).bool(), float("-inf"))
    ref = (torch.softmax(s, -1) @ v64).permute(0, 2, 1, 3).reshape(B, P, HD)
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"prefill attn {(B, H, D, P, Tmax)}: relative error {err:.3e} against fp64 (bar 1e-5)")
    assert err < 1e-5
    # the cache-write-only form
    _, _, _, kcb2, vcb2 = _attn_boxes(B, H, D, P, Tmax, 1)
    ops.decode_prefill_attn(None, k, v, P, scale, kcb2.view.view(B, H, Tmax, D), vcb2.view.view(B, H, Tmax, D), None)
    torch.cuda.synchronize()
    _check_caches(kcb2, vcb2, kvb, B, H, D, P, Tmax)
    assert torch.equal(kcb2.view, kcb.view) and torch.equal(vcb2.view, vcb.view)


def test_prefill_attn_rejects_bad_arguments_and_opcheck():
    """D > 64, P < 1, P > Tmax, a pointer off a 4-byte boundary, q without o and o without q: CG_EINVAL with
    a message that names the argument, nothing launched.  opcheck on both forms."""
    from replicatinggpt_amd import _lib as L, ops
    lib = L.load()
    B, H, D, P, Tmax = 2, 2, 8, 5, 9
    HD = H * D
    qkv = torch.randn(B * P, 3 * HD, device=DEV)
    kc = torch.full((B, H, Tmax, D), SENTINEL, device=DEV)
    vc = torch.full((B, H, Tmax, D), SENTINEL, device=DEV)
    o = torch.full((B * P, HD), SENTINEL, device=DEV)
    st = L.stream_ptr(qkv.device)

    def call(q=qkv.data_ptr(), k=qkv.data_ptr() + 4 * HD, o_=o.data_ptr(), D_=D, P_=P, Tmax_=Tmax):
        p = lambda a: None if a is None else ctypes.c_void_p(a)   # noqa: E731
        rc = lib.cg_decode_prefill_attn(p(q), 3 * HD, p(k), p(qkv.data_ptr() + 8 * HD), 3 * HD, B, P_, H, D_, Tmax_, 0.25,
                                        p(kc.data_ptr()), p(vc.data_ptr()), p(o_), HD, st)
        L.check(rc, "decode_prefill_attn")

    for kw, msg in ((dict(D_=65), "D = 65"), (dict(P_=0), "P = 0"), (dict(P_=Tmax + 1), f"P = {Tmax + 1}"),
                    (dict(k=qkv.data_ptr() + 4 * HD + 2), "4-B aligned"), (dict(q=qkv.data_ptr() + 1), "4-B aligned"),
                    (dict(o_=None), "both"), (dict(q=None), "both")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    with pytest.raises(ValueError, match="both"):
        ops.decode_prefill_attn(qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:], P, 0.25, kc, vc, None)
    with pytest.raises(RuntimeError, match="D = 65"):
        wide = torch.zeros(3, 65, device=DEV)
        big = torch.zeros(1, 1, 4, 65, device=DEV)
        ops.decode_prefill_attn(None, wide, wide, 3, 0.25, big, big.clone(), None)
    torch.cuda.synchronize()
    for t in (kc, vc, o):
        assert bool((t == SENTINEL).all()), "a refused call wrote something"
    call()                                                      # the same arguments, valid: runs
    torch.cuda.synchronize()
    assert torch.equal(kc[:, :, :P], qkv[:, HD:2 * HD].reshape(B, P, H, D).permute(0, 2, 1, 3))
    q2, k2, v2 = (qkv[:, i * HD:(i + 1) * HD].contiguous() for i in range(3))
    torch.library.opcheck(ops.decode_prefill_attn, (q2, k2, v2, P, 0.25, kc, vc, o))
    torch.library.opcheck(ops.decode_prefill_attn, (None, k2, v2, P, 0.25, kc, vc, None))


# ---------------------------------------------------------------------------------------
# 2. the log-prob rows
# ---------------------------------------------------------------------------------------
def _i64(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("Vn", [1, 65, 200])
def test_logprob_rows_are_decode_emit_columns(Vn):
    """logprob[b, t + 1] from one launch over the B P logits rows against ops.decode_emit run column by
    column on the same rows as forced tokens: the same bits -- NaN for the row holding NaN, the row holding
    +inf and the two tokens outside [0, V) included.  Only columns 1..P are written."""
    from replicatinggpt_amd import ops
    B, P, width = 3, 7, 10
    g = torch.Generator().manual_seed(7 * Vn)
    x = torch.rand(B * P, Vn, generator=g) * 40 - 20
    x[4, Vn // 2] = float("nan")
    x[9, Vn - 1] = float("inf")
    tok = torch.randint(0, Vn, (B, width), generator=g)
    tok[0, 3], tok[2, 6] = Vn + 5, -4                      # columns 3 and 6: scored by rows (0, 2) and (2, 5)
    lb = Box(B * P, Vn, torch.float32, ld=Vn + 3, device=DEV).fill(x).snapshot()
    ib = Box(B, width, torch.int64, ld=width + 2, device=DEV, pad=0).fill(tok).snapshot()
    pb = Box(B, width, torch.float32, ld=width + 5, device=DEV).fill(torch.full((B, width), -3.0))
    ops.decode_logprob_rows(lb.view, P, ib.view, pb.view)
    torch.cuda.synchronize()
    lb.assert_unchanged("logits")
    ib.assert_unchanged("idx")
    pb.assert_clean("logprob")
    got = pb.view.cpu()
    assert bool((got[:, 0] == -3.0).all()) and bool((got[:, P + 1:] == -3.0).all()), "a column outside 1..P was written"
    # cg_decode_emit, one forced column per launch, on the same logits rows read in place
    idx = tok.to(DEV)
    want = torch.full((B, width), -3.0, device=DEV)
    plen = torch.full((B,), width, dtype=torch.int64, device=DEV)
    end = torch.zeros(B, dtype=torch.int64, device=DEV)
    words = torch.zeros((Vn + 63) // 64, dtype=torch.int64, device=DEV)
    rows = lb.view.as_strided((B, P, Vn), (P * lb.ld, lb.ld, 1))
    for t in range(P):
        ops.decode_emit(rows[:, t], 0, None, _i64(1), _i64(t + 1), plen, plen + 4, end, words, _i64(PAD), idx, want)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), tok) and end.tolist() == [0] * B
    want = want.cpu()
    assert torch.equal(_bits(got), _bits(want)), (got, want)
    nan = torch.isnan(got)
    expect_nan = torch.zeros_like(nan)
    expect_nan[0, 3] = expect_nan[2, 6] = True             # the tokens outside the vocabulary
    expect_nan[4 // P, 4 % P + 1] = expect_nan[9 // P, 9 % P + 1] = True   # the NaN row, the +inf row
    assert torch.equal(nan, expect_nan)
    fine = ~nan
    fine[:, 0] = False
    fine[:, P + 1:] = False
    ref = torch.log_softmax(x.double(), dim=-1).reshape(B, P, Vn)
    ref = ref.gather(2, tok[:, 1:P + 1].clamp(0, Vn - 1)[:, :, None])[:, :, 0]
    err = (got[:, 1:P + 1].double() - ref)[fine[:, 1:P + 1]].abs().max()
    assert float(err) <= LOGPROB_ABS
    from replicatinggpt_amd import _lib as L
    with pytest.raises(RuntimeError, match="stride_logits"):
        L.check(L.load().cg_decode_logprob_rows(L.ptr(lb.view), Vn - 1, Vn, B, P, L.ptr(ib.view), ib.ld, L.ptr(pb.view),
                                                pb.ld, L.stream_ptr(idx.device)), "decode_logprob_rows")
    if Vn == 65:
        torch.library.opcheck(ops.decode_logprob_rows, (lb.view, P, ib.view, pb.view))


# ---------------------------------------------------------------------------------------
# 3. the engine: one pass against per-token steps, bit for bit
# ---------------------------------------------------------------------------------------
# name: (T, C, H, L), prompt lengths (ragged, shortest >= 3), new tokens (the longest rows end in the window phase)
MODELS = {
    "T64": ((64, 96, 4, 3), (7, 19, 33, 41), 30),
    "T128": ((128, 128, 2, 2), (70, 90, 101, 128), 6),
    "D21": ((48, 126, 6, 2), (5, 17, 30, 47), 8),          # the model.pth shape's head size
    "K192": ((32, 192, 3, 2), (3, 12, 20, 32), 5),         # K > 128: the LayerNorm launch + GEMM route
}
_MODEL = {}
SAMPLING = (0.8, 20, 0.9)


def model(name):
    if name not in _MODEL:
        (T, C, H, L), lens, new = MODELS[name]
        m = make_model(T, C, H, L, 40 + len(_MODEL)).eval()
        idx = torch.randint(0, V, (len(lens), max(lens)), generator=torch.Generator().manual_seed(T + C)).to(DEV)
        _MODEL[name] = (m, idx, torch.tensor(lens), new)
    return _MODEL[name]


def engines(m, B, width, **kw):
    from replicatinggpt_amd.decode import DecodeEngine
    return (DecodeEngine(m, B, width, prefill_pass=True, prefill_min=1, **kw),
            DecodeEngine(m, B, width, prefill_pass=False, **kw))


@pytest.mark.parametrize("name", list(MODELS))
def test_pass_leaves_the_caches_of_per_token_steps(name):
    """Straight after the prefill: kc / vc [..., :Pn, :] of every layer and len, from one _prefill_pass and
    from Pn phase-1 steps; with and without the scoring head (the last layer in full / K and V only)."""
    m, idx, lens, new = model(name)
    B, Pn = idx.shape[0], int(lens.min()) - 1
    with torch.no_grad():
        for score in (False, True):
            one, per = engines(m, B, idx.shape[1] + 1, ragged=True, logprobs=score, use_graph=False)
            for eng in (one, per):
                eng.idx[:, :idx.shape[1]].copy_(idx)
                eng.kc.fill_(SENTINEL)
                eng.vc.fill_(SENTINEL)
            one._prefill_pass(Pn, score)
            per.len.fill_(1)
            for _ in range(Pn):
                per._step1(False)
            torch.cuda.synchronize()
            assert torch.equal(one.len, per.len) and int(one.len) == Pn + 1
            for l in range(one.L):
                for a, b, nm in ((one.kc, per.kc, "k"), (one.vc, per.vc, "v")):
                    d = (_bits(a[l, :, :, :Pn]) != _bits(b[l, :, :, :Pn])).nonzero()
                    assert d.numel() == 0, (f"{name} score={score}: layer {l} {nm} cache differs in {d.shape[0]} "
                                            f"element(s), first (b, h, t, e) = {d[0].tolist()}")
                    assert bool((a[l, :, :, Pn:] == SENTINEL).all()), "the pass wrote a cache row >= Pn"


@pytest.mark.parametrize("logprobs", [False, True])
@pytest.mark.parametrize("name", list(MODELS))
def test_complete_with_pass_equals_complete_with_steps(name, logprobs):
    """Ragged complete() on two engines, greedy, sampled and filtered: tokens, lengths, log-probs and steps
    equal; the pass engine ran one pass over the planned positions and, without log-probs, no prefill step."""
    from replicatinggpt_amd.decode import prefill_plan
    m, idx, lens, new = model(name)
    B, pmin, T = idx.shape[0], int(lens.min()), m.config.block_size
    one, per = engines(m, B, idx.shape[1] + new, ragged=True, logprobs=logprobs)
    Pn = prefill_plan(pmin, T, logprobs, 1)
    assert Pn == (pmin - 2 if logprobs else pmin - 1) and Pn >= 1
    for mode, sampling in ((0, None), (1, None), (2, SAMPLING)):
        out = [eng.complete(idx, lens, new, mode=mode, seed=1234 + mode, sampling=sampling, pad=PAD) for eng in (one, per)]
        torch.cuda.synchronize()
        (tok1, len1, lp1, steps1), (tok0, len0, lp0, steps0) = out
        assert torch.equal(tok1, tok0), f"{name} mode {mode}: tokens differ"
        assert torch.equal(len1, len0) and steps1 == steps0
        assert len1.tolist() == (lens + new).tolist()
        if logprobs:
            assert torch.equal(_bits(lp1), _bits(lp0)), f"{name} mode {mode}: log-probs differ"
            assert steps1 == int(lens.max()) + new - 1 and bool((lp1[:, 1:pmin] < 0).all())
        else:
            assert lp1 is None and steps1 == int(lens.max()) + new - pmin
        assert one.prefill_stats == {"passes": 1, "positions": Pn, "step_replays": 0}
        assert per.prefill_stats == {"passes": 0, "positions": 0, "step_replays": 0 if logprobs else pmin - 1}
    assert one.g1_prefill is not None, "the prefill step graph is still captured"


@pytest.mark.parametrize("name", list(MODELS))
def test_generate_with_pass_equals_generate_with_steps(name):
    """generate() from a 40-token prompt, greedy and sampled: the pass covers 39 positions where the prompt
    fits the window (a longer prompt starts in the window phase: no pass)."""
    m, _, _, _ = model(name)
    T, B, L0, new = m.config.block_size, 3, 40, 6
    idx = torch.randint(0, V, (B, L0), generator=torch.Generator().manual_seed(T)).to(DEV)
    for greedy in (True, False):
        one, per = engines(m, B, L0 + new, greedy=greedy)
        a, b = one.generate(idx, new, seed=99), per.generate(idx, new, seed=99)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a[:, :L0], idx)
        fits = L0 <= T
        assert one.prefill_stats == {"passes": int(fits), "positions": 39 * fits, "step_replays": 0}
        assert per.prefill_stats == {"passes": 0, "positions": 0, "step_replays": 39 * fits}


def test_pass_without_graphs():
    """The T64 run on engines built with use_graph=False."""
    m, idx, lens, new = model("T64")
    one, per = engines(m, idx.shape[0], idx.shape[1] + new, ragged=True, logprobs=True, use_graph=False)
    a, b = (eng.complete(idx, lens, new, mode=1, seed=5, pad=PAD) for eng in (one, per))
    torch.cuda.synchronize()
    assert one.g1_prefill is None and not one.rg and one.prefill_stats["passes"] == 1
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2])) and a[3] == b[3]


# ---------------------------------------------------------------------------------------
# 4. a row does not depend on its batch-mates
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_long_prompt_row_alone_and_beside_shorter_rows(mode):
    """Row 0 (41 tokens) alone: the pass covers 39 of its positions.  Beside rows of 7 and 19 tokens it
    covers 5 and steps do the rest.  Tokens and log-probs of row 0 are equal."""
    from replicatinggpt_amd.decode import DecodeEngine
    m, idx, lens, new = model("T64")
    row = idx[3:4, :41]
    alone = DecodeEngine(m, 1, 41 + new, ragged=True, logprobs=True, prefill_pass=True, prefill_min=1)
    t1, l1, lp1, _ = alone.complete(row, torch.tensor([41]), new, mode=mode, seed=77, pad=PAD)
    assert alone.prefill_stats["positions"] == 39
    three = torch.cat([row, idx[0:1, :41], idx[1:2, :41]])
    mates = DecodeEngine(m, 3, 41 + new, ragged=True, logprobs=True, prefill_pass=True, prefill_min=1)
    t3, l3, lp3, _ = mates.complete(three, torch.tensor([41, 7, 19]), new, mode=mode, seed=77, pad=PAD)
    torch.cuda.synchronize()
    assert mates.prefill_stats["positions"] == 5
    assert torch.equal(t3[0], t1[0]) and int(l3[0]) == int(l1[0]) == 41 + new
    assert torch.equal(_bits(lp3[0]), _bits(lp1[0]))


# ---------------------------------------------------------------------------------------
# 5. the oracle
# ---------------------------------------------------------------------------------------
def test_pass_then_greedy_matches_oracle_per_row():
    """Prompts (100, 120, 128) at T = 128 (test_gpu_complete.py's R2): the pass covers 99 positions and every
    row is the oracle's greedy stream of that row run alone."""
    from replicatinggpt_amd.completion import Completion, pack_prompts
    from replicatinggpt_amd.decode import DecodeEngine
    m, par, ocfg, prompts, P, new = case("R2")
    streams = [oracle_stream("R2", b) for b in range(len(P))]
    idx, lens = pack_prompts(prompts)
    eng = DecodeEngine(m, len(P), max(P) + new, ragged=True, prefill_pass=True, prefill_min=1)
    out = eng.complete(idx.to(DEV), lens, new, mode=0, pad=PAD)
    torch.cuda.synchronize()
    assert eng.prefill_stats == {"passes": 1, "positions": 99, "step_replays": 0}
    check_rows_against(Completion(*out), streams, P, new)


def test_scored_rows_longer_than_the_window_match_oracle():
    """score() of three rows of T + 3 = 67 tokens at T = 64: columns 1..T-1 from the pass, column T from a
    phase-1 step, the rest from the window phase, each within 2 * 1e-5 * max|logit| + 1e-4 of the fp64
    teacher-forced oracle (test_logprobs_match_oracle_and_score_changes_no_token's bound)."""
    from replicatinggpt_amd.decode import DecodeEngine
    m, par, ocfg, _, _, _ = case("R1")
    T, n = ocfg.block_size, ocfg.block_size + 3
    rows = torch.randint(0, V, (3, n), generator=torch.Generator().manual_seed(5))
    eng = DecodeEngine(m, 3, n, ragged=True, logprobs=True, prefill_pass=True, prefill_min=1)
    tokens, lengths, lp, steps = eng.complete(rows.to(DEV), torch.full((3,), n), 0, mode=0, pad=PAD)
    torch.cuda.synchronize()
    assert eng.prefill_stats == {"passes": 1, "positions": T - 1, "step_replays": 0}
    assert steps == n - 1 and lengths.tolist() == [n] * 3 and torch.equal(tokens.cpu(), rows)
    lp = lp.cpu()
    for b in range(3):
        ref, amax = teacher_logprobs(par, ocfg, rows[b], n)
        bound = 2 * FP32_BAR * amax + LOGPROB_ABS
        err = (lp[b].double() - ref).abs()
        print(f"row {b}: score error {float(err.max()):.3e} (pass columns {float(err[1:T].max()):.3e}), bound {bound:.3e}")
        assert float(err.max()) <= bound, (b, float(err.max()), bound)
        assert float(lp[b, 0]) == 0.0 and bool((lp[b, 1:] < 0).all())


# ---------------------------------------------------------------------------------------
# 6. no pass where it must not run
# ---------------------------------------------------------------------------------------
def test_no_pass_for_one_token_prompts_and_prompts_past_the_window():
    from replicatinggpt_amd.decode import DecodeEngine
    m, idx, lens, new = model("T64")
    T = m.config.block_size
    for logprobs in (False, True):
        eng = DecodeEngine(m, 2, 30, ragged=True, logprobs=logprobs, prefill_pass=True, prefill_min=1)
        eng.complete(idx[:2, :20], torch.tensor([1, 20]), 4, mode=0, pad=PAD)                 # pmin = 1
        assert eng.prefill_stats == {"passes": 0, "positions": 0, "step_replays": 0}
    long = torch.randint(0, V, (2, T + 6), generator=torch.Generator().manual_seed(3)).to(DEV)
    eng = DecodeEngine(m, 2, T + 10, ragged=True, prefill_pass=True, prefill_min=1)
    eng.complete(long, torch.tensor([T + 1, T + 6]), 4, mode=0, pad=PAD)                      # pmin > T: phase 2 only
    torch.cuda.synchronize()
    assert eng.prefill_stats == {"passes": 0, "positions": 0, "step_replays": 0}
    eng = DecodeEngine(m, 2, 30, ragged=True, prefill_pass=True, prefill_min=25)              # below prefill_min
    eng.complete(idx[:2, :20], torch.tensor([20, 20]), 4, mode=0, pad=PAD)
    assert eng.prefill_stats == {"passes": 0, "positions": 0, "step_replays": 19}


def test_bf16_engine_keeps_the_per_token_prefill(monkeypatch):
    """A bf16 engine asked for the pass runs none, and its tokens are those of a run with the pass switched
    off globally (CHARPT_PREFILL_PASS=0's module flag)."""
    from replicatinggpt_amd import decode
    m = make_model(64, 128, 2, 2, 61, "bf16").eval()
    idx = torch.randint(0, V, (3, 30), generator=torch.Generator().manual_seed(8)).to(DEV)
    lens = torch.tensor([9, 21, 30])
    eng = decode.DecodeEngine(m, 3, 40, ragged=True, prefill_pass=True, prefill_min=1)
    a = eng.complete(idx, lens, 10, mode=0, pad=PAD)
    assert not eng.prefill_pass and eng.prefill_stats == {"passes": 0, "positions": 0, "step_replays": 8}
    monkeypatch.setattr(decode, "PREFILL_PASS", False)
    off = decode.DecodeEngine(m, 3, 40, ragged=True)
    b = off.complete(idx, lens, 10, mode=0, pad=PAD)
    torch.cuda.synchronize()
    assert not off.prefill_pass and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_pass_is_on_by_default_and_the_switch_turns_it_off(monkeypatch):
    from replicatinggpt_amd import decode
    m, idx, lens, new = model("T64")
    eng = decode.DecodeEngine(m, 4, 60, ragged=True)
    assert decode.PREFILL_PASS and eng.prefill_pass and eng.prefill_min == decode.PREFILL_MIN
    monkeypatch.setattr(decode, "PREFILL_PASS", False)
    assert not decode.DecodeEngine(m, 4, 60, ragged=True).prefill_pass
    assert decode.DecodeEngine(m, 4, 60, ragged=True, prefill_pass=True).prefill_pass
