"""cg_gemm_wgrad_group on the MI355X: several split-K weight gradients (dW = dy^T x, GPT1.py:111-112,136
backward) as one launch of the 128x128 persistent kernel.  Each problem's output must have the bits of
its own cg_gemm call at the same split and flags -- across problem boundaries in a block's item
sequence, with fp32 and bf16 slabs, the reduce in line or deferred, beta 0 and 1 -- and the training
step with functional.WGRAD_GROUP on must match the step with it off."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIDE_MIN = 64   # csrc/gemm_common.h: free slots from which a launch runs pending work beside its items


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from replicatinggpt_amd import _lib as L
    L.load()
    yield


def ops():
    from replicatinggpt_amd import ops as O
    return O


def L():
    from replicatinggpt_amd import _lib
    return _lib


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _ws(M, N, split):
    return torch.empty(ops().gemm_workspace(M, N, split) // 4, dtype=torch.float32, device=DEV)


def _flush():
    """A following small persistent GEMM (takes pending reduces in its tail), then the flush."""
    x = torch.randn(256, 128, device=DEV).to(torch.bfloat16)
    y = torch.empty(256, 128, dtype=torch.bfloat16, device=DEV)
    ops().gemm(x, x[:128], y, True, False, False, 256, 128, 128, 128, 128, 128, 0, None, None, 0, None, 0, 0.0, 0,
               None, 0, 0.0, 1, None)
    L().check(L().load().cg_flush_deferred(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _single(A, B, init, beta, split, flags):
    """out (+)= A^T B through cg_gemm: A [K, M] and B [K, N] (views with their own row strides).  Returns
    out and the workspace, which a deferred reduce still reads until the flush."""
    K, M = A.shape
    N = B.shape[1]
    out, ws = init.clone(), _ws(M, N, split)
    ops().gemm(A, B, out, True, True, True, M, N, K, A.stride(0), B.stride(0), N, 0, None, None, 0, None, 0, 0.0, 0,
               None, 0, float(beta), split, ws, flags)
    return out, ws


def _flags(bf16, defer):
    return (L().GEMM_SLAB_BF16 if bf16 else 0) | (L().GEMM_DEFER_REDUCE if defer else 0)


def _unequal_pair():
    """K = 1024 tokens (16 K-tiles): 128x128 at split 3 (6, 6, 4 K-tiles) and 384x128 at split 2, the
    operands column slices of wider buffers -- four different leading dimensions, none a width."""
    torch.manual_seed(11)
    K = 1024
    wa0 = (torch.randn(K, 200, device=DEV) * 0.5).to(torch.bfloat16)
    wa1 = (torch.randn(K, 456, device=DEV) * 0.5).to(torch.bfloat16)
    wb = (torch.randn(K, 264, device=DEV) * 0.5).to(torch.bfloat16)
    wb1 = (torch.randn(K, 328, device=DEV) * 0.5).to(torch.bfloat16)
    probs = [(wa0[:, 8:136], wb[:, 16:144], 3), (wa1[:, 8:392], wb1[:, 136:264], 2)]
    inits = [torch.randn(A.shape[1], B.shape[1], device=DEV) for A, B, _ in probs]
    return probs, inits


_REF = {}


def _unequal_reference(bf16, defer, beta):
    """The two cg_gemm calls' outputs, computed once per flag combination and left unchanged."""
    key = (bf16, defer, beta)
    if key not in _REF:
        probs, inits = _unequal_pair()
        want = []
        for (A, B, split), init in zip(probs, inits):
            out, ws = _single(A, B, init, beta, split, _flags(bf16, defer))
            if defer:
                _flush()
            want.append(out)
        torch.cuda.synchronize()
        _REF[key] = want
    return _REF[key]


def _group(probs, inits, beta, flags):
    outs = [i.clone() for i in inits]
    dys, xs, splits = [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs]
    wss = [_ws(A.shape[1], B.shape[1], s) for A, B, s in probs]
    betas = [float(beta)] * len(probs)
    assert ops().gemm_wgrad_group_supported(dys, xs, outs, wss, betas, splits, flags)
    ops().gemm_wgrad_group(dys, xs, outs, wss, betas, splits, flags)
    return outs, wss


@pytest.mark.parametrize("mode", ["slots", "grid5", "side"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
def test_group_unequal_problems_bitwise(bf16, defer, beta, mode):
    """Two problems unequal in shape, split and leading dimensions: each output equals its own cg_gemm.
    grid5: five blocks take the nine items, so blocks cross the problem boundary with the DMA cursor
    and with the compute cursor.  side: a reduce is pending when the group is launched and the launch
    has just SIDE_MIN blocks beyond its items, which run that reduce beside the items."""
    lib = L().load()
    want = _unequal_reference(bf16, defer, beta)
    probs, inits = _unequal_pair()
    flags = _flags(bf16, defer)
    nitems = sum((A.shape[1] // 128) * (B.shape[1] // 128) * s for A, B, s in probs)
    assert nitems == 9
    pend = None
    try:
        if mode == "grid5":
            L().check(lib.cg_set_tuning(b"gemm_max_grid", 5))
        if mode == "side":
            # an earlier weight gradient leaves its reduce pending; the group's side blocks sum it
            A, B, split = probs[1]
            pend_want = _unequal_reference(True, True, 0.0)[1]
            pend_out = torch.full_like(pend_want, float("nan"))
            pend_ws = _ws(A.shape[1], B.shape[1], split)
            ops().gemm(A, B, pend_out, True, True, True, A.shape[1], B.shape[1], A.shape[0], A.stride(0), B.stride(0),
                       B.shape[1], 0, None, None, 0, None, 0, 0.0, 0, None, 0, 0.0, split, pend_ws, _flags(True, True))
            pend = (pend_out, pend_want, pend_ws)
            L().check(lib.cg_set_tuning(b"gemm_max_grid", nitems + SIDE_MIN))
        outs, wss = _group(probs, inits, beta, flags)
    finally:
        L().check(lib.cg_set_tuning(b"gemm_max_grid", 0))
    if defer:
        _flush()
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert not torch.isnan(o).any()
        assert torch.equal(o, w)
    if pend is not None:
        assert torch.equal(pend[0], pend[1])


@pytest.mark.parametrize("bf16", [False, True])
def test_group_of_one_and_fp64(bf16):
    """A one-problem group equals cg_gemm bit for bit; and the pair against the fp64 product: 1e-5
    relative with fp32 slabs, 2^-8 with bf16 slabs (each split's partial rounded once to bf16, 2^-9) --
    the bounds tests/test_gpu_ops.py holds the same paths to."""
    probs, inits = _unequal_pair()
    flags = _flags(bf16, False)
    want = _unequal_reference(bf16, False, 0.0)
    outs, _ = _group(probs[:1], inits[:1], 0.0, flags)
    pair, _ = _group(probs, inits, 0.0, flags)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], want[0])
    for (A, B, _), o in zip(probs, pair):
        ref = A.double().t() @ B.double()
        err = relerr(o, ref)
        print(f"bf16 slabs {bf16}: {tuple(o.shape)} relative error {err:.3e}")
        assert err < (2 ** -8 if bf16 else 1e-5)


def test_group_c2_shapes_bitwise():
    """The C2 attention sublayer's pair: (384, 384) + (1152, 384) at K = 16384 tokens, split 14 each
    (504 items), bf16 slabs, deferred -- bitwise the two single launches."""
    torch.manual_seed(5)
    K = 16384
    dy = (torch.randn(K, 384, device=DEV) * 0.1).to(torch.bfloat16)
    o = (torch.randn(K, 384, device=DEV) * 0.5).to(torch.bfloat16)
    dqkv = (torch.randn(K, 1152, device=DEV) * 0.1).to(torch.bfloat16)
    a = (torch.randn(K, 384, device=DEV) * 0.5).to(torch.bfloat16)
    probs = [(dy, o, 14), (dqkv, a, 14)]
    inits = [torch.full((384, 384), float("nan"), device=DEV), torch.full((1152, 384), float("nan"), device=DEV)]
    flags = _flags(True, True)
    want = []
    for (A, B, s), init in zip(probs, inits):
        out, ws = _single(A, B, init, 0.0, s, flags)
        _flush()
        want.append(out)
    outs, wss = _group(probs, inits, 0.0, flags)
    _flush()
    torch.cuda.synchronize()
    for o_, w in zip(outs, want):
        assert not torch.isnan(o_).any()
        assert torch.equal(o_, w)


def test_group_unsupported_says_no():
    """Problems the persistent kernel does not take (split 1, a width that is no multiple of 128, fp32
    operands) are declined, so the caller issues the single calls."""
    K = 1024
    A = torch.randn(K, 128, device=DEV).to(torch.bfloat16)
    B = torch.randn(K, 128, device=DEV).to(torch.bfloat16)
    out = torch.empty(128, 128, device=DEV)
    ws = _ws(128, 128, 4)
    sup = ops().gemm_wgrad_group_supported
    assert sup([A, A], [B, B], [out, out.clone()], [ws, ws.clone()], [0.0, 0.0], [4, 4], 0)
    assert not sup([A, A], [B, B], [out, out.clone()], [ws, ws.clone()], [0.0, 0.0], [4, 1], 0)
    A96 = torch.randn(K, 96, device=DEV).to(torch.bfloat16)
    assert not sup([A96], [B], [torch.empty(96, 128, device=DEV)], [ws], [0.0], [4], 0)
    assert not sup([A.float()], [B.float()], [out], [ws], [0.0], [4], 0)


def test_training_step_group_on_and_off():
    """One small training step (2 layers, 128d, 2 heads, block 64, batch 8) with functional.WGRAD_GROUP
    on (the attention pair alone, and with the FeedForward pair) and off: the loss is equal and every gradient is within 2^-8
    relative of the other (both sum bf16-rounded partials of the same products).  At this size the
    grouped plan picks the splits the single calls pick (2 each: 8 K-tiles, at least 4 per split), so
    the gradients are identical bits."""
    from replicatinggpt_amd import AdamW, BigramLanguageModel, GPTConfig
    from replicatinggpt_amd import functional as Fn
    from replicatinggpt_amd.data import BatchSampler, TokenStream
    from replicatinggpt_amd.engine import TrainStep
    cfg = GPTConfig(block_size=64, n_embd=128, n_head=2, n_layers=2, dropout=0.2, dtype="bf16", batch_size=8)
    assert Fn._split_for_tiles(1 + 3, 8) == Fn._wgrad_split(128, 128, 512, True) == Fn._wgrad_split(384, 128, 512, True)
    saved = Fn.WGRAD_GROUP, Fn.WGRAD_GROUP_FFN
    runs = []
    try:
        for on, ffn in ((0, 0), (1, 0), (1, 1)):
            Fn.WGRAD_GROUP, Fn.WGRAD_GROUP_FFN = on, ffn
            torch.manual_seed(1337)
            m = BigramLanguageModel(cfg).to(DEV)
            opt = AdamW(m.parameters(), lr=1e-3)
            s = BatchSampler(TokenStream.synthetic(device=DEV), cfg.block_size, cfg.batch_size)
            st = TrainStep(m, opt, s, use_graph=False)
            loss = float(st.step().detach())
            torch.cuda.synchronize()
            grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
            runs.append((loss, grads, m.flat.master.detach().cpu().clone()))
    finally:
        Fn.WGRAD_GROUP, Fn.WGRAD_GROUP_FFN = saved
    base = runs[0]
    assert all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in base[1].values())
    for r in runs[1:]:
        assert r[0] == base[0]
        for n, g in base[1].items():
            err = relerr(r[1][n], g)
            assert err < 2 ** -8, (n, err)
            assert torch.equal(r[1][n], g), n
        assert torch.equal(r[2], base[2])


def test_grouped_split_at_c2_is_14():
    """The split of the C2 attention pair from _wgrad_split's cost over the sum of the tiles (9 + 27 on
    512 slots, 256 K-tiles): 14, the FeedForward weight gradients' split."""
    from replicatinggpt_amd import functional as Fn
    assert Fn._split_for_tiles(9 + 27, 16384 // 64, slots=512) == 14
    assert Fn._split_for_tiles(36, 16384 // 64, slots=512) == Fn._split_for_tiles(72, 16384 // 64, slots=512) * 2
