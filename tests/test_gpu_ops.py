"""Per-kernel parity on the MI355X: each charpt op against a plain fp32/fp64 torch CPU
reference (and the numpy Philox oracle for dropout masks).  Tolerances: fp32 path rtol 1e-5
(relative to the output scale), bf16 path 2e-2 -- the north_star's bars."""
import math

import numpy as np
import os

import pytest

import torch

from numerics import fma32 as _fma32    # the exactly rounded float32 fma of the AdamW restatements

from conftest import bf16_close

from oracle import philox

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def F():
    from replicatinggpt_amd import functional as Fn
    return Fn


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_device_is_gfx950():
    from replicatinggpt_amd import _lib as L
    import ctypes
    n, ma, mi = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.check(L.load().cg_device_info(ctypes.byref(n), ctypes.byref(ma), ctypes.byref(mi)))
    assert (ma.value, mi.value) == (9, 5) and n.value >= 64


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_dropout_mask_matches_oracle(p):
    n = 10007
    call = torch.tensor([5], dtype=torch.int64, device=DEV)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    ops().dropout_mask(out, p, 0x1337, call, 3)
    want = philox.keep_mask(0x1337, (5 << 8) | 3, np.arange(n), p)
    assert np.array_equal(out.cpu().numpy() > 0.5, want)


@pytest.mark.parametrize("C", [126, 384, 512, 768, 1024, 33, 128, 64, 2])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_layernorm(C, out_dtype):
    torch.manual_seed(0)
    rows = 300
    x = torch.randn(rows, C) * 2 + 0.5
    w = torch.randn(C) * 0.1 + 1
    b = torch.randn(C) * 0.1
    xr = x.clone().double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (C,), wr, br, 1e-5)
    gy = torch.randn(rows, C)
    yr.backward(gy.double())
    Fn = F()
    y, mean, rstd = Fn.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), out_dtype)
    tol = 1e-5 if out_dtype == torch.float32 else 1e-2
    assert relerr(y, yr) < tol
    dres = torch.randn(rows, C)
    wreg, breg = Fn.Region.of(torch.nn.Parameter(w.to(DEV))), Fn.Region.of(torch.nn.Parameter(b.to(DEV)))
    dx, _, grads = Fn.layernorm_bwd(gy.to(DEV).to(out_dtype), x.to(DEV), wreg, breg, mean, rstd, dres=dres.to(DEV))
    gyq = gy.to(out_dtype).double()
    yr2 = torch.nn.functional.layer_norm(x.double().requires_grad_(True), (C,), w.double(), b.double(), 1e-5)
    xr2 = x.double().requires_grad_(True)
    wr2, br2 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xr2, (C,), wr2, br2, 1e-5).backward(gyq)
    assert relerr(dx, xr2.grad + dres.double()) < 1e-5
    assert relerr(grads[0], wr2.grad) < 1e-5
    assert relerr(grads[1], br2.grad) < 1e-5


@pytest.mark.parametrize("C,B,H,T", [(384, 64, 6, 256), (768, 4, 12, 1024), (126, 2, 6, 256), (384, 3, 6, 64)])
@pytest.mark.parametrize("p", [0.2, 0.6])
def test_layernorm_fwd_attn_dropmask_matches_separate_launches(C, B, H, T, p):
    """cg_layernorm_fwd_attn_dropmask (ln1 forward + the attention keep bits in one launch,
    GPT1.py:163,117) == cg_layernorm_fwd then cg_attn_dropmask, bit for bit: y, mean, rstd and every
    mask word (p = 0.6 takes the thr > 2^15 Philox compare).  C = 126: the two-launch fallback."""
    O = ops()
    torch.manual_seed(5)
    rows = B * T
    x = (torch.randn(rows, C, device=DEV) * 2 + 0.5)
    w = torch.randn(C, device=DEV) * 0.1 + 1
    b = torch.randn(C, device=DEV) * 0.1
    call = torch.tensor([3], dtype=torch.int64, device=DEV)
    n = O.attn_mask_bytes(B, H, T) // 8
    outs = []
    for fused in (True, False):
        y = torch.full((rows, C), float("nan"), device=DEV).to(torch.bfloat16)
        mean, rstd = torch.full((rows,), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV)
        mask = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        if fused:
            O.layernorm_fwd_attn_dropmask(x, w, b, y, mean, rstd, 1e-5, B, H, T, p, 77, call, 2, mask)
        else:
            O.layernorm_fwd(x, w, b, y, mean, rstd, 1e-5)
            O.attn_dropmask(B, H, T, p, 77, call, 2, mask)
        torch.cuda.synchronize()
        outs.append((y.view(torch.int16), mean, rstd, mask))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    assert not torch.isnan(outs[0][1]).any()


@pytest.mark.parametrize("M,K", [(16384, 384), (16384, 1536), (64, 64), (192, 640)])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("inplace", [False, True])
def test_gemm_resid_layernorm_matches_two_launches(M, K, p, inplace):
    """cg_gemm_resid_layernorm (the C2 projection / FFN2 forward with the next LayerNorm in its
    epilogue, GPT1.py:136,145-147 + 159-160,173) == cg_gemm (bias + [dropout +] residual, fp32) then
    cg_layernorm_fwd, bit for bit at the step's shapes: x, y, mean and rstd -- also with x written
    over the residual (the in-place residual stream); x against fp64 and the oracle's dropout mask."""
    O = ops()
    N = 384
    torch.manual_seed(17)
    a = (torch.randn(M, K, device=DEV) * 0.5).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV) * 0.1
    resid = torch.randn(M, N, device=DEV)
    lw = torch.randn(N, device=DEV) * 0.1 + 1
    lb = torch.randn(N, device=DEV) * 0.1
    assert O.gemm_resid_layernorm_supported(M, N, K)
    outs = []
    for fused in (True, False):
        call = torch.tensor([6], dtype=torch.int64, device=DEV)
        x = resid.clone() if inplace else torch.full((M, N), float("nan"), device=DEV)
        r = x if inplace else resid
        y = torch.full((M, N), float("nan"), device=DEV).to(torch.bfloat16)
        mean, rstd = torch.full((M,), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
        if fused:
            O.gemm_resid_layernorm(a, w, x, M, N, K, K, K, N, bias, r, N, p, 41, call, 2, lw, lb, y, mean, rstd, 1e-5)
        else:
            kind = 4 if p > 0 else 3
            O.gemm(a, w, x, True, False, False, M, N, K, K, K, N, kind, bias, r, N, None, 0, p, 41, call, 2, 0.0, 1,
                   None)
            O.layernorm_fwd(x, lw, lb, y, mean, rstd, 1e-5)
        torch.cuda.synchronize()
        outs.append((x, y.view(torch.int16), mean, rstd))
    # x: the same K order as cg_gemm's persistent kernels (M % 128 == 0); the generic kernel that
    # cg_gemm falls back to below that sums in another order
    if M % 128 == 0:
        assert torch.equal(outs[0][0], outs[1][0])
    else:
        assert relerr(outs[0][0], outs[1][0]) < 1e-6
    # y, mean, rstd: k_ln_fwd's bits on the fused kernel's own x
    y2 = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    m2, r2 = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    O.layernorm_fwd(outs[0][0], lw, lb, y2, m2, r2, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][1], y2.view(torch.int16))
    assert torch.equal(outs[0][2], m2) and torch.equal(outs[0][3], r2)
    assert not torch.isnan(outs[0][0]).any() and not torch.isnan(outs[0][2]).any()
    acc = a.double() @ w.double().t() + bias.double()
    if p > 0:
        keep = philox.keep_mask(41, (6 << 8) | 2, np.arange(M * N), p).reshape(M, N)
        acc = torch.from_numpy(keep).to(DEV).double() * acc * float(np.float32(1 / (1 - p)))
    assert relerr(outs[0][0], resid.double() + acc) < 1e-5


def test_gemm_resid_layernorm_rejects_unsupported():
    O = ops()
    assert not O.gemm_resid_layernorm_supported(128, 768, 384)
    assert not O.gemm_resid_layernorm_supported(100, 384, 384)
    a = torch.zeros(128, 384, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(768, 384, device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(128, 768, device=DEV)
    y = torch.zeros(128, 768, device=DEV, dtype=torch.bfloat16)
    v = torch.zeros(768, device=DEV)
    st = torch.zeros(128, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        O.gemm_resid_layernorm(a, w, x, 128, 768, 384, 384, 384, 768, v, x, 768, 0.0, 0, None, 0, v, v, y, st, st,
                               1e-5)


@pytest.mark.parametrize("C", [384, 768, 126])
@pytest.mark.parametrize("with_link", [False, True])
def test_layernorm_bwd_rows_then_reduce_is_bitwise_ex(C, with_link):
    """cg_layernorm_bwd_rows + cg_layernorm_bwd_reduce on a second stream (the training path's
    side-stream split) == cg_layernorm_bwd_ex bit for bit: dx, the consumer's dropout-applied bf16
    copy, dgamma / dbeta (accumulated) and the copy's column sums."""
    torch.manual_seed(3)
    O = ops()
    rows = 1000
    x = (torch.randn(rows, C) * 2 + 0.5).to(DEV)
    w = (torch.randn(C) * 0.1 + 1).to(DEV)
    mean, rstd = x.mean(1), x.var(1, unbiased=False).add(1e-5).rsqrt()
    dy = torch.randn(rows, C, device=DEV).to(torch.bfloat16)
    dres = torch.randn(rows, C, device=DEV)
    call = torch.tensor([9], dtype=torch.int64, device=DEV)
    p = 0.2 if with_link else 0.0
    outs = []
    for split in (False, True):
        dx = torch.empty(rows, C, device=DEV)
        lp = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV) if with_link else None
        dw, db = torch.ones(C, device=DEV), torch.ones(C, device=DEV)
        cs = torch.ones(C, device=DEV) if with_link else None
        ws = torch.full((O.layernorm_bwd_workspace(rows, C) // 4 + 1,), float("nan"), device=DEV)
        if split:
            O.layernorm_bwd_rows(dy, x, w, mean, rstd, dres, dx, lp, ws, with_link, p, 11, call if p else None, 4)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                O.layernorm_bwd_reduce(ws, rows, C, with_link, dw, db, cs, True, True)
            torch.cuda.current_stream().wait_stream(side)
        else:
            O.layernorm_bwd(dy, x, w, mean, rstd, dres, dx, lp, dw, db, True, ws, cs, True, p, 11,
                            call if p else None, 4)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (dx, lp, dw, db, cs) if t is not None])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rows", [16384, 1000, 7])
@pytest.mark.parametrize("with_link", [False, True])
def test_layernorm_bwd_row_loop_order_is_bitwise(rows, with_link):
    """The C = 384 backward rows with the next row's loads issued before the current row's stores
    (ln_rl 1, the default) == the load / compute / store order (ln_rl 0) bit for bit: dx, the
    consumer's dropout-applied bf16 copy, dgamma / dbeta and the copy's column sums; C2's 16384 rows
    (4 rows per wave), a ragged count and fewer rows than waves."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    torch.manual_seed(5)
    O = ops()
    C = 384
    x = (torch.randn(rows, C) * 2 + 0.5).to(DEV)
    w = (torch.randn(C) * 0.1 + 1).to(DEV)
    mean, rstd = x.mean(1), x.var(1, unbiased=False).add(1e-5).rsqrt()
    dy = torch.randn(rows, C, device=DEV).to(torch.bfloat16)
    dres = torch.randn(rows, C, device=DEV)
    call = torch.tensor([9], dtype=torch.int64, device=DEV)
    p = 0.2 if with_link else 0.0
    outs = []
    try:
        for rl in (0, 1):
            L.check(lib.cg_set_tuning(b"ln_rl", rl))
            dx = torch.full((rows, C), float("nan"), device=DEV)
            lp = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV) if with_link else None
            dw, db = torch.ones(C, device=DEV), torch.ones(C, device=DEV)
            cs = torch.ones(C, device=DEV) if with_link else None
            ws = torch.full((O.layernorm_bwd_workspace(rows, C) // 4 + 1,), float("nan"), device=DEV)
            O.layernorm_bwd(dy, x, w, mean, rstd, dres, dx, lp, dw, db, True, ws, cs, True, p, 11,
                            call if p else None, 4)
            torch.cuda.synchronize()
            outs.append([t.cpu() for t in (dx, lp, dw, db, cs) if t is not None])
    finally:
        L.check(lib.cg_set_tuning(b"ln_rl", 1))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.isnan(outs[1][0]).any()


@pytest.mark.parametrize("M,Fh,C", [(2048, 1536, 384), (16384, 3072, 768)])
def test_relu_keep_bits_roundtrip(M, Fh, C):
    """FeedForward's ReLU keep bits (CG_BITS): the W1 forward with bits gives the same bf16 h as the
    plain bias+ReLU epilogue and bits == (h != 0) packed 32 per word; the W2 ReLU-backward dgrad
    reading the bits (plain and with the fused b1 column partials) equals the one reading h, bit for
    bit.  C2 shapes take the 128x128 kernel, the C4-width ones the 8-wave 256x256 kernel."""
    Fn = F()
    O = ops()
    torch.manual_seed(8)
    a = (torch.randn(M, C, device=DEV) * 0.5).to(torch.bfloat16)
    w1 = (torch.randn(Fh, C, device=DEV) * 0.05).to(torch.bfloat16)
    b1 = torch.randn(Fh, device=DEV) * 0.1
    w2 = (torch.randn(C, Fh, device=DEV) * 0.05).to(torch.bfloat16)
    dz2 = torch.randn(M, C, device=DEV).to(torch.bfloat16)
    assert Fn._relu_bits_ok(a, w1, w2, Fh)
    h_ref = torch.empty(M, Fh, dtype=torch.bfloat16, device=DEV)
    Fn.linear_fwd(a, w1, h_ref, "bias_relu", bias=b1)
    h = torch.empty_like(h_ref)
    bits = torch.empty(M, Fh // 32, dtype=torch.int32, device=DEV)
    O.gemm_bias_relu_bits(a, w1, h, M, Fh, C, C, C, Fh, b1, bits, Fh // 32)
    torch.cuda.synchronize()
    assert torch.equal(h, h_ref)
    nz = (h.view(torch.int16) & 0x7FFF) != 0
    weights = (torch.ones(32, dtype=torch.int64, device=DEV) << torch.arange(32, device=DEV))
    want = (nz.view(M, Fh // 32, 32).long() * weights).sum(-1)
    assert torch.equal(bits.long() & 0xFFFFFFFF, want)
    d_ref, d_bits = torch.empty_like(h), torch.empty_like(h)
    Fn.linear_dgrad(dz2, w2, d_ref, "relu_bwd", aux=h)
    Fn.linear_dgrad(dz2, w2, d_bits, "relu_bwd", aux=bits)
    p_ref, p_bits = (torch.empty(M // 64, Fh, device=DEV) for _ in range(2))
    c_ref, c_bits = torch.empty_like(h), torch.empty_like(h)
    O.gemm_relu_bwd_colpart(dz2, w2, c_ref, M, Fh, C, C, Fh, Fh, h, Fh, p_ref)
    O.gemm_relu_bwd_colpart(dz2, w2, c_bits, M, Fh, C, C, Fh, Fh, bits, Fh // 32, p_bits)
    torch.cuda.synchronize()
    assert torch.equal(d_ref, d_bits) and torch.equal(c_ref, c_bits) and torch.equal(p_ref, p_bits)
    assert torch.equal(c_ref, d_ref)


@pytest.mark.parametrize("C", [384, 768, 1024, 512, 126])
def test_layernorm_bwd_link_dropout_matches_oracle(C):
    """The LayerNorm backward's consumer copy with FeedForward's output dropout (GPT1.py:146; the
    keep bits of a row shared across lanes, one Philox group per lane, when C % 8 == 0) equals
    bf16(dx * keep / (1 - p)) with keep from the oracle's Philox stream, bit for bit."""
    torch.manual_seed(4)
    O = ops()
    rows, p, seed, call_v, site = 700, 0.2, 11, 9, 4
    x = (torch.randn(rows, C) * 2 + 0.5).to(DEV)
    w = (torch.randn(C) * 0.1 + 1).to(DEV)
    mean, rstd = x.mean(1), x.var(1, unbiased=False).add(1e-5).rsqrt()
    dy = torch.randn(rows, C, device=DEV).to(torch.bfloat16)
    dx = torch.empty(rows, C, device=DEV)
    lp = torch.empty(rows, C, dtype=torch.bfloat16, device=DEV)
    dw, db, cs = (torch.zeros(C, device=DEV) for _ in range(3))
    ws = torch.empty(O.layernorm_bwd_workspace(rows, C) // 4 + 1, device=DEV)
    call = torch.tensor([call_v], dtype=torch.int64, device=DEV)
    O.layernorm_bwd(dy, x, w, mean, rstd, None, dx, lp, dw, db, False, ws, cs, False, p, seed, call, site)
    torch.cuda.synchronize()
    keep = torch.from_numpy(philox.keep_mask(seed, (call_v << 8) | site, np.arange(rows * C), p).reshape(rows, C))
    want = (dx.cpu() * keep.float() * (1.0 / (1.0 - p))).to(torch.bfloat16)
    assert torch.equal(lp.cpu(), want)


@pytest.mark.parametrize("M,F,K", [(512, 384, 128), (1024, 1536, 384), (16384, 1536, 384), (32768, 3072, 768),
                                   (65536, 3072, 768)])
def test_relu_bwd_colpart_matches_colsum(M, F, K):
    """The ReLU-backward dgrad with fused column partials (cg_epilogue_t.colpart): the output is
    bitwise the plain relu_bwd GEMM's, and the folded partials equal the column sums of that bf16
    output (the values cg_colsum and the W1 weight gradient see) to 1e-5 relative.  The last two
    shapes (C4's FFN2 dgrad and half of it) run the 8-wave 256x256 kernel, the others the 128x128."""
    O = ops()
    torch.manual_seed(5)
    dy = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(K, F, device=DEV) * 0.05).to(torch.bfloat16)
    h = torch.relu(torch.randn(M, F, device=DEV)).to(torch.bfloat16)
    ref = torch.empty(M, F, dtype=torch.bfloat16, device=DEV)
    O.gemm(dy, w, ref, True, False, True, M, F, K, K, F, F, 5, None, None, 0, h, F, 0.0, 0, None, 0, 0.0, 1, None)
    out = torch.empty_like(ref)
    part = torch.full((M // 64, F), float("nan"), device=DEV)
    O.gemm_relu_bwd_colpart(dy, w, out, M, F, K, K, F, F, h, F, part)
    cs = torch.empty(F, device=DEV)
    O.reduce_rows(part, M // 64, F, cs, False)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert relerr(cs, out.double().sum(0)) < 1e-5
    # and they are the exact product's column sums up to the bf16 rounding of the output
    want = ((dy.double() @ w.double()) * (h.double() > 0)).sum(0)
    assert relerr(cs, want) < 1e-2


def _ref_gemm(A, B, at, bt):
    a = A.double().t() if at else A.double()
    b = B.double().t() if bt else B.double()
    return a @ b.t()


@pytest.mark.parametrize("at,bt", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("shape", [(37, 65, 126), (128, 384, 192), (256, 128, 1536)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_gemm_layouts(at, bt, shape, dt):
    M, N, K = shape
    torch.manual_seed(1)
    A = (torch.randn(K, M) if at else torch.randn(M, K)).to(dt)
    B = (torch.randn(K, N) if bt else torch.randn(N, K)).to(dt)
    ref = _ref_gemm(A, B, at, bt)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    lda = A.shape[1]
    ldb = B.shape[1]
    ops().gemm(A.to(DEV), B.to(DEV), out, dt == torch.bfloat16, bool(at), bool(bt), M, N, K, lda, ldb, N, 0, None,
               None, 0, None, 0, 0.0, 0, None, 0, 0.0, 1, None)
    assert relerr(out, ref) < 1e-5


# the product library's variants; the whole matrix when the A/B build is loaded (CHARPT_LIB=...ab.so)
_GEMM_VARIANTS = ([(1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0),
                   (9, 5), (10, 0), (10, 7), (11, 0), (11, 3), (12, 0),
                   (20, 0), (21, 0), (21, 3), (22, 0), (22, 5), (23, 0), (23, 7),
                   (24, 0), (24, 1), (25, 0), (25, 2)]
                  if "_ab" in os.environ.get("CHARPT_LIB", "") else [(2, 0), (9, 0), (9, 5), (24, 0), (24, 1)])


@pytest.mark.parametrize("variant,max_grid", _GEMM_VARIANTS)
@pytest.mark.parametrize("at,bt", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(512, 384, 768), (512, 512, 640)])
def test_gemm_kernel_variants(variant, max_grid, at, bt, M, N, K):
    """Every bf16 MFMA kernel variant (register-staged 1-4, LDS-DMA 5-8, persistent LDS-DMA 9-12,
    persistent 8-wave LDS-DMA 20-25 -- with the grid capped so that each block walks several tiles)
    on all four layouts, with split-K and the fused bias+ReLU and bias+dropout+residual epilogues.
    The product library carries 2, 9 and 24; the others only the A/B build (`make ab`,
    CHARPT_LIB=replicatinggpt_amd/libcharpt_hip_ab.so), where the whole matrix runs."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    if lib.cg_set_tuning(b"gemm_variant", variant) != 0:
        pytest.skip(f"gemm_variant {variant} is A/B-only (not in this library build)")
    torch.manual_seed(7)
    A = (torch.randn(K, M) if at else torch.randn(M, K)).to(torch.bfloat16)
    B = (torch.randn(K, N) if bt else torch.randn(N, K)).to(torch.bfloat16)
    bias = torch.randn(N)
    ref = _ref_gemm(A, B, at, bt)
    Ad, Bd = A.to(DEV), B.to(DEV)
    L.check(lib.cg_set_tuning(b"gemm_variant", variant))
    L.check(lib.cg_set_tuning(b"gemm_max_grid", max_grid))
    try:
        out = torch.empty(M, N, dtype=torch.float32, device=DEV)
        ops().gemm(Ad, Bd, out, True, bool(at), bool(bt), M, N, K, A.shape[1], B.shape[1], N, 0, None, None, 0,
                   None, 0, 0.0, 0, None, 0, 0.0, 1, None)
        ws = torch.empty(ops().gemm_workspace(M, N, 3) // 4, dtype=torch.float32, device=DEV)
        out3 = torch.empty(M, N, dtype=torch.float32, device=DEV)
        ops().gemm(Ad, Bd, out3, True, bool(at), bool(bt), M, N, K, A.shape[1], B.shape[1], N, 0, None, None, 0,
                   None, 0, 0.0, 0, None, 0, 0.0, 3, ws)
        h = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        ops().gemm(Ad, Bd, h, True, bool(at), bool(bt), M, N, K, A.shape[1], B.shape[1], N, 2, bias.to(DEV), None,
                   0, None, 0, 0.0, 0, None, 0, 0.0, 1, None)
        resid = torch.randn(M, N)
        call = torch.tensor([6], dtype=torch.int64, device=DEV)
        o = torch.empty(M, N, dtype=torch.float32, device=DEV)
        ops().gemm(Ad, Bd, o, True, bool(at), bool(bt), M, N, K, A.shape[1], B.shape[1], N, 4, bias.to(DEV),
                   resid.to(DEV), N, None, 0, 0.2, 99, call, 3, 0.0, 1, None)
        torch.cuda.synchronize()
    finally:
        L.check(lib.cg_set_tuning(b"gemm_variant", 0))
        L.check(lib.cg_set_tuning(b"gemm_max_grid", 0))
    assert relerr(out, ref) < 1e-5
    assert relerr(out3, ref) < 1e-5
    assert relerr(h, torch.relu(ref + bias.double())) < 8e-3
    keep = philox.keep_mask(99, (6 << 8) | 3, np.arange(M * N), 0.2).reshape(M, N)
    want = resid.double() + torch.from_numpy(keep).double() * (ref + bias.double()) * float(np.float32(1 / 0.8))
    assert relerr(o, want) < 1e-5


@pytest.mark.parametrize("bt", [0, 1])
def test_gemm_default_picks_large_tile(bt):
    """At >= 2 256x256 tiles per CU the default dispatch takes the 8-wave 256x256 kernel (C4 forward
    and dgrad shapes): plain store, bias+ReLU and bias+dropout+residual epilogues at such a shape."""
    M, N, K = 8192, 4096, 128
    torch.manual_seed(11)
    A = torch.randn(M, K).to(torch.bfloat16)
    B = (torch.randn(K, N) if bt else torch.randn(N, K)).to(torch.bfloat16)
    bias = torch.randn(N)
    ref = _ref_gemm(A, B, 0, bt)
    Ad, Bd = A.to(DEV), B.to(DEV)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ops().gemm(Ad, Bd, out, True, False, bool(bt), M, N, K, K, B.shape[1], N, 0, None, None, 0,
               None, 0, 0.0, 0, None, 0, 0.0, 1, None)
    h = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops().gemm(Ad, Bd, h, True, False, bool(bt), M, N, K, K, B.shape[1], N, 2, bias.to(DEV), None,
               0, None, 0, 0.0, 0, None, 0, 0.0, 1, None)
    resid = torch.randn(M, N)
    call = torch.tensor([4], dtype=torch.int64, device=DEV)
    o = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ops().gemm(Ad, Bd, o, True, False, bool(bt), M, N, K, K, B.shape[1], N, 4, bias.to(DEV),
               resid.to(DEV), N, None, 0, 0.2, 5, call, 1, 0.0, 1, None)
    torch.cuda.synchronize()
    assert relerr(out, ref) < 1e-5
    assert relerr(h, torch.relu(ref + bias.double())) < 8e-3
    keep = philox.keep_mask(5, (4 << 8) | 1, np.arange(M * N), 0.2).reshape(M, N)
    want = resid.double() + torch.from_numpy(keep).double() * (ref + bias.double()) * float(np.float32(1 / 0.8))
    assert relerr(o, want) < 1e-5


@pytest.mark.parametrize("split", [2, 4, 8, 3, 5, 12, 14, 31])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_gemm_splitk_deterministic(split, dt):
    """Split-K weight-gradient layout (TT), deterministic run to run and equal to fp64; splits that
    do not divide the 32 K-tiles run the persistent kernel's uneven split (last split shorter)."""
    M, N, K = 128, 256, 2048
    torch.manual_seed(2)
    A = torch.randn(K, M).to(dt).to(DEV)
    B = torch.randn(K, N).to(dt).to(DEV)
    ref = _ref_gemm(A.cpu(), B.cpu(), 1, 1)
    outs = []
    for _ in range(2):
        out = torch.empty(M, N, dtype=torch.float32, device=DEV)
        ws = torch.empty(ops().gemm_workspace(M, N, split) // 4, dtype=torch.float32, device=DEV)
        ops().gemm(A, B, out, dt == torch.bfloat16, True, True, M, N, K, M, N, N, 0, None, None, 0, None, 0, 0.0,
                   0, None, 0, 0.0, split, ws)
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    assert relerr(outs[0], ref) < 1e-5


@pytest.mark.parametrize("M,N,K,split", [(384, 1536, 16384, 14), (1152, 384, 16384, 18), (384, 384, 16384, 24),
                                         (768, 3072, 65536, 10)])
def test_gemm_uneven_splitk_wgrad_shapes(M, N, K, split):
    """The C2 / C4 weight-gradient shapes at uneven split counts (the persistent 128x128 kernel's
    ceil-sized K chunks) against an fp64 product of the same bf16 operands (fp32 accumulation:
    1e-5 relative)."""
    torch.manual_seed(11)
    A = (torch.randn(K, M, device=DEV) * 0.5).to(torch.bfloat16)
    B = (torch.randn(K, N, device=DEV) * 0.5).to(torch.bfloat16)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops().gemm_workspace(M, N, split) // 4, dtype=torch.float32, device=DEV)
    ops().gemm(A, B, out, True, True, True, M, N, K, M, N, N, 0, None, None, 0, None, 0, 0.0, 0, None, 0, 0.0, split,
               ws)
    ref = A.double().t() @ B.double()
    assert relerr(out, ref) < 1e-5


@pytest.mark.parametrize("M,N,K,split", [(384, 1536, 16384, 14), (768, 3072, 65536, 7), (256, 2048, 4096, 4),
                                         (1536, 384, 16384, 14)])
def test_gemm_tile_order_is_bitwise_invariant(M, N, K, split):
    """The persistent kernel's automatic tile order (column-major where B panels outnumber A panels:
    the FFN2 weight gradient dW2 = dz2^T h, GPT1.py:145 backward) against forced row-major
    (cg_set_tuning gemm_group_pk = 1) and a 3-row grouping: the order only moves items between
    blocks, so the output is equal bit for bit."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    torch.manual_seed(13)
    A = (torch.randn(K, M, device=DEV) * 0.5).to(torch.bfloat16)
    B = (torch.randn(K, N, device=DEV) * 0.5).to(torch.bfloat16)
    ws = torch.empty(ops().gemm_workspace(M, N, split) // 4, dtype=torch.float32, device=DEV)
    outs = []
    try:
        for g in (0, 1, 3):
            L.check(lib.cg_set_tuning(b"gemm_group_pk", g))
            out = torch.full((M, N), float("nan"), device=DEV)
            ops().gemm(A, B, out, True, True, True, M, N, K, M, N, N, 0, None, None, 0, None, 0, 0.0, 0, None, 0,
                       0.0, split, ws)
            outs.append(out)
    finally:
        L.check(lib.cg_set_tuning(b"gemm_group_pk", 0))
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("M,N,K,split", [(1152, 384, 16384, 16), (384, 1536, 16384, 14), (384, 384, 16384, 24),
                                         (256, 2048, 4096, 4)])
@pytest.mark.parametrize("defer", [False, True])
def test_gemm_bf16_slabs(M, N, K, split, defer):
    """cg_epilogue_t.flags CG_GEMM_SLAB_BF16 (the training backward's weight gradients, GPT1.py:232 backward):
    the split-K partial sums go through bf16 slabs.  The output is exactly the fp32 sum, in split
    order, of each split's fp32 partial (a split-1 GEMM over that K chunk: same MFMA order) rounded
    to bf16 -- bit for bit, with the reduce in line or deferred into the next GEMM's tail / the
    flush -- and within bf16 rounding of the fp64 product."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    torch.manual_seed(19)
    A = (torch.randn(K, M, device=DEV) * 0.5).to(torch.bfloat16)
    B = (torch.randn(K, N, device=DEV) * 0.5).to(torch.bfloat16)
    ws = torch.empty(ops().gemm_workspace(M, N, split) // 4, dtype=torch.float32, device=DEV)
    out = torch.full((M, N), float("nan"), device=DEV)
    flags = L.GEMM_SLAB_BF16 | (L.GEMM_DEFER_REDUCE if defer else 0)
    ops().gemm(A, B, out, True, True, True, M, N, K, M, N, N, 0, None, None, 0, None, 0, 0.0, 0, None, 0, 0.0,
               split, ws, flags)
    if defer:   # a later persistent launch on the stream takes the pending reduce in its tail
        x = torch.randn(256, 128, device=DEV).to(torch.bfloat16)
        y = torch.empty(256, 128, dtype=torch.bfloat16, device=DEV)
        ops().gemm(x, x[:128], y, True, False, False, 256, 128, 128, 128, 128, 128, 0, None, None, 0, None, 0,
                   0.0, 0, None, 0, 0.0, 1, None)
        L.check(lib.cg_flush_deferred(L.ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    kc = -(-(K // 64) // split) * 64
    want = None
    for sp in range(split):
        k0, k1 = sp * kc, min(K, (sp + 1) * kc)
        part = torch.empty(M, N, device=DEV)
        Ak, Bk = A[k0:k1], B[k0:k1]
        ops().gemm(Ak, Bk, part, True, True, True, M, N, k1 - k0, M, N, N, 0, None, None, 0, None, 0, 0.0, 0, None, 0,
                   0.0, 1, None)
        p16 = part.to(torch.bfloat16).float()
        want = p16 if want is None else want + p16
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    assert torch.equal(out, want)
    ref = A.double().t() @ B.double()
    assert relerr(out, ref) < 2 ** -8   # each partial rounded once to bf16 (2^-9 relative)


@pytest.mark.parametrize("c_dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_gemm_splitk_reduce_vec_matches_scalar(c_dt, beta):
    """The vectorised split-K reducer (16-B rows) and the scalar one (odd ldc) give bitwise the same
    bias + residual epilogue, and both match the fp64 reference."""
    M, N, K, split = 96, 256, 1024, 4
    torch.manual_seed(3)
    A = torch.randn(M, K).to(torch.bfloat16).to(DEV)
    B = torch.randn(N, K).to(torch.bfloat16).to(DEV)
    bias = torch.randn(N, device=DEV)
    resid = torch.randn(M, N, device=DEV)
    init = torch.randn(M, N + 1, device=DEV).to(c_dt)
    ws = torch.empty(ops().gemm_workspace(M, N, split) // 4, dtype=torch.float32, device=DEV)
    res = []
    for ldc in (N, N + 1):
        out = init[:, :ldc].contiguous() if ldc == N else init.clone()
        ops().gemm(A, B, out, True, False, False, M, N, K, K, K, ldc, 3, bias, resid, N, None, 0, 0.0, 0, None, 0,
                   beta, split, ws)
        res.append(out[:, :N].float().cpu())
    assert torch.equal(res[0], res[1])
    ref = (A.double() @ B.double().t()).cpu() + bias.double().cpu() + resid.double().cpu()
    ref = ref + beta * init[:, :N].double().cpu()
    assert relerr(res[0], ref) < (1e-5 if c_dt == torch.float32 else 1e-2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(256, 384, 128), (96, 70, 40)])
def test_gemm_epilogues(dt, M, N, K):
    Fn = F()
    torch.manual_seed(3)
    x = torch.randn(M, K).to(dt)
    w = torch.randn(N, K).to(dt)
    bias = torch.randn(N)
    resid = torch.randn(M, N)
    acc = x.double() @ w.double().t()
    xd, wd = x.to(DEV), w.to(DEV)
    tol = 1e-5 if dt == torch.float32 else 8e-3
    # bias + relu
    h = torch.empty(M, N, dtype=dt, device=DEV)
    Fn.linear_fwd(xd, wd, h, "bias_relu", bias=bias.to(DEV))
    assert relerr(h, torch.relu(acc + bias.double())) < tol
    # bias + residual (fp32 out)
    o = torch.empty(M, N, dtype=torch.float32, device=DEV)
    Fn.linear_fwd(xd, wd, o, "bias_resid", bias=bias.to(DEV), resid=resid.to(DEV))
    assert relerr(o, acc + bias.double() + resid.double()) < 1e-5
    # bias + dropout + residual against the oracle mask
    call = torch.tensor([9], dtype=torch.int64, device=DEV)
    Fn.linear_fwd(xd, wd, o, "bias_drop_resid", bias=bias.to(DEV), resid=resid.to(DEV), dropout_p=0.2, seed=77,
                  rng_call=call, site=5)
    keep = philox.keep_mask(77, (9 << 8) | 5, np.arange(M * N), 0.2).reshape(M, N)
    want = resid.double() + torch.from_numpy(keep).double() * (acc + bias.double()) * float(np.float32(1 / 0.8))
    assert relerr(o, want) < 1e-5
    # relu backward with an aux mask
    aux = torch.randn(M, N).to(dt)
    g = torch.empty(M, N, dtype=dt, device=DEV)
    ops().gemm(xd, wd, g, dt == torch.bfloat16, False, False, M, N, K, K, K, N, 5, None, None, 0, aux.to(DEV), N,
               0.0, 0, None, 0, 0.0, 1, None)
    assert relerr(g, acc * (aux.double() > 0)) < tol


@pytest.mark.parametrize("M,K", [(16384, 384), (16384, 1536), (256, 128), (1024, 640)])
@pytest.mark.parametrize("kind", ["bias_resid", "bias_drop_resid"])
def test_gemm_n96_matches_128x128_bitwise(M, K, kind):
    """The 128x96 tiles of the part-filling fp32 residual forwards (gemm_pk.hip launch_n96: the C2
    projection and FFN2 forwards, GPT1.py:136,145-147) against the 128x128 tiles (cg_set_tuning
    gemm_n96 = 0; their dropout mask is the oracle's, test_gemm_epilogues): same K order per output
    element, so equal bit for bit, dropout included."""
    from replicatinggpt_amd import _lib as L
    Fn, lib = F(), L.load()
    N = 384
    torch.manual_seed(11)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV)
    resid = torch.randn(M, N, device=DEV)
    call = torch.tensor([4], dtype=torch.int64, device=DEV)
    outs = []
    try:
        for n96 in (1, 0):
            L.check(lib.cg_set_tuning(b"gemm_n96", n96))
            o = torch.full((M, N), float("nan"), device=DEV)
            kw = dict(dropout_p=0.2, seed=5, rng_call=call, site=3) if kind == "bias_drop_resid" else {}
            Fn.linear_fwd(x, w, o, kind, bias=bias, resid=resid, **kw)
            outs.append(o)
    finally:
        L.check(lib.cg_set_tuning(b"gemm_n96", 1))
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0], outs[1])
    ref = (x.double() @ w.double().t() + bias.double())
    if kind == "bias_resid":
        assert relerr(outs[0], ref + resid.double()) < 1e-5


@pytest.mark.parametrize("kind", ["bias_resid", "bias_drop_resid"])
@pytest.mark.parametrize("inplace", [False, True])
def test_gemm_p8_residual_epilogue_matches_128x128_bitwise(kind, inplace):
    """The 256x256 kernel's fp32 residual epilogue (gemm_p8.hip P8_RESID: the C4 projection and FFN2
    forwards, GPT1.py:136,145-147; residual loaded per 32-row half band before its stores, dropout
    bits from drop_nibbles_rows) against the 128x128 persistent kernel on the same operands: the
    same K order per output element and the same bias -> dropout -> residual order, so equal bit for
    bit -- also when the output overwrites the residual in place (x += ...)."""
    from replicatinggpt_amd import _lib as L
    Fn, lib = F(), L.load()
    M, N, K = 1024, 768, 640
    torch.manual_seed(13)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV)
    resid = torch.randn(M, N, device=DEV)
    outs = []
    try:
        for v in (24, 9):
            L.check(lib.cg_set_tuning(b"gemm_variant", v))
            call = torch.tensor([4], dtype=torch.int64, device=DEV)
            o = resid.clone() if inplace else torch.full((M, N), float("nan"), device=DEV)
            r = o if inplace else resid
            kw = dict(dropout_p=0.2, seed=5, rng_call=call, site=3) if kind == "bias_drop_resid" else {}
            Fn.linear_fwd(x, w, o, kind, bias=bias, resid=r, **kw)
            outs.append(o)
    finally:
        L.check(lib.cg_set_tuning(b"gemm_variant", 0))
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0], outs[1])
    ref = x.double() @ w.double().t() + bias.double()
    if kind == "bias_resid":
        assert relerr(outs[0], ref + resid.double()) < 1e-5
    else:
        keep = philox.keep_mask(5, (4 << 8) | 3, np.arange(M * N), 0.2).reshape(M, N)
        want = resid.double() + torch.from_numpy(keep).to(DEV).double() * ref * float(np.float32(1 / 0.8))
        assert relerr(outs[0], want) < 1e-5

# every 256x256 (8-wave) variant in the loaded library: the product's 24, and with the A/B build 20-26
_P8_FULL = ([20, 21, 22, 23, 24, 25, 26] if "_ab" in os.environ.get("CHARPT_LIB", "") else [24])


@pytest.mark.parametrize("variant", _P8_FULL)
@pytest.mark.parametrize("N,K,bt,kind", [(2304, 768, 0, "store"), (768, 3072, 0, "bias_resid"),
                                         (768, 2304, 1, "store")])
def test_gemm_256_variants_full_size(variant, N, K, bt, kind):
    """each 256x256 variant at the C4 row count (M = 65,536: the QKV forward,
    FFN2 forward with its fp32 residual epilogue and the QKV dgrad, GPT1.py:111-112,121,145) -- a
    size-dependent indexing fault (round 5's half-row-shift trial passed at M <= 8192 and faulted at
    its first M = 65,536 launch) fails here, not on the first real launch.  Bitwise against the
    128x128 persistent kernel (same K order per element), and against torch's fp32 GEMM on the GPU."""
    from replicatinggpt_amd import _lib as L
    Fn, lib = F(), L.load()
    if lib.cg_set_tuning(b"gemm_variant", variant) != 0:
        pytest.skip(f"gemm_variant {variant} is A/B-only (not in this library build)")
    L.check(lib.cg_set_tuning(b"gemm_variant", 0))
    M = 65536
    torch.manual_seed(17)
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(K, N, device=DEV) if bt else torch.randn(N, K, device=DEV)).mul_(K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device=DEV) if kind == "bias_resid" else None
    resid = torch.randn(M, N, device=DEV) if kind == "bias_resid" else None
    outs = []
    try:
        for v in (variant, 9):
            L.check(lib.cg_set_tuning(b"gemm_variant", v))
            f32 = kind == "bias_resid"
            o = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32 if f32 else torch.bfloat16)
            epi = Fn.EPI["bias_resid"] if f32 else 0
            ops().gemm(x, w, o, True, False, bool(bt), M, N, K, K, N if bt else K, N, epi, bias, resid, N if f32 else 0,
                       None, 0, 0.0, 0, None, 0, 0.0, 1, None)
            torch.cuda.synchronize()
            outs.append(o)
    finally:
        L.check(lib.cg_set_tuning(b"gemm_variant", 0))
    assert not torch.isnan(outs[0].float()).any()
    assert torch.equal(outs[0], outs[1])
    ref = x.float() @ (w.float() if bt else w.float().t())
    if kind == "bias_resid":
        ref = ref + bias + resid
    assert relerr(outs[0].float(), ref) < (1e-5 if kind == "bias_resid" else 8e-3)


@pytest.mark.parametrize("M,C,T", [(16384, 384, 256), (2048, 768, 128), (1024, 384, 64), (512, 128, 256)])
def test_gemm_store_rowdot(M, C, T):
    """CG_EPI_STORE_ROWDOT (the projection dgrad dO = dy W, GPT1.py:136, with the attention backward's
    delta = rowsum(dO * O) per head): dO bit-equal to the plain dgrad, delta within fp32 summation
    order of the fp64 row dots of the written bf16 dO and O."""
    from replicatinggpt_amd import _lib as L
    Fn, O = F(), ops()
    torch.manual_seed(17)
    dy = torch.randn(M, C, device=DEV).to(torch.bfloat16)
    w = (torch.randn(C, C, device=DEV) * C ** -0.5).to(torch.bfloat16)
    o = torch.randn(M, C, device=DEV).to(torch.bfloat16)
    assert O.gemm_rowdot_supported(M, C, C, C, C, C)
    ref = torch.full((M, C), float("nan"), device=DEV).to(torch.bfloat16)
    Fn.linear_dgrad(dy, w, ref)
    do = torch.full((M, C), float("nan"), device=DEV).to(torch.bfloat16)
    H, B = C // 64, M // T
    delta = torch.full((B, H, T), float("nan"), device=DEV)
    O.gemm_store_rowdot(dy, w, do, M, C, C, C, C, C, o, C, T, delta)
    torch.cuda.synchronize()
    assert torch.equal(do.view(torch.int16), ref.view(torch.int16))
    exp = (do.double() * o.double()).view(B, T, H, 64).sum(-1).permute(0, 2, 1)
    assert not torch.isnan(delta).any()
    err = (delta.double() - exp).abs().max().item()
    assert err <= 1e-5 * max(1.0, exp.abs().max().item()), err
    # outside the persistent kernel's shapes the call fails instead of silently skipping delta
    assert not O.gemm_rowdot_supported(1000, C, C, C, C, C)
    dy1, o1 = torch.zeros(1000, C, device=DEV, dtype=torch.bfloat16), torch.zeros(1000, C, device=DEV, dtype=torch.bfloat16)
    do1 = torch.empty(1000, C, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROWDOT"):
        O.gemm_store_rowdot(dy1, w, do1, 1000, C, C, C, C, C, o1, C, 200, delta)


@pytest.mark.parametrize("T", [256, 192, 128, 64])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attention_bwd_precomputed_delta(T, p):
    """cg_attn_bwd_delta: the merged resident backward reading delta instead of loading O.  Given the
    delta the dQ kernel itself computes (the two-launch variant leaves it in the workspace), dQ / dK /
    dV equal the default launch's bit for bit; given the projection dgrad's delta
    (gemm_store_rowdot, another fp32 summation order) they agree to bf16 rounding."""
    from replicatinggpt_amd import _lib as L
    O, lib = ops(), L.load()
    B, H, D = 4, 6, 64   # B T % 128 == 0: the dO GEMM's persistent tiles
    torch.manual_seed(90 + T)
    d = H * D
    qkv = (torch.randn(B * T, 3 * d) * 0.7).to(torch.bfloat16).to(DEV)
    dout = torch.randn(B * T, d).to(torch.bfloat16).to(DEV)
    call = torch.tensor([5], dtype=torch.int64, device=DEV)
    scale = (3.0 * D) ** -0.5
    o = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
    lse, mask = F().attention_fwd(qkv, B, T, H, D, o, scale, p, 21, call, 4)
    nws = O.attn_bwd_workspace(B, T, H, D) // 4 + 1

    def bwd(delta=None):
        ws = torch.zeros(nws, device=DEV)
        dqkv = torch.full_like(qkv, float("nan"))
        O.attn_bwd(qkv, B, T, H, D, 0, d, 2 * d, qkv.stride(0), o, d, dout, d, lse, dqkv, 3 * d, scale, p, 21, call,
                   4, mask, ws, delta)
        return dqkv, ws

    base, _ = bwd()
    try:
        L.check(lib.cg_set_tuning(b"attn_variant", 2))
        two, ws = bwd()
    finally:
        L.check(lib.cg_set_tuning(b"attn_variant", 0))
    own = ws[:B * H * T].view(B, H, T).clone()
    din, _ = bwd(own)
    torch.cuda.synchronize()
    assert torch.equal(base.view(torch.int16), two.view(torch.int16))
    assert torch.equal(base.view(torch.int16), din.view(torch.int16))
    # delta from the dO GEMM's epilogue
    dy = torch.randn(B * T, d, device=DEV).to(torch.bfloat16)
    w = (torch.randn(d, d, device=DEV) * d ** -0.5).to(torch.bfloat16)
    do = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
    delta = torch.empty(B, H, T, device=DEV)
    O.gemm_store_rowdot(dy, w, do, B * T, d, d, d, d, d, o, d, T, delta)
    dout.copy_(do)
    ref, _ = bwd()
    got, _ = bwd(delta)
    torch.cuda.synchronize()
    assert not torch.isnan(got.float()).any()
    diff = (got.float() - ref.float()).abs().max().item()
    assert diff <= 2 ** -7 * ref.float().abs().max().item(), diff


def _attn_ref(q, k, v, scale, p=0.0, seed=0, stream=0):
    """q,k,v [B,T,H,D] float64; reference softmax attention with the oracle dropout mask."""
    B, T, H, D = q.shape
    s = torch.einsum("bthd,bshd->bhts", q, k) * scale
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    s = s.masked_fill(~mask, float("-inf"))
    P = torch.softmax(s, dim=-1)
    if p > 0:
        idx = np.arange(B * H * T * T, dtype=np.uint64).reshape(B, H, T, T)
        keep = torch.from_numpy(philox.keep_mask(seed, stream, idx, p)).double()
        P = P * keep * float(np.float32(1 / (1 - p)))
    return torch.einsum("bhts,bshd->bthd", P, v)


@pytest.mark.parametrize("B,T,H,D", [(2, 37, 3, 21), (2, 64, 2, 64), (1, 256, 2, 64), (2, 96, 1, 8)])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_attention_fwd_bwd(B, T, H, D, p, dt):
    Fn = F()
    torch.manual_seed(4)
    d = H * D
    qkv = (torch.randn(B * T, 3 * d) * 0.7).to(dt)
    scale = (3.0 * D) ** -0.5
    q = qkv[:, :d].double().view(B, T, H, D).requires_grad_(True)
    k = qkv[:, d:2 * d].double().view(B, T, H, D).requires_grad_(True)
    v = qkv[:, 2 * d:].double().view(B, T, H, D).requires_grad_(True)
    call = torch.tensor([2], dtype=torch.int64, device=DEV)
    ref = _attn_ref(q, k, v, scale, p, 11, (2 << 8) | 7)
    dout = torch.randn(B, T, H, D).to(dt)
    ref.backward(dout.double())
    qkv_d = qkv.to(DEV)
    o = torch.empty(B * T, d, dtype=dt, device=DEV)
    lse, mask = Fn.attention_fwd(qkv_d, B, T, H, D, o, scale, p, 11, call, 7)
    if dt == torch.float32:
        assert relerr(o, ref.reshape(B * T, d)) < 1e-5
    else:   # the bf16 bar element by element (conftest.bf16_close), as for dq / dk / dv below
        ok, st = bf16_close(o, ref.reshape(B * T, d))
        assert ok, ("o", st)
    dqkv = Fn.attention_bwd(qkv_d, B, T, H, D, o, dout.reshape(B * T, d).to(DEV), lse, scale, p, 11, call, 7, mask)
    dq, dk, dv = dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:]
    if dt == torch.float32:
        assert relerr(dq, q.grad.reshape(B * T, d)) < 1e-5
        assert relerr(dk, k.grad.reshape(B * T, d)) < 1e-5
        assert relerr(dv, v.grad.reshape(B * T, d)) < 1e-5
    else:
        for name, got, t in (("dq", dq, q), ("dk", dk, k), ("dv", dv, v)):
            ok, st = bf16_close(got, t.grad.reshape(B * T, d))
            assert ok, (name, st)


@pytest.mark.parametrize("B,T,H,D", [(256, 256, 6, 21), (2, 37, 3, 21), (3, 200, 2, 8), (2, 256, 2, 32),
                                     (1, 130, 4, 16), (2, 16, 1, 21)])
def test_attention_fp32_resident_matches_query_blocks(B, T, H, D):
    """The sequence-resident fp32 MFMA forward (k_attn_fwd_f32res, T <= 256: the generate() window at
    C5, 256 x 256 x 6 heads of 21) gives the 64-query-block kernel's bits (attn_variant 1) for O and
    lse, and fp64 within 1e-5."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    Fn = F()
    torch.manual_seed(8)
    d = H * D
    qkv = (torch.randn(B * T, 3 * d) * 0.7).to(DEV)
    scale = (3.0 * D) ** -0.5
    outs = []
    for v in (1, 0):
        L.check(lib.cg_set_tuning(b"attn_variant", v))
        try:
            o = torch.full((B * T, d), float("nan"), device=DEV)
            lse, _ = Fn.attention_fwd(qkv, B, T, H, D, o, scale, 0.0, 0, None, 0)
            torch.cuda.synchronize()
        finally:
            L.check(lib.cg_set_tuning(b"attn_variant", 0))
        outs.append((o, lse.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    if B * T <= 4096:
        qd = qkv.double().cpu()
        q, k, v = (qd[:, i * d:(i + 1) * d].view(B, T, H, D) for i in range(3))
        ref = _attn_ref(q, k, v, scale, 0.0, 0, 0)
        assert relerr(outs[1][0], ref.reshape(B * T, d)) < 1e-5


def test_attention_fast_matches_generic_bf16():
    """The MFMA head_size-64 kernels against the generic kernels on identical bf16 inputs."""
    Fn = F()
    B, T, H, D = 2, 256, 3, 64
    torch.manual_seed(5)
    d = H * D
    qkv = (torch.randn(B * T, 3 * d)).to(torch.bfloat16).to(DEV)
    call = torch.tensor([1], dtype=torch.int64, device=DEV)
    o_fast = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
    lse_fast = Fn.attention_fwd(qkv, B, T, H, D, o_fast, 0.05, 0.2, 3, call, 1)
    # generic path: a non-16B-aligned leading dimension forces it
    wide = torch.zeros(B * T, 3 * d + 4, dtype=torch.bfloat16, device=DEV)
    wide[:, :3 * d] = qkv
    view = wide[:, :3 * d]
    o_gen = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=DEV)
    ops().attn_fwd(view, B, T, H, D, 0, d, 2 * d, view.stride(0), o_gen, d, lse, 0.05, 0.2, 3, call, 1, None)
    assert relerr(o_fast, o_gen) < 2e-2
    # the bf16 kernels' row sums run on the matrix core over the bf16-rounded weights O is built from
    # (each within 2^-8 relative), so |lse - ref| <= ln(1 + 2^-8) < 2^-8 per row
    assert float((lse_fast[0].double().cpu() - lse.double().cpu()).abs().max()) < 2.0 ** -8


@pytest.mark.parametrize("T", [64, 128, 192, 320, 512])
def test_attention_fast_block_shapes(T):
    """The 32x32x16 MFMA kernels at sequence lengths that leave the 256-query (forward / dQ) and
    128-key (dK/dV) blocks partially filled, several 64-key tiles per block, and the causal group
    pairing (g, 7-g), with dropout, against the fp64 reference with the oracle's keep mask."""
    Fn = F()
    B, H, D, p = 2, 3, 64, 0.2
    torch.manual_seed(6 + T)
    d = H * D
    qkv = (torch.randn(B * T, 3 * d) * 0.7).to(torch.bfloat16)
    q = qkv[:, :d].double().view(B, T, H, D).requires_grad_(True)
    k = qkv[:, d:2 * d].double().view(B, T, H, D).requires_grad_(True)
    v = qkv[:, 2 * d:].double().view(B, T, H, D).requires_grad_(True)
    scale = (3.0 * D) ** -0.5
    ref = _attn_ref(q, k, v, scale, p, 21, (3 << 8) | 4)
    dout = torch.randn(B, T, H, D).to(torch.bfloat16)
    ref.backward(dout.double())
    call = torch.tensor([3], dtype=torch.int64, device=DEV)
    qkv_d = qkv.to(DEV)
    o = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
    lse, mask = Fn.attention_fwd(qkv_d, B, T, H, D, o, scale, p, 21, call, 4)
    dqkv = Fn.attention_bwd(qkv_d, B, T, H, D, o, dout.reshape(B * T, d).to(DEV), lse, scale, p, 21, call, 4, mask)
    torch.cuda.synchronize()
    assert relerr(o, ref.reshape(B * T, d)) < 2e-2
    for i, t in enumerate((q, k, v)):
        ok, st = bf16_close(dqkv[:, i * d:(i + 1) * d], t.grad.reshape(B * T, d))
        assert ok, ("qkv"[i], T, st)


@pytest.mark.parametrize("T", [256, 128, 64])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attention_resident_kernels_match_ring_kernels(T, p):
    """T <= 256 runs the sequence-resident kernels (forward; dQ and dK/dV merged into one launch
    that computes delta itself).  Same per-tile arithmetic as the ring kernels (attn_variant 1)
    and the two-launch resident backward (attn_variant 2): all three give identical bits."""
    from replicatinggpt_amd import _lib as L
    Fn = F()
    lib = L.load()
    B, H, D = 3, 6, 64
    torch.manual_seed(40 + T)
    d = H * D
    qkv = (torch.randn(B * T, 3 * d) * 0.7).to(torch.bfloat16).to(DEV)
    dout = torch.randn(B * T, d).to(torch.bfloat16).to(DEV)
    call = torch.tensor([5], dtype=torch.int64, device=DEV)
    scale = (3.0 * D) ** -0.5
    outs = []
    try:
        for variant in (0, 1, 2):
            L.check(lib.cg_set_tuning(b"attn_variant", variant))
            o = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
            lse, mask = Fn.attention_fwd(qkv, B, T, H, D, o, scale, p, 21, call, 4)
            dqkv = Fn.attention_bwd(qkv, B, T, H, D, o, dout, lse, scale, p, 21, call, 4, mask)
            torch.cuda.synchronize()
            outs.append((o.cpu(), lse.cpu(), dqkv.cpu()))
    finally:
        L.check(lib.cg_set_tuning(b"attn_variant", 0))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("T", [1024, 576, 320])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attention_forward_ring_variants_identical(T, p):
    """T > 256 forward rings: the default LDS-DMA ring (Q fragments in registers, 4 slots, two tiles
    ahead), attn_variant 6 (Q image in LDS, 3 slots, one tile ahead) and attn_variant 5 (the
    register-staged ring) run the same per-tile arithmetic: identical o and lse bits (the A/B build
    runs all three; the product library the default against itself).  T = 576 / 320
    leave the last 256-query block partly empty (inactive query groups, short rings)."""
    from replicatinggpt_amd import _lib as L
    Fn = F()
    lib = L.load()
    B, H, D = 2, 3, 64
    torch.manual_seed(70 + T)
    d = H * D
    qkv = (torch.randn(B * T, 3 * d) * 0.7).to(torch.bfloat16).to(DEV)
    call = torch.tensor([3], dtype=torch.int64, device=DEV)
    scale = (3.0 * D) ** -0.5
    outs = []
    try:
        for variant in (0, 6, 5):   # 5 / 6: A/B build only (CHARPT_LIB=...libcharpt_hip_ab.so)
            if lib.cg_set_tuning(b"attn_variant", variant) != 0:
                continue
            o = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
            lse, _ = Fn.attention_fwd(qkv, B, T, H, D, o, scale, p, 21, call, 4)
            torch.cuda.synchronize()
            outs.append((o.cpu(), lse.cpu()))
    finally:
        L.check(lib.cg_set_tuning(b"attn_variant", 0))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


def test_attention_forward_rescale_branch():
    """The forward's lazy rescale (running max moved only when a tile's max exceeds it by 2^8) with
    inputs that force it: one key row spiked against every query so that the max jumps at a late
    tile, plus a query row whose scores all collapse to a huge common value.  fp64 reference."""
    Fn = F()
    B, T, H, D = 1, 512, 2, 64
    torch.manual_seed(31)
    d = H * D
    qkv = torch.randn(B * T, 3 * d) * 0.5
    qkv[:, :d] += 2.0                    # queries share a direction ...
    qkv[300, d:2 * d] = 8.0              # ... that key 300 (tile 4) matches strongly
    qkv[:, d:2 * d][:, :D] *= torch.linspace(0.1, 3.0, T)[:, None]   # growing key norms: the max climbs tile by tile
    qkv = qkv.to(torch.bfloat16)
    q = qkv[:, :d].double().view(B, T, H, D)
    k = qkv[:, d:2 * d].double().view(B, T, H, D)
    v = qkv[:, 2 * d:].double().view(B, T, H, D)
    scale = D ** -0.5
    ref = _attn_ref(q, k, v, scale)
    o = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
    lse, _ = Fn.attention_fwd(qkv.to(DEV), B, T, H, D, o, scale, 0.0, 0, None, 0)
    torch.cuda.synchronize()
    assert relerr(o, ref.reshape(B * T, d)) < 2e-2
    s = torch.einsum("bthd,bshd->bhts", q, k) * scale
    s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
    # the bf16 kernels' row sums run on the matrix core over the bf16-rounded weights O is built from
    # (each within 2^-8 relative), so |lse - ref| <= ln(1 + 2^-8) < 2^-8 per row
    assert float((lse.double().cpu() - torch.logsumexp(s, -1).double().cpu()).abs().max()) < 2.0 ** -8


def test_attention_bwd_regenerates_mask():
    """cg_attn_bwd with mask=NULL regenerates the forward's keep bits: identical gradients."""
    Fn = F()
    B, T, H, D = 2, 128, 2, 64
    torch.manual_seed(9)
    d = H * D
    qkv = torch.randn(B * T, 3 * d).to(torch.bfloat16).to(DEV)
    call = torch.tensor([4], dtype=torch.int64, device=DEV)
    o = torch.empty(B * T, d, dtype=torch.bfloat16, device=DEV)
    lse, mask = Fn.attention_fwd(qkv, B, T, H, D, o, 0.1, 0.2, 5, call, 2)
    assert mask is not None
    do = torch.randn(B * T, d).to(torch.bfloat16).to(DEV)
    g1 = Fn.attention_bwd(qkv, B, T, H, D, o, do, lse, 0.1, 0.2, 5, call, 2, mask)
    g2 = Fn.attention_bwd(qkv, B, T, H, D, o, do, lse, 0.1, 0.2, 5, call, 2, None)
    assert torch.equal(g1, g2)


@pytest.mark.parametrize("V,T,C,B", [(65, 40, 126, 3), (65, 256, 126, 7), (65, 9, 21, 2), (65, 256, 384, 64), (65, 100, 200, 5), (200, 64, 128, 4),
                                     (600, 64, 96, 3), (65, 64, 384, 16), (65, 32, 192, 128), (65, 1024, 768, 64)])
def test_embedding_fwd_bwd(V, T, C, B):
    """Token + position embeddings and their deterministic backward (the token gradient's 4-wave
    partial histograms, added in wave then chunk order) against fp64, ragged and C2-sized; larger
    vocabularies take the 2- and 1-wave histogram blocks (V 200, 600).  B = 64 / 16 / 128 take the
    fused pass (both gradients from one read of dx, 2 / 8 / 1 positions per chunk)."""
    Fn = F()
    torch.manual_seed(6)
    wte = torch.randn(V, C)
    wpe = torch.randn(max(64, T), C)
    idx = torch.randint(0, V, (B, T))
    x = torch.empty(B, T, C, device=DEV)
    ops().embed_fwd(idx.to(DEV), wte.to(DEV), wpe.to(DEV), x)
    ref = wte[idx] + wpe[:T]
    assert torch.equal(x.cpu(), ref)   # one fp32 add per element
    dx = torch.randn(B, T, C)
    dwte = torch.empty(V, C, device=DEV)
    dwpe = torch.empty(max(64, T), C, device=DEV)
    ws = torch.empty(ops().embed_bwd_workspace(B, T, C, V) // 4 + 1, device=DEV)
    ops().embed_bwd(idx.to(DEV), dx.to(DEV), dwte, dwpe[:T], False, ws)
    want_te = torch.zeros(V, C, dtype=torch.float64).index_add_(0, idx.reshape(-1), dx.reshape(-1, C).double())
    assert relerr(dwte, want_te) < 2e-6
    assert relerr(dwpe[:T], dx.double().sum(0)) < 2e-6


def test_cross_entropy():
    M, V = 300, 65
    torch.manual_seed(7)
    logits = torch.randn(M, V) * 3
    tgt = torch.randint(0, V, (M,))
    lr = logits.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lr, tgt)
    loss.backward()
    ld, td = logits.to(DEV), tgt.to(DEV)
    rows = torch.empty(M, device=DEV)
    lse = torch.empty(M, device=DEV)
    ops().ce_fwd(ld, td, rows, lse)
    out = torch.empty((), device=DEV)
    ops().sum_scaled(rows, 1.0 / M, out, torch.empty(1024, device=DEV))
    assert abs(float(out) - float(loss)) < 1e-5
    dl = torch.empty(M, V, device=DEV)
    ops().ce_bwd(ld, td, lse, torch.ones(1, device=DEV), 1.0 / M, dl, None)
    assert relerr(dl, lr.grad) < 1e-5


@pytest.mark.parametrize("M,C,V", [(256, 384, 65), (1024, 128, 65), (64, 96, 16), (128, 64, 128)])
def test_head_fused(M, C, V):
    """cg_head_fwd/bwd (bf16 LM head + cross entropy, csrc/head.hip) against torch fp64 on the same
    bf16-rounded operands: logits/lse/loss/dlogits/dbias at the bf16 bar (2e-2)."""
    torch.manual_seed(11)
    a = torch.randn(M, C).to(torch.bfloat16)
    W = (torch.randn(V, C) / math.sqrt(C)).to(torch.bfloat16)
    b = torch.randn(V)
    tgt = torch.randint(0, V, (M,))
    KP = 128
    wpad = torch.zeros(KP, C, dtype=torch.bfloat16)
    wpad[:V] = W
    lg = (a.double() @ W.double().t() + b.double()).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lg, tgt)
    loss.backward()
    logits = torch.empty(M, V, device=DEV)
    lse = torch.empty(M, device=DEV)
    out = torch.empty((), device=DEV)
    ws = torch.empty(ops().head_workspace(M, V) // 4, device=DEV)
    ops().head_fwd(a.to(DEV), wpad.to(DEV), b.to(DEV), tgt.to(DEV), logits, lse, out, ws)
    assert relerr(logits, lg) < 1e-5      # same bf16 operands, fp32 accumulate
    assert relerr(lse, torch.logsumexp(lg.detach(), 1)) < 1e-5
    assert abs(float(out) - float(loss)) < 1e-4 * max(1.0, abs(float(loss)))
    dl = torch.empty(M, KP, dtype=torch.bfloat16, device=DEV)
    db = torch.full((V,), 0.5, device=DEV)
    ops().head_bwd(logits, lse, tgt.to(DEV), torch.full((1,), 2.0, device=DEV), 1.0 / M, None, dl, db, True, ws)
    want = 2.0 * lg.grad
    assert relerr(dl[:, :V], want) < 2e-2
    if V < KP:
        assert float(dl[:, V:].float().abs().max()) == 0.0
    assert relerr(db, 0.5 + want.sum(0)) < 1e-5
    # logits-only forward (generate path) and logits-gradient backward
    logits2 = torch.empty(M, V, device=DEV)
    ops().head_fwd(a.to(DEV), wpad.to(DEV), b.to(DEV), None, logits2, lse, None, None)
    assert torch.equal(logits2, logits)
    gl = torch.randn(M, V)
    ops().head_bwd(logits, lse, None, None, 1.0 / M, gl.to(DEV), dl, None, False, ws)
    assert relerr(dl[:, :V], gl) < 1e-2


@pytest.mark.parametrize("at,bt", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K,split", [(300, 126, 126, 1), (257, 378, 504, 1), (126, 504, 1000, 4), (64, 65, 33, 1)])
def test_gemm_f32_mfma_matches_generic(at, bt, M, N, K, split):
    """fp32 MFMA GEMM (exact path) against torch fp64 and the generic fp32 kernel, odd sizes, all
    layouts, split-K, bias+relu epilogue."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    torch.manual_seed(12)
    A = torch.randn(K, M) if at else torch.randn(M, K)
    B = torch.randn(K, N) if bt else torch.randn(N, K)
    bias = torch.randn(N)
    ref = torch.relu(_ref_gemm(A, B, at, bt) + bias.double())
    outs = []
    for v in (0, 99):
        L.check(lib.cg_set_tuning(b"gemm_variant", v))
        try:
            out = torch.empty(M, N, device=DEV)
            ws = torch.empty(max(1, ops().gemm_workspace(M, N, split) // 4), device=DEV)
            if split > 1:
                ops().gemm(A.to(DEV), B.to(DEV), out, False, bool(at), bool(bt), M, N, K, A.shape[1], B.shape[1], N,
                           0, None, None, 0, None, 0, 0.0, 0, None, 0, 0.0, split, ws)
                out = torch.relu(out + bias.to(DEV))
            else:
                ops().gemm(A.to(DEV), B.to(DEV), out, False, bool(at), bool(bt), M, N, K, A.shape[1], B.shape[1], N,
                           2, bias.to(DEV), None, 0, None, 0, 0.0, 0, None, 0, 0.0, 1, None)
            torch.cuda.synchronize()
        finally:
            L.check(lib.cg_set_tuning(b"gemm_variant", 0))
        outs.append(out)
        assert relerr(out, ref) < 1e-5


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("M,N,K", [(256, 378, 126), (256, 126, 504), (256, 65, 126), (1, 504, 126), (33, 70, 5),
                                   (2048, 126, 200), (100, 33, 257), (70, 90, 624), (64, 64, 2), (31, 17, 640)])
def test_gemm_f32_small_m_matches_128x64_bitwise(kind, M, N, K):
    """The small-M fp32 forward kernels (M <= 2048: k_gemm_f32r with the K slab in LDS for even K <= 624,
    else k_gemm_f32s; gemm_variant 97 forces k_gemm_f32s) against k_gemm_f32 (gemm_variant 98): same
    MFMA lane / k order and padded depth, same epilogue arithmetic -> bitwise equal."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    torch.manual_seed(31)
    A = torch.randn(M, K, device=DEV)
    B = torch.randn(N, K, device=DEV)
    bias = torch.randn(N, device=DEV)
    resid = torch.randn(M, N, device=DEV)
    outs = []
    for v in (98, 97, 0):
        L.check(lib.cg_set_tuning(b"gemm_variant", v))
        try:
            out = torch.full((M, N), float("nan"), device=DEV)
            ops().gemm(A, B, out, False, False, False, M, N, K, K, K, N, kind, bias if kind else None,
                       resid if kind == 3 else None, N if kind == 3 else 0, None, 0, 0.0, 0, None, 0, 0.0, 1, None)
            torch.cuda.synchronize()
        finally:
            L.check(lib.cg_set_tuning(b"gemm_variant", 0))
        outs.append(out)
    ref = A.double().cpu() @ B.double().cpu().T
    if kind:
        ref = ref + bias.double().cpu()
    if kind == 2:
        ref = torch.relu(ref)
    if kind == 3:
        ref = ref + resid.double().cpu()
    assert relerr(outs[2], ref) < 1e-5
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32))


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("M,N,K,variant", [(65536, 378, 126, 0), (65536, 504, 126, 0), (65536, 126, 126, 0),
                                           (65536, 126, 504, 0), (4129, 70, 200, 0), (2049, 129, 34, 0),
                                           (256, 378, 126, 96), (33, 70, 6, 96), (300, 65, 48, 96), (130, 257, 2, 96),
                                           (4097, 126, 624, 0)])
def test_gemm_f32_persistent_matches_128x64_bitwise(kind, M, N, K, variant):
    """The persistent fp32 forward kernel (k_gemm_f32p: M > 2048 by default, gemm_variant 96 at any M;
    v_mfma_f32_32x32x2_f32 over 32-deep steps) against k_gemm_f32 (gemm_variant 98, 16x16x4 over 16-deep
    steps): both k-ordered f32 fma chains over the same zero-padded depth, same epilogue -> bitwise equal,
    at generate()'s window shapes (M = 65536), ragged M / N, K with a half-used last 32-deep step."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    torch.manual_seed(41)
    A = torch.randn(M, K, device=DEV)
    B = torch.randn(N, K, device=DEV)
    bias = torch.randn(N, device=DEV)
    resid = torch.randn(M, N, device=DEV)
    outs = []
    for v in (98, variant):
        L.check(lib.cg_set_tuning(b"gemm_variant", v))
        try:
            out = torch.full((M, N), float("nan"), device=DEV)
            ops().gemm(A, B, out, False, False, False, M, N, K, K, K, N, kind, bias if kind else None,
                       resid if kind == 3 else None, N if kind == 3 else 0, None, 0, 0.0, 0, None, 0, 0.0, 1, None)
            torch.cuda.synchronize()
        finally:
            L.check(lib.cg_set_tuning(b"gemm_variant", 0))
        outs.append(out)
    rows = slice(0, min(M, 2048))   # fp64 reference on a row sample
    ref = A[rows].double().cpu() @ B.double().cpu().T
    if kind:
        ref = ref + bias.double().cpu()
    if kind == 2:
        ref = torch.relu(ref)
    if kind == 3:
        ref = ref + resid[rows].double().cpu()
    assert relerr(outs[1][rows], ref) < 1e-5
    assert not torch.isnan(outs[1]).any()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("M,C,H,variant", [(65536, 126, 504, 0), (65536, 126, 504, 98), (4129, 126, 504, 0),
                                           (300, 64, 256, 98), (2049, 128, 2048, 0), (1000, 126, 130, 98),
                                           (777, 100, 66, 0), (129, 2, 6, 98), (64, 6, 34, 0)])
def test_ffn_f32_fused_matches_two_gemms(M, C, H, variant, ln):
    """The fused inference FFN (k_ffn_f32: h in registers, never in memory; with ln, the block's ln2
    computed in the launch with k_ln_fwd's row body) against what it replaces -- [layernorm_fwd,]
    bias_relu GEMM into an [M, H] buffer, bias_resid GEMM -- under the default dispatch (k_gemm_f32p
    above 2048 rows) and k_gemm_f32 (gemm_variant 98): bitwise equal, and within fp32 rounding of an
    fp64 reference; ragged M, C below 16 / not a multiple of 16, H not a multiple of 32."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    torch.manual_seed(43)
    x = torch.randn(M, C, device=DEV)
    w1 = torch.randn(H, C, device=DEV) / C ** 0.5
    b1 = torch.randn(H, device=DEV) * 0.1
    w2 = torch.randn(C, H, device=DEV) / H ** 0.5
    b2 = torch.randn(C, device=DEV) * 0.1
    resid = torch.randn(M, C, device=DEV)
    lw = 1.0 + 0.1 * torch.randn(C, device=DEV)
    lb = 0.1 * torch.randn(C, device=DEV)
    assert ops().ffn_fwd_f32_supported(M, C, H)
    out = torch.full((M, C), float("nan"), device=DEV)
    ops().ffn_fwd_f32(x, lw if ln else None, lb if ln else None, 1e-5, w1, b1, w2, b2, resid, out)
    if ln:
        a = torch.full((M, C), float("nan"), device=DEV)
        ops().layernorm_fwd(x, lw, lb, a, torch.empty(M, device=DEV), torch.empty(M, device=DEV), 1e-5)
    else:
        a = x
    L.check(lib.cg_set_tuning(b"gemm_variant", variant))
    try:
        h = torch.full((M, H), float("nan"), device=DEV)
        ops().gemm(a, w1, h, False, False, False, M, H, C, C, C, H, 2, b1, None, 0, None, 0, 0.0, 0, None, 0, 0.0, 1,
                   None)
        ref2 = torch.full((M, C), float("nan"), device=DEV)
        ops().gemm(h, w2, ref2, False, False, False, M, C, H, H, H, C, 3, b2, resid, C, None, 0, 0.0, 0, None, 0, 0.0,
                   1, None)
        torch.cuda.synchronize()
    finally:
        L.check(lib.cg_set_tuning(b"gemm_variant", 0))
    assert not torch.isnan(out).any()
    assert torch.equal(out.view(torch.int32), ref2.view(torch.int32))
    rows = slice(0, min(M, 2048))
    ad = x[rows].double().cpu()
    if ln:
        ad = torch.nn.functional.layer_norm(ad, (C,), lw.double().cpu(), lb.double().cpu(), 1e-5)
    hd = torch.relu(ad @ w1.double().cpu().T + b1.double().cpu())
    ref = resid[rows].double().cpu() + hd @ w2.double().cpu().T + b2.double().cpu()
    assert relerr(out[rows], ref) < 1e-5


@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("M,N,K,variant", [(65536, 378, 126, 0), (65536, 126, 126, 98), (4129, 70, 128, 0),
                                           (300, 2, 2, 98), (2049, 2048, 64, 0), (777, 130, 100, 98),
                                           (256, 378, 126, 98), (256, 504, 126, 0), (256, 65, 126, 98),
                                           (1, 65, 126, 0), (2048, 17, 6, 98)])
def test_linear_rows_f32_matches_gemm(M, N, K, variant, kind, ln):
    """The row-resident fp32 Linear (above 2048 rows k_linear_f32q / k_linear_f32t: the wave's rows in
    registers, W streamed in column slices; up to 2048 rows -- generate()'s per-token steps --
    k_gemm_f32r with the A slab in LDS, any N; with ln, the LayerNorm before it in the launch) against
    [layernorm_fwd +] the fp32 GEMM with the same epilogue (store / bias / bias_relu / bias_resid) under
    the default dispatch and k_gemm_f32 (gemm_variant 98): bitwise equal, and within fp32 rounding of
    fp64."""
    from replicatinggpt_amd import _lib as L
    lib = L.load()
    torch.manual_seed(45)
    x = torch.randn(M, K, device=DEV)
    w = torch.randn(N, K, device=DEV) / K ** 0.5
    bias = torch.randn(N, device=DEV) if kind else None
    resid = torch.randn(M, N, device=DEV) if kind == 3 else None
    lw = 1.0 + 0.1 * torch.randn(K, device=DEV)
    lb = 0.1 * torch.randn(K, device=DEV)
    assert ops().linear_rows_f32_supported(M, N, K)
    outs = []
    for nb in (2, 1, 0):   # cg_set_tuning "linear_rows_nb": 32-row waves with 2 / 1 column blocks per slice, 0 (default) 16-row waves
        L.check(lib.cg_set_tuning(b"linear_rows_nb", nb))
        try:
            o = torch.full((M, N), float("nan"), device=DEV)
            ops().linear_rows_f32(x, lw if ln else None, lb if ln else None, 1e-5, w, bias, resid, o, kind == 2)
            torch.cuda.synchronize()
        finally:
            L.check(lib.cg_set_tuning(b"linear_rows_nb", 0))
        outs.append(o)
    assert torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32))
    assert torch.equal(outs[1].view(torch.int32), outs[2].view(torch.int32))
    out = outs[2]
    if ln:
        a = torch.full((M, K), float("nan"), device=DEV)
        ops().layernorm_fwd(x, lw, lb, a, torch.empty(M, device=DEV), torch.empty(M, device=DEV), 1e-5)
    else:
        a = x
    L.check(lib.cg_set_tuning(b"gemm_variant", variant))
    try:
        ref2 = torch.full((M, N), float("nan"), device=DEV)
        ops().gemm(a, w, ref2, False, False, False, M, N, K, K, K, N, kind, bias, resid, N if kind == 3 else 0, None,
                   0, 0.0, 0, None, 0, 0.0, 1, None)
        torch.cuda.synchronize()
    finally:
        L.check(lib.cg_set_tuning(b"gemm_variant", 0))
    assert not torch.isnan(out).any()
    assert torch.equal(out.view(torch.int32), ref2.view(torch.int32))
    rows = slice(0, min(M, 2048))
    ad = x[rows].double().cpu()
    if ln:
        ad = torch.nn.functional.layer_norm(ad, (K,), lw.double().cpu(), lb.double().cpu(), 1e-5)
    ref = ad @ w.double().cpu().T
    if kind:
        ref = ref + bias.double().cpu()
    if kind == 2:
        ref = torch.relu(ref)
    if kind == 3:
        ref = ref + resid[rows].double().cpu()
    assert relerr(out[rows], ref) < 1e-5


def test_ffn_f32_fused_in_place_and_unsupported():
    """out may alias resid (the residual stream updated in place); unsupported shapes fail loudly."""
    from replicatinggpt_amd import _lib as L
    torch.manual_seed(44)
    M, C, H = 3000, 126, 504
    a = torch.randn(M, C, device=DEV)
    w1 = torch.randn(H, C, device=DEV) / C ** 0.5
    b1 = torch.randn(H, device=DEV)
    w2 = torch.randn(C, H, device=DEV) / H ** 0.5
    b2 = torch.randn(C, device=DEV)
    x = torch.randn(M, C, device=DEV)
    out = torch.empty_like(x)
    ops().ffn_fwd_f32(a, None, None, 0.0, w1, b1, w2, b2, x, out)
    lib = L.load()
    L.check(lib.cg_ffn_fwd_f32(M, C, H, L.ptr(a), C, None, None, 0.0, L.ptr(w1), C, L.ptr(b1), L.ptr(w2), H,
                               L.ptr(b2), L.ptr(x), C, L.ptr(x), C, L.stream_ptr(x.device)))
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), out.view(torch.int32))
    assert not ops().ffn_fwd_f32_supported(M, 130, H) and not ops().ffn_fwd_f32_supported(M, 127, H)
    assert lib.cg_ffn_fwd_f32(M, 130, H, L.ptr(a), C, None, None, 0.0, L.ptr(w1), C, L.ptr(b1), L.ptr(w2), H,
                              L.ptr(b2), L.ptr(x), C, L.ptr(x), C, L.stream_ptr(x.device)) != 0


def test_adamw_matches_torch():
    n = 1000
    torch.manual_seed(8)
    p = torch.randn(n)
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=2e-4)
    pd = p.clone().to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    sh = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for i in range(5):
        g = torch.randn(n)
        ref.grad = g.clone()
        opt.step()
        ops().counter_add(step, 1)
        ops().adamw(pd, g.to(DEV), m, v, sh, 2e-4, 0.9, 0.999, 1e-8, 1e-2, step)
    assert relerr(pd, ref.detach()) < 1e-6
    assert torch.equal(sh.cpu(), pd.cpu().to(torch.bfloat16))


def test_bf16_rounding_matches_torch():
    """Every bf16 the kernels write goes through gfx950's v_cvt_pk_bf16_f32 (csrc/common.h
    f2bf / pack_bf2): round-to-nearest-even, bit-identical to torch's float -> bfloat16 cast,
    including ties, denormals, overflow to inf and signed zeros."""
    torch.manual_seed(11)
    x = torch.randn(1 << 16) * torch.exp(torch.randn(1 << 16) * 8)
    ties = (torch.randint(0, 0x7f00, (4096,), dtype=torch.int32) << 16 | 0x8000).view(torch.float32)  # finite
    edge = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 3.4e38, -3.4e38, 1e-40, -1e-40, 1.17e-38,
                         2.0 ** -133, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    src = torch.cat([x, ties, edge]).contiguous()
    out = torch.empty(src.numel(), dtype=torch.bfloat16, device=DEV)
    ops().cast_bf16(src.to(DEV), out)
    torch.cuda.synchronize()
    got, want = out.cpu().view(torch.int16), src.to(torch.bfloat16).view(torch.int16)
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, [(float(src[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    nan = torch.full((64,), float("nan"))
    out = torch.empty(64, dtype=torch.bfloat16, device=DEV)
    ops().cast_bf16(nan.to(DEV), out)
    assert torch.isnan(out.cpu().float()).all()


def test_deferred_partial_reduces_match_immediate():
    """CG_DEFER (cg_reduce_rows_ex / cg_layernorm_bwd_reduce_ex): the reduce calls are queued and
    cg_flush_deferred runs them as one multi-job kernel -- the same per-job bits as the immediate
    launches, including a second job accumulating into the first job's output (queued jobs whose
    outputs it overlaps are flushed first) and an immediate reduce into a queued output."""
    import ctypes
    from replicatinggpt_amd import _lib as L
    O = ops()
    lib = L.load()
    torch.manual_seed(5)
    shapes = [(256, 1152), (256, 1536), (33, 70), (512, 384)]
    parts = [torch.randn(r, n, device=DEV) for r, n in shapes]
    extra = torch.randn(128, 1536, device=DEV)

    def run(defer):
        outs = [torch.full((n,), 0.5, device=DEV) for _, n in shapes]
        for p, o in zip(parts, outs):
            O.reduce_rows(p, p.shape[0], p.shape[1], o, False, defer)
        O.reduce_rows(extra, 128, 1536, outs[1], True, defer)         # accumulates onto a queued output
        ws = torch.empty(O.colsum_workspace(64, 384) // 4 + 1, device=DEV)
        O.colsum(extra[:64, :384].contiguous(), outs[3], True, ws)   # immediate reduce, queued target
        O.reduce_rows(parts[0], 256, 1152, outs[0], True, defer)
        L.check(lib.cg_flush_deferred(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return [o.cpu() for o in outs]

    ref, got = run(False), run(True)
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    want1 = parts[1].double().sum(0) + extra.double().sum(0)
    assert relerr(got[1], want1) < 1e-5






def test_adamw_rounding_is_explicit():
    """csrc/adamw.h adam_one rounds every step explicitly (contraction off, two __builtin_fmaf where
    torch's CPU kernels fuse: lerp and addcmul) -- so cg_adamw equals a numpy restatement of exactly
    those roundings bit for bit, whatever loop shape the compiler builds around it (VERDICT r4
    item 7: the GEMM-hosted AdamW jobs run the same function)."""
    f = np.float32
    n = 1 << 14
    rng = np.random.default_rng(3)
    P = rng.standard_normal(n).astype(f)
    M = (rng.standard_normal(n) * 0.01).astype(f)
    V = (rng.random(n) * 1e-3).astype(f)
    pd, md, vd = (torch.from_numpy(x.copy()).to(DEV) for x in (P, M, V))
    sh = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    lr, b1, b2, eps, wd = 3e-3, 0.9, 0.999, 1e-8, 1e-2
    for t in range(1, 4):
        G = rng.standard_normal(n).astype(f)
        ops().counter_add(step, 1)
        ops().adamw(pd, torch.from_numpy(G).to(DEV), md, vd, sh, lr, b1, b2, eps, wd, step)
        decay, w1, B2, omb2, E = f(1 - lr * wd), f(1 - b1), f(b2), f(1 - b2), f(eps)
        neg, bc2s = f(-(lr / (1 - b1 ** t))), f(math.sqrt(1 - b2 ** t))
        P = (P * decay).astype(f)
        M = _fma32(w1, (G - M).astype(f), M)
        V = _fma32((omb2 * G).astype(f), G, (V * B2).astype(f))
        den = ((np.sqrt(V).astype(f) / bc2s).astype(f) + E).astype(f)
        P = (P + ((neg * M).astype(f) / den).astype(f)).astype(f)
    torch.cuda.synchronize()
    assert np.array_equal(md.cpu().numpy(), M) and np.array_equal(vd.cpu().numpy(), V)
    assert np.array_equal(pd.cpu().numpy(), P)


@pytest.mark.parametrize("C", [126, 64])
def test_layernorm_fwd_narrow_row_paths_bitwise(C):
    """Narrow-row LayerNorm forward: the one-row-per-wave launch (< 8192 rows, generate()'s 256-row
    steps) and the 8-rows-per-wave launch (the decode window's 65536 rows) share ln_fwd_row -> the
    same bits for the same rows."""
    torch.manual_seed(C)
    x = torch.randn(65536, C, device=DEV) * 3 + 1
    w = torch.randn(C, device=DEV)
    b = torch.randn(C, device=DEV)
    outs = []
    for rows in (65536, 256, 8191, 1):
        y = torch.empty(rows, C, device=DEV)
        mean = torch.empty(rows, device=DEV)
        rstd = torch.empty(rows, device=DEV)
        ops().layernorm_fwd(x[:rows], w, b, y, mean, rstd, 1e-5)
        torch.cuda.synchronize()
        outs.append((y, mean, rstd))
    ref = torch.nn.functional.layer_norm(x[:256].double().cpu(), (C,), w.double().cpu(), b.double().cpu(), 1e-5)
    assert relerr(outs[1][0], ref) < 1e-5
    for y, mean, rstd in outs[1:]:
        n = y.shape[0]
        assert torch.equal(y, outs[0][0][:n]) and torch.equal(mean, outs[0][1][:n])
        assert torch.equal(rstd, outs[0][2][:n])


@pytest.mark.parametrize("B,C,H,Tmax,pos", [(256, 126, 6, 256, 1), (256, 126, 6, 256, 200), (33, 64, 4, 20, 20),
                                            (1, 6, 2, 4, 3)])
def test_decode_qkv_f32_matches_ln_linear_and_append(B, C, H, Tmax, pos):
    """generate()'s per-token ln1 + QKV + K/V append in one launch (k_gemm_f32r with the LayerNorm in its
    prologue and the cache writes in its epilogue) against layernorm_fwd + gemm + decode_kv_append:
    qkv and both caches bitwise equal (cache rows other than pos untouched)."""
    torch.manual_seed(46)
    D = C // H
    x = torch.randn(B, C, device=DEV)
    w = torch.randn(3 * C, C, device=DEV) / C ** 0.5
    lw = 1.0 + 0.1 * torch.randn(C, device=DEV)
    lb = 0.1 * torch.randn(C, device=DEV)
    ln = torch.full((1,), pos, dtype=torch.int64, device=DEV)
    kc0 = torch.randn(B, H, Tmax, D, device=DEV)
    vc0 = torch.randn(B, H, Tmax, D, device=DEV)
    kc, vc = kc0.clone(), vc0.clone()
    qkv = torch.full((B, 3 * C), float("nan"), device=DEV)
    ops().decode_qkv_f32(x, lw, lb, 1e-5, w, qkv, ln, kc, vc)
    a = torch.full((B, C), float("nan"), device=DEV)
    ops().layernorm_fwd(x, lw, lb, a, torch.empty(B, device=DEV), torch.empty(B, device=DEV), 1e-5)
    ref = torch.full((B, 3 * C), float("nan"), device=DEV)
    ops().gemm(a, w, ref, False, False, False, B, 3 * C, C, C, C, 3 * C, 0, None, None, 0, None, 0, 0.0, 0, None, 0,
               0.0, 1, None)
    kr, vr = kc0.clone(), vc0.clone()
    ops().decode_kv_append(ref, C, 2 * C, ln, kr, vr)
    torch.cuda.synchronize()
    assert torch.equal(qkv.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(kc.view(torch.int32), kr.view(torch.int32))
    assert torch.equal(vc.view(torch.int32), vr.view(torch.int32))
    assert not torch.equal(kc[:, :, pos - 1], kc0[:, :, pos - 1])
