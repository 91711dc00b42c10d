"""Memory footprint of the weight-stationary bf16 GEMM (csrc/gemm_ws.hip, gemm_variant 31) on guard-banded,
padded operands (tests/footprint.py): it writes every owned element of C, of the keep-bit words and of the
column partials and nothing else -- not the row padding, not the guard bands --, leaves A, B, the bias and
the keep bits it reads as they were, and does not care what its outputs held on entry."""
import ctypes

import pytest
import torch

from footprint import Box

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
CASES = [("store_nt", 192, 384, 192), ("store_bt", 192, 384, 192), ("bias_relu_bits", 192, 384, 192),
         ("relu_bwd_colpart", 192, 384, 192), ("store_bt", "bpp+1", 1152, 384), ("bias_relu_bits", "bpp+1", 1152, 384),
         ("relu_bwd_colpart", "bpp+1", 1152, 384), ("relu_bwd_colpart", 64, 128, 64)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    yield
    L().check(lib().cg_set_tuning(b"gemm_variant", 0), "tuning")


def L():
    from replicatinggpt_amd import _lib
    return _lib


def lib():
    return L().load()


def P(box):
    return None if box is None else ctypes.c_void_p(box.view.data_ptr())


@pytest.mark.parametrize("kind,M,N,K", CASES)
def test_writes_only_its_outputs(kind, M, N, K):
    if M == "bpp+1":   # one block of each panel gets two tiles
        M = 64 * (torch.cuda.get_device_properties(0).multi_processor_count // (N // 128)) + 64
    g = torch.Generator().manual_seed(11)
    bt = kind in ("store_bt", "relu_bwd_colpart")
    # 16-B aligned origins and strides (what the kernel takes), every stride padded beyond the logical width
    A = Box(M, K, BF16, ld=K + 8, offset_bytes=16, device=DEV).fill(torch.randn(M, K, generator=g) * 0.5).snapshot()
    Bs = (K, N) if bt else (N, K)
    B = Box(*Bs, BF16, ld=Bs[1] + 24, offset_bytes=32, device=DEV).fill(torch.randn(*Bs, generator=g) * 0.05).snapshot()
    C = Box(M, N, BF16, ld=N + 8, offset_bytes=16, device=DEV)
    bias = bits = part = None
    kcode, aux_code = 0, 0
    if kind == "bias_relu_bits":
        bias = Box(1, N, F32, offset_bytes=16, device=DEV).fill(torch.randn(N, generator=g) * 0.1).snapshot()
        bits = Box(M, N // 32, I32, ld=N // 32 + 4, device=DEV)
        kcode, aux_code = L().EPI_BIAS_RELU, L().CG_BITS
    elif kind == "relu_bwd_colpart":
        words = torch.randint(-2 ** 31, 2 ** 31 - 1, (M, N // 32), generator=g, dtype=torch.int64).to(I32)
        bits = Box(M, N // 32, I32, ld=N // 32 + 4, device=DEV, pad=0).fill(words).snapshot()
        part = Box(M // 64, N, F32, offset_bytes=16, device=DEV)   # [M / 64][N], row stride N by the ABI
        kcode, aux_code = L().EPI_RELU_BWD, L().CG_BITS
    outs = [("C", C)] + ([("bits", bits)] if kind == "bias_relu_bits" else [])
    outs += [("colpart", part)] if part is not None else []
    epi = L().Epilogue(kcode, P(bias), None, 0, P(bits), aux_code, bits.ld if bits is not None else 0, 0.0, 0, None, 0,
                       0.0, P(part), 0)
    got = {}
    L().check(lib().cg_set_tuning(b"gemm_variant", 31), "tuning")
    try:
        for prefill in ("nan", "zero"):
            for _, b in outs:
                b.prefill(prefill)
            n0 = lib().cg_gemm_ws_launches()
            rc = lib().cg_gemm(L().CG_BF16, 0, int(bt), M, N, K, P(A), A.ld, P(B), B.ld, P(C), L().CG_BF16, C.ld,
                               ctypes.byref(epi), 1, None, L().stream_ptr())
            L().check(rc, "cg_gemm")
            torch.cuda.synchronize()
            assert lib().cg_gemm_ws_launches() == n0 + 1, "k_gemm_ws did not take the call"
            for name, b in outs:
                b.assert_clean(f"{kind} {name} ({prefill} prefill)")
            for name, b in (("A", A), ("B", B), ("bias", bias), ("bits", bits if kind == "relu_bwd_colpart" else None)):
                if b is not None:
                    b.assert_unchanged(f"{kind} {name}")
            got[prefill] = [b.bits() for _, b in outs]
    finally:
        L().check(lib().cg_set_tuning(b"gemm_variant", 0), "tuning")
    # every owned element was written (none keeps the NaN poison) and does not depend on what was there
    assert not torch.isnan(C.view.float()).any()
    if part is not None:
        assert not torch.isnan(part.view).any()
    for a, b in zip(got["nan"], got["zero"]):
        assert torch.equal(a, b)
