"""Memory footprint of the packed-row attention entry points (cg_attn_fwd_seg, cg_attn_fwd_seg_premasked,
cg_attn_bwd_seg) on guard-banded operands (tests/footprint.py), as test_gpu_footprint.py holds their
unsegmented neighbours: padded row strides for qkv / o / dout / dqkv, lse, seg_start, seg_end, the keep-bit
buffer and the workspace in exactly sized Boxes, outputs poisoned on entry.  Nothing outside the owned
elements is written, no const operand changes, no poison reaches an output, and the padded layout gives
the tight layout's bits.  (These declarations spell their strides stride_*: test_gpu_footprint.py's
registry counts the ld_* entry points of its own file only.)"""
import ctypes

import pytest
import torch

import packing as PK
from footprint import Box, WsBox

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
RAN_PADDED = {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    L().load()
    yield


def L():
    from replicatinggpt_amd import _lib
    return _lib


def P(box, col=0):
    return None if box is None else ctypes.c_void_p(box.view.data_ptr() + col * box.view.element_size())


def run(dt, B, T, H, D, p, lay, premasked=False, delta=False):
    """One forward + backward through the C ABI on Boxes; layout "T" tight, "P" padded strides (a multiple
    of 16 bytes: the MFMA path stays), "O" odd padding (fp32: the generic kernels' any-stride path).
    Returns the written operands' bits."""
    lib = L().load()
    d = H * D
    padq, pado = {"T": (0, 0), "P": (16, 8), "O": (3, 5)}[lay]
    g = torch.Generator().manual_seed(7)
    qkv = Box(B * T, 3 * d, dt, ld=3 * d + padq, device=DEV).fill((torch.randn(B * T, 3 * d, generator=g) * 0.7).to(DEV)).snapshot()
    dout = Box(B * T, d, dt, ld=d + pado, device=DEV).fill(torch.randn(B * T, d, generator=g).to(DEV)).snapshot()
    segs = torch.stack([PK.seg_of_lengths(r, T) for r in ([T // 3, 1, T // 4], [T // 2 + 1])][:B])
    ss = Box(B, T, I32, device=DEV, pad=0).fill(segs.to(DEV)).snapshot()
    se = Box(B, T, I32, device=DEV, pad=0)
    st = L().stream_ptr()
    assert lib.cg_seg_bounds(P(ss), P(se), B, T, st) == 0
    torch.cuda.synchronize()
    se.assert_clean("seg_end")
    assert torch.equal(se.view.cpu(), PK.seg_end_of(segs))
    se.snapshot()
    o = Box(B * T, d, dt, ld=d + pado, device=DEV).prefill("nan")
    lse = Box(B * H, T, F32, device=DEV).prefill("nan")
    dqkv = Box(B * T, 3 * d, dt, ld=3 * d + padq, device=DEV).prefill("nan")
    call = torch.tensor([2], dtype=torch.int64, device=DEV)
    fast = dt == BF16 and D == 64 and T % 64 == 0
    mask = WsBox(lib.cg_attn_mask_bytes(B, H, T), "nan", DEV) if fast and p > 0 else None
    es = qkv.view.element_size()
    scale = (3.0 * D) ** -0.5
    qp = [ctypes.c_void_p(qkv.view.data_ptr() + j * d * es) for j in range(3)]
    fwd = lib.cg_attn_fwd_seg
    if premasked and mask is not None:
        assert lib.cg_attn_dropmask(B, H, T, p, 11, ctypes.c_void_p(call.data_ptr()), 7, P(mask), st) == 0
        fwd = lib.cg_attn_fwd_seg_premasked
    rc = fwd(L().dtype_code(dt), B, T, H, D, *qp, qkv.ld, P(o), o.ld, P(lse), scale, p, 11,
             ctypes.c_void_p(call.data_ptr()), 7, P(mask), P(ss), P(se), st)
    assert rc == 0, lib.cg_last_error_string()
    ws = WsBox(lib.cg_attn_bwd_workspace(B, T, H, D), "nan", DEV)
    dl = None
    if delta:   # rowsum(dO * O) per head, in plain torch
        dl = Box(B * H, T, F32, device=DEV)
        dl.fill((o.view.float() * dout.view.float()).view(B, T, H, D).sum(-1).permute(0, 2, 1).reshape(B * H, T)).snapshot()
    dp = [ctypes.c_void_p(dqkv.view.data_ptr() + j * d * es) for j in range(3)]
    rc = lib.cg_attn_bwd_seg(L().dtype_code(dt), B, T, H, D, *qp, qkv.ld, P(o), o.ld, P(dout), dout.ld, P(lse), P(dl),
                             *dp, dqkv.ld, scale, p, 11, ctypes.c_void_p(call.data_ptr()), 7, P(mask), P(ss), P(se),
                             P(ws), st)
    assert rc == 0, lib.cg_last_error_string()
    torch.cuda.synchronize()
    what = f"[{dt} T {T} D {D} p {p} layout {lay} premasked {premasked} delta {delta}]"
    for name, box in (("o", o), ("lse", lse), ("dqkv", dqkv), ("workspace", ws), ("qkv", qkv), ("dout", dout),
                      ("seg_start", ss), ("seg_end", se)) + ((("mask", mask),) if mask is not None else ()) + (
                          (("delta", dl),) if dl is not None else ()):
        box.assert_clean(f"{name} {what}")
    for name, box in (("qkv", qkv), ("dout", dout), ("seg_start", ss), ("seg_end", se)) + (
            (("delta", dl),) if dl is not None else ()):
        box.assert_unchanged(f"{name} {what}")
    for name, box in (("o", o), ("lse", lse), ("dqkv", dqkv)):
        assert torch.isfinite(box.view.float()).all(), f"{name} {what}: poison or a non-finite value in an output"
    if lay != "T":
        for fn in ("cg_attn_fwd_seg_premasked" if fwd is lib.cg_attn_fwd_seg_premasked else "cg_attn_fwd_seg",
                   "cg_attn_bwd_seg"):
            RAN_PADDED[fn] = RAN_PADDED.get(fn, 0) + 1
    return {"o": o.bits(), "lse": lse.bits(), "dqkv": dqkv.bits()}


SHAPES = [(BF16, 2, 128, 2, 64, "P"), (BF16, 1, 64, 1, 64, "P"), (F32, 2, 37, 3, 21, "O"), (BF16, 1, 96, 1, 32, "P"),
          (BF16, 1, 320, 1, 64, "P"), (BF16, 2, 576, 2, 64, "P"), (F32, 2, 130, 4, 16, "O")]


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("dt,B,T,H,D,lay", SHAPES)
def test_padded_operands_stay_inside_and_give_the_tight_bits(dt, B, T, H, D, lay, p):
    tight = run(dt, B, T, H, D, p, "T")
    padded = run(dt, B, T, H, D, p, lay)
    for name in tight:
        assert torch.equal(tight[name], padded[name]), (name, lay)
    if dt == BF16 and D == 64 and T <= 256:
        if p > 0:
            pre = run(dt, B, T, H, D, p, lay, premasked=True)
            for name in tight:
                assert torch.equal(tight[name], pre[name]), (name, "premasked")
        run(dt, B, T, H, D, p, lay, delta=True)   # delta read from a Box of exactly B H T floats


def test_every_packed_attention_entry_point_ran_padded():
    assert all(RAN_PADDED.get(fn, 0) > 0 for fn in ("cg_attn_fwd_seg", "cg_attn_fwd_seg_premasked", "cg_attn_bwd_seg")), RAN_PADDED
