"""Segment-masked attention (cg_attn_fwd_seg / cg_attn_bwd_seg) at the op level: against the dense fp64
reference with the block-diagonal causal mask (tests/packing.py), bitwise against the unsegmented entry
points for an all-zero seg_start, bitwise independence of a segment from its neighbours' data, and the
precomputed-delta form.  Shapes: the sequence-resident bf16 kernels (D 64, T 64 / 128 / 192 / 256), the
generic kernels (fp32 D 21 -- its forward at p = 0 the fp32 MFMA kernel --, bf16 D 32) and long bf16 rows
(D 64, T 320: the ring kernels; longer rows, more heads: test_gpu_packed_attn_long.py)."""
import pytest
import torch

import packing as PK
from conftest import bf16_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, SITE, CALL = 11, 7, 2
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from replicatinggpt_amd import _lib as L
    L.load()
    yield


def Fn():
    from replicatinggpt_amd import functional
    return functional


def ops():
    from replicatinggpt_amd import ops as O
    return O


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# Segment lengths per row (what is left of the row is a last segment -- a padding tail in a sampler's
# batch), at the places the 32 x 32 tile code can go wrong:
#   []                 one segment: the unsegmented mask
#   boundaries on 32 / 64, one off either side (31, 33, 63, 65), length-1 segments
#   segments that start at >= 64 and >= 128: whole key tiles masked for every query of a group
#   a boundary inside a 32-query group: some lanes' first subtiles wholly masked, their neighbours' not
SEGS = {
    64: [[], [32], [31, 2], [33, 1, 10], [16, 1, 19, 20], [63]],
    128: [[], [64], [63, 2, 1], [65, 31], [32, 64, 7], [100, 1], [77, 20, 20]],
    192: [[], [64, 64], [63, 2, 63, 2], [65, 63, 33], [128], [129, 50], [96, 1, 95]],
    256: [[], [64, 64, 64], [63, 2, 63, 2, 100], [65, 63, 33, 31], [128], [129, 100], [140, 1, 50],
          [32, 32, 100, 37, 40]],
    37: [[], [5, 1, 20], [36], [12, 12]],
    96: [[], [33, 31, 1], [64, 10], [95]],
    320: [[], [64, 65, 127, 1], [300], [129, 130]],
}
#        dtype B  T    H  D
RESIDENT = [(BF, 2, 64, 2, 64), (BF, 2, 128, 2, 64), (BF, 2, 256, 2, 64)]
GENERIC = [(F32, 2, 37, 3, 21), (BF, 1, 96, 1, 32), (BF, 1, 320, 1, 64)]
RESIDENT_NT3 = [(BF, 2, 192, 2, 64)]   # resident too; listed last so that the ids of the cases above stay
SHAPES = RESIDENT + GENERIC + RESIDENT_NT3


def batches(B, T):
    """The segmentations of T, B rows at a time (different rows of a batch get different ones)."""
    rows = SEGS[T]
    rows = rows + rows[:(-len(rows)) % B]
    return [torch.stack([PK.seg_of_lengths(r, T) for r in rows[i:i + B]]) for i in range(0, len(rows), B)]


CASES = [(dt, B, T, H, D, i) for dt, B, T, H, D in SHAPES for i in range(len(batches(B, T)))]


def make(dt, B, T, H, D, seed=4):
    g = torch.Generator().manual_seed(seed)
    d = H * D
    qkv = (torch.randn(B * T, 3 * d, generator=g) * 0.7).to(dt)
    dout = torch.randn(B * T, d, generator=g).to(dt)
    return qkv, dout, (3.0 * D) ** -0.5


def run(qkv, dout, B, T, H, D, scale, p, seg_start=None, delta=None, want_ws=False):
    """o, lse, dqkv (and the backward workspace) of one forward + backward on the device; seg_start None:
    the unsegmented entry points."""
    d = H * D
    qkv_d, dout_d = qkv.to(DEV), dout.to(DEV)
    call = torch.tensor([CALL], dtype=torch.int64, device=DEV)
    seg = None
    if seg_start is not None:
        ss = seg_start.to(DEV)
        se = torch.empty_like(ss)
        ops().seg_bounds(ss, se)
        assert torch.equal(se.cpu(), PK.seg_end_of(seg_start))
        seg = (ss, se)
    o = torch.full((B * T, d), float("nan"), dtype=qkv.dtype, device=DEV)
    lse, mask = Fn().attention_fwd(qkv_d, B, T, H, D, o, scale, p, SEED, call, SITE, seg=seg)
    if not want_ws:
        dqkv = Fn().attention_bwd(qkv_d, B, T, H, D, o, dout_d, lse, scale, p, SEED, call, SITE, mask, delta, seg=seg)
        return o, lse, dqkv
    O = ops()
    ws = torch.zeros(O.attn_bwd_workspace(B, T, H, D) // 4 + 1, device=DEV)
    dqkv = torch.full_like(qkv_d, float("nan"))
    O.attn_bwd_seg(qkv_d, B, T, H, D, 0, d, 2 * d, 3 * d, o, d, dout_d, d, lse, dqkv, 3 * d, float(scale), float(p), SEED,
                   call, SITE, mask, ws, seg[0], seg[1], delta)
    return o, lse, dqkv, ws


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("dt,B,T,H,D,i", CASES)
def test_against_dense_reference(dt, B, T, H, D, i, p):
    """o, dq, dk, dv against the fp64 reference with the block-diagonal causal mask and the Philox keep
    bits, at test_attention_fwd_bwd's bars; nothing non-finite anywhere, lse included."""
    seg_start = batches(B, T)[i]
    qkv, dout, scale = make(dt, B, T, H, D)
    d = H * D
    q, k, v = (qkv[:, j * d:(j + 1) * d].double().view(B, T, H, D).requires_grad_(True) for j in range(3))
    ref = PK.attn_ref_seg(q, k, v, scale, seg_start, p, SEED, (CALL << 8) | SITE)
    ref.backward(dout.double().view(B, T, H, D))
    o, lse, dqkv = run(qkv, dout, B, T, H, D, scale, p, seg_start)
    torch.cuda.synchronize()
    for name, t in (("o", o), ("lse", lse), ("dqkv", dqkv)):
        assert torch.isfinite(t.float()).all(), name
    got = {"o": o, "dq": dqkv[:, :d], "dk": dqkv[:, d:2 * d], "dv": dqkv[:, 2 * d:]}
    want = {"o": ref, "dq": q.grad, "dk": k.grad, "dv": v.grad}
    for name in got:
        if dt == F32:
            assert relerr(got[name], want[name].reshape(B * T, d)) < 1e-5, name
        else:
            ok, st = bf16_close(got[name], want[name].reshape(B * T, d))
            assert ok, (name, st)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("dt,B,T,H,D", SHAPES)
def test_all_zero_seg_start_is_the_unsegmented_entry_point(dt, B, T, H, D, p):
    """One segment per row: o, lse, dq, dk and dv are bitwise those of cg_attn_fwd / cg_attn_bwd.
    A segmented call runs the kernel family of the unsegmented call of its shape."""
    qkv, dout, scale = make(dt, B, T, H, D, seed=8)
    base = run(qkv, dout, B, T, H, D, scale, p)
    seg = run(qkv, dout, B, T, H, D, scale, p, torch.zeros((B, T), dtype=torch.int32))
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dqkv"), base, seg):
        print(f"{name}: max |seg - unsegmented| / max |unsegmented| = {relerr(b, a):.3e}")
        assert torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32),
                           b.view(torch.int16 if b.dtype == BF else torch.int32)), name


LEAK = {64: [13, 20, 1, 18], 128: [40, 30, 33, 20], 256: [70, 61, 66, 40], 37: [9, 11, 10], 96: [31, 34, 20],
        320: [100, 97, 90], 192: [50, 47, 55, 20]}


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("which", ["first", "middle", "last"])
@pytest.mark.parametrize("dt,B,T,H,D", SHAPES)
def test_no_leak_between_segments_bitwise(dt, B, T, H, D, which, p):
    """Two runs whose q / k / v / dout differ in every segment but one (other values, large finite ones
    among them): the kept segment's o, lse, dq, dk and dv are bit-identical.  A mask that is off by one
    key or one query cannot pass, nor can a running maximum shared between the segments of a wave."""
    seg_row = PK.seg_of_lengths(LEAK[T], T)
    spans = PK.segments(seg_row)
    no_leak(dt, B, T, H, D, seg_row, {"first": spans[0], "middle": spans[1], "last": spans[-1]}[which], p)


def no_leak(dt, B, T, H, D, seg_row, span, p):
    """The statement of test_no_leak_between_segments_bitwise for the segment ``span`` of ``seg_row`` (every
    row of the batch segmented alike)."""
    s, e = span
    seg_start = seg_row[None].repeat(B, 1)
    qkv, dout, scale = make(dt, B, T, H, D, seed=21)
    qkv2, dout2, _ = make(dt, B, T, H, D, seed=22)
    g = torch.Generator().manual_seed(23)
    big = torch.rand(qkv2.shape, generator=g) < 0.05
    sign = (torch.rand(qkv2.shape, generator=g) < 0.5).to(dt) * 2 - 1
    qkv2 = torch.where(big, sign * 1e3, qkv2)
    dout2[::7] = 1e3
    keep = torch.zeros(B, T, dtype=torch.bool)
    keep[:, s:e] = True
    keep = keep.view(B * T, 1)
    qkv2, dout2 = torch.where(keep, qkv, qkv2), torch.where(keep, dout, dout2)
    assert not torch.equal(qkv2, qkv) and torch.isfinite(qkv2.float()).all()
    a = run(qkv, dout, B, T, H, D, scale, p, seg_start)
    b = run(qkv2, dout2, B, T, H, D, scale, p, seg_start)
    torch.cuda.synchronize()
    bits = torch.int16 if dt == BF else torch.int32
    d = H * D
    for name, x, y in (("o", a[0], b[0]), ("dqkv", a[2], b[2])):
        assert torch.isfinite(y.float()).all(), name
        x, y = x.view(B, T, -1)[:, s:e], y.view(B, T, -1)[:, s:e]
        assert torch.equal(x.contiguous().view(bits), y.contiguous().view(bits)), name
    assert torch.isfinite(b[1]).all()
    assert torch.equal(a[1][:, :, s:e].contiguous().view(torch.int32), b[1][:, :, s:e].contiguous().view(torch.int32))


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("T", [64, 128, 256, 192])
def test_precomputed_delta_gives_the_bits_of_the_form_that_computes_it(T, p):
    """cg_attn_bwd_seg with delta = the rowsum(dO * O) its dQ half left in the workspace: dq, dk and dv
    bit for bit those of the call without it (the resident kernels then load neither O nor sum it)."""
    B, H, D = 2, 2, 64
    seg_start = batches(B, T)[1]
    qkv, dout, scale = make(BF, B, T, H, D, seed=31)
    _, _, base, ws = run(qkv, dout, B, T, H, D, scale, p, seg_start, want_ws=True)
    own = ws[:B * H * T].view(B, H, T).clone()
    assert torch.isfinite(own).all() and float(own.abs().max()) > 0
    _, _, din, _ = run(qkv, dout, B, T, H, D, scale, p, seg_start, delta=own, want_ws=True)
    torch.cuda.synchronize()
    assert torch.equal(base.view(torch.int16), din.view(torch.int16))


def test_operand_checks():
    O = ops()
    B, T, H, D = 1, 64, 1, 64
    qkv, dout, scale = make(BF, B, T, H, D)
    qkv = qkv.to(DEV)
    o = torch.empty(B * T, D, dtype=BF, device=DEV)
    lse = torch.empty(B, H, T, device=DEV)
    ss = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    for bad in (ss.long(), ss[:, :32], torch.zeros((B, 2 * T), dtype=torch.int32, device=DEV)[:, ::2]):
        with pytest.raises(ValueError, match="dense int32"):
            O.attn_fwd_seg(qkv, B, T, H, D, 0, D, 2 * D, 3 * D, o, D, lse, scale, 0.0, 0, None, 0, None, bad, ss)
