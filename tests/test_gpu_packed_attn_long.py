"""Segment-masked attention past one key tile, one head and T 320 (tables and recipes: tests/packing.py;
make / run / no_leak: test_gpu_packed_attn.py, whose arithmetic this file does not repeat).

* the bf16 ring kernels (D 64, T 512 / 576 / 1024, H 2 and 3, B 2): grids of two workgroups with their
  (last, x) pass pairs and the single-pass middle block, whole leading tiles skipped while the keep words
  advance, bounds on the 256-query and 128-key block edges, seg_start / seg_end rows shared by the heads
  of a batch row (bh != b);
* the fp32 MFMA forward over more than one 64-key tile (D 8 / 16 / 21 / 32, T 130 .. 300), tiles masked for
  all or for some of a wave's queries; at p = 0.2 the generic kernels at the same shapes;
* lse against the fp64 logsumexp of the masked scores everywhere, the resident kernels included;
* the lazy rescale forced inside a segment, its precondition asserted from the fp64 scores first;
* a given delta ignored beyond T 256.

Bars: bf16_close at its defaults and relerr < 1e-5 (fp32), as test_gpu_packed_attn.py; |lse - ref| < 2^-8
for bf16 (test_attention_forward_rescale_branch's derivation: the row sums run over bf16-rounded weights,
each within 2^-8 relative, so ln(1 + 2^-8) < 2^-8 -- dropout does not enter lse) and 1e-5 max(1, max|ref|)
for fp32."""
import pytest
import torch

import packing as PK
import test_gpu_packed_attn as A
from conftest import bf16_close

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SEED, SITE, CALL = A.SEED, A.SITE, A.CALL
PS = [0.0, 0.2]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from replicatinggpt_amd import _lib as L
    L.load()
    yield


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def reference(dt, B, T, H, D, key, i, p):
    """(seg_start, qkv, dout, scale, {o, dq, dk, dv} and lse in fp64) of batch i of the table ``key``."""
    rows = {"ring": PK.RING_SEGS, "f32": PK.F32_SEGS, "resident": A.SEGS}[key][T]
    seg_start = PK.seg_batches(rows, B, T)[i]
    qkv, dout, scale = A.make(dt, B, T, H, D)
    d = H * D
    q, k, v = (qkv[:, j * d:(j + 1) * d].double().view(B, T, H, D).requires_grad_(True) for j in range(3))
    ref = PK.attn_ref_seg(q, k, v, scale, seg_start, p, SEED, (CALL << 8) | SITE)
    ref.backward(dout.double().view(B, T, H, D))
    with torch.no_grad():
        lse = PK.lse_ref_seg(q, k, scale, seg_start)
    want = {"o": ref.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    return seg_start, qkv, dout, scale, {n: t.reshape(B * T, d) for n, t in want.items()}, lse


def against_reference(dt, B, T, H, D, key, i, p):
    seg_start, qkv, dout, scale, want, lse_ref = reference(dt, B, T, H, D, key, i, p)
    d = H * D
    o, lse, dqkv = A.run(qkv, dout, B, T, H, D, scale, p, seg_start)
    torch.cuda.synchronize()
    for name, t in (("o", o), ("lse", lse), ("dqkv", dqkv)):
        assert torch.isfinite(t.float()).all(), name
    got = {"o": o, "dq": dqkv[:, :d], "dk": dqkv[:, d:2 * d], "dv": dqkv[:, 2 * d:]}
    lse_err = float((lse.double().cpu() - lse_ref).abs().max())
    lse_bar = 2.0 ** -8 if dt == BF else 1e-5 * max(1.0, float(lse_ref.abs().max()))
    print(f"lse: max |got - ref| {lse_err:.3e} (bar {lse_bar:.3e})")
    for name in got:
        if dt == F32:
            err = A.relerr(got[name], want[name])
            print(f"{name}: relerr {err:.3e}")
            assert err < 1e-5, name
        else:
            ok, st = bf16_close(got[name], want[name])
            print(f"{name}: {st}")
            assert ok, (name, st)
    assert lse_err < lse_bar, (lse_err, lse_bar)


def all_zero_is_unsegmented(dt, B, T, H, D, p):
    qkv, dout, scale = A.make(dt, B, T, H, D, seed=8)
    base = A.run(qkv, dout, B, T, H, D, scale, p)
    seg = A.run(qkv, dout, B, T, H, D, scale, p, torch.zeros((B, T), dtype=torch.int32))
    torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dqkv"), base, seg):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(bits(a), bits(b)), name


# ---------------------------------------------------------------------------------------
# the ring kernels: bf16, D 64, T > 256
# ---------------------------------------------------------------------------------------
RING_CASES = [(B, T, H, i) for B, T, H in PK.RING_SHAPES for i in range(len(PK.seg_batches(PK.RING_SEGS[T], B, T)))]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,T,H,i", RING_CASES)
def test_ring_against_dense_reference(B, T, H, i, p):
    """o, dq, dk, dv (bf16_close) and lse (2^-8) against fp64 with the block-diagonal causal mask and the
    Philox keep bits; the rows of a batch segmented differently, every head of a row alike."""
    against_reference(BF, B, T, H, 64, "ring", i, p)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,T,H", PK.RING_SHAPES)
def test_ring_all_zero_seg_start_is_the_unsegmented_entry_point(B, T, H, p):
    all_zero_is_unsegmented(BF, B, T, H, 64, p)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("which", list(PK.RING_LEAK))
def test_ring_no_leak_between_segments_bitwise(which, p):
    """A segment across the query-block edge, one wholly inside the last query block and the first: their
    o, lse, dq, dk, dv do not depend on the other segments' data (1e3 entries among it), bit for bit."""
    T, lengths, n = PK.RING_LEAK[which]
    seg_row = PK.seg_of_lengths(lengths, T)
    A.no_leak(BF, 2, T, 2, 64, seg_row, PK.segments(seg_row)[n], p)


@pytest.mark.parametrize("p", PS)
def test_ring_backward_ignores_a_given_delta(p):
    """Beyond T 256 cg_attn_bwd_seg computes delta in its dQ kernel whatever it is handed: a delta full of
    NaN gives the bits of the call without one, and the workspace holds the same computed delta."""
    B, T, H, D = 2, 512, 2, 64
    seg_start = PK.seg_batches(PK.RING_SEGS[T], B, T)[1]
    qkv, dout, scale = A.make(BF, B, T, H, D, seed=31)
    _, _, base, ws = A.run(qkv, dout, B, T, H, D, scale, p, seg_start, want_ws=True)
    nan = torch.full((B, H, T), float("nan"), device=A.DEV)
    _, _, given, ws2 = A.run(qkv, dout, B, T, H, D, scale, p, seg_start, delta=nan, want_ws=True)
    torch.cuda.synchronize()
    assert torch.isfinite(base.float()).all() and torch.isfinite(given.float()).all()
    assert torch.equal(bits(base), bits(given))
    own, own2 = ws[:B * H * T], ws2[:B * H * T]
    assert torch.isfinite(own).all() and float(own.abs().max()) > 0 and torch.equal(bits(own), bits(own2))
    assert torch.isnan(nan).all()


# ---------------------------------------------------------------------------------------
# fp32, D <= 32: the MFMA forward (p = 0) over more than one key tile; the generic kernels (p = 0.2)
# ---------------------------------------------------------------------------------------
F32_CASES = [(B, T, H, D, i) for B, T, H, D in PK.F32_SHAPES for i in range(len(PK.seg_batches(PK.F32_SEGS[T], B, T)))]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,T,H,D,i", F32_CASES)
def test_f32_against_dense_reference(B, T, H, D, i, p):
    """o, dq, dk, dv relerr < 1e-5 and lse within 1e-5 max(1, max|ref|) of fp64."""
    against_reference(F32, B, T, H, D, "f32", i, p)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,T,H,D", PK.F32_SHAPES)
def test_f32_all_zero_seg_start_is_the_unsegmented_entry_point(B, T, H, D, p):
    """At p = 0 and T <= 256 cg_attn_fwd is the sequence-resident fp32 kernel, the segmented call the
    64-query-block one: bitwise equal, as launch_fwd_f32_seg promises."""
    all_zero_is_unsegmented(F32, B, T, H, D, p)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("which", ["first", "middle", "last"])
@pytest.mark.parametrize("B,T,H,D", [s for s in PK.F32_SHAPES if s[1] in PK.F32_LEAK])
def test_f32_no_leak_between_segments_bitwise(B, T, H, D, which, p):
    seg_row = PK.seg_of_lengths(PK.F32_LEAK[T], T)
    spans = PK.segments(seg_row)
    A.no_leak(F32, B, T, H, D, seg_row, {"first": spans[0], "middle": spans[1], "last": spans[-1]}[which], p)


# ---------------------------------------------------------------------------------------
# the resident kernels' lse
# ---------------------------------------------------------------------------------------
RESIDENT_CASES = [(B, T, H, i) for _, B, T, H, _ in A.RESIDENT + A.RESIDENT_NT3 for i in range(len(A.batches(B, T)))]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,T,H,i", RESIDENT_CASES)
def test_resident_lse_against_dense_reference(B, T, H, i, p):
    """The sequence-resident kernels (NT 1 .. 4) at test_gpu_packed_attn.py's segmentations, lse included."""
    against_reference(BF, B, T, H, 64, "resident", i, p)


# ---------------------------------------------------------------------------------------
# the lazy rescale inside a segment
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,lengths", PK.RESCALE_RECIPES, ids=[f"T{T}" for T, _ in PK.RESCALE_RECIPES])
def test_forced_rescale_inside_a_segment(T, lengths):
    """packing.rescale_data: in every segment of >= 130 positions some query meets a later 64-key tile whose
    maximum exceeds that of its earlier visible tiles by more than RESCALE_THR (asserted here from the fp64
    scores, before the device runs), so rescale_if_seg must move that segment's running max.  o within 2e-2
    and lse within 2^-8 of fp64 (test_attention_forward_rescale_branch's bars); dq, dk, dv bf16_close."""
    B, H, D = 1, 2, 64
    d = H * D
    qkv, seg_row, scale = PK.rescale_data(T, lengths, H, D)
    seg_start = seg_row[None]
    q, k, v = (qkv[:, j * d:(j + 1) * d].double().view(B, T, H, D).requires_grad_(True) for j in range(3))
    with torch.no_grad():
        fires = PK.rescale_query_tiles(q, k, scale, seg_row)
        lse_ref = PK.lse_ref_seg(q, k, scale, seg_start)
    print("query-tiles that force the rescale, per segment:", fires)
    long = [sp for sp in fires if sp[1] - sp[0] >= PK.RESCALE_MIN_SEGMENT]
    assert long and all(fires[sp] > 0 for sp in long), fires
    dout = torch.randn(B * T, d, generator=torch.Generator().manual_seed(32)).to(BF)
    ref = PK.attn_ref_seg(q, k, v, scale, seg_start)
    ref.backward(dout.double().view(B, T, H, D))
    o, lse, dqkv = A.run(qkv, dout, B, T, H, D, scale, 0.0, seg_start)
    torch.cuda.synchronize()
    for name, t in (("o", o), ("lse", lse), ("dqkv", dqkv)):
        assert torch.isfinite(t.float()).all(), name
    err_o = A.relerr(o, ref.reshape(B * T, d))
    err_lse = float((lse.double().cpu() - lse_ref).abs().max())
    print(f"o relerr {err_o:.3e}, lse max |got - ref| {err_lse:.3e}")
    assert err_o < 2e-2
    assert err_lse < 2.0 ** -8
    for name, got, want in (("dq", dqkv[:, :d], q.grad), ("dk", dqkv[:, d:2 * d], k.grad), ("dv", dqkv[:, 2 * d:], v.grad)):
        ok, st = bf16_close(got, want.reshape(B * T, d))
        print(f"{name}: {st}")
        assert ok, (name, st)
