"""cg_seg_bounds, cg_embed_fwd_seg and cg_embed_bwd_seg against plain torch indexing: positions restart at
each segment, dwpe is summed over all (b, t) with t - seg_start[b, t] = p in fp64, both accumulate modes,
run-to-run bit equality, and a seg_start with out-of-range values that must stay inside guard bands."""
import pytest
import torch

import packing as PK
from footprint import Box, WsBox

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


def random_seg(B, T, g, mean_len):
    """seg_start [B, T]: random segment lengths around mean_len; row 0 is one segment, the last row has
    length-1 segments at its start."""
    rows = []
    for b in range(B):
        lens, left = [], T
        if b == B - 1:
            lens, left = [1, 1], T - 2
        while left > 0 and b > 0:
            n = min(left, int(torch.randint(1, 2 * mean_len, (1,), generator=g)))
            lens.append(n)
            left -= n
        rows.append(PK.seg_of_lengths(lens, T))
    return torch.stack(rows)


def plain(idx, seg, wte, wpe, dx):
    """x by torch indexing; (dwte, its error budget), (dwpe, its budget): the sums in fp64, the budget of
    an element the bound of any fp32 summation order of its n addends, n 2^-24 sum |addend|."""
    B, T = idx.shape
    pos = torch.arange(T)[None] - seg.long()
    x = wte[idx] + wpe[pos]
    d2 = dx.double().reshape(B * T, -1)

    def scatter(rows, index):
        total = torch.zeros((rows, d2.shape[1]), dtype=torch.float64).index_add_(0, index, d2)
        mass = torch.zeros_like(total).index_add_(0, index, d2.abs())
        n = torch.bincount(index, minlength=rows).double()[:, None]
        return total, n * 2.0 ** -24 * mass

    return x, scatter(wte.shape[0], idx.reshape(-1)), scatter(T, pos.reshape(-1))


CASES = [(3, 40, 12, 7, 9), (4, 256, 384, 65, 40), (2, 1024, 8, 5, 100)]   # B, T, C, V, mean segment length


@pytest.mark.parametrize("B,T,C,V,mean", CASES)
def test_forward_and_gradients_match_plain_indexing(B, T, C, V, mean):
    O = ops()
    g = torch.Generator().manual_seed(B * T)
    idx = torch.randint(0, V, (B, T), generator=g)
    seg = random_seg(B, T, g, mean)
    wte, wpe = torch.randn(V, C, generator=g), torch.randn(T + 3, C, generator=g)   # block_size > T
    dx = torch.randn(B, T, C, generator=g)
    rx, (rdwte, bud_t), (rdwpe, bud_p) = plain(idx, seg, wte, wpe, dx)
    idx_d, seg_d = idx.to(DEV), seg.to(DEV)
    se = torch.empty_like(seg_d)
    O.seg_bounds(seg_d, se)
    assert torch.equal(se.cpu(), PK.seg_end_of(seg))
    x = torch.full((B, T, C), float("nan"), device=DEV)
    O.embed_fwd_seg(idx_d, seg_d, wte.to(DEV), wpe.to(DEV), x)
    assert torch.equal(x.cpu(), rx)                      # one fp32 add per element: exact
    ws = torch.empty(O.embed_bwd_workspace(B, T, C, V) // 4, device=DEV)
    dx_d = dx.to(DEV)
    # accumulate off: whatever the destinations held is overwritten
    dwte = torch.full((V, C), float("nan"), device=DEV)
    dwpe = torch.full((T, C), float("nan"), device=DEV)
    O.embed_bwd_seg(idx_d, se, dx_d, dwte, dwpe, False, ws)
    assert ((dwte.double().cpu() - rdwte).abs() <= bud_t + 2.0 ** -24 * rdwte.abs()).all()   # + the final rounding
    assert ((dwpe.double().cpu() - rdwpe).abs() <= bud_p + 2.0 ** -24 * rdwpe.abs()).all()
    # two runs bitwise equal
    dwte2, dwpe2 = torch.empty_like(dwte), torch.empty_like(dwpe)
    O.embed_bwd_seg(idx_d, se, dx_d, dwte2, dwpe2, False, ws)
    assert torch.equal(dwte.view(torch.int32), dwte2.view(torch.int32))
    assert torch.equal(dwpe.view(torch.int32), dwpe2.view(torch.int32))
    # accumulate on: added to what is there; each gradient also on its own
    base_t, base_p = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g)
    at, ap = base_t.to(DEV), base_p.to(DEV)
    O.embed_bwd_seg(idx_d, se, dx_d, at, None, True, ws)
    O.embed_bwd_seg(idx_d, se, dx_d, None, ap, True, ws)
    assert torch.equal(at, base_t.to(DEV) + dwte) and torch.equal(ap, base_p.to(DEV) + dwpe)
    # the token gradient is cg_embed_bwd's, bit for bit
    plain_t = torch.empty_like(dwte)
    O.embed_bwd(idx_d, dx_d, plain_t, None, False, ws)
    assert torch.equal(plain_t.view(torch.int32), dwte.view(torch.int32))


def test_all_zero_seg_start_is_the_plain_embedding():
    O = ops()
    B, T, C, V = 4, 64, 128, 65
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, V, (B, T), generator=g).to(DEV)
    wte, wpe = torch.randn(V, C, generator=g).to(DEV), torch.randn(T, C, generator=g).to(DEV)
    a, b = torch.empty(B, T, C, device=DEV), torch.empty(B, T, C, device=DEV)
    O.embed_fwd(idx, wte, wpe, a)
    O.embed_fwd_seg(idx, torch.zeros((B, T), dtype=torch.int32, device=DEV), wte, wpe, b)
    assert torch.equal(a, b)


@pytest.mark.parametrize("C", [12, 7])
def test_out_of_range_seg_start_stays_inside_the_operands(C):
    """A malformed seg_start (negative, beyond t, beyond T, huge) and the seg_end derived from it -- and a
    hand-made seg_end with values at or before t and beyond T -- read and write nothing outside the
    operands: guard bands stay clean, outputs hold no poison."""
    O = ops()
    B, T, V = 2, 40, 7
    g = torch.Generator().manual_seed(5)
    idx = Box(B, T, torch.int64, device=DEV, pad=0).fill(torch.randint(0, V, (B, T), generator=g))
    bad = torch.randint(-50, 90, (B, T), generator=g).to(torch.int32)
    bad[0, :4] = torch.tensor([-2 ** 31, 2 ** 31 - 1, T, T + 1], dtype=torch.int32)
    seg = Box(B, T, torch.int32, device=DEV, pad=0).fill(bad)
    seg_end = Box(B, T, torch.int32, device=DEV, pad=0)
    wte = Box(V, C, torch.float32, device=DEV).fill(torch.randn(V, C, generator=g)).snapshot()
    wpe = Box(T, C, torch.float32, device=DEV).fill(torch.randn(T, C, generator=g)).snapshot()
    x = Box(B * T, C, torch.float32, device=DEV)
    ss, se = seg.view.view(B, T), seg_end.view.view(B, T)
    O.seg_bounds(ss, se)
    O.embed_fwd_seg(idx.view.view(B, T), ss, wte.view, wpe.view, x.view.view(B, T, C))
    torch.cuda.synchronize()
    for name, box in (("idx", idx), ("seg_start", seg), ("seg_end", seg_end), ("wte", wte), ("wpe", wpe), ("x", x)):
        box.assert_clean(name)
    wte.assert_unchanged("wte")
    wpe.assert_unchanged("wpe")
    assert torch.isfinite(x.view).all()
    dx = Box(B * T, C, torch.float32, device=DEV).fill(torch.randn(B * T, C, generator=g)).snapshot()
    for ends in (se, None):
        if ends is None:   # a seg_end nobody derived: values at or before t, beyond T
            seg_end.fill(torch.randint(-5, 2 * T, (B, T), generator=g).to(torch.int32))
            ends = se
        dwte, dwpe = Box(V, C, torch.float32, device=DEV), Box(T, C, torch.float32, device=DEV)
        ws = WsBox(O.embed_bwd_workspace(B, T, C, V), device=DEV)
        O.embed_bwd_seg(idx.view.view(B, T), ends, dx.view.view(B, T, C), dwte.view, dwpe.view, False, ws.view.view(-1))
        torch.cuda.synchronize()
        for name, box in (("dwte", dwte), ("dwpe", dwpe), ("ws", ws), ("dx", dx), ("seg_end", seg_end)):
            box.assert_clean(name)
        dx.assert_unchanged("dx")
        assert torch.isfinite(dwte.view).all() and torch.isfinite(dwpe.view).all()
