"""The masked (ignore_index) cross-entropy entry points and cg_gather_pairs on the MI355X.

Shapes: V = 65, M = 80 -- five waves of 16 rows, two 64-row blocks, the last one partly empty; the fused
head forward at C = 384 (unrolled, KS = 12), C = 128 (KS = 4) and C = 32 (the runtime-K loop);
cg_ce_mean_masked also at 8200 rows, where it walks two of cg_sum_f32's blocks.

Every call runs on guard-banded, tightly laid out outputs and workspace (tests/footprint.py): nothing
may be written outside them.  With nothing ignored the masked entries must give the unmasked entries'
bits (test_cpu_pairs.py::test_reciprocal_identity_up_to_2_20 is why that is a fair demand); with a
mask they are judged against F.cross_entropy in fp64 on the kernel's own fp32 logits at the bars
test_gpu_ops.py holds the unmasked kernels to (fp32 path: loss 1e-5, dlogits 1e-5 of the maximum; fused
head: loss 1e-4, dl 2e-2 -- bf16 -- and db 1e-5).  NaN / inf in an ignored row must not change one bit
of anything else."""
import math

import pytest
import torch

import pairs as pr
from footprint import Box, WsBox

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, V, KP, IGN = 80, 65, 128, -100
F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64


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


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# rows that are IGNORED under each pattern
PATTERNS = {
    "none": lambda m: torch.zeros(m, dtype=torch.bool),
    "all": lambda m: torch.ones(m, dtype=torch.bool),
    "one-wave": lambda m: (torch.arange(m) // 16) == 2,
    "first-block": lambda m: torch.arange(m) < 64,
    "every-other": lambda m: torch.arange(m) % 2 == 1,
    "last-row-only-valid": lambda m: torch.arange(m) < m - 1,
}
MASKED = [p for p in PATTERNS if p not in ("none", "all")]


def targets(pattern, m=M, seed=3):
    t = torch.randint(0, V, (m,), generator=torch.Generator().manual_seed(seed))
    t[PATTERNS[pattern](m)] = IGN
    return t


_IN = {}


def head_inputs(C):
    """(a bf16 [M, C], wpad bf16 [KP, C], bias [V]) on the device, made once per C and never modified."""
    if C not in _IN:
        g = torch.Generator().manual_seed(100 + C)
        a = torch.randn(M, C, generator=g).to(BF16)
        wpad = torch.zeros(KP, C, dtype=BF16)
        wpad[:V] = (torch.randn(V, C, generator=g) / math.sqrt(C)).to(BF16)
        _IN[C] = (a.to(DEV), wpad.to(DEV), torch.randn(V, generator=g).to(DEV))
    return _IN[C]


def ce_logits(m=M):
    if ("ce", m) not in _IN:
        _IN[("ce", m)] = (torch.randn(m, V, generator=torch.Generator().manual_seed(7)) * 3).to(DEV)
    return _IN[("ce", m)]


def reference(logits, tgt, g=1.0, g_logits=None):
    """F.cross_entropy (ignore_index = -100, the default) in fp64 on the CPU: loss and g * dloss/dlogits."""
    lg = logits.detach().double().cpu().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lg, tgt.cpu())
    loss.backward()
    d = g * lg.grad
    return float(loss.detach()), d if g_logits is None else d + g_logits.double().cpu()


# ---------------------------------------------------------------------------------------
# the entry points on guard-banded boxes; every call checks its bands
# ---------------------------------------------------------------------------------------
def clean(**boxes):
    for name, b in boxes.items():
        b.assert_clean(name)


def run_head_fwd(a, wpad, bias, tgt):
    m = a.shape[0]
    lo, ls, l1, nm = Box(m, V, F32, device=DEV), Box(1, m, F32, device=DEV), Box(1, 1, F32, device=DEV), Box(1, 2, F32, device=DEV)
    ws = WsBox(ops().head_masked_workspace(m, V), "nan", DEV)
    ops().head_fwd_masked(a, wpad, bias, tgt.to(DEV), IGN, lo.view, ls.view, l1.view, nm.view, ws.view)
    torch.cuda.synchronize()
    clean(logits=lo, lse=ls, loss=l1, norm=nm, workspace=ws)
    return lo.view.clone(), ls.view.reshape(m).clone(), l1.view.reshape(()).clone(), nm.view.reshape(2).clone()


def run_head_bwd(logits, lse, tgt, norm, g=2.0, g_logits=None, db0=0.5):
    m = logits.shape[0]
    dl, db = Box(m, KP, BF16, device=DEV), Box(1, V, F32, device=DEV)
    db.fill(torch.full((V,), db0))
    ws = WsBox(ops().head_masked_workspace(m, V), "nan", DEV)
    ops().head_bwd_masked(logits, lse, tgt.to(DEV), IGN, torch.full((1,), g, device=DEV), norm,
                          None if g_logits is None else g_logits.to(DEV), dl.view, db.view, True, ws.view)
    torch.cuda.synchronize()
    clean(dl=dl, db=db, workspace=ws)
    return dl.view.clone(), db.view.reshape(V).clone()


def run_ce_fwd(logits, tgt):
    m = logits.shape[0]
    rows, ls, l1, nm = Box(1, m, F32, device=DEV), Box(1, m, F32, device=DEV), Box(1, 1, F32, device=DEV), Box(1, 2, F32, device=DEV)
    ws = WsBox(ops().ce_mean_masked_workspace(m), "nan", DEV)
    ops().ce_fwd_masked(logits, tgt.to(DEV), IGN, rows.view, ls.view)
    ops().ce_mean_masked(rows.view, tgt.to(DEV), IGN, l1.view, nm.view, ws.view)
    torch.cuda.synchronize()
    clean(loss_rows=rows, lse=ls, loss=l1, norm=nm, workspace=ws)
    return rows.view.reshape(m).clone(), ls.view.reshape(m).clone(), l1.view.reshape(()).clone(), nm.view.reshape(2).clone()


def run_ce_bwd(logits, lse, tgt, norm, g=2.0):
    m = logits.shape[0]
    d32, d16 = Box(m, V, F32, device=DEV), Box(m, V, BF16, device=DEV)
    ops().ce_bwd_masked(logits, tgt.to(DEV), IGN, lse, torch.full((1,), g, device=DEV), norm, d32.view, d16.view)
    torch.cuda.synchronize()
    clean(dlogits=d32, dlogits_lp=d16)
    return d32.view.clone(), d16.view.clone()


def unmasked_head(a, wpad, bias, tgt, g=2.0, g_logits=None, db0=0.5):
    m = a.shape[0]
    logits, lse, loss = torch.empty(m, V, device=DEV), torch.empty(m, device=DEV), torch.empty((), device=DEV)
    ws = torch.empty(ops().head_workspace(m, V) // 4, device=DEV)
    ops().head_fwd(a, wpad, bias, tgt.to(DEV), logits, lse, loss, ws)
    dl, db = torch.empty(m, KP, dtype=BF16, device=DEV), torch.full((V,), db0, device=DEV)
    ops().head_bwd(logits, lse, tgt.to(DEV), torch.full((1,), g, device=DEV), 1.0 / m,
                   None if g_logits is None else g_logits.to(DEV), dl, db, True, ws)
    return logits, lse, loss, dl, db


# ---------------------------------------------------------------------------------------
# 1. nothing ignored: the unmasked entry points' bits
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [384, 128, 32])
def test_head_no_mask_is_bitwise_the_unmasked_head(C):
    a, wpad, bias = head_inputs(C)
    tgt = targets("none")
    gl = torch.randn(M, V, generator=torch.Generator().manual_seed(5))
    for g_logits in (None, gl):
        logits, lse, loss, norm = run_head_fwd(a, wpad, bias, tgt)
        dl, db = run_head_bwd(logits, lse, tgt, norm, g_logits=g_logits)
        u_logits, u_lse, u_loss, u_dl, u_db = unmasked_head(a, wpad, bias, tgt, g_logits=g_logits)
        assert same_bits(logits, u_logits) and same_bits(lse, u_lse) and same_bits(loss, u_loss)
        assert same_bits(dl, u_dl) and same_bits(db, u_db)
        assert norm.tolist() == [float(M), float(torch.tensor(1.0) / torch.tensor(float(M)))]


@pytest.mark.parametrize("m", [M, 8200])
def test_ce_no_mask_is_bitwise_the_unmasked_ce(m):
    logits, tgt = ce_logits(m), targets("none", m)
    rows, lse, loss, norm = run_ce_fwd(logits, tgt)
    d32, d16 = run_ce_bwd(logits, lse, tgt, norm)
    u_rows, u_lse, u_loss = torch.empty(m, device=DEV), torch.empty(m, device=DEV), torch.empty((), device=DEV)
    ops().ce_fwd(logits, tgt.to(DEV), u_rows, u_lse)
    ops().sum_scaled(u_rows, 1.0 / m, u_loss, torch.empty(1024, device=DEV))
    u32, u16 = torch.empty(m, V, device=DEV), torch.empty(m, V, dtype=BF16, device=DEV)
    ops().ce_bwd(logits, tgt.to(DEV), u_lse, torch.full((1,), 2.0, device=DEV), 1.0 / m, u32, u16)
    assert same_bits(rows, u_rows) and same_bits(lse, u_lse) and same_bits(loss, u_loss)
    assert same_bits(d32, u32) and same_bits(d16, u16)
    assert norm.tolist() == [float(m), float(torch.tensor(1.0) / torch.tensor(float(m)))]


# ---------------------------------------------------------------------------------------
# 2. masks: F.cross_entropy in fp64 on the kernel's own logits
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", MASKED)
@pytest.mark.parametrize("C", [384, 128, 32])
def test_head_masked_matches_torch(C, pattern):
    a, wpad, bias = head_inputs(C)
    tgt = targets(pattern)
    ign = PATTERNS[pattern](M)
    logits, lse, loss, norm = run_head_fwd(a, wpad, bias, tgt)
    u_logits, u_lse = unmasked_head(a, wpad, bias, targets("none"))[:2]
    assert same_bits(logits, u_logits) and same_bits(lse, u_lse)      # written for every row, ignored or not
    count = int((~ign).sum())
    assert norm.tolist() == [float(count), float(torch.tensor(1.0) / torch.tensor(float(count)))]
    gl = torch.randn(M, V, generator=torch.Generator().manual_seed(6)).to(BF16).float()   # exact in dl's bf16
    for g_logits in (None, gl):
        ref_loss, want = reference(logits, tgt, 2.0, g_logits)
        print(f"head C {C} {pattern}: loss {float(loss):.7f} ref {ref_loss:.7f}")
        assert abs(float(loss) - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
        dl, db = run_head_bwd(logits, lse, tgt, norm, g_logits=g_logits)
        assert relerr(dl[:, :V], want) < 2e-2
        assert float(dl[:, V:].float().abs().max()) == 0.0
        assert relerr(db, 0.5 + want.sum(0)) < 1e-5
        if g_logits is None:
            assert not bits(dl[ign.to(DEV)]).any()                       # exactly +0
        else:
            assert same_bits(dl[ign.to(DEV)][:, :V], gl[ign].to(BF16))   # exactly g_logits


@pytest.mark.parametrize("pattern", MASKED)
def test_ce_masked_matches_torch(pattern):
    logits, tgt = ce_logits(), targets(pattern)
    ign = PATTERNS[pattern](M)
    rows, lse, loss, norm = run_ce_fwd(logits, tgt)
    ref_loss, want = reference(logits, tgt, 2.0)
    print(f"ce {pattern}: loss {float(loss):.7f} ref {ref_loss:.7f}")
    assert abs(float(loss) - ref_loss) < 1e-5
    assert norm[0].item() == float((~ign).sum())
    assert not bits(rows[ign.to(DEV)]).any()
    d32, d16 = run_ce_bwd(logits, lse, tgt, norm)
    assert relerr(d32, want) < 1e-5
    assert not bits(d32[ign.to(DEV)]).any() and not bits(d16[ign.to(DEV)]).any()
    assert same_bits(d16, d32.to(BF16))


def test_ce_mean_counts_across_virtual_blocks():
    m = 8200
    tgt = targets("every-other", m)
    rows, lse, loss, norm = run_ce_fwd(ce_logits(m), tgt)
    ref_loss, _ = reference(ce_logits(m), tgt)
    assert norm[0].item() == float(m // 2) and abs(float(loss) - ref_loss) < 1e-5


# ---------------------------------------------------------------------------------------
# 3. poison in the ignored rows
# ---------------------------------------------------------------------------------------
def poison_rows(t, ign):
    """NaN, +inf and -inf in turn over the ignored rows of a copy of t."""
    t = t.clone()
    vals = torch.tensor([float("nan"), float("inf"), float("-inf")], device=t.device)
    idx = ign.nonzero().flatten().to(t.device)
    shape = (-1,) + (1,) * (t.dim() - 1)
    t[idx] = vals[torch.arange(len(idx), device=t.device) % 3].reshape(shape).expand_as(t[idx]).to(t.dtype)
    return t


@pytest.mark.parametrize("pattern", MASKED)
@pytest.mark.parametrize("C", [384, 32])
def test_head_poison_in_ignored_rows_does_not_leak(C, pattern):
    a, wpad, bias = head_inputs(C)
    tgt = targets(pattern)
    ign = PATTERNS[pattern](M)
    keep = (~ign).to(DEV)
    logits, lse, loss, norm = run_head_fwd(a, wpad, bias, tgt)
    a_inf = a.clone()
    a_inf[ign.to(DEV)] = float("inf")
    p_logits, p_lse, p_loss, p_norm = run_head_fwd(a_inf, wpad, bias, tgt)
    assert not torch.isfinite(p_logits[ign.to(DEV)]).any()              # the poison did reach the ignored rows
    assert same_bits(p_loss, loss) and same_bits(p_norm, norm) and math.isfinite(float(loss))
    assert same_bits(p_logits[keep], logits[keep]) and same_bits(p_lse[keep], lse[keep])
    gl = torch.randn(M, V, generator=torch.Generator().manual_seed(6)).to(BF16).float()
    for g_logits in (None, gl):
        dl, db = run_head_bwd(logits, lse, tgt, norm, g_logits=g_logits)
        p_dl, p_db = run_head_bwd(poison_rows(logits, ign), poison_rows(lse, ign), tgt, norm, g_logits=g_logits)
        assert same_bits(p_dl, dl) and same_bits(p_db, db)


@pytest.mark.parametrize("pattern", MASKED)
def test_ce_poison_in_ignored_rows_does_not_leak(pattern):
    tgt = targets(pattern)
    ign = PATTERNS[pattern](M)
    keep = (~ign).to(DEV)
    logits = ce_logits()
    rows, lse, loss, norm = run_ce_fwd(logits, tgt)
    bad = poison_rows(logits, ign)
    p_rows, p_lse, p_loss, p_norm = run_ce_fwd(bad, tgt)
    assert same_bits(p_rows, rows) and same_bits(p_loss, loss) and same_bits(p_norm, norm) and math.isfinite(float(loss))
    assert same_bits(p_lse[keep], lse[keep])
    d32, d16 = run_ce_bwd(logits, lse, tgt, norm)
    p32, p16 = run_ce_bwd(bad, p_lse, tgt, norm)
    assert same_bits(p32, d32) and same_bits(p16, d16)


# ---------------------------------------------------------------------------------------
# 4. everything ignored, 5. a bad target
# ---------------------------------------------------------------------------------------
def test_all_ignored_is_nan_loss_and_zero_gradients():
    tgt = targets("all")
    a, wpad, bias = head_inputs(384)
    logits, lse, loss, norm = run_head_fwd(a, wpad, bias, tgt)
    assert math.isnan(float(loss)) and norm.tolist() == [0.0, float("inf")]
    dl, db = run_head_bwd(logits, lse, tgt, norm, db0=0.0)
    assert not bits(dl).any() and not bits(db).any()
    rows, lse, loss, norm = run_ce_fwd(ce_logits(), tgt)
    assert math.isnan(float(loss)) and norm.tolist() == [0.0, float("inf")]
    d32, d16 = run_ce_bwd(ce_logits(), lse, tgt, norm)
    assert not bits(d32).any() and not bits(d16).any()


@pytest.mark.parametrize("bad", [V, -1])
def test_bad_target_still_makes_the_loss_nan(bad):
    tgt = targets("every-other")
    tgt[10] = bad                       # row 10 is valid under this pattern
    a, wpad, bias = head_inputs(384)
    assert math.isnan(float(run_head_fwd(a, wpad, bias, tgt)[2]))
    assert math.isnan(float(run_ce_fwd(ce_logits(), tgt)[2]))


# ---------------------------------------------------------------------------------------
# 7. cg_gather_pairs
# ---------------------------------------------------------------------------------------
def test_gather_pairs_matches_the_reference():
    T, PAD = 64, 3
    s = pr.train_sampler(device=DEV)
    s.pad_token = PAD
    full = [n for n in range(len(pr.TRAIN_PAIRS)) if int(s.tlen_cpu[n]) == T + 1]
    one = [([9, 8, 7, 6], [5])]                                          # plen = tlen - 1: a single valid target
    from replicatinggpt_amd.data import PairSampler
    s1 = PairSampler(pr.TRAIN_PAIRS + one, T, 4, device=DEV, pad_token=PAD)
    assert full and int(s1.plen_cpu[-1]) == int(s1.tlen_cpu[-1]) - 1
    ix = list(range(len(pr.TRAIN_PAIRS) + 1))
    xb, yb = Box(len(ix), T, I64, device=DEV), Box(len(ix), T, I64, device=DEV)
    ops().gather_pairs(s1.table_dev, s1.plen_dev, s1.tlen_dev, torch.tensor(ix, device=DEV), xb.view, yb.view, PAD, IGN)
    torch.cuda.synchronize()
    clean(x=xb, y=yb)
    rx, ry = pr.reference_batch(pr.TRAIN_PAIRS + one, ix, T, pad=PAD)
    assert torch.equal(xb.view.cpu(), rx) and torch.equal(yb.view.cpu(), ry)
    assert int((ry[-1] != IGN).sum()) == 1 and int((ry[full[0]] != IGN).sum()) == len(pr.TRAIN_PAIRS[full[0]][1])
    # get_batch: the drawn rows, in the draw's order
    g = torch.Generator().manual_seed(pr.SAMPLER_SEED)
    want = torch.randint(s.n, (s.B,), generator=g).tolist()
    x, y = s.get_batch("train")
    rx, ry = pr.reference_batch(pr.TRAIN_PAIRS, want, T, pad=PAD)
    assert torch.equal(x.cpu(), rx) and torch.equal(y.cpu(), ry)
