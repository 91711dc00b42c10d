"""CPU side of the numerics tests (tests/numerics.py): the data profiles have the properties they
claim, the plain implementations stay inside the rigorous caps, the element-wise budget rho reports
every planted fault on the profile built for it -- while the same fault passes the parity tests' own
bar (relerr < 1e-5, or bf16_close) -- and the power-of-two scaling checker reports bitwise equality
on torch's CPU kernels.  No GPU; test_gpu_numerics.py runs the same budgets on the library."""
import math

import pytest
import torch

import numerics as nm
from conftest import bf16_close
from numerics import BF16, F64, MARGIN, U32, UBF, relerr, rho


def gen(seed=0):
    return torch.Generator().manual_seed(seed)


# ---- profile properties ------------------------------------------------------------------------------------
def test_peaked_profile_is_peaked_in_every_class():
    B, T, H, D = 2, 192, 2, 64
    q, k, v, scale = nm.attn_operands(gen(1), B, T, H, D, "peaked")
    q, k = nm.rnd(q, BF16), nm.rnd(k, BF16)
    s, _, P = nm.attn_scores(q, k, scale)
    top = P.max(-1).values[..., 8:]                      # [B, H, T - 8]
    t = torch.arange(8, T)
    assert float((top > 0.9).double().mean()) >= 0.5
    for cls in range(4):
        assert int((top[..., t % 4 == cls] > 0.9).sum()) > 0, f"class t mod 4 == {cls} has no peaked row"
    assert float((top < 0.5).double().mean()) >= 0.01
    assert 8 < float(s[torch.isfinite(s)].abs().max()) < 40


def test_unit_profile_is_near_uniform():
    """The control: the parity tests' data gives a median largest weight of a few percent."""
    q, k, v, scale = nm.attn_operands(gen(1), 2, 192, 2, 64, "unit")
    P = nm.attn_scores(nm.rnd(q, BF16), nm.rnd(k, BF16), scale)[2]
    assert float(P.max(-1).values[..., 8:].median()) < 0.05


def test_sink_profile_attends_key_zero():
    q, k, v, scale = nm.attn_operands(gen(2), 2, 64, 2, 64, "sink")
    P = nm.attn_scores(nm.rnd(q, BF16), nm.rnd(k, BF16), scale)[2]
    assert float((P[..., 0] > 0.9).double().mean()) >= 0.5


def test_shifted_profile_keeps_the_softmax():
    B, T, H, D = 2, 64, 2, 64
    q, k, v, scale = nm.attn_operands(gen(3), B, T, H, D, "unit")
    q2, k2, v2, scale2 = nm.attn_operands(gen(3), B, T, H, D, "shifted")
    assert torch.equal(q, q2) and torch.equal(v, v2) and scale == scale2
    s, _, P = nm.attn_scores(q, k, scale)
    s2, _, P2 = nm.attn_scores(q2, k2, scale)
    assert float((P - P2).abs().max()) < 1e-12
    shift = (s2 - s)[:, :, :, 0].abs()                   # one amount per row
    assert 30 < float(shift.median()) < 150 and float(shift.max()) > 100


def test_spiked_profile_is_the_rescale_test_s_data():
    """At T = 512 the operands are test_attention_forward_rescale_branch's, bit for bit."""
    B, T, H, D = 1, 512, 2, 64
    d = H * D
    torch.manual_seed(31)
    qkv = torch.randn(B * T, 3 * d) * 0.5
    qkv[:, :d] += 2.0
    qkv[300, d:2 * d] = 8.0
    qkv[:, d:2 * d][:, :D] *= torch.linspace(0.1, 3.0, T)[:, None]
    q, k, v, scale = nm.attn_operands(gen(0), B, T, H, D, "spiked")
    assert torch.equal(torch.cat([t.reshape(B * T, d) for t in (q, k, v)], 1).float(), qkv) and scale == D ** -0.5
    # and at the T the GPU tests use, the running max still jumps by more than 2^8 (in log2 units: 8
    # / log2(e) = 5.5 in score units) at the spiked key's tile
    q, k, v, scale = nm.attn_operands(gen(0), 1, 192, 2, 64, "spiked")
    s = nm.attn_scores(nm.rnd(q, BF16), nm.rnd(k, BF16), scale)[0]
    spike = 300 * 192 // 512
    before = s[0, 0, -1, :spike // 64 * 64].max()
    assert float(s[0, 0, -1, spike] - before) > 8 / math.log2(math.e)


@pytest.mark.parametrize("C", [33, 384])
def test_layernorm_profiles(C):
    rows, eps = 66, nm.EPS
    x = nm.ln_rows(gen(4), rows, C, "flat").double()
    var = x.var(1, unbiased=False)
    assert int((var == 0).sum()) == rows // 2 and bool((var[1::2] > 0).all()) and float(var.max()) < eps
    x = nm.ln_rows(gen(4), rows, C, "offset").double()
    assert float((x.mean(1).abs() / x.std(1)).min()) >= 1000 * 0.85      # std of C samples of a unit normal
    assert float(x.mean(1).abs().min()) >= 1024 and float(x.mean(1).abs().max()) <= 2048 + 1
    g = gen(4)
    base = nm.ln_rows(g, rows, C, "unit")
    out = nm.ln_rows(gen(4), rows, C, "outlier")
    ratio = (out / base).abs().median(0).values
    assert int((ratio > 63).sum()) == 4 and int((ratio < 1.01).sum()) == C - 4


def test_gemm_outlier_profile():
    A, W, info = nm.gemm_operands(gen(5), 64, 96, 192, "outlier")
    A0, W0, _ = nm.gemm_operands(gen(5), 64, 96, 192, "unit")
    assert torch.equal(A[:, info["a_cols"]], A0[:, info["a_cols"]] * 64) and torch.equal(W[info["w_rows"]], W0[info["w_rows"]] * 64)
    assert torch.equal(A.to(BF16).float(), A)            # bf16 values


def test_certain_profile_underflows_every_other_weight():
    x, tgt = nm.ce_logits(gen(6), 64, 200, "certain")
    r = torch.arange(64)
    hit = r % 4 != 3
    rest = x.clone()
    rest[r, tgt] = -math.inf
    assert bool(((x[r, tgt] - rest.max(1).values)[hit] >= 99.99).all()) and float(torch.exp(torch.tensor(-99.99))) < nm.TINY
    assert math.isinf(float(torch.exp(torch.tensor(99.99))))
    assert int((tgt[hit] >= 64).sum()) > 0


@pytest.mark.parametrize("profile", ["confident", "wrong", "offset"])
def test_cross_entropy_and_head_profiles(profile):
    rows, V = 64, 65
    x, tgt = nm.ce_logits(gen(6), rows, V, profile)
    M, C = 64, 96
    a, W, bias, htgt = nm.head_operands(gen(6), M, C, V, profile)
    hx = a.double() @ W.double().t() + bias.double()
    for lg, t in ((x.double(), tgt), (hx, htgt)):
        r = torch.arange(lg.shape[0])
        hit = r % 4 != 3
        xt = lg[r, t]
        rest = lg.clone()
        if profile == "confident":
            rest[r, t] = -math.inf
            assert bool(((xt - rest.max(1).values)[hit] >= 29.99).all())
        elif profile == "wrong":
            rest[r, t] = math.inf
            assert bool(((rest.min(1).values - xt)[hit] >= 29.99).all())
        else:
            assert float(lg[hit].min()) > 980
        assert int((~hit).sum()) > 0                     # some rows stay unit


def test_embedding_profile():
    idx, dx, hot = nm.embed_operands(gen(7), 65, 40, 126, 3)
    assert float((idx == hot).double().mean()) >= 0.85


# ---- rigorous caps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["unit", "outlier"])
@pytest.mark.parametrize("M,N,K", [(256, 384, 192), (37, 65, 126)])
def test_gemm_plain_inside_the_cap(profile, M, N, K):
    A, W, _ = nm.gemm_operands(gen(8), M, N, K, profile)
    bias = torch.randn(N, generator=gen(9))
    ref, S = nm.gemm_budget(A, W, bias=bias)
    for chunk in (None, 32):
        r = rho(nm.gemm_plain(A, W, bias=bias, chunk=chunk), ref, S, U32)
        assert r.value <= nm.dot_cap(K, 1), (chunk, str(r))
    r = rho(nm.gemm_plain(A, W, bias=bias, out_dtype=BF16), ref, S, UBF)
    assert r.value <= nm.dot_cap(K, 1, BF16), str(r)


def test_sum_and_mean_plain_inside_the_cap():
    x = nm.ln_rows(gen(10), 257, 384, "outlier")
    ref, S = nm.sum_budget(x, 0)
    assert nm.sum_rho_plain(x, ref, S, 0) <= 257 + 2
    b = nm.ln_fwd_budget(x, *nm.ln_params(gen(11), 384))
    for order in ("torch", "twopass"):
        mu = nm.ln_fwd_plain(x, *nm.ln_params(gen(11), 384), order=order)[1]
        assert rho(mu, *b["mean"], U32).value <= 384 + 2


def test_embedding_plain_inside_the_cap():
    idx, dx, _ = nm.embed_operands(gen(7), 65, 40, 126, 3)
    b, got = nm.embed_budget(idx, dx, 65), nm.embed_plain(idx, dx, 65)
    assert rho(got["dwte"], *b["dwte"], U32).value <= 3 * 40 + 2 and rho(got["dwpe"], *b["dwpe"], U32).value <= 3 + 2


def test_rho_reports_the_worst_element():
    ref, S = torch.zeros(3, 4, dtype=F64), torch.ones(3, 4, dtype=F64)
    got = torch.zeros(3, 4)
    got[1, 2] = 5 * U32
    r = rho(got, ref, S, U32)
    assert abs(r.value - 5) < 1e-6 and r.index == (1, 2) and r.S == 1 and "rho 5" in str(r)
    got[2, 3] = float("nan")
    assert rho(got, ref, S, U32).value == math.inf and rho(got, ref, S, U32).index == (2, 3)
    assert rho(torch.ones(2), torch.ones(2, dtype=F64), torch.zeros(2, dtype=F64), U32).value == 0
    assert rho(torch.ones(2), torch.zeros(2, dtype=F64), torch.zeros(2, dtype=F64), U32).value > 1e30       # S = 0: any error is huge
    assert rho(torch.zeros(1), torch.full((1,), 1e-60, dtype=F64), torch.full((1,), 1e-60, dtype=F64), U32).value < 1e-20   # underflow


# ---- planted faults ----------------------------------------------------------------------------------------
FAULTS = []      # (fault, profile, rho_plain, rho_fault, passes today's bar on)


def _record(name, profile, rp, rf, passes_on):
    FAULTS.append((name, profile, rp, rf, passes_on))
    assert rf > MARGIN * rp, f"{name} on {profile}: rho_fault {rf:.4g} is within {MARGIN} x rho_plain {rp:.4g}"


def test_fault_gemm_ordinary_columns():
    """Every ordinary column of a GEMM output off by 3e-4 relative.  On unit data the parity bar sees
    it (all columns have the scale of the maximum); on outlier data -- where the outlier columns set
    max|ref| -- relerr stays below 1e-5 and bf16_close passes, and only rho reports it."""
    M, N, K = 256, 384, 192
    A, W, info = nm.gemm_operands(gen(20), M, N, K, "outlier")
    ref, S = nm.gemm_budget(A, W)
    ordinary = torch.ones(N, dtype=torch.bool)
    ordinary[info["w_rows"]] = False
    bad = nm.gemm_plain(A, W)
    bad[:, ordinary] *= 1 + 3e-4
    assert relerr(bad, ref) < 1e-5 and bf16_close(nm.rnd(bad, BF16), ref)[0]          # today's bars pass
    _record("gemm: ordinary columns off by 3e-4", "outlier", nm.gemm_rho_plain(A, W, ref, S),
            rho(bad, ref, S, U32).value, "outlier")
    A, W, _ = nm.gemm_operands(gen(20), M, N, K, "unit")
    ref, S = nm.gemm_budget(A, W)
    assert relerr(nm.gemm_plain(A, W) * (1 + 3e-4), ref) > 1e-5      # unit data: today's bar does see it


def _ln_one_pass(x, w, b, eps=nm.EPS):
    x = x.float()
    mu = x.mean(1, keepdim=True)
    var = (x * x).mean(1, keepdim=True) - mu * mu
    return (x - mu) / torch.sqrt(var.clamp(min=0) + eps) * w + b


def _ln_eps_outside(x, w, b, eps=nm.EPS):
    x = x.float()
    mu = x.mean(1, keepdim=True)
    d = x - mu
    return d / (torch.sqrt((d * d).mean(1, keepdim=True)) + eps) * w + b


@pytest.mark.parametrize("name,fault,profile", [("layernorm: one-pass variance", _ln_one_pass, "offset"),
                                                ("layernorm: eps added after the square root", _ln_eps_outside, "flat")])
def test_fault_layernorm(name, fault, profile):
    rows, C = 67, 384
    w, b = nm.ln_params(gen(21), C)
    x = nm.ln_rows(gen(22), rows, C, "unit")
    assert relerr(fault(x, w, b), nm.ln_fwd_budget(x, w, b)["y"][0]) < 1e-5           # today's bar passes on unit
    x = nm.ln_rows(gen(22), rows, C, profile)
    bud = nm.ln_fwd_budget(x, w, b)
    _record(name, profile, nm.ln_fwd_rho_plain(x, w, b, bud)["y"], rho(fault(x, w, b), *bud["y"], U32).value, "unit")


def test_fault_softmax_scale():
    """A softmax scale 3 % off, judged on o alone (dq and dk carry the scale as a factor and are
    caught by any bar): passes bf16_close on unit data, outside the budget on peaked rows."""
    B, T, H, D = 2, 192, 2, 64
    for profile in ("unit", "peaked"):
        q, k, v, scale = nm.attn_operands(gen(23), B, T, H, D, profile)
        q, k, v = (nm.rnd(t, BF16) for t in (q, k, v))
        dO = torch.zeros_like(q)
        bud = nm.attn_budget(q, k, v, dO, scale)
        bad = nm.attn_plain(q, k, v, dO, scale * 1.03, round_p=True)["o"]
        if profile == "unit":
            assert bf16_close(bad, bud["o"][0])[0]
        else:
            good = nm.attn_plain(q, k, v, dO, scale, round_p=True)["o"]
            _record("attention: softmax scale off by 3 %", profile, rho(good, *bud["o"], UBF).value,
                    rho(bad, *bud["o"], UBF).value, "unit")


def test_fault_small_softmax_weights_dropped():
    """Weights below 2^-20 of the row maximum dropped (an absolute threshold in the exponent), fp32:
    nothing to drop on unit data, far outside the budget on peaked rows."""
    B, T, H, D = 2, 192, 2, 64

    def run(profile, drop):
        q, k, v, scale = nm.attn_operands(gen(24), B, T, H, D, profile)
        q, k, v = (nm.rnd(t, BF16) for t in (q, k, v))
        bud = nm.attn_budget(q, k, v, torch.zeros_like(q), scale, fp32_cond=True)
        s, _, _ = nm.attn_scores(q, k, scale)
        s = s.float()
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        if drop:
            p = torch.where(p < 2.0 ** -20, torch.zeros_like(p), p)
        o = torch.einsum("bhts,bshd->bthd", p, v.float()) / p.sum(-1).permute(0, 2, 1)[..., None]
        return o, bud["o"]

    o, (ref, S) = run("unit", True)
    assert relerr(o, ref) < 1e-5
    good, (ref, S) = run("peaked", False)
    bad, _ = run("peaked", True)
    _record("attention: weights below 2^-20 of the row maximum dropped", "peaked", rho(good, ref, S, U32).value,
            rho(bad, ref, S, U32).value, "unit")


def test_fault_logsumexp_without_the_max():
    rows, V = 64, 65
    x, tgt = nm.ce_logits(gen(25), rows, V, "unit")
    naive = torch.log(torch.exp(x).sum(1))
    assert relerr(naive, nm.ce_budget(x, tgt)["lse"][0]) < 1e-5
    x, tgt = nm.ce_logits(gen(25), rows, V, "offset")
    bud = nm.ce_budget(x, tgt)
    naive = torch.log(torch.exp(x).sum(1))
    assert not bool(torch.isfinite(naive).all())
    _record("cross entropy: log(sum(exp(x))) without the max", "offset", rho(nm.ce_plain(x, tgt)["lse"], *bud["lse"], U32).value,
            rho(naive, *bud["lse"], U32).value, "unit")


def test_fault_lse_rounded_to_bf16():
    """dlogits = exp(x - lse) - onehot with lse rounded to bf16.  This fault passes today's bars on no
    profile (not forced): a bf16 lse moves every probability by up to 2^-8 |lse| relative, 2.4 % on unit
    data, which the fp32 bar (1e-5) and the head's bf16 bar (2e-2) both see.  Recorded for rho only."""
    rows, V = 64, 65

    def run(profile):
        x, tgt = nm.ce_logits(gen(26), rows, V, profile)
        lse = nm.ce_plain(x, tgt)["lse"]
        bud = nm.ce_budget(x, tgt, lse_in=lse)
        good = nm.ce_plain(x, tgt, lse_in=lse)["dlogits"]
        bad = nm.ce_plain(x, tgt, lse_in=nm.rnd(lse, BF16))["dlogits"]
        return good, bad, bud["dlogits"]

    good, bad, (ref, S) = run("unit")
    assert relerr(bad, ref) > 1e-5 and relerr(nm.rnd(bad, BF16), ref) > 2e-2
    good, bad, (ref, S) = run("confident")
    _record("cross entropy: lse rounded to bf16", "confident", rho(good, ref, S, U32).value, rho(bad, ref, S, U32).value,
            "no profile")


# ---- the inference path: a CPU stand-in of decode.hip's online softmax and of its log-probability --------------
DEC = dict(B=2, T=130, H=2)
DEC_PROFILES = ("unit", "peaked", "sink", "shifted", "spiked")


def _online_softmax(q, k, v, scale, fault=None, chunk=64):
    """nm.decode_attn_plain with a place for each planted fault (fault None: the same bits)."""
    q, k, v = (t.float() for t in (q, k, v))
    B, T, H, D = q.shape
    raw = torch.einsum("bthd,bshd->bhts", q, k)
    vis = torch.tril(torch.ones(T, T, dtype=torch.bool))
    if fault == "last key dropped":          # n - 1 keys where there are at least two
        vis = vis & ~torch.diag(torch.arange(T) >= 1)
    s = (raw * torch.tensor(scale, dtype=torch.float32)).masked_fill(~vis, -math.inf)
    stat = raw.masked_fill(~vis, -math.inf) if fault == "scale applied after the max" else s
    m = torch.full((B, H, T, 1), -math.inf)
    l = torch.zeros(B, H, T, 1)
    acc = torch.zeros(B, H, T, D)
    for c0 in range(0, T, chunk):
        sc = s[..., c0:c0 + chunk]
        m_new = torch.maximum(m, stat[..., c0:c0 + chunk].max(-1, keepdim=True).values)
        alpha = torch.exp(m - m_new)
        arg = sc - m_new
        if fault == "exp argument rounded to bf16":
            arg = nm.rnd(arg, BF16)
        p = torch.exp(arg)
        l = (l if fault == "l not rescaled" else l * alpha) + p.sum(-1, keepdim=True)
        acc = acc * alpha + torch.einsum("bhts,bshd->bhtd", p, v[:, c0:c0 + chunk])
        m = m_new
    if fault == "stale key admitted":        # the zero row past n: score 0, value 0, weight exp(0 - m)
        l = l + torch.exp(0 - m)
    return (acc * (1.0 / l)).permute(0, 2, 1, 3).contiguous()


def _dec_case(D, profile):
    q, k, v, scale = nm.attn_operands(gen(5), DEC["B"], DEC["T"], DEC["H"], D, profile)
    q, k, v = (nm.rnd(t, nm.F32) for t in (q, k, v))
    ref, S = nm.attn_budget(q, k, v, torch.zeros_like(q), scale, fp32_cond=True)["o"]
    return q, k, v, scale, ref, S


@pytest.mark.parametrize("D", [21, 64])
def test_online_softmax_plain_orders_agree(D):
    """The stand-in without a fault is nm.decode_attn_plain bit for bit, and the two plain orders of
    the GPU bar are inside MARGIN of each other on every profile (per row the bar uses the larger)."""
    for profile in DEC_PROFILES:
        q, k, v, scale, ref, S = _dec_case(D, profile)
        online = nm.decode_attn_plain(q, k, v, scale)
        assert torch.equal(online, _online_softmax(q, k, v, scale))
        a = rho(nm.attn_plain(q, k, v, torch.zeros_like(q), scale, dtype=nm.F32)["o"], ref, S, U32).value
        b = rho(online, ref, S, U32).value
        assert max(a, b) <= MARGIN * min(a, b), (profile, a, b)
        assert float(nm.decode_attn_rho_plain(q, k, v, scale, ref, S).max()) == max(a, b)


def test_max_norm_bar_cannot_referee_shifted():
    """A correct plain online softmax misses the parity tests' 1e-5 max-norm bar on shifted data at D 64."""
    q, k, v, scale, ref, S = _dec_case(64, "shifted")
    assert relerr(nm.decode_attn_plain(q, k, v, scale), ref) > 1e-5


# fault, the profile whose budget catches it, the profiles on which it passes the 1e-5 max-norm bar
DEC_FAULTS = [("l not rescaled", "spiked", ("sink",)), ("last key dropped", "peaked", ()), ("stale key admitted", "sink", ()),
              ("scale applied after the max", "shifted", ("unit", "peaked", "sink")),
              ("exp argument rounded to bf16", "peaked", ())]


@pytest.mark.parametrize("fault,profile,bar_passes", DEC_FAULTS)
def test_fault_online_softmax(fault, profile, bar_passes):
    """Each fault is far outside the budget on the profile built for it (D 21 and D 64), and the 1e-5
    max-norm bar passes it on exactly the profiles stated (none: the bar sees that fault on all five)."""
    for D in (21, 64):
        q, k, v, scale, ref, S = _dec_case(D, profile)
        rp = float(nm.decode_attn_rho_plain(q, k, v, scale, ref, S).max())
        rf = rho(_online_softmax(q, k, v, scale, fault), ref, S, U32).value
        passes = []
        for prof in DEC_PROFILES:
            q2, k2, v2, sc2, ref2, _ = _dec_case(D, prof)
            if relerr(_online_softmax(q2, k2, v2, sc2, fault), ref2) < 1e-5:
                passes.append(prof)
        assert tuple(passes) == bar_passes, (fault, D, passes)
        _record(f"decode attention D {D}: {fault}", profile, rp, rf, ", ".join(passes) or "no profile")


def _logprob(x, tgt, fault=None):
    """nm.logprob_plain(order="formula") with a place for each planted fault."""
    x = x.float()
    r = torch.arange(x.shape[0])
    m = (x[:, :64] if fault == "max over the first 64 columns" else x).max(1).values
    arg = x - m[:, None]
    if fault == "exp argument rounded to bf16":
        arg = nm.rnd(arg, BF16)
    return (x[r, tgt] - m) - torch.log(torch.exp(arg).sum(1))


@pytest.mark.parametrize("fault,profile,bar_passes", [("max over the first 64 columns", "certain", ("unit", "confident", "wrong", "offset")),
                                                      ("exp argument rounded to bf16", "wrong", ())])
def test_fault_logprob(fault, profile, bar_passes):
    """V 200, 64 rows.  A maximum over the first 64 columns alone leaves the formula valid in exact
    arithmetic (it is shift-invariant), and in fp32 too as long as nothing overflows: with a missed
    margin d both terms grow by d, but |ref| or the common rounding of x_t - m grows with them, so on
    `confident` (d = 30) the fault stays inside one u S (measured: rho 0.92 against 0.71 plain) and no
    bar can see it.  It becomes an error where exp(d) leaves fp32's range: `certain` (d = 100) on the
    rows whose target lies past column 64 gives -inf."""
    rows, V = 64, 200
    x, tgt = nm.ce_logits(gen(27), rows, V, profile)
    assert torch.equal(_logprob(x, tgt), nm.logprob_plain(x, tgt, "formula"))
    ref, S = nm.logprob_budget(x, tgt)
    passes = []
    for prof in ("unit", "confident", "wrong", "offset"):
        x2, t2 = nm.ce_logits(gen(27), rows, V, prof)
        if relerr(_logprob(x2, t2, fault), nm.logprob_budget(x2, t2)[0]) < 1e-5:
            passes.append(prof)
    assert tuple(passes) == bar_passes, (fault, passes)
    _record(f"log-probability: {fault}", profile, nm.logprob_rho_plain(x, tgt, ref, S), rho(_logprob(x, tgt, fault), ref, S, U32).value,
            ", ".join(passes) or "no profile")


@pytest.mark.parametrize("V", [65, 200])
def test_logprob_plain_orders_agree(V):
    for profile in ("unit", "confident", "wrong", "offset", "certain"):
        x, tgt = nm.ce_logits(gen(28), 64, V, profile)
        ref, S = nm.logprob_budget(x, tgt)
        a, b = (rho(nm.logprob_plain(x, tgt, o), ref, S, U32).value for o in ("torch", "formula"))
        assert max(a, b) <= MARGIN * max(min(a, b), 0.25) and max(a, b) < 8, (profile, a, b)
    # shift-invariant: the budget of offset rows is the budget of the same rows without the offset
    x, tgt = nm.ce_logits(gen(28), 64, V, "unit")
    r0, S0 = nm.logprob_budget(x, tgt)
    r1, S1 = nm.logprob_budget(x.double() + 1024.0, tgt)
    assert float((r0 - r1).abs().max()) < 1e-11 and float((S0 - S1).abs().max()) < 1e-11


def test_inference_rows_plain_inside_their_budgets():
    """linear_ln_budget / ffn_budget: the plain fp32 forms stay at rho of order 1 on offset, flat and
    outlier data, and a second product fed a bf16-rounded hidden activation does not."""
    M, C, Hh = 33, 126, 504
    for profile in ("offset", "flat"):
        g = gen(29)
        a = nm.ln_rows(g, M, C, profile)
        lw, lb = nm.ln_params(g, C)
        W1, b1 = torch.randn(Hh, C, generator=g) / C ** 0.5, torch.randn(Hh, generator=g)
        W2, b2, resid = torch.randn(C, Hh, generator=g) / Hh ** 0.5, torch.randn(C, generator=g), torch.randn(M, C, generator=g)
        ref, S = nm.linear_ln_budget(a, lw, lb, W1, b1, relu=True)
        assert nm.linear_ln_rho_plain(a, lw, lb, W1, ref, S, b1, relu=True) < 16
        ref, S = nm.ffn_budget(a, lw, lb, W1, b1, W2, b2, resid)
        rp = nm.ffn_rho_plain(a, lw, lb, W1, b1, W2, b2, resid, ref, S)
        assert rp < 16
        h = nm.rnd(torch.relu(nm.ln_fwd_plain(a, lw, lb)[0] @ W1.t() + b1), BF16)
        assert rho(resid + (h @ W2.t() + b2), ref, S, U32).value > MARGIN * rp


def test_planted_faults_table():
    """Every planted fault was reported; prints the record (-s shows it).  Runs after the fault tests:
    pytest keeps the file's order."""
    assert len(FAULTS) == 7 + 2 * 5 + 2, [f[0] for f in FAULTS]
    print("\nfault | profile | rho_plain | rho_fault | passes today's bar on")
    for f in FAULTS:
        print(f"  {f[0]} | {f[1]} | {f[2]:.3g} | {f[3]:.3g} | {f[4]}")


# ---- exact scaling on the CPU ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-24, 24])
def test_scaling_checker_on_torch_cpu(k):
    A, W, _ = nm.gemm_operands(gen(30), 256, 384, 192, "unit")
    base = A @ W.t()
    assert nm.scaled_equal(base, (A * 2.0 ** k) @ W.t(), k) and nm.scaled_equal(base, A @ (W * 2.0 ** k).t(), k)
    rows, C = 67, 384
    x, (w, b) = nm.ln_rows(gen(31), rows, C, "unit"), nm.ln_params(gen(32), C)
    dy = torch.randn(rows, C, generator=gen(33))
    _, mu, rstd = nm.ln_fwd_plain(x, w, b)
    for order in ("torch", "formula"):
        one, two = nm.ln_bwd_plain(dy, x, w, mu, rstd, order=order), nm.ln_bwd_plain(dy * 2.0 ** k, x, w, mu, rstd, order=order)
        for name in ("dx", "dw", "db"):
            assert nm.scaling_mismatch(one[name], two[name], k) == "", (order, name)
    q, kk, v, scale = nm.attn_operands(gen(34), 2, 64, 2, 64, "unit")
    q, kk, v = (nm.rnd(t, BF16) for t in (q, kk, v))
    dO = nm.rnd(torch.randn(2, 64, 2, 64, generator=gen(35)), BF16)
    one = nm.attn_plain(q, kk, v, dO, scale, round_p=True)
    two = nm.attn_plain(q, kk, v * 2.0 ** k, dO, scale, round_p=True)
    assert nm.scaled_equal(one["o"], two["o"], k) and torch.equal(one["lse"], two["lse"])
    two = nm.attn_plain(q, kk, v, dO * 2.0 ** k, scale, round_p=True)
    for name in ("dq", "dk", "dv"):
        assert nm.scaling_mismatch(one[name], two[name], k) == "", name
    # and the checker can fail: an absolute epsilon breaks the scaling
    assert not nm.scaled_equal(base + 1e-3, (A * 2.0 ** k) @ W.t() + 1e-3, k)
    assert "differ" in nm.scaling_mismatch(base + 1e-3, (A * 2.0 ** k) @ W.t() + 1e-3, k)


def test_adamw_numpy_restatement_handles_the_edges():
    """The numpy restatement the GPU test compares cg_adamw with: finite inputs, and the documented
    overflow (v = 3.3e38, |g| = 2e20: v = inf, the update 0) and underflow (|g| = 1e-30: v stays 0) outcomes."""
    import numpy as np
    p, g, m, v = nm.adamw_edge_state()
    P, M, V = nm.adamw_numpy(p, g, m, v, 3e-3, 0.9, 0.999, 1e-8, 1e-2, 1000)
    i = np.arange(p.size) % 16
    assert np.isinf(V[i == 15]).all() and np.isfinite(V[i != 15]).all() and np.isfinite(P).all() and not np.isnan(M).any()
    assert (V[(i == 1) | (i == 2)] == 0).all() and (V[(i == 3) | (i == 4)] > 0).all() and (V[(i == 3) | (i == 4)] < 1.2e-38).all()
    assert (P[i == 0] == (p[i == 0] * np.float32(1 - 3e-3 * 1e-2)).astype(np.float32)).all()
    assert np.array_equal(nm.fma32(np.float32(3), np.float32(5), np.float32([7])), np.float32([22]))
