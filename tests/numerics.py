"""Ill-scaled data and element-wise error budgets for the numerics tests (test_cpu_numerics.py,
test_gpu_numerics.py).

The parity tests of the training kernels draw operands near unit scale and judge a result by one
number, max|got - ref| / max|ref|.  Both hide faults: a regime that is never visited (peaked softmax
rows, LayerNorm rows far from zero mean, confident logits) cannot fail, and with outlier channels in
the data the max-norm forgives every ordinary element an error far above its own rounding.  This
module holds the three things the tests share.

DATA PROFILES.  Functions of a torch.Generator that return CPU tensors (so test_cpu_numerics.py can
assert each profile's stated property): `unit` is what the parity tests use and serves as control;
`outlier`, `offset`, `flat` (GEMM / LayerNorm / reductions), `peaked`, `sink`, `shifted`, `spiked`
(attention), `confident`, `wrong`, `offset`, `certain` (cross entropy, head and log-probabilities).

BUDGETS.  For an output element let S be the sum of the absolute values of the terms that add up to
it: the reference formula evaluated in fp64 with every operand replaced by its absolute value and
every subtraction by an addition.  rho = max over elements of |got - ref| / (u S + 2^-126), u = 2^-24 where
the kernel accumulates and stores fp32 and u = 2^-9 where a bf16 rounding lies on the path of the
output (bf16's RNE rounding is up to 2^-8 relative, so one such rounding alone costs rho up to 2).  A correct implementation has rho of order 1 to 20 whatever the
scale of the data; a wrong one is off by orders of magnitude on the profile that exercises the
fault.  Softmax weights P are held at their reference values inside S; on the fp32 paths S carries
their own conditioning P (1 + |s| + |lse|) (an exp argument s - lse formed in fp32 is off by
u (|s| + |lse|), which is P's relative error).  The quantities that are no plain sums (rstd, lse)
use the first-order propagation of the same per-term errors; each *_budget function states it.

WHICH ROUNDINGS u COUNTS (by kernel, with the place in replicatinggpt_amd/csrc/):
  cg_gemm, fp32 output            u = 2^-24: fp32 MFMA accumulation and the fp32 epilogue
                                  (gemm_tile.h / gemm_pk.hip / gemm_p8.hip / gemm_f32.hip epilogues).
  cg_gemm, bf16 output            u = 2^-9: the one RNE rounding of the stored value (pack_bf2 in the
                                  epilogues); ReLU keep bits, column partials and row dots are
                                  functions of the STORED values and are judged from them
                                  (column partials / row dots: fp32 sums, u = 2^-24).
  cg_gemm split-K, bf16 slabs     u = 2^-9: each split's partial sum is rounded once to bf16
                                  (CG_GEMM_SLAB_BF16, gemm_pk.hip slab store) before the fp32 fold.
  cg_gemm_wgrad_group             as cg_gemm split-K (gemm_pk_group.hip runs the same tiles).
  cg_gemm_resid_layernorm         x: u = 2^-24 (the GEMM); y: 2^-9 (bf16 store of ln_fwd_row);
                                  mean / rstd: 2^-24 -- the three judged as the LayerNorm of the x
                                  the launch wrote (gemm_ln.hip calls ln_fwd.h ln_fwd_row on it).
  cg_layernorm_fwd[_attn_dropmask] ln_fwd.h ln_fwd_row: two passes in fp32, u = 2^-24; bf16 y 2^-9.
  cg_layernorm_bwd / _ex / _rows + _reduce   layernorm.hip k_ln_bwd: fp32 throughout, u = 2^-24 for
                                  dx, dw, db; the GradLink copy is bf16(keep ? dx / (1 - p) : 0) of
                                  the written dx (bitwise), its column sums fp32 (u = 2^-24).
  cg_linear_rows_f32, cg_decode_qkv_f32, cg_ffn_fwd_f32   rows_f32.hip (and gemm_f32.hip k_gemm_f32r at
                                  M <= 2048): the fp32 LayerNorm of ln_fwd.h, fp32 fmaf products, the fp32
                                  epilogue; the FFN's hidden activations stay fp32 registers: u = 2^-24
                                  everywhere (linear_ln_budget, ffn_budget).  The cache rows
                                  cg_decode_qkv_f32 appends are copies (bitwise).
  cg_decode_attn, cg_decode_prefill_attn   decode.hip attn_chunk / attn_finish: the score an fp32 fmaf
                                  chain times scale, __expf of fp32 differences against the running
                                  maximum of 64-key chunks, alpha = __expf(m - m_new) on l and acc, fp32
                                  fmaf accumulation, one * (1 / l): u = 2^-24 with the conditioning of P
                                  in S (attn_budget fp32_cond), as the fp32 training attention.
  cg_decode_logprob_rows, cg_decode_emit step 4   decode.hip row_logprob: (x_t - m) - logf(sum __expf(x_v
                                  - m)), fp32 lane-strided sums: u = 2^-24 (logprob_budget).
  attention bf16 D = 64           attention_d64_tile.h: softmax_pack packs P = exp2(s c - m) to bf16
  (resident and ring)             before the PV product and the matrix-core row sums, dq_group_tile /
                                  dkdv_tile pack dS = P (dP - delta) and P to bf16 (pack16), outputs
                                  are bf16 (store_rows_wide): u = 2^-9 for o, lse, dq, dk, dv.
  attention generic bf16          attention_generic.hip: fp32 inside, bf16 stores: u = 2^-9.
  attention fp32                  attention_f32.hip / attention_generic.hip: u = 2^-24 with the
                                  conditioning of P in S (expf(s scale - lse) in fp32).
  cg_ce_fwd / cg_ce_bwd           ce.hip k_ce_fwd / k_ce_bwd: expf / logf in fp32, u = 2^-24.
  cg_head_fwd                     head.hip: logits fp32 MFMA accumulation (u = 2^-24); lse and the
                                  loss from those logits with __expf / __logf (u = 2^-24).
  cg_head_bwd[_ex]                head.hip k_head_bwd: dl is stored bf16 (pack_bf2): u = 2^-9; db
                                  sums the fp32 values before rounding: u = 2^-24.
  cg_embed_bwd, cg_colsum, cg_reduce_rows, cg_sum_f32   fp32 sums in a fixed order (embed.hip,
                                  reduce.hip, util.hip): u = 2^-24, rigorous cap terms + 2.

PLAIN IMPLEMENTATIONS.  Each operation in plain torch on the CPU at the kernel's working precision
(fp32 arithmetic on the same, already rounded operands; P and dS rounded to bf16 where the kernel
rounds them; the output rounded to the kernel's output type), written from the mathematics and
oracle/gpt1_oracle.py, in torch's own summation order.  Where a second valid order is cheap (K
chunks of 32 for a GEMM, an explicit two-pass LayerNorm, a sequential sum) both are run and
rho_plain is the larger: the bar of the GPU tests, rho_kernel <= 8 rho_plain, then rests on the
spread between valid orders and not on one of them.

Not a conftest and no fixtures: plain helpers, as tests/footprint.py.
"""
import collections
import math

import numpy as np
import torch

U32 = 2.0 ** -24
UBF = 2.0 ** -9
MARGIN = 8.0
TINY = 2.0 ** -126
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EPS = 1e-5


def u_of(dtype):
    return UBF if dtype == BF16 else U32


def rnd(t, dtype):
    """t rounded (RNE) to dtype, returned as float32 values."""
    return t.to(F32).to(dtype).to(F32)


# ---- rho ---------------------------------------------------------------------------------------------------
class Rho(collections.namedtuple("Rho", "value index got ref S")):
    def __str__(self):
        return (f"rho {self.value:.4g} at {self.index}: got {self.got!r}, ref {self.ref!r}, S {self.S!r}")


def rho(got, ref, S, u):
    """max |got - ref| / (u S + 2^-126) over the elements, with the worst element's index, got, ref and S.
    2^-126, the smallest normal number of fp32 and of bf16, is the one absolute term of the arithmetic:
    a result below it is flushed or loses bits whatever the algorithm (a softmax weight of 1e-60 is 0 in
    fp32).  An element with got == ref counts 0 whatever S; a non-finite got counts inf."""
    g = got.detach().to("cpu", F64).reshape(ref.shape)
    r, s = ref.to(F64), S.to(F64).expand_as(ref)
    err = (g - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (u * s + TINY))
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, math.inf))
    ratio = torch.nan_to_num(ratio, nan=math.inf, posinf=math.inf)
    flat = int(ratio.reshape(-1).argmax()) if ratio.numel() else 0
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(ratio.shape))) if ratio.dim() else ()
    return Rho(float(ratio.reshape(-1)[flat]), idx, float(g.reshape(-1)[flat]), float(r.reshape(-1)[flat]),
               float(s.reshape(-1)[flat]))


def relerr(a, b):
    """The parity tests' max-norm metric."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---- exact power-of-two scaling ----------------------------------------------------------------------------
def scaled_equal(base, scaled, k):
    """Whether `scaled` == `base` * 2^k bit for bit (compared as values: +-0 alike, finite)."""
    b = base.detach().to("cpu", F64) * 2.0 ** k
    s = scaled.detach().to("cpu", F64)
    return bool(torch.isfinite(s).all()) and torch.equal(b, s)


def scaling_mismatch(base, scaled, k):
    """'' when scaled_equal, else a description of the first differing element."""
    if scaled_equal(base, scaled, k):
        return ""
    b = (base.detach().to("cpu", F64) * 2.0 ** k).reshape(-1)
    s = scaled.detach().to("cpu", F64).reshape(-1)
    bad = ((b != s) | ~torch.isfinite(s)).nonzero().flatten()
    i = int(bad[0])
    return f"{bad.numel()} of {b.numel()} elements differ; first at flat {i}: base*2^{k} {float(b[i])!r}, got {float(s[i])!r}"


# ---- GEMM ------------------------------------------------------------------------------------------------------
def gemm_operands(g, M, N, K, profile, dtype=BF16):
    """A [M, K] (the K-side operand) and W [N, K] (the weight), rounded to dtype, as float32.
    outlier: 4 random columns of A and 4 random rows of W scaled by 64."""
    A = torch.randn(M, K, generator=g) * 0.5
    W = torch.randn(N, K, generator=g) * 0.5
    info = {}
    if profile == "outlier":
        info["a_cols"] = torch.randperm(K, generator=g)[:4]
        info["w_rows"] = torch.randperm(N, generator=g)[:4]
        A[:, info["a_cols"]] *= 64
        W[info["w_rows"]] *= 64
    elif profile != "unit":
        raise ValueError(profile)
    return rnd(A, dtype), rnd(W, dtype), info


def gemm_budget(A, W, bias=None, resid=None, beta=0.0, C0=None, relu=False, keep=None, gate=None):
    """ref and S of epilogue(A W^T): |A| |W|^T + |bias| + |resid| + beta |C0|.  keep: the dropout
    multiplier keep / (1 - p) per element (applied to acc + bias); gate: the ReLU-backward mask."""
    acc, S = A.double() @ W.double().t(), A.double().abs() @ W.double().abs().t()
    if bias is not None:
        acc, S = acc + bias.double(), S + bias.double().abs()
    if relu:
        acc = torch.relu(acc)
    if keep is not None:
        acc, S = acc * keep.double(), S * keep.double()
    if resid is not None:
        acc, S = acc + resid.double(), S + resid.double().abs()
    if gate is not None:
        acc, S = acc * gate.double(), S * gate.double()
    if beta:
        acc, S = acc + beta * C0.double(), S + beta * C0.double().abs()
    return acc, S


def gemm_plain(A, W, bias=None, resid=None, beta=0.0, C0=None, relu=False, keep=None, gate=None, out_dtype=F32,
               chunk=None, slab_splits=None):
    """The same in fp32.  chunk: K in chunks of that width, summed in order (a second valid order).
    slab_splits: split-K with each split's partial sum rounded to bf16 first (CG_GEMM_SLAB_BF16)."""
    A, W = A.float(), W.float()
    K = A.shape[1]
    if slab_splits:
        per = (K + slab_splits - 1) // slab_splits
        acc = sum(rnd(A[:, k:k + per] @ W[:, k:k + per].t(), BF16) for k in range(0, K, per))
    elif chunk:
        acc = torch.zeros(A.shape[0], W.shape[0])
        for k in range(0, K, chunk):
            acc = acc + A[:, k:k + chunk] @ W[:, k:k + chunk].t()
    else:
        acc = A @ W.t()
    if bias is not None:
        acc = acc + bias.float()
    if relu:
        acc = torch.relu(acc)
    if keep is not None:
        acc = acc * keep.float()
    if resid is not None:
        acc = acc + resid.float()
    if gate is not None:
        acc = acc * gate.float()
    if beta:
        acc = acc + beta * C0.float()
    return rnd(acc, out_dtype)


def gemm_rho_plain(A, W, ref, S, out_dtype=F32, **kw):
    """The larger rho of torch's own order and K chunks of 32."""
    u = UBF if kw.get("slab_splits") else u_of(out_dtype)
    a = rho(gemm_plain(A, W, out_dtype=out_dtype, **kw), ref, S, u).value
    if kw.get("slab_splits"):
        return a
    return max(a, rho(gemm_plain(A, W, out_dtype=out_dtype, chunk=32, **kw), ref, S, u).value)


def dot_cap(K, extra=0, out_dtype=F32):
    """Rigorous cap on rho of a length-K dot product accumulated in fp32 in any order, with `extra`
    further fp32 operations in the epilogue: K + 2 + extra.  With one bf16 rounding after it (judged
    at u = 2^-9, the rounding itself is up to 2^-8 relative): |got - acc| <= 2^-8 (|ref| + cap32 2^-24 S)
    and |ref| <= S, so 2 + cap32 2^-15 (1 + 2^-8)."""
    cap32 = K + 2 + extra
    return cap32 if out_dtype == F32 else 2.0 + cap32 * 2.0 ** -15 * (1 + 2.0 ** -8)


# ---- LayerNorm ---------------------------------------------------------------------------------------------
def ln_rows(g, rows, C, profile):
    """x [rows, C] fp32.  unit: randn * 2 + 0.5 (the parity tests'); outlier: 4 channels x 64; offset:
    randn + 1024 (1 + rand) per row; flat: even rows exactly constant, odd rows c + 1e-4 randn (a
    variance of 1e-8, below eps = 1e-5)."""
    if profile == "unit":
        return torch.randn(rows, C, generator=g) * 2 + 0.5
    if profile == "outlier":
        x = torch.randn(rows, C, generator=g) * 2 + 0.5
        x[:, torch.randperm(C, generator=g)[:min(4, C)]] *= 64
        return x
    if profile == "offset":
        return torch.randn(rows, C, generator=g) + 1024 * (1 + torch.rand(rows, 1, generator=g))
    if profile == "flat":
        c = torch.randn(rows, 1, generator=g) * 2 + 0.5
        x = c + 1e-4 * torch.randn(rows, C, generator=g)
        x[0::2] = c[0::2]
        return x
    raise ValueError(profile)


def ln_params(g, C):
    return torch.randn(C, generator=g) * 0.1 + 1, torch.randn(C, generator=g) * 0.1


def ln_fwd_budget(x, w, b, eps=EPS):
    """{name: (ref, S)} for y, mean, rstd.
    y: (|x| + |mu|) rstd |w| + |b|.  mean: mean|x|.  rstd is no sum: with d = x - mu carrying the
    error u (|x| + |mu|), var + eps carries u (mean((|x| + |mu|)^2) + eps) and rstd = (var + eps)^-1/2
    half of that relatively, plus its own two roundings: S = rstd (0.5 S_var / (var + eps) + 1)."""
    x, w, b = x.double(), w.double(), b.double()
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    ax = x.abs() + mu.abs()
    y = (x - mu) * rstd * w + b
    S_var = (ax ** 2).mean(1, keepdim=True) + eps
    return {"y": (y, ax * rstd * w.abs() + b.abs()),
            "mean": (mu[:, 0], x.abs().mean(1)),
            "rstd": (rstd[:, 0], (rstd * (0.5 * S_var / (var + eps) + 1))[:, 0])}


def ln_fwd_plain(x, w, b, eps=EPS, out_dtype=F32, order="torch"):
    """fp32 LayerNorm: torch's own (order "torch") or the explicit two-pass formula."""
    x, w, b = x.float(), w.float(), b.float()
    if order == "torch":
        y, mu, rstd = torch.native_layer_norm(x, [x.shape[1]], w, b, eps)
        return rnd(y, out_dtype), mu.reshape(-1), rstd.reshape(-1)
    mu = x.mean(1, keepdim=True)
    d = x - mu
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    return rnd(d * rstd * w + b, out_dtype), mu[:, 0], rstd[:, 0]


def ln_fwd_rho_plain(x, w, b, budget, out_dtype=F32, eps=EPS):
    out = {}
    for order in ("torch", "twopass"):
        y, mu, rstd = ln_fwd_plain(x, w, b, eps, out_dtype, order)
        for name, got, u in (("y", y, u_of(out_dtype)), ("mean", mu, U32), ("rstd", rstd, U32)):
            out[name] = max(out.get(name, 0.0), rho(got, *budget[name], u).value)
    return out


def ln_bwd_budget(dy, x, w, mean, rstd, dres=None):
    """{name: (ref, S)} for dx, dw, db of the LayerNorm backward GIVEN mean and rstd (the forward's fp32
    values, inputs of the kernel): xh = (x - mu) rs, g = dy w, dx = rs (g - mean g - xh mean(g xh))
    [+ dres], dw = sum_r dy xh, db = sum_r dy; S: |x| + |mu| for x - mu, sums for differences."""
    dy, x, w = dy.double(), x.double(), w.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh, xa = (x - mu) * rs, (x.abs() + mu.abs()) * rs
    gg, ga = dy * w, dy.abs() * w.abs()
    dx = rs * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    S = rs * (ga + ga.mean(1, keepdim=True) + xa * (ga * xa).mean(1, keepdim=True))
    if dres is not None:
        dx, S = dx + dres.double(), S + dres.double().abs()
    return {"dx": (dx, S), "dw": ((dy * xh).sum(0), (dy.abs() * xa).sum(0)), "db": (dy.sum(0), dy.abs().sum(0))}


def ln_bwd_plain(dy, x, w, mean, rstd, dres=None, order="torch"):
    dy, x, w, mean, rstd = (t.float() for t in (dy, x, w, mean, rstd))
    C = x.shape[1]
    if order == "torch":
        dx, dw, db = torch.ops.aten.native_layer_norm_backward(dy, x, [C], mean[:, None], rstd[:, None], w,
                                                               torch.zeros(C), [True, True, True])
    else:
        xh = (x - mean[:, None]) * rstd[:, None]
        gg = dy * w
        dx = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
        dw, db = (dy * xh).sum(0), dy.sum(0)
    if dres is not None:
        dx = dx + dres.float()
    return {"dx": dx, "dw": dw, "db": db}


def ln_bwd_rho_plain(dy, x, w, mean, rstd, budget, dres=None):
    out = {}
    for order in ("torch", "formula"):
        got = ln_bwd_plain(dy, x, w, mean, rstd, dres, order)
        for name in ("dx", "dw", "db"):
            out[name] = max(out.get(name, 0.0), rho(got[name], *budget[name], U32).value)
    return out


# ---- sums --------------------------------------------------------------------------------------------------
def sum_budget(x, dim=0):
    return x.double().sum(dim), x.double().abs().sum(dim)


def sum_rho_plain(x, ref, S, dim=0):
    """The largest rho of four valid fp32 orders: torch's own, one element after the other from the
    front and from the back (cumsum), and four interleaved partial sums added at the end (the order
    of a 4-lane vector loop)."""
    x = x.float().movedim(dim, 0)
    n = x.shape[0]
    lanes = torch.stack([x[i::4].cumsum(0)[-1] if i < n else torch.zeros_like(x[0]) for i in range(4)])
    orders = (x.sum(0), x.cumsum(0)[-1], x.flip(0).cumsum(0)[-1], (lanes[0] + lanes[1]) + (lanes[2] + lanes[3]))
    return max(rho(o, ref, S, U32).value for o in orders)


# ---- attention ---------------------------------------------------------------------------------------------
def attn_operands(g, B, T, H, D, profile):
    """(q, k, v) fp64 [B, T, H, D], NOT yet rounded (round with rnd(., dtype)), and the softmax scale.
    unit     randn * 0.7, scale (3 D)^-0.5: scores of standard deviation ~0.3, a near-uniform softmax
    peaked   q_t = 0.3 n_t + 8 k_j(t) / sqrt(D), j(t) = 0, t, t // 2 or a random key <= t by t mod 4;
             n, k, v randn; scale D^-0.5
    sink     q_t = 0.3 n_t + 8 k_0 / sqrt(D): every query attends key 0
    shifted  unit with one vector c added to every key: every score of row t moves by scale q_t . c (of
             order 50-100), the softmax is unchanged
    spiked   test_attention_forward_rescale_branch's operands at this T (queries share a direction that
             one key at 300 / 512 of the sequence matches strongly; key norms grow along the sequence)"""
    d = H * D
    if profile in ("unit", "shifted"):
        q, k, v = (torch.randn(B, T, H, D, generator=g).double() * 0.7 for _ in range(3))
        if profile == "shifted":
            k = k + 180.0 * torch.randn(1, 1, H, D, generator=g).double()
        return q, k, v, (3.0 * D) ** -0.5
    if profile in ("peaked", "sink"):
        n, k, v = (torch.randn(B, T, H, D, generator=g).double() for _ in range(3))
        t = torch.arange(T)
        j = torch.zeros(T, dtype=torch.int64)
        if profile == "peaked":
            rand_j = (torch.rand(T, generator=g) * (t + 1)).long().clamp(max=T - 1)
            j = torch.where(t % 4 == 1, t, torch.where(t % 4 == 2, t // 2, torch.where(t % 4 == 3, rand_j, j)))
        return 0.3 * n + 8.0 * k[:, j] / math.sqrt(D), k, v, D ** -0.5
    if profile == "spiked":
        g.manual_seed(31)
        qkv = torch.randn(B * T, 3 * d, generator=g) * 0.5
        qkv[:, :d] += 2.0
        qkv[300 * T // 512, d:2 * d] = 8.0
        qkv[:, d:2 * d][:, :D] *= torch.linspace(0.1, 3.0, T).repeat(B)[:, None]
        return tuple(qkv[:, i * d:(i + 1) * d].double().view(B, T, H, D) for i in range(3)) + (D ** -0.5,)
    raise ValueError(profile)


def _causal(T):
    return torch.tril(torch.ones(T, T, dtype=torch.bool))


def attn_scores(q, k, scale):
    """fp64 masked scores [B, H, T, T], their logsumexp and the softmax."""
    s = torch.einsum("bthd,bshd->bhts", q.double(), k.double()) * scale
    s = s.masked_fill(~_causal(q.shape[1]), -math.inf)
    lse = torch.logsumexp(s, -1)
    return s, lse, torch.exp(s - lse[..., None])


def attn_budget(q, k, v, dO, scale, keep=None, fp32_cond=False):
    """{name: (ref, S)} for o, lse, dq, dk, dv ([B, T, H, D]; lse [B, H, T]).  keep: the dropout
    multiplier keep / (1 - p) [B, H, T, T] or None.  fp32_cond: P carries (1 + |s| + |lse|) in S."""
    q, k, v, dO = (t.double() for t in (q, k, v, dO))
    s, lse, P = attn_scores(q, k, scale)
    kd = torch.ones_like(P) if keep is None else keep.double()
    Pd = P * kd
    s0 = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s))
    cond = 1 + s0 + lse.abs()[..., None] if fp32_cond else torch.ones_like(P)
    o = torch.einsum("bhts,bshd->bthd", Pd, v)
    out = {"o": (o, torch.einsum("bhts,bshd->bthd", Pd * cond, v.abs()))}
    # lse = log sum exp(s): the score errors weighted by P, its own magnitude and the log's rounding
    S_s = torch.einsum("bthd,bshd->bhts", q.abs(), k.abs()) * scale
    out["lse"] = (lse, (P * S_s).sum(-1) + lse.abs() + 1)
    dP = torch.einsum("bthd,bshd->bhts", dO, v)
    delta = (dO * o).sum(-1).permute(0, 2, 1)[..., None]               # [B, H, T, 1]
    dS = P * (kd * dP - delta)
    aP = torch.einsum("bthd,bshd->bhts", dO.abs(), v.abs())
    adelta = (dO.abs() * o.abs()).sum(-1).permute(0, 2, 1)[..., None]
    aS = P * cond * (kd * aP + adelta)
    out["dq"] = (scale * torch.einsum("bhts,bshd->bthd", dS, k), scale * torch.einsum("bhts,bshd->bthd", aS, k.abs()))
    out["dk"] = (scale * torch.einsum("bhts,bthd->bshd", dS, q), scale * torch.einsum("bhts,bthd->bshd", aS, q.abs()))
    out["dv"] = (torch.einsum("bhts,bthd->bshd", Pd, dO), torch.einsum("bhts,bthd->bshd", Pd * cond, dO.abs()))
    return out


def attn_plain(q, k, v, dO, scale, keep=None, dtype=BF16, round_p=False):
    """fp32 attention forward and backward on the (rounded) operands.  round_p: the unnormalised
    weights, and in the backward P and dS, are rounded to bf16 before the products they feed, and the
    row sums are taken over the rounded weights (the D = 64 kernels).  Those kernels are online
    softmaxes with a lazy rescale (attention_d64_tile.h rescale_if, RESCALE_THR = 8 in log2 units):
    the weights are taken relative to a running maximum that may lag the row maximum by up to 2^8, so
    a row's largest weight is not exactly 1 and is rounded to bf16 like every other.  The plain form
    has the same rounding by the same rule over its own blocking, two halves of the keys: the
    reference point is the first half's maximum unless the row maximum exceeds it by more than 2^8.
    Outputs rounded to dtype; the backward reads the rounded o and the fp32 lse, as the kernels do."""
    q, k, v, dO = (t.float() for t in (q, k, v, dO))
    T = q.shape[1]
    s = (torch.einsum("bthd,bshd->bhts", q, k) * scale).masked_fill(~_causal(T), -math.inf)
    m = s.max(-1, keepdim=True).values
    if round_p:
        m1 = s[..., :max(T // 2, 1)].max(-1, keepdim=True).values       # key 0 is visible to every query
        m = torch.where(m > m1 + 8 * math.log(2.0), m, m1)
    p = torch.exp(s - m)
    if round_p:
        p = rnd(p, BF16)
    l = p.sum(-1, keepdim=True)
    kd = torch.ones_like(p) if keep is None else keep.float()
    o = rnd(torch.einsum("bhts,bshd->bthd", p * kd, v) / l[..., 0].permute(0, 2, 1)[..., None], dtype)
    lse = (m + torch.log(l))[..., 0]
    P = torch.exp(s - lse[..., None])
    dP = torch.einsum("bthd,bshd->bhts", dO, v)
    delta = (dO * o).sum(-1).permute(0, 2, 1)[..., None]
    dS = P * (kd * dP - delta)
    Pd = P * kd
    if round_p:
        dS, Pd = rnd(dS, BF16), rnd(Pd, BF16)
    return {"o": o, "lse": lse,
            "dq": rnd(scale * torch.einsum("bhts,bshd->bthd", dS, k), dtype),
            "dk": rnd(scale * torch.einsum("bhts,bthd->bshd", dS, q), dtype),
            "dv": rnd(torch.einsum("bhts,bthd->bshd", Pd, dO), dtype)}


def decode_attn_plain(q, k, v, scale, chunk=64):
    """The decode path's attention in plain fp32 torch: row t is the query at position t against keys
    0..t, as an online softmax over chunks of `chunk` keys in the statistics order of decode.hip's
    attn_chunk -- per chunk m_new = max(m, chunk max), alpha = exp(m - m_new), p = exp(s - m_new),
    l = l alpha + sum p, acc = acc alpha + p v, and o = acc (1 / l) at the end.  Written from the
    mathematics (the dot products and chunk sums in torch's own order); q, k, v [B, T, H, D] already
    rounded to fp32.  Returns o [B, T, H, D]."""
    q, k, v = (t.float() for t in (q, k, v))
    B, T, H, D = q.shape
    s = (torch.einsum("bthd,bshd->bhts", q, k) * np.float32(scale)).masked_fill(~_causal(T), -math.inf)
    m = torch.full((B, H, T, 1), -math.inf)
    l = torch.zeros(B, H, T, 1)
    acc = torch.zeros(B, H, T, D)
    for c0 in range(0, T, chunk):
        sc = s[..., c0:c0 + chunk]
        m_new = torch.maximum(m, sc.max(-1, keepdim=True).values)
        alpha = torch.exp(m - m_new)
        p = torch.exp(sc - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + torch.einsum("bhts,bshd->bhtd", p, v[:, c0:c0 + chunk])
        m = m_new
    return (acc * (1.0 / l)).permute(0, 2, 1, 3).contiguous()


def decode_attn_rho_plain(q, k, v, scale, ref, S):
    """rho of the two plain orders (torch's whole-row softmax, the chunk-64 online softmax) per row t:
    [T] tensors of the larger, so that a run with n keys is judged against row n - 1's own figure and
    the whole o against the maximum."""
    z = torch.zeros_like(q)
    out = None
    for got in (attn_plain(q, k, v, z, scale, dtype=F32)["o"], decode_attn_plain(q, k, v, scale)):
        r = torch.tensor([rho(got[:, t], ref[:, t], S[:, t], U32).value for t in range(q.shape[1])], dtype=F64)
        out = r if out is None else torch.maximum(out, r)
    return out


# ---- cross entropy and the head --------------------------------------------------------------------------
def ce_logits(g, rows, V, profile):
    """logits [rows, V] fp32 and targets.  unit: randn * 3.  Rows r % 4 == 3 stay unit in every profile.
    confident: the target logit is 30 above the largest other one; wrong: 30 below the smallest;
    offset: every logit + 1e3; certain: confident with a margin of 100 (exp(-100) is below fp32's normal
    range: every other weight underflows against the right maximum, and exp(+100) overflows against a wrong one)."""
    x = torch.randn(rows, V, generator=g) * 3
    tgt = torch.randint(0, V, (rows,), generator=g)
    hit = torch.arange(rows) % 4 != 3
    if profile in ("confident", "wrong", "certain"):
        others = x.clone()
        others[torch.arange(rows), tgt] = math.inf if profile == "wrong" else -math.inf
        new = others.min(1).values - 30 if profile == "wrong" else others.max(1).values + (30 if profile == "confident" else 100)
        x[hit, tgt[hit]] = new[hit]
    elif profile == "offset":
        x[hit] += 1e3
    elif profile != "unit":
        raise ValueError(profile)
    return x, tgt


def ce_budget(x, tgt, g=1.0, lse_in=None):
    """{name: (ref, S)}: lse (S = |lse| + max|x| + 1), loss = lse - x_t (S = |lse| + |x_t| + max|x|),
    dlogits = g (exp(x - lse) - onehot) (S = |g| (p (1 + max|x| + |lse|) + onehot)).  lse_in: the lse
    the backward is GIVEN (its input); the forward's own otherwise."""
    x = x.double()
    rows = x.shape[0]
    lse = torch.logsumexp(x, 1)
    xm = x.abs().max(1).values
    xt = x[torch.arange(rows), tgt]
    onehot = torch.zeros_like(x)
    onehot[torch.arange(rows), tgt] = 1
    lb = lse if lse_in is None else lse_in.double()
    p = torch.exp(x - lb[:, None])
    return {"lse": (lse, lse.abs() + xm + 1),
            "loss": (lse - xt, lse.abs() + xt.abs() + xm),
            "dlogits": (g * (p - onehot), abs(g) * (p * (1 + xm + lb.abs())[:, None] + onehot))}


def ce_plain(x, tgt, g=1.0, lse_in=None):
    x = x.float()
    rows = x.shape[0]
    lse = torch.logsumexp(x, 1)
    onehot = torch.zeros_like(x)
    onehot[torch.arange(rows), tgt] = 1
    lb = lse if lse_in is None else lse_in.float()
    return {"lse": lse, "loss": lse - x[torch.arange(rows), tgt],
            "dlogits": np.float32(g) * (torch.exp(x - lb[:, None]) - onehot)}


def logprob_budget(x, tgt):
    """(ref, S) of the decode path's log-probability of token tgt_r in row r, from the header's formula
    (x_t - m) - log sum_v exp(x_v - m), m = max x: ref = x_t - lse; S = |x_t - m| + |lse - m| + 1.  The
    two differences are the terms that are added (x_v - m of fp32 numbers within a factor 2 of each
    other is exact, of others it carries u |x_v - m|, which the sum's weights exp(x_v - m) <= 1 damp
    below u |lse - m| + u); the 1 is the sum's and the log's own rounding, relative errors of the sum
    being absolute ones of its log.  Shift-invariant, as the contract is: adding a constant to a row
    changes neither ref nor S, so on `offset` this is tighter than ce_budget's max|x| term."""
    x = x.double()
    r = torch.arange(x.shape[0])
    m = x.max(1).values
    lse = torch.logsumexp(x, 1)
    xt = x[r, tgt]
    return xt - lse, (xt - m).abs() + (lse - m).abs() + 1


def logprob_plain(x, tgt, order="torch"):
    """fp32: torch.log_softmax's own order, or ("formula") the header's formula term by term."""
    x = x.float()
    r = torch.arange(x.shape[0])
    if order == "torch":
        return torch.log_softmax(x, 1)[r, tgt]
    m = x.max(1).values
    return (x[r, tgt] - m) - torch.log(torch.exp(x - m[:, None]).sum(1))


def logprob_rho_plain(x, tgt, ref, S):
    return max(rho(logprob_plain(x, tgt, o), ref, S, U32).value for o in ("torch", "formula"))


# ---- the fp32 inference rows (rows_f32.hip) ---------------------------------------------------------------
def linear_ln_budget(a, lw, lb, W, bias=None, resid=None, relu=False, eps=EPS):
    """(ref, S) of out = [resid +] act(a' W^T [+ bias]) with a' = LayerNorm(a; lw, lb) (lw given) or a' = a.
    Every a'_k carries the error u S_LN,k of ln_fwd_budget's y (0 without the LayerNorm, where a' is an
    operand) and |a'_k| <= S_LN,k, so the product's own roundings and the propagated ones are both
    inside S = S_a' |W|^T + |bias| + |resid|, S_a' = S_LN or |a|.  ReLU is 1-Lipschitz: |relu(got) -
    relu(ref)| <= |got - ref|, the same S serves and no decision rule is needed in a forward."""
    if lw is not None:
        y, Sy = ln_fwd_budget(a, lw, lb, eps)["y"]
    else:
        y, Sy = a.double(), a.double().abs()
    ref, S = y @ W.double().t(), Sy @ W.double().abs().t()
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if relu:
        ref = torch.relu(ref)
    if resid is not None:
        ref, S = ref + resid.double(), S + resid.double().abs()
    return ref, S


def linear_ln_rho_plain(a, lw, lb, W, ref, S, bias=None, resid=None, relu=False, eps=EPS):
    """The larger rho of the fp32 product on both ln_fwd_plain orders (on a itself and in K chunks of 32
    without the LayerNorm)."""
    def tail(acc):
        acc = acc if bias is None else acc + bias.float()
        acc = torch.relu(acc) if relu else acc
        return acc if resid is None else acc + resid.float()
    if lw is None:
        return gemm_rho_plain(a, W, ref, S, bias=bias, resid=resid, relu=relu)
    return max(rho(tail(ln_fwd_plain(a, lw, lb, eps, order=o)[0] @ W.float().t()), ref, S, U32).value
               for o in ("torch", "twopass"))


def ffn_budget(a, lw, lb, W1, b1, W2, b2, resid, eps=EPS):
    """(ref, S) of out = resid + relu(a' W1^T + b1) W2^T + b2, a' as in linear_ln_budget.
    The hidden pre-activation z = a' W1^T + b1 carries u S_h, S_h = S_a' |W1|^T + |b1| (linear_ln_budget);
    h = relu(z) carries no more (1-Lipschitz).  The second product sums the terms h_j W2_cj, each with
    its own rounding u |h_ref,j| |W2_cj| and the propagated u S_h,j |W2_cj|, then b2 and resid:
    S_out = |resid| + |b2| + (|h_ref| + S_h) |W2|^T."""
    z, S_h = linear_ln_budget(a, lw, lb, W1, b1, eps=eps)
    h = torch.relu(z)
    ref = resid.double() + h @ W2.double().t() + b2.double()
    S = resid.double().abs() + b2.double().abs() + (h.abs() + S_h) @ W2.double().abs().t()
    return ref, S


def ffn_rho_plain(a, lw, lb, W1, b1, W2, b2, resid, ref, S, eps=EPS):
    out = 0.0
    for o in ("torch", "twopass"):
        y = ln_fwd_plain(a, lw, lb, eps, order=o)[0] if lw is not None else a.float()
        got = resid.float() + (torch.relu(y @ W1.float().t() + b1.float()) @ W2.float().t() + b2.float())
        out = max(out, rho(got, ref, S, U32).value)
        if lw is None:
            break
    return out


def head_operands(g, M, C, V, profile):
    """a [M, C], W [V, C] (bf16 values as fp32), bias [V], targets.  Column 0 of `a` is 1 (a constant
    feature), so one weight row carries the margin: confident / wrong put +-40 into W[t0, 0] and make
    t0 the target of the rows r % 4 != 3 (class t0's logit is then >= 30 above / below the others
    there); offset adds 1e3 to the whole bias."""
    a = torch.randn(M, C, generator=g)
    a[:, 0] = 1.0
    W = torch.randn(V, C, generator=g) / C ** 0.5
    bias = torch.randn(V, generator=g)
    tgt = torch.randint(0, V, (M,), generator=g)
    t0 = V // 3
    if profile in ("confident", "wrong"):
        W[t0, 0] = 40.0 if profile == "confident" else -40.0
        tgt[torch.arange(M) % 4 != 3] = t0
    elif profile == "offset":
        bias = bias + 1e3
    elif profile != "unit":
        raise ValueError(profile)
    return rnd(a, BF16), rnd(W, BF16), bias, tgt


# ---- embeddings ----------------------------------------------------------------------------------------------
def embed_operands(g, V, T, C, B):
    """idx [B, T] with one token in 90 % of the positions, dx [B T, C] with 4 channels x 64."""
    idx = torch.randint(0, V, (B, T), generator=g)
    hot = int(torch.randint(0, V, (1,), generator=g))
    idx[torch.rand(B, T, generator=g) < 0.9] = hot
    dx = torch.randn(B * T, C, generator=g)
    dx[:, torch.randperm(C, generator=g)[:4]] *= 64
    return idx, dx, hot


def embed_budget(idx, dx, V):
    B, T = idx.shape
    d = dx.double()
    z = torch.zeros(V, d.shape[1], dtype=F64)
    flat = idx.reshape(-1)
    return {"dwte": (z.clone().index_add_(0, flat, d), z.clone().index_add_(0, flat, d.abs())),
            "dwpe": (d.view(B, T, -1).sum(0), d.abs().view(B, T, -1).sum(0))}


def embed_plain(idx, dx, V):
    B, T = idx.shape
    d = dx.float()
    return {"dwte": torch.zeros(V, d.shape[1]).index_add_(0, idx.reshape(-1), d), "dwpe": d.view(B, T, -1).sum(0)}


# ---- AdamW: csrc/adamw.h adam_one / adam_scalars restated rounding by rounding in numpy -------------------
def fma32(a, b, c, every=False):
    """Exactly rounded float32 fma(a, b, c) on numpy arrays (float64 sum, fixed up with exact
    rationals where rounding that sum to float32 could differ from rounding the exact value).

    The product of two float32 is exact in float64, so r = fl64(a b + c) is the one inexact step, and
    rounding to float64 is monotonic: the exact value and r lie on the same side of every float32
    midpoint (all of them are float64 numbers) unless r IS such a midpoint.  Only there, and only if
    the float64 sum was inexact (its TwoSum error is not 0), can float32(r) be the wrong neighbour --
    a handful of elements in 10^9, so whole flat parameter buffers are affordable (tests/trajectory.py).
    every=True fixes up every element whose r is not a float32, the slow original selection
    (test_cpu_trajectory.py holds the two equal)."""
    from fractions import Fraction
    f = np.float32
    a, b, c = (np.broadcast_to(np.asarray(x, f), np.shape(c)).astype(f) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
        r = p + c64
        out = r.astype(f)
        sel = np.isfinite(r) & np.isfinite(out) & (r != out.astype(np.float64))
        if not every:
            bb = r - p
            err = (p - (r - bb)) + (c64 - bb)          # TwoSum: p + c64 == r + err exactly
            toward = np.where(r > out.astype(np.float64), f(np.inf), f(-np.inf)).astype(f)
            other = np.nextafter(out, toward).astype(np.float64)
            tie = np.abs(r - out.astype(np.float64)) == np.abs(other - r)
            sel &= tie & ~(err == 0)                   # (a NaN err keeps the element: fixed up exactly)
    for i in np.nonzero(sel)[0]:
        ex = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = f(float(ex))
        cands = [np.nextafter(lo, f(-np.inf)), lo, np.nextafter(lo, f(np.inf))]
        cands = [x for x in cands if np.isfinite(x)]
        out[i] = min(cands, key=lambda x: (abs(Fraction(float(x)) - ex), int(f(x).view(np.uint32)) & 1))
    return out


def adamw_numpy(P, G, M, V, lr, b1, b2, eps, wd, t, gscale=None):
    """One AdamW step as csrc/adamw.h rounds it (the sequence of test_adamw_rounding_is_explicit);
    gscale: the gradient times that fp32 coefficient, rounded once, first (cg_adamw_dyn)."""
    f = np.float32
    with np.errstate(all="ignore"):
        if gscale is not None:
            G = (G * f(gscale)).astype(f)
        decay, w1, B2, omb2, E = f(1 - lr * wd), f(1 - b1), f(b2), f(1 - b2), f(eps)
        neg, bc2s = f(-(lr / (1 - b1 ** t))), f(math.sqrt(1 - b2 ** t))
        P = (P * decay).astype(f)
        M = fma32(w1, (G - M).astype(f), M)
        V = fma32((omb2 * G).astype(f), G, (V * B2).astype(f))
        den = ((np.sqrt(V).astype(f) / bc2s).astype(f) + E).astype(f)
        P = (P + ((neg * M).astype(f) / den).astype(f)).astype(f)
    return P, M, V


def adamw_edge_state(n=4096 + 3, seed=5):
    """p, g, m, v (float32 numpy, n elements) mixing, in repeating groups of 16: g = m = v = 0;
    |g| = 1e-30, 1e-20, 1e-10, 1, 1e10, 1e20 of both signs with small m, v (v + (1 - b2) g^2 is
    subnormal at 1e-20, underflows at 1e-30, is 1e37 at 1e20); v = 1e30 with g = 1e-30; subnormal m
    and v; v = 3.3e38 with g = 2e20 (the new v overflows to inf); ordinary elements in between.  Nothing is a NaN or an infinity."""
    rng = np.random.default_rng(seed)
    f = np.float32
    p = rng.standard_normal(n).astype(f)
    g = rng.standard_normal(n).astype(f)
    m = (rng.standard_normal(n) * 0.01).astype(f)
    v = (rng.random(n) * 1e-3).astype(f)
    i = np.arange(n) % 16
    zero = i == 0
    g[zero] = m[zero] = v[zero] = 0
    for slot, mag in enumerate((1e-30, 1e-20, 1e-10, 1.0, 1e10, 1e20)):
        for sgn, s in ((1, 1 + 2 * slot), (-1, 2 + 2 * slot)):
            sel = i == s
            g[sel] = f(sgn * mag) * (1 + rng.random(sel.sum()).astype(f))
            m[sel] = (g[sel] * f(0.1)).astype(f)
            v[sel] = 0 if slot < 3 else v[sel]
    big = i == 13
    v[big], g[big], m[big] = f(1e30), f(1e-30), f(1e-30)
    tiny = i == 14
    v[tiny], m[tiny] = f(1e-44), f(1e-42)       # subnormal moments, ordinary gradient
    top = i == 15
    v[top], g[top], m[top] = f(3.3e38), f(2e20), f(1e19)     # v b2 + (1 - b2) g^2 overflows to inf
    assert np.isfinite(p).all() and np.isfinite(g).all() and np.isfinite(m).all() and np.isfinite(v).all()
    return p, g, m, v


def bf16_bits_of(p):
    """The bf16 (RNE) bits of a float32 numpy array, as int16 (NaN kept NaN)."""
    return torch.from_numpy(np.ascontiguousarray(p)).to(BF16).view(torch.int16).numpy()
