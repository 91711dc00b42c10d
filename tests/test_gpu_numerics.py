"""The training and the inference kernels on ill-scaled data, judged element by element (tests/numerics.py),
on the MI355X.

BUDGET TESTS.  Every case runs a kernel on a data profile, computes rho_kernel = max |got - ref| / (u S)
against the fp64 reference and the element-wise budget S, and asserts rho_kernel <= 8 rho_plain, with
rho_plain the same figure of the plain torch implementation at the kernel's working precision; where
a rigorous cap exists (a length-K fp32 dot product: K + 2) it is asserted too.  On lse the bf16
kernels' own bound, 2^-8 absolute, stays a hard cap on every profile.

EXACT SCALING.  Multiplying an operand by a power of two commutes with every rounding, so a kernel
that is linear in an operand must scale bit for bit: each is called on the unit operands and again
with the operand times 2^-24 and 2^+24.

ADAMW AT THE EDGES.  cg_adamw / _segments / _dyn against the numpy restatement of csrc/adamw.h on
zero, subnormal, tiny, huge and overflowing moments, bit for bit.

THE INFERENCE KERNELS (decode.hip, rows_f32.hip) have the same three kinds of case at u = 2^-24: the decode
attention's online softmax over 64-key chunks in every dispatch form and the one-pass prefill, with the
stale cache rows NaN in one run and zero in another; the log-probabilities of cg_decode_logprob_rows and
cg_decode_emit (no operand to scale: the two must agree bit for bit instead); the fp32 Linear / QKV / FFN
rows with and without their LayerNorm.

Every case appends a line to RECORDS; the last tests check that every kernel family saw a non-unit
profile and a scaling case, and write the table to the file CHARPT_NUMERICS_REPORT names (the
committed record: profiles/numerics_gpu_tests.txt).  Calls go through the C ABI, as
test_gpu_footprint.py does, or through ops where that reaches the same kernel.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import numerics as nm
from numerics import BF16, F32, F64, MARGIN, U32, UBF, rho
from oracle import philox

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64, I32 = torch.int64, torch.int32
NAN = float("nan")

FAMILIES = ["GEMM bf16", "GEMM fp32", "grouped wgrad", "GEMM + LayerNorm", "LayerNorm forward", "LayerNorm backward",
            "attention D = 64 resident", "attention ring", "attention generic", "attention fp32", "cross entropy",
            "head", "embedding", "reductions", "decode attention", "inference rows", "log-probabilities"]
# Families with no operand they are linear in: their exact check is a bit equality (Checks.same) instead.
# Keep this to the log-probabilities (log softmax is linear in nothing): a family whose kernels are linear
# in an operand belongs to the scaling rule, and an entry here exempts it from that rule.
NONLINEAR = {"log-probabilities"}
RECORDS = []     # budget lines: (family, kernel, shape, profile, output, rho_plain, rho_kernel, cap)
SCALINGS = []    # (family, kernel, what, k, "bitwise")
SEEN = {f: {"profiles": set(), "scaling": 0, "same": 0} for f in FAMILIES}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    L().load()
    yield


def L():
    from replicatinggpt_amd import _lib
    return _lib


def lib():
    return L().load()


def ops():
    from replicatinggpt_amd import ops as o
    return o


def gen(seed):
    return torch.Generator().manual_seed(seed)


def D(t, dt=None):
    """A CPU tensor on the device, contiguous, in dtype dt."""
    return None if t is None else t.to(dtype=dt or t.dtype).contiguous().to(DEV)


def P(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def stream():
    return L().stream_ptr()


def code(dt):
    return L().dtype_code(dt)


def sync(what):
    """Wait for the device; a HIP error ends the whole session (nothing more runs on a faulted device)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error after {what}: {e}", returncode=3)


def ok(rc, what):
    assert rc == 0, f"{what}: code {rc}: {lib().cg_last_error_string().decode(errors='replace')}"
    sync(what)


def tuning(key, value):
    return lib().cg_set_tuning(key.encode(), value)


def dev_i64(v):
    return torch.tensor([v], dtype=I64, device=DEV)


def keep_mult(seed, call, site, shape, p):
    """keep / (1 - p) as the kernels apply it (fp32(1 / (1 - p))), fp64 tensor of `shape`."""
    n = int(np.prod(shape))
    keep = torch.from_numpy(philox.keep_mask(seed, (call << 8) | site, np.arange(n, dtype=np.uint64), p))
    return keep.reshape(shape).double() * float(np.float32(1 / (1 - p)))


class Checks:
    """Collects the failures of one test, so that a failing run still records every figure."""

    def __init__(self, family):
        self.family, self.bad = family, []

    def budget(self, kernel, shape, profile, output, got, ref, S, u, rho_plain, cap=None):
        r = rho(got, ref, S, u)
        RECORDS.append((self.family, kernel, str(shape), profile, output, rho_plain, r.value, cap))
        SEEN[self.family]["profiles"].add(profile)
        if not r.value <= MARGIN * rho_plain:
            self.bad.append(f"{kernel} {shape} {profile} {output}: rho_kernel {r.value:.4g} > {MARGIN:g} x rho_plain "
                            f"{rho_plain:.4g} ({r})")
        if cap is not None and not r.value <= cap:
            self.bad.append(f"{kernel} {shape} {profile} {output}: rho_kernel {r.value:.4g} above the cap {cap:.4g} ({r})")
        return r

    def scaling(self, kernel, what, base, scaled, k):
        msg = nm.scaling_mismatch(base, scaled, k)
        SCALINGS.append((self.family, kernel, what, k, "bitwise" if not msg else "DIFFERS"))
        SEEN[self.family]["scaling"] += 1
        if msg:
            self.bad.append(f"{kernel} {what} x 2^{k}: {msg}")

    def same(self, kernel, what, a, b):
        SEEN[self.family]["same"] += 1
        if not torch.equal(a.cpu(), b.cpu()):
            self.bad.append(f"{kernel} {what}: bits differ")

    def require(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


# ==== cg_gemm =============================================================================================
def pack_bits(nz):
    M, N = nz.shape
    w = (nz.view(M, N // 32, 32).long() << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(I32)


def run_gemm(dt, A, W, at=0, bt=0, kind=0, c_dt=F32, bias=None, resid=None, beta=0.0, C0=None, split=1, flags=0,
             aux=None, aux_code=0, ld_aux=0, colpart_shape=None, p=0.0, ld_resid=None, expect_rc=0):
    """cg_gemm on tight tensors.  A [M, K], W [N, K] logical CPU values (stored transposed for at / bt).
    aux: a CPU tensor (input) or a shape (output, int32 keep bits).  Returns (C, aux_out, colpart) on the
    CPU, or the return code when expect_rc is None."""
    M, K = A.shape
    N = W.shape[0]
    a, w = D(A.t() if at else A, dt), D(W.t() if bt else W, dt)
    out = D(C0, c_dt) if beta else torch.full((M, N), NAN, dtype=c_dt, device=DEV)
    bb, rr = D(bias, F32), D(resid, F32)
    aux_d = None
    if isinstance(aux, torch.Tensor):
        aux_d = D(aux)
    elif aux is not None:
        aux_d = torch.zeros(aux, dtype=I32, device=DEV)
    cp = torch.full(colpart_shape, NAN, dtype=F32, device=DEV) if colpart_shape else None
    nws = lib().cg_gemm_workspace(M, N, split)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
    call = dev_i64(6)
    epi = L().Epilogue(kind, P(bb), P(rr), ld_resid if ld_resid is not None else (N if rr is not None else 0), P(aux_d),
                       aux_code, ld_aux, p, 99, P(call), 3, beta, P(cp), flags)
    rc = lib().cg_gemm(code(dt), at, bt, M, N, K, P(a), a.shape[1], P(w), w.shape[1], P(out), code(c_dt), N, epi, split,
                       P(ws) if nws else None, stream())
    if expect_rc is None:
        sync("cg_gemm")
        return rc
    ok(rc, f"cg_gemm {M}x{N}x{K} kind {kind}")
    return out.cpu(), (aux_d.cpu() if aux_d is not None else None), (cp.cpu() if cp is not None else None)


def gemm_cases():
    """name -> (keywords of the case).  The plain store in all four layouts, the other epilogues in the
    form the header names for them (special epilogues: non-transposed A; weight gradients: TT)."""
    c = {}
    for at, bt in ((0, 0), (0, 1), (1, 0), (1, 1)):
        lay = "NT"[at] + "NT"[bt]
        c[f"store_f32 {lay}"] = dict(at=at, bt=bt)
        c[f"store_bf16 {lay}"] = dict(at=at, bt=bt, c_dt=BF16)
    c["bias_relu"] = dict(kind=2, c_dt=BF16, bias=True, bits_out=True)
    c["bias_resid"] = dict(kind=3, bias=True, resid=True)
    c["bias_drop_resid"] = dict(kind=4, bias=True, resid=True, p=0.2)
    c["relu_bwd"] = dict(kind=5, c_dt=BF16, bt=1, gate=True)
    c["store_rowdot"] = dict(kind=7, c_dt=BF16, bt=1, rowdot=True)
    c["split3_f32_slabs"] = dict(at=1, bt=1, split=3)
    c["split3_bf16_slabs"] = dict(at=1, bt=1, split=3, flags=1)
    c["beta1"] = dict(at=1, bt=1, beta=1.0)
    return c


def gemm_inputs(g, M, N, K, profile, dt):
    A, W, _ = nm.gemm_operands(g, M, N, K, profile, dt)
    x = dict(A=A, W=W, bias=torch.randn(N, generator=g), resid=torch.randn(M, N, generator=g),
             C0=torch.randn(M, N, generator=g), gate=torch.rand(M, N, generator=g) < 0.5,
             o=nm.rnd(torch.randn(M, N, generator=g), BF16))
    return x


def gemm_launch(dt, x, kw, scale_a=0, scale_w=0):
    """One case's launch; scale_a / scale_w: the operand times 2^k, and with scale_a the bias, the residual
    and C with it.  Returns dict(out=, bits=, colpart=, delta=) and the budget keywords."""
    A, W = x["A"] * 2.0 ** scale_a, x["W"] * 2.0 ** scale_w
    M, K = A.shape
    N = W.shape[0]
    f = 2.0 ** (scale_a + scale_w)
    at, bt, kind, c_dt = kw.get("at", 0), kw.get("bt", 0), kw.get("kind", 0), kw.get("c_dt", F32)
    bud = dict(bias=x["bias"] * f if kw.get("bias") else None, resid=x["resid"] * f if kw.get("resid") else None,
               beta=kw.get("beta", 0.0), C0=x["C0"] * f if kw.get("beta") else None, relu=kind == 2)
    args = dict(at=at, bt=bt, kind=kind, c_dt=c_dt, bias=bud["bias"], resid=bud["resid"], beta=bud["beta"],
                C0=bud["C0"], split=kw.get("split", 1), flags=kw.get("flags", 0), p=kw.get("p", 0.0))
    lda, ldb = (M if at else K), (N if bt else K)
    res = {}
    if kw.get("p"):
        bud["keep"] = keep_mult(99, 6, 3, (M, N), kw["p"])
    if kw.get("bits_out") and dt == BF16 and N % 64 == 0 and lib().cg_gemm_relu_bits_supported(at, bt, M, N, K, lda, ldb, N):
        args.update(aux=(M, N // 32), aux_code=L().CG_BITS, ld_aux=N // 32)
        res["has_bits"] = True
    if kw.get("gate"):
        bud["gate"] = x["gate"]
        if dt == BF16 and N % 64 == 0 and lib().cg_gemm_relu_bits_supported(at, bt, M, N, K, lda, ldb, N):
            args.update(aux=pack_bits(x["gate"]), aux_code=L().CG_BITS, ld_aux=N // 32)
        else:
            h = torch.where(x["gate"], torch.ones(M, N), -torch.ones(M, N))
            args.update(aux=h.to(c_dt), aux_code=code(c_dt), ld_aux=N)
        if dt == BF16 and M % 64 == 0 and lib().cg_gemm_colpart_supported(at, bt, M, N, K, lda, ldb, N):
            args["colpart_shape"] = (M // 64, N)
    if kw.get("rowdot"):
        if not (dt == BF16 and lib().cg_gemm_rowdot_supported(at, bt, M, N, K, lda, ldb, N)):
            return None, None
        args.update(aux=x["o"].to(BF16), aux_code=L().CG_BF16, ld_aux=N, colpart_shape=(M * (N // 64),), ld_resid=64)
    out, aux_out, cp = run_gemm(dt, A, W, **args)
    res["out"] = out
    if res.get("has_bits"):
        res["bits"] = aux_out
    if kw.get("rowdot"):
        res["delta"] = cp
    elif cp is not None:
        res["colpart"] = cp
    return res, bud


def gemm_budget_case(ck, name, variant, dt, x, kw, profile, kernel="cg_gemm"):
    res, bud = gemm_launch(dt, x, kw)
    if res is None:
        return
    A, W = x["A"], x["W"]
    M, K = A.shape
    N = W.shape[0]
    shape = f"({M}, {N}, {K}) v{variant} {name}"
    c_dt = kw.get("c_dt", F32)
    slabs = bool(kw.get("flags", 0) & 1) and variant == 9
    ref, S = nm.gemm_budget(A, W, **bud)
    pk = dict(bud, slab_splits=kw["split"]) if slabs else bud
    u = UBF if (slabs or c_dt == BF16) else U32
    extra = 1 + sum(1 for key in ("bias", "resid", "keep", "C0") if bud.get(key) is not None) + kw.get("split", 1)
    ck.budget(kernel, shape, profile, "C", res["out"], ref, S, u, nm.gemm_rho_plain(A, W, ref, S, c_dt, **pk),
              nm.dot_cap(K, extra, BF16 if u == UBF else F32))
    got = res["out"].double()
    if "bits" in res:       # the keep bits of the values written
        ck.same(kernel, f"{shape} keep bits", res["bits"], pack_bits(res["out"].float() != 0))
    if "colpart" in res:    # column sums of each 64-row block of the bf16 values written
        blocks = got.view(M // 64, 64, N)
        r_, s_ = blocks.sum(1), blocks.abs().sum(1)
        ck.budget(kernel, shape, profile, "colpart", res["colpart"], r_, s_, U32, nm.sum_rho_plain(blocks, r_, s_, 1), 64 + 2)
    if "delta" in res:      # row dots of the written values with o, per 64-column head
        T = 64
        prod = (got * x["o"].double()).view(M // T, T, N // 64, 64).permute(0, 2, 1, 3)
        r_, s_ = prod.sum(-1), prod.abs().sum(-1)
        ck.budget(kernel, shape, profile, "delta", res["delta"].view(M // T, N // 64, T), r_, s_, U32,
                  nm.sum_rho_plain(prod, r_, s_, 3), 64 + 2)


GEMM_SHAPE = {2: (256, 384, 192), 9: (256, 384, 192), 24: (256, 512, 192)}


@pytest.mark.parametrize("profile", ["unit", "outlier"])
@pytest.mark.parametrize("variant", [2, 9, 24])
def test_gemm_bf16_budget(variant, profile):
    """The bf16 MFMA kernels (register-staged 2, persistent 128x128 9, 8-wave 256x256 24) at the smallest
    shapes that reach them, every epilogue."""
    M, N, K = GEMM_SHAPE[variant]
    if tuning("gemm_variant", variant) != 0:
        pytest.skip(f"gemm_variant {variant} is A/B-only (not in this library build)")
    ck = Checks("GEMM bf16")
    try:
        x = gemm_inputs(gen(100 + variant), M, N, K, profile, BF16)
        for name, kw in gemm_cases().items():
            gemm_budget_case(ck, name, variant, BF16, x, kw, profile)
    finally:
        tuning("gemm_variant", 0)
    ck.done()


def gemm_scaling_cases(ck, kernel, variant, dt, x, cases, ks=(-24, 24)):
    for name, kw in cases.items():
        base, _ = gemm_launch(dt, x, kw)
        if base is None:
            continue
        for operand in ("A", "W"):
            for k in ks:
                got, _ = gemm_launch(dt, x, kw, **{"scale_a" if operand == "A" else "scale_w": k})
                for key in base:
                    if key == "has_bits":
                        continue
                    if key == "bits":
                        ck.same(kernel, f"v{variant} {name} keep bits under {operand} x 2^{k}", base[key], got[key])
                    else:
                        ck.scaling(kernel, f"v{variant} {name} {key} in {operand}", base[key], got[key], k)


@pytest.mark.parametrize("variant", [2, 9, 24])
def test_gemm_bf16_scaling(variant):
    """Every epilogue scales bit for bit in A and in B (bias, residual and C under beta 1 scaled with it;
    the ReLU keep bits unchanged; row dots and column partials scaled)."""
    M, N, K = GEMM_SHAPE[variant]
    if tuning("gemm_variant", variant) != 0:
        pytest.skip(f"gemm_variant {variant} is A/B-only (not in this library build)")
    ck = Checks("GEMM bf16")
    try:
        gemm_scaling_cases(ck, "cg_gemm", variant, BF16, gemm_inputs(gen(100 + variant), M, N, K, "unit", BF16),
                           gemm_cases())
    finally:
        tuning("gemm_variant", 0)
    ck.done()


F32_GEMMS = [  # name, (M, N, K), gemm_variant, cases
    ("mfma", (257, 378, 504), 0, {"bias NN": dict(kind=1, bias=True), "store NT": dict(bt=1), "store TN": dict(at=1),
                                  "bias TT": dict(kind=1, bias=True, at=1, bt=1), "bias_resid NN": dict(kind=3, bias=True, resid=True),
                                  "bias_relu NN": dict(kind=2, bias=True), "beta1 TT": dict(at=1, bt=1, beta=1.0)}),
    ("small-M", (33, 70, 5), 0, {"bias NN": dict(kind=1, bias=True), "bias_resid NN": dict(kind=3, bias=True, resid=True)}),
    ("small-M", (256, 126, 504), 0, {"bias NN": dict(kind=1, bias=True), "bias_resid NN": dict(kind=3, bias=True, resid=True)}),
    ("generic", (37, 65, 126), 99, {"bias NN": dict(kind=1, bias=True), "store NT": dict(bt=1), "store TN": dict(at=1),
                                    "bias_drop_resid TT": dict(kind=4, bias=True, resid=True, p=0.2, at=1, bt=1)}),
    ("split 4", (126, 504, 1000), 0, {"bias NN split4": dict(kind=1, bias=True, split=4),
                                      "bias TT split4": dict(kind=1, bias=True, split=4, at=1, bt=1)}),
]


@pytest.mark.parametrize("profile", ["unit", "outlier", "scaling"])
@pytest.mark.parametrize("name,shape,variant,cases", F32_GEMMS, ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}" for n, s, _, _ in F32_GEMMS])
def test_gemm_f32(name, shape, variant, cases, profile):
    """The fp32 kernels: MFMA, small-M, generic, split-K 4.  profile "scaling": the exact-scaling runs."""
    M, N, K = shape
    assert tuning("gemm_variant", variant) == 0
    ck = Checks("GEMM fp32")
    try:
        x = gemm_inputs(gen(200 + M), M, N, K, "unit" if profile == "scaling" else profile, F32)
        if profile == "scaling":
            gemm_scaling_cases(ck, "cg_gemm f32", f"{variant} {name} {shape}", F32, x, cases)
        else:
            for cname, kw in cases.items():
                gemm_budget_case(ck, f"{name} {cname}", variant, F32, x, kw, profile, kernel="cg_gemm f32")
    finally:
        tuning("gemm_variant", 0)
    ck.done()


# ==== cg_gemm_wgrad_group ================================================================================
WGRAD_PAIRS = {"attention": [(384, 384), (1152, 384)], "ffn": [(1536, 384), (384, 1536)]}


def run_wgrad_group(probs, tokens, flags, beta, scale=None):
    """probs: [(dy [tokens, N], x [tokens, K], C0 [N, K])] CPU; scale: (operand 0 / 1, k).  Returns the outs."""
    dys, xs, outs, wss = [], [], [], []
    for dy, xx, C0 in probs:
        f = [1.0, 1.0]
        if scale:
            f[scale[0]] = 2.0 ** scale[1]
        dys.append(D(dy * f[0], BF16))
        xs.append(D(xx * f[1], BF16))
        outs.append(D(C0 * f[0] * f[1], F32) if beta else torch.full(C0.shape, NAN, device=DEV))
        wss.append(torch.empty(max(16, ops().gemm_workspace(dy.shape[1], xx.shape[1], 2)), dtype=torch.uint8, device=DEV))
    betas, splits = [float(beta)] * len(probs), [2] * len(probs)
    if not ops().gemm_wgrad_group_supported(dys, xs, outs, wss, betas, splits, flags):
        return None
    ops().gemm_wgrad_group(dys, xs, outs, wss, betas, splits, flags)
    sync("cg_gemm_wgrad_group")
    return [o.cpu() for o in outs]


def wgrad_tokens(pair):
    """The smallest token count (the products' K) the group's predicate accepts at split 2."""
    for tokens in (128, 256, 512, 1024):
        probs = [(torch.zeros(tokens, n), torch.zeros(tokens, k), torch.zeros(n, k)) for n, k in WGRAD_PAIRS[pair]]
        if run_wgrad_group(probs, tokens, 0, 0.0) is not None:
            return tokens
    raise AssertionError(f"cg_gemm_wgrad_group_supported refuses the {pair} pair up to 1024 tokens")


@pytest.mark.parametrize("profile", ["unit", "outlier", "scaling"])
@pytest.mark.parametrize("pair", ["attention", "ffn"])
def test_gemm_wgrad_group(pair, profile):
    """The attention sublayer's and the FeedForward's weight-gradient pairs as one split-K launch each,
    fp32 and bf16 slabs, beta 0 and 1."""
    ck = Checks("grouped wgrad")
    tokens = wgrad_tokens(pair)
    g = gen(300)
    probs = []
    for n, k in WGRAD_PAIRS[pair]:
        A, W, _ = nm.gemm_operands(g, n, k, tokens, "unit" if profile == "scaling" else profile, BF16)
        probs.append((A.t().contiguous(), W.t().contiguous(), torch.randn(n, k, generator=g)))
    for flags, beta in ((0, 0.0), (1, 0.0), (0, 1.0)):
        outs = run_wgrad_group(probs, tokens, flags, beta)
        assert outs is not None
        for (dy, xx, C0), out in zip(probs, outs):
            shape = f"({dy.shape[1]}, {xx.shape[1]}, {tokens}) split 2 flags {flags} beta {beta:g}"
            if profile == "scaling":
                continue
            A, W = dy.t(), xx.t()
            kw = dict(beta=beta, C0=C0 if beta else None)
            ref, S = nm.gemm_budget(A, W, **kw)
            pk = dict(kw, slab_splits=2) if flags else kw
            u = UBF if flags else U32
            ck.budget("cg_gemm_wgrad_group", shape, profile, "C", out, ref, S, u, nm.gemm_rho_plain(A, W, ref, S, F32, **pk),
                      nm.dot_cap(tokens, 4, BF16 if flags else F32))
        if profile == "scaling":
            for operand in (0, 1):
                for k in (-24, 24):
                    got = run_wgrad_group(probs, tokens, flags, beta, scale=(operand, k))
                    for i, (b_, g_) in enumerate(zip(outs, got)):
                        ck.scaling("cg_gemm_wgrad_group", f"{pair} problem {i} flags {flags} beta {beta:g} in {'AB'[operand]}", b_, g_, k)
    ck.done()


# ==== cg_gemm_resid_layernorm ============================================================================
@pytest.mark.parametrize("profile", ["offset", "outlier", "flat"])
@pytest.mark.parametrize("M,K", [(64, 64), (192, 640)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_gemm_resid_layernorm(M, K, p, profile):
    """out = resid + [dropout](A W^T + bias) and the LayerNorm of it, the residual carrying the profile.
    flat: the product is scaled by 2^-20 so that the rows stay flat (variance below eps)."""
    N = 384
    assert lib().cg_gemm_resid_layernorm_supported(M, N, K)
    ck = Checks("GEMM + LayerNorm")
    g = gen(400 + M)
    A, W, _ = nm.gemm_operands(g, M, N, K, "unit", BF16)
    W = W * (K ** -0.5 if profile != "flat" else 2.0 ** -20)
    W = nm.rnd(W, BF16)
    bias = torch.randn(N, generator=g) * (0.1 if profile != "flat" else 1e-6)
    resid = nm.ln_rows(g, M, N, profile)
    lw, lb = nm.ln_params(g, N)
    a, w, bb, rr, lwd, lbd = D(A, BF16), D(W, BF16), D(bias), D(resid), D(lw), D(lb)
    out = torch.full((M, N), NAN, device=DEV)
    y = torch.full((M, N), NAN, dtype=BF16, device=DEV)
    mean, rstd = torch.full((M,), NAN, device=DEV), torch.full((M,), NAN, device=DEV)
    call = dev_i64(6)
    ops().gemm_resid_layernorm(a, w, out, M, N, K, K, K, N, bb, rr, N, p, 41, call if p else None, 2, lwd, lbd, y, mean,
                               rstd, nm.EPS)
    sync("cg_gemm_resid_layernorm")
    shape = f"({M}, {N}, {K}) p {p}"
    kw = dict(bias=bias, resid=resid, keep=keep_mult(41, 6, 2, (M, N), p) if p else None)
    ref, S = nm.gemm_budget(A, W, **kw)
    ck.budget("cg_gemm_resid_layernorm", shape, profile, "x", out, ref, S, U32, nm.gemm_rho_plain(A, W, ref, S, F32, **kw),
              nm.dot_cap(K, 4))
    xg = out.cpu()      # y, mean, rstd: the LayerNorm of the x just written
    bud = nm.ln_fwd_budget(xg, lw, lb)
    plain = nm.ln_fwd_rho_plain(xg, lw, lb, bud, BF16)
    for name, got, u in (("y", y, UBF), ("mean", mean, U32), ("rstd", rstd, U32)):
        ck.budget("cg_gemm_resid_layernorm", shape, profile, name, got, *bud[name], u, plain[name])
    ck.done()


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_gemm_resid_layernorm_scaling(p):
    """x = resid + [dropout](A W^T + bias) is linear in (A, bias, resid): x scales bit for bit (y does not:
    eps is an absolute term of the LayerNorm by design)."""
    M, N, K = 192, 384, 640
    ck = Checks("GEMM + LayerNorm")
    g = gen(450)
    A, W, _ = nm.gemm_operands(g, M, N, K, "unit", BF16)
    W = nm.rnd(W * K ** -0.5, BF16)
    bias, resid = torch.randn(N, generator=g) * 0.1, torch.randn(M, N, generator=g)
    lw, lb = nm.ln_params(g, N)

    def run(k):
        f = 2.0 ** k
        out = torch.full((M, N), NAN, device=DEV)
        y = torch.full((M, N), NAN, dtype=BF16, device=DEV)
        mean, rstd = torch.full((M,), NAN, device=DEV), torch.full((M,), NAN, device=DEV)
        call = dev_i64(6)
        ops().gemm_resid_layernorm(D(A * f, BF16), D(W, BF16), out, M, N, K, K, K, N, D(bias * f), D(resid * f), N, p, 41,
                                   call if p else None, 2, D(lw), D(lb), y, mean, rstd, nm.EPS)
        sync("cg_gemm_resid_layernorm")
        return out.cpu()

    base = run(0)
    for k in (-24, 24):
        ck.scaling("cg_gemm_resid_layernorm", f"({M}, {N}, {K}) p {p} x in (A, bias, resid)", base, run(k), k)
    ck.done()


# ==== LayerNorm forward =====================================================================================
def run_ln_fwd(x, w, b, y_dt, fused):
    rows, C = x.shape
    xd, wd, bd = D(x), D(w), D(b)
    y = torch.full((rows, C), NAN, dtype=y_dt, device=DEV)
    mean, rstd = torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    a = (P(xd), P(wd), P(bd), P(y), code(y_dt), P(mean), P(rstd), rows, C, nm.EPS)
    if fused:
        B, H, T = 1, 2, 64
        mask = torch.zeros(lib().cg_attn_mask_bytes(B, H, T), dtype=torch.uint8, device=DEV)
        call = dev_i64(3)
        ok(lib().cg_layernorm_fwd_attn_dropmask(*a, B, H, T, 0.2, 77, P(call), 2, P(mask), stream()), "cg_layernorm_fwd_attn_dropmask")
    else:
        ok(lib().cg_layernorm_fwd(*a, stream()), "cg_layernorm_fwd")
    return y.cpu(), mean.cpu(), rstd.cpu()


@pytest.mark.parametrize("profile", ["unit", "offset", "outlier", "flat"])
@pytest.mark.parametrize("C", [2, 33, 64, 126, 384, 768, 1024])
def test_layernorm_fwd(C, profile):
    """cg_layernorm_fwd with fp32 and bf16 output and cg_layernorm_fwd_attn_dropmask, 67 rows: y, mean, rstd."""
    rows = 67
    ck = Checks("LayerNorm forward")
    g = gen(500 + C)
    x = nm.ln_rows(g, rows, C, profile)
    w, b = nm.ln_params(g, C)
    bud = nm.ln_fwd_budget(x, w, b)
    for kernel, y_dt, fused in (("cg_layernorm_fwd", F32, False), ("cg_layernorm_fwd", BF16, False),
                                ("cg_layernorm_fwd_attn_dropmask", BF16, True)):
        y, mean, rstd = run_ln_fwd(x, w, b, y_dt, fused)
        plain = nm.ln_fwd_rho_plain(x, w, b, bud, y_dt)
        shape = f"({rows}, {C}) y {str(y_dt)[6:]}"
        ck.budget(kernel, shape, profile, "y", y, *bud["y"], nm.u_of(y_dt), plain["y"])
        ck.budget(kernel, shape, profile, "mean", mean, *bud["mean"], U32, plain["mean"], C + 2)
        ck.budget(kernel, shape, profile, "rstd", rstd, *bud["rstd"], U32, plain["rstd"])
    ck.done()


@pytest.mark.parametrize("C", [126, 384])
def test_layernorm_fwd_scaling(C):
    """The forward is linear in (w, b): y scales bit for bit, mean and rstd keep their bits."""
    rows = 67
    ck = Checks("LayerNorm forward")
    g = gen(500 + C)
    x = nm.ln_rows(g, rows, C, "unit")
    w, b = nm.ln_params(g, C)
    for kernel, y_dt, fused in (("cg_layernorm_fwd", F32, False), ("cg_layernorm_fwd", BF16, False),
                                ("cg_layernorm_fwd_attn_dropmask", BF16, True)):
        y, mean, rstd = run_ln_fwd(x, w, b, y_dt, fused)
        for k in (-24, 24):
            y2, mean2, rstd2 = run_ln_fwd(x, w * 2.0 ** k, b * 2.0 ** k, y_dt, fused)
            ck.scaling(kernel, f"({rows}, {C}) y {str(y_dt)[6:]} in (w, b)", y.float(), y2.float(), k)
            ck.same(kernel, f"mean, rstd under (w, b) x 2^{k}", torch.stack([mean, rstd]), torch.stack([mean2, rstd2]))
    ck.done()


@pytest.mark.parametrize("profile", ["offset", "flat"])
def test_linear_rows_f32_with_layernorm(profile):
    """The fused LayerNorm + Linear of the fp32 inference path (cg_linear_rows_f32 with ln), above 2048
    rows: out = LN(a) W^T + bias; S = S_LN |W|^T + |bias|."""
    M, N, K = 2050, 70, 128
    assert ops().linear_rows_f32_supported(M, N, K)
    ck = Checks("LayerNorm forward")
    g = gen(550)
    a = nm.ln_rows(g, M, K, profile)
    lw, lb = nm.ln_params(g, K)
    W, bias = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    out = torch.full((M, N), NAN, device=DEV)
    ops().linear_rows_f32(D(a), D(lw), D(lb), nm.EPS, D(W), D(bias), None, out, False)
    sync("cg_linear_rows_f32")
    yb = nm.ln_fwd_budget(a, lw, lb)["y"]
    ref = yb[0] @ W.double().t() + bias.double()
    S = yb[1] @ W.double().abs().t() + bias.double().abs()
    rp = 0.0
    for order in ("torch", "twopass"):
        yp = nm.ln_fwd_plain(a, lw, lb, order=order)[0]
        rp = max(rp, rho(yp @ W.t() + bias, ref, S, U32).value)
    ck.budget("cg_linear_rows_f32 ln", (M, N, K), profile, "out", out, ref, S, U32, rp)
    ck.done()


# ==== LayerNorm backward ====================================================================================
LN_BWD_FORMS = [  # form, dy dtype, dres, link copy p (None: no copy), column sums
    ("bwd", BF16, False, None, False), ("bwd", F32, True, 0.0, False), ("ex", BF16, True, 0.0, True),
    ("ex", BF16, False, 0.2, True), ("rows_reduce", F32, True, 0.2, True), ("rows_reduce", BF16, False, None, False)]


def run_ln_bwd(form, dy, dy_dt, x, w, mean, rstd, dres, lp_p, colsum):
    rows, C = x.shape
    dyd, xd, wd, md, rd, dr = D(dy, dy_dt), D(x), D(w), D(mean), D(rstd), D(dres)
    dx = torch.full((rows, C), NAN, device=DEV)
    lp = torch.full((rows, C), NAN, dtype=BF16, device=DEV) if lp_p is not None else None
    dw, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    cs = torch.full((C,), NAN, device=DEV) if colsum else None
    ws = torch.empty(max(16, lib().cg_layernorm_bwd_workspace(rows, C)), dtype=torch.uint8, device=DEV)
    call = dev_i64(9)
    p = lp_p or 0.0
    head = (P(dyd), code(dy_dt), P(xd), P(wd), P(md), P(rd), P(dr), P(dx), P(lp))
    rng = (p, 11, P(call) if p else None, 4)
    if form == "bwd":
        ok(lib().cg_layernorm_bwd(*head, P(dw), P(db), 0, P(ws), rows, C, stream()), "cg_layernorm_bwd")
    elif form == "ex":
        ok(lib().cg_layernorm_bwd_ex(*head, *rng, P(dw), P(db), P(cs), 0, 0, P(ws), rows, C, stream()), "cg_layernorm_bwd_ex")
    else:
        ok(lib().cg_layernorm_bwd_rows(*head, *rng, int(colsum), P(ws), rows, C, stream()), "cg_layernorm_bwd_rows")
        ok(lib().cg_layernorm_bwd_reduce(P(ws), rows, C, int(colsum), P(dw), P(db), P(cs), 0, 0, stream()), "cg_layernorm_bwd_reduce")
    return {"dx": dx.cpu(), "dw": dw.cpu(), "db": db.cpu(), "lp": lp.cpu() if lp is not None else None,
            "cs": cs.cpu() if cs is not None else None}


def ln_bwd_inputs(g, rows, C, profile):
    x = nm.ln_rows(g, rows, C, profile)
    w, b = nm.ln_params(g, C)
    _, mean, rstd = nm.ln_fwd_plain(x, w, b)
    return x, w, mean, rstd, torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)


@pytest.mark.parametrize("profile", ["unit", "offset", "outlier", "flat"])
@pytest.mark.parametrize("C", [126, 384, 768])
@pytest.mark.parametrize("rows", [7, 1000])
def test_layernorm_bwd(rows, C, profile):
    """cg_layernorm_bwd / _ex / _rows + _reduce with bf16 and fp32 dy, with and without dres and the
    GradLink copy (plain and with dropout): dx, dw, db and the copy's column sums."""
    ck = Checks("LayerNorm backward")
    x, w, mean, rstd, dy32, dres = ln_bwd_inputs(gen(600 + C + rows), rows, C, profile)
    for form, dy_dt, has_dres, lp_p, colsum in LN_BWD_FORMS:
        dy = nm.rnd(dy32, dy_dt)
        dr = dres if has_dres else None
        got = run_ln_bwd(form, dy, dy_dt, x, w, mean, rstd, dr, lp_p, colsum)
        bud = nm.ln_bwd_budget(dy, x, w, mean, rstd, dr)
        plain = nm.ln_bwd_rho_plain(dy, x, w, mean, rstd, bud, dr)
        kernel = {"bwd": "cg_layernorm_bwd", "ex": "cg_layernorm_bwd_ex", "rows_reduce": "cg_layernorm_bwd_rows+reduce"}[form]
        shape = f"({rows}, {C}) dy {str(dy_dt)[6:]} dres {int(has_dres)} link {lp_p}"
        for name, cap in (("dx", None), ("dw", None), ("db", rows + 2)):
            ck.budget(kernel, shape, profile, name, got[name], *bud[name], U32, plain[name], cap)
        if lp_p is not None:    # the copy is bf16(keep ? dx / (1 - p) : 0) of the dx just written
            mult = keep_mult(11, 9, 4, (rows, C), lp_p).float() if lp_p else torch.ones(rows, C)
            z = got["dx"] * mult
            ck.same(kernel, f"{shape} link copy", got["lp"], z.to(BF16))
            if colsum:
                r_, s_ = nm.sum_budget(z, 0)
                ck.budget(kernel, shape, profile, "link colsum", got["cs"], r_, s_, U32, nm.sum_rho_plain(z, r_, s_, 0), rows + 3)
    ck.done()


@pytest.mark.parametrize("form,dy_dt,has_dres,lp_p,colsum", LN_BWD_FORMS)
def test_layernorm_bwd_scaling(form, dy_dt, has_dres, lp_p, colsum):
    """Linear in (dy, dres): dx, dw, db, the link copy and its column sums scale bit for bit."""
    rows, C = 1000, 384
    ck = Checks("LayerNorm backward")
    x, w, mean, rstd, dy32, dres = ln_bwd_inputs(gen(700), rows, C, "unit")
    dy = nm.rnd(dy32, dy_dt)
    base = run_ln_bwd(form, dy, dy_dt, x, w, mean, rstd, dres if has_dres else None, lp_p, colsum)
    for k in (-24, 24):
        f = 2.0 ** k
        got = run_ln_bwd(form, dy * f, dy_dt, x, w, mean, rstd, dres * f if has_dres else None, lp_p, colsum)
        for name in base:
            if base[name] is not None:
                ck.scaling(f"cg_layernorm_{form}", f"{name} in dy{' and dres' if has_dres else ''} (link {lp_p})", base[name], got[name], k)
    ck.done()


# ==== attention =============================================================================================
ATTN_CASES = [  # family, dt, B, T, H, D, profiles
    ("attention D = 64 resident", BF16, 2, 64, 2, 64, ("unit", "peaked", "sink", "shifted", "spiked")),
    ("attention D = 64 resident", BF16, 2, 192, 2, 64, ("unit", "peaked", "sink", "shifted", "spiked")),
    ("attention ring", BF16, 1, 320, 2, 64, ("unit", "peaked", "sink", "shifted", "spiked")),
    ("attention generic", BF16, 2, 37, 3, 21, ("unit", "peaked", "sink", "shifted")),
    ("attention fp32", F32, 2, 37, 3, 21, ("unit", "peaked", "sink", "shifted")),
    ("attention fp32", F32, 1, 130, 4, 16, ("unit", "peaked", "sink", "shifted")),
]


def run_attn(dt, q, k, v, dO, scale, p, bwd=("mask", "regen", "delta"), fwd_only=False):
    """cg_attn_fwd and the backward forms on [B, T, H, D] CPU operands.  Returns {"o", "lse", and per
    backward form b: "dq b", "dk b", "dv b"} on the CPU ([B, T, H, D]; lse [B, H, T])."""
    B, T, H, Dh = q.shape
    d, BT = H * Dh, B * T
    fast = dt == BF16 and Dh == 64 and T % 64 == 0
    qkv = D(torch.cat([t.reshape(BT, d) for t in (q, k, v)], 1), dt)
    o = torch.full((BT, d), NAN, dtype=dt, device=DEV)
    lse = torch.full((B * H * T,), NAN, device=DEV)
    call = dev_i64(2)
    nmask = lib().cg_attn_mask_bytes(B, H, T) if fast and p > 0 else 0
    mask = torch.zeros(max(nmask, 8), dtype=torch.uint8, device=DEV) if nmask else None
    ok(lib().cg_attn_fwd(code(dt), B, T, H, Dh, P(qkv), P(qkv, d), P(qkv, 2 * d), 3 * d, P(o), d, P(lse), scale, p, 11,
                         P(call), 7, P(mask), stream()), "cg_attn_fwd")
    res = {"o": o.cpu().float().view(B, T, H, Dh), "lse": lse.cpu().view(B, H, T)}
    if fwd_only:
        return res
    dod = D(dO.reshape(BT, d), dt)
    ws = torch.empty(max(16, lib().cg_attn_bwd_workspace(B, T, H, Dh)), dtype=torch.uint8, device=DEV)
    for form in bwd:
        if form == "regen" and mask is None:
            continue
        dqkv = torch.full((BT, 3 * d), NAN, dtype=dt, device=DEV)
        delta = None
        if form == "delta":     # rowsum(dO * O) over each head, fp32 [B, H, T], from the o the forward wrote
            delta = (dod.float() * o.float()).view(B, T, H, Dh).sum(-1).permute(0, 2, 1).contiguous()
        a = (code(dt), B, T, H, Dh, P(qkv), P(qkv, d), P(qkv, 2 * d), 3 * d, P(o), d, P(dod), d, P(lse))
        z = (P(dqkv), P(dqkv, d), P(dqkv, 2 * d), 3 * d, scale, p, 11, P(call), 7, P(None if form == "regen" else mask), P(ws),
             stream())
        ok(lib().cg_attn_bwd_delta(*a, P(delta), *z), f"cg_attn_bwd_delta ({form})")
        g = dqkv.cpu().float()
        for i, nme in enumerate(("dq", "dk", "dv")):
            res[f"{nme} {form}"] = g[:, i * d:(i + 1) * d].reshape(B, T, H, Dh)
    return res


def attn_inputs(g, dt, B, T, H, Dh, profile):
    q, k, v, scale = nm.attn_operands(g, B, T, H, Dh, profile)
    q, k, v = (nm.rnd(t, dt) for t in (q, k, v))
    dO = nm.rnd(torch.randn(B, T, H, Dh, generator=gen(801)), dt)
    return q, k, v, dO, scale


def _attn_ids():
    return [f"{f.split()[-1]}-{str(dt)[6:]}-T{T}-D{Dh}" for f, dt, B, T, H, Dh, _ in ATTN_CASES]


ATTN_BUDGET = [(c[:6], prof) for c in ATTN_CASES for prof in c[6]]


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("case,profile", ATTN_BUDGET,
                         ids=[f"{c[0].split()[-1]}-{str(c[1])[6:]}-T{c[3]}-D{c[5]}-{prof}" for c, prof in ATTN_BUDGET])
def test_attention_budget(case, profile, p):
    """Forward o and lse, backward dq, dk, dv with the keep bits supplied, regenerated, and with delta
    precomputed (cg_attn_bwd_delta)."""
    family, dt, B, T, H, Dh = case
    ck = Checks(family)
    q, k, v, dO, scale = attn_inputs(gen(800 + T), dt, B, T, H, Dh, profile)
    got = run_attn(dt, q, k, v, dO, scale, p)
    keep = keep_mult(11, 2, 7, (B, H, T, T), p) if p else None
    d64 = dt == BF16 and Dh == 64
    bud = nm.attn_budget(q, k, v, dO, scale, keep, fp32_cond=dt == F32)
    plain = nm.attn_plain(q, k, v, dO, scale, keep, dt, round_p=d64)
    u = nm.u_of(dt)
    shape = f"({B}, {T}, {H}, {Dh}) {str(dt)[6:]} p {p}"
    for name in got:
        base = name.split()[0]
        ck.budget("cg_attn_fwd" if base in ("o", "lse") else "cg_attn_bwd_delta", shape, profile, name, got[name], *bud[base], u,
                  rho(plain[base], *bud[base], u).value)
    if dt == BF16:      # the bf16 kernels' own bound on lse: 2^-8 absolute
        err = float((got["lse"].double() - bud["lse"][0]).abs().max())
        ck.require(err < 2.0 ** -8, f"cg_attn_fwd {shape} {profile}: |lse - ref| {err:.3g} >= 2^-8")
    ck.done()


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("family,dt,B,T,H,Dh,profiles", ATTN_CASES, ids=_attn_ids())
def test_attention_scaling(family, dt, B, T, H, Dh, profiles, p):
    """Forward in v (o scales, lse unchanged to the bit), forward with q 2^k and scale 2^-k (o and lse
    unchanged to the bit), backward in dO (dq, dk, dv scale)."""
    ck = Checks(family)
    q, k, v, dO, scale = attn_inputs(gen(800 + T), dt, B, T, H, Dh, "unit")
    base = run_attn(dt, q, k, v, dO, scale, p)
    shape = f"({B}, {T}, {H}, {Dh}) {str(dt)[6:]} p {p}"
    for e in (-24, 24):
        f = 2.0 ** e
        got = run_attn(dt, q, k, v * f, dO, scale, p, fwd_only=True)
        ck.scaling("cg_attn_fwd", f"{shape} o in v", base["o"], got["o"], e)
        ck.same("cg_attn_fwd", f"{shape} lse under v x 2^{e}", base["lse"], got["lse"])
        got = run_attn(dt, q * f, k, v, dO, scale / f, p, fwd_only=True)
        ck.scaling("cg_attn_fwd", f"{shape} o under q 2^k, scale 2^-k", base["o"], got["o"], 0)
        ck.same("cg_attn_fwd", f"{shape} lse under q x 2^{e}, scale x 2^{-e}", base["lse"], got["lse"])
        got = run_attn(dt, q, k, v, dO * f, scale, p)
        for name in base:
            if name not in ("o", "lse"):
                ck.scaling("cg_attn_bwd_delta", f"{shape} {name} in dO", base[name], got[name], e)
    ck.done()


# ==== cross entropy and the head ============================================================================
@pytest.mark.parametrize("profile", ["unit", "confident", "wrong", "offset", "scaling"])
def test_cross_entropy(profile):
    """cg_ce_fwd / cg_ce_bwd at (64, 65): the loss per row, lse, dlogits (and its bf16 copy)."""
    rows, V = 64, 65
    ck = Checks("cross entropy")
    x, tgt = nm.ce_logits(gen(900), rows, V, "unit" if profile == "scaling" else profile)
    xd, td = D(x), D(tgt)
    loss, lse = torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    ok(lib().cg_ce_fwd(P(xd), rows, V, V, P(td), P(loss), P(lse), stream()), "cg_ce_fwd")

    def bwd(gval):
        gd = torch.full((1,), gval, device=DEV)
        dl = torch.full((rows, V), NAN, device=DEV)
        lp = torch.full((rows, V), NAN, dtype=BF16, device=DEV)
        ok(lib().cg_ce_bwd(P(xd), rows, V, V, P(td), P(lse), P(gd), 1.0 / rows, P(dl), V, P(lp), stream()), "cg_ce_bwd")
        return dl.cpu(), lp.cpu()

    dl, lp = bwd(2.0)
    gm = float(np.float32(2.0) * np.float32(1.0 / rows))
    if profile == "scaling":
        for k in (-24, 24):
            dl2, lp2 = bwd(2.0 * 2.0 ** k)
            ck.scaling("cg_ce_bwd", "dlogits in g_loss", dl, dl2, k)
            ck.scaling("cg_ce_bwd", "bf16 dlogits in g_loss", lp, lp2, k)
    else:
        bud, plain = nm.ce_budget(x, tgt), nm.ce_plain(x, tgt)
        for name, got in (("lse", lse), ("loss", loss)):
            ck.budget("cg_ce_fwd", (rows, V), profile, name, got, *bud[name], U32, rho(plain[name], *bud[name], U32).value)
        lse_in = lse.cpu()
        bud = nm.ce_budget(x, tgt, gm, lse_in)
        ck.budget("cg_ce_bwd", (rows, V), profile, "dlogits", dl, *bud["dlogits"], U32,
                  rho(nm.ce_plain(x, tgt, gm, lse_in)["dlogits"], *bud["dlogits"], U32).value)
        ck.same("cg_ce_bwd", "bf16 copy", lp, dl.to(BF16))
    ck.done()


@pytest.mark.parametrize("profile", ["unit", "confident", "wrong", "offset", "scaling"])
@pytest.mark.parametrize("M,C,V", [(256, 384, 65), (64, 96, 16)])
def test_head(M, C, V, profile):
    """cg_head_fwd (logits, lse, the mean loss) and cg_head_bwd / cg_head_bwd_ex (dl bf16, db)."""
    ck = Checks("head")
    a, W, bias, tgt = nm.head_operands(gen(950 + M), M, C, V, "unit" if profile == "scaling" else profile)
    rowsW = (V + 15) // 16 * 16
    wpad = torch.zeros(rowsW, C)
    wpad[:V] = W
    ad, wd, bd, td = D(a, BF16), D(wpad, BF16), D(bias), D(tgt)
    logits = torch.full((M, V), NAN, device=DEV)
    lse, loss = torch.full((M,), NAN, device=DEV), torch.full((1,), NAN, device=DEV)
    ws = torch.empty(max(16, lib().cg_head_workspace(M, V)), dtype=torch.uint8, device=DEV)
    ok(lib().cg_head_fwd(P(ad), P(wd), rowsW, P(bd), P(td), P(logits), P(lse), P(loss), P(ws), M, C, V, stream()), "cg_head_fwd")

    def bwd(gval, ex):
        gd = torch.full((1,), gval, device=DEV)
        dl = torch.full((M, rowsW), NAN, dtype=BF16, device=DEV)
        db = torch.full((V,), NAN, device=DEV)
        a_ = (P(logits), P(lse), P(td), P(gd), 1.0 / M, None, P(dl), rowsW, P(db), 0, P(ws), M, V)
        ok(lib().cg_head_bwd_ex(*a_, 0, stream()) if ex else lib().cg_head_bwd(*a_, stream()), "cg_head_bwd")
        return dl.cpu().float(), db.cpu()

    shape = (M, C, V)
    if profile == "scaling":
        for ex in (False, True):
            dl, db = bwd(2.0, ex)
            for k in (-24, 24):
                dl2, db2 = bwd(2.0 * 2.0 ** k, ex)
                ck.scaling("cg_head_bwd_ex" if ex else "cg_head_bwd", "dl in g_loss", dl, dl2, k)
                ck.scaling("cg_head_bwd_ex" if ex else "cg_head_bwd", "db in g_loss", db, db2, k)
        ck.done()
        return
    ref, S = nm.gemm_budget(a, W, bias=bias)
    ck.budget("cg_head_fwd", shape, profile, "logits", logits, ref, S, U32, nm.gemm_rho_plain(a, W, ref, S, F32, bias=bias),
              nm.dot_cap(C, 1))
    xg = logits.cpu()       # lse and the loss: functions of the logits just written
    bud, plain = nm.ce_budget(xg, tgt), nm.ce_plain(xg, tgt)
    ck.budget("cg_head_fwd", shape, profile, "lse", lse, *bud["lse"], U32, rho(plain["lse"], *bud["lse"], U32).value)
    lref, lS = bud["loss"][0].mean().reshape(1), bud["loss"][1].mean().reshape(1)
    ck.budget("cg_head_fwd", shape, profile, "loss", loss, lref, lS, U32,
              nm.sum_rho_plain(plain["loss"][:, None] / M, lref, lS, 0), M + 3)
    gm = float(np.float32(2.0) * np.float32(1.0 / M))
    lse_in = lse.cpu()
    bud = nm.ce_budget(xg, tgt, gm, lse_in)["dlogits"]
    pl = nm.ce_plain(xg, tgt, gm, lse_in)["dlogits"]
    for ex in (False, True):
        dl, db = bwd(2.0, ex)
        kernel = "cg_head_bwd_ex" if ex else "cg_head_bwd"
        ck.budget(kernel, shape, profile, "dl", dl[:, :V], *bud, UBF, rho(nm.rnd(pl, BF16), *bud, UBF).value)
        ck.require(float(dl[:, V:].abs().max()) == 0.0 if rowsW > V else True, f"{kernel} {shape}: padding columns of dl not zero")
        r_, s_ = bud[0].sum(0), bud[1].sum(0)
        ck.budget(kernel, shape, profile, "db", db, r_, s_, U32, nm.sum_rho_plain(pl, r_, s_, 0), M + 4)
    ck.done()


# ==== embeddings and reductions ==============================================================================
@pytest.mark.parametrize("mode", ["outlier", "scaling"])
@pytest.mark.parametrize("V,T,C,B", [(65, 40, 126, 3), (65, 64, 384, 16)])
def test_embedding_bwd(V, T, C, B, mode):
    """cg_embed_bwd (the histogram form and the fused pass) with one token in 90 % of the positions and
    outlier channels in dx."""
    ck = Checks("embedding")
    idx, dx, _ = nm.embed_operands(gen(1000 + B), V, T, C, B)

    def run(dxx):
        dwte, dwpe = torch.full((V, C), NAN, device=DEV), torch.full((T, C), NAN, device=DEV)
        ws = torch.empty(max(16, lib().cg_embed_bwd_workspace(B, T, C, V)), dtype=torch.uint8, device=DEV)
        ixd, dxd = D(idx), D(dxx)
        ok(lib().cg_embed_bwd(P(ixd), P(dxd), P(dwte), P(dwpe), B, T, C, V, 0, P(ws), stream()), "cg_embed_bwd")
        return {"dwte": dwte.cpu(), "dwpe": dwpe.cpu()}

    got = run(dx)
    if mode == "scaling":
        for k in (-24, 24):
            g2 = run(dx * 2.0 ** k)
            for name in got:
                ck.scaling("cg_embed_bwd", f"({V}, {T}, {C}, {B}) {name} in dx", got[name], g2[name], k)
    else:
        bud, plain = nm.embed_budget(idx, dx, V), nm.embed_plain(idx, dx, V)
        for name, cap in (("dwte", B * T + 2), ("dwpe", B + 2)):
            ck.budget("cg_embed_bwd", (V, T, C, B), "outlier", name, got[name], *bud[name], U32,
                      rho(plain[name], *bud[name], U32).value, cap)
    ck.done()


@pytest.mark.parametrize("mode", ["outlier", "scaling"])
def test_reductions(mode):
    """cg_colsum (fp32 and bf16), cg_reduce_rows, cg_sum_f32 on outlier data; with cg_dropout_apply and
    cg_grad_norm in the scaling runs."""
    ck = Checks("reductions")
    ks = (-24, 24)

    def colsum(x, dt):
        rows, N = x.shape
        xd, out = D(x, dt), torch.full((N,), NAN, device=DEV)
        ws = torch.empty(max(16, lib().cg_colsum_workspace(rows, N)), dtype=torch.uint8, device=DEV)
        ok(lib().cg_colsum(P(xd), code(dt), rows, N, N, P(out), 0, P(ws), stream()), "cg_colsum")
        return out.cpu()

    def reduce_rows(x):
        rows, N = x.shape
        xd, out = D(x), torch.full((N,), NAN, device=DEV)
        ok(lib().cg_reduce_rows(P(xd), rows, N, P(out), 0, stream()), "cg_reduce_rows")
        return out.cpu()

    def sum_f32(x):
        xd, out = D(x), torch.full((1,), NAN, device=DEV)
        ws = torch.empty(1024, device=DEV)
        ok(lib().cg_sum_f32(P(xd), x.numel(), 0.5, P(out), P(ws), stream()), "cg_sum_f32")
        return out.cpu()

    profile = "outlier" if mode == "outlier" else "unit"
    for dt in (F32, BF16):
        for rows, N in ((33, 70), (1024, 384)):
            x = nm.rnd(nm.ln_rows(gen(1100 + rows), rows, N, profile), dt)
            got = colsum(x, dt)
            if mode == "outlier":
                r_, s_ = nm.sum_budget(x, 0)
                ck.budget("cg_colsum", f"({rows}, {N}) {str(dt)[6:]}", profile, "out", got, r_, s_, U32, nm.sum_rho_plain(x, r_, s_, 0), rows + 2)
            else:
                for k in ks:
                    ck.scaling("cg_colsum", f"({rows}, {N}) {str(dt)[6:]} in x", got, colsum(x * 2.0 ** k, dt), k)
    for rows, N in ((33, 70), (33, 4099)):
        x = nm.ln_rows(gen(1200 + N), rows, N, profile)
        got = reduce_rows(x)
        if mode == "outlier":
            r_, s_ = nm.sum_budget(x, 0)
            ck.budget("cg_reduce_rows", (rows, N), profile, "out", got, r_, s_, U32, nm.sum_rho_plain(x, r_, s_, 0), rows + 2)
        else:
            for k in ks:
                ck.scaling("cg_reduce_rows", f"({rows}, {N}) in part", got, reduce_rows(x * 2.0 ** k), k)
    for n in (1023, 4096 + 3):
        x = nm.ln_rows(gen(1300 + n), 1, n, profile)[0]
        got = sum_f32(x)
        if mode == "outlier":
            r_, s_ = 0.5 * x.double().sum().reshape(1), 0.5 * x.double().abs().sum().reshape(1)
            ck.budget("cg_sum_f32", (n,), profile, "out", got, r_, s_, U32, nm.sum_rho_plain(0.5 * x[:, None], r_, s_, 0), n + 3)
        else:
            for k in ks:
                ck.scaling("cg_sum_f32", f"({n},) in x", got, sum_f32(x * 2.0 ** k), k)
    if mode == "scaling":
        call = dev_i64(5)
        for y_dt in (F32, BF16):
            for p in (0.0, 0.2):
                rows, C = 33, 70
                x = torch.randn(rows, C, generator=gen(1400))

                def drop(xx):
                    xd, y = D(xx), torch.full((rows, C), NAN, dtype=y_dt, device=DEV)
                    ok(lib().cg_dropout_apply(P(xd), rows, C, C, P(y), code(y_dt), p, 31, P(call), 6, stream()), "cg_dropout_apply")
                    return y.cpu().float()

                base = drop(x)
                for k in ks:
                    ck.scaling("cg_dropout_apply", f"({rows}, {C}) y {str(y_dt)[6:]} p {p} in x", base, drop(x * 2.0 ** k), k)
        for n in (1023, 4096 + 3):
            gvec = torch.randn(n, generator=gen(1500))

            def norm(xx):
                xd, out = D(xx), torch.full((2,), NAN, device=DEV)
                ws = torch.empty(max(16, lib().cg_grad_norm_workspace(n)), dtype=torch.uint8, device=DEV)
                ok(lib().cg_grad_norm(P(xd), n, 0.25, P(out), P(ws), stream()), "cg_grad_norm")
                return out.cpu()[:1]

            base = norm(gvec)
            for k in ks:
                ck.scaling("cg_grad_norm", f"({n},) the norm in g", base, norm(gvec * 2.0 ** k), k)
    ck.done()


# ==== AdamW at the edges =================================================================================
@pytest.mark.parametrize("step", [1, 1000, 10 ** 6])
@pytest.mark.parametrize("form", ["adamw", "segments", "dyn", "dyn_gscale"])
def test_adamw_edges(form, step):
    """cg_adamw, cg_adamw_segments and cg_adamw_dyn (with and without the clip coefficient) against the
    numpy restatement of csrc/adamw.h on zero, subnormal, tiny, huge and overflowing moments: the bits
    of p, m, v and p_bf16; where numpy gives an infinity or a NaN the kernel gives the same."""
    p0, g0, m0, v0 = nm.adamw_edge_state()
    n = p0.size
    lr, b1, b2, eps, wd, gs = 3e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5
    pd, gd, md, vd = (torch.from_numpy(a.copy()).to(DEV) for a in (p0, g0, m0, v0))
    sh = torch.zeros(n, dtype=BF16, device=DEV)
    st = dev_i64(step)
    head = (P(pd), P(gd), P(md), P(vd), P(sh))
    inside = np.ones(n, dtype=bool)
    if form == "adamw":
        ok(lib().cg_adamw(*head, n, lr, b1, b2, eps, wd, P(st), stream()), "cg_adamw")
    elif form == "segments":     # multiples of 4: the last 3 elements stay outside
        segs = [(0, 1024), (2048, n // 4 * 4 - 2048)]
        inside[:] = False
        for s0, ln in segs:
            inside[s0:s0 + ln] = True
        arr = (ctypes.c_int64 * 4)(*[v_ for s in segs for v_ in s])
        ok(lib().cg_adamw_segments(*head, arr, 2, lr, b1, b2, eps, wd, P(st), stream()), "cg_adamw_segments")
    else:
        lr_dev = torch.tensor([lr], dtype=F64, device=DEV)
        gs_dev = torch.tensor([gs], dtype=F32, device=DEV)
        ok(lib().cg_adamw_dyn(*head, n, P(lr_dev), P(gs_dev) if form == "dyn_gscale" else None, b1, b2, eps, wd, P(st),
                              stream()), "cg_adamw_dyn")
    Pn, Mn, Vn = nm.adamw_numpy(p0, g0, m0, v0, lr, b1, b2, eps, wd, step, gs if form == "dyn_gscale" else None)
    bad = []
    for name, got, want, init in (("p", pd, Pn, p0), ("m", md, Mn, m0), ("v", vd, Vn, v0)):
        got = got.cpu().numpy()
        want = np.where(inside, want, init)
        nan = np.isnan(want)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (nan & np.isnan(got))
        if not same.all():
            i = int(np.nonzero(~same)[0][0])
            bad.append(f"{name}: {int((~same).sum())} of {n} differ; first at {i} (slot {i % 16}): got {got[i]!r}, numpy {want[i]!r}; "
                       f"inputs p {p0[i]!r} g {g0[i]!r} m {m0[i]!r} v {v0[i]!r}")
    shb = sh.cpu().view(torch.int16).numpy()
    want_sh = np.where(inside, nm.bf16_bits_of(np.where(inside, Pn, 0).astype(np.float32)), 0)
    if not (shb == want_sh).all():
        i = int(np.nonzero(shb != want_sh)[0][0])
        bad.append(f"p_bf16: first difference at {i} (slot {i % 16})")
    assert not bad, f"cg_adamw {form} step {step}:\n" + "\n".join(bad)


# ==== the inference kernels: decode attention ================================================================
DEC_B, DEC_T, DEC_H = 2, 130, 2
DEC_PROFILES = ["unit", "peaked", "sink", "shifted", "spiked"]
DEC_NS = (1, 64, 65, 130)
# form -> (D, Tmax of the cache or None for a window's qkv rows, decode_attn_rows tuning, the kernel it reaches)
DEC_FORMS = {
    "cache130-D21": (21, 130, 1, "k_decode_attn_rows<24,SJ> (sh = 130 x 21 is no multiple of 4)"),
    "cache132-D21": (21, 132, 1, "k_decode_attn_rows<24>"),
    "qkvrows-D21": (21, None, 1, "k_decode_attn_rows<24,SJ>"),
    "generic-D21": (21, 130, 0, "k_decode_attn<24>"),
    "cache130-D64": (64, 130, 1, "k_decode_attn<64>"),
}
_DEC_CACHE = {}


def decode_case(D_, profile):
    """Operands (fp32 values), the budget of o and the per-row rho_plain, computed once per (D, profile)."""
    key = (D_, profile)
    if key not in _DEC_CACHE:
        q, k, v, scale = nm.attn_operands(gen(5), DEC_B, DEC_T, DEC_H, D_, profile)
        q, k, v = (nm.rnd(t, F32) for t in (q, k, v))
        scale = float(np.float32(scale))
        ref, S = nm.attn_budget(q, k, v, torch.zeros_like(q), scale, fp32_cond=True)["o"]
        _DEC_CACHE[key] = (q, k, v, scale, ref, S, nm.decode_attn_rho_plain(q, k, v, scale, ref, S))
    return _DEC_CACHE[key]


def run_decode_attn(form, q, k, v, n, scale, stale=NAN, fixed=False):
    """cg_decode_attn for the query at position n - 1 against keys 0..n-1 in the layout of `form`; the key
    rows >= n hold `stale`.  Returns o [B, H, D] on the CPU."""
    D_, Tmax, _, _ = DEC_FORMS[form]
    B, T, H, _ = q.shape
    HD = H * D_
    qd = D(q[:, n - 1].reshape(B, HD))
    o = torch.full((B, HD), NAN, device=DEV)
    if Tmax is None:
        buf = torch.cat([t.reshape(B, T, HD) for t in (q, k, v)], 2).clone()
        buf[:, n:, HD:] = stale
        bufd = D(buf)
        kp, vp, sb, sh, sj = P(bufd, HD), P(bufd, 2 * HD), T * 3 * HD, D_, 3 * HD
    else:
        kc = torch.full((B, H, Tmax, D_), stale)
        vc = torch.full((B, H, Tmax, D_), stale)
        kc[:, :, :n], vc[:, :, :n] = k[:, :n].permute(0, 2, 1, 3), v[:, :n].permute(0, 2, 1, 3)
        kd, vd = D(kc), D(vc)
        kp, vp, sb, sh, sj = P(kd), P(vd), H * Tmax * D_, Tmax * D_, D_
    ln = None if fixed else dev_i64(n)
    ok(lib().cg_decode_attn(P(qd), HD, kp, vp, sb, sh, sj, B, H, D_, P(ln), n if fixed else 0, scale, P(o), HD, stream()),
       f"cg_decode_attn {form} n {n}")
    return o.cpu().view(B, H, D_)


@pytest.mark.parametrize("profile", DEC_PROFILES)
@pytest.mark.parametrize("form", list(DEC_FORMS))
def test_decode_attn_budget(form, profile):
    """cg_decode_attn at n in {1, 64, 65, 130} keys in every dispatch form, the cache rows past n NaN in one
    run and zero in another (both with a device length): finite, bitwise equal, and inside 8 rho_plain of
    row n - 1; a third run with the key count as an argument gives the same bits."""
    D_, Tmax, rows_tuning, kernel = DEC_FORMS[form]
    q, k, v, scale, ref, S, rp = decode_case(D_, profile)
    ck = Checks("decode attention")
    assert tuning("decode_attn_rows", rows_tuning) == 0
    try:
        for n in DEC_NS:
            got = run_decode_attn(form, q, k, v, n, scale, NAN)
            ck.require(bool(torch.isfinite(got).all()), f"cg_decode_attn {form} n {n} {profile}: non-finite output over NaN stale rows")
            ck.same("cg_decode_attn", f"{form} n {n} {profile}: NaN against zero stale rows (len_dev)", got,
                    run_decode_attn(form, q, k, v, n, scale, 0.0))
            ck.same("cg_decode_attn", f"{form} n {n} {profile}: a fixed nkeys against len_dev (NaN stale rows)", got,
                    run_decode_attn(form, q, k, v, n, scale, NAN, fixed=True))
            ck.budget(f"cg_decode_attn {kernel.split(' ')[0]}", f"({DEC_B}, {DEC_H}, {D_}) {form} n {n}", profile, "o", got,
                      ref[:, n - 1], S[:, n - 1], U32, float(rp[n - 1]))
    finally:
        tuning("decode_attn_rows", 1)
    ck.done()


def run_prefill_attn(q, k, v, scale, Tmax):
    """cg_decode_prefill_attn over all P = T positions from a qkv row buffer.  Returns o [B, T, H, D], kc, vc."""
    B, T, H, D_ = q.shape
    HD = H * D_
    buf = D(torch.cat([t.reshape(B * T, HD) for t in (q, k, v)], 1))
    kc = torch.full((B, H, Tmax, D_), NAN, device=DEV)
    vc = torch.full((B, H, Tmax, D_), NAN, device=DEV)
    o = torch.full((B * T, HD), NAN, device=DEV)
    ok(lib().cg_decode_prefill_attn(P(buf), 3 * HD, P(buf, HD), P(buf, 2 * HD), 3 * HD, B, T, H, D_, Tmax, scale, P(kc), P(vc),
                                    P(o), HD, stream()), "cg_decode_prefill_attn")
    return o.cpu().view(B, T, H, D_), kc.cpu(), vc.cpu()


@pytest.mark.parametrize("profile", DEC_PROFILES)
@pytest.mark.parametrize("D_", [21, 64])
def test_decode_prefill_attn_budget(D_, profile):
    """cg_decode_prefill_attn with P = 130 (QB 8 at D 21, QB 4 at D 64): the whole o against every row of
    the budget; the cache rows are exact copies and the rows past P stay untouched."""
    q, k, v, scale, ref, S, rp = decode_case(D_, profile)
    ck = Checks("decode attention")
    Tmax = DEC_T + 2
    o, kc, vc = run_prefill_attn(q, k, v, scale, Tmax)
    ck.budget(f"cg_decode_prefill_attn QB {8 if D_ <= 24 else 4}", f"({DEC_B}, {DEC_T}, {DEC_H}, {D_})", profile, "o", o, ref, S, U32,
              float(rp.max()))
    ck.same("cg_decode_prefill_attn", "k cache rows", kc[:, :, :DEC_T], k.permute(0, 2, 1, 3).float())
    ck.same("cg_decode_prefill_attn", "v cache rows", vc[:, :, :DEC_T], v.permute(0, 2, 1, 3).float())
    ck.require(bool(torch.isnan(kc[:, :, DEC_T:]).all() and torch.isnan(vc[:, :, DEC_T:]).all()), "cache rows past P written")
    ck.done()


@pytest.mark.parametrize("form", list(DEC_FORMS) + ["prefill-D21", "prefill-D64"])
def test_decode_attn_scaling(form):
    """o scales bit for bit in v (2^-24, 2^24) and keeps its bits under q 2^k with scale 2^-k."""
    ck = Checks("decode attention")
    prefill = form.startswith("prefill")
    D_ = int(form.split("-D")[1])
    q, k, v, scale, _, _, _ = decode_case(D_, "unit")
    assert tuning("decode_attn_rows", 1 if prefill else DEC_FORMS[form][2]) == 0

    def run(q_, v_, sc, n):
        return run_prefill_attn(q_, k, v_, sc, DEC_T)[0] if prefill else run_decode_attn(form, q_, k, v_, n, sc, 0.0)

    try:
        for n in ((DEC_T,) if prefill else (65, 130)):
            base = run(q, v, scale, n)
            for e in (-24, 24):
                f = 2.0 ** e
                ck.scaling("cg_decode_prefill_attn" if prefill else "cg_decode_attn", f"{form} n {n} o in v", base, run(q, v * f, scale, n), e)
                ck.scaling("cg_decode_prefill_attn" if prefill else "cg_decode_attn", f"{form} n {n} o under q 2^{e}, scale 2^{-e}", base,
                           run(q * f, v, scale / f, n), 0)
    finally:
        tuning("decode_attn_rows", 1)
    ck.done()


# ==== the inference kernels: log-probabilities ==============================================================
def run_logprob_rows(x, tgt, B, P_):
    """cg_decode_logprob_rows on rows b P + t of x with idx[b, t + 1] = tgt; returns the B P values."""
    V = x.shape[1]
    idx = torch.zeros(B, P_ + 1, dtype=I64)
    idx[:, 1:] = tgt.view(B, P_)
    xd, ixd = D(x), D(idx)
    lp = torch.full((B, P_ + 1), NAN, device=DEV)
    ok(lib().cg_decode_logprob_rows(P(xd), V, V, B, P_, P(ixd), P_ + 1, P(lp), P_ + 1, stream()), "cg_decode_logprob_rows")
    lp = lp.cpu()
    assert bool(torch.isnan(lp[:, 0]).all()), "cg_decode_logprob_rows wrote column 0"
    return lp[:, 1:].reshape(-1)


def run_emit_logprob(x, tgt):
    """Step 4 of cg_decode_emit with forced tokens (n = 3 < prompt_len = 5): the token is the target."""
    rows, V = x.shape
    n, ld = 3, 8
    idx = torch.zeros(rows, ld, dtype=I64)
    idx[:, n] = tgt
    xd, ixd = D(x), D(idx)
    lp = torch.full((rows, ld), NAN, device=DEV)
    plen, lim, end = (torch.full((rows,), val, dtype=I64, device=DEV) for val in (5, 100, 0))
    stop = torch.zeros((V + 63) // 64, dtype=I64, device=DEV)
    pad, ln = dev_i64(0), dev_i64(n)
    ok(lib().cg_decode_emit(P(xd), V, V, rows, 0, None, None, P(ln), P(plen), P(lim), P(end), P(stop), P(pad), P(ixd), ld, P(lp),
                            stream()), "cg_decode_emit")
    assert torch.equal(ixd.cpu(), idx) and int(end.abs().sum()) == 0, "cg_decode_emit wrote a forced row's token or ended it"
    return lp.cpu()[:, n]


@pytest.mark.parametrize("profile", ["unit", "confident", "wrong", "offset", "certain"])
@pytest.mark.parametrize("V", [65, 200])
def test_logprob_budget(V, profile):
    """cg_decode_logprob_rows and cg_decode_emit's step 4 on 64 rows: inside the shift-invariant budget,
    and equal to each other bit for bit on every profile."""
    rows = 64
    ck = Checks("log-probabilities")
    x, tgt = nm.ce_logits(gen(900 + V), rows, V, profile)
    ref, S = nm.logprob_budget(x, tgt)
    rp = nm.logprob_rho_plain(x, tgt, ref, S)
    a, b = run_logprob_rows(x, tgt, 4, 16), run_emit_logprob(x, tgt)
    ck.budget("cg_decode_logprob_rows", (rows, V), profile, "logprob", a, ref, S, U32, rp)
    ck.budget("cg_decode_emit step 4", (rows, V), profile, "logprob", b, ref, S, U32, rp)
    ck.same("cg_decode_emit / cg_decode_logprob_rows", f"({rows}, {V}) {profile}", a, b)
    ck.done()


# ==== the inference kernels: rows_f32.hip ===================================================================
def run_linear_rows(a, lw, lb, W, bias=None, relu=False, resid=None):
    M, K = a.shape
    N = W.shape[0]
    ad, lwd, lbd, wd, bd, rd = D(a), D(lw), D(lb), D(W), D(bias), D(resid)
    out = torch.full((M, N), NAN, device=DEV)
    ok(lib().cg_linear_rows_f32(M, N, K, P(ad), K, P(lwd), P(lbd), nm.EPS, P(wd), K, P(bd), int(relu), P(rd), N, P(out), N, stream()),
       f"cg_linear_rows_f32 {M}x{N}x{K}")
    return out.cpu()


ROW_KINDS = {"store": {}, "bias": dict(bias=True), "bias_relu": dict(bias=True, relu=True), "bias_resid": dict(bias=True, resid=True)}


def row_epilogue(kind, bias, resid, f=1.0):
    kw = ROW_KINDS[kind]
    return dict(bias=bias * f if kw.get("bias") else None, relu=bool(kw.get("relu")), resid=resid * f if kw.get("resid") else None)


@pytest.mark.parametrize("profile", ["offset", "flat", "scaling"])
@pytest.mark.parametrize("K", [126, 128])
def test_linear_rows_f32_ln_small(K, profile):
    """cg_linear_rows_f32 with the LayerNorm at M 33 (the <= 2048-row path through k_gemm_f32r), every
    epilogue kind; profile "scaling": linear in (W, bias) with the residual scaled along."""
    M, N = 33, 70
    ck = Checks("inference rows")
    g = gen(560 + K)
    a = nm.ln_rows(g, M, K, "unit" if profile == "scaling" else profile)
    lw, lb = nm.ln_params(g, K)
    W, bias, resid = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    for kind in ROW_KINDS:
        e = row_epilogue(kind, bias, resid)
        got = run_linear_rows(a, lw, lb, W, **e)
        if profile == "scaling":
            for k in (-24, 24):
                f = 2.0 ** k
                ck.scaling("cg_linear_rows_f32 ln", f"({M}, {N}, {K}) {kind} in (W, bias, resid)", got,
                           run_linear_rows(a, lw, lb, W * f, **row_epilogue(kind, bias, resid, f)), k)
        else:
            ref, S = nm.linear_ln_budget(a, lw, lb, W, **e)
            ck.budget("cg_linear_rows_f32 ln", f"({M}, {N}, {K}) {kind}", profile, "out", got, ref, S, U32,
                      nm.linear_ln_rho_plain(a, lw, lb, W, ref, S, **e))
    ck.done()


@pytest.mark.parametrize("profile", ["outlier", "scaling"])
@pytest.mark.parametrize("M,nb", [(33, 0), (2050, 0), (2050, 1), (2050, 2)])
def test_linear_rows_f32_plain(M, nb, profile):
    """cg_linear_rows_f32 without the LayerNorm on outlier operands: M 33, and M 2050 under every
    linear_rows_nb tuning (k_linear_f32q, k_linear_f32t<1>, <2>); "scaling": linear in a (bias, resid along)."""
    N, K = 70, 126
    ck = Checks("inference rows")
    g = gen(570 + M)
    a, W, _ = nm.gemm_operands(g, M, N, K, "unit" if profile == "scaling" else profile, F32)
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    assert tuning("linear_rows_nb", nb) == 0
    try:
        for kind in ROW_KINDS:
            e = row_epilogue(kind, bias, resid)
            got = run_linear_rows(a, None, None, W, **e)
            name = f"cg_linear_rows_f32 nb {nb}"
            if profile == "scaling":
                for k in (-24, 24):
                    f = 2.0 ** k
                    ck.scaling(name, f"({M}, {N}, {K}) {kind} in (a, bias, resid)", got,
                               run_linear_rows(a * f, None, None, W, **row_epilogue(kind, bias, resid, f)), k)
            else:
                ref, S = nm.linear_ln_budget(a, None, None, W, **e)
                ck.budget(name, f"({M}, {N}, {K}) {kind}", profile, "out", got, ref, S, U32,
                          nm.linear_ln_rho_plain(a, None, None, W, ref, S, **e), nm.dot_cap(K, 3))
    finally:
        tuning("linear_rows_nb", 0)
    ck.done()


@pytest.mark.parametrize("profile", ["offset", "flat", "scaling"])
def test_decode_qkv_f32(profile):
    """cg_decode_qkv_f32 at B 33, C 126, H 6, Tmax 16, position 7: qkv inside the LayerNorm + product
    budget, the appended cache rows exact copies of it, every other cache row untouched."""
    B, C, H, Tmax, pos = 33, 126, 6, 16, 7
    Dh = C // H
    ck = Checks("inference rows")
    g = gen(580)
    x = nm.ln_rows(g, B, C, "unit" if profile == "scaling" else profile)
    lw, lb = nm.ln_params(g, C)
    W = torch.randn(3 * C, C, generator=g) / C ** 0.5

    def run(Wx):
        xd, lwd, lbd, wd = D(x), D(lw), D(lb), D(Wx)
        qkv = torch.full((B, 3 * C), NAN, device=DEV)
        kc, vc = torch.full((B, H, Tmax, Dh), NAN, device=DEV), torch.full((B, H, Tmax, Dh), NAN, device=DEV)
        ln = dev_i64(pos + 1)
        ok(lib().cg_decode_qkv_f32(B, C, H, P(xd), C, P(lwd), P(lbd), nm.EPS, P(wd), C, P(qkv), 3 * C, P(ln), Tmax, P(kc), P(vc),
                                   stream()), "cg_decode_qkv_f32")
        return qkv.cpu(), kc.cpu(), vc.cpu()

    qkv, kc, vc = run(W)
    for name, cache, off in (("k", kc, C), ("v", vc, 2 * C)):
        ck.same("cg_decode_qkv_f32", f"{name} cache row {pos}", cache[:, :, pos], qkv[:, off:off + C].reshape(B, H, Dh))
        rest = torch.cat([cache[:, :, :pos], cache[:, :, pos + 1:]], 2)
        ck.require(bool(torch.isnan(rest).all()), f"cg_decode_qkv_f32 wrote {name} cache rows other than {pos}")
    if profile == "scaling":
        for k in (-24, 24):
            q2, kc2, vc2 = run(W * 2.0 ** k)
            ck.scaling("cg_decode_qkv_f32", f"({B}, {C}, {H}) qkv in W", qkv, q2, k)
            ck.scaling("cg_decode_qkv_f32", f"({B}, {C}, {H}) k cache row in W", kc[:, :, pos], kc2[:, :, pos], k)
    else:
        ref, S = nm.linear_ln_budget(x, lw, lb, W)
        ck.budget("cg_decode_qkv_f32", (B, C, H), profile, "qkv", qkv, ref, S, U32, nm.linear_ln_rho_plain(x, lw, lb, W, ref, S))
    ck.done()


@pytest.mark.parametrize("profile", ["hard", "scaling"])
@pytest.mark.parametrize("ln", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("M", [33, 2050])
def test_ffn_fwd_f32(M, ln, profile):
    """cg_ffn_fwd_f32 at C 126, H 504: with the LayerNorm on offset and flat rows, without it on outlier
    operands; "scaling": linear in (W2, b2, resid)."""
    C, Hh = 126, 504
    assert lib().cg_ffn_fwd_f32_supported(M, C, Hh)
    ck = Checks("inference rows")
    for prof in (("unit",) if profile == "scaling" else (("offset", "flat") if ln else ("outlier",))):
        g = gen(590 + M)
        if ln:
            a = nm.ln_rows(g, M, C, prof)
            W1 = torch.randn(Hh, C, generator=g) / C ** 0.5
            lw, lb = nm.ln_params(g, C)
        else:
            a, W1, _ = nm.gemm_operands(g, M, Hh, C, prof, F32)
            lw = lb = None
        b1, b2 = torch.randn(Hh, generator=g), torch.randn(C, generator=g)
        W2, resid = torch.randn(C, Hh, generator=g) / Hh ** 0.5, torch.randn(M, C, generator=g)

        def run(f=1.0):
            ad, lwd, lbd, w1d, b1d, w2d, b2d, rd = (D(t) for t in (a, lw, lb, W1, b1, W2 * f, b2 * f, resid * f))
            out = torch.full((M, C), NAN, device=DEV)
            ok(lib().cg_ffn_fwd_f32(M, C, Hh, P(ad), C, P(lwd), P(lbd), nm.EPS, P(w1d), C, P(b1d), P(w2d), Hh, P(b2d), P(rd), C, P(out),
                                    C, stream()), "cg_ffn_fwd_f32")
            return out.cpu()

        got = run()
        shape = f"({M}, {C}, {Hh}) ln {int(ln)}"
        if profile == "scaling":
            for k in (-24, 24):
                ck.scaling("cg_ffn_fwd_f32", f"{shape} in (W2, b2, resid)", got, run(2.0 ** k), k)
        else:
            ref, S = nm.ffn_budget(a, lw, lb, W1, b1, W2, b2, resid)
            ck.budget("cg_ffn_fwd_f32", shape, prof, "out", got, ref, S, U32, nm.ffn_rho_plain(a, lw, lb, W1, b1, W2, b2, resid, ref, S))
    ck.done()


# ==== the record ==============================================================================================
def test_every_family_saw_a_hard_profile_and_a_scaling_case():
    """Run last (pytest keeps the file's order): each kernel family has at least one budget case on a
    non-unit profile and one exact-scaling case (a family in NONLINEAR: one bit-equality case)."""
    missing = []
    for fam in FAMILIES:
        if not SEEN[fam]["profiles"] - {"unit"}:
            missing.append(f"{fam}: no budget case on a non-unit profile")
        if fam in NONLINEAR:
            if SEEN[fam]["same"] == 0:
                missing.append(f"{fam}: no bit-equality case")
        elif SEEN[fam]["scaling"] == 0:
            missing.append(f"{fam}: no exact-scaling case")
    assert not missing, "\n".join(missing)


def test_write_numerics_report():
    """Writes the table of every budget case (kernel, shape, profile, output, rho_plain, rho_kernel, cap)
    and the scaling summary to the path in CHARPT_NUMERICS_REPORT, if set.  The numbers are measured."""
    lines = ["family | kernel | shape | profile | output | rho_plain | rho_kernel | cap"]
    for fam, kernel, shape, profile, output, rp, rk, cap in RECORDS:
        lines.append(f"{fam} | {kernel} | {shape} | {profile} | {output} | {rp:.4g} | {rk:.4g} | {'-' if cap is None else f'{cap:.4g}'}")
    lines.append("")
    lines.append("largest rho_kernel / rho_plain per family (cases with rho_plain > 0):")
    for fam in FAMILIES:
        rs = [(rk / rp, kernel, shape, profile, output) for f, kernel, shape, profile, output, rp, rk, _ in RECORDS if f == fam and rp > 0]
        if rs:
            worst = max(rs)
            lines.append(f"  {fam}: {worst[0]:.3g} ({worst[1]} {worst[2]} {worst[3]} {worst[4]}); {len(rs)} cases")
    lines.append("")
    lines.append("exact scaling: family | kernel | cases | bitwise | differing")
    agg = {}
    for fam, kernel, what, k, res in SCALINGS:
        a = agg.setdefault((fam, kernel), [0, 0, []])
        a[0] += 1
        if res == "bitwise":
            a[1] += 1
        else:
            a[2].append(f"{what} x 2^{k}")
    for (fam, kernel), (n, okc, diff) in agg.items():
        lines.append(f"  {fam} | {kernel} | {n} | {okc} | {'; '.join(diff) if diff else '-'}")
    lines.append("")
    lines.append(f"{len(RECORDS)} budget cases, {len(SCALINGS)} scaling cases")
    path = os.environ.get("CHARPT_NUMERICS_REPORT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(f"\nnumerics: {len(RECORDS)} budget cases, {len(SCALINGS)} scaling cases")
