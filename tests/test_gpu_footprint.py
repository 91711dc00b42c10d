"""The memory-footprint contract of the C ABI (include/charpt.h, "memory footprint"), per entry point, on
the MI355X: every operand lives in a tests/footprint.py Box -- a poisoned allocation with guard bands
and a padded row stride -- and every workspace in a WsBox of exactly the bytes the library's own
*_workspace() asked for.  Each case runs in up to three layouts

    T  tight: ld == width, 16-B aligned
    P  padded, fast-path legal: bf16 strides + multiples of 8, fp32 strides + multiples of 4, every
       stride of one call different from the others
    O  odd: strides + 1, + 3, ... and the base one element off 16-B alignment -- where the header allows
       any stride or promises a fallback; where it requires alignment the case asserts CG_EINVAL, its
       message, and that no byte of any output changed

and asserts (1) the result against the fp64 reference of the logical inputs at the bar the op's
existing tight test uses, (2) layout P's bits == layout T's, (3) nothing written outside the owned
elements of outputs, in/out operands and workspaces, (4) const operands bitwise untouched, (5) the
same output bits whether workspaces and outputs held NaN or zeros on entry.

The calls go through the C ABI (replicatinggpt_amd._lib), as test_gpu_library.py does: the refusals
are asserted on the return code, which the ops wrappers turn into an exception.
tests/test_cpu_footprint.py holds the positive controls that show these checks can fail.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import bf16_close
from footprint import Box, WsBox
from oracle import philox

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, I64, I32 = torch.float32, torch.bfloat16, torch.int64, torch.int32
CG_EINVAL = 1

RAN_P = {}       # entry point -> layout-P cases that ran its kernel (the last test counts them)
REFUSALS = []    # (case, message): every asserted CG_EINVAL
FELL_BACK = []   # (case, reason): cases that keep check 1 only in place of check 2
CASES = [0]
# stride-taking entry points this file leaves to other files.  The three samplers: test_gpu_decode.py /
# test_gpu_sampling.py / test_gpu_complete.py run them on padded rows with 50.0 planted past V and assert
# that no other column is written.  cg_decode_prefill_attn and cg_decode_logprob_rows have their Box tests
# (guard bands, const snapshots, NaN against zero prefill) in test_gpu_prefill.py, and the three
# segment-masked attention calls (stride_* arguments too) in test_gpu_packed_footprint.py, which keeps its
# own count of padded runs.
ELSEWHERE = {"cg_decode_sample", "cg_decode_sample_filtered", "cg_decode_emit", "cg_decode_prefill_attn",
             "cg_decode_logprob_rows", "cg_attn_fwd_seg", "cg_attn_fwd_seg_premasked", "cg_attn_bwd_seg"}
MOVED_HERE = {"cg_linear_rows_f32", "cg_ffn_fwd_f32", "cg_decode_qkv_f32", "cg_decode_window", "cg_decode_embed",
              "cg_decode_kv_append", "cg_decode_attn"}


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


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def P(box, col=0):
    """Device pointer of a Box's logical origin (+ col elements), None for no operand."""
    if box is None:
        return None
    return ctypes.c_void_p(box.view.data_ptr() + col * box.view.element_size())


def P_t(t):
    """Device pointer of a plain tensor (scalars the kernels read: counters, steps, scales)."""
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return L().stream_ptr()


def dev_i64(v):
    return torch.tensor([v], dtype=I64, device=DEV)


def pad(lay, dtype, i):
    """Extra row stride of a call's i-th operand (i >= 1, different i: different strides)."""
    if lay == "T":
        return 0
    if lay == "P":
        return (8 if dtype == BF16 else 4) * i
    return 2 * i - 1


def off(lay, dtype):
    """O: the base one element off alignment."""
    return torch.empty((), dtype=dtype).element_size() if lay == "O" else 0


def box(rows, cols, dtype, lay="T", i=0, **kw):
    return Box(rows, cols, dtype, ld=cols + (pad(lay, dtype, i) if i else 0), offset_bytes=off(lay, dtype),
               device=DEV, **kw)


def vec(n, dtype, lay="T", **kw):
    return Box(1, n, dtype, offset_bytes=off(lay, dtype), device=DEV, **kw)


class Call:
    """One library call (or short sequence) on Boxes: const inputs, outputs (written, not accumulated),
    in/out operands with their initial value, exact-size workspaces, the launch and the result check."""

    def __init__(self, name):
        self.name = name
        self.const, self.out, self.inout, self.ws_bytes = {}, {}, {}, []
        self.launch = self.verify = self.keep = None

    def cin(self, name, b, data):
        self.const[name] = b.fill(data.to(DEV)).snapshot()
        return b

    def cout(self, name, b):
        self.out[name] = b
        return b

    def cio(self, name, b, init):
        self.inout[name] = (b, init.to(DEV))
        return b

    def written(self):
        return list(self.out.items()) + [(n, b) for n, (b, _) in self.inout.items()]


def sync(what):
    """Wait for the device; a HIP error ends the whole session (nothing more runs on a faulted device)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error after {what}: {e}", returncode=3)


def _ws_ptr(w):
    return P(w) if w.nbytes else None


def execute(c, fill):
    """One run with workspaces and outputs holding `fill` on entry: checks 3 and 4; returns the bits."""
    for b in c.out.values():
        b.prefill(fill)
    for b, init in c.inout.values():
        b.fill(init)
    ws = [WsBox(n, fill, DEV) for n in c.ws_bytes]
    rc = c.launch(*ws)
    sync(c.name)
    assert rc == 0, f"{c.name}: code {rc}: {lib().cg_last_error_string().decode(errors='replace')}"
    for name, b in c.written():
        b.assert_clean(f"{c.name} {name}")
    for i, w in enumerate(ws):
        w.assert_clean(f"{c.name} workspace {i} ({w.nbytes} bytes)")
    for name, b in c.const.items():
        b.assert_unchanged(f"{c.name} {name}")
    return {name: b.bits() for name, b in c.written()}


def same_bits(a, b, what):
    for name in a:
        if not torch.equal(a[name], b[name]):
            w = (a[name] != b[name]).nonzero()
            raise AssertionError(f"{what}: {name} differs in {w.shape[0]} element(s), first at (row {int(w[0][0])}, "
                                 f"col {int(w[0][1])})")


def footprint(entry, make, layouts=("T", "P"), fallback=None):
    """Checks 1-5 of make(layout) for every layout.  entry: the entry point(s) a layout-P run counts
    for.  fallback: the reason layout P's bits may differ from layout T's (check 1 only, recorded)."""
    bits = {}
    for lay in layouts:
        c = make(lay)
        got = execute(c, "nan")
        c.verify(c)
        same_bits(got, execute(c, "zero"), f"{c.name}: NaN against zero prefill")
        bits[lay] = got
        CASES[0] += 1
        if lay == "P":
            for e in ([entry] if isinstance(entry, str) else entry):
                RAN_P[e] = RAN_P.get(e, 0) + 1
    if "T" in bits and "P" in bits:
        if fallback:
            FELL_BACK.append((str(entry), fallback))
        else:
            same_bits(bits["T"], bits["P"], f"{entry}: layout T against layout P")
    return bits


def refused(c, match):
    """The call must fail with CG_EINVAL and a message, leaving every output byte as it was."""
    for b in c.out.values():
        b.prefill("nan").snapshot()
    for b, init in c.inout.values():
        b.fill(init).snapshot()
    ws = [WsBox(n, "nan", DEV).snapshot() for n in c.ws_bytes]
    rc = c.launch(*ws)
    sync(c.name)
    msg = lib().cg_last_error_string().decode(errors="replace")
    assert rc == CG_EINVAL and re.search(match, msg), f"{c.name}: expected CG_EINVAL /{match}/, got code {rc}: {msg}"
    for name, b in c.written():
        b.assert_unchanged(f"{c.name} (refused) {name}")
    for w in ws:
        w.assert_unchanged(f"{c.name} (refused) workspace")
    REFUSALS.append((c.name, msg))
    CASES[0] += 1


def tuning(key, value):
    return lib().cg_set_tuning(key.encode(), value)


def keep_mask(seed, call, site, n, p):
    return torch.from_numpy(philox.keep_mask(seed, (call << 8) | site, np.arange(n, dtype=np.uint64), p))


def f32(x):
    return float(np.float32(x))


# ---- cg_gemm ------------------------------------------------------------------------------------------
def _ref_gemm(A, B, at, bt):
    a = A.double().t() if at else A.double()
    b = B.double().t() if bt else B.double()
    return a @ b.t()


def pack_bits(nz):
    """[M, N] bool -> [M, N / 32] int32 words, bit n % 32 of word n / 32."""
    M, N = nz.shape
    w = (nz.view(M, N // 32, 32).long() << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(I32)


def make_gemm(lay, dt, M, N, K, at, bt, kind, c_dt=F32, beta=0.0, split=1, aux=None, colpart=False, p=0.0, flags=0,
              ldc_extra=None, rowdot_T=0, seed=1, pk128=False):
    """cg_gemm on Boxes.  aux: None, "bf16" / "f32" (RELU_BWD input), "bits_out" (BIAS_RELU writes
    CG_BITS), "bits_in" (RELU_BWD reads them), "o" (STORE_ROWDOT's attention output)."""
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn((K, M) if at else (M, K), generator=g) * 0.5).to(dt)
    B = (torch.randn((K, N) if bt else (N, K), generator=g) * 0.5).to(dt)
    bias = torch.randn(N, generator=g) if kind in (1, 2, 3, 4) else None
    resid = torch.randn(M, N, generator=g) if kind in (3, 4) else None
    init = torch.randn(M, N, generator=g).to(c_dt)
    c = Call(f"cg_gemm[{lay} {str(dt)[6:]}->{str(c_dt)[6:]} {M}x{N}x{K} {'T' if at else 'N'}{'T' if bt else 'N'} "
             f"kind {kind} aux {aux} beta {beta} split {split} flags {flags} colpart {int(colpart)} p {p}]")
    a = c.cin("A", box(*A.shape, dt, lay, 1), A)
    b = c.cin("B", box(*B.shape, dt, lay, 2), B)
    # C: + 8 in layout P (the bf16 kernels need ldc % 8 == 0 whatever the output type)
    ldc = N + (ldc_extra if ldc_extra is not None else {"T": 0, "P": 8, "O": 5}[lay])
    C = Box(M, N, c_dt, ld=ldc, offset_bytes=off(lay, c_dt), device=DEV)
    if beta:
        c.cio("C", C, init)
    else:
        c.cout("C", C)
    bb = c.cin("bias", vec(N, F32, lay), bias) if bias is not None else None
    rr = c.cin("resid", box(M, N, F32, lay, 1 if lay == "P" else 4), resid) if resid is not None else None
    acc = _ref_gemm(A, B, at, bt)
    ax, aux_code, cp, mask = None, 0, None, None
    if aux in ("bf16", "f32"):
        adt = BF16 if aux == "bf16" else F32
        h = torch.randn(M, N, generator=g).to(adt)
        ax = c.cin("aux", box(M, N, adt, lay, 3 if lay == "P" else 5), h)
        aux_code, mask = L().dtype_code(adt), h.double() > 0
    elif aux == "bits_in":
        mask = torch.rand(M, N, generator=g) < 0.5
        ax = c.cin("aux", Box(M, N // 32, I32, ld=N // 32 + {"T": 0, "P": 4, "O": 1}[lay], device=DEV, pad=0),
                   pack_bits(mask))
        aux_code = L().CG_BITS
    elif aux == "bits_out":
        ax = c.cout("aux", Box(M, N // 32, I32, ld=N // 32 + {"T": 0, "P": 4, "O": 1}[lay], device=DEV))
        aux_code = L().CG_BITS
    elif aux == "o":
        h = torch.randn(M, N, generator=g).to(BF16)
        ax = c.cin("aux", box(M, N, BF16, lay, 3), h)
        aux_code = L().CG_BF16
        cp = c.cout("delta", vec(M * (N // 64), F32, lay))
    if colpart:
        cp = c.cout("colpart", box(M // 64, N, F32))
    call = c.keep = dev_i64(6)      # the epilogue holds its address: alive as long as the case
    c.ws_bytes = [lib().cg_gemm_workspace(M, N, split)]
    ld_r = rowdot_T if kind == 7 else (rr.ld if rr is not None else 0)
    epi = L().Epilogue(kind, P(bb), P(rr), ld_r, P(ax), aux_code, ax.ld if ax is not None else 0, p, 99, P_t(call), 3,
                       beta, P(cp), flags)

    def launch(ws):
        return lib().cg_gemm(L().dtype_code(dt), at, bt, M, N, K, P(a), a.ld, P(b), b.ld, P(C), L().dtype_code(c_dt),
                             ldc, epi, split, _ws_ptr(ws), stream())

    def verify(c_):
        want = acc
        if kind in (1, 2, 3, 4):
            want = want + bias.double()
        if kind == 2:
            want = torch.relu(want)
        if kind == 4:
            want = keep_mask(99, 6, 3, M * N, p).reshape(M, N).double() * want * f32(1 / (1 - p))
        if kind in (3, 4):
            want = want + resid.double()
        if kind == 5:
            want = want * mask
        want = want + beta * init.double()
        got = C.view
        if flags & L().GEMM_SLAB_BF16 and split > 1 and ldc == N and pk128:
            assert relerr(got, want) < 2 ** -8, c_.name     # test_gemm_bf16_slabs: each partial rounded once to bf16
        elif c_dt == F32:
            assert relerr(got, want) < 1e-5, (c_.name, relerr(got, want))
        elif kind in (2, 5):
            assert relerr(got, want) < 8e-3, (c_.name, relerr(got, want))
        else:
            ok, st = bf16_close(got, want)
            assert ok, (c_.name, st)
        if aux == "bits_out":
            nz = (C.view.cpu().view(torch.int16) & 0x7FFF) != 0
            assert torch.equal(ax.view.cpu(), pack_bits(nz)), c_.name
        if colpart:      # the column sums of each 64-row block of the bf16 values written
            blocks = C.view.double().cpu().view(M // 64, 64, N).sum(1)
            assert relerr(cp.view, blocks) < 1e-5, c_.name
        if kind == 7:    # delta[(m / T) * (N / 64) + n / 64][m % T] = rowsum over the head of bf16(acc) * o
            T = rowdot_T
            exp = (C.view.double().cpu() * h.double()).view(M // T, T, N // 64, 64).sum(-1).permute(0, 2, 1)
            err = float((cp.view.double().cpu().view(M // T, N // 64, T) - exp).abs().max())
            assert err <= 1e-5 * max(1.0, float(exp.abs().max())), (c_.name, err)

    c.launch, c.verify = launch, verify
    return c


# name -> make_gemm keywords
FAST_EPILOGUES = {
    "store_f32": dict(kind=0),
    "store_f32_beta1": dict(kind=0, beta=1.0),
    "store_bf16": dict(kind=0, c_dt=BF16),
    "store_bf16_beta1": dict(kind=0, c_dt=BF16, beta=1.0),
    "bias_relu": dict(kind=2, c_dt=BF16),
    "bias_relu_bits": dict(kind=2, c_dt=BF16, aux="bits_out"),
    "relu_bwd_bf16": dict(kind=5, c_dt=BF16, aux="bf16"),
    "relu_bwd_bits": dict(kind=5, c_dt=BF16, aux="bits_in"),
    "relu_bwd_bits_colpart": dict(kind=5, c_dt=BF16, aux="bits_in", colpart=True),
    "relu_bwd_bf16_colpart": dict(kind=5, c_dt=BF16, aux="bf16", colpart=True),
    "bias_resid": dict(kind=3),
    "bias_drop_resid": dict(kind=4, p=0.2),
    "store_rowdot": dict(kind=7, c_dt=BF16, aux="o", rowdot_T=64),
    "split3_vec": dict(kind=0, split=3),
    "split3_bf16_slabs": dict(kind=0, split=3, flags=1),
}


def _special_form(kw):
    """The (a_trans, b_trans) form the header names for the keep-bit, column-partial and row-dot
    epilogues (non-transposed A; bits written NN by the W1 forward, read NT by the W2 dgrad; column
    partials and row dots NT), None for the plain epilogues."""
    if kw.get("aux") == "bits_out":
        return (0, 0)
    if kw.get("aux") in ("bits_in", "o") or kw.get("colpart"):
        return (0, 1)
    return None


def _fast_params():
    out = []
    for variant in (2, 9, 24):
        for name, kw in FAST_EPILOGUES.items():
            form = _special_form(kw)
            # special epilogues: their form, and the same with A transposed (a refusal by the header)
            for at, bt in ([(0, 0), (0, 1), (1, 0), (1, 1)] if form is None else [form, (1, form[1])]):
                out.append((variant, at, bt, name))
    return out


@pytest.mark.parametrize("variant,at,bt,name", _fast_params())
def test_gemm_bf16_fast_kernels(variant, at, bt, name):
    """The bf16 MFMA kernels (register-staged 2, persistent 128x128 9, 8-wave 256x256 24) at the smallest
    shape that reaches them: (256, 384, 192), and (256, 512, 192) for variant 24, whose tile needs
    N % 256 == 0 (gemm_p8.hip p8_gemm_launch).  The library's own predicates say whether the dispatch
    under this variant takes a keep-bit / column-partial / row-dot epilogue; where they say no the
    refusal is asserted."""
    kw = dict(FAST_EPILOGUES[name], pk128=variant == 9)
    M, N, K = (256, 512, 192) if variant == 24 else (256, 384, 192)
    if tuning("gemm_variant", variant) != 0:
        pytest.skip(f"gemm_variant {variant} is A/B-only (not in this library build)")
    try:
        if _special_form(kw) is not None:
            pred = {"o": lib().cg_gemm_rowdot_supported, "bits_in": lib().cg_gemm_relu_bits_supported,
                    "bits_out": lib().cg_gemm_relu_bits_supported, "bf16": lib().cg_gemm_colpart_supported}[kw["aux"]]
            if not pred(at, bt, M, N, K, K + 8, K + 16, N + 8):
                refused(make_gemm("T", BF16, M, N, K, at, bt, **kw), "cg_gemm: ")
                return
        fallback = None
        if name == "split3_bf16_slabs" and variant == 9:
            fallback = ("gemm.hip cg_gemm: e.slab_bf16 needs ldc == N, so layout P (ldc = N + 8) sums fp32 slabs "
                        "where layout T sums bf16 ones")
        footprint("cg_gemm", lambda lay: make_gemm(lay, BF16, M, N, K, at, bt, **kw), fallback=fallback)
        if kw.get("aux") in ("bits_in", "bits_out"):     # odd strides, odd word stride: no generic kernel has keep bits
            refused(make_gemm("O", BF16, M, N, K, at, bt, **kw), "cg_gemm: CG_BITS ReLU keep bits need")
    finally:
        tuning("gemm_variant", 0)


@pytest.mark.parametrize("c_dt", [F32, BF16])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_gemm_splitk_reduce_paths(c_dt, beta):
    """Split-K 3 with ldc == N (vector reduce), ldc = N + 8 (vector rows, padded) and ldc = N + 1 (the
    generic kernel and the scalar reduce: gemm_bf16.hip fast_shape_ok wants ldc % 8 == 0): all within
    fp64's bar; the product kernel differs between ldc % 8 == 0 and not, so no bitwise claim there."""
    M, N, K = 256, 384, 192
    res = {}
    for extra in (0, 8, 1):
        for at, bt in ((0, 0), (1, 1)):
            def make(lay, extra=extra, at=at, bt=bt):
                return make_gemm(lay, BF16, M, N, K, at, bt, kind=1, c_dt=c_dt, beta=beta, split=3, ldc_extra=extra)
            res[extra, at] = footprint("cg_gemm", make, layouts=("P",))["P"]
    for at in (0, 1):
        same_bits(res[0, at], res[8, at], "split-K 3: ldc == N against ldc == N + 8")
    FELL_BACK.append(("cg_gemm split 3 ldc = N + 1", "gemm_bf16.hip fast_shape_ok: ldc % 8 != 0 takes the generic "
                      "kernel, another K order than the 128x128 tiles of ldc == N"))


@pytest.mark.parametrize("at,bt", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(37, 65, 126), (96, 70, 40)])
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
def test_gemm_generic_and_f32_kernels(kind, dt, M, N, K, at, bt):
    """The generic kernel (bf16 at shapes the MFMA tiles do not divide) and the fp32 kernels at odd
    sizes, layouts P and O (cg_gemm takes any stride and alignment: its vector paths fall back)."""
    kw = dict(kind=kind)
    if kind in (2, 5):
        kw["c_dt"] = dt
    if kind == 5:
        kw["aux"] = "bf16" if dt == BF16 else "f32"
    if kind == 4:
        kw["p"] = 0.2
    footprint("cg_gemm", lambda lay: make_gemm(lay, dt, M, N, K, at, bt, **kw), layouts=("P", "O"))


@pytest.mark.parametrize("M,N,K,split", [(126, 504, 1000, 4), (1, 504, 126, 1)])
@pytest.mark.parametrize("at,bt", [(0, 0), (1, 1)])
def test_gemm_f32_splitk_and_small_m(M, N, K, split, at, bt):
    """fp32 split-K 4 and the small-M chunked kernel (M = 1)."""
    footprint("cg_gemm", lambda lay: make_gemm(lay, F32, M, N, K, at, bt, kind=1, split=split), layouts=("T", "P", "O"))


# ---- cg_gemm_wgrad_group -----------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_gemm_wgrad_group(flags, beta):
    """Two weight gradients, (128, 256, 1024) and (256, 128, 1024) at split 4, as one launch: each C has
    the bits of its own cg_gemm call on the same Boxes; slab workspaces of exact size.  bf16 slabs
    apply at ldc == N only (header), so layout P with the flag runs fp32 slabs in both forms."""
    shapes = [(128, 256, 1024), (256, 128, 1024)]

    def make(lay, grouped, bad_ld=False):
        c = Call(f"cg_gemm_wgrad_group[{lay} flags {flags} beta {beta} grouped {grouped} bad ld {bad_ld}]")
        g = torch.Generator().manual_seed(5)
        ops = []
        for i, (M, N, K) in enumerate(shapes):
            A = (torch.randn(K, M, generator=g) * 0.5).to(BF16)
            B = (torch.randn(K, N, generator=g) * 0.5).to(BF16)
            init = torch.randn(M, N, generator=g)
            a = c.cin(f"A{i}", box(K, M, BF16, lay, 1 + i), A)
            b = c.cin(f"B{i}", box(K, N, BF16, lay, 3 + i), B)
            C = Box(M, N, F32, ld=N + (8 * (i + 1) if lay == "P" else 0), device=DEV)
            c.cio(f"C{i}", C, init) if beta else c.cout(f"C{i}", C)
            c.ws_bytes.append(lib().cg_gemm_workspace(M, N, 4))
            ops.append((M, N, K, a, b, C, A.double().t() @ B.double() + beta * init.double()))

        def problems(ws):
            arr = (L().WgradProblem * 2)()
            for i, (M, N, K, a, b, C, _) in enumerate(ops):
                arr[i] = L().WgradProblem(M, N, K, a.view.data_ptr(), a.ld, b.view.data_ptr(), b.ld, C.view.data_ptr(),
                                          C.ld, beta, 4, ws[i].view.data_ptr(), flags)
            if bad_ld:
                arr[0].lda += 1      # ld % 8 != 0
            return arr

        def launch(*ws):
            if grouped:
                return lib().cg_gemm_wgrad_group(problems(ws), 2, stream())
            for i, (M, N, K, a, b, C, _) in enumerate(ops):
                epi = L().Epilogue(0, None, None, 0, None, 0, 0, 0.0, 0, None, 0, beta, None, flags)
                rc = lib().cg_gemm(L().CG_BF16, 1, 1, M, N, K, P(a), a.ld, P(b), b.ld, P(C), L().CG_F32, C.ld, epi, 4,
                                   P(ws[i]), stream())
                if rc:
                    return rc
            return 0

        def verify(c_):
            for M, N, K, a, b, C, want in ops:
                bar = 2 ** -8 if flags and lay == "T" else 1e-5
                assert relerr(C.view, want) < bar, (c_.name, relerr(C.view, want))

        c.launch, c.verify, c.problems = launch, verify, problems
        return c

    for lay in ("T", "P"):
        probe = make(lay, True)
        arr = probe.problems([WsBox(n, "nan", DEV) for n in probe.ws_bytes])
        assert lib().cg_gemm_wgrad_group_supported(arr, 2) == 1, lay
    fallback = ("gemm.hip cg_gemm / plan_group_problem: CG_GEMM_SLAB_BF16 applies at ldc == N only, so layout P sums "
                "fp32 slabs where layout T sums bf16 ones") if flags else None
    one = footprint("cg_gemm", lambda lay: make(lay, False), fallback=fallback)
    grp = footprint("cg_gemm_wgrad_group", lambda lay: make(lay, True), fallback=fallback)
    for lay in ("T", "P"):
        same_bits(one[lay], grp[lay], f"cg_gemm_wgrad_group against cg_gemm, layout {lay}")
    # ld % 8 != 0: the group refuses, nothing written
    c = make("T", True, bad_ld=True)
    assert lib().cg_gemm_wgrad_group_supported(c.problems([WsBox(n, "nan", DEV) for n in c.ws_bytes]), 2) == 0
    refused(c, "cg_gemm_wgrad_group: unsupported group")


# ---- cg_gemm_resid_layernorm ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(64, 64), (192, 640)])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("inplace", [False, True])
def test_gemm_resid_layernorm(M, K, p, inplace):
    """out = resid + [dropout](A W^T + bias) with the LayerNorm of the result: lda, ldw, ldc, ld_resid
    padded and mutually different, out over resid and not; y / mean / rstd in Boxes."""
    N = 384
    assert lib().cg_gemm_resid_layernorm_supported(M, N, K)

    def make(lay):
        g = torch.Generator().manual_seed(17)
        A = (torch.randn(M, K, generator=g) * 0.5).to(BF16)
        W = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF16)
        bias, resid = torch.randn(N, generator=g) * 0.1, torch.randn(M, N, generator=g)
        lw, lb = torch.randn(N, generator=g) * 0.1 + 1, torch.randn(N, generator=g) * 0.1
        c = Call(f"cg_gemm_resid_layernorm[{lay} M {M} K {K} p {p} inplace {inplace}]")
        a, w = c.cin("A", box(M, K, BF16, lay, 1), A), c.cin("W", box(N, K, BF16, lay, 2), W)
        bb, lwb, lbb = c.cin("bias", vec(N, F32), bias), c.cin("ln_w", vec(N, F32), lw), c.cin("ln_b", vec(N, F32), lb)
        if inplace:
            out = rr = c.cio("out", box(M, N, F32, lay, 3), resid)
        else:
            out, rr = c.cout("out", box(M, N, F32, lay, 3)), c.cin("resid", box(M, N, F32, lay, 1), resid)
        y, mean, rstd = c.cout("y", box(M, N, BF16)), c.cout("mean", vec(M, F32)), c.cout("rstd", vec(M, F32))
        call = c.keep = dev_i64(6)      # the epilogue holds its address: alive as long as the case
        epi = L().Epilogue(4 if p > 0 else 3, P(bb), P(rr), rr.ld, None, 0, 0, p, 41, P_t(call), 2, 0.0, None, 0)

        def launch():
            return lib().cg_gemm_resid_layernorm(M, N, K, P(a), a.ld, P(w), w.ld, P(out), out.ld, epi, P(lwb), P(lbb),
                                                 P(y), P(mean), P(rstd), 1e-5, stream())

        def verify(c_):
            acc = A.double() @ W.double().t() + bias.double()
            if p > 0:
                acc = keep_mask(41, 6, 2, M * N, p).reshape(M, N).double() * acc * f32(1 / (1 - p))
            x = resid.double() + acc
            assert relerr(out.view, x) < 1e-5, c_.name
            xg = out.view.double().cpu()       # y, mean, rstd: the LayerNorm of the fp32 out just written
            mu, var = xg.mean(1), xg.var(1, unbiased=False)
            assert relerr(mean.view[0], mu) < 1e-5 and relerr(rstd.view[0], (var + 1e-5).rsqrt()) < 1e-5, c_.name
            yr = torch.nn.functional.layer_norm(xg, (N,), lw.double(), lb.double(), 1e-5)
            assert relerr(y.view, yr) < 1e-2, c_.name     # test_layernorm's bf16 bar

        c.launch, c.verify = launch, verify
        return c

    footprint("cg_gemm_resid_layernorm", make)
    o = make("O")       # header: 16-B aligned operands, lda / ldw % 8, ldc / ld_resid % 4
    refused(o, "cg_gemm_resid_layernorm: (bad leading dimensions|operands must be 16-B aligned)")


# ---- attention --------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, scale, p, seed, call, site):
    B, T, H, D = q.shape
    s = torch.einsum("bthd,bshd->bhts", q, k) * scale
    s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
    Pm = torch.softmax(s, dim=-1)
    if p > 0:
        Pm = Pm * keep_mask(seed, call, site, B * H * T * T, p).reshape(B, H, T, T).double() * f32(1 / (1 - p))
    return torch.einsum("bhts,bshd->bthd", Pm, v)


def _close(dt, got, want, what):
    if dt == F32:
        assert relerr(got, want) < 1e-5, (what, relerr(got, want))
    else:
        ok, st = bf16_close(got, want)
        assert ok, (what, st)


ATTN_CASES = [  # dt, B, T, H, D, layouts, path
    # O: everything off 16-B alignment; V: layout T with v alone 8 bytes off (its own pointer in the ABI):
    # both must leave the MFMA path (attention.hip fast_attn_ok) for the generic kernels
    (BF16, 2, 64, 2, 64, ("T", "P", "O", "V"), "bf16 D = 64 resident"),
    (BF16, 2, 192, 2, 64, ("T", "P"), "bf16 D = 64 resident"),
    (BF16, 1, 320, 2, 64, ("T", "P"), "bf16 D = 64 ring"),
    (BF16, 2, 37, 3, 21, ("T", "P", "O"), "generic bf16"),
    (F32, 2, 37, 3, 21, ("T", "P", "O"), "fp32 resident forward (p = 0) / generic"),
    (F32, 1, 130, 4, 16, ("T", "P", "O"), "fp32 resident forward (p = 0) / generic"),
]


@pytest.mark.parametrize("dt,B,T,H,D,layouts,path", ATTN_CASES)
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_attention(dt, B, T, H, D, layouts, path, p):
    """cg_attn_fwd / cg_attn_fwd_premasked / cg_attn_bwd / cg_attn_bwd_delta: ld_qkv = 3d + 8, ld_o = d + 8,
    ld_do = d + 16, ld_dqkv = 3d + 24, the q / k / v block at a non-zero column offset of a wider
    buffer (the Box origin sits 16 elements into its row), the keep bits in a Box of exactly
    cg_attn_mask_bytes (supplied, and NULL: regenerated inside the workspace), lse and delta in Boxes."""
    d, BT = H * D, B * T
    scale = (3.0 * D) ** -0.5
    fast = dt == BF16 and D == 64 and T % 64 == 0
    g = torch.Generator().manual_seed(4)
    qkv = (torch.randn(BT, 3 * d, generator=g) * 0.7).to(dt)
    dout = torch.randn(BT, d, generator=g).to(dt)
    q, k, v = (qkv[:, i * d:(i + 1) * d].double().view(B, T, H, D).requires_grad_(True) for i in range(3))
    ref = _attn_ref(q, k, v, scale, p, 11, 2, 7)
    ref.backward(dout.double().view(B, T, H, D))
    want_o = ref.detach().reshape(BT, d)
    want_d = torch.cat([t.grad.reshape(BT, d) for t in (q, k, v)], 1)
    isz = qkv.element_size()
    call = dev_i64(2)
    mask_bytes = lib().cg_attn_mask_bytes(B, H, T) if fast and p > 0 else 0
    fwd_out = {}

    def qkv_box(c, lay):
        """The qkv Box and the three pointers (layout V: v from a Box of its own with the same stride)."""
        b = Box(BT, 3 * d, dt, ld=3 * d + (pad(lay, dt, 1) if lay != "P" else 8),
                offset_bytes=(16 * isz if lay != "O" else 17 * isz), device=DEV)
        c.cin("qkv", b, qkv)
        vp = P(b, 2 * d)
        if c.v_apart:
            vp = P(c.cin("v", Box(BT, d, dt, ld=b.ld, offset_bytes=8, device=DEV), qkv[:, 2 * d:]))
        return b, (P(b), P(b, d), vp)

    def make_fwd(lay, premasked=False):
        c = Call(f"cg_attn_fwd[{lay} {path} T {T} p {p} premasked {premasked}]")
        c.v_apart, key = lay == "V", lay
        lay = "T" if lay == "V" else lay
        mb = mask_bytes if key in ("T", "P") else 0      # the generic kernels draw their own keep decisions
        x, qkv_p = qkv_box(c, lay)
        o = c.cout("o", box(BT, d, dt, lay, 1 if lay == "P" else 2))
        lse = c.cout("lse", vec(B * H * T, F32))
        mask = c.cout("mask", WsBox(mb, "nan", DEV)) if mb else None
        fn = lib().cg_attn_fwd_premasked if premasked else lib().cg_attn_fwd

        def launch():
            if premasked and mask is not None:      # the keep bits filled ahead, as on a side stream
                rc = lib().cg_attn_dropmask(B, H, T, p, 11, P_t(call), 7, P(mask), stream())
                if rc:
                    return rc
            return fn(L().dtype_code(dt), B, T, H, D, *qkv_p, x.ld, P(o), o.ld, P(lse), scale, p, 11,
                      P_t(call), 7, P(mask), stream())

        def verify(c_):
            fwd_out[key] = (o.view.clone(), lse.view.clone(), mask.view.clone() if mask else None)
            _close(dt, o.view, want_o, c_.name)

        c.launch, c.verify = launch, verify
        return c

    def make_bwd(lay, null_mask=False, delta=False):
        c = Call(f"cg_attn_bwd[{lay} {path} T {T} p {p} null mask {null_mask} delta {delta}]")
        o_t, lse_t, mask_t = fwd_out[lay]
        c.v_apart = lay == "V"
        lay = "T" if lay == "V" else lay
        x, qkv_p = qkv_box(c, lay)
        o = c.cin("o", box(BT, d, dt, lay, 1 if lay == "P" else 2), o_t)
        do = c.cin("dout", box(BT, d, dt, lay, 2 if lay == "P" else 3), dout)
        lse = c.cin("lse", vec(B * H * T, F32), lse_t)
        mask = None
        if mask_t is not None and not null_mask:
            mask = WsBox(mask_t.numel(), "nan", DEV)
            mask.view.copy_(mask_t)
            c.const["mask"] = mask.snapshot()
        dl = None
        if delta:       # rowsum(dO * O) over each head, [B][H][T]
            dd = (dout.double() * o_t.double().cpu()).view(B, T, H, D).sum(-1).permute(0, 2, 1).reshape(-1)
            dl = c.cin("delta", vec(B * H * T, F32, lay), dd.float())
        dqkv = c.cout("dqkv", box(BT, 3 * d, dt, lay, 3 if lay == "P" else 4))
        c.ws_bytes = [lib().cg_attn_bwd_workspace(B, T, H, D)]

        def launch(ws):
            a = (L().dtype_code(dt), B, T, H, D, *qkv_p, x.ld, P(o), o.ld, P(do), do.ld, P(lse))
            z = (P(dqkv), P(dqkv, d), P(dqkv, 2 * d), dqkv.ld, scale, p, 11, P_t(call), 7, P(mask), P(ws), stream())
            return lib().cg_attn_bwd_delta(*a, P(dl), *z) if delta else lib().cg_attn_bwd(*a, *z)

        def verify(c_):
            for i, nm in enumerate("qkv"):
                _close(dt, dqkv.view[:, i * d:(i + 1) * d], want_d[:, i * d:(i + 1) * d], f"{c_.name} d{nm}")

        c.launch, c.verify = launch, verify
        return c

    f = footprint("cg_attn_fwd", make_fwd, layouts)
    fp = footprint("cg_attn_fwd_premasked", lambda lay: make_fwd(lay, True), layouts)
    b = footprint("cg_attn_bwd", make_bwd, layouts)
    footprint("cg_attn_bwd_delta", lambda lay: make_bwd(lay, delta=True), layouts)
    for lay in layouts:
        same_bits(f[lay], fp[lay], f"cg_attn_fwd_premasked against cg_attn_fwd, layout {lay}")
    if mask_bytes:
        nb = footprint("cg_attn_bwd", lambda lay: make_bwd(lay, null_mask=True), layouts)
        for lay in layouts:
            same_bits(b[lay], nb[lay], f"cg_attn_bwd: regenerated keep bits against the supplied ones, layout {lay}")


# ---- LayerNorm (rows contiguous by contract: layouts T and O-offset) ---------------------------------------
def _ln_data(rows, C, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 2 + 0.5
    w, b = torch.randn(C, generator=g) * 0.1 + 1, torch.randn(C, generator=g) * 0.1
    return g, x, w, b


@pytest.mark.parametrize("rows", [7, 1000])
@pytest.mark.parametrize("C", [126, 384])
@pytest.mark.parametrize("y_dt", [F32, BF16])
@pytest.mark.parametrize("fused_mask", [False, True])
def test_layernorm_fwd(rows, C, y_dt, fused_mask):
    """cg_layernorm_fwd and cg_layernorm_fwd_attn_dropmask (B = 1, H = 2, T = 64 keep bits beside it, in a
    Box of exactly cg_attn_mask_bytes)."""
    g, x, w, b = _ln_data(rows, C)
    B, H, T, p = 1, 2, 64, 0.2
    nmask = lib().cg_attn_mask_bytes(B, H, T)
    call = dev_i64(3)
    want = torch.nn.functional.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-5)

    def make(lay):
        c = Call(f"cg_layernorm_fwd[{lay} rows {rows} C {C} y {str(y_dt)[6:]} with keep bits {fused_mask}]")
        xb, wb, bb = c.cin("x", box(rows, C, F32, lay), x), c.cin("w", vec(C, F32, lay), w), c.cin("b", vec(C, F32, lay), b)
        y, mean, rstd = c.cout("y", box(rows, C, y_dt, lay)), c.cout("mean", vec(rows, F32, lay)), c.cout("rstd", vec(rows, F32, lay))
        mask = c.cout("mask", WsBox(nmask, "nan", DEV)) if fused_mask else None

        def launch():
            a = (P(xb), P(wb), P(bb), P(y), L().dtype_code(y_dt), P(mean), P(rstd), rows, C, 1e-5)
            if fused_mask:
                return lib().cg_layernorm_fwd_attn_dropmask(*a, B, H, T, p, 77, P_t(call), 2, P(mask), stream())
            return lib().cg_layernorm_fwd(*a, stream())

        def verify(c_):
            assert relerr(y.view, want) < (1e-5 if y_dt == F32 else 1e-2), c_.name      # test_layernorm's bars
            assert relerr(mean.view[0], x.double().mean(1)) < 1e-5, c_.name
            assert relerr(rstd.view[0], (x.double().var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5, c_.name

        c.launch, c.verify = launch, verify
        return c

    bits = footprint("cg_layernorm_fwd", make, layouts=("T", "O"))
    if fused_mask:      # the keep bits do not depend on the LayerNorm's alignment path
        assert torch.equal(bits["T"]["mask"], bits["O"]["mask"])
        m = WsBox(nmask, "nan", DEV)
        assert lib().cg_attn_dropmask(B, H, T, p, 77, P_t(call), 2, P(m), stream()) == 0
        torch.cuda.synchronize()
        m.assert_clean("cg_attn_dropmask mask")
        assert torch.equal(m.bits(), bits["T"]["mask"])


@pytest.mark.parametrize("rows", [7, 1000])
@pytest.mark.parametrize("C", [126, 384])
@pytest.mark.parametrize("form,extras,p,acc", [      # extras: d = dres, l = the bf16 copy, c = lp_colsum
    ("bwd", "", 0.0, 0), ("bwd", "dl", 0.0, 1), ("bwd", "d", 0.0, 0),      # cg_layernorm_bwd has no dropout argument
    ("ex", "", 0.0, 0), ("ex", "dlc", 0.0, 1), ("ex", "dlc", 0.2, 0), ("ex", "lc", 0.2, 1), ("ex", "l", 0.2, 0),
    ("rows_reduce", "", 0.0, 0), ("rows_reduce", "dlc", 0.0, 1), ("rows_reduce", "dl", 0.2, 0),
    ("rows_reduce", "lc", 0.2, 1)])
def test_layernorm_bwd(rows, C, form, extras, p, acc):
    """cg_layernorm_bwd (dx_bf16 copy), cg_layernorm_bwd_ex (consumer copy with dropout and its column
    sums) and cg_layernorm_bwd_rows + cg_layernorm_bwd_reduce, with and without dres, the bf16 copy and
    (ex forms) lp_colsum; the workspace has exactly cg_layernorm_bwd_workspace bytes."""
    g, x, w, _ = _ln_data(rows, C)
    mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()
    dy = torch.randn(rows, C, generator=g).to(BF16)
    dres = torch.randn(rows, C, generator=g) if "d" in extras else None
    call = dev_i64(9)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xr, (C,), wr, br, 1e-5).backward(dy.double())
    want_dx = xr.grad + (dres.double() if "d" in extras else 0)
    colsum = "c" in extras

    def make(lay):
        c = Call(f"cg_layernorm_{form}[{lay} rows {rows} C {C} extras {extras} p {p} accumulate {acc}]")
        dyb, xb, wb = c.cin("dy", box(rows, C, BF16, lay), dy), c.cin("x", box(rows, C, F32, lay), x), c.cin("w", vec(C, F32, lay), w)
        mb, rb = c.cin("mean", vec(rows, F32, lay), mean), c.cin("rstd", vec(rows, F32, lay), rstd)
        db_ = c.cin("dres", box(rows, C, F32, lay), dres) if "d" in extras else None
        dx = c.cout("dx", box(rows, C, F32, lay))
        lp = c.cout("lp", box(rows, C, BF16, lay)) if "l" in extras else None
        one = torch.ones(C)
        red = {}
        for nm in ("dw", "db") + (("cs",) if colsum else ()):
            red[nm] = c.cio(nm, vec(C, F32, lay), one) if acc else c.cout(nm, vec(C, F32, lay))
        c.ws_bytes = [lib().cg_layernorm_bwd_workspace(rows, C)]
        head = (P(dyb), L().CG_BF16, P(xb), P(wb), P(mb), P(rb), P(db_), P(dx), P(lp))
        rng = (p, 11, P_t(call) if p else None, 4)

        def launch(ws):
            if form == "bwd":
                return lib().cg_layernorm_bwd(*head, P(red["dw"]), P(red["db"]), acc, P(ws), rows, C, stream())
            if form == "ex":
                return lib().cg_layernorm_bwd_ex(*head, *rng, P(red["dw"]), P(red["db"]), P(red.get("cs")), acc, acc,
                                                 P(ws), rows, C, stream())
            rc = lib().cg_layernorm_bwd_rows(*head, *rng, int(colsum), P(ws), rows, C, stream())
            return rc or lib().cg_layernorm_bwd_reduce(P(ws), rows, C, int(colsum), P(red["dw"]), P(red["db"]),
                                                       P(red.get("cs")), acc, acc, stream())

        def verify(c_):
            assert relerr(dx.view, want_dx) < 1e-5, c_.name
            assert relerr(red["dw"].view[0], wr.grad + acc) < 1e-5 and relerr(red["db"].view[0], br.grad + acc) < 1e-5, c_.name
            if "l" in extras:      # test_layernorm_bwd_link_dropout_matches_oracle: the copy of the dx just written
                keep = keep_mask(11, 9, 4, rows * C, p).reshape(rows, C).float() if p else torch.ones(rows, C)
                t = dx.view.cpu() * keep * (1.0 / (1.0 - p))
                assert torch.equal(lp.view.cpu(), t.to(BF16)), c_.name
                if colsum:
                    assert relerr(red["cs"].view[0], t.double().sum(0) + acc) < 1e-5, c_.name

        c.launch, c.verify = launch, verify
        return c

    footprint(f"cg_layernorm_{form}", make, layouts=("T", "O"))


# ---- column and row reductions ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("rows", [33, 1024])
@pytest.mark.parametrize("N", [70, 384])
@pytest.mark.parametrize("acc", [0, 1])
def test_colsum(dt, rows, N, acc):
    g = torch.Generator().manual_seed(2)
    X, init = torch.randn(rows, N, generator=g).to(dt), torch.randn(N, generator=g)

    def make(lay):
        c = Call(f"cg_colsum[{lay} {str(dt)[6:]} rows {rows} N {N} accumulate {acc}]")
        xb = c.cin("X", box(rows, N, dt, lay, 1), X)
        out = c.cio("out", vec(N, F32, lay), init) if acc else c.cout("out", vec(N, F32, lay))
        c.ws_bytes = [lib().cg_colsum_workspace(rows, N)]
        c.launch = lambda ws: lib().cg_colsum(P(xb), L().dtype_code(dt), rows, N, xb.ld, P(out), acc, _ws_ptr(ws), stream())
        c.verify = lambda c_: _assert(relerr(out.view[0], X.double().sum(0) + acc * init.double()) < 1e-5, c_.name)
        return c

    footprint("cg_colsum", make, layouts=("T", "P", "O"))


def _assert(ok, what):
    assert ok, what


@pytest.mark.parametrize("rows,N", [(33, 70), (4, 384), (33, 4099)])
@pytest.mark.parametrize("acc", [0, 1])
def test_reduce_rows(rows, N, acc):
    g = torch.Generator().manual_seed(2)
    part, init = torch.randn(rows, N, generator=g), torch.randn(N, generator=g)

    def make(lay):
        c = Call(f"cg_reduce_rows[{lay} rows {rows} N {N} accumulate {acc}]")
        pb = c.cin("part", box(rows, N, F32, lay), part)
        out = c.cio("out", vec(N, F32, lay), init) if acc else c.cout("out", vec(N, F32, lay))
        c.launch = lambda: lib().cg_reduce_rows(P(pb), rows, N, P(out), acc, stream())
        c.verify = lambda c_: _assert(relerr(out.view[0], part.double().sum(0) + acc * init.double()) < 1e-5, c_.name)
        return c

    footprint("cg_reduce_rows", make, layouts=("T", "O"))


@pytest.mark.parametrize("y_dt", [F32, BF16])
@pytest.mark.parametrize("rows,C", [(33, 70), (1024, 384)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_dropout_apply(y_dt, rows, C, p):
    """y[r, c] = x[r, c] keep(r C + c) / (1 - p): the element index is the logical one, not the address."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(rows, C, generator=g)
    call = dev_i64(5)
    keep = keep_mask(31, 5, 6, rows * C, p).reshape(rows, C).double() if p else torch.ones(rows, C).double()
    want = x.double() * keep * f32(1 / (1 - p))

    def make(lay):
        c = Call(f"cg_dropout_apply[{lay} y {str(y_dt)[6:]} rows {rows} C {C} p {p}]")
        xb, y = c.cin("x", box(rows, C, F32, lay, 1), x), c.cout("y", box(rows, C, y_dt, lay))
        c.launch = lambda: lib().cg_dropout_apply(P(xb), rows, C, xb.ld, P(y), L().dtype_code(y_dt), p, 31, P_t(call), 6,
                                                  stream())
        c.verify = lambda c_: _close(y_dt, y.view, want, c_.name)
        return c

    footprint("cg_dropout_apply", make, layouts=("T", "P", "O"))


@pytest.mark.parametrize("n", [1, 1023, 4096 + 3])
def test_sum_and_cast(n):
    """cg_sum_f32 (workspace of exactly 1024 floats) and cg_cast_f32_bf16 (x 16-B, y 8-B aligned by
    its check: the off-by-one-element layout is refused)."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, generator=g)

    def make_sum(lay):
        c = Call(f"cg_sum_f32[{lay} n {n}]")
        xb, out = c.cin("x", vec(n, F32, lay), x), c.cout("out", vec(1, F32, lay))
        c.ws_bytes = [1024 * 4]
        c.launch = lambda ws: lib().cg_sum_f32(P(xb), n, 0.5, P(out), P(ws), stream())
        c.verify = lambda c_: _assert(abs(float(out.view[0, 0]) - 0.5 * float(x.double().sum())) <
                                      1e-5 * max(1.0, float(x.double().abs().sum())), c_.name)
        return c

    def make_cast(lay):
        c = Call(f"cg_cast_f32_bf16[{lay} n {n}]")
        xb, y = c.cin("x", vec(n, F32, lay), x), c.cout("y", vec(n, BF16, lay))
        c.launch = lambda: lib().cg_cast_f32_bf16(P(xb), P(y), n, stream())
        c.verify = lambda c_: _assert(torch.equal(y.view[0].cpu(), x.to(BF16)), c_.name)
        return c

    footprint("cg_sum_f32", make_sum, layouts=("T", "O"))
    footprint("cg_cast_f32_bf16", make_cast, layouts=("T",))
    refused(make_cast("O"), "cg_cast_f32_bf16: misaligned")


# ---- cross entropy and the fused head ------------------------------------------------------------------------
@pytest.mark.parametrize("with_lp", [False, True])
def test_cross_entropy(with_lp):
    """cg_ce_fwd / cg_ce_bwd at rows = 48, V = 65, ld = V + 3, ld_d = V + 7 (layout O; P: + 4, + 8)."""
    rows, V = 48, 65
    g = torch.Generator().manual_seed(7)
    logits, tgt = torch.randn(rows, V, generator=g) * 3, torch.randint(0, V, (rows,), generator=g)
    lr = logits.double().requires_grad_(True)
    loss_rows = torch.nn.functional.cross_entropy(lr, tgt, reduction="none")
    loss_rows.sum().backward()
    lse_ref = torch.logsumexp(logits.double(), 1)
    ld_pad = {"T": (0, 0), "P": (4, 8), "O": (3, 7)}

    def make_fwd(lay):
        c = Call(f"cg_ce_fwd[{lay}]")
        lb = c.cin("logits", Box(rows, V, F32, ld=V + ld_pad[lay][0], offset_bytes=off(lay, F32), device=DEV), logits)
        tb = c.cin("targets", vec(rows, I64, pad=(int(tgt[0]) + 1) % V), tgt)
        lo, ls = c.cout("loss_rows", vec(rows, F32, lay)), c.cout("lse", vec(rows, F32, lay))
        c.launch = lambda: lib().cg_ce_fwd(P(lb), rows, V, lb.ld, P(tb), P(lo), P(ls), stream())
        c.verify = lambda c_: _assert(relerr(lo.view[0], loss_rows.detach()) < 1e-5 and relerr(ls.view[0], lse_ref) < 1e-5,
                                      c_.name)
        return c

    def make_bwd(lay):
        c = Call(f"cg_ce_bwd[{lay} bf16 copy {with_lp}]")
        lb = c.cin("logits", Box(rows, V, F32, ld=V + ld_pad[lay][0], offset_bytes=off(lay, F32), device=DEV), logits)
        tb = c.cin("targets", vec(rows, I64, pad=(int(tgt[0]) + 1) % V), tgt)
        ls, gb = c.cin("lse", vec(rows, F32, lay), lse_ref.float()), c.cin("g", vec(1, F32), torch.full((1,), 2.0))
        dl = c.cout("dlogits", Box(rows, V, F32, ld=V + ld_pad[lay][1], offset_bytes=off(lay, F32), device=DEV))
        lp = c.cout("dlogits_bf16", Box(rows, V, BF16, ld=V + ld_pad[lay][1], offset_bytes=off(lay, BF16), device=DEV)) \
            if with_lp else None
        c.launch = lambda: lib().cg_ce_bwd(P(lb), rows, V, lb.ld, P(tb), P(ls), P(gb), 1.0 / rows, P(dl), dl.ld, P(lp),
                                           stream())

        def verify(c_):
            assert relerr(dl.view, 2.0 / rows * lr.grad) < 1e-5, c_.name
            if with_lp:
                assert torch.equal(lp.view.cpu(), dl.view.cpu().to(BF16)), c_.name

        c.verify = verify
        return c

    footprint("cg_ce_fwd", make_fwd, layouts=("T", "P", "O"))
    footprint("cg_ce_bwd", make_bwd, layouts=("T", "P", "O"))


@pytest.mark.parametrize("M,C,V", [(64, 96, 16), (256, 384, 65)])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ex", [False, True])
def test_head(M, C, V, acc, ex):
    """cg_head_fwd and cg_head_bwd / cg_head_bwd_ex: dl is [M, ld_dl] with ld_dl the K-padded width --
    columns V..ld_dl-1 are OWNED and must be zero (header), beyond them is poison.  Layout T:
    ld_dl = 16 ceil(V / 16); layout P: that + 8.  Workspace of exactly cg_head_workspace bytes."""
    g = torch.Generator().manual_seed(11)
    a = torch.randn(M, C, generator=g).to(BF16)
    W = (torch.randn(V, C, generator=g) / C ** 0.5).to(BF16)
    bias, tgt = torch.randn(V, generator=g), torch.randint(0, V, (M,), generator=g)
    rowsW = (V + 15) // 16 * 16
    wpad = torch.zeros(rowsW, C, dtype=BF16)
    wpad[:V] = W
    lg = (a.double() @ W.double().t() + bias.double()).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lg, tgt)
    loss.backward()
    nws = lib().cg_head_workspace(M, V)
    saved = {}

    def make_fwd(lay):
        c = Call(f"cg_head_fwd[{lay} M {M} C {C} V {V}]")
        ab, wb = c.cin("a", box(M, C, BF16), a), c.cin("wpad", box(rowsW, C, BF16), wpad)
        bb, tb = c.cin("bias", vec(V, F32), bias), c.cin("targets", vec(M, I64, pad=(int(tgt[0]) + 1) % V), tgt)
        lo, ls, l1 = c.cout("logits", box(M, V, F32)), c.cout("lse", vec(M, F32)), c.cout("loss", vec(1, F32))
        c.ws_bytes = [nws]
        c.launch = lambda ws: lib().cg_head_fwd(P(ab), P(wb), rowsW, P(bb), P(tb), P(lo), P(ls), P(l1), P(ws), M, C, V,
                                                stream())

        def verify(c_):     # test_head_fused's bars
            saved["logits"], saved["lse"] = lo.view.clone(), ls.view[0].clone()
            assert relerr(lo.view, lg) < 1e-5 and relerr(ls.view[0], torch.logsumexp(lg.detach(), 1)) < 1e-5, c_.name
            assert abs(float(l1.view[0, 0]) - float(loss.detach())) < 1e-4 * max(1.0, abs(float(loss.detach()))), c_.name

        c.verify = verify
        return c

    def make_bwd(lay):
        ld_dl = rowsW + (8 if lay == "P" else 0)
        c = Call(f"cg_head_bwd{'_ex' if ex else ''}[{lay} M {M} V {V} ld_dl {ld_dl} accumulate {acc}]")
        lo, ls = c.cin("logits", box(M, V, F32), saved["logits"]), c.cin("lse", vec(M, F32), saved["lse"])
        tb, gb = c.cin("targets", vec(M, I64, pad=(int(tgt[0]) + 1) % V), tgt), c.cin("g_loss", vec(1, F32), torch.full((1,), 2.0))
        dl = c.cout("dl", box(M, ld_dl, BF16))
        init = torch.full((V,), 0.5)
        db = c.cio("db", vec(V, F32), init) if acc else c.cout("db", vec(V, F32))
        c.ws_bytes = [nws]

        def launch(ws):
            a_ = (P(lo), P(ls), P(tb), P(gb), 1.0 / M, None, P(dl), ld_dl, P(db), acc, P(ws), M, V)
            return lib().cg_head_bwd_ex(*a_, 0, stream()) if ex else lib().cg_head_bwd(*a_, stream())

        def verify(c_):
            want = 2.0 * lg.grad
            assert relerr(dl.view[:, :V], want) < 2e-2, c_.name
            assert float(dl.view[:, V:].float().abs().max()) == 0.0 if ld_dl > V else True, c_.name
            assert relerr(db.view[0], 0.5 * acc + want.sum(0)) < 1e-5, c_.name

        c.launch, c.verify = launch, verify
        return c

    footprint("cg_head_fwd", make_fwd, layouts=("T",))
    b = footprint("cg_head_bwd_ex" if ex else "cg_head_bwd", make_bwd, layouts=("T", "P"),
                  fallback="the owned width differs (ld_dl is the row stride AND the zero-padded width): compared "
                           "below on columns 0..V-1 and db")
    assert torch.equal(b["T"]["dl"][:, :V], b["P"]["dl"][:, :V]) and torch.equal(b["T"]["db"], b["P"]["db"])
    if not ex and not acc:      # ld_dl not a multiple of 8: refused, nothing written
        c = make_bwd("T")
        dl, db = c.out["dl"], c.out["db"]
        lo, ls, tb, gb = (c.const[k] for k in ("logits", "lse", "targets", "g_loss"))
        c.launch = lambda ws: lib().cg_head_bwd(P(lo), P(ls), P(tb), P(gb), 1.0 / M, None, P(dl), rowsW - 1, P(db), 0,
                                                P(ws), M, V, stream())
        refused(c, "cg_head_bwd: ld_dl must be a multiple of 8")


# ---- embeddings and the batch gather ------------------------------------------------------------------------
@pytest.mark.parametrize("V,T,C,B", [(65, 9, 21, 2), (65, 40, 126, 3)])
@pytest.mark.parametrize("acc", [0, 1])
def test_embedding(V, T, C, B, acc):
    g = torch.Generator().manual_seed(6)
    wte, wpe = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g)
    idx = torch.randint(0, V, (B, T), generator=g)
    dx = torch.randn(B * T, C, generator=g)
    i1, i2 = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g)
    padv = (int(idx[0, 0]) + 1) % V

    def make_fwd(lay):
        c = Call(f"cg_embed_fwd[{lay} V {V} T {T} C {C} B {B}]")
        ib = c.cin("idx", box(B, T, I64, pad=padv), idx)
        tb, pb = c.cin("wte", box(V, C, F32, lay), wte), c.cin("wpe", box(T, C, F32, lay), wpe)
        x = c.cout("x", box(B * T, C, F32, lay))
        c.launch = lambda: lib().cg_embed_fwd(P(ib), P(tb), P(pb), P(x), B, T, C, V, stream())
        c.verify = lambda c_: _assert(torch.equal(x.view.cpu(), (wte[idx] + wpe).reshape(B * T, C)), c_.name)
        return c

    def make_bwd(lay):
        c = Call(f"cg_embed_bwd[{lay} V {V} T {T} C {C} B {B} accumulate {acc}]")
        ib, db = c.cin("idx", box(B, T, I64, pad=padv), idx), c.cin("dx", box(B * T, C, F32, lay), dx)
        te = c.cio("dwte", box(V, C, F32, lay), i1) if acc else c.cout("dwte", box(V, C, F32, lay))
        pe = c.cio("dwpe", box(T, C, F32, lay), i2) if acc else c.cout("dwpe", box(T, C, F32, lay))
        c.ws_bytes = [lib().cg_embed_bwd_workspace(B, T, C, V)]
        c.launch = lambda ws: lib().cg_embed_bwd(P(ib), P(db), P(te), P(pe), B, T, C, V, acc, P(ws), stream())

        def verify(c_):     # test_embedding_fwd_bwd's bar
            want = torch.zeros(V, C, dtype=torch.float64).index_add_(0, idx.reshape(-1), dx.double())
            assert relerr(te.view, want + acc * i1.double()) < 2e-6, c_.name
            assert relerr(pe.view, dx.double().view(B, T, C).sum(0) + acc * i2.double()) < 2e-6, c_.name

        c.verify = verify
        return c

    if not acc:
        footprint("cg_embed_fwd", make_fwd, layouts=("T", "O"))
    footprint("cg_embed_bwd", make_bwd, layouts=("T", "O"))


@pytest.mark.parametrize("u8", [False, True])
def test_gather_batch(u8):
    """x[b, t] = data[ix[b] + t], y = the next token; the last window ends exactly at the end of data."""
    n, B, T = 500, 5, 33
    g = torch.Generator().manual_seed(1)
    data = torch.randint(0, 65, (n,), generator=g).to(torch.uint8 if u8 else I64)
    ix = torch.tensor([0, 17, 250, 311, n - T - 1])

    def make(lay):
        c = Call(f"cg_gather_batch[{lay} u8 {u8}]")
        d = c.cin("data", vec(n, data.dtype, pad=66), data)
        ib = c.cin("ix", vec(B, I64, pad=1), ix)
        x, y = c.cout("x", box(B, T, I64)), c.cout("y", box(B, T, I64))
        c.launch = lambda: lib().cg_gather_batch(P(d), int(u8), P(ib), P(x), P(y), B, T, stream())
        win = torch.stack([data[i:i + T + 1].long() for i in ix.tolist()])
        c.verify = lambda c_: _assert(torch.equal(x.view.cpu(), win[:, :T]) and torch.equal(y.view.cpu(), win[:, 1:]), c_.name)
        return c

    footprint("cg_gather_batch", make, layouts=("T",))


# ---- optimizer ---------------------------------------------------------------------------------------------------
def _adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step):
    p, g, m, v = (t.double() for t in (p, g, m, v))
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p * (1 - lr * wd)
    p = p - lr / (1 - b1 ** step) * m / ((v / (1 - b2 ** step)).sqrt() + eps)
    return p, m, v


@pytest.mark.parametrize("n", [4, 1000, 4096 + 4])
@pytest.mark.parametrize("form", ["adamw", "dyn", "dyn_gscale", "segments"])
def test_adamw(n, form):
    """cg_adamw, cg_adamw_dyn and cg_adamw_segments (two segments with a gap: the gap and everything
    outside keep their bits in p, m, v and p_bf16); p / g / m / v / p_bf16 each in their own Box."""
    g_ = torch.Generator().manual_seed(8)
    p0, gr = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    m0, v0 = torch.randn(n, generator=g_) * 0.1, torch.rand(n, generator=g_) * 0.1
    sh0 = torch.randn(n, generator=g_).to(BF16)
    lr, b1, b2, eps, wd, step, gs = 2e-4, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5
    segs = [(0, n // 4 // 4 * 4), (n // 2 // 4 * 4, n - n // 2 // 4 * 4)] if n > 4 else [(0, 4)]
    inside = torch.zeros(n, dtype=torch.bool)
    for s0, ln in segs if form == "segments" else [(0, n)]:
        inside[s0:s0 + ln] = True
    geff = (gr * np.float32(gs)) if form == "dyn_gscale" else gr
    rp, rm, rv = _adamw_ref(p0, geff, m0, v0, lr, b1, b2, eps, wd, step)

    def make(lay):
        c = Call(f"cg_adamw[{form} {lay} n {n}]")
        pb, mb, vb = c.cio("p", vec(n, F32, lay), p0), c.cio("m", vec(n, F32, lay), m0), c.cio("v", vec(n, F32, lay), v0)
        sb = c.cio("p_bf16", vec(n, BF16, lay), sh0)
        gb = c.cin("g", vec(n, F32, lay), gr)
        st = dev_i64(step)
        lr_dev = torch.tensor([lr], dtype=torch.float64, device=DEV)
        gs_dev = torch.tensor([gs], dtype=F32, device=DEV)
        arr = (ctypes.c_int64 * (2 * len(segs)))(*[x for s in segs for x in s])
        head = (P(pb), P(gb), P(mb), P(vb), P(sb))

        def launch():
            if form == "adamw":
                return lib().cg_adamw(*head, n, lr, b1, b2, eps, wd, P_t(st), stream())
            if form == "segments":
                return lib().cg_adamw_segments(*head, arr, len(segs), lr, b1, b2, eps, wd, P_t(st), stream())
            return lib().cg_adamw_dyn(*head, n, P_t(lr_dev), P_t(gs_dev) if form == "dyn_gscale" else None, b1, b2, eps,
                                      wd, P_t(st), stream())

        def verify(c_):     # test_adamw_matches_torch's bar; m and v: two fp32 roundings each, far inside it
            for nm, bx, want, init in (("p", pb, rp, p0), ("m", mb, rm, m0), ("v", vb, rv, v0)):
                got = bx.view[0].cpu()
                assert relerr(got[inside], want[inside]) < 1e-6, (c_.name, nm)
                assert torch.equal(got[~inside].view(I32), init[~inside].view(torch.int32)), (c_.name, nm, "outside the segments")
            sh = sb.view[0].cpu()
            assert torch.equal(sh[inside], pb.view[0].cpu().to(BF16)[inside]), c_.name
            assert torch.equal(sh[~inside].view(torch.int16), sh0[~inside].view(torch.int16)), (c_.name, "p_bf16 outside")

        c.launch, c.verify = launch, verify
        return c

    footprint(f"cg_adamw_{form}", make, layouts=("T",))
    if form == "segments":      # header: p, g, m, v 16-B aligned
        refused(make("O"), "cg_adamw_segments")
    else:                       # no alignment stated: the 4-B offset base takes the same update
        footprint(f"cg_adamw_{form}", make, layouts=("O",))


@pytest.mark.parametrize("n", [1, 1023, 4096 + 3])
@pytest.mark.parametrize("align", [0, 4, 8, 12])
def test_grad_norm_and_scale(n, align):
    """cg_grad_norm at every 4-B alignment of g with a workspace of exactly cg_grad_norm_workspace
    bytes, and cg_scale_f32 in place."""
    g_ = torch.Generator().manual_seed(12)
    gr = torch.randn(n, generator=g_)
    want = np.float32(np.sqrt(float((gr.double() ** 2).sum())))

    def make(lay):
        c = Call(f"cg_grad_norm[n {n} align {align}]")
        gb = c.cin("g", Box(1, n, F32, offset_bytes=align, device=DEV), gr)
        out = c.cout("out", vec(2, F32))
        c.ws_bytes = [lib().cg_grad_norm_workspace(n)]
        c.launch = lambda ws: lib().cg_grad_norm(P(gb), n, 0.25, P(out), P(ws), stream())

        def verify(c_):     # test_grad_norm_matches_float64: within one ulp; the coefficient from the returned norm
            norm, coef = (float(t) for t in out.view[0].cpu())
            assert abs(norm - float(want)) <= float(np.spacing(want)), (c_.name, norm, want)
            cw = np.float32(0.25) / (np.float32(norm) + np.float32(1e-6))
            assert coef == float(cw if cw < 1 else np.float32(1.0)), (c_.name, coef)

        c.verify = verify
        return c

    def make_scale(lay):
        c = Call(f"cg_scale_f32[n {n} align {align}]")
        xb = c.cio("x", Box(1, n, F32, offset_bytes=align, device=DEV), gr)
        sc = torch.tensor([0.3], device=DEV)
        c.launch = lambda: lib().cg_scale_f32(P(xb), n, P_t(sc), stream())
        c.verify = lambda c_: _assert(torch.equal(xb.view[0].cpu(), gr * np.float32(0.3)), c_.name)
        return c

    footprint("cg_grad_norm", make, layouts=("T",))
    footprint("cg_scale_f32", make_scale, layouts=("T",))


# ---- the inference path: decode.hip and rows_f32.hip ------------------------------------------------------------
DEC_FORMS = ("cache-D21", "qkvrows-D21", "generic-D21", "cache-D64")


def make_decode_attn(lay, form, fixed):
    """cg_decode_attn, one query per (b, h) against n = 70 of Tmax = 128 keys; the K / V rows >= n are
    NaN (const operands: the stale part of a cache).  cache-D21: tight key rows reach
    k_decode_attn_rows<24>, padded ones (layouts P, O) its SJ form; qkvrows: K / V inside a window's qkv
    rows (SJ); generic: decode_attn_rows 0, k_decode_attn<24>; cache-D64: k_decode_attn<64>."""
    D_ = 64 if form.endswith("D64") else 21
    B, H, Tmax, n = 3, 2, 128, 70
    HD = H * D_
    g = torch.Generator().manual_seed(21)
    q = torch.randn(B, HD, generator=g)
    K, V = torch.randn(B, H, Tmax, D_, generator=g), torch.randn(B, H, Tmax, D_, generator=g)
    scale = f32(HD ** -0.5)
    s = torch.einsum("bhd,bhjd->bhj", q.view(B, H, D_).double(), K[:, :, :n].double()) * scale
    want = torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1), V[:, :, :n].double()).reshape(B, HD)
    K[:, :, n:] = float("nan")
    V[:, :, n:] = float("nan")
    c = Call(f"cg_decode_attn[{lay} {form} {'nkeys' if fixed else 'len_dev'} n {n}]")
    qb = c.cin("q", box(B, HD, F32, lay, 1), q)
    ob = c.cout("o", box(B, HD, F32, lay, 2))
    if form.startswith("qkvrows"):
        rows = torch.cat([torch.randn(B, Tmax, HD, generator=g), K.permute(0, 2, 1, 3).reshape(B, Tmax, HD),
                          V.permute(0, 2, 1, 3).reshape(B, Tmax, HD)], 2).reshape(B * Tmax, 3 * HD)
        kv = c.cin("qkv rows", box(B * Tmax, 3 * HD, F32, lay, 3), rows)
        kp, vp, sb, sh, sj = P(kv, HD), P(kv, 2 * HD), Tmax * kv.ld, D_, kv.ld
    else:
        kb = c.cin("k", box(B * H * Tmax, D_, F32, lay, 3), K.reshape(-1, D_))
        vb = c.cin("v", box(B * H * Tmax, D_, F32, lay, 3), V.reshape(-1, D_))
        kp, vp, sj = P(kb), P(vb), kb.ld
        sh, sb = Tmax * sj, H * Tmax * sj
    ln = c.keep = dev_i64(n)
    c.launch = lambda: lib().cg_decode_attn(P(qb), qb.ld, kp, vp, sb, sh, sj, B, H, D_, None if fixed else P_t(ln),
                                            n if fixed else 0, scale, P(ob), ob.ld, stream())
    c.verify = lambda c_: _assert(relerr(ob.view, want) < 1e-5, (c_.name, relerr(ob.view, want)))
    return c


@pytest.mark.parametrize("fixed", [False, True], ids=["len_dev", "nkeys"])
@pytest.mark.parametrize("form", DEC_FORMS)
def test_decode_attn(form, fixed):
    """The four dispatch forms in layouts T, P and O (the header states no alignment and takes any
    strides): checks 1-5, the three layouts' bits equal (the kernels are bitwise twins)."""
    assert tuning("decode_attn_rows", 0 if form.startswith("generic") else 1) == 0
    try:
        bits = footprint("cg_decode_attn", lambda lay: make_decode_attn(lay, form, fixed), layouts=("T", "P", "O"))
        same_bits(bits["T"], bits["O"], f"cg_decode_attn {form}: layout T against layout O")
    finally:
        tuning("decode_attn_rows", 1)


def test_decode_kv_append():
    """The caches are in/out operands: only row len - 1 of every (b, h) changes, to the qkv row's bits."""
    B, H, D_, Tmax, n = 3, 2, 21, 16, 8
    HD = H * D_
    g = torch.Generator().manual_seed(22)
    qkv = torch.randn(B, 3 * HD, generator=g)
    k0, v0 = torch.randn(B * H * Tmax, D_, generator=g), torch.randn(B * H * Tmax, D_, generator=g)

    def make(lay):
        c = Call(f"cg_decode_kv_append[{lay}]")
        qb = c.cin("qkv", box(B, 3 * HD, F32, lay, 1), qkv)
        kb = c.cio("kcache", Box(B * H * Tmax, D_, F32, offset_bytes=off(lay, F32), device=DEV), k0)
        vb = c.cio("vcache", Box(B * H * Tmax, D_, F32, offset_bytes=off(lay, F32), device=DEV), v0)
        ln = c.keep = dev_i64(n)
        c.launch = lambda: lib().cg_decode_kv_append(P(qb), qb.ld, HD, 2 * HD, B, H, D_, Tmax, P_t(ln), P(kb), P(vb), stream())

        def verify(c_):
            for name, bx, init, col in (("k", kb, k0, HD), ("v", vb, v0, 2 * HD)):
                want = init.clone().view(B, H, Tmax, D_)
                want[:, :, n - 1] = qkv[:, col:col + HD].view(B, H, D_)
                assert torch.equal(bx.view.cpu().view(I32), want.view(-1, D_).view(I32)), (c_.name, name)

        c.verify = verify
        return c

    footprint("cg_decode_kv_append", make, layouts=("T", "P", "O"))


@pytest.mark.parametrize("n", [5, 12, 20])
def test_decode_window(n):
    """out[b, j] = idx[b, max(0, len - T) + j] at len below, at and above T = 12; idx rows of 20 tokens."""
    B, T, Lx = 3, 12, 20
    idx = torch.randint(0, 65, (B, Lx), generator=torch.Generator().manual_seed(23))

    def make(lay):
        c = Call(f"cg_decode_window[{lay} len {n}]")
        ib = c.cin("idx", box(B, Lx, I64, lay, 1, pad=3), idx)
        ob = c.cout("out", Box(B, T, I64, offset_bytes=off(lay, I64), device=DEV))
        ln = c.keep = dev_i64(n)
        c.launch = lambda: lib().cg_decode_window(P(ib), ib.ld, B, T, P_t(ln), P(ob), stream())
        start = max(0, n - T)
        c.verify = lambda c_: _assert(torch.equal(ob.view.cpu(), idx[:, start:start + T]), c_.name)
        return c

    footprint("cg_decode_window", make, layouts=("T", "P", "O"))


def test_decode_embed():
    """x[b] = wte[idx[b, len - 1]] + wpe[len - 1], bit for bit."""
    B, C, Vn, Tmax, n = 5, 126, 65, 16, 9
    g = torch.Generator().manual_seed(24)
    idx = torch.randint(0, Vn, (B, Tmax), generator=g)
    wte, wpe = torch.randn(Vn, C, generator=g), torch.randn(Tmax, C, generator=g)

    def make(lay):
        c = Call(f"cg_decode_embed[{lay}]")
        ib = c.cin("idx", box(B, Tmax, I64, lay, 1, pad=3), idx)
        tb = c.cin("wte", Box(Vn, C, F32, offset_bytes=off(lay, F32), device=DEV), wte)
        pb = c.cin("wpe", Box(Tmax, C, F32, offset_bytes=off(lay, F32), device=DEV), wpe)
        xb = c.cout("x", Box(B, C, F32, offset_bytes=off(lay, F32), device=DEV))
        ln = c.keep = dev_i64(n)
        c.launch = lambda: lib().cg_decode_embed(P(ib), ib.ld, P(tb), P(pb), C, P_t(ln), P(xb), B, stream())
        c.verify = lambda c_: _assert(torch.equal(xb.view.cpu(), wte[idx[:, n - 1]] + wpe[n - 1]), c_.name)
        return c

    footprint("cg_decode_embed", make, layouts=("T", "P", "O"))


def _ln64(x, w, b, eps=1e-5):
    x = x.double()
    mu = x.mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps) * w.double() + b.double()


@pytest.mark.parametrize("kind", ["store", "bias_relu", "bias_resid"])
@pytest.mark.parametrize("ln", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("M", [33, 2050])
def test_linear_rows_f32(M, ln, kind):
    """cg_linear_rows_f32 on both sides of 2048 rows (k_gemm_f32r, k_linear_f32q), with and without the
    LayerNorm.  Layout O: odd strides and a 4-B offset base are refused (the header: lda / ldw even, a / W
    8-B aligned).  The header names no aliasing for this call, so resid and out stay apart."""
    N, K = 70, 126
    g = torch.Generator().manual_seed(25)
    a = torch.randn(M, K, generator=g) * 2 + 0.5
    W, bias, resid = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    lw, lb = torch.randn(K, generator=g) * 0.1 + 1, torch.randn(K, generator=g) * 0.1
    want = (_ln64(a, lw, lb) if ln else a.double()) @ W.double().t()
    if kind != "store":
        want = want + bias.double()
    want = torch.relu(want) if kind == "bias_relu" else want
    want = want + resid.double() if kind == "bias_resid" else want

    def make(lay):
        c = Call(f"cg_linear_rows_f32[{lay} M {M} ln {int(ln)} {kind}]")
        dense_a = ln and M > 2048 and lay == "P"        # the header: lda == K with the LayerNorm above 2048 rows
        ab = c.cin("a", box(M, K, F32, lay, 0 if dense_a else 1), a)
        wb = c.cin("w", box(N, K, F32, lay, 2), W)
        lwb = c.cin("ln_w", vec(K, F32, lay), lw) if ln else None
        lbb = c.cin("ln_b", vec(K, F32, lay), lb) if ln else None
        bb = c.cin("bias", vec(N, F32, lay), bias) if kind != "store" else None
        rb = c.cin("resid", box(M, N, F32, lay, 3), resid) if kind == "bias_resid" else None
        ob = c.cout("out", box(M, N, F32, lay, 4))
        c.launch = lambda: lib().cg_linear_rows_f32(M, N, K, P(ab), ab.ld, P(lwb), P(lbb), 1e-5, P(wb), wb.ld, P(bb),
                                                    int(kind == "bias_relu"), P(rb), rb.ld if rb is not None else 0, P(ob), ob.ld,
                                                    stream())
        c.verify = lambda c_: _assert(relerr(ob.view, want) < 1e-5, (c_.name, relerr(ob.view, want)))
        return c

    footprint("cg_linear_rows_f32", make)
    refused(make("O"), "cg_linear_rows_f32")


@pytest.mark.parametrize("ln", [True, False], ids=["ln", "noln"])
@pytest.mark.parametrize("M", [33, 300])
def test_ffn_fwd_f32(M, ln):
    """cg_ffn_fwd_f32 with out aliasing resid (an in/out operand), one block and three; layout O refused."""
    C, Hh = 126, 504
    g = torch.Generator().manual_seed(26)
    a = torch.randn(M, C, generator=g) * 2 + 0.5
    W1, b1 = torch.randn(Hh, C, generator=g) / C ** 0.5, torch.randn(Hh, generator=g)
    W2, b2 = torch.randn(C, Hh, generator=g) / Hh ** 0.5, torch.randn(C, generator=g)
    resid = torch.randn(M, C, generator=g)
    lw, lb = torch.randn(C, generator=g) * 0.1 + 1, torch.randn(C, generator=g) * 0.1
    y = _ln64(a, lw, lb) if ln else a.double()
    want = resid.double() + torch.relu(y @ W1.double().t() + b1.double()) @ W2.double().t() + b2.double()

    def make(lay):
        c = Call(f"cg_ffn_fwd_f32[{lay} M {M} ln {int(ln)} out = resid]")
        ab = c.cin("a", box(M, C, F32, lay, 0 if ln and lay == "P" else 1), a)       # the header: lda == C with the LayerNorm
        w1b, w2b = c.cin("w1", box(Hh, C, F32, lay, 2), W1), c.cin("w2", box(C, Hh, F32, lay, 3), W2)
        b1b, b2b = c.cin("b1", vec(Hh, F32, lay), b1), c.cin("b2", vec(C, F32, lay), b2)
        lwb = c.cin("ln_w", vec(C, F32, lay), lw) if ln else None
        lbb = c.cin("ln_b", vec(C, F32, lay), lb) if ln else None
        ob = c.cio("out = resid", box(M, C, F32, lay, 4), resid)
        c.launch = lambda: lib().cg_ffn_fwd_f32(M, C, Hh, P(ab), ab.ld, P(lwb), P(lbb), 1e-5, P(w1b), w1b.ld, P(b1b), P(w2b), w2b.ld,
                                                P(b2b), P(ob), ob.ld, P(ob), ob.ld, stream())
        c.verify = lambda c_: _assert(relerr(ob.view, want) < 1e-5, (c_.name, relerr(ob.view, want)))
        return c

    footprint("cg_ffn_fwd_f32", make)
    refused(make("O"), "cg_ffn_fwd_f32")


def test_decode_qkv_f32():
    """cg_decode_qkv_f32: qkv an output, the caches in/out (only row len - 1 of every (b, h) changes, to
    the bits of the qkv row just written); layout O refused (ldx / ldw even, x / W / ln_w / ln_b 8-B aligned)."""
    B, C, H, Tmax, n = 5, 126, 3, 16, 8
    Dh = C // H
    g = torch.Generator().manual_seed(27)
    x = torch.randn(B, C, generator=g) * 2 + 0.5
    W = torch.randn(3 * C, C, generator=g) / C ** 0.5
    lw, lb = torch.randn(C, generator=g) * 0.1 + 1, torch.randn(C, generator=g) * 0.1
    k0, v0 = torch.randn(B * H * Tmax, Dh, generator=g), torch.randn(B * H * Tmax, Dh, generator=g)
    want = _ln64(x, lw, lb) @ W.double().t()

    def make(lay):
        c = Call(f"cg_decode_qkv_f32[{lay}]")
        xb, wb = c.cin("x", box(B, C, F32, lay, 1), x), c.cin("w", box(3 * C, C, F32, lay, 2), W)
        lwb, lbb = c.cin("ln_w", vec(C, F32, lay), lw), c.cin("ln_b", vec(C, F32, lay), lb)
        qb = c.cout("qkv", box(B, 3 * C, F32, lay, 3))
        kb = c.cio("kcache", Box(B * H * Tmax, Dh, F32, offset_bytes=off(lay, F32), device=DEV), k0)
        vb = c.cio("vcache", Box(B * H * Tmax, Dh, F32, offset_bytes=off(lay, F32), device=DEV), v0)
        ln = c.keep = dev_i64(n)
        c.launch = lambda: lib().cg_decode_qkv_f32(B, C, H, P(xb), xb.ld, P(lwb), P(lbb), 1e-5, P(wb), wb.ld, P(qb), qb.ld, P_t(ln),
                                                   Tmax, P(kb), P(vb), stream())

        def verify(c_):
            got = qb.view.cpu()
            assert relerr(got, want) < 1e-5, (c_.name, relerr(got, want))
            for name, bx, init, col in (("k", kb, k0, C), ("v", vb, v0, 2 * C)):
                exp = init.clone().view(B, H, Tmax, Dh)
                exp[:, :, n - 1] = got[:, col:col + C].reshape(B, H, Dh)
                assert torch.equal(bx.view.cpu().view(I32), exp.view(-1, Dh).view(I32)), (c_.name, name)

        c.verify = verify
        return c

    footprint("cg_decode_qkv_f32", make)
    refused(make("O"), "cg_decode_qkv_f32")


# ---- the registry: no entry point left out, nothing skipped silently --------------------------------------
def strided_entry_points():
    """Every cg_* function of the header that takes a stride argument (ld*, stride_*, sb / sh / sj, or a
    problem list)."""
    src = re.sub(r"/\*.*?\*/", "", open(L().HEADER_PATH).read(), flags=re.S)
    out = set()
    for name, args in re.findall(r"\b(cg_\w+)\s*\(([^;{]*?)\)\s*;", src):
        if re.search(r"int64_t\s+(ld\w*|stride_\w+|sb|sh|sj)\b", args) or "cg_wgrad_problem_t" in args:
            out.add(name)
    return out


def test_every_strided_entry_point_ran_padded():
    """For every entry point of the header that takes a stride, at least one layout-P case ran the
    kernel (the samplers and the two prefill calls have theirs in the files ELSEWHERE names).  Also prints the
    run's record: the case count, every asserted refusal and every check-2 fallback."""
    entries = strided_entry_points()
    assert {"cg_gemm", "cg_attn_bwd_delta", "cg_ce_bwd", "cg_colsum", "cg_head_bwd_ex"} <= entries
    assert ELSEWHERE <= entries and MOVED_HERE <= entries and not (ELSEWHERE & MOVED_HERE)
    need = sorted(e for e in entries - ELSEWHERE if not e.endswith("_supported"))
    print(f"\nfootprint cases run: {CASES[0]}")
    print(f"layout-P runs per strided entry point: { {e: RAN_P.get(e, 0) for e in need} }")
    print(f"asserted refusals ({len(REFUSALS)}):")
    for case, msg in sorted(set(REFUSALS)):
        print(f"  {case}: {msg}")
    print("check 2 replaced by check 1:")
    for case, why in sorted(set(FELL_BACK)):
        print(f"  {case}: {why}")
    assert MOVED_HERE <= set(need)
    missing = [e for e in need if RAN_P.get(e, 0) == 0]
    assert not missing, f"no layout-P case ran {missing}"
