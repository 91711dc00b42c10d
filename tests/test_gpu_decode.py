"""The decode engine (replicatinggpt_amd/decode.py, csrc/decode.hip, the fp32 row kernels of
csrc/rows_f32.hip and csrc/gemm_f32.hip) on the MI355X against the fp64 CPU oracle, through every
dispatch branch and A/B switch, plus the device sampler against an exact expectation and the row kernels with the strides
and views the engine hands them.

Teacher forcing: the oracle is given the engine's own output as context, so one near-tie decides one
(row, step) pair and not the rest of that row.  Every gate below is derived from the number formats
(the project's 1e-5 fp32 logits bar, the 24-bit uniform and V sequential fp32 additions of the
sampler), never from what the engine returns, and every gated test prints its gated share and fails
above its cap."""
import hashlib
import json

import numpy as np
import pytest
import torch

from conftest import bf16_close, golden_path, ROOT
from oracle import gpt1_oracle as O
from oracle import philox

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 65
FP32_BAR = 1e-5   # relative to the largest logit: test_gpu_model.py::test_model_fp32_matches_reference


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------
# models, oracle parameters, teacher-forced oracle logits (cached per distinct stream)
# ---------------------------------------------------------------------------------------
def make_model(T, C, H, L, seed, dtype="fp32"):
    """Seeded random init with the LayerNorm weights / biases moved off 1 / 0 (the init would hide a
    kernel that dropped or misread them)."""
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    torch.manual_seed(seed)
    m = BigramLanguageModel(GPTConfig(block_size=T, n_embd=C, n_head=H, n_layers=L, dropout=0.0, dtype=dtype))
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if ".ln1." in name or ".ln2." in name or name.startswith("ln_f."):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m.to(DEV)


def oracle_params(m):
    return {k: v.double().cpu() for k, v in m.state_dict().items() if "tril" not in k}


def oracle_cfg(T, C, H, L):
    return O.OracleConfig(block_size=T, n_embd=C, n_head=H, n_layers=L, dropout=0.0)


_TEACHER = {}


def teacher_logits(P, ocfg, got, L0, tag):
    """fp64 oracle logits [B, total - L0, V] of the last row of O.forward(P, got[:, max(0, n - T):n])
    for every generated column n; cached per (weights tag, stream)."""
    got = got.cpu()
    key = (tag, L0, tuple(got.shape), hashlib.sha1(got.numpy().tobytes()).hexdigest())
    if key not in _TEACHER:
        T = ocfg.block_size
        rows = []
        with torch.no_grad():
            for n in range(L0, got.shape[1]):
                lg, _ = O.forward(P, got[:, max(0, n - T):n], ocfg)
                rows.append(lg[:, -1, :])
        _TEACHER[key] = torch.stack(rows, dim=1)
    return _TEACHER[key]


def check_greedy_fp32(got, idx, ref, eng_logits, label):
    """Section A, fp32 greedy: prompt kept; got[b, n] == the oracle's argmax, except where the oracle's
    top-2 gap is below 2 * 1e-5 * max|logit| of that step (each of two logits may move by the fp32
    logits bar) -- there the token is still one of the top two; gated pairs at most 1 % of the case;
    the engine's final-step logits within 1e-5 of the oracle's, ungated."""
    got = got.cpu()
    B, L0 = idx.shape
    assert got.shape[0] == B and torch.equal(got[:, :L0], idx.cpu()), f"{label}: prompt columns changed"
    gen = got[:, L0:]
    assert int(gen.min()) >= 0 and int(gen.max()) < V, f"{label}: token outside the vocabulary"
    top = ref.topk(2, dim=-1)
    gap = top.values[..., 0] - top.values[..., 1]
    bar = 2 * FP32_BAR * ref.abs().amax(dim=(0, 2))[None, :]          # per step
    gated = gap < bar
    share = float(gated.double().mean())
    print(f"{label}: gated pairs {int(gated.sum())} of {gated.numel()} ({100 * share:.3f} %)")
    is_top1 = gen == top.indices[..., 0]
    is_top2 = gen == top.indices[..., 1]
    bad = (~gated & ~is_top1) | (gated & ~(is_top1 | is_top2))
    if bool(bad.any()):
        b, s = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{label}: {int(bad.sum())} of {bad.numel()} tokens differ from the oracle "
                             f"({int(bad.any(dim=1).sum())} of {B} rows); first at row {b} column {L0 + s}: "
                             f"got {int(gen[b, s])}, oracle {int(top.indices[b, s, 0])}, gap {float(gap[b, s]):.3e}")
    assert share <= 0.01, f"{label}: {100 * share:.2f} % of pairs gated (cap 1 %)"
    e = relerr(eng_logits, ref[:, -1, :])
    print(f"{label}: final-step logits relerr {e:.3e}")
    assert e < FP32_BAR, f"{label}: final-step logits relerr {e:.3e}"


# ---------------------------------------------------------------------------------------
# B. path matrix
# ---------------------------------------------------------------------------------------
# (B, T, C, H, L, L0, new to end in phase 2, new to end in phase 1)
SHAPES = {
    "S1": (3, 64, 96, 4, 3, 5, 90, 40),         # below 2048 window rows: no split path
    "S2": (33, 64, 96, 4, 2, 5, 70, 40),        # 2112 window rows: LAST_KV_SPLIT branch; D = 24: both k_decode_attn_rows layouts
    "S3": (2049, 8, 32, 2, 2, 3, 12, 4),        # B > 2048: every _ln_linear falls back, _step1's else branch
    "S4": (17, 128, 128, 2, 2, 120, 16, 4),     # D = 64: k_decode_attn<64>; C = 128: the row kernels' K limit
    "S5": (17, 128, 132, 6, 2, 120, 16, 4),     # C > 128: no row kernel, _step2's generic fp32 branch
}
SEEDS = {"S1": 11, "S2": 12, "S3": 13, "S4": 14, "S5": 15}
OFF = {"DECODE_ROWS": False, "LAST_KV_SPLIT": False, "ATTN_ROWS": False, "FFN_FUSED": False, "FFN_LN": False}
SWITCHES = {
    "defaults": {},
    "decode_rows0": {"DECODE_ROWS": False},
    "last_kv_split0": {"LAST_KV_SPLIT": False},
    "attn_rows0_ffn_fused0": {"ATTN_ROWS": False, "FFN_FUSED": False},
    "ffn_ln0": {"FFN_LN": False},
    "all_off": OFF,
    "no_graph": {},
}
_RUNS = {}


def _set_switches(mp, sw):
    from replicatinggpt_amd import decode
    from replicatinggpt_amd import functional as Fn
    for k, v in sw.items():
        mp.setattr(decode if k in ("DECODE_ROWS", "LAST_KV_SPLIT") else Fn, k, v)


def run_case(shape, ending, sw):
    """One greedy fp32 generate of a fresh model (no cached engine, no stale graph) under a switch
    set; checks section A; returns (stream, final logits) on the CPU, cached per case."""
    key = (shape, ending, sw)
    if key in _RUNS:
        return _RUNS[key]
    from replicatinggpt_amd.decode import DecodeEngine
    B, T, C, H, L, L0, new2, new1 = SHAPES[shape]
    new = new2 if ending == "p2" else new1
    assert (L0 + new > T) == (ending == "p2")
    label = f"{shape}/{ending}/{sw}"
    m = make_model(T, C, H, L, SEEDS[shape])
    training = ending == "p1"
    m.train(training)
    idx = torch.randint(0, V, (B, L0), generator=torch.Generator().manual_seed(SEEDS[shape] + 100)).to(DEV)
    with pytest.MonkeyPatch.context() as mp:
        _set_switches(mp, SWITCHES[sw])
        with torch.no_grad():
            if sw == "no_graph":
                eng = DecodeEngine(m, B, L0 + new, greedy=True, use_graph=False)
                got = eng.generate(idx, new)
                assert eng.g1 is None and eng.g2 is None
            else:
                got = m.generate(idx, new, greedy=True)
                (eng,) = m._decode_engines.values()
        torch.cuda.synchronize()
    assert m.training == training, f"{label}: generate() left m.training changed"
    assert got.shape == (B, L0 + new)
    logits = eng.logits.detach().cpu().clone()
    got = got.cpu()
    ref = teacher_logits(oracle_params(m), oracle_cfg(T, C, H, L), got, L0, shape)
    check_greedy_fp32(got, idx, ref, logits, label)
    _RUNS[key] = (got, logits)
    return _RUNS[key]


@pytest.mark.parametrize("sw", list(SWITCHES))
@pytest.mark.parametrize("ending", ["p1", "p2"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_decode_paths_match_oracle(shape, ending, sw):
    """Every dispatch branch of the decode engine (SHAPES) under every A/B switch set, ending in
    phase 1 (K/V cache) and in phase 2 (sliding window): section A against the fp64 oracle, the prompt
    kept, m.training kept -- and, because each switch's docstring claims the bits of the path it
    replaces, the same stream and bitwise the same final logits as the default switches.

    On the parent commit S3/defaults and the S2 / S3 DECODE_ROWS=0 cases failed in phase 2: the last
    block's final rows reached cg_layernorm_fwd as a row-strided view, which it read as dense."""
    got, logits = run_case(shape, ending, sw)
    if sw != "defaults":
        got0, logits0 = run_case(shape, ending, "defaults")
        assert torch.equal(got, got0), f"{shape}/{ending}/{sw}: stream differs from the default switches'"
        assert torch.equal(logits.view(torch.int32), logits0.view(torch.int32)), \
            f"{shape}/{ending}/{sw}: final logits not bitwise the default switches' (relerr {relerr(logits, logits0):.3e})"


# ---------------------------------------------------------------------------------------
# C. the LayerNorm op refuses rows it cannot address
# ---------------------------------------------------------------------------------------
def test_layernorm_fwd_refuses_strided_rows():
    """cg_layernorm_fwd takes a pointer and no row stride: ops.layernorm_fwd raises on a non-dense x
    (or y) instead of normalising the wrong rows, and still takes the dense copy."""
    from replicatinggpt_amd import ops
    B, T, C = 5, 4, 32
    x = torch.randn(B, T, C, device=DEV)
    w = 1.0 + 0.1 * torch.randn(C, device=DEV)
    b = 0.1 * torch.randn(C, device=DEV)
    y = torch.empty(B, C, device=DEV)
    mean, rstd = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    xl = x[:, T - 1, :]
    with pytest.raises(ValueError, match="dense"):
        ops.layernorm_fwd(xl, w, b, y, mean, rstd, 1e-5)
    with pytest.raises(ValueError, match="dense"):
        ops.layernorm_fwd(xl.contiguous(), w, b, torch.empty(B, 2 * C, device=DEV)[:, :C], mean, rstd, 1e-5)
    ops.layernorm_fwd(xl.contiguous(), w, b, y, mean, rstd, 1e-5)
    ref = torch.nn.functional.layer_norm(xl.double().cpu(), (C,), w.double().cpu(), b.double().cpu(), 1e-5)
    assert relerr(y, ref) < 1e-5


# ---------------------------------------------------------------------------------------
# D. the sampler against an exact expectation
# ---------------------------------------------------------------------------------------
def sample_gate(Vn):
    """Relative to the softmax sum: V sequential fp32 additions plus __expf and the u * s product
    (V + 16 roundings of 2^-24), times a safety factor of 4."""
    return 4 * (Vn + 16) * 2.0 ** -24


def expected_sample(logits64, seed, length, g):
    """k_decode_sample's non-greedy token per row in fp64 and the rows whose draw lies within g * S of a
    CDF boundary: u = (Philox4x32-10(counter (row, 0, length, 0), key seed)[0] >> 8) / 2^24, the first
    v with u * S < cumsum(exp(l - max))[v], else V - 1."""
    l = logits64.double().numpy()
    Bn, Vn = l.shape
    b = np.arange(Bn, dtype=np.uint64)
    r0 = philox.philox4x32_10(b, 0, length, 0, seed & 0xffffffff, seed >> 32)[0]
    u = (r0 >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    c = np.cumsum(np.exp(l - l.max(axis=1, keepdims=True)), axis=1)
    S = c[:, -1]
    t = u * S
    tok = np.minimum((c <= t[:, None]).sum(axis=1), Vn - 1)
    gate = np.broadcast_to(np.asarray(g, dtype=np.float64), S.shape)
    gated = (np.abs(t[:, None] - c) < (gate * S)[:, None]).any(axis=1)
    return tok, gated


@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("Vn", [1, 2, 64, 65, 200])
def test_decode_sample_matches_inverse_cdf(Vn, scale):
    """ops.decode_sample, non-greedy, 4096 rows of scale * randn logits: every row whose draw is not
    within the gate of a CDF boundary gets exactly the fp64 inverse-CDF token of its (seed, length,
    row) Philox draw -- dense and padded logits rows, two lengths, a seed below 2^32 and one with high
    bits; only column `length` of idx is written.  Gated rows at most 3 % of a case (printed)."""
    from replicatinggpt_amd import ops
    Bn = 4096
    g = sample_gate(Vn)
    gen = torch.Generator().manual_seed(1000 * Vn + scale)
    logits = scale * torch.randn(Bn, Vn, generator=gen)
    wide = torch.full((Bn, Vn + 7), 50.0)        # a padded row: a kernel reading past V would pick these
    wide[:, :Vn] = logits
    dense_d, wide_d = logits.to(DEV), wide.to(DEV)
    for length in (1, 37):
        for seed in (987654321, 2 ** 61 + 12345):
            want, gated = expected_sample(logits, seed, length, g)
            share = float(gated.mean())
            for name, lg in (("dense", dense_d), ("padded", wide_d[:, :Vn])):
                assert lg.stride(0) == (Vn if name == "dense" else Vn + 7)
                idx = torch.full((Bn, length + 3), -7, dtype=torch.int64, device=DEV)
                ops.decode_sample(lg, False, torch.tensor([seed], dtype=torch.int64, device=DEV),
                                  torch.tensor([length], dtype=torch.int64, device=DEV), idx)
                torch.cuda.synchronize()
                out = idx.cpu()
                keep = torch.ones(length + 3, dtype=torch.bool)
                keep[length] = False
                assert bool((out[:, keep] == -7).all()), "a column other than `length` was written"
                tok = out[:, length].numpy()
                assert tok.min() >= 0 and tok.max() < Vn
                miss = (tok != want) & ~gated
                print(f"V={Vn} scale={scale} len={length} seed={seed} {name}: gated {100 * share:.2f} %, "
                      f"gated rows differing {int(((tok != want) & gated).sum())}, ungated mismatches {int(miss.sum())}")
                assert not miss.any(), (name, length, seed, int(miss.sum()), int(np.nonzero(miss)[0][0]))
            assert share <= 0.03, f"V={Vn} scale={scale} len={length} seed={seed}: {100 * share:.2f} % gated (cap 3 %)"


def _greedy(logits):
    from replicatinggpt_amd import ops
    Bn = logits.shape[0]
    idx = torch.full((Bn, 4), -7, dtype=torch.int64, device=DEV)
    ops.decode_sample(logits.to(DEV), True, torch.zeros(1, dtype=torch.int64, device=DEV),
                      torch.tensor([2], dtype=torch.int64, device=DEV), idx)
    torch.cuda.synchronize()
    out = idx.cpu()
    assert bool((out[:, [0, 1, 3]] == -7).all())
    return out[:, 2]


def _tie_rows(Vn):
    """Rows of randn logits with the maximum duplicated / infinite, for V = Vn."""
    gen = torch.Generator().manual_seed(Vn)
    inf = float("inf")
    rows, names = [], []

    def add(name, edit):
        r = torch.randn(Vn, generator=gen)
        edit(r)
        rows.append(r)
        names.append(name)

    hi = Vn - 30            # a second column: lane hi % 64 (V = 100: 70 -> lane 6)
    add("plain", lambda r: None)
    add("max twice across lanes", lambda r: r.__setitem__([3, hi], 9.0))
    add("max twice across lanes, later first", lambda r: r.__setitem__([hi, Vn - 1], 9.0))
    add("all equal", lambda r: r.fill_(0.25))
    add("all -inf", lambda r: r.fill_(-inf))
    add("+inf twice", lambda r: r.__setitem__([5, hi], inf))
    add("-inf but one", lambda r: (r.fill_(-inf), r.__setitem__(Vn - 1, -3.0)))
    if Vn > 70:
        add("max twice in one lane", lambda r: r.__setitem__([6, 70], 9.0))
        add("max in lanes 3, 6 and lane 6 again", lambda r: r.__setitem__([6, 70, 67], 9.0))
        add("+inf twice in one lane", lambda r: r.__setitem__([70, 6], inf))
    return torch.stack(rows), names


@pytest.mark.parametrize("Vn", [100, 40, 65])
def test_decode_sample_greedy_ties_and_infinities(Vn):
    """Greedy = torch.argmax of the CPU copy: the first maximum when it is duplicated across lanes,
    within one lane (columns v and v + 64) or everywhere, with +inf twice, on an all -inf row, for a
    vocabulary below, at and above one 64-lane pass."""
    rows, names = _tie_rows(Vn)
    got = _greedy(rows)
    want = torch.argmax(rows, dim=-1)
    for i, name in enumerate(names):
        assert int(got[i]) == int(want[i]), (name, int(got[i]), int(want[i]))


@pytest.mark.parametrize("Vn", [100, 40])
def test_decode_sample_greedy_nan_rows(Vn):
    """A NaN logit counts as the maximum, the first one winning (torch.argmax's rule), so the token is
    always inside [0, V).  (The parent commit's kernel returned 0x7fffffff for such a row -- every
    comparison with NaN is false -- which the next step's embedding gather would have read at.)  Op
    level only: no engine or model is run on NaN values."""
    gen = torch.Generator().manual_seed(7 * Vn)
    nan = float("nan")
    rows = torch.randn(8, Vn, generator=gen)
    rows[0, 17] = nan                      # one NaN
    rows[1, 0] = nan                       # in column 0
    rows[2, Vn - 1] = nan                  # in the last column
    rows[3, [Vn - 2, 9]] = nan             # two, in different lanes
    rows[4, :] = nan                       # all NaN
    rows[5, 11] = nan
    rows[5, 4] = float("inf")              # NaN beats +inf
    rows[6, 20] = nan
    rows[6, :20] = float("-inf")
    if Vn > 70:
        rows[7, [70, 6]] = nan             # two in one lane
    got = _greedy(rows)
    want = torch.argmax(rows, dim=-1)
    assert int(got.min()) >= 0 and int(got.max()) < Vn, got.tolist()
    assert torch.equal(got, want), (got.tolist(), want.tolist())


# ---------------------------------------------------------------------------------------
# E. sampled engine streams, bf16, stale graphs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,seed", [("small", (4, 32, 64, 2, 2, 1, 60), 4), ("S2", SHAPES["S2"][:7], 12)])
def test_decode_engine_sampled_stream_matches_oracle_draws(name, shape, seed):
    """generate(..., generator=...) through both graphs: every generated (row, column n) token is the
    inverse-CDF token of the oracle's teacher-forced fp64 logits for the Philox draw (seed, stream n,
    row) -- the seed drawn as model.generate draws it, stream = the length at the sample call, which
    is the column written (_step1 / _step2: decode_sample(..., self.len, ...) writes idx[b, len]).
    Gate: the sampler's plus 2 * 1e-5 * max|logit| (the fp32 logits bar through exp); cap 5 %."""
    B, T, C, H, L, L0, new = shape
    m = make_model(T, C, H, L, seed).eval()
    idx = torch.randint(0, V, (B, L0), generator=torch.Generator().manual_seed(seed + 100)).to(DEV)
    gseed = 77
    with torch.no_grad():
        got = m.generate(idx, new, generator=torch.Generator().manual_seed(gseed)).cpu()
    want_seed = int(torch.randint(0, 2 ** 62, (1,), generator=torch.Generator().manual_seed(gseed)))
    assert torch.equal(got[:, :L0], idx.cpu()) and got.shape == (B, L0 + new)
    assert L0 + new > T
    ref = teacher_logits(oracle_params(m), oracle_cfg(T, C, H, L), got, L0, f"sampled-{name}")
    n_gated = n_miss = 0
    for s in range(new):
        lg = ref[:, s, :]
        g = sample_gate(V) + 2 * FP32_BAR * float(lg.abs().max())
        want, gated = expected_sample(lg, want_seed, L0 + s, g)
        tok = got[:, L0 + s].numpy()
        n_gated += int(gated.sum())
        n_miss += int(((tok != want) & ~gated).sum())
    share = n_gated / (B * new)
    print(f"sampled {name}: gated pairs {n_gated} of {B * new} ({100 * share:.2f} %), ungated mismatches {n_miss}")
    assert n_miss == 0
    assert share <= 0.05


def _bf16_check(m, ocfg, got, idx, eng_logits, label, cap):
    """The bf16 bar of test_c2_full_size_bf16_step_matches_oracle on the final step's logits: e_t = the
    error (by norm, against the fp64 oracle) of the oracle's own forward under torch.autocast(bfloat16)
    on the GPU; charpt's must be within bound = max(2e-2, 1.25 e_t).  Teacher-forced tokens: got[b, n]
    has an oracle logit within 2 * bound * max|logit| of the step's maximum, and is the argmax wherever
    the oracle's top-2 gap exceeds that; pairs below the gap at most `cap` (None: printed only)."""
    got = got.cpu()
    B, L0 = idx.shape
    T = ocfg.block_size
    assert torch.equal(got[:, :L0], idx.cpu())
    P = oracle_params(m)
    ref = teacher_logits(P, ocfg, got, L0, label)
    last = ref[:, -1, :]
    Pd = {k: v.float().to(DEV) for k, v in P.items()}
    ctx = got[:, :-1][:, -T:].to(DEV)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        tl, _ = O.forward(Pd, ctx, ocfg)
    e_t = float((tl[:, -1, :].double().cpu() - last).norm() / last.norm())
    e_c = float((eng_logits.double().cpu() - last).norm() / last.norm())
    bound = max(2e-2, 1.25 * e_t)
    print(f"{label}: final-step logits error by norm: charpt {e_c:.4e}, torch autocast e_t {e_t:.4e}, bound {bound:.4e}")
    assert e_c < bound, (label, e_c, e_t)
    gen = got[:, L0:]
    top = ref.topk(2, dim=-1)
    gap = top.values[..., 0] - top.values[..., 1]
    tol = 2 * bound * ref.abs().amax(dim=(0, 2))[None, :]
    chosen = ref.gather(-1, gen.unsqueeze(-1)).squeeze(-1)
    assert bool((top.values[..., 0] - chosen <= tol).all()), f"{label}: a token's oracle logit is outside the bf16 bar"
    clear = gap > tol
    assert bool((gen == top.indices[..., 0])[clear].all()), f"{label}: a clear argmax was missed"
    share = 1.0 - float(clear.double().mean())
    print(f"{label}: pairs below the gap {100 * share:.2f} % of {clear.numel()}")
    if cap is not None:
        assert share <= cap, f"{label}: {100 * share:.1f} % of pairs below the gap (cap {100 * cap:.0f} %)"
    return e_c, e_t


def _c1_prompts(n, length):
    chars = json.load(open(golden_path("tokenizer.json")))["chars"]
    stoi = {c: i for i, c in enumerate(chars)}
    text = open(f"{ROOT}/data/input.txt").read()
    return torch.tensor([[stoi[c] for c in text[100000 * i + 1000:100000 * i + 1000 + length]] for i in range(n)])


def test_decode_engine_bf16_trained_weights_match_oracle():
    """bf16 generate() on the reference-trained C1 weights, 9 sequences (2304 window rows) from nine
    different 250-character prompts of the corpus, 20 new tokens (6 in phase 1, 14 in phase 2): final-step
    logits and teacher-forced tokens to the bf16 bar of _bf16_check; pairs below the gap at most 25 %."""
    from safetensors.torch import load_file
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    sd = load_file(golden_path("model_c1_trained.safetensors"))
    m = BigramLanguageModel(GPTConfig(dtype="bf16"))
    m.load_state_dict(sd, strict=False)
    m = m.to(DEV).eval()
    cfg = m.config
    idx = _c1_prompts(9, 250).to(DEV)
    with torch.no_grad():
        got = m.generate(idx, 20, greedy=True)
    (eng,) = m._decode_engines.values()
    assert got.shape == (9, 270) and 9 * cfg.block_size > 2048
    ocfg = oracle_cfg(cfg.block_size, cfg.n_embd, cfg.n_head, cfg.n_layers)
    _bf16_check(m, ocfg, got, idx, eng.logits, "bf16-c1", 0.25)


@pytest.mark.parametrize("dtype,shape", [("fp32", (3, 64, 96, 4, 3, 5, 90)), ("bf16", (3, 64, 128, 2, 2, 5, 70))])
def test_decode_engine_graphs_follow_new_weights(dtype, shape):
    """load_state_dict of different weights into a model whose engine and graphs are cached, then the
    same shapes again: the replayed graphs read the new weights (bf16: _sync_shadow refreshes the
    operands the graph reads), checked against the oracle on the NEW weights."""
    B, T, C, H, L, L0, new = shape
    m = make_model(T, C, H, L, 31, dtype).eval()
    other = make_model(T, C, H, L, 32, dtype)
    idx = torch.randint(0, V, (B, L0), generator=torch.Generator().manual_seed(33)).to(DEV)
    ocfg = oracle_cfg(T, C, H, L)
    with torch.no_grad():
        first = m.generate(idx, new, greedy=True)
        (eng,) = m._decode_engines.values()
        g1, g2 = eng.g1, eng.g2
        assert g1 is not None and g2 is not None
        m.load_state_dict(other.state_dict())
        got = m.generate(idx, new, greedy=True)
    assert list(m._decode_engines.values()) == [eng] and eng.g1 is g1 and eng.g2 is g2, "the cached graphs were not reused"
    assert not torch.equal(first, got)
    if dtype == "fp32":
        ref = teacher_logits(oracle_params(m), ocfg, got, L0, "stale-fp32")
        check_greedy_fp32(got, idx, ref, eng.logits, "stale-fp32")
    else:
        _bf16_check(m, ocfg, got, idx, eng.logits, "stale-bf16", None)


# ---------------------------------------------------------------------------------------
# F. the row kernels as the engine calls them
# ---------------------------------------------------------------------------------------
def _ln_vectors(K, misaligned):
    """ln_w / ln_b as views into one flat buffer (the engine's are views of the master buffer);
    misaligned: offset by one float, 4-B but not 8-B aligned."""
    flat = torch.randn(2 * K + 64, device=DEV)
    o = 1 if misaligned else 0
    lw, lb = flat[o:o + K], flat[K + 32 + o:2 * K + 32 + o]
    lw.mul_(0.1).add_(1.0)
    lb.mul_(0.1)
    assert lw.data_ptr() % 8 == (4 if misaligned else 0) and lb.data_ptr() % 8 == (4 if misaligned else 0)
    return lw, lb


def _unfused(a_dense, lw, lb, w, kind, bias, resid_dense):
    """layernorm_fwd on dense rows, then ops.gemm with the epilogue `kind` (0 store, 1 bias, 2 bias_relu,
    3 bias_resid)."""
    from replicatinggpt_amd import ops
    M, K = a_dense.shape
    N = w.shape[0]
    a = a_dense
    if lw is not None:
        a = torch.full((M, K), float("nan"), device=DEV)
        ops.layernorm_fwd(a_dense, lw, lb, a, torch.empty(M, device=DEV), torch.empty(M, device=DEV), 1e-5)
    ref = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm(a, w, ref, False, False, False, M, N, K, K, w.stride(0), N, kind, bias, resid_dense,
             N if kind == 3 else 0, None, 0, 0.0, 0, None, 0, 0.0, 1, None)
    return ref


def _fp64_linear(a, lw, lb, w, kind, bias, resid):
    ad = a.double().cpu()
    if lw is not None:
        ad = torch.nn.functional.layer_norm(ad, (ad.shape[1],), lw.double().cpu(), lb.double().cpu(), 1e-5)
    ref = ad @ w.double().cpu().T
    if kind:
        ref = ref + bias.double().cpu()
    if kind == 2:
        ref = torch.relu(ref)
    if kind == 3:
        ref = ref + resid.double().cpu()
    return ref


@pytest.mark.parametrize("ln_mode", ["off", "on", "misaligned"])
@pytest.mark.parametrize("M,T,K", [(33, 5, 126), (2048, 3, 96)])
def test_linear_rows_f32_engine_views(M, T, K, ln_mode):
    """ops.linear_rows_f32 the way decode.py calls it: a = the final rows x[:, T-1, :] of a [M, T, K]
    window (lda = T K), w = the K/V rows wq[K:] and the Q rows wq[:K] of a [3K, K] weight, out and resid
    column slices of wider buffers (ldo, ldr > N), ln_w / ln_b views into a flat buffer; all four
    epilogues: bitwise layernorm_fwd on a dense copy + ops.gemm, and within 1e-5 of fp64.  ln_w / ln_b
    4-B but not 8-B aligned: bitwise the same, or a loud error (never a silently different result)."""
    from replicatinggpt_amd import ops
    ln, misaligned = ln_mode != "off", ln_mode == "misaligned"
    torch.manual_seed(M + K)
    x3 = torch.randn(M, T, K, device=DEV)
    a = x3[:, T - 1, :]
    wq = torch.randn(3 * K, K, device=DEV) / K ** 0.5
    lw, lb = _ln_vectors(K, misaligned) if ln else (None, None)
    assert a.stride(0) == T * K and a.data_ptr() % 8 == 0
    for w in (wq[K:], wq[:K]):
        N = w.shape[0]
        bias_full = torch.randn(N, device=DEV)
        rbuf = torch.randn(M, N + 3, device=DEV)
        resid_v = rbuf[:, :N]
        for kind in (0, 1, 2, 3):
            bias = bias_full if kind else None
            resid = resid_v if kind == 3 else None
            obuf = torch.full((M, N + 5), float("nan"), device=DEV)
            out = obuf[:, :N]
            try:
                ops.linear_rows_f32(a, lw, lb, 1e-5, w, bias, resid, out, kind == 2)
            except (RuntimeError, ValueError) as e:
                assert misaligned and "aligned" in str(e), e
                continue
            torch.cuda.synchronize()
            assert bool(torch.isnan(obuf[:, N:]).all()), "wrote past the N columns of out"
            ref2 = _unfused(a.contiguous(), lw, lb, w, kind, bias, resid.contiguous() if kind == 3 else None)
            torch.cuda.synchronize()
            assert torch.equal(out.contiguous().view(torch.int32), ref2.view(torch.int32)), (N, kind)
            assert relerr(out, _fp64_linear(a, lw, lb, w, kind, bias, resid)) < 1e-5, (N, kind)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("B,T,C,H,Tmax,pos", [(33, 5, 126, 6, 16, 7), (256, 3, 96, 4, 8, 8)])
def test_decode_qkv_f32_engine_views(B, T, C, H, Tmax, pos, misaligned):
    """ops.decode_qkv_f32 with x = the final rows of a [B, T, C] buffer (ldx = T C), qkv a column slice
    of a wider buffer and ln_w / ln_b views into a flat buffer: qkv and both caches bitwise
    layernorm_fwd on a dense copy + ops.gemm + decode_kv_append, qkv within 1e-5 of fp64.  Misaligned
    LayerNorm vectors: bitwise the same, or a loud error."""
    from replicatinggpt_amd import ops
    torch.manual_seed(B + C)
    D = C // H
    x3 = torch.randn(B, T, C, device=DEV)
    x = x3[:, T - 1, :]
    w = torch.randn(3 * C, C, device=DEV) / C ** 0.5
    lw, lb = _ln_vectors(C, misaligned)
    ln = torch.full((1,), pos, dtype=torch.int64, device=DEV)
    kc0 = torch.randn(B, H, Tmax, D, device=DEV)
    vc0 = torch.randn(B, H, Tmax, D, device=DEV)
    kc, vc = kc0.clone(), vc0.clone()
    qbuf = torch.full((B, 3 * C + 5), float("nan"), device=DEV)
    qkv = qbuf[:, :3 * C]
    try:
        ops.decode_qkv_f32(x, lw, lb, 1e-5, w, qkv, ln, kc, vc)
    except (RuntimeError, ValueError) as e:
        assert misaligned and "aligned" in str(e), e
        torch.cuda.synchronize()
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0)
        return
    torch.cuda.synchronize()
    assert bool(torch.isnan(qbuf[:, 3 * C:]).all())
    ref = _unfused(x.contiguous(), lw, lb, w, 0, None, None)
    kr, vr = kc0.clone(), vc0.clone()
    ops.decode_kv_append(ref, C, 2 * C, ln, kr, vr)
    torch.cuda.synchronize()
    assert torch.equal(qkv.contiguous().view(torch.int32), ref.view(torch.int32))
    assert torch.equal(kc.view(torch.int32), kr.view(torch.int32))
    assert torch.equal(vc.view(torch.int32), vr.view(torch.int32))
    assert not torch.equal(kc[:, :, pos - 1], kc0[:, :, pos - 1])
    keep = torch.ones(Tmax, dtype=torch.bool)
    keep[pos - 1] = False
    assert torch.equal(kc[:, :, keep], kc0[:, :, keep]) and torch.equal(vc[:, :, keep], vc0[:, :, keep])
    assert relerr(qkv, _fp64_linear(x, lw, lb, w, 0, None, None)) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [3, 33, 2049])
def test_linear_fwd_bias_resid_strided_residual(M, dtype):
    """functional.linear_fwd(..., "bias_resid") with the residual a row-strided view (the window's
    final rows x[:, T-1, :], as the last block's projection takes it), fp32 and bf16 operands, against
    fp64 of the same operands: 1e-5 (fp32), conftest.bf16_close (bf16)."""
    from replicatinggpt_amd import functional as Fn
    torch.manual_seed(M)
    T, K, N = 4, 126, 126
    x2 = torch.randn(M, K, device=DEV).to(dtype)
    w = (torch.randn(N, K, device=DEV) / K ** 0.5).to(dtype)
    bias = torch.randn(N, device=DEV)
    r3 = torch.randn(M, T, N, device=DEV)
    resid = r3[:, T - 1, :]
    assert resid.stride(0) == T * N
    out = torch.full((M, N), float("nan"), device=DEV)
    Fn.linear_fwd(x2, w, out, "bias_resid", bias=bias, resid=resid)
    torch.cuda.synchronize()
    ref = x2.double().cpu() @ w.double().cpu().T + bias.double().cpu() + resid.double().cpu()
    if dtype == torch.float32:
        assert relerr(out, ref) < 1e-5
    else:
        ok, stats = bf16_close(out, ref)
        assert ok, stats
