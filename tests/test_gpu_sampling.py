"""Temperature / top-k / top-p sampling on the MI355X: ops.decode_sample_filtered
(csrc/decode.hip k_decode_sample_filtered) against the fp64 reference of its contract
(tests/test_cpu_sampling.py::reference, written from include/charpt.h), and the filtered decode
engine behind generate(temperature=, top_k=, top_p=) against the fp64 oracle, teacher-forced.

Every gate comes from the number formats (filtered_gate: the fp32 additions of the two scans, the
exp, the temperature and the two products; for the engine also the project's 1e-5 fp32 logits bar),
never from what the kernel returns; each gated test prints its gated share and fails above its cap."""
import numpy as np
import pytest
import torch

from test_cpu_sampling import filtered_gate, reference
from test_gpu_decode import FP32_BAR, SHAPES, make_model, oracle_cfg, oracle_params, teacher_logits

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 65
PAIRS = [(1, 987654321), (37, 2 ** 61 + 12345)]     # (length, seed): a seed below 2^32 and one with high bits
NEUTRAL = (1.0, 0, 1.0)
SETTINGS = [(0.7, 0, 1.0), (1.5, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95), (1.0, "V", 1.0), (1.0, 0, 0.5),
            (2.0, 3, 0.6)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def _params(tau, k, p):
    from replicatinggpt_amd.sampling import sampling_params
    return sampling_params(tau, k, p).to(DEV)


def _i64(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def run_filtered(lg, setting, seed, length, params=None):
    """One launch on device logits lg [B, V]: the tokens of column `length`; no other column written."""
    from replicatinggpt_amd import ops
    idx = torch.full((lg.shape[0], length + 3), -7, dtype=torch.int64, device=DEV)
    ops.decode_sample_filtered(lg, _params(*setting) if params is None else params, _i64(seed), _i64(length), idx)
    torch.cuda.synchronize()
    out = idx.cpu()
    keep = torch.ones(length + 3, dtype=torch.bool)
    keep[length] = False
    assert bool((out[:, keep] == -7).all()), "a column other than `length` was written"
    tok = out[:, length].numpy()
    assert tok.min() >= 0 and tok.max() < lg.shape[1], (int(tok.min()), int(tok.max()))
    return tok


def run_plain(lg, seed, length):
    from replicatinggpt_amd import ops
    idx = torch.full((lg.shape[0], length + 3), -7, dtype=torch.int64, device=DEV)
    ops.decode_sample(lg, False, _i64(seed), _i64(length), idx)
    torch.cuda.synchronize()
    return idx[:, length].cpu().numpy()


def _logits(Vn, scale, Bn=4096):
    """test_decode_sample_matches_inverse_cdf's rows: scale * randn, dense and as the first V columns
    of rows padded by 7 columns of 50.0 (a kernel reading past V would pick those)."""
    gen = torch.Generator().manual_seed(1000 * Vn + scale)
    logits = scale * torch.randn(Bn, Vn, generator=gen)
    wide = torch.full((Bn, Vn + 7), 50.0)
    wide[:, :Vn] = logits
    views = (("dense", logits.to(DEV)), ("padded", wide.to(DEV)[:, :Vn]))
    assert views[0][1].stride(0) == Vn and views[1][1].stride(0) == Vn + 7
    return logits, views


# ---------------------------------------------------------------------------------------
# 1. neutral settings: bitwise the existing sampler
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("Vn", [1, 2, 64, 65, 66, 200, 1024])
def test_neutral_is_bitwise_decode_sample(Vn, scale):
    """temperature 1, top-k off, top-p off (as 0, as V and above V; p = 1): exactly the tokens
    ops.decode_sample(greedy=False) writes for the same logits, seed, length and rows."""
    _, views = _logits(Vn, scale)
    for length, seed in PAIRS:
        for name, lg in views:
            want = run_plain(lg, seed, length)
            for setting in (NEUTRAL, (1.0, Vn, 1.0), (1.0, Vn + 5, 1.0)):
                got = run_filtered(lg, setting, seed, length)
                assert np.array_equal(got, want), (name, length, seed, setting, int((got != want).sum()))


# ---------------------------------------------------------------------------------------
# 2. exact against the fp64 contract
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("Vn", [1, 2, 3, 64, 65])
def test_filtered_matches_fp64_contract(Vn, scale):
    """4096 rows, eight settings, two (length, seed) pairs, dense and padded rows: every row whose draw
    and whose nucleus threshold are not within the gate of a cumulative boundary gets exactly the
    reference's token.  Gated rows at most 3 % of a case (printed)."""
    logits, views = _logits(Vn, scale)
    g = filtered_gate(Vn)
    for tau, k, p in SETTINGS:
        k = Vn if k == "V" else k
        for length, seed in PAIRS:
            ref = reference(logits, tau, k, p, seed, length, g)
            want, gated = ref["tok"], ref["gated"]
            share = float(gated.mean())
            for name, lg in views:
                tok = run_filtered(lg, (tau, k, p), seed, length)
                miss = (tok != want) & ~gated
                print(f"V={Vn} scale={scale} (t,k,p)=({tau},{k},{p}) len={length} seed={seed} {name}: gated "
                      f"{100 * share:.2f} %, gated rows differing {int(((tok != want) & gated).sum())}, "
                      f"ungated mismatches {int(miss.sum())}")
                assert not miss.any(), (name, tau, k, p, length, seed, int(miss.sum()), int(np.nonzero(miss)[0][0]))
                assert bool(ref["kept"][np.arange(len(tok)), tok][~gated].all())
            assert share <= 0.03, f"V={Vn} scale={scale} ({tau},{k},{p}) len={length}: {100 * share:.2f} % gated (cap 3 %)"


ILL_SETTINGS = [(0.05, 0, 1.0), (20.0, 0, 0.9), (1.0, 0, 0.9), (0.05, 5, 0.5), (20.0, 40, 0.95)]


def ill_scaled_logits(profile, Bn=1024, Vn=V):
    """1024 rows of 3 * randn at V 65: as they are ("unit"), every logit + 1e3 ("offset": the fp32
    logits lose 13 bits below the point, the differences against the row maximum stay exact), or one
    column per row raised 30 above the row maximum ("raised": at tau 0.05 every other weight is
    exp(-600 or less) = 0, at tau 20 the raised column has a fifth of the weight of its row)."""
    gen = torch.Generator().manual_seed(4242)
    x = 3 * torch.randn(Bn, Vn, generator=gen)
    if profile == "offset":
        x = x + 1e3
    elif profile == "raised":
        col = torch.randint(0, Vn, (Bn,), generator=gen)
        x[torch.arange(Bn), col] = x.max(1).values + 30
    elif profile != "unit":
        raise ValueError(profile)
    return x


@pytest.mark.parametrize("profile", ["unit", "offset", "raised"])
def test_filtered_on_ill_scaled_logits(profile):
    """A sharp and a flat temperature (0.05, 20) with and without the cuts, on logits far from zero and
    on rows with one dominant column: every ungated row draws the reference's token; at most 3 % of a
    case's rows are gated (the reference alone gates at most 1.3 % of these on the CPU)."""
    logits = ill_scaled_logits(profile)
    lg = logits.to(DEV)
    g = filtered_gate(V)
    length, seed = 37, 987654321
    for tau, k, p in ILL_SETTINGS:
        ref = reference(logits, tau, k, p, seed, length, g)
        want, gated = ref["tok"], ref["gated"]
        share = float(gated.mean())
        tok = run_filtered(lg, (tau, k, p), seed, length)
        miss = (tok != want) & ~gated
        print(f"{profile} (t,k,p)=({tau},{k},{p}): gated {100 * share:.2f} %, gated rows differing "
              f"{int(((tok != want) & gated).sum())}, ungated mismatches {int(miss.sum())}")
        assert not miss.any(), (profile, tau, k, p, int(miss.sum()), int(np.nonzero(miss)[0][0]))
        assert bool(ref["kept"][np.arange(len(tok)), tok][~gated].all())
        assert share <= 0.03, f"{profile} ({tau},{k},{p}): {100 * share:.2f} % gated (cap 3 %)"


# ---------------------------------------------------------------------------------------
# 3. degenerate settings are greedy
# ---------------------------------------------------------------------------------------
def _tie_rows(Vn):
    """randn rows, then rows whose maximum is duplicated: in another lane, in a later 64-column pass of
    the same lane, in adjacent columns, at both ends, everywhere."""
    gen = torch.Generator().manual_seed(3 * Vn)
    x = torch.randn(512, Vn, generator=gen) * 3
    x[0, [0, Vn - 1]] = 9.0
    x[1, :] = 0.25
    x[2, [Vn - 1, Vn // 2]] = 9.0
    x[3, [Vn // 2, Vn // 2 - 1]] = 9.0
    if Vn > 70:
        x[4, [6, 70]] = 9.0                    # one lane of a 64-lane strided loop, two passes
        x[5, [70, 3]] = 9.0
        x[6, [6, 70, 67]] = 9.0
    if Vn > 300:
        x[7, [261, 5]] = 9.0                   # one thread of a 256-thread strided loop, two passes
        x[8, [5 + 256, 5 + 512, 5 + 768]] = 9.0
        x[9, [Vn - 1, Vn - 257]] = 9.0
    x[10, :] = float("-inf")
    x[10, Vn - 1] = -2.0
    return x


@pytest.mark.parametrize("Vn", [2, 65, 200, 1024])
def test_degenerate_settings_are_greedy(Vn):
    """top_k = 1, and a top_p the top token alone reaches (1e-9), give torch.argmax for every row and
    every draw, at two temperatures."""
    x = _tie_rows(Vn)
    want = torch.argmax(x, dim=-1).numpy()
    lg = x.to(DEV)
    for setting in ((1.0, 1, 1.0), (1.0, 0, 1e-9), (0.5, 1, 0.3), (3.0, 0, 1e-9), (1.0, 1, 1e-9)):
        for length, seed in PAIRS:
            got = run_filtered(lg, setting, seed, length)
            assert np.array_equal(got, want), (setting, length, np.nonzero(got != want)[0][:5].tolist())


# ---------------------------------------------------------------------------------------
# 4. support at large V, without gating
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("Vn", [130, 200, 1024])
def test_support_at_large_vocabularies(Vn, scale):
    """Every token is in the exact top-k set (ranked on the raw logits: no rounding in it), and with
    top-p the cumulative weight of the ranks before the token's is below p S_k + g S_k."""
    logits, views = _logits(Vn, scale, Bn=2048)
    g = filtered_gate(Vn)
    rows = np.arange(logits.shape[0])
    for tau, k, p in ((1.0, 5, 1.0), (0.8, 40, 0.95), (1.0, 0, 0.5)):
        ref = reference(logits, tau, k, p)
        kk = k if k else Vn
        before = np.concatenate([np.zeros((len(rows), 1)), ref["cum_rank"][:, :-1]], axis=1)
        for length, seed in PAIRS:
            for name, lg in views:
                tok = run_filtered(lg, (tau, k, p), seed, length)
                rk = ref["rank"][rows, tok]
                assert bool((rk < kk).all()), (name, tau, k, p, int((rk >= kk).sum()))
                if p < 1:
                    ahead = before[rows, rk]
                    assert bool((ahead < (p + g) * ref["S_k"]).all()), (name, tau, k, p)


# ---------------------------------------------------------------------------------------
# 5. special values
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Vn", [65, 200])
def test_minus_infinity_logits_are_never_drawn(Vn):
    """Rows with -inf entries -- the last column, a whole 64-column pass, every other column: an
    ungated row gets the reference's token, which is never a -inf one."""
    gen = torch.Generator().manual_seed(9 * Vn)
    x = torch.randn(1024, Vn, generator=gen) * 2
    ninf = float("-inf")
    x[0::4, Vn - 1] = ninf
    x[1::4, :64] = ninf                      # a whole pass: only columns 64.. remain
    x[2::4, 1::2] = ninf
    x[3::8, 64:] = ninf
    lg = x.to(DEV)
    g = filtered_gate(Vn)
    for setting in (NEUTRAL, (0.7, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95)):
        for length, seed in PAIRS:
            ref = reference(x, *setting, seed, length, g)
            tok = run_filtered(lg, setting, seed, length)
            ok = ~ref["gated"]
            assert np.array_equal(tok[ok], ref["tok"][ok]), setting
            drawn = x.numpy()[np.arange(len(tok)), tok]
            assert bool(np.isfinite(drawn[ok]).all()), setting
            # no cap here: flat V = 200 rows under top-p gate several per cent in the reference alone
            # (many near-equal rank boundaries); the check must still cover most rows
            print(f"V={Vn} {setting} len={length}: gated {100 * float(ref['gated'].mean()):.2f} %")
            assert float(ref["gated"].mean()) < 0.5


@pytest.mark.parametrize("Vn", [100, 40])
def test_nan_and_infinite_rows_give_the_greedy_token(Vn):
    """Rows built like test_decode_sample_greedy_nan_rows, plus +inf rows: the greedy rule's token (the
    first NaN, else the first +inf) under every setting, always inside [0, V)."""
    gen = torch.Generator().manual_seed(7 * Vn)
    nan, inf = float("nan"), float("inf")
    rows = torch.randn(12, Vn, generator=gen)
    rows[0, 17] = nan
    rows[1, 0] = nan
    rows[2, Vn - 1] = nan
    rows[3, [Vn - 2, 9]] = nan
    rows[4, :] = nan
    rows[5, 11] = nan
    rows[5, 4] = inf
    rows[6, 20] = nan
    rows[6, :20] = -inf
    rows[7, [70, 6] if Vn > 70 else [Vn - 1, 6]] = nan      # V > 70: two NaN in one lane of a 64-lane pass
    rows[8, 13] = inf
    rows[9, [Vn - 1, 2]] = inf
    rows[10, :] = inf
    rows[11, 5] = inf
    rows[11, :5] = -inf
    want = torch.argmax(rows, dim=-1).numpy()
    lg = rows.to(DEV)
    for setting in (NEUTRAL, (0.7, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95), (1.0, 1, 1.0)):
        for length, seed in PAIRS:
            got = run_filtered(lg, setting, seed, length)
            assert np.array_equal(got, want), (setting, got.tolist(), want.tolist())


def test_vocabulary_above_the_limit_is_an_error():
    from replicatinggpt_amd import ops
    lg = torch.randn(2, 1025, device=DEV)
    idx = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="1024"):
        ops.decode_sample_filtered(lg, _params(*NEUTRAL), _i64(1), _i64(1), idx)
    torch.cuda.synchronize()
    assert int(idx.abs().sum()) == 0


# ---------------------------------------------------------------------------------------
# 6. the settings are read on the device when the kernel runs
# ---------------------------------------------------------------------------------------
def test_params_are_read_at_run_time_and_opcheck():
    """Two launches on the same buffers that differ only in what the params tensor holds: each gets its
    own setting's reference tokens -- through a captured graph too, replayed after the params change."""
    from replicatinggpt_amd import ops
    logits, views = _logits(65, 1, Bn=1024)
    lg = views[0][1]
    length, seed = PAIRS[0]
    g = filtered_gate(65)
    params = _params(*NEUTRAL)
    seed_t, len_t = _i64(seed), _i64(length)
    idx = torch.zeros((1024, length + 1), dtype=torch.int64, device=DEV)
    settings = [(1.0, 1, 1.0), (0.8, 10, 0.9), (1.0, 1, 1.0), (1.5, 0, 0.7)]
    toks = []
    for s in settings:
        params.copy_(_params(*s))
        toks.append(run_filtered(lg, None, seed, length, params=params))
    # one captured launch, replayed under each setting
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.decode_sample_filtered(lg, params, seed_t, len_t, idx)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.decode_sample_filtered(lg, params, seed_t, len_t, idx)
    for s, tok in zip(settings, toks):
        ref = reference(logits, *s, seed, length, g)
        ok = ~ref["gated"]
        assert np.array_equal(tok[ok], ref["tok"][ok]), s
        params.copy_(_params(*s))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(idx[:, length].cpu().numpy(), tok), s
    assert np.array_equal(toks[0], toks[2]) and not np.array_equal(toks[0], toks[1])
    assert not np.array_equal(toks[1], toks[3])
    torch.library.opcheck(ops.decode_sample_filtered, (lg, params, seed_t, len_t, idx))


# ---------------------------------------------------------------------------------------
# 7. the engine
# ---------------------------------------------------------------------------------------
ENGINE_SHAPES = [("small", (4, 32, 64, 2, 2, 1, 60), 4), ("S2", SHAPES["S2"][:7], 12)]
_MODELS = {}


def _model(name, shape, seed, dtype="fp32"):
    key = (name, dtype)
    if key not in _MODELS:
        B, T, C, H, L, L0, new = shape
        m = make_model(T, C, H, L, seed, dtype).eval()
        idx = torch.randint(0, V, (B, L0), generator=torch.Generator().manual_seed(seed + 100)).to(DEV)
        _MODELS[key] = (m, idx)
    return _MODELS[key]


def _gen(m, idx, new, gseed=77, **kw):
    # the engine takes its seed from a CPU generator; the literal loop's torch.multinomial draws on the device
    gen = torch.Generator(device=DEV if kw.get("engine") is False else "cpu").manual_seed(gseed)
    with torch.no_grad():
        out = m.generate(idx, new, generator=gen, **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("name,shape,seed", ENGINE_SHAPES)
def test_engine_top_k_1_is_greedy_and_neutral_is_unchanged(name, shape, seed):
    """(a) generate(top_k=1) is generate(greedy=True) exactly; (b) neutral keyword values are the call
    without them (same generator seed, same engine); (e) the prompt columns stay."""
    B, T, C, H, L, L0, new = shape
    m, idx = _model(name, shape, seed)
    assert L0 + new > T
    greedy = _gen(m, idx, new, greedy=True)
    k1 = _gen(m, idx, new, top_k=1)
    assert torch.equal(k1, greedy)
    assert torch.equal(k1[:, :L0], idx.cpu()) and k1.shape == (B, L0 + new)
    assert torch.equal(_gen(m, idx, new, top_p=1e-9, temperature=0.3), greedy)
    plain = _gen(m, idx, new)
    n_eng = len(m._decode_engines)
    assert torch.equal(_gen(m, idx, new, temperature=1.0, top_k=None, top_p=1.0), plain)
    assert torch.equal(_gen(m, idx, new, temperature=1, top_k=0, top_p=1), plain)
    assert len(m._decode_engines) == n_eng, "neutral keyword values built another engine"
    assert not torch.equal(plain, greedy)
    flt = [e for e in m._decode_engines.values() if e.filtered]
    assert len(flt) == 1 and sum(not e.filtered for e in m._decode_engines.values()) == 2


@pytest.mark.parametrize("name,shape,seed", ENGINE_SHAPES)
def test_engine_filtered_stream_matches_oracle_draws(name, shape, seed):
    """(c) generate(temperature=0.8, top_k=10, top_p=0.9) through both graphs: every generated (row,
    column n) token is the contract's token of the oracle's teacher-forced fp64 logits for the draw
    (seed, n, row).  Gate: the sampler's plus 2 * 1e-5 * max|logit| / temperature (the fp32 logits bar
    through the exp), and pairs whose k-th and (k+1)-th oracle logits are closer than 2 * 1e-5 *
    max|logit| (either could be the k-th on the device); cap 5 %.  (d) another setting replays the
    same graph objects, and a repeated call reproduces its stream.  (e) the prompt stays."""
    B, T, C, H, L, L0, new = shape
    tau, k, p = 0.8, 10, 0.9
    m, idx = _model(name, shape, seed)
    gseed = 78
    got = _gen(m, idx, new, gseed, temperature=tau, top_k=k, top_p=p)
    want_seed = int(torch.randint(0, 2 ** 62, (1,), generator=torch.Generator().manual_seed(gseed)))
    assert torch.equal(got[:, :L0], idx.cpu()) and got.shape == (B, L0 + new)
    ref = teacher_logits(oracle_params(m), oracle_cfg(T, C, H, L), got, L0, f"filtered-{name}")
    n_gated = n_miss = 0
    for s in range(new):
        lg = ref[:, s, :]
        amax = float(lg.abs().max())
        g = filtered_gate(V) + 2 * FP32_BAR * amax / tau
        r = reference(lg, tau, k, p, want_seed, L0 + s, g)
        srt = np.take_along_axis(lg.numpy(), r["order"], axis=1)
        gated = r["gated"] | (srt[:, k - 1] - srt[:, k] < 2 * FP32_BAR * amax)
        tok = got[:, L0 + s].numpy()
        n_gated += int(gated.sum())
        n_miss += int(((tok != r["tok"]) & ~gated).sum())
    share = n_gated / (B * new)
    print(f"filtered {name}: gated pairs {n_gated} of {B * new} ({100 * share:.2f} %), ungated mismatches {n_miss}")
    assert n_miss == 0
    assert share <= 0.05
    # (d) the same graphs serve another setting; the same call reproduces its stream
    (eng,) = [e for e in m._decode_engines.values() if e.filtered]
    graphs = (eng.g1, eng.g1_prefill, eng.g2)
    assert all(gr is not None for gr in graphs)
    other = _gen(m, idx, new, gseed, temperature=1.3, top_k=3, top_p=0.7)
    assert (eng.g1, eng.g1_prefill, eng.g2) == graphs and all(a is b for a, b in zip((eng.g1, eng.g1_prefill, eng.g2), graphs))
    assert [e for e in m._decode_engines.values() if e.filtered] == [eng], "a new setting built another engine"
    assert not torch.equal(other, got) and torch.equal(other[:, :L0], idx.cpu())
    assert eng.params.cpu().tolist() == pytest.approx([1.3, 3.0, 0.7])
    assert torch.equal(_gen(m, idx, new, gseed, temperature=tau, top_k=k, top_p=p), got)
    assert (eng.g1, eng.g1_prefill, eng.g2) == graphs


def test_engine_bf16_filtered_tokens_in_range():
    """(f) a bf16 model runs filtered generation through both graphs (the logits are fp32 on both
    paths); tokens inside the vocabulary, the prompt kept, top_k = 1 the greedy stream."""
    name, shape, seed = ENGINE_SHAPES[0]
    B, T, C, H, L, L0, new = shape
    m, idx = _model(name, shape, seed, "bf16")
    got = _gen(m, idx, new, temperature=0.8, top_k=10, top_p=0.9)
    assert got.shape == (B, L0 + new) and torch.equal(got[:, :L0], idx.cpu())
    assert int(got.min()) >= 0 and int(got.max()) < V
    assert torch.equal(_gen(m, idx, new, top_k=1), _gen(m, idx, new, greedy=True))


# ---------------------------------------------------------------------------------------
# 8. the literal loop
# ---------------------------------------------------------------------------------------
def test_literal_loop_top_k_1_is_greedy():
    """engine=False applies sampling.filter_logits before softmax / multinomial: top_k = 1 leaves one
    token whatever the multinomial draw, so the stream is the literal loop's greedy one."""
    name, shape, seed = ENGINE_SHAPES[0]
    B, T, C, H, L, L0, new = shape
    m, idx = _model(name, shape, seed)
    lit = _gen(m, idx, new, engine=False, top_k=1)
    assert lit.shape == (B, L0 + new) and torch.equal(lit[:, :L0], idx.cpu())
    assert torch.equal(lit, _gen(m, idx, new, engine=False, greedy=True))
    out = _gen(m, idx, 8, engine=False, temperature=0.8, top_k=10, top_p=0.9)
    assert out.shape == (B, L0 + 8) and int(out.min()) >= 0 and int(out.max()) < V
