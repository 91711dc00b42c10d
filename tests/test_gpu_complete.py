"""BigramLanguageModel.complete / score on the MI355X: ragged prompts in lock step, stop tokens, the
per-row budget and per-token log-probabilities (decode.py's ragged mode, csrc/decode.hip
k_decode_emit) against the fp64 CPU oracle run on each row alone, against generate() for equal
prompts, against a plain DecodeEngine for the sampled stream, and ops.decode_emit on crafted logits
against the two existing samplers.

Token checks are exact: along every oracle stream used here the smallest top-2 logit gap is at least
6.1e-4 of that step's max |logit| (R1; 1.0e-2 for R2; 8.7e-3 for the stop test's rebuilt row 2), the
project's fp32 logits bar moves a gap by at most 2e-5, so no pair is near a tie.  The log-prob
bounds are derived in the tests that use them, from the number formats only."""
import math

import pytest
import torch

from oracle import gpt1_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 65
PAD = 7
FP32_BAR = 1e-5     # relative to the largest logit: test_gpu_model.py::test_model_fp32_matches_reference
LOGPROB_ABS = 1e-4  # the kernel's own error: see test_decode_emit_kernel


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


# ---------------------------------------------------------------------------------------
# models, prompts, oracle streams (computed once per case, never modified)
# ---------------------------------------------------------------------------------------
def make_model(T, C, H, L, seed, dtype="fp32"):
    """tests/test_gpu_decode.py::make_model: seeded random init with the LayerNorm weights / biases moved
    off 1 / 0 (the init would hide a kernel that dropped or misread them)."""
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    torch.manual_seed(seed)
    m = BigramLanguageModel(GPTConfig(block_size=T, n_embd=C, n_head=H, n_layers=L, dropout=0.0, dtype=dtype))
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if ".ln1." in name or ".ln2." in name or name.startswith("ln_f."):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m.to(DEV)


# name: (T, C, H, L, model seed, prompt seed, prompt matrix shape, prompt lengths, max_new_tokens)
CASES = {
    "R1": (64, 96, 4, 3, 21, 121, (6, 70), (1, 5, 17, 40, 64, 70), 40),
    "R2": (128, 128, 2, 2, 22, 122, (3, 128), (100, 120, 128), 12),
}
_CASE = {}
_STREAM = {}


def case(name):
    """(model in eval mode, oracle parameters, oracle config, prompts as a list of CPU rows, lengths, new)."""
    if name not in _CASE:
        T, C, H, L, seed, pseed, shape, P, new = CASES[name]
        m = make_model(T, C, H, L, seed).eval()
        par = {k: v.double().cpu() for k, v in m.state_dict().items() if "tril" not in k}
        ocfg = O.OracleConfig(block_size=T, n_embd=C, n_head=H, n_layers=L, dropout=0.0)
        base = torch.randint(0, V, shape, generator=torch.Generator().manual_seed(pseed))
        prompts = [base[b, :p].clone() for b, p in enumerate(P)]
        _CASE[name] = (m, par, ocfg, prompts, P, new)
    return _CASE[name]


def oracle_stream(name, b, prompt=None, tag=""):
    """generate_greedy of row b alone (its own prompt, or the given one): [P_b + new] tokens."""
    key = (name, b, tag)
    if key not in _STREAM:
        m, par, ocfg, prompts, P, new = case(name)
        pr = prompts[b] if prompt is None else prompt
        _STREAM[key] = O.generate_greedy(par, pr[None, :], ocfg, new)[0]
    return _STREAM[key]


def run_complete(m, prompts, new, **kw):
    with torch.no_grad():
        out = m.complete(prompts, new, **kw)
    torch.cuda.synchronize()
    return out


def check_rows_against(out, streams, P, new, lengths=None):
    """tokens[b, :len_b] == the stream's, pad after, prompt columns kept, lengths as expected."""
    tokens, got_len = out.tokens.cpu(), out.lengths.cpu()
    assert tokens.shape == (len(P), max(P) + new) and tokens.dtype == torch.int64
    for b, p in enumerate(P):
        want_len = p + new if lengths is None else lengths[b]
        assert int(got_len[b]) == want_len, (b, int(got_len[b]), want_len)
        assert torch.equal(tokens[b, :p], streams[b][:p]), f"row {b}: prompt columns changed"
        diff = (tokens[b, :want_len] != streams[b][:want_len]).nonzero()
        assert diff.numel() == 0, f"row {b}: first difference from the oracle at column {int(diff[0])}"
        assert bool((tokens[b, want_len:] == PAD).all()), f"row {b}: columns past its length are not pad"


# ---------------------------------------------------------------------------------------
# 1. ragged greedy against the oracle, row by row
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R1", "R2"])
def test_ragged_greedy_matches_oracle_per_row(name):
    """Every row of the ragged batch is the oracle's greedy stream of that row run alone -- rows ending
    in phase 1, crossing into the window phase, a prompt of exactly the window and a longer one."""
    m, par, ocfg, prompts, P, new = case(name)
    streams = [oracle_stream(name, b) for b in range(len(P))]
    out = run_complete(m, prompts, new, greedy=True, pad_token=PAD)
    check_rows_against(out, streams, P, new)
    assert out.logprobs is None
    assert out.steps == max(P) + new - min(P)        # head steps from column min(P): no row stops early
    (eng,) = [e for e in m._complete_engines.values() if e.logprob is None and e.max_len == max(P) + new]
    n_eng = len(m._complete_engines)
    assert eng.ragged and all(g is not None for g in eng.rg[0]) and eng.g1_prefill is not None
    assert not m.__dict__.get("_decode_engines"), "complete() must not touch generate()'s engine cache"
    # the (idx, lens) form of the same prompts, with junk past each row's length
    idx = torch.full((len(P), max(P) + 3), 11, dtype=torch.int64)
    for b, p in enumerate(P):
        idx[b, :p] = prompts[b]
    again = run_complete(m, (idx.to(DEV), torch.tensor(P)), new, greedy=True, pad_token=PAD)
    assert again.tokens.shape[1] == max(P) + new
    assert torch.equal(again.tokens, out.tokens) and torch.equal(again.lengths, out.lengths)
    assert len(m._complete_engines) == n_eng, "the same shape built another engine"


def test_ragged_greedy_without_graphs():
    """R1 on an engine built with use_graph=False: the same tokens as the captured graphs give."""
    from replicatinggpt_amd.completion import Completion, pack_prompts
    from replicatinggpt_amd.decode import DecodeEngine
    m, par, ocfg, prompts, P, new = case("R1")
    streams = [oracle_stream("R1", b) for b in range(len(P))]
    idx, lens = pack_prompts(prompts)
    eng = DecodeEngine(m, len(P), max(P) + new, ragged=True, use_graph=False)
    tokens, lengths, logprobs, steps = eng.complete(idx.to(DEV), lens, new, mode=0, pad=PAD)
    torch.cuda.synchronize()
    assert not eng.rg and eng.g1_prefill is None and logprobs is None
    check_rows_against(Completion(tokens, lengths, logprobs, steps), streams, P, new)
    graphed = run_complete(m, prompts, new, greedy=True, pad_token=PAD)
    assert torch.equal(graphed.tokens, tokens)


# ---------------------------------------------------------------------------------------
# 2. equal prompts: generate(), bit for bit
# ---------------------------------------------------------------------------------------
_EQ = {}
MODES = {"greedy": dict(greedy=True), "sampled": {}, "filtered": dict(temperature=0.8, top_k=20, top_p=0.9)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_equal_prompts_reproduce_generate(dtype, mode):
    """B = 4 rows of one length, ending in phase 2: complete() and generate() with the same generator
    seed write the same tokens."""
    B, L0, new = 4, 5, 90
    if dtype not in _EQ:
        m = make_model(64, 96, 4, 3, 11, dtype).eval()
        idx = torch.randint(0, V, (B, L0), generator=torch.Generator().manual_seed(111)).to(DEV)
        _EQ[dtype] = (m, idx)
    m, idx = _EQ[dtype]
    kw = MODES[mode]
    with torch.no_grad():
        want = m.generate(idx, new, generator=torch.Generator().manual_seed(77), **kw)
    out = run_complete(m, (idx, torch.full((B,), L0)), new, generator=torch.Generator().manual_seed(77), **kw)
    assert want.shape == (B, L0 + new)
    assert torch.equal(out.tokens, want)
    assert out.lengths.tolist() == [L0 + new] * B and out.steps == new
    if mode != "greedy":
        other = run_complete(m, (idx, torch.full((B,), L0)), new, generator=torch.Generator().manual_seed(78), **kw)
        assert not torch.equal(other.tokens, want)


# ---------------------------------------------------------------------------------------
# 3. the sampled stream of a row does not depend on its batch-mates
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sampled", "filtered"])
def test_sampled_rows_are_independent_of_batch_mates(mode):
    """Row b of the ragged R1 batch against a plain DecodeEngine (no graphs) whose six rows all hold
    prompt b, run with the seed complete() drew: the same tokens in row b over [P_b, P_b + 40)."""
    from replicatinggpt_amd.decode import DecodeEngine
    m, par, ocfg, prompts, P, new = case("R1")
    kw = MODES[mode]
    out = run_complete(m, prompts, new, generator=torch.Generator().manual_seed(91), pad_token=PAD, **kw)
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=torch.Generator().manual_seed(91)))
    assert out.lengths.tolist() == [p + new for p in P]
    for b in (0, 2, 5):
        p = P[b]
        eng = DecodeEngine(m, len(P), p + new, greedy=False, use_graph=False, filtered=mode == "filtered")
        idx = prompts[b][None, :].repeat(len(P), 1).to(DEV)
        sampling = (kw["temperature"], kw["top_k"], kw["top_p"]) if mode == "filtered" else None
        with torch.no_grad():
            alone = eng.generate(idx, new, seed=seed, sampling=sampling)
        torch.cuda.synchronize()
        assert torch.equal(out.tokens[b, :p].cpu(), prompts[b])
        assert torch.equal(out.tokens[b, p:p + new], alone[b, p:]), f"{mode}: row {b} depends on its batch-mates"


# ---------------------------------------------------------------------------------------
# 4. stop tokens
# ---------------------------------------------------------------------------------------
STOP = 46


def test_stop_tokens_end_rows():
    """Greedy R1 with stop set {46}: a row ends with its first generated 46 (kept), pad follows; a 46
    inside a prompt (row 2's, put there) ends nothing.  Expected lengths come from the oracle's streams."""
    m, par, ocfg, prompts, P, new = case("R1")
    prompts = [p.clone() for p in prompts]
    prompts[2][8] = STOP
    streams = [oracle_stream("R1", b) for b in range(len(P))]
    streams[2] = oracle_stream("R1", 2, prompt=prompts[2], tag="stop46")
    lengths = []
    for b, p in enumerate(P):
        hit = (streams[b][p:] == STOP).nonzero()
        lengths.append(p + int(hit[0]) + 1 if hit.numel() else p + new)
    print("stop test: expected lengths", lengths, "of", [p + new for p in P])
    assert sum(l < p + new for l, p in zip(lengths, P)) >= 3 and lengths[2] > P[2] and STOP in prompts[2].tolist()
    out = run_complete(m, prompts, new, greedy=True, pad_token=PAD, stop_tokens=[STOP])
    check_rows_against(out, streams, P, new, lengths)
    for b, l in enumerate(lengths):
        if l < P[b] + new:
            assert int(out.tokens[b, l - 1]) == STOP


def test_every_token_stops_and_the_poll_ends_the_run():
    """stop_tokens = the whole vocabulary, poll_every = 1: every row ends with its first generated token,
    and the run stops after the step that decides column max(P) instead of after the last column."""
    m, par, ocfg, prompts, P, new = case("R1")
    streams = [oracle_stream("R1", b) for b in range(len(P))]
    out = run_complete(m, prompts, new, greedy=True, pad_token=PAD, stop_tokens=range(V), poll_every=1)
    check_rows_against(out, streams, P, new, [p + 1 for p in P])
    assert out.steps == max(P) - min(P) + 1          # columns min(P) .. max(P)
    assert out.steps < max(P) + new - min(P)         # the full run's
    never = run_complete(m, prompts, new, greedy=True, pad_token=PAD, stop_tokens=range(V), poll_every=0)
    assert never.steps == max(P) + new - min(P)
    assert torch.equal(never.tokens, out.tokens) and torch.equal(never.lengths, out.lengths)


# ---------------------------------------------------------------------------------------
# 5. the kernel on crafted logits
# ---------------------------------------------------------------------------------------
def _i64(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("Vn", [1, 2, 64, 65, 200, 1024])
def test_decode_emit_kernel(Vn, mode):
    """ops.decode_emit on logits uniform in [-20, 20], 160 rows cycling through five states (ended,
    forced, forced with its limit at this column, emitted, emitted with its limit at this column),
    the last ten rows holding NaN / +inf.  Emitted tokens equal ops.decode_sample /
    ops.decode_sample_filtered on the same inputs; only column n of idx / logprob is written.

    Log-prob bound 1e-4 absolute against log_softmax in fp64, derived: a worst-case sequential fp32
    sum of V = 1024 terms errs by V * 2^-24 = 6.1e-5 relative, the same absolute error in its log;
    the roundings of x - m, of the exponent argument and of the final subtraction at magnitude <= 47
    (40 + log 1024) add a few 1e-6."""
    from replicatinggpt_amd import ops
    from replicatinggpt_amd.completion import stop_words
    from replicatinggpt_amd.sampling import sampling_params
    Bn, n, width, seed = 160, 5, 9, 2 ** 61 + 12345
    gen = torch.Generator().manual_seed(50 * Vn + mode)
    x = torch.rand(Bn, Vn, generator=gen) * 40 - 20
    nan, inf = float("nan"), float("inf")
    special = torch.arange(Bn - 10, Bn)
    x[Bn - 10, Vn // 2] = nan
    x[Bn - 9, 0] = nan
    x[Bn - 8, Vn - 1] = inf
    x[Bn - 7, :] = nan
    x[Bn - 6, [0, Vn - 1]] = inf
    x[Bn - 5, Vn // 3] = inf
    x[Bn - 4, Vn - 1] = nan
    x[Bn - 3, :] = inf
    x[Bn - 2, Vn // 2] = inf
    x[Bn - 1, Vn // 2] = nan
    wide = torch.full((Bn, Vn + 3), 50.0)
    wide[:, :Vn] = x
    lg = wide.to(DEV)[:, :Vn]                      # row stride V + 3: a kernel reading past V would see 50
    state = torch.arange(Bn) % 5                   # 0 ended, 1 forced, 2 forced at its limit, 3 emitted, 4 emitted at its limit
    state[special] = torch.tensor([3, 3, 3, 3, 4, 1, 1, 2, 3, 4])
    prompt_len = torch.where((state == 1) | (state == 2), torch.tensor(n + 1), torch.tensor(3))
    prompt_len[state == 1] += torch.arange(int((state == 1).sum())) % 3
    limit = prompt_len + 4
    limit[state == 2] = n + 1
    limit[state == 4] = n + 1
    end0 = torch.where(state == 0, torch.tensor(4), torch.tensor(0))
    params = sampling_params(0.8, 20, 0.9).to(DEV)
    seed_t, len_t = _i64(seed), _i64(n)
    # what the existing samplers write for these logits
    ref_idx = torch.full((Bn, width), -7, dtype=torch.int64, device=DEV)
    if mode == 2:
        ops.decode_sample_filtered(lg, params, seed_t, len_t, ref_idx)
    else:
        ops.decode_sample(lg, mode == 0, seed_t, len_t, ref_idx)
    want_tok = ref_idx[:, n].cpu()
    assert int(want_tok.min()) >= 0 and int(want_tok.max()) < Vn
    if mode != 1:   # the greedy rule on NaN / +inf rows is the contract of modes 0 and 2; mode 1 is whatever decode_sample draws
        assert torch.equal(want_tok[special], torch.argmax(x[special], dim=-1))
    # stop set: the tokens of every fourth emitted row, plus token 63 / 127 (bit 63 of a word) where they exist
    emitted = (state == 3) | (state == 4)
    if Vn <= 2:
        stop = {0}
    else:
        stop = set(want_tok[emitted][::4].tolist()) | {t for t in (63, 127) if t < Vn}
        stop.discard(int(want_tok[3]))             # row 3's token stops nothing
    words = stop_words(sorted(stop), Vn)
    assert words.numel() == (Vn + 63) // 64
    idx0 = torch.randint(0, Vn, (Bn, width), generator=torch.Generator().manual_seed(7))
    idx = idx0.to(DEV)
    lp = torch.full((Bn, width), -3.0, device=DEV)
    end = end0.to(DEV)
    ops.decode_emit(lg, mode, params if mode == 2 else None, seed_t, len_t, prompt_len.to(DEV), limit.to(DEV), end,
                    words.to(DEV), _i64(PAD), idx, lp)
    torch.cuda.synchronize()
    got, got_lp, got_end = idx.cpu(), lp.cpu(), end.cpu()
    other = torch.ones(width, dtype=torch.bool)
    other[n] = False
    assert torch.equal(got[:, other], idx0[:, other]) and bool((got_lp[:, other] == -3.0).all()), "a column other than n was written"
    forced = (state == 1) | (state == 2)
    tok = torch.where(forced, idx0[:, n], want_tok)
    assert torch.equal(got[forced, n], idx0[forced, n]), "a forced row's token was overwritten"
    assert torch.equal(got[emitted, n], want_tok[emitted]), "an emitted token differs from the sampler's"
    assert bool((got[state == 0, n] == PAD).all()) and bool((got_lp[state == 0, n] == 0).all())
    stop_t = torch.tensor(sorted(stop), dtype=torch.int64)
    hit = emitted & torch.isin(tok, stop_t)
    want_end = torch.where(hit | (limit == n + 1), torch.tensor(n + 1), torch.tensor(0))
    want_end[state == 0] = 4
    assert torch.equal(got_end, want_end), (got_end - want_end).nonzero().flatten().tolist()[:8]
    assert int(hit.sum()) > 0 and (Vn == 1 or int((emitted & ~hit & (state == 3)).sum()) > 0)
    # log-probs
    live = state != 0
    clean = live.clone()
    clean[special] = False
    ref = torch.log_softmax(x.double(), dim=-1)[torch.arange(Bn), tok.clamp(0, Vn - 1)]
    err = (got_lp[:, n].double() - ref)[clean].abs().max()
    print(f"V={Vn} mode={mode}: max |log-prob - fp64| {float(err):.3e} (bound {LOGPROB_ABS:.0e})")
    assert float(err) <= LOGPROB_ABS
    assert bool(torch.isnan(got_lp[special, n]).all()), "a NaN / +inf row must give a NaN log-prob"
    # without a log-prob buffer: the same tokens and ends, nothing else
    idx2, end2 = idx0.to(DEV), end0.to(DEV)
    ops.decode_emit(lg, mode, params, seed_t, len_t, prompt_len.to(DEV), limit.to(DEV), end2, words.to(DEV), _i64(PAD),
                    idx2, None)
    torch.cuda.synchronize()
    assert torch.equal(idx2.cpu(), got) and torch.equal(end2.cpu(), got_end)


def test_decode_emit_forced_token_outside_vocabulary_reads_nothing():
    from replicatinggpt_amd import ops
    x = torch.zeros(2, 65, device=DEV)
    idx = torch.tensor([[3, 10 ** 12, 0], [3, -4, 0]], dtype=torch.int64, device=DEV)
    lp = torch.zeros((2, 3), device=DEV)
    end = torch.zeros(2, dtype=torch.int64, device=DEV)
    full = torch.full((2,), 3, dtype=torch.int64, device=DEV)
    ops.decode_emit(x, 0, None, _i64(1), _i64(1), full, full, end, torch.zeros(2, dtype=torch.int64, device=DEV),
                    _i64(PAD), idx, lp)
    torch.cuda.synchronize()
    assert bool(torch.isnan(lp[:, 1]).all()) and idx[:, 1].tolist() == [10 ** 12, -4] and end.tolist() == [0, 0]


def test_decode_emit_state_is_read_at_run_time_and_opcheck():
    """One captured launch, replayed after the prompt lengths, the stop set, the end flags and the pad
    token change in device memory: each replay follows the values of its own time."""
    from replicatinggpt_amd import ops
    from replicatinggpt_amd.completion import stop_words
    Bn, n, width = 8, 2, 5
    lg = torch.randn(Bn, V, generator=torch.Generator().manual_seed(3)).to(DEV)
    greedy = torch.argmax(lg, dim=-1).cpu()
    seed_t, len_t = _i64(5), _i64(n)
    plen, limit, end = (torch.zeros(Bn, dtype=torch.int64, device=DEV) for _ in range(3))
    words = torch.zeros(2, dtype=torch.int64, device=DEV)
    pad = _i64(PAD)
    idx = torch.zeros((Bn, width), dtype=torch.int64, device=DEV)
    lp = torch.zeros((Bn, width), device=DEV)
    args = (lg, 0, None, seed_t, len_t, plen, limit, end, words, pad, idx, lp)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.decode_emit(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.decode_emit(*args)

    def replay(plen_v, limit_v, end_v, stop, pad_v):
        for t, v in ((plen, plen_v), (limit, limit_v), (end, end_v), (pad, pad_v), (idx, 9), (lp, -3.0)):
            t.fill_(v)
        words.copy_(torch.zeros(2, dtype=torch.int64) if not stop else stop_words(stop, V))
        graph.replay()
        torch.cuda.synchronize()
        return idx[:, n].cpu(), lp[:, n].cpu(), end.cpu()

    tok, l, e = replay(1, 10, 0, (), PAD)                       # emitted, running on
    assert torch.equal(tok, greedy) and bool((l < 0).all()) and e.tolist() == [0] * Bn
    tok, l, e = replay(n + 1, 10, 0, range(V), PAD)             # forced: a stop bit on a prompt token ends nothing
    assert tok.tolist() == [9] * Bn and e.tolist() == [0] * Bn
    want = torch.log_softmax(lg.double(), dim=-1)[:, 9].cpu()
    assert float((l.double() - want).abs().max()) <= LOGPROB_ABS
    tok, l, e = replay(1, 10, 0, range(V), PAD)                 # emitted and stopped
    assert torch.equal(tok, greedy) and e.tolist() == [n + 1] * Bn
    tok, l, e = replay(1, n + 1, 0, (), PAD)                    # emitted, at its limit
    assert torch.equal(tok, greedy) and e.tolist() == [n + 1] * Bn
    tok, l, e = replay(1, 10, 2, (), 33)                        # ended: this call's pad
    assert tok.tolist() == [33] * Bn and l.tolist() == [0.0] * Bn and e.tolist() == [2] * Bn
    end.zero_()
    torch.library.opcheck(ops.decode_emit, args)
    torch.library.opcheck(ops.decode_emit, (lg, 1, None, seed_t, len_t, plen, limit, end, words, pad, idx, None))


def test_decode_emit_rejects_bad_arguments():
    """V above 1024 and a mode outside {0, 1, 2}: the error status, the message names the argument,
    nothing is written."""
    from replicatinggpt_amd import ops
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=DEV)     # noqa: E731
    idx = z(2, 4)
    for Vn, mode, name in ((1025, 0, "V = 1025"), (65, 3, "mode = 3"), (65, -1, "mode = -1")):
        lg = torch.randn(2, Vn, device=DEV)
        with pytest.raises(RuntimeError, match=name):
            ops.decode_emit(lg, mode, None, _i64(1), _i64(1), z(2), z(2), z(2), z((Vn + 63) // 64), _i64(PAD), idx, None)
    with pytest.raises(RuntimeError, match="params_dev"):
        ops.decode_emit(torch.randn(2, 65, device=DEV), 2, None, _i64(1), _i64(1), z(2), z(2), z(2), z(2), _i64(PAD), idx,
                        None)
    torch.cuda.synchronize()
    assert int(idx.abs().sum()) == 0


# ---------------------------------------------------------------------------------------
# 6. log-probs end to end
# ---------------------------------------------------------------------------------------
_TEACHER = {}


def teacher_logprobs(par, ocfg, row, length):
    """fp64: (log_softmax of the oracle's last-row logits of row[max(0, n - T):n] at row[n] for 1 <= n <
    length, as [length] with entry 0 = 0; max |logit| over every forward used)."""
    T = ocfg.block_size
    out = torch.zeros(length, dtype=torch.float64)
    with torch.no_grad():
        lg, _ = O.forward(par, row[None, :min(T, length)], ocfg)       # causal: position n - 1 predicts column n
        amax = float(lg.abs().max())
        ls = torch.log_softmax(lg[0], dim=-1)
        for n in range(1, min(T, length - 1) + 1):
            out[n] = ls[n - 1, row[n]]
        for n in range(T + 1, length):
            lg, _ = O.forward(par, row[None, n - T:n], ocfg)
            amax = max(amax, float(lg.abs().max()))
            out[n] = torch.log_softmax(lg[0, -1], dim=-1)[row[n]]
    return out, amax


def test_logprobs_match_oracle_and_score_changes_no_token():
    """R1 greedy with return_logprobs=True, and score() of the R1 prompts: logprobs[b, n] within
    2 * 1e-5 * max|ref logits| + 1e-4 of the fp64 oracle's teacher-forced log_softmax at tokens[b, n],
    1 <= n < lengths[b].  The first term is the project's fp32 logits bar (relative to the largest
    logit of a forward; here the largest over the row's forwards) applied to the token's logit and to
    the log-sum-exp, which is 1-Lipschitz in the sup norm; the second is the kernel's own bound
    (test_decode_emit_kernel).  Column 0 and the pad columns are 0."""
    m, par, ocfg, prompts, P, new = case("R1")
    out = run_complete(m, prompts, new, greedy=True, pad_token=PAD, return_logprobs=True)
    streams = [oracle_stream("R1", b) for b in range(len(P))]
    check_rows_against(out, streams, P, new)
    assert out.steps == max(P) + new - 1             # with log-probs every column from 1 runs the head
    lp = out.logprobs.cpu()
    assert lp.shape == out.tokens.shape and lp.dtype == torch.float32
    with torch.no_grad():
        s_lp, s_len = m.score(prompts)
        kept = m.complete(prompts, 0, return_logprobs=True, greedy=True, pad_token=PAD)
    torch.cuda.synchronize()
    s_lp = s_lp.cpu()
    assert s_lp.shape == (len(P), max(P)) and s_len.tolist() == list(P)
    assert kept.lengths.tolist() == list(P) and kept.tokens.shape == (len(P), max(P))
    worst = 0.0
    for b, p in enumerate(P):
        ref, amax = teacher_logprobs(par, ocfg, streams[b], p + new)
        bound = 2 * FP32_BAR * amax + LOGPROB_ABS
        e1 = float((lp[b, :p + new].double() - ref).abs().max())
        e2 = float((s_lp[b, :p].double() - ref[:p]).abs().max())
        print(f"row {b}: complete log-prob error {e1:.3e}, score error {e2:.3e}, bound {bound:.3e} (max |logit| {amax:.2f})")
        worst = max(worst, e1 / bound, e2 / bound)
        assert e1 <= bound and e2 <= bound, (b, e1, e2, bound)
        assert float(lp[b, 0]) == 0.0 and bool((lp[b, p + new:] == 0).all())
        assert float(s_lp[b, 0]) == 0.0 and bool((s_lp[b, p:] == 0).all())
        assert bool((lp[b, 1:p + new] < 0).all())
        assert torch.equal(kept.tokens[b, :p].cpu(), prompts[b]) and bool((kept.tokens[b, p:] == PAD).all())
    assert math.isfinite(worst)


def test_complete_needs_eval_forward_and_vocabulary_pad():
    m, par, ocfg, prompts, P, new = case("R2")
    with pytest.raises(ValueError, match="pad_token"):
        m.complete(prompts, 2, pad_token=V)
    assert m.complete(prompts, 0).tokens.shape == (3, 128)      # nothing to run: the prompts, padded
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    d = BigramLanguageModel(GPTConfig(block_size=8, n_embd=32, n_head=2, n_layers=1, dropout=0.1)).to(DEV).train()
    with pytest.raises(RuntimeError, match="eval"):
        d.complete([torch.tensor([1, 2])], 2)
