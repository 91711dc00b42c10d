"""Temperature / top-k / top-p sampling, the parts that need no GPU: the fp64 reference of the
contract (include/charpt.h, cg_decode_sample_filtered -- written from the contract, shared with
tests/test_gpu_sampling.py), sampling.filter_logits against it, generate()'s argument validation on
a CPU model, the C ABI's declaration and the command-line sampler's parsing and prompt encoding."""
import numpy as np
import pytest
import torch

from oracle import philox

NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------
# the contract in fp64
# ---------------------------------------------------------------------------------------
def filtered_gate(Vn):
    """Relative to the weight sums: V sequential fp32 additions in the nucleus scan, V in the draw scan,
    and 32 roundings for the exp, the temperature and the u * S and p * S_k products, of 2^-24 each,
    times a safety factor of 4 (as sample_gate in test_gpu_decode.py)."""
    return 4 * (2 * Vn + 32) * 2.0 ** -24


def reference(logits, tau, k, p, seed=0, length=0, g=0.0, g_draw=None):
    """The contract per row of ``logits`` ([B, V], any float dtype, no NaN / +inf), in fp64.

    Returns a dict: ``kept`` [B, V] bool, ``n_keep`` [B], ``order`` [B, V] (token at each rank),
    ``rank`` [B, V], ``cum_rank`` [B, k'] (rank-order cumulative weight of the top-k'), ``S_k``,
    ``tok`` [B] (the draw (seed, length, row)), and ``gated`` [B]: the draw lies within g_draw * S of a
    cumulative boundary of the kept set, or p * S_k within g * S_k of a rank-order boundary."""
    x = np.asarray(logits.double().numpy() if isinstance(logits, torch.Tensor) else logits, dtype=np.float64)
    Bn, Vn = x.shape
    g_draw = g if g_draw is None else g_draw
    # 1. rank: descending, lower index first among equals
    order = np.argsort(-x, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(Vn), (Bn, Vn)), axis=1)
    # 2. weights
    with np.errstate(invalid="ignore"):
        w = np.where(np.isneginf(x), 0.0, np.exp((x - x.max(axis=1, keepdims=True)) / tau))
    # 3. top-k
    kk = Vn if (not k or k >= Vn) else int(k)
    ws = np.take_along_axis(w, order, axis=1)[:, :kk]
    cum = np.cumsum(ws, axis=1)
    S_k = cum[:, -1]
    # 4. top-p: the shortest prefix with cum >= p * S_k
    n_keep = np.full(Bn, kk)
    gated = np.zeros(Bn, dtype=bool)
    if p < 1:
        thr = p * S_k
        reach = cum >= thr[:, None]
        n_keep = np.where(reach.any(axis=1), reach.argmax(axis=1) + 1, kk)
        gated |= (np.abs(cum - thr[:, None]) < (g * S_k)[:, None]).any(axis=1)
    kept = rank < n_keep[:, None]
    # 5. the draw over the kept set, in vocabulary order
    b = np.arange(Bn, dtype=np.uint64)
    r0 = philox.philox4x32_10(b, 0, length, 0, seed & 0xffffffff, seed >> 32)[0]
    u = (r0 >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    c = np.cumsum(np.where(kept, w, 0.0), axis=1)
    S = c[:, -1]
    t = u * S
    first = (c <= t[:, None]).sum(axis=1)                      # the first v with t < c[v]: a kept one
    last_kept = Vn - 1 - np.argmax(kept[:, ::-1], axis=1)
    tok = np.where(first < Vn, first, last_kept)
    bound = np.where(kept, c, np.inf)
    gated |= (np.abs(t[:, None] - bound) < (g_draw * S)[:, None]).any(axis=1)
    return dict(kept=kept, n_keep=n_keep, order=order, rank=rank, cum_rank=cum, S_k=S_k, tok=tok, gated=gated, w=w)


def test_reference_by_hand():
    """The reference on rows small enough to do by hand."""
    x = torch.tensor([[0.0, np.log(2.0), np.log(2.0), np.log(4.0)]])           # weights 1/4, 1/2, 1/2, 1
    r = reference(x, 1.0, 0, 1.0)
    assert r["order"].tolist() == [[3, 1, 2, 0]] and r["kept"].all()
    assert np.allclose(r["w"], [[0.25, 0.5, 0.5, 1.0]])
    r = reference(x, 1.0, 2, 1.0)                                               # the tie: index 1 before 2
    assert r["kept"].tolist() == [[False, True, False, True]]
    r = reference(x, 1.0, 0, 0.6)                                               # 1, 1.5 of 2.25: 1.5 >= 1.35
    assert r["kept"].tolist() == [[False, True, False, True]] and r["n_keep"].tolist() == [2]
    r = reference(x, 1.0, 3, 0.76)                                              # S_k = 2: 1, 1.5, 2 >= 1.52
    assert r["n_keep"].tolist() == [3] and r["kept"].tolist() == [[False, True, True, True]]
    r = reference(x, 0.5, 0, 1.0)                                               # weights squared
    assert np.allclose(r["w"], [[1 / 16, 0.25, 0.25, 1.0]])
    r = reference(x, 1.0, 1, 1.0)
    assert r["kept"].tolist() == [[False, False, False, True]] and r["tok"].tolist() == [3]
    r = reference(x, 1.0, 0, 1e-9)
    assert r["n_keep"].tolist() == [1] and r["tok"].tolist() == [3]


# ---------------------------------------------------------------------------------------
# the C ABI's declaration
# ---------------------------------------------------------------------------------------
def test_filtered_sampler_is_declared_and_exported():
    from replicatinggpt_amd import _lib
    name = "cg_decode_sample_filtered"
    assert name in _lib.header_symbols()
    assert name in _lib._SIGS
    assert len(_lib._SIGS[name][1]) == 10
    assert hasattr(_lib.load(), name)


# ---------------------------------------------------------------------------------------
# filter_logits against the reference
# ---------------------------------------------------------------------------------------
SETTINGS = [(0.7, 0, 1.0), (1.5, None, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.9), (0.8, 40, 0.95), (1.0, 0, 0.5),
            (2.0, 3, 0.6), (1.0, 1, 1.0), (1.0, 0, 1e-9), (1.0, 2, 0.999)]


def _rows(Vn):
    """randn rows plus the edge rows: duplicated logits straddling a top-k boundary, -inf entries
    (also ranked last, also in the last column), everything equal."""
    gen = torch.Generator().manual_seed(50 + Vn)
    x = torch.randn(64, Vn, generator=gen) * 2
    x[1] = 0.25                                           # all equal: the lower indices are kept
    x[2, -1] = NEG_INF
    if Vn >= 3:
        x[3, [0, Vn - 1]] = 7.0                           # the maximum twice: top_k = 1 keeps index 0
        x[4, :] = torch.arange(Vn, 0, -1).float()
        x[4, 1:3] = 5.5                                   # ranks 1 and 2 equal (k = 2 cuts between them)
        x[5, 1::2] = NEG_INF
    if Vn >= 6:
        x[6, :] = -torch.arange(Vn).float() * 0.1
        x[6, 4:6] = -0.45                                 # ranks 4 and 5 equal (k = 5 cuts between them)
        x[7, [Vn - 1, Vn - 2, 2]] = 3.0                   # equal across the ends of the row
    if Vn > 64:
        x[8, [0, 64]] = 9.0                               # columns one 64-lane pass apart
    return x


@pytest.mark.parametrize("Vn", [1, 2, 3, 64, 65, 130])
def test_filter_logits_keeps_the_reference_set(Vn):
    """filter_logits(x, t, k, p) is x / t on exactly the reference's kept set and -inf elsewhere: for
    every setting of SETTINGS plus k = V, k > V; rows whose p * S_k lies within 1e-12 S_k of a rank
    boundary are left out (none expected)."""
    from replicatinggpt_amd.sampling import filter_logits
    x = _rows(Vn)
    for tau, k, p in SETTINGS + [(0.9, Vn, 1.0), (0.9, Vn + 3, 1.0), (1.0, Vn, 0.7)]:
        ref = reference(x, tau, k, p, g=1e-12)
        got = filter_logits(x, tau, k, p)
        assert got.shape == x.shape and got.dtype == x.dtype
        want = torch.where(torch.from_numpy(ref["kept"]), x / tau, torch.full_like(x, NEG_INF))
        ok = torch.from_numpy(~ref["gated"])
        assert int((~ok).sum()) <= 1, (Vn, tau, k, p, int((~ok).sum()))
        assert torch.equal(got[ok], want[ok]), (Vn, tau, k, p)
        assert bool((ref["n_keep"] >= 1).all())
        if k and k < Vn:
            assert int(ref["kept"].sum(axis=1).max()) <= k
        if k == 1 or p == 1e-9:                            # degenerate: the first maximum alone
            am = torch.argmax(x, dim=-1)
            assert torch.equal(torch.isfinite(got).sum(dim=-1), torch.isfinite(x.gather(1, am[:, None]))[:, 0].long())
            assert bool((torch.from_numpy(ref["kept"]).long().argmax(dim=-1) == am).all())


def test_filter_logits_ties_at_the_top_k_boundary():
    from replicatinggpt_amd.sampling import filter_logits
    x = torch.tensor([[1.0, 3.0, 3.0, 3.0, 2.0, NEG_INF]])
    assert filter_logits(x, 1.0, 2, 1.0).tolist() == [[NEG_INF, 3.0, 3.0, NEG_INF, NEG_INF, NEG_INF]]
    assert filter_logits(x, 0.5, 1, 1.0).tolist() == [[NEG_INF, 6.0, NEG_INF, NEG_INF, NEG_INF, NEG_INF]]
    assert filter_logits(x, 1.0, 4, 1.0).tolist() == [[NEG_INF, 3.0, 3.0, 3.0, 2.0, NEG_INF]]
    # batched leading dimensions
    y = filter_logits(x.expand(2, 3, 6), 1.0, 2, 1.0)
    assert y.shape == (2, 3, 6) and y[1, 2].tolist() == [NEG_INF, 3.0, 3.0, NEG_INF, NEG_INF, NEG_INF]


def test_filter_logits_neutral_is_identity():
    from replicatinggpt_amd.sampling import filter_logits
    x = torch.randn(5, 65)
    for args in ((), (1.0, None, 1.0), (1.0, 0, 1.0), (1, 0, 1)):
        assert filter_logits(x, *args) is x
    assert torch.equal(filter_logits(x, 1.0, 65, 1.0), x) and torch.equal(filter_logits(x, 1.0, 1000, 1.0), x)
    assert torch.equal(filter_logits(x, 2.0, None, 1.0), x / 2.0)


def test_filtered_multinomial_stays_in_the_kept_set():
    """softmax + multinomial after filter_logits, as the literal loop runs them."""
    from replicatinggpt_amd.sampling import filter_logits
    x = _rows(65)
    ref = reference(x, 0.8, 10, 0.9)
    probs = torch.softmax(filter_logits(x, 0.8, 10, 0.9), dim=-1)
    draws = torch.multinomial(probs, 200, replacement=True, generator=torch.Generator().manual_seed(1))
    assert bool(torch.from_numpy(ref["kept"]).gather(1, draws).all())


# ---------------------------------------------------------------------------------------
# generate()'s validation, before any device work
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_model():
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    torch.manual_seed(0)
    return BigramLanguageModel(GPTConfig(block_size=8, n_embd=16, n_head=2, n_layers=1, dropout=0.0, dtype="fp32")).eval()


@pytest.mark.parametrize("kw,name", [
    (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
    (dict(temperature=float("nan")), "temperature"), (dict(temperature=float("inf")), "temperature"),
    (dict(top_k=-1), "top_k"), (dict(top_k=2.5), "top_k"),
    (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=-0.1), "top_p"), (dict(top_p=float("nan")), "top_p"),
    (dict(greedy=True, temperature=0.5), "greedy"), (dict(greedy=True, top_k=3), "greedy"),
    (dict(greedy=True, top_p=0.9), "greedy"),
])
def test_generate_rejects_bad_sampling_arguments_on_cpu(cpu_model, kw, name):
    idx = torch.zeros((1, 1), dtype=torch.long)
    with pytest.raises(ValueError, match=name):
        cpu_model.generate(idx, 4, **kw)
    with pytest.raises(ValueError, match=name):
        cpu_model.generate(idx, 4, engine=False, **kw)


def test_temperature_error_points_to_greedy(cpu_model):
    with pytest.raises(ValueError, match="greedy=True"):
        cpu_model.generate(torch.zeros((1, 1), dtype=torch.long), 4, temperature=0)


def test_check_sampling_and_params():
    from replicatinggpt_amd.sampling import check_sampling, sampling_params
    assert check_sampling() is True and check_sampling(1.0, 0, 1.0, greedy=True) is True
    assert check_sampling(1.0, None, 1) is True
    assert check_sampling(0.8, None, 1.0) is False and check_sampling(1.0, 3, 1.0) is False
    assert check_sampling(1.0, 0, 0.9) is False
    assert sampling_params().tolist() == [1.0, 0.0, 1.0]
    assert sampling_params(0.5, 40, 0.25).tolist() == [0.5, 40.0, 0.25]
    assert sampling_params(1.0, 10 ** 12, 1.0).tolist() == [1.0, float(1 << 24), 1.0]
    assert sampling_params().dtype == torch.float32


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def test_sample_cli_arguments():
    from replicatinggpt_amd import sample
    from replicatinggpt_amd.data import DEFAULT_INPUT
    a = sample.parse_args(["--model", "m.pth"])
    assert (a.model, a.preset, a.dtype, a.input, a.prompt) == ("m.pth", "c1", "fp32", DEFAULT_INPUT, "")
    assert (a.num_samples, a.max_new_tokens, a.temperature, a.top_k, a.top_p, a.greedy) == (1, 500, 1.0, None, 1.0, False)
    a = sample.parse_args(["--model", "m.pth", "--preset", "c2", "--dtype", "bf16", "--input", "x.txt", "--prompt",
                           "ROMEO:", "--num-samples", "3", "--max-new-tokens", "20", "--temperature", "0.8", "--top-k",
                           "40", "--top-p", "0.95", "--seed", "9", "--greedy"])
    assert (a.preset, a.dtype, a.input, a.prompt, a.num_samples, a.max_new_tokens) == ("c2", "bf16", "x.txt", "ROMEO:", 3, 20)
    assert (a.temperature, a.top_k, a.top_p, a.seed, a.greedy) == (0.8, 40, 0.95, 9, True)
    with pytest.raises(SystemExit):
        sample.parse_args([])                                   # --model is required
    with pytest.raises(SystemExit):
        sample.parse_args(["--model", "m.pth", "--num-samples", "0"])


def test_sample_cli_prompt_encoding():
    from replicatinggpt_amd import sample
    from replicatinggpt_amd.data import DEFAULT_INPUT
    tok = sample.load_tokenizer(DEFAULT_INPUT)
    assert tok.vocab_size == 65
    ctx = sample.encode_prompt(tok, "ROMEO:", 3)
    assert ctx.shape == (3, 6) and ctx.dtype == torch.long
    assert tok.decode(ctx[2].tolist()) == "ROMEO:" and torch.equal(ctx[0], ctx[1])
    empty = sample.encode_prompt(tok, "", 2)                   # GPT1.py:235: zeros((1, 1)), per row
    assert torch.equal(empty, torch.zeros((2, 1), dtype=torch.long))
    with pytest.raises(ValueError, match="vocabulary") as e:
        sample.encode_prompt(tok, "ROMEO~ and JULIET#", 1)
    assert "~" in str(e.value) and "#" in str(e.value)


def test_gpt1_driver_has_the_sampling_flags():
    from replicatinggpt_amd import gpt1
    a = gpt1.parse_args([])
    assert (a.temperature, a.top_k, a.top_p) == (1.0, None, 1.0)          # neutral: the final sample is unchanged
    a = gpt1.parse_args(["--temperature", "0.7", "--top-k", "20", "--top-p", "0.9"])
    assert (a.temperature, a.top_k, a.top_p) == (0.7, 20, 0.9)
