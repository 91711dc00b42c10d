"""The bf16 training path at shapes off its fast branches.

The path is a lattice of shape predicates (functional.premask_ok / rowdot_ok / _relu_bits_ok /
_colpart_ok / _head_fused_ok, the ``fast`` of _wgrad_single and linear_wgrad_group, _split_for_tiles;
csrc/gemm_bf16.hip fast_shape_ok, csrc/attention.hip fast_attn_ok), and every other whole-model bf16
test runs where all of them hold (test_gpu_grad_targets.build asserts it).  The fallback kernels have
their per-op tests; here the glue that strings them together runs inside a model: linear_fwd(...,
"bias_relu") with h read back, linear_dgrad(..., "relu_bwd", aux=h) plus colsum_into, linear_dgrad in
place of the ROWDOT epilogue with the attention backward computing delta itself, _head_plain_fwd/_bwd
with to_act(dl) at ld 65, _wgrad_single asking for bf16 slabs and deferral that cg_gemm declines, a
grouped split-K launch next to generic dgrads, the ring attention (T > 256) inside a model.

1. ROW-PADDED TWINS (tests/twins.py PAIRS, T1..T4): a ragged batch against the same rows padded with
   ignored filler rows up to a shape on which every predicate holds -- the same function of the same
   bf16 operands with the same rounding points (tests/test_cpu_twins.py shows the identity on the
   fp64 oracle), computed by the generic launches on one side and the persistent / MFMA / fused ones
   on the other.  Gate: conftest.bf16_close with its defaults, element by element, on the logits and
   every parameter gradient; the loss within 1 %.  What ran is asserted from a spy over one step
   against a table computed from the library's own predicates.
2. SHAPES WITH NO TWIN (twins.SHAPES, X1..X5) and the four ragged runs, against the fp32 CPU oracle by
   the reference-relative rule of twins.rule_records, e_t from the oracle's forward under
   torch.autocast(bfloat16) on the same GPU, every e_t <= 6e-2 as its own "torch-bf16" record.
3. STEP MODES at T3's ragged shape and at X1: eager, one graph, segmented, deferral off, early AdamW
   off -- the same losses, master weights and flat gradient bit for bit.

Run with -s for the figures; profiles/bf16_offpath_gpu_tests.txt holds those measured on MI355X:
every launch count as the predicates give it and as the table of twins.py expects; ragged against twin
at most 2.9e-3 by norm (T3 blocks.0.ln1.weight), 4.0e-3 of the maximum and 0.35 of the element-wise bar,
the losses within 5.5e-7 (T3: equal), the logits within 8.2e-4 of their maximum; against the oracle the
worst e_c / e_t is 1.19 (X3 micro-batch B blocks.0.ffwd.net.0.bias 4.57e-2 against 3.83e-2; T4
blocks.1.ln2.weight 4.18e-2 against 3.52e-2), no parameter between 1.25 and 1.5 e_t, torch's own largest
e_t 5.67e-2 (X3 micro-batch B blocks.1.ln2.bias), the losses within 5e-5; the masked loss with nothing
ignored is bit-equal to the unmasked one at T1 and T3; every step mode bit-identical.  No product fault."""
import functools

import pytest
import torch

import twins as TW
from test_cpu_grad_targets import DROPOUT, INIT_SEED, N_LAYERS
from test_gpu_grad_targets import grads_of

pytestmark = pytest.mark.gpu
DEV = "cuda"

SPIED = ("layernorm_fwd_attn_dropmask", "gemm_bias_relu_bits", "gemm_relu_bwd_colpart", "gemm_store_rowdot",
         "gemm_wgrad_group", "head_fwd", "head_fwd_masked", "head_bwd", "head_bwd_masked")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


# ---------------------------------------------------------------------------------------
# models, steps, references (each computed once and never modified)
# ---------------------------------------------------------------------------------------
def gpt_config(spec, **kw):
    from replicatinggpt_amd import GPTConfig
    return GPTConfig(vocab_size=spec["vocab_size"], block_size=spec["block_size"], n_embd=spec["n_embd"],
                     n_head=spec["n_head"], n_layers=N_LAYERS, dropout=DROPOUT, dtype="bf16", **kw)


def build(spec):
    from replicatinggpt_amd import BigramLanguageModel
    torch.manual_seed(INIT_SEED)
    m = BigramLanguageModel(gpt_config(spec)).to(DEV)
    assert m.training
    return m


def step(m, batch):
    """test_gpu_grad_targets.run(m, batch, defer=True) that keeps the logits: one forward / backward
    inside ``with DEFER:`` as engine.TrainStep runs it.  ``batch``: (idx, targets[, ignore_index]).
    Returns (loss, logits [B T, V] on the CPU, {name: grad})."""
    from replicatinggpt_amd import functional as Fn
    m.zero_grad(set_to_none=True)
    logits, loss = m(*batch)
    with Fn.DEFER:
        loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), logits.detach().float().cpu(), {k: g.cpu() for k, g in grads_of(m).items()}


def on_dev(batch):
    return tuple(t.to(DEV) for t in batch)


def census(m, B, T):
    """The training path's dispatch predicates for model ``m`` at B rows of T tokens, asked from the
    library's own functions (as test_gpu_grad_targets.fast_branches, which asserts them all true)."""
    from replicatinggpt_amd import _lib as L
    from replicatinggpt_amd import functional as Fn
    cfg = m.config
    C, H, V = cfg.n_embd, cfg.n_head, cfg.vocab_size
    M, D, F4 = B * T, C // H, 4 * C
    R = m._store.regions
    bf = torch.bfloat16
    a = torch.zeros((M, C), dtype=bf, device=DEV)
    h = torch.zeros((M, F4), dtype=bf, device=DEV)
    w1, w2, wp = R["0.w1"].operand(bf), R["0.w2"].operand(bf), R["0.proj_w"].operand(bf)
    lib = L.load()

    def persistent(bt, m_, n_, k_, lda, ldb, ldc):
        # csrc/gemm_bf16.hip fast_shape_ok at the default dispatch, through an exported predicate that adds
        # nothing to it for a non-transposed A at split 1 (cg_gemm_colpart_supported)
        return bool(lib.cg_gemm_colpart_supported(0, bt, m_, n_, k_, lda, ldb, ldc))

    def wgrad(n, k):   # functional._wgrad_single's view of out[n, k] = dy[M, n]^T x[M, k]
        fast = n % 128 == 0 and k % 128 == 0 and M % 64 == 0
        return fast, Fn._wgrad_split(n, k, M, fast)

    def grouped(*nk):  # functional.linear_wgrad_group's view of a sublayer's pair
        if not (Fn._wgrad_group_on(bf) and M % 64 == 0 and all(n % 128 == 0 and k % 128 == 0 for n, k in nk)):
            return False
        return Fn._split_for_tiles(sum((n // 128) * (k // 128) for n, k in nk), M // 64) > 1
    fused = Fn._head_fused_ok(bf, R["lm_w"], M, C, V)
    head_nk = (128, C) if fused else (V, C)
    out = {
        "tokens": M,
        "premask_ok (LN + keep-bit launch, MFMA attention)": Fn.premask_ok(bf, T, D) and Fn.LN_MASK
        and not Fn.SIDE.premask,
        "_relu_bits_ok": Fn._relu_bits_ok(a, w1, w2, F4),
        "_colpart_ok": Fn._colpart_ok(a, w2, h, F4),
        "rowdot_ok": Fn.rowdot_ok(a, wp, a, T, D),
        "_head_fused_ok": fused,
        "persistent forward QKV / proj / FFN-1 / FFN-2": (persistent(0, M, 3 * C, C, C, C, 3 * C),
                                                          persistent(0, M, C, C, C, C, C),
                                                          persistent(0, M, F4, C, C, C, F4),
                                                          persistent(0, M, C, F4, F4, F4, C)),
        "persistent dgrad proj / QKV / FFN-2 / FFN-1": (persistent(1, M, C, C, C, C, C),
                                                        persistent(1, M, C, 3 * C, 3 * C, C, C),
                                                        persistent(1, M, F4, C, C, F4, F4),
                                                        persistent(1, M, C, F4, F4, C, C)),
        "wgrad (fast, split) proj / QKV / FFN-2 / FFN-1 / lm_head": (wgrad(C, C), wgrad(3 * C, C), wgrad(C, F4),
                                                                     wgrad(F4, C), wgrad(*head_nk)),
        "attention pair grouped": grouped((C, C), (3 * C, C)),
        "FeedForward pair grouped": bool(Fn.WGRAD_GROUP_FFN) and grouped((C, F4), (F4, C)),
        "DEFER enabled": Fn.DEFER.enabled and Fn.DEFER.partials_on,
        "bf16 slabs": bool(Fn.SLAB_BF16),
    }
    return {k: (v if isinstance(v, (tuple, int)) and not isinstance(v, bool) else bool(v)) for k, v in out.items()}


def expected_calls(cen, masked):
    """The spied launches of one step that ``cen`` implies."""
    fused = cen["_head_fused_ok"]
    return {
        "layernorm_fwd_attn_dropmask": N_LAYERS * cen["premask_ok (LN + keep-bit launch, MFMA attention)"],
        "gemm_bias_relu_bits": N_LAYERS * cen["_relu_bits_ok"],
        "gemm_relu_bwd_colpart": N_LAYERS * cen["_colpart_ok"],
        "gemm_store_rowdot": N_LAYERS * cen["rowdot_ok"],
        "gemm_wgrad_group": N_LAYERS * (cen["attention pair grouped"] + cen["FeedForward pair grouped"]),
        "head_fwd": int(fused and not masked), "head_fwd_masked": int(fused and masked),
        "head_bwd": int(fused and not masked), "head_bwd_masked": int(fused and masked),
    }


def spied_step(monkeypatch, m, batch):
    """step(m, batch) with the launches of SPIED counted and every weight-gradient request through
    ops.gemm recorded as (N, K, tokens, split, flags).  Returns (step's result, counts, requests)."""
    from replicatinggpt_amd import ops
    calls = dict.fromkeys(SPIED, 0)
    wgrads = []
    with monkeypatch.context() as mp:
        for fn in SPIED:
            def spy(*args, _fn=fn, _real=getattr(ops, fn), **kw):
                calls[_fn] += 1
                return _real(*args, **kw)
            mp.setattr(ops, fn, spy)
        real_gemm = ops.gemm

        def gemm_spy(a, b, out, op_bf16, a_trans, b_trans, M, N, K, *rest, **kw):
            if a_trans and b_trans:   # rest: lda, ldb, ldc, epi, ..., beta, split_k [14], ws [15], flags [16]
                wgrads.append((M, N, K, rest[14], rest[16] if len(rest) > 16 else kw.get("flags", 0)))
            return real_gemm(a, b, out, op_bf16, a_trans, b_trans, M, N, K, *rest, **kw)
        mp.setattr(ops, "gemm", gemm_spy)
        res = step(m, batch)
    return res, calls, wgrads


def show_census(label, cen, calls, wgrads):
    for k, v in cen.items():
        print(f"[census {label}] {k}: {v}")
    print(f"[census {label}] launches in one step: {calls}")
    print(f"[census {label}] weight-gradient requests through cg_gemm (N, K, tokens, split, flags): "
          f"{sorted(set(wgrads))}")


@functools.lru_cache(maxsize=None)
def batches(name):
    """The micro-batches of ``name`` on the CPU: a pair's ragged batch, or a shape's."""
    return [TW.make_pair(name)[0]] if name in TW.PAIRS else TW.shape_batches(name)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """[(loss, logits, {name: grad})] of the fp32 CPU oracle, one per micro-batch (dropout calls 0, 1, ...)."""
    spec = TW.spec_of(name)
    P, cfg, seed = TW.oracle_params(spec), TW.oracle_config(spec), gpt_config(spec).dropout_seed
    out = []
    for call, (idx, tgt) in enumerate(batches(name)):
        z, l, g = TW.oracle_step(P, idx, tgt, cfg, seed, call)
        out.append((float(l), z, g))
    return out


@functools.lru_cache(maxsize=None)
def torch_bf16(name):
    """The same from the oracle's forward under autocast(bfloat16) on the GPU, from the same parameters
    and batches: the calibration of the rule (test_gpu_grad_targets.torch_bf16's method)."""
    spec = TW.spec_of(name)
    P = {k: v.to(DEV) for k, v in TW.oracle_params(spec).items()}
    cfg, seed = TW.oracle_config(spec), gpt_config(spec).dropout_seed
    out = []
    for call, (idx, tgt) in enumerate(batches(name)):
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            z, l, g = TW.oracle_step(P, idx.to(DEV), tgt.to(DEV), cfg, seed, call)
        out.append((float(l), z.float().cpu(), {k: v.double().cpu() for k, v in g.items()}))
    return out


def check_rule(label, name, results):
    """``results``: one (loss, logits, grads) per micro-batch of ``name`` from the HIP path; the loss
    within 1 % of the oracle's and every gradient by the reference-relative rule."""
    for call, ((loss, _, got), (l_ref, _, g_ref), (l_t, _, g_t)) in enumerate(zip(results, oracle(name),
                                                                                 torch_bf16(name))):
        tag = f"{label} call {call}"
        print(f"[{tag}] loss {loss:.6f}, oracle {l_ref:.6f} (rel {abs(loss - l_ref) / l_ref:.3e}), "
              f"torch-bf16 {l_t:.6f}")
        bad, capped = TW.rule_report(tag, TW.rule_records(got, g_ref, g_t))
        assert not capped, ("torch-bf16", tag, capped)
        assert TW.loss_close(loss, l_ref), (tag, loss, l_ref)
        assert not bad, (tag, bad)


# ---------------------------------------------------------------------------------------
# 1. row-padded twins
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_run(pair):
    """The unspied ragged step of a fresh model (the tests that need only its numbers)."""
    return step(build(TW.spec_of(pair)), on_dev(TW.make_pair(pair)[0]))


@pytest.mark.parametrize("pair", sorted(TW.PAIRS))
def test_ragged_matches_padded_twin(pair, monkeypatch):
    """The ragged batch through the fallback launches against its twin through the fast ones:
    bf16_close on the logits and every gradient, the loss within 1 %, and the launches each side made.

    Named entries, all as the predicates give them: the ragged run makes no gemm_bias_relu_bits /
    gemm_relu_bwd_colpart / gemm_store_rowdot call; the twin makes N_LAYERS of each its shape allows
    (all three at T1 / T2; no ROWDOT at T3 / T4, T % 64 != 0); T2's ragged run makes 2 N_LAYERS grouped
    weight-gradient launches, T3's none; T4's ragged run makes no fused-head call and its twin one
    head_fwd_masked."""
    p = TW.PAIRS[pair]
    spec = TW.spec_of(pair)
    ragged, twin = TW.make_pair(pair)
    runs = {}
    for side, batch, B in (("ragged", ragged, p["B_r"]), ("twin", (*twin, TW.IGNORE), p["B_a"])):
        m = build(spec)
        cen = census(m, B, p["T"])
        res, calls, wgrads = spied_step(monkeypatch, m, on_dev(batch[:2]) + tuple(batch[2:]))
        show_census(f"{pair} {side}", cen, calls, wgrads)
        assert calls == expected_calls(cen, masked=side == "twin"), (pair, side, calls, cen)
        runs[side] = (res, calls, cen)
    (res_r, calls_r, cen_r), (res_t, calls_t, cen_t) = runs["ragged"], runs["twin"]
    # the named entries
    for fn in ("gemm_bias_relu_bits", "gemm_relu_bwd_colpart", "gemm_store_rowdot"):
        assert calls_r[fn] == 0, (pair, fn, calls_r)
    assert calls_t["gemm_bias_relu_bits"] == calls_t["gemm_relu_bwd_colpart"] == N_LAYERS, calls_t
    assert calls_t["gemm_store_rowdot"] == (N_LAYERS if pair in ("T1", "T2") else 0), calls_t
    assert not any(cen_r["persistent forward QKV / proj / FFN-1 / FFN-2"]), cen_r
    assert all(cen_t["persistent forward QKV / proj / FFN-1 / FFN-2"]), cen_t
    assert all(cen_t["persistent dgrad proj / QKV / FFN-2 / FFN-1"]) and cen_t["_head_fused_ok"], cen_t
    premask = "premask_ok (LN + keep-bit launch, MFMA attention)"
    assert cen_r[premask] == cen_t[premask] == (pair in ("T1", "T2"))
    if pair == "T1":   # the weight gradients stay on the persistent kernel at split 1
        assert all(w == (True, 1) for w in cen_r["wgrad (fast, split) proj / QKV / FFN-2 / FFN-1 / lm_head"]), cen_r
    if pair == "T2":
        assert calls_r["gemm_wgrad_group"] == 2 * N_LAYERS, calls_r
    if pair == "T3":
        assert calls_r["gemm_wgrad_group"] == 0, calls_r
        assert not any(f for f, _ in cen_r["wgrad (fast, split) proj / QKV / FFN-2 / FFN-1 / lm_head"]), cen_r
    if pair == "T4":
        assert calls_r["head_fwd"] == calls_r["head_fwd_masked"] == 0 and not cen_r["_head_fused_ok"], calls_r
        assert calls_t["head_fwd_masked"] == 1, calls_t
    # the spied step is the plain step
    plain = ragged_run(pair)
    assert plain[0] == res_r[0] and torch.equal(plain[1], res_r[1])
    assert all(torch.equal(plain[2][k], res_r[2][k]) for k in plain[2])
    # ragged against twin
    bad = TW.twin_report(f"twin {pair}", TW.twin_records(res_r, res_t, p["B_r"] * p["T"]))
    assert not bad, (pair, [(r[0], r[2]) for r in bad])


@pytest.mark.parametrize("pair", sorted(TW.PAIRS))
def test_ragged_matches_oracle(pair):
    """The ragged run by the reference-relative rule, as the absolute anchor: two paths that are wrong
    the same way would pass the twin."""
    check_rule(f"rule {pair}", pair, [ragged_run(pair)])


@pytest.mark.parametrize("pair", ["T1", "T3"])
def test_ragged_with_nothing_ignored(pair):
    """ignore_index=-100 passed and no target ignored: the masked loss kernels on the ragged shape give
    the unmasked run's loss and gradients (bf16_close; whether bit-equal is printed, not asserted)."""
    plain = ragged_run(pair)
    masked = step(build(TW.spec_of(pair)), on_dev(TW.make_pair(pair)[0]) + (TW.IGNORE,))
    equal = plain[0] == masked[0] and torch.equal(plain[1], masked[1]) and \
        all(torch.equal(plain[2][k], masked[2][k]) for k in plain[2])
    print(f"[ignore {pair}] masked run with nothing ignored bit-equal to the unmasked run: {equal}")
    bad = TW.twin_report(f"ignore {pair}", TW.twin_records(masked, plain))
    assert not bad, (pair, [(r[0], r[2]) for r in bad])


# ---------------------------------------------------------------------------------------
# 2. shapes with no twin
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TW.SHAPES))
def test_shape_matches_oracle(name, monkeypatch):
    """One model, its micro-batches in turn (X3: A as dropout call 0, zero_grad(set_to_none=True), B as
    call 1), each against the fp32 oracle by the reference-relative rule -- after the census entries the
    shape is here for."""
    from replicatinggpt_amd import _lib as L
    spec = TW.spec_of(name)
    m = build(spec)
    results = []
    for call, batch in enumerate(batches(name)):
        B, T = batch[0].shape
        cen = census(m, B, T)
        res, calls, wgrads = spied_step(monkeypatch, m, on_dev(batch))
        show_census(f"{name} call {call}", cen, calls, wgrads)
        assert calls == expected_calls(cen, masked=False), (name, calls, cen)
        results.append(res)
        fwd = cen["persistent forward QKV / proj / FFN-1 / FFN-2"]
        dgr = cen["persistent dgrad proj / QKV / FFN-2 / FFN-1"]
        wg = cen["wgrad (fast, split) proj / QKV / FFN-2 / FFN-1 / lm_head"]
        premask = cen["premask_ok (LN + keep-bit launch, MFMA attention)"]
        if name == "X1":
            # FFN-1 and the ReLU-backward dgrad fast with keep bits and column partials; QKV / proj / FFN-2
            # generic, so no ROWDOT; generic weight gradients whose split-K requests carry the flags
            assert premask and cen["_relu_bits_ok"] and cen["_colpart_ok"] and not cen["rowdot_ok"], cen
            assert fwd == (False, False, True, False) and dgr == (False, False, True, False), cen
            assert not any(f for f, _ in wg) and all(s == 2 for _, s in wg[:4]), cen
            both = L.GEMM_SLAB_BF16 | L.GEMM_DEFER_REDUCE
            assert calls["gemm_wgrad_group"] == 0
            assert sum(1 for w in wgrads if w[3] == 2 and w[4] == both) >= 4 * N_LAYERS, wgrads
        elif name == "X2":
            assert all(fwd) and all(dgr) and cen["_relu_bits_ok"] and cen["_colpart_ok"], cen
            assert not premask and not cen["rowdot_ok"], cen
        elif name == "X3":
            assert not (any(fwd) or any(dgr) or premask or cen["_relu_bits_ok"] or cen["_colpart_ok"]
                        or cen["rowdot_ok"] or cen["_head_fused_ok"] or any(f for f, _ in wg)), cen
            assert sum(calls.values()) == 0
        elif name == "X4":
            assert all(fwd) and all(dgr) and premask and cen["rowdot_ok"] and not cen["_head_fused_ok"], cen
            assert calls["head_fwd"] == calls["head_bwd"] == 0
        elif name == "X5":
            assert T > 256 and all(fwd) and all(dgr) and premask and not cen["rowdot_ok"], cen
            assert cen["_relu_bits_ok"] and cen["_colpart_ok"] and cen["_head_fused_ok"], cen
    check_rule(f"rule {name}", name, results)


# ---------------------------------------------------------------------------------------
# 3. step modes, bit for bit
# ---------------------------------------------------------------------------------------
STEP_SHAPES = {
    "T3-ragged": dict(TW.PAIR_MODEL, B=TW.PAIRS["T3"]["B_r"], T=TW.PAIRS["T3"]["T"]),
    "X1": dict(TW.SHAPES["X1"], T=TW.SHAPES["X1"]["T"][0]),
}
#        label              graph  segmented  DEFER  EARLY
MODES = [("one graph",      True,  False,     True,  True),
         ("eager",          False, False,     True,  True),
         ("segmented",      True,  True,      True,  True),
         ("deferral off",   True,  False,     False, True),
         ("early AdamW off", True, False,     True,  False)]


@pytest.mark.parametrize("shape", sorted(STEP_SHAPES))
def test_step_modes_bit_identical(shape):
    """engine.TrainStep, 2 steps after capture(restore=True), in every mode: the same losses, master
    weights and flat gradient bit for bit (test_gpu_train.py requires this at the C2 width).  Off the
    fast path the deferral flags sit on launches that decline them, the early AdamW jobs are queued
    where few or no persistent launches follow to host them, and the segment boundaries fall between
    generic launches."""
    from replicatinggpt_amd import AdamW, BigramLanguageModel
    from replicatinggpt_amd import functional as Fn
    from replicatinggpt_amd.data import BatchSampler, TokenStream
    from replicatinggpt_amd.engine import GradReducer, TrainStep
    s = STEP_SHAPES[shape]
    cfg = gpt_config(s, batch_size=s["B"])
    runs = []
    saved = Fn.DEFER.enabled, Fn.EARLY.enabled
    try:
        for label, graph, segmented, defer, early in MODES:
            Fn.DEFER.enabled, Fn.EARLY.enabled = defer, early
            torch.manual_seed(INIT_SEED)
            m = BigramLanguageModel(cfg).to(DEV)
            opt = AdamW(m.parameters(), lr=1e-3)
            sampler = BatchSampler(TokenStream.synthetic(device=DEV), s["T"], s["B"])
            red = GradReducer(m.flat.grad) if segmented else None   # world size 1: the segmentation only
            st = TrainStep(m, opt, sampler, red, use_graph=graph, overlap=segmented, seg_layers=1)
            st.capture(restore=True)
            losses = [float(st.step().detach()) for _ in range(2)]
            torch.cuda.synchronize()
            assert (st.g_fb is not None or bool(st.g_seg)) == graph and bool(st.g_seg) == segmented
            runs.append((label, losses, m.flat.master.detach().cpu().clone(), m.flat.grad.detach().cpu().clone()))
    finally:
        Fn.DEFER.enabled, Fn.EARLY.enabled = saved
    print(f"[modes {shape}] losses {runs[0][1]}")
    assert all(l == l and l > 0 for l in runs[0][1]) and bool(runs[0][3].any())
    for label, losses, master, grad in runs[1:]:
        same = losses == runs[0][1], torch.equal(master, runs[0][2]), torch.equal(grad, runs[0][3])
        print(f"[modes {shape}] {label} against one graph: losses / master / gradient equal = {same}")
        assert all(same), (shape, label, same)
