"""Every gradient-destination state of the training backward against the oracle.

The backward's kernels write parameter gradients themselves, into the destination
functional.Region.grad_target() picks from the state of ``p.grad``: the flat slot overwritten
(beta 0), the flat slot accumulated onto (beta 1), a temporary handed back to autograd, or nothing.
Here one small shape per dtype is fixed and the gradient state varies: micro-batches A then B on
one model (dropout calls 0 and 1), with ``p.grad`` left alone, zeroed in place, dropped for some
parameters, replaced by copies, or the parameters frozen.

References and bars (none invented here): the fp32 path against the fp32 CPU oracle, per parameter
max-abs error over max-abs reference < 1e-4 and the loss within 1e-5 -- the bars of
test_gpu_model.py::test_dropout_model_matches_oracle_fp32, on data whose oracle gradients
tests/test_cpu_grad_targets.py shows stable to 1e-5; the bf16 path by the rule of
test_c2_full_size_bf16_step_matches_oracle, per parameter by norm e_c < max(2e-2, 1.25 e_t) with
cosine > 0.999, e_t the error of the oracle's forward under torch.autocast(bfloat16) on the same GPU
for the same combination of micro-batches (bf16 loss within 1 %, the bar of
test_c2_full_size_bf16_step_close_to_fp32).  Run with -s for the worst (name, e_c, e_t) per scenario.

Measured on MI355X (profiles/grad_targets_gpu_tests.txt): the fp32 paths are within 1.1e-6 of the
oracle in every scenario.  On E-bf16 the LayerNorm-2 / FFN-1 parameters sit at e_c 3.4e-2 .. 4.5e-2
with torch's own bf16 path at 3.4e-2 .. 4.4e-2 (the flipped ReLU decisions of DESIGN section 2, as at
C2), every other parameter under 1.4e-2; the lowest cosine of any checked tensor is 0.999012 (scenario 4,
blocks.1.ln2.weight = g(B) alone; torch 0.999106).  A norm error e means a cosine of about 1 - e^2 / 2,
so the 0.999 rule is an absolute e < 4.5e-2 and these parameters are close to it: micro-batch B ALONE
gives blocks.0.ln2.weight e_c 4.64e-2 / cosine 0.998924 (torch 4.36e-2 / 0.999050).  No scenario below
expects that tensor alone -- B enters in sums, and bit for bit in scenario 3.

Every bf16 run here takes every fast branch (build() asserts it).  The bf16 fallbacks -- generic GEMMs and
attention, the plain head, weight gradients that decline slabs and deferral, the ring attention -- run
inside a model in tests/test_gpu_bf16_offpath.py.
"""
import functools

import pytest
import torch

from oracle import gpt1_oracle as O
from test_cpu_grad_targets import CASES, DROPOUT, INIT_SEED, N_LAYERS, micro_batches, oracle_config, oracle_params

pytestmark = pytest.mark.gpu
DEV = "cuda"

PATHS = [("E", "bf16"), ("E", "fp32"), ("O", "fp32")]
PATH_IDS = ["E-bf16", "E-fp32", "O-fp32"]
E_PATHS = PATHS[:2]

# one member of each kind of region (scenarios 4 and 5)
MEMBERS = [
    "blocks.0.ln1.bias",                        # LayerNorm bias, its weight kept
    "blocks.1.ln2.weight",                      # LayerNorm weight, its bias kept
    "blocks.1.sa_heads.heads.1.key.weight",     # one part of the multi-part QKV region
    "blocks.0.sa_heads.proj.bias",              # GradLink column-sum targets
    "blocks.1.ffwd.net.2.bias",
    "blocks.0.ffwd.net.0.bias",                 # column-partial reduce
    "token_embedding_table.weight",             # wpe kept
    "lm_head.bias",
    "lm_head.weight",
]
FROZEN = [
    "blocks.0.ln1.bias",
    "blocks.1.ln2.weight",
    "blocks.0.sa_heads.heads.0.query.weight",
    "blocks.0.sa_heads.proj.bias",
    "blocks.0.ffwd.net.0.bias",
    "blocks.1.ffwd.net.0.weight", "blocks.1.ffwd.net.0.bias",     # one whole FeedForward
    "blocks.1.ffwd.net.2.weight", "blocks.1.ffwd.net.2.bias",
    "token_embedding_table.weight",
    "lm_head.bias",
    "lm_head.weight",
]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


# ---------------------------------------------------------------------------------------
# models, data, references (each computed once and never modified)
# ---------------------------------------------------------------------------------------
def gpt_config(shape, dtype):
    from replicatinggpt_amd import GPTConfig
    c = CASES[shape]
    return GPTConfig(block_size=c["block_size"], n_embd=c["n_embd"], n_head=c["n_head"], n_layers=N_LAYERS,
                     dropout=DROPOUT, dtype=dtype)


def build(shape, dtype):
    from replicatinggpt_amd import BigramLanguageModel
    torch.manual_seed(INIT_SEED)
    m = BigramLanguageModel(gpt_config(shape, dtype)).to(DEV)
    assert m.training
    if dtype == "bf16":   # every bf16 test here is about the fast branches: fail, never skip, if one is not taken
        preds = fast_branches(m)
        assert all(preds.values()), preds
    return m


def fast_branches(m):
    """The training path's dispatch predicates for model ``m`` at its case's micro-batch size, asked
    from the library's own functions: the LN + keep-bit launch, the ReLU keep bits, the column
    partials, the ROWDOT dgrad, the grouped split-K weight gradients (split > 1 for both sublayer
    pairs), the fused head -- and the deferral and bf16-slab switches at their defaults."""
    from replicatinggpt_amd import functional as Fn
    cfg = m.config
    shape = next(k for k, c in CASES.items() if (c["block_size"], c["n_embd"]) == (cfg.block_size, cfg.n_embd))
    T, C, H = cfg.block_size, cfg.n_embd, cfg.n_head
    M, D, F4 = CASES[shape]["B"] * T, C // H, 4 * C
    R = m._store.regions
    bf = torch.bfloat16
    a = torch.zeros((M, C), dtype=bf, device=DEV)
    h = torch.zeros((M, F4), dtype=bf, device=DEV)
    w1, w2, wp = R["0.w1"].operand(bf), R["0.w2"].operand(bf), R["0.proj_w"].operand(bf)
    preds = {
        "premask_ok (LN + keep-bit launch, MFMA attention)": Fn.premask_ok(bf, T, D) and Fn.LN_MASK
        and not Fn.SIDE.premask,
        "_relu_bits_ok": Fn._relu_bits_ok(a, w1, w2, F4),
        "_colpart_ok": Fn._colpart_ok(a, w2, h, F4),
        "rowdot_ok": Fn.rowdot_ok(a, wp, a, T, D),
        "_head_fused_ok": Fn._head_fused_ok(bf, R["lm_w"], M, C, cfg.vocab_size),
        "_wgrad_group_on": Fn._wgrad_group_on(bf) and bool(Fn.WGRAD_GROUP_FFN),
        "attention pair: _split_for_tiles > 1": Fn._split_for_tiles((C // 128) ** 2 + (3 * C // 128) * (C // 128),
                                                                    M // 64) > 1,
        "FeedForward pair: _split_for_tiles > 1": Fn._split_for_tiles(2 * (F4 // 128) * (C // 128), M // 64) > 1,
        "DEFER enabled": Fn.DEFER.enabled and Fn.DEFER.partials_on,
        "bf16 slabs": bool(Fn.SLAB_BF16),
    }
    return {k: bool(v) for k, v in preds.items()}


@functools.lru_cache(maxsize=None)
def batches(shape):
    return [(i.to(DEV), t.to(DEV)) for i, t in micro_batches(shape)]


def _oracle_run(P, idx, tgt, shape, call, frozen):
    seed = gpt_config(shape, "fp32").dropout_seed
    if not frozen:
        _, loss, grads = O.loss_and_grads(P, idx, tgt, oracle_config(shape), train=True, seed=seed, call=call)
        return float(loss), grads
    # the same run with the frozen leaves detached
    leaf = {k: v.detach().clone().requires_grad_(k not in frozen) for k, v in P.items()}
    _, loss = O.forward(leaf, idx, oracle_config(shape), tgt, True, seed, call)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in leaf.items()}


@functools.lru_cache(maxsize=None)
def oracle(shape, frozen=()):
    """[(loss, {name: grad})] of the fp32 CPU oracle for micro-batches A (call 0) and B (call 1)."""
    P = oracle_params(shape)
    return [_oracle_run(P, idx, tgt, shape, call, frozen) for call, (idx, tgt) in enumerate(micro_batches(shape))]


@functools.lru_cache(maxsize=None)
def torch_bf16(shape, frozen=()):
    """The same from the oracle's functional forward under autocast(bfloat16) on the GPU: the
    calibration of the bf16 bar."""
    P = {k: v.to(DEV) for k, v in oracle_params(shape).items()}
    out = []
    for call, (idx, tgt) in enumerate(batches(shape)):
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            loss, grads = _oracle_run(P, idx, tgt, shape, call, frozen)
        out.append((loss, {k: (None if g is None else g.double().cpu()) for k, g in grads.items()}))
    return out


def run(m, batch, defer=False):
    """One forward / backward of ``m``; the loss as a float."""
    from replicatinggpt_amd import functional as Fn
    _, loss = m(*batch)
    if defer:
        with Fn.DEFER:   # as engine.TrainStep runs its backward
            loss.backward()
    else:
        loss.backward()
    return float(loss.detach())


def grads_of(m):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


@functools.lru_cache(maxsize=None)
def fresh(shape, dtype):
    """G_A and G_B from overwriting backwards (every .grad None) of one model: A as call 0, then
    zero_grad(set_to_none=True), then B as call 1."""
    m = build(shape, dtype)
    A, B = batches(shape)
    la = run(m, A)
    ga = grads_of(m)
    m.zero_grad(set_to_none=True)
    lb = run(m, B)
    return (la, ga), (lb, grads_of(m))


@functools.lru_cache(maxsize=None)
def accumulated(shape, dtype, defer=False):
    """backward(A), backward(B) on one model with .grad left alone in between."""
    m = build(shape, dtype)
    A, B = batches(shape)
    la = run(m, A, defer)
    only_a = grads_of(m)
    lb = run(m, B, defer)
    return (la, lb), only_a, grads_of(m)


# ---------------------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def combine(per_batch, only_b=()):
    """g(A) + g(B) per parameter in fp64, g(B) alone for the names in ``only_b``."""
    (_, ga), (_, gb) = per_batch
    return {k: (gb[k].double() if k in only_b else ga[k].double() + gb[k].double()) for k in ga}


def check_loss(shape, dtype, got, call, frozen=()):
    ref = oracle(shape, frozen)[call][0]
    if dtype == "fp32":
        assert abs(got - ref) < 1e-5, (call, got, ref)
    else:
        assert abs(got - ref) < 1e-2 * ref, (call, got, ref)


def check_grads(label, shape, dtype, got, expect, expect_t=None):
    """``got`` {name: gradient} against ``expect`` {name: fp64 oracle combination}; bf16: ``expect_t``
    the same combination of torch's bf16 path."""
    assert set(got) == set(expect)
    rows = []
    if dtype == "fp32":
        for name, g in got.items():
            rows.append((name, relerr(g, expect[name])))
        worst = max(rows, key=lambda r: r[1])
        print(f"[{label} {shape}-{dtype}] worst (name, relerr) = ({worst[0]}, {worst[1]:.3e})")
        bad = [r for r in rows if not r[1] < 1e-4]
        assert not bad, (label, bad)
        return
    for name, g in got.items():
        a, b = g.double().cpu().flatten(), expect[name].flatten()
        e_c = float((a - b).norm() / b.norm())
        e_t = float((expect_t[name].flatten() - b).norm() / b.norm())
        cos = float(torch.nn.functional.cosine_similarity(a, b, dim=0))
        rows.append((name, e_c, e_t, cos))
    worst = max(rows, key=lambda r: r[1] / max(2e-2, 1.25 * r[2]))
    print(f"[{label} {shape}-{dtype}] worst (name, e_c, e_t) = ({worst[0]}, {worst[1]:.3e}, {worst[2]:.3e}); "
          f"lowest cosine {min(r[3] for r in rows):.6f}")
    bad = [r for r in rows if not (r[1] < max(2e-2, 1.25 * r[2]) and r[3] > 0.999)]
    assert not bad, (label, bad)


def check_sum(label, shape, dtype, got, only_b=()):
    check_grads(label, shape, dtype, got, combine(oracle(shape), only_b),
                combine(torch_bf16(shape), only_b) if dtype == "bf16" else None)


def assert_equal_grads(a, b):
    assert set(a) == set(b)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def stale_slots(m, shape):
    """Three backwards and zero_grad(set_to_none=True): every flat slot holds a stale nonzero
    gradient, every .grad is None, and the dropout call counter is back at 0 (so the micro-batches
    that follow are calls 0 and 1 again, the oracle's)."""
    A, B = batches(shape)
    for batch in (A, B, A):
        run(m, batch)
        m.zero_grad(set_to_none=True)
    m._rng_counter.zero_()
    assert float(m._store.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------
# the bf16 shape really takes the fast branches
# ---------------------------------------------------------------------------------------
def test_e_bf16_takes_every_fast_branch(monkeypatch):
    """Shape E on the bf16 path: the library's own predicates say the LN + keep-bit launch, the ReLU
    keep bits, the column partials, the ROWDOT dgrad, the grouped split-K weight gradients (split > 1
    for both sublayer pairs) and the fused head are taken -- and one training step calls each of them."""
    from replicatinggpt_amd import functional as Fn
    from replicatinggpt_amd import ops
    m = build("E", "bf16")   # asserts the predicates
    for name, ok in fast_branches(m).items():
        print(f"[branches E-bf16] {name}: {ok}")
    # the fp32 path of the same shape: the generic split-K engages for every weight gradient
    c = CASES["E"]
    M, C = c["B"] * c["block_size"], c["n_embd"]
    splits = {k: Fn._wgrad_split(n, C * kc, M, False) for k, n, kc in
              (("proj", C, 1), ("qkv", 3 * C, 1), ("w1", 4 * C, 1), ("w2", C, 4))}
    print(f"[branches E-fp32] split-K of the weight gradients: {splits}")
    assert all(s > 1 for s in splits.values()), splits
    # ... and a bf16 step goes through the fast branches
    calls = {}
    for fn in ("layernorm_fwd_attn_dropmask", "gemm_bias_relu_bits", "gemm_relu_bwd_colpart", "gemm_store_rowdot",
               "gemm_wgrad_group", "head_fwd", "head_bwd"):
        def spy(*args, _fn=fn, _real=getattr(ops, fn), **kw):
            calls[_fn] = calls.get(_fn, 0) + 1
            return _real(*args, **kw)
        monkeypatch.setattr(ops, fn, spy)
    run(m, batches("E")[0], defer=True)
    torch.cuda.synchronize()
    print(f"[branches E-bf16] launches in one step: {calls}")
    assert calls == {"layernorm_fwd_attn_dropmask": N_LAYERS, "gemm_bias_relu_bits": N_LAYERS,
                     "gemm_relu_bwd_colpart": N_LAYERS, "gemm_store_rowdot": N_LAYERS,
                     "gemm_wgrad_group": 2 * N_LAYERS, "head_fwd": 1, "head_bwd": 1}


# ---------------------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", PATHS, ids=PATH_IDS)
def test_1_fresh(shape, dtype):
    """Every .grad None: the slots are overwritten with g(A).  The control, and the oracle check of
    the bf16 fast path at a small shape."""
    loss, got = fresh(shape, dtype)[0]
    check_loss(shape, dtype, loss, 0)
    check_grads("fresh", shape, dtype, got, {k: g.double() for k, g in oracle(shape)[0][1].items()},
                torch_bf16(shape)[0][1] if dtype == "bf16" else None)


@pytest.mark.parametrize("shape,dtype", PATHS, ids=PATH_IDS)
def test_2_accumulate(shape, dtype):
    """No zero_grad between the two backwards: every kernel accumulates (beta 1) onto its slot."""
    (la, lb), only_a, got = accumulated(shape, dtype)
    check_loss(shape, dtype, la, 0)
    check_loss(shape, dtype, lb, 1)
    check_sum("accumulate", shape, dtype, got)
    if shape == "O":   # micro-batch B is shorter than block_size: the wpe rows past its T are g(A)'s, untouched
        T = CASES[shape]["T"][1]
        name = "position_embedding_table.weight"
        assert torch.equal(got[name][T:], only_a[name][T:])
        assert float(only_a[name][T:].abs().max()) > 0


@pytest.mark.parametrize("shape,dtype", PATHS, ids=PATH_IDS)
def test_2_accumulate_deferred_is_bitwise_the_same(shape, dtype):
    """The same inside ``with DEFER:`` (pending split-K reduces, queued column-sum reduces): same
    summation order, same bits."""
    losses, only_a, got = accumulated(shape, dtype)
    losses_d, only_a_d, got_d = accumulated(shape, dtype, True)
    assert losses == losses_d
    assert_equal_grads(only_a, only_a_d)
    assert_equal_grads(got, got_d)


@pytest.mark.parametrize("shape,dtype", PATHS, ids=PATH_IDS)
def test_3_zero_in_place(shape, dtype):
    """zero_grad(set_to_none=False) keeps the slot views: backward(B) accumulates onto exact zeros,
    which is exact -- so it equals, bit for bit, the overwriting backward(B) of a model that ran A
    and dropped its gradients.  A difference is a slot region skipped or added twice."""
    from replicatinggpt_amd import AdamW
    m = build(shape, dtype)
    opt = AdamW(m.parameters(), lr=1e-3).attach(m)
    A, B = batches(shape)
    run(m, A)
    opt.zero_grad(set_to_none=False)
    assert all(p.grad is not None and not bool(p.grad.any()) for p in m.parameters())
    lb = run(m, B)
    got = grads_of(m)
    (_, _), (lb_ref, gb_ref) = fresh(shape, dtype)
    assert lb == lb_ref
    assert_equal_grads(got, gb_ref)
    if shape == "O":
        T = CASES[shape]["T"][1]
        rest = got["position_embedding_table.weight"][T:]
        assert rest.numel() > 0 and not bool(rest.any())


@pytest.mark.parametrize("shape,dtype", PATHS, ids=PATH_IDS)
def test_4_mixed(shape, dtype):
    """backward(A), then ``.grad = None`` on one member of each kind of region, then backward(B), on
    slots that held stale gradients before: g(B) for those members (their slot overwritten, or for
    the QKV part a temporary), g(A) + g(B) for everything else -- including each member's partner
    in the same kernel (the LayerNorm's other parameter, wpe, the other QKV parts)."""
    m = build(shape, dtype)
    stale_slots(m, shape)
    A, B = batches(shape)
    check_loss(shape, dtype, run(m, A), 0)
    params = dict(m.named_parameters())
    for name in MEMBERS:
        params[name].grad = None
    check_loss(shape, dtype, run(m, B), 1)
    check_sum("mixed", shape, dtype, grads_of(m), only_b=MEMBERS)


@pytest.mark.parametrize("shape,dtype", PATHS, ids=PATH_IDS)
def test_5_strays(shape, dtype):
    """backward(A), then ``p.grad = p.grad.clone()`` for the same members, then backward(B): their
    regions go to temporaries that autograd adds to the copies -- g(A) + g(B) everywhere.  Then
    AdamW.step() copies the strays into their flat slots."""
    from replicatinggpt_amd import AdamW
    m = build(shape, dtype)
    opt = AdamW(m.parameters(), lr=1e-3).attach(m)
    stale_slots(m, shape)
    A, B = batches(shape)
    run(m, A)
    params = dict(m.named_parameters())
    for name in MEMBERS:
        params[name].grad = params[name].grad.clone()
    run(m, B)
    got = grads_of(m)
    check_sum("strays", shape, dtype, got)
    st = m._store
    before = st.master.clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(st.master, before)
    for r in st.regions.values():
        for p, off in r.parts:
            slot = r.slot.view(-1)[off:off + p.numel()].view(p.shape)
            assert torch.equal(slot, p.grad)
    for name in MEMBERS:   # still copies, and the step did not disturb them
        assert params[name].grad.data_ptr() < st.grad.data_ptr() or \
            params[name].grad.data_ptr() >= st.grad.data_ptr() + 4 * st.grad.numel()
        assert torch.equal(params[name].grad, got[name])


@pytest.mark.parametrize("shape,dtype", PATHS, ids=PATH_IDS)
def test_6_frozen(shape, dtype):
    """requires_grad False on one member of each kind of region (a whole FeedForward and one head's
    query weight among them) before the first forward: those keep ``.grad is None``, all others match
    g(A) of an oracle run with the same leaves detached."""
    m = build(shape, dtype)
    params = dict(m.named_parameters())
    for name in FROZEN:
        params[name].requires_grad_(False)
    frozen = tuple(FROZEN)
    check_loss(shape, dtype, run(m, batches(shape)[0]), 0, frozen)
    got = grads_of(m)
    for name in FROZEN:
        assert got.pop(name) is None, name
    ref = {k: g.double() for k, g in oracle(shape, frozen)[0][1].items() if g is not None}
    assert set(ref) == set(params) - set(FROZEN)
    ref_t = torch_bf16(shape, frozen)[0][1] if dtype == "bf16" else None
    check_grads("frozen", shape, dtype, got, ref, ref_t)


@pytest.mark.parametrize("shape,dtype", E_PATHS, ids=PATH_IDS[:2])
def test_7_additivity(shape, dtype):
    """The accumulated gradient against G_A + G_B of the same path's own overwriting backwards,
    formed in fp64.  The accumulating kernels differ from that only by reassociating at most 33 fp32
    additions (split <= 32, plus the old value), so every element is within
    64 * 2^-24 * (max|G_A| + max|G_B|) of it -- far inside the oracle bars: a beta applied to part of
    a tile set shows here."""
    (_, ga), (_, gb) = fresh(shape, dtype)
    _, _, got = accumulated(shape, dtype)
    rows = []
    for name, g in got.items():
        a, b = ga[name].double(), gb[name].double()
        bound = 64 * 2.0 ** -24 * (float(a.abs().max()) + float(b.abs().max()))
        rows.append((name, float((g.double() - (a + b)).abs().max()), bound))
    worst = max(rows, key=lambda r: r[1] / r[2])
    print(f"[additivity {shape}-{dtype}] worst (name, max error, bound) = ({worst[0]}, {worst[1]:.3e}, {worst[2]:.3e})")
    for name, err, bound in rows:
        assert err <= bound, (name, err, bound)
