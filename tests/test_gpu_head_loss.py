"""functional.HeadLossFn's call matrix on the MI355X, by bitwise relations only (no tolerances).

Two tiny models: fp32 (the plain path: cg_gemm + cg_ce_*) and bf16 with the packed store (the fused head,
cg_head_fwd / cg_head_bwd and their masked forms; _head_fused_ok is asserted).  V = 65; C = 32 (pairs.E2E_SHAPE:
the runtime-K loop of k_head_fwd) and C = 128 (pairs.E_SHAPE: KS = 4); B T = 80 rows -- two 64-row blocks, the
second partly empty, five 16-row waves.  A fixed random leaf ``h`` stands in for the block stack's output.

Three gradient modes: the loss alone; the logits alone (targets=None, backward of (logits * w).sum() for a fixed
random w); both (loss + (logits * w).sum()).

1. ignore_index = -100 with no target ignored gives the unmasked call's loss, logits, dx and every parameter
   gradient (m.flat.grad), in each mode that has targets.
2. With targets=None, passing ignore_index changes nothing.
3. The trailing-argument convention with ignore_index=None is the call that omits the argument.
4. A second backward into existing slots (beta = 1) doubles the bias gradient's slot exactly (x + x is exact);
   unmasked only."""
import pytest
import torch

import pairs as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, T, V = 5, 16, 65
M = B * T
OMIT = "omit"          # HeadLossFn.apply called without the trailing argument
SHAPES = {32: pr.E2E_SHAPE, 128: {k: v for k, v in pr.E_SHAPE.items() if k != "B"}}
CASES = [(dt, C) for dt in ("fp32", "bf16") for C in SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


_MODELS, _RUNS = {}, {}


def model(dtype, C):
    if (dtype, C) not in _MODELS:
        from replicatinggpt_amd import BigramLanguageModel, GPTConfig
        torch.manual_seed(1337)
        m = BigramLanguageModel(GPTConfig(dropout=0.0, dtype=dtype, batch_size=B, **SHAPES[C])).to(DEV)
        g = torch.Generator().manual_seed(11 + C)
        _MODELS[(dtype, C)] = (m, torch.randn(B, T, C, generator=g).to(DEV), torch.randint(0, V, (B, T), generator=g).to(DEV),
                               torch.randn(M, V, generator=g).to(DEV))
    return _MODELS[(dtype, C)]


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def one_pass(dtype, C, mode, tail):
    """One forward and backward of HeadLossFn on the fixed inputs; gradients go where they are told to."""
    from replicatinggpt_amd import functional as Fn
    from replicatinggpt_amd.model import _act_dtype
    m, h0, y, w = model(dtype, C)
    if dtype == "bf16":
        m._sync_shadow()
    R = m.flat.regions
    lw, lb, hw, hb = R["lnf_w"], R["lnf_b"], R["lm_w"], R["lm_b"]
    assert Fn._head_fused_ok(_act_dtype(m.config), hw, M, C, V) == (dtype == "bf16")
    h = h0.clone().requires_grad_(True)
    out = Fn.HeadLossFn.apply(h, None if mode == "logits" else y, _act_dtype(m.config), lw, lb, hw, hb, *lw.params,
                              *lb.params, *hw.params, *hb.params, *(() if tail == OMIT else (tail,)))
    if mode == "logits":
        logits, loss = out, None
        assert logits.shape == (B, T, V)
        obj = (logits * w.view(B, T, V)).sum()
    else:
        logits, loss = out
        assert logits.shape == (M, V)
        obj = loss if mode == "loss" else loss + (logits * w).sum()
    obj.backward()
    torch.cuda.synchronize()
    return {"loss": None if loss is None else bits(loss), "logits": bits(logits.reshape(M, V)), "dx": bits(h.grad),
            "grad": bits(m.flat.grad), "db": bits(hb.slot)}


def run(dtype, C, mode, tail):
    """one_pass into a fresh gradient state, once per case (the results are compared, never modified)."""
    key = (dtype, C, mode, tail)
    if key not in _RUNS:
        m = model(dtype, C)[0]
        m.zero_grad(set_to_none=True)
        m.flat.grad.zero_()
        _RUNS[key] = one_pass(dtype, C, mode, tail)
    return _RUNS[key]


def assert_same(a, b, what):
    for k in ("loss", "logits", "dx", "grad"):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("mode", ["loss", "both"])
@pytest.mark.parametrize("dtype,C", CASES)
def test_nothing_ignored_is_the_unmasked_call(dtype, C, mode):
    got, want = run(dtype, C, mode, pr.IGNORE), run(dtype, C, mode, OMIT)
    assert want["grad"].any() and want["dx"].any()
    assert_same(got, want, (dtype, C, mode))


@pytest.mark.parametrize("dtype,C", CASES)
def test_ignore_index_without_targets_changes_nothing(dtype, C):
    assert_same(run(dtype, C, "logits", pr.IGNORE), run(dtype, C, "logits", OMIT), (dtype, C))


@pytest.mark.parametrize("mode", ["loss", "logits", "both"])
@pytest.mark.parametrize("dtype,C", CASES)
def test_trailing_none_is_the_call_without_the_argument(dtype, C, mode):
    assert_same(run(dtype, C, mode, None), run(dtype, C, mode, OMIT), (dtype, C, mode))


@pytest.mark.parametrize("mode", ["loss", "logits", "both"])
@pytest.mark.parametrize("dtype,C", CASES)
def test_second_backward_doubles_the_bias_gradient(dtype, C, mode):
    first = run(dtype, C, mode, OMIT)
    m = model(dtype, C)[0]
    m.zero_grad(set_to_none=True)
    m.flat.grad.zero_()
    one_pass(dtype, C, mode, OMIT)                 # beta 0: the slots are assigned as the .grad of their parameters
    assert m.lm_head.bias.grad.data_ptr() == m.flat.regions["lm_b"].slot.data_ptr()
    second = one_pass(dtype, C, mode, OMIT)        # beta 1: accumulated into them
    x = first["db"].view(torch.float32)
    assert x.abs().max() > 0
    assert torch.equal(second["db"], bits(x + x))
