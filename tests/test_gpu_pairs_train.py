"""Fine-tuning on (prompt, completion) pairs end to end on the MI355X: data.PairSampler -> the masked loss
of model.forward(..., ignore_index) -> engine.TrainStep / Evaluator -> complete().

Gradients are judged by tests/trajectory.py's Checker -- its bars, unchanged: fp32 loss 1e-5 and per
parameter max|got - ref| / max|ref| < 1e-4 against oracle.gpt1_oracle.loss_and_grads (whose
F.cross_entropy ignores -100 by default); bf16 per parameter by norm e_c < max(2e-2, 1.25 e_t) with cosine
> 0.999, e_t the oracle's own forward under autocast(bfloat16) on the same GPU, loss within 1 %.  Shape E of
test_gpu_trajectory.py (B 16, T 64, d 128, 2 heads, 2 layers), dropout 0.  The sampler seed
(pairs.SAMPLER_SEED) is one at which torch's own bf16 path is inside that rule on the first batch -- the
"torch-bf16" records hold the calibration to it, as in test_gpu_trajectory.py.

test_cpu_pairs.py checks on the CPU that the oracle accepts these batches and that they have three
different valid counts on the first three steps."""
import numpy as np
import pytest
import torch

import pairs as pr
import trajectory as tj
from oracle import gpt1_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def gpt_config(dtype, shape=pr.E_SHAPE, **kw):
    from replicatinggpt_amd import GPTConfig
    s = dict(shape)
    B = s.pop("B", pr.E2E_B)
    return GPTConfig(dropout=0.0, dtype=dtype, batch_size=B, **s, **kw)


def setup(dtype, lr=1e-3, seed=1337):
    from replicatinggpt_amd import AdamW, BigramLanguageModel
    torch.manual_seed(seed)
    m = BigramLanguageModel(gpt_config(dtype)).to(DEV)
    opt = AdamW(m.parameters(), lr=lr)
    return m, opt, pr.train_sampler(DEV)


class _Shown:
    """What trajectory.Checker.check_grads needs of a trainer: one rank, the model's state by name."""

    world, rank = 1, 0

    def __init__(self, model):
        cfg = model.config
        self.dtype = cfg.dtype
        self.ocfg = O.OracleConfig(block_size=cfg.block_size, n_embd=cfg.n_embd, n_head=cfg.n_head,
                                   n_layers=cfg.n_layers, dropout=cfg.dropout)
        self.seed_base = cfg.dropout_seed
        self.master = {n: p.detach().cpu().numpy().copy() for n, p in model.named_parameters()}

    def snapshot(self):
        return tj.State(self.master, None, None, 0, 0)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_loss_and_gradients_match_the_oracle(dtype):
    from replicatinggpt_amd import functional as Fn
    m, _, s = setup(dtype)
    x, y = s.get_batch("train")
    g = torch.Generator().manual_seed(pr.SAMPLER_SEED)
    rx, ry = pr.reference_batch(pr.TRAIN_PAIRS, torch.randint(s.n, (s.B,), generator=g).tolist(), s.T)
    assert torch.equal(x.cpu(), rx) and torch.equal(y.cpu(), ry)
    share = pr.valid_share(ry)
    assert 0.25 <= share <= 0.75, share
    if dtype == "bf16":      # the fused head (cg_head_fwd_masked / cg_head_bwd_masked) is what runs
        assert Fn._head_fused_ok(torch.bfloat16, m._store.regions["lm_w"], s.B * s.T, m.config.n_embd, m.config.vocab_size)
    tr = _Shown(m)
    _, loss = m(x, y, ignore_index=s.ignore_index)
    loss.backward()
    torch.cuda.synchronize()
    obs = tj.Obs(rx, ry, float(loss.detach()), {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()},
                 None)
    ck = tj.Checker(tr)
    ck.check_grads("pairs", tr, tr.snapshot(), obs)
    for r in sorted(ck.records, key=lambda r: -(r.measured / r.bound if r.bound else 0))[:6]:
        print(f"{dtype} share {share:.3f}: {r.what} {r.name}: {r.measured:.3e} (bound {r.bound:.3e}) {'ok' if r.ok else 'FAIL'}")
    assert {r.what for r in ck.records} >= ({"loss", "grad"} if dtype == "fp32" else {"loss", "grad", "cosine", "torch-bf16"})
    assert not ck.failures(), ck.failures()


def _state(m, opt):
    torch.cuda.synchronize()
    return [t.detach().cpu().clone() for t in (m.flat.master, opt._m, opt._v)]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_graph_replay_follows_the_valid_count(dtype):
    """Three replayed steps whose batches have three different numbers of valid targets give an eager
    TrainStep's losses, weights and moments bit for bit: the normaliser is computed and read on the
    device at every replay, not baked in at capture."""
    from replicatinggpt_amd.engine import TrainStep
    runs = []
    for graph in (False, True):
        m, opt, s = setup(dtype)
        st = TrainStep(m, opt, s, use_graph=graph)
        st.capture(restore=True)
        assert (st.g_fb is not None) == graph
        losses, counts = [], []
        for _ in range(3):
            losses.append(st.step().detach().clone())
            counts.append(int((st.y != s.ignore_index).sum()))
        runs.append(([float(l) for l in losses], counts, _state(m, opt)))
    (l0, c0, s0), (l1, c1, s1) = runs
    assert c0 == c1 and len(set(c0)) == 3, (c0, c1)
    assert all(np.isfinite(l0)) and l0 == l1, (l0, l1)
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_evaluator_replay_is_the_eager_masked_loss(dtype):
    from replicatinggpt_amd.engine import Evaluator
    m, _, s = setup(dtype)
    m.eval()
    ev = Evaluator(m, s)
    counts = set()
    for split in ("train", "val", "train"):
        got = ev.loss(split).clone()
        assert ev.graph is not None
        with torch.no_grad():
            _, want = m(ev.x, ev.y, ignore_index=s.ignore_index)
        assert torch.isfinite(want) and torch.equal(got.view(torch.int32), want.view(torch.int32)), (float(got), float(want))
        counts.add(int((ev.y != s.ignore_index).sum()))
    assert len(counts) == 3


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_default_path_is_the_unmasked_one(dtype):
    """ignore_index=None with a BatchSampler: model.forward and a TrainStep step give the bits of
    HeadLossFn called as it was before it had the argument."""
    from replicatinggpt_amd import functional as Fn
    from replicatinggpt_amd.data import BatchSampler
    from replicatinggpt_amd.engine import TrainStep
    from replicatinggpt_amd.model import _act_dtype
    runs = []
    for how in ("model", "plain"):
        m, opt, _ = setup(dtype)
        s = BatchSampler(tj.synthetic_stream(DEV), m.config.block_size, pr.E_SHAPE["B"],
                         generator=torch.Generator().manual_seed(3))
        assert getattr(s, "ignore_index", None) is None
        assert TrainStep(m, opt, s, use_graph=False)._loss_kw == {}      # the engine passes nothing new either
        x, y = s.get_batch("train")
        if how == "model":
            _, loss = m(x, y)
        else:
            if dtype == "bf16":
                m._sync_shadow()
            R = m._store.regions
            h = m.blocks(Fn.EmbeddingFn.apply(x, R["wte"], R["wpe"], *R["wte"].params, *R["wpe"].params))
            lw, lb, hw, hb = R["lnf_w"], R["lnf_b"], R["lm_w"], R["lm_b"]
            _, loss = Fn.HeadLossFn.apply(h, y, _act_dtype(m.config), lw, lb, hw, hb, *lw.params, *lb.params, *hw.params,
                                          *hb.params)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        runs.append((loss.detach().cpu().clone(), m.flat.grad.detach().cpu().clone(), _state(m, opt)))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1], runs[1][1])
    for a, b in zip(runs[0][2], runs[1][2]):
        assert torch.equal(a, b)


def test_finetune_then_complete_returns_the_completions():
    """Four short pairs, a tiny fp32 model (T 16, d 32, 2 heads, 1 layer), AdamW at lr 1e-2, graph replay:
    after pairs.E2E_STEPS = 18 steps greedy complete() on the four prompts returns the four completions.
    The oracle's own AdamW loop on the same batches first reproduces them after pairs.E2E_ORACLE_STEPS = 9
    steps (test_cpu_pairs.py::test_oracle_finetune_fixes_the_step_count holds both numbers to the oracle);
    the product trains twice that."""
    from replicatinggpt_amd import AdamW, BigramLanguageModel
    from replicatinggpt_amd.engine import TrainStep
    torch.manual_seed(pr.E2E_INIT_SEED)
    m = BigramLanguageModel(gpt_config("fp32", pr.E2E_SHAPE)).to(DEV)
    opt = AdamW(m.parameters(), lr=pr.E2E_LR)
    st = TrainStep(m, opt, pr.e2e_sampler(DEV))
    st.capture(restore=True)
    losses = [float(st.step().detach()) for _ in range(pr.E2E_STEPS)]
    print("fine-tune losses", " ".join(f"{l:.3f}" for l in losses))
    assert losses[-1] < losses[0]
    m.eval()
    new = max(len(c) for _, c in pr.E2E_FOUR)
    with torch.no_grad():
        out = m.complete([torch.tensor(p) for p, _ in pr.E2E_FOUR], new, greedy=True)
    tokens = out.tokens.cpu()
    for b, (p, c) in enumerate(pr.E2E_FOUR):
        assert tokens[b, len(p):len(p) + len(c)].tolist() == c, (b, tokens[b].tolist(), c)
