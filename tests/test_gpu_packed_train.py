"""Packed rows at the model level on the MI355X: model.forward(..., seg_start=) against the oracle run on
every segment alone (packing.packed_oracle), engine.TrainStep / Evaluator replaying batches with different
segmentations, fine-tuning on packed rows end to end, and the unpacked path left bit for bit alone.

Bars (tests/trajectory.py's constants, unchanged): fp32 loss 1e-5, logits and every parameter gradient
max|got - ref| / max|ref| < 1e-4; bf16 loss within 1 %, per parameter by norm e_c < max(2e-2, 1.25 e_t)
with cosine > 0.999, e_t the packed oracle's own error under autocast(bfloat16) on the same GPU, which must
itself be inside the cosine rule on the chosen batch (packing.PACKED_SAMPLER_SEED)."""
import numpy as np
import pytest
import torch

import packing as PK
import pairs as PR
import trajectory as tj
from oracle import gpt1_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def gpt_config(dtype, shape, dropout=0.0):
    from replicatinggpt_amd import GPTConfig
    s = dict(shape)
    B = s.pop("B", PK.E2E_B)
    return GPTConfig(dropout=dropout, dtype=dtype, batch_size=B, **s)


def oracle_of(model):
    cfg = model.config
    ocfg = O.OracleConfig(block_size=cfg.block_size, n_embd=cfg.n_embd, n_head=cfg.n_head, n_layers=cfg.n_layers,
                          dropout=0.0)
    return ocfg, {n: p.detach().cpu().clone() for n, p in model.named_parameters()}


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_fp32_logits_loss_and_gradients_match_the_packed_oracle():
    """The generic kernels' model (block 16, n_embd 32, 2 heads of 16, 1 layer): rows of two or three
    short segments and a padding tail."""
    from replicatinggpt_amd import BigramLanguageModel
    from replicatinggpt_amd.data import PackedPairSampler
    torch.manual_seed(PK.E2E_INIT_SEED)
    m = BigramLanguageModel(gpt_config("fp32", PR.E2E_SHAPE)).to(DEV)
    s = PackedPairSampler(PR.E2E_PAIRS, 16, 4, generator=torch.Generator().manual_seed(2), device=DEV)
    x, y, seg = s.get_batch("train")
    assert all(2 <= len(PK.segments(r)) for r in seg.cpu())
    ocfg, P = oracle_of(m)
    rlog, rloss, rg = PK.packed_oracle(P, x.cpu(), y.cpu(), seg.cpu(), ocfg)
    with torch.no_grad():    # no targets, no autograd: the same kernels, the logits of every position
        logits, none = m(x, seg_start=seg)
    assert none is None and relmax(logits, rlog) < tj.FP32_GRAD
    lg2, loss = m(x, y, ignore_index=s.ignore_index, seg_start=seg)
    loss.backward()
    torch.cuda.synchronize()
    assert relmax(lg2.view(logits.shape), rlog) < tj.FP32_GRAD
    assert abs(float(loss) - float(rloss)) < tj.FP32_LOSS, (float(loss), float(rloss))
    worst = {n: relmax(p.grad, rg[n]) for n, p in m.named_parameters()}
    print("fp32 packed: worst", max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) < tj.FP32_GRAD, worst
    # and the unpacked forward of the same tokens is something else: the mask is not a no-op here
    with torch.no_grad():
        assert relmax(m(x)[0], rlog) > 1e-2


LONG_F32_SHAPE = dict(block_size=160, n_embd=42, n_head=2, n_layers=1, B=2)


def test_fp32_long_rows_match_the_packed_oracle():
    """Rows of 160 tokens holding eight to twelve pairs (2 heads of 21, 1 layer): the fp32 MFMA forward
    under a segment mask over three key tiles, segments that start beyond keys 64 and 128, and wpe
    positions that restart beyond index 64.  Bars as test_fp32_logits_loss_and_gradients_match_the_packed_oracle."""
    from replicatinggpt_amd import BigramLanguageModel
    from replicatinggpt_amd.data import PackedPairSampler
    torch.manual_seed(PK.E2E_INIT_SEED)
    m = BigramLanguageModel(gpt_config("fp32", LONG_F32_SHAPE)).to(DEV)
    s = PackedPairSampler(PK.PACKED_PAIRS, 160, 2, generator=torch.Generator().manual_seed(2), device=DEV)
    x, y, seg = s.get_batch("train")
    nseg = [len(PK.segments(r)) for r in seg.cpu()]
    print("segments per row", nseg)
    assert min(nseg) >= 6, nseg
    assert all(max(a for a, _ in PK.segments(r)) >= 128 for r in seg.cpu())
    ocfg, P = oracle_of(m)
    rlog, rloss, rg = PK.packed_oracle(P, x.cpu(), y.cpu(), seg.cpu(), ocfg)
    with torch.no_grad():
        logits, none = m(x, seg_start=seg)
    assert none is None and relmax(logits, rlog) < tj.FP32_GRAD
    lg2, loss = m(x, y, ignore_index=s.ignore_index, seg_start=seg)
    loss.backward()
    torch.cuda.synchronize()
    assert relmax(lg2.view(logits.shape), rlog) < tj.FP32_GRAD
    assert abs(float(loss) - float(rloss)) < tj.FP32_LOSS, (float(loss), float(rloss))
    worst = {n: relmax(p.grad, rg[n]) for n, p in m.named_parameters()}
    print("fp32 packed, long rows: worst", max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) < tj.FP32_GRAD, worst
    with torch.no_grad():
        assert relmax(m(x)[0], rlog) > 1e-2


def test_bf16_loss_and_gradients_match_the_packed_oracle():
    """Shape E (block 64, n_embd 128, 2 heads of 64: the sequence-resident kernels, 2 layers), rows of
    three to five segments."""
    from replicatinggpt_amd import BigramLanguageModel
    torch.manual_seed(1337)
    m = BigramLanguageModel(gpt_config("bf16", PK.E_SHAPE)).to(DEV)
    s = PK.packed_train_sampler(DEV)
    x, y, seg = s.get_batch("train")
    nseg = [len(PK.segments(r)) for r in seg.cpu()]
    assert min(nseg) >= 3, nseg
    ocfg, P = oracle_of(m)
    _, rloss, rg = PK.packed_oracle(P, x.cpu(), y.cpu(), seg.cpu(), ocfg)
    _, tloss, tg = PK.packed_oracle(P, x, y, seg, ocfg, device=DEV, autocast=True)
    _, loss = m(x, y, ignore_index=s.ignore_index, seg_start=seg)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(rloss)) < tj.BF16_LOSS * float(rloss), (float(loss), float(rloss))
    bad = []
    for n, p in m.named_parameters():
        a, b, t = (v.detach().double().cpu().numpy().ravel() for v in (p.grad, rg[n], tg[n]))
        nb = np.linalg.norm(b)
        e_c, e_t = np.linalg.norm(a - b) / nb, np.linalg.norm(t - b) / nb
        cos, cos_t = a @ b / (np.linalg.norm(a) * nb), t @ b / (np.linalg.norm(t) * nb)
        print(f"bf16 packed {n}: e_c {e_c:.3e} e_t {e_t:.3e} 1-cos {1 - cos:.2e} torch 1-cos {1 - cos_t:.2e}")
        if not cos_t > tj.BF16_COS:
            bad.append((n, "torch-bf16: the seed is no fair test", 1 - cos_t))
        if not e_c < max(tj.BF16_FLOOR, tj.BF16_SLACK * e_t):
            bad.append((n, "grad", e_c, e_t))
        if not cos > tj.BF16_COS:
            bad.append((n, "cosine", 1 - cos))
    assert not bad, bad


def _state(m, opt):
    torch.cuda.synchronize()
    return [t.detach().cpu().clone() for t in (m.flat.master, opt._m, opt._v)]


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_graph_replay_follows_the_segmentation(dtype):
    """Three replayed steps are an eager TrainStep's, bit for bit -- losses, weights, moments -- with
    attention dropout 0.2 on and three batches of different segmentations and valid counts: seg_start is
    read on the device at every replay."""
    from replicatinggpt_amd import AdamW, BigramLanguageModel
    from replicatinggpt_amd.engine import TrainStep
    runs = []
    for graph in (False, True):
        torch.manual_seed(1337)
        m = BigramLanguageModel(gpt_config(dtype, PK.E_SHAPE, dropout=0.2)).to(DEV)
        opt = AdamW(m.parameters(), lr=1e-3)
        s = PK.packed_train_sampler(DEV)
        st = TrainStep(m, opt, s, use_graph=graph)
        assert st._loss_kw["seg_start"] is st.seg and st.seg.dtype == torch.int32
        st.capture(restore=True)
        assert (st.g_fb is not None) == graph
        losses, segs = [], []
        for _ in range(3):
            losses.append(float(st.step().detach()))
            segs.append(st.seg.cpu().clone())
        runs.append((losses, segs, _state(m, opt)))
    (l0, g0, s0), (l1, g1, s1) = runs
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert not torch.equal(g0[0], g0[1]) and not torch.equal(g0[1], g0[2])
    assert all(np.isfinite(l0)) and l0 == l1, (l0, l1)
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_evaluator_replay_is_the_eager_packed_loss(dtype):
    from replicatinggpt_amd import BigramLanguageModel
    from replicatinggpt_amd.engine import Evaluator
    torch.manual_seed(1337)
    m = BigramLanguageModel(gpt_config(dtype, PK.E_SHAPE)).to(DEV)
    s = PK.packed_train_sampler(DEV)
    m.eval()
    ev = Evaluator(m, s)
    seen = []
    for split in ("train", "val", "train"):
        got = ev.loss(split).clone()
        assert ev.graph is not None
        with torch.no_grad():
            _, want = m(ev.x, ev.y, ignore_index=s.ignore_index, seg_start=ev.seg)
        assert torch.isfinite(want) and torch.equal(got.view(torch.int32), want.view(torch.int32)), (float(got), float(want))
        seen.append(ev.seg.cpu().clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2])


def test_finetune_on_packed_rows_then_complete_returns_the_completions():
    """pairs.E2E_FOUR packed four or five to a row of 32 (tiny fp32 model, AdamW at lr 1e-2, graph replay):
    after packing.E2E_STEPS = 14 steps greedy complete() returns the four completions.  The oracle's own
    loop on the packed batches first reproduces them after 7 (test_cpu_packing.py holds both numbers)."""
    from replicatinggpt_amd import AdamW, BigramLanguageModel
    from replicatinggpt_amd.engine import TrainStep
    torch.manual_seed(PK.E2E_INIT_SEED)
    m = BigramLanguageModel(gpt_config("fp32", PK.E2E_SHAPE)).to(DEV)
    opt = AdamW(m.parameters(), lr=PK.E2E_LR)
    st = TrainStep(m, opt, PK.e2e_sampler(DEV))
    st.capture(restore=True)
    losses = [float(st.step().detach()) for _ in range(PK.E2E_STEPS)]
    print("packed fine-tune losses", " ".join(f"{l:.3f}" for l in losses))
    assert losses[-1] < losses[0]
    m.eval()
    new = max(len(c) for _, c in PR.E2E_FOUR)
    with torch.no_grad():
        out = m.complete([torch.tensor(p) for p, _ in PR.E2E_FOUR], new, greedy=True)
    tokens = out.tokens.cpu()
    for b, (p, c) in enumerate(PR.E2E_FOUR):
        assert tokens[b, len(p):len(p) + len(c)].tolist() == c, (b, tokens[b].tolist(), c)


@pytest.mark.parametrize("ignore", [None, -100])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_without_seg_start_nothing_moves(dtype, ignore):
    """model(idx, targets[, ignore_index]) gives, bit for bit, the loss and the gradients of the nodes
    called directly with the unsegmented ops -- EmbeddingFn, the blocks, HeadLossFn, as before packing."""
    from replicatinggpt_amd import AdamW, BigramLanguageModel
    from replicatinggpt_amd import functional as Fn
    from replicatinggpt_amd.model import _act_dtype
    runs = []
    for how in ("model", "plain"):
        torch.manual_seed(1337)
        m = BigramLanguageModel(gpt_config(dtype, PR.E_SHAPE)).to(DEV)
        opt = AdamW(m.parameters(), lr=1e-3)
        x, y = PR.train_sampler(DEV).get_batch("train")
        if ignore is None:
            y = y.clamp_min(0)
        if how == "model":
            _, loss = m(x, y) if ignore is None else m(x, y, ignore_index=ignore)
        else:
            if dtype == "bf16":
                m._sync_shadow()
            R = m._store.regions
            assert m._fwd_seg is None
            h = m.blocks(Fn.EmbeddingFn.apply(x, R["wte"], R["wpe"], *R["wte"].params, *R["wpe"].params))
            lw, lb, hw, hb = R["lnf_w"], R["lnf_b"], R["lm_w"], R["lm_b"]
            extra = () if ignore is None else (ignore,)
            _, loss = Fn.HeadLossFn.apply(h, y, _act_dtype(m.config), lw, lb, hw, hb, *lw.params, *lb.params, *hw.params,
                                          *hb.params, *extra)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().cpu().clone(), m.flat.grad.detach().cpu().clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][0]) and float(runs[0][1].abs().max()) > 0


def test_seg_start_operand_checks():
    from replicatinggpt_amd import BigramLanguageModel
    m = BigramLanguageModel(gpt_config("fp32", PR.E2E_SHAPE)).to(DEV)
    x = torch.zeros((2, 16), dtype=torch.int64, device=DEV)
    for bad in (torch.zeros((2, 16), dtype=torch.int64, device=DEV), torch.zeros((2, 8), dtype=torch.int32, device=DEV),
                torch.zeros((2, 16), dtype=torch.int32)):
        with pytest.raises(ValueError, match="seg_start must be an int32"):
            m(x, seg_start=bad)
