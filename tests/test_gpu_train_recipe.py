"""The training recipe end to end on the MI355X: optim.AdamW's dynamic mode (device learning rate,
global-norm clipping) through engine.TrainStep -- eager, hipGraph replay and two data-parallel ranks --
on the small config of tests/test_gpu_dp.py (T 64, d 64, 2 heads, 3 layers, fp32, dropout 0), 4 steps."""
import functools
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
STEPS, B_RANK, WORLD = 4, 4, 2
LR = 1e-3
CLIP = 0.05   # far below this model's gradient norm at initialisation: every step clips (asserted)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    yield


def _schedule(it):
    """A learning rate that differs on each of the 4 steps: warm-up, peak, two points of the decay."""
    from replicatinggpt_amd.schedule import warmup_cosine
    return warmup_cosine(2 * it, LR, 3, 9, 1e-4)


def _build(batch=B_RANK, world=1, rank=0, **opt_kw):
    from replicatinggpt_amd import AdamW, BigramLanguageModel, GPTConfig
    from replicatinggpt_amd.data import BatchSampler, TokenStream
    cfg = GPTConfig(block_size=64, n_embd=64, n_head=2, n_layers=3, dropout=0.0, dtype="fp32", batch_size=batch)
    torch.manual_seed(1337)
    model = BigramLanguageModel(cfg).to("cuda")
    opt = AdamW(model.parameters(), lr=LR, **opt_kw).attach(model)
    sampler = BatchSampler(TokenStream.synthetic(n_tokens=1 << 16, device="cuda"), cfg.block_size, batch,
                           world_size=world, rank=rank, generator=torch.Generator().manual_seed(5))
    return model, opt, sampler


def _grad_norm64(model):
    return math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in model.parameters()))


def _state(model, opt):
    torch.cuda.synchronize()
    return {"master": model.flat.master.detach().cpu().clone(), "m": opt._m.cpu().clone(), "v": opt._v.cpu().clone(),
            "step": int(opt._step_t)}


def _run(graph=True, schedule=None, **opt_kw):
    """4 TrainStep steps from the seeded initial state; the optimizer state afterwards, the learning
    rates used and, with clipping, per step (opt.grad_norm, opt.clip_coef, float64 norm of the .grads)."""
    from replicatinggpt_amd.engine import TrainStep
    model, opt, sampler = _build(**opt_kw)
    step = TrainStep(model, opt, sampler, use_graph=graph, lr_schedule=schedule)
    step.capture(restore=True)
    assert (step.g_fb is not None) == graph
    rec, lrs = [], []
    for _ in range(STEPS):
        step.step()
        lrs.append(opt.param_groups[0]["lr"])
        if opt.max_grad_norm is not None:
            rec.append((float(opt.grad_norm), float(opt.clip_coef), _grad_norm64(model)))
    out = _state(model, opt)
    out.update(rec=rec, lrs=lrs, it=step.it)
    return out


@functools.lru_cache(maxsize=None)
def _default_run():
    return _run()


def _same_state(a, b):
    return (torch.equal(a["master"], b["master"]) and torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"])
            and a["step"] == b["step"] == STEPS)


def test_dynamic_lr_at_constant_lr_is_the_default_optimizer():
    """The device learning rate is a double: at a constant value the dynamic path (no early updates,
    cg_adamw_dyn) gives the default path's masters, moments and step count bit for bit."""
    assert _same_state(_run(dynamic_lr=True), _default_run())


def test_inactive_clip_is_the_default_optimizer():
    got = _run(max_grad_norm=1e30)
    assert all(c == 1.0 for _, c, _ in got["rec"])
    assert _same_state(got, _default_run())


def test_graph_replay_follows_the_schedule():
    """A replayed step reads the learning rate set_lr wrote before the replay: masters bit-identical
    to the eager steps under the same schedule, and not those of the constant learning rate."""
    g = _run(graph=True, schedule=_schedule, dynamic_lr=True)
    e = _run(graph=False, schedule=_schedule, dynamic_lr=True)
    assert g["lrs"] == e["lrs"] == [_schedule(i) for i in range(STEPS)] and len(set(g["lrs"])) == STEPS
    assert g["it"] == e["it"] == STEPS
    assert _same_state(g, e)
    assert not torch.equal(g["master"], _default_run()["master"])


def test_clipping_graph_equals_eager_and_norm_is_the_parameters():
    """Clip active on every step: graph replay equals eager bit for bit (clip and schedule together),
    and opt.grad_norm -- taken over the whole flat buffer, padding included -- is the float64 norm
    of the per-parameter .grads to fp32 rounding (2^-22), so the padding contributes nothing."""
    g = _run(graph=True, schedule=_schedule, max_grad_norm=CLIP)
    e = _run(graph=False, schedule=_schedule, max_grad_norm=CLIP)
    assert _same_state(g, e)
    assert g["rec"] == e["rec"]
    for norm, coef, norm64 in g["rec"]:
        assert coef < 1.0, (norm, coef)
        assert abs(norm - norm64) <= 2.0 ** -22 * norm64, (norm, norm64)
        assert abs(coef - CLIP / (norm + 1e-6)) <= 1e-6 * coef


def _hand_loop(clip_in_optimizer):
    """GPT1.py's loop written by hand (no TrainStep): forward, zero_grad, backward, [clip], step."""
    from replicatinggpt_amd import clip_grad_norm_
    model, opt, sampler = _build(**({"max_grad_norm": CLIP} if clip_in_optimizer else {}))
    norms = []
    for _ in range(STEPS):
        x, y = sampler.get_batch("train")
        _, loss = model(x, y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if clip_in_optimizer:
            opt.step()
            norms.append(float(opt.grad_norm))
        else:
            norms.append(float(clip_grad_norm_(model, CLIP)))
            # the flat gradient -- every p.grad -- is scaled in place, as torch scales it: the norm is
            # now CLIP * norm / (norm + 1e-6), to a few fp32 roundings (2^-21)
            assert abs(_grad_norm64(model) - CLIP) <= (1e-6 / norms[-1] + 2.0 ** -21) * CLIP
            opt.step()
    return _state(model, opt), norms


def test_clip_grad_norm_then_default_step_equals_clipping_optimizer():
    (a, na), (b, nb) = _hand_loop(False), _hand_loop(True)
    assert na == nb and all(n > CLIP for n in na)
    assert _same_state(a, b)


def test_missing_grad_with_clipping_raises():
    from replicatinggpt_amd import clip_grad_norm_
    model, opt, sampler = _build(max_grad_norm=CLIP)
    x, y = sampler.get_batch("train")
    _, loss = model(x, y)
    loss.backward()
    model.lm_head.bias.grad = None
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        opt.step()
    with pytest.raises(RuntimeError, match="missing from its slot"):
        clip_grad_norm_(model, CLIP)
    # the per-parameter path still works with a device learning rate and no clipping
    model2, opt2, _ = _build(dynamic_lr=True)
    _, loss = model2(x, y)
    loss.backward()
    model2.lm_head.bias.grad = None
    before = model2.lm_head.bias.detach().clone()
    w_before = model2.lm_head.weight.detach().clone()
    opt2.step()
    torch.cuda.synchronize()
    assert torch.equal(model2.lm_head.bias.detach(), before)            # skipped, as torch skips it
    assert not torch.equal(model2.lm_head.weight.detach(), w_before)


def test_capture_restore_keeps_lr_and_iteration():
    from replicatinggpt_amd.engine import TrainStep
    model, opt, sampler = _build(max_grad_norm=CLIP)
    step = TrainStep(model, opt, sampler, use_graph=True, lr_schedule=_schedule)
    step.it = 5
    opt.set_lr(1.25e-4)
    before = _state(model, opt)
    step.capture(restore=True)
    after = _state(model, opt)
    assert step.it == 5 and opt.param_groups[0]["lr"] == 1.25e-4 and float(opt._lr_t) == 1.25e-4
    assert torch.equal(before["master"], after["master"]) and before["step"] == after["step"] == 0
    step.step()
    assert step.it == 6 and opt.param_groups[0]["lr"] == _schedule(5) == float(opt._lr_t)


# -- two data-parallel ranks on one GPU (the pattern of tests/test_gpu_dp.py) ------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _train_dp(world, rank, batch):
    from replicatinggpt_amd.engine import GradReducer, TrainStep
    model, opt, sampler = _build(batch, world, rank, max_grad_norm=CLIP)
    reducer = GradReducer(model.flat.grad, bucket_bytes=64 << 10) if world > 1 else None
    step = TrainStep(model, opt, sampler, reducer, use_graph=True, seg_layers=1, lr_schedule=_schedule)
    step.capture(restore=True)
    norms, coefs = [], []
    for _ in range(STEPS):
        step.step()
        norms.append(float(opt.grad_norm))
        coefs.append(float(opt.clip_coef))
    torch.cuda.synchronize()
    return model.flat.master.detach().cpu().clone(), norms, coefs, len(step.g_seg)


def _worker(rank, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        torch.cuda.set_device(0)
        master, norms, coefs, nseg = _train_dp(WORLD, rank, B_RANK)
        q.put((rank, master.numpy(), norms, coefs, nseg))   # by value: the worker exits right after
    finally:
        dist.destroy_process_group()


def test_dp_two_ranks_clip_the_averaged_gradient():
    """The optimizer graph replays after the all-reduce, so both ranks take the norm of the same
    averaged gradient: equal norms, bitwise-equal masters, and the W = 1 step on the concatenated
    batch to the tolerance tests/test_gpu_dp.py holds that comparison to."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(WORLD):
            r, master, norms, coefs, nseg = q.get(timeout=300)
            res[r] = (torch.from_numpy(master), norms, coefs, nseg)
    finally:
        for p in procs:
            p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs)
    want_master, want_norms, want_coefs, nseg1 = _train_dp(1, 0, WORLD * B_RANK)
    assert nseg1 == 0 and res[0][3] == res[1][3] == 3
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert all(c < 1.0 for c in res[0][2] + want_coefs)
    scale = float(want_master.abs().max())
    assert float((res[0][0] - want_master).abs().max()) / scale < 1e-5
