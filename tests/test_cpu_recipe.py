"""Host-side checks of the training recipe (no GPU): the warm-up / cosine schedule against its
closed form, the constructor validation of optim.AdamW's dynamic mode and engine.TrainStep's
lr_schedule, the unchanged torch state-dict layout, and the new C-ABI symbols."""
import math
import types

import pytest
import torch


def _model():
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    torch.manual_seed(0)
    return BigramLanguageModel(GPTConfig(block_size=16, n_embd=24, n_head=4, n_layers=2))


def test_warmup_cosine_closed_form():
    from replicatinggpt_amd.schedule import warmup_cosine
    base, warm, decay, floor = 6e-4, 10, 110, 6e-5
    assert warmup_cosine(0, base, warm, decay, floor) == base / warm           # starts at base / warmup_iters
    assert warmup_cosine(4, base, warm, decay, floor) == base * 5 / warm       # linear
    assert warmup_cosine(warm - 1, base, warm, decay, floor) == base
    assert warmup_cosine(warm, base, warm, decay, floor) == base               # the cosine starts at base_lr
    mid = warmup_cosine((warm + decay) // 2, base, warm, decay, floor)
    assert abs(mid - 0.5 * (base + floor)) <= 1e-15                            # cos(pi / 2) = 0: the midpoint
    q = warmup_cosine(warm + 25, base, warm, decay, floor)                     # a quarter of the way
    assert abs(q - (floor + (base - floor) * 0.5 * (1 + math.cos(math.pi / 4)))) <= 1e-15
    assert warmup_cosine(decay, base, warm, decay, floor) == floor
    assert warmup_cosine(decay + 1000, base, warm, decay, floor) == floor
    lrs = [warmup_cosine(i, base, warm, decay, floor) for i in range(warm, decay + 1)]
    assert all(a > b for a, b in zip(lrs, lrs[1:]))                            # strictly decreasing decay
    assert warmup_cosine(0, base, 0, 100, floor) == base                       # no warm-up
    with pytest.raises(ValueError):
        warmup_cosine(0, base, 10, 5, floor)


def test_constructor_validation():
    from replicatinggpt_amd import AdamW
    m = _model()
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            AdamW(m.parameters(), lr=1e-3, max_grad_norm=bad)
    assert not AdamW(m.parameters(), lr=1e-3).dynamic_lr
    assert AdamW(m.parameters(), lr=1e-3, dynamic_lr=True).dynamic_lr
    clip = AdamW(m.parameters(), lr=1e-3, max_grad_norm=1.0)
    assert clip.dynamic_lr and clip.max_grad_norm == 1.0                       # clipping implies the device lr
    with pytest.raises(RuntimeError, match="dynamic_lr"):
        AdamW(m.parameters(), lr=1e-3).set_lr(1e-4)


def test_dynamic_optimizer_never_takes_early_updates():
    from replicatinggpt_amd import AdamW
    m = _model()
    assert not AdamW(m.parameters(), lr=1e-3, dynamic_lr=True).early_ok()
    assert not AdamW(m.parameters(), lr=1e-3, max_grad_norm=1.0).early_ok()


def test_set_lr_writes_group_and_device_scalar():
    from replicatinggpt_amd import AdamW
    opt = AdamW(_model().parameters(), lr=1e-3, dynamic_lr=True)
    opt.set_lr(2.5e-4)
    assert opt.param_groups[0]["lr"] == 2.5e-4
    assert opt._lr_t.dtype == torch.float64 and float(opt._lr_t) == 2.5e-4
    assert opt.grad_norm is None and opt.clip_coef is None                     # no clipping asked for


def test_trainstep_lr_schedule_needs_dynamic_optimizer():
    from replicatinggpt_amd import AdamW
    from replicatinggpt_amd.engine import TrainStep
    m = _model()
    sampler = types.SimpleNamespace(B=2, T=16, generator=None)
    with pytest.raises(ValueError, match="lr_schedule"):
        TrainStep(m, AdamW(m.parameters(), lr=1e-3), sampler, use_graph=False, lr_schedule=lambda it: 1e-3)
    step = TrainStep(m, AdamW(m.parameters(), lr=1e-3, dynamic_lr=True), sampler, use_graph=False,
                     lr_schedule=lambda it: 1e-3)
    assert step.it == 0
    step.it = 7                                                                # settable, for resume
    assert step.it == 7
    assert TrainStep(m, AdamW(m.parameters(), lr=1e-3), sampler, use_graph=False).lr_schedule is None


def test_dynamic_state_dict_is_torch_format():
    """max_grad_norm / dynamic_lr are constructor settings, not checkpoint state: the state dict of
    a dynamic optimizer has torch's keys only and loads into torch.optim.AdamW (and back)."""
    from replicatinggpt_amd import AdamW
    m = _model()
    ref = torch.optim.AdamW(m.parameters(), lr=3e-3)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    plain = AdamW(m.parameters(), lr=5e-1)
    ours = AdamW(m.parameters(), lr=5e-1, max_grad_norm=1.0)
    plain.load_state_dict(ref.state_dict())
    ours.load_state_dict(ref.state_dict())
    assert ours.param_groups[0]["lr"] == 3e-3 and float(ours._lr_t) == 3e-3   # the device lr follows the load
    sd, psd = ours.state_dict(), plain.state_dict()
    assert set(sd) == {"state", "param_groups"}
    assert sd["param_groups"] == psd["param_groups"]
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    back = torch.optim.AdamW(m.parameters(), lr=1.0)
    back.load_state_dict(sd)
    for p in m.parameters():
        assert torch.equal(back.state[p]["exp_avg"], ref.state[p]["exp_avg"])
        assert torch.equal(back.state[p]["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
    assert back.param_groups[0]["lr"] == 3e-3


def test_library_has_the_recipe_symbols():
    from replicatinggpt_amd import _lib, ops  # noqa: F401
    lib = _lib.load()
    for s in ("cg_grad_norm_workspace", "cg_grad_norm", "cg_scale_f32", "cg_adamw_dyn"):
        assert hasattr(lib, s), s
        assert s in _lib._SIGS and s in _lib.header_symbols(), s
    for name in ("grad_norm", "scale_", "adamw_dyn"):
        assert hasattr(torch.ops.charpt, name), name
    # one double per block, a grid that depends only on n: 1 block up to 4096 floats, at most 2048
    assert lib.cg_grad_norm_workspace(0) == 8 and lib.cg_grad_norm_workspace(4096) == 8
    assert lib.cg_grad_norm_workspace(4100) == 16
    assert lib.cg_grad_norm_workspace(1 << 30) == 2048 * 8


def test_driver_flags_default_to_todays_objects():
    from replicatinggpt_amd.gpt1 import parse_args
    a = parse_args([])
    assert a.grad_clip is None and a.warmup_iters is None and a.lr_decay_iters is None and a.min_lr is None
    b = parse_args(["--grad-clip", "1.0", "--warmup-iters", "100", "--lr-decay-iters", "5000", "--min-lr", "6e-5"])
    assert (b.grad_clip, b.warmup_iters, b.lr_decay_iters, b.min_lr) == (1.0, 100, 5000, 6e-5)
