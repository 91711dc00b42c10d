"""Global-norm gradient clipping and the device-lr AdamW on the MI355X: cg_grad_norm against float64
numpy (every size class of its launch, aligned and not), cg_adamw_dyn bit for bit against the numpy
restatement of adam_one's roundings and against cg_scale_f32 + cg_adamw, and the pair against
torch's clip_grad_norm_ + torch.optim.AdamW on the CPU."""
import math

import numpy as np
import pytest
import torch

from numerics import fma32 as _fma32    # the exactly rounded float32 fma of the AdamW restatements

pytestmark = pytest.mark.gpu
DEV = "cuda"

# cg_grad_norm's launch (csrc/grad_norm.hip): at most 2048 blocks of 256 threads, 4 float4 groups per
# thread per iteration -- one sweep of the full grid covers 2048 * 256 * 4 * 4 floats
GRID_SWEEP = 2048 * 256 * 4 * 4
SIZES = [0, 1, 3, 255, 1000, 4099, 2 * GRID_SWEEP + 3]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from replicatinggpt_amd import _lib as L
    L.load()
    yield


def ops():
    from replicatinggpt_amd import ops as O
    return O


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _norm(g, max_norm, stream=None):
    """(norm, coef) of cg_grad_norm as numpy float32 scalars."""
    out = torch.full((2,), -7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops().grad_norm_workspace(g.numel()) // 8, dtype=torch.float64, device=DEV)
    if stream is None:
        ops().grad_norm(g, max_norm, out, ws)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ops().grad_norm(g, max_norm, out, ws)
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[0], o[1]


def _coef32(max_norm, norm):
    """torch's clip_grad_norm_ coefficient in fp32: min(1, max_norm / (norm + 1e-6))."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return c if c < 1 else np.float32(1.0)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_grad_norm_matches_float64(n, offset):
    """|norm - float32(sqrt(sum64))| <= 1 ulp, the coefficient bit-equal to the fp32 formula on the
    returned norm, for max_norm below (coef < 1) and above (coef == 1) the norm; the same bits from a
    second call on another stream.  offset 1: g starts 4 bytes past a 16-B boundary."""
    torch.manual_seed(n + offset)
    buf = torch.randn(n + offset, device=DEV)
    g = buf[offset:]
    assert n == 0 or g.data_ptr() % 16 == 4 * offset
    x = g.cpu().numpy().astype(np.float64)
    want = np.float32(math.sqrt(float(np.dot(x, x))))
    if n == 0:
        norm, coef = _norm(g, 1.0)
        assert norm == 0.0 and coef == 1.0
        return
    seen = set()
    for max_norm in (0.5 * float(want), 2.0 * float(want)):
        norm, coef = _norm(g, max_norm)
        assert abs(float(norm) - float(want)) <= float(np.spacing(want)), (norm, want)
        assert coef.view(np.uint32) == _coef32(max_norm, norm).view(np.uint32), (coef, _coef32(max_norm, norm))
        seen.add(bool(coef < 1))
        norm2, coef2 = _norm(g, max_norm, stream=torch.cuda.Stream())
        assert norm2.view(np.uint32) == norm.view(np.uint32) and coef2.view(np.uint32) == coef.view(np.uint32)
    assert seen == {True, False}


def test_grad_norm_inf_and_nan():
    g = torch.randn(4099, device=DEV)
    g[77] = float("inf")
    norm, coef = _norm(g, 1.0)
    assert np.isposinf(norm) and coef == 0.0
    g[77] = float("nan")
    norm, coef = _norm(g, 1.0)
    assert np.isnan(norm)




def test_adamw_dyn_bitwise():
    """cg_adamw_dyn with a clip coefficient: every gradient is (g * coef) rounded once to fp32, then
    adam_one unchanged -- bit-equal to the numpy restatement of test_adamw_rounding_is_explicit fed
    (G * coef).astype(float32), and to cg_scale_f32 on the gradient followed by cg_adamw.  Without a
    coefficient and with *lr_dev = lr: cg_adamw's bits.  n = 2^14 + 3: vector body and a 3-element tail."""
    f = np.float32
    n = (1 << 14) + 3
    rng = np.random.default_rng(3)
    P = rng.standard_normal(n).astype(f)
    M = (rng.standard_normal(n) * 0.01).astype(f)
    V = (rng.random(n) * 1e-3).astype(f)
    lr, b1, b2, eps, wd = 3e-3, 0.9, 0.999, 1e-8, 1e-2
    coef = f(0.37)

    def state():
        p, m, v = (torch.from_numpy(x.copy()).to(DEV) for x in (P, M, V))
        return p, m, v, torch.empty(n, dtype=torch.bfloat16, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)

    dyn, two, nul, ref = state(), state(), state(), state()   # dyn+coef | scale, adamw | dyn, no coef | adamw
    lr_dev = torch.tensor([lr], dtype=torch.float64, device=DEV)
    coef_dev = torch.tensor([coef], dtype=torch.float32, device=DEV)
    for t in range(1, 4):
        G = rng.standard_normal(n).astype(f)
        gd = torch.from_numpy(G).to(DEV)
        for p, m, v, sh, step in (dyn, two, nul, ref):
            ops().counter_add(step, 1)
        ops().adamw_dyn(dyn[0], gd, dyn[1], dyn[2], dyn[3], lr_dev, coef_dev, b1, b2, eps, wd, dyn[4])
        gs = gd.clone()
        ops().scale_(gs, coef_dev)
        ops().adamw(two[0], gs, two[1], two[2], two[3], lr, b1, b2, eps, wd, two[4])
        ops().adamw_dyn(nul[0], gd, nul[1], nul[2], nul[3], lr_dev, None, b1, b2, eps, wd, nul[4])
        ops().adamw(ref[0], gd, ref[1], ref[2], ref[3], lr, b1, b2, eps, wd, ref[4])
        assert torch.equal(gd.cpu(), torch.from_numpy(G))          # the gradient itself is not written
        G = (G * coef).astype(f)
        assert np.array_equal(gs.cpu().numpy(), G)
        decay, w1, B2, omb2, E = f(1 - lr * wd), f(1 - b1), f(b2), f(1 - b2), f(eps)
        neg, bc2s = f(-(lr / (1 - b1 ** t))), f(math.sqrt(1 - b2 ** t))
        P = (P * decay).astype(f)
        M = _fma32(w1, (G - M).astype(f), M)
        V = _fma32((omb2 * G).astype(f), G, (V * B2).astype(f))
        den = ((np.sqrt(V).astype(f) / bc2s).astype(f) + E).astype(f)
        P = (P + ((neg * M).astype(f) / den).astype(f)).astype(f)
    torch.cuda.synchronize()
    assert np.array_equal(dyn[1].cpu().numpy(), M) and np.array_equal(dyn[2].cpu().numpy(), V)
    assert np.array_equal(dyn[0].cpu().numpy(), P)
    for a, b in ((dyn, two), (nul, ref)):
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32),
                               y.view(torch.int16) if y.dtype == torch.bfloat16 else y.view(torch.int32))


def test_clip_and_adamw_match_torch():
    """cg_grad_norm + cg_adamw_dyn against clip_grad_norm_ + torch.optim.AdamW on the CPU, 5 steps,
    n = 1000, to test_adamw_matches_torch's bar; the gradient scale alternates so that the clip is
    active on some steps and inactive on others."""
    n = 1000
    torch.manual_seed(8)
    p = torch.randn(n)
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=2e-4)
    pd = p.clone().to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    sh = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    lr_dev = torch.tensor([2e-4], dtype=torch.float64, device=DEV)
    out = torch.empty(2, dtype=torch.float32, device=DEV)
    ws = torch.empty(ops().grad_norm_workspace(n) // 8, dtype=torch.float64, device=DEV)
    active = []
    for i in range(5):
        g = torch.randn(n) * (1.0 if i % 2 == 0 else 0.01)    # norms ~ 31.6 and ~ 0.32 around max_norm 1
        ref.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([ref], 1.0)
        opt.step()
        gd = g.to(DEV)
        ops().grad_norm(gd, 1.0, out, ws)
        ops().counter_add(step, 1)
        ops().adamw_dyn(pd, gd, m, v, sh, lr_dev, out[1:2], 0.9, 0.999, 1e-8, 1e-2, step)
        norm, coef = out.cpu().tolist()
        assert abs(norm - float(total)) <= 1e-6 * float(total)
        active.append(coef < 1.0)
        assert active[-1] == (float(total) > 1.0)
    assert any(active) and not all(active)
    assert relerr(pd, ref.detach()) < 1e-6
    assert torch.equal(sh.cpu(), pd.cpu().to(torch.bfloat16))
