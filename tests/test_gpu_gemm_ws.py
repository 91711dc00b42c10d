"""The weight-stationary bf16 GEMM (csrc/gemm_ws.hip, gemm_variant 31) against the 128x128 persistent
kernel (gemm_variant 9), bit for bit: same MFMA instruction, operand roles and k order, so every
output element, keep-bit word and column partial must be identical.

k_gemm_ws works on 64-row tiles and variant 9 on 128-row ones, so the oracle runs on the rows padded
to a multiple of 128 (a row of the output depends on its own row of A only, a column partial on its
own 64 rows) and the first M rows are compared.  Shapes: one tile with almost every block idle
(M = 64), M = 192, one block of a panel with two tiles and the rest one (M = 64 (blocks per panel)
+ 64), M = 4096, and nine or ten tiles per block (M = 16384 at N = 1152; a grid capped at one block per
panel) for the ring's steady state; one, three and nine 128-column panels; K = 64, 192, 384; row strides
padded beyond the logical width.  cg_gemm_ws_launches() says that the kernel under test served the call."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
STORE_NT, STORE_BT, BIAS_RELU_BITS, RELU_BWD_COLPART = "store_nt", "store_bt", "bias_relu_bits", "relu_bwd_colpart"
KINDS = [STORE_NT, STORE_BT, BIAS_RELU_BITS, RELU_BWD_COLPART]
# the other instantiations cg_gemm reaches: bias + ReLU + keep bits on a transposed B, bias + ReLU without
# keep bits, ReLU-backward on a K-contiguous B and without column partials
BIAS_RELU_BITS_BT, BIAS_RELU_PLAIN, RELU_BWD_NT = "bias_relu_bits_bt", "bias_relu_plain", "relu_bwd_nt"
OTHER_KINDS = [BIAS_RELU_BITS_BT, BIAS_RELU_PLAIN, RELU_BWD_NT]
# (M, N, K, padded strides); M = "bpp+1": 64 * (blocks per panel) + 64
SHAPES = [(64, 128, 64, 1), (192, 128, 192, 0), (64, 384, 384, 1), (192, 384, 64, 1), ("bpp+1", 128, 384, 0),
          ("bpp+1", 384, 192, 1), ("bpp+1", 1152, 384, 1), (4096, 128, 192, 1), (4096, 384, 384, 0),
          (4096, 1152, 384, 1), (4096, 1152, 64, 0), (4096, 1152, 384, 0),
          # 9 or 10 tiles per block: the ring's steady state (stage reuse, the wrap of the stage index)
          (16384, 1152, 384, 1)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from replicatinggpt_amd import _lib
    _lib.load()
    yield
    tuning("gemm_variant", 0)
    tuning("gemm_ws", 1)


def lib():
    from replicatinggpt_amd import _lib
    return _lib.load()


def ops():
    from replicatinggpt_amd import ops as O
    return O


def tuning(key, value):
    from replicatinggpt_amd import _lib
    _lib.check(lib().cg_set_tuning(key.encode(), value), f"cg_set_tuning({key})")


def launches():
    return int(lib().cg_gemm_ws_launches())


def blocks_per_panel(N):
    return torch.cuda.get_device_properties(0).multi_processor_count // (N // 128)


def rows_of(M, N):
    return 64 * blocks_per_panel(N) + 64 if M == "bpp+1" else M


def strided(rows, cols, ld, dtype, gen=None, scale=1.0):
    """A [rows, ld] buffer whose first `cols` columns are the operand: the rest is NaN padding (int: -1)."""
    if dtype == I32:
        buf = torch.full((rows, ld), -1, dtype=I32)
    else:
        buf = torch.full((rows, ld), float("nan"), dtype=dtype)
        buf[:, :cols] = (torch.randn(rows, cols, generator=gen) * scale).to(dtype)
    return buf.to(DEV)


class Case:
    """One product's operands (rows padded to a multiple of 128 for the oracle) and its two runs."""

    def __init__(self, kind, M, N, K, pad, seed=0):
        g = torch.Generator().manual_seed(1000 + seed)
        self.kind, self.M, self.N, self.K = kind, M, N, K
        self.Mp = (M + 127) // 128 * 128
        self.bt = kind in (STORE_BT, RELU_BWD_COLPART, BIAS_RELU_BITS_BT)
        self.lda, self.ldc = K + 8 * pad, N + 8 * pad
        self.ldb = (N if self.bt else K) + 16 * pad
        self.ldw = N // 32 + 4 * pad
        self.A = strided(self.Mp, K, self.lda, BF16, g, 0.5)
        self.B = strided(K if self.bt else N, N if self.bt else K, self.ldb, BF16, g, 0.05)
        self.bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
        keep = torch.rand(self.Mp, N, generator=g) < 0.5
        words = (keep.view(self.Mp, N // 32, 32).long() << torch.arange(32)).sum(-1)
        self.keep = keep.to(DEV)
        self.bits_in = torch.full((self.Mp, self.ldw), -1, dtype=I32)
        self.bits_in[:, :N // 32] = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(I32)
        self.bits_in = self.bits_in.to(DEV)

    def run(self, variant, rows):
        """(C, bits, colpart) of the first `rows` rows under gemm_variant `variant`; untouched bytes stay NaN / -1."""
        O, N, K = ops(), self.N, self.K
        C = torch.full((rows, self.ldc), float("nan"), dtype=BF16, device=DEV)
        bits = torch.full((rows, self.ldw), -1, dtype=I32, device=DEV)
        part = torch.full((rows // 64, N), float("nan"), dtype=F32, device=DEV)
        tuning("gemm_variant", variant)
        try:
            if self.kind in (STORE_NT, STORE_BT):
                O.gemm(self.A, self.B, C, True, False, self.bt, rows, N, K, self.lda, self.ldb, self.ldc, 0, None, None,
                       0, None, 0, 0.0, 0, None, 0, 0.0, 1, None)
            elif self.kind in (BIAS_RELU_BITS_BT, BIAS_RELU_PLAIN):
                aux = bits if self.kind == BIAS_RELU_BITS_BT else None
                O.gemm(self.A, self.B, C, True, False, self.bt, rows, N, K, self.lda, self.ldb, self.ldc, 2, self.bias,
                       None, 0, aux, self.ldw if aux is not None else 0, 0.0, 0, None, 0, 0.0, 1, None)
            elif self.kind == RELU_BWD_NT:
                O.gemm(self.A, self.B, C, True, False, False, rows, N, K, self.lda, self.ldb, self.ldc, 5, None, None, 0,
                       self.bits_in, self.ldw, 0.0, 0, None, 0, 0.0, 1, None)
            elif self.kind == BIAS_RELU_BITS:
                O.gemm_bias_relu_bits(self.A, self.B, C, rows, N, K, self.lda, self.ldb, self.ldc, self.bias, bits,
                                      self.ldw)
            else:
                O.gemm_relu_bwd_colpart(self.A, self.B, C, rows, N, K, self.lda, self.ldb, self.ldc, self.bits_in,
                                        self.ldw, part)
            torch.cuda.synchronize()
        finally:
            tuning("gemm_variant", 0)
        return C, bits, part

    def exact(self):
        """The product's epilogue in fp64 from the bf16 operands, [M, N]."""
        a = self.A[:self.M, :self.K].double()
        b = self.B[:self.K, :self.N].double() if self.bt else self.B[:self.N, :self.K].double().t()
        acc = a @ b
        if self.kind in (BIAS_RELU_BITS, BIAS_RELU_BITS_BT, BIAS_RELU_PLAIN):
            return torch.relu(acc + self.bias.double())
        if self.kind in (RELU_BWD_COLPART, RELU_BWD_NT):
            return acc * self.keep[:self.M].double()
        return acc


def bits_equal(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == BF16 else a.view(I32), b.view(torch.int16) if b.dtype == BF16 else b.view(I32))


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def compare_with_variant_9(kind, M, N, K, pad, max_grid=0):
    c = Case(kind, M, N, K, pad)
    n0 = launches()
    tuning("gemm_max_grid", max_grid)
    try:
        C, bits, part = c.run(31, M)
    finally:
        tuning("gemm_max_grid", 0)
    assert launches() == n0 + 1, "k_gemm_ws did not take the call"
    Cr, bits_r, part_r = c.run(9, c.Mp)
    assert launches() == n0 + 1
    # every element of the padded buffers: the outputs equal the oracle's, the padding is untouched
    assert bits_equal(C, Cr[:M]), "output bits differ from gemm_variant 9"
    assert not torch.isnan(C[:, :N].float()).any()
    if kind in (BIAS_RELU_BITS, BIAS_RELU_BITS_BT):
        assert torch.equal(bits, bits_r[:M]), "keep-bit words differ"
        nz = (C[:, :N].contiguous().view(torch.int16) & 0x7FFF) != 0
        want = (nz.view(M, N // 32, 32).long() << torch.arange(32, device=DEV)).sum(-1)
        assert torch.equal(bits[:, :N // 32].long() & 0xFFFFFFFF, want)
    else:
        assert torch.equal(bits, torch.full_like(bits, -1))
    if kind == RELU_BWD_COLPART:
        assert bits_equal(part, part_r[:M // 64]), "column partials differ"
    else:
        assert torch.isnan(part).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N,K,pad", SHAPES)
def test_bitwise_against_the_128x128_kernel(kind, M, N, K, pad):
    compare_with_variant_9(kind, rows_of(M, N), N, K, pad)


@pytest.mark.parametrize("kind", OTHER_KINDS)
@pytest.mark.parametrize("M,N,K,pad", [(192, 384, 192, 1), ("bpp+1", 1152, 384, 1), (4096, 1152, 384, 0)])
def test_other_instantiations_bitwise(kind, M, N, K, pad):
    compare_with_variant_9(kind, rows_of(M, N), N, K, pad)


@pytest.mark.parametrize("kind", KINDS + OTHER_KINDS)
def test_many_tiles_per_block_bitwise(kind):
    """Three blocks for three panels (gemm_max_grid 3): each walks all ten 64-row tiles, so tile t + 2 lands in
    tile t - 1's stage, the stage index wraps three times and every loop-head wait count is taken."""
    compare_with_variant_9(kind, 640, 384, 384, 1, max_grid=3)


@pytest.mark.parametrize("kind", KINDS + OTHER_KINDS)
def test_against_fp64(kind):
    """The bound tests/test_gpu_ops.py holds these epilogue kinds to (bf16: 8e-3 of the largest element),
    and the folded partials against the column sums of the stored output (1e-5, test_relu_bwd_colpart_matches_colsum)."""
    M, N, K = 4096, 1152, 384
    c = Case(kind, M, N, K, 1, seed=7)
    n0 = launches()
    C, _, part = c.run(31, M)
    assert launches() == n0 + 1
    err = relerr(C[:, :N], c.exact())
    print(f"{kind}: max error / max |reference| = {err:.3e}")
    assert err < 8e-3
    if kind == RELU_BWD_COLPART:
        cs = part.double().sum(0)
        e2 = relerr(cs, C[:, :N].double().sum(0))
        print(f"{kind}: folded partials against the stored output's column sums: {e2:.3e}")
        assert e2 < 1e-5


def test_automatic_routing():
    """The default dispatch hands only the wide-N, large-M, K <= 384 products to k_gemm_ws, the gemm_ws knob
    turns that off, and the result does not depend on it."""
    def run(M, N, K):
        c = Case(BIAS_RELU_BITS, M, N, K, 0, seed=3)
        n0 = launches()
        out = c.run(0, M)
        return launches() - n0, out
    took, on = run(4096, 1152, 384)
    assert took == 1
    tuning("gemm_ws", 0)
    try:
        took, off = run(4096, 1152, 384)
    finally:
        tuning("gemm_ws", 1)
    assert took == 0
    assert bits_equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert run(4096, 384, 384)[0] == 0      # N < 1152
    assert run(2048, 1152, 384)[0] == 0     # M < 4096
    assert run(4096, 1152, 512)[0] == 0     # K > 384


def test_deferred_reduce_survives_a_ws_launch():
    """A split-K reduce deferred on the stream stays queued across a k_gemm_ws launch (which hosts no deferred
    work and does not flush it: the output is untouched after it) and is summed by the next k_gemm_pk launch:
    the weight gradient equals the in-line reduce's."""
    from replicatinggpt_amd import _lib as L
    O = ops()
    g = torch.Generator().manual_seed(5)
    Mk, N1, K1, split = 1024, 128, 128, 4
    dy = torch.randn(Mk, N1, generator=g).to(BF16).to(DEV)
    x = torch.randn(Mk, K1, generator=g).to(BF16).to(DEV)
    ws = torch.empty(split * N1 * K1, dtype=F32, device=DEV)

    def wgrad(flags):
        out = torch.full((N1, K1), float("nan"), dtype=F32, device=DEV)
        O.gemm(dy, x, out, True, True, True, N1, K1, Mk, N1, K1, K1, 0, None, None, 0, None, 0, 0.0, 0, None, 0, 0.0,
               split, ws, flags)
        return out
    ref = wgrad(0)
    torch.cuda.synchronize()
    got = wgrad(L.GEMM_DEFER_REDUCE)
    c = Case(STORE_NT, 256, 128, 128, 0, seed=9)
    n0 = launches()
    c.run(31, 256)      # (synchronises)
    assert launches() == n0 + 1
    # neither summed in the ws launch's tail nor flushed by it: the output still holds its NaN prefill
    assert torch.isnan(got).all(), "the k_gemm_ws launch ran or flushed the deferred reduce"
    c.run(9, 256)       # the persistent 128x128 kernel: takes the pending reduce
    assert torch.equal(got, ref), "the next k_gemm_pk launch did not sum the deferred reduce"
    L.check(lib().cg_flush_deferred(L.stream_ptr()), "flush")   # nothing may be left either way
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


def test_c2_step_identical_with_and_without():
    """One training step of a C2-shaped model (6 layers, 6 heads, 384 wide, block 256) at batch 16 -- 4096 rows,
    the smallest batch the automatic routing takes -- with gemm_ws on and off: loss, gradients and
    parameters are the same bits, and the on-run did go through k_gemm_ws (QKV, FFN1, FFN2 dgrad per layer)."""
    from replicatinggpt_amd import AdamW, BigramLanguageModel, GPTConfig
    from replicatinggpt_amd.data import BatchSampler, TokenStream
    from replicatinggpt_amd.engine import TrainStep
    cfg = GPTConfig(block_size=256, n_embd=384, n_head=6, n_layers=6, dropout=0.2, dtype="bf16", batch_size=16)
    runs = []
    try:
        for on in (1, 0):
            tuning("gemm_ws", on)
            torch.manual_seed(1337)
            m = BigramLanguageModel(cfg).to(DEV)
            opt = AdamW(m.parameters(), lr=1e-3)
            s = BatchSampler(TokenStream.synthetic(device=DEV), cfg.block_size, cfg.batch_size)
            st = TrainStep(m, opt, s, use_graph=False)
            n0 = launches()
            loss = float(st.step().detach())
            torch.cuda.synchronize()
            runs.append((loss, m.flat.grad.detach().clone(), m.flat.master.detach().clone(), launches() - n0))
    finally:
        tuning("gemm_ws", 1)
    assert runs[0][3] >= 3 * cfg.n_layers and runs[1][3] == 0
    assert runs[0][0] == runs[1][0]
    assert bits_equal(runs[0][1], runs[1][1]) and bits_equal(runs[0][2], runs[1][2])
