"""The block shape of the weight-stationary bf16 GEMM (csrc/gemm_ws.hip): two independent 4-wave blocks per CU
on 32-row half tiles.  Every case is bitwise against the 128x128 persistent kernel (gemm_variant 9) through
tests/test_gpu_gemm_ws.py's compare_with_variant_9 -- outputs, keep-bit words and column partials, on padded
strides with NaN / -1 prefill.  (The earlier form, one 8-wave block per CU, passed the same cases while it was
measured against this one, profiles/gemm_ws_blocks_ab.txt; it and its knob are gone.)

What the shapes pin, in 32-row half tiles (P = 2 x CUs blocks, bpp = P / panels per
panel; the plain-store and bias + ReLU kinds are dealt 32-row units, the ReLU-backward kinds 64-row units):
  * M = 64: one 64-row tile is two half tiles of one block, every other block idle, one K-tile;
  * gemm_max_grid 1 at M = 128 / 192 / 320: one block walks 4 / 6 / 10 half tiles -- the first stage reuse,
    every loop-head wait count, three wraps of the stage index, an odd 64-row tile count;
  * every instantiation at M = 320, N = 384, K = 384 with 3 and 6 blocks (one and two per panel);
  * K = 64 / 256 / 384 on a transposed B: one pass, 3 + 1 and 3 + 3 K-tiles of the panel staging;
  * ReLU-backward at M = 64 bpp + 64: one block gets an extra 64-row unit; at M = 192 with one block per
    panel: an odd number of 64-row tiles in one block;
  * a leftover 32-row unit for the plain-store and bias + ReLU kinds: M = 32 bpp + 32.  M is a multiple of
    64 (the kernel's contract), so bpp has to be odd: N = 896 (7 panels, bpp = 73 on 256 CUs) when the
    device gives an odd bpp for some panel count up to 12, and always N = 384 under gemm_max_grid 9
    (bpp = 3, M = 128: one block two half tiles, two blocks one each);
  * M = 64 x 2 x CUs at N = 128: every slot of every CU holds a block;
  * the runtime's occupancy query says two blocks per CU for every instantiation the dispatch can reach."""
import pytest
import torch

from test_gpu_gemm_ws import (BIAS_RELU_BITS, BIAS_RELU_BITS_BT, KINDS, OTHER_KINDS, RELU_BWD_COLPART, RELU_BWD_NT,
                              STORE_BT, STORE_NT, compare_with_variant_9, lib, tuning)

pytestmark = pytest.mark.gpu
BT_KINDS = [STORE_BT, RELU_BWD_COLPART, BIAS_RELU_BITS_BT]
EPI_STORE, EPI_BIAS_RELU, EPI_RELU_BWD = 0, 2, 5   # include/charpt.h cg_epilogue kinds


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from replicatinggpt_amd import _lib
    _lib.load()
    yield
    tuning("gemm_variant", 0)
    tuning("gemm_max_grid", 0)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def bpp(N):
    """blocks per panel"""
    return 2 * cus() // (N // 128)


@pytest.mark.parametrize("kind", KINDS)
def test_one_tile_two_half_tiles(kind):
    compare_with_variant_9(kind, 64, 128, 64, 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [128, 192, 320])
def test_one_block_walks_the_ring(kind, M):
    compare_with_variant_9(kind, M, 128, 384, 1, max_grid=1)


@pytest.mark.parametrize("kind", KINDS + OTHER_KINDS)
@pytest.mark.parametrize("grid", [3, 6])
def test_every_instantiation_one_and_two_blocks_per_panel(kind, grid):
    compare_with_variant_9(kind, 320, 384, 384, 1, max_grid=grid)


@pytest.mark.parametrize("kind", BT_KINDS)
@pytest.mark.parametrize("K", [64, 256, 384])
def test_transposed_panel_passes(kind, K):
    compare_with_variant_9(kind, 192, 256, K, 1)


@pytest.mark.parametrize("kind", [RELU_BWD_COLPART, RELU_BWD_NT])
@pytest.mark.parametrize("N", [128, 384])
def test_relu_bwd_extra_64_row_unit(kind, N):
    compare_with_variant_9(kind, 64 * bpp(N) + 64, N, 384, 0)


@pytest.mark.parametrize("N", [128, 384])
def test_relu_bwd_odd_tiles_per_block(N):
    compare_with_variant_9(RELU_BWD_COLPART, 192, N, 384, 1, max_grid=N // 128)


@pytest.mark.parametrize("kind", [STORE_NT, BIAS_RELU_BITS])
@pytest.mark.parametrize("how", ["device", "grid9"])
def test_leftover_32_row_unit(kind, how):
    if how == "grid9":
        compare_with_variant_9(kind, 128, 384, 384, 1, max_grid=9)
        return
    odd = [p for p in range(1, 13) if (2 * cus() // p) % 2 == 1]
    if odd:
        N = 128 * odd[-1]
        compare_with_variant_9(kind, 32 * bpp(N) + 32, N, 384, 0)
    else:   # no panel count with an odd bpp on this device: three blocks per panel by the grid cap
        compare_with_variant_9(kind, 128, 128, 384, 0, max_grid=3)


@pytest.mark.parametrize("kind", KINDS)
def test_every_slot_of_every_cu(kind):
    compare_with_variant_9(kind, 64 * 2 * cus(), 128, 64, 0)


def test_resident_blocks_per_cu():
    for bt in (0, 1):
        for kind in (EPI_STORE, EPI_BIAS_RELU, EPI_RELU_BWD):
            for nkt in range(1, 7):
                got = int(lib().cg_gemm_ws_blocks_per_cu(bt, kind, nkt))
                print(f"bt {bt} kind {kind} nkt {nkt}: {got} resident")
                assert got == 2   # exactly: the grid is 2 x CUs
    assert int(lib().cg_gemm_ws_blocks_per_cu(0, EPI_STORE, 7)) == -1
