// charpt: what the persistent LDS-DMA bf16 GEMM kernels share -- k_gemm_pk (gemm_pk.hip) and the grouped
// split-K weight-gradient kernel (gemm_pk_group.hip): the vmcnt wait, a lane's LDS-DMA sources and the
// block geometry.  A diagnostic build (CG_PK_BOUNDS) defines bounds_chk before including this.
#pragma once
#include "gemm_tile.h"

namespace cg {
namespace {
using namespace gt;

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// per-lane part of one operand's LDS-DMA sources: R rows (K-contiguous) or R columns (TR) x BK k
template <bool TR, int R, int WAVES, int BK>
struct DmaP {
    static constexpr int INSTR = R * BK * 2 / 1024;  // 1-KB wave instructions per K-tile
    static constexpr int PER_WAVE = INSTR / WAVES;
    static_assert(PER_WAVE * WAVES == INSTR, "tile/wave mismatch");
    static_assert(!TR || R >= 128, "transposed image swizzle needs >= 16 chunks per row");
    uint32_t off[PER_WAVE];  // byte offset of this lane's 16-B chunk from the tile origin
    int64_t kstep;
#ifdef CG_PK_BOUNDS
    const void* lo = nullptr;
    const void* hi = nullptr;
    int slot = 0;
#endif

    __device__ __forceinline__ void init(int64_t ld, int wave, int lane) {
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const int pos = (wave * PER_WAVE + i) * 1024 + lane * 16;
            if (!TR) {
                const int r = BK == 64 ? pos >> 7 : pos >> 6;
                const int c = BK == 64 ? ((pos >> 4) & 7) ^ row_swz(r) : ((pos >> 4) & 3) ^ row_swz32(r);
                off[i] = 2u * (uint32_t)((int)(r * ld) + c * 8);
            } else {
                const int k = pos / (2 * R), c = ((pos % (2 * R)) >> 4) ^ col_swz(k);
                off[i] = 2u * (uint32_t)((int)(k * ld) + c * 8);
            }
        }
        kstep = TR ? (int64_t)BK * ld : (int64_t)BK;
    }
    // instruction i (0..PER_WAVE-1) of one K-tile, from that K-tile's (wave-uniform) base address into
    // the image at 32-bit LDS address img: the saddr form (SGPR base + per-lane byte offset) and an
    // SGPR LDS address.  With a generic image pointer and a 64-bit lane address hipcc spent ~6
    // instructions per DMA (two 64-bit VALU adds, two v_readfirstlane, a null-pointer select) on a
    // VALU -> SGPR -> m0 dependency chain.
    __device__ __forceinline__ void issue1(const bf16_t* base, int i, uint32_t img, int wave) const {
#ifdef CG_PK_BOUNDS
        bounds_chk((const char*)base + off[i], 16, lo, hi, slot);
#endif
        dma16sl(base, off[i], img + (uint32_t)((wave * PER_WAVE + i) * 1024));
    }
};

// Wave grid: 64 x 64 wave tiles, except BN = 96 (two 64 x 48 wave tiles per 64-row band: NJ = 3
// fragments of 16 columns instead of 4).
template <int BM, int BN, int NBUF, int BK = FBK>
struct GeoP {
    static constexpr int WM = BM / 64, WN = BN == 96 ? 2 : BN / 64, WAVES = WM * WN, THREADS = WAVES * 64;
    static constexpr int WTN = BN / WN, NJ = WTN / 16;   // wave tile columns, 16-column fragments per wave
    static_assert(WTN == 64 || WTN == 48, "wave tile");
    static constexpr int IMG_A = BM * BK * 2, IMG_B = BN * BK * 2, STAGE = IMG_A + IMG_B;
    static constexpr int LDS = NBUF * STAGE;
    static constexpr int OCC_LDS = (160 * 1024) / LDS;
    static constexpr int OCC = OCC_LDS > 4 ? 4 : (OCC_LDS < 1 ? 1 : OCC_LDS);  // resident blocks per CU (LDS-bound)
    static constexpr int WPE = (WAVES * OCC + 3) / 4;   // waves per SIMD
};

}  // namespace
}  // namespace cg
