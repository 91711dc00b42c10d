// charpt: the sequence-resident head_size-64 attention kernels for T <= 256 (the C2 path):
// k_attn_fwd_d64r, k_attn_dq_d64r, k_attn_dkdv_d64r and the merged backward k_attn_bwd_d64r.
// Tile helpers and structure notes: attention_d64_tile.h; launchers: attention_d64.hip.
#pragma once
#include "attention_d64_tile.h"

namespace cg {

#ifdef CG_ATTN_STAMPS
// Diagnostic build only (make attnstamps; tools/attn_stamps.py): per workgroup of the resident
// kernels, {start, operands landed (the prologue's wait), end} in s_memrealtime ticks (100 MHz) and
// {kind << 48 | XCC << 40 | HW_ID} -- written by lane 0 of wave 0 with a plain vector store into a
// buffer no other code reads.  Never in the product library.
constexpr int ATTN_STAMP_WG = 4096;
__device__ unsigned long long g_attn_stamps[ATTN_STAMP_WG * 4];
extern "C" int cg_debug_attn_stamps(unsigned long long* host, int n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_attn_stamps), (size_t)n * 4 * sizeof(unsigned long long)) ==
                   hipSuccess ? 0 : 1;
}
__device__ __forceinline__ void attn_stamp(int slot, unsigned long long v) {
    const int wg = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    if (threadIdx.x == 0 && wg < ATTN_STAMP_WG) {
        volatile unsigned long long* p = g_attn_stamps + 4 * wg + slot + (threadIdx.x & 63);
        *p = v;
    }
}
__device__ __forceinline__ unsigned long long attn_now() { return __builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ unsigned long long attn_where(int kind) {
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return ((unsigned long long)kind << 48) | ((unsigned long long)(xcc & 0xff) << 40) | hw;
}
#define ATTN_STAMP(slot, v) attn_stamp(slot, v)
#else
#define ATTN_STAMP(slot, v)
#endif

namespace {

// =====================================================================================
// T <= 256: sequence-resident kernels (the C2 shape, T = 256)
// =====================================================================================
// At T = 256 the ring kernels (attention_d64_ring.h) are latency-bound: a workgroup per (b, h) stages one 16-KB tile
// at a time through registers (one tile in flight per 256 threads), and 384 workgroups fill 1.5 of
// the 2 slots per CU (forward 23 us for 52.7 MB, 2.3 TB/s).  Here every K/V (or Q/dO) tile of the
// (b, h) is requested at once by LDS-DMA (64 KB per workgroup), the query-side (key-side) operands
// are loaded to registers right behind them, and after one wait + barrier the tile loop runs with
// no staging barriers.  Same wave/group assignment, per-tile arithmetic and keep-bit words as the
// ring kernels, so the results are bitwise the same.  (The register loads follow the DMAs: vmcnt
// retires in order, so waiting for them covers the tiles too -- see common.h dma16.)

// Resident forward (T = 64 NT <= 256).  Every load is issued up front -- the query-side operands
// first (Q fragments and keep words: hidden register loads, common.h gload16/gload4), then the
// K/V tiles in tile order by LDS-DMA -- and tile t waits only for what it reads: the register
// loads and tiles 0..t (vmcnt counts them in issue order), so the first tile's MFMAs start while
// the later tiles are still in flight.  Same per-tile arithmetic and keep words as the ring kernel.
template <bool DROP, int NT>
__global__ __launch_bounds__(256, 2) void k_attn_fwd_d64r(int H, const bf16_t* __restrict__ q,
                                                          const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                          int64_t ld, bf16_t* __restrict__ o, int64_t ldo,
                                                          float* __restrict__ lse, float scale_log2,
                                                          const uint32_t* __restrict__ mask, float dscale) {
    constexpr int T = 64 * NT;
    __shared__ __attribute__((aligned(16))) char smem[NT * 2 * TILE];   // K, V images of tile t at 2 t TILE
    ATTN_STAMP(0, attn_now());
    int x, bh;
    block_coords<false>(x, bh);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = bh / H, hh = bh % H;
    const int64_t boff = (int64_t)b * T, ntile = mask_tiles(T);
    const int qg[2] = {32 * (7 - wave), 32 * wave};   // A = 7 - w (longer causal prefix), B = w
    const bool act[2] = {qg[0] < T, qg[1] < T};
    sv8 qv[2][4];
    uint32_t mw[2][NT];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int qa = (act[g] ? qg[g] : 0) + (lane & 31);   // inactive groups load a valid row, unused
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) gload16(qv[g][ks], q + (boff + qa) * ld + hh * 64 + 16 * ks + 8 * (lane >> 5));
        if constexpr (DROP) {
            const int qb = act[g] ? qg[g] >> 5 : 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {   // tiles past the group's diagonal re-read tile 0 (unused)
                const int tt = 64 * t <= 32 * qb + 31 ? t : 0;
                gload4(mw[g][t], mask + ((int64_t)bh * ntile + mask_fwd_tile(qb, tt)) * 64 + lane);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        dma_tile(k + boff * ld + hh * 64, ld, 64 * t, lds_base(smem) + 2u * t * TILE, wave, lane);
        dma_tile(v + boff * ld + hh * 64, ld, 64 * t, lds_base(smem) + (2u * t + 1) * TILE, wave, lane);
    }
    // the register loads and tile 0 have landed (4 DMA instructions per tile per wave stay younger)
    if constexpr (!DROP) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < NT; ++t) mw[g][t] = 0u;
    }
    // then every destination is named "+v" by an (ordered, volatile) empty statement after the wait,
    // so nothing reads it earlier
    asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT - 1)) : "memory");
    ATTN_STAMP(1, attn_now());
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(qv[g][ks]));
#pragma unroll
        for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(mw[g][t]));
    }
    const sv8 (&qf)[2][4] = qv;
    fv16 oacc[2][2];
#pragma unroll
    for (int g = 0; g < 2; ++g) oacc[g][0] = oacc[g][1] = fv16{};
    float m_run[2] = {-FLT_MAX, -FLT_MAX};
    fv4 l_run[2] = {fv4{}, fv4{}};
    const sv8 ones = rowsum_ones(lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t) {   // tile t's DMAs (every wave's) have landed
            if constexpr (NT >= 2) {
                if (t == 1) asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT > 1 ? NT - 2 : 0)) : "memory");
            }
            if constexpr (NT >= 3) {
                if (t == 2) asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT > 2 ? NT - 3 : 0)) : "memory");
            }
            if constexpr (NT >= 4) {
                if (t == 3) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            }
        }
        const char* Ki = smem + 2 * t * TILE;
        const char* Vi = Ki + TILE;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (!act[g] || 64 * t > qg[g] + 31) continue;
            const int rel = __builtin_amdgcn_readfirstlane(qg[g] - 64 * t);
            if (rel >= 64)
                fwd_group_tile<DROP, 2, -1, true>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g], oacc[g],
                                                  mw[g][t], ones, qf[g]);
            else if (rel == 32)
                fwd_group_tile<DROP, 2, 1, true>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g], oacc[g],
                                                 mw[g][t], ones, qf[g]);
            else
                fwd_group_tile<DROP, 1, 0, true>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g], oacc[g],
                                                 mw[g][t], ones, qf[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (!act[g]) continue;
        const float lt = l_run[g][0];   // every accumulator register holds query lane & 31's sum
        const int64_t qa = qg[g] + (lane & 31);
        store_rows_wide(o + (boff + qa) * ldo + hh * 64, oacc[g], dscale / lt, lane);
        if (lane < 32) lse[(int64_t)bh * T + qa] = (m_run[g] + __log2f(lt)) * LN2;
    }
    ATTN_STAMP(2, attn_now());
    ATTN_STAMP(3, attn_where(2));
}

// The same on packed rows (k_attn_fwd_d64r_seg; a copy of the kernel above rather than a template flag
// on it: sharing the body moved the unsegmented kernels' register allocation -- so SEG is always true
// here, and marks the lines the copy adds).  Each lane also loads its queries' seg_start / seg_end
// (int32 [B][T]) with the other register operands; key tiles wholly before every lane's segment are
// skipped, the others masked per lane (fwd_group_tile).
template <bool DROP, int NT, bool SEG>
__device__ __forceinline__ void fwd_res(int H, const bf16_t* __restrict__ q,
                                        const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t ld,
                                        bf16_t* __restrict__ o, int64_t ldo, float* __restrict__ lse,
                                        float scale_log2, const uint32_t* __restrict__ mask, float dscale,
                                        const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_end) {
    constexpr int T = 64 * NT;
    __shared__ __attribute__((aligned(16))) char smem[NT * 2 * TILE];   // K, V images of tile t at 2 t TILE
    ATTN_STAMP(0, attn_now());
    int x, bh;
    block_coords<false>(x, bh);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = bh / H, hh = bh % H;
    const int64_t boff = (int64_t)b * T, ntile = mask_tiles(T);
    const int qg[2] = {32 * (7 - wave), 32 * wave};   // A = 7 - w (longer causal prefix), B = w
    const bool act[2] = {qg[0] < T, qg[1] < T};
    sv8 qv[2][4];
    uint32_t mw[2][NT], ssw[2] = {0u, 0u}, sew[2] = {0u, 0u};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int qa = (act[g] ? qg[g] : 0) + (lane & 31);   // inactive groups load a valid row, unused
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) gload16(qv[g][ks], q + (boff + qa) * ld + hh * 64 + 16 * ks + 8 * (lane >> 5));
        if constexpr (SEG) {
            gload4(ssw[g], seg_start + boff + qa);
            gload4(sew[g], seg_end + boff + qa);
        }
        if constexpr (DROP) {
            const int qb = act[g] ? qg[g] >> 5 : 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {   // tiles past the group's diagonal re-read tile 0 (unused)
                const int tt = 64 * t <= 32 * qb + 31 ? t : 0;
                gload4(mw[g][t], mask + ((int64_t)bh * ntile + mask_fwd_tile(qb, tt)) * 64 + lane);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        dma_tile(k + boff * ld + hh * 64, ld, 64 * t, lds_base(smem) + 2u * t * TILE, wave, lane);
        dma_tile(v + boff * ld + hh * 64, ld, 64 * t, lds_base(smem) + (2u * t + 1) * TILE, wave, lane);
    }
    // the register loads and tile 0 have landed (4 DMA instructions per tile per wave stay younger)
    if constexpr (!DROP) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < NT; ++t) mw[g][t] = 0u;
    }
    // then every destination is named "+v" by an (ordered, volatile) empty statement after the wait,
    // so nothing reads it earlier
    asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT - 1)) : "memory");
    ATTN_STAMP(1, attn_now());
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(qv[g][ks]));
#pragma unroll
        for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(mw[g][t]));
        if constexpr (SEG) asm volatile("" : "+v"(ssw[g]), "+v"(sew[g]));
    }
    int ss[2] = {0, 0};
    uint32_t peers[2] = {0u, 0u};
    if constexpr (SEG) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (!act[g]) continue;
            const int qa = qg[g] + (lane & 31);
            ss[g] = seg_lo(ssw[g], qa);
            peers[g] = seg_peers(ss[g], seg_hi(sew[g], qa), qg[g]);
        }
    }
    const sv8 (&qf)[2][4] = qv;
    fv16 oacc[2][2];
#pragma unroll
    for (int g = 0; g < 2; ++g) oacc[g][0] = oacc[g][1] = fv16{};
    float m_run[2] = {-FLT_MAX, -FLT_MAX};
    fv4 l_run[2] = {fv4{}, fv4{}};
    const sv8 ones = rowsum_ones(lane);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t) {   // tile t's DMAs (every wave's) have landed
            if constexpr (NT >= 2) {
                if (t == 1) asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT > 1 ? NT - 2 : 0)) : "memory");
            }
            if constexpr (NT >= 3) {
                if (t == 2) asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT > 2 ? NT - 3 : 0)) : "memory");
            }
            if constexpr (NT >= 4) {
                if (t == 3) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            }
        }
        const char* Ki = smem + 2 * t * TILE;
        const char* Vi = Ki + TILE;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (!act[g] || 64 * t > qg[g] + 31) continue;
            const int rel = __builtin_amdgcn_readfirstlane(qg[g] - 64 * t);
            const int srel = SEG ? ss[g] - 64 * t : 0;
            if constexpr (SEG) {
                if (__all(srel >= 64)) continue;   // the tile precedes every lane's segment
            }
            if (rel >= 64)
                fwd_group_tile<DROP, 2, -1, true, SEG>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g],
                                                       oacc[g], mw[g][t], ones, qf[g], srel, peers[g]);
            else if (rel == 32)
                fwd_group_tile<DROP, 2, 1, true, SEG>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g],
                                                      oacc[g], mw[g][t], ones, qf[g], srel, peers[g]);
            else
                fwd_group_tile<DROP, 1, 0, true, SEG>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g],
                                                      oacc[g], mw[g][t], ones, qf[g], srel, peers[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (!act[g]) continue;
        const float lt = l_run[g][0];   // every accumulator register holds query lane & 31's sum
        const int64_t qa = qg[g] + (lane & 31);
        store_rows_wide(o + (boff + qa) * ldo + hh * 64, oacc[g], dscale / lt, lane);
        if (lane < 32) lse[(int64_t)bh * T + qa] = (m_run[g] + __log2f(lt)) * LN2;
    }
    ATTN_STAMP(2, attn_now());
    ATTN_STAMP(3, attn_where(2));
}

template <bool DROP, int NT>
__global__ __launch_bounds__(256, 2) void k_attn_fwd_d64r_seg(int H, const bf16_t* __restrict__ q,
                                                              const bf16_t* __restrict__ k,
                                                              const bf16_t* __restrict__ v, int64_t ld,
                                                              bf16_t* __restrict__ o, int64_t ldo,
                                                              float* __restrict__ lse, float scale_log2,
                                                              const uint32_t* __restrict__ mask, float dscale,
                                                              const int32_t* __restrict__ seg_start,
                                                              const int32_t* __restrict__ seg_end) {
    fwd_res<DROP, NT, true>(H, q, k, v, ld, o, ldo, lse, scale_log2, mask, dscale, seg_start, seg_end);
}

// tile t > 0 of a resident kernel: this wave's DMAs of tiles 0..t have landed (4 DMA instructions per
// tile per wave, issued in tile order after the first register loads; X hidden loads issued after the
// DMAs stay in flight too), then every wave's (barrier)
template <int NT, int X = 0>
__device__ __forceinline__ void res_tile_wait(int t) {
    if constexpr (NT >= 2) {
        if (t == 1) asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT > 1 ? NT - 2 : 0) + X) : "memory");
    }
    if constexpr (NT >= 3) {
        if (t == 2) asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT > 2 ? NT - 3 : 0) + X) : "memory");
    }
    if constexpr (NT >= 4) {
        if (t == 3) asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(X) : "memory");
    }
}

// Resident dQ (T = 64 NT <= 256): the query-side operands (Q, dO and O fragments, lse, keep words)
// by hidden register loads first, then the K/V tiles by LDS-DMA in tile order; tile t waits only
// for tiles 0..t (as k_attn_fwd_d64r).  Per-group setup (delta in dq_group_setup's summation order)
// and per-tile arithmetic as the ring kernel.
template <bool DROP, int NT, bool DIN = false, bool SEG = false>
__device__ __forceinline__ void dq_res(int bh, char* smem, int H, const bf16_t* __restrict__ q,
                                       const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t ld,
                                       const bf16_t* __restrict__ o, int64_t ldo, const bf16_t* __restrict__ dout,
                                       int64_t ldd, const float* __restrict__ lse, float* __restrict__ delta,
                                       bf16_t* __restrict__ dq, int64_t lddq, float scale,
                                       const uint32_t* __restrict__ mask, float dscale,
                                       const int32_t* __restrict__ seg_start = nullptr) {
    constexpr int T = 64 * NT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = bh / H, hh = bh % H;
    const int64_t boff = (int64_t)b * T, ntile = mask_tiles(T);
    const float c2 = scale * LOG2E;
    const int qg[2] = {32 * (7 - wave), 32 * wave};
    const bool act[2] = {qg[0] < T, qg[1] < T};
    sv8 qf[2][4], df[2][4], of[2][4];
    uint32_t lsew[2], delw[2] = {0u, 0u}, mw[2][NT], ssw[2] = {0u, 0u};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int64_t qa = (act[g] ? qg[g] : 0) + (lane & 31);   // inactive groups: a valid row, unused
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int col = hh * 64 + 16 * ks + 8 * (lane >> 5);
            gload16(qf[g][ks], q + (boff + qa) * ld + col);
            gload16(df[g][ks], dout + (boff + qa) * ldd + col);
            if constexpr (!DIN) gload16(of[g][ks], o + (boff + qa) * ldo + col);
        }
        gload4(lsew[g], lse + (int64_t)bh * T + qa);
        if constexpr (DIN) gload4(delw[g], delta + (int64_t)bh * T + qa);
        if constexpr (SEG) gload4(ssw[g], seg_start + boff + qa);
        if constexpr (DROP) {
            const int qb = act[g] ? qg[g] >> 5 : 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int tt = 64 * t <= 32 * qb + 31 ? t : 0;
                gload4(mw[g][t], mask + ((int64_t)bh * ntile + mask_fwd_tile(qb, tt)) * 64 + lane);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        dma_tile(k + boff * ld + hh * 64, ld, 64 * t, lds_base(smem) + 2u * t * TILE, wave, lane);
        dma_tile(v + boff * ld + hh * 64, ld, 64 * t, lds_base(smem) + (2u * t + 1) * TILE, wave, lane);
    }
    if constexpr (!DROP) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < NT; ++t) mw[g][t] = 0u;
    }
    asm volatile("s_waitcnt vmcnt(%c0)\n\ts_barrier" ::"i"(4 * (NT - 1)) : "memory");
    ATTN_STAMP(1, attn_now());
#pragma unroll
    for (int g = 0; g < 2; ++g) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            asm volatile("" : "+v"(qf[g][ks]));
            asm volatile("" : "+v"(df[g][ks]));
            if constexpr (!DIN) asm volatile("" : "+v"(of[g][ks]));
        }
        asm volatile("" : "+v"(lsew[g]), "+v"(delw[g]));
        if constexpr (SEG) asm volatile("" : "+v"(ssw[g]));
#pragma unroll
        for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(mw[g][t]));
    }
    float lse2[2], dl[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {   // dq_group_setup's arithmetic on the loaded fragments
        float dsum = 0.f;
        if constexpr (DIN) {
            dsum = act[g] ? __uint_as_float(delw[g]) : 0.f;
        } else {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int j = 0; j < 8; ++j) dsum += bf2f((bf16_t)of[g][ks][j]) * bf2f((bf16_t)df[g][ks][j]);
            if (!act[g]) dsum = 0.f;
            dsum += __shfl_xor(dsum, 32, 64);
        }
        dl[g] = -dsum / dscale;
        lse2[g] = act[g] ? __uint_as_float(lsew[g]) * LOG2E : 0.f;
        if (!DIN && act[g] && lane < 32) delta[(int64_t)bh * T + qg[g] + (lane & 31)] = dsum;
    }
    fv16 dqa[2][2];
#pragma unroll
    for (int g = 0; g < 2; ++g) dqa[g][0] = dqa[g][1] = fv16{};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        res_tile_wait<NT>(t);
        const char* Ki = smem + 2 * t * TILE;
#pragma unroll
        for (int g = 0; g < 2; ++g)
            if (act[g] && 64 * t <= qg[g] + 31)
                dq_group_tile<DROP, SEG>(Ki, Ki + TILE, 64 * t, qg[g], qf[g], df[g], lse2[g], dl[g], mw[g][t], c2,
                                         dqa[g], lane, SEG ? seg_lo(ssw[g], qg[g] + (lane & 31)) : 0);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (!act[g]) continue;
        const int64_t qa = qg[g] + (lane & 31);
        store_rows_wide(dq + (boff + qa) * lddq + hh * 64, dqa[g], scale * dscale, lane);
    }
}

template <bool DROP, int NT>
__global__ __launch_bounds__(256, 2) void k_attn_dq_d64r(int H, const bf16_t* __restrict__ q,
                                                         const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                         int64_t ld, const bf16_t* __restrict__ o, int64_t ldo,
                                                         const bf16_t* __restrict__ dout, int64_t ldd,
                                                         const float* __restrict__ lse, float* __restrict__ delta,
                                                         bf16_t* __restrict__ dq, int64_t lddq, float scale,
                                                         const uint32_t* __restrict__ mask, float dscale) {
    __shared__ __attribute__((aligned(16))) char smem[NT * 2 * TILE];
    int x, bh;
    block_coords<false>(x, bh);
    dq_res<DROP, NT>(bh, smem, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, scale, mask, dscale);
}

// dK/dV: one workgroup per (b, h); wave w takes key group w, then key group 7 - w (equal causal
// work per wave: 8 + 1, 7 + 2, ... 32-query subtiles at T = 256), Q / dO / lse / delta resident.
// o != NULL: delta = rowsum(dO * O) is computed here (in dq_group_setup's summation order, so
// bitwise the dQ kernel's value) instead of read from `delta` -- the merged backward launch.
// Register operands (row statistics, the first key group's K / V fragments, keep words) by hidden
// loads first, then the Q / dO tiles by LDS-DMA; the first key group's tile t waits only for tiles
// 0..t.  OD: delta from O and dO (o != NULL), else read from `delta`.
template <bool DROP, int NT, bool OD, bool SEG = false>
__device__ __forceinline__ void dkdv_res(int bh, char* smem, int H, const bf16_t* __restrict__ q,
                                         const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t ld,
                                         const bf16_t* __restrict__ dout, int64_t ldd, const float* __restrict__ lse,
                                         const float* __restrict__ delta, const bf16_t* __restrict__ o, int64_t ldo,
                                         bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int64_t lddkv, float scale,
                                         const uint32_t* __restrict__ mask, float dscale,
                                         const int32_t* __restrict__ seg_end = nullptr) {
    constexpr int T = 64 * NT;
    float* st_lse = (float*)(smem + NT * 2 * TILE);
    float* st_del = st_lse + T;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = bh / H, hh = bh % H;
    const int64_t boff = (int64_t)b * T, ntile = mask_tiles(T);
    const float c2 = scale * LOG2E;
    const int kqs[2] = {32 * wave, 32 * (7 - wave)};
    const bf16_t* kb_ = k + boff * ld + hh * 64;
    const bf16_t* vb_ = v + boff * ld + hh * 64;
    const bool srow = tid < T;   // whole waves (T % 64 == 0)
    const int64_t sr = srow ? tid : 0;
    uint32_t lsew = 0u, delw = 0u;
    sv8 ov[2][4], dv_[2][4];   // O / dO row of query tid: halves h, columns 16 ks + 8 h .. +7
    if (srow) {
        gload4(lsew, lse + (int64_t)bh * T + sr);
        if constexpr (OD) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    gload16(ov[h][ks], o + (boff + sr) * ldo + hh * 64 + 16 * ks + 8 * h);
                    gload16(dv_[h][ks], dout + (boff + sr) * ldd + hh * 64 + 16 * ks + 8 * h);
                }
        } else {
            gload4(delw, delta + (int64_t)bh * T + sr);
        }
    }
    uint32_t mw[2][NT];
    if constexpr (DROP) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int kbw = kqs[p] >> 5, qtm = kbw >> 1;
            const bool ok = kqs[p] < T;
#pragma unroll
            for (int t = 0; t < NT; ++t) {   // tiles before the key group's first query tile re-read its first
                const int tt = ok && t >= qtm ? t - qtm : 0;
                gload4(mw[p][t], mask + ((int64_t)bh * ntile + mask_bwd_tile(ok ? kbw : 0, ok ? qtm : 0, NT)) * 64 +
                                     lane + tt * 64);
            }
        }
    }
    uint32_t sew[2] = {0u, 0u};   // SEG: the segment end of this lane's key, per key group
    if constexpr (SEG) {
#pragma unroll
        for (int p = 0; p < 2; ++p) gload4(sew[p], seg_end + boff + (kqs[p] < T ? kqs[p] : 0) + (lane & 31));
    }
    sv8 kf[4], vf[4];
    {
        const int key0 = (kqs[0] < T ? kqs[0] : 0) + (lane & 31);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            gload16(kf[ks], kb_ + (int64_t)key0 * ld + 16 * ks + 8 * (lane >> 5));
            gload16(vf[ks], vb_ + (int64_t)key0 * ld + 16 * ks + 8 * (lane >> 5));
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        dma_tile(q + boff * ld + hh * 64, ld, 64 * t, lds_base(smem) + 2u * t * TILE, wave, lane);
        dma_tile(dout + boff * ldd + hh * 64, ldd, 64 * t, lds_base(smem) + (2u * t + 1) * TILE, wave, lane);
    }
    // the second key group's K / V fragments behind the tiles (in flight until that group starts)
    sv8 kf1[4], vf1[4];
    {
        const int key1 = (kqs[1] < T ? kqs[1] : 0) + (lane & 31);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            gload16(kf1[ks], kb_ + (int64_t)key1 * ld + 16 * ks + 8 * (lane >> 5));
            gload16(vf1[ks], vb_ + (int64_t)key1 * ld + 16 * ks + 8 * (lane >> 5));
        }
    }
    asm volatile("s_waitcnt vmcnt(%c0)" ::"i"(4 * (NT - 1) + 8) : "memory");
    asm volatile("" : "+v"(lsew), "+v"(delw));
    if constexpr (SEG) asm volatile("" : "+v"(sew[0]), "+v"(sew[1]));
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            asm volatile("" : "+v"(ov[h][ks]));
            asm volatile("" : "+v"(dv_[h][ks]));
        }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        asm volatile("" : "+v"(kf[ks]));
        asm volatile("" : "+v"(vf[ks]));
    }
    if constexpr (DROP) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(mw[p][t]));
    } else {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int t = 0; t < NT; ++t) mw[p][t] = 0u;
    }
    if (srow) {
        st_lse[tid] = __uint_as_float(lsew) * LOG2E;
        float dsum;
        if constexpr (OD) {   // query tid: halves h = 0, 1 (columns 16 ks + 8 h + j) summed as dq_group_setup's lanes
            float sh[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float acc = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc += bf2f((bf16_t)ov[h][ks][j]) * bf2f((bf16_t)dv_[h][ks][j]);
                sh[h] = acc;
            }
            dsum = sh[0] + sh[1];
        } else {
            dsum = __uint_as_float(delw);
        }
        st_del[tid] = -dsum / dscale;   // -delta' = -(1-p) delta
    }
    // the row statistics are visible to every wave, and tile 0 has landed for every wave
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    ATTN_STAMP(1, attn_now());
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int kq = kqs[p], key = kq + (lane & 31);
        const bool act = kq < T;
        if (p) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                asm volatile("" : "+v"(kf1[ks]));
                asm volatile("" : "+v"(vf1[ks]));
                kf[ks] = kf1[ks];
                vf[ks] = vf1[ks];
            }
        }
        fv16 dka[2] = {fv16{}, fv16{}}, dva[2] = {fv16{}, fv16{}};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (!p) res_tile_wait<NT, 8>(t);
            if (act && 64 * t + 63 >= kq)
                dkdv_tile<DROP, SEG>(smem + 2 * t * TILE, smem + (2 * t + 1) * TILE, st_lse + 64 * t, st_del + 64 * t,
                                     64 * t, kq, key, kf, vf, mw[p][t], c2, dka, dva, lane,
                                     SEG ? seg_hi(sew[p], key) : 0);
        }
        if (act) {
            store_rows_wide(dk + (boff + key) * lddkv + hh * 64, dka, scale * dscale, lane);
            store_rows_wide(dv + (boff + key) * lddkv + hh * 64, dva, DROP ? dscale : 1.f, lane);
        }
    }
}

template <bool DROP, int NT>
__global__ __launch_bounds__(256, 2) void k_attn_dkdv_d64r(int H, const bf16_t* __restrict__ q,
                                                           const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                           int64_t ld, const bf16_t* __restrict__ dout, int64_t ldd,
                                                           const float* __restrict__ lse,
                                                           const float* __restrict__ delta, bf16_t* __restrict__ dk,
                                                           bf16_t* __restrict__ dv, int64_t lddkv, float scale,
                                                           const uint32_t* __restrict__ mask, float dscale) {
    __shared__ __attribute__((aligned(16))) char smem[NT * 2 * TILE + 2 * 64 * NT * 4];
    int x, bh;
    block_coords<false>(x, bh);
    dkdv_res<DROP, NT, false>(bh, smem, H, q, k, v, ld, dout, ldd, lse, delta, nullptr, 0, dk, dv, lddkv, scale, mask,
                       dscale);
}

// The whole T <= 256 backward in one launch: workgroup 2i computes dQ of (b, h) = i, 2i + 1 its
// dK/dV (with delta from O and dO itself, so the two do not depend on each other; DIN: both read
// delta, precomputed by the dO GEMM's epilogue, and neither loads O).  768
// workgroups fill the 512 slots and the second wave of them starts as slots free up, where the
// two separate 384-workgroup launches each ran 3/4 full and back to back.  The pair of one (b, h)
// stays on one XCD (block_coords: consecutive logical ids), sharing its K/V/Q/dO lines in L2.
template <bool DROP, int NT, bool DIN, bool SEG>
__device__ __forceinline__ void bwd_res(char* smem, int H, const bf16_t* __restrict__ q,
                                        const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t ld,
                                        const bf16_t* __restrict__ o, int64_t ldo, const bf16_t* __restrict__ dout,
                                        int64_t ldd, const float* __restrict__ lse, float* __restrict__ delta,
                                        bf16_t* __restrict__ dq, int64_t lddq, bf16_t* __restrict__ dk,
                                        bf16_t* __restrict__ dv, int64_t lddkv, float scale,
                                        const uint32_t* __restrict__ mask_fwd, const uint32_t* __restrict__ mask_bwd,
                                        float dscale, int lpt, const int32_t* __restrict__ seg_start,
                                        const int32_t* __restrict__ seg_end) {
    ATTN_STAMP(0, attn_now());
    int x, id;
    const int n = (int)gridDim.y, w = (int)blockIdx.y;
    if (lpt && (n & 15) == 0) {
        // longest first within each XCD: the dispatcher deals workgroup w to XCD w & 7, in order of
        // w >> 3 there; each XCD owns n/16 consecutive (b, h) and runs all their dK/dV workgroups (22 us
        // at C2) before their dQ workgroups (16 us), so the 1.5-round grid's second round is dQ only
        const int half = n >> 4, xcd = w & 7, j = w >> 3, bh0 = xcd * half;
        id = j < half ? 2 * (bh0 + j) + 1 : 2 * (bh0 + j - half);
    } else {
        block_coords<false>(x, id);
    }
    if (id & 1)
        dkdv_res<DROP, NT, !DIN, SEG>(id >> 1, smem, H, q, k, v, ld, dout, ldd, lse, delta, o, ldo, dk, dv, lddkv,
                                      scale, mask_bwd, dscale, seg_end);
    else
        dq_res<DROP, NT, DIN, SEG>(id >> 1, smem, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, scale,
                                   mask_fwd, dscale, seg_start);
    ATTN_STAMP(2, attn_now());
    ATTN_STAMP(3, attn_where(id & 1));
}

template <bool DROP, int NT, bool DIN>
__global__ __launch_bounds__(256, 2) void k_attn_bwd_d64r(int H, const bf16_t* __restrict__ q,
                                                          const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                          int64_t ld, const bf16_t* __restrict__ o, int64_t ldo,
                                                          const bf16_t* __restrict__ dout, int64_t ldd,
                                                          const float* __restrict__ lse, float* __restrict__ delta,
                                                          bf16_t* __restrict__ dq, int64_t lddq, bf16_t* __restrict__ dk,
                                                          bf16_t* __restrict__ dv, int64_t lddkv, float scale,
                                                          const uint32_t* __restrict__ mask_fwd,
                                                          const uint32_t* __restrict__ mask_bwd, float dscale,
                                                          int lpt) {
    __shared__ __attribute__((aligned(16))) char smem[NT * 2 * TILE + 2 * 64 * NT * 4];
    bwd_res<DROP, NT, DIN, false>(smem, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, dk, dv, lddkv, scale,
                                  mask_fwd, mask_bwd, dscale, lpt, nullptr, nullptr);
}

// the same for packed rows: dQ reads seg_start, dK/dV seg_end (int32 [B][T])
template <bool DROP, int NT, bool DIN>
__global__ __launch_bounds__(256, 2) void k_attn_bwd_d64r_seg(
    int H, const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t ld,
    const bf16_t* __restrict__ o, int64_t ldo, const bf16_t* __restrict__ dout, int64_t ldd,
    const float* __restrict__ lse, float* __restrict__ delta, bf16_t* __restrict__ dq, int64_t lddq,
    bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int64_t lddkv, float scale,
    const uint32_t* __restrict__ mask_fwd, const uint32_t* __restrict__ mask_bwd, float dscale, int lpt,
    const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_end) {
    __shared__ __attribute__((aligned(16))) char smem[NT * 2 * TILE + 2 * 64 * NT * 4];
    bwd_res<DROP, NT, DIN, true>(smem, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, dk, dv, lddkv, scale,
                                 mask_fwd, mask_bwd, dscale, lpt, seg_start, seg_end);
}

}  // namespace

}  // namespace cg
