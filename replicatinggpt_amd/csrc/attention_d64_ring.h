// charpt: the head_size-64 attention kernels that stream K/V (or Q/dO) tiles through an LDS-DMA
// ring, for any T % 64 == 0 (the C4 path, T > 256): k_attn_dq_d64, k_attn_dkdv_d64 and
// k_attn_fwd_d64d.  Tile helpers and structure notes: attention_d64_tile.h; launchers:
// attention_d64.hip (the A/B-only instantiations: ab/attention_ab.hip).
#pragma once
#include "attention_d64_tile.h"

namespace cg {
namespace {

// =====================================================================================
// dQ (per-tile arithmetic: dq_group_tile)
// =====================================================================================
// query-side operands of one dQ group (query qa = qg + (lane & 31)): Q and dO fragments, lse in
// log2 units and -delta' = -(1-p) delta, where delta = rowsum(dO * O) (dropout-invariant: O already
// holds the dropped P) is also written for the dK/dV kernel.  Bases are the (b, h) row-0 pointers.
__device__ __forceinline__ void dq_group_setup(bool act, int64_t qa, const bf16_t* qb, int64_t ld, const bf16_t* ob,
                                               int64_t ldo, const bf16_t* db, int64_t ldd, const float* lse_bh,
                                               float* delta_bh, float dscale, int lane, sv8 (&qf)[4], sv8 (&df)[4],
                                               float& lse2, float& dl) {
    float dsum = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        qf[ks] = act ? ld_frag(qb, ld, qa, ks, lane) : sv8{};
        df[ks] = act ? ld_frag(db, ldd, qa, ks, lane) : sv8{};
        if (act) {
            const sv8 of = ld_frag(ob, ldo, qa, ks, lane);
#pragma unroll
            for (int j = 0; j < 8; ++j) dsum += bf2f((bf16_t)of[j]) * bf2f((bf16_t)df[ks][j]);
        }
    }
    dsum += __shfl_xor(dsum, 32, 64);
    dl = -dsum / dscale;   // -delta' = -(1-p) delta
    lse2 = act ? lse_bh[qa] * LOG2E : 0.f;
    if (act && lane < 32) delta_bh[qa] = dsum;
}

// K/V tiles by LDS-DMA (common.h dma16) into a 2-slot ring, the next tile's DMAs issued before the
// current tile's products (round 2: register staging measured 706 -> 686 us for the C4 backward)
// SEG (packed rows): each lane also holds its queries' segment start (dq_group_tile masks and skips)
template <bool DROP, int NS, bool SEG = false>
__device__ __forceinline__ void dq_qblock(int qblk, int bh, char* smem, int64_t T_, int H, const bf16_t* __restrict__ q,
                                          const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t ld,
                                          const bf16_t* __restrict__ o, int64_t ldo, const bf16_t* __restrict__ dout,
                                          int64_t ldd, const float* __restrict__ lse, float* __restrict__ delta,
                                          bf16_t* __restrict__ dq, int64_t lddq, float scale,
                                          const uint32_t* __restrict__ mask, float dscale,
                                          const int32_t* __restrict__ seg_start = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = (int)T_, b = bh / H, hh = bh % H;
    const int Q0 = qblk * 256;
    const int64_t boff = (int64_t)b * T_, ntile = mask_tiles(T_);
    const float c2 = scale * LOG2E;
    const bf16_t* kb_ = k + boff * ld + hh * 64;
    const bf16_t* vb_ = v + boff * ld + hh * 64;
    const int qg[2] = {Q0 + 32 * (7 - wave), Q0 + 32 * wave};
    const bool act[2] = {qg[0] < T, qg[1] < T};
    const uint32_t* mrow[2];
    uint32_t mw[2] = {0u, 0u};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        mrow[g] = DROP ? mask + ((int64_t)bh * ntile + mask_fwd_tile(qg[g] >> 5, 0)) * 64 + lane : nullptr;
        if (DROP && act[g]) mw[g] = mrow[g][0];
    }
    sv8 qf[2][4], df[2][4];
    float lse2[2], dl[2];
#pragma unroll
    for (int g = 0; g < 2; ++g)
        dq_group_setup(act[g], qg[g] + (lane & 31), q + boff * ld + hh * 64, ld, o + boff * ldo + hh * 64, ldo,
                       dout + boff * ldd + hh * 64, ldd, lse + (int64_t)bh * T_, delta + (int64_t)bh * T_, dscale, lane,
                       qf[g], df[g], lse2[g], dl[g]);
    int ss[2] = {0, 0};
    if constexpr (SEG) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
            if (act[g]) ss[g] = seg_lo((uint32_t)seg_start[boff + qg[g] + (lane & 31)], qg[g] + (lane & 31));
    }
    fv16 dqa[2][2];
#pragma unroll
    for (int g = 0; g < 2; ++g) dqa[g][0] = dqa[g][1] = fv16{};
    const int qlast = (Q0 + 255 < T - 1) ? Q0 + 255 : T - 1;
    const int nkv = qlast / 64 + 1;
    const int wave_ = __builtin_amdgcn_readfirstlane(tid >> 6);
    // K/V ring of NS slots, tile kv + AH requested at the head of tile kv into the slot of tile
    // kv + AH - NS (read before an earlier barrier); NS = 4: two tiles of compute to land
    constexpr int AH = NS / 2;
    auto slot = [&](int t) { return smem + (t & (NS - 1)) * 2 * TILE; };
    const uint32_t l0 = lds_base(smem);
    auto lslot = [&](int t) { return l0 + (uint32_t)((t & (NS - 1)) * 2 * TILE); };
#pragma unroll
    for (int t = 0; t < AH; ++t) {
        if (t < nkv) {
            dma_tile(kb_, ld, (int64_t)t * 64, lslot(t), wave_, lane);
            dma_tile(vb_, ld, (int64_t)t * 64, lslot(t) + TILE, wave_, lane);
        }
    }
    ring_wait<AH == 2 ? 4 : 0>(AH == 2 && nkv > 1);   // operands and tile 0 have landed
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) mark_ready(qf[g][ks], df[g][ks]);
    mark_ready(mw[0], mw[1], lse2[0], lse2[1], dl[0], dl[1]);
    if constexpr (SEG) mark_ready(ss[0], ss[1]);
    for (int kv = 0; kv < nkv; ++kv) {
        const int nxt = kv + 1 < nkv ? kv + 1 : kv;
        // the next tile's keep words by hidden loads, issued before the DMAs so that the counted wait
        // at the tile's end retires them (a compiler-counted load issued after the DMAs made hipcc
        // wait vmcnt(0) -- for the DMAs too -- at the head of the tile)
        uint32_t mn[2] = {0u, 0u};
        if constexpr (DROP) {
#pragma unroll
            for (int g = 0; g < 2; ++g)
                if (act[g] && nxt * 64 <= qg[g] + 31) gload4(mn[g], mrow[g] + nxt * 64);
        }
        const bool pf = kv + AH < nkv;
        if (pf) {
            dma_tile(kb_, ld, (int64_t)(kv + AH) * 64, lslot(kv + AH), wave_, lane);
            dma_tile(vb_, ld, (int64_t)(kv + AH) * 64, lslot(kv + AH) + TILE, wave_, lane);
        }
        const char* Ki = slot(kv);
        const int k0 = kv * 64;
#pragma unroll
        for (int g = 0; g < 2; ++g)
            if (act[g] && k0 <= qg[g] + 31)
                dq_group_tile<DROP, SEG>(Ki, Ki + TILE, k0, qg[g], qf[g], df[g], lse2[g], dl[g], mw[g], c2, dqa[g], lane,
                                         ss[g]);
        ring_wait<AH == 2 ? 4 : 0>(pf);   // tile kv + 1 (and the keep words) have landed for every wave
        asm volatile("" : "+v"(mn[0]), "+v"(mn[1]));
        mw[0] = mn[0];
        mw[1] = mn[1];
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (!act[g]) continue;
        const int64_t qa = qg[g] + (lane & 31);
        store_rows(dq + (boff + qa) * lddq + hh * 64, dqa[g], scale * dscale, lane);
    }
}

// pairs of query blocks per workgroup, as the forward
template <bool DROP, int NS>
__global__ __launch_bounds__(256, 2) void k_attn_dq_d64(int64_t T_, int H, const bf16_t* __restrict__ q,
                                                        const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                        int64_t ld, const bf16_t* __restrict__ o, int64_t ldo,
                                                        const bf16_t* __restrict__ dout, int64_t ldd,
                                                        const float* __restrict__ lse, float* __restrict__ delta,
                                                        bf16_t* __restrict__ dq, int64_t lddq, float scale,
                                                        const uint32_t* __restrict__ mask, float dscale) {
    __shared__ __attribute__((aligned(16))) char smem[NS * 2 * TILE];
    int x, bh;
    block_coords<false>(x, bh);
    const int nq = (int)((T_ + 255) / 256), first = nq - 1 - x;
    const int npass = x == first ? 1 : 2;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
        if (pass) __syncthreads();
        dq_qblock<DROP, NS>(pass ? x : first, bh, smem, T_, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, scale,
                        mask, dscale);
    }
}

template <bool DROP, int NS>
__global__ __launch_bounds__(256, 2) void k_attn_dq_d64_seg(int64_t T_, int H, const bf16_t* __restrict__ q,
                                                            const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                            int64_t ld, const bf16_t* __restrict__ o, int64_t ldo,
                                                            const bf16_t* __restrict__ dout, int64_t ldd,
                                                            const float* __restrict__ lse, float* __restrict__ delta,
                                                            bf16_t* __restrict__ dq, int64_t lddq, float scale,
                                                            const uint32_t* __restrict__ mask, float dscale,
                                                            const int32_t* __restrict__ seg_start) {
    __shared__ __attribute__((aligned(16))) char smem[NS * 2 * TILE];
    int x, bh;
    block_coords<false>(x, bh);
    const int nq = (int)((T_ + 255) / 256), first = nq - 1 - x;
    const int npass = x == first ? 1 : 2;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
        if (pass) __syncthreads();
        dq_qblock<DROP, NS, true>(pass ? x : first, bh, smem, T_, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq,
                                  scale, mask, dscale, seg_start);
    }
}

// =====================================================================================
// dK / dV: block = 4 waves x 32 keys; stream 64-query tiles (Q, dO, lse, delta)
// =====================================================================================
constexpr int KV_STAGE = 2 * TILE + 512;   // Q image, dO image, lse*log2e [64], delta [64]

// SEG (packed rows): each lane also holds the end of its key's segment (dkdv_tile masks and skips)
template <bool DROP, int NS, bool SEG = false>
__device__ __forceinline__ void dkdv_kblock(int kblk, int bh, char* smem, int64_t T_, int H,
                                            const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                            const bf16_t* __restrict__ v, int64_t ld, const bf16_t* __restrict__ dout,
                                            int64_t ldd, const float* __restrict__ lse,
                                            const float* __restrict__ delta, bf16_t* __restrict__ dk,
                                            bf16_t* __restrict__ dv, int64_t lddkv, float scale,
                                            const uint32_t* __restrict__ mask, float dscale,
                                            const int32_t* __restrict__ seg_end = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = (int)T_, b = bh / H, hh = bh % H;
    const int K0 = kblk * 128, kq = K0 + 32 * wave;
    const bool act = kq < T;
    const int64_t boff = (int64_t)b * T_, ntile = mask_tiles(T_);
    const float c2 = scale * LOG2E;
    const int key = kq + (lane & 31);
    sv8 kf[4], vf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        kf[ks] = act ? ld_frag(k + boff * ld + hh * 64, ld, key, ks, lane) : sv8{};
        vf[ks] = act ? ld_frag(v + boff * ld + hh * 64, ld, key, ks, lane) : sv8{};
    }
    int se = 0;
    if constexpr (SEG) {
        if (act) se = seg_hi((uint32_t)seg_end[boff + key], key);
    }
    fv16 dka[2] = {fv16{}, fv16{}}, dva[2] = {fv16{}, fv16{}};
    const bf16_t* qb_ = q + boff * ld + hh * 64;
    const bf16_t* ob_ = dout + boff * ldd + hh * 64;
    const float* lse_b = lse + (int64_t)bh * T_;
    const float* del_b = delta + (int64_t)bh * T_;
    const int nq = T / 64, qt0 = K0 / 64;
    // keep words: BWD tiles (key block kq/32, query tile qt >= kq/64), prefetched one tile ahead
    const int kbw = kq >> 5, qtm = kbw >> 1;
    const uint32_t* mcol =
        DROP && act ? mask + ((int64_t)bh * ntile + mask_bwd_tile(kbw, qtm, nq)) * 64 + lane : nullptr;
    uint32_t mw = (DROP && act && qt0 >= qtm) ? mcol[(qt0 - qtm) * 64] : 0u;
    auto stat_load = [&](int qt) {
        float s = 0.f;
        if (tid < 64) s = lse_b[qt * 64 + tid] * LOG2E;
        else if (tid < 128) s = -del_b[qt * 64 + tid - 64] / dscale;   // -delta' = -(1-p) delta
        return s;
    };
    const int wave_ = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Q/dO ring of NS slots (images + row statistics), tile qt + AH requested at the head of tile qt
    // into the slot of tile qt + AH - NS (read before an earlier barrier); NS = 4: two tiles of
    // compute to land.  A slot's statistics are written from hidden loads issued with its DMA.
    constexpr int AH = NS / 2;
    auto slot = [&](int it_) { return smem + (it_ & (NS - 1)) * KV_STAGE; };
    const uint32_t l0 = lds_base(smem);
    auto lslot = [&](int it_) { return l0 + (uint32_t)((it_ & (NS - 1)) * KV_STAGE); };
    {
        const float s0 = stat_load(qt0);
        const float s1 = (AH == 2 && qt0 + 1 < nq) ? stat_load(qt0 + 1) : 0.f;
#pragma unroll
        for (int t = 0; t < AH; ++t) {
            if (qt0 + t < nq) {
                dma_tile(qb_, ld, (int64_t)(qt0 + t) * 64, lslot(t), wave_, lane);
                dma_tile(ob_, ldd, (int64_t)(qt0 + t) * 64, lslot(t) + TILE, wave_, lane);
                if (tid < 128) ((float*)(slot(t) + 2 * TILE))[tid] = t ? s1 : s0;
            }
        }
    }
    ring_wait<AH == 2 ? 4 : 0>(AH == 2 && qt0 + 1 < nq);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) mark_ready(kf[ks], vf[ks]);
    mark_ready(mw);
    if constexpr (SEG) mark_ready(se);
    for (int qt = qt0; qt < nq; ++qt) {
        const int it = qt - qt0;
        const int nxt = qt + 1 < nq ? qt + 1 : qt;
        const bool pf = qt + AH < nq;
        // tile qt + AH's row statistics and tile qt + 1's keep word by hidden loads issued before the
        // DMAs, so the counted wait at the tile's end retires them (compiler-counted loads issued
        // after the DMAs made hipcc wait vmcnt(0) -- for the DMAs too -- inside this tile's products)
        uint32_t sw = 0u, mn = 0u;
        if (pf) {
            if (tid < 64) gload4(sw, lse_b + (qt + AH) * 64 + tid);
            else if (tid < 128) gload4(sw, del_b + (qt + AH) * 64 + tid - 64);
        }
        if (DROP && act && nxt >= qtm) gload4(mn, mcol + (nxt - qtm) * 64);
        if (pf) {
            dma_tile(qb_, ld, (int64_t)(qt + AH) * 64, lslot(it + AH), wave_, lane);
            dma_tile(ob_, ldd, (int64_t)(qt + AH) * 64, lslot(it + AH) + TILE, wave_, lane);
        }
        const char* S0 = slot(it);
        const char* Qi = S0;
        const char* Oi = S0 + TILE;
        const float* st_lse = (const float*)(S0 + 2 * TILE);
        const float* st_del = st_lse + 64;
        const int q0 = qt * 64;
        if (act && q0 + 63 >= kq)
            dkdv_tile<DROP, SEG>(Qi, Oi, st_lse, st_del, q0, kq, key, kf, vf, mw, c2, dka, dva, lane, se);
        // tile qt + 1, the statistics and the keep word have landed (tile qt + AH's DMAs may not)
        if (AH == 2 && pf) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" : "+v"(sw), "+v"(mn));
        if (pf) {   // stat_load's arithmetic on the loaded word
            char* D = slot(it + AH);
            if (tid < 64) ((float*)(D + 2 * TILE))[tid] = __uint_as_float(sw) * LOG2E;
            else if (tid < 128) ((float*)(D + 2 * TILE))[tid] = -__uint_as_float(sw) / dscale;
        }
        mw = mn;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (!act) return;
    store_rows(dk + (boff + key) * lddkv + hh * 64, dka, scale * dscale, lane);
    store_rows(dv + (boff + key) * lddkv + hh * 64, dva, DROP ? dscale : 1.f, lane);
}

// pairs of 128-key blocks per workgroup (x, then nk - 1 - x): uniform causal work per workgroup
template <bool DROP, int NS>
__global__ __launch_bounds__(256, 2) void k_attn_dkdv_d64(int64_t T_, int H, const bf16_t* __restrict__ q,
                                                          const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                          int64_t ld, const bf16_t* __restrict__ dout, int64_t ldd,
                                                          const float* __restrict__ lse,
                                                          const float* __restrict__ delta, bf16_t* __restrict__ dk,
                                                          bf16_t* __restrict__ dv, int64_t lddkv, float scale,
                                                          const uint32_t* __restrict__ mask, float dscale) {
    __shared__ __attribute__((aligned(16))) char smem[NS * KV_STAGE];
    int x, bh;
    block_coords<false>(x, bh);
    const int nk = (int)((T_ + 127) / 128), second = nk - 1 - x;
    const int npass = x == second ? 1 : 2;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
        if (pass) __syncthreads();
        dkdv_kblock<DROP, NS>(pass ? second : x, bh, smem, T_, H, q, k, v, ld, dout, ldd, lse, delta, dk, dv, lddkv, scale,
                          mask, dscale);
    }
}

template <bool DROP, int NS>
__global__ __launch_bounds__(256, 2) void k_attn_dkdv_d64_seg(int64_t T_, int H, const bf16_t* __restrict__ q,
                                                              const bf16_t* __restrict__ k,
                                                              const bf16_t* __restrict__ v, int64_t ld,
                                                              const bf16_t* __restrict__ dout, int64_t ldd,
                                                              const float* __restrict__ lse,
                                                              const float* __restrict__ delta, bf16_t* __restrict__ dk,
                                                              bf16_t* __restrict__ dv, int64_t lddkv, float scale,
                                                              const uint32_t* __restrict__ mask, float dscale,
                                                              const int32_t* __restrict__ seg_end) {
    __shared__ __attribute__((aligned(16))) char smem[NS * KV_STAGE];
    int x, bh;
    block_coords<false>(x, bh);
    const int nk = (int)((T_ + 127) / 128), second = nk - 1 - x;
    const int npass = x == second ? 1 : 2;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
        if (pass) __syncthreads();
        dkdv_kblock<DROP, NS, true>(pass ? second : x, bh, smem, T_, H, q, k, v, ld, dout, ldd, lse, delta, dk, dv, lddkv,
                                    scale, mask, dscale, seg_end);
    }
}

// =====================================================================================
// Forward at T > 256 with an LDS-DMA K/V ring.  Same two-group software pipeline and per-tile
// arithmetic as fwd_qblock (identical bits), but K/V tiles arrive by LDS-DMA requested at the head
// of a tile (no staging VGPRs or ds_writes in the loop), so a tile has a whole tile of compute (QR:
// two) to land instead of the half tile the register staging gave it.  The keep words of tile kv + 1
// are hidden register loads issued just before the DMA, retired by the same counted wait.
//   QR = false: Q image in LDS (32 KB) + 3-slot ring (48 KB), tile kv + 1 requested at tile kv into
//               the slot tile kv - 2 used (B read V(kv - 2) during tile kv - 1);
//   QR = true:  the groups' Q fragments in registers (hidden loads) + 4-slot ring (64 KB), tile kv + 2
//               requested at tile kv.
// Both fit two blocks per CU.
// =====================================================================================
template <bool QR>
struct FwdRing {
    static constexpr int NSLOT = QR ? 4 : 3, AHEAD = QR ? 2 : 1;
    static constexpr int LDS = NSLOT * 2 * TILE + (QR ? 0 : 4 * TILE);
    static __device__ __forceinline__ int slot_of(int t) { return QR ? (t & 3) : (t + 3) % 3; }
};

// dma_tile with a uniform tile base and the per-lane byte offsets precomputed (dma_lane_offs): the
// same 8 wave-instructions, 2 per wave
__device__ __forceinline__ void dma_lane_offs(int64_t ldx, int wave, int lane, uint32_t (&off)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ins = 2 * wave + i, r = 8 * ins + (lane >> 3), c = (lane & 7) ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3));
        off[i] = (uint32_t)((r * ldx + 8 * c) * 2);
    }
}
// img as a 32-bit LDS byte address (lds_base of the kernel's __shared__ array + an integer offset):
// casting a generic slot pointer back to LDS per call made hipcc emit a null-pointer select -- and,
// once the forward ring kernel ran out of SGPRs, an illegal v_cmp on src_shared_base for it
__device__ __forceinline__ void dma_tile_s(const bf16_t* X, int64_t ldx, int64_t row0, const uint32_t (&off)[2],
                                           uint32_t img, int wave) {
    const bf16_t* base = X + row0 * ldx;
#pragma unroll
    for (int i = 0; i < 2; ++i) dma16sl(base, off[i], img + 1024 * (2 * wave + i));
}

__device__ __forceinline__ void qk_tile_reg(fv16 (&s)[2], const char* Ki, const sv8 (&qf)[4], int lane) {
    s[0] = fv16{};
    s[1] = fv16{};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        s[0] = mfma32(frag_row(Ki, 0, ks, lane), qf[ks], s[0]);
        s[1] = mfma32(frag_row(Ki, 32, ks, lane), qf[ks], s[1]);
    }
}

// SEG (packed rows, QR only): the lanes' segment bounds come in with the Q fragments; every tile goes
// through fwd_group_tile (no two-group pipeline: the same per-group arithmetic in the same order, so
// an all-zero seg_start gives the pipelined kernel's bits), tiles before every lane's segment skipped
template <bool DROP, bool QR, bool SEG = false>
__device__ __forceinline__ void fwd_qblock_dma(int qblk, int bh, char* smem, int64_t T_, int H,
                                               const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                               const bf16_t* __restrict__ v, int64_t ld, bf16_t* __restrict__ o,
                                               int64_t ldo, float* __restrict__ lse, float scale_log2,
                                               const uint32_t* __restrict__ mask, float dscale,
                                               const int32_t* __restrict__ seg_start = nullptr,
                                               const int32_t* __restrict__ seg_end = nullptr) {
    static_assert(QR || !SEG, "the segment mask is built for the register-Q form");
    using R = FwdRing<QR>;
    constexpr int AH = R::AHEAD;
    // tile kv + AH is requested at tile kv: 4 DMA instructions per wave stay in flight at its end
    // when AH = 2 (tile kv + 1 must have landed), none when AH = 1
    constexpr int NWAIT = AH == 2 ? 4 : 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = (int)T_, b = bh / H, hh = bh % H;
    const int Q0 = qblk * 256;
    const int64_t boff = (int64_t)b * T_, ntile = mask_tiles(T_);
    const bf16_t* kb_ = k + boff * ld + hh * 64;
    const bf16_t* vb_ = v + boff * ld + hh * 64;
    const bf16_t* qb_ = q + boff * ld + hh * 64;
    char* const Qimg = smem + R::NSLOT * 2 * TILE;   // !QR only
    const int qg[2] = {Q0 + 32 * (7 - wave), Q0 + 32 * wave};   // g = 0 (A): the longer causal prefix
    const int qr[2] = {32 * (7 - wave), 32 * wave};             // the groups' rows in the Q image
    const bool act[2] = {qg[0] < T, qg[1] < T};
    uint32_t doff[2];   // per-lane DMA byte offsets (K, V and Q share ld and the image layout)
    dma_lane_offs(ld, wave, lane, doff);
    auto slot = [&](int t) { return smem + R::slot_of(t) * 2 * TILE; };
    const uint32_t lds0 = lds_base(smem);
    auto lslot = [&](int t) { return lds0 + (uint32_t)(R::slot_of(t) * 2 * TILE); };
    // keep words of (group, key tile t) at mrow[g] + 64 t + lane (uniform bases, one lane offset); an
    // inactive group reads block 0's (unused)
    const uint32_t* mrow[2];
    const uint32_t loff = 4u * lane;
    sv8 qf[2][4];
    uint32_t mw[2] = {0u, 0u}, ssw[2] = {0u, 0u}, sew[2] = {0u, 0u};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        mrow[g] = mask + ((int64_t)bh * ntile + mask_fwd_tile(act[g] ? qg[g] >> 5 : 0, 0)) * 64;
        if constexpr (QR) {
            const int qa = (act[g] ? qg[g] : 0) + (lane & 31);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) gload16(qf[g][ks], qb_ + (int64_t)qa * ld + 16 * ks + 8 * (lane >> 5));
            if constexpr (SEG) {
                gload4(ssw[g], seg_start + boff + qa);
                gload4(sew[g], seg_end + boff + qa);
            }
        }
        if constexpr (DROP) gload4s(mw[g], mrow[g], loff);
    }
    const int qlast = (Q0 + 255 < T - 1) ? Q0 + 255 : T - 1;
    const int nkv = qlast / 64 + 1;
    const int npipe = SEG ? 0 : (act[1] ? (qg[1] + 31) / 64 : 0);   // B's diagonal tile: first unpipelined tile
    {   // the V half of tile -1's slot is the pipeline head's "previous tile": zeros
        const int r = tid >> 3, c = tid & 7;
        *(uint4*)(slot(-1) + TILE + aoff(r, c)) = make_uint4(0, 0, 0, 0);
        *(uint4*)(slot(-1) + TILE + aoff(r + 32, c)) = make_uint4(0, 0, 0, 0);
    }
    if constexpr (!QR) {   // Q image: the block's 64-row tiles by LDS-DMA, rows past T zero
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (Q0 + 64 * t < T) {
                dma_tile_s(qb_, ld, Q0 + 64 * t, doff, lds0 + (uint32_t)(R::NSLOT * 2 * TILE + t * TILE), wave);
            } else {
                const int r = tid >> 3, c = tid & 7;
                *(uint4*)(Qimg + t * TILE + aoff(r, c)) = make_uint4(0, 0, 0, 0);
                *(uint4*)(Qimg + t * TILE + aoff(r + 32, c)) = make_uint4(0, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < AH; ++t) {
        if (t < nkv) {
            dma_tile_s(kb_, ld, (int64_t)t * 64, doff, lslot(t), wave);
            dma_tile_s(vb_, ld, (int64_t)t * 64, doff, lslot(t) + TILE, wave);
        }
    }
    ring_wait<NWAIT>(AH == 2 && nkv > 1);   // the register loads, Q and tile 0 have landed
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if constexpr (QR) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(qf[g][ks]));
        }
        asm volatile("" : "+v"(mw[g]));
        if constexpr (SEG) asm volatile("" : "+v"(ssw[g]), "+v"(sew[g]));
    }
    if constexpr (!DROP) mw[0] = mw[1] = 0u;
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
    auto qk = [&](fv16 (&s)[2], const char* Ki, int g) {
        if constexpr (QR) qk_tile_reg(s, Ki, qf[g], lane);
        else qk_tile(s, Ki, Qimg, qr[g], lane);
    };
    fv16 oacc[2][2];
#pragma unroll
    for (int g = 0; g < 2; ++g) oacc[g][0] = oacc[g][1] = fv16{};
    float m_run[2] = {-FLT_MAX, -FLT_MAX};
    fv4 l_run[2] = {fv4{}, fv4{}};
    const sv8 ones = rowsum_ones(lane);
    fv16 sA[2], sB[2] = {fv16{} - INFINITY, fv16{} - INFINITY};
    sv8 pfA[2][2], pfB[2][2];
    uint32_t mwBp = 0u;   // B's keep word of the previous tile
    int kv = 0;
    for (; kv < npipe; ++kv) {
        uint32_t mn[2] = {0u, 0u};   // tile kv + 1 <= npipe: both groups full through it
        if constexpr (DROP) {
            gload4s(mn[0], mrow[0] + (kv + 1) * 64, loff);
            gload4s(mn[1], mrow[1] + (kv + 1) * 64, loff);
        }
        const bool pf = kv + AH < nkv;
        if (pf) {
            dma_tile_s(kb_, ld, (int64_t)(kv + AH) * 64, doff, lslot(kv + AH), wave);
            dma_tile_s(vb_, ld, (int64_t)(kv + AH) * 64, doff, lslot(kv + AH) + TILE, wave);
        }
        const char* Ki = slot(kv);
        const char* Vi = Ki + TILE;
        const char* Vp = slot(kv - 1) + TILE;
        // at kv = 0, B's "previous tile" is sB = -inf against the zeroed V slot: it adds exactly 0
        qk(sA, Ki, 0);
        softmax_pack<DROP>(sB, scale_log2, m_run[1], l_run[1], mwBp, pfB, ones);
        pv_tile(oacc[1], Vp, pfB, lane);
        rescale_if(tile_max(sA) * scale_log2, m_run[0], l_run[0], oacc[0]);
        qk(sB, Ki, 1);
        softmax_pack<DROP>(sA, scale_log2, m_run[0], l_run[0], mw[0], pfA, ones);
        pv_tile(oacc[0], Vi, pfA, lane);
        rescale_if(tile_max(sB) * scale_log2, m_run[1], l_run[1], oacc[1]);
        ring_wait<NWAIT>(pf);
        if constexpr (DROP) asm volatile("" : "+v"(mn[0]), "+v"(mn[1]));
        mwBp = mw[1];
        mw[0] = mn[0];
        mw[1] = mn[1];
    }
    if (npipe > 0) {   // pipeline tail: B's pending tile npipe - 1 (its V still in that tile's slot)
        softmax_pack<DROP>(sB, scale_log2, m_run[1], l_run[1], mwBp, pfB, ones);
        pv_tile(oacc[1], slot(npipe - 1) + TILE, pfB, lane);   // the tail requests kv + AH: another slot
    }
    for (; kv < nkv; ++kv) {
        uint32_t mn[2] = {0u, 0u};
        const int nxt = kv + 1 < nkv ? kv + 1 : kv;
        if constexpr (DROP) {
#pragma unroll
            for (int g = 0; g < 2; ++g)   // past a group's diagonal: re-read its tile 0 (unused)
                gload4s(mn[g], mrow[g] + (act[g] && nxt * 64 <= qg[g] + 31 ? nxt : 0) * 64, loff);
        }
        const bool pf = kv + AH < nkv;
        if (pf) {
            dma_tile_s(kb_, ld, (int64_t)(kv + AH) * 64, doff, lslot(kv + AH), wave);
            dma_tile_s(vb_, ld, (int64_t)(kv + AH) * 64, doff, lslot(kv + AH) + TILE, wave);
        }
        const char* Ki = slot(kv);
        const char* Vi = Ki + TILE;
        const int k0 = kv * 64;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (!act[g] || k0 > qg[g] + 31) continue;
            const int rel = __builtin_amdgcn_readfirstlane(qg[g] - k0);
            if constexpr (QR) {
                const int srel = SEG ? ss[g] - k0 : 0;
                if constexpr (SEG) {
                    if (__all(srel >= 64)) continue;   // the tile precedes every lane's segment
                }
                if (rel >= 64)
                    fwd_group_tile<DROP, 2, -1, true, SEG>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g],
                                                           oacc[g], mw[g], ones, qf[g], srel, peers[g]);
                else if (rel == 32)
                    fwd_group_tile<DROP, 2, 1, true, SEG>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g],
                                                          oacc[g], mw[g], ones, qf[g], srel, peers[g]);
                else
                    fwd_group_tile<DROP, 1, 0, true, SEG>(Ki, Vi, nullptr, 0, lane, scale_log2, m_run[g], l_run[g],
                                                          oacc[g], mw[g], ones, qf[g], srel, peers[g]);
            } else {
                if (rel >= 64)
                    fwd_group_tile<DROP, 2, -1>(Ki, Vi, Qimg, qr[g], lane, scale_log2, m_run[g], l_run[g], oacc[g],
                                                mw[g], ones);
                else if (rel == 32)
                    fwd_group_tile<DROP, 2, 1>(Ki, Vi, Qimg, qr[g], lane, scale_log2, m_run[g], l_run[g], oacc[g],
                                               mw[g], ones);
                else
                    fwd_group_tile<DROP, 1, 0>(Ki, Vi, Qimg, qr[g], lane, scale_log2, m_run[g], l_run[g], oacc[g],
                                               mw[g], ones);
            }
        }
        ring_wait<NWAIT>(pf);
        if constexpr (DROP) asm volatile("" : "+v"(mn[0]), "+v"(mn[1]));
        mw[0] = mn[0];
        mw[1] = mn[1];
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (!act[g]) continue;
        const float lt = l_run[g][0];   // every accumulator register holds query lane & 31's sum
        const int64_t qa = qg[g] + (lane & 31);
        store_rows_wide(o + (boff + qa) * ldo + hh * 64, oacc[g], dscale / lt, lane);
        if (lane < 32) lse[(int64_t)bh * T_ + qa] = (m_run[g] + __log2f(lt)) * LN2;
    }
}

template <bool DROP, bool QR>
__global__ __launch_bounds__(256, 2) void k_attn_fwd_d64d(int64_t T_, int H, const bf16_t* __restrict__ q,
                                                          const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                          int64_t ld, bf16_t* __restrict__ o, int64_t ldo,
                                                          float* __restrict__ lse, float scale_log2,
                                                          const uint32_t* __restrict__ mask, float dscale) {
    __shared__ __attribute__((aligned(16))) char smem[FwdRing<QR>::LDS];
    int x, bh;
    block_coords<false>(x, bh);
    const int nq = (int)((T_ + 255) / 256), first = nq - 1 - x;
    const int npass = x == first ? 1 : 2;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
        if (pass) __syncthreads();
        fwd_qblock_dma<DROP, QR>(pass ? x : first, bh, smem, T_, H, q, k, v, ld, o, ldo, lse, scale_log2, mask,
                                 dscale);
    }
}

template <bool DROP>
__global__ __launch_bounds__(256, 2) void k_attn_fwd_d64d_seg(int64_t T_, int H, const bf16_t* __restrict__ q,
                                                              const bf16_t* __restrict__ k,
                                                              const bf16_t* __restrict__ v, int64_t ld,
                                                              bf16_t* __restrict__ o, int64_t ldo,
                                                              float* __restrict__ lse, float scale_log2,
                                                              const uint32_t* __restrict__ mask, float dscale,
                                                              const int32_t* __restrict__ seg_start,
                                                              const int32_t* __restrict__ seg_end) {
    __shared__ __attribute__((aligned(16))) char smem[FwdRing<true>::LDS];
    int x, bh;
    block_coords<false>(x, bh);
    const int nq = (int)((T_ + 255) / 256), first = nq - 1 - x;
    const int npass = x == first ? 1 : 2;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
        if (pass) __syncthreads();
        fwd_qblock_dma<DROP, true, true>(pass ? x : first, bh, smem, T_, H, q, k, v, ld, o, ldo, lse, scale_log2, mask,
                                         dscale, seg_start, seg_end);
    }
}

}  // namespace

#ifdef CG_AB_VARIANTS
namespace attn_ab {
// ab/attention_ab.hip: the measured-slower attention variants, selected by cg_set_tuning("attn_variant");
// each returns false when the variant does not apply (the product kernel then runs)
bool launch_fwd(int variant, dim3 grid, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v,
                int64_t ld, bf16_t* o, int64_t ldo, float* lse, float scale, const DropArgs& d, hipStream_t st);
bool launch_dq(int variant, dim3 grid, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v,
               int64_t ld, const bf16_t* o, int64_t ldo, const bf16_t* dout, int64_t ldd, const float* lse,
               float* delta, bf16_t* dq, int64_t lddq, float scale, const DropArgs& d, hipStream_t st);
bool launch_dkdv(int variant, dim3 grid, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v,
                 int64_t ld, const bf16_t* dout, int64_t ldd, const float* lse, const float* delta, bf16_t* dk,
                 bf16_t* dv, int64_t lddkv, float scale, const DropArgs& d, hipStream_t st);
}  // namespace attn_ab
#endif

}  // namespace cg
