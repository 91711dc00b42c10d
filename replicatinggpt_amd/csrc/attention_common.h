// charpt attention internals shared by attention.hip (the C ABI and the dispatch) and the kernel
// families it launches, each through the host launchers declared here: attention_dropmask.hip (keep
// bits), attention_f32.hip (fp32 MFMA forward), attention_generic.hip (fp32-math VALU kernels) and
// attention_d64.hip (bf16 MFMA kernels for head_size 64).
#pragma once
#include <type_traits>

#include "common.h"

namespace cg {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

struct DropArgs {
    uint32_t thr;
    float dscale;
    uint64_t seed;
    const uint64_t* rng_call;
    int site;
    const uint32_t* mask;      // fast kernels: precomputed keep bits, FWD tiles; NULL = no dropout
    const uint32_t* mask_bwd;  // the same bits, BWD tiles (mask + B*H*mask_tiles(T)*64)
};

// Keep-bit image of the MFMA kernels, generated once per forward (k_attn_dropmask) from the
// canonical Philox stream (same bits as keep_of on element ((b*H + h)*T + q)*T + k) and read by the
// forward, dQ and dK/dV kernels with one coalesced 32-bit load per lane per 64-row tile, prefetched
// a tile ahead (a VGPR: no scalar-load latency in the inner loop, one v_bfe_i32 + v_and per use).
// T % 64 == 0; NB = T/32 blocks of 32, NP = T/64 tiles of 64.  Accumulator register r of 32x32
// sub-block s (32x32x16 MFMA layout: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
// =: row(r, l)) is bit f(s, r) = 8 s + (r >> 1) + 16 (r & 1) of a FWD word -- the two registers the
// forward packs into one bf16 pair at bits j and j + 16, so one shift + v_perm_b32 makes the pair's
// mask -- and bit 16 s + r of a BWD word:
//   FWD (forward, dQ: swapped products, lane = query), tile (qb, kt) for kt <= qb/2:
//        bit f(s, r) of lane l = keep(q = 32 qb + (l & 31), k = 64 kt + 32 s + row(r, l))
//   BWD (dK/dV: lane = key), tile (kb, qt) for qt >= kb/2:
//        bit 16 s + r of lane l = keep(q = 64 qt + 32 s + row(r, l), k = 32 kb + (l & 31))
// Sub-blocks wholly above the diagonal are 0; diagonal sub-blocks are stored whole (the kernels
// apply the causal mask themselves).  Per (b*H + h): mask_tiles(T) tiles of 64 words each, FWD
// row-major over qb, BWD column-major over kb.
__host__ __device__ __forceinline__ int64_t mask_tiles(int64_t T) {
    const int64_t nb = T / 32;
    return nb + (nb - 1) * (nb - 1) / 4;
}
__device__ __forceinline__ int64_t mask_fwd_tile(int qb, int kt) { return qb + (qb ? (qb - 1) * (qb - 1) / 4 : 0) + kt; }
__device__ __forceinline__ int64_t mask_bwd_tile(int kb, int qt, int np) {
    return (int64_t)kb * np - (kb ? (kb - 1) * (kb - 1) / 4 : 0) + qt - kb / 2;
}
// all-ones where bit `bit` of a lane's mask word is set (one v_bfe_i32)
__device__ __forceinline__ uint32_t keep_lanes(uint32_t w, int bit) { return (uint32_t)((int32_t)(w << (31 - bit)) >> 31); }

// f(std::bool_constant<flag>): a run-time flag as a kernel's compile-time template argument
template <typename F>
inline void with_flag(bool flag, F&& f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}
// DROP of the bf16 MFMA kernels.  Without dropout make_drop leaves d.mask = d.mask_bwd = nullptr and
// d.dscale = 1.f, so the launch sites pass them unconditionally.
template <typename F>
inline void with_drop(const DropArgs& d, F&& f) {
    with_flag(d.mask != nullptr, f);
}

namespace attn {
// keep bits (attention_dropmask.hip).  make_drop: the arguments of dropout probability p, no keep-bit
// image yet (mask = mask_bwd = nullptr); mask_bytes: the image's size, FWD and BWD tiles;
// launch_dropmask: generate it into `mask`; set_masks: point d at a generated image
DropArgs make_drop(double p, uint64_t seed, const uint64_t* rng_call, int site);
int64_t mask_bytes(int64_t B, int64_t H, int64_t T);
void set_masks(DropArgs& d, const uint64_t* mask, int64_t B, int64_t H, int64_t T);
void launch_dropmask(int64_t B, int64_t H, int64_t T, uint64_t* mask, const DropArgs& d, hipStream_t st);

// fp32 MFMA forward, D <= 32, no dropout (attention_f32.hip): sequence-resident at T <= 256
void launch_fwd_f32(int64_t B, int64_t T, int H, int D, const float* q, const float* k, const float* v, int64_t ld,
                    float* o, int64_t ldo, float* lse, float scale, hipStream_t st);

// the same on packed rows (seg_start int32 [B][T]): the 64-query-block kernel, launch_fwd_f32's bits for
// an all-zero seg_start
void launch_fwd_f32_seg(int64_t B, int64_t T, int H, int D, const float* q, const float* k, const float* v, int64_t ld,
                        float* o, int64_t ldo, float* lse, float scale, const int32_t* seg_start, hipStream_t st);

// fp32-math VALU kernels, any D <= 128 and any T, dtype CG_BF16 or CG_F32 (attention_generic.hip); the
// backward computes delta = rowsum(dO * O) into `delta` first.  seg_start / seg_end (int32 [B][T], both
// or neither): the packed-row mask, query i sees key j iff seg_start[b, i] <= j <= i
void launch_fwd_generic(int dtype, int64_t B, int64_t T_, int H, int D, const void* q, const void* k, const void* v,
                        int64_t ld, void* o, int64_t ldo, float* lse, float scale, const DropArgs& d, hipStream_t st,
                        const int32_t* seg_start = nullptr);
void launch_bwd_generic(int dtype, int64_t B, int64_t T_, int H, int D, const void* q, const void* k, const void* v,
                        int64_t ld, const void* o, int64_t ldo, const void* dout, int64_t ldd, const float* lse,
                        float* delta, void* dq, void* dk, void* dv, int64_t lddqkv, float scale, const DropArgs& d,
                        hipStream_t st, const int32_t* seg_start = nullptr, const int32_t* seg_end = nullptr);

// bf16 MFMA kernels, head_size 64, T % 64 == 0 (attention_d64.hip)
void launch_fwd_d64(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                    bf16_t* o, int64_t ldo, float* lse, float scale, const DropArgs& d, hipStream_t st);
// dQ then dK/dV (T <= 256: one merged launch, bwd_merged(T)); delta_ready (merged launch only):
// `delta` already holds rowsum(dO * O) and is read, not computed
bool bwd_merged(int64_t T);
void launch_bwd_d64(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                    const bf16_t* o, int64_t ldo, const bf16_t* dout, int64_t ldd, const float* lse, float* delta,
                    bool delta_ready, bf16_t* dq, int64_t lddq, bf16_t* dk, bf16_t* dv, int64_t lddkv, float scale, const DropArgs& d,
                    hipStream_t st);
// packed rows (seg_start / seg_end int32 [B][T]): the sequence-resident kernels at T <= 256
// (seg_resident: the backward is the merged launch, delta_ready as launch_bwd_d64), the ring kernels
// beyond (delta is computed into `delta`; delta_ready must be false)
bool seg_resident(int64_t T);
void launch_fwd_d64_seg(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                        bf16_t* o, int64_t ldo, float* lse, float scale, const DropArgs& d, const int32_t* seg_start,
                        const int32_t* seg_end, hipStream_t st);
void launch_bwd_d64_seg(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                        const bf16_t* o, int64_t ldo, const bf16_t* dout, int64_t ldd, const float* lse, float* delta,
                        bool delta_ready, bf16_t* dq, int64_t lddq, bf16_t* dk, bf16_t* dv, int64_t lddkv, float scale,
                        const DropArgs& d, const int32_t* seg_start, const int32_t* seg_end, hipStream_t st);
}  // namespace attn
// cg_set_tuning knobs (attention_d64.hip)
extern int g_attn_variant;
extern int g_attn_bwd_lpt;

}  // namespace cg
