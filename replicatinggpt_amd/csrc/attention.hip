// charpt: the attention C ABI and its dispatch among the kernel families (attention_common.h):
// the bf16 MFMA kernels for head_size 64 (attention_d64.hip), the fp32 MFMA forward for small heads
// (attention_f32.hip) and the generic kernels (attention_generic.hip); the keep bits of the MFMA
// path come from attention_dropmask.hip.  Head.forward x n_head, GPT1.py:109-123,134-135.
#include "attention_common.h"

using namespace cg;

namespace {

// (every pointer the MFMA kernels read or write in 16-B segments: q, k, v each on their own, since the
// ABI takes them as three pointers)
bool fast_attn_ok(int dtype, int64_t T, int64_t D, const void* a, const void* b, const void* c, const void* e,
                  int64_t ld1, int64_t ld2) {
    return dtype == CG_BF16 && D == 64 && T % 64 == 0 &&
           (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)e) & 15) == 0 && ld1 % 8 == 0 && ld2 % 8 == 0;
}

// the backward workspace: delta = rowsum(dO * O) rounded up to 256 B, then a keep-bit image
int64_t delta_bytes(int64_t B, int64_t T, int64_t H) { return (B * H * T * (int64_t)sizeof(float) + 255) / 256 * 256; }

int attn_fwd_impl(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k, const void* v,
                  int64_t ld_qkv, void* o, int64_t ld_o, float* lse, float scale, double dropout_p, uint64_t seed,
                  const uint64_t* rng_call, int site, uint64_t* mask, bool mask_ready, void* stream,
                  const int32_t* seg_start = nullptr, const int32_t* seg_end = nullptr) {
    CG_REQUIRE(B > 0 && T > 0 && H > 0 && D > 0 && D <= 128, "cg_attn_fwd: bad shape (D must be <= 128)");
    CG_REQUIRE(dropout_p >= 0 && dropout_p < 1, "cg_attn_fwd: dropout_p must be in [0,1)");
    hipStream_t st = (hipStream_t)stream;
    DropArgs d = attn::make_drop(dropout_p, seed, rng_call, site);
    const bool seg = seg_start != nullptr;
    if (fast_attn_ok(dtype, T, D, q, k, v, o, ld_qkv, ld_o)) {
        if (d.thr) {
            CG_REQUIRE(mask, "cg_attn_fwd: dropout on the MFMA path needs a mask buffer (cg_attn_mask_bytes)");
            if (!mask_ready) attn::launch_dropmask(B, H, T, mask, d, st);
            attn::set_masks(d, mask, B, H, T);
        }
        if (seg)
            attn::launch_fwd_d64_seg(B, T, (int)H, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld_qkv,
                                     (bf16_t*)o, ld_o, lse, scale, d, seg_start, seg_end, st);
        else
            attn::launch_fwd_d64(B, T, (int)H, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ld_qkv,
                                 (bf16_t*)o, ld_o, lse, scale, d, st);
    } else if (dtype == CG_F32 && !d.thr && D <= 32) {
        if (seg)
            attn::launch_fwd_f32_seg(B, T, (int)H, (int)D, (const float*)q, (const float*)k, (const float*)v, ld_qkv,
                                     (float*)o, ld_o, lse, scale, seg_start, st);
        else
            attn::launch_fwd_f32(B, T, (int)H, (int)D, (const float*)q, (const float*)k, (const float*)v, ld_qkv,
                                 (float*)o, ld_o, lse, scale, st);
    } else {
        attn::launch_fwd_generic(dtype, B, T, (int)H, (int)D, q, k, v, ld_qkv, o, ld_o, lse, scale, d, st, seg_start);
    }
    CG_LAUNCH_CHECK("cg_attn_fwd");
    return CG_OK;
}

// delta_in: rowsum(dO * O) precomputed (cg_attn_bwd_delta), read only by the merged resident kernel
int attn_bwd_impl(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                  const void* v, int64_t ld_qkv, const void* o, int64_t ld_o, const void* dout, int64_t ld_do,
                  const float* lse, const float* delta_in, void* dq, void* dk, void* dv, int64_t ld_dqkv, float scale,
                  double dropout_p, uint64_t seed, const uint64_t* rng_call, int site, const uint64_t* mask,
                  void* workspace, void* stream, const int32_t* seg_start = nullptr,
                  const int32_t* seg_end = nullptr) {
    CG_REQUIRE(B > 0 && T > 0 && H > 0 && D > 0 && D <= 128, "cg_attn_bwd: bad shape (D must be <= 128)");
    CG_REQUIRE(workspace, "cg_attn_bwd: workspace required");
    hipStream_t st = (hipStream_t)stream;
    DropArgs d = attn::make_drop(dropout_p, seed, rng_call, site);
    float* delta = (float*)workspace;
    const bool seg = seg_start != nullptr;
    const bool fast = fast_attn_ok(dtype, T, D, q, k, v, dout, ld_qkv, ld_do) && ld_dqkv % 8 == 0 &&
                      ((((uintptr_t)dq) | ((uintptr_t)dk) | ((uintptr_t)dv) | ((uintptr_t)o)) & 15) == 0 &&
                      ld_o % 8 == 0;
    if (fast) {
        // delta = rowsum(dO * O) is computed inside the dQ kernel (which runs before dK/dV)
        if (d.thr) {
            if (!mask) {  // regenerate the forward's keep bits (identical Philox stream)
                uint64_t* m = (uint64_t*)((char*)workspace + delta_bytes(B, T, H));
                attn::launch_dropmask(B, H, T, m, d, st);
                mask = m;
            }
            attn::set_masks(d, mask, B, H, T);
        }
        const bf16_t *Q = (const bf16_t*)q, *K = (const bf16_t*)k, *V = (const bf16_t*)v, *DO = (const bf16_t*)dout;
        const bool din = delta_in && (seg ? attn::seg_resident(T) : attn::bwd_merged(T));
        if (seg)
            attn::launch_bwd_d64_seg(B, T, (int)H, Q, K, V, ld_qkv, (const bf16_t*)o, ld_o, DO, ld_do, lse,
                                     din ? (float*)delta_in : delta, din, (bf16_t*)dq, ld_dqkv, (bf16_t*)dk,
                                     (bf16_t*)dv, ld_dqkv, scale, d, seg_start, seg_end, st);
        else
            attn::launch_bwd_d64(B, T, (int)H, Q, K, V, ld_qkv, (const bf16_t*)o, ld_o, DO, ld_do, lse,
                                 din ? (float*)delta_in : delta, din, (bf16_t*)dq, ld_dqkv, (bf16_t*)dk, (bf16_t*)dv,
                                 ld_dqkv, scale, d, st);
    } else {
        attn::launch_bwd_generic(dtype, B, T, (int)H, (int)D, q, k, v, ld_qkv, o, ld_o, dout, ld_do, lse, delta, dq, dk,
                                 dv, ld_dqkv, scale, d, st, seg_start, seg_end);
    }
    CG_LAUNCH_CHECK("cg_attn_bwd");
    return CG_OK;
}

// seg_end[b, t] = the first t' > t with seg_start[b, t'] != seg_start[b, t], else T: one thread per
// position walks to the end of its segment (a forward's one small launch, shared by every layer)
__global__ __launch_bounds__(256) void k_seg_bounds(const int32_t* __restrict__ seg_start, int32_t* __restrict__ seg_end,
                                                    int64_t rows, int64_t T) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * T) return;
    const int64_t r0 = i / T * T, t = i - r0;
    const int32_t s = seg_start[i];
    int64_t e = t + 1;
    while (e < T && seg_start[r0 + e] == s) ++e;
    seg_end[i] = (int32_t)e;
}

#define CG_REQUIRE_SEG(name)                                                                          \
    CG_REQUIRE(seg_start && seg_end, name ": seg_start and seg_end are required");                    \
    CG_REQUIRE(((((uintptr_t)seg_start) | ((uintptr_t)seg_end)) & 3) == 0, name ": seg_start / seg_end must be 4-byte aligned"); \
    CG_REQUIRE(T < ((int64_t)1 << 31), name ": T must fit int32")

}  // namespace

extern "C" int cg_seg_bounds(const int32_t* seg_start, int32_t* seg_end, int64_t B, int64_t T, void* stream) {
    CG_REQUIRE(B > 0 && T > 0 && T < ((int64_t)1 << 31), "cg_seg_bounds: bad shape");
    CG_REQUIRE(seg_start && seg_end, "cg_seg_bounds: seg_start and seg_end are required");
    k_seg_bounds<<<(unsigned)ceil_div(B * T, 256), 256, 0, (hipStream_t)stream>>>(seg_start, seg_end, B, T);
    CG_LAUNCH_CHECK("cg_seg_bounds");
    return CG_OK;
}

extern "C" int cg_attn_fwd_seg(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                               const void* v, int64_t ld_qkv, void* o, int64_t ld_o, float* lse, float scale,
                               double dropout_p, uint64_t seed, const uint64_t* rng_call, int site, uint64_t* mask,
                               const int32_t* seg_start, const int32_t* seg_end, void* stream) {
    CG_REQUIRE_SEG("cg_attn_fwd_seg");
    return attn_fwd_impl(dtype, B, T, H, D, q, k, v, ld_qkv, o, ld_o, lse, scale, dropout_p, seed, rng_call, site,
                         mask, false, stream, seg_start, seg_end);
}

extern "C" int cg_attn_fwd_seg_premasked(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q,
                                         const void* k, const void* v, int64_t ld_qkv, void* o, int64_t ld_o,
                                         float* lse, float scale, double dropout_p, uint64_t seed,
                                         const uint64_t* rng_call, int site, uint64_t* mask, const int32_t* seg_start,
                                         const int32_t* seg_end, void* stream) {
    CG_REQUIRE_SEG("cg_attn_fwd_seg_premasked");
    return attn_fwd_impl(dtype, B, T, H, D, q, k, v, ld_qkv, o, ld_o, lse, scale, dropout_p, seed, rng_call, site,
                         mask, true, stream, seg_start, seg_end);
}

extern "C" int cg_attn_bwd_seg(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                               const void* v, int64_t ld_qkv, const void* o, int64_t ld_o, const void* dout,
                               int64_t ld_do, const float* lse, const float* delta, void* dq, void* dk, void* dv,
                               int64_t ld_dqkv, float scale, double dropout_p, uint64_t seed, const uint64_t* rng_call,
                               int site, const uint64_t* mask, const int32_t* seg_start, const int32_t* seg_end,
                               void* workspace, void* stream) {
    CG_REQUIRE_SEG("cg_attn_bwd_seg");
    CG_REQUIRE(!delta || (((uintptr_t)delta) & 3) == 0, "cg_attn_bwd_seg: delta must be 4-byte aligned");
    return attn_bwd_impl(dtype, B, T, H, D, q, k, v, ld_qkv, o, ld_o, dout, ld_do, lse, delta, dq, dk, dv, ld_dqkv,
                         scale, dropout_p, seed, rng_call, site, mask, workspace, stream, seg_start, seg_end);
}

extern "C" int cg_attn_fwd(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                           const void* v, int64_t ld_qkv, void* o, int64_t ld_o, float* lse, float scale,
                           double dropout_p, uint64_t seed, const uint64_t* rng_call, int site, uint64_t* mask,
                           void* stream) {
    return attn_fwd_impl(dtype, B, T, H, D, q, k, v, ld_qkv, o, ld_o, lse, scale, dropout_p, seed, rng_call, site,
                         mask, false, stream);
}

extern "C" int cg_attn_fwd_premasked(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q,
                                     const void* k, const void* v, int64_t ld_qkv, void* o, int64_t ld_o, float* lse,
                                     float scale, double dropout_p, uint64_t seed, const uint64_t* rng_call, int site,
                                     uint64_t* mask, void* stream) {
    return attn_fwd_impl(dtype, B, T, H, D, q, k, v, ld_qkv, o, ld_o, lse, scale, dropout_p, seed, rng_call, site,
                         mask, true, stream);
}

extern "C" int64_t cg_attn_bwd_workspace(int64_t B, int64_t T, int64_t H, int64_t D) {
    (void)D;
    return delta_bytes(B, T, H) + attn::mask_bytes(B, H, T);
}

extern "C" int cg_attn_bwd(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                           const void* v, int64_t ld_qkv, const void* o, int64_t ld_o, const void* dout, int64_t ld_do,
                           const float* lse, void* dq, void* dk, void* dv, int64_t ld_dqkv, float scale,
                           double dropout_p, uint64_t seed, const uint64_t* rng_call, int site, const uint64_t* mask,
                           void* workspace, void* stream) {
    return attn_bwd_impl(dtype, B, T, H, D, q, k, v, ld_qkv, o, ld_o, dout, ld_do, lse, nullptr, dq, dk, dv, ld_dqkv,
                         scale, dropout_p, seed, rng_call, site, mask, workspace, stream);
}

extern "C" int cg_attn_bwd_delta(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                                 const void* v, int64_t ld_qkv, const void* o, int64_t ld_o, const void* dout,
                                 int64_t ld_do, const float* lse, const float* delta, void* dq, void* dk, void* dv,
                                 int64_t ld_dqkv, float scale, double dropout_p, uint64_t seed,
                                 const uint64_t* rng_call, int site, const uint64_t* mask, void* workspace,
                                 void* stream) {
    CG_REQUIRE(!delta || (((uintptr_t)delta) & 3) == 0, "cg_attn_bwd_delta: delta must be 4-byte aligned");
    return attn_bwd_impl(dtype, B, T, H, D, q, k, v, ld_qkv, o, ld_o, dout, ld_do, lse, delta, dq, dk, dv, ld_dqkv,
                         scale, dropout_p, seed, rng_call, site, mask, workspace, stream);
}
