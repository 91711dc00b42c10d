// charpt: cross entropy over the character vocabulary (F.cross_entropy, GPT1.py:189-192), with and
// without F.cross_entropy's ignore_index.
#include <math.h>

#include <type_traits>

#include "common.h"

using namespace cg;

// ---- cross entropy: one wave per row, V <= 64*16 ------------------------------------------
// MASKED (cg_ce_fwd_masked): targets and loss_rows are required, and a row whose target equals
// `ignore` gets a literal 0 row loss; the unmasked instantiation never reads `ignore`
template <bool MASKED>
__global__ __launch_bounds__(256) void k_ce_fwd(const float* __restrict__ logits, int64_t rows, int V, int64_t ld,
                                                const int64_t* __restrict__ targets, float* __restrict__ loss_rows,
                                                float* __restrict__ lse, int64_t ignore) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* x = logits + r * ld;
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, x[v]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(x[v] - mx);
    s = wave_sum(s);
    const float l = mx + logf(s);
    if (lane == 0) {
        lse[r] = l;
        if (MASKED || (targets && loss_rows)) {
            // F.cross_entropy raises on a target outside [0, V) that is not its ignore_index: the row
            // loss turns NaN instead, so a bad label cannot pass silently
            const int64_t t = targets[r];
            if (MASKED && t == ignore) loss_rows[r] = 0.f;
            else loss_rows[r] = (t < 0 || t >= V) ? __builtin_nanf("") : l - x[t];
        }
    }
}

extern "C" int cg_ce_fwd(const float* logits, int64_t rows, int64_t V, int64_t ld, const int64_t* targets,
                         float* loss_rows, float* lse, void* stream) {
    CG_REQUIRE(rows > 0 && V > 0 && V <= 1024, "cg_ce_fwd: bad shape");
    k_ce_fwd<false><<<ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(logits, rows, (int)V, ld, targets, loss_rows,
                                                                        lse, 0);
    CG_LAUNCH_CHECK("cg_ce_fwd");
    return CG_OK;
}

extern "C" int cg_ce_fwd_masked(const float* logits, int64_t rows, int64_t V, const int64_t* targets,
                                int64_t ignore_index, float* loss_rows, float* lse, void* stream) {
    CG_REQUIRE(rows > 0 && V > 0 && V <= 1024, "cg_ce_fwd_masked: bad shape");
    CG_REQUIRE(logits && targets && loss_rows && lse, "cg_ce_fwd_masked: null operand");
    k_ce_fwd<true><<<ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(logits, rows, (int)V, V, targets, loss_rows, lse,
                                                                       ignore_index);
    CG_LAUNCH_CHECK("cg_ce_fwd_masked");
    return CG_OK;
}

// What scales the loss gradient in k_ce_bwd: the host's g_mult or, MASKED (cg_ce_bwd_masked), the
// normaliser norm[1] read when the kernel runs, with the target value whose rows are left out.  A type
// per instantiation (as adamw.hip's AdamLr), so the unmasked kernel keeps the arguments it always had.
struct CeMask {
    const float* norm;
    int64_t ignore;
};
template <bool MASKED>
using CeScale = std::conditional_t<MASKED, CeMask, float>;

// dlogits = (*gp) g_mult (softmax - onehot); MASKED: norm[1] in place of g_mult, and an ignored row's
// dlogits is a literal 0, no product
template <bool MASKED>
__global__ void k_ce_bwd(const float* __restrict__ logits, int64_t rows, int V, int64_t ld,
                         const int64_t* __restrict__ targets, const float* __restrict__ lse,
                         const float* __restrict__ gp, CeScale<MASKED> sc, float* __restrict__ dlogits, int64_t ldd,
                         bf16_t* __restrict__ dlp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * V) return;
    const int64_t r = i / V;
    const int v = (int)(i % V);
    const int64_t t = targets[r];
    bool ign = false;
    if constexpr (MASKED) ign = t == sc.ignore;
    float d = 0.f;
    if (!ign) {
        float g;
        if constexpr (MASKED) g = *gp * sc.norm[1];
        else g = *gp * sc;
        const float p = expf(logits[r * ld + v] - lse[r]);
        d = (t < 0 || t >= V) ? __builtin_nanf("") : g * (p - (v == t ? 1.f : 0.f));
    }
    if (dlogits) dlogits[r * ldd + v] = d;
    if (dlp) dlp[r * ldd + v] = f2bf(d);
}

extern "C" int cg_ce_bwd(const float* logits, int64_t rows, int64_t V, int64_t ld, const int64_t* targets,
                         const float* lse, const float* g, float g_mult, float* dlogits, int64_t ld_d,
                         void* dst_lp, void* stream) {
    CG_REQUIRE(rows > 0 && V > 0, "cg_ce_bwd: bad shape");
    k_ce_bwd<false><<<ceil_div(rows * V, 256), 256, 0, (hipStream_t)stream>>>(
        logits, rows, (int)V, ld, targets, lse, g, g_mult, dlogits, ld_d, (bf16_t*)dst_lp);
    CG_LAUNCH_CHECK("cg_ce_bwd");
    return CG_OK;
}

extern "C" int cg_ce_bwd_masked(const float* logits, int64_t rows, int64_t V, const int64_t* targets,
                                int64_t ignore_index, const float* lse, const float* g, const float* norm,
                                float* dlogits, void* dst_lp, void* stream) {
    CG_REQUIRE(rows > 0 && V > 0, "cg_ce_bwd_masked: bad shape");
    CG_REQUIRE(logits && targets && lse && g && norm, "cg_ce_bwd_masked: null operand");
    k_ce_bwd<true><<<ceil_div(rows * V, 256), 256, 0, (hipStream_t)stream>>>(
        logits, rows, (int)V, V, targets, lse, g, CeMask{norm, ignore_index}, dlogits, V, (bf16_t*)dst_lp);
    CG_LAUNCH_CHECK("cg_ce_bwd_masked");
    return CG_OK;
}

// ---- the masked mean: dense row losses ------------------------------------------------------
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum of the row losses, count of the valid rows and the normaliser in one launch of one block.  The
// block walks cg_sum_f32's nb virtual blocks one after the other in that kernel pair's association
// order, so with no row ignored the loss has the bits of cg_sum_f32(loss_rows, 1 / rows).
// fpart / cpart: nb partials each (the workspace).
__global__ __launch_bounds__(256) void k_ce_mean_masked(const float* __restrict__ loss_rows,
                                                        const int64_t* __restrict__ targets, int64_t n,
                                                        int64_t ignore, int nb, float* fpart, int* cpart,
                                                        float* __restrict__ loss, float* __restrict__ norm) {
    __shared__ float red[4];
    __shared__ int redc[4];
    const int tid = threadIdx.x;
    for (int vb = 0; vb < nb; ++vb) {
        float s = 0.f;
        int c = 0;
        for (int64_t i = (int64_t)vb * 256 + tid; i < n; i += (int64_t)nb * 256) {
            s += loss_rows[i];
            c += targets[i] != ignore ? 1 : 0;
        }
        s = wave_sum(s);
        c = wave_sum_int(c);
        if ((tid & 63) == 0) {
            red[tid >> 6] = s;
            redc[tid >> 6] = c;
        }
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
            int tc = 0;
            for (int w = 0; w < 4; ++w) {
                t += red[w];
                tc += redc[w];
            }
            fpart[vb] = t;
            cpart[vb] = tc;
        }
        __syncthreads();
    }
    float s = 0.f;
    int c = 0;
    for (int i = tid; i < nb; i += 256) {
        s += fpart[i];
        c += cpart[i];
    }
    s = wave_sum(s);
    c = wave_sum_int(c);
    if ((tid & 63) == 0) {
        red[tid >> 6] = s;
        redc[tid >> 6] = c;
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        int tc = 0;
        for (int w = 0; w < 4; ++w) {
            t += red[w];
            tc += redc[w];
        }
        const float cnt = (float)tc;
        const float inv = __fdiv_rn(1.f, cnt);   // no valid row: inf, the loss 0 * inf = NaN (torch's)
        norm[0] = cnt;
        norm[1] = inv;
        *loss = t * inv;
    }
}

extern "C" int64_t cg_ce_mean_masked_workspace(int64_t rows) {
    int64_t nb = rows / 4096;
    nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
    return 2 * nb * (int64_t)sizeof(float);
}

extern "C" int cg_ce_mean_masked(const float* loss_rows, const int64_t* targets, int64_t rows, int64_t ignore_index,
                                 float* loss, float* norm, void* workspace, void* stream) {
    CG_REQUIRE(rows > 0 && rows < ((int64_t)1 << 24), "cg_ce_mean_masked: rows must be in [1, 2^24)");
    CG_REQUIRE(loss_rows && targets && loss && norm && workspace, "cg_ce_mean_masked: null operand");
    int nb = (int)(rows / 4096);   // cg_sum_f32's block count
    nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
    k_ce_mean_masked<<<1, 256, 0, (hipStream_t)stream>>>(loss_rows, targets, rows, ignore_index, nb,
                                                         (float*)workspace, (int*)workspace + nb, loss, norm);
    CG_LAUNCH_CHECK("cg_ce_mean_masked");
    return CG_OK;
}
