// charpt: global-norm gradient clipping over the flat gradient buffer (torch.nn.utils.clip_grad_norm_
// with norm_type 2): the L2 norm and the clip coefficient on the device, and the in-place scale for
// hand-written loops.  The training step multiplies by the coefficient inside AdamW instead
// (adamw.hip cg_adamw_dyn), so clipping costs one 4 B/param read pass.
#include <math.h>

#include "common.h"

using namespace cg;

namespace {
// The launch depends only on n: ceil(n4 / (256 * GN_U)) blocks of 256 threads, at most GN_MAX_BLOCKS;
// one sweep of the full grid covers GN_MAX_BLOCKS * 256 * GN_U float4 groups = 8 Mi floats.
constexpr int GN_THREADS = 256, GN_U = 4, GN_MAX_BLOCKS = 2048;

inline int gn_blocks(int64_t n) {
    const int64_t nb = (n / 4 + (int64_t)GN_THREADS * GN_U - 1) / ((int64_t)GN_THREADS * GN_U);
    return nb < 1 ? 1 : (nb > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : (int)nb);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the block in a fixed order (lane butterflies, then waves 0..3 in turn); thread 0 has it
__device__ __forceinline__ double block_sum_f64(double s) {
    __shared__ double red[GN_THREADS / 64];
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < GN_THREADS / 64; ++w) t += red[w];
    return t;
}

__device__ __forceinline__ double sq4(double s, const float4 x) {
    // the product of two floats is exact in fp64; only the additions round
    s = fma((double)x.x, (double)x.x, s);
    s = fma((double)x.y, (double)x.y, s);
    s = fma((double)x.z, (double)x.z, s);
    return fma((double)x.w, (double)x.w, s);
}

// pass 1: part[block] = the block's sum of squares.  g: the caller's pointer (any 4-B alignment);
// head: elements before the first 16-B boundary (0..3, <= n); the float4 body follows; the head and
// the (n - head) % 4 tail elements go to block 0's first threads.  Which thread sums which elements
// is fixed by (n, alignment, grid), and every fold is ordered: the same bits on every run and rank.
__global__ __launch_bounds__(GN_THREADS) void k_grad_sumsq(const float* __restrict__ g, int64_t n, int head,
                                                            double* __restrict__ part) {
    const float* body = g + head;
    const int64_t n4 = (n - head) / 4;
    const int64_t stride = (int64_t)gridDim.x * GN_THREADS;
    int64_t i = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x;
    double s = 0.0;
    for (; i + (GN_U - 1) * stride < n4; i += GN_U * stride) {
        float4 x[GN_U];
#pragma unroll
        for (int u = 0; u < GN_U; ++u) x[u] = *(const float4*)(body + 4 * (i + u * stride));
#pragma unroll
        for (int u = 0; u < GN_U; ++u) s = sq4(s, x[u]);
    }
    for (; i < n4; i += stride) s = sq4(s, *(const float4*)(body + 4 * i));
    if (blockIdx.x == 0) {
        const int tail = (int)(n - head - 4 * n4);
        const int t = threadIdx.x;
        if (t < head) s = fma((double)g[t], (double)g[t], s);
        else if (t < head + tail) {
            const float x = body[4 * n4 + (t - head)];
            s = fma((double)x, (double)x, s);
        }
    }
    s = block_sum_f64(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// pass 2 (one block): out[0] = (float)sqrt(sum of the partials), out[1] = min(1, max_norm / (norm + 1e-6))
// in fp32 as torch's clip_grad_norm_ computes it (one add, one correctly rounded divide, no contraction)
__global__ __launch_bounds__(GN_THREADS) void k_grad_norm_final(const double* __restrict__ part, int np,
                                                                 float max_norm, float* __restrict__ out) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += GN_THREADS) s += part[i];
    s = block_sum_f64(s);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const float c = __fdiv_rn(max_norm, norm + 1e-6f);
        out[0] = norm;
        out[1] = c < 1.f ? c : 1.f;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_scale_f32(float* __restrict__ x, int64_t n, const float* __restrict__ scale) {
    const float c = *scale;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if (VEC && i + 3 < n) {
            float4 v = *(const float4*)(x + i);
            v.x *= c;
            v.y *= c;
            v.z *= c;
            v.w *= c;
            *(float4*)(x + i) = v;
        } else {
            for (int64_t j = i; j < n && j < i + 4; ++j) x[j] *= c;
        }
    }
}
}  // namespace

extern "C" int64_t cg_grad_norm_workspace(int64_t n) { return (int64_t)gn_blocks(n < 0 ? 0 : n) * (int64_t)sizeof(double); }

extern "C" int cg_grad_norm(const float* g, int64_t n, float max_norm, float* out, void* workspace, void* stream) {
    CG_REQUIRE(n >= 0 && out && workspace && (g || n == 0), "cg_grad_norm: bad arguments");
    CG_REQUIRE((((uintptr_t)g) & 3) == 0 && (((uintptr_t)workspace) & 7) == 0,
               "cg_grad_norm: g must be 4-B aligned, the workspace 8-B aligned");
    hipStream_t st = (hipStream_t)stream;
    int nb = 0;
    if (n > 0) {
        int64_t head = ((16 - (int64_t)(((uintptr_t)g) & 15)) & 15) / 4;
        head = head > n ? n : head;
        nb = gn_blocks(n);
        k_grad_sumsq<<<nb, GN_THREADS, 0, st>>>(g, n, (int)head, (double*)workspace);
    }
    k_grad_norm_final<<<1, GN_THREADS, 0, st>>>((const double*)workspace, nb, max_norm, out);
    CG_LAUNCH_CHECK("cg_grad_norm");
    return CG_OK;
}

extern "C" int cg_scale_f32(float* x, int64_t n, const float* scale_dev, void* stream) {
    CG_REQUIRE(n >= 0 && scale_dev && (x || n == 0), "cg_scale_f32: bad arguments");
    if (n == 0) return CG_OK;
    int grid = ceil_div((n + 3) / 4, 256);
    grid = grid > 8192 ? 8192 : grid;
    if ((((uintptr_t)x) & 15) == 0) k_scale_f32<true><<<grid, 256, 0, (hipStream_t)stream>>>(x, n, scale_dev);
    else k_scale_f32<false><<<grid, 256, 0, (hipStream_t)stream>>>(x, n, scale_dev);
    CG_LAUNCH_CHECK("cg_scale_f32");
    return CG_OK;
}
