// charpt: the deterministic reduce kernels -- the split-K slab sums behind cg_gemm (and the deferred
// ones cg_flush_deferred launches), the bias-gradient column sums (cg_colsum) and the column reduction of
// per-block partials (LayerNorm dgamma / dbeta, cg_reduce_rows), single-job and multi-job.
#include "defer.h"

using namespace cg;

namespace {

template <typename TC>
__global__ void k_splitk_reduce(const float* __restrict__ ws, int split_k, int64_t M, int64_t N, TC* __restrict__ C,
                                int64_t ldc, EpiArgs epi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * N) return;
    const int64_t m = i / N, n = i % N;
    float s = 0.f;
    for (int k = 0; k < split_k; ++k) s += ws[(int64_t)k * M * N + i];
    const uint64_t stream = (epi.kind == CG_EPI_BIAS_DROP_RESID && epi.thr) ? dropout_stream(epi.rng_call, epi.site) : 0;
    store_out<TC>(C, m * ldc + n, epi_scalar(epi, s, m, n, N, stream), epi.beta);
}

// Vectorised form for the MFMA path's slabs (N % 4 == 0, 16-B aligned rows): four consecutive
// columns per thread, every slab load issued before the sum, 32-bit index math (the scalar form
// above spent its time in 64-bit division; measured 12.8 us for the C2 FFN weight gradient, split 8).
// Same summation order (k = 0..split-1) and epilogue arithmetic as epi_scalar, so results are
// bitwise those of the scalar form.
// S > 0: compile-time split, every slab's float4 loaded before the first add (S loads in flight per
// thread instead of 4); the adds still run k = 0..S-1 in order.
// bf16 slabs of an fp32 STORE output (cg_set_tuning "slab_bf16"): 8 outputs per thread
__global__ __launch_bounds__(256) void k_slab16_reduce8(const void* __restrict__ ws, int S, int64_t n8,
                                                        float* __restrict__ out, float beta) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n8) slab16_chunk8(ws, S, 8 * n8, i, out, beta);
}

template <typename TC, int S>
__global__ __launch_bounds__(256) void k_splitk_reduce4(const float* __restrict__ ws, int split_k, int M, int N,
                                                        TC* __restrict__ C, int64_t ldc, EpiArgs epi) {
    const int n4 = N >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M * n4) return;
    const int m = i / n4, n = (i - m * n4) * 4;
    const int64_t slab = (int64_t)M * N, p = (int64_t)m * N + n;
    const bool sb = epi.slab_bf16;   // bf16 slabs (cg_set_tuning "slab_bf16"): same order, widened exactly
    fv4 s;
    int k = 1;
    if constexpr (S > 0) {
        fv4 a[S];
#pragma unroll
        for (int j = 0; j < S; ++j) a[j] = ld_slab4(ws, p + j * slab, sb);   // slabs are read once
        s = a[0];
#pragma unroll
        for (int j = 1; j < S; ++j) s += a[j];
        k = split_k;
    } else {
        s = ld_slab4(ws, p, sb);
    }
    for (; k + 4 <= split_k; k += 4) {
        const fv4 a = ld_slab4(ws, p + k * slab, sb), b = ld_slab4(ws, p + (k + 1) * slab, sb);
        const fv4 c = ld_slab4(ws, p + (k + 2) * slab, sb), d = ld_slab4(ws, p + (k + 3) * slab, sb);
        s += a;
        s += b;
        s += c;
        s += d;
    }
    for (; k < split_k; ++k) s += ld_slab4(ws, p + k * slab, sb);
    float v[4] = {s[0], s[1], s[2], s[3]};
    if (epi.kind != CG_EPI_STORE && epi.bias) {
        const float4 b = *(const float4*)(epi.bias + n);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    if (epi.kind == CG_EPI_BIAS_RESID && epi.resid) {
        const float4 r = *(const float4*)(epi.resid + (int64_t)m * epi.ld_resid + n);
        v[0] = r.x + v[0]; v[1] = r.y + v[1]; v[2] = r.z + v[2]; v[3] = r.w + v[3];
    }
    TC* o = C + (int64_t)m * ldc + n;
#pragma unroll
    for (int q = 0; q < 4; ++q) store_out<TC>(o, q, v[q], epi.beta);
}

// =====================================================================================
// column sums (bias gradients): out[n] (=|+=) sum_m X[m,n]
// =====================================================================================
constexpr int CS_ROWS = 256;

// per 256-row chunk column partials: 64 columns x 4 row-lanes, 8 loads in flight per thread
template <typename TX>
__global__ __launch_bounds__(256) void k_colsum_partial(const TX* __restrict__ X, int64_t rows, int64_t N,
                                                        int64_t ldx, float* __restrict__ part) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * 64 + c;
    const int64_t r0 = (int64_t)blockIdx.y * CS_ROWS;
    float s = 0.f;
    if (n < N) {
        if (r0 + CS_ROWS <= rows) {
#pragma unroll
            for (int j0 = 0; j0 < CS_ROWS / 4; j0 += 16) {
                float v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = ld_as_f32<TX>(X + (r0 + rl + 4 * (j0 + j)) * ldx + n);
#pragma unroll
                for (int j = 0; j < 16; ++j) s += v[j];
            }
        } else {
            for (int64_t r = r0 + rl; r < rows; r += 4) s += ld_as_f32<TX>(X + r * ldx + n);
        }
    }
    red[rl][c] = s;
    __syncthreads();
    if (rl == 0 && n < N) part[(int64_t)blockIdx.y * N + n] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

}  // namespace

// --------------------------------------------------------------------------------------
// column reduction of per-block partials [K][N] (LayerNorm dgamma/dbeta, bias column sums):
// 16 columns x 64 row-lanes per block, float4 loads, all of a lane's rows (8 at K = 512) in flight,
// then the 64 row-lane sums added in a fixed order (deterministic).  The former 32-column blocks
// (72 blocks at C4, 8 loads in flight per lane) ran 130 us for 9.4 MB.
// Column n goes to out_a[n] (n < S), out_b[n - S] (n < 2S) or out_c[n - 2S]; NULL drops it.
// One block's work (block blk of the job's ceil(N / 16)): shared by the single-job kernel and the
// deferred multi-job one, so both give the same bits.
__device__ __forceinline__ void reduce_partials_block(const float* __restrict__ part, int64_t K, int64_t N,
                                                      float* __restrict__ out_a, float* __restrict__ out_b,
                                                      float* __restrict__ out_c, int64_t S, int accumulate,
                                                      int accumulate_c, int64_t blk, float (*red)[17]) {
    const int cq = threadIdx.x & 3, rl = threadIdx.x >> 2;
    const int64_t n0 = blk * 16 + 4 * cq;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if ((N & 3) == 0 && (((uintptr_t)part) & 15) == 0) {
        if (n0 < N) {
            int64_t k = rl;
            for (; k + 7 * 64 < K; k += 8 * 64) {
                float4 v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = *(const float4*)(part + (k + 64 * j) * N + n0);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    a[0] += v[j].x;
                    a[1] += v[j].y;
                    a[2] += v[j].z;
                    a[3] += v[j].w;
                }
            }
            for (; k < K; k += 64) {
                const float4 v = *(const float4*)(part + k * N + n0);
                a[0] += v.x;
                a[1] += v.y;
                a[2] += v.z;
                a[3] += v.w;
            }
        }
    } else {
        for (int64_t k = rl; k < K; k += 64)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (n0 + q < N) a[q] += part[k * N + n0 + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[rl][4 * cq + q] = a[q];
    __syncthreads();
    if (threadIdx.x < 16) {
        const int c = threadIdx.x;
        const int64_t n = blk * 16 + c;
        if (n < N) {
            float t = 0.f;
            for (int j = 0; j < 64; ++j) t += red[j][c];
            float* dst;
            int acc = accumulate;
            if (n < S) dst = out_a ? out_a + n : nullptr;
            else if (n < 2 * S) dst = out_b ? out_b + (n - S) : nullptr;
            else {
                dst = out_c ? out_c + (n - 2 * S) : nullptr;
                acc = accumulate_c;
            }
            if (dst) *dst = acc ? *dst + t : t;
        }
    }
}

__global__ __launch_bounds__(256) void k_reduce_partials(const float* __restrict__ part, int64_t K, int64_t N,
                                                         float* __restrict__ out_a, float* __restrict__ out_b,
                                                         float* __restrict__ out_c, int64_t S, int accumulate,
                                                         int accumulate_c) {
    __shared__ float red[64][17];
    reduce_partials_block(part, K, N, out_a, out_b, out_c, S, accumulate, accumulate_c, blockIdx.x, red);
}

__global__ __launch_bounds__(256) void k_reduce_partials_multi(cg::PartJobs jobs) {
    __shared__ float red[64][17];
    const int b = blockIdx.x;
    int q = 0;
    while (q + 1 < jobs.n && b >= jobs.start[q + 1]) ++q;
    const cg::PartJob& j = jobs.j[q];
    reduce_partials_block(j.part, j.K, j.N, j.a, j.b, j.c, j.S, j.acc, j.acc_c, b - jobs.start[q], red);
}

namespace cg {
// the split-K reduce's one launch site (cg_gemm; a flushed deferred job is one row of 4 n4 elements):
// bf16 slabs of an fp32 STORE output 8 per thread, else with vec4 four columns per thread (the split
// unrolled for the splits the training shapes use), else the scalar form
void launch_splitk_reduce(const void* ws, int S, int64_t M, int64_t N, void* C, int c_dtype, int64_t ldc,
                          const EpiArgs& e, bool vec4, hipStream_t st) {
    if (e.slab_bf16 && M * N % 8 == 0) {
        const int64_t n8 = M * N / 8;
        k_slab16_reduce8<<<ceil_div(n8, 256), 256, 0, st>>>(ws, S, n8, (float*)C, e.beta);
    } else if (vec4) {
        const int n4 = (int)(M * N / 4);
#define SKR(TC_, S_) \
    k_splitk_reduce4<TC_, S_><<<ceil_div(n4, 256), 256, 0, st>>>((const float*)ws, S, (int)M, (int)N, (TC_*)C, ldc, e)
#define SKR_ANY(TC_)                  \
    switch (S) {                      \
        case 2: SKR(TC_, 2); break;   \
        case 4: SKR(TC_, 4); break;   \
        case 8: SKR(TC_, 8); break;   \
        case 12: SKR(TC_, 12); break; \
        case 14: SKR(TC_, 14); break; \
        case 16: SKR(TC_, 16); break; \
        case 32: SKR(TC_, 32); break; \
        default: SKR(TC_, 0); break;  \
    }
        if (c_dtype == CG_BF16) {
            SKR_ANY(bf16_t)
        } else {
            SKR_ANY(float)
        }
#undef SKR_ANY
#undef SKR
    } else if (c_dtype == CG_BF16) {
        k_splitk_reduce<bf16_t><<<ceil_div(M * N, 256), 256, 0, st>>>((const float*)ws, S, M, N, (bf16_t*)C, ldc, e);
    } else {
        k_splitk_reduce<float><<<ceil_div(M * N, 256), 256, 0, st>>>((const float*)ws, S, M, N, (float*)C, ldc, e);
    }
}

void launch_reduce_partials_multi(const PartJobs& jobs, hipStream_t st) {
    k_reduce_partials_multi<<<jobs.start[jobs.n], 256, 0, st>>>(jobs);
}


void launch_reduce_partials(const float* part, int64_t K, int64_t N, float* out_a, float* out_b, int64_t S,
                            int accumulate, hipStream_t st) {
    {
        std::lock_guard<std::mutex> lk(defer_mutex());
        DeferQueue* q = defer_queue(st, false);
        flush_parts_touching_locked(q, out_a, S);
        flush_parts_touching_locked(q, out_b, N - S);
    }
    k_reduce_partials<<<ceil_div(N, 16), 256, 0, st>>>(part, K, N, out_a, out_b, nullptr, S, accumulate, 0);
}
void launch_reduce_partials3(const float* part, int64_t K, int64_t N, float* out_a, float* out_b, float* out_c,
                             int64_t S, int accumulate, int accumulate_c, hipStream_t st) {
    {
        std::lock_guard<std::mutex> lk(defer_mutex());
        DeferQueue* q = defer_queue(st, false);
        flush_parts_touching_locked(q, out_a, S);
        flush_parts_touching_locked(q, out_b, S);
        flush_parts_touching_locked(q, out_c, N - 2 * S);
    }
    k_reduce_partials<<<ceil_div(N, 16), 256, 0, st>>>(part, K, N, out_a, out_b, out_c, S, accumulate, accumulate_c);
}
// the deferrable forms (cg_layernorm_bwd_reduce_ex, cg_reduce_rows_ex, cg_head_bwd_ex): queued on the
// stream's DeferQueue with CG_DEFER, else launched now
void reduce_partials_deferrable(const float* part, int64_t K, int64_t N, float* out_a, float* out_b, float* out_c,
                                int64_t S, int accumulate, int accumulate_c, int defer, hipStream_t st) {
    if (defer) {
        enqueue_partials(PartJob{part, K, N, S, out_a, out_b, out_c, accumulate, accumulate_c}, st);
        return;
    }
    launch_reduce_partials3(part, K, N, out_a, out_b, out_c, S, accumulate, accumulate_c, st);
}
}  // namespace cg

extern "C" int cg_reduce_rows_ex(const float* part, int64_t rows, int64_t N, float* out, int accumulate, int flags,
                                 void* stream) {
    CG_REQUIRE(part && out && rows > 0 && N > 0, "cg_reduce_rows: bad arguments");
    CG_REQUIRE((flags & ~CG_DEFER) == 0, "cg_reduce_rows_ex: unknown flags %#x", flags);
    reduce_partials_deferrable(part, rows, N, out, nullptr, nullptr, N, accumulate, 0, flags & CG_DEFER,
                               (hipStream_t)stream);
    CG_LAUNCH_CHECK("cg_reduce_rows");
    return CG_OK;
}

extern "C" int cg_reduce_rows(const float* part, int64_t rows, int64_t N, float* out, int accumulate, void* stream) {
    return cg_reduce_rows_ex(part, rows, N, out, accumulate, 0, stream);
}

extern "C" int64_t cg_colsum_workspace(int64_t rows, int64_t N) {
    return ((rows + CS_ROWS - 1) / CS_ROWS) * N * (int64_t)sizeof(float);
}

extern "C" int cg_colsum(const void* X, int x_dtype, int64_t rows, int64_t N, int64_t ldx, float* out, int accumulate,
                         void* workspace, void* stream) {
    CG_REQUIRE(rows > 0 && N > 0, "cg_colsum: empty");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunk = (rows + CS_ROWS - 1) / CS_ROWS;
    dim3 grid(ceil_div(N, 64), (unsigned)nchunk);
    if (x_dtype == CG_BF16)
        k_colsum_partial<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)X, rows, N, ldx, (float*)workspace);
    else
        k_colsum_partial<float><<<grid, 256, 0, st>>>((const float*)X, rows, N, ldx, (float*)workspace);
    launch_reduce_partials((const float*)workspace, nchunk, N, out, nullptr, N, accumulate, st);
    CG_LAUNCH_CHECK("cg_colsum");
    return CG_OK;
}
