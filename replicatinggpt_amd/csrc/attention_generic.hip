// charpt: fused causal self-attention over all heads -- Head.forward (GPT1.py:109-123) run for
// every head of MultiHeadAttention (GPT1.py:134-135) without materialising the T x T scores.
//
//   S = q k^T * scale (scale = n_embd^-0.5); S[j > i] = -inf (tril, GPT1.py:115);
//   P = softmax(S) (GPT1.py:116); P = dropout(P) (GPT1.py:117); out = P v (GPT1.py:122).
//
// Online softmax, logsumexp saved for the backward, dropout regenerated from the Philox
// counter (element idx = ((b*H + h)*T + i)*T + j).  Backward = FlashAttention-2 style
// recompute split in two deterministic kernels (dK/dV per key block, dQ per query block), so no
// float atomics are needed.
//
// This file: the *_generic kernels -- fp32 math, any head size D <= 128 and any T; the fp32 parity
// path and the as-shipped head_size 21.  32x32 blocks, VALU dot products.  The other
// families: attention_f32.hip (fp32 MFMA forward, D <= 32, no dropout) and attention_d64.hip (bf16
// MFMA 32x32x16, D = 64, T % 64 == 0 -- the C2/C4 perf path); attention.hip picks among them.
#include "attention_common.h"

using namespace cg;

namespace {

__device__ __forceinline__ bool keep_elem(const DropArgs& d, uint64_t stream, uint64_t idx) {
    return keep_of(philox_of(d.seed, stream, idx), idx, d.thr);
}

// =====================================================================================
// generic fp32 kernels
// =====================================================================================
constexpr int GB = 32;  // rows per block (queries or keys)

template <typename T>
__device__ __forceinline__ void load_rows(float* dst, int DP, const T* base, int64_t ld, int64_t row0, int64_t T_,
                                          int D, int tid) {
    for (int i = tid; i < GB * D; i += 256) {
        const int r = i / D, e = i % D;
        const int64_t t = row0 + r;
        dst[r * DP + e] = t < T_ ? ld_as_f32<T>(base + t * ld + e) : 0.f;
    }
}

// SEG: packed rows -- query i sees key j iff seg_start[b, i] <= j <= i (seg_lo / seg_hi below clamp a
// malformed bound so that every query still sees itself); the dK/dV kernel reads the same mask from
// the key's side, seg_end[b, j] > i.
__device__ __forceinline__ int64_t seg_lo(const int32_t* seg_start, int64_t row, int64_t qa) {
    const int64_t s = seg_start[row];
    return s < 0 ? 0 : (s > qa ? qa : s);
}
__device__ __forceinline__ int64_t seg_hi(const int32_t* seg_end, int64_t row, int64_t ka, int64_t T_) {
    const int64_t e = seg_end[row];
    return e <= ka ? ka + 1 : (e > T_ ? T_ : e);
}

template <typename T, bool SEG>
__global__ __launch_bounds__(256) void k_attn_fwd_generic(int64_t T_, int H, int D, const T* __restrict__ q,
                                                          const T* __restrict__ k, const T* __restrict__ v, int64_t ld,
                                                          T* __restrict__ o, int64_t ldo, float* __restrict__ lse,
                                                          float scale, DropArgs drop,
                                                          const int32_t* __restrict__ seg_start) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int DP = D + 1;
    float* Qs = sm;
    float* Ks = Qs + GB * DP;
    float* Vs = Ks + GB * DP;
    float* Ps = Vs + GB * DP;  // [GB][GB+1]
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int qb = blockIdx.x;
    const int64_t q0 = (int64_t)qb * GB;
    const int tid = threadIdx.x, qi = tid >> 3, sub = tid & 7;
    const int64_t qa = q0 + qi;
    const T* qbase = q + (int64_t)b * T_ * ld + h * D;
    const T* kbase = k + (int64_t)b * T_ * ld + h * D;
    const T* vbase = v + (int64_t)b * T_ * ld + h * D;
    load_rows<T>(Qs, DP, qbase, ld, q0, T_, D, tid);
    int64_t ss = 0;
    if constexpr (SEG) ss = qa < T_ ? seg_lo(seg_start, (int64_t)b * T_ + qa, qa) : 0;
    const uint64_t stream = drop.thr ? dropout_stream(drop.rng_call, drop.site) : 0;
    float m_run = -INFINITY, l_run = 0.f;
    float oacc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) oacc[j] = 0.f;
    for (int kb = 0; kb <= qb; ++kb) {
        const int64_t k0 = (int64_t)kb * GB;
        __syncthreads();
        load_rows<T>(Ks, DP, kbase, ld, k0, T_, D, tid);
        load_rows<T>(Vs, DP, vbase, ld, k0, T_, D, tid);
        __syncthreads();
        float s[4], mx = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = sub + 8 * jj;
            const int64_t key = k0 + j;
            float acc = 0.f;
            for (int e = 0; e < D; ++e) acc += Qs[qi * DP + e] * Ks[j * DP + e];
            acc *= scale;
            if (key > qa || key >= T_) acc = -INFINITY;
            if constexpr (SEG) {
                if (key < ss) acc = -INFINITY;
            }
            s[jj] = acc;
            mx = fmaxf(mx, acc);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = m_new == -INFINITY ? 1.f : expf(m_run - m_new);
        float psum = 0.f;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = sub + 8 * jj;
            const float p = s[jj] == -INFINITY ? 0.f : expf(s[jj] - m_new);
            psum += p;
            float pd = p;
            if (drop.thr && p != 0.f) {
                const uint64_t idx = (((uint64_t)bh * T_ + qa) * T_ + (k0 + j));
                pd = keep_elem(drop, stream, idx) ? p * drop.dscale : 0.f;
            }
            Ps[qi * (GB + 1) + j] = pd;
        }
        psum += __shfl_xor(psum, 1, 64);
        psum += __shfl_xor(psum, 2, 64);
        psum += __shfl_xor(psum, 4, 64);
        l_run = l_run * alpha + psum;
        m_run = m_new;
        __syncthreads();
#pragma unroll
        for (int j8 = 0; j8 < 16; ++j8) {
            const int e = sub + 8 * j8;
            if (e < D) {
                float a = oacc[j8] * alpha;
                for (int j = 0; j < GB; ++j) a += Ps[qi * (GB + 1) + j] * Vs[j * DP + e];
                oacc[j8] = a;
            }
        }
    }
    if (qa < T_) {
        const float inv = 1.f / l_run;
        T* orow = o + ((int64_t)b * T_ + qa) * ldo + h * D;
#pragma unroll
        for (int j8 = 0; j8 < 16; ++j8) {
            const int e = sub + 8 * j8;
            if (e < D) st_from_f32<T>(orow + e, oacc[j8] * inv);
        }
        if (sub == 0) lse[(int64_t)bh * T_ + qa] = m_run + logf(l_run);
    }
}

// delta[bh, t] = sum_e dO * O  -- one thread per (b, t, h) row
template <typename T>
__global__ void k_attn_delta(int64_t B, int64_t T_, int H, int D, const T* __restrict__ o, int64_t ldo,
                             const T* __restrict__ dout, int64_t ldd, float* __restrict__ delta) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (b*T + t)*H + h
    if (row >= B * T_ * H) return;
    const int64_t bt = row / H;
    const int h = (int)(row % H);
    const int64_t b = bt / T_, t = bt % T_;
    const T* op = o + bt * ldo + h * D;
    const T* dp = dout + bt * ldd + h * D;
    float s = 0.f;
    if (sizeof(T) == 2 && D % 8 == 0 && ((((uintptr_t)op) | ((uintptr_t)dp)) & 15) == 0) {
        for (int e = 0; e < D; e += 8) {
            const uint4 a = *(const uint4*)(op + e), c = *(const uint4*)(dp + e);
            const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, cw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s += __uint_as_float(aw[q] << 16) * __uint_as_float(cw[q] << 16);
                s += __uint_as_float(aw[q] & 0xffff0000u) * __uint_as_float(cw[q] & 0xffff0000u);
            }
        }
    } else {
        for (int e = 0; e < D; ++e) s += ld_as_f32<T>(op + e) * ld_as_f32<T>(dp + e);
    }
    delta[(b * H + h) * T_ + t] = s;
}

template <typename T, bool SEG>
__global__ __launch_bounds__(256) void k_attn_dq_generic(int64_t T_, int H, int D, const T* __restrict__ q,
                                                         const T* __restrict__ k, const T* __restrict__ v, int64_t ld,
                                                         const T* __restrict__ dout, int64_t ldd,
                                                         const float* __restrict__ lse,
                                                         const float* __restrict__ delta, T* __restrict__ dq,
                                                         int64_t lddq, float scale, DropArgs drop,
                                                         const int32_t* __restrict__ seg_start) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int DP = D + 1;
    float* Qs = sm;
    float* Os = Qs + GB * DP;  // dO rows
    float* Ks = Os + GB * DP;
    float* Vs = Ks + GB * DP;
    float* Ss = Vs + GB * DP;  // dS [GB][GB+1]
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int qb = blockIdx.x;
    const int64_t q0 = (int64_t)qb * GB;
    const int tid = threadIdx.x, qi = tid >> 3, sub = tid & 7;
    const int64_t qa = q0 + qi;
    const int64_t boff = (int64_t)b * T_;
    load_rows<T>(Qs, DP, q + boff * ld + h * D, ld, q0, T_, D, tid);
    load_rows<T>(Os, DP, dout + boff * ldd + h * D, ldd, q0, T_, D, tid);
    const bool valid_q = qa < T_;
    const float lq = valid_q ? lse[(int64_t)bh * T_ + qa] : 0.f;
    const float dq_ = valid_q ? delta[(int64_t)bh * T_ + qa] : 0.f;
    int64_t ss = 0;
    if constexpr (SEG) ss = valid_q ? seg_lo(seg_start, boff + qa, qa) : 0;
    const uint64_t stream = drop.thr ? dropout_stream(drop.rng_call, drop.site) : 0;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int kb = 0; kb <= qb; ++kb) {
        const int64_t k0 = (int64_t)kb * GB;
        __syncthreads();
        load_rows<T>(Ks, DP, k + boff * ld + h * D, ld, k0, T_, D, tid);
        load_rows<T>(Vs, DP, v + boff * ld + h * D, ld, k0, T_, D, tid);
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = sub + 8 * jj;
            const int64_t key = k0 + j;
            float ds = 0.f;
            if (valid_q && key <= qa && (!SEG || key >= ss)) {
                float s = 0.f, dp = 0.f;
                for (int e = 0; e < D; ++e) {
                    s += Qs[qi * DP + e] * Ks[j * DP + e];
                    dp += Os[qi * DP + e] * Vs[j * DP + e];
                }
                const float p = expf(s * scale - lq);
                if (drop.thr) {
                    const uint64_t idx = (((uint64_t)bh * T_ + qa) * T_ + key);
                    dp = keep_elem(drop, stream, idx) ? dp * drop.dscale : 0.f;
                }
                ds = p * (dp - dq_);
            }
            Ss[qi * (GB + 1) + j] = ds;
        }
        __syncthreads();
#pragma unroll
        for (int j8 = 0; j8 < 16; ++j8) {
            const int e = sub + 8 * j8;
            if (e < D) {
                float a = acc[j8];
                for (int j = 0; j < GB; ++j) a += Ss[qi * (GB + 1) + j] * Ks[j * DP + e];
                acc[j8] = a;
            }
        }
    }
    if (valid_q) {
        T* row = dq + (boff + qa) * lddq + h * D;
#pragma unroll
        for (int j8 = 0; j8 < 16; ++j8) {
            const int e = sub + 8 * j8;
            if (e < D) st_from_f32<T>(row + e, acc[j8] * scale);
        }
    }
}

template <typename T, bool SEG>
__global__ __launch_bounds__(256) void k_attn_dkdv_generic(int64_t T_, int H, int D, const T* __restrict__ q,
                                                           const T* __restrict__ k, const T* __restrict__ v,
                                                           int64_t ld, const T* __restrict__ dout, int64_t ldd,
                                                           const float* __restrict__ lse,
                                                           const float* __restrict__ delta, T* __restrict__ dk,
                                                           T* __restrict__ dv, int64_t lddkv, float scale,
                                                           DropArgs drop, const int32_t* __restrict__ seg_end) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int DP = D + 1;
    float* Ks = sm;
    float* Vs = Ks + GB * DP;
    float* Qs = Vs + GB * DP;
    float* Os = Qs + GB * DP;
    float* Zs = Os + GB * DP;        // [key][q]
    float* Ds = Zs + GB * (GB + 1);  // [key][q]
    float* Ls = Ds + GB * (GB + 1);  // lse[GB], delta[GB]
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int kb = blockIdx.x;
    const int64_t k0 = (int64_t)kb * GB;
    const int tid = threadIdx.x, kj = tid >> 3, sub = tid & 7;
    const int64_t ka = k0 + kj;
    const int64_t boff = (int64_t)b * T_;
    load_rows<T>(Ks, DP, k + boff * ld + h * D, ld, k0, T_, D, tid);
    load_rows<T>(Vs, DP, v + boff * ld + h * D, ld, k0, T_, D, tid);
    int64_t se = T_;
    if constexpr (SEG) se = ka < T_ ? seg_hi(seg_end, boff + ka, ka, T_) : T_;
    const uint64_t stream = drop.thr ? dropout_stream(drop.rng_call, drop.site) : 0;
    float adk[16], adv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) adk[j] = adv[j] = 0.f;
    const int nqb = (int)((T_ + GB - 1) / GB);
    for (int qb = kb; qb < nqb; ++qb) {
        const int64_t q0 = (int64_t)qb * GB;
        __syncthreads();
        load_rows<T>(Qs, DP, q + boff * ld + h * D, ld, q0, T_, D, tid);
        load_rows<T>(Os, DP, dout + boff * ldd + h * D, ldd, q0, T_, D, tid);
        if (tid < GB) {
            const int64_t t = q0 + tid;
            Ls[tid] = t < T_ ? lse[(int64_t)bh * T_ + t] : 0.f;
            Ls[GB + tid] = t < T_ ? delta[(int64_t)bh * T_ + t] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int qi = sub + 8 * ii;
            const int64_t qa = q0 + qi;
            float z = 0.f, ds = 0.f;
            if (ka < T_ && qa < T_ && ka <= qa && (!SEG || qa < se)) {
                float s = 0.f, dp = 0.f;
                for (int e = 0; e < D; ++e) {
                    s += Ks[kj * DP + e] * Qs[qi * DP + e];
                    dp += Vs[kj * DP + e] * Os[qi * DP + e];
                }
                const float p = expf(s * scale - Ls[qi]);
                z = p;
                if (drop.thr) {
                    const uint64_t idx = (((uint64_t)bh * T_ + qa) * T_ + ka);
                    const bool kp = keep_elem(drop, stream, idx);
                    z = kp ? p * drop.dscale : 0.f;
                    dp = kp ? dp * drop.dscale : 0.f;
                }
                ds = p * (dp - Ls[GB + qi]);
            }
            Zs[kj * (GB + 1) + qi] = z;
            Ds[kj * (GB + 1) + qi] = ds;
        }
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < GB; ++i) {
            const float zi = Zs[kj * (GB + 1) + i], di = Ds[kj * (GB + 1) + i];
#pragma unroll
            for (int j8 = 0; j8 < 16; ++j8) {
                const int e = sub + 8 * j8;
                if (e < D) {
                    adv[j8] += zi * Os[i * DP + e];
                    adk[j8] += di * Qs[i * DP + e];
                }
            }
        }
    }
    if (ka < T_) {
        T* krow = dk + (boff + ka) * lddkv + h * D;
        T* vrow = dv + (boff + ka) * lddkv + h * D;
#pragma unroll
        for (int j8 = 0; j8 < 16; ++j8) {
            const int e = sub + 8 * j8;
            if (e < D) {
                st_from_f32<T>(krow + e, adk[j8] * scale);
                st_from_f32<T>(vrow + e, adv[j8]);
            }
        }
    }
}

template <typename T>
size_t generic_lds(int D, int nrows_blocks, int nsq) {
    return (size_t)(nrows_blocks * GB * (D + 1) + nsq * GB * (GB + 1) + 2 * GB) * sizeof(float);
}

// f(T{}): the element type of a CG_BF16 / CG_F32 tensor
template <typename F>
void with_dtype(int dtype, F&& f) {
    if (dtype == CG_BF16) f(bf16_t{});
    else f(float{});
}

}  // namespace

namespace cg {
namespace attn {
void launch_fwd_generic(int dtype, int64_t B, int64_t T_, int H, int D, const void* q, const void* k, const void* v,
                        int64_t ld, void* o, int64_t ldo, float* lse, float scale, const DropArgs& d, hipStream_t st,
                        const int32_t* seg_start) {
    const dim3 grid(ceil_div(T_, GB), (unsigned)(B * H));
    with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        with_flag(seg_start != nullptr, [&](auto seg) {
            k_attn_fwd_generic<T, decltype(seg)::value><<<grid, 256, generic_lds<float>(D, 3, 1), st>>>(
                T_, H, D, (const T*)q, (const T*)k, (const T*)v, ld, (T*)o, ldo, lse, scale, d, seg_start);
        });
    });
}

void launch_bwd_generic(int dtype, int64_t B, int64_t T_, int H, int D, const void* q, const void* k, const void* v,
                        int64_t ld, const void* o, int64_t ldo, const void* dout, int64_t ldd, const float* lse,
                        float* delta, void* dq, void* dk, void* dv, int64_t lddqkv, float scale, const DropArgs& d,
                        hipStream_t st, const int32_t* seg_start, const int32_t* seg_end) {
    const dim3 grid(ceil_div(T_, GB), (unsigned)(B * H));
    with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const T *Q = (const T*)q, *K = (const T*)k, *V = (const T*)v, *DO = (const T*)dout;
        k_attn_delta<T><<<ceil_div(B * T_ * H, 256), 256, 0, st>>>(B, T_, H, D, (const T*)o, ldo, DO, ldd, delta);
        with_flag(seg_start != nullptr, [&](auto seg) {
            constexpr bool SEG = decltype(seg)::value;
            k_attn_dq_generic<T, SEG><<<grid, 256, generic_lds<float>(D, 4, 1), st>>>(
                T_, H, D, Q, K, V, ld, DO, ldd, lse, delta, (T*)dq, lddqkv, scale, d, seg_start);
            k_attn_dkdv_generic<T, SEG><<<grid, 256, generic_lds<float>(D, 4, 2), st>>>(
                T_, H, D, Q, K, V, ld, DO, ldd, lse, delta, (T*)dk, (T*)dv, lddqkv, scale, d, seg_end);
        });
    });
}
}  // namespace attn
}  // namespace cg

