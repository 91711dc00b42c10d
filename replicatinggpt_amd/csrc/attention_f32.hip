// charpt: the fp32 MFMA attention forward for small heads (D <= 32), no dropout -- the eval /
// generate() path of the fp32 model (Head.forward, GPT1.py:109-123): the 64-query-block kernel and
// its sequence-resident form for T <= 256, bitwise equal.
#include "attention_common.h"

using namespace cg;

namespace {

// =====================================================================================
// fp32 MFMA forward for small heads (D <= 32, e.g. the as-shipped head_size 21), no dropout:
// the eval / generate path of the fp32 model.  v_mfma_f32_16x16x4_f32 (exact f32 products, f32
// accumulation).  Block = 4 waves x 16 queries; 64-key K/V tiles in LDS (zero-padded to DP4 / 32
// columns).  S^T = K Q^T puts the query on the lane column (softmax statistics lane-local + two
// shuffles); P^T is consumed straight from the S^T accumulator as the B operand of O^T = V^T P^T in
// the permuted key order {4g + s} (k-step s, lane group g), V read in the same order.
// =====================================================================================
__device__ __forceinline__ fv4 mfma_f32x4(float a, float b, fv4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// SEG (packed rows, k_attn_fwd_f32mfma_seg): keys before the lane's query's segment start are masked
// as well; a 64-key tile wholly masked for a query leaves its statistics alone (m_new == -inf guards).
template <int DP4, bool SEG>  // D padded to a multiple of 4 (<= 32)
__device__ __forceinline__ void fwd_f32mfma(int64_t T_, int H, int D, const float* __restrict__ q,
                                            const float* __restrict__ k, const float* __restrict__ v, int64_t ld,
                                            float* __restrict__ o, int64_t ldo, float* __restrict__ lse, float scale,
                                            const int32_t* __restrict__ seg_start) {
    constexpr int KS = DP4 / 4;           // k-steps of S^T
    constexpr int KLD = DP4 + 1, VLD = 33;
    __shared__ float Ks[64 * KLD];
    __shared__ float Vs[64 * VLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int bh = blockIdx.y, b = bh / H, h = bh % H;
    const int64_t qblk0 = (int64_t)blockIdx.x * 64;
    const int64_t qw0 = qblk0 + wave * 16;
    const int64_t qa = qw0 + li;                       // this lane's query (S^T column)
    const float* qb = q + (int64_t)b * T_ * ld + h * D;
    const float* kb = k + (int64_t)b * T_ * ld + h * D;
    const float* vb = v + (int64_t)b * T_ * ld + h * D;
    float qf[KS];                                      // Q^T B operand: Q[qa][4t + g]
#pragma unroll
    for (int t = 0; t < KS; ++t) {
        const int e = 4 * t + g;
        qf[t] = (qa < T_ && e < D) ? qb[qa * ld + e] : 0.f;
    }
    int64_t ss = 0;   // SEG: the first key this lane's query sees, clamped into [0, qa]
    if constexpr (SEG) {
        if (qa < T_) {
            ss = seg_start[(int64_t)b * T_ + qa];
            ss = ss < 0 ? 0 : (ss > qa ? qa : ss);
        }
    }
    fv4 oacc[2] = {fv4{0.f, 0.f, 0.f, 0.f}, fv4{0.f, 0.f, 0.f, 0.f}};
    float m_run = -INFINITY, l_run = 0.f;
    const int64_t qlast = (qblk0 + 63) < (T_ - 1) ? (qblk0 + 63) : (T_ - 1);
    const int nkv = (int)(qlast / 64) + 1;
    for (int kv = 0; kv < nkv; ++kv) {
        const int64_t k0 = (int64_t)kv * 64;
        __syncthreads();
        for (int i = tid; i < 64 * 32; i += 256) {
            const int r = i >> 5, e = i & 31;
            const int64_t key = k0 + r;
            const bool ok = key < T_ && e < D;
            if (e < DP4) Ks[r * KLD + e] = ok ? kb[key * ld + e] : 0.f;
            Vs[r * VLD + e] = ok ? vb[key * ld + e] : 0.f;
        }
        __syncthreads();
        if (qw0 >= T_ || k0 > qw0 + 15) continue;      // wave past the end / tile fully masked
        fv4 st[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            fv4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KS; ++t) c = mfma_f32x4(Ks[(16 * kt + li) * KLD + 4 * t + g], qf[t], c);
            st[kt] = c;
        }
        // lane: query qa, keys k0 + 16kt + 4g + r
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t key = k0 + 16 * kt + 4 * g + r;
                float x = st[kt][r] * scale;
                if (key > qa || key >= T_) x = -INFINITY;
                if constexpr (SEG) {
                    if (key < ss) x = -INFINITY;
                }
                st[kt][r] = x;
                mx = fmaxf(mx, x);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = m_new == -INFINITY ? 1.f : expf(m_run - m_new);
        float ps = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = st[kt][r] == -INFINITY ? 0.f : expf(st[kt][r] - m_new);
                st[kt][r] = p;
                ps += p;
            }
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        l_run = l_run * alpha + ps;
        m_run = m_new;
        oacc[0] *= alpha;
        oacc[1] *= alpha;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int key = 16 * kt + 4 * g + s;   // permuted order: k-step s, lane group g
#pragma unroll
                for (int et = 0; et < 2; ++et)
                    oacc[et] = mfma_f32x4(Vs[key * VLD + 16 * et + li], st[kt][s], oacc[et]);
            }
    }
    if (qa >= T_) return;
    // O^T accumulator: lane holds e = 16 et + 4g + r for query qa
    const float inv = 1.f / l_run;
    float* orow = o + ((int64_t)b * T_ + qa) * ldo + h * D;
#pragma unroll
    for (int et = 0; et < 2; ++et)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = 16 * et + 4 * g + r;
            if (e < D) orow[e] = oacc[et][r] * inv;
        }
    if (g == 0) lse[(int64_t)bh * T_ + qa] = m_run + logf(l_run);
}

template <int DP4>
__global__ __launch_bounds__(256) void k_attn_fwd_f32mfma(int64_t T_, int H, int D, const float* __restrict__ q,
                                                          const float* __restrict__ k, const float* __restrict__ v,
                                                          int64_t ld, float* __restrict__ o, int64_t ldo,
                                                          float* __restrict__ lse, float scale) {
    fwd_f32mfma<DP4, false>(T_, H, D, q, k, v, ld, o, ldo, lse, scale, nullptr);
}

template <int DP4>
__global__ __launch_bounds__(256) void k_attn_fwd_f32mfma_seg(int64_t T_, int H, int D, const float* __restrict__ q,
                                                              const float* __restrict__ k,
                                                              const float* __restrict__ v, int64_t ld,
                                                              float* __restrict__ o, int64_t ldo,
                                                              float* __restrict__ lse, float scale,
                                                              const int32_t* __restrict__ seg_start) {
    fwd_f32mfma<DP4, true>(T_, H, D, q, k, v, ld, o, ldo, lse, scale, seg_start);
}

// Sequence-resident form of k_attn_fwd_f32mfma for T <= 256 (the generate() window and the fp32
// model's eval forward): one 8-wave block per (b, h) stages every K / V row of the sequence in LDS
// once (the 64-query blocks above re-load the causal prefix: 10 tile loads per (b, h) at T = 256
// instead of 4, each behind its own barrier), then wave w runs 16-query groups w and 15 - w (equal
// causal work per wave) with the per-group arithmetic of k_attn_fwd_f32mfma unchanged -- the same
// MFMAs in the same order, the same online softmax over the same 64-key tiles -- so the outputs
// are bitwise those of the 64-query-block kernel.
#ifdef CG_F32RES_FASTEXP   // what-if build only (make fastexp): the hardware exp2 path, not bitwise
#define F32RES_EXP(x) __expf(x)
#else
#define F32RES_EXP(x) expf(x)
#endif
template <int DP4>
__global__ __launch_bounds__(512, 4) void k_attn_fwd_f32res(int64_t T_, int H, int D, const float* __restrict__ q,
                                                         const float* __restrict__ k, const float* __restrict__ v,
                                                         int64_t ld, float* __restrict__ o, int64_t ldo,
                                                         float* __restrict__ lse, float scale) {
    constexpr int KS = DP4 / 4;
    // V rows hold only the DP4 padded dimensions (the O^T MFMAs' dims DP4..31 read zeros): 51 KB of
    // LDS at DP4 = 24; the operand look-ahead's 93 VGPRs make it two blocks per CU
    constexpr int KLD = DP4 + 1, VLD = DP4 + 1;
    __shared__ float Ks[256 * KLD];
    __shared__ float Vs[256 * VLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, li = lane & 15;
    // XCD-contiguous (b, h): the dispatcher deals block i to XCD i % 8, so XCD x runs the x-th eighth of
    // the (b, h) range in order and a sequence's heads share its L2 -- each head reads 84 of a row's
    // 1512 B, so with the heads spread over 6 XCDs every row's lines came from HBM ~6 times (234 MB read
    // per launch against the 99 MB of q / k / v)
    const int nblk = (int)gridDim.x, id = (int)blockIdx.x, nq = nblk >> 3, nr = nblk & 7, xcd = id & 7;
    const int bh = (xcd < nr ? xcd * (nq + 1) : nr * (nq + 1) + (xcd - nr) * nq) + (id >> 3);
    const int b = bh / H, h = bh % H;
    const float* qb = q + (int64_t)b * T_ * ld + h * D;
    const float* kb = k + (int64_t)b * T_ * ld + h * D;
    const float* vb = v + (int64_t)b * T_ * ld + h * D;
    // every K / V element of the thread loaded before the first LDS write (a load-write loop waits
    // for each load in turn: 32 dependent round trips per thread before any MFMA)
    constexpr int NL = 256 * DP4 / 512;
    float kx[NL], vx[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int i = tid + 512 * u, r = i / DP4, e = i - r * DP4;
        const bool ok = r < T_ && e < D;
        kx[u] = ok ? kb[(int64_t)r * ld + e] : 0.f;
        vx[u] = ok ? vb[(int64_t)r * ld + e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int i = tid + 512 * u, r = i / DP4, e = i - r * DP4;
        Ks[r * KLD + e] = kx[u];
        Vs[r * VLD + e] = vx[u];
    }
    __syncthreads();
#pragma unroll 1
    for (int gi = 0; gi < 2; ++gi) {
        const int64_t qw0 = 16 * (gi == 0 ? wave : 15 - wave);
        if (qw0 >= T_) continue;
        const int64_t qa = qw0 + li;
        float qf[KS];
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            const int e = 4 * t + g;
            qf[t] = (qa < T_ && e < D) ? qb[qa * ld + e] : 0.f;
        }
        fv4 oacc[2] = {fv4{0.f, 0.f, 0.f, 0.f}, fv4{0.f, 0.f, 0.f, 0.f}};
        float m_run = -INFINITY, l_run = 0.f;
        const int nkv = (int)((qw0 + 15) / 64) + 1;   // the 64-key tiles with k0 <= qw0 + 15, in order
        // one 64-key tile.  FULL: every key of the tile precedes the group's first query (and T) -- no
        // causal mask, no -inf scores, all four 16-key sub-tiles: the same arithmetic with the masking
        // compares, the -inf tests and the sub-tile guards compiled out (int32 indices), bitwise equal
        auto tile = [&](int kv, auto fullc) {
            constexpr bool FULL = decltype(fullc)::value;
            const int k0 = kv * 64;
            const float* Kt = Ks + k0 * KLD;
            const float* Vt = Vs + k0 * VLD;
            // 16-key sub-tiles past the group's last query (k0 + 16 kt > qw0 + 15) are fully masked: their
            // scores are -inf, their p exact zeros, so their S and O MFMAs and softmax terms change
            // nothing (max with -inf, + 0, MFMA products all 0) -- skipped, the result bitwise the same
            const int nkt = FULL ? 4 : ((int)qw0 + 15 - k0) / 16 + 1 < 4 ? ((int)qw0 + 15 - k0) / 16 + 1 : 4;
            // operands read one 16-key sub-tile ahead of their MFMAs, unconditionally (rows < 256 of the
            // staged sequence): K for the S products, then V's first sub-tile under the softmax and
            // each next one under the current one's O MFMAs -- not one LDS round trip per MFMA
            auto rdk = [&](float (&kr)[KS], int kt) {
#pragma unroll
                for (int t = 0; t < KS; ++t) kr[t] = Kt[(16 * kt + li) * KLD + 4 * t + g];
            };
            auto rdv = [&](float (&vr)[4][2], int kt) {
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int et = 0; et < 2; ++et) {
                        const int e = 16 * et + li;
                        vr[s][et] = e < DP4 ? Vt[(16 * kt + 4 * g + s) * VLD + e] : 0.f;
                    }
            };
            fv4 st[4];
            float kr[2][KS];
            rdk(kr[0], 0);
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                if (kt < 3) rdk(kr[(kt + 1) & 1], kt + 1);
                __builtin_amdgcn_sched_barrier(0);
                fv4 c = {0.f, 0.f, 0.f, 0.f};
                if (kt < nkt) {
#pragma unroll
                    for (int t = 0; t < KS; ++t) c = mfma_f32x4(kr[kt & 1][t], qf[t], c);
                }
                st[kt] = c;
            }
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = k0 + 16 * kt + 4 * g + r;
                    float x = st[kt][r] * scale;
                    if constexpr (FULL) asm("" : "+v"(x));   // keep x * scale rounded: the masked path's
                    else if (key > (int)qa || key >= (int)T_) x = -INFINITY;   // select stops its fma with - m_new
                    st[kt][r] = x;
                    if (kt < nkt) mx = fmaxf(mx, x);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = m_new == -INFINITY ? 1.f : F32RES_EXP(m_run - m_new);
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (kt < nkt) {
                        const float p = (!FULL && st[kt][r] == -INFINITY) ? 0.f : F32RES_EXP(st[kt][r] - m_new);
                        st[kt][r] = p;
                        ps += p;
                    }
                }
            ps += __shfl_xor(ps, 16, 64);
            ps += __shfl_xor(ps, 32, 64);
            l_run = l_run * alpha + ps;
            m_run = m_new;
            oacc[0] *= alpha;
            oacc[1] *= alpha;
            float vr[2][4][2];
            rdv(vr[0], 0);
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                if (kt >= nkt) break;
                if (kt < 3) rdv(vr[(kt + 1) & 1], kt + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int et = 0; et < 2; ++et) oacc[et] = mfma_f32x4(vr[kt & 1][s][et], st[kt][s], oacc[et]);
            }
        };
        for (int kv = 0; kv < nkv; ++kv) {
            if (kv * 64 + 63 <= (int)qw0 && kv * 64 + 63 < (int)T_) tile(kv, std::true_type{});
            else tile(kv, std::false_type{});
        }
        if (qa >= T_) continue;
        const float inv = 1.f / l_run;
        float* orow = o + ((int64_t)b * T_ + qa) * ldo + h * D;
#pragma unroll
        for (int et = 0; et < 2; ++et)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 16 * et + 4 * g + r;
                if (e < D) orow[e] = oacc[et][r] * inv;
            }
        if (g == 0) lse[(int64_t)bh * T_ + qa] = m_run + logf(l_run);
    }
}

// f(std::integral_constant<int, DP4>): D padded to the kernels' next instantiated multiple of 4
template <typename F>
void with_dp4(int D, F&& f) {
    const int dp4 = (D + 3) / 4 * 4;
    if (dp4 <= 8) f(std::integral_constant<int, 8>{});
    else if (dp4 <= 16) f(std::integral_constant<int, 16>{});
    else if (dp4 <= 24) f(std::integral_constant<int, 24>{});
    else f(std::integral_constant<int, 32>{});
}

}  // namespace

namespace cg {
namespace attn {
void launch_fwd_f32(int64_t B, int64_t T, int H, int D, const float* q, const float* k, const float* v, int64_t ld,
                    float* o, int64_t ldo, float* lse, float scale, hipStream_t st) {
    with_dp4(D, [&](auto dp) {
        // attn_variant 1 (A/B, tests): the 64-query-block kernel at T <= 256 too
        if (T <= 256 && g_attn_variant != 1)
            k_attn_fwd_f32res<decltype(dp)::value><<<(unsigned)(B * H), 512, 0, st>>>(T, H, D, q, k, v, ld, o, ldo, lse,
                                                                                       scale);
        else
            k_attn_fwd_f32mfma<decltype(dp)::value><<<dim3(ceil_div(T, 64), (unsigned)(B * H)), 256, 0, st>>>(
                T, H, D, q, k, v, ld, o, ldo, lse, scale);
    });
}
// packed rows: the 64-query-block kernel at every T (the sequence-resident form, bitwise its equal,
// takes no mask), so an all-zero seg_start gives launch_fwd_f32's bits
void launch_fwd_f32_seg(int64_t B, int64_t T, int H, int D, const float* q, const float* k, const float* v, int64_t ld,
                        float* o, int64_t ldo, float* lse, float scale, const int32_t* seg_start, hipStream_t st) {
    with_dp4(D, [&](auto dp) {
        k_attn_fwd_f32mfma_seg<decltype(dp)::value><<<dim3(ceil_div(T, 64), (unsigned)(B * H)), 256, 0, st>>>(
            T, H, D, q, k, v, ld, o, ldo, lse, scale, seg_start);
    });
}
}  // namespace attn
}  // namespace cg
