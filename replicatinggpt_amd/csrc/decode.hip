// charpt: batched autoregressive decode kernels for generate() (GPT1.py:196-212).
//
// The reference crops the context to the last block_size tokens and re-runs the full forward
// every step (positions are re-indexed from 0 after the crop, so once the window slides no K/V can
// be reused -- SURVEY Q7).  The decode engine (replicatinggpt_amd/decode.py) therefore runs
//   phase 1 (length <= block_size): one new token per step against a per-layer K/V cache
//            (cg_decode_kv_append + cg_decode_attn), positions identical to the full recompute;
//   phase 2 (sliding window): the full window forward (cg_decode_window gathers it), last row only
//            through ln_f / lm_head;
// and samples on the device (cg_decode_sample: argmax, or inverse-CDF sampling from a Philox
// stream; cg_decode_sample_filtered: that draw under a temperature, a top-k and a top-p cut read
// from device memory; cg_decode_emit: either, as the per-row epilogue of a ragged batch -- forced
// prompt tokens, stop tokens, per-row limits, log-probabilities).  Every step's shapes are static and the current length lives in device
// memory, so each phase is captured once as a hipGraph and replayed per token.  A prompt's shared positions
// are prefilled in one pass (cg_decode_prefill_attn: phase 1's attention for every position at once, the
// same arithmetic per position; cg_decode_logprob_rows: cg_decode_emit's log-prob for every scored column).
#include "common.h"

namespace cg {
int g_decode_attn_rows = 1;   // cg_set_tuning("decode_attn_rows"): 0 = k_decode_attn for every layout (A/B, tests)
}
namespace {
using namespace cg;

// out[b, j] = idx[b, start + j], start = max(0, len - T)  (len = *len_dev; idx row stride ld)
__global__ void k_decode_window(const int64_t* __restrict__ idx, int64_t ld, int64_t B, int64_t T,
                                const int64_t* __restrict__ len_dev, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * T) return;
    const int64_t b = i / T, j = i % T;
    const int64_t len = *len_dev;
    const int64_t start = len > T ? len - T : 0;
    out[i] = start + j < ld ? idx[b * ld + start + j] : 0;   // rows shorter than T: zero padding
}

// x[b, :] = wte[idx[b, pos]] + wpe[pos]   (pos = *len_dev - 1: the newest token)
__global__ void k_decode_embed(const int64_t* __restrict__ idx, int64_t ld, const float* __restrict__ wte,
                               const float* __restrict__ wpe, int64_t C, const int64_t* __restrict__ len_dev,
                               float* __restrict__ x, int64_t B) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C) return;
    const int64_t b = i / C, c = i % C;
    const int64_t pos = *len_dev - 1;
    x[i] = wte[idx[b * ld + pos] * C + c] + wpe[pos * C + c];
}

// K/V cache [B, H, Tmax, D]: row pos = *len_dev - 1 from the qkv rows (k at k_off, v at v_off)
__global__ void k_decode_kv_append(const float* __restrict__ qkv, int64_t ld, int64_t k_off, int64_t v_off,
                                   int64_t B, int64_t H, int64_t D, int64_t Tmax,
                                   const int64_t* __restrict__ len_dev, float* __restrict__ kc,
                                   float* __restrict__ vc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H * D) return;
    const int64_t b = i / (H * D), r = i % (H * D), h = r / D, e = r % D;
    const int64_t pos = *len_dev - 1;
    const int64_t dst = ((b * H + h) * Tmax + pos) * D + e;
    kc[dst] = qkv[b * ld + k_off + h * D + e];
    vc[dst] = qkv[b * ld + v_off + h * D + e];
}

// The per-query value chain of cg_decode_attn, shared by every kernel that must give its bits
// (k_decode_attn, k_decode_attn_rows, k_decode_prefill_attn).  One wave per query; a chunk is 64 keys,
// key 64 c + lane on lane `lane`, kv / vv that key's row padded with zeros to DP (ok: the key is one
// of the query's n).  attn_chunk: s as the fmaf chain over e < DP, s * scale, the online statistics
// (wave_max / __expf / wave_sum) and acc[e] = fmaf(p, v, acc[e] * alpha).  attn_finish: the output
// row, element e on lane e (a wave_sum_dpp per dimension, * (1 / l)).
template <int DP>
__device__ __forceinline__ void attn_chunk(const float (&qv)[DP], const float (&kv)[DP], const float (&vv)[DP], bool ok,
                                           float scale, float& m, float& l, float (&acc)[DP]) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < DP; ++e) s = fmaf(qv[e], kv[e], s);
    s = ok ? s * scale : -INFINITY;
    const float m_new = fmaxf(m, wave_max(s));
    const float alpha = __expf(m - m_new);
    const float p = ok ? __expf(s - m_new) : 0.f;
    l = l * alpha + wave_sum(p);
    m = m_new;
#pragma unroll
    for (int e = 0; e < DP; ++e) acc[e] = fmaf(p, vv[e], acc[e] * alpha);
}

template <int DP>
__device__ __forceinline__ float attn_finish(const float (&acc)[DP], float l, int64_t D, int lane) {
    const float inv = 1.f / l;
    float out = 0.f;
#pragma unroll
    for (int e = 0; e < DP; ++e) {
        if (e < D) {   // wave-uniform
            const float t = wave_sum_dpp(acc[e]);
            out = lane == e ? t * inv : out;
        }
    }
    return out;
}

// XCD-contiguous work order: block id runs on XCD id % 8, so work item xcd_contiguous(id, nblk) gives
// every XCD one contiguous run of the nblk items (the first nblk % 8 XCDs one item more).
__device__ __forceinline__ int64_t xcd_contiguous(int id, int nblk) {
    const int nq = nblk >> 3, nr = nblk & 7, xcd = id & 7;
    return (xcd < nr ? xcd * (nq + 1) : nr * (nq + 1) + (xcd - nr) * nq) + (id >> 3);
}

// one wave per (b, h): the newest query against cached keys 0..n-1 (causal by construction),
// scale = n_embd^-0.5.  Keys are spread over the lanes -- chunk c holds key 64 c + lane
// -- and each lane keeps its key's whole dot product and its own partial output row acc[0..D) (D
// padded to DP at compile time): a chunk's softmax statistics are two wave reductions (online over
// chunks), every K / V element load of a chunk is independent, and the output row is one DPP wave
// sum per dimension at the end.  (The previous form put 4 lanes on a key and accumulated V with a
// serial 16-step __shfl + dependent-load loop per chunk, and its vector loads needed D == 64: 73 us
// per call for the C5 model's head size 21, 10 % of generate().)
// K/V element (b, h, key j, e) at base + b*sb + h*sh + j*sj + e: the [B, H, Tmax, D] cache
// (sb = H*Tmax*D, sh = Tmax*D, sj = D) or the rows of a window's qkv buffer (sb = T*ld, sh = D, sj = ld).
template <int DP>
__global__ __launch_bounds__(256) void k_decode_attn(const float* __restrict__ q, int64_t ldq,
                                                     const float* __restrict__ kc, const float* __restrict__ vc,
                                                     int64_t sb, int64_t sh, int64_t sj, int64_t B, int64_t H,
                                                     int64_t D, const int64_t* __restrict__ len_dev, int64_t nfix,
                                                     float scale, float* __restrict__ o, int64_t ldo) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t bh = (int64_t)blockIdx.x * 4 + w;
    if (bh >= B * H) return;
    const int64_t b = bh / H, h = bh % H;
    const int64_t n = len_dev ? *len_dev : nfix;  // keys 0..n-1
    const float* K = kc + b * sb + h * sh;
    const float* V = vc + b * sb + h * sh;
    float qv[DP], acc[DP];
#pragma unroll
    for (int e = 0; e < DP; ++e) {
        qv[e] = e < D ? q[b * ldq + h * D + e] : 0.f;
        acc[e] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int64_t c0 = 0; c0 < n; c0 += 64) {
        const int64_t j = c0 + lane;
        const bool ok = j < n;
        const float* kr = K + (ok ? j : 0) * sj;
        const float* vr = V + (ok ? j : 0) * sj;
        float kv[DP], vv[DP];
#pragma unroll
        for (int e = 0; e < DP; ++e) {   // every load of the chunk in flight together
            kv[e] = e < D ? kr[e] : 0.f;
            vv[e] = e < D ? vr[e] : 0.f;
        }
        attn_chunk<DP>(qv, kv, vv, ok, scale, m, l, acc);
    }
    const float out = attn_finish<DP>(acc, l, D, lane);
    if (lane < D) o[b * ldo + h * D + lane] = out;
}

// k_decode_attn for the phase-1 cache ([B, H, Tmax, D], key rows contiguous, 16-B aligned chunks): one
// 64-thread block per (b, h).  A lane-per-key load reads one float of each of 64 rows per instruction --
// D instructions per chunk and operand, each touching ~D/1.5 cache lines -- and the rows of 6 waves a CU
// holds do not stay in its L1 between those instructions: the kernel ran at 1.4 TB/s of K / V at 256 keys
// and its time grew with the line count per instruction (row stride 32 floats: 0.75 TB/s;
// tools/decode_attn_probe.py).  Here a chunk's 64 K and V rows (64 D contiguous floats each) are read as
// float4s, lane l taking float4 l + 64 r, the next chunk's loads issued before the current chunk's
// arithmetic, and staged through LDS so that each lane then reads its key's row (stride D: conflict-free
// for odd D).  Per lane the arithmetic is k_decode_attn's, value for value (a lane past the last key
// reads zero rows instead of key 0's: its p is 0 either way), so the output is bitwise the same.
// SJ: key rows sj floats apart (phase 2's last layer: the window's qkv rows, sj = 3 C) -- the chunk's
// floats read as dwords, lane l taking float l + 64 r of the chunk's 64 D (row (l + 64 r) / D), so an
// instruction spans ~64 / D rows instead of 64.
template <int DP, bool SJ = false>
__global__ __launch_bounds__(64) void k_decode_attn_rows(const float* __restrict__ q, int64_t ldq,
                                                         const float* __restrict__ kc, const float* __restrict__ vc,
                                                         int64_t sb, int64_t sh, int64_t sj, int64_t B, int64_t H,
                                                         int64_t D,
                                                         const int64_t* __restrict__ len_dev, int64_t nfix, float scale,
                                                         float* __restrict__ o, int64_t ldo) {
    constexpr int R4 = DP;   // float4s per lane per operand: 64 rows x DP floats / 4 / 64 lanes
    __shared__ float4 ks4[16 * DP], vs4[16 * DP];
    const float* ks = (const float*)ks4;
    const float* vs = (const float*)vs4;
    const int lane = threadIdx.x;
    // XCD-contiguous (b, h) (block i runs on XCD i % 8): a sequence's heads share one L2 -- with the
    // window's row-strided K / V (SJ) each head reads 84 B of every 1 KB row
    const int64_t bh = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int64_t b = bh / H, h = bh % H;
    const int64_t n = len_dev ? *len_dev : nfix;  // keys 0..n-1
    const float4* K4 = (const float4*)(kc + b * sb + h * sh);
    const float4* V4 = (const float4*)(vc + b * sb + h * sh);
    const int64_t f4 = 16 * D;   // float4s per 64-row chunk
    float qv[DP], acc[DP];
#pragma unroll
    for (int e = 0; e < DP; ++e) {
        qv[e] = e < D ? q[b * ldq + h * D + e] : 0.f;
        acc[e] = 0.f;
    }
    float4 kr[R4 / 4], vr[R4 / 4];
    float kr1[SJ ? DP : 1], vr1[SJ ? DP : 1];
    const float* Kb = kc + b * sb + h * sh;
    const float* Vb = vc + b * sb + h * sh;
    int off[SJ ? DP : 1];   // SJ: float l + 64 r of a chunk at row * sj + e (INT_MAX: past the chunk)
    if constexpr (SJ) {
        int row = lane / (int)D, e = lane - row * (int)D;
        const int drow = 64 / (int)D, de = 64 - drow * (int)D;
#pragma unroll
        for (int r = 0; r < DP; ++r) {
            off[r] = lane + 64 * r < 64 * D ? row * (int)sj + e : INT_MAX;
            row += drow;
            e += de;
            if (e >= D) e -= (int)D, ++row;
        }
    }
    auto load = [&](int64_t c0) {
        if constexpr (SJ) {
            const int64_t rows = n - c0 < 64 ? n - c0 : 64;
            const int lim = (int)(rows * sj);   // offsets of the chunk's keys (e < D <= sj)
            const float* kb = Kb + c0 * sj;
            const float* vb = Vb + c0 * sj;
#pragma unroll
            for (int r = 0; r < DP; ++r) {
                const bool in = off[r] < lim;
                kr1[r] = in ? kb[off[r]] : 0.f;
                vr1[r] = in ? vb[off[r]] : 0.f;
            }
            return;
        }
        const int64_t lim = ((n - c0 < 64 ? n - c0 : 64) * D + 3) / 4;   // float4s holding the chunk's keys
#pragma unroll
        for (int r = 0; r < R4 / 4; ++r) {
            const int64_t i = lane + 64 * r;
            const bool in = i < f4 && i < lim;
            kr[r] = in ? K4[c0 / 4 * D + i] : float4{0.f, 0.f, 0.f, 0.f};
            vr[r] = in ? V4[c0 / 4 * D + i] : float4{0.f, 0.f, 0.f, 0.f};
        }
    };
    float m = -INFINITY, l = 0.f;
    load(0);
    for (int64_t c0 = 0; c0 < n; c0 += 64) {
        const int64_t cnt = (n - c0 < 64 ? n - c0 : 64) * D;   // floats of the chunk's keys
        __syncthreads();   // the previous chunk's rows are read (one wave: no wait for other waves)
        if constexpr (SJ) {
#pragma unroll
            for (int r = 0; r < DP; ++r) {
                const int64_t i = lane + 64 * r;
                if (i < 64 * D) {
                    ((float*)ks4)[i] = kr1[r];
                    ((float*)vs4)[i] = vr1[r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < (SJ ? 0 : R4 / 4); ++r) {
            const int64_t i = lane + 64 * r;
            if (i < f4) {
                float4 kx = kr[r], vx = vr[r];
                // a float4 straddling the last key: floats past it zero (key 0's floats in k_decode_attn
                // never reach a valid lane's row either way)
                const int64_t f = 4 * i;
                if (f + 4 > cnt) {
                    if (f + 0 >= cnt) kx.x = vx.x = 0.f;
                    if (f + 1 >= cnt) kx.y = vx.y = 0.f;
                    if (f + 2 >= cnt) kx.z = vx.z = 0.f;
                    if (f + 3 >= cnt) kx.w = vx.w = 0.f;
                }
                ks4[i] = kx;
                vs4[i] = vx;
            }
        }
        __syncthreads();
        if (c0 + 64 < n) load(c0 + 64);
        const int64_t j = c0 + lane;
        const bool ok = j < n;
        float kv[DP], vv[DP];
#pragma unroll
        for (int e = 0; e < DP; ++e) {
            kv[e] = e < D ? ks[lane * D + e] : 0.f;
            vv[e] = e < D ? vs[lane * D + e] : 0.f;
        }
        attn_chunk<DP>(qv, kv, vv, ok, scale, m, l, acc);
    }
    const float out = attn_finish<DP>(acc, l, D, lane);
    if (lane < D) o[b * ldo + h * D + lane] = out;
}

// One-pass prompt prefill (include/charpt.h cg_decode_prefill_attn): every position t < P of a (b, h) is
// one wave running k_decode_attn's chain with n = t + 1 keys, so its output row and the cache are what P
// per-token steps leave, bit for bit.  A block of QB waves owns positions t0 .. t0 + QB - 1 of one (b, h):
// it copies their K / V rows into the [B, H, Tmax, D] caches, and every 64-key chunk up to its last
// position is staged in LDS once (all 64 QB threads: float i = tid + 64 QB r of the chunk's 64 D, row
// i / D of the source at k + (b P + j) stride_kv + h D; the next chunk's loads issued before the current
// chunk's arithmetic) and read by all QB waves -- P^2 / (2 QB) K / V rows per (b, h) instead of P^2 / 2.
// LDS rows are DP + 1 floats apart: lane l reads row l, conflict-free for every D.  Keys past P are
// staged as zeros; a lane whose key is past its wave's own position takes a zero V row, as
// k_decode_attn_rows' lanes past n do (p is 0 there).  A wave skips the chunks past its position and a
// wave past P computes nothing, but both meet every barrier of the block's chunk loop.
// Work item bh * ceil(P / QB) + block-of-positions, XCD-contiguous: a (b, h)'s blocks share one L2.
template <int DP, int QB>
__global__ __launch_bounds__(64 * QB) void k_decode_prefill_attn(
    const float* __restrict__ q, int64_t stride_q, const float* __restrict__ k, const float* __restrict__ v,
    int64_t stride_kv, int64_t B, int64_t P, int64_t H, int64_t D, int64_t Tmax, float scale,
    float* __restrict__ kc, float* __restrict__ vc, float* __restrict__ o, int64_t stride_o) {
    constexpr int NT = 64 * QB, R = (64 * DP + NT - 1) / NT, DS = DP + 1;
    __shared__ float ks[64 * DS], vs[64 * DS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t nqb = (P + QB - 1) / QB;
    const int64_t item = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int64_t bh = item / nqb, t0 = (item - bh * nqb) * QB;
    const int64_t b = bh / H, h = bh - b * H;
    const int64_t t = t0 + w;                      // this wave's position
    const int64_t n = t < P ? t + 1 : 0;           // its keys 0..n-1 (0: a wave past the prompt)
    const float* Kb = k + b * P * stride_kv + h * D;
    const float* Vb = v + b * P * stride_kv + h * D;
    if (n > 0 && lane < D) {                       // the cache rows of the block's positions: exact copies
        const int64_t dst = ((b * H + h) * Tmax + t) * D + lane;
        kc[dst] = Kb[t * stride_kv + lane];
        vc[dst] = Vb[t * stride_kv + lane];
    }
    if (!q) return;                                // block-uniform: the cache-write-only form
    float qv[DP], acc[DP];
#pragma unroll
    for (int e = 0; e < DP; ++e) {
        qv[e] = n > 0 && e < D ? q[(b * P + t) * stride_q + h * D + e] : 0.f;
        acc[e] = 0.f;
    }
    const int64_t nblock = (t0 + QB < P ? t0 + QB : P);   // keys the block's last position sees
    const int cnt = 64 * (int)D;
    int row[R], col[R];                            // float tid + NT r of a chunk: (row, e), row 64 = past it
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + NT * r;
        row[r] = i < cnt ? i / (int)D : 64;
        col[r] = i < cnt ? i - row[r] * (int)D : 0;
    }
    float kr[R], vr[R];
    auto load = [&](int64_t c0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t j = c0 + row[r];
            const bool in = row[r] < 64 && j < P;
            kr[r] = in ? Kb[j * stride_kv + col[r]] : 0.f;
            vr[r] = in ? Vb[j * stride_kv + col[r]] : 0.f;
        }
    };
    float m = -INFINITY, l = 0.f;
    load(0);
    for (int64_t c0 = 0; c0 < nblock; c0 += 64) {   // block-uniform trip count
        __syncthreads();   // every wave has read the previous chunk's rows
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (row[r] < 64) {
                ks[row[r] * DS + col[r]] = kr[r];
                vs[row[r] * DS + col[r]] = vr[r];
            }
        }
        __syncthreads();
        if (c0 + 64 < nblock) load(c0 + 64);
        if (c0 < n) {      // wave-uniform: the chunk holds keys of this wave's query
            const bool ok = c0 + lane < n;
            float kv[DP], vv[DP];
#pragma unroll
            for (int e = 0; e < DP; ++e) {
                kv[e] = e < D ? ks[lane * DS + e] : 0.f;
                vv[e] = ok && e < D ? vs[lane * DS + e] : 0.f;
            }
            attn_chunk<DP>(qv, kv, vv, ok, scale, m, l, acc);
        }
    }
    if (n == 0) return;
    const float out = attn_finish<DP>(acc, l, D, lane);
    if (lane < D) o[(b * P + t) * stride_o + h * D + lane] = out;
}

// (x, v) ahead of (best, bi) in torch.argmax's order: NaN counts as the maximum, the lower index
// wins among equals (so a row holding NaN yields its first NaN's index, never an index outside [0, V))
__device__ __forceinline__ bool argmax_ahead(float x, int v, float best, int bi) {
    if (x != x) return best == best || v < bi;
    return best == best && (x > best || (x == best && v < bi));
}

// The token k_decode_sample writes for one row, computed by one wave (lane = 0..63, every lane active);
// the return value is the token in lane 0 (cg_decode_emit's modes 0 and 1 call this too, so the two
// kernels agree by construction): greedy = first argmax (torch.argmax tie and NaN rule); else
// inverse-CDF sampling of softmax(row) with u = Philox(seed, stream = len)[b] / 2^32.
__device__ __forceinline__ int64_t choose_plain(const float* __restrict__ row, int64_t V, int greedy,
                                                const uint64_t* __restrict__ seed_dev, int64_t len, int64_t b,
                                                int lane) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
        const float x = row[v];
        if (argmax_ahead(x, v, best, bi)) { best = x; bi = v; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (argmax_ahead(ob, oi, best, bi)) { best = ob; bi = oi; }
    }
    int64_t tok = bi;
    if (!greedy) {
        float s = 0.f;
        for (int v = lane; v < V; v += 64) s += __expf(row[v] - best);
        s = wave_sum(s);
        const u32x4 r = philox_group(seed_dev ? *seed_dev : 0ull, (uint64_t)len, (uint64_t)b);
        const float u = (float)(r.x >> 8) * (1.0f / 16777216.0f) * s;  // 24-bit uniform in [0, s)
        // sequential inverse CDF in vocabulary order (lane 0; V is the 65-char vocabulary)
        if (lane == 0) {
            float c = 0.f;
            tok = V - 1;
            for (int v = 0; v < V; ++v) {
                c += __expf(row[v] - best);
                if (u < c) { tok = v; break; }
            }
        }
    }
    return tok;
}

// next token per row from logits [B, V] (choose_plain).
// Writes idx[b, len] (len = *len_dev) -- the caller then advances *len_dev.
__global__ __launch_bounds__(64) void k_decode_sample(const float* __restrict__ logits, int64_t ldl, int64_t V,
                                                      int64_t B, int greedy, const uint64_t* __restrict__ seed_dev,
                                                      const int64_t* __restrict__ len_dev,
                                                      int64_t* __restrict__ idx, int64_t ld) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const int lane = threadIdx.x;
    const int64_t len = *len_dev;
    const int64_t tok = choose_plain(logits + b * ldl, V, greedy, seed_dev, len, b, lane);
    if (lane == 0) idx[b * ld + len] = tok;
}

// k_decode_sample's draw with a temperature, a top-k cut and a nucleus (top-p) cut, all three read from
// device memory (params = {tau, k, p}: one captured graph serves every setting); the contract is
// include/charpt.h's.  One 256-thread block per row, V <= SAMPLE_VMAX, the row in LDS:
//   xs  the logits (padded to a float4 with -inf: a pad entry is ahead of nothing in the ranking);
//   wv  the weights exp((x - max) / tau) in vocabulary order, then the kept ones (dropped: +0);
//   ws  the weights in rank order (ws[rank[v]] = wv[v]).
// Thread t owns columns t + 256 j: its ranks stay in registers.  The rank of v is the number of
// columns ahead of it (greater, or equal with a lower index: argmax_ahead's order on rows without
// NaN), counted against the whole row read as broadcast float4s -- V^2 / 256 compares per thread,
// 17 float4 reads at V = 65; skipped when both cuts are off.  Wave 0 then sums the first k' ranked
// weights, finds the nucleus prefix with a 64-wide inclusive scan per chunk, and draws exactly as
// k_decode_sample does over wv: the lane-strided sum + wave_sum for S, lane 0's sequential scan in
// vocabulary order.  A dropped column adds +0 there, which changes no partial sum and so can never
// be the first column past the draw: with everything kept and tau = 1 (x / 1.0f is exact) the token
// is k_decode_sample's bit for bit.
constexpr int SAMPLE_VMAX = 1024;
// choose_filtered: the token for row b, valid in thread 0 (what other threads return is unspecified);
// every thread of the 256-thread block must call it (it holds block barriers).  k_decode_sample_filtered
// and cg_decode_emit's mode 2 both call it.
__device__ __forceinline__ int choose_filtered(const float* __restrict__ row, int V, const float* __restrict__ params,
                                               uint64_t seed, int64_t len, int64_t b) {
    constexpr int NT = 256, J = SAMPLE_VMAX / NT;
    __shared__ float4 xs4[SAMPLE_VMAX / 4], wv4[SAMPLE_VMAX / 4];
    __shared__ float ws[SAMPLE_VMAX];
    __shared__ int sh_keep, sh_last;
    float* xs = (float*)xs4;
    float* wv = (float*)wv4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int Vp = (V + 3) & ~3;
    const int nj = (V + NT - 1) / NT;   // column passes in use (1 up to V = 256)
    // every scalar the kernel needs is loaded beside the row (not one global round trip after another):
    // the caller reads len and the seed before the call
    const float tau = params[0], kf = params[1], p = params[2];
    for (int v = tid; v < Vp; v += NT) xs[v] = v < V ? row[v] : -INFINITY;
    if (tid == 0) sh_last = -1;
    __syncthreads();
    // the greedy token (k_decode_sample's loop), in every wave: block-uniform without a broadcast
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
        const float x = xs[v];
        if (argmax_ahead(x, v, best, bi)) { best = x; bi = v; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (argmax_ahead(ob, oi, best, bi)) { best = ob; bi = oi; }
    }
    if (best != best || best == INFINITY) return bi;   // a NaN or +inf in the row: the greedy rule's token
    const int kk = kf >= 1.f && kf < (float)V ? (int)kf : V;   // 0, k >= V (and NaN): top-k off
    const bool nucleus = p < 1.f;                                // p >= 1 (and NaN): top-p off
    const bool filtered = kk < V || nucleus;
    float w[J];
    int rank[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int v = tid + NT * j;
        w[j] = 0.f;
        rank[j] = 0;
        if (j < nj) {   // block-uniform
            const float x = v < V ? xs[v] : -INFINITY;
            w[j] = x == -INFINITY ? 0.f : __expf((x - best) / tau);
            if (v < Vp) wv[v] = w[j];
        }
    }
    int keep = V;
    if (filtered) {   // block-uniform
        if (tid < V) {   // a thread with no column skips the pass (its J columns are all past V)
            float xv[J];
#pragma unroll
            for (int j = 0; j < J; ++j) xv[j] = tid + NT * j < V ? xs[tid + NT * j] : INFINITY;
            for (int u = 0; u < Vp; u += 4) {
                const float4 q = xs4[u >> 2];
                const float xu[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    if (j < nj) {   // block-uniform
                        const int v = tid + NT * j;
#pragma unroll
                        for (int e = 0; e < 4; ++e)   // no short circuit: compares and bit operations, no branches
                            rank[j] += (int)((xu[e] > xv[j]) | ((xu[e] == xv[j]) & (u + e < v)));
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < J; ++j)
                if (tid + NT * j < V) ws[rank[j]] = w[j];   // ranks are a permutation of 0..V-1
        }
        __syncthreads();
        if (tid < 64) {
            float sk = 0.f;
            for (int r = lane; r < kk; r += 64) sk += ws[r];
            sk = wave_sum(sk);
            int n = kk;
            if (nucleus) {
                // the shortest rank-order prefix whose weight reaches p * S_k (at least one token)
                const float thr = p * sk;
                float carry = 0.f;
                for (int base = 0; base < kk; base += 64) {
                    const int r = base + lane;
                    float c = r < kk ? ws[r] : 0.f;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const float t = __shfl_up(c, o, 64);
                        if (lane >= o) c += t;
                    }
                    c += carry;
                    const unsigned long long hit = __ballot(r < kk && c >= thr);
                    if (hit) {   // wave-uniform
                        n = base + __ffsll(hit);
                        break;
                    }
                    carry = __shfl(c, 63, 64);
                }
            }
            if (lane == 0) sh_keep = n;
        }
        __syncthreads();
        keep = sh_keep;
        int last = -1;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int v = tid + NT * j;
            if (v < V) {
                if (rank[j] < keep) last = v;   // v grows with j
                else wv[v] = 0.f;
            }
        }
        if (last >= 0) atomicMax(&sh_last, last);
    }
    __syncthreads();
    if (tid >= 64) return 0;
    // the draw: k_decode_sample's sum pattern and sequential scan over the kept weights
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += wv[v];
    s = wave_sum(s);
    const u32x4 r = philox_group(seed, (uint64_t)len, (uint64_t)b);
    const float u = (float)(r.x >> 8) * (1.0f / 16777216.0f) * s;  // 24-bit uniform in [0, s)
    int tok = 0;
    if (lane == 0) {
        tok = filtered ? sh_last : V - 1;   // no column past the draw: the last kept one
        float c = 0.f;
        bool found = false;
        float4 next = wv4[0];
        for (int v = 0; v < Vp && !found; v += 4) {   // a float4 of weights per LDS read; pad weights are 0
            const float4 q = next;
            if (v + 4 < Vp) next = wv4[(v >> 2) + 1];   // in flight under this float4's additions
            const float wq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c += wq[e];
                if (!found && u < c) { tok = v + e; found = true; }
            }
        }
    }
    return tok;
}

__global__ __launch_bounds__(256) void k_decode_sample_filtered(const float* __restrict__ logits, int64_t ldl,
                                                                int V, int64_t B,
                                                                const float* __restrict__ params,
                                                                const uint64_t* __restrict__ seed_dev,
                                                                const int64_t* __restrict__ len_dev,
                                                                int64_t* __restrict__ idx, int64_t ld) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const int64_t len = *len_dev;
    const uint64_t seed = seed_dev ? *seed_dev : 0ull;
    const int tok = choose_filtered(logits + b * ldl, V, params, seed, len, b);
    if (threadIdx.x == 0) idx[b * ld + len] = tok;
}

// log softmax(row)[tok] over the raw logits (temperature 1, no cuts), by one wave: (x[tok] - m) - log of
// the sum of exp(x[v] - m), m the row maximum, fp32 (lane-strided partial sums, then wave_sum).  NaN for a
// row holding NaN or +inf, and for a tok outside [0, V) (a caller's prompt token: nothing is read there).
__device__ __forceinline__ float row_logprob(const float* __restrict__ row, int V, int64_t tok, int lane) {
    float m = -INFINITY;
    bool bad = false;
    for (int v = lane; v < V; v += 64) {
        const float x = row[v];
        bad |= x != x || x == INFINITY;
        m = fmaxf(m, x);
    }
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += __expf(row[v] - m);
    s = wave_sum(s);
    if (__ballot(bad) || tok < 0 || tok >= V) return __builtin_nanf("");
    return (row[tok] - m) - logf(s);
}

// The log-probs of a one-pass prefill (include/charpt.h cg_decode_logprob_rows): one wave per logits row
// b P + t, logprob[b, t + 1] = row_logprob of idx[b, t + 1] -- what k_decode_emit stores for that column
// when the row holds these logits.
__global__ __launch_bounds__(256) void k_decode_logprob_rows(const float* __restrict__ logits, int64_t stride_logits,
                                                             int V, int64_t B, int64_t P,
                                                             const int64_t* __restrict__ idx, int64_t stride_idx,
                                                             float* __restrict__ logprob, int64_t stride_logprob) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B * P) return;   // wave-uniform
    const int64_t b = r / P, t = r - b * P;
    const float lp = row_logprob(logits + r * stride_logits, V, idx[b * stride_idx + t + 1], lane);
    if (lane == 0) logprob[b * stride_logprob + t + 1] = lp;
}

// The ragged engine's per-row epilogue (include/charpt.h cg_decode_emit): one block per row, 64 threads
// (modes 0 and 1: choose_plain) or 256 (mode 2: choose_filtered), so an emitted token is the old
// samplers' by construction.  Every branch below is block-uniform; thread 0 does all the stores.
template <bool FILTERED>
__global__ __launch_bounds__(FILTERED ? 256 : 64) void k_decode_emit(
    const float* __restrict__ logits, int64_t ldl, int V, int64_t B, int greedy, const float* __restrict__ params,
    const uint64_t* __restrict__ seed_dev, const int64_t* __restrict__ len_dev,
    const int64_t* __restrict__ prompt_len, const int64_t* __restrict__ limit, int64_t* __restrict__ end,
    const uint64_t* __restrict__ stop_bits, const int64_t* __restrict__ pad_dev, int64_t* __restrict__ idx,
    int64_t ld, float* __restrict__ logprob) {
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const int tid = threadIdx.x;
    const int64_t n = *len_dev;
    const uint64_t seed = seed_dev ? *seed_dev : 0ull;
    const int64_t plen = prompt_len[b], lim = limit[b], ended = end[b];
    if (ended != 0) {   // an ended row: pad, log-prob 0
        if (tid == 0) {
            idx[b * ld + n] = *pad_dev;
            if (logprob) logprob[b * ld + n] = 0.f;
        }
        return;
    }
    const float* row = logits + b * ldl;
    const bool forced = n < plen;
    int64_t tok;
    if (forced) {
        tok = idx[b * ld + n];
    } else {
        if constexpr (FILTERED) tok = choose_filtered(row, V, params, seed, n, b);
        else tok = choose_plain(row, V, greedy, seed_dev, n, b, tid);
    }
    if (tid >= 64) return;
    if (!forced) tok = __shfl((int)tok, 0, 64);   // thread 0 holds it
    float lp = 0.f;
    if (logprob) lp = row_logprob(row, V, tok, tid);
    if (tid != 0) return;
    if (!forced) idx[b * ld + n] = tok;
    if (logprob) logprob[b * ld + n] = lp;
    if (!forced && ((stop_bits[tok >> 6] >> (tok & 63)) & 1ull)) end[b] = n + 1;
    else if (n + 1 == lim) end[b] = n + 1;
}

}  // namespace

extern "C" int cg_decode_window(const int64_t* idx, int64_t ld, int64_t B, int64_t T, const int64_t* len_dev,
                                int64_t* out, void* stream) {
    CG_REQUIRE(B > 0 && T > 0 && ld > 0, "cg_decode_window: bad sizes");
    k_decode_window<<<ceil_div(B * T, 256), 256, 0, (hipStream_t)stream>>>(idx, ld, B, T, len_dev, out);
    CG_LAUNCH_CHECK("cg_decode_window");
    return CG_OK;
}

extern "C" int cg_decode_embed(const int64_t* idx, int64_t ld, const float* wte, const float* wpe, int64_t C,
                               const int64_t* len_dev, float* x, int64_t B, void* stream) {
    CG_REQUIRE(B > 0 && C > 0, "cg_decode_embed: bad sizes");
    k_decode_embed<<<ceil_div(B * C, 256), 256, 0, (hipStream_t)stream>>>(idx, ld, wte, wpe, C, len_dev, x, B);
    CG_LAUNCH_CHECK("cg_decode_embed");
    return CG_OK;
}

extern "C" int cg_decode_kv_append(const float* qkv, int64_t ld, int64_t k_off, int64_t v_off, int64_t B, int64_t H,
                                   int64_t D, int64_t Tmax, const int64_t* len_dev, float* kcache, float* vcache,
                                   void* stream) {
    CG_REQUIRE(B > 0 && H > 0 && D > 0 && Tmax > 0, "cg_decode_kv_append: bad sizes");
    k_decode_kv_append<<<ceil_div(B * H * D, 256), 256, 0, (hipStream_t)stream>>>(qkv, ld, k_off, v_off, B, H, D,
                                                                                  Tmax, len_dev, kcache, vcache);
    CG_LAUNCH_CHECK("cg_decode_kv_append");
    return CG_OK;
}

extern "C" int cg_decode_attn(const float* q, int64_t ldq, const float* k, const float* v, int64_t sb, int64_t sh,
                              int64_t sj, int64_t B, int64_t H, int64_t D, const int64_t* len_dev, int64_t nkeys,
                              float scale, float* o, int64_t ldo, void* stream) {
    CG_REQUIRE(B > 0 && H > 0 && D > 0 && D <= 64, "cg_decode_attn: needs D <= 64");
    CG_REQUIRE(len_dev || nkeys > 0, "cg_decode_attn: needs at least one key");
    // contiguous, 16-B aligned key rows (the phase-1 cache): the coalesced-chunk kernel
    const bool rows = g_decode_attn_rows && D <= 24 && sj == D && sh % 4 == 0 && sb % 4 == 0 &&
                      ((uintptr_t)k & 15) == 0 && ((uintptr_t)v & 15) == 0;
    if (rows)
        k_decode_attn_rows<24><<<(unsigned)(B * H), 64, 0, (hipStream_t)stream>>>(q, ldq, k, v, sb, sh, sj, B, H, D,
                                                                                  len_dev, nkeys, scale, o, ldo);
    else if (g_decode_attn_rows && D <= 24 && sj >= D && sj < (1 << 24))   // key rows sj floats apart (a window's qkv rows)
        k_decode_attn_rows<24, true><<<(unsigned)(B * H), 64, 0, (hipStream_t)stream>>>(
            q, ldq, k, v, sb, sh, sj, B, H, D, len_dev, nkeys, scale, o, ldo);
    else if (D <= 24)
        k_decode_attn<24><<<ceil_div(B * H, 4), 256, 0, (hipStream_t)stream>>>(q, ldq, k, v, sb, sh, sj, B, H, D,
                                                                               len_dev, nkeys, scale, o, ldo);
    else
        k_decode_attn<64><<<ceil_div(B * H, 4), 256, 0, (hipStream_t)stream>>>(q, ldq, k, v, sb, sh, sj, B, H, D,
                                                                               len_dev, nkeys, scale, o, ldo);
    CG_LAUNCH_CHECK("cg_decode_attn");
    return CG_OK;
}

extern "C" int cg_decode_prefill_attn(const float* q, int64_t stride_q, const float* k, const float* v,
                                      int64_t stride_kv, int64_t B, int64_t P, int64_t H, int64_t D, int64_t Tmax,
                                      float scale, float* kcache, float* vcache, float* o, int64_t stride_o,
                                      void* stream) {
    // positions (waves) per block: 8, or 4 at DP = 64, whose 192 row registers per lane leave room for
    // one wave per SIMD
    const int QB = D <= 24 ? 8 : 4;
    CG_REQUIRE(B > 0 && H > 0 && D > 0 && Tmax > 0, "cg_decode_prefill_attn: bad sizes (B = %lld, H = %lld, D = %lld, "
               "Tmax = %lld)", (long long)B, (long long)H, (long long)D, (long long)Tmax);
    CG_REQUIRE(D <= 64, "cg_decode_prefill_attn: D = %lld, needs D <= 64", (long long)D);
    CG_REQUIRE(P >= 1 && P <= Tmax, "cg_decode_prefill_attn: P = %lld is outside 1..Tmax = %lld", (long long)P,
               (long long)Tmax);
    CG_REQUIRE(k && v && kcache && vcache, "cg_decode_prefill_attn: null k / v / kcache / vcache");
    CG_REQUIRE((q == nullptr) == (o == nullptr), "cg_decode_prefill_attn: q and o must both be given or both be NULL");
    CG_REQUIRE(stride_kv >= H * D && (!q || (stride_q >= H * D && stride_o >= H * D)),
               "cg_decode_prefill_attn: a row stride is below H * D = %lld", (long long)(H * D));
    CG_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)o) & 3) == 0,
               "cg_decode_prefill_attn: a pointer is not 4-B aligned");
    const int64_t nblk = B * H * ((P + QB - 1) / QB);
    CG_REQUIRE(nblk < (1ll << 31), "cg_decode_prefill_attn: B * H * ceil(P / %d) = %lld blocks is above the grid limit", QB,
               (long long)nblk);
    if (D <= 24)
        k_decode_prefill_attn<24, 8><<<(unsigned)nblk, 64 * 8, 0, (hipStream_t)stream>>>(
            q, stride_q, k, v, stride_kv, B, P, H, D, Tmax, scale, kcache, vcache, o, stride_o);
    else
        k_decode_prefill_attn<64, 4><<<(unsigned)nblk, 64 * 4, 0, (hipStream_t)stream>>>(
            q, stride_q, k, v, stride_kv, B, P, H, D, Tmax, scale, kcache, vcache, o, stride_o);
    CG_LAUNCH_CHECK("cg_decode_prefill_attn");
    return CG_OK;
}

extern "C" int cg_decode_logprob_rows(const float* logits, int64_t stride_logits, int64_t V, int64_t B, int64_t P,
                                      const int64_t* idx, int64_t stride_idx, float* logprob, int64_t stride_logprob,
                                      void* stream) {
    CG_REQUIRE(B > 0 && P > 0 && B * P < (1ll << 32), "cg_decode_logprob_rows: bad sizes (B = %lld, P = %lld)", (long long)B,
               (long long)P);
    CG_REQUIRE(V >= 1 && V <= INT_MAX, "cg_decode_logprob_rows: V = %lld is outside 1..%d", (long long)V, INT_MAX);
    CG_REQUIRE(stride_logits >= V, "cg_decode_logprob_rows: stride_logits = %lld is below V = %lld",
               (long long)stride_logits, (long long)V);
    CG_REQUIRE(stride_idx > P && stride_logprob > P, "cg_decode_logprob_rows: stride_idx = %lld / stride_logprob = %lld "
               "do not hold column P = %lld", (long long)stride_idx, (long long)stride_logprob, (long long)P);
    CG_REQUIRE(logits && idx && logprob, "cg_decode_logprob_rows: null pointer");
    k_decode_logprob_rows<<<ceil_div(B * P, 4), 256, 0, (hipStream_t)stream>>>(logits, stride_logits, (int)V, B, P, idx,
                                                                              stride_idx, logprob, stride_logprob);
    CG_LAUNCH_CHECK("cg_decode_logprob_rows");
    return CG_OK;
}

extern "C" int cg_decode_sample(const float* logits, int64_t ldl, int64_t V, int64_t B, int greedy,
                                const uint64_t* seed_dev, const int64_t* len_dev, int64_t* idx, int64_t ld,
                                void* stream) {
    CG_REQUIRE(B > 0 && V > 0, "cg_decode_sample: bad sizes");
    k_decode_sample<<<(unsigned)B, 64, 0, (hipStream_t)stream>>>(logits, ldl, V, B, greedy, seed_dev, len_dev, idx,
                                                                 ld);
    CG_LAUNCH_CHECK("cg_decode_sample");
    return CG_OK;
}

extern "C" int cg_decode_sample_filtered(const float* logits, int64_t ldl, int64_t V, int64_t B,
                                         const float* params_dev, const uint64_t* seed_dev, const int64_t* len_dev,
                                         int64_t* idx, int64_t ld, void* stream) {
    CG_REQUIRE(B > 0 && V > 0 && ldl >= V, "cg_decode_sample_filtered: bad sizes");
    CG_REQUIRE(V <= SAMPLE_VMAX, "cg_decode_sample_filtered: V = %lld is above the kernel's limit of %d",
               (long long)V, SAMPLE_VMAX);
    CG_REQUIRE(logits && params_dev && len_dev && idx, "cg_decode_sample_filtered: null pointer");
    k_decode_sample_filtered<<<(unsigned)B, 256, 0, (hipStream_t)stream>>>(logits, ldl, (int)V, B, params_dev,
                                                                           seed_dev, len_dev, idx, ld);
    CG_LAUNCH_CHECK("cg_decode_sample_filtered");
    return CG_OK;
}

extern "C" int cg_decode_emit(const float* logits, int64_t ldl, int64_t V, int64_t B, int mode, const float* params_dev,
                              const uint64_t* seed_dev, const int64_t* len_dev, const int64_t* prompt_len,
                              const int64_t* limit, int64_t* end, const uint64_t* stop_bits, const int64_t* pad_dev,
                              int64_t* idx, int64_t ld, float* logprob, void* stream) {
    CG_REQUIRE(B > 0 && ld > 0, "cg_decode_emit: bad sizes (B = %lld, ld = %lld)", (long long)B, (long long)ld);
    CG_REQUIRE(V >= 1 && V <= SAMPLE_VMAX, "cg_decode_emit: V = %lld is outside the kernel's range 1..%d", (long long)V,
               SAMPLE_VMAX);
    CG_REQUIRE(ldl >= V, "cg_decode_emit: ldl = %lld is below V = %lld", (long long)ldl, (long long)V);
    CG_REQUIRE(mode >= 0 && mode <= 2, "cg_decode_emit: mode = %d is not 0 (greedy), 1 (draw) or 2 (filtered draw)", mode);
    CG_REQUIRE(logits && len_dev && prompt_len && limit && end && stop_bits && pad_dev && idx,
               "cg_decode_emit: null pointer");
    CG_REQUIRE(mode != 2 || params_dev, "cg_decode_emit: mode 2 needs params_dev");
    if (mode == 2)
        k_decode_emit<true><<<(unsigned)B, 256, 0, (hipStream_t)stream>>>(logits, ldl, (int)V, B, 0, params_dev, seed_dev,
                                                                           len_dev, prompt_len, limit, end, stop_bits,
                                                                           pad_dev, idx, ld, logprob);
    else
        k_decode_emit<false><<<(unsigned)B, 64, 0, (hipStream_t)stream>>>(logits, ldl, (int)V, B, mode == 0, params_dev,
                                                                           seed_dev, len_dev, prompt_len, limit, end,
                                                                           stop_bits, pad_dev, idx, ld, logprob);
    CG_LAUNCH_CHECK("cg_decode_emit");
    return CG_OK;
}
