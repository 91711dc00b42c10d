// charpt: the fp32 MFMA GEMM kernels behind cg_gemm's exact (dtype="fp32") path and their launchers:
// k_gemm_f32 (128 x 64 tiles: any shape, layout and split), k_gemm_f32s / k_gemm_f32r (forward
// products with few rows) and the persistent k_gemm_f32p (forward products with many rows).
#include "gemm_common.h"
#include "ln_fwd.h"

using namespace cg;

namespace {

// ---------------------------------------------------------------------------------------
// fp32 MFMA GEMM (v_mfma_f32_16x16x4_f32: exact f32 products, f32 accumulation) -- the exact
// (dtype="fp32") model path: parity runs, the as-shipped fp32 training and generate() on
// model.pth.  128 x 64 block tile, BK = 16, 4 waves of 64 x 32; operand tiles staged k-major in
// LDS ([k][rows], so a fragment read is 16 consecutive floats) with the next K-tile prefetched
// into registers during the MFMAs; any M / N / K (masked), all four layouts, split-K slabs.
// ---------------------------------------------------------------------------------------
constexpr int FBM = 128, FBN = 64, FBKK = 16;

template <bool TR, int R>
struct F32Tile {
    static constexpr int PER = R * FBKK / 256;  // elements per thread
    float v[PER];
    __device__ __forceinline__ void load(const float* __restrict__ X, int64_t ld, int64_t r0, int64_t rmax,
                                         int64_t k0, int64_t kmax, int tid) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int lin = tid + 256 * i;
            int r, kk;
            if (!TR) { kk = lin % FBKK; r = lin / FBKK; }
            else { r = lin % R; kk = lin / R; }
            const int64_t gr = r0 + r, gk = k0 + kk;
            v[i] = (gr < rmax && gk < kmax) ? (TR ? X[gk * ld + gr] : X[gr * ld + gk]) : 0.f;
        }
    }
    __device__ __forceinline__ void store(float* Xs, int tid) const {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int lin = tid + 256 * i;
            int r, kk;
            if (!TR) { kk = lin % FBKK; r = lin / FBKK; }
            else { r = lin % R; kk = lin / R; }
            Xs[kk * (R + 4) + r] = v[i];
        }
    }
};

template <bool AT, bool BT>
__global__ __launch_bounds__(256, 2) void k_gemm_f32(int64_t M, int64_t N, int64_t K, const float* __restrict__ A,
                                                     int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                     float* __restrict__ C, int64_t ldc, EpiArgs epi, int split_k,
                                                     int64_t kchunk, float* __restrict__ ws) {
    __shared__ float As[FBKK * (FBM + 4)];
    __shared__ float Bs[FBKK * (FBN + 4)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 4, li = lane & 15;
    const int64_t tilesN = (N + FBN - 1) / FBN;
    const int64_t m0 = (int64_t)(blockIdx.x / tilesN) * FBM, n0 = (int64_t)(blockIdx.x % tilesN) * FBN;
    const int split = blockIdx.y;
    const int64_t kb = split * kchunk, ke = kb + kchunk < K ? kb + kchunk : K;
    fv4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = fv4{0.f, 0.f, 0.f, 0.f};
    F32Tile<AT, FBM> ta;
    F32Tile<BT, FBN> tb;
    ta.load(A, lda, m0, M, kb, ke, tid);
    tb.load(B, ldb, n0, N, kb, ke, tid);
    for (int64_t k0 = kb; k0 < ke; k0 += FBKK) {
        __syncthreads();
        ta.store(As, tid);
        tb.store(Bs, tid);
        __syncthreads();
        if (k0 + FBKK < ke) {
            ta.load(A, lda, m0, M, k0 + FBKK, ke, tid);
            tb.load(B, ldb, n0, N, k0 + FBKK, ke, tid);
        }
#pragma unroll
        for (int k4 = 0; k4 < FBKK / 4; ++k4) {
            const int kr = 4 * k4 + g;
            float a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[kr * (FBM + 4) + wm * 64 + 16 * i + li];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[kr * (FBN + 4) + wn * 32 + 16 * j + li];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    const int kind = epi.kind;
    if (split_k == 1 && epi.beta == 0.f &&
        (kind == CG_EPI_STORE || kind == CG_EPI_BIAS || kind == CG_EPI_BIAS_RELU || kind == CG_EPI_BIAS_RESID)) {
        // every operand of the tile's epilogue (bias, residual) loaded before its first store: loaded
        // per element (epi_scalar + store_out), each load waited for every earlier store too (vmcnt
        // counts both), one HBM round trip per output element of the lane.  Same arithmetic and
        // order as epi_scalar: bias added only when present, ReLU, then resid + v.
        const bool hb = kind != CG_EPI_STORE && epi.bias, hr = kind == CG_EPI_BIAS_RESID && epi.resid;
        float bv[2] = {0.f, 0.f}, rv[2][2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t n = n0 + wn * 32 + 16 * j + li;
            if (hb && n < N) bv[j] = epi.bias[n];
        }
        // row fragments in two halves (i = 0-1, 2-3): each half's residuals loaded before the previous
        // half's stores, one half's registers live at a time
        auto load_half = [&](int hf) {
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t m = m0 + wm * 64 + 16 * (2 * hf + ii) + 4 * g + r;
                        const int64_t n = n0 + wn * 32 + 16 * j + li;
                        rv[ii][j][r] = (hr && m < M && n < N) ? epi.resid[m * epi.ld_resid + n] : 0.f;
                    }
        };
        load_half(0);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 2 * hf + ii;
                        float v = acc[i][j][r];
                        if (hb) v += bv[j];
                        if (kind == CG_EPI_BIAS_RELU) v = fmaxf(v, 0.f);
                        if (hr) v = rv[ii][j][r] + v;
                        acc[i][j][r] = v;
                    }
            if (hf == 0) load_half(1);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 2 * hf + ii;
                        const int64_t m = m0 + wm * 64 + 16 * i + 4 * g + r;
                        const int64_t n = n0 + wn * 32 + 16 * j + li;
                        if (m < M && n < N) C[m * ldc + n] = acc[i][j][r];
                    }
        }
        return;
    }
    const uint64_t stream = (epi.kind == CG_EPI_BIAS_DROP_RESID && epi.thr) ? dropout_stream(epi.rng_call, epi.site) : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + wm * 64 + 16 * i + 4 * g + r;
                const int64_t n = n0 + wn * 32 + 16 * j + li;
                if (m < M && n < N) {
                    if (split_k > 1)
                        ws[((int64_t)split * M + m) * N + n] = acc[i][j][r];
                    else
                        store_out<float>(C, m * ldc + n, epi_scalar(epi, acc[i][j][r], m, n, N, stream), epi.beta);
                }
            }
}

// ---------------------------------------------------------------------------------------
// fp32 forward (NT) products with few rows (M <= 2048: generate()'s per-token steps, 256 rows) --
// k_gemm_f32's 128 x 64 tiles leave most CUs idle there and pay a global-load round trip per 16-deep
// K-step.  One wave per 32 x 32 tile: each 128-deep K chunk's operands (a lane's A / B values for 32
// k4-steps) are loaded straight to registers, all in flight together, then its MFMAs.  The same
// v_mfma_f32_16x16x4_f32 lane / k assignment, k order and zero-padded K (to a multiple of 16) as
// k_gemm_f32, and its epilogue arithmetic with the operands loaded before the stores: bitwise its
// result.
template <int EK>
__global__ __launch_bounds__(64) void k_gemm_f32s(int64_t M, int64_t N, int64_t K, const float* __restrict__ A,
                                                  int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                  float* __restrict__ C, int64_t ldc, EpiArgs epi) {
    const int lane = threadIdx.x & 63, g = lane >> 4, li = lane & 15;
    const int64_t m0 = (int64_t)blockIdx.x * 32, n0 = (int64_t)blockIdx.y * 32;
    const int64_t kpad = (K + 15) / 16 * 16;   // k_gemm_f32's padded depth
    fv4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i][0] = acc[i][1] = fv4{0.f, 0.f, 0.f, 0.f};
    const int64_t ra0 = m0 + li, ra1 = m0 + 16 + li, rb0 = n0 + li, rb1 = n0 + 16 + li;
    for (int64_t kc = 0; kc < kpad; kc += 128) {
        float a[2][32], b[2][32];
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const int64_t k = kc + 4 * t + g;
            const bool kin = k < K;
            a[0][t] = (kin && ra0 < M) ? A[ra0 * lda + k] : 0.f;
            a[1][t] = (kin && ra1 < M) ? A[ra1 * lda + k] : 0.f;
            b[0][t] = (kin && rb0 < N) ? B[rb0 * ldb + k] : 0.f;
            b[1][t] = (kin && rb1 < N) ? B[rb1 * ldb + k] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            if (kc + 4 * t < kpad) {   // wave-uniform: k_gemm_f32's k4-steps only
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][t], b[j][t], acc[i][j], 0, 0, 0);
            }
        }
    }
    constexpr bool BIAS = EK == CG_EPI_BIAS || EK == CG_EPI_BIAS_RELU || EK == CG_EPI_BIAS_RESID;
    const bool hb = BIAS && epi.bias, hr = EK == CG_EPI_BIAS_RESID && epi.resid;
    float bv[2] = {0.f, 0.f}, rv[2][2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t n = n0 + 16 * j + li;
        if (hb && n < N) bv[j] = epi.bias[n];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + 16 * i + 4 * g + r, n = n0 + 16 * j + li;
                rv[i][j][r] = (hr && m < M && n < N) ? epi.resid[m * epi.ld_resid + n] : 0.f;
            }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + 16 * i + 4 * g + r, n = n0 + 16 * j + li;
                float v = acc[i][j][r];
                if (hb) v += bv[j];
                if (EK == CG_EPI_BIAS_RELU) v = fmaxf(v, 0.f);
                if (hr) v = rv[i][j][r] + v;
                if (m < M && n < N) C[m * ldc + n] = v;
            }
}

// The same products with the whole K slab resident (K <= 624, even; 8-B aligned rows): one 4-wave block per
// 32 x 32 tile loads its 32 A rows and 32 B rows once (every float2 of the slab in flight together,
// coalesced along K) into LDS, then each wave runs its 16 x 16 fragment's MFMA chain from LDS.  k_gemm_f32s
// walked K in 128-deep register chunks, one load round trip each, on 32 waves for the C5 FFN2 (19 us).
// Same lane / k order, padded depth and epilogue as k_gemm_f32: bitwise its result.
// Every global load is unconditional at a clamped address (row M - 1, column K - 2), the zero selected
// after it: a guarded load compiles to an exec-masked branch that waits for its own load (64 dependent
// round trips per thread at K = 504).  The chain reads its operands from LDS one 4-step group ahead of
// the MFMAs (a wait every 2 MFMAs before).
// LN (U == 1, K <= 128): A' = LayerNorm(A; ln_w, ln_b, eps) in the launch -- wave rr holds rows rr + 4 s
// with lane l on columns 2l, 2l + 1, k_ln_fwd's own row layout, so each row goes through its row body
// (ln_fwd.h ln_fwd_row, cg_layernorm_fwd's choice for C <= 128 even) into the LDS slab: the same bits
// as cg_layernorm_fwd then this GEMM (generate()'s per-token ln1 + QKV, ln2 + FFN1, lnf + lm_head).
// KV (generate()'s per-token QKV product): columns C..3C-1 of each row also go to the layer's K / V
// caches [rows][H][Tmax][D] at position *len - 1 -- the same values cg_decode_kv_append copies.
template <int EK, int U, bool LN = false, bool KV = false>   // U = ceil(kpad / 128): float2 columns per thread and row
__global__ __launch_bounds__(256, 1) void k_gemm_f32r(int64_t M, int64_t N, int64_t K, const float* __restrict__ A,
                                                      int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                      float* __restrict__ C, int64_t ldc, EpiArgs epi,
                                                      const float* __restrict__ ln_w = nullptr,
                                                      const float* __restrict__ ln_b = nullptr, float eps = 0.f,
                                                      KvAppend kva = KvAppend{}) {
    static_assert(!LN || U == 1, "k_gemm_f32r: the LayerNorm form needs K <= 128");
    static_assert(!KV || EK == CG_EPI_STORE, "k_gemm_f32r: the K / V append goes with the plain store");
    extern __shared__ __attribute__((aligned(16))) float smr[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, li = lane & 15;
    const int kpad = (int)((K + 15) / 16 * 16);   // k_gemm_f32's padded depth
    const int KS = kpad + 4;                       // LDS row stride (floats)
    float* As = smr;
    float* Bs = smr + 32 * KS;
    const int64_t mb = (int64_t)blockIdx.x * 32, nb = (int64_t)blockIdx.y * 32;
    const int rr = tid >> 6, c = tid & 63;      // rows rr + 4 s, float2 columns c + 64 u
    const int Ki = (int)K;
    float2 av[8][U], bv[8][U];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int r = rr + 4 * s;
        const int64_t ra = mb + r < M ? mb + r : M - 1, rb = nb + r < N ? nb + r : N - 1;
        const float* ap = A + ra * lda;
        const float* bp = B + rb * ldb;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = 2 * (c + 64 * u), kc = k < Ki ? k : Ki - 2;   // K even: k + 1 < K as well
            av[s][u] = *(const float2*)(ap + kc);
            bv[s][u] = *(const float2*)(bp + kc);
        }
    }
    if constexpr (LN) {
        // rows past M normalise row M - 1 (their outputs are not stored); columns K..kpad-1 zero
        const int k = 2 * c;
        const float invC = 1.0f / (float)Ki;
        float wl[1][2] = {{0.f, 0.f}}, bl[1][2] = {{0.f, 0.f}};
        if (k < Ki) {
            wl[0][0] = ln_w[k], wl[0][1] = ln_w[k + 1];
            bl[0][0] = ln_b[k], bl[0][1] = ln_b[k + 1];
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int r = rr + 4 * s;
            float v[1][2] = {{k < Ki ? av[s][0].x : 0.f, k < Ki ? av[s][0].y : 0.f}};
            float mu, rs;
            ln_fwd_row<2, 1, float, false>(v, wl, bl, Ki, invC, eps, c, As + r * KS, mu, rs);
            if (k >= Ki && k < kpad) *(float2*)(As + r * KS + k) = make_float2(0.f, 0.f);
            if (k < kpad) *(float2*)(Bs + r * KS + k) = (k < Ki && nb + r < N) ? bv[s][0] : make_float2(0.f, 0.f);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int r = rr + 4 * s, k = 2 * (c + 64 * u);
                if (k < kpad) {
                    const float2 z = make_float2(0.f, 0.f);
                    *(float2*)(As + r * KS + k) = (k < Ki && mb + r < M) ? av[s][u] : z;
                    *(float2*)(Bs + r * KS + k) = (k < Ki && nb + r < N) ? bv[s][u] : z;
                }
            }
    }
    constexpr bool BIAS = EK == CG_EPI_BIAS || EK == CG_EPI_BIAS_RELU || EK == CG_EPI_BIAS_RESID;
    const bool hb = BIAS && epi.bias, hr = EK == CG_EPI_BIAS_RESID && epi.resid;
    const int i = w >> 1, j = w & 1;
    const int64_t m0 = mb + 16 * i, n = nb + 16 * j + li, nc = n < N ? n : N - 1;
    // the epilogue's operands in flight under the chain
    float bb = 0.f, rv[4] = {0.f, 0.f, 0.f, 0.f};
    if (hb) bb = epi.bias[nc];
    if (hr) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + 4 * g + r, mc = m < M ? m : M - 1;
            rv[r] = epi.resid[mc * epi.ld_resid + nc];
        }
    }
    __syncthreads();
    const float* ar = As + (16 * i + li) * KS + g;
    const float* br = Bs + (16 * j + li) * KS + g;
    fv4 acc = fv4{0.f, 0.f, 0.f, 0.f};
    const int nt = kpad / 4;   // a multiple of 4
    float pa[4], pb[4], qa[4], qb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        pa[u] = ar[4 * u];
        pb[u] = br[4 * u];
    }
    // the look-ahead reads are unconditional (clamped to the last group: no LDS op under a branch, so
    // each wait counts only the group the MFMAs need)
    for (int t0 = 0;; t0 += 8) {
        const int t1 = t0 + 4 < nt ? t0 + 4 : nt - 4, t2 = t0 + 8 < nt ? t0 + 8 : nt - 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            qa[u] = ar[4 * (t1 + u)];
            qb[u] = br[4 * (t1 + u)];
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead of the MFMAs
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[u], pb[u], acc, 0, 0, 0);
        if (t0 + 4 >= nt) break;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            pa[u] = ar[4 * (t2 + u)];
            pb[u] = br[4 * (t2 + u)];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[u], qb[u], acc, 0, 0, 0);
        if (t0 + 8 >= nt) break;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + 4 * g + r;
        float v = acc[r];
        if (hb) v += (n < N ? bb : 0.f);
        if (EK == CG_EPI_BIAS_RELU) v = fmaxf(v, 0.f);
        if (hr) v = ((m < M && n < N) ? rv[r] : 0.f) + v;
        if (m < M && n < N) C[m * ldc + n] = v;
        if constexpr (KV) {
            const int64_t pos = *kva.len - 1;   // a position outside the cache writes nothing
            if (m < M && n < N && n >= kva.C && pos >= 0 && pos < kva.Tmax) {
                const bool isv = n >= 2 * kva.C;
                const int64_t t = n - (isv ? 2 * kva.C : kva.C), h = t / kva.D, e = t - h * kva.D;
                (isv ? kva.vc : kva.kc)[((m * kva.H + h) * kva.Tmax + pos) * kva.D + e] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Persistent fp32 forward (NT) GEMM for many rows (M > 2048: generate()'s sliding-window products,
// M = 65536, N = 126-504, K = 126 / 504).  k_gemm_f32's 128 x 64 grid runs 2.4-3.2 rounds of
// 5 blocks per CU there (1024-4096 blocks), each block's 8-16 K-steps behind two barriers and its
// own prologue load, at ~55 % of the f32 MFMA rate (profiles/r5_gemm_f32_pmc.txt).  Here 2 blocks
// per CU own equal contiguous runs of 128 x 128 tiles (row-band-major: a run's tiles share the A row
// panel, read once into the XCD's L2), K in 32-deep steps through a 2-stage [k][row] LDS ring with
// one barrier per step, the next K-tile (or the next tile's first one) loaded to registers as float2
// along K during the current step's MFMAs, so the ring never drains at a tile seam.  4 waves of
// 64 x 64 = 2 x 2 v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation, 4 independent
// chains per wave).  An f32 MFMA accumulates as a k-ordered fma chain (cdna guide §3 'FP32-input
// MFMA'), so the 32x32x2 chain over k = 0..kpad-1 (kpad = K rounded up to 16, zero padding, the
// 32-deep step's second half skipped past kpad) is k_gemm_f32's 16x16x4 chain, and the epilogue is
// its beta-0 arithmetic: bitwise k_gemm_f32 (test_gemm_f32_persistent_matches_128x64_bitwise).
// Needs K even, lda / ldb even and 8-B aligned A / B (float2 loads).
constexpr int PBM = 128, PBN = 128, PBK = 32, PLD = PBM + 4;   // LDS row stride over k (floats)

template <int EK>
__global__ __launch_bounds__(256, 2) void k_gemm_f32p(int64_t M, int64_t N, int64_t K, const float* __restrict__ A,
                                                      int64_t lda, const float* __restrict__ B, int64_t ldb,
                                                      float* __restrict__ C, int64_t ldc, EpiArgs epi,
                                                      int wflags) {
    __shared__ __attribute__((aligned(16))) float sm[2][2][PBK * PLD];   // [stage][A | B][k][row]: 66 KB
#ifdef CG_F32P_WHATIF
    // diagnostic build only (make whatif; tools/f32p_whatif.py): pk_flags bit 4 skips the in-loop loads
    // after each tile's first K-step, bit 5 the MFMAs, bit 6 the epilogue stores -- timing only
    // bit 8: fragment reads only in each tile's first K-step (MFMAs on stale registers after it),
    // bit 9: LDS store + barrier only in each tile's first K-step
    const bool WI_NOLOAD = wflags & 16, WI_NOMFMA = wflags & 32, WI_NOEPI = wflags & 64, WI_NOREAD = wflags & 256,
               WI_NOSYNC = wflags & 512;
#else
    constexpr bool WI_NOLOAD = false, WI_NOMFMA = false, WI_NOEPI = false, WI_NOREAD = false, WI_NOSYNC = false;
#endif
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int wm = w >> 1, wn = w & 1;
    const int64_t tilesN = (N + PBN - 1) / PBN, ntiles = (M + PBM - 1) / PBM * tilesN;
    const int kpad = (int)((K + 15) / 16 * 16);
    const int nks = (kpad + PBK - 1) / PBK;
    const int64_t G = gridDim.x, bid = blockIdx.x;
    const int64_t t_begin = bid * ntiles / G, t_end = (bid + 1) * ntiles / G;
    // loads: rows lr + 16 i (i = 0..7) of the A and B tiles, k pair lc (a wave: 4 rows x 128 B).  Rows
    // past M / N read row M-1 / N-1 instead (they only reach outputs that are not stored), k past K reads
    // k = K-2 and is zeroed (the padded depth must add exact zeros) -- no branches around the loads.
    const int lr = tid >> 4, lc = tid & 15;
    const char* ta = nullptr;   // the tile's row m0 / n0 (wave-uniform), 32-bit byte offsets per lane
    const char* tb = nullptr;
    uint32_t oa[8], ob[8];
    auto rows_of = [&](int64_t m0, int64_t n0) {
        ta = (const char*)(A + m0 * lda);
        tb = (const char*)(B + n0 * ldb);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t ma = m0 + lr + 16 * i < M ? lr + 16 * i : M - 1 - m0;
            const int64_t nb = n0 + lr + 16 * i < N ? lr + 16 * i : N - 1 - n0;
            oa[i] = (uint32_t)(ma * lda * 4);
            ob[i] = (uint32_t)(nb * ldb * 4);
        }
    };
    float2 ra[8], rb[8];
    bool rk = true;   // the loaded k pair is inside K (else it is stored as zeros: a select at the LDS
                      // write, not a write to the load's registers, which would wait for the load)
    auto load = [&](int ks) {
        const int k = ks * PBK + 2 * lc;
        rk = k < (int)K;
        const uint32_t kc = 4u * (uint32_t)(rk ? k : (int)K - 2);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ra[i] = *(const float2*)(ta + (oa[i] + kc));
            rb[i] = *(const float2*)(tb + (ob[i] + kc));
        }
    };
    auto store = [&](int st) {
        float* As = sm[st][0];
        float* Bs = sm[st][1];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = lr + 16 * i;
            As[2 * lc * PLD + r] = rk ? ra[i].x : 0.f;
            As[(2 * lc + 1) * PLD + r] = rk ? ra[i].y : 0.f;
            Bs[2 * lc * PLD + r] = rk ? rb[i].x : 0.f;
            Bs[(2 * lc + 1) * PLD + r] = rk ? rb[i].y : 0.f;
        }
    };
    constexpr bool BIAS = EK == CG_EPI_BIAS || EK == CG_EPI_BIAS_RELU || EK == CG_EPI_BIAS_RESID;
    const bool hb = BIAS && epi.bias, hr = EK == CG_EPI_BIAS_RESID && epi.resid;
    // tile coordinates advance without division: a block's tiles are consecutive in row-band-major order
    int64_t tm = t_begin / tilesN, tn = t_begin - tm * tilesN;
    int stc = 0;
    if (t_begin < t_end) {
        rows_of(tm * PBM, tn * PBN);
        load(0);
    }
#pragma unroll 1
    for (int64_t t = t_begin; t < t_end; ++t) {
        const int64_t m0t = tm * PBM, n0t = tn * PBN;
        if (++tn == tilesN) {
            tn = 0;
            ++tm;
        }
        fv16f acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][0] = acc[i][1] = fv16f{};
#pragma unroll 1
        for (int ks = 0; ks < nks; ++ks) {
            const int st = stc & 1;
            ++stc;
            if (!WI_NOSYNC || ks == 0) {
                store(st);   // stage st was last read two steps ago, before the previous step's barrier
                __syncthreads();
            }
            if (ks + 1 < nks) {
                if (!WI_NOLOAD) load(ks + 1);
            } else if (t + 1 < t_end) {
                rows_of(tm * PBM, tn * PBN);
                load(0);
            }
            const float* As = sm[st][0] + h * PLD + 64 * wm + l32;
            const float* Bs = sm[st][1] + h * PLD + 64 * wn + l32;
            const bool full = kpad - ks * PBK > 16;   // wave-uniform: the step's second 16 k are inside kpad
            // a half step's fragments (8 k2-steps, 32 registers) read before its MFMAs: one LDS round
            // trip per 32 MFMAs instead of one per 4
            float fa[8][2], fb[8][2];
#pragma unroll
            for (int hs = 0; hs < 2; ++hs) {
                if ((hs == 1 && !full) || WI_NOMFMA) break;
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    if (WI_NOREAD && (ks > 0 || hs > 0)) break;
                    const int o = 2 * (8 * hs + s) * PLD;
                    fa[s][0] = As[o];
                    fa[s][1] = As[o + 32];
                    fb[s][0] = Bs[o];
                    fb[s][1] = Bs[o + 32];
                }
                __builtin_amdgcn_sched_barrier(0);   // keep the batch together (hipcc sinks each read to its MFMAs)
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][0], fb[s][0], acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][0], fb[s][1], acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][1], fb[s][0], acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][1], fb[s][1], acc[1][1], 0, 0, 0);
                }
            }
        }
        // epilogue (k_gemm_f32's beta-0 arithmetic): bias, ReLU, resid + v, per 32-row half i, the
        // half's residuals loaded before its stores.  Lane column
        // n = l32; register r holds row (r & 3) + 8 (r >> 2) + 4 h of the 32 x 32 fragment.
        const int64_t m0 = m0t + 64 * wm + 4 * h, n0 = n0t + 64 * wn + l32;
        float bv[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (hb && n0 + 32 * j < N) bv[j] = epi.bias[n0 + 32 * j];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float rv[2][16];
            if (hr) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t m = m0 + 32 * i + (r & 3) + 8 * (r >> 2), n = n0 + 32 * j;
                        rv[j][r] = (m < M && n < N) ? epi.resid[m * epi.ld_resid + n] : 0.f;
                    }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t m = m0 + 32 * i + (r & 3) + 8 * (r >> 2), n = n0 + 32 * j;
                    float v = acc[i][j][r];
                    if (hb) v += bv[j];
                    if (EK == CG_EPI_BIAS_RELU) v = fmaxf(v, 0.f);
                    if (hr) v = rv[j][r] + v;
                    if (m < M && n < N && !WI_NOEPI) C[m * ldc + n] = v;
                }
        }
    }
}

bool launch_f32p(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                 int64_t ldc, const EpiArgs& e, hipStream_t st) {
    // 96 forces this kernel at any M (tests); 98 / 97 leave the fp32 products to k_gemm_f32 / the small-M kernels
    if (g_gemm_variant == 98 || g_gemm_variant == 97 || e.beta != 0.f || (M <= 2048 && g_gemm_variant != 96) ||
        M <= 0 || N <= 0 || K <= 0 || K % 2 || lda % 2 || ldb % 2 || (((uintptr_t)A | (uintptr_t)B) & 7))
        return false;
    if (!f32_epi_kind(e.kind)) return false;
    // the kernel's 32-bit lane offsets within a 128-row tile (rows_of): 128 rows of lda floats under 4 GB
    if (lda >= ((int64_t)1 << 22) || ldb >= ((int64_t)1 << 22) || K >= ((int64_t)1 << 22)) return false;
    const int64_t ntiles = (M + PBM - 1) / PBM * ((N + PBN - 1) / PBN);
    const int64_t slots = 2 * (int64_t)gemm_cu_count();
    const unsigned grid = (unsigned)(ntiles < slots ? ntiles : slots);
    with_epi_kind(e.kind, [&](auto ek) {
        k_gemm_f32p<decltype(ek)::value><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, e, g_pk_flags);
    });
    return true;
}

// the small-M kernel's conditions (else k_gemm_f32); gemm_variant 98 forces k_gemm_f32,
// 97 k_gemm_f32s (A/B, tests)
bool launch_f32s(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                 int64_t ldc, const EpiArgs& e, hipStream_t st) {
    if (g_gemm_variant == 98 || e.beta != 0.f || M > 2048 || !f32_epi_kind(e.kind)) return false;
    if (g_gemm_variant != 97 && K >= 2 && K % 2 == 0 && (K + 15) / 16 * 16 <= 624 && lda % 2 == 0 && ldb % 2 == 0 &&
        (((uintptr_t)A | (uintptr_t)B) & 7) == 0) {
        launch_f32r(M, N, K, A, lda, B, ldb, C, ldc, e, nullptr, nullptr, 0.f, nullptr, st);
        return true;
    }
    const dim3 grid((unsigned)((M + 31) / 32), (unsigned)((N + 31) / 32));
    with_epi_kind(e.kind, [&](auto ek) {
        k_gemm_f32s<decltype(ek)::value><<<grid, 64, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, e);
    });
    return true;
}

}  // namespace

namespace cg {
// k_gemm_f32r's one launch site (cg_gemm's small-M products, cg_linear_rows_f32 at M <= 2048,
// cg_decode_qkv_f32): the grid, the LDS slab and the kernel form.  ln_w / ln_b: the LayerNorm prologue
// (K <= 128); kv: also the K / V append (with the LayerNorm and a plain store).  The callers check the
// kernel's conditions (K even, kpad <= 624, even lda / ldb, 8-B aligned A / B and ln_w / ln_b, a
// beta-0 epilogue kind).
void launch_f32r(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                 int64_t ldc, const EpiArgs& e, const float* ln_w, const float* ln_b, float eps, const KvAppend* kv,
                 hipStream_t st) {
    const int64_t kpad = (K + 15) / 16 * 16;
    const dim3 grid((unsigned)((M + 31) / 32), (unsigned)((N + 31) / 32));
    const size_t lds = (size_t)2 * 32 * (kpad + 4) * sizeof(float);
    if (kv) {
        k_gemm_f32r<CG_EPI_STORE, 1, true, true><<<grid, 256, lds, st>>>(M, N, K, A, lda, B, ldb, C, ldc, e, ln_w, ln_b,
                                                                        eps, *kv);
        return;
    }
    with_epi_kind(e.kind, [&](auto ek) {
        constexpr int EK = decltype(ek)::value;
#define KR(U_, LN_) \
    k_gemm_f32r<EK, U_, LN_><<<grid, 256, lds, st>>>(M, N, K, A, lda, B, ldb, C, ldc, e, ln_w, ln_b, eps)
        if (ln_w) {
            KR(1, true);
            return;
        }
        switch ((int)((kpad + 127) / 128)) {   // U: float2 columns per thread and row
            case 1: KR(1, false); break;
            case 2: KR(2, false); break;
            case 3: KR(3, false); break;
            case 4: KR(4, false); break;
            default: KR(5, false); break;
        }
#undef KR
    });
}

void launch_f32(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                const float* B, int64_t ldb, float* C, int64_t ldc, const EpiArgs& e, int split_k, float* ws,
                hipStream_t st) {
    if (!a_trans && !b_trans && split_k == 1 &&
        (launch_f32p(M, N, K, A, lda, B, ldb, C, ldc, e, st) || launch_f32s(M, N, K, A, lda, B, ldb, C, ldc, e, st)))
        return;
    int64_t kchunk = (K + split_k - 1) / split_k;
    kchunk = (kchunk + FBKK - 1) / FBKK * FBKK;
    dim3 grid((unsigned)(((M + FBM - 1) / FBM) * ((N + FBN - 1) / FBN)), (unsigned)split_k);
#define KF(at_, bt_) k_gemm_f32<at_, bt_><<<grid, 256, 0, st>>>(M, N, K, A, lda, B, ldb, C, ldc, e, split_k, kchunk, ws)
    if (!a_trans && !b_trans) KF(false, false);
    else if (!a_trans && b_trans) KF(false, true);
    else if (a_trans && !b_trans) KF(true, false);
    else KF(true, true);
#undef KF
}
}  // namespace cg
