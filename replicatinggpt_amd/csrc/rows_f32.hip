// charpt: the fp32 inference row kernels of generate() -- the fused FFN forward (k_ffn_f32) and the
// row-resident Linear with its LayerNorm inside (k_linear_f32q / k_linear_f32t) -- and their entry points
// cg_ffn_fwd_f32, cg_linear_rows_f32 and cg_decode_qkv_f32 (the last two run gemm_f32.hip's k_gemm_f32r
// for the per-token steps' few rows).
#include "gemm_common.h"
#include "ln_fwd.h"

using namespace cg;

namespace {

// ---------------------------------------------------------------------------------------
// Fused fp32 FFN forward for inference (FeedForward GPT1.py:142-147 in eval: no dropout) --
// generate()'s sliding-window blocks, M = 65536 rows of C = 126:
//     out = resid + (relu(a W1^T + b1) W2^T + b2),   a [M][C], W1 [H][C], W2 [C][H]
// without writing h (M x H fp32: 132 MB per launch at C5) to HBM and reading it back.  A block owns
// 128 rows, each wave 32 of them, and walks the hidden units in chunks of 32:
//   * GEMM 1 transposed, D[unit][row] = W1 a^T: its "B" operand is the wave's a rows, held in 64
//     registers for the whole block (xr[s] = a[row][2s + h] after one v_permlane32_swap per float2),
//     its "A" operand the chunk's 32 W1 rows (all of k) staged in LDS;
//   * D's accumulator layout puts the row on the lane and the hidden unit on the register, which is
//     GEMM 2's A-operand layout up to a pairing of k: two v_permlane32_swap per 8 hidden units
//     (below) make lane half 0 hold the even and half 1 the odd units, so h = relu(D + b1) feeds
//     out += h W2^T straight from registers; the chunk's 32 W2 columns are staged in LDS.
// Each chunk is two 64-MFMA slices per wave (W1, then W2) through a 2-stage LDS ring -- the next
// slice loaded to registers during the current one's MFMAs, one barrier per slice; biases in LDS.
// Bitwise the two-GEMM path (k_gemm_f32 / k_gemm_f32p BIAS_RELU then BIAS_RESID): every h element
// is the same k-ordered f32 fma chain over k < ceil16(C) plus b1 then max(., 0), every output the
// chain over hidden units < ceil16(H) (zero-padded h and W2 past H) plus b2 then resid + v
// (test_ffn_f32_fused_matches_two_gemms).  C <= 128 even, H <= 2048 even, lda / ldw1 / ldw2 even.
// The B operand of a transposed row GEMM held in registers for a whole block (k_ffn_f32 GEMM 1,
// k_linear_f32t): the wave's 32 rows of a [M][C] (C <= 128 even), xr[s] = a'[row mw + l32][2s + h]
// with a' = a or (LN) LayerNorm(a; ln_w, ln_b, eps) computed with k_ln_fwd's own row body --
// cg_layernorm_fwd's choice for C <= 128 even and 8-B aligned pointers, so the same bits -- through
// a per-wave scratch at the start of the caller's LDS ring (>= 4 x 16 x 130 floats; the LN form ends
// in a block barrier).
template <bool LN>
__device__ __forceinline__ void rows_b_operand(float (&xr)[64], float* ring, const float* __restrict__ a, int64_t lda,
                                               int64_t M, int C, int64_t mw, const float* __restrict__ ln_w,
                                               const float* __restrict__ ln_b, float eps, int lane, int w) {
    const int h = lane >> 5, l32 = lane & 31;
    if constexpr (LN) {
        // a = LayerNorm(x; ln_w, ln_b) of the wave's rows, with k_ln_fwd's own row body (ln_fwd.h
        // ln_fwd_row: one wave per row, lane l holding elements 2l, 2l+1) -- the same bits -- into a
        // per-wave LDS scratch in the ring (16 rows per pass, row stride 130 floats), read back in
        // GEMM 1's B-operand layout: xr[s] = a[row][2s + h]
        constexpr int LDR = 130;
        float* scr = ring + w * 16 * LDR;
        const float invC = 1.0f / (float)C;
        float wv[1][2] = {{0.f, 0.f}}, bv[1][2] = {{0.f, 0.f}};
        if (2 * lane < C) {
            wv[0][0] = ln_w[2 * lane], wv[0][1] = ln_w[2 * lane + 1];
            bv[0][0] = ln_b[2 * lane], bv[0][1] = ln_b[2 * lane + 1];
        }
        float v[32][1][2];   // all 32 rows in flight at once (one load latency, not two)
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int64_t row = mw + i < M ? mw + i : M - 1;
            const float2 t = *(const float2*)(a + row * lda + (2 * lane < C ? 2 * lane : 0));
            v[i][0][0] = 2 * lane < C ? t.x : 0.f;
            v[i][0][1] = 2 * lane < C ? t.y : 0.f;
        }
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float mu, rs;
                ln_fwd_row<2, 1, float, false>(v[16 * pass + i], wv, bv, C, invC, eps, lane, scr + i * LDR, mu, rs);
            }
            if ((l32 >> 4) == pass) {
#pragma unroll
                for (int s = 0; s < 64; ++s) {
                    const int k = 2 * s + h;
                    xr[s] = k < C ? scr[(l32 & 15) * LDR + k] : 0.f;
                }
            }
        }
        __syncthreads();   // the scratch is the caller's LDS ring
    } else {
        // the wave's a rows in GEMM 1's B-operand layout: lane (l32, h) loads a[row][4t + 2h, +1]; one
        // swap of h1's .x with h0's .y leaves xr[2t] = a[row][4t + h], xr[2t + 1] = a[row][4t + 2 + h]
        const int64_t row = mw + l32 < M ? mw + l32 : M - 1;
        const float* ar = a + row * lda;
        float2 v[32];
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const int k = 4 * t + 2 * h;
            v[t] = *(const float2*)(ar + (k < C ? k : C - 2));
            if (k >= C) v[t] = make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[t].x), __float_as_uint(v[t].y), false,
                                                            false);
            xr[2 * t] = __uint_as_float(r[0]);
            xr[2 * t + 1] = __uint_as_float(r[1]);
        }
    }

}

constexpr int FFN_LD1 = 33, FFN_LD2 = 132, FFN_STAGE = 32 * FFN_LD2;   // W1 [128 k][32 + 1], W2 [32 unit][128 + 4]

template <bool LN>
__global__ __launch_bounds__(256, 2) void k_ffn_f32(int64_t M, int C, int H, const float* __restrict__ a, int64_t lda,
                                                    const float* __restrict__ w1, int64_t ldw1,
                                                    const float* __restrict__ b1, const float* __restrict__ w2,
                                                    int64_t ldw2, const float* __restrict__ b2,
                                                    const float* resid, int64_t ldr, float* out, int64_t ldo,
                                                    const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                    float eps) {
    __shared__ __attribute__((aligned(16))) float sm[2][FFN_STAGE];   // 33.8 KB
    __shared__ float sb1[2048], sb2[128];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int64_t mw = (int64_t)blockIdx.x * 128 + 32 * w;   // the wave's first row
    const int kpad1 = (C + 15) / 16 * 16, kpad2 = (H + 15) / 16 * 16;
    const int nc = (H + 31) / 32;
    for (int i = tid; i < H; i += 256) sb1[i] = b1[i];
    for (int i = tid; i < C; i += 256) sb2[i] = b2[i];

    // slice staging, 8 float2 per thread.  kind 0: W1 rows 32 c + (tid >> 6) + 4 i at k = 2 (tid & 63)
    // (a wave reads one 512-B row), stored [k][unit] with row stride FFN_LD1; kind 1: W2 rows
    // (tid >> 4) + 16 i at unit 32 c + 2 (tid & 15), stored [unit][column] with row stride FFN_LD2
    float2 ra[8];
    bool rk = true;
    auto load = [&](int c, int kind) {
        const float* base;
        int ld, rmax, k, kmax, r0, rs;
        if (kind == 0) {
            base = w1, ld = (int)ldw1, rmax = H, kmax = C, k = 2 * (tid & 63), r0 = 32 * c + (tid >> 6), rs = 4;
        } else {
            base = w2, ld = (int)ldw2, rmax = C, kmax = H, k = 32 * c + 2 * (tid & 15), r0 = tid >> 4, rs = 16;
        }
        rk = k < kmax;
        const int kc = rk ? k : kmax - 2;
#pragma unroll
        for (int i = 0; i < 8; ++i) {   // cg_ffn_fwd_f32 checks: rows * ld under 2^31
            const int r = r0 + rs * i < rmax ? r0 + rs * i : rmax - 1;
            ra[i] = *(const float2*)(base + (uint32_t)(r * ld + kc));
        }
    };
    auto store = [&](int st, int kind) {   // kind: the staged slice's (that of the step storing it)
        float* S = sm[st];
        const int LD = kind == 0 ? FFN_LD1 : FFN_LD2;
        const int kk = kind == 0 ? 2 * (tid & 63) : 2 * (tid & 15);
        const int r0 = kind == 0 ? tid >> 6 : tid >> 4, rs = kind == 0 ? 4 : 16;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int r = r0 + rs * i;
            S[kk * LD + r] = rk ? ra[i].x : 0.f;
            S[(kk + 1) * LD + r] = rk ? ra[i].y : 0.f;
        }
    };
    load(0, 0);   // the first W1 slice in flight under the a / LayerNorm prologue

    float xr[64];
    rows_b_operand<LN>(xr, &sm[0][0], a, lda, M, C, mw, ln_w, ln_b, eps, lane, w);

    int stc = 0;
    // one ring step: the staged slice (chunk c, kind) to LDS, barrier, the following slice's load;
    // returns the stage to compute from
    auto step = [&](int c, int kind) {
        const int st = stc & 1;
        ++stc;
        store(st, kind);
        __syncthreads();
        if (kind == 0) load(c, 1);
        else if (c + 1 < nc) load(c + 1, 0);
        return st;
    };

    fv16f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fv16f{};
    const int nst1 = kpad1 / 2;   // GEMM 1 k2-steps (<= 64)
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
        // GEMM 1: D (hidden units 32 c.., the wave's rows) over k: one accumulator chain
        fv16f D = fv16f{};
        {
            const float* S = sm[step(c, 0)] + h * FFN_LD1 + l32;
#pragma unroll
            for (int b = 0; b < 16; ++b) {   // 4 k2-steps per fragment batch
                if (4 * b >= nst1) break;
                float fa[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) fa[u] = S[2 * (4 * b + u) * FFN_LD1];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 4; ++u) D = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[u], xr[4 * b + u], D, 0, 0, 0);
            }
        }
        // h = relu(D + b1), zero past H; then lane half 0 takes the even, half 1 the odd hidden units:
        // register 4q + t holds unit 8q + t + 4h; swapping h1's 4q+0 with h0's 4q+1 and h1's 4q+2 with
        // h0's 4q+3 leaves h0 {8q+0, 8q+4, 8q+2, 8q+6}, h1 {8q+1, 8q+5, 8q+3, 8q+7}
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int hc = 32 * c + (r & 3) + 8 * (r >> 2) + 4 * h;
            float v = D[r];
            v += sb1[hc < H ? hc : 0];
            v = fmaxf(v, 0.f);
            D[r] = hc < H ? v : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            auto r0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(D[4 * q]), __float_as_uint(D[4 * q + 1]), false,
                                                       false);
            auto r1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(D[4 * q + 2]), __float_as_uint(D[4 * q + 3]),
                                                       false, false);
            D[4 * q] = __uint_as_float(r0[0]);
            D[4 * q + 1] = __uint_as_float(r0[1]);
            D[4 * q + 2] = __uint_as_float(r1[0]);
            D[4 * q + 3] = __uint_as_float(r1[1]);
        }
        // GEMM 2: acc[j] (output columns 32 j.., the wave's rows) over the chunk's units; k2-step s
        // reads register 4 (s >> 2) + {0, 2, 1, 3}[s & 3]
        {
            const float* S = sm[step(c, 1)] + h * FFN_LD2 + l32;
            const int nst = kpad2 - 32 * c >= 32 ? 16 : 8;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                if (2 * b >= nst) break;
                float fb[2][4];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) fb[u][j] = S[2 * (2 * b + u) * FFN_LD2 + 32 * j];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    constexpr int perm[4] = {0, 2, 1, 3};
                    const int sstep = 2 * b + u;
                    const float ha = D[4 * (sstep >> 2) + perm[sstep & 3]];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ha, fb[u][j], acc[j], 0, 0, 0);
                }
            }
        }
    }
    // out = resid + (acc + b2): lane column n = 32 j + l32, register r row (r & 3) + 8 (r >> 2) + 4 h;
    // every residual loaded before the first store (out may alias resid); residual rows / columns
    // clamped, not branched around, so the loads stay in flight together
    const int64_t mr = M - 1 - mw;   // the wave's last valid row offset
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = 32 * j + l32 < C ? 32 * j + l32 : C - 1;
        const float bb = sb2[n];
        float rv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t dm = (r & 3) + 8 * (r >> 2) + 4 * h;
            rv[r] = resid[(mw + (dm < mr ? dm : mr)) * ldr + n];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[j][r];
            v += bb;
            acc[j][r] = rv[r] + v;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = mw + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int n = 32 * j + l32;
            if (m < M && n < C) out[m * ldo + n] = acc[j][r];
        }
}

// ---------------------------------------------------------------------------------------
// Row-resident fp32 forward for K <= 128 (generate()'s window: the QKV product with its ln1
// inside, GPT1.py:111-112,163; the projection with its residual, :136): out[m][n] =
// epi(a'[m] . W[n]) with a' = a or LayerNorm(a) (rows_b_operand: the wave's 32 rows in 64 registers
// for the whole block, the LayerNorm with k_ln_fwd's row body).  Computed transposed, D[n][m] =
// W a'^T, 32 output columns per slice: the W slice (32 rows x all of K) through a 2-stage LDS ring,
// 64 MFMAs per wave per slice in one accumulator chain, then the slice's epilogue -- each lane holds
// 4 consecutive columns of its row per 8 (registers 4q..4q+3 = columns 8q + 4h + 0..3), stored as two
// float2 -- with its residuals loaded under the slice's MFMAs.  Same k-ordered f32 fma chain over
// ceil16(K) and the same beta-0 epilogue as k_gemm_f32 / k_gemm_f32p: bitwise
// (test_linear_rows_f32_matches_gemm).  K even <= 128, N even <= 2048.
template <bool LN, int EK, int NB>   // NB: 32-column blocks per slice (independent accumulator chains)
__global__ __launch_bounds__(256, 2) void k_linear_f32t(int64_t M, int C, int N, const float* __restrict__ a,
                                                        int64_t lda, const float* __restrict__ w, int64_t ldw,
                                                        const float* __restrict__ bias, const float* resid,
                                                        int64_t ldr, float* out, int64_t ldo,
                                                        const float* __restrict__ ln_w,
                                                        const float* __restrict__ ln_b, float eps) {
    constexpr int LDW = 32 * NB + 1;   // [128 k][32 NB + 1] per stage
    __shared__ __attribute__((aligned(16))) float sm[2][128 * LDW];
    __shared__ float sbias[2048];
    constexpr bool BIAS = EK == CG_EPI_BIAS || EK == CG_EPI_BIAS_RELU || EK == CG_EPI_BIAS_RESID;
    const bool hb = BIAS && bias, hr = EK == CG_EPI_BIAS_RESID && resid;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, l32 = lane & 31;
    const int64_t mw = (int64_t)blockIdx.x * 128 + 32 * wv;   // the wave's first row
    const int nst = (C + 15) / 16 * 8;                          // k2-steps over ceil16(K) (<= 64)
    const int nc = (N + 32 * NB - 1) / (32 * NB);
    if (hb)
        for (int i = tid; i < N; i += 256) sbias[i] = bias[i];
    // W slice c: rows 32 NB c + (tid >> 6) + 4 i, k = 2 (tid & 63) (a wave reads one row), stored [k][row]
    float2 ra[8 * NB];
    bool rk = true;
    auto load = [&](int c) {
        const int k = 2 * (tid & 63), r0 = 32 * NB * c + (tid >> 6);
        rk = k < C;
        const int kc = rk ? k : C - 2;
#pragma unroll
        for (int i = 0; i < 8 * NB; ++i) {   // cg_linear_rows_f32 checks: rows * ldw under 2^31
            const int r = r0 + 4 * i < N ? r0 + 4 * i : N - 1;
            ra[i] = *(const float2*)(w + (uint32_t)(r * (int)ldw + kc));
        }
    };
    auto store = [&](int st) {
        float* S = sm[st];
        const int kk = 2 * (tid & 63), r0 = tid >> 6;
#pragma unroll
        for (int i = 0; i < 8 * NB; ++i) {
            S[kk * LDW + r0 + 4 * i] = rk ? ra[i].x : 0.f;
            S[(kk + 1) * LDW + r0 + 4 * i] = rk ? ra[i].y : 0.f;
        }
    };
    load(0);   // in flight under the row / LayerNorm prologue
    float xr[64];
    rows_b_operand<LN>(xr, &sm[0][0], a, lda, M, C, mw, ln_w, ln_b, eps, lane, wv);
    const int64_t m = mw + l32;
    const int64_t mc = m < M ? m : M - 1;   // residual row, clamped (not branched around)
    int stc = 0;
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
        const int st = stc & 1;
        ++stc;
        store(st);   // stage st was last read two slices ago, before the previous slice's barrier
        __syncthreads();
        if (c + 1 < nc) load(c + 1);
        float2 rv[NB][4][2];
        if (hr) {
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int n = 32 * (NB * c + j) + 8 * q + 4 * h + 2 * e;
                        rv[j][q][e] = *(const float2*)(resid + mc * ldr + (n < N ? n : N - 2));
                    }
        }
        fv16f D[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) D[j] = fv16f{};
        const float* S = sm[st] + h * LDW + l32;
#pragma unroll
        for (int b = 0; b < 16; ++b) {   // 4 k2-steps per fragment batch
            if (4 * b >= nst) break;
            float fa[4][NB];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < NB; ++j) fa[u][j] = S[2 * (4 * b + u) * LDW + 32 * j];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    D[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[u][j], xr[4 * b + u], D[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int n = 32 * (NB * c + j) + 8 * q + 4 * h + 2 * e;
                    float v0 = D[j][4 * q + 2 * e], v1 = D[j][4 * q + 2 * e + 1];
                    if (hb) {
                        v0 += sbias[n < N ? n : 0];
                        v1 += sbias[n + 1 < N ? n + 1 : 0];
                    }
                    if (EK == CG_EPI_BIAS_RELU) {
                        v0 = fmaxf(v0, 0.f);
                        v1 = fmaxf(v1, 0.f);
                    }
                    if (hr) {
                        v0 = rv[j][q][e].x + v0;
                        v1 = rv[j][q][e].y + v1;
                    }
                    if (m < M && n < N) *(float2*)(out + m * ldo + n) = make_float2(v0, v1);
                }
    }
}

// 16-row form of rows_b_operand (v_mfma_f32_16x16x4_f32's B operand): the wave's rows mw..mw+15 of
// a [M][C] (C <= 128 even), lane l loading elements 2l, 2l+1 of each (k_ln_fwd's layout), LayerNorm in
// that layout where asked (k_ln_fwd's row body: the same bits), through a per-wave scratch [16][130]
// at the start of the caller's LDS ring, read back as xr[t] = a'[row mw + (l & 15)][4t + (l >> 4)];
// ends in a block barrier.
template <bool LN>
__device__ __forceinline__ void rows16_b_operand(float (&xr)[32], float* ring, const float* __restrict__ a,
                                                 int64_t lda, int64_t M, int C, int64_t mw,
                                                 const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                 float eps, int lane, int wv) {
    const int li = lane & 15, g = lane >> 4;
    {
        constexpr int LDR = 130;
        float* scr = ring + wv * 16 * LDR;
        float v[16][1][2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t row = mw + i < M ? mw + i : M - 1;
            const float2 t = *(const float2*)(a + row * lda + (2 * lane < C ? 2 * lane : 0));
            v[i][0][0] = 2 * lane < C ? t.x : 0.f;
            v[i][0][1] = 2 * lane < C ? t.y : 0.f;
        }
        if constexpr (LN) {
            const float invC = 1.0f / (float)C;
            float wl[1][2] = {{0.f, 0.f}}, bl[1][2] = {{0.f, 0.f}};
            if (2 * lane < C) {
                wl[0][0] = ln_w[2 * lane], wl[0][1] = ln_w[2 * lane + 1];
                bl[0][0] = ln_b[2 * lane], bl[0][1] = ln_b[2 * lane + 1];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float mu, rs;
                ln_fwd_row<2, 1, float, false>(v[i], wl, bl, C, invC, eps, lane, scr + i * LDR, mu, rs);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (2 * lane < C) *(float2*)(scr + i * LDR + 2 * lane) = make_float2(v[i][0][0], v[i][0][1]);
        }
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const int k = 4 * t + g;
            xr[t] = k < C ? scr[li * LDR + k] : 0.f;
        }
        __syncthreads();   // the scratch is the ring's first stage
    }
}

// The same Linear with 16-row waves on v_mfma_f32_16x16x4_f32 (k_gemm_f32's own instruction):
// 64-row blocks, 1,024 workgroups at C5 and four per CU (34 KB of LDS, <= 128 VGPRs), so four waves
// per SIMD instead of two, and two independent 16 x 16 accumulator chains per 32-column slice.  The
// wave's rows go through an LDS scratch (coalesced row loads, the LayerNorm with k_ln_fwd's row body
// where asked) and come back as the B operand xr[t] = a'[row li][4t + g] (lane li + 16 g).  D[j] holds
// output columns 32 c + 16 j + 4 g + r of row li: one float4 of consecutive columns per tile.  Same
// k-ordered fma chain over ceil16(K) and epilogue as k_gemm_f32: bitwise.
template <bool LN, int EK>
__global__ __launch_bounds__(256, 4) void k_linear_f32q(int64_t M, int C, int N, const float* __restrict__ a,
                                                        int64_t lda, const float* __restrict__ w, int64_t ldw,
                                                        const float* __restrict__ bias, const float* resid,
                                                        int64_t ldr, float* out, int64_t ldo,
                                                        const float* __restrict__ ln_w,
                                                        const float* __restrict__ ln_b, float eps) {
    __shared__ __attribute__((aligned(16))) float sm[2][FFN_STAGE];   // W slices [128 k][32 + 1]
    constexpr bool BIAS = EK == CG_EPI_BIAS || EK == CG_EPI_BIAS_RELU || EK == CG_EPI_BIAS_RESID;
    const bool hb = BIAS && bias, hr = EK == CG_EPI_BIAS_RESID && resid;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, g = lane >> 4;
    const int64_t mw = (int64_t)blockIdx.x * 64 + 16 * wv;   // the wave's first row
    const int nk4 = (C + 15) / 16 * 4;                         // k4-steps over ceil16(K) (<= 32)
    const int nc = (N + 31) / 32;
    float2 ra[8];
    bool rk = true;
    auto load = [&](int c) {
        const int k = 2 * (tid & 63), r0 = 32 * c + (tid >> 6);
        rk = k < C;
        const int kc = rk ? k : C - 2;
#pragma unroll
        for (int i = 0; i < 8; ++i) {   // cg_linear_rows_f32 checks: rows * ldw under 2^31
            const int r = r0 + 4 * i < N ? r0 + 4 * i : N - 1;
            ra[i] = *(const float2*)(w + (uint32_t)(r * (int)ldw + kc));
        }
    };
    auto store = [&](int st) {
        float* S = sm[st];
        const int kk = 2 * (tid & 63), r0 = tid >> 6;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            S[kk * FFN_LD1 + r0 + 4 * i] = rk ? ra[i].x : 0.f;
            S[(kk + 1) * FFN_LD1 + r0 + 4 * i] = rk ? ra[i].y : 0.f;
        }
    };
    load(0);
    float xr[32];
    rows16_b_operand<LN>(xr, &sm[0][0], a, lda, M, C, mw, ln_w, ln_b, eps, lane, wv);
    const int64_t m = mw + li;
    const int64_t mc = m < M ? m : M - 1;   // residual row, clamped (not branched around)
    int stc = 0;
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
        const int st = stc & 1;
        ++stc;
        store(st);   // stage st was last read two slices ago, before the previous slice's barrier
        __syncthreads();
        if (c + 1 < nc) load(c + 1);
        float2 rv[2][2];
        float2 bv[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int n = 32 * c + 16 * j + 4 * g + 2 * e, nn = n < N ? n : N - 2;
                if (hr) rv[j][e] = *(const float2*)(resid + mc * ldr + nn);
                if (hb) bv[j][e] = make_float2(bias[nn], bias[nn + 1]);
            }
        fv4 D[2] = {fv4{0.f, 0.f, 0.f, 0.f}, fv4{0.f, 0.f, 0.f, 0.f}};
        const float* S = sm[st] + g * FFN_LD1 + li;
#pragma unroll
        for (int b = 0; b < 8; ++b) {   // 4 k4-steps per fragment batch
            if (4 * b >= nk4) break;
            float fa[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 2; ++j) fa[u][j] = S[4 * (4 * b + u) * FFN_LD1 + 16 * j];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    D[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[u][j], xr[4 * b + u], D[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int n = 32 * c + 16 * j + 4 * g + 2 * e;
                float v0 = D[j][2 * e], v1 = D[j][2 * e + 1];
                if (hb) {
                    v0 += bv[j][e].x;
                    v1 += bv[j][e].y;
                }
                if (EK == CG_EPI_BIAS_RELU) {
                    v0 = fmaxf(v0, 0.f);
                    v1 = fmaxf(v1, 0.f);
                }
                if (hr) {
                    v0 = rv[j][e].x + v0;
                    v1 = rv[j][e].y + v1;
                }
                if (m < M && n < N) *(float2*)(out + m * ldo + n) = make_float2(v0, v1);
            }
    }
}

// M <= 2048: k_gemm_f32r (32 x 32 tiles, any N); above: k_linear_f32q / k_linear_f32t (N <= 2048 even)
bool linear_rows_f32_supported(int64_t M, int64_t N, int64_t K) {
    return M > 0 && K >= 2 && K <= 128 && K % 2 == 0 && N >= 1 &&
           (M <= 2048 || (N >= 2 && N <= 2048 && N % 2 == 0));
}

bool ffn_f32_supported(int64_t M, int64_t C, int64_t H) {
    return M > 0 && C >= 2 && C <= 128 && C % 2 == 0 && H >= 2 && H <= 2048 && H % 2 == 0;
}

}  // namespace

namespace cg {
int g_linear_rows_nb = 0;   // cg_set_tuning("linear_rows_nb"): 0 k_linear_f32q (16-row waves), 1 / 2 k_linear_f32t
}  // namespace cg

extern "C" int cg_linear_rows_f32_supported(int64_t M, int64_t N, int64_t K) {
    return linear_rows_f32_supported(M, N, K) ? 1 : 0;
}

extern "C" int cg_linear_rows_f32(int64_t M, int64_t N, int64_t K, const float* a, int64_t lda, const float* ln_w,
                                  const float* ln_b, float eps, const float* w, int64_t ldw, const float* bias, int relu,
                                  const float* resid, int64_t ldr, float* out, int64_t ldo, void* stream) {
    CG_REQUIRE(linear_rows_f32_supported(M, N, K),
               "cg_linear_rows_f32: unsupported shape M=%lld N=%lld K=%lld (K <= 128 even; above 2048 rows N <= 2048 even)",
               (long long)M, (long long)N, (long long)K);
    CG_REQUIRE(a && w && out, "cg_linear_rows_f32: null pointer");
    CG_REQUIRE(!relu || (bias && !resid), "cg_linear_rows_f32: relu needs a bias and no residual");
    CG_REQUIRE(!ln_w == !ln_b, "cg_linear_rows_f32: ln_w and ln_b both or neither");
    hipStream_t st = (hipStream_t)stream;
    const int kind = resid ? CG_EPI_BIAS_RESID : relu ? CG_EPI_BIAS_RELU : bias ? CG_EPI_BIAS : CG_EPI_STORE;
    if (M <= 2048) {
        // generate()'s per-token rows: k_gemm_f32r (the kernel cg_gemm runs there), the LayerNorm in its
        // prologue -- the bits of [cg_layernorm_fwd +] cg_gemm at any N
        CG_REQUIRE(lda >= K && lda % 2 == 0 && ldw >= K && ldw % 2 == 0 && ldo >= N && (!resid || ldr >= N),
                   "cg_linear_rows_f32: bad leading dimensions");
        CG_REQUIRE((((uintptr_t)a | (uintptr_t)w) & 7) == 0, "cg_linear_rows_f32: a, w must be 8-B aligned");
        // (the in-launch LayerNorm is k_ln_fwd's narrow-row body, cg_layernorm_fwd's choice only for 8-B
        // aligned x / w / b: with other ln_w / ln_b the two launches sum a row in another order)
        CG_REQUIRE(!ln_w || (((uintptr_t)ln_w | (uintptr_t)ln_b) & 7) == 0,
                   "cg_linear_rows_f32: ln_w / ln_b must be 8-B aligned");
        EpiArgs e{};
        e.kind = kind;
        e.bias = bias;
        e.resid = resid;
        e.ld_resid = ldr;
        launch_f32r(M, N, K, a, lda, w, ldw, out, ldo, e, ln_w, ln_b, eps, nullptr, st);
        CG_LAUNCH_CHECK("cg_linear_rows_f32");
        return CG_OK;
    }
    CG_REQUIRE(lda >= K && lda % 2 == 0 && ldw >= K && ldw % 2 == 0 && ldo >= N && ldo % 2 == 0 &&
                   (!resid || (ldr >= N && ldr % 2 == 0)) && N * ldw < ((int64_t)1 << 31),
               "cg_linear_rows_f32: bad leading dimensions");
    CG_REQUIRE((((uintptr_t)a | (uintptr_t)w | (uintptr_t)out | (uintptr_t)(resid ? resid : out)) & 7) == 0,
               "cg_linear_rows_f32: a, w, out, resid must be 8-B aligned");
    CG_REQUIRE(!ln_w || ((((uintptr_t)ln_w | (uintptr_t)ln_b) & 7) == 0 && lda == K),
               "cg_linear_rows_f32: ln_w / ln_b must be 8-B aligned and a dense (lda == K) with the LayerNorm");
    const dim3 grid((unsigned)((M + 127) / 128));
    // 16-row waves (k_linear_f32q: four waves per SIMD) by default; cg_set_tuning("linear_rows_nb", 1 / 2):
    // 32-row waves with one / two 32-column chains per slice -- 3.3 % / 5.4 % slower in generate
    // (profiles/r6_linear_rows_gen.txt)
    with_epi_kind(kind, ln_w != nullptr, [&](auto ek, auto ln) {
        constexpr int EK = decltype(ek)::value;
        constexpr bool LN = decltype(ln)::value;
#define KL(KERNEL_, GRID_) \
    KERNEL_<<<GRID_, 256, 0, st>>>(M, (int)K, (int)N, a, lda, w, ldw, bias, resid, ldr, out, ldo, ln_w, ln_b, eps)
        if (g_linear_rows_nb == 0) KL((k_linear_f32q<LN, EK>), dim3((unsigned)((M + 63) / 64)));
        else if (g_linear_rows_nb == 1) KL((k_linear_f32t<LN, EK, 1>), grid);
        else KL((k_linear_f32t<LN, EK, 2>), grid);
#undef KL
    });
    CG_LAUNCH_CHECK("cg_linear_rows_f32");
    return CG_OK;
}

extern "C" int cg_decode_qkv_f32(int64_t B, int64_t C, int64_t H, const float* x, int64_t ldx, const float* ln_w,
                                 const float* ln_b, float eps, const float* w, int64_t ldw, float* qkv, int64_t ldq,
                                 const int64_t* len_dev, int64_t Tmax, float* kcache, float* vcache, void* stream) {
    CG_REQUIRE(B > 0 && B <= 2048 && C >= 2 && C <= 128 && C % 2 == 0 && H > 0 && C % H == 0 && Tmax > 0,
               "cg_decode_qkv_f32: needs 0 < B <= 2048, C <= 128 even, H | C (B=%lld C=%lld H=%lld)", (long long)B,
               (long long)C, (long long)H);
    CG_REQUIRE(x && ln_w && ln_b && w && qkv && len_dev && kcache && vcache, "cg_decode_qkv_f32: null pointer");
    CG_REQUIRE(ldx >= C && ldx % 2 == 0 && ldw >= C && ldw % 2 == 0 && ldq >= 3 * C,
               "cg_decode_qkv_f32: bad leading dimensions");
    CG_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)ln_w | (uintptr_t)ln_b) & 7) == 0,
               "cg_decode_qkv_f32: x, w, ln_w, ln_b must be 8-B aligned");
    EpiArgs e{};
    e.kind = CG_EPI_STORE;
    const KvAppend kva{kcache, vcache, len_dev, C, H, C / H, Tmax};
    launch_f32r(B, 3 * C, C, x, ldx, w, ldw, qkv, ldq, e, ln_w, ln_b, eps, &kva, (hipStream_t)stream);
    CG_LAUNCH_CHECK("cg_decode_qkv_f32");
    return CG_OK;
}

extern "C" int cg_ffn_fwd_f32_supported(int64_t M, int64_t C, int64_t H) { return ffn_f32_supported(M, C, H) ? 1 : 0; }

extern "C" int cg_ffn_fwd_f32(int64_t M, int64_t C, int64_t H, const float* a, int64_t lda, const float* ln_w,
                              const float* ln_b, float eps, const float* w1, int64_t ldw1, const float* b1,
                              const float* w2, int64_t ldw2, const float* b2, const float* resid, int64_t ldr,
                              float* out, int64_t ldo, void* stream) {
    CG_REQUIRE(ffn_f32_supported(M, C, H),
               "cg_ffn_fwd_f32: unsupported shape M=%lld C=%lld H=%lld (C <= 128 even, H <= 2048 even)", (long long)M,
               (long long)C, (long long)H);
    CG_REQUIRE(a && w1 && b1 && w2 && b2 && resid && out, "cg_ffn_fwd_f32: null pointer");
    CG_REQUIRE(lda >= C && lda % 2 == 0 && ldw1 >= C && ldw1 % 2 == 0 && ldw2 >= H && ldw2 % 2 == 0 && ldr >= C &&
                   ldo >= C && (int64_t)H * ldw1 < ((int64_t)1 << 31) && C * ldw2 < ((int64_t)1 << 31),
               "cg_ffn_fwd_f32: bad leading dimensions");
    CG_REQUIRE((((uintptr_t)a | (uintptr_t)w1 | (uintptr_t)w2) & 7) == 0, "cg_ffn_fwd_f32: a, w1, w2 must be 8-B aligned");
    CG_REQUIRE(!ln_w == !ln_b, "cg_ffn_fwd_f32: ln_w and ln_b both or neither");
    // (k_ln_fwd's narrow-row body -- the one the in-launch LayerNorm repeats -- is cg_layernorm_fwd's
    // choice for C <= 128 even with 8-B aligned x / w / b)
    CG_REQUIRE(!ln_w || ((((uintptr_t)ln_w | (uintptr_t)ln_b) & 7) == 0 && lda == C),
               "cg_ffn_fwd_f32: ln_w / ln_b must be 8-B aligned and a dense (lda == C) with the LayerNorm");
    const dim3 grid((unsigned)((M + 127) / 128));
    if (ln_w)
        k_ffn_f32<true><<<grid, 256, 0, (hipStream_t)stream>>>(M, (int)C, (int)H, a, lda, w1, ldw1, b1, w2, ldw2, b2,
                                                                resid, ldr, out, ldo, ln_w, ln_b, eps);
    else
        k_ffn_f32<false><<<grid, 256, 0, (hipStream_t)stream>>>(M, (int)C, (int)H, a, lda, w1, ldw1, b1, w2, ldw2, b2,
                                                                 resid, ldr, out, ldo, nullptr, nullptr, 0.f);
    CG_LAUNCH_CHECK("cg_ffn_fwd_f32");
    return CG_OK;
}
