// charpt: weight-stationary bf16 MFMA GEMM (gfx950) for the K <= 384 wide-N training products -- the QKV
// forward, the FFN1 forward (bias + ReLU + keep bits) and the FFN2 input gradient (ReLU-backward + b1
// column partials) of GPT1.py:111-112,143-145.
//
// k_gemm_pk stages both operands of every 128x128 item through LDS and is bound by how fast a CU fills
// its LDS (profiles/r6_gemm_fill_c2.txt); half of those bytes are weights, fetched again for every item.
// Here a block owns one 128-column panel of the output for the whole launch:
//  * each of its 8 waves holds 32 columns x K of weights in registers (K = 384: 96 VGPRs), loaded once
//    -- K-contiguous B straight from memory in the MFMA operand layout, transposed B once through LDS
//    with the ds_read_b64_tr_b16 fragment reads;
//  * the LDS ring (3 stages of 64 rows x K, LDS-DMA, two tiles in flight) carries activations only;
//  * per 64-row tile: one counted wait, one barrier, the full-K MFMA chain of the wave's 32 x 32 outputs
//    (waves: 2 row halves x 4 column groups), the epilogue in registers; the tile after next's DMA
//    instructions are issued between the K-tiles' MFMAs, before the epilogue's stores.
// Same MFMA instruction, operand roles (weights first) and ascending k order as k_gemm_pk, so every
// output bit is gemm_variant 9's.  Blocks are dealt panel-major after xcd_remap: the blocks of one row
// range (one per panel) are consecutive, so they share an XCD's L2 while they walk the same activations.
// No block waits on another, and the kernel hosts no deferred work (the stream's queue stays as it is).
#include "gemm_pk.h"

namespace cg {
// cg_set_tuning("gemm_ws", v): 1 routes the products ws_gemm_auto names to k_gemm_ws, 0 none; the per-product
// A/B arms 2 / 3 / 4 route only the plain-store / bias + ReLU / ReLU-backward ones
int g_gemm_ws = 1;
namespace {
using namespace gt;

long long g_ws_launches = 0;

constexpr int WS_NBUF = 3;          // ring stages: tiles t + 1 and t + 2 in flight while tile t is computed
constexpr int WS_KT_A = 64 * 64 * 2;    // one K-tile of a 64-row activation tile: [64][64] bf16, row-swizzled
constexpr int WS_KT_B = 64 * 128 * 2;   // one K-tile of the transposed weight panel: [64 k][128] bf16
constexpr int WS_XCHG = 8 * 1024;   // ReLU-backward: the lower row half's 16 bf16 per lane, 4 column groups
constexpr int WS_BITS = 1024;       // ReLU-backward: a tile's keep words, 64 rows x 4 words (one DMA instruction)
constexpr int WS_LPT = 1;           // activation DMA instructions per wave per K-tile
// the epilogue's output stores (two 16-B row segments per wave; every kind issues at least these, last)
constexpr int WS_STORES = 2;

constexpr int ws_lds_bytes(int nkt) { return WS_NBUF * nkt * WS_KT_A + WS_XCHG + WS_NBUF * WS_BITS; }

// two 16 x 16 fragments (columns nc .. nc+3 and nc+16 .. nc+19 of a lane's row, packed bf16 pairs x / y)
// as one 16-B row segment per lane: store_bf16_wide's exchange for a single fragment pair
__device__ __forceinline__ void store_pair(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bf16_t* C, int64_t ldc,
                                           int64_t m, int64_t nb, int q) {
    const int64_t col = nb + ((q & 1) ? 16 : 0) + ((q >> 1) ? 8 : 0);
    const auto sx = __builtin_amdgcn_permlane16_swap(x0, x1, false, false);
    const auto sy = __builtin_amdgcn_permlane16_swap(y0, y1, false, false);
    st_out16((uint4*)(C + m * ldc + col), make_uint4(sx[0], sy[0], sx[1], sy[1]));
}

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// BT: B is [K][N] (the input gradient's weight), else [N][K].  EK: CG_EPI_STORE, CG_EPI_BIAS_RELU (bias,
// and with bits the ReLU keep words: a wave's 32 columns are one word per row) or CG_EPI_RELU_BWD (keep
// words in, and with colpart the per-64-row column sums of the bf16-rounded outputs, in
// k_gemm_pk's order: rows 16 i + r of a lane summed i = 0..3, then the 16 lanes of a DPP row).
// NKT = K / 64.  M % 64 == 0, N % 128 == 0, gridDim.x >= N / 128.
template <bool BT, int EK, int NKT>
__global__ __launch_bounds__(512, 1) __attribute__((amdgpu_waves_per_eu(1, 2)))
void k_gemm_ws(int M, int N, const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ B, int64_t ldb,
               bf16_t* __restrict__ C, int64_t ldc, const float* __restrict__ bias, uint32_t* __restrict__ bits,
               int64_t ldw, float* __restrict__ colpart) {
    static_assert(NKT >= 1 && NKT <= 6, "K <= 384");
    constexpr int STAGE = NKT * WS_KT_A;
    static_assert(!BT || NKT * WS_KT_B <= (WS_NBUF - 1) * STAGE, "the transposed panel fits in stages 1..");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3, g = lane >> 4;
    const int npanels = N / 128, P = gridDim.x, bpp = P / npanels;
    const int lb = xcd_remap(blockIdx.x, P);
    const int panel = lb % npanels, rslot = lb / npanels;
    if (rslot >= bpp) return;
    // the M / 64 row tiles over the panel's bpp blocks: leftover tiles one each to the first blocks.  bpp is
    // rounded down, so P % npanels blocks stay idle (4 of 256 at N = 1152 and N = 1536), and the launch ends
    // with the blocks that got a leftover tile (M = 16384: 10 against 9 tiles at N = 1152, 13 against 12 at 1536)
    const int T = M / 64, base = T / bpp, rem = T % bpp;
    const int ntile = base + (rslot < rem ? 1 : 0);
    if (ntile == 0) return;
    const int tile0 = rslot * base + (rslot < rem ? rslot : rem);
    const int64_t n0 = (int64_t)panel * 128, nb = n0 + wc * 32;

    const uint32_t lds0 = lds_base(smem);
    char* const xchg = smem + WS_NBUF * STAGE;
    const uint32_t bits0 = lds0 + (uint32_t)(WS_NBUF * STAGE + WS_XCHG);
    DmaP<false, 64, 8, FBK> da;
    da.init(lda, wave, lane);
    // K-tile kt of this block's tile t into ring stage sg (each wave: one 1-KB instruction, 8 rows)
    auto issue_a = [&](int t, int kt, int sg) {
        const bf16_t* src = A + (int64_t)(tile0 + t) * 64 * lda + kt * FBK;
        da.issue1(src, 0, lds0 + (uint32_t)(sg * STAGE + kt * WS_KT_A), wave);
    };
    // tile t's keep words: lane l fetches row l's four words of this panel (wave 0 only)
    const uint32_t bits_off = (uint32_t)(lane * (int)ldw * 4);
    auto issue_bits = [&](int t, int sg) {
        if (EK == CG_EPI_RELU_BWD && wave == 0)
            dma16sl(bits + (int64_t)(tile0 + t) * 64 * ldw + panel * 4, bits_off, bits0 + (uint32_t)(sg * WS_BITS));
    };

    // ---- prologue: tile 0 on its way, then the wave's 32 x K weights into registers, then tile 1
    issue_bits(0, 0);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) issue_a(0, kt, 0);
    sv8 bw[NKT][2][2];   // [K-tile][32-deep half][16-column fragment]
    if constexpr (!BT) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    bw[kt][s][j] = *(const sv8*)(B + (nb + 16 * j + (lane & 15)) * ldb + kt * FBK + 32 * s + 8 * g);
    } else {
        DmaP<true, 128, 8, FBK> db;
        db.init(ldb, wave, lane);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                db.issue1(B + (int64_t)kt * FBK * ldb + n0, i, lds0 + (uint32_t)(STAGE + kt * WS_KT_B), wave);
        wait_vm<0>();
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    bw[kt][s][j] = frag<true, 128>(smem + STAGE + kt * WS_KT_B, wc * 32 + 16 * j, s, lane);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // every wave has its weights: stages 1.. are free for the ring
    }
    float4 bv[2];
    if constexpr (EK == CG_EPI_BIAS_RELU) {
#pragma unroll
        for (int j = 0; j < 2; ++j) bv[j] = *(const float4*)(bias + nb + 4 * g + 16 * j);
    }
    if (ntile > 1) {
        issue_bits(1, 1);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) issue_a(1, kt, 1);
    }

    // Vector-memory operations younger than tile t's DMAs when the loop head waits for them: tile t + 1's
    // (NKT per wave, if there is one) and tile t - 1's output stores (at least WS_STORES, the youngest).
    // Wave 0's keep-word DMA and any further epilogue store only make the count conservative.
    constexpr int LPT = NKT * WS_LPT;
    int sg = 0;
    for (int t = 0; t < ntile; ++t) {
        const bool more = t + 1 < ntile;
        if (t > 0) {
            if (more) wait_vm<LPT + WS_STORES>();
            else wait_vm<WS_STORES>();
        } else {
            if (more) wait_vm<LPT>();
            else wait_vm<0>();
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // tile t landed for every wave; tile t - 1's stage is free
        const bool pf = t + 2 < ntile;
        const int sg2 = sg == 0 ? 2 : sg - 1;   // stage of tile t + 2 (= tile t - 1's)
        const char* img = smem + sg * STAGE;
        if (pf) issue_bits(t + 2, sg2);

        fv4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = fv4{0.f, 0.f, 0.f, 0.f};
        // the row fragments of K-tile kt + 1 are read before K-tile kt's MFMAs (two register sets)
        sv8 af[2][2][2];
        auto read_a = [&](int kt) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    af[kt & 1][s][i] = frag<false, 64>(img + kt * WS_KT_A, wr * 32 + 16 * i, s, lane);
        };
        read_a(0);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt + 1 < NKT) read_a(kt + 1);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma_bf16(bw[kt][s][j], af[kt & 1][s][i], acc[i][j]);
            if (pf) issue_a(t + 2, kt, sg2);
        }

        // acc[i][j][q] = C[mr + 16 i][nb + 16 j + 4 g + q]
        const int64_t mr = (int64_t)(tile0 + t) * 64 + wr * 32 + (lane & 15);
        uint32_t px[2][2], py[2][2];
        if constexpr (EK == CG_EPI_BIAS_RELU) {
            uint32_t w[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    fv4& v = acc[i][j];
                    v[0] = fmaxf(v[0] + bv[j].x, 0.f); v[1] = fmaxf(v[1] + bv[j].y, 0.f);
                    v[2] = fmaxf(v[2] + bv[j].z, 0.f); v[3] = fmaxf(v[3] + bv[j].w, 0.f);
                    px[i][j] = pack_bf2(v[0], v[1]);
                    py[i][j] = pack_bf2(v[2], v[3]);
                }
                w[i] = (nz4_bf16(make_uint2(px[i][0], py[i][0])) << (4 * g)) |
                       (nz4_bf16(make_uint2(px[i][1], py[i][1])) << (16 + 4 * g));
                w[i] |= (uint32_t)__shfl_xor((int)w[i], 16, 64);
                w[i] |= (uint32_t)__shfl_xor((int)w[i], 32, 64);
            }
            // lane quarter g stores the word of its row in fragment row i = g
            if (bits && g < 2) bits[(mr + 16 * g) * ldw + (nb >> 5)] = g ? w[1] : w[0];
        } else if constexpr (EK == CG_EPI_RELU_BWD) {
            const char* bimg = smem + WS_NBUF * STAGE + WS_XCHG + sg * WS_BITS;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t w = *(const uint32_t*)(bimg + (wr * 32 + 16 * i + (lane & 15)) * 16 + wc * 4);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint32_t kb = (w >> (16 * j + 4 * g)) & 0xfu;
                    fv4& v = acc[i][j];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = ((kb >> q) & 1u) ? v[q] : 0.f;
                    px[i][j] = pack_bf2(v[0], v[1]);
                    py[i][j] = pack_bf2(v[2], v[3]);
                }
            }
            if (colpart) {
                // the upper row half (rows 32 .. 63 of the tile) hands its rounded outputs to the lower
                // one, whose lanes then sum rows r, 16 + r, 32 + r, 48 + r in that order
                uint4* xp = (uint4*)(xchg + (wc * 64 + lane) * 32);
                if (wr == 1) {
                    xp[0] = make_uint4(px[0][0], py[0][0], px[0][1], py[0][1]);
                    xp[1] = make_uint4(px[1][0], py[1][0], px[1][1], py[1][1]);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (wr == 0) {
                    const uint4 o2 = xp[0], o3 = xp[1];
                    const uint32_t u2[2][2] = {{o2.x, o2.y}, {o2.z, o2.w}}, u3[2][2] = {{o3.x, o3.y}, {o3.z, o3.w}};
                    float* cp = colpart + (int64_t)(tile0 + t) * N + nb + 4 * g;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        fv4 s;
                        s[0] = ((bf_lo(px[0][j]) + bf_lo(px[1][j])) + bf_lo(u2[j][0])) + bf_lo(u3[j][0]);
                        s[1] = ((bf_hi(px[0][j]) + bf_hi(px[1][j])) + bf_hi(u2[j][0])) + bf_hi(u3[j][0]);
                        s[2] = ((bf_lo(py[0][j]) + bf_lo(py[1][j])) + bf_lo(u2[j][1])) + bf_lo(u3[j][1]);
                        s[3] = ((bf_hi(py[0][j]) + bf_hi(py[1][j])) + bf_hi(u2[j][1])) + bf_hi(u3[j][1]);
                        fv4 r;
#pragma unroll
                        for (int q = 0; q < 4; ++q) r[q] = row16_sum_dpp(s[q]);
                        if ((lane & 15) == 0) *(fv4*)(cp + 16 * j) = r;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);   // the output stores stay the youngest
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    px[i][j] = pack_bf2(acc[i][j][0], acc[i][j][1]);
                    py[i][j] = pack_bf2(acc[i][j][2], acc[i][j][3]);
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) store_pair(px[i][0], py[i][0], px[i][1], py[i][1], C, ldc, mr + 16 * i, nb, g);
        sg = sg == WS_NBUF - 1 ? 0 : sg + 1;
    }
    wait_vm<0>();
}

template <bool BT, int EK>
void launch_nkt(int nkt, unsigned grid, int M, int N, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb,
                bf16_t* C, int64_t ldc, const float* bias, uint32_t* bits, int64_t ldw, float* colpart, hipStream_t st) {
#define WS(NKT_)                                                                                                   \
    case NKT_:                                                                                                     \
        k_gemm_ws<BT, EK, NKT_><<<grid, 512, ws_lds_bytes(NKT_), st>>>(M, N, A, lda, B, ldb, C, ldc, bias, bits, ldw, \
                                                                      colpart);                                    \
        break
    switch (nkt) {
        WS(1); WS(2); WS(3); WS(4); WS(5); WS(6);
        default: break;
    }
#undef WS
}

}  // namespace

long long ws_gemm_launches() { return g_ws_launches; }

// the shapes the automatic dispatch hands to k_gemm_ws: the bound the products were specified with.  Measured
// (profiles/gemm_ws_ab.txt) are K = 384, M = 16384 with N = 1152 and N = 1536 only; every other shape inside the
// bound (smaller K, other N, M down to 4096) is extrapolated from those, not measured.
bool ws_gemm_auto(int64_t M, int64_t N, int kind) {
    const int only = g_gemm_ws == 2 ? CG_EPI_STORE : g_gemm_ws == 3 ? CG_EPI_BIAS_RELU : g_gemm_ws == 4 ? CG_EPI_RELU_BWD : -1;
    return g_gemm_ws && (only < 0 || kind == only) && N >= 1152 && M >= 4096;
}

bool ws_gemm_launch(int at, int bt, int64_t M, int64_t N, int64_t K, const bf16_t* A, int64_t lda, const bf16_t* B,
                    int64_t ldb, void* C, int c_dtype, int64_t ldc, const EpiArgs& e, int split_k, hipStream_t st) {
    if (at || split_k != 1 || e.beta != 0.f || c_dtype != CG_BF16 || g_pk_flags) return false;
    if (K % FBK || K > 6 * FBK || M % 64 || N % 128 || lda % 8 || ldb % 8 || ldc % 8) return false;
    if (M >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31)) return false;
    // per-lane DMA byte offsets (64 rows of A, 64 k-rows of a transposed B, 64 rows of keep words) are 32-bit
    if (lda >= ((int64_t)1 << 24) || ldb >= ((int64_t)1 << 24)) return false;
    if ((((uintptr_t)A) | ((uintptr_t)B) | ((uintptr_t)C)) & 15) return false;
    const bool with_bits = e.aux_dtype == CG_BITS && e.aux;
    uint32_t* bits = with_bits ? (uint32_t*)e.aux : nullptr;
    switch (e.kind) {
        case CG_EPI_STORE:
            if (e.colpart) return false;
            break;
        case CG_EPI_BIAS_RELU:
            if (!e.bias || (((uintptr_t)e.bias) & 15) || e.colpart) return false;
            if (e.aux_dtype == CG_BITS && (!e.aux || (((uintptr_t)e.aux) & 3) || e.ld_aux < N / 32)) return false;
            break;
        case CG_EPI_RELU_BWD:
            // the keep words come by LDS-DMA, 16 B (this panel's four words) per row
            if (!with_bits || (((uintptr_t)e.aux) & 15) || e.ld_aux % 4 || e.ld_aux < N / 32 ||
                e.ld_aux >= ((int64_t)1 << 24))
                return false;
            if (e.colpart && (((uintptr_t)e.colpart) & 15)) return false;
            break;
        default: return false;
    }
    int64_t P = gemm_cu_count();
    if (g_gemm_max_grid > 0 && g_gemm_max_grid < P) P = g_gemm_max_grid;
    if (P < N / 128) return false;   // one block per panel at least
    const int nkt = (int)(K / FBK);
#define WSL(BT_, EK_)                                                                                               \
    launch_nkt<BT_, EK_>(nkt, (unsigned)P, (int)M, (int)N, A, lda, B, ldb, (bf16_t*)C, ldc, e.bias, bits, e.ld_aux, \
                         e.colpart, st)
    if (e.kind == CG_EPI_STORE) {
        if (bt) WSL(true, CG_EPI_STORE);
        else WSL(false, CG_EPI_STORE);
    } else if (e.kind == CG_EPI_BIAS_RELU) {
        if (bt) WSL(true, CG_EPI_BIAS_RELU);
        else WSL(false, CG_EPI_BIAS_RELU);
    } else {
        if (bt) WSL(true, CG_EPI_RELU_BWD);
        else WSL(false, CG_EPI_RELU_BWD);
    }
#undef WSL
    ++g_ws_launches;
    return true;
}

}  // namespace cg
