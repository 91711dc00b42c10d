// charpt: weight-stationary bf16 MFMA GEMM (gfx950) for the K <= 384 wide-N training products -- the QKV
// forward, the FFN1 forward (bias + ReLU + keep bits) and the FFN2 input gradient (ReLU-backward + b1
// column partials) of GPT1.py:111-112,143-145.
//
// k_gemm_pk stages both operands of every 128x128 item through LDS and is bound by how fast a CU fills
// its LDS (profiles/r6_gemm_fill_c2.txt); half of those bytes are weights, fetched again for every item.
// Here a block owns one 128-column panel of the output for the whole launch:
//  * a block is four waves, one per 32 columns of the panel, and two blocks are resident per CU (P = 2 CUs
//    blocks); each wave holds 32 columns x K of weights in registers (K = 384: 96 VGPRs), loaded once
//    -- K-contiguous B straight from memory in the MFMA operand layout, transposed B through LDS with the
//    ds_read_b64_tr_b16 fragment reads;
//  * the LDS ring (3 stages of 32 rows x K, LDS-DMA, two half tiles in flight) carries activations only:
//    72 KB at K = 384 plus two keep-word slots, so two blocks fit the CU's 160 KB;
//  * per 32-row half tile: one counted wait, one barrier of the block's four waves, the full-K MFMA chain of
//    the wave's 32 x 32 outputs, the epilogue in registers; the half tile after next's DMA instructions (one
//    1-KB instruction per wave per K-tile) are issued between the K-tiles' MFMAs, before the epilogue's stores.
//    The two blocks of a CU share nothing and drift apart, so one's MFMA chain runs under the other's stores
//    and waits (profiles/gemm_ws_blocks_stamps.txt; the earlier form, one 8-wave block per CU on 64-row
//    tiles, is measured against this one in profiles/gemm_ws_blocks_ab.txt).
//  * A transposed B panel ([64 k][128] per K-tile, 96 KB at K = 384) goes through the ring's upper end in
//    passes of three K-tiles; at K = 384 that leaves stage 0 free, so tile 0 is requested first, else after
//    the passes.
//  * The ReLU-backward kinds are dealt whole 64-row tiles (two half tiles in turn): the keep words come once
//    per 64 rows, and the lower half's column sums wait in registers for the upper half's, added in
//    k_gemm_pk's order (rows r, 16 + r, 32 + r, 48 + r, then the DPP row).
//    Balance at M = 16384 on 256 CUs (P = 512; bpp = P / panels rounded down, 8 blocks idle):
//      N = 1152: bpp 56, 512 half tiles -> 10 against 9.14
//      N = 1536: bpp 42, 512 half tiles -> 13 against 12.19
//      N = 1536 ReLU-backward: 256 whole tiles -> 7 against 6.10, i.e. 14 half tiles against 12.19
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
constexpr int WS_KT_B = 64 * 128 * 2;   // one K-tile of the transposed weight panel: [64 k][128] bf16
constexpr int WS_BITS = 1024;       // ReLU-backward: 64 rows' keep words, 64 rows x 4 words (one DMA instruction)
constexpr int WS_LPT = 1;           // activation DMA instructions per wave per K-tile
// the epilogue's output stores (two 16-B row segments per wave; every kind issues at least these, last)
constexpr int WS_STORES = 2;

// LDS geometry of a block: four waves on 32-row half tiles
template <int NKT>
struct WsGeo {
    static constexpr int WAVES = 4, ROWS = 32;
    static constexpr int KT_A = ROWS * 64 * 2;   // one K-tile of an activation half tile: [32][64] bf16, row-swizzled
    static constexpr int STAGE = NKT * KT_A;
    // K-tiles of a transposed B panel staged at once, at the ring's upper end
    static constexpr int PK = NKT < 3 ? NKT : 3;
    static constexpr int RING = WS_NBUF * STAGE > PK * WS_KT_B ? WS_NBUF * STAGE : PK * WS_KT_B;
    static constexpr int PANEL = RING - PK * WS_KT_B;
    static constexpr int NBITS = 2;   // keep-word slots
    static constexpr int LDS = RING + NBITS * WS_BITS;
};

#ifdef CG_WS_STAMPS
// Diagnostic build only (make wsstamps; tools/ws_stamps.py): per block, s_memrealtime ticks (100 MHz) of
// [0] start, [1] weights in registers, [2] end, [3] XCC << 32 | HW_ID, [4] row tiles walked, [5] panel-major
// slot, and per tile t [8 + 3t ..] loop-head wait and barrier passed / MFMA chain done / stores issued.
// Lane 0 of wave 0 keeps them in the block's LDS (no vector-memory operation joins the counted waits) and
// copies them with plain vector stores, after the block's last wait, into a buffer no other code reads.
// Never in the product library.
constexpr int WS_ST_TILES = 24, WS_ST_WORDS = 8 + 3 * WS_ST_TILES, WS_ST_BLOCKS = 1024;
constexpr int WS_ST_LDS = WS_ST_WORDS * 8;
__device__ unsigned long long g_ws_stamps[WS_ST_BLOCKS * WS_ST_WORDS];
__device__ __forceinline__ unsigned long long ws_where() {
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    return ((unsigned long long)(xcc & 0xff) << 32) | hw;
}
#define WS_STAMP_AT(slot, v)                                                  \
    do {                                                                      \
        if (threadIdx.x == 0) ((volatile unsigned long long*)stamps)[slot] = (v); \
    } while (0)
#define WS_STAMP(slot) WS_STAMP_AT(slot, __builtin_amdgcn_s_memrealtime())
#define WS_STAMP_TILE(t, k)                                  \
    do {                                                     \
        if ((t) < WS_ST_TILES) WS_STAMP(8 + 3 * (t) + (k));  \
    } while (0)
#else
constexpr int WS_ST_LDS = 0;
#define WS_STAMP_AT(slot, v)
#define WS_STAMP(slot)
#define WS_STAMP_TILE(t, k)
#endif

constexpr int ws_lds_bytes(int nkt) {
    return nkt == 1 ? WsGeo<1>::LDS : nkt == 2 ? WsGeo<2>::LDS : nkt == 3 ? WsGeo<3>::LDS :
           nkt == 4 ? WsGeo<4>::LDS : nkt == 5 ? WsGeo<5>::LDS : WsGeo<6>::LDS;
}

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
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(1, 2)))
void k_gemm_ws(int M, int N, const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ B, int64_t ldb,
               bf16_t* __restrict__ C, int64_t ldc, const float* __restrict__ bias, uint32_t* __restrict__ bits,
               int64_t ldw, float* __restrict__ colpart) {
    static_assert(NKT >= 1 && NKT <= 6, "K <= 384");
    using G = WsGeo<NKT>;
    constexpr int STAGE = G::STAGE, ROWS = G::ROWS;
    // half tiles dealt together: the ReLU-backward kinds take whole 64-row tiles, half by half
    constexpr int UT = EK == CG_EPI_RELU_BWD ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wave, g = lane >> 4;
    const int npanels = N / 128, P = gridDim.x, bpp = P / npanels;
    const int lb = xcd_remap(blockIdx.x, P);
    const int panel = lb % npanels, rslot = lb / npanels;
    if (rslot >= bpp) return;
    // the M / (ROWS UT) row units over the panel's bpp blocks: leftover units one each to the first blocks.  bpp
    // is rounded down, so P % npanels blocks stay idle, and the launch ends with the blocks that got a leftover
    // unit (the header's arithmetic)
    const int T = M / (ROWS * UT), base = T / bpp, rem = T % bpp;
    const int ntile = (base + (rslot < rem ? 1 : 0)) * UT;
    if (ntile == 0) return;
    const int64_t row0 = (int64_t)(rslot * base + (rslot < rem ? rslot : rem)) * (ROWS * UT);
    const int64_t n0 = (int64_t)panel * 128, nb = n0 + wc * 32;

    const uint32_t lds0 = lds_base(smem);
    const uint32_t bits0 = lds0 + (uint32_t)G::RING;
#ifdef CG_WS_STAMPS
    char* const stamps = smem + G::LDS;
    WS_STAMP(0);
    WS_STAMP_AT(3, ws_where());
    WS_STAMP_AT(4, (unsigned long long)ntile);
    WS_STAMP_AT(5, (unsigned long long)lb);
#endif
    DmaP<false, ROWS, G::WAVES, FBK> da;
    da.init(lda, wave, lane);
    // K-tile kt of this block's half tile t into ring stage sg (each wave: one 1-KB instruction, 8 rows)
    auto issue_a = [&](int t, int kt, int sg) {
        const bf16_t* src = A + (row0 + (int64_t)t * ROWS) * lda + kt * FBK;
        da.issue1(src, 0, lds0 + (uint32_t)(sg * STAGE + kt * G::KT_A), wave);
    };
    // the keep words of the block's 64 rows u: lane l fetches row l's four words of this panel (wave 0 only)
    const uint32_t bits_off = (uint32_t)(lane * (int)ldw * 4);
    auto issue_bits = [&](int u, int slot) {
        if (EK == CG_EPI_RELU_BWD && wave == 0)
            dma16sl(bits + (row0 + (int64_t)u * 64) * ldw + panel * 4, bits_off, bits0 + (uint32_t)(slot * WS_BITS));
    };
    auto issue_tile0 = [&]() {
        issue_bits(0, 0);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) issue_a(0, kt, 0);
    };

    // ---- prologue: tile 0 on its way (if the transposed panel leaves stage 0 free), then the wave's 32 x K
    // weights into registers, then tile 1
    constexpr bool EARLY0 = !BT || STAGE <= G::PANEL;
    if constexpr (EARLY0) issue_tile0();
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
        using DB = DmaP<true, 128, G::WAVES, FBK>;
        DB db;
        db.init(ldb, wave, lane);
#pragma unroll
        for (int k0 = 0; k0 < NKT; k0 += G::PK) {
#pragma unroll
            for (int kt = k0; kt < k0 + G::PK && kt < NKT; ++kt)
#pragma unroll
                for (int i = 0; i < DB::PER_WAVE; ++i)
                    db.issue1(B + (int64_t)kt * FBK * ldb + n0, i, lds0 + (uint32_t)(G::PANEL + (kt - k0) * WS_KT_B), wave);
            wait_vm<0>();
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int kt = k0; kt < k0 + G::PK && kt < NKT; ++kt)
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        bw[kt][s][j] = frag<true, 128>(smem + G::PANEL + (kt - k0) * WS_KT_B, wc * 32 + 16 * j, s, lane);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();   // every wave has these weights: the panel's bytes are free again
        }
    }
    if constexpr (!EARLY0) issue_tile0();
    float4 bv[2];
    if constexpr (EK == CG_EPI_BIAS_RELU) {
#pragma unroll
        for (int j = 0; j < 2; ++j) bv[j] = *(const float4*)(bias + nb + 4 * g + 16 * j);
    }
    if (ntile > 1) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) issue_a(1, kt, 1);
    }
    WS_STAMP(1);

    // Vector-memory operations younger than tile t's DMAs when the loop head waits for them: tile t + 1's
    // (NKT per wave, if there is one) and tile t - 1's output stores (at least WS_STORES, the youngest).
    // Wave 0's keep-word DMA and any further epilogue store only make the count conservative.
    constexpr int LPT = NKT * WS_LPT;
    int sg = 0;
    fv4 slo[2];   // ReLU-backward: the lower half tile's column sums, rows r and 16 + r
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
        WS_STAMP_TILE(t, 0);
        const bool pf = t + 2 < ntile;
        const int sg2 = sg == 0 ? 2 : sg - 1;   // stage of tile t + 2 (= tile t - 1's)
        const char* img = smem + sg * STAGE;
        // the keep words of half tiles t + 2 and t + 3, into the slot of half tiles t - 2 and t - 1
        if (pf && !(t & 1)) issue_bits(t / 2 + 1, (t / 2 + 1) & 1);

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
                    af[kt & 1][s][i] = frag<false, 64>(img + kt * G::KT_A, 16 * i, s, lane);
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
        WS_STAMP_TILE(t, 1);

        // acc[i][j][q] = C[mr + 16 i][nb + 16 j + 4 g + q]
        const int64_t mr = row0 + (int64_t)t * ROWS + (lane & 15);
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
            // the words of this half tile's rows: half t & 1 of the 64-row slot (t / 2) & 1
            const char* bimg = smem + G::RING + ((t >> 1) & 1) * WS_BITS + (t & 1) * 32 * 16;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t w = *(const uint32_t*)(bimg + (16 * i + (lane & 15)) * 16 + wc * 4);
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
                if (!(t & 1)) {
                    // the lower half tile: rows r and 16 + r wait in registers for the upper half's
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        slo[j][0] = bf_lo(px[0][j]) + bf_lo(px[1][j]);
                        slo[j][1] = bf_hi(px[0][j]) + bf_hi(px[1][j]);
                        slo[j][2] = bf_lo(py[0][j]) + bf_lo(py[1][j]);
                        slo[j][3] = bf_hi(py[0][j]) + bf_hi(py[1][j]);
                    }
                } else {
                    // the upper half tile: rows 32 + r and 48 + r added in that order, then the DPP row sum
                    float* cp = colpart + (row0 / 64 + (t >> 1)) * N + nb + 4 * g;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        fv4 s;
                        s[0] = (slo[j][0] + bf_lo(px[0][j])) + bf_lo(px[1][j]);
                        s[1] = (slo[j][1] + bf_hi(px[0][j])) + bf_hi(px[1][j]);
                        s[2] = (slo[j][2] + bf_lo(py[0][j])) + bf_lo(py[1][j]);
                        s[3] = (slo[j][3] + bf_hi(py[0][j])) + bf_hi(py[1][j]);
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
        WS_STAMP_TILE(t, 2);
        sg = sg == WS_NBUF - 1 ? 0 : sg + 1;
    }
    wait_vm<0>();
#ifdef CG_WS_STAMPS
    WS_STAMP(2);
    if (tid == 0 && blockIdx.x < WS_ST_BLOCKS) {
        volatile unsigned long long* out = g_ws_stamps + (size_t)blockIdx.x * WS_ST_WORDS;
        for (int i = 0; i < WS_ST_WORDS; ++i) out[i] = ((volatile unsigned long long*)stamps)[i];
    }
#endif
}

using ws_fn = void (*)(int, int, const bf16_t*, int64_t, const bf16_t*, int64_t, bf16_t*, int64_t, const float*, uint32_t*,
                       int64_t, float*);

template <bool BT, int EK>
ws_fn pick_nkt(int nkt) {
    switch (nkt) {
        case 1: return k_gemm_ws<BT, EK, 1>;
        case 2: return k_gemm_ws<BT, EK, 2>;
        case 3: return k_gemm_ws<BT, EK, 3>;
        case 4: return k_gemm_ws<BT, EK, 4>;
        case 5: return k_gemm_ws<BT, EK, 5>;
        case 6: return k_gemm_ws<BT, EK, 6>;
        default: return nullptr;
    }
}
// the instantiation and its dynamic LDS bytes
ws_fn pick(int bt, int kind, int nkt, int& lds) {
    if (nkt < 1 || nkt > 6) return nullptr;
    lds = ws_lds_bytes(nkt) + WS_ST_LDS;
    // the grid is two blocks per CU: at a small K a third would fit beside them and leave another CU with one, so
    // every block asks for more than a third of the CU's 160 KB
    if (lds < 56 * 1024) lds = 56 * 1024;
    switch (kind) {
        case CG_EPI_STORE: return bt ? pick_nkt<true, CG_EPI_STORE>(nkt) : pick_nkt<false, CG_EPI_STORE>(nkt);
        case CG_EPI_BIAS_RELU: return bt ? pick_nkt<true, CG_EPI_BIAS_RELU>(nkt) : pick_nkt<false, CG_EPI_BIAS_RELU>(nkt);
        case CG_EPI_RELU_BWD: return bt ? pick_nkt<true, CG_EPI_RELU_BWD>(nkt) : pick_nkt<false, CG_EPI_RELU_BWD>(nkt);
        default: return nullptr;
    }
}

}  // namespace

long long ws_gemm_launches() { return g_ws_launches; }

// the shapes the automatic dispatch hands to k_gemm_ws: the bound the products were specified with.  Measured
// (profiles/gemm_ws_ab.txt against k_gemm_pk, profiles/gemm_ws_blocks_ab.txt for the 4-wave blocks) are K = 384,
// M = 16384 with N = 1152 and N = 1536 only; every other shape inside the bound (smaller K, other N, M down to
// 4096) is extrapolated from those, not measured.
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
    int64_t P = (int64_t)gemm_cu_count() * 2;   // every resident slot: two blocks per CU
    if (g_gemm_max_grid > 0 && g_gemm_max_grid < P) P = g_gemm_max_grid;
    if (P < N / 128) return false;   // one block per panel at least
    int lds = 0;
    const ws_fn fn = pick(bt, e.kind, (int)(K / FBK), lds);
    if (!fn) return false;
    fn<<<(unsigned)P, 256, lds, st>>>((int)M, (int)N, A, lda, B, ldb, (bf16_t*)C, ldc, e.bias, bits, e.ld_aux,
                                         e.colpart);
    ++g_ws_launches;
    return true;
}

// resident blocks per CU of the instantiation a product of this kind runs, by the runtime's occupancy query;
// -1 if there is no such instantiation
int ws_gemm_blocks_per_cu(int bt, int kind, int nkt) {
    int lds = 0, n = 0;
    const ws_fn fn = pick(bt, kind, nkt, lds);
    if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)fn, 256, (size_t)lds) != hipSuccess)
        return -1;
    return n;
}

#ifdef CG_WS_STAMPS
extern "C" int cg_debug_ws_stamps(unsigned long long* host, int nblocks) {
    if (nblocks < 0 || nblocks > WS_ST_BLOCKS) return 1;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_ws_stamps), (size_t)nblocks * WS_ST_WORDS * sizeof(unsigned long long)) ==
                   hipSuccess ? 0 : 1;
}
extern "C" int cg_debug_ws_stamps_reset() {
    static unsigned long long z[WS_ST_BLOCKS * WS_ST_WORDS];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_ws_stamps), z, sizeof(z)) == hipSuccess ? 0 : 1;
}
extern "C" int cg_debug_ws_stamps_words() { return WS_ST_WORDS; }
#endif

}  // namespace cg
