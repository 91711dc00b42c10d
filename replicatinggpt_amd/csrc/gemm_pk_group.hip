// charpt: several split-K weight gradients (dW = dy^T x: GPT1.py:111-112,136 -- the attention
// sublayer's projection and QKV weights) as ONE launch of the persistent 128x128 2-stage kernel with both
// operands transposed, behind cg_gemm_wgrad_group.
//
// Two weight gradients of one sublayer are each too small for the machine on their own: at C2 the
// projection's 9 output tiles need split 32 (8 K-tiles per item) to reach 288 of 512 resident slots, and
// each launch pays its fixed cost.  Here the launch's item list is the concatenation of the problems'
// split-major item lists, so the caller can choose one split for the whole group (9 + 27 tiles at split
// 14: 504 items of 18-19 K-tiles, one round) and the LDS-DMA stream runs across problem boundaries as it
// runs across item boundaries in k_gemm_pk (gemm_pk.hip, whose loop this is).
//
// Per problem: operand origins and leading dimensions (so the DMA lane offsets), K-tile counts, slab
// base.  The DMA cursor re-derives its lane offsets when it enters another problem; the compute cursor
// looks its item's problem up at the item's end.  An item covers the K-tiles its single launch covers, in
// the same order, and writes the same slab element: each problem's slabs -- and so its reduced output --
// equal cg_gemm's at the same split bit for bit.  No block waits for another.
#include "gemm_pk.h"

namespace cg {
namespace {

struct GroupArgs {
    GroupProb p[MAX_GROUP];
    int n, nitems, flags;
};

// EK16: bf16 slabs (16-B row segments, 8 stores per item) instead of fp32 ones (16 stores)
template <bool EK16>
__global__ __launch_bounds__((GeoP<128, 128, 2>::THREADS), (GeoP<128, 128, 2>::OCC))
__attribute__((amdgpu_waves_per_eu(1, GeoP<128, 128, 2>::WPE)))
void k_gemm_pk_group(GroupArgs ga, RedJobs red) {
    constexpr int BM = 128, BN = 128, NBUF = 2, BK = FBK, NS = BK / 32;
    using G = GeoP<BM, BN, NBUF, BK>;
    using DA = DmaP<true, BM, G::WAVES, BK>;
    using DB = DmaP<true, BN, G::WAVES, BK>;
    constexpr int LPT = DA::PER_WAVE + DB::PER_WAVE;  // DMA instructions per thread per K-tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / G::WN, wn = wave % G::WN;
    const int nitems = ga.nitems;
    const int P = gridDim.x, b = blockIdx.x;
    const int my_items = b < nitems ? (nitems - 1 - b) / P + 1 : 0;

    // item j of this block: its problem, output tile and split (the problem's own split-major order
    // and tile order, as k_gemm_pk decodes them)
    auto decode = [&](int j, int& pi, int64_t& m0, int64_t& n0, int& split) {
        const int it = xcd_remap(b + j * P, nitems);
        pi = 0;
        for (int q = 1; q < ga.n; ++q)
            if (it >= ga.p[q].item0) pi = q;
        const GroupProb& p = ga.p[pi];
        const int loc = it - p.item0;
        int tm, tn;
        split = loc / p.ntiles;
        tile_rc(loc - split * p.ntiles, p.ntiles / p.tilesN, p.tilesN, p.gm, tm, tn);
        m0 = (int64_t)tm * BM;
        n0 = (int64_t)tn * BN;
    };
    // split s covers K-tiles [s*nkc, min((s+1)*nkc, nkt)): the last split may be shorter
    auto split_nk = [&](int pi, int sp) {
        const GroupProb& p = ga.p[pi];
        return p.nkt - sp * p.nkc < p.nkc ? p.nkt - sp * p.nkc : p.nkc;
    };
    int total = 0;
    for (int j = 0; j < my_items; ++j) {
        int64_t m0, n0;
        int pi, sp;
        decode(j, pi, m0, n0, sp);
        total += split_nk(pi, sp);
    }

    DA da;
    DB db;
    const uint32_t lds0 = lds_base(smem);
    // DMA issue cursor (item ij, K-tile ikt), its problem and operand origins; prep_next() as in k_gemm_pk
    int ij = 0, ikt = 0, ink = 0, dpi = -1;
    const bf16_t* oa = ga.p[0].A;
    const bf16_t* ob = ga.p[0].B;
    const bf16_t* na = oa;
    const bf16_t* nbp = ob;
    auto prep_next = [&](bool real) {
        if (real) {
            if (ikt == 0) {
                int64_t m0, n0;
                int pi, sp;
                decode(ij, pi, m0, n0, sp);
                const GroupProb& p = ga.p[pi];
                if (pi != dpi) {   // another problem: its leading dimensions
                    da.init(p.lda, wave, lane);
                    db.init(p.ldb, wave, lane);
                    dpi = pi;
                }
                ink = split_nk(pi, sp);
                const int64_t kb = (int64_t)sp * p.nkc * BK;
                oa = p.A + kb * p.lda + m0;
                ob = p.B + kb * p.ldb + n0;
            }
            na = oa + ikt * da.kstep;
            nbp = ob + ikt * db.kstep;
            if (++ikt == ink) {
                ikt = 0;
                ++ij;
            }
        }
    };

    fv4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fv4{0.f, 0.f, 0.f, 0.f};

    if (total > 0) {   // NBUF - 1 = 1 stage ahead
        prep_next(true);
#pragma unroll
        for (int i = 0; i < DA::PER_WAVE; ++i) da.issue1(na, i, lds0, wave);
#pragma unroll
        for (int i = 0; i < DB::PER_WAVE; ++i) db.issue1(nbp, i, lds0 + G::IMG_A, wave);
    }

    // an item's slab stores are the youngest EPI_OPS vector-memory operations at the next step's wait
    // (k_gemm_pk): they drain under the next MFMAs
    constexpr int EPI_OPS = EK16 ? 8 : 16;
    int cur = 0, cj = 0, ckt = 0, cnk = 0;
    if (my_items) {
        int64_t m0, n0;
        int pi, sp;
        decode(0, pi, m0, n0, sp);
        cnk = split_nk(pi, sp);
    }
    bool stored = false;
    for (int g = 0; g < total; ++g) {
        if (stored && !(ga.flags & 1)) wait_vm<EPI_OPS>();
        else wait_vm<0>();
        stored = false;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const int nb = cur ^ 1;
        prep_next(g + 1 < total);   // past the last K-tile: the same (valid) addresses again, into the free stage
        const uint32_t dimg = lds0 + (uint32_t)(nb * G::STAGE);
        const char* imgA = smem + cur * G::STAGE;
        const char* imgB = imgA + G::IMG_A;
        sv8 af[NS][4], bf[NS][4];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[s][j] = frag<true, BN>(imgB, wn * 64 + j * 16, s, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i) af[s][i] = frag<true, BM>(imgA, wm * 64 + i * 16, s, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
        // 8 groups of 4 MFMAs, one of the next stage's DMA instructions after each
        auto issue_dma = [&](int t) {
            if (t < DA::PER_WAVE) da.issue1(na, t, dimg, wave);
            else db.issue1(nbp, t - DA::PER_WAVE, dimg + G::IMG_A, wave);
        };
        static_assert(LPT <= 4 * NS, "one DMA instruction per MFMA group");
#pragma unroll
        for (int t = 0; t < 4 * NS; ++t) {
            const int s = t >> 2, i = t & 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma_bf16(bf[s][j], af[s][i], acc[i][j]);
            if (t < LPT) issue_dma(t);
        }
#pragma unroll
        for (int t = 0; t < 4 * NS; ++t) {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            if (t < LPT) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        cur = nb;
        if (++ckt == cnk) {
            // item done: acc[i][j][r] = C[mw + 16i + (lane&15)][nw + 16j + 4(lane>>4) + r]
            int64_t m0, n0;
            int pi, sp;
            decode(cj, pi, m0, n0, sp);
            const GroupProb& p = ga.p[pi];
            const int64_t mr = m0 + wm * 64 + (lane & 15), nc = n0 + wn * 64 + 4 * (lane >> 4);
            const int64_t M = p.M, N = p.N;
            if constexpr (EK16) {
                store_bf16_wide<4>(acc, (bf16_t*)p.ws + (int64_t)sp * M * N, N, mr, nc);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        *(fv4*)((float*)p.ws + ((int64_t)sp * M + mr + 16 * i) * N + nc + 16 * j) = acc[i][j];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fv4{0.f, 0.f, 0.f, 0.f};
            ckt = 0;
            ++cj;
            if (cj < my_items) {
                int64_t m1, n1;
                int p1, sp1;
                decode(cj, p1, m1, n1, sp1);
                cnk = split_nk(p1, sp1);
            }
            stored = true;
        }
    }
    wait_vm<0>();  // the dummy DMAs past the last K-tile land before the workgroup's LDS is released
    // deferred work of earlier launches, as in k_gemm_pk: on the blocks beyond the items when the
    // launch has them, else in every block's tail
    if (red.n || red.na) red_tail(red, P > nitems ? nitems : 0);
}

}  // namespace

// grid, side slots and pending work as gemm_pk.hip launch_p / launch_1 give a single problem
void pk_group_launch(const GroupProb* probs, int n, bool slab_bf16, hipStream_t st) {
    using G = GeoP<128, 128, 2>;
    GroupArgs ga = {};
    int64_t nitems = 0;
    for (int i = 0; i < n; ++i) {
        ga.p[i] = probs[i];
        ga.p[i].item0 = (int)nitems;
        // tile order: gemm_pk.hip launch_1's choice for this problem
        const int tM = probs[i].ntiles / probs[i].tilesN, tN = probs[i].tilesN;
        ga.p[i].gm = g_gemm_group_pk > 0 ? g_gemm_group_pk : (tN > tM ? tM : 0);
        nitems += (int64_t)probs[i].ntiles * probs[i].split_k;
    }
    ga.n = n;
    ga.nitems = (int)nitems;
    ga.flags = g_pk_flags;
    int64_t slots = (int64_t)gemm_cu_count() * G::OCC;
    if (g_gemm_max_grid > 0 && g_gemm_max_grid < slots) slots = g_gemm_max_grid;
    const bool side = g_red_side && slots - nitems >= SIDE_MIN && has_pending_reduces(st, true);
    const unsigned grid = (unsigned)(nitems < slots && !side ? nitems : slots);
    const bool side_ok = (int64_t)grid - nitems >= SIDE_MIN;
    if (slab_bf16) k_gemm_pk_group<true><<<grid, G::THREADS, G::LDS, st>>>(ga, take_pending_reduces(st, side_ok));
    else k_gemm_pk_group<false><<<grid, G::THREADS, G::LDS, st>>>(ga, take_pending_reduces(st, side_ok));
}

}  // namespace cg
