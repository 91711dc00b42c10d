// charpt: GEMMs for every nn.Linear in the hot path (GPT1.py:111-112,121,136,143,145,184) and
// their dgrad/wgrad in the backward: cg_gemm's dispatch and the generic kernel.  (The fp32 MFMA kernels
// are in gemm_f32.hip, the split-K and column-sum reduces in reduce.hip, the deferred-work queues in
// defer.hip.)
//
//   C[m,n] = epilogue( sum_k A(m,k) * B(n,k) ),  A(m,k) = A[m*lda+k] | A[k*lda+m] (a_trans),
//                                                B(n,k) = B[n*ldb+k] | B[k*ldb+n] (b_trans).
//
// Two kernels:
//   * k_gemm_bf16  -- the perf path: 128x128x64 tiles, 4 waves (2x2, 64x64 each), bf16 MFMA
//     16x16x32 with fp32 accumulation, register-staged double-buffered LDS (one barrier per
//     K-tile), XOR-swizzled LDS images: K-contiguous operands are read with ds_read_b128,
//     M/N-contiguous ("transposed") operands with the gfx950 transpose read ds_read_b64_tr_b16,
//     so forward (NT), dgrad (NN) and wgrad (TN) share one kernel.  Epilogue staged through LDS
//     and stored 16 B per lane.  Needs M%128 = N%128 = K%64 = 0, 16-B aligned rows.
//   * k_gemm_generic -- exact-f32 MFMA (16x16x4 f32) on 64x64x16 tiles with bounds checks:
//     any shape/stride/dtype; the fp32 parity path and odd shapes (n_embd=126, V=65).
// Both support deterministic split-K through fp32 slabs reduced in a fixed order.
#include "defer.h"

using namespace cg;

namespace {

// =====================================================================================
// generic exact-f32 GEMM
// =====================================================================================
constexpr int GBM = 64, GBN = 64, GBK = 16;

template <typename TA, typename TB, typename TC>
__global__ __launch_bounds__(256) void k_gemm_generic(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K,
                                                      const TA* __restrict__ A, int64_t lda,
                                                      const TB* __restrict__ B, int64_t ldb, TC* __restrict__ C,
                                                      int64_t ldc, EpiArgs epi, int split_k, int64_t kchunk,
                                                      float* __restrict__ ws) {
    __shared__ float As[GBK][GBM + 4];
    __shared__ float Bs[GBK][GBN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t tilesN = (N + GBN - 1) / GBN;
    const int64_t m0 = (int64_t)(blockIdx.x / tilesN) * GBM;
    const int64_t n0 = (int64_t)(blockIdx.x % tilesN) * GBN;
    const int split = blockIdx.y;
    const int64_t kb = split * kchunk;
    const int64_t ke = kb + kchunk < K ? kb + kchunk : K;

    fv4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = fv4{0.f, 0.f, 0.f, 0.f};

    for (int64_t k0 = kb; k0 < ke; k0 += GBK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int mm, kk;
            if (!a_trans) {
                kk = tid & 15;
                mm = (tid >> 4) + 16 * i;
            } else {
                mm = tid & 63;
                kk = (tid >> 6) + 4 * i;
            }
            const int64_t gm = m0 + mm, gk = k0 + kk;
            float v = 0.f;
            if (gm < M && gk < ke) v = ld_as_f32<TA>(A + (a_trans ? gk * lda + gm : gm * lda + gk));
            As[kk][mm] = v;
            int nn;
            if (!b_trans) {
                kk = tid & 15;
                nn = (tid >> 4) + 16 * i;
            } else {
                nn = tid & 63;
                kk = (tid >> 6) + 4 * i;
            }
            const int64_t gn = n0 + nn, gk2 = k0 + kk;
            float w = 0.f;
            if (gn < N && gk2 < ke) w = ld_as_f32<TB>(B + (b_trans ? gk2 * ldb + gn : gn * ldb + gk2));
            Bs[kk][nn] = w;
        }
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < GBK / 4; ++k4) {
            const int kr = k4 * 4 + (lane >> 4);
            float a0 = As[kr][wm * 32 + (lane & 15)];
            float a1 = As[kr][wm * 32 + 16 + (lane & 15)];
            float b0 = Bs[kr][wn * 32 + (lane & 15)];
            float b1 = Bs[kr][wn * 32 + 16 + (lane & 15)];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    const uint64_t stream = (epi.kind == CG_EPI_BIAS_DROP_RESID && epi.thr) ? dropout_stream(epi.rng_call, epi.site) : 0;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + wm * 32 + mt * 16 + 4 * (lane >> 4) + r;
                const int64_t n = n0 + wn * 32 + nt * 16 + (lane & 15);
                if (m < M && n < N) {
                    if (split_k > 1) {
                        ws[((int64_t)split * M + m) * N + n] = acc[mt][nt][r];
                    } else {
                        store_out<TC>(C, m * ldc + n, epi_scalar(epi, acc[mt][nt][r], m, n, N, stream), epi.beta);
                    }
                }
            }
}

EpiArgs make_epi(const cg_epilogue_t* e) {
    EpiArgs a;
    memset(&a, 0, sizeof(a));
    a.kind = CG_EPI_STORE;
    a.dscale = 1.f;
    if (!e) return a;
    a.kind = e->kind;
    a.bias = e->bias;
    a.resid = e->resid;
    a.ld_resid = e->ld_resid;
    a.aux = e->aux;
    a.aux_dtype = e->aux_dtype;
    a.ld_aux = e->ld_aux;
    a.thr = e->dropout_p > 0 ? dropout_threshold(e->dropout_p) : 0u;
    a.dscale = e->dropout_p > 0 ? dropout_scale(e->dropout_p) : 1.f;
    a.seed = e->seed;
    a.rng_call = e->rng_call;
    a.site = e->site;
    a.beta = e->beta;
    a.colpart = e->colpart;
    return a;
}

template <typename TA, typename TB>
int launch_generic(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
                   const void* B, int64_t ldb, void* C, int c_dtype, int64_t ldc, const EpiArgs& e, int split_k,
                   void* ws, hipStream_t st) {
    int64_t kchunk = (K + split_k - 1) / split_k;
    kchunk = (kchunk + GBK - 1) / GBK * GBK;
    const int64_t tiles = ((M + GBM - 1) / GBM) * ((N + GBN - 1) / GBN);
    dim3 grid((unsigned)tiles, (unsigned)split_k);
    if (c_dtype == CG_BF16)
        k_gemm_generic<TA, TB, bf16_t><<<grid, 256, 0, st>>>(a_trans, b_trans, M, N, K, (const TA*)A, lda,
                                                             (const TB*)B, ldb, (bf16_t*)C, ldc, e, split_k, kchunk,
                                                             (float*)ws);
    else
        k_gemm_generic<TA, TB, float><<<grid, 256, 0, st>>>(a_trans, b_trans, M, N, K, (const TA*)A, lda,
                                                            (const TB*)B, ldb, (float*)C, ldc, e, split_k, kchunk,
                                                            (float*)ws);
    return CG_OK;
}

}  // namespace

namespace cg {
int g_gemm_variant = 0;
int g_gemm_max_grid = 0;
int g_gemm_group_p8 = 0;   // persistent-kernel tile order (gemm_tile.h tile_rc), cg_set_tuning knobs
int g_gemm_group_pk = 0;
int g_gemm_n96 = 1;       // cg_set_tuning("gemm_n96"): 128x96 tiles for the part-filling fp32 residual forwards (gemm_pk.hip launch_n96)
}  // namespace cg

extern "C" int cg_gemm_colpart_supported(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, int64_t lda,
                                         int64_t ldb, int64_t ldc) {
    return gemm_colpart_supported(a_trans, b_trans, M, N, K, lda, ldb, ldc) ? 1 : 0;
}

extern "C" int cg_gemm_relu_bits_supported(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, int64_t lda,
                                           int64_t ldb, int64_t ldc) {
    return gemm_relu_bits_supported(a_trans, b_trans, M, N, K, lda, ldb, ldc) ? 1 : 0;
}

extern "C" int64_t cg_gemm_ws_launches(void) { return (int64_t)ws_gemm_launches(); }

extern "C" int cg_gemm_ws_blocks_per_cu(int b_trans, int kind, int nkt) { return ws_gemm_blocks_per_cu(b_trans, kind, nkt); }

extern "C" int cg_gemm_rowdot_supported(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, int64_t lda,
                                        int64_t ldb, int64_t ldc) {
    return gemm_rowdot_supported(a_trans, b_trans, M, N, K, lda, ldb, ldc) ? 1 : 0;
}

extern "C" int64_t cg_gemm_workspace(int64_t M, int64_t N, int split_k) {
    return split_k > 1 ? (int64_t)split_k * M * N * (int64_t)sizeof(float) : 0;
}

extern "C" int cg_gemm_resid_layernorm_supported(int64_t M, int64_t N, int64_t K) {
    return gemm_resid_ln_supported(M, N, K) ? 1 : 0;
}

extern "C" int cg_gemm_resid_layernorm(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W,
                                       int64_t ldw, float* out, int64_t ldc, const cg_epilogue_t* epi,
                                       const float* ln_w, const float* ln_b, void* y, float* mean, float* rstd,
                                       float eps, void* stream) {
    CG_REQUIRE(gemm_resid_ln_supported(M, N, K),
               "cg_gemm_resid_layernorm: unsupported shape M=%lld N=%lld K=%lld (N == 384, M %% 64 == 0, K %% 64 == 0)",
               (long long)M, (long long)N, (long long)K);
    CG_REQUIRE(epi && (epi->kind == CG_EPI_BIAS_RESID || epi->kind == CG_EPI_BIAS_DROP_RESID) && epi->bias &&
                   epi->resid && epi->beta == 0.f && epi->flags == 0 && !epi->colpart,
               "cg_gemm_resid_layernorm: needs a BIAS_RESID / BIAS_DROP_RESID epilogue with bias and residual, beta 0");
    CG_REQUIRE(A && W && out && ln_w && ln_b && y && mean && rstd, "cg_gemm_resid_layernorm: null pointer");
    CG_REQUIRE(lda >= K && ldw >= K && lda % 8 == 0 && ldw % 8 == 0 && ldc >= N && ldc % 4 == 0 &&
                   epi->ld_resid >= N && epi->ld_resid % 4 == 0,
               "cg_gemm_resid_layernorm: bad leading dimensions");
    CG_REQUIRE((((uintptr_t)A | (uintptr_t)W | (uintptr_t)out | (uintptr_t)epi->resid | (uintptr_t)epi->bias |
                 (uintptr_t)ln_w | (uintptr_t)ln_b | (uintptr_t)y) & 15) == 0,
               "cg_gemm_resid_layernorm: operands must be 16-B aligned");
    const EpiArgs e = make_epi(epi);
    gemm_resid_ln_launch(M, K, (const bf16_t*)A, lda, (const bf16_t*)W, ldw, out, ldc, e, ln_w, ln_b, (bf16_t*)y, mean,
                         rstd, eps, (hipStream_t)stream);
    CG_LAUNCH_CHECK("cg_gemm_resid_layernorm");
    return CG_OK;
}

extern "C" int cg_gemm(int op_dtype, int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, const void* A,
                       int64_t lda, const void* B, int64_t ldb, void* C, int c_dtype, int64_t ldc,
                       const cg_epilogue_t* epi, int split_k, void* workspace, void* stream) {
    CG_REQUIRE(M > 0 && N > 0 && K > 0, "cg_gemm: empty problem M=%lld N=%lld K=%lld", (long long)M, (long long)N,
               (long long)K);
    CG_REQUIRE(split_k >= 1 && split_k <= 64, "cg_gemm: split_k out of range");
    CG_REQUIRE(split_k == 1 || workspace, "cg_gemm: split_k > 1 needs a workspace");
    CG_REQUIRE(op_dtype == CG_BF16 || op_dtype == CG_F32, "cg_gemm: bad op dtype");
    hipStream_t st = (hipStream_t)stream;
    EpiArgs e = make_epi(epi);
    CG_REQUIRE(split_k == 1 || e.kind == CG_EPI_STORE || e.kind == CG_EPI_BIAS || e.kind == CG_EPI_BIAS_RESID,
               "cg_gemm: split-K supports STORE/BIAS/BIAS_RESID epilogues only");
    const bool vec4 = N % 4 == 0 && ldc % 4 == 0 && M * N < (int64_t)1 << 31 &&
                      (((uintptr_t)C | (uintptr_t)workspace | (uintptr_t)(e.bias ? e.bias : (const float*)C) |
                        (uintptr_t)(e.resid ? e.resid : (const float*)C)) & 15) == 0 &&
                      (!e.resid || e.ld_resid % 4 == 0);
    bool fast = false;
    const int flags = epi ? epi->flags : 0;
    CG_REQUIRE((flags & ~(CG_GEMM_SLAB_BF16 | CG_GEMM_DEFER_REDUCE)) == 0, "cg_gemm: unknown epilogue flags %#x", flags);
    // bf16 slabs (CG_GEMM_SLAB_BF16): only the 128x128 persistent kernel writes them (fast_gemm_launch
    // declines otherwise, nothing launched) and only the vectorised reduces read them
    e.slab_bf16 = (flags & CG_GEMM_SLAB_BF16) && split_k > 1 && op_dtype == CG_BF16 && e.kind == CG_EPI_STORE &&
                  c_dtype == CG_F32 && vec4 && ldc == N && (M * N) % 8 == 0 && !g_skip_splitk_reduce;
    if (e.slab_bf16) {
        fast = fast_gemm_launch(a_trans, b_trans, M, N, K, (const bf16_t*)A, lda, (const bf16_t*)B, ldb, C, c_dtype,
                                ldc, e, split_k, (float*)workspace, st);
        if (!fast) e.slab_bf16 = 0;
    }
    if (fast) {
    } else if (op_dtype == CG_BF16 && fast_gemm_launch(a_trans, b_trans, M, N, K, (const bf16_t*)A, lda,
                                                       (const bf16_t*)B, ldb, C, c_dtype, ldc, e, split_k,
                                                       (float*)workspace, st)) {
        fast = true;
    } else if (e.aux_dtype == CG_BITS) {
        set_error("cg_gemm: CG_BITS ReLU keep bits need a persistent bf16 kernel (cg_gemm_relu_bits_supported)");
        return CG_EINVAL;
    } else if (e.kind == CG_EPI_STORE_ROWDOT) {
        set_error("cg_gemm: CG_EPI_STORE_ROWDOT needs the 128x128 persistent bf16 kernel (cg_gemm_rowdot_supported; "
                  "bf16 aux, colpart, ld_resid = T dividing M)");
        return CG_EINVAL;
    } else if (e.colpart) {
        set_error("cg_gemm: colpart needs a persistent bf16 kernel (bf16 operands and output, NT/NN, beta 0, "
                  "split 1, M %% 128 == 0, default dispatch)");
        return CG_EINVAL;
    } else if (op_dtype == CG_BF16) {
        launch_generic<bf16_t, bf16_t>(a_trans, b_trans, M, N, K, A, lda, B, ldb, C, c_dtype, ldc, e, split_k,
                                       workspace, st);
    } else if (c_dtype == CG_F32 && g_gemm_variant != 99) {  // 99: force the generic kernel (tests)
        launch_f32(a_trans, b_trans, M, N, K, (const float*)A, lda, (const float*)B, ldb, (float*)C, ldc, e, split_k,
                   (float*)workspace, st);
    } else {
        launch_generic<float, float>(a_trans, b_trans, M, N, K, A, lda, B, ldb, C, c_dtype, ldc, e, split_k,
                                     workspace, st);
    }
    // (slab sets above 40 MB -- the C4 FFN / QKV weight gradients -- keep their own reduce kernel: in
    // the next 256x256 GEMM's tail they measured no gain, C4 58.2 vs 57.9 ms/step)
    if (split_k > 1 && vec4 && !g_skip_splitk_reduce && (flags & CG_GEMM_DEFER_REDUCE) && fast &&
        e.kind == CG_EPI_STORE && c_dtype == CG_F32 && ldc == N &&
        (int64_t)split_k * M * N * 4 <= ((int64_t)40 << 20)) {
        // deferred: summed in the tail of the next persistent GEMM launch on this stream of this
        // device (or cg_flush_deferred(st) there) -- the queue key holds the device, so the null
        // stream, whose handle names a different queue on every device, is fine too
        std::lock_guard<std::mutex> lk(defer_mutex());
        DeferQueue& q = *defer_queue(st, true);
        if (q.nred == MAX_RED) flush_red_locked(q);
        q.red[q.nred++] = RedJob{(const float*)workspace, (float*)C, M * N / 4, split_k, e.beta, e.slab_bf16};
    } else if (split_k > 1) {
        launch_splitk_reduce(workspace, split_k, M, N, C, c_dtype, ldc, e, vec4 && !g_skip_splitk_reduce, st);
    }
    CG_LAUNCH_CHECK("cg_gemm");
    return CG_OK;
}


// ---- grouped split-K weight gradients (gemm_pk_group.hip) -----------------------------------------
namespace {

// cg_gemm's view of one problem of the group: what its slabs are and whether it applies at all
struct GroupPlan {
    bool ok, slab_bf16, defer;
};
GroupPlan plan_group_problem(const cg_wgrad_problem_t& p) {
    GroupPlan g = {false, false, false};
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || !p.A || !p.B || !p.C || !p.workspace || p.split_k < 2 || p.split_k > 64)
        return g;
    if (p.flags & ~(CG_GEMM_SLAB_BF16 | CG_GEMM_DEFER_REDUCE)) return g;
    if (g_skip_splitk_reduce || (((uintptr_t)p.workspace) & 15)) return g;
    if (!gemm_wgrad_group_ok(p.M, p.N, p.K, p.A, p.lda, p.B, p.ldb, p.C, p.ldc, p.split_k)) return g;
    // (the shape conditions above make cg_gemm's vec4 true)
    g.ok = true;
    g.slab_bf16 = (p.flags & CG_GEMM_SLAB_BF16) && p.ldc == p.N && (p.M * p.N) % 8 == 0;
    g.defer = (p.flags & CG_GEMM_DEFER_REDUCE) && p.ldc == p.N &&
              (int64_t)p.split_k * p.M * p.N * 4 <= ((int64_t)40 << 20);
    return g;
}

bool plan_group(const cg_wgrad_problem_t* probs, int n, GroupPlan* plans) {
    if (!probs || n < 1 || n > MAX_GROUP) return false;
    int64_t items = 0;
    for (int i = 0; i < n; ++i) {
        plans[i] = plan_group_problem(probs[i]);
        if (!plans[i].ok || plans[i].slab_bf16 != plans[0].slab_bf16) return false;   // one slab type per launch
        items += (probs[i].M / 128) * (probs[i].N / 128) * probs[i].split_k;
    }
    return items < ((int64_t)1 << 30);
}

}  // namespace

extern "C" int cg_gemm_wgrad_group_supported(const cg_wgrad_problem_t* probs, int n) {
    GroupPlan plans[MAX_GROUP];
    return plan_group(probs, n, plans) ? 1 : 0;
}

extern "C" int cg_gemm_wgrad_group(const cg_wgrad_problem_t* probs, int n, void* stream) {
    GroupPlan plans[MAX_GROUP];
    CG_REQUIRE(plan_group(probs, n, plans),
               "cg_gemm_wgrad_group: unsupported group (cg_gemm_wgrad_group_supported: 1..%d bf16 problems the "
               "128x128 persistent kernel takes at split_k >= 2, one slab type)", MAX_GROUP);
    hipStream_t st = (hipStream_t)stream;
    GroupProb gp[MAX_GROUP];
    for (int i = 0; i < n; ++i) {
        const cg_wgrad_problem_t& p = probs[i];
        GroupProb& q = gp[i];
        q = GroupProb{};
        q.A = (const bf16_t*)p.A;
        q.B = (const bf16_t*)p.B;
        q.ws = p.workspace;
        q.lda = p.lda;
        q.ldb = p.ldb;
        q.M = (int)p.M;
        q.N = (int)p.N;
        q.tilesN = (int)(p.N / 128);
        q.ntiles = (int)(p.M / 128) * q.tilesN;
        q.nkt = (int)(p.K / 64);
        q.nkc = (q.nkt + p.split_k - 1) / p.split_k;
        q.split_k = p.split_k;
    }
    pk_group_launch(gp, n, plans[0].slab_bf16, st);
    // each problem's reduce: deferred or launched exactly as cg_gemm does after its own launch
    for (int i = 0; i < n; ++i) {
        const cg_wgrad_problem_t& p = probs[i];
        if (plans[i].defer) {
            std::lock_guard<std::mutex> lk(defer_mutex());
            DeferQueue& q = *defer_queue(st, true);
            if (q.nred == MAX_RED) flush_red_locked(q);
            q.red[q.nred++] = RedJob{(const float*)p.workspace, p.C, p.M * p.N / 4, p.split_k, p.beta, plans[i].slab_bf16};
        } else {
            EpiArgs e = make_epi(nullptr);
            e.beta = p.beta;
            e.slab_bf16 = plans[i].slab_bf16;
            launch_splitk_reduce(p.workspace, p.split_k, p.M, p.N, p.C, CG_F32, p.ldc, e, true, st);
        }
    }
    CG_LAUNCH_CHECK("cg_gemm_wgrad_group");
    return CG_OK;
}
