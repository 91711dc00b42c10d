// charpt: the dropout keep bits of the bf16 MFMA attention kernels (attention_common.h: FWD and BWD
// tiles) -- the Philox generator, its launch fused with a sublayer's LayerNorm forward, and the
// host side of the keep-bit image (DropArgs, its size, the FWD / BWD pointer split).
#include "attention_common.h"
#include "ln_fwd.h"

using namespace cg;

namespace {

// Keep bits of the MFMA kernels (attention_common.h: FWD and BWD tiles).  One wave per 64x64
// (query tile QT, key tile KT <= QT) region, DM_TPW regions per wave: its four 32x32 sub-blocks
// (qs, ks) give FWD tiles (2 QT + qs, KT) and BWD tiles (2 KT + ks, QT) whole.  Per sub-block, lane
// l = 32 h + i takes query 32 qs + sig(i) -- sig(i) = (i & 3) + 8 ((i >> 2) & 3) + 4 (i >> 4), a lane
// order chosen for the BWD words below -- and keys 32 ks + 16 h .. +15: two Philox calls, 16
// decisions, each made by one packed saturating u16 add (or subtract, thr > 2^15) whose top bit is
// the decision and one packed shift.  A lane gathers its 32 decisions of sub-block row qs into one
// word R (bit 8 ks + 4 (w >> 1) + 2 c + (w & 1) + 16 e for call c, Philox word w, half e), an order in
// which
//   FWD: the lane's own decisions already sit at their FWD bits and its lane^32 partner's sit 4 bits
//        off: one v_permlane32_swap, one rotate and one v_bfi_b32 make the FWD word (stored at the
//        lane of query sig(i));
//   BWD: a 32x32 bit transpose inside each half-wave (five butterfly stages: one lane exchange, one
//        rotate, one v_bfi_b32 each) gives lane 32 h + j the column j of R over the 32 queries in
//        sig order, which makes every BWD lane's 16 query bits contiguous: one ds_bpermute and one
//        v_bfe_u32 per (qs, ks).
// (The round-2 form spent ~880 of its ~1200 instructions per region on keep8_bits compares, nibble
// assembly and an LDS transpose; Philox itself -- 19 v_mad_u64_u32 per call -- is what remains.)
constexpr int DM_TPW = 2;
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// keep decisions of the two u16 halves of a Philox word as bits 0 and 16: u >= thr <=> the top bit of
// sat(u + (2^15 - thr)) (thr <= 2^15) or of sat(u - (thr - 2^15)) (thr > 2^15)
template <bool SUBF>
__device__ __forceinline__ uint32_t keep2(uint32_t w, us2 k) {
    const us2 u = __builtin_bit_cast(us2, w);
    const us2 t = SUBF ? __builtin_elementwise_sub_sat(u, k) : __builtin_elementwise_add_sat(u, k);
    return __builtin_bit_cast(uint32_t, (us2)(t >> (us2)15));
}

// block `bid` (256 threads) of the keep-bit generation: regions (bid * 4 + wave) * DM_TPW ..
template <bool SUBF>
__device__ __forceinline__ void dropmask_block(int64_t T_, int64_t nbh, uint32_t* __restrict__ mask_f,
                                               uint32_t* __restrict__ mask_b, const DropArgs& d, int bid) {
    const int NB = (int)(T_ >> 5), NP = NB >> 1;
    const int64_t nreg = (int64_t)NP * (NP + 1) / 2, ntile = mask_tiles(T_);
    const int64_t total = nbh * nreg;
    const int lane = threadIdx.x & 63, h = lane >> 5, lq = lane & 31, w = threadIdx.x >> 6;
    const int qsig = (lq & 3) + 8 * ((lq >> 2) & 3) + 4 * (lq >> 4);
    const uint64_t stream = dropout_stream(d.rng_call, d.site);
    const uint16_t kc = (uint16_t)(SUBF ? d.thr - 0x8000u : 0x8000u - d.thr);
    const us2 K = us2{kc, kc};
    const int64_t first = ((int64_t)bid * 4 + w) * DM_TPW;
    if (first >= total) return;
    // butterfly stage j = 16 >> t: lanes with bit j clear keep the low blocks (mask m_j) and take their
    // partner's low blocks into the high ones (rotate right by 32 - j), the others the reverse
    uint32_t bmask[5], brot[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int j = 16 >> t;
        const uint32_t m = t == 0 ? 0x0000FFFFu : t == 1 ? 0x00FF00FFu : t == 2 ? 0x0F0F0F0Fu : t == 3 ? 0x33333333u : 0x55555555u;
        const bool lo = (lane & j) == 0;
        bmask[t] = lo ? m : ~m;
        brot[t] = lo ? (uint32_t)(32 - j) : (uint32_t)j;
    }
    // BWD gather source: column j of R (key lq of the sub-block) in half-wave lq >> 4
    const int kk = lq;
    const int jcol = 16 * (kk & 1) + 4 * ((kk >> 2) & 1) + 2 * ((kk >> 3) & 1) + ((kk >> 1) & 1);
    const int src0 = 32 * (kk >> 4) + jcol;   // + 8 ks
    const uint32_t fmask = h ? 0xF0F0F0F0u : 0x0F0F0F0Fu, frot = h ? 4u : 28u;
    uint64_t bh = (uint64_t)(first / nreg);
    const int r0 = (int)(first - (int64_t)bh * nreg);
    int QT = (int)((sqrtf(8.f * r0 + 1.f) - 1.f) * 0.5f);
    while ((QT + 1) * (QT + 2) / 2 <= r0) ++QT;
    while (QT * (QT + 1) / 2 > r0) --QT;
    int KT = r0 - QT * (QT + 1) / 2;
#pragma unroll 1
    for (int i = 0; i < DM_TPW; ++i) {
        if (first + i >= total) return;
        if (i && ++KT > QT) {
            KT = 0;
            if (++QT == NP) {
                QT = 0;
                ++bh;
            }
        }
        uint32_t R[2] = {0u, 0u};
        // Philox group of (query 64 QT + 32 qs + sig, keys 64 KT + 32 ks + 16 h + 8 c ..): g0 + 4 T qs + 4 ks + c
        const uint64_t g0 = ((bh * (uint64_t)T_ + (uint64_t)(64 * QT + qsig)) * (uint64_t)T_ + (uint64_t)(64 * KT + 16 * h)) >> 3;
#pragma unroll
        for (int qs = 0; qs < 2; ++qs)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint64_t grp = g0 + (uint64_t)(4 * T_ * qs + 4 * ks);
                // (the sub-block above the diagonal is computed too -- branch-free -- and zeroed below)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const u32x4 r = philox_group(d.seed, stream, grp + c);
                    const int b0 = 8 * ks + 2 * c;
                    R[qs] |= keep2<SUBF>(r.x, K) << b0;
                    R[qs] |= keep2<SUBF>(r.y, K) << (b0 + 1);
                    R[qs] |= keep2<SUBF>(r.z, K) << (b0 + 4);
                    R[qs] |= keep2<SUBF>(r.w, K) << (b0 + 5);
                }
            }
        if (QT == KT) R[0] &= 0x00FF00FFu;   // sub-block (0, 1) wholly above the diagonal: zero bits
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
            const auto sw = __builtin_amdgcn_permlane32_swap(R[qs], R[qs], false, false);
            const uint32_t part = h ? sw[0] : sw[1];
            const uint32_t rp = __builtin_amdgcn_alignbit(part, part, frot);
            mask_f[((int64_t)bh * ntile + mask_fwd_tile(2 * QT + qs, KT)) * 64 + 32 * h + qsig] =
                (R[qs] & fmask) | (rp & ~fmask);
        }
        uint32_t W[2];
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
            uint32_t x = R[qs];
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const uint32_t y = (uint32_t)__shfl_xor((int)x, 16 >> t, 64);
                const uint32_t ry = __builtin_amdgcn_alignbit(y, y, brot[t]);
                x = (x & bmask[t]) | (ry & ~bmask[t]);
            }
            W[qs] = x;
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const uint32_t a = (uint32_t)__shfl((int)W[0], src0 + 8 * ks, 64);
            const uint32_t b = (uint32_t)__shfl((int)W[1], src0 + 8 * ks, 64);
            mask_b[((int64_t)bh * ntile + mask_bwd_tile(2 * KT + ks, QT, NP)) * 64 + lane] =
                __builtin_amdgcn_ubfe(a, 16 * h, 16) | (__builtin_amdgcn_ubfe(b, 16 * h, 16) << 16);
        }
    }
}

template <bool SUBF>
__global__ __launch_bounds__(256) void k_attn_dropmask(int64_t T_, int64_t nbh, uint32_t* __restrict__ mask_f,
                                                       uint32_t* __restrict__ mask_b, DropArgs d) {
    dropmask_block<SUBF>(T_, nbh, mask_f, mask_b, d, (int)blockIdx.x);
}

// One launch for a sublayer's LayerNorm forward and its attention's keep bits (the two are
// independent: LN1 feeds the QKV GEMM, the bits the attention after it).  Blocks 0..n_dm-1 generate
// keep bits (Philox: VALU-bound), the rest run LayerNorm rows (HBM-bound) -- co-resident on the CUs,
// so the Philox arithmetic hides under the LayerNorm's memory time instead of running as its own
// 7.8 us launch at C2.  Bits and rows are exactly those of k_attn_dropmask and k_ln_fwd.
template <bool SUBF, int VEC, int NJ>
__global__ __launch_bounds__(256) void k_ln_fwd_dropmask(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, bf16_t* __restrict__ y,
                                                         float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                         int64_t rows, int C, float eps, int n_ln, int64_t T_,
                                                         int64_t nbh, uint32_t* __restrict__ mask_f,
                                                         uint32_t* __restrict__ mask_b, DropArgs d, int n_dm) {
    const int bid = (int)blockIdx.x;
    if (bid < n_dm)
        dropmask_block<SUBF>(T_, nbh, mask_f, mask_b, d, bid);
    else
        ln_fwd_rows<VEC, NJ, bf16_t, 2, true>(x, w, b, y, mean_out, rstd_out, rows, C, eps, bid - n_dm, n_ln);
}

// the image's BWD tiles: behind the B*H*mask_tiles(T) FWD tiles of 64 words
uint32_t* bwd_tiles(const uint64_t* mask, int64_t B, int64_t H, int64_t T) {
    return (uint32_t*)mask + B * H * mask_tiles(T) * 64;
}

// the generator's grid: 4 waves per block, DM_TPW regions per wave
int dropmask_blocks(int64_t B, int64_t H, int64_t T) {
    const int64_t np = T / 64, regions = B * H * np * (np + 1) / 2;
    return ceil_div(regions, 4 * DM_TPW);
}

}  // namespace

namespace cg {
namespace attn {
DropArgs make_drop(double p, uint64_t seed, const uint64_t* rng_call, int site) {
    DropArgs d;
    d.thr = p > 0 ? dropout_threshold(p) : 0u;
    d.dscale = p > 0 ? dropout_scale(p) : 1.f;
    d.seed = seed;
    d.rng_call = rng_call;
    d.site = site;
    d.mask = nullptr;
    d.mask_bwd = nullptr;
    return d;
}

// FWD and BWD tiles, 256 B each
int64_t mask_bytes(int64_t B, int64_t H, int64_t T) { return 2 * B * H * mask_tiles(T) * 256; }

void set_masks(DropArgs& d, const uint64_t* mask, int64_t B, int64_t H, int64_t T) {
    d.mask = (const uint32_t*)mask;
    d.mask_bwd = bwd_tiles(mask, B, H, T);
}

void launch_dropmask(int64_t B, int64_t H, int64_t T, uint64_t* mask, const DropArgs& d, hipStream_t st) {
    with_flag(d.thr > 0x8000u, [&](auto subf) {
        k_attn_dropmask<decltype(subf)::value><<<dropmask_blocks(B, H, T), 256, 0, st>>>(
            T, B * H, (uint32_t*)mask, bwd_tiles(mask, B, H, T), d);
    });
}
}  // namespace attn
}  // namespace cg

extern "C" int64_t cg_attn_mask_bytes(int64_t B, int64_t H, int64_t T) { return attn::mask_bytes(B, H, T); }

extern "C" int cg_attn_dropmask(int64_t B, int64_t H, int64_t T, double dropout_p, uint64_t seed,
                                const uint64_t* rng_call, int site, uint64_t* mask, void* stream) {
    CG_REQUIRE(B > 0 && H > 0 && T > 0 && T % 64 == 0, "cg_attn_dropmask: bad shape (T %% 64 == 0 required)");
    CG_REQUIRE(dropout_p > 0 && dropout_p < 1 && mask, "cg_attn_dropmask: needs 0 < p < 1 and a mask buffer");
    DropArgs d = attn::make_drop(dropout_p, seed, rng_call, site);
    attn::launch_dropmask(B, H, T, mask, d, (hipStream_t)stream);
    CG_LAUNCH_CHECK("cg_attn_dropmask");
    return CG_OK;
}

extern "C" int cg_layernorm_fwd_attn_dropmask(const float* x, const float* w, const float* b, void* y, int y_dtype,
                                              float* mean, float* rstd, int64_t rows, int64_t C, float eps, int64_t B,
                                              int64_t H, int64_t T, double dropout_p, uint64_t seed,
                                              const uint64_t* rng_call, int site, uint64_t* mask, void* stream) {
    CG_REQUIRE(B > 0 && H > 0 && T > 0 && T % 64 == 0, "cg_layernorm_fwd_attn_dropmask: bad shape (T %% 64 == 0 required)");
    CG_REQUIRE(dropout_p > 0 && dropout_p < 1 && mask, "cg_layernorm_fwd_attn_dropmask: needs 0 < p < 1 and a mask buffer");
    CG_REQUIRE(rows > 0 && C > 0 && C <= 2048, "cg_layernorm_fwd_attn_dropmask: need 0 < C <= 2048");
    hipStream_t st = (hipStream_t)stream;
    const DropArgs d = attn::make_drop(dropout_p, seed, rng_call, site);
    const bool al16 = (((uintptr_t)x | (uintptr_t)w | (uintptr_t)b) & 15) == 0;
    if (y_dtype != CG_BF16 || !al16 || (C != 384 && C != 768)) {   // the shapes without a fused form: two launches
        const int rc = cg_layernorm_fwd(x, w, b, y, y_dtype, mean, rstd, rows, C, eps, stream);
        if (rc != CG_OK) return rc;
        attn::launch_dropmask(B, H, T, mask, d, st);
        CG_LAUNCH_CHECK("cg_layernorm_fwd_attn_dropmask");
        return CG_OK;
    }
    const int n_dm = dropmask_blocks(B, H, T);
    int n_ln = (int)ceil_div(rows, 8);   // k_ln_fwd's grid: 4 waves x 2 rows per block
    n_ln = n_ln > 4096 ? 4096 : n_ln;
    with_flag(d.thr > 0x8000u, [&](auto subf) {
        with_flag(C == 384, [&](auto c384) {   // VEC: 2 at C = 384, 4 at C = 768
            k_ln_fwd_dropmask<decltype(subf)::value, decltype(c384)::value ? 2 : 4, 3><<<n_dm + n_ln, 256, 0, st>>>(
                x, w, b, (bf16_t*)y, mean, rstd, rows, (int)C, eps, n_ln, T, B * H, (uint32_t*)mask,
                bwd_tiles(mask, B, H, T), d, n_dm);
        });
    });
    CG_LAUNCH_CHECK("cg_layernorm_fwd_attn_dropmask");
    return CG_OK;
}
