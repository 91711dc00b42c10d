// charpt: bf16 MFMA causal attention for head_size 64 -- the launchers, one launch site per kernel
// (kernels: attention_d64_ring.h, attention_d64_res.h; the A/B-only variants: ab/attention_ab.hip).
// GPT1.py:109-123,134-135.
#include "attention_d64_res.h"
#include "attention_d64_ring.h"

namespace cg {
int g_attn_variant = 0;
int g_attn_bwd_lpt = 1;   // merged resident backward: dK/dV workgroups first per XCD (0: interleaved, A/B)


namespace attn {
// sequence-resident kernels for T <= 256 unless cg_set_tuning("attn_variant", 1) selects the ring
// kernels (A/B and tests); attn_variant 2: resident dQ and dK/dV as two launches instead of one
static bool resident(int64_t T) { return T <= 256 && g_attn_variant != 1; }
// f(std::integral_constant<int, NT>): the resident kernels' tile count NT = T / 64 at compile time
template <typename F>
static void with_nt(int64_t T, F&& f) {
    switch ((int)(T / 64)) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}
// the same doubled by dropout (with_drop): f(NT constant, std::bool_constant<DROP>)
template <typename F>
static void with_nt_drop(int64_t T, const DropArgs& d, F&& f) {
    with_nt(T, [&](auto nt) { with_drop(d, [&](auto drop) { f(nt, drop); }); });
}

// packed rows: the sequence-resident kernels at T <= 256 and the ring kernels beyond, whatever
// attn_variant says; seg_resident: the backward is the merged launch, which can read a given delta
bool seg_resident(int64_t T) { return T <= 256; }

void launch_fwd_d64_seg(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                        bf16_t* o, int64_t ldo, float* lse, float scale, const DropArgs& d, const int32_t* seg_start,
                        const int32_t* seg_end, hipStream_t st) {
    if (!seg_resident(T)) {
        const dim3 grid((unsigned)((ceil_div(T, 256) + 1) / 2), (unsigned)(B * H));
        with_drop(d, [&](auto drop) {
            k_attn_fwd_d64d_seg<decltype(drop)::value><<<grid, 256, 0, st>>>(T, H, q, k, v, ld, o, ldo, lse, scale * LOG2E,
                                                                              d.mask, d.dscale, seg_start, seg_end);
        });
        return;
    }
    with_nt_drop(T, d, [&](auto nt, auto drop) {
        k_attn_fwd_d64r_seg<decltype(drop)::value, decltype(nt)::value><<<dim3(1, (unsigned)(B * H)), 256, 0, st>>>(
            H, q, k, v, ld, o, ldo, lse, scale * LOG2E, d.mask, d.dscale, seg_start, seg_end);
    });
}

void launch_bwd_d64_seg(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                        const bf16_t* o, int64_t ldo, const bf16_t* dout, int64_t ldd, const float* lse, float* delta,
                        bool delta_ready, bf16_t* dq, int64_t lddq, bf16_t* dk, bf16_t* dv, int64_t lddkv, float scale,
                        const DropArgs& d, const int32_t* seg_start, const int32_t* seg_end, hipStream_t st) {
    if (!seg_resident(T)) {   // dQ (writes delta), then dK/dV, as launch_dq_d64 / launch_dkdv_d64
        const dim3 gq((unsigned)((ceil_div(T, 256) + 1) / 2), (unsigned)(B * H));
        const dim3 gk((unsigned)((ceil_div(T, 128) + 1) / 2), (unsigned)(B * H));
        with_drop(d, [&](auto drop) {
            k_attn_dq_d64_seg<decltype(drop)::value, 4><<<gq, 256, 0, st>>>(T, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta,
                                                                             dq, lddq, scale, d.mask, d.dscale, seg_start);
            k_attn_dkdv_d64_seg<decltype(drop)::value, 4><<<gk, 256, 0, st>>>(T, H, q, k, v, ld, dout, ldd, lse, delta, dk,
                                                                               dv, lddkv, scale, d.mask_bwd, d.dscale,
                                                                               seg_end);
        });
        return;
    }
    const dim3 grid(1, (unsigned)(2 * B * H));
    with_nt_drop(T, d, [&](auto nt, auto drop) {
        with_flag(delta_ready, [&](auto din) {
            k_attn_bwd_d64r_seg<decltype(drop)::value, decltype(nt)::value, decltype(din)::value>
                <<<grid, 256, 0, st>>>(H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, dk, dv, lddkv, scale,
                                       d.mask, d.mask_bwd, d.dscale, g_attn_bwd_lpt, seg_start, seg_end);
        });
    });
}

void launch_fwd_d64(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                    bf16_t* o, int64_t ldo, float* lse, float scale, const DropArgs& d, hipStream_t st) {
    if (resident(T)) {
        with_nt_drop(T, d, [&](auto nt, auto drop) {
            k_attn_fwd_d64r<decltype(drop)::value, decltype(nt)::value><<<dim3(1, (unsigned)(B * H)), 256, 0, st>>>(
                H, q, k, v, ld, o, ldo, lse, scale * LOG2E, d.mask, d.dscale);
        });
        return;
    }
    const dim3 grid((unsigned)((ceil_div(T, 256) + 1) / 2), (unsigned)(B * H));   // pairs of query blocks
#ifdef CG_AB_VARIANTS   // attn_variant 4 / 5 / 6: ab/attention_ab.hip
    if (attn_ab::launch_fwd(g_attn_variant, grid, T, H, q, k, v, ld, o, ldo, lse, scale, d, st)) return;
#endif
    // Q fragments in registers, 4-slot LDS-DMA ring two tiles ahead: C4 forward 248 -> 223 us against
    // the register-staged ring, 244 us for the one-tile-ahead DMA ring with the Q image in LDS
    // (same-process interleaved A/B, profiles/r3_attn_fwd_ring_ab.txt)
    with_drop(d, [&](auto drop) {
        k_attn_fwd_d64d<decltype(drop)::value, true><<<grid, 256, 0, st>>>(T, H, q, k, v, ld, o, ldo, lse,
                                                                            scale * LOG2E, d.mask, d.dscale);
    });
}

// also computes delta = rowsum(dO * O) for its queries and writes it (read by launch_dkdv_d64 next)
static void launch_dq_d64(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                          const bf16_t* o, int64_t ldo, const bf16_t* dout, int64_t ldd, const float* lse, float* delta,
                          bf16_t* dq, int64_t lddq, float scale, const DropArgs& d, hipStream_t st) {
    if (resident(T)) {
        with_nt_drop(T, d, [&](auto nt, auto drop) {
            k_attn_dq_d64r<decltype(drop)::value, decltype(nt)::value><<<dim3(1, (unsigned)(B * H)), 256, 0, st>>>(
                H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, scale, d.mask, d.dscale);
        });
        return;
    }
    const dim3 grid((unsigned)((ceil_div(T, 256) + 1) / 2), (unsigned)(B * H));
#ifdef CG_AB_VARIANTS   // attn_variant 7: ab/attention_ab.hip
    if (attn_ab::launch_dq(g_attn_variant, grid, T, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, scale, d, st))
        return;
#endif
    with_drop(d, [&](auto drop) {
        k_attn_dq_d64<decltype(drop)::value, 4><<<grid, 256, 0, st>>>(T, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta,
                                                                       dq, lddq, scale, d.mask, d.dscale);
    });
}

static void launch_dkdv_d64(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                            const bf16_t* dout, int64_t ldd, const float* lse, const float* delta, bf16_t* dk, bf16_t* dv,
                            int64_t lddkv, float scale, const DropArgs& d, hipStream_t st) {
    if (resident(T)) {
        with_nt_drop(T, d, [&](auto nt, auto drop) {
            k_attn_dkdv_d64r<decltype(drop)::value, decltype(nt)::value><<<dim3(1, (unsigned)(B * H)), 256, 0, st>>>(
                H, q, k, v, ld, dout, ldd, lse, delta, dk, dv, lddkv, scale, d.mask_bwd, d.dscale);
        });
        return;
    }
    const dim3 grid((unsigned)((ceil_div(T, 128) + 1) / 2), (unsigned)(B * H));
#ifdef CG_AB_VARIANTS   // attn_variant 7: ab/attention_ab.hip
    if (attn_ab::launch_dkdv(g_attn_variant, grid, T, H, q, k, v, ld, dout, ldd, lse, delta, dk, dv, lddkv, scale, d, st))
        return;
#endif
    with_drop(d, [&](auto drop) {
        k_attn_dkdv_d64<decltype(drop)::value, 4><<<grid, 256, 0, st>>>(T, H, q, k, v, ld, dout, ldd, lse, delta, dk, dv,
                                                                         lddkv, scale, d.mask_bwd, d.dscale);
    });
}

bool bwd_merged(int64_t T) { return resident(T) && g_attn_variant != 2; }   // 2: the two resident kernels (A/B)

void launch_bwd_d64(int64_t B, int64_t T, int H, const bf16_t* q, const bf16_t* k, const bf16_t* v, int64_t ld,
                    const bf16_t* o, int64_t ldo, const bf16_t* dout, int64_t ldd, const float* lse, float* delta,
                    bool delta_ready, bf16_t* dq, int64_t lddq, bf16_t* dk, bf16_t* dv, int64_t lddkv, float scale,
                    const DropArgs& d, hipStream_t st) {
    if (bwd_merged(T)) {
        const dim3 grid(1, (unsigned)(2 * B * H));
        with_nt_drop(T, d, [&](auto nt, auto drop) {
            with_flag(delta_ready, [&](auto din) {   // DIN: delta is read, not computed
                k_attn_bwd_d64r<decltype(drop)::value, decltype(nt)::value, decltype(din)::value>
                    <<<grid, 256, 0, st>>>(H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, dk, dv, lddkv, scale,
                                           d.mask, d.mask_bwd, d.dscale, g_attn_bwd_lpt);
            });
        });
        return;
    }
    launch_dq_d64(B, T, H, q, k, v, ld, o, ldo, dout, ldd, lse, delta, dq, lddq, scale, d, st);
    launch_dkdv_d64(B, T, H, q, k, v, ld, dout, ldd, lse, delta, dk, dv, lddkv, scale, d, st);
}
}  // namespace attn

}  // namespace cg
