// charpt: error plumbing, counters, RNG helpers, sums, batch gather, timing events, and the tuning
// knobs' one setter (cg_set_tuning).
#include <limits.h>
#include <stdarg.h>

#include "attention_common.h"
#include "defer.h"
#include "ln_fwd.h"

namespace cg {
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace cg

using namespace cg;

extern "C" const char* cg_last_error_string(void) { return g_err; }
extern "C" int cg_version(void) { return 1; }

extern "C" int cg_device_info(int* n_cu, int* major, int* minor) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        set_error("cg_device_info: no HIP device");
        return CG_EHIP;
    }
    *n_cu = prop.multiProcessorCount;
    *major = prop.major;
    *minor = prop.minor;
    return CG_OK;
}

// --------------------------------------------------------------------------------------
__global__ void k_counter_add(int64_t* c, int64_t d) { *c += d; }
__global__ void k_rng_snapshot(uint64_t* c, uint64_t* s) {
    uint64_t v = *c;
    *s = v;
    *c = v + 1;
}

extern "C" int cg_counter_add(int64_t* counter, int64_t delta, void* stream) {
    k_counter_add<<<1, 1, 0, (hipStream_t)stream>>>(counter, delta);
    CG_LAUNCH_CHECK("cg_counter_add");
    return CG_OK;
}

extern "C" int cg_rng_snapshot(uint64_t* counter, uint64_t* snap, void* stream) {
    k_rng_snapshot<<<1, 1, 0, (hipStream_t)stream>>>(counter, snap);
    CG_LAUNCH_CHECK("cg_rng_snapshot");
    return CG_OK;
}

__global__ void k_dropout_mask(float* dst, int64_t n, uint32_t thr, uint64_t seed, const uint64_t* rng_call,
                               int site) {
    const uint64_t stream = dropout_stream(rng_call, site);
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // group of 8 consecutive elements
    const int64_t i0 = g * 8;
    if (i0 >= n) return;
    const uint32_t kb = keep8_bits(philox_group(seed, stream, (uint64_t)g), thr);
    for (int j = 0; j < 8 && i0 + j < n; ++j) dst[i0 + j] = ((kb >> j) & 1u) ? 1.f : 0.f;
}

extern "C" int cg_dropout_mask(float* dst, int64_t n, double p, uint64_t seed, const uint64_t* rng_call, int site,
                               void* stream) {
    CG_REQUIRE(n >= 0, "cg_dropout_mask: n < 0");
    if (n == 0) return CG_OK;
    const int64_t groups = (n + 7) / 8;
    k_dropout_mask<<<ceil_div(groups, 256), 256, 0, (hipStream_t)stream>>>(dst, n, dropout_threshold(p),
                                                                                 seed, rng_call, site);
    CG_LAUNCH_CHECK("cg_dropout_mask");
    return CG_OK;
}

// y = x * keep * 1/(1-p), element index r*C + c (FFN dropout backward, GPT1.py:146)
template <typename TY>
__global__ void k_dropout_apply(const float* __restrict__ x, int64_t rows, int64_t C, int64_t ldx, TY* __restrict__ y,
                                uint32_t thr, float dscale, uint64_t seed, const uint64_t* rng_call, int site) {
    const uint64_t stream = thr ? dropout_stream(rng_call, site) : 0;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // group of 8 consecutive elements
    const int64_t n = rows * C;
    const int64_t i0 = g * 8;
    if (i0 >= n) return;
    const uint32_t kb = thr ? keep8_bits(philox_group(seed, stream, (uint64_t)g), thr) : 0xffu;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t i = i0 + j;
        if (i < n) {
            const int64_t row = i / C, col = i % C;
            float v = x[row * ldx + col];
            if (thr) v = ((kb >> j) & 1u) ? v * dscale : 0.f;
            st_from_f32<TY>(y + i, v);
        }
    }
}

extern "C" int cg_dropout_apply(const float* x, int64_t rows, int64_t C, int64_t ldx, void* y, int y_dtype, double p,
                                uint64_t seed, const uint64_t* rng_call, int site, void* stream) {
    CG_REQUIRE(rows >= 0 && C > 0 && p >= 0 && p < 1, "cg_dropout_apply: bad args");
    const int64_t n = rows * C;
    if (n == 0) return CG_OK;
    const uint32_t thr = p > 0 ? dropout_threshold(p) : 0u;
    const float ds = p > 0 ? dropout_scale(p) : 1.f;
    const int grid = ceil_div((n + 7) / 8, 256);
    if (y_dtype == CG_BF16)
        k_dropout_apply<bf16_t><<<grid, 256, 0, (hipStream_t)stream>>>(x, rows, C, ldx, (bf16_t*)y, thr, ds, seed,
                                                                        rng_call, site);
    else
        k_dropout_apply<float><<<grid, 256, 0, (hipStream_t)stream>>>(x, rows, C, ldx, (float*)y, thr, ds, seed,
                                                                       rng_call, site);
    CG_LAUNCH_CHECK("cg_dropout_apply");
    return CG_OK;
}

// deterministic two-pass sum: pass 1 -> one partial per block (fixed order), pass 2 one block
__global__ void k_sum_partial(const float* x, int64_t n, float* part) {
    __shared__ float red[16];
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        s += x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        part[blockIdx.x] = t;
    }
}
__global__ void k_sum_final(const float* part, int np, float scale, float* out) {
    __shared__ float red[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < np; i += blockDim.x) s += part[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        *out = t * scale;
    }
}

extern "C" int cg_sum_f32(const float* x, int64_t n, float scale, float* out, float* ws, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int nb = (int)(n / 4096);
    nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
    k_sum_partial<<<nb, 256, 0, st>>>(x, n, ws);
    k_sum_final<<<1, 256, 0, st>>>(ws, nb, scale, out);
    CG_LAUNCH_CHECK("cg_sum_f32");
    return CG_OK;
}

__global__ void k_cast_f32_bf16(const float* x, bf16_t* y, int64_t n) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        float4 v = *(const float4*)(x + i);
        uint2 o;
        o.x = pack_bf2(v.x, v.y);
        o.y = pack_bf2(v.z, v.w);
        *(uint2*)(y + i) = o;
    } else {
        for (; i < n; ++i) y[i] = f2bf(x[i]);
    }
}

extern "C" int cg_cast_f32_bf16(const float* x, uint16_t* y, int64_t n, void* stream) {
    if (n == 0) return CG_OK;
    CG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 7) == 0, "cg_cast_f32_bf16: misaligned");
    k_cast_f32_bf16<<<ceil_div((n + 3) / 4, 256), 256, 0, (hipStream_t)stream>>>(x, (bf16_t*)y, n);
    CG_LAUNCH_CHECK("cg_cast_f32_bf16");
    return CG_OK;
}

// --------------------------------------------------------------------------------------
// get_batch windows on device (GPT1.py:79-80)
template <typename D>
__global__ void k_gather_batch(const D* data, const int64_t* ix, int64_t* x, int64_t* y, int64_t B, int64_t T) {
    int64_t b = blockIdx.y;
    int64_t base = ix[b];
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
        x[b * T + t] = (int64_t)data[base + t];
        y[b * T + t] = (int64_t)data[base + t + 1];
    }
}

extern "C" int cg_gather_batch(const void* data, int data_is_u8, const int64_t* ix, int64_t* x, int64_t* y,
                               int64_t B, int64_t T, void* stream) {
    CG_REQUIRE(B > 0 && T > 0 && B < 65536, "cg_gather_batch: bad shape");
    dim3 grid(ceil_div(T, 256), (unsigned)B);
    if (data_is_u8)
        k_gather_batch<uint8_t><<<grid, 256, 0, (hipStream_t)stream>>>((const uint8_t*)data, ix, x, y, B, T);
    else
        k_gather_batch<int64_t><<<grid, 256, 0, (hipStream_t)stream>>>((const int64_t*)data, ix, x, y, B, T);
    CG_LAUNCH_CHECK("cg_gather_batch");
    return CG_OK;
}

// (prompt, completion) rows for fine-tuning: row ix[b] of the packed table, padded past its length,
// with the targets of the prompt and of the padding set to ignore
__global__ void k_gather_pairs(const int64_t* __restrict__ table, const int64_t* __restrict__ plen,
                               const int64_t* __restrict__ tlen, const int64_t* __restrict__ ix,
                               int64_t* __restrict__ x, int64_t* __restrict__ y, int64_t T, int64_t pad,
                               int64_t ignore) {
    const int64_t b = blockIdx.y;
    const int64_t r = ix[b];
    const int64_t pl = plen[r], tl = tlen[r];
    const int64_t* row = table + r * (T + 1);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (int64_t)gridDim.x * blockDim.x) {
        x[b * T + t] = t < tl - 1 ? row[t] : pad;
        y[b * T + t] = (pl <= t + 1 && t + 1 < tl) ? row[t + 1] : ignore;
    }
}

extern "C" int cg_gather_pairs(const int64_t* table, const int64_t* plen, const int64_t* tlen, const int64_t* ix,
                               int64_t* x, int64_t* y, int64_t B, int64_t T, int64_t pad_token, int64_t ignore_index,
                               void* stream) {
    CG_REQUIRE(B > 0 && T > 0 && B < 65536, "cg_gather_pairs: bad shape");
    CG_REQUIRE(table && plen && tlen && ix && x && y, "cg_gather_pairs: null operand");
    dim3 grid(ceil_div(T, 256), (unsigned)B);
    k_gather_pairs<<<grid, 256, 0, (hipStream_t)stream>>>(table, plen, tlen, ix, x, y, T, pad_token, ignore_index);
    CG_LAUNCH_CHECK("cg_gather_pairs");
    return CG_OK;
}

extern "C" int cg_timing_event_create(void** event) {
    CG_REQUIRE(event, "cg_timing_event_create: null");
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) {
        cg::set_error("cg_timing_event_create: hipEventCreate failed");
        return CG_EHIP;
    }
    *event = (void*)e;
    return CG_OK;
}

extern "C" int cg_timing_event_record(void* event, void* stream) {
    CG_REQUIRE(event, "cg_timing_event_record: null event");
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    hipGraph_t g = nullptr;
    const hipGraphNode_t* deps = nullptr;
    size_t nd = 0;
    hipError_t r = hipStreamGetCaptureInfo_v2(st, &cs, &id, &g, &deps, &nd);
    if (r == hipSuccess && cs == hipStreamCaptureStatusActive) {
        // an event-record node appended to the capture by hand (hipEventRecordWithFlags with
        // hipEventRecordExternal is refused during capture on this runtime): it depends on the
        // stream's current capture frontier and becomes the new frontier
        hipGraphNode_t node = nullptr;
        r = hipGraphAddEventRecordNode(&node, g, deps, nd, (hipEvent_t)event);
        if (r == hipSuccess) r = hipStreamUpdateCaptureDependencies(st, &node, 1, hipStreamSetCaptureDependencies);
    } else if (r == hipSuccess) {
        r = hipEventRecord((hipEvent_t)event, st);
    }
    if (r != hipSuccess) {
        (void)hipGetLastError();   // leave no sticky error for the caller's next launch check
        cg::set_error("cg_timing_event_record: %s", hipGetErrorString(r));
        return CG_EHIP;
    }
    return CG_OK;
}

extern "C" int cg_timing_event_elapsed(void* start, void* end, float* ms) {
    CG_REQUIRE(start && end && ms, "cg_timing_event_elapsed: null");
    const hipError_t r = hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)end);
    if (r != hipSuccess) {
        cg::set_error("cg_timing_event_elapsed: %s", hipGetErrorString(r));
        return CG_EHIP;
    }
    return CG_OK;
}

extern "C" int cg_timing_event_destroy(void* event) {
    if (event) (void)hipEventDestroy((hipEvent_t)event);
    return CG_OK;
}

namespace {
#ifdef CG_AB_VARIANTS
constexpr bool AB_BUILD = true;
#else
constexpr bool AB_BUILD = false;   // the measured-slower A/B variants exist only in libcharpt_hip_ab.so (`make ab`)
#endif
constexpr int ANY_LO = INT_MIN, ANY_HI = INT_MAX;
constexpr int AB_LO(int lo) { return AB_BUILD ? ANY_LO : lo; }   // a bound only the product build applies
constexpr int AB_HI(int hi) { return AB_BUILD ? ANY_HI : hi; }

struct Knob {
    const char* key;
    int* knob;
    int lo, hi;   // accepted values, inclusive
};
const Knob KNOBS[] = {
    // gemm.hip: kernel choice; 0 automatic -- the product build takes only gemm_variant_in_product's values
    {"gemm_variant", &g_gemm_variant, ANY_LO, ANY_HI},
    {"gemm_max_grid", &g_gemm_max_grid, ANY_LO, ANY_HI},   // gemm.hip: cap on persistent-kernel blocks, 0 = resident slots
    {"gemm_group_p8", &g_gemm_group_p8, 0, 255},   // gemm.hip: gemm_tile.h tile_rc row panels per group (0/1: row-major)
    {"gemm_group_pk", &g_gemm_group_pk, 0, 255},   // gemm.hip: the same for k_gemm_pk
    {"gemm_n96", &g_gemm_n96, ANY_LO, ANY_HI},     // gemm.hip: 128x96 tiles for the part-filling fp32 residual forwards
    {"gemm_ws", &g_gemm_ws, 0, 4},                 // gemm_ws.hip: the weight-stationary kernel for the K <= 384 wide-N products (2-4: one product)
    {"pk_flags", &g_pk_flags, ANY_LO, ANY_HI},     // gemm_pk.hip: the persistent kernels' epilogue / what-if bits
    {"linear_rows_nb", &g_linear_rows_nb, 0, 2},   // rows_f32.hip: 0 k_linear_f32q (16-row waves), 1 / 2 k_linear_f32t
    {"skip_splitk_reduce", &g_skip_splitk_reduce, ANY_LO, ANY_HI},   // defer.hip: WRONG results, timing only
    {"adam_per_launch", &g_adam_per_launch, ANY_LO, ANY_HI},   // defer.hip: AdamW jobs per launch's free blocks
    {"adam_batch", &g_adam_batch, AB_LO(1), AB_HI(1)},   // defer.hip: side-block AdamW chunks in flight (A/B: 4, 5)
    {"red_side", &g_red_side, ANY_LO, ANY_HI},     // defer.hip: part-filling launches take a pending reduce on extra blocks
    // attention_d64.hip: 0 automatic, 1 ring kernels at T <= 256 (and, attention_f32.hip, the 64-query-block
    // fp32 forward instead of the sequence-resident one), 2 separate resident dQ / dK-dV launches (A/B
    // build, ab/attention_ab.hip, also 4: the 8-wave ping-pong forward at T % 256 == 0, 512..1024; 5 / 6:
    // the earlier forward rings; 7: the 2-slot backward rings)
    {"attn_variant", &g_attn_variant, AB_LO(0), AB_HI(2)},
    {"attn_bwd_lpt", &g_attn_bwd_lpt, 0, 1},       // attention_d64.hip k_attn_bwd_d64r: merged resident backward order (1 = dK/dV first)
    {"decode_attn_rows", &g_decode_attn_rows, 0, 1},   // decode.hip: the coalesced-chunk phase-1 decode attention
    {"adamw_mode", &g_adamw_mode, 0, 5},           // adamw.hip: cg_adamw's kernel form, 0 = by size
    {"ln_rl", &g_ln_rl, 0, 2},   // layernorm.hip: backward rows' next loads before the current stores (2: also at C = 768)
    {"ln_nt", &g_ln_nt, ANY_LO, ANY_HI},           // layernorm.hip: the backward's non-temporal streams (-1 automatic, 0..3)
    {"ln_pf", &g_ln_pf, ANY_LO, ANY_HI},           // layernorm.hip: next row's loads before the current row
    {"ln_waves", &g_ln_waves, ANY_LO, ANY_HI},     // layernorm.hip: takes effect for workspaces sized after the call
    {"ln_rpb", &g_ln_rpb, ANY_LO, ANY_HI},         // layernorm.hip: takes effect for workspaces sized after the call
};

// product build: automatic (0), the register-staged fallback (2), the persistent 128x128 (9) and 256x256 (24)
// tiles, the weight-stationary kernel (31: gemm_ws.hip, whatever it takes; the rest as 2),
// k_gemm_f32 for every fp32 product (98: not the small-M or persistent kernels; 97: k_gemm_f32s, not the
// K-resident one; 96: the persistent k_gemm_f32p at any M), the generic kernels (99); the measured-slower A/B
// tiles (among them 26, the 256x256 tile on the staggered 8-phase schedule) only in the A/B build
bool gemm_variant_in_product(int v) {
    return v == 0 || v == 2 || v == 9 || v == 24 || v == 31 || v == 96 || v == 97 || v == 98 || v == 99;
}
}  // namespace

extern "C" int cg_set_tuning(const char* key, int value) {
    CG_REQUIRE(key, "cg_set_tuning: null key");
    if (!strcmp(key, "defer_splitk") || !strcmp(key, "slab_bf16") || !strcmp(key, "defer_partials")) {
        set_error("cg_set_tuning: %s is a per-call flag since round 5 (cg_epilogue_t.flags CG_GEMM_DEFER_REDUCE / "
                  "CG_GEMM_SLAB_BF16, the CG_DEFER flag of the _ex reduces)", key);
        return CG_EINVAL;
    }
    for (const Knob& k : KNOBS) {
        if (strcmp(key, k.key)) continue;
        const bool ok = value >= k.lo && value <= k.hi &&
                        (AB_BUILD || k.knob != &g_gemm_variant || gemm_variant_in_product(value));
        CG_REQUIRE(ok, "cg_set_tuning: %s = %d is not accepted by this build (out of range, or an A/B variant: make ab)",
                   key, value);
        *k.knob = value;
        return CG_OK;
    }
    set_error("cg_set_tuning: unknown key %s", key);
    return CG_EINVAL;
}
