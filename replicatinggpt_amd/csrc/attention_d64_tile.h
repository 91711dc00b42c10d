// charpt: the tile helpers of the head_size-64 attention kernels -- MFMA wrappers, the LDS tile
// image and its swizzle, the softmax / pack / keep-bit pieces, the per-tile arithmetic of each
// direction and the DMA helpers -- shared by the ring kernels (attention_d64_ring.h), the
// sequence-resident kernels (attention_d64_res.h) and the A/B-only ones (ab/attention_ab.hip,
// `make ab`).  attention_d64.hip is the product translation unit and holds the launchers.
#pragma once
// bf16 MFMA causal attention for head_size 64 (the C2/C4 perf path of Head.forward x
// n_head, GPT1.py:109-123,134-135) -- forward, dQ and dK/dV kernels on v_mfma_f32_32x32x16_bf16.
//
// Structure (CDNA4: 64-wide waves, 32x32 MFMA tiles):
//  * forward / dQ: a block of 4 waves owns 256 queries; each wave two 32-query groups, g and 7-g
//    of the block, so every wave walks the same number of causal key tiles (1+4, 1+4, 2+3, 2+3 at
//    the first block: the causal triangle is balanced inside the block).  Products are swapped --
//    S^T = K Q^T, dP^T = V dO^T -- so the query is the accumulator column (lane & 31): softmax
//    statistics are lane-local plus one lane^32 exchange, and the accumulator, packed to bf16, is
//    directly the B operand of O^T = V^T P^T / dQ^T = K^T dS^T (V / K read transposed).
//  * dK/dV: a block of 4 waves owns 128 keys (32 per wave); S = Q K^T, dP = dO V^T with the key
//    as the column, Z = dropped P and dS feed dV^T = dO^T Z and dK^T = Q^T dS as B operands.
//  * 64-row K/V (or Q/dO) tiles, register-staged into a double-buffered LDS ring (next tile's
//    global loads issued before the current tile's MFMAs, written after them, one barrier per
//    tile).  One XOR swizzle serves both the row reads (ds_read_b128) and the transposed reads
//    (ds_read_b64_tr_b16) conflict-free.
//  * Forward: lazy rescaling -- the running max is only moved (and O, l rescaled) when a tile's max
//    exceeds it by 2^8, so the O-wide multiply is off the common path; probabilities stay <= 256.
//  * Dropout keep bits (k_attn_dropmask, attention_common.h): one 32-bit word per lane per 64-row
//    tile, loaded a tile ahead with the K/V (or Q/dO) staging loads and applied as v_bfe_i32 +
//    v_and_b32 per element; the 1/(1-p) is applied once at the end.
#include <float.h>

#include "attention_common.h"

namespace cg {

namespace {

typedef float fv16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) sv4 lds_sv4;

constexpr int TILE = 8192;             // [64 rows][64 bf16] image
constexpr float RESCALE_THR = 8.0f;    // log2 units (forward lazy rescale)

__device__ __forceinline__ fv16 mfma32(sv8 a, sv8 b, fv16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bfv8, a), __builtin_bit_cast(bfv8, b), c, 0, 0,
                                                   0);
}

// Forward row sums on the matrix core.  A 32x32x16 B-operand fragment of P^T (lane l: keys 8 (l>>5) + j,
// query l & 31) read as the B operand of v_mfma_f32_16x16x32_bf16 (lane l: k' = 8 (l>>4) + j, column
// l & 15) mixes two queries per column; the A operand below is 1 exactly where the k' group's query
// half ((k'>>3) & 1 = (l>>4) & 1 of the source lane) equals the output row's ((m>>2) & 1), so output
// row m, column n sums the 16 keys of query n + 16 ((m>>2) & 1), and lane l's four accumulator
// registers (rows 4 (l>>4) + i) all hold the running sum of query l & 31.  One 16-cycle MFMA per
// 16 keys replaces 16 v_add_f32 per lane (the sum is over the bf16-rounded P that O^T also sums).
typedef float fv4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ fv4 mfma16(sv8 a, sv8 b, fv4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bfv8, a), __builtin_bit_cast(bfv8, b), c, 0, 0,
                                                   0);
}
__device__ __forceinline__ sv8 rowsum_ones(int lane) {
    const short o = (((lane >> 4) ^ (lane >> 2)) & 1) ? (short)0 : (short)0x3F80;   // bf16 1.0
    return sv8{o, o, o, o, o, o, o, o};
}

// [64][64] bf16 image, 128-B rows; 16-B chunk c of row r at r*128 + ((c ^ X(r)) << 4) with
// X(r) = ((r>>1)&1)<<2 | (r>>2)&3.  Row reads of the 32x32x16 operand (16-lane groups of
// ds_read_b128 over rows {0-3,12-15,20-27} / {4-11,16-19,28-31}) land on 16 distinct 16-B slots;
// transposed reads (a 32-lane half reads rows r0..r0+3, 64 bytes each) on 64 distinct banks.
__device__ __forceinline__ int aoff(int r, int c) { return r * 128 + ((c ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3))) << 4); }

// A operand, tile rows rb..rb+31: lane l holds X(rb + (l&31), 16 ks + 8 (l>>5) + j), j = 0..7
__device__ __forceinline__ sv8 frag_row(const char* img, int rb, int ks, int lane) {
    return *(const sv8*)(img + aoff(rb + (lane & 31), 2 * ks + (lane >> 5)));
}

// A operand = tile^T, tile columns cb..cb+31 as rows: lane l, element j <-> tile row
// rb + 16 ks + 8 (j>>2) + 4 (l>>5) + (j&3), column cb + (l&31) -- the k order of an accumulator
// packed as the B operand (pack16 below).  Two ds_read_b64_tr_b16: each 16-lane group reads a
// 4-row x 16-column block, lane 4q+p addressing row q, columns 4p..4p+3.
__device__ __forceinline__ sv8 frag_tr(const char* img, int rb, int ks, int cb, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int col = cb + 16 * (g & 1) + 4 * p;
    const int r0 = rb + 16 * ks + 4 * (g >> 1) + q;
    const int chunk = col >> 3, byte = (col & 7) * 2;
    const sv4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_sv4*)(img + aoff(r0, chunk) + byte));
    const sv4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_sv4*)(img + aoff(r0 + 8, chunk) + byte));
    return sv8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// FWD keep-word bit of accumulator register r of 32-key subtile kt (attention_common.h: the two
// registers packed into one bf16 pair sit at bits j and j + 16, j = 8 kt + (r >> 1))
__device__ __forceinline__ constexpr int fwd_bit(int kt, int r) { return 8 * kt + (r >> 1) + 16 * (r & 1); }

// accumulator registers 8s..8s+7 -> bf16 B-operand fragment of k-step s
__device__ __forceinline__ sv8 pack16(const fv16& x, int s) {
    const uint32_t w0 = pack_bf2(x[8 * s + 0], x[8 * s + 1]), w1 = pack_bf2(x[8 * s + 2], x[8 * s + 3]);
    const uint32_t w2 = pack_bf2(x[8 * s + 4], x[8 * s + 5]), w3 = pack_bf2(x[8 * s + 6], x[8 * s + 7]);
    sv8 r;
    r[0] = (short)(w0 & 0xffff); r[1] = (short)(w0 >> 16);
    r[2] = (short)(w1 & 0xffff); r[3] = (short)(w1 >> 16);
    r[4] = (short)(w2 & 0xffff); r[5] = (short)(w2 >> 16);
    r[6] = (short)(w3 & 0xffff); r[7] = (short)(w3 >> 16);
    return r;
}

// accumulator row of register r (column = lane & 31)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// all-ones / zero lane mask from bit `bit` of this lane's keep word (one v_bfe_i32).  The empty asm
// hides that the value is a sign-extended bit: hipcc otherwise rewrites `x & mask` as a select,
// v_and + v_cmp + v_cndmask, sunk past the bf16 packing (+v_lshr / v_perm): 4-5 instructions per
// element instead of v_bfe_i32 + v_and_b32.  (No real instruction in asm here: an asm consumer of a
// v_exp result would bypass the transcendental-use hazard padding.)
__device__ __forceinline__ uint32_t keep_mask(uint32_t w, int bit) {
    uint32_t m = keep_lanes(w, bit);
    asm("" : "+v"(m));
    return m;
}
// kept ? a : b through the keep mask: one gfx950 v_bitop3_b32 (truth table 0xe4 = s2 ? s0 : s1,
// bitwise); the plain C form became v_and, v_xor, v_and, v_or once the mask had a second use
__device__ __forceinline__ float keep_sel2(uint32_t m, float a, float b) {
    return __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(a), __float_as_uint(b), m, 0xe4));
}

// causal mask of one 32x32 accumulator tile whose key rows start at key0 (column = query qa):
// rows acc_row(r) > qa - key0 become -inf.  Called under a wave-uniform branch (diagonal tiles only).
__device__ __forceinline__ void mask_upper(fv16& x, int qa, int key0, int lane, float fill) {
    const int rel = qa - key0 - 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if ((r & 3) + 8 * (r >> 2) > rel) x[r] = fill;
}

// ---- packed rows (the SEG instantiations): query i sees key j iff seg_start[i] <= j <= i ------------
// Forward / dQ orientation (column = query): rows whose key, key0 + acc_row(r), lies before the
// lane's segment start become -inf -- the mirror of mask_upper; rel = seg_start - key0.  Called
// under a wave-uniform branch (some lane's segment starts inside or after the subtile).
__device__ __forceinline__ void mask_before(fv16& x, int rel, int lane) {
    const int lim = rel - 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if ((r & 3) + 8 * (r >> 2) < lim) x[r] = -INFINITY;
}
// dK/dV orientation (column = key): rows whose query, q0 + acc_row(r), lies at or beyond the lane's
// segment end become -inf; rel = seg_end - q0
__device__ __forceinline__ void mask_from(fv16& x, int rel, int lane) {
    const int lim = rel - 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if ((r & 3) + 8 * (r >> 2) >= lim) x[r] = -INFINITY;
}
// seg_start / seg_end of this lane's row as loaded, made safe: 0 <= start <= row < end (a malformed
// bound then still leaves every query its own key, so no softmax row is empty)
__device__ __forceinline__ int seg_lo(uint32_t w, int row) {
    const int s = (int)w;
    return s < 0 ? 0 : (s > row ? row : s);
}
__device__ __forceinline__ int seg_hi(uint32_t w, int row) {
    const int e = (int)w;
    return e <= row ? row + 1 : e;
}
// the lanes (as query bits 0..31 of a 32-query group starting at qg) of this lane's segment [lo, hi)
__device__ __forceinline__ uint32_t seg_peers(int lo, int hi, int qg) {
    const int a = lo - qg, b = hi - qg;
    const uint32_t below_b = b >= 32 ? 0xffffffffu : (1u << b) - 1u;
    const uint32_t below_a = a <= 0 ? 0u : (1u << a) - 1u;
    return below_b & ~below_a;
}

// XCD-aware block order for a (row blocks, B*H) grid: the dispatcher deals linear block ids to the
// 8 XCDs round-robin and each XCD has its own L2; the bijective remap hands every XCD a contiguous
// run of logical ids (whole (b, h) groups, which stream the same K/V or Q/dO), measured 35 -> 81 %
// L2 hits at C4.  REV runs a group's blocks last-first (longest causal prefix first).
template <bool REV>
__device__ __forceinline__ void block_coords(int& blk, int& bh) {
    const int nx = (int)gridDim.x, n = nx * (int)gridDim.y;
    const int id = (int)blockIdx.y * nx + (int)blockIdx.x;
    const int q = n >> 3, r = n & 7, xcd = id & 7;
    const int lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
    bh = lid / nx;
    blk = lid - bh * nx;
    if (REV) blk = nx - 1 - blk;
}

// 16-B fragment of row `row` of a row-major bf16 matrix, columns 16 ks + 8 (lane>>5) .. +7
__device__ __forceinline__ sv8 ld_frag(const bf16_t* base, int64_t ld, int64_t row, int ks, int lane) {
    return *(const sv8*)(base + row * ld + 16 * ks + 8 * (lane >> 5));
}

// store an O^T-layout accumulator pair (dims 32 dt + acc_row, one row per lane) as bf16, x mult
__device__ __forceinline__ void store_rows(bf16_t* row, const fv16 (&acc)[2], float mult, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* x = &((const float*)&acc[dt])[4 * i];
            *(uint2*)(row + 32 * dt + 8 * i + 4 * h) =
                make_uint2(pack_bf2(x[0] * mult, x[1] * mult), pack_bf2(x[2] * mult, x[3] * mult));
        }
}

// LDS-DMA (global_load_lds_dwordx4, common.h dma16) of one [64][64] bf16 tile -- rows row0..row0+63 of a row-major
// matrix -- into an aoff-swizzled image: 8 wave-instructions of 1 KB, two per wave.  LDS slot s of
// image row r holds global chunk s ^ X(r), so each lane fetches that chunk.
// img: 32-bit LDS byte address (lds_base of the __shared__ array + an offset), wave wave-uniform; the
// source as a wave-uniform base + per-lane byte offset (saddr form, common.h dma16sl)
__device__ __forceinline__ void dma_tile(const bf16_t* X, int64_t ldx, int64_t row0, uint32_t img, int wave, int lane) {
    const bf16_t* base = X + row0 * ldx;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ins = 2 * wave + i, r = 8 * ins + (lane >> 3), c = (lane & 7) ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3));
        dma16sl(base, (uint32_t)((r * ldx + 8 * c) * 2), img + 1024u * ins);
    }
}

// Tell hipcc that registers loaded by compiler-counted loads before a loop are ready here (after a
// hidden wait that drained them): otherwise its wait-count pass puts the s_waitcnt for them at their
// first use INSIDE the loop, where it runs every iteration -- vmcnt(0), which also waits for the
// next tile's DMAs issued at the iteration head (no prefetch left).
template <typename R>
__device__ __forceinline__ void ready1(const R& r) {
    asm volatile("" ::"v"(r));
}
template <typename... R>
__device__ __forceinline__ void mark_ready(const R&... r) {
    (ready1(r), ...);
}

// end of a ring tile: this wave's vector-memory operations older than the N DMA instructions just
// requested have landed, then every wave's (LDS reads drained too: the slot read now is rewritten
// after a later barrier)
template <int N>
__device__ __forceinline__ void ring_wait(bool pf) {
    if (pf) asm volatile("s_waitcnt vmcnt(%c0) lgkmcnt(0)\n\ts_barrier" ::"i"(N) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}


// =====================================================================================
// forward
// =====================================================================================
// S^T (64 keys x 32 queries) of one query group (rows qr..qr+31 of the block's Q image) against a
// K image: two independent MFMA chains, Q fragments read from LDS (not held in registers)
__device__ __forceinline__ void qk_tile(fv16 (&s)[2], const char* Ki, const char* Qimg, int qr, int lane) {
    s[0] = fv16{};
    s[1] = fv16{};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const sv8 qf = frag_row(Qimg, qr, ks, lane);
        s[0] = mfma32(frag_row(Ki, 0, ks, lane), qf, s[0]);
        s[1] = mfma32(frag_row(Ki, 32, ks, lane), qf, s[1]);
    }
}

// max over this lane's 32 scores (two interleaved v_max3 chains: a 2-input fmaxf of raw MFMA
// results would be preceded by canonicalising v_max x, x on each input), then over the lane^32
// partner (v_permlane32_swap: no LDS round trip)
template <int NSUB = 2>
__device__ __forceinline__ float tile_max(const fv16 (&s)[2]) {
    float m;
    if (NSUB == 2) {
        float m0 = fmaxf(fmaxf(s[0][0], s[0][1]), s[0][2]), m1 = fmaxf(fmaxf(s[1][0], s[1][1]), s[1][2]);
#pragma unroll
        for (int r = 3; r < 15; r += 2) {
            m0 = fmaxf(fmaxf(m0, s[0][r]), s[0][r + 1]);
            m1 = fmaxf(fmaxf(m1, s[1][r]), s[1][r + 1]);
        }
        m0 = fmaxf(fmaxf(m0, s[0][15]), s[1][15]);
        m = fmaxf(m0, m1);
    } else {
        float m0 = fmaxf(fmaxf(s[0][0], s[0][1]), s[0][2]), m1 = fmaxf(fmaxf(s[0][3], s[0][4]), s[0][5]);
#pragma unroll
        for (int r = 6; r < 14; r += 4) {
            m0 = fmaxf(fmaxf(m0, s[0][r]), s[0][r + 1]);
            m1 = fmaxf(fmaxf(m1, s[0][r + 2]), s[0][r + 3]);
        }
        m = fmaxf(fmaxf(m0, s[0][14]), fmaxf(m1, s[0][15]));
    }
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    return __builtin_amdgcn_fmed3f(__uint_as_float(sw[0]), __uint_as_float(sw[1]), INFINITY);   // max, no re-canonicalising
}

// lazy online-softmax rescale (threshold RESCALE_THR in log2 units): called after the group's
// previous tiles are all in O and l, before this tile is exponentiated
__device__ __forceinline__ void rescale_if(float mt, float& m_run, fv4& l_run, fv16 (&o)[2]) {
    if (__any(mt > m_run + RESCALE_THR)) {   // rare after the first tiles
        const float mn = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_run - mn);
        o[0] *= alpha;
        o[1] *= alpha;
        l_run *= alpha;
        m_run = mn;
    }
}

// The same for packed rows.  rescale_if moves the running max of EVERY lane once any lane of the wave
// asks for it, so a query's rounding would depend on the other segments that share its wave.  Here a
// lane moves iff a lane of its own segment asks (peers: seg_peers; lanes l and l + 32 hold the same
// query and vote alike), which is rescale_if itself when the wave holds one segment.  A lane whose
// keys so far were all masked has mt = -inf and m_run = -FLT_MAX: it never asks, and moved by a peer
// it keeps m_run (alpha = exp2(0)), so no exp2(-inf - -inf) arises.
__device__ __forceinline__ void rescale_if_seg(float mt, float& m_run, fv4& l_run, fv16 (&o)[2], uint32_t peers) {
    const uint64_t ask = __ballot(mt > m_run + RESCALE_THR);
    if (ask) {
        const bool move = (((uint32_t)ask | (uint32_t)(ask >> 32)) & peers) != 0;
        const float mn = move ? fmaxf(m_run, mt) : m_run;
        const float alpha = __builtin_amdgcn_exp2f(m_run - mn);
        o[0] *= alpha;
        o[1] *= alpha;
        l_run *= alpha;
        m_run = mn;
    }
}

// low / high 16 bits all-ones where bit j / j + 16 of a FWD keep word is set: v_lshlrev_b32 puts them
// at bits 15 / 31, v_perm_b32 selectors 8 / 9 replicate those bits over bytes 0-1 / 2-3
__device__ __forceinline__ uint32_t pair_mask(uint32_t w, int j) {
    const uint32_t x = w << (15 - j), sel = 0x09090808u;
    uint32_t m;
    // (the builtin form made hipcc emit an illegal v_cmp against src_shared_base in the forward ring kernel)
    asm("v_perm_b32 %0, %1, %1, %2" : "=v"(m) : "v"(x), "s"(sel));
    return m;
}

// P = exp2(S scale_log2 - m) of a tile's NSUB subtiles, packed to the bf16 B operands of
// O^T += V^T P^T; the row sums of the packed (undropped) P go to the matrix core (rowsum_ones), then
// the dropout keep bits are applied to the packed pairs: the pair j = 8 kt + 4 sk + i of fragment
// (kt, sk) has its keep bits at j and j + 16 of the FWD word, so w << (15 - j) puts them at bits 15
// and 31, v_perm_b32 selectors 8 / 9 replicate those into the low / high 16 bits, and one v_and_b32
// drops the pair's halves -- 3 instructions per pair instead of v_bfe_i32 + v_and_b32 per element
template <bool DROP, int NSUB = 2>
__device__ __forceinline__ void softmax_pack(fv16 (&s)[2], float scale_log2, float m_run, fv4& l_run, uint32_t mw,
                                             sv8 (&pf)[2][2], const sv8& ones) {
    const float mneg = -m_run;
#pragma unroll
    for (int kt = 0; kt < NSUB; ++kt) {
#pragma unroll
        for (int r = 0; r < 16; ++r)   // raw v_exp_f32: weights below 2^-126 of the stale max flush to 0
            s[kt][r] = __builtin_amdgcn_exp2f(fmaf(s[kt][r], scale_log2, mneg));
#pragma unroll
        for (int sk = 0; sk < 2; ++sk) {
            sv8 u = pack16(s[kt], sk);
            l_run = mfma16(ones, u, l_run);
            if (DROP) {
                const int j = 8 * kt + 4 * sk;
                uint4 w = __builtin_bit_cast(uint4, u);
                w.x &= pair_mask(mw, j);
                w.y &= pair_mask(mw, j + 1);
                w.z &= pair_mask(mw, j + 2);
                w.w &= pair_mask(mw, j + 3);
                u = __builtin_bit_cast(sv8, w);
            }
            pf[kt][sk] = u;
        }
    }
}

// O^T += V^T P^T over a 64-key tile's NSUB live subtiles (two independent chains, one per 32-dim half)
template <int NSUB = 2>
__device__ __forceinline__ void pv_tile(fv16 (&o)[2], const char* Vi, const sv8 (&pf)[2][2], int lane) {
#pragma unroll
    for (int kt = 0; kt < NSUB; ++kt)
#pragma unroll
        for (int sk = 0; sk < 2; ++sk) {
            o[0] = mfma32(frag_tr(Vi, 32 * kt, sk, 0, lane), pf[kt][sk], o[0]);
            o[1] = mfma32(frag_tr(Vi, 32 * kt, sk, 32, lane), pf[kt][sk], o[1]);
        }
}

// One query group's 64-key tile outside the pipeline: NSUB live 32-key subtiles (1 when the second
// lies wholly above the diagonal); DIAG = the subtile holding the diagonal (-1: none) -- the only
// one masked.  Straight-line code per case (the merged form copied accumulators between paths).
// QREG: the group's Q fragments come from registers (qreg[4]) instead of the Q image.
// SEG (packed rows): srel = the lane's segment start relative to the tile's first key, peers = the
// lanes of its segment (seg_peers); subtiles that begin before some lane's segment are masked below it.
template <bool DROP, int NSUB, int DIAG, bool QREG = false, bool SEG = false>
__device__ __forceinline__ void fwd_group_tile(const char* Ki, const char* Vi, const char* Qimg, int qr, int lane,
                                               float scale_log2, float& m_run, fv4& l_run, fv16 (&o)[2],
                                               uint32_t mw, const sv8& ones, const sv8* qreg = nullptr, int srel = 0,
                                               uint32_t peers = 0u) {
    fv16 s[2];
    s[0] = fv16{};
    s[1] = fv16{};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const sv8 qf = QREG ? qreg[ks] : frag_row(Qimg, qr, ks, lane);
        s[0] = mfma32(frag_row(Ki, 0, ks, lane), qf, s[0]);
        if (NSUB == 2) s[1] = mfma32(frag_row(Ki, 32, ks, lane), qf, s[1]);
    }
    if (DIAG >= 0) mask_upper(s[DIAG], lane & 31, 0, lane, -INFINITY);   // key0 = the group's first query
    if constexpr (SEG) {
#pragma unroll
        for (int kt = 0; kt < NSUB; ++kt)
            if (__any(srel > 32 * kt)) mask_before(s[kt], srel - 32 * kt, lane);
        rescale_if_seg(tile_max<NSUB>(s) * scale_log2, m_run, l_run, o, peers);
    } else {
        rescale_if(tile_max<NSUB>(s) * scale_log2, m_run, l_run, o);
    }
    sv8 pf[2][2];
    softmax_pack<DROP, NSUB>(s, scale_log2, m_run, l_run, mw, pf, ones);
    pv_tile<NSUB>(o, Vi, pf, lane);
}

// =====================================================================================
// dQ: S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (keep/(1-p) dP^T - delta), dQ^T += K^T dS^T.
// The 1/(1-p) is factored out of dS (dS = 1/(1-p) P (keep dP - (1-p) delta), applied with scale in
// the epilogue), so an element costs dP - delta', one v_bfi_b32 select (dropped: -delta') and P x.
// =====================================================================================
// one 64-key tile (K / V images, first key k0) of a dQ query group starting at query qg: its 32-key
// subtiles up to the diagonal; only the subtile whose first key is qg holds the diagonal
// SEG (packed rows): ss = the lane's segment start; subtiles wholly before every lane's segment are
// skipped, those that begin before some lane's are masked below it (P = exp2(-inf) = 0 there)
template <bool DROP, bool SEG = false>
__device__ __forceinline__ void dq_group_tile(const char* Ki, const char* Vi, int k0, int qg, const sv8 (&qf)[4],
                                              const sv8 (&df)[4], float lse2, float dl, uint32_t mw, float c2,
                                              fv16 (&dqa)[2], int lane, int ss = 0) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        if (k0 + 32 * kt > qg + 31) break;   // subtile fully masked
        if constexpr (SEG) {
            if (__all(ss >= k0 + 32 * kt + 32)) continue;
        }
        const bool diag = __builtin_amdgcn_readfirstlane(k0 + 32 * kt == qg);
        // dP^T starts from -delta' (its column's, lane-uniform), so the chain leaves dP - delta'
        fv16 s = fv16{}, dp = fv16{} + dl;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = mfma32(frag_row(Ki, 32 * kt, ks, lane), qf[ks], s);
            dp = mfma32(frag_row(Vi, 32 * kt, ks, lane), df[ks], dp);
        }
        if (diag) mask_upper(s, lane & 31, 0, lane, -INFINITY);
        if constexpr (SEG) {
            if (__any(ss > k0 + 32 * kt)) mask_before(s, ss - (k0 + 32 * kt), lane);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -lse2));
            float d = dp[r];
            if (DROP) d = keep_sel2(keep_mask(mw, fwd_bit(kt, r)), d, dl);
            s[r] = p * d;
        }
        const sv8 d0 = pack16(s, 0), d1 = pack16(s, 1);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            dqa[dt] = mfma32(frag_tr(Ki, 32 * kt, 0, 32 * dt, lane), d0, dqa[dt]);
            dqa[dt] = mfma32(frag_tr(Ki, 32 * kt, 1, 32 * dt, lane), d1, dqa[dt]);
        }
    }
}

// =====================================================================================
// dK / dV: S = Q K^T, dP = dO V^T with the key as the column
// =====================================================================================
// one 64-query tile (Q / dO images, their lse*log2e and -delta' rows) of a dK/dV key group starting
// at key kq (key = kq + (lane & 31)): the 32-query subtiles that reach the group's keys
// SEG (packed rows): se = the end (exclusive) of the segment of the lane's key; subtiles at or beyond
// every lane's segment end are skipped, those that reach past some lane's are masked from it on
template <bool DROP, bool SEG = false>
__device__ __forceinline__ void dkdv_tile(const char* Qi, const char* Oi, const float* st_lse, const float* st_del,
                                          int q0, int kq, int key, const sv8 (&kf)[4], const sv8 (&vf)[4], uint32_t mw,
                                          float c2, fv16 (&dka)[2], fv16 (&dva)[2], int lane, int se = 0) {
#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
        const int q0s = q0 + 32 * qs;
        if (q0s + 31 < kq) continue;   // every query of the subtile precedes every key
        if constexpr (SEG) {
            if (__all(se <= q0s)) continue;
        }
        // dP starts from -delta' of its rows (the accumulator's initial value), so the MFMA
        // chain leaves dP - delta'; dS = 1/(1-p) P (keep dP - delta'), the 1/(1-p) in the epilogue
        fv16 s = fv16{}, dp;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 d4 = *(const float4*)(st_del + 32 * qs + 8 * i + 4 * (lane >> 5));
            dp[4 * i] = d4.x;
            dp[4 * i + 1] = d4.y;
            dp[4 * i + 2] = d4.z;
            dp[4 * i + 3] = d4.w;
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = mfma32(frag_row(Qi, 32 * qs, ks, lane), kf[ks], s);
            dp = mfma32(frag_row(Oi, 32 * qs, ks, lane), vf[ks], dp);
        }
        if (__builtin_amdgcn_readfirstlane(q0s < kq + 31)) {
            // diagonal subtile: queries (rows) before the key (column) are masked
            const int rel = key - q0s - 4 * (lane >> 5);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((r & 3) + 8 * (r >> 2) < rel) s[r] = -INFINITY;
        }
        if constexpr (SEG) {
            if (__any(se < q0s + 32)) mask_from(s, se - q0s, lane);
        }
        fv16 z;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // rows 8i + 4(lane>>5) + 0..3 of the subtile: one 16-B LDS read each (broadcast)
            const int row = 32 * qs + 8 * i + 4 * (lane >> 5);
            const float4 l4 = *(const float4*)(st_lse + row);
            const float4 d4 = *(const float4*)(st_del + row);
            const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dvv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * i + e;
                const float p = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -lv[e]));
                float d = dp[r];   // dP - delta'
                if (DROP) {
                    const uint32_t kp = keep_mask(mw, 16 * qs + r);   // 1/(1-p) of dV: epilogue
                    z[r] = __uint_as_float(__float_as_uint(p) & kp);
                    d = keep_sel2(kp, d, dvv[e]);                     // dropped: -delta'
                } else {
                    z[r] = p;
                }
                s[r] = p * d;
            }
        }
        const sv8 z0 = pack16(z, 0), z1 = pack16(z, 1), s0 = pack16(s, 0), s1 = pack16(s, 1);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            dva[dt] = mfma32(frag_tr(Oi, 32 * qs, 0, 32 * dt, lane), z0, dva[dt]);
            dva[dt] = mfma32(frag_tr(Oi, 32 * qs, 1, 32 * dt, lane), z1, dva[dt]);
            dka[dt] = mfma32(frag_tr(Qi, 32 * qs, 0, 32 * dt, lane), s0, dka[dt]);
            dka[dt] = mfma32(frag_tr(Qi, 32 * qs, 1, 32 * dt, lane), s1, dka[dt]);
        }
    }
}

// O^T accumulator pair of one query (lane & 31; dims 32 dt + acc_row) as bf16, x mult, in 16-B
// row segments: lanes l and l + 32 hold the two 4-dim halves of each 8-dim group, so for each
// pair of groups (i, i + 1) one v_permlane32_swap per dword leaves lanes 0-31 with dims 8i..8i+7
// and lanes 32-63 with 8(i+1)..8(i+1)+7 (cdna_hip_programming.md T21): 4 dwordx4 stores per lane
// instead of 8 dwordx2.  Same bytes as store_rows.
__device__ __forceinline__ void store_rows_wide(bf16_t* row, const fv16 (&acc)[2], float mult, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            const float* x = &((const float*)&acc[dt])[4 * i];
            const float* y = &((const float*)&acc[dt])[4 * i + 4];
            const uint32_t a0 = pack_bf2(x[0] * mult, x[1] * mult), a1 = pack_bf2(x[2] * mult, x[3] * mult);
            const uint32_t b0 = pack_bf2(y[0] * mult, y[1] * mult), b1 = pack_bf2(y[2] * mult, y[3] * mult);
            const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
            *(uint4*)(row + 32 * dt + 8 * (i + h)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
        }
}

}  // namespace

}  // namespace cg
