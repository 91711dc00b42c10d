/*
 * charpt -- MI355X-native (gfx950/CDNA4) kernels for the char-level GPT hot path of
 * ChaitIITB/ReplicatingGPT GPT1.py.  C ABI of libcharpt_hip.so.
 *
 * The reference has no native plugin API: its replaceable seam is the nn.Module surface and
 * the aten ops those modules call.  Every entry point below replaces one or
 * more of those aten call sites; the citation on each names the GPT1.py line(s) it stands in
 * for.  Python binds these through ctypes (replicatinggpt_amd/_lib.py) and registers them as
 * torch.library custom ops (replicatinggpt_amd/ops.py).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless noted; the caller (PyTorch's caching allocator)
 *     owns every buffer; the library never allocates, frees or synchronises the host.
 *   - every function is stream-ordered on `stream` (a hipStream_t, passed as void*), so it is
 *     capturable into a hipGraph.
 *   - state: the library keeps no per-call state except the DEFERRED WORK below and the
 *     cg_set_tuning knobs, which only select kernels / schedules for A/B and test runs (never the
 *     numerics of a call: precision and deferral are per-call flags).
 *   - deferred work (per stream): a call asks for it explicitly -- cg_epilogue_t.flags
 *     CG_GEMM_DEFER_REDUCE (a split-K weight-gradient reduce left pending), cg_adamw_defer, and the
 *     CG_DEFER flag of cg_reduce_rows_ex / cg_layernorm_bwd_reduce_ex / cg_head_bwd_ex (column-sum
 *     reduces queued for one multi-job launch).  The queue is that of the call's stream, keyed by
 *     (the stream's own device, stream) whatever device is current in the calling thread: only a
 *     later persistent GEMM launch on the SAME stream takes its jobs (in its tail / free blocks),
 *     and cg_flush_deferred(stream) launches the rest on that stream, with the stream's device made
 *     current for the launches (the caller's restored).  A flushed or discarded queue is dropped,
 *     so a new stream that reuses a destroyed stream's handle starts with an empty one.  A mutex guards the
 *     queue registry, so host threads that each drive their own stream are safe; two threads
 *     sharing one stream must order their calls themselves, as with any stream.  Until the flush,
 *     the caller keeps every queued job's workspace alive and reads none of its outputs.
 *   - memory footprint: a call writes only the listed elements of its outputs (rows r, columns 0..width-1
 *     at r * ld; never the ld - width padding of a row, nor past the last row) and only the bytes its
 *     *_workspace() function states of its workspace; it reads nothing outside the logical extent of its
 *     inputs whose value can affect the result (so padding and neighbouring memory may hold anything, NaN
 *     included); it never modifies a const operand; and what outputs (where it writes, not accumulates)
 *     and workspaces hold on entry is irrelevant: a workspace needs no initialisation.  A call refused
 *     with CG_EINVAL for its shapes, strides or alignment has written nothing.
 *     tests/test_gpu_footprint.py holds the training-path entry points to this on guard-banded, padded
 *     and misaligned operands.
 *   - cg_last_error_string() is per thread.
 *   - return CG_OK (0) or an error code; cg_last_error_string() gives the message.
 *   - dtype codes: CG_F32 = 0 (float), CG_BF16 = 1 (bfloat16 bits, RNE rounding).
 *   - dropout: Philox4x32-10 counter RNG, spec in oracle/philox.py and DESIGN.md; the stream id
 *     is ((*rng_call) << 8) | site, with rng_call a device uint64 snapshot per forward call.
 */
#ifndef CHARPT_H
#define CHARPT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CG_OK = 0, CG_EINVAL = 1, CG_EHIP = 2, CG_EUNSUPPORTED = 3 };
enum { CG_F32 = 0, CG_BF16 = 1 };
/* cg_epilogue_t.aux_dtype only: ReLU keep bits, uint32 words [M][ld_aux], bit n % 32 of word n / 32
   of row m = (bf16 ReLU output (m, n) != 0).  CG_EPI_BIAS_RELU WRITES them (aux is an output there),
   CG_EPI_RELU_BWD reads them instead of the bf16 ReLU output (1/16 of its bytes).  Only where
   cg_gemm_relu_bits_supported() says so (bf16, split 1, beta 0, N % 64 == 0, persistent kernels) and
   the words are 8-B aligned with an even ld_aux (a row's 64 columns are one 8-B access); elsewhere
   cg_gemm returns CG_EINVAL. */
enum { CG_BITS = 2 };

/* GEMM epilogues (applied to acc = sum_k A(m,k) B(n,k), per output element (m,n)) */
enum {
    CG_EPI_STORE = 0,        /* out = acc                                                       */
    CG_EPI_BIAS = 1,         /* out = acc + bias[n]                                             */
    CG_EPI_BIAS_RELU = 2,    /* out = relu(acc + bias[n])               (GPT1.py:143-144)       */
    CG_EPI_BIAS_RESID = 3,   /* out = resid[m,n] + acc + bias[n]  (resid NULL: no add; :136,163) */
    CG_EPI_BIAS_DROP_RESID = 4, /* out = resid + dropout(acc + bias)    (GPT1.py:145-146,164)   */
    CG_EPI_RELU_BWD = 5,     /* out = acc * (aux[m,n] > 0)              (ReLU backward, :144)   */
    /* 6 unused.  out = acc (bf16), and the attention backward's delta = rowsum(dO * O) per head from
       the written values: colpart[((m / T) * (N / 64) + n / 64) * T + m % T] = sum over the head's 64
       columns of bf16(acc) * aux[m, n]  (aux = the attention output O, bf16, stride ld_aux;
       T = ld_resid, M % T == 0).  Only where cg_gemm_rowdot_supported() says so.               */
    CG_EPI_STORE_ROWDOT = 7
};

typedef struct {
    int kind;                 /* CG_EPI_*                                                    */
    const float* bias;        /* [N] fp32 or NULL                                            */
    const float* resid;       /* fp32, row stride ld_resid                                   */
    int64_t ld_resid;
    const void* aux;          /* CG_EPI_RELU_BWD: relu output, dtype aux_dtype, stride ld_aux */
    int aux_dtype;
    int64_t ld_aux;
    double dropout_p;         /* CG_EPI_BIAS_DROP_RESID                                      */
    uint64_t seed;
    const uint64_t* rng_call; /* device scalar                                               */
    int site;
    float beta;               /* out = epi(acc) + beta * out   (beta in {0,1}: grad accumulate) */
    float* colpart;           /* CG_EPI_RELU_BWD, bf16, beta 0, split 1 only, and only where the
                                 dispatch takes the 128x128 persistent kernel (else CG_EINVAL):
                                 column sums of each 64-row block of the output (of its bf16-
                                 rounded values, as cg_colsum would see them), [M/64][N] -- the consumer's bias-gradient partials,
                                 folded by cg_reduce_rows.  NULL: none.                     */
    int flags;                /* CG_GEMM_* below; 0 = plain (fp32 slabs, reduce in this call) */
} cg_epilogue_t;

/* cg_epilogue_t.flags -- split-K (split_k > 1) fp32 CG_EPI_STORE outputs (the weight gradients):
   CG_GEMM_SLAB_BF16     each split's partial sum is stored as a bf16 slab (rounded once, 2^-9
                         relative) and the slabs are summed in split order in fp32: half the slab
                         bytes.  Applies where the 128x128 persistent kernel runs the product (bf16
                         operands, vectorisable output); elsewhere the call uses fp32 slabs.
   CG_GEMM_DEFER_REDUCE  the slab reduce may stay pending on the stream's deferral queue (above):
                         the next persistent bf16 GEMM on the stream sums it in its tail, or
                         cg_flush_deferred(stream).  Keep the workspace alive until then.  Calls the
                         deferral does not apply to (slab sets > 40 MB) reduce now.                */
enum { CG_GEMM_SLAB_BF16 = 1, CG_GEMM_DEFER_REDUCE = 2 };
/* flags of the _ex column-sum reduces: queue on the stream's deferral queue instead of launching */
enum { CG_DEFER = 1 };

const char* cg_last_error_string(void);
int cg_version(void);
/* process-wide A/B and test knobs (kernel / schedule selection, never a call's numerics): e.g.
   "gemm_variant" 0 = automatic, 2 = register-staged, 9 = persistent 128x128, 24 = 8-wave 256x256,
   31 = the weight-stationary kernel for K <= 384 (whatever it takes, the rest as 2), 97 / 98 = fp32
   small-M chunked kernel / 128x64 kernel only, 99 = generic; "gemm_ws" 0 / 1 = the automatic use of
   the weight-stationary kernel off / on (2, 3, 4: one product only, for A/B); "decode_attn_rows",
   "red_side", "adam_per_launch", "gemm_n96", "ln_nt", ... (gemm.hip cg_set_tuning).
   Set them before the calls they affect, from one thread.                                       */
int cg_set_tuning(const char* key, int value);
/* launches cg_gemm has run through the weight-stationary kernel (gemm_ws.hip) in this process: for
   tests and A/B tools that must know which kernel served a call                                  */
int64_t cg_gemm_ws_launches(void);
/* resident blocks per CU (the runtime's occupancy query) of the weight-stationary instantiation that a
   product with this B layout, epilogue kind and K / 64 runs (the kernel is built for two 4-wave blocks
   per CU); -1 if there is none                                                                       */
int cg_gemm_ws_blocks_per_cu(int b_trans, int kind, int nkt);
int cg_device_info(int* n_cu, int* arch_major, int* arch_minor);
/* measurement (bench.py's in-step roofline): a timing event recorded on `stream` -- inside a
   hipGraph capture as an EXTERNAL event-record node (hipEventRecordExternal), so that each replay
   re-records it and two such events time the kernels captured between them on that stream.
   cg_timing_event_elapsed: milliseconds between two recorded events (after they completed).     */
int cg_timing_event_create(void** event);
int cg_timing_event_record(void* event, void* stream);
int cg_timing_event_elapsed(void* start, void* end, float* ms);
int cg_timing_event_destroy(void* event);

/* ---- utility ------------------------------------------------------------------------ */
/* *counter += delta (one thread); snapshot variant: *snap = *counter, *counter += 1.       */
int cg_counter_add(int64_t* counter, int64_t delta, void* stream);
int cg_rng_snapshot(uint64_t* counter, uint64_t* snap, void* stream);
/* dst[i] = dropout keep-mask (1.0 / 0.0) for element i in [0,n), for tests of the RNG.    */
int cg_dropout_mask(float* dst, int64_t n, double p, uint64_t seed, const uint64_t* rng_call, int site,
                    void* stream);
/* y[r,c] = x[r,c] * keep(r*C+c) * 1/(1-p)  (dropout backward / apply; p=0 -> plain cast);
   x fp32 [rows, C] (row stride ldx), y dtype y_dtype [rows, C] contiguous.                  */
int cg_dropout_apply(const float* x, int64_t rows, int64_t C, int64_t ldx, void* y, int y_dtype, double p,
                     uint64_t seed, const uint64_t* rng_call, int site, void* stream);
/* deterministic sum of n floats into *out (two-pass); ws >= 1024 floats; out = scale*sum   */
int cg_sum_f32(const float* x, int64_t n, float scale, float* out, float* ws, void* stream);
/* fp32 -> bf16 cast (RNE), n elements                                                       */
int cg_cast_f32_bf16(const float* x, uint16_t* y, int64_t n, void* stream);

/* ---- data: get_batch on device (GPT1.py:75-83) ---------------------------------------- */
/* x[b,t] = data[ix[b]+t], y[b,t] = data[ix[b]+t+1]; data is the token stream (int64 or uint8) */
int cg_gather_batch(const void* data, int data_is_u8, const int64_t* ix, int64_t* x, int64_t* y,
                    int64_t B, int64_t T, void* stream);

/* (prompt, completion) rows for fine-tuning.  table int64 [N, T+1]: row n holds tlen[n] <= T+1 packed
   tokens, the first plen[n] of them the prompt (1 <= plen < tlen); ix[B] row indices in [0, N).
   x[b,j] = table[ix[b], j] for j < tlen-1, else pad_token;
   y[b,j] = table[ix[b], j+1] when plen <= j+1 < tlen, else ignore_index.  x, y int64 [B, T] dense. */
int cg_gather_pairs(const int64_t* table, const int64_t* plen, const int64_t* tlen, const int64_t* ix, int64_t* x,
                    int64_t* y, int64_t B, int64_t T, int64_t pad_token, int64_t ignore_index, void* stream);

/* ---- embeddings (GPT1.py:179-181) ------------------------------------------------------ */
/* x[b,t,:] = wte[idx[b,t],:] + wpe[t,:]  (fp32)                                          */
int cg_embed_fwd(const int64_t* idx, const float* wte, const float* wpe, float* x, int64_t B, int64_t T,
                 int64_t C, int64_t V, void* stream);
/* dwte[v,:] (=|+=) sum_{idx=v} dx ; dwpe[t,:] (=|+=) sum_b dx[b,t,:]   deterministic.
   workspace: cg_embed_bwd_workspace(B,T,C,V) bytes.                                          */
int64_t cg_embed_bwd_workspace(int64_t B, int64_t T, int64_t C, int64_t V);
int cg_embed_bwd(const int64_t* idx, const float* dx, float* dwte, float* dwpe, int64_t B, int64_t T,
                 int64_t C, int64_t V, int accumulate, void* workspace, void* stream);

/* ---- packed rows: several (prompt, completion) pairs per row --------------------------------
   A row of T tokens is a concatenation of segments, described by seg_start int32 [B, T]:
   seg_start[b,t] = the index of the first token of the segment that holds position t -- non-decreasing
   along a row, constant on a segment, <= t.  cg_seg_bounds derives seg_end[b,t] (int32 [B, T], the
   exclusive end of t's segment) on the device; one launch per forward serves every layer.
   Positions restart at each segment: x[b,t,:] = wte[idx[b,t],:] + wpe[t - seg_start[b,t],:], and
   dwpe[p,:] (=|+=) the sum of dx[b,t,:] over all (b, t) with t - seg_start[b,t] = p, in (b, segment)
   order -- deterministic, any T; dwte as cg_embed_bwd (same workspace).  Out-of-contract bounds are
   clamped (position into [0, T), seg_end into (t, T]): wrong numbers, never an access outside the
   operands.  Attention with the same mask: cg_attn_fwd_seg / cg_attn_bwd_seg below.              */
int cg_seg_bounds(const int32_t* seg_start, int32_t* seg_end, int64_t B, int64_t T, void* stream);
int cg_embed_fwd_seg(const int64_t* idx, const int32_t* seg_start, const float* wte, const float* wpe, float* x,
                     int64_t B, int64_t T, int64_t C, int64_t V, void* stream);
int cg_embed_bwd_seg(const int64_t* idx, const int32_t* seg_end, const float* dx, float* dwte, float* dwpe,
                     int64_t B, int64_t T, int64_t C, int64_t V, int accumulate, void* workspace, void* stream);

/* ---- LayerNorm (nn.LayerNorm, GPT1.py:159-160,173) -------------------------------------- */
/* y = (x-mu)*rstd*w + b, biased variance, eps; y dtype y_dtype; saves mean/rstd [rows]     */
int cg_layernorm_fwd(const float* x, const float* w, const float* b, void* y, int y_dtype, float* mean,
                     float* rstd, int64_t rows, int64_t C, float eps, void* stream);
/* dx = dres + LN'(dy)  (dres may be NULL); dx_bf16 optional bf16 copy of dx;
   dw/db (=|+=) column sums; workspace: cg_layernorm_bwd_workspace(rows,C) bytes.           */
int64_t cg_layernorm_bwd_workspace(int64_t rows, int64_t C);
int cg_layernorm_bwd(const void* dy, int dy_dtype, const float* x, const float* w, const float* mean,
                     const float* rstd, const float* dres, float* dx, uint16_t* dx_bf16, float* dw, float* db,
                     int accumulate, void* workspace, int64_t rows, int64_t C, void* stream);
/* the same, with the consumer-side extras: lp_out = bf16(keep ? dx / (1 - p) : 0) (keep from the
   Philox stream (lp_seed, lp_rng_call, lp_site), element idx = r*C + c; p = 0: plain bf16 copy) and
   lp_colsum (+)= column sums of that tensor (fp32, before rounding).                              */
int cg_layernorm_bwd_ex(const void* dy, int dy_dtype, const float* x, const float* w, const float* mean,
                        const float* rstd, const float* dres, float* dx, uint16_t* lp_out, double lp_dropout_p,
                        uint64_t lp_seed, const uint64_t* lp_rng_call, int lp_site, float* dw, float* db,
                        float* lp_colsum, int accumulate, int colsum_accumulate, void* workspace, int64_t rows,
                        int64_t C, void* stream);
/* cg_layernorm_bwd_ex in two launches, so the column-sum reduce can run off the critical path:
   _rows writes dx / lp_out and leaves the per-block column partials (dw, db, and with lp_colsum=1
   the lp_out column sums) in the workspace; _reduce (any stream ordered after _rows) folds them
   into dw / db / lp_colsum exactly as cg_layernorm_bwd_ex does (same order, same bits).       */
int cg_layernorm_bwd_rows(const void* dy, int dy_dtype, const float* x, const float* w, const float* mean,
                          const float* rstd, const float* dres, float* dx, uint16_t* lp_out, double lp_dropout_p,
                          uint64_t lp_seed, const uint64_t* lp_rng_call, int lp_site, int lp_colsum,
                          void* workspace, int64_t rows, int64_t C, void* stream);
int cg_layernorm_bwd_reduce(const void* workspace, int64_t rows, int64_t C, int lp_colsum_partials, float* dw,
                            float* db, float* lp_colsum, int accumulate, int colsum_accumulate, void* stream);
/* the same with flags: CG_DEFER queues the reduce on the stream's deferral queue                */
int cg_layernorm_bwd_reduce_ex(const void* workspace, int64_t rows, int64_t C, int lp_colsum_partials, float* dw,
                               float* db, float* lp_colsum, int accumulate, int colsum_accumulate, int flags,
                               void* stream);

/* ---- GEMM (nn.Linear fwd/dgrad/wgrad: GPT1.py:111-112,121,136,143,145,184) -------------
   C[m,n] = epilogue( sum_k A(m,k) * B(n,k) )
   A(m,k) = A[m*lda+k] (a_trans=0) or A[k*lda+m] (a_trans=1); same for B with b_trans.
   op_dtype: CG_BF16 (bf16 MFMA, fp32 accumulate) or CG_F32 (exact-f32 MFMA).
   c_dtype: output dtype.  split_k > 1 (CG_EPI_STORE/BIAS only) needs workspace of
   cg_gemm_workspace(M,N,split_k) bytes; results are deterministic for any split_k.            */
int64_t cg_gemm_workspace(int64_t M, int64_t N, int split_k);
/* 1 if cg_gemm (bf16, split_k 1, CG_EPI_RELU_BWD with bf16 aux, beta 0) can fill epi->colpart for
   this problem under the current dispatch and tuning knobs (16-B aligned operands assumed), else 0
   -- the caller then computes the bias gradient with cg_colsum instead.                          */
int cg_gemm_colpart_supported(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                              int64_t ldc);
/* 1 if cg_gemm can write (CG_EPI_BIAS_RELU) and read (CG_EPI_RELU_BWD) CG_BITS ReLU keep bits for
   this non-transposed-A bf16 problem (split 1, beta 0) under the current dispatch, else 0.  The
   FeedForward uses them when both its W1 forward and its W2 dgrad products say yes.           */
int cg_gemm_relu_bits_supported(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                int64_t ldc);
/* 1 if cg_gemm can run CG_EPI_STORE_ROWDOT (bf16 output, split 1, beta 0, N % 64 == 0) for this
   problem under the current dispatch, else 0 -- the attention backward then computes delta itself. */
int cg_gemm_rowdot_supported(int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                             int64_t ldc);
/* launch everything still pending on `stream`'s deferral queue (split-K reduces, AdamW jobs, the
   queued column-sum reduces as one launch) on that stream; call it before reading the outputs.
   Same summation order as the in-call forms, so the same bits.                                  */
int cg_flush_deferred(void* stream);
/* drop everything pending on `stream`'s queue without launching it (a failed backward: its
   gradients are abandoned).  *adam_jobs_taken (may be NULL) = the AdamW jobs GEMM launches
   already took from this queue since its last flush / discard -- updates that have run or will
   run; 0 means no parameter has been touched.                                                   */
int cg_discard_deferred(void* stream, int* adam_jobs_taken);
/* out[n] (=|+=) sum_r part[r*N + n] over rows r in order (fixed order: deterministic)          */
int cg_reduce_rows(const float* part, int64_t rows, int64_t N, float* out, int accumulate, void* stream);
int cg_reduce_rows_ex(const float* part, int64_t rows, int64_t N, float* out, int accumulate, int flags,
                      void* stream);
int cg_gemm(int op_dtype, int a_trans, int b_trans, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda,
            const void* B, int64_t ldb, void* C, int c_dtype, int64_t ldc, const cg_epilogue_t* epi, int split_k,
            void* workspace, void* stream);
/* Several split-K weight gradients (dW = dy^T x) as ONE launch of the 128x128 persistent bf16 kernel
   (the attention sublayer's projection and QKV weights: GPT1.py:111-112,136).  Problem i is the call
       cg_gemm(CG_BF16, 1, 1, M, N, K, A, lda, B, ldb, C, CG_F32, ldc, {CG_EPI_STORE, beta, flags}, split_k,
               workspace, stream)
   -- A [K][M] and B [K][N] bf16, C [M][N] fp32 (+= beta C), split_k >= 2, workspace of
   cg_gemm_workspace(M, N, split_k) bytes, flags CG_GEMM_SLAB_BF16 / CG_GEMM_DEFER_REDUCE -- and its C
   equals that call's bit for bit; its slab reduce runs or stays pending as that call's would.  The
   launch's item list is the problems' item lists one after the other, so splits chosen over the sum of
   the problems' tiles fill the machine in one round where each problem alone could not.
   cg_gemm_wgrad_group_supported: 1 if every problem is one the persistent kernel takes under the
   current dispatch (M, N % 128 == 0, K % 64 == 0, no empty split, 16-B aligned operands, ld % 8 == 0)
   and all use the same slab type; otherwise cg_gemm_wgrad_group returns CG_EINVAL and the caller
   issues the cg_gemm calls.                                                                    */
enum { CG_GEMM_GROUP_MAX = 4 };
typedef struct {
    int64_t M, N, K;
    const void* A;
    int64_t lda;
    const void* B;
    int64_t ldb;
    float* C;
    int64_t ldc;
    float beta;
    int split_k;
    void* workspace;
    int flags;                /* CG_GEMM_SLAB_BF16 | CG_GEMM_DEFER_REDUCE */
} cg_wgrad_problem_t;
int cg_gemm_wgrad_group_supported(const cg_wgrad_problem_t* problems, int n);
int cg_gemm_wgrad_group(const cg_wgrad_problem_t* problems, int n, void* stream);
/* A residual-stream GEMM with the LayerNorm that reads its output, in one launch (the attention
   projection + ln2, the FFN's second Linear + the next block's ln1 / ln_f: GPT1.py:136,145-147,
   159-160,163-164,173): out = resid + [dropout](A W^T + bias) (fp32; epi kind CG_EPI_BIAS_RESID or
   CG_EPI_BIAS_DROP_RESID with bias and resid, beta 0, flags 0), and y = LN(out; ln_w, ln_b) (bf16,
   row stride N), mean, rstd -- bit for bit cg_gemm followed by cg_layernorm_fwd.  A [M][K] and
   W [N][K] bf16 (lda, ldw), 16-B aligned operands.  Only where
   cg_gemm_resid_layernorm_supported(M, N, K) says 1 (N == 384, M % 64 == 0, K % 64 == 0);
   otherwise CG_EINVAL.                                                                         */
int cg_gemm_resid_layernorm_supported(int64_t M, int64_t N, int64_t K);
int cg_gemm_resid_layernorm(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw,
                            float* out, int64_t ldc, const cg_epilogue_t* epi, const float* ln_w, const float* ln_b,
                            void* y, float* mean, float* rstd, float eps, void* stream);
/* A Linear over rows of K <= 128 for inference, fp32, optionally with the LayerNorm before it in the
   same launch: out = [resid +] act(a' W^T [+ bias]), a' = LayerNorm(a; ln_w, ln_b, eps) (ln_w, ln_b
   non-NULL: the block's ln1 before the QKV product, GPT1.py:111-112,163; ln2 before FFN1, lnf before
   lm_head) or a' = a; act = relu when relu != 0 (needs bias, no resid); a [M][K] (lda), W [N][K]
   (ldw), resid / out [M][N] (ldr / ldo) -- bit for bit [cg_layernorm_fwd +] cg_gemm (fp32,
   CG_EPI_STORE / CG_EPI_BIAS / CG_EPI_BIAS_RELU / CG_EPI_BIAS_RESID), without the normalised rows in
   memory.  Only where cg_linear_rows_f32_supported(M, N, K) says 1 (K <= 128 even; above 2048 rows
   N <= 2048 even); lda / ldw even, a / W 8-B aligned and, with the LayerNorm, ln_w / ln_b 8-B aligned
   (cg_layernorm_fwd sums a row in this launch's order only then); above 2048 rows also ldo / ldr
   even, out / resid 8-B aligned and, with the LayerNorm, lda == K; else CG_EINVAL.                */
int cg_linear_rows_f32_supported(int64_t M, int64_t N, int64_t K);
int cg_linear_rows_f32(int64_t M, int64_t N, int64_t K, const float* a, int64_t lda, const float* ln_w,
                       const float* ln_b, float eps, const float* w, int64_t ldw, const float* bias, int relu,
                       const float* resid, int64_t ldr, float* out, int64_t ldo, void* stream);
/* generate()'s per-token ln1 + QKV product + K/V cache append (GPT1.py:111-113,163 for the newest
   token of each row; the decode engine's phase 1), fp32, one launch: qkv = LayerNorm(x; ln_w, ln_b,
   eps) W^T (x [B][C] (ldx), W [3C][C] (ldw), qkv [B][3C] (ldq)), and columns C..3C-1 of row b also
   to kcache / vcache [B][H][Tmax][C/H] at position *len_dev - 1 -- bit for bit cg_linear_rows_f32
   (with the LayerNorm) then cg_decode_kv_append(qkv, ldq, C, 2C, ...).  B <= 2048, C <= 128 even,
   H | C, ldx / ldw even, x / W / ln_w / ln_b 8-B aligned; else CG_EINVAL.                        */
int cg_decode_qkv_f32(int64_t B, int64_t C, int64_t H, const float* x, int64_t ldx, const float* ln_w,
                      const float* ln_b, float eps, const float* w, int64_t ldw, float* qkv, int64_t ldq,
                      const int64_t* len_dev, int64_t Tmax, float* kcache, float* vcache, void* stream);
/* The FeedForward sublayer's forward for inference (GPT1.py:142-147,164 in eval, no dropout), fp32,
   in one launch: out = resid + (relu(a' W1^T + b1) W2^T + b2) with a' = LayerNorm(a; ln_w, ln_b,
   eps) (ln_w, ln_b non-NULL: the block's ln2, GPT1.py:164) or a' = a (both NULL); a [M][C] (lda),
   W1 [H][C] (ldw1), W2 [C][H] (ldw2), resid / out [M][C] (ldr / ldo; out may alias resid) -- bit for
   bit cg_layernorm_fwd, cg_gemm (fp32, CG_EPI_BIAS_RELU) into an [M][H] buffer and cg_gemm
   (CG_EPI_BIAS_RESID), without the normalised rows or the hidden activations in memory.  Only where
   cg_ffn_fwd_f32_supported(M, C, H) says 1 (C <= 128 even, H <= 2048 even); lda / ldw1 / ldw2 even,
   a / W1 / W2 8-B aligned (with the LayerNorm also ln_w / ln_b, and lda == C); else CG_EINVAL.  (Replaces, in generate()'s window, FeedForward.net's
   two Linear calls and the ln2 before them.)                                                    */
int cg_ffn_fwd_f32_supported(int64_t M, int64_t C, int64_t H);
int cg_ffn_fwd_f32(int64_t M, int64_t C, int64_t H, const float* a, int64_t lda, const float* ln_w, const float* ln_b,
                   float eps, const float* w1, int64_t ldw1, const float* b1, const float* w2, int64_t ldw2,
                   const float* b2, const float* resid, int64_t ldr, float* out, int64_t ldo, void* stream);
/* column sums of a [rows, N] matrix (bias gradients): out[n] (=|+=) sum_m X[m,n]            */
int64_t cg_colsum_workspace(int64_t rows, int64_t N);
int cg_colsum(const void* X, int x_dtype, int64_t rows, int64_t N, int64_t ldx, float* out, int accumulate,
              void* workspace, void* stream);

/* ---- causal self-attention, all heads (Head.forward GPT1.py:109-123 x n_head, :135) -------
   q/k/v element (b,t,h,e) at ptr[(b*T+t)*ld_qkv + h*D + e]; o at o[(b*T+t)*ld_o + h*D + e].
   P = softmax(mask(q k^T * scale)); P = dropout(P); o = P v.  lse[b,h,t] (fp32) saved.      */
int cg_attn_fwd(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                const void* v, int64_t ld_qkv, void* o, int64_t ld_o, float* lse, float scale, double dropout_p,
                uint64_t seed, const uint64_t* rng_call, int site, uint64_t* mask, void* stream);
/* the same with the keep bits already in `mask` (cg_attn_dropmask, e.g. launched ahead on another
   stream so the Philox work overlaps earlier kernels); identical results to cg_attn_fwd.        */
int cg_attn_fwd_premasked(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                          const void* v, int64_t ld_qkv, void* o, int64_t ld_o, float* lse, float scale,
                          double dropout_p, uint64_t seed, const uint64_t* rng_call, int site, uint64_t* mask,
                          void* stream);
/* fill the MFMA path's keep-bit buffer for one attention call (0 < p < 1, T % 64 == 0)          */
int cg_attn_dropmask(int64_t B, int64_t H, int64_t T, double dropout_p, uint64_t seed, const uint64_t* rng_call,
                     int site, uint64_t* mask, void* stream);
/* one launch for a sublayer's LayerNorm forward (cg_layernorm_fwd arguments, GPT1.py:163 ln1) and
   the keep bits of the attention it feeds (cg_attn_dropmask arguments): the two are independent and
   the launch runs them side by side on the CUs (Philox VALU work under the LayerNorm's memory time).
   Results identical to cg_layernorm_fwd followed by cg_attn_dropmask; shapes without a fused form
   (y not bf16, C not 384 / 768, unaligned) take those two launches.                             */
int cg_layernorm_fwd_attn_dropmask(const float* x, const float* w, const float* b, void* y, int y_dtype, float* mean,
                                   float* rstd, int64_t rows, int64_t C, float eps, int64_t B, int64_t H, int64_t T,
                                   double dropout_p, uint64_t seed, const uint64_t* rng_call, int site,
                                   uint64_t* mask, void* stream);
/* keep-bit buffer for dropout on the MFMA (bf16, head_size 64) path: the forward fills it from the
   Philox stream (cg_attn_fwd `mask`, may be NULL on the generic path or with p = 0) and the
   backward reads it (cg_attn_bwd `mask`; NULL -> regenerated inside the workspace).  Layout
   (attention_common.h): per (b*H + h), T/32 + (T/32 - 1)^2/4 tiles of 64 x 32-bit lane words in
   each of two orientations (query-major for the forward / dQ, key-major for dK/dV).            */
int64_t cg_attn_mask_bytes(int64_t B, int64_t H, int64_t T);
/* dq/dk/dv written (not accumulated) with stride ld_dqkv; workspace cg_attn_bwd_workspace. */
int64_t cg_attn_bwd_workspace(int64_t B, int64_t T, int64_t H, int64_t D);
int cg_attn_bwd(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                const void* v, int64_t ld_qkv, const void* o, int64_t ld_o, const void* dout, int64_t ld_do,
                const float* lse, void* dq, void* dk, void* dv, int64_t ld_dqkv, float scale, double dropout_p,
                uint64_t seed, const uint64_t* rng_call, int site, const uint64_t* mask, void* workspace,
                void* stream);
/* cg_attn_bwd with delta = rowsum(dO * O) already computed (fp32 [B][H][T], e.g. by the dO GEMM's
   CG_EPI_STORE_ROWDOT epilogue); the sequence-resident kernels (T <= 256) read it instead of
   loading O, other paths recompute it in the workspace.  NULL delta: exactly cg_attn_bwd.         */
int cg_attn_bwd_delta(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                      const void* v, int64_t ld_qkv, const void* o, int64_t ld_o, const void* dout, int64_t ld_do,
                      const float* lse, const float* delta, void* dq, void* dk, void* dv, int64_t ld_dqkv,
                      float scale, double dropout_p, uint64_t seed, const uint64_t* rng_call, int site,
                      const uint64_t* mask, void* workspace, void* stream);
/* The same for packed rows (seg_start / seg_end int32 [B, T] dense, 4-byte aligned: cg_seg_bounds):
   query i sees key j iff seg_start[b,i] <= j <= i, so a segment's outputs and gradients are those of
   its tokens alone in a row of their own; every query sees at least itself.  The dropout keep bits
   stay indexed by (b, h, query, key) of the whole row (same `mask` buffer and cg_attn_dropmask).
   All-zero seg_start gives the bits of the entry points above.  bf16, head_size 64, T in {64, 128,
   192, 256} runs the sequence-resident MFMA kernels (the backward always as one launch; `delta`, if
   given, is read there), longer rows the ring kernels, fp32 with head_size <= 32 and no dropout the
   fp32 MFMA forward, every other shape the generic kernels -- the family of the unsegmented call.
   The attn_variant tuning knob does not apply.  cg_attn_bwd_seg's `delta` may be NULL.  stride_* are
   the row strides in elements, ld_* of the entry points above.                                   */
int cg_attn_fwd_seg(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                    const void* v, int64_t stride_qkv, void* o, int64_t stride_o, float* lse, float scale, double dropout_p,
                    uint64_t seed, const uint64_t* rng_call, int site, uint64_t* mask, const int32_t* seg_start,
                    const int32_t* seg_end, void* stream);
int cg_attn_fwd_seg_premasked(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                              const void* v, int64_t stride_qkv, void* o, int64_t stride_o, float* lse, float scale,
                              double dropout_p, uint64_t seed, const uint64_t* rng_call, int site, uint64_t* mask,
                              const int32_t* seg_start, const int32_t* seg_end, void* stream);
int cg_attn_bwd_seg(int dtype, int64_t B, int64_t T, int64_t H, int64_t D, const void* q, const void* k,
                    const void* v, int64_t stride_qkv, const void* o, int64_t stride_o, const void* dout, int64_t stride_do,
                    const float* lse, const float* delta, void* dq, void* dk, void* dv, int64_t stride_dqkv, float scale,
                    double dropout_p, uint64_t seed, const uint64_t* rng_call, int site, const uint64_t* mask,
                    const int32_t* seg_start, const int32_t* seg_end, void* workspace, void* stream);

/* ---- cross entropy over the char vocabulary (F.cross_entropy, GPT1.py:189-192) ----------
   logits fp32 [rows, V] (row stride ld); loss_rows[r] = lse_r - logit[r, tgt_r]; lse saved.
   bwd: dlogits = (*g) * g_mult * (softmax - onehot)   (g = dLoss, g_mult = 1/rows).                    */
int cg_ce_fwd(const float* logits, int64_t rows, int64_t V, int64_t ld, const int64_t* targets, float* loss_rows,
              float* lse, void* stream);
int cg_ce_bwd(const float* logits, int64_t rows, int64_t V, int64_t ld, const int64_t* targets, const float* lse,
              const float* g, float g_mult, float* dlogits, int64_t ld_d, void* dst_lp /* optional bf16 copy */,
              void* stream);

/* ---- fused LM head for the bf16 path (ln_f output -> lm_head -> cross entropy, GPT1.py:174,183-192)
   a bf16 [M, C]; wpad bf16 [wpad_rows, C] = lm_head.weight with zero rows V..wpad_rows-1
   (wpad_rows >= 16*ceil(V/16), V <= 128, M % 16 == 0, C % 32 == 0); bias fp32 [V].
   fwd: logits fp32 [M, V] = a wpad^T + b, lse [M]; with targets also *loss = mean CE (workspace
   cg_head_workspace).  bwd: dl bf16 [M, ld_dl] = (*g_loss) g_mult (softmax - onehot) [+ g_logits],
   zero in columns V..ld_dl-1 (the K-padded operand of the dgrad/wgrad GEMMs); db (+)= colsum(dl). */
int64_t cg_head_workspace(int64_t M, int64_t V);
int cg_head_fwd(const void* a, const void* wpad, int64_t wpad_rows, const float* bias, const int64_t* targets,
                float* logits, float* lse, float* loss, void* workspace, int64_t M, int64_t C, int64_t V,
                void* stream);
int cg_head_bwd(const float* logits, const float* lse, const int64_t* targets, const float* g_loss, float g_mult,
                const float* g_logits, void* dl, int64_t ld_dl, float* db, int db_accumulate, void* workspace,
                int64_t M, int64_t V, void* stream);
/* the same with flags: CG_DEFER queues the db column-sum reduce on the stream's deferral queue  */
int cg_head_bwd_ex(const float* logits, const float* lse, const int64_t* targets, const float* g_loss, float g_mult,
                   const float* g_logits, void* dl, int64_t ld_dl, float* db, int db_accumulate, void* workspace,
                   int64_t M, int64_t V, int flags, void* stream);

/* ---- masked cross entropy (F.cross_entropy's ignore_index; DESIGN.md "Masked cross entropy") ----
   Every operand is dense.  A row whose target equals ignore_index adds nothing to the loss and has a
   zero gradient (a literal 0: NaN or inf in its logits cannot leak); the mean is over the other
   ("valid") rows.  The normaliser lives on the device: float norm[2] = {valid rows, 1 / valid rows},
   written by the forward (cg_head_fwd_masked / cg_ce_mean_masked) and read by the backward, so a
   captured graph follows the batch.  No valid row: norm = {0, inf}, the loss is NaN (torch's 0 / 0)
   and every gradient 0.  A target that is neither ignore_index nor in [0, V) makes the loss NaN.
   With no row ignored the results have the bits of the unmasked entry points.
   Fused bf16 head: the shapes of cg_head_fwd / cg_head_bwd_ex; logits and lse are written for every
   row; workspace cg_head_masked_workspace(M, V) bytes (both directions); dl bf16 [M, KP] dense.     */
int64_t cg_head_masked_workspace(int64_t M, int64_t V);
int cg_head_fwd_masked(const void* a, const void* wpad, int64_t wpad_rows, const float* bias, const int64_t* targets,
                       int64_t ignore_index, float* logits, float* lse, float* loss, float* norm, void* workspace,
                       int64_t M, int64_t C, int64_t V, void* stream);
int cg_head_bwd_masked(const float* logits, const float* lse, const int64_t* targets, int64_t ignore_index,
                       const float* g_loss, const float* norm, const float* g_logits, void* dl, int64_t KP, float* db,
                       int db_accumulate, void* workspace, int64_t M, int64_t V, int flags, void* stream);
/* fp32 path: logits fp32 [rows, V] dense.  fwd: loss_rows[r] = lse_r - logit[r, tgt_r], 0 on ignored
   rows.  mean: *loss = sum(loss_rows) * norm[1] and norm, one launch, fixed order (workspace
   cg_ce_mean_masked_workspace(rows) bytes).  bwd: dlogits = (*g) norm[1] (softmax - onehot).          */
int cg_ce_fwd_masked(const float* logits, int64_t rows, int64_t V, const int64_t* targets, int64_t ignore_index,
                     float* loss_rows, float* lse, void* stream);
int64_t cg_ce_mean_masked_workspace(int64_t rows);
int cg_ce_mean_masked(const float* loss_rows, const int64_t* targets, int64_t rows, int64_t ignore_index, float* loss,
                      float* norm, void* workspace, void* stream);
int cg_ce_bwd_masked(const float* logits, int64_t rows, int64_t V, const int64_t* targets, int64_t ignore_index,
                     const float* lse, const float* g, const float* norm, float* dlogits,
                     void* dst_lp /* optional bf16 copy */, void* stream);

/* ---- batched decode for generate() (GPT1.py:196-212; replicatinggpt_amd/decode.py) ----------
   len_dev: device int64 = current sequence length (tokens in idx rows, row stride ld).          */
/* out[b, j] = idx[b, max(0, len - T) + j]: the cropped context of GPT1.py:200                   */
int cg_decode_window(const int64_t* idx, int64_t ld, int64_t B, int64_t T, const int64_t* len_dev, int64_t* out,
                     void* stream);
/* x[b] = wte[idx[b, len-1]] + wpe[len-1]  (fp32, the newest token)                              */
int cg_decode_embed(const int64_t* idx, int64_t ld, const float* wte, const float* wpe, int64_t C,
                    const int64_t* len_dev, float* x, int64_t B, void* stream);
/* K/V cache [B, H, Tmax, D] row len-1 <- qkv rows (k / v at column offsets k_off / v_off)        */
int cg_decode_kv_append(const float* qkv, int64_t ld, int64_t k_off, int64_t v_off, int64_t B, int64_t H,
                        int64_t D, int64_t Tmax, const int64_t* len_dev, float* kcache, float* vcache,
                        void* stream);
/* one query per (b, h) against keys 0..n-1 (n = *len_dev, or nkeys when len_dev is NULL; any n
   >= 1: online softmax over 16-key chunks); K/V element (b, h, j, e) at base + b*sb + h*sh + j*sj
   + e; o[b, h*D + e]; D <= 64                                                                    */
int cg_decode_attn(const float* q, int64_t ldq, const float* k, const float* v, int64_t sb, int64_t sh, int64_t sj,
                   int64_t B, int64_t H, int64_t D, const int64_t* len_dev, int64_t nkeys, float scale, float* o,
                   int64_t ldo, void* stream);
/* idx[b, len] <- argmax(logits[b]) (greedy: first index on ties, NaN counts as the maximum --
   torch.argmax's rules, so always inside [0, V)) or an inverse-CDF draw from softmax(logits[b])
   with u from Philox(*seed_dev, stream = len, counter = b)                                        */
int cg_decode_sample(const float* logits, int64_t ldl, int64_t V, int64_t B, int greedy, const uint64_t* seed_dev,
                     const int64_t* len_dev, int64_t* idx, int64_t ld, void* stream);
/* cg_decode_sample's draw with a temperature, a top-k cut and a nucleus (top-p) cut, in HF's order
   (temperature, top-k, top-p on the renormalised top-k distribution).  params_dev: three device
   floats {tau, k, p} read when the kernel runs (a captured graph serves every setting): tau > 0;
   k = 0 or k >= V: top-k off; 0 < p <= 1, p = 1: top-p off.  Per row of fp32 logits x[0..V):
     1. rank by logit descending, the lower index first among equals (compared on the raw logits);
     2. w[v] = exp((x[v] - max x) / tau); a -inf logit has weight 0;
     3. keep the first min(k, V) ranked tokens (all when top-k is off); S_k = the sum of their weights;
     4. p < 1: of those keep the shortest rank-order prefix whose weight reaches p * S_k (never
        fewer than one token);
     5. u24 = Philox4x32-10(counter (row, 0, len, 0), key *seed_dev)[0] >> 8, t = u24 / 2^24 * S with
        S the kept weights' sum; the token is the first kept v in vocabulary order with t < the kept
        weight summed through v, else the last kept v.  idx[row, len] <- token (len = *len_dev);
        nothing else is written.
   tau = 1 with both cuts off: bit for bit the token cg_decode_sample(greedy = 0) writes.  k = 1, or
   a p so small that the top token alone reaches p * S_k: the greedy token.  A row holding NaN or
   +inf: the greedy rule's token (the first NaN's index, else the first +inf's).  The token is always
   inside [0, V).  1 <= V <= 1024 and ldl >= V, else CG_EINVAL.                                    */
int cg_decode_sample_filtered(const float* logits, int64_t ldl, int64_t V, int64_t B, const float* params_dev,
                              const uint64_t* seed_dev, const int64_t* len_dev, int64_t* idx, int64_t ld,
                              void* stream);
/* The per-row epilogue of a ragged batch (BigramLanguageModel.complete): the two samplers above plus
   forced prompt tokens, stop tokens, a per-row budget and per-token log-probabilities, one launch per
   decode step, one row per workgroup.  All rows share n = *len_dev; every argument below except
   mode, the sizes and the strides is device memory read when the kernel runs, so a captured graph
   serves every prompt set, stop set, pad token and sampling setting.
     mode          0: greedy, 1: plain draw (cg_decode_sample greedy = 1 / 0), 2: filtered draw
                   (cg_decode_sample_filtered with params_dev = {tau, k, p}; NULL allowed otherwise);
     prompt_len[B] int64: the row's prompt length;
     limit[B]      int64: the length at which the row ends (prompt_len + max_new_tokens);
     end[B]        int64, read and written: 0 = the row is running, else its final length;
     stop_bits     ceil(V / 64) uint64 words: bit v (word v / 64, bit v % 64) set = token v ends a row;
     pad_dev       one int64: the token written into ended rows;
     idx[B, ld], logprob[B, ld] (fp32; NULL: no log-probabilities): one row stride for both.
   Per row b:
     1. end[b] != 0 (ended): idx[b, n] <- *pad_dev and logprob[b, n] <- 0; nothing else is written.
     2. n < prompt_len[b] (forced): the token is idx[b, n]; idx is not written.
     3. otherwise (emitted): the token is exactly what cg_decode_sample (modes 0, 1) or
        cg_decode_sample_filtered (mode 2) writes for these logits, *seed_dev, len = n and row b --
        their NaN and +inf rules included (the kernels share the choice code); idx[b, n] <- token.
     4. logprob given: logprob[b, n] <- (x[tok] - m) - log(sum_v exp(x[v] - m)) over the raw fp32
        logits x (temperature 1, no cuts; m = max x; fp32 accumulation), for forced tokens too; NaN
        when the row holds NaN or +inf, or a forced token lies outside [0, V).
     5. an emitted (not forced) token whose stop bit is set: end[b] <- n + 1; otherwise n + 1 ==
        limit[b]: end[b] <- n + 1.
   Plain stores only; the host polls end[] outside the graph.  The caller keeps n < ld and then
   advances *len_dev.  1 <= V <= 1024, ldl >= V and mode in {0, 1, 2}, else CG_EINVAL.             */
int cg_decode_emit(const float* logits, int64_t ldl, int64_t V, int64_t B, int mode, const float* params_dev,
                   const uint64_t* seed_dev, const int64_t* len_dev, const int64_t* prompt_len, const int64_t* limit,
                   int64_t* end, const uint64_t* stop_bits, const int64_t* pad_dev, int64_t* idx, int64_t ld,
                   float* logprob, void* stream);
/* One-pass prompt prefill: the attention of P per-token steps in one launch, and the K/V cache they
   leave.  q, k, v: the fp32 rows of a layer's QKV product for B x P positions, row b*P + t, element
   h*D + e of each (three base pointers; row stride stride_q for q, stride_kv for both k and v).
     kcache / vcache [B, H, Tmax, D] (dense): rows t < P of every (b, h) <- the k / v rows, exact
       copies; rows t >= P are not written.
     o (row b*P + t, element h*D + e, row stride stride_o): bit for bit what cg_decode_attn returns
       for that (b, h) with q's row b*P + t as the query and nkeys = t + 1 keys of that cache.
   The per-query arithmetic is cg_decode_attn's, one wave per position: keys in chunks of 64, key
   64c + lane on lane `lane`; the score an fmaf chain over e < DP (D padded to 24 or 64 with zeros),
   times scale; online softmax statistics per chunk (wave max, __expf, wave sum); acc[e] =
   fmaf(p, v[e], acc[e] * alpha); one wave sum per dimension and * (1 / l) at the end -- the kernels
   share that code, so a prefill by this call and a prefill by P decode steps leave the same bits.
   q == NULL and o == NULL: the cache rows only (a last layer whose outputs nobody reads).  Reads
   nothing outside the P rows' H*D elements, writes nothing but the cache rows and o elements named
   above.  D <= 64, 1 <= P <= Tmax, every stride >= H*D, every pointer 4-B aligned, q and o both
   NULL or both given, else CG_EINVAL.                                                              */
int cg_decode_prefill_attn(const float* q, int64_t stride_q, const float* k, const float* v, int64_t stride_kv,
                           int64_t B, int64_t P, int64_t H, int64_t D, int64_t Tmax, float scale, float* kcache,
                           float* vcache, float* o, int64_t stride_o, void* stream);
/* The log-probabilities of a one-pass prefill: for logits row b*P + t (fp32, V columns, row stride
   stride_logits; the model's output at position t of row b), logprob[b, t + 1] <- log
   softmax(row)[idx[b, t + 1]], t < P, computed by the code of cg_decode_emit's step 4 -- the same
   bits, NaN for a row holding NaN or +inf and for a token outside [0, V) (nothing is read there)
   included.  idx [B, > P] int64 (row stride stride_idx) is only read; of logprob (row stride
   stride_logprob) only columns 1..P are written.  V >= 1, stride_logits >= V, both other strides
   > P, else CG_EINVAL.                                                                             */
int cg_decode_logprob_rows(const float* logits, int64_t stride_logits, int64_t V, int64_t B, int64_t P,
                           const int64_t* idx, int64_t stride_idx, float* logprob, int64_t stride_logprob,
                           void* stream);

/* ---- fused AdamW over a flat fp32 buffer (torch.optim.AdamW, GPT1.py:218,233) ------------
   step_ptr: device int64 step count (already incremented for this step).
   p_bf16: optional bf16 shadow written after the update (GEMM operands).                    */
int cg_adamw(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, double lr, double beta1,
             double beta2, double eps, double weight_decay, const int64_t* step_ptr, void* stream);
/* the same update for [0, n) of one region, deferred on `stream`'s queue: run by the free blocks of
   the next persistent GEMM launch on `stream` that has >= 64 of them (a part-filling launch; at most 4 jobs per launch,
   oldest first), else by cg_flush_deferred -- the jobs left, when they are slices of one set of
   buffers, as one segmented launch -- same bits either way.  The gradient must be final in stream order (a
   pending split-K reduce or queued column-sum reduce writing into g is launched first) and nothing launched before the flush may
   read p / p_bf16 / m / v.  n % 4 == 0, p, g, m, v 16-B and p_bf16 8-B aligned. */
int cg_adamw_defer(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, double lr,
                   double beta1, double beta2, double eps, double weight_decay, const int64_t* step_ptr,
                   void* stream);
/* cg_adamw over a host list of nseg (start, length) element segments of the same flat buffers
   (multiples of 4, at most 64): the parameters a step did not defer.  Same bits as cg_adamw. */
int cg_adamw_segments(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, const int64_t* segs, int nseg,
                      double lr, double beta1, double beta2, double eps, double weight_decay,
                      const int64_t* step_ptr, void* stream);
/* cg_adamw with the learning rate read from the device when the kernel runs (*lr_dev, a double: a
   schedule that happens to be constant gives cg_adamw's bits), so a captured graph follows a
   schedule.  gscale_dev != NULL: every gradient is g * *gscale_dev rounded once to fp32 before the
   update (g itself is not written) -- the bits of cg_scale_f32 on g followed by cg_adamw, without
   that pass.  NULL: no multiply.  The same kernel forms by size as cg_adamw.  The GEMM-hosted
   updates (cg_adamw_defer) and cg_adamw_segments have no device-lr form yet.                   */
int cg_adamw_dyn(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, const double* lr_dev,
                 const float* gscale_dev, double beta1, double beta2, double eps, double weight_decay,
                 const int64_t* step_ptr, void* stream);

/* ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) ------------
   out[0] = ||g||_2 over n floats = (float)sqrt(sum of squares accumulated in fp64), out[1] = the
   clip coefficient min(1, max_norm / (out[0] + 1e-6)) in fp32 (one add, one correctly rounded
   divide: torch's formula).  One read pass, two launches (per-block partials in `workspace`, then an
   ordered fold): the grid depends only on n and every fold has a fixed order, so the result is
   bit-identical run to run and on every rank that holds the same gradients.  g: any 4-B alignment
   (16-B loads from the first 16-B boundary), any n; n == 0: norm 0.  +inf in g: (inf, 0).  NaN in g:
   a NaN norm, coefficient 1.  workspace: cg_grad_norm_workspace(n) bytes, 8-B aligned.             */
int64_t cg_grad_norm_workspace(int64_t n);
int cg_grad_norm(const float* g, int64_t n, float max_norm, float* out, void* workspace, void* stream);
/* x[i] *= *scale_dev for i in [0, n) (clip_grad_norm_'s in-place scale, for hand-written loops) */
int cg_scale_f32(float* x, int64_t n, const float* scale_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHARPT_H */
