"""torch.library custom ops over the charpt C ABI (include/charpt.h).

Each op is a thin, out-style wrapper: the caller (replicatinggpt_amd.functional) allocates every
output/workspace through PyTorch's caching allocator, and the op launches the HIP kernel on the
current stream (so whole training steps are capturable into a hipGraph).  Ops are registered for
the "cuda" (= HIP on ROCm) device only: calling them on CPU tensors raises -- the product has no
CPU fallback.
"""
from typing import List, Optional

import torch
from torch import Tensor

from . import _lib as L

_NS = "charpt"


def _s(t):
    return L.stream_ptr(t.device)


def _op(name, mutates):
    return torch.library.custom_op(f"{_NS}::{name}", mutates_args=mutates, device_types="cuda")


# ---------------------------------------------------------------------------------------
@_op("rng_snapshot", ("counter", "snap"))
def rng_snapshot(counter: Tensor, snap: Tensor) -> None:
    L.check(L.load().cg_rng_snapshot(L.ptr(counter), L.ptr(snap), _s(counter)), "rng_snapshot")


@_op("counter_add", ("counter",))
def counter_add(counter: Tensor, delta: int) -> None:
    L.check(L.load().cg_counter_add(L.ptr(counter), delta, _s(counter)), "counter_add")


@_op("dropout_mask", ("out",))
def dropout_mask(out: Tensor, p: float, seed: int, rng_call: Optional[Tensor], site: int) -> None:
    L.check(L.load().cg_dropout_mask(L.ptr(out), out.numel(), p, seed, L.ptr(rng_call), site, _s(out)), "dropout_mask")


@_op("dropout_apply", ("out",))
def dropout_apply(x: Tensor, out: Tensor, p: float, seed: int, rng_call: Optional[Tensor], site: int) -> None:
    C = x.shape[-1]
    rows = x.numel() // C
    L.check(L.load().cg_dropout_apply(L.ptr(x), rows, C, C, L.ptr(out), L.dtype_code(out.dtype), p, seed,
                                      L.ptr(rng_call), site, _s(x)), "dropout_apply")


@_op("sum_scaled", ("out", "ws"))
def sum_scaled(x: Tensor, scale: float, out: Tensor, ws: Tensor) -> None:
    L.check(L.load().cg_sum_f32(L.ptr(x), x.numel(), scale, L.ptr(out), L.ptr(ws), _s(x)), "sum_f32")


@_op("cast_bf16", ("out",))
def cast_bf16(x: Tensor, out: Tensor) -> None:
    L.check(L.load().cg_cast_f32_bf16(L.ptr(x), L.ptr(out), x.numel(), _s(x)), "cast_f32_bf16")


@_op("gather_batch", ("x", "y"))
def gather_batch(data: Tensor, ix: Tensor, x: Tensor, y: Tensor) -> None:
    B, T = x.shape
    L.check(L.load().cg_gather_batch(L.ptr(data), int(data.dtype == torch.uint8), L.ptr(ix), L.ptr(x), L.ptr(y), B,
                                     T, _s(x)), "gather_batch")


@_op("gather_pairs", ("x", "y"))
def gather_pairs(table: Tensor, plen: Tensor, tlen: Tensor, ix: Tensor, x: Tensor, y: Tensor, pad_token: int,
                 ignore_index: int) -> None:
    """table int64 [N, T+1] packed (prompt + completion) rows; see cg_gather_pairs."""
    B, T = x.shape
    if table.shape[1] != T + 1 or not (table.is_contiguous() and x.is_contiguous() and y.is_contiguous()):
        raise ValueError(f"gather_pairs: table must be dense [N, T+1] (T={T}, table {tuple(table.shape)}), x and y dense")
    L.check(L.load().cg_gather_pairs(L.ptr(table), L.ptr(plen), L.ptr(tlen), L.ptr(ix), L.ptr(x), L.ptr(y), B, T,
                                     pad_token, ignore_index, _s(x)), "gather_pairs")


# ---------------------------------------------------------------------------------------
@_op("embed_fwd", ("x",))
def embed_fwd(idx: Tensor, wte: Tensor, wpe: Tensor, x: Tensor) -> None:
    B, T = idx.shape
    V, C = wte.shape
    L.check(L.load().cg_embed_fwd(L.ptr(idx), L.ptr(wte), L.ptr(wpe), L.ptr(x), B, T, C, V, _s(x)), "embed_fwd")


@_op("embed_bwd", ("dwte", "dwpe", "ws"))
def embed_bwd(idx: Tensor, dx: Tensor, dwte: Optional[Tensor], dwpe: Optional[Tensor], accumulate: bool,
              ws: Tensor) -> None:
    B, T = idx.shape
    C = dx.shape[-1]
    V = dwte.shape[0] if dwte is not None else 1
    L.check(L.load().cg_embed_bwd(L.ptr(idx), L.ptr(dx), L.ptr(dwte), L.ptr(dwpe), B, T, C, V, int(accumulate),
                                  L.ptr(ws), _s(dx)), "embed_bwd")


def embed_bwd_workspace(B, T, C, V):
    return L.load().cg_embed_bwd_workspace(B, T, C, V)


# packed rows (several pairs per row): seg_start / seg_end int32 [B, T], see cg_seg_bounds
def _seg_check(name, B, T, ref, **segs):
    for k, t in segs.items():
        if t.dtype != torch.int32 or tuple(t.shape) != (B, T) or not t.is_contiguous() or t.device != ref.device:
            raise ValueError(f"{name}: {k} must be a dense int32 [{B}, {T}] tensor on {ref.device} "
                             f"(got {t.dtype} {tuple(t.shape)}, strides {tuple(t.stride())}, {t.device})")


@_op("seg_bounds", ("seg_end",))
def seg_bounds(seg_start: Tensor, seg_end: Tensor) -> None:
    if seg_start.dim() != 2:
        raise ValueError(f"seg_bounds: seg_start must be [B, T] (got {tuple(seg_start.shape)})")
    B, T = seg_start.shape
    _seg_check("seg_bounds", B, T, seg_start, seg_start=seg_start, seg_end=seg_end)
    L.check(L.load().cg_seg_bounds(L.ptr(seg_start), L.ptr(seg_end), B, T, _s(seg_start)), "seg_bounds")


@_op("embed_fwd_seg", ("x",))
def embed_fwd_seg(idx: Tensor, seg_start: Tensor, wte: Tensor, wpe: Tensor, x: Tensor) -> None:
    B, T = idx.shape
    V, C = wte.shape
    _seg_check("embed_fwd_seg", B, T, idx, seg_start=seg_start)
    if wpe.shape[0] < T:
        raise ValueError(f"embed_fwd_seg: wpe has {wpe.shape[0]} rows, T = {T}")
    L.check(L.load().cg_embed_fwd_seg(L.ptr(idx), L.ptr(seg_start), L.ptr(wte), L.ptr(wpe), L.ptr(x), B, T, C, V,
                                      _s(x)), "embed_fwd_seg")


@_op("embed_bwd_seg", ("dwte", "dwpe", "ws"))
def embed_bwd_seg(idx: Tensor, seg_end: Tensor, dx: Tensor, dwte: Optional[Tensor], dwpe: Optional[Tensor],
                  accumulate: bool, ws: Tensor) -> None:
    B, T = idx.shape
    C = dx.shape[-1]
    V = dwte.shape[0] if dwte is not None else 1
    _seg_check("embed_bwd_seg", B, T, idx, seg_end=seg_end)
    if dwpe is not None and dwpe.shape[0] < T:
        raise ValueError(f"embed_bwd_seg: dwpe has {dwpe.shape[0]} rows, T = {T}")
    L.check(L.load().cg_embed_bwd_seg(L.ptr(idx), L.ptr(seg_end), L.ptr(dx), L.ptr(dwte), L.ptr(dwpe), B, T, C, V,
                                      int(accumulate), L.ptr(ws), _s(dx)), "embed_bwd_seg")


# ---------------------------------------------------------------------------------------
@_op("layernorm_fwd", ("y", "mean", "rstd"))
def layernorm_fwd(x: Tensor, w: Tensor, b: Tensor, y: Tensor, mean: Tensor, rstd: Tensor, eps: float) -> None:
    """y = LayerNorm(x; w, b, eps) over the last dim, mean / rstd per row.  cg_layernorm_fwd takes
    pointers and no row stride: x and y must be dense (contiguous) -- a row-strided view raises instead
    of having the wrong rows normalised."""
    C = x.shape[-1]
    rows = x.numel() // C
    if not x.is_contiguous() or not y.is_contiguous():
        raise ValueError(f"layernorm_fwd: x and y must be dense (x strides {tuple(x.stride())}, y strides "
                         f"{tuple(y.stride())}): pass x.contiguous()")
    L.check(L.load().cg_layernorm_fwd(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.dtype_code(y.dtype), L.ptr(mean),
                                      L.ptr(rstd), rows, C, eps, _s(x)), "layernorm_fwd")


@_op("layernorm_fwd_attn_dropmask", ("y", "mean", "rstd", "mask"))
def layernorm_fwd_attn_dropmask(x: Tensor, w: Tensor, b: Tensor, y: Tensor, mean: Tensor, rstd: Tensor, eps: float,
                                B: int, H: int, T: int, dropout_p: float, seed: int, rng_call: Optional[Tensor],
                                site: int, mask: Tensor) -> None:
    """layernorm_fwd and attn_dropmask (the keep bits of the attention the LayerNorm feeds) in one
    launch; same results as the two ops."""
    C = x.shape[-1]
    rows = x.numel() // C
    L.check(L.load().cg_layernorm_fwd_attn_dropmask(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.dtype_code(y.dtype),
                                                    L.ptr(mean), L.ptr(rstd), rows, C, eps, B, H, T, dropout_p, seed,
                                                    L.ptr(rng_call), site, L.ptr(mask), _s(x)),
            "layernorm_fwd_attn_dropmask")


@_op("layernorm_bwd", ("dx", "dx_lp", "dw", "db", "ws", "lp_colsum"))
def layernorm_bwd(dy: Tensor, x: Tensor, w: Tensor, mean: Tensor, rstd: Tensor, dres: Optional[Tensor], dx: Tensor,
                  dx_lp: Optional[Tensor], dw: Optional[Tensor], db: Optional[Tensor], accumulate: bool,
                  ws: Tensor, lp_colsum: Optional[Tensor], colsum_accumulate: bool, lp_p: float, lp_seed: int,
                  lp_rng_call: Optional[Tensor], lp_site: int) -> None:
    # (no defaults: torch.library drops trailing default-valued arguments from the boxed call, which
    #  would hide a mutated argument from its version-counter bookkeeping)
    C = x.shape[-1]
    rows = x.numel() // C
    L.check(L.load().cg_layernorm_bwd_ex(L.ptr(dy), L.dtype_code(dy.dtype), L.ptr(x), L.ptr(w), L.ptr(mean),
                                         L.ptr(rstd), L.ptr(dres), L.ptr(dx), L.ptr(dx_lp), lp_p, lp_seed,
                                         L.ptr(lp_rng_call), lp_site, L.ptr(dw), L.ptr(db), L.ptr(lp_colsum),
                                         int(accumulate), int(colsum_accumulate), L.ptr(ws), rows, C, _s(x)),
            "layernorm_bwd")


@_op("layernorm_bwd_rows", ("dx", "dx_lp", "ws"))
def layernorm_bwd_rows(dy: Tensor, x: Tensor, w: Tensor, mean: Tensor, rstd: Tensor, dres: Optional[Tensor],
                       dx: Tensor, dx_lp: Optional[Tensor], ws: Tensor, lp_colsum: bool, lp_p: float, lp_seed: int,
                       lp_rng_call: Optional[Tensor], lp_site: int) -> None:
    """layernorm_bwd without its column-sum reduce: the partials stay in ``ws`` for
    layernorm_bwd_reduce (launched on any stream ordered after this one)."""
    C = x.shape[-1]
    rows = x.numel() // C
    L.check(L.load().cg_layernorm_bwd_rows(L.ptr(dy), L.dtype_code(dy.dtype), L.ptr(x), L.ptr(w), L.ptr(mean),
                                           L.ptr(rstd), L.ptr(dres), L.ptr(dx), L.ptr(dx_lp), lp_p, lp_seed,
                                           L.ptr(lp_rng_call), lp_site, int(lp_colsum), L.ptr(ws), rows, C, _s(x)),
            "layernorm_bwd_rows")


@_op("layernorm_bwd_reduce", ("dw", "db", "lp_colsum"))
def layernorm_bwd_reduce(ws: Tensor, rows: int, C: int, colsum_partials: bool, dw: Optional[Tensor],
                         db: Optional[Tensor], lp_colsum: Optional[Tensor], accumulate: bool,
                         colsum_accumulate: bool, defer: bool = False) -> None:
    """defer: queued on the stream's deferral queue (CG_DEFER) until cg_flush_deferred."""
    L.check(L.load().cg_layernorm_bwd_reduce_ex(L.ptr(ws), rows, C, int(colsum_partials), L.ptr(dw), L.ptr(db),
                                                L.ptr(lp_colsum), int(accumulate), int(colsum_accumulate),
                                                L.DEFER if defer else 0, _s(ws)), "layernorm_bwd_reduce")


def layernorm_bwd_workspace(rows, C):
    return L.load().cg_layernorm_bwd_workspace(rows, C)


# ---------------------------------------------------------------------------------------
def _gemm_extents(a, b, out, a_trans, b_trans, M, N, K, lda, ldb, ldc, what="gemm"):
    """Host check that every element cg_gemm will address lies inside its tensor (the C ABI sees
    only pointers): A(m,k) = A[k lda + m] (a_trans) or A[m lda + k]; B(n,k) likewise; C[m ldc + n]."""
    need_a = (K - 1) * lda + M if a_trans else (M - 1) * lda + K
    need_b = (K - 1) * ldb + N if b_trans else (N - 1) * ldb + K
    need_c = (M - 1) * ldc + N
    for name, t, need in (("A", a, need_a), ("B", b, need_b), ("C", out, need_c)):
        if t is None or t.device.type == "meta":
            continue
        # views (a column block of qkv, ...) address their storage past their own numel
        avail = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        if need > avail:
            raise ValueError(f"charpt {what}: operand {name} needs {need} elements for M={M} N={N} K={K} "
                             f"(trans {int(a_trans)}{int(b_trans)}, ld {lda}/{ldb}/{ldc}), its storage has {avail}")


@_op("gemm", ("out", "ws"))
def gemm(a: Tensor, b: Tensor, out: Tensor, op_bf16: bool, a_trans: bool, b_trans: bool, M: int, N: int, K: int,
         lda: int, ldb: int, ldc: int, epi: int, bias: Optional[Tensor], resid: Optional[Tensor], ld_resid: int,
         aux: Optional[Tensor], ld_aux: int, dropout_p: float, seed: int, rng_call: Optional[Tensor], site: int,
         beta: float, split_k: int, ws: Optional[Tensor], flags: int = 0) -> None:
    """flags: cg_epilogue_t.flags (L.GEMM_SLAB_BF16 | L.GEMM_DEFER_REDUCE) of a split-K weight gradient."""
    _gemm_extents(a, b, out, a_trans, b_trans, M, N, K, lda, ldb, ldc)
    e = L.Epilogue(epi, L.ptr(bias), L.ptr(resid), ld_resid, L.ptr(aux),
                   L.dtype_code(aux.dtype) if aux is not None else 0, ld_aux, dropout_p, seed, L.ptr(rng_call), site,
                   beta, None, flags)
    L.check(L.load().cg_gemm(L.CG_BF16 if op_bf16 else L.CG_F32, int(a_trans), int(b_trans), M, N, K, L.ptr(a), lda,
                             L.ptr(b), ldb, L.ptr(out), L.dtype_code(out.dtype), ldc, e, split_k, L.ptr(ws), _s(out)),
            "gemm")


def _wgrad_problems(dy: List[Tensor], x: List[Tensor], out: List[Tensor], ws: List[Tensor], betas: List[float],
                    splits: List[int], flags: int):
    """The cg_wgrad_problem_t array of out[i][N, K] (+)= dy[i][M, N]^T @ x[i][M, K]."""
    n = len(dy)
    arr = (L.WgradProblem * n)()
    for i in range(n):
        M, N = dy[i].shape
        K = x[i].shape[1]
        lda, ldb, ldc = dy[i].stride(0), x[i].stride(0), out[i].stride(0)
        _gemm_extents(dy[i], x[i], out[i], True, True, N, K, M, lda, ldb, ldc, "gemm_wgrad_group")
        arr[i] = L.WgradProblem(N, K, M, dy[i].data_ptr(), lda, x[i].data_ptr(), ldb, out[i].data_ptr(), ldc,
                                betas[i], splits[i], ws[i].data_ptr(), flags)
    return arr, n


def gemm_wgrad_group_supported(dy, x, out, ws, betas, splits, flags):
    """Whether gemm_wgrad_group takes these weight gradients as one launch (cg_gemm_wgrad_group_supported:
    asked from the library, current tuning knobs included; False for a library without the entry point)."""
    lib = L.load()
    if not hasattr(lib, "cg_gemm_wgrad_group_supported") or not 1 <= len(dy) <= 4:
        return False
    if any(t.dtype != torch.bfloat16 or t.stride(1) != 1 for t in (*dy, *x)):
        return False
    if any(t.dtype != torch.float32 or t.stride(1) != 1 for t in out) or any(w is None for w in ws):
        return False
    arr, n = _wgrad_problems(dy, x, out, ws, betas, splits, flags)
    return bool(lib.cg_gemm_wgrad_group_supported(arr, n))


@_op("gemm_wgrad_group", ("out", "ws"))
def gemm_wgrad_group(dy: List[Tensor], x: List[Tensor], out: List[Tensor], ws: List[Tensor], betas: List[float],
                     splits: List[int], flags: int) -> None:
    """out[i][N, K] (+)= dy[i][M, N]^T @ x[i][M, K] for every i as ONE split-K launch (cg_gemm_wgrad_group):
    each out[i] has the bits of gemm() at splits[i] with the same flags.  Fails (CG_EINVAL) unless
    gemm_wgrad_group_supported."""
    arr, n = _wgrad_problems(dy, x, out, ws, betas, splits, flags)
    L.check(L.load().cg_gemm_wgrad_group(arr, n, _s(out[0])), "gemm_wgrad_group")


@_op("gemm_bias_relu_bits", ("out", "bits"))
def gemm_bias_relu_bits(a: Tensor, b: Tensor, out: Tensor, M: int, N: int, K: int, lda: int, ldb: int, ldc: int,
                        bias: Tensor, bits: Tensor, ld_bits: int) -> None:
    """out = bf16 relu(a[M,K] @ b[N,K]^T + bias) and its ReLU keep bits (CG_BITS: int32 words
    [M, ld_bits], bit n % 32 of word n / 32 = out[m, n] != 0) for the ReLU-backward dgrad.  Fails
    (CG_EINVAL) unless cg_gemm_relu_bits_supported."""
    _gemm_extents(a, b, out, False, False, M, N, K, lda, ldb, ldc, "gemm_bias_relu_bits")
    e = L.Epilogue(L.EPI_BIAS_RELU, L.ptr(bias), None, 0, L.ptr(bits), L.CG_BITS, ld_bits, 0.0, 0, None, 0, 0.0)
    L.check(L.load().cg_gemm(L.CG_BF16, 0, 0, M, N, K, L.ptr(a), lda, L.ptr(b), ldb, L.ptr(out),
                             L.dtype_code(out.dtype), ldc, e, 1, None, _s(out)), "gemm_bias_relu_bits")


@_op("gemm_relu_bwd_colpart", ("out", "colpart"))
def gemm_relu_bwd_colpart(a: Tensor, b: Tensor, out: Tensor, M: int, N: int, K: int, lda: int, ldb: int, ldc: int,
                          aux: Tensor, ld_aux: int, colpart: Tensor) -> None:
    """out = relu_bwd(a[M,K] @ b[N,K]^T, aux) in bf16 with the column sums of every 64-row block of
    the output into colpart [M/64, N] (the consumer's bias-gradient partials; cg_reduce_rows folds
    them).  Fails (CG_EINVAL) unless the dispatch takes the 128x128 persistent kernel."""
    _gemm_extents(a, b, out, False, True, M, N, K, lda, ldb, ldc, "gemm_relu_bwd_colpart")
    e = L.Epilogue(L.EPI_RELU_BWD, None, None, 0, L.ptr(aux), L.dtype_code(aux.dtype), ld_aux, 0.0, 0, None, 0, 0.0,
                   L.ptr(colpart))
    L.check(L.load().cg_gemm(L.CG_BF16, 0, 1, M, N, K, L.ptr(a), lda, L.ptr(b), ldb, L.ptr(out),
                             L.dtype_code(out.dtype), ldc, e, 1, None, _s(out)), "gemm_relu_bwd_colpart")


@_op("gemm_store_rowdot", ("out", "delta"))
def gemm_store_rowdot(a: Tensor, b: Tensor, out: Tensor, M: int, N: int, K: int, lda: int, ldb: int, ldc: int,
                      o: Tensor, ld_o: int, T: int, delta: Tensor) -> None:
    """out = bf16(a[M,K] @ b[N,K]^T) (the attention-output gradient dO) and the attention backward's
    delta[b, h, t] = sum_e out[b*T + t, 64h + e] * o[b*T + t, 64h + e] (fp32 [M/T, N/64, T]) from
    the rounded values.  Fails (CG_EINVAL) unless cg_gemm_rowdot_supported."""
    _gemm_extents(a, b, out, False, True, M, N, K, lda, ldb, ldc, "gemm_store_rowdot")
    e = L.Epilogue(L.EPI_STORE_ROWDOT, None, None, T, L.ptr(o), L.dtype_code(o.dtype), ld_o, 0.0, 0, None, 0, 0.0,
                   L.ptr(delta))
    L.check(L.load().cg_gemm(L.CG_BF16, 0, 1, M, N, K, L.ptr(a), lda, L.ptr(b), ldb, L.ptr(out),
                             L.dtype_code(out.dtype), ldc, e, 1, None, _s(out)), "gemm_store_rowdot")


@_op("gemm_resid_layernorm", ("out", "y", "mean", "rstd"))
def gemm_resid_layernorm(a: Tensor, w: Tensor, out: Tensor, M: int, N: int, K: int, lda: int, ldw: int, ldc: int,
                         bias: Tensor, resid: Tensor, ld_resid: int, dropout_p: float, seed: int,
                         rng_call: Optional[Tensor], site: int, ln_w: Tensor, ln_b: Tensor, y: Tensor, mean: Tensor,
                         rstd: Tensor, eps: float) -> None:
    """out = resid + dropout(a[M,K] @ w[N,K]^T + bias) (fp32; dropout_p 0: none) and y = LayerNorm(out;
    ln_w, ln_b) (bf16, row stride N), mean, rstd in one launch -- the bits of gemm(...,
    "bias_[drop_]resid") followed by layernorm_fwd.  Fails (CG_EINVAL) unless
    gemm_resid_layernorm_supported(M, N, K)."""
    _gemm_extents(a, w, out, False, False, M, N, K, lda, ldw, ldc, "gemm_resid_layernorm")
    kind = L.EPI_BIAS_DROP_RESID if dropout_p > 0 else L.EPI_BIAS_RESID
    e = L.Epilogue(kind, L.ptr(bias), L.ptr(resid), ld_resid, None, 0, 0, dropout_p, seed, L.ptr(rng_call), site, 0.0)
    L.check(L.load().cg_gemm_resid_layernorm(M, N, K, L.ptr(a), lda, L.ptr(w), ldw, L.ptr(out), ldc, e, L.ptr(ln_w),
                                             L.ptr(ln_b), L.ptr(y), L.ptr(mean), L.ptr(rstd), eps, _s(out)),
            "gemm_resid_layernorm")


@_op("linear_rows_f32", ("out",))
def linear_rows_f32(a: Tensor, ln_w: Optional[Tensor], ln_b: Optional[Tensor], eps: float, w: Tensor,
                    bias: Optional[Tensor], resid: Optional[Tensor], out: Tensor, relu: bool = False) -> None:
    """out = [resid +] act(a' @ w^T [+ bias]), a' = LayerNorm(a; ln_w, ln_b, eps) (or a when ln_w is None),
    act = relu when relu (bias, no resid), fp32, K <= 128, one launch -- the bits of [layernorm_fwd +]
    gemm(..., "store" / "bias" / "bias_relu" / "bias_resid").  a may be row-strided (even stride), w a
    row slice, out / resid column slices.  Fails (CG_EINVAL) unless linear_rows_f32_supported(M, N, K),
    a / w and, with the LayerNorm, ln_w / ln_b 8-B aligned."""
    M, K = a.shape
    N = w.shape[0]
    for t, name in ((a, "a"), (w, "w"), (bias, "bias"), (resid, "resid"), (out, "out"), (ln_w, "ln_w"),
                    (ln_b, "ln_b")):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"linear_rows_f32: {name} must be a float32 device tensor")
        if t.dim() == 2 and t.stride(1) != 1:
            raise ValueError(f"linear_rows_f32: {name} must have unit column stride")
    if (ln_w is None) != (ln_b is None) or (ln_w is not None and (ln_w.numel() != K or ln_b.numel() != K)):
        raise ValueError("linear_rows_f32: ln_w and ln_b both [K] or both None")
    if tuple(w.shape) != (N, K) or (bias is not None and bias.numel() != N) or tuple(out.shape) != (M, N) or \
            (resid is not None and tuple(resid.shape) != (M, N)):
        raise ValueError(f"linear_rows_f32: shapes a {tuple(a.shape)} w {tuple(w.shape)} out {tuple(out.shape)}")
    L.check(L.load().cg_linear_rows_f32(M, N, K, L.ptr(a), a.stride(0), L.ptr(ln_w), L.ptr(ln_b), eps, L.ptr(w),
                                        w.stride(0), L.ptr(bias), int(relu), L.ptr(resid),
                                        resid.stride(0) if resid is not None else 0, L.ptr(out), out.stride(0),
                                        _s(out)), "linear_rows_f32")


def linear_rows_f32_supported(M, N, K):
    return bool(L.load().cg_linear_rows_f32_supported(M, N, K))


@_op("ffn_fwd_f32", ("out",))
def ffn_fwd_f32(a: Tensor, ln_w: Optional[Tensor], ln_b: Optional[Tensor], eps: float, w1: Tensor, b1: Tensor,
                w2: Tensor, b2: Tensor, resid: Tensor, out: Tensor) -> None:
    """out = resid + (relu(a' @ w1^T + b1) @ w2^T + b2), a' = LayerNorm(a; ln_w, ln_b, eps) (or a when
    ln_w is None), fp32, one launch (FeedForward + its ln2 in eval) -- the bits of layernorm_fwd, then
    gemm(..., "bias_relu") into an [M, H] buffer, then gemm(..., "bias_resid").  Fails (CG_EINVAL)
    unless ffn_fwd_f32_supported(M, C, H)."""
    M, C = a.shape
    H = w1.shape[0]
    for t, name in ((a, "a"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (resid, "resid"), (out, "out"),
                    (ln_w, "ln_w"), (ln_b, "ln_b")):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"ffn_fwd_f32: {name} must be a float32 device tensor")
        if t.dim() == 2 and t.stride(1) != 1:
            raise ValueError(f"ffn_fwd_f32: {name} must have unit column stride")
    if (ln_w is None) != (ln_b is None) or (ln_w is not None and (ln_w.numel() != C or ln_b.numel() != C)):
        raise ValueError("ffn_fwd_f32: ln_w and ln_b both [C] or both None")
    if tuple(w1.shape) != (H, C) or tuple(w2.shape) != (C, H) or b1.numel() != H or b2.numel() != C or \
            tuple(resid.shape) != (M, C) or tuple(out.shape) != (M, C):
        raise ValueError(f"ffn_fwd_f32: shapes a {tuple(a.shape)} w1 {tuple(w1.shape)} w2 {tuple(w2.shape)} "
                         f"b1 {b1.numel()} b2 {b2.numel()} resid {tuple(resid.shape)} out {tuple(out.shape)}")
    L.check(L.load().cg_ffn_fwd_f32(M, C, H, L.ptr(a), a.stride(0), L.ptr(ln_w), L.ptr(ln_b), eps, L.ptr(w1),
                                    w1.stride(0), L.ptr(b1), L.ptr(w2), w2.stride(0), L.ptr(b2), L.ptr(resid),
                                    resid.stride(0), L.ptr(out), out.stride(0), _s(out)), "ffn_fwd_f32")


def ffn_fwd_f32_supported(M, C, H):
    return bool(L.load().cg_ffn_fwd_f32_supported(M, C, H))


def gemm_resid_layernorm_supported(M, N, K):
    return bool(L.load().cg_gemm_resid_layernorm_supported(M, N, K))


def gemm_rowdot_supported(M, N, K, lda, ldb, ldc):
    return bool(L.load().cg_gemm_rowdot_supported(0, 1, M, N, K, lda, ldb, ldc))


@_op("reduce_rows", ("out",))
def reduce_rows(part: Tensor, rows: int, N: int, out: Tensor, accumulate: bool, defer: bool = False) -> None:
    """defer: queued on the stream's deferral queue (CG_DEFER) until cg_flush_deferred."""
    L.check(L.load().cg_reduce_rows_ex(L.ptr(part), rows, N, L.ptr(out), int(accumulate), L.DEFER if defer else 0,
                                       _s(out)), "reduce_rows")


def gemm_workspace(M, N, split_k):
    return L.load().cg_gemm_workspace(M, N, split_k)


@_op("colsum", ("out", "ws"))
def colsum(x: Tensor, out: Tensor, accumulate: bool, ws: Tensor) -> None:
    N = x.shape[-1]
    rows = x.numel() // N
    L.check(L.load().cg_colsum(L.ptr(x), L.dtype_code(x.dtype), rows, N, N, L.ptr(out), int(accumulate), L.ptr(ws),
                               _s(x)), "colsum")


def colsum_workspace(rows, N):
    return L.load().cg_colsum_workspace(rows, N)


# ---------------------------------------------------------------------------------------
@_op("attn_fwd", ("o", "lse", "mask"))
def attn_fwd(qkv: Tensor, B: int, T: int, H: int, D: int, q_off: int, k_off: int, v_off: int, ld: int, o: Tensor,
             ld_o: int, lse: Tensor, scale: float, dropout_p: float, seed: int, rng_call: Optional[Tensor],
             site: int, mask: Optional[Tensor], mask_ready: bool = False) -> None:
    es = qkv.element_size()
    base = qkv.data_ptr()
    fn = L.load().cg_attn_fwd_premasked if mask_ready else L.load().cg_attn_fwd
    L.check(fn(L.dtype_code(qkv.dtype), B, T, H, D, base + q_off * es, base + k_off * es, base + v_off * es, ld,
               L.ptr(o), ld_o, L.ptr(lse), scale, dropout_p, seed, L.ptr(rng_call), site, L.ptr(mask), _s(qkv)),
            "attn_fwd")


@_op("attn_dropmask", ("mask",))
def attn_dropmask(B: int, H: int, T: int, dropout_p: float, seed: int, rng_call: Optional[Tensor], site: int,
                  mask: Tensor) -> None:
    L.check(L.load().cg_attn_dropmask(B, H, T, dropout_p, seed, L.ptr(rng_call), site, L.ptr(mask), _s(mask)),
            "attn_dropmask")


def attn_mask_bytes(B, H, T):
    return L.load().cg_attn_mask_bytes(B, H, T)


@_op("attn_bwd", ("dqkv", "ws"))
def attn_bwd(qkv: Tensor, B: int, T: int, H: int, D: int, q_off: int, k_off: int, v_off: int, ld: int, o: Tensor,
             ld_o: int, dout: Tensor, ld_do: int, lse: Tensor, dqkv: Tensor, ld_d: int, scale: float,
             dropout_p: float, seed: int, rng_call: Optional[Tensor], site: int, mask: Optional[Tensor],
             ws: Tensor, delta: Optional[Tensor] = None) -> None:
    """delta: rowsum(dO * O) precomputed (gemm_store_rowdot), fp32 [B, H, T]; None: computed here."""
    es = qkv.element_size()
    base, dbase = qkv.data_ptr(), dqkv.data_ptr()
    L.check(L.load().cg_attn_bwd_delta(L.dtype_code(qkv.dtype), B, T, H, D, base + q_off * es, base + k_off * es,
                                       base + v_off * es, ld, L.ptr(o), ld_o, L.ptr(dout), ld_do, L.ptr(lse),
                                       L.ptr(delta), dbase + q_off * es, dbase + k_off * es, dbase + v_off * es, ld_d,
                                       scale, dropout_p, seed, L.ptr(rng_call), site, L.ptr(mask), L.ptr(ws),
                                       _s(qkv)), "attn_bwd")


def attn_bwd_workspace(B, T, H, D):
    return L.load().cg_attn_bwd_workspace(B, T, H, D)


@_op("attn_fwd_seg", ("o", "lse", "mask"))
def attn_fwd_seg(qkv: Tensor, B: int, T: int, H: int, D: int, q_off: int, k_off: int, v_off: int, ld: int, o: Tensor,
                 ld_o: int, lse: Tensor, scale: float, dropout_p: float, seed: int, rng_call: Optional[Tensor],
                 site: int, mask: Optional[Tensor], seg_start: Tensor, seg_end: Tensor,
                 mask_ready: bool = False) -> None:
    """attn_fwd on packed rows: query i sees key j iff seg_start[b, i] <= j <= i (cg_attn_fwd_seg)."""
    _seg_check("attn_fwd_seg", B, T, qkv, seg_start=seg_start, seg_end=seg_end)
    es = qkv.element_size()
    base = qkv.data_ptr()
    fn = L.load().cg_attn_fwd_seg_premasked if mask_ready else L.load().cg_attn_fwd_seg
    L.check(fn(L.dtype_code(qkv.dtype), B, T, H, D, base + q_off * es, base + k_off * es, base + v_off * es, ld,
               L.ptr(o), ld_o, L.ptr(lse), scale, dropout_p, seed, L.ptr(rng_call), site, L.ptr(mask),
               L.ptr(seg_start), L.ptr(seg_end), _s(qkv)), "attn_fwd_seg")


@_op("attn_bwd_seg", ("dqkv", "ws"))
def attn_bwd_seg(qkv: Tensor, B: int, T: int, H: int, D: int, q_off: int, k_off: int, v_off: int, ld: int, o: Tensor,
                 ld_o: int, dout: Tensor, ld_do: int, lse: Tensor, dqkv: Tensor, ld_d: int, scale: float,
                 dropout_p: float, seed: int, rng_call: Optional[Tensor], site: int, mask: Optional[Tensor],
                 ws: Tensor, seg_start: Tensor, seg_end: Tensor, delta: Optional[Tensor] = None) -> None:
    """attn_bwd on packed rows (cg_attn_bwd_seg); delta as attn_bwd's."""
    _seg_check("attn_bwd_seg", B, T, qkv, seg_start=seg_start, seg_end=seg_end)
    es = qkv.element_size()
    base, dbase = qkv.data_ptr(), dqkv.data_ptr()
    L.check(L.load().cg_attn_bwd_seg(L.dtype_code(qkv.dtype), B, T, H, D, base + q_off * es, base + k_off * es,
                                     base + v_off * es, ld, L.ptr(o), ld_o, L.ptr(dout), ld_do, L.ptr(lse),
                                     L.ptr(delta), dbase + q_off * es, dbase + k_off * es, dbase + v_off * es, ld_d,
                                     scale, dropout_p, seed, L.ptr(rng_call), site, L.ptr(mask), L.ptr(seg_start),
                                     L.ptr(seg_end), L.ptr(ws), _s(qkv)), "attn_bwd_seg")


# ---------------------------------------------------------------------------------------
@_op("ce_fwd", ("loss_rows", "lse"))
def ce_fwd(logits: Tensor, targets: Optional[Tensor], loss_rows: Optional[Tensor], lse: Tensor) -> None:
    V = logits.shape[-1]
    rows = logits.numel() // V
    L.check(L.load().cg_ce_fwd(L.ptr(logits), rows, V, V, L.ptr(targets), L.ptr(loss_rows), L.ptr(lse),
                               _s(logits)), "ce_fwd")


@_op("ce_bwd", ("dlogits", "dlogits_lp"))
def ce_bwd(logits: Tensor, targets: Tensor, lse: Tensor, g: Tensor, g_mult: float, dlogits: Optional[Tensor],
           dlogits_lp: Optional[Tensor]) -> None:
    V = logits.shape[-1]
    rows = logits.numel() // V
    L.check(L.load().cg_ce_bwd(L.ptr(logits), rows, V, V, L.ptr(targets), L.ptr(lse), L.ptr(g), g_mult,
                               L.ptr(dlogits), V, L.ptr(dlogits_lp), _s(logits)), "ce_bwd")


def head_workspace(M: int, V: int) -> int:
    return int(L.load().cg_head_workspace(M, V))


@_op("head_fwd", ("logits", "lse", "loss", "ws"))
def head_fwd(a: Tensor, wpad: Tensor, bias: Tensor, targets: Optional[Tensor], logits: Tensor, lse: Tensor,
             loss: Optional[Tensor], ws: Optional[Tensor]) -> None:
    M, C = a.shape
    V = logits.shape[-1]
    L.check(L.load().cg_head_fwd(L.ptr(a), L.ptr(wpad), wpad.shape[0], L.ptr(bias), L.ptr(targets), L.ptr(logits),
                                 L.ptr(lse), L.ptr(loss), L.ptr(ws), M, C, V, _s(a)), "head_fwd")


@_op("head_bwd", ("dl", "db", "ws"))
def head_bwd(logits: Tensor, lse: Tensor, targets: Optional[Tensor], g_loss: Optional[Tensor], g_mult: float,
             g_logits: Optional[Tensor], dl: Tensor, db: Optional[Tensor], db_accumulate: bool, ws: Tensor,
             defer: bool = False) -> None:
    """defer: the db column-sum reduce is queued on the stream's deferral queue (CG_DEFER)."""
    M, V = logits.shape
    L.check(L.load().cg_head_bwd_ex(L.ptr(logits), L.ptr(lse), L.ptr(targets), L.ptr(g_loss), g_mult,
                                    L.ptr(g_logits), L.ptr(dl), dl.stride(0), L.ptr(db), int(db_accumulate), L.ptr(ws),
                                    M, V, L.DEFER if defer else 0, _s(logits)), "head_bwd")


# masked cross entropy (ignore_index): dense operands, the normaliser norm[2] on the device
def _dense(name, **tensors):
    for k, t in tensors.items():
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: {k} must be dense (strides {tuple(t.stride())}); the masked entry points take "
                             "no row stride")


def head_masked_workspace(M: int, V: int) -> int:
    return int(L.load().cg_head_masked_workspace(M, V))


def ce_mean_masked_workspace(rows: int) -> int:
    return int(L.load().cg_ce_mean_masked_workspace(rows))


@_op("head_fwd_masked", ("logits", "lse", "loss", "norm", "ws"))
def head_fwd_masked(a: Tensor, wpad: Tensor, bias: Tensor, targets: Tensor, ignore_index: int, logits: Tensor,
                    lse: Tensor, loss: Tensor, norm: Tensor, ws: Tensor) -> None:
    M, C = a.shape
    V = logits.shape[-1]
    _dense("head_fwd_masked", a=a, wpad=wpad, targets=targets, logits=logits, lse=lse)
    L.check(L.load().cg_head_fwd_masked(L.ptr(a), L.ptr(wpad), wpad.shape[0], L.ptr(bias), L.ptr(targets),
                                        ignore_index, L.ptr(logits), L.ptr(lse), L.ptr(loss), L.ptr(norm), L.ptr(ws),
                                        M, C, V, _s(a)), "head_fwd_masked")


@_op("head_bwd_masked", ("dl", "db", "ws"))
def head_bwd_masked(logits: Tensor, lse: Tensor, targets: Tensor, ignore_index: int, g_loss: Tensor, norm: Tensor,
                    g_logits: Optional[Tensor], dl: Tensor, db: Optional[Tensor], db_accumulate: bool, ws: Tensor,
                    defer: bool = False) -> None:
    """dl: dense bf16 [M, KP].  defer: the db column-sum reduce is queued on the stream's deferral queue."""
    M, V = logits.shape
    _dense("head_bwd_masked", logits=logits, lse=lse, targets=targets, g_logits=g_logits, dl=dl)
    L.check(L.load().cg_head_bwd_masked(L.ptr(logits), L.ptr(lse), L.ptr(targets), ignore_index, L.ptr(g_loss),
                                        L.ptr(norm), L.ptr(g_logits), L.ptr(dl), dl.shape[1], L.ptr(db),
                                        int(db_accumulate), L.ptr(ws), M, V, L.DEFER if defer else 0, _s(logits)),
            "head_bwd_masked")


@_op("ce_fwd_masked", ("loss_rows", "lse"))
def ce_fwd_masked(logits: Tensor, targets: Tensor, ignore_index: int, loss_rows: Tensor, lse: Tensor) -> None:
    V = logits.shape[-1]
    rows = logits.numel() // V
    _dense("ce_fwd_masked", logits=logits, targets=targets)
    L.check(L.load().cg_ce_fwd_masked(L.ptr(logits), rows, V, L.ptr(targets), ignore_index, L.ptr(loss_rows),
                                      L.ptr(lse), _s(logits)), "ce_fwd_masked")


@_op("ce_mean_masked", ("loss", "norm", "ws"))
def ce_mean_masked(loss_rows: Tensor, targets: Tensor, ignore_index: int, loss: Tensor, norm: Tensor,
                   ws: Tensor) -> None:
    _dense("ce_mean_masked", loss_rows=loss_rows, targets=targets)
    L.check(L.load().cg_ce_mean_masked(L.ptr(loss_rows), L.ptr(targets), loss_rows.numel(), ignore_index,
                                       L.ptr(loss), L.ptr(norm), L.ptr(ws), _s(loss_rows)), "ce_mean_masked")


@_op("ce_bwd_masked", ("dlogits", "dlogits_lp"))
def ce_bwd_masked(logits: Tensor, targets: Tensor, ignore_index: int, lse: Tensor, g: Tensor, norm: Tensor,
                  dlogits: Optional[Tensor], dlogits_lp: Optional[Tensor]) -> None:
    V = logits.shape[-1]
    rows = logits.numel() // V
    _dense("ce_bwd_masked", logits=logits, targets=targets, dlogits=dlogits, dlogits_lp=dlogits_lp)
    L.check(L.load().cg_ce_bwd_masked(L.ptr(logits), rows, V, L.ptr(targets), ignore_index, L.ptr(lse), L.ptr(g),
                                      L.ptr(norm), L.ptr(dlogits), L.ptr(dlogits_lp), _s(logits)), "ce_bwd_masked")


# ---------------------------------------------------------------------------------------
# batched decode (decode.py)
@_op("decode_window", ("out",))
def decode_window(idx: Tensor, len_dev: Tensor, out: Tensor) -> None:
    B, T = out.shape
    L.check(L.load().cg_decode_window(L.ptr(idx), idx.stride(0), B, T, L.ptr(len_dev), L.ptr(out), _s(idx)),
            "decode_window")


@_op("decode_embed", ("x",))
def decode_embed(idx: Tensor, wte: Tensor, wpe: Tensor, len_dev: Tensor, x: Tensor) -> None:
    B, C = x.shape
    L.check(L.load().cg_decode_embed(L.ptr(idx), idx.stride(0), L.ptr(wte), L.ptr(wpe), C, L.ptr(len_dev), L.ptr(x),
                                     B, _s(x)), "decode_embed")


@_op("decode_kv_append", ("kcache", "vcache"))
def decode_kv_append(qkv: Tensor, k_off: int, v_off: int, len_dev: Tensor, kcache: Tensor, vcache: Tensor) -> None:
    B, H, Tmax, D = kcache.shape
    L.check(L.load().cg_decode_kv_append(L.ptr(qkv), qkv.stride(0), k_off, v_off, B, H, D, Tmax, L.ptr(len_dev),
                                         L.ptr(kcache), L.ptr(vcache), _s(qkv)), "decode_kv_append")


@_op("decode_qkv_f32", ("qkv", "kcache", "vcache"))
def decode_qkv_f32(x: Tensor, ln_w: Tensor, ln_b: Tensor, eps: float, w: Tensor, qkv: Tensor, len_dev: Tensor,
                   kcache: Tensor, vcache: Tensor) -> None:
    """qkv = LayerNorm(x) @ w^T and its K / V columns appended to the caches at position len - 1, fp32,
    one launch -- the bits of linear_rows_f32(x, ln_w, ln_b, eps, w, ...) then decode_kv_append.  Fails
    (CG_EINVAL) unless x / w / ln_w / ln_b are 8-B aligned."""
    B, C = x.shape
    _, H, Tmax, D = kcache.shape
    for t, name in ((x, "x"), (w, "w"), (qkv, "qkv"), (kcache, "kcache"), (vcache, "vcache")):
        if t.dtype != torch.float32 or not t.is_cuda or t.stride(-1) != 1:
            raise ValueError(f"decode_qkv_f32: {name} must be a float32 device tensor with unit column stride")
    if tuple(w.shape) != (3 * C, C) or tuple(qkv.shape) != (B, 3 * C) or H * D != C or \
            tuple(kcache.shape) != (B, H, Tmax, D) or not kcache.is_contiguous() or \
            tuple(vcache.shape) != tuple(kcache.shape) or not vcache.is_contiguous():
        raise ValueError(f"decode_qkv_f32: shapes x {tuple(x.shape)} w {tuple(w.shape)} kcache {tuple(kcache.shape)}")
    L.check(L.load().cg_decode_qkv_f32(B, C, H, L.ptr(x), x.stride(0), L.ptr(ln_w), L.ptr(ln_b), eps, L.ptr(w),
                                       w.stride(0), L.ptr(qkv), qkv.stride(0), L.ptr(len_dev), Tmax, L.ptr(kcache),
                                       L.ptr(vcache), _s(x)), "decode_qkv_f32")


@_op("decode_attn", ("o",))
def decode_attn(q: Tensor, ldq: int, k: Tensor, k_off: int, v: Tensor, v_off: int, sb: int, sh: int, sj: int, B: int,
                H: int, D: int, len_dev: Optional[Tensor], nkeys: int, scale: float, o: Tensor) -> None:
    es = k.element_size()
    L.check(L.load().cg_decode_attn(L.ptr(q), ldq, k.data_ptr() + k_off * es, v.data_ptr() + v_off * es, sb, sh, sj,
                                    B, H, D, L.ptr(len_dev), nkeys, scale, L.ptr(o), o.stride(0), _s(q)),
            "decode_attn")


@_op("decode_sample", ("idx",))
def decode_sample(logits: Tensor, greedy: bool, seed: Tensor, len_dev: Tensor, idx: Tensor) -> None:
    B, V = logits.shape
    L.check(L.load().cg_decode_sample(L.ptr(logits), logits.stride(0), V, B, int(greedy), L.ptr(seed),
                                      L.ptr(len_dev), L.ptr(idx), idx.stride(0), _s(logits)), "decode_sample")


@_op("decode_sample_filtered", ("idx",))
def decode_sample_filtered(logits: Tensor, params: Tensor, seed: Tensor, len_dev: Tensor, idx: Tensor) -> None:
    """decode_sample's draw under a temperature, a top-k and a top-p cut (include/charpt.h
    cg_decode_sample_filtered): params = three device floats (temperature, top_k or 0, top_p) read by
    the kernel, so a captured graph serves every setting."""
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("decode_sample_filtered: logits must be float32 [B, V] with unit column stride")
    if params.dtype != torch.float32 or params.numel() < 3 or not params.is_contiguous():
        raise ValueError("decode_sample_filtered: params must be three contiguous float32 (temperature, top_k, top_p)")
    B, V = logits.shape
    L.check(L.load().cg_decode_sample_filtered(L.ptr(logits), logits.stride(0), V, B, L.ptr(params), L.ptr(seed),
                                               L.ptr(len_dev), L.ptr(idx), idx.stride(0), _s(logits)),
            "decode_sample_filtered")


@_op("decode_emit", ("end", "idx", "logprob"))
def decode_emit(logits: Tensor, emit_mode: int, params: Optional[Tensor], seed: Tensor, len_dev: Tensor,
                prompt_len: Tensor, limit: Tensor, end: Tensor, stop_bits: Tensor, pad: Tensor, idx: Tensor,
                logprob: Optional[Tensor]) -> None:
    """The ragged batch's per-row epilogue (include/charpt.h cg_decode_emit): forced prompt tokens, the
    samplers' token (emit_mode 0 greedy, 1 plain draw, 2 filtered draw with params), stop tokens, the per-row
    limit and, when logprob is given, the token's log-probability -- column *len_dev of idx / logprob.
    (The C ABI's `mode` is `emit_mode` here: torch's functionalization wrapper of a mutating op has an
    argument called `mode` of its own, and opcheck fails on the clash.)"""
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("decode_emit: logits must be float32 [B, V] with unit column stride")
    B, V = logits.shape
    for t, name in ((prompt_len, "prompt_len"), (limit, "limit"), (end, "end")):
        if t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous():
            raise ValueError(f"decode_emit: {name} must be {B} contiguous int64")
    if stop_bits.dtype != torch.int64 or stop_bits.numel() < (V + 63) // 64 or not stop_bits.is_contiguous():
        raise ValueError("decode_emit: stop_bits must be ceil(V / 64) contiguous 64-bit words (an int64 tensor)")
    if pad.dtype != torch.int64 or pad.numel() != 1:
        raise ValueError("decode_emit: pad must be one int64")
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != B or idx.stride(1) != 1:
        raise ValueError("decode_emit: idx must be int64 [B, ld] with unit column stride")
    if logprob is not None and (logprob.dtype != torch.float32 or logprob.dim() != 2 or logprob.stride(1) != 1
                                or logprob.stride(0) != idx.stride(0) or logprob.shape[0] != B):
        raise ValueError("decode_emit: logprob must be float32 [B, ld] with idx's row stride")
    if params is not None and (params.dtype != torch.float32 or params.numel() < 3 or not params.is_contiguous()):
        raise ValueError("decode_emit: params must be three contiguous float32 (temperature, top_k, top_p)")
    L.check(L.load().cg_decode_emit(L.ptr(logits), logits.stride(0), V, B, emit_mode, L.ptr(params), L.ptr(seed),
                                    L.ptr(len_dev), L.ptr(prompt_len), L.ptr(limit), L.ptr(end), L.ptr(stop_bits),
                                    L.ptr(pad), L.ptr(idx), idx.stride(0), L.ptr(logprob), _s(logits)), "decode_emit")


@_op("decode_prefill_attn", ("kcache", "vcache", "o"))
def decode_prefill_attn(q: Optional[Tensor], k: Tensor, v: Tensor, P: int, scale: float, kcache: Tensor,
                        vcache: Tensor, o: Optional[Tensor]) -> None:
    """One-pass prompt prefill of a layer (include/charpt.h cg_decode_prefill_attn): q, k, v [B * P, H * D]
    float32 views (unit column stride; k and v one row stride) of the QKV rows of B x P positions; the
    [B, H, Tmax, D] caches get rows t < P, o [B * P, H * D] what decode_attn gives position t with t + 1
    keys, bit for bit.  q = o = None: the cache rows only."""
    if kcache.dim() != 4 or kcache.dtype != torch.float32 or not kcache.is_contiguous() or \
            vcache.dtype != torch.float32 or tuple(vcache.shape) != tuple(kcache.shape) or not vcache.is_contiguous():
        raise ValueError("decode_prefill_attn: kcache and vcache must be dense float32 [B, H, Tmax, D] of one shape")
    B, H, Tmax, D = kcache.shape
    if (q is None) != (o is None):
        raise ValueError("decode_prefill_attn: q and o must both be given or both be None")
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (B * P, H * D)
                              or t.stride(1) != 1 or t.device != kcache.device):
            raise ValueError(f"decode_prefill_attn: {name} must be float32 [B * P, H * D] = [{B * P}, {H * D}] with "
                             f"unit column stride on {kcache.device}")
    if k.stride(0) != v.stride(0):
        raise ValueError("decode_prefill_attn: k and v must have one row stride")
    L.check(L.load().cg_decode_prefill_attn(L.ptr(q), 0 if q is None else q.stride(0), L.ptr(k), L.ptr(v), k.stride(0),
                                            B, P, H, D, Tmax, scale, L.ptr(kcache), L.ptr(vcache), L.ptr(o),
                                            0 if o is None else o.stride(0), _s(k)), "decode_prefill_attn")


@_op("decode_logprob_rows", ("logprob",))
def decode_logprob_rows(logits: Tensor, P: int, idx: Tensor, logprob: Tensor) -> None:
    """logprob[b, t + 1] = log softmax(logits[b * P + t])[idx[b, t + 1]] for t < P, decode_emit's log-prob bit
    for bit (include/charpt.h cg_decode_logprob_rows): logits float32 [B * P, V], idx int64 and logprob
    float32 [B, > P], unit column strides."""
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("decode_logprob_rows: logits must be float32 [B * P, V] with unit column stride")
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.stride(1) != 1:
        raise ValueError("decode_logprob_rows: idx must be int64 [B, > P] with unit column stride")
    B = idx.shape[0]
    if P < 1 or logits.shape[0] != B * P or idx.shape[1] <= P:
        raise ValueError(f"decode_logprob_rows: logits {tuple(logits.shape)} and idx {tuple(idx.shape)} do not hold "
                         f"B x P = {B} x {P} rows and column P")
    if logprob.dtype != torch.float32 or logprob.dim() != 2 or logprob.stride(1) != 1 or logprob.shape[0] != B or \
            logprob.shape[1] <= P:
        raise ValueError("decode_logprob_rows: logprob must be float32 [B, > P] with unit column stride")
    L.check(L.load().cg_decode_logprob_rows(L.ptr(logits), logits.stride(0), logits.shape[1], B, P, L.ptr(idx),
                                            idx.stride(0), L.ptr(logprob), logprob.stride(0), _s(logits)),
            "decode_logprob_rows")


# ---------------------------------------------------------------------------------------
@_op("adamw", ("p", "m", "v", "p_bf16"))
def adamw(p: Tensor, g: Tensor, m: Tensor, v: Tensor, p_bf16: Optional[Tensor], lr: float, beta1: float, beta2: float,
          eps: float, weight_decay: float, step: Tensor) -> None:
    L.check(L.load().cg_adamw(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(p_bf16), p.numel(), lr, beta1, beta2, eps,
                              weight_decay, L.ptr(step), _s(p)), "adamw")


@_op("adamw_defer", ("p", "m", "v", "p_bf16"))
def adamw_defer(p: Tensor, g: Tensor, m: Tensor, v: Tensor, p_bf16: Tensor, lr: float, beta1: float, beta2: float,
                eps: float, weight_decay: float, step: Tensor) -> None:
    """adamw over one region, queued: run by the free blocks of the next part-filling persistent GEMM
    launch on this stream, or by cg_flush_deferred (csrc defer.hip cg_adamw_defer); same bits."""
    L.check(L.load().cg_adamw_defer(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(p_bf16), p.numel(), lr, beta1,
                                    beta2, eps, weight_decay, L.ptr(step), _s(p)), "adamw_defer")


@_op("adamw_segments", ("p", "m", "v", "p_bf16"))
def adamw_segments(p: Tensor, g: Tensor, m: Tensor, v: Tensor, p_bf16: Optional[Tensor], segs: List[int],
                   lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: Tensor) -> None:
    """adamw over [start, start + length) segments of the flat buffers (segs = [s0, n0, s1, n1, ...])."""
    arr = (L.ctypes.c_int64 * len(segs))(*segs)
    L.check(L.load().cg_adamw_segments(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(p_bf16), arr, len(segs) // 2, lr,
                                       beta1, beta2, eps, weight_decay, L.ptr(step), _s(p)), "adamw_segments")


@_op("adamw_dyn", ("p", "m", "v", "p_bf16"))
def adamw_dyn(p: Tensor, g: Tensor, m: Tensor, v: Tensor, p_bf16: Optional[Tensor], lr: Tensor,
              gscale: Optional[Tensor], beta1: float, beta2: float, eps: float, weight_decay: float,
              step: Tensor) -> None:
    """adamw with the learning rate a device float64 scalar read when the kernel runs and, when given,
    the gradient multiplied by the device float32 scalar ``gscale`` first (g itself stays as it is)."""
    if lr.dtype != torch.float64 or (gscale is not None and gscale.dtype != torch.float32):
        raise TypeError("charpt adamw_dyn: lr must be a float64 tensor, gscale a float32 tensor")
    L.check(L.load().cg_adamw_dyn(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(p_bf16), p.numel(), L.ptr(lr),
                                  L.ptr(gscale), beta1, beta2, eps, weight_decay, L.ptr(step), _s(p)), "adamw_dyn")


def grad_norm_workspace(n: int) -> int:
    return int(L.load().cg_grad_norm_workspace(n))


@_op("grad_norm", ("out", "ws"))
def grad_norm(g: Tensor, max_norm: float, out: Tensor, ws: Tensor) -> None:
    """out[0] = the L2 norm of g (fp64 accumulation, deterministic), out[1] = min(1, max_norm / (norm + 1e-6));
    out: 2 float32, ws: grad_norm_workspace(g.numel()) bytes."""
    if not g.is_contiguous() or g.dtype != torch.float32 or out.dtype != torch.float32 or out.numel() < 2:
        raise ValueError("charpt grad_norm: g must be contiguous float32, out two float32")
    if ws.numel() * ws.element_size() < grad_norm_workspace(g.numel()):
        raise ValueError("charpt grad_norm: workspace too small")
    L.check(L.load().cg_grad_norm(L.ptr(g), g.numel(), max_norm, L.ptr(out), L.ptr(ws), _s(g)), "grad_norm")


@_op("scale_", ("x",))
def scale_(x: Tensor, scale: Tensor) -> None:
    """x *= scale (a device float32 scalar), in place."""
    if not x.is_contiguous() or x.dtype != torch.float32 or scale.dtype != torch.float32:
        raise ValueError("charpt scale_: x must be contiguous float32, scale a float32 tensor")
    L.check(L.load().cg_scale_f32(L.ptr(x), x.numel(), L.ptr(scale), _s(x)), "scale_f32")


# ---------------------------------------------------------------------------------------
# Fake (meta) implementations of the out-style ops above: each returns None and only writes
# buffers it declares as mutated, so FakeTensor / torch.compile tracing treats it as a no-op on
# shapes.
for _name, _obj in list(globals().items()):
    if isinstance(_obj, torch._library.custom_ops.CustomOpDef):
        _obj.register_fake(lambda *a, **k: None)


# ---------------------------------------------------------------------------------------
# Functional ops with fake + autograd registrations (torch.library.register_fake /
# register_autograd): the traceable seam of the GPT1.py module surface outside the fused model
# path -- nn.LayerNorm (GPT1.py:159-160,173), nn.Linear (:103-105,131,143,145,174) and the causal
# softmax-attention of Head / MultiHeadAttention (:109-123,134-135), all heads at once.  The
# fused training nodes (functional.AttnSublayerFn / FFNSublayerFn / HeadLossFn) stay
# autograd.Functions: they write parameter gradients straight into the model's flat gradient
# buffer, hand bf16 gradient copies between sublayers (GradLink) and fork side-stream work --
# effects a functional custom op cannot express.  Forward and backward are each ONE custom op, so a
# tracer only ever sees their fakes; all host-side kernel selection stays inside the real bodies.
def _flat_rows(x):
    return x.reshape(-1, x.shape[-1])


@torch.library.custom_op(f"{_NS}::layer_norm", mutates_args=(), device_types="cuda")
def layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float) -> tuple[Tensor, Tensor, Tensor]:
    """y = (x - mean) * rstd * weight + bias over the last dim (fp32); also returns mean, rstd."""
    x2 = _flat_rows(x).contiguous()
    rows = x2.shape[0]
    y = torch.empty_like(x2)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    layernorm_fwd(x2, weight, bias, y, mean, rstd, eps)
    return y.view(x.shape), mean, rstd


@layer_norm.register_fake
def _(x, weight, bias, eps):
    rows = x.numel() // x.shape[-1]
    return torch.empty_like(x), x.new_empty(rows), x.new_empty(rows)


@torch.library.custom_op(f"{_NS}::layer_norm_backward", mutates_args=(), device_types="cuda")
def layer_norm_backward(dy: Tensor, x: Tensor, weight: Tensor, mean: Tensor, rstd: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    x2 = _flat_rows(x).contiguous()
    rows, C = x2.shape
    dx = torch.empty_like(x2)
    dw = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = torch.empty(layernorm_bwd_workspace(rows, C) // 4 + 1, dtype=torch.float32, device=x.device)
    layernorm_bwd(_flat_rows(dy).float().contiguous(), x2, weight, mean, rstd, None, dx, None, dw, db, False, ws, None,
                  False, 0.0, 0, None, 0)
    return dx.view(x.shape), dw, db


@layer_norm_backward.register_fake
def _(dy, x, weight, mean, rstd):
    C = x.shape[-1]
    return torch.empty_like(x), x.new_empty(C), x.new_empty(C)


def _ln_setup(ctx, inputs, output):
    x, weight, _, _ = inputs
    _, mean, rstd = output
    ctx.save_for_backward(x, weight, mean, rstd)


def _ln_backward(ctx, dy, _dmean, _drstd):
    x, weight, mean, rstd = ctx.saved_tensors
    dx, dw, db = layer_norm_backward(dy, x, weight, mean, rstd)
    return dx, dw, db, None


layer_norm.register_autograd(_ln_backward, setup_context=_ln_setup)


@torch.library.custom_op(f"{_NS}::linear", mutates_args=(), device_types="cuda")
def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    """y = x weight^T (+ bias): fp32 (exact f32 MFMA) or bf16 (bf16 MFMA, fp32 accumulate) operands,
    bias fp32, output in x's dtype."""
    from . import functional as Fn
    x2 = _flat_rows(x).contiguous()
    out = torch.empty((x2.shape[0], weight.shape[0]), dtype=x.dtype, device=x.device)
    Fn.linear_fwd(x2, weight.contiguous(), out, "bias" if bias is not None else "store", bias=bias)
    return out.view(*x.shape[:-1], weight.shape[0])


@linear.register_fake
def _(x, weight, bias):
    return x.new_empty((*x.shape[:-1], weight.shape[0]))


@torch.library.custom_op(f"{_NS}::linear_backward", mutates_args=(), device_types="cuda")
def linear_backward(dy: Tensor, x: Tensor, weight: Tensor, with_bias: bool) -> tuple[Tensor, Tensor, Tensor]:
    """(dx, dweight, dbias): dy weight, dy^T x (fp32 accumulation, deterministic split-K), colsum(dy);
    dbias is empty when with_bias is False."""
    from . import functional as Fn
    dy2 = _flat_rows(dy).to(x.dtype).contiguous()
    x2 = _flat_rows(x).contiguous()
    w = weight.contiguous()
    dx = torch.empty_like(x2)
    Fn.linear_dgrad(dy2, w, dx)
    dw32 = torch.empty(w.shape, dtype=torch.float32, device=x.device)
    Fn.linear_wgrad(dy2, x2, dw32, 0.0)
    dw = dw32 if w.dtype == torch.float32 else Fn.to_act(dw32, w.dtype)
    db = torch.empty(w.shape[0] if with_bias else 0, dtype=torch.float32, device=x.device)
    if with_bias:
        Fn.colsum_into(dy2, db, 0.0)
    return dx.view(x.shape), dw, db


@linear_backward.register_fake
def _(dy, x, weight, with_bias):
    return torch.empty_like(x), torch.empty_like(weight), x.new_empty(weight.shape[0] if with_bias else 0,
                                                                      dtype=torch.float32)


def _lin_setup(ctx, inputs, output):
    x, weight, bias = inputs
    ctx.save_for_backward(x, weight)
    ctx.with_bias = bias is not None


def _lin_backward(ctx, dy):
    x, weight = ctx.saved_tensors
    dx, dw, db = linear_backward(dy, x, weight, ctx.with_bias)
    return dx, dw, (db if ctx.with_bias else None)


linear.register_autograd(_lin_backward, setup_context=_lin_setup)


@torch.library.custom_op(f"{_NS}::causal_attention", mutates_args=(), device_types="cuda")
def causal_attention(qkv: Tensor, n_head: int, head_size: int, scale: float, dropout_p: float, seed: int,
                     rng_call: Optional[Tensor], site: int) -> tuple[Tensor, Tensor]:
    """All heads of GPT1.py's Head.forward at once: qkv [B, T, 3*H*D] (queries of every head, then
    keys, then values; head-major inside each) -> (out [B, T, H*D] = the torch.cat of GPT1.py:135,
    logsumexp [B, H, T]).  Causal mask, softmax with scale (n_embd^-0.5), Philox dropout on
    the probabilities (dropout stream (rng_call, site), key seed)."""
    from . import functional as Fn
    B, T, _ = qkv.shape
    d = n_head * head_size
    q2 = qkv.reshape(B * T, 3 * d).contiguous()
    o = torch.empty((B * T, d), dtype=qkv.dtype, device=qkv.device)
    lse, _mask = Fn.attention_fwd(q2, B, T, n_head, head_size, o, scale, dropout_p, seed, rng_call, site)
    return o.view(B, T, d), lse


@causal_attention.register_fake
def _(qkv, n_head, head_size, scale, dropout_p, seed, rng_call, site):
    B, T, _ = qkv.shape
    return qkv.new_empty((B, T, n_head * head_size)), qkv.new_empty((B, n_head, T), dtype=torch.float32)


@torch.library.custom_op(f"{_NS}::causal_attention_backward", mutates_args=(), device_types="cuda")
def causal_attention_backward(dout: Tensor, qkv: Tensor, out: Tensor, lse: Tensor, n_head: int, head_size: int,
                              scale: float, dropout_p: float, seed: int, rng_call: Optional[Tensor],
                              site: int) -> Tensor:
    """d qkv of causal_attention (the forward's dropout keep bits are regenerated from the stream)."""
    from . import functional as Fn
    B, T, _ = qkv.shape
    d = n_head * head_size
    q2 = qkv.reshape(B * T, 3 * d).contiguous()
    dq = Fn.attention_bwd(q2, B, T, n_head, head_size, out.reshape(B * T, d).contiguous(),
                          dout.reshape(B * T, d).to(qkv.dtype).contiguous(), lse.contiguous(), scale, dropout_p, seed,
                          rng_call, site, None)
    return dq.view(qkv.shape)


@causal_attention_backward.register_fake
def _(dout, qkv, out, lse, n_head, head_size, scale, dropout_p, seed, rng_call, site):
    return torch.empty_like(qkv)


def _attn_setup(ctx, inputs, output):
    qkv, n_head, head_size, scale, p, seed, rng_call, site = inputs
    o, lse = output
    ctx.save_for_backward(qkv, o, lse, rng_call)
    ctx.args = (n_head, head_size, scale, p, seed, site)


def _attn_backward(ctx, dout, _dlse):
    qkv, o, lse, rng_call = ctx.saved_tensors
    n_head, head_size, scale, p, seed, site = ctx.args
    dq = causal_attention_backward(dout, qkv, o, lse, n_head, head_size, scale, p, seed, rng_call, site)
    return dq, None, None, None, None, None, None, None


causal_attention.register_autograd(_attn_backward, setup_context=_attn_setup)
