"""Batched autoregressive decode engine for ``BigramLanguageModel.generate`` (GPT1.py:196-212).

The reference loop (per new token): crop ``idx[:, -block_size:]`` (GPT1.py:200), full forward
(:202), last row (:204), softmax (:206), multinomial (:208), append (:210).  Same token stream here,
computed as:

* phase 1 -- context length <= block_size: the window starts at position 0, so positions never
  change and each step pushes only the newest token through the blocks against a per-layer K/V
  cache (``cg_decode_embed``, ``cg_decode_kv_append``, ``cg_decode_attn``), plus ln_f / lm_head
  on those B rows;
* phase 2 -- context longer than block_size: the crop re-indexes positions from 0 every step
  (absolute learned position embeddings), so no K/V survives a step: the full window
  forward runs (``cg_decode_window`` gathers it on the device), except that the LAST block needs
  its queries / attention / projection / FFN only for the final row and ln_f / lm_head run on B
  rows instead of B x block_size;
* sampling on the device (``cg_decode_sample``): greedy = argmax (torch.argmax tie rule, the
  parity mode), else inverse-CDF draws from a Philox stream keyed by (seed, length, row) --
  torch.multinomial's CPU-generator stream is not reproducible on a GPU, so the sampled
  (non-greedy) stream is charpt's own, statistically the same distribution;
* a filtered engine (``filtered=True``: generate()'s temperature / top_k / top_p) samples with
  ``cg_decode_sample_filtered`` instead -- the same Philox draw over the tokens the top-k and
  nucleus cuts keep, weights at the temperature.  The three settings live in a device buffer the
  kernel reads when it runs, so ``generate(..., sampling=(t, k, p))`` rewrites twelve bytes and
  replays the graphs captured once; neutral settings there give ``cg_decode_sample``'s tokens
  bit for bit;
* a ragged engine (``ragged=True``: ``BigramLanguageModel.complete`` / ``score``) runs prompts of
  different lengths in lock step through the same two steps with ``cg_decode_emit`` as the sampling
  launch: it leaves ``idx[b, len]`` alone while ``len < prompt_len[b]`` (a forced token), writes the
  samplers' token after that, ends a row at a stop token or at its limit, pads ended rows and, on
  request, stores every token's log-probability.  Prompt lengths, limits, end flags, the stop set,
  the pad token and the sampling settings are device buffers rewritten per call.

The current length lives in a device int64, so each phase's step is one static-shape hipGraph
captured once and replayed per token.

Prompt prefill: an fp32 engine runs the prompt positions every row shares (``prefill_plan``) in one
eager forward over B x Pn rows (``_prefill_pass``: the engine's own row operations, whose values do
not depend on the row count, around ``cg_decode_prefill_attn``, which gives each position
``cg_decode_attn``'s arithmetic; with log-probs ``cg_decode_logprob_rows`` scores those columns) and
continues with the per-token steps from there -- the caches, tokens and log-probabilities are bit for
bit those of a per-token prefill, so a row still does not depend on its batch-mates.  Prompts below
``prefill_min`` positions, bf16 engines (their GEMM kernel, and so the order of every sum, is chosen
by the row count) and ``CHARPT_PREFILL_PASS=0`` replay the phase-1 graph without sampling once per
prompt position instead.  ``prefill_stats`` tells which happened in the last call.  fp32 models give
the reference's greedy stream (tests/test_gpu_model.py).
"""
import os

import torch

from . import functional as Fn
from . import ops
from .sampling import check_sampling, sampling_params

# CHARPT_DECODE_ROWS=0: the per-token LayerNorms in their own launches before ln1/ln2/lnf's Linears (A/B)
DECODE_ROWS = os.environ.get("CHARPT_DECODE_ROWS", "1") == "1"
# CHARPT_LAST_KV_SPLIT=0: the window step's last block computes Q for every row too (A/B)
LAST_KV_SPLIT = os.environ.get("CHARPT_LAST_KV_SPLIT", "1") == "1"
EMIT_GREEDY, EMIT_DRAW, EMIT_FILTERED = 0, 1, 2   # cg_decode_emit's mode
# CHARPT_PREFILL_PASS=0: every prompt position through its own phase-1 step, as before the one-pass prefill (A/B)
PREFILL_PASS = os.environ.get("CHARPT_PREFILL_PASS", "1") == "1"
# the shortest run of prompt positions the pass takes over from the per-token steps: the pass is a dozen eager
# launches per layer (1.6 ms at the C5 shape however short the prompt), a step one graph replay (0.25 ms), and
# a 16-token prompt is the shortest measured at which the pass wins by more than both spreads
# (profiles/prefill_ab.txt)
PREFILL_MIN = 15
# the pass's logits workspace: at most this many floats per row chunk of the scoring head
PREFILL_LOGITS_CAP = 1 << 26


def prefill_plan(pmin, T, logprobs, prefill_min):
    """How many prompt positions 0..Pn-1 the one-pass prefill covers (0: no pass) for a batch whose
    shortest prompt has ``pmin`` tokens, on a window of ``T``.  Without log-probs the pass replaces the
    no-head prefill steps: Pn = pmin - 1, and only when the first decided column pmin is still in phase
    1 (pmin <= T).  With log-probs it also scores the columns it covers (1..Pn) and stops one position
    early, Pn = min(pmin - 1, T) - 1: every such column n has n + 1 < pmin <= limit[b], so no row can end
    there and cg_decode_emit's rule for it is the log-prob store alone.  Below ``prefill_min`` positions
    the per-token steps stay."""
    if logprobs:
        Pn = min(pmin - 1, T) - 1
    else:
        Pn = pmin - 1 if pmin <= T else 0
    return Pn if Pn >= max(1, prefill_min) else 0


class DecodeEngine:
    def __init__(self, model, batch, max_len, greedy=True, seed=0, use_graph=True, filtered=False, ragged=False,
                 logprobs=False, prefill_pass=None, prefill_min=None):
        cfg = model.config
        if filtered and greedy and not ragged:
            raise ValueError("DecodeEngine: filtered sampling and greedy exclude each other")
        if logprobs and not ragged:
            raise ValueError("DecodeEngine: logprobs=True needs ragged=True")
        self.m, self.B, self.max_len = model, int(batch), int(max_len)
        self.T, self.C, self.H = cfg.block_size, cfg.n_embd, cfg.n_head
        self.D = self.C // self.H
        self.V = cfg.vocab_size
        self.L = len(model.blocks)
        self.greedy = bool(greedy)
        self.act = torch.bfloat16 if cfg.dtype == "bf16" else torch.float32
        self.dev = model.flat.master.device
        self.scale = Fn.attention_scale(self.C)
        dev, B, C = self.dev, self.B, self.C
        self.idx = torch.zeros((B, self.max_len), dtype=torch.int64, device=dev)
        self.len = torch.zeros(1, dtype=torch.int64, device=dev)
        self.seed = torch.full((1,), int(seed), dtype=torch.int64, device=dev)   # read by the sampler
        self.filtered = bool(filtered)
        # (temperature, top_k, top_p), read by the filtered sampler when it runs
        self.params = sampling_params().to(dev) if self.filtered else None
        self.kc = torch.zeros((self.L, B, self.H, self.T, self.D), dtype=torch.float32, device=dev)
        self.vc = torch.zeros_like(self.kc)
        self.win = torch.empty((B, self.T), dtype=torch.int64, device=dev)
        self.x1 = torch.empty((B, C), dtype=torch.float32, device=dev)
        self.logits = torch.empty((B, self.V), dtype=torch.float32, device=dev)
        self.use_graph = use_graph and dev.type == "cuda"
        self.g1 = self.g1_prefill = self.g2 = None
        # one-pass prefill: fp32 only -- a bf16 GEMM's kernel, and with it the k order of every sum, is
        # chosen by the row count, so a pass over B * Pn rows could not give the per-token steps' bits
        on = PREFILL_PASS if prefill_pass is None else bool(prefill_pass)
        self.prefill_pass = on and self.act == torch.float32 and self.D <= 64
        self.prefill_min = PREFILL_MIN if prefill_min is None else int(prefill_min)
        self.prefill_stats = {"passes": 0, "positions": 0, "step_replays": 0}   # of the last call
        self.ragged = bool(ragged)
        if self.ragged:
            # everything complete() varies per call is device memory cg_decode_emit reads when it runs
            self.params = sampling_params().to(dev)
            self.mode = EMIT_GREEDY            # a launch argument: one (g1, g2) pair per mode used
            self.prompt_len = torch.zeros(B, dtype=torch.int64, device=dev)
            self.limit = torch.zeros(B, dtype=torch.int64, device=dev)
            self.end = torch.zeros(B, dtype=torch.int64, device=dev)
            self.stop_bits = torch.zeros((self.V + 63) // 64, dtype=torch.int64, device=dev)
            self.pad = torch.zeros(1, dtype=torch.int64, device=dev)
            self.logprob = torch.zeros((B, self.max_len), dtype=torch.float32, device=dev) if logprobs else None
            self.rg = {}                       # mode -> (g1, g2)

    # -- regions -------------------------------------------------------------------------
    def _R(self, key):
        return self.m.flat.regions[key]

    def _w(self, key):
        return self._R(key).operand(self.act)

    def _b(self, key):
        return self._R(key).master

    def _ln(self, x2, key):
        # layernorm_fwd takes no row stride: a row-strided view (the window's final rows) goes in as a dense copy
        y, _, _ = Fn.layernorm(x2.contiguous(), self._b(key + "_w"), self._b(key + "_b"), self.act)
        return y

    def _ln_linear(self, x2, key, w, out, bias=None, relu=False):
        """out = act(LayerNorm_key(x2) @ w^T [+ bias]): fp32 per-token rows in one launch
        (ops.linear_rows_f32, k_gemm_f32r with the LayerNorm in its prologue -- the bits of the two
        launches); else the LayerNorm launch (on dense rows) and the GEMM.  x2 may be row-strided."""
        lw, lb = self._b(key + "_w"), self._b(key + "_b")
        M, K = x2.shape
        if (DECODE_ROWS and self.act == torch.float32 and M <= 2048 and x2.stride(0) % 2 == 0
                and ops.linear_rows_f32_supported(M, w.shape[0], K) and w.stride(0) % 2 == 0
                and ((x2.data_ptr() | w.data_ptr() | lw.data_ptr() | lb.data_ptr()) & 7) == 0):
            ops.linear_rows_f32(x2, lw, lb, 1e-5, w, bias, None, out, relu)
            return
        a = self._ln(x2, key)
        if bias is None:
            Fn.linear_fwd(a, w, out)
        else:
            Fn.linear_fwd(a, w, out, "bias_relu" if relu else "bias", bias=bias)

    def _ffn_tail(self, l, x2):
        """x + W2 relu(W1 ln2(x) + b1) + b2 for rows x2 [R, C] (eval: no dropout)."""
        h = torch.empty((x2.shape[0], 4 * self.C), dtype=self.act, device=self.dev)
        self._ln_linear(x2, f"{l}.ln2", self._w(f"{l}.w1"), h, bias=self._b(f"{l}.b1"), relu=True)
        out = torch.empty_like(x2)
        Fn.linear_fwd(h, self._w(f"{l}.w2"), out, "bias_resid", bias=self._b(f"{l}.b2"), resid=x2)
        return out

    def _head(self, x2):
        self._ln_linear(x2, "lnf", self._R("lm_w").operand(self.act), self.logits, bias=self._b("lm_b"))

    def _sample(self):
        if self.ragged:
            ops.decode_emit(self.logits, self.mode, self.params, self.seed, self.len, self.prompt_len, self.limit,
                            self.end, self.stop_bits, self.pad, self.idx, self.logprob)
        elif self.filtered:
            ops.decode_sample_filtered(self.logits, self.params, self.seed, self.len, self.idx)
        else:
            ops.decode_sample(self.logits, self.greedy, self.seed, self.len, self.idx)

    # -- phase 1: one token against the K/V caches ---------------------------------------------
    def _step1(self, sample):
        C, B = self.C, self.B
        ops.decode_embed(self.idx, self._b("wte"), self._b("wpe"), self.len, self.x1)
        x = self.x1
        for l in range(self.L):
            qkv = torch.empty((B, 3 * C), dtype=self.act, device=self.dev)
            wq = self._w(f"{l}.qkv")
            lw, lb = self._b(f"{l}.ln1_w"), self._b(f"{l}.ln1_b")
            if (DECODE_ROWS and self.act == torch.float32 and B <= 2048 and C <= 128 and C % 2 == 0
                    and x.stride(0) % 2 == 0 and wq.stride(0) % 2 == 0
                    and ((x.data_ptr() | wq.data_ptr() | lw.data_ptr() | lb.data_ptr()) & 7) == 0):
                # ln1 + QKV + the K / V append in one launch
                ops.decode_qkv_f32(x, lw, lb, 1e-5, wq, qkv, self.len, self.kc[l], self.vc[l])
                qkv32 = qkv
            else:
                self._ln_linear(x, f"{l}.ln1", wq, qkv)
                qkv32 = qkv if qkv.dtype == torch.float32 else qkv.float()
                ops.decode_kv_append(qkv32, C, 2 * C, self.len, self.kc[l], self.vc[l])
            o = torch.empty((B, C), dtype=torch.float32, device=self.dev)
            T, H, D = self.T, self.H, self.D
            ops.decode_attn(qkv32, qkv32.stride(0), self.kc[l], 0, self.vc[l], 0, H * T * D, T * D, D, B, H, D,
                            self.len, 0, self.scale, o)
            o = o if self.act == torch.float32 else o.to(self.act)
            x2 = torch.empty((B, C), dtype=torch.float32, device=self.dev)
            Fn.linear_fwd(o, self._w(f"{l}.proj_w"), x2, "bias_resid", bias=self._b(f"{l}.proj_b"), resid=x)
            x = self._ffn_tail(l, x2)
        if sample:
            self._head(x)
            self._sample()
        ops.counter_add(self.len, 1)

    # -- phase 2: the sliding window -------------------------------------------------------
    def _step2(self):
        B, T, C, H, D = self.B, self.T, self.C, self.H, self.D
        ops.decode_window(self.idx, self.len, self.win)
        x = torch.empty((B, T, C), dtype=torch.float32, device=self.dev)
        ops.embed_fwd(self.win, self._b("wte"), self._b("wpe"), x)
        for blk in self.m.blocks[:-1]:
            x = blk(x)
        # last block: K/V for every row, everything else for the final row only
        l = self.L - 1
        x2 = x.reshape(B * T, C)
        lw, lb = self._b(f"{l}.ln1_w"), self._b(f"{l}.ln1_b")
        wq = self._w(f"{l}.qkv")   # [3C, C]: Q rows, then K, then V
        o = torch.empty((B, C), dtype=torch.float32, device=self.dev)
        xl = x[:, T - 1, :]        # the final rows in place (row stride T C)
        if (LAST_KV_SPLIT and self.act == torch.float32 and Fn.ATTN_ROWS and Fn.FFN_LN and B * T > 2048
                and ops.linear_rows_f32_supported(B * T, 2 * C, C) and C % 2 == 0
                and ((lw.data_ptr() | lb.data_ptr() | x2.data_ptr() | wq.data_ptr()) & 7) == 0):
            # ln1 + the K / V columns for every row, ln1 + Q for the final rows only: each value the
            # same k-ordered chain as in the full QKV product, a third of its MFMAs skipped
            kv = torch.empty((B * T, 2 * C), dtype=torch.float32, device=self.dev)
            ops.linear_rows_f32(x2, lw, lb, 1e-5, wq[C:], None, None, kv)
            q = torch.empty((B, C), dtype=torch.float32, device=self.dev)
            self._ln_linear(xl, f"{l}.ln1", wq[:C], q)
            ops.decode_attn(q, q.stride(0), kv, 0, kv, C, T * 2 * C, D, 2 * C, B, H, D, None, T, self.scale, o)
        else:
            qkv = torch.empty((B * T, 3 * C), dtype=self.act, device=self.dev)
            Fn.linear_fwd(self._ln(x2, f"{l}.ln1"), wq, qkv)
            qkv32 = qkv if qkv.dtype == torch.float32 else qkv.float()
            qlast = qkv32.view(B, T, 3 * C)[:, T - 1, :]
            ld = qkv32.stride(0)
            ops.decode_attn(qlast, qlast.stride(0), qkv32, C, qkv32, 2 * C, T * ld, D, ld, B, H, D, None, T,
                            self.scale, o)
        o = o if self.act == torch.float32 else o.to(self.act)
        x3 = torch.empty((B, C), dtype=torch.float32, device=self.dev)
        Fn.linear_fwd(o, self._w(f"{l}.proj_w"), x3, "bias_resid", bias=self._b(f"{l}.proj_b"), resid=xl)
        x4 = self._ffn_tail(l, x3)
        self._head(x4)
        self._sample()
        ops.counter_add(self.len, 1)

    # -- one-pass prefill: prompt positions 0..Pn-1 of every row in one forward --------------------
    def _prefill_pass(self, Pn, score):
        """What Pn phase-1 steps from len = 1 leave, bit for bit: the K/V cache rows 0..Pn-1 of every
        layer, len = Pn + 1 and, with ``score``, logprob[:, 1..Pn].  The engine's own fp32 row operations at
        M = B Pn rows (each row's value is independent of the row count) around cg_decode_prefill_attn,
        which gives every position k_decode_attn's chain.  Eager, once per call: Pn varies per call.
        Without ``score`` nothing reads the last layer's output, so it computes ln1 + the K / V columns only."""
        B, C, H, D, T = self.B, self.C, self.H, self.D, self.T
        M = B * Pn
        x = torch.empty((M, C), dtype=torch.float32, device=self.dev)
        ops.embed_fwd(self.idx[:, :Pn].contiguous(), self._b("wte"), self._b("wpe"), x)
        for l in range(self.L):
            wq = self._w(f"{l}.qkv")   # [3C, C]: Q rows, then K, then V
            if l == self.L - 1 and not score:
                kv = torch.empty((M, 2 * C), dtype=torch.float32, device=self.dev)
                self._ln_linear(x, f"{l}.ln1", wq[C:], kv)
                ops.decode_prefill_attn(None, kv[:, :C], kv[:, C:], Pn, self.scale, self.kc[l], self.vc[l], None)
                break
            qkv = torch.empty((M, 3 * C), dtype=torch.float32, device=self.dev)
            self._ln_linear(x, f"{l}.ln1", wq, qkv)
            o = torch.empty((M, C), dtype=torch.float32, device=self.dev)
            ops.decode_prefill_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], Pn, self.scale, self.kc[l],
                                    self.vc[l], o)
            x2 = torch.empty((M, C), dtype=torch.float32, device=self.dev)
            Fn.linear_fwd(o, self._w(f"{l}.proj_w"), x2, "bias_resid", bias=self._b(f"{l}.proj_b"), resid=x)
            x = self._ffn_tail(l, x2)
        if score:
            # ln_f + lm_head + the log-prob of the next prompt token, whole batch rows per chunk
            nb = max(1, PREFILL_LOGITS_CAP // (Pn * self.V))
            lm_w, lm_b = self._R("lm_w").operand(self.act), self._b("lm_b")
            for b0 in range(0, B, nb):
                b1 = min(B, b0 + nb)
                logits = torch.empty(((b1 - b0) * Pn, self.V), dtype=torch.float32, device=self.dev)
                self._ln_linear(x[b0 * Pn:b1 * Pn], "lnf", lm_w, logits, bias=lm_b)
                ops.decode_logprob_rows(logits, Pn, self.idx[b0:b1], self.logprob[b0:b1])
        self.len.fill_(Pn + 1)
        self.prefill_stats["passes"] += 1
        self.prefill_stats["positions"] += Pn

    # -- driver ------------------------------------------------------------------------------
    def _graph(self, fn):
        if not self.use_graph:
            return None
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        saved = self.len.clone()
        with torch.cuda.stream(s):
            fn()                       # warm-up (allocator, kernels); state restored below
        torch.cuda.current_stream().wait_stream(s)
        self.len.copy_(saved)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        self.len.copy_(saved)          # capture does not execute, but keep the invariant explicit
        return g

    @torch.no_grad()
    def generate(self, idx, max_new_tokens, seed=None, sampling=None):
        """``sampling``: (temperature, top_k, top_p) for a filtered engine -- written to the device
        buffer the sampler reads, so every setting replays the same graphs; None keeps the last."""
        if self.ragged:
            raise ValueError("DecodeEngine: a ragged engine runs complete(), not generate()")
        B, L0 = idx.shape
        if sampling is not None:
            if not self.filtered:
                raise ValueError("DecodeEngine: sampling=(temperature, top_k, top_p) needs an engine built with filtered=True")
            check_sampling(*sampling)
        if B != self.B or L0 < 1 or L0 + max_new_tokens > self.max_len:
            raise ValueError(f"DecodeEngine(batch={self.B}, max_len={self.max_len}) cannot run idx {tuple(idx.shape)} "
                             f"+ {max_new_tokens} tokens")
        if sampling is not None:
            self.params.copy_(sampling_params(*sampling))
        was_training = self.m.training
        self.m.eval()
        try:
            if self.act == torch.bfloat16:
                self.m._sync_shadow()
            run1 = lambda: self._step1(True)      # noqa: E731
            run1p = lambda: self._step1(False)    # noqa: E731
            if self.use_graph and self.g1 is None:
                # capture before the prompt is written: the warm-up runs scribble on idx / caches
                self.len.fill_(1)
                self.g1 = self._graph(run1)
                self.g1_prefill = self._graph(run1p)
                if self.max_len > self.T:
                    self.g2 = self._graph(self._step2)
            if seed is not None:
                self.seed.fill_(int(seed))
            self.idx[:, :L0].copy_(idx)
            total = L0 + max_new_tokens
            self.prefill_stats = {"passes": 0, "positions": 0, "step_replays": 0}
            Pn = prefill_plan(L0, self.T, False, self.prefill_min) if self.prefill_pass else 0
            if L0 > self.T:                        # prompt longer than the window: phase 2 only
                self.len.fill_(L0)
                n = L0
            elif Pn:                               # positions 0..L0-2 in one pass
                self._prefill_pass(Pn, False)
                n = L0
            else:
                self.len.fill_(1)
                n = 1                              # tokens present, mirrored on the host
            while n < L0:                          # prompt prefill: positions 0..L0-2
                self.g1_prefill.replay() if self.g1_prefill else run1p()
                self.prefill_stats["step_replays"] += 1
                n += 1
            while n < total:
                if n <= self.T:
                    self.g1.replay() if self.g1 else run1()
                else:
                    self.g2.replay() if self.g2 else self._step2()
                n += 1
            return self.idx[:, :total].clone()
        finally:
            self.m.train(was_training)

    # -- ragged batches (BigramLanguageModel.complete) ---------------------------------------------
    def _ragged_graphs(self):
        """(g1, g1_prefill, g2) for the current mode, captured on first use (None each without graphs).
        The prefill step launches no emit kernel, so one graph serves every mode."""
        if not self.use_graph:
            return None, None, None
        if self.mode not in self.rg:
            # the warm-up runs scribble on idx / caches / end / logprob: complete() writes them afterwards
            self.len.fill_(1)
            if self.g1_prefill is None:
                self.g1_prefill = self._graph(lambda: self._step1(False))
            g1 = self._graph(lambda: self._step1(True))
            g2 = self._graph(self._step2) if self.max_len > self.T else None
            self.rg[self.mode] = (g1, g2)
        g1, g2 = self.rg[self.mode]
        return g1, self.g1_prefill, g2

    @torch.no_grad()
    def complete(self, idx, lens, max_new_tokens, mode=EMIT_GREEDY, seed=None, sampling=None, stop_bits=None, pad=0,
                 poll_every=32):
        """Continue a ragged batch in lock step: row b's prompt is idx[b, :lens[b]] (lens a CPU int64
        tensor, every entry in [1, idx.shape[1]]), and it runs until a stop token or lens[b] +
        max_new_tokens.  Column n of every row is decided by one cg_decode_emit launch after the step
        that consumed column n - 1: forced while n < lens[b], the sampler's token after that, pad once
        the row has ended -- so the phase-1 and phase-2 steps above run unchanged.  stop_bits: a CPU
        int64 tensor of ceil(V / 64) words (None: no stop token).  Returns (tokens [B, max(lens) +
        max_new_tokens], lengths [B], logprobs or None, head steps run)."""
        if not self.ragged:
            raise ValueError("DecodeEngine: complete() needs an engine built with ragged=True")
        B, Lmax = idx.shape
        pmin, pmax = int(lens.min()), int(lens.max())
        total = pmax + max_new_tokens
        if B != self.B or lens.numel() != B or pmin < 1 or pmax > Lmax or max_new_tokens < 0 or total > self.max_len:
            raise ValueError(f"DecodeEngine(batch={self.B}, max_len={self.max_len}) cannot run prompts of lengths "
                             f"{lens.tolist()} in idx {tuple(idx.shape)} + {max_new_tokens} tokens")
        if mode not in (EMIT_GREEDY, EMIT_DRAW, EMIT_FILTERED):
            raise ValueError(f"DecodeEngine: mode must be 0 (greedy), 1 (draw) or 2 (filtered draw), got {mode!r}")
        if sampling is not None:
            check_sampling(*sampling)
        want_lp = self.logprob is not None
        # the first column an emit launch has to decide: with log-probs every column from 1, else the
        # first one past the shortest prompt
        n0 = 1 if want_lp else (pmin if max_new_tokens > 0 else total)
        was_training = self.m.training
        self.m.eval()
        try:
            if self.act == torch.bfloat16:
                self.m._sync_shadow()
            self.mode = int(mode)
            g1, g1p, g2 = self._ragged_graphs() if n0 < total else (None, None, None)
            if sampling is not None:
                self.params.copy_(sampling_params(*sampling))
            if seed is not None:
                self.seed.fill_(int(seed))
            limit = lens + max_new_tokens
            self.prompt_len.copy_(lens)
            self.limit.copy_(limit)
            # a row whose budget is spent before the first emit launch has ended already
            self.end.copy_(torch.where(limit <= n0, limit, torch.zeros_like(limit)))
            if stop_bits is None:
                self.stop_bits.zero_()
            else:
                self.stop_bits.copy_(stop_bits)
            self.pad.fill_(int(pad))
            self.idx[:, :Lmax].copy_(idx)
            if want_lp:
                self.logprob.zero_()
            self.prefill_stats = {"passes": 0, "positions": 0, "step_replays": 0}
            steps = 0
            n = n0
            if n0 < total:                             # else no column is left to decide
                Pn = prefill_plan(pmin, self.T, want_lp, self.prefill_min) if self.prefill_pass else 0
                if n0 > self.T:                        # every prompt longer than the window: phase 2 only
                    self.len.fill_(n0)
                elif Pn:
                    # positions 0..Pn-1 in one pass; with log-probs it decides columns 1..Pn too (each
                    # counts as a head step), else it ends where the no-head steps would: len = n0
                    self._prefill_pass(Pn, want_lp)
                    if want_lp:
                        n, steps = Pn + 1, Pn
                else:
                    self.len.fill_(1)
                    for _ in range(1, n0):             # no output needed yet: the no-head prefill step
                        g1p.replay() if g1p else self._step1(False)
                        self.prefill_stats["step_replays"] += 1
                while n < total:
                    if n <= self.T:
                        g1.replay() if g1 else self._step1(True)
                    else:
                        g2.replay() if g2 else self._step2()
                    n += 1
                    steps += 1
                    if poll_every and steps % poll_every == 0 and n < total and not bool((self.end == 0).any()):
                        break
            tokens = self.idx[:, :total].clone()
            lengths = self.end.clone()
            logprobs = self.logprob[:, :total].clone() if want_lp else None
            # columns no step reached: pad / 0 (rows ended before n0 never met an emit launch either)
            cols = torch.arange(total, device=self.dev)[None, :]
            past = cols >= lengths[:, None]
            tokens.masked_fill_(past, int(pad))
            if want_lp:
                logprobs.masked_fill_(past, 0.0)
            return tokens, lengths, logprobs, steps
        finally:
            self.m.train(was_training)
