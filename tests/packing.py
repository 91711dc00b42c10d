"""Shared statements and references of the packed-row tests (test_cpu_packing.py, test_gpu_packed_*.py).

* ``plain_first_fit`` / ``plain_rows`` / ``plain_sampler`` -- what data.PackedPairSampler must build and
  return, from the raw pairs in plain Python.
* ``seg_of_lengths`` / ``seg_end_of`` / ``segments`` -- seg_start rows from segment lengths and back.
* ``attn_ref_seg`` -- the dense fp64 attention reference with the block-diagonal causal mask and the
  Philox keep bits (test_gpu_ops._attn_ref plus the segment mask); ``attn_ref_alone`` -- every segment
  run through the unmasked causal reference in a row of its own (p = 0), reassembled; ``lse_ref_seg`` --
  the masked scores' logsumexp.
* ``RING_*`` / ``F32_*`` / ``RESCALE_*`` -- the segmentations and data recipes of the long-row op tests
  (test_gpu_packed_attn_long.py), with ``rescale_query_tiles``: where the lazy rescale must fire.
* ``packed_oracle`` -- the oracle run on each segment alone, reassembled: the model-level reference.
* ``PACKED_*`` / ``packed_train_sampler`` -- the seeded short pairs of the model-level tests at shape E.

Not a conftest and no fixtures: plain helpers, as tests/pairs.py and tests/footprint.py.
"""
import numpy as np
import torch

from oracle import gpt1_oracle as O
from oracle import philox

import pairs as PR

IGNORE = -100


# ---------------------------------------------------------------------------------------
# the sampler in plain Python
# ---------------------------------------------------------------------------------------
def truncated(pair, T):
    """pack_pairs' rule: a pair longer than T + 1 loses the front of its prompt."""
    p, c = list(pair[0]), list(pair[1])
    return p[max(0, len(p) + len(c) - (T + 1)):], c


def plain_first_fit(lengths, order, capacity):
    rows, used = [], []
    for n in order:
        for r in range(len(rows)):
            if used[r] + lengths[n] <= capacity:
                rows[r].append(n)
                used[r] += lengths[n]
                break
        else:
            rows.append([n])
            used.append(lengths[n])
    return rows


def plain_rows(pairs, rows, T, pad=0, ignore=IGNORE):
    """x, y, seg_start [len(rows), T] of packed rows given as lists of pair indices."""
    xs, ys, ss = [], [], []
    for members in rows:
        x, y, s = [], [], []
        for n in members:
            p, c = truncated(pairs[n], T)
            row, at = p + c, len(x)
            x += row[:-1]
            y += [ignore] * (len(p) - 1) + c
            s += [at] * (len(row) - 1)
        at = len(x)
        xs.append(x + [pad] * (T - at))
        ys.append(y + [ignore] * (T - at))
        ss.append(s + [at] * (T - at))
    return (torch.tensor(xs, dtype=torch.int64), torch.tensor(ys, dtype=torch.int64),
            torch.tensor(ss, dtype=torch.int32))


def plain_sampler(pairs, T, seed, pad=0):
    """The packed tables of both splits as PackedPairSampler(generator seeded ``seed``) builds them:
    90/10 split of the pairs, each split shuffled by one randperm (train first) and packed first-fit.
    Returns ({split: (x, y, seg_start, rows)}, generator) -- the generator as get_batch finds it."""
    g = torch.Generator().manual_seed(seed)
    n = int(0.9 * len(pairs))
    lengths = [len(sum(truncated(pr, T), [])) - 1 for pr in pairs]
    out = {}
    for split, lo, cnt in (("train", 0, n), ("val", n, len(pairs) - n)):
        if cnt > 0:
            order = (torch.randperm(cnt, generator=g) + lo).tolist()
            rows = plain_first_fit(lengths, order, T)
            out[split] = (*plain_rows(pairs, rows, T, pad), rows)
    return out, g


# ---------------------------------------------------------------------------------------
# segmentations
# ---------------------------------------------------------------------------------------
def seg_of_lengths(lengths, T):
    """seg_start row [T] (int32) of consecutive segments of these lengths; what is left is a last segment."""
    s, at = [], 0
    for n in lengths:
        s += [at] * n
        at += n
    assert at <= T, (lengths, T)
    return torch.tensor(s + [at] * (T - at), dtype=torch.int32)


def segments(seg_row):
    """[(start, end)] of one seg_start row."""
    T = len(seg_row)
    starts = sorted(set(int(v) for v in seg_row))
    return [(s, e) for s, e in zip(starts, starts[1:] + [T])]


def seg_end_of(seg_start):
    """seg_end [B, T] (int32) in plain Python: cg_seg_bounds' contract."""
    out = torch.empty_like(seg_start)
    for b in range(seg_start.shape[0]):
        for s, e in segments(seg_start[b]):
            out[b, s:e] = e
    return out


def seg_mask(seg_start):
    """bool [B, T, T]: query i sees key j iff seg_start[b, i] <= j <= i."""
    B, T = seg_start.shape
    j = torch.arange(T)
    return (j[None, None, :] <= j[None, :, None]) & (j[None, None, :] >= seg_start.long()[:, :, None])


# ---------------------------------------------------------------------------------------
# attention references (fp64)
# ---------------------------------------------------------------------------------------
def attn_ref_seg(q, k, v, scale, seg_start, p=0.0, seed=0, stream=0):
    """q, k, v [B, T, H, D] float64: softmax attention under the segment mask, with the oracle's
    dropout keep bits indexed by (b, h, query, key) of the whole row."""
    B, T, H, D = q.shape
    s = torch.einsum("bthd,bshd->bhts", q, k) * scale
    s = s.masked_fill(~seg_mask(seg_start)[:, None], float("-inf"))
    P = torch.softmax(s, dim=-1)
    if p > 0:
        idx = np.arange(B * H * T * T, dtype=np.uint64).reshape(B, H, T, T)
        keep = torch.from_numpy(philox.keep_mask(seed, stream, idx, p)).double()
        P = P * keep * float(np.float32(1 / (1 - p)))
    return torch.einsum("bhts,bshd->bthd", P, v)


def attn_ref_alone(q, k, v, scale, seg_start):
    """Every segment through the plain causal reference in a row of exactly its length (no dropout)."""
    out = torch.empty_like(q)
    for b in range(q.shape[0]):
        for s, e in segments(seg_start[b]):
            qs, ks, vs = q[b:b + 1, s:e], k[b:b + 1, s:e], v[b:b + 1, s:e]
            sc = torch.einsum("bthd,bshd->bhts", qs, ks) * scale
            sc = sc.masked_fill(~torch.tril(torch.ones(e - s, e - s, dtype=torch.bool)), float("-inf"))
            out[b:b + 1, s:e] = torch.einsum("bhts,bshd->bthd", torch.softmax(sc, dim=-1), vs)
    return out


def lse_ref_seg(q, k, scale, seg_start):
    """[B, H, T] float64: logsumexp of the scaled scores under the segment mask (independent of dropout)."""
    s = torch.einsum("bthd,bshd->bhts", q, k) * scale
    return torch.logsumexp(s.masked_fill(~seg_mask(seg_start)[:, None], float("-inf")), dim=-1)


# ---------------------------------------------------------------------------------------
# long rows (test_gpu_packed_attn_long.py; held without a GPU by test_cpu_packing.py)
# ---------------------------------------------------------------------------------------
def cycling(T, top=40):
    """Lengths 1, 2, .. top, 1, .. for as long as the next one fits; what is left is the last segment."""
    out, at, n = [], 0, 1
    while at + n <= T:
        out.append(n)
        at, n = at + n, n % top + 1
    return out


# bf16 D 64 beyond T 256: the ring kernels.  256-query blocks run as (last, x) pass pairs per workgroup
# (T 576: blocks (2, 0) and the single pass 1; T 1024: (3, 0) and (2, 1)), the dK/dV kernel cuts keys in
# blocks of 128.  The lists put bounds on 256 k and either side of it, on 128 k +- 1, segments that start in
# every query block >= 1 (whole leading tiles skipped while the keep words advance), long single segments
# that begin late ([300], [513]) and many short ones.
RING_SHAPES = [(2, 512, 2), (2, 576, 3), (1, 1024, 2)]   # B, T, H
RING_SEGS = {
    512: [[], [256], [255, 2], [257, 1, 200], [128, 128, 128], [127, 2, 127, 129], [300], [10, 490], [273, 40, 7],
          cycling(512)],
    576: [[], [512], [511, 2], [513], [300], [64] * 8, [200, 150, 100], [320, 1, 1, 200]],
    1024: [[], [512], [767, 2, 200], [700, 300]],
}
# (T, lengths, index of the kept segment): one across the query-block edge at 256, one wholly inside the last
# query block, the first; at T 1024 one inside the last block of a two-workgroup grid
RING_LEAK = {"straddle": (576, [200, 150, 100], 1), "last-block": (576, [200, 150, 170, 30], 3),
             "first": (576, [200, 150, 100], 0), "last-block-1024": (1024, [300, 500, 100], 2)}

# fp32, D <= 32, p = 0: the MFMA forward in 64-query blocks of 4 waves x 16 queries over 64-key tiles.
# Bounds on 64 k and either side, on a wave's 16-query edge and either side ([79, 2, ..], [81], 16 k), inside a
# wave ([70, ..]: tiles masked for some of its lanes only), segments that start at >= 64 and >= 128 (whole
# tiles masked for every query of a wave), length-1 segments on a tile edge, and [].
F32_SHAPES = [(2, 130, 4, 16), (2, 200, 2, 8), (2, 256, 2, 32), (1, 300, 3, 21)]   # B, T, H, D
F32_SEGS = {
    130: [[], [64], [63, 2], [65, 1, 62], [81], [70, 58, 1], [128, 1], [127, 1, 1], [129], [16, 48, 1, 63],
          [79, 2, 31]],
    200: [[], [79, 2, 80], [81], [64, 64, 64], [63, 2, 63, 2, 63], [128, 48], [129, 1, 60], [100, 92], [192, 1],
          [127, 1, 64]],
    256: [[], [64, 64, 64], [63, 2, 127, 1, 62], [65, 127], [79, 2, 80], [81, 95], [128, 127], [129, 63, 1],
          [200, 50], [255]],
    300: [[], [256], [255, 2], [257, 1, 41], [64, 64, 64, 64], [79, 2, 79, 130], [81, 47, 129], [192, 100],
          [290, 9], [63, 1, 64, 1, 127, 1]],
}
F32_LEAK = {130: [60, 44, 10], 300: [70, 122, 64]}


def seg_batches(rows, B, T):
    """The segmentations ``rows`` of T as seg_start tensors [B, T], B rows at a time (the first ones again
    to fill the last batch): different rows of a batch get different segmentations."""
    rows = rows + rows[:(-len(rows)) % B]
    return [torch.stack([seg_of_lengths(r, T) for r in rows[i:i + B]]) for i in range(0, len(rows), B)]


# the lazy rescale forced inside a segment (bf16 D 64, H 2): (T, lengths)
RESCALE_THR = 8.0          # attention_common.h: the running max moves when a tile's max exceeds it by 2^8
RESCALE_MIN_SEGMENT = 130
RESCALE_RECIPES = [(256, [40, 200]), (512, [100, 250]), (1024, [300, 5, 400])]


def rescale_data(T, lengths, H=2, D=64, seed=31):
    """test_attention_forward_rescale_branch's recipe inside every segment of >= 130 positions: queries that
    share a direction, one key row (at 70 % of the segment) that matches it strongly, and the first head's
    key norms growing over the segment.  Returns qkv [T, 3 H D] bf16, the seg_start row and scale."""
    g = torch.Generator().manual_seed(seed)
    d = H * D
    seg_row = seg_of_lengths(lengths, T)
    qkv = torch.randn(T, 3 * d, generator=g) * 0.5
    qkv[:, :d] += 2.0
    for s, e in segments(seg_row):
        n = e - s
        if n >= RESCALE_MIN_SEGMENT:
            qkv[s + int(0.7 * n), d:2 * d] = 8.0
            qkv[s:e, d:d + D] *= torch.linspace(0.1, 3.0, n)[:, None]
    return qkv.to(torch.bfloat16), seg_row, D ** -0.5


def rescale_fires(q, k, scale, seg_row):
    """bool [H, T, tiles - 1]: (head, query, 64-key tile t + 1) at which the kernels' lazy rescale must fire --
    the tile (absolute tiles, as the kernels cut them) is not the query's first visible one and its maximum
    exceeds that of the query's earlier visible tiles by more than RESCALE_THR in log2 units.  q, k
    [1, T, H, D] float64.  (The kernels' stale running max never exceeds the true one.)"""
    T = q.shape[1]
    s = torch.einsum("bthd,bshd->bhts", q, k)[0] * (scale * 1.4426950408889634)
    s = s.masked_fill(~seg_mask(seg_row[None])[0][None], float("-inf"))
    tm = s.view(s.shape[0], T, T // 64, 64).amax(-1)                    # [H, T, tiles]
    before = torch.cummax(tm, dim=-1).values[..., :-1]
    return (before > float("-inf")) & (tm[..., 1:] > before + RESCALE_THR)


def rescale_query_tiles(q, k, scale, seg_row):
    """{(start, end): n} per segment: how many (head, query, tile) triples of rescale_fires it holds."""
    per_query = rescale_fires(q, k, scale, seg_row).sum((0, 2))
    return {(a, b): int(per_query[a:b].sum()) for a, b in segments(seg_row)}


# ---------------------------------------------------------------------------------------
# the model-level reference
# ---------------------------------------------------------------------------------------
def packed_oracle(P, x, y, seg_start, ocfg, device="cpu", autocast=False):
    """(logits [B, T, V], loss, grads) of the packed batch from the oracle run on every segment alone, in
    a row of exactly its length: logits placed back by segment, loss = sum of the segments' summed losses
    / the batch's valid count, gradients combined with the same weights (dropout off).  ``autocast``: the
    same under torch.autocast(bfloat16) on ``device`` -- the calibration e_t of the bf16 bar."""
    import contextlib
    B, T = x.shape
    P = {k: v.to(device) for k, v in P.items()}
    x, y = x.to(device), y.to(device)
    ctx = torch.autocast(device_type="cuda", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    logits = torch.empty((B, T, ocfg.vocab_size), dtype=torch.float32)
    total = int((y != IGNORE).sum())
    loss = torch.zeros((), dtype=torch.float64)
    grads = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in P.items()}
    seg_cpu = seg_start.cpu()
    with ctx:
        for b in range(B):
            for s, e in segments(seg_cpu[b]):
                xi, yi = x[b:b + 1, s:e], y[b:b + 1, s:e]
                n = int((yi != IGNORE).sum())
                if n == 0:   # the padding tail: logits only
                    with torch.no_grad():
                        logits[b, s:e] = O.forward(P, xi, ocfg)[0][0].float().cpu()
                    continue
                lg, l, g = O.loss_and_grads(P, xi, yi, ocfg)   # cross_entropy's mean over the segment's valid targets
                logits[b, s:e] = lg.float().cpu()
                loss += l.double().cpu() * n
                for k2, gv in g.items():
                    if gv is not None:
                        grads[k2] += gv.double().cpu() * n
    return logits, (loss / total).float(), {k2: (gv / total).float() for k2, gv in grads.items()}


# ---------------------------------------------------------------------------------------
# model-level data: shape E of tests/pairs.py with short pairs (3 .. 5 segments per row)
# ---------------------------------------------------------------------------------------
E_SHAPE = PR.E_SHAPE
PACKED_PAIRS_SEED, V = 777, PR.V
# PACKED_SAMPLER_SEED: chosen from the reference alone, by the procedure at pairs.SAMPLER_SEED -- of the seeds
# 60 .. 99 the one at whose first batch the packed oracle under autocast(bfloat16) on the GPU is furthest
# inside the bf16 rule's 0.999 cosine against the fp32 packed oracle (worst parameter 1 - cos 6.4e-4, at
# blocks.1.ln2.weight; 18 of the 40 seeds are inside at all, the worst of them all 1.44e-3).  A seed that
# stops being fair fails test_gpu_packed_train's "torch-bf16" entries and is replaced; the bars are not.
PACKED_SAMPLER_SEED = 65


def make_packed_pairs(n=120, seed=PACKED_PAIRS_SEED):
    """Prompts of 2 .. 6 and completions of 8 .. 14 tokens: 10 .. 20 tokens a pair, so a 64-token row
    holds three to five of them plus, usually, a short padding tail."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        lp = int(torch.randint(2, 7, (1,), generator=g))
        lc = int(torch.randint(8, 15, (1,), generator=g))
        out.append((torch.randint(1, V, (lp,), generator=g).tolist(), torch.randint(1, V, (lc,), generator=g).tolist()))
    return out


PACKED_PAIRS = make_packed_pairs()


def packed_train_sampler(device=None, world=1, rank=0, seed=PACKED_SAMPLER_SEED, B=None):
    from replicatinggpt_amd.data import PackedPairSampler
    return PackedPairSampler(PACKED_PAIRS, E_SHAPE["block_size"], E_SHAPE["B"] if B is None else B, world_size=world,
                             rank=rank, generator=torch.Generator().manual_seed(seed), device=device)


# ---------------------------------------------------------------------------------------
# end to end: pairs.E2E_FOUR packed into rows of 32
# ---------------------------------------------------------------------------------------
E2E_SHAPE = dict(PR.E2E_SHAPE, block_size=32)
E2E_B, E2E_LR, E2E_INIT_SEED, E2E_SAMPLER_SEED = PR.E2E_B, PR.E2E_LR, PR.E2E_INIT_SEED, PR.E2E_SAMPLER_SEED
# oracle_finetune_packed: the oracle reproduces all four completions first after 7 steps (and at every
# later one up to 40); the product trains twice as long (test_cpu_packing.py holds both numbers to the oracle)
E2E_ORACLE_STEPS, E2E_STEPS = 7, 14


def e2e_sampler(device=None):
    from replicatinggpt_amd.data import PackedPairSampler
    return PackedPairSampler(PR.E2E_PAIRS, E2E_SHAPE["block_size"], E2E_B,
                             generator=torch.Generator().manual_seed(E2E_SAMPLER_SEED), device=device)


def oracle_finetune_packed(steps):
    """The oracle's AdamW loop on the packed end-to-end batches (each segment alone: packed_oracle): per
    step, whether greedy decoding reproduces all four completions after it."""
    ocfg = O.OracleConfig(dropout=0.0, **E2E_SHAPE)
    torch.manual_seed(E2E_INIT_SEED)
    P = O.init_params(ocfg)
    opt = O.AdamWOracle(P, lr=E2E_LR)
    s = e2e_sampler(device="cpu")
    done = []
    for _ in range(steps):
        x, y, seg = s.get_batch("train")
        _, _, g = packed_oracle(P, x, y, seg, ocfg)
        opt.step(g)
        done.append(PR.oracle_reproduces(P, ocfg))
    return done
