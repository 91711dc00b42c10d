"""Standalone A/B of the grouped split-K weight-gradient launch (cg_gemm_wgrad_group) against the single
launches it replaces, at the C2 shapes (16384 tokens): the attention sublayer's projection + QKV pair
(single splits 32 / 16, grouped 14) and the FeedForward's W2 + W1 pair (single 14 / 14, grouped 7).  Each
variant is 20 calls captured in a hipGraph -- GEMM launch(es) plus the in-line bf16-slab reduces -- replayed
7 times; the figure is the median replay / 20.  GPU only.  usage: python tools/wgrad_group_ab.py"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from replicatinggpt_amd import _lib as L  # noqa: E402
from replicatinggpt_amd import functional as Fn  # noqa: E402
from replicatinggpt_amd import ops  # noqa: E402

DEV = "cuda"
CALLS, REPLAYS = 20, 7


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    ts = []
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    K = 16384
    torch.manual_seed(0)

    def op(n):
        return (torch.randn(K, n, device=DEV) * 0.1).to(torch.bfloat16)
    pairs = {"attn proj+qkv": [(op(384), op(384)), (op(1152), op(384))],
             "ffn w2+w1": [(op(384), op(1536)), (op(1536), op(384))]}
    flags = L.GEMM_SLAB_BF16
    for name, pr in pairs.items():
        outs = [torch.empty(dy.shape[1], x.shape[1], device=DEV) for dy, x in pr]
        singles = [Fn._wgrad_split(dy.shape[1], x.shape[1], K, True) for dy, x in pr]
        gsplit = Fn._split_for_tiles(sum((dy.shape[1] // 128) * (x.shape[1] // 128) for dy, x in pr), K // 64)
        ws1 = [torch.empty(ops.gemm_workspace(dy.shape[1], x.shape[1], s) // 4, device=DEV)
               for (dy, x), s in zip(pr, singles)]
        wsg = [torch.empty(ops.gemm_workspace(dy.shape[1], x.shape[1], gsplit) // 4, device=DEV) for dy, x in pr]
        dys, xs = [p[0] for p in pr], [p[1] for p in pr]

        def two(splits=singles, wss=ws1):
            for (dy, x), o, s, w in zip(pr, outs, splits, wss):
                ops.gemm(dy, x, o, True, True, True, dy.shape[1], x.shape[1], K, dy.shape[1], x.shape[1], x.shape[1],
                         L.EPI_STORE, None, None, 0, None, 0, 0.0, 0, None, 0, 0.0, s, w, flags)

        def group():
            ops.gemm_wgrad_group(dys, xs, outs, wsg, [0.0, 0.0], [gsplit, gsplit], flags)
        assert ops.gemm_wgrad_group_supported(dys, xs, outs, wsg, [0.0, 0.0], [gsplit, gsplit], flags)
        for label, fn in ((f"two launches, splits {singles}", two),
                          (f"two launches, split {gsplit} each", lambda: two([gsplit, gsplit], wsg)),
                          (f"one grouped launch, split {gsplit}", group)):
            med, lo, hi = timed(fn)
            print(f"{name:14s} {label:36s} {med:7.2f} us  (min {lo:.2f}, max {hi:.2f})", flush=True)


if __name__ == "__main__":
    main()
