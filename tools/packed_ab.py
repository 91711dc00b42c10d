"""Same-process interleaved A/B of packed rows in the training step on one GPU, at the C2 shape (bf16,
dropout 0.2, hipGraph replay), on one fixed seeded synthetic pair set:
  "pairs"   data.PairSampler, one pair per row (the rest of the row is padding);
  "packed"  data.PackedPairSampler, the same pairs packed first-fit (segment-masked attention,
            positions restarting at each segment);
  "dense"   the bench path (BatchSampler, dense windows, no masks): what a step costs without the
            segment mask at the same B and T.
Each variant is its own model + optimizer + captured graph; rounds time each variant's replays in turn
(tools/masked_ce_ab.py's method), median / min ms per step, and valid targets per second from the valid
targets the timed batches actually held.  The pairs' lengths are those of tests/pairs.py: prompts of
6 .. 24 and completions of 36 .. 52 tokens.
usage: python tools/packed_ab.py [rounds] [steps] [n_pairs]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from replicatinggpt_amd import AdamW, BigramLanguageModel, PRESETS  # noqa: E402
from replicatinggpt_amd.data import BatchSampler, PackedPairSampler, PairSampler, TokenStream  # noqa: E402
from replicatinggpt_amd.engine import TrainStep  # noqa: E402


def synthetic_pairs(n, vocab, seed=4242):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        lp = int(torch.randint(6, 25, (1,), generator=g))
        lc = int(torch.randint(36, 53, (1,), generator=g))
        out.append((torch.randint(1, vocab, (lp,), generator=g).tolist(), torch.randint(1, vocab, (lc,), generator=g).tolist()))
    return out


def make(variant, pairs, dev):
    cfg = PRESETS["c2"].with_(dtype="bf16")
    torch.manual_seed(cfg.seed)
    model = BigramLanguageModel(cfg).to(dev)
    opt = AdamW(model.parameters(), lr=cfg.learning_rate).attach(model)
    gen = torch.Generator().manual_seed(cfg.seed)
    if variant == "dense":
        sampler = BatchSampler(TokenStream.synthetic(device=dev), cfg.block_size, cfg.batch_size, generator=gen)
    else:
        cls = PackedPairSampler if variant == "packed" else PairSampler
        sampler = cls(pairs, cfg.block_size, cfg.batch_size, generator=gen, device=dev)
    step = TrainStep(model, opt, sampler, None)
    step.capture()
    return step


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    n_pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    dev = torch.device("cuda")
    cfg = PRESETS["c2"]
    pairs = synthetic_pairs(n_pairs, cfg.vocab_size)
    variants = ("pairs", "packed", "dense")
    runs = {v: make(v, pairs, dev) for v in variants}
    for st in runs.values():
        for _ in range(10):
            st.step()
    torch.cuda.synchronize()
    res = {v: [] for v in variants}
    valid = {v: torch.zeros((), dtype=torch.int64, device=dev) for v in variants}
    for r in range(rounds):
        for v in variants:
            st = runs[v]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                st.step()
            torch.cuda.synchronize()
            res[v].append((time.perf_counter() - t0) / steps * 1e3)
        for v in variants:   # untimed: what one more batch of each variant holds
            runs[v].step()
            valid[v] += (runs[v].y != -100).sum() if v != "dense" else runs[v].y.numel()
        print(f"round {r}: " + "  ".join(f"{v} {res[v][-1]:.4f}" for v in variants), flush=True)
    out = {}
    for v, x in res.items():
        med = statistics.median(x)
        per_step = float(valid[v]) / rounds
        out[v] = {"median_ms": round(med, 4), "min_ms": round(min(x), 4), "all": [round(t, 4) for t in x],
                  "valid_targets_per_step": round(per_step, 1),
                  "valid_targets_per_s": round(per_step / (med * 1e-3))}
    tokens = cfg.batch_size * cfg.block_size
    fill = {"pairs": out["pairs"]["valid_targets_per_step"] / tokens, "packed": runs["packed"].sampler.fill}
    print(json.dumps({"config": "c2", "steps_per_round": steps, "rounds": rounds, "n_pairs": n_pairs, "variants": out,
                      "fill_packed_rows": round(fill["packed"], 4),
                      "valid_share_one_pair_per_row": round(fill["pairs"], 4),
                      "packed_rows": len(runs["packed"].sampler.rows["train"]),
                      "mask_cost_ms_packed_minus_dense": round(out["packed"]["median_ms"] - out["dense"]["median_ms"], 4),
                      "valid_targets_per_s_ratio": round(out["packed"]["valid_targets_per_s"] / out["pairs"]["valid_targets_per_s"], 3)}))


if __name__ == "__main__":
    main()
