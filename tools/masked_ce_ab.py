"""Same-process interleaved A/B of the masked cross entropy's cost in the training step on one GPU:
"unmasked" is the bench path (BatchSampler, cg_head_fwd / cg_head_bwd_ex), "masked" the same step with the
sampler announcing ignore_index = -100 (every target stays valid), so the loss runs
cg_head_fwd_masked / cg_head_bwd_masked: the count of valid targets and the normaliser read from the device.
Each variant is its own model + optimizer + captured graph; rounds time each variant's replays in turn
(tools/step_ab.py's method), median / min ms per step.
usage: python tools/masked_ce_ab.py [c2|c4] [rounds] [steps]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from replicatinggpt_amd import AdamW, BigramLanguageModel, PRESETS  # noqa: E402
from replicatinggpt_amd.data import BatchSampler, TokenStream  # noqa: E402
from replicatinggpt_amd.engine import TrainStep  # noqa: E402


class AllValid(BatchSampler):
    """BatchSampler's batches, trained through the masked loss (no target equals ignore_index)."""
    ignore_index = -100


def make(variant, cfgname, dev):
    cfg = PRESETS[cfgname].with_(dtype="bf16")
    torch.manual_seed(cfg.seed)
    model = BigramLanguageModel(cfg).to(dev)
    opt = AdamW(model.parameters(), lr=cfg.learning_rate).attach(model)
    cls = AllValid if variant == "masked" else BatchSampler
    sampler = cls(TokenStream.synthetic(device=dev), cfg.block_size, cfg.batch_size,
                  generator=torch.Generator().manual_seed(cfg.seed))
    step = TrainStep(model, opt, sampler, None)
    step.capture()
    return step


def main():
    cfgname = sys.argv[1] if len(sys.argv) > 1 else "c2"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    dev = torch.device("cuda")
    variants = ("unmasked", "masked")
    runs = {v: make(v, cfgname, dev) for v in variants}
    losses = {}
    for v, st in runs.items():
        for _ in range(10):
            st.step()
        losses[v] = float(st.loss)
    torch.cuda.synchronize()
    res = {v: [] for v in variants}
    for r in range(rounds):
        for v in variants:
            st = runs[v]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                st.step()
            torch.cuda.synchronize()
            res[v].append((time.perf_counter() - t0) / steps * 1e3)
        print(f"round {r}: " + "  ".join(f"{v} {res[v][-1]:.4f}" for v in variants), flush=True)
    out = {v: {"median_ms": round(statistics.median(x), 4), "min_ms": round(min(x), 4),
               "all": [round(t, 4) for t in x]} for v, x in res.items()}
    print(json.dumps({"config": cfgname, "steps_per_round": steps, "rounds": rounds, "variants": out,
                      "loss_after_10_steps": losses, "same_loss_bits": losses["unmasked"] == losses["masked"]}))


if __name__ == "__main__":
    main()
