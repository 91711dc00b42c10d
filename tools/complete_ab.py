"""A/B of complete() against generate() on the C5 workload (256 rows x 500 new tokens from one-token
prompts, the reference-trained C1 weights, fp32, greedy), interleaved in one process after capture
and warm-up: generate(); complete() with equal prompts at poll_every = 32 (the default), 0 (never)
and 1 (a host round trip per step: the poll's cost per poll is (t_1 - t_0) / steps); complete() with
return_logprobs.  Prints each round's times, then one JSON line with the medians.

    python tools/complete_ab.py [--rounds 6] [--json out.json]
    python tools/complete_ab.py --only generate      # one variant: a library built from another tree
                                                     # (CHARPT_LIB) has no cg_decode_emit
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--new", type=int, default=500)
    ap.add_argument("--only", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from safetensors.torch import load_file
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda:0")
    m = BigramLanguageModel(GPTConfig(dtype="fp32"))
    m.load_state_dict(load_file(os.path.join(ROOT, "tests", "golden", "model_c1_trained.safetensors")), strict=False)
    m = m.to(dev).eval()
    idx = torch.zeros((a.rows, 1), dtype=torch.long, device=dev)
    prompts = (idx, torch.ones(a.rows, dtype=torch.int64))
    variants = {
        "generate": lambda: m.generate(idx, a.new, greedy=True),
        "complete_poll32": lambda: m.complete(prompts, a.new, greedy=True).tokens,
        "complete_poll0": lambda: m.complete(prompts, a.new, greedy=True, poll_every=0).tokens,
        "complete_poll1": lambda: m.complete(prompts, a.new, greedy=True, poll_every=1).tokens,
        "complete_logprobs": lambda: m.complete(prompts, a.new, greedy=True, return_logprobs=True).tokens,
    }
    if a.only:
        variants = {a.only: variants[a.only]}

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    with torch.no_grad():
        sums = set()
        for fn in variants.values():          # capture + warm-up, every path
            run(fn)
            sums.add(int(run(fn)[1].sum()))
        assert len(sums) == 1, f"the variants disagree on the greedy stream: {sums}"
        times = {k: [] for k in variants}
        for r in range(a.rounds):
            for name, fn in variants.items():
                dt, out = run(fn)
                times[name].append(dt)
                print(f"round {r} {name}: {dt:.4f} s, {a.rows * a.new / dt:.0f} tokens/s, checksum {int(out.sum())}", flush=True)
    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"median_s": round(med, 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5),
                     "tokens_per_s": round(a.rows * a.new / med, 1)}
    if "complete_poll1" in res and "complete_poll0" in res:
        res["poll_cost_us_per_poll"] = round((res["complete_poll1"]["median_s"] - res["complete_poll0"]["median_s"]) / a.new * 1e6, 2)
    res["workload"] = f"{a.rows} rows x {a.new} new tokens, C1 trained weights, fp32 greedy, {a.rounds} interleaved rounds"
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
