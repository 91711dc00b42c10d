"""A/B of generate() on the C5 workload (256 rows x 500 new tokens, the reference-trained C1 weights,
fp32): the plain sampler (neutral settings: cg_decode_sample) against the filtered one
(temperature 0.8, top_k 40, top_p 0.95: cg_decode_sample_filtered), interleaved in one process
after warm-up.  Prints each round's times, then one JSON line with the medians and the ratio
filtered / neutral in tokens/s.

    python tools/gen_sample_ab.py [--rounds 8] [--json out.json]
    python tools/gen_sample_ab.py --trace-only     # two filtered calls: run under a kernel trace
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
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--new", type=int, default=500)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace-only", action="store_true")
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
    gen = torch.Generator().manual_seed(1337)
    modes = {"neutral": {}, "filtered": dict(temperature=0.8, top_k=40, top_p=0.95)}
    if a.trace_only:
        modes.pop("neutral")

    def run(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(idx, a.new, generator=gen, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    with torch.no_grad():
        for kw in modes.values():          # capture + warm-up, both paths
            run(kw)
            run(kw)
        times = {k: [] for k in modes}
        for r in range(1 if a.trace_only else a.rounds):
            for name, kw in modes.items():
                dt, out = run(kw)
                times[name].append(dt)
                print(f"round {r} {name}: {dt:.4f} s, {a.rows * a.new / dt:.0f} tokens/s, checksum {int(out.sum())}", flush=True)
    if a.trace_only:
        return
    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"median_s": round(med, 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5),
                     "tokens_per_s": round(a.rows * a.new / med, 1)}
    res["ratio_filtered_over_neutral"] = round(res["filtered"]["tokens_per_s"] / res["neutral"]["tokens_per_s"], 4)
    res["workload"] = f"{a.rows} rows x {a.new} new tokens, C1 trained weights, fp32, {a.rounds} interleaved rounds"
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
