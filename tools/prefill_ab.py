"""A/B of the one-pass prompt prefill against the per-token prefill steps on the C5-shaped model (256 rows,
the reference-trained C1 weights, fp32, greedy): complete() with max_new_tokens = 1 at prompt lengths 2,
4, 8, 16, 64, 128 and 255, and score() of 255-token rows.  Each workload has two engines, one with the pass
(prefill_min = 1) and one without; all are captured and warmed up first, then timed in interleaved rounds
in one process.  A timing is a host clock around `reps` calls ending in a device synchronise (reps chosen
per workload so that a window is about 0.2 s of the steps arm; both arms use the same reps), reported per
call.  Every round checks that both arms return the same tokens / log-probs, bit for bit.

Prints each round's times, a table of medians and spreads (max - min), and one JSON line.  The pass "wins"
at a length when the steps' median exceeds its median by more than the two spreads together; the smallest
such length L gives decode.PREFILL_MIN = L - 1 positions.

    python tools/prefill_ab.py [--rounds 7] [--rows 256] [--json out.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (2, 4, 8, 16, 64, 128, 255)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of the steps arm per timing window")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from safetensors.torch import load_file
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    from replicatinggpt_amd.decode import DecodeEngine
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda:0")
    m = BigramLanguageModel(GPTConfig(dtype="fp32"))
    m.load_state_dict(load_file(os.path.join(ROOT, "tests", "golden", "model_c1_trained.safetensors")), strict=False)
    m = m.to(dev).eval()
    B, V = a.rows, m.config.vocab_size
    text = torch.randint(0, V, (B, 255), generator=torch.Generator().manual_seed(1337)).to(dev)

    # workload -> {arm: callable returning the tensor both arms must agree on}
    work = {}
    for Lp in LENGTHS:
        idx, lens = text[:, :Lp].contiguous(), torch.full((B,), Lp, dtype=torch.int64)
        arms = {}
        for arm, on in (("pass", True), ("steps", False)):
            eng = DecodeEngine(m, B, Lp + 1, ragged=True, prefill_pass=on, prefill_min=1)
            arms[arm] = (eng, lambda eng=eng, idx=idx, lens=lens: eng.complete(idx, lens, 1, mode=0)[0])
        work[f"complete_L{Lp}"] = arms
    lens = torch.full((B,), 255, dtype=torch.int64)
    arms = {}
    for arm, on in (("pass", True), ("steps", False)):
        eng = DecodeEngine(m, B, 255, ragged=True, logprobs=True, prefill_pass=on, prefill_min=1)
        arms[arm] = (eng, lambda eng=eng: eng.complete(text, lens, 0, mode=0)[2])
    work["score_L255"] = arms

    def run(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, out

    reps, times = {}, {}
    with torch.no_grad():
        for name, arms in work.items():            # capture + warm-up of every engine, then size the window
            for eng, fn in arms.values():
                run(fn, 1)
                run(fn, 2)
            reps[name] = max(1, min(200, math.ceil(a.window / run(arms["steps"][1], 2)[0])))
            times[name] = {arm: [] for arm in arms}
        for r in range(a.rounds):
            for name, arms in work.items():
                outs = {}
                for arm, (eng, fn) in arms.items():
                    dt, outs[arm] = run(fn, reps[name])
                    times[name][arm].append(dt)
                    print(f"round {r} {name} {arm}: {dt * 1e3:.3f} ms per call ({reps[name]} calls), "
                          f"stats {eng.prefill_stats}", flush=True)
                same = torch.equal(outs["pass"].view(torch.int32) if outs["pass"].dtype == torch.float32 else outs["pass"],
                                   outs["steps"].view(torch.int32) if outs["steps"].dtype == torch.float32 else outs["steps"])
                assert same, f"{name}: the two arms disagree"
    res = {"workload": f"{B} rows, C1 trained weights, fp32 greedy, {a.rounds} interleaved rounds; ms per call"}
    print(f"\n{'workload':>14} {'pass med':>9} {'spread':>7} {'steps med':>10} {'spread':>7} {'steps/pass':>10}  pass wins")
    first = None
    for name, t in times.items():
        med = {arm: statistics.median(ts) * 1e3 for arm, ts in t.items()}
        spr = {arm: (max(ts) - min(ts)) * 1e3 for arm, ts in t.items()}
        wins = med["steps"] - med["pass"] > spr["pass"] + spr["steps"]
        if wins and first is None and name.startswith("complete_L"):
            first = int(name[len("complete_L"):])
        res[name] = {"pass_median_ms": round(med["pass"], 4), "pass_spread_ms": round(spr["pass"], 4),
                     "steps_median_ms": round(med["steps"], 4), "steps_spread_ms": round(spr["steps"], 4),
                     "steps_over_pass": round(med["steps"] / med["pass"], 3), "pass_wins": bool(wins), "reps": reps[name]}
        print(f"{name:>14} {med['pass']:9.3f} {spr['pass']:7.3f} {med['steps']:10.3f} {spr['steps']:7.3f} "
              f"{med['steps'] / med['pass']:10.2f}  {'yes' if wins else 'no'}")
    res["smallest_winning_length"] = first
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
