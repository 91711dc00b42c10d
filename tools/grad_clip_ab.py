"""What the training recipe (device learning rate, global-norm clipping) costs on one GPU.

  steps <c2|c4> [rounds] [steps]
      Same-process interleaved A/B (the manner of tools/step_ab.py) of the one-graph training step
      with three optimizers: default (early updates beside the backward's GEMMs, by-value lr),
      dynamic (AdamW(dynamic_lr=True): one cg_adamw_dyn launch, no early updates) and clip
      (AdamW(max_grad_norm=1.0): cg_grad_norm + cg_adamw_dyn).  Median / min ms per step.

  trees <c2|c4> <tree A> <tree B> [reps] [rounds] [steps]
      Two checkouts (each built) with default arguments: ``tools/step_ab.py <cfg> single`` run in a
      fresh process per tree, alternating A B A B ..., ``reps`` times each.  Reports every process's
      median ms per step, so the A-vs-A spread stands beside the A-vs-B difference.

  norm [rounds]
      cg_grad_norm alone at the C2 and C4 parameter counts: HIP events around a hipGraph of 20
      back-to-back calls, GB/s of the 4 B/param read against the HBM peak (8 TB/s), with cg_adamw's
      time at the same size for scale.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_PARAMS = {"c2": 10788992, "c4": 85997568}   # flat-buffer lengths (tools/ab_interleave.py adamw_work)
HBM_PEAK_GBS = 8000.0


def steps_main(cfgname, rounds, steps):
    import torch
    from replicatinggpt_amd import AdamW, BigramLanguageModel, PRESETS
    from replicatinggpt_amd.data import BatchSampler, TokenStream
    from replicatinggpt_amd.engine import TrainStep
    dev = torch.device("cuda")
    kinds = {"default": {}, "dynamic": {"dynamic_lr": True}, "clip": {"max_grad_norm": 1.0}}
    runs = {}
    for name, kw in kinds.items():
        cfg = PRESETS[cfgname].with_(dtype="bf16")
        torch.manual_seed(cfg.seed)
        model = BigramLanguageModel(cfg).to(dev)
        opt = AdamW(model.parameters(), lr=cfg.learning_rate, **kw).attach(model)
        sampler = BatchSampler(TokenStream.synthetic(device=dev), cfg.block_size, cfg.batch_size,
                               generator=torch.Generator().manual_seed(cfg.seed))
        sched = (lambda it, lr=cfg.learning_rate: lr) if kw else None   # set_lr every step, as a recipe would
        runs[name] = TrainStep(model, opt, sampler, None, lr_schedule=sched)
        runs[name].capture()
    for st in runs.values():
        for _ in range(10):
            st.step()
    torch.cuda.synchronize()
    res = {v: [] for v in runs}
    for r in range(rounds):
        for v, st in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                st.step()
            torch.cuda.synchronize()
            res[v].append((time.perf_counter() - t0) / steps * 1e3)
        print(f"round {r}: " + "  ".join(f"{v} {res[v][-1]:.4f}" for v in runs), flush=True)
    coef = float(runs["clip"].opt.clip_coef)
    out = {v: {"median_ms": round(statistics.median(x), 4), "min_ms": round(min(x), 4),
               "all": [round(t, 4) for t in x]} for v, x in res.items()}
    print(json.dumps({"config": cfgname, "steps_per_round": steps, "rounds": rounds, "variants": out,
                      "last_clip_coef": coef}))


def trees_main(cfgname, tree_a, tree_b, reps, rounds, steps):
    res = {"A": [], "B": []}
    for r in range(reps):
        for tag, tree in (("A", tree_a), ("B", tree_b)):
            env = {k: v for k, v in os.environ.items() if k != "CHARPT_LIB"}
            p = subprocess.run([sys.executable, os.path.join(tree, "tools", "step_ab.py"), cfgname, "single", str(rounds),
                                str(steps)], cwd=tree, env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                raise SystemExit(f"{tree}: step_ab.py exited {p.returncode}")
            v = json.loads(p.stdout.strip().splitlines()[-1])["variants"]["single"]
            res[tag].append(v["median_ms"])
            print(f"rep {r} {tag} ({tree}): median {v['median_ms']:.4f} ms  min {v['min_ms']:.4f} ms  {v['all']}",
                  flush=True)
    med = {t: statistics.median(x) for t, x in res.items()}
    print(json.dumps({"config": cfgname, "A": tree_a, "B": tree_b, "process_medians_ms": res,
                      "median_of_medians_ms": med, "A_spread_ms": round(max(res["A"]) - min(res["A"]), 4),
                      "B_spread_ms": round(max(res["B"]) - min(res["B"]), 4),
                      "B_minus_A_ms": round(med["B"] - med["A"], 4)}))


def norm_main(rounds):
    import torch
    from replicatinggpt_amd import ops
    from tools.attn_bench import _time
    dev = torch.device("cuda")
    for cfgname, n in N_PARAMS.items():
        g, p, m, v = (torch.randn(n, device=dev) * 0.01 for _ in range(4))
        v.abs_()
        p16 = torch.empty(n, dtype=torch.bfloat16, device=dev)
        step = torch.ones(1, dtype=torch.int64, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        ws = torch.empty(ops.grad_norm_workspace(n) // 8, dtype=torch.float64, device=dev)
        lr = torch.tensor([1e-3], dtype=torch.float64, device=dev)
        work = {"grad_norm": lambda: ops.grad_norm(g, 1.0, out, ws),
                "adamw": lambda: ops.adamw(p, g, m, v, p16, 1e-3, 0.9, 0.999, 1e-8, 0.01, step),
                "adamw_dyn+coef": lambda: ops.adamw_dyn(p, g, m, v, p16, lr, out[1:2], 0.9, 0.999, 1e-8, 0.01, step)}
        res = {k: [] for k in work}
        for _ in range(rounds):
            for k, fn in work.items():
                res[k].append(_time(fn))
        want = float(g.double().norm())
        print(f"{cfgname} n={n}: norm {float(out[0]):.6f} (float64 {want:.6f})")
        for k, x in res.items():
            us = statistics.median(x)
            byts = n * (4 if k == "grad_norm" else 30)
            print(f"  {k:15s} median {us:8.1f} us  min {min(x):8.1f} us  {byts / us / 1e3:7.0f} GB/s "
                  f"({100 * byts / us / 1e3 / HBM_PEAK_GBS:4.1f} % of {HBM_PEAK_GBS:.0f} GB/s)  "
                  f"[{' '.join(f'{t:.1f}' for t in x)}]", flush=True)


def main():
    a = sys.argv[1:]
    if not a or a[0] not in ("steps", "trees", "norm"):
        raise SystemExit(__doc__)
    if a[0] == "steps":
        steps_main(a[1], int(a[2]) if len(a) > 2 else 5, int(a[3]) if len(a) > 3 else 50)
    elif a[0] == "trees":
        trees_main(a[1], os.path.abspath(a[2]), os.path.abspath(a[3]), int(a[4]) if len(a) > 4 else 3,
                   int(a[5]) if len(a) > 5 else 3, int(a[6]) if len(a) > 6 else 50)
    else:
        norm_main(int(a[1]) if len(a) > 1 else 7)


if __name__ == "__main__":
    main()
