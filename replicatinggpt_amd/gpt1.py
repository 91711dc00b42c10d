"""GPT1.py's script on charpt (GPT1.py:1-241 with encoder='base').

Hyper-parameters (GPT1.py:8-23), tokenizer and split (:25-70), get_batch (:75-83), estimate_loss
(:85-98), the training loop (:221-233), the final sample (:235-236) and the model.pth save
(:239-241), printing the reference's lines::

    python -m replicatinggpt_amd.gpt1                          # as shipped: C1 shape, lr 5e-1
    python -m replicatinggpt_amd.gpt1 --lr 2e-4 --max-iters 500 --dtype bf16
    python -m replicatinggpt_amd.gpt1 --preset c4 --dtype bf16 --lr 6e-4 --grad-clip 1.0 \
        --warmup-iters 100 --lr-decay-iters 5000 --min-lr 6e-5   # a recipe GPT1.py does not have

Deliberate differences from GPT1.py:

* the training step replays a hipGraph (engine.TrainStep).  The warm-up steps of its capture are
  rolled back (weights, AdamW moments and step, dropout counter, CPU generator), so iteration 0
  starts from exactly the state the reference starts from;
* estimate_loss keeps its per-batch losses on the device and reads them once per split (GPT1.py:94
  synchronises on ``loss.item()`` once per batch); each evaluation forward replays a hipGraph
  (engine.Evaluator).  The mean is taken on the host over the same float32 values, as at :95;
* ``--grad-clip`` (global-norm clipping) and ``--warmup-iters`` / ``--lr-decay-iters`` / ``--min-lr``
  (linear warm-up, cosine decay: schedule.warmup_cosine) put the optimizer in its dynamic mode
  (optim.AdamW); with none of them given the driver builds exactly the objects it built before.  A
  resumed run continues the schedule from the checkpoint's iteration;
* ``--pairs FILE`` fine-tunes on (prompt, completion) pairs -- JSON lines ``{"prompt": ..., "completion":
  ...}`` tokenised with the ``--input`` vocabulary -- with the loss on the completions only
  (data.PairSampler, the masked cross entropy of DESIGN.md §4); ``--init-from model.pth`` loads a state
  dict first, since fine-tuning starts from a trained model.  Without them nothing changes;
  ``--pack`` (with ``--pairs`` only) puts several pairs in each row (data.PackedPairSampler: attention
  masked between them, positions restarting at each) and prints the share of non-pad positions once;
* dropout masks come from charpt's Philox stream, so with Dropout > 0 the loss
  curve matches the reference's within tolerance, not bit for bit (tests/test_gpu_train.py).
"""
import argparse
import json

import torch

from . import checkpoint
from .config import PRESETS
from .data import DEFAULT_INPUT, BatchSampler, PackedPairSampler, PairSampler, TokenStream
from .engine import Evaluator, TrainStep
from .model import BigramLanguageModel
from .optim import AdamW
from .schedule import warmup_cosine
from .sampling import add_sampling_args


@torch.no_grad()
def estimate_loss(model, sampler, eval_iters, evaluator=None):
    """GPT1.py:85-98: mean loss over ``eval_iters`` batches of each split, in eval mode."""
    out = {}
    model.eval()                                                              # :88
    dev = model.flat.master.device
    for split in ("train", "val"):                                            # :89
        losses = torch.zeros(eval_iters, dtype=torch.float32, device=dev)     # :90
        for k in range(eval_iters):                                           # :91
            if evaluator is not None:
                losses[k] = evaluator.loss(split)                             # :92-93, graph replay
            else:
                X, Y, *seg = sampler.get_batch(split)                         # :92
                ignore = getattr(sampler, "ignore_index", None)               # PairSampler: masked targets
                kw = {} if ignore is None else {"ignore_index": ignore}
                if seg:                                                       # PackedPairSampler: packed rows
                    kw["seg_start"] = seg[0]
                _, loss = model(X, Y, **kw)                                   # :93
                losses[k] = loss                                              # :94 (no host sync)
        out[split] = losses.cpu().mean()                                      # :95
    model.train()                                                             # :96
    return out


def read_pairs(path, tok):
    """JSON lines {"prompt": str, "completion": str} -> [(prompt_tokens, completion_tokens)] in
    ``tok``'s vocabulary; a character outside it is an error naming the line."""
    pairs = []
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                rec = json.loads(line)
                prompt, completion = rec["prompt"], rec["completion"]
            except (ValueError, KeyError, TypeError) as e:
                raise SystemExit(f"{path}:{no}: expected a JSON object with \"prompt\" and \"completion\": {e!r}")
            for side, text in (("prompt", prompt), ("completion", completion)):
                bad = sorted(set(c for c in text if c not in tok.stoi))
                if bad:
                    raise SystemExit(f"{path}:{no}: {side} has characters outside the --input vocabulary: {bad!r}")
            pairs.append((tok.encode(prompt), tok.encode(completion)))
    return pairs


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="GPT1.py on charpt (MI355X)")
    ap.add_argument("--preset", default="c1", choices=sorted(PRESETS), help="model shape (c1: GPT1.py as shipped)")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"], help="GEMM operand / activation dtype")
    ap.add_argument("--input", default=DEFAULT_INPUT)
    ap.add_argument("--batch-size", type=int)
    ap.add_argument("--max-iters", type=int)
    ap.add_argument("--eval-interval", type=int)
    ap.add_argument("--eval-iters", type=int)
    ap.add_argument("--dropout", type=float)
    ap.add_argument("--lr", type=float, help="optimizer lr (GPT1.py:218 uses 5e-1; its learning_rate = 2e-4 is unused)")
    ap.add_argument("--grad-clip", type=float, help="clip the global gradient norm to this (torch clip_grad_norm_)")
    ap.add_argument("--warmup-iters", type=int, help="linear learning-rate warm-up over this many iterations")
    ap.add_argument("--lr-decay-iters", type=int, help="cosine decay to --min-lr at this iteration (default: max-iters)")
    ap.add_argument("--min-lr", type=float, help="the learning rate after the decay (default 0)")
    ap.add_argument("--max-new-tokens", type=int, default=500)
    add_sampling_args(ap)   # --temperature / --top-k / --top-p of the final sample; neutral defaults (GPT1.py:236)
    ap.add_argument("--out", default="model.pth", help="state dict file (GPT1.py:240); '' to skip")
    ap.add_argument("--save-checkpoint", default=None, help="also write a resumable training checkpoint")
    ap.add_argument("--resume", default=None, help="continue from a --save-checkpoint file")
    ap.add_argument("--pairs", default=None, help="fine-tune on JSON lines {\"prompt\", \"completion\"}: loss on the "
                    "completions only")
    ap.add_argument("--pack", action="store_true", help="with --pairs: several pairs per row, attention masked "
                    "between them")
    ap.add_argument("--init-from", default=None, help="load this state dict (a --out file) before training")
    ap.add_argument("--no-graph", action="store_true", help="eager steps instead of hipGraph replay")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    if a.pack and not a.pairs:
        raise SystemExit("charpt: --pack packs (prompt, completion) pairs: it needs --pairs FILE")
    print(torch.cuda.is_available())                                          # GPT1.py:7
    if not torch.cuda.is_available():
        raise SystemExit("charpt: the GPT1 driver needs an AMD GPU (HIP); the hot path has no CPU version")
    device = "cuda"
    over = {k: v for k, v in dict(batch_size=a.batch_size, max_iters=a.max_iters, eval_interval=a.eval_interval,
                                  eval_iters=a.eval_iters, dropout=a.dropout).items() if v is not None}
    cfg = PRESETS[a.preset].with_(dtype=a.dtype, **over)
    torch.manual_seed(cfg.seed)                                               # GPT1.py:10
    tok, stream = TokenStream.from_file(a.input, device=device)               # GPT1.py:25-70
    cfg = cfg.with_(vocab_size=tok.vocab_size)
    model = BigramLanguageModel(cfg)                                          # GPT1.py:215
    m = model.to(device)                                                      # GPT1.py:216
    if a.init_from:
        checkpoint.load_model(m, a.init_from)
    lr = a.lr if a.lr is not None else cfg.optimizer_lr
    schedule = None
    if a.warmup_iters is not None or a.lr_decay_iters is not None or a.min_lr is not None:
        warm = a.warmup_iters or 0
        decay = a.lr_decay_iters if a.lr_decay_iters is not None else max(cfg.max_iters, warm)
        floor = a.min_lr or 0.0

        def schedule(it):
            return warmup_cosine(it, lr, warm, decay, floor)
    if schedule is None and a.grad_clip is None:
        optimizer = AdamW(m.parameters(), lr=lr)                              # GPT1.py:218
    else:
        optimizer = AdamW(m.parameters(), lr=lr, max_grad_norm=a.grad_clip, dynamic_lr=True)
    if a.pairs and a.pack:
        sampler = PackedPairSampler(read_pairs(a.pairs, tok), cfg.block_size, cfg.batch_size, device=device)
        print(f"packed rows: {100 * sampler.fill:.1f}% of the positions hold pair tokens "
              f"({sum(len(r) for r in sampler.rows.values())} rows)")
    elif a.pairs:
        sampler = PairSampler(read_pairs(a.pairs, tok), cfg.block_size, cfg.batch_size, device=device)
    else:
        sampler = BatchSampler(stream, cfg.block_size, cfg.batch_size)       # GPT1.py:75-83
    start = checkpoint.load_checkpoint(a.resume, m, optimizer) if a.resume else 0
    if schedule is None:
        step = TrainStep(m, optimizer, sampler, use_graph=not a.no_graph)
    else:
        step = TrainStep(m, optimizer, sampler, use_graph=not a.no_graph, lr_schedule=schedule)
        step.it = start   # the checkpoint's iteration: the schedule continues where the run stopped
    step.capture(restore=True)
    evaluator = Evaluator(m, sampler, use_graph=not a.no_graph)
    for it in range(start, cfg.max_iters):                                    # GPT1.py:221
        if it % cfg.eval_interval == 0:                                       # GPT1.py:223
            losses = estimate_loss(m, sampler, cfg.eval_iters, evaluator)     # GPT1.py:224
            print(f"step {it} : train loss {losses['train']:.4f}, val loss = {losses['val']:.4f}",  # GPT1.py:225
                  flush=True)
        step.step()                                                           # GPT1.py:227-233
    if a.save_checkpoint:
        checkpoint.save_checkpoint(a.save_checkpoint, m, optimizer, cfg.max_iters)
    context = torch.zeros((1, 1), dtype=torch.long, device=device)            # GPT1.py:235
    print(tok.decode(m.generate(context, max_new_tokens=a.max_new_tokens, temperature=a.temperature, top_k=a.top_k,
                                top_p=a.top_p)[0].tolist()))                  # GPT1.py:236
    if a.out:
        checkpoint.save_model(m, a.out)                                       # GPT1.py:239-241
    return m


if __name__ == "__main__":
    main()
