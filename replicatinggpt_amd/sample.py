"""Sample text from a saved ``model.pth`` on the decode engine::

    python -m replicatinggpt_amd.sample --model model.pth --prompt "ROMEO:" --temperature 0.8 --top-k 40
    python -m replicatinggpt_amd.sample --model model.pth --num-samples 4 --top-p 0.95 --seed 7
    python -m replicatinggpt_amd.sample --model model.pth --prompt "ROMEO:" --prompt "First Citizen:" --stop "." --logprobs
    python -m replicatinggpt_amd.sample --model model.pth --prompt-file prompts.txt --greedy

``--model`` is a state dict as GPT1.py:239-241 (or ``python -m replicatinggpt_amd.gpt1``) writes it,
loaded with ``checkpoint.load_model`` into the ``--preset`` shape.  The tokenizer is rebuilt from the
corpus (``--input``), as the reference builds it.  ``--prompt`` is encoded with it; an empty prompt
is the reference's ``zeros((1, 1))`` context (GPT1.py:235).  ``--num-samples`` repeats the prompt
over that many rows of one batched ``generate`` call: the rows differ because the engine's Philox
draw is keyed by row.

``--prompt`` given several times, ``--prompt-file`` (one prompt per line), ``--stop`` (each of its
characters ends a row once generated) and ``--logprobs`` run ``BigramLanguageModel.complete``
instead: prompts of different lengths in one batch, each row printed up to its own end.  One
``--prompt`` and none of these flags is the ``generate`` call above, output unchanged.
"""
import argparse
import math

import torch

from . import checkpoint
from .config import PRESETS
from .data import DEFAULT_INPUT, CharTokenizer
from .model import BigramLanguageModel
from .sampling import add_sampling_args


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="sample from a trained charpt / GPT1.py model (MI355X)")
    ap.add_argument("--model", required=True, help="model.pth: the state dict GPT1.py:239-241 saves")
    ap.add_argument("--preset", default="c1", choices=sorted(PRESETS), help="model shape the file was trained with")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"], help="GEMM operand / activation dtype")
    ap.add_argument("--input", default=DEFAULT_INPUT, help="corpus the character vocabulary is built from")
    ap.add_argument("--prompt", action="append", default=None,
                    help="text to continue; empty: the reference's zeros((1, 1)) context; repeat for several prompts")
    ap.add_argument("--prompt-file", default=None, help="a file with one prompt per line (added to --prompt's)")
    ap.add_argument("--stop", default="", help="characters that end a completion once generated (kept in the output)")
    ap.add_argument("--logprobs", action="store_true",
                    help="print each completion's mean log-probability and bits per character")
    ap.add_argument("--num-samples", type=int, default=1, help="rows of the batched call per prompt")
    ap.add_argument("--max-new-tokens", type=int, default=500)
    add_sampling_args(ap)
    ap.add_argument("--greedy", action="store_true", help="argmax instead of sampling")
    ap.add_argument("--seed", type=int, default=1337, help="seed of the generator the draw's seed is taken from")
    a = ap.parse_args(argv)
    if a.num_samples < 1:
        ap.error("--num-samples must be >= 1")
    if a.max_new_tokens < 0:
        ap.error("--max-new-tokens must be >= 0")
    a.prompts = list(a.prompt or [])
    if a.prompt_file is not None:
        a.prompts += read_prompt_file(a.prompt_file)
    if not a.prompts:
        a.prompts = [""]
    # one prompt and no completion flag: the generate() call, as before
    a.ragged = len(a.prompts) > 1 or a.prompt_file is not None or bool(a.stop) or a.logprobs
    a.prompt = a.prompts[0] if len(a.prompts) == 1 else a.prompts
    return a


def read_prompt_file(path):
    """One prompt per line (the line break is not part of it); a trailing empty line is no prompt."""
    with open(path, "r", encoding="utf-8") as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return lines


def _check_chars(tok, text, flag):
    unknown = sorted(set(c for c in text if c not in tok.stoi))
    if unknown:
        raise ValueError(f"{flag}: character(s) {unknown!r} are not in the tokenizer's vocabulary "
                         f"({tok.vocab_size} characters of the --input corpus)")


def encode_prompt(tok, prompt, num_samples=1):
    """[num_samples, len] int64 context: the prompt's characters, or one 0 token for an empty prompt
    (GPT1.py:235).  A character the corpus does not contain raises a ValueError that names it."""
    _check_chars(tok, prompt, "--prompt")
    ids = tok.encode(prompt) if prompt else [0]
    return torch.tensor([ids] * num_samples, dtype=torch.long)


def encode_prompts(tok, prompts, num_samples=1):
    """complete()'s prompt list: every prompt's rows (encode_prompt), num_samples of each in a row."""
    return [row for p in prompts for row in encode_prompt(tok, p, num_samples)]


def encode_stop(tok, stop):
    """The token ids of --stop's characters; an unknown character raises encode_prompt's error."""
    _check_chars(tok, stop, "--stop")
    return sorted(set(tok.encode(stop))) if stop else []


def load_tokenizer(path):
    with open(path, "r", encoding="utf-8") as f:
        return CharTokenizer(f.read())


def logprob_line(logprobs, prompt_len, length):
    """--logprobs' line for one row: over the generated tokens, or over the prompt (from its second
    token) when nothing was generated -- the row was scored."""
    lo = prompt_len if length > prompt_len else 1
    n = length - lo
    if n <= 0:
        return "[no token to score]"
    lp = float(logprobs[lo:length].double().sum())
    what = "new" if length > prompt_len else "prompt"
    return f"[{n} {what} tokens: mean log-prob {lp / n:.4f}, {-lp / n / math.log(2):.4f} bits per character]"


def main(argv=None):
    a = parse_args(argv)
    tok = load_tokenizer(a.input)
    if a.ragged:
        rows = encode_prompts(tok, a.prompts, a.num_samples)
        stop = encode_stop(tok, a.stop)
    else:
        context = encode_prompt(tok, a.prompt, a.num_samples)
    if not torch.cuda.is_available():
        raise SystemExit("charpt: sampling runs the decode engine on an AMD GPU (HIP); there is no CPU version")
    cfg = PRESETS[a.preset].with_(dtype=a.dtype, vocab_size=tok.vocab_size)
    model = BigramLanguageModel(cfg)
    checkpoint.load_model(model, a.model)
    model = model.to("cuda").eval()
    gen = torch.Generator().manual_seed(a.seed)
    if not a.ragged:
        with torch.no_grad():
            out = model.generate(context.to("cuda"), a.max_new_tokens, greedy=a.greedy, generator=gen,
                                 temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
        for i, row in enumerate(out.tolist()):
            if a.num_samples > 1:
                print(f"--- sample {i} ---")
            print(tok.decode(row))
        return out
    with torch.no_grad():
        out = model.complete(rows, a.max_new_tokens, stop_tokens=stop, return_logprobs=a.logprobs, greedy=a.greedy,
                             generator=gen, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    lengths = out.lengths.tolist()
    logprobs = out.logprobs.cpu() if a.logprobs else None
    for i, row in enumerate(out.tokens.tolist()):
        if len(rows) > 1:
            print(f"--- sample {i} ---")
        print(tok.decode(row[:lengths[i]]))     # the row's own tokens, not the pad after them
        if a.logprobs:
            print(logprob_line(logprobs[i], rows[i].numel(), lengths[i]))
    return out


if __name__ == "__main__":
    main()
