"""Sample text from a saved ``model.pth`` on the decode engine::

    python -m replicatinggpt_amd.sample --model model.pth --prompt "ROMEO:" --temperature 0.8 --top-k 40
    python -m replicatinggpt_amd.sample --model model.pth --num-samples 4 --top-p 0.95 --seed 7

``--model`` is a state dict as GPT1.py:239-241 (or ``python -m replicatinggpt_amd.gpt1``) writes it,
loaded with ``checkpoint.load_model`` into the ``--preset`` shape.  The tokenizer is rebuilt from the
corpus (``--input``), as the reference builds it.  ``--prompt`` is encoded with it; an empty prompt
is the reference's ``zeros((1, 1))`` context (GPT1.py:235).  ``--num-samples`` repeats the prompt
over that many rows of one batched ``generate`` call: the rows differ because the engine's Philox
draw is keyed by row.
"""
import argparse

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
    ap.add_argument("--prompt", default="", help="text to continue; empty: the reference's zeros((1, 1)) context")
    ap.add_argument("--num-samples", type=int, default=1, help="rows of the batched generate call")
    ap.add_argument("--max-new-tokens", type=int, default=500)
    add_sampling_args(ap)
    ap.add_argument("--greedy", action="store_true", help="argmax instead of sampling")
    ap.add_argument("--seed", type=int, default=1337, help="seed of the generator the draw's seed is taken from")
    a = ap.parse_args(argv)
    if a.num_samples < 1:
        ap.error("--num-samples must be >= 1")
    if a.max_new_tokens < 0:
        ap.error("--max-new-tokens must be >= 0")
    return a


def encode_prompt(tok, prompt, num_samples=1):
    """[num_samples, len] int64 context: the prompt's characters, or one 0 token for an empty prompt
    (GPT1.py:235).  A character the corpus does not contain raises a ValueError that names it."""
    unknown = sorted(set(c for c in prompt if c not in tok.stoi))
    if unknown:
        raise ValueError(f"--prompt: character(s) {unknown!r} are not in the tokenizer's vocabulary "
                         f"({tok.vocab_size} characters of the --input corpus)")
    ids = tok.encode(prompt) if prompt else [0]
    return torch.tensor([ids] * num_samples, dtype=torch.long)


def load_tokenizer(path):
    with open(path, "r", encoding="utf-8") as f:
        return CharTokenizer(f.read())


def main(argv=None):
    a = parse_args(argv)
    tok = load_tokenizer(a.input)
    context = encode_prompt(tok, a.prompt, a.num_samples)
    if not torch.cuda.is_available():
        raise SystemExit("charpt: sampling runs the decode engine on an AMD GPU (HIP); there is no CPU version")
    cfg = PRESETS[a.preset].with_(dtype=a.dtype, vocab_size=tok.vocab_size)
    model = BigramLanguageModel(cfg)
    checkpoint.load_model(model, a.model)
    model = model.to("cuda").eval()
    gen = torch.Generator().manual_seed(a.seed)
    with torch.no_grad():
        out = model.generate(context.to("cuda"), a.max_new_tokens, greedy=a.greedy, generator=gen,
                             temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    for i, row in enumerate(out.tolist()):
        if a.num_samples > 1:
            print(f"--- sample {i} ---")
        print(tok.decode(row))
    return out


if __name__ == "__main__":
    main()
