"""Host side of ``BigramLanguageModel.complete`` / ``score``: the result tuple, prompt packing and
argument validation.  Everything here is plain CPU torch; the work runs in the ragged mode of
``decode.DecodeEngine`` and in ``cg_decode_emit`` (include/charpt.h holds the per-row contract).
"""
from collections import namedtuple

import torch

# tokens [B, max(lens) + max_new_tokens] int64; lengths [B] int64 (the kernel's end[]); logprobs
# [B, same width] fp32 or None (column 0 and pad columns 0); steps: head steps actually run
Completion = namedtuple("Completion", ["tokens", "lengths", "logprobs", "steps"])


def pack_prompts(prompts):
    """``prompts``: a list of 1-D int64 tensors (each of length >= 1), or a pair ``(idx[B, Lmax],
    lens[B])``.  Returns CPU tensors ``(idx[B, max(lens)], lens[B])``, int64, rows zero-filled past
    their length (those columns are never read)."""
    if isinstance(prompts, tuple) and len(prompts) == 2 and torch.is_tensor(prompts[0]) and prompts[0].dim() == 2:
        idx, lens = prompts
        lens = torch.as_tensor(lens, dtype=torch.int64).reshape(-1).cpu()
        if idx.dtype != torch.int64:
            raise ValueError(f"prompts: idx must be int64, got {idx.dtype}")
        if lens.numel() != idx.shape[0]:
            raise ValueError(f"prompts: {idx.shape[0]} rows in idx but {lens.numel()} lengths")
        if lens.numel() == 0:
            raise ValueError("prompts: no prompt given")
        if int(lens.min()) < 1 or int(lens.max()) > idx.shape[1]:
            raise ValueError(f"prompts: every length must be in [1, {idx.shape[1]}] (idx's width), got {lens.tolist()}")
        return idx[:, :int(lens.max())].cpu().contiguous(), lens
    rows = list(prompts)
    if not rows:
        raise ValueError("prompts: no prompt given")
    for b, r in enumerate(rows):
        if not torch.is_tensor(r) or r.dim() != 1 or r.dtype != torch.int64:
            raise ValueError(f"prompts[{b}]: expected a 1-D int64 tensor")
        if r.numel() < 1:
            raise ValueError(f"prompts[{b}] is empty: every prompt needs at least one token")
    lens = torch.tensor([r.numel() for r in rows], dtype=torch.int64)
    idx = torch.zeros((len(rows), int(lens.max())), dtype=torch.int64)
    for b, r in enumerate(rows):
        idx[b, :r.numel()] = r.cpu()
    return idx, lens


def stop_words(stop_tokens, vocab_size):
    """``cg_decode_emit``'s stop_bits as a CPU int64 tensor of ceil(V / 64) words (bit v of the set:
    word v // 64, bit v % 64), or None for an empty set.  A token outside [0, V) is a ValueError."""
    words = [0] * ((vocab_size + 63) // 64)
    toks = [int(t) for t in stop_tokens]
    for t in toks:
        if not 0 <= t < vocab_size:
            raise ValueError(f"stop_tokens: token {t} is outside the vocabulary [0, {vocab_size})")
        words[t >> 6] |= 1 << (t & 63)
    if not toks:
        return None
    return torch.tensor([w - (1 << 64) if w >> 63 else w for w in words], dtype=torch.int64)   # two's complement


def check_complete_args(idx, lens, max_new_tokens, pad_token, vocab_size, poll_every):
    if int(max_new_tokens) != max_new_tokens or max_new_tokens < 0:
        raise ValueError(f"max_new_tokens must be an integer >= 0, got {max_new_tokens!r}")
    if int(poll_every) != poll_every or poll_every < 0:
        raise ValueError(f"poll_every must be an integer >= 0 (0: never poll), got {poll_every!r}")
    # ended rows keep running in lock step on pad tokens, so the pad is embedded like any other token
    if int(pad_token) != pad_token or not 0 <= pad_token < vocab_size:
        raise ValueError(f"pad_token must be a token of the vocabulary [0, {vocab_size}), got {pad_token!r}")
    cols = torch.arange(idx.shape[1])[None, :]
    tok = idx[cols < lens[:, None]]
    if int(tok.min()) < 0 or int(tok.max()) >= vocab_size:
        raise ValueError(f"prompts: token outside the vocabulary [0, {vocab_size})")
