"""Temperature, top-k and nucleus (top-p) sampling controls for ``BigramLanguageModel.generate``.

The order is HF's: temperature, then top-k, then top-p on the renormalised top-k distribution.

* ``check_sampling`` -- the argument validation ``generate`` runs before it looks at the device.
* ``filter_logits`` -- the filter as one pure torch function, for the literal loop
  (``engine=False`` / dropout on): ``softmax`` and ``torch.multinomial`` follow it as before.
* On the device the decode engine applies the same rule inside its sampling kernel
  (``cg_decode_sample_filtered``, whose header comment in include/charpt.h is the contract both
  follow); the settings live in a three-float device buffer (``sampling_params``).
"""
import math

import torch


def is_neutral(temperature=1.0, top_k=None, top_p=1.0):
    return float(temperature) == 1.0 and not top_k and float(top_p) == 1.0


def check_sampling(temperature=1.0, top_k=None, top_p=1.0, greedy=False):
    """Raise a ValueError naming the offending argument; return True when the settings are neutral
    (temperature 1, top-k off, top-p off)."""
    t = float(temperature)
    if not math.isfinite(t) or t <= 0.0:
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r} "
                         "(for the temperature -> 0 limit use greedy=True)")
    if top_k is not None and (int(top_k) != top_k or top_k < 0):
        raise ValueError(f"top_k must be an integer >= 0 (0 or None: off), got {top_k!r}")
    p = float(top_p)
    if not (0.0 < p <= 1.0):
        raise ValueError(f"top_p must be in (0, 1] (1: off), got {top_p!r}")
    neutral = is_neutral(t, top_k, p)
    if greedy and not neutral:
        raise ValueError("greedy=True takes the argmax: it cannot be combined with temperature, top_k or top_p "
                         f"(got temperature={temperature!r}, top_k={top_k!r}, top_p={top_p!r})")
    return neutral


def add_sampling_args(ap):
    ap.add_argument("--temperature", type=float, default=1.0, help="softmax temperature (> 0; 1: as trained)")
    ap.add_argument("--top-k", type=int, default=None, help="sample among the k most likely tokens (0 / unset: off)")
    ap.add_argument("--top-p", type=float, default=1.0, help="nucleus: the smallest set of tokens reaching this mass (1: off)")


def sampling_params(temperature=1.0, top_k=None, top_p=1.0):
    """The kernel's params buffer as a CPU tensor: (temperature, top_k or 0, top_p), float32.  A
    top_k at or above the vocabulary means off in the kernel, so it is capped where a float still
    holds it exactly."""
    return torch.tensor([float(temperature), float(min(int(top_k or 0), 1 << 24)), float(top_p)], dtype=torch.float32)


def filter_logits(logits, temperature=1.0, top_k=None, top_p=1.0):
    """``logits / temperature`` over the last dimension with the tokens that top-k / top-p drop set
    to ``-inf``; neutral settings return ``logits`` itself.

    Tokens are ranked by logit descending with a stable sort, so equal logits keep index order (the
    lower index first).  Weights are ``exp((x - max x) / temperature)`` in float64.  Top-k keeps the
    first ``min(top_k, V)`` of the ranking; top-p keeps, of those, the shortest prefix whose weight
    reaches ``top_p`` times their sum -- never fewer than one token."""
    if is_neutral(temperature, top_k, top_p):
        return logits
    V = logits.shape[-1]
    vals, order = torch.sort(logits, dim=-1, descending=True, stable=True)
    v64 = vals.double()
    w = torch.exp((v64 - v64[..., :1]) / float(temperature))
    w = torch.where(torch.isneginf(v64), torch.zeros_like(w), w)    # an all -inf row: weights 0, not NaN
    keep = torch.ones_like(vals, dtype=torch.bool)
    if top_k and top_k < V:
        keep[..., int(top_k):] = False
    w = w * keep
    if float(top_p) < 1.0:
        cum = torch.cumsum(w, dim=-1)
        # rank r stays while the ranks ahead of it have not reached top_p * S_k (rank 0 always stays)
        keep[..., 1:] &= cum[..., :-1] < float(top_p) * cum[..., -1:]
    mask = torch.zeros_like(keep).scatter(-1, order, keep)
    return (logits / temperature).masked_fill(~mask, float("-inf"))
