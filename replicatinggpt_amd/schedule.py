"""Learning-rate schedules: pure functions of the iteration, for engine.TrainStep(lr_schedule=...)
and optim.AdamW.set_lr (the reference trains at a constant learning rate, GPT1.py:218)."""
import math


def warmup_cosine(it, base_lr, warmup_iters, decay_iters, min_lr=0.0):
    """Linear warm-up, cosine decay, then a floor:

    * it < warmup_iters:   base_lr * (it + 1) / warmup_iters  (the first step runs at base_lr / warmup_iters)
    * it >= decay_iters:   min_lr
    * between:             min_lr + (base_lr - min_lr) * (1 + cos(pi * r)) / 2 with
                           r = (it - warmup_iters) / (decay_iters - warmup_iters), so base_lr at
                           it == warmup_iters and min_lr at decay_iters
    """
    if warmup_iters < 0 or decay_iters < warmup_iters:
        raise ValueError("warmup_cosine: need 0 <= warmup_iters <= decay_iters")
    if it < warmup_iters:
        return base_lr * (it + 1) / warmup_iters
    if it >= decay_iters:
        return min_lr
    r = (it - warmup_iters) / (decay_iters - warmup_iters)
    return min_lr + 0.5 * (1.0 + math.cos(math.pi * r)) * (base_lr - min_lr)
