"""data.PairSampler on the CPU: packing, truncation and masking against a plain-Python reference
(tests/pairs.py), the index stream against BatchSampler's rank-slicing rule, the float identity the
masked kernels' bit-equality tests rest on, and the oracle's verdict on the batches the GPU tests use."""
import numpy as np
import pytest
import torch

import pairs as pr
from oracle import gpt1_oracle as O


def _sampler(pairs, T, B, **kw):
    from replicatinggpt_amd.data import PairSampler
    return PairSampler(pairs, T, B, **kw)


def test_packing_and_masking_match_the_reference():
    """Every row of the packed table, read through cg_gather_pairs' stated formula, is the reference's
    (x, y): short rows (padding), rows longer than T + 1 (left-truncated prompt), rows of exactly T + 1."""
    T = 64
    s = _sampler(pr.TRAIN_PAIRS, T, 4, pad_token=3)
    N = len(pr.TRAIN_PAIRS)
    lens = [len(p) + len(c) for p, c in pr.TRAIN_PAIRS]
    assert min(lens) < T + 1 and max(lens) > T + 1 and (T + 1) in lens      # all three kinds are present
    assert s.ignore_index == -100 and s.B == 4 and s.T == T and s.table_cpu.shape == (N, T + 1)
    ix = list(range(N))
    x, y = pr.gather_formula(s.table_cpu, s.plen_cpu, s.tlen_cpu, ix, T, 3, s.ignore_index)
    rx, ry = pr.reference_batch(pr.TRAIN_PAIRS, ix, T, pad=3)
    assert torch.equal(x, rx) and torch.equal(y, ry)
    for n, (p, c) in enumerate(pr.TRAIN_PAIRS):
        assert int((y[n] != -100).sum()) == len(c)                       # the loss is on the completion, all of it
        assert int(s.tlen_cpu[n]) == min(len(p) + len(c), T + 1) and int(s.plen_cpu[n]) >= 1


def test_left_truncation_keeps_the_completion():
    T = 8
    s = _sampler([(list(range(1, 21)), [30, 31, 32]), ([1], [2, 3, 4, 5, 6, 7, 8, 9])], T, 1)
    assert s.table_cpu[0].tolist() == [15, 16, 17, 18, 19, 20, 30, 31, 32] and int(s.plen_cpu[0]) == 6
    assert s.table_cpu[1].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9] and (int(s.plen_cpu[1]), int(s.tlen_cpu[1])) == (1, 9)
    x, y = pr.gather_formula(s.table_cpu, s.plen_cpu, s.tlen_cpu, [0, 1], T, 0, -100)
    assert y[0].tolist() == [-100] * 5 + [30, 31, 32] and y[1].tolist() == [2, 3, 4, 5, 6, 7, 8, 9]
    assert x[0].tolist() == [15, 16, 17, 18, 19, 20, 30, 31]


@pytest.mark.parametrize("bad", [([], [1]), ([1], []), ([1], list(range(9)))])
def test_bad_pairs_raise(bad):
    with pytest.raises(ValueError):
        _sampler([([1, 2], [3])] * 3 + [bad], 8, 1)


def test_split_and_rank_slicing_follow_batch_sampler():
    """One global draw of B*W indices per get_batch, rank r keeps [rB, (r+1)B) -- BatchSampler.draw_ix's
    rule -- over the 90/10 split of the rows."""
    B, W, N = 6, 2, len(pr.TRAIN_PAIRS)
    n_train = int(0.9 * N)
    ranks = [pr.train_sampler(world=W, rank=r, seed=9, B=B) for r in range(W)]
    g = torch.Generator().manual_seed(9)
    for split, lo, n in (("train", 0, n_train), ("val", n_train, N - n_train), ("train", 0, n_train)):
        want = torch.randint(n, (B * W,), generator=g) + lo
        for r, s in enumerate(ranks):
            assert torch.equal(s.draw_ix(split), want[r * B:(r + 1) * B])
        assert int(want.min()) >= lo and int(want.max()) < lo + n
    # the rule is BatchSampler's own: same generator state, same bound -> the same slice
    from replicatinggpt_amd.data import BatchSampler, TokenStream
    T = 4
    bs = BatchSampler(TokenStream(torch.arange(100) % 7), T, B, world_size=W, rank=1,
                      generator=torch.Generator().manual_seed(5))
    n_bs = len(bs.s.train_cpu) - T
    ps = _sampler([([1], [2])] * ((n_bs * 10 + 8) // 9), T, B, world_size=W, rank=1,
                  generator=torch.Generator().manual_seed(5))
    assert ps.n == n_bs
    assert torch.equal(ps.draw_ix("train"), bs.draw_ix("train"))


def test_empty_split_raises():
    s = _sampler([([1], [2])] * 3, 4, 1)      # int(0.9 * 3) = 2 train rows, 1 val row
    s.draw_ix("val")
    with pytest.raises(ValueError):
        _sampler([([1], [2])], 4, 1).draw_ix("train")


def test_reciprocal_identity_up_to_2_20():
    """The masked forward divides in fp32 on the device (1.0f / (float)count); the unmasked backward
    takes the host's double 1.0 / M rounded to fp32 by the call.  They are the same float for every
    M in 1 .. 2^20 (double rounding is harmless here: 1 / M with M < 2^24 is never within 2^-53 relative
    of an fp32 rounding boundary), which is what lets test_gpu_masked_ce.py ask for bit equality of the
    masked and unmasked entry points when nothing is ignored."""
    M = np.arange(1, (1 << 20) + 1, dtype=np.int64)
    dev = np.float32(1) / M.astype(np.float32)
    host = (1.0 / M.astype(np.float64)).astype(np.float32)
    assert dev.dtype == np.float32 and np.array_equal(dev.view(np.uint32), host.view(np.uint32))


def test_oracle_accepts_the_gradient_batch():
    """The first batches of the seeded sampler that test_gpu_pairs_train.py trains on: a quarter to
    three quarters of the targets valid, three different counts on three steps, and a finite oracle loss and
    gradient (F.cross_entropy's ignore_index = -100 is the oracle's default)."""
    s = pr.train_sampler()
    T = pr.E_SHAPE["block_size"]
    counts = []
    for k in range(3):
        x, y = pr.reference_batch(pr.TRAIN_PAIRS, s.draw_ix("train").tolist(), T)
        assert 0.25 <= pr.valid_share(y) <= 0.75
        counts.append(int((y != pr.IGNORE).sum()))
        if k == 0:
            ocfg = O.OracleConfig(block_size=T, n_embd=pr.E_SHAPE["n_embd"], n_head=pr.E_SHAPE["n_head"],
                                  n_layers=pr.E_SHAPE["n_layers"], dropout=0.0)
            torch.manual_seed(1337)
            _, loss, g = O.loss_and_grads(O.init_params(ocfg), x, y, ocfg)
            assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in g.values())
            # the mean is over the valid targets: an all-ignored row set changes nothing
            x2, y2 = torch.cat([x, x[:2]]), torch.cat([y, torch.full_like(y[:2], pr.IGNORE)])
            torch.manual_seed(1337)
            _, loss2, _ = O.loss_and_grads(O.init_params(ocfg), x2, y2, ocfg)
            assert abs(float(loss2) - float(loss)) < 1e-6
    assert len(set(counts)) == 3


def test_oracle_finetune_fixes_the_step_count():
    """The oracle's AdamW loop at lr 1e-2 reproduces all four completions first after E2E_ORACLE_STEPS
    steps; the GPU test trains twice as long (pairs.E2E_STEPS), where the oracle still does."""
    done = pr.oracle_finetune(pr.E2E_STEPS)
    assert done.index(True) + 1 == pr.E2E_ORACLE_STEPS and done[-1]
    assert pr.E2E_STEPS == 2 * pr.E2E_ORACLE_STEPS


def test_read_pairs_names_the_bad_line(tmp_path):
    from replicatinggpt_amd.data import CharTokenizer
    from replicatinggpt_amd.gpt1 import read_pairs
    tok = CharTokenizer("abc: xyz")
    f = tmp_path / "p.jsonl"
    f.write_text('{"prompt": "ab: ", "completion": "xyz"}\n\n{"prompt": "abQ", "completion": "x"}\n')
    with pytest.raises(SystemExit) as e:
        read_pairs(str(f), tok)
    assert ":3:" in str(e.value) and "Q" in str(e.value)
    f.write_text('{"prompt": "ab: ", "completion": "xyz"}\n')
    assert read_pairs(str(f), tok) == [(tok.encode("ab: "), tok.encode("xyz"))]
