"""data.PackedPairSampler against its plain-Python statement, and the two references the GPU tests of
packed rows lean on against each other (tests/packing.py).  No GPU: the sampler's tables are built on
the CPU and its gather is plain torch indexing, so it runs here with device="cpu"."""
import pytest
import torch

import packing as PK
import pairs as PR
from replicatinggpt_amd.data import PackedPairSampler, first_fit

T, B = 64, 6
PAIRS = PK.PACKED_PAIRS


def sampler(seed=3, **kw):
    kw.setdefault("device", "cpu")
    return PackedPairSampler(PAIRS, T, B, generator=torch.Generator().manual_seed(seed), **kw)


def test_first_fit_is_the_plain_statement():
    lengths = [len(p) + len(c) - 1 for p, c in PAIRS]
    order = torch.randperm(len(PAIRS), generator=torch.Generator().manual_seed(0)).tolist()
    rows = first_fit(lengths, order, T)
    assert rows == PK.plain_first_fit(lengths, order, T)
    assert sorted(n for r in rows for n in r) == list(range(len(PAIRS)))
    assert all(sum(lengths[n] for n in r) <= T for r in rows)


def test_tables_and_batches_match_the_plain_statement():
    s = sampler()
    ref, g = PK.plain_sampler(PAIRS, T, 3)
    for split in ("train", "val"):
        x, y, seg, rows = ref[split]
        assert s.rows[split] == rows
        for got, want in zip(s.tables_cpu[split], (x, y, seg)):
            assert got.dtype == want.dtype and torch.equal(got, want)
    for split in ("train", "val", "train"):
        x, y, seg, rows = ref[split]
        ix = torch.randint(len(rows), (B,), generator=g)
        bx, by, bs = s.get_batch(split)
        assert bs.dtype == torch.int32 and bx.dtype == by.dtype == torch.int64
        assert torch.equal(bx, x[ix]) and torch.equal(by, y[ix]) and torch.equal(bs, seg[ix])


def test_rows_hold_three_to_five_pairs_and_fill():
    s = sampler()
    sizes = [len(r) for r in s.rows["train"][:-1]]   # the last row takes what is left
    assert min(sizes) >= 3 and max(sizes) <= 5, sizes
    used = sum(len(p) + len(c) - 1 for rows in s.rows.values() for r in rows for p, c in (PAIRS[n] for n in r))
    assert s.fill == pytest.approx(used / (T * sum(len(r) for r in s.rows.values())))
    assert 0.8 < s.fill <= 1.0
    assert s.packed is True and s.ignore_index == -100


def test_targets_ignored_at_prompts_segment_ends_and_padding():
    s = sampler()
    x, y, seg, rows = s.tables_cpu["train"] + [s.rows["train"]]
    for r, members in enumerate(rows):
        at = 0
        for n in members:
            p, c = PAIRS[n]
            L = len(p) + len(c) - 1
            assert x[r, at:at + L].tolist() == (p + c)[:-1]
            assert (y[r, at:at + len(p) - 1] == -100).all()                  # prompt positions
            assert y[r, at + len(p) - 1:at + L].tolist() == c                # the completion, last one included
            if at + L < T:                                                   # the next position starts another
                assert seg[r, at + L] == at + L                              # segment: no target crosses the end
            at += L
        assert (y[r, at:] == -100).all() and (x[r, at:] == 0).all()          # padding tail


def test_seg_start_invariants():
    s = sampler()
    for split in ("train", "val"):
        seg = s.tables_cpu[split][2].long()
        t = torch.arange(T)[None]
        assert (seg <= t).all() and (seg >= 0).all()
        assert (seg[:, 1:] >= seg[:, :-1]).all()                             # non-decreasing
        assert (seg.gather(1, seg) == seg).all()                             # constant on a segment: start's start
        assert (seg[:, 0] == 0).all()
        changed = seg[:, 1:] != seg[:, :-1]
        assert (seg[:, 1:][changed] == t.expand_as(seg)[:, 1:][changed]).all()   # a new value is the position itself


def test_split_is_90_10_of_the_pairs():
    s = sampler()
    n = int(0.9 * len(PAIRS))
    assert sorted(m for r in s.rows["train"] for m in r) == list(range(n))
    assert sorted(m for r in s.rows["val"] for m in r) == list(range(n, len(PAIRS)))


def test_rank_slicing():
    W = 3
    whole = sampler(seed=9)
    whole.B = B * W
    ranks = [PackedPairSampler(PAIRS, T, B, world_size=W, rank=r, generator=torch.Generator().manual_seed(9),
                               device="cpu") for r in range(W)]
    for _ in range(2):
        ix = whole.draw_ix("train")
        for r, s in enumerate(ranks):
            assert torch.equal(s.draw_ix("train"), ix[r * B:(r + 1) * B])


def test_seeded_generator_is_deterministic_and_repack_changes_rows():
    a, b = sampler(seed=5), sampler(seed=5)
    assert a.rows == b.rows
    for _ in range(3):
        for u, v in zip(a.get_batch("train"), b.get_batch("train")):
            assert torch.equal(u, v)
    before = [list(r) for r in a.rows["train"]]
    a.repack()
    assert a.rows["train"] != before
    assert sorted(m for r in a.rows["train"] for m in r) == sorted(m for r in before for m in r)
    b.repack()
    assert a.rows == b.rows and torch.equal(a.get_batch("val")[2], b.get_batch("val")[2])


def test_truncation_reuses_pack_pairs_rule():
    long = [(list(range(1, 41)), list(range(1, 31)))] * 10          # 70 tokens: the prompt loses its front
    s = PackedPairSampler(long, T, 2, generator=torch.Generator().manual_seed(0), device="cpu")
    x, y, seg = s.tables_cpu["train"]
    rx, ry = PR.reference_batch(long, [0], T)
    assert torch.equal(x[0], rx[0]) and torch.equal(y[0], ry[0]) and (seg[0] == 0).all()


def test_errors():
    with pytest.raises(ValueError, match="train split is empty"):   # int(0.9 * 1) = 0 training pairs
        PackedPairSampler(PAIRS[:1], T, 2, device="cpu").get_batch("train")
    with pytest.raises(ValueError, match="does not fit block_size"):
        PackedPairSampler([([1], list(range(T + 1)))], T, 2, device="cpu")
    with pytest.raises(ValueError, match="non-empty"):
        PackedPairSampler([([], [1])], T, 2, device="cpu")


# ---------------------------------------------------------------------------------------
# the references against each other
# ---------------------------------------------------------------------------------------
SEGMENTATIONS = [[], [1, 31, 1], [32, 32], [31, 2, 30], [63], [5, 17, 9], [64]]


@pytest.mark.parametrize("lengths", SEGMENTATIONS)
def test_dense_masked_reference_is_each_segment_alone(lengths):
    """At p = 0 the block-diagonal reference and the per-segment-alone reference agree to fp64 round-off:
    the two statements of "packed = alone" that the GPU tests use say the same thing."""
    g = torch.Generator().manual_seed(1)
    Bq, Tq, H, D = 2, 64, 2, 8
    q, k, v = (torch.randn(Bq, Tq, H, D, generator=g, dtype=torch.float64) for _ in range(3))
    seg = torch.stack([PK.seg_of_lengths(lengths, Tq), PK.seg_of_lengths([7, 20], Tq)])
    a = PK.attn_ref_seg(q, k, v, 0.3, seg)
    b = PK.attn_ref_alone(q, k, v, 0.3, seg)
    assert float((a - b).abs().max()) < 1e-13
    assert torch.equal(PK.seg_end_of(seg)[0], torch.tensor(
        [e for s, e in PK.segments(seg[0]) for _ in range(e - s)], dtype=torch.int32))


def test_all_zero_seg_start_is_the_causal_reference():
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(1, 24, 2, 4, generator=g, dtype=torch.float64) for _ in range(3))
    seg = torch.zeros((1, 24), dtype=torch.int32)
    s = torch.einsum("bthd,bshd->bhts", q, k) * 0.5
    s = s.masked_fill(~torch.tril(torch.ones(24, 24, dtype=torch.bool)), float("-inf"))
    ref = torch.einsum("bhts,bshd->bthd", torch.softmax(s, -1), v)
    assert torch.equal(PK.attn_ref_seg(q, k, v, 0.5, seg), ref)


# ---------------------------------------------------------------------------------------
# the tables of the long-row op tests (packing.RING_* / F32_* / RESCALE_*, test_gpu_packed_attn's T 192)
# ---------------------------------------------------------------------------------------
def _t192():
    import test_gpu_packed_attn as A   # plain tables; nothing in it touches a device at import
    return A.SEGS[192], A.LEAK[192]


def _tables():
    segs192, leak192 = _t192()
    out = [("ring", T, rows) for T, rows in PK.RING_SEGS.items()] + [("f32", T, rows) for T, rows in PK.F32_SEGS.items()]
    return out + [("resident", 192, segs192)]


def bounds(rows):
    """Every position at which a segment other than the first starts, over the rows of a table."""
    return {at for r in rows for at in torch.tensor([0] + r).cumsum(0).tolist()[1:]}


def test_long_tables_fit_their_rows():
    for _, T, rows in _tables():
        assert all(sum(r) <= T and min(r, default=1) >= 1 for r in rows), (T, rows)
    assert sum(_t192()[1]) <= 192
    assert all(sum(l) <= T and 0 <= n < len(PK.segments(PK.seg_of_lengths(l, T))) for T, l, n in PK.RING_LEAK.values())
    assert all(sum(l) <= T for T, l in list(PK.F32_LEAK.items()) + PK.RESCALE_RECIPES)
    assert {T for _, T, _ in PK.RING_SHAPES} == set(PK.RING_SEGS) and {s[1] for s in PK.F32_SHAPES} == set(PK.F32_SEGS)
    assert set(PK.F32_LEAK) <= set(PK.F32_SEGS)
    assert sum(PK.cycling(512)) <= 512 < sum(PK.cycling(512)) + len(PK.cycling(512)) + 1 and PK.cycling(512)[:3] == [1, 2, 3]


@pytest.mark.parametrize("kind,T,rows", [t for t in _tables() if t[1] <= 576],
                         ids=[f"{k}-{T}" for k, T, _ in _tables() if T <= 576])
def test_long_tables_dense_reference_is_each_segment_alone(kind, T, rows):
    g = torch.Generator().manual_seed(3)
    B, H, D = 2, 1, 4
    q, k, v = (torch.randn(B, T, H, D, generator=g, dtype=torch.float64) for _ in range(3))
    for seg in PK.seg_batches(rows, B, T):
        a, b = PK.attn_ref_seg(q, k, v, 0.3, seg), PK.attn_ref_alone(q, k, v, 0.3, seg)
        assert float((a - b).abs().max()) < 1e-13
        assert torch.equal(PK.seg_end_of(seg)[0], torch.tensor(
            [e for s, e in PK.segments(seg[0]) for _ in range(e - s)], dtype=torch.int32))


def test_ring_tables_hold_their_edge_classes():
    """Per T: [] is there; a bound on 256 k and on each side of one; a bound on 128 k - 1 and 128 k + 1; a
    segment starting in every 256-query block >= 1 (T 1024: blocks 2 and 3 -- its four rows are all the fp64
    reference affords; block 1 gets its start from RING_LEAK's T 1024 row, the bitwise test)."""
    for T, rows in PK.RING_SEGS.items():
        bs = bounds(rows)
        assert [] in rows
        assert {0, 1, 255} <= {b % 256 for b in bs}, (T, sorted(bs))
        assert {1, 127} <= {b % 128 for b in bs}, (T, sorted(bs))
        blocks = set(range(1, (T + 255) // 256)) - ({1} if T == 1024 else set())
        assert blocks <= {b // 256 for b in bs}, (T, sorted(bs))
        assert any(max(r, default=0) >= 300 for r in rows)          # a run of leading tiles skipped whole
    T, lengths, n = PK.RING_LEAK["last-block-1024"]
    assert 1 in {b // 256 for b in bounds([lengths])}
    for which, (T, lengths, n) in PK.RING_LEAK.items():
        s, e = PK.segments(PK.seg_of_lengths(lengths, T))[n]
        last = (T - 1) // 256 * 256
        if which == "straddle":
            assert s < 256 < e
        elif which.startswith("last-block"):
            assert last <= s and e < T
        else:
            assert s == 0


def test_f32_tables_hold_their_edge_classes():
    """Per T: []; bounds on 64 k and either side; on a wave's 16-query edge away from 64 k, one either side;
    a bound inside a wave; segments that start at >= 64 and at >= 128; a length-1 segment on a tile edge."""
    for T, rows in PK.F32_SEGS.items():
        bs = bounds(rows)
        assert [] in rows
        assert {0, 1, 63} <= {b % 64 for b in bs}, (T, sorted(bs))
        on16 = {b % 64 for b in bs}
        assert on16 & {15, 31, 47} and on16 & {16, 32, 48} and on16 & {17, 33, 49}, (T, sorted(bs))
        assert any(b % 16 not in (0, 1, 15) for b in bs), (T, sorted(bs))
        assert any(64 <= b < 128 for b in bs) and any(b >= 128 for b in bs), (T, sorted(bs))
        ones = [s for r in rows for s, e in PK.segments(PK.seg_of_lengths(r, T)) if e - s == 1]
        assert any(s % 64 in (0, 63) for s in ones), (T, ones)
    for T, lengths in PK.F32_LEAK.items():
        spans = PK.segments(PK.seg_of_lengths(lengths, T))
        assert len(spans) >= 3 and spans[1][0] < 64 * (spans[1][1] // 64) and spans[-1][0] >= 64


def test_resident_192_table_holds_its_edge_classes():
    segs, leak = _t192()
    assert [] in segs and {63, 64, 65, 128, 129} <= bounds(segs)
    assert len(PK.segments(PK.seg_of_lengths(leak, 192))) >= 3


@pytest.mark.parametrize("T,lengths", PK.RESCALE_RECIPES, ids=[f"T{T}" for T, _ in PK.RESCALE_RECIPES])
def test_rescale_recipes_force_the_rescale_in_every_long_segment(T, lengths):
    """The precondition test_forced_rescale_inside_a_segment asserts again before its device call: every
    segment of >= 130 positions has queries with a later visible 64-key tile more than RESCALE_THR (log2
    units) above their earlier ones; shorter segments are left alone and have none."""
    H, D = 2, 64
    d = H * D
    qkv, seg_row, scale = PK.rescale_data(T, lengths, H, D)
    q, k = (qkv[:, j * d:(j + 1) * d].double().view(1, T, H, D) for j in range(2))
    fires = PK.rescale_query_tiles(q, k, scale, seg_row)
    print(fires)
    long = [sp for sp in fires if sp[1] - sp[0] >= PK.RESCALE_MIN_SEGMENT]
    assert len(long) == {256: 1, 512: 2, 1024: 3}[T]
    assert all(fires[sp] > 0 for sp in long), fires
    assert all(fires[sp] == 0 for sp in fires if sp not in long), fires
    # rescale_fires against its plain statement, for the last query of the last long segment (head 0)
    s, e = long[-1]
    i = e - 1
    sc = (k[0, s:i + 1, 0] @ q[0, i, 0]) * scale * 1.4426950408889634
    tiles = {}
    for j in range(s, i + 1):
        tiles[j // 64] = max(tiles.get(j // 64, float("-inf")), float(sc[j - s]))
    order = sorted(tiles)
    plain = [t for n, t in enumerate(order) if n and tiles[t] > max(tiles[u] for u in order[:n]) + PK.RESCALE_THR]
    got = (torch.nonzero(PK.rescale_fires(q, k, scale, seg_row)[0, i]).flatten() + 1).tolist()
    assert got == plain and len(plain) >= 1, (got, plain)


def test_packed_oracle_of_one_segment_rows_is_the_oracle():
    """Rows that hold one pair and no padding: packed_oracle is O.loss_and_grads on the batch."""
    from oracle import gpt1_oracle as O
    ocfg = O.OracleConfig(dropout=0.0, **PR.E2E_SHAPE)
    torch.manual_seed(0)
    P = O.init_params(ocfg)
    g = torch.Generator().manual_seed(4)
    x = torch.randint(1, 65, (3, 16), generator=g)
    y = torch.randint(1, 65, (3, 16), generator=g)
    y[:, :5] = -100
    seg = torch.zeros((3, 16), dtype=torch.int32)
    lg, loss, grads = PK.packed_oracle(P, x, y, seg, ocfg)
    rlg, rloss, rgrads = O.loss_and_grads(P, x, y, ocfg)
    assert torch.allclose(lg.reshape(-1, 65), rlg, rtol=1e-5, atol=1e-6)
    assert abs(float(loss) - float(rloss)) < 1e-6
    for k2 in rgrads:
        assert torch.allclose(grads[k2], rgrads[k2], rtol=1e-4, atol=1e-7), k2


def test_e2e_step_count_comes_from_the_packed_oracle():
    """The packed end-to-end test trains twice as long as the oracle's own loop on the packed batches
    needs to reproduce the four completions (as pairs.oracle_finetune fixes test_gpu_pairs_train's)."""
    done = PK.oracle_finetune_packed(PK.E2E_STEPS)
    assert done.index(True) + 1 == PK.E2E_ORACLE_STEPS and done[PK.E2E_STEPS - 1]
    assert PK.E2E_STEPS == 2 * PK.E2E_ORACLE_STEPS
