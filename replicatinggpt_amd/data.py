"""Tokenizer, train/val split and get_batch (GPT1.py:25-83), MI355X-side.

* ``CharTokenizer`` -- the ``encoder == 'base'`` branch (GPT1.py:54-66): sorted character
  vocabulary, encode/decode.  (The tiktoken/nltk branches need the network and are out of scope,
  SURVEY §0.)
* ``TokenStream`` -- the int64 token tensor and its 90/10 split (GPT1.py:66-70), kept resident in
  HBM as uint8 (the vocabulary has 65 symbols).
* ``BatchSampler.get_batch`` -- GPT1.py:75-83: the offsets ``ix`` are drawn with ``torch.randint``
  on the CPU default generator exactly like the reference (so index streams are bit-identical for a
  fixed seed), then the (B,T) windows and shifted targets are gathered on the device by a HIP
  kernel instead of 2*B Python slices + stack + H2D copy.  With data parallelism every rank draws the
  same global ``B*W`` offsets and keeps its own slice (one draw of B*W == W consecutive reference
  draws).
* ``PairSampler`` -- fine-tuning on (prompt, completion) pairs, which GPT1.py does not have: one pair
  per batch row, the loss taken on the completion only (targets elsewhere are ``ignore_index``, the
  masked cross entropy of DESIGN.md §4).  Row indices are drawn like BatchSampler's offsets; the rows
  are gathered, padded and masked on the device (cg_gather_pairs).
"""
import os

import torch

from . import ops

DEFAULT_INPUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "input.txt")


class CharTokenizer:
    def __init__(self, text):
        self.chars = sorted(list(set(text)))               # GPT1.py:58
        self.vocab_size = len(self.chars)                   # GPT1.py:59
        self.stoi = {ch: i for i, ch in enumerate(self.chars)}   # GPT1.py:61
        self.itos = {i: ch for i, ch in enumerate(self.chars)}   # GPT1.py:62

    def encode(self, s):
        return [self.stoi[c] for c in s]                    # GPT1.py:63

    def decode(self, ids):
        return "".join([self.itos[i] for i in ids])          # GPT1.py:64


class TokenStream:
    def __init__(self, data, device=None):
        self.data = data                                    # int64 CPU, GPT1.py:66
        n = int(0.9 * len(data))                            # GPT1.py:68
        self.n = n
        self.train_cpu = data[:n]                           # GPT1.py:69
        self.val_cpu = data[n:]                             # GPT1.py:70
        self.device = None
        self.train_dev = self.val_dev = None
        if device is not None:
            self.to(device)

    def to(self, device):
        device = torch.device(device)
        self.device = device
        dt = torch.uint8 if int(self.data.max()) < 256 else torch.int64
        self.train_dev = self.train_cpu.to(dt).to(device)
        self.val_dev = self.val_cpu.to(dt).to(device)
        return self

    @classmethod
    def from_file(cls, path=DEFAULT_INPUT, device=None):
        with open(path, "r", encoding="utf-8") as f:        # GPT1.py:26-27,55-56
            text = f.read()
        tok = CharTokenizer(text)
        data = torch.tensor(tok.encode(text), dtype=torch.long)
        return tok, cls(data, device)

    @classmethod
    def synthetic(cls, n_tokens=1 << 20, vocab=65, seed=1337, device=None):
        """SURVEY §8d synthetic stream: randint(65, (2^20,)) on a seeded private generator."""
        g = torch.Generator().manual_seed(seed)
        return cls(torch.randint(vocab, (n_tokens,), generator=g, dtype=torch.long), device)


class BatchSampler:
    def __init__(self, stream, block_size, batch_size, world_size=1, rank=0, generator=None):
        self.s = stream
        self.T = block_size
        self.B = batch_size
        self.W = world_size
        self.rank = rank
        self.generator = generator
        self._ring = None
        self._ring_i = 0

    def _staging(self, dev):
        """Ring of pinned host buffers; an event per slot keeps a host write behind the H2D copy
        that last read the slot (no stream-wide synchronisation)."""
        if self._ring is None:
            pin = dev.type == "cuda"
            self._ring = [(torch.empty(self.B, dtype=torch.int64, pin_memory=pin), None) for _ in range(4)]
        i = self._ring_i
        self._ring_i = (i + 1) % len(self._ring)
        buf, ev = self._ring[i]
        if ev is not None:
            ev.synchronize()
        return i, buf

    def draw_ix(self, split):
        """GPT1.py:78 -- global draw of B*W offsets on the CPU generator (rank-sliced)."""
        n = len(self.s.train_cpu if split == "train" else self.s.val_cpu)
        ix = torch.randint(n - self.T, (self.B * self.W,), generator=self.generator)
        return ix[self.rank * self.B:(self.rank + 1) * self.B]

    def get_batch(self, split, out=None):
        ix = self.draw_ix(split)
        data = self.s.train_dev if split == "train" else self.s.val_dev
        dev = data.device
        i, buf = self._staging(dev)
        buf.copy_(ix)
        ix_dev = buf.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring[i] = (buf, ev)
        if out is None:
            x = torch.empty((self.B, self.T), dtype=torch.int64, device=dev)
            y = torch.empty((self.B, self.T), dtype=torch.int64, device=dev)
        else:
            x, y = out
        ops.gather_batch(data, ix_dev, x, y)
        return x, y


def pack_pairs(pairs, block_size):
    """Pack (prompt_tokens, completion_tokens) pairs into an int64 table [N, T+1] (row = prompt +
    completion, zero-filled past its length) with the prompt lengths ``plen`` and total lengths
    ``tlen``.  A row longer than T+1 loses the front of its prompt; at least one prompt token stays,
    since the first completion token is predicted from it."""
    T = block_size
    table = torch.zeros((len(pairs), T + 1), dtype=torch.int64)
    plen = torch.empty(len(pairs), dtype=torch.int64)
    tlen = torch.empty(len(pairs), dtype=torch.int64)
    for n, (prompt, completion) in enumerate(pairs):
        prompt, completion = list(prompt), list(completion)
        if not prompt or not completion:
            raise ValueError(f"pair {n}: the prompt and the completion must both be non-empty")
        if len(completion) > T:
            raise ValueError(f"pair {n}: a completion of {len(completion)} tokens does not fit block_size {T} "
                             "(one prompt token must precede it)")
        over = len(prompt) + len(completion) - (T + 1)
        if over > 0:
            prompt = prompt[over:]
        row = prompt + completion
        table[n, :len(row)] = torch.tensor(row, dtype=torch.int64)
        plen[n], tlen[n] = len(prompt), len(row)
    return table, plen, tlen


class PairSampler:
    """get_batch over (prompt, completion) pairs: x[b] = the packed row up to its last input token,
    ``pad_token`` after it; y[b, j] = the next token where that token belongs to the completion,
    ``ignore_index`` (-100, F.cross_entropy's default) elsewhere.  90/10 train/val split of the rows,
    as TokenStream's.  Every rank draws the same global B*W row indices on the CPU generator and
    keeps its own slice, exactly as BatchSampler does."""

    ignore_index = -100

    def __init__(self, pairs, block_size, batch_size, world_size=1, rank=0, generator=None, pad_token=0,
                 device=None):
        self.T = block_size
        self.B = batch_size
        self.W = world_size
        self.rank = rank
        self.generator = generator
        self.pad_token = int(pad_token)
        self.table_cpu, self.plen_cpu, self.tlen_cpu = pack_pairs(pairs, block_size)
        self.n = int(0.9 * len(pairs))      # rows [0, n) train, [n, N) val
        self.device = None
        self.table_dev = self.plen_dev = self.tlen_dev = None
        self._ring = None
        self._ring_i = 0
        if device is not None:
            self.to(device)

    def to(self, device):
        self.device = torch.device(device)
        self.table_dev = self.table_cpu.to(self.device)
        self.plen_dev = self.plen_cpu.to(self.device)
        self.tlen_dev = self.tlen_cpu.to(self.device)
        return self

    _staging = BatchSampler._staging

    def draw_ix(self, split):
        """Global draw of B*W row indices of ``split`` on the CPU generator (rank-sliced)."""
        lo, n = (0, self.n) if split == "train" else (self.n, len(self.table_cpu) - self.n)
        if n <= 0:
            raise ValueError(f"PairSampler: the {split} split is empty ({len(self.table_cpu)} pairs, 90/10 split)")
        ix = torch.randint(n, (self.B * self.W,), generator=self.generator)
        return ix[self.rank * self.B:(self.rank + 1) * self.B] + lo

    def get_batch(self, split, out=None):
        ix = self.draw_ix(split)
        if self.table_dev is None:
            self.to("cuda")
        dev = self.device
        i, buf = self._staging(dev)
        buf.copy_(ix)
        ix_dev = buf.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring[i] = (buf, ev)
        if out is None:
            x = torch.empty((self.B, self.T), dtype=torch.int64, device=dev)
            y = torch.empty((self.B, self.T), dtype=torch.int64, device=dev)
        else:
            x, y = out
        ops.gather_pairs(self.table_dev, self.plen_dev, self.tlen_dev, ix_dev, x, y, self.pad_token,
                         self.ignore_index)
        return x, y


def first_fit(lengths, order, capacity):
    """First-fit packing: the items, taken in ``order``, each go into the first row that still has
    room for their length, else into a new row.  Returns the rows as lists of item indices."""
    rows, room = [], []
    for n in order:
        need = int(lengths[n])
        for r, free in enumerate(room):
            if need <= free:
                rows[r].append(int(n))
                room[r] -= need
                break
        else:
            rows.append([int(n)])
            room.append(capacity - need)
    return rows


class PackedPairSampler:
    """get_batch over (prompt, completion) pairs with several pairs per row (DESIGN.md §4 "Packed
    rows").  A pair takes ``tlen - 1`` input positions (its packed row without the last token, as
    PairSampler's x); a row is a concatenation of such segments and, where they leave room, a tail of
    ``pad_token``.  get_batch returns (x, y, seg_start): seg_start[b, t] (int32) is the index of the
    first token of the segment that holds position t, the padding tail being a segment of its own.
    y[b, j] is the next token where that token belongs to the segment's completion and
    ``ignore_index`` elsewhere -- PairSampler's rule per segment, so no target crosses a segment's end
    -- and ``ignore_index`` on the padding.

    The pairs are split 90/10 as PairSampler's rows; each split's pairs are shuffled with
    ``generator`` (train first, then val) and packed first-fit into rows of capacity ``block_size``;
    ``repack()`` reshuffles and repacks.  get_batch draws B*W packed-row indices of the split on the
    CPU generator, every rank the same ones, and keeps its own slice, as the other samplers do."""

    ignore_index = -100
    packed = True

    def __init__(self, pairs, block_size, batch_size, world_size=1, rank=0, generator=None, pad_token=0,
                 device=None):
        self.T = block_size
        self.B = batch_size
        self.W = world_size
        self.rank = rank
        self.generator = generator
        self.pad_token = int(pad_token)
        self.table_cpu, self.plen_cpu, self.tlen_cpu = pack_pairs(pairs, block_size)
        self.n = int(0.9 * len(pairs))      # pairs [0, n) train, [n, N) val
        self.device = None
        self._dev = {}
        self._ring = None
        self._ring_i = 0
        self.repack()
        if device is not None:
            self.to(device)

    def _build(self, lo, n):
        """Shuffle pairs lo .. lo+n-1 and pack them: (x, y, seg_start) tables [rows, T] and the rows."""
        T = self.T
        order = (torch.randperm(n, generator=self.generator) + lo).tolist()
        rows = first_fit(self.tlen_cpu - 1, order, T)
        x = torch.full((len(rows), T), self.pad_token, dtype=torch.int64)
        y = torch.full((len(rows), T), self.ignore_index, dtype=torch.int64)
        seg = torch.empty((len(rows), T), dtype=torch.int32)
        for r, members in enumerate(rows):
            at = 0
            for m in members:
                pl, tl = int(self.plen_cpu[m]), int(self.tlen_cpu[m])
                row = self.table_cpu[m]
                x[r, at:at + tl - 1] = row[:tl - 1]
                y[r, at + pl - 1:at + tl - 1] = row[pl:tl]     # targets inside the completion only
                seg[r, at:at + tl - 1] = at
                at += tl - 1
            seg[r, at:] = at                                    # the padding tail: a segment of its own
        return x, y, seg, rows

    def repack(self):
        """Reshuffle each split's pairs (on ``generator``) and pack them again."""
        N = len(self.table_cpu)
        self.tables_cpu, self.rows = {}, {}
        for split, lo, n in (("train", 0, self.n), ("val", self.n, N - self.n)):
            if n > 0:
                *self.tables_cpu[split], self.rows[split] = self._build(lo, n)
        used = sum(sum(int(self.tlen_cpu[m]) - 1 for m in members) for rows in self.rows.values() for members in rows)
        total = sum(len(rows) for rows in self.rows.values()) * self.T
        self.fill = used / total if total else 0.0   # share of non-pad positions of the packed tables
        if self.device is not None:
            self.to(self.device)
        return self

    def to(self, device):
        self.device = torch.device(device)
        self._dev = {s: tuple(t.to(self.device) for t in tabs) for s, tabs in self.tables_cpu.items()}
        return self

    _staging = BatchSampler._staging

    def draw_ix(self, split):
        """Global draw of B*W packed-row indices of ``split`` on the CPU generator (rank-sliced)."""
        if split not in self.tables_cpu:
            raise ValueError(f"PackedPairSampler: the {split} split is empty ({len(self.table_cpu)} pairs, 90/10 "
                             "split)")
        n = len(self.rows[split])
        ix = torch.randint(n, (self.B * self.W,), generator=self.generator)
        return ix[self.rank * self.B:(self.rank + 1) * self.B]

    def get_batch(self, split, out=None):
        ix = self.draw_ix(split)
        if self.device is None:
            self.to("cuda")
        dev = self.device
        i, buf = self._staging(dev)
        buf.copy_(ix)
        ix_dev = buf.to(dev, non_blocking=True)
        if dev.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            self._ring[i] = (buf, ev)
        if out is None:
            x = torch.empty((self.B, self.T), dtype=torch.int64, device=dev)
            y = torch.empty((self.B, self.T), dtype=torch.int64, device=dev)
            seg = torch.empty((self.B, self.T), dtype=torch.int32, device=dev)
        else:
            x, y, seg = out
        xt, yt, st = self._dev[split]
        # not on the hot path: three row gathers (the tables hold whole packed rows)
        torch.index_select(xt, 0, ix_dev, out=x)
        torch.index_select(yt, 0, ix_dev, out=y)
        torch.index_select(st, 0, ix_dev, out=seg)
        return x, y, seg
