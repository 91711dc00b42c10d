"""Guard-band boxes for the memory-footprint tests (test_cpu_footprint.py, test_gpu_footprint.py).

A kernel's contract (include/charpt.h, "memory footprint") is about bytes: it writes only the listed
elements of its outputs and the stated bytes of its workspace, reads nothing outside the logical
extent of its inputs that can change the result, leaves const operands alone and does not care
what its outputs and workspace held on entry.  A tightly packed tensor in an exactly sized
allocation cannot show a violation of any of these; a Box can.

    [ front guard | rows x ld body (cols owned per row, ld - cols padding) | back guard ]

Every byte of the allocation is prefilled with a poison pattern: a quiet NaN with a recognisable
payload for floating types (0x7FC5BEEF as fp32, 0x7FC5 as bf16: each is a NaN, and stays one when
converted to the other), a fixed out-of-range value for integer outputs, and for integer INPUTS
(token ids, targets, offsets) a caller-chosen valid index (`pad`), so an over-read can change the
answer but can never form a wild address.  Each guard holds at least 256 x ld elements plus 4 KiB,
so an overshoot by a whole 256-row tile (the largest in the library) lands inside the allocation
and is seen, not faulted on.

Not a conftest and no fixtures: plain helpers, device-agnostic (the CPU tests run them with torch
"kernels", the GPU tests with the library).
"""
import torch

GUARD_ROWS = 256
GUARD_EXTRA_BYTES = 4096
_ALIGN = 256     # the logical origin (before offset_bytes) sits on a multiple of this

_F32_NAN = 0x7FC5BEEF
_BF16_NAN = 0x7FC5
# little-endian byte patterns, 8 bytes each (every element size divides 8)
_POISON_BYTES = {
    torch.float32: _F32_NAN.to_bytes(4, "little") * 2,
    torch.bfloat16: _BF16_NAN.to_bytes(2, "little") * 4,
    torch.float64: (0x7FF8C5BEEFC5BEEF).to_bytes(8, "little"),
    torch.int64: (0x7BAD7BAD7BAD7BAD).to_bytes(8, "little"),     # far outside any index range
    torch.int32: (0x7BAD7BAD).to_bytes(4, "little") * 2,
    torch.uint8: _F32_NAN.to_bytes(4, "little") * 2,             # raw bytes: a NaN when read as floats
}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _round_up(x, m):
    return (x + m - 1) // m * m


class Box:
    """A logical [rows, cols] operand of `dtype` with row stride `ld` inside a poisoned allocation.

    ld            row stride in elements (default cols)
    offset_bytes  shifts the logical origin: a multiple of 16 keeps the kernels' fast paths, 4 or 8
                  exercises their alignment fallbacks (a multiple of the element size)
    pad           integer INPUT boxes: the valid index every byte outside (and inside, until fill())
                  holds instead of the out-of-range poison
    guard_bytes   overrides the guard size (WsBox)
    """

    def __init__(self, rows, cols, dtype, ld=None, offset_bytes=0, device="cpu", pad=None, guard_bytes=None):
        ld = cols if ld is None else ld
        if ld < cols or rows < 1 or cols < 1:
            raise ValueError(f"Box: rows {rows}, cols {cols}, ld {ld}")
        isz = torch.empty((), dtype=dtype).element_size()
        if offset_bytes < 0 or offset_bytes % isz:
            raise ValueError(f"Box: offset_bytes {offset_bytes} is no multiple of the element size {isz}")
        if pad is not None and dtype.is_floating_point:
            raise ValueError("Box: pad is for integer inputs")
        self.rows, self.cols, self.ld, self.dtype, self.device = rows, cols, ld, dtype, device
        self.offset_bytes = offset_bytes
        guard = GUARD_ROWS * ld * isz + GUARD_EXTRA_BYTES if guard_bytes is None else guard_bytes
        front = _round_up(guard, _ALIGN)
        total = _round_up(front + offset_bytes + rows * ld * isz + guard, 8)
        if pad is None:
            pattern = torch.tensor(list(_POISON_BYTES[dtype]), dtype=torch.uint8)
        else:
            pattern = torch.tensor([pad], dtype=dtype).view(torch.uint8).repeat(8 // isz)
        self._raw = pattern.repeat(total // 8).to(device)
        self._ref = self._raw.clone()                   # what every byte we do not own must still hold
        self._flat = self._raw.view(dtype)
        self._bits = self._raw.view(_INT_VIEW[isz])
        self._ref_bits = self._ref.view(_INT_VIEW[isz])
        self.origin = (front + offset_bytes) // isz     # element index of logical (0, 0)
        self.view = torch.as_strided(self._flat, (rows, cols), (ld, 1), self.origin)
        self._bits_view = torch.as_strided(self._bits, (rows, cols), (ld, 1), self.origin)
        owned = torch.zeros(self._flat.numel(), dtype=torch.bool, device=device)
        torch.as_strided(owned, (rows, cols), (ld, 1), self.origin).fill_(True)
        self._owned = owned
        self._snap = None

    # ---- contents -----------------------------------------------------------------------------
    def fill(self, t):
        """Copy the logical [rows, cols] (or, for rows == 1, [cols]) data in; returns self."""
        self.view.copy_(t.reshape(self.rows, self.cols).to(self.dtype))
        return self

    def prefill(self, how):
        """Set the OWNED elements to "nan" (the poison), "zero" or "ones" (0xFF bytes); returns self."""
        if how == "nan":
            self._bits_view.copy_(torch.as_strided(self._ref_bits, (self.rows, self.cols), (self.ld, 1), self.origin))
        elif how == "zero":
            self._bits_view.zero_()
        elif how == "ones":
            self._bits_view.fill_(-1 if self._bits.dtype != torch.uint8 else 255)
        else:
            raise ValueError(f"prefill {how!r}")
        return self

    def bits(self):
        """The logical elements' bits, as a dense integer tensor on the CPU (for bitwise comparisons)."""
        return self._bits_view.clone().cpu()

    # ---- checks -------------------------------------------------------------------------------
    def _where(self, flat_idx):
        e = flat_idx.cpu().to(torch.int64) - self.origin
        row = torch.div(e, self.ld, rounding_mode="floor")
        return torch.stack([row, e - row * self.ld], 1)

    def stray(self):
        """(row, col) of every element outside the owned ones whose bits differ from the poison: both
        guards and the ld - cols padding of every row.  Relative to the logical origin, so the front
        guard has negative rows and the padding has col >= cols.  An int64 [n, 2] tensor."""
        bad = (self._bits != self._ref_bits) & ~self._owned
        return self._where(bad.nonzero().flatten())

    def snapshot(self):
        """Remember every byte of the allocation (const operands: call after fill())."""
        self._snap = self._raw.clone()
        return self

    def changed(self):
        """(row, col) of every element whose bytes differ from the snapshot."""
        if self._snap is None:
            raise RuntimeError("Box.changed() before snapshot()")
        bad = self._bits != self._snap.view(self._bits.dtype)
        return self._where(bad.nonzero().flatten())

    def unchanged(self):
        return self.changed().shape[0] == 0

    # ---- assertions with (row, col) messages -------------------------------------------------------
    @staticmethod
    def _fmt(where, limit=6):
        head = ", ".join(f"(row {int(r)}, col {int(c)})" for r, c in where[:limit].tolist())
        more = where.shape[0] - limit
        return head + (f" and {more} more" if more > 0 else "")

    def assert_clean(self, name="box"):
        w = self.stray()
        assert w.shape[0] == 0, (f"{name} [{self.rows} x {self.cols}, ld {self.ld}]: {w.shape[0]} element(s) written "
                                 f"outside the owned region at {self._fmt(w)}")

    def assert_unchanged(self, name="box"):
        w = self.changed()
        assert w.shape[0] == 0, (f"{name} [{self.rows} x {self.cols}, ld {self.ld}]: const operand modified at "
                                 f"{self._fmt(w)}")


class WsBox(Box):
    """A workspace of exactly `nbytes` bytes (what the library's *_workspace() returned) between NaN
    guards.  `prefill`: what the owned bytes hold on entry -- "nan", "zero" or "ones" (0xFF).  Offsets
    in messages are (0, byte)."""

    def __init__(self, nbytes, prefill="nan", device="cpu"):
        nbytes = int(nbytes)
        self.nbytes = nbytes
        guard = max(65536, min(nbytes, 1 << 20))
        super().__init__(1, max(nbytes, 1), torch.uint8, device=device, guard_bytes=guard)
        self._where = lambda flat_idx: torch.stack([torch.zeros_like(flat_idx.cpu()), flat_idx.cpu() - self.origin], 1)
        if nbytes == 0:      # nothing owned: the one placeholder byte belongs to the guard
            self._owned.zero_()
        else:
            self.prefill(prefill)
