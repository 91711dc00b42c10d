"""The one-pass prefill's host side: decode.prefill_plan on its edges, and the two new entry points in the
header and in the ctypes signatures (no GPU)."""
import ctypes

import pytest

from replicatinggpt_amd import _lib
from replicatinggpt_amd.decode import prefill_plan

T = 64


@pytest.mark.parametrize("pmin,want", [(1, 0), (2, 1), (3, 2), (T, T - 1), (T + 1, 0), (T + 9, 0)])
def test_plan_without_logprobs(pmin, want):
    """Pn = pmin - 1 positions, and only while the first decided column pmin is in phase 1 (pmin <= T): a
    batch whose every prompt is longer than the window runs phase 2 only."""
    assert prefill_plan(pmin, T, False, 1) == want


@pytest.mark.parametrize("pmin,want", [(1, 0), (2, 0), (3, 1), (T, T - 2), (T + 1, T - 1), (T + 9, T - 1)])
def test_plan_with_logprobs(pmin, want):
    """Pn = min(pmin - 1, T) - 1: one position short of the shortest prompt's last, so every scored column n
    <= Pn has n + 1 < pmin; never past the window's T - 1 cached positions."""
    Pn = prefill_plan(pmin, T, True, 1)
    assert Pn == want
    assert Pn == 0 or (Pn + 1 < pmin and Pn <= T - 1)


@pytest.mark.parametrize("logprobs", [False, True])
def test_plan_prefill_min(logprobs):
    pmin = 20
    Pn = prefill_plan(pmin, T, logprobs, 1)
    assert Pn == (18 if logprobs else 19)
    assert prefill_plan(pmin, T, logprobs, Pn) == Pn          # at the threshold: the pass runs
    assert prefill_plan(pmin, T, logprobs, Pn - 5) == Pn      # below it
    assert prefill_plan(pmin, T, logprobs, Pn + 1) == 0       # above it: the per-token steps stay
    assert prefill_plan(pmin, T, logprobs, 0) == Pn           # 0 is no threshold, and never a pass of 0 positions
    assert prefill_plan(1, T, logprobs, 0) == 0


def test_new_entry_points_are_declared():
    syms = _lib.header_symbols()
    for name, nargs in (("cg_decode_prefill_attn", 16), ("cg_decode_logprob_rows", 10)):
        assert name in syms, f"{name} is not in include/charpt.h"
        res, args = _lib._SIGS[name]
        assert res is ctypes.c_int and len(args) == nargs and args[-1] is ctypes.c_void_p
    header = open(_lib.HEADER_PATH).read()
    for name in ("cg_decode_prefill_attn", "cg_decode_logprob_rows"):
        decl = header[header.index(f"int {name}("):]
        decl = decl[:decl.index(";")]
        assert "stride_" in decl and "int64_t ld" not in decl, f"{name}: row strides are named stride_*"
