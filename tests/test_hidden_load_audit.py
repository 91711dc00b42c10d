"""The hidden-load hazard, pinned on the product sources.

Kernels that issue register loads hipcc cannot see (common.h gload16 / gload4 / gload4s: inline-asm
global loads counted in the kernel's own `s_waitcnt vmcnt(N)`) are correct only while hipcc never
touches a destination register between the load and the wait that retires it.  The round-5
residual-prefetch trial produced wrong bits exactly that way (a copy of a loop-carried destination
register before the data landed, profiles/r5_gemm_resid_prefetch_trial.txt).  This test compiles
every product .hip that uses hidden loads to gfx950 assembly with the Makefile's flags and asserts
that tools/audit_hidden_loads.py finds no such instruction, and that the audit does flag the pattern
(positive controls).  CPU only: hipcc cross-compiles."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "replicatinggpt_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import audit_hidden_loads as audit_mod  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"


def _makefile():
    return open(os.path.join(CSRC, "Makefile")).read()


def _text_with_local_headers(src):
    """the source and the csrc headers it includes (the kernels may live in headers: attention_d64_ring.h, attention_d64_res.h)"""
    text = open(os.path.join(CSRC, src)).read()
    for h in re.findall(r'^#include "([^"]+)"', text, re.M):
        if os.path.exists(os.path.join(CSRC, h)) and not h.endswith("common.h"):
            text += open(os.path.join(CSRC, h)).read()
    return text


def _product_sources():
    mk = _makefile()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    return [s for s in srcs if re.search(r"\bgload(16|4|4s)\(", _text_with_local_headers(s))]


def _flags(src):
    """the Makefile's flags for this object: FLAGS plus the source's extras (XFLAGS_<stem>)"""
    mk = _makefile()
    flags = re.search(r"^FLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    m = re.search(r"^XFLAGS_" + re.escape(src.replace(".hip", "")) + r" := (.*)$", mk, re.M)
    return flags + (m.group(1).split() if m else [])


def test_hidden_load_sources_are_known():
    # the kernels with hidden loads today; a new user of gload* joins the audit below automatically
    assert "attention_d64.hip" in _product_sources()
    # and the audit compiles it as the product does (the Makefile's per-source extras are found)
    assert "-fno-honor-nans" in _flags("attention_d64.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("make") is None, reason="needs hipcc")
@pytest.mark.parametrize("src", _product_sources())
def test_product_kernels_have_no_hidden_load_hazard(src, tmp_path):
    out = tmp_path / (src + ".s")
    cmd = [HIPCC] + _flags(src) + ["--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", str(out)]
    subprocess.run(cmd, check=True, cwd=CSRC, capture_output=True, timeout=600)
    text = out.read_text()
    kernels = re.findall(r"^(_Z\S+):", text, re.M)
    hidden = len(re.findall(r";;#ASMSTART\n\s*global_load_dword(?:x4)? v", text))
    assert kernels and hidden > 0, "no hidden loads in the assembly: the audit would be vacuous"
    bad = audit_mod.audit(text)
    assert not bad, "\n".join(f"{k[:70]} line {ln}: {t} (v{r})" for k, ln, t, r in bad[:20])


def _kernel(name, body):
    return f"{name}:\n" + "\n".join("\t" + ln if not ln.startswith(".L") else ln for ln in body) + "\n.Lfunc_end_" + name + ":\n"


def _hidden(reg):
    return [";;#ASMSTART", f"global_load_dword {reg}, v[4:5], off", ";;#ASMEND"]


def _wait(n):
    return [";;#ASMSTART", f"s_waitcnt vmcnt({n})", ";;#ASMEND"]


def _dma():
    return [";;#ASMSTART", "global_load_lds_dwordx4 v1, s[0:1]", ";;#ASMEND"]


def test_audit_flags_copy_before_wait():
    k = _kernel("_Zcopy", _hidden("v3") + ["v_mov_b32_e32 v7, v3"] + _wait(0) + ["s_endpgm"])
    bad = audit_mod.audit(k)
    assert len(bad) == 1 and bad[0][3] == 3


def test_audit_flags_copy_round_a_loop_back_edge():
    # the next iteration's word loaded at the end of the body, copied at the loop head before the wait
    body = _hidden("v3") + [".LBB1_1:", "v_mov_b32_e32 v7, v3"] + _wait(0) + ["v_add_u32_e32 v8, v7, v8"] + \
        _hidden("v3") + ["s_cbranch_scc1 .LBB1_1", "s_endpgm"]
    bad = audit_mod.audit(_kernel("_Zloop", body))
    assert [b[2] for b in bad] == ["v_mov_b32_e32 v7, v3"]


def test_audit_counts_vmcnt_in_issue_order():
    use = ["v_add_u32_e32 v8, v3, v8", "s_endpgm"]
    ok = audit_mod.audit(_kernel("_Zok", _hidden("v3") + _dma() + _dma() + _wait(2) + use))
    short = audit_mod.audit(_kernel("_Zshort", _hidden("v3") + _dma() + _dma() + _wait(3) + use))
    assert ok == [] and len(short) == 1
