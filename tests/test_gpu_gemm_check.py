"""tools/gemm_check: every bf16 GEMM entry point engine.cpp reaches (gemm.hip, gemm_8p.hip, gemm_big.hip,
gemm_dec.hip) in isolation against an f64 reference of the same operation, at the row / column / K edges of each
route, with per-element tolerances derived from the reference (tools/gemm_check_ref.h), canary guards around every
buffer, sentinel-prefilled outputs (K/V caches, ldc pads, split-K scratch) and memcmp checks of the bit-identity
promises of gemm.h.  One case per family; the program is built by __graft_entry__.build()."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["skinny", "tiled", "ring", "ring_big", "oneshot", "gemv", "p8", "big", "combine"]


@pytest.mark.parametrize("family", FAMILIES)
def test_gemm_family_against_f64_reference(family):
    exe = os.path.join(ROOT, "tools", "gemm_check")
    # a missing program is a failure, not a skip: a skip would leave the whole family unchecked unnoticed
    assert os.path.exists(exe), "tools/gemm_check is not built: make -C vlog_amd/csrc ../../tools/gemm_check"
    r = subprocess.run([exe, family], capture_output=True, text=True, timeout=300)
    tail = "\n".join(l for l in r.stdout.splitlines() if not l.startswith("  ok ")) + r.stderr
    print(tail)
    assert r.returncode == 0, tail
    assert f"family {family}: ok" in r.stdout, tail
