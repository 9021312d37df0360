"""tools/attn_check: every decoder attention launcher (attn_dec.hip, attn_xenc.hip) in isolation against an f64
reference of the same operation on the same bf16 inputs, with forcing inputs (score staircases above and below the
deferred-rescale threshold, maxima in the ragged last tile, split maxima > 150 log2 units apart, mixed rows in one
wave), per-element tolerances counted from the kernels' rounding steps (tools/attn_check_ref.h), guards around every
buffer, sentinel-prefilled outputs / scratch / probabilities and memcmp checks of the bit-identity promises.  One case
per family; the program is built by __graft_entry__.build().

A family that ends by a signal, at its time limit or with status 2 (a HIP error) has left the GPU in an unknown state:
the remaining families then fail at once without starting the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["self", "cross_group", "cross_capture", "cross_tf", "xq", "xattn", "xcomb", "xchain"]
LIMIT = {"xattn": 180, "xcomb": 180}      # seconds per family (others: 120); each takes a few seconds
_stop = {}


@pytest.mark.parametrize("family", FAMILIES)
def test_attention_family_against_f64_reference(family):
    assert not _stop, f"not started: family {_stop.get('family')} ended with {_stop.get('how')}"
    exe = os.path.join(ROOT, "tools", "attn_check")
    # a missing program is a failure, not a skip: a skip would leave the whole family unchecked unnoticed
    assert os.path.exists(exe), "tools/attn_check is not built: make -C vlog_amd/csrc ../../tools/attn_check"
    try:
        r = subprocess.run([exe, family], capture_output=True, text=True, timeout=LIMIT.get(family, 120))
    except subprocess.TimeoutExpired:
        _stop.update(family=family, how="its time limit")
        raise
    if r.returncode < 0 or r.returncode == 2:
        _stop.update(family=family, how=f"status {r.returncode}")
    tail = r.stdout + r.stderr
    print(tail)
    assert r.returncode == 0, tail
    assert f"family {family}: ok" in r.stdout, tail
    assert "loose" not in r.stdout, tail
