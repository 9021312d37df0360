"""tools/attn_kv8_check: the fp8 K/V panel instantiations of the projected form's cross-attention kernels (option
cross_kv_fp8) in isolation.  Panels are quantised by the device quantiser and dequantised on the host; every case runs
on the fp8 launcher and on the bf16 launcher over the dequantised panels.  (a) the fp8 launcher passes the bf16
family's f64 criterion with the same per-element tolerances (tools/attn_check_ref.h), the dequantised panels being the
inputs; (b) output, split partials and captured probabilities are memcmp-equal between the two launchers: required for
cross_tf (decode and teacher-forced), reported for the VALU kernels.  One case per family; the program is built by
__graft_entry__.build().

A family that ends by a signal, at its time limit or with status 2 (a HIP error) has left the GPU in an unknown state:
the remaining families then fail at once without starting the program."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["cross_tf", "cross_group", "cross_capture", "cross_dec"]
LIMIT = 120                                # seconds per family; each takes a few seconds
_stop = {}


@pytest.mark.parametrize("family", FAMILIES)
def test_fp8_panel_family(family):
    assert not _stop, f"not started: family {_stop.get('family')} ended with {_stop.get('how')}"
    exe = os.path.join(ROOT, "tools", "attn_kv8_check")
    # a missing program is a failure, not a skip: a skip would leave the whole family unchecked unnoticed
    assert os.path.exists(exe), "tools/attn_kv8_check is not built: make -C vlog_amd/csrc ../../tools/attn_kv8_check"
    try:
        r = subprocess.run([exe, family], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        _stop.update(family=family, how="its time limit")
        raise
    if r.returncode < 0 or r.returncode == 2:
        _stop.update(family=family, how=f"status {r.returncode}")
    tail = r.stdout + r.stderr
    print(tail)
    assert r.returncode == 0, tail
    assert f"family {family}: ok" in r.stdout, tail
    assert f"family {family}: bit identity with the bf16 launcher in" in r.stdout, tail
