"""tools/attn_check_selftest (CPU only): the host-only f64 reference, input generators and tolerances of
tools/attn_check.  Plain f32 emulations of the decoder attention algorithms (one-pass online softmax in 128 / 64-key
chunks with lane-group and wave merges; deferred-rescale tiles of 32 and 64 keys with bf16 P and bf16 u / l partials)
must pass on every generator at an error / tolerance ratio <= 0.5, each seeded fault (a rescale that skips l_run, that
leaves m_run, that uses another lane's maximum; unmasked ragged keys; a dropped or doubled key; a merge without m_s; an
identity lineage; row_pos without the +1; a finished row stored) must be rejected on the forcing inputs, the rescale
faults must pass unseen on the plain input, and the blocked-slot / xswap23 / partial-record layouts must round-trip."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attn_check_reference_flags_seeded_faults():
    exe = os.path.join(ROOT, "tools", "attn_check_selftest")
    if not os.path.exists(exe):      # host compiler only: no HIP needed
        subprocess.run(["make", "-C", os.path.join(ROOT, "vlog_amd", "csrc"), "../../tools/attn_check_selftest"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "selftest ok" in r.stdout, r.stdout + r.stderr
    emu = [line for line in r.stdout.splitlines() if line.startswith("emulation: ")]
    assert len(emu) == 3, emu
    for line in emu:
        assert float(re.search(r"worst error/tolerance ([0-9.]+)", line).group(1)) <= 0.5, line
    defects = [line for line in r.stdout.splitlines() if line.startswith("defect: ")]
    for defect in ("does not scale l_run", "leaves m_run unchanged", "another lane's mx", "ragged tile not masked",
                   "ragged chunk keys", "last key of a split dropped", "first key of a split read twice",
                   "merge ignores m_s", "lineage read as identity", "row_pos taken without the +1", "finished row stored"):
        hits = [line for line in defects if defect in line]
        assert hits, defect
        assert all("ACCEPTED" not in line for line in hits), hits
    for defect in ("does not scale l_run", "leaves m_run unchanged", "another lane's mx"):
        assert all("plain accepted" in line for line in defects if defect in line), defect
