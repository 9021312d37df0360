"""tools/gemm_check_selftest (CPU only): the host-only reference and comparator of tools/gemm_check must flag each
planted kernel defect (two bf16 ulps, 4 E on an f32 element, a dropped K-tile, swapped K/V rows, a sentinel byte in
an ldc pad, a guard byte, a one-pass LayerNorm variance at offset 1000) and nothing else, and must pass an f32
recomputation in a shuffled summation order.  Built by __graft_entry__.build() with the host compiler."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gemm_check_reference_flags_planted_defects():
    exe = os.path.join(ROOT, "tools", "gemm_check_selftest")
    assert os.path.exists(exe), "tools/gemm_check_selftest is not built: make -C vlog_amd/csrc ../../tools/gemm_check_selftest"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "selftest ok" in r.stdout, r.stdout + r.stderr
    defects = [line for line in r.stdout.splitlines() if line.startswith("defect: ")]
    for defect in ("two ulps", "4 E", "dropped K-tile", "each other's slot", "ldc pad", "guard byte", "one-pass variance"):
        assert any(defect in line for line in defects), defect
