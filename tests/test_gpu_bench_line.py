"""The driver's contract for bench.py (one JSON line from rank 0): the keys the driver and the judge read, with the
values they check (config.workload must name the workload, roofline.traffic must say where it comes
from).  A tiny model on 8 windows, one timed step, so the line is produced in seconds; the headline itself is the
driver's own run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_schema_tiny():
    # --full: the roofline and parity blocks checked below are not part of a plain run
    d = _run("--model", "tiny", "--windows", "8", "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline",
             "--no-variable", "--parity-windows", "2")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 0 and d["value"] > 0
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "bf16"
    cfg = d["config"]
    # the descriptive workload is not overwritten by the corpus name (bench.py used to clobber it with "uniform")
    assert cfg["workload"].startswith("non-config variant: tiny bf16 greedy"), cfg["workload"]
    assert cfg["corpus"] == "uniform" and cfg["windows_per_gpu"] == 8
    roof = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof, k
    # no committed PMC file applies to this workload: traffic is null and carries no source label
    assert roof["traffic"] is None and "traffic_source" not in roof
    assert d["parity"]["n"] == 2


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run carries the headline keys and none of the --full blocks; --dump-outputs writes the last timed
    step's results as float .npy files that agree with the line (token counts, the token CRC)."""
    import zlib

    import numpy as np

    d = _run("--model", "tiny", "--windows", "8", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 8 * 30.0 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
    for k in ("parity", "cpu_baseline", "variable", "kernels_one_step", "encoder_mfma", "decoder_kv_read"):
        assert k not in d, k
    arrays = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in sorted(os.listdir(tmp_path))}
    assert set(arrays) == set(d["dumped_outputs"]) >= {"tokens", "token_counts", "scores", "segment_times",
                                                        "logmel_sample", "encoder_output_sample"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2**20
    assert all(np.isfinite(a).all() for a in arrays.values())
    tokens, counts = arrays["tokens"], arrays["token_counts"].astype(int)
    assert tokens.shape == (8, 448) and counts.tolist() == [int((row >= 0).sum()) for row in tokens]
    assert round(float(counts.mean()), 1) == d["config"]["mean_tokens_per_window"]
    crc = 0
    for row, n in zip(tokens, counts):
        crc = zlib.crc32(row[:n].astype(np.int32).tobytes(), crc)
    assert crc == d["config"]["token_crc32"]
    assert arrays["scores"].shape == (8, 3) and arrays["segment_times"].shape[1] == 2
