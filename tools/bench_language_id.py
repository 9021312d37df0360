#!/usr/bin/env python3
"""Builder-run measurement of language identification: wm_detect_language (one decoder step, the full-vocabulary
logits GEMM into an [n][V] f32 buffer, then the language softmax) against wm_language_id (the same step, then the
language head on the last hidden state, no mask), on the same filled slots of one engine.

A large-v3 synthetic model; n = 1 and n = 150 rows; the two arms alternated call by call in one process, --calls (20)
calls each after --warmup (3) calls of each; every call ends in the engine's own stream synchronise, so a host clock
around it is the call's time.  Reports the median and the spread (min, max, 10th and 90th percentile) in
milliseconds, one JSON line per arm and n, printed and appended to profiles/language_id.jsonl.  It also prints the
largest |log p| difference between the arms over the languages with p >= 1e-4.  No sanitizer, no profiler counters.

usage: python tools/bench_language_id.py [--model large-v3] [--rows 1,150] [--calls 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vlog_amd.audio import speech_like  # noqa: E402
from vlog_amd.dims import model_dims  # noqa: E402
from vlog_amd.engine import GpuEngine  # noqa: E402
from vlog_amd.weights import synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--rows", default="1,150")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "language_id.jsonl"))
    a = ap.parse_args()
    rows = [int(v) for v in a.rows.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("bench_language_id needs the GPU: there is nothing to measure without it")
    dims = model_dims(a.model)
    st = dims.specials
    eng = GpuEngine(dims, synthetic_state_dict(dims, seed=3), 0)
    # four distinct encoded windows, repeated over the slots (the step's cost does not depend on what a slot holds)
    distinct = 4
    x = np.concatenate([speech_like(30.0, 200 + i) for i in range(distinct)])
    mel = eng.features(torch.from_numpy(x))
    enc = eng.encode(mel, [3000 * i for i in range(distinct)], [3000] * distinct)
    n_max = max(rows)
    eng.reserve(n_max, n_max)
    eng.cross_kv(enc.repeat((n_max + distinct - 1) // distinct, 1, 1)[:n_max].contiguous(), 0)
    arms = {
        "wm_detect_language": lambda s: eng.detect_language(s, st.lang_begin, st.n_langs),
        "wm_language_id": lambda s: eng.language_id(s, st.lang_begin, st.n_langs)[0],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for n in rows:
        slots = list(range(n))
        last = {}
        for _ in range(a.warmup):
            for name, fn in arms.items():
                last[name] = fn(slots)
        big = last["wm_detect_language"] >= 1e-4
        diff = float(np.abs(np.log(last["wm_language_id"][big].astype(np.float64)) -
                            np.log(last["wm_detect_language"][big].astype(np.float64))).max())
        same_top = bool((last["wm_language_id"].argmax(1) == last["wm_detect_language"].argmax(1)).all())
        times = {name: [] for name in arms}
        for _ in range(a.calls):
            for name, fn in arms.items():                    # alternated: both arms see the same drift
                t0 = time.perf_counter()
                fn(slots)
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name in arms:
            t = np.asarray(times[name])
            line = dict(tool="bench_language_id", model=a.model, arm=name, n=n, calls=a.calls, warmup=a.warmup,
                        median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4),
                        max_ms=round(float(t.max()), 4), p10_ms=round(float(np.percentile(t, 10)), 4),
                        p90_ms=round(float(np.percentile(t, 90)), 4), max_abs_dlogp=round(diff, 6), same_top=same_top)
            text = json.dumps(line)
            print(text, flush=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
