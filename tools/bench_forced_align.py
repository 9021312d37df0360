"""Per-window time of WhisperModel.align (forced alignment) on a synthetic model.

    python tools/bench_forced_align.py [--model large-v3] [--minutes 5] [--words 700]

A seeded clip of --minutes and a seeded text of --words words in lines of 12; model.align runs once to warm up and
once timed (wall clock around the whole call, which holds every synchronise), then once more with the engine's
event profiler on, for the time per kernel class.  Prints one JSON line: wall seconds, windows, ms per window, the
profiled classes in ms per window, and the rows offered / reached.  A synthetic model's attention is near uniform,
so the numbers say what a window costs, not where its words land."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlog_amd.audio import speech_like  # noqa: E402
from vlog_amd.transcribe import WhisperModel  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--words", type=int, default=700)
    a = ap.parse_args()
    model = WhisperModel(f"synthetic:{a.model}:0", device="cuda")
    n30 = int(np.ceil(a.minutes * 2))
    clip = np.concatenate([speech_like(30.0, 300 + i) for i in range(n30)])[: int(a.minutes * 60 * 16000)]
    rng = np.random.default_rng(1)
    ws = ["".join(rng.choice(list("abcdefghijklmnoprstu"), int(rng.integers(2, 9)))) for _ in range(a.words)]
    text = [" ".join(ws[i: i + 12]) for i in range(0, len(ws), 12)]
    out = {"bench": "forced_align", "model": a.model, "clip_s": len(clip) / 16000, "words": a.words}
    for rep in ("warmup", "timed", "profiled"):
        torch.cuda.synchronize()
        if rep == "profiled":
            model.engine.profile(True)
        t0 = time.perf_counter()
        segments, info = model.align(clip, text, language="en")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep == "timed":
            out.update(align_s=round(dt, 4), windows=info.windows, ms_per_window=round(1e3 * dt / max(info.windows, 1), 2),
                       unaligned_words=info.unaligned_words, segments=len(segments),
                       rows_offered=[r[1] for r in info.window_rows], rows_reached=[r[2] for r in info.window_rows])
        if rep == "profiled":
            model.engine.profile(False)
            out["profiled_s"] = round(dt, 4)
            out["classes_ms_per_window"] = {k: round(v["ms"] / max(info.windows, 1), 3)
                                            for k, v in model.engine.profile_read().items() if v["launches"]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
