#!/usr/bin/env python3
"""Selection-kernel time per decode step with a sequence-bias table set (wm_set_sequence_bias), read from the engine's
event profiler (class "select"): the flagship decode (large-v3 margin weights, --windows rows of the seeded corpus,
greedy with timestamps) once per table.

Tables: none (the instantiations without the rule), `phrases` (entries of 2 to 4 random text ids, so nearly all
inactive at a step: the match alone), and `ids` (length-1 entries with distinct ids, all active at every step: the
match, and per biased id the search and the sum).  Biases are +-0.5, far below the planted margins, so every run
decodes the same tokens (checked).  One JSON line per table.

  python tools/bench_sequence_bias.py [--model large-v3] [--windows 150] [--out profiles/sequence_bias_select.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vlog_amd.audio import speech_like  # noqa: E402
from vlog_amd.dims import model_dims  # noqa: E402
from vlog_amd.engine import GpuEngine  # noqa: E402
from vlog_amd.tokenizer import Tokenizer  # noqa: E402
from vlog_amd.weights import synthetic_state_dict  # noqa: E402


def tables(st, rng):
    text = lambda n: [int(t) for t in rng.integers(1000, st.eot, size=n)]
    out = [("none", [])]
    for n in (64, 1024):
        out.append((f"phrases{n}", [(tuple(text(int(rng.integers(2, 5)))), float(rng.choice([-0.5, 0.5]))) for _ in range(n)]))
    for n in (64, 1024):
        ids = rng.choice(np.arange(1000, st.eot), size=n, replace=False)
        out.append((f"ids{n}", [((int(t),), float(rng.choice([-0.5, 0.5]))) for t in ids]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--windows", type=int, default=150)
    ap.add_argument("--chunk", type=int, default=50, help="windows per log-mel / encoder call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = model_dims(a.model)
    st = dims.specials
    eng = GpuEngine(dims, synthetic_state_dict(dims, seed=0, plant="margin"), 0)
    tok = Tokenizer(dims, task="transcribe", language="en")
    W = a.windows
    eng.reserve(W, W)
    for w0 in range(0, W, a.chunk):
        n = min(a.chunk, W - w0)
        mel = eng.features(torch.from_numpy(np.concatenate([speech_like(30.0, w0 + i) for i in range(n)])))
        eng.cross_kv(eng.encode(mel, [3000 * i for i in range(n)], [3000] * n), w0)
        del mel
    prompt = [st.sot, st.lang_token("en"), st.transcribe]
    kw = dict(suppress_tokens=list(tok.suppressed_tokens([-1])), max_length=448)
    ref = None
    lines = []
    for name, table in tables(st, np.random.default_rng(0)):
        eng.generate(list(range(W)), [prompt] * W, sequence_bias=table, **kw)          # warm-up (graph capture)
        eng.profile(True, ["select"])
        res, steps = eng.generate(list(range(W)), [prompt] * W, sequence_bias=table, **kw)
        torch.cuda.synchronize()
        p = eng.profile_read()["select"]
        eng.profile(False)
        toks = [r.tokens for r in res]
        ref = toks if ref is None else ref
        line = dict(tool="bench_sequence_bias", model=a.model, rows=W, table=name, entries=len(table), steps=steps,
                    select_launches=p["launches"], select_ms=round(p["ms"], 4),
                    select_us_per_step=round(1e3 * p["ms"] / max(p["launches"], 1), 3), same_tokens=toks == ref)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
