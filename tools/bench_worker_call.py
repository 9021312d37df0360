#!/usr/bin/env python3
"""Builder-run benchmark of the UNCHANGED worker's exact call (reference worker/transcription.py:81-85, 105-133):

    model = WhisperModel(WHISPER_MODEL, device="cpu", compute_type="int8")
    segments, info = model.transcribe(str(wav), language=None, task="transcribe", beam_size=5, vad_filter=True)
    for segment in segments: ...; text = " ".join(...); captions = generate_webvtt(...)

timed from the call to the VTT string, in the default sequential mode (faster-whisper seek loop) and in the
opt-in throughput mode (VLOG_AMD_THROUGHPUT=1 -> BatchedInferencePipeline).  Reports RTFx of each and the WER
of the throughput transcript against the sequential one on the same clip.  Synthetic large-v3 weights with the
margin-planted decoder program (decisive like a trained model: windows pass faster-whisper's thresholds at
temperature 0, so the default fallback ladder costs nothing extra); --random-weights: plain random init, whose
average log-probability (about -7) fails the -1.0 threshold on every window, so the fallback re-decodes every
window at five temperatures (best_of 5).  Prints one JSON line.
usage: python tools/bench_worker_call.py [--minutes-seq 5] [--minutes-tp 60] [--model large-v3]

--files 1,2,4,8,16,32: the sequential mode over several pending files instead (WhisperModel.transcribe_many, the
worker's call per file): for each N, N distinct clips of --minutes-seq minutes with N files in flight; one JSON line per
point with the RTFx summed over the files and the milliseconds per decoder pass of the shared first-pass decodes (wall
time inside engine.generate over its pass count); N = 1 is `transcribe` on one file.

--sections 1,2,4,8,16 [--sections-in-flight K]: the worker's call on ONE clip of --minutes-seq minutes with
transcribe(sections=N) (the file's sections decoded in lockstep); one JSON line per N with the sections the plan gave,
the wall times of --repeats calls (from the call to the VTT string), the RTFx of their median, and the decoder-pass
figures of --files.  N = 0 calls transcribe without the argument, so the same file measures a tree from before it.

--lockstep-fallback 0 | 1 | 0,1 (with --sections or --files): pass lockstep_fallback to the call (the fallback
temperatures of a lockstep round decoded alone, or by levels in one seeded generate per temperature).  "0,1" times both
at every point, alternated call by call inside the same process (--sections: --repeats calls of each), one JSON line per
flag.  Every line then also splits engine.generate's counters (wm_generate h_stats, per call) into the first passes
(temperature 0) and the fallback passes (temperature > 0): calls, decoder passes, rows per pass, ms per pass.  Without
the option the argument is not passed at all, so the same file measures a tree from before it.

--max-line-width W (with --sections): caption shaping (transcribe's max_line_width) off and on at every point,
alternated call by call inside the same process as the two --lockstep-fallback flags are: max_line_width=0, then
max_line_width=W with transcribe's defaults for the line count and the cue length; one JSON line per arm with
"max_line_width" 0 or W (the lines of profiles/worker_call_captions.jsonl).  Without the option the argument is not
passed at all.

--multilingual (with --sections): per-window language switching (transcribe's multilingual) off and on at every point,
alternated call by call inside the same process: multilingual=False, then multilingual=True; one JSON line per arm with
"multilingual" false or true.  After the last point the same clip is timed in throughput mode (VLOG_AMD_THROUGHPUT's
route), off and on alternated the same way, one JSON line per arm with "mode": "throughput" (the lines of
profiles/worker_call_multilingual.jsonl).  Without the option the argument is not passed at all.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vlog_amd.audio import speech_like, write_wav  # noqa: E402
from vlog_amd.metrics import word_error_rate  # noqa: E402
from vlog_amd.transcribe import WhisperModel  # noqa: E402
from vlog_amd.vtt import generate_webvtt  # noqa: E402


def worker_call(model, wav, temperature=None):
    """The worker's TranscriptionWorker.transcribe + generate_webvtt (worker/transcription.py:92-133, 377).
    temperature=None keeps faster-whisper's default fallback ladder (the worker's call as written)."""
    t = time.perf_counter()
    kw = {} if temperature is None else {"temperature": temperature}
    segments, info = model.transcribe(str(wav), language=None, task="transcribe", beam_size=5, vad_filter=True, **kw)
    segs, parts = [], []
    for s in segments:
        segs.append({"start": s.start, "end": s.end, "text": s.text})
        parts.append(s.text.strip())
    vtt = generate_webvtt(segs)
    return time.perf_counter() - t, " ".join(parts), info, len(segs), len(vtt)


def time_generate(eng):
    """Wraps eng.generate -> the dict that accumulates its wall seconds, decoder passes, row steps and calls."""
    acc = dict(ACC_ZERO)
    inner = eng.generate

    def timed_generate(*a, **kw):
        st = {}
        kw["stats"] = st
        t = time.perf_counter()
        r = inner(*a, **kw)
        dt = time.perf_counter() - t
        acc["s"] += dt
        acc["passes"] += st["passes"]
        acc["rows"] += st["row_steps"]
        acc["calls"] += 1
        if kw.get("temperature", 0.0) > 0:      # the fallback ladder's share (a sampled decode)
            acc["fb_s"] += dt
            acc["fb_passes"] += st["passes"]
            acc["fb_rows"] += st["row_steps"]
            acc["fb_calls"] += 1
        return r

    eng.generate = timed_generate
    return acc


ACC_ZERO = {"s": 0.0, "passes": 0, "rows": 0, "calls": 0, "fb_s": 0.0, "fb_passes": 0, "fb_rows": 0, "fb_calls": 0}


def split_stats(acc, per=1):
    """the first-pass / fallback split of time_generate's counters, per call of the measured function"""
    first = {k: acc[k] - acc["fb_" + k] for k in ("s", "passes", "rows", "calls")}
    out = {}
    for name, d in (("first", first), ("fallback", {k: acc["fb_" + k] for k in ("s", "passes", "rows", "calls")})):
        out[name] = {"generate_calls": d["calls"] // per, "decoder_passes": d["passes"] // per,
                     "rows_per_pass": round(d["rows"] / max(d["passes"], 1), 2),
                     "ms_per_decoder_pass": round(1e3 * d["s"] / max(d["passes"], 1), 4),
                     "generate_s": round(d["s"] / per, 3)}
    return out


def fallback_flags(args):
    """--lockstep-fallback -> the flags to time at every point ([None]: the argument is not passed)"""
    if args.lockstep_fallback is None:
        return [None]
    flags = [int(v) for v in args.lockstep_fallback.split(",")]
    if not flags or any(v not in (0, 1) for v in flags):
        raise SystemExit("--lockstep-fallback takes 0, 1 or 0,1")
    return flags


def sectioned(model, args, spec, tmp):
    counts = [int(v) for v in args.sections.split(",")]
    n_win = int(round(args.minutes_seq * 2))
    path = os.path.join(tmp, "long.wav")
    write_wav(path, np.concatenate([speech_like(30.0, i) for i in range(n_win)]))
    audio_s = n_win * 30.0
    acc = time_generate(model.engine)
    aligned = {"s": 0.0, "calls": 0, "groups": 0}       # engine.align_batch: the word alignment shaping turns on
    inner_align = model.engine.align_batch

    def timed_align(slots, *a, **kw):
        t = time.perf_counter()
        r = inner_align(slots, *a, **kw)
        aligned["s"] += time.perf_counter() - t
        aligned["calls"] += 1
        aligned["groups"] += len(slots)
        return r

    model.engine.align_batch = timed_align

    # the arms timed at every point: (lockstep_fallback, max_line_width, multilingual), None = the argument is not passed
    widths = [None] if args.max_line_width is None else [0, args.max_line_width]
    mls = [False, True] if args.multilingual else [None]
    flags = [(f, w, ml) for f in fallback_flags(args) for w in widths for ml in mls]

    def call(n, arm=(None, None, None)):
        flag, width, ml = arm
        kw = dict(language=None, task="transcribe", beam_size=5, vad_filter=True)
        if ml is not None:
            kw["multilingual"] = ml
        if args.temperature is not None:
            kw["temperature"] = args.temperature
        if flag is not None:
            kw["lockstep_fallback"] = bool(flag)
        if width is not None:
            kw["max_line_width"] = width
        if n > 0:
            kw["sections"] = n
            if args.sections_in_flight is not None:
                kw["sections_in_flight"] = args.sections_in_flight
        t = time.perf_counter()
        segments, info = model.transcribe(path, **kw)
        segs = [{"start": s.start, "end": s.end, "text": s.text} for s in segments]
        generate_webvtt(segs)
        dt = time.perf_counter() - t
        print(f"sections={n} lockstep_fallback={flag} max_line_width={width} multilingual={ml} "
              f"throughput={model.throughput}: {dt:.3f} s", file=sys.stderr, flush=True)             # progress
        return dt, info, len(segs)

    call(0)                                                        # warm-up (allocations, kernels)
    points = [(n, False) for n in counts] + ([(0, True)] if args.multilingual else [])
    for n, throughput in points:
        model.throughput = throughput                              # (the last point of --multilingual: throughput mode)
        for flag in flags:
            call(n, flag)                                          # (the slots and rows of this point)
        # the arms alternate call by call, so drift of the box lands on both; counters are kept per flag
        accs = {flag: dict(ACC_ZERO) for flag in flags}
        walls = {flag: [] for flag in flags}
        aligns = {flag: {"s": 0.0, "calls": 0, "groups": 0} for flag in flags}
        last = {}
        for _ in range(args.repeats):
            for flag in flags:
                acc.update(ACC_ZERO)
                aligned.update(s=0.0, calls=0, groups=0)
                dt, info, nseg = call(n, flag)
                for k in aligned:
                    aligns[flag][k] += aligned[k]
                walls[flag].append(dt)
                last[flag] = (info, nseg)
                for k in ACC_ZERO:
                    accs[flag][k] += acc[k]
        for flag in flags:
            info, nseg = last[flag]
            a = accs[flag]
            bounds = getattr(info.transcription_options, "section_frames", None)
            med = float(np.median(walls[flag]))
            line = {"model": args.model, "weights": spec, "mode": "throughput" if throughput else "sequential",
                    "sections": n if n > 0 else None,
                    "sections_planned": len(bounds) if bounds else 1,
                    "sections_in_flight": args.sections_in_flight, "audio_s": audio_s,
                    "duration_after_vad": round(info.duration_after_vad, 2),
                    "wall_s": [round(w, 3) for w in walls[flag]], "rtfx": round(audio_s / med, 2),
                    "rtfx_runs": [round(audio_s / w, 2) for w in walls[flag]], "segments": nseg,
                    "generate_calls": a["calls"] // args.repeats, "decoder_passes": a["passes"] // args.repeats,
                    "ms_per_decoder_pass": round(1e3 * a["s"] / max(a["passes"], 1), 4),
                    "rows_per_pass": round(a["rows"] / max(a["passes"], 1), 2)}
            if flag[0] is not None:
                line["lockstep_fallback"] = flag[0]
                line.update(split_stats(a, args.repeats))
            if flag[1] is not None:
                line["max_line_width"] = flag[1]
                line["word_timestamps"] = bool(info.transcription_options.word_timestamps)
                al = aligns[flag]
                line["align"] = {"calls": al["calls"] // args.repeats, "windows": al["groups"] // args.repeats,
                                 "s": round(al["s"] / args.repeats, 3),
                                 "ms_per_window": round(1e3 * al["s"] / max(al["groups"], 1), 3)}
            if flag[2] is not None:
                line["multilingual"] = flag[2]
                line["multilingual_in_force"] = bool(info.transcription_options.multilingual)
            print(json.dumps(line), flush=True)


def many_files(model, args, spec, tmp):
    counts = [int(v) for v in args.files.split(",")]
    n_win = int(round(args.minutes_seq * 2))
    paths = []
    for f in range(max(counts)):
        path = os.path.join(tmp, f"file{f}.wav")
        write_wav(path, np.concatenate([speech_like(30.0, 100 * f + i) for i in range(n_win)]))
        paths.append(path)
    audio_s = n_win * 30.0
    acc = time_generate(model.engine)
    kw = dict(language=None, task="transcribe", beam_size=5, vad_filter=True)
    if args.temperature is not None:
        kw["temperature"] = args.temperature
    list(model.transcribe(paths[0], **kw)[0])                      # warm-up
    for n in counts:
        for flag in fallback_flags(args):
            fkw = dict(kw) if flag is None else dict(kw, lockstep_fallback=bool(flag))
            acc.update(ACC_ZERO)
            t = time.perf_counter()
            if n == 1:
                nseg = len(list(model.transcribe(paths[0], **fkw)[0]))
            else:
                nseg = sum(len(s) for s, _ in model.transcribe_many(paths[:n], max_files=n, **fkw))
            dt = time.perf_counter() - t
            line = {"model": args.model, "weights": spec, "files_in_flight": n, "call": "transcribe" if n == 1 else
                    "transcribe_many", "audio_s_per_file": audio_s, "wall_s": round(dt, 3),
                    "rtfx_sum": round(n * audio_s / dt, 2), "segments": nseg, "generate_calls": acc["calls"],
                    "decoder_passes": acc["passes"], "ms_per_decoder_pass": round(1e3 * acc["s"] / max(acc["passes"], 1), 4),
                    "rows_per_pass": round(acc["rows"] / max(acc["passes"], 1), 2)}
            if flag is not None:
                line["lockstep_fallback"] = flag
                line.update(split_stats(acc))
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--minutes-seq", type=float, default=5.0)
    ap.add_argument("--minutes-tp", type=float, default=60.0)
    ap.add_argument("--temperature", type=float, default=None,
                    help="fixed temperature (e.g. 0: no fallback ladder, the cost of the call on a model whose windows "
                         "pass faster-whisper's thresholds); default: the worker's call as written")
    ap.add_argument("--random-weights", action="store_true",
                    help="plain random-init weights (every window fails the log-prob threshold and is re-decoded at "
                         "five temperatures); default: the margin-planted model, whose windows pass like a trained one")
    ap.add_argument("--no-graph", action="store_true", help="decode steps launched eagerly (decode_graph=0)")
    ap.add_argument("--files", default=None,
                    help="comma-separated numbers of files in flight: measure transcribe_many instead (module docstring)")
    ap.add_argument("--sections", default=None,
                    help="comma-separated section counts: measure transcribe(sections=N) on one clip (module docstring); "
                         "0 = the call without the argument")
    ap.add_argument("--sections-in-flight", type=int, default=None,
                    help="sections decoded per round (default: all; 1 = one after another, the A/B baseline)")
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per --sections point")
    ap.add_argument("--lockstep-fallback", default=None,
                    help="0, 1 or 0,1: the lockstep_fallback argument at every --sections / --files point (module "
                         "docstring); default: the argument is not passed")
    ap.add_argument("--max-line-width", type=int, default=None,
                    help="with --sections: time caption shaping off (max_line_width=0) and on (this width) at every "
                         "point, alternated call by call (module docstring); default: the argument is not passed")
    ap.add_argument("--multilingual", action="store_true",
                    help="with --sections: time multilingual off and on at every point and, last, in throughput mode on "
                         "the same clip, alternated call by call (module docstring)")
    args = ap.parse_args()
    if args.multilingual and not args.sections:
        raise SystemExit("--multilingual goes with --sections")
    if args.max_line_width is not None and (not args.sections or args.max_line_width < 1):
        raise SystemExit("--max-line-width takes a width >= 1 and goes with --sections")
    spec = f"synthetic:{args.model}:0" + ("" if args.random_weights else ":margin")
    model = WhisperModel(spec, device="cpu", compute_type="int8", eot_after=110)
    if args.no_graph:
        model.engine.set_option("decode_graph", 0)
    tmp = tempfile.mkdtemp()
    if args.files:
        return many_files(model, args, spec, tmp)
    if args.sections:
        return sectioned(model, args, spec, tmp)

    def clip(minutes, name):
        n = int(round(minutes * 2))
        path = os.path.join(tmp, name)
        write_wav(path, np.concatenate([speech_like(30.0, i) for i in range(n)]))
        return path, n * 30.0

    short, short_s = clip(args.minutes_seq, "short.wav")
    long_, long_s = clip(args.minutes_tp, "long.wav")
    out = {"model": args.model, "weights": spec, "decode_graph": not args.no_graph, "call": "transcribe(str(wav), language=None, task='transcribe', beam_size=5, "
                                        "vad_filter=True) + generate_webvtt"}
    T = args.temperature
    if T is not None:
        out["temperature"] = T
    model.throughput = True
    worker_call(model, short, T)                                   # warm-up (allocations, kernels)
    model.throughput = False
    dt, text_seq, info, nseg, _ = worker_call(model, short, T)
    out["sequential"] = {"audio_s": short_s, "wall_s": round(dt, 3), "rtfx": round(short_s / dt, 2), "segments": nseg,
                         "duration_after_vad": round(info.duration_after_vad, 2)}
    model.throughput = True
    dt, text_tp, info, nseg, _ = worker_call(model, short, T)
    out["throughput_same_clip"] = {"audio_s": short_s, "wall_s": round(dt, 3), "rtfx": round(short_s / dt, 2),
                                   "segments": nseg}
    out["wer_throughput_vs_sequential"] = round(word_error_rate(text_seq, text_tp), 4)
    dt, _, info, nseg, _ = worker_call(model, long_, T)
    out["throughput"] = {"audio_s": long_s, "wall_s": round(dt, 3), "rtfx": round(long_s / dt, 2), "segments": nseg,
                         "duration_after_vad": round(info.duration_after_vad, 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
