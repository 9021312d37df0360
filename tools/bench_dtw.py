"""Time of the closed DTW (wm_dtw) of one library build, for the A/B of the open-end form's template.

    python tools/bench_dtw.py --lib PATH --label NAME [--reps 20] [--open]

Loads PATH with plain ctypes (a build from before wm_dtw_open has no such symbol, so vlog_amd._capi is not used),
creates an engine handle without weights, and times wm_dtw on seeded normal matrices of 225 x 750 and 120 x 1500:
warm-up calls first, then --reps calls, each a host clock around the call (which ends in a stream synchronise and
the path's copy back).  --open adds wm_dtw_open on the same matrices.  One JSON line per shape.  Run the two
builds alternately in one job and compare the medians against the spread between the runs of one build."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlog_amd._capi import ModelDimsC  # noqa: E402
from vlog_amd.dims import model_dims  # noqa: E402

SHAPES = [(225, 750), (120, 1500)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--label", required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--open", action="store_true")
    a = ap.parse_args()
    lib = C.CDLL(os.path.abspath(a.lib))
    vp, i32 = C.c_void_p, C.c_int32
    ip = C.POINTER(i32)
    lib.wm_create.argtypes = [C.POINTER(ModelDimsC), i32, C.POINTER(vp)]
    lib.wm_dtw.argtypes = [vp, vp, i32, i32, ip, ip, ip, vp]
    lib.wm_destroy.argtypes = [vp]
    lib.wm_destroy.restype = None
    if a.open:
        lib.wm_dtw_open.argtypes = [vp, vp, i32, i32, ip, ip, ip, ip, vp]
    dims = model_dims("tiny")
    st = dims.specials
    cd = ModelDimsC(dims.n_mels, dims.n_state, dims.n_head, dims.n_enc_layer, dims.n_dec_layer, dims.n_vocab,
                    dims.n_audio_ctx, dims.n_text_ctx, st.eot, st.sot, st.no_speech, st.no_timestamps,
                    st.timestamp_begin, st.blank)
    h = vp()
    if lib.wm_create(C.byref(cd), 0, C.byref(h)) != 0:
        raise RuntimeError("wm_create failed")
    stream = vp(torch.cuda.current_stream().cuda_stream)
    for N, M in SHAPES:
        x = torch.from_numpy(np.random.default_rng(N).standard_normal((N, M)).astype(np.float32)).cuda()
        ti = np.zeros(N + M + 2, np.int32)
        tj = np.zeros(N + M + 2, np.int32)
        n = np.zeros(1, np.int32)
        rows = np.zeros(1, np.int32)
        p = lambda v: v.ctypes.data_as(ip)  # noqa: E731

        def closed():
            if lib.wm_dtw(h, vp(x.data_ptr()), N, M, p(ti), p(tj), p(n), stream) != 0:
                raise RuntimeError("wm_dtw failed")

        def opened():
            if lib.wm_dtw_open(h, vp(x.data_ptr()), N, M, p(ti), p(tj), p(n), p(rows), stream) != 0:
                raise RuntimeError("wm_dtw_open failed")

        for name, fn in [("wm_dtw", closed)] + ([("wm_dtw_open", opened)] if a.open else []):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"bench": "dtw", "label": a.label, "call": name, "shape": [N, M], "reps": a.reps,
                              "median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4),
                              "max_ms": round(max(ts), 4), "path_len": int(n[0]),
                              "path_sum": int(ti[: n[0]].sum() + tj[: n[0]].sum())}), flush=True)
    lib.wm_destroy(h)


if __name__ == "__main__":
    main()
