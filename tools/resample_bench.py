"""Time of the device resampler (wm_resample, csrc/resample.hip) on one call over a whole file.

The representative shape is 1 h of 48 kHz stereo s16: 172.8 M frames in, 57.6 M samples out, 691 MB read and 230 MB
written.  Seeded int16 noise is generated on the device, the call is warmed up, and `--iters` launches are timed
with device events, one pair per launch.  Prints one JSON line: the median and the fastest launch, and the
algorithmic bytes (source read once + output written once) over the median time as GB/s and as a share of the 8 TB/s
HBM peak.  Fails without a GPU.

  python tools/resample_bench.py [--rate 48000] [--channels 2] [--seconds 3600] [--iters 30] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--f32", action="store_true", help="float32 frames instead of int16")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from vlog_amd.dims import model_dims
    from vlog_amd.engine import GpuEngine
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a GPU")
    eng = GpuEngine.frontend(model_dims("tiny"), 0)
    up, down, half = eng.resample_plan(a.rate)
    n = int(round(a.seconds * a.rate))
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randint(-32768, 32768, (n, a.channels), generator=g, device="cuda", dtype=torch.int16)
    if a.f32:
        x = x.float() / 32768.0
    n_out = -((-n * up) // down)
    out = torch.empty(n_out, dtype=torch.float32, device="cuda")
    for _ in range(a.warmup):
        eng.resample_into(x, a.channels, a.rate, 0, n, 0, n_out, out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.resample_into(x, a.channels, a.rate, 0, n, 0, n_out, out)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    med = ms[len(ms) // 2]
    nbytes = x.numel() * x.element_size() + n_out * 4
    line = json.dumps(dict(tool="resample_bench", rate=a.rate, channels=a.channels, fmt="f32" if a.f32 else "s16",
                           seconds=a.seconds, frames_in=n, samples_out=n_out, up=up, down=down, taps=2 * half + 1,
                           iters=a.iters, ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4),
                           bytes=nbytes, gbps=round(nbytes / med / 1e6, 1),
                           hbm_peak_share=round(nbytes / (med * 1e-3) / HBM_PEAK, 4),
                           checksum=float(out[:: max(1, n_out // 4096)].double().abs().sum().item()),
                           device=torch.cuda.get_device_name(0)))
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
