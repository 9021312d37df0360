"""Device sample-rate conversion (csrc/resample.hip, wm_resample): the kernel against the f64 definition
(vlog_amd.audio.resample_host), bit-invariance under any split of the outputs and of the source span, the argument
errors, the streaming ingest of 48 kHz stereo s16le, and files that are not 16 kHz through the transcribe surfaces."""
import ctypes as C
import os
import threading
import wave

import numpy as np
import pytest
import torch
from scipy.signal import resample_poly

from vlog_amd.audio import downmix, resample_host, resample_plan, resample_taps, speech_like

pytestmark = pytest.mark.gpu

N_OUTS = (0, 1, 5, 255, 256, 257, 1023, 1025, 4097)


@pytest.fixture(scope="module")
def model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cuda", eot_after=60)


def _frames(n, ch, seed, f32=False):
    """Seeded full-scale int16 noise mixed with speech_like, per channel."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(n, ch)).astype(np.int64)
    for c in range(ch):
        s = np.round(speech_like(max(n / 16000.0, 0.01), seed + c)[:n] * 32768).astype(np.int64)
        x[: s.size, c] = (x[: s.size, c] + s) // 2
    x = np.clip(x, -32768, 32767).astype(np.int16)
    return (x.astype(np.float32) / 32768.0) if f32 else x


def _length_for(n_out, up, down):
    """A source length whose output count is n_out (where up > down not every count exists: the next one that does)."""
    for n in (n_out * down // up, -((-n_out * down) // up)):
        if -((-n * up) // down) == n_out:
            return n
    return -((-n_out * down) // up)


def _bound(mono, up, down, half):
    """Per output j: (K_j + 4) 2^-24 sum_i |h| |mono_i|, K_j the in-file terms of output j's sum."""
    h = np.abs(resample_taps(up, down))
    n = mono.size
    n_out = -((-n * up) // down)
    j = np.arange(n_out, dtype=np.int64)[:, None]
    a = j * down + half
    t = np.arange(2 * half // up + 1, dtype=np.int64)[None, :]
    i = a // up - t
    k = a % up + t * up
    ok = (k <= 2 * half) & (i >= 0) & (i < n)
    mag = np.where(ok, h[np.minimum(k, 2 * half)] * np.abs(mono)[np.clip(i, 0, n - 1)], 0.0).sum(axis=1)
    return (ok.sum(axis=1) + 4) * 2.0 ** -24 * mag


CASES = [(48000, 2, "s16", -1), (44100, 2, "s16", -1), (8000, 1, "s16", -1), (22050, 1, "f32", -1),
         (96000, 1, "s16", -1), (11025, 1, "s16", -1), (48000, 6, "s16", -1), (44100, 2, "s16", 1)]


@pytest.mark.parametrize("rate,ch,fmt,channel", CASES)
def test_kernel_against_the_definition(model, rate, ch, fmt, channel):
    eng = model.engine
    up, down, half = resample_plan(rate)
    assert eng.resample_plan(rate) == (up, down, half)
    for n_out in N_OUTS:
        n = _length_for(n_out, up, down)
        x = _frames(n, ch, 7 * rate + n_out, f32=fmt == "f32")
        y = eng.resample(x, rate, channel).cpu().numpy()
        ref64 = downmix(x, channel)
        want = -((-n * up) // down)
        assert want >= n_out and (want == n_out or up > down)
        assert y.dtype == np.float32 and y.shape == (want,)
        if want == 0:
            continue
        ref = resample_poly(ref64, up, down)
        assert np.array_equal(ref.astype(np.float32), resample_host(x, rate, channel))
        err = np.abs(y.astype(np.float64) - ref)
        bound = _bound(ref64, up, down, half)
        assert n_out < 255 or np.abs(ref).max() > 0.05
        print(f"rate {rate} ch {ch} {fmt} channel {channel} n_out {want}: worst err/bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound)


def _need(out0, n_out, up, down, half, n):
    """Source frames outputs [out0, out0 + n_out) read: (lo, hi clipped to the file, hi unclipped)."""
    lo = max(0, -((-(out0 * down - half)) // up))
    hi = ((out0 + n_out - 1) * down + half) // up
    return lo, min(hi, n - 1), hi


@pytest.mark.parametrize("rate,ch,fmt", [(44100, 2, "s16"), (48000, 2, "s16"), (8000, 1, "s16"), (22050, 1, "f32")])
def test_pieces_are_bit_identical_to_one_call(model, rate, ch, fmt):
    eng = model.engine
    up, down, half = resample_plan(rate)
    n = _length_for(6000, up, down) + 3
    x = torch.from_numpy(_frames(n, ch, rate + 1, f32=fmt == "f32")).cuda()
    whole = eng.resample(x, rate)
    n_out = whole.numel()
    rng = np.random.default_rng(rate)
    cuts = sorted(set([0, n_out, 1, 2047, 2048, 2049] + [int(c) for c in rng.integers(0, n_out, size=8)]))
    open_ended = 0
    for a, b in zip(cuts, cuts[1:]):
        lo, hi, hi_raw = _need(a, b - a, up, down, half, n)
        span = x[lo: hi + 1].contiguous()
        for n_total in (n, -1):
            if n_total < 0 and hi_raw > hi:
                continue                                   # reads past the end: needs the true length
            open_ended += n_total < 0
            piece = torch.full((b - a,), float("nan"), dtype=torch.float32, device="cuda")
            eng.resample_into(span, ch, rate, lo, n_total, a, b - a, piece)
            assert torch.equal(piece, whole[a:b]), (a, b, n_total)
    assert open_ended >= 3


def test_argument_errors_launch_nothing(model):
    eng = model.engine
    lib = eng.lib
    x = torch.from_numpy(_frames(4800, 2, 3)).cuda()
    out = torch.zeros(1600, dtype=torch.float32, device="cuda")

    def call(rate=48000, channels=2, channel=-1, src_offset=0, n_src=4800, n_total=4800, out0=0, n_out=1600, fmt=0):
        with torch.cuda.device(eng.device):
            rc = lib.wm_resample(eng.h, C.c_void_p(x.data_ptr()), fmt, channels, channel, rate, src_offset, n_src, n_total,
                                 out0, n_out, C.c_void_p(out.data_ptr()), eng.stream_ptr())
        return rc, lib.wm_last_error().decode()

    rc, msg = call(rate=44101)
    assert rc == -1 and "44101" in msg
    rc, msg = call(n_src=4000)                                  # the last outputs read frames past 4000
    assert rc == -1 and "source frames" in msg and "4000" in msg
    rc, msg = call(n_total=-1)                                  # end unknown: frames at or past the span's end are missing
    assert rc == -1 and "source frames" in msg
    rc, msg = call(src_offset=1, n_src=4799)                    # output 0 reads frame 0
    assert rc == -1 and "source frames" in msg
    rc, msg = call(channels=0)
    assert rc == -1 and "channels" in msg
    rc, msg = call(channel=2)
    assert rc == -1 and "channel" in msg
    rc, msg = call(n_out=1601)
    assert rc == -1 and "past the end of the output" in msg
    rc, msg = call(n_src=4801)
    assert rc == -1 and "past the end of the file" in msg
    rc, msg = call(n_out=-1)
    assert rc == -1 and "negative" in msg
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                        # nothing was launched
    assert call(n_out=0)[0] == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    rc, msg = call()
    assert rc == 0, msg
    assert torch.equal(out, eng.resample(x, 48000))


def _producer(fd, data: bytes, seed: int):
    rng = np.random.default_rng(seed)
    o = 0
    with os.fdopen(fd, "wb", buffering=0) as w:
        while o < len(data):
            n = int(rng.integers(1, 70000))
            w.write(data[o: o + n])
            o += n


@pytest.mark.parametrize("seconds", [12.7, 0.05])
def test_streamed_48k_stereo_bitexact(model, seconds):
    from vlog_amd.ingest import StreamingIngest
    eng = model.engine
    n = int(seconds * 48000)
    fr = _frames(n, 2, 31)
    r, w = os.pipe()
    t = threading.Thread(target=_producer, args=(w, fr.astype("<i2").tobytes(), 5))
    t.start()
    ing = StreamingIngest(eng, staging_samples=1 << 15, initial_capacity=16000, sample_rate=48000, channels=2)
    rng = np.random.default_rng(6)
    held = 0
    with os.fdopen(r, "rb", buffering=0) as f:
        while True:
            b = f.read(int(rng.integers(1, 50000)))
            if not b:
                break
            ing.feed(b)
            held = max(held, ing.n_in - ing.src0)
    t.join()
    res = ing.finish()
    up, down, half = resample_plan(48000)
    assert held <= 2 * half // up + 1
    assert res.n_samples == -((-n * up) // down) == res.pcm.numel()
    assert torch.equal(res.pcm, eng.resample(fr, 48000))
    ref = eng.features(res.pcm)
    assert res.features.shape == ref.shape and torch.equal(res.features, ref)


def _wav(path, frames: np.ndarray, rate: int):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(frames.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(frames.astype("<i2").tobytes())


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample")
    fr = np.stack([np.round(speech_like(35.0, 91, sr=48000) * 32768), np.round(speech_like(35.0, 92, sr=48000) * 16384)],
                  axis=1).astype(np.int16)
    _wav(d / "a48k.wav", fr, 48000)
    x16 = speech_like(31.0, 93, as_int16=True)
    _wav(d / "b16k.wav", x16[:, None], 16000)
    return str(d / "a48k.wav"), fr, str(d / "b16k.wav"), x16.astype(np.float32) / 32768.0


def _sig(segments):
    return [(s.tokens, s.start, s.end) for s in segments]


def test_transcribe_a_48k_stereo_file(model, clips):
    from vlog_amd.transcribe import BatchedInferencePipeline
    path48, fr, path16, x16 = clips
    audio = model.engine.resample(fr, 48000).cpu().numpy()
    assert audio.shape == (35 * 16000,)
    kw = dict(language="en", beam_size=1, temperature=0.0)
    a, ia = model.transcribe(path48, **kw)
    b, ib = model.transcribe(audio, **kw)
    a, b = _sig(a), _sig(b)
    assert a == b and len(a) >= 2
    assert ia.duration == audio.shape[0] / 16000 == ib.duration

    pipe = BatchedInferencePipeline(model, max_batch_windows=8)
    a, ia = pipe.transcribe(path48, **kw)
    b, ib = pipe.transcribe(audio, **kw)
    assert _sig(a) == _sig(b) and ia.duration == audio.shape[0] / 16000 == ib.duration

    for many in (model.transcribe_many, pipe.transcribe_many):
        got = many([path48, path16], **kw)
        want = many([audio, x16], **kw)
        assert len(got) == 2
        for (sa, fa), (sb, fb) in zip(got, want):
            assert _sig(sa) == _sig(sb) and fa.duration == fb.duration
        assert got[0][1].duration == audio.shape[0] / 16000
