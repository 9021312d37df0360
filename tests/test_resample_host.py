"""Sample-rate conversion to 16 kHz, the host side (no GPU): the plan and the taps of the C-ABI against the f64
definition in vlog_amd/audio.py, resample_host against a direct double loop of the formula, the WAV loaders on files
that are not 16 kHz mono, the streaming bookkeeping, and the ffmpeg command."""
import ctypes as C
import io
import math
import os
import sys
import wave

import numpy as np
import pytest

from vlog_amd import _capi
from vlog_amd.audio import (load_audio, read_wav, resample_host, resample_plan, resample_taps, speech_like, stream_plan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


def _c_plan(lib, rate):
    up, down, half = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.wm_resample_plan(rate, C.byref(up), C.byref(down), C.byref(half))
    return rc, (up.value, down.value, half.value)


def test_plan_matches_the_library():
    lib = _capi.load()
    for rate in RATES:
        up, down, half = resample_plan(rate)
        g = math.gcd(16000, rate)
        assert (up, down, half) == (16000 // g, rate // g, 10 * max(16000 // g, rate // g))
        assert 2 * half + 1 <= 16384
        assert _c_plan(lib, rate) == (0, (up, down, half))
    assert resample_plan(16000)[:2] == (1, 1)
    rc, p = _c_plan(lib, 16000)
    assert rc == 0 and p[:2] == (1, 1) and p == resample_plan(16000)
    for bad in (44101, 0):
        with pytest.raises(ValueError, match=str(bad)):
            resample_plan(bad)
        assert _c_plan(lib, bad)[0] == -1
        assert str(bad).encode() in lib.wm_last_error()


@pytest.mark.parametrize("rate", RATES + (16000,))
def test_taps_match_the_definition(rate):
    lib = _capi.load()
    up, down, half = resample_plan(rate)
    h = resample_taps(up, down)
    assert h.dtype == np.float64 and h.shape == (2 * half + 1,)
    t32 = np.zeros(2 * half + 1, dtype=np.float32)
    assert lib.wm_resample_taps(rate, t32.ctypes.data_as(C.POINTER(C.c_float))) == 0
    err = np.abs(t32.astype(np.float64) - h)
    bound = 2.0 ** -24 * np.abs(h) + 2.0 ** -36 * np.abs(h).max()
    print(f"rate {rate}: worst err/bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)
    if rate != 16000:
        from scipy.signal import firwin
        assert np.abs(h - firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up).max() <= 1e-15 * up


def _noise16(n, seed, ch=1):
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(n, ch)).astype(np.int64)
    s = np.round(speech_like(max(n / 16000.0, 0.01), seed)[:n] * 32768).astype(np.int64)
    if s.size < n:
        s = np.pad(s, (0, n - s.size))
    return np.clip((x + s[:, None]) // 2, -32768, 32767).astype(np.int16)


def _direct(mono, up, down, half, h):
    """y[j] = sum_i mono[i] h[j down - i up + half]; also sum_i |mono[i]| |h[...]|."""
    n = mono.size
    n_out = -((-n * up) // down)
    y, mag = np.zeros(n_out), np.zeros(n_out)
    for j in range(n_out):
        for i in range(max(0, -((-(j * down - half)) // up)), min(n - 1, (j * down + half) // up) + 1):
            k = j * down - i * up + half
            y[j] += mono[i] * h[k]
            mag[j] += abs(mono[i] * h[k])
    return y, mag


@pytest.mark.parametrize("rate", [48000, 44100, 11025])
def test_resample_host_against_the_direct_sum(rate):
    up, down, half = resample_plan(rate)
    h = resample_taps(up, down)
    n = {48000: 3001, 44100: 2999, 11025: 3000}[rate]
    x = _noise16(n, rate)[:, 0]
    mono = x.astype(np.float64) / 32768.0
    assert np.abs(mono).max() > 0.5
    got = resample_host(x, rate)
    assert got.dtype == np.float32 and got.shape == (-((-n * up) // down),)
    ref, mag = _direct(mono, up, down, half, h)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"rate {rate}: n {n}, worst err/bound {float((err / (2.0 ** -23 * mag + 1e-300)).max()):.3f}")
    assert np.all(err <= 2.0 ** -23 * mag)
    for m in (0, 1, 7):
        small = resample_host(x[:m], rate)
        r2, g2 = _direct(mono[:m], up, down, half, h)
        assert small.shape == (-((-m * up) // down),)
        assert np.all(np.abs(small.astype(np.float64) - r2) <= 2.0 ** -23 * g2)


def _wav_bytes(frames: np.ndarray, rate: int) -> bytes:
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(frames.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(frames.astype("<i2").tobytes())
    return buf.getvalue()


def test_wav_loaders_and_overlay(tmp_path):
    fr = _noise16(4800, 5, ch=2)
    assert np.any(fr[:, 0] != fr[:, 1])
    path = tmp_path / "clip48k.wav"
    path.write_bytes(_wav_bytes(fr, 48000))
    frames, rate = read_wav(str(path))
    assert rate == 48000 and frames.dtype == np.int16 and np.array_equal(frames, fr)
    want = resample_host(fr, 48000)
    assert want.shape == (1600,)
    assert np.array_equal(load_audio(str(path)), want)
    assert np.array_equal(want, resample_host(fr.astype(np.float64).mean(axis=1) / 32768.0, 48000))

    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import faster_whisper
    finally:
        sys.path.pop(0)
    assert np.array_equal(faster_whisper.decode_audio(str(path)), want)
    left, right = faster_whisper.decode_audio(str(path), split_stereo=True)
    assert np.array_equal(left, resample_host(fr[:, 0], 48000)) and np.array_equal(right, resample_host(fr[:, 1], 48000))
    assert not np.array_equal(left, right)

    mono16 = _noise16(1000, 6)
    p16 = tmp_path / "clip16k.wav"
    p16.write_bytes(_wav_bytes(mono16, 16000))
    got = load_audio(str(p16))
    assert got.dtype == np.float32 and np.array_equal(got, mono16[:, 0].astype(np.float32) / 32768.0)
    with pytest.raises(ValueError):
        faster_whisper.decode_audio(str(p16), split_stereo=True)
    st16 = tmp_path / "stereo16k.wav"
    st16.write_bytes(_wav_bytes(fr, 16000))
    left, right = faster_whisper.decode_audio(str(st16), split_stereo=True)
    assert np.array_equal(left, fr[:, 0].astype(np.float32) / 32768.0)
    assert np.array_equal(right, fr[:, 1].astype(np.float32) / 32768.0)


@pytest.mark.parametrize("rate,ch", [(48000, 2), (44100, 2), (11025, 1), (8000, 1), (192000, 1)])
def test_stream_plan_tiles_the_output(rate, ch):
    up, down, half = resample_plan(rate)
    span = 2 * half // up + 2
    for seed in range(4):
        rng = np.random.default_rng(1000 * seed + rate)
        n = int(rng.integers(3 * span, 9 * span)) + seed
        total_bytes = n * 2 * ch
        # ragged reads in bytes: shorter than the filter span, exactly one frame, and ends inside a frame
        reads = [2 * ch, 2 * ch + 1, 2 * ch * max(1, span // 3)]
        o = sum(reads)
        while o < total_bytes:
            kind = int(rng.integers(0, 5))
            b = (2 * ch, 2 * ch * int(rng.integers(1, max(2, span // 3))) + 1, int(rng.integers(1, 2 * ch * 4 * span)),
                 2 * ch * int(rng.integers(span, 3 * span)), 1)[kind]
            reads.append(min(b, total_bytes - o))
            o += reads[-1]
        got_bytes = done = src0 = n_in = 0
        ranges = []
        for r in reads + [None]:
            final = r is None
            if not final:
                got_bytes += r
                chunk = got_bytes // (2 * ch) - n_in
                n_in += chunk
                assert n_in - src0 <= chunk + span                       # what is held while this chunk is processed
            ready, keep = stream_plan(up, down, half, n_in, final)
            assert ready >= done and src0 <= keep <= n_in
            if ready > done:
                lo = max(0, -((-(done * down - half)) // up))
                hi = ((ready - 1) * down + half) // up
                if final:
                    hi = min(hi, n_in - 1)
                assert src0 <= lo and hi < n_in
                ranges.append((done, ready))
                done = ready
            src0 = keep
            if not final:
                assert n_in - src0 <= 2 * half // up + 1
        assert n_in == n
        assert ranges[0][0] == 0 and ranges[-1][1] == -((-n * up) // down)
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


def test_stream_plan_short_streams():
    up, down, half = resample_plan(48000)
    assert stream_plan(up, down, half, 0, False) == (0, 0)
    assert stream_plan(up, down, half, 0, True) == (0, 0)
    assert stream_plan(up, down, half, half, False) == (0, 0)           # output 0 reads frame `half`
    assert stream_plan(up, down, half, half + 1, False)[0] == 1
    assert stream_plan(up, down, half, 1, True) == (1, 1)


def test_ffmpeg_command_carries_rate_and_channels():
    from vlog_amd.ingest import ffmpeg_pcm_command
    assert ffmpeg_pcm_command("a.mp4") == ["ffmpeg", "-nostdin", "-loglevel", "error", "-i", "a.mp4", "-vn", "-ac", "1",
                                           "-ar", "16000", "-f", "s16le", "-"]
    cmd = ffmpeg_pcm_command("a.mp4", 48000, 2)
    assert cmd[cmd.index("-ar") + 1] == "48000" and cmd[cmd.index("-ac") + 1] == "2"
    assert cmd[-3:] == ["-f", "s16le", "-"]
