"""Audio input: RIFF/WAVE s16le reader (the worker's ffmpeg output format) and a seeded speech-like generator.

The worker extracts `pcm_s16le`, 16 kHz, mono WAV with ffmpeg (`worker/transcription.py:276-292`) and passes
the path to `transcribe` (`:105`); faster-whisper decodes it to float32 = int16 / 32768 [FW↑].  `load_audio`
does the same for WAV files (no ffmpeg/PyAV in this environment; other containers raise ValueError).  A WAV at
another rate, with any number of channels, is converted to 16 kHz mono by the definition further down
(`resample_host` on the host; `Engine.resample`, the same sum in f32, on the device).

`speech_like(seconds, seed)` is the BASELINE.md synthetic source: glottal pulse train 90-250 Hz with
jitter, 3 moving formants per 150-300 ms syllable, unvoiced noise bursts, pauses 0.2-3 s, RMS about
-26 dBFS, int16-quantised.  `numpy.random.default_rng(seed)`; corpora concatenate clips with seed = index.
"""
from __future__ import annotations

import io
import math
import struct
import wave
from typing import Tuple, Union

import numpy as np
from scipy.signal import lfilter, resample_poly

SR = 16000


def read_wav(src: Union[str, bytes, io.IOBase]):
    """WAV (PCM s16le/s32le/u8) -> (frames [n, ch], rate): int16 as stored for s16, float32 in [-1, 1) for s32 / u8."""
    if isinstance(src, (bytes, bytearray)):
        src = io.BytesIO(src)
    try:
        with wave.open(src, "rb") as w:
            ch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            raw = w.readframes(n)
    except (wave.Error, EOFError) as e:
        raise ValueError(f"unsupported audio container (only RIFF/WAVE PCM is decoded here): {e}") from None
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.int16, copy=False)
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise ValueError(f"unsupported sample width {width}")
    return x.reshape(-1, ch), rate


def mono_f32(frames: np.ndarray) -> np.ndarray:
    """The 16 kHz path of load_audio: float32 = int16 / 32768, channels averaged in float32."""
    x = frames.astype(np.float32) / 32768.0 if frames.dtype == np.int16 else frames
    x = x.mean(axis=1) if x.shape[1] > 1 else x.reshape(-1)
    return np.ascontiguousarray(x, dtype=np.float32)


def load_audio(src: Union[str, bytes, io.IOBase], sampling_rate: int = SR) -> np.ndarray:
    """WAV (PCM s16le/s32le/u8, mono or multi-channel, any rate) -> float32 mono at 16 kHz.  A 16 kHz file is
    int16 / 32768 (channels averaged), as faster-whisper's decode_audio gives it; any other rate goes through
    `resample_host` (the engine-less path; WhisperModel resamples on the device, Engine.resample)."""
    if sampling_rate != SR:
        raise ValueError(f"sampling_rate {sampling_rate}: the engine works at {SR} Hz")
    frames, rate = read_wav(src)
    if rate == SR:
        return mono_f32(frames)
    return resample_host(frames, rate)


# ---------------------------------------------------------------------------------------------------------------
# Sample-rate conversion to 16 kHz: the definition (f64).  The filter is scipy.signal.resample_poly's default.
#
#   g = gcd(16000, rate), up = 16000 / g, down = rate / g, m = max(up, down), half = 10 m, N = 2 half + 1 taps
#   h[k] = (1/m) sinc((k - half) / m) I0(5 sqrt(1 - ((k - half) / half)^2)) / I0(5),  sinc(x) = sin(pi x) / (pi x)
#   h /= sum(h);  h *= up                      (= scipy.signal.firwin(N, 1/m, window=("kaiser", 5.0)) * up)
#   mono[i] = mean of the channels of frame i (or one chosen channel); frames outside the file are zero
#   y[j] = sum_i mono[i] h[j down - i up + half]   over 0 <= i < n with the tap index in [0, 2 half]
#   n_out = ceil(n up / down); the output is not clipped.  rate == 16000 is the identity (up = down = 1, half = 0,
#   the single tap 1): downmix only.
#
# Output j reads frames ceil((j down - half) / up) .. floor((j down + half) / up).  The device kernel
# (csrc/resample.hip, wm_resample) evaluates the same sum in f32 with these taps rounded to f32; it supports
# N <= 16384 taps (max(up, down) <= 819), which covers 8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200,
# 96000, 176400 and 192000 Hz.
MAX_TAPS = 16384


def resample_plan(rate: int) -> Tuple[int, int, int]:
    """(up, down, half) of the conversion rate -> 16 kHz; ValueError for a rate the kernel does not support."""
    rate = int(rate)
    if rate <= 0:
        raise ValueError(f"unsupported sample rate {rate} Hz")
    g = math.gcd(SR, rate)
    up, down = SR // g, rate // g
    if up == 1 and down == 1:
        return 1, 1, 0
    half = 10 * max(up, down)
    if 2 * half + 1 > MAX_TAPS:
        raise ValueError(f"unsupported sample rate {rate} Hz: {SR}/{rate} = {up}/{down} needs {2 * half + 1} filter "
                         f"taps (at most {MAX_TAPS})")
    return up, down, half


def resample_taps(up: int, down: int) -> np.ndarray:
    """The float64 taps h[0 .. 2 half] of the definition above."""
    if up == 1 and down == 1:
        return np.ones(1, dtype=np.float64)
    m = max(up, down)
    half = 10 * m
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = (1.0 / m) * np.sinc(k / m) * np.i0(5.0 * np.sqrt(1.0 - (k / half) ** 2)) / np.i0(5.0)
    h /= h.sum()
    return h * up


def downmix(x: np.ndarray, channel: int = -1) -> np.ndarray:
    """[n] or [n, ch], int16 or float -> float64 mono: int16 / 32768; the mean of the channels, or channel `channel`."""
    x = np.asarray(x)
    scale = 1.0 / 32768.0 if x.dtype == np.int16 else 1.0
    x = x.astype(np.float64) * scale
    if x.ndim == 1:
        x = x[:, None]
    if channel >= x.shape[1] or channel < -1:
        raise ValueError(f"channel {channel} of {x.shape[1]}")
    return x.mean(axis=1) if channel < 0 else np.ascontiguousarray(x[:, channel])


def resample_host(x: np.ndarray, rate: int, channel: int = -1) -> np.ndarray:
    """The definition on the host: downmix, scipy.signal.resample_poly(mono, up, down) in float64, one rounding to
    float32.  -> float32 [ceil(n up / down)]"""
    up, down, _ = resample_plan(rate)
    mono = downmix(x, channel)
    if mono.size == 0 or (up == 1 and down == 1):
        return mono.astype(np.float32)
    return resample_poly(mono, up, down).astype(np.float32)


def resample_len(n: int, up: int, down: int) -> int:
    return -((-n * up) // down)


def stream_plan(up: int, down: int, half: int, n_in: int, final: bool) -> Tuple[int, int]:
    """Streaming resampler bookkeeping, for a stream of which frames [0, n_in) have arrived (`final`: it has ended).
    -> (ready, keep): outputs [0, ready) have their whole source span inside the frames received (all ceil(n_in up /
    down) of them once the stream has ended), and frames before `keep` are needed by no output >= ready, so the
    caller retains frames [keep, n_in) only: at most 2 half / up + 1 of them."""
    if final:
        return resample_len(n_in, up, down), n_in
    # output j reads up to frame floor((j down + half) / up): complete once j down + half < n_in up
    ready = max(0, -((-(n_in * up - half)) // down))
    keep = min(n_in, max(0, -((-(ready * down - half)) // up)))
    return ready, keep


def write_wav(path_or_buf, pcm: np.ndarray, sr: int = SR) -> None:
    x = np.asarray(pcm)
    if x.dtype != np.int16:
        x = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(path_or_buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(x.astype("<i2").tobytes())


def _resonator(f: float, bw: float, sr: int = SR):
    r = np.exp(-np.pi * bw / sr)
    th = 2 * np.pi * f / sr
    return [1.0 - r], [1.0, -2 * r * np.cos(th), r * r]


def speech_like(seconds: float, seed: int = 0, sr: int = SR, as_int16: bool = False) -> np.ndarray:
    rng = np.random.default_rng(seed)
    n_total = int(round(seconds * sr))
    out = np.zeros(n_total, dtype=np.float64)
    pos = int(rng.integers(0, int(0.3 * sr)))
    while pos < n_total:
        r = rng.random()
        if r < 0.12:                                 # pause (>= 2 s ones exercise VAD-style gaps)
            pos += int(rng.uniform(0.2, 3.0 if rng.random() < 0.3 else 0.8) * sr)
            continue
        dur = rng.uniform(0.15, 0.30)
        n = int(dur * sr)
        if pos + n > n_total:
            n = n_total - pos
        if n <= 16:
            break
        t = np.arange(n) / sr
        if rng.random() < 0.2:                       # unvoiced burst (fricative-like)
            nb = min(n, int(rng.uniform(0.05, 0.12) * sr))
            noise = rng.standard_normal(nb)
            b, a = _resonator(rng.uniform(3000, 6000), 1500)
            seg = lfilter(b, a, noise) * 0.3
            out[pos: pos + nb] += seg
            pos += nb + int(rng.uniform(0.01, 0.05) * sr)
            continue
        f0 = rng.uniform(90, 250)
        vib = 1 + 0.03 * np.sin(2 * np.pi * rng.uniform(3, 6) * t) + 0.01 * rng.standard_normal(n).cumsum() / np.sqrt(n)
        phase = np.cumsum(f0 * vib / sr)
        src = np.diff(np.floor(phase), prepend=0.0)          # one impulse per glottal period
        src = lfilter([1.0], [1.0, -0.95], src)               # glottal roll-off
        seg = np.zeros(n)
        for (lo, hi, bw) in ((300, 900, 80), (900, 2500, 120), (2400, 3500, 200)):
            fa, fb = rng.uniform(lo, hi), rng.uniform(lo, hi)
            k = 4
            edges = np.linspace(0, n, k + 1).astype(int)
            for j in range(k):                                  # piecewise-static moving formant
                fj = fa + (fb - fa) * (j + 0.5) / k
                b, a = _resonator(fj, bw)
                seg[edges[j]: edges[j + 1]] += lfilter(b, a, src[edges[j]: edges[j + 1]])
        env = np.sin(np.pi * np.linspace(0, 1, n)) ** 0.5
        out[pos: pos + n] += seg * env * rng.uniform(0.5, 1.0)
        pos += n + int(rng.uniform(0.0, 0.06) * sr)
    rms = np.sqrt(np.mean(out ** 2)) + 1e-12
    out *= (10 ** (-26 / 20)) / rms
    x16 = np.clip(np.round(out * 32768.0), -32768, 32767).astype(np.int16)
    return x16 if as_int16 else x16.astype(np.float32) / 32768.0


def room_tone(seconds: float, seed: int = 0, sr: int = SR, dbfs: float = -70.0, as_int16: bool = False) -> np.ndarray:
    """Silence as a recording has it: low-level pink-ish room noise at `dbfs` RMS (int16-quantised like
    speech_like), e.g. the gaps between the parts of a long-form programme."""
    rng = np.random.default_rng(10_000_019 + seed)
    n = int(round(seconds * sr))
    x = lfilter([1.0], [1.0, -0.9], rng.standard_normal(n))
    x *= (10 ** (dbfs / 20)) / (np.sqrt(np.mean(x ** 2)) + 1e-12)
    x16 = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    return x16 if as_int16 else x16.astype(np.float32) / 32768.0


QUIET_EVERY = 10


def long_form_window(i: int, seconds: float = 30.0) -> np.ndarray:
    """Window i of the variable-length corpus (bench.py --workload variable, the variable gates): speech_like(seed i),
    except every QUIET_EVERY-th window (i % QUIET_EVERY == QUIET_EVERY - 1) is room tone, so the corpus holds the
    near-empty windows (silence between programme parts) real long-form audio has."""
    if i % QUIET_EVERY == QUIET_EVERY - 1:
        return room_tone(seconds, i)
    return speech_like(seconds, i)


def corpus(n_clips: int, clip_seconds: float = 30.0, seed0: int = 0) -> np.ndarray:
    """Concatenation of n_clips speech-like clips with seeds seed0 .. seed0+n_clips-1 (float32)."""
    return np.concatenate([speech_like(clip_seconds, seed0 + i) for i in range(n_clips)])
