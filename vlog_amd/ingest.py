"""Streaming ingest: s16le PCM from a pipe straight into device memory, log-mel computed
while the audio is still arriving.

The reference worker extracts audio with ffmpeg into a temporary WAV file and faster-whisper then reads and
decodes that file (reference worker/transcription.py:259-299, 342-351).  Here the bytes of
`ffmpeg ... -f s16le -ac 1 -ar 16000 -` (or any producer of 16 kHz mono s16le) are read from the pipe into
pinned host staging buffers, copied to the device asynchronously (double-buffered: the next read overlaps the
previous copy), converted on the device (`wm_pcm_from_s16`), and every log-mel frame whose 400-sample window
lies inside the samples received so far is computed right away (`wm_logmel` on that frame range).  At EOF the
remaining frames (those touching the end padding) are computed with the true length and the whole matrix is
normalised with the file's global max (`wm_logmel_finalize`), exactly as the one-shot path does — so the
features are bit-identical to `engine.features(pcm)` (tests/test_gpu_ingest.py).

A producer may instead hand over the source's own format (`sample_rate`, `channels`: e.g. `ffmpeg ... -f s16le
-ac 2 -ar 48000 -`), so that ffmpeg neither downmixes nor resamples: the interleaved frames go to the device as they
arrive, every 16 kHz sample whose source span is complete is produced there (`wm_resample`, the kernel's output does
not depend on how the file is cut), and only the few source frames later samples still read are retained
(`audio.stream_plan`).  The PCM is bit-identical to `engine.resample(whole file)` (tests/test_gpu_resample.py).
"""
from __future__ import annotations

import ctypes as C
import shutil
import subprocess
from dataclasses import dataclass
from typing import BinaryIO, List, Optional

import numpy as np
import torch

from . import _capi
from .audio import SR as SAMPLE_RATE, stream_plan

HOP_LENGTH = 160

N_FFT = 400


@dataclass
class IngestResult:
    pcm: torch.Tensor          # f32 [n] on the device
    features: torch.Tensor     # finalised log-mel [n_mels, n // 160 + 1] on the device
    n_samples: int

    @property
    def duration(self) -> float:
        return self.n_samples / SAMPLE_RATE


class StreamingIngest:
    """sample_rate / channels: the format of the s16le stream.  The defaults (16 kHz mono) are the worker's ffmpeg
    extraction and convert with wm_pcm_from_s16; any other format is interleaved frames at the source rate, downmixed
    and resampled on the device (wm_resample) as the stream arrives."""

    def __init__(self, engine, staging_samples: int = 1 << 20, initial_capacity: int = SAMPLE_RATE * 600,
                 sample_rate: int = SAMPLE_RATE, channels: int = 1):
        self.eng = engine
        self.dev = engine.device
        self.stage = [torch.empty(staging_samples, dtype=torch.int16, pin_memory=True) for _ in range(2)]
        self.stage_ev: List[Optional[torch.cuda.Event]] = [None, None]
        self.pcm = torch.empty(max(initial_capacity, 1), dtype=torch.float32, device=self.dev)
        self.n = 0                       # 16 kHz samples in self.pcm
        self.done = 0                    # log-mel frames computed
        self.mels: List[torch.Tensor] = []
        self.gmax = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._carry = b""                # a partial trailing frame between reads (the odd byte of a mono stream)
        self._k = 0
        self.rate, self.ch = int(sample_rate), int(channels)
        self.native = self.rate == SAMPLE_RATE and self.ch == 1
        if self.native:
            self.stage_dev = torch.empty(staging_samples, dtype=torch.int16, device=self.dev)
        else:
            if not 1 <= self.ch <= 8:
                raise ValueError(f"channels {channels} (1 .. 8)")
            if staging_samples < self.ch:
                raise ValueError("staging_samples smaller than one frame")
            self.up, self.down, self.half = engine.resample_plan(self.rate)
            self.n_in = 0                # source frames received
            self.src0 = 0                # the first source frame still held: self.src holds frames [src0, n_in)
            self.src = torch.empty(max(staging_samples, 1), dtype=torch.int16, device=self.dev)

    # -- device PCM
    def _reserve(self, n: int) -> None:
        if n <= self.pcm.numel():
            return
        cap = self.pcm.numel()
        while cap < n:
            cap *= 2
        grown = torch.empty(cap, dtype=torch.float32, device=self.dev)
        grown[: self.n].copy_(self.pcm[: self.n])
        self.pcm = grown

    def feed(self, data) -> None:
        """Append s16le bytes (or an int16 array of whole frames)."""
        if isinstance(data, np.ndarray):
            samples = np.ascontiguousarray(data, dtype=np.int16).reshape(-1)
            if samples.size % self.ch:
                raise ValueError("an int16 array must hold whole frames")
        else:
            buf = self._carry + bytes(data)
            cut = len(buf) - len(buf) % (2 * self.ch)
            self._carry = buf[cut:]
            samples = np.frombuffer(buf[:cut], dtype=np.int16)
        cap = self.stage[0].numel() // self.ch * self.ch
        for o in range(0, samples.size, cap):
            self._push(samples[o: o + cap])
        self._frames(final=False)

    def _push(self, s: np.ndarray) -> None:
        k = self._k
        self._k ^= 1
        if self.stage_ev[k] is not None:
            self.stage_ev[k].synchronize()          # the copy out of this pinned buffer has finished
        m = s.size
        self.stage[k][:m].numpy()[:] = s
        if not self.native:
            self._push_frames(k, m)
            return
        self._reserve(self.n + m)
        st = torch.cuda.current_stream(self.dev)
        self.stage_dev[:m].copy_(self.stage[k][:m], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(st)
        self.stage_ev[k] = ev
        with torch.cuda.device(self.dev):
            _capi.check(self.eng.lib.wm_pcm_from_s16(self.eng.h, C.c_void_p(self.stage_dev.data_ptr()), m,
                                                     C.c_void_p(self.pcm.data_ptr() + 4 * self.n),
                                                     self.eng.stream_ptr()), "wm_pcm_from_s16")
        self.n += m

    def _push_frames(self, k: int, m: int) -> None:
        """m interleaved samples of staging buffer k: append them to the retained source frames on the device, then
        resample every output whose source span is now complete straight into self.pcm."""
        held = (self.n_in - self.src0) * self.ch
        if held + m > self.src.numel():
            grown = torch.empty(max(2 * self.src.numel(), held + m), dtype=torch.int16, device=self.dev)
            grown[:held].copy_(self.src[:held])
            self.src = grown
        self.src[held: held + m].copy_(self.stage[k][:m], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self.stage_ev[k] = ev
        self.n_in += m // self.ch
        self._resample(final=False)

    def _resample(self, final: bool) -> None:
        ready, keep = stream_plan(self.up, self.down, self.half, self.n_in, final)
        held = (self.n_in - self.src0) * self.ch
        if ready > self.n:
            self._reserve(ready)
            self.eng.resample_into(self.src[:held], self.ch, self.rate, self.src0, self.n_in if final else -1, self.n,
                                   ready - self.n, self.pcm[self.n:])
            self.n = ready
        if keep > self.src0:                 # drop the frames no later output reads (the tail is at most 2 half / up + 1)
            tail = self.src[(keep - self.src0) * self.ch: held].clone()
            self.src[: tail.numel()].copy_(tail)
            self.src0 = keep

    def _frames(self, final: bool) -> None:
        if final:
            ready = (self.n + HOP_LENGTH) // HOP_LENGTH          # N // 160 + 1 frames in all
        else:
            # frame f reads samples [160 f - 200, 160 f + 200): complete once 160 f + 200 <= n; frames are
            # transformed in (even, odd) pairs, so a chunk ends on an even frame (bit-identical to one shot)
            ready = max(0, (self.n - N_FFT // 2) // HOP_LENGTH + 1) if self.n >= N_FFT // 2 else 0
            ready &= ~1
        if ready <= self.done:
            return
        nf = ready - self.done
        mel = torch.empty((self.eng.dims.n_mels, nf), device=self.dev, dtype=torch.float32)
        with torch.cuda.device(self.dev):
            _capi.check(self.eng.lib.wm_logmel(self.eng.h, C.c_void_p(self.pcm.data_ptr()), 0, self.n, self.done, nf,
                                               C.c_void_p(mel.data_ptr()), nf, C.c_void_p(self.gmax.data_ptr()),
                                               self.eng.stream_ptr()), "wm_logmel")
        self.mels.append(mel)
        self.done = ready

    def finish(self) -> IngestResult:
        if self._carry:
            raise ValueError("odd number of bytes in an s16le stream" if self.native
                             else "the s16le stream ends inside a frame")
        if not self.native:
            self._resample(final=True)
        self._frames(final=True)
        mel = torch.cat(self.mels, dim=1) if len(self.mels) > 1 else self.mels[0]
        self.eng.logmel_finalize(mel, self.gmax)
        return IngestResult(self.pcm[: self.n], mel, self.n)


def ingest_pipe(engine, stream: BinaryIO, read_bytes: int = 1 << 20, sample_rate: int = SAMPLE_RATE,
                channels: int = 1) -> IngestResult:
    """Read s16le PCM (16 kHz mono, or interleaved frames of `channels` channels at `sample_rate` Hz) from `stream`
    (a pipe or file object) until EOF."""
    ing = StreamingIngest(engine, sample_rate=sample_rate, channels=channels)
    while True:
        b = stream.read(read_bytes)
        if not b:
            break
        ing.feed(b)
    return ing.finish()


def ffmpeg_pcm_command(path: str, sample_rate: int = SAMPLE_RATE, channels: int = 1) -> List[str]:
    """The extraction the worker runs, writing raw PCM to stdout instead of a temporary WAV.  A caller that knows
    the source's own rate and channel count passes them, so that ffmpeg converts nothing and the device does."""
    return ["ffmpeg", "-nostdin", "-loglevel", "error", "-i", path, "-vn", "-ac", str(int(channels)),
            "-ar", str(int(sample_rate)), "-f", "s16le", "-"]


def ingest_media(engine, path: str, sample_rate: int = SAMPLE_RATE, channels: int = 1) -> IngestResult:
    """ffmpeg -> pipe -> device.  Raises if ffmpeg is not installed (it is not in this build image; the
    tests drive ingest_pipe with a simulated s16le producer)."""
    exe = shutil.which("ffmpeg")
    if exe is None:
        raise RuntimeError("ffmpeg not found")
    with subprocess.Popen(ffmpeg_pcm_command(path, sample_rate, channels), stdout=subprocess.PIPE) as p:
        res = ingest_pipe(engine, p.stdout, sample_rate=sample_rate, channels=channels)
        if p.wait() != 0:
            raise RuntimeError(f"ffmpeg failed on {path}")
    return res
