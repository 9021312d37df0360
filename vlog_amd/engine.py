"""GPU engine wrapper: packs weights into the C-ABI layout and calls libwhisper_mi355 on one MI355X.

PyTorch-ROCm is plumbing here: it allocates the device buffers the C-ABI reads and writes and provides the
stream.  All arithmetic runs in the hand-written gfx950 kernels behind vlog_amd/_capi.py.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _capi
from .dims import ModelDims, N_FRAMES, HOP_LENGTH


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@dataclass
class GenResult:
    tokens: List[int]
    score: float
    cum_logprob: float
    no_speech_prob: float
    # per-step records (generate(record_logprobs=True)): log-prob of the token chosen at each step, the final
    # <|endoftext|> included when the window ended on it; greedy / sampling also the best other allowed token's
    token_logprobs: Optional[np.ndarray] = None
    token_logprobs_other: Optional[np.ndarray] = None


def pack_weights(dims: ModelDims, sd: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    """HF-named float32 weights -> the engine's packed names/layouts (include/whisper_mi355.h)."""
    d, m = dims.n_state, dims.n_mels
    k1p = ((3 * m + 63) // 64) * 64
    bf, f32 = torch.bfloat16, torch.float32
    out: Dict[str, torch.Tensor] = {}

    def g(n):
        return sd[n].to(device=device, dtype=f32)

    w1 = g("model.encoder.conv1.weight").permute(0, 2, 1).reshape(d, 3 * m)
    out["enc.conv1.w"] = torch.nn.functional.pad(w1, (0, k1p - 3 * m)).to(bf).contiguous()
    out["enc.conv1.b"] = g("model.encoder.conv1.bias")
    out["enc.conv2.w"] = g("model.encoder.conv2.weight").permute(0, 2, 1).reshape(d, 3 * d).to(bf).contiguous()
    out["enc.conv2.b"] = g("model.encoder.conv2.bias")
    out["enc.pos"] = g("model.encoder.embed_positions.weight")[: dims.n_audio_ctx].contiguous()
    zeros = torch.zeros(d, device=device, dtype=f32)

    def attn(dst, src):
        out[dst + "qkv.w"] = torch.cat([g(src + "q_proj.weight"), g(src + "k_proj.weight"), g(src + "v_proj.weight")]).to(bf).contiguous()
        out[dst + "qkv.b"] = torch.cat([g(src + "q_proj.bias"), zeros, g(src + "v_proj.bias")]).contiguous()
        out[dst + "out.w"] = g(src + "out_proj.weight").to(bf).contiguous()
        out[dst + "out.b"] = g(src + "out_proj.bias")

    def ln(dst, src):
        out[dst + ".w"] = g(src + ".weight")
        out[dst + ".b"] = g(src + ".bias")

    def mlp(dst, src):
        out[dst + "fc1.w"] = g(src + "fc1.weight").to(bf).contiguous()
        out[dst + "fc1.b"] = g(src + "fc1.bias")
        out[dst + "fc2.w"] = g(src + "fc2.weight").to(bf).contiguous()
        out[dst + "fc2.b"] = g(src + "fc2.bias")

    for l in range(dims.n_enc_layer):
        s, t = f"model.encoder.layers.{l}.", f"enc.{l}."
        attn(t, s + "self_attn.")
        ln(t + "ln1", s + "self_attn_layer_norm")
        ln(t + "ln2", s + "final_layer_norm")
        mlp(t, s)
    ln("enc.ln", "model.encoder.layer_norm")
    out["dec.embed"] = g("model.decoder.embed_tokens.weight").to(bf).contiguous()
    out["dec.pos"] = g("model.decoder.embed_positions.weight")[: dims.n_text_ctx].contiguous()
    ckv_w, ckv_b = [], []
    for l in range(dims.n_dec_layer):
        s, t = f"model.decoder.layers.{l}.", f"dec.{l}."
        attn(t, s + "self_attn.")
        ln(t + "ln1", s + "self_attn_layer_norm")
        ln(t + "ln2", s + "encoder_attn_layer_norm")
        ln(t + "ln3", s + "final_layer_norm")
        out[t + "cq.w"] = g(s + "encoder_attn.q_proj.weight").to(bf).contiguous()
        out[t + "cq.b"] = g(s + "encoder_attn.q_proj.bias")
        out[t + "cout.w"] = g(s + "encoder_attn.out_proj.weight").to(bf).contiguous()
        out[t + "cout.b"] = g(s + "encoder_attn.out_proj.bias")
        mlp(t, s)
        ckv_w += [g(s + "encoder_attn.k_proj.weight"), g(s + "encoder_attn.v_proj.weight")]
        ckv_b += [zeros, g(s + "encoder_attn.v_proj.bias")]
    out["dec.ckv.w"] = torch.cat(ckv_w).to(bf).contiguous()
    out["dec.ckv.b"] = torch.cat(ckv_b).contiguous()
    ln("dec.ln", "model.decoder.layer_norm")
    return out


class GpuEngine:
    """One engine per GPU process.  Thread-safe (the C-ABI serialises calls and sets the device itself)."""

    def __init__(self, dims: ModelDims, state_dict: Dict[str, torch.Tensor], device_index: int = 0):
        self.lib = _capi.load()
        self.dims = dims
        self.device = torch.device("cuda", device_index)
        st = dims.specials
        cd = _capi.ModelDimsC(dims.n_mels, dims.n_state, dims.n_head, dims.n_enc_layer, dims.n_dec_layer,
                              dims.n_vocab, dims.n_audio_ctx, dims.n_text_ctx, st.eot, st.sot, st.no_speech,
                              st.no_timestamps, st.timestamp_begin, st.blank)
        h = C.c_void_p()
        _capi.check(self.lib.wm_create(C.byref(cd), device_index, C.byref(h)), "wm_create")
        self.h = h
        self.n_slots = 0
        self.n_hyp = 0
        with torch.cuda.device(self.device):
            packed = pack_weights(dims, state_dict, self.device)
            s = self.stream_ptr()
            for name, t in packed.items():
                _capi.check(self.lib.wm_set_weight(self.h, name.encode(), C.c_void_p(t.data_ptr()),
                                                   t.numel() * t.element_size(), s), f"wm_set_weight({name})")
            torch.cuda.synchronize(self.device)
            del packed
        if not self.lib.wm_weights_complete(self.h):
            raise RuntimeError("engine weights incomplete")

    @classmethod
    def frontend(cls, dims: ModelDims, device_index: int = 0) -> "GpuEngine":
        """An engine handle with NO weights loaded, for the front end alone (log-mel, frame energy, VAD): a shard
        coordinator needs the features (and the global log-mel max) before any model pass.  wm_create builds the
        n_mels filterbank, so features() runs the same kernels as a full engine of these dims; the decoder and
        encoder entry points fail (wm_weights_complete is false)."""
        self = cls.__new__(cls)
        self.lib = _capi.load()
        self.dims = dims
        self.device = torch.device("cuda", device_index)
        st = dims.specials
        cd = _capi.ModelDimsC(dims.n_mels, dims.n_state, dims.n_head, dims.n_enc_layer, dims.n_dec_layer,
                              dims.n_vocab, dims.n_audio_ctx, dims.n_text_ctx, st.eot, st.sot, st.no_speech,
                              st.no_timestamps, st.timestamp_begin, st.blank)
        h = C.c_void_p()
        _capi.check(self.lib.wm_create(C.byref(cd), device_index, C.byref(h)), "wm_create")
        self.h = h
        self.n_slots = 0
        self.n_hyp = 0
        return self

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            try:
                self.lib.wm_destroy(h)
            except Exception:
                pass
            self.h = None

    def stream_ptr(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def profile(self, enable: bool, classes: Optional[Sequence[str]] = None) -> None:
        """Reset + enable the built-in event profiler (all classes, or only `classes`); False disables."""
        if not enable:
            _capi.check(self.lib.wm_profile_select(self.h, 0), "wm_profile_select")
            return
        if classes is None:
            _capi.check(self.lib.wm_profile(self.h, 1), "wm_profile")
            return
        names = [self.lib.wm_profile_name(c).decode() for c in range(self.lib.wm_profile_classes())]
        mask = 0
        for n in classes:
            mask |= 1 << names.index(n)
        _capi.check(self.lib.wm_profile_select(self.h, mask), "wm_profile_select")

    def profile_read(self) -> Dict[str, dict]:
        out = {}
        for c in range(self.lib.wm_profile_classes()):
            n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            _capi.check(self.lib.wm_profile_read(self.h, c, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)), "wm_profile_read")
            out[self.lib.wm_profile_name(c).decode()] = dict(launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value)
        return out

    def encoder_attention(self, qkv: torch.Tensor) -> torch.Tensor:
        """The encoder self-attention kernel alone: qkv bf16 [B, T, 3d] -> bf16 [B, T, d] (diagnostics/tests)."""
        B, T, three_d = qkv.shape
        if qkv.dtype != torch.bfloat16 or three_d != 3 * self.dims.n_state or not qkv.is_contiguous():
            raise ValueError("encoder_attention: qkv must be contiguous bf16 [B, T, 3 n_state]")
        out = torch.empty(B, T, self.dims.n_state, dtype=torch.bfloat16, device=self.device)
        _capi.check(self.lib.wm_encoder_attention(self.h, C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()),
                                                  B, T, self.stream_ptr()), "wm_encoder_attention")
        return out

    def cross_fp8_quantize(self, enc: torch.Tensor):
        """wm_cross_fp8_quantize on bf16 rows [..., n_state] -> (uint8 codes, f32 scale per row), device tensors."""
        x = enc.reshape(-1, enc.shape[-1]).contiguous()
        codes = torch.empty(x.shape, dtype=torch.uint8, device=self.device)
        scale = torch.empty(x.shape[0], dtype=torch.float32, device=self.device)
        _capi.check(self.lib.wm_cross_fp8_quantize(self.h, C.c_void_p(x.data_ptr()), x.shape[0],
                                                    C.c_void_p(codes.data_ptr()), C.c_void_p(scale.data_ptr()),
                                                    self.stream_ptr()), "wm_cross_fp8_quantize")
        return codes, scale

    def cross_kv_fp8_quantize(self, rows: torch.Tensor, codes: Optional[torch.Tensor] = None,
                              exps: Optional[torch.Tensor] = None):
        """wm_cross_kv_fp8_quantize on bf16 rows [..., 64] -> (uint8 codes [n][64], uint8 exponent bytes [n]), device
        tensors (the projected form's fp8 K/V panels, option cross_kv_fp8).  `codes` / `exps`: write into these
        (contiguous uint8 device tensors of n * 64 / n elements, e.g. views inside guarded buffers)."""
        if rows.dtype != torch.bfloat16 or rows.shape[-1] != 64:
            raise ValueError("cross_kv_fp8_quantize: rows of 64 bf16 values")
        x = rows.reshape(-1, 64).contiguous()
        n = x.shape[0]
        if codes is None:
            codes = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        if exps is None:
            exps = torch.empty(n, dtype=torch.uint8, device=self.device)
        if codes.numel() != n * 64 or exps.numel() != n or not codes.is_contiguous() or not exps.is_contiguous():
            raise ValueError("cross_kv_fp8_quantize: output sizes")
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_cross_kv_fp8_quantize(self.h, C.c_void_p(x.data_ptr()), n,
                                                          C.c_void_p(codes.data_ptr()), C.c_void_p(exps.data_ptr()),
                                                          self.stream_ptr()), "wm_cross_kv_fp8_quantize")
        return codes, exps

    def set_option(self, key: str, value: int) -> None:
        """Engine scheduling knob (wm_set_option), e.g. set_option("decode_split", 0)."""
        _capi.check(self.lib.wm_set_option(self.h, key.encode(), int(value)), "wm_set_option")

    def option(self, key: str, default: Optional[int] = None) -> Optional[int]:
        """The engine's current value of an option (wm_get_option: includes environment overrides and defaults);
        `default` only for keys the engine does not know."""
        v = C.c_int64()
        if self.lib.wm_get_option(self.h, key.encode(), C.byref(v)) != 0:
            if default is not None:
                return default
            _capi.check(-1, f"wm_get_option({key})")
        return int(v.value)

    def device_bytes(self) -> int:
        return int(self.lib.wm_device_bytes(self.h))

    # ------------------------------------------------------------------ log-mel
    def logmel(self, pcm: torch.Tensor, n_samples: Optional[int] = None, pcm_offset: int = 0, frame0: int = 0,
               n_frames: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Unclamped log10 mel of frames [frame0, frame0+n_frames) of a file of n_samples samples.
        -> (mel f32 [n_mels, n_frames] on device, gmax uint32 [1] ordered-max accumulator)."""
        if n_samples is None:
            n_samples = pcm.numel()
        if n_frames is None:
            n_frames = (n_samples + HOP_LENGTH) // HOP_LENGTH - frame0
        pcm = pcm.to(self.device, torch.float32).contiguous()
        mel = torch.empty((self.dims.n_mels, max(n_frames, 1)), device=self.device, dtype=torch.float32)
        gmax = torch.zeros(1, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_logmel(self.h, C.c_void_p(pcm.data_ptr()), pcm_offset, n_samples, frame0, n_frames,
                                           C.c_void_p(mel.data_ptr()), mel.shape[1], C.c_void_p(gmax.data_ptr()),
                                           self.stream_ptr()), "wm_logmel")
        return mel, gmax

    def logmel_finalize(self, mel: torch.Tensor, gmax: torch.Tensor, gmax_value: Optional[float] = None) -> float:
        hv = (C.c_float * 1)(gmax_value) if gmax_value is not None else None
        out = (C.c_float * 1)()
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_logmel_finalize(self.h, C.c_void_p(mel.data_ptr()), mel.shape[1], mel.shape[1],
                                                    C.c_void_p(gmax.data_ptr()),
                                                    C.cast(hv, C.POINTER(C.c_float)) if hv is not None else None,
                                                    C.cast(out, C.POINTER(C.c_float)), self.stream_ptr()),
                        "wm_logmel_finalize")
        return float(out[0])

    def gmax_value(self, gmax: torch.Tensor) -> float:
        u = int(gmax.cpu().view(torch.int32).numpy().astype(np.uint32)[0])
        u = (u & 0x7FFFFFFF) if (u & 0x80000000) else (~u & 0xFFFFFFFF)
        return float(np.array([u], dtype=np.uint32).view(np.float32)[0])

    def frame_energy_db(self, pcm: torch.Tensor, frame: int = 512) -> np.ndarray:
        pcm = pcm.to(self.device, torch.float32).contiguous()
        n = pcm.numel()
        out = torch.empty(max(1, (n + frame - 1) // frame), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_frame_energy(self.h, C.c_void_p(pcm.data_ptr()), n, frame, C.c_void_p(out.data_ptr()),
                                                 self.stream_ptr()), "wm_frame_energy")
        return out.cpu().numpy()[: (n + frame - 1) // frame]

    # ------------------------------------------------------------------ sample-rate conversion
    def resample_plan(self, rate: int) -> Tuple[int, int, int]:
        """wm_resample_plan: (up, down, half) of rate -> 16 kHz; RuntimeError for a rate the kernel does not support."""
        up, down, half = C.c_int32(), C.c_int32(), C.c_int32()
        _capi.check(self.lib.wm_resample_plan(int(rate), C.byref(up), C.byref(down), C.byref(half)), "wm_resample_plan")
        return up.value, down.value, half.value

    def resample_into(self, src: torch.Tensor, channels: int, rate: int, src_offset: int, n_total: int, out0: int,
                      n_out: int, dst: torch.Tensor, channel: int = -1) -> None:
        """wm_resample: outputs [out0, out0 + n_out) of the file into dst[:n_out]; `src` (contiguous device int16 or
        float32) holds frames [src_offset, src_offset + src.numel() // channels); n_total -1: end not yet known."""
        if src.dtype not in (torch.int16, torch.float32) or not src.is_contiguous() or src.device != self.device:
            raise ValueError("resample: contiguous int16 or float32 frames on the engine's device")
        if dst.dtype != torch.float32 or not dst.is_contiguous() or dst.numel() < n_out or dst.device != self.device:
            raise ValueError("resample: dst must be a contiguous float32 device tensor of >= n_out samples")
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_resample(self.h, C.c_void_p(src.data_ptr()), 0 if src.dtype == torch.int16 else 1,
                                             channels, channel, int(rate), src_offset, src.numel() // max(channels, 1),
                                             n_total, out0, n_out, C.c_void_p(dst.data_ptr()), self.stream_ptr()),
                        "wm_resample")

    def resample(self, frames, rate: int, channel: int = -1) -> torch.Tensor:
        """PCM frames [n] or [n, ch] (numpy or tensor, int16 or float32) at `rate` Hz -> f32 mono at 16 kHz on the
        device, [ceil(n up / down)]: the mean of the channels (or channel `channel`) through the polyphase filter of
        vlog_amd/audio.py (resample_host is the same definition in f64)."""
        if isinstance(frames, np.ndarray):
            frames = np.ascontiguousarray(frames)
            frames = torch.from_numpy(frames if frames.flags.writeable else frames.copy())
        x = frames
        if x.dim() == 1:
            x = x[:, None]
        if x.dim() != 2 or x.dtype not in (torch.int16, torch.float32):
            raise ValueError("resample: frames must be int16 or float32, [n] or [n, channels]")
        n, ch = x.shape
        x = x.to(self.device).contiguous()
        up, down, _ = self.resample_plan(rate)
        n_out = -((-n * up) // down)
        out = torch.empty(n_out, dtype=torch.float32, device=self.device)
        self.resample_into(x, ch, rate, 0, n, 0, n_out, out, channel)
        return out

    def features(self, pcm: torch.Tensor) -> torch.Tensor:
        """faster-whisper FeatureExtractor(audio): clamped log-mel [n_mels, N//160 + 1] on device."""
        mel, gmax = self.logmel(pcm)
        self.logmel_finalize(mel, gmax)
        return mel

    # ------------------------------------------------------------------ encoder / decoder
    def encode(self, mel: torch.Tensor, seeks: Sequence[int], nframes: Sequence[int]) -> torch.Tensor:
        B = len(seeks)
        s = np.ascontiguousarray(seeks, dtype=np.int32)
        n = np.ascontiguousarray(nframes, dtype=np.int32)
        enc = torch.empty((B, self.dims.n_audio_ctx, self.dims.n_state), device=self.device, dtype=torch.bfloat16)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_encode(self.h, C.c_void_p(mel.data_ptr()), mel.shape[1], _i32p(s), _i32p(n), B,
                                           C.c_void_p(enc.data_ptr()), self.stream_ptr()), "wm_encode")
        return enc

    def reserve(self, n_slots: int, n_hyp: int) -> None:
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_reserve(self.h, n_slots, n_hyp, self.stream_ptr()), "wm_reserve")
        self.n_slots = max(self.n_slots, n_slots)
        self.n_hyp = max(self.n_hyp, n_hyp)

    def cross_kv(self, enc: torch.Tensor, slot0: int = 0) -> None:
        B = enc.shape[0]
        if slot0 + B > self.n_slots:
            self.reserve(slot0 + B, max(self.n_hyp, 1))
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_cross_kv(self.h, C.c_void_p(enc.data_ptr()), B, slot0, self.stream_ptr()), "wm_cross_kv")

    def generate(self, slots: Sequence[int], prompts: Sequence[Sequence[int]], *, beam_size: int = 1,
                 patience: float = 1.0, length_penalty: float = 1.0, max_length: Union[int, Sequence[int]] = 448,
                 temperature: float = 0.0, num_hypotheses: int = 1, seed: int = 0,
                 suppress_tokens: Sequence[int] = (), suppress_blank: bool = True,
                 max_initial_timestamp_index: Optional[int] = 50, with_timestamps: bool = True,
                 sot_index: Union[None, int, Sequence[int]] = None, check_every: int = 4, max_rows: int = 0,
                 compact: bool = False, record_logprobs: bool = False, stats: Optional[dict] = None,
                 repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                 prompt_lens: Optional[Sequence[int]] = None,
                 sequence_bias: Optional[Sequence[Tuple[Sequence[int], float]]] = None,
                 seeds: Optional[Sequence[int]] = None,
                 language_auto: Optional[dict] = None) -> Tuple[List[GenResult], int]:
        """ctranslate2 Whisper.generate over windows in slots (wm_generate).  max_rows / compact: the row-set decode
        (greedy / one sampled hypothesis; windows refill finished rows in the given order, include/whisper_mi355.h);
        beam search with compact drops finished windows' hypotheses from the passes.
        record_logprobs: per-step log-prob records in each GenResult.  stats: filled with the decode's counters.
        repetition_penalty / no_repeat_ngram_size: CTranslate2's two logit rules over each hypothesis' generated tokens,
        applied on the device before every other rule (1.0 and 0: off; a negative value raises RuntimeError).
        sequence_bias: a list of (token tuple, float) (wm_set_sequence_bias: an additive bias on the token that would
        complete the sequence after the generated tokens, after the penalty and before every mask; scores and records
        are those of the biased distribution).  The table is set for this call and cleared when it ends, so a shared
        engine never keeps another caller's table; None and [] set none.  An invalid table raises RuntimeError naming
        the entry.
        Ragged prompts (ABI 4): the prompts may differ in length (they are padded to the longest and the lengths passed
        on); sot_index=None then derives one index per prompt, and max_length may be one total length per window
        (prompt included).  prompt_lens: the prompts are rows of one length already and window w's prompt is the first
        prompt_lens[w] tokens of its row (the padding is passed as it is: the engine neither reads nor validates it).
        A call whose prompts share one length, with an int max_length and sot_index and no prompt_lens, builds the
        one-length arguments (NULL for the three per-window pointers).
        seeds: one sampling seed per window (wm_generate_seeded; each taken mod 2^64 like `seed`, which is then not
        read): window w's hypothesis j draws its noise from (seeds[w], j), so the window's result is that of a call
        with it alone and seed=seeds[w], wherever it stands in the call.  None calls wm_generate.
        language_auto: dict(lang_begin, n_langs, allowed, positions) (wm_generate_multilingual): window w with
        positions[w] >= 0 is identified on the device before its prefill and the chosen language token replaces the
        placeholder at that prompt position (-1: the window keeps its prompt; `allowed` as language_id's, None = all).
        The call then returns (results, steps, (top [W] i32, top_prob [W] f32, probs [W, n_langs] f32)), top -1 where
        the position is -1."""
        W = len(slots)
        h_seeds = None
        if seeds is not None:
            if len(seeds) != W:
                raise ValueError("seeds needs one seed per window")
            h_seeds = np.ascontiguousarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64)
        st = self.dims.specials
        if prompt_lens is not None:
            lens_in = [int(n) for n in prompt_lens]
            P = len(prompts[0])
            if len(lens_in) != W or any(len(p) != P for p in prompts):
                raise ValueError("prompt_lens needs one length per window and prompts padded to one row length")
        else:
            lens_in = [len(p) for p in prompts]
            P = max(lens_in)
        per_ml = not isinstance(max_length, (int, np.integer))
        per_sot = sot_index is not None and not isinstance(sot_index, (int, np.integer))
        ragged = prompt_lens is not None or any(n != P for n in lens_in) or per_ml or per_sot
        ml_in = [int(v) for v in max_length] if per_ml else [int(max_length)] * W
        if len(ml_in) != W:
            raise ValueError("max_length needs one value per window")
        max_length = max(ml_in)                  # the stride of the output rows
        h_slots = np.ascontiguousarray(slots, dtype=np.int32)
        h_lens = h_sots = h_mls = None
        if not ragged:
            if sot_index is None:
                sot_index = list(prompts[0]).index(st.sot) if st.sot in prompts[0] else -1
            h_prompts = np.ascontiguousarray(np.asarray(prompts, dtype=np.int32).reshape(W, P))
        else:
            h_prompts = np.full((W, P), -1, dtype=np.int32)      # the padding is no token: the engine never reads it
            for w, p in enumerate(prompts):
                h_prompts[w, :len(p)] = np.asarray(p, dtype=np.int32)
            if sot_index is None:
                sots = [list(p[:n]).index(st.sot) if st.sot in list(p[:n]) else -1 for p, n in zip(prompts, lens_in)]
            elif per_sot:
                sots = [int(v) for v in sot_index]
                if len(sots) != W:
                    raise ValueError("sot_index needs one value per window")
            else:
                sots = [int(sot_index)] * W
            h_lens = np.ascontiguousarray(lens_in, dtype=np.int32)
            h_sots = np.ascontiguousarray(sots, dtype=np.int32)
            h_mls = np.ascontiguousarray(ml_in, dtype=np.int32)
            sot_index = int(sots[0])
        sup = np.ascontiguousarray(sorted(set(int(t) for t in suppress_tokens)), dtype=np.int32)
        if sup.size == 0:
            sup = np.zeros(1, dtype=np.int32) - 1
        toks = np.zeros((W, max_length), dtype=np.int32)
        lens = np.zeros(W, dtype=np.int32)
        scores = np.zeros(W, dtype=np.float32)
        cum = np.zeros(W, dtype=np.float32)
        ns = np.zeros(W, dtype=np.float32)
        steps = np.zeros(1, dtype=np.int32)
        lp = np.full((W, max_length), np.nan, dtype=np.float32) if record_logprobs else None
        lpo = np.full((W, max_length), np.nan, dtype=np.float32) if record_logprobs else None
        st64 = np.zeros(4, dtype=np.int64)
        a = _capi.GenerateArgsC(
            W, _i32p(h_slots), P, _i32p(h_prompts), sot_index, beam_size, patience, length_penalty, max_length,
            temperature, num_hypotheses, seed, _i32p(sup), int(sup.size), int(bool(suppress_blank)),
            -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index), int(bool(with_timestamps)),
            check_every, _i32p(toks), _i32p(lens), _f32p(scores), _f32p(cum), _f32p(ns), _i32p(steps),
            int(max_rows), int(bool(compact)), _f32p(lp) if lp is not None else None,
            _f32p(lpo) if lpo is not None else None, st64.ctypes.data_as(C.POINTER(C.c_int64)),
            float(repetition_penalty), int(no_repeat_ngram_size),
            _i32p(h_lens) if ragged else None, _i32p(h_sots) if ragged else None, _i32p(h_mls) if ragged else None)
        la = lang_out = None
        if language_auto is not None:
            n_langs = int(language_auto["n_langs"])
            h_pos = np.ascontiguousarray(language_auto["positions"], dtype=np.int32)
            if h_pos.shape != (W,):
                raise ValueError("language_auto: positions needs one entry per window")
            mask = None
            if language_auto.get("allowed") is not None:
                mask = np.ascontiguousarray(np.asarray(language_auto["allowed"]) != 0, dtype=np.uint8)
                if mask.shape != (n_langs,):
                    raise ValueError(f"language_auto: allowed must have n_langs = {n_langs} entries, got {mask.shape}")
            lang_out = (np.full(W, -1, dtype=np.int32), np.zeros(W, dtype=np.float32),
                        np.zeros((W, max(n_langs, 0)), dtype=np.float32))
            la = _capi.LanguageAutoC(int(language_auto["lang_begin"]), n_langs,
                                     mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None,
                                     _i32p(h_pos), _i32p(lang_out[0]), _f32p(lang_out[1]), _f32p(lang_out[2]))
        with torch.cuda.device(self.device):
            if sequence_bias:
                self.set_sequence_bias(sequence_bias)
            try:
                if la is not None:
                    _capi.check(self.lib.wm_generate_multilingual(
                        self.h, C.byref(a), C.byref(la),
                        h_seeds.ctypes.data_as(C.POINTER(C.c_uint64)) if h_seeds is not None else None,
                        self.stream_ptr()), "wm_generate_multilingual")
                elif h_seeds is None:
                    _capi.check(self.lib.wm_generate(self.h, C.byref(a), self.stream_ptr()), "wm_generate")
                else:
                    _capi.check(self.lib.wm_generate_seeded(self.h, C.byref(a), h_seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                            self.stream_ptr()), "wm_generate_seeded")
            finally:
                if sequence_bias:
                    self.set_sequence_bias(())
        res = []
        for w in range(W):
            n = int(lens[w])
            r = GenResult(toks[w, :n].tolist(), float(scores[w]), float(cum[w]), float(ns[w]))
            if lp is not None:
                nr = min(max_length, n + (1 if lens_in[w] + n < ml_in[w] else 0))
                r.token_logprobs = lp[w, :nr].copy()
                r.token_logprobs_other = lpo[w, :nr].copy()
            res.append(r)
        if stats is not None:
            stats.update(passes=int(st64[0]), row_steps=int(st64[1]), refills=int(st64[2]), graph_captures=int(st64[3]))
        if lang_out is not None:
            return res, int(steps[0]), lang_out
        return res, int(steps[0])

    def set_sequence_bias(self, table: Sequence[Tuple[Sequence[int], float]]) -> None:
        """wm_set_sequence_bias: the engine's table for every later generate until it is replaced (empty: cleared)."""
        seqs = [[int(t) for t in s] for s, _ in table]
        off = np.zeros(len(seqs) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.int64).astype(np.int32) if seqs else 0
        toks = np.ascontiguousarray([t for s in seqs for t in s] or [0], dtype=np.int32)
        bias = np.ascontiguousarray([float(b) for _, b in table] or [0.0], dtype=np.float32)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_set_sequence_bias(self.h, len(seqs), _i32p(off), _i32p(toks), _f32p(bias),
                                                      self.stream_ptr()), "wm_set_sequence_bias")

    def forward(self, slots: Sequence[int], tokens: np.ndarray, last_only: bool = False,
                align_heads: Sequence[Tuple[int, int]] = ()) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """Teacher-forced decoder forward. tokens [n_seq, S] -> logits [n_seq, S, V] (or [n_seq, V])."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        n_seq, S = tokens.shape
        V = self.dims.n_vocab
        logits = torch.empty((n_seq, V) if last_only else (n_seq, S, V), device=self.device, dtype=torch.float32)
        h_slots = np.ascontiguousarray(slots, dtype=np.int32)
        na = len(align_heads)
        heads = np.ascontiguousarray(np.asarray(align_heads, dtype=np.int32).reshape(max(na, 1), 2) if na else np.zeros((1, 2), np.int32))
        attn = torch.empty((n_seq, S, na, self.dims.n_audio_ctx), device=self.device, dtype=torch.float32) if na else None
        if n_seq > self.n_hyp:
            self.reserve(max(self.n_slots, 1), n_seq)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_forward(self.h, n_seq, _i32p(h_slots), S, _i32p(tokens), C.c_void_p(logits.data_ptr()),
                                            int(last_only), _i32p(heads), na,
                                            C.c_void_p(attn.data_ptr()) if attn is not None else None,
                                            self.stream_ptr()), "wm_forward")
        return logits, attn

    def detect_language(self, slots: Sequence[int], lang_begin: int, n_langs: int) -> np.ndarray:
        """wm_detect_language: language-token probabilities [len(slots), n_langs] of one decoder step from
        <|startoftranscript|> per window (softmax on the device)."""
        h_slots = np.ascontiguousarray(slots, dtype=np.int32)
        probs = np.zeros((len(slots), n_langs), dtype=np.float32)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_detect_language(self.h, len(slots), _i32p(h_slots), lang_begin, n_langs, _f32p(probs),
                                                    self.stream_ptr()), "wm_detect_language")
        return probs

    def language_id(self, slots: Sequence[int], lang_begin: int, n_langs: int,
                    allowed: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """wm_language_id: one decoder step from <|startoftranscript|> per slot and the language head on the device
        (no full-vocabulary logits).  `allowed` ([n_langs] of 0 / 1, None = all) restricts the softmax; a masked
        language's probability is exactly 0.  -> (probs [n, n_langs] f32, top [n] i32, top_prob [n] f32)."""
        h_slots = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(h_slots)
        probs = np.zeros((n, max(n_langs, 0)), dtype=np.float32)
        top = np.zeros(n, dtype=np.int32)
        top_prob = np.zeros(n, dtype=np.float32)
        mask = None
        if allowed is not None:
            mask = np.ascontiguousarray(np.asarray(allowed) != 0, dtype=np.uint8)
            if mask.shape != (n_langs,):
                raise ValueError(f"language_id: allowed must have n_langs = {n_langs} entries, got {mask.shape}")
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_language_id(self.h, n, _i32p(h_slots), lang_begin, n_langs,
                                                mask.ctypes.data_as(C.POINTER(C.c_uint8)) if mask is not None else None,
                                                _f32p(probs), _i32p(top), _f32p(top_prob), self.stream_ptr()),
                        "wm_language_id")
        return probs, top, top_prob

    def align(self, slot: int, sot_sequence: Sequence[int], text_tokens: Sequence[int], num_frames: int,
              alignment_heads: Sequence[Tuple[int, int]], median_filter_width: int = 7):
        """-> (text_token_probs [n_text], text_indices, time_indices) (CTranslate2 Whisper.align for one window)."""
        sot = np.ascontiguousarray(sot_sequence, dtype=np.int32)
        text = np.ascontiguousarray(text_tokens, dtype=np.int32)
        heads = np.ascontiguousarray(np.asarray(alignment_heads, dtype=np.int32).reshape(-1, 2))
        cap = len(text) + 1 + num_frames // 2 + 2
        probs = np.zeros(max(len(text), 1), dtype=np.float32)
        ti = np.zeros(cap, dtype=np.int32)
        tj = np.zeros(cap, dtype=np.int32)
        n = np.zeros(1, dtype=np.int32)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.wm_align(self.h, slot, len(sot), _i32p(sot), len(text), _i32p(text), num_frames,
                                          _i32p(heads), heads.shape[0], median_filter_width, _f32p(probs), _i32p(ti),
                                          _i32p(tj), _i32p(n), self.stream_ptr()), "wm_align")
        k = int(n[0])
        return probs[: len(text)], ti[:k].copy(), tj[:k].copy()

    def align_batch(self, slots: Sequence[int], sot_sequence: Sequence[int], texts: Sequence[Sequence[int]],
                    num_frames: Sequence[int], alignment_heads: Sequence[Tuple[int, int]], median_filter_width: int = 7):
        """wm_align_batch: CTranslate2 Whisper.align for several windows at once -> one (text_token_probs,
        text_indices, time_indices) per window (every window needs >= 1 text token)."""
        return self._align_batch(False, slots, sot_sequence, texts, num_frames, alignment_heads, median_filter_width)

    def align_open_batch(self, slots: Sequence[int], sot_sequence: Sequence[int], texts: Sequence[Sequence[int]],
                         num_frames: Sequence[int], heads: Sequence[Tuple[int, int]], median_filter_width: int = 7):
        """wm_align_open_batch: align_batch with the open-end DTW (forced alignment: a window's text may run past its
        audio) -> one (text_token_probs, text_indices, time_indices, rows) per window.  rows = R, the smallest end row
        in [1, n_text + 1] of minimum cost: the path visits rows 0 .. R-1; R == n_text + 1 is align_batch's path."""
        return self._align_batch(True, slots, sot_sequence, texts, num_frames, heads, median_filter_width)

    def _align_batch(self, open_end: bool, slots, sot_sequence, texts, num_frames, alignment_heads, median_filter_width):
        n = len(slots)
        if n == 0:
            return []
        sot = np.ascontiguousarray(sot_sequence, dtype=np.int32)
        lens = [len(t) for t in texts]
        off = np.zeros(n + 1, dtype=np.int32)
        off[1:] = np.cumsum(lens)
        text = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t in texts]), dtype=np.int32)
        nf = np.ascontiguousarray(num_frames, dtype=np.int32)
        cap = [l + 1 + f // 2 for l, f in zip(lens, nf)]
        poff = np.zeros(n, dtype=np.int64)
        poff[1:] = np.cumsum(cap)[:-1]
        heads = np.ascontiguousarray(np.asarray(alignment_heads, dtype=np.int32).reshape(-1, 2))
        probs = np.zeros(max(int(off[-1]), 1), dtype=np.float32)
        ti = np.zeros(sum(cap), dtype=np.int32)
        tj = np.zeros(sum(cap), dtype=np.int32)
        plen = np.zeros(n, dtype=np.int32)
        rows = np.zeros(n, dtype=np.int32)
        hs = np.ascontiguousarray(slots, dtype=np.int32)
        args = (self.h, n, _i32p(hs), len(sot), _i32p(sot), _i32p(off), _i32p(text), _i32p(nf), _i32p(heads), heads.shape[0],
                median_filter_width, _f32p(probs), poff.ctypes.data_as(C.POINTER(C.c_int64)), _i32p(ti), _i32p(tj),
                _i32p(plen))
        with torch.cuda.device(self.device):
            if open_end:
                _capi.check(self.lib.wm_align_open_batch(*args, _i32p(rows), self.stream_ptr()), "wm_align_open_batch")
            else:
                _capi.check(self.lib.wm_align_batch(*args, self.stream_ptr()), "wm_align_batch")
        out = []
        for i in range(n):
            a, k = int(poff[i]), int(plen[i])
            item = (probs[off[i]: off[i + 1]].copy(), ti[a: a + k].copy(), tj[a: a + k].copy())
            out.append(item + (int(rows[i]),) if open_end else item)
        return out

    def dtw(self, cost: torch.Tensor, open_end: bool = False):
        """DTW path of a device cost matrix [N, M] (f32) -> (text_indices, time_indices).  open_end=True: the open-end
        form (wm_dtw_open: the path ends at the smallest row R of minimum cost in the last column) ->
        (text_indices, time_indices, R); a matrix whose minimum end cost is not finite raises RuntimeError."""
        cost = cost.to(self.device, torch.float32).contiguous()
        N, M = cost.shape
        ti = np.zeros(N + M + 2, dtype=np.int32)
        tj = np.zeros(N + M + 2, dtype=np.int32)
        n = np.zeros(1, dtype=np.int32)
        rows = np.zeros(1, dtype=np.int32)
        with torch.cuda.device(self.device):
            if open_end:
                _capi.check(self.lib.wm_dtw_open(self.h, C.c_void_p(cost.data_ptr()), N, M, _i32p(ti), _i32p(tj), _i32p(n),
                                                 _i32p(rows), self.stream_ptr()), "wm_dtw_open")
            else:
                _capi.check(self.lib.wm_dtw(self.h, C.c_void_p(cost.data_ptr()), N, M, _i32p(ti), _i32p(tj), _i32p(n),
                                            self.stream_ptr()), "wm_dtw")
        k = int(n[0])
        if open_end:
            return ti[:k].copy(), tj[:k].copy(), int(rows[0])
        return ti[:k].copy(), tj[:k].copy()
