"""faster-whisper-shaped drop-in: WhisperModel(...).transcribe(...) -> (Iterable[Segment], TranscriptionInfo).

This is the surface the vlog transcription worker calls (reference `worker/transcription.py:78-111`):

    model = WhisperModel(WHISPER_MODEL, device="cpu", compute_type=TRANSCRIPTION_COMPUTE_TYPE)   # :81-85
    segments, info = model.transcribe(str(wav), language=lang, task="transcribe", beam_size=5,
                                      vad_filter=True)                                          # :105-111
    for segment in segments: segment.start, segment.end, segment.text                           # :117-125
    info.language                                                                               # :131

Semantics follow faster-whisper 1.1.x `WhisperModel.transcribe` / `generate_segments` /
`generate_with_fallback` / `add_word_timestamps` [FW↑] (restated; the package is not installed here):
sequential seek loop over 30 s windows, previous-text prompt (`<|startofprev|>` + last 223 tokens),
temperature fallback on compression ratio / average log-probability with the no-speech exemption, segment
split at timestamp pairs, optional cross-attention word alignment.  Every tensor operation runs on the
MI355X through libwhisper_mi355 (vlog_amd/engine.py); there is no CPU compute path: device="cpu" (the
worker's literal argument) is remapped to the GPU and logged, and construction fails loudly when no GPU or
no HIP library is available.

`BatchedInferencePipeline` is the throughput mode (faster-whisper's class of the same name): fixed 30 s
windows decoded independently (no text conditioning), batched on one GPU, or sharded over several GPUs
with vlog_amd/shard.py.
"""
from __future__ import annotations

import inspect
import itertools
import logging
import os
import threading
import types
from dataclasses import MISSING, asdict, dataclass, fields
from typing import Any, BinaryIO, Iterable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import segments as segs
from .segments import _word_means, merge_punctuations
from .audio import mono_f32, read_wav
from .captions import resolve_caption_options, set_word_tokens, shape_captions
from .language_id import (LanguageWindow, candidate_mask, candidates_in_force, detection_rule, detection_windows,
                          timeline_windows, window_probs, window_times)
from .seek_state import (ENERGY_FRAME_MEL, MAX_SECTIONS, SeekState, chunk_joins, decode_round_levels, decode_round_with,
                         fallback_ladder, iter_lockstep, plan_sections, run_lockstep, window_max_length)
from .dims import CHUNK_LENGTH, HOP_LENGTH, N_FRAMES, SAMPLE_RATE, TIME_PRECISION
from .tokenizer import Tokenizer
from .weights import resolve_model

logger = logging.getLogger("vlog_amd")

FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH          # 100
INPUT_STRIDE = 2
TOKENS_PER_SECOND = SAMPLE_RATE // (HOP_LENGTH * INPUT_STRIDE)   # 50
MAX_LENGTH = 448


@dataclass
class Word:
    start: float
    end: float
    word: str
    probability: float

    def _asdict(self):
        return asdict(self)


@dataclass
class Segment:
    id: int
    seek: int
    start: float
    end: float
    text: str
    tokens: List[int]
    avg_logprob: float
    compression_ratio: float
    no_speech_prob: float
    words: Optional[List[Word]]
    temperature: Optional[float]
    language: Optional[str] = None      # multilingual=True: the language this segment's window was decoded under

    def _asdict(self):
        d = asdict(self)
        if self.language is None:           # with the option off a segment's dict is what it was
            del d["language"]
        return d


@dataclass
class TranscriptionOptions:
    beam_size: int
    best_of: int
    patience: float
    length_penalty: float
    repetition_penalty: float
    no_repeat_ngram_size: int
    log_prob_threshold: Optional[float]
    no_speech_threshold: Optional[float]
    compression_ratio_threshold: Optional[float]
    condition_on_previous_text: bool
    prompt_reset_on_temperature: float
    temperatures: List[float]
    initial_prompt: Optional[Union[str, Iterable[int]]]
    prefix: Optional[str]
    suppress_blank: bool
    suppress_tokens: Optional[List[int]]
    without_timestamps: bool
    max_initial_timestamp: float
    word_timestamps: bool
    prepend_punctuations: str
    append_punctuations: str
    multilingual: bool
    max_new_tokens: Optional[int]
    clip_timestamps: Union[str, List[float]]
    hallucination_silence_threshold: Optional[float]
    hotwords: Optional[str]
    section_frames: Optional[List[Tuple[int, int]]] = None     # transcribe(sections=N): the (start, end) chosen
    sequence_bias: Optional[Mapping[Union[str, Tuple[int, ...]], float]] = None   # as passed (or the environment file's)
    sequence_bias_table: Optional[List[Tuple[Tuple[int, ...], float]]] = None     # ... as the engine takes it
    lockstep_fallback: bool = False     # the fallback temperatures of a lockstep round decode by levels (as resolved)
    max_line_width: Optional[int] = None        # caption shaping (captions.shape_captions) as in force; None: off.
    max_line_count: Optional[int] = None        # ... while it is on, word_timestamps reads True
    max_cue_seconds: Optional[float] = None
    language_candidates: Optional[Tuple[str, ...]] = None      # the language whitelist in force (None: off)


@dataclass
class VadOptions:
    threshold: float = 0.5
    neg_threshold: Optional[float] = None
    min_speech_duration_ms: int = 0
    max_speech_duration_s: float = float("inf")
    min_silence_duration_ms: int = 2000
    speech_pad_ms: int = 400


@dataclass
class TranscriptionInfo:
    language: str
    language_probability: float
    duration: float
    duration_after_vad: float
    all_language_probs: Optional[List[Tuple[str, float]]]
    transcription_options: TranscriptionOptions
    vad_options: Optional[VadOptions]


@dataclass
class AlignmentInfo:
    """What WhisperModel.align reports beside its segments.  window_rows: per window (seek in mel frames, rows
    offered = candidate tokens + 1, rows the open-end DTW reached)."""
    language: str
    language_probability: float
    duration: float
    duration_after_vad: float
    windows: int
    unaligned_words: int
    window_rows: List[Tuple[int, int, int]]


@dataclass
class _GenOut:
    tokens: List[int]
    score: float
    no_speech_prob: float
    language: Optional[str] = None      # multilingual=True, a window's first decode: the language detected for it


def _resolve_multilingual(value: Optional[bool]) -> bool:
    """The multilingual argument of the transcribe calls: None reads VLOG_AMD_MULTILINGUAL (0 / 1; unset or empty:
    off)."""
    if value is not None:
        return bool(value)
    env = os.environ.get("VLOG_AMD_MULTILINGUAL", "")
    if env not in ("", "0", "1"):
        raise ValueError(f"VLOG_AMD_MULTILINGUAL must be 0 or 1, got {env!r}")
    return env == "1"


def _resolve_lockstep_fallback(value: Optional[bool]) -> bool:
    """The lockstep_fallback argument of transcribe / transcribe_many: None reads VLOG_AMD_LOCKSTEP_FALLBACK (0 / 1;
    unset or empty: off)."""
    if value is not None:
        return bool(value)
    env = os.environ.get("VLOG_AMD_LOCKSTEP_FALLBACK", "")
    if env not in ("", "0", "1"):
        raise ValueError(f"VLOG_AMD_LOCKSTEP_FALLBACK must be 0 or 1, got {env!r}")
    return env == "1"


def _word(w: dict) -> Word:
    """An aligned word dict of add_word_timestamps -> Word.  The word's text tokens ride along outside the dataclass
    fields (captions.word_tokens), so caption shaping can give every cue its own tokens."""
    word = Word(start=w["start"], end=w["end"], word=w["word"], probability=w["probability"])
    if "tokens" in w:
        set_word_tokens(word, w["tokens"])
    return word


def _shaped(segments, options: TranscriptionOptions):
    """The last stage of every segment stream: shape_captions when the options have it on."""
    if not options.max_line_width:
        return segments
    return shape_captions(segments, options.max_line_width, options.max_line_count, options.max_cue_seconds)


def _finished(segments, speech_chunks, options: Optional[TranscriptionOptions] = None):
    """The tail of a sequential segment stream: the VAD's times restored to file time, then caption shaping
    (options None: align, which does not shape)."""
    if speech_chunks:
        from .vad import restore_speech_timestamps
        segments = restore_speech_timestamps(segments, speech_chunks, SAMPLE_RATE)
    return segments if options is None else _shaped(segments, options)


def _vad_options(vad_parameters) -> VadOptions:
    return vad_parameters if isinstance(vad_parameters, VadOptions) else VadOptions(**(vad_parameters or {}))


def _decode_kwargs(options: TranscriptionOptions, temperature: float) -> dict:
    """The engine.generate keyword arguments that every decode form takes from the options at one temperature.  The
    call sites add what is theirs: slots, prompts, max_length, sot_index, the suppress list, seed or seeds,
    num_hypotheses, compact, language_auto."""
    return dict(beam_size=1 if temperature > 0 else options.beam_size, patience=options.patience,
                length_penalty=options.length_penalty, temperature=temperature, suppress_blank=options.suppress_blank,
                max_initial_timestamp_index=int(round(options.max_initial_timestamp / TIME_PRECISION)),
                with_timestamps=not options.without_timestamps, check_every=4,
                repetition_penalty=options.repetition_penalty, no_repeat_ngram_size=options.no_repeat_ngram_size,
                sequence_bias=options.sequence_bias_table)


@dataclass
class _File:
    """One file before its decode: the log-mel, its language and what TranscriptionInfo reports.  speech_chunks: the
    VAD chunks the sequential path collected (None: no VAD); windows: the throughput path's (seek, size) ranges."""
    features: torch.Tensor
    duration: float
    duration_after_vad: float
    vad_options: Optional[VadOptions]
    language: str
    language_probability: float
    all_language_probs: Optional[List[Tuple[str, float]]]
    language_candidates: Optional[Tuple[str, ...]]      # the whitelist in force for this file (None: off, or named)
    speech_chunks: Optional[List[dict]] = None
    windows: Optional[List[Tuple[int, int]]] = None

    def info(self, options: TranscriptionOptions) -> TranscriptionInfo:
        return TranscriptionInfo(language=self.language, language_probability=self.language_probability,
                                 duration=self.duration, duration_after_vad=self.duration_after_vad,
                                 all_language_probs=self.all_language_probs, transcription_options=options,
                                 vad_options=self.vad_options)


_NO_CLIPS = ("0", [0], [0.0])           # the clip_timestamps values that clip nothing
_PER_FILE = ("language", "initial_prompt", "hotwords", "prefix")


@dataclass(frozen=True)
class _Call:
    """A public transcribe call after validation and environment resolution (_resolve_call): built once, at the top
    of the entry point, and handed on as it is (to the throughput pipeline too).
    args: every argument by its public name, as resolved: multilingual, lockstep_fallback and sections as in force;
    language_candidates the call's tuple or None; max_line_width / max_line_count / max_cue_seconds as in force (None:
    shaping off) with word_timestamps forced on by them; language, initial_prompt, hotwords and prefix as lists with one
    value per file (one file: one value).
    throughput: the options are BatchedInferencePipeline's (no text conditioning, no prefix, no clips)."""
    args: Mapping[str, Any]
    throughput: bool

    def options(self, model: "WhisperModel", tokenizer: Tokenizer, f: int = 0,
                language_candidates: Optional[Tuple[str, ...]] = None) -> TranscriptionOptions:
        """The TranscriptionOptions of file f under `tokenizer` (the suppress list and the sequence-bias table depend on
        it).  Where each field comes from:
          * a field with the name of an argument of the call is that argument as resolved: the plain decode options,
            and multilingual, lockstep_fallback, word_timestamps and the three caption fields as in force.  A new
            option that TranscriptionOptions echoes under its own name needs nothing here; a field that shares its
            name with an argument of ANOTHER meaning must be set explicitly below;
          * derived below: temperatures (from `temperature`), suppress_tokens and the sequence-bias pair (both through
            the tokenizer), the per-file initial_prompt / prefix / hotwords, and the file's language_candidates;
          * section_frames is set by `transcribe` once the sections are planned;
          * BatchedInferencePipeline's entry points have no condition_on_previous_text, prompt_reset_on_temperature
            or lockstep_fallback argument: the throughput block sets them, with the other constants of that mode,
            and overrides what a WhisperModel call in throughput mode passed for them."""
        a = self.args
        o = {fd.name: a[fd.name] for fd in fields(TranscriptionOptions) if fd.name in a}
        t, sup = a["temperature"], a["suppress_tokens"]
        o["sequence_bias"], o["sequence_bias_table"] = model._sequence_bias(tokenizer, a["sequence_bias"])
        o.update(temperatures=list(t) if isinstance(t, (list, tuple)) else [t],
                 suppress_tokens=list(tokenizer.suppressed_tokens(sup)) if sup else [],
                 initial_prompt=a["initial_prompt"][f], prefix=a["prefix"][f], hotwords=a["hotwords"][f],
                 language_candidates=language_candidates or None)
        if self.throughput:
            o.update(condition_on_previous_text=False, prompt_reset_on_temperature=0.5, prefix=None,
                     hallucination_silence_threshold=None, clip_timestamps=a["clip_timestamps"] or "0",
                     lockstep_fallback=False)       # (throughput mode has its own batched re-decode)
        return TranscriptionOptions(**o)


def _resolve_call(model: "WhisperModel", entry: str, args: Mapping[str, Any], n_files: Optional[int] = None) -> _Call:
    """The one resolver of the four public entry points.  entry: "transcribe" / "transcribe_many" (WhisperModel) or
    "batched" / "batched_many" (BatchedInferencePipeline); args: the entry point's arguments by name (its locals());
    n_files: len(audios) of a _many entry.  Every check and every environment default of a call lives here; the
    checks run in the order each entry point has always run them (`order` below), so a call with two mistakes keeps
    reporting the same one."""
    a = {k: v for k, v in args.items() if k not in ("self", "audio", "audios", "kw")}
    many, batched = n_files is not None, entry.startswith("batched")
    n = n_files if many else 1

    def hallucination():
        if a["hallucination_silence_threshold"] is not None:
            raise NotImplementedError(f"hallucination_silence_threshold={a['hallucination_silence_threshold']!r} is "
                                      "not supported by the MI355X engine")

    def multilingual():
        named = a["language"]
        a["multilingual"] = model._multilingual(
            a["multilingual"], named if many and isinstance(named, (list, tuple)) else [named])

    def chunk_length():
        if a["chunk_length"] not in (None, CHUNK_LENGTH):
            raise NotImplementedError("chunk_length other than 30 s is not supported")

    def task():
        if a["task"] not in ("transcribe", "translate"):
            raise ValueError(f"unknown task {a['task']!r}")

    def sections():
        if a["sections"] is None:
            a["sections"] = int(os.environ.get("VLOG_AMD_SECTIONS", "") or 1)
        if not 1 <= a["sections"] <= MAX_SECTIONS:
            raise ValueError(f"sections must be between 1 and {MAX_SECTIONS}, got {a['sections']}")
        if a["sections_in_flight"] is not None and a["sections_in_flight"] < 1:
            raise ValueError("sections_in_flight must be >= 1")
        if a["sections"] > 1 and model.throughput:
            raise ValueError("sections > 1 is the sequential mode's; throughput mode cuts the file its own way")
        if a["sections"] > 1 and a["clip_timestamps"] not in _NO_CLIPS:
            raise ValueError("sections > 1 cannot be combined with clip_timestamps")

    def max_files():
        if a["max_files"] < 1:
            raise ValueError("max_files must be >= 1")

    def one_bias():
        if a["sequence_bias"] is not None and not isinstance(a["sequence_bias"], Mapping):
            raise ValueError("sequence_bias: one mapping for all files expected, not a per-file list")

    def lockstep_fallback():
        a["lockstep_fallback"] = _resolve_lockstep_fallback(a["lockstep_fallback"])

    def captions():
        caps = resolve_caption_options(a["max_line_width"], a["max_line_count"], a["max_cue_seconds"], os.environ)
        a["max_line_width"], a["max_line_count"], a["max_cue_seconds"] = caps or (None, None, None)
        if caps:
            a["word_timestamps"] = True         # the shaper needs word times

    def candidates():
        a["language_candidates"] = model._language_candidates(a["language_candidates"])

    def per_file():
        for name in _PER_FILE:
            v = a[name]
            # (a list as the initial prompt of ONE call, or of the pipeline's transcribe_many, is token ids)
            if many and isinstance(v, (list, tuple)) and (name == "language" or not batched):
                if len(v) != n:
                    raise ValueError("one language per file" if batched else
                                     f"{name}: one value per file expected ({n}), got {len(v)}")
                a[name] = list(v)
            else:
                a[name] = [v] * n

    def no_prefix():        # every window of a batch shares one prompt length; a prefix belongs to the first only
        if a["prefix"] is not None:
            raise NotImplementedError("initial_prompt / clip_timestamps / prefix in throughput mode")

    def throughput_forward():
        if not model.throughput:
            return
        if any(p is not None for p in a["initial_prompt"]) or a["clip_timestamps"] not in _NO_CLIPS or \
                any(p is not None for p in a["prefix"]):
            raise NotImplementedError("initial_prompt / clip_timestamps / prefix in throughput mode")
        if len(set(a["hotwords"])) > 1:
            raise NotImplementedError("per-file hotwords in throughput mode")
        a["clip_timestamps"] = None             # (nothing is clipped: the pipeline's own default)

    order = {"transcribe": (hallucination, multilingual, chunk_length, task, sections, lockstep_fallback, captions,
                            candidates, per_file, throughput_forward),
             "transcribe_many": (hallucination, multilingual, chunk_length, task, max_files, one_bias,
                                 lockstep_fallback, captions, candidates, per_file, throughput_forward),
             "batched": (hallucination, multilingual, no_prefix, captions, candidates, per_file),
             "batched_many": (no_prefix, captions, one_bias, candidates, multilingual, per_file)}
    for check in order[entry]:
        check()
    return _Call(args=types.MappingProxyType(a), throughput=batched or model.throughput)


def _resolve_device_index(device: str, device_index) -> int:
    if isinstance(device_index, (list, tuple)):
        if len(device_index) != 1:
            raise ValueError("one WhisperModel drives one GPU; use BatchedInferencePipeline(shards=...) or "
                             "vlog_amd.shard for several")
        device_index = device_index[0]
    env = os.environ.get("VLOG_AMD_DEVICE")
    if env is not None:
        device_index = int(env)
    if device in ("cpu", "auto", "cuda", "rocm", "hip"):
        if device == "cpu":
            logger.warning("WhisperModel(device='cpu') remapped to MI355X GPU %d (vlog_amd has no CPU path)", device_index)
    else:
        raise ValueError(f"unsupported device {device!r}")
    if not torch.cuda.is_available():
        raise RuntimeError("vlog_amd.WhisperModel needs an AMD Instinct GPU (torch.cuda.is_available() is False)")
    return int(device_index)


class WhisperModel:
    """faster_whisper.WhisperModel-compatible constructor (model_size_or_path, device, device_index,
    compute_type, cpu_threads, num_workers, download_root, local_files_only, files, revision, ...)."""

    def __init__(self, model_size_or_path: str, device: str = "auto", device_index: Union[int, List[int]] = 0,
                 compute_type: str = "default", cpu_threads: int = 0, num_workers: int = 1,
                 download_root: Optional[str] = None, local_files_only: bool = False, files: dict = None,
                 revision: Optional[str] = None, use_auth_token=None, seed: int = 0,
                 eot_after: Optional[int] = None, throughput: Optional[bool] = None, vad_model: Optional[str] = None,
                 **model_kwargs):
        """throughput: route transcribe() through BatchedInferencePipeline (default: the VLOG_AMD_THROUGHPUT
        environment variable, so the unchanged worker can opt in without code changes).
        vad_model: Silero VAD v5 weights for vad_filter=True — a local .safetensors/.npz file or
        "synthetic:<seed>" (default: the VLOG_AMD_SILERO_VAD environment variable; unset = the frame-energy
        stand-in, vlog_amd/vad.py)."""
        from .engine import GpuEngine

        if throughput is None:
            throughput = os.environ.get("VLOG_AMD_THROUGHPUT", "0") not in ("", "0")
        self.throughput = bool(throughput)
        self._batched = None

        if files:
            raise NotImplementedError("in-memory model files are not supported")
        if compute_type not in ("default", "auto", "int8", "int8_float16", "int8_float32", "int8_bfloat16",
                                "float16", "bfloat16", "float32"):
            raise ValueError(f"unsupported compute_type {compute_type!r}")
        if compute_type not in ("default", "auto", "bfloat16"):
            logger.info("compute_type=%s mapped to bf16 weights / f32 accumulation on MI355X", compute_type)
        self.device_index = _resolve_device_index(device, device_index)
        self.dims, sd, model_dir = resolve_model(model_size_or_path, seed=seed, eot_after=eot_after)
        self.model_dir = model_dir
        tj = os.path.join(model_dir, "tokenizer.json") if model_dir else None
        self._tokenizer_json = tj if tj and os.path.isfile(tj) else None
        self._tok_seed = seed
        self.engine = GpuEngine(self.dims, sd, self.device_index)
        del sd
        self.engine.reserve(1, 8)
        from .silero import SileroVad, default_spec
        vad_spec = vad_model if vad_model is not None else default_spec()
        self.vad_net = SileroVad.from_spec(self.engine, vad_spec) if vad_spec else None
        self._lock = threading.RLock()
        # VLOG_AMD_SEQUENCE_BIAS=<JSON file {"phrase": bias}>: the sequence bias of every call that passes none (the
        # unchanged worker's custom vocabulary); read and tokenised once here, so a bad file fails the construction
        self._env_sequence_bias = None
        if os.environ.get("VLOG_AMD_SEQUENCE_BIAS"):
            self._env_sequence_bias = segs.load_sequence_bias_file(os.environ["VLOG_AMD_SEQUENCE_BIAS"])
            segs.build_sequence_bias(self.tokenizer().encode, self._env_sequence_bias, self.dims.n_vocab)
        self.feature_size = self.dims.n_mels
        self.num_samples_per_token = HOP_LENGTH * INPUT_STRIDE
        self.frames_per_second = FRAMES_PER_SECOND
        self.tokens_per_second = TOKENS_PER_SECOND
        self.input_stride = INPUT_STRIDE
        self.time_precision = TIME_PRECISION
        self.max_length = MAX_LENGTH

    def _pipeline(self) -> "BatchedInferencePipeline":
        with self._lock:                      # created once even when several worker threads race here
            if self._batched is None:
                self._batched = BatchedInferencePipeline(
                    self, max_batch_windows=int(os.environ.get("VLOG_AMD_BATCH_WINDOWS", "150")))
            return self._batched

    @property
    def is_multilingual(self) -> bool:
        return self.dims.multilingual

    @property
    def supported_languages(self) -> List[str]:
        return list(self.dims.specials.lang_codes) if self.is_multilingual else ["en"]

    def tokenizer(self, task: Optional[str] = "transcribe", language: Optional[str] = None) -> Tokenizer:
        return Tokenizer(self.dims, task=task, language=language, tokenizer_json=self._tokenizer_json, seed=self._tok_seed)

    def _language_candidates(self, value, language: Optional[str] = None) -> Optional[Tuple[str, ...]]:
        """The `language_candidates` argument of a call -> the tuple in force, or None (language_id.py): None reads
        VLOG_AMD_LANGUAGE_CANDIDATES, an empty sequence is off; ignored when the call names its language and in an
        English-only model."""
        codes = self.dims.specials.lang_codes if self.is_multilingual else ()
        return candidates_in_force(value, os.environ, codes, self.is_multilingual, language)

    def _multilingual(self, value: Optional[bool], languages: Sequence[Optional[str]] = ()) -> bool:
        """The `multilingual` argument of a call -> what is in force: None reads VLOG_AMD_MULTILINGUAL; an English-only
        model turns it off (logged once, as faster-whisper does).  languages: the languages the call names (None: to be
        detected).  A call that names a language asks for that language in every window, so multilingual=True with it
        stays refused with NotImplementedError, as it was; the environment's default is then simply off (logged once),
        so a worker that configures a language keeps it."""
        on = _resolve_multilingual(value)
        if on and not self.is_multilingual:
            if not getattr(self, "_warned_multilingual", False):
                logger.warning("The current model is English-only but the multilingual parameter is set to True; "
                               "setting to False instead.")
                self._warned_multilingual = True
            return False
        named = [c for c in languages if c is not None]
        if on and named:
            if value is not None:
                raise NotImplementedError(f"multilingual=True with language={named[0]!r} is not supported by the MI355X "
                                          "engine: a named language holds for every window (pass language=None)")
            if not getattr(self, "_warned_multilingual_named", False):
                logger.warning("VLOG_AMD_MULTILINGUAL is ignored by calls that name their language")
                self._warned_multilingual_named = True
            return False
        return on

    def _language_auto(self, options, positions: Sequence[int]) -> dict:
        """engine.generate's language_auto for a multilingual first decode: the language tokens, the call's whitelist as
        the mask (language_candidates applies to the per-window detection too) and the windows' prompt positions."""
        st = self.dims.specials
        cand = options.language_candidates
        return dict(lang_begin=st.lang_begin, n_langs=st.n_langs,
                    allowed=candidate_mask(cand, st.lang_codes) if cand else None, positions=list(positions))

    def _sequence_bias(self, tokenizer: Tokenizer, sequence_bias):
        """The `sequence_bias` argument of a transcribe call -> (the mapping in force, the engine's table or None).
        None takes the VLOG_AMD_SEQUENCE_BIAS file's mapping when there is one; anything but a mapping (a per-file
        list, say: the table is one per call, like the suppress list) raises ValueError."""
        if sequence_bias is None:
            sequence_bias = self._env_sequence_bias
        if sequence_bias is None:
            return None, None
        table = segs.build_sequence_bias(tokenizer.encode, sequence_bias, self.dims.n_vocab)
        return dict(sequence_bias), (table or None)

    # ------------------------------------------------------------------ features / encoder
    def _load_audio(self, src) -> np.ndarray:
        """A WAV path / file object -> float32 mono at 16 kHz.  A 16 kHz file is int16 / 32768 with the channels
        averaged (audio.load_audio's path, bit for bit); any other rate is downmixed and resampled on the device
        (Engine.resample) and copied back for the host stages (VAD, chunk collection)."""
        frames, rate = read_wav(src)
        if rate == SAMPLE_RATE:
            return mono_f32(frames)
        with self._lock:
            return self.engine.resample(frames, rate).cpu().numpy()

    def _features(self, audio: np.ndarray) -> torch.Tensor:
        return self.engine.features(torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)))

    def _use_cross_form(self, rows_per_window: int) -> None:
        """Cross-attention form for decodes with `rows_per_window` rows per window: the factored form (attention
        over the encoder output; half the bytes of K and V) for one row, the projected K/V form when several
        rows share a window (beam search: every row of the group reads the window's K/V panels once, while the
        factored kernel re-reads the encoder output per 32 (row, head) pairs).  The opt-in fp8
        cross memory is a factored-form mode and is never overridden; VLOG_AMD_CROSS_AUTO=0 disables the choice.
        The projected form's own fp8 option (cross_kv_fp8 / VLOG_AMD_CROSS_KV_FP8) leaves the choice on: beam groups
        then read fp8 K/V panels and one-row decodes the factored bf16 form."""
        if os.environ.get("VLOG_AMD_CROSS_AUTO", "1") == "0" or self.engine.option("cross_fp8", 0):
            return
        self.engine.set_option("cross_mode", 0 if rows_per_window > 1 else 1)

    def _encode(self, features: torch.Tensor, seek: int, size: int, slot: int = 0) -> torch.Tensor:
        enc = self.engine.encode(features, [seek], [size])
        self.engine.cross_kv(enc, slot)
        return enc

    # ------------------------------------------------------------------ language detection
    def detect_language(self, audio: Optional[np.ndarray] = None, features: Optional[torch.Tensor] = None,
                        vad_filter: bool = False, vad_parameters=None, language_detection_segments: int = 1,
                        language_detection_threshold: float = 0.5,
                        language_candidates: Optional[Sequence[str]] = None) -> Tuple[str, float, List[Tuple[str, float]]]:
        """faster-whisper `detect_language`: encode up to `language_detection_segments` windows, one decoder
        step from <|startoftranscript|>, softmax over the language tokens; majority vote if no window is
        confident.

        language_candidates (see `transcribe`): with candidates in force the windows are encoded in ONE encode call
        and identified in ONE wm_language_id call with the candidates' mask; the rule above is then applied on the
        host to the per-window results in window order (language_id.detection_rule), and the probabilities returned
        are over the candidates only.  Off (and VLOG_AMD_LANGUAGE_CANDIDATES unset): the loop below, untouched."""
        candidates = self._language_candidates(language_candidates)
        if not self.is_multilingual:
            return "en", 1.0, [("en", 1.0)]
        if candidates is not None:
            st = self.dims.specials
            with self._lock:
                if features is None:
                    features = self._features(audio)
                content = features.shape[1] - 1 if features.shape[1] > 1 else features.shape[1]
                wins = detection_windows(content, language_detection_segments)
                enc = self.engine.encode(features, [s for s, _ in wins], [n for _, n in wins])
                self.engine.cross_kv(enc, 0)
                probs, _, _ = self.engine.language_id(list(range(len(wins))), st.lang_begin, st.n_langs,
                                                      candidate_mask(candidates, st.lang_codes))
            return detection_rule([window_probs(p, st.lang_codes, candidates) for p in probs],
                                  language_detection_threshold)
        with self._lock:
            if features is None:
                features = self._features(audio)
            st = self.dims.specials
            content = features.shape[1] - 1 if features.shape[1] > 1 else features.shape[1]
            info = {}
            all_probs: List[Tuple[str, float]] = []
            lang, prob = "en", 0.0
            n_seg = max(1, language_detection_segments)
            for i in range(n_seg):
                seek = i * N_FRAMES
                if i > 0 and seek >= content:
                    break
                size = max(0, min(N_FRAMES, content - seek))
                self._encode(features, seek, size, 0)
                p = self.engine.detect_language([0], st.lang_begin, st.n_langs)[0]
                order = np.argsort(-p, kind="stable")
                all_probs = [(st.lang_codes[j], float(p[j])) for j in order]
                lang, prob = all_probs[0]
                if prob > language_detection_threshold:
                    break
                info.setdefault(lang, []).append(prob)
            else:
                lang = max(info, key=lambda k: len(info[k]))
                prob = max(info[lang])
            return lang, prob, all_probs

    def language_timeline(self, audio: Union[str, BinaryIO, np.ndarray], vad_filter: bool = False, vad_parameters=None,
                          language_candidates: Optional[Sequence[str]] = None,
                          max_windows: Optional[int] = None) -> List[LanguageWindow]:
        """Which language is spoken where: one LanguageWindow(start, end, language, probability, probs) per
        consecutive 30 s window of the audio (of the VAD-collected audio with vad_filter=True; start and end are then
        moved back to file time with restore_speech_timestamps' arithmetic), at most max_windows of them.  Nothing is
        decoded: the windows are encoded max_batch_windows at a time, as the throughput pipeline encodes them, with one
        wm_language_id call per batch; the model lock is held per batch.  language_candidates as in `transcribe`
        (None reads VLOG_AMD_LANGUAGE_CANDIDATES); `probs` is (code, p) over the languages in force, in
        language-token order.  ValueError in an English-only model."""
        if not self.is_multilingual:
            raise ValueError("language_timeline needs a multilingual model (this one is English-only)")
        candidates = self._language_candidates(language_candidates)
        if max_windows is not None and max_windows < 1:
            raise ValueError("max_windows must be >= 1")
        if not isinstance(audio, np.ndarray):
            audio = self._load_audio(audio)
        audio = np.asarray(audio, dtype=np.float32)
        speech_chunks = None
        if vad_filter:
            from .vad import collect_chunks, get_speech_timestamps
            speech_chunks = get_speech_timestamps(audio, _vad_options(vad_parameters), self)
            if not speech_chunks:
                return []
            audio = collect_chunks(audio, speech_chunks)
        with self._lock:
            features = self._features(audio)
        st = self.dims.specials
        wins = timeline_windows(features.shape[1] - 1, max_windows)
        times = window_times(wins, speech_chunks)
        mask = candidate_mask(candidates, st.lang_codes) if candidates is not None else None
        keep = [j for j in range(st.n_langs) if mask is None or mask[j]]
        batch = max(1, self._pipeline().max_batch_windows)
        out: List[LanguageWindow] = []
        for b0 in range(0, len(wins), batch):
            part = wins[b0: b0 + batch]
            with self._lock:
                enc = self.engine.encode(features, [s for s, _ in part], [n for _, n in part])
                self.engine.cross_kv(enc, 0)
                probs, top, top_prob = self.engine.language_id(list(range(len(part))), st.lang_begin, st.n_langs, mask)
            for i in range(len(part)):
                start, end = times[b0 + i]
                out.append(LanguageWindow(start=start, end=end, language=st.lang_codes[int(top[i])],
                                          probability=float(top_prob[i]),
                                          probs=tuple((st.lang_codes[j], float(probs[i, j])) for j in keep)))
        return out

    # ------------------------------------------------------------------ transcribe
    def transcribe(self, audio: Union[str, BinaryIO, np.ndarray], language: Optional[str] = None,
                   task: str = "transcribe", log_progress: bool = False, beam_size: int = 5, best_of: int = 5,
                   patience: float = 1, length_penalty: float = 1, repetition_penalty: float = 1,
                   no_repeat_ngram_size: int = 0,
                   temperature: Union[float, List[float], Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                   compression_ratio_threshold: Optional[float] = 2.4, log_prob_threshold: Optional[float] = -1.0,
                   no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = True,
                   prompt_reset_on_temperature: float = 0.5, initial_prompt: Optional[Union[str, Iterable[int]]] = None,
                   prefix: Optional[str] = None, suppress_blank: bool = True, suppress_tokens: Optional[List[int]] = [-1],
                   without_timestamps: bool = False, max_initial_timestamp: float = 1.0, word_timestamps: bool = False,
                   prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
                   multilingual: Optional[bool] = None, vad_filter: bool = False, vad_parameters=None,
                   max_new_tokens: Optional[int] = None, chunk_length: Optional[int] = None,
                   clip_timestamps: Union[str, List[float]] = "0", hallucination_silence_threshold: Optional[float] = None,
                   hotwords: Optional[str] = None, language_detection_threshold: Optional[float] = 0.5,
                   language_detection_segments: int = 1, sections: Optional[int] = None,
                   sections_in_flight: Optional[int] = None,
                   sequence_bias: Optional[Mapping[Union[str, Tuple[int, ...]], float]] = None,
                   lockstep_fallback: Optional[bool] = None, max_line_width: Optional[int] = None,
                   max_line_count: Optional[int] = None, max_cue_seconds: Optional[float] = None,
                   language_candidates: Optional[Sequence[str]] = None):
        """faster-whisper's `WhisperModel.transcribe`, plus these arguments of this engine:

        multilingual: faster-whisper's code-switching option.  True: every 30 s window is decoded under the language
        detected for that window instead of the file's.  The detection runs on the device inside the window's first
        decode (wm_generate_multilingual: one decoder step from <|startoftranscript|>, the language head, and a kernel
        that writes the chosen language token into the prompt before the prefill), once per window and before the
        fallback temperatures, which then decode with that language; word alignment uses its sot sequence and the next
        window's prompt starts from it.  language_candidates confines the per-window detection too.  info.language,
        info.language_probability and info.all_language_probs keep their meaning (the file-level detection, which is
        also where the first window starts from); every Segment carries `language`, its window's code (None with the
        option off).  A call that names its `language` asks for it in every window: multilingual=True with it raises
        NotImplementedError, as before.  None reads VLOG_AMD_MULTILINGUAL (0 / 1, default off; ignored, and logged
        once, by a call that names its language); an English-only model turns the option off and logs that once.  What is in force is echoed in
        info.transcription_options.multilingual.  Every decode form takes it: sections=N, transcribe_many and
        throughput mode.  Measurement: DESIGN.md §8.

        language_candidates: the language codes this deployment serves, e.g. ["en", "es", "de"].  Used only when
        `language` is None and the model is multilingual (otherwise ignored; the English-only case is logged once):
        language detection then runs through wm_language_id with the candidates' mask, so the language chosen is
        one of them, and info.language_probability / info.all_language_probs are over the candidates only (they sum
        to 1, sorted descending): the model's probabilities conditioned on the language being a candidate.  The
        language_detection_segments windows are encoded in one call and identified in one call; faster-whisper's
        rule (the first window above language_detection_threshold, else the majority of the windows' tops) is
        applied to the per-window results in window order.  None reads VLOG_AMD_LANGUAGE_CANDIDATES
        (comma-separated codes); an empty sequence turns it off whatever the environment says.  An unknown code, a
        duplicate or a malformed variable raises ValueError at the call.  The tuple in force is echoed in
        info.transcription_options.language_candidates (None when off).  WhisperModel.language_timeline reports the
        language per 30 s window without decoding anything.

        max_line_width, max_line_count, max_cue_seconds: caption shaping (vlog_amd/captions.py).  With a width > 0 the
        call decodes exactly as the same call with word_timestamps=True (the shaper needs word times; they move the
        seek to the last word's end, as they do today), and the final stream, after the VAD's times are restored, is
        cut into cues of at most max_line_count (default 2, 1..4) lines of at most max_line_width characters, the
        lines of a cue joined by "\n" in `text`; a cue also ends at a pause above 3 s, when it would last longer than
        max_cue_seconds (default: no limit), and after a sentence end once it is half full (captions.shape_captions
        states the rule).  Every cue is a Segment with its own words and tokens and its source segment's statistics;
        ids run 1, 2, ... over the cues.  max_line_width=None reads VLOG_AMD_MAX_LINE_WIDTH (unset: off), 0 turns
        shaping off whatever the environment says; the other two read VLOG_AMD_MAX_LINE_COUNT and
        VLOG_AMD_MAX_CUE_SECONDS while shaping is on, and raise ValueError when passed while it is off.  What is in
        force is echoed in info.transcription_options (word_timestamps then reads True).  Every decode form takes
        them: sections=N, transcribe_many (per file) and throughput mode.

        sequence_bias: {phrase or token tuple: bias}, deterministic custom-vocabulary boosts (bias > 0) and soft or
        hard bans (bias < 0; -100 is a ban) applied on the device at every decode step of every decode form (beam
        search, the fallback temperatures, sections=N; transformers' SequenceBiasLogitsProcessor over the window's
        generated tokens, segments.build_sequence_bias).  A phrase stands for its tokenisations with and without a
        leading space.  Only the token that COMPLETES an entry is biased, and only when the tokens before it were just
        generated: to favour a multi-token name from its first token, list its prefixes as keys of their own.  The
        bias is part of the distribution: avg_logprob, the fallback thresholds and the beam scores are those of the
        biased distribution.  Default: the VLOG_AMD_SEQUENCE_BIAS file, else none.  The mapping in force is echoed in
        info.transcription_options.sequence_bias.

        sections: cut the file at up to sections - 1 long silences into contiguous sections (seek_state.plan_sections:
        near the even split points, at a VAD chunk join with at least 0.5 s removed, or without VAD at the quietest
        20 ms within 3 s; every section at least 30 s) and decode the sections in lockstep, one ragged engine.generate
        per round over the next window of every section, as transcribe_many decodes files.  Inside a section the
        sequential loop is unchanged (previous-text prompt, timestamp seek, fallback ladder, word-timestamp seek).
        What differs from sections=1: the first window after each cut starts without previous text, as after a prompt
        reset; `initial_prompt` seeds every section; `prefix` applies to section 0 only; the window counter, and so the
        fallback seeds, restart at 0 in every section.  Default: the VLOG_AMD_SECTIONS environment variable, else 1
        (today's one-file loop, untouched).  1..32; not with throughput mode or clip_timestamps.  The bounds chosen are
        in info.transcription_options.section_frames.
        sections_in_flight: sections decoded per round (default: all); 1 decodes them one after another, which gives
        the same transcript and is the baseline of the measurement.
        Measured on one MI355X (large-v3 margin weights, the worker's call on a 12-minute clip, 591 s after VAD;
        tools/bench_worker_call.py --sections, profiles/worker_call_sections.jsonl): sections -> RTFx /
        rows per decoder pass / ms per pass: 1 -> 144 / 5.0 / 2.11, 2 -> 237 / 9.6 / 2.32, 4 -> 345 / 18.3 / 2.90,
        8 -> 476 / 30.0 / 3.11, 16 (13 after the 30 s rule) -> 551 / 48.3 / 3.50; the same 13 sections one after
        another (sections_in_flight=1): 103.  The doublings gain x1.65, 1.46, 1.38, 1.16 (every cut adds a short
        window, and load, VAD and log-mel are not shared), so by the rule of transcribe_many's max_files (the last
        doubling that gains at least x1.5) the recommended value is 2; the default stays 1.

        lockstep_fallback: how a lockstep round (sections > 1; one window per round has nothing to share) decodes the
        windows that need a fallback temperature.  False: each alone, with generate_with_fallback's calls, bit-identical
        to the one-file loop.  True: by levels, the windows that fail temperature i together in ONE seeded
        engine.generate at temperature i + 1 (rows = failing windows x best_of, every window with its own seed
        window + i + 1; a sampled first pass is one such call too).  A window's rows then share decoder passes with
        other windows' rows, so its result agrees with the solo decode to f32 rounding, not bit for bit.  Default: the
        VLOG_AMD_LOCKSTEP_FALLBACK environment variable (0 / 1), else False.  Echoed in
        info.transcription_options.lockstep_fallback.  Throughput mode has its own batched re-decode and ignores it.
        Measurement: DESIGN.md §8 (tools/bench_worker_call.py --lockstep-fallback)."""
        args = dict(locals())
        call = _resolve_call(self, "transcribe", args)
        if self.throughput:
            # opt-in throughput mode for the UNCHANGED worker (VLOG_AMD_THROUGHPUT=1): its call
            # transcribe(wav, language, task, beam_size=5, vad_filter=True) runs as BatchedInferencePipeline:
            # VAD-bounded windows decoded independently in large batches (no previous-text prompt), with
            # timestamps kept so the worker's WebVTT still gets per-segment times.
            return self._pipeline()._transcribe(audio, call)
        sections, in_flight = call.args["sections"], call.args["sections_in_flight"]
        if sections > 1 and not isinstance(audio, np.ndarray):
            audio = self._load_audio(audio)     # (the cuts without VAD are chosen on the samples)
        file, tokenizer, options = self._prepare_file(audio, call)
        bounds = self._plan_sections(audio, file.features, file.speech_chunks, sections) if sections > 1 else None
        if bounds is not None:
            options.section_frames = bounds
        if bounds is not None and len(bounds) > 1:
            gen = self._generate_sections(file.features, tokenizer, options, bounds, in_flight or len(bounds))
        else:
            gen = self.generate_segments(file.features, tokenizer, options)
        return _finished(gen, file.speech_chunks, options), file.info(options)

    def _plan_sections(self, audio: np.ndarray, features: torch.Tensor, speech_chunks, n: int) -> List[Tuple[int, int]]:
        """plan_sections for one prepared file: at the VAD chunk joins when VAD ran, else at the quietest 20 ms frames
        of the samples (wm_frame_energy)."""
        content = features.shape[1] - 1
        if speech_chunks is not None:
            return plan_sections(content, n, joins=chunk_joins(speech_chunks))
        if content < 2 * N_FRAMES:              # one section whatever the energies say
            return plan_sections(content, n)
        with self._lock:
            energy = self.engine.frame_energy_db(
                torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)), ENERGY_FRAME_MEL * HOP_LENGTH)
        return plan_sections(content, n, energy=energy)

    def _load_file(self, audio, language: Optional[str], vad_filter: bool, vad_parameters, clip_timestamps="0",
                   language_detection_segments: int = 1, language_detection_threshold: Optional[float] = 0.5,
                   language_candidates: Optional[Tuple[str, ...]] = None) -> _File:
        """The sequential path's file: load, VAD-collect, then log-mel of the collected speech, then the language."""
        if not isinstance(audio, np.ndarray):
            audio = self._load_audio(audio)
        audio = np.asarray(audio, dtype=np.float32)
        duration = audio.shape[0] / SAMPLE_RATE
        speech_chunks = vad_opts = None
        if vad_filter and clip_timestamps in _NO_CLIPS:
            from .vad import collect_chunks, get_speech_timestamps
            vad_opts = _vad_options(vad_parameters)
            speech_chunks = get_speech_timestamps(audio, vad_opts, self)
            audio = collect_chunks(audio, speech_chunks)
        with self._lock:
            features = self._features(audio)
        # only this path maps a named non-English language to "en" in an English-only model (and warns); it detects
        # whatever the VAD left
        return _File(features, duration, audio.shape[0] / SAMPLE_RATE, vad_opts,
                     *self._file_language(language, features, language_detection_segments, language_detection_threshold,
                                          language_candidates, english_only_remap=True), speech_chunks=speech_chunks)

    def _file_language(self, language: Optional[str], features: torch.Tensor, detection_segments: int,
                       detection_threshold: Optional[float], candidates: Optional[Tuple[str, ...]], *,
                       english_only_remap: bool = False, detect: bool = True):
        """Which language a file gets -> (language, probability, all_language_probs, the candidates in force for it).
        A named language holds (english_only_remap: an English-only model maps another one to "en" and warns);
        language=None is detected under the call's `candidates`, or is "en" in an English-only model and with
        detect=False."""
        if language is not None:
            if english_only_remap and not self.is_multilingual and language != "en":
                logger.warning("English-only model used with language=%s; using 'en'", language)
                language = "en"
            return language, 1.0, None, None
        if not (self.is_multilingual and detect):
            return "en", 1.0, None, candidates
        return (*self.detect_language(features=features, language_detection_segments=detection_segments,
                                      language_detection_threshold=detection_threshold or 0.5,
                                      language_candidates=candidates or ()), candidates)

    def _prepare_file(self, audio, call: _Call, f: int = 0):
        """What `transcribe` does for file f of a call before its seek loop: load, VAD, log-mel, language, tokenizer,
        options.  -> (_File, tokenizer, options)"""
        a = call.args
        file = self._load_file(audio, a["language"][f], a["vad_filter"], a["vad_parameters"], a["clip_timestamps"],
                               a["language_detection_segments"], a["language_detection_threshold"],
                               a["language_candidates"])
        tokenizer = self.tokenizer(task=a["task"], language=file.language)
        return file, tokenizer, call.options(self, tokenizer, f, file.language_candidates)

    # ------------------------------------------------------------------ prompt / generate
    def get_prompt(self, tokenizer: Tokenizer, previous_tokens: List[int], without_timestamps: bool = False,
                   prefix: Optional[str] = None, hotwords: Optional[str] = None) -> List[int]:
        return segs.build_prompt(tokenizer.encode, tokenizer.sot_sequence, tokenizer.sot_prev, tokenizer.no_timestamps,
                                 tokenizer.timestamp_begin, self.max_length, previous_tokens, without_timestamps,
                                 prefix, hotwords)

    def _generate(self, prompt: List[int], options: TranscriptionOptions, temperature: float, max_length: int,
                  seed: int, slot: int = 0, lang_pos: int = -1) -> _GenOut:
        """One window's decode at one temperature.  lang_pos >= 0 (multilingual=True, the window's first decode): the
        engine identifies the window and decodes it under that language in the same call (wm_generate_multilingual;
        the prompt holds a placeholder at lang_pos); the result names the language."""
        st = self.dims.specials
        kw = dict(language_auto=self._language_auto(options, [lang_pos])) if lang_pos >= 0 else {}
        res, *lang = self.engine.generate(
            [slot], [prompt], max_length=max_length, num_hypotheses=options.best_of if temperature > 0 else 1,
            seed=seed, suppress_tokens=options.suppress_tokens,
            sot_index=prompt.index(st.sot) if st.sot in prompt else -1, **_decode_kwargs(options, temperature), **kw)
        r = res[0]
        return _GenOut(r.tokens, r.score, r.no_speech_prob,
                       st.lang_codes[int(lang[1][0][0])] if lang_pos >= 0 else None)

    def generate_with_fallback(self, prompt: List[int], tokenizer: Tokenizer, options: TranscriptionOptions,
                               seed: int = 0, slot: int = 0, first: Optional[_GenOut] = None):
        """faster-whisper generate_with_fallback -> (result, avg_logprob, temperature, compression_ratio), decoding
        against the window in cross slot `slot`.  `first`: the result at temperatures[0] when a shared pass already
        computed it (transcribe_many); the ladder then only runs the temperatures after it."""
        max_length = window_max_length(prompt, options.max_new_tokens, self.max_length)
        return fallback_ladder(lambda t, sd: self._generate(prompt, options, t, max_length, sd, slot), tokenizer.decode,
                               options, seed=seed, first=first)

    # ------------------------------------------------------------------ seek loop
    def _segment(self, d: dict) -> Segment:
        words = d.pop("words")
        return Segment(words=[_word(w) for w in words] if words is not None else None, **d)

    def generate_segments(self, features: torch.Tensor, tokenizer: Tokenizer, options: TranscriptionOptions):
        """The one-file driver of vlog_amd/seek_state.py SeekState (faster-whisper generate_segments)."""
        state = SeekState(features.shape[1] - 1, tokenizer, options, self.max_length, self.frames_per_second)
        while True:
            req = state.next_request()
            if req is None:
                return
            # one lock scope from the encode to the word alignment: the alignment reads the window's encoder
            # output from slot 0, which another thread's transcribe must not replace in between
            with self._lock:
                self._use_cross_form(options.beam_size)
                self._encode(features, req.seek, req.size, 0)
                first = None
                if state.multilingual and options.temperatures:
                    # the window's language is detected once, inside its first decode; the fallback temperatures
                    # then run with the prompt that carries it
                    first = self._generate(req.prompt, options, options.temperatures[0], req.max_length, req.window,
                                           lang_pos=req.lang_pos)
                    state.set_window_language(first.language)
                decode = self.generate_with_fallback(req.prompt, tokenizer, options, seed=req.window, first=first)
                out = state.consume(decode, lambda current, size, last, tokenizer=tokenizer: self.add_word_timestamps(
                    [current], tokenizer, size, options.prepend_punctuations, options.append_punctuations, last))
            for d in out:
                yield self._segment(d)

    def _lockstep_round(self, batch, reserved: List[int], emit, features_of=None,
                        shared: Optional[torch.Tensor] = None) -> None:
        """One round of run_lockstep on the GPU, for transcribe_many (items = files, each with its own log-mel,
        features_of(item)) and for the sections of one file (`shared`: the one log-mel every item reads).
        batch: [(item, state, request)], entry i = cross slot i.  Reserve, ONE encoder call, cross_kv into slots
        0..nb-1, the ragged first pass at temperatures[0] grouped by suppress list, the fallback passes (solo, or with
        options.lockstep_fallback by levels: the windows that fail a temperature re-decode in one seeded generate per
        suppress list against the slots the round filled), per-item word alignment; emit(item, segment dicts).
        reserved: [slots reserved by the caller's earlier rounds]."""
        nb = len(batch)
        opt0 = batch[0][1].options              # everything but the per-file prompt parts is common to the items
        temps = opt0.temperatures
        t0 = temps[0] if temps else 0.0
        sampling = t0 > 0
        levels = bool(opt0.lockstep_fallback)
        # by levels a round may decode nb windows x best_of rows: reserved once, so no level re-allocates the
        # hypothesis state while the slots are in use
        per = max(opt0.beam_size, opt0.best_of) if levels else (opt0.best_of if sampling else opt0.beam_size)
        sot = self.dims.specials.sot
        with self._lock:                        # one lock scope per round: the slots hold this round's windows
            self._use_cross_form(opt0.beam_size)      # (a no-op unless another caller changed the form)
            if nb != reserved[0]:
                self.engine.reserve(nb, max(nb * max(per, 1), 8))
                reserved[0] = nb
            if shared is not None:
                # the items are ranges of one log-mel: the encoder reads each window where it lies
                enc = self.engine.encode(shared, [req.seek for _, _, req in batch], [req.size for _, _, req in batch])
            else:
                # ONE encoder call over the round's windows, into slots 0..nb-1: window i's frames are copied to columns
                # [i * 3000, i * 3000 + size) of one matrix (the encoder zero-pads each window to 3000 frames itself)
                mel = torch.zeros((self.dims.n_mels, nb * N_FRAMES), device=features_of(batch[0][0]).device,
                                  dtype=torch.float32)
                for i, (f, _, req) in enumerate(batch):
                    mel[:, i * N_FRAMES: i * N_FRAMES + req.size] = features_of(f)[:, req.seek: req.seek + req.size]
                enc = self.engine.encode(mel, [i * N_FRAMES for i in range(nb)], [req.size for _, _, req in batch])
            self.engine.cross_kv(enc, 0)

            def shared_pass(idx, t, seeds=None, auto=False):
                """entries idx decoded together at temperature t, one generate per suppress list; seeds (sampling):
                one per entry, so every window draws as in a call of its own (engine.generate seeds).  auto (the first
                pass of a multilingual round): the entries with the option on choose their language in the call"""
                out: List[Optional[_GenOut]] = [None] * len(idx)
                groups: dict = {}
                for k, i in enumerate(idx):     # the suppress list is one per generate call, and so is the language mask
                    o = batch[i][1].options
                    mask = o.language_candidates if auto and batch[i][2].lang_pos >= 0 else None
                    groups.setdefault((tuple(o.suppress_tokens), mask), []).append(k)
                for (sup, _), ks in groups.items():
                    members = [idx[k] for k in ks]
                    prompts = [batch[i][2].prompt for i in members]
                    kw = {}
                    if t > 0:                   # the arguments _generate passes for a sampled decode
                        kw = dict(num_hypotheses=opt0.best_of, seeds=[seeds[k] for k in ks])
                    pos = [batch[i][2].lang_pos if auto else -1 for i in members]
                    if any(p >= 0 for p in pos):
                        first_auto = members[next(j for j, p in enumerate(pos) if p >= 0)]
                        kw["language_auto"] = self._language_auto(batch[first_auto][1].options, pos)
                    # (the group's suppress list, not opt0's; no `seed`: a sampled pass has its `seeds`)
                    res, *lang = self.engine.generate(
                        members, prompts, max_length=[batch[i][2].max_length for i in members],
                        suppress_tokens=list(sup), sot_index=[p.index(sot) if sot in p else -1 for p in prompts],
                        **_decode_kwargs(opt0, t), **kw)
                    for j, (k, r) in enumerate(zip(ks, res)):
                        out[k] = _GenOut(r.tokens, r.score, r.no_speech_prob)
                        if pos[j] >= 0:
                            out[k].language = self.dims.specials.lang_codes[int(lang[1][0][j])]
                return out

            def first_pass(idx):
                if sampling and levels:
                    return shared_pass(idx, t0, [batch[i][2].window for i in idx], auto=True)
                if sampling:
                    # a sampled pass draws noise keyed on (seed, hypothesis index): a file's draws would depend on
                    # its place in the round, so each window decodes alone, with generate_with_fallback's call
                    return [self._generate(batch[i][2].prompt, batch[i][1].options, t0, batch[i][2].max_length,
                                           batch[i][2].window, slot=i, lang_pos=batch[i][2].lang_pos) for i in idx]
                return shared_pass(idx, t0, auto=True)

            def fallback_generate(i, t, seed):
                _, state, req = batch[i]
                return self._generate(req.prompt, state.options, t, req.max_length, seed, slot=i)

            def align(i, current, size, last, tokenizer=None):
                # (a round without multilingual: one wm_align_batch per item, as before)
                _, state, _ = batch[i]
                o = state.options
                return self.add_word_timestamps([current], tokenizer or state.tokenizer, size, o.prepend_punctuations,
                                                o.append_punctuations, last, slots=[i])

            def align_group(items):
                # a multilingual round: the items of one language in ONE wm_align_batch, each against its own slot and
                # with its own last-speech time (items: seek_state.consume_round_grouped)
                return self.add_word_timestamps([it[1] for it in items], items[0][4], [it[2] for it in items],
                                                opt0.prepend_punctuations, opt0.append_punctuations,
                                                [it[3] for it in items], slots=[it[0] for it in items])

            if levels:
                decode_round_levels(batch, first_pass, shared_pass, align if opt0.word_timestamps else None, emit,
                                    align_group)
            else:
                decode_round_with(batch, first_pass, fallback_generate, align if opt0.word_timestamps else None, emit,
                                  align_group)

    def _generate_sections(self, features: torch.Tensor, tokenizer: Tokenizer, options: TranscriptionOptions,
                           bounds: Sequence[Tuple[int, int]], in_flight: int):
        """The sectioned driver (transcribe(sections=N)): one SeekState per frame range of `bounds` (plan_sections),
        decoded in lockstep with at most `in_flight` sections per round, as transcribe_many decodes files; the model
        lock is held per round.  A generator: after every round it yields, in section order, the segments that are now
        final (a section's segments wait until every earlier section has ended), with id 1, 2, ... in output order
        and seek the absolute frame."""
        content = features.shape[1] - 1
        states: dict = {}
        held: List[List[Segment]] = [[] for _ in bounds]
        reserved = [0]
        head, next_id = 0, 1

        def open_section(k: int) -> SeekState:
            states[k] = SeekState(content, tokenizer, options, self.max_length, self.frames_per_second,
                                  clip_frames=bounds[k])
            return states[k]

        def decode_round(batch):
            self._lockstep_round(batch, reserved, lambda k, out: held[k].extend(self._segment(d) for d in out),
                                 shared=features)

        for _ in iter_lockstep(len(bounds), in_flight, open_section, decode_round):
            while head < len(bounds):
                for seg in held[head]:
                    seg.id = next_id
                    next_id += 1
                    yield seg
                held[head] = []
                if head not in states or states[head].next_request() is not None:
                    break                       # the head section has windows left (or has not started yet)
                head += 1

    def transcribe_many(self, audios: Sequence[Union[str, BinaryIO, np.ndarray]],
                        language: Union[None, str, Sequence[Optional[str]]] = None, task: str = "transcribe",
                        log_progress: bool = False, beam_size: int = 5, best_of: int = 5, patience: float = 1,
                        length_penalty: float = 1, repetition_penalty: float = 1, no_repeat_ngram_size: int = 0,
                        temperature: Union[float, List[float], Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                        compression_ratio_threshold: Optional[float] = 2.4, log_prob_threshold: Optional[float] = -1.0,
                        no_speech_threshold: Optional[float] = 0.6, condition_on_previous_text: bool = True,
                        prompt_reset_on_temperature: float = 0.5, initial_prompt=None, prefix=None,
                        suppress_blank: bool = True, suppress_tokens: Optional[List[int]] = [-1],
                        without_timestamps: bool = False, max_initial_timestamp: float = 1.0,
                        word_timestamps: bool = False, prepend_punctuations: str = "\"'“¿([{-",
                        append_punctuations: str = "\"'.。,，!！?？:：”)]}、", multilingual: Optional[bool] = None,
                        vad_filter: bool = False, vad_parameters=None, max_new_tokens: Optional[int] = None,
                        chunk_length: Optional[int] = None, clip_timestamps: Union[str, List[float]] = "0",
                        hallucination_silence_threshold: Optional[float] = None, hotwords=None,
                        language_detection_threshold: Optional[float] = 0.5, language_detection_segments: int = 1,
                        max_files: int = 16,
                        sequence_bias: Optional[Mapping[Union[str, Tuple[int, ...]], float]] = None,
                        lockstep_fallback: Optional[bool] = None, max_line_width: Optional[int] = None,
                        max_line_count: Optional[int] = None, max_cue_seconds: Optional[float] = None,
                        language_candidates: Optional[Sequence[str]] = None):
        """`transcribe` for several files at once in the sequential (parity) mode -> [(list_of_segments, info)] in
        input order; each file gets what `transcribe(file, same arguments)` gives for it alone.

        The files decode in lockstep: each round takes the next 30 s window of every file in flight (at most
        `max_files`; when a file ends the next pending one takes its place), encodes them in one call, and decodes
        them in ONE ragged `engine.generate` at temperatures[0] (rows = files x beam), every file with its own seek
        position and previous-text prompt.  The sequential decode is launch-bound at one file's few rows (DESIGN.md
        §10.5), so the extra files' rows ride along in the same decoder passes.  A window that needs a fallback
        temperature is re-decoded alone, with the calls `generate_with_fallback` makes (same seeds, same best_of);
        word timestamps are aligned per file against its own slot.  language / initial_prompt / hotwords / prefix take
        one value, or a list / tuple with one value per file (pass token ids of ONE initial prompt as a numpy array or
        repeat them per file).  Files of different languages share rounds (the prompt carries the language); files whose
        suppress lists differ are decoded in separate generate calls of the round.  sequence_bias (see `transcribe`) is
        ONE mapping for all files, as the engine holds one table per generate call: a per-file list raises ValueError.
        max_files: files in flight.  Measured on one MI355X (large-v3 margin weights, the worker's call on 5-minute
        clips, tools/bench_worker_call.py --files, profiles/worker_call_many.jsonl): files in flight -> RTFx summed
        over the files / ms per decoder pass: 1 -> 133 / 2.10, 2 -> 240 / 2.31, 4 -> 365 / 3.03, 8 -> 593 / 3.64,
        16 -> 924 / 4.45, 32 -> 1379 / 5.56.  The curve has no sharp knee: a pass never costs twice what half the rows
        cost, so every doubling still pays (x1.80, 1.52, 1.62, 1.56, 1.49), while each file's own latency grows (2.3 s
        alone, 5.2 s at 16, 7.0 s at 32 for a 5-minute clip).  The default is the last doubling that gains at least
        x1.5 (the 16-files line); a worker that only wants throughput can pass 32.
        lockstep_fallback (see `transcribe`; default VLOG_AMD_LOCKSTEP_FALLBACK, else False): True decodes the
        fallback temperatures by levels, the round's failing windows together in one seeded generate per temperature;
        each file then gets what `transcribe` gives for it alone to f32 rounding, not bit for bit.
        max_line_width, max_line_count, max_cue_seconds (see `transcribe`): caption shaping, applied to every file's
        segments on their own (ids 1, 2, ... per file).
        language_candidates (see `transcribe`): ONE sequence of codes for all files, in force for every file whose
        language is None; a per-file list of lists raises ValueError.
        With throughput mode on, this is BatchedInferencePipeline.transcribe_many."""
        args = dict(locals())
        n = len(audios)
        call = _resolve_call(self, "transcribe_many", args, n)
        if self.throughput:
            return self._pipeline()._transcribe_many(audios, call)
        files: dict = {}
        results: List[List[Segment]] = [[] for _ in range(n)]

        def open_file(f: int) -> SeekState:
            # per file, as `transcribe`: load, VAD, log-mel, language detection (with language=None), options
            file, tokenizer, options = self._prepare_file(audios[f], call, f)
            files[f] = (file, options)
            return SeekState(file.features.shape[1] - 1, tokenizer, options, self.max_length, self.frames_per_second)

        reserved = [0]

        def decode_round(batch):
            self._lockstep_round(batch, reserved, lambda f, out: results[f].extend(self._segment(d) for d in out),
                                 features_of=lambda f: files[f][0].features)

        def close_file(f: int) -> None:
            files[f][0].features = None             # the file's log-mel leaves the device with its last window

        run_lockstep(n, max_files, open_file, decode_round, close_file)
        return [(list(_finished(iter(results[f]), file.speech_chunks, options)), file.info(options))
                for f, (file, options) in sorted(files.items())]

    # ------------------------------------------------------------------ forced alignment
    def align(self, audio: Union[str, BinaryIO, np.ndarray], text: Union[str, Sequence[str]],
              language: Optional[str] = None, task: str = "transcribe", vad_filter: bool = False, vad_parameters=None,
              max_window_tokens: int = 224, max_cue_chars: Optional[int] = 84, median_filter_width: int = 7,
              prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、"
              ) -> Tuple[List[Segment], AlignmentInfo]:
        """Forced alignment: time a GIVEN transcript against the audio (re-timing an edited transcript; nothing is
        decoded).  text: a str (one caption line per "\n") or a sequence of lines.  -> (segments, AlignmentInfo):
        one Segment per line, or its cues when the line is longer than max_cue_chars (None: never cut), each with
        its Words; ids 1, 2, ...; temperature and no_speech_prob 0.0; avg_logprob the mean log-probability the
        model gives the line's tokens.

        The loop (vlog_amd/forced_align.py): every 30 s window is offered the next max_window_tokens tokens of
        whole words, runs the teacher-forced pass with the alignment heads captured, and the open-end DTW
        (wm_align_open_batch) returns the path and how many text rows the window's audio reached; the words whose
        end was reached are timed and the next window starts at the last of them.  Words left when the audio ends get
        start = end = duration and probability 0.0 (info.unaligned_words).  vad_filter=True runs the loop on the
        collected speech and maps the times back (a silent window gives the DTW nothing to hold on to).
        Audio loading, resampling, log-mel and language detection are transcribe's; the whole call holds the
        model lock.  Raises ValueError in throughput mode and for an empty text."""
        from . import forced_align as fa
        if self.throughput:
            raise ValueError("align is the sequential mode's; throughput mode has no forced alignment")
        if task not in ("transcribe", "translate"):
            raise ValueError(f"unknown task {task!r}")
        if not fa.split_lines(text):
            raise ValueError("align: empty text")
        with self._lock:
            file = self._load_file(audio, language, vad_filter, vad_parameters)
            features, tokenizer = file.features, self.tokenizer(task=task, language=file.language)
            heads = self.dims.default_alignment_heads()
            self._use_cross_form(1)             # one teacher-forced row set per window, as a greedy decode's alignment

            def align_window(seek: int, size: int, tokens: List[int]):
                self._encode(features, seek, size, 0)
                return self.engine.align_open_batch([0], tokenizer.sot_sequence, [tokens], [size], heads,
                                                    median_filter_width)[0]

            out, stats = fa.forced_align(tokenizer, text, features.shape[1] - 1, file.duration_after_vad, align_window,
                                         max_window_tokens, max_cue_chars, prepend_punctuations, append_punctuations,
                                         self.frames_per_second, self.tokens_per_second)
        segments = list(_finished((self._segment(d) for d in out), file.speech_chunks))
        info = AlignmentInfo(language=file.language, language_probability=file.language_probability,
                             duration=file.duration, duration_after_vad=file.duration_after_vad,
                             windows=stats["windows"], unaligned_words=stats["unaligned_words"],
                             window_rows=stats["window_rows"])
        return segments, info

    # ------------------------------------------------------------------ word timestamps
    def find_alignment(self, tokenizer: Tokenizer, text_tokens: List[List[int]], num_frames: Union[int, Sequence[int]],
                       median_filter_width: int = 7, slots: Optional[Sequence[int]] = None) -> List[List[dict]]:
        """faster-whisper find_alignment over CTranslate2 align: teacher-forced decoder pass over
        [sot_sequence, <|notimestamps|>, text, <|endoftext|>] with the alignment heads' cross-attention
        captured on the GPU, normalise + median filter + DTW on the GPU — every segment group of the call in
        ONE batched align (wm_align_batch).  Group i reads the encoder output in slot slots[i] (default 0) and
        num_frames[i] mel frames (an int applies to every group)."""
        n = len(text_tokens)
        nfs = list(num_frames) if isinstance(num_frames, (list, tuple, np.ndarray)) else [int(num_frames)] * n
        sl = list(slots) if slots is not None else [0] * n
        todo = [i for i in range(n) if text_tokens[i]]
        aligned = dict(zip(todo, self.engine.align_batch([sl[i] for i in todo], tokenizer.sot_sequence,
                                                         [text_tokens[i] for i in todo], [nfs[i] for i in todo],
                                                         self.dims.default_alignment_heads(), median_filter_width)))
        out = []
        for i, tt in enumerate(text_tokens):
            if not tt:
                out.append([])
                continue
            probs, text_idx, time_idx = aligned[i]
            words, word_tokens = tokenizer.split_to_word_tokens(tt + [tokenizer.eot])
            if len(word_tokens) <= 1:
                out.append([])
                continue
            wb = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
            if len(wb) <= 1:
                out.append([])
                continue
            jumps = np.pad(np.diff(text_idx), (1, 0), constant_values=1).astype(bool)
            jump_times = time_idx[jumps] / self.tokens_per_second
            starts = jump_times[wb[:-1]]
            ends = jump_times[wb[1:]]
            wprob = _word_means(probs, wb)
            out.append([dict(word=w, tokens=t, start=float(s), end=float(e), probability=p)
                        for w, t, s, e, p in zip(words, word_tokens, starts, ends, wprob)])
        return out

    def add_word_timestamps(self, segments: List[List[dict]], tokenizer: Tokenizer, num_frames: Union[int, Sequence[int]],
                            prepend_punctuations: str, append_punctuations: str, last_speech_timestamp: float,
                            slots: Optional[Sequence[int]] = None) -> float:
        """faster-whisper add_word_timestamps: segment group i (one window's segments) is aligned against the
        encoder output in slot slots[i] with num_frames[i] frames (BatchedInferencePipeline passes one group
        per window of a batch).  last_speech_timestamp: one time threaded through the groups in order, or a list with
        one time per group (groups of different files or sections, aligned in one call: each keeps its own) -> a list."""
        per_group = isinstance(last_speech_timestamp, (list, tuple))
        lasts = list(last_speech_timestamp) if per_group else None
        if len(segments) == 0:
            return lasts if per_group else last_speech_timestamp
        text_tokens, per_seg = [], []
        for segment in segments:
            st = [[t for t in sub["tokens"] if t < tokenizer.eot] for sub in segment]
            text_tokens.append(list(itertools.chain.from_iterable(st)))
            per_seg.append(st)
        alignments = self.find_alignment(tokenizer, text_tokens, num_frames, slots=slots)
        med_max = []
        for alignment in alignments:
            durs = np.array([w["end"] - w["start"] for w in alignment])
            durs = durs[durs.nonzero()]
            med = min(0.7, float(np.median(durs))) if len(durs) > 0 else 0.0
            mx = med * 2
            if len(durs) > 0:
                marks = ".。!！?？"
                for i in range(1, len(alignment)):
                    if alignment[i]["end"] - alignment[i]["start"] > mx:
                        if alignment[i]["word"] in marks:
                            alignment[i]["end"] = alignment[i]["start"] + mx
                        elif alignment[i - 1]["word"] in marks:
                            alignment[i]["start"] = alignment[i]["end"] - mx
            merge_punctuations(alignment, prepend_punctuations, append_punctuations)
            med_max.append((med, mx))
        for si, segment in enumerate(segments):
            wi = 0
            time_offset = segment[0]["seek"] / self.frames_per_second
            med, mx = med_max[si]
            if per_group:
                last_speech_timestamp = lasts[si]
            for ssi, sub in enumerate(segment):
                saved = 0
                words = []
                while wi < len(alignments[si]) and saved < len(per_seg[si][ssi]):
                    timing = alignments[si][wi]
                    if timing["word"]:
                        words.append(dict(word=timing["word"], start=round(time_offset + timing["start"], 2),
                                          end=round(time_offset + timing["end"], 2), probability=timing["probability"],
                                          tokens=timing["tokens"]))
                    saved += len(timing["tokens"])
                    wi += 1
                if words:
                    if words[0]["end"] - last_speech_timestamp > med * 4 and (
                            words[0]["end"] - words[0]["start"] > mx
                            or (len(words) > 1 and words[1]["end"] - words[0]["start"] > mx * 2)):
                        if len(words) > 1 and words[1]["end"] - words[1]["start"] > mx:
                            boundary = max(words[1]["end"] / 2, words[1]["end"] - mx)
                            words[0]["end"] = words[1]["start"] = boundary
                        words[0]["start"] = max(0, words[0]["end"] - mx)
                    if sub["start"] < words[0]["end"] and sub["start"] - 0.5 > words[0]["start"]:
                        words[0]["start"] = max(0, min(words[0]["end"] - med, sub["start"]))
                    else:
                        sub["start"] = words[0]["start"]
                    if sub["end"] > words[-1]["start"] and sub["end"] + 0.5 < words[-1]["end"]:
                        words[-1]["end"] = max(words[-1]["start"] + med, sub["end"])
                    else:
                        sub["end"] = words[-1]["end"]
                    last_speech_timestamp = sub["end"]
                segments[si][ssi]["words"] = words
            if per_group:
                lasts[si] = last_speech_timestamp
        return lasts if per_group else last_speech_timestamp


@dataclass
class WindowResult:
    index: int
    seek: int
    size: int
    time_offset: float
    tokens: List[int]
    avg_logprob: float
    temperature: float
    compression_ratio: float
    no_speech_prob: float
    segments: Optional[List[dict]] = None      # split (and, with word timestamps, word-aligned) segments
    language: Optional[str] = None             # multilingual=True: the language detected for the window


class BatchedInferencePipeline:
    """Throughput mode (faster-whisper `BatchedInferencePipeline`): the file's 30 s windows — fixed, or bounded
    by VAD speech chunks — are decoded independently (no previous-text prompt) in large batches on one GPU:
    one encoder call per batch, cross-KV for every window resident in HBM, one on-device batched
    greedy/beam decode, then a batched re-decode of the windows that need temperature fallback.
    Window-sharding over several GPUs: vlog_amd/shard.py."""

    def __init__(self, model: WhisperModel, max_batch_windows: int = 150):
        self.model = model
        self.max_batch_windows = max_batch_windows
        # finished windows leave the decode passes (greedy: the row-set decode's compaction; beam: finished windows'
        # hypotheses); VLOG_AMD_COMPACT=0 keeps every row to the batch's end
        self.compact = os.environ.get("VLOG_AMD_COMPACT", "1") != "0"

    # -- windows of the whole-file feature matrix
    @staticmethod
    def fixed_windows(content_frames: int) -> List[Tuple[int, int]]:
        return [(s, min(N_FRAMES, content_frames - s)) for s in range(0, content_frames, N_FRAMES)]

    @staticmethod
    def vad_windows(chunks: List[dict], content_frames: int) -> List[Tuple[int, int]]:
        """Merge speech chunks (sample ranges) greedily into windows of at most 30 s (frame ranges)."""
        out: List[Tuple[int, int]] = []
        cur_s = cur_e = None
        for c in chunks:
            s, e = c["start"] // HOP_LENGTH, min(content_frames, -(-c["end"] // HOP_LENGTH))
            while e - s > N_FRAMES:                          # a single over-long chunk: cut in 30 s pieces
                if cur_s is not None:
                    out.append((cur_s, cur_e - cur_s)); cur_s = None
                out.append((s, N_FRAMES)); s += N_FRAMES
            if cur_s is None:
                cur_s, cur_e = s, e
            elif e - cur_s <= N_FRAMES:
                cur_e = e
            else:
                out.append((cur_s, cur_e - cur_s)); cur_s, cur_e = s, e
        if cur_s is not None and cur_e > cur_s:
            out.append((cur_s, cur_e - cur_s))
        return out

    def decode_windows(self, features: torch.Tensor, windows: Sequence[Tuple[int, int]], time_offsets: Sequence[float],
                       tokenizer: Tokenizer, options: TranscriptionOptions, seed: int = 0,
                       files: Optional[Sequence[int]] = None,
                       seek_bases: Optional[Sequence[int]] = None,
                       last_speech: Optional[dict] = None) -> List[WindowResult]:
        """files: the source file of each window when windows of several files share batches (transcribe_many):
        word timestamps then keep one last-speech time per file.  seek_bases: frame offset of each window's file
        inside `features` (its segments and word timestamps are reported relative to the file).  last_speech:
        the caller's per-file last-speech times (word-timestamp heuristics); owned by ONE transcribe call, so
        threads sharing this pipeline never see each other's state."""
        if last_speech is None:
            last_speech = {}
        m = self.model
        eng = m.engine
        st = m.dims.specials
        if options.prefix is not None:
            raise NotImplementedError("initial_prompt / clip_timestamps / prefix in throughput mode")
        ip: List[int] = []
        if options.initial_prompt:
            ip = (tokenizer.encode(" " + options.initial_prompt.strip()) if isinstance(options.initial_prompt, str)
                  else list(options.initial_prompt))
        # one prompt for every window (wm_generate takes one prompt length): hotwords fit, a prefix does not
        prompt = m.get_prompt(tokenizer, ip, options.without_timestamps, hotwords=options.hotwords)
        max_length = min(m.max_length, len(prompt) + options.max_new_tokens) if options.max_new_tokens else m.max_length
        per = max(options.beam_size, options.best_of, 1)
        # cross-attention form per batch (WhisperModel._use_cross_form), chosen for the FIRST pass: greedy
        # (beam 1) decodes one row per window -> factored; beam groups -> projected (large-v3, 150 windows, beam 5
        # + words: 1474 vs 1237 RTFx).  The temperature-fallback passes (best_of rows) reuse the batch's form.
        auto_form = os.environ.get("VLOG_AMD_CROSS_AUTO", "1") != "0" and not eng.option("cross_fp8", 0)
        prev_form = eng.option("cross_mode")
        try:
            return self._decode_batches(features, windows, time_offsets, tokenizer, options, seed, files, seek_bases,
                                        last_speech, prompt, max_length, per, auto_form)
        finally:
            if auto_form:                      # leave the engine in the form the caller had configured
                with m._lock:
                    eng.set_option("cross_mode", 1 if prev_form is None else prev_form)

    def _decode_batches(self, features, windows, time_offsets, tokenizer, options, seed, files, seek_bases,
                        last_speech, prompt, max_length, per, auto_form) -> List[WindowResult]:
        m = self.model
        eng = m.engine
        st = m.dims.specials
        out: List[WindowResult] = []
        B = self.max_batch_windows
        for b0 in range(0, len(windows), B):
            wins = list(windows[b0: b0 + B])
            with m._lock:
                if auto_form:
                    m._use_cross_form(options.beam_size)
                eng.reserve(len(wins), len(wins) * per)
                enc = eng.encode(features, [w[0] for w in wins], [w[1] for w in wins])
                eng.cross_kv(enc, 0)
                del enc
                pending = list(range(len(wins)))
                results: dict = {}
                tries: dict = {i: [] for i in pending}
                # multilingual: the first temperature's call keeps the one shared prompt and every window chooses its
                # language in it (one position for all); later temperatures pass per-window prompts, of one length
                # still, that carry the returned tokens
                auto = bool(options.multilingual) and tokenizer.language is not None
                lang_pos = prompt.index(st.sot) + 1
                win_lang: dict = {}
                for ti, T in enumerate(options.temperatures):
                    if not pending:
                        break
                    prompts = [prompt] * len(pending)
                    kw = {}
                    if auto and ti == 0:
                        kw["language_auto"] = m._language_auto(options, [lang_pos] * len(pending))
                    elif auto:
                        prompts = [prompt[:lang_pos] + [tokenizer.for_language(win_lang[i]).language] +
                                   prompt[lang_pos + 1:] for i in pending]
                    res, *lang = eng.generate(
                        pending, prompts, max_length=max_length, num_hypotheses=options.best_of if T > 0 else 1,
                        seed=seed + 7919 * ti + b0, suppress_tokens=options.suppress_tokens,
                        sot_index=prompt.index(st.sot), compact=self.compact, **_decode_kwargs(options, T), **kw)
                    if auto and ti == 0:
                        win_lang = {i: st.lang_codes[int(t)] for i, t in zip(pending, lang[1][0])}
                    still = []
                    for i, r in zip(pending, res):
                        alp = segs.avg_logprob(r.score, len(r.tokens), options.length_penalty)
                        cr = segs.compression_ratio(tokenizer.decode(r.tokens).strip())
                        fb, below = segs.needs_fallback(cr, alp, r.no_speech_prob, options.compression_ratio_threshold,
                                                        options.log_prob_threshold, options.no_speech_threshold)
                        tries[i].append((r, alp, T, cr, below))
                        if fb:
                            still.append(i)
                        else:
                            results[i] = (r, alp, T, cr)
                    pending = still
                for i in pending:                      # every temperature failed: best avg logprob
                    cand = [t for t in tries[i] if t[4]] or tries[i]
                    r, alp, _, cr, _ = max(cand, key=lambda t: t[1])
                    results[i] = (r, alp, options.temperatures[-1], cr)
                batch = []
                for i, (s, n) in enumerate(wins):
                    r, alp, T, cr = results[i]
                    sb = seek_bases[b0 + i] if seek_bases is not None else 0
                    wr = WindowResult(b0 + i, s - sb, n, time_offsets[b0 + i], r.tokens, alp, T, cr, r.no_speech_prob,
                                      language=win_lang.get(i))
                    wr.segments = self.window_segments(wr, tokenizer, options)
                    batch.append(wr)
                if options.word_timestamps:
                    # the batch's encoder outputs are still in slots 0..B-1: one batched alignment for every
                    # window with text (faster-whisper aligns a whole batch of segments in one model.align); with
                    # several files, one call per file so each keeps its own last-speech time; multilingual: inside a
                    # file one call per run of windows of one language (wm_align_batch takes one sot sequence), in
                    # window order, so the last-speech time still runs through the file's windows in order
                    fid = [files[b0 + i] if files is not None else 0 for i in range(len(batch))]
                    for f in sorted(set(fid)):
                        idx = [i for i, wr in enumerate(batch) if wr.segments and fid[i] == f]
                        for lang_code, run in itertools.groupby(idx, key=lambda i: batch[i].language):
                            run = list(run)
                            last_speech[f] = m.add_word_timestamps(
                                [batch[i].segments for i in run],
                                tokenizer.for_language(lang_code) if lang_code else tokenizer,
                                [batch[i].size for i in run], options.prepend_punctuations,
                                options.append_punctuations, last_speech.get(f, 0.0), slots=run)
                out.extend(batch)
        return out

    def window_segments(self, wr: WindowResult, tokenizer: Tokenizer, options: TranscriptionOptions) -> List[dict]:
        if segs.should_skip_window(wr.no_speech_prob, wr.avg_logprob, options.no_speech_threshold,
                                   options.log_prob_threshold):
            return []
        dur = wr.size * HOP_LENGTH / SAMPLE_RATE
        if options.without_timestamps:
            cur = [dict(seek=wr.seek, start=wr.time_offset, end=wr.time_offset + dur,
                        tokens=[t for t in wr.tokens if t < tokenizer.eot])]
        else:
            cur, _, _ = segs.split_segments_by_timestamps(wr.tokens, tokenizer.timestamp_begin, wr.time_offset,
                                                          wr.size, dur, wr.seek)
        return cur

    def transcribe(self, audio: Union[str, BinaryIO, np.ndarray], language: Optional[str] = None,
                   task: str = "transcribe", log_progress: bool = False, beam_size: int = 5, best_of: int = 5,
                   patience: float = 1, length_penalty: float = 1, repetition_penalty: float = 1,
                   no_repeat_ngram_size: int = 0,
                   temperature: Union[float, List[float], Tuple[float, ...]] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                   compression_ratio_threshold: Optional[float] = 2.4, log_prob_threshold: Optional[float] = -1.0,
                   no_speech_threshold: Optional[float] = 0.6, initial_prompt=None, prefix: Optional[str] = None,
                   suppress_blank: bool = True, suppress_tokens: Optional[List[int]] = [-1],
                   without_timestamps: bool = True, max_initial_timestamp: float = 1.0, word_timestamps: bool = False,
                   prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
                   multilingual: Optional[bool] = None, vad_filter: bool = True, vad_parameters=None,
                   max_new_tokens: Optional[int] = None, chunk_length: Optional[int] = None, clip_timestamps=None,
                   hallucination_silence_threshold: Optional[float] = None, batch_size: int = 16,
                   hotwords: Optional[str] = None, language_detection_threshold: Optional[float] = 0.5,
                   language_detection_segments: int = 1,
                   sequence_bias: Optional[Mapping[Union[str, Tuple[int, ...]], float]] = None,
                   max_line_width: Optional[int] = None, max_line_count: Optional[int] = None,
                   max_cue_seconds: Optional[float] = None, language_candidates: Optional[Sequence[str]] = None):
        """sequence_bias: as WhisperModel.transcribe (one table for every window of the file).
        language_candidates: as WhisperModel.transcribe (the whitelist of the file's language detection).
        max_line_width, max_line_count, max_cue_seconds: caption shaping as in WhisperModel.transcribe; the windows
        then decode as with word_timestamps=True and the segments leave through captions.shape_captions."""
        args = dict(locals())
        return self._transcribe(audio, _resolve_call(self.model, "batched", args))

    def _transcribe(self, audio, call: _Call):
        """`transcribe` for a resolved call: the public method's, or WhisperModel.transcribe's in throughput mode."""
        file = self._prepare(audio, call)
        tokenizer = self.model.tokenizer(task=call.args["task"], language=file.language)
        options = call.options(self.model, tokenizer, 0, file.language_candidates)
        offsets = [s * HOP_LENGTH / SAMPLE_RATE for s, _ in file.windows]
        results = self.decode_windows(file.features, file.windows, offsets, tokenizer, options, last_speech={})
        return self._segments(results, tokenizer, options), file.info(options)

    def transcribe_many(self, audios: Sequence[Union[str, BinaryIO, np.ndarray]],
                        language: Union[None, str, Sequence[Optional[str]]] = None, task: str = "transcribe",
                        vad_filter: bool = True, vad_parameters=None, language_detection_segments: int = 1,
                        language_detection_threshold: Optional[float] = 0.5, **kw):
        """Several files in shared decode batches: the worker transcribes one video at a time
        (reference worker/transcription.py:496-506), so a short file leaves most of a 150-window batch empty.
        Here the windows of all files (same task; grouped by language, since the prompt carries it) are packed
        into the same batches: the files' log-mel matrices are concatenated along time (each normalised with
        its own global max, as faster-whisper does per file) and every window keeps its file's time offsets.
        Returns [(segments, info)] per file, in input order; each file's result is what `transcribe` gives for
        it alone (same windows, prompts and options).  sequence_bias (in **kw, see WhisperModel.transcribe) is one
        mapping for all files; a per-file list raises ValueError.  max_line_width, max_line_count, max_cue_seconds
        (in **kw too): caption shaping as in WhisperModel.transcribe, applied to every file's segments on their own.
        language_candidates (in **kw): one sequence of codes for all files, as WhisperModel.transcribe_many."""
        args = dict(locals())
        unknown = [k for k in kw if k not in _BATCHED_DEFAULTS]
        if unknown:
            raise TypeError(f"transcribe_many() got an unexpected keyword argument {unknown[0]!r}")
        args.update(_BATCHED_DEFAULTS, **kw)     # **kw: the options of `transcribe`, with their defaults there
        return self._transcribe_many(audios, _resolve_call(self.model, "batched_many", args, len(audios)))

    def _transcribe_many(self, audios, call: _Call):
        """`transcribe_many` for a resolved call: the public method's, or WhisperModel.transcribe_many's in throughput
        mode."""
        preps = [self._prepare(a, call, f) for f, a in enumerate(audios)]
        out: List[Optional[tuple]] = [None] * len(audios)
        last_speech: dict = {}
        for lang in sorted({p.language for p in preps}):
            files = [i for i, p in enumerate(preps) if p.language == lang]
            tokenizer = self.model.tokenizer(task=call.args["task"], language=lang)
            # (the options are one object per language group: they echo the call's whitelist when any file of the
            # group had its language detected under it)
            options = call.options(self.model, tokenizer, files[0], next(
                (preps[i].language_candidates for i in files if preps[i].language_candidates), None))
            feats = torch.cat([preps[i].features for i in files], dim=1) if len(files) > 1 else preps[files[0]].features
            windows, offsets, fids, bases = [], [], [], {}
            base = 0
            for i in files:
                bases[i] = base
                for s, nf in preps[i].windows:
                    windows.append((base + s, nf))
                    offsets.append(s * HOP_LENGTH / SAMPLE_RATE)
                    fids.append(i)
                base += preps[i].features.shape[1]
            results = self.decode_windows(feats, windows, offsets, tokenizer, options, files=fids,
                                          seek_bases=[bases[f] for f in fids], last_speech=last_speech)
            for i in files:
                mine = [wr for wr, f in zip(results, fids) if f == i]
                out[i] = (list(self._segments(mine, tokenizer, options)), preps[i].info(options))
        return out

    def _prepare(self, audio, call: _Call, f: int = 0) -> _File:
        """The throughput path's file: PCM, then log-mel of the WHOLE file, then its windows (VAD-bounded or fixed) and
        its language.  `audio` may be an IngestResult (vlog_amd/ingest.py: PCM and log-mel already on the device,
        computed while streaming)."""
        from .ingest import IngestResult
        m, a = self.model, call.args
        if isinstance(audio, IngestResult):
            features, duration = audio.features, audio.duration
            audio = audio.pcm
        else:
            if not isinstance(audio, np.ndarray):
                audio = m._load_audio(audio)
            audio = np.asarray(audio, dtype=np.float32)
            duration = audio.shape[0] / SAMPLE_RATE
            with m._lock:
                features = m._features(audio)
        content = features.shape[1] - 1
        vad_opts = None
        if a["vad_filter"]:
            from .vad import get_speech_timestamps
            vad_opts = _vad_options(a["vad_parameters"])
            chunks = get_speech_timestamps(audio, vad_opts, m)
            windows = self.vad_windows(chunks, content)
            duration_after_vad = sum(c["end"] - c["start"] for c in chunks) / SAMPLE_RATE
        else:
            windows = self.fixed_windows(content)
            duration_after_vad = duration
        # only this path skips the detection for a file with no windows; it keeps a named language as it is, in an
        # English-only model too
        return _File(features, duration, duration_after_vad, vad_opts,
                     *m._file_language(a["language"][f], features, a["language_detection_segments"],
                                       a["language_detection_threshold"], a["language_candidates"],
                                       detect=bool(windows)), windows=windows)

    def _segments(self, results: List[WindowResult], tokenizer: Tokenizer, options: TranscriptionOptions):
        """The windows' segments in order, ids 1, 2, ...; through captions.shape_captions when the options have it on."""
        return _shaped(self._window_stream(results, tokenizer, options), options)

    def _window_stream(self, results: List[WindowResult], tokenizer: Tokenizer, options: TranscriptionOptions):
        idx = 0
        for wr in results:
            cur = wr.segments if wr.segments is not None else self.window_segments(wr, tokenizer, options)
            for s in cur:
                text = tokenizer.decode(s["tokens"])
                if s["start"] == s["end"] or not text.strip():
                    continue
                idx += 1
                yield Segment(id=idx, seek=wr.seek, start=s["start"], end=s["end"], text=text, tokens=s["tokens"],
                              avg_logprob=wr.avg_logprob, compression_ratio=wr.compression_ratio,
                              no_speech_prob=wr.no_speech_prob, temperature=wr.temperature,
                              words=[_word(w) for w in s["words"]] if options.word_timestamps else None,
                              language=wr.language)


def _defaults(fn) -> dict:
    return {p.name: p.default for p in inspect.signature(fn).parameters.values() if p.default is not p.empty}


# The one table of defaults is the public signatures themselves, read once: WhisperModel.transcribe's for
# default_batched_options, and for the **kw of BatchedInferencePipeline.transcribe_many the arguments of its
# `transcribe` that it neither names itself nor has ever taken (the four that `transcribe` accepts and ignores or
# refuses; in **kw they are a TypeError, as every unknown name).
_SEQUENTIAL_DEFAULTS = _defaults(WhisperModel.transcribe)
_BATCHED_DEFAULTS = {k: v for k, v in _defaults(BatchedInferencePipeline.transcribe).items()
                     if k not in _defaults(BatchedInferencePipeline.transcribe_many)
                     and k not in ("log_progress", "chunk_length", "hallucination_silence_threshold", "batch_size")}


def default_batched_options(**kw) -> dict:
    """TranscriptionOptions fields (as a dict) for the batched/sharded throughput mode."""
    base = {fd.name: _SEQUENTIAL_DEFAULTS[fd.name] for fd in fields(TranscriptionOptions)
            if fd.default is MISSING and fd.name != "temperatures"}            # the fields without a default
    base.update({fd.name: float(base[fd.name]) for fd in fields(TranscriptionOptions)
                 if fd.type == "float" and fd.name in base})                   # (the signatures write 1 for 1.0)
    base.update(condition_on_previous_text=False, temperatures=list(_SEQUENTIAL_DEFAULTS["temperature"]),
                suppress_tokens=[-1], multilingual=False)
    if "temperature" in kw:
        t = kw.pop("temperature")
        kw["temperatures"] = list(t) if isinstance(t, (list, tuple)) else [t]
    unknown = set(kw) - set(base)
    if unknown:
        raise TypeError(f"unknown options {sorted(unknown)}")
    base.update(kw)
    return base
