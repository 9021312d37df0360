"""CPU: what the public entry points of vlog_amd/transcribe.py hand on, call by call, against a recording fake engine.

WhisperModel.transcribe / transcribe_many / align and BatchedInferencePipeline.transcribe / transcribe_many run on a
model built with WhisperModel.__new__ whose engine records every call it receives (features, encode, cross_kv, reserve,
option, set_option, frame_energy_db, align_batch, align_open_batch and generate with its full keyword arguments) and
answers generate with scripted results: every window yields one segment with text, the window at mel frame 3000 fails
the log-probability threshold at temperature 0 (so the fallback calls are part of the trace), and a language_auto call
returns the language tuple.  detect_language and vad.get_speech_timestamps are replaced by recorders with canned
answers.  Nothing is decoded and nothing numeric is computed, so a case's trace (the ordered calls, the logged
warnings, info.transcription_options as a dict, the info fields and the emitted segments, or the exception's type and
message) is compared with tests/golden/transcribe_calls.json for equality.  The same file pins inspect.signature of the
public methods and of default_batched_options.  To keep the file small it holds every trace in a compact form
(`compact`: each repeated dict as its difference from a base that the file keeps too), which loses nothing.

The golden was recorded once, before the entry points were refactored to resolve a call's options in one place
(`python tests/test_transcribe_calls_host.py --record`, which refuses to overwrite an existing file); the commit it was
recorded at is in the file's "recorded_at".  It is the behaviour to keep, not a snapshot to refresh.
"""
import dataclasses
import hashlib
import inspect
import json
import logging
import os
import sys
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vlog_amd import language_id  # noqa: E402
from vlog_amd import transcribe as tr  # noqa: E402
from vlog_amd.dims import model_dims  # noqa: E402
from vlog_amd.tokenizer import Tokenizer  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "transcribe_calls.json")
RATE = 16000
FAIL_SEEK = 3000          # the window at this mel frame fails temperature 0


def _plain(x):
    """JSON-able, and equal to itself after a JSON round trip: tuples -> lists, arrays and tensors -> lists or shapes,
    mapping keys -> str, dataclasses -> dicts."""
    if dataclasses.is_dataclass(x) and not isinstance(x, type):
        return _plain(dataclasses.asdict(x))
    if isinstance(x, torch.Tensor):
        return {"tensor": list(x.shape)}
    if isinstance(x, np.ndarray):
        return _plain(x.tolist())
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, float) and x == float("inf"):
        return "inf"
    return x


class FakeEngine:
    def __init__(self, dims, trace):
        self.dims, self.trace = dims, trace
        self.slot_seek = {}
        self.tb = Tokenizer(dims, language="en", seed=3).timestamp_begin

    def log(self, name, **kw):
        self.trace.append([name, _plain(kw)])

    def features(self, pcm):
        self.log("features", samples=int(pcm.shape[0]))
        return torch.zeros((self.dims.n_mels, int(pcm.shape[0]) // 160 + 1), dtype=torch.float32)

    def encode(self, mel, seeks, nframes):
        self.log("encode", mel=mel, seeks=list(seeks), nframes=list(nframes))
        return SimpleNamespace(seeks=list(seeks))

    def cross_kv(self, enc, slot0=0):
        self.log("cross_kv", slot0=slot0)
        for i, s in enumerate(enc.seeks):
            self.slot_seek[slot0 + i] = s

    def reserve(self, n_slots, n_hyp):
        self.log("reserve", n_slots=n_slots, n_hyp=n_hyp)

    def option(self, key, default=None):
        self.log("option", key=key, default=default)
        return default

    def set_option(self, key, value):
        self.log("set_option", key=key, value=value)

    def frame_energy_db(self, pcm, frame=512):
        self.log("frame_energy_db", samples=int(pcm.shape[0]), frame=frame)
        db = np.full(int(pcm.shape[0]) // frame, -30.0, dtype=np.float32)
        db[1600:1602] = -80.0                       # the quietest 20 ms: mel frame 3200
        return db

    @staticmethod
    def _path(n_tokens, frames):
        n, F = n_tokens + 1, max(1, frames // 2)
        step = max(1, F // n)
        ti = np.array([min(c // step, n - 1) for c in range(F)])
        return np.full(n_tokens, 0.5, dtype=np.float32), ti, np.arange(F), int(ti[-1]) + 1

    def align_batch(self, slots, sot, texts, frames, heads, medw):
        self.log("align_batch", slots=list(slots), sot=list(sot), texts=[list(t) for t in texts], frames=list(frames),
                 medw=medw)
        return [self._path(len(t), f)[:3] for t, f in zip(texts, frames)]

    def align_open_batch(self, slots, sot, texts, frames, heads, medw):
        self.log("align_open_batch", slots=list(slots), sot=list(sot), texts=[list(t) for t in texts],
                 frames=list(frames), medw=medw)
        return [self._path(len(t), f) for t, f in zip(texts, frames)]

    def generate(self, slots, prompts, **kw):
        self.log("generate", slots=list(slots), prompts=[list(p) for p in prompts], **kw)
        T = kw.get("temperature", 0.0)
        res = []
        for k, (slot, prompt) in enumerate(zip(slots, prompts)):
            seek = self.slot_seek.get(slot)
            seed = kw["seeds"][k] if kw.get("seeds") is not None else kw.get("seed", 0)
            h = hashlib.sha256(repr((seek, tuple(prompt), round(T, 3), int(seed))).encode()).digest()
            rng = np.random.default_rng(int.from_bytes(h[:8], "little"))
            toks = [int(v) for v in rng.integers(300, 20000, size=5)]
            if kw.get("with_timestamps", True):
                toks = [self.tb] + toks + [self.tb + 100]
            failing = seek == FAIL_SEEK and T < 0.1
            res.append(SimpleNamespace(tokens=toks, score=-1.5 if failing else -0.3, no_speech_prob=0.05))
        auto = kw.get("language_auto")
        if auto is None:
            return res, 7
        allowed = auto.get("allowed")
        codes = list(self.dims.specials.lang_codes)
        cands = [j for j in range(auto["n_langs"]) if allowed[j]] if allowed is not None else \
            [codes.index("en"), codes.index("es")]
        top = np.array([cands[(self.slot_seek.get(s, 0) // 3000) % len(cands)] if p >= 0 else -1
                        for s, p in zip(slots, auto["positions"])], dtype=np.int32)
        return res, 7, (top, np.full(len(slots), 0.75, dtype=np.float32),
                        np.zeros((len(slots), auto["n_langs"]), dtype=np.float32))


def _model(name, throughput, trace, env_bias=None):
    m = tr.WhisperModel.__new__(tr.WhisperModel)
    m.dims = model_dims(name)
    m.engine = FakeEngine(m.dims, trace)
    m.throughput, m._batched = throughput, None
    m.model_dir = m._tokenizer_json = None
    m._tok_seed = 3
    m.vad_net = None
    m._lock = threading.RLock()
    m._env_sequence_bias = env_bias
    m.feature_size = m.dims.n_mels
    m.frames_per_second, m.tokens_per_second, m.input_stride = 100, 50, 2
    m.time_precision, m.max_length = 0.02, 448

    def detect_language(audio=None, features=None, **kw):
        trace.append(["detect_language", _plain(dict(audio=audio is not None, features=features, **kw))])
        return "es", 0.9, [("es", 0.9), ("en", 0.1)]

    m.detect_language = detect_language
    return m


def _chunks(n, kind):
    if kind == "none":
        return []
    # two speech chunks with 2 s of silence removed between them and 0.5 s at either end
    return [dict(start=8000, end=n // 2 - 16000), dict(start=n // 2 + 16000, end=n - 8000)]


class _Records(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.lines = []

    def emit(self, record):
        self.lines.append([record.levelname, record.getMessage()])


BIAS = {"hello": 2.0, (400, 401): -100.0}
DECODE_OPTIONS = dict(beam_size=3, best_of=2, patience=1.5, length_penalty=0.8, repetition_penalty=1.2,
                      no_repeat_ngram_size=3, temperature=(0.0, 0.3), compression_ratio_threshold=2.0,
                      log_prob_threshold=-0.8, no_speech_threshold=0.5, suppress_blank=False, suppress_tokens=[-1, 500],
                      max_initial_timestamp=0.5, prepend_punctuations="(", append_punctuations=".,")
LONG, SHORT, PAIR = 65.0, 35.0, [35.0, 40.0]


def C(name, entry, secs=SHORT, model="tiny", throughput=False, env=None, vad="two", env_bias=None, text=None, **kw):
    return dict(name=name, entry=entry, secs=secs, model=model, throughput=throughput, env=env or {}, vad=vad,
                env_bias=env_bias, text=text, kw=kw)


T, TM, PT, PM, AL = "transcribe", "transcribe_many", "pipeline.transcribe", "pipeline.transcribe_many", "align"
TEXT = "hello vlog this is a line\nand a second line of the transcript"

CASES = [
    # ---- the four entry points with their defaults (the two classes' defaults differ and are left untouched)
    C("transcribe_defaults", T),
    C("transcribe_many_defaults", TM, PAIR),
    C("pipeline_transcribe_defaults", PT),
    C("pipeline_transcribe_many_defaults", PM, PAIR),
    # ---- language, temperature, beam, VAD
    C("transcribe_named_language", T, language="de"),
    C("pipeline_named_language", PT, language="de"),
    C("transcribe_temperature_float_beam1", T, temperature=0.0, beam_size=1),
    C("transcribe_temperature_tuple_beam5", T, temperature=(0.0, 0.4), beam_size=5),
    C("transcribe_sampled_first", T, temperature=0.2, best_of=3),
    C("pipeline_temperature_list", PT, temperature=[0.0, 0.4, 0.8], best_of=2),
    C("transcribe_vad", T, vad_filter=True),
    C("transcribe_vad_parameters", T, vad_filter=True, vad_parameters=dict(threshold=0.4, speech_pad_ms=100)),
    C("transcribe_vad_options_object", T, vad_filter=True,
      vad_parameters=tr.VadOptions(min_silence_duration_ms=500)),
    C("transcribe_vad_no_speech", T, vad_filter=True, vad="none"),
    C("transcribe_vad_skipped_by_clip", T, vad_filter=True, clip_timestamps="5,20"),
    C("pipeline_vad_off", PT, vad_filter=False),
    C("pipeline_vad_no_speech", PT, vad="none"),
    C("transcribe_detection_arguments", T, language_detection_threshold=None, language_detection_segments=3),
    # ---- every decode option at a non-default value, on every decode form; the prompt parts
    C("transcribe_decode_options", T, **DECODE_OPTIONS),
    C("transcribe_sections_decode_options", T, LONG, sections=2, **DECODE_OPTIONS),
    C("pipeline_decode_options", PT, **DECODE_OPTIONS),
    C("throughput_decode_options", T, throughput=True, **DECODE_OPTIONS),
    C("transcribe_prompt_parts", T, initial_prompt="hello there", prefix="So", hotwords="vlog",
      condition_on_previous_text=False, prompt_reset_on_temperature=0.1),
    C("transcribe_prompt_tokens", T, initial_prompt=[400, 401, 402], suppress_tokens=None),
    C("pipeline_prompt_parts", PT, initial_prompt="hello there", hotwords="vlog", clip_timestamps="0"),
    C("transcribe_word_timestamps", T, word_timestamps=True),
    C("transcribe_without_timestamps", T, without_timestamps=True),
    C("pipeline_word_timestamps", PT, word_timestamps=True),
    C("pipeline_with_timestamps", PT, without_timestamps=False),
    C("transcribe_max_new_tokens", T, max_new_tokens=10),
    C("pipeline_max_new_tokens", PT, max_new_tokens=10),
    C("transcribe_clip_timestamps", T, clip_timestamps=[2.0, 12.0]),
    C("pipeline_ignores_chunk_length_and_batch_size", PT, chunk_length=20, batch_size=4, log_progress=True),
    # ---- sections
    C("sections2_fallback_off", T, LONG, sections=2, lockstep_fallback=False),
    C("sections2_fallback_on", T, LONG, sections=2, lockstep_fallback=True),
    C("sections2_vad", T, LONG, sections=2, vad_filter=True),
    C("sections2_in_flight1", T, LONG, sections=2, sections_in_flight=1),
    C("sections2_sampled_first_off", T, LONG, sections=2, temperature=(0.2, 0.4), best_of=3,
      lockstep_fallback=False),
    C("sections2_sampled_first_on", T, LONG, sections=2, temperature=(0.2, 0.4), best_of=3, lockstep_fallback=True),
    C("sections2_word_timestamps", T, LONG, sections=2, word_timestamps=True, lockstep_fallback=True),
    C("sections2_short_file_one_section", T, sections=2),
    # ---- transcribe_many
    C("many_per_file_lists", TM, PAIR, language=["de", None], initial_prompt=["hello there", None], hotwords=[None,
      "vlog"], prefix=["So", None]),
    C("many_per_file_tuples_fallback_on", TM, PAIR, language=("de", "en"), hotwords=("a", "b"),
      lockstep_fallback=True),
    C("many_sampled_first", TM, PAIR, temperature=0.2, best_of=2),
    C("many_no_files", TM, []),
    C("pipeline_many_per_file_languages", PM, PAIR, language=["de", None], vad_filter=False),
    C("pipeline_many_options", PM, PAIR, language="de", beam_size=2, temperature=0.0, hotwords="vlog",
      initial_prompt="hello there", clip_timestamps=None, without_timestamps=False),
    # ---- throughput mode reached through WhisperModel
    C("throughput_worker_call", T, throughput=True, language=None, task="transcribe", beam_size=5, vad_filter=True),
    C("throughput_named_language_words", T, throughput=True, language="de", word_timestamps=True, hotwords="vlog"),
    C("throughput_many", TM, PAIR, throughput=True, vad_filter=True, hotwords="vlog"),
    C("throughput_many_per_file_languages", TM, PAIR, throughput=True, language=["de", None]),
    C("throughput_ignored_options", T, throughput=True, condition_on_previous_text=False,
      prompt_reset_on_temperature=0.1, lockstep_fallback=True, sections_in_flight=2, sections=1),
    # ---- multilingual
    C("multilingual_transcribe", T, multilingual=True),
    C("multilingual_sections2_fallback_on_words", T, LONG, sections=2, multilingual=True, lockstep_fallback=True,
      word_timestamps=True),
    C("multilingual_many", TM, PAIR, multilingual=True),
    C("multilingual_pipeline", PT, multilingual=True),
    C("multilingual_throughput", T, throughput=True, multilingual=True),
    C("multilingual_candidates", T, multilingual=True, language_candidates=["en", "de"]),
    # ---- language_candidates
    C("candidates_transcribe", T, language_candidates=["en", "es"]),
    C("candidates_named_language", T, language_candidates=["en", "es"], language="de"),
    C("candidates_empty_beats_environment", T, language_candidates=[], env={"VLOG_AMD_LANGUAGE_CANDIDATES":
      "en,es"}),
    C("candidates_many", TM, PAIR, language_candidates=("en", "es"), language=["de", None]),
    C("candidates_pipeline_many", PM, PAIR, language_candidates=["en", "es"], language=[None, "de"]),
    C("candidates_throughput", T, throughput=True, language_candidates=["en", "es"]),
    # ---- sequence_bias
    C("bias_transcribe", T, sequence_bias=BIAS),
    C("bias_sections2", T, LONG, sections=2, sequence_bias=BIAS),
    C("bias_pipeline", PT, sequence_bias=BIAS),
    C("bias_throughput", T, throughput=True, sequence_bias=BIAS),
    C("bias_environment_transcribe", T, env_bias={"vlog": 1.5}),
    C("bias_argument_beats_environment", T, env_bias={"vlog": 1.5}, sequence_bias=BIAS),
    # ---- caption shaping
    C("captions_transcribe_all", T, max_line_width=16, max_line_count=1, max_cue_seconds=3, vad_filter=True),
    C("captions_many", TM, PAIR, max_line_width=20, vad_filter=True),
    C("captions_pipeline", PT, max_line_width=20, max_line_count=3),
    C("captions_throughput", T, throughput=True, max_line_width=20, max_cue_seconds=2.5),
    C("captions_zero_beats_environment", T, max_line_width=0, env={"VLOG_AMD_MAX_LINE_WIDTH": "20"}),
    # ---- the environment forms
    C("env_multilingual", T, env={"VLOG_AMD_MULTILINGUAL": "1"}),
    C("env_multilingual_named_language", T, language="de", env={"VLOG_AMD_MULTILINGUAL": "1"}),
    C("env_multilingual_throughput_named", T, throughput=True, language="de", env={"VLOG_AMD_MULTILINGUAL": "1"}),
    C("env_multilingual_bad", T, env={"VLOG_AMD_MULTILINGUAL": "on"}),
    C("env_lockstep_fallback", T, LONG, sections=2, env={"VLOG_AMD_LOCKSTEP_FALLBACK": "1"}),
    C("env_lockstep_fallback_bad", T, env={"VLOG_AMD_LOCKSTEP_FALLBACK": "yes"}),
    C("env_sections", T, LONG, env={"VLOG_AMD_SECTIONS": "2"}),
    C("env_sections_throughput", T, throughput=True, env={"VLOG_AMD_SECTIONS": "2"}),
    C("env_captions", T, env={"VLOG_AMD_MAX_LINE_WIDTH": "20", "VLOG_AMD_MAX_LINE_COUNT": "3",
      "VLOG_AMD_MAX_CUE_SECONDS": "4"}),
    C("env_captions_bad", T, env={"VLOG_AMD_MAX_LINE_WIDTH": "wide"}),
    C("env_candidates", T, env={"VLOG_AMD_LANGUAGE_CANDIDATES": "en,es"}),
    C("env_candidates_bad", T, env={"VLOG_AMD_LANGUAGE_CANDIDATES": "en,xx"}),
    C("env_cross_auto_off", T, env={"VLOG_AMD_CROSS_AUTO": "0"}),
    C("env_batch_windows_and_compact", T, LONG, throughput=True, env={"VLOG_AMD_BATCH_WINDOWS": "2",
      "VLOG_AMD_COMPACT": "0"}),
    # ---- an English-only model
    C("en_model_named_other_language", T, model="tiny.en", language="de"),
    C("en_model_multilingual", T, model="tiny.en", multilingual=True),
    C("en_model_candidates", T, model="tiny.en", language_candidates=["en", "es"]),
    C("en_model_pipeline_named_other_language", PT, model="tiny.en", language="de"),
    C("en_model_many", TM, PAIR, model="tiny.en", language=["de", None], multilingual=True),
    C("en_model_align", AL, model="tiny.en", text=TEXT, language="de"),
    # ---- the refusals, one case each (and where entry points repeat a check, one per entry point)
    C("refuse_hallucination_transcribe", T, hallucination_silence_threshold=2.0),
    C("refuse_hallucination_many", TM, PAIR, hallucination_silence_threshold=2.0),
    C("refuse_hallucination_pipeline", PT, hallucination_silence_threshold=2.0),
    C("refuse_hallucination_throughput", T, throughput=True, hallucination_silence_threshold=2.0),
    C("refuse_chunk_length_transcribe", T, chunk_length=20),
    C("refuse_chunk_length_many", TM, PAIR, chunk_length=20),
    C("refuse_task_transcribe", T, task="summarise"),
    C("refuse_task_many", TM, PAIR, task="summarise"),
    C("refuse_task_align", AL, text=TEXT, task="summarise"),
    C("refuse_sections_zero", T, sections=0),
    C("refuse_sections_33", T, sections=33),
    C("refuse_sections_environment", T, env={"VLOG_AMD_SECTIONS": "40"}),
    C("refuse_sections_in_flight_zero", T, LONG, sections=2, sections_in_flight=0),
    C("refuse_sections_throughput", T, LONG, throughput=True, sections=2),
    C("refuse_sections_clip_timestamps", T, LONG, sections=2, clip_timestamps=[0.0, 10.0]),
    C("refuse_throughput_initial_prompt", T, throughput=True, initial_prompt="hello"),
    C("refuse_throughput_clip_timestamps", T, throughput=True, clip_timestamps="5"),
    C("refuse_throughput_prefix", T, throughput=True, prefix="So"),
    C("refuse_throughput_many_initial_prompt", TM, PAIR, throughput=True, initial_prompt=[None, "hello"]),
    C("refuse_throughput_many_clip_timestamps", TM, PAIR, throughput=True, clip_timestamps="5"),
    C("refuse_throughput_many_prefix", TM, PAIR, throughput=True, prefix="So"),
    C("refuse_throughput_many_per_file_hotwords", TM, PAIR, throughput=True, hotwords=["a", "b"]),
    C("accept_throughput_many_same_hotwords", TM, PAIR, throughput=True, hotwords=["a", "a"]),
    C("refuse_pipeline_prefix", PT, prefix="So"),
    C("refuse_pipeline_many_prefix", PM, PAIR, prefix="So"),
    C("refuse_bias_list_many", TM, PAIR, sequence_bias=[BIAS, BIAS]),
    C("refuse_bias_list_throughput_many", TM, PAIR, throughput=True, sequence_bias=[BIAS, BIAS]),
    C("refuse_bias_list_pipeline_many", PM, PAIR, sequence_bias=[BIAS, BIAS]),
    C("refuse_bias_list_transcribe", T, sequence_bias=[BIAS]),
    C("refuse_max_files_zero", TM, PAIR, max_files=0),
    C("refuse_multilingual_named", T, multilingual=True, language="de"),
    C("refuse_multilingual_named_many", TM, PAIR, multilingual=True, language=[None, "de"]),
    C("refuse_multilingual_named_pipeline", PT, multilingual=True, language="de"),
    C("refuse_multilingual_named_pipeline_many", PM, PAIR, multilingual=True, language="de"),
    C("refuse_caption_count_while_off", T, max_line_count=2),
    C("refuse_caption_count_while_off_pipeline", PT, max_line_count=2),
    C("refuse_caption_count_while_off_pipeline_many", PM, PAIR, max_cue_seconds=2.0),
    C("refuse_caption_width_negative", T, max_line_width=-1),
    C("refuse_caption_count_5", TM, PAIR, max_line_width=20, max_line_count=5),
    C("refuse_candidates_unknown", T, language_candidates=["en", "xx"]),
    C("refuse_candidates_unknown_named", T, language_candidates=["en", "xx"], language="de"),
    C("refuse_candidates_duplicate_pipeline", PT, language_candidates=["en", "en"]),
    C("refuse_candidates_per_file_many", TM, PAIR, language_candidates=[["en"], ["es"]]),
    C("refuse_many_list_length", TM, PAIR, language=["en"]),
    C("refuse_many_prompt_list_length", TM, PAIR, initial_prompt=["a", "b", "c"]),
    C("refuse_pipeline_many_language_length", PM, PAIR, language=["en"]),
    C("refuse_align_throughput", AL, throughput=True, text=TEXT),
    C("refuse_align_empty_text", AL, text=" \n "),
    # ---- two errors at once: the one detected first
    C("order_hallucination_before_task", T, hallucination_silence_threshold=2.0, task="summarise"),
    C("order_multilingual_before_chunk_length", T, multilingual=True, language="de", chunk_length=20),
    C("order_chunk_length_before_task", TM, PAIR, chunk_length=20, task="summarise"),
    C("order_task_before_sections", T, task="summarise", sections=0),
    C("order_sections_before_captions", T, sections=0, max_line_count=2),
    C("order_fallback_environment_before_captions", T, max_line_count=2, env={"VLOG_AMD_LOCKSTEP_FALLBACK": "yes"}),
    C("order_captions_before_candidates", T, max_line_count=2, language_candidates=["xx"]),
    C("order_candidates_before_throughput_refusal", T, throughput=True, language_candidates=["xx"], prefix="So"),
    C("order_max_files_before_bias", TM, PAIR, max_files=0, sequence_bias=[BIAS]),
    C("order_bias_before_captions_many", TM, PAIR, sequence_bias=[BIAS], max_line_count=2),
    C("order_candidates_before_list_length", TM, PAIR, language_candidates=["xx"], initial_prompt=["a"]),
    C("order_list_length_before_throughput_refusal", TM, PAIR, throughput=True, initial_prompt=["a"], prefix="So"),
    C("order_pipeline_hallucination_before_multilingual", PT, hallucination_silence_threshold=1.0,
      multilingual=True, language="de"),
    C("order_pipeline_multilingual_before_prefix", PT, multilingual=True, language="de", prefix="So"),
    C("order_pipeline_prefix_before_captions", PT, prefix="So", max_line_count=2),
    C("order_pipeline_many_prefix_before_captions", PM, PAIR, prefix="So", max_line_count=2),
    C("order_pipeline_many_captions_before_bias", PM, PAIR, max_line_count=2, sequence_bias=[BIAS]),
    C("order_pipeline_many_bias_before_candidates", PM, PAIR, sequence_bias=[BIAS], language_candidates=["xx"]),
    C("order_pipeline_many_candidates_before_multilingual", PM, PAIR, language_candidates=["xx"], multilingual=True,
      language="de"),
    C("order_pipeline_many_multilingual_before_length", PM, PAIR, multilingual=True, language=["de"]),
    # ---- align
    C("align_defaults", AL, text=TEXT),
    C("align_vad", AL, text=TEXT, vad_filter=True),
    C("align_named_language_lines", AL, text=TEXT.split("\n"), language="de", task="translate", max_cue_chars=12,
      max_window_tokens=8, median_filter_width=5, prepend_punctuations="(", append_punctuations=".,"),
    C("align_ignores_environment", AL, text=TEXT, env_bias={"vlog": 1.5}, env={"VLOG_AMD_MULTILINGUAL": "1",
      "VLOG_AMD_MAX_LINE_WIDTH": "20", "VLOG_AMD_LANGUAGE_CANDIDATES": "en,es", "VLOG_AMD_SECTIONS": "2",
      "VLOG_AMD_LOCKSTEP_FALLBACK": "1"}),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def _segment(s):
    return [s.id, s.start, s.end, s.text, s.temperature, s.language, None if s.words is None else len(s.words)]


def _result(segments, info):
    out = dict(segments=[_segment(s) for s in segments])
    for f in dataclasses.fields(info):
        out[f.name] = _plain(getattr(info, f.name))
    return out


def run_case(case):
    """One case -> its trace (module docstring), JSON-able."""
    trace = []
    records = _Records()
    logger = logging.getLogger("vlog_amd")
    with pytest.MonkeyPatch.context() as mp:
        for k in [k for k in os.environ if k.startswith("VLOG_AMD_")]:
            mp.delenv(k)
        for k, v in case["env"].items():
            mp.setenv(k, v)
        mp.setattr(language_id, "_english_only_logged", False)

        def get_speech_timestamps(audio, opts, model=None, **kw):
            trace.append(["get_speech_timestamps", _plain(dict(samples=len(audio), opts=opts, model=model is not None, **kw))])
            return _chunks(len(audio), case["vad"])

        mp.setattr("vlog_amd.vad.get_speech_timestamps", get_speech_timestamps)
        logger.addHandler(records)
        model = _model(case["model"], case["throughput"], trace, case["env_bias"])
        many = not isinstance(case["secs"], float)
        audios = [np.zeros(int(s * RATE), dtype=np.float32) for s in (case["secs"] if many else [case["secs"]])]
        entry, kw = case["entry"], case["kw"]
        try:
            if entry == AL:
                segments, info = model.align(audios[0], case["text"], **kw)
                out = _result(segments, info)
            else:
                target = tr.BatchedInferencePipeline(model, max_batch_windows=3) if entry.startswith("pipeline.") else model
                fn = getattr(target, entry.split(".")[-1])
                if many:
                    out = dict(files=[_result(list(s), i) for s, i in fn(audios, **kw)])
                else:
                    segments, info = fn(audios[0], **kw)
                    out = _result(list(segments), info)
        except Exception as ex:                     # the refusals: type and message are the trace
            out = dict(raises=[type(ex).__name__, str(ex)])
        finally:
            logger.removeHandler(records)
    out["calls"] = trace
    out["log"] = records.lines
    return json.loads(json.dumps(out))


ABSENT = "<absent>"


def _delta(d, base):
    """d as what differs from base (a key of base that d lacks reads ABSENT): one-to-one for a given base."""
    out = {k: v for k, v in d.items() if k not in base or base[k] != v}
    out.update({k: ABSENT for k in base if k not in d})
    return out


def compact(trace, base):
    """A trace with every dict that the cases repeat reduced to what differs from its counterpart in `base`: each
    call's keyword arguments against those of the case's previous call of that name (the first against
    base["calls"][name]), transcription_options and then the result's other fields
    against base["result"].  The golden keeps `base` beside its compact traces; for a given base the mapping is
    one-to-one, so equality of compact traces is equality of the traces."""
    def result(res):
        if "raises" in res or "files" in res:
            return dict(res)
        res = dict(res)
        for k in ("transcription_options", "vad_options"):
            if isinstance(res.get(k), dict):
                res[k] = _delta(res[k], base[k])
        keep = {k: res.pop(k) for k in ("segments", "files", "calls", "log") if k in res}
        return dict(_delta(res, base["result"]), **keep)

    out = result(trace)
    last = dict(base["calls"])          # a call is written against the case's previous call of its name
    out["calls"] = []
    for name, kw in trace["calls"]:
        out["calls"].append([name, _delta(kw, last.get(name, {}))])
        last[name] = kw
    if "files" in out:
        out["files"] = [result(f) for f in out["files"]]
    return out


def base_of(traces):
    """The base of `compact`: the result of `transcribe` with its defaults, and for every engine call the keyword
    arguments of its first occurrence over the cases in order."""
    first = traces["transcribe_defaults"]
    calls = {}
    for trace in traces.values():
        for name, kw in trace["calls"]:
            calls.setdefault(name, kw)
    result = {k: v for k, v in first.items() if k not in ("segments", "calls", "log", "transcription_options")}
    return dict(calls=calls, transcription_options=first["transcription_options"],
                vad_options=_plain(tr.VadOptions()), result=dict(result, transcription_options={}))


def write_golden(path, data):
    """One line per top-level entry and per case, so a case is one line of a diff."""
    def dumps(v):
        return json.dumps(v, ensure_ascii=False, separators=(",", ":"))

    with open(path, "w", encoding="utf-8") as f:
        f.write("{\n")
        for k in [k for k in data if k != "cases"]:
            f.write(f" {dumps(k)}: {dumps(data[k])},\n")
        f.write(' "cases": {\n' + ",\n".join(f"  {dumps(k)}: {dumps(v)}" for k, v in data["cases"].items()) + "\n }\n}\n")


def signatures(module=tr):
    """Names, kinds and defaults of every public callable of the two classes (their constructors too) and of
    default_batched_options."""
    fns = {"default_batched_options": module.default_batched_options}
    for cls in (module.WhisperModel, module.BatchedInferencePipeline):
        for name, f in vars(cls).items():
            f = getattr(f, "__func__", f)
            if inspect.isfunction(f) and (name == "__init__" or not name.startswith("_")):
                fns[f"{cls.__name__}.{name}"] = f
    return {name: [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                   for p in inspect.signature(fn).parameters.values()] for name, fn in sorted(fns.items())}


def _golden():
    with open(GOLDEN, "r", encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    return _golden()


def test_the_golden_holds_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASE_BY_NAME)


@pytest.mark.parametrize("name", list(CASE_BY_NAME))
def test_call_trace_is_the_recorded_one(name, golden):
    got, want = compact(run_case(CASE_BY_NAME[name]), golden["base"]), golden["cases"][name]
    for key in ("raises", "log", "calls"):
        assert got.get(key) == want.get(key), key
    assert got == want


def test_public_signatures_are_the_recorded_ones(golden):
    assert signatures() == golden["signatures"]


@pytest.mark.parametrize("name", ["chunk_length", "batch_size", "log_progress", "hallucination_silence_threshold", "beam"])
def test_pipeline_transcribe_many_takes_no_other_keyword(name):
    """its **kw is the options of `transcribe`: the four arguments that `transcribe` takes and ignores or refuses were
    never among them, and are a TypeError like any unknown name"""
    pipe = tr.BatchedInferencePipeline(_model("tiny", False, []))
    with pytest.raises(TypeError, match=f"unexpected keyword argument '{name}'"):
        pipe.transcribe_many([np.zeros(RATE, dtype=np.float32)], vad_filter=False, **{name: None})


def test_default_batched_options_are_the_recorded_ones(golden):
    got = tr.default_batched_options()
    assert {k: type(v).__name__ for k, v in got.items()} == \
        {k: type(v).__name__ for k, v in golden["default_batched_options"].items()}       # (1.0 stays a float)
    assert json.loads(json.dumps(tr.default_batched_options())) == golden["default_batched_options"]
    assert json.loads(json.dumps(tr.default_batched_options(beam_size=1, temperature=0.0))) == \
        golden["default_batched_options_greedy"]
    with pytest.raises(TypeError, match=r"unknown options \['beam', 'sections'\]"):
        tr.default_batched_options(beam=1, sections=2)


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) != 3:
        raise SystemExit("usage: python tests/test_transcribe_calls_host.py --record <commit the tree is at>")
    if os.path.exists(GOLDEN):
        raise SystemExit(f"{GOLDEN} exists: the golden is recorded once, on the code before the refactor")
    traces = {c["name"]: run_case(c) for c in CASES}
    base = base_of(traces)
    data = dict(recorded_at=sys.argv[2], signatures=signatures(),
                default_batched_options=tr.default_batched_options(),
                default_batched_options_greedy=tr.default_batched_options(beam_size=1, temperature=0.0), base=base,
                cases={k: compact(v, base) for k, v in traces.items()})
    write_golden(GOLDEN, data)
    raised = sum("raises" in v for v in data["cases"].values())
    print(f"recorded {len(data['cases'])} cases ({raised} raise) at {sys.argv[2]}: {os.path.getsize(GOLDEN)} bytes")
