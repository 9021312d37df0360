"""Host-side segment logic of the transcription path (faster-whisper `generate_segments` helpers [FW↑ 1.1.x]).

  split_segments_by_timestamps — `_split_segments_by_timestamps`: slice the token stream at consecutive
      timestamp pairs; start/end = window offset + (token - timestamp_begin) * 0.02 s; a single trailing
      timestamp means "no speech after it" (seek advances a whole window), otherwise seek moves to the last
      timestamp (2 mel frames per timestamp step).
  build_prompt — `get_prompt`: previous text, hotwords, sot sequence and prefix into one decoder prompt.
  build_sequence_bias, load_sequence_bias_file — the sequence-bias option: {phrase or token tuple: bias} into the
      engine's table of (token tuple, bias) entries, and the VLOG_AMD_SEQUENCE_BIAS file.
  compression_ratio — len(utf8) / len(zlib(utf8)) (fallback trigger above 2.4).
  needs_fallback — the generate_with_fallback decision (compression ratio, avg logprob, silence exemption).
  avg_logprob — recovered from the CTranslate2 score: score * len**length_penalty / (len + 1).
  _word_means, merge_punctuations — the word tail of `find_alignment` / `add_word_timestamps`, shared by the word
      timestamps (transcribe.py) and the forced alignment (forced_align.py).
"""
from __future__ import annotations

import zlib
import json
import math
from typing import Callable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

TIME_PRECISION = 0.02
INPUT_STRIDE = 2


def split_segments_by_timestamps(tokens: Sequence[int], timestamp_begin: int, time_offset: float,
                                 segment_size: int, segment_duration: float, seek: int
                                 ) -> Tuple[List[dict], int, bool]:
    tokens = list(tokens)
    tb = timestamp_begin
    segs: List[dict] = []
    single_ending = len(tokens) >= 2 and tokens[-2] < tb <= tokens[-1]
    cuts = [i for i in range(1, len(tokens)) if tokens[i] >= tb and tokens[i - 1] >= tb]
    if cuts:
        if single_ending:
            cuts.append(len(tokens))
        last = 0
        for cut in cuts:
            piece = tokens[last:cut]
            segs.append(dict(seek=seek,
                             start=time_offset + (piece[0] - tb) * TIME_PRECISION,
                             end=time_offset + (piece[-1] - tb) * TIME_PRECISION,
                             tokens=piece))
            last = cut
        if single_ending:
            seek += segment_size
        else:
            seek += (tokens[last - 1] - tb) * INPUT_STRIDE
    else:
        duration = segment_duration
        stamps = [t for t in tokens if t >= tb]
        if stamps and stamps[-1] != tb:
            duration = (stamps[-1] - tb) * TIME_PRECISION
        segs.append(dict(seek=seek, start=time_offset, end=time_offset + duration, tokens=tokens))
        seek += segment_size
    return segs, seek, single_ending


def build_prompt(encode: Callable[[str], List[int]], sot_sequence: Sequence[int], sot_prev: int, no_timestamps: int,
                 timestamp_begin: int, max_length: int, previous_tokens: Sequence[int] = (),
                 without_timestamps: bool = False, prefix: Optional[str] = None,
                 hotwords: Optional[str] = None) -> List[int]:
    """faster-whisper 1.1 `WhisperModel.get_prompt`, as a pure function of the tokenizer's ids and `encode`:

      [sot_prev, hotwords (only without a prefix), previous text]  — each cut to max_length // 2 - 1 tokens (the
          hotwords keep their head, the previous text its tail); the block is there when either part is
      sot_sequence, then no_timestamps when `without_timestamps`
      [timestamp_begin (with timestamps on), prefix]               — when a prefix is given
    """
    half = max_length // 2
    previous_tokens = list(previous_tokens)
    prompt: List[int] = []
    if previous_tokens or (hotwords and not prefix):
        prompt.append(sot_prev)
        if hotwords and not prefix:
            hw = list(encode(" " + hotwords.strip()))
            if len(hw) >= half:
                hw = hw[: half - 1]
            prompt.extend(hw)
        if previous_tokens:
            prompt.extend(previous_tokens[-(half - 1):])
    prompt.extend(sot_sequence)
    if without_timestamps:
        prompt.append(no_timestamps)
    if prefix:
        pf = list(encode(" " + prefix.strip()))
        if len(pf) >= half:
            pf = pf[: half - 1]
        if not without_timestamps:
            prompt.append(timestamp_begin)
        prompt.extend(pf)
    return prompt


SEQUENCE_BIAS_MAX_ENTRIES = 1024        # the engine's limits (wm_set_sequence_bias)
SEQUENCE_BIAS_MAX_TOKENS = 16


def build_sequence_bias(encode: Callable[[str], List[int]], mapping: Mapping[Union[str, Tuple[int, ...]], float],
                        n_vocab: int) -> List[Tuple[Tuple[int, ...], float]]:
    """The `sequence_bias` option -> the engine's table [(token tuple, bias)], in the mapping's order.

    A str key becomes two entries, the tokenisations of " " + text (the word inside a sentence) and of text (the word
    at the start of a window), one entry when both are the same ids.  A tuple of ints is taken as it is.  Every entry
    adds its bias to the logit of its LAST token when the generated tokens end in the ones before it (transformers'
    SequenceBiasLogitsProcessor): only the completing token is biased, so to favour a multi-token name from its
    first token, list its prefixes as keys of their own.  Raises ValueError naming the key on an empty tokenisation,
    one of more than 16 tokens, an id outside [0, n_vocab), a non-finite bias, or more than 1024 entries."""
    if not isinstance(mapping, Mapping):
        raise ValueError("sequence_bias must be a mapping {phrase or token tuple: bias}")
    table: List[Tuple[Tuple[int, ...], float]] = []
    for key, bias in mapping.items():
        try:
            b = float(bias)
        except (TypeError, ValueError):
            raise ValueError(f"sequence_bias[{key!r}]: the bias must be a number, got {bias!r}") from None
        if not math.isfinite(b) or abs(b) > float(np.finfo(np.float32).max):
            raise ValueError(f"sequence_bias[{key!r}]: the bias must be finite (f32), got {bias!r}")
        if isinstance(key, str):
            seqs = [tuple(int(t) for t in encode(" " + key)), tuple(int(t) for t in encode(key))]
            if seqs[0] == seqs[1]:
                seqs.pop()
        elif isinstance(key, tuple) and all(isinstance(t, (int, np.integer)) and not isinstance(t, bool) for t in key):
            seqs = [tuple(int(t) for t in key)]
        else:
            raise ValueError(f"sequence_bias key {key!r}: a str or a tuple of token ids expected")
        for seq in seqs:
            if not 1 <= len(seq) <= SEQUENCE_BIAS_MAX_TOKENS:
                raise ValueError(f"sequence_bias[{key!r}]: {len(seq)} tokens, 1 to {SEQUENCE_BIAS_MAX_TOKENS} expected")
            if any(t < 0 or t >= n_vocab for t in seq):
                raise ValueError(f"sequence_bias[{key!r}]: token id outside the vocabulary in {seq}")
            table.append((seq, b))
    if len(table) > SEQUENCE_BIAS_MAX_ENTRIES:
        raise ValueError(f"sequence_bias: {len(table)} entries, at most {SEQUENCE_BIAS_MAX_ENTRIES}")
    return table


def load_sequence_bias_file(path: str) -> dict:
    """The VLOG_AMD_SEQUENCE_BIAS file: one JSON object {"phrase": bias} -> {str: float}.  Raises ValueError naming the
    file when it is missing, no JSON object, or holds a value that is no finite number."""
    try:
        with open(path, "r", encoding="utf-8") as f:
            data = json.load(f)
    except (OSError, ValueError) as ex:
        raise ValueError(f"VLOG_AMD_SEQUENCE_BIAS={path!r}: {ex}") from None
    if not isinstance(data, dict):
        raise ValueError(f"VLOG_AMD_SEQUENCE_BIAS={path!r}: a JSON object {{\"phrase\": bias}} expected")
    out = {}
    for k, v in data.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"VLOG_AMD_SEQUENCE_BIAS={path!r}: the bias of {k!r} must be a finite number, got {v!r}")
        out[k] = float(v)
    return out


def compression_ratio(text: str) -> float:
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b)) if b else 0.0


def avg_logprob(score: float, n_tokens: int, length_penalty: float = 1.0) -> float:
    return score * (n_tokens ** length_penalty) / (n_tokens + 1)


def needs_fallback(comp_ratio: float, avg_lp: float, no_speech_prob: float,
                   compression_ratio_threshold: Optional[float] = 2.4, log_prob_threshold: Optional[float] = -1.0,
                   no_speech_threshold: Optional[float] = 0.6) -> Tuple[bool, bool]:
    """-> (needs_fallback, below_compression_threshold)."""
    fb = False
    below = True
    if compression_ratio_threshold is not None and comp_ratio > compression_ratio_threshold:
        fb = True
        below = False
    if log_prob_threshold is not None and avg_lp < log_prob_threshold:
        fb = True
    if (no_speech_threshold is not None and no_speech_prob > no_speech_threshold
            and log_prob_threshold is not None and avg_lp < log_prob_threshold):
        fb = False
    return fb, below


def should_skip_window(no_speech_prob: float, avg_lp: float, no_speech_threshold: Optional[float] = 0.6,
                       log_prob_threshold: Optional[float] = -1.0) -> bool:
    """faster-whisper's "no voice activity" skip after generate_with_fallback."""
    if no_speech_threshold is None:
        return False
    skip = no_speech_prob > no_speech_threshold
    if log_prob_threshold is not None and avg_lp > log_prob_threshold:
        skip = False
    return skip


def _word_means(probs: np.ndarray, wb: np.ndarray) -> List[float]:
    """[float(np.mean(probs[i:j])) ...] over consecutive word boundaries, with np.mean's own arithmetic spelled out for
    float32 (np.add.reduce of the slice, divided by the count in float64, rounded to float32): the same values
    without np.mean's per-call overhead (half the host time of config 5's word probabilities)."""
    p = np.asarray(probs)
    b = np.asarray(wb).tolist()
    if p.dtype != np.float32:
        return [float(np.mean(p[i:j])) for i, j in zip(b[:-1], b[1:])]
    add = np.add.reduce
    return [float(np.float32(float(add(p[i:j])) / (j - i))) if j > i else float(np.mean(p[i:j]))
            for i, j in zip(b[:-1], b[1:])]


def merge_punctuations(alignment: List[dict], prepended: str, appended: str) -> None:
    """faster-whisper / openai merge_punctuations."""
    i = len(alignment) - 2
    j = len(alignment) - 1
    while i >= 0:
        prev, foll = alignment[i], alignment[j]
        if prev["word"].startswith(" ") and prev["word"].strip() in prepended:
            foll["word"] = prev["word"] + foll["word"]
            foll["tokens"] = prev["tokens"] + foll["tokens"]
            prev["word"] = ""
            prev["tokens"] = []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(alignment):
        prev, foll = alignment[i], alignment[j]
        if not prev["word"].endswith(" ") and foll["word"] in appended:
            prev["word"] = prev["word"] + foll["word"]
            prev["tokens"] = prev["tokens"] + foll["tokens"]
            foll["word"] = ""
            foll["tokens"] = []
        else:
            i = j
        j += 1
