"""Host side of language identification (WhisperModel.detect_language / language_timeline; the device side is
wm_language_id): the candidate whitelist, faster-whisper's detection rule over per-window results, and the windows
of a language timeline.  Pure Python and numpy: nothing here touches the GPU.

Candidates.  `language_candidates` is a sequence of language codes the deployment serves.  The engine then masks the
language softmax to them (wm_language_id's h_allowed): p_j = exp(x_j - max) / sum over the candidates, a language
outside them has probability exactly 0, so the probabilities are those of the model CONDITIONED on the language being
one of the candidates.  None reads VLOG_AMD_LANGUAGE_CANDIDATES (comma-separated codes, e.g. "en,es,de"); an empty
sequence is off whatever the environment says.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np

from .dims import HOP_LENGTH, N_FRAMES, SAMPLE_RATE

logger = logging.getLogger("vlog_amd")

ENV_CANDIDATES = "VLOG_AMD_LANGUAGE_CANDIDATES"

_english_only_logged = False


@dataclass
class LanguageWindow:
    """One 30 s window of WhisperModel.language_timeline: file times in seconds, the window's best language, its
    probability, and (code, probability) for every language in force, in language-token order."""
    start: float
    end: float
    language: str
    probability: float
    probs: Tuple[Tuple[str, float], ...]


def resolve_language_candidates(value: Optional[Sequence[str]], environ: Mapping[str, str],
                                lang_codes: Sequence[str]) -> Optional[Tuple[str, ...]]:
    """The `language_candidates` argument -> the tuple in force, or None when off.  None reads the environment;
    an empty sequence is off.  ValueError (naming the code, or the variable) for a code outside `lang_codes`, a
    duplicate, a per-file list of lists, and a malformed environment value."""
    if value is None:
        env = environ.get(ENV_CANDIDATES, "")
        if not env.strip():
            return None
        codes = [c.strip() for c in env.split(",")]
        if any(not c for c in codes):
            raise ValueError(f"{ENV_CANDIDATES} must be comma-separated language codes (e.g. en,es,de), got {env!r}")
        where = f"{ENV_CANDIDATES}: "
    else:
        if isinstance(value, str):
            raise ValueError(f"language_candidates: a sequence of language codes expected, got the string {value!r}")
        codes = list(value)
        if any(not isinstance(c, str) for c in codes):
            raise ValueError("language_candidates: one sequence of language codes for all files expected, "
                             "not a per-file list")
        if not codes:
            return None
        where = "language_candidates: "
    known = set(lang_codes)
    seen = set()
    for c in codes:
        if c not in known:
            raise ValueError(f"{where}unknown language code {c!r}")
        if c in seen:
            raise ValueError(f"{where}duplicate language code {c!r}")
        seen.add(c)
    return tuple(codes)


def candidates_in_force(value: Optional[Sequence[str]], environ: Mapping[str, str], lang_codes: Sequence[str],
                        multilingual: bool, language: Optional[str]) -> Optional[Tuple[str, ...]]:
    """resolve_language_candidates, then the two cases in which the candidates are ignored: a call that names its
    language, and an English-only model (logged once per process)."""
    global _english_only_logged
    if not multilingual:
        on = value if value is not None else environ.get(ENV_CANDIDATES, "").strip()
        if on and not _english_only_logged:
            _english_only_logged = True
            logger.warning("language_candidates ignored: the model is English-only")
        return None
    cands = resolve_language_candidates(value, environ, lang_codes)
    return None if language is not None else cands


def candidate_mask(candidates: Sequence[str], lang_codes: Sequence[str]) -> np.ndarray:
    """[n_langs] uint8, 1 at the candidates (wm_language_id's h_allowed)."""
    mask = np.zeros(len(lang_codes), dtype=np.uint8)
    index = {c: j for j, c in enumerate(lang_codes)}
    for c in candidates:
        mask[index[c]] = 1
    return mask


def window_probs(p: np.ndarray, lang_codes: Sequence[str],
                 candidates: Optional[Sequence[str]] = None) -> List[Tuple[str, float]]:
    """One window's probability row -> [(code, p)] sorted descending (stable: the lower language index first), over
    the candidates only when there are any."""
    order = np.argsort(-p, kind="stable")
    if candidates is not None:
        keep = set(candidates)
        return [(lang_codes[j], float(p[j])) for j in order if lang_codes[j] in keep]
    return [(lang_codes[j], float(p[j])) for j in order]


def detection_rule(windows: Sequence[List[Tuple[str, float]]],
                   threshold: float) -> Tuple[str, float, List[Tuple[str, float]]]:
    """faster-whisper's detect_language rule over the per-window results (each sorted descending), in window order:
    the first window whose top probability exceeds `threshold` wins with that window's probabilities; if none does,
    the language most windows put first (the earliest such language on a tie) with its highest probability and the
    last window's probabilities."""
    votes: dict = {}
    all_probs: List[Tuple[str, float]] = []
    for all_probs in windows:
        lang, prob = all_probs[0]
        if prob > threshold:
            return lang, prob, all_probs
        votes.setdefault(lang, []).append(prob)
    lang = max(votes, key=lambda k: len(votes[k]))
    return lang, max(votes[lang]), all_probs


def detection_windows(content_frames: int, segments: int) -> List[Tuple[int, int]]:
    """(seek, size) in mel frames of the windows detect_language looks at: the first always, window i > 0 while it
    starts inside the content."""
    out = []
    for i in range(max(1, segments)):
        seek = i * N_FRAMES
        if i > 0 and seek >= content_frames:
            break
        out.append((seek, max(0, min(N_FRAMES, content_frames - seek))))
    return out


def timeline_windows(content_frames: int, max_windows: Optional[int] = None) -> List[Tuple[int, int]]:
    """(seek, size) of the consecutive 30 s windows of `content_frames` mel frames (the last one ragged), at most
    max_windows of them."""
    if max_windows is not None and max_windows < 1:
        raise ValueError("max_windows must be >= 1")
    wins = [(s, min(N_FRAMES, content_frames - s)) for s in range(0, max(content_frames, 0), N_FRAMES)]
    return wins if max_windows is None else wins[:max_windows]


def window_times(windows: Sequence[Tuple[int, int]], speech_chunks: Optional[List[dict]]) -> List[Tuple[float, float]]:
    """(start, end) of each window in file time: seconds of the decoded audio, moved back through the VAD's chunks
    with restore_speech_timestamps' arithmetic (a start through the chunk it falls in, an end that falls on a chunk's
    last sample stays in that chunk)."""
    sec = HOP_LENGTH / SAMPLE_RATE
    times = [(round(s * sec, 2), round((s + n) * sec, 2)) for s, n in windows]
    if not speech_chunks:
        return times
    from .vad import SpeechTimestampsMap
    m = SpeechTimestampsMap(speech_chunks, SAMPLE_RATE)
    return [(m.get_original_time(a), m.get_original_time(b, is_end=True)) for a, b in times]
