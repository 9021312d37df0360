"""Language identification as defined, in float64 (the reference of tests/test_language_id_host.py and
tests/test_gpu_language_id.py; include/whisper_mi355.h wm_language_id, vlog_amd/language_id.py):

  * the probabilities are the softmax of the language logits over the ALLOWED languages; a masked language has
    probability exactly 0;
  * the best language is the argmax, the lowest index winning ties;
  * over several windows, faster-whisper's rule: the first window whose top probability exceeds the threshold wins;
    when none does, the language most windows put first (the earliest such language on a tie), with the highest
    probability it reached.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np


def masked_softmax(logits: Sequence[float], allowed: Optional[Sequence[int]] = None) -> np.ndarray:
    x = np.asarray(logits, dtype=np.float64)
    keep = np.ones(x.shape, dtype=bool) if allowed is None else (np.asarray(allowed) != 0)
    if not keep.any():
        raise ValueError("no language allowed")
    out = np.zeros_like(x)
    z = x[keep] - x[keep].max()
    e = np.exp(z)
    out[keep] = e / e.sum()
    return out


def renormalised(probs: Sequence[float], allowed: Sequence[int]) -> np.ndarray:
    """The masked softmax from the unmasked one: the allowed entries divided by their sum, the rest 0."""
    p = np.asarray(probs, dtype=np.float64)
    keep = np.asarray(allowed) != 0
    out = np.zeros_like(p)
    out[keep] = p[keep] / p[keep].sum()
    return out


def top(probs: Sequence[float]) -> Tuple[int, float]:
    p = np.asarray(probs, dtype=np.float64)
    j = int(np.argmax(p))                      # numpy returns the first maximum: the lowest index wins ties
    return j, float(p[j])


def detection_rule(window_tops: Sequence[Tuple[str, float]], threshold: float) -> Tuple[str, float, int]:
    """window_tops: (language, probability) of each window's best language, in window order.
    -> (language, probability, index of the window whose probabilities are reported)."""
    votes: dict = {}
    order: List[str] = []
    for i, (lang, prob) in enumerate(window_tops):
        if prob > threshold:
            return lang, prob, i
        if lang not in votes:
            votes[lang] = []
            order.append(lang)
        votes[lang].append(prob)
    best = order[0]
    for lang in order[1:]:
        if len(votes[lang]) > len(votes[best]):
            best = lang
    return best, max(votes[best]), len(window_tops) - 1
