"""The history rules' reference (tests/repetition_ref.py) pinned against transformers' RepetitionPenaltyLogitsProcessor
and NoRepeatNGramLogitsProcessor applied to the generated slice, and the prompt builder (vlog_amd/segments.py
build_prompt, faster-whisper 1.1 get_prompt with prefix and hotwords) against literal prompts."""
import numpy as np
import pytest
import torch
from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

from tests.repetition_ref import apply_history_rules, repeated_ngrams
from vlog_amd.segments import build_prompt

V = 300


def _history(rng, g):
    """g tokens over a small alphabet, so that ids and n-grams repeat"""
    return [int(t) for t in rng.integers(0, 4, size=g)]


def _hf(proc, history, logits):
    ids = torch.tensor([history], dtype=torch.long).reshape(1, len(history))
    return proc(ids, torch.from_numpy(logits[None].copy()))[0].numpy()


@pytest.mark.parametrize("penalty", [1.3, 0.7, 2.0])
@pytest.mark.parametrize("g", [0, 1, 7, 40])
def test_repetition_penalty_matches_transformers(penalty, g):
    rng = np.random.default_rng(100 * g + int(penalty * 10))
    logits = (rng.standard_normal(V) * 3).astype(np.float32)
    hist = _history(rng, g)
    got = apply_history_rules(logits, hist, repetition_penalty=penalty)
    ref = _hf(RepetitionPenaltyLogitsProcessor(penalty), hist, logits)
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-6)
    touched = np.zeros(V, bool)
    touched[hist] = True
    assert np.array_equal(got[~touched], logits[~touched].astype(np.float64))
    if g:
        assert not np.allclose(got[touched], logits[touched])


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_no_repeat_ngram_matches_transformers(n):
    # g < n (incl. 0), g == n - 1, g == n, and longer histories with repeats
    for g in sorted({0, max(n - 2, 0), n - 1, n, n + 1, 12, 40}):
        for trial in range(6):
            rng = np.random.default_rng(1000 * n + 10 * g + trial)
            logits = (rng.standard_normal(V) * 3).astype(np.float32)
            hist = _history(rng, g)
            got = apply_history_rules(logits, hist, no_repeat_ngram_size=n)
            ref = _hf(NoRepeatNGramLogitsProcessor(n), hist, logits)
            assert np.array_equal(np.isneginf(got), np.isneginf(ref)), (n, g, hist)
            keep = ~np.isneginf(ref)
            assert np.array_equal(got[keep], logits[keep].astype(np.float64))
            if g < n:
                assert keep.all()
    # the histories above do ban something
    hist = [1, 2, 3, 1, 2, 3, 1, 2][: max(n + 3, 4)] if n <= 3 else [1, 2, 3, 4, 5, 1, 2, 3, 4]
    assert np.isneginf(apply_history_rules(np.zeros(V), hist, no_repeat_ngram_size=n)).any()


def test_both_rules_and_the_invariant_helper():
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal(V) * 3).astype(np.float32)
    hist = [7, 8, 9, 7, 8]
    got = apply_history_rules(logits, hist, 1.3, 3)
    ref = _hf(NoRepeatNGramLogitsProcessor(3), hist, _hf(RepetitionPenaltyLogitsProcessor(1.3), hist, logits))
    assert np.isneginf(got[9]) and np.array_equal(np.isneginf(got), np.isneginf(ref))
    assert np.allclose(got[np.isfinite(got)], ref[np.isfinite(ref)], rtol=1e-6, atol=1e-6)
    assert repeated_ngrams(hist, 2) == [(7, 8)] and repeated_ngrams(hist, 3) == []
    assert repeated_ngrams(hist + [9], 3) == [(7, 8, 9)]
    assert repeated_ngrams([4, 5, 4], 1) == [(4,)]


# ---- prompt builder: a character-code `encode`, so the expected prompts are literal
SOT_SEQ, SOT_PREV, NO_TS, TS_BEGIN = [500, 501, 502], 490, 503, 504


def _encode(text):
    return [ord(c) for c in text]


def _prompt(**kw):
    return build_prompt(_encode, SOT_SEQ, SOT_PREV, NO_TS, TS_BEGIN, 448, **kw)


def test_prompt_plain_and_previous_text():
    assert _prompt() == [500, 501, 502]
    assert _prompt(without_timestamps=True) == [500, 501, 502, 503]
    assert _prompt(previous_tokens=[1, 2, 3]) == [490, 1, 2, 3, 500, 501, 502]
    long_prev = list(range(1000, 1300))
    assert _prompt(previous_tokens=long_prev) == [490] + list(range(1077, 1300)) + [500, 501, 502]


def test_prompt_hotwords_only():
    assert _prompt(hotwords=" ab ") == [490, 32, 97, 98, 500, 501, 502]


def test_prompt_hotwords_with_previous_tokens():
    assert _prompt(hotwords="ab", previous_tokens=[1, 2]) == [490, 32, 97, 98, 1, 2, 500, 501, 502]


def test_prompt_prefix_with_and_without_timestamps():
    assert _prompt(prefix="hi") == [500, 501, 502, 504, 32, 104, 105]
    assert _prompt(prefix=" hi", without_timestamps=True) == [500, 501, 502, 503, 32, 104, 105]
    assert _prompt(prefix="hi", previous_tokens=[9]) == [490, 9, 500, 501, 502, 504, 32, 104, 105]


def test_prompt_prefix_drops_hotwords():
    assert _prompt(prefix="hi", hotwords="ab") == [500, 501, 502, 504, 32, 104, 105]
    assert _prompt(prefix="hi", hotwords="ab", previous_tokens=[9]) == [490, 9, 500, 501, 502, 504, 32, 104, 105]


def test_prompt_long_hotwords_and_prefix_are_truncated():
    # " " + 300 x "a" = 301 tokens >= 224 = max_length // 2: the first 223 stay
    assert _prompt(hotwords="a" * 300) == [490, 32] + [97] * 222 + [500, 501, 502]
    assert _prompt(prefix="a" * 300) == [500, 501, 502, 504, 32] + [97] * 222
    # 223 tokens are below the bound and stay whole
    assert _prompt(hotwords="a" * 222) == [490, 32] + [97] * 222 + [500, 501, 502]
