"""WhisperModel.align end to end on the MI355X (synthetic tiny model): a 40-word, 3-line text against a 70 s clip,
with a token budget of 48 so that the text needs at least three windows.  What is pinned is the plumbing and the
loop: every word once and in order, sane times, line -> segment / cue mapping, determinism, equality with the
host loop driven by hand over engine.align_open_batch, VAD restoration, WebVTT, and the refusals.  Alignment
quality on real speech is not claimed (no trained weights)."""
import numpy as np
import pytest
import torch

from vlog_amd import forced_align as fa
from vlog_amd.audio import speech_like
from vlog_amd.vtt import generate_webvtt

pytestmark = pytest.mark.gpu

TEXT = ("the river ran slow and wide below the old stone bridge where nobody had walked since the morning rain\n"
        "two boats lay still against the bank\n"
        "far off a bell rang once and then the whole valley went quiet again")
LINES = TEXT.split("\n")
BUDGET = 48


@pytest.fixture(scope="module")
def model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cpu", compute_type="int8", eot_after=60)


@pytest.fixture(scope="module")
def clip():
    return np.concatenate([speech_like(30.0, 900), speech_like(30.0, 901), speech_like(10.0, 902)])


@pytest.fixture(scope="module")
def aligned(model, clip):
    return model.align(clip, TEXT, language="en", max_window_tokens=BUDGET)


def _plain(segments):
    return [s._asdict() for s in segments]


def test_every_word_once_in_order_with_sane_times(model, aligned):
    segments, info = aligned
    assert len(TEXT.split()) == 40
    words = [w for s in segments for w in s.words]
    assert [w.word for w in words] == [" " + w for w in TEXT.split()]
    assert info.duration == pytest.approx(70.0) and info.duration_after_vad == info.duration and info.language == "en"
    starts = [w.start for w in words]
    assert all(0.0 <= w.start <= w.end <= info.duration for w in words)
    assert all(a <= b for a, b in zip(starts[:-1], starts[1:]))
    assert all(0.0 <= w.probability <= 1.0 for w in words)
    # the words the audio did not reach: a tail at the clip's end with probability 0
    tail = 0
    for w in reversed(words):
        if not (w.start == w.end == round(info.duration, 2) and w.probability == 0.0):
            break
        tail += 1
    assert tail == info.unaligned_words and sum(len(s.words) for s in segments) == 40
    # the windows: within the budget, in seek order, and as many as the budget forces
    n_tok = sum(len(w["tokens"]) for w in fa.prepare_words(model.tokenizer(language="en"), TEXT)[1])
    assert info.windows == len(info.window_rows)
    assert all(1 <= reached <= offered <= BUDGET + 1 for _, offered, reached in info.window_rows)
    assert [r[0] for r in info.window_rows] == sorted(r[0] for r in info.window_rows)
    if info.unaligned_words == 0:
        assert info.windows >= -(-n_tok // BUDGET) >= 3
    print("window_rows", info.window_rows, "unaligned", info.unaligned_words)


def test_one_segment_per_line_or_its_cues(aligned):
    segments, _ = aligned
    assert [s.id for s in segments] == list(range(1, len(segments) + 1))
    assert len(LINES[0]) > 84 >= max(len(LINES[1]), len(LINES[2]))
    texts = [s.text for s in segments]
    assert texts[-2:] == [" " + LINES[1], " " + LINES[2]]
    head = texts[:-2]
    assert len(head) >= 2 and "".join(head) == " " + LINES[0] and all(len(t.strip()) <= 84 for t in head)
    for s in segments:
        assert s.start == s.words[0].start and s.end == s.words[-1].end
        assert s.temperature == 0.0 and s.no_speech_prob == 0.0 and s.avg_logprob <= 0.0
        assert "".join(w.word for w in s.words) == s.text


def test_two_calls_are_identical(model, clip, aligned):
    again = model.align(clip, TEXT, language="en", max_window_tokens=BUDGET)
    assert _plain(again[0]) == _plain(aligned[0]) and again[1] == aligned[1]


def test_equals_the_host_loop_driven_by_hand(model, clip, aligned):
    eng = model.engine
    tok = model.tokenizer(task="transcribe", language="en")
    feats = model._features(clip)
    heads = model.dims.default_alignment_heads()
    seen = []

    def window(seek, size, tokens):
        seen.append((seek, len(tokens) + 1))
        eng.cross_kv(eng.encode(feats, [seek], [size]), 0)
        return eng.align_open_batch([0], tok.sot_sequence, [tokens], [size], heads, 7)[0]

    segs, stats = fa.forced_align(tok, LINES, feats.shape[1] - 1, len(clip) / 16000, window, max_window_tokens=BUDGET)
    assert segs == _plain(aligned[0])
    assert stats["window_rows"] == aligned[1].window_rows and seen == [r[:2] for r in aligned[1].window_rows]


def test_vad_filter_restores_times_into_the_speech_spans(model):
    """A word's times go back through restore_speech_timestamps by the chunk that holds its midpoint, so the
    restored midpoint lies inside that speech span, and every time lies between the first span's start and the
    last span's end."""
    from vlog_amd.transcribe import VadOptions
    from vlog_amd.vad import get_speech_timestamps
    x = np.concatenate([speech_like(20.0, 910), np.zeros(16000 * 12, np.float32), speech_like(20.0, 911)])
    spans = [(c["start"] / 16000, c["end"] / 16000) for c in get_speech_timestamps(x, VadOptions(), model)]
    kept = sum(e - s for s, e in spans)
    assert spans and kept < len(x) / 16000 - 5.0                  # the silence was found
    segments, info = model.align(x, TEXT, language="en", vad_filter=True, max_window_tokens=BUDGET)
    assert info.duration == pytest.approx(52.0) and info.duration_after_vad == pytest.approx(kept, abs=1e-3)
    words = [w for s in segments for w in s.words]
    assert len(words) == 40
    eps = 0.011                                                   # times are rounded to 0.01
    for w in words:
        assert spans[0][0] - eps <= w.start <= w.end <= spans[-1][1] + eps
        mid = (w.start + w.end) / 2
        assert any(s - eps <= mid <= e + eps for s, e in spans), (w, spans)


def test_webvtt_accepts_the_segments(aligned):
    vtt = generate_webvtt(_plain(aligned[0]))
    assert vtt.startswith("WEBVTT\n\n") and vtt.count(" --> ") == len(aligned[0])
    assert LINES[1] in vtt


def test_refusals(model, clip):
    for empty in ("", " \n \n", []):
        with pytest.raises(ValueError, match="empty"):
            model.align(clip, empty, language="en")
    model.throughput = True
    try:
        with pytest.raises(ValueError, match="throughput"):
            model.align(clip, TEXT, language="en")
    finally:
        model.throughput = False
