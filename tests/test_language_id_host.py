"""CPU: the host side of language identification (vlog_amd/language_id.py and its callers in transcribe.py) against
tests/lang_id_ref.py: argument / environment resolution of language_candidates, the k-window detection rule against
the one-window-at-a-time loop, and language_timeline's windows and restored times (a stub engine stands in for
wm_encode / wm_language_id; no GPU needed)."""
import logging
import threading

import numpy as np
import pytest
import torch

import lang_id_ref as ref
from vlog_amd import language_id as lid
from vlog_amd.dims import model_dims
from vlog_amd.transcribe import LanguageWindow, WhisperModel

ENV = "VLOG_AMD_LANGUAGE_CANDIDATES"
CODES = model_dims("tiny").specials.lang_codes


class _StubEngine:
    """encode records its windows; detect_language / language_id answer from `tables` (one row per window, by the
    window's index seek // 3000), masked and renormalised in float64 as lang_id_ref defines."""

    def __init__(self, tables):
        self.tables = np.asarray(tables, dtype=np.float64)
        self.calls = []
        self.seeks = []

    def encode(self, features, seeks, sizes):
        self.calls.append(("encode", list(seeks), list(sizes)))
        self.seeks = list(seeks)
        return torch.zeros((len(seeks), 1, 1))

    def cross_kv(self, enc, slot0=0):
        self.calls.append(("cross_kv", enc.shape[0], slot0))

    def detect_language(self, slots, lang_begin, n_langs):
        self.calls.append(("detect_language", list(slots)))
        return np.stack([self.tables[self.seeks[s] // 3000] for s in slots]).astype(np.float32)

    def language_id(self, slots, lang_begin, n_langs, allowed=None):
        self.calls.append(("language_id", list(slots), None if allowed is None else np.asarray(allowed).copy()))
        rows = [self.tables[self.seeks[s] // 3000] for s in slots]
        if allowed is not None:
            rows = [ref.renormalised(r, allowed) for r in rows]
        probs = np.stack(rows).astype(np.float32)
        top = probs.argmax(1).astype(np.int32)
        return probs, top, probs[np.arange(len(slots)), top]


def _model(tables, name="tiny", batch=150):
    m = WhisperModel.__new__(WhisperModel)
    m.dims = model_dims(name)
    m.engine = _StubEngine(tables)
    m._lock = threading.RLock()
    m.throughput = False
    m._batched = type("P", (), {"max_batch_windows": batch})()
    m._features = lambda audio: torch.zeros((m.dims.n_mels, len(audio) // 160 + 1))
    return m


# ---------------------------------------------------------------------------------------------- resolution
def test_off_by_default(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    assert lid.resolve_language_candidates(None, {}, CODES) is None
    assert _model([])._language_candidates(None) is None


def test_argument_environment_and_the_empty_sequence(monkeypatch):
    m = _model([])
    monkeypatch.delenv(ENV, raising=False)
    assert m._language_candidates(["en", "es"]) == ("en", "es")
    assert m._language_candidates(("de",)) == ("de",)
    monkeypatch.setenv(ENV, "en, es,de")
    assert m._language_candidates(None) == ("en", "es", "de")
    assert m._language_candidates(["fr", "it"]) == ("fr", "it")          # the argument beats the environment
    assert m._language_candidates([]) is None                              # the empty sequence turns it off
    assert m._language_candidates(()) is None
    monkeypatch.setenv(ENV, "  ")
    assert m._language_candidates(None) is None


def test_ignored_with_a_language_and_in_an_english_only_model(monkeypatch, caplog):
    monkeypatch.setenv(ENV, "en,es")
    m = _model([])
    assert m._language_candidates(None, "de") is None
    assert m._language_candidates(["en", "fr"], "de") is None
    with pytest.raises(ValueError):                                        # still validated when ignored
        m._language_candidates(["en", "xx"], "de")
    en = _model([], "tiny.en")
    monkeypatch.setattr(lid, "_english_only_logged", False)
    with caplog.at_level(logging.WARNING, logger="vlog_amd"):
        assert en._language_candidates(["en", "es"]) is None
        assert en._language_candidates(None) is None
        assert en.detect_language(features=torch.zeros((80, 3001)), language_candidates=["en"]) == ("en", 1.0, [("en", 1.0)])
    assert sum("English-only" in r.getMessage() for r in caplog.records) == 1      # logged once


@pytest.mark.parametrize("value, env, needle", [
    (["en", "xx"], None, "language_candidates: unknown language code 'xx'"),
    (["en", "es", "en"], None, "language_candidates: duplicate language code 'en'"),
    ([["en"], ["es"]], None, "not a per-file list"),
    ("en", None, "a sequence of language codes expected"),
    (None, "en,,es", "VLOG_AMD_LANGUAGE_CANDIDATES must be comma-separated language codes"),
    (None, "en,", "VLOG_AMD_LANGUAGE_CANDIDATES must be comma-separated language codes"),
    (None, "en,klingon", "VLOG_AMD_LANGUAGE_CANDIDATES: unknown language code 'klingon'"),
    (None, "es,es", "VLOG_AMD_LANGUAGE_CANDIDATES: duplicate language code 'es'"),
])
def test_value_errors_name_the_code_or_the_variable(monkeypatch, value, env, needle):
    if env is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, env)
    with pytest.raises(ValueError) as ei:
        _model([])._language_candidates(value)
    assert needle in str(ei.value)


def test_candidate_mask_and_window_probs():
    mask = lid.candidate_mask(("es", "en"), CODES)
    assert mask.dtype == np.uint8 and mask.sum() == 2 and mask[CODES.index("en")] == 1 and mask[CODES.index("es")] == 1
    p = np.zeros(len(CODES), np.float32)
    p[CODES.index("en")], p[CODES.index("es")] = 0.25, 0.75
    assert lid.window_probs(p, CODES, ("en", "es")) == [("es", 0.75), ("en", 0.25)]
    q = np.full(len(CODES), 1.0 / len(CODES), np.float32)                  # all tied: language-token order
    assert [c for c, _ in lid.window_probs(q, CODES)] == list(CODES)


# ---------------------------------------------------------------------------------------------- the k-window rule
def _tables(rng, k):
    """k per-window probability tables whose tops come from three languages (so votes tie and repeat) with top
    probabilities on both sides of the thresholds used."""
    pool = rng.choice(len(CODES), 3, replace=False)
    out = []
    for _ in range(k):
        t = float(rng.uniform(0.2, 0.97))
        p = rng.dirichlet(np.ones(len(CODES))) * (1.0 - t)
        p[int(rng.choice(pool))] += t
        out.append(p)
    return np.stack(out)


@pytest.mark.parametrize("block", range(4))
def test_k_window_rule_matches_the_one_window_loop(monkeypatch, block):
    """200 seeded tables (4 x 50): the batched path with every language a candidate gives the language and the
    probability of today's loop, and of the float64 definition; it encodes once and identifies once."""
    monkeypatch.delenv(ENV, raising=False)
    for seed in range(50 * block, 50 * block + 50):
        rng = np.random.default_rng(seed)
        k = int(rng.integers(1, 6))
        thr = float(rng.choice([0.3, 0.5, 0.7, 0.9]))
        tables = _tables(rng, k)
        feats = torch.zeros((80, 3000 * k + 1))
        old_m, new_m = _model(tables), _model(tables)
        old = old_m.detect_language(features=feats, language_detection_segments=k, language_detection_threshold=thr)
        new = new_m.detect_language(features=feats, language_detection_segments=k, language_detection_threshold=thr,
                                    language_candidates=list(CODES))
        assert new[0] == old[0] and new[1] == old[1], (seed, old[:2], new[:2])
        assert new[2] == old[2]
        tops = [(CODES[int(np.argmax(t.astype(np.float32)))], float(t.astype(np.float32).max())) for t in tables]
        want = ref.detection_rule(tops, thr)
        assert (new[0], new[1]) == want[:2], (seed, want, new[:2])
        assert [c[0] for c in old_m.engine.calls].count("detect_language") == want[2] + 1     # the loop stops there
        assert [c[0] for c in new_m.engine.calls] == ["encode", "cross_kv", "language_id"]
        assert new_m.engine.calls[0][1] == [3000 * i for i in range(k)]
        assert new_m.engine.calls[2][1] == list(range(k))


def test_k_window_rule_under_a_mask(monkeypatch):
    """Three candidates: the probabilities are over them only (sum 1, sorted descending) and the rule runs on the
    renormalised tables."""
    monkeypatch.setenv(ENV, "en,es,de")
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        k = int(rng.integers(1, 5))
        tables = _tables(rng, k)
        m = _model(tables)
        lang, prob, allp = m.detect_language(features=torch.zeros((80, 3000 * k + 1)), language_detection_segments=k,
                                             language_detection_threshold=0.6)
        mask = lid.candidate_mask(("en", "es", "de"), CODES)
        assert np.array_equal(m.engine.calls[2][2], mask)
        rows = [ref.renormalised(t, mask).astype(np.float32) for t in tables]
        tops = [(CODES[ref.top(r)[0]], float(r.max())) for r in rows]
        want = ref.detection_rule(tops, 0.6)
        assert (lang, prob) == want[:2]
        assert sorted(c for c, _ in allp) == ["de", "en", "es"]
        assert abs(sum(p for _, p in allp) - 1.0) < 1e-6
        assert [p for _, p in allp] == sorted((p for _, p in allp), reverse=True)


def test_detection_windows_stop_at_the_content():
    assert lid.detection_windows(7000, 5) == [(0, 3000), (3000, 3000), (6000, 1000)]
    assert lid.detection_windows(100, 3) == [(0, 100)]
    assert lid.detection_windows(0, 2) == [(0, 0)]                        # the first window always (as the loop)
    assert lid.detection_windows(6000, 0) == [(0, 3000)]


# ---------------------------------------------------------------------------------------------- language_timeline
def _timeline_tables(n):
    rng = np.random.default_rng(7)
    return np.stack([rng.dirichlet(np.ones(len(CODES))) for _ in range(n)])


@pytest.mark.parametrize("seconds, want", [
    (12.5, [(0.0, 12.5)]),                                  # shorter than one window
    (60.0, [(0.0, 30.0), (30.0, 60.0)]),                    # an exact multiple
    (70.0, [(0.0, 30.0), (30.0, 60.0), (60.0, 70.0)]),      # a ragged tail
])
def test_timeline_window_bounds(monkeypatch, seconds, want):
    monkeypatch.delenv(ENV, raising=False)
    tables = _timeline_tables(3)
    m = _model(tables)
    out = m.language_timeline(np.zeros(int(seconds * 16000), np.float32))
    assert [(w.start, w.end) for w in out] == want
    assert all(isinstance(w, LanguageWindow) for w in out)
    for i, w in enumerate(out):
        row = tables[i].astype(np.float32)
        assert w.language == CODES[int(row.argmax())] and w.probability == float(row.max())
        assert w.probs == tuple((c, float(p)) for c, p in zip(CODES, row))
    assert [c[0] for c in m.engine.calls] == ["encode", "cross_kv", "language_id"]      # one batch, nothing decoded
    frames = int(seconds * 100)
    assert m.engine.calls[0][1:] == ([3000 * i for i in range(len(want))],
                                     [min(3000, frames - 3000 * i) for i in range(len(want))])


def test_timeline_batches_max_windows_and_candidates(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    tables = _timeline_tables(5)
    m = _model(tables, batch=2)
    out = m.language_timeline(np.zeros(135 * 16000, np.float32), language_candidates=["es", "en"])
    assert [(w.start, w.end) for w in out] == [(0.0, 30.0), (30.0, 60.0), (60.0, 90.0), (90.0, 120.0), (120.0, 135.0)]
    assert [c[0] for c in m.engine.calls] == ["encode", "cross_kv", "language_id"] * 3          # batches of 2, 2, 1
    assert [c[1] for c in m.engine.calls if c[0] == "encode"] == [[0, 3000], [6000, 9000], [12000]]
    mask = lid.candidate_mask(("en", "es"), CODES)
    for i, w in enumerate(out):
        row = ref.renormalised(tables[i], mask).astype(np.float32)
        assert [c for c, _ in w.probs] == ["en", "es"]                                     # language-token order
        assert w.probs == (("en", float(row[CODES.index("en")])), ("es", float(row[CODES.index("es")])))
        assert w.language == ("en" if w.probs[0][1] >= w.probs[1][1] else "es")
        assert w.probability == max(p for _, p in w.probs)
    few = _model(tables, batch=2).language_timeline(np.zeros(135 * 16000, np.float32), max_windows=3)
    assert [(w.start, w.end) for w in few] == [(0.0, 30.0), (30.0, 60.0), (60.0, 90.0)]
    with pytest.raises(ValueError, match="max_windows"):
        m.language_timeline(np.zeros(16000, np.float32), max_windows=0)


@pytest.mark.parametrize("chunks, want", [
    # 20 s + 25 s of speech with gaps of 5 s and 15 s: the first window's end falls inside the second chunk
    ([(5, 25), (40, 65)], [(5.0, 50.0), (50.0, 65.0)]),
    # a window's end exactly on a chunk's last sample stays in that chunk; the next window starts after the gap
    ([(0, 30), (40, 50)], [(0.0, 30.0), (40.0, 50.0)]),
    ([(2, 10)], [(2.0, 10.0)]),
])
def test_timeline_restores_file_times_through_the_vad_chunks(monkeypatch, chunks, want):
    monkeypatch.delenv(ENV, raising=False)
    import vlog_amd.vad as vad
    sc = [dict(start=a * 16000, end=b * 16000) for a, b in chunks]
    monkeypatch.setattr(vad, "get_speech_timestamps", lambda audio, opts, model: sc)
    m = _model(_timeline_tables(3))
    out = m.language_timeline(np.zeros(70 * 16000, np.float32), vad_filter=True)
    assert [(w.start, w.end) for w in out] == want
    # the same arithmetic as a segment without words going through restore_speech_timestamps
    seg = type("S", (), {})
    segs = []
    t = 0.0
    total = sum(b - a for a, b in chunks)
    while t < total:
        s = seg()
        s.start, s.end, s.words = t, min(t + 30.0, float(total)), None
        segs.append(s)
        t += 30.0
    restored = list(vad.restore_speech_timestamps(iter(segs), sc, 16000))
    assert [(s.start, s.end) for s in restored] == want


def test_timeline_without_speech_and_in_an_english_only_model(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    import vlog_amd.vad as vad
    monkeypatch.setattr(vad, "get_speech_timestamps", lambda audio, opts, model: [])
    m = _model(_timeline_tables(1))
    assert m.language_timeline(np.zeros(16000, np.float32), vad_filter=True) == []
    assert m.engine.calls == []
    with pytest.raises(ValueError, match="multilingual"):
        _model([], "tiny.en").language_timeline(np.zeros(16000, np.float32))


def test_exported_from_the_compat_package():
    import os
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat")
    sys.path.insert(0, compat)
    try:
        import faster_whisper
        assert faster_whisper.LanguageWindow is LanguageWindow and "LanguageWindow" in faster_whisper.__all__
    finally:
        sys.path.remove(compat)
