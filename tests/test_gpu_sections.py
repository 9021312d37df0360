"""WhisperModel.transcribe(sections=N): one file cut at long silences into contiguous sections, the sections decoded in
lockstep (each round one ragged engine.generate over the next window of every section in flight).

Two references.  Without VAD a section is exactly a clip: the sectioned transcript must equal, section by section,
`transcribe(x, clip_timestamps=[b0 / 100, b1 / 100])` with the ids renumbered.  With VAD (where clip_timestamps is
not available) the reference is the same call with sections_in_flight=1, which decodes the sections one after another
through the same driver, every window alone in its pass as in the one-file loop.  `_same` compares id, seek, tokens,
temperature, start, end and text exactly and avg_logprob / no_speech_prob to 1e-3, as
tests/test_gpu_transcribe_many_seq.py does.

Files: 140 s (speech_like pieces of 44, 44 and 46 s with 3 s of zeros between them) and 148 s (four 34 s pieces with
4 s of zeros between them, which VAD removes); a 20 s file for the one-section case.

Near-ties: rows of different sections share decoder passes, so the GEMM routes follow another row count than in the
reference and a top-2 tie below f32 rounding could flip a token (the docstring of tests/test_gpu_transcribe_many_seq.py
has a worked case).  The comparisons are exact all the same; the seeds below met no such tie."""
import numpy as np
import pytest

from vlog_amd.audio import speech_like
from vlog_amd.seek_state import chunk_joins

pytestmark = pytest.mark.gpu


def _pieces(lengths, seed0, gap_s):
    gap = np.zeros(int(16000 * gap_s), np.float32)
    parts = []
    for i, s in enumerate(lengths):
        parts += [speech_like(float(s), seed0 + i), gap]
    return np.concatenate(parts[:-1])


@pytest.fixture(scope="module")
def gapped():
    return _pieces((44, 44, 46), 2100, 3.0)                 # 140 s; the gaps are 44-47 s and 91-94 s


@pytest.fixture(scope="module")
def long_vad():
    return _pieces((34, 34, 34, 34), 2200, 4.0)             # 148 s


@pytest.fixture(scope="module")
def model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cuda", eot_after=60)


@pytest.fixture(scope="module")
def margin_model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:0:margin", device="cuda")


def _same(a, b, words=False):
    assert len(a) == len(b), (len(a), len(b))
    for x, y in zip(a, b):
        assert (x.id, x.seek, x.tokens, x.temperature) == (y.id, y.seek, y.tokens, y.temperature), (x, y)
        assert (x.start, x.end, x.text) == (y.start, y.end, y.text), (x, y)
        assert abs(x.avg_logprob - y.avg_logprob) <= 1e-3 and abs(x.no_speech_prob - y.no_speech_prob) <= 1e-3, (x, y)
        if words:
            assert [(w.word, w.start, w.end) for w in x.words] == [(w.word, w.start, w.end) for w in y.words], (x, y)


def _run(model, x, **kw):
    segs, info = model.transcribe(x, **kw)
    return list(segs), info


def _count_first_passes(model, t0=0.0):
    """wraps engine.generate -> (list that receives the number of slots of every call at temperature t0, undo)"""
    eng = model.engine
    inner = eng.generate
    calls = []

    def counted(slots, *a, **kw):
        if kw.get("temperature", 0.0) == t0:
            calls.append(len(slots))
        return inner(slots, *a, **kw)

    eng.generate = counted

    def undo():
        del eng.generate                                    # (the instance attribute: the class's method is back)

    return calls, undo


def _by_clips(model, x, bounds, **kw):
    """the sections as clips of the one-file loop, ids renumbered in output order -> (segments, windows per section)"""
    out, windows = [], []
    for b0, b1 in bounds:
        calls, undo = _count_first_passes(model, 0.0)
        try:
            segs, _ = _run(model, x, clip_timestamps=[b0 / 100, b1 / 100], **kw)
        finally:
            undo()
        windows.append(len(calls))
        for s in segs:
            s.id = len(out) + 1
            out.append(s)
    return out, windows


GREEDY = dict(language="en", beam_size=1, temperature=0.0)


@pytest.fixture(scope="module")
def greedy_ref(model, gapped):
    """sections=3 of the 140 s file, greedy, and its reference by clips; shared by cases a and e, left unchanged"""
    segs, info = _run(model, gapped, sections=3, **GREEDY)
    bounds = info.transcription_options.section_frames
    ref, windows = _by_clips(model, gapped, bounds, **GREEDY)
    return segs, bounds, ref, windows


def test_a_greedy_sections_equal_clips(greedy_ref, gapped):
    segs, bounds, ref, windows = greedy_ref
    content = len(gapped) // 160
    assert len(bounds) == 3 and bounds[0][0] == 0 and bounds[-1][1] == content
    assert bounds[0][1] == bounds[1][0] and bounds[1][1] == bounds[2][0]
    assert 4400 <= bounds[0][1] <= 4700 and 9100 <= bounds[1][1] <= 9400, bounds        # inside the zero gaps
    _same(segs, ref)
    assert len(segs) > 6 and [s.id for s in segs] == list(range(1, len(segs) + 1))
    assert all(w >= 2 for w in windows)                     # later windows of a section carry its previous text
    for (b0, b1) in bounds:
        assert [s for s in segs if b0 <= s.seek < b1]


def test_b_workers_call_on_margin_model(margin_model, long_vad):
    from vlog_amd.transcribe import VadOptions
    from vlog_amd.vad import get_speech_timestamps
    kw = dict(language=None, task="transcribe", beam_size=5, vad_filter=True)
    segs, info = _run(margin_model, long_vad, sections=4, **kw)
    ref, rinfo = _run(margin_model, long_vad, sections=4, sections_in_flight=1, **kw)
    bounds = info.transcription_options.section_frames
    assert bounds == rinfo.transcription_options.section_frames and len(bounds) >= 3, bounds
    assert info.language == rinfo.language and info.duration_after_vad == rinfo.duration_after_vad
    _same(segs, ref)
    assert segs and not [s for s in segs if s.temperature > 0]
    assert [s.id for s in segs] == list(range(1, len(segs) + 1))
    assert [s.seek for s in segs] == sorted(s.seek for s in segs)            # section order, window order
    joins = chunk_joins(get_speech_timestamps(long_vad, VadOptions(), margin_model))
    assert {b0 for b0, _ in bounds[1:]} <= {f for f, s in joins if s >= 0.5}, (bounds, joins)
    assert all(b1 - b0 >= 3000 for b0, b1 in bounds)


def test_c_word_timestamps(model, long_vad):
    kw = dict(word_timestamps=True, vad_filter=True, **GREEDY)
    segs, info = _run(model, long_vad, sections=4, **kw)
    ref, _ = _run(model, long_vad, sections=4, sections_in_flight=1, **kw)
    assert len(info.transcription_options.section_frames) >= 3
    _same(segs, ref, words=True)
    assert any(s.words for s in segs)


def test_d_every_window_falls_back(model, gapped):
    """random weights fail the log-prob threshold: every window is re-decoded alone at 0.4 with seed window + 1
    against its own slot"""
    kw = dict(language="en", beam_size=5, temperature=(0.0, 0.4))
    segs, info = _run(model, gapped, sections=3, **kw)
    ref, _ = _run(model, gapped, sections=3, sections_in_flight=1, **kw)
    assert len(info.transcription_options.section_frames) == 3
    _same(segs, ref)
    assert segs and {s.temperature for s in segs} == {0.4}


def test_e_rounds_share_one_generate(model, gapped, greedy_ref):
    segs, bounds, _, windows = greedy_ref
    for in_flight, expect, rows in ((None, max(windows), 3), (1, sum(windows), 1), (2, None, 2)):
        calls, undo = _count_first_passes(model, 0.0)
        try:
            got, info = _run(model, gapped, sections=3, sections_in_flight=in_flight, **GREEDY)
        finally:
            undo()
        assert info.transcription_options.section_frames == bounds
        _same(got, segs)
        assert max(calls) == rows and (expect is None or len(calls) == expect), (in_flight, calls, windows)
        assert sum(calls) == sum(windows)                   # every window decoded once


def test_f_switch_off_and_argument_checks(model, gapped, greedy_ref, monkeypatch):
    plain, pinfo = _run(model, gapped[: 16000 * 70], **GREEDY)
    one, oinfo = _run(model, gapped[: 16000 * 70], sections=1, **GREEDY)
    _same(one, plain)
    assert pinfo.transcription_options == oinfo.transcription_options
    assert oinfo.transcription_options.section_frames is None

    monkeypatch.setenv("VLOG_AMD_SECTIONS", "3")
    env, einfo = _run(model, gapped, **GREEDY)
    monkeypatch.delenv("VLOG_AMD_SECTIONS")
    assert einfo.transcription_options.section_frames == greedy_ref[1]
    _same(env, greedy_ref[0])

    for bad in (0, -2, 33):
        with pytest.raises(ValueError):
            model.transcribe(gapped, sections=bad, **GREEDY)
    with pytest.raises(ValueError):
        model.transcribe(gapped, sections=2, clip_timestamps="10", **GREEDY)
    monkeypatch.setattr(model, "throughput", True)
    with pytest.raises(ValueError):
        model.transcribe(gapped, sections=2, **GREEDY)
    monkeypatch.undo()

    short = speech_like(20.0, 2300)
    four, finfo = _run(model, short, sections=4, **GREEDY)
    assert finfo.transcription_options.section_frames == [(0, 2000)]
    _same(four, _run(model, short, **GREEDY)[0])
    assert four
