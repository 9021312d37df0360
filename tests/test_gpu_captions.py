"""Caption shaping (max_line_width / max_line_count / max_cue_seconds) through every decode form of transcribe.

The yardstick of every case is the same form's own unshaped run: the same call with word_timestamps=True and shaping
off makes the same engine calls in the same order, and `shape_captions` over its segments must equal the shaped call
exactly: id, seek, start, end, text, tokens, the statistics, and every word's text, start, end and probability
(dataclass equality over all fields).  The rule itself is checked on the CPU (tests/test_captions_host.py).

Tiny synthetic models, speech_like clips of 21 to 75 s as in tests/test_gpu_transcribe_many_seq.py.  Every decode form
runs on both models, because they show different things.  The margin-planted model writes segments of 65 to 94
characters in 5 to 12 words, so the rule cuts nearly every parent: that is where a third of the parents cut is
asserted.  The random-weight model (eot_after=60) writes segments of 4 to 8 characters with one word or none on these
clips (measured: 9 parents on the 75 s clip, 6 with a word, none with two), so no width can cut them; what it shows is
the rest of the plumbing: parents without words passing through, a word that runs across a timestamp pair and is given
whole to the earlier segment with its tokens, and the ids."""
import numpy as np
import pytest

from vlog_amd.audio import speech_like, write_wav
from vlog_amd.captions import shape_captions
from vlog_amd.vtt import generate_webvtt

pytestmark = pytest.mark.gpu

GREEDY = dict(language="en", beam_size=1, temperature=0.0)
WIDTH = 20
ENV = ("VLOG_AMD_MAX_LINE_WIDTH", "VLOG_AMD_MAX_LINE_COUNT", "VLOG_AMD_MAX_CUE_SECONDS")


@pytest.fixture(scope="module")
def margin_model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:0:margin", device="cuda")


@pytest.fixture(scope="module")
def random_model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cuda", eot_after=60)


@pytest.fixture(params=["margin", "random"])
def model(request, margin_model, random_model):
    """-> (the model, whether its text is long enough for the rule to cut)"""
    return (margin_model, True) if request.param == "margin" else (random_model, False)


@pytest.fixture(scope="module")
def long_clip():
    return speech_like(75.0, 1300)


@pytest.fixture(scope="module")
def gap_clip():
    return np.concatenate([speech_like(24.0, 1302), np.zeros(16000 * 4, np.float32), speech_like(20.0, 1303)])


@pytest.fixture(autouse=True)
def no_caption_environment(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _run(call, *a, **kw):
    segs, info = call(*a, **kw)
    return list(segs), info


def _equal(got, expected):
    assert len(got) == len(expected), (len(got), len(expected))
    for x, y in zip(got, expected):
        assert x == y, (x, y)
    assert [s.id for s in got] == list(range(1, len(got) + 1))
    assert all(s.words is not None for s in got)


def _cut(parents, *opts):
    """how many of the parents the rule cuts into more than one cue"""
    return sum(1 for p in parents if len(list(shape_captions([p], *opts))) > 1)


def test_one_file_loop_greedy(model, long_clip):
    model, cuts = model
    base, _ = _run(model.transcribe, long_clip, word_timestamps=True, **GREEDY)
    got, info = _run(model.transcribe, long_clip, word_timestamps=False, max_line_width=WIDTH, **GREEDY)
    _equal(got, list(shape_captions(base, WIDTH)))
    cut = _cut(base, WIDTH)
    print(f"parents {len(base)}, cut {cut}, cues {len(got)}")
    assert len(base) >= 3
    if cuts:
        assert 3 * cut >= len(base), (cut, len(base))                       # a test that never cuts shows nothing
        assert any("\n" in s.text for s in got)
    o = info.transcription_options
    assert (o.max_line_width, o.max_line_count, o.max_cue_seconds, o.word_timestamps) == (WIDTH, 2, None, True)
    for s in got:
        lines = s.text.strip().split("\n")
        assert len(lines) <= 2, s
        assert all(len(l) <= WIDTH or l in [w.word.strip() for w in s.words] for l in lines), s


def test_beam5_vad_with_a_removed_gap(model, gap_clip):
    model, cuts = model
    kw = dict(language="en", beam_size=5, temperature=0.0, vad_filter=True)
    base, binfo = _run(model.transcribe, gap_clip, word_timestamps=True, **kw)
    got, info = _run(model.transcribe, gap_clip, max_line_width=WIDTH, max_line_count=1, max_cue_seconds=4.0, **kw)
    _equal(got, list(shape_captions(base, WIDTH, 1, 4.0)))
    assert info.duration_after_vad == binfo.duration_after_vad <= info.duration - 2.5      # the gap was removed
    assert any(s.start > 28.0 for s in got)                                  # ... and the times are the file's own
    for s in got:                                                            # no cue stays up over the removed gap
        assert all(b.start - a.end <= 3.0 for a, b in zip(s.words, s.words[1:]))
        assert "\n" not in s.text and (len(s.words) <= 1 or s.end - s.start <= 4.0)
    assert len(got) > len(base) or not cuts


def test_sections(model, long_clip):
    model, cuts = model
    base, binfo = _run(model.transcribe, long_clip, sections=2, word_timestamps=True, **GREEDY)
    got, info = _run(model.transcribe, long_clip, sections=2, max_line_width=WIDTH, **GREEDY)
    bounds = info.transcription_options.section_frames
    assert len(bounds) == 2 and bounds == binfo.transcription_options.section_frames
    _equal(got, list(shape_captions(base, WIDTH)))
    assert [s.seek for s in got] == sorted(s.seek for s in got)              # file order
    assert all([s for s in got if b0 <= s.seek < b1] for b0, b1 in bounds)
    assert len(got) > len(base) or not cuts


def test_transcribe_many(model, long_clip):
    model, cuts = model
    files = [long_clip, speech_like(21.0, 1301), speech_like(33.0, 1305)]
    base = model.transcribe_many(files, max_files=2, word_timestamps=True, **GREEDY)
    got = model.transcribe_many(files, max_files=2, max_line_width=WIDTH, max_cue_seconds=5.0, **GREEDY)
    assert len(got) == 3
    for (segs, info), (bsegs, _) in zip(got, base):
        _equal(segs, list(shape_captions(bsegs, WIDTH, 2, 5.0)))             # ids 1, 2, ... per file
        o = info.transcription_options
        assert (o.max_line_width, o.max_line_count, o.max_cue_seconds, o.word_timestamps) == (WIDTH, 2, 5.0, True)
    assert sum(len(s) for s, _ in got) > sum(len(s) for s, _ in base) or not cuts


def test_batched_pipeline(model, gap_clip):
    model, cuts = model
    from vlog_amd.transcribe import BatchedInferencePipeline
    pipe = BatchedInferencePipeline(model)
    kw = dict(without_timestamps=False, **GREEDY)
    base, _ = _run(pipe.transcribe, gap_clip, word_timestamps=True, **kw)
    got, info = _run(pipe.transcribe, gap_clip, max_line_width=WIDTH, **kw)
    _equal(got, list(shape_captions(base, WIDTH)))
    assert len(base) >= 2 and (len(got) > len(base) or not cuts)
    o = info.transcription_options
    assert (o.max_line_width, o.max_line_count, o.max_cue_seconds, o.word_timestamps) == (WIDTH, 2, None, True)
    many = pipe.transcribe_many([gap_clip], max_line_width=WIDTH, **kw)
    _equal(many[0][0], got)


def test_workers_call_reads_the_environment(margin_model, gap_clip, tmp_path, monkeypatch):
    wav = tmp_path / "clip.wav"
    write_wav(str(wav), gap_clip)
    worker = dict(language=None, task="transcribe", beam_size=5, vad_filter=True)
    today, tinfo = _run(margin_model.transcribe, str(wav), **worker)
    explicit, _ = _run(margin_model.transcribe, str(wav), max_line_width=24, max_line_count=2, max_cue_seconds=4.0,
                       **worker)
    monkeypatch.setenv(ENV[0], "24")
    monkeypatch.setenv(ENV[1], "2")
    monkeypatch.setenv(ENV[2], "4")
    got, info = _run(margin_model.transcribe, str(wav), **worker)
    _equal(got, explicit)
    assert len(got) > len(today)
    o = info.transcription_options
    assert (o.max_line_width, o.max_line_count, o.max_cue_seconds, o.word_timestamps) == (24, 2, 4.0, True)
    off, oinfo = _run(margin_model.transcribe, str(wav), max_line_width=0, **worker)
    assert off == today and all(s.words is None for s in off)
    assert oinfo.transcription_options == tinfo.transcription_options
    assert oinfo.transcription_options.max_line_width is None and not oinfo.transcription_options.word_timestamps
    monkeypatch.setenv(ENV[0], "wide")
    with pytest.raises(ValueError, match=ENV[0]):
        margin_model.transcribe(str(wav), **worker)
    with pytest.raises(ValueError, match="max_line_count"):
        margin_model.transcribe(str(wav), max_line_width=0, max_line_count=2, **worker)


def test_workers_collector_and_webvtt(margin_model, gap_clip):
    width = 24
    segments, info = margin_model.transcribe(gap_clip, language=None, task="transcribe", beam_size=5, vad_filter=True,
                                             max_line_width=width)
    cues, words = [], []
    for segment in segments:                    # the worker's loop: start, end, stripped text
        cues.append({"start": segment.start, "end": segment.end, "text": segment.text.strip()})
        words.append(segment.words)
    assert cues and info.language
    vtt = generate_webvtt(cues)
    blocks = vtt[len("WEBVTT\n\n"):].rstrip("\n").split("\n\n")
    assert len(blocks) == len(cues)
    for block, ws in zip(blocks, words):
        payload = block.split("\n")[2:]
        assert 1 <= len(payload) <= 2, block
        for line in payload:
            assert line and (len(line) <= width or line in [w.word.strip() for w in ws]), (line, block)
