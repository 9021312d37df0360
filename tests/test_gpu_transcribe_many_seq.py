"""WhisperModel.transcribe_many in the sequential (parity) mode: several files decoded in lockstep, each round one
ragged engine.generate over the next window of every file in flight.  Each file must get exactly what
`transcribe(file, same arguments)` gives for it alone: segment tokens, seek, start, end, temperature and id, avg_logprob
and no_speech_prob to 1e-3, info.language and info.duration.

Files: 75 s (three windows), 21 s, 48 s with a 4 s zero gap, 30 s of room tone, 33 s; max_files 2 (files take over
finished files' places, so a file's first window shares a pass with another's later window: prompts of 3 and of dozens
of tokens) and 5 (all in flight).

Near-ties (as tests/test_gpu_multi.py): on the random-weight model a file's rows share decoder passes with other
files' rows, so the GEMM routes follow another row count and results agree to f32 rounding, not bit for bit; a
top-2 tie below that level could flip a token.  The comparisons are exact all the same.  One seed set met such a tie:
with 1300 as the 75 s file's seed, case b at max_files=5 chose ' hea' (31893) where the one-file call chose ' boudol'
(28171) as the only text token of that file's last segment: the second of the 15 tokens of that window's best beam
hypothesis.  The CPU oracle, teacher-forced on the window's encoder output with the window's prompt and rules, gives
the two 15-token hypotheses cumulative log-probs of -106.24857 (the one-file call's) and -106.24682 (the lockstep
call's): 0.0018 nats apart, an order below the 0.02-nat bf16 noise floor of DESIGN.md §4, and in favour of the
lockstep call's choice (the GPU's own normalised scores: -7.082761 and -7.082679).  Case b therefore uses seed 1320
for that file."""
import numpy as np
import pytest

from vlog_amd.audio import room_tone, speech_like

pytestmark = pytest.mark.gpu

MAX_FILES = (2, 5)


def _files(seed0=1300):
    gap = np.zeros(16000 * 4, np.float32)
    return [speech_like(75.0, seed0),
            speech_like(21.0, 1301),
            np.concatenate([speech_like(24.0, 1302), gap, speech_like(20.0, 1303)]),
            room_tone(30.0, 1304).astype(np.float32),
            speech_like(33.0, 1305)]


@pytest.fixture(scope="module")
def files():
    return _files()


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


def _check(model, files, per_file_kw=None, words=False, **kw):
    """transcribe_many at both max_files against transcribe per file; -> the per-file references"""
    n = len(files)
    per_file_kw = per_file_kw or {}
    refs = []
    for i, x in enumerate(files):
        segs, info = model.transcribe(x, **kw, **{k: v[i] for k, v in per_file_kw.items()})
        refs.append((list(segs), info))
    for mf in MAX_FILES:
        many = model.transcribe_many(files, max_files=mf, **kw, **per_file_kw)
        assert len(many) == n
        for i, ((segs, info), (rsegs, rinfo)) in enumerate(zip(many, refs)):
            assert info.language == rinfo.language and info.duration == rinfo.duration, (mf, i)
            assert info.duration_after_vad == rinfo.duration_after_vad, (mf, i)
            try:
                _same(segs, rsegs, words)
            except AssertionError as e:
                raise AssertionError(f"max_files={mf} file {i}: {e}") from e
    return refs


def test_a_greedy_first_pass_is_final(model, files):
    refs = _check(model, files, language="en", beam_size=1, temperature=0.0)
    assert len({s.seek for s in refs[0][0]}) >= 2            # the 75 s file's later windows carry previous text
    assert sum(len(r[0]) for r in refs) > 8
    # later windows ran with a previous-text prompt: the ragged pass is what is being compared
    assert all(s.temperature == 0.0 for r in refs for s in r[0])


def test_b_beam5_vad(model):
    refs = _check(model, _files(1320), language="en", beam_size=5, temperature=0.0, vad_filter=True)
    assert sum(len(r[0]) for r in refs) > 8


def test_c_every_window_falls_back(model, files):
    """random weights fail the log-prob threshold (tools/bench_worker_call.py): every window is re-decoded alone at
    0.4 with seed window + 1 against its own slot"""
    refs = _check(model, files, language="en", beam_size=5, temperature=(0.0, 0.4))
    temps = {s.temperature for r in refs for s in r[0]}
    assert temps == {0.4}, temps


def test_d_workers_call_on_margin_model(margin_model, files):
    refs = _check(margin_model, files, language=None, task="transcribe", beam_size=5, vad_filter=True)
    segs = [s for r in refs for s in r[0]]
    assert segs and not [s for s in segs if s.temperature > 0]


def test_e_word_timestamps(model, files):
    refs = _check(model, files, words=True, language="en", beam_size=1, temperature=0.0, word_timestamps=True)
    assert any(s.words for r in refs for s in r[0])


def test_f_per_file_initial_prompt_and_prefix(model, files):
    three = files[:3]
    refs = _check(model, three, per_file_kw=dict(initial_prompt=["hello world", None, "another start"],
                                                 prefix=[None, "so then", None]),
                  language="en", beam_size=1, temperature=0.0)
    plain = [list(model.transcribe(x, language="en", beam_size=1, temperature=0.0)[0]) for x in three]
    assert [s.tokens for s in refs[0][0]] != [s.tokens for s in plain[0]]       # the prompts did something
    assert [s.tokens for s in refs[1][0]] != [s.tokens for s in plain[1]]


def test_g_without_previous_text(model, files):
    _check(model, files, language="en", beam_size=1, temperature=0.0, condition_on_previous_text=False)


def test_h_sampled_first_pass(model, files):
    """temperature[0] > 0: the first pass is sampled, so every window decodes alone against its slot, with the seed
    (window) and best_of of the one-file call"""
    refs = _check(model, files, language="en", beam_size=5, best_of=3, temperature=(0.4,))
    assert {s.temperature for r in refs for s in r[0]} == {0.4}


def test_refused_options_and_argument_checks(model, files):
    with pytest.raises(NotImplementedError):
        model.transcribe_many(files[:2], language="en", multilingual=True)
    with pytest.raises(NotImplementedError):
        model.transcribe_many(files[:2], language="en", hallucination_silence_threshold=2.0)
    with pytest.raises(ValueError):
        model.transcribe_many(files[:2], language=["en"])
    assert model.transcribe_many([], language="en") == []
