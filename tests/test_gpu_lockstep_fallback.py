"""lockstep_fallback=True: the fallback temperatures of a lockstep round (transcribe_many, transcribe(sections=N))
decoded by LEVELS, the windows that fail temperature i together in one seeded engine.generate at temperature i + 1.

Margin model (synthetic:tiny:0:margin): its avg_logprob is exactly 0.0, so with log_prob_threshold=0.5 every level
fails and the whole ladder is walked; its sampled tokens at T = 0.4 and 1.0 equal its beam-5 tokens (the Gumbel draws
lie in [-2.81, 16.64], the planted margins are thousands of nats), so the level form must give every file exactly what
the one-file call gives, whichever rows share its passes.  engine.generate is wrapped to record its calls: with the
flag one call per level holding all windows of the round, seeds [window + level]; without it every call at T > 0 has
one window and no seeds.

Random model (synthetic:tiny:3): every window falls back to 0.4 (tests/test_gpu_transcribe_many_seq.py test_c); the
level form is compared with itself (two calls, the environment variable), not with the solo decode, whose sampled
near-ties may flip when other windows' rows share the passes."""
import pytest

from vlog_amd.audio import speech_like

from tests.test_gpu_transcribe_many_seq import _same

pytestmark = pytest.mark.gpu

TEMPS = (0.0, 0.4, 0.8)
MARGIN_KW = dict(language="en", beam_size=5, temperature=TEMPS, log_prob_threshold=0.5, no_speech_threshold=None)


@pytest.fixture(scope="module")
def margin_model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:0:margin", device="cuda")


@pytest.fixture(scope="module")
def model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cuda", eot_after=60)


@pytest.fixture(scope="module")
def files():
    return [speech_like(45.0, 1400), speech_like(21.0, 1401), speech_like(33.0, 1402)]


@pytest.fixture(scope="module")
def x75():
    return speech_like(75.0, 1410)


@pytest.fixture(scope="module")
def solo_refs(margin_model, files):
    """the one-file call per file (the reference; left unchanged)"""
    return [list(margin_model.transcribe(x, **MARGIN_KW)[0]) for x in files]


def _record(model):
    """wraps engine.generate -> (calls: one dict(slots, temperature, seeds, num_hypotheses) per call, undo)"""
    eng = model.engine
    inner = eng.generate
    calls = []

    def recorded(slots, *a, **kw):
        calls.append(dict(slots=list(slots), temperature=kw.get("temperature", 0.0), seeds=kw.get("seeds"),
                          num_hypotheses=kw.get("num_hypotheses", 1)))
        return inner(slots, *a, **kw)

    eng.generate = recorded

    def undo():
        del eng.generate                                    # (the instance attribute: the class's method is back)

    return calls, undo


def _check_level_calls(calls, temps, best_of=5):
    """the calls of a run by levels: per round one call per temperature, all over the round's windows (slots 0..nb-1),
    the sampled ones seeded with [window + level]; in these runs every item of round r is at its window r"""
    assert calls and len(calls) % len(temps) == 0, len(calls)
    sizes = []
    for r in range(len(calls) // len(temps)):
        rnd = calls[r * len(temps): (r + 1) * len(temps)]
        nb = len(rnd[0]["slots"])
        sizes.append(nb)
        for level, (c, t) in enumerate(zip(rnd, temps)):
            assert c["temperature"] == t and c["slots"] == list(range(nb)), (r, level, c)
            if t > 0:
                assert c["seeds"] == [r + level] * nb and c["num_hypotheses"] == best_of, (r, level, c)
            else:
                assert c["seeds"] is None, (r, level, c)
    return sizes


def test_margin_many_by_levels_equals_one_file_calls(margin_model, files, solo_refs):
    assert all(s.temperature == TEMPS[-1] for r in solo_refs for s in r) and all(solo_refs)   # the whole ladder was walked
    calls, undo = _record(margin_model)
    try:
        many = margin_model.transcribe_many(files, lockstep_fallback=True, max_files=3, **MARGIN_KW)
    finally:
        undo()
    for (segs, info), ref in zip(many, solo_refs):
        _same(segs, ref)
        assert info.transcription_options.lockstep_fallback is True
    sizes = _check_level_calls(calls, TEMPS)
    assert sizes[0] == 3 and len(sizes) >= 2 and sizes[1] >= 2, sizes        # rounds that share their levels


def test_margin_many_flag_off_decodes_fallbacks_alone(margin_model, files, solo_refs):
    for kw in (dict(), dict(lockstep_fallback=False)):
        calls, undo = _record(margin_model)
        try:
            many = margin_model.transcribe_many(files, max_files=3, **kw, **MARGIN_KW)
        finally:
            undo()
        for (segs, info), ref in zip(many, solo_refs):
            _same(segs, ref)
            assert info.transcription_options.lockstep_fallback is False
        sampled = [c for c in calls if c["temperature"] > 0]
        assert sampled and all(len(c["slots"]) == 1 and c["seeds"] is None for c in sampled), sampled
        assert max(len(c["slots"]) for c in calls if c["temperature"] == 0) == 3


def test_margin_sections_by_levels(margin_model, x75):
    ref, rinfo = margin_model.transcribe(x75, sections=2, **MARGIN_KW)
    ref = list(ref)
    assert len(rinfo.transcription_options.section_frames) == 2 and ref
    calls, undo = _record(margin_model)
    try:
        segs, info = margin_model.transcribe(x75, sections=2, lockstep_fallback=True, **MARGIN_KW)
        segs = list(segs)
    finally:
        undo()
    _same(segs, ref)
    assert info.transcription_options.lockstep_fallback is True and not rinfo.transcription_options.lockstep_fallback
    assert all(s.temperature == TEMPS[-1] for s in segs)
    sizes = _check_level_calls(calls, TEMPS)
    assert sizes[0] == 2, sizes
    # one window per round has nothing to share: the flag changes no call of the one-file loop
    calls, undo = _record(margin_model)
    try:
        one = list(margin_model.transcribe(x75, lockstep_fallback=True, **MARGIN_KW)[0])
    finally:
        undo()
    assert one and all(len(c["slots"]) == 1 and c["seeds"] is None for c in calls)


def test_margin_sampled_first_pass(margin_model, files):
    kw = dict(language="en", beam_size=5, best_of=3, temperature=(0.4,), log_prob_threshold=0.5, no_speech_threshold=None)
    refs = [list(margin_model.transcribe(x, **kw)[0]) for x in files]
    calls, undo = _record(margin_model)
    try:
        many = margin_model.transcribe_many(files, lockstep_fallback=True, max_files=3, **kw)
    finally:
        undo()
    for (segs, _), ref in zip(many, refs):
        _same(segs, ref)
    sizes = _check_level_calls(calls, (0.4,), best_of=3)     # one call per round, seeds [window]
    assert sizes[0] == 3, sizes


def _plain(segs):
    return [(s.id, s.seek, s.tokens, s.temperature, s.start, s.end, s.avg_logprob, s.no_speech_prob) for s in segs]


def test_random_model_sections_by_levels(model, x75, monkeypatch):
    kw = dict(language="en", beam_size=5, temperature=(0.0, 0.4), sections=2)
    monkeypatch.delenv("VLOG_AMD_LOCKSTEP_FALLBACK", raising=False)
    a, info = model.transcribe(x75, lockstep_fallback=True, **kw)
    a = list(a)
    assert a and {s.temperature for s in a} == {0.4}
    assert info.transcription_options.lockstep_fallback is True
    b = list(model.transcribe(x75, lockstep_fallback=True, **kw)[0])
    assert _plain(a) == _plain(b)
    off = model.transcribe(x75, **kw)[1]
    assert off.transcription_options.lockstep_fallback is False
    monkeypatch.setenv("VLOG_AMD_LOCKSTEP_FALLBACK", "1")
    calls, undo = _record(model)
    try:
        c, cinfo = model.transcribe(x75, **kw)
        c = list(c)
    finally:
        undo()
    assert _plain(a) == _plain(c)
    assert cinfo.transcription_options.lockstep_fallback is True
    _check_level_calls(calls, (0.0, 0.4))
    # the argument wins over the environment
    monkeypatch.setenv("VLOG_AMD_LOCKSTEP_FALLBACK", "1")
    assert model.transcribe(x75, lockstep_fallback=False, **kw)[1].transcription_options.lockstep_fallback is False
