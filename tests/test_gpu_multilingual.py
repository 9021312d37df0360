"""wm_generate_multilingual on the MI355X (transcribe(multilingual=True)): every window of a call is identified on
the device before its prefill and decoded under the language chosen for it, in every decode form.

Synthetic weights make real audio useless here: on the CPU with the bf16 oracle, speech_like, room tone, a sine,
noise and silence all detect one language (`sw` on tiny).  So the engine-level tests fill the cross-KV slots with
crafted encoder outputs through eng.cross_kv.  For window seed s:
    rng = np.random.default_rng(s)
    enc = scale * rng.standard_normal((1, 1, d)) + 0.1 * rng.standard_normal((1, 1500, d)),  rounded to bf16
The bf16-format oracle (computed on the CPU before any GPU run) gives, best language and gap to the runner-up in nats:
    tiny  scale 1.0  seeds 402, 404, 405, 407:  ca 0.2484, ca 0.1411, hu 0.4374, yi 0.3050
    base  scale 4.0  seeds 402, 403, 404, 407:  gl 0.3040, hy 0.2556, eu 0.2321, fa 0.3796
Three distinct languages per model, every gap above 2 EPS = 0.04 nats (EPS as in test_gpu_language_id.py), so no
window is skipped in the oracle comparison.  The placeholder in the auto calls' prompts is `en`, which no window
detects: a missing assignment fails the comparison with the plain call.

Public interface (synthetic:tiny:3): the 70 s clip speech_like(70.0, 11) has the windows of the 30 s grid with
without_timestamps=True; the oracle detects `sw` in all three, gaps 0.0822, 0.0828, 0.0742 nats to `ca`, and among the
candidates (de, ja) it puts `ja` 0.341, 0.341, 0.337 nats above `de`.  A limit of synthetic weights: every window of
the clip detects the file's own language, so in the public tests the placeholder already equals the chosen token and a
lost device assignment would not change their transcripts; the assignment itself is pinned by the engine-level tests
above (placeholder `en`) and the host's handling of differing languages by tests/test_multilingual_host.py.  What the
public tests add is that every form makes the multilingual call and carries its answer on (a spy on engine.generate).
"""
import numpy as np
import pytest
import torch

from oracle.decode import detect_language
from oracle.model import OracleWhisper
from vlog_amd.audio import speech_like
from vlog_amd.dims import model_dims
from vlog_amd.weights import round_bf16, synthetic_state_dict

pytestmark = pytest.mark.gpu

EPS = 0.02   # nats, the bf16 logit noise floor (tests/test_gpu_language_id.py)
W = 4
CASES = {"tiny": (1.0, (402, 404, 405, 407)), "base": (4.0, (402, 403, 404, 407))}
ML = 40      # total decoder length of the engine-level decodes (prompts of up to 12 tokens)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def crafted(seed, scale, d):
    rng = np.random.default_rng(seed)
    enc = scale * rng.standard_normal((1, 1, d)) + 0.1 * rng.standard_normal((1, 1500, d))
    return torch.from_numpy(enc.astype(np.float32)).to(torch.bfloat16)


@pytest.fixture(scope="module", params=["tiny", "base"])
def setup(request):
    from vlog_amd.engine import GpuEngine
    dims = model_dims(request.param)
    scale, seeds = CASES[request.param]
    sd = synthetic_state_dict(dims, seed=3, eot_after=60)
    eng = GpuEngine(dims, sd, 0)
    bf = OracleWhisper(round_bf16(sd), dims, np.float32, bf16_acts=True)      # the engine's numeric format
    enc = torch.cat([crafted(s, scale, dims.n_state) for s in seeds]).cuda()
    eng.reserve(W, 40)
    eng.cross_kv(enc, 0)
    st = dims.specials
    encf = enc.float().cpu().numpy()
    # computed once, shared, never modified
    oracle = [detect_language(bf, bf.cross_kv(encf[w: w + 1]), st) for w in range(W)]
    lid = eng.language_id(list(range(W)), st.lang_begin, st.n_langs)
    s = dict(dims=dims, eng=eng, st=st, oracle=oracle, lid=lid, en=st.lang_token("en"))
    s["sup"] = [st.transcribe, st.translate, st.sot, st.sot_prev, st.sot_lm]
    return s


def _la(s, positions, allowed=None):
    st = s["st"]
    return dict(lang_begin=st.lang_begin, n_langs=st.n_langs, allowed=allowed, positions=positions)


def _prompts(s, langs, prev=None):
    """[sot, language, transcribe] per window, behind <|startofprev|> + prev[w] tokens where given"""
    st = s["st"]
    out = []
    for w, lang in enumerate(langs):
        head = [st.sot_prev] + list(prev[w]) if prev and prev[w] else []
        out.append(head + [st.sot, int(lang), st.transcribe])
    return out


def _gen(s, prompts, slots=None, **kw):
    kw.setdefault("max_length", ML)
    return s["eng"].generate(list(range(W)) if slots is None else slots, prompts, suppress_tokens=s["sup"], **kw)


def _same(a, b):
    """two lists of GenResult, bit for bit"""
    assert len(a) == len(b)
    for w, (x, y) in enumerate(zip(a, b)):
        assert x.tokens == y.tokens and x.tokens, w
        assert _bits([x.score, x.cum_logprob, x.no_speech_prob]).tolist() == \
            _bits([y.score, y.cum_logprob, y.no_speech_prob]).tolist(), w
        assert (x.token_logprobs is None) == (y.token_logprobs is None)
        if x.token_logprobs is not None:
            assert np.array_equal(_bits(x.token_logprobs), _bits(y.token_logprobs)), w
            assert np.array_equal(_bits(x.token_logprobs_other), _bits(y.token_logprobs_other)), w


def test_detection_matches_the_oracle_and_language_id(setup):
    """h_lang is the oracle's best language per window, its probability within 5e-3 of the oracle's (the bound of
    test_gpu_language_id.py), and h_lang / h_lang_prob / h_probs carry the bits of language_id on the same slots in the
    same order."""
    s, st = setup, setup["st"]
    langs = []
    for w in range(W):
        want = s["oracle"][w]
        gap = np.log(want[0][1]) - np.log(want[1][1])
        print(f"d = {s['dims'].n_state} window {w}: oracle {want[0]} over {want[1]} gap {gap:.4f} nats")
        assert gap > 2 * EPS
        langs.append(want[0][0])
    assert len(set(langs)) >= 3 and "en" not in langs
    _, _, (top, top_prob, probs) = _gen(s, _prompts(s, [s["en"]] * W), language_auto=_la(s, [1] * W))
    for w in range(W):
        assert st.lang_codes[int(top[w])] == s["oracle"][w][0][0]
        assert abs(float(top_prob[w]) - s["oracle"][w][0][1]) < 5e-3
    assert np.array_equal(_bits(probs), _bits(s["lid"][0])) and np.array_equal(top, s["lid"][1])
    assert np.array_equal(_bits(top_prob), _bits(s["lid"][2]))
    # another order, a repeated slot: still language_id on that list of slots
    slots = [3, 1, 1, 0]
    _, _, (top, top_prob, probs) = _gen(s, _prompts(s, [s["en"]] * W), slots=slots, language_auto=_la(s, [1] * W))
    want = s["eng"].language_id(slots, st.lang_begin, st.n_langs)
    assert np.array_equal(_bits(probs), _bits(want[0])) and np.array_equal(top, want[1])
    assert np.array_equal(_bits(top_prob), _bits(want[2]))


FORMS = {
    "greedy": dict(record_logprobs=True),
    "beam5": dict(beam_size=5, record_logprobs=True),
    "sampling_best_of_3_seeds": dict(temperature=0.7, num_hypotheses=3, seeds=[11, 12, 13, 14], record_logprobs=True),
    "sampling_best_of_3": dict(temperature=0.7, num_hypotheses=3, seed=5),
    "rows2_greedy": dict(max_rows=2, record_logprobs=True),
    "rows2_sampled_seeds": dict(max_rows=2, temperature=0.7, seeds=[11, 12, 13, 14]),
    "rows_beam": dict(beam_size=5, max_rows=10),
    "compact_greedy": dict(compact=True, record_logprobs=True),
    "compact_beam": dict(beam_size=5, compact=True),
}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("ragged", [False, True], ids=["one_length", "ragged"])
def test_the_decode_is_the_plain_call(setup, form, ragged):
    """Tokens, scores, no-speech and the recorded log-probs of the auto call (placeholder `en` in every prompt) equal,
    bit for bit, generate with host prompts that hold the chosen tokens: same windows, order and options.  ragged:
    previous-text prefixes of 0, 3, 1 and 8 tokens, so the language position differs per window."""
    s, st = setup, setup["st"]
    prev = [[], [400, 401, 402], [500], list(range(600, 608))] if ragged else None
    chosen = [st.lang_begin + int(t) for t in s["lid"][1]]
    auto = _prompts(s, [s["en"]] * W, prev)
    pos = [p.index(st.sot) + 1 for p in auto]
    assert (len(set(pos)) > 1) == ragged
    kw = FORMS[form]
    stats_a, stats_p = {}, {}
    got, steps_a, (top, _, _) = _gen(s, auto, language_auto=_la(s, pos), stats=stats_a, **kw)
    want, steps_p = _gen(s, _prompts(s, chosen, prev), stats=stats_p, **kw)
    assert np.array_equal(top, s["lid"][1])
    _same(got, want)
    assert steps_a == steps_p and stats_a == stats_p
    if "max_rows" in kw:
        assert stats_a["refills"] > 0                   # windows did start at a refill
    # and the placeholder was replaced: the plain call under `en` decodes something else somewhere
    other, _ = _gen(s, auto, **kw)
    assert any(a.tokens != b.tokens or a.score != b.score for a, b in zip(got, other))


def test_mixed_windows(setup):
    """Windows 0 and 2 choose their language, windows 1 and 3 keep a pinned one: the pinned windows are the plain
    call's, bit for bit, with h_lang -1; the auto windows are those of the run where only they are in the call."""
    s, st = setup, setup["st"]
    pinned = st.lang_token("de")
    prompts = _prompts(s, [s["en"], pinned, s["en"], pinned])
    for kw in (dict(record_logprobs=True), dict(beam_size=5), dict(max_rows=2)):
        got, _, (top, top_prob, probs) = _gen(s, prompts, language_auto=_la(s, [1, -1, 1, -1]), **kw)
        assert top[1] == top[3] == -1 and top_prob[1] == top_prob[3] == 0.0 and not probs[[1, 3]].any()
        assert top[0] == s["lid"][1][0] and top[2] == s["lid"][1][2]
        assert np.array_equal(_bits(probs[[0, 2]]), _bits(s["lid"][0][[0, 2]]))
        chosen = [st.lang_begin + int(s["lid"][1][0]), pinned, st.lang_begin + int(s["lid"][1][2]), pinned]
        plain, _ = _gen(s, _prompts(s, chosen), **kw)
        _same(got, plain)
        # the run where only the auto windows are in the call chooses the same languages
        _, _, (top2, _, probs2) = _gen(s, [prompts[0], prompts[2]], slots=[0, 2], language_auto=_la(s, [1, 1]), **kw)
        assert np.array_equal(top2, top[[0, 2]]) and np.array_equal(_bits(probs2), _bits(probs[[0, 2]]))


def test_masks(setup):
    """A two-language mask with a window's runner-up but not its top: the choice is the masked language_id's; a
    single-language mask gives that language with probability exactly 1.0."""
    s, st = setup, setup["st"]
    n = st.n_langs
    order = np.argsort(-s["lid"][0][0], kind="stable")
    allowed = np.zeros(n, np.uint8)
    allowed[[int(order[1]), int(order[7])]] = 1          # window 0's runner-up and a lesser language; not its top
    auto = _prompts(s, [s["en"]] * W)
    got, _, (top, top_prob, probs) = _gen(s, auto, language_auto=_la(s, [1] * W, allowed))
    want = s["eng"].language_id(list(range(W)), st.lang_begin, n, allowed)
    assert np.array_equal(top, want[1]) and np.array_equal(_bits(top_prob), _bits(want[2]))
    assert np.array_equal(_bits(probs), _bits(want[0]))
    assert int(top[0]) == int(order[1]) and set(top.tolist()) <= {int(order[1]), int(order[7])}
    plain, _ = _gen(s, _prompts(s, [st.lang_begin + int(t) for t in top]))
    _same(got, plain)
    one = np.zeros(n, np.uint8)
    one[st.lang_codes.index("ja")] = 1
    got, _, (top, top_prob, probs) = _gen(s, auto, language_auto=_la(s, [1] * W, one))
    assert top.tolist() == [st.lang_codes.index("ja")] * W and np.all(top_prob == np.float32(1.0))
    plain, _ = _gen(s, _prompts(s, [st.lang_token("ja")] * W))
    _same(got, plain)


def test_null_language_argument_is_generate_seeded(setup):
    """wm_generate_multilingual(la = NULL) through the C ABI: the bits of wm_generate_seeded."""
    s, eng = setup, setup["eng"]
    prompts = _prompts(s, [setup["st"].lang_token("fr")] * W)
    kw = dict(temperature=0.7, num_hypotheses=2, seeds=[1, 2, 3, 4], record_logprobs=True)
    want, _ = _gen(s, prompts, **kw)
    real = eng.lib.wm_generate_seeded

    def through_null(h, a, seeds, stream):
        return eng.lib.wm_generate_multilingual(h, a, None, seeds, stream)

    class Lib:                                           # the engine's library with the seeded entry rerouted
        def __getattr__(self, name):
            return through_null if name == "wm_generate_seeded" else getattr(real_lib, name)

    real_lib = eng.lib
    eng.lib = Lib()
    try:
        got, _ = _gen(s, prompts, **kw)
    finally:
        eng.lib = real_lib
    assert real is real_lib.wm_generate_seeded
    _same(got, want)


def test_refusals_leave_the_engine_usable(setup):
    s, st = setup, setup["st"]
    good = _prompts(s, [s["en"]] * W)
    before, _ = _gen(s, good)
    with pytest.raises(RuntimeError, match=r"wm_generate_multilingual: window 2: language position 3 outside its prompt "
                                           r"of 3 tokens"):
        _gen(s, good, language_auto=_la(s, [1, 1, 3, 1]))
    with pytest.raises(RuntimeError, match=rf"wm_generate_multilingual: window 1: token {st.transcribe} at language "
                                           r"position 2 is not a language token"):
        _gen(s, good, language_auto=_la(s, [1, 2, 1, 1]))
    bad = [list(p) for p in good]
    bad[3] = [st.sot_prev, s["en"], st.transcribe]
    with pytest.raises(RuntimeError, match=r"wm_generate_multilingual: window 3: the token before language position 1 "
                                           r"is not <\|startoftranscript\|>"):
        _gen(s, bad, language_auto=_la(s, [1] * W))
    with pytest.raises(RuntimeError, match=r"wm_generate_multilingual: window 0: the token before language position 0"):
        _gen(s, [[s["en"], st.sot, st.transcribe]] * W, language_auto=_la(s, [0] * W))
    with pytest.raises(RuntimeError, match=r"wm_generate_multilingual: h_allowed sets no language"):
        _gen(s, good, language_auto=_la(s, [1] * W, np.zeros(st.n_langs, np.uint8)))
    with pytest.raises(RuntimeError, match=r"wm_generate_multilingual: n_langs outside 1\.\.128"):
        _gen(s, good, language_auto=dict(lang_begin=st.lang_begin, n_langs=0, allowed=None, positions=[1] * W))
    with pytest.raises(RuntimeError, match=r"wm_generate_multilingual: lang_begin \.\. lang_begin \+ n_langs outside"):
        _gen(s, good, language_auto=dict(lang_begin=s["dims"].n_vocab - 10, n_langs=st.n_langs, allowed=None,
                                         positions=[1] * W))
    after, _ = _gen(s, good)
    _same(after, before)
    got, _, (top, _, _) = _gen(s, good, language_auto=_la(s, [1] * W))
    assert np.array_equal(top, s["lid"][1])


# ------------------------------------------------------------------------------------------------ public interface
@pytest.fixture(scope="module")
def model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cuda", eot_after=60)


@pytest.fixture(scope="module")
def clip():
    return speech_like(70.0, 11)


CLIP = dict(without_timestamps=True, beam_size=1, temperature=0.0)


def _tokens(segs):
    return [s.tokens for s in segs]


def _window_language(timeline, seg):
    return next(w.language for w in timeline if w.start <= seg.start < w.end)


def test_transcribe_multilingual(model, clip, monkeypatch):
    monkeypatch.delenv("VLOG_AMD_MULTILINGUAL", raising=False)
    monkeypatch.delenv("VLOG_AMD_LANGUAGE_CANDIDATES", raising=False)
    timeline = model.language_timeline(clip)
    assert [(w.start, w.end) for w in timeline] == [(0.0, 30.0), (30.0, 60.0), (60.0, 70.0)]
    segs, info = model.transcribe(clip, multilingual=True, **CLIP)
    segs = list(segs)
    assert len(segs) == 3 and info.transcription_options.multilingual is True
    for s in segs:
        assert s.language == _window_language(timeline, s)
    # all windows agree (module docstring): the call with that language pinned decodes the same tokens
    langs = {w.language for w in timeline}
    assert len(langs) == 1
    pinned, pinfo = model.transcribe(clip, language=langs.pop(), multilingual=False, **CLIP)
    pinned = list(pinned)
    assert _tokens(pinned) == _tokens(segs) and all(s.language is None for s in pinned)
    assert pinfo.transcription_options.multilingual is False
    # info keeps its meaning: the file-level detection
    off, info_off = model.transcribe(clip, **CLIP)
    off = list(off)
    assert (info.language, info.language_probability, info.all_language_probs) == \
        (info_off.language, info_off.language_probability, info_off.all_language_probs)
    assert all(s.language is None for s in off) and info_off.transcription_options.multilingual is False
    false_, _ = model.transcribe(clip, multilingual=False, **CLIP)
    assert [s for s in false_] == off
    # a call that names its language asks for it in every window: the combination stays refused
    with pytest.raises(NotImplementedError, match="multilingual=True with language='en'"):
        model.transcribe(clip, language="en", multilingual=True, **CLIP)
    # the whitelist confines every window
    cands = ["de", "ja"]
    csegs, cinfo = model.transcribe(clip, multilingual=True, language_candidates=cands, **CLIP)
    csegs = list(csegs)
    ctl = model.language_timeline(clip, language_candidates=cands)
    assert csegs and all(s.language in cands and s.language == _window_language(ctl, s) for s in csegs)
    assert cinfo.language in cands and cinfo.transcription_options.language_candidates == tuple(cands)
    # the environment does what the argument does
    monkeypatch.setenv("VLOG_AMD_MULTILINGUAL", "1")
    esegs, einfo = model.transcribe(clip, **CLIP)
    assert [s for s in esegs] == segs and einfo.transcription_options.multilingual is True
    monkeypatch.setenv("VLOG_AMD_MULTILINGUAL", "yes")
    with pytest.raises(ValueError, match="VLOG_AMD_MULTILINGUAL must be 0 or 1"):
        model.transcribe(clip, **CLIP)


def test_the_other_decode_forms_carry_languages(model, clip, monkeypatch):
    from vlog_amd.transcribe import BatchedInferencePipeline
    monkeypatch.delenv("VLOG_AMD_MULTILINGUAL", raising=False)
    timeline = model.language_timeline(clip)
    ref, _ = model.transcribe(clip, multilingual=True, **CLIP)
    ref = list(ref)

    def check(segs):
        segs = list(segs)
        assert segs
        for s in segs:
            assert s.language == _window_language(timeline, s)
        return segs

    segs, info = model.transcribe(clip, multilingual=True, sections=2, **CLIP)     # (its windows leave the 30 s grid)
    segs = list(segs)
    assert segs and all(s.language in model.supported_languages for s in segs)
    assert info.transcription_options.multilingual is True and len(info.transcription_options.section_frames) == 2
    short = speech_like(20.0, 12)
    many = model.transcribe_many([clip, short], multilingual=True, **CLIP)
    check(many[0][0])
    assert many[1][0] and all(s.language is not None for s in many[1][0])
    lv = model.transcribe_many([clip, short], multilingual=True, lockstep_fallback=True, **CLIP)
    assert [s.language for s in lv[0][0]] == [s.language for s in ref]
    pipe = BatchedInferencePipeline(model, max_batch_windows=4)
    segs, info = pipe.transcribe(clip, multilingual=True, vad_filter=False, beam_size=1, temperature=0.0)
    check(segs)
    assert info.transcription_options.multilingual is True
    out = pipe.transcribe_many([clip, short], multilingual=True, vad_filter=False, beam_size=1, temperature=0.0)
    check(out[0][0])
    assert out[1][0] and all(s.language is not None for s in out[1][0])
    segs, _ = pipe.transcribe(clip, vad_filter=False, beam_size=1, temperature=0.0)
    assert all(s.language is None for s in segs)
    # word timestamps: aligned under each window's language, words present
    for segs in (model.transcribe(clip, multilingual=True, word_timestamps=True, beam_size=1, temperature=0.0)[0],
                 pipe.transcribe(clip, multilingual=True, word_timestamps=True, vad_filter=False, beam_size=1,
                                 temperature=0.0)[0]):
        segs = list(segs)
        assert segs and all(s.language is not None and s.words is not None for s in segs)
        assert any(s.words for s in segs)
    # a lockstep round aligns by language: both files' windows detect `sw`, so a round of two items is ONE align call
    # over two slots (the last round holds the long file alone)
    aligns = []
    inner_align = model.engine.align_batch

    def align_spy(slots, sot, *a, **kw):
        aligns.append((list(slots), list(sot)))
        return inner_align(slots, sot, *a, **kw)

    monkeypatch.setattr(model.engine, "align_batch", align_spy)
    many = model.transcribe_many([clip, short], multilingual=True, word_timestamps=True, beam_size=1, temperature=0.0)
    monkeypatch.setattr(model.engine, "align_batch", inner_align)
    assert all(segs and all(s.language == "sw" and s.words is not None for s in segs) for segs, _ in many)
    assert aligns and aligns[0][0] == [0, 1] and all(len(sl) <= 2 for sl, _ in aligns)
    sw = model.tokenizer(task="transcribe", language="sw").sot_sequence
    assert all(sot == sw for _, sot in aligns)
    # the fallback temperatures decode under the window's language too (every temperature fails this threshold):
    # the first decode of each window is the multilingual call, the fallback's prompt carries the returned token
    st = model.dims.specials
    calls = []
    inner = model.engine.generate

    def spy(slots, prompts, **kw):
        out = inner(slots, prompts, **kw)
        calls.append((kw.get("temperature", 0.0), [list(p) for p in prompts], kw.get("language_auto"),
                      out[2][0].tolist() if len(out) > 2 else None))
        return out

    monkeypatch.setattr(model.engine, "generate", spy)
    segs, _ = model.transcribe(clip, multilingual=True, without_timestamps=True, beam_size=1, best_of=2,
                               temperature=(0.0, 0.4), log_prob_threshold=0.0, no_speech_threshold=None)
    segs = list(segs)
    monkeypatch.setattr(model.engine, "generate", inner)
    assert segs and {s.temperature for s in segs} == {0.4}
    for s in segs:
        assert s.language == _window_language(timeline, s)
    assert [c[0] for c in calls] == [0.0, 0.4] * 3
    for first, fallback in zip(calls[0::2], calls[1::2]):
        pos = first[2]["positions"][0]
        assert first[1][0][pos - 1] == st.sot and first[3] is not None and fallback[2] is None
        assert fallback[1][0][pos] == st.lang_begin + first[3][0]
        assert fallback[1][0][:pos] == first[1][0][:pos] and fallback[1][0][pos + 1:] == first[1][0][pos + 1:]
    # caption shaping copies the language to the cues
    cues, _ = model.transcribe(clip, multilingual=True, max_line_width=20, beam_size=1, temperature=0.0)
    cues = list(cues)
    assert len(cues) >= 3 and all(c.language is not None for c in cues)
