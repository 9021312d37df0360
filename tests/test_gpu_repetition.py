"""repetition_penalty / no_repeat_ngram_size on the MI355X (logits_select_kernel's RULES instantiations) in every
decode form of wm_generate, and the transcribe arguments they (and prefix / hotwords) open.

The no-repeat invariant is exact whatever the bf16 near-ties.  The penalty is checked teacher-forced: the GPU's own
tokens go through the CPU oracle once, the reference rules (tests/repetition_ref.py, pinned against transformers)
come first, then oracle.decode.apply_rules and log-softmax; no test asks for token equality with an oracle decode
(per-step top-2 margins of this model are often below the EPS noise floor)."""
import numpy as np
import pytest
import torch

from oracle import mel as omel
from oracle.model import OracleWhisper
from tests.repetition_ref import repeated_ngrams, teacher_forced_logprobs
from vlog_amd.audio import speech_like
from vlog_amd.dims import model_dims
from vlog_amd.weights import round_bf16, synthetic_state_dict

pytestmark = pytest.mark.gpu

EPS = 0.02        # nats, the bf16 logit noise floor
ML = 100


def _sup(st):
    return [st.transcribe, st.translate, st.sot, st.sot_prev, st.sot_lm]


@pytest.fixture(scope="module")
def setup():
    from vlog_amd.engine import GpuEngine
    dims = model_dims("tiny")
    sd = synthetic_state_dict(dims, seed=3, eot_after=60)
    eng = GpuEngine(dims, sd, 0)
    orc = OracleWhisper(round_bf16(sd), dims, np.float32)
    W = 4
    x = np.concatenate([speech_like(30.0, 200 + i) for i in range(W)])
    feats = omel.log_mel(x, dims.n_mels)
    enc = eng.encode(torch.from_numpy(feats).cuda(), [3000 * i for i in range(W)], [3000] * W)
    eng.reserve(W, 40)
    eng.cross_kv(enc, 0)
    st = dims.specials
    prompt = [st.sot, st.lang_token("en"), st.transcribe]

    def gen(**kw):
        return eng.generate(list(range(W)), [prompt] * W, suppress_tokens=_sup(st), max_length=ML, **kw)[0]

    return dict(dims=dims, eng=eng, orc=orc, encf=enc.float().cpu().numpy(), W=W, st=st, prompt=prompt, gen=gen)


def _oracle(s, w, r, penalty=1.0, ngram=0):
    """teacher-forced (chosen, best) log-probs of window w's result under the reference rules"""
    cross = s["orc"].cross_kv(s["encf"][w: w + 1])
    ended = len(s["prompt"]) + len(r.tokens) < ML
    return teacher_forced_logprobs(s["orc"], cross, s["prompt"], r.tokens, s["st"], _sup(s["st"]), ended, penalty, ngram)


def test_ngram_invariant_greedy(setup):
    plain = setup["gen"]()
    assert any(repeated_ngrams(r.tokens, 3) for r in plain)       # the ban below has something to do
    for n in (1, 2, 3):
        res = setup["gen"](no_repeat_ngram_size=n)
        for w, r in enumerate(res):
            assert r.tokens and not repeated_ngrams(r.tokens, n), (n, w, r.tokens)
        assert [r.tokens for r in res] != [r.tokens for r in plain]


def test_penalty_greedy_teacher_forced(setup):
    res = setup["gen"](repetition_penalty=1.3, record_logprobs=True)
    reused, ok_unpenalised = 0, True
    for w, r in enumerate(res):
        chosen, best = _oracle(setup, w, r, penalty=1.3)
        print(f"window {w}: {len(r.tokens)} tokens, min(chosen - best) {np.min(chosen - best):.4f}, "
              f"max |record - oracle| {np.max(np.abs(r.token_logprobs - chosen)):.4f}")
        assert np.all(chosen >= best - EPS), (w, chosen - best)
        assert r.token_logprobs.shape == chosen.shape
        assert np.all(np.abs(r.token_logprobs - chosen) <= EPS), (w, r.token_logprobs - chosen)
        # a chosen token that was already in the history: its log-prob comes from the PENALISED logit
        reused += sum(t in r.tokens[:i] for i, t in enumerate(r.tokens))
        c1, b1 = _oracle(setup, w, r, penalty=1.0)
        ok_unpenalised = ok_unpenalised and bool(np.all(c1 >= b1 - EPS))
    assert reused >= 1
    assert not ok_unpenalised                                     # without the penalty this output is not EPS-greedy


@pytest.mark.parametrize("rules", [dict(no_repeat_ngram_size=3), dict(repetition_penalty=1.3)], ids=["ngram3", "pen1.3"])
def test_beam_with_rules(setup, rules):
    res = setup["gen"](beam_size=5, patience=1.0, **rules)
    for w, r in enumerate(res):
        if "no_repeat_ngram_size" in rules:
            assert not repeated_ngrams(r.tokens, 3), (w, r.tokens)
        chosen, _ = _oracle(setup, w, r, rules.get("repetition_penalty", 1.0), rules.get("no_repeat_ngram_size", 0))
        assert np.all(np.isfinite(chosen))                        # every token legal under rules + reference
        score = float(np.sum(chosen)) / max(len(r.tokens), 1)
        print(f"window {w}: score {r.score:.4f} oracle {score:.4f}")
        assert abs(score - r.score) < 2e-2 * max(1.0, abs(score)), (w, score, r.score)


def test_sampling_with_ngram_ban(setup):
    kw = dict(temperature=1.0, num_hypotheses=3, seed=7, no_repeat_ngram_size=2)
    a, b = setup["gen"](**kw), setup["gen"](**kw)
    for ra, rb in zip(a, b):
        assert ra.tokens and not repeated_ngrams(ra.tokens, 2), ra.tokens
        assert ra.tokens == rb.tokens and ra.score == rb.score    # seeded -> reproducible


@pytest.mark.parametrize("beam", [1, 5])
def test_row_set_decode_with_ngram_ban(setup, beam):
    """Two windows in flight over the four (beam search counts rows: two groups of beam_size), so two slots are
    refilled: a refilled slot's history restarts with its new window."""
    stats = {}
    res = setup["gen"](beam_size=beam, max_rows=2 * beam, compact=True, no_repeat_ngram_size=2, stats=stats)
    assert stats["refills"] >= 1
    for w, r in enumerate(res):
        assert r.tokens and not repeated_ngrams(r.tokens, 2), (w, r.tokens)


@pytest.mark.parametrize("beam", [1, 5])
def test_defaults_are_inert(setup, beam):
    a = setup["gen"](beam_size=beam)
    b = setup["gen"](beam_size=beam, repetition_penalty=1.0, no_repeat_ngram_size=0)
    assert [r.tokens for r in a] == [r.tokens for r in b]
    assert [(r.score, r.cum_logprob) for r in a] == [(r.score, r.cum_logprob) for r in b]


def test_invalid_values_raise(setup):
    with pytest.raises(RuntimeError, match="repetition_penalty"):
        setup["gen"](repetition_penalty=-1)
    with pytest.raises(RuntimeError, match="no_repeat_ngram_size"):
        setup["gen"](no_repeat_ngram_size=-2)
    with pytest.raises(RuntimeError, match="no_repeat_ngram_size"):
        setup["gen"](no_repeat_ngram_size=ML + 1)
    assert setup["gen"]()[0].tokens                               # the engine is usable afterwards


# ---- public surface
@pytest.fixture(scope="module")
def model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cuda", eot_after=60)


@pytest.fixture(scope="module")
def clip():
    return speech_like(20.0, 410)                                 # one window


def _tokens(segments):
    return [t for s in segments for t in s.tokens]


def _window_tokens(segments):
    """concatenated tokens per decoded window (the rule's history is one window's generated tokens; the seek loop
    may decode the clip's tail as a window of its own)"""
    by_seek = {}
    for s in segments:
        by_seek.setdefault(s.seek, []).extend(s.tokens)
    return list(by_seek.values())


def test_transcribe_no_repeat_ngram(model, clip):
    from vlog_amd.transcribe import BatchedInferencePipeline
    kw = dict(language="en", beam_size=1, temperature=0, no_repeat_ngram_size=2)
    segs, info = model.transcribe(clip, condition_on_previous_text=False, **kw)
    wins = _window_tokens(segs)
    assert wins and all(toks and not repeated_ngrams(toks, 2) for toks in wins), wins
    assert info.transcription_options.no_repeat_ngram_size == 2
    segs, info = BatchedInferencePipeline(model).transcribe(clip, vad_filter=False, **kw)
    wins = _window_tokens(segs)
    assert len(wins) == 1 and wins[0] and not repeated_ngrams(wins[0], 2), wins
    assert info.transcription_options.no_repeat_ngram_size == 2


def test_transcribe_prefix_hotwords_and_refusals(model, clip):
    from vlog_amd.transcribe import BatchedInferencePipeline
    segs, info = model.transcribe(clip, language="en", beam_size=1, temperature=0, prefix="hello", hotwords="foo bar")
    list(segs)
    assert info.transcription_options.prefix == "hello" and info.transcription_options.hotwords == "foo bar"
    segs, info = model.transcribe(clip, language="en", beam_size=1, temperature=0, repetition_penalty=1.3,
                                  hotwords="foo bar")
    assert _tokens(segs) and info.transcription_options.repetition_penalty == 1.3
    with pytest.raises(NotImplementedError):
        model.transcribe(clip, language="en", multilingual=True)
    with pytest.raises(NotImplementedError):
        model.transcribe(clip, language="en", hallucination_silence_threshold=2.0)
    pipe = BatchedInferencePipeline(model)
    segs, info = pipe.transcribe(clip, language="en", beam_size=1, temperature=0, vad_filter=False, hotwords="foo bar")
    assert _tokens(segs) and info.transcription_options.hotwords == "foo bar"
    with pytest.raises(NotImplementedError, match="prefix in throughput mode"):
        pipe.transcribe(clip, language="en", prefix="hello")
    with pytest.raises(NotImplementedError):
        pipe.transcribe(clip, language="en", multilingual=True)
