"""The sequence bias on the MI355X (logits_select_kernel's BIAS instantiations, wm_set_sequence_bias) in every decode
form of wm_generate, and the `sequence_bias` argument of the transcribe calls.

A ban (-100) is an exact invariant whatever the bf16 near-ties.  A boost is checked teacher-forced, as the repetition
penalty is (tests/test_gpu_repetition.py): the GPU's own tokens go through the CPU oracle once, the reference rules
(tests/sequence_bias_ref.py, pinned against transformers) come first, then oracle.decode.apply_rules and log-softmax;
no test asks for token equality with an oracle decode."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest
import torch

from oracle import mel as omel
from oracle.decode import apply_rules, log_softmax
from oracle.model import OracleWhisper
from tests.repetition_ref import apply_history_rules
from tests.sequence_bias_ref import apply_sequence_bias, completions, teacher_forced_logprobs
from vlog_amd.audio import speech_like
from vlog_amd.dims import model_dims
from vlog_amd.weights import round_bf16, synthetic_state_dict

pytestmark = pytest.mark.gpu

EPS = 0.02        # nats, the bf16 logit noise floor
ML = 100
BAN = -100.0
BOOST = 30.0


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

    def gen(prompts=None, **kw):
        return eng.generate(list(range(W)), prompts or [prompt] * W, suppress_tokens=_sup(st), max_length=ML, **kw)[0]

    s = dict(dims=dims, eng=eng, orc=orc, encf=enc.float().cpu().numpy(), W=W, st=st, prompt=prompt, gen=gen)
    # the plain greedy output and what the tables below are made of, computed once
    s["plain"] = plain = gen()
    text = Counter(t for r in plain for t in r.tokens if t < st.eot and t != st.blank)
    s["ban_ids"] = [t for t, _ in text.most_common(3)]
    s["a"] = a = text.most_common(1)[0][0]
    used = {t for r in plain for t in r.tokens}
    s["c"] = next(t for t in range(1000, st.eot) if t not in used and t != st.blank)       # an unsuppressed text id
    s["bigram"] = next((p, q) for r in plain for p, q in zip(r.tokens, r.tokens[1:]) if p < st.eot and q < st.eot)
    assert a != s["c"] and len(s["ban_ids"]) == 3
    return s


def _oracle(s, w, r, table=(), penalty=1.0, prompt=None, with_timestamps=True):
    """teacher-forced (chosen, best) log-probs of window w's result under the reference rules"""
    prompt = prompt or s["prompt"]
    cross = s["orc"].cross_kv(s["encf"][w: w + 1])
    ended = len(prompt) + len(r.tokens) < ML
    return teacher_forced_logprobs(s["orc"], cross, prompt, r.tokens, s["st"], _sup(s["st"]), ended, table, penalty,
                                   with_timestamps=with_timestamps)


def _ban_table(s):
    return [((t,), BAN) for t in s["ban_ids"]] + [(s["bigram"], BAN)]


def _ban_holds(s, tokens):
    return not (set(tokens) & set(s["ban_ids"])) and completions(tokens, s["bigram"]) == 0


def test_ban_single_ids_greedy(setup):
    res = setup["gen"](sequence_bias=[((t,), BAN) for t in setup["ban_ids"]])
    for w, r in enumerate(res):
        assert r.tokens and not set(r.tokens) & set(setup["ban_ids"]), (w, r.tokens)
    assert [r.tokens for r in res] != [r.tokens for r in setup["plain"]]


def test_ban_bigram_greedy(setup):
    p, q = setup["bigram"]
    assert any(completions(r.tokens, (p, q)) for r in setup["plain"])         # the ban below has something to do
    res = setup["gen"](sequence_bias=[((p, q), BAN)])
    for w, r in enumerate(res):
        assert r.tokens and completions(r.tokens, (p, q)) == 0, (w, r.tokens)
    assert [r.tokens for r in res] != [r.tokens for r in setup["plain"]]
    # an entry whose prefix never matches (c is in no plain output) changes nothing
    res = setup["gen"](sequence_bias=[((setup["c"], q), BAN)])
    assert [r.tokens for r in res] == [r.tokens for r in setup["plain"]]


def test_boost_greedy_teacher_forced(setup):
    a, c = setup["a"], setup["c"]
    table = [((a, c), BOOST)]
    res = setup["gen"](sequence_bias=table, record_logprobs=True)
    adjacent, ok_unbiased = 0, True
    for w, r in enumerate(res):
        chosen, best = _oracle(setup, w, r, table)
        print(f"window {w}: {len(r.tokens)} tokens, min(chosen - best) {np.min(chosen - best):.4f}, "
              f"max |record - oracle| {np.max(np.abs(r.token_logprobs - chosen)):.4f}")
        assert np.all(chosen >= best - EPS), (w, chosen - best)
        assert r.token_logprobs.shape == chosen.shape
        assert np.all(np.abs(r.token_logprobs - chosen) <= EPS), (w, r.token_logprobs - chosen)
        adjacent += completions(r.tokens, (a, c))
        c0, b0 = _oracle(setup, w, r)
        ok_unbiased = ok_unbiased and bool(np.all(c0 >= b0 - EPS))
    assert adjacent >= 1                          # the boosted pair now exists (c is in no plain output)
    assert not ok_unbiased                        # without the bias this output is not EPS-greedy


def test_entries_ending_in_one_id_add_up(setup):
    a, c = setup["a"], setup["c"]
    table = [((a, c), 20.0), ((c,), -5.0), ((a, c), 15.0)]         # after a: +30 on c; elsewhere: -5
    res = setup["gen"](sequence_bias=table, record_logprobs=True)
    again = setup["gen"](sequence_bias=table, record_logprobs=True)
    adjacent = 0
    for w, (r, r2) in enumerate(zip(res, again)):
        chosen, best = _oracle(setup, w, r, table)
        print(f"window {w}: max |record - oracle| {np.max(np.abs(r.token_logprobs - chosen)):.4f}")
        assert np.all(chosen >= best - EPS), (w, chosen - best)
        assert np.all(np.abs(r.token_logprobs - chosen) <= EPS), (w, r.token_logprobs - chosen)
        adjacent += completions(r.tokens, (a, c))
        assert r.tokens == r2.tokens and r.score == r2.score and r.cum_logprob == r2.cum_logprob
        assert np.array_equal(r.token_logprobs, r2.token_logprobs)             # bit for bit
    assert adjacent >= 1


def test_composition_with_repetition_penalty(setup):
    """Penalty first, then the bias.  Length-1 entries on the ids the plain output uses most: they are in the history
    (so penalised) and carry real probability mass (so the normaliser feels their logits).  The same records miss
    the bound under the other order."""
    table = [((t,), 4.0) for t in setup["ban_ids"]]
    res = setup["gen"](sequence_bias=table, repetition_penalty=1.3, record_logprobs=True)
    worst_other_order = 0.0
    for w, r in enumerate(res):
        chosen, best = _oracle(setup, w, r, table, penalty=1.3)
        print(f"window {w}: max |record - oracle| {np.max(np.abs(r.token_logprobs - chosen)):.4f}")
        assert np.all(chosen >= best - EPS), (w, chosen - best)
        assert np.all(np.abs(r.token_logprobs - chosen) <= EPS), (w, r.token_logprobs - chosen)
        # the other order (bias, then penalty) on the same oracle logits
        st, prompt = setup["st"], setup["prompt"]
        cross = setup["orc"].cross_kv(setup["encf"][w: w + 1])
        logits, _ = setup["orc"].decode(np.asarray([prompt + r.tokens]), cross)
        seq = r.tokens + ([st.eot] if len(prompt) + len(r.tokens) < ML else [])
        for i, t in enumerate(seq):
            x = apply_history_rules(apply_sequence_bias(logits[0, len(prompt) - 1 + i], r.tokens[:i], table),
                                    r.tokens[:i], 1.3)
            lp = log_softmax(apply_rules(x, r.tokens[:i], st, _sup(st), True, 50))
            worst_other_order = max(worst_other_order, abs(float(lp[t]) - float(r.token_logprobs[i])))
    print(f"other order: max |record - oracle| {worst_other_order:.4f}")
    assert worst_other_order > EPS                # the other order would miss the bound above


def test_beam_with_bias(setup):
    table = _ban_table(setup)
    res = setup["gen"](beam_size=5, patience=1.0, sequence_bias=table)
    for w, r in enumerate(res):
        assert r.tokens and _ban_holds(setup, r.tokens), (w, r.tokens)
        chosen, _ = _oracle(setup, w, r, table)
        assert np.all(np.isfinite(chosen))
        score = float(np.sum(chosen)) / max(len(r.tokens), 1)
        print(f"window {w}: score {r.score:.4f} oracle {score:.4f}")
        assert abs(score - r.score) < 2e-2 * max(1.0, abs(score)), (w, score, r.score)


def test_sampling_with_bias(setup):
    kw = dict(temperature=1.0, num_hypotheses=3, seed=7, sequence_bias=_ban_table(setup))
    a, b = setup["gen"](**kw), setup["gen"](**kw)
    for ra, rb in zip(a, b):
        assert ra.tokens and _ban_holds(setup, ra.tokens), ra.tokens
        assert ra.tokens == rb.tokens and ra.score == rb.score    # seeded -> reproducible


@pytest.mark.parametrize("beam", [1, 5])
def test_row_set_decode_with_bias(setup, beam):
    """Two windows in flight over the four, so two slots are refilled: a refilled slot's history restarts with its
    new window (the bigram's prefix is matched against the new window's tokens only)."""
    stats = {}
    res = setup["gen"](beam_size=beam, max_rows=2 * beam, compact=True, sequence_bias=_ban_table(setup), stats=stats)
    assert stats["refills"] >= 1
    for w, r in enumerate(res):
        assert r.tokens and _ban_holds(setup, r.tokens), (w, r.tokens)


def test_ragged_prompts_history_starts_after_the_prompt(setup):
    """Two prompt lengths in one call, without timestamps so that a text id is legal at step 0.  Windows 1 and 3 have
    a prompt that ENDS in a; the entry (a, c) must not fire at their step 0 (G = 0: the history is empty).  A kernel
    that matched into the prompt would add 30 to c there."""
    st = setup["st"]
    nots = setup["prompt"] + [st.no_timestamps]
    plain = setup["gen"](prompts=[nots] * setup["W"], with_timestamps=False)
    a = Counter(t for r in plain for t in r.tokens if t < st.eot and t != st.blank).most_common(1)[0][0]
    used = {t for r in plain for t in r.tokens}
    c = next(t for t in range(1000, st.eot) if t not in used and t != st.blank)
    prompts = [nots + [a] if w % 2 else nots for w in range(setup["W"])]
    table = [((a, c), BOOST)]
    res = setup["gen"](prompts=prompts, with_timestamps=False, sequence_bias=table, record_logprobs=True)
    adjacent = 0
    for w, r in enumerate(res):
        chosen, best = _oracle(setup, w, r, table, prompt=prompts[w], with_timestamps=False)
        err = np.abs(r.token_logprobs - chosen)
        print(f"window {w}: prompt {len(prompts[w])}, first token {r.tokens[0]}, |record - oracle| step 0 {err[0]:.4f} "
              f"max {np.max(err):.4f}")
        assert err[0] <= EPS and np.all(err <= EPS), (w, err)
        assert np.all(chosen >= best - EPS), (w, chosen - best)
        if w % 2:
            assert r.tokens[0] != c
        adjacent += completions(r.tokens, (a, c))
    assert adjacent >= 1                          # the entry does fire once a is GENERATED


@pytest.mark.parametrize("beam", [1, 5])
def test_no_table_is_inert_and_the_table_is_cleared(setup, beam):
    key = lambda res: [(r.tokens, r.score, r.cum_logprob) for r in res]
    first = setup["gen"](beam_size=beam)
    assert key(setup["gen"](beam_size=beam, sequence_bias=None)) == key(first)
    assert key(setup["gen"](beam_size=beam, sequence_bias=[])) == key(first)
    assert key(setup["gen"](beam_size=beam, sequence_bias=_ban_table(setup))) != key(first)
    assert key(setup["gen"](beam_size=beam)) == key(first)                     # the biased call left no table behind


def test_invalid_tables_raise_and_name_the_entry(setup):
    V, gen = setup["dims"].n_vocab, setup["gen"]
    ok = ((5,), 1.0)
    for table, what in (([ok, ((), 1.0)], "entry 1"), ([ok, ok, (tuple(range(17)), 1.0)], "entry 2"),
                        ([((5, V), 1.0)], "entry 0"), ([ok, ((-1,), 1.0)], "entry 1"),
                        ([ok, ((6,), float("nan"))], "entry 1"), ([((6,), float("inf"))], "entry 0"),
                        ([((1 + i,), 1.0) for i in range(1025)], "1024")):
        with pytest.raises(RuntimeError, match=what):
            gen(sequence_bias=table)
    assert [r.tokens for r in gen()] == [r.tokens for r in setup["plain"]]     # the engine is usable afterwards
    # offsets that do not ascend (the raw entry point), with a table in place: the refused call leaves it there
    eng = setup["eng"]
    eng.set_sequence_bias(_ban_table(setup))
    try:
        off = (C.c_int32 * 3)(0, 2, 1)
        tok = (C.c_int32 * 2)(5, 6)
        val = (C.c_float * 2)(1.0, 1.0)
        assert eng.lib.wm_set_sequence_bias(eng.h, 2, off, tok, val, eng.stream_ptr()) == -1
        assert b"entry 1" in eng.lib.wm_last_error()
        for w, r in enumerate(gen()):             # no sequence_bias argument: the engine's table holds
            assert r.tokens and _ban_holds(setup, r.tokens), (w, r.tokens)
    finally:
        eng.set_sequence_bias(())
    assert [r.tokens for r in gen()] == [r.tokens for r in setup["plain"]]


def test_table_of_the_limits(setup):
    """1024 entries, 1021 of them 16 tokens long (the table's capacity, the longest prefix compare, a binary search
    over the full list): entries that never fire around the three that act."""
    st = setup["st"]
    filler = [(tuple([setup["c"]] * 15 + [(7 * i) % st.eot]), BOOST) for i in range(1024 - 3)]   # prefix c c c ...: never
    table = filler[:500] + [((t,), BAN) for t in setup["ban_ids"]] + filler[500:]
    res = setup["gen"](sequence_bias=table)
    want = setup["gen"](sequence_bias=[((t,), BAN) for t in setup["ban_ids"]])
    assert [r.tokens for r in res] == [r.tokens for r in want]
    assert [r.tokens for r in res] != [r.tokens for r in setup["plain"]]


# ---- public surface
@pytest.fixture(scope="module")
def model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cuda", eot_after=60)


@pytest.fixture(scope="module")
def clip():
    return speech_like(20.0, 410)                                 # one window


def _window_tokens(segments):
    by_seek = {}
    for s in segments:
        by_seek.setdefault(s.seek, []).extend(s.tokens)
    return list(by_seek.values())


def test_transcribe_bans_a_word(model, clip):
    from vlog_amd.segments import build_sequence_bias
    from vlog_amd.transcribe import BatchedInferencePipeline
    kw = dict(language="en", beam_size=1, temperature=0)
    tok = model.tokenizer(language="en")
    segs, info = model.transcribe(clip, condition_on_previous_text=False, **kw)
    plain = [t for s in segs for t in s.tokens]
    assert info.transcription_options.sequence_bias is None and info.transcription_options.sequence_bias_table is None
    # a piece of the plain transcript whose text encodes back to that one token: the string key bans at least that id
    t = next(t for t in plain if t < tok.eot and t != model.dims.specials.blank and tok.decode([t]).strip()
             and tok.encode(tok.decode([t])) == [t])
    word = tok.decode([t])
    mapping = {word: BAN}
    table = build_sequence_bias(tok.encode, mapping, model.dims.n_vocab)
    assert ((t,), BAN) in table

    def banned(wins):
        return wins and all(toks and completions(toks, seq) == 0 for toks in wins for seq, _ in table)

    segs, info = model.transcribe(clip, condition_on_previous_text=False, sequence_bias=mapping, **kw)
    wins = _window_tokens(segs)
    assert banned(wins), wins
    assert info.transcription_options.sequence_bias == mapping
    assert info.transcription_options.sequence_bias_table == table
    pipe = BatchedInferencePipeline(model)
    segs, info = pipe.transcribe(clip, vad_filter=False, sequence_bias=mapping, **kw)
    wins = _window_tokens(segs)
    assert len(wins) == 1 and banned(wins), wins
    assert info.transcription_options.sequence_bias == mapping
    # several files: one mapping for all of them
    clip2 = speech_like(20.0, 411)
    for segs, info in model.transcribe_many([clip, clip2], condition_on_previous_text=False, sequence_bias=mapping, **kw):
        assert banned(_window_tokens(segs)) and info.transcription_options.sequence_bias == mapping
    for segs, info in pipe.transcribe_many([clip, clip2], vad_filter=False, sequence_bias=mapping, **kw):
        assert banned(_window_tokens(segs)) and info.transcription_options.sequence_bias == mapping
    with pytest.raises(ValueError, match="per-file"):
        model.transcribe_many([clip, clip2], sequence_bias=[mapping, mapping], **kw)
    with pytest.raises(ValueError, match="per-file"):
        pipe.transcribe_many([clip, clip2], sequence_bias=[mapping, mapping], **kw)
