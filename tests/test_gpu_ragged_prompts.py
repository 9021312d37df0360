"""Ragged prompts in wm_generate (ABI 4): one call whose windows have prompts of different lengths, as the lockstep
sequential mode produces them (`<|startofprev|>` + each file's own previous text), in every decode form.

Seven windows of speech_like audio on one random-weight tiny model; the prompts come from segments.build_prompt:
the bare sot sequence (shortest), two of equal mid length (20 previous tokens), one with a single previous token, the
longest build_prompt makes (223 previous tokens), one with a prefix; the sot sequence + <|notimestamps|> decodes
without timestamps in a call of its own.  The padding behind every prompt is -1: the engine neither reads nor
validates it.

Margins: the aim was audio and previous-text seeds whose oracle greedy decode keeps 0.1 nats between the two
best tokens at every step, so that no window needs a near-tie exemption.  tools/ragged_seed_search.py walks
candidates on the CPU oracle; on this random-weight model none comes near (the best of 12 bare-prompt candidates held 0.005 nats, the rest 0.001 to 0.004: the model's top-2
margins sit below the bf16 noise floor, as tests/test_gpu_repetition.py also notes), so the seeds are the first ones
and ONE window carries the exemption from strict identity with the oracle: window 3 (one previous token, 32 generated
tokens), whose GPU decode sits 0.0023 nats below the oracle's argmax at its worst step.  Every other check of that
window (margin within eps, score, no-speech, equality with its solo call) holds without exemption, and all other
windows are strictly identical.
"""
import numpy as np
import pytest
import torch

from oracle import mel as omel
from oracle.decode import GenerateOptions
from oracle.model import OracleWhisper
from tests.parity_util import GATE_CUM_REL, GATE_NO_SPEECH, window_parity
from tests.repetition_ref import repeated_ngrams, teacher_forced_logprobs
from vlog_amd import segments as segs
from vlog_amd.audio import speech_like
from vlog_amd.dims import model_dims
from vlog_amd.tokenizer import Tokenizer
from vlog_amd.weights import round_bf16, synthetic_state_dict

pytestmark = pytest.mark.gpu

MODEL_SEED = 3
ML = 448
EXEMPT = 3                        # the one window that may miss strict identity with the oracle (module docstring)
# (audio seed, previous-text seed) per window
AUDIO_SEEDS = [700, 701, 702, 703, 704, 705, 706]
PREV_SEEDS = [0, 11, 12, 13, 14, 15, 16]
KINDS = ["bare", "prev20", "prev20", "prev1", "prev223", "prefix", "bare"]
NOTS_AUDIO_SEED = 707             # the <|notimestamps|> window (its own call)
REC_EPS = 0.02                    # nats: the bound tests/test_gpu_configs.py holds per-step records to


def _sup(st):
    return [st.transcribe, st.translate, st.sot, st.sot_prev, st.sot_lm]


def build_prompts(dims, kinds=KINDS, prev_seeds=PREV_SEEDS):
    st = dims.specials
    tok = Tokenizer(dims, task="transcribe", language="en", seed=MODEL_SEED)

    def bp(prev=(), without_timestamps=False, prefix=None):
        return segs.build_prompt(tok.encode, tok.sot_sequence, tok.sot_prev, tok.no_timestamps, tok.timestamp_begin, ML,
                                 prev, without_timestamps, prefix, None)

    out = []
    for kind, seed in zip(kinds, prev_seeds):
        rng = np.random.default_rng(1000 + seed)
        n = {"bare": 0, "prev1": 1, "prev20": 20, "prev223": 400, "prefix": 0, "nots": 0}[kind]   # 400: cut to 223
        prev = [int(t) for t in rng.integers(300, st.eot - 1, size=n)]
        out.append(bp(prev, without_timestamps=kind == "nots", prefix="hello there" if kind == "prefix" else None))
    return out


def pad(prompts, fill=-1):
    P = max(len(p) for p in prompts)
    return [list(p) + [fill] * (P - len(p)) for p in prompts], [len(p) for p in prompts]


@pytest.fixture(scope="module")
def setup():
    from vlog_amd.engine import GpuEngine
    dims = model_dims("tiny")
    sd = synthetic_state_dict(dims, seed=MODEL_SEED, eot_after=60)
    eng = GpuEngine(dims, sd, 0)
    orc = OracleWhisper(round_bf16(sd), dims, np.float32)
    W = len(AUDIO_SEEDS)
    x = np.concatenate([speech_like(30.0, s) for s in AUDIO_SEEDS + [NOTS_AUDIO_SEED]])
    feats = omel.log_mel(x, dims.n_mels)
    enc = eng.encode(torch.from_numpy(feats).cuda(), [3000 * i for i in range(W + 1)], [3000] * (W + 1))
    eng.reserve(W + 1, 40)
    eng.cross_kv(enc, 0)
    st = dims.specials
    prompts = build_prompts(dims)
    assert len(prompts[0]) == min(map(len, prompts)) and len(prompts[1]) == len(prompts[2])
    assert len(prompts[4]) == 1 + 223 + len(prompts[0]) and len(set(map(len, prompts))) >= 5
    rows, lens = pad(prompts)

    def gen(slots=None, padded=False, **kw):
        """the ragged call over all seven windows: prompts of different lengths (GpuEngine.generate pads the rows with
        -1 and passes the lengths), or with padded=True rows padded here and the lengths passed explicitly"""
        slots = list(range(W)) if slots is None else slots
        kw.setdefault("max_length", ML)
        if padded:
            return eng.generate(slots, [rows[w] for w in slots], prompt_lens=[lens[w] for w in slots],
                                suppress_tokens=_sup(st), **kw)[0]
        return eng.generate(slots, [prompts[w] for w in slots], suppress_tokens=_sup(st), **kw)[0]

    def solo(w, **kw):
        """window w alone through the one-length path (NULL per-window pointers)"""
        kw.setdefault("max_length", ML)
        return eng.generate([w], [prompts[w]], suppress_tokens=_sup(st), **kw)[0][0]

    s = dict(dims=dims, eng=eng, orc=orc, encf=enc.float().cpu().numpy(), W=W, st=st, prompts=prompts, gen=gen, solo=solo)
    s["greedy"] = gen(record_logprobs=True)              # shared by the tests below, never modified
    return s


def _opt(st, **kw):
    return GenerateOptions(beam_size=1, max_length=ML, suppress_tokens=_sup(st), **kw)


def test_greedy_ragged_vs_oracle(setup):
    """Each window of the ragged call against the CPU oracle with that window's own prompt."""
    s, st = setup, setup["st"]
    not_identical = []
    for w, r in enumerate(s["greedy"]):
        p = window_parity(s["orc"], s["encf"][w], s["prompts"][w], r, st, _opt(st), w)
        print(f"window {w}: prompt {len(s['prompts'][w])}, {p.n_tokens} tokens, identical {p.identical}, min margin "
              f"{p.min_margin:.4f} (rule tie {p.min_margin_rule_tie:.4f}), score {p.score_gpu:.5f} / {p.score_oracle:.5f}, "
              f"no_speech {p.no_speech_gpu:.6f} / {p.no_speech_oracle:.6f}")
        assert p.n_tokens > 0
        assert p.min_margin_rule_tie >= -0.05, p
        assert abs(p.score_gpu - p.score_oracle) / max(1.0, abs(p.score_oracle)) <= GATE_CUM_REL, p
        assert abs(p.no_speech_gpu - p.no_speech_oracle) <= GATE_NO_SPEECH, p
        if not p.identical:
            not_identical.append(w)
    assert not_identical in ([], [EXEMPT]), not_identical


def test_no_timestamps_window_own_call(setup):
    """sot sequence + <|notimestamps|>: decoded without timestamps, ragged arguments with one window."""
    s, st = setup, setup["st"]
    prompt = build_prompts(s["dims"], ["nots"], [0])[0]
    assert prompt[-1] == st.no_timestamps
    W = s["W"]
    row = prompt + [-1] * 5
    r = s["eng"].generate([W], [row], prompt_lens=[len(prompt)], suppress_tokens=_sup(st), max_length=ML,
                          with_timestamps=False)[0][0]
    assert r.tokens and all(t < st.timestamp_begin for t in r.tokens)
    p = window_parity(s["orc"], s["encf"][W], prompt, r, st, _opt(st, with_timestamps=False), W)
    print(p)
    assert p.min_margin_rule_tie >= -0.05 and abs(p.no_speech_gpu - p.no_speech_oracle) <= GATE_NO_SPEECH, p
    ref = s["eng"].generate([W], [prompt], suppress_tokens=_sup(st), max_length=ML, with_timestamps=False)[0][0]
    assert r.tokens == ref.tokens


def test_ragged_equals_solo_calls(setup):
    s = setup
    diff = []
    for w, r in enumerate(s["greedy"]):
        ref = s["solo"](w, record_logprobs=True)
        if r.tokens != ref.tokens:
            diff.append(w)
            continue
        assert abs(r.no_speech_prob - ref.no_speech_prob) <= GATE_NO_SPEECH, (w, r.no_speech_prob, ref.no_speech_prob)
        assert r.token_logprobs.shape == ref.token_logprobs.shape == (len(r.tokens) + 1,), (w, r.token_logprobs.shape)
        d = float(np.max(np.abs(r.token_logprobs - ref.token_logprobs)))
        do = float(np.max(np.abs(r.token_logprobs_other - ref.token_logprobs_other)))
        print(f"window {w}: {len(r.tokens)} tokens, max record diff {d:.5f} (other {do:.5f})")
        assert d <= REC_EPS and do <= REC_EPS, (w, d, do)
    assert not diff, diff          # (the exemption of window EXEMPT is against the oracle only; it is not needed here)


@pytest.mark.parametrize("compact", [False, True])
def test_row_set_refills_mixed_lengths(setup, compact):
    stats = {}
    res = setup["gen"](max_rows=2, compact=compact, stats=stats)
    assert stats["refills"] > 0, stats
    assert [r.tokens for r in res] == [r.tokens for r in setup["greedy"]]
    assert [r.tokens for r in setup["gen"](padded=True, max_rows=2, compact=compact)] == [r.tokens for r in res]
    for r, g in zip(res, setup["greedy"]):
        assert abs(r.no_speech_prob - g.no_speech_prob) <= GATE_NO_SPEECH


@pytest.fixture(scope="module")
def beam_solo(setup):
    return [setup["solo"](w, beam_size=5, patience=1.0) for w in range(setup["W"])]


@pytest.mark.parametrize("form", [dict(), dict(max_rows=10), dict(compact=True)], ids=["lockstep", "rows10", "compact"])
def test_beam5_ragged_equals_solo(setup, beam_solo, form):
    stats = {}
    res = setup["gen"](beam_size=5, patience=1.0, stats=stats, **form)
    if "max_rows" in form:
        assert stats["refills"] > 0, stats
    for w, (r, ref) in enumerate(zip(res, beam_solo)):
        print(f"window {w}: {len(r.tokens)} tokens, cum {r.cum_logprob:.4f} / solo {ref.cum_logprob:.4f}")
        assert r.tokens == ref.tokens, w
        assert abs(r.cum_logprob - ref.cum_logprob) / max(1.0, abs(ref.cum_logprob)) <= GATE_CUM_REL, w
        assert abs(r.no_speech_prob - ref.no_speech_prob) <= GATE_NO_SPEECH, w


def test_beam5_records_ragged(setup, beam_solo):
    """per-step records with beam search (max_rows 0): the finished hypothesis' records start at its own prompt length"""
    res = setup["gen"](beam_size=5, patience=1.0, record_logprobs=True)
    for w, (r, ref) in enumerate(zip(res, beam_solo)):
        assert r.tokens == ref.tokens, w
        solo = setup["solo"](w, beam_size=5, patience=1.0, record_logprobs=True)
        assert r.token_logprobs.shape == solo.token_logprobs.shape, (w, r.token_logprobs.shape, solo.token_logprobs.shape)
        d = float(np.max(np.abs(r.token_logprobs - solo.token_logprobs)))
        print(f"window {w}: {len(r.tokens)} tokens, max beam record diff {d:.5f}")
        assert d <= REC_EPS, (w, d)


def test_sampling_reproducible_and_tables_keep_meaning(setup):
    s, st = setup, setup["st"]
    kw = dict(temperature=0.4, num_hypotheses=3, seed=5)
    a, b = s["gen"](**kw), s["gen"](**kw)
    assert all(r.tokens for r in a)
    assert [r.tokens for r in a] == [r.tokens for r in b] and [r.score for r in a] == [r.score for r in b]
    # equal lengths: the call with the per-window tables equals the one-length call token for token
    same = [1, 2]
    P = len(s["prompts"][1])
    uni = s["eng"].generate(same, [s["prompts"][w] for w in same], suppress_tokens=_sup(st), max_length=ML, **kw)[0]
    rag = s["eng"].generate(same, [s["prompts"][w] for w in same], prompt_lens=[P, P], suppress_tokens=_sup(st),
                            max_length=ML, **kw)[0]
    assert [r.tokens for r in uni] == [r.tokens for r in rag]
    # one sampled hypothesis through the row-set form (max_rows 1: the second window refills the slot)
    one_r = s["eng"].generate(same, [s["prompts"][w] for w in same], prompt_lens=[P, P], suppress_tokens=_sup(st),
                              max_length=ML, temperature=0.4, num_hypotheses=1, seed=5, max_rows=1)[0]
    one_u = s["eng"].generate(same, [s["prompts"][w] for w in same], suppress_tokens=_sup(st), max_length=ML,
                              temperature=0.4, num_hypotheses=1, seed=5, max_rows=1)[0]
    assert all(r.tokens for r in one_u) and [r.tokens for r in one_r] == [r.tokens for r in one_u]


def test_rules_start_at_each_windows_prompt(setup):
    """repetition penalty + bigram ban on the ragged call.  The rules' history is the window's GENERATED tokens
    (tests/repetition_ref.py), so the scan starts at the window's own prompt length: were it to start at another
    window's shorter length, the ids of this window's previous text would be penalised and its bigrams banned, and the
    decode would leave its solo decode (whose one-length call the existing repetition tests pin to the reference)."""
    s, st = setup, setup["st"]
    res = s["gen"](repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert [r.tokens for r in res] != [r.tokens for r in s["greedy"]]          # the rules had something to do
    for w, r in enumerate(res):
        assert r.tokens and not repeated_ngrams(r.tokens, 2), (w, r.tokens)
        ref = s["solo"](w, repetition_penalty=1.3, no_repeat_ngram_size=2)
        assert r.tokens == ref.tokens, w
        # every token is legal under the reference rules over the generated history alone
        cross = s["orc"].cross_kv(s["encf"][w: w + 1])
        ended = len(s["prompts"][w]) + len(r.tokens) < ML
        chosen, _ = teacher_forced_logprobs(s["orc"], cross, s["prompts"][w], r.tokens, st, _sup(st), ended, 1.3, 2)
        assert np.all(np.isfinite(chosen)), w
    # A previous text that already holds a bigram must not ban it.  Forced by construction: every id but two text
    # tokens a, b is suppressed (<|endoftext|> and the timestamps too, decoded without timestamps) and the window may
    # generate exactly 3 tokens, so it MUST emit two bigrams over {a, b}; its previous text holds all four of them
    # (a a b b a).  A scan that started before the window's own prompt length would find every continuation of the
    # first token banned and fail the call with "no token allowed".  The other window of the call has another length.
    a, b = 300, 301
    tok = Tokenizer(s["dims"], task="transcribe", language="en", seed=MODEL_SEED)
    prompt = segs.build_prompt(tok.encode, tok.sot_sequence, tok.sot_prev, tok.no_timestamps, tok.timestamp_begin, ML,
                               [a, a, b, b, a], True, None, None)
    other = s["prompts"][1]
    assert len(prompt) != len(other) and len(prompt) != len(s["prompts"][0])
    only_ab = [t for t in range(s["dims"].n_vocab) if t not in (a, b)]
    kw = dict(suppress_tokens=only_ab, with_timestamps=False, no_repeat_ngram_size=2)
    rr = s["eng"].generate([0, 1], [prompt, other], max_length=[len(prompt) + 3, len(other) + 3], **kw)[0]
    ref = s["eng"].generate([0], [prompt], max_length=len(prompt) + 3, **kw)[0][0]
    got = rr[0].tokens
    assert got == ref.tokens and len(got) == 3 and set(got) <= {a, b}, got
    held = {(a, a), (a, b), (b, b), (b, a)}
    assert (got[0], got[1]) in held and (got[1], got[2]) in held and not repeated_ngrams(got, 2), got
    assert len(rr[1].tokens) == 3 and not repeated_ngrams(rr[1].tokens, 2)


def test_per_window_max_length(setup):
    s = setup
    w = 3
    mls = [ML] * s["W"]
    mls[w] = len(s["prompts"][w]) + 5
    res = s["gen"](max_length=mls)
    assert len(s["greedy"][w].tokens) > 5
    assert res[w].tokens == s["greedy"][w].tokens[:5]
    for v in range(s["W"]):
        if v != w:
            assert res[v].tokens == s["greedy"][v].tokens, v
    # the row-set form reads the limit from the same table
    res = s["gen"](max_length=mls, max_rows=2)
    assert res[w].tokens == s["greedy"][w].tokens[:5]
    res = s["gen"](max_length=mls, beam_size=5, max_rows=10)
    assert 0 < len(res[w].tokens) <= 5


def test_validation_names_the_window(setup):
    s, st = setup, setup["st"]
    eng, V, C = s["eng"], s["dims"].n_vocab, s["dims"].n_text_ctx
    assert all(r.tokens for r in s["gen"](slots=[0, 4]))      # a good ragged call first
    good = [[st.sot, st.lang_token("en"), st.transcribe, -1, -1]] * 3
    lens = [3, 3, 3]

    def call(rows=good, lens=lens, **kw):
        kw.setdefault("max_length", 40)
        return eng.generate([0, 1, 2], rows, prompt_lens=lens, suppress_tokens=_sup(st), **kw)[0]

    for bad in (0, -2, 6):
        with pytest.raises(RuntimeError, match=r"window 1.*prompt length"):
            call(lens=[3, bad, 3])
    with pytest.raises(RuntimeError, match=r"window 2.*max length"):          # length >= its max length
        call(max_length=[40, 40, 3])
    with pytest.raises(RuntimeError, match=r"window 0.*max length"):          # above n_text_ctx
        call(max_length=[C + 1, 40, 40])
    with pytest.raises(RuntimeError, match=r"window 1.*sot index"):
        call(sot_index=[0, 3, 0])
    rows = [list(r) for r in good]
    rows[2][1] = V
    with pytest.raises(RuntimeError, match=r"window 2.*prompt token"):
        call(rows=rows)
    rows[2][1] = -1
    with pytest.raises(RuntimeError, match=r"window 2.*prompt token"):
        call(rows=rows)
    # an entry of h_max_lengths above max_length (the stride of h_tokens and of the record rows): GpuEngine.generate
    # takes the stride from the entries, so this one goes to the C entry point with a struct filled by hand
    import ctypes as C
    from vlog_amd import _capi
    W, P, stride = 3, 5, 40
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)       # noqa: E731
    ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))         # noqa: E731
    fptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))        # noqa: E731
    slots, prm, sup = i32([0, 1, 2]), i32(good), i32(_sup(st))
    lens_c, sots_c, mls_c = i32([3, 3, 3]), i32([0, 0, 0]), i32([stride, stride + 1, stride])
    toks, ln, steps = np.zeros((W, stride), np.int32), np.zeros(W, np.int32), np.zeros(1, np.int32)
    sc, cum, ns = (np.zeros(W, np.float32) for _ in range(3))
    a = _capi.GenerateArgsC()                                      # zero-filled, then the fields of a greedy call
    a.n_windows, a.h_slots, a.prompt_len, a.h_prompts, a.sot_index = W, ptr(slots), P, ptr(prm), 0
    a.beam_size, a.patience, a.length_penalty, a.max_length, a.num_hypotheses = 1, 1.0, 1.0, stride, 1
    a.h_suppress, a.n_suppress, a.suppress_blank, a.max_initial_timestamp_index = ptr(sup), int(sup.size), 1, 50
    a.with_timestamps, a.check_every = 1, 4
    a.h_tokens, a.h_lengths, a.h_scores, a.h_cum_logprob, a.h_no_speech = ptr(toks), ptr(ln), fptr(sc), fptr(cum), fptr(ns)
    a.h_steps = ptr(steps)
    a.h_prompt_lens, a.h_sot_indices, a.h_max_lengths = ptr(lens_c), ptr(sots_c), ptr(mls_c)
    with torch.cuda.device(0):
        rc = eng.lib.wm_generate(eng.h, C.byref(a), eng.stream_ptr())
        assert rc == -1
        msg = eng.lib.wm_last_error().decode()
        assert "window 1" in msg and "max length" in msg, msg
        assert not toks.any() and not ln.any()                     # nothing was decoded
        mls_c[1] = stride                                          # the same struct, corrected, succeeds
        assert eng.lib.wm_generate(eng.h, C.byref(a), eng.stream_ptr()) == 0, eng.lib.wm_last_error()
    assert all(0 < n <= stride - 3 for n in ln)
    # A correct call afterwards still succeeds, and the padding (-1, and an id >= V) is exempt
    rows = [list(r) for r in good]
    rows[0][4] = V + 7
    res = call(rows=rows)
    assert all(r.tokens for r in res)
