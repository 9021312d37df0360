"""wm_language_id on the MI355X: the language head (lang_head_kernel: final LayerNorm + the language rows of the tied
embedding + mask + softmax + argmax) against the CPU oracle, against the full-vocabulary path (wm_detect_language),
its exact properties, row independence, the call-time refusals, and the public interface end to end
(language_candidates, VLOG_AMD_LANGUAGE_CANDIDATES, language_timeline).

The model and the windows are those of tests/test_gpu_decode.py's fixture, rebuilt here: synthetic `tiny`, seed 3,
W = 4 windows of speech_like audio (seeds 200..203); the engine-level tests also run on `base` (d = 512: every lane of
a wave owns a chunk of an embedding row, where d = 384 leaves lanes 48..63 idle).

Gaps between the two best languages in the bf16-format oracle's log-probabilities (computed on the CPU with the
oracle's own encoder before any GPU run; a window may be skipped in the oracle comparison when its gap is within
2 EPS = 0.04 nats, at most one of the four):
    tiny   window 0..3: 0.0828, 0.0845, 0.0843, 0.0811 nats  (sw over ca)
    base   window 0..3: 0.3228, 0.3121, 0.3066, 0.3028 nats  (yi over la)
so with these seeds no window is skipped.
"""
import numpy as np
import pytest
import torch

import lang_id_ref as ref
from oracle import mel as omel
from oracle.decode import detect_language
from oracle.model import OracleWhisper
from vlog_amd.audio import speech_like
from vlog_amd.dims import model_dims
from vlog_amd.weights import round_bf16, synthetic_state_dict

pytestmark = pytest.mark.gpu

EPS = 0.02   # nats, the bf16 logit noise floor
W = 4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module", params=["tiny", "base"])
def setup(request):
    from vlog_amd.engine import GpuEngine
    dims = model_dims(request.param)
    sd = synthetic_state_dict(dims, seed=3, eot_after=60)
    eng = GpuEngine(dims, sd, 0)
    bf = OracleWhisper(round_bf16(sd), dims, np.float32, bf16_acts=True)      # the engine's numeric format
    x = np.concatenate([speech_like(30.0, 200 + i) for i in range(W)])
    feats = omel.log_mel(x, dims.n_mels)
    enc = eng.encode(torch.from_numpy(feats).cuda(), [3000 * i for i in range(W)], [3000] * W)
    eng.reserve(W, 40)
    eng.cross_kv(enc, 0)
    st = dims.specials
    encf = enc.float().cpu().numpy()
    # computed once, shared, never modified: the oracle's answer per window, and one n = 1 call per window
    oracle = [detect_language(bf, bf.cross_kv(encf[w: w + 1]), st) for w in range(W)]
    single = [eng.language_id([w], st.lang_begin, st.n_langs) for w in range(W)]
    return dict(dims=dims, eng=eng, st=st, oracle=oracle, single=single)


def _lid(s, slots, allowed=None):
    return s["eng"].language_id(slots, s["st"].lang_begin, s["st"].n_langs, allowed)


def test_against_the_oracle(setup):
    """Per window: the oracle's language and its probability within 5e-3 (the bound test_gpu_decode.py uses for the
    full-vocabulary path); a window whose two best oracle languages are within 2 EPS may be skipped, at most one."""
    st = setup["st"]
    skipped = 0
    for w in range(W):
        want = setup["oracle"][w]
        probs, top, top_prob = setup["single"][w]
        gap = np.log(want[0][1]) - np.log(want[1][1])
        print(f"d = {setup['dims'].n_state} window {w}: oracle {want[0]} gap {gap:.4f} nats, "
              f"engine {st.lang_codes[int(top[0])]} {float(top_prob[0]):.6f}")
        if gap <= 2 * EPS:
            skipped += 1
            continue
        assert st.lang_codes[int(top[0])] == want[0][0]
        assert abs(float(top_prob[0]) - want[0][1]) < 5e-3
        assert top_prob[0] == probs[0, top[0]] == probs[0].max()
        assert abs(float(probs[0].astype(np.float64).sum()) - 1.0) < 1e-6
    assert skipped <= 1


def test_against_the_full_vocabulary_path(setup):
    """language_id without a mask vs detect_language on the same slots: the same best language, and for every
    language with p >= 1e-4 the log-probabilities within 2 EPS (both are f32 sums of the same bf16 x bf16 products, in
    different orders).  The largest difference observed is recorded in DESIGN.md §8."""
    st, eng = setup["st"], setup["eng"]
    slots = list(range(W))
    old = eng.detect_language(slots, st.lang_begin, st.n_langs)
    new, top, _ = _lid(setup, slots)
    worst = 0.0
    for w in range(W):
        assert int(top[w]) == int(np.argmax(old[w]))
        big = old[w] >= 1e-4
        assert big.any()
        diff = np.abs(np.log(new[w][big].astype(np.float64)) - np.log(old[w][big].astype(np.float64)))
        worst = max(worst, float(diff.max()))
    print(f"largest |log p_new - log p_old| over p >= 1e-4: {worst:.3e} nats")
    assert worst <= 2 * EPS


def test_exact_properties_of_the_mask(setup):
    st = setup["st"]
    n = st.n_langs
    full = [setup["single"][w][0][0] for w in range(W)]
    rng = np.random.default_rng(5)
    for w in range(W):
        allowed = np.zeros(n, np.uint8)
        allowed[rng.choice(n, 7, replace=False)] = 1
        allowed[int(np.argmin(full[w]))] = 1                  # the least likely language too
        probs, top, top_prob = _lid(setup, [w], allowed)
        p = probs[0]
        assert np.all(_bits(p[allowed == 0]) == 0)            # masked entries: exactly +0.0
        assert abs(float(p.astype(np.float64).sum()) - 1.0) < 1e-6
        want = ref.renormalised(full[w], allowed)
        on = allowed != 0
        assert np.all(np.abs(p[on].astype(np.float64) - want[on]) <= 1e-6 * want[on])
        assert int(top[0]) == ref.top(want)[0] and top_prob[0] == p[top[0]]
    # an all-ones mask is the unmasked call, bit for bit
    probs, top, top_prob = _lid(setup, [1], np.ones(n, np.uint8))
    one = setup["single"][1]
    assert np.array_equal(_bits(probs), _bits(one[0])) and np.array_equal(top, one[1])
    assert np.array_equal(_bits(top_prob), _bits(one[2]))
    # a single language: that language with probability 1 (first, last and a middle one)
    for j in (0, n // 2, n - 1):
        allowed = np.zeros(n, np.uint8)
        allowed[j] = 1
        probs, top, top_prob = _lid(setup, [2], allowed)
        assert int(top[0]) == j and float(top_prob[0]) == 1.0
        assert probs[0, j] == 1.0 and np.all(_bits(np.delete(probs[0], j)) == 0)


def test_rows_do_not_depend_on_the_call(setup):
    """n = 9 over repeated, shuffled slots is bit-identical, row by row, to nine n = 1 calls; and across the engine's
    seam between decoder passes (160 rows per pass; no option reaches it, so n = 169 does): the rows of the second pass
    (9 rows, the one-row calls' decoder route) are bit-identical to the n = 1 calls, the rows of the first pass are
    bit-identical among the rows of the same slot and agree with the n = 1 calls to 2 EPS (a 160-row pass takes other
    GEMM routes through the decoder: DESIGN.md §3), in call order."""
    slots = [2, 0, 3, 1, 2, 2, 0, 1, 3]
    probs, top, top_prob = _lid(setup, slots)
    for r, s in enumerate(slots):
        one = setup["single"][s]
        assert np.array_equal(_bits(probs[r]), _bits(one[0][0])), (r, s)
        assert top[r] == one[1][0] and _bits(top_prob[r: r + 1])[0] == _bits(one[2])[0]
    allowed = np.zeros(setup["st"].n_langs, np.uint8)
    allowed[[3, 11, 40]] = 1
    masked, mtop, _ = _lid(setup, slots, allowed)
    for r, s in enumerate(slots):
        m1, t1, _ = _lid(setup, [s], allowed)
        assert np.array_equal(_bits(masked[r]), _bits(m1[0])) and mtop[r] == t1[0]
    long_slots = [(7 * i + i // 5) % W for i in range(160)] + slots
    probs, top, _ = _lid(setup, long_slots)
    first = {}
    for r, s in enumerate(long_slots):
        one = setup["single"][s]
        if r >= 160:
            assert np.array_equal(_bits(probs[r]), _bits(one[0][0])), (r, s)
            continue
        first.setdefault(s, r)
        assert np.array_equal(_bits(probs[r]), _bits(probs[first[s]])), (r, s)
        assert top[r] == one[1][0]
        big = one[0][0] >= 1e-4
        assert np.abs(np.log(probs[r][big].astype(np.float64)) - np.log(one[0][0][big].astype(np.float64))).max() <= 2 * EPS
    assert sorted(first) == list(range(W))


def test_refusals_leave_the_engine_usable(setup):
    st, eng, dims = setup["st"], setup["eng"], setup["dims"]
    prompt = [st.sot, st.lang_token("en"), st.transcribe]
    before, _ = eng.generate([1], [prompt], max_length=24)
    n = st.n_langs
    with pytest.raises(RuntimeError, match=r"wm_language_id: lang_begin \.\. lang_begin \+ n_langs outside the vocabulary"):
        eng.language_id([0], dims.n_vocab - 10, n)
    with pytest.raises(RuntimeError, match=r"wm_language_id: lang_begin \.\. lang_begin \+ n_langs outside the vocabulary"):
        eng.language_id([0], -1, n)
    with pytest.raises(RuntimeError, match=r"wm_language_id: n_langs outside 1\.\.128"):
        eng.language_id([0], 0, 129)
    with pytest.raises(RuntimeError, match=r"wm_language_id: n_langs outside 1\.\.128"):
        eng.language_id([0], st.lang_begin, 0)
    with pytest.raises(RuntimeError, match=r"wm_language_id: h_allowed sets no language"):
        eng.language_id([0], st.lang_begin, n, np.zeros(n, np.uint8))
    with pytest.raises(RuntimeError, match=r"wm_language_id: h_slots\[1\] outside the reserved slots"):
        eng.language_id([0, eng.n_slots], st.lang_begin, n)
    probs, top, top_prob = eng.language_id([], st.lang_begin, n)          # nothing to do is not an error
    assert probs.shape == (0, n) and top.shape == (0,)
    after, _ = eng.generate([1], [prompt], max_length=24)
    assert after[0].tokens == before[0].tokens and after[0].tokens
    again = _lid(setup, [3])
    assert np.array_equal(_bits(again[0]), _bits(setup["single"][3][0]))


def test_non_finite_rows_are_reported():
    """A NaN in the final LayerNorm's weight makes every language logit NaN: the kernel sets the device error word
    and the call fails naming a row, instead of returning NaN probabilities (an engine of its own, `tiny`)."""
    from vlog_amd.engine import GpuEngine
    dims = model_dims("tiny")
    sd = synthetic_state_dict(dims, seed=3, eot_after=60)
    sd["model.decoder.layer_norm.weight"][5] = float("nan")
    eng = GpuEngine(dims, sd, 0)
    feats = omel.log_mel(np.concatenate([speech_like(30.0, 200), speech_like(30.0, 201)]), dims.n_mels)
    enc = eng.encode(torch.from_numpy(feats).cuda(), [0, 3000], [3000, 3000])
    eng.reserve(2, 8)
    eng.cross_kv(enc, 0)
    st = dims.specials
    with pytest.raises(RuntimeError, match=r"wm_language_id: non-finite logits, row [01]$"):
        eng.language_id([0, 1], st.lang_begin, st.n_langs)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model():
    from vlog_amd.transcribe import WhisperModel
    return WhisperModel("synthetic:tiny:3", device="cuda", eot_after=60)


CLIP = dict(beam_size=1, temperature=0.0)


def _tokens(segs):
    return [s.tokens for s in segs]


def test_transcribe_with_candidates(model, monkeypatch):
    monkeypatch.delenv("VLOG_AMD_LANGUAGE_CANDIDATES", raising=False)
    clip = np.concatenate([speech_like(30.0, 300), speech_like(12.0, 301)])
    segs0, info0 = model.transcribe(clip, language=None, **CLIP)            # today's path, before anything is set
    toks0 = _tokens(segs0)
    assert info0.transcription_options.language_candidates is None
    assert len(info0.all_language_probs) == model.dims.specials.n_langs
    winner = info0.language
    other = "en" if winner != "en" else "es"
    segs, info = model.transcribe(clip, language=None, language_candidates=[other, winner], **CLIP)
    toks = _tokens(segs)
    assert info.language in {other, winner} and info.language == winner
    assert sorted(c for c, _ in info.all_language_probs) == sorted([other, winner])
    assert abs(sum(p for _, p in info.all_language_probs) - 1.0) < 1e-6
    assert info.all_language_probs[0] == (info.language, info.language_probability)
    assert info.all_language_probs[0][1] >= info.all_language_probs[1][1]
    assert info.transcription_options.language_candidates == (other, winner)
    pinned, _ = model.transcribe(clip, language=winner, **CLIP)
    assert toks == _tokens(pinned) and toks
    # a whitelist without the unrestricted winner: the language is still one of the candidates
    _, info2 = model.transcribe(clip, language=None, language_candidates=["de", "fr"], language_detection_segments=2, **CLIP)
    assert info2.language in {"de", "fr"} and sorted(c for c, _ in info2.all_language_probs) == ["de", "fr"]
    # a call that names its language ignores the whitelist
    _, info3 = model.transcribe(clip, language="en", language_candidates=["de", "fr"], **CLIP)
    assert info3.language == "en" and info3.transcription_options.language_candidates is None
    with pytest.raises(ValueError, match="unknown language code 'xx'"):
        model.transcribe(clip, language_candidates=["en", "xx"], **CLIP)
    # the environment does the same for a call without the argument; the empty sequence turns it off again
    monkeypatch.setenv("VLOG_AMD_LANGUAGE_CANDIDATES", f"{other},{winner}")
    segs_e, info_e = model.transcribe(clip, language=None, **CLIP)
    assert _tokens(segs_e) == toks
    assert (info_e.language, info_e.language_probability, info_e.all_language_probs) == \
        (info.language, info.language_probability, info.all_language_probs)
    assert info_e.transcription_options.language_candidates == (other, winner)
    segs_off, info_off = model.transcribe(clip, language=None, language_candidates=[], **CLIP)
    assert _tokens(segs_off) == toks0
    assert (info_off.language, info_off.language_probability, info_off.all_language_probs) == \
        (info0.language, info0.language_probability, info0.all_language_probs)
    assert info_off.transcription_options.language_candidates is None
    assert info_off.transcription_options == info0.transcription_options


def test_the_other_entry_points_echo_the_option(model, monkeypatch):
    from vlog_amd.transcribe import BatchedInferencePipeline
    monkeypatch.delenv("VLOG_AMD_LANGUAGE_CANDIDATES", raising=False)
    a, b = speech_like(20.0, 340), speech_like(14.0, 341)
    cands = ["es", "en", "de"]
    many = model.transcribe_many([a, b], language=[None, "fr"], language_candidates=cands, **CLIP)
    assert many[0][1].language in cands and many[0][1].transcription_options.language_candidates == tuple(cands)
    assert sorted(c for c, _ in many[0][1].all_language_probs) == sorted(cands)
    assert many[1][1].language == "fr" and many[1][1].transcription_options.language_candidates is None
    with pytest.raises(ValueError, match="not a per-file list"):
        model.transcribe_many([a, b], language_candidates=[["en"], ["es"]], **CLIP)
    pipe = BatchedInferencePipeline(model, max_batch_windows=4)
    _, info = pipe.transcribe(a, language_candidates=cands, vad_filter=False, **CLIP)
    assert info.language in cands and info.transcription_options.language_candidates == tuple(cands)
    assert abs(sum(p for _, p in info.all_language_probs) - 1.0) < 1e-6 and len(info.all_language_probs) == 3
    out = pipe.transcribe_many([a, b], language_candidates=cands, vad_filter=False, **CLIP)
    for _, inf in out:
        assert inf.language in cands and inf.transcription_options.language_candidates == tuple(cands)
    _, info = pipe.transcribe(a, vad_filter=False, **CLIP)
    assert info.transcription_options.language_candidates is None and len(info.all_language_probs) > 3
    lang, prob, allp = model.detect_language(a, language_candidates=cands, language_detection_segments=3)
    assert lang in cands and allp[0] == (lang, prob) and len(allp) == 3


def test_language_timeline(model, monkeypatch):
    monkeypatch.delenv("VLOG_AMD_LANGUAGE_CANDIDATES", raising=False)
    st = model.dims.specials
    clip = np.concatenate([speech_like(30.0, 350), speech_like(30.0, 351), speech_like(10.0, 352)])
    out = model.language_timeline(clip)
    assert [(w.start, w.end) for w in out] == [(0.0, 30.0), (30.0, 60.0), (60.0, 70.0)]
    # the three windows are still in slots 0..2: the same encoded windows through the engine
    probs, top, top_prob = model.engine.language_id([0, 1, 2], st.lang_begin, st.n_langs)
    for i, w in enumerate(out):
        assert w.language == st.lang_codes[int(top[i])] and w.probability == float(top_prob[i])
        assert w.probs == tuple((c, float(p)) for c, p in zip(st.lang_codes, probs[i]))
    cands = ("en", "ja")
    out = model.language_timeline(clip, language_candidates=cands, max_windows=2)
    probs, top, top_prob = model.engine.language_id([0, 1], st.lang_begin, st.n_langs,
                                                    [int(c in cands) for c in st.lang_codes])
    assert len(out) == 2
    for i, w in enumerate(out):
        assert w.language in cands and w.language == st.lang_codes[int(top[i])] and w.probability == float(top_prob[i])
        assert w.probs == tuple((c, float(probs[i, st.lang_codes.index(c)])) for c in cands)
        assert abs(sum(p for _, p in w.probs) - 1.0) < 1e-6
