"""Opt-in fp8 K/V panels of the projected cross-attention form (wm_set_option "cross_kv_fp8" / VLOG_AMD_CROSS_KV_FP8),
end to end on synthetic tiny / base models.

  * Mode 1 (fp8 panels, converted on load) against mode 2 (the same quantiser, panels stored dequantised as bf16, the
    unchanged bf16 kernels): the two hold the same values, so every call gives identical tokens; scores,
    no_speech_prob and the per-step records are IDENTICAL where the passes run on cross_tf_kernel (beam groups, best_of
    groups: its arithmetic after LDS is the bf16 kernel's) and within the project's 0.02-nat record bound on the VALU
    kernels (one row per window).
  * Mode 1 against mode 0 (bf16 panels) on the margin-planted model: identical tokens; the largest record deviation is
    measured against what the existing factored cross_fp8 costs on the same windows and may be twice that.
  * Slot memory, re-allocation on switching, the option surface, and the form choice of transcribe().
"""
import numpy as np
import pytest
import torch

from vlog_amd.audio import speech_like
from vlog_amd.dims import model_dims
from vlog_amd.tokenizer import Tokenizer
from vlog_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

RECORD_BOUND = 0.02        # nats: the project's bound on per-step records between two routes of one computation
W = 4


class Bench:
    def __init__(self, name, seed=3, plant=None, windows=W, eot_after=40):
        from vlog_amd.engine import GpuEngine
        self.dims = model_dims(name)
        self.sd = synthetic_state_dict(self.dims, seed=seed, eot_after=None if plant else eot_after, plant=plant)
        self.eng = GpuEngine(self.dims, self.sd, 0)
        self.W = windows
        x = np.concatenate([speech_like(30.0, 700 + i) for i in range(windows)])
        mel = self.eng.features(torch.from_numpy(x))
        self.enc = self.eng.encode(mel, [3000 * i for i in range(windows)], [3000] * windows)
        tok = Tokenizer(self.dims, language="en")
        self.prompt, self.sup = list(tok.sot_sequence), list(tok.suppressed_tokens([-1]))
        self.prev = self.dims.specials.sot_prev

    def load(self, eng=None, **opts):
        """Options set, slots reserved, the windows' cross memory written."""
        eng = eng or self.eng
        for k, v in opts.items():
            eng.set_option(k, v)
        eng.reserve(self.W, self.W * 5)
        eng.cross_kv(self.enc, 0)
        return eng

    def calls(self, eng=None):
        """The decode forms of wm_generate that read projected panels: name -> results."""
        eng = eng or self.eng
        sl, kw = list(range(self.W)), dict(suppress_tokens=self.sup, max_length=96, record_logprobs=True)
        ragged = [([self.prev] + [1000 + 3 * w + i for i in range(2 * w)] if w else []) + self.prompt for w in range(self.W)]
        out = {}
        out["greedy"] = eng.generate(sl, [self.prompt] * self.W, **kw)[0]
        out["beam5"] = eng.generate(sl, [self.prompt] * self.W, beam_size=5, patience=1.0, **kw)[0]
        out["best_of5"] = eng.generate(sl, [self.prompt] * self.W, temperature=0.8, num_hypotheses=5, seed=11, **kw)[0]
        out["ragged"] = eng.generate(sl, ragged, **kw)[0]
        out["ragged_beam5"] = eng.generate(sl, ragged, beam_size=5, patience=1.0, **kw)[0]
        out["rowset"] = eng.generate(sl, [self.prompt] * self.W, max_rows=2, compact=True, **kw)[0]
        return out


CROSS_TF = ("beam5", "best_of5", "ragged_beam5")      # every pass has 2..32 rows per window: cross_tf_kernel


def _same_tokens(a, b, what):
    for w, (x, y) in enumerate(zip(a, b)):
        assert x.tokens == y.tokens, (what, w, x.tokens, y.tokens)


def _record_dev(a, b):
    """Largest |difference| of the per-step records of two results with identical tokens."""
    dev = 0.0
    for x, y in zip(a, b):
        assert x.tokens == y.tokens
        la, lb = np.asarray(x.token_logprobs, np.float64), np.asarray(y.token_logprobs, np.float64)
        assert la.shape == lb.shape
        if la.size:
            dev = max(dev, float(np.max(np.abs(la - lb))))
    return dev


@pytest.fixture(scope="module", params=["tiny", "base"])
def bench(request):
    return Bench(request.param)


def test_mode1_against_mode2_generate(bench):
    eng = bench.eng
    try:
        bench.load(cross_mode=0, cross_kv_fp8=1)
        r1 = bench.calls()
        bench.load(cross_kv_fp8=2)
        r2 = bench.calls()
    finally:
        eng.set_option("cross_kv_fp8", 0)
        eng.set_option("cross_mode", 1)
    assert sum(len(r.tokens) for r in r1["greedy"]) > 5 * bench.W
    for name in r1:
        _same_tokens(r1[name], r2[name], name)
        dev = _record_dev(r1[name], r2[name])
        ds = max(abs(x.score - y.score) for x, y in zip(r1[name], r2[name]))
        dn = max(abs(x.no_speech_prob - y.no_speech_prob) for x, y in zip(r1[name], r2[name]))
        print(f"{bench.dims.name} {name}: record dev {dev:.3g}, score dev {ds:.3g}, no_speech dev {dn:.3g}")
        if name in CROSS_TF:
            for x, y in zip(r1[name], r2[name]):
                assert x.score == y.score and x.cum_logprob == y.cum_logprob and x.no_speech_prob == y.no_speech_prob, name
                assert np.array_equal(x.token_logprobs, y.token_logprobs, equal_nan=True), name
                assert np.array_equal(x.token_logprobs_other, y.token_logprobs_other, equal_nan=True), name
        else:
            assert dev <= RECORD_BOUND, (name, dev)
            assert dn <= 1e-3, (name, dn)


def test_mode1_against_mode2_forward_detect_align(bench):
    """The teacher-forced entry points on projected panels: wm_forward with capture, wm_detect_language, wm_align,
    wm_align_batch and wm_align_open_batch."""
    eng, dims = bench.eng, bench.dims
    heads = dims.default_alignment_heads()
    texts = [list(range(1000 + 7 * i, 1000 + 7 * i + n)) for i, n in enumerate((5, 40, 17, 30))][:bench.W]
    frames = [3000, 2400, 3000, 1200][:bench.W]
    toks = np.asarray([bench.prompt + t[:5] for t in texts], dtype=np.int32)
    st = dims.specials
    got = {}
    try:
        for mode in (1, 2):
            bench.load(cross_mode=0, cross_kv_fp8=mode)
            logits, attn = eng.forward(list(range(bench.W)), toks, align_heads=heads[:2])
            got[mode] = dict(
                logits=logits.cpu().numpy(), attn=attn.cpu().numpy(),
                lang=eng.detect_language(list(range(bench.W)), st.sot + 1, len(st.lang_codes)),
                one=eng.align(1, bench.prompt, texts[1], frames[1], heads, 7),
                batch=eng.align_batch(list(range(bench.W)), bench.prompt, texts, frames, heads, 7),
                open=eng.align_open_batch(list(range(bench.W)), bench.prompt, texts, frames, heads, 7))
    finally:
        eng.set_option("cross_kv_fp8", 0)
        eng.set_option("cross_mode", 1)
    a, b = got[1], got[2]
    assert np.isfinite(a["logits"]).all()
    # 8 rows per window without capture-sized groups: the VALU kernels -> the record bound on logits' log-softmax
    la = torch.log_softmax(torch.from_numpy(a["logits"]), -1).numpy()
    lb = torch.log_softmax(torch.from_numpy(b["logits"]), -1).numpy()
    assert np.max(np.abs(np.take_along_axis(la, lb.argmax(-1)[..., None], -1) - lb.max(-1, keepdims=True))) <= RECORD_BOUND
    assert np.allclose(a["attn"], b["attn"], rtol=1e-4, atol=1e-7)
    assert np.allclose(a["lang"], b["lang"], rtol=1e-3, atol=1e-6)
    assert np.allclose(a["one"][0], b["one"][0], rtol=1e-3, atol=1e-6)
    # the 40-token window's pass runs on cross_tf_kernel (>= 16 rows): the same path, step for step
    assert np.array_equal(a["one"][1], b["one"][1]) and np.array_equal(a["one"][2], b["one"][2])
    for key in ("batch", "open"):
        for x, y in zip(a[key], b[key]):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]), key


def test_mode1_against_mode2_transcribe_beam5_words():
    """The worker's call (beam 5 + word timestamps) on a 70 s clip: segments, tokens and word times."""
    from vlog_amd.transcribe import WhisperModel
    model = WhisperModel("synthetic:tiny:0:margin", device="cpu", compute_type="int8")
    audio = speech_like(70.0, 321)
    out = {}
    for mode in (1, 2):
        model.engine.set_option("cross_kv_fp8", mode)
        segs, _ = model.transcribe(audio, language="en", beam_size=5, word_timestamps=True, temperature=0.0,
                                   condition_on_previous_text=False)
        out[mode] = [(s.start, s.end, tuple(s.tokens), s.avg_logprob, s.no_speech_prob,
                      tuple((w.word, w.start, w.end, w.probability) for w in s.words)) for s in segs]
        assert model.engine.option("cross_mode") == 0
    print(f"{len(out[1])} segments, {sum(len(s[5]) for s in out[1])} words")
    assert len(out[1]) >= 2 and sum(len(s[5]) for s in out[1]) >= 3
    assert out[1] == out[2]


def test_mode1_against_mode0_margin_model():
    """Identical tokens on the margin-planted model (8 windows, beam 5); the record deviation against twice what the
    factored cross_fp8 shows on the same windows (the reference for what fp8 costs here)."""
    b = Bench("tiny", seed=0, plant="margin", windows=8)
    eng, sl = b.eng, list(range(8))
    kw = dict(beam_size=5, patience=1.0, suppress_tokens=b.sup, max_length=448, record_logprobs=True)
    res = {}
    try:
        for name, opts in (("factored bf16", dict(cross_mode=1, cross_fp8=0, cross_kv_fp8=0)),
                           ("factored fp8", dict(cross_mode=1, cross_fp8=1)),
                           ("projected bf16", dict(cross_mode=0, cross_fp8=0, cross_kv_fp8=0)),
                           ("projected fp8", dict(cross_mode=0, cross_kv_fp8=1))):
            b.load(**opts)
            res[name] = eng.generate(sl, [b.prompt] * 8, **kw)[0]
    finally:
        eng.set_option("cross_fp8", 0)
        eng.set_option("cross_kv_fp8", 0)
        eng.set_option("cross_mode", 1)
    assert sum(len(r.tokens) for r in res["projected bf16"]) > 8 * 5
    _same_tokens(res["projected fp8"], res["projected bf16"], "cross_kv_fp8 1 vs 0")
    _same_tokens(res["factored fp8"], res["factored bf16"], "cross_fp8 1 vs 0")
    ref = _record_dev(res["factored fp8"], res["factored bf16"])
    dev = _record_dev(res["projected fp8"], res["projected bf16"])
    print(f"record deviation, nats: cross_kv_fp8 {dev:.6g}, factored cross_fp8 {ref:.6g}")
    assert dev <= 2 * ref, (dev, ref)


def _prefix_record_dev(a, b):
    """Largest |difference| of the per-step records over the steps both results took from the same history with the
    same token (the common token prefix of each window) -> (deviation, steps compared, windows with identical tokens)."""
    dev, steps, same = 0.0, 0, 0
    for x, y in zip(a, b):
        k = 0
        while k < min(len(x.tokens), len(y.tokens)) and x.tokens[k] == y.tokens[k]:
            k += 1
        same += x.tokens == y.tokens
        if x.tokens == y.tokens:
            k = min(len(x.token_logprobs), len(y.token_logprobs))      # the closing <|endoftext|> record too
        if k:
            la, lb = np.asarray(x.token_logprobs[:k], np.float64), np.asarray(y.token_logprobs[:k], np.float64)
            dev = max(dev, float(np.max(np.abs(la - lb))))
            steps += k
    return dev, steps, same


def test_mode1_against_mode0_small_margins():
    """The same measurement where it is not 0 against 0: the random-weight model (near-tied logits, so a chosen token's
    log-prob moves with every perturbation), 8 windows greedy, records compared over each window's common token prefix.
    The bound is the margin test's: twice what the factored cross_fp8 shows on the same windows.  DESIGN.md §4 quotes
    the two figures this prints."""
    b = Bench("tiny", seed=3, windows=8, eot_after=60)
    eng, sl = b.eng, list(range(8))
    kw = dict(suppress_tokens=b.sup, max_length=448, record_logprobs=True)
    res = {}
    try:
        for name, opts in (("factored bf16", dict(cross_mode=1, cross_fp8=0, cross_kv_fp8=0)),
                           ("factored fp8", dict(cross_mode=1, cross_fp8=1)),
                           ("projected bf16", dict(cross_mode=0, cross_fp8=0, cross_kv_fp8=0)),
                           ("projected fp8", dict(cross_mode=0, cross_kv_fp8=1))):
            b.load(**opts)
            res[name] = eng.generate(sl, [b.prompt] * 8, **kw)[0]
    finally:
        eng.set_option("cross_fp8", 0)
        eng.set_option("cross_kv_fp8", 0)
        eng.set_option("cross_mode", 1)
    ref, nref, sref = _prefix_record_dev(res["factored fp8"], res["factored bf16"])
    dev, ndev, sdev = _prefix_record_dev(res["projected fp8"], res["projected bf16"])
    print(f"small margins, record deviation in nats: cross_kv_fp8 {dev:.5f} over {ndev} steps ({sdev}/8 windows identical), "
          f"factored cross_fp8 {ref:.5f} over {nref} steps ({sref}/8 windows identical)")
    assert ndev >= 100 and nref >= 100
    assert ref > 0
    assert dev <= 2 * ref, (dev, ref)


def test_slot_memory_and_reallocation():
    b = Bench("tiny")
    eng, dims = b.eng, b.dims
    try:
        b.load(cross_mode=0)
        r0 = eng.generate(list(range(b.W)), [b.prompt] * b.W, beam_size=5, suppress_tokens=b.sup, max_length=96)[0]
        bytes0 = eng.device_bytes()                            # (after a decode: its scratch is sized)
        eng.set_option("cross_kv_fp8", 1)                      # re-allocates the slots: their content is dropped
        bytes1 = eng.device_bytes()
        bf16_slots = dims.n_dec_layer * 2 * b.W * dims.n_head * dims.n_audio_ctx * 64 * 2
        fp8_slots = bf16_slots - (bytes0 - bytes1)
        assert 0.5 * bf16_slots < fp8_slots <= 0.52 * bf16_slots, (fp8_slots, bf16_slots)      # (64 + 1) / 128
        eng.cross_kv(b.enc, 0)
        assert eng.device_bytes() > bytes1                     # the bounded staging of wm_cross_kv is counted
        r1 = eng.generate(list(range(b.W)), [b.prompt] * b.W, beam_size=5, suppress_tokens=b.sup, max_length=96)[0]
        eng.set_option("cross_kv_fp8", 0)
        assert eng.device_bytes() == bytes0
        eng.cross_kv(b.enc, 0)
        r0b = eng.generate(list(range(b.W)), [b.prompt] * b.W, beam_size=5, suppress_tokens=b.sup, max_length=96)[0]
    finally:
        eng.set_option("cross_kv_fp8", 0)
        eng.set_option("cross_mode", 1)
    for x, y in zip(r0, r0b):
        assert x.tokens == y.tokens and x.score == y.score
    from vlog_amd.engine import GpuEngine
    fresh = GpuEngine(dims, b.sd, 0)
    b.load(fresh, cross_mode=0, cross_kv_fp8=1)
    rf = fresh.generate(list(range(b.W)), [b.prompt] * b.W, beam_size=5, suppress_tokens=b.sup, max_length=96)[0]
    for x, y in zip(r1, rf):
        assert x.tokens == y.tokens and x.score == y.score and x.no_speech_prob == y.no_speech_prob


def test_option_surface(monkeypatch):
    from vlog_amd.engine import GpuEngine
    b = Bench("tiny")
    assert b.eng.option("cross_kv_fp8") == 0
    for bad in (3, -1, 100):
        with pytest.raises(RuntimeError):
            b.eng.set_option("cross_kv_fp8", bad)
    assert b.eng.option("cross_kv_fp8") == 0
    monkeypatch.setenv("VLOG_AMD_CROSS_KV_FP8", "1")
    env = GpuEngine(b.dims, b.sd, 0)
    monkeypatch.delenv("VLOG_AMD_CROSS_KV_FP8")
    assert env.option("cross_kv_fp8") == 1 and env.option("cross_fp8") == 0
    b.load(env, cross_mode=0)
    b.load(cross_mode=0, cross_kv_fp8=1)
    kw = dict(beam_size=5, suppress_tokens=b.sup, max_length=96)
    ra = env.generate(list(range(b.W)), [b.prompt] * b.W, **kw)[0]
    rb = b.eng.generate(list(range(b.W)), [b.prompt] * b.W, **kw)[0]
    for x, y in zip(ra, rb):
        assert x.tokens == y.tokens and x.score == y.score


def test_transcribe_keeps_choosing_forms():
    """With only cross_kv_fp8 on, beam search takes the projected fp8 panels and a one-row decode the factored form."""
    from vlog_amd.transcribe import WhisperModel
    model = WhisperModel("synthetic:tiny:3", device="cpu", compute_type="int8", eot_after=40)
    model.engine.set_option("cross_kv_fp8", 1)
    audio = speech_like(30.0, 5)
    segs, _ = model.transcribe(audio, language="en", beam_size=5, temperature=0.0)
    assert len(list(segs)) >= 1
    assert model.engine.option("cross_mode") == 0 and model.engine.option("cross_kv_fp8") == 1
    segs, _ = model.transcribe(audio, language="en", beam_size=1, temperature=0.0)
    assert len(list(segs)) >= 1
    assert model.engine.option("cross_mode") == 1 and model.engine.option("cross_kv_fp8") == 1
