"""wm_generate_seeded (GpuEngine.generate(seeds=...)): one sampling seed per window, so a window draws the Gumbel
noise of (its own seed, its hypothesis' index inside the window) wherever it stands in the call.

The check is the one of tests/test_gpu_sampling.py: teacher-force the GPU's tokens through the CPU oracle and compare
every chosen token's key with the best key at its step under the noise the engine must have used (`_key_margins`, 0.02
nats of bf16 logit noise at a near-tie).  Here the noise is gumbel_noise(seeds[w], j, step, V) with j < num_hypotheses;
the negative control holds the same tokens against the noise of today's keying (seeds[w], w * nh + j) and against
another seed, which miss by many nats at their worst step (the oracle alone gives -10.9 to -15.4 nats for these four
windows and seeds at T 0.4 and 1.0, and exactly 0.0 under the own keying)."""
import numpy as np
import pytest
import torch

from oracle import mel as omel
from oracle.decode import GenerateOptions
from oracle.model import OracleWhisper
from vlog_amd import segments as segs
from vlog_amd.audio import speech_like
from vlog_amd.dims import model_dims
from vlog_amd.tokenizer import Tokenizer
from vlog_amd.weights import round_bf16, synthetic_state_dict

from tests.parity_util import GATE_CUM_REL
from tests.test_gpu_sampling import EPS, _key_margins

pytestmark = pytest.mark.gpu

W = 4
NH = 3
ML = 120
SEEDS = [11, 7, 11, 2 ** 40 + 5]        # windows 0 and 2 share a seed: only the place in the call would tell them apart
WRONG = -5.0                            # nats: a token chosen under other noise misses its best key by far more


class _Oracle:
    """The oracle's teacher-forced decode, computed once per (sequence, window) and shared by every check."""

    def __init__(self, orc):
        self.orc = orc
        self.memo = {}

    def decode(self, tokens, cross):
        key = (np.asarray(tokens).tobytes(), id(cross))
        if key not in self.memo:
            self.memo[key] = (self.orc.decode(tokens, cross), cross)     # (cross is kept alive: its id is the key)
        return self.memo[key][0]


@pytest.fixture(scope="module")
def setup():
    from vlog_amd.engine import GpuEngine
    dims = model_dims("tiny")
    sd = synthetic_state_dict(dims, seed=3, eot_after=60)
    eng = GpuEngine(dims, sd, 0)
    orc = OracleWhisper(round_bf16(sd), dims, np.float32, bf16_acts=True)
    x = np.concatenate([speech_like(30.0, 800 + i) for i in range(W)])
    feats = omel.log_mel(x, dims.n_mels)
    enc = eng.encode(torch.from_numpy(feats).cuda(), [3000 * i for i in range(W)], [3000] * W)
    eng.reserve(W, 16)
    eng.cross_kv(enc, 0)
    encf = enc.float().cpu().numpy()
    cross = [orc.cross_kv(encf[w: w + 1]) for w in range(W)]
    st = dims.specials
    prompt = [st.sot, st.lang_token("en"), st.transcribe]
    sup = [st.transcribe, st.translate, st.sot, st.sot_prev, st.sot_lm]
    return dims, eng, _Oracle(orc), encf, cross, prompt, sup


def _worst(orc, cross, prompt, tokens, st, sup, T, seed, hyps, ml=ML):
    """the worst step's key margin of `tokens` under the noise of (seed, hyp), for the best hyp of `hyps`"""
    opt = GenerateOptions(suppress_tokens=sup, max_length=ml, sampling_temperature=T, num_hypotheses=len(hyps), seed=seed)
    ended = len(prompt) + len(tokens) < ml
    return max(float(_key_margins(orc, cross, prompt, tokens, st, opt, h, ended)[:, 0].min()) for h in hyps)


@pytest.fixture(scope="module")
def seeded(setup):
    """the seeded call over the four windows, per temperature (shared by the tests that only read it)"""
    dims, eng, orc, encf, cross, prompt, sup = setup
    out = {}
    for T in (0.4, 1.0):
        out[T], _ = eng.generate(list(range(W)), [prompt] * W, temperature=T, num_hypotheses=NH, seeds=SEEDS,
                                 suppress_tokens=sup, max_length=ML)
    return out


@pytest.mark.parametrize("T", [0.4, 1.0])
def test_own_keying(setup, seeded, T):
    dims, eng, orc, encf, cross, prompt, sup = setup
    st = dims.specials
    plain, _ = eng.generate(list(range(W)), [prompt] * W, temperature=T, num_hypotheses=NH, seed=11,
                            suppress_tokens=sup, max_length=ML)
    for w in range(W):
        r = seeded[T][w]
        assert r.tokens
        m = _worst(orc, cross[w], prompt, r.tokens, st, sup, T, SEEDS[w], range(NH))
        print(f"T={T} window {w}: worst own-key margin {m:.4f} nats over {len(r.tokens)} tokens")
        assert m >= -EPS, (w, m, len(r.tokens))
        assert abs(r.no_speech_prob - plain[w].no_speech_prob) < 1e-3


@pytest.mark.parametrize("T", [0.4, 1.0])
def test_negative_control(setup, seeded, T):
    dims, eng, orc, encf, cross, prompt, sup = setup
    st = dims.specials
    for w in range(1, W):
        toks = seeded[T][w].tokens
        place = _worst(orc, cross[w], prompt, toks, st, sup, T, SEEDS[w], range(w * NH, (w + 1) * NH))
        other = _worst(orc, cross[w], prompt, toks, st, sup, T, 5, range(NH))
        print(f"T={T} window {w}: keyed on its place {place:.2f} nats, on seed 5 {other:.2f} nats")
        assert place < WRONG and other < WRONG, (w, place, other)


def _bits(res):
    return [(r.tokens, np.float32(r.score).tobytes(), np.float32(r.cum_logprob).tobytes(),
             np.float32(r.no_speech_prob).tobytes()) for r in res]


def test_null_and_greedy_equivalence(setup):
    dims, eng, orc, encf, cross, prompt, sup = setup
    kw = dict(suppress_tokens=sup, max_length=ML)
    a, _ = eng.generate(list(range(W)), [prompt] * W, temperature=0.4, num_hypotheses=NH, seed=11, seeds=None, **kw)
    b, _ = eng.generate(list(range(W)), [prompt] * W, temperature=0.4, num_hypotheses=NH, seed=11, **kw)
    assert _bits(a) == _bits(b)
    for beam in (1, 5):
        a, _ = eng.generate(list(range(W)), [prompt] * W, temperature=0.0, beam_size=beam, seeds=SEEDS, **kw)
        b, _ = eng.generate(list(range(W)), [prompt] * W, temperature=0.0, beam_size=beam, **kw)
        assert _bits(a) == _bits(b), beam
    with pytest.raises(ValueError):
        eng.generate(list(range(W)), [prompt] * W, temperature=0.4, seeds=SEEDS[:2], **kw)
    # seeds are taken mod 2^64, like `seed`
    a, _ = eng.generate([1], [prompt], temperature=0.4, num_hypotheses=NH, seeds=[7 + 2 ** 64], **kw)
    b, _ = eng.generate([1], [prompt], temperature=0.4, num_hypotheses=NH, seeds=[7], **kw)
    assert _bits(a) == _bits(b)


def test_one_window_equals_the_call_seed(setup):
    dims, eng, orc, encf, cross, prompt, sup = setup
    for w in range(W):
        a, _ = eng.generate([w], [prompt], temperature=0.4, num_hypotheses=NH, seeds=[SEEDS[w]], suppress_tokens=sup,
                            max_length=ML)
        b, _ = eng.generate([w], [prompt], temperature=0.4, num_hypotheses=NH, seed=SEEDS[w], suppress_tokens=sup,
                            max_length=ML)
        assert _bits(a) == _bits(b), w


def test_place_in_the_call(setup, seeded):
    dims, eng, orc, encf, cross, prompt, sup = setup
    order = [2, 0, 3, 1]
    res, _ = eng.generate(order, [prompt] * W, temperature=0.4, num_hypotheses=NH, seeds=[SEEDS[w] for w in order],
                          suppress_tokens=sup, max_length=ML)
    for k, w in enumerate(order):
        ref = seeded[0.4][w]
        assert res[k].tokens == ref.tokens, (k, w)
        assert abs(res[k].cum_logprob - ref.cum_logprob) / max(1.0, abs(ref.cum_logprob)) <= GATE_CUM_REL, (k, w)


def test_row_set_form(setup):
    dims, eng, orc, encf, cross, prompt, sup = setup
    st = dims.specials
    stats = {}
    res, _ = eng.generate(list(range(W)), [prompt] * W, temperature=0.4, num_hypotheses=1, seeds=SEEDS, max_rows=2,
                          suppress_tokens=sup, max_length=ML, stats=stats)
    assert stats["refills"] > 0, stats
    for w in range(W):
        m = _worst(orc, cross[w], prompt, res[w].tokens, st, sup, 0.4, SEEDS[w], [0])
        print(f"row set window {w}: worst own-key margin {m:.4f} nats over {len(res[w].tokens)} tokens")
        assert m >= -EPS, (w, m)
    # the compacting form reads the same tables
    res_c, _ = eng.generate(list(range(W)), [prompt] * W, temperature=0.4, num_hypotheses=1, seeds=SEEDS, compact=True,
                            suppress_tokens=sup, max_length=ML)
    for w in range(W):
        m = _worst(orc, cross[w], prompt, res_c[w].tokens, st, sup, 0.4, SEEDS[w], [0])
        assert m >= -EPS, (w, m)


def test_ragged_prompts(setup):
    dims, eng, orc, encf, cross, prompt, sup = setup
    st = dims.specials
    tok = Tokenizer(dims, task="transcribe", language="en", seed=3)
    prev = [int(t) for t in np.random.default_rng(41).integers(300, st.eot - 1, size=20)]
    long = segs.build_prompt(tok.encode, tok.sot_sequence, tok.sot_prev, tok.no_timestamps, tok.timestamp_begin,
                             dims.n_text_ctx, prev, False, None, None)
    assert long[-len(prompt):] == prompt and len(long) == len(prompt) + 21      # <|startofprev|>, 20 tokens, the sot sequence
    prompts = [prompt, long]
    mls = [ML, len(long) + ML - len(prompt)]
    res, _ = eng.generate([0, 1], prompts, temperature=0.4, num_hypotheses=NH, seeds=[SEEDS[3], SEEDS[1]],
                          suppress_tokens=sup, max_length=mls)
    for w, seed in enumerate((SEEDS[3], SEEDS[1])):
        m = _worst(orc, cross[w], prompts[w], res[w].tokens, st, sup, 0.4, seed, range(NH), ml=mls[w])
        print(f"ragged window {w}: worst own-key margin {m:.4f} nats over {len(res[w].tokens)} tokens")
        assert m >= -EPS, (w, m)


def test_projected_form(setup):
    """cross_mode 0 with best_of 5: what the product runs for best-of groups"""
    dims, eng, orc, encf, cross, prompt, sup = setup
    st = dims.specials
    nh, nw = 5, 3
    enc = torch.from_numpy(encf).to(torch.bfloat16).cuda()
    eng.set_option("cross_mode", 0)
    try:
        eng.reserve(W, W * nh)
        eng.cross_kv(enc, 0)
        res, _ = eng.generate(list(range(nw)), [prompt] * nw, temperature=0.4, num_hypotheses=nh, seeds=SEEDS[1:1 + nw],
                              suppress_tokens=sup, max_length=ML)
    finally:
        eng.set_option("cross_mode", 1)
        eng.cross_kv(enc, 0)
    for w in range(nw):
        m = _worst(orc, cross[w], prompt, res[w].tokens, st, sup, 0.4, SEEDS[1 + w], range(nh))
        print(f"projected window {w}: worst own-key margin {m:.4f} nats over {len(res[w].tokens)} tokens")
        assert m >= -EPS, (w, m)
