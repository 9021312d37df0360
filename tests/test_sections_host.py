"""transcribe(sections=N) on the host: the section plan (vlog_amd.seek_state.plan_sections) and the sections of one
file driven through the lockstep scheduler with a scripted decoder.  No torch device, no engine.

plan_sections: the ranges are contiguous, cover [0, content) and are each at least 3000 frames; with VAD joins every
cut is a join with at least 0.5 s removed and a target without one loses its cut; with frame energies the cut is the
argmin within 3 s of the target with the documented tie rules; the plan depends on its arguments alone.

Scheduler: the scripted decoder of tests/test_seek_state.py (copied below: tokens are a function of (file, seek of the
window, the prompt, temperature, seed), so a window handed another section's prompt, seed or frames changes the
output).  Each section must equal oracle.transcribe.transcribe on the section's slice of the features,
feats[:, b0:b1 + 1], with b0 / 100 added to the times (sums of the same terms in another order: compared to 1e-9 s,
far below the 0.02 s step of the timestamps), and with the same (window, temperature, seed) calls."""
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import transcribe as otr
from vlog_amd.dims import N_FRAMES, model_dims
from vlog_amd.seek_state import (MAX_SECTIONS, SECTION_ENERGY_REACH_S, SECTION_JOIN_REACH, SECTION_MIN_JOIN_SILENCE_S,
                                 SeekState, chunk_joins, decode_round_with, fallback_ladder, iter_lockstep,
                                 plan_sections, run_lockstep)
from vlog_amd.tokenizer import Tokenizer

DIMS = model_dims("tiny")
ST = DIMS.specials
TEMPS = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
CONTENT = 14100                      # one 141 s file
BOUNDS = [(0, 4630), (4630, 9470), (9470, CONTENT)]
SILENT = (1, 0)          # (section, index of the window in decode order): no_speech_prob high, score low -> skipped
FALLBACK = (2, 0)        # its T = 0 result scores below the log-prob threshold; T = 0.2 is fine


# ------------------------------------------------------------------------------------------------ plan_sections
def _check_cover(bounds, content):
    assert bounds[0][0] == 0 and bounds[-1][1] == content
    assert all(a[1] == b[0] for a, b in zip(bounds[:-1], bounds[1:]))
    if len(bounds) > 1:
        assert all(e - s >= N_FRAMES for s, e in bounds), bounds


def test_thresholds_are_the_documented_ones():
    assert (SECTION_MIN_JOIN_SILENCE_S, SECTION_JOIN_REACH, SECTION_ENERGY_REACH_S, MAX_SECTIONS) == (0.5, 0.5, 3.0, 32)


@pytest.mark.parametrize("content", [1, 2999, 3000, 5999, 6000, 14100, 90000, 720000])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 16, 32])
def test_cover_and_minimum_length(content, n):
    rng = np.random.default_rng(content + n)
    joins = sorted((int(f), float(s)) for f, s in zip(rng.integers(1, max(content, 2), 40), rng.uniform(0.0, 3.0, 40)))
    energy = rng.uniform(-90.0, -10.0, content // 2 + 1)
    for kw in ({}, {"joins": joins}, {"energy": energy}):
        b = plan_sections(content, n, **kw)
        _check_cover(b, content)
        assert 1 <= len(b) <= max(1, min(n, content // N_FRAMES))
        assert b == plan_sections(content, n, **kw)                     # the same inputs, the same plan
    assert plan_sections(content, 1, joins=joins) == [(0, content)]


def test_short_files_and_bad_n():
    assert plan_sections(4000, 4) == [(0, 4000)]                        # a 40 s file at n = 4
    assert plan_sections(2000, 4, energy=np.zeros(1001)) == [(0, 2000)]
    assert plan_sections(0, 3) == [(0, 0)]
    assert plan_sections(12000, 4) == [(0, 3000), (3000, 6000), (6000, 9000), (9000, 12000)]
    assert plan_sections(11999, 4) == [(0, 4000), (4000, 7999), (7999, 11999)]      # n lowered to 3
    for n in (0, -1, 33):
        with pytest.raises(ValueError):
            plan_sections(90000, n)


def test_cuts_are_joins_with_enough_silence():
    content, n = 40000, 4                                               # targets 10000, 20000, 30000; reach 5000
    joins = [(9000, 0.4),            # nearest to 10000 but too little silence removed
             (8000, 0.5),            # qualifies (exactly the threshold)
             (12100, 2.0),           # qualifies, farther (2100 against 2000)
             (19000, 1.0), (21000, 2.5),     # a tie in distance: the longer silence wins
             (24000, 0.2), (26000, 0.1)]     # nothing qualifies near 30000: that cut is dropped
    b = plan_sections(content, n, joins=joins)
    assert b == [(0, 8000), (8000, 21000), (21000, content)]
    ok = {f for f, s in joins if s >= 0.5}
    assert {s for s, _ in b[1:]} <= ok
    # a tie in distance and silence: the lower frame
    assert plan_sections(content, 2, joins=[(21000, 1.0), (19000, 1.0)]) == [(0, 19000), (19000, content)]
    # a join farther than content / (2 n) from its target is out of reach
    assert plan_sections(content, 2, joins=[(9999, 9.0)]) == [(0, content)]
    assert plan_sections(content, 2, joins=[(10000, 9.0)]) == [(0, 10000), (10000, content)]
    # no joins at all (one speech chunk): never cut inside it
    assert plan_sections(content, 8, joins=[]) == [(0, content)]


def test_short_sections_are_merged_shortest_first():
    # cuts at 2100 and 9000 of 12100: sections 2100 / 6900 / 3100; the cut at 2100 has the shortest neighbour
    assert plan_sections(12100, 3, joins=[(2100, 1.0), (9000, 1.0)]) == [(0, 9000), (9000, 12100)]
    # 5000 | 2000 | 5000: both cuts border the short section; the lower one goes
    assert plan_sections(12000, 3, joins=[(5000, 1.0), (7000, 1.0)]) == [(0, 7000), (7000, 12000)]


def test_chunk_joins():
    chunks = [dict(start=1000, end=33000), dict(start=65000, end=100000), dict(start=100000, end=180100)]
    assert chunk_joins(chunks) == [(200, 2.0), (67000 // 160, 0.0)]
    assert chunk_joins(chunks[:1]) == [] and chunk_joins([]) == []


def test_energy_cut_is_the_argmin_within_three_seconds():
    content = 20000                                                     # n = 2: target 10000 = energy frame 5000
    e = np.full(content // 2 + 1, -30.0)
    e[4849] = -95.0                                                     # 302 mel frames before the target: out of reach
    e[4850] = -60.0                                                     # exactly 300 before: in reach
    e[5120] = -50.0
    assert plan_sections(content, 2, energy=e) == [(0, 9700), (9700, content)]
    e[5150] = -60.0                                                     # a tie at the same distance: the lower frame
    assert plan_sections(content, 2, energy=e) == [(0, 9700), (9700, content)]
    e[5100] = -60.0                                                     # a tie nearer to the target wins
    assert plan_sections(content, 2, energy=e) == [(0, 10200), (10200, content)]
    e[5151] = -99.0                                                     # 302 after the target: out of reach
    assert plan_sections(content, 2, energy=e) == [(0, 10200), (10200, content)]
    flat = np.full(content // 2 + 1, -40.0)                             # all equal: the target's own frame
    assert plan_sections(content, 2, energy=flat) == [(0, 10000), (10000, content)]
    rng = np.random.default_rng(7)
    e = rng.uniform(-80.0, -20.0, content // 2 + 1)
    for n, targets in ((2, [10000]), (4, [5000, 10000, 15000])):
        cuts = [s for s, _ in plan_sections(content, n, energy=e)[1:]]
        assert cuts == [2 * (t // 2 - 150 + int(np.argmin(e[t // 2 - 150: t // 2 + 151]))) for t in targets]


# ------------------------------------------------------------------------------------------------ scheduler
def _tok(language="en"):
    return Tokenizer(DIMS, task="transcribe", language=language, seed=3)


def _options(**kw):
    o = dict(beam_size=5, best_of=5, patience=1.0, length_penalty=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0,
             log_prob_threshold=-1.0, no_speech_threshold=0.6, compression_ratio_threshold=2.4,
             condition_on_previous_text=True, prompt_reset_on_temperature=0.5, temperatures=list(TEMPS),
             initial_prompt=None, prefix=None, suppress_blank=True, suppress_tokens=[], without_timestamps=False,
             max_initial_timestamp=1.0, word_timestamps=False, prepend_punctuations="", append_punctuations="",
             multilingual=False, max_new_tokens=None, clip_timestamps="0", hallucination_silence_threshold=None,
             hotwords=None)
    o.update(kw)
    return SimpleNamespace(**o)


def _features():
    """[n_mels, frames + 1] whose second row names the frame: a window's first column tells its absolute seek"""
    x = np.zeros((DIMS.n_mels, CONTENT + 1), np.float32)
    x[1] = np.arange(CONTENT + 1)
    return x


def _section_of(seek):
    return next(k for k, (s, e) in enumerate(BOUNDS) if s <= seek < e)


class Script:
    """The scripted decoder of tests/test_seek_state.py, keyed on the window's absolute seek.  `calls` logs
    (seek, temperature, seed, n_prompt) of every generate."""

    def __init__(self):
        self.calls = []
        self.windows = {}        # section -> seeks in decode order

    def result(self, seek, prompt, temperature, seed):
        k = _section_of(seek)
        order = self.windows.setdefault(k, [])
        if seek not in order:
            order.append(seek)
        wi = order.index(seek)
        self.calls.append((seek, temperature, seed, len(prompt)))
        h = int.from_bytes(hashlib.sha256(repr((seek, tuple(prompt), round(temperature, 3), seed)).encode()).digest()[:8],
                           "little")
        rng = np.random.default_rng(h)
        tb = ST.timestamp_begin
        n_seg = int(rng.integers(1, 4))
        toks, t = [], int(rng.integers(0, 20))
        for j in range(n_seg):
            toks.append(tb + t)
            toks.extend(int(x) for x in rng.integers(300, ST.eot - 1, size=int(rng.integers(3, 9))))
            t += int(rng.integers(100, 400))
            last_open = j == n_seg - 1 and rng.random() < 0.4
            if not last_open:
                toks.append(tb + min(t, 1500))
        score, ns = -0.3 - 0.2 * float(rng.random()), 0.05
        if (k, wi) == SILENT:
            score, ns = -1.6, 0.9
        if (k, wi) == FALLBACK and temperature == 0.0:
            score = -1.5
        return SimpleNamespace(tokens=toks, score=score, no_speech_prob=ns)

    # ---- oracle.transcribe backend
    def encode(self, window):
        return int(round(float(window[1, 0])))

    def generate(self, cross, prompt, opt):
        return self.result(cross, prompt, opt.sampling_temperature, opt.seed)


def _oracle_section(k, script):
    b0, b1 = BOUNDS[k]
    out, _ = otr.transcribe(SimpleNamespace(dims=DIMS), _tok, np.zeros(1, np.float32), beam_size=5, temperatures=TEMPS,
                            suppress_tokens=[], language="en", features=_features()[:, b0: b1 + 1], backend=script)
    for s in out:
        s["start"] += b0 / 100
        s["end"] += b0 / 100
    return out


def _same(got, ref):
    assert len(got) == len(ref), (len(got), len(ref))
    for g, r in zip(got, ref):
        assert (g["tokens"], g["temperature"], g["no_speech_prob"]) == (r["tokens"], r["temperature"], r["no_speech_prob"])
        assert abs(g["avg_logprob"] - r["avg_logprob"]) <= 1e-12
        assert abs(g["start"] - r["start"]) <= 1e-9 and abs(g["end"] - r["end"]) <= 1e-9, (g, r)


@pytest.fixture(scope="module")
def oracle_sections():
    scripts = [Script() for _ in BOUNDS]
    return [(_oracle_section(k, s), s.calls) for k, s in enumerate(scripts)]


def _drive(in_flight, driver):
    script = Script()
    results = [[] for _ in BOUNDS]
    rounds = []

    def open_section(k):
        return SeekState(CONTENT, _tok(), _options(), DIMS.n_text_ctx, clip_frames=BOUNDS[k])

    def decode_round(batch):
        rounds.append([k for k, _, _ in batch])
        assert len(batch) <= in_flight

        def first_pass(idx):
            return [script.result(batch[i][2].seek, batch[i][2].prompt, TEMPS[0], batch[i][2].window) for i in idx]

        decode_round_with(batch, first_pass,
                          lambda i, t, seed: script.result(batch[i][2].seek, batch[i][2].prompt, t, seed),
                          None, lambda k, out: results[k].extend(out))

    if driver == "run":
        assert run_lockstep(len(BOUNDS), in_flight, open_section, decode_round) == len(rounds)
    else:
        assert sum(1 for _ in iter_lockstep(len(BOUNDS), in_flight, open_section, decode_round)) == len(rounds)
    return script, results, rounds


@pytest.mark.parametrize("driver", ["run", "iter"])
@pytest.mark.parametrize("in_flight", [1, 2, 3])
def test_sections_in_lockstep_equal_oracle_per_section(oracle_sections, in_flight, driver):
    script, results, rounds = _drive(in_flight, driver)
    for k, (b0, b1) in enumerate(BOUNDS):
        ref, ref_calls = oracle_sections[k]
        _same(results[k], ref)
        assert len(ref) >= 2
        assert [s["id"] for s in results[k]] == list(range(1, len(ref) + 1))
        assert all(b0 <= s["seek"] < b1 for s in results[k])                    # seek stays the absolute frame
        # the same (window, temperature, seed) calls, with the same prompt lengths
        assert [c for c in script.calls if b0 <= c[0] < b1] == ref_calls, k
        assert ref_calls[0][2] == 0 and ref_calls[0][3] == len(_tok().sot_sequence)   # window 0, no previous text
    assert sorted(script.windows) == [0, 1, 2] and all(len(w) >= 2 for w in script.windows.values())
    assert any(c[3] > len(_tok().sot_sequence) for c in script.calls)          # later windows carry previous text
    if in_flight >= len(BOUNDS):
        assert len(rounds) == max(len(w) for w in script.windows.values())
    if in_flight == 1:
        assert len(rounds) == sum(len(w) for w in script.windows.values())
        assert [r[0] for r in rounds] == sorted(r[0] for r in rounds)           # one section after another
    # the script did what it says: a skipped window, and one fallback with seed window + 1
    first1, first2 = script.windows[SILENT[0]][0], script.windows[FALLBACK[0]][0]
    assert [c[1] for c in script.calls if c[0] == first1] == [0.0]
    assert [(c[1], c[2]) for c in script.calls if c[0] == first2] == [(0.0, 0), (0.2, 1)]


def _run_state(state, script):
    out = []
    while (req := state.next_request()) is not None:
        out.extend(state.consume(fallback_ladder(lambda t, seed: script.result(req.seek, req.prompt, t, seed),
                                                 state.tokenizer.decode, state.options, seed=req.window)))
    return out


@pytest.mark.parametrize("k", range(len(BOUNDS)))
def test_clip_frames_equals_clip_timestamps(k):
    b0, b1 = BOUNDS[k]
    assert (round(b0 / 100 * 100), round(b1 / 100 * 100)) == (b0, b1)
    a, b = Script(), Script()
    got = _run_state(SeekState(CONTENT, _tok(), _options(), DIMS.n_text_ctx, clip_frames=(b0, b1)), a)
    ref = _run_state(SeekState(CONTENT, _tok(), _options(clip_timestamps=[b0 / 100, b1 / 100]), DIMS.n_text_ctx), b)
    assert got and got == ref and a.calls == b.calls


def test_prefix_on_the_first_section_only_and_initial_prompt_on_all():
    opts = _options(prefix="hello", initial_prompt=[301, 302, 303])
    n_sot = len(_tok().sot_sequence)
    first = []
    for b in BOUNDS:
        req = SeekState(CONTENT, _tok(), opts, DIMS.n_text_ctx, clip_frames=b).next_request()
        assert req.window == 0 and req.seek == b[0]
        first.append(len(req.prompt))
    assert first[1] == first[2] == 1 + 3 + n_sot and first[0] > first[1]
