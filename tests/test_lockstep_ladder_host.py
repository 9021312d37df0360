"""The fallback ladder decoded by LEVELS (vlog_amd/seek_state.py FallbackLadder, decode_round_levels), on the CPU with
the scripted decoder of tests/test_seek_state.py: no torch device, no engine.

The script here adds scores: per (file, window) the number of temperatures whose result scores below the log-prob
threshold, so several windows fail several levels, one fails all six (the "best of all" branch) and most pass at once.
Every file's segments must equal oracle.transcribe.transcribe driven by the same script, and the call log must show
one level_pass per round and level, holding exactly the entries still failing, with the seeds window + level."""
from types import SimpleNamespace

import pytest

from vlog_amd import segments as segs
from vlog_amd.seek_state import (ACCEPTED, EXHAUSTED, NEXT, FallbackLadder, SeekState, decode_round_levels,
                                 decode_round_with, fallback_ladder, run_lockstep)

from tests.test_seek_state import DIMS, FRAMES, TEMPS, Script, _key, _options, _oracle, _tok

# (file, index of the window in decode order) -> temperatures that fail, from the first on
FAILS = {(0, 0): 2, (0, 1): 6, (1, 0): 1, (2, 1): 3, (3, 0): 1, (4, 0): 4, (4, 1): 2}


class LadderScript(Script):
    """tests/test_seek_state.py Script whose results fail the log-prob threshold at the first FAILS[(file, window)]
    temperatures (the scores differ per level, so the "all failed" branch has a best one to pick)."""

    def result(self, f, seek, prompt, temperature, seed):
        r = super().result(f, seek, prompt, temperature, seed)
        wi = self.windows[f].index(seek)
        level = TEMPS.index(temperature)
        if level < FAILS.get((f, wi), 0):
            # below log_prob_threshold -1.0 whatever the token count: avg = score * n / (n + 1), n >= 5
            r.score = -2.0 - 0.1 * ((level * 7 + f + wi) % 5)
        return r


def _old_fallback_ladder(generate, decode_text, options, seed=0, first=None):
    """a literal copy of fallback_ladder as it was before it became a loop over FallbackLadder"""
    all_results, below_cr = [], []
    decode_result = None
    temperature = options.temperatures[0] if options.temperatures else 0.0
    for i, temperature in enumerate(options.temperatures):
        result = first if (i == 0 and first is not None) else generate(temperature, seed + i)
        n = len(result.tokens)
        avg_lp = segs.avg_logprob(result.score, n, options.length_penalty)
        text = decode_text(result.tokens).strip()
        cr = segs.compression_ratio(text)
        decode_result = (result, avg_lp, temperature, cr)
        all_results.append(decode_result)
        fb, below = segs.needs_fallback(cr, avg_lp, result.no_speech_prob, options.compression_ratio_threshold,
                                        options.log_prob_threshold, options.no_speech_threshold)
        if below:
            below_cr.append(decode_result)
        if not fb:
            break
    else:
        best = max(below_cr or all_results, key=lambda x: x[1])
        decode_result = (best[0], best[1], temperature, best[3])
    return decode_result


def _run_levels(max_files, temperatures=TEMPS):
    """run_lockstep over the five files with decode_round_levels -> (results per file, script, log) where log holds
    one ("first", round, files) and one ("level", round, temperature, [(file, window, seed)]) per call"""
    n = len(FRAMES)
    script = LadderScript()
    results = [[] for _ in range(n)]
    log = []
    rounds = [0]

    def decode_round(batch):
        rnd = rounds[0]
        rounds[0] += 1

        def first_pass(idx):
            log.append(("first", rnd, [batch[i][0] for i in idx]))
            return [script.result(batch[i][0], batch[i][2].seek, batch[i][2].prompt, temperatures[0], batch[i][2].window)
                    for i in idx]

        def level_pass(idx, temperature, seeds):
            assert len(idx) == len(seeds) and idx == sorted(idx)            # batch order
            log.append(("level", rnd, temperature, [(batch[i][0], batch[i][2].window, s) for i, s in zip(idx, seeds)]))
            return [script.result(batch[i][0], batch[i][2].seek, batch[i][2].prompt, temperature, s)
                    for i, s in zip(idx, seeds)]

        decode_round_levels(batch, first_pass, level_pass, None, lambda f, out: results[f].extend(out))

    run_lockstep(n, max_files, lambda f: SeekState(FRAMES[f], _tok(), _options(temperatures=list(temperatures)),
                                                   DIMS.n_text_ctx), decode_round)
    return results, script, log


@pytest.mark.parametrize("max_files", [1, 2, 5])
def test_levels_equal_oracle_per_file(max_files):
    results, script, log = _run_levels(max_files)
    for f in range(len(FRAMES)):
        ref_script = LadderScript()
        ref = _oracle(f, ref_script)
        assert _key(results[f]) == _key(ref), (max_files, f)
        assert [s["id"] for s in results[f]] == list(range(1, len(ref) + 1))
        # the same decodes as the one-file loop made for this file: windows, temperatures, seeds, prompt lengths
        assert sorted(c for c in script.calls if c[0] == f) == sorted(ref_script.calls), (max_files, f)
    temps = {s["temperature"] for r in results for s in r}
    assert {0.0, 0.2, 0.4, 0.8, 1.0} <= temps, temps          # several depths, the exhausted ladder included


@pytest.mark.parametrize("max_files", [1, 2, 5])
def test_call_log_one_level_pass_per_round_and_level(max_files):
    results, script, log = _run_levels(max_files)
    n_rounds = 1 + max(e[1] for e in log)
    seen_fallback = 0
    for rnd in range(n_rounds):
        firsts = [e for e in log if e[0] == "first" and e[1] == rnd]
        assert len(firsts) == 1
        files = firsts[0][2]
        levels = [e for e in log if e[0] == "level" and e[1] == rnd]
        # exactly one level_pass per level that some entry needs, in ladder order
        assert [e[2] for e in levels] == list(TEMPS[1:1 + len(levels)])
        for li, e in enumerate(levels, start=1):
            entries = e[3]
            # its seeds are window + level
            assert all(seed == window + li for _, window, seed in entries), (rnd, li, entries)
            # its entries are entries of this round, each once, in batch order (which ones: checked against the
            # script below, per window)
            got = [f for f, _, _ in entries]
            assert got == [f for f in files if f in got]
            seen_fallback += len(entries)
        # every entry of the round: re-decoded at level li iff it failed levels 0 .. li - 1, never after it passed
        for f in files:
            in_levels = [li for li, e in enumerate(levels, start=1) if f in [x[0] for x in e[3]]]
            assert in_levels == list(range(1, len(in_levels) + 1)), (rnd, f, in_levels)
    # against the script: per (file, window) the temperatures decoded are exactly 0 .. min(FAILS, 5), each once
    for f, order in script.windows.items():
        for wi, seek in enumerate(order):
            ts = [c[2] for c in script.calls if c[0] == f and c[1] == seek]
            depth = min(FAILS.get((f, wi), 0), len(TEMPS) - 1)
            if (f, wi) == (2, 0):               # test_seek_state.SILENT: skipped as silence, no fallback
                depth = 0
            if (f, wi) == (3, 0):               # test_seek_state.FALLBACK fails T = 0 by itself
                depth = max(depth, 1)
            assert ts == list(TEMPS[:depth + 1]), (f, wi, ts)
    assert seen_fallback == sum(len(e[3]) for e in log if e[0] == "level") > 0
    if max_files == 5:
        # the first round holds all five files; its levels shrink as entries are accepted
        lv0 = [e for e in log if e[0] == "level" and e[1] == 0]
        assert [[f for f, _, _ in e[3]] for e in lv0] == [[0, 1, 3, 4], [0, 4], [4], [4]]


def test_one_temperature_makes_no_level_call():
    results, script, log = _run_levels(5, temperatures=(0.0,))
    assert not [e for e in log if e[0] == "level"]
    assert all(c[2] == 0.0 for c in script.calls)
    for f in range(len(FRAMES)):
        state = SeekState(FRAMES[f], _tok(), _options(temperatures=[0.0]), DIMS.n_text_ctx)
        solo, ref = LadderScript(), []
        while (req := state.next_request()) is not None:
            ref.extend(state.consume(_old_fallback_ladder(lambda t, seed: solo.result(f, req.seek, req.prompt, t, seed),
                                                          state.tokenizer.decode, state.options, seed=req.window)))
        assert _key(results[f]) == _key(ref)


@pytest.mark.parametrize("with_first", [False, True])
def test_fallback_ladder_over_the_resumable_form_is_unchanged(with_first):
    tok = _tok()
    for f in range(len(FRAMES)):
        for wi in range(2):
            opts = _options()
            seek, prompt, window = 3000 * wi, list(tok.sot_sequence), wi
            a, b = LadderScript(), LadderScript()
            for s in (a, b):
                s.windows[f] = [0, 3000][:wi + 1]
            fa = a.result(f, seek, prompt, TEMPS[0], window) if with_first else None
            fb = b.result(f, seek, prompt, TEMPS[0], window) if with_first else None
            new = fallback_ladder(lambda t, sd: a.result(f, seek, prompt, t, sd), tok.decode, opts, seed=window, first=fa)
            old = _old_fallback_ladder(lambda t, sd: b.result(f, seek, prompt, t, sd), tok.decode, opts, seed=window,
                                       first=fb)
            assert a.calls == b.calls, (f, wi)
            assert (new[0].tokens, new[0].score, new[1], new[2], new[3]) == (old[0].tokens, old[0].score, old[1], old[2],
                                                                             old[3]), (f, wi)
    # the window that fails all six: the best of all results, reported at the last temperature
    s = LadderScript()
    s.windows[0] = [0, 3000]
    r = fallback_ladder(lambda t, sd: s.result(0, 3000, list(tok.sot_sequence), t, sd), tok.decode, _options(), seed=1)
    assert [c[2] for c in s.calls] == list(TEMPS) and [c[3] for c in s.calls] == [1, 2, 3, 4, 5, 6]
    assert r[2] == TEMPS[-1]


def test_ladder_states():
    tok = _tok()
    good = SimpleNamespace(tokens=[400, 401, 402, 403, 404], score=-0.2, no_speech_prob=0.05)
    bad = SimpleNamespace(tokens=[400, 401, 402, 403, 404], score=-3.0, no_speech_prob=0.05)
    ladder = FallbackLadder(tok.decode, _options(), seed=7)
    assert ladder.request() == (0.0, 7) and not ladder.done
    assert ladder.judge(bad) == NEXT and ladder.request() == (0.2, 8)
    with pytest.raises(RuntimeError):
        ladder.result()
    assert ladder.judge(good) == ACCEPTED and ladder.done and ladder.result()[2] == 0.2
    with pytest.raises(RuntimeError):
        ladder.judge(good)
    ladder = FallbackLadder(tok.decode, _options(temperatures=[0.0, 0.4]), seed=0)
    assert ladder.judge(bad) == NEXT and ladder.judge(bad) == EXHAUSTED and ladder.result()[2] == 0.4


def test_levels_and_solo_drivers_agree_on_the_script():
    """decode_round_levels against decode_round_with (the driver in use today) on the same script"""
    n = len(FRAMES)
    levels, _, _ = _run_levels(2)
    script = LadderScript()
    solo = [[] for _ in range(n)]

    def decode_round(batch):
        decode_round_with(batch,
                          lambda idx: [script.result(batch[i][0], batch[i][2].seek, batch[i][2].prompt, 0.0, batch[i][2].window)
                                       for i in idx],
                          lambda i, t, seed: script.result(batch[i][0], batch[i][2].seek, batch[i][2].prompt, t, seed),
                          None, lambda f, out: solo[f].extend(out))

    run_lockstep(n, 2, lambda f: SeekState(FRAMES[f], _tok(), _options(), DIMS.n_text_ctx), decode_round)
    for f in range(n):
        assert _key(levels[f]) == _key(solo[f]), f
