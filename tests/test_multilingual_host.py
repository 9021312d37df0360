"""multilingual=True on the host (vlog_amd/seek_state.py and the option's plumbing), on the CPU with a scripted
decoder: no torch device, no engine.

The script's first-pass result names the language of each window, `en, es, es, en` over four windows, as the engine's
multilingual call does (the `language` of the decode callable's result); the second window fails temperature 0 and needs
the fallback ladder.  Checked: the prompt handed to every fallback temperature carries the window's language token; the
next window's placeholder is the previous window's language (the file's on the first window); the alignment callable
receives that language's tokenizer, so its sot sequence; the emitted segments carry `language`; an English-only tokenizer
turns the option off; and with the option off requests and results are today's.  The alignment of a lockstep round
with the option on is grouped by language: ONE call per distinct language among the round's items, every item with its
own last-speech time; a round without the option keeps its one call per item.
"""
import hashlib
import logging
from types import SimpleNamespace

import numpy as np
import pytest

from vlog_amd.dims import model_dims
from vlog_amd.seek_state import SeekState, decode_round_levels, decode_round_with, fallback_ladder, run_lockstep
from vlog_amd.tokenizer import Tokenizer

DIMS = model_dims("tiny")
ST = DIMS.specials
TEMPS = (0.0, 0.2, 0.4)
LANGS = ["en", "es", "es", "en"]      # what the first pass detects, per window
FALLBACK = 1                          # the window whose temperature-0 result fails the log-prob threshold
FAIL_TWICE = 2                        # ... and one that fails 0.0 and 0.2 (round drivers only)


def _tok(dims=DIMS, language="en"):
    return Tokenizer(dims, task="transcribe", language=language, seed=3)


def _options(**kw):
    o = dict(beam_size=5, best_of=5, patience=1.0, length_penalty=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0,
             log_prob_threshold=-1.0, no_speech_threshold=0.6, compression_ratio_threshold=2.4,
             condition_on_previous_text=True, prompt_reset_on_temperature=0.5, temperatures=list(TEMPS),
             initial_prompt=None, prefix=None, suppress_blank=True, suppress_tokens=[], without_timestamps=True,
             max_initial_timestamp=1.0, word_timestamps=True, prepend_punctuations="", append_punctuations="",
             multilingual=True, max_new_tokens=None, clip_timestamps="0", hallucination_silence_threshold=None,
             hotwords=None)
    o.update(kw)
    return SimpleNamespace(**o)


class Script:
    """The scripted backend: tokens are a function of (window key, prompt, temperature, seed); `log` keeps every call's
    (kind, window key, temperature, prompt copy)."""

    def __init__(self, fail=((FALLBACK, 1),), name_language=True, langs=LANGS):
        self.fail = dict(fail)            # window key -> temperatures (from the first) that fail
        self.name_language = name_language
        self.langs = list(langs)
        self.log = []
        self.aligned = []                 # (window key, language code, sot sequence) per align call
        self.group_calls = []             # per grouped align call: (language code, sot sequence, [(key, last)])

    def result(self, key, prompt, temperature, seed, first):
        self.log.append(("first" if first else "fallback", key, temperature, list(prompt)))
        h = hashlib.sha256(repr((key, tuple(prompt), round(temperature, 3), seed)).encode()).digest()
        rng = np.random.default_rng(int.from_bytes(h[:8], "little"))
        toks = [int(x) for x in rng.integers(300, ST.eot - 1, size=int(rng.integers(4, 9)))]
        failing = TEMPS.index(temperature) < self.fail.get(key, 0)
        r = SimpleNamespace(tokens=toks, score=-1.5 if failing else -0.3, no_speech_prob=0.05)
        if first and self.name_language:
            r.language = self.langs[key]
        return r

    def align(self, key, current, size, last, tokenizer=None):
        self.aligned.append((key, tokenizer.language_code if tokenizer else None,
                             list(tokenizer.sot_sequence) if tokenizer else None))
        for s in current:
            s["words"] = []
        return last

    def align_group(self, items):
        tk = items[0][4]
        assert all(it[4] is tk or list(it[4].sot_sequence) == list(tk.sot_sequence) for it in items)
        self.group_calls.append((tk.language_code, list(tk.sot_sequence), [(it[0], it[3]) for it in items]))
        for it in items:
            for s in it[1]:
                s["words"] = []
        return [100.0 + it[0] for it in items]          # a last-speech time of its own per item


def _drive_one(script, options, tokenizer=None):
    """one file of four 30 s windows, as WhisperModel.generate_segments runs the state with the option on"""
    state = SeekState(12000, tokenizer or _tok(), options, DIMS.n_text_ctx)
    out, requests = [], []
    while True:
        req = state.next_request()
        if req is None:
            return state, requests, out
        key = req.seek // 3000
        requests.append((req.language, req.lang_pos, list(req.prompt)))
        first = script.result(key, req.prompt, options.temperatures[0], req.window, True)
        state.set_window_language(getattr(first, "language", None))
        decode = fallback_ladder(lambda t, seed: script.result(key, req.prompt, t, seed, False), state.tokenizer.decode,
                                 options, seed=req.window, first=first)
        out.extend(state.consume(decode, lambda cur, size, last, **kw: script.align(key, cur, size, last, **kw)))


def _lang_token(code):
    return ST.lang_token(code)


def test_one_file_loop():
    script = Script()
    state, requests, out = _drive_one(script, _options())
    assert state.multilingual and len(requests) == 4
    # the placeholder: the file's language on the first window, then the previous window's
    assert [r[0] for r in requests] == ["en", "en", "es", "es"]
    for placeholder, pos, prompt in requests:
        assert prompt[pos - 1] == ST.sot and prompt[pos] == _lang_token(placeholder)
    assert requests[0][1] == 1 and requests[1][1] > 1            # previous text moves the position
    # every fallback temperature of the failing window decodes with its own language's token, not the placeholder's
    fallbacks = [c for c in script.log if c[0] == "fallback"]
    assert [(c[1], c[2]) for c in fallbacks] == [(FALLBACK, 0.2)]
    pos = requests[FALLBACK][1]
    assert requests[FALLBACK][2][pos] == _lang_token("en") and fallbacks[0][3][pos] == _lang_token("es")
    assert fallbacks[0][3][:pos] == requests[FALLBACK][2][:pos] and fallbacks[0][3][pos + 1:] == requests[FALLBACK][2][pos + 1:]
    # alignment under the window's language
    assert [(k, c) for k, c, _ in script.aligned] == list(enumerate(LANGS))
    for _, code, sot in script.aligned:
        assert sot == [ST.sot, _lang_token(code), ST.transcribe]
    # the segments carry the language; the fallback window reports its temperature
    assert [s["language"] for s in out] == LANGS and [s["temperature"] for s in out] == [0.0, 0.2, 0.0, 0.0]
    assert state.language == "en"


def _round_run(driver, script, options_of, n=4, grouped=True):
    """n files of one window each in ONE lockstep round (entry i = window key i), through decode_round_with or
    decode_round_levels; -> (requests at first-pass time, emitted segments per file)"""
    states, emitted, seen = {}, {f: [] for f in range(n)}, {}

    def open_file(f):
        states[f] = SeekState(3000, _tok(), options_of(f), DIMS.n_text_ctx)
        return states[f]

    def decode_round(batch):
        def first_pass(idx):
            for i in idx:
                seen[i] = (batch[i][2].language, batch[i][2].lang_pos, list(batch[i][2].prompt))
            return [script.result(i, batch[i][2].prompt, TEMPS[0], batch[i][2].window, True) for i in idx]

        def fallback_generate(i, t, seed):
            return script.result(i, batch[i][2].prompt, t, seed, False)

        def level_pass(idx, t, seeds):
            return [script.result(i, batch[i][2].prompt, t, sd, False) for i, sd in zip(idx, seeds)]

        emit = lambda f, segs: emitted[f].extend(segs)
        if driver is decode_round_levels:
            decode_round_levels(batch, first_pass, level_pass, script.align, emit,
                                script.align_group if grouped else None)
        else:
            decode_round_with(batch, first_pass, fallback_generate, script.align, emit,
                              script.align_group if grouped else None)

    assert run_lockstep(n, n, open_file, decode_round) == 1
    return states, seen, emitted


@pytest.mark.parametrize("driver", [decode_round_with, decode_round_levels], ids=["solo_fallback", "levels"])
def test_lockstep_round(driver):
    script = Script(fail=((FALLBACK, 1), (FAIL_TWICE, 2)))
    states, seen, emitted = _round_run(driver, script, lambda f: _options())
    assert all(seen[i][0] == "en" and seen[i][2][seen[i][1]] == _lang_token("en") for i in range(4))
    # the fallback passes (solo, or by levels) receive prompts that carry each window's language
    fallbacks = [c for c in script.log if c[0] == "fallback"]
    assert sorted((c[1], c[2]) for c in fallbacks) == [(FALLBACK, 0.2), (FAIL_TWICE, 0.2), (FAIL_TWICE, 0.4)]
    for _, key, _, prompt in fallbacks:
        assert prompt[seen[key][1]] == _lang_token(LANGS[key]) == _lang_token("es")
    # the shared pass aligns by language: ONE call per distinct language among the four items, under that language's
    # sot sequence, the items in batch order, each with its own last-speech time in and out; no per-item call
    assert script.aligned == []
    assert [(code, [k for k, _ in items]) for code, _, items in script.group_calls] == [("en", [0, 3]), ("es", [1, 2])]
    for code, sot, items in script.group_calls:
        assert sot == [ST.sot, _lang_token(code), ST.transcribe] and all(last == 0.0 for _, last in items)
    for f in range(4):
        assert emitted[f] and all(s["language"] == LANGS[f] and s["words"] == [] for s in emitted[f])
        assert states[f].language == LANGS[f] and states[f].last_speech_timestamp == 100.0 + f
    assert [emitted[f][0]["temperature"] for f in range(4)] == [0.0, 0.2, 0.4, 0.0]
    # a driver without a grouped aligner keeps one call per item, each under its own language, and emits the same
    script1 = Script(fail=((FALLBACK, 1), (FAIL_TWICE, 2)))
    _, _, emitted1 = _round_run(driver, script1, lambda f: _options(), grouped=False)
    assert sorted((k, c) for k, c, _ in script1.aligned) == list(enumerate(LANGS)) and script1.group_calls == []
    assert emitted1 == emitted and script1.log == script.log


def test_mixed_round_only_patches_the_states_with_the_option():
    """files 1 and 3 have the option off: their requests, prompts and results are untouched by a first pass that names
    a language for every entry"""
    script = Script()
    states, seen, emitted = _round_run(decode_round_with, script, lambda f: _options(multilingual=f % 2 == 0))
    for f in (1, 3):
        assert not states[f].multilingual and seen[f][0] is None and seen[f][1] == -1
        assert all("language" not in s for s in emitted[f])
    assert [c[3][1] for c in script.log if c[0] == "fallback"] == [_lang_token("en")]        # window 1 keeps `en`
    # one call per distinct sot sequence: the two files without the option decode under `en` and share file 0's call
    assert script.aligned == []
    assert [(code, [k for k, _ in items]) for code, _, items in script.group_calls] == [("en", [0, 1, 3]), ("es", [2])]
    for f in (0, 2):
        assert all(s["language"] == LANGS[f] for s in emitted[f])


def test_round_without_the_option_keeps_one_call_per_item():
    script = Script(name_language=False)
    _, _, emitted = _round_run(decode_round_with, script, lambda f: _options(multilingual=False))
    assert script.group_calls == [] and [(k, c) for k, c, _ in script.aligned] == [(k, None) for k in range(4)]
    assert all(emitted[f] and "language" not in emitted[f][0] for f in range(4))


def test_english_only_tokenizer_turns_the_option_off():
    dims = model_dims("tiny.en")
    tk = Tokenizer(dims, task="transcribe", language="en", seed=3)
    assert tk.language is None and tk.for_language("es") is tk
    state = SeekState(6000, tk, _options(word_timestamps=False), dims.n_text_ctx)
    assert not state.multilingual and state.language is None
    req = state.next_request()
    assert req.language is None and req.lang_pos == -1
    state.set_window_language("es")                               # a no-op
    assert req.prompt == list(tk.sot_sequence) + [tk.no_timestamps]
    out = state.consume((SimpleNamespace(tokens=[400, 401], score=-0.2, no_speech_prob=0.0, language="es"), -0.1, 0.0, 1.0))
    assert out and "language" not in out[0]


def test_option_off_is_todays_loop():
    """With the option off, a backend that names languages all the same changes nothing: the requests, the prompts the
    fallbacks receive, the alignment calls (no tokenizer argument) and the segment dicts equal those of a backend that
    names none, and carry no new key."""
    a, b = Script(name_language=True), Script(name_language=False)
    sa, ra, oa = _drive_one(a, _options(multilingual=False))
    sb, rb, ob = _drive_one(b, _options(multilingual=False))
    assert not sa.multilingual and ra == rb and oa == ob and a.log == b.log
    assert all(r[0] is None and r[1] == -1 for r in ra)
    assert all(code is None and sot is None for _, code, sot in a.aligned) and len(a.aligned) == 4
    assert set(oa[0]) == {"id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob",
                          "compression_ratio", "no_speech_prob", "words"}
    # and the prompts are those of the option on with every window in the file's language
    _, rc, oc = _drive_one(Script(langs=["en"] * 4), _options(multilingual=True))
    assert [r[2] for r in rc] == [r[2] for r in ra]
    assert [{k: v for k, v in s.items() if k != "language"} for s in oc] == oa


def test_for_language_and_the_public_dataclasses(monkeypatch, caplog):
    tk = _tok()
    es = tk.for_language("es")
    assert es is tk.for_language("es") and es is not tk and tk.for_language("en") is tk
    assert es.sot_sequence == [ST.sot, _lang_token("es"), ST.transcribe] and tk.sot_sequence[1] == _lang_token("en")
    assert es.language_code == "es" and es.vocab is tk.vocab and es.encode(" hello") == tk.encode(" hello")
    from vlog_amd import transcribe as tr
    seg = tr.Segment(1, 0, 0.0, 1.0, "x", [1], -0.1, 1.0, 0.0, None, 0.0)          # today's positional construction
    assert seg.language is None and tr.Segment(1, 0, 0.0, 1.0, "x", [1], -0.1, 1.0, 0.0, None, 0.0, "es").language == "es"
    assert "language" not in seg._asdict()                                          # off: the dict is what it was
    assert list(tr.Segment(1, 0, 0.0, 1.0, "x", [1], -0.1, 1.0, 0.0, None, 0.0, "es")._asdict())[-1] == "language"
    monkeypatch.delenv("VLOG_AMD_MULTILINGUAL", raising=False)
    assert tr._resolve_multilingual(None) is False and tr._resolve_multilingual(True) is True
    monkeypatch.setenv("VLOG_AMD_MULTILINGUAL", "1")
    assert tr._resolve_multilingual(None) is True and tr._resolve_multilingual(False) is False
    monkeypatch.setenv("VLOG_AMD_MULTILINGUAL", "on")
    with pytest.raises(ValueError, match="VLOG_AMD_MULTILINGUAL must be 0 or 1"):
        tr._resolve_multilingual(None)
    # an English-only model turns the option off and says so once
    fake = SimpleNamespace(is_multilingual=False)
    with caplog.at_level(logging.WARNING, logger="vlog_amd"):
        assert tr.WhisperModel._multilingual(fake, True) is False and tr.WhisperModel._multilingual(fake, True) is False
    assert sum("English-only" in r.getMessage() for r in caplog.records) == 1
    multi = SimpleNamespace(is_multilingual=True)
    assert tr.WhisperModel._multilingual(multi, True) is True and tr.WhisperModel._multilingual(multi, True, [None]) is True
    # a named language: the argument stays refused, the environment's default is off
    with pytest.raises(NotImplementedError, match="multilingual=True with language='es'"):
        tr.WhisperModel._multilingual(multi, True, [None, "es"])
    monkeypatch.setenv("VLOG_AMD_MULTILINGUAL", "1")
    assert tr.WhisperModel._multilingual(multi, None, ["es"]) is False and tr.WhisperModel._multilingual(multi, None, [None]) is True
    assert tr.WhisperModel._multilingual(multi, False, ["es"]) is False
    # caption shaping copies the language to the cues
    from vlog_amd.captions import shape_captions
    words = [tr.Word(0.2 * i, 0.2 * i + 0.1, f" w{i}", 0.9) for i in range(12)]
    seg = tr.Segment(1, 0, 0.0, 2.4, "".join(w.word for w in words), list(range(12)), -0.1, 1.0, 0.0, words, 0.0, "es")
    cues = list(shape_captions(iter([seg]), 12, 1, None))
    assert len(cues) > 1 and all(c.language == "es" for c in cues)
