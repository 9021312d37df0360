"""CPU: the caption rule (vlog_amd/captions.py shape_captions, resolve_caption_options) on hand-written cases with
literal texts, on seeded random word streams against the straight-line restatement tests/captions_ref.py, and through
the worker's WebVTT writer."""
import random

import pytest

from tests.captions_ref import ref_cues
from vlog_amd import captions as cap
from vlog_amd.captions import resolve_caption_options, set_word_tokens, shape_captions, word_tokens
from vlog_amd.transcribe import Segment, Word
from vlog_amd.vtt import generate_webvtt

TS = 50364          # a timestamp token: every id from <|endoftext|> (50257) up is no text


def _parent(words, seek=0, text=None, pid=7):
    """words: [(text, start, end)] or [(text, start, end, tokens)] -> a Segment as transcribe yields it with word
    timestamps: tokens = timestamp, the words' tokens, timestamp"""
    ws, toks = [], []
    for k, w in enumerate(words):
        t = list(w[3]) if len(w) > 3 else ([1000 * (seek + 1) + k] if w[0] else [])
        ws.append(set_word_tokens(Word(start=w[1], end=w[2], word=w[0], probability=0.5), t))
        toks += t
    return Segment(id=pid, seek=seek, start=ws[0].start if ws else 0.0, end=ws[-1].end if ws else 1.0,
                   text="".join(w[0] for w in words) if text is None else text, tokens=[TS] + toks + [TS + 50],
                   avg_logprob=-0.25 - seek, compression_ratio=1.5 + seek, no_speech_prob=0.125, words=ws,
                   temperature=0.2)


def _even(texts, step=0.5):
    return [(t, k * step, (k + 1) * step) for k, t in enumerate(texts)]


def _texts(cues):
    return [c.text for c in cues]


# ---------------------------------------------------------------------------------------------- hand-written cases
def test_break_on_line_count():
    p = _parent(_even([" aaaa", " bbbb", " cccc", " dddd", " eeee"]))
    cues = list(shape_captions([p], 10, 2))
    assert _texts(cues) == [" aaaa bbbb\ncccc dddd", " eeee"]
    assert [[w.word for w in c.words] for c in cues] == [[" aaaa", " bbbb", " cccc", " dddd"], [" eeee"]]
    assert [(c.id, c.start, c.end) for c in cues] == [(1, 0.0, 2.0), (2, 2.0, 2.5)]
    assert [c.tokens for c in cues] == [[1000, 1001, 1002, 1003], [1004]]
    for c in cues:
        assert (c.seek, c.avg_logprob, c.compression_ratio, c.no_speech_prob, c.temperature) == \
               (0, -0.25, 1.5, 0.125, 0.2)
    assert _texts(shape_captions([p], 10, 1)) == [" aaaa bbbb", " cccc dddd", " eeee"]
    assert _texts(shape_captions([p], 10, 3)) == [" aaaa bbbb\ncccc dddd\neeee"]


def test_break_on_a_pause_above_three_seconds_only():
    p = _parent([(" a", 0.0, 1.0), (" b", 3.9, 4.5), (" c", 7.7, 8.0)])       # pauses of 2.9 s and 3.2 s
    cues = list(shape_captions([p], 42, 2))
    assert _texts(cues) == [" a b", " c"]
    assert [(c.start, c.end) for c in cues] == [(0.0, 4.5), (7.7, 8.0)]
    assert cap.CUE_BREAK_PAUSE_S == 3.0


def test_break_on_max_cue_seconds():
    p = _parent([(" a", 0.0, 0.5), (" b", 0.5, 1.0), (" c", 1.0, 2.5), (" d", 2.5, 3.0), (" e", 3.0, 6.0),
                 (" f", 6.0, 6.25)])
    # c would end 2.5 s after a: new cue; d ends exactly 2.0 s after c starts: stays; e is longer than the limit: alone
    assert _texts(shape_captions([p], 42, 2, 2.0)) == [" a b", " c d", " e", " f"]
    assert _texts(shape_captions([p], 42, 2)) == [" a b c d e f"]


def test_sentence_end_breaks_at_exactly_half_capacity():
    # 10 x 2 = 20 characters: "abcd efgh." is 10, half of it
    at = _parent(_even([" abcd", " efgh.", " xy"]))
    assert _texts(shape_captions([at], 10, 2)) == [" abcd efgh.", " xy"]
    below = _parent(_even([" abcd", " efg.", " xy"]))                        # 9 characters: one below
    assert _texts(shape_captions([below], 10, 2)) == [" abcd efg.\nxy"]
    for mark in "?!。？！":
        assert len(list(shape_captions([_parent(_even([" abcd", " efgh" + mark, " xy"]))], 10, 2))) == 2
    assert len(list(shape_captions([_parent(_even([" abcd", " efgh,", " xy"]))], 10, 2))) == 1


def test_an_over_wide_word_has_a_line_to_itself():
    p = _parent(_even([" hi", " extraordinary", " ok"]))
    assert _texts(shape_captions([p], 5, 2)) == [" hi\nextraordinary", " ok"]
    assert _texts(shape_captions([_parent(_even([" extraordinary"]))], 5, 2)) == [" extraordinary"]


def test_a_parent_without_words_passes_through():
    a = _parent(_even([" aaaa", " bbbb", " cccc"]), seek=0)
    none = Segment(id=9, seek=3000, start=30.0, end=31.0, text=" no words here at all", tokens=[TS, 5, 6, TS + 9],
                   avg_logprob=-0.5, compression_ratio=1.0, no_speech_prob=0.0, words=None, temperature=0.0)
    empty = Segment(id=10, seek=3000, start=31.0, end=32.0, text=" nor here", tokens=[TS, 7, TS + 9],
                    avg_logprob=-0.5, compression_ratio=1.0, no_speech_prob=0.0, words=[], temperature=0.0)
    cues = list(shape_captions([a, none, empty], 10, 2))
    assert [c.id for c in cues] == [1, 2, 3] and _texts(cues)[0] == " aaaa bbbb\ncccc"
    for got, src in ((cues[1], none), (cues[2], empty)):
        src.id = got.id
        assert got == src


def test_leading_space_kept_iff_the_parent_has_one():
    assert _texts(shape_captions([_parent(_even([" one", " two"]))], 42))[0] == " one two"
    assert _texts(shape_captions([_parent(_even(["one", " two"]))], 42))[0] == "one two"
    assert _texts(shape_captions([_parent(_even([" one", " two"]), text="one two")], 42))[0] == "one two"


def test_words_stay_as_they_are_and_empty_ones_are_skipped():
    p = _parent(_even([" aaaa", "", " bbbb", " cccc"]))
    before = [(w.word, w.start, w.end, w.probability) for w in p.words]
    cues = list(shape_captions([p], 10, 1))
    assert [[w.word for w in c.words] for c in cues] == [[" aaaa", " bbbb"], [" cccc"]]
    assert [id(w) for c in cues for w in c.words] == [id(w) for w in p.words if w.word]      # the same objects
    assert [(w.word, w.start, w.end, w.probability) for w in p.words] == before
    assert all("\n" not in w.word for c in cues for w in c.words)
    assert p.words[0]._asdict() == dict(start=0.0, end=0.5, word=" aaaa", probability=0.5)     # four public fields


def test_words_without_tokens_leave_the_tokens_on_the_first_cue():
    ws = [Word(start=k * 0.5, end=k * 0.5 + 0.5, word=t, probability=1.0) for k, t in enumerate([" aaaa", " bbbb", " cc"])]
    p = Segment(id=1, seek=0, start=0.0, end=1.5, text=" aaaa bbbb cc", tokens=[TS, 1, 2, 3, TS + 5], avg_logprob=0.0,
                compression_ratio=1.0, no_speech_prob=0.0, words=ws, temperature=0.0)
    assert [c.tokens for c in shape_captions([p], 6, 1)] == [[TS, 1, 2, 3, TS + 5], [], []]
    assert word_tokens(ws[0]) == []


def test_arguments_are_checked():
    for bad in ((0, 2, None), (-1, 2, None), (10, 0, None), (10, 5, None), (10, 2, 0.0), (10, 2, -1.0)):
        with pytest.raises(ValueError):
            list(shape_captions([], *bad))


# ------------------------------------------------------------------------------------- random streams, the reference
N_STREAMS = 320
GAPS = (0.0, 0.0, 0.0, 0.04, 0.3, 1.0, 2.9, 2.99, 3.0, 3.01, 3.2, 6.0)
LETTERS = "abcdefghijklmnopqrstuvwxyz"


def _stream(seed):
    """-> (parents, (width, count, seconds), per parent its (text, start, end, tokens) tuples or None)"""
    rng = random.Random(seed)
    n = rng.randint(1, 40)
    t = round(rng.uniform(0.0, 5.0), 2)
    words = []
    for k in range(n):
        body = "".join(rng.choice(LETTERS) for _ in range(rng.randint(1, 14)))
        r = rng.random()
        if r < 0.15:
            body = body[:13] + rng.choice(".?!。？！")
        elif r < 0.2:
            body = body[:13] + ","
        text = (" " if rng.random() < 0.9 else "") + body
        if rng.random() < 0.04:
            text = ""                                   # a word merge_punctuations emptied
        start = round(t + rng.choice(GAPS), 2)
        end = round(start + rng.choice((0.0, 0.08, 0.3, 0.7, 1.6, 8.0 if rng.random() < 0.05 else 0.5)), 2)
        t = end
        toks = [rng.randrange(50257) for _ in range(rng.randint(1, 3))] if text else []
        words.append((text, start, end, toks))
    cuts = sorted(rng.sample(range(1, n), min(n - 1, rng.randint(0, 3)))) if n > 1 else []
    raw, parents = [], []
    for s, e in zip([0] + cuts, cuts + [n]):
        if rng.random() < 0.1:                          # a segment that got no words
            parents.append(Segment(id=99, seek=len(parents), start=words[s][1], end=words[s][1] + 1.0, text=" wordless",
                                   tokens=[TS, 11, TS + 1], avg_logprob=-1.0, compression_ratio=1.0,
                                   no_speech_prob=0.5, words=None if rng.random() < 0.5 else [], temperature=0.0))
            raw.append(None)
        parents.append(_parent(words[s:e], seek=len(parents), pid=50 + len(parents)))
        raw.append(words[s:e])
    opts = (rng.randint(8, 42), rng.randint(1, 3), None if rng.random() < 0.4 else rng.choice((2, 3, 4.5, 7)))
    return parents, opts, raw


STREAMS = [_stream(s) for s in range(N_STREAMS)]


def test_the_streams_cover_the_rule():
    assert len(STREAMS) >= 300
    lens = [sum(len(r) for r in raw if r) for _, _, raw in STREAMS]
    assert min(lens) == 1 and max(lens) == 40
    assert {o[0] for _, o, _ in STREAMS} >= {8, 42} and {o[1] for _, o, _ in STREAMS} == {1, 2, 3}
    assert {o[2] for _, o, _ in STREAMS} >= {None, 2, 7}
    split = sum(1 for parents, o, _ in STREAMS if len(list(shape_captions(parents, *o))) > len(parents))
    assert split > N_STREAMS // 2


@pytest.mark.parametrize("block", range(8))
def test_random_streams_equal_the_reference(block):
    for parents, (width, count, seconds), raw in STREAMS[block::8]:
        got = list(shape_captions(iter(parents), width, count, seconds))
        exp = []
        for parent, words in zip(parents, raw):
            if words is None or not any(w[0] for w in words):
                exp.append((parent.seek, parent.start, parent.end, parent.text, parent.tokens,
                            [w[:3] for w in words] if words else None))
                continue
            lead = " " if parent.text.startswith(" ") else ""
            for c in ref_cues(words, width, count, seconds):
                exp.append((parent.seek, c["start"], c["end"], lead + "\n".join(c["lines"]), c["tokens"],
                            [words[k][:3] for k in c["words"]]))
        assert [c.id for c in got] == list(range(1, len(got) + 1))
        assert [(c.seek, c.start, c.end, c.text, c.tokens,
                 [(w.word, w.start, w.end) for w in c.words] if c.words else None) for c in got] == exp


@pytest.mark.parametrize("block", range(8))
def test_properties_on_the_random_streams(block):
    for parents, (width, count, seconds), raw in STREAMS[block::8]:
        pulls = []

        def source():
            for k, p in enumerate(parents):
                pulls.append(k)
                yield p

        by_parent = {k: [] for k in range(len(parents))}
        ids = []
        for cue in shape_captions(source(), width, count, seconds):
            # seek is the parent's index here: the cue comes out while its parent is the last one pulled
            assert pulls[-1] == cue.seek, "a cue was held back past the next pull"
            by_parent[cue.seek].append(cue)
            ids.append(cue.id)
        assert pulls == list(range(len(parents))) and ids == list(range(1, len(ids) + 1))
        for k, parent in enumerate(parents):
            cues = by_parent[k]
            assert cues, "every parent yields something"
            kept = [w for w in (parent.words or []) if w.word]
            if not kept:
                assert len(cues) == 1 and cues[0].words == parent.words and cues[0].text == parent.text
                continue
            # the words, and the tokens below <|endoftext|>, in order; no cue spans parents
            assert [id(w) for c in cues for w in c.words] == [id(w) for w in kept]
            assert [t for c in cues for t in c.tokens] == [t for t in parent.tokens if t < 50257]
            for c in cues:
                assert (c.seek, c.avg_logprob, c.compression_ratio, c.no_speech_prob, c.temperature) == \
                       (parent.seek, parent.avg_logprob, parent.compression_ratio, parent.no_speech_prob,
                        parent.temperature)
                assert c.start == c.words[0].start and c.end == c.words[-1].end
                assert c.tokens == [t for w in c.words for t in word_tokens(w)]
                lines = c.text[1:].split("\n") if c.text.startswith(" ") else c.text.split("\n")
                assert c.text.startswith(" ") == parent.text.startswith(" ")
                assert 1 <= len(lines) <= count
                assert "".join(lines).replace(" ", "") == "".join(w.word for w in c.words).replace(" ", "")
                for line in lines:
                    assert line and line == line.strip()
                    assert len(line) <= width or len(line.split()) == 1, (line, width)
                if seconds is not None and len(c.words) > 1:
                    assert c.words[-1].end - c.words[0].start <= seconds
                for a, b in zip(c.words, c.words[1:]):
                    assert b.start - a.end <= 3.0


def test_webvtt_payloads_of_shaped_cues():
    for parents, (width, count, seconds), _ in STREAMS[::5]:
        cues = list(shape_captions(parents, width, count, seconds))
        vtt = generate_webvtt({"start": c.start, "end": c.end, "text": c.text} for c in cues)
        blocks = vtt[len("WEBVTT\n\n"):].rstrip("\n").split("\n\n")
        assert len(blocks) == len(cues)                 # an empty line inside a payload would end its block early
        for n, (block, cue) in enumerate(zip(blocks, cues), start=1):
            head, times, *payload = block.split("\n")
            assert head == str(n) and " --> " in times
            assert payload == cue.text.strip().split("\n") and all(payload)
            if cue.words:
                assert len(payload) <= count


# ------------------------------------------------------------------------------------------ resolve_caption_options
W, C, S = "VLOG_AMD_MAX_LINE_WIDTH", "VLOG_AMD_MAX_LINE_COUNT", "VLOG_AMD_MAX_CUE_SECONDS"


def test_resolve_off_and_on():
    assert resolve_caption_options(None, None, None, {}) is None
    assert resolve_caption_options(None, None, None, {W: ""}) is None
    assert resolve_caption_options(None, None, None, {W: "0"}) is None
    assert resolve_caption_options(0, None, None, {}) is None
    assert resolve_caption_options(42, None, None, {}) == (42, 2, None)
    assert resolve_caption_options(42, 1, 7, {}) == (42, 1, 7.0)
    assert resolve_caption_options(None, None, None, {W: "42"}) == (42, 2, None)
    assert resolve_caption_options(None, None, None, {W: " 42 ", C: "3", S: "6.5"}) == (42, 3, 6.5)


def test_resolve_arguments_win_over_the_environment():
    env = {W: "42", C: "3", S: "7"}
    assert resolve_caption_options(0, None, None, env) is None              # 0 turns it off whatever is set
    assert resolve_caption_options(20, None, None, env) == (20, 3, 7.0)
    assert resolve_caption_options(None, 1, 2.5, env) == (42, 1, 2.5)
    assert resolve_caption_options(20, 4, 1, env) == (20, 4, 1.0)


def test_resolve_count_and_seconds_apply_only_while_on():
    assert resolve_caption_options(None, None, None, {C: "3", S: "7"}) is None
    assert resolve_caption_options(None, None, None, {C: "nine", S: "-1"}) is None      # not looked at while off
    assert resolve_caption_options(0, None, None, {W: "42", C: "9"}) is None


@pytest.mark.parametrize("args, env, names", [
    ((-1, None, None), {}, "max_line_width"),
    ((None, None, None), {W: "-3"}, W),
    ((42, 0, None), {}, "max_line_count"),
    ((42, 5, None), {}, "max_line_count"),
    ((42, None, None), {C: "0"}, C),
    ((42, None, None), {C: "5"}, C),
    ((42, None, 0), {}, "max_cue_seconds"),
    ((42, None, -2.0), {}, "max_cue_seconds"),
    ((42, None, None), {S: "0"}, S),
    ((42, None, None), {S: "nan"}, S),
    ((None, 2, None), {}, "max_line_count"),            # passed while shaping is off
    ((None, None, 7.0), {}, "max_cue_seconds"),
    ((0, 2, None), {W: "42"}, "max_line_count"),
    ((0, None, 7.0), {W: "42"}, "max_cue_seconds"),
    ((None, None, None), {W: "wide"}, W),               # environment values that do not parse
    ((None, None, None), {W: "4.5"}, W),
    ((42, None, None), {C: "two"}, C),
    ((None, None, None), {W: "42", S: "7s"}, S),
    ((4.5, None, None), {}, "max_line_width"),
    ((True, None, None), {}, "max_line_width"),
    ((42, None, "7"), {}, "max_cue_seconds"),
])
def test_resolve_value_errors(args, env, names):
    with pytest.raises(ValueError, match=names):
        resolve_caption_options(*args, env)


def test_no_torch_in_the_module():
    import subprocess
    import sys
    code = "import sys; import vlog_amd.captions; sys.exit(1 if 'torch' in sys.modules else 0)"
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


def test_exported_from_the_compat_package():
    import os
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat")
    sys.path.insert(0, compat)
    try:
        import faster_whisper
        assert faster_whisper.shape_captions is shape_captions and "shape_captions" in faster_whisper.__all__
    finally:
        sys.path.remove(compat)
