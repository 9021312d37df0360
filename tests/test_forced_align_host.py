"""CPU: the forced-alignment host loop (vlog_amd/forced_align.py) against a fake align_window that knows a
ground-truth word schedule and returns the exact staircase path and rows reached for what fits in each window."""
import math
import re

import numpy as np
import pytest

from vlog_amd import forced_align as fa
from vlog_amd.dims import model_dims
from vlog_amd.tokenizer import Tokenizer

PREPEND, APPEND = "\"'“¿([{-", "\"'.。,，!！?？:：”)]}、"


class _Tok:
    """Words at spaces, punctuation marks as words of their own; every token id is used once, so the fake window
    can look a candidate up in the schedule (a line encoded again gets the same ids)."""
    eot = 1 << 20

    def __init__(self):
        self.piece, self.memo = {}, {}

    def encode(self, text):
        if text in self.memo:
            return list(self.memo[text])
        out = self.memo.setdefault(text, [])
        for w in re.findall(r" ?[\w']+| ?[^\w\s]", text):
            n = 1 + (len(w.strip()) - 1) // 4                     # 1..3 tokens per word
            cuts = [round(k * len(w) / n) for k in range(n + 1)]
            for a, b in zip(cuts[:-1], cuts[1:]):
                t = len(self.piece)
                self.piece[t] = (w[a:b], a == 0)
                out.append(t)
        return list(out)

    def split_to_word_tokens(self, tokens):
        words, toks = [], []
        for t in tokens:
            if t == self.eot:
                words.append("")
                toks.append([t])
                continue
            p, first = self.piece[t]
            if first:
                words.append(p)
                toks.append([t])
            else:
                words[-1] += p
                toks[-1].append(t)
        return words, toks


class _Schedule:
    """entry[t]: the 20 ms frame at which token t is entered; end: the frame at which the speech ends."""

    def __init__(self, entry, end):
        self.entry, self.end = entry, end
        self.calls = []

    def window(self, seek, size, tokens):
        assert seek % 2 == 0
        g0, F = seek // 2, size // 2
        nxt = tokens[-1] + 1
        ent = [self.entry[t] for t in tokens] + [self.entry.get(nxt, self.end)]
        loc = [max(0, e - g0) for e in ent]
        R = max(1, sum(1 for l in loc if l < F))
        ti, tj = [], []
        for r in range(R):
            last = (loc[r + 1] - 1) if r + 1 < R else F - 1
            for c in range(loc[r], max(loc[r], last) + 1):
                ti.append(r)
                tj.append(c)
        self.calls.append((seek, size, len(tokens), R))
        probs = np.full(len(tokens), 0.5, dtype=np.float32)
        return probs, np.array(ti), np.array(tj), R


def _text(n_words, per_line, seed):
    rng = np.random.default_rng(seed)
    ws = ["".join(rng.choice(list("abcdefghij"), int(rng.integers(2, 10)))) for _ in range(n_words)]
    return [" ".join(ws[i: i + per_line]) for i in range(0, n_words, per_line)]


def _schedule(tok, lines, t0, step, gaps=()):
    """Word k starts at frame t0 + k step (+ the gaps (word index, frames) before it); a word's tokens enter 2
    frames apart.  -> (_Schedule, words, true (start, end) seconds per word)"""
    _, words = fa.prepare_words(tok, lines)
    entry, starts, f = {}, [], t0
    gaps = dict(gaps)
    for k, w in enumerate(words):
        f += gaps.get(k, 0)
        starts.append(f)
        for q, t in enumerate(w["tokens"]):
            entry[t] = f + 2 * q
        f += step
    end = f
    truth = [(s * 0.02, (starts[k + 1] if k + 1 < len(starts) else end) * 0.02) for k, s in enumerate(starts)]
    return _Schedule(entry, end), words, truth


def test_95s_schedule_over_four_windows():
    tok = _Tok()
    lines = _text(230, 12, 1)
    sch, words, truth = _schedule(tok, lines, 10, 20)             # a word every 0.4 s: 0.2 s .. 92.2 s
    segs, stats = fa.forced_align(tok, lines, 9500, 95.0, sch.window, max_cue_chars=None)
    assert stats["windows"] == 4 and stats["unaligned_words"] == 0
    got = [w for s in segs for w in s["words"]]
    assert len(got) == len(words)
    for w, (s, e) in zip(got, truth):
        assert abs(w["start"] - s) <= 0.02 + 1e-9 and abs(w["end"] - e) <= 0.02 + 1e-9, (w, s, e)
        assert w["probability"] == 0.5
    rows = stats["window_rows"]
    assert all(reached < offered for _, offered, reached in rows[:-1])
    assert rows[-1][2] == rows[-1][1]
    assert [r[0] for r in rows] == sorted(r[0] for r in rows) and rows[0][0] == 0
    assert len(segs) == len(lines) and [s["id"] for s in segs] == list(range(1, len(lines) + 1))
    assert all(abs(s["avg_logprob"] - math.log(0.5)) < 1e-6 and s["temperature"] == 0.0 and s["no_speech_prob"] == 0.0
               for s in segs)


def test_silent_window_advances_seek_and_loses_no_word():
    tok = _Tok()
    lines = _text(60, 10, 2)
    sch, words, truth = _schedule(tok, lines, 10, 20, gaps={30: 2600})     # 12 s of speech, 52 s of silence, speech
    segs, stats = fa.forced_align(tok, lines, 9000, 90.0, sch.window, max_cue_chars=None)
    rows = stats["window_rows"]
    silent = [k for k, r in enumerate(rows) if r[2] == 1]
    assert silent and all(rows[k + 1][0] == rows[k][0] + 3000 for k in silent)
    assert stats["unaligned_words"] == 0
    got = [w for s in segs for w in s["words"]]
    assert len(got) == len(words)
    for k, (w, (s, e)) in enumerate(zip(got, truth)):
        if k != 29:                                  # the word before the silence starts where its window starts
            assert abs(w["start"] - s) <= 0.02 + 1e-9, (k, w, s)
        assert abs(w["end"] - e) <= 0.02 + 1e-9, (k, w, e)


def test_text_longer_than_the_audio():
    tok = _Tok()
    lines = _text(100, 10, 3)
    sch, words, truth = _schedule(tok, lines, 10, 30)             # 60 s of words
    segs, stats = fa.forced_align(tok, lines, 4000, 40.0, sch.window, max_cue_chars=None)
    assert 0 < stats["unaligned_words"] < len(words)
    got = [w for s in segs for w in s["words"]]
    assert len(got) == len(words)
    tail = got[-stats["unaligned_words"]:]
    assert all(w["start"] == w["end"] == 40.0 and w["probability"] == 0.0 for w in tail)
    assert all(w["end"] <= 40.0 for w in got)
    head = got[: len(words) - stats["unaligned_words"]]
    assert all(abs(w["start"] - s) <= 0.02 + 1e-9 for w, (s, _) in zip(head, truth))
    assert segs[-1]["avg_logprob"] == pytest.approx(math.log(1e-30))


def test_token_budget_and_overlong_word():
    tok = _Tok()
    lines = _text(80, 8, 4)
    sch, words, _ = _schedule(tok, lines, 10, 20)
    _, stats = fa.forced_align(tok, lines, 4000, 40.0, sch.window, max_window_tokens=12)
    assert all(n <= 12 for _, _, n, _ in sch.calls) and max(n for _, _, n, _ in sch.calls) >= 10
    assert stats["unaligned_words"] == 0
    assert all(offered == n + 1 for (_, offered, _), (_, _, n, _) in zip(stats["window_rows"], sch.calls))
    tok2 = _Tok()
    long_line = ["ab " + "x" * 40 + " cd"]                       # a word of 10 tokens
    sch2, _, _ = _schedule(tok2, long_line, 10, 20)
    with pytest.raises(ValueError, match="max_window_tokens"):
        fa.forced_align(tok2, long_line, 3000, 30.0, sch2.window, max_window_tokens=9)
    with pytest.raises(ValueError, match="empty"):
        fa.forced_align(_Tok(), " \n\n ", 3000, 30.0, sch2.window)


def test_lines_map_to_segments_and_punctuation_merges():
    tok = _Tok()
    text = 'hello there, world.\n\n  "quoted" words here!  \nlast line'
    assert fa.split_lines(text) == ["hello there, world.", '"quoted" words here!', "last line"]
    sch, words, truth = _schedule(tok, text, 10, 20)
    assert [w["word"] for w in words][:5] == [" hello", " there", ",", " world", "."]
    segs, stats = fa.forced_align(tok, text, 3000, 30.0, sch.window, prepend_punctuations=PREPEND,
                                  append_punctuations=APPEND)
    assert [s["text"] for s in segs] == [" hello there, world.", ' "quoted" words here!', " last line"]
    assert [[w["word"] for w in s["words"]] for s in segs] == [
        [" hello", " there,", " world."], [' "quoted"', " words", " here!"], [" last", " line"]]
    # a merged mark keeps its host word's times; the segment spans its words; the tokens are the line's, in order
    assert segs[0]["words"][1]["start"] == pytest.approx(truth[1][0], abs=0.02)
    assert segs[0]["words"][1]["end"] == pytest.approx(truth[1][1], abs=0.02)
    for s in segs:
        assert s["start"] == s["words"][0]["start"] and s["end"] == s["words"][-1]["end"]
    assert [t for s in segs for t in s["tokens"]] == [t for w in words for t in w["tokens"]]
    assert fa.split_lines(["  a ", "", "b"]) == ["a", "b"]


def test_prepare_words_with_the_model_tokenizer():
    tok = Tokenizer(model_dims("tiny"), language="en")
    lines, words = fa.prepare_words(tok, "some words here\nand more")
    assert lines == ["some words here", "and more"]
    for li, line in enumerate(lines):
        mine = [w for w in words if w["line"] == li]
        assert "".join(w["word"] for w in mine) == " " + line
        assert [t for w in mine for t in w["tokens"]] == tok.encode(" " + line)
    assert all(t < tok.eot for w in words for t in w["tokens"])


def _cue_words(text):
    ws = re.findall(r" ?\S+", text)
    return [dict(line=0, word=w if w.startswith(" ") else " " + w, tokens=[k], start=k * 1.0, end=k + 1.0,
                 probability=1.0, token_probs=[1.0], seek=0, aligned=True) for k, w in enumerate(ws)]


def test_cue_shaping():
    text = ("the quick brown fox jumps over the lazy dog. then it rests for a while under the old tree! "
            "nobody knows why it does that")
    words = _cue_words(text)
    one = fa.build_segments([text], words, PREPEND, APPEND, max_cue_chars=None)
    assert len(one) == 1 and one[0]["text"].strip() == text
    for limit in (20, 84):
        cues = fa.build_segments([text], words, PREPEND, APPEND, max_cue_chars=limit)
        assert len(cues) > 1 and [c["id"] for c in cues] == list(range(1, len(cues) + 1))
        assert "".join(c["text"] for c in cues).strip() == text
        assert all(len(c["text"].strip()) <= limit for c in cues)
        assert [w["word"] for c in cues for w in c["words"]] == [w["word"] for w in words]
        for a, b in zip(cues[:-1], cues[1:]):
            nxt = b["words"][0]["word"]
            full = len((a["text"] + nxt).strip()) > limit
            sentence = a["text"].strip()[-1] in ".?!。？！" and 2 * len(a["text"].strip()) >= limit
            assert full or sentence, (a["text"], nxt)
            assert a["end"] == a["words"][-1]["end"] and b["start"] == b["words"][0]["start"]
    at84 = fa.build_segments([text], words, PREPEND, APPEND, max_cue_chars=84)
    assert at84[0]["text"].strip().endswith("dog.")              # 44 characters >= 42: cut at the sentence end
    short = "a short line"
    assert len(fa.build_segments([short], _cue_words(short), PREPEND, APPEND, max_cue_chars=20)) == 1


def test_adversarial_window_terminates():
    tok = _Tok()
    lines = _text(50, 10, 5)
    calls = []

    def stuck(seek, size, tokens):
        calls.append(seek)
        F = size // 2
        return np.full(len(tokens), 0.5, np.float32), np.zeros(F, dtype=int), np.arange(F), 1

    segs, stats = fa.forced_align(tok, lines, 9003, 90.03, stuck)
    # a rest of 3 mel frames is one attention column: no window (its z-score over the rows is 0 / 0)
    assert calls == [0, 3000, 6000] and stats["windows"] == 3
    assert stats["unaligned_words"] == 50
    assert all(w["start"] == w["end"] == 90.03 for s in segs for w in s["words"])
    calls.clear()
    fa.forced_align(tok, lines, 9004, 90.04, stuck)
    assert calls == [0, 3000, 6000, 9000]
