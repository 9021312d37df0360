"""Forced alignment: put times on a GIVEN transcript (`WhisperModel.align`), the host side.

`word_timestamps=True` times the text the decoder emitted, window by window, and every window's text lies inside
its 30 s of audio.  Here the text comes from outside (an edited transcript) and nobody knows which words fall into
which window, so every window is offered more text than it can hold and the device's open-end DTW
(`wm_align_open_batch`, csrc/align.hip) says how far the audio got: it returns the path and R, the rows reached.

Pure functions over a callable

    align_window(seek, size, tokens) -> (probs [n_tokens], text_idx, time_idx, rows)

(the teacher-forced pass over the window of `size` mel frames at `seek`, with `tokens` as its text; no torch and no
GPU in this module, so the loop is tested on a CPU against a known word schedule).

  prepare_words  text -> lines and one global word list of (line, word, tokens)
  run_alignment  the long-form loop: state = (seek, first pending word); every round advances one of them
  build_segments per line: merge_punctuations, cue shaping, Segment-shaped dicts
  forced_align   the three together
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .dims import N_FRAMES
from .segments import _word_means, compression_ratio, merge_punctuations

SENTENCE_END = ".?!。？！"


def split_lines(text: Union[str, Sequence[str]]) -> List[str]:
    """A str is split at newlines; lines are stripped and empty ones dropped."""
    lines = text.split("\n") if isinstance(text, str) else list(text)
    return [s for s in (str(l).strip() for l in lines) if s]


def prepare_words(tokenizer, text: Union[str, Sequence[str]]) -> Tuple[List[str], List[dict]]:
    """-> (lines, words): every line encoded as " " + line and split with the tokenizer's word splitter, as
    find_alignment splits a window's text; one global list of dict(line, word, tokens)."""
    lines = split_lines(text)
    words: List[dict] = []
    for li, line in enumerate(lines):
        tokens = list(tokenizer.encode(" " + line))
        ws, wts = tokenizer.split_to_word_tokens(tokens + [tokenizer.eot])
        for w, t in zip(ws[:-1], wts[:-1]):
            words.append(dict(line=li, word=w, tokens=list(t)))
    return lines, words


def window_candidate(words: Sequence[dict], w0: int, max_window_tokens: int) -> int:
    """-> w1: words[w0:w1] is the longest run from w0 whose tokens total <= max_window_tokens (at least one word:
    a single word above the budget raises ValueError)."""
    total, w1 = 0, w0
    while w1 < len(words) and total + len(words[w1]["tokens"]) <= max_window_tokens:
        total += len(words[w1]["tokens"])
        w1 += 1
    if w1 == w0:
        raise ValueError(f"word {words[w0]['word']!r} has {len(words[w0]['tokens'])} tokens, above "
                         f"max_window_tokens={max_window_tokens}")
    return w1


def accept_window(counts: Sequence[int], probs, text_idx, time_idx, rows: int, tokens_per_second: int = 50
                  ) -> List[Tuple[float, float, float]]:
    """One window's result -> (local start, local end, probability) of the words it accepts.  counts: tokens per
    candidate word; the matrix has sum(counts) + 1 rows (the last predicts <|endoftext|>) and the path reached rows
    0 .. rows-1.  jump_times[r] is the time at which row r is entered (find_alignment's jumps, over the rows
    reached); word k spans rows wb[k] .. wb[k+1]-1 and is accepted iff row wb[k+1], the one that predicts the next
    word's first token or <|endoftext|>, was entered: its end time is known."""
    text_idx = np.asarray(text_idx)
    time_idx = np.asarray(time_idx)
    if rows <= 0 or len(text_idx) == 0:
        return []
    jumps = np.pad(np.diff(text_idx), (1, 0), constant_values=1).astype(bool)
    jump_times = time_idx[jumps] / tokens_per_second
    wb = np.pad(np.cumsum(counts), (1, 0))
    n_acc = int(np.searchsorted(wb[1:], min(rows, len(jump_times)) - 1, side="right"))
    if n_acc == 0:
        return []
    wprob = _word_means(np.asarray(probs), wb[: n_acc + 1])
    return [(float(jump_times[wb[k]]), float(jump_times[wb[k + 1]]), wprob[k]) for k in range(n_acc)]


def run_alignment(words: List[dict], content_frames: int, duration: float, align_window: Callable,
                  max_window_tokens: int = 224, frames_per_second: int = 100, tokens_per_second: int = 50) -> dict:
    """The long-form loop.  Fills start / end / probability / token_probs / seek / aligned into every word and
    returns dict(windows, unaligned_words, window_rows=[(seek, candidate_rows, rows_reached)]).

    While words remain and seek < content_frames: the window is min(3000, content_frames - seek) frames at seek
    (the loop stops at a rest of fewer than two attention columns, 4 mel frames);
    the candidate is the longest run of pending words within the token budget (default 224 = n_text_ctx // 2, the
    most a window ever decodes); align_window gives the open-end path; accepted words (accept_window) get
    seek / 100 + their local times, rounded to 0.01 as add_word_timestamps rounds, and seek moves to the last
    accepted end.  A window that accepts nothing (silence: the DTW has nothing to hold on to) moves seek by the
    window.  Every round advances the first pending word or seek, so the loop ends.  Words still pending when the
    audio ends get start = end = duration and probability 0.0 and are counted in unaligned_words."""
    if max_window_tokens < 1:
        raise ValueError("max_window_tokens must be >= 1")
    seek, w0 = 0, 0
    window_rows: List[Tuple[int, int, int]] = []
    while w0 < len(words) and seek < content_frames:
        size = min(N_FRAMES, content_frames - seek)
        if size // 2 < 2:                           # one attention column cannot be z-scored over the rows: every
            break                                   # renormalised weight is 1, the deviation 0, the cost NaN
        w1 = window_candidate(words, w0, max_window_tokens)
        counts = [len(w["tokens"]) for w in words[w0:w1]]
        tokens = [t for w in words[w0:w1] for t in w["tokens"]]
        probs, text_idx, time_idx, rows = align_window(seek, size, tokens)
        rows = int(rows)
        window_rows.append((seek, len(tokens) + 1, rows))
        accepted = accept_window(counts, probs, text_idx, time_idx, rows, tokens_per_second)
        offset = seek / frames_per_second
        pos = 0
        for w, (s, e, p) in zip(words[w0:], accepted):
            n = len(w["tokens"])
            w.update(start=round(offset + s, 2), end=round(offset + e, 2), probability=p,
                     token_probs=[float(x) for x in probs[pos: pos + n]], seek=seek, aligned=True)
            pos += n
        if accepted:
            w0 += len(accepted)
            seek += int(round(accepted[-1][1] * frames_per_second))
        else:
            seek += size
    end_seek = max(0, min(seek, content_frames))
    for w in words[w0:]:
        w.update(start=round(duration, 2), end=round(duration, 2), probability=0.0,
                 token_probs=[0.0] * len(w["tokens"]), seek=end_seek, aligned=False)
    return dict(windows=len(window_rows), unaligned_words=len(words) - w0, window_rows=window_rows)


def shape_cues(words: Sequence[dict], max_cue_chars: Optional[int]) -> List[List[dict]]:
    """One line's words -> its cues.  A line of at most max_cue_chars characters (None: any line) is one cue; a
    longer one is cut greedily at word boundaries: a new cue starts when the next word would exceed the limit, or
    when the previous word ends a sentence (one of .?!。？！) and the cue already holds at least half the limit."""
    words = list(words)
    if not words:
        return []
    if max_cue_chars is None or len("".join(w["word"] for w in words).strip()) <= max_cue_chars:
        return [words]
    cues: List[List[dict]] = [[]]
    text = ""
    for w in words:
        if cues[-1]:
            prev = cues[-1][-1]["word"].strip()
            if len((text + w["word"]).strip()) > max_cue_chars or (
                    prev and prev[-1] in SENTENCE_END and 2 * len(text.strip()) >= max_cue_chars):
                cues.append([])
                text = ""
        cues[-1].append(w)
        text += w["word"]
    return cues


def build_segments(lines: Sequence[str], words: Sequence[dict], prepend_punctuations: str, append_punctuations: str,
                   max_cue_chars: Optional[int] = 84) -> List[dict]:
    """Per line: merge_punctuations over its words, cue shaping, one Segment-shaped dict per cue (ids 1, 2, ...):
    start of its first word, end of its last, text, words, tokens, avg_logprob = the mean log of the token
    probabilities (the log's input floored at 1e-30), temperature 0.0, no_speech_prob 0.0."""
    out: List[dict] = []
    for li in range(len(lines)):
        mine = [w for w in words if w["line"] == li]
        al = [dict(word=w["word"], tokens=list(w["tokens"]), start=w["start"], end=w["end"],
                   probability=w["probability"], seek=w["seek"]) for w in mine]
        tprobs = [p for w in mine for p in w["token_probs"]]          # merging moves tokens between neighbours only,
        merge_punctuations(al, prepend_punctuations, append_punctuations)   # so the line's token order is kept
        pos = 0
        for cue in shape_cues([w for w in al if w["word"]], max_cue_chars):
            tokens = [t for w in cue for t in w["tokens"]]
            lp = [math.log(max(p, 1e-30)) for p in tprobs[pos: pos + len(tokens)]]
            pos += len(tokens)
            text = "".join(w["word"] for w in cue)
            out.append(dict(id=len(out) + 1, seek=cue[0]["seek"], start=cue[0]["start"], end=cue[-1]["end"], text=text,
                            tokens=tokens, avg_logprob=float(np.mean(lp)) if lp else 0.0,
                            compression_ratio=compression_ratio(text), no_speech_prob=0.0, temperature=0.0,
                            words=[dict(word=w["word"], start=w["start"], end=w["end"], probability=w["probability"])
                                   for w in cue]))
    return out


def forced_align(tokenizer, text: Union[str, Sequence[str]], content_frames: int, duration: float,
                 align_window: Callable, max_window_tokens: int = 224, max_cue_chars: Optional[int] = 84,
                 prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
                 frames_per_second: int = 100, tokens_per_second: int = 50) -> Tuple[List[dict], dict]:
    """text against content_frames mel frames of audio (duration seconds) -> (segment dicts, loop statistics)."""
    lines, words = prepare_words(tokenizer, text)
    if not words:
        raise ValueError("align: empty text")
    stats = run_alignment(words, content_frames, duration, align_window, max_window_tokens, frames_per_second,
                          tokens_per_second)
    return build_segments(lines, words, prepend_punctuations, append_punctuations, max_cue_chars), stats
