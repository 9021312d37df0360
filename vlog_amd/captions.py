"""Caption shaping: the segments of a transcribe call cut into caption-sized cues, the host side.

A `Segment` is whatever Whisper's timestamp tokens delimit: one word, or 30 s and several hundred characters.  The
worker writes one WebVTT cue per segment, so with shaping on (`max_line_width`, `VLOG_AMD_MAX_LINE_WIDTH`) the
stream's last stage turns every segment that has word times into cues of at most `max_line_count` lines of at most
`max_line_width` characters (openai-whisper's --max_line_width / --max_line_count, which need word timestamps too).

No torch and no GPU in this module; the segments are any dataclass with the fields of `transcribe.Segment`, the
words any object with `word`, `start`, `end` (tests drive the rule on a CPU).

  shape_captions           the rule, a streaming generator over the final segment stream
  resolve_caption_options  the three arguments of the transcribe calls and their environment variables
  word_tokens              the text tokens an aligned word carries (transcribe attaches them to its Words)
"""
from __future__ import annotations

import dataclasses
import numbers
from typing import Iterable, Iterator, List, Mapping, Optional, Sequence, Tuple

from .forced_align import SENTENCE_END

# A pause between two words longer than this starts a new cue.  A design choice, not a measurement: the speech
# pads of the VAD (0.4 s a side) and its 2 s minimum silence put a removed silence at about 3 s or more between
# the words around it, and a caption that stays up over that long a silence reads as stuck.
CUE_BREAK_PAUSE_S = 3.0

MAX_LINE_COUNT = 4                      # the most lines a cue may be asked to hold
DEFAULT_LINE_COUNT = 2

ENV_WIDTH = "VLOG_AMD_MAX_LINE_WIDTH"
ENV_COUNT = "VLOG_AMD_MAX_LINE_COUNT"
ENV_SECONDS = "VLOG_AMD_MAX_CUE_SECONDS"


def word_tokens(word) -> List[int]:
    """The text tokens of an aligned word: find_alignment splits the window's tokens into words and
    merge_punctuations moves them with the words; transcribe keeps them on every `Word` it builds as the private
    attribute `_tokens` (no dataclass field: ==, repr and _asdict() are the four public fields').  A word from
    elsewhere has none."""
    return list(getattr(word, "_tokens", ()))


def set_word_tokens(word, tokens: Sequence[int]):
    """Puts the word's text tokens where word_tokens finds them; -> the word."""
    word._tokens = list(tokens)
    return word


def _cue_text(lines: Sequence[str]) -> str:
    return "\n".join(l.strip() for l in lines)


def shape_captions(segments: Iterable, max_line_width: int, max_line_count: int = DEFAULT_LINE_COUNT,
                   max_cue_seconds: Optional[float] = None) -> Iterator:
    """The final segment stream (after restore_speech_timestamps: the times are the file's own, so a silence the VAD
    removed is a pause) -> caption cues, ids 1, 2, ... in output order.

    A segment (a "parent") without words passes through with the new id.  A parent with words becomes one or more
    cues; no cue spans two parents, and a parent's cues are yielded before the next parent is pulled.  One greedy
    pass over the parent's words, those with empty text skipped:

      lines  a word joins the current line when len((line + word).strip()) <= max_line_width, else it opens a new
             line; a word wider than the limit has a line to itself and is never split.
      cues   a new cue starts before word i > 0 when
             1. the word needs a new line and the cue has max_line_count lines already;
             2. word[i].start - word[i-1].end > CUE_BREAK_PAUSE_S;
             3. max_cue_seconds is set and word[i].end - (the cue's first word).start > max_cue_seconds (so a word
                longer than the limit is a cue of its own);
             4. word[i-1] ends in one of forced_align.SENTENCE_END and the cue's text (its stripped lines joined by
                "\\n", as it would be emitted without the leading space) already holds at least half of
                max_line_width * max_line_count characters (forced_align.shape_cues' rule).

    A cue has the parent's seek, avg_logprob, compression_ratio, no_speech_prob and temperature; start / end are its
    first word's start and last word's end; text is its stripped lines joined by "\\n", with one leading space iff the
    parent's text had one; words are the parent's word objects, untouched.  tokens: the text tokens of the cue's
    words (word_tokens), so they decode to the cue's text.  Over a parent's cues they are the parent's tokens below
    <|endoftext|> in order whenever the parent's words are made of exactly its tokens; add_word_timestamps gives a
    word that runs across a timestamp pair to the earlier segment whole, and its tokens go where the word goes.  A
    parent whose words carry no tokens (none built by transcribe) leaves its tokens, as they are, on its first cue."""
    if max_line_width < 1:
        raise ValueError(f"max_line_width must be >= 1, got {max_line_width}")
    if not 1 <= max_line_count <= MAX_LINE_COUNT:
        raise ValueError(f"max_line_count must be between 1 and {MAX_LINE_COUNT}, got {max_line_count}")
    if max_cue_seconds is not None and not max_cue_seconds > 0:
        raise ValueError(f"max_cue_seconds must be > 0, got {max_cue_seconds}")
    capacity = max_line_width * max_line_count
    next_id = 1
    for parent in segments:
        words = [w for w in (parent.words or []) if w.word]
        if not words:
            yield dataclasses.replace(parent, id=next_id)
            next_id += 1
            continue
        cues: List[Tuple[list, List[str]]] = []         # (words, lines)
        cue: list = []
        lines: List[str] = []
        for w in words:
            new_line = bool(cue) and len((lines[-1] + w.word).strip()) > max_line_width
            if cue:
                prev = cue[-1]
                tail = prev.word.strip()
                if (new_line and len(lines) == max_line_count) \
                        or w.start - prev.end > CUE_BREAK_PAUSE_S \
                        or (max_cue_seconds is not None and w.end - cue[0].start > max_cue_seconds) \
                        or (tail and tail[-1] in SENTENCE_END and 2 * len(_cue_text(lines)) >= capacity):
                    cues.append((cue, lines))
                    cue, lines, new_line = [], [], False
            if not cue or new_line:
                lines.append(w.word)
            else:
                lines[-1] += w.word
            cue.append(w)
        cues.append((cue, lines))
        lead = " " if parent.text.startswith(" ") else ""
        known = any(hasattr(w, "_tokens") for w in words)
        for k, (cue, lines) in enumerate(cues):
            if known:
                tokens = [t for w in cue for t in word_tokens(w)]
            else:
                tokens = list(parent.tokens) if k == 0 else []
            yield dataclasses.replace(parent, id=next_id, start=cue[0].start, end=cue[-1].end,
                                      text=lead + _cue_text(lines), tokens=tokens, words=cue)
            next_id += 1


def _parse(environ: Mapping[str, str], name: str, kind):
    raw = environ.get(name, "")
    if raw is None or not str(raw).strip():
        return None
    try:
        return kind(str(raw).strip())
    except ValueError:
        raise ValueError(f"{name} must be {'an integer' if kind is int else 'a number'}, got {raw!r}") from None


def resolve_caption_options(max_line_width: Optional[int], max_line_count: Optional[int],
                            max_cue_seconds: Optional[float], environ: Mapping[str, str]
                            ) -> Optional[Tuple[int, int, Optional[float]]]:
    """The caption arguments of a transcribe call and the environment -> (max_line_width, max_line_count,
    max_cue_seconds) as shape_captions takes them, or None: shaping is off.

    max_line_width=None reads VLOG_AMD_MAX_LINE_WIDTH (unset or empty: 0).  Shaping is on iff the width is > 0, so
    max_line_width=0 turns it off whatever the environment says.  While it is on, max_line_count=None reads
    VLOG_AMD_MAX_LINE_COUNT (default 2) and max_cue_seconds=None reads VLOG_AMD_MAX_CUE_SECONDS (default: no limit);
    while it is off those two variables are not looked at.  ValueError: a negative width, a count outside 1..4,
    seconds <= 0 (or not finite), a count or seconds argument while shaping is off, and an environment value that
    does not parse, naming the variable."""
    def integer(v, name):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{name} must be an integer, got {v!r}")
        return int(v)

    if max_line_width is None:
        width, source = _parse(environ, ENV_WIDTH, int) or 0, ENV_WIDTH
    else:
        width, source = integer(max_line_width, "max_line_width"), "max_line_width"
    if width < 0:
        raise ValueError(f"{source} must be >= 0, got {width}")
    if width == 0:
        for name, v in (("max_line_count", max_line_count), ("max_cue_seconds", max_cue_seconds)):
            if v is not None:
                raise ValueError(f"{name}={v!r} needs caption shaping on (max_line_width or {ENV_WIDTH} > 0)")
        return None
    if max_line_count is None:
        count, source = _parse(environ, ENV_COUNT, int), ENV_COUNT
        count = DEFAULT_LINE_COUNT if count is None else count
    else:
        count, source = integer(max_line_count, "max_line_count"), "max_line_count"
    if not 1 <= count <= MAX_LINE_COUNT:
        raise ValueError(f"{source} must be between 1 and {MAX_LINE_COUNT}, got {count}")
    if max_cue_seconds is None:
        seconds, source = _parse(environ, ENV_SECONDS, float), ENV_SECONDS
    else:
        if isinstance(max_cue_seconds, bool) or not isinstance(max_cue_seconds, numbers.Real):
            raise ValueError(f"max_cue_seconds must be a number, got {max_cue_seconds!r}")
        seconds, source = float(max_cue_seconds), "max_cue_seconds"
    if seconds is not None and not (0 < seconds < float("inf")):
        raise ValueError(f"{source} must be a finite number > 0, got {seconds}")
    return width, count, seconds
