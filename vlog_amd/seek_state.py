"""The sequential (parity) mode's host state, one object per file, and the lockstep scheduler over several files.

faster-whisper `generate_segments` [FW↑ 1.1.x] is a loop over one file: seek position, clip list, previous-text
prompt, temperature fallback, segment split, word alignment.  Here the loop's body is an object with two operations,
so that one driver can hold several files and decode the next window of each in shared decoder passes
(`WhisperModel.transcribe_many`), while `WhisperModel.generate_segments` stays the one-file driver:

  SeekState.next_request() -> the next window to decode (seek, size, prompt, seed base), or None at the file's end
  SeekState.consume(...)   -> takes the window's decode result, returns the segments to yield

The same scheduler decodes the sections of ONE file (`WhisperModel.transcribe(sections=N)`): plan_sections cuts the
file at long silences, and each section is a SeekState confined to its frame range (clip_frames).

Nothing here touches the GPU (no torch import): the decode, the fallback passes and the alignment are callables the
driver supplies, so tests run both the state and the scheduler against a scripted backend.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

from . import segments as segs
from .dims import HOP_LENGTH, N_FRAMES, SAMPLE_RATE

FRAMES_PER_SECOND = SAMPLE_RATE // HOP_LENGTH


@dataclass
class WindowRequest:
    window: int            # the file's window counter: the seed of temperature i is window + i
    seek: int
    size: int              # mel frames of the window
    time_offset: float
    duration: float
    prompt: List[int]
    max_length: int        # total decoder length of this window, prompt included
    # multilingual=True: the language code the prompt carries (a placeholder until the window's first decode has
    # detected its language: SeekState.set_window_language) and that token's position in the prompt; else None / -1
    language: Optional[str] = None
    lang_pos: int = -1


def window_max_length(prompt: Sequence[int], max_new_tokens: Optional[int], model_max_length: int) -> int:
    """faster-whisper generate_with_fallback's max_length: len(prompt) + max_new_tokens, within the model's."""
    max_length = len(prompt) + max_new_tokens if max_new_tokens is not None else model_max_length
    if max_length > model_max_length:
        raise ValueError(f"the length of the prompt is {len(prompt)}, and the max_new_tokens {max_length - len(prompt)}. "
                         f"Thus, the combined length of the prompt and max_new_tokens is: {max_length}. This exceeds "
                         f"the max_length of the Whisper model: {model_max_length}.")
    return max_length


ACCEPTED, NEXT, EXHAUSTED = "accepted", "next", "exhausted"


class FallbackLadder:
    """faster-whisper generate_with_fallback as a resumable object, so a driver can hold one per window and decode
    the windows that fail a temperature together (decode_round_levels) instead of looping over one window.

      request()      -> (temperature, seed) of the decode whose result the ladder waits for: temperature `level` of
                        options.temperatures with seed + level
      judge(result)  -> ACCEPTED (the result stands), NEXT (it needs a fallback: request() names the next decode) or
                        EXHAUSTED (every temperature failed: the best of those below the compression-ratio
                        threshold, or of all, stands, reported at the last temperature)
      result()       -> (result, avg_logprob, temperature, compression_ratio), once `done`

    `done` is set from the start when the temperature list is empty; result() then fails as the loop form did."""

    def __init__(self, decode_text: Callable[[Sequence[int]], str], options, seed: int = 0):
        self.decode_text = decode_text
        self.options = options
        self.seed = seed
        self.level = 0
        self.done = not options.temperatures
        self._all: List[tuple] = []
        self._below_cr: List[tuple] = []
        self._decode: Optional[tuple] = None

    def request(self) -> Tuple[float, int]:
        if self.done:
            raise RuntimeError("FallbackLadder.request after the ladder ended")
        return self.options.temperatures[self.level], self.seed + self.level

    def judge(self, result) -> str:
        if self.done:
            raise RuntimeError("FallbackLadder.judge after the ladder ended")
        o = self.options
        temperature = o.temperatures[self.level]
        n = len(result.tokens)
        avg_lp = segs.avg_logprob(result.score, n, o.length_penalty)
        text = self.decode_text(result.tokens).strip()
        cr = segs.compression_ratio(text)
        decode_result = (result, avg_lp, temperature, cr)
        self._all.append(decode_result)
        fb, below = segs.needs_fallback(cr, avg_lp, result.no_speech_prob, o.compression_ratio_threshold,
                                        o.log_prob_threshold, o.no_speech_threshold)
        if below:
            self._below_cr.append(decode_result)
        if not fb:
            self._decode, self.done = decode_result, True
            return ACCEPTED
        if self.level + 1 < len(o.temperatures):
            self.level += 1
            return NEXT
        best = max(self._below_cr or self._all, key=lambda x: x[1])
        self._decode, self.done = (best[0], best[1], temperature, best[3]), True
        return EXHAUSTED

    def result(self) -> tuple:
        if not self.done:
            raise RuntimeError("FallbackLadder.result before the ladder ended")
        if self._decode is None:                # no temperature at all: nothing to choose from
            raise ValueError("fallback ladder without temperatures")
        return self._decode


def fallback_ladder(generate: Callable[[float, int], object], decode_text: Callable[[Sequence[int]], str], options,
                    seed: int = 0, first=None):
    """faster-whisper generate_with_fallback -> (result, avg_logprob, temperature, compression_ratio).
    generate(temperature, seed) -> an object with tokens / score / no_speech_prob; temperature i runs with seed + i.
    `first`: the result at temperatures[0] when a shared pass already computed it (the ladder then starts by judging
    it, and calls generate only for the temperatures after it).  The loop over one FallbackLadder."""
    ladder = FallbackLadder(decode_text, options, seed)
    while not ladder.done:
        ladder.judge(first if (ladder.level == 0 and first is not None) else generate(*ladder.request()))
    return ladder.result()


def _get_end(segments: List[dict]) -> Optional[float]:
    return next((w["end"] for s in reversed(segments) for w in reversed(s.get("words") or [])),
                segments[-1]["end"] if segments else None)


class SeekState:
    """One file's position in the sequential mode: seek, clips, previous text, window counter, segment id."""

    def __init__(self, content_frames: int, tokenizer, options, model_max_length: int = 448,
                 frames_per_second: int = FRAMES_PER_SECOND, clip_frames: Optional[Tuple[int, int]] = None):
        """clip_frames: one exact (start, end) frame range that replaces the clip list of options.clip_timestamps (a
        section of plan_sections).  The state is then a file of its own between those frames: `prefix` applies only
        where seek == 0 (so to the section that starts the file), `initial_prompt` seeds this section's history as it
        seeds a file's, and the window counter (so the fallback seeds window + i) starts at 0."""
        self.content_frames = content_frames
        self.tokenizer = tokenizer
        self.options = options
        self.model_max_length = model_max_length
        self.frames_per_second = frames_per_second
        if clip_frames is not None:
            self.seek_clips = [(int(clip_frames[0]), int(clip_frames[1]))]
        else:
            ct = options.clip_timestamps
            if isinstance(ct, str):
                ct = [float(t) for t in (ct.split(",") if ct else [])]
            seek_points = [round(t * frames_per_second) for t in ct]
            if not seek_points:
                seek_points.append(0)
            if len(seek_points) % 2 == 1:
                seek_points.append(content_frames)
            self.seek_clips = list(zip(seek_points[::2], seek_points[1::2]))
        self.idx = 0                    # id of the last segment yielded
        self.clip_idx = 0
        self.seek = self.seek_clips[0][0]
        self.all_tokens: List[int] = []
        self.prompt_reset_since = 0
        if options.initial_prompt is not None:
            if isinstance(options.initial_prompt, str):
                self.all_tokens.extend(tokenizer.encode(" " + options.initial_prompt.strip()))
            else:
                self.all_tokens.extend(options.initial_prompt)
        self.last_speech_timestamp = 0.0
        self.window = 0
        self._request: Optional[WindowRequest] = None
        # multilingual=True (faster-whisper's code switching): every window is decoded under the language detected for
        # it.  `language` is the code the next window's prompt starts from: the file's, then the previous window's.
        # An English-only tokenizer has no language token: the option is off.
        self.multilingual = bool(getattr(options, "multilingual", False)) and \
            getattr(tokenizer, "language", None) is not None
        self.language: Optional[str] = tokenizer.language_code if self.multilingual else None

    def next_request(self) -> Optional[WindowRequest]:
        """The window to decode next (the same object until it is consumed), or None when the file is done."""
        if self._request is not None:
            return self._request
        o, tk = self.options, self.tokenizer
        while self.clip_idx < len(self.seek_clips):
            clip_start, clip_end = self.seek_clips[self.clip_idx]
            clip_end = min(clip_end, self.content_frames)
            if self.seek < clip_start:
                self.seek = clip_start
            if self.seek >= clip_end:
                self.clip_idx += 1
                if self.clip_idx < len(self.seek_clips):
                    self.seek = self.seek_clips[self.clip_idx][0]
                continue
            seek = self.seek
            size = min(N_FRAMES, self.content_frames - seek, clip_end - seek)
            if self.multilingual:
                tk = tk.for_language(self.language)
            prompt = segs.build_prompt(tk.encode, tk.sot_sequence, tk.sot_prev, tk.no_timestamps, tk.timestamp_begin,
                                       self.model_max_length, self.all_tokens[self.prompt_reset_since:],
                                       o.without_timestamps, prefix=o.prefix if seek == 0 else None, hotwords=o.hotwords)
            self._request = WindowRequest(window=self.window, seek=seek, size=size,
                                          time_offset=seek * HOP_LENGTH / SAMPLE_RATE,
                                          duration=size * HOP_LENGTH / SAMPLE_RATE, prompt=prompt,
                                          max_length=window_max_length(prompt, o.max_new_tokens, self.model_max_length))
            if self.multilingual:
                self._request.language = self.language
                self._request.lang_pos = prompt.index(tk.sot) + 1
            return self._request
        return None

    def set_window_language(self, code: Optional[str]) -> None:
        """multilingual=True: the language the pending window's first decode detected (the `language` of its result;
        faster-whisper detects once per window, before the fallback loop).  The request's prompt then carries that
        language's token, so every fallback temperature decodes under it, and consume() aligns and labels the window
        with it and hands it to the next window as its placeholder.  A no-op with the option off or code None."""
        req = self._request
        if req is None:
            raise RuntimeError("SeekState.set_window_language without a pending request")
        if not self.multilingual or code is None:
            return
        req.prompt[req.lang_pos] = self.tokenizer.for_language(code).language
        req.language = code

    def consume(self, decode_result: Tuple[object, float, float, float],
                align: Optional[Callable[[List[dict], int, float], float]] = None) -> List[dict]:
        """Takes the pending window's (result, avg_logprob, temperature, compression_ratio) and returns the segments
        to yield, as dicts with the fields of `Segment` (words: the aligned word dicts or None).
        align(current_segments, segment_size, last_speech_timestamp) -> last_speech_timestamp adds the word times in
        place (word_timestamps; it runs before the seek position is final, which depends on the last word's end).
        multilingual=True: the window's language is its request's (set_window_language); align is then called with
        tokenizer=<that language's tokenizer> (its sot_sequence and word splitting), every segment dict carries
        language=<code>, and the next window's prompt starts from it.
        The two halves, for a driver that aligns several states' windows in one call: begin_consume, finish_consume."""
        item = self.begin_consume(decode_result)
        if item is None:
            return self.finish_consume()
        current, size, last, tk = item
        if self.multilingual:
            return self.finish_consume(align(current, size, last, tokenizer=tk))
        return self.finish_consume(align(current, size, last))

    def begin_consume(self, decode_result: Tuple[object, float, float, float]):
        """The first half of consume: everything before the word alignment.  -> None when nothing is to be aligned (the
        window is skipped as silence, or word_timestamps is off), else (current_segments, segment_size,
        last_speech_timestamp, tokenizer): the caller adds the word times to current_segments in place, under that
        tokenizer (the window's language's with multilingual=True), and passes the new last-speech time to
        finish_consume."""
        req = self._request
        if req is None:
            raise RuntimeError("SeekState.consume without a pending request")
        self._request = None
        o, tk = self.options, self.tokenizer
        result, avg_lp, temperature, cr = decode_result
        self.window += 1
        if self.multilingual:
            self.language = req.language
        if segs.should_skip_window(result.no_speech_prob, avg_lp, o.no_speech_threshold, o.log_prob_threshold):
            self.seek += req.size
            self._begun = (req, decode_result, None, True)
            return None
        current, self.seek, single_ending = segs.split_segments_by_timestamps(
            result.tokens, tk.timestamp_begin, req.time_offset, req.size, req.duration, req.seek)
        self._begun = (req, decode_result, current, single_ending)
        if not o.word_timestamps:
            return None
        return current, req.size, self.last_speech_timestamp, tk.for_language(req.language) if self.multilingual else tk

    def finish_consume(self, last_speech_timestamp: Optional[float] = None) -> List[dict]:
        """The second half of consume: last_speech_timestamp is the alignment's (None when begin_consume returned
        None).  -> the segments to yield."""
        begun, self._begun = getattr(self, "_begun", None), None
        if begun is None:
            raise RuntimeError("SeekState.finish_consume without begin_consume")
        req, (result, avg_lp, temperature, cr), current, single_ending = begun
        if current is None:
            return []
        o, tk = self.options, self.tokenizer
        if o.word_timestamps:
            self.last_speech_timestamp = last_speech_timestamp
            if not single_ending:
                last_word_end = _get_end(current)
                if last_word_end is not None and last_word_end > req.time_offset:
                    self.seek = round(last_word_end * self.frames_per_second)
        out = []
        for s in current:
            text = tk.decode(s["tokens"])
            if s["start"] == s["end"] or not text.strip():
                continue
            self.all_tokens.extend(s["tokens"])
            self.idx += 1
            out.append(dict(id=self.idx, seek=req.seek, start=s["start"], end=s["end"], text=text, tokens=s["tokens"],
                            temperature=temperature, avg_logprob=avg_lp, compression_ratio=cr,
                            no_speech_prob=result.no_speech_prob, words=s["words"] if o.word_timestamps else None))
            if self.multilingual:
                out[-1]["language"] = req.language
        if not o.condition_on_previous_text or temperature > o.prompt_reset_on_temperature:
            self.prompt_reset_since = len(self.all_tokens)
        return out


def consume_round_grouped(batch, decodes, align_group, emit) -> None:
    """The consume step of a lockstep round whose word alignment is grouped by language: every entry's window is split
    (begin_consume), the entries with something to align are grouped by their tokenizer's sot sequence (with
    multilingual=True the window's language's), align_group(items) is called ONCE per distinct sot sequence with
    items = [(entry index, current_segments, segment_size, last_speech_timestamp, tokenizer)] in batch order and returns
    one new last-speech time per item (each item keeps its own: the entries are different files or sections), and every
    entry is finished and emitted in batch order."""
    items = []
    for i, (_, state, _) in enumerate(batch):
        item = state.begin_consume(decodes[i])
        if item is not None:
            items.append((i,) + tuple(item))
    groups: dict = {}
    for it in items:
        groups.setdefault(tuple(it[4].sot_sequence), []).append(it)
    lasts: dict = {}
    for group in groups.values():
        out = align_group(group)
        if len(out) != len(group):
            raise RuntimeError("consume_round_grouped: align_group must return one last-speech time per item")
        for it, last in zip(group, out):
            lasts[it[0]] = last
    for i, (f, state, _) in enumerate(batch):
        emit(f, state.finish_consume(lasts.get(i)))


def _grouped(batch, align, align_group) -> bool:
    """a round aligns by language groups when the driver can (align_group) and some entry has multilingual on; every
    other round keeps its one alignment call per entry, as before"""
    return align is not None and align_group is not None and any(state.multilingual for _, state, _ in batch)


def run_lockstep(n_files: int, max_files: int, open_file: Callable[[int], SeekState],
                 decode_round: Callable[[List[Tuple[int, SeekState, WindowRequest]]], None],
                 close_file: Optional[Callable[[int], None]] = None) -> int:
    """Decodes n_files files with at most max_files in flight.  Each round takes the next window of every file in
    flight, in the order the files entered (entry i of the round is cross slot i), and hands them to
    decode_round([(file, state, request)]), which must consume every request.  When a file ends, the next pending
    file takes its place in the following round; close_file(file) is called once a file has no window left (the
    driver drops what it held for it).  -> the number of rounds."""
    if max_files < 1:
        raise ValueError("max_files must be >= 1")
    return sum(1 for _ in iter_lockstep(n_files, max_files, open_file, decode_round, close_file))


def iter_lockstep(n_files: int, max_files: int, open_file: Callable[[int], SeekState],
                  decode_round: Callable[[List[Tuple[int, SeekState, WindowRequest]]], None],
                  close_file: Optional[Callable[[int], None]] = None):
    """run_lockstep as a generator: yields the round's batch after every decode_round, so a driver that streams its
    output (the sections of one file) can hand on what the round made final before the next round starts."""
    if max_files < 1:
        raise ValueError("max_files must be >= 1")
    pending = deque(range(n_files))
    active: List[Tuple[int, SeekState]] = []
    while pending or active:
        batch: List[Tuple[int, SeekState, WindowRequest]] = []
        keep: List[Tuple[int, SeekState]] = []
        for f, state in active:
            req = state.next_request()
            if req is not None:
                batch.append((f, state, req))
                keep.append((f, state))
            elif close_file is not None:
                close_file(f)
        while pending and len(keep) < max_files:
            f = pending.popleft()
            state = open_file(f)
            req = state.next_request()
            if req is not None:                 # (an empty file never enters a round)
                batch.append((f, state, req))
                keep.append((f, state))
            elif close_file is not None:
                close_file(f)
        active = keep
        if not batch:
            continue
        decode_round(batch)
        for _, state, _ in batch:
            if state._request is not None:
                raise RuntimeError("run_lockstep: decode_round left a request unconsumed")
        yield batch


def decode_round_with(batch: Sequence[Tuple[int, SeekState, WindowRequest]],
                      first_pass: Callable[[List[int]], List[object]],
                      fallback_generate: Callable[[int, float, int], object],
                      align: Optional[Callable[[int, List[dict], int, float], float]],
                      emit: Callable[[int, List[dict]], None], align_group=None) -> None:
    """One lockstep round over `batch` (entry i = cross slot i).
    first_pass(indices) -> the results at temperatures[0] of those entries, decoded together (the caller may split
    them further, e.g. by suppress list); with multilingual=True each result's `language` is the code detected for its
    window, which the entry's request takes before any fallback (SeekState.set_window_language), and align receives
    tokenizer=<that language's>; fallback_generate(i, temperature, seed) re-decodes entry i alone, for the
    temperatures after the first; align(i, segments, size, last_speech) word-aligns entry i against its own slot;
    emit(file, segments) receives each file's new segments.
    align_group (consume_round_grouped): with it, a round in which some entry has multilingual on aligns its entries
    in ONE call per distinct language among them instead of one call per entry; the ladders all run first."""
    firsts = first_pass(list(range(len(batch))))
    if _grouped(batch, align, align_group):
        decodes = []
        for i, (f, state, req) in enumerate(batch):
            state.set_window_language(getattr(firsts[i], "language", None))
            decodes.append(fallback_ladder(lambda t, seed, i=i: fallback_generate(i, t, seed), state.tokenizer.decode,
                                           state.options, seed=req.window, first=firsts[i]))
        consume_round_grouped(batch, decodes, align_group, emit)
        return
    for i, (f, state, req) in enumerate(batch):
        state.set_window_language(getattr(firsts[i], "language", None))
        decode = fallback_ladder(lambda t, seed, i=i: fallback_generate(i, t, seed), state.tokenizer.decode, state.options,
                                 seed=req.window, first=firsts[i])
        emit(f, state.consume(decode, (lambda cur, size, last, i=i, **kw: align(i, cur, size, last, **kw)) if align else None))


def decode_round_levels(batch: Sequence[Tuple[int, SeekState, WindowRequest]],
                        first_pass: Callable[[List[int]], List[object]],
                        level_pass: Callable[[List[int], float, List[int]], List[object]],
                        align: Optional[Callable[[int, List[dict], int, float], float]],
                        emit: Callable[[int, List[dict]], None], align_group=None) -> None:
    """decode_round_with (align_group included) with the fallback ladder walked by LEVELS: the entries whose result at temperature i - 1
    needs a fallback are re-decoded together.
    first_pass(indices): as decode_round_with.  level_pass(indices, temperature, seeds) -> the results of those
    entries at `temperature`, entry k with seeds[k]; level i is called once, with the entries still failing in batch
    order, temperatures[i] (the list is common to the round's entries) and seeds [req.window + i]; an accepted entry
    never appears again, and a level nobody needs is not called.  Once no entry is left, every entry is consumed and
    emitted in batch order, word-aligned (align, at consume time) against its own slot.  Per entry the decode tuple
    is what fallback_ladder returns for the same results."""
    firsts = first_pass(list(range(len(batch))))
    for i, (_, state, _) in enumerate(batch):
        state.set_window_language(getattr(firsts[i], "language", None))
    ladders = [FallbackLadder(state.tokenizer.decode, state.options, seed=req.window) for _, state, req in batch]
    failing = [i for i, ladder in enumerate(ladders) if not ladder.done and ladder.judge(firsts[i]) == NEXT]
    while failing:
        requests = [ladders[i].request() for i in failing]
        temperature = requests[0][0]
        if any(t != temperature for t, _ in requests):
            raise ValueError("decode_round_levels: the entries of a round must share one temperature list")
        results = level_pass(list(failing), temperature, [s for _, s in requests])
        if len(results) != len(failing):
            raise RuntimeError("decode_round_levels: level_pass must return one result per entry")
        failing = [i for i, r in zip(failing, results) if ladders[i].judge(r) == NEXT]
    if _grouped(batch, align, align_group):
        consume_round_grouped(batch, [ladder.result() for ladder in ladders], align_group, emit)
        return
    for i, (f, state, req) in enumerate(batch):
        emit(f, state.consume(ladders[i].result(),
                              (lambda cur, size, last, i=i, **kw: align(i, cur, size, last, **kw)) if align else None))


# ---------------------------------------------------------------------------------------------------- sections
# One long file cut at a few long silences into contiguous sections, each decoded by a SeekState of its own
# (clip_frames) while run_lockstep / iter_lockstep decodes the sections together as it decodes files.  The three
# thresholds below are design choices, not measurements.
MAX_SECTIONS = 32
SECTION_MIN_JOIN_SILENCE_S = 0.5    # a VAD join is a cut candidate only when at least this much silence was removed there
SECTION_JOIN_REACH = 0.5            # a join may lie this fraction of an even section's length away from its target
SECTION_ENERGY_REACH_S = 3.0        # without VAD, the quietest 20 ms frame is sought this far to each side of a target
ENERGY_FRAME_MEL = 2                # a wm_frame_energy frame of 320 samples is two mel frames


def chunk_joins(speech_chunks: Sequence[dict], hop_length: int = HOP_LENGTH,
                sampling_rate: int = SAMPLE_RATE) -> List[Tuple[int, float]]:
    """[(frame, removed_silence_seconds)] for plan_sections: one entry per boundary between two collected speech
    chunks (vad.collect_chunks), at the cumulative chunk samples // hop_length of the concatenated audio."""
    out: List[Tuple[int, float]] = []
    cum = 0
    for a, b in zip(speech_chunks[:-1], speech_chunks[1:]):
        cum += a["end"] - a["start"]
        out.append((cum // hop_length, (b["start"] - a["end"]) / sampling_rate))
    return out


def plan_sections(content_frames: int, n: int, joins: Optional[Sequence[Tuple[int, float]]] = None,
                  energy: Optional[Sequence[float]] = None) -> List[Tuple[int, int]]:
    """Contiguous frame ranges [(start, end)] that cover [0, content_frames), at most n of them, each at least
    N_FRAMES long; in mel frames of the audio the seek loop sees (after VAD concatenation).  The result depends on the
    arguments alone.

    Cut j aims at t_j = round(j * content_frames / n).  With `joins` (VAD ran; see chunk_joins) it is the join nearest
    to t_j among those with >= SECTION_MIN_JOIN_SILENCE_S removed and within SECTION_JOIN_REACH * content_frames / n
    frames of t_j (ties: the longer silence, then the lower frame); a target without such a join loses its cut, so a
    speech chunk is never cut.  With `energy` (dB per 20 ms frame, engine.frame_energy_db(audio, 320)) it is the first
    mel frame of the quietest energy frame within SECTION_ENERGY_REACH_S of t_j (ties: nearest to t_j, then the lower).
    With neither, the cuts are the targets.  A file too short for n sections of N_FRAMES gets fewer targets, and cuts
    that would still leave a section shorter than N_FRAMES are dropped, first the one whose shorter neighbouring
    section is shortest (ties: the lower frame)."""
    if not 1 <= n <= MAX_SECTIONS:
        raise ValueError(f"sections must be between 1 and {MAX_SECTIONS}, got {n}")
    content_frames = max(int(content_frames), 0)
    n = max(1, min(n, content_frames // N_FRAMES))
    cuts = set()
    for j in range(1, n):
        t = round(j * content_frames / n)
        if joins is not None:
            reach = SECTION_JOIN_REACH * content_frames / n
            cand = [(abs(f - t), -s, f) for f, s in joins
                    if s >= SECTION_MIN_JOIN_SILENCE_S and abs(f - t) <= reach and 0 < f < content_frames]
            if cand:
                cuts.add(min(cand)[2])
        elif energy is not None:
            reach = int(SECTION_ENERGY_REACH_S * FRAMES_PER_SECOND)
            lo = max(0, -((reach - t) // ENERGY_FRAME_MEL))             # ceil((t - reach) / 2)
            hi = min(len(energy) - 1, (t + reach) // ENERGY_FRAME_MEL)
            cand = [(float(energy[e]), abs(e * ENERGY_FRAME_MEL - t), e) for e in range(lo, hi + 1)]
            if cand:
                f = min(cand)[2] * ENERGY_FRAME_MEL
                if 0 < f < content_frames:
                    cuts.add(f)
        else:
            cuts.add(t)
    cuts = sorted(cuts)
    while cuts:
        edges = [0] + cuts + [content_frames]
        lengths = [b - a for a, b in zip(edges[:-1], edges[1:])]
        if min(lengths) >= N_FRAMES:
            break
        cuts.remove(min(cuts, key=lambda c: (min(lengths[cuts.index(c)], lengths[cuts.index(c) + 1]), c)))
    edges = [0] + cuts + [content_frames]
    return list(zip(edges[:-1], edges[1:]))
