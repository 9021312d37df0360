"""The sequential mode's per-file state (vlog_amd/seek_state.py) and the lockstep scheduler, on the CPU with a scripted
decoder: no torch device, no engine.

The script's `generate` returns tokens as a deterministic function of (file, seek of the window, a hash of the prompt,
temperature), so handing a window another file's prompt, seek, seed or slot changes the output.  Every file's segments
must equal oracle.transcribe.transcribe driven by the SAME script (the independent restatement of faster-whisper's
loop that the GPU seek-loop tests use).  One window is skipped as silence and one triggers the temperature fallback.
Also: the ctypes mirror of wm_generate_args against the struct the host compiler builds from the header."""
import ctypes
import hashlib
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import transcribe as otr
from vlog_amd import _capi
from vlog_amd.dims import model_dims
from vlog_amd.seek_state import SeekState, decode_round_with, fallback_ladder, run_lockstep
from vlog_amd.tokenizer import Tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = model_dims("tiny")
ST = DIMS.specials
TEMPS = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
# content frames per file (unequal; the third has a window the script marks silent, the fourth one that falls back)
FRAMES = [7500, 2100, 4800, 3000, 3300]
SILENT = (2, 0)          # (file, index of the window in decode order): no_speech_prob high, score low -> skipped
FALLBACK = (3, 0)        # its T = 0 result scores below the log-prob threshold; T = 0.2 is fine


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


def _features(f):
    """[n_mels, frames + 1] whose first two rows name the file and the frame: a window's first column identifies it"""
    n = FRAMES[f] + 1
    x = np.zeros((DIMS.n_mels, n), np.float32)
    x[0] = f
    x[1] = np.arange(n)
    return x


class Script:
    """The scripted decoder.  `calls` logs (file, seek, temperature, seed, n_prompt) of every generate."""

    def __init__(self):
        self.calls = []
        self.windows = {}        # file -> seeks in decode order

    def result(self, f, seek, prompt, temperature, seed):
        order = self.windows.setdefault(f, [])
        if seek not in order:
            order.append(seek)
        wi = order.index(seek)
        self.calls.append((f, seek, temperature, seed, len(prompt)))
        h = int.from_bytes(hashlib.sha256(repr((f, seek, tuple(prompt), round(temperature, 3), seed)).encode()).digest()[:8],
                           "little")
        rng = np.random.default_rng(h)
        tb = ST.timestamp_begin
        n_seg = int(rng.integers(1, 4))
        toks, t = [], int(rng.integers(0, 20))
        for k in range(n_seg):
            toks.append(tb + t)
            toks.extend(int(x) for x in rng.integers(300, ST.eot - 1, size=int(rng.integers(3, 9))))
            t += int(rng.integers(100, 400))
            last_open = k == n_seg - 1 and rng.random() < 0.4
            if not last_open:
                toks.append(tb + min(t, 1500))
        score, ns = -0.3 - 0.2 * float(rng.random()), 0.05
        if (f, wi) == SILENT:
            score, ns = -1.6, 0.9
        if (f, wi) == FALLBACK and temperature == 0.0:
            score = -1.5
        return SimpleNamespace(tokens=toks, score=score, no_speech_prob=ns)

    # ---- oracle.transcribe backend
    def encode(self, window):
        return (int(round(float(window[0, 0]))), int(round(float(window[1, 0]))))

    def generate(self, cross, prompt, opt):
        return self.result(cross[0], cross[1], prompt, opt.sampling_temperature, opt.seed)


def _oracle(f, script, **kw):
    model = SimpleNamespace(dims=DIMS)
    out, _ = otr.transcribe(model, _tok, np.zeros(1, np.float32), beam_size=5, temperatures=TEMPS, suppress_tokens=[],
                            language="en", features=_features(f), backend=script, **kw)
    return out


def _key(segments):
    return [(s["start"], s["end"], s["tokens"], s["temperature"], round(s["avg_logprob"], 9), s["no_speech_prob"])
            for s in segments]


def _drive_one(f, script, **opt_kw):
    """the one-file driver, as WhisperModel.generate_segments runs the state"""
    state = SeekState(FRAMES[f], _tok(), _options(**opt_kw), DIMS.n_text_ctx)
    out = []
    while True:
        req = state.next_request()
        if req is None:
            return out
        assert state.next_request() is req                       # idempotent until consumed
        decode = fallback_ladder(lambda t, seed: script.result(f, req.seek, req.prompt, t, seed), state.tokenizer.decode,
                                 state.options, seed=req.window)
        out.extend(state.consume(decode))


@pytest.mark.parametrize("cond", [True, False])
def test_one_file_driver_equals_oracle_loop(cond):
    for f in range(len(FRAMES)):
        a, b = Script(), Script()
        got = _drive_one(f, a, condition_on_previous_text=cond)
        ref = _oracle(f, b, condition_on_previous_text=cond)
        assert _key(got) == _key(ref), f
        assert a.calls == b.calls, f                              # same windows, prompts' lengths, temperatures, seeds
        assert [s["id"] for s in got] == list(range(1, len(got) + 1))
    # the script does what the module docstring says
    s = Script()
    _drive_one(SILENT[0], s)
    first = s.windows[SILENT[0]][0]
    assert not [c for c in s.calls if c[0] == SILENT[0] and c[1] == first and c[2] > 0]      # silence: no fallback
    s = Script()
    got = _drive_one(FALLBACK[0], s)
    assert [c[2] for c in s.calls if c[1] == s.windows[FALLBACK[0]][0]] == [0.0, 0.2] and got[0]["temperature"] == 0.2


@pytest.mark.parametrize("max_files", [1, 2, 5])
def test_lockstep_scheduler_equals_oracle_per_file(max_files):
    n = len(FRAMES)
    script = Script()
    results = [[] for _ in range(n)]
    rounds = []

    def open_file(f):
        return SeekState(FRAMES[f], _tok(), _options(), DIMS.n_text_ctx)

    def decode_round(batch):
        rounds.append([f for f, _, _ in batch])
        assert len(batch) <= max_files and len({f for f, _, _ in batch}) == len(batch)

        def first_pass(idx):           # one shared pass at temperatures[0]: entry i decodes against slot i
            return [script.result(batch[i][0], batch[i][2].seek, batch[i][2].prompt, TEMPS[0], batch[i][2].window)
                    for i in idx]

        def fallback_generate(i, t, seed):
            f, _, req = batch[i]
            return script.result(f, req.seek, req.prompt, t, seed)

        decode_round_with(batch, first_pass, fallback_generate, None, lambda f, out: results[f].extend(out))

    n_rounds = run_lockstep(n, max_files, open_file, decode_round)
    assert n_rounds == len(rounds)
    for f in range(n):
        ref = _oracle(f, Script())
        assert _key(results[f]) == _key(ref), (max_files, f)
        assert [s["id"] for s in results[f]] == list(range(1, len(ref) + 1))
    # the schedule: files enter in input order, a pending file takes over when one ends, never more than max_files
    assert rounds[0] == list(range(min(max_files, n)))
    assert sorted({f for r in rounds for f in r}) == list(range(n))
    if max_files >= n:
        assert len(rounds) == max(len(w) for w in script.windows.values())
    if max_files == 1:
        assert all(len(r) == 1 for r in rounds)
    # every fallback pass ran for one window alone with the seed window + i
    fb = [c for c in script.calls if c[2] > 0]
    assert fb and all(c[3] >= 1 for c in fb)


def test_per_file_prompts_do_not_mix():
    """initial prompts differ per file: a state that handed file 1's previous text to file 0 would change the hash."""
    script = Script()
    opts = [_options(initial_prompt=[301, 302, 303]), _options(initial_prompt=None), _options(prefix="hello")]
    results = [[] for _ in opts]

    def decode_round(batch):
        decode_round_with(batch,
                          lambda idx: [script.result(batch[i][0], batch[i][2].seek, batch[i][2].prompt, 0.0, batch[i][2].window)
                                       for i in idx],
                          lambda i, t, seed: script.result(batch[i][0], batch[i][2].seek, batch[i][2].prompt, t, seed),
                          None, lambda f, out: results[f].extend(out))

    run_lockstep(3, 3, lambda f: SeekState(FRAMES[f], _tok(), opts[f], DIMS.n_text_ctx), decode_round)
    for f, o in enumerate(opts):
        solo = Script()
        state = SeekState(FRAMES[f], _tok(), o, DIMS.n_text_ctx)
        ref = []
        while (req := state.next_request()) is not None:
            ref.extend(state.consume(fallback_ladder(lambda t, seed: solo.result(f, req.seek, req.prompt, t, seed),
                                                     state.tokenizer.decode, o, seed=req.window)))
        assert _key(results[f]) == _key(ref)
    first = {c[0]: c[4] for c in reversed(script.calls)}           # prompt length of each file's first window
    assert first[0] == 1 + 3 + len(_tok().sot_sequence) and first[1] == len(_tok().sot_sequence)
    assert first[2] > len(_tok().sot_sequence)                     # prefix on the first window only


def test_run_lockstep_rejects_unconsumed_and_bad_max_files():
    with pytest.raises(ValueError):
        run_lockstep(1, 0, lambda f: None, lambda b: None)
    with pytest.raises(RuntimeError, match="unconsumed"):
        run_lockstep(1, 1, lambda f: SeekState(FRAMES[1], _tok(), _options(), DIMS.n_text_ctx), lambda b: None)


def test_generate_args_struct_matches_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "whisper_mi355.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(wm_generate_args),\n'
                   '  offsetof(wm_generate_args, h_prompt_lens), offsetof(wm_generate_args, h_sot_indices),\n'
                   '  offsetof(wm_generate_args, h_max_lengths), offsetof(wm_generate_args, no_repeat_ngram_size));\n'
                   '  return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    size, o_len, o_sot, o_ml, o_ng = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True,
                                                             timeout=60).stdout.split())
    G = _capi.GenerateArgsC
    assert ctypes.sizeof(G) == size
    assert (G.h_prompt_lens.offset, G.h_sot_indices.offset, G.h_max_lengths.offset) == (o_len, o_sot, o_ml)
    assert G.no_repeat_ngram_size.offset == o_ng
    assert [n for n, _ in G._fields_][-3:] == ["h_prompt_lens", "h_sot_indices", "h_max_lengths"]
    assert _capi.ABI_VERSION == 4
    z = G()                                                        # a zero-filled tail: the three pointers are NULL
    assert not z.h_prompt_lens and not z.h_sot_indices and not z.h_max_lengths
