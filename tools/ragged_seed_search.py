"""CPU search for the (audio seed, previous-text seed) pairs of tests/test_gpu_ragged_prompts.py.

For each of the test's prompt kinds it walks candidate seeds and keeps the first whose greedy decode on the CPU oracle
(oracle encoder, oracle decoder, the test's logit rules) holds at least `--margin` nats between the chosen and the
best other token at every step, so that bf16-level differences between two GPU decoder passes cannot flip a token.
Prints the lists to paste into the test, with each window's margin.  No GPU is used.

    python tools/ragged_seed_search.py [--margin 0.1] [--first-audio 700]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import mel as omel                                   # noqa: E402
from oracle.decode import GenerateOptions, generate_one          # noqa: E402
from oracle.model import OracleWhisper                           # noqa: E402
from tests.parity_util import teacher_force_batch                # noqa: E402
from tests.test_gpu_ragged_prompts import KINDS, ML, MODEL_SEED, _sup, build_prompts   # noqa: E402
from vlog_amd.audio import speech_like                           # noqa: E402
from vlog_amd.dims import model_dims                             # noqa: E402
from vlog_amd.weights import round_bf16, synthetic_state_dict    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--margin", type=float, default=0.1)
    ap.add_argument("--first-audio", type=int, default=700)
    ap.add_argument("--tries", type=int, default=12)
    a = ap.parse_args()
    dims = model_dims("tiny")
    st = dims.specials
    orc = OracleWhisper(round_bf16(synthetic_state_dict(dims, seed=MODEL_SEED, eot_after=60)), dims, np.float32)
    audio_seed, prev_seed = a.first_audio, 0
    audio, prev = [], []
    for kind in KINDS + ["nots"]:
        with_ts = kind != "nots"
        opt = GenerateOptions(beam_size=1, max_length=ML, suppress_tokens=_sup(st), with_timestamps=with_ts)
        for _ in range(a.tries):
            enc = orc.encode(omel.pad_or_trim(omel.log_mel(speech_like(30.0, audio_seed), dims.n_mels)[:, :3000])[None])
            prompt = build_prompts(dims, [kind], [prev_seed])[0]
            r = generate_one(orc, orc.cross_kv(enc), prompt, st, opt)
            ended = len(prompt) + len(r.tokens) < ML
            ms, _, _ = teacher_force_batch(orc, enc, prompt, [r.tokens], [ended], st, opt)[0]
            m = float(np.min(ms)) if len(ms) else 0.0
            print(f"{kind:8s} audio {audio_seed} prev {prev_seed}: prompt {len(prompt)}, {len(r.tokens)} tokens, "
                  f"min margin {m:.4f}", flush=True)
            if m >= a.margin and len(r.tokens) > 8:
                break
            audio_seed += 1
            prev_seed += 1
        else:
            raise SystemExit(f"no seed found for {kind}")
        audio.append(audio_seed)
        prev.append(prev_seed)
        audio_seed += 1
        prev_seed += 1
    print("AUDIO_SEEDS =", audio[:-1])
    print("PREV_SEEDS =", prev[:-1])
    print("NOTS_AUDIO_SEED =", audio[-1], " NOTS_PREV_SEED =", prev[-1])


if __name__ == "__main__":
    main()
