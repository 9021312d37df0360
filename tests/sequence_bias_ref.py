"""Reference statement (float64 numpy) of the engine's sequence bias, the third rule over a hypothesis' generated
tokens (include/whisper_mi355.h wm_set_sequence_bias).  tests/test_sequence_bias_rules.py pins it against
transformers' SequenceBiasLogitsProcessor applied to the generated slice with one unused dummy id in front
(transformers skips an entry longer than input_ids, which would drop the case G = n_j - 1);
tests/test_gpu_sequence_bias.py uses it as the reference for the device rule.

The rule reads `generated` only: the hypothesis' tokens after the prompt.  Entry (s, b) is active iff
len(s) - 1 <= len(generated) and the last len(s) - 1 generated tokens equal s[:-1]; every active entry adds b to
the logit of s[-1], the entries that end in one id summed in entry order.  Order: repetition penalty, sequence bias,
no-repeat n-gram mask (a mask wins: -inf stays -inf), then oracle.decode.apply_rules."""
from typing import Sequence, Tuple

import numpy as np

from tests.repetition_ref import apply_history_rules


def apply_sequence_bias(logits: np.ndarray, generated: Sequence[int],
                        table: Sequence[Tuple[Sequence[int], float]]) -> np.ndarray:
    """logits [V] of ONE hypothesis -> float64 copy with the bias applied."""
    x = np.array(logits, dtype=np.float64, copy=True)
    gen = [int(t) for t in generated]
    add = np.zeros_like(x)
    for seq, b in table:
        seq = [int(t) for t in seq]
        k = len(seq) - 1
        if k <= len(gen) and (k == 0 or gen[len(gen) - k:] == seq[:-1]):
            add[seq[-1]] += float(b)
    return x + add


def apply_all_history_rules(logits: np.ndarray, generated: Sequence[int], table=(), repetition_penalty: float = 1.0,
                            no_repeat_ngram_size: int = 0) -> np.ndarray:
    """tests/repetition_ref.apply_history_rules (penalty, n-gram mask), then the bias.  The mask is -inf and the bias
    finite, so this is the engine's order penalty, bias, mask: the bias sees the penalised logit and -inf stays."""
    x = apply_history_rules(logits, generated, repetition_penalty, no_repeat_ngram_size)
    return apply_sequence_bias(x, generated, table)


def teacher_forced_logprobs(orc, cross, prompt: Sequence[int], tokens: Sequence[int], st, suppress_tokens,
                            ended_with_eot: bool, table=(), repetition_penalty: float = 1.0,
                            no_repeat_ngram_size: int = 0, max_initial_timestamp_index=50, with_timestamps: bool = True):
    """tests/repetition_ref.teacher_forced_logprobs with the bias between the history rules and
    oracle.decode.apply_rules: one oracle pass over prompt + tokens; per generated step (the final <|endoftext|>
    included when the hypothesis ended on it) -> (chosen [n], best [n]) float64 log-probs."""
    from oracle.decode import apply_rules, log_softmax
    tokens = [int(t) for t in tokens]
    seq = tokens + ([st.eot] if ended_with_eot else [])
    logits, _ = orc.decode(np.asarray([list(prompt) + tokens]), cross)
    P = len(prompt)
    chosen, best = [], []
    for i, t in enumerate(seq):
        x = apply_all_history_rules(logits[0, P - 1 + i], tokens[:i], table, repetition_penalty, no_repeat_ngram_size)
        lp = log_softmax(apply_rules(x, tokens[:i], st, suppress_tokens, True, max_initial_timestamp_index,
                                     with_timestamps=with_timestamps))
        chosen.append(float(lp[t]))
        best.append(float(np.max(lp)))
    return np.array(chosen), np.array(best)


def completions(tokens: Sequence[int], seq: Sequence[int]) -> int:
    """How often `seq` occurs as a contiguous run of `tokens`."""
    tokens, seq = [int(t) for t in tokens], [int(t) for t in seq]
    n = len(seq)
    return sum(tokens[i: i + n] == seq for i in range(len(tokens) - n + 1))
