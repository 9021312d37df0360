"""Reference statement (float64 numpy) of the engine's two history rules, the repetition penalty and the no-repeat
n-gram ban, as CTranslate2's logit processors of those names define them.  tests/test_repetition_rules.py pins it
against transformers' RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor applied to the generated
slice; tests/test_gpu_repetition.py uses it as the reference for the device rules.

Both rules read `generated` only: the hypothesis' tokens after the prompt (no prompt, previous text, prefix or
hotwords).  They come before every other rule (oracle.decode.apply_rules runs on their output)."""
from typing import List, Sequence

import numpy as np


def apply_history_rules(logits: np.ndarray, generated: Sequence[int], repetition_penalty: float = 1.0,
                        no_repeat_ngram_size: int = 0) -> np.ndarray:
    """logits [V] of ONE hypothesis -> float64 copy with the two rules applied."""
    x = np.array(logits, dtype=np.float64, copy=True)
    gen = [int(t) for t in generated]
    if repetition_penalty != 1.0 and gen:
        ids = np.unique(np.asarray(gen, dtype=np.int64))
        x[ids] = np.where(x[ids] < 0, x[ids] * repetition_penalty, x[ids] / repetition_penalty)
    n, g = int(no_repeat_ngram_size), len(gen)
    if n >= 1 and g >= n:
        tail = gen[g - (n - 1):] if n > 1 else []
        for i in range(g - n + 1):
            if gen[i: i + n - 1] == tail:
                x[gen[i + n - 1]] = -np.inf
    return x


def repeated_ngrams(tokens: Sequence[int], n: int) -> List[tuple]:
    """The n-grams of `tokens` that occur more than once (empty: the no-repeat invariant holds)."""
    seen, rep = set(), []
    for i in range(len(tokens) - n + 1):
        gram = tuple(tokens[i: i + n])
        if gram in seen:
            rep.append(gram)
        seen.add(gram)
    return rep


def teacher_forced_logprobs(orc, cross, prompt: Sequence[int], tokens: Sequence[int], st, suppress_tokens,
                            ended_with_eot: bool, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                            max_initial_timestamp_index=50):
    """One oracle pass over prompt + tokens; per generated step (the final <|endoftext|> included when the
    hypothesis ended on it) the log-probs after the history rules, then oracle.decode.apply_rules, then
    log-softmax.  -> (chosen [n], best [n]) float64."""
    from oracle.decode import apply_rules, log_softmax
    tokens = [int(t) for t in tokens]
    seq = tokens + ([st.eot] if ended_with_eot else [])
    logits, _ = orc.decode(np.asarray([list(prompt) + tokens]), cross)
    P = len(prompt)
    chosen, best = [], []
    for i, t in enumerate(seq):
        x = apply_history_rules(logits[0, P - 1 + i], tokens[:i], repetition_penalty, no_repeat_ngram_size)
        lp = log_softmax(apply_rules(x, tokens[:i], st, suppress_tokens, True, max_initial_timestamp_index))
        chosen.append(float(lp[t]))
        best.append(float(np.max(lp)))
    return np.array(chosen), np.array(best)
