"""The sequence bias' reference (tests/sequence_bias_ref.py) pinned against transformers' SequenceBiasLogitsProcessor,
and the host side of the option: segments.build_sequence_bias on the synthetic tokenizer and the
VLOG_AMD_SEQUENCE_BIAS file.

Framing: the processor sees [DUMMY] + generated, DUMMY an id no entry uses.  transformers skips an entry longer than
input_ids, so on the bare generated slice it drops the case G = n_j - 1 (the whole history is the entry's prefix);
with the dummy in front every prefix comparison stays inside the generated tokens.  transformers keeps its table as
a dict keyed by the sequence, so a table with duplicates goes in as a chain of processors, one per repeat."""
import json

import numpy as np
import pytest
import torch
from transformers.generation.logits_process import SequenceBiasLogitsProcessor

from tests.sequence_bias_ref import apply_all_history_rules, apply_sequence_bias, completions
from vlog_amd.dims import model_dims
from vlog_amd.segments import build_sequence_bias, load_sequence_bias_file
from vlog_amd.tokenizer import Tokenizer

V = 300
DUMMY = V - 1
ALPHA = 5                 # histories and entries over ids 1 .. ALPHA, so that prefixes do match


def _hf(table, history, logits):
    """the chain of processors (duplicates: one more processor per repeat) on [DUMMY] + history"""
    layers = []
    for seq, b in table:
        seq = tuple(int(t) for t in seq)
        for layer in layers:
            if seq not in layer:
                layer[seq] = float(b)
                break
        else:
            layers.append({seq: float(b)})
    ids = torch.tensor([[DUMMY] + list(history)], dtype=torch.long)
    scores = torch.from_numpy(logits[None].copy())
    for layer in layers:
        scores = SequenceBiasLogitsProcessor([[list(s), b] for s, b in layer.items()])(ids, scores)
    return scores[0].numpy()


def _random_table(rng, n, max_len):
    table = []
    for _ in range(n):
        L = int(rng.integers(1, max_len + 1))
        table.append((tuple(int(t) for t in rng.integers(1, ALPHA + 1, size=L)), float(np.round(rng.normal() * 5, 3))))
    return table


def test_reference_matches_transformers_on_random_tables():
    mismatches, active = 0, 0
    for trial in range(300):
        rng = np.random.default_rng(trial)
        logits = (rng.standard_normal(V) * 3).astype(np.float32)
        G = int(rng.integers(0, 9))
        hist = [int(t) for t in rng.integers(1, ALPHA + 1, size=G)]
        table = _random_table(rng, int(rng.integers(1, 12)), 4)
        got = apply_sequence_bias(logits, hist, table)
        ref = _hf(table, hist, logits)
        mismatches += not np.allclose(got, ref, rtol=1e-6, atol=1e-5)
        active += int(np.any(got != logits))
    assert mismatches == 0
    assert active >= 200                          # the tables did act


@pytest.mark.parametrize("G", [0, 1, 2, 3])
def test_history_is_exactly_the_prefix(G):
    """G = n_j - 1: the entry whose prefix is the whole history is active (the case the dummy id keeps), one token
    more in the entry and it is not; G = 0 leaves the length-1 entries."""
    rng = np.random.default_rng(40 + G)
    logits = (rng.standard_normal(V) * 3).astype(np.float32)
    hist = [1 + (i % ALPHA) for i in range(G)]
    table = [(tuple(hist) + (7,), 4.0), ((2,) + tuple(hist) + (8,), 4.0), ((9,), -2.5)]
    got = apply_sequence_bias(logits, hist, table)
    x = logits.astype(np.float64)
    assert got[7] == x[7] + 4.0 and got[8] == x[8] and got[9] == x[9] - 2.5
    assert np.allclose(got, _hf(table, hist, logits), rtol=1e-6, atol=1e-5)
    bare = SequenceBiasLogitsProcessor([[list(s), b] for s, b in table])(
        torch.tensor([hist], dtype=torch.long).reshape(1, G), torch.from_numpy(logits[None].copy()))[0].numpy()
    if G >= 1:
        assert bare[7] == logits[7]               # without the dummy transformers drops it


def test_duplicates_and_shared_last_id_add_up_in_entry_order():
    logits = np.zeros(V, dtype=np.float32)
    hist = [3, 4]
    table = [((4, 6), 1.5), ((6,), 0.25), ((4, 6), 1.5), ((3, 4, 6), -0.125), ((5, 6), 100.0)]
    got = apply_sequence_bias(logits, hist, table)
    assert got[6] == 1.5 + 0.25 + 1.5 - 0.125
    assert np.count_nonzero(got) == 1
    assert np.allclose(got, _hf(table, hist, logits), rtol=1e-6, atol=1e-6)


def test_order_with_the_other_history_rules():
    """penalty first (the bias is added to the penalised logit), and a mask wins over a bias"""
    logits = np.full(V, 2.0, dtype=np.float32)
    hist = [1, 2, 1]
    table = [((1, 2), 30.0), ((1,), 1.0)]
    got = apply_all_history_rules(logits, hist, table, repetition_penalty=2.0, no_repeat_ngram_size=2)
    assert np.isneginf(got[2])                    # (1, 2) would repeat a bigram: -inf stays -inf under +30
    assert got[1] == 2.0 / 2.0 + 1.0              # penalised, then biased
    assert got[5] == 2.0
    assert completions([1, 2, 1, 2, 2], (1, 2)) == 2 and completions([1], (1, 2)) == 0


# ---- build_sequence_bias on the synthetic tokenizer
@pytest.fixture(scope="module")
def tok():
    return Tokenizer(model_dims("tiny"), task="transcribe", language="en")


def _word(tok, lead_space):
    """a vocabulary piece of letters only, with / without the leading space, that encodes to itself"""
    for t in range(300, 5000):
        s = tok.decode([t])
        if s.startswith(" ") == lead_space and s.strip().isalpha() and len(s.strip()) >= 4 and tok.encode(s) == [t]:
            return t, s
    raise AssertionError("no such piece")


def test_build_two_tokenisations(tok):
    V_ = model_dims("tiny").n_vocab
    t, s = _word(tok, True)                       # " word" is one token; "word" without the space is another sequence
    text = s.strip()
    table = build_sequence_bias(tok.encode, {text: -100.0}, V_)
    assert table == [((t,), -100.0), (tuple(tok.encode(text)), -100.0)]
    assert table[0][0] != table[1][0]
    assert all(tok.decode(list(seq)).strip() == text for seq, _ in table)


def test_build_deduplicates_and_keeps_tuples(tok):
    V_ = model_dims("tiny").n_vocab
    # a key that starts with a space: " " + key and key differ; a key whose two tokenisations agree gives one entry
    same = build_sequence_bias(lambda s: [11, 12], {"x": 2.0}, V_)
    assert same == [((11, 12), 2.0)]
    mixed = build_sequence_bias(tok.encode, {(5, 6, 7): 1.0, (5, 6, 7, 8): 0.5, (9,): -3}, V_)
    assert mixed == [((5, 6, 7), 1.0), ((5, 6, 7, 8), 0.5), ((9,), -3.0)]
    assert build_sequence_bias(tok.encode, {}, V_) == []


def test_build_refusals_name_the_key(tok):
    V_ = model_dims("tiny").n_vocab
    with pytest.raises(ValueError, match="'empty'"):
        build_sequence_bias(lambda s: [] if s.strip() == "empty" else [1], {"empty": 1.0}, V_)
    with pytest.raises(ValueError, match=r"\(\)"):
        build_sequence_bias(tok.encode, {(): 1.0}, V_)
    long_text = "a b c d e f g h i j k l m n o p q r s t"
    assert len(tok.encode(" " + long_text)) > 16
    with pytest.raises(ValueError, match="a b c d"):
        build_sequence_bias(tok.encode, {long_text: 1.0}, V_)
    with pytest.raises(ValueError, match="17 tokens"):
        build_sequence_bias(tok.encode, {tuple(range(17)): 1.0}, V_)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39):
        with pytest.raises(ValueError, match="'word'"):
            build_sequence_bias(tok.encode, {"word": bad}, V_)
    with pytest.raises(ValueError, match="vocabulary"):
        build_sequence_bias(tok.encode, {(1, V_): 1.0}, V_)
    with pytest.raises(ValueError, match="vocabulary"):
        build_sequence_bias(tok.encode, {(-1,): 1.0}, V_)
    with pytest.raises(ValueError, match="mapping"):
        build_sequence_bias(tok.encode, [((1,), 1.0)], V_)
    with pytest.raises(ValueError, match="1025 entries"):
        build_sequence_bias(tok.encode, {(1 + i,): 1.0 for i in range(1025)}, V_)
    assert len(build_sequence_bias(tok.encode, {(1 + i,): 1.0 for i in range(1024)}, V_)) == 1024


# ---- the environment file
def test_environment_file(tmp_path):
    good = tmp_path / "bias.json"
    good.write_text(json.dumps({"Kubernetes": 4, "thanks for watching": -100.0}))
    assert load_sequence_bias_file(str(good)) == {"Kubernetes": 4.0, "thanks for watching": -100.0}
    with pytest.raises(ValueError, match="nothere.json"):
        load_sequence_bias_file(str(tmp_path / "nothere.json"))
    for text in ("{not json", "[1, 2]", '{"a": "loud"}', '{"a": true}', '{"a": NaN}', '{"a": null}'):
        bad = tmp_path / "bad.json"
        bad.write_text(text)
        with pytest.raises(ValueError, match="bad.json"):
            load_sequence_bias_file(str(bad))
