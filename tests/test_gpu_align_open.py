"""wm_align_open_batch on the MI355X: the teacher-forced pass, capture, probabilities and matrix kernels of
wm_align_batch with the open-end DTW.  Three ragged items (5 / 40 / 200 text tokens against 3000 / 1500 / 700 mel
frames, in different slots): each equals the same item aligned alone; against the oracle's alignment matrix of the
SAME captured attention and the numpy definition of the open-end rule (tests/forced_align_ref.py); and an item that
reaches every row gives wm_align_batch's path.

The text seed was chosen on the CPU oracle (f32 and bf16-activation decoder alike): the best and second-best end
rows of the items differ by 0.32, 0.019 and 7.5e-4 of the cost, so at most the third can take the near-tie branch;
it ends at row 200 of 201, the other two reach every row."""
import numpy as np
import pytest
import torch

from oracle import mel as omel
from oracle.align import alignment_matrix
from tests.forced_align_ref import dtw_open, jumps
from vlog_amd.audio import speech_like
from vlog_amd.dims import model_dims
from vlog_amd.tokenizer import Tokenizer
from vlog_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

LENS, FRAMES, SLOTS = (5, 40, 200), (3000, 1500, 700), (2, 0, 1)


@pytest.fixture(scope="module")
def setup():
    from vlog_amd.engine import GpuEngine
    dims = model_dims("tiny")
    eng = GpuEngine(dims, synthetic_state_dict(dims, seed=3, eot_after=60), 0)
    x = np.concatenate([speech_like(30.0, 700 + i) for i in range(3)])
    feats = torch.from_numpy(omel.log_mel(x, dims.n_mels)).cuda()
    eng.reserve(3, 4)
    for i, (f, s) in enumerate(zip(FRAMES, SLOTS)):
        eng.cross_kv(eng.encode(feats, [3000 * i], [f]), s)
    rng = np.random.default_rng(2)
    texts = [[int(v) for v in rng.integers(200, 20000, n)] for n in LENS]
    tok = Tokenizer(dims, language="en")
    heads = dims.default_alignment_heads()
    batch = eng.align_open_batch(list(SLOTS), tok.sot_sequence, texts, list(FRAMES), heads, 7)
    return dims, eng, tok, heads, texts, batch


def test_batch_items_equal_the_items_alone(setup):
    dims, eng, tok, heads, texts, batch = setup
    for i, (probs, ti, tj, rows) in enumerate(batch):
        ap, ai, aj, ar = eng.align_open_batch([SLOTS[i]], tok.sot_sequence, [texts[i]], [FRAMES[i]], heads, 7)[0]
        assert rows == ar and np.array_equal(ti, ai) and np.array_equal(tj, aj), (i, rows, ar)
        assert np.array_equal(probs, ap)
        assert len(probs) == LENS[i] and 1 <= rows <= LENS[i] + 1
        assert ti[0] == 0 and tj[0] == 0 and ti[-1] == rows - 1 and tj[-1] == FRAMES[i] // 2 - 1
        assert len(ti) <= LENS[i] + 1 + FRAMES[i] // 2
        assert np.all(np.diff(ti) >= 0) and np.all(np.diff(tj) >= 0) and np.all(np.diff(ti) + np.diff(tj) >= 1)


def test_open_alignment_matches_oracle_matrix_and_definition(setup):
    dims, eng, tok, heads, texts, batch = setup
    st = dims.specials
    near_ties = 0
    for i, (probs, ti, tj, rows) in enumerate(batch):
        toks = tok.sot_sequence + [st.no_timestamps] + texts[i] + [st.eot]
        _, attn = eng.forward([SLOTS[i]], np.array([toks]), align_heads=heads)
        m = alignment_matrix(attn[0].cpu().numpy().transpose(1, 0, 2), FRAMES[i], len(tok.sot_sequence))
        ri, rj, R, last = dtw_open((-m).astype(np.float32))
        jg, jr = jumps(ti, tj), jumps(ri, rj)
        assert len(jg) == rows and len(jr) == R
        c = min(rows, R)
        agree = float(np.mean(jg[:c] == jr[:c]))
        gap = float(last[rows - 1] - last.min())
        print(f"item {i}: rows gpu {rows} ref {R} of {LENS[i] + 1}, jumps agree {agree:.4f}, cost gap {gap:.3e} "
              f"of |min| {abs(float(last.min())):.3f}")
        assert agree >= 0.97, (i, agree)
        if rows != R:
            near_ties += 1
            assert gap <= 1e-3 * abs(float(last.min())), (i, rows, R, gap)
    assert near_ties <= 1


def test_every_row_reached_gives_the_closed_path(setup):
    dims, eng, tok, heads, texts, batch = setup
    closed = eng.align_batch(list(SLOTS), tok.sot_sequence, texts, list(FRAMES), heads, 7)
    full = [i for i, b in enumerate(batch) if b[3] == LENS[i] + 1]
    assert full                                         # the 5- and 40-token items reach every row (module docstring)
    for i in full:
        assert np.array_equal(batch[i][1], closed[i][1]) and np.array_equal(batch[i][2], closed[i][2])
        assert np.array_equal(batch[i][0], closed[i][0])
