"""The open-end DTW kernel (wm_dtw_open, csrc/align.hip dtw_kernel_body<true>) against its definition in numpy
(tests/forced_align_ref.py): the same input and the same f32 order, so path, length and rows reached are equal
exactly; plus ties, crafted end rows, the closed path when every row is reached, and a non-finite matrix."""
import numpy as np
import pytest
import torch

from tests.forced_align_ref import dtw_open
from vlog_amd.dims import model_dims

pytestmark = pytest.mark.gpu

# N > M, M > N, one cell, one row, one column, N above one 256-thread stride, and a full forced-alignment window
SHAPES = [(1, 1), (1, 7), (5, 1), (40, 3), (3, 40), (37, 64), (257, 300), (225, 750)]


@pytest.fixture(scope="module")
def eng():
    from vlog_amd.engine import GpuEngine
    return GpuEngine.frontend(model_dims("tiny"), 0)      # the DTW entry points need no weights


def _check(eng, x):
    gi, gj, rows = eng.dtw(torch.from_numpy(x), open_end=True)
    ri, rj, R, _ = dtw_open(x)
    assert rows == R, (rows, R)
    assert len(gi) == len(ri) and np.array_equal(gi, ri) and np.array_equal(gj, rj)
    assert gi[-1] == rows - 1 and gj[-1] == x.shape[1] - 1 and gi[0] == 0 and gj[0] == 0
    if rows == x.shape[0]:                                 # every row reached: the closed DTW's path
        ci, cj = eng.dtw(torch.from_numpy(x))
        assert np.array_equal(gi, ci) and np.array_equal(gj, cj)
    return rows


@pytest.mark.parametrize("shape", SHAPES)
def test_dtw_open_matches_definition(eng, shape):
    x = np.random.default_rng(1000 + shape[0] * 7 + shape[1]).standard_normal(shape).astype(np.float32)
    _check(eng, x)


def test_dtw_open_ties_take_the_smallest_row(eng):
    assert _check(eng, np.zeros((6, 9), dtype=np.float32)) == 1


def _staircase(N, M, k):
    """Rows 0..k-1: -1 on a staircase that covers every column once (0 elsewhere); rows k..N-1: +1.  Ending at row k
    collects -M (integers: exact in f32); any earlier row misses a step, any later row pays +1."""
    x = np.zeros((N, M), dtype=np.float32)
    x[k:] = 1.0
    for i in range(k):
        x[i, i * M // k: (i + 1) * M // k] = -1.0
    return x


@pytest.mark.parametrize("nmk", [(12, 40, 5), (12, 40, 12)])
def test_dtw_open_crafted_end_row(eng, nmk):
    N, M, k = nmk
    assert _check(eng, _staircase(N, M, k)) == k


def test_dtw_open_non_finite_raises_and_the_process_goes_on(eng):
    x = np.random.default_rng(5).standard_normal((9, 20)).astype(np.float32)
    bad = x.copy()
    bad[:, 3] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        eng.dtw(torch.from_numpy(bad), open_end=True)
    _check(eng, x)                                          # the engine still answers


def test_dtw_default_keeps_returning_two_arrays(eng):
    x = np.random.default_rng(6).standard_normal((7, 30)).astype(np.float32)
    out = eng.dtw(torch.from_numpy(x))
    assert isinstance(out, tuple) and len(out) == 2
    assert len(eng.dtw(torch.from_numpy(x), open_end=False)) == 2
