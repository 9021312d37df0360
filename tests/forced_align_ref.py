"""The open-end DTW's definition in numpy (test reference for wm_dtw_open / wm_align_open_batch).

oracle.align.dtw plus the end-row pick: the same recurrence with f32 adds in the same order, the same tie rules and
trace; then R = the smallest i in [1, N] that minimises cost[i][M], and the backtrace starts at (R, M) instead of
(N, M).  -> (text_indices, time_indices, R, last cost column cost[1..N][M])."""
import numpy as np


def dtw_open(x: np.ndarray):
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = -np.ones((N + 1, M + 1), dtype=np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = x[i - 1, j - 1] + c          # one f32 add, as the kernel's
            trace[i, j] = t
    last = cost[1:, M].copy()
    if not np.isfinite(last.min()) or np.isnan(last).any():
        raise ValueError("non-finite alignment cost")
    R = int(np.argmin(last)) + 1                      # argmin: the first (smallest) row of the minimum
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = R, M
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    p = np.array(path[::-1])
    return p[:, 0], p[:, 1], R, last


def jumps(ti, tj):
    """Time index at which each row of the path is entered (find_alignment's jumps)."""
    ti, tj = np.asarray(ti), np.asarray(tj)
    return tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)]
