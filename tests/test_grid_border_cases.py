"""CPU checks of tests/grid_border_cases.py: the clouds reach the clamp of the grid on both sides, and no query has two candidates at the
same distance unless they are the same point repeated (then the lower index is the answer) -- so the brute-force oracles' answers,
which tests/test_gpu_grid_border.py demands bit for bit, are unambiguous."""
import numpy as np
import pytest

from tests import fpfh_oracle as fo
from tests import grid_border_cases as gb


@pytest.mark.parametrize("cell", [1.0, 0.37, 1e-3, 1e-7])
def test_nn3_border_inputs_reach_the_clamp_and_hold_no_ties(cell):
    P, names = gb.nn3_cloud(cell)
    assert len(P) <= 3000
    raw = np.floor(P * (1.0 / cell))
    c = gb.cells(P, cell, gb.NN3_L)
    for axis, sign in ((0, 1), (1, -1), (2, 1), (2, -1)):
        assert (sign * raw[:, axis] > gb.NN3_L).sum() >= 50 and (sign * c[:, axis] == gb.NN3_L).sum() >= 50
        inside = (sign * raw[:, axis] < gb.NN3_L) & (sign * raw[:, axis] > gb.NN3_L - 12)
        assert inside.sum() >= 50
    assert ((raw > gb.NN3_L).all(1)).sum() >= 300 and ((raw < -gb.NN3_L).all(1)).sum() >= 300
    qs = gb.nn3_queries(P, cell)
    assert (np.abs(qs["far"]).max(1) * (1.0 / cell) > 2.9e6).all()
    if cell == 1e-7:
        assert (np.abs(qs["far"]) * (1.0 / cell) > 2.0 ** 63).any()
    uniq, first = np.unique(P, axis=0, return_index=True)
    assert len(P) - len(uniq) == 90                                   # the repeated points
    for name, Q in qs.items():
        # (the queries at 1e12 are left out: a difference to 1e12 is rounded to 1.2e-4, so points of a small cloud DO tie there;
        # these ties are meant, and the oracle and the kernel both give the lower index)
        Q = Q[np.abs(Q).max(1) < 1e11]
        for s in range(0, len(Q), 512):
            q = Q[s:s + 512]
            d = fo._d2(uniq[None, :, :], q[:, None, :])
            two = np.partition(d, 1, axis=1)[:, :2]
            assert (two[:, 0] < two[:, 1]).all(), name               # distinct points: distinct distances


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("r", [0.5, 0.2])
def test_fpfh_border_inputs_reach_the_clamp_and_hold_no_ties(r, sign):
    pts = gb.fpfh_cloud(r, sign)
    assert len(pts) <= 2000
    cell = r * (1.0 + 1e-6)
    raw = np.floor(pts * (1.0 / cell)) * sign
    L = gb.FPFH_L
    c = gb.cells(pts, cell, L)
    assert ((c == sign * L).all(1)).sum() >= 100                       # queries whose 27 cells end in the last (first) key of all
    idx, d2, cnt = fo.hybrid_search_brute(pts, r, 1024)
    live = np.arange(d2.shape[1]) < cnt[:, None]
    assert (np.diff(d2, axis=1)[live[:, 1:]] > 0).all()                # strictly ascending: no equal distances in a row
    # pairs less than r apart in the cells (L - 1, L), (L, clamped L + 1) and (clamped, clamped), per axis
    q, k = np.nonzero(live)
    j = idx[q, k]
    for axis in range(3):
        a, b = raw[q, axis], raw[j, axis]
        for lo, hi in ((L - 1, L), (L, L + 1), (L + 2, L + 3)):
            assert ((a == lo) & (b == hi)).sum() >= 1, (axis, lo, hi)
