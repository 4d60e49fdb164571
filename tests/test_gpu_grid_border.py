"""The clamped border of the sorted-key grid (csrc/grid3.h) on the GPU: nn3 (clamp 2^20 - 16, 8 shells) and the FPFH search (clamp
2^20 - 2, 27 cells) with points and queries on both sides of the clamp, beyond it in all three axes, NaN coordinates and products
x / cell beyond 2^63, against the brute-force oracles, which know nothing about cells: indices, distances and counts EQUAL.
tests/test_grid_border_cases.py checks on the CPU that the inputs reach the clamp and hold no unintended equal distances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import fpfh_oracle as fo  # noqa: E402
from tests import grid_border_cases as gb  # noqa: E402
from tests import nn3_oracle  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _nn3(grid, Q):
    from vfmreg import ops
    idx, dist, fb = ops.nn3_query(grid, dev(Q), want_fallbacks=True)
    return idx.cpu().numpy(), dist.cpu().numpy(), int(fb.item())


@pytest.mark.parametrize("cell", [1.0, 0.37, 1e-3, 1e-7])
def test_nn3_across_the_clamp(cell):
    from vfmreg import ops
    P, _ = gb.nn3_cloud(cell)
    grid = ops.nn3_build(dev(P), cell)
    keys = grid.keys.cpu().numpy()
    c = gb.cells(P, cell, gb.NN3_L)[grid.order.cpu().numpy().astype(np.int64)] + (1 << 20)
    np.testing.assert_array_equal(keys, (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2])     # the clamp itself
    for name, Q in gb.nn3_queries(P, cell).items():
        idx, dist, fb = _nn3(grid, Q)
        want_i, want_d = nn3_oracle.nearest(P, Q)
        np.testing.assert_array_equal(idx, want_i, err_msg=name)
        np.testing.assert_array_equal(dist, want_d, err_msg=name)                        # bit for bit
        if name == "rows":
            assert fb == 0               # d2 = 0 in the query's own (border) cell ends the search in the 27 cells
        if name == "near":
            assert fb == 0               # < half a cell from a point of the cloud
        if name == "far":
            assert fb == len(Q)          # nothing within 8 cells: every point is read


def test_nn3_nan_queries_and_a_nan_point():
    from vfmreg import ops
    cell = 0.37
    P, _ = gb.nn3_cloud(cell, seed=3)
    Q = gb.nn3_queries(P, cell, seed=4)["border"]
    want_i, want_d = nn3_oracle.nearest(P, Q)
    grid = ops.nn3_build(dev(P), cell)
    Qn = Q.copy()
    rows = np.arange(5, len(Q), 11)
    Qn[rows, rows % 3] = np.nan
    idx, dist, fb = _nn3(grid, Qn)
    assert (idx[rows] == -1).all() and np.isnan(dist[rows]).all()       # nn3_query_kernel: "not found: every d2 is a NaN"
    keep = np.setdiff1d(np.arange(len(Q)), rows)
    np.testing.assert_array_equal(idx[keep], want_i[keep])              # the others of the launch: untouched
    np.testing.assert_array_equal(dist[keep], want_d[keep])
    assert fb >= len(rows)
    # a NaN point of the cloud sits in the cell -L of its axis and is never an answer
    Pn = P.copy()
    bad = np.array([7, 500, 1999])
    Pn[bad, [0, 1, 2]] = np.nan
    grid = ops.nn3_build(dev(Pn), cell)
    Q = np.concatenate([Q, P[bad], -gb.NN3_L * cell + np.random.default_rng(5).uniform(-3, 3, (200, 3)) * cell])
    clean = np.delete(Pn, bad, axis=0)
    back = np.delete(np.arange(len(Pn)), bad)
    want_i, want_d = nn3_oracle.nearest(clean, Q)
    idx, dist, _ = _nn3(grid, Q)
    np.testing.assert_array_equal(idx, back[want_i])
    np.testing.assert_array_equal(dist, want_d)


def test_kdtree_on_utm_like_coordinates():
    from vfmreg import synth
    from vfmreg.neighbors import KDTree
    P = synth.make_structured_scene(2000, 3000, seed=8)["map"][:3000] + np.array([3.0e5, 5.0e6, 100.0])
    rng = np.random.default_rng(9)
    Q = np.concatenate([P[:400], P[400:800] + rng.uniform(-5e-4, 5e-4, (400, 3)), P[:100] + rng.uniform(-40, 40, (100, 3))])
    tree = KDTree(P)
    assert np.abs(gb.cells(P, tree.grid.cell, gb.NN3_L)).max() < gb.NN3_L        # choose_cell's floor: no cell is clamped
    dist, ind = tree.query(Q)
    want_i, want_d = nn3_oracle.nearest(P, Q)
    np.testing.assert_array_equal(ind[:, 0], want_i)
    np.testing.assert_array_equal(dist[:, 0], want_d)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("r,max_nn", [(0.5, 30), (0.2, 100), (0.5, 100), (0.2, 30)])
def test_fpfh_search_across_the_clamp(r, max_nn, sign):
    """Found with this test: a query whose cell is clamped to +(2^20 - 2) in x and y probes the column (2^20 - 1, 2^20 - 1), whose run
    ends at key(2^20 - 1, 2^20 - 1, cz + 1) + 1; with cz clamped too that key is 2^63 - 1 and the + 1 wrapped to -2^63, so the run's
    end was searched as position 0, its length came out as -n and the query lost candidates of its other runs."""
    from vfmreg import ops
    pts = gb.fpfh_cloud(r, sign)
    out = ops.fpfh_search(dev(pts), r, max_nn)
    torch.cuda.synchronize()
    ref_i, ref_d, ref_c = fo.hybrid_search_brute(pts, r, max_nn)
    np.testing.assert_array_equal(out["count"].cpu().numpy(), ref_c)
    np.testing.assert_array_equal(out["idx"].cpu().numpy(), ref_i)
    np.testing.assert_array_equal(out["d2"].cpu().numpy(), ref_d)
