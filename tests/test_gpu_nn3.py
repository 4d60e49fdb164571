"""The exact 3-D 1-nearest-neighbour search on the GPU (csrc/nn3.hip, ``ops.nn3_build`` / ``ops.nn3_query``,
``vfmreg.neighbors.KDTree``) against the brute-force oracle of tests/nn3_oracle.py: indices and distances EQUAL, for queries on,
next to and far from the cloud, at several cell sizes, and with every buffer between guard bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import nn3_oracle  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _search(P, Q, cell=None):
    """(idx, dist, queries that took the scan of all points) from the product; cell None = the host's own choice"""
    from vfmreg import neighbors, ops
    grid = neighbors.choose_cell(dev(P)) if cell is None else ops.nn3_build(dev(P), cell)
    idx, dist, fb = ops.nn3_query(grid, dev(Q), want_fallbacks=True)
    assert idx.dtype == torch.int64 and dist.dtype == torch.float64 and idx.shape == dist.shape == (len(Q),)
    return idx.cpu().numpy(), dist.cpu().numpy(), int(fb.item()), grid


def _check(P, Q, cell=None):
    idx, dist, fb, grid = _search(P, Q, cell)
    want_i, want_d = nn3_oracle.nearest(P, Q)
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(dist, want_d)       # bit for bit
    return fb, grid


@pytest.fixture(scope="module")
def scene():
    from vfmreg import synth
    return synth.make_structured_scene(6000, 30000, seed=0)["map"]


def test_rows_near_rows_and_far_queries(scene):
    P = scene
    rng = np.random.default_rng(1)
    rows = P[rng.choice(len(P), 5000, replace=False)]
    fb, grid = _check(P, rows)
    assert fb == 0                                                        # a row of the cloud ends in the 27 cells
    idx, dist, _, _ = _search(P, rows)
    assert (dist == 0).all() and np.array_equal(P[idx], rows)
    near = rows + rng.uniform(-5e-4, 5e-4, rows.shape)                    # moved by < 1 mm
    fb, _ = _check(P, near)
    assert fb == 0
    far = rng.uniform(-30, 30, (600, 3)) + np.array([400.0, -250.0, 90.0])   # uniform, far outside the cloud
    fb, _ = _check(P, far)
    assert fb == len(far) and 9 * grid.cell < 50.0                        # all of them took the scan of every point
    mixed = np.concatenate([rows[:100], far[:100], near[:100], rng.uniform(-35, 35, (300, 3))])
    fb, _ = _check(P, mixed)
    assert 100 <= fb < len(mixed)                                         # both paths in one launch


def test_duplicate_points_give_the_lower_index(scene):
    rng = np.random.default_rng(2)
    base = scene[:4000]
    P = np.concatenate([base, base[::3], base[::7]])[rng.permutation(4000 + 1334 + 572)]
    fb, _ = _check(P, base)
    idx, dist, _, _ = _search(P, base)
    assert (dist == 0).all()
    first = {}
    for j, row in enumerate(map(bytes, P)):
        first.setdefault(row, j)
    assert idx.tolist() == [first[bytes(r)] for r in base]


def test_lattice_ties_across_cells():
    g = np.arange(-6, 7, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    P = P[np.random.default_rng(3).permutation(len(P))]
    centres = P[:500] + 0.5                      # 8 lattice points at the same distance, in up to 8 cells
    edges = P[500:900] + np.array([0.5, 0, 0])   # 2 at the same distance
    for cell in (None, 0.3, 1.0, 2.5):
        _check(P, np.concatenate([centres, edges, P[:100]]), cell)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_small_clouds(n):
    rng = np.random.default_rng(n)
    P = rng.normal(0, 1, (n, 3))
    Q = np.concatenate([P, rng.normal(0, 3, (200, 3)), rng.normal(0, 1000, (50, 3))])
    for cell in (None, 0.01, 0.5, 100.0):
        _check(P, Q, cell)
    _check(P, Q[:1])                             # nq = 1


def test_all_points_in_one_cell_and_points_over_many_cells():
    rng = np.random.default_rng(5)
    P = 7.0 + rng.uniform(0, 1e-3, (5000, 3))    # one cell of edge 1
    assert len(np.unique(np.floor(P / 1.0), axis=0)) == 1
    Q = np.concatenate([P[:300], 7.0 + rng.uniform(-1e-3, 2e-3, (300, 3)), rng.uniform(-50, 50, (100, 3))])
    fb, _ = _check(P, Q, 1.0)
    assert fb >= 90                               # the far ones
    _check(P, Q, None)
    # a volume cloud spread over >= 1e5 cells, negative coordinates
    P = rng.uniform(-40, 40, (200000, 3))
    cell = 0.8
    assert len(np.unique(np.floor(P / cell).astype(np.int64), axis=0)) >= 100000 and (P < 0).any()
    Q = np.concatenate([P[rng.choice(len(P), 700, replace=False)], rng.uniform(-45, 45, (300, 3))])
    _check(P, Q, cell)


def test_200000_points_5000_queries_at_four_cell_sizes():
    from vfmreg import synth
    sc = synth.make_structured_scene(20000, 200000, seed=2)
    P = sc["map"]
    rng = np.random.default_rng(6)
    rows = rng.choice(len(P), 3000, replace=False)
    Q = np.concatenate([P[rows], P[rows[:1500]] + rng.uniform(-5e-4, 5e-4, (1500, 3)), rng.uniform(-35, 35, (450, 3)),
                        rng.uniform(200, 300, (50, 3))])
    assert len(Q) == 5000 and (P < 0).any()
    want_i, want_d = nn3_oracle.nearest(P, Q)
    cells = []
    for cell in (None, 0.07, 0.5, 4.0):
        idx, dist, fb, grid = _search(P, Q, cell)
        np.testing.assert_array_equal(idx, want_i)
        np.testing.assert_array_equal(dist, want_d)
        assert fb >= 50 or cell == 4.0            # the 50 far queries scan every point unless 8 shells of 4 m reach the cloud
        cells.append(grid.cell)
    assert 0.01 < cells[0] < 4.0 and len(set(cells)) == 4


def test_kdtree_stand_in(scene):
    from vfmreg.neighbors import KDTree
    P = scene[:5000]
    rng = np.random.default_rng(7)
    Q = np.concatenate([P[:50], rng.uniform(-30, 30, (50, 3))])
    want_i, want_d = nn3_oracle.nearest(P, Q)
    tree = KDTree(P, metric="euclidean")
    dist, ind = tree.query(Q, k=1, return_distance=True)
    assert isinstance(dist, np.ndarray) and dist.shape == ind.shape == (100, 1) and ind.dtype == np.int64 and dist.dtype == np.float64
    np.testing.assert_array_equal(ind[:, 0], want_i)
    np.testing.assert_array_equal(dist[:, 0], want_d)
    np.testing.assert_array_equal(tree.query(Q, return_distance=False), ind)
    tdist, tind = KDTree(dev(P)).query(dev(Q))                              # device tensors in, device tensors out
    assert tdist.is_cuda and tind.is_cuda and tuple(tdist.shape) == (100, 1)
    np.testing.assert_array_equal(tind.cpu().numpy(), ind)
    np.testing.assert_array_equal(tdist.cpu().numpy(), dist)
    dist0, ind0 = tree.query(np.zeros((0, 3)))                              # nq == 0
    assert dist0.shape == ind0.shape == (0, 1)
    P32 = P.astype(np.float32)                                              # other dtypes are searched as fp64, as sklearn does
    d32, i32 = KDTree(P32).query(Q.astype(np.float32))
    w_i, w_d = nn3_oracle.nearest(P32.astype(np.float64), Q.astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(i32[:, 0], w_i)
    np.testing.assert_array_equal(d32[:, 0], w_d)
    with pytest.raises(NotImplementedError):
        tree.query(Q, k=2)
    with pytest.raises(ValueError):
        tree.query(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        KDTree(np.zeros((0, 3)))


@pytest.mark.parametrize("n,nq,cell", [(1, 1, 1.0), (63, 65, 0.5), (256, 64, 0.2), (257, 255, 3.0), (5000, 1000, 0.4)])
def test_nn3_stays_inside_the_callers_buffers(n, nq, cell):
    """include/vfmreg.h: inputs, outputs and the workspace at exactly their sizes between guard bytes; guards and inputs untouched;
    the same result whatever the outputs held before, with a workspace a larger call used first, and with the inputs' guards
    poisoned (NaN coordinates, index 0) -- a read past an end would change an answer."""
    from vfmreg import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(100 + n)
    P = rng.normal(0, 2, (n, 3))
    Q = np.concatenate([P[rng.integers(0, n, nq // 2)], rng.normal(0, 2, (nq - nq // 2 - nq // 8, 3)), rng.normal(300, 5, (nq // 8, 3))])
    assert len(Q) == nq
    want_i, want_d = nn3_oracle.nearest(P, Q)
    ws_bytes = lib.vfm_nn3_workspace_bytes(n)
    big_n = 4 * n + 100
    big_bytes = lib.vfm_nn3_workspace_bytes(big_n)
    assert 0 < ws_bytes <= big_bytes
    pts = GuardedBuffer((n, 3), torch.float64, seed=1).set(P)
    qs = GuardedBuffer((nq, 3), torch.float64, seed=2).set(Q)
    keys = GuardedBuffer(n, torch.int64, seed=3)
    order = GuardedBuffer(n, torch.int32, seed=4)
    srt = GuardedBuffer((n, 3), torch.float64, seed=5)
    idx = GuardedBuffer(nq, torch.int64, seed=6)
    dist = GuardedBuffer(nq, torch.float64, seed=7)
    fb = GuardedBuffer(1, torch.int32, seed=8)
    ws = GuardedBuffer(big_bytes, torch.uint8, seed=9)          # the larger call's workspace; the small call is told ws_bytes of it
    ws_exact = GuardedBuffer(ws_bytes, torch.uint8, seed=10)
    bufs = dict(pts=pts, qs=qs, keys=keys, order=order, srt=srt, idx=idx, dist=dist, fb=fb, ws_exact=ws_exact)
    # a larger call first, through the big workspace: what it leaves is what the small call finds
    bigP = GuardedBuffer((big_n, 3), torch.float64, seed=11).set(rng.normal(0, 2, (big_n, 3)))
    bk, bo, bs = GuardedBuffer(big_n, torch.int64, seed=12), GuardedBuffer(big_n, torch.int32, seed=13), GuardedBuffer((big_n, 3), torch.float64, seed=14)
    _lib.check(lib.vfm_nn3_build(bigP.ptr(), big_n, cell, bk.ptr(), bo.ptr(), bs.ptr(), ws.ptr(), big_bytes, ops._stream()), "nn3_build")
    torch.cuda.synchronize()
    assert all(b.intact() for b in (bigP, bk, bo, bs, ws))
    results = []
    for fill, poison, w in ((0x00, False, ws_exact), (0xFF, False, ws_exact), (0xFF, True, ws_exact), (0x00, False, ws)):
        for b in (keys, order, srt, idx, dist, fb):
            b.fill_bytes(fill)
        if w is ws_exact:
            w.fill_bytes(fill)
        if poison:
            pts.poison_guards("nan")
            qs.poison_guards("nan")
        _lib.check(lib.vfm_nn3_build(pts.ptr(), n, cell, keys.ptr(), order.ptr(), srt.ptr(), w.ptr(), ws_bytes, ops._stream()), "nn3_build")
        if poison:                                               # the structure is the query's input
            keys.poison_guards("zero")
            order.poison_guards("zero")
            srt.poison_guards("nan")
        _lib.check(lib.vfm_nn3_query(keys.ptr(), order.ptr(), srt.ptr(), n, cell, qs.ptr(), nq, idx.ptr(), dist.ptr(), fb.ptr(),
                                     ops._stream()), "nn3_query")
        torch.cuda.synchronize()
        for name, b in list(bufs.items()) + [("ws", ws)]:
            assert b.intact(), f"{name}: {b.intact()!r}"
        np.testing.assert_array_equal(pts.numpy(), P)
        np.testing.assert_array_equal(qs.numpy(), Q)
        np.testing.assert_array_equal(idx.numpy(), want_i)
        np.testing.assert_array_equal(dist.numpy(), want_d)
        k, o, s = keys.numpy(), order.numpy(), srt.numpy()
        assert (np.diff(k) >= 0).all() and sorted(o.tolist()) == list(range(n))
        np.testing.assert_array_equal(s, P[o])
        results.append((k, o, int(fb.numpy()[0])))
        assert results[-1][2] >= nq // 8 or 9 * cell > 250      # the far queries scan every point
        for b in (pts, qs, keys, order, srt):
            b.restore_guards()
    for k, o, f in results[1:]:
        np.testing.assert_array_equal(k, results[0][0])
        np.testing.assert_array_equal(o, results[0][1])
        assert f == results[0][2]
    # nq == 0: nothing but the count is written; the count is optional
    idx.fill_bytes(0xFF)
    dist.fill_bytes(0xFF)
    fb.fill_bytes(0xFF)
    _lib.check(lib.vfm_nn3_query(keys.ptr(), order.ptr(), srt.ptr(), n, cell, qs.ptr(), 0, idx.ptr(), dist.ptr(), fb.ptr(), ops._stream()), "nn3_query")
    _lib.check(lib.vfm_nn3_query(keys.ptr(), order.ptr(), srt.ptr(), n, cell, qs.ptr(), nq, idx.ptr(), dist.ptr(), None, ops._stream()), "nn3_query")
    torch.cuda.synchronize()
    assert fb.numpy()[0] == 0 and idx.intact() and dist.intact()
    np.testing.assert_array_equal(idx.numpy(), want_i)
    # an empty cloud has no nearest point; a workspace one byte short is refused
    assert lib.vfm_nn3_query(keys.ptr(), order.ptr(), srt.ptr(), 0, cell, qs.ptr(), nq, idx.ptr(), dist.ptr(), None, ops._stream()) == -1
    assert lib.vfm_nn3_build(pts.ptr(), n, cell, keys.ptr(), order.ptr(), srt.ptr(), ws_exact.ptr(), ws_bytes - 1, ops._stream()) == -1
