"""The exact 3-D k-nearest-neighbour search on the GPU (csrc/nn3.hip ``nn3_knn_kernel``, ``ops.nn3_knn``, ``KDTree.query_knn``) and the
stand-ins on it (``vfmreg.utils.FaissKNeighbors``, ``grow_deletion_set``) against the brute-force oracle of tests/knn3_oracle.py:
indices, squared distances, counts and padding EQUAL bit for bit, no case left out -- for queries on, next to and far from the cloud,
exact ties, every k from 1 to 64 that takes another path, cell sizes from "every query reads all points" to "one cell", caps, NaNs,
the clamped border of the grid, and with every output between guard bytes."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import grid_border_cases as gb  # noqa: E402
from tests import knn3_oracle  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402

INF = math.inf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _grid(P, cell=None):
    from vfmreg import neighbors, ops
    return neighbors.choose_cell(dev(P)) if cell is None else ops.nn3_build(dev(P), cell)


def _knn(grid, Q, k, max_d2=INF):
    """(idx, d2, count, queries that read every point) from the product"""
    from vfmreg import ops
    idx, d2, count, fb = ops.nn3_knn(grid, dev(Q), k, max_d2, want_fallbacks=True)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float64 and count.dtype == torch.int32
    assert tuple(idx.shape) == tuple(d2.shape) == (len(Q), k) and tuple(count.shape) == (len(Q),)
    return idx.cpu().numpy(), d2.cpu().numpy(), count.cpu().numpy(), int(fb.item())


def _check(P, Q, k, cell=None, max_d2=INF, grid=None, want=None, msg=""):
    grid = _grid(P, cell) if grid is None else grid
    idx, d2, count, fb = _knn(grid, Q, k, max_d2)
    want_i, want_d, want_c = knn3_oracle.knn(P, Q, k, max_d2) if want is None else want
    np.testing.assert_array_equal(count, want_c, err_msg=msg)
    np.testing.assert_array_equal(idx, want_i, err_msg=msg)
    np.testing.assert_array_equal(d2, want_d, err_msg=msg)          # bit for bit, the (-1, +inf) padding included
    return fb, grid


@pytest.fixture(scope="module")
def scene():
    """~3000 points on planes and cylinders, the host's grid of them, and ~600 queries: rows, rows moved by 3 cm, points 2-6 cells off"""
    from vfmreg import synth
    P = synth.make_structured_scene(500, 3000, seed=11)["map"]
    grid = _grid(P)
    rng = np.random.default_rng(12)
    rows = P[rng.choice(len(P), 200, replace=False)]
    unit = rng.normal(0, 1, (200, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    moved = P[rng.choice(len(P), 200, replace=False)] + 0.03 * unit
    off = P[rng.choice(len(P), 200, replace=False)] + np.c_[np.zeros((200, 2)), rng.uniform(2, 6, 200) * grid.cell]
    return dict(P=P, grid=grid, rows=rows, Q=np.concatenate([rows, moved, off]))


@pytest.mark.parametrize("k", [1, 2, 10, 25, 50, 63, 64])
def test_structured_cloud(scene, k):
    from vfmreg import ops
    P, grid, Q = scene["P"], scene["grid"], scene["Q"]
    _check(P, Q, k, grid=grid)
    fb, _ = _check(P, scene["rows"], k, grid=grid)
    assert fb == 0                                                   # a row of the cloud finds its k within the 8 shells
    if k == 1:
        idx, d2, count, _ = ops.nn3_knn(grid, dev(Q), 1, want_fallbacks=True)
        i1, dist1 = ops.nn3_query(grid, dev(Q))
        assert torch.equal(idx[:, 0], i1) and torch.equal(torch.sqrt(d2[:, 0]), dist1) and bool((count == 1).all())


def _lattice():
    g = np.arange(8, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    P = P[np.random.default_rng(3).permutation(len(P))]
    return P, np.concatenate([P[:150], P[150:300] + 0.5])            # ties on the shells' borders at every cell size below


def _scene500():
    from vfmreg import synth
    P = synth.make_structured_scene(100, 500, seed=11)["map"]
    rng = np.random.default_rng(14)
    return P, P[:300] + rng.normal(0, 0.03, (300, 3))                # centimetres off a row: 8 shells of 0.1 mm hold no point


def _border(name):
    """the first 512 rows of the border cloud (rows are in random order: every sub-cloud is among them) and at most 300 queries of a set"""
    P = gb.nn3_cloud(1.0)[0][:512]
    Q = gb.nn3_queries(P, 1.0)[name]
    return P, Q[np.linspace(0, len(Q) - 1, min(len(Q), 300)).astype(np.int64)]


def _one_cell():
    P, Q = _scene500()
    shift = 1.0 - P.min(axis=0)
    return P + shift, Q + shift


def _nan_queries():
    P, Q = _scene500()
    Q = Q[:20].copy()
    Q[np.arange(20), np.arange(20) % 3] = np.nan
    return P, Q


# name -> (cloud and queries, cell, queries that read every point: "all", "none" or None for whatever the two kernels agree on)
ONE_WALK_CASES = {
    "lattice, cell 0.3": (_lattice, 0.3, None),
    "lattice, cell 1": (_lattice, 1.0, "none"),
    "lattice, cell 2.5": (_lattice, 2.5, "none"),
    "scene, cell 1e-4": (_scene500, 1e-4, "all"),
    "scene in one cell": (_one_cell, 1000.0, "none"),
    "border, rows": (lambda: _border("rows"), 1.0, None),
    "border, near": (lambda: _border("near"), 1.0, None),
    "border, border": (lambda: _border("border"), 1.0, None),
    "border, far": (lambda: _border("far"), 1.0, "all"),
    "border, opposite": (lambda: _border("opposite"), 1.0, None),
    "NaN queries": (_nan_queries, 0.5, "all"),
}


@pytest.mark.parametrize("case", list(ONE_WALK_CASES))
def test_one_nearest_and_k_nearest_of_one_agree_bit_for_bit(case):
    """``ops.nn3_query`` and ``ops.nn3_knn(k = 1)`` walk the same shells: the same row, the same bits of the distance, the same number
    of queries that read every point -- and both are the oracle's k = 1"""
    from vfmreg import ops
    make, cell, fallbacks = ONE_WALK_CASES[case]
    P, Q = make()
    assert len(P) <= 512 and len(Q) <= 300
    grid = ops.nn3_build(dev(P), cell)
    if case == "scene in one cell":
        assert len(torch.unique(grid.keys)) == 1
    idx1, dist1, fb1 = ops.nn3_query(grid, dev(Q), want_fallbacks=True)
    idx, d2, count, fb = ops.nn3_knn(grid, dev(Q), 1, want_fallbacks=True)
    assert int(fb1.item()) == int(fb.item())
    if fallbacks is not None:
        assert int(fb.item()) == (len(Q) if fallbacks == "all" else 0)
    want_i, want_d, want_c = knn3_oracle.knn(P, Q, 1)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(d2.cpu().numpy(), want_d)
    np.testing.assert_array_equal(count.cpu().numpy(), want_c)
    if case == "NaN queries":
        assert bool((idx1 == -1).all()) and bool(torch.isnan(dist1).all())
        assert bool((count == 0).all()) and bool((idx == -1).all()) and bool((d2 == INF).all())
    else:
        assert torch.equal(idx[:, 0], idx1) and bool((idx1 >= 0).all())
        assert torch.equal(torch.sqrt(d2[:, 0]), dist1)              # torch.equal on fp64: the same bits (no NaN here)
        assert bool((count == 1).all())


@pytest.mark.parametrize("n", [1, 5])
def test_fewer_points_than_k(n):
    rng = np.random.default_rng(20 + n)
    P = rng.normal(0, 1, (n, 3))
    Q = np.concatenate([P, rng.normal(0, 2, (40, 3))])
    for cell in (None, 0.05, 50.0):
        idx, d2, count, fb = _knn(_grid(P, cell), Q, 10)
        assert (count == n).all() and (idx[:, n:] == -1).all() and np.isinf(d2[:, n:]).all() and (idx[:, :n] >= 0).all()
        assert fb == len(Q)                                          # a list that never fills reads every point
        _check(P, Q, 10, cell)


def test_exact_ties_on_a_lattice_and_with_repeated_points():
    g = np.arange(8, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    P = P[np.random.default_rng(3).permutation(len(P))]
    Q = np.concatenate([P[:150], P[150:300] + 0.5])                  # lattice points (6 / 12 / 8 equal distances) and cell centres (8 / 24)
    for k in (7, 27):
        want = knn3_oracle.knn(P, Q, k)
        assert (np.diff(want[1], axis=1) == 0).any()
        for cell in (None, 0.3, 1.0, 2.5):
            _check(P, Q, k, cell, want=want, msg=f"k={k} cell={cell}")
    rng = np.random.default_rng(4)
    base = rng.uniform(-3, 3, (700, 3))
    P3 = np.concatenate([base, base, base])[rng.permutation(2100)]   # every point three times: order is by index
    Q3 = np.concatenate([base[:200], rng.uniform(-3, 3, (100, 3))])
    for k in (3, 7, 64):
        want = knn3_oracle.knn(P3, Q3, k)
        _check(P3, Q3, k, want=want)
        _check(P3, Q3, k, 0.9, want=want)


def test_cell_sizes_change_no_answer(scene):
    P, Q = scene["P"], scene["Q"][::3]
    for k in (10, 50):
        want = knn3_oracle.knn(P, Q, k)
        _check(P, Q, k, grid=scene["grid"], want=want)
        fb, _ = _check(P, Q, k, 1e-4, want=want)
        assert fb == len(Q)                                          # 8 shells of 0.1 mm hold no k points: every query reads all
        fb, _ = _check(P, Q, k, 1000.0, want=want)
        assert fb == 0                                               # the eight cells that meet at the origin
    # cells begin at multiples of the cell size, so a cloud around the origin lies in eight of them whatever the size: move it (and the
    # queries) into x, y, z > 0, where one cell of 1000 m holds it all
    shift = 1.0 - P.min(axis=0)
    Ps, Qs = P + shift, Q + shift
    assert Ps.min() > 0 and Ps.max() < 1000.0
    for k in (10, 50):
        fb, grid = _check(Ps, Qs, k, 1000.0)
        assert fb == 0 and len(torch.unique(grid.keys)) == 1         # all points share one cell


def test_the_cap(scene):
    P, grid, Q = scene["P"], scene["grid"], scene["Q"]
    free_i, free_d, _ = knn3_oracle.knn(P, Q, 10)
    for k in (10, 50):
        want = knn3_oracle.knn(P, Q, k, 0.5)
        assert (want[2] < k).any() and (want[2] > 0).any()
        fb, _ = _check(P, Q, k, max_d2=0.5, grid=grid, want=want)
        assert fb == 0                                               # reach^2 > 0.5 ends the walk
    # below the nearest neighbour of every query that is no row: nothing for them, the row itself for rows
    off = Q[400:]
    low = 0.5 * free_d[400:, 0].min()
    assert low > 0
    idx, d2, count, _ = _knn(grid, off, 10, low)
    assert (count == 0).all() and (idx == -1).all() and np.isinf(d2).all()
    _check(P, Q, 10, max_d2=low, grid=grid)
    # equal to a pair's d2 exactly: that neighbour is in (the cap is inclusive), the next one is out
    q = 450
    cap = float(free_d[q, 3])
    assert free_d[q, 2] < cap < free_d[q, 4]
    idx, d2, count, _ = _knn(grid, Q, 10, cap)
    assert count[q] == 4 and d2[q, 3] == cap and idx[q, 3] == free_i[q, 3] and idx[q, 4] == -1
    _check(P, Q, 10, max_d2=cap, grid=grid)
    _check(P, Q, 10, max_d2=0.0, grid=grid)                          # only the rows themselves
    # far away with a cap: the walk stops when the cube covers the cap, long before 8 shells
    far = np.array([[400.0, -250.0, 90.0], [1e6, 1e6, 1e6]])
    idx, d2, count, fb = _knn(grid, far, 10, 0.5)
    assert fb == 0 and (count == 0).all() and (idx == -1).all()
    assert _knn(grid, far, 10)[3] == 2                               # without one: every point


def test_nan_queries_nan_points_and_queries_1e12_away(scene):
    P, Q = scene["P"].copy(), scene["Q"][:300].copy()
    bad_q = np.arange(5, len(Q), 11)
    Q[bad_q, bad_q % 3] = np.nan
    bad_p = np.array([7, 500, 1999])
    P[bad_p, [0, 1, 2]] = np.nan
    Q = np.concatenate([Q, scene["P"][bad_p]])                       # where the NaN points were
    grid = _grid(P, scene["grid"].cell)
    for k in (8, 64):
        idx, d2, count, fb = _knn(grid, Q, k)
        assert (count[bad_q] == 0).all() and (idx[bad_q] == -1).all() and np.isinf(d2[bad_q]).all()
        assert not np.isin(idx, bad_p).any() and fb >= len(bad_q)
        _check(P, Q, k, grid=grid)
    rng = np.random.default_rng(13)
    far = np.concatenate([rng.uniform(-1, 1, (20, 3)) + np.array([1e12, 0.0, 0.0]), rng.uniform(-1, 1, (20, 3)) + np.array([-1e12, 1e12, -1e12])])
    fb, _ = _check(P, far, 10, grid=grid)
    assert fb == len(far)


@pytest.mark.parametrize("cell", [1.0, 1e-3])
def test_the_clamped_border(cell):
    P, _ = gb.nn3_cloud(cell)
    grid = _grid(P, cell)
    for name, Q in gb.nn3_queries(P, cell).items():
        fb, _ = _check(P, Q, 8, grid=grid, msg=name)
        if name == "far":
            assert fb == len(Q)


@pytest.mark.parametrize("n,nq,k,cell", [(1, 1, 64, 1.0), (63, 65, 10, 0.5), (257, 255, 64, 3.0), (5000, 1000, 50, 0.4), (300, 1, 64, 0.7)])
def test_knn_stays_inside_the_callers_buffers(n, nq, k, cell):
    """include/vfmreg.h: idx_out and d2_out are [nq k], count_out [nq], between guard bytes; the structure and the queries between
    poisoned guards (NaN coordinates, index 0: a read past an end would change an answer); the same result whatever the outputs held."""
    from vfmreg import _lib, ops
    lib = _lib.load()
    rng = np.random.default_rng(200 + n)
    P = rng.normal(0, 2, (n, 3))
    Q = np.concatenate([P[rng.integers(0, n, nq // 2)], rng.normal(0, 2, (nq - nq // 2 - nq // 8, 3)), rng.normal(300, 5, (nq // 8, 3))])
    assert len(Q) == nq
    want_i, want_d, want_c = knn3_oracle.knn(P, Q, k)
    built = ops.nn3_build(dev(P), cell)
    keys = GuardedBuffer(n, torch.int64, seed=3).set(built.keys)
    order = GuardedBuffer(n, torch.int32, seed=4).set(built.order)
    srt = GuardedBuffer((n, 3), torch.float64, seed=5).set(built.sorted)
    qs = GuardedBuffer((nq, 3), torch.float64, seed=2).set(Q)
    idx = GuardedBuffer((nq, k), torch.int64, seed=6)
    d2 = GuardedBuffer((nq, k), torch.float64, seed=7)
    cnt = GuardedBuffer(nq, torch.int32, seed=8)
    fb = GuardedBuffer(1, torch.int32, seed=9)
    fbs = []
    for fill, poison, cap in ((0x00, False, INF), (0xFF, False, INF), (0xFF, True, INF), (0x00, True, 1e30)):
        for b in (idx, d2, cnt, fb):
            b.fill_bytes(fill)
        if poison:
            keys.poison_guards("zero")
            order.poison_guards("zero")
            srt.poison_guards("nan")
            qs.poison_guards("nan")
        _lib.check(lib.vfm_nn3_knn(keys.ptr(), order.ptr(), srt.ptr(), n, cell, qs.ptr(), nq, k, cap, idx.ptr(), d2.ptr(), cnt.ptr(), fb.ptr(),
                                   ops._stream()), "nn3_knn")
        torch.cuda.synchronize()
        for name, b in dict(keys=keys, order=order, srt=srt, qs=qs, idx=idx, d2=d2, cnt=cnt, fb=fb).items():
            assert b.intact(), f"{name}: {b.intact()!r}"
        np.testing.assert_array_equal(idx.numpy(), want_i)
        np.testing.assert_array_equal(d2.numpy(), want_d)
        np.testing.assert_array_equal(cnt.numpy(), want_c)
        np.testing.assert_array_equal(qs.numpy(), Q)
        fbs.append(int(fb.numpy()[0]))
        for b in (keys, order, srt, qs):
            b.restore_guards()
    assert len(set(fbs)) == 1 and (fbs[0] >= nq // 8 or 9 * cell > 250 or n < k)
    # nq == 0 writes nothing but the count, which is optional
    for b in (idx, d2, cnt, fb):
        b.fill_bytes(0xFF)
    before = idx.body_bytes(), d2.body_bytes(), cnt.body_bytes()
    _lib.check(lib.vfm_nn3_knn(keys.ptr(), order.ptr(), srt.ptr(), n, cell, qs.ptr(), 0, k, INF, idx.ptr(), d2.ptr(), cnt.ptr(), fb.ptr(),
                               ops._stream()), "nn3_knn")
    torch.cuda.synchronize()
    assert fb.numpy()[0] == 0
    for b, was in zip((idx, d2, cnt), before):
        np.testing.assert_array_equal(b.body_bytes(), was)
    _lib.check(lib.vfm_nn3_knn(keys.ptr(), order.ptr(), srt.ptr(), n, cell, qs.ptr(), nq, k, INF, idx.ptr(), d2.ptr(), cnt.ptr(), None,
                               ops._stream()), "nn3_knn")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(idx.numpy(), want_i)
    assert idx.intact() and d2.intact() and cnt.intact()


def test_abi_refusals_launch_nothing():
    from vfmreg import _lib, ops
    lib = _lib.load()
    P = np.random.default_rng(30).normal(0, 1, (100, 3))
    g = ops.nn3_build(dev(P), 0.5)
    q = dev(P[:4])
    idx = torch.full((4, 64), 77, dtype=torch.int64, device="cuda")
    d2 = torch.full((4, 64), 77.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    fb = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    for k, cap, word in ((0, INF, b"k must be in 1..64"), (65, INF, b"k must be in 1..64"), (10, -0.5, b"max_d2"), (10, math.nan, b"max_d2")):
        rc = lib.vfm_nn3_knn(g.keys.data_ptr(), g.order.data_ptr(), g.sorted.data_ptr(), g.n, g.cell, q.data_ptr(), 4, k, cap, idx.data_ptr(),
                             d2.data_ptr(), cnt.data_ptr(), fb.data_ptr(), ops._stream())
        assert rc == -1 and word in lib.vfm_last_error()
    torch.cuda.synchronize()
    assert bool((idx == 77).all()) and bool((d2 == 77.0).all()) and bool((cnt == 77).all()) and int(fb.item()) == 77
    with pytest.raises(RuntimeError, match="k must be in"):
        ops.nn3_knn(g, q, 65)


def test_kdtree_query_knn(scene):
    from vfmreg.neighbors import KDTree
    P = scene["P"]
    Q = scene["Q"][::6]
    tree = KDTree(P, metric="euclidean")
    for k in (2, 10, 64):
        want_i, want_d, _ = knn3_oracle.knn(P, Q, k)
        dist, ind = tree.query_knn(Q, k)
        assert isinstance(dist, np.ndarray) and dist.shape == ind.shape == (len(Q), k) and ind.dtype == np.int64 and dist.dtype == np.float64
        np.testing.assert_array_equal(ind, want_i)
        np.testing.assert_array_equal(dist, np.sqrt(want_d))        # roots, as sklearn returns them
    np.testing.assert_array_equal(tree.query_knn(Q, 64, return_distance=False), ind)
    tdist, tind = tree.query_knn(dev(Q), 64)                        # device tensors in, device tensors out
    assert tdist.is_cuda and tind.is_cuda
    np.testing.assert_array_equal(tind.cpu().numpy(), ind)
    np.testing.assert_array_equal(tdist.cpu().numpy(), dist)
    dist0, ind0 = tree.query_knn(np.zeros((0, 3)), 5)
    assert dist0.shape == ind0.shape == (0, 5)
    small = KDTree(P[:5])
    assert small.query_knn(Q, 5)[1].shape == (len(Q), 5)
    with pytest.raises(ValueError, match="number of training points"):
        small.query_knn(Q, 6)
    with pytest.raises(NotImplementedError):
        tree.query(Q, k=2)


@pytest.fixture(scope="module")
def filter_scene():
    """2000 map points (~10 per m^2) and 400 deletion candidates: three dense patches, scattered single points of the surface, and
    points put alone, in pairs and in threes far above it -- candidates with 0, 1 and 2 neighbours"""
    from vfmreg import synth
    rng = np.random.default_rng(40)
    surf = synth.make_structured_scene(500, 1970, seed=41, extent=6.0, boxes=4, cylinders=3)["map"]
    lone = np.array([[0, 0, 30.0], [3, 3, 40.0], [-4, 2, 50.0], [5, -5, 60.0]])
    pairs = np.array([[0, 0, 80.0], [0.3, 0, 80.0], [4, 4, 90.0], [4, 4.2, 90.1]])
    threes = np.array([[-3, -3, 100.0], [-3.2, -3, 100.0], [-3, -3.3, 100.0]])
    fours = np.array([[2, -2, 120.0], [2.2, -2, 120.0], [2, -2.2, 120.0], [2.1, -2.1, 120.2]])
    near = surf[:15] + np.array([0, 0, 0.6])                         # kept points within reach of candidates
    xyz = np.concatenate([surf, lone, pairs, threes, fours, near]).astype(np.float32)
    assert len(xyz) == 2000
    centres = surf[rng.choice(1970, 3, replace=False)]
    d = np.min(np.linalg.norm(surf[:, None, :] - centres[None], axis=2), axis=1)
    patch = np.argsort(d)[:345]
    scattered = np.setdiff1d(rng.choice(1970, 60, replace=False), patch)[:40]
    cand = np.concatenate([patch, scattered, np.arange(1970, 1985)])
    assert len(cand) == 400 and len(np.unique(cand)) == 400
    return xyz, rng.permutation(cand)


def test_faiss_stand_in_and_grow_deletion_set(filter_scene):
    from vfmreg import utils
    xyz, cand = filter_scene
    rng = np.random.default_rng(42)
    others = np.setdiff1d(np.arange(len(xyz)), cand)
    for pts_rows, q_rows in ((cand, cand), (others, cand), (others, rng.choice(len(xyz), 300, replace=False))):
        y = rng.permutation(10000)[:len(pts_rows)]
        ours, ref = utils.FaissKNeighbors(), knn3_oracle.FaissRestated()
        ours.fit(xyz[pts_rows], y)
        ref.fit(xyz[pts_rows], y)
        for k, r in ((10, .5), (50, .5), (64, 2.0), (3, 1e-3)):
            got = ours.query(xyz[q_rows], k, r)
            want = ref.query(xyz[q_rows], k, r)
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got, want)
            got = ours.n_neighbors_in_radius(xyz[q_rows], k, r)
            want = ref.n_neighbors_in_radius(xyz[q_rows], k, r)
            assert got.shape == want.shape == (len(q_rows),)
            np.testing.assert_array_equal(got, want)
    counts = knn3_oracle.FaissRestated()
    counts.fit(xyz[cand], cand)
    nn = counts.n_neighbors_in_radius(xyz[cand], 10, .5)
    assert {0, 1, 2, 3} <= set(nn.tolist()) and (nn == 9).any()      # isolated candidates, and rows whose own zero takes a slot of the 10
    want_del, want_keep = knn3_oracle.grow_restated(xyz, cand)
    got_del, got_keep = utils.grow_deletion_set(xyz, cand)
    np.testing.assert_array_equal(got_del, want_del)
    np.testing.assert_array_equal(got_keep, want_keep)
    assert (nn < 3).sum() > 0 and len(want_del) > (nn >= 3).sum() and len(want_del) + len(want_keep) == len(xyz)
    # fewer points than k: faiss pads with -1, and the cuts drop the padding
    few, ref = utils.FaissKNeighbors(), knn3_oracle.FaissRestated()
    few.fit(xyz[:5], np.arange(5))
    ref.fit(xyz[:5], np.arange(5))
    np.testing.assert_array_equal(few.query(xyz[:50], 10, 100.0), ref.query(xyz[:50], 10, 100.0))
    np.testing.assert_array_equal(few.n_neighbors_in_radius(xyz[:50], 10, 100.0), ref.n_neighbors_in_radius(xyz[:50], 10, 100.0))
