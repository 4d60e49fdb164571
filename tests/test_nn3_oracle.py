"""CPU checks of the FPFH + RANSAC row: the 1-NN oracle (tests/nn3_oracle.py) anchored against sklearn's KDTree, the row filter of
registration_node.py:301-309 in its three cases (oracle and product -- the product's filter is torch ops and runs on CPU tensors too),
and the opt-in rule of ``RegistrationNode(baseline_methods=...)`` as far as it goes without a device."""
import numpy as np
import pytest

from tests import nn3_oracle


def test_oracle_equals_sklearn_kdtree_bit_for_bit():
    neighbors = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(0)
    for n, k, scale in ((20000, 5000, 30.0), (1200, 5000, 5.0), (1, 7, 1.0)):
        P = rng.uniform(-scale, scale, (n, 3))
        Q = np.concatenate([P[rng.integers(0, n, k // 2)] + rng.normal(0, 1e-4, (k // 2, 3)), rng.uniform(-2 * scale, 2 * scale, (k - k // 2, 3))])
        dist, ind = neighbors.KDTree(P, metric="euclidean").query(Q, k=1, return_distance=True)
        idx, d = nn3_oracle.nearest(P, Q)
        assert dist.shape == ind.shape == (k, 1) and ind.dtype == np.int64 and dist.dtype == np.float64
        np.testing.assert_array_equal(idx, ind[:, 0])
        np.testing.assert_array_equal(d, dist[:, 0])          # bit-equal
    # queries that ARE rows: distance exactly 0, the row itself
    idx, d = nn3_oracle.nearest(P, P)
    assert (d == 0).all()


def test_oracle_takes_the_lower_index_on_equal_distances():
    P = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, 0], [-1.0, 0, 0]])
    idx, d = nn3_oracle.nearest(P, np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]]))
    assert idx.tolist() == [0, 0, 0] and d.tolist() == [1.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        nn3_oracle.nearest(np.zeros((0, 3)), np.zeros((2, 3)))
    idx, d = nn3_oracle.nearest(P, np.zeros((0, 3)))
    assert idx.shape == d.shape == (0,)


FILTER_CASES = {
    # name: (src_dist, tgt_dist, surviving positions)
    "nothing above 1 mm": ([0.0, 0.0005, 0.0], [0.0, 0.0, 0.0009], [0, 1, 2]),
    "exactly 1 mm, nothing above: kept": ([0.0, 0.001, 0.0], [0.001, 0.0, 0.0], [0, 1, 2]),
    "some above": ([0.0, 0.5, 0.0, 0.0], [0.0, 0.0, 0.02, 0.0], [0, 3]),
    "exactly 1 mm next to one above: dropped": ([0.001, 0.0, 0.0, 0.0, 0.3], [0.0, 0.001, 0.0, 0.0, 0.0], [2, 3]),
    "only the target side above": ([0.0, 0.0], [0.0, 0.0011], [0]),
    "all dropped": ([0.2, 0.0], [0.0, 0.2], []),
}


@pytest.mark.parametrize("name", list(FILTER_CASES))
def test_row_filter_cases_oracle_and_product(name):
    torch = pytest.importorskip("torch")
    from vfmreg.registration import filter_recovered_rows
    sd, td, keep = FILTER_CASES[name]
    k = len(sd)
    si, ti = np.arange(100, 100 + k), np.arange(200, 200 + k)
    want = np.stack([si[keep], ti[keep]], 1).reshape(-1, 2).astype(np.int64)
    # the (K, 1) shapes sklearn returns, as the reference holds them
    got = nn3_oracle.filter_pairs(si.reshape(-1, 1), np.array(sd).reshape(-1, 1), ti.reshape(-1, 1), np.array(td).reshape(-1, 1))
    np.testing.assert_array_equal(got, want)
    prod = filter_recovered_rows(torch.from_numpy(si), torch.tensor(sd, dtype=torch.float64), torch.from_numpy(ti),
                                 torch.tensor(td, dtype=torch.float64))
    assert prod.dtype == torch.int64 and tuple(prod.shape) == want.shape
    np.testing.assert_array_equal(prod.numpy(), want)


def test_row_filter_is_the_reference_statement_on_random_inputs():
    torch = pytest.importorskip("torch")
    from vfmreg.registration import filter_recovered_rows
    rng = np.random.default_rng(3)
    for trial in range(20):
        k = int(rng.integers(1, 60))
        sd = np.where(rng.random(k) < 0.6, 0.0, rng.choice([0.001, 0.0009999, 0.0010001, 0.3], k))
        td = np.where(rng.random(k) < 0.6, 0.0, rng.choice([0.001, 0.0005, 0.02], k))
        if trial % 4 == 0:
            sd, td = np.minimum(sd, 0.001), np.minimum(td, 0.001)     # the unfiltered branch
        si, ti = rng.integers(0, 1000, k), rng.integers(0, 1000, k)
        want = nn3_oracle.filter_pairs(si, sd, ti, td)
        got = filter_recovered_rows(*(torch.from_numpy(a) for a in (si, sd, ti, td)))
        np.testing.assert_array_equal(got.numpy(), want)
    empty = filter_recovered_rows(*(torch.zeros(0, dtype=t) for t in (torch.int64, torch.float64, torch.int64, torch.float64)))
    assert tuple(empty.shape) == (0, 2)


def test_baselines_are_opt_in():
    pytest.importorskip("torch")
    from vfmreg.registration import RegistrationNode
    m, s = np.zeros((4, 3)), np.zeros((4, 3))
    node = RegistrationNode()
    assert node.baseline_methods == ()
    for name in ("fpfh", "dip", "gedi", "fcgf", "gcl", "spinnet", "teaser"):
        with pytest.raises(ValueError, match=f"Invalid method: {name}"):
            node.ransac_registration(m, s, name)
    node = RegistrationNode(baseline_methods=("fpfh",))
    for name in ("dip", "gedi", "fcgf", "gcl", "spinnet"):
        with pytest.raises(NotImplementedError):
            node.ransac_registration(m, s, name)
    with pytest.raises(ValueError, match="Invalid method: teaser"):
        node.ransac_registration(m, s, "teaser")
    with pytest.raises(ValueError, match="Invalid method"):
        RegistrationNode(baseline_methods=("teaser",))
    with pytest.raises(ValueError, match="Invalid shape"):
        node.ransac_registration(np.zeros((4, 2)), s, "fpfh")


def test_kdtree_stand_in_argument_checks():
    pytest.importorskip("torch")
    from vfmreg.neighbors import KDTree
    with pytest.raises(ValueError, match="0 sample"):
        KDTree(np.zeros((0, 3)), metric="euclidean")          # sklearn raises ValueError for an empty tree too
    with pytest.raises(NotImplementedError):
        KDTree(np.zeros((4, 3)), metric="manhattan")
    with pytest.raises(NotImplementedError):
        KDTree(np.zeros((4, 2)))
    with pytest.raises(ValueError):
        KDTree(np.zeros(4))


def test_nn3_entry_points_check_their_arguments_on_the_host():
    pytest.importorskip("torch")
    from vfmreg import _lib
    lib = _lib.load()
    assert {"vfm_nn3_workspace_bytes", "vfm_nn3_build", "vfm_nn3_query"} <= set(_lib.SIGNATURES)
    assert lib.vfm_nn3_workspace_bytes(200000) >= 200000 * 12
    assert lib.vfm_nn3_build(1, 0, 0.5, 1, 1, 1, 1, 1 << 30, None) == -1 and b"empty cloud" in lib.vfm_last_error()
    assert lib.vfm_nn3_query(1, 1, 1, 0, 0.5, 1, 0, 1, 1, None, None) == -1 and b"empty cloud" in lib.vfm_last_error()
    assert lib.vfm_nn3_build(1, 10, 0.0, 1, 1, 1, 1, 1 << 30, None) == -1 and b"cell" in lib.vfm_last_error()
    assert lib.vfm_nn3_build(1, 10, 0.5, 1, 1, 1, 1, lib.vfm_nn3_workspace_bytes(10) - 1, None) == -1 and b"workspace" in lib.vfm_last_error()
    assert lib.vfm_nn3_query(1, 1, 1, 10, -1.0, 1, 5, 1, 1, None, None) == -1
