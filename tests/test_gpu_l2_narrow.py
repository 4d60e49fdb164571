"""VFM_MATCH_NARROW on the device (csrc/match_l2_narrow.hip): the inputs of tests/l2_narrow_cases.py through vfm_match_mutual_l2 (with and
without the reverse direction), vfm_match_mutual_pairs and the guarded-buffer harness of tests/test_gpu_bounds.py.  Every comparison is
exact equality with oracle.nn_l2 / oracle.find_correspondences."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import l2_narrow_cases as cases  # noqa: E402
from tests.test_gpu_bounds import check_case, mutual_l2_case, mutual_pairs_case  # noqa: E402

pytestmark = pytest.mark.gpu

NARROW = cases.NARROW


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def ops():
    from vfmreg import ops as o
    return o


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_REFS = {}


def _ref(orc, a, b, key):
    """the oracle's answers for one input, computed once: (nn_ab, dist_ab, nn_ba, mutual idx0, mutual idx1)"""
    if key not in _REFS:
        i_ab, dist = orc.nn_l2(a, b)
        i_ba, _ = orc.nn_l2(b, a)
        keep = i_ba[i_ab] == np.arange(len(i_ab))
        _REFS[key] = (i_ab, dist, i_ba, np.arange(len(i_ab))[keep], i_ab[keep])
    return _REFS[key]


def _evals(ws):
    from vfmreg import _lib
    out = (C.c_int64 * 2)()
    _lib.check(_lib.load().vfm_debug_l2_narrow_evals(ws.data_ptr(), out), "l2_narrow_evals")
    return int(out[0]), int(out[1])


def _check_all(ops, orc, a, b, key):
    """both forms of vfm_match_mutual_l2 and vfm_match_mutual_pairs against the oracle"""
    i_ab, dist, i_ba, m0, m1 = _ref(orc, a, b, key)
    ad, bd = _dev(a), _dev(b)
    for mutual in (True, False):
        nn_ab, d2, nn_ba = ops.match_mutual_l2(ad, bd, mutual=mutual, prec=ops.NARROW)
        np.testing.assert_array_equal(nn_ab.cpu().numpy(), i_ab, err_msg=f"{key} nn_ab mutual={mutual}")
        np.testing.assert_array_equal(np.sqrt(d2.cpu().numpy()), dist, err_msg=f"{key} d2 mutual={mutual}")
        if mutual:
            np.testing.assert_array_equal(nn_ba.cpu().numpy(), i_ba, err_msg=f"{key} nn_ba")
        else:
            assert nn_ba is None
    i0, i1, cnt, nn_ab, d2 = ops.match_mutual_pairs(ad, bd, want_nn=True)
    k = int(cnt.item())
    np.testing.assert_array_equal(i0[:k].cpu().numpy(), m0, err_msg=f"{key} pairs idx0")
    np.testing.assert_array_equal(i1[:k].cpu().numpy(), m1, err_msg=f"{key} pairs idx1")
    np.testing.assert_array_equal(nn_ab.cpu().numpy(), i_ab, err_msg=f"{key} pairs nn_ab")
    np.testing.assert_array_equal(np.sqrt(d2.cpu().numpy()), dist, err_msg=f"{key} pairs d2")


# ------------------------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("d", cases.WIDTHS)
def test_shapes_equal_the_oracle(ops, orc, d):
    for n, m in cases.SHAPES:
        a, b = cases.random_pair(n, m, d)
        _check_all(ops, orc, a, b, ("shape", n, m, d))


def test_one_slice_and_several_slices_are_launched_and_counted(ops, orc):
    from vfmreg import _lib
    lib = _lib.load()
    slices = {(n, m): lib.vfm_debug_l2_narrow_slices(n, m) for n, m in cases.SHAPES}
    assert 1 in slices.values() and max(slices.values()) >= 2, slices
    d = 33
    for (n, m), s in slices.items():
        a, b = cases.random_pair(n, m, d)
        ad, bd = _dev(a), _dev(b)
        nn_ab = torch.empty(n, dtype=torch.int64, device="cuda")
        d2 = torch.empty(n, dtype=torch.float64, device="cuda")
        nn_ba = torch.empty(m, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.vfm_match_mutual_l2_workspace_bytes(n, m, d, NARROW, 1), dtype=torch.uint8, device="cuda")
        _lib.check(lib.vfm_match_mutual_l2(ad.data_ptr(), n, bd.data_ptr(), m, d, NARROW, nn_ab.data_ptr(), d2.data_ptr(), nn_ba.data_ptr(),
                                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "mutual_l2")
        fwd, rev = _evals(ws)
        # every (query, slice) evaluates at least the first row it screens; nothing is evaluated twice
        assert n * s <= fwd <= n * m and m * lib.vfm_debug_l2_narrow_slices(m, n) <= rev <= n * m, (n, m, s, fwd, rev)
        np.testing.assert_array_equal(nn_ab.cpu().numpy(), _ref(orc, a, b, ("shape", n, m, d))[0])


# ------------------------------------------------------------------------------------------------------------------ 2. exact ties
@pytest.mark.parametrize("d", cases.TIE_WIDTHS)
def test_exact_ties_return_the_lowest_index(ops, orc, d):
    for name, (a, b, pairs) in cases.tie_cases(d).items():
        _check_all(ops, orc, a, b, ("tie", name, d))
        nn = ops.match_mutual_l2(_dev(a), _dev(b), mutual=False, prec=ops.NARROW)[0].cpu().numpy()
        for q, lo, hi in pairs:
            assert nn[q] == lo, (name, q, lo, hi, nn[q])
    for name, gen in (("zero distance", cases.zero_distance_case), ("zero rows", cases.all_zero_case), ("only zero rows", cases.only_zero_case),
                      ("identical map", cases.identical_map_case)):
        a, b = gen(d)
        _check_all(ops, orc, a, b, (name, d))
    a, b = cases.identical_map_case(d)
    assert not ops.match_mutual_l2(_dev(a), _dev(b), mutual=False, prec=ops.NARROW)[0].any().item()


# ------------------------------------------------------------------------------------------------------------------ 3. near-ties
def test_near_ties_below_the_f32_window_are_decided_in_fp64(ops, orc):
    a, b, order = cases.near_tie_case()
    _check_all(ops, orc, a, b, ("near ties",))
    nn_ab, d2, _ = ops.match_mutual_l2(_dev(a), _dev(b), mutual=False, prec=ops.NARROW)
    assert int(nn_ab[0].item()) == int(np.argmin(order)) != 0 and float(d2[0].item()) == 2.0 ** -34
    # ... among many other rows, too
    rng = np.random.default_rng(11)
    others = np.stack([cases.fpfh_like_row(rng) for _ in range(2000)])
    big = np.concatenate([others[:777], b, others[777:]])
    _check_all(ops, orc, a, big, ("near ties in a map",))


# ------------------------------------------------------------------------------------------------------------------ 4. scale
def test_scaled_inputs_and_one_long_row(ops, orc):
    for name, (a, b) in cases.scale_cases().items():
        _check_all(ops, orc, a, b, ("scale", name))


# ------------------------------------------------------------------------------------------------------------------ 5. real features
@pytest.mark.parametrize("seed", cases.FPFH_SEEDS)
def test_fpfh_features_of_a_structured_scene(ops, orc, seed):
    from vfmreg.descriptors import extract_fpfh_features_device
    from vfmreg.registration import find_correspondences_device
    sc = cases.fpfh_scene(seed)
    f0 = extract_fpfh_features_device(_dev(sc["scan"]), 0.1)[1].float().contiguous()
    f1 = extract_fpfh_features_device(_dev(sc["map"]), 0.1)[1].float().contiguous()
    a, b = f0.cpu().numpy(), f1.cpu().numpy()
    assert a.shape[1] == 33 and a.shape[0] > 200 and b.shape[0] > 1000
    _check_all(ops, orc, a, b, ("fpfh", seed))
    for mutual_filter in (True, False):
        i0, i1 = find_correspondences_device(f0, f1, 500, mutual_filter)
        r0, r1 = orc.find_correspondences(a, b, 500, mutual_filter)
        np.testing.assert_array_equal(i0.cpu().numpy(), r0, err_msg=f"mutual_filter={mutual_filter}")
        np.testing.assert_array_equal(i1.cpu().numpy(), r1, err_msg=f"mutual_filter={mutual_filter}")


# ------------------------------------------------------------------------------------------------------------------ buffers
@pytest.mark.parametrize("d", cases.WIDTHS)
@pytest.mark.parametrize("n,m", cases.SHAPES)
def test_narrow_search_stays_in_its_buffers(orc, n, m, d):
    for mutual in (True, False):
        check_case(mutual_l2_case(n, m, d, NARROW, mutual, orc))
    check_case(mutual_pairs_case(n, m, d, orc))
