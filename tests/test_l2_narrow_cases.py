"""CPU: the inputs of tests/l2_narrow_cases.py have the properties their docstrings claim (checked with the oracle alone), and the host
side of VFM_MATCH_NARROW refuses what it must before anything is launched."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import l2_narrow_cases as cases

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def built():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------ the generators
@pytest.mark.parametrize("d", cases.TIE_WIDTHS)
def test_tie_cases_hold_ties_and_the_oracle_picks_the_lower_copy(orc, d):
    for name, (a, b, pairs) in cases.tie_cases(d).items():
        idx, dist = orc.nn_l2(a, b)
        for q, lo, hi in pairs:
            assert lo < hi and np.array_equal(b[lo], b[hi]), name
            assert idx[q] == lo, f"{name}: query {q} -> {idx[q]}, planted {lo} | {hi}"
            d_hi = np.sqrt(((a[q].astype(np.float64) - b[hi].astype(np.float64)) ** 2).sum())
            assert np.isclose(dist[q], d_hi, rtol=1e-12), name
    # the geometry the names claim
    t = cases.tie_cases(d)
    assert t["tile edge"][2] == [(0, 31, 32)]
    assert all(lo // 32 == hi // 32 and hi - lo == 4 and (lo % 8) < 4 for _, lo, hi in t["lane halves"][2])
    m = t["every tile edge"][1].shape[0]
    assert sorted(hi for _, _, hi in t["every tile edge"][2]) == list(range(32, m, 32))


@pytest.mark.parametrize("d", cases.TIE_WIDTHS)
def test_degenerate_cases(orc, d):
    a, b = cases.zero_distance_case(d)
    idx, dist = orc.nn_l2(a, b)
    assert np.array_equal(dist, np.zeros(len(a))) and list(idx) == [17, 0, 299, 150]   # row 17 again at 200: the lower copy
    a, b = cases.all_zero_case(d)
    idx, dist = orc.nn_l2(a, b)
    assert idx[1] == 3 and idx[4] == 3 and dist[1] == 0 and dist[4] == 0
    a, b = cases.only_zero_case(d)
    idx, dist = orc.nn_l2(a, b)
    assert not idx.any() and not dist.any()
    a, b = cases.identical_map_case(d)
    assert b.shape[0] == 300 and (b == b[0]).all() and not orc.nn_l2(a, b)[0].any()


def test_near_ties_are_below_what_f32_resolves(orc):
    a, b, order = cases.near_tie_case()
    idx, dist = orc.nn_l2(a, b)
    # fp64: six distinct distances j 2^-17, the nearest row (j = 1) is not row 0
    d64 = np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(1))
    assert np.array_equal(d64, order * 2.0 ** -17) and len(set(d64)) == 6
    assert idx[0] == int(np.argmin(order)) != 0 and dist[0] == 2.0 ** -17
    # f32: |b|^2 - 2 a.b of the six rows differ, in exact arithmetic, by less than half an ulp of its f32 value -- the f32 values coincide
    # (up to their own rounding), on the raw rows and on the scaled ones
    s = cases.common_scale(a, b)
    for scale in (1.0, s):
        A, B = a.astype(np.float64) * scale, b.astype(np.float64) * scale
        c = (B * B).sum(1) - 2.0 * (B @ A[0])
        assert np.ptp(c) < 0.5 * float(np.spacing(np.float32(np.abs(c).min())))
    c32 = (np.float32(s) * b).astype(np.float32)
    c32 = (c32 * c32).sum(1, dtype=np.float32) - np.float32(2) * (c32 @ (np.float32(s) * a[0]))
    assert np.ptp(c32.astype(np.float64)) <= cases.window(33)   # ... and whatever f32 makes of them stays inside the window


def test_scale_cases_need_the_common_scale(orc):
    sc = cases.scale_cases()
    assert set(sc) == {"x 2^40", "x 2^-40", "x 2^62", "one long map row"}
    base_idx = None
    for name, (a, b) in sc.items():
        assert np.isfinite(a).all() and np.isfinite(b).all(), name
        s = cases.common_scale(a, b)
        As, Bs = (np.float32(s) * a).astype(np.float32), (np.float32(s) * b).astype(np.float32)
        na, nb = np.sqrt((As.astype(np.float64) ** 2).sum(1)), np.sqrt((Bs.astype(np.float64) ** 2).sum(1))
        assert max(na.max(), nb.max()) <= 1.0 and max(na.max(), nb.max()) > 0.24, name
        with np.errstate(over="ignore", invalid="ignore"):
            raw = a[:, None, :] * b[None, :8, :]              # f32 products a_k b_k on the rows as given
            scaled = As[:, None, :] * Bs[None, :8, :]
        assert np.isfinite(scaled).all(), name
        if name == "x 2^62":
            assert not np.isfinite(raw).all()   # finite in f32 only after the common scaling
        else:
            assert np.isfinite(raw).all()
        # the window is absolute on the scaled rows: on the raw ones it would be far above every c (nothing pruned) or far below one ulp
        # of c (no bound at all)
        c_raw = np.abs((b.astype(np.float64) ** 2).sum(1)).max()
        if name != "one long map row":
            assert c_raw < 1e-3 * cases.window(33) or float(np.spacing(np.float32(min(c_raw, 3e38)))) > 1e3 * cases.window(33), name
            idx = orc.nn_l2(a, b)[0]      # powers of two: the answer does not change
            base_idx = idx if base_idx is None else base_idx
            assert np.array_equal(idx, base_idx), name
        else:
            assert nb[123] > 1e3 * np.delete(nb, 123).max()
            assert 123 not in orc.nn_l2(a, b)[0]


def test_shapes_cover_the_widths_and_both_launch_forms(built):
    lib = built.load()
    assert 33 in cases.WIDTHS and 64 in cases.WIDTHS and any(d % 2 for d in cases.WIDTHS)
    slices = [lib.vfm_debug_l2_narrow_slices(n, m) for n, m in cases.SHAPES]
    assert 1 in slices and max(slices) >= 2, slices
    n, m = cases.tie_cases(7)["every tile edge"][0].shape[0], 4099
    assert lib.vfm_debug_l2_narrow_slices(n, m) >= 2
    assert lib.vfm_debug_l2_narrow_slices(0, 5) == 0


# ------------------------------------------------------------------------------------------------------------ the host side of the ABI
def test_narrow_mode_is_checked_on_the_host(built):
    lib = built.load()
    need = lib.vfm_match_mutual_l2_workspace_bytes(10, 10, 64, cases.NARROW, 1)
    assert need > lib.vfm_match_mutual_l2_workspace_bytes(10, 10, 64, cases.NARROW, 0) > 256
    # d = 65: refused, the message names the mode and the limit
    assert lib.vfm_match_mutual_l2(1, 10, 1, 10, 65, cases.NARROW, 1, None, None, 1, 1 << 30, None) == -1
    msg = lib.vfm_last_error()
    assert b"NARROW" in msg and b"64" in msg, msg
    # d = 64: accepted as a mode -- the call gets as far as the workspace check, which refuses an undersized one
    rc = lib.vfm_match_mutual_l2(1, 10, 1, 10, 64, cases.NARROW, 1, None, 1, 1, need - 1, None)
    assert rc != 0 and rc != -1 and b"workspace" in lib.vfm_last_error()
    rc = lib.vfm_match_mutual_l2(1, 10, 1, 10, 33, cases.NARROW, 1, None, None, 1, 16, None)
    assert rc != 0 and b"workspace" in lib.vfm_last_error()
    # the pairs entry point sizes its narrow path the same way
    need = lib.vfm_match_mutual_pairs_workspace_bytes(10, 10, 33)
    assert lib.vfm_match_mutual_pairs(1, 10, 1, 10, 33, 1, 1, 1, None, None, 1, need - 1, None) != 0 and b"workspace" in lib.vfm_last_error()
    # FAST and EXACT size their workspaces as before
    assert lib.vfm_match_mutual_l2_workspace_bytes(10, 10, 65, cases.NARROW, 1) == 256
    assert lib.vfm_match_mutual_l2_workspace_bytes(10, 10, 33, 1, 1) == 256


def test_ops_refuses_wide_rows_before_calling_the_library(built):
    torch = pytest.importorskip("torch")
    from vfmreg import ops
    assert ops.NARROW == cases.NARROW and ops.NARROW_MAX_D == cases.NARROW_MAX_D

    class _Fake(torch.Tensor):   # passes the wrapper's device check without a device
        is_cuda = True
    a = torch.zeros(3, 65).as_subclass(_Fake)
    with pytest.raises(ValueError, match="NARROW"):
        ops.match_mutual_l2(a, a, prec=ops.NARROW)


def test_the_forward_search_takes_narrow_from_the_measured_size_on():
    """profiles/l2_narrow_timing.md: NARROW lost to FAST on random 5000 x 5000 x 33, so find_correspondences_device picks it by size"""
    pytest.importorskip("torch")
    from vfmreg import ops, registration
    x = registration.NARROW_MIN_ROWS
    assert 5000 < x <= 17651                                   # the random shape that lost stays on FAST, the FPFH row's scan side alone qualifies
    assert registration.l2_search_mode(5000, 5000, 33) == ops.FAST
    assert registration.l2_search_mode(x - 1, x - 1, 33) == ops.FAST
    assert registration.l2_search_mode(x, 1, 33) == ops.NARROW and registration.l2_search_mode(1, x, 33) == ops.NARROW
    assert registration.l2_search_mode(18563, 200000, 33) == ops.NARROW
    assert registration.l2_search_mode(18563, 200000, 64) == ops.NARROW
    assert registration.l2_search_mode(18563, 200000, 65) == ops.FAST
    assert registration.l2_search_mode(20000, 200000, 384) == ops.FAST
