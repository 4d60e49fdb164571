"""csrc/fpfh.hip through the exits its structured-scene test never takes: the hand-made neighbour rows of tests/fpfh_branch_cases.py
fed straight into ops.fpfh_normals / fpfh_spfh / fpfh_fpfh, against the numpy oracle.  tests/test_fpfh_oracle.py counts on the CPU
which exit every row takes (at least 3 rows each) and that no row is within 1e-9 of a bin edge or of the swap decision unless it
sits there exactly; so no row is left out here."""
import numpy as np
import pytest
import torch

from tests import fpfh_branch_cases as bc
from tests import fpfh_oracle as fo
from tests.test_fpfh_oracle import gapped_rows

pytestmark = pytest.mark.gpu


def dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def rows_dev(c):
    nb = dict(idx=dev(c["idx"], np.int32), count=dev(c["count"], np.int32))
    if "d2" in c:
        nb["d2"] = dev(c["d2"])
    return nb


def test_normals_of_the_crafted_rows():
    from vfmreg import ops
    c = bc.normal_cases()
    C = fo.covariances(c["pts"], c["idx"], c["count"])
    _, ex, _, _ = fo.fast_eigen3x3(C, branches=True)
    ref = fo.estimate_normals(c["pts"], c["idx"], c["count"])
    nv = ops.fpfh_normals(dev(c["pts"]), rows_dev(c)).cpu().numpy()
    assert np.isfinite(nv).all()
    # exits without a libm call (zero, diagonal, fewer than 3 neighbours): bit-equal
    plain = ex <= fo.EIG_DIAG_TIE
    np.testing.assert_array_equal(nv[plain], ref[plain])
    # a unique smallest eigenvalue: the existing scene test's rule and number
    gapped, _ = gapped_rows(C)
    g = gapped & ~plain
    assert g.sum() >= 60
    err = np.abs(nv[g] - ref[g]).max(1)
    print("gapped rows", int(g.sum()), "max |normal - oracle|", err.max())
    assert err.max() <= 1e-9, np.flatnonzero(g)[err.argmax()]
    big = np.abs(ref[g]) > 1e-6
    np.testing.assert_array_equal(np.sign(nv[g][big]), np.sign(ref[g][big]))
    # the normal is not unique (needles, prolate and isotropic blobs): properties
    free = ~gapped & ~plain
    assert free.sum() >= 60
    length = np.sqrt((nv[free] ** 2).sum(1))
    print("free rows", int(free.sum()), "max |length - 1|", np.abs(length - 1).max())
    assert np.abs(length - 1.0).max() <= 1e-9
    has_axis = free & (np.abs(c["axis"]).sum(1) > 0)
    assert has_axis.sum() >= 30
    dot_ref = np.abs(np.einsum("ij,ij->i", ref[has_axis], c["axis"][has_axis]))
    dot = np.abs(np.einsum("ij,ij->i", nv[has_axis], c["axis"][has_axis]))
    print("perpendicularity: oracle", dot_ref.max(), "device", dot.max())
    # the oracle's own worst |normal . axis| on these rows is 6.8e-4 (a needle jittered by 1e-3 over a length of 2); ten times that
    assert dot_ref.max() <= 6.8e-4 and dot.max() <= 6.8e-3


def test_spfh_and_fpfh_of_the_crafted_rows():
    from vfmreg import ops
    f = bc.feature_cases()
    sp_ref, near = fo.spfh(f["pts"], f["normals"], f["idx"], f["count"], exact_ok=True)
    f_ref, fnear = fo.fpfh(sp_ref, f["idx"], f["d2"], f["count"], near)
    assert not near.any() and not fnear.any()
    nb = rows_dev(f)
    sp = ops.fpfh_spfh(dev(f["pts"]), dev(f["normals"]), nb)
    out = ops.fpfh_fpfh(sp, nb).cpu().numpy()
    sp = sp.cpu().numpy()
    bad = np.flatnonzero((sp != sp_ref).any(1))
    assert len(bad) == 0, [(int(r), f["kind"][r]) for r in bad[:10]]           # counts times one increment: bit-equal, no row left out
    err = np.abs(out - f_ref) / np.maximum(np.abs(f_ref), 1.0)
    print("fpfh max scaled error", err.max())
    bad = np.flatnonzero((err > 1e-9).any(1))
    assert len(bad) == 0, [(int(r), f["kind"][r]) for r in bad[:10]]
    # the oracle's rows on the device's own SPFH: the FPFH kernel alone
    f2, _ = fo.fpfh(sp, f["idx"], f["d2"], f["count"])
    assert (np.abs(out - f2) <= 1e-9 * np.maximum(np.abs(f2), 1.0)).all()
    assert (out[f["count"] <= 1] == 0).all()
