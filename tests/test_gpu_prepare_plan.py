"""Every row of the preparation's case table (tests/prep_plan_cases.py) through its real entry on the device: the call succeeds inside
guarded buffers, the images the plan does not list are not written, the images it lists decode to what tests/test_gpu_int8.py and
tests/test_gpu_mx6.py require of them, and the three gated entries that take a schedule write the same bytes.

Shape: 300 map rows and 130 scan rows -- three and two 128-row groups, each operand with a partly filled last group and tile, the
operand boundary inside every grid; the per-compute-unit and persistent rows run once more with two workgroups ("prep_grid" 2), so
that a workgroup walks several groups across that boundary."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402
from vfmreg import _lib  # noqa: E402

from . import prep_plan_cases as ppc  # noqa: E402
from .prepared_layout import prepared_layout  # noqa: E402
from .test_gpu_half_noi8 import workspace_layout  # noqa: E402
from .test_gpu_int8 import _heavy_tailed  # noqa: E402
from .test_gpu_mx6 import mx6_image  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
DEVICE_CASES = [c for c in ppc.CASES if c.images is not None and c.entry not in ppc.NO_EXPORT]
IMAGE_REGION = {"f16": "tiles", "i8": "tiles8", "fp6": "tiles6", "fp6h": "tiles6"}

_operands = {}


def _operand(d, which, f16):
    """rows of operand `which` (0: map, 1: scan) as the device gets them, and the oracle's normalised rows of what they widen to: made
    once per (d, operand, type), never written"""
    key = (d, which, f16)
    if key not in _operands:
        rng = np.random.default_rng(1000 * d + which)
        x = _heavy_tailed(rng, ppc.ROWS1, d) if which == 0 else rng.standard_normal((ppc.ROWS2, d)).astype(np.float32)
        if f16:
            x = x.astype(np.float16)
        xn, _ = orc.l2norm_rows(x.astype(np.float32))
        _operands[key] = (torch.from_numpy(x).cuda(), xn)
    return _operands[key]


def _run(case, cfg=None, schedule=None):
    """the case's entry in guarded buffers filled with 0xA5 (workspace: 0xFF); returns the GuardedBuffers [prepared1, prepared2 or None,
    workspace or None] and the operands' normalised rows"""
    lib = _lib.load()
    d = case.d
    schedule = case.schedule if schedule is None else schedule
    rows1, rows2 = ppc.rows_of(case)
    st = torch.cuda.current_stream().cuda_stream
    x1, n1 = _operand(d, 0, case.dtypes[0] == ppc.F16)
    x2, n2 = _operand(d, 1, case.dtypes[1] == ppc.F16) if rows2 else (None, None)
    p1 = GuardedBuffer(lib.vfm_match_prepared_bytes(rows1, d), torch.uint8, seed=3).fill_bytes(FILL)
    p2 = GuardedBuffer(lib.vfm_match_prepared_bytes(rows2, d), torch.uint8, seed=5).fill_bytes(FILL) if rows2 else None
    ws = None
    with _lib.using(_lib.Config(**dict(case.cfg if cfg is None else cfg))):
        if case.entry == "prepare":
            rc = lib.vfm_match_prepare(x1.data_ptr(), rows1, d, p1.ptr(), st)
        elif case.entry == "prepare2":
            rc = lib.vfm_match_prepare2(x1.data_ptr(), rows1, p1.ptr(), x2.data_ptr(), rows2, p2.ptr(), d, st)
        elif case.entry == "gated":
            rc = lib.vfm_match_prepare2_gated(x1.data_ptr(), rows1, p1.ptr(), x2.data_ptr(), rows2, p2.ptr(), d, st)
        elif case.entry == "gated_p":
            rc = lib.vfm_match_prepare2_gated_p(x1.data_ptr(), rows1, p1.ptr(), x2.data_ptr(), rows2, p2.ptr(), d, schedule, st)
        elif case.entry == "gated_t":
            rc = lib.vfm_match_prepare2_gated_t(x1.data_ptr(), case.dtypes[0], rows1, p1.ptr(), x2.data_ptr(), case.dtypes[1], rows2, p2.ptr(), d,
                                                schedule, st)
        else:
            ws = GuardedBuffer(lib.vfm_match_search_workspace_bytes(rows2, rows1, d), torch.uint8, seed=7).fill_bytes(0xFF)
            rc = lib.vfm_match_prepare2_gated_z(x1.data_ptr(), rows1, p1.ptr(), x2.data_ptr(), rows2, p2.ptr(), d, schedule, ws.ptr(), ws.nbytes,
                                                rows2, rows1, st)
        _lib.check(rc, case.id)
    torch.cuda.synchronize()
    return [p1, p2, ws], [n1, n2]


def _region(buf, lay, name):
    off, nbytes = lay[name]
    return buf.body[off:off + nbytes]


def _check_i8(buf, rows, d, xn):
    """tests/test_gpu_int8.py, test_quantisation_bound_holds_for_every_pair: the measured E bounds the residual of the oracle's rows"""
    lib = _lib.load()
    q8 = np.empty((rows, d), np.int8)
    step, err, gerr = (np.empty(rows, np.float32) for _ in range(3))
    _lib.check(lib.vfm_debug_i8_rows(buf.ptr(), rows, d, q8.ctypes.data, step.ctypes.data, err.ctypes.data, gerr.ctypes.data))
    res = np.linalg.norm(xn.astype(np.float64) - step[:, None].astype(np.float64) * q8.astype(np.float64), axis=1)
    assert (err.astype(np.float64) >= res).all()
    assert (np.abs(q8.astype(np.int32)) <= 127).all()
    assert (gerr >= err).all()


def _check_fp6(buf, rows, d, xn, half):
    """tests/test_gpu_mx6.py, the two image tests: the image is the definition's, bit for bit; E is at least the true residual and at
    most that + the declared roundings; a group's value is the maximum of its rows.  Half: the first d / 2 columns, the full-width E infinite."""
    lib = _lib.load()
    v6 = np.empty((rows, d), np.float32)
    err, gerr, errh, gerrh = (np.empty(rows, np.float32) for _ in range(4))
    _lib.check(lib.vfm_debug_mx6_rows(buf.ptr(), rows, d, v6.ctypes.data, err.ctypes.data, gerr.ctypes.data))
    _lib.check(lib.vfm_debug_mx6_half_err(buf.ptr(), rows, d, errh.ctypes.data, gerrh.ctypes.data))
    h = d // 2
    want = mx6_image(xn)
    if half:
        np.testing.assert_array_equal(v6[:, :h].astype(np.float64), want[:, :h])
        assert np.isinf(err).all() and np.isinf(gerr).all()
    else:
        np.testing.assert_array_equal(v6.astype(np.float64), want)
        true = np.linalg.norm(xn.astype(np.float64) - v6.astype(np.float64), axis=1)
        assert (err >= true).all() and (err <= true * 1.0003 + 1.1e-3).all()
        np.testing.assert_array_equal(gerr[::128], np.array([err[g:g + 128].max() for g in range(0, rows, 128)]))
        assert (errh <= err).all()
    true_h = np.linalg.norm(xn[:, :h].astype(np.float64) - v6[:, :h].astype(np.float64), axis=1)
    assert (errh >= true_h).all() and (errh <= true_h * 1.0003 + 1.1e-3).all()
    np.testing.assert_array_equal(gerrh[::128], np.array([errh[g:g + 128].max() for g in range(0, rows, 128)]))


def _check(case, bufs, normed):
    for buf in bufs:
        if buf is not None:
            chk = buf.intact()
            assert chk, repr(chk)
    for buf, xn, rows in zip(bufs[:2], normed, ppc.rows_of(case)):
        if buf is None:
            continue
        lay = prepared_layout(rows, case.d)
        assert lay["_end"][0] == buf.nbytes
        listed = {IMAGE_REGION[im] for im in case.images}
        for name in ("tiles", "tiles8", "tiles6"):
            if name in lay and name not in listed:
                assert bool((_region(buf, lay, name) == FILL).all()), (case.id, name)
            elif name in lay:
                assert bool((_region(buf, lay, name) != FILL).any()), (case.id, name)
        if "i8" in case.images:
            _check_i8(buf, rows, case.d, xn)
        if "fp6" in case.images or "fp6h" in case.images:
            _check_fp6(buf, rows, case.d, xn, "fp6h" in case.images)
    ws = bufs[2]
    if case.entry == "gated_z":   # what a coarse pass wants zero is zero, and not a byte more
        lay, _, _ = workspace_layout(ppc.ROWS2, ppc.ROWS1)
        assert lay["_end"][0] == ws.nbytes
        cleared = torch.zeros(ws.nbytes, dtype=torch.bool, device="cuda")
        for lo, hi in ((lay["cand_cnt"][0], lay["cand_cnt"][0] + lay["cand_cnt"][1]), (lay["fb_count"][0], lay["qbest"][0] + lay["qbest"][1])):
            cleared[lo:hi] = True
        assert bool((ws.body[cleared] == 0).all()) and bool((ws.body[~cleared] == 0xFF).all()), case.id


@pytest.mark.parametrize("case", DEVICE_CASES, ids=lambda c: c.id)
def test_a_row_of_the_table_through_its_entry(case):
    bufs, normed = _run(case)
    _check(case, bufs, normed)
    if case.grid in ("cu", "2cu-stream"):
        # two workgroups for five groups: the chunk kernel takes "prep_grid" under VFM_PREPARE_DEFAULT, the persistent one-read form always
        again, _ = _run(case, cfg=tuple(dict(case.cfg, prep_grid=2).items()), schedule=case.schedule & ~3)
        _check(case, again, normed)
        for a, b in zip(bufs, again):
            assert a is None or torch.equal(a.body, b.body), case.id


@pytest.mark.parametrize("schedule,d", [(0, 384), (ppc.PERSISTENT, 768), (ppc.MX6, 256), (ppc.MX6 | ppc.MX6_HALF, 384), (ppc.MX6, 512),
                                        (ppc.MX6 | ppc.MX6_HALF, 768), (ppc.MX6, 640), (ppc.INTERLEAVED, 128)])
def test_the_three_scheduled_entries_write_the_same_bytes_for_fp32_rows(schedule, d):
    runs = [_run(ppc.Case(f"{entry}-s{schedule}-d{d}", entry, schedule, d, (), (ppc.F32, ppc.F32), ()))[0] for entry in ("gated_p", "gated_z", "gated_t")]
    for other in runs[1:]:
        for a, b in zip(runs[0][:2], other[:2]):
            assert torch.equal(a.body, b.body), (schedule, d)
