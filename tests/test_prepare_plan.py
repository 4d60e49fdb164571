"""CPU checks of the preparation's plan (csrc/match_internal.h: resolve_prepare; read back through vfm_debug_prepare_plan): what a
preparation launches is resolved once, from the entry, its arguments and the calling thread's policy, and the read-back reports it without
touching a device.  The cases are tests/prep_plan_cases.py -- written from the launcher as it stood before the plan -- and the refusals of
tests/test_half_noi8_refusals.py."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import pytest

from . import prep_plan_cases as ppc
from .test_half_noi8_refusals import BIG

ROOT = Path(__file__).resolve().parent.parent
MX6, MX6_HALF, NO_I8 = ppc.MX6, ppc.MX6_HALF, ppc.NO_I8
# the preparation refusals of tests/test_half_noi8_refusals.py: (schedule, d) of _gated_p / _gated_z, and d of _gated_t with the flag
REFUSED_PZ = [(NO_I8, 384), (MX6 | NO_I8, 384), (MX6_HALF | NO_I8, 384), (1 | NO_I8, 256), (MX6 | MX6_HALF | NO_I8, 512),
              (MX6 | MX6_HALF | NO_I8, 768), (MX6 | MX6_HALF | NO_I8, 128), (MX6 | MX6_HALF | NO_I8 | 64, 384)]
REFUSED_T = [(d, dt1, dt2) for d in (256, 384) for dt1, dt2 in ((0, 0), (1, 1), (0, 1))]


@pytest.fixture(scope="module")
def built():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib


def plan_of(lib, case):
    rows1, rows2 = ppc.rows_of(case)
    with lib.using(lib.Config(**dict(case.cfg))):
        return lib.prepare_plan(ppc.ENTRIES[case.entry], case.schedule, case.d, rows1, rows2, *case.dtypes, zero=case.entry == "gated_z")


@pytest.mark.parametrize("case", [c for c in ppc.CASES if c.images is not None], ids=lambda c: c.id)
def test_the_read_back_equals_the_table(built, case):
    plan = plan_of(built, case)
    assert plan == {"images": list(case.images), "kernels": list(case.kernels), "grid": case.grid, "zero": case.zero}, plan


@pytest.mark.parametrize("case", [c for c in ppc.CASES if c.images is None], ids=lambda c: c.id)
def test_the_read_back_refuses_what_the_table_says_is_refused(built, case):
    with pytest.raises(RuntimeError, match=case.refusal):
        plan_of(built, case)
    # ... and so does the entry, with the same message, before any device call (fake pointers)
    lib = built.load()
    message = lib.vfm_last_error()
    with built.using(built.Config(**dict(case.cfg))):
        if case.entry == "gated_p":
            rc = lib.vfm_match_prepare2_gated_p(1, ppc.ROWS1, 1, 1, ppc.ROWS2, 1, case.d, case.schedule, None)
        else:
            rc = lib.vfm_match_prepare2_gated_z(1, ppc.ROWS1, 1, 1, ppc.ROWS2, 1, case.d, case.schedule, 1, BIG, ppc.ROWS2, ppc.ROWS1, None)
    assert rc != 0 and lib.vfm_last_error() == message


def test_the_zero_ranges_ride_inside_the_one_read_kernels_only(built):
    seen = set()
    for case in ppc.CASES:
        if case.images is None:
            continue
        assert (case.zero != "none") == (case.entry == "gated_z"), case.id
        if case.entry == "gated_z":
            assert (case.zero == "inside") == case.kernels[0].startswith("prep_once_kernel"), case.id
            seen.add(case.zero)
    assert seen == {"inside", "behind"}


def _read_back(lib, entry, schedule, d, dt1=0, dt2=0, zero=0, rows=(4096, 2100)):
    buf = C.create_string_buffer(1024)
    rc = lib.vfm_debug_prepare_plan(ppc.ENTRIES[entry], schedule, d, rows[0], dt1, rows[1], dt2, zero, buf, len(buf))
    return rc, lib.vfm_last_error()


@pytest.mark.parametrize("schedule,d", REFUSED_PZ)
def test_the_refusals_of_the_flag_come_from_the_read_back_with_the_entries_message(built, schedule, d):
    lib = built.load()
    for entry in ("gated_p", "gated_z"):
        rc, message = _read_back(lib, entry, schedule, d, zero=entry == "gated_z")
        assert rc != 0 and b"prepare2" in message
        if entry == "gated_p":
            assert lib.vfm_match_prepare2_gated_p(1, 4096, 1, 1, 2100, 1, d, schedule, None) != 0
        else:
            assert lib.vfm_match_prepare2_gated_z(1, 4096, 1, 1, 2100, 1, d, schedule, 1, BIG, 2100, 4096, None) != 0
        assert lib.vfm_last_error() == message


@pytest.mark.parametrize("d,dt1,dt2", REFUSED_T)
def test_the_typed_entrys_refusal_of_the_flag_too(built, d, dt1, dt2):
    lib = built.load()
    rc, message = _read_back(lib, "gated_t", MX6 | MX6_HALF | NO_I8, d, dt1, dt2)
    assert rc != 0 and b"VFM_PREPARE_NO_I8" in message
    assert lib.vfm_match_prepare2_gated_t(1, dt1, 4096, 1, 1, dt2, 2100, 1, d, MX6 | MX6_HALF | NO_I8, None) != 0
    assert lib.vfm_last_error() == message


def test_every_other_refusal_is_made_before_any_device_call(built):
    """bad width, unknown schedule, unknown row type, fp16 rows where the fp16 image or a non-int8 width is wanted: through the real
    entries with fake pointers, and through the read-back with the same message"""
    lib = built.load()
    calls = [
        ("prepare", 0, 100, 0, 0, lambda: lib.vfm_match_prepare(1, 4096, 100, 1, None), b"prepare: d must be"),
        ("prepare2", 0, 896, 0, 0, lambda: lib.vfm_match_prepare2(1, 4096, 1, 1, 2100, 1, 896, None), b"prepare2: d must be"),
        ("gated", 0, 0, 0, 0, lambda: lib.vfm_match_prepare2_gated(1, 4096, 1, 1, 2100, 1, 0, None), b"prepare2: d must be"),
        ("gated_p", 3, 384, 0, 0, lambda: lib.vfm_match_prepare2_gated_p(1, 4096, 1, 1, 2100, 1, 384, 3, None), b"unknown schedule"),
        ("gated_p", 64, 384, 0, 0, lambda: lib.vfm_match_prepare2_gated_p(1, 4096, 1, 1, 2100, 1, 384, 64, None), b"unknown schedule"),
        ("gated_t", 0, 384, 2, 0, lambda: lib.vfm_match_prepare2_gated_t(1, 2, 4096, 1, 1, 0, 2100, 1, 384, 0, None), b"unknown row type"),
        ("gated_t", MX6, 128, 1, 1, lambda: lib.vfm_match_prepare2_gated_t(1, 1, 4096, 1, 1, 1, 2100, 1, 128, MX6, None), b"fp16 rows"),
    ]
    for entry, schedule, d, dt1, dt2, call, text in calls:
        rows = (4096, 0) if entry == "prepare" else (4096, 2100)
        rc, message = _read_back(lib, entry, schedule, d, dt1, dt2, rows=rows)
        assert rc != 0 and text in message, (entry, message)
        assert call() != 0
        assert lib.vfm_last_error() == message
    with built.using(built.Config(i8_min_queries=2100)):   # the fp16 pass: it reads fp32 rows only
        rc, message = _read_back(lib, "gated_t", MX6, 384, 1, 0)
        assert rc != 0 and b"fp16 rows" in message
        assert lib.vfm_match_prepare2_gated_t(1, 1, 4096, 1, 1, 0, 2100, 1, 384, MX6, None) != 0 and lib.vfm_last_error() == message
    for rows in ((0, 2100), (4096, 0), (4096, -1)):
        assert _read_back(lib, "prepare2", 0, 384, rows=rows)[0] != 0
    assert lib.vfm_match_prepare2(1, 0, 1, 1, 2100, 1, 384, None) != 0
    assert lib.vfm_match_prepare2(None, 4096, 1, 1, 2100, 1, 384, None) != 0 and b"null pointer" in lib.vfm_last_error()


def test_the_read_back_checks_its_own_arguments(built):
    lib = built.load()
    buf = C.create_string_buffer(1024)
    assert lib.vfm_debug_prepare_plan(8, 0, 384, 4096, 0, 2100, 0, 0, buf, len(buf)) != 0 and b"unknown entry" in lib.vfm_last_error()
    assert lib.vfm_debug_prepare_plan(1, 0, 384, 4096, 0, 2100, 0, 0, buf, 8) != 0 and b"buffer" in lib.vfm_last_error()
    assert lib.vfm_debug_prepare_plan(1, 8, 384, 4096, 0, 2100, 0, 0, buf, len(buf)) != 0 and b"unknown schedule" in lib.vfm_last_error()


@pytest.mark.parametrize("d", [256, 384, 512])
@pytest.mark.parametrize("f16_rows", [False, True])
def test_the_pipeline_asks_for_no_int8_image_only_where_the_preparation_takes_the_flag(built, d, f16_rows):
    """RegistrationPipeline's condition for or-ing VFM_PREPARE_NO_I8 into the schedule against resolve_prepare, over the policy keys both
    read: true only where the plan of that schedule exists"""
    from vfmreg.pipeline import RegistrationPipeline
    n, m = 2100, 4096
    for half_noi8 in (0, 1):
        for form in (0, 1, 3, 4):
            cfg = built.Config(half_noi8=half_noi8, prep_form=form)
            pipe = RegistrationPipeline.__new__(RegistrationPipeline)   # (the rule's inputs only: no device)
            pipe.d, pipe.n, pipe.m, pipe.config, pipe._ws_clean = d, n, m, cfg, True
            pipe._noi8_shape = pipe._resolves(8 | 0x200)
            with built.using(cfg):
                wants = pipe._prepares_without_i8(8, False, f16_rows)
                try:
                    entry, dt = ("gated_t", 1) if f16_rows else ("gated_z", 0)
                    plan = built.prepare_plan(ppc.ENTRIES[entry], MX6 | MX6_HALF | NO_I8, d, m, n, dt, dt, zero=not f16_rows)
                except RuntimeError:
                    plan = None
            assert not wants or plan is not None, (half_noi8, form)
            if plan is not None:
                assert plan["images"] == ["fp6h"]
            assert wants == (half_noi8 == 1 and form in (3, 4) and d in (256, 384) and not f16_rows), (half_noi8, form)
