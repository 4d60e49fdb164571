"""CPU checks of the coarse pass's launch plan (csrc/match_internal.h: resolve_coarse; read back through vfm_debug_coarse_plan): which
kernel a search launches and on what grid is resolved once, and the read-back reports it without touching a device.  The cases are the
dispatch table's (tests/match_dispatch_cases.py): every "this shape and config gives this kernel" of it is checked here, on the host."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

from . import match_dispatch_cases as mdc

ROOT = Path(__file__).resolve().parent.parent
CUS = 256
ALL_CASES = mdc.CASES + mdc.PADDING_CASES


@pytest.fixture(scope="module")
def built():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib


def l2_padded_k(d: int) -> int:
    """the width the Euclidean entry's fp16 pass runs at: d + 2 columns padded to 128 for d <= 510, d itself (with a row bias) above"""
    return (d + 2 + 127) // 128 * 128 if d <= 510 else d


def ask(lib, case, compute_units=CUS):
    """(the case's coarse plan under its config, chunks of its padded map).  An "l2" case is asked at what its LAST launch has: the reverse
    direction -- the m rows of b as queries among the n rows of a -- at the padded K, dense fp16 records, a row bias where K = d."""
    with lib.using(lib.Config(**dict(case.cfg))):
        if case.entry == "l2":
            n, m = case.m, case.n
            plan = lib.coarse_plan(mdc.BEST, l2_padded_k(case.d), n, m, gated=False, inner_product=False, row_bias=case.d > 510,
                                   compute_units=compute_units)
        else:
            n, m = case.n, case.m
            plan = lib.coarse_plan(case.records, case.d, n, m, gated=case.gated, compute_units=compute_units)
    return plan, (m + 255) // 256 * 2


def fp6_shape(kernel: str):
    """(KS6, KIND, IMG_KS6, T) of an fp6 kernel's name, None for the others"""
    hit = re.match(r"mx6q2<(\d+),(\w+),low=\d,img=(\d+),ring=\d,T=(\d),", kernel)
    return hit and (int(hit.group(1)), hit.group(2), int(hit.group(3)), int(hit.group(4)))


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_the_plan_names_the_kernel_of_the_case_on_a_grid_that_fits(built, case):
    plan, nchunks = ask(built, case)
    assert plan["kernel"] == case.kernel, plan
    assert 1 <= plan["nslices"] <= nchunks and plan["nqb"] >= 1, (plan, nchunks)
    assert (plan["seed"] > 0) == ("+seed" in plan["kernel"]), plan
    assert plan["block"] in (256, 512) and 0 < plan["lds"] <= 160 * 1024, plan
    fp6 = fp6_shape(plan["kernel"])
    if fp6:
        assert -(-nchunks // plan["nslices"]) + 1 <= 256, (plan, nchunks)        # a slice's constants fit the kernel's LDS table
        if fp6[3] == 8:                                                         # two chunks per barrier: whole pairs of chunks per slice
            assert plan["nslices"] <= nchunks // 2, (plan, nchunks)
    else:
        assert "T=8" not in plan["kernel"] and plan["tune"] == 0, plan


def test_the_table_has_l2_cases_at_every_padded_width():
    assert sorted(l2_padded_k(c.d) for c in mdc.CASES if c.entry == "l2") == [128, 256, 384, 512, 640, 768]


@pytest.mark.parametrize("cfg", mdc.VARIANT_CONFIGS, ids=["-".join(f"{k}={v}" for k, v in c) for c in mdc.VARIANT_CONFIGS])
def test_the_read_back_refuses_the_slice_counts_the_survivor_slots_cannot_hold(built, cfg):
    for d, n, m, records in mdc.VARIANT_WORKLOADS:
        with built.using(built.Config(**dict(cfg))):
            if mdc.mx6_fused_slices_refused(records, m, cfg):
                with pytest.raises(RuntimeError, match="survivor slots"):
                    built.coarse_plan(records, d, n, m, compute_units=CUS)
            else:
                assert built.coarse_plan(records, d, n, m, compute_units=CUS)["nslices"] >= 1


def test_the_compute_unit_count_moves_slices_of_the_fused_half_width_fp6_pass_and_never_the_kernel(built):
    moved = []
    for case in ALL_CASES:
        small, _ = ask(built, case, 256)
        large, _ = ask(built, case, 304)
        assert small["kernel"] == large["kernel"] == case.kernel
        fp6 = fp6_shape(case.kernel)
        if small["nslices"] != large["nslices"]:
            assert fp6 and 2 * fp6[0] == fp6[2], (case.id, small, large)       # only the half-width fp6 slice search asks for the count
            if fp6[1] == "FUSE":
                moved.append(case.id)
    assert moved


def test_the_read_back_checks_its_arguments_and_refuses_what_the_search_refuses(built):
    import ctypes as C
    lib = built.load()
    buf = C.create_string_buffer(1024)
    assert lib.vfm_debug_coarse_plan(11, 384, 2100, 4096, 1, 1, 0, CUS, buf, len(buf)) != 0 and b"unknown record kind" in lib.vfm_last_error()
    assert lib.vfm_debug_coarse_plan(0, 384, 2100, 4096, 1, 1, 0, CUS, buf, 8) != 0 and b"buffer" in lib.vfm_last_error()
    assert lib.vfm_debug_coarse_plan(0, 100, 2100, 4096, 1, 1, 0, CUS, buf, len(buf)) != 0
    assert lib.vfm_debug_coarse_plan(0, 384, 300, 1300, 0, 0, 1, CUS, buf, len(buf)) != 0 and b"row bias" in lib.vfm_last_error()
    assert built.coarse_plan(mdc.BEST, 384, mdc.N_HI, mdc.M, compute_units=0)["kernel"] == built.coarse_plan(mdc.BEST, 384, mdc.N_HI, mdc.M,
                                                                                                          compute_units=CUS)["kernel"]
