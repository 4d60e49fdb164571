"""CPU checks of the search plan (csrc/match_internal.h: resolve_search; read back through vfm_debug_search_plan): what a search does is
resolved once, for the coarse and the finish stage alike, and the read-back reports it without touching a device.  The cases are the
dispatch table's (tests/match_dispatch_cases.py) and the refusals of tests/test_half_noi8_refusals.py."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

from . import match_dispatch_cases as mdc
from .test_half_noi8_refusals import BIG, REFUSED

ROOT = Path(__file__).resolve().parent.parent
NO_I8 = 0x200
F16, MX6_PILOT = 2, 9
CHUNK_MAJOR = {"match_rescan_chunk_kernel", "match_rescan_chunk_mx6h_kernel"}
PLAN_CASES = [c for c in mdc.CASES + mdc.PADDING_CASES if c.entry in ("gated", "ip")]


@pytest.fixture(scope="module")
def built():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib


def family(kernel: str):
    """(pass, effective record kind) of the coarse-kernel family a case names"""
    if kernel.startswith("pipe<") and "sparse" in kernel:
        return "f16-sparse", F16
    if kernel.startswith(("pipe<", "v<", "r<")):
        return "f16-dense", F16
    args = dict(kv.split("=") for kv in re.findall(r"\w+=\w+", kernel))
    if kernel.startswith(("i8<", "i8q2<")):
        if args.get("fused") == "1":
            return "int8", mdc.HALF_FUSED
        return "int8", mdc.TOP2 if args["top2"] == "1" else (mdc.HALF if args["low"] == "0" else mdc.BEST)
    ks, kind = re.match(r"mx6q2<(\d+),(\w+),", kernel).groups()
    half = 2 * int(ks) == int(args["img"])      # the pass multiplies half of the image's k-steps
    return "fp6", {("BEST", False): mdc.MX6, ("TOP2", False): mdc.MX6_TOP2, ("BEST", True): mdc.MX6_HALF,
                   ("FUSE", True): mdc.MX6_HALF_FUSED, ("FUSE", False): mdc.MX6_FUSED}[kind, half]


def plan_of(lib, case, records=None):
    with lib.using(lib.Config(**dict(case.cfg))):
        return lib.search_plan(case.records if records is None else records, case.d, case.n, case.m, case.gated)


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c.id for c in PLAN_CASES])
def test_pass_and_kind_agree_with_the_kernel_family_the_case_names(built, case):
    plan = plan_of(built, case)
    assert (plan["pass"], plan["kind"]) == family(case.kernel), (plan, case.kernel)
    fused = plan["kind"] in (mdc.HALF_FUSED, mdc.MX6_HALF_FUSED, mdc.MX6_FUSED)
    assert plan["fused"] == fused
    if fused:   # a fused kind's survivors are in the bins already: a finish stage that does not rescan them loses every match
        assert plan["bins"] and CHUNK_MAJOR & set(plan["finish"]), plan
    assert plan["finish"][-2:] == ["match_rescore_kernel", "match_exact_kernel"]
    assert plan["bins"] == bool(CHUNK_MAJOR & set(plan["finish"]))


def test_the_padding_cases_stay_fused_between_the_two_chunk_counts(built):
    assert len(mdc.PADDING_CASES) == 3
    for case in mdc.PADDING_CASES:
        plan = plan_of(built, case)
        assert plan["fused"] and plan["bins"] and CHUNK_MAJOR & set(plan["finish"]), (case.id, plan)


@pytest.mark.parametrize("case", [c for c in PLAN_CASES if c.kernel.startswith("i8<") and "top2=0,low=1" in c.kernel and c.n <= 2048],
                         ids=lambda c: c.id)
def test_the_fp6_kinds_fall_back_to_best_score_int8_records_at_2048_queries(built, case):
    for records in (mdc.MX6, MX6_PILOT, mdc.MX6_FUSED, mdc.MX6_HALF, mdc.MX6_HALF_FUSED):
        plan = plan_of(built, case, records)
        assert (plan["pass"], plan["kind"]) == ("int8", mdc.BEST), (records, plan)
    assert plan_of(built, case, mdc.MX6_TOP2)["kind"] == mdc.TOP2


@pytest.mark.parametrize("d", [256, 384])
def test_a_plan_without_the_int8_image_lists_no_kernel_that_reads_it(built, d):
    plan = built.search_plan(mdc.MX6_HALF_FUSED | NO_I8, d, mdc.N_HI, mdc.M)
    assert plan["no_i8"] and plan["kind"] == mdc.MX6_HALF_FUSED and plan["pass"] == "fp6"
    assert not {"match_rescan_kernel", "match_gatepass_kernel", "match_refine_kernel", "match_rescan_chunk_kernel"} & set(plan["finish"])
    assert plan["finish"] == ["match_bin_survivors_kernel", "half_guard_kernel", "match_guard_fallback_kernel", "match_rescan_chunk_mx6h_kernel",
                              "match_rescan_close_kernel", "match_rescore_kernel", "match_exact_kernel"]
    with_i8 = built.search_plan(mdc.MX6_HALF_FUSED, d, mdc.N_HI, mdc.M)
    assert not with_i8["no_i8"] and "match_rescan_chunk_kernel" in with_i8["finish"] and "match_gatepass_kernel" in with_i8["finish"]


@pytest.mark.parametrize("records,n,m,d", REFUSED)
def test_the_read_back_refuses_what_the_search_refuses_with_the_same_message(built, records, n, m, d):
    import ctypes as C
    lib = built.load()
    buf = C.create_string_buffer(1024)
    assert lib.vfm_debug_search_plan(records, d, n, m, 1, buf, len(buf)) != 0
    message = lib.vfm_last_error()
    assert b"VFM_RECORDS_NO_I8" in message
    assert lib.vfm_match_search_coarse_gated_g(1, n, 1, m, d, 1, BIG, records, 0.8, None) != 0
    assert lib.vfm_last_error() == message
    assert lib.vfm_match_search_finish_gated_r(1, 1, n, 1, 1, m, d, 1, 1, 1, BIG, 0.8, records, None) != 0
    assert lib.vfm_last_error() == message
    with pytest.raises(RuntimeError, match="VFM_RECORDS_NO_I8"):
        built.search_plan(records, d, n, m)


def test_the_read_back_checks_its_arguments(built):
    import ctypes as C
    lib = built.load()
    buf = C.create_string_buffer(1024)
    assert lib.vfm_debug_search_plan(11, 384, 2100, 4096, 1, buf, len(buf)) != 0 and b"unknown record kind" in lib.vfm_last_error()
    assert lib.vfm_debug_search_plan(0, 384, 2100, 4096, 1, buf, 8) != 0 and b"buffer" in lib.vfm_last_error()
    assert lib.vfm_debug_search_plan(0, 100, 2100, 4096, 1, buf, len(buf)) != 0


def test_coarse_variant_5_sends_a_gated_search_to_the_sparse_fp16_pass(built):
    assert built.search_plan(mdc.BEST, 384, mdc.N_SPARSE, mdc.M)["pass"] == "int8"
    with built.using(built.Config(coarse_variant=5)):
        plan = built.search_plan(mdc.BEST, 384, mdc.N_SPARSE, mdc.M)
    assert plan["pass"] == "f16-sparse" and plan["kind"] == F16 and plan["finish"][0] == "match_filter_refine_kernel"
    assert built.search_plan(mdc.BEST, 384, mdc.N_SPARSE, mdc.M)["pass"] == "int8"      # the binding ended with the block
