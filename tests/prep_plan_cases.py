"""The case table of the operand preparation's plan (csrc/match_internal.h: resolve_prepare), shared by tests/test_prepare_plan.py (CPU: the
read-back vfm_debug_prepare_plan), tests/test_gpu_prepare_plan.py (every row through its real entry) and tools/ab_two_libs_prep.py --cases
(bytes against another build).  What a row expects was read off do_prepare2 / do_prepare_perm and the six entries as they stood BEFORE the
plan existed -- the launcher with its decisions inline -- and is written out here, never asked of the resolver."""
from __future__ import annotations

from typing import NamedTuple, Optional

ROWS1, ROWS2 = 300, 130        # (map, scan): three and two 128-row groups, a partly filled last group and tile each
PERSISTENT, INTERLEAVED = 1, 2
MX6, MX6_HALF, NO_I8 = 8, 16, 32
F32, F16 = 0, 1
ENTRIES = {"prepare": 0, "prepare2": 1, "gated": 2, "gated_p": 3, "gated_z": 4, "gated_t": 5, "perm": 6, "oneshot": 7}   # enum vfm_debug_prepare_entry
ONE_OPERAND = ("prepare", "perm")
NO_EXPORT = ("perm", "oneshot")   # inside vfm_match_mutual_l2 / vfm_match_ip_top1: no exported call hands out their prepared buffers


class Case(NamedTuple):
    id: str
    entry: str
    schedule: int
    d: int
    cfg: tuple                     # ((policy key, value), ...) beside the factory settings
    dtypes: tuple                  # (dtype1, dtype2)
    images: Optional[tuple]        # None: refused, and `refusal` is a substring of the message
    kernels: tuple = ()
    grid: str = ""
    zero: str = "none"
    refusal: str = ""


def _chunk(d):
    return "prep_chunk_kernel<false,2>" if d <= 512 else "prep_chunk_kernel<false,3>"


def _wide(d):
    return ("prep_mx6_rows_kernel<16>" if d == 512 else "prep_mx6_rows_kernel<32>", "prep_mx6_group_kernel")


CHUNK_MX6 = "prep_chunk_kernel<false,2,true,8>"
ROWS = "prep_rows_kernel"


def _cases():
    out = []

    def add(entry, schedule, d, images, kernels, grid, zero=None, cfg=(), dtypes=(F32, F32), refusal="", tag=""):
        if zero is None:
            zero = "none"
        name = f"{entry}-s{schedule}-d{d}" + "".join(f"-{k}{v}" for k, v in cfg) + ("-f16rows%d%d" % dtypes if dtypes != (F32, F32) else "") + tag
        out.append(Case(name, entry, schedule, d, tuple(cfg), dtypes, images, tuple(kernels), grid, zero, refusal))

    # the ungated entries: the fp16 image always; both images from one read up to d = 384
    for entry in ("prepare", "prepare2", "oneshot"):
        add(entry, 0, 128, ("f16",), [ROWS], "tile")
        for d in (256, 384):
            add(entry, 0, d, ("f16", "i8"), ["prep_chunk_kernel<true,2>"], "group")
        for d in (512, 640, 768):
            add(entry, 0, d, ("f16", "i8"), [_chunk(d), ROWS], "group")
    # the gated entries without the fp6 flag: the int8 image alone; the schedule's low bits choose the grid
    for d in (256, 384, 512, 640, 768):
        add("gated", 0, d, ("i8",), [_chunk(d)], "group")
        for schedule, grid in ((0, "group"), (PERSISTENT, "cu"), (INTERLEAVED, "group")):
            add("gated_p", schedule, d, ("i8",), [_chunk(d)], grid)
    add("gated", 0, 128, ("f16",), [ROWS], "tile")
    add("gated_p", PERSISTENT, 128, ("f16",), [ROWS], "tile")
    for grid_key, grid in ((0, "cu"), (5, "5"), (-1, "group")):
        add("gated_p", 0, 384, ("i8",), [_chunk(384)], grid, cfg=(("prep_grid", grid_key),))
    # the fp6 image at d = 256 / 384: the form is the policy's
    for d in (256, 384):
        for schedule, width, image in ((MX6, "full", "fp6"), (MX6 | MX6_HALF, "half", "fp6h"), (MX6_HALF, "half", "fp6h")):
            for form, kernel, grid in ((3, f"prep_once_kernel<{d},{width},short>", "group"), (4, f"prep_once_kernel<{d},{width},persist>", "2cu-stream"),
                                       (1, f"prep_stream_kernel<{d},{width}>", "group"), (0, CHUNK_MX6, "group"), (7, CHUNK_MX6, "group")):
                add("gated_p", schedule, d, ("i8", image), [kernel], grid, cfg=(("prep_form", form),))
        add("gated_p", MX6 | PERSISTENT, d, ("i8", "fp6"), [CHUNK_MX6], "cu", cfg=(("prep_form", 0),))
        add("gated_p", MX6, d, ("i8", "fp6"), [f"prep_once_kernel<{d},full,persist>"], "2", cfg=(("prep_form", 4), ("prep_grid", 2)))
        # ... without the int8 image: the one-read forms or nothing
        for entry in ("gated_p", "gated_z"):
            for form, shape, grid in ((3, "short", "group"), (4, "persist", "2cu-stream")):
                add(entry, MX6 | MX6_HALF | NO_I8, d, ("fp6h",), [f"prep_once_kernel<{d},half,{shape},noi8>"], grid,
                    zero="inside" if entry == "gated_z" else None, cfg=(("prep_form", form),))
            for form in (0, 1):
                add(entry, MX6 | MX6_HALF | NO_I8, d, None, [], "", cfg=(("prep_form", form),), refusal="VFM_PREPARE_NO_I8")
    # d = 512 / 768: the fp6 image by kernels of their own; d = 640 has none
    for d in (512, 768):
        for schedule, image in ((MX6, "fp6"), (MX6 | MX6_HALF, "fp6h")):
            add("gated_p", schedule, d, ("i8", image), [_chunk(d), *_wide(d)], "group")
    add("gated_p", MX6, 640, ("i8",), [_chunk(640)], "group")
    # too few queries for the quantised passes: the fp16 image as well
    few = (("i8_min_queries", ROWS2),)
    add("gated_p", MX6, 384, ("f16", "i8", "fp6"), ["prep_once_kernel<384,full,short>", ROWS], "group", cfg=few)
    add("gated", 0, 384, ("f16", "i8"), ["prep_chunk_kernel<true,2>"], "group", cfg=few)
    # fp16 rows: the chunk kernel under every form
    for d in (256, 384):
        for dtypes in ((F16, F16), (F32, F16), (F16, F32)):
            for schedule, image in ((MX6, "fp6"), (MX6 | MX6_HALF, "fp6h")):
                for form in (0, 1, 3, 4):
                    add("gated_t", schedule, d, ("i8", image), [CHUNK_MX6], "group", cfg=(("prep_form", form),), dtypes=dtypes)
    for d in (512, 768):
        add("gated_t", MX6, d, ("i8", "fp6"), [_chunk(d), *_wide(d)], "group", dtypes=(F16, F16))
    add("gated_t", MX6, 384, ("i8", "fp6"), ["prep_once_kernel<384,full,short>"], "group")   # (fp32 rows through the typed entry)
    # the zero ranges: inside the one-read kernels, by prep_zero_kernel behind every other form
    add("gated_z", 0, 384, ("i8",), [_chunk(384)], "group", zero="behind")
    add("gated_z", MX6, 512, ("i8", "fp6"), [_chunk(512), *_wide(512)], "group", zero="behind")
    add("gated_z", PERSISTENT, 128, ("f16",), [ROWS], "tile", zero="behind")
    for form, kernel, grid, zero in ((3, "prep_once_kernel<384,full,short>", "group", "inside"), (4, "prep_once_kernel<384,full,persist>", "2cu-stream", "inside"),
                                     (1, "prep_stream_kernel<384,full>", "group", "behind"), (0, CHUNK_MX6, "group", "behind")):
        add("gated_z", MX6, 384, ("i8", "fp6"), [kernel], grid, zero=zero, cfg=(("prep_form", form),))
    # one operand, the int8 image alone (the Euclidean search)
    for d in (512, 768):
        add("perm", 0, d, ("i8",), [_chunk(d)], "group")
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)


def rows_of(case):
    """(rows1, rows2) a case is resolved and run at"""
    return (ROWS1, 0) if case.entry in ONE_OPERAND else (ROWS1, ROWS2)
