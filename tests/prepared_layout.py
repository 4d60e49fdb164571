"""Where a prepared operand keeps its regions: carve_prepared (csrc/match_internal.h) in Python, for the tests and tools that look at
single regions of the buffer."""
from __future__ import annotations


def _al(x, a=256):
    return (x + a - 1) // a * a


def prepared_layout(rows, d):
    """{region: (offset, bytes)} of a prepared operand of any width the FAST search takes; "_end": the buffer's size"""
    rp = _al(rows)
    sizes = [("inv", 4 * rp), ("tiles", rp // 32 * (d // 16) * 64 * 16)]
    if d in (256, 384, 512, 640, 768):       # the int8 image
        sizes += [("err", 4 * rp), ("gstep", 4 * rp // 128), ("gerr", 4 * rp // 128), ("tiles8", rp // 32 * (d // 32) * 64 * 16),
                  ("tiles8h", rp // 32 * (d // 64) * 64 * 16), ("rest", 4 * rp), ("grest", 4 * rp // 128)]
        if d != 640:                         # the fp6 image
            ks = d // 64
            tile6 = 512 + ks * 1536 + (512 if ks > 8 else 0)
            sizes += [("tiles6", rp // 32 * tile6), ("err6", 4 * rp), ("gerr6", 4 * rp // 128), ("gstep6", 4 * rp // 128), ("err6h", 4 * rp),
                      ("gerr6h", 4 * rp // 128)]
        if rp <= 131072:
            sizes.append(("rows8", rp * d))
    out, off = {}, 0
    for name, nbytes in sizes:
        off = _al(off)
        out[name] = (off, nbytes)
        off += nbytes
    out["_end"] = (_al(off), 0)
    return out
