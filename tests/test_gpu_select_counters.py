"""The selection kernels laid out for the sweep (match_select_best_kernel, match_select_top2_kernel) and the general kernel's int8
branches ("coarse_variant" 20) evaluate the same bounds (csrc/match_select.h): they must take the same decision.  The answers
cannot show a difference -- a candidate more or less changes no arg-max -- but the counters the selection leaves do, and the
caller's policy reads them.

Compared are the counters of vfm_debug_match_stats that only the selection writes in these plans (FIN_SELECT* of resolve_search):
[2] candidate entries, [5] the load figure, [8 .. 23] the histogram of entries per query.  (match_filter_refine_kernel, which also
writes [2] and [8 ..], belongs to the fp16 pass; half_guard_kernel, which rewrites [5], runs behind the half-width kinds only.)
Left out: [0], the all-pairs fallbacks -- match_rescan_kernel, match_rescan_close_kernel and match_refine_kernel add theirs to the
same counter, and the two configurations run different rescans (chunk-major by default, query-major under variant 20).

Shapes.  (d 384, n 2113, m 4100): the last query tile has one live row, the last chunk is partly padded, n >= 4 x chunks: the rescan
is chunk-major and match_select_best_kernel takes its per-chunk histogram path; all four kinds.  (d 256, n 300, m 32 900): 258
chunks, n < 4 x chunks: no bins, everything lands in the queries' own lists; BEST and TOP2 only -- 300 queries run the fp6 kinds as
these two (resolve_search), so they would repeat them."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from vfmreg import _lib  # noqa: E402

from . import match_dispatch_cases as mdc  # noqa: E402
from .test_gpu_coarse_dispatch import Gated, _dev  # noqa: E402

BINS, NO_BINS = (384, mdc.N_HI, mdc.M), (256, mdc.N_LO, mdc.M_SEED)
KINDS = {"BEST": mdc.BEST, "TOP2": mdc.TOP2, "MX6": mdc.MX6, "MX6_TOP2": mdc.MX6_TOP2}
CASES = [(k, *BINS) for k in KINDS] + [(k, *NO_BINS) for k in ("BEST", "TOP2")]
SELECTION_ONLY = [2, 5] + list(range(8, 24))


def _search_with_counters(q, b, records, cfg):
    lib = _lib.load()
    with _lib.using(_lib.Config(match_stats=1, **cfg)):
        run = Gated(q, b, records)                       # (the preparation reads the thread's config too)
        idx, sim, _ = run.search(gate=float("-inf"))     # no query is dead or below the gate: every one is resolved
        out = (C.c_int32 * 64)()
        _lib.check(lib.vfm_debug_match_stats(run.ws.data_ptr(), run.n, run.m, C.cast(out, C.c_void_p)))
    return idx, sim, list(out)


@pytest.mark.parametrize("kind,d,n,m", CASES, ids=[f"{k}-d{d}-n{n}-m{m}" for k, d, n, m in CASES])
def test_sweep_kernels_and_general_kernel_leave_the_same_counters(kind, d, n, m):
    q, b, ridx, rsim = mdc.data_ip(d, n, m)
    dq, db = _dev(q), _dev(b)
    idx0, sim0, st0 = _search_with_counters(dq, db, KINDS[kind], {})
    idx1, sim1, st1 = _search_with_counters(dq, db, KINDS[kind], {"coarse_variant": 20})
    for what, idx, sim in (("default", idx0, sim0), ("coarse_variant 20", idx1, sim1)):
        np.testing.assert_array_equal(idx, ridx, err_msg=what)
        np.testing.assert_array_equal(sim, rsim, err_msg=what)
    print({k: (st0[k], st1[k]) for k in SELECTION_ONLY})
    assert st0[2] > 0 and st0[5] > 0 and sum(st0[8:24]) > 0.9 * n          # the counters were kept at all
    assert [st0[k] for k in SELECTION_ONLY] == [st1[k] for k in SELECTION_ONLY]
