"""The persistent form of the one-read fp6 operand preparation ("coarse_variant" 44: prep_once_kernel as a grid of at most two workgroups
per compute unit, each walking several 128-row groups with the next group's first loads requested under a group's second pass), the
search-workspace zeroing that rides along with the preparation (vfm_match_prepare2_gated_z) and the coarse call that is told so
(VFM_RECORDS_WS_CLEAN), and the pipeline that uses both.

What is compared is always bytes: the persistent form against the one-group-per-workgroup form (43), the new entry points against the
old ones, the overlapped pipeline against the serial one."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.guarded import GuardedBuffer  # noqa: E402
from vfmreg import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PREPARE_MX6, PREPARE_MX6_HALF = 8, 16
WS_CLEAN = 0x100   # VFM_RECORDS_WS_CLEAN

SHAPES = [(384, 3000, 9001, PREPARE_MX6), (384, 3000, 9001, PREPARE_MX6 | PREPARE_MX6_HALF), (256, 1234, 5000, PREPARE_MX6),
          (256, 129, 5000, PREPARE_MX6 | PREPARE_MX6_HALF), (384, 1, 127, PREPARE_MX6 | PREPARE_MX6_HALF),
          (384, 257, 131, PREPARE_MX6 | PREPARE_MX6_HALF)]
# workgroups of the persistent form: the default (two per compute unit, clamped to the groups); ONE workgroup that walks every group,
# crosses from the map's groups to the scan's and runs a long steady state; 3 (no divisor of any shape's group count: the last sweep is
# ragged); more workgroups than groups (the loop body runs once per workgroup, nothing is prefetched)
GRIDS = [-1, 1, 3, 10000]

_cache = {}


def _hostile_rows(d, n, m, flags):
    """the rows of tests/test_gpu_mx6.py::test_the_one_read_form_of_the_fp6_preparation: a zero row, a row x 1e18, half a row x 1e-3"""
    g = torch.Generator(device="cuda")
    g.manual_seed(d + n + m + flags)
    q = torch.randn((n, d), generator=g, device="cuda")
    b = torch.randn((m, d), generator=g, device="cuda")
    b[m // 2] = 0.0
    b[m // 4] *= 1e18
    q[0, : d // 2] *= 1e-3
    return q, b


def _prepared_pair(lib, q, b, flags, variant, grid):
    """both prepared buffers, pre-filled with 0xA5, after one preparation under (variant, prep_grid)"""
    n, d = q.shape
    m = b.shape[0]
    qb = torch.full((lib.vfm_match_prepared_bytes(n, d),), 0xA5, dtype=torch.uint8, device="cuda")
    bb = torch.full((lib.vfm_match_prepared_bytes(m, d),), 0xA5, dtype=torch.uint8, device="cuda")
    with _lib.using(_lib.Config(coarse_variant=variant, prep_grid=grid)):
        _lib.check(lib.vfm_match_prepare2_gated_p(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), d, flags,
                                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return qb, bb


def _one_read_form(lib, shape):
    """the inputs of a shape and what variant 43 writes for them: made once, shared by the shape's four grids, never written"""
    if shape not in _cache:
        d, n, m, flags = shape
        q, b = _hostile_rows(d, n, m, flags)
        _cache[shape] = (q, b) + _prepared_pair(lib, q, b, flags, 43, -1)
    return _cache[shape]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("d,n,m,flags", SHAPES)
def test_the_persistent_form_writes_the_bytes_of_the_one_read_form(d, n, m, flags, grid):
    """Variant 44 against variant 43 on the WHOLE of both prepared buffers (pre-filled with 0xA5: what is written and what is left
    alone are both the same), at every grid that changes the path through the kernel's loop.  The shapes reach: a workgroup that runs
    the prologue only (grid 10000), prologue + one prefetched group, a long steady state and the map -> scan boundary inside one
    workgroup (grid 1: 72 + 24 groups at 3000 x 9001), a ragged last sweep (grid 3), a partial last group, and last groups with fewer
    than 8 (n = 1: one row; 257 = 2 groups + 1 row), fewer than 32 (m = 131: 3 rows in its second group) and fewer than 128 valid
    rows (n = 129, m = 127)."""
    lib = _lib.load()
    q, b, want_q, want_b = _one_read_form(lib, (d, n, m, flags))
    got_q, got_b = _prepared_pair(lib, q, b, flags, 44, grid)
    assert torch.equal(got_b, want_b), f"map image differs at byte {int(torch.nonzero(got_b != want_b)[0])}"
    assert torch.equal(got_q, want_q), f"scan image differs at byte {int(torch.nonzero(got_q != want_q)[0])}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the zeroing
# ---------------------------------------------------------------------------------------------------------------------------------
def _zeroed_ranges(n, m):
    """[(offset, bytes)] of what a coarse call fills with zeros in a search workspace, from the layout of carve_search
    (csrc/match_internal.h; every array starts on a 256-byte boundary): partials | cand_cnt | cand | fb_list | fb_count ... qbest | ...
    -- cand_cnt[npad], and one region [fb_count (256 B) | qmax (npad) | rec_cnt (npad) | bin_cnt (chunks padded to 64, x 32) |
    hit_cnt (npad x 32) | qbest (npad x 8 B)]."""
    al = lambda x: (x + 255) // 256 * 256
    npad, mpad = al(n), al(m)
    nch = mpad // 128
    slices = max(1, min(64, nch // 8))
    slices = max(slices, (nch + 254) // 255)
    slots = (npad // 512 + 1) * slices * (2047 + 4)
    off = al(8 * max(nch * npad, (slots + 1) // 2))                 # partials
    cand_cnt = (off, 4 * npad)
    off = al(off + 4 * npad)
    cap = min(max((mpad // 128 + 63) // 64 * 64, 64), 2048)          # cand_cap
    off = al(off + 4 * npad * cap)                                    # cand
    off = al(off + 4 * npad)                                          # fb_list
    zero = 256 + 2 * 4 * npad + (nch + 63) // 64 * 64 * 32 * 4 + npad * 32 * 4 + npad * 8
    return [cand_cnt, (off, zero)]


@pytest.fixture(scope="module")
def zero_case():
    from vfmreg import synth
    n, m, d = 3000, 9001, 384   # (the fused kinds need n > 2048)
    p = synth.make_pair_device(n, m, d, seed=5)
    return n, m, d, p["q_desc"], p["b_desc"]


def _search_through(lib, zero_case, records, flags, new_path):
    """preparation -> coarse -> finish of one pair in a guarded workspace poisoned with 0xFF; new_path: the preparation clears the
    workspace's zeroed region and the coarse call is told so.  Returns idx, sim, the guarded workspace and its bytes right after the
    preparation."""
    n, m, d, q, b = zero_case
    st = torch.cuda.current_stream().cuda_stream
    gate = float(np.nextafter(np.float32(0.8), np.float32(-np.inf)))
    qb = torch.zeros(lib.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device="cuda")
    bb = torch.zeros(lib.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device="cuda")
    ws = GuardedBuffer(lib.vfm_match_search_workspace_bytes(n, m, d), torch.uint8, seed=97).fill_bytes(0xFF)
    idx = torch.empty(n, dtype=torch.int64, device="cuda")
    sim = torch.empty(n, dtype=torch.float32, device="cuda")
    if new_path:
        _lib.check(lib.vfm_match_prepare2_gated_z(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), d, flags, ws.ptr(),
                                                  ws.nbytes, n, m, st))
    else:
        _lib.check(lib.vfm_match_prepare2_gated_p(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), d, flags, st))
    torch.cuda.synchronize()
    after_prepare = ws.body.clone()
    _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.ptr(), ws.nbytes,
                                                   records | (WS_CLEAN if new_path else 0), gate, st))
    _lib.check(lib.vfm_match_search_finish_gated_r(q.data_ptr(), qb.data_ptr(), n, b.data_ptr(), bb.data_ptr(), m, d, idx.data_ptr(),
                                                   sim.data_ptr(), ws.ptr(), ws.nbytes, gate, records, st))
    torch.cuda.synchronize()
    return idx, sim, ws, after_prepare


@pytest.mark.parametrize("variant", [43, 44, 41])
@pytest.mark.parametrize("records,flags", [(8, PREPARE_MX6 | PREPARE_MX6_HALF), (5, PREPARE_MX6), (0, PREPARE_MX6)])
def test_the_preparation_clears_exactly_what_the_coarse_call_would(zero_case, records, flags, variant):
    """vfm_match_prepare2_gated_z -> coarse with VFM_RECORDS_WS_CLEAN -> finish in a workspace poisoned with 0xFF, against the old
    entry points in a workspace poisoned the same way: idx and sim bit-equal (record kinds 8, 5, 0), both guards of the workspace
    intact, and right after the preparation the workspace is 0x00 inside the two ranges the coarse call's fills cover and 0xFF
    everywhere else -- not a byte more.  Variants 43 / 44 clear inside the preparation kernel, 41 (the stream form) by the small kernel
    behind it."""
    lib = _lib.load()
    n, m, d = zero_case[:3]
    with _lib.using(_lib.Config(coarse_variant=variant)):
        want_idx, want_sim, ws_old, old_after = _search_through(lib, zero_case, records, flags, False)
        got_idx, got_sim, ws_new, new_after = _search_through(lib, zero_case, records, flags, True)
    assert bool((old_after == 0xFF).all()), "the plain preparation wrote to the search workspace"
    expect = torch.full_like(new_after, 0xFF)
    for off, nbytes in _zeroed_ranges(n, m):
        assert off + nbytes <= expect.numel()
        expect[off:off + nbytes] = 0
    if not torch.equal(new_after, expect):
        bad = torch.nonzero(new_after != expect)
        pytest.fail(f"workspace after the preparation: {bad.numel()} bytes differ from the two zeroed ranges, first at {int(bad[0])}, "
                    f"last at {int(bad[-1])} (ranges {_zeroed_ranges(n, m)})")
    for ws in (ws_old, ws_new):
        chk = ws.intact()
        assert chk, repr(chk)
    assert torch.equal(got_idx, want_idx)
    assert torch.equal(got_sim.view(torch.int32), want_sim.view(torch.int32))
    assert int((want_idx >= 0).sum()) > n // 4   # (the pair has matches: the comparison is not one of empty answers)


# ---------------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------------------------------------------
KEYS = ("T", "count", "idx", "sim")


@pytest.fixture(scope="module")
def two_pairs():
    from vfmreg import synth
    return [synth.make_pair_device(3000, 9001, 384, seed=11 + p) for p in range(2)]


def _run_pipeline(pipe, pairs, ready, settle):
    out = []
    for i in range(12):
        p = pairs[i % 2]
        o = pipe.register(p["q_desc"], p["q_xyz"], p["b_desc"], p["b_xyz"], inputs_ready=ready)
        with torch.cuda.stream(o["result_stream"]):
            out.append({k: o[k].clone() for k in KEYS})
        if settle:
            pipe.synchronize()
            torch.cuda.synchronize()
    pipe.synchronize()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("coarse", ["mx6-half", "auto"])
def test_the_overlapped_pipeline_with_a_precleared_workspace_gives_the_serial_answers(two_pairs, coarse):
    """12 registrations alternating two pairs through the bench's pipeline form (preparation on its own stream -- where it now clears the
    buffer set's search workspace --, coarse pass on the caller's, two solve streams, three buffer sets: every set and its workspace is
    reused four times, the preparation of pair i + 1 running beside the stages of pair i), against the same registrations through a
    serial pipeline that still lets the coarse call fill for itself: T, count, idx and sim bit-equal.  "mx6-half" runs back to back.
    "auto" starts cold, so its first registration runs the half-width probe in the set's workspace and must NOT take the flag; here
    both pipelines are synchronised after every registration, so that the policy reads the same feedback at the same step in both
    (its modes resolve different sets of queries that miss the gate; which mode a step runs in must not depend on timing)."""
    from vfmreg.pipeline import RegistrationPipeline
    settle = coarse == "auto"
    serial = RegistrationPipeline(3000, 9001, 384, n_iter=2000, coarse=coarse)
    serial._ws_clean = False
    want = _run_pipeline(serial, two_pairs, None, settle)
    torch.cuda.synchronize()
    ready = torch.cuda.Event()
    ready.record()
    over = RegistrationPipeline(3000, 9001, 384, n_iter=2000, overlap_ransac=True, overlap_prepare=True, solve_streams=2, coarse=coarse)
    assert over._ws_clean
    got = _run_pipeline(over, two_pairs, ready, settle)
    for i, (w, g) in enumerate(zip(want, got)):
        for k in KEYS:
            assert torch.equal(w[k].view(torch.uint8), g[k].view(torch.uint8)), (k, i)
    assert all(int(w["count"]) > 500 for w in want)
