"""VFM_RECORDS_MX6_HALF_FUSED without the int8 image: the preparation that leaves it out (VFM_PREPARE_NO_I8), the chunk-major rescan
on the fp6 half image (match_rescan_chunk_mx6h_kernel) and the finish path behind it (VFM_RECORDS_NO_I8), the pipeline that uses them.

Every answer is compared with oracle.match_ip_top1 plus the gate, exactly (the decision is fp64 on both sides), and with the search
that keeps the int8 image, bit for bit.  Shapes are the smallest at which these paths run: more than 2048 queries and at least four
queries per map chunk."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402
from vfmreg import _lib, synth  # noqa: E402

from .prepared_layout import _al, prepared_layout  # noqa: E402
from .test_gpu_int8 import _gate_contract  # noqa: E402

pytestmark = pytest.mark.gpu

PREPARE_HALF = 8 | 16      # VFM_PREPARE_MX6 | VFM_PREPARE_MX6_HALF
PREPARE_NO_I8 = 32
KIND = 8                   # VFM_RECORDS_MX6_HALF_FUSED
NO_I8 = 0x200              # VFM_RECORDS_NO_I8
GATE = float(np.nextafter(np.float32(0.8), np.float32(-np.inf)))
N = 2100
SHAPES = [(d, N, m) for d in (256, 384) for m in (1000, 4096)]   # m = 1000: a padded last chunk


KEPT = ("inv", "tiles6", "err6h", "gerr6h", "err6", "gerr6", "gstep6", "rest", "grest")
INT8_ONLY = ("err", "gstep", "gerr", "tiles8", "tiles8h", "rows8")


def workspace_layout(n, m):
    """{array: (offset, bytes)} of a search workspace -- carve_search (csrc/match_internal.h) -- and its bin capacity"""
    npad, mpad = _al(n), _al(m)
    nch = mpad // 128
    slices = max(1, min(64, nch // 8))
    slices = max(slices, (nch + 254) // 255)
    slots = (npad // 512 + 1) * slices * (2047 + 4)
    cap = min(max((nch + 63) // 64 * 64, 64), 2048)
    bin_cap = min(max((128 * npad // nch + 63) // 64 * 64, 1024), 65536)
    sizes = [("partials", 8 * max(nch * npad, (slots + 1) // 2)), ("cand_cnt", 4 * npad), ("cand", 4 * npad * cap), ("fb_list", 4 * npad),
             ("fb_count", 4 * 64), ("qmax", 4 * npad), ("rec_cnt", 4 * npad), ("bin_cnt", (nch + 63) // 64 * 64 * 32 * 4),
             ("hit_cnt", 4 * npad * 32), ("qbest", 8 * npad), ("bins", 4 * nch * bin_cap), ("rec", 8 * npad * 1024), ("cand_up", 4 * npad * cap)]
    out, off = {}, 0
    for name, nbytes in sizes:
        off = _al(off)
        out[name] = (off, nbytes)
        off += nbytes
    out["_end"] = (_al(off), 0)
    return out, cap, bin_cap


def _view(buf, layout, name, dtype):
    off, nbytes = layout[name]
    return buf[off:off + nbytes].view(dtype)


def _fill(nbytes, pattern):
    if pattern == "counter":
        return (torch.arange(nbytes, device="cuda", dtype=torch.int64) % 251).to(torch.uint8)
    return torch.full((nbytes,), int(pattern), dtype=torch.uint8, device="cuda")


def _search(q, b, no_i8, pattern=0xA5, guarded=False):
    """preparation (-> both prepared buffers pre-filled with `pattern`) -> coarse -> finish of one pair.  Returns idx, sim, the prepared
    buffers and the workspace (GuardedBuffers when asked for)."""
    lib = _lib.load()
    n, d = q.shape
    m = b.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    nq, nb, nw = lib.vfm_match_prepared_bytes(n, d), lib.vfm_match_prepared_bytes(m, d), lib.vfm_match_search_workspace_bytes(n, m, d)
    if guarded:
        qg, bg, wg = (GuardedBuffer(x, torch.uint8, seed=s) for x, s in ((nq, 3), (nb, 5), (nw, 7)))
        qg.body.copy_(_fill(nq, pattern))
        bg.body.copy_(_fill(nb, pattern))
        wg.fill_bytes(0xFF)
        qb, bb, ws = qg.body, bg.body, wg.body
    else:
        qb, bb = _fill(nq, pattern), _fill(nb, pattern)
        ws = torch.full((nw,), 0xFF, dtype=torch.uint8, device="cuda")
    flags = PREPARE_HALF | (PREPARE_NO_I8 if no_i8 else 0)
    records = KIND | (NO_I8 if no_i8 else 0)
    idx = torch.empty(n, dtype=torch.int64, device="cuda")
    sim = torch.empty(n, dtype=torch.float32, device="cuda")
    _lib.check(lib.vfm_match_prepare2_gated_p(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), d, flags, st))
    _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), nw, records, GATE, st))
    _lib.check(lib.vfm_match_search_finish_gated_r(q.data_ptr(), qb.data_ptr(), n, b.data_ptr(), bb.data_ptr(), m, d, idx.data_ptr(),
                                                   sim.data_ptr(), ws.data_ptr(), nw, GATE, records, st))
    torch.cuda.synchronize()
    if guarded:
        return idx, sim, qg, bg, wg
    return idx, sim, qb, bb, ws


def _oracle(q, b):
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    return orc.match_ip_top1(qn, bn)


_pairs = {}


def _d2_pair(d, n, m):
    """a D.2 pair of a shape with its oracle answers: made once, shared, never written"""
    if (d, n, m) not in _pairs:
        p = synth.make_pair(n, m, d, seed=7 + d + m)
        q, b = p["q_desc"], p["b_desc"]
        _pairs[(d, n, m)] = (q, b, torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda()) + tuple(_oracle(q, b))
    return _pairs[(d, n, m)]


def _bins(ws, n, m):
    """the survivor bins of a finished search: per chunk the sorted queries (a bin's order is that of its atomics)"""
    lay, cap, bin_cap = workspace_layout(n, m)
    assert lay["_end"][0] == ws.numel()
    cnt = _view(ws, lay, "bin_cnt", torch.int32).cpu().numpy()[::32]
    bins = _view(ws, lay, "bins", torch.int32).cpu().numpy().reshape(-1, bin_cap)
    return [np.sort(bins[c, :min(int(cnt[c]), bin_cap)]) for c in range(bins.shape[0])], cnt[:bins.shape[0]]


def _fb_count(ws, n, m):
    lay, _, _ = workspace_layout(n, m)
    return _view(ws, lay, "fb_count", torch.int32).cpu().numpy()


@pytest.mark.parametrize("d,n,m", SHAPES)
def test_the_flagged_preparation_keeps_every_other_byte(d, n, m):
    """VFM_PREPARE_NO_I8 against flags 24 in buffers pre-filled alike: inv, the fp6 half image (whole tiles: what neither form writes
    is the fill), err6h / gerr6h, err6 / gerr6, gstep6, rest / grest byte-equal; the int8 regions still hold the fill."""
    lib = _lib.load()
    _, _, q, b, _, _ = _d2_pair(d, n, m)
    st = torch.cuda.current_stream().cuda_stream
    bufs = {}
    for flags in (PREPARE_HALF, PREPARE_HALF | PREPARE_NO_I8):
        qb, bb = _fill(lib.vfm_match_prepared_bytes(n, d), 0xA5), _fill(lib.vfm_match_prepared_bytes(m, d), 0xA5)
        _lib.check(lib.vfm_match_prepare2_gated_p(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), d, flags, st))
        torch.cuda.synchronize()
        bufs[flags] = (qb, bb)
    for which, rows in ((0, n), (1, m)):
        lay = prepared_layout(rows, d)
        want, got = bufs[PREPARE_HALF][which], bufs[PREPARE_HALF | PREPARE_NO_I8][which]
        assert lay["_end"][0] == want.numel()
        for name in KEPT:
            assert torch.equal(_view(got, lay, name, torch.uint8), _view(want, lay, name, torch.uint8)), (name, which)
        for name in INT8_ONLY:
            if name in lay:
                assert bool((_view(got, lay, name, torch.uint8) == 0xA5).all()), (name, which)
        assert bool((_view(want, lay, "tiles8", torch.uint8) != 0xA5).any())   # (the other form does write it)


@pytest.mark.parametrize("d,n,m", SHAPES)
def test_search_with_and_without_the_int8_image(d, n, m):
    """D.2 pairs: idx / sim of both forms equal to the oracle under the gate contract and bit-equal to each other; the same survivor
    bins; the guard down."""
    _, _, q, b, ridx, rsim = _d2_pair(d, n, m)
    off_idx, off_sim, _, _, off_ws = _search(q, b, False)
    on_idx, on_sim, _, _, on_ws = _search(q, b, True)
    for idx, sim in ((off_idx, off_sim), (on_idx, on_sim)):
        solved = _gate_contract(idx, sim, ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all()
    assert int((on_idx >= 0).sum()) > n // 4
    assert torch.equal(on_idx, off_idx)
    assert torch.equal(on_sim.view(torch.int32), off_sim.view(torch.int32))
    (off_bins, off_cnt), (on_bins, on_cnt) = _bins(off_ws, n, m), _bins(on_ws, n, m)
    np.testing.assert_array_equal(on_cnt, off_cnt)
    assert int(on_cnt.sum()) > 0
    for c, (x, y) in enumerate(zip(on_bins, off_bins)):
        np.testing.assert_array_equal(x, y, err_msg=f"chunk {c}")
    assert _fb_count(on_ws, n, m)[7] == 0 and _fb_count(off_ws, n, m)[7] == 0


@pytest.mark.parametrize("d,n,m", SHAPES)
def test_nothing_reads_the_unwritten_int8_bytes(d, n, m):
    """both prepared buffers filled with 0xFF, then with a counter, before the flagged preparation: the oracle's answers both times"""
    _, _, q, b, ridx, rsim = _d2_pair(d, n, m)
    first = None
    for pattern in (0xFF, "counter"):
        idx, sim, _, _, _ = _search(q, b, True, pattern=pattern)
        solved = _gate_contract(idx, sim, ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all()
        if first is None:
            first = (idx, sim)
        else:
            assert torch.equal(idx, first[0]) and torch.equal(sim.view(torch.int32), first[1].view(torch.int32))


def test_duplicated_map_rows_tie_to_the_lowest_index():
    """the same row twice inside one chunk (5, 77) and in two chunks (10, 300; 200, 3000): every query of such a row gets the lower index"""
    d, n, m = 384, N, 4096
    q0, b0 = _d2_pair(d, n, m)[:2]
    q, b = q0.copy(), b0.copy()
    rng = np.random.default_rng(3)
    for lo, hi in ((5, 77), (10, 300), (200, 3000)):
        b[hi] = b[lo]
    for k, row in enumerate((5, 77, 10, 300, 200, 3000)):
        q[3 * k] = b[row]
        q[3 * k + 1] = b[row] + 0.01 * rng.standard_normal(d).astype(np.float32)
        q[3 * k + 2] = 2.5 * b[row]
    ridx, rsim = _oracle(q, b)
    assert set(ridx[:18].tolist()) == {5, 10, 200}
    for no_i8 in (False, True):
        idx, sim, _, _, _ = _search(torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda(), no_i8)
        solved = _gate_contract(idx, sim, ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all() and solved[:18].all()


def test_zero_rows_and_a_best_row_in_the_partly_filled_last_chunk():
    d, n, m = 384, N, 1000   # rows 896 .. 999 of the last chunk exist, 1000 .. 1023 are padding
    q0, b0 = _d2_pair(d, n, m)[:2]
    q, b = q0.copy(), b0.copy()
    rng = np.random.default_rng(4)
    q[7] = 0.0
    b[130] = 0.0
    q[8] = b0[130]                  # its row is gone: whatever the oracle says now
    for k, row in enumerate((999, 896, 960)):
        q[20 + k] = b[row] + 0.01 * rng.standard_normal(d).astype(np.float32)
    ridx, rsim = _oracle(q, b)
    assert ridx[20:23].tolist() == [999, 896, 960] and ridx[7] == 0 and rsim[7] == 0.0
    for no_i8 in (False, True):
        idx, sim, _, _, _ = _search(torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda(), no_i8)
        solved = _gate_contract(idx, sim, ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all() and solved[20:23].all()
        assert int(idx[7]) == 0 and float(sim[7]) == 0.0


def test_a_full_bin_leaves_whole_chunk_entries_that_the_fp64_decision_scores():
    """n = 2100, m = 34 000 (266 chunks; bin capacity rescan_bin_cap(2304, 266) = 1152): 1300 queries matched to rows of ONE chunk
    overflow its bin, the rest of them stay in their own lists as whole-chunk entries; the answers are the oracle's."""
    d, n, m, chunk = 384, N, 34000, 77
    rng = np.random.default_rng(5)
    b = rng.standard_normal((m, d)).astype(np.float32)
    q = rng.standard_normal((n, d)).astype(np.float32)
    crowd = 1300
    rows = chunk * 128 + rng.integers(0, 128, crowd)
    q[:crowd] = b[rows] + 0.02 * rng.standard_normal((crowd, d)).astype(np.float32)
    other = rng.integers(0, m, 300)
    q[crowd:crowd + 300] = b[other] + 0.02 * rng.standard_normal((300, d)).astype(np.float32)
    ridx, rsim = _oracle(q, b)
    lay, cap, bin_cap = workspace_layout(n, m)
    assert bin_cap == 1152 and crowd >= 1100 and crowd > bin_cap
    idx, sim, _, _, ws = _search(torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda(), True)
    solved = _gate_contract(idx, sim, ridx, rsim, GATE)
    assert solved[rsim >= 0.8].all() and solved[:crowd + 300].all()
    bin_cnt = _view(ws, lay, "bin_cnt", torch.int32).cpu().numpy()[::32]
    assert bin_cnt[chunk] >= crowd
    cand_cnt = _view(ws, lay, "cand_cnt", torch.int32).cpu().numpy()[:n]
    cand = _view(ws, lay, "cand", torch.int32).cpu().numpy().reshape(-1, cap)[:n]
    whole = [(qi, e) for qi in range(crowd) for e in cand[qi, :max(cand_cnt[qi], 0)] if e & 128]
    assert len(whole) >= bin_cnt[chunk] - bin_cap > 0
    assert all((e >> 8) == chunk for _, e in whole)
    assert _fb_count(ws, n, m)[7] == 0


def test_a_duplicate_rich_chunk_overflows_the_hit_staging_of_the_fp6_rescan():
    """d = 256, n = 2304, m = 4096 (32 chunks, n >= 4 x 32: kind 8 is kept).  All 128 rows of chunk 3 are near-copies of one row with 48
    queries aimed at it: 32 queries x 128 rows = 4096 hits in one block of match_rescan_chunk_mx6h_kernel against 1024 staged -- hits
    are appended on the spot and the staging buffer is flushed inside the loop.  k rows of chunk 7 are near-copies of another row with
    40 queries aimed at it (1600 hits; k + the rest of such a query's list stays under the list's capacity, so these are decided from
    their lists).  Answers: the fp64 all-pairs oracle's wherever its similarity reaches 0.8, the gate contract elsewhere, and bit-equal
    to the same search with the int8 image."""
    d, n, m = 256, 2304, 4096
    lay, cap, _ = workspace_layout(n, m)
    k = min(40, cap - 16)
    assert n >= 4 * (m // 128) and k == 40
    rng = np.random.default_rng(8)
    b = rng.standard_normal((m, d)).astype(np.float32)
    q = rng.standard_normal((n, d)).astype(np.float32)           # the odd queries stay unrelated
    pick = rng.integers(8 * 128, m, n // 2)                      # the planted half, on rows outside the two crowded chunks
    q[::2] = b[pick] + 0.25 * rng.standard_normal((n // 2, d)).astype(np.float32)
    r0, r1 = rng.standard_normal((2, d)).astype(np.float32)
    b[3 * 128:4 * 128] = r0 + 1e-3 * rng.standard_normal((128, d)).astype(np.float32)
    b[7 * 128:7 * 128 + k] = r1 + 1e-3 * rng.standard_normal((k, d)).astype(np.float32)
    group3, group7 = np.arange(1, 97, 2), np.arange(101, 181, 2)
    q[group3] = r0 + 0.05 * rng.standard_normal((48, d)).astype(np.float32)
    q[group7] = r1 + 0.05 * rng.standard_normal((40, d)).astype(np.float32)
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    ridx, rsim = orc.match_ip_top1_bruteforce(qn, bn)            # fp64 over all pairs, ties to the lowest index
    assert (ridx[group3] // 128 == 3).all() and (ridx[group7] // 128 == 7).all() and (rsim[group7] > 0.99).all()
    qd, bd = torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda()
    idx, sim, _, _, ws = _search(qd, bd, True)
    solved = _gate_contract(idx, sim, ridx, rsim, GATE)
    assert solved[rsim >= 0.8].all() and solved[group3].all() and solved[group7].all()
    ref_idx, ref_sim, _, _, _ = _search(qd, bd, False)
    assert torch.equal(idx, ref_idx) and torch.equal(sim.view(torch.int32), ref_sim.view(torch.int32))
    fb = _fb_count(ws, n, m)
    assert fb[7] == 0, "the guard is up"
    fb_list = _view(ws, lay, "fb_list", torch.int32).cpu().numpy()[:fb[0]]
    assert not np.isin(group7, fb_list).any()
    # every row of chunk 3 is a hit for each of its 48 queries: 6144 hits in the bin's two blocks, at least 3072 in one of them
    hit_cnt = _view(ws, lay, "hit_cnt", torch.int32).cpu().numpy()[::32]
    assert (hit_cnt[group3] >= 128).all() and (hit_cnt[group7] >= k).all()


def test_descriptors_that_are_all_alike_raise_the_guard_and_the_exact_kernel_decides_every_query():
    d, n, m = 384, N, 1024
    rng = np.random.default_rng(6)
    base = rng.standard_normal(d).astype(np.float32)
    b = (base + 0.05 * rng.standard_normal((m, d))).astype(np.float32)
    q = (base + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    q[11] = 0.0
    ridx, rsim = _oracle(q, b)
    idx, sim, _, _, ws = _search(torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda(), True)
    fb = _fb_count(ws, n, m)
    assert fb[7] == 1, "the guard is down"
    assert fb[0] == n - 1, "queries handed to the all-pairs kernel"
    lay, _, _ = workspace_layout(n, m)
    cand_cnt = _view(ws, lay, "cand_cnt", torch.int32).cpu().numpy()[:n]
    assert (np.delete(cand_cnt, 11) == -1).all()
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(sim.cpu().numpy(), rsim)


@pytest.mark.parametrize("d,n,m", [(256, N, 1000), (384, N, 4096)])
def test_the_new_kernels_stay_inside_the_callers_buffers(d, n, m):
    """flagged preparation, coarse pass and the finish path in guarded buffers: every guard of qprep / bprep / ws intact"""
    _, _, q, b, ridx, rsim = _d2_pair(d, n, m)
    idx, sim, qg, bg, wg = _search(q, b, True, guarded=True)
    for buf in (qg, bg, wg):
        chk = buf.intact()
        assert chk, repr(chk)
    _gate_contract(idx, sim, ridx, rsim, GATE)


def test_the_pipeline_drops_the_int8_image_once_it_runs_kind_8():
    """RegistrationPipeline(coarse="auto"), eight registrations, policy key half_noi8 at 1 and at 0: every returned array equal; the
    preparation's flags include VFM_PREPARE_NO_I8 from the first kind-8 registration on and never before (nor with the key at 0)."""
    from vfmreg.pipeline import RegistrationPipeline
    n, m, d = N, 4096, 384
    p = synth.make_pair_device(n, m, d, seed=21)
    keys = ("T", "fitness", "rmse", "best_hyp", "mask", "idx", "sim", "keep", "count", "corres")
    runs = {}
    for key in (1, 0):
        pipe = RegistrationPipeline(n, m, d, n_iter=2000, overlap_ransac=True, overlap_prepare=True, solve_streams=2, coarse="auto",
                                    config=_lib.Config(half_noi8=key))
        outs, trace = [], []
        for _ in range(8):
            o = pipe.register(p["q_desc"], p["q_xyz"], p["b_desc"], p["b_xyz"])
            trace.append((pipe.last_records, pipe.last_prep_schedule))
            pipe.synchronize()
            torch.cuda.synchronize()   # (the policy reads the same feedback at the same step in both runs)
            outs.append({k: o[k].clone() for k in keys})
        runs[key] = (outs, trace)
    for records, schedule in runs[0][1]:
        assert not (schedule & PREPARE_NO_I8) and not (records & NO_I8)
    kinds = [r & 0xFF for r, _ in runs[1][1]]
    assert KIND in kinds and kinds[0] != KIND      # (the first registration probes)
    assert kinds == [r & 0xFF for r, _ in runs[0][1]]
    for records, schedule in runs[1][1]:
        assert bool(schedule & PREPARE_NO_I8) == ((records & 0xFF) == KIND) == bool(records & NO_I8)
    for i, (w, g) in enumerate(zip(runs[0][0], runs[1][0])):
        c = int(w["count"])
        for k in keys:
            # (the per-correspondence arrays end at `count`: the rows behind it are whatever the buffer set held before)
            x, y = (w[k][:c], g[k][:c]) if k in ("mask", "keep", "corres") else (w[k], g[k])
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (k, i)
    assert int(runs[1][0][-1]["count"]) > 500
