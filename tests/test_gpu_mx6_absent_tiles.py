"""Query tiles past the end of the scan in the fp6 coarse kernel (csrc/match_coarse_mx6.hip, run_sets): a wave multiplies, folds and
emits its PRESENT 32-query sets only; `vfm_config` "mx6_tune" bit 2 multiplies the absent ones as copies of tile 0 again, the way the
kernel did before.  Scan sizes put every count of present sets into the last query block of the three-set kernel (d = 384, record
kind 8: 24 tiles per workgroup): tiles mod 24 = 0, 1 (whole and partly filled tile), 2, 3, 23.

Per case, with the bit off and on: the gate contract of tests/test_gpu_mx6.py against the oracle (resolved queries have the oracle's
index and similarity bit for bit, unresolved ones lie below the gate there, every match at the gate is resolved -- the best-score and
top-2 kinds run WITHOUT a gate, where that is "idx and sim equal the oracle's on every row"); equal idx and sim between the two runs;
the guard flag down (the half-width pass decided, not the fallback); and the survivor lists of the fused kinds -- read from the
workgroups' slots between the coarse and the finish call -- the same (query, chunk) pairs, all of them of existing queries: a kernel
that dropped a live set would otherwise pass through the fallback."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from vfmreg import _lib, synth  # noqa: E402
from vfmreg.pipeline import RegistrationPipeline  # noqa: E402

from .test_gpu_int8 import _gate_contract  # noqa: E402
from .test_gpu_mx6 import (PREPARE_MX6, RECORDS_MX6, RECORDS_MX6_FUSED, RECORDS_MX6_HALF_FUSED, RECORDS_MX6_TOP2)  # noqa: E402

D = 384
N_MAX = 3040            # 95 tiles
M_FULL = 8192           # 64 whole chunks
M_PADDED = 8192 - 77    # the last chunk is partly padding
GATE = float(np.nextafter(np.float32(0.8), np.float32(-np.inf)))
ABSENT_MULTIPLIED = 4   # "mx6_tune" bit 2
SLOT_WORDS = 2047 + 4   # a workgroup's survivor slot: header + entries (csrc/match_internal.h, MX6_SURV_SLOT_WORDS)
GRID_SLOT, GUARD_FLAG = 32, 7   # the search's counters (vfm_debug_match_stats): survivor slots written / the half-width guard
# scan size -> tiles mod 24
SIZES = {2304: 0, 2305: 1, 2320: 1, 2368: 2, 2400: 3, 3040: 23}


@functools.lru_cache(maxsize=None)
def _data(m):
    """One D.2-style pair for every case: the scans are prefixes of its queries, the map its first m rows; the oracle's answer once."""
    p = synth.make_pair(N_MAX, M_FULL, D, seed=17)
    q, b = p["q_desc"], np.ascontiguousarray(p["b_desc"][:m])
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    ridx, rsim = orc.match_ip_top1(qn, bn)
    for a in (ridx, rsim):
        a.setflags(write=False)
    return torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda(), ridx, rsim


def _stats(lib, ws, n, m):
    st64 = (C.c_int32 * 64)()
    _lib.check(lib.vfm_debug_match_stats(ws.data_ptr(), n, m, C.cast(st64, C.c_void_p)))
    return list(st64)


def _search(q, b, gate, records, tune):
    """prepare -> coarse -> finish with "mx6_tune" = tune.  Returns idx, sim, the guard flag and -- fused kinds -- the sorted
    (query, chunk) pairs of the survivor lists."""
    lib = _lib.load()
    n, m = q.shape[0], b.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    qb = torch.empty(lib.vfm_match_prepared_bytes(n, D), dtype=torch.uint8, device="cuda")
    bb = torch.empty(lib.vfm_match_prepared_bytes(m, D), dtype=torch.uint8, device="cuda")
    ws = torch.empty(lib.vfm_match_search_workspace_bytes(n, m, D), dtype=torch.uint8, device="cuda")
    idx = torch.empty(n, dtype=torch.int64, device="cuda")
    sim = torch.empty(n, dtype=torch.float32, device="cuda")
    pairs = None
    with _lib.using(_lib.Config(mx6_tune=tune)):
        _lib.check(lib.vfm_match_prepare2_gated_p(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), D, PREPARE_MX6, st))
        _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, D, ws.data_ptr(), ws.numel(), records, gate, st))
        if records in (RECORDS_MX6_HALF_FUSED, RECORDS_MX6_FUSED):
            torch.cuda.synchronize()
            grid = _stats(lib, ws, n, m)[GRID_SLOT]
            assert grid > 0
            slots = ws[:grid * SLOT_WORDS * 4].view(torch.int32).cpu().numpy().reshape(grid, SLOT_WORDS)
            found = []
            for s in slots:
                cnt, qblock, c0, ns = int(s[0]), int(s[1]), int(s[2]), int(s[3]) >> 8
                assert (int(s[3]) & 1) == 0 and ns == (3 if records == RECORDS_MX6_HALF_FUSED else 2)   # no overflow; the kernel under test
                bits = 10 if ns == 3 else 9
                e = s[4:4 + cnt].astype(np.int64)
                found.append(np.stack([qblock * 256 * ns + (e & ((1 << bits) - 1)), c0 + (e >> bits)], 1))
            pairs = np.concatenate(found)
            pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
            assert (pairs[:, 0] < n).all()
        _lib.check(lib.vfm_match_search_finish_gated_r(q.data_ptr(), qb.data_ptr(), n, b.data_ptr(), bb.data_ptr(), m, D, idx.data_ptr(),
                                                       sim.data_ptr(), ws.data_ptr(), ws.numel(), gate, records, st))
        torch.cuda.synchronize()
        guard = _stats(lib, ws, n, m)[GUARD_FLAG]
    return idx, sim, guard, pairs


def _check(n, m, records, gate):
    q, b, ridx, rsim = _data(m)
    ridx, rsim = ridx[:n], rsim[:n]
    runs = [_search(q[:n].contiguous(), b, gate, records, tune) for tune in (0, ABSENT_MULTIPLIED)]
    for idx, sim, guard, pairs in runs:
        solved = _gate_contract(idx, sim, ridx, rsim, gate)
        assert solved[rsim >= 0.8].all()
        if gate == float("-inf"):
            assert solved.all()
        assert guard == 0
    (i0, s0, _, p0), (i1, s1, _, p1) = runs
    assert torch.equal(i0, i1) and torch.equal(s0, s1)
    if p0 is not None:
        assert len(p0) >= int((rsim >= 0.8).sum())       # every match at the gate survived in its chunk
        np.testing.assert_array_equal(p0, p1)
        np.testing.assert_array_equal(np.bincount(p0[:, 0], minlength=n), np.bincount(p1[:, 0], minlength=n))


@pytest.mark.parametrize("n", sorted(SIZES))
def test_fused_half_width_kernel_with_every_count_of_present_sets(n):
    assert ((n + 31) // 32) % 24 == SIZES[n] and n > 2048
    _check(n, M_FULL, RECORDS_MX6_HALF_FUSED, GATE)


@pytest.mark.parametrize("records", [RECORDS_MX6_FUSED, RECORDS_MX6, RECORDS_MX6_TOP2])
@pytest.mark.parametrize("n", [2305, 2368])
def test_two_set_kernels_with_absent_sets(n, records):
    """The full-width fused kind and the two record kinds (16 tiles per workgroup: 73 and 74 tiles leave 9 and 10 in the last one --
    a wave with one of two sets, waves with none).  The record kinds run without a gate: every row is the oracle's."""
    _check(n, M_FULL, records, GATE if records == RECORDS_MX6_FUSED else float("-inf"))


@pytest.mark.parametrize("n", [2305, 2400])
def test_remainder_block_against_a_map_whose_last_chunk_is_padding(n):
    assert M_PADDED % 128 != 0
    _check(n, M_PADDED, RECORDS_MX6_HALF_FUSED, GATE)


def test_pipeline_auto_at_one_live_tile_equals_the_int8_pass():
    """RegistrationPipeline.register with coarse="auto" (it settles on the fused fp6 half-width pass) at 73 tiles against
    coarse="int8": pose, scores, winner, inlier mask, count, correspondences and the kept queries' idx / sim equal; below the gate the
    two kinds may resolve different queries, and agree wherever both resolve."""
    n, m = 2305, M_FULL
    p = synth.make_pair_device(n, m, D, seed=23)
    outs = {}
    for coarse in ("auto", "int8"):
        pipe = RegistrationPipeline(n, m, D, n_iter=2000, coarse=coarse)
        for _ in range(3):
            out = pipe.register(p["q_desc"], p["q_xyz"], p["b_desc"], p["b_xyz"])
            pipe.synchronize()
            torch.cuda.synchronize()
            pipe._poll_feedback()
        if coarse == "auto":
            assert pipe.half and pipe.mx6_half
        outs[coarse] = {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}
    a, b = outs["auto"], outs["int8"]
    k = int(a["count"].item())
    assert k == int(b["count"].item()) and k > 500
    for key in ("T", "fitness", "rmse", "best_hyp"):
        assert torch.equal(a[key], b[key]), key
    for key in ("corres", "mask", "keep"):
        assert torch.equal(a[key][:k], b[key][:k]), key
    kept = a["sim"] >= GATE
    assert torch.equal(kept, b["sim"] >= GATE)
    both = (a["idx"] >= 0) & (b["idx"] >= 0)
    assert bool((both | ~kept).all())
    assert torch.equal(a["idx"][both], b["idx"][both]) and torch.equal(a["sim"][both], b["sim"][both])
