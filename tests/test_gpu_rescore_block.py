"""match_rescore_kernel with 64 and with 256 queries per workgroup (policy key "rescore_block"): the fp64 decision adds the same products
in the same order either way, so idx / sim of the two forms are bit-equal, and equal to the oracle (under the gate contract where the
search is gated).  Shapes are the smallest at which the 256 form can go wrong: a last block that is partly filled, one block that holds
several epochs of pairs, whole-chunk entries, ties between queries of different waves of a block, zero rows, lists handed to
match_exact_kernel, and one plan that reaches the kernel behind the int8 pass."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from vfmreg import _lib, ops  # noqa: E402

from .test_gpu_half_noi8 import GATE, N, _d2_pair, _fb_count, _oracle, _search, _view, workspace_layout  # noqa: E402
from .test_gpu_int8 import _gate_contract  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCKS = (64, 256)


def _both(run):
    """run() under either block size -> {block: what run returned}"""
    out = {}
    for block in BLOCKS:
        with _lib.using(_lib.Config(rescore_block=block)):
            assert _lib.policy("rescore_block") == block
            out[block] = run()
            torch.cuda.synchronize()
    return out


def _same(a, b):
    assert torch.equal(a[0], b[0]), "idx of the two forms differ"
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "sim of the two forms differ"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def test_a_scan_that_is_no_multiple_of_256_behind_the_fp6_pass():
    """n = 2100 = 8 x 256 + 52, m = 4096, records 8 | VFM_RECORDS_NO_I8 on a D.2 pair"""
    _, _, q, b, ridx, rsim = _d2_pair(384, N, 4096)
    got = _both(lambda: _search(q, b, True)[:2])
    _same(got[64], got[256])
    for block in BLOCKS:
        solved = _gate_contract(*got[block], ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all()
    assert int((got[256][0] >= 0).sum()) > N // 4


@pytest.mark.parametrize("d", [256, 384])
def test_one_full_block_and_one_partly_filled(d):
    """n = 300: queries 0 .. 255 and 256 .. 299 (vfm_match_ip_top1, ungated: every query is resolved and equal to the oracle)"""
    from vfmreg import synth
    p = synth.make_pair(300, 1500, d, seed=3)
    q, b = p["q_desc"] * np.float32(3.7), p["b_desc"] * np.float32(0.21)
    ridx, rsim = _oracle(q, b)
    qd, bd = _dev(q), _dev(b)
    got = _both(lambda: ops.match_ip_top1(qd, bd, ops.FAST))
    _same(got[64], got[256])
    np.testing.assert_array_equal(got[256][0].cpu().numpy(), ridx)
    np.testing.assert_array_equal(got[256][1].cpu().numpy(), rsim)


def test_more_than_1024_single_row_candidates_in_one_block():
    """35 near-duplicates of one direction, one per 128-row chunk, and 230 queries of ONE 256-query block pointing at them: 8050 pairs =
    eight epochs of the pair table in the 256 form (in the 64 form: 2240, 2240, 2240 and 1330 pairs in four blocks); the queries of
    the second block (256 .. 299) point there too"""
    rng = np.random.default_rng(99)
    d, m, n = 384, 40 * 128, 300
    b = rng.standard_normal((m, d)).astype(np.float32)
    base = rng.standard_normal(d).astype(np.float32)
    rows = np.arange(35) * 128 + rng.integers(0, 128, 35)
    b[rows] = base + 2e-4 * rng.standard_normal((35, d)).astype(np.float32)
    q = rng.standard_normal((n, d)).astype(np.float32)
    aimed = np.r_[0:230, 256:290]
    q[aimed] = base + 1e-3 * rng.standard_normal((len(aimed), d)).astype(np.float32)
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    ridx, rsim = orc.match_ip_top1_bruteforce(qn, bn)
    assert np.isin(ridx[aimed], rows).all()
    qp, bp = ops.PreparedRows(_dev(q)), ops.PreparedRows(_dev(b))
    lay, cap, _ = workspace_layout(n, m)
    ws = torch.zeros(_lib.load().vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device="cuda")
    assert lay["_end"][0] == ws.numel()
    got = _both(lambda: tuple(t.clone() for t in ops.match_search(qp, bp, ws=ws)))
    _same(got[64], got[256])
    np.testing.assert_array_equal(got[256][0].cpu().numpy(), ridx)
    np.testing.assert_array_equal(got[256][1].cpu().numpy(), rsim)
    # the lists the decision saw: block 0 of the 256 form really holds several epochs of single-row pairs
    cand_cnt = _view(ws, lay, "cand_cnt", torch.int32).cpu().numpy()[:n]
    cand = _view(ws, lay, "cand", torch.int32).cpu().numpy().reshape(-1, cap)[:n]
    pairs = [int(((cand[qi, :max(cand_cnt[qi], 0)] & 128) == 0).sum()) for qi in range(n)]
    assert sum(pairs[:256]) > 4 * 1024, sum(pairs[:256])
    assert max(sum(pairs[g:g + 64]) for g in range(0, 256, 64)) > 1024


def test_a_full_bin_leaves_whole_chunk_entries_in_the_other_waves_of_a_block():
    """1700 queries (seven 256-query blocks) matched to rows of one chunk overflow its bin of 1152: at least 548 of them keep a
    whole-chunk entry that the fp64 decision scores row by row -- more than the 7 x 64 that wave 0 of those blocks could hold, so
    some belong to the other waves of a 256-query block whichever queries the bin's atomics let in"""
    d, n, m, chunk = 384, N, 34000, 77
    rng = np.random.default_rng(5)
    b = rng.standard_normal((m, d)).astype(np.float32)
    q = rng.standard_normal((n, d)).astype(np.float32)
    crowd = 1700
    rows = chunk * 128 + rng.integers(0, 128, crowd)
    q[:crowd] = b[rows] + 0.02 * rng.standard_normal((crowd, d)).astype(np.float32)
    ridx, rsim = _oracle(q, b)
    lay, cap, bin_cap = workspace_layout(n, m)
    assert crowd > bin_cap
    qd, bd = _dev(q), _dev(b)
    got = _both(lambda: _search(qd, bd, True))
    _same(got[64], got[256])
    for block in BLOCKS:
        idx, sim, _, _, ws = got[block]
        solved = _gate_contract(idx, sim, ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all() and solved[:crowd].all()
        cand_cnt = _view(ws, lay, "cand_cnt", torch.int32).cpu().numpy()[:n]
        cand = _view(ws, lay, "cand", torch.int32).cpu().numpy().reshape(-1, cap)[:n]
        whole = np.array([qi for qi in range(crowd) if (cand[qi, :max(cand_cnt[qi], 0)] & 128).any()])
        assert len(whole) >= crowd - bin_cap > 7 * 64
        # (wave 0 of the seven blocks owns 448 of the crowd's queries: at least 100 of the entries belong to waves 1 - 3)
        assert int(((whole % 256) // 64 > 0).sum()) >= crowd - bin_cap - 7 * 64 >= 100


def test_duplicated_map_rows_tie_to_the_lowest_index_across_the_waves_of_a_block():
    """the same map row three times (in one chunk and in two others); its queries -- exact copies, scaled copies, near copies -- sit in
    the four 64-query groups of block 1 (queries 256 .. 511) and in the partly filled last block; a zero query row in a wave other than
    wave 0 and one in the last block"""
    d, n, m = 384, N, 4096
    q0, b0 = _d2_pair(d, n, m)[:2]
    q, b = q0.copy(), b0.copy()
    rng = np.random.default_rng(3)
    for lo, his in ((5, (77, 3000)), (200, (210, 1500))):
        for hi in his:
            b[hi] = b[lo]
    tied = []
    for k, at in enumerate((256 + 3, 256 + 64 + 9, 256 + 128 + 60, 256 + 192 + 63, 2048 + 40)):
        for j, row in enumerate((5, 77, 3000, 200, 210, 1500)):
            qi = at - j if at % 64 > 32 else at + j
            q[qi] = (b[row], 2.5 * b[row], b[row] + 0.01 * rng.standard_normal(d).astype(np.float32))[(k + j) % 3]
            tied.append(qi)
    q[256 + 100] = 0.0
    q[2099] = 0.0
    ridx, rsim = _oracle(q, b)
    assert set(ridx[tied].tolist()) == {5, 200} and len(set(tied)) == 30
    qd, bd = _dev(q), _dev(b)
    got = _both(lambda: _search(qd, bd, True)[:2])
    _same(got[64], got[256])
    for block in BLOCKS:
        idx, sim = got[block]
        solved = _gate_contract(idx, sim, ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all() and solved[tied].all()
        for z in (256 + 100, 2099):
            assert int(idx[z]) == 0 and float(sim[z]) == 0.0


def test_descriptors_that_are_all_alike_are_left_to_the_exact_kernel():
    """the guard comes up: cand_cnt = -1 for every live query, match_rescore_kernel writes only the zero row's answer"""
    d, n, m = 384, N, 1024
    rng = np.random.default_rng(6)
    base = rng.standard_normal(d).astype(np.float32)
    b = (base + 0.05 * rng.standard_normal((m, d))).astype(np.float32)
    q = (base + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    q[11] = 0.0
    q[300] = 0.0
    ridx, rsim = _oracle(q, b)
    qd, bd = _dev(q), _dev(b)
    got = _both(lambda: _search(qd, bd, True))
    _same(got[64], got[256])
    lay, _, _ = workspace_layout(n, m)
    for block in BLOCKS:
        idx, sim, _, _, ws = got[block]
        assert _fb_count(ws, n, m)[7] == 1
        cand_cnt = _view(ws, lay, "cand_cnt", torch.int32).cpu().numpy()[:n]
        assert (np.delete(cand_cnt, [11, 300]) == -1).all()
        np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
        np.testing.assert_array_equal(sim.cpu().numpy(), rsim)


def test_behind_the_int8_pass():
    """records 0 (best-score int8 records) on prepared operands, m = 4096: the plan's other route to the kernel"""
    _, _, q, b, ridx, rsim = _d2_pair(384, N, 4096)
    qp, bp = ops.PreparedRows(q), ops.PreparedRows(b)
    assert _lib.search_plan(0, 384, N, 4096)["pass"] == "int8"
    got = _both(lambda: ops.match_search_gated(qp, bp, GATE, records=0))
    _same(got[64], got[256])
    for block in BLOCKS:
        solved = _gate_contract(*got[block], ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all()
