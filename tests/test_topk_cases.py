"""CPU: the launch plans and scenes of tests/topk_cases.py have the properties their docstrings claim -- checked with the arithmetic of
csrc/match_topk.hip written down again and with the oracle of tests/topk_oracle.py alone, never with a device."""
import importlib.util
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import topk_cases as cases
from tests import topk_oracle as to

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def lib():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib.load()


def cosines(orc, q, b):
    """fp64 scores of the rows as the search normalises them, [n, m]"""
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    return qn.astype(np.float64) @ bn.astype(np.float64).T


# ------------------------------------------------------------------------------------------------------------ the launches
def chunks_slices(plan):
    return [(c, s) for _, c, s in plan]


def test_pinned_plans():
    for d in cases.FAST_WIDTHS:
        assert [c for _, c, _ in cases.launch_plan(33, 2049, d)] == [16, 2], d
        assert [c for _, c, _ in cases.launch_plan(33, 4097, d)] == [16, 18], d
        assert [c for _, c, _ in cases.launch_plan(33, 8193, d)] == [16, 48, 2], d
        for n in (33, 257):
            assert chunks_slices(cases.launch_plan(n, 4097, d, 1000)) == [(16, 1), (18, 18)], (n, d)   # 18 one-chunk slices
            assert chunks_slices(cases.launch_plan(n, 4097, d, 5)) == [(16, 1), (18, 5)], (n, d)
            assert chunks_slices(cases.launch_plan(n, 4097, d, 2)) == [(16, 1), (18, 2)], (n, d)
        assert chunks_slices(cases.launch_plan(33, 2049, d, 1000)) == [(16, 1), (2, 2)], d
        assert chunks_slices(cases.launch_plan(33, 8193, d, 1000)) == [(16, 1), (48, 48), (2, 2)], d
        # the first launch is one slice whatever is forced; the short last launch of two chunks stays one slice unforced
        assert cases.launch_plan(33, 2049, d)[1][2] == 1 and cases.launch_plan(33, 8193, d)[2][2] == 1
    assert cases.launch_plan(1, 1, 128) == [(0, 2, 1)]
    assert cases.launch_plan(4, 2048, 128) == [(0, 16, 1)] and cases.launch_plan(4, 2048, 768) == [(0, 16, 1)]
    assert cases.max_slices(257, 4097, 768, 1000) == 18 and cases.max_slices(1, 300, 128, 1000) == 1


def test_plans_are_the_tools_plans_when_nothing_is_forced():
    spec = importlib.util.spec_from_file_location("sim_topk_records", ROOT / "tools" / "sim_topk_records.py")
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    assert (sim.SEED_CHUNKS, float(sim.WINDOW)) == (cases.SEED_CHUNKS, float(np.float32(cases.WINDOW)))
    for d in cases.FAST_WIDTHS:
        for n in (1, 33, 129, 257, 4000, 70000):
            for m in (1, 5, 129, 300, 2049, 4097, 8193, 20000, 200000):
                assert cases.launch_plan(n, m, d) == sim.launches(n, m, d), (n, m, d)
    for nqb in (1, 2, 3, 16, 100, 300):
        for nchunks in (1, 2, 8, 18, 48, 156, 1563):
            assert cases.choose_slices(nqb, nchunks) == sim.choose_slices(nqb, nchunks), (nqb, nchunks)


@pytest.mark.parametrize("forced", [0, 2, 5, 1000])
def test_every_plan_covers_the_map_in_slices_of_whole_chunks(forced):
    for d in (128, 768):
        for n, m in ((1, 1), (33, 2049), (257, 4097), (33, 8193), (64, 20000)):
            plan = cases.launch_plan(n, m, d, forced)
            total = (m + 255) // 256 * 2
            assert plan[0][:2] == (0, min(total, 16)) and plan[0][2] == 1
            assert sum(c for _, c, _ in plan) == total
            for (c0, c, s), nxt in zip(plan, plan[1:] + [(total, 0, 0)]):
                assert c0 + c == nxt[0] and 1 <= s <= c    # a slice holds at least one chunk: four tiles
                assert forced == 0 or plan.index((c0, c, s)) == 0 or s == min(forced, c)


# ------------------------------------------------------------------------------------------------------------ the crowded workgroup
@pytest.mark.parametrize("d", [128, 256, 768])
def test_crowded_workgroup_fills_the_buffer_and_no_list(orc, d):
    q, b = cases.crowded_workgroup(d)
    assert q.shape == (cases.CROWD_N, d) and b.shape == (cases.CROWD_M, d) and q.dtype == b.dtype == np.float32
    assert cases.launch_plan(cases.CROWD_N, cases.CROWD_M, d) == [(0, 16, 1)]      # one launch, one slice
    assert (cases.CROWD_N + 127) // 128 == 1                                       # the live queries sit in one workgroup in both forms
    s = cosines(orc, q, b)
    near_before_winners = 0
    for j in range(cases.CROWD_N):
        near = s[j, cases.crowded_near_rows(j)]
        spread = near.max() - near.min()
        print(f"d={d} query {j}: near-copies {near.min():.6f} .. {near.max():.6f} (spread {spread:.2e})")
        assert spread <= 2e-4                                                      # (a)
        assert spread + 2 * cases.COARSE_ERROR <= cases.WINDOW                     # ... so every one is inside any window
        in_window = int((s[j] >= near.min() - 2 * cases.WINDOW).sum())
        print(f"d={d} query {j}: {in_window} rows in the window, {in_window + cases.FIRST_STEPS_ROWS} with the first steps")
        assert in_window == cases.CROWD_NEAR + 8
        assert in_window + cases.FIRST_STEPS_ROWS < cases.RECORD_CAP               # (b)
        rows = cases.crowded_near_rows(j)
        assert rows.max() < cases.CROWD_FIRST_WINNER
        near_before_winners += len(rows)
        # the winners are nearer than the coarse pass can tell: only the fp64 finish separates them from the near-copies
        assert 0 < s[j, cases.crowded_winners(j)].min() - near.max() < cases.COARSE_ERROR
    assert len({int(r) for j in range(cases.CROWD_N) for r in cases.crowded_near_rows(j)}) == near_before_winners
    assert near_before_winners > cases.LREC_CAP                                    # (c)
    idx, sim = to.topk(q, b, cases.CROWD_K)
    for j in range(cases.CROWD_N):                                                 # (d)
        np.testing.assert_array_equal(idx[j], cases.crowded_winners(j))
        assert len(set(sim[j].view(np.uint32).tolist())) == 1


# ------------------------------------------------------------------------------------------------------------ the stale workspace
@pytest.mark.parametrize("d", [128, 768])
def test_stale_maker_overflows_a_list_and_is_the_larger_call(orc, lib, d):
    q, b = cases.stale_maker(d)
    assert q.shape == (cases.STALE_N, d) and b.shape == (cases.STALE_M, d) and cases.STALE_N == 2 * 257 + 3
    copies = (b == q[cases.STALE_QUERIES[0]]).all(1)
    assert copies.sum() == cases.STALE_COPIES > cases.RECORD_CAP
    for i in cases.STALE_QUERIES:
        assert np.array_equal(q[i], q[cases.STALE_QUERIES[0]])
    assert max(cases.STALE_QUERIES) > 257                      # a stale fallback list names a query the later calls do not have
    assert len(cases.launch_plan(cases.STALE_N, cases.STALE_M, d)) == 2
    # every row of one score: more of them than a list holds inside every window, whatever the bound
    s = cosines(orc, q[[cases.STALE_QUERIES[0]]], b)[0]
    assert int((s >= s.max() - 1e-9).sum()) == cases.STALE_COPIES
    need = lib.vfm_match_ip_topk_workspace_bytes(cases.STALE_N, cases.STALE_M, d, cases.STALE_K, 0)
    for n, m in ((257, 2049), (257, 300), (33, 2049), (129, 300), (1, 1)):
        assert need >= lib.vfm_match_ip_topk_workspace_bytes(n, m, d, 8, 0) > 0
    assert lib.vfm_match_ip_topk_prepared_workspace_bytes(cases.STALE_N, d, 8) > lib.vfm_match_ip_topk_prepared_workspace_bytes(257, d, 8)
