"""The k-best descriptor search (csrc/match_topk.hip) where its launch arithmetic and its record buffers change behaviour, against the
oracle of tests/topk_oracle.py: ``idx`` and ``sim`` EQUAL bit for bit.

  1. forced map slices at every width -- ``coarse_slices`` of vfm_config, which choose_slices honours: 2, 5 and 18 one-chunk slices in
     one launch, whose workgroups tighten one another's bound through the published ``tau``; a one-chunk slice is four tiles, the
     shortest walk the LDS ring can make (the 8-wave form stages all of it in the prologue);
  2. a last launch of two chunks, after one launch and after two;
  3. a workgroup whose LDS record buffer is full while every query stays under its own cap: the late records take the buffer-full
     branch and the fp64 finish -- not the all-pairs kernel -- must find the answer among them (tests/topk_cases.py, conditions
     checked on the CPU by tests/test_topk_cases.py);
  4. one workspace, pre-filled with bytes 0xFF, through calls of different sizes and k, on the default and on a side stream.

The plans the shapes are chosen for are asserted with tests/topk_cases.py, so the shapes keep meaning what they are for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import topk_cases as tc  # noqa: E402
from tests import topk_oracle as to  # noqa: E402
from tests.test_gpu_topk_wide import INFO, dev, equal, oracle8, rows  # noqa: E402  (one cache of rows and oracles for both files)

FAST = 0
WIDTHS = tc.FAST_WIDTHS


def lib_():
    from vfmreg import _lib
    return _lib


def search(q, b, k, slices=0, prepared=False, ws=None):
    """(idx, sim, info) of the FAST search, with ``coarse_slices`` forced when ``slices`` > 0"""
    from vfmreg import ops
    L = lib_()
    qd, bd = dev(q), dev(b)
    with L.using(L.Config(coarse_slices=slices) if slices else None):
        if prepared:
            idx, sim, info = ops.match_ip_topk_prepared(ops.PreparedRows(qd), ops.PreparedRows(bd), k, ws=ws, return_info=True)
        else:
            idx, sim, info = ops.match_ip_topk(qd, bd, k, FAST, ws=ws, return_info=True)
    return idx.cpu().numpy(), sim.cpu().numpy(), dict(zip(INFO, info.cpu().tolist()))


def first_k(want, n, k):
    """the oracle's answer for the first n queries and k candidates from its eight best (it picks round by round, query by query)"""
    return want[0][:n, :k], want[1][:n, :k]


# ------------------------------------------------------------------------------------------------- 1. forced slices
def test_ops_widths_are_the_cases_widths():
    from vfmreg import ops
    assert ops.MATCH_TOPK_FAST_WIDTHS == WIDTHS and ops.MATCH_TOPK_RECORD_CAP == tc.RECORD_CAP


@pytest.mark.parametrize("common", [False, True], ids=["gaussian", "common-component"])
@pytest.mark.parametrize("d", WIDTHS)
def test_forced_slices_share_one_bound_at_every_width(d, common):
    """(33 | 257) x 4097: the second launch holds 18 chunks -- in 2, 5 and 18 slices.  The 33 queries are the first 33 of the 257, on
    the same map: one oracle serves both.  The common-component rows have the densest records."""
    m = 4097
    q, b = rows(257, m, d, 1, common)
    want = oracle8(257, m, d, 1, common)
    assert [(c, s) for _, c, s in tc.launch_plan(257, m, d, 1000)] == [(16, 1), (18, 18)]
    for n in (33, 257):
        for k in (1, 8):
            free = search(q[:n], b, k)
            print(f"d={d} n={n} k={k} unforced: {free[2]}")
            equal(free[0], free[1], first_k(want, n, k), "unforced")
            assert free[2]["slices"] == tc.max_slices(n, m, d) and free[2]["fallback"] == 0
            for s in (2, 5, 1000):
                idx, sim, info = search(q[:n], b, k, slices=s)
                print(f"d={d} n={n} k={k} coarse_slices={s}: {info}")
                equal(idx, sim, first_k(want, n, k), f"coarse_slices={s}")
                equal(idx, sim, free[:2], f"coarse_slices={s} against the unforced call")
                assert info["fallback"] == 0 and info["reserved"] == 0
                assert info["slices"] == tc.max_slices(n, m, d, s) == min(s, 18)
                assert k <= info["max_records"] <= tc.RECORD_CAP


# ------------------------------------------------------------------------------------------------- 2. a short last launch
@pytest.mark.parametrize("m,launches", [(2049, 2), (8193, 3)])
@pytest.mark.parametrize("d", [128, 256, 768])
def test_last_launch_of_two_chunks(d, m, launches):
    """m = 2049: launches of 16 + 2 chunks; m = 8193: 16 + 48 + 2.  The bound kernel runs, then a launch of eight tiles follows."""
    n, k = 33, 8
    plan = tc.launch_plan(n, m, d)
    assert len(plan) == launches and plan[-1][1:] == (2, 1)
    assert tc.launch_plan(n, m, d, 1000)[-1][1:] == (2, 2)
    q, b = rows(n, m, d, 21)
    want = to.topk(q, b, k)
    for s in (0, 1000):
        for prepared in (False, True):
            idx, sim, info = search(q, b, k, slices=s, prepared=prepared)
            print(f"d={d} m={m} coarse_slices={s} prepared={prepared}: {info}")
            equal(idx, sim, want, f"coarse_slices={s} prepared={prepared}")
            assert info["fallback"] == 0 and info["slices"] == tc.max_slices(n, m, d, s)
            assert k <= info["max_records"] <= tc.RECORD_CAP


# ------------------------------------------------------------------------------------------------- 3. a crowded workgroup
@pytest.mark.parametrize("prepared", [False, True], ids=["unprepared", "prepared"])
@pytest.mark.parametrize("d", [128, 256, 768])
def test_crowded_workgroup_is_decided_from_its_records(d, prepared):
    """tests/topk_cases.py, crowded_workgroup: 1920 near-copies fill the workgroup's buffer of 1536 before the 32 winners arrive, and no
    query comes near its own cap of 1024 -- so the winners' records take the buffer-full branch and the finish kernel decides from
    them.  A record lost there is a wrong answer here: nothing falls back to the all-pairs kernel."""
    q, b = tc.crowded_workgroup(d)
    want = to.topk(q, b, tc.CROWD_K)
    for j in range(tc.CROWD_N):
        np.testing.assert_array_equal(want[0][j], tc.crowded_winners(j))
    idx, sim, info = search(q, b, tc.CROWD_K, prepared=prepared)
    print(f"d={d} prepared={prepared}: {info}")
    equal(idx, sim, want)
    assert info["fallback"] == 0 and info["slices"] == 1
    assert tc.CROWD_NEAR + 8 <= info["max_records"] <= tc.RECORD_CAP


# ------------------------------------------------------------------------------------------------- 4. one workspace, many calls
def workspace_sequence(d):
    """[(q, b, k, oracle)]: the call that overflows two lists, then smaller calls of other sizes and k, the second one again at the end"""
    sq, sb = tc.stale_maker(d)
    big = (*rows(257, 4097, d), 8, oracle8(257, 4097, d))
    mid_q, mid_b = rows(33, 300, d)
    small_q, small_b = rows(1, 5, d)
    return [(sq, sb, tc.STALE_K, to.topk(sq, sb, tc.STALE_K)), big, (mid_q, mid_b, 1, to.topk(mid_q, mid_b, 1)),
            (small_q, small_b, 8, to.topk(small_q, small_b, 8)), big]


@pytest.mark.parametrize("d", [256, 768])
def test_one_workspace_serves_calls_of_every_size(d):
    from vfmreg import ops
    L = lib_().load()
    seq = workspace_sequence(d)
    need = max(L.vfm_match_ip_topk_workspace_bytes(len(q), len(b), d, k, FAST) for q, b, k, _ in seq)
    side = torch.cuda.Stream()
    for name, stream in (("default stream", torch.cuda.current_stream()), ("side stream", side)):
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
        got = []
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for q, b, k, _ in seq:
                idx, sim, info = ops.match_ip_topk(dev(q), dev(b), k, FAST, ws=ws, return_info=True)
                got.append((idx, sim, info))
        stream.synchronize()
        for i, ((q, b, k, want), (idx, sim, info)) in enumerate(zip(seq, got)):
            info = dict(zip(INFO, info.cpu().tolist()))
            print(f"d={d} {name} call {i}: n={len(q)} m={len(b)} k={k}: {info}")
            equal(idx.cpu().numpy(), sim.cpu().numpy(), want, f"{name}, call {i}")
            assert info["slices"] == tc.max_slices(len(q), len(b), d) and info["reserved"] == 0
            if i == 0:   # a query whose eight best are all copies of the repeated row has all 1100 of them inside its window
                copies = (b == q[tc.STALE_QUERIES[0]]).all(1)
                sure = int(copies[want[0]].all(1).sum())
                assert len(tc.STALE_QUERIES) <= sure <= info["fallback"] <= len(q), (name, sure, info)
            else:
                assert info["fallback"] == 0, (name, i, info)
            assert (info["max_records"] > tc.RECORD_CAP) == (i == 0), (name, i, info)
        assert torch.equal(got[4][0], got[1][0]) and torch.equal(got[4][1].view(torch.int32), got[1][1].view(torch.int32)), name
