"""Exact ties across the four waves of the all-pairs kernels (match_exact_kernel, match_topk_exact_kernel, nn_l2_kernel): they share
one order and one workgroup-wide arg-max (csrc/match_exact.h), and a tie between waves is where a fold that keeps the winner it saw
first differs from the oracle's rule -- equal scores go to the lowest map index.  Thread t of the 256 scores map rows t, t + 256, ...;
of 300 map rows at d = 36 (no matrix-core kernel at that width in either search) four are identical copies of the row every query
is a noisy copy of:
  "ascending"  rows 5, 70, 135, 200: one copy per wave, waves 0 to 3 -- the answer is 5;
  "wave 0 last" rows 70, 135, 200, 260: row 260 is thread 4's second row, so wave 0, whose winner every fold sees first, holds the
                HIGHEST index -- the answer is 70, and 260 comes last of the four.
idx / sim / nn / d2 are compared bit for bit with the oracles the other tests of these entry points use."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from tests import topk_oracle as to  # noqa: E402

M, D, NQ = 300, 36, 9
COPIES = {"ascending": (5, 70, 135, 200), "wave 0 last": (70, 135, 200, 260)}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


@pytest.fixture(scope="module", params=list(COPIES))
def case(request):
    """(copies, q, b) and the oracles' answers, computed once per map"""
    copies = COPIES[request.param]
    rng = np.random.default_rng(36)
    b = rng.standard_normal((M, D)).astype(np.float32)
    b[list(copies)] = b[copies[0]]
    q = (b[copies[0]] + 0.01 * rng.standard_normal((NQ, D))).astype(np.float32)
    assert len({w for w in ((r % 256) // 64 for r in copies)}) == 4, "one copy per wave"
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    return dict(copies=copies, q=q, b=b, top1=orc.match_ip_top1_bruteforce(qn, bn), topk=to.topk(q, b, 4), l2=orc.nn_l2(q, b))


def test_top1_exact_takes_the_lowest_of_four_equal_rows(case):
    from vfmreg import ops
    idx, sim = ops.match_ip_top1(_dev(case["q"]), _dev(case["b"]), ops.EXACT)
    want_idx, want_sim = case["top1"]
    assert (want_idx == case["copies"][0]).all()
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(sim.cpu().numpy().view(np.uint32), want_sim.view(np.uint32))


def test_topk_exact_lists_the_four_equal_rows_in_index_order(case):
    from vfmreg import ops
    idx, sim = ops.match_ip_topk(_dev(case["q"]), _dev(case["b"]), 4, ops.EXACT)
    want_idx, want_sim = case["topk"]
    assert (want_idx == np.array(case["copies"])).all() and (want_sim == want_sim[:, :1]).all()
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(sim.cpu().numpy().view(np.uint32), want_sim.view(np.uint32))


def test_l2_exact_takes_the_lowest_of_four_equally_near_rows(case):
    from vfmreg import ops
    nn, d2, _ = ops.match_mutual_l2(_dev(case["q"]), _dev(case["b"]), mutual=False, prec=ops.EXACT)
    want_nn, want_dist = case["l2"]
    assert (want_nn == case["copies"][0]).all()
    np.testing.assert_array_equal(nn.cpu().numpy(), want_nn)
    np.testing.assert_array_equal(np.sqrt(d2.cpu().numpy()), want_dist)
