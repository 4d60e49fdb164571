"""RANSAC's bounds, selection and exact re-scoring on the GPU, hypothesis by hypothesis (csrc/ransac.hip).

The other RANSAC tests compare the winner, its pose and its mask with the oracle: an unsound bound shows there only when it prunes the one
hypothesis that wins.  Here every case of tests/ransac_bound_cases.py runs under each of the three chains ("ransac_fused" 2, 1, 0) with a
caller-owned workspace, vfm_debug_ransac_state reads back what the call left in it, and the oracle's per-hypothesis record
(orc.ransac_corr(per_hyp=True)) is the reference for
    bounds      n_hi < 0 <=> degenerate sample; n_lo <= inliers <= n_hi; r_lo <= rmse <= r_hi -- for EVERY hypothesis; and not vacuous
    state       F = max n_lo, R* = min r_hi over n_lo = n_hi = F, unsure / overflow as the case declares
    survivors   the candidate list is exactly {n_hi > 0, n_hi >= F, n_hi > F or r_lo <= R*} and holds the oracle's winner
    scores      every survivor's stored (fitness, rmse) is the oracle's record bit for bit; per-block slots hold the best of their block
    result      T, fitness, rmse, best_hyp, mask equal the oracle's
tests/test_ransac_bound_cases.py shows on the CPU that bounds computed from the documented formulas meet all of this."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from tests import ransac_bound_cases as rb  # noqa: E402

CHAINS = (2, 1, 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def read_state(ws, c_max, n_iter):
    from vfmreg import _lib
    nslots = rb.CAND_MAX + (n_iter + 63) // 64
    st = dict(n_lo=np.empty(n_iter, np.int32), n_hi=np.empty(n_iter, np.int32), r_lo=np.empty(n_iter), r_hi=np.empty(n_iter),
              sel=np.empty(4, np.int32), rstar=np.empty(1), list=np.full(rb.CAND_MAX, -1, np.int32),
              fit=np.empty(nslots), rmse=np.empty(nslots), hyp=np.empty(nslots, np.int32))
    p = lambda k: C.c_void_p(st[k].ctypes.data)  # noqa: E731
    _lib.check(_lib.load().vfm_debug_ransac_state(ws.data_ptr(), c_max, n_iter, p("n_lo"), p("n_hi"), p("r_lo"), p("r_hi"), p("sel"),
                                                  p("rstar"), p("list"), p("fit"), p("rmse"), p("hyp")), "debug_ransac_state")
    st.update(F=int(st["sel"][0]), count=int(st["sel"][1]), overflow=int(st["sel"][2]), unsure=int(st["sel"][3]), Rstar=float(st["rstar"][0]))
    return st


def run(case, chain, count=None, c_max=None):
    from vfmreg import _lib, ops
    corres = case["corres"]
    if c_max is not None:
        corres = np.ascontiguousarray(np.resize(corres, (c_max, 2)))
    need = _lib.load().vfm_ransac_workspace_bytes(len(corres), case["n_iter"])
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    with _lib.using(_lib.Config(ransac_fused=chain)):
        out = ops.ransac_corr(dev(case["src"]), dev(case["tgt"]), dev(corres), case["max_dist"], case["n_iter"], seed=case["seed"],
                              count=count, ws=ws)
        torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    return res, read_state(ws, len(corres), case["n_iter"])


def test_table_has_every_path_for_every_chain():
    """closed-form, point-wise and overflow are each declared by some case; test_bounds_survivors_and_scores holds every chain to the
    declaration of every case (chain 1 has no list, so an "overflow" case is one with more than CAND_MAX survivors there)"""
    assert {rb.make(n)["path"] for n in rb.NAMES if n != "loop-second-round"} == {"closed-form", "point-wise", "overflow"}


@pytest.mark.parametrize("name", rb.NAMES)
def test_bounds_survivors_and_scores(name):
    kw = {}
    if name == "loop-second-round":
        kw["cus"] = torch.cuda.get_device_properties(0).multi_processor_count
    case = rb.make(name, **kw)
    C_ = len(case["corres"])
    ref = orc.ransac_corr(case["src"], case["tgt"], case["corres"], case["max_dist"], case["n_iter"], seed=case["seed"], per_hyp=True)
    T, _ = rb.hypotheses(case, orc)
    eta = rb.eta_of(case, T)
    for chain in CHAINS:
        tag = f"{name}, chain {chain}"
        res, st = run(case, chain)
        print(f"{tag}: unsure {st['unsure']} overflow {st['overflow']} survivors {st['count']} F {st['F']} R* {st['Rstar']:.6g}")
        rb.check_bounds(tag, case, st, ref)
        rb.check_not_vacuous(tag, case, st, st["unsure"], eta)
        surv = rb.check_state(tag, case, st, chain)
        rb.check_survivors_and_scores(tag, case, st, ref, chain, surv)
        assert res["best_hyp"].item() == ref.best_hyp, f"{tag}: winner h = {res['best_hyp'].item()}, the oracle's is h = {ref.best_hyp}"
        np.testing.assert_array_equal(res["T"], ref.transformation, err_msg=tag)
        assert res["fitness"].item() == ref.fitness and res["rmse"].item() == ref.inlier_rmse, tag
        np.testing.assert_array_equal(res["mask"][:C_], ref.inlier_mask, err_msg=tag)
        if name in rb.DEGENERATE:
            assert ref.best_hyp == -1 and ref.fitness == 0.0 and not ref.inlier_mask.any()
            np.testing.assert_array_equal(ref.transformation, np.eye(4))
            assert st["count"] == 0 and (st["n_hi"] < 0).all(), tag


@pytest.mark.parametrize("count", [0, 1, 2])
def test_fewer_than_three_correspondences_on_the_device(count):
    """the number of correspondences is known on the device only: with 0, 1 or 2 of c_max = 70 every chain returns the default result,
    clears the mask over all of c_max and finds nothing to score"""
    case = rb.make("chunk-127-65")
    cnt = torch.tensor([count], dtype=torch.int64, device="cuda")
    for chain in CHAINS:
        tag = f"count {count}, chain {chain}"
        res, st = run(case, chain, count=cnt, c_max=70)
        np.testing.assert_array_equal(res["T"], np.eye(4), err_msg=tag)
        assert res["fitness"].item() == 0.0 and res["rmse"].item() == 0.0 and res["best_hyp"].item() == -1, tag
        assert len(res["mask"]) == 70 and not res["mask"].any(), tag
        assert (st["n_hi"] < 0).all() and st["count"] == 0 and st["overflow"] == 0 and st["F"] == 0, tag
        assert (st["hyp"][rb.CAND_MAX:] == -1).all() and (chain == 1 or (st["hyp"][:rb.CAND_MAX] == -1).all()), tag
