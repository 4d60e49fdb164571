"""tests/ransac_bound_cases.py on the CPU: the two bound generators of csrc/ransac.hip, emulated in numpy from the formulas of DESIGN.md 4.3,
meet the contract that tests/test_gpu_ransac_bounds.py holds the kernels to -- [n_lo, n_hi] contains the oracle's inlier count and
[r_lo, r_hi] its RMSE for EVERY hypothesis -- on every case of the table, and every case takes the path and shows the property it was
built for.  This pins the inputs and shows that the claims can be met."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import ransac_bound_cases as rb


@pytest.fixture(scope="module")
def done():
    cache = {}

    def get(name):
        if name not in cache:
            case = rb.make(name)
            ref = orc.ransac_corr(case["src"], case["tgt"], case["corres"], case["max_dist"], case["n_iter"], seed=case["seed"], per_hyp=True)
            cache[name] = (case, ref, rb.emulate(case, orc))
        return cache[name]
    return get


def test_philox_picks_are_the_oracles():
    picks = rb.philox_picks(300, 0x1234567890ABCDEF, 1000)
    for h in (0, 1, 63, 64, 299):
        w = orc.philox(h, 0x1234567890ABCDEF)
        assert [(int(w[k]) * 1000) >> 32 for k in range(3)] == picks[h].tolist()


def test_table_covers_every_path_and_stays_small():
    paths = {}
    for name in rb.NAMES:
        case = rb.make(name)
        paths.setdefault(case["path"], []).append(name)
        assert len(case["corres"]) <= 3000
        assert case["n_iter"] <= 6000 or name == "loop-second-round"
    assert set(paths) == {"closed-form", "point-wise", "overflow"}      # chains 0 and 2 see all three, chain 1 the first two
    assert rb.make("loop-second-round", cus=304)["n_iter"] == 64 * 306 + 1


@pytest.mark.parametrize("name", rb.NAMES)
def test_emulated_bounds_contain_the_oracle(done, name):
    case, ref, st = done(name)
    valid = ref.hyp_fit >= 0
    np.testing.assert_array_equal(st["valid"], valid)                 # the samples the oracle skips are the ones Kabsch rejects
    rb.check_bounds(name, case, st, ref)
    rb.check_not_vacuous(name, case, st, st["unsure"], rb.eta_of(case, st["T"]))
    # the path the case is built for
    assert st["unsure"] == int(case["unsure"]), (st["unsure"], case["path"])
    assert (st["count"] > rb.CAND_MAX) == (case["path"] == "overflow"), st["count"]
    if ref.best_hyp >= 0:
        assert ref.best_hyp in set(st["survivors"].tolist())
    # the property the case exists for
    if name in rb.UNDECIDED_COUNTS:
        assert (st["n_lo"][valid] < st["n_hi"][valid]).any()
    if name in rb.PARTLY_DEGENERATE:
        assert 0.1 <= 1.0 - valid.mean() <= 0.9, valid.mean()
    if name in rb.DEGENERATE:
        assert not valid.any()
        assert ref.best_hyp == -1 and ref.fitness == 0.0 and ref.inlier_rmse == 0.0 and not ref.inlier_mask.any()
        np.testing.assert_array_equal(ref.transformation, np.eye(4))
    if name == "outlier-dominated-6000":
        assert st["F"] > 100 and ref.fitness > 0.05                   # some clean sample was drawn
    if name == "eta-above-threshold":
        assert (rb.eta_of(case, st["T"])[valid] > case["max_dist"]).all() and st["F"] == 0 and (st["n_lo"] == 0).all()
    if name == "below-fp32-resolution":
        assert (st["n_lo"] == 0).all()                                 # nothing is decidable
    if name == "moment-mixed":
        _, sure = rb.emulate_moment(case, st["T"], st["valid"])
        assert sure.any() and (valid & ~sure).any()                    # provable and unprovable hypotheses side by side
    if name == "threshold-260":
        _, sure = rb.emulate_moment(case, st["T"], st["valid"])
        assert not sure.any()                                          # 3 (4.01 M)^2 > 260^2 on the +-60 m scene: nothing is provable
