"""CPU checks of the policy key "rescore_block" (include/vfmreg.h, vfm_config_set): 64 and 256 are accepted and read back, anything else
is refused and leaves the setting alone (0, what an untouched config reads back: the choice by the plan, included), and the search plan -- FIN_RESCORE is one step whichever form runs it -- reads the same."""
import subprocess
import sys
from pathlib import Path

import pytest

from . import match_dispatch_cases as mdc

ROOT = Path(__file__).resolve().parent.parent
NO_I8 = 0x200


@pytest.fixture(scope="module")
def built():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib


def test_rescore_block_takes_64_and_256_and_reads_them_back(built):
    cfg = built.Config()
    assert cfg.get("rescore_block") == 0                  # untouched: the library chooses by the plan (and 0 itself cannot be set)
    for value in (256, 64, 256):
        assert cfg.set("rescore_block", value).get("rescore_block") == value
    with built.using(built.Config(rescore_block=256)):
        assert built.policy("rescore_block") == 256
    with built.using(built.Config(rescore_block=64)):
        assert built.policy("rescore_block") == 64
    assert built.policy("rescore_block") == built.Config().get("rescore_block")   # the bindings ended with their blocks


@pytest.mark.parametrize("value", [0, 1, -1, 63, 65, 128, 255, 257, 512, 1024, 1 << 40])
def test_other_rescore_block_values_are_refused(built, value):
    cfg = built.Config(rescore_block=256)
    with pytest.raises(RuntimeError, match="rescore_block"):
        cfg.set("rescore_block", value)
    assert cfg.get("rescore_block") == 256


@pytest.mark.parametrize("records,d,n,m,gated", [(mdc.MX6_HALF_FUSED | NO_I8, 384, mdc.N_HI, mdc.M, True),
                                                 (mdc.MX6_HALF_FUSED | NO_I8, 256, mdc.N_HI, mdc.M, True),
                                                 (mdc.MX6_HALF_FUSED, 384, mdc.N_HI, mdc.M, True), (mdc.BEST, 384, mdc.N_HI, mdc.M, True),
                                                 (mdc.TOP2, 768, mdc.N_HI, mdc.M, True), (mdc.BEST, 384, 300, 1500, False)])
def test_the_search_plan_is_the_same_with_either_block(built, records, d, n, m, gated):
    plans = {}
    for block in (64, 256):
        with built.using(built.Config(rescore_block=block)):
            plans[block] = built.search_plan(records, d, n, m, gated)
    assert plans[64] == plans[256]
    assert plans[64]["finish"].count("match_rescore_kernel") == 1
    assert plans[64]["finish"][-2:] == ["match_rescore_kernel", "match_exact_kernel"]
