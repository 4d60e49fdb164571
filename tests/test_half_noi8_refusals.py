"""CPU checks of VFM_PREPARE_NO_I8 / VFM_RECORDS_NO_I8 (include/vfmreg.h): every combination the header rules out is refused on the host,
before anything is launched -- such operands would be searched through an int8 image that was never written."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MX6, MX6_HALF, NO_I8_PREP = 8, 16, 32
KIND, NO_I8 = 8, 0x200
BIG = 1 << 60   # "workspace bytes": the size check passes, nothing is ever dereferenced


@pytest.fixture(scope="module")
def lib():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib.load()


@pytest.mark.parametrize("schedule,d", [(NO_I8_PREP, 384), (MX6 | NO_I8_PREP, 384), (MX6_HALF | NO_I8_PREP, 384), (1 | NO_I8_PREP, 256),
                                        (MX6 | MX6_HALF | NO_I8_PREP, 512), (MX6 | MX6_HALF | NO_I8_PREP, 768),
                                        (MX6 | MX6_HALF | NO_I8_PREP, 128), (MX6 | MX6_HALF | NO_I8_PREP | 64, 384)])
def test_the_preparation_flag_needs_the_half_width_fp6_image_at_d_256_or_384(lib, schedule, d):
    assert lib.vfm_match_prepare2_gated_p(1, 4096, 1, 1, 2100, 1, d, schedule, None) != 0
    assert b"prepare2" in lib.vfm_last_error()
    assert lib.vfm_match_prepare2_gated_z(1, 4096, 1, 1, 2100, 1, d, schedule, 1, BIG, 2100, 4096, None) != 0
    assert b"prepare2" in lib.vfm_last_error()


@pytest.mark.parametrize("d", [256, 384])
def test_the_entry_for_typed_rows_refuses_the_flag(lib, d):
    for dt1, dt2 in ((0, 0), (1, 1), (0, 1)):
        assert lib.vfm_match_prepare2_gated_t(1, dt1, 4096, 1, 1, dt2, 2100, 1, d, MX6 | MX6_HALF | NO_I8_PREP, None) != 0
        assert b"VFM_PREPARE_NO_I8" in lib.vfm_last_error()


# (records, n, m, d): another kind; 2048 queries or fewer; fewer than four queries per map chunk; widths without the fp6 rescan
REFUSED = [(7 | NO_I8, 2100, 4096, 384), (5 | NO_I8, 2100, 4096, 384), (0 | NO_I8, 2100, 4096, 384), (4 | NO_I8, 2100, 4096, 384),
           (10 | NO_I8, 2100, 4096, 256), (KIND | NO_I8, 2048, 4096, 384), (KIND | NO_I8, 2100, 200000, 384), (KIND | NO_I8, 3000, 4096, 512),
           (KIND | NO_I8, 3000, 4096, 768), (KIND | NO_I8, 3000, 4096, 128), (KIND | NO_I8, 3000, 4096, 640)]


@pytest.mark.parametrize("records,n,m,d", REFUSED)
def test_the_option_bit_is_refused_where_the_search_would_not_run_as_kind_8(lib, records, n, m, d):
    assert lib.vfm_match_search_coarse_gated_g(1, n, 1, m, d, 1, BIG, records, 0.8, None) != 0
    assert b"VFM_RECORDS_NO_I8" in lib.vfm_last_error()
    assert lib.vfm_match_search_coarse_gated_g(1, n, 1, m, d, 1, BIG, records | 0x100, 0.8, None) != 0   # (with VFM_RECORDS_WS_CLEAN beside it)
    assert b"VFM_RECORDS_NO_I8" in lib.vfm_last_error()
    assert lib.vfm_match_search_finish_gated_r(1, 1, n, 1, 1, m, d, 1, 1, 1, BIG, 0.8, records, None) != 0
    assert b"VFM_RECORDS_NO_I8" in lib.vfm_last_error()


def test_the_option_bit_is_no_kind_and_goes_to_no_other_entry(lib):
    assert lib.vfm_match_search_coarse_gated_g(1, 2100, 1, 4096, 384, 1, BIG, NO_I8 | 11, 0.8, None) != 0
    assert b"unknown record kind" in lib.vfm_last_error()
    assert lib.vfm_match_search_coarse_gated_r(1, 2100, 1, 4096, 384, 1, BIG, KIND | NO_I8, None) != 0
    assert b"unknown record kind" in lib.vfm_last_error()
    assert lib.vfm_match_search_finish_gated_t(1, 0, 1, 2100, 1, 0, 1, 4096, 384, 1, 1, 1, BIG, 0.8, KIND | NO_I8, None) != 0
    assert b"unknown record kind" in lib.vfm_last_error()
    # a finite gate, as for every half-width kind
    assert lib.vfm_match_search_finish_gated_r(1, 1, 2100, 1, 1, 4096, 384, 1, 1, 1, BIG, float("-inf"), KIND | NO_I8, None) != 0
    assert b"finite gate" in lib.vfm_last_error()
    assert lib.vfm_match_search_coarse_gated_g(1, 2100, 1, 4096, 384, 1, BIG, KIND | NO_I8, float("-inf"), None) != 0
    assert b"finite gate" in lib.vfm_last_error()


def test_the_policy_key(lib):
    from vfmreg import _lib
    assert _lib.policy("half_noi8") == 1
    cfg = _lib.Config(half_noi8=0)
    assert cfg.get("half_noi8") == 0
    with _lib.using(cfg):
        assert _lib.policy("half_noi8") == 0
    assert _lib.policy("half_noi8") == 1
