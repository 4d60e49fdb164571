"""CPU checks of the coarse pass's dispatch table (tests/match_dispatch_cases.py): the library lists its launcher instantiations
itself (vfm_debug_coarse_kernel_names), and the table must name every one of them.  No device is touched."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from . import match_dispatch_cases as mdc

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def built():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib


def test_every_instantiation_has_a_case(built):
    names = built.coarse_kernel_names()
    assert len(names) == len(set(names)) >= 60 and names == sorted(names)       # unique per instantiation, sorted
    expected = {c.kernel for c in mdc.CASES}
    assert not set(mdc.UNREACHABLE) - set(names), "UNREACHABLE lists a kernel the library does not have"
    assert not set(mdc.UNREACHABLE) & expected, "a kernel with a case is not unreachable"
    missing = set(names) - set(mdc.UNREACHABLE) - expected
    unknown = expected - set(names)
    assert not missing, f"launcher instantiations without a case: {sorted(missing)}"
    assert not unknown, f"cases that expect a kernel the library does not have: {sorted(unknown)}"
    for reason in mdc.UNREACHABLE.values():
        assert reason and "\n" not in reason


def test_read_back_is_empty_before_any_search_and_checks_its_buffer(built):
    import ctypes as C
    import threading
    lib = built.load()
    seen = []
    t = threading.Thread(target=lambda: seen.append(built.last_coarse_kernel()))    # a thread that has launched nothing
    t.start()
    t.join()
    assert seen == [""]
    small = C.create_string_buffer(8)
    assert lib.vfm_debug_coarse_kernel_names(small, len(small)) != 0 and b"buffer" in lib.vfm_last_error()
    assert lib.vfm_debug_last_coarse_kernel(None, 0) != 0


@pytest.mark.parametrize("d,n,m", [(128, 300, 4100), (126, 300, 1300), (768, 2113, 4100)])
def test_data_set_holds_what_it_promises(d, n, m):
    q, b = mdc.make(d, n, m, seed=1)
    q2, b2 = mdc.make(d, n, m, seed=1)
    assert np.array_equal(q, q2) and np.array_equal(b, b2) and q.dtype == b.dtype == np.float32
    qn = q.astype(np.float64) / np.maximum(np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True), 1e-300)
    bn = b.astype(np.float64) / np.maximum(np.linalg.norm(b.astype(np.float64), axis=1, keepdims=True), 1e-300)
    s = qn @ bn.T
    best = s.max(1)
    assert (best[::2] > 0.9).all()                                    # the planted half
    odd = np.ones(n, bool)
    odd[::2] = False
    odd[[7] + list(range(61, 120, 2))] = False                        # the scaled copy and the cluster's queries
    assert (best[odd] < 0.7).all()
    assert np.array_equal(b[700], b[200]) and np.array_equal(b[m - 2], b[330]) and (m - 2) // 128 == (m - 1) // 128 != 330 // 128
    assert s[42].argmax() == 200 and s[46].argmax() == 330 and best[42] > 0.999999
    cluster = [128 * c + 17 for c in range(min(20, (m + 127) // 128 - 1))]
    assert len(cluster) >= 10 and (s[61][cluster] > best[61] - 1e-4).all()      # all of them inside any window
    assert not b[1000].any() and not q[5].any() and best[7] > 0.999999
    assert best[9] == 0.0 and (np.delete(s[9], 1000) < 0).all()
    norms = np.linalg.norm(q, axis=1)
    assert norms[3] > 3 * np.median(norms) and norms[11] < 0.3 * np.median(norms)


def test_refusal_rule_of_the_fused_fp6_kinds():
    f = mdc.mx6_fused_slices_refused
    assert not f(mdc.MX6_HALF_FUSED, mdc.M, (("coarse_slices", 2),)) and not f(mdc.MX6_HALF_FUSED, mdc.M, (("coarse_slices", 4),))
    assert f(mdc.MX6_HALF_FUSED, mdc.M, (("coarse_slices", 5),)) and f(mdc.MX6_FUSED, mdc.M, (("coarse_slices", 1000),))
    assert not f(mdc.HALF_FUSED, mdc.M, (("coarse_slices", 1000),)) and not f(mdc.MX6_HALF_FUSED, mdc.M, (("mx6_tune", 3),))


def test_by_width_choice_of_the_fp6_preparation_is_gone(built):
    """coarse_variant 42 chose between the two preparation forms that prep_once_kernel superseded: refused, by
    either name, and the config is left as it was; the forms it chose between are still selectable."""
    cfg = built.Config()
    for key, value in (("coarse_variant", 42), ("prep_form", 2)):
        with pytest.raises(RuntimeError, match="removed"):
            cfg.set(key, value)
        assert cfg.get("prep_form") == 3
    for variant, form in ((40, 0), (41, 1), (44, 4), (43, 3)):
        assert cfg.set("coarse_variant", variant).get("prep_form") == form
