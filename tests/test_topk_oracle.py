"""CPU checks of the k-best search (include/vfmreg.h, vfm_match_ip_topk): the oracle helper of tests/topk_oracle.py against numpy,
its tie rule, and the entry point's refusals -- all of them made before anything is launched, so they need no GPU."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import topk_oracle

ROOT = Path(__file__).resolve().parent.parent
FAST, EXACT = 0, 1
EINVAL, EWORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib.load()


def test_oracle_equals_numpy_on_separated_scores():
    from oracle import oracle as orc
    for seed in range(100):   # a case whose scores are separated by more than 1e-6: the order cannot hinge on the summation
        rng = np.random.default_rng(seed)
        q, b = rng.standard_normal((7, 16)).astype(np.float32), rng.standard_normal((50, 16)).astype(np.float32)
        qn, _ = orc.l2norm_rows(q)
        bn, _ = orc.l2norm_rows(b)
        s = qn.astype(np.float64) @ bn.astype(np.float64).T
        if np.diff(np.sort(s, axis=1), axis=1).min() > 1e-6:
            break
    else:
        pytest.fail("no separated case among 100 seeds")
    for k in (1, 3, 8):
        idx, sim = topk_oracle.topk(q, b, k)
        want = np.argsort(-s, axis=1, kind="stable")[:, :k]
        np.testing.assert_array_equal(idx, want)
        np.testing.assert_allclose(sim, np.take_along_axis(s, want, 1), rtol=0, atol=1e-6)
        assert idx.dtype == np.int64 and sim.dtype == np.float32


def test_oracle_orders_exact_copies_by_index_and_pads():
    rng = np.random.default_rng(1)
    b = rng.standard_normal((40, 16)).astype(np.float32)
    b[31] = b[5]
    b[17] = b[5]
    q = (b[5] + 0.01 * rng.standard_normal(16)).astype(np.float32)[None]
    idx, sim = topk_oracle.topk(q, b, 4)
    assert idx[0, :3].tolist() == [5, 17, 31] and sim[0, 0] == sim[0, 1] == sim[0, 2] > sim[0, 3]
    # fewer map rows than k: (-1, lowest finite float32) behind the last row; no map rows: nothing else
    idx, sim = topk_oracle.topk(q, b[:2], 5)
    assert sorted(idx[0, :2].tolist()) == [0, 1] and idx[0, 2:].tolist() == [-1] * 3
    assert (sim[0, 2:] == np.finfo(np.float32).min).all() and sim[0, 0] >= sim[0, 1]
    idx, sim = topk_oracle.topk(q, b[:0], 3)
    assert (idx == -1).all() and (sim == np.finfo(np.float32).min).all()
    # a zero query scores 0.0 everywhere: rows 0 .. k-1
    idx, sim = topk_oracle.topk(np.zeros((1, 16), np.float32), b, 3)
    assert idx[0].tolist() == [0, 1, 2] and (sim == 0).all()


def test_abi_refuses_before_any_launch(lib):
    need = lib.vfm_match_ip_topk_workspace_bytes(10, 100, 128, 2, FAST)
    assert need > 0

    def call(n=10, m=100, d=128, k=2, prec=FAST, idx=1, sim=1, ws=1, ws_bytes=need):
        return lib.vfm_match_ip_topk(1, n, 1, m, d, k, prec, idx, sim, None, ws, ws_bytes, None)

    for k in (0, 9, -1):
        assert call(k=k) == EINVAL and b"k must be" in lib.vfm_last_error()
    assert call(idx=None) == EINVAL and b"null output" in lib.vfm_last_error()
    assert call(sim=None) == EINVAL and b"null output" in lib.vfm_last_error()
    assert call(d=0) == EINVAL and b"d must be" in lib.vfm_last_error()
    assert call(prec=7) == EINVAL and b"prec_mode" in lib.vfm_last_error()
    assert call(ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.vfm_last_error()
    need_exact = lib.vfm_match_ip_topk_workspace_bytes(10, 100, 33, 2, EXACT)
    assert call(d=33, prec=EXACT, ws_bytes=need_exact - 1) == EWORKSPACE
    # no queries: success, nothing launched, nothing written (the outputs here are not even memory)
    assert call(n=0) == 0
    assert call(n=0, ws=None, ws_bytes=0) == 0


def test_workspace_size_is_positive_and_grows_with_the_queries(lib):
    for prec, d in ((FAST, 128), (FAST, 384), (EXACT, 33), (FAST, 512), (FAST, 33)):
        sizes = [lib.vfm_match_ip_topk_workspace_bytes(n, 4097, d, 8, prec) for n in (1, 33, 256, 257, 2000, 20000)]
        assert sizes[0] > 0 and sizes == sorted(sizes), (prec, d, sizes)
    # a shape FAST has no kernel for runs EXACT: the same workspace
    assert lib.vfm_match_ip_topk_workspace_bytes(100, 1000, 512, 4, FAST) == lib.vfm_match_ip_topk_workspace_bytes(100, 1000, 512, 4, EXACT)
    assert lib.vfm_match_ip_topk_workspace_bytes(100, 1000, 128, 4, FAST) > lib.vfm_match_ip_topk_workspace_bytes(100, 1000, 128, 4, EXACT)
    assert lib.vfm_match_ip_topk_workspace_bytes(100, 0, 128, 4, FAST) > 0


def test_constants_agree_with_the_header(lib):
    from vfmreg import ops
    text = (ROOT / "include" / "vfmreg.h").read_text()
    assert int(re.search(r"#define\s+VFM_MATCH_TOPK_MAX\s+(\d+)", text).group(1)) == ops.MATCH_TOPK_MAX_K == 8
    assert ops.MATCH_TOPK_RECORD_CAP >= 1024
    src = (ROOT / "vfm-registration_amd" / "csrc" / "match_internal.h").read_text()
    assert int(re.search(r"FILTER_LDS_ROWS\s*=\s*(\d+)", src).group(1)) == ops.MATCH_TOPK_RECORD_CAP


def test_ops_refuse_cpu_tensors(lib):
    import torch
    from vfmreg import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.match_ip_topk(torch.zeros(4, 128), torch.zeros(8, 128), 2)


def test_node_refuses_a_candidate_count_outside_the_range(lib):
    from vfmreg.registration import RegistrationNode
    for k in (0, 9):
        with pytest.raises(ValueError, match="vfm_candidates"):
            RegistrationNode(vfm_candidates=k)
    assert RegistrationNode().vfm_candidates == 1 and RegistrationNode(vfm_candidates=3).vfm_candidates == 3
