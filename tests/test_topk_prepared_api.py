"""CPU checks of the k-best search on prepared operands (include/vfmreg.h, vfm_match_ip_topk_prepared) and of the widths the k-best
search has a matrix-core kernel for: the entry point's refusals -- all of them made before anything is launched, so they need no GPU --
and the workspace sizes, in the manner of tests/test_topk_oracle.py."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FAST, EXACT = 0, 1
EINVAL, EWORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib.load()


def test_prepared_abi_refuses_before_any_launch(lib):
    need = lib.vfm_match_ip_topk_prepared_workspace_bytes(10, 128, 2)
    assert need > 0

    # (the operands and outputs here are not even memory: every refusal comes before anything is read or launched)
    def call(q=1, qp=1, n=10, b=1, bp=1, m=100, d=128, k=2, idx=1, sim=1, ws=1, ws_bytes=need):
        return lib.vfm_match_ip_topk_prepared(q, qp, n, b, bp, m, d, k, idx, sim, None, ws, ws_bytes, None)

    for k in (0, 9, -1):
        assert call(k=k) == EINVAL and b"k must be" in lib.vfm_last_error()
    assert call(idx=None) == EINVAL and b"null output" in lib.vfm_last_error()
    assert call(sim=None) == EINVAL and b"null output" in lib.vfm_last_error()
    for operand in ("q", "qp", "b", "bp"):
        assert call(**{operand: None}) == EINVAL and b"null operand" in lib.vfm_last_error(), operand
    # a shape FAST has no kernel for is refused -- no all-pairs fallback on a prepared image
    for d in (512, 33, 0):
        assert call(d=d) == EINVAL and b"no kernel for this shape" in lib.vfm_last_error(), d
    assert call(m=0) == EINVAL and b"no kernel for this shape" in lib.vfm_last_error()
    assert call(m=(1 << 24) + 1) == EINVAL and b"no kernel for this shape" in lib.vfm_last_error()
    for d in (128, 256, 384, 640, 768):
        need_d = lib.vfm_match_ip_topk_prepared_workspace_bytes(10, d, 2)
        assert call(d=d, ws_bytes=need_d - 1) == EWORKSPACE and b"workspace" in lib.vfm_last_error(), d
    assert call(ws=None) == EWORKSPACE
    # no queries: success, nothing launched, nothing written
    assert call(n=0) == 0
    assert call(n=0, ws=None, ws_bytes=0) == 0
    assert call(n=0, d=512, ws=None, ws_bytes=0) == EINVAL


def test_prepared_workspace_size(lib):
    for d in (128, 256, 384, 640, 768):
        sizes = [lib.vfm_match_ip_topk_prepared_workspace_bytes(n, d, 8) for n in (1, 33, 256, 257, 2000, 20000)]
        assert sizes[0] > 0 and sizes == sorted(sizes), (d, sizes)
        # the records alone: the unprepared call's workspace holds both operands' images besides
        prepared = lib.vfm_match_prepared_bytes(257, d) + lib.vfm_match_prepared_bytes(4097, d)
        assert lib.vfm_match_ip_topk_workspace_bytes(257, 4097, d, 8, FAST) == prepared + sizes[3]
    # 0 for arguments the call would refuse
    for n, d, k in ((10, 512, 2), (10, 33, 2), (10, 0, 2), (10, 128, 0), (10, 128, 9), (-1, 128, 2)):
        assert lib.vfm_match_ip_topk_prepared_workspace_bytes(n, d, k) == 0, (n, d, k)


def test_wide_widths_have_the_fast_workspace_and_512_does_not(lib):
    for d in (640, 768):
        assert lib.vfm_match_ip_topk_workspace_bytes(100, 1000, d, 4, FAST) > lib.vfm_match_ip_topk_workspace_bytes(100, 1000, d, 4, EXACT)
    assert lib.vfm_match_ip_topk_workspace_bytes(100, 1000, 512, 4, FAST) == lib.vfm_match_ip_topk_workspace_bytes(100, 1000, 512, 4, EXACT)


def test_header_declares_both_functions(lib):
    text = (ROOT / "include" / "vfmreg.h").read_text()
    assert re.search(r"size_t\s+vfm_match_ip_topk_prepared_workspace_bytes\s*\(\s*int64_t n,\s*int d,\s*int k\s*\)\s*;", text)
    assert re.search(r"int\s+vfm_match_ip_topk_prepared\s*\(\s*const float \*q,\s*const void \*q_prepared,\s*int64_t n,", text)
    assert hasattr(lib, "vfm_match_ip_topk_prepared") and hasattr(lib, "vfm_match_ip_topk_prepared_workspace_bytes")


def test_ops_refuse_widths_without_a_kernel(lib):
    from vfmreg import ops
    assert ops.MATCH_TOPK_FAST_WIDTHS == (128, 256, 384, 640, 768)

    class Rows:   # (what match_ip_topk_prepared looks at before it touches the device)
        def __init__(self, rows, d):
            self.rows, self.d = rows, d

    for dq, db in ((512, 512), (33, 33), (128, 384)):
        with pytest.raises(ValueError, match="Invalid shape"):
            ops.match_ip_topk_prepared(Rows(4, dq), Rows(8, db), 2)
    with pytest.raises(ValueError, match="k must be"):
        ops.match_ip_topk_prepared(Rows(4, 128), Rows(8, 128), 9)
