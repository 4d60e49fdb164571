"""CPU checks of the buffer-contract tooling: the GuardedBuffer helper (tests/guarded.py) sees a one-byte write on either side of its
body, and every entry point that takes a workspace refuses one a byte smaller than its *_workspace_bytes() on the host, before it
enqueues anything (include/vfmreg.h: "scratch is caller-provided and sized by the matching vfm_*_workspace_bytes()")."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.guarded import GUARD_BYTES, GuardedBuffer

ROOT = Path(__file__).resolve().parent.parent
VFM_EINVAL, VFM_EWORKSPACE = -1, -2


def test_guarded_buffer_reports_a_byte_on_either_side():
    g = GuardedBuffer((5, 7), torch.float32, device="cpu", guard=4096, seed=3)
    assert g.guard % 512 == 0 and GUARD_BYTES % 512 == 0 and GUARD_BYTES >= 128 * 768 * 4
    assert g.t.shape == (5, 7) and g.t.dtype == torch.float32
    assert g.t.data_ptr() - g.raw.data_ptr() == 4096
    g.fill_bytes(0xFF)
    assert torch.isnan(g.t).all() and g.intact()
    g.t.fill_(1.0)            # writes to the body are not damage
    assert g.intact()
    # one byte just before the body
    before = g.raw[g.guard - 1].item()
    g.raw[g.guard - 1] = (before + 1) % 256
    chk = g.intact()
    assert not chk and "front guard" in repr(chk) and "offset -1 " in repr(chk)
    g.raw[g.guard - 1] = before
    assert g.intact()
    # one byte just after the body
    after = g.raw[g.guard + g.nbytes].item()
    g.raw[g.guard + g.nbytes] = (after + 1) % 256
    chk = g.intact()
    assert not chk and "back guard" in repr(chk) and "offset +0 " in repr(chk)
    # both at once: both named
    g.raw[g.guard - 1] = (before + 7) % 256
    assert "front guard" in repr(g.intact()) and "back guard" in repr(g.intact())
    g.restore_guards()
    assert g.intact()


def test_guarded_buffer_poison_and_alignment():
    g = GuardedBuffer(3, torch.float64, device="cpu", guard=1024)
    g.poison_guards("nan")
    assert g.intact()
    assert torch.isnan(g.raw[:1024].view(torch.float64)).all() and torch.isnan(g.raw[-1024:].view(torch.float64)).all()
    g.raw[g.guard + g.nbytes + 5] = 0x11
    assert not g.intact()
    i = GuardedBuffer(4, torch.int64, device="cpu", guard=512)
    i.poison_guards("zero")
    assert i.intact() and not i.raw[:512].any()
    with pytest.raises(ValueError):
        i.poison_guards("nan")
    with pytest.raises(ValueError):
        GuardedBuffer(4, torch.int64, device="cpu", guard=500)
    i.set(np.arange(4))
    assert i.numpy().tolist() == [0, 1, 2, 3] and i.intact()
    # two buffers of the same seed carry the same guard bytes, different seeds different ones
    a, b, c = (GuardedBuffer(1, torch.uint8, device="cpu", guard=512, seed=s) for s in (1, 1, 2))
    assert torch.equal(a.front, b.front) and not torch.equal(a.front, c.front)


# ------------------------------------------------------------------------------------------------------------ host-side size checks
@pytest.fixture(scope="module")
def lib():
    subprocess.run([sys.executable, str(ROOT / "vfm-registration_amd" / "build.py")], check=True, stdout=subprocess.DEVNULL)
    from vfmreg import _lib
    return _lib.load()


class _Slots:
    """Device pointers for calls that must be refused on the host.  Without a GPU they are addresses nothing dereferences (a call that
    got as far as a launch fails with VFM_EHIP, not with the refusal the test wants); with one, every pointer is a slot of a real,
    zeroed allocation larger than anything these small shapes address -- so even a missing check could not write outside memory the
    test owns."""
    SLOT = 4 << 20

    def __init__(self, k=24):
        self.buf = torch.zeros(k * self.SLOT, dtype=torch.uint8, device="cuda") if torch.cuda.is_available() else None
        self.base = self.buf.data_ptr() if self.buf is not None else 1 << 40
        self.i = 0

    def __call__(self):
        p = self.base + self.i * self.SLOT
        self.i += 1
        return p


def _refused(lib, rc, what):
    err = lib.vfm_last_error().decode()
    assert rc in (VFM_EINVAL, VFM_EWORKSPACE), f"{what}: a workspace one byte short was not refused on the host ({rc}: {err})"


def test_every_workspace_one_byte_short_is_refused_on_the_host(lib):
    from vfmreg import _lib as L
    p = _Slots()
    n, m = 65, 129
    st = None
    for d in (128, 384, 768):
        for prec in (0, 1):
            need = lib.vfm_match_ip_top1_workspace_bytes(n, m, d, prec)
            if need:
                _refused(lib, lib.vfm_match_ip_top1(p(), n, p(), m, d, prec, p(), p(), p(), need - 1, st), f"ip_top1 d={d} prec={prec}")
                _refused(lib, lib.vfm_match_ip_top1_gated(p(), n, p(), m, d, prec, 0.8, p(), p(), p(), need - 1, st), "ip_top1_gated")
            p.i = 0
        need = lib.vfm_match_search_workspace_bytes(n, m, d)
        ws = need - 1
        _refused(lib, lib.vfm_match_search_prepared(p(), p(), n, p(), p(), m, d, p(), p(), p(), ws, st), f"search_prepared d={d}")
        _refused(lib, lib.vfm_match_search_coarse(p(), n, p(), m, d, p(), ws, st), "search_coarse")
        _refused(lib, lib.vfm_match_search_finish(p(), p(), n, p(), p(), m, d, p(), p(), p(), ws, st), "search_finish")
        _refused(lib, lib.vfm_match_search_coarse_gated(p(), n, p(), m, d, p(), ws, st), "search_coarse_gated")
        _refused(lib, lib.vfm_match_search_finish_gated(p(), p(), n, p(), p(), m, d, p(), p(), p(), ws, 0.8, st), "search_finish_gated")
        for rec in range(11):
            _refused(lib, lib.vfm_match_search_coarse_gated_r(p(), n, p(), m, d, p(), ws, rec, st), f"coarse_gated_r {rec}")
            _refused(lib, lib.vfm_match_search_coarse_gated_g(p(), n, p(), m, d, p(), ws, rec, 0.8, st), f"coarse_gated_g {rec}")
            _refused(lib, lib.vfm_match_search_finish_gated_r(p(), p(), n, p(), p(), m, d, p(), p(), p(), ws, 0.8, rec, st),
                     f"finish_gated_r {rec}")
            _refused(lib, lib.vfm_match_search_finish_gated_t(p(), 0, p(), n, p(), 0, p(), m, d, p(), p(), p(), ws, 0.8, rec, st),
                     f"finish_gated_t {rec}")
            p.i = 0
        out = (C.c_int32 * 1)()
        _refused(lib, lib.vfm_match_search_probe_half(p(), n, p(), m, d, p(), ws, 0.8, C.cast(out, C.c_void_p), st), "probe_half")
        p.i = 0
    for d in (7, 126, 384, 768):
        for prec in (0, 1):
            for mutual in (0, 1):
                need = lib.vfm_match_mutual_l2_workspace_bytes(n, m, d, prec, mutual)
                if need == 0:   # (no workspace: nothing to be short of)
                    continue
                _refused(lib, lib.vfm_match_mutual_l2(p(), n, p(), m, d, prec, p(), p(), p() if mutual else None, p(), need - 1, st),
                         f"mutual_l2 d={d} prec={prec} mutual={mutual}")
                p.i = 0
        need = lib.vfm_match_mutual_pairs_workspace_bytes(n, m, d)
        _refused(lib, lib.vfm_match_mutual_pairs(p(), n, p(), m, d, p(), p(), p(), p(), p(), p(), need - 1, st), f"mutual_pairs d={d}")
        p.i = 0
    for c_max, n_iter in ((3, 50), (1000, 500)):
        need = lib.vfm_ransac_workspace_bytes(c_max, n_iter)
        _refused(lib, lib.vfm_ransac_corr(p(), p(), p(), p(), c_max, 0.5, n_iter, 42, p(), p(), p(), p(), p(), p(), need - 1, st), "ransac")
        _refused(lib, lib.vfm_ransac_corr_bounded(p(), c_max, p(), c_max, p(), p(), c_max, 0.5, n_iter, 42, p(), p(), p(), p(), p(), p(),
                                                  p(), need - 1, st), "ransac_bounded")
        p.i = 0
    mats = (C.c_double * 48)(*([1.0] * 48))
    fc = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    win = (C.c_int64 * 4)(0, 0, 10, 10)
    for mode in (0, 1, 2):
        need = lib.vfm_project_workspace_bytes(n)
        _refused(lib, lib.vfm_project_pinhole_f64(mode, p(), n, C.cast(mats, C.c_void_p), C.cast(fc, C.c_void_p), 1.0,
                                                  C.cast(win, C.c_void_p), p() if mode == 0 else None, 20, 20, p(), p(), p(), p(), p(),
                                                  need - 1, st), f"project mode={mode}")
        p.i = 0
    info = (C.c_int64 * 4)()
    for nn in (1, 513):
        _refused(lib, lib.vfm_voxel_first(p(), nn, 3, 1.0, 1, p(), p(), p(), lib.vfm_voxel_first_workspace_bytes(nn) - 1, st), "voxel_first")
        need = lib.vfm_voxel_robin_workspace_bytes(nn)
        _refused(lib, lib.vfm_voxel_robin(p(), nn, 3, 1.0, 1, 19349663, nn, p(), p(), C.cast(info, C.c_void_p), p(), need - 1, st),
                 "voxel_robin")
        _refused(lib, lib.vfm_voxel_robin_level(p(), 3, None, nn, None, None, 1.0, 19349663, p(), None, p(), p(), p(), need - 1, st),
                 "voxel_robin_level")
        need = lib.vfm_fpfh_workspace_bytes(nn)
        _refused(lib, lib.vfm_fpfh_grid_build(p(), nn, 0.5, p(), p(), p(), need - 1, st), "fpfh_grid_build")
        _refused(lib, lib.vfm_fpfh_voxel_down_sample(p(), p(), nn, 0.1, p(), p(), p(), p(), need - 1, st), "fpfh_voxel_down_sample")
        p.i = 0
    cfg = L.VitConfig(128, 2, 2, 256, 14, 16, 18)
    for B in (1, 3):
        need = lib.vfm_vit_workspace_bytes(C.byref(cfg), B)
        _refused(lib, lib.vfm_vit_forward(C.byref(cfg), p(), p(), B, 700, 820, p(), p(), need - 1, st), f"vit B={B}")
        p.i = 0
