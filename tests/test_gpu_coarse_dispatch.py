"""Every instantiation of the coarse kernels and every A/B variant the tools select, run once on adversarial data: each case of
tests/match_dispatch_cases.py must launch the kernel the launchers' rules give for it (vfm_debug_last_coarse_kernel) and return the
fp64 oracle's answers; the finish-stage and launch variants must not change an answer."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from vfmreg import _lib, ops  # noqa: E402

from . import match_dispatch_cases as mdc  # noqa: E402

def _dev(x):
    return torch.from_numpy(np.array(x)).cuda()      # (the shared arrays are read-only: a copy goes to the device)


def _search_ip(q, b):
    """ungated: vfm_match_prepare of both sides -> vfm_match_search_coarse -> vfm_match_search_finish"""
    lib = _lib.load()
    n, d = q.shape
    m = b.shape[0]
    Q, B = ops.PreparedRows(q), ops.PreparedRows(b)
    ws = torch.empty(lib.vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device="cuda")
    idx = torch.empty(n, dtype=torch.int64, device="cuda")
    sim = torch.empty(n, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.vfm_match_search_coarse(Q.buf.data_ptr(), n, B.buf.data_ptr(), m, d, ws.data_ptr(), ws.numel(), st))
    kernel = _lib.last_coarse_kernel()
    _lib.check(lib.vfm_match_search_finish(q.data_ptr(), Q.buf.data_ptr(), n, b.data_ptr(), B.buf.data_ptr(), m, d, idx.data_ptr(),
                                           sim.data_ptr(), ws.data_ptr(), ws.numel(), st))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sim.cpu().numpy(), kernel


class Gated:
    """The gated family as the pipeline calls it: vfm_match_prepare2_gated_p (with the fp6 image for the fp6 kinds) once, then
    vfm_match_search_coarse_gated_g -> vfm_match_search_finish_gated_r as often as asked, on one workspace."""

    def __init__(self, q, b, records):
        lib = _lib.load()
        self.q, self.b, self.records = q, b, records
        self.n, self.d = q.shape
        self.m = b.shape[0]
        n, m, d = self.n, self.m, self.d
        self.qb = torch.empty(lib.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device="cuda")
        self.bb = torch.empty(lib.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device="cuda")
        self.ws = torch.empty(lib.vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device="cuda")
        self.prepare()

    def prepare(self):
        lib = _lib.load()
        flags = mdc.PREPARE_MX6 if self.records in mdc.MX6_KINDS else 0
        _lib.check(lib.vfm_match_prepare2_gated_p(self.b.data_ptr(), self.m, self.bb.data_ptr(), self.q.data_ptr(), self.n, self.qb.data_ptr(),
                                                  self.d, flags, torch.cuda.current_stream().cuda_stream))

    def search(self, gate=mdc.GATE):
        lib = _lib.load()
        n, m, d = self.n, self.m, self.d
        idx = torch.empty(n, dtype=torch.int64, device="cuda")
        sim = torch.empty(n, dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.vfm_match_search_coarse_gated_g(self.qb.data_ptr(), n, self.bb.data_ptr(), m, d, self.ws.data_ptr(), self.ws.numel(),
                                                       self.records, gate, st))
        kernel = _lib.last_coarse_kernel()
        _lib.check(lib.vfm_match_search_finish_gated_r(self.q.data_ptr(), self.qb.data_ptr(), n, self.b.data_ptr(), self.bb.data_ptr(), m, d,
                                                       idx.data_ptr(), sim.data_ptr(), self.ws.data_ptr(), self.ws.numel(), gate,
                                                       self.records, st))
        torch.cuda.synchronize()
        return idx.cpu().numpy(), sim.cpu().numpy(), kernel


def _assert_gate_contract(idx, sim, ridx, rsim, what):
    """every query at or above the gate is solved with the oracle's index and similarity, bit for bit; an unsolved query comes back as
    (-1, -2.0) and is below the gate in the oracle; the planted half is there"""
    solved = idx >= 0
    np.testing.assert_array_equal(idx[solved], ridx[solved], err_msg=what)
    np.testing.assert_array_equal(sim[solved], rsim[solved], err_msg=what)
    assert (rsim[~solved] < mdc.GATE).all(), what
    assert (sim[~solved] == -2.0).all(), what
    assert solved[rsim >= mdc.GATE].all(), what
    assert solved.mean() > 0.4, (what, solved.mean())
    return solved


@pytest.mark.parametrize("case", mdc.CASES, ids=[c.id for c in mdc.CASES])
def test_case_runs_its_kernel_and_gives_the_oracle_answers(case):
    before = _lib.current()
    with _lib.using(_lib.Config(**dict(case.cfg))):
        if case.entry == "l2":
            a, b, i_ref, dist_ref, j_ref = mdc.data_l2(case.d, case.n, case.m)
            nn_ab, d2, nn_ba = ops.match_mutual_l2(_dev(a), _dev(b), prec=ops.FAST)
            torch.cuda.synchronize()
            kernel = _lib.last_coarse_kernel()
            assert kernel == case.kernel
            np.testing.assert_array_equal(nn_ab.cpu().numpy(), i_ref)
            np.testing.assert_array_equal(nn_ba.cpu().numpy(), j_ref)
            np.testing.assert_array_equal(np.sqrt(d2.cpu().numpy()), dist_ref)
            return
        q, b, ridx, rsim = mdc.data_ip(case.d, case.n, case.m)
        if case.entry == "ip":
            idx, sim, kernel = _search_ip(_dev(q), _dev(b))
            assert kernel == case.kernel
            assert _lib.coarse_plan(case.records, case.d, case.n, case.m, gated=False, compute_units=0)["kernel"] == kernel
            np.testing.assert_array_equal(idx, ridx)
            np.testing.assert_array_equal(sim, rsim)
        else:
            idx, sim, kernel = Gated(_dev(q), _dev(b), case.records).search()
            assert kernel == case.kernel
            assert _lib.coarse_plan(case.records, case.d, case.n, case.m, gated=True, compute_units=0)["kernel"] == kernel
            _assert_gate_contract(idx, sim, ridx, rsim, case.id)
    assert _lib.current() is before     # the block's config is unbound again


@pytest.mark.parametrize("case", mdc.PADDING_CASES, ids=[c.id for c in mdc.PADDING_CASES])
def test_fused_kinds_rescan_their_bins_where_padding_adds_a_chunk(case):
    """n between four times the chunks that hold rows and four times the padded chunk count: the coarse pass runs the fused kernel, and
    the finish stage must read the bins that kernel filled -- the gate contract, and the planted half solved."""
    q, b, ridx, rsim = mdc.data_ip_large(case.d, case.n, case.m)
    idx, sim, kernel = Gated(_dev(q), _dev(b), case.records).search()
    assert kernel == case.kernel
    _assert_gate_contract(idx, sim, ridx, rsim, case.id)


@pytest.mark.parametrize("cfg", mdc.VARIANT_CONFIGS, ids=["-".join(f"{k}={v}" for k, v in c) for c in mdc.VARIANT_CONFIGS])
def test_finish_and_launch_variants_change_no_answer(cfg):
    """the general select kernel / no chunk-major rescan (20 / 21), both forms of the chunk-major rescan (50 / 51, 60 / 61), forced slice
    counts (1000 is clamped to the 34 chunks) and the fp6 kernel's tuning bits: index, similarity and solved flag of every query as
    under the default config and as in the oracle.  A fused fp6 search refuses a slice count its survivor slots cannot hold, before it
    launches anything; the workspace then serves the next default search as before."""
    for d, n, m, records in mdc.VARIANT_WORKLOADS:
        what = f"d={d} n={n} records={records} {cfg}"
        q, b, ridx, rsim = mdc.data_ip(d, n, m)
        run = Gated(_dev(q), _dev(b), records)
        idx0, sim0, kernel0 = run.search()
        _assert_gate_contract(idx0, sim0, ridx, rsim, what + " (default)")
        with _lib.using(_lib.Config(**dict(cfg))):
            if mdc.mx6_fused_slices_refused(records, m, cfg):
                with pytest.raises(RuntimeError, match="survivor slots"):
                    run.search()
                idx, sim = None, None
            else:
                run.prepare()      # (the preparation reads the thread's config too)
                idx, sim, _ = run.search()
        if idx is None:
            idx, sim, kernel = run.search()          # default config again, same workspace
            assert kernel == kernel0
        _assert_gate_contract(idx, sim, ridx, rsim, what)
        np.testing.assert_array_equal(idx, idx0, err_msg=what)
        np.testing.assert_array_equal(sim, sim0, err_msg=what)
