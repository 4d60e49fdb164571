"""The correspondence search on the data the reference actually sends: maps whose every row is a lifted ViT feature
(registration_node.py:562 keeps only rows with a descriptor, prepare_scenes.py:85-104 lifts all of them from the same ViT), so every
row is a near-duplicate of many others and shares a large common component -- hundreds of candidate chunks per query, every query tile
past match_select_best_kernel's LDS staging -- and scans voxelised down to a few hundred / thousand rows (registration_node.py:399-414)
against kept maps of 10^5 - 10^6 rows.  Every comparison is against the oracle on every row: indices and similarities bit for bit,
the gate contract where a gate applies.  Each data set is checked to be in the regime it is meant to test."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from vfmreg import _lib, ops, synth  # noqa: E402
from vfmreg.pipeline import RegistrationPipeline  # noqa: E402

from .test_gpu_int8 import _gate_contract  # noqa: E402
from .test_gpu_mx6 import (HALF_KINDS, PREPARE_MX6, PREPARE_MX6_HALF, RECORDS_MX6, RECORDS_MX6_FUSED, RECORDS_MX6_HALF,  # noqa: E402
                           RECORDS_MX6_HALF_FUSED, RECORDS_MX6_PILOT, RECORDS_MX6_TOP2)

GATE = float(np.nextafter(np.float32(0.8), np.float32(-np.inf)))
# (records, preparation flags): int8 best-score, fp6 best-score, int8 top-2, fp6 top-2, pilot, fused gate, both half-width kinds
KINDS = ((0, PREPARE_MX6), (RECORDS_MX6, PREPARE_MX6), (1, PREPARE_MX6), (RECORDS_MX6_TOP2, PREPARE_MX6), (RECORDS_MX6_PILOT, PREPARE_MX6),
         (RECORDS_MX6_FUSED, PREPARE_MX6), (RECORDS_MX6_HALF, PREPARE_MX6 | PREPARE_MX6_HALF),
         (RECORDS_MX6_HALF_FUSED, PREPARE_MX6 | PREPARE_MX6_HALF))
GATE_ONLY = HALF_KINDS + (RECORDS_MX6_FUSED,)   # kinds whose coarse pass tests the gate itself: they need a finite one
CROWDED_BIN = 9                                 # stats [8 + b]: queries with 2^(b-1) < candidate entries <= 2^b; b >= 9: more than 256


def _search(q, b, gate, records, flags, cfg):
    """The explicit split search (tests/test_gpu_mx6.py::_search) under ``cfg``, with the workspace's counters (vfm_debug_match_stats)."""
    lib = _lib.load()
    n, d = q.shape
    m = b.shape[0]
    with _lib.using(cfg):
        st = torch.cuda.current_stream().cuda_stream
        qb = torch.empty(lib.vfm_match_prepared_bytes(n, d), dtype=torch.uint8, device="cuda")
        bb = torch.empty(lib.vfm_match_prepared_bytes(m, d), dtype=torch.uint8, device="cuda")
        ws = torch.empty(lib.vfm_match_search_workspace_bytes(n, m, d), dtype=torch.uint8, device="cuda")
        idx = torch.empty(n, dtype=torch.int64, device="cuda")
        sim = torch.empty(n, dtype=torch.float32, device="cuda")
        _lib.check(lib.vfm_match_prepare2_gated_p(b.data_ptr(), m, bb.data_ptr(), q.data_ptr(), n, qb.data_ptr(), d, flags, st))
        _lib.check(lib.vfm_match_search_coarse_gated_g(qb.data_ptr(), n, bb.data_ptr(), m, d, ws.data_ptr(), ws.numel(), records, gate, st))
        _lib.check(lib.vfm_match_search_finish_gated_r(q.data_ptr(), qb.data_ptr(), n, b.data_ptr(), bb.data_ptr(), m, d, idx.data_ptr(),
                                                       sim.data_ptr(), ws.data_ptr(), ws.numel(), gate, records, st))
        torch.cuda.synchronize()
        out = (C.c_int32 * 64)()
        _lib.check(lib.vfm_debug_match_stats(ws.data_ptr(), n, m, C.cast(out, C.c_void_p)))
    return idx, sim, list(out)


def _oracle(q, b):
    qn, _ = orc.l2norm_rows(q.cpu().numpy())
    bn, _ = orc.l2norm_rows(b.cpu().numpy())
    return orc.match_ip_top1(qn, bn, block=256)


def _mean_row(b):
    """|mean of the normalised rows| (0 for independent directions, 1 for one direction)"""
    return float(torch.nn.functional.normalize(b.double(), dim=1).mean(0).norm())


def _check_regime(name, b, st, rsim):
    """the data are the crowded regime the test is for: a large common component, and most queries that pass the gate with more than
    256 candidate chunks behind the fp6 best-score pass (the stats of ``st``)"""
    mean = _mean_row(b)
    live = int((rsim >= 0.8).sum())
    nonzero = sum(st[8:24])
    crowded = sum(st[8 + CROWDED_BIN:24])
    print(f"[{name}] |mean of the normalised map rows| {mean:.3f}; {live} queries reach the gate; candidate chunks per query "
          f"{st[2] / max(1, nonzero):.1f}; {crowded} queries with more than 256; all-pairs fallbacks {st[0]}")
    assert mean >= 0.5, mean
    assert crowded > live // 2, (crowded, live, st[8:24])


@pytest.fixture(scope="module")
def c2():
    """C2 size, all lifted, 5 % of the scan rows without a descriptor; the oracle's answers (the ViT is only the data source)"""
    n, m, d = 20000, 200000, 384
    p = synth.make_all_lifted_pair_device(n, m, d, seed=42, zero_rows=0.05)
    ridx, rsim = _oracle(p["q_desc"], p["b_desc"])
    assert int((rsim >= 0.8).sum()) > n // 2
    return p, ridx, rsim


def test_all_lifted_c2_every_record_kind_and_both_preparations_give_the_oracle_answers(c2):
    """20 000 x 200 000 x 384 on all-lifted rows: every record kind (int8 / fp6 best-score, both top-2 kinds, pilot, fused gate, both
    half-width kinds), gate at 0.8 and no gate (the gate-only kinds: gate only), behind both forms of the fp6 preparation
    (prep_stream_kernel, variant 41; prep_once_kernel, 43 = the default).  With ~10^2 candidate chunks per query every query tile
    overflows the selection's LDS staging: the direct placement, the chunk-major rescan and the refinement run their crowded paths."""
    p, ridx, rsim = c2
    q, b = p["q_desc"], p["b_desc"]
    zero = (q == 0).all(dim=1).cpu().numpy()
    assert zero.sum() > 500 and (ridx[zero] == 0).all() and (rsim[zero] == 0).all()
    fallbacks = {}
    for variant in (41, 43):
        cfg = _lib.Config(coarse_variant=variant, match_stats=1)
        for records, flags in KINDS:
            for g in (GATE, float("-inf")):
                if g == float("-inf") and records in GATE_ONLY:
                    continue
                idx, sim, st = _search(q, b, g, records, flags, cfg)
                solved = _gate_contract(idx, sim, ridx, rsim, g)
                assert solved[rsim >= 0.8].all(), (variant, records, g)
                if g == float("-inf"):
                    assert solved.all(), (variant, records)
                fallbacks[(variant, records, g)] = st[0]
                if variant == 43 and records == RECORDS_MX6 and g == GATE:
                    _check_regime("C2 all lifted, fp6 best-score", b, st, rsim)
                if variant == 43 and records == 0 and g == GATE:
                    print(f"[C2 all lifted, int8 best-score] candidate chunks per query {st[2] / max(1, sum(st[8:24])):.1f}; "
                          f"{sum(st[8 + CROWDED_BIN:24])} queries with more than 256")
    print("all-pairs fallbacks per search (variant, records, gate):", fallbacks)


def _scans(p, sizes):
    """consecutive slices of the pair's scan rows: several scans of one map"""
    out, at = [], 0
    for s in sizes:
        out.append((p["q_xyz"][at:at + s], p["q_desc"][at:at + s].contiguous()))
        at += s
    return out


def _pair(data, n, m, seed):
    if data == "D.2":
        return synth.make_pair_device(n, m, 384, seed=seed)
    return synth.make_all_lifted_pair_device(n, m, 384, seed=seed, zero_rows=0.05)


@pytest.mark.parametrize("data", ["D.2", "all lifted"])
@pytest.mark.parametrize("n", [300, 2000])
def test_reference_shaped_scans_against_a_kept_200k_map(data, n):
    """VoxelHashMap.search_device as registration_node.py drives it: a map of 200 000 rows built once with add_points, then searched by
    scans of a few hundred / thousand rows (none a multiple of 32) -- the first search probes the half-width pass, the next ones reuse
    the kept prepared operand, a third runs with the half-width decision flipped (the switch on the search's own load figure), a last
    one is a scan whose rows are all zero.  Every search equals orc.get_vfm_correspondences: pairs, and the gate contract per query."""
    from vfmreg.config import load_config
    from vfmreg.mapping import VoxelHashMap, get_voxel_hash_map
    VoxelHashMap.quiet = True
    m = 200000
    sizes = (n, n, n + 1)
    p = _pair(data, sum(sizes), m, seed=n + 7)
    vm = get_voxel_hash_map(load_config(None, None))
    vm.add_points(np.c_[p["b_xyz"].cpu().numpy(), p["b_desc"].cpu().numpy()].astype(np.float32))
    mp = vm.point_cloud_n()
    assert len(mp) > 0.99 * m
    if data == "all lifted":
        print(f"[{data}, {n} x {len(mp)}] |mean of the normalised map rows| {_mean_row(torch.from_numpy(mp[:, 3:]))}")
        assert _mean_row(torch.from_numpy(mp[:, 3:])) >= 0.5
    scans = _scans(p, sizes)
    scans.append((scans[0][0], torch.zeros_like(scans[0][1])))
    prep = None
    for k, (xyz, desc) in enumerate(scans):
        if k == 2:
            vm._half = not vm._half
        qi, mi, sim = vm.search_device(None, 0.8, q_desc=desc)
        if k == 0:
            prep, probed = vm._prep, vm._half
            print(f"[{data}, {n} x {len(mp)}] the probe chose the {'half' if probed else 'full'}-width pass")
        assert vm._prep is prep                         # prepared once, kept
        _, _, qr, mr, rsim = orc.get_vfm_correspondences(np.c_[xyz.cpu().numpy(), desc.cpu().numpy()], mp, 0.8)
        np.testing.assert_array_equal(qi.cpu().numpy(), qr, err_msg=f"scan {k}")
        np.testing.assert_array_equal(mi.cpu().numpy(), mr, err_msg=f"scan {k}")
        sim = sim.cpu().numpy()
        solved = sim != -2.0
        np.testing.assert_array_equal(sim[solved], rsim[solved], err_msg=f"scan {k}")
        assert (rsim[~solved] < 0.8).all(), k
        if k < 3:
            assert len(qr) > n // 10, (k, len(qr))
        else:
            assert len(qr) == 0 and solved.all()
    if data == "all lifted":
        assert probed is False                          # descriptors that are all alike: no half-width pass


@pytest.mark.parametrize("data", ["D.2", "all lifted"])
def test_reference_shaped_scans_against_a_1m_map_in_the_prepared_operand_form(data):
    """2 000 / 2 001 / all-zero scans against 1 000 000 rows in the form mapping.py's kept map uses (ops.PreparedRows once, the half-width
    probe, ops.match_search_gated with the probed record kind), and every explicit record kind at that shape (fewer than 2 048 queries:
    the fp6 kinds run as their int8 counterparts): oracle answers on every row, gate contract, no gate where the kind allows."""
    n, m = 2000, 1000000
    p = _pair(data, 2 * n + 1, m, seed=11)
    b = p["b_desc"]
    if data == "all lifted":
        print(f"[{data}, {n} x {m}] |mean of the normalised map rows| {_mean_row(b):.3f}")
        assert _mean_row(b) >= 0.5
    bn, _ = orc.l2norm_rows(b.cpu().numpy())
    bp = ops.PreparedRows(b)
    load = torch.zeros(1, dtype=torch.int32).pin_memory()
    scans = [d for _, d in _scans(p, (n, n + 1))]
    scans.append(torch.zeros_like(scans[0]))
    half = None
    cfg = _lib.Config(match_stats=1)
    for k, q in enumerate(scans):
        qn, _ = orc.l2norm_rows(q.cpu().numpy())
        ridx, rsim = orc.match_ip_top1(qn, bn, block=256)
        qp = ops.PreparedRows(q)
        if half is None:
            ops.match_probe_half(qp, bp, GATE, load)
            torch.cuda.current_stream().synchronize()
            half = int(load.item()) <= 24 * q.shape[0]
            print(f"[{data}, {n} x {m}] half-width survivors per query {int(load.item()) / q.shape[0]:.1f}")
        idx, sim = ops.match_search_gated(qp, bp, GATE, records=3 if half else 0, rescans_out=load)
        torch.cuda.synchronize()
        solved = _gate_contract(idx, sim, ridx, rsim, GATE)
        assert solved[rsim >= 0.8].all(), k
        if k == 2:
            assert (ridx == 0).all() and (rsim == 0).all() and solved.all()
            continue
        assert int((rsim >= 0.8).sum()) > n // 10, k
        fallbacks = {}
        for records, flags in KINDS:
            for g in (GATE, float("-inf")):
                if g == float("-inf") and records in GATE_ONLY:
                    continue
                i2, s2, st = _search(q, b, g, records, flags, cfg)
                solved = _gate_contract(i2, s2, ridx, rsim, g)
                assert solved[rsim >= 0.8].all(), (k, records, g)
                if g == float("-inf"):
                    assert solved.all(), (k, records)
                fallbacks[(records, g)] = st[0]
        print(f"[{data}, {q.shape[0]} x {m}] all-pairs fallbacks per search (records, gate): {fallbacks}")


@pytest.mark.parametrize("coarse", ["auto", "int8", "mx6", "mx6-fused", "mx6-half", "fp16", "auto, fp16 map"])
def test_pipeline_on_all_lifted_rows_equals_the_oracle_registration(c2, coarse):
    """RegistrationPipeline at C2 size on all-lifted rows, every coarse mode (and the fp16-rows form once: auto with an fp16 map, whose
    oracle is the search of the widened rows): correspondences, inlier mask, winning hypothesis and pose bit for bit against the
    oracle's registration; four registrations each, so that auto's feedback has moved where it moves."""
    p, ridx, rsim = c2
    n, m, d, iters = 20000, 200000, 384, 3000
    b = p["b_desc"]
    mode = coarse
    if coarse == "auto, fp16 map":
        mode, b = "auto", p["b_desc"].half().contiguous()
        ridx, rsim = _oracle(p["q_desc"], b.float())
    keep = ~(rsim.astype(np.float64) < 0.8)
    corres = np.stack([np.nonzero(keep)[0], ridx[keep]], 1).astype(np.int32)
    ref = orc.ransac_corr(p["q_xyz"].cpu().numpy(), p["b_xyz"].cpu().numpy(), corres, 10000.0, iters, seed=42)
    pipe = RegistrationPipeline(n, m, d, n_iter=iters, overlap_ransac=True, overlap_prepare=True, solve_streams=2, coarse=mode)
    for _ in range(4):
        out = pipe.register(p["q_desc"], p["q_xyz"], b, p["b_xyz"])
        pipe.synchronize()
        torch.cuda.synchronize()
        pipe._poll_feedback()
    c = int(out["count"].item())
    assert c == len(corres) and c > n // 2
    np.testing.assert_array_equal(out["corres"].cpu().numpy()[:c], corres)
    np.testing.assert_array_equal(out["mask"].cpu().numpy()[:c], ref.inlier_mask[:c])
    assert int(out["best_hyp"].item()) == ref.best_hyp
    np.testing.assert_array_equal(out["T"].cpu().numpy(), ref.transformation)
