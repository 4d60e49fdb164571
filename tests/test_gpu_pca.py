"""csrc/pca.hip and what stands on it (vfmreg.pca, ImageFeatureGenerator.run_pca, utils.colour_gate / filter_map_semantic,
evaluate_scene(cluster_removal_prob=...)) against tests/pca_oracle.py.

What is exact is compared bit for bit: the scatter of integer data, and everything behind a GIVEN fit -- projection in the contract's
order of addition, extremes, zero-row flags, normalised values, colours, the gate, the filter.  What passes through an eigen-solve is
held to bounds computed here from the data (pca_oracle.scatter_bound / fit_bound / colour_delta: derived, not measured).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import pca_oracle as po  # noqa: E402
from tests.guarded import GuardedBuffer  # noqa: E402
from tests.test_pca_oracle import E2E_SEED, E2E_SHAPE, data  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS_F32, ROWS_F16 = 0, 1


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the shared data are read-only)


def _moments(X):
    from vfmreg import ops
    mean, S = ops.pca_moments(_dev(X))
    return mean.cpu().numpy(), S.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else a.dtype)


# ---------------------------------------------------------------------------------------------------------------------- moments
def _integer_rows(seed, n, d):
    """integers in [-8, 8], every row followed by its negation: the mean is exactly 0 and the scatter exactly integral"""
    half = np.random.RandomState(seed).randint(-8, 9, size=(n // 2, d))
    X = np.empty((n, d), dtype=np.float32)
    X[0::2], X[1::2] = half, -half
    return X


@pytest.mark.parametrize("d", [1, 3, 16, 17, 100, 384, 768])
def test_moments_of_integer_rows_are_exact(d):
    for n in (2, 6, 126, 130, 1002, 10006):      # off the multiple of 4, around a slab's edge, fewer rows than slabs
        X = _integer_rows(1000 * d + n, n, d)
        mean, S = _moments(X)
        ref = X.astype(np.float64).T @ X.astype(np.float64)
        assert not mean.any(), (n, d)
        assert np.array_equal(_bits(S), _bits(ref)), (n, d, np.argwhere(S != ref)[:4])


def test_moments_of_both_row_types_agree():
    X = _integer_rows(5, 130, 100)
    for rows in (X, X.astype(np.float16)):
        mean, S = _moments(rows)
        assert not mean.any() and np.array_equal(S, X.astype(np.float64).T @ X.astype(np.float64))
    H = data(1, 1000, 17).astype(np.float16)                 # general values: float16 rows equal their widened float32 rows
    a, b = _moments(H), _moments(H.astype(np.float32))
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("seed,shape", [(E2E_SEED, E2E_SHAPE), (1, (1000, 17))])
def test_moments_within_the_dot_product_bound_symmetric_and_reproducible(seed, shape):
    from vfmreg import _lib
    X = data(seed, *shape)
    mean, S = _moments(X)
    ref_mean, ref_S = po.moments(X)
    excess = np.abs(S - ref_S) / po.scatter_bound(ref_S, len(X))
    print(f"{shape}: max |S - S_ref| / bound = {excess.max():.3g}, max |mean - ref| = {np.abs(mean - ref_mean).max():.3g}")
    assert excess.max() <= 1.0
    assert np.abs(mean - ref_mean).max() <= 2 * len(X) * po.U * np.abs(X).max()      # (n u max|x| for each of the two sums)
    assert np.array_equal(_bits(S), _bits(S.T.copy()))
    again = _moments(X)
    assert np.array_equal(_bits(again[0]), _bits(mean)) and np.array_equal(_bits(again[1]), _bits(S))
    with _lib.using(_lib.Config(coarse_variant=4, ransac_exact_only=1)):
        other = _moments(X)
    assert np.array_equal(_bits(other[0]), _bits(mean)) and np.array_equal(_bits(other[1]), _bits(S))


def test_fit_within_davis_kahan_of_the_oracle():
    from vfmreg import pca
    X = data(E2E_SEED, *E2E_SHAPE)
    f = pca.fit(X, 3)
    ref_mean, ref_S = po.moments(X)
    comps, sv, w = po.fit_from_scatter(ref_S, 3)
    bound = po.fit_bound(ref_S, len(X), 3)
    print(f"fit: max |components - oracle| = {np.abs(f.components_ - comps).max():.3g}, bound {bound:.3g}")
    assert f.components_.shape == (3, X.shape[1]) and f.n_samples_ == len(X)
    assert np.abs(f.components_ - comps).max() <= bound
    assert all(row[np.argmax(np.abs(row))] > 0 for row in f.components_)
    assert np.abs(f.singular_values_ / sv - 1).max() <= bound
    assert np.array_equal(f.mean_, _moments(X)[0])


# ------------------------------------------------------------------------------------------------------------------- projection
def _projection_rows(d, n):
    rng = np.random.RandomState(7 * d + n)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[rng.rand(n, d) < 0.1] = -0.0
    if n > 2:
        X[1] = 0.0
        X[n // 2] = -0.0          # compares equal to zero: a row without features
    return X


def _product_chain(X, mean, comps):
    from vfmreg import ops
    y, zero, lo, hi = ops.pca_project(_dev(X), _dev(mean), _dev(comps))
    values = ops.pca_colours(y, None, lo, hi, rgb=False)
    rgb = ops.pca_colours(y, zero, lo, hi, rgb=True).cpu().numpy() if len(comps) == 3 else None
    return y.cpu().numpy(), zero.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy(), values.cpu().numpy(), rgb


def _check_chain(X, mean, comps):
    y, zero, lo, hi, values, rgb = _product_chain(X, mean, comps)
    X64 = X.astype(np.float64)
    Y = po.project_ordered(X64, mean, comps)
    where = (X.shape, len(comps), X.dtype)
    assert np.array_equal(_bits(y), _bits(Y)), where
    assert np.array_equal(_bits(lo), _bits(Y.min(0))) and np.array_equal(_bits(hi), _bits(Y.max(0))), where
    assert np.array_equal(zero.astype(bool), po.zero_rows(X)), where
    want = po.normalise(Y).astype(np.float32)
    assert np.array_equal(np.isnan(values), np.isnan(want)), where
    assert np.array_equal(_bits(values)[~np.isnan(want)], _bits(want)[~np.isnan(want)]), where
    if rgb is not None:
        assert np.array_equal(rgb, po.colours(Y, X)), where
    return want, rgb


@pytest.mark.parametrize("d", [1, 3, 63, 64, 65, 384, 768])
def test_projection_behind_a_given_fit_is_exact(d):
    mean, comps, _ = po.fit(_projection_rows(d, 1000), min(8, d))       # the ORACLE's fit, handed to both sides
    for k in (1, 2, 3, 8):
        if k > d:
            continue
        for n in (1, 2, 65, 1000):
            c = comps[:k].copy()
            values, rgb = _check_chain(_projection_rows(d, n), mean, c)
            if k >= 2:
                c[1] = 0.0                                              # a constant component: NaN as a value, 0 as a colour
                values, rgb = _check_chain(_projection_rows(d, n), mean, c)
                assert np.isnan(values[:, 1]).all() and (rgb is None or not rgb[:, 1].any())
    if d == 384:
        _check_chain(_projection_rows(d, 1000).astype(np.float16), mean, comps[:3].copy())


# -------------------------------------------------------------------------------------------------------------------- end to end
def test_run_pca_end_to_end():
    from vfmreg import pca
    from vfmreg.image_features import ImageFeatureGenerator
    X = data(E2E_SEED, *E2E_SHAPE)
    ref_mean, ref_S = po.moments(X)
    comps, _, _ = po.fit_from_scatter(ref_S, 3)
    Y = po.project_ordered(X, ref_mean, comps)
    want = po.colours(Y, X)
    delta = po.colour_delta(X, ref_mean, ref_S, Y, 3)
    exempt = po.near_integer(po.normalise(Y) * 255.0, delta)
    gen = ImageFeatureGenerator("dinov2", use_featup=False)
    assert gen.fit_pca == {}
    got = gen.run_pca(X, n_components=3)
    assert got.dtype == np.uint8 and got.shape == want.shape
    differ = got != want
    print(f"run_pca: delta = {delta:.3g}, exempt {exempt.mean():.3%}, differing {differ.sum()} of {differ.size}")
    assert exempt.mean() <= 0.01
    assert not (differ & ~exempt).any()
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    # fitted once, kept per n_components
    first = gen.fit_pca[3]
    assert gen._pca.fits_computed == 1 and isinstance(first, pca.PCAFit)
    assert np.array_equal(gen.run_pca(X[:100]), pca.colours(X[:100], first)) and gen.fit_pca[3] is first and gen._pca.fits_computed == 1
    five = gen.run_pca(X, n_components=5)
    assert five.dtype == np.float32 and five.shape == (len(X), 5) and set(gen.fit_pca) == {3, 5} and gen._pca.fits_computed == 2
    m5, c5 = gen.fit_pca[5].mean_, gen.fit_pca[5].components_
    assert np.array_equal(_bits(five), _bits(po.normalise(po.project_ordered(X, m5, c5)).astype(np.float32)))
    # the reference's quirk: after refit_pca the entry is None and stays None, and every later call fits again (IF:170-178)
    part = gen.run_pca(X[:2000], refit_pca=True)
    assert gen.fit_pca[3] is None and gen._pca.fits_computed == 3
    assert part.shape == (2000, 3)
    gen.run_pca(X[:2000])
    assert gen.fit_pca[3] is None and gen._pca.fits_computed == 4
    # a fit from elsewhere: anything with mean_ and components_, numpy or torch
    class Foreign:
        mean_ = torch.from_numpy(ref_mean).reshape(1, -1)
        components_ = torch.from_numpy(comps)
    gen.fit_pca[3] = Foreign()
    assert np.array_equal(gen.run_pca(X), want) and gen._pca.fits_computed == 4
    dev = gen.run_pca(_dev(X))                                    # device tensors in, device tensors out
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)


def test_fit_pca_file_round_trip(tmp_path):
    from vfmreg import pca
    X = data(1, 1000, 17)
    path = tmp_path / "fits" / "pca_fit.npz"
    a = pca.DescriptorPCA(path)
    rgb = a.run_pca(X)
    assert path.exists()
    b = pca.DescriptorPCA(path)
    assert np.array_equal(b.fit_pca[3].components_, a.fit_pca[3].components_) and b.fit_pca[3].n_samples_ == 1000
    assert np.array_equal(b.run_pca(X), rgb) and b.fits_computed == 0
    none = pca.DescriptorPCA()
    none.run_pca(X)
    assert none.fit_pca_file is None and list(tmp_path.iterdir()) == [tmp_path / "fits"]


def test_get_image_features_pca():
    from vfmreg.image_features import ImageFeatureGenerator
    rng = np.random.RandomState(3)
    image = rng.randint(1, 256, size=(112, 154, 3)).astype(np.uint8)
    gen = ImageFeatureGenerator("dinov2", use_featup=False)
    features, rgb = gen.get_image_features_pca(image)
    assert np.allclose(features, gen.get_image_features(image), rtol=1e-4, atol=1e-4)
    rows = features.reshape(-1, features.shape[-1])
    f = gen.fit_pca[3]
    v = po.normalise(po.project_ordered(rows, f.mean_, f.components_)).astype(np.float32)
    assert rgb.dtype == np.uint8 and rgb.shape == features.shape[:2] + (3,)
    assert np.array_equal(rgb.reshape(-1, 3), (v * np.float32(255.0)).astype(np.uint8))      # no blacking here (IF:156-158)
    four = gen.get_image_features_pca(image, n_components=4)[1]
    assert four.dtype == np.float32 and four.shape == features.shape[:2] + (4,) and four.min() == 0.0 and four.max() == 1.0
    up_features, up_rgb = gen.get_image_features_pca(image, upsample=True)
    assert np.allclose(up_features, gen.get_image_features(image, upsample=True), rtol=1e-4, atol=1e-4)
    assert up_rgb.dtype == np.uint8 and up_rgb.shape == (112, 154, 3)
    # the upsampled colours are the bilinear upsample of the normalised values, times 255 (IF:143-158)
    import torch.nn.functional as F
    ref = F.interpolate(torch.from_numpy(v.reshape(features.shape[:2] + (3,))).permute(2, 0, 1)[None], (112, 154), mode="bilinear",
                        align_corners=False)[0].permute(1, 2, 0).numpy() * 255.0
    assert np.abs(up_rgb.astype(np.float64) - np.floor(ref)).max() <= 1       # (a value within rounding of an integer may truncate either way)
    assert (up_rgb == np.floor(ref)).mean() >= 0.99


# -------------------------------------------------------------------------------------------------------------------------- gate
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 5000])
def test_colour_gate(n):
    from vfmreg import utils
    rng = np.random.RandomState(n)
    colour = np.array([100., 100., 100.])
    rows = np.clip(colour + rng.randint(-60, 61, size=(n, 3)), 0, 255).astype(np.uint8)
    if n >= 255:
        at = rng.permutation(n)[:8]
        rows[at] = np.concatenate([colour + po.BOUNDARY_OFFSETS, colour - po.BOUNDARY_OFFSETS]).astype(np.uint8)
        rows[n - 1] = (colour + po.BOUNDARY_OFFSETS[1]).astype(np.uint8)       # the last row, inside
        inside = po.gate(rows, [colour])
        assert np.isin(at[[0, 1, 4, 5]], inside).all() and not np.isin(at[[2, 3, 6, 7]], inside).any() and inside[-1] == n - 1
    for remove_class in ([colour], [colour, colour + [20, 0, 0]], np.float32([[131.5, 90.25, 77], [0, 0, 0], [100, 100, 100]])):
        got = utils.colour_gate(rows, remove_class)
        want = po.gate(rows, remove_class)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, remove_class)
    assert np.array_equal(utils.colour_gate(_dev(rows), [colour], radius=30.5), po.gate(rows, [colour], radius=30.5))
    if n == 5000:
        two = utils.colour_gate(rows, [colour, colour + [20, 0, 0]])
        assert len(np.unique(two)) < len(two)                                   # a row near both colours appears twice


# ------------------------------------------------------------------------------------------------------------ the semantic filter
D_MAP = 128


def _semantic_scene():
    """A ground sheet and four blobs whose descriptors cluster around a second direction; two scans cut from it."""
    rng = np.random.RandomState(11)
    gx, gy = np.meshgrid(np.arange(40) * 0.3 - 6.0, np.arange(40) * 0.3 - 6.0, indexing="ij")
    ground = np.c_[gx.ravel(), gy.ravel(), np.zeros(1600)]
    centres = np.array([[-3., -3., 2.5], [-3., 3., 2.5], [3., -3., 2.5], [3., 3., 2.5]])
    blobs = np.concatenate([c + rng.standard_normal((450, 3)) * [0.5, 0.5, 1.0] for c in centres])
    xyz = np.concatenate([ground, blobs])
    Q, _ = np.linalg.qr(rng.standard_normal((D_MAP, D_MAP)))
    coef = np.zeros((len(xyz), 3))
    coef[:1600, 1] = ground[:, 0] / 3.0            # the ground's descriptors vary with x and y ...
    coef[:1600, 2] = ground[:, 1] / 6.0
    coef[1600:, 0] = 4.0                           # ... the blobs' sit together, away from all of them
    desc = 1.0 + coef @ Q[:, :3].T + 0.01 * rng.standard_normal((len(xyz), D_MAP))
    assert (desc.sum(1) > 0).all()
    cloud = np.c_[xyz, desc].astype(np.float32)
    order = rng.permutation(len(cloud))
    cloud = cloud[order]
    scans, poses = [], []
    for s in range(2):
        sel = rng.permutation(len(cloud))[:1500]
        scans.append(cloud[sel] + np.c_[rng.normal(0, 0.01, (1500, 3)), np.zeros((1500, D_MAP))].astype(np.float32))
        poses.append(np.eye(4))
    return dict(map_poses=[np.eye(4)], map_point_clouds=[cloud], map_clip=[], scene_poses=poses, scene_point_clouds=scans,
                scene_sequences=["scanA", "scanB"]), order >= 1600


@functools.lru_cache(maxsize=None)
def _semantic_case():
    """(scene, the scene's map as evaluate_scene builds it, the oracle's fit and colours of it, the class read from the blob rows'
    colours, the restated filter's results for two scans with one shared RandomState(42)) -- computed once, never written."""
    from vfmreg.evaluation import build_local_map
    from vfmreg.mapping import VoxelHashMap
    VoxelHashMap.quiet = True
    scene, _ = _semantic_scene()
    local_map = build_local_map(scene["map_poses"], scene["map_point_clouds"], n_descriptors=D_MAP)
    X = local_map[:, 3:]
    mean, comps, _ = po.fit(X, 3)
    rgb = po.colours(po.project_ordered(X, mean, comps), X)
    is_blob = local_map[:, 2] > 0.15           # (the ground sheet lies at z = 0)
    assert local_map.shape[0] >= 2800 and is_blob.sum() >= 4 * 300
    remove_classes = [np.median(rgb[is_blob], axis=0, keepdims=True).astype(np.float32)]
    near = po.gate(rgb, remove_classes[0])
    assert 0.9 * is_blob.sum() <= len(near) <= 1.1 * is_blob.sum()
    rng = np.random.RandomState(42)
    runs = [po.filter_semantic_restated(local_map, rgb, remove_classes, 0.5, rng) for _ in scene["scene_poses"]]
    assert len(runs[0][2]) < len(local_map)
    for a in (local_map, rgb):
        a.setflags(write=False)
    return scene, local_map, (mean, comps), rgb, remove_classes, runs


class _Fit:
    def __init__(self, mean_, components_):
        self.mean_, self.components_ = mean_, components_


def test_filter_map_semantic():
    from vfmreg import pca, utils
    _, local_map, fit, rgb, remove_classes, runs = _semantic_case()
    holder = pca.DescriptorPCA()
    holder.fit_pca[3] = _Fit(*fit)                 # the oracle's fit: the colours are then equal bit for bit, and so is the gate
    got = utils.filter_map_semantic(local_map, holder, remove_classes, 0.5, np.random.RandomState(42))
    want = runs[0]
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[1].dtype == np.uint8 and len(got[2]) < len(local_map)
    # a fit of its own (the default): the same map up to the colours that an eigen-solve's rounding can move across the radius
    own = utils.filter_map_semantic(local_map, pca.DescriptorPCA(), remove_classes, 0.5, np.random.RandomState(42))
    assert abs(len(own[2]) - len(want[2])) <= 0.02 * len(local_map)


def test_evaluate_scene_with_cluster_removal():
    from vfmreg import pca
    from vfmreg.evaluation import Evaluation, evaluate_scene
    from vfmreg.registration import RegistrationNode
    scene, local_map, fit, rgb, remove_classes, runs = _semantic_case()
    plain = evaluate_scene(scene, RegistrationNode(ransac_iterations=1000, cache_map=True), Evaluation())
    zero = evaluate_scene(scene, RegistrationNode(ransac_iterations=1000, cache_map=True), Evaluation(), cluster_removal_prob=0.0)
    assert zero.points_in_map == plain.points_in_map == [len(local_map)] * 2
    assert zero.rot_errors == plain.rot_errors and zero.trans_errors == plain.trans_errors
    holder = pca.DescriptorPCA()
    holder.fit_pca[3] = _Fit(*fit)
    ev = evaluate_scene(scene, RegistrationNode(ransac_iterations=1000, cache_map=True), Evaluation(), cluster_removal_prob=0.5,
                        remove_classes=remove_classes, pca=holder)
    assert ev.points_in_map == [len(r[2]) for r in runs]          # one RandomState(42), shared by the scans (RN:584)
    assert set(ev.rot_errors) == {"vfm_ransac", "vfm_ransac_icp"} and all(len(v) == 2 for v in ev.rot_errors.values())


# ----------------------------------------------------------------------------------------------------------------------- buffers
def _guarded_chain(X, mean, comps, rows_u8, gate_colours, poison, fill):
    """all four entry points with every buffer guarded; returns the outputs and the guarded buffers"""
    from vfmreg import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    n, d = X.shape
    k, m = len(comps), len(gate_colours)
    tdt = torch.float16 if X.dtype == np.float16 else torch.float32
    ins = dict(x=GuardedBuffer((n, d), tdt, seed=1).set(X), mean=GuardedBuffer(d, torch.float64, seed=2).set(mean),
               comps=GuardedBuffer((k, d), torch.float64, seed=3).set(comps), rows=GuardedBuffer((n, 3), torch.uint8, seed=4).set(rows_u8),
               gate=GuardedBuffer((m, 3), torch.float64, seed=5).set(gate_colours))
    outs = dict(mean_out=GuardedBuffer(d, torch.float64, seed=6), scatter=GuardedBuffer((d, d), torch.float64, seed=7),
                y=GuardedBuffer((n, k), torch.float64, seed=8), zero=GuardedBuffer(n, torch.uint8, seed=9),
                lo=GuardedBuffer(k, torch.float64, seed=10), hi=GuardedBuffer(k, torch.float64, seed=11),
                values=GuardedBuffer((n, k), torch.float32, seed=12), rgb=GuardedBuffer((n, 3), torch.uint8, seed=13),
                idx=GuardedBuffer((m, n), torch.int64, seed=14), counts=GuardedBuffer(m, torch.int64, seed=15),
                ws_m=GuardedBuffer(lib.vfm_pca_moments_workspace_bytes(d), torch.uint8, seed=16),
                ws_p=GuardedBuffer(lib.vfm_pca_project_workspace_bytes(), torch.uint8, seed=17))
    for g in outs.values():
        g.fill_bytes(fill)
    if poison:
        for name, g in ins.items():
            g.poison_guards("ff" if name == "rows" else "nan")
    dt = ROWS_F16 if X.dtype == np.float16 else ROWS_F32
    _lib.check(lib.vfm_pca_moments(ins["x"].ptr(), dt, n, d, outs["mean_out"].ptr(), outs["scatter"].ptr(), outs["ws_m"].ptr(),
                                   outs["ws_m"].nbytes, st), "moments")
    _lib.check(lib.vfm_pca_project(ins["x"].ptr(), dt, n, d, ins["mean"].ptr(), ins["comps"].ptr(), k, outs["y"].ptr(), outs["zero"].ptr(),
                                   outs["lo"].ptr(), outs["hi"].ptr(), outs["ws_p"].ptr(), outs["ws_p"].nbytes, st), "project")
    _lib.check(lib.vfm_pca_colours(outs["y"].ptr(), outs["zero"].ptr(), n, k, outs["lo"].ptr(), outs["hi"].ptr(), outs["values"].ptr(),
                                   outs["rgb"].ptr() if k == 3 else None, st), "colours")      # (colours need three components)
    _lib.check(lib.vfm_colour_gate(ins["rows"].ptr(), n, ins["gate"].ptr(), m, 50.0, outs["idx"].ptr(), outs["counts"].ptr(), st), "gate")
    torch.cuda.synchronize()
    for name, g in list(ins.items()) + list(outs.items()):
        assert g.intact(), f"{name}: {g.intact()!r} (n = {n}, d = {d})"
    res = {name: outs[name].numpy() for name in ("mean_out", "scatter", "y", "zero", "lo", "hi", "values", "counts") + (("rgb",) if k == 3 else ())}
    res["idx"] = [outs["idx"].numpy()[c, :res["counts"][c]] for c in range(m)]
    return res


@pytest.mark.parametrize("n,d,half", [(1, 1, False), (3, 17, False), (65, 65, False), (1001, 384, False), (130, 768, True)])
def test_every_buffer_stays_inside_its_guards(n, d, half):
    rng = np.random.RandomState(n + d)
    X = rng.standard_normal((n, d)).astype(np.float16 if half else np.float32)
    if n > 2:
        X[1] = 0.0
    mean = rng.standard_normal(d)
    comps = rng.standard_normal((min(3, d), d))
    rows = rng.randint(60, 141, size=(n, 3)).astype(np.uint8)
    gate = np.array([[100., 100., 100.], [110., 100., 100.]])
    plain = _guarded_chain(X, mean, comps, rows, gate, poison=False, fill=0x00)
    other = _guarded_chain(X, mean, comps, rows, gate, poison=True, fill=0xFF)      # poisoned input guards, stale outputs and workspaces
    for name, a in plain.items():
        b = other[name]
        if name == "idx":
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
        else:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name
    # ... and still the oracle's answer
    X64 = X.astype(np.float64)
    assert np.array_equal(_bits(plain["y"]), _bits(po.project_ordered(X64, mean, comps)))
    assert np.array_equal(np.concatenate(plain["idx"]), po.gate(rows, gate))
    ref_mean, ref_S = po.moments(X64)
    assert (np.abs(plain["scatter"] - ref_S) <= po.scatter_bound(ref_S, n)).all()
