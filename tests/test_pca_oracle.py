"""CPU anchors of tests/pca_oracle.py: every piece of the oracle against a source that is independent of it (sklearn, torch's
pca_lowrank, a literal transcription of the reference's lines), and the conditions of its data generator that tests/test_gpu_pca.py
relies on."""
import functools

import numpy as np
import pytest

from . import pca_oracle as po

E2E_SEED, E2E_SHAPE = 6, (5003, 384)      # what the end-to-end GPU test runs on


@functools.lru_cache(maxsize=None)
def data(seed, n, d):
    X = po.spectrum_data(seed, n, d)
    X.setflags(write=False)
    return X


def _abs_cos(a, b):
    return np.abs((a * b).sum(axis=1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def test_components_span_sklearns():
    from sklearn.decomposition import PCA
    X = data(1, 1000, 17).astype(np.float64)
    mean, comps, sv = po.fit(X, 3)
    ref = PCA(n_components=3, svd_solver="full").fit(X)
    assert np.allclose(mean, ref.mean_, rtol=0, atol=1e-12)
    assert _abs_cos(comps, ref.components_).min() >= 1 - 1e-5
    assert np.allclose(sv, ref.singular_values_, rtol=1e-10)
    assert np.allclose(np.linalg.norm(comps, axis=1), 1.0, atol=1e-12)


def test_components_span_pca_lowranks():
    import torch
    X = data(1, 1000, 17).astype(np.float64)
    mean, comps, _ = po.fit(X, 3)
    torch.manual_seed(0)
    _, _, V = torch.pca_lowrank(torch.from_numpy(X - mean), q=3, center=False, niter=4)
    assert _abs_cos(comps, V.T.numpy()).min() >= 1 - 1e-5


def test_sign_rule():
    c = po.apply_sign_rule(np.array([[0.1, -0.9, 0.2], [0.5, 0.1, -0.5], [-0.5, 0.1, 0.5], [0.2, 0.3, 0.1]]))
    assert np.array_equal(c, [[-0.1, 0.9, -0.2], [0.5, 0.1, -0.5], [0.5, -0.1, -0.5], [0.2, 0.3, 0.1]])   # ties: the lowest index decides
    X = data(1, 1000, 17)
    _, comps, _ = po.fit(X, 3)
    assert all(row[np.argmax(np.abs(row))] > 0 for row in comps)


@pytest.mark.parametrize("d", [1, 3, 63, 64, 65, 384])
def test_ordered_projection_is_the_projection(d):
    rng = np.random.RandomState(d)
    X = rng.standard_normal((37, d)).astype(np.float32)
    mean = rng.standard_normal(d)
    comps = rng.standard_normal((min(3, d), d))
    Y = po.project_ordered(X, mean, comps)
    ref = (X.astype(np.float64) - mean) @ comps.T
    assert np.abs(Y - ref).max() <= 1e-9
    # the order itself, spelled out element by element for one row
    t = (X[5].astype(np.float64) - mean) * comps[0]
    p = [0.0] * 64
    for c in range(d):
        p[c % 64] = p[c % 64] + t[c]
    for s in (32, 16, 8, 4, 2, 1):
        p = [p[l] + p[l ^ s] for l in range(64)]
    assert len(set(p)) == 1 and p[0] == Y[5, 0]


def test_normalisation_and_colours_transcribe_the_reference():
    X = data(1, 1000, 17).copy()
    X[3] = 0.0
    X[7] = -0.0
    mean, comps, _ = po.fit(X, 3)
    Y = po.project_ordered(X, mean, comps)
    ref = (X.astype(np.float64) - mean) @ comps.T          # Y = (X - mean_) @ components_.T
    assert np.abs(Y - ref).max() <= 1e-9
    lit = Y.copy()
    lit -= lit.min(0)                                       # Y -= Y.min(0)
    lit /= lit.max(0)                                       # Y /= Y.max(0)
    assert np.array_equal(po.normalise(Y), lit)
    assert lit.min() == 0.0 and lit.max() == 1.0
    rgb = (lit * 255.0).astype(np.uint8)                    # IF:185
    rgb[np.all(X == 0, axis=-1)] = 0                        # IF:188-190
    assert np.array_equal(po.colours(Y, X), rgb)
    assert not rgb[3].any() and not rgb[7].any() and rgb.max() == 255
    # a constant component: NaN as a value, 0 as a colour
    Yc = Y.copy()
    Yc[:, 1] = 2.5
    assert np.isnan(po.normalise(Yc)[:, 1]).all() and not po.colours(Yc, X)[:, 1].any()


def test_gate_boundary_and_overlap():
    colour = np.array([100., 100., 100.])
    offsets = po.BOUNDARY_OFFSETS
    assert list((offsets ** 2).sum(1)) == [2498, 2499, 2500, 2501]
    rows = np.concatenate([colour + offsets, [[0, 0, 0]], colour - offsets]).astype(np.uint8)
    got = po.gate(rows, [colour])
    assert list(got) == [0, 1, 5, 6]                        # 2499 is inside, 2500 is not
    d2 = ((rows.astype(np.float64) - colour) ** 2).sum(1)
    assert np.array_equal(got, np.flatnonzero(d2 < 50.0 * 50.0))
    two = po.gate(rows, [colour, colour + [10, 0, 0]])
    assert list(two[:4]) == [0, 1, 5, 6] and len(two) > 4 and len(np.unique(two)) < len(two)   # a row near both colours appears twice
    assert two.dtype == np.int64 or two.dtype == np.intp


@pytest.mark.parametrize("shape", [(5003, 384), (1000, 17)])
def test_generator_has_separated_leading_eigenvalues(shape):
    X = data(E2E_SEED if shape == E2E_SHAPE else 1, *shape)
    _, S = po.moments(X)
    w = np.linalg.eigvalsh(S)
    for k in (1, 2, 3):
        assert po.eigen_gap(w, k) >= np.trace(S) / 100


def test_generator_has_no_colour_on_an_integer_boundary():
    """For the seed of the end-to-end GPU test: no oracle value * 255 within delta of an integer, apart from the exact 0s and 255s."""
    X = data(E2E_SEED, *E2E_SHAPE)
    mean, S = po.moments(X)
    comps, _, _ = po.fit_from_scatter(S, 3)
    Y = po.project_ordered(X, mean, comps)
    delta = po.colour_delta(X, mean, S, Y, 3)
    assert 1e-7 < delta < 1e-4, delta
    v = po.normalise(Y) * 255.0
    assert not po.near_integer(v, delta).any()
    assert (v == 0.0).sum() == 3 and (v == 255.0).sum() == 3
    assert po.fit_bound(S, len(X), 3) < 1e-9
