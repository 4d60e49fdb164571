"""RANSAC's per-hypothesis bounds (csrc/ransac.hip): the table of inputs, a numpy emulation of the two bound generators, and
the checks that tests/test_ransac_bound_cases.py (CPU, on the emulation) and tests/test_gpu_ransac_bounds.py (GPU, on what
vfm_debug_ransac_state reads back) share.  The reference is the oracle's per-hypothesis record: orc.ransac_corr(..., per_hyp=True).

Every case is a dict: src, tgt (fp64 clouds), corres (int32 [C, 2]), max_dist, n_iter, seed, and
    path    "closed-form"  every hypothesis is bounded by the moment pass (unsure = 0), at most CAND_MAX survivors
            "point-wise"   some hypothesis is not provably all-inlier (unsure = 1): the fp32 pass recomputes every bound
            "overflow"     more than CAND_MAX survivors; `unsure` says which generator made the bounds
The shapes are the smallest at which each mechanism still has something to get wrong (see the comment of each builder)."""
import ctypes as C

import numpy as np

CAND_MAX = 2048            # capacity of the candidate list (VFM_DEBUG_RANSAC_CAND_MAX)
DBL_MAX = np.finfo(np.float64).max
U32 = 2.0 ** -24           # unit round-off of fp32
U64 = 2.0 ** -53
MI355X_CUS = 256           # compute units the CPU test assumes for "loop-second-round" (the GPU test asks the device)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _pose(rng):
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q, rng.uniform(-20, 20, 3)


def _shuffle(rng, src, tgt):
    """correspondences index into the clouds in shuffled order (as tests/test_gpu_parity.py::_ransac_case does)"""
    n = len(src)
    ps, pt = rng.permutation(n), rng.permutation(n)
    sc, tc = np.empty_like(src), np.empty_like(tgt)
    sc[ps] = src
    tc[pt] = tgt
    return sc, tc, np.stack([ps, pt], 1).astype(np.int32)


def _scene(n, outlier, seed, noise=0.02, extent=60.0):
    rng = np.random.default_rng(seed)
    R, t = _pose(rng)
    box = lambda k: np.c_[rng.uniform(-extent, extent, k), rng.uniform(-extent, extent, k), rng.uniform(-3, 12, k)]  # noqa: E731
    src = box(n)
    tgt = src @ R.T + t
    if noise > 0:
        tgt = tgt + rng.normal(0, noise, src.shape)
    bad = rng.random(n) < outlier
    tgt[bad] = box(int(bad.sum()))
    return _shuffle(rng, src, tgt)


def _case(path, scene, max_dist, n_iter, seed, unsure=None):
    src, tgt, corres = scene
    if unsure is None:
        unsure = path == "point-wise"
    return dict(path=path, unsure=bool(unsure), src=src, tgt=tgt, corres=corres, max_dist=float(max_dist), n_iter=int(n_iter),
                seed=int(seed))


def _far(scene, off=3.0e5):
    src, tgt, corres = scene
    return src + off, tgt + np.array([off, -2.0 * off, 0.25 * off]), corres


def _lattice(seed):
    """8 x 8 x 8 integer lattice, a 90 degree turn about z, an integer shift; 40 % of the targets moved by exactly one unit along an axis:
    every residual of a hypothesis drawn from three unmoved pairs is 0 or 1 up to rounding, i.e. within an ulp of max_dist = 1"""
    rng = np.random.default_rng(seed)
    g = np.arange(8.0)
    src = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tgt = src @ R.T + np.array([5.0, -3.0, 2.0])
    moved = np.nonzero(rng.random(len(src)) < 0.4)[0]
    tgt[moved, rng.integers(0, 3, len(moved))] += rng.choice([-1.0, 1.0], len(moved))
    return _shuffle(rng, src, tgt)


def _line(n, seed, jitter, length):
    rng = np.random.default_rng(seed)
    R, t = _pose(rng)
    d = np.array([0.6, 0.64, 0.48])
    src = rng.uniform(-length, length, (n, 1)) * d
    tgt = src @ R.T + t
    if jitter > 0:
        src = src + rng.normal(0, jitter, src.shape)
        tgt = tgt + rng.normal(0, jitter, tgt.shape)
    return _shuffle(rng, src, tgt)


def _identical(n):
    src = np.tile(np.array([[1.5, -2.25, 0.75]]), (n, 1))
    tgt = np.tile(np.array([[4.0, 0.5, -1.0]]), (n, 1))
    return src, tgt, np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)


def loop_second_round_iters(cus):
    """hypothesis blocks of 64 for `cus` workgroups, two more, and one hypothesis: ransac_coarse_loop_kernel's first workgroups walk a
    second block (reusing their LDS tables), the last block holds a single hypothesis"""
    return 64 * (int(cus) + 2) + 1


def _builders():
    b = {}
    # ---- point-wise fp32 pass
    b["borderline"] = lambda: _case("point-wise", _scene(1500, 0.5, 101), 0.06, 600, 7)            # threshold at ~1.7 sigma of the residuals
    # 90 % outliers: one sample in 1000 is clean.  600 draws hold none (no hypothesis has a single possible inlier: n_hi = 0, r_hi undefined),
    # 6000 draws hold a few, and fitness decides among them
    b["outlier-dominated"] = lambda: _case("point-wise", _scene(1500, 0.9, 102), 0.5, 600, 7)
    b["outlier-dominated-6000"] = lambda: _case("point-wise", _scene(1500, 0.9, 102), 0.5, 6000, 7)
    b["far-from-origin"] = lambda: _case("point-wise", _far(_scene(1000, 0.3, 103)), 0.5, 600, 11)
    b["eta-above-threshold"] = lambda: _case("point-wise", _scene(1000, 0.3, 104, extent=3.0e4), 0.05, 600, 7)    # lo clamps to 0: n_lo = 0
    b["below-fp32-resolution"] = lambda: _case("overflow", _scene(1000, 0.0, 105, noise=0.0), 1e-5, 3000, 7, unsure=True)
    b["lattice-1"] = lambda: _case("point-wise", _lattice(106), 1.0, 600, 7)
    b["lattice-sqrt2"] = lambda: _case("point-wise", _lattice(106), np.sqrt(2.0), 600, 7)
    b["near-collinear"] = lambda: _case("point-wise", _line(200, 107, 1e-3, 100.0), 0.5, 300, 7)   # n2 ~ n1 1e-20: a third fail
    b["tiny"] = lambda: _case("point-wise", _scene(5, 0.0, 108), 0.5, 300, 7)
    # 128 = COARSE_CHUNK = SCORE_CHUNK, 1024 = EXACT_CHUNK = the centring stride, odd C = the float4 tail of pts32;
    # n_iter 65 / 257: one hypothesis in the last block of 64
    for c in (127, 128, 129, 1023, 1024, 1025):
        for n_iter in (65, 257):
            b[f"chunk-{c}-{n_iter}"] = lambda c=c, n_iter=n_iter: _case("point-wise", _scene(c, 0.3, 200 + c), 0.3, n_iter, 7)
    b["loop-second-round"] = lambda cus=MI355X_CUS: _case("point-wise", _scene(300, 0.3, 109), 0.3, loop_second_round_iters(cus), 7)
    # ---- closed-form moment pass
    b["moment-plain"] = lambda: _case("closed-form", _scene(3000, 0.0, 110), 10000.0, 3000, 11)
    b["moment-half-wrong"] = lambda: _case("closed-form", _scene(2000, 0.5, 111), 10000.0, 2000, 11)
    b["moment-far"] = lambda: _case("closed-form", _far(_scene(3000, 0.0, 112)), 1.0e7, 2000, 11)     # heavy cancellation in the moments
    b["moment-near-perfect"] = lambda: _case("closed-form", _scene(3000, 0.0, 113, noise=1e-7), 10000.0, 2000, 11)
    # thresholds near the scene extent.  "All inliers" needs 3 (4.01 M + |tau|)^2 1.001 < d^2 with M = 87 m here: at 260 m NO hypothesis is
    # provable (the moment pass only raises `unsure`); at 650 m those with |tau|_inf < 24 m are and the others are not, and most blocks of
    # the point-wise pass take its all-inlier branch
    b["threshold-260"] = lambda: _case("point-wise", _scene(2500, 0.2, 114), 260.0, 1000, 11)
    b["moment-mixed"] = lambda: _case("point-wise", _scene(2500, 0.2, 114), 650.0, 1000, 11)
    b["moment-noise-free"] = lambda: _case("overflow", _scene(1000, 0.0, 115, noise=0.0), 10000.0, 3000, 11, unsure=False)
    # ---- every sample degenerate: the default result, nothing to bound
    b["all-collinear"] = lambda: _case("closed-form", _line(200, 116, 0.0, 30.0), 0.5, 300, 7)
    b["all-identical"] = lambda: _case("closed-form", _identical(50), 0.5, 300, 7)
    return b


BUILDERS = _builders()
NAMES = list(BUILDERS)
DEGENERATE = ("all-collinear", "all-identical")
# the property each of these cases exists for (asserted on the CPU)
UNDECIDED_COUNTS = ("borderline", "lattice-1", "lattice-sqrt2")      # some hypothesis with n_lo < n_hi
PARTLY_DEGENERATE = ("near-collinear", "tiny")                       # 10 % .. 90 % of the samples degenerate


def make(name, **kw):
    case = BUILDERS[name](**kw)
    case["name"] = name
    return case


def stream(case):
    """the gathered correspondence stream [C, 6] (source point, target point): ransac_gather_kernel's output"""
    c = case["corres"]
    return np.concatenate([case["src"][c[:, 0]], case["tgt"][c[:, 1]]], 1)


# ------------------------------------------------------------------------------------------------------------------ hypotheses
def philox_picks(n_iter, seed, C_):
    """the three picks of every hypothesis: Philox4x32-10 with counter (h, 0, 0, 0) and the seed as key, pick = word * C >> 32"""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.arange(n_iter, dtype=np.uint64)] + [np.zeros(n_iter, dtype=np.uint64) for _ in range(3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([(c[j] * np.uint64(C_)) >> np.uint64(32) for j in range(3)], 1).astype(np.int64)


def hypotheses(case, orc):
    """(T [n_iter, 4, 4], valid [n_iter]): the oracle's Kabsch on every sample (the device's is bit-identical to it)"""
    pts = stream(case)
    picks = philox_picks(case["n_iter"], case["seed"], len(pts))
    A = np.ascontiguousarray(pts[picks, :3])
    B = np.ascontiguousarray(pts[picks, 3:])
    n = case["n_iter"]
    T = np.empty((n, 4, 4))
    valid = np.empty(n, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    orc.lib().orc_kabsch_batched(vp(A), vp(B), None, C.c_int64(n), C.c_int64(3), C.c_double(0.0), vp(T), vp(valid))
    return T, valid.astype(bool)


def _centred(pts):
    cen = pts.mean(0)
    v = pts - cen
    return cen, v, float(np.abs(v).max())


def _tau(T, cen):
    """t' = (t + R cs) - cq per hypothesis, in the kernels' operation order"""
    R, t = T[:, :3, :3], T[:, :3, 3]
    cs, cq = cen[:3], cen[3:]
    return (t + ((R[:, :, 0] * cs[0] + R[:, :, 1] * cs[1]) + R[:, :, 2] * cs[2])) - cq


def eta_of(case, T):
    """eta_h = sqrt(3) u32 (32 M + 8 |t'|_inf) of the point-wise pass, from its definition"""
    cen, _, M = _centred(stream(case))
    return 1.7321 * (U32 * (32.0 * M + 8.0 * np.abs(_tau(T, cen)).max(1)))


# ------------------------------------------------------------------------------------------------------------------ emulation
def emulate_pointwise(case, T, valid):
    """ransac_coarse_block in numpy: fp32 residuals WITHOUT fused multiply-add (the kernel fuses: the difference is inside delta),
    fp32 sums per chunk of 128, fp64 across chunks"""
    pts = stream(case)
    C_, n = len(pts), case["n_iter"]
    cen, v, M = _centred(pts)
    p32 = v.astype(np.float32)
    tau = _tau(T, cen)
    eta = 1.7321 * (U32 * (32.0 * M + 8.0 * np.abs(tau).max(1)))
    d = case["max_dist"]
    if d > 0:
        lo, hi = np.maximum(0.0, d - eta), d + eta
        Lf, Hf = (lo * lo * (1.0 - 1e-6)).astype(np.float32), (hi * hi * (1.0 + 1e-6)).astype(np.float32)
    else:
        Lf = Hf = np.full(n, -1.0, dtype=np.float32)
    R32, t32 = T[:, :3, :3].astype(np.float32), tau.astype(np.float32)
    n_lo, n_hi = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    E_lo, E_hi = np.zeros(n), np.zeros(n)
    pad = (-C_) % 128
    for s in range(0, n, 256):
        e = min(n, s + 256)
        d2 = np.zeros((e - s, C_), dtype=np.float32)
        for a in range(3):
            x = R32[s:e, a, 2, None] * p32[None, :, 2] + t32[s:e, a, None]
            x = R32[s:e, a, 1, None] * p32[None, :, 1] + x
            x = R32[s:e, a, 0, None] * p32[None, :, 0] + x
            x = x - p32[None, :, 3 + a]
            d2 = x * x + d2
        for thr, cnt, acc in ((Lf, n_lo, E_lo), (Hf, n_hi, E_hi)):
            inl = d2 < thr[s:e, None]
            cnt[s:e] = inl.sum(1)
            part = np.pad(np.where(inl, d2, np.float32(0)), ((0, 0), (0, pad))).reshape(e - s, -1, 128)
            acc[s:e] = part.sum(2, dtype=np.float32).astype(np.float64).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_lo = np.where(n_lo > 0, np.maximum(0.0, np.sqrt(E_lo / n_lo) * (1.0 - 1e-4) - 3.0 * eta), 0.0)
        r_hi = np.where(n_hi > 0, np.sqrt(E_hi / n_hi) * (1.0 + 1e-4) + eta, DBL_MAX)
    n_lo[~valid], n_hi[~valid], r_lo[~valid], r_hi[~valid] = 0, -1, 0.0, 0.0
    return dict(n_lo=n_lo, n_hi=n_hi, r_lo=r_lo, r_hi=r_hi)


def emulate_moment(case, T, valid):
    """ransac_moment_kernel in numpy (numpy's summation for the 22 moments).  Returns the bounds and `sure` [n_iter]: the hypothesis is
    provably all-inlier; where it is not, the bound is not produced (the kernel raises `unsure`)"""
    pts = stream(case)
    C_, n = len(pts), case["n_iter"]
    cen, v, M = _centred(pts)
    sg, kp = v[:, :3], v[:, 3:]
    S = sg.T @ sg
    K = kp.T @ sg                      # K[a][b] = sum kappa_a sigma_b
    Akk = float((kp * kp).sum())
    sbar, kbar = sg.sum(0), kp.sum(0)
    Xs, Xq = float(np.abs(pts[:, :3]).max()), float(np.abs(pts[:, 3:]).max())
    gm = float((C_ + 1023) // 1024) + 32.0
    R, t = T[:, :3, :3], T[:, :3, 3]
    tau = _tau(T, cen)
    taumax, tt = np.abs(tau).max(1), (tau * tau).sum(1)
    tabs, rmax = np.abs(t).max(1), np.abs(R).reshape(n, 9).max(1)
    max_d2 = case["max_dist"] ** 2 if case["max_dist"] > 0 else -1.0
    reach = 4.01 * M + taumax
    sure = valid & (rmax <= 1.001) & (max_d2 > 0.0) & (3.0 * reach * reach * 1.001 < max_d2)
    q1 = np.einsum("hab,bc,hac->h", R, S, R)
    rk = (R * K[None]).sum((1, 2))
    t4 = (tau * (R @ sbar - kbar)).sum(1)
    Cd = float(C_)
    E = (((q1 + Cd * tt) + Akk) + 2.0 * t4) - 2.0 * rk
    B = ((13.0 * np.trace(S) + 5.0 * Akk) + 1.01 * Cd * tt) + 6.0 * taumax * (3.01 * np.abs(sbar).max() + np.abs(kbar).max())
    eps1 = U64 * (gm + 80.0) * B
    Ep = np.maximum(E, 0.0) + eps1
    A = (3.01 * Xs + tabs) + Xq
    eps = (eps1 + (Cd + 8.0) * U64 * Ep) + 48.0 * U64 * A * np.sqrt(Cd * Ep)
    r_lo = np.sqrt(np.maximum(0.0, E - eps) / Cd) * (1.0 - 1e-13)
    r_hi = np.sqrt(np.maximum(0.0, E + eps) / Cd) * (1.0 + 1e-13)
    n_lo = np.where(sure, C_, 0).astype(np.int32)
    n_hi = np.where(sure, C_, -1).astype(np.int32)
    return dict(n_lo=n_lo, n_hi=n_hi, r_lo=np.where(sure, r_lo, 0.0), r_hi=np.where(sure, r_hi, 0.0)), sure


def select(b):
    """F, R* and the survivors from a set of bounds.  r_hi = DBL_MAX is the kernels' "no possible inlier: the RMSE
    is undefined" and never sets R* (ransac_select_rmin_kernel skips it; such a hypothesis has n_hi = 0 and cannot survive either)"""
    F = int(max(0, b["n_lo"].max()))
    tie = (b["n_hi"] >= 0) & (b["n_lo"] == F) & (b["n_hi"] == F) & (b["r_hi"] < DBL_MAX)
    Rs = float(b["r_hi"][tie].min()) if tie.any() else np.inf
    surv = np.nonzero((b["n_hi"] > 0) & (b["n_hi"] >= F) & ((b["n_hi"] > F) | (b["r_lo"] <= Rs)))[0]
    return F, Rs, surv


def emulate(case, orc):
    """what the library should leave behind: the moment pass, and the point-wise pass over everything if it raised `unsure`"""
    T, valid = hypotheses(case, orc)
    b, sure = emulate_moment(case, T, valid)
    unsure = bool((valid & ~sure).any())
    if unsure:
        b = emulate_pointwise(case, T, valid)
    F, Rs, surv = select(b)
    st = dict(b, T=T, valid=valid, F=F, Rstar=Rs, count=len(surv), unsure=int(unsure), survivors=surv)
    return st


# ------------------------------------------------------------------------------------------------------------------ checks
def _first(mask):
    i = np.nonzero(mask)[0]
    return (int(i[0]), len(i)) if len(i) else (None, 0)


def _fail(tag, what, mask, detail):
    h, n = _first(mask)
    if h is not None:
        raise AssertionError(f"{tag}: {what}: {n} hypotheses, first h = {h}: {detail(h)}")


def check_bounds(tag, case, b, ref):
    """DESIGN.md 4.3's contract per hypothesis: validity, [n_lo, n_hi] contains the oracle's inlier count, [r_lo, r_hi] its RMSE.
    The two forms of the RMSE claim that the selection needs (r_lo <= rmse where the count reaches n_hi, rmse <= r_hi where the count
    is decided) are checked first, then the documented claim for every valid hypothesis."""
    C_ = len(case["corres"])
    fit, rm = ref.hyp_fit, ref.hyp_rmse
    n_lo, n_hi, r_lo, r_hi = b["n_lo"], b["n_hi"], b["r_lo"], b["r_hi"]
    _fail(tag, "validity (n_hi < 0 <=> degenerate sample)", (n_hi < 0) != (fit < 0), lambda h: f"n_hi {n_hi[h]}, hyp_fit {fit[h]}")
    ok = fit >= 0
    good = np.rint(fit * C_).astype(np.int64)
    _fail(tag, "count outside [n_lo, n_hi]", ok & ((n_lo > good) | (good > n_hi)), lambda h: f"n_lo {n_lo[h]} good {good[h]} n_hi {n_hi[h]}")
    show = lambda h: f"r_lo {r_lo[h]!r} rmse {rm[h]!r} r_hi {r_hi[h]!r} (n_lo {n_lo[h]} good {good[h]} n_hi {n_hi[h]})"  # noqa: E731
    _fail(tag, "rmse below r_lo although the count reaches n_hi", ok & (good == n_hi) & (r_lo > rm), show)
    _fail(tag, "rmse above r_hi although the count is decided", ok & (n_lo == n_hi) & (rm > r_hi), show)
    _fail(tag, "rmse outside [r_lo, r_hi] (only the documented claim, the selection's weaker forms hold)", ok & ((r_lo > rm) | (rm > r_hi)),
          show)


def check_not_vacuous(tag, case, b, unsure, eta):
    """the bounds are as tight as their formulas say: closed-form hypotheses have n_lo = n_hi = C; a point-wise hypothesis with a decided
    count and r_lo > 0 has r_hi - r_lo = 2e-4 s + 4 eta <= 2e-4 r_hi + 4 eta (1e-6: the centroid's rounding inside eta)"""
    C_ = len(case["corres"])
    n_lo, n_hi, r_lo, r_hi = b["n_lo"], b["n_hi"], b["r_lo"], b["r_hi"]
    ok = n_hi >= 0
    if not unsure:
        _fail(tag, "closed-form bound without n_lo = n_hi = C", ok & ((n_lo != C_) | (n_hi != C_)), lambda h: f"n_lo {n_lo[h]} n_hi {n_hi[h]} C {C_}")
        return
    sel = ok & (n_lo == n_hi) & (n_lo > 0) & (r_lo > 0)
    width = np.where(sel, r_hi - r_lo, 0.0)
    room = np.where(sel, (2e-4 * r_hi + 4.0 * eta) * (1.0 + 1e-6), 0.0)
    _fail(tag, "r_hi - r_lo wider than 2e-4 r_hi + 4 eta", sel & (width > room), lambda h: f"width {width[h]!r} allowed {room[h]!r} eta {eta[h]!r}")


def check_state(tag, case, st, chain):
    """F, R*, count, unsure and overflow against the read-back bounds and the path the case declares.  Returns the survivors."""
    F, Rs, surv = select(st)
    assert st["F"] == F, f"{tag}: F = {st['F']}, max n_lo = {F} (first h with n_lo = max: {int(np.argmax(st['n_lo']))})"
    assert st["Rstar"] == Rs, f"{tag}: R* = {st['Rstar']!r}, min r_hi over n_lo = n_hi = F is {Rs!r}"
    assert st["count"] == len(surv), f"{tag}: count = {st['count']}, the bounds leave {len(surv)} survivors (first h = {surv[:1]})"
    assert st["unsure"] == int(case["unsure"]), f"{tag}: unsure = {st['unsure']}, the case is built for {case['path']} / unsure = {case['unsure']}"
    over = int(case["path"] == "overflow" and chain != 1)
    assert (len(surv) > CAND_MAX) == (case["path"] == "overflow"), f"{tag}: {len(surv)} survivors, the case is built for {case['path']}"
    assert st["overflow"] == over, f"{tag}: overflow = {st['overflow']}, expected {over} ({len(surv)} survivors, chain {chain})"
    return surv


def _want_score(ref, h):
    """what an exact re-scoring of hypothesis h stores: the oracle's record, or the empty slot for a hypothesis without an inlier"""
    if h < 0 or not ref.hyp_fit[h] > 0:
        return (0.0, 0.0, -1)
    return (float(ref.hyp_fit[h]), float(ref.hyp_rmse[h]), int(h))


def _best_of(ref, hs):
    """the best of hypotheses hs under (fitness desc, rmse asc, id asc) from the oracle's records; empty if none has an inlier"""
    hs = [int(h) for h in hs if ref.hyp_fit[h] > 0]
    if not hs:
        return (0.0, 0.0, -1)
    h = min(hs, key=lambda h: (-ref.hyp_fit[h], ref.hyp_rmse[h], h))
    return _want_score(ref, h)


def _slot(st, k):
    return (float(st["fit"][k]), float(st["rmse"][k]), int(st["hyp"][k]))


def check_survivors_and_scores(tag, case, st, ref, chain, surv):
    """the candidate list is exactly the survivors of the read-back bounds and holds the oracle's winner; every stored exact score is the
    oracle's record of that hypothesis bit for bit; per-block slots hold the best of their 64 hypotheses (of their survivors: chain 1)"""
    n_iter = case["n_iter"]
    nblocks = (n_iter + 63) // 64
    empty = (0.0, 0.0, -1)
    if ref.best_hyp >= 0:
        assert ref.best_hyp in set(surv.tolist()), f"{tag}: the oracle's winner h = {ref.best_hyp} is not among the {len(surv)} survivors"
    if chain == 1:
        for b in range(nblocks):
            want = _best_of(ref, surv[(surv >= 64 * b) & (surv < 64 * b + 64)])
            got = _slot(st, CAND_MAX + b)
            assert got == want, f"{tag}: block {b} (first h = {64 * b}) holds {got}, the best of its survivors is {want}"
        return
    if st["overflow"]:
        for k in range(CAND_MAX):
            assert _slot(st, k) == empty, f"{tag}: candidate slot {k} holds {_slot(st, k)} after an overflow"
        for b in range(nblocks):
            want = _best_of(ref, range(64 * b, min(n_iter, 64 * b + 64)))
            got = _slot(st, CAND_MAX + b)
            assert got == want, f"{tag}: block {b} (first h = {64 * b}) holds {got}, the best of its 64 hypotheses is {want}"
        return
    lst = st["list"][:st["count"]]
    assert len(lst) <= CAND_MAX
    missing, extra = np.setdiff1d(surv, lst), np.setdiff1d(lst, surv)
    assert len(missing) == 0 and len(extra) == 0 and len(set(lst.tolist())) == len(lst), \
        f"{tag}: candidate list differs from the survivors of the bounds: missing h = {missing[:5]}, unexpected h = {extra[:5]}, {len(lst)} entries"
    for k, h in enumerate(lst.tolist()):
        assert _slot(st, k) == _want_score(ref, h), f"{tag}: h = {h} (slot {k}) scored {_slot(st, k)}, the oracle has {_want_score(ref, h)}"
    for k in range(len(lst), CAND_MAX + nblocks):
        assert _slot(st, k) == empty, f"{tag}: slot {k} holds {_slot(st, k)}, nothing was scored there"
