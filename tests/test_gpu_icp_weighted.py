"""The descriptor-weighted search on rows kept in their own type (csrc/icp_rows.hip: ``vfm_icp_rows_stats``, ``vfm_icp_step_nearest_rows``)
against ``orc_icp_desc_stats`` / ``orc_icp_nearest_desc`` on the rows' fp64 image: ``tgt``, ``valid``, the moved points and the statistics
bit for bit, for fp32 and fp64 rows.  Every buffer of a call is a guarded one of exactly the documented size; the inputs' guards are poisoned.

One scene per (dtype, f), voxel size 1, about 5000 map rows:
  * a block of 5 x 5 x 5 voxels at the cap of 20: a source inside has all 27 neighbours full -- 540 candidates, nine rounds of 64;
  * about 2400 scattered rows, on both sides of zero;
  * special places on the line y = 50, far from each other, at coordinates that are exact in binary (so that equal costs ARE equal):
      A  two rows with one descriptor at -+0.25 from the source in ONE voxel: equal costs, the earlier insertion wins
      B  the same at -+0.75 in TWO voxels: the voxel scanned first wins, although it was inserted later
      C  nothing around the source
      D  one row 1.4 away, in the next voxel: chosen, and refused on its Euclidean distance (max_dist 0.8)
      E  one row with a NaN: its cost is NaN, it never wins, nothing is found
      F  a row with an inf next to a finite one
      G  a source whose descriptor is all zero (every weight 1)
      H  a row with the opposite descriptor at 0.1 and one with the identical descriptor at 0.4: c = 1 against c = 0.01, the farther wins
      I  rows with a zero element sum, all zero at 0.1 and [1, -1, 0, ...] at 0.3 (weight 1), and the opposite descriptor at 0.4
The sources are numbered dense, A .. I, then the rest, so n = 1 is the nine-round point and n = 7 ends at F."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.guarded import GuardedBuffer  # noqa: E402

VS, CAP, MAX_DIST = 1.0, 20, 0.8
WIDTHS = [1, 5, 64, 384, 1032]      # 1032 columns: more than one staged chunk of the source descriptor
DTYPES = [np.float32, np.float64]
SIZES = [0, 1, 7, 1000]
STEPS = ["none", "shift", "rigid"]
SPECIALS = "ABCDEFGHI"
Y0, Z0 = 50.5, 0.5


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _stats_ref(desc64):
    from oracle import oracle
    n, f = desc64.shape
    norm, has = np.empty(n), np.empty(n, np.uint8)
    oracle.lib().orc_icp_desc_stats(_f64p(desc64), C.c_int64(n), C.c_int32(f), _f64p(norm), _u8p(has))
    return norm, has


def _nearest_ref(moved, sdesc64, snorm, shas, grid, mdesc64, mnorm, mhas):
    from oracle import oracle
    keys, start, pts = grid
    n, f = sdesc64.shape
    tgt, valid = np.empty((n, 3)), np.empty(n, np.uint8)
    oracle.lib().orc_icp_nearest_desc(_f64p(moved), C.c_int64(n), _f64p(sdesc64), _f64p(snorm), _u8p(shas), C.c_int32(f),
                                      keys.ctypes.data_as(C.POINTER(C.c_int64)), start.ctypes.data_as(C.POINTER(C.c_int32)), _f64p(pts),
                                      _f64p(mdesc64), _f64p(mnorm), _u8p(mhas), C.c_int32(len(keys)), C.c_double(VS), C.c_double(MAX_DIST),
                                      _f64p(tgt), _u8p(valid))
    return tgt, valid


def _step_matrix(kind):
    from oracle import oracle
    if kind == "none":
        return None
    if kind == "shift":          # exact in binary: the moved special sources land where the scene put them
        T = np.eye(4)
        T[:3, 3] = [0.5, -1.25, 2.0]
        return T
    return oracle.se3_exp(np.array([0.3, -0.2, 0.1, 0.02, -0.01, 0.03]))


def _build_scene(dtype, f):
    rng = np.random.default_rng(1000 * f + np.dtype(dtype).itemsize)
    xyz, desc = [], []

    def rnd(k):
        return rng.normal(size=(k, f))

    # the block at the cap
    for a in range(5):
        for b in range(5):
            for c in range(5):
                xyz.append(np.array([a, b, c]) + rng.uniform(0.01, 0.99, (CAP, 3)))
                desc.append(rnd(CAP))
    # scattered rows on both sides of zero
    xyz.append(np.c_[rng.uniform(8.0, 30.0, 2400), rng.uniform(-6.0, 6.0, 2400), rng.uniform(-2.0, 2.0, 2400)])
    desc.append(rnd(2400))
    scattered = xyz[-1]
    d = {k: rnd(1)[0] for k in SPECIALS}
    zero_sum = np.zeros(f)
    if f >= 2:
        zero_sum[:2] = [1.0, -1.0]
    nan_row, inf_row = rnd(1)[0], rnd(1)[0]
    nan_row[f // 2] = np.nan
    inf_row[0] = np.inf
    special_rows = [
        ((40.75, Y0, Z0), d["A"]), ((40.25, Y0, Z0), d["A"]),                  # A: the later coordinate first
        ((46.25, Y0, Z0), d["B"]), ((44.75, Y0, Z0), d["B"]),                  # B: the voxel scanned later is inserted first
        ((66.9, Y0, Z0), d["D"]),
        ((70.6, Y0, Z0), nan_row),
        ((75.6, Y0, Z0), inf_row), ((75.9, Y0, Z0), d["F"]),
        ((80.7, Y0, Z0), -d["G"]), ((80.2, Y0, Z0), d["G"]),
        ((85.6, Y0, Z0), -d["H"]), ((85.9, Y0, Z0), d["H"]),
        ((90.6, Y0, Z0), np.zeros(f)), ((90.8, Y0, Z0), zero_sum), ((90.1, Y0, Z0), -d["I"]),
        ((12.3, 0.4, 0.2), nan_row), ((20.6, -0.4, -0.3), inf_row),            # ... and a NaN and an inf among the scattered rows
    ]
    xyz.append(np.array([p for p, _ in special_rows]))
    desc.append(np.array([r for _, r in special_rows]))
    xyz, desc = np.concatenate(xyz), np.concatenate(desc).astype(dtype)
    # the grid: (voxel key, insertion) order
    v = np.trunc(xyz / VS).astype(np.int64) + (1 << 20)
    key = (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]
    order = np.argsort(key, kind="stable")
    keys, first = np.unique(key[order], return_index=True)
    start = np.r_[first, len(order)].astype(np.int32)
    assert np.diff(start).max() == CAP
    pts, mdesc = np.ascontiguousarray(xyz[order]), np.ascontiguousarray(desc[order])
    # the sources, where they are searched
    dense = rng.uniform(1.0, 4.0, (291, 3))
    sx = dict(A=40.5, B=45.5, C=60.5, D=65.5, E=70.5, F=75.5, G=80.5, H=85.5, I=90.5)
    special_src = np.array([(sx[k], Y0, Z0) for k in SPECIALS])
    pick = rng.permutation(len(scattered))[:700]
    sparse = scattered[pick] + rng.normal(0.0, 0.2, (700, 3))
    at = np.concatenate((dense[:1], special_src, dense[1:], sparse))
    sdesc = rnd(len(at))
    for i, k in enumerate(SPECIALS):
        sdesc[1 + i] = d[k]
    sdesc[1 + SPECIALS.index("G")] = 0.0
    sdesc[300:320] = 0.0                                                        # more sources without a descriptor ...
    sdesc[320:340] = zero_sum                                                   # ... and with a zero element sum
    of_scattered = desc[-len(special_rows) - 2400:]
    sdesc[340:400] = of_scattered[pick[40:100]]                                 # the descriptor of the scattered row they were made from ...
    sdesc[400:430] = -of_scattered[pick[100:130]].astype(np.float64)            # ... and its opposite
    sdesc = np.ascontiguousarray(sdesc.astype(dtype))
    assert len(at) == 1000
    mdesc64, sdesc64 = mdesc.astype(np.float64), sdesc.astype(np.float64)
    mnorm, mhas = _stats_ref(mdesc64)
    snorm, shas = _stats_ref(sdesc64)
    scene = dict(f=f, dtype=dtype, grid=(np.ascontiguousarray(keys), start, pts), mdesc=mdesc, sdesc=sdesc, mnorm=mnorm, mhas=mhas, snorm=snorm,
                 shas=shas, at=at, ref={})
    from oracle import oracle
    for kind in STEPS:
        T = _step_matrix(kind)
        if kind == "rigid":
            src = np.ascontiguousarray((at - T[:3, 3]) @ T[:3, :3])            # about where T takes them back to ``at``
            moved = oracle._transform_rows(src, T)
        elif kind == "shift":
            src = at - T[:3, 3]
            moved = oracle._transform_rows(src, T)
            np.testing.assert_array_equal(moved[1:10], at[1:10])
        else:
            src = moved = at
        tgt, valid = _nearest_ref(np.ascontiguousarray(moved), sdesc64, snorm, shas, scene["grid"], mdesc64, mnorm, mhas)
        scene["ref"][kind] = dict(T=T, src=np.ascontiguousarray(src), moved=moved, tgt=tgt, valid=valid)
    _check_the_scene(scene)
    return scene


def _check_the_scene(scene):
    """the cases of the module docstring are in the reference's answers (where the coordinates are exact)"""
    for kind in ("none", "shift"):
        r = scene["ref"][kind]
        t = {k: r["tgt"][1 + i] for i, k in enumerate(SPECIALS)}
        ok = {k: r["valid"][1 + i] for i, k in enumerate(SPECIALS)}
        assert t["A"].tolist() == [40.75, Y0, Z0] and ok["A"]                   # equal costs in a voxel: the earlier insertion
        assert t["B"].tolist() == [44.75, Y0, Z0] and ok["B"]                   # ... across voxels: the earlier voxel
        assert t["C"].tolist() == [0.0, 0.0, 0.0] and not ok["C"]
        assert t["D"].tolist() == [66.9, Y0, Z0] and not ok["D"]
        assert t["E"].tolist() == [0.0, 0.0, 0.0] and not ok["E"]
        assert t["F"].tolist() == [75.9, Y0, Z0] and ok["F"]
        assert t["G"].tolist() == [80.7, Y0, Z0] and ok["G"]                    # no weight: the nearer row, whatever its descriptor
        assert t["H"].tolist() == [85.9, Y0, Z0] and ok["H"]                    # c = 0.01 at 0.4 beats c = 1 at 0.1
        assert t["I"].tolist() == [90.6, Y0, Z0] and ok["I"]                    # no weight at 0.1 (cost 0.01) beats c = 1 at 0.4
        assert 0.3 < r["valid"].mean() < 1.0
    assert np.isnan(scene["mnorm"]).sum() == 2 and np.isinf(scene["mnorm"]).sum() == 2 and (scene["mhas"] == 0).sum() >= 1
    assert (scene["shas"] == 0).sum() >= 21


_SCENES = {}


def _scene(dtype, f):
    """one scene per (dtype, f), with its map on the device in guarded buffers whose guards are poisoned; never written"""
    key = (np.dtype(dtype).name, f)
    if key not in _SCENES:
        _SCENES.clear()                                                         # (the cases come grouped by scene: one at a time is kept)
        s = _build_scene(dtype, f)
        tdt = torch.float32 if dtype == np.float32 else torch.float64
        keys, start, pts = s["grid"]
        nk = len(pts)
        dev = dict(keys=GuardedBuffer(len(keys), torch.int64, seed=11).set(keys), start=GuardedBuffer(len(start), torch.int32, seed=12).set(start),
                   pts=GuardedBuffer((nk, 3), torch.float64, seed=13).set(pts), mdesc=GuardedBuffer((nk, f), tdt, seed=14).set(s["mdesc"]),
                   mnorm=GuardedBuffer(nk, torch.float64, seed=15).set(s["mnorm"]), mhas=GuardedBuffer(nk, torch.uint8, seed=16).set(s["mhas"]))
        for name, b in dev.items():
            b.poison_guards("zero" if name in ("keys", "start") else "ff" if name == "mhas" else "nan")
        s["dev"], s["tdt"] = dev, tdt
        _SCENES[key] = s
    return _SCENES[key]


def _intact(bufs):
    for name, b in bufs.items():
        assert b.intact(), f"{name}: {b.intact()!r}"


@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_rows_stats_equal_the_oracle(dtype, f):
    from vfmreg import _lib, ops
    lib = _lib.load()
    s = _scene(dtype, f)
    rows = s["dev"]["mdesc"]
    nk = rows.shape[0]
    for n in (0, 1, 257, nk):
        norm = GuardedBuffer(n, torch.float64, seed=1).fill_bytes(0xFF)
        has = GuardedBuffer(n, torch.uint8, seed=2).fill_bytes(0xFF)
        _lib.check(lib.vfm_icp_rows_stats(rows.ptr(), rows.itemsize, n, f, norm.ptr(), has.ptr(), ops._stream()), "icp_rows_stats")
        torch.cuda.synchronize()
        _intact(dict(rows=rows, norm=norm, has=has))
        np.testing.assert_array_equal(norm.numpy(), s["mnorm"][:n])
        np.testing.assert_array_equal(has.numpy(), s["mhas"][:n])
    norm, has = ops.icp_rows_stats(rows.t)                                      # the wrapper
    np.testing.assert_array_equal(norm.cpu().numpy(), s["mnorm"])
    np.testing.assert_array_equal(has.cpu().numpy(), s["mhas"])
    norm, has = ops.icp_rows_stats(rows.t[:0])
    assert norm.shape == (0,) and has.shape == (0,)


def _search(s, n, kind, alias=False, offset=0):
    """vfm_icp_step_nearest_rows on the first ``n`` sources of the scene, every buffer guarded; ``offset``: bytes by which both descriptor
    arrays are moved off their alignment"""
    from vfmreg import _lib, ops
    lib = _lib.load()
    r, d, f = s["ref"][kind], s["dev"], s["f"]
    src = GuardedBuffer((n, 3), torch.float64, seed=21).set(r["src"][:n])
    sdesc = GuardedBuffer((n, f), s["tdt"], seed=22).set(s["sdesc"][:n])
    snorm = GuardedBuffer(n, torch.float64, seed=23).set(s["snorm"][:n])
    shas = GuardedBuffer(n, torch.uint8, seed=24).set(s["shas"][:n])
    for b, poison in ((src, "nan"), (sdesc, "nan"), (snorm, "nan"), (shas, "ff")):
        b.poison_guards(poison)
    out = src if alias else GuardedBuffer((n, 3), torch.float64, seed=25).fill_bytes(0xFF)
    tgt = GuardedBuffer((n, 3), torch.float64, seed=26).fill_bytes(0xFF)
    valid = GuardedBuffer(n, torch.uint8, seed=27).fill_bytes(0xFF)
    mdesc, sptr, mptr = d["mdesc"], sdesc.ptr(), d["mdesc"].ptr()
    if offset:
        esz = sdesc.itemsize
        shifted_s = GuardedBuffer(n * f + offset // esz, s["tdt"], seed=28)
        shifted_m = GuardedBuffer(mdesc.t.numel() + offset // esz, s["tdt"], seed=29)
        shifted_s.t[offset // esz:].copy_(sdesc.t.reshape(-1))
        shifted_m.t[offset // esz:].copy_(mdesc.t.reshape(-1))
        shifted_s.poison_guards("nan")
        shifted_m.poison_guards("nan")
        sptr, mptr = shifted_s.ptr() + offset, shifted_m.ptr() + offset
    T = r["T"]
    _lib.check(lib.vfm_icp_step_nearest_rows(src.ptr(), n, None if T is None else T.ctypes.data, None if T is None else out.ptr(), sptr,
                                             snorm.ptr(), shas.ptr(), sdesc.itemsize, f, d["keys"].ptr(), d["start"].ptr(), d["pts"].ptr(),
                                             mptr, d["mnorm"].ptr(), d["mhas"].ptr(), d["keys"].shape[0], VS, MAX_DIST, tgt.ptr(), valid.ptr(),
                                             ops._stream()), "icp_step_nearest_rows")
    torch.cuda.synchronize()
    bufs = dict(src=src, sdesc=sdesc, snorm=snorm, shas=shas, out=out, tgt=tgt, valid=valid, **d)
    if offset:
        bufs.update(shifted_s=shifted_s, shifted_m=shifted_m)
    _intact(bufs)
    return dict(src=src.numpy(), out=out.numpy(), out_bytes=out.body_bytes(), tgt=tgt.numpy(), valid=valid.numpy())


def _assert_equals_the_reference(got, r, n, kind, alias=False):
    np.testing.assert_array_equal(got["valid"], r["valid"][:n])
    np.testing.assert_array_equal(got["tgt"], r["tgt"][:n])
    if kind == "none":
        np.testing.assert_array_equal(got["src"], r["src"][:n])                # searched where they are: nothing moved, src_out not touched
        assert (got["out_bytes"] == 0xFF).all()
    else:
        np.testing.assert_array_equal(got["out"], r["moved"][:n])
        if not alias:
            np.testing.assert_array_equal(got["src"], r["src"][:n])            # the input is not written


@pytest.mark.parametrize("kind", STEPS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_the_search_equals_the_oracle(dtype, f, n, kind):
    s = _scene(dtype, f)
    r = s["ref"][kind]
    _assert_equals_the_reference(_search(s, n, kind), r, n, kind)
    if kind != "none" and n in (7, 1000):                                       # src aliasing src_out: moved in place
        _assert_equals_the_reference(_search(s, n, kind, alias=True), r, n, kind, alias=True)


@pytest.mark.parametrize("f", [64, 384])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_rows_off_16_bytes_give_the_same_answers(dtype, f):
    """a width whose rows could move in 16-byte units, from base pointers that are not 16-byte aligned: element by element, the same values"""
    s = _scene(dtype, f)
    got = _search(s, 1000, "rigid", offset=8)
    _assert_equals_the_reference(got, s["ref"]["rigid"], 1000, "rigid")


def test_the_candidates_of_a_full_neighbourhood_take_several_rounds():
    s = _scene(np.float32, 5)
    keys, start, pts = s["grid"]
    p = s["at"][0]
    v = np.trunc(p / VS).astype(np.int64)
    count = 0
    for a in range(-1, 2):
        for b in range(-1, 2):
            for c in range(-1, 2):
                k = ((v[0] + a + (1 << 20)) << 42) | ((v[1] + b + (1 << 20)) << 21) | (v[2] + c + (1 << 20))
                i = np.searchsorted(keys, k)
                assert i < len(keys) and keys[i] == k
                count += start[i + 1] - start[i]
    assert count == 27 * CAP == 540                                             # nine rounds of 64 lanes for source 0 (n = 1 searches it alone)


def test_the_entries_check_their_arguments():
    from vfmreg import _lib
    lib = _lib.load()
    T = np.eye(4)
    assert lib.vfm_icp_rows_stats(8, 2, 5, 4, 8, 8, None) == -1 and b"elem_bytes" in lib.vfm_last_error()
    assert lib.vfm_icp_rows_stats(8, 4, 5, 0, 8, 8, None) == -1 and b"sizes" in lib.vfm_last_error()
    assert lib.vfm_icp_rows_stats(8, 4, -1, 4, 8, 8, None) == -1 and b"sizes" in lib.vfm_last_error()
    assert lib.vfm_icp_rows_stats(None, 4, 5, 4, 8, 8, None) == -1 and b"null" in lib.vfm_last_error()
    assert lib.vfm_icp_rows_stats(None, 8, 0, 4, None, None, None) == 0        # n == 0: nothing to do
    head = lambda src, eb, f, T_, out: (src, 5, T_, out, 8, 8, 8, eb, f)   # noqa: E731
    tail = (8, 8, 8, 8, 8, 8, 3, 1.0, 1.0, 8, 8, None)
    assert lib.vfm_icp_step_nearest_rows(*head(8, 2, 4, None, None), *tail) == -1 and b"elem_bytes" in lib.vfm_last_error()
    assert lib.vfm_icp_step_nearest_rows(*head(8, 8, 0, None, None), *tail) == -1 and b"sizes" in lib.vfm_last_error()
    assert lib.vfm_icp_step_nearest_rows(*head(None, 8, 4, None, None), *tail) == -1 and b"null" in lib.vfm_last_error()
    assert lib.vfm_icp_step_nearest_rows(*head(8, 8, 4, T.ctypes.data, None), *tail) == -1 and b"null" in lib.vfm_last_error()
    no_map = (None, 8, None, None, None, None, 3, 1.0, 1.0, 8, 8, None)
    assert lib.vfm_icp_step_nearest_rows(*head(8, 8, 4, None, None), *no_map) == -1 and b"map" in lib.vfm_last_error()
    assert lib.vfm_icp_step_nearest_rows(None, 0, None, None, None, None, None, 4, 4, None, None, None, None, None, None, 0, 1.0, 1.0, None, None,
                                         None) == 0                             # n == 0: nothing to do


def test_an_empty_map_and_the_wrappers_argument_rules():
    from vfmreg import ops
    s = _scene(np.float32, 5)
    d = s["dev"]
    src = torch.from_numpy(s["ref"]["none"]["src"][:7]).cuda()
    sdesc = torch.from_numpy(s["sdesc"][:7]).cuda()
    snorm, shas = ops.icp_rows_stats(sdesc)
    np.testing.assert_array_equal(snorm.cpu().numpy(), s["snorm"][:7])
    grid = (d["keys"].t, d["start"].t, d["pts"].t, d["mdesc"].t, d["mnorm"].t, d["mhas"].t)
    moved, tgt, valid = ops.icp_step_nearest_rows(src, None, sdesc, snorm, shas, *grid, VS, MAX_DIST)
    assert moved is src
    np.testing.assert_array_equal(tgt.cpu().numpy(), s["ref"]["none"]["tgt"][:7])
    np.testing.assert_array_equal(valid.cpu().numpy(), s["ref"]["none"]["valid"][:7])
    T = s["ref"]["rigid"]["T"]
    src_r = torch.from_numpy(s["ref"]["rigid"]["src"][:7]).cuda()
    moved, tgt, valid = ops.icp_step_nearest_rows(src_r, T, sdesc, snorm, shas, *grid, VS, MAX_DIST, src_out=src_r)
    assert moved is src_r
    np.testing.assert_array_equal(moved.cpu().numpy(), s["ref"]["rigid"]["moved"][:7])
    np.testing.assert_array_equal(tgt.cpu().numpy(), s["ref"]["rigid"]["tgt"][:7])
    # an empty map: nothing is found
    empty = (torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
             torch.zeros((0, 3), dtype=torch.float64, device="cuda"), torch.zeros((0, 5), dtype=torch.float32, device="cuda"),
             torch.zeros(0, dtype=torch.float64, device="cuda"), torch.zeros(0, dtype=torch.uint8, device="cuda"))
    _, tgt, valid = ops.icp_step_nearest_rows(src, None, sdesc, snorm, shas, *empty, VS, MAX_DIST)
    assert not valid.any() and not tgt.any()
    # the rules
    with pytest.raises(TypeError, match="map_desc"):
        ops.icp_step_nearest_rows(src, None, sdesc.double(), snorm, shas, *grid, VS, MAX_DIST)
    with pytest.raises(ValueError, match="Invalid shape"):
        ops.icp_step_nearest_rows(src, None, sdesc[:, :4].contiguous(), snorm, shas, *grid, VS, MAX_DIST)
    with pytest.raises(ValueError, match="contiguous"):
        ops.icp_step_nearest_rows(src, None, sdesc.t().contiguous().t(), snorm, shas, *grid, VS, MAX_DIST)
    with pytest.raises(ValueError, match="one entry per row"):
        ops.icp_step_nearest_rows(src, None, sdesc, snorm[:5], shas, *grid, VS, MAX_DIST)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.icp_step_nearest_rows(src.cpu(), None, sdesc, snorm, shas, *grid, VS, MAX_DIST)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.icp_rows_stats(sdesc.cpu())
    with pytest.raises(TypeError, match="float32 or float64"):
        ops.icp_rows_stats(sdesc.half())
    with pytest.raises(ValueError, match="4 x 4"):
        ops.icp_step_nearest_rows(src, np.eye(3), sdesc, snorm, shas, *grid, VS, MAX_DIST)
