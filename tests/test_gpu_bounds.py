"""The buffer contract of include/vfmreg.h, executed: "the caller owns every buffer; scratch is caller-provided and sized by the matching
vfm_*_workspace_bytes()".  Every entry point below is called with EVERY input, output and workspace in a GuardedBuffer
(tests/guarded.py: [guard | body | guard], seeded random guards), workspaces and prepared operands at exactly the size the library
reports, and every call must show five properties:

  1. guards intact   -- no byte before or after any buffer is written;
  2. inputs unchanged -- byte for byte (documented in/out arguments excepted);
  3. no dependence on earlier contents -- outputs pre-filled with 0 and with -1 / NaN (bytes 0xFF) give the same result; a workspace
     used first by a LARGER call of the same entry point (stale counters that are plausible in-range values, as product reuse leaves
     them) gives the same result as a fresh, zeroed one -- and so does, for the k-best search, a fresh one filled with bytes 0xFF;
  4. no reads past the ends of inputs -- guards of every input poisoned (NaN for floating-point data, 0 -- a valid index -- for index
     arrays, 0x00 then 0xFF for images, 0x00 for opaque prepared operands) give the same result, bit for bit;
  5. still the reference answer at these edge shapes (oracle.oracle, tests/fpfh_oracle.py; for the ViT the unguarded forward).

Shapes sit at and next to the kernels' tile sizes (32 / 64 / 128-row tiles, 128-row map chunks, 4-points-per-wave lifting).  Fill and
poison values are chosen so they can never become far addresses: a stray read or write lands in a guard, never outside the test's memory.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.guarded import GuardedBuffer  # noqa: E402

pytestmark = pytest.mark.gpu

IN, OUT, INOUT, SCRATCH = "in", "out", "inout", "scratch"
NAN, ZERO, FF = "nan", "zero", "ff"

FAST, EXACT = 0, 1
PREP_DEFAULT, PREP_PERSISTENT, PREP_INTERLEAVED, PREP_MX6, PREP_MX6_HALF = 0, 1, 2, 8, 16
REC_BEST, REC_TOP2, REC_HALF_FUSED, REC_MX6, REC_MX6_HALF_FUSED = 0, 1, 4, 5, 8
ROWS_F32, ROWS_F16 = 0, 1


def _lib():
    from vfmreg import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(rc, what):
    _lib().check(rc, what)


_TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.float16): torch.float16,
             np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


class Buf:
    """One argument of a call.  role IN / INOUT: ``data`` (numpy) is its content; OUT: ``shape`` / ``dtype``; SCRATCH: an opaque
    buffer the call writes and reads back itself (prepared operands) -- pre-filled like an output, poisoned like an opaque input, not
    compared byte-wise (what it feeds is).  ``view(results, arr)`` selects what of an output is defined (a device count's prefix)."""

    def __init__(self, role, data=None, shape=None, dtype=None, poison=None, view=None, host=False):
        self.role = role
        self.host = host
        self.view = view
        if data is not None:
            self.data = np.ascontiguousarray(data)
            self.shape, self.np_dtype = self.data.shape, self.data.dtype
        else:
            self.data = None
            self.shape, self.np_dtype = tuple(np.atleast_1d(shape)), np.dtype(dtype)
        self.dtype = _TORCH_DT[self.np_dtype]
        if poison is None:
            poison = (NAN,) if self.np_dtype.kind == "f" else (ZERO,)
        self.poison = tuple(poison)


class Case:
    def __init__(self, name, bufs, call, ws_bytes=None, ref=None, big=None, cfg=None):
        self.name, self.bufs, self.call, self.ws_bytes, self.ref, self.big, self.cfg = name, bufs, call, ws_bytes, ref, big, cfg


def _bound(cfg):
    if not cfg:
        return contextlib.nullcontext()
    L = _lib()
    return L.using(L.Config(**cfg))


def _run(case, out_byte=0x00, poison_round=None, ws=None, tag="", ws_byte=0x00):
    where = f"{case.name} [{tag}]"
    bufs = {}
    for i, (name, s) in enumerate(case.bufs.items()):
        g = GuardedBuffer(s.shape, s.dtype, device="cpu" if s.host else "cuda", seed=i, pin_memory=s.host)
        if s.role in (IN, INOUT):
            g.set(torch.from_numpy(s.data))
        else:
            g.fill_bytes(out_byte)
        if poison_round is not None and s.role in (IN, SCRATCH):
            g.poison_guards(s.poison[min(poison_round, len(s.poison) - 1)] if s.role == IN else ZERO)
        bufs[name] = g
    if ws is None and case.ws_bytes is not None:
        ws = GuardedBuffer(case.ws_bytes, torch.uint8, seed=97).fill_bytes(ws_byte)
    with _bound(case.cfg):
        case.call(bufs, ws)
    torch.cuda.synchronize()
    for name, g in list(bufs.items()) + ([("workspace", ws)] if ws is not None else []):
        chk = g.intact()
        assert chk, f"{where}: {name}: {chk!r}"
    for name, s in case.bufs.items():
        if s.role == IN:
            assert np.array_equal(bufs[name].body_bytes(), s.data.reshape(-1).view(np.uint8)), f"{where}: input {name} was written"
    return {name: bufs[name].numpy() for name, s in case.bufs.items() if s.role in (OUT, INOUT)}


def _same(case, A, B, what):
    for name, s in case.bufs.items():
        if s.role not in (OUT, INOUT):
            continue
        a, b = A[name], B[name]
        if s.view is not None:
            a, b = s.view(A, a), s.view(B, b)
            assert a.shape == b.shape, f"{case.name}: {name}: {a.shape} vs {b.shape} {what}"
        ab, bb = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
        if not np.array_equal(ab, bb):
            first = int(np.flatnonzero(ab != bb)[0]) // max(a.itemsize, 1)
            pytest.fail(f"{case.name}: {name} differs {what} (first at flat element {first}: {a.reshape(-1)[first]} vs "
                        f"{b.reshape(-1)[first]})")


def check_case(case, ws_ff=False):
    """The five properties of the module docstring for one call.  ``ws_ff``: one more run, in a fresh workspace pre-filled with bytes
    0xFF instead of 0 (counts of 4 billion, bounds above every score, list entries of -1), must give the same outputs."""
    A = _run(case, 0x00, tag="outputs pre-filled with 0")
    B = _run(case, 0xFF, tag="outputs pre-filled with -1 / NaN")
    _same(case, A, B, "between outputs pre-filled with 0 and with -1 / NaN")
    rounds = max([len(s.poison) for s in case.bufs.values() if s.role == IN] + [1])
    for r in range(rounds):
        P = _run(case, 0x00, poison_round=r, tag=f"input guards poisoned, round {r}")
        _same(case, A, P, f"with the guards of the inputs poisoned (round {r})")
    if case.ws_bytes is not None and case.big is not None:
        big = case.big()
        assert big.ws_bytes >= case.ws_bytes, (big.ws_bytes, case.ws_bytes)
        W = GuardedBuffer(max(big.ws_bytes, 1), torch.uint8, seed=98).fill_bytes(0)
        _run(big, 0x00, ws=W, tag="the larger call")
        R = _run(case, 0x00, ws=W, tag="workspace reused from a larger call")
        _same(case, A, R, "in a workspace used by a larger call first")
    if ws_ff and case.ws_bytes is not None:
        F = _run(case, 0x00, ws_byte=0xFF, tag="workspace pre-filled with bytes 0xFF")
        _same(case, A, F, "in a workspace pre-filled with bytes 0xFF")
    if case.ref is not None:
        case.ref(A)
    return A


def _prefix(count_name, scale=1):
    return lambda res, a: a[:int(res[count_name].reshape(-1)[0]) * scale]


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    return o


# ================================================================================================================ matcher
def _desc_pair(n, m, d, seed):
    """Half the queries are noisy copies of map rows (cosine ~0.96, above the 0.8 gate), the rest background (< 0.3)."""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((m, d)).astype(np.float32)
    q = rng.standard_normal((n, d)).astype(np.float32)
    k = (n + 1) // 2
    pick = rng.integers(0, m, k)
    q[:k] = b[pick] + 0.3 * rng.standard_normal((k, d)).astype(np.float32)
    if n > 2:
        q[n - 1] = 0.0   # a zero-norm query row (idx 0, sim 0 / unresolved)
    return q, b


_REF_CACHE = {}


def _match_ref(orc, q, b):
    key = (q.shape, b.shape, q.tobytes()[:64], b.tobytes()[:64], q.dtype.str)
    if key not in _REF_CACHE:
        qn, _ = orc.l2norm_rows(q.astype(np.float32))
        bn, _ = orc.l2norm_rows(b.astype(np.float32))
        _REF_CACHE.clear()
        _REF_CACHE[key] = (orc.match_ip_top1_bruteforce(qn, bn) if q.shape[0] * b.shape[0] <= 1 << 18 else orc.match_ip_top1(qn, bn))
    return _REF_CACHE[key]


def _match_check(orc, q, b, gate, name):
    def ref(A):
        idx, sim = A["idx"], A["sim"]
        ridx, rsim = _match_ref(orc, q, b)
        if gate is None:
            np.testing.assert_array_equal(idx, ridx, err_msg=name)
            np.testing.assert_array_equal(sim, rsim, err_msg=name)
        else:
            ok = idx >= 0
            np.testing.assert_array_equal(idx[ok], ridx[ok], err_msg=name)
            np.testing.assert_array_equal(sim[ok], rsim[ok], err_msg=name)
            assert (rsim[~ok] < gate).all() and (sim[~ok] == -2.0).all(), name
            assert ok[:(len(q) + 1) // 2].all(), f"{name}: a planted match above the gate was left unresolved"
    return ref


def match_case(form, n, m, d, prec=FAST, gate=None, records=None, sched=PREP_DEFAULT, rows=ROWS_F32, seed=1, orc=None):
    L = _lib()
    lib = L.load()
    q, b = _desc_pair(n, m, d, seed + n + m + d)
    if rows == ROWS_F16:
        q, b = q.astype(np.float16), b.astype(np.float16)
    name = f"{form} n={n} m={m} d={d} prec={prec} gate={gate} records={records} sched={sched} rows={rows}"
    bufs = dict(q=Buf(IN, q), b=Buf(IN, b), idx=Buf(OUT, shape=n, dtype=np.int64), sim=Buf(OUT, shape=n, dtype=np.float32))
    g = -np.inf if gate is None else float(gate)
    big = lambda: match_case(form, 2 * n + 3, 2 * m + 5, d, prec, gate, records, sched, rows, seed + 1)   # noqa: E731
    if form in ("ip_top1", "ip_top1_gated"):
        ws = lib.vfm_match_ip_top1_workspace_bytes(n, m, d, prec)

        def call(B, W):
            if form == "ip_top1":
                _chk(lib.vfm_match_ip_top1(B["q"].ptr(), n, B["b"].ptr(), m, d, prec, B["idx"].ptr(), B["sim"].ptr(), W.ptr(), W.nbytes,
                                           _stream()), name)
            else:
                _chk(lib.vfm_match_ip_top1_gated(B["q"].ptr(), n, B["b"].ptr(), m, d, prec, g, B["idx"].ptr(), B["sim"].ptr(), W.ptr(),
                                                 W.nbytes, _stream()), name)
        return Case(name, bufs, call, ws, _match_check(orc, q, b, gate, name) if orc else None, big)
    if form == "probe":
        bufs = dict(q=Buf(IN, q), b=Buf(IN, b))
    bufs["qp"] = Buf(SCRATCH, shape=lib.vfm_match_prepared_bytes(n, d), dtype=np.uint8)
    bufs["bp"] = Buf(SCRATCH, shape=lib.vfm_match_prepared_bytes(m, d), dtype=np.uint8)
    ws = lib.vfm_match_search_workspace_bytes(n, m, d)
    if form == "probe":
        bufs["count"] = Buf(OUT, shape=1, dtype=np.int32, host=True)

    def call(B, W):
        st = _stream()
        qx, bx, qp, bp = B["q"].ptr(), B["b"].ptr(), B["qp"].ptr(), B["bp"].ptr()
        if form == "prepared":
            _chk(lib.vfm_match_prepare(qx, n, d, qp, st), name)
            _chk(lib.vfm_match_prepare(bx, m, d, bp, st), name)
            _chk(lib.vfm_match_search_prepared(qx, qp, n, bx, bp, m, d, B["idx"].ptr(), B["sim"].ptr(), W.ptr(), W.nbytes, st), name)
        elif form == "split":
            _chk(lib.vfm_match_prepare2(bx, m, bp, qx, n, qp, d, st), name)
            _chk(lib.vfm_match_search_coarse(qp, n, bp, m, d, W.ptr(), W.nbytes, st), name)
            _chk(lib.vfm_match_search_finish(qx, qp, n, bx, bp, m, d, B["idx"].ptr(), B["sim"].ptr(), W.ptr(), W.nbytes, st), name)
        elif form == "gated":
            _chk(lib.vfm_match_prepare2_gated(bx, m, bp, qx, n, qp, d, st), name)
            _chk(lib.vfm_match_search_coarse_gated(qp, n, bp, m, d, W.ptr(), W.nbytes, st), name)
            _chk(lib.vfm_match_search_finish_gated(qx, qp, n, bx, bp, m, d, B["idx"].ptr(), B["sim"].ptr(), W.ptr(), W.nbytes, g, st), name)
        elif form == "gated_p":
            _chk(lib.vfm_match_prepare2_gated_p(bx, m, bp, qx, n, qp, d, sched, st), name)
            _chk(lib.vfm_match_search_coarse_gated_g(qp, n, bp, m, d, W.ptr(), W.nbytes, records, g, st), name)
            _chk(lib.vfm_match_search_finish_gated_r(qx, qp, n, bx, bp, m, d, B["idx"].ptr(), B["sim"].ptr(), W.ptr(), W.nbytes, g, records,
                                                     st), name)
        elif form == "gated_t":
            _chk(lib.vfm_match_prepare2_gated_t(bx, rows, m, bp, qx, rows, n, qp, d, sched, st), name)
            _chk(lib.vfm_match_search_coarse_gated_r(qp, n, bp, m, d, W.ptr(), W.nbytes, records, st), name)
            _chk(lib.vfm_match_search_finish_gated_t(qx, rows, qp, n, bx, rows, bp, m, d, B["idx"].ptr(), B["sim"].ptr(), W.ptr(), W.nbytes,
                                                     g, records, st), name)
        elif form == "probe":
            _chk(lib.vfm_match_prepare2_gated(bx, m, bp, qx, n, qp, d, st), name)
            _chk(lib.vfm_match_search_probe_half(qp, n, bp, m, d, W.ptr(), W.nbytes, g, B["count"].ptr(), st), name)
        else:
            raise ValueError(form)

    ref = None
    if orc is not None and form != "probe":
        ref = _match_check(orc, q.astype(np.float32), b.astype(np.float32), gate, name)
    return Case(name, bufs, call, ws, ref, big)


MATCH = [
    ("ip_top1", dict(n=1, m=1, d=128)), ("ip_top1", dict(n=63, m=65, d=128)), ("ip_top1", dict(n=257, m=2049, d=384)),
    ("ip_top1", dict(n=65, m=129, d=768)), ("ip_top1", dict(n=63, m=65, d=384, prec=EXACT)),
    ("ip_top1", dict(n=1, m=257, d=768, prec=EXACT)),
    ("ip_top1_gated", dict(n=257, m=1025, d=384, gate=0.8)), ("ip_top1_gated", dict(n=65, m=63, d=768, gate=0.8)),
    ("ip_top1_gated", dict(n=2049, m=1023, d=384, gate=0.8)),
    ("prepared", dict(n=1, m=65, d=128)), ("prepared", dict(n=65, m=257, d=384)), ("prepared", dict(n=257, m=1, d=768)),
    ("prepared", dict(n=2049, m=1025, d=384)),
    ("split", dict(n=63, m=129, d=384)), ("split", dict(n=257, m=127, d=768)),
    ("gated", dict(n=257, m=1025, d=384, gate=0.8)), ("gated", dict(n=65, m=4097, d=768, gate=0.8)),
    ("gated", dict(n=1, m=129, d=384, gate=0.8)),
    ("gated_p", dict(n=2049, m=1025, d=384, gate=0.8, records=REC_BEST, sched=PREP_PERSISTENT)),
    ("gated_p", dict(n=257, m=1023, d=384, gate=0.8, records=REC_TOP2, sched=PREP_INTERLEAVED)),
    ("gated_p", dict(n=2049, m=1025, d=384, gate=0.8, records=REC_TOP2)),
    ("gated_p", dict(n=2049, m=1025, d=384, gate=0.8, records=REC_HALF_FUSED)),
    ("gated_p", dict(n=2049, m=1025, d=384, gate=0.8, records=REC_MX6, sched=PREP_MX6)),
    ("gated_p", dict(n=2049, m=4097, d=384, gate=0.8, records=REC_MX6, sched=PREP_MX6)),
    ("gated_p", dict(n=2049, m=1025, d=384, gate=0.8, records=REC_MX6_HALF_FUSED, sched=PREP_MX6_HALF)),
    ("gated_p", dict(n=2049, m=1023, d=768, gate=0.8, records=REC_MX6_HALF_FUSED, sched=PREP_MX6_HALF)),
    ("gated_t", dict(n=257, m=1025, d=384, gate=0.8, records=REC_BEST, rows=ROWS_F16)),
    ("gated_t", dict(n=2049, m=1023, d=384, gate=0.8, records=REC_MX6, sched=PREP_MX6, rows=ROWS_F16)),
    ("probe", dict(n=257, m=1025, d=384, gate=0.8)), ("probe", dict(n=2049, m=129, d=384, gate=0.8)),
]


@pytest.mark.parametrize("form,kw", MATCH, ids=[f"{f}-" + "-".join(f"{k}{v}" for k, v in kw.items()) for f, kw in MATCH])
def test_matcher_stays_in_its_buffers(orc, form, kw):
    check_case(match_case(form, orc=orc, **kw))


@pytest.mark.parametrize("n", [1, 65, 2049])
def test_threshold_compact_stays_in_its_buffers(orc, n):
    lib = _lib().load()
    rng = np.random.default_rng(n)
    m = 300
    sim = rng.uniform(-1, 1, n).astype(np.float32)
    idx = rng.integers(0, m, n).astype(np.int64)
    qx, bx = rng.uniform(-50, 50, (n, 3)), rng.uniform(-50, 50, (m, 3))
    thr = 0.25
    pre = _prefix("count")
    bufs = dict(sim=Buf(IN, sim), idx=Buf(IN, idx), q_xyz=Buf(IN, qx), b_xyz=Buf(IN, bx),
                keep=Buf(OUT, shape=n, dtype=np.int64, view=pre), count=Buf(OUT, shape=1, dtype=np.int64),
                corres=Buf(OUT, shape=(n, 2), dtype=np.int32, view=pre), src=Buf(OUT, shape=(n, 3), dtype=np.float64, view=pre),
                tgt=Buf(OUT, shape=(n, 3), dtype=np.float64, view=pre))

    def call(B, W):
        _chk(lib.vfm_threshold_compact(B["sim"].ptr(), B["idx"].ptr(), n, thr, B["keep"].ptr(), B["count"].ptr(), B["corres"].ptr(),
                                       B["q_xyz"].ptr(), B["b_xyz"].ptr(), B["src"].ptr(), B["tgt"].ptr(), _stream()), "threshold_compact")

    def ref(A):
        keep = orc.threshold_compact(sim, thr)
        k = len(keep)
        assert int(A["count"][0]) == k
        np.testing.assert_array_equal(A["keep"][:k], keep)
        np.testing.assert_array_equal(A["corres"][:k], np.stack([keep, idx[keep]], 1))
        np.testing.assert_array_equal(A["src"][:k], qx[keep])
        np.testing.assert_array_equal(A["tgt"][:k], bx[idx[keep]])
    check_case(Case(f"threshold_compact n={n}", bufs, call, None, ref))


# ================================================================================================================ L2
def _l2_pair(n, m, d, seed):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((m, d)).astype(np.float32)
    a = rng.standard_normal((n, d)).astype(np.float32)
    k = n // 2
    a[:k] = b[rng.integers(0, m, k)] + 0.05 * rng.standard_normal((k, d)).astype(np.float32)
    return a, b


def mutual_l2_case(n, m, d, prec, mutual, orc=None):
    lib = _lib().load()
    a, b = _l2_pair(n, m, d, n + m + d)
    name = f"mutual_l2 n={n} m={m} d={d} prec={prec} mutual={mutual}"
    bufs = dict(a=Buf(IN, a), b=Buf(IN, b), nn_ab=Buf(OUT, shape=n, dtype=np.int64), d2=Buf(OUT, shape=n, dtype=np.float64))
    if mutual:
        bufs["nn_ba"] = Buf(OUT, shape=m, dtype=np.int64)
    ws = lib.vfm_match_mutual_l2_workspace_bytes(n, m, d, prec, int(mutual))

    def call(B, W):
        _chk(lib.vfm_match_mutual_l2(B["a"].ptr(), n, B["b"].ptr(), m, d, prec, B["nn_ab"].ptr(), B["d2"].ptr(),
                                     B["nn_ba"].ptr() if mutual else None, W.ptr(), W.nbytes, _stream()), name)

    def ref(A):
        i_ref, dist_ref = orc.nn_l2(a, b)
        np.testing.assert_array_equal(A["nn_ab"], i_ref, err_msg=name)
        np.testing.assert_array_equal(np.sqrt(A["d2"]), dist_ref, err_msg=name)
        if mutual:
            np.testing.assert_array_equal(A["nn_ba"], orc.nn_l2(b, a)[0], err_msg=name)
    return Case(name, bufs, call, ws, ref if orc else None, lambda: mutual_l2_case(2 * n + 3, 2 * m + 5, d, prec, mutual))


def mutual_pairs_case(n, m, d, orc=None):
    lib = _lib().load()
    a, b = _l2_pair(n, m, d, 7 * n + m + d)
    name = f"mutual_pairs n={n} m={m} d={d}"
    pre = _prefix("count")
    bufs = dict(a=Buf(IN, a), b=Buf(IN, b), idx0=Buf(OUT, shape=n, dtype=np.int64, view=pre),
                idx1=Buf(OUT, shape=n, dtype=np.int64, view=pre), count=Buf(OUT, shape=1, dtype=np.int64),
                nn_ab=Buf(OUT, shape=n, dtype=np.int64), d2=Buf(OUT, shape=n, dtype=np.float64))
    ws = lib.vfm_match_mutual_pairs_workspace_bytes(n, m, d)

    def call(B, W):
        _chk(lib.vfm_match_mutual_pairs(B["a"].ptr(), n, B["b"].ptr(), m, d, B["idx0"].ptr(), B["idx1"].ptr(), B["count"].ptr(),
                                        B["nn_ab"].ptr(), B["d2"].ptr(), W.ptr(), W.nbytes, _stream()), name)

    def ref(A):
        i0, i1 = orc.find_correspondences(a, b)
        k = int(A["count"][0])
        assert k == len(i0), name
        np.testing.assert_array_equal(A["idx0"][:k], i0, err_msg=name)
        np.testing.assert_array_equal(A["idx1"][:k], i1, err_msg=name)
        i_ref, dist_ref = orc.nn_l2(a, b)
        np.testing.assert_array_equal(A["nn_ab"], i_ref, err_msg=name)
        np.testing.assert_array_equal(np.sqrt(A["d2"]), dist_ref, err_msg=name)
    return Case(name, bufs, call, ws, ref if orc else None, lambda: mutual_pairs_case(2 * n + 3, 2 * m + 5, d))


L2 = [(1, 257, 7), (65, 1, 126), (257, 63, 384), (63, 1025, 768), (1, 129, 384), (129, 2049, 384)]


@pytest.mark.parametrize("n,m,d", L2)
@pytest.mark.parametrize("prec", [FAST, EXACT])
def test_mutual_l2_stays_in_its_buffers(orc, n, m, d, prec):
    for mutual in (True, False):
        check_case(mutual_l2_case(n, m, d, prec, mutual, orc))


@pytest.mark.parametrize("n,m,d", L2)
def test_mutual_pairs_stays_in_its_buffers(orc, n, m, d):
    check_case(mutual_pairs_case(n, m, d, orc))


@pytest.mark.parametrize("n,d", [(1, 384), (65, 4), (257, 124), (63, 768), (2049, 384)])
def test_l2norm_rows_stays_in_its_buffers(orc, n, d):
    lib = _lib().load()
    x = np.random.default_rng(n + d).standard_normal((n, d)).astype(np.float32)
    if n > 2:
        x[1] = 0.0
    bufs = dict(x=Buf(INOUT, x), inv=Buf(OUT, shape=n, dtype=np.float32))

    def call(B, W):
        _chk(lib.vfm_l2norm_rows_f32(B["x"].ptr(), n, d, B["inv"].ptr(), _stream()), "l2norm")

    def ref(A):
        xn, inv = orc.l2norm_rows(x)
        np.testing.assert_array_equal(A["x"], xn)
        np.testing.assert_array_equal(A["inv"], inv)
    check_case(Case(f"l2norm n={n} d={d}", bufs, call, None, ref))


# ================================================================================================================ solve
def _ransac_data(c_max, seed):
    rng = np.random.default_rng(seed)
    ns, nt = c_max + 17, c_max + 29
    src = rng.uniform(-30, 30, (ns, 3))
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    R *= np.sign(np.linalg.det(R))
    tgt = rng.uniform(-30, 30, (nt, 3))
    ps, pt = rng.permutation(ns)[:c_max], rng.permutation(nt)[:c_max]
    tgt[pt] = src[ps] @ R.T + np.array([1.0, -2.0, 0.5]) + 0.01 * rng.standard_normal((c_max, 3))
    out = rng.random(c_max) < 0.3
    tgt[pt[out]] = rng.uniform(-30, 30, (out.sum(), 3))
    return src, tgt, np.stack([ps, pt], 1).astype(np.int32)


def ransac_case(count, c_max, bounded, fused, orc=None, n_iter=300, max_dist=0.5):
    lib = _lib().load()
    src, tgt, corres = _ransac_data(c_max, count * 7 + c_max)
    name = f"ransac count={count} c_max={c_max} bounded={bounded} fused={fused}"
    bufs = dict(src=Buf(IN, src), tgt=Buf(IN, tgt), corres=Buf(IN, corres), count=Buf(IN, np.array([count], np.int64)),
                T=Buf(OUT, shape=16, dtype=np.float64), fit=Buf(OUT, shape=1, dtype=np.float64), rmse=Buf(OUT, shape=1, dtype=np.float64),
                mask=Buf(OUT, shape=c_max, dtype=np.uint8), best=Buf(OUT, shape=1, dtype=np.int32))
    if bounded:
        bufs["bad"] = Buf(INOUT, np.zeros(1, np.int32))
    ws = lib.vfm_ransac_workspace_bytes(c_max, n_iter)

    def call(B, W):
        p = {k: B[k].ptr() for k in B}
        if bounded:
            _chk(lib.vfm_ransac_corr_bounded(p["src"], len(src), p["tgt"], len(tgt), p["corres"], p["count"], c_max, max_dist, n_iter, 42,
                                             p["T"], p["fit"], p["rmse"], p["mask"], p["best"], p["bad"], W.ptr(), W.nbytes, _stream()), name)
        else:
            _chk(lib.vfm_ransac_corr(p["src"], p["tgt"], p["corres"], p["count"], c_max, max_dist, n_iter, 42, p["T"], p["fit"], p["rmse"],
                                     p["mask"], p["best"], W.ptr(), W.nbytes, _stream()), name)

    def ref(A):
        r = orc.ransac_corr(src, tgt, corres[:count], max_dist, n_iter, seed=42)
        np.testing.assert_array_equal(A["T"].reshape(4, 4), r.transformation, err_msg=name)
        assert A["fit"][0] == r.fitness and A["rmse"][0] == r.inlier_rmse and A["best"][0] == r.best_hyp, name
        np.testing.assert_array_equal(A["mask"][:count], r.inlier_mask, err_msg=name)
        assert not A["mask"][count:].any(), name
        if bounded:
            assert A["bad"][0] == 0, name
    return Case(name, bufs, call, ws, ref if orc else None,
                lambda: ransac_case(min(2 * count + 3, 2 * c_max + 7), 2 * c_max + 7, bounded, fused, n_iter=n_iter, max_dist=max_dist),
                cfg=dict(ransac_fused=fused))


@pytest.mark.parametrize("count,c_max", [(3, 3), (64, 64), (65, 65), (1000, 1000), (3, 70), (65, 1000)])
@pytest.mark.parametrize("fused", [2, 1, 0])
def test_ransac_stays_in_its_buffers(orc, count, c_max, fused):
    for bounded in (False, True):
        check_case(ransac_case(count, c_max, bounded, fused, orc))


@pytest.mark.parametrize("n", [3, 64, 65, 1000])
@pytest.mark.parametrize("weighted", [False, True])
def test_kabsch_batched_stays_in_its_buffers(orc, n, weighted):
    lib = _lib().load()
    rng = np.random.default_rng(n)
    b = 5
    A_ = rng.uniform(-20, 20, (b, n, 3))
    B_ = A_ @ np.linalg.qr(rng.standard_normal((3, 3)))[0] + 1.5 + 0.01 * rng.standard_normal((b, n, 3))
    A_[3] = A_[3, 0]   # degenerate sample
    w = rng.uniform(0.1, 1, (b, n))
    eps = 1e-6 if weighted else 0.0
    bufs = dict(A=Buf(IN, A_), B=Buf(IN, B_), T=Buf(OUT, shape=(b, 16), dtype=np.float64), valid=Buf(OUT, shape=b, dtype=np.int32))
    if weighted:
        bufs["w"] = Buf(IN, w)

    def call(B, W):
        _chk(lib.vfm_kabsch_batched(B["A"].ptr(), B["B"].ptr(), B["w"].ptr() if weighted else None, b, n, eps, B["T"].ptr(),
                                    B["valid"].ptr(), _stream()), "kabsch")

    def ref(A):
        for i in range(b):
            Tr, ok = orc.kabsch(A_[i], B_[i], w[i] if weighted else None, eps)
            assert bool(A["valid"][i]) == ok
            np.testing.assert_array_equal(A["T"][i].reshape(4, 4), Tr)
    check_case(Case(f"kabsch n={n} weighted={weighted}", bufs, call, None, ref))


# ================================================================================================================ lifting
PROJ_N = [1, 2, 3, 5, 403]


def _proj_setup(golden, mode, n):
    """A subset of the projection fixtures' points: half of them from the points the reference keeps."""
    if mode == 0:
        g = golden("proj_nclt.npz")
        sub = float(g["subsample"])
        mats, fc, win, image, H, W = [g["T_c_body"], g["K"]], None, g["coords"] // int(sub), g["image"], 0, 0
    elif mode == 1:
        g = golden("proj_oxf.npz")
        sub = float(g["subsample"])
        mats, fc, win, image, H, W = [g["lidar_in_ego"], g["cam_in_ego"], g["Ginv"]], g["fc"], None, None, int(g["H"]), int(g["W"])
    else:
        g = golden("proj_kitti.npz")
        sub = float(g["subsample"])
        mats, fc, win, image, H, W = [g["P2Tr"]], None, None, None, int(g["H"]), int(g["W"])
    pcl = g["pcl"].astype(np.float64)
    rng = np.random.default_rng(n + mode)
    seen = rng.permutation(g["idx"])[:(n + 1) // 2]
    rest = rng.permutation(np.setdiff1d(np.arange(pcl.shape[1]), seen))[:n - len(seen)]
    sel = np.sort(np.r_[seen, rest])
    return np.ascontiguousarray(pcl[:, sel]), mats, fc, sub, win, image, H, W


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", PROJ_N)
def test_project_pinhole_stays_in_its_buffers(orc, golden, mode, n):
    lib = _lib().load()

    def make(n_):
        pcl, mats, fc, sub, win, image, H, W = _proj_setup(golden, mode, n_)
        if image is not None:
            H, W = image.shape[0], image.shape[1]
        flat = [0.0] * 48
        for k, mm in enumerate(mats):
            vals = np.asarray(mm, np.float64).reshape(-1).tolist()
            flat[16 * k:16 * k + len(vals)] = vals
        mats_c = (C.c_double * 48)(*flat)
        fc_c = (C.c_double * 4)(*([float(x) for x in fc] if fc is not None else [0.0] * 4))
        win_c = (C.c_int64 * 4)(*([int(x) for x in win] if win is not None else [0] * 4))
        pre = _prefix("count")
        bufs = dict(pcl=Buf(IN, pcl), u=Buf(OUT, shape=n_, dtype=np.int32, view=pre), v=Buf(OUT, shape=n_, dtype=np.int32, view=pre),
                    idx=Buf(OUT, shape=n_, dtype=np.int64, view=pre), count=Buf(OUT, shape=1, dtype=np.int64))
        if image is not None:
            bufs["image"] = Buf(IN, image, poison=(ZERO, FF))
        name = f"project mode={mode} n={n_}"

        def call(B, Wk):
            _chk(lib.vfm_project_pinhole_f64(mode, B["pcl"].ptr(), n_, C.cast(mats_c, C.c_void_p), C.cast(fc_c, C.c_void_p), sub,
                                             C.cast(win_c, C.c_void_p), B["image"].ptr() if image is not None else None, H, W,
                                             B["u"].ptr(), B["v"].ptr(), B["idx"].ptr(), B["count"].ptr(), Wk.ptr(), Wk.nbytes,
                                             _stream()), name)

        def ref(A):
            u, v, idx = orc.project(mode, pcl, mats, fc, sub, win, image, H, W)
            k = int(A["count"][0])
            assert k == len(idx), name
            np.testing.assert_array_equal(A["idx"][:k], idx)
            np.testing.assert_array_equal(A["u"][:k], u)
            np.testing.assert_array_equal(A["v"][:k], v)
        return Case(name, bufs, call, lib.vfm_project_workspace_bytes(n_), ref, lambda: make(2 * n_ + 5))
    check_case(make(n))


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("Cc", [384, 768, 30])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 403])
def test_gather_bilinear_stays_in_its_buffers(orc, rot, Cc, k):
    lib = _lib().load()
    rng = np.random.default_rng(k + Cc + rot)
    gh, gw, H, W, npts = 16, 21, 120, 160, 2 * k + 9
    grid = rng.standard_normal((gh, gw, Cc)).astype(np.float32)
    img = rng.integers(0, 255, (H, W, 3)).astype(np.uint8)
    img[rng.random((H, W)) < 0.1] = 0    # black pixels
    # u / v address the (rotated, for rot 1) upsampled image
    uh, vh = (W, H) if rot == 0 else (H, W)
    u = rng.integers(0, uh, k).astype(np.int32)
    v = rng.integers(0, vh, k).astype(np.int32)
    idx = rng.permutation(npts)[:k].astype(np.int64)
    desc0 = rng.standard_normal((npts, Cc)).astype(np.float32)   # rows earlier cameras filled stay as they are
    filled0 = np.zeros(npts, np.uint8)
    filled0[idx[::3]] = 1
    desc0[filled0 == 0] = 0.0
    count = np.array([k - (k > 2)], np.int64)
    bufs = dict(grid=Buf(IN, grid), image=Buf(IN, img, poison=(ZERO, FF)), u=Buf(IN, u), v=Buf(IN, v), idx=Buf(IN, idx),
                count=Buf(IN, count), desc=Buf(INOUT, desc0), filled=Buf(INOUT, filled0))
    name = f"gather rot={rot} C={Cc} k={k}"

    def call(B, Wk):
        _chk(lib.vfm_gather_bilinear_patchgrid(B["grid"].ptr(), gh, gw, Cc, H, W, rot, B["image"].ptr(), B["u"].ptr(), B["v"].ptr(),
                                               B["idx"].ptr(), B["count"].ptr(), k, B["desc"].ptr(), B["filled"].ptr(), _stream()), name)

    def ref(A):
        c = int(count[0])
        f = orc.gather_bilinear(grid, H, W, rot, u[:c].astype(np.int64), v[:c].astype(np.int64))
        black = (img == 0).all(-1)
        blk = black[u[:c], W - 1 - v[:c]] if rot == 1 else black[v[:c], u[:c]]
        f[blk] = 0.0
        desc, filled = desc0.copy(), filled0.copy()
        for j in range(c):
            if not filled[idx[j]]:
                desc[idx[j]] = f[j]
                filled[idx[j]] = 1
        np.testing.assert_array_equal(A["filled"], filled, err_msg=name)
        np.testing.assert_array_equal(A["desc"], desc, err_msg=name)
    check_case(Case(name, bufs, call, None, ref))


def _cameras(n_cam, W, H):
    K = np.array([[W / 2.0, 0, W / 2.0], [0, W / 2.0, H / 2.0], [0, 0, 1.0]])
    Ps = []
    for i in range(n_cam):
        yaw = np.deg2rad(60.0 * i)
        R = np.stack([[np.sin(yaw), -np.cos(yaw), 0.0], [0.0, 0.0, -1.0], [np.cos(yaw), np.sin(yaw), 0.0]])
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = -R @ np.array([0.1 * np.cos(yaw), 0.1 * np.sin(yaw), 0.3])
        Ps.append(K @ T[:3, :])
    return Ps


@pytest.mark.parametrize("ncam", [1, 3, 6])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 403])
def test_lift_multicam_stays_in_its_buffers(orc, ncam, n):
    from vfmreg import ops
    rng = np.random.default_rng(n * 10 + ncam)
    H, W, gh, gw, Cc = 84, 112, 16, 21, 384
    xyz = np.c_[rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-2.5, 6, n)]
    pcl = np.ascontiguousarray(np.insert(xyz, 3, 1, axis=1).T)
    Ps = _cameras(ncam, W, H)
    grids = [rng.standard_normal((gh, gw, Cc)).astype(np.float32) for _ in range(ncam)]
    imgs = [rng.integers(0, 255, (H, W, 3)).astype(np.uint8) for _ in range(ncam)]
    for im in imgs:
        im[rng.random((H, W)) < 0.1] = 0
    bufs = dict(pcl=Buf(IN, pcl), desc=Buf(OUT, shape=(n, Cc), dtype=np.float32), filled=Buf(INOUT, np.zeros(n, np.uint8)))
    for c in range(ncam):
        bufs[f"grid{c}"] = Buf(IN, grids[c])
        bufs[f"img{c}"] = Buf(IN, imgs[c], poison=(ZERO, FF))
    name = f"lift ncam={ncam} n={n}"

    def call(B, Wk):
        cams = [dict(mode=ops.PROJ_KITTI, mats=[Ps[c]], fc=None, subsample=1.0, win=None, H=H, W=W, proj_image=None,
                     grid=B[f"grid{c}"].t, Hup=H, Wup=W, rot_mode=0, raw_image=B[f"img{c}"].t) for c in range(ncam)]
        ops.LiftPlan(cams, Cc)(B["pcl"].t, B["desc"].t, B["filled"].t)

    def ref(A):
        cams = []
        for c in range(ncam):
            u, v, idx = orc.project(2, pcl, [Ps[c]], None, 1.0, None, None, H, W)
            cams.append(dict(grid=grids[c], Hup=H, Wup=W, rot_mode=0, black=(imgs[c] == 0).all(-1), u=u, v=v, idx=idx))
        desc = orc.create_descriptors(n, cams)
        seen = np.zeros(n, np.uint8)
        for cam in cams:
            seen[cam["idx"]] = 1
        np.testing.assert_array_equal(A["filled"], seen, err_msg=name)
        np.testing.assert_allclose(A["desc"], desc, rtol=0, atol=1e-6, err_msg=name)
    check_case(Case(name, bufs, call, None, ref))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4003])
def test_transform_xyz_stays_in_its_buffers(orc, n):
    lib = _lib().load()
    rng = np.random.default_rng(n)
    xyz = rng.uniform(-50, 50, (n, 3))
    T = np.eye(4)
    T[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    T[:3, 3] = [1.0, 2.0, -3.0]
    bufs = dict(xyz=Buf(IN, xyz), T=Buf(IN, T.reshape(-1)), out=Buf(OUT, shape=(n, 3), dtype=np.float64))

    def call(B, Wk):
        _chk(lib.vfm_transform_xyz_f64(B["xyz"].ptr(), n, B["T"].ptr(), B["out"].ptr(), _stream()), "transform")

    def ref(A):
        np.testing.assert_array_equal(A["out"], orc.transform_pcl(xyz, T))
    check_case(Case(f"transform n={n}", bufs, call, None, ref))


# ================================================================================================================ voxel / ICP
VOX_N = [1, 7, 513, 8000]


def _cloud(n, seed, stride=4):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-20, 20, (n, stride))
    if n > 4:
        pts[n // 2:n // 2 + n // 4, :3] = pts[:n // 4, :3] + 0.01   # many points per voxel
    return pts


@pytest.mark.parametrize("n", VOX_N)
@pytest.mark.parametrize("K", [1, 3])
def test_voxel_first_stays_in_its_buffers(orc, n, K):
    lib = _lib().load()

    def make(n_):
        pts = _cloud(n_, n_)
        pre = _prefix("count")
        bufs = dict(pts=Buf(IN, pts), keep=Buf(OUT, shape=n_, dtype=np.int64, view=pre), count=Buf(OUT, shape=1, dtype=np.int64))

        def call(B, W):
            _chk(lib.vfm_voxel_first(B["pts"].ptr(), n_, 4, 1.0, K, B["keep"].ptr(), B["count"].ptr(), W.ptr(), W.nbytes, _stream()), "vf")

        def ref(A):
            np.testing.assert_array_equal(A["keep"][:int(A["count"][0])], orc.voxel_first(pts, 1.0, K))
        return Case(f"voxel_first n={n_} K={K}", bufs, call, lib.vfm_voxel_first_workspace_bytes(n_), ref, lambda: make(2 * n_ + 3))
    check_case(make(n))


@pytest.mark.parametrize("n", VOX_N)
@pytest.mark.parametrize("reserve", [True, False])
def test_voxel_robin_stays_in_its_buffers(orc, n, reserve):
    lib = _lib().load()
    K, hm = (1, 19349663) if reserve else (3, 19349669)

    def make(n_):
        pts = _cloud(n_, n_ + 1)
        pre = _prefix("count")
        bufs = dict(pts=Buf(IN, pts), keep=Buf(OUT, shape=n_, dtype=np.int64, view=pre), count=Buf(OUT, shape=1, dtype=np.int64),
                    info=Buf(OUT, shape=4, dtype=np.int64, host=True))

        def call(B, W):
            _chk(lib.vfm_voxel_robin(B["pts"].ptr(), n_, 4, 1.0, K, hm, n_ if reserve else -1, B["keep"].ptr(), B["count"].ptr(),
                                     B["info"].ptr(), W.ptr(), W.nbytes, _stream()), "voxel_robin")

        def ref(A):
            r, info = orc.voxel_robin(pts, 1.0, K, reserve, hm, return_info=True)
            np.testing.assert_array_equal(A["keep"][:int(A["count"][0])], r)
            np.testing.assert_array_equal(A["info"][:2], info[:2])
        return Case(f"voxel_robin n={n_} reserve={reserve}", bufs, call, lib.vfm_voxel_robin_workspace_bytes(n_), ref,
                    lambda: make(2 * n_ + 3))
    check_case(make(n))


@pytest.mark.parametrize("n", VOX_N)
def test_voxel_robin_level_chained_stays_in_its_buffers(orc, n):
    """The second level of a chain: its points are pts[idx[:n_dev]] of the first level's survivors, moved by T on the device."""
    lib = _lib().load()

    def make(n_):
        pts = _cloud(n_, n_ + 2)
        idx = orc.voxel_robin(pts, 0.5)
        c = len(idx)
        n_max = n_
        idx_full = np.r_[idx, np.zeros(n_max - c, np.int64)] if c < n_max else idx
        T = np.eye(4)
        T[:3, :3] = np.linalg.qr(np.random.default_rng(n_).standard_normal((3, 3)))[0]
        T[:3, 3] = [0.25, -0.5, 1.0]
        pre = _prefix("count")
        bufs = dict(pts=Buf(IN, pts), idx=Buf(IN, idx_full), n_dev=Buf(IN, np.array([c], np.int64)), T=Buf(IN, T.reshape(-1)),
                    keep=Buf(OUT, shape=n_max, dtype=np.int64, view=pre), local=Buf(OUT, shape=n_max, dtype=np.int64, view=pre),
                    count=Buf(OUT, shape=1, dtype=np.int64),
                    info=Buf(OUT, shape=8, dtype=np.int64, view=lambda res, a: a[[0, 1, 2, 3, 5]]))

        def call(B, W):
            _chk(lib.vfm_voxel_robin_level(B["pts"].ptr(), 4, B["idx"].ptr(), n_max, B["n_dev"].ptr(), B["T"].ptr(), 1.0, 19349663,
                                           B["keep"].ptr(), B["local"].ptr(), B["count"].ptr(), B["info"].ptr(), W.ptr(), W.nbytes,
                                           _stream()), "voxel_robin_level")

        def ref(A):
            assert A["info"][5] == 1 and A["info"][1] != -1, A["info"]
            moved = orc.transform_pcl(pts[idx], T)
            r = orc.voxel_robin(moved, 1.0, 1, True, 19349663)
            k = int(A["count"][0])
            np.testing.assert_array_equal(A["local"][:k], r)
            np.testing.assert_array_equal(A["keep"][:k], idx[r])
        return Case(f"voxel_robin_level n={n_}", bufs, call, lib.vfm_voxel_robin_workspace_bytes(n_), ref, lambda: make(2 * n_ + 3))
    check_case(make(n))


@pytest.fixture(scope="module")
def icp_map(orc):
    rng = np.random.default_rng(17)
    mp = rng.uniform(-15, 15, (20000, 3))
    keys, start, pts = orc.voxel_grid_csr(mp, 1.0)
    f = 7
    mdesc = rng.standard_normal((len(pts), f))
    mdesc[::11] = 0.0
    return mp, keys, start, pts, mdesc, f


def _icp_src(mp, n, seed):
    rng = np.random.default_rng(seed)
    src = mp[rng.integers(0, len(mp), n)] + 0.2 * rng.standard_normal((n, 3))
    if n > 5:
        src[5] = [500.0, 500.0, 500.0]
    return src


@pytest.mark.parametrize("n", VOX_N)
def test_icp_kernels_stay_in_their_buffers(orc, icp_map, n):
    lib = _lib().load()
    o = orc
    mp, keys, start, pts, mdesc, f = icp_map
    nv, vs, md = len(keys), 1.0, 0.6
    src = _icp_src(mp, n, n)
    T = np.eye(4)
    T[:3, 3] = [0.05, -0.02, 0.01]
    Th = np.ascontiguousarray(T.reshape(-1))
    valid_view = lambda res, a: a[res["valid"].astype(bool)]   # noqa: E731  (tgt is defined where valid)
    grid = dict(keys=Buf(IN, keys), start=Buf(IN, start), pts=Buf(IN, pts))

    # vfm_icp_nearest
    def call(B, W):
        _chk(lib.vfm_icp_nearest(B["src"].ptr(), n, B["keys"].ptr(), B["start"].ptr(), B["pts"].ptr(), nv, vs, md, B["tgt"].ptr(),
                                 B["valid"].ptr(), _stream()), "icp_nearest")

    def ref(A):
        tgt_r, val_r = np.empty((n, 3)), np.empty(n, np.uint8)
        o.lib().orc_icp_nearest(o._p(src, o._f64p), C.c_int64(n), o._p(keys, o._i64p), o._p(start, o._i32p), o._p(pts, o._f64p),
                                C.c_int32(nv), C.c_double(vs), C.c_double(md), o._p(tgt_r, o._f64p), o._p(val_r, o._u8p))
        np.testing.assert_array_equal(A["valid"], val_r)
        np.testing.assert_array_equal(A["tgt"][val_r > 0], tgt_r[val_r > 0])
    check_case(Case(f"icp_nearest n={n}", dict(src=Buf(IN, src), **grid, tgt=Buf(OUT, shape=(n, 3), dtype=np.float64, view=valid_view),
                                                valid=Buf(OUT, shape=n, dtype=np.uint8)), call, None, ref))

    # vfm_icp_step_nearest: moved points + the search
    moved = o.transform_pcl(src, T)

    def call(B, W):
        _chk(lib.vfm_icp_step_nearest(B["src"].ptr(), n, Th.ctypes.data, B["src_out"].ptr(), B["keys"].ptr(), B["start"].ptr(),
                                      B["pts"].ptr(), nv, vs, md, B["tgt"].ptr(), B["valid"].ptr(), _stream()), "icp_step_nearest")

    def ref(A):
        np.testing.assert_array_equal(A["src_out"], moved)
        tgt_r, val_r = np.empty((n, 3)), np.empty(n, np.uint8)
        o.lib().orc_icp_nearest(o._p(moved, o._f64p), C.c_int64(n), o._p(keys, o._i64p), o._p(start, o._i32p), o._p(pts, o._f64p),
                                C.c_int32(nv), C.c_double(vs), C.c_double(md), o._p(tgt_r, o._f64p), o._p(val_r, o._u8p))
        np.testing.assert_array_equal(A["valid"], val_r)
        np.testing.assert_array_equal(A["tgt"][val_r > 0], tgt_r[val_r > 0])
    check_case(Case(f"icp_step_nearest n={n}", dict(src=Buf(IN, src), **grid, src_out=Buf(OUT, shape=(n, 3), dtype=np.float64),
                                                     tgt=Buf(OUT, shape=(n, 3), dtype=np.float64, view=valid_view),
                                                     valid=Buf(OUT, shape=n, dtype=np.uint8)), call, None, ref))

    # vfm_icp_desc_stats
    sdesc = np.random.default_rng(n + 1).standard_normal((n, f))
    sdesc[::5] = 0.0

    def stats(d):
        nr, hs = np.empty(len(d)), np.empty(len(d), np.uint8)
        o.lib().orc_icp_desc_stats(o._p(np.ascontiguousarray(d), o._f64p), C.c_int64(len(d)), C.c_int32(f), o._p(nr, o._f64p),
                                   o._p(hs, o._u8p))
        return nr, hs
    snorm, shas = stats(sdesc)
    mnorm, mhas = stats(mdesc)

    def call(B, W):
        _chk(lib.vfm_icp_desc_stats(B["desc"].ptr(), n, f, B["norm"].ptr(), B["has"].ptr(), _stream()), "icp_desc_stats")

    def ref(A):
        np.testing.assert_array_equal(A["norm"], snorm)
        np.testing.assert_array_equal(A["has"], shas)
    check_case(Case(f"icp_desc_stats n={n}", dict(desc=Buf(IN, sdesc), norm=Buf(OUT, shape=n, dtype=np.float64),
                                                   has=Buf(OUT, shape=n, dtype=np.uint8)), call, None, ref))

    # vfm_icp_step_nearest_desc
    def call(B, W):
        _chk(lib.vfm_icp_step_nearest_desc(B["src"].ptr(), n, Th.ctypes.data, B["src_out"].ptr(), B["sdesc"].ptr(), B["snorm"].ptr(),
                                           B["shas"].ptr(), f, B["keys"].ptr(), B["start"].ptr(), B["pts"].ptr(), B["mdesc"].ptr(),
                                           B["mnorm"].ptr(), B["mhas"].ptr(), nv, vs, md, B["tgt"].ptr(), B["valid"].ptr(), _stream()),
             "icp_step_nearest_desc")

    def ref(A):
        np.testing.assert_array_equal(A["src_out"], moved)
        tgt_r, val_r = np.empty((n, 3)), np.empty(n, np.uint8)
        o.lib().orc_icp_nearest_desc(o._p(moved, o._f64p), C.c_int64(n), o._p(sdesc, o._f64p), o._p(snorm, o._f64p), o._p(shas, o._u8p),
                                     C.c_int32(f), o._p(keys, o._i64p), o._p(start, o._i32p), o._p(pts, o._f64p), o._p(mdesc, o._f64p),
                                     o._p(mnorm, o._f64p), o._p(mhas, o._u8p), C.c_int32(nv), C.c_double(vs), C.c_double(md),
                                     o._p(tgt_r, o._f64p), o._p(val_r, o._u8p))
        np.testing.assert_array_equal(A["valid"], val_r)
        np.testing.assert_array_equal(A["tgt"][val_r > 0], tgt_r[val_r > 0])
    check_case(Case(f"icp_step_nearest_desc n={n}",
                    dict(src=Buf(IN, src), sdesc=Buf(IN, sdesc), snorm=Buf(IN, snorm), shas=Buf(IN, shas), **grid, mdesc=Buf(IN, mdesc),
                         mnorm=Buf(IN, mnorm), mhas=Buf(IN, mhas), src_out=Buf(OUT, shape=(n, 3), dtype=np.float64),
                         tgt=Buf(OUT, shape=(n, 3), dtype=np.float64, view=valid_view), valid=Buf(OUT, shape=n, dtype=np.uint8)),
                    call, None, ref))

    # vfm_icp_build_system
    rng = np.random.default_rng(n + 2)
    tgt = src + 0.05 * rng.standard_normal((n, 3))
    valid = (rng.random(n) < 0.8).astype(np.uint8)

    def call(B, W):
        _chk(lib.vfm_icp_build_system(B["src"].ptr(), B["tgt"].ptr(), B["valid"].ptr(), n, 0.3, B["out"].ptr(), _stream()), "icp_system")

    def ref(A):
        out_r = np.empty(43)
        o.lib().orc_icp_system(o._p(src, o._f64p), o._p(tgt, o._f64p), o._p(valid, o._u8p), C.c_int64(n), C.c_double(0.3),
                               o._p(out_r, o._f64p))
        np.testing.assert_array_equal(A["out"], out_r)
    check_case(Case(f"icp_build_system n={n}", dict(src=Buf(IN, src), tgt=Buf(IN, tgt), valid=Buf(IN, valid),
                                                     out=Buf(OUT, shape=43, dtype=np.float64)), call, None, ref))


# ================================================================================================================ FPFH
def _fpfh_cloud(n, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, (n, 3))
    if n > 8:
        pts[n // 2:n // 2 + n // 8] = pts[:n // 8]          # duplicates: equal distances
    return pts


@pytest.mark.parametrize("n", [1, 2, 65, 5000])
@pytest.mark.parametrize("max_nn", [30, 100, 1024])
def test_fpfh_search_chain_stays_in_its_buffers(n, max_nn):
    from tests import fpfh_oracle as fo
    lib = _lib().load()
    r = 0.2
    pts = _fpfh_cloud(n, n + max_nn)

    def grid_case(n_):
        p = _fpfh_cloud(n_, n_ + max_nn)

        def call(B, W):
            _chk(lib.vfm_fpfh_grid_build(B["pts"].ptr(), n_, r, B["keys"].ptr(), B["order"].ptr(), W.ptr(), W.nbytes, _stream()), "grid")

        def ref(A):
            keys, order = A["keys"], A["order"]
            assert np.array_equal(np.sort(order), np.arange(n_))
            assert (np.diff(keys) >= 0).all()
            same = np.diff(keys) == 0
            assert (np.diff(order)[same] > 0).all()
        return Case(f"fpfh_grid n={n_}", dict(pts=Buf(IN, p), keys=Buf(OUT, shape=n_, dtype=np.int64),
                                               order=Buf(OUT, shape=n_, dtype=np.int32)),
                    call, lib.vfm_fpfh_workspace_bytes(n_), ref, lambda: grid_case(2 * n_ + 3))
    A = check_case(grid_case(n))
    keys, order = A["keys"], A["order"]

    ri, rd, rc = fo.hybrid_search(pts, r, max_nn)
    by_count = lambda res, a: a[res["idx"] >= 0]   # noqa: E731  (d2 is defined up to each row's count)

    def call(B, W):
        _chk(lib.vfm_fpfh_search_hybrid(B["pts"].ptr(), n, B["keys"].ptr(), B["order"].ptr(), r, max_nn, B["idx"].ptr(), B["d2"].ptr(),
                                        B["cnt"].ptr(), None, _stream()), "search")

    def ref(A):
        np.testing.assert_array_equal(A["cnt"], rc)
        np.testing.assert_array_equal(A["idx"], ri)
        np.testing.assert_array_equal(A["d2"][ri >= 0], rd[ri >= 0])
    check_case(Case(f"fpfh_search n={n} max_nn={max_nn}",
                    dict(pts=Buf(IN, pts), keys=Buf(IN, keys), order=Buf(IN, order), idx=Buf(OUT, shape=(n, max_nn), dtype=np.int32),
                         d2=Buf(OUT, shape=(n, max_nn), dtype=np.float64, view=by_count), cnt=Buf(OUT, shape=n, dtype=np.int32)),
                    call, None, ref))

    if max_nn != 30:
        return
    # normals from the rows
    nv_ref = fo.estimate_normals(pts, ri, rc)

    def call(B, W):
        _chk(lib.vfm_fpfh_normals(B["pts"].ptr(), n, B["idx"].ptr(), B["cnt"].ptr(), max_nn, B["out"].ptr(), _stream()), "normals")

    def ref(A):
        assert np.abs(A["out"] - nv_ref).max() <= 1e-9
    check_case(Case(f"fpfh_normals n={n}", dict(pts=Buf(IN, pts), idx=Buf(IN, ri), cnt=Buf(IN, rc),
                                                 out=Buf(OUT, shape=(n, 3), dtype=np.float64)), call, None, ref))


@pytest.mark.parametrize("n", [1, 2, 65, 5000])
@pytest.mark.parametrize("with_normals", [True, False])
def test_fpfh_voxel_down_sample_stays_in_its_buffers(n, with_normals):
    from tests import fpfh_oracle as fo
    lib = _lib().load()
    vs = 0.1

    def make(n_):
        pts = _fpfh_cloud(n_, n_ + 3)
        nrm = np.random.default_rng(n_).standard_normal((n_, 3))
        pre = _prefix("count")
        bufs = dict(pts=Buf(IN, pts), out=Buf(OUT, shape=(n_, 3), dtype=np.float64, view=pre), count=Buf(OUT, shape=1, dtype=np.int32))
        if with_normals:
            bufs["nrm"] = Buf(IN, nrm)
            bufs["nout"] = Buf(OUT, shape=(n_, 3), dtype=np.float64, view=pre)

        def call(B, W):
            _chk(lib.vfm_fpfh_voxel_down_sample(B["pts"].ptr(), B["nrm"].ptr() if with_normals else None, n_, vs, B["out"].ptr(),
                                                B["nout"].ptr() if with_normals else None, B["count"].ptr(), W.ptr(), W.nbytes,
                                                _stream()), "down_sample")

        def ref(A):
            d, dn = fo.voxel_down_sample(pts, vs, nrm if with_normals else None)
            k = int(A["count"][0])
            assert k == len(d)
            np.testing.assert_array_equal(A["out"][:k], d)
            if with_normals:
                np.testing.assert_array_equal(A["nout"][:k], dn)
        return Case(f"fpfh_down_sample n={n_} normals={with_normals}", bufs, call, lib.vfm_fpfh_workspace_bytes(n_), ref,
                    lambda: make(2 * n_ + 3))
    check_case(make(n))


@pytest.mark.parametrize("n", [1, 2, 65, 5000])
def test_fpfh_features_stay_in_their_buffers(n):
    from tests import fpfh_oracle as fo
    lib = _lib().load()
    max_nn, r = 100, 0.25
    pts = _fpfh_cloud(n, n + 5)
    ri, rd, rc = fo.hybrid_search(pts, r, max_nn)
    nrm = fo.estimate_normals(pts, *fo.hybrid_search(pts, 0.2, 30)[::2])
    sp_ref, near = fo.spfh(pts, nrm, ri, rc)
    f_ref, fnear = fo.fpfh(sp_ref, ri, rd, rc, near)

    def close(got, refv, nr, what):
        bad = (np.abs(got - refv) > 1e-9 * np.maximum(np.abs(refv), 1.0)).any(1)
        assert not (bad & ~nr).any(), (what, np.flatnonzero(bad & ~nr)[:10])

    def call(B, W):
        _chk(lib.vfm_fpfh_spfh(B["pts"].ptr(), B["nrm"].ptr(), n, B["idx"].ptr(), B["cnt"].ptr(), max_nn, B["out"].ptr(), _stream()), "spfh")
    A = check_case(Case(f"fpfh_spfh n={n}", dict(pts=Buf(IN, pts), nrm=Buf(IN, nrm), idx=Buf(IN, ri), cnt=Buf(IN, rc),
                                                  out=Buf(OUT, shape=(n, 33), dtype=np.float64)), call, None,
                        lambda A: close(A["out"], sp_ref, near, "spfh")))
    sp = A["out"]

    def call(B, W):
        _chk(lib.vfm_fpfh_fpfh(B["sp"].ptr(), n, B["idx"].ptr(), B["d2"].ptr(), B["cnt"].ptr(), max_nn, B["out"].ptr(), _stream()), "fpfh")
    check_case(Case(f"fpfh_fpfh n={n}", dict(sp=Buf(IN, sp_ref), idx=Buf(IN, ri), d2=Buf(IN, np.where(ri >= 0, rd, 0.0)), cnt=Buf(IN, rc),
                                              out=Buf(OUT, shape=(n, 33), dtype=np.float64)), call, None,
                    lambda A: close(A["out"], f_ref, fnear, "fpfh")))
    assert sp.shape == (n, 33)


# ================================================================================================================ ViT
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("policy", ["default", "fused"])
def test_vit_forward_stays_in_its_buffers(B, policy):
    from tests.test_gpu_vit import _smooth_images
    from vfmreg import vit as V
    L = _lib()
    lib = L.load()
    H, W = 700, 820
    dim, depth, mlp = (128, 2, 256) if policy == "default" else (384, 1, 1536)
    cfg = {} if policy == "default" else dict(vit_fused_qkv=1, vit_fused_mlp=1)
    model = V.ViTS14(V.random_weights(seed=5, dim=dim, depth=depth, mlp=mlp), H, W)
    blob = model.blob.cpu().numpy()
    imgs = _smooth_images(np.random.default_rng(B), B, H, W)
    with _bound(cfg):
        expect = model.forward(torch.from_numpy(imgs).cuda()).cpu().numpy()
    ccfg = model.cfg
    shape = (B, 16, model.patch_w, dim)

    def make(b_):
        im = _smooth_images(np.random.default_rng(b_), b_, H, W)

        def call(Bf, Wk):
            _chk(lib.vfm_vit_forward(C.byref(ccfg), Bf["w"].ptr(), Bf["img"].ptr(), b_, H, W, Bf["out"].ptr(), Wk.ptr(), Wk.nbytes,
                                     _stream()), "vit_forward")
        return Case(f"vit {policy} B={b_}", dict(w=Buf(IN, blob, poison=(ZERO,)), img=Buf(IN, im, poison=(ZERO, FF)),
                                                  out=Buf(OUT, shape=(b_, 16, model.patch_w, dim), dtype=np.float32)),
                    call, lib.vfm_vit_workspace_bytes(C.byref(ccfg), b_), None, lambda: make(b_ + 2), cfg)

    case = make(B)
    case.ref = lambda A: np.testing.assert_array_equal(A["out"].reshape(shape), expect)
    check_case(case)


# ================================================================================================================ k-best search
# vfm_match_ip_topk / vfm_match_ip_topk_prepared (csrc/match_topk.hip).  The state where stale memory would bite: counters | rec_cnt |
# tau cleared by ONE memset whose length rests on the three arrays being contiguous; fb_list and rec never cleared and trusted only up
# to the counts; info written by a kernel of its own; both prepared images promised to be left as they were found.
TOPK_INFO = ("max_records", "fallback", "slices", "reserved")
EINVAL, EWORKSPACE = -1, -2


def _topk_rows(n, m, d, zero_rows=False):
    from tests import topk_oracle as to
    q, b = to.gaussian_rows(n, m, d, seed=n + m + d)
    if zero_rows:
        q[n // 2] = 0.0
        b[min(3, m - 1)] = 0.0
    return q, b


def _prepared_image(x, d):
    """vfm_match_prepare's image of the rows x, written into a guarded buffer of exactly vfm_match_prepared_bytes: its bytes"""
    lib = _lib().load()
    rows = x.shape[0]
    src = GuardedBuffer(x.shape, torch.float32, seed=11)
    src.set(torch.from_numpy(x))
    img = GuardedBuffer(lib.vfm_match_prepared_bytes(rows, d), torch.uint8, seed=12).fill_bytes(0)
    _chk(lib.vfm_match_prepare(src.ptr(), rows, d, img.ptr(), _stream()), "match_prepare")
    torch.cuda.synchronize()
    for g in (src, img):
        chk = g.intact()
        assert chk, f"vfm_match_prepare rows={rows} d={d}: {chk!r}"
    return img.body_bytes()


def topk_case(form, n, m, d, k, prec=FAST, rows=None, zero_rows=False, want_info=None, big=True):
    """form "topk": vfm_match_ip_topk; "prepared": vfm_match_ip_topk_prepared on images written beforehand (role IN: unchanged byte
    for byte).  The reference is tests/topk_oracle.py, bit for bit, and ``info`` as include/vfmreg.h documents it."""
    from tests import topk_cases as tc
    from tests import topk_oracle as to
    lib = _lib().load()
    q, b = rows if rows is not None else _topk_rows(n, m, d, zero_rows)
    name = f"{form} n={n} m={m} d={d} k={k} prec={prec}" + (" zero rows" if zero_rows else "")
    fast = prec == FAST and d in tc.FAST_WIDTHS and m >= 1
    # info[0], the largest record count, is compared with its documented range below and not between runs
    bufs = dict(q=Buf(IN, q), b=Buf(IN, b), idx=Buf(OUT, shape=(n, k), dtype=np.int64), sim=Buf(OUT, shape=(n, k), dtype=np.float32),
                info=Buf(OUT, shape=4, dtype=np.int32, view=lambda res, a: a[1:]))
    if form == "prepared":
        bufs["qp"] = Buf(IN, _prepared_image(q, d), poison=(ZERO,))
        bufs["bp"] = Buf(IN, _prepared_image(b, d), poison=(ZERO,))
        ws = lib.vfm_match_ip_topk_prepared_workspace_bytes(n, d, k)

        def call(B, W):
            _chk(lib.vfm_match_ip_topk_prepared(B["q"].ptr(), B["qp"].ptr(), n, B["b"].ptr(), B["bp"].ptr(), m, d, k, B["idx"].ptr(),
                                                B["sim"].ptr(), B["info"].ptr(), W.ptr(), W.nbytes, _stream()), name)
    else:
        ws = lib.vfm_match_ip_topk_workspace_bytes(n, m, d, k, prec)

        def call(B, W):
            _chk(lib.vfm_match_ip_topk(B["q"].ptr(), n, B["b"].ptr(), m, d, k, prec, B["idx"].ptr(), B["sim"].ptr(), B["info"].ptr(),
                                       W.ptr(), W.nbytes, _stream()), name)
    assert ws > 0, name

    def ref(A):
        info = dict(zip(TOPK_INFO, A["info"].tolist()))
        print(f"{name}: {info}")
        want_idx, want_sim = to.topk(q, b, k)
        np.testing.assert_array_equal(A["idx"], want_idx, err_msg=name)
        np.testing.assert_array_equal(A["sim"].view(np.uint32), want_sim.view(np.uint32), err_msg=name)
        if want_info is not None:
            assert tuple(A["info"].tolist()) == want_info, (name, info)
        elif fast:   # ordinary rows: the matrix-core pass answered every query from its records
            assert info["fallback"] == 0 and info["reserved"] == 0 and info["slices"] == tc.max_slices(n, m, d), (name, info)
            assert min(k, m) <= info["max_records"] <= min(m, tc.RECORD_CAP), (name, info)
        else:        # a call that ran the all-pairs kernel
            assert tuple(A["info"].tolist()) == (0, n, 0, 0), (name, info)

    make_big = None
    if big and fast:   # the larger call that leaves plausible counters, bounds, records and a fallback list behind
        make_big = lambda: topk_case(form, tc.STALE_N, tc.STALE_M, d, tc.STALE_K, rows=tc.stale_maker(d), big=False)   # noqa: E731
    return Case(name, bufs, call, ws, ref, make_big)


TOPK = [
    ("topk", dict(n=1, m=1, d=128, k=1)), ("topk", dict(n=33, m=129, d=256, k=5)), ("topk", dict(n=257, m=2049, d=384, k=8)),
    ("topk", dict(n=129, m=300, d=640, k=8)), ("topk", dict(n=33, m=2049, d=768, k=2)), ("topk", dict(n=257, m=5, d=256, k=8)),
    ("topk", dict(n=65, m=300, d=128, k=5, zero_rows=True)),
    ("topk", dict(n=33, m=129, d=33, k=2, prec=EXACT)), ("topk", dict(n=257, m=300, d=128, k=8, prec=EXACT)),
    ("topk", dict(n=1, m=5, d=1028, k=8, prec=EXACT)),
    ("topk", dict(n=33, m=300, d=512, k=5, want_info=(0, 33, 0, 0))),      # FAST at a width without a kernel runs EXACT
    ("topk", dict(n=5, m=0, d=128, k=3, want_info=(0, 0, 0, 0))),          # no map rows: all padding
    ("prepared", dict(n=1, m=129, d=128, k=1)), ("prepared", dict(n=257, m=2049, d=256, k=8)),
    ("prepared", dict(n=129, m=300, d=640, k=5)), ("prepared", dict(n=33, m=2049, d=768, k=8)),
]


@pytest.mark.parametrize("form,kw", TOPK, ids=[f"{f}-" + "-".join(f"{k}{v}" for k, v in kw.items()) for f, kw in TOPK])
def test_topk_stays_in_its_buffers(form, kw):
    A = check_case(topk_case(form, **kw), ws_ff=True)
    if kw["m"] == 0:
        assert (A["idx"] == -1).all() and (A["sim"] == np.finfo(np.float32).min).all()


def test_topk_refusals_launch_nothing():
    """Every refusal of the two entry points returns its documented code and leaves outputs, info, workspace and guards as they were;
    the size functions return 0 for arguments the calls refuse; an empty query set succeeds and writes nothing."""
    lib = _lib().load()
    n, m, d, k = 33, 129, 128, 5
    q, b = _topk_rows(n, m, d)
    need = lib.vfm_match_ip_topk_workspace_bytes(n, m, d, k, FAST)
    need_p = lib.vfm_match_ip_topk_prepared_workspace_bytes(n, d, k)
    assert need > need_p > 0
    G = dict(q=GuardedBuffer(q.shape, torch.float32, seed=1), b=GuardedBuffer(b.shape, torch.float32, seed=2),
             idx=GuardedBuffer((n, 8), torch.int64, seed=3), sim=GuardedBuffer((n, 8), torch.float32, seed=4),
             info=GuardedBuffer(4, torch.int32, seed=5), ws=GuardedBuffer(need, torch.uint8, seed=6),
             qp=GuardedBuffer(lib.vfm_match_prepared_bytes(n, d), torch.uint8, seed=7),
             bp=GuardedBuffer(lib.vfm_match_prepared_bytes(m, d), torch.uint8, seed=8))
    G["q"].set(torch.from_numpy(q))
    G["b"].set(torch.from_numpy(b))
    for name in ("idx", "sim", "info", "ws", "qp", "bp"):
        G[name].fill_bytes(0xA5)
    before = {name: g.body_bytes() for name, g in G.items()}

    def plain(k=k, d=d, n=n, idx=G["idx"].ptr(), sim=G["sim"].ptr(), ws=G["ws"].ptr(), ws_bytes=need, prec=FAST):
        return lib.vfm_match_ip_topk(G["q"].ptr(), n, G["b"].ptr(), m, d, k, prec, idx, sim, G["info"].ptr(), ws, ws_bytes, _stream())

    def prepared(k=k, d=d, n=n, m=m, idx=G["idx"].ptr(), sim=G["sim"].ptr(), ws=G["ws"].ptr(), ws_bytes=need_p, qp=G["qp"].ptr()):
        return lib.vfm_match_ip_topk_prepared(G["q"].ptr(), qp, n, G["b"].ptr(), G["bp"].ptr(), m, d, k, idx, sim, G["info"].ptr(), ws,
                                              ws_bytes, _stream())

    calls = [("k = 0", lambda: plain(k=0), EINVAL), ("k = 9", lambda: plain(k=9), EINVAL), ("null idx", lambda: plain(idx=None), EINVAL),
             ("null sim", lambda: plain(sim=None), EINVAL), ("d = 0", lambda: plain(d=0), EINVAL),
             ("unknown mode", lambda: plain(prec=7), EINVAL), ("one byte short", lambda: plain(ws_bytes=need - 1), EWORKSPACE),
             ("null workspace", lambda: plain(ws=None), EWORKSPACE),
             ("prepared k = 0", lambda: prepared(k=0), EINVAL), ("prepared k = 9", lambda: prepared(k=9), EINVAL),
             ("prepared null idx", lambda: prepared(idx=None), EINVAL), ("prepared null sim", lambda: prepared(sim=None), EINVAL),
             ("prepared d = 512", lambda: prepared(d=512), EINVAL), ("prepared m = 0", lambda: prepared(m=0), EINVAL),
             ("prepared null image", lambda: prepared(qp=None), EINVAL),
             ("prepared one byte short", lambda: prepared(ws_bytes=need_p - 1), EWORKSPACE),
             ("prepared null workspace", lambda: prepared(ws=None), EWORKSPACE),
             ("no queries", lambda: plain(n=0), 0), ("prepared no queries", lambda: prepared(n=0), 0)]
    for what, fn, code in calls:
        assert fn() == code, what
        torch.cuda.synchronize()
        for name, g in G.items():
            chk = g.intact()
            assert chk, f"{what}: {name}: {chk!r}"
            assert np.array_equal(g.body_bytes(), before[name]), f"{what}: {name} was written"
    # the size functions: 0 for what the calls refuse
    for args in ((n, m, d, 0, FAST), (n, m, d, 9, FAST), (n, m, 0, k, FAST), (n, m, d, k, 7), (-1, m, d, k, FAST), (n, -1, d, k, EXACT)):
        assert lib.vfm_match_ip_topk_workspace_bytes(*args) == 0, args
    for args in ((n, 512, k), (n, 33, k), (n, d, 0), (n, d, 9), (-1, d, k)):
        assert lib.vfm_match_ip_topk_prepared_workspace_bytes(*args) == 0, args
    # ... and after all of them the same buffers still serve a real call
    _chk(plain(), "match_ip_topk")
    torch.cuda.synchronize()
    from tests import topk_oracle as to
    want_idx, want_sim = to.topk(q, b, k)
    np.testing.assert_array_equal(G["idx"].numpy().reshape(-1)[:n * k].reshape(n, k), want_idx)
    np.testing.assert_array_equal(G["sim"].numpy().reshape(-1)[:n * k].reshape(n, k).view(np.uint32), want_sim.view(np.uint32))
    assert all(g.intact() for g in G.values())


# ================================================================================================================ the harness itself
def test_the_harness_sees_each_kind_of_violation():
    """Negative controls, with torch ops in place of a kernel: a write one element past an output, a write to an input, a result that
    depends on what the output held, one that reads past the end of an input, one that depends on a reused workspace -- each one must
    fail check_case, and the honest version of the same call must pass."""
    x = np.arange(10, dtype=np.float32)

    def make(fault):
        bufs = dict(x=Buf(IN, x), y=Buf(OUT, shape=10, dtype=np.float32))

        def call(B, W):
            xs, y = B["x"], B["y"]
            before = y.t[9].clone()
            y.t.copy_(xs.t * 2)
            if fault == "overrun":
                y.raw[y.guard + y.nbytes:y.guard + y.nbytes + 4] = 1
            elif fault == "input":
                xs.t[3] = 0.0
            elif fault == "stale_out":
                y.t[9] = y.t[9] + torch.nan_to_num(before, nan=1.0)
            elif fault == "overread":
                y.t[9] = xs.raw[xs.guard + xs.nbytes:xs.guard + xs.nbytes + 4].view(torch.float32)[0]
            elif fault == "stale_ws":
                y.t[0] = W.t[0].float()
                W.t[0] = 7
        return Case(f"control {fault}", bufs, call, 16, lambda A: np.testing.assert_array_equal(A["y"], 2 * x), lambda: make(fault))
    check_case(make(None))
    for fault in ("overrun", "input", "stale_out", "overread", "stale_ws"):
        with pytest.raises((AssertionError, pytest.fail.Exception)):
            check_case(make(fault))
