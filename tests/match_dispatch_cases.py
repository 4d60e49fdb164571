"""The dispatch tree of the matcher's coarse pass as a table of cases, and one adversarial data set for all of them.

Which coarse kernel a search launches is decided at call time (csrc/match_internal.h: resolve_search, then resolve_coarse; csrc/match_api.hip:
use_i8, use_sparse) from the width, the record kind, gated or
not, size thresholds and the thread's vfm_config.  Every case below names the kernel resolve_coarse's rules give for it, with the rule
beside it; tests/test_gpu_coarse_dispatch.py runs each case, reads back which kernel ran (vfm_debug_last_coarse_kernel) and compares
the answers with the fp64 oracle; tests/test_coarse_dispatch_table.py checks that the table names every launcher instantiation in the
library.  No GPU and no torch in this module.

Sizes: 2113 queries = 67 query tiles -- above the 2048-query threshold of the 64-resident-query kernels, and neither a multiple of
16 (tiles per workgroup of those kernels) nor of 24 (three tiles per wave): the last workgroup has absent tiles; 300 and 2048 below
the threshold; 4100 map rows = 33 chunks with rows, 4 valid rows in the last one, and one chunk of padding (operands are padded to 256 rows: nchunks =
34) -- enough for four slices of at least 8 chunks (choose_slices keeps 8 chunks per slice; the half-width fp6 kernel takes
nchunks / 8 = 4 slices), so `t8`'s nslices <= nchunks / 2 holds; 600 queries
for the sparse fp16 records (use_sparse: n > 512), with 32 900 map rows = 258 chunks for the seed units (nchunks >= 256)."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

# record kinds and preparation flags of include/vfmreg.h
BEST, TOP2, HALF, HALF_FUSED, MX6, MX6_TOP2, MX6_HALF, MX6_HALF_FUSED, MX6_FUSED = 0, 1, 3, 4, 5, 6, 7, 8, 10
PREPARE_MX6 = 8
MX6_KINDS = (MX6, MX6_TOP2, MX6_HALF, MX6_HALF_FUSED, MX6_FUSED)
GATE = float(np.float32(0.8))

N_LO, N_EDGE, N_HI, N_SPARSE = 300, 2048, 2113, 600
M, M_SEED, M_L2 = 4100, 32900, 1300


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def make(d: int, n: int, m: int, seed: int):
    """fp32 queries q [n][d] and map b [m][d] that hold, all at once:
      - planted matches (cosine ~0.97 > 0.9) for the even queries; the odd ones are unrelated rows (cosine < 0.7 to everything);
      - an exact duplicate of a map row in a different 128-row chunk, and one in the last chunk (the partly padded one when
        m % 128 != 0), each with queries aimed at it: the lower index must win;
      - a cluster of 20 near-duplicates (jitter 1e-4), one per chunk, and 30 queries aimed at it: many candidates inside every window;
      - a zero map row, a zero query row, and a query that is a map row times 2.0;
      - a query whose score is negative against every map row but the zero one (which it therefore matches with similarity exactly
        0.0 -- a zero map row and "all scores negative" cannot both hold; what is kept is that nothing positive exists for it);
      - un-normalised rows: scales 3.7 and 0.21 on a stride of queries and map rows.
    Every row shares a component `mu` (0.6 per column against unit noise) so that the negative query exists; it lifts the background
    cosine to ~0.26, far below the gate."""
    assert n >= 200 and m >= 1200 and d >= 100
    rng = np.random.default_rng(seed)
    mu = 0.6 * rng.standard_normal(d)
    b = mu + rng.standard_normal((m, d))
    q = mu + rng.standard_normal((n, d))
    nchunks = (m + 127) // 128
    last = 128 * (nchunks - 1)
    # duplicates: row 200 (chunk 1) again as row 700 (chunk 5); row 330 (chunk 2) again as the map's last row but one
    b[700] = b[200]
    b[m - 2] = b[330]
    assert m - 2 >= last and last > 700
    # near-duplicates, one per chunk (at row 17 of chunks 0, 1, ...; as many chunks as the map has, 20 at most)
    centre = mu + rng.standard_normal(d)
    for c in range(min(20, nchunks - 1)):
        b[128 * c + 17] = centre + 1e-4 * rng.standard_normal(d)
    # the planted half (on the map as it now is; never on the row that becomes the zero row)
    pick = rng.integers(0, m, n)
    pick[pick == 1000] = 1001
    q[::2] = b[pick[::2]] + 0.25 * rng.standard_normal((len(q[::2]), d))
    q[40] = b[700] + 0.1 * rng.standard_normal(d)
    q[42] = b[700]
    q[44] = b[m - 2] + 0.1 * rng.standard_normal(d)
    q[46] = b[330]
    for i in range(30):
        q[60 + 2 * i + 1] = centre + 0.05 * rng.standard_normal(d)      # (odd queries: the planted half stays as it is)
    # zero rows, a scaled copy, the negative query
    b[1000] = 0.0
    q[5] = 0.0
    q[7] = 2.0 * b[450]
    q[9] = -mu
    # un-normalised rows
    q[3::50] *= 3.7
    q[11::50] *= 0.21
    b[5::40] *= 0.21
    b[9::40] *= 3.7
    q, b = q.astype(np.float32), b.astype(np.float32)
    scores = q[9].astype(np.float64) @ b.astype(np.float64).T
    assert (np.delete(scores, 1000) < 0).all(), "the negative query has a non-negative score"
    return q, b


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def data_ip(d: int, n: int, m: int):
    """(q, b, reference idx, reference sim) of an inner-product case: the fp64 decision over all pairs on the oracle's normalised rows,
    ties to the lowest index.  Computed once per shape, shared read-only."""
    from oracle import oracle as orc
    q, b = make(d, n, m, seed=d + n + m)
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    ridx, rsim = orc.match_ip_top1_bruteforce(qn, bn)
    return _frozen(q, b, ridx, rsim)


@functools.lru_cache(maxsize=None)
def data_ip_large(d: int, n: int, m: int):
    """data_ip where all pairs in fp64 would take too long: the oracle's accelerated form of the same decision (an fp32 product proposes
    every row within a proven window of the row maximum, fp64 decides among them)."""
    from oracle import oracle as orc
    q, b = make(d, n, m, seed=d + n + m)
    qn, _ = orc.l2norm_rows(q)
    bn, _ = orc.l2norm_rows(b)
    ridx, rsim = orc.match_ip_top1(qn, bn)
    return _frozen(q, b, ridx, rsim)


@functools.lru_cache(maxsize=None)
def data_l2(d: int, n: int, m: int):
    """(a, b, nn_ab, dist_ab, nn_ba) of a Euclidean case: the oracle's exact 1-NN in both directions."""
    from oracle import oracle as orc
    a, b = make(d, n, m, seed=d + n + m)
    i_ref, dist_ref = orc.nn_l2(a, b)
    j_ref, _ = orc.nn_l2(b, a)
    return _frozen(a, b, i_ref, dist_ref, j_ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    entry: str          # "ip": vfm_match_prepare + _search_coarse + _search_finish (ungated); "gated": vfm_match_prepare2_gated_p +
                        # _search_coarse_gated_g + _search_finish_gated_r; "l2": vfm_match_mutual_l2, both directions
    d: int
    n: int
    m: int
    records: int        # record kind of the gated entry (ignored by the others)
    cfg: tuple          # ((vfm_config key, value), ...) bound to the thread for the whole search, preparation included
    kernel: str         # vfm_debug_last_coarse_kernel after the search

    @property
    def id(self) -> str:
        cfg = "".join(f"-{k}={v}" for k, v in self.cfg)
        return f"{self.entry}-d{self.d}-n{self.n}-m{self.m}-r{self.records}{cfg}"

    @property
    def gated(self) -> bool:
        return self.entry == "gated"


def _pipe(ks, kind):
    return f"pipe<{ks},{kind}>"


def _v(ks, qsets):
    return f"v<{ks},qsets={qsets}>"


def _r(ks, bias):
    return f"r<{ks},qsets=1,nbuf=3,bias={bias}>"


def _i8(ks, t, top2, low):
    return f"i8<{ks},T={t},top2={top2},low={low}>"


def _i8q2(ks, top2, low, fused):
    return f"i8q2<{ks},top2={top2},low={low},fused={fused}>"


def _mx6(ks, kind, low, img, ring=4, t=4, ns=2):
    return f"mx6q2<{ks},{kind},low={low},img={img},ring={ring},T={t},NS={ns}>"


def _variant(v):
    return (("coarse_variant", v),)


CASES = []


def _add(entry, d, n, m, records, cfg, kernel):
    CASES.append(Case(entry, d, n, m, records, tuple(cfg), kernel))


# ---- the fp16 pass (launch_coarse_f16): every ungated search below 8192 queries x 1e9 pairs (use_i8), d = 128 ... 768
for d in (128, 256, 384):
    ks = d // 16
    # n <= 512: use_sparse is false -> a.rec == nullptr -> launch_coarse_pipe<KSTEPS, false>
    _add("ip", d, N_LO, M, BEST, (), _pipe(ks, "dense"))
    # n > 512: sparse records; 34 chunks < 256: no seed units
    _add("ip", d, N_SPARSE, M, BEST, (), _pipe(ks, "sparse"))
    # nchunks = 258 >= 256 and nqb = 3 <= 256: seed units at the head of the grid
    _add("ip", d, N_SPARSE, M_SEED, BEST, (), _pipe(ks, "sparse") + "+seed")
    # coarse_variant 1 / 2: coarse_qsets 1 / 2 -> launch_coarse_v<KSTEPS, 1 | 2> (use_sparse false: dense records)
    _add("ip", d, N_SPARSE, M, BEST, _variant(1), _v(ks, 1))
    _add("ip", d, N_SPARSE, M, BEST, _variant(2), _v(ks, 2))
# coarse_variant 7: seed_units = 0 -> the unseeded sparse kernel at the size that is seeded by default
_add("ip", 384, N_SPARSE, M_SEED, BEST, _variant(7), _pipe(24, "sparse"))
# coarse_variant 4: use_sparse false at every size -> the pipelined kernel with dense records
_add("ip", 384, N_SPARSE, M, BEST, _variant(4), _pipe(24, "dense"))
# coarse_variant 5: use_i8 false in the gated family too -> the fp16 pass, sparse records (use_sparse accepts 5)
_add("gated", 384, N_SPARSE, M, BEST, _variant(5), _pipe(24, "sparse"))
# d = 512: KSTEPS = 32 > 24 -> launch_coarse_v<32, 1>
_add("ip", 512, N_LO, M, BEST, (), _v(32, 1))
# d = 640 / 768: the 4-wave kernel; no row bias in an inner-product search
_add("ip", 640, N_LO, M, BEST, (), _r(40, 0))
_add("ip", 768, N_LO, M, BEST, (), _r(48, 0))
# the Euclidean entry: records are always dense; K = d + 2 padded to 128 for d <= 510 (l2_padded_k), the reverse direction (b -> a, fp16
# at every width) launches last.  d = 126 / 254 / 382 -> K = 128 / 256 / 384: launch_coarse_pipe<., false>; d = 384 -> K = 512:
# launch_coarse_v<32, 1>; d = 640 / 768: K = d with the row bias (launch_coarse_r<., 1, 3, true>)
_add("l2", 126, N_LO, M_L2, BEST, (), _pipe(8, "dense"))
_add("l2", 254, N_LO, M_L2, BEST, (), _pipe(16, "dense"))
_add("l2", 382, N_LO, M_L2, BEST, (), _pipe(24, "dense"))
_add("l2", 384, N_LO, M_L2, BEST, (), _v(32, 1))
_add("l2", 640, N_LO, M_L2, BEST, (), _r(40, 1))
_add("l2", 768, N_LO, M_L2, BEST, (), _r(48, 1))

# ---- the int8 pass (launch_coarse_int8): the gated family, d = 256 ... 768; KSTEPS = d / 32 (half-width kinds: d / 64)
# best-score and top-2 records, d <= 384: n <= 2048 -> the one-set kernel, four tiles per step; n > 2048 -> 64 resident queries
_add("gated", 256, N_EDGE, M, BEST, (), _i8(8, 4, 0, 1))
_add("gated", 384, N_EDGE, M, BEST, (), _i8(12, 4, 0, 1))
_add("gated", 256, N_LO, M, TOP2, (), _i8(8, 4, 1, 1))
_add("gated", 384, N_EDGE, M, TOP2, (), _i8(12, 4, 1, 1))
_add("gated", 256, N_HI, M, BEST, (), _i8q2(8, 0, 1, 0))
_add("gated", 384, N_HI, M, BEST, (), _i8q2(12, 0, 1, 0))
_add("gated", 256, N_HI, M, TOP2, (), _i8q2(8, 1, 1, 0))
_add("gated", 384, N_HI, M, TOP2, (), _i8q2(12, 1, 1, 0))
# d >= 512: the one-set kernel with two tiles per step at every query count
_add("gated", 512, N_LO, M, BEST, (), _i8(16, 2, 0, 1))
_add("gated", 640, N_LO, M, BEST, (), _i8(20, 2, 0, 1))
_add("gated", 768, N_LO, M, BEST, (), _i8(24, 2, 0, 1))
_add("gated", 768, N_HI, M, BEST, (), _i8(24, 2, 0, 1))
_add("gated", 512, N_HI, M, TOP2, (), _i8(16, 2, 1, 1))
_add("gated", 640, N_HI, M, TOP2, (), _i8(20, 2, 1, 1))
_add("gated", 768, N_HI, M, TOP2, (), _i8(24, 2, 1, 1))
# coarse_variant 10: the one-set kernel with TWO tiles per step at d <= 384, every size; 12: the default one-set kernels at every size
_add("gated", 256, N_HI, M, BEST, _variant(10), _i8(8, 2, 0, 1))
_add("gated", 384, N_HI, M, BEST, _variant(10), _i8(12, 2, 0, 1))
_add("gated", 384, N_HI, M, BEST, _variant(12), _i8(12, 4, 0, 1))
_add("gated", 384, N_HI, M, HALF, _variant(12), _i8(6, 4, 0, 0))
# the half-width pass (VFM_RECORDS_HALF): n > 2048 -> 64 resident queries at EVERY width; else the one-set kernel, four tiles per step
for d, n_small in ((256, N_LO), (384, N_EDGE), (512, N_LO), (640, N_EDGE), (768, N_LO)):
    _add("gated", d, N_HI, M, HALF, (), _i8q2(d // 64, 0, 0, 0))
    _add("gated", d, n_small, M, HALF, (), _i8(d // 64, 4, 0, 0))
# ... with the selection fused into the kernel (resolve_search: d = 256 / 384, n > 2048, n >= 4 chunks)
_add("gated", 256, N_HI, M, HALF_FUSED, (), _i8q2(4, 0, 0, 1))
_add("gated", 384, N_HI, M, HALF_FUSED, (), _i8q2(6, 0, 0, 1))

# ---- the fp6 pass (launch_coarse_mx6): operands prepared with VFM_PREPARE_MX6, more than 2048 queries; KS6 = d / 64 (half: d / 128)
for d in (256, 384):
    _add("gated", d, N_HI, M, MX6, (), _mx6(d // 64, "BEST", 1, d // 64))
    _add("gated", d, N_HI, M, MX6_TOP2, (), _mx6(d // 64, "TOP2", 1, d // 64))
    # n = 2113 >= 4 x 33 chunks with rows: the fused full-width form stays (resolve_search)
    _add("gated", d, N_HI, M, MX6_FUSED, (), _mx6(d // 64, "FUSE", 0, d // 64))
for d in (256, 384, 512, 768):
    _add("gated", d, N_HI, M, MX6_HALF, (), _mx6(d // 128, "BEST", 0, d // 64))
# the fused half-width pass: d = 384 takes three query tiles per wave by default (mx6_ns3 && mx6_t4)
_add("gated", 256, N_HI, M, MX6_HALF_FUSED, (), _mx6(2, "FUSE", 0, 4))
_add("gated", 384, N_HI, M, MX6_HALF_FUSED, (), _mx6(3, "FUSE", 0, 6, ns=3))
_add("gated", 512, N_HI, M, MX6_HALF_FUSED, (), _mx6(4, "FUSE", 0, 8))
_add("gated", 768, N_HI, M, MX6_HALF_FUSED, (), _mx6(6, "FUSE", 0, 12))
# mx6_tune bit 0 (s_setprio: same instantiation), bit 1 (the ring of five steps, three-tile shape only)
_add("gated", 384, N_HI, M, MX6_HALF_FUSED, (("mx6_tune", 1),), _mx6(3, "FUSE", 0, 6, ns=3))
_add("gated", 384, N_HI, M, MX6_HALF_FUSED, (("mx6_tune", 2),), _mx6(3, "FUSE", 0, 6, ring=5, ns=3))
# coarse_variant 32: mx6_ns3 = 0 -> two query tiles per wave at d = 384
_add("gated", 384, N_HI, M, MX6_HALF_FUSED, _variant(32), _mx6(3, "FUSE", 0, 6))
# coarse_variant 31: mx6_t4 = 0 -> two chunks per barrier (T = 8, ring of 3) where nslices = 4 <= nchunks / 2 = 17; 30 = the default
_add("gated", 256, N_HI, M, MX6_HALF_FUSED, _variant(31), _mx6(2, "FUSE", 0, 4, ring=3, t=8))
_add("gated", 384, N_HI, M, MX6_HALF_FUSED, _variant(31), _mx6(3, "FUSE", 0, 6, ring=3, t=8))
_add("gated", 256, N_HI, M, MX6_HALF_FUSED, _variant(30), _mx6(2, "FUSE", 0, 4))

assert len({c.id for c in CASES}) == len(CASES)

# The fused kinds where the two chunk counts disagree: a fused kind is kept from n >= 4 x chunks_with_rows(m) on, the finish stage
# used to choose the chunk-major rescan from n >= 4 x chunks_padded(m) (the map padded to 256 rows) on.  65 600 rows are 513 chunks with
# rows and 514 padded ones; 2053 queries lie between 4 x 513 and 4 x 514.  (Until this table existed the finish stage then left the
# survivors the coarse kernel had binned unread, and every match came back as "below the gate".)
M_ODD, N_BETWEEN = 65600, 2053
PADDING_CASES = [Case("gated", 256, N_BETWEEN, M_ODD, HALF_FUSED, (), _i8q2(4, 0, 0, 1)),
                 Case("gated", 256, N_BETWEEN, M_ODD, MX6_HALF_FUSED, (), _mx6(2, "FUSE", 0, 4)),
                 Case("gated", 256, N_BETWEEN, M_ODD, MX6_FUSED, (), _mx6(4, "FUSE", 0, 4))]
assert 4 * ((M_ODD + 127) // 128) <= N_BETWEEN < 4 * ((M_ODD + 255) // 256 * 2)

# launcher instantiations that no size and no config reaches: name -> reason
UNREACHABLE = {}


# the cases of test_finish_and_launch_variants_change_no_answer: (d, n, m, record kind), and the configs they run under
VARIANT_WORKLOADS = [(384, N_HI, M, BEST), (384, N_HI, M, HALF_FUSED), (768, 1300, M, BEST), (768, 1300, M, HALF), (384, N_HI, M, MX6_HALF_FUSED)]
VARIANT_CONFIGS = ([_variant(v) for v in (20, 21, 50, 51, 60, 61)] + [(("coarse_slices", s),) for s in (1, 2, 5, 1000)] +
                   [(("mx6_tune", t),) for t in (1, 2, 3)])


def mx6_fused_slices_refused(records, m, cfg):
    """launch_coarse_mx6 sizes nothing: the fused fp6 kinds leave one survivor slot per workgroup in the record buffer, which
    carve_search sized for max(min(nchunks / 8, 64), ceil(nchunks / 255)) slices.  A forced slice count (clamped to nchunks) above
    that is refused with VFM_EINVAL before anything is launched."""
    forced = dict(cfg).get("coarse_slices", 0)
    if records not in (MX6_HALF_FUSED, MX6_FUSED) or forced <= 0:
        return False
    nchunks = (m + 255) // 256 * 256 // 128
    cap = max(max(1, min(nchunks // 8, 64)), (nchunks + 254) // 255)
    return min(forced, nchunks) > cap
