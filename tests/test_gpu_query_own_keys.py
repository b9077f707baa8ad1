"""Every forest QUERY against the reference descent of its OWN keys (tests/descent_ref.py, pinned to
the oracle by tests/test_descent_ref_host.py).

rpt_knn_* / rpt_candidates compute Pq = project_columns(queries, f->R, T * L, f->mode) and then walk
on Pq, thr, mglo, mghi and the topology alone; rpt_project_host calls the same function with the same
arguments, so `rp.project(query_dataset, f.R.reshape(T * L, d), mode=f.mode)` downloads the very keys
the query path descends on, and given them the candidate list is fixed.  So whatever computed the
keys (f64 MFMA, f32 rows, bf16 rows in every projection option, CSR rows in exact and tolerance
mode) the query is held to an exact reference: for EVERY query and EVERY tree, offsets and ids of
`candidatesBatch`, the candidate total and the answer of every kNN path, and the buckets of
`knnHBatch`.  No share of the queries is left out and nothing is statistical; the only numeric
tolerances are the projection's own stated bounds on the keys (a) and twice them where build keys
meet query keys (e).

The options `proj_bf16_terms`, `proj_bf16_f32` and `proj_csr_nodense` are read at CALL time and are
not stored in the forest: a source's options stay switched on for its queries and for `rp.project`,
as they were for its build (Source.on()).

What this does not cover: the accuracy of the keys beyond those bounds, and equality of the keys a
row gets at build time and as a query (different kernels may compute them: (e) bounds and prints)."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descent_ref as dr  # noqa: E402
import knn_f32_ref as f32ref  # noqa: E402
import knn_l2_cut_ref as l2ref  # noqa: E402
import split_ref  # noqa: E402
from test_gpu_forest_own_keys import SOURCES as BUILD_SOURCES  # noqa: E402

pytestmark = pytest.mark.gpu

SOURCES = {s: BUILD_SOURCES[s] for s in ("f64_mfma", "f64_exact", "f32", "bf16", "bf16_terms3", "bf16_f32", "csr_f64",
                                         "csr_f32", "csr_mfma", "csr_mfma_nodense")}
NQS = (1, 5, 17, 64, 130)       # less than one 16-row MFMA tile, ..., more than two waves of queries
K_FR, K_WR = 512, 128           # csrc/knn_plan.h: leaf ranges per query of the workgroup / one-wave kernels
PATHS = {
    "default": {}, "wave": {"knn_wave": 1}, "workgroup": {"knn_wave": 0}, "general": {"knn_general": 1},
    "no_pre8": {"knn_no_pre8": 1}, "no_pre16": {"knn_no_pre16": 1}, "shard_old": {"knn_wave": 1, "knn_shard_old": 1},
    "l2_exact": {"knn_l2_exact": 1},                     # f64 rows only
}


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


@contextlib.contextmanager
def options(ctx, **kw):
    old = {k: ctx.set_option(k, v) for k, v in kw.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def last_candidates(ctx):
    from rptree_amd import _lib
    v = C.c_int64(-1)
    _lib.check(_lib.lib().rpt_knn_last_candidates(ctx._h, C.byref(v)))
    return int(v.value)


# --------------------------------------------------------------------------- rows, queries, keys
def to_csr(X):
    nz = X != 0                                          # (a NaN is stored)
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    return rowptr, np.nonzero(nz)[1].astype(np.int32), X[nz]


def rounded(elem, A):
    """A as the element type holds it, widened exactly to f64"""
    A = np.asarray(A, dtype=np.float64)
    if elem in ("f32", "csr32"):
        return A.astype(np.float32).astype(np.float64)
    if elem == "bf16":
        return f32ref.from_bf16(f32ref.to_bf16(A.astype(np.float32))).astype(np.float64)
    return A


def dataset(rp, ctx, elem, A):
    """A (already `rounded`) on the device in the source's layout"""
    if elem == "bf16":
        return rp.Dataset.dense(ctx, rp.to_bf16(A.astype(np.float32)), dtype=rp.RPT_BF16)
    if elem.startswith("csr"):
        rowptr, col, val = to_csr(A)
        return rp.Dataset.csr(ctx, rowptr, col, val.astype(np.float32 if elem == "csr32" else np.float64), A.shape[1])
    return rp.Dataset.dense(ctx, A.astype(np.float32) if elem == "f32" else A)


def inner_exact(X, r):
    """the exact-order kernels (csrc/project.hip, proj_exact): acc = x_k * r_k + acc from the last index
    to the first over ALL k, separate multiply and add, in the rows' type.  On finite rows this is
    innerSD / innerSS over the hyperplane's nonzeros (a zero adds an exact +-0 to an accumulator that
    is never -0); a NaN or inf coordinate also meets the hyperplane's dense-ified zeros."""
    acc = np.zeros(X.shape[0], dtype=X.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(X.shape[1] - 1, -1, -1):
            acc = X[:, k] * X.dtype.type(r[k]) + acc
    return acc


def tol_of(src, d):
    """the project's stated bounds on a tolerance-mode key, relative to |x||r| (test_project_mfma_*)"""
    return {"f64_mfma": 1e-13, "f32": 1e-5, "bf16": 8e-6 if d % 8 == 0 else 1e-5,
            "bf16_terms3": 2e-6 if d % 8 == 0 else 1e-5, "bf16_f32": 1e-5, "csr_mfma": 1e-5,
            "csr_mfma_nodense": 1e-5}[src]


class Batch:
    def __init__(self, kind, Q, qd):
        self.kind, self.Q, self.qd, self.nq = kind, Q, qd, len(Q)
        self.finite = np.isfinite(Q).all(axis=1)
        self.Pq = self.ranges = None


class Source:
    """rows of one source on the device, a forest over them built with the source's options, and query
    batches with their downloaded keys and reference ranges (computed once, never changed)"""

    def __init__(self, rp, ctx, src, kind, n, d, T, min_leaf, chunk=None, seed=0):
        self.rp, self.ctx, self.src, self.kind, self.n, self.d, self.T, self.min_leaf = rp, ctx, src, kind, n, d, T, min_leaf
        self.elem, mode, self.opts = SOURCES[src]
        self.csr = self.elem.startswith("csr")
        self.L = L = dr.depth(n, max(min_leaf, 1))
        self.rng = rng = np.random.default_rng([seed, n, d, T, len(src)])
        if kind == "lattice":
            X, R = dr.lattice_rows(rng, n, d), dr.lattice_planes(rng, T, L, d)
        elif kind == "axes":
            X, R = dr.axes_rows(rng, n, d), dr.axes_planes(rng, T, L, d)
        else:
            X = rng.standard_normal((n, d))
            R = rng.standard_normal((T, L, d)) * (rng.random((T, L, d)) < 0.6)
        if self.csr:
            X = X * (rng.random((n, d)) < 0.2)
        self.X = rounded(self.elem, X)
        self.R = R
        self.ds = dataset(rp, ctx, self.elem, self.X)
        with self.on():
            if chunk:
                self.f = rp.forest(0, L, min_leaf, T, chunk, 0, d, self.ds, ctx=ctx, hyperplanes=R,
                                   mode=getattr(rp, "RPT_PROJ_" + mode))
            else:
                self.f = rp._build(ctx, self.ds, R, L, min_leaf, getattr(rp, "RPT_PROJ_" + mode))
        self.streamed = bool(chunk)
        self.exact = self.f.mode == rp.RPT_PROJ_EXACT or (self.f.mode == rp.RPT_PROJ_AUTO and self.elem in ("f64", "csr64"))
        # the hyperplanes as the projection kernels hold them
        self.Rq = R.astype(np.float32).astype(np.float64) if self.elem in ("f32", "bf16", "csr32") else R
        self.batches = {}

    def on(self, **extra):
        return options(self.ctx, **dict(self.opts, **extra))

    def name(self):
        return "%s %s n=%d d=%d T=%d min_leaf=%d" % (self.src, self.kind, self.n, self.d, self.T, self.min_leaf)

    def project(self, qd):
        with self.on():
            P = self.rp.project(qd, self.R.reshape(self.T * self.L, self.d), mode=self.f.mode, ctx=self.ctx)
        return P.reshape(self.T, self.L, qd.n)

    def batch(self, kind, nq):
        """the batch, its keys (downloaded twice: the same bits) and the reference ranges of every query"""
        key = (kind, nq)
        if key not in self.batches:
            if kind.startswith("fan"):                   # ("axes" rows: about 2^m leaves per tree)
                Q = rounded(self.elem, dr.fan_queries(self.rng, self.X, nq, int(kind[3:])))
            else:
                Q = rounded(self.elem, dr.make_queries(kind, self.rng, self.X, nq))
            b = Batch(kind, Q, dataset(self.rp, self.ctx, self.elem, Q))
            b.Pq = self.project(b.qd)
            again = self.project(b.qd)
            assert b.Pq.dtype == (np.float64 if self.elem in ("f64", "csr64") else np.float32)
            assert b.Pq.tobytes() == again.tobytes(), "%s: the keys of %s x %d change between two calls" % (self.name(), kind, nq)
            f = self.f
            b.trace = dr.Trace()
            if self.streamed:
                b.ranges = [dr.candidates_h_of_keys_x(b.Pq[:, :, i], f.thr, f.mglo, f.mghi, f.kind, f.leaf_off,
                                                      f.leaf_len, trace=b.trace) for i in range(nq)]
            else:
                b.ranges = [dr.candidates_h_of_keys(b.Pq[:, :, i], f.thr, f.mglo, f.mghi, self.n, self.L,
                                                    self.min_leaf, trace=b.trace) for i in range(nq)]
            b.nranges = np.array([[len(tree) for tree in rg] for rg in b.ranges])          # [nq][T]
            b.cands = [[np.concatenate([f.perm[t, o:o + m] for o, m, _ in tree] + [np.empty(0, np.int32)])
                        for t, tree in enumerate(rg)] for rg in b.ranges]
            b.flat = [np.concatenate(c) for c in b.cands]
            b.total = sum(len(c) for c in b.flat)
            self.batches[key] = b
        return self.batches[key]


_sources = {}


def source(rp, ctx, *args, **kw):
    key = args + tuple(sorted(kw.items()))
    if key not in _sources:
        _sources[key] = Source(rp, ctx, *args, **kw)
    return _sources[key]


# --------------------------------------------------------------------------- (a) the keys
def check_keys(s, b, oracle):
    """exact mode: the bits of the reference's order of summation; else within the mode's bound of the f64
    contraction of the exactly widened rows (finite queries; a non-finite query's keys are only
    required to be deterministic, which batch() asserted)"""
    P = b.Pq.reshape(s.T * s.L, b.nq)
    R = s.R.reshape(s.T * s.L, s.d)
    fin = np.nonzero(b.finite)[0]
    if s.exact:
        Xq = b.Q.astype(P.dtype)
        rows = np.arange(b.nq) if not s.csr else fin     # (CSR: a stored NaN meets only what the row stores)
        for c in range(len(R)):
            split_ref.assert_same_bits(P[c, rows], inner_exact(Xq[rows], R[c]), "%s %s key column %d" % (s.name(), b.kind, c))
        if P.dtype == np.float64 and s.T <= 5:           # ... which is the oracle's innerSD / innerSS there
            for i in fin[:3]:
                qi = np.nonzero(b.Q[i])[0]
                for c in range(len(R)):
                    idx = np.nonzero(R[c])[0]
                    want = (oracle.inner_ss(idx, R[c, idx], qi, b.Q[i, qi]) if s.csr
                            else oracle.inner_sd(idx, R[c, idx], b.Q[i]))
                    assert P[c, i] == want, (s.name(), b.kind, c, i)
        return
    Rq = s.Rq.reshape(s.T * s.L, s.d)
    want = Rq @ b.Q[fin].T
    scale = np.linalg.norm(Rq, axis=1)[:, None] * np.linalg.norm(b.Q[fin], axis=1)[None, :]
    err = np.abs(P[:, fin].astype(np.float64) - want)
    tol = tol_of(s.src, s.d)
    assert (err <= tol * scale + 1e-300).all(), "%s %s x %d: a key %.3g |x||r| off, the bound is %.3g" % (
        s.name(), b.kind, b.nq, float((err / (scale + 1e-300)).max()), tol)
    if s.kind == "lattice" and b.kind in ("fresh", "stored", "x8", "gap", "mid"):
        assert np.array_equal(P[:, fin], want)           # small integers and quarters: exact in every arithmetic


# --------------------------------------------------------------------------- (b) the candidate lists
def check_candidates(s, b):
    off, ids = s.rp.candidatesBatch(s.f, b.qd)
    lens = np.array([len(c) for cs in b.cands for c in cs])
    want_off = np.concatenate([[0], np.cumsum(lens)])
    if not np.array_equal(off, want_off):
        j = int(np.argmax(np.diff(off) != lens))
        raise AssertionError("%s %s x %d: query %d, tree %d has %d candidates, the reference descent of its keys %d (keys %r)"
                             % (s.name(), b.kind, b.nq, j // s.T, j % s.T, off[j + 1] - off[j], lens[j],
                                b.Pq[j % s.T, :, j // s.T].tolist()))
    want = np.concatenate(b.flat) if b.total else np.empty(0, np.int32)
    if not np.array_equal(ids, want):
        p = int(np.argmax(ids != want))
        j = int(np.searchsorted(off, p, side="right")) - 1
        raise AssertionError("%s %s x %d: query %d, tree %d: other ids than the reference descent"
                             % (s.name(), b.kind, b.nq, j // s.T, j % s.T))


def kinds_of(nq):
    return dr.QUERY_KINDS if nq <= 17 else ("fresh", "mid", "mixed")


# source, rows, n, d, T, min_leaf: C = T L on both sides of the projection kernels' column switches
# (2: C <= 16 and CSR's 16-column kernel; 3; 5: C > 32; 33: 96 + 96 + a tail), row lengths for every
# kernel (bf16: 64 A resident, 264 A streamed, 36 the f32-MFMA fallback), deep trees at min_leaf 1
CASES = [
    ("f64_mfma", "lattice", 5000, 16, 3, 40), ("f64_mfma", "cont", 1023, 128, 5, 1), ("f64_mfma", "cont", 5000, 16, 33, 40),
    ("f64_mfma", "cont", 2500, 16, 2, 1),
    ("f64_exact", "lattice", 5000, 16, 3, 40), ("f64_exact", "cont", 1023, 16, 5, 1), ("f64_exact", "cont", 5000, 128, 33, 40),
    ("f32", "lattice", 5000, 16, 3, 40), ("f32", "cont", 1023, 16, 5, 1), ("f32", "cont", 5000, 128, 33, 40),
    ("f32", "cont", 2500, 128, 2, 1), ("f32", "lattice", 1023, 16, 5, 1),
    ("bf16", "lattice", 5000, 64, 3, 40), ("bf16", "cont", 1023, 64, 5, 1), ("bf16", "cont", 5000, 264, 33, 40),
    ("bf16", "cont", 2500, 36, 2, 1), ("bf16", "lattice", 1023, 36, 5, 1),
    ("bf16_terms3", "cont", 5000, 64, 5, 40), ("bf16_terms3", "lattice", 1023, 264, 3, 1), ("bf16_terms3", "cont", 2500, 36, 33, 40),
    ("bf16_f32", "cont", 5000, 64, 3, 40), ("bf16_f32", "cont", 1023, 264, 5, 1),
    ("csr_f64", "lattice", 5000, 64, 2, 40), ("csr_f64", "cont", 1023, 64, 5, 1), ("csr_f64", "cont", 5000, 64, 33, 40),
    ("csr_f32", "lattice", 5000, 64, 3, 40), ("csr_f32", "cont", 1023, 64, 5, 1),
    ("csr_mfma", "lattice", 5000, 64, 2, 40), ("csr_mfma", "cont", 1023, 64, 5, 1), ("csr_mfma", "cont", 5000, 64, 33, 40),
    ("csr_mfma_nodense", "lattice", 5000, 64, 3, 40), ("csr_mfma_nodense", "cont", 2500, 64, 5, 1),
]


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_keys_and_candidates_of_every_query(rp, ctx, oracle, case):
    """(a) and (b): every batch size, every kind of query, every query, every tree"""
    s = source(rp, ctx, *case)
    tr = dr.Trace()
    nr = []
    with s.on():
        for nq in NQS:
            for kind in kinds_of(nq):
                b = s.batch(kind, nq)
                check_keys(s, b, oracle)
                check_candidates(s, b)
                tr.add(b.trace)
                nr.append(b.nranges.ravel())
    nr = np.concatenate(nr)
    print("%s: %d (query, tree) pairs, %d with >= 2 ranges, %d with >= 3; %s" % (s.name(), len(nr), (nr >= 2).sum(), (nr >= 3).sum(), tr))
    assert tr.nan_keys > 0 and (tr.inf_keys > 0 or not s.exact)      # (0 * inf = NaN on the matrix pipe)
    if s.kind == "lattice":
        assert tr.key_eq_thr >= 20 and tr.dl_eq_dr >= 100
    if s.min_leaf == 1:
        assert (nr >= 3).sum() >= 5 and tr.both >= 40


# --------------------------------------------------------------------------- streamed forests
STREAMED = [("f64_exact", 4000, 12, 3, 20, 33), ("f64_exact", 4000, 12, 3, 20, 100), ("f32", 4000, 16, 3, 20, 33),
            ("f64_mfma", 3000, 16, 5, 0, 64), ("csr_f64", 4000, 64, 3, 20, 33), ("csr_mfma", 4000, 64, 2, 20, 100)]


@pytest.mark.parametrize("case", STREAMED, ids=["-".join(map(str, c)) for c in STREAMED])
def test_streamed_forests(rp, ctx, oracle, case):
    """rp.forest with chunks smaller than the data: the walk over the explicit topology (traverse_x),
    dense and SVector rows; a short last chunk drops subtrees (absent slots), Tips may be empty"""
    src, n, d, T, ml, chunk = case
    s = source(rp, ctx, src, "cont", n, d, T, ml, chunk=chunk)
    f = s.f
    empty = int(((f.kind == 2) & (f.leaf_len == 0)).sum())
    print("%s chunk %d: held %d of %d, dropped %d, %d empty Tips" % (s.name(), chunk, f.held, n, f.dropped, empty))
    if chunk == 33:
        assert f.dropped > 0 and f.held < n
    with s.on():
        for nq in (1, 17, 130):
            for kind in ("fresh", "mid", "near", "stored", "mixed"):
                b = s.batch(kind, nq)
                check_keys(s, b, oracle)
                check_candidates(s, b)
        b = s.batch("mid", 17)
        assert (b.nranges >= 2).any()
        if not s.csr:
            check_knn(s, b, ("default", "general"), oracle=oracle)
        check_knn_h(s, b)


# --------------------------------------------------------------------------- (c) every kNN path
def csr_reference_metric(s, b, oracle):
    """D[i][j]: the reference's metricSSL2 (through the oracle) of query i to its j-th reference candidate"""
    X, out = s.X, []
    for i, c in enumerate(b.flat):
        qi = np.nonzero(b.Q[i])[0]
        u, inv = np.unique(c, return_inverse=True)
        du = np.array([oracle.metric_ss(np.nonzero(X[r])[0], X[r][X[r] != 0], qi, b.Q[i, qi]) for r in u])
        out.append(du[inv] if len(u) else np.empty(0))
    return out


def want_knn(s, b, k, oracle):
    """the cell's reference applied to the REFERENCE candidate list -> per query a checker of (ids, dist, cnt)"""
    if s.csr:                                            # the reference metric, bit for bit
        D = csr_reference_metric(s, b, oracle)
        return [(lambda ids, dist, cnt, c=c, Di=Di: l2ref.mismatch(ids, dist, cnt, l2ref.select(c, Di, k, 0)))
                for c, Di in zip(b.flat, D)]
    if s.elem == "f64":                                  # the fold definition, bit for bit
        return [(lambda ids, dist, cnt, c=c, q=q: l2ref.mismatch(ids, dist, cnt, l2ref.select(c, l2ref.fold_l2(s.X[c], q), k, 0)))
                for c, q in zip(b.flat, b.Q)]
    D = []
    for c, q in zip(b.flat, b.Q):
        u, inv = np.unique(c, return_inverse=True)
        D.append(f32ref.exact_dist(s.X[u], q)[inv] if len(u) else np.empty(0))
    if s.kind == "lattice":                              # f32 arithmetic is exact: the definition, bit for bit

        def exact(ids, dist, cnt, c, Di):
            wi, wd, wc = f32ref.knn_from_candidates(c, Di, k, f32ref.KEEP)
            ok = cnt == wc and np.array_equal(ids, wi) and f32ref.same_bits(dist, wd)
            return None if ok else "not the definition's answer"
        return [(lambda ids, dist, cnt, c=c, Di=Di: exact(ids, dist, cnt, c, Di)) for c, Di in zip(b.flat, D)]
    return [(lambda ids, dist, cnt, c=c, Di=Di: f32ref.interval_violation(c, Di, ids, dist, cnt, k, f32ref.KEEP, s.d))
            for c, Di in zip(b.flat, D)]


def check_knn(s, b, paths, k=10, oracle=None):
    assert b.finite.all() or s.elem == "f64"
    checks = want_knn(s, b, k, oracle)
    bad = []
    for path in paths:
        if path == "l2_exact" and s.elem != "f64":
            continue
        with s.on(**PATHS[path]):
            ids, dist, cnt = s.rp.knnBatch(k, s.f, b.qd, reference_metric=s.csr)
            total = last_candidates(s.ctx)
        if total != b.total:
            bad.append((path, "rpt_knn_last_candidates %d, the reference total %d" % (total, b.total)))
        for i, chk in enumerate(checks):
            why = chk(ids[i], dist[i], int(cnt[i]))
            if why:
                bad.append((path, i, why))
    assert not bad, (s.name(), b.kind, b.nq, len(bad), bad[:8])


KNN_CASES = [
    # source, rows, n, d, T, min_leaf, nq (the last wave of 64 / T queries partly empty), query kinds
    ("f64_mfma", "cont", 1023, 16, 3, 1, 17, ("mid", "mixed")), ("f64_mfma", "lattice", 5000, 16, 7, 40, 5, ("gap", "fresh")),
    ("f64_exact", "cont", 1023, 16, 33, 1, 17, ("mid",)), ("f64_mfma", "cont", 1023, 16, 64, 1, 5, ("mid", "fresh")),
    ("f32", "cont", 1023, 16, 3, 1, 17, ("mid", "near")), ("f32", "lattice", 1023, 16, 7, 1, 17, ("gap", "mid", "x8")),
    ("f32", "cont", 1023, 16, 33, 1, 5, ("mid",)), ("f32", "cont", 1023, 16, 64, 1, 17, ("mid", "fresh")),
    ("f32", "lattice", 5000, 16, 3, 40, 64, ("fresh", "stored")),
    ("f32", "cont", 1023, 16, 200, 1, 17, ("mid",)), ("f32", "cont", 1023, 16, 600, 1, 5, ("mid",)),
    ("f64_mfma", "cont", 1023, 16, 200, 1, 5, ("mid",)), ("f64_mfma", "cont", 1023, 16, 600, 1, 5, ("mid",)),
    ("bf16", "cont", 1023, 64, 7, 1, 17, ("mid", "near")), ("bf16", "lattice", 1023, 36, 3, 1, 17, ("gap", "mid")),
    ("bf16_terms3", "lattice", 5000, 64, 33, 40, 5, ("fresh", "gap")), ("bf16_f32", "cont", 1023, 264, 64, 1, 5, ("mid",)),
    # rows in two clusters per level and queries in the gap: 2^m leaves per tree.  T = 64: totals on either side of
    # kWR = 128 (fan1) and of kFR = 512 (fan3); T = 3, 7: dozens of ranges in ONE tree
    ("f32", "axes", 1023, 16, 64, 1, 17, ("fan1", "fan3")), ("f64_mfma", "axes", 1023, 16, 64, 1, 17, ("fan1", "fan3")),
    ("bf16", "axes", 1023, 64, 64, 1, 17, ("fan1", "fan3")), ("f32", "axes", 1023, 16, 7, 1, 17, ("fan4",)),
    ("f64_exact", "axes", 1023, 16, 3, 1, 17, ("fan4",)),
    ("csr_f64", "cont", 1023, 64, 7, 1, 17, ("mid", "near")), ("csr_f32", "lattice", 5000, 64, 3, 40, 17, ("fresh", "gap")),
    ("csr_mfma", "cont", 1023, 64, 33, 1, 5, ("mid",)), ("csr_mfma_nodense", "lattice", 5000, 64, 3, 40, 17, ("gap", "stored")),
]


@pytest.mark.parametrize("case", KNN_CASES, ids=["-".join(map(str, c[:7])) for c in KNN_CASES])
def test_every_knn_path_answers_from_the_reference_candidates(rp, ctx, oracle, case):
    """(c): rpt_knn_last_candidates is the reference total and the answer is the cell's reference applied
    to the reference descent's candidate list, on every path, every query"""
    *src, nq, kinds = case
    s = source(rp, ctx, *src)
    T = s.T
    for kind in kinds:
        b = s.batch(kind, nq)
        check_candidates(s, b)
        check_knn(s, b, PATHS, oracle=oracle)
        tot = b.nranges.sum(axis=1)
        print("%s %s x %d: ranges per query %d .. %d, per (query, tree) up to %d; %d queries above kWR = 128, %d above kFR = 512"
              % (s.name(), kind, nq, tot.min(), tot.max(), b.nranges.max(), (tot > K_WR).sum(), (tot > K_FR).sum()))
        if s.min_leaf == 1 and kind == "mid":
            assert (b.nranges >= 3).any()                # shard_ranges_kernel's re-walk, the slots' second pass
        if T == 64 and kind == "fan1" and s.elem != "bf16":         # the one-wave kernels hand queries to the general path
            assert (tot > K_WR).any() and (tot <= K_WR).any()
        if T == 64 and kind == "fan3":                   # ... and so does the workgroup kernel (knn_wave = 0)
            assert (tot > K_FR).any() and (tot <= K_FR).any()
        if kind == "fan4":
            assert b.nranges.max() >= 8
        if T == 200:                                     # slots of 2 per tree: a tree outgrows them, the slab holds all
            assert ((b.nranges.max(axis=1) > K_FR // T) & (tot <= K_FR)).any()
        if T == 600:                                     # no slots, and more ranges than the slab: the general path
            assert (tot > K_FR).all()


# --------------------------------------------------------------------------- (d) knnH
def check_knn_h(s, b, ks=(1, 10, 100)):
    assert b.finite.all()
    for k in ks:
        off, ids, _ = s.rp.knnHBatch(k, s.f, b.qd)
        want = [dr.knn_h_ids(s.f.perm, rg, k) for rg in b.ranges]
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])])), (s.name(), b.kind, k)
        assert np.array_equal(ids, np.concatenate(want)), (s.name(), b.kind, k)


KNNH_CASES = [("f32", "cont", 1023, 16, 5, 1), ("f32", "lattice", 5000, 16, 3, 40), ("bf16", "cont", 1023, 64, 5, 1),
              ("bf16", "lattice", 5000, 64, 3, 40), ("bf16_f32", "cont", 5000, 64, 3, 40)]


@pytest.mark.parametrize("case", KNNH_CASES, ids=["-".join(map(str, c)) for c in KNNH_CASES])
def test_knn_h_takes_the_reference_buckets(rp, ctx, case):
    """(d): offsets and ids are the reference selection over the reference ranges and priorities"""
    s = source(rp, ctx, *case)
    with s.on():
        for kind, nq in (("mid", 17), ("near", 5), ("fresh", 64), ("gap", 1), ("stored", 17)):
            check_knn_h(s, s.batch(kind, nq))


# --------------------------------------------------------------------------- (e) build keys against query keys
BUILD_QUERY = [(src, "cont", 5000, 64 if SOURCES[src][0] in ("bf16", "csr64", "csr32") else 16, 3, 40) for src in SOURCES]
BUILD_QUERY.append(("csr_mfma", "cont", 70000, 64, 2, 40))          # the build projects on the dense-ified bf16 path


@pytest.mark.parametrize("case", BUILD_QUERY, ids=["-".join(map(str, c)) for c in BUILD_QUERY])
def test_stored_rows_as_queries_against_the_build_keys(rp, ctx, case):
    """64 stored rows sent back as queries: the key a row got at build time and the key it gets as a
    query are within twice the mode's bound of each other (both are within the bound of one number:
    that is all the contract gives), and bit-equal in exact mode.  Printed, not asserted: the share of
    bit-equal keys, and the rows on tie-free keys that do not find themselves."""
    s = source(rp, ctx, *case)
    rows = np.random.default_rng(5).choice(s.n, 64, replace=False)
    Q = s.X[rows]
    with s.on():
        qd = dataset(rp, ctx, s.elem, Q)
        Pq = s.project(qd)
        Pb = np.ascontiguousarray(s.f.proj()[:, :, rows])
        off, ids = rp.candidatesBatch(s.f, qd)
    assert Pq.dtype == Pb.dtype
    share = float((Pq.view(np.uint8).reshape(Pq.shape + (-1,)) == Pb.view(np.uint8).reshape(Pb.shape + (-1,))).all(axis=-1).mean())
    if s.exact:
        assert share == 1.0
    else:
        scale = np.linalg.norm(s.Rq, axis=2)[:, :, None] * np.linalg.norm(Q, axis=1)[None, None, :]
        err = np.abs(Pq.astype(np.float64) - Pb.astype(np.float64))
        assert (err <= 2 * tol_of(s.src, s.d) * scale + 1e-300).all(), float((err / scale).max())
    lost = pairs = 0
    f = s.f
    for i in range(64):
        rg = dr.candidates_of_keys(Pq[:, :, i], f.thr, f.mglo, f.mghi, s.n, s.L, s.min_leaf)
        for t in range(s.T):
            got = ids[off[i * s.T + t]:off[i * s.T + t + 1]]
            assert np.array_equal(got, np.concatenate([f.perm[t, o:o + m] for o, m in rg[t]]))
            tr = dr.Trace()
            dr.candidates_of_keys(Pq[t:t + 1, :, i], f.thr[t:t + 1], f.mglo[t:t + 1], f.mghi[t:t + 1], s.n, s.L, s.min_leaf, trace=tr)
            if tr.key_eq_thr == 0:
                pairs += 1
                lost += rows[i] not in got
    print("%s: %.4f of the query keys bit-equal to the build keys; %d of %d (row, tree) pairs on tie-free keys do not find themselves"
          % (s.name(), share, lost, pairs))
