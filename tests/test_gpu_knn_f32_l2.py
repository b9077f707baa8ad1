"""The L2 kNN on dense f32 and bf16 rows against an independent f64 reference (tests/knn_f32_ref.py,
pinned to the oracle by tests/test_knn_f32_host.py): every query, every query path on its own.

The candidate list the reference ranks is the device's own `candidatesBatch` (the traversal is pinned
elsewhere; rpt_knn_last_candidates must agree with it), so this file pins distance and selection:

  3a  lattice rows, on which f32 arithmetic is exact: ids, distance bits and counts EQUAL the
      definition under all three duplicate rules; also scaled by 2^40 / 2^-40, and with vote = 2;
  3b  continuous and hostile rows: `check_interval`, the kernels' stated error bound and everything
      the definition implies with it, and all paths bit-identical to each other;
  3c  bruteKnn and recallHits' truth under L2, the same two ways."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_f32_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PATHS = {
    "default": {},
    "wave": {"knn_wave": 1},
    "workgroup": {"knn_wave": 0},
    "general": {"knn_general": 1},
    "no_pre8": {"knn_no_pre8": 1},
    "no_pre16": {"knn_no_pre16": 1},
    "shard_old": {"knn_wave": 1, "knn_shard_old": 1},
    "kp8": {"knn_kp8": 58},                              # bf16 rows only: opts them into the int8 tier
}
RULES = (ref.KEEP, ref.DEDUP, ref.DEDUP_DISTANCE)
CASES = [("f32", s) for s in ref.SHAPES_F32] + [("bf16", s) for s in ref.SHAPES_BF16]
TIERS = set()                                            # every rpt_knn_last_tier this file has seen


def case_id(c):
    return "%s-%s" % (c[0], "x".join(str(v) for v in c[1]))


def paths_of(dtype):
    return [p for p in PATHS if p != "kp8" or dtype == "bf16"]


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


@contextlib.contextmanager
def on_path(ctx, path, k):
    """the options of one path, switched for the enclosed calls (knn_kp8: 58, 200 at k = 50)"""
    old = []
    try:
        for name, v in PATHS[path].items():
            old.append((name, ctx.set_option(name, 200 if name == "knn_kp8" and k == 50 else v)))
        yield
    finally:
        for name, v in reversed(old):
            ctx.set_option(name, v)


def last(ctx, what, ctype=C.c_int64):
    from rptree_amd import _lib
    v = ctype(-1)
    _lib.check(getattr(_lib.lib(), "rpt_knn_last_" + what)(ctx._h, C.byref(v)))
    return int(v.value)


class Case:
    """rows X and queries Q (float32 arrays holding values of the element type) on the device, a
    forest over them built there (f32: exact mode, bf16: the default mode), the device's candidate
    list of every query and the true distance of every entry.  Built once, never changed."""

    def __init__(self, rp, ctx, dtype, X, Q, T, min_leaf, seed=9):
        n, d = X.shape
        self.dtype, self.d, self.T, self.ctx = dtype, d, T, ctx
        bf = dtype == "bf16"
        self.ds = rp.Dataset.dense(ctx, rp.to_bf16(X) if bf else X, dtype=rp.RPT_BF16 if bf else None)
        self.qd = rp.Dataset.dense(ctx, rp.to_bf16(Q) if bf else Q, dtype=rp.RPT_BF16 if bf else None)
        assert not bf or (np.array_equal(rp.from_bf16(rp.to_bf16(X)), X) and np.array_equal(rp.from_bf16(rp.to_bf16(Q)), Q))
        self.f = None
        if T:
            cfg = rp.rpTreeCfg(min_leaf, n, d)
            _, R = rp.gen.forest_hyperplanes(seed, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
            self.f = rp._build(ctx, self.ds, R, cfg.fpMaxTreeDepth, min_leaf, rp.RPT_PROJ_AUTO if bf else rp.RPT_PROJ_EXACT)
            self.off, flat = rp.candidatesBatch(self.f, self.qd)
            self.flat = flat
            self.cands = [flat[self.off[i * T]:self.off[(i + 1) * T]] for i in range(len(Q))]
            self.total = int(self.off[-1])
        else:                                            # brute force: every row, in id order
            self.cands = [np.arange(n, dtype=np.int32)] * len(Q)
        self.X64, self.Q64 = X.astype(np.float64), Q.astype(np.float64)
        self.D = []
        for c, q in zip(self.cands, self.Q64):
            u, inv = np.unique(c, return_inverse=True)
            self.D.append(ref.exact_dist(self.X64[u], q)[inv])
        for a in [X, Q, self.X64, self.Q64] + self.D + (self.cands if T else self.cands[:1]):
            a.setflags(write=False)
        self._ranked = {}

    def knn(self, rp, k, rule=ref.KEEP, vote=0):
        """knnBatch; the call must have visited exactly the candidates candidatesBatch lists"""
        got = rp.knnBatch(k, self.f, self.qd, dedup=rule, vote=vote)
        if vote or not self.ctx.get_option("knn_general"):       # (the general path ranks on no tier and reports none)
            TIERS.add(last(self.ctx, "tier", C.c_int32))
        assert last(self.ctx, "candidates") == self.total, "knn and candidatesBatch traverse differently"
        return got

    def want(self, k, rule):
        """the definition's answer to every query -> (ids[nq][k], dist[nq][k], cnt[nq])"""
        if rule not in self._ranked:
            self._ranked[rule] = [ref.ranked(c, D, rule) for c, D in zip(self.cands, self.D)]
        rows = [ref.padded(*r, k) for r in self._ranked[rule]]
        return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]),
                np.array([r[2] for r in rows], dtype=np.int32))


def differs(got, want):
    """None when two answers (ids, dist, cnt) are equal bit for bit, else where they first differ"""
    for name, a, b in zip(("ids", "dist", "cnt"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        if not np.array_equal(a, b):
            if a.shape != b.shape:
                return "%s: shape %s, want %s" % (name, a.shape, b.shape)
            i = np.argwhere(a != b)[0]
            return "%s of query %d (first at rank %s)" % (name, i[0], i[1:].tolist())
    return None


_cases = {}


def lattice_case(rp, ctx, dtype, shape, scale=1.0):
    key = ("lattice", dtype, shape, scale)
    if key not in _cases:
        n, d, T, ml = shape
        assert ref.lattice_is_exact(d)
        X, Q = ref.lattice_set(n, d, dtype, seed=5)
        _cases[key] = Case(rp, ctx, dtype, X * np.float32(scale), Q * np.float32(scale), T, ml)
    return _cases[key]


# ------------------------------------------------------------------ 3a. lattice rows: bit-exact
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lattice_rows_equal_the_definition_on_every_path(rp, ctx, case):
    """ids, distance bits (sqrt of the exact sum, in f64) and counts, all three duplicate rules,
    k in {1, 10, 24, 50}, every path against the reference on its own"""
    dtype, shape = case
    c = lattice_case(rp, ctx, dtype, shape)
    assert sum(len(D) - len(np.unique(D)) for D in c.D) > 20 * len(c.D)       # ties everywhere
    bad = []
    for rule in RULES:
        for k in ref.KS:
            want = c.want(k, rule)
            for path in paths_of(dtype):
                with on_path(ctx, path, k):
                    why = differs(c.knn(rp, k, rule), want)
                if why:
                    bad.append((path, rule, k, why))
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("shape", ref.SHAPES_F32, ids=lambda s: "x".join(map(str, s)))
def test_lattice_rows_scaled_by_powers_of_two(rp, ctx, shape):
    """the rows and queries times 2^40 and 2^-40 (squares stay normal and finite): the definition on
    the scaled rows, and the same ids with the distances scaled exactly"""
    base = lattice_case(rp, ctx, "f32", shape)
    bad = []
    for scale in (2.0 ** 40, 2.0 ** -40):
        c = lattice_case(rp, ctx, "f32", shape, scale)
        for rule in RULES:
            for k in (1, 10, 50):
                want, unscaled = c.want(k, rule), base.want(k, rule)
                for path in ("default", "no_pre8", "no_pre16", "general", "shard_old"):
                    with on_path(ctx, path, k):
                        got = c.knn(rp, k, rule)
                    why = differs(got, want) or differs(got, (unscaled[0], unscaled[1] * scale, unscaled[2]))
                    if why:
                        bad.append((scale, path, rule, k, why))
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lattice_rows_with_a_vote_of_two(rp, ctx, case):
    """RPT_KNN_VOTE(2): the candidates found by at least 2 trees, ascending, each once; the k best by
    (distance, id)"""
    dtype, shape = case
    c = lattice_case(rp, ctx, dtype, shape)
    voted = [ref.voted(cd, 2) for cd in c.cands]
    ranked = [ref.ranked(v, ref.exact_dist(c.X64[v], q), ref.KEEP) for v, q in zip(voted, c.Q64)]
    assert min(len(v) for v in voted) > 0
    bad = []
    for k in ref.KS:
        rows = [ref.padded(*r, k) for r in ranked]
        want = tuple(np.array([r[j] for r in rows]) for j in range(3))
        for path in ("default", "general", "no_pre16"):
            with on_path(ctx, path, k):
                why = differs(c.knn(rp, k, vote=2), want)
            if why:
                bad.append((path, k, why))
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ 3b. rounded arithmetic: the interval check
def family_case(rp, ctx, dtype, shape, kind):
    key = (kind, dtype, shape)
    if key not in _cases:
        n, d, T, ml = shape
        X, Q = ref.family_set(kind, n, d, dtype, seed=6)
        _cases[key] = Case(rp, ctx, dtype, X, Q, T, ml)
    return _cases[key]


def interval_failures(c, got, k, rule):
    """every query of one answer against check_interval; a row equal to the query is at distance 0.0"""
    ids, dist, cnt = got
    bad = []
    for i in range(len(c.cands)):
        why = ref.interval_violation(c.cands[i], c.D[i], ids[i], dist[i], cnt[i], k, rule, c.d)
        if why is None and np.any(dist[i][np.isin(ids[i], c.cands[i][c.D[i] == 0.0])] != 0.0):
            why = "a row equal to the query is not at distance 0.0"
        if why:
            bad.append((i, why))
    return bad


@pytest.mark.parametrize("kind", ref.FAMILIES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rounded_rows_pass_the_interval_check_on_every_path(rp, ctx, case, kind):
    """every query, k and path under the keep and dedup rules: each path's answer is held to
    check_interval on its own (an answer bit-equal to one already checked is not checked twice), and
    all the paths are bit-identical to each other"""
    dtype, shape = case
    c = family_case(rp, ctx, dtype, shape, kind)
    if kind == "self":
        assert all((D == 0.0).sum() >= 1 for D in c.D)
    bad = []
    for rule in (ref.KEEP, ref.DEDUP):
        for k in ref.KS:
            first, checked = None, set()
            for path in paths_of(dtype):
                with on_path(ctx, path, k):
                    got = c.knn(rp, k, rule)
                key = b"".join(a.tobytes() for a in got)
                if key not in checked:
                    checked.add(key)
                    bad += [(path, rule, k) + b for b in interval_failures(c, got, k, rule)]
                if first is None:
                    first = got
                elif differs(got, first):
                    bad.append((path, rule, k, "differs from the default path: " + differs(got, first)))
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ 3c. brute force and recall
BRUTE_CASES = [(t, s) for t in ("f32", "bf16") for s in ref.BRUTE_SHAPES]
NTIE = 25


def brute_lattice(n, d, dtype):
    """the lattice set, and NTIE different rows planted at scattered ids at distance exactly 1/2 from
    the last query (one coordinate moved by 1/2): they tie at the cut of every k <= NTIE"""
    X, Q = ref.lattice_set(n, d, dtype, seed=7)
    X, Q = X.copy(), Q.copy()
    rng = np.random.default_rng(8)
    q = np.clip(Q[-1], -7.5, 7.5)
    Q[-1] = q
    rows = rng.choice(n, NTIE, replace=False)
    moves = rng.permutation(2 * d)[:NTIE]                # (coordinate, sign): pairwise different rows
    for r, m in zip(rows, moves):
        X[r] = q
        X[r, m // 2] += np.float32(0.5 if m % 2 else -0.5)
    assert np.abs(X).max() <= ref.LATTICE_M
    return X, Q


@pytest.mark.parametrize("case", BRUTE_CASES, ids=case_id)
def test_brute_force_on_lattice_rows_equals_the_definition(rp, ctx, case):
    """bruteKnn: the k best of all rows by (distance, id), ids and distance bits; 25 rows tie at the
    cut of the last query for k = 1 and 10; k = 1024, the largest the entry point accepts, as well"""
    dtype, (n, d) = case
    X, Q = brute_lattice(n, d, dtype)
    c = Case(rp, ctx, dtype, X, Q, 0, 0)
    assert (c.D[-1] == 0.5).sum() == NTIE and (c.D[-1] < 0.5).sum() == 0
    bad = []
    for k in ref.BRUTE_KS + (1024,):
        ids, dist = rp.bruteKnn(c.ds, c.qd, k)
        want = c.want(k, ref.KEEP)
        why = differs((ids, dist), want[:2])
        if why:
            bad.append((k, why))
    assert not bad, bad


@pytest.mark.parametrize("kind", ["cont", "offset"])
@pytest.mark.parametrize("case", BRUTE_CASES, ids=case_id)
def test_brute_force_on_rounded_rows_passes_the_interval_check(rp, ctx, case, kind):
    dtype, (n, d) = case
    X, Q = ref.family_set(kind, n, d, dtype, seed=10)
    c = Case(rp, ctx, dtype, X, Q, 0, 0)
    bad = []
    for k in ref.BRUTE_KS:
        ids, dist = rp.bruteKnn(c.ds, c.qd, k)
        cnt = np.full(len(Q), min(k, n), dtype=np.int32)
        bad += [(k,) + b for b in interval_failures(c, (ids, dist, cnt), k, ref.KEEP)]
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("case", BRUTE_CASES, ids=case_id)
def test_recall_hits_on_lattice_rows(rp, ctx, case):
    """recallHits(metricL2): truth == the brute-force answer of the definition, hits[i][t] ==
    |candidates(t, q_i) & truth_i| counted in numpy from candidatesBatch"""
    dtype, (n, d) = case
    X, Q = brute_lattice(n, d, dtype)
    T = 4
    c = Case(rp, ctx, dtype, X, Q, T, 100)
    allrows = np.arange(n, dtype=np.int32)
    ranked = [ref.ranked(allrows, ref.exact_dist(c.X64, q), ref.KEEP) for q in c.Q64]
    for k in ref.BRUTE_KS:
        hits, truth = rp.recallHits(rp.metricL2, c.f, k, c.qd)
        want = np.array([r[0][:k] for r in ranked])
        assert np.array_equal(truth, want), k
        for i in range(len(Q)):
            for t in range(T):
                ct = c.flat[c.off[i * T + t]:c.off[i * T + t + 1]]
                assert hits[i, t] == len(np.intersect1d(ct, want[i])), (k, i, t)


# ------------------------------------------------------------------ the tiers all ran
def test_every_ranking_tier_ran(rp, ctx):
    """tiers 0 (the all-f32 kernel), 2 (half shadow) and 3 (int8 shadow) each answered at least one
    call of this file (this test makes the calls itself when it is run alone)"""
    c = lattice_case(rp, ctx, "f32", ref.SHAPES_F32[0])
    for path in ("default", "no_pre8", "no_pre16"):
        with on_path(ctx, path, 10):
            assert differs(c.knn(rp, 10), c.want(10, ref.KEEP)) is None
    assert {0, 2, 3} <= TIERS, TIERS
