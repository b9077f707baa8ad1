"""The cut of the L2 kNN on dense f64 rows, on inputs chosen to break it, against the host
restatement of the definition (tests/knn_l2_cut_ref.py), bit for bit and on every query path.

The device ranks the candidates on a lane-parallel sum and re-evaluates the best of them as the
reference's left fold.  These inputs put dozens of DIFFERENT rows with mathematically equal
distances (coordinate permutations of one row) around the k-th place, and T copies of two such rows
across it, so that a fixed margin of kept entries cannot hold every row the fold might prefer: the
cut has to be certified per query and an uncertified query answered on the fold alone.

Every forest is maxDepth-0 (one Tip per tree): every point is a candidate of every tree."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_l2_cut_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

PATHS = {
    "default": {},
    "pre32": {"knn_no_pre16": 1},
    "no_pre32": {"knn_no_pre32": 1},
    "wave": {"knn_no_pre32": 1, "knn_wave": 1},
    "workgroup": {"knn_no_pre32": 1, "knn_wave": 0},
    "general": {"knn_general": 1},
    "shard": {"knn_wave": 1},                          # the small-shard kernels (prefiltered tiers)
    "shard_old": {"knn_wave": 1, "knn_shard_old": 1},
}
K_FUSED = 64           # the fused kernels' largest k; a larger one takes the general path by itself
K_GENERAL = 1024


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


@pytest.fixture
def option(ctx):
    """option(name, value): context manager switching one option of the context for the enclosed calls"""
    @contextlib.contextmanager
    def switch(name, value):
        old = ctx.set_option(name, value)
        try:
            yield
        finally:
            ctx.set_option(name, old)
    return switch


@contextlib.contextmanager
def on_path(option, path):
    with contextlib.ExitStack() as st:
        for name, v in PATHS[path].items():
            st.enter_context(option(name, v))
        yield


class Flat:
    """a maxDepth-0 forest of T trees over the f64 rows X: the candidate list of a query is T
    copies of 0 .. n-1"""

    def __init__(self, rp, ctx, X, T):
        n, d = X.shape
        self.X, self.T = X, T
        self.ds = rp.Dataset.dense(ctx, np.ascontiguousarray(X))
        self.f = rp._build(ctx, self.ds, np.zeros((T, 0, d)), 0, 1, rp.RPT_PROJ_AUTO)
        self.cands = ref.flat_candidates(n, T)

    def close(self):
        self.f.close()
        self.ds.close()


_cache = {}


def band(name):
    """(X, Q, band mask, per query the fold values of every row): computed once, never changed"""
    if name not in _cache:
        X, Q, mask = ref.band_set(**ref.BANDS[name][0])
        Q = ref.with_nonfinite_queries(Q) if name == "d37" else Q
        vals = [ref.fold_l2(X, q) for q in Q]
        for a in (X, Q, mask) + tuple(vals):
            a.setflags(write=False)
        _cache[name] = (X, Q, mask, vals)
    return _cache[name]


def check(rp, fl, Q, vals, ks, dedups, tag):
    """knnBatch on fl for every (k, dedup) against the definition on the candidate values vals[i]
    (one array per query, in candidate order); returns the failures.  RPT_KNN_DEDUP_DISTANCE (2) is
    held to the definition as well, knnPQ's nub on the fold values: the wide band has fewer than 63
    different values, and the count says so."""
    bad = []
    for dedup in dedups:
        for k in ks:
            ids, dist, cnt = rp.knnBatch(k, fl.f, Q, dedup=dedup)
            for i in range(len(Q)):
                why = ref.mismatch(ids[i], dist[i], cnt[i], ref.select(fl.cands, vals[i], k, dedup))
                if why:
                    bad.append((tag, dedup, k, i, why))
    return bad


# ------------------------------------------------------------------ 1. the band, 2. the wide band
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(ref.BANDS))
def test_cut_inside_a_band_of_permutations(rp, ctx, option, name, path):
    """d37 also carries a NaN query and one whose squares overflow: both are answered (NaN and +inf
    tie, ranked by position) and the other queries of the batch are unaffected"""
    X, Q, _, vals = band(name)
    ks = ref.BANDS[name][1]
    fl = Flat(rp, ctx, X, 1)
    try:
        with on_path(option, path):
            bad = check(rp, fl, Q, vals, ks, (0, 1, 2), (name, path))
    finally:
        fl.close()
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ 3. copies
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("T", ref.COPY_TREES)
def test_cut_inside_the_copies_of_a_pair(rp, ctx, option, T, path):
    """T trees = T copies of every candidate; k inside the 2 T copies of a (row, permutation) pair:
    the copies of the member the lane-parallel sum prefers must not crowd out the other"""
    if "copies" not in _cache:
        X, Q = ref.copies_set()
        X.setflags(write=False)
        _cache["copies"] = (X, Q)
    X, Q = _cache["copies"]
    fl = Flat(rp, ctx, X, T)
    vals = [ref.fold_l2(X[fl.cands], Q[0])]
    ks = ref.copies_ks(12, T, K_GENERAL if path == "general" else K_FUSED)
    try:
        with on_path(option, path):
            bad = check(rp, fl, Q, vals, ks, (0, 1), ("copies", T, path))
    finally:
        fl.close()
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ 4. the re-run route
def test_tie_at_the_prefilter_cut_ends_on_the_definition(rp, ctx):
    """default options, duplicates kept, k = 10 inside a band at d = 128: the prefilter cannot
    certify its cut, and what answers the query again is the definition.  The band of 48 in 104
    rows never gets there (the small-shard kernels serve such a forest, and a tier that keeps
    k + 48 entries holds that band whole: 0 uncertified queries, measured on the parent as well), so
    this one is ref.RERUN_BAND: 300 permutations in 2706 rows."""
    X, Q, _ = ref.band_set(**ref.RERUN_BAND)
    k = ref.RERUN_K
    fl = Flat(rp, ctx, X, 1)
    try:
        ids, dist, cnt = rp.knnBatch(k, fl.f, Q)
        unc = rp.knn_last_uncertified(ctx)
        bad = [ref.mismatch(ids[i], dist[i], cnt[i], ref.select(fl.cands, ref.fold_l2(X, Q[i]), k, 0))
               for i in range(len(Q))]
    finally:
        fl.close()
    assert bad == [None] * len(Q), bad
    assert unc > 0, unc


def test_l2_exact_option_answers_as_the_default(rp, ctx, option):
    """knn_l2_exact = 1 sends every query to the exact variant: the same answers, every query counted"""
    X, Q, _, vals = band("d37")
    fl = Flat(rp, ctx, X, 3)
    bad = []
    try:
        vals3 = [np.tile(v, 3) for v in vals]
        for path in ("default", "no_pre32", "wave", "general"):
            with on_path(option, path), option("knn_l2_exact", 1):
                bad += check(rp, fl, Q, vals3, (1, 10, 33, 70), (0, 1, 2), ("exact", path))
                rp.knnBatch(10, fl.f, Q)
                assert rp.knn_last_uncertified(ctx) == len(Q), path
    finally:
        fl.close()
    assert not bad, (len(bad), bad[:12])


# ------------------------------------------------------------------ 5. brute force and recall
@pytest.mark.parametrize("name", ["d37", "d128", "wide"])
def test_brute_force_and_recall_truth_inside_the_band(rp, ctx, name):
    """bruteKnn (L2): the k best by (fold distance, id); recallHits' truth: the same ids"""
    X, Q, _, vals = band(name)
    Qf = np.ascontiguousarray(Q[:2])                   # (the finite queries)
    n = len(X)
    allids = np.arange(n, dtype=np.int32)
    fl = Flat(rp, ctx, X, 1)
    bad = []
    try:
        for k in ref.BANDS[name][1]:
            ids, dist = rp.bruteKnn(fl.ds, Qf, k)
            _, truth = rp.recallHits(None, fl.f, k, Qf)
            for i in range(len(Qf)):
                want = ref.select(allids, vals[i], k, 0)
                why = ref.mismatch(ids[i], dist[i], k, want)
                if why:
                    bad.append((name, k, i, why))
                if not np.array_equal(truth[i], want[0]):
                    bad.append((name, k, i, "recall truth"))
    finally:
        fl.close()
    assert not bad, (len(bad), bad[:12])
