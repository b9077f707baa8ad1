"""The kNN graph and its NN-descent rounds on SVector (CSR) rows under the cosine and inner-product
distances on the device (rpt_knn_graph_csr_metric_*, rpt_knn_graph_refine_csr_metric_*,
csrc/graph_csr.hip): ids, counts and distance BITS, no tolerance anywhere, against the numpy
restatement over dotS (tests/knn_graph_metric_csr_ref.py), against the independent brute-force
kernels, against the dense entry points on the dense-ified rows where every stored value is finite,
and on rows that store inf / NaN, where the dense entry points give another answer."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_metric_csr_ref as mc  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
NP = {"f64": np.float64, "f32": np.float32}
METRICS = mc.METRICS
DTYPES = ("f64", "f32")


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


@contextlib.contextmanager
def option(ctx, name, value):
    old = ctx.set_option(name, value)
    try:
        yield
    finally:
        ctx.set_option(name, old)


def distf(rp, metric):
    return {"cosine": rp.metricCosine, "inner": rp.metricInner, "l2": rp.metricL2, None: None}[metric]


def leaves_of(f):
    return mc.leaf_slices(f.topology())


def model_pairs(f, ordered=False):
    """the pair model of test_gpu_knn_graph_csr.py: every pair of a leaf once (leaf kernel) or both
    ways (tiled kernel), per tree"""
    tot = sum(s * (s - 1) // 2 for _, s in leaves_of(f))
    return f.T * tot * (2 if ordered else 1)


def cut(graph, k):
    """the first k of every row: the graph for k of a graph for a larger k (a prefix of a total order)"""
    ids, dist, cnt = graph
    return ids[:, :k].copy(), dist[:, :k].copy(), np.minimum(cnt, k).astype(np.int32)


def build(rp, ctx, csr, minl, T, seed=1234, maxd=None, hyperplanes=None):
    n, d = len(csr[0]) - 1, csr[3]
    cfg = rp.rpTreeCfg(minl, max(n, 2), d)
    maxd = cfg.fpMaxTreeDepth if maxd is None else maxd
    return rp.forestBatch(seed, maxd, minl, T, cfg.fpProjNzDensity, d, csr, ctx=ctx, hyperplanes=hyperplanes)


def reimport(rp, ctx, f, data):
    """f's trees over another carrier of the same points (dense-ified rows, or rows whose values changed)"""
    return rp.importForest(ctx, data, f.R, f.min_leaf, f.perm, f.thr, f.mglo, f.mghi, mode=f.mode)


def both_kernels(rp, ctx, f, metric, k, want, tag):
    got = rp.knnGraphMetricSV(distf(rp, metric), k, f)
    mc.assert_same_graph(got, want, tag + ", default kernel")
    pairs = rp.knnGraphLastPairs(ctx)
    with option(ctx, "graph_general", 1):
        tiled = rp.knnGraphMetricSV(distf(rp, metric), k, f)
        assert rp.knnGraphLastPairs(ctx) == model_pairs(f, ordered=True)
    mc.assert_same_graph(tiled, want, tag + ", graph_general")
    return got, pairs


# ---------------------------------------------------------------- 1: the grid, both kernels, both folds
_grid = {}


def grid_case(rp, ctx, dtype, d, density):
    """one set, forest and dotS matrix per (dtype, d, density); the references (at k = 64; smaller k
    are their prefixes) per metric on demand"""
    key = (dtype, d, density)
    if key not in _grid:
        n, T, minl = 1000, 4 + (d % 5), 40
        csr = mc.make_csr(d + int(100 * density), n, d, density, NP[dtype])
        if d == 200:                                          # one full row: longer than a piece of 64
            rows = mc.rows_of(csr)
            rows[5] = (np.arange(d, dtype=np.int32), np.random.default_rng(5).standard_normal(d).astype(NP[dtype]))
            csr = mc.from_rows(rows, d, NP[dtype])
        f = build(rp, ctx, csr, minl, T, seed=1234 + d)
        X, P = mc.dense(csr)
        _grid[key] = {"csr": csr, "f": f, "X": X, "G": mc.dots_matrix(X, P), "D": {}, "want": {}}
    return _grid[key]


def grid_ref(case, metric):
    if metric not in case["want"]:
        f = case["f"]
        case["D"][metric] = mc.dist_matrix(metric, case["G"])
        case["want"][metric] = mc.knn_graph_ref(case["X"], f.perm, leaves_of(f), 64, case["D"][metric])
    return case["D"][metric], case["want"][metric]


@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("density", [0.05, 0.3])
@pytest.mark.parametrize("d", [24, 70, 200])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_graph_matches_the_restatement(rp, ctx, metric, dtype, d, density, k, masked):
    case = grid_case(rp, ctx, dtype, d, density)
    f = case["f"]
    _, want64 = grid_ref(case, metric)
    assert f.data.is_csr and 4 <= f.T <= 8 and max(s for _, s in leaves_of(f)) <= 128
    with option(ctx, "graph_csr_masked", masked):
        got, pairs = both_kernels(rp, ctx, f, metric, k, cut(want64, k),
                                  "%s %s d %d density %g k %d masked %d" % (metric, dtype, d, density, k, masked))
    assert pairs == model_pairs(f)
    assert not (got[0] == np.arange(f.N, dtype=np.int32)[:, None]).any()   # no row lists itself


# ---------------------------------------------------------------- 2: against the independent kernels
@pytest.mark.parametrize("n", [100, 300])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_depth_zero_equals_the_brute_force_and_the_dense_graph(rp, ctx, metric, dtype, n):
    """one leaf of all points: row i is bruteKnn's answer for x_i with i removed; n = 100 takes the
    leaf kernel, n = 300 (above 128) the tiled kernel"""
    d, k = 40, 10
    csr = mc.make_csr(3 + n, n, d, 0.2, NP[dtype], empty=(9, 10))
    f = build(rp, ctx, csr, 10, 2, maxd=0)
    assert leaves_of(f) == [(0, n)]
    got = rp.knnGraphMetricSV(distf(rp, metric), k, f)
    assert rp.knnGraphLastPairs(ctx) == model_pairs(f, ordered=n > 128)
    bi, bd = rp.bruteKnn(f.data, csr, k + 1, metric=distf(rp, metric))
    for i in range(n):
        keep = np.nonzero(bi[i] != i)[0][:k]
        assert np.array_equal(got[0][i], bi[i, keep]), (i, got[0][i], bi[i])
        assert np.array_equal(mc.bits(got[1][i]), mc.bits(bd[i, keep])), i
        assert got[2][i] == k
    # every stored value is finite: bit-equal to the dense entry point on the dense-ified rows
    X = mc.densify(csr)
    dense = reimport(rp, ctx, f, X.astype(NP[dtype]))
    assert not dense.data.is_csr
    for kk in (k, 64):
        mc.assert_same_graph(rp.knnGraphMetricSV(distf(rp, metric), kk, f),
                             rp.knnGraphMetric(distf(rp, metric), kk, dense), "dense witness k %d" % kk)
    with option(ctx, "graph_csr_masked", 1):
        mc.assert_same_graph(rp.knnGraphMetricSV(distf(rp, metric), k, f), got, "masked")


@pytest.mark.parametrize("dtype,density", [("f64", 0.05), ("f32", 0.3)])
@pytest.mark.parametrize("metric", METRICS)
def test_dense_entry_point_on_the_densified_rows_gives_the_same(rp, ctx, metric, dtype, density):
    case = grid_case(rp, ctx, dtype, 70, density)
    f = case["f"]
    dense = reimport(rp, ctx, f, case["X"].astype(NP[dtype]))
    assert not dense.data.is_csr
    for k in (10, 64):
        mc.assert_same_graph(rp.knnGraphMetricSV(distf(rp, metric), k, f),
                             rp.knnGraphMetric(distf(rp, metric), k, dense), "witness k %d" % k)


# ---------------------------------------------------------------- 3: awkward rows in one set
EMPTY = [3, 50, 51, 400, 599]


def awkward_rows(d, dtype):
    n = 600
    rows = [(c.copy(), v.copy()) for c, v in mc.rows_of(mc.make_csr(7 + d, n, d, 0.3, NP[dtype]))]
    rng = np.random.default_rng(d)
    none = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=NP[dtype]))
    for e in EMPTY:
        rows[e] = none
    rows[7] = rows[17]                                      # exact duplicates under other ids
    rows[590] = rows[17]
    rows[31] = rows[30]
    rows[11] = (np.arange(d, dtype=np.int32), rng.standard_normal(d).astype(NP[dtype]))   # one full row
    cz = np.arange(0, d, 2, dtype=np.int32)                 # stored +0.0 and -0.0 entries
    vz = rng.standard_normal(len(cz)).astype(NP[dtype])
    vz[::2] = 0.0
    vz[::4] = -0.0
    rows[20] = (cz, vz)
    rows[23] = (np.array([0], dtype=np.int32), np.array([-0.0], dtype=NP[dtype]))         # nothing but a stored -0.0
    rows[21] = (np.array([0], dtype=np.int32), np.array([1.5], dtype=NP[dtype]))          # only column 0
    rows[22] = (np.array([d - 1], dtype=np.int32), np.array([-2.5], dtype=NP[dtype]))     # only column d - 1
    for i in range(60, 70):                                  # rows x 10
        rows[i] = (rows[i][0], rows[i][1] * NP[dtype](10))
    return mc.from_rows(rows, d, NP[dtype])


_awk = {}


def awkward_case(d, dtype):
    if (d, dtype) not in _awk:
        csr = awkward_rows(d, dtype)
        X, P = mc.dense(csr)
        _awk[(d, dtype)] = (csr, X, mc.dots_matrix(X, P))
    return _awk[(d, dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [33, 32, 1])
@pytest.mark.parametrize("metric", METRICS)
def test_awkward_rows(rp, ctx, metric, d, dtype):
    csr, X, G = awkward_case(d, dtype)
    D = mc.dist_matrix(metric, G)
    n = X.shape[0]
    f = build(rp, ctx, csr, 30, 4, seed=5 + d)
    for k in (10, 64):
        want = mc.knn_graph_ref(X, f.perm, leaves_of(f), k, D)
        for masked in (0, 1):
            with option(ctx, "graph_csr_masked", masked):
                both_kernels(rp, ctx, f, metric, k, want, "awkward %s d %d k %d masked %d" % (metric, d, k, masked))
    # all pairs (depth 0, one leaf of 600: the tiled kernel)
    k = 10
    f0 = build(rp, ctx, csr, 30, 1, maxd=0)
    got = rp.knnGraphMetricSV(distf(rp, metric), k, f0)
    mc.assert_same_graph(got, mc.knn_graph_ref(X, f0.perm, leaves_of(f0), k, D), "awkward, all pairs")
    zero = np.nonzero(np.diagonal(G) == 0.0)[0].tolist()      # empty and all-zero rows: dotS(x, x) is 0
    assert set(EMPTY + [23]) <= set(zero)
    if metric == "cosine":
        # their dotS(x, x) is 0: NaN against everything, so their lists are the first other ids ...
        for e in zero:
            others = [j for j in range(n) if j != e][:k]
            assert got[0][e].tolist() == others and np.isnan(got[1][e]).all()
        # ... and in a list that holds NaN entries they come last, by id
        D64 = mc.knn_graph_ref(X, f0.perm, leaves_of(f0), 64, D)
        g64 = rp.knnGraphMetricSV(distf(rp, metric), 64, f0)
        mc.assert_same_graph(g64, D64, "awkward, all pairs, k 64")
        small = mc.from_rows(mc.rows_of(csr)[:40], d, NP[dtype])          # 40 rows, k = 39: every list holds row 3 last
        fs = build(rp, ctx, small, 30, 1, maxd=0)
        gs = rp.knnGraphMetricSV(distf(rp, metric), 39, fs)
        Xs, Ps = mc.dense(small)
        mc.assert_same_graph(gs, mc.knn_graph_ref(Xs, fs.perm, leaves_of(fs), 39,
                                                  mc.dist_matrix(metric, mc.dots_matrix(Xs, Ps))), "awkward, 40 rows")
        zs = [z for z in zero if z < 40]
        for i in range(40):
            if i in zs:
                continue
            tail = gs[0][i, 39 - len(zs):].tolist()
            assert tail == zs and np.isnan(gs[1][i, 39 - len(zs):]).all() and not np.isnan(gs[1][i, :39 - len(zs)]).any()
    else:
        # row 23 stores nothing but -0.0: every dotS with it is +0.0, every distance -0.0, and the id decides
        others = [j for j in range(n) if j != 23][:k]
        assert got[0][23].tolist() == others
        assert np.all(got[1][23] == 0.0) and np.signbit(got[1][23]).all()
        if d > 1:
            # rows 21 and 22 store disjoint single columns: -0.0, bits kept
            assert D[21, 22] == 0.0 and np.signbit(D[21, 22])
            small = mc.from_rows(mc.rows_of(csr)[20:24], d, NP[dtype])     # rows 20 .. 23 alone: 21 and 22 are mates
            fs = build(rp, ctx, small, 30, 1, maxd=0)
            gs = rp.knnGraphMetricSV(distf(rp, metric), 3, fs)
            Xs, Ps = mc.dense(small)
            mc.assert_same_graph(gs, mc.knn_graph_ref(Xs, fs.perm, leaves_of(fs), 3,
                                                      mc.dist_matrix(metric, mc.dots_matrix(Xs, Ps))), "awkward, 4 rows")
            at = gs[0][1].tolist().index(2)
            assert gs[1][1][at] == 0.0 and np.signbit(gs[1][1][at])
            zeros = [j for j, v in zip(gs[0][1].tolist(), gs[1][1].tolist()) if v == 0.0]
            assert zeros == sorted(zeros)                                   # -0.0 ties with +0.0: by id


# ---------------------------------------------------------------- 4: stored inf and NaN
_bad = {}


def bad_case(rp, ctx, dtype):
    """600 x 33; a few rows store +inf, -inf and NaN, some in a column their mates store, some in a
    column that few rows store.  The trees are built on the rows with those values replaced by finite
    ones (nothing non-finite is projected) and imported over the real rows."""
    if dtype not in _bad:
        n, d = 600, 33
        csr = mc.make_csr(77, n, d, 0.3, NP[dtype])
        rowptr, col, val, _ = csr
        finite = val.copy()
        val = val.copy()
        rng = np.random.default_rng(4)
        special = {}
        for i, v in zip(rng.choice(n, size=12, replace=False), [np.inf, -np.inf, np.nan] * 4):
            if rowptr[i + 1] > rowptr[i]:
                at = rowptr[i] + int(rng.integers(rowptr[i + 1] - rowptr[i]))
                val[at] = v
                special[int(i)] = int(col[at])
        assert len(special) >= 9
        bad = (rowptr, col, val, d)
        f_fin = build(rp, ctx, (rowptr, col, finite, d), 40, 4, seed=31)
        f = reimport(rp, ctx, f_fin, bad)
        assert f.data.is_csr and max(s for _, s in leaves_of(f)) <= 128
        X, P = mc.dense(bad)
        _bad[dtype] = {"csr": bad, "f": f, "X": X, "P": P, "G": mc.dots_matrix(X, P), "special": special}
    return _bad[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_stored_inf_and_nan(rp, ctx, metric, dtype):
    case = bad_case(rp, ctx, dtype)
    f, X, P, G = case["f"], case["X"], case["P"], case["G"]
    D = mc.dist_matrix(metric, G)
    # some mates share the special column and some do not
    for i, c in case["special"].items():
        assert P[:, c].sum() > 1 and (~P[:, c]).sum() > 1
    k = 10
    want = mc.knn_graph_ref(X, f.perm, leaves_of(f), k, D)
    got, _ = both_kernels(rp, ctx, f, metric, k, want, "inf / NaN %s %s" % (metric, dtype))
    with option(ctx, "graph_csr_masked", 1):
        both_kernels(rp, ctx, f, metric, k, want, "inf / NaN %s %s, masked" % (metric, dtype))
    mc.assert_same_graph(rp.knnGraphMetricSV(distf(rp, metric), 64, f),
                         mc.knn_graph_ref(X, f.perm, leaves_of(f), 64, D), "inf / NaN k 64")
    # the dense entry point on the dense-ified rows meets inf * 0 = NaN: another answer, so the case bites
    dense = reimport(rp, ctx, f, X.astype(NP[dtype]))
    dg = rp.knnGraphMetric(distf(rp, metric), k, dense)
    differs = (dg[0] != got[0]).any(axis=1) | (mc.bits(dg[1]) != mc.bits(got[1])).any(axis=1)
    assert differs.any()
    # the refinement over the same rows
    for r, iters in ((10, 1), (0, 2)):
        rwant, rounds, upd, cand = mc.refine_ref(X, want, k, r, iters, D)
        rgot = rp.knnGraphRefineMetricSV(distf(rp, metric), got, f, iters=iters, reverse=r)
        assert rp.knnGraphRefineLast(ctx) == (rounds, upd, cand)
        mc.assert_same_graph(rgot, rwant, "inf / NaN refine r %d" % r)
    # depth 0 (one leaf of 600): the tiled kernel decides from the same statistic
    f0 = build(rp, ctx, case["csr"], 40, 1, maxd=0)           # nothing is projected at depth 0
    mc.assert_same_graph(rp.knnGraphMetricSV(distf(rp, metric), k, f0),
                         mc.knn_graph_ref(X, f0.perm, leaves_of(f0), k, D), "inf / NaN, all pairs")


# ---------------------------------------------------------------- 5: refinement
_steps = {}


def refine_steps(key, X, D, g0, k, r, iters):
    """the reference after `iters` rounds, taken one round at a time and kept: (graph, rounds,
    updates, candidates)"""
    st = _steps.setdefault(key, {"seq": [], "ended": False})
    seq = st["seq"]
    while len(seq) < iters and not st["ended"]:
        g, rounds, upd, cand = seq[-1] if seq else (g0, 0, 0, 0)
        new, one, u, c = mc.refine_ref(X, g, k, r, 1, D)
        seq.append((new, rounds + one, upd + u, cand + c))
        st["ended"] = u == 0
    return seq[min(iters, len(seq)) - 1]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("reverse", [0, 10])
@pytest.mark.parametrize("k", [5, 10])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_refine_matches_the_restatement(rp, ctx, metric, dtype, k, reverse, iters):
    case = grid_case(rp, ctx, dtype, 70, 0.05 if dtype == "f64" else 0.3)
    f, X = case["f"], case["X"]
    D, want64 = grid_ref(case, metric)
    g0 = cut(want64, k)
    want, rounds, upd, cand = refine_steps((metric, dtype, k, reverse), X, D, g0, k, reverse, iters)
    got = rp.knnGraphRefineMetricSV(distf(rp, metric), g0, f, iters=iters, reverse=reverse)
    stats = rp.knnGraphRefineLast(ctx)
    mc.assert_same_graph(got, want, "refine")
    assert stats == (rounds, upd, cand)
    # finite values: the dense entry point on the dense-ified data set gives the same bits and numbers
    dense = rp.Dataset.dense(ctx, X.astype(NP[dtype]))
    mc.assert_same_graph(rp.knnGraphRefineMetric(distf(rp, metric), g0, dense, iters=iters, reverse=reverse), got,
                         "dense refine")
    assert rp.knnGraphRefineLast(ctx) == stats
    with option(ctx, "graph_refine_general", 1):
        mc.assert_same_graph(rp.knnGraphRefineMetricSV(distf(rp, metric), g0, f.data, iters=iters, reverse=reverse),
                             got, "graph_refine_general")
        assert rp.knnGraphRefineLast(ctx) == stats


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_refine_hand_graph_long_rows_and_the_fixed_point(rp, ctx, metric, dtype):
    # a hand-made graph with short rows, over the d = 200 set whose row 5 is full (200 entries: x_5
    # passes through LDS in four pieces, and a candidate's row crosses a piece boundary)
    case = grid_case(rp, ctx, dtype, 200, 0.3)
    f, X = case["f"], case["X"]
    D, _ = grid_ref(case, metric)
    n, k = X.shape[0], 6
    assert np.diff(case["csr"][0])[5] == 200 and np.diff(case["csr"][0]).max() == 200
    rows = {i: [(i + 1) % n, (i * 7 + 3) % n] for i in range(0, n, 2)}
    rows.update({5: [6, 7, 8, 9, 10, 11, 12], 6: [5], 7: [], 999: [5, 0]})
    g0 = mc.hand_graph(D, k, rows)
    assert g0[2].min() == 0 and g0[2][5] == k and g0[2][1] == 0
    for r, iters in ((0, 1), (6, 1), (6, 3)):
        want, rounds, upd, cand = mc.refine_ref(X, g0, k, r, iters, D)
        got = rp.knnGraphRefineMetricSV(distf(rp, metric), g0, f, iters=iters, reverse=r)
        assert rp.knnGraphRefineLast(ctx) == (rounds, upd, cand)
        mc.assert_same_graph(got, want, "hand graph r %d iters %d" % (r, iters))
        with option(ctx, "graph_refine_general", 1):
            mc.assert_same_graph(rp.knnGraphRefineMetricSV(distf(rp, metric), g0, f, iters=iters, reverse=r), want,
                                 "hand graph, graph_refine_general")
    # an early end: a round that changes nothing is the last one applied
    small = mc.make_csr(8, 300, 30, 0.25, NP[dtype])
    Xs, Ps = mc.dense(small)
    Ds = mc.dist_matrix(metric, mc.dots_matrix(Xs, Ps))
    ds = rp.Dataset.csr(ctx, *small)
    perm = np.stack([np.arange(300), np.random.default_rng(300).permutation(300)]).astype(np.int32)
    s0 = mc.knn_graph_ref(Xs, perm, [(o, 20) for o in range(0, 300, 20)], 6, Ds)
    want, rounds, upd, cand = mc.refine_ref(Xs, s0, 6, 4, 50, Ds)
    assert 1 < rounds < 50
    got = rp.knnGraphRefineMetricSV(distf(rp, metric), s0, ds, iters=50, reverse=4)
    assert rp.knnGraphRefineLast(ctx) == (rounds, upd, cand)
    mc.assert_same_graph(got, want, "fixed point")
    same = rp.knnGraphRefineMetricSV(distf(rp, metric), got, ds, iters=3, reverse=4)
    assert rp.knnGraphRefineLast(ctx)[:2] == (1, 0)
    mc.assert_same_graph(same, got, "at the fixed point")


# ---------------------------------------------------------------- 6: accumulate
@pytest.mark.parametrize("metric,dtype,k", [("cosine", "f64", 10), ("inner", "f32", 64)])
def test_accumulate_folds_tree_shards_in_any_order(rp, ctx, metric, dtype, k):
    n, d, T, minl = 1000, 70, 5, 40
    csr = mc.make_csr(21, n, d, 0.3, NP[dtype])
    X, P = mc.dense(csr)
    D = mc.dist_matrix(metric, mc.dots_matrix(X, P))
    cfg = rp.rpTreeCfg(minl, n, d)
    _, R = rp.gen.forest_hyperplanes(99, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    whole, fa, fb = (build(rp, ctx, csr, minl, len(r), seed=0, hyperplanes=r) for r in (R, R[:2], R[2:]))
    assert np.array_equal(whole.perm, np.concatenate([fa.perm, fb.perm]))
    m = distf(rp, metric)
    g = rp.knnGraphMetricSV(m, k, whole)
    mc.assert_same_graph(g, mc.knn_graph_ref(X, whole.perm, leaves_of(whole), k, D), "whole")
    mc.assert_same_graph(rp.knnGraphMetricSV(m, k, fb, accumulate=rp.knnGraphMetricSV(m, k, fa)), g, "a then b")
    mc.assert_same_graph(rp.knnGraphMetricSV(m, k, fa, accumulate=rp.knnGraphMetricSV(m, k, fb)), g, "b then a")
    with option(ctx, "graph_general", 1):
        mc.assert_same_graph(rp.knnGraphMetricSV(m, k, fb, accumulate=rp.knnGraphMetricSV(m, k, fa)), g,
                             "a then b, tiled")
    with option(ctx, "graph_csr_masked", 1):
        mc.assert_same_graph(rp.knnGraphMetricSV(m, k, fa, accumulate=rp.knnGraphMetricSV(m, k, fb)), g,
                             "b then a, masked")


# ---------------------------------------------------------------- 7: metric 0
@pytest.mark.parametrize("dtype", DTYPES)
def test_metric_none_gives_the_l2_entry_points_bits(rp, ctx, dtype):
    case = grid_case(rp, ctx, dtype, 70, 0.3)
    f = case["f"]
    for k in (10, 64):
        base = rp.knnGraphSV(k, f)
        for m in (None, rp.metricL2):
            mc.assert_same_graph(rp.knnGraphMetricSV(m, k, f), base, "metric 0, k %d" % k)
        with option(ctx, "graph_general", 1), option(ctx, "graph_csr_masked", 1):
            mc.assert_same_graph(rp.knnGraphMetricSV(None, k, f), base, "metric 0, tiled")
    g0 = rp.knnGraphSV(10, f)
    want = rp.knnGraphRefineSV(g0, f, iters=2, reverse=10)
    stats = rp.knnGraphRefineLast(ctx)
    for m in (None, rp.metricL2):
        mc.assert_same_graph(rp.knnGraphRefineMetricSV(m, g0, f, iters=2, reverse=10), want, "metric 0 refine")
        assert rp.knnGraphRefineLast(ctx) == stats


# ---------------------------------------------------------------- 8: errors and side effects
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, T, minl, k = 1000, 16, 4, 30, 10
    csr = mc.make_csr(12, n, d, 0.3)
    X, P = mc.dense(csr)
    G = mc.dots_matrix(X, P)
    ds = rp.Dataset.csr(ctx, *csr)
    cfg = rp.rpTreeCfg(minl, n, d)
    _, R = rp.gen.forest_hyperplanes(7, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    f = rp.forestBatch(0, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx, hyperplanes=R)
    ids = np.empty((n, 64), dtype=np.int32)
    dist = np.empty((n, 64), dtype=np.float64)
    cnt = np.empty(n, dtype=np.int32)
    ptrs = lambda g: [C.c_void_p(a.ctypes.data) for a in g]  # noqa: E731
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, forest, data, kk, metric, flags):
        assert L.rpt_knn_graph_csr_metric_host(ctx._h, forest._h, data._h, kk, metric, flags,
                                               *ptrs((ids, dist, cnt))) == code
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        return msg

    dense = rp.Dataset.dense(ctx, mc.densify(csr))
    assert "rpt_knn_graph_*" in refused(RPT_E_ARG, f, dense, k, COS, 0)          # names the dense entry point
    assert "exclusive" in refused(RPT_E_ARG, f, ds, k, COS | INN, 0)
    assert "metric" in refused(RPT_E_ARG, f, ds, k, REF, 0)
    assert "metric" in refused(RPT_E_ARG, f, ds, k, 1, 0)
    for flag in (COS, INN, REF, 2):                                              # a metric bit in flags
        refused(RPT_E_ARG, f, ds, k, COS, flag)
    for kk in (0, 65, -3):
        assert "k" in refused(RPT_E_ARG, f, ds, kk, INN, 0)
    short = mc.from_rows(mc.rows_of(csr)[:-1], d)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.csr(ctx, *short), k, COS, 0)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.csr(ctx, csr[0], csr[1], csr[2].astype(np.float32), d), k,
                                 COS, 0)
    fs = rp.forest(0, cfg.fpMaxTreeDepth, minl, T, 500, cfg.fpProjNzDensity, d, ds, ctx=ctx, hyperplanes=R)
    for m in (COS, INN, 0):
        assert "streamed" in refused(RPT_E_UNSUPPORTED, fs, ds, k, m, 0)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphMetricSV(rp.metricCosine, 65, f)
    assert e.value.code == RPT_E_ARG
    with pytest.raises(NotImplementedError):
        rp.knnGraphMetricSV(lambda u, v: 0.0, k, f)

    # a correct call afterwards
    D = mc.dist_matrix("cosine", G)
    g0 = rp.knnGraphMetricSV(rp.metricCosine, k, f)
    want0 = mc.knn_graph_ref(X, f.perm, leaves_of(f), k, D)
    mc.assert_same_graph(g0, want0, "after the refusals")

    def rrefused(code, data, kk, r, iters, metric, flags, graph):
        assert L.rpt_knn_graph_refine_csr_metric_host(ctx._h, data._h, kk, r, iters, metric, flags,
                                                      *ptrs(graph)) == code
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        return msg

    work = lambda: tuple(a.copy() for a in g0)  # noqa: E731
    assert "rpt_knn_graph_refine_*" in rrefused(RPT_E_ARG, dense, k, k, 1, COS, 0, work())
    assert "exclusive" in rrefused(RPT_E_ARG, ds, k, k, 1, COS | INN, 0, work())
    assert "metric" in rrefused(RPT_E_ARG, ds, k, k, 1, REF, 0, work())
    for flag in (COS, INN, REF, 1):
        rrefused(RPT_E_ARG, ds, k, k, 1, COS, flag, work())
    assert "k" in rrefused(RPT_E_ARG, ds, 0, k, 1, COS, 0, work())
    assert "k" in rrefused(RPT_E_ARG, ds, 65, k, 1, COS, 0, work())
    assert "reverse" in rrefused(RPT_E_ARG, ds, k, 65, 1, INN, 0, work())
    assert "iters" in rrefused(RPT_E_ARG, ds, k, k, 0, INN, 0, work())
    bad = work()
    bad[0][703, 1] = bad[0][703, 0]
    assert "row 703" in rrefused(RPT_E_ARG, ds, k, k, 1, COS, 0, bad)
    bad = work()
    bad[0][12, 0] = n
    assert "row 12" in rrefused(RPT_E_ARG, ds, k, k, 1, COS, 0, bad)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphRefineMetricSV(rp.metricInner, g0, ds, iters=0)
    assert e.value.code == RPT_E_ARG

    # the dense metric entry points keep refusing CSR rows, and say where they go
    assert L.rpt_knn_graph_metric_host(ctx._h, f._h, ds._h, k, COS, 0, *ptrs((ids, dist, cnt))) == RPT_E_UNSUPPORTED
    assert "rpt_knn_graph_csr_metric_*" in L.rpt_last_error().decode()
    assert L.rpt_knn_graph_refine_metric_host(ctx._h, ds._h, k, k, 1, COS, 0, *ptrs(work())) == RPT_E_UNSUPPORTED
    assert "rpt_knn_graph_refine_csr_metric_*" in L.rpt_last_error().decode()
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphMetric(rp.metricCosine, k, f)
    assert e.value.code == RPT_E_UNSUPPORTED and "rpt_knn_graph_csr_metric_*" in str(e.value)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphRefineMetric(rp.metricCosine, g0, ds)
    assert e.value.code == RPT_E_UNSUPPORTED
    # the L2 CSR entry points keep refusing the metric bits in flags
    for flag in (COS, INN, REF):
        assert L.rpt_knn_graph_csr_host(ctx._h, f._h, ds._h, k, flag, *ptrs((ids, dist, cnt))) == RPT_E_UNSUPPORTED
        assert L.rpt_knn_graph_refine_csr_host(ctx._h, ds._h, k, k, 1, flag, *ptrs(work())) == RPT_E_UNSUPPORTED

    # the context answers correct calls: a round, and the graph again
    want1, rounds, upd, cand = mc.refine_ref(X, want0, k, k, 1, D)
    mc.assert_same_graph(rp.knnGraphRefineMetricSV(rp.metricCosine, g0, ds, iters=1), want1, "after the refusals, refine")
    assert rp.knnGraphRefineLast(ctx) == (rounds, upd, cand)
    mc.assert_same_graph(rp.knnGraphMetricSV(rp.metricCosine, k, f), want0, "again")


# ---------------------------------------------------------------- 9: device arrays
@pytest.mark.parametrize("metric", METRICS)
def test_dev_entry_points_with_torch_tensors(rp, ctx, metric):
    import torch
    case = grid_case(rp, ctx, "f64", 70, 0.3)
    f = case["f"]
    _, want64 = grid_ref(case, metric)
    n, k = f.N, 10
    m = distf(rp, metric)
    dev = torch.device("cuda", ctx.device)
    ids = torch.full((n, k), 7, dtype=torch.int32, device=dev)
    dist = torch.zeros((n, k), dtype=torch.float64, device=dev)
    cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.knnGraphMetricSVDev(m, k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    ctx.sync()
    assert rp.knnGraphLastPairs(ctx) == model_pairs(f)
    g0 = cut(want64, k)
    mc.assert_same_graph((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), g0, "dev")
    rp.knnGraphMetricSVDev(m, k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), accumulate=True)
    rp.knnGraphRefineMetricSVDev(m, k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), iters=3)
    ctx.sync()
    want = rp.knnGraphRefineMetricSV(m, g0, f, iters=3)
    mc.assert_same_graph((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), want, "dev refine")


# ---------------------------------------------------------------- 10: the C++ mirror
def checksum(graph):
    """host/example_knn_graph_sparse_metric.cpp's: sum of (bits(dist) ^ id * G) * (2 p + 1) over the
    slots p plus sum of count * (2 i + 1) * G over the rows i, wrapping in 64 bits"""
    ids, dist, cnt = graph
    G = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        bits = np.ascontiguousarray(dist, dtype=np.float64).ravel().view(np.uint64)
        idw = ids.ravel().astype(np.uint32).astype(np.uint64) * G
        p = np.arange(bits.size, dtype=np.uint64)
        h = ((bits ^ idw) * (np.uint64(2) * p + np.uint64(1))).sum(dtype=np.uint64)
        i = np.arange(cnt.size, dtype=np.uint64)
        h = h + (cnt.astype(np.uint32).astype(np.uint64) * (np.uint64(2) * i + np.uint64(1)) * G).sum(dtype=np.uint64)
    return int(h)


def test_cpp_example(rp, ctx, tmp_path):
    """host/example_knn_graph_sparse_metric.cpp evaluates every reported distance again on the host from
    dotS, and its checksums are those of the Python layer over the same rows and the same forest"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "example_knn_graph_sparse_metric")
    src = os.path.join(root, "rp-tree_amd", "host", "example_knn_graph_sparse_metric.cpp")
    lib = os.path.join(root, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src, "-L" + lib,
                           "-lrptree_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    n, d, T, minl, k, iters, r = 1000, 60, 3, 40, 8, 2, 8
    csr = mc.make_csr(2024, n, d, 0.2)                        # every row holds something: no NaN, whose payload is open
    assert np.diff(csr[0]).min() > 0
    rows = str(tmp_path / "rows.bin")
    with open(rows, "wb") as out:
        np.array([n, d], dtype=np.int64).tofile(out)
        csr[0].astype(np.int64).tofile(out)
        csr[1].astype(np.int32).tofile(out)
        csr[2].astype(np.float64).tofile(out)
    res = subprocess.run([exe, rows, str(T), str(minl), str(k), str(iters), str(r)], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == 3
    cfg = rp.rpTreeCfg(minl, n, d)
    f = rp.forestBatch(7, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, csr, ctx=ctx)
    for line, metric in zip(lines, METRICS):
        g = rp.knnGraphMetricSV(distf(rp, metric), k, f)
        refined = rp.knnGraphRefineMetricSV(distf(rp, metric), g, f, iters=iters, reverse=r)
        rounds, upd, cand = rp.knnGraphRefineLast(ctx)
        assert line == "%s rounds %d updates %d candidates %d checksum %016x %016x" % (
            metric, rounds, upd, cand, checksum(g), checksum(refined)), line
