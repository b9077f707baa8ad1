"""The kNN graph and its NN-descent rounds on SVector (CSR) rows on the device (rpt_knn_graph_csr_*,
rpt_knn_graph_refine_csr_*, csrc/graph_csr.hip): ids, counts and distance BITS, no tolerance
anywhere, against the dense definition on the dense-ified rows (tests/knn_graph_ref.py and
tests/knn_graph_refine_ref.py through tests/knn_graph_csr_ref.py) and against the dense entry
points on the dense-ified data set."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_csr_ref as cref  # noqa: E402
import knn_graph_refine_ref as rref  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
NP = {"f64": np.float64, "f32": np.float32}


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


def leaves_of(f):
    return cref.leaf_slices(f.topology())


def model_pairs(f, ordered=False):
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


def both_kernels(rp, ctx, f, k, want, tag):
    got = rp.knnGraphSV(k, f)
    cref.assert_same_graph(got, want, tag + ", leaf kernel")
    pairs = rp.knnGraphLastPairs(ctx)
    with option(ctx, "graph_general", 1):
        tiled = rp.knnGraphSV(k, f)
        assert rp.knnGraphLastPairs(ctx) == model_pairs(f, ordered=True)
    cref.assert_same_graph(tiled, want, tag + ", graph_general")
    return got, pairs


# ---------------------------------------------------------------- 1: the grid, both kernels
_grid = {}


def grid_case(rp, ctx, dtype, d, density):
    """one set, forest and reference (at k = 64; smaller k are its prefixes) per (dtype, d, density)"""
    key = (dtype, d, density)
    if key not in _grid:
        n, T, minl = 1500, 4 + (d % 5), 40
        csr = cref.make_csr(d + int(100 * density), n, d, density, NP[dtype])
        f = build(rp, ctx, csr, minl, T, seed=1234 + d)
        X64 = cref.densify(csr)
        _grid[key] = (csr, f, X64, cref.knn_graph_ref(X64, f.perm, leaves_of(f), 64))
    return _grid[key]


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("density", [0.05, 0.3])
@pytest.mark.parametrize("d", [24, 70, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_graph_matches_the_dense_definition(rp, ctx, dtype, d, density, k):
    csr, f, X64, want64 = grid_case(rp, ctx, dtype, d, density)
    assert f.data.is_csr and 4 <= f.T <= 8
    got, pairs = both_kernels(rp, ctx, f, k, cut(want64, k), "%s d %d density %g k %d" % (dtype, d, density, k))
    assert max(s for _, s in leaves_of(f)) <= 128 and pairs == model_pairs(f)
    assert not (got[0] == np.arange(f.N, dtype=np.int32)[:, None]).any()   # no row lists itself


# ---------------------------------------------------------------- 2: awkward rows in one set
def awkward_rows(d, dtype):
    n = 600
    rows = [(c.copy(), v.copy()) for c, v in cref.rows_of(cref.make_csr(7 + d, n, d, 0.3, NP[dtype]))]
    rng = np.random.default_rng(d)
    none = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=NP[dtype]))
    empty = [3, 50, 51, 400, 599]
    for e in empty:
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
    rows[23] = (np.array([0], dtype=np.int32), np.array([-0.0], dtype=NP[dtype]))         # nothing but a stored zero
    rows[21] = (np.array([0], dtype=np.int32), np.array([1.5], dtype=NP[dtype]))          # only column 0
    rows[22] = (np.array([d - 1], dtype=np.int32), np.array([-2.5], dtype=NP[dtype]))     # only column d - 1
    for i in range(60, 70):                                  # rows x 10
        rows[i] = (rows[i][0], rows[i][1] * NP[dtype](10))
    return cref.from_rows(rows, d, NP[dtype]), empty


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("d", [33, 32, 1])
def test_awkward_rows(rp, ctx, d, dtype):
    csr, empty = awkward_rows(d, dtype)
    X64 = cref.densify(csr)
    f = build(rp, ctx, csr, 30, 4, seed=5 + d)
    for k in (10, 64):
        want = cref.knn_graph_ref(X64, f.perm, leaves_of(f), k)
        both_kernels(rp, ctx, f, k, want, "awkward d %d k %d" % (d, k))
    # all pairs (depth 0): rows without nonzeros, and the row of one stored zero, are at distance 0
    # from each other and come first, by id
    f0 = build(rp, ctx, csr, 30, 1, maxd=0)
    got = rp.knnGraphSV(10, f0)
    cref.assert_same_graph(got, cref.knn_graph_ref(X64, f0.perm, leaves_of(f0), 10), "awkward, all pairs")
    if d > 1:
        zero = sorted(empty + [23])
        for e in zero:
            others = [z for z in zero if z != e]
            assert got[0][e, :len(others)].tolist() == others and np.all(got[1][e, :len(others)] == 0.0)


# ---------------------------------------------------------------- 3: wide and empty
def test_wide_rows_with_mostly_empty_windows(rp, ctx):
    n, d, nnz, k = 400, 20000, 12, 10
    rng = np.random.default_rng(3)
    centres = np.array([40, 5000, 5100, 12345, d - 40])
    rows = []
    for i in range(n):
        c = rng.choice(centres, size=3, replace=False)
        cols = np.unique(np.clip(np.concatenate([cc + rng.integers(-40, 40, size=nnz) for cc in c]), 0, d - 1))
        cols = np.sort(rng.choice(cols, size=nnz, replace=False)).astype(np.int32)
        rows.append((cols, rng.standard_normal(nnz)))
    rows[123] = (np.concatenate([rows[123][0][:-1], [d - 1]]).astype(np.int32), rows[123][1])
    assert np.all(np.diff(rows[123][0]) > 0)
    csr = cref.from_rows(rows, d)
    windows = {int(c) // 32 for c in csr[1]}
    assert len(windows) * 8 < d // 32                       # most 32-column windows hold nothing
    f = build(rp, ctx, csr, 12, 2, seed=9)             # small leaves: the dense reference folds 20 000 columns per pair
    want = cref.knn_graph_ref(cref.densify(csr), f.perm, leaves_of(f), k)
    both_kernels(rp, ctx, f, k, want, "wide")


# ---------------------------------------------------------------- 4: leaf sizes and tiny inputs
@pytest.mark.parametrize("n,minl,maxd,k", [(3000, 100, 5, 10), (3000, 100, 5, 64), (130, 10, 1, 64),
                                           (1, 1, 3, 4), (2, 1, 3, 4)])
def test_leaf_sizes_and_padding(rp, ctx, n, minl, maxd, k):
    csr = cref.make_csr(n, n, 40, 0.2)
    f = build(rp, ctx, csr, minl, 3, seed=77, maxd=maxd)
    want = cref.knn_graph_ref(cref.densify(csr), f.perm, leaves_of(f), k)
    got = rp.knnGraphSV(k, f)
    cref.assert_same_graph(got, want, "n %d" % n)
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][pad] == -1) and np.all(np.isposinf(got[1][pad]))
    with option(ctx, "graph_general", 1):
        cref.assert_same_graph(rp.knnGraphSV(k, f), want, "n %d tiled" % n)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_depth_zero_is_all_pairs(rp, ctx, dtype):
    """maxDepth 0: one leaf, every pair.  Only here, where nothing is projected, a NaN and an inf:
    NaN both ways, last, by id"""
    n, d, k = 300, 40, 10
    rows = cref.rows_of(cref.make_csr(3, n, d, 0.2, NP[dtype], empty=(9, 10)))
    rows[44] = (rows[44][0], rows[44][1].copy())
    assert len(rows[44][0]) > 1 and len(rows[70][0]) > 0
    rows[44][1][1] = np.nan
    rows[70] = (rows[70][0], rows[70][1].copy())
    rows[70][1][0] = np.inf
    csr = cref.from_rows(rows, d, NP[dtype])
    X64 = cref.densify(csr)
    f = build(rp, ctx, csr, 10, 2, maxd=0)
    assert leaves_of(f) == [(0, n)]
    want = cref.knn_graph_ref(X64, f.perm, leaves_of(f), k)
    got = rp.knnGraphSV(k, f)                               # 300 > 128 points: the tiled kernel
    cref.assert_same_graph(got, want, "depth 0")
    assert np.all(np.isnan(got[1][44])) and got[0][44].tolist() == list(range(k))
    assert np.all(np.isposinf(got[1][70][:got[2][70]]))
    cref.assert_same_graph(rp.knnGraphSV(64, f), cref.knn_graph_ref(X64, f.perm, leaves_of(f), 64), "depth 0, k 64")
    small = cref.from_rows(rows[20:80], d, NP[dtype])       # 60 rows, the NaN row is 24, the inf row 50
    S64 = cref.densify(small)
    f2 = build(rp, ctx, small, 10, 1, maxd=0)
    g2 = rp.knnGraphSV(59, f2)                              # 60 points: the leaf kernel; k = n - 1
    cref.assert_same_graph(g2, cref.knn_graph_ref(S64, f2.perm, leaves_of(f2), 59), "depth 0, leaf kernel")
    others = [i for i in range(60) if i != 24]
    assert np.all(g2[0][others, -1] == 24) and np.all(np.isnan(g2[1][others, -1]))


# ---------------------------------------------------------------- 5: the dense kernels as a witness
@pytest.mark.parametrize("dtype,density", [("f64", 0.05), ("f32", 0.3)])
def test_dense_entry_point_on_the_densified_rows_gives_the_same(rp, ctx, dtype, density):
    csr, f, X64, _ = grid_case(rp, ctx, dtype, 70, density)
    dense = rp.importForest(ctx, X64.astype(NP[dtype]), f.R, f.min_leaf, f.perm, f.thr, f.mglo, f.mghi, mode=f.mode)
    assert not dense.data.is_csr
    for k in (10, 64):
        cref.assert_same_graph(rp.knnGraphSV(k, f), rp.knnGraph(k, dense), "witness k %d" % k)


# ---------------------------------------------------------------- 6: accumulate
@pytest.mark.parametrize("dtype,k", [("f64", 10), ("f32", 64)])
def test_accumulate_folds_tree_shards_in_any_order(rp, ctx, dtype, k):
    n, d, T, minl = 1500, 70, 5, 40
    csr = cref.make_csr(21, n, d, 0.3, NP[dtype])
    X64 = cref.densify(csr)
    cfg = rp.rpTreeCfg(minl, n, d)
    _, R = rp.gen.forest_hyperplanes(99, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    whole, fa, fb = (build(rp, ctx, csr, minl, len(r), seed=0, hyperplanes=r) for r in (R, R[:2], R[2:]))
    assert np.array_equal(whole.perm, np.concatenate([fa.perm, fb.perm]))
    g = rp.knnGraphSV(k, whole)
    cref.assert_same_graph(g, cref.knn_graph_ref(X64, whole.perm, leaves_of(whole), k), "whole")
    cref.assert_same_graph(rp.knnGraphSV(k, fb, accumulate=rp.knnGraphSV(k, fa)), g, "a then b")
    cref.assert_same_graph(rp.knnGraphSV(k, fa, accumulate=rp.knnGraphSV(k, fb)), g, "b then a")
    with option(ctx, "graph_general", 1):
        cref.assert_same_graph(rp.knnGraphSV(k, fb, accumulate=rp.knnGraphSV(k, fa)), g, "a then b, tiled")


# ---------------------------------------------------------------- 7: refinement
_steps = {}


def refine_steps(key, X64, g0, k, r, iters):
    """the reference after `iters` rounds, taken one round at a time and kept: (graph, rounds,
    updates, candidates)"""
    st = _steps.setdefault(key, {"D": None, "seq": [], "ended": False})
    if st["D"] is None:
        st["D"] = rref.fold_matrix(X64)
    seq = st["seq"]
    while len(seq) < iters and not st["ended"]:
        g, rounds, upd, cand = seq[-1] if seq else (g0, 0, 0, 0)
        new, one, u, c = rref.refine_ref(X64, g, k, r, 1, st["D"])
        seq.append((new, rounds + one, upd + u, cand + c))
        st["ended"] = u == 0
    return seq[min(iters, len(seq)) - 1]


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("k", [5, 10])
@pytest.mark.parametrize("density", [0.05, 0.3])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refine_matches_the_dense_definition(rp, ctx, dtype, density, k, iters):
    csr, f, X64, want64 = grid_case(rp, ctx, dtype, 70, density)
    g0 = cut(want64, k)
    want, rounds, upd, cand = refine_steps((dtype, density, k), X64, g0, k, k, iters)
    got = rp.knnGraphRefineSV(g0, f, iters=iters, reverse=k)
    stats = rp.knnGraphRefineLast(ctx)
    cref.assert_same_graph(got, want, "refine")
    assert stats == (rounds, upd, cand)
    # the dense entry point on the dense-ified data set: the same bits and the same three numbers
    dense = rp.Dataset.dense(ctx, X64.astype(NP[dtype]))
    cref.assert_same_graph(rp.knnGraphRefine(g0, dense, iters=iters, reverse=k), got, "dense refine")
    assert rp.knnGraphRefineLast(ctx) == stats
    with option(ctx, "graph_refine_general", 1):
        cref.assert_same_graph(rp.knnGraphRefineSV(g0, f.data, iters=iters, reverse=k), got, "graph_refine_general")
        assert rp.knnGraphRefineLast(ctx) == stats


def block_graph(X64, size, k):
    """a start graph that needs no forest: two "trees" whose leaves are blocks of `size` ids, in id
    order and in a shuffled order"""
    n = X64.shape[0]
    perm = np.stack([np.arange(n), np.random.default_rng(n).permutation(n)]).astype(np.int32)
    return cref.knn_graph_ref(X64, perm, [(o, min(size, n - o)) for o in range(0, n, size)], k)


def test_refine_to_the_fixed_point_and_twice_the_same_bits(rp, ctx):
    n, d, k = 300, 30, 6
    csr = cref.make_csr(8, n, d, 0.25)
    X64 = cref.densify(csr)
    ds = rp.Dataset.csr(ctx, *csr)
    g0 = block_graph(X64, 20, k)
    want, rounds, upd, cand = rref.refine_ref(X64, g0, k, 4, 50)
    assert 1 < rounds < 50
    got = rp.knnGraphRefineSV(g0, ds, iters=50, reverse=4)
    assert rp.knnGraphRefineLast(ctx) == (rounds, upd, cand)
    cref.assert_same_graph(got, want, "fixed point")
    again = rp.knnGraphRefineSV(g0, ds, iters=50, reverse=4)
    cref.assert_same_graph(again, got, "two calls")
    same = rp.knnGraphRefineSV(got, ds, iters=3, reverse=4)  # a fixed point: one round, nothing new
    assert rp.knnGraphRefineLast(ctx)[:2] == (1, 0)
    cref.assert_same_graph(same, got, "at the fixed point")
    # k = reverse = 64: the candidate set of a point takes a workgroup's whole LDS share
    wide = block_graph(X64, 100, 64)
    w_want, w_rounds, w_upd, w_cand = rref.refine_ref(X64, wide, 64, 64, 1)
    cref.assert_same_graph(rp.knnGraphRefineSV(wide, ds, iters=1, reverse=64), w_want, "k 64")
    assert rp.knnGraphRefineLast(ctx) == (w_rounds, w_upd, w_cand)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refine_awkward_rows(rp, ctx, dtype):
    """empty rows, duplicates, a full row, stored zeros; rows longer than one staged piece of x_i"""
    csr, _ = awkward_rows(33, dtype)
    rows = cref.rows_of(csr)
    rng = np.random.default_rng(1)
    wide_d = 400
    for i in (11, 100, 101):                                # 150 .. 400 nonzeros: several pieces of 64
        cols = np.sort(rng.choice(wide_d, size=150 if i > 11 else wide_d, replace=False)).astype(np.int32)
        rows[i] = (cols, rng.standard_normal(len(cols)).astype(NP[dtype]))
    csr = cref.from_rows(rows, wide_d, NP[dtype])
    X64 = cref.densify(csr)
    f = build(rp, ctx, csr, 30, 3, seed=2)
    k = 8
    g0 = rp.knnGraphSV(k, f)
    cref.assert_same_graph(g0, cref.knn_graph_ref(X64, f.perm, leaves_of(f), k), "awkward graph")
    for iters, r in ((1, 8), (2, 0)):
        want, rounds, upd, cand = rref.refine_ref(X64, g0, k, r, iters)
        cref.assert_same_graph(rp.knnGraphRefineSV(g0, f, iters=iters, reverse=r), want, "awkward refine")
        assert rp.knnGraphRefineLast(ctx) == (rounds, upd, cand)


@pytest.mark.parametrize("n", [1, 2])
def test_refine_tiny_data_sets(rp, ctx, n):
    csr = cref.from_rows([(np.array([1], dtype=np.int32), np.array([float(i + 1)])) for i in range(n)], 4)
    ds = rp.Dataset.csr(ctx, *csr)
    k = 3
    ids = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), np.inf)
    cnt = np.zeros(n, dtype=np.int32)
    if n == 2:
        ids[0, 0], dist[0, 0], cnt[0] = 1, 1.0, 1
    got = rp.knnGraphRefineSV((ids, dist, cnt), ds, iters=2)
    want, rounds, upd, cand = rref.refine_ref(cref.densify(csr), (ids, dist, cnt), k, k, 2)
    cref.assert_same_graph(got, want, "tiny")
    assert rp.knnGraphRefineLast(ctx) == (rounds, upd, cand)


# ---------------------------------------------------------------- 8: errors and side effects
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, T, minl, k = 1500, 16, 4, 30, 10
    csr = cref.make_csr(12, n, d, 0.3)
    X64 = cref.densify(csr)
    ds = rp.Dataset.csr(ctx, *csr)
    cfg = rp.rpTreeCfg(minl, n, d)
    _, R = rp.gen.forest_hyperplanes(7, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    f = rp.forestBatch(0, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx, hyperplanes=R)
    ids = np.empty((n, 64), dtype=np.int32)
    dist = np.empty((n, 64), dtype=np.float64)
    cnt = np.empty(n, dtype=np.int32)
    ptrs = lambda g: [C.c_void_p(a.ctypes.data) for a in g]  # noqa: E731

    def refused(code, forest, data, kk, flags):
        assert L.rpt_knn_graph_csr_host(ctx._h, forest._h, data._h, kk, flags, *ptrs((ids, dist, cnt))) == code
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        return msg

    Q = cref.make_csr(1, 64, d, 0.3)
    before = rp.knnBatch(k, f, Q)
    tier = C.c_int32(-1)
    _lib.check(L.rpt_knn_last_tier(ctx._h, C.byref(tier)))
    tier_before = tier.value

    dense = rp.Dataset.dense(ctx, X64)
    assert "rpt_knn_graph_*" in refused(RPT_E_ARG, f, dense, k, 0)          # names the dense entry point
    for kk in (0, 65, -3):
        assert "k" in refused(RPT_E_ARG, f, ds, kk, 0)
    short = cref.from_rows(cref.rows_of(csr)[:-1], d)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.csr(ctx, *short), k, 0)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.csr(ctx, csr[0], csr[1], csr[2], d + 1), k, 0)
    assert "data set" in refused(RPT_E_ARG, f, rp.Dataset.csr(ctx, csr[0], csr[1], csr[2].astype(np.float32), d), k, 0)
    refused(RPT_E_ARG, f, ds, k, 2)
    for flag in (rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE,
                 rp.RPT_KNN_METRIC_COSINE | 1):
        assert "metric" in refused(RPT_E_UNSUPPORTED, f, ds, k, flag)
    fs = rp.forest(0, cfg.fpMaxTreeDepth, minl, T, 500, cfg.fpProjNzDensity, d, ds, ctx=ctx, hyperplanes=R)
    assert "streamed" in refused(RPT_E_UNSUPPORTED, fs, ds, k, 0)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphSV(65, f)
    assert e.value.code == RPT_E_ARG

    # the refinement
    g0 = rp.knnGraphSV(k, f)
    cref.assert_same_graph(g0, cref.knn_graph_ref(X64, f.perm, leaves_of(f), k), "after the refusals")

    def rrefused(code, data, kk, r, iters, flags, graph):
        assert L.rpt_knn_graph_refine_csr_host(ctx._h, data._h, kk, r, iters, flags, *ptrs(graph)) == code
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        return msg

    work = lambda: tuple(a.copy() for a in g0)  # noqa: E731
    assert "rpt_knn_graph_refine_*" in rrefused(RPT_E_ARG, dense, k, k, 1, 0, work())
    assert "k" in rrefused(RPT_E_ARG, ds, 0, k, 1, 0, work())
    assert "k" in rrefused(RPT_E_ARG, ds, 65, k, 1, 0, work())
    assert "reverse" in rrefused(RPT_E_ARG, ds, k, 65, 1, 0, work())
    assert "iters" in rrefused(RPT_E_ARG, ds, k, k, 0, 0, work())
    rrefused(RPT_E_ARG, ds, k, k, 1, 1, work())
    for flag in (rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE):
        assert "metric" in rrefused(RPT_E_UNSUPPORTED, ds, k, k, 1, flag, work())
    bad = work()
    bad[0][703, 1] = bad[0][703, 0]
    assert "row 703" in rrefused(RPT_E_ARG, ds, k, k, 1, 0, bad)
    bad = work()
    bad[0][12, 0] = n
    assert "row 12" in rrefused(RPT_E_ARG, ds, k, k, 1, 0, bad)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphRefineSV(g0, ds, iters=0)
    assert e.value.code == RPT_E_ARG
    # the dense entry points keep refusing CSR rows
    assert L.rpt_knn_graph_host(ctx._h, f._h, ds._h, k, 0, *ptrs((ids, dist, cnt))) == RPT_E_UNSUPPORTED
    assert L.rpt_knn_graph_refine_host(ctx._h, ds._h, k, k, 1, 0, *ptrs(work())) == RPT_E_UNSUPPORTED

    # a knnBatch on the same context answers as before, and the ranking tier is untouched
    rp.knnGraphRefineSV(g0, ds, iters=1)
    after = rp.knnBatch(k, f, Q)
    _lib.check(L.rpt_knn_last_tier(ctx._h, C.byref(tier)))
    assert tier.value == tier_before
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------- device arrays
def test_dev_entry_points_with_torch_tensors(rp, ctx):
    import torch
    csr, f, X64, want64 = grid_case(rp, ctx, "f64", 70, 0.3)
    n, k = f.N, 10
    dev = torch.device("cuda", ctx.device)
    ids = torch.full((n, k), 7, dtype=torch.int32, device=dev)
    dist = torch.zeros((n, k), dtype=torch.float64, device=dev)
    cnt = torch.full((n,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.knnGraphSVDev(k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    ctx.sync()
    assert rp.knnGraphLastPairs(ctx) == model_pairs(f)
    g0 = cut(want64, k)
    cref.assert_same_graph((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), g0, "dev")
    rp.knnGraphSVDev(k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), accumulate=True)
    rp.knnGraphRefineSVDev(k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), iters=3)
    ctx.sync()
    want = rp.knnGraphRefineSV(g0, f, iters=3)
    cref.assert_same_graph((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), want, "dev refine")


def test_prof_class_3_times_both(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    csr, f, _, _ = grid_case(rp, ctx, "f64", 24, 0.3)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        _lib.check(L.rpt_prof_reset(ctx._h))
        g = rp.knnGraphSV(5, f)
        rp.knnGraphRefineSV(g, f)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
        assert cnt.value == 2 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_example(tmp_path):
    """host/example_knn_graph_sparse.cpp folds every reported distance again on the host over the
    union of the two supports and compares the bits"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "example_knn_graph_sparse")
    src = os.path.join(root, "rp-tree_amd", "host", "example_knn_graph_sparse.cpp")
    lib = os.path.join(root, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "1200", "60", "0.2", "3", "40", "8", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[-2].startswith("rounds 2 updates ")
