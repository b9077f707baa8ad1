"""The search-graph preparation on SVector (CSR) rows under the cosine and inner-product distances on
the device (rpt_graph_prepare_csr_metric_host / _dev, graph_diversify_csr_kernel in
csrc/graph_prepare.hip): ids, counts, distance BITS and the three statistics, no tolerance anywhere,
against (a) the numpy restatement under dotS (tests/graph_metric_csr_ref.py) and (b)
rp.graphPrepare(metric=) on Dataset.dense of the dense-ified rows while every stored value is finite;
each again with no point resident in LDS (graph_prepare_csr_resident = -1) and under a small cap."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_metric_csr_ref as gm  # noqa: E402
import graph_prepare_ref as pref  # noqa: E402
import knn_graph_metric_ref as mref  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
NP = {"f64": np.float64, "f32": np.float32}
FLAGS = (0, 1, 2, 3)
OPTION = "graph_prepare_csr_resident"
METRICS = gm.METRICS


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


def distf_of(rp, metric):
    return {"cosine": rp.metricCosine, "inner": rp.metricInner, "l2": rp.metricL2}[metric]


@contextlib.contextmanager
def option(ctx, name, value):
    old = ctx.set_option(name, value)
    try:
        yield
    finally:
        ctx.set_option(name, old)


def build(rp, ctx, csr, minl, T, seed=1234):
    n, d = len(csr[0]) - 1, csr[3]
    cfg = rp.rpTreeCfg(minl, max(n, 2), d)
    return rp.forestBatch(seed, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, csr, ctx=ctx)


def prepare(rp, ctx, metric, graph, ds, kout, flags, resident=0):
    with option(ctx, OPTION, resident):
        got = rp.graphPrepareMetricSV(distf_of(rp, metric), graph, ds, kout=kout, diversify=bool(flags & 1),
                                      reverse=bool(flags & 2))
        return got, rp.graphPrepareLast(ctx)


def check_all(rp, ctx, metric, graph, ds, dense, D, kouts, tag, flags=FLAGS, residents=(0, -1)):
    """every flag value and every kout under every resident setting against (a) the restatement on D
    and, with `dense`, (b) the dense entry point under the same metric: bits and statistics"""
    for fl in flags:
        unions, (pairs, occluded) = pref.unions_of(graph, D, fl)
        for kout in kouts:
            want, capped = pref.cut_unions(unions, kout)
            for res in residents:
                got, stats = prepare(rp, ctx, metric, graph, ds, kout, fl, res)
                t = "%s %s flags %d kout %d resident %d" % (tag, metric, fl, kout, res)
                pref.assert_same_answer(got, want, t)
                assert stats == (pairs, occluded, capped), (t, stats)
            print("%s %s flags %d kout %d: pairs %d occluded %d capped %d" % (tag, metric, fl, kout, pairs, occluded,
                                                                               capped))
            if dense is not None:
                t = "%s %s flags %d kout %d, dense entry point" % (tag, metric, fl, kout)
                pref.assert_same_answer(rp.graphPrepare(graph, dense, kout=kout, diversify=bool(fl & 1),
                                                        reverse=bool(fl & 2), metric=distf_of(rp, metric)), want, t)
                assert rp.graphPrepareLast(ctx) == (pairs, occluded, capped), t


def neighbour_entries(csr, graph):
    """per point the entries its valid neighbours hold together: what the kernel compares with the cap"""
    lens = np.diff(csr[0])
    ids, _, cnt = graph
    return np.array([int(lens[ids[i, :cnt[i]]].sum()) for i in range(len(cnt))])


def dist_matrices(csr):
    """the pair distances under both metrics from one Gram matrix.  Every value here is finite, so the
    fold over the zero-filled rows is dotS bit for bit (tests/test_graph_metric_csr_host.py)"""
    G = mref.dot_matrix(gm.densify(csr))
    return {m: gm.mc.dist_matrix(m, G) for m in METRICS}


# ---------------------------------------------------------------- 1: the grid
_grid = {}


def grid_case(rp, ctx, dtype, d, density):
    """CSR rows, their forest, the pair distances and the dense twin; only the last key is kept"""
    key = (dtype, d, density)
    if key not in _grid:
        _grid.clear()
        n = 1500
        csr = gm.make_csr(d + int(100 * density), n, d, density, NP[dtype])
        f = build(rp, ctx, csr, 40, 3, seed=1234 + d)
        Ds = dist_matrices(csr)
        if d == 24:                                          # the shortcut of dist_matrices, held to dotS itself
            for m in METRICS:
                assert np.array_equal(gm.bits(Ds[m]), gm.bits(gm.rows_matrix(csr, m)))
        _grid[key] = (csr, f, Ds, rp.Dataset.dense(ctx, gm.densify(csr).astype(NP[dtype])))
    return _grid[key]


@pytest.mark.parametrize("k", [10, 64])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("density", [0.05, 0.3])
@pytest.mark.parametrize("d", [24, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_prepare_matches_the_definition(rp, ctx, dtype, d, density, metric, k):
    """k = 10 has one pair per lane, 64 has 32; d = 24 at density 0.05 leaves three rows in ten empty
    (cosine: NaN against everything, kept and never occluding); under a cap of 64 entries some points
    are resident and some are not"""
    csr, f, Ds, dense = grid_case(rp, ctx, dtype, d, density)
    assert f.data.is_csr
    graph = rp.knnGraphMetricSV(distf_of(rp, metric), k, f)
    kouts = sorted({k, min(64, 2 * k)})
    tag = "%s d %d density %g k %d" % (dtype, d, density, k)
    check_all(rp, ctx, metric, graph, f.data, dense, Ds[metric], kouts, tag, residents=(0, -1, 64))
    if k == 10 and (d, density) == (24, 0.3):
        tot = neighbour_entries(csr, graph)
        # the cap of 64 divides this set; the inner product prefers long rows, so fewer points lie below it
        few = 100 if metric == "cosine" else 0
        assert (tot <= 64).sum() > few and (tot > 64).sum() > few


# ---------------------------------------------------------------- 2: cap edges
@pytest.mark.parametrize("metric", METRICS)
def test_cap_edges(rp, ctx, metric):
    """d = 6 000, rows of 40 entries and: three points whose neighbours hold 1 535, 1 536 and 1 537
    entries together (the built-in cap is 1 536), a row of 5 000 entries among short neighbours, a
    point all of whose neighbours are empty rows"""
    d, n, k = 6000, 160, 8
    rng = np.random.default_rng(11)

    def row(m):
        return np.sort(rng.choice(d, size=m, replace=False)).astype(np.int32), rng.standard_normal(m)

    rows = [row(40) for _ in range(n)]
    for i, m in ((0, 512), (1, 512), (2, 512), (3, 511), (4, 513), (5, 5000), (6, 0), (7, 0), (8, 0), (9, 0)):
        rows[i] = row(m)
    rows[1] = (rows[0][0].copy(), rng.standard_normal(512))           # the support of row 0: every step folds
    csr = gm.from_rows(rows, d)
    members = {i: rng.choice(np.arange(10, n), k, replace=False).tolist() for i in range(n)}
    members.update({100: [0, 1, 3], 101: [0, 1, 2], 102: [0, 1, 4], 103: [5, 20, 21, 22, 23], 104: [6, 7, 8, 9],
                    105: [6, 0, 7, 30], 106: [5, 0, 1]})
    X = gm.densify(csr)
    G = mref.dot_matrix(X[:, np.any(X != 0, axis=0)])        # a column nobody stores adds +0.0: no bit changes
    D = gm.mc.dist_matrix(metric, G)
    graph = mref.hand_graph(D, k, members)
    tot = neighbour_entries(csr, graph)
    assert [int(tot[i]) for i in (100, 101, 102)] == [1535, 1536, 1537] and tot[103] == 5160 and tot[104] == 0
    if metric == "cosine":
        assert np.isnan(D[6]).all()
    ds = rp.Dataset.csr(ctx, *csr)
    check_all(rp, ctx, metric, graph, ds, rp.Dataset.dense(ctx, X), D, [4, 16], "cap edges", residents=(0, -1, 128))


@pytest.mark.parametrize("metric", METRICS)
def test_sixty_four_long_neighbours(rp, ctx, metric):
    """k = 64 over rows of 300 entries: 19 200 entries per point (no point is resident), 2 016 pairs,
    32 per lane"""
    n, d, k = 130, 2000, 64
    rng = np.random.default_rng(9)
    rows = [(np.sort(rng.choice(d, size=300, replace=False)).astype(np.int32), rng.standard_normal(300))
            for _ in range(n)]
    rows[5] = rows[77]
    csr = gm.from_rows(rows, d)
    D = dist_matrices(csr)[metric]
    graph = mref.exact_graph(D, k)
    assert neighbour_entries(csr, graph).min() == 19200
    check_all(rp, ctx, metric, graph, rp.Dataset.csr(ctx, *csr), rp.Dataset.dense(ctx, gm.densify(csr)), D, [64],
              "k 64 x 300", flags=(1, 3))


# ---------------------------------------------------------------- 3, 4: awkward values, the keep rule
def awkward_rows(d, dtype):
    """the awkward rows of test_gpu_knn_graph_csr.py (empty rows 3, 50, 51, 400, 599; 7 and 590 equal
    17; stored +0.0 and -0.0 in row 20; row 23 nothing but a stored -0.0) with an inf entry planted
    in row 40 and a NaN entry in row 41, both full rows"""
    from test_gpu_knn_graph_csr import awkward_rows as base
    csr, empty = base(d, dtype)
    rows = gm.rows_of(csr)
    full = np.arange(d, dtype=np.int32)
    rng = np.random.default_rng(100 + d)
    vi, vn = rng.standard_normal(d).astype(NP[dtype]), rng.standard_normal(d).astype(NP[dtype])
    vi[0], vn[d - 1] = np.inf, np.nan
    rows[40], rows[41] = (full, vi), (full, vn)
    return gm.from_rows(rows, d, NP[dtype]), len(rows)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("metric", METRICS)
def test_awkward_values_and_the_keep_rule(rp, ctx, metric, dtype):
    """held to the dotS restatement alone: with the stored inf the dense definition gives another
    graph, which the test asserts (in the restatement and of the dense entry point).  Under cosine:
    a NaN keeps, an equal distance keeps, duplicates of a kept neighbour go"""
    d, k = 33, 12
    csr, n = awkward_rows(d, dtype)
    rng = np.random.default_rng(d)
    special = ([3, 50, 51], [7, 17, 590], [40, 41, 20, 23], [11, 21, 22])
    members = {i: rng.choice(n, 6, replace=False).tolist() + special[i % 4] for i in range(n)}
    members[400] = [3, 50, 51, 599, 23]                      # an empty row lists rows without a nonzero
    members[17] = [7, 590, 100, 101]                         # duplicates of x_i itself
    D = gm.rows_matrix(csr, metric)
    graph = mref.hand_graph(D, k, members)
    ds = rp.Dataset.csr(ctx, *csr)
    check_all(rp, ctx, metric, graph, ds, None, D, [k, 24], "awkward %s" % dtype, residents=(0, -1, 16))
    # the case bites: the dense definition on the dense-ified rows keeps other entries
    Z = gm.dense_rows_matrix(csr, metric)
    assert not np.array_equal(gm.bits(Z), gm.bits(D))
    want, wst = pref.graph_prepare_ref(graph, D, k, 1)
    other, ost = pref.graph_prepare_ref(graph, Z, k, 1)
    assert not np.array_equal(want[0], other[0])
    dense = rp.Dataset.dense(ctx, gm.densify(csr).astype(NP[dtype]))
    twin = rp.graphPrepare(graph, dense, kout=k, diversify=True, reverse=False, metric=distf_of(rp, metric))
    pref.assert_same_answer(twin, other, "the dense entry point, on its own definition")
    if metric != "cosine":
        return
    (ids, dist, cnt), _ = prepare(rp, ctx, metric, graph, ds, k, 1)
    row = lambda i: ids[i, :cnt[i]].tolist()  # noqa: E731
    # rows without nonzeros are NaN against everything: nothing in row 400 is occluded
    assert sorted(row(400)) == [3, 23, 50, 51, 599] and np.isnan(dist[400, :5]).all()
    # 7 and 590 in row 17 are x_17 itself: dist(7, 590) has the bits of the distance stored with 590, and
    # an equal distance keeps
    assert gm.bits(D[7, 590]) == gm.bits(D[17, 590]) and 7 in row(17) and 590 in row(17)
    # i % 4 == 1 lists 7, 17 and 590, equal rows: whichever comes first stays or falls, the other two go
    dup_rows = [i for i in range(1, n, 4) if i not in (17, 41) and D[i, 7] > D[7, 17]]
    assert len(dup_rows) > 100 and all(17 not in row(i) and 590 not in row(i) for i in dup_rows)
    nan_rows = [i for i in range(2, n, 4) if i not in (40, 41)]
    assert all(41 in row(i) for i in nan_rows)               # a NaN distance is never occluded
    assert np.isnan(D[41]).all() and cnt[41] == graph[2][41]  # ... and row 41, NaN against all, occludes nothing


# ---------------------------------------------------------------- 5: repeat calls and entry points
@pytest.fixture(scope="module")
def plain_case(rp, ctx):
    n, d = 2500, 64
    csr = gm.make_csr(13, n, d, 0.2)
    return csr, build(rp, ctx, csr, 50, 3, seed=8)


@pytest.mark.parametrize("metric", METRICS)
def test_two_calls_and_the_dev_entry_point_give_the_same_bits(rp, ctx, plain_case, metric):
    import torch
    csr, f = plain_case
    n, d, k, kout = 2500, 64, 10, 16
    graph = rp.knnGraphMetricSV(distf_of(rp, metric), k, f)
    a, sa = prepare(rp, ctx, metric, graph, f.data, kout, 3)
    b, sb = prepare(rp, ctx, metric, graph, f.data, kout, 3)
    pref.assert_same_answer(a, b, "second call")
    assert sa == sb and sa[0] > 0
    dev = torch.device("cuda", ctx.device)
    tx = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in csr[:3]]
    dx = rp.Dataset.csr_from_torch(ctx, tx[0], tx[1], tx[2], d)
    ti, td, tc = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in graph)
    keep = (ti.clone(), td.clone(), tc.clone())
    oi = torch.empty((n, kout), dtype=torch.int32, device=dev)
    od = torch.empty((n, kout), dtype=torch.float64, device=dev)
    oc = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.graphPrepareMetricSVDev(distf_of(rp, metric), k, dx, ti.data_ptr(), td.data_ptr(), tc.data_ptr(), kout,
                               oi.data_ptr(), od.data_ptr(), oc.data_ptr(), diversify=True, reverse=True)
    ctx.sync()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((ti, td, tc), keep))
    pref.assert_same_answer((oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()), a, "dev against host")
    assert rp.graphPrepareLast(ctx) == sa


def test_metric_0_gives_the_bits_of_the_l2_entry_point(rp, ctx, plain_case):
    csr, f = plain_case
    graph = rp.knnGraphSV(10, f)
    for fl in (1, 3):
        want = rp.graphPrepareSV(graph, f.data, kout=16, diversify=bool(fl & 1), reverse=bool(fl & 2))
        stats = rp.graphPrepareLast(ctx)
        for distf in (None, rp.metricL2):
            for res in (0, -1):
                with option(ctx, OPTION, res):
                    got = rp.graphPrepareMetricSV(distf, graph, f.data, kout=16, diversify=bool(fl & 1),
                                                  reverse=bool(fl & 2))
                pref.assert_same_answer(got, want, "metric 0, flags %d resident %d" % (fl, res))
                assert rp.graphPrepareLast(ctx) == stats


# ---------------------------------------------------------------- 6: end to end
@pytest.mark.parametrize("metric", METRICS)
def test_search_on_a_prepared_graph(rp, ctx, metric):
    """knnGraphMetricSV -> knnGraphRefineMetricSV -> graphPrepareMetricSV -> graphSearchMetricSV with
    kg = kout: the search equals its restatement on the prepared graph, which equals the restatement
    of the preparation"""
    n, d, k, kout, nq = 2000, 32, 10, 16, 50
    distf = distf_of(rp, metric)
    fl = 3 if metric == "cosine" else 2                      # diversify assumes a metric; the inner product is none
    csr = gm.make_csr(21, n, d, 0.3, np.float32)
    f = build(rp, ctx, csr, 60, 2, seed=9)
    graph = rp.knnGraphRefineMetricSV(distf, rp.knnGraphMetricSV(distf, k, f), f, iters=1)
    sg, stats = prepare(rp, ctx, metric, graph, f.data, kout, fl)
    want, wst = pref.graph_prepare_ref(graph, dist_matrices(csr)[metric], kout, fl)
    pref.assert_same_answer(sg, want, "prepared")
    assert stats == wst
    rng = np.random.default_rng(8)
    rows = gm.rows_of(csr)
    csrQ = gm.from_rows([(rows[i][0], (rows[i][1] + 0.2 * rng.standard_normal(len(rows[i][1]))).astype(np.float32))
                         for i in rng.choice(n, nq)], d, np.float32)
    seeds = rng.integers(0, n, size=(nq, 4)).astype(np.int32)
    got = rp.graphSearchMetricSV(distf, sg, f.data, csrQ, 10, ef=32, seeds=seeds)
    model = gm.graph_search_ref(csr, csrQ, sg[0], sg[2], seeds, 10, 32, metric)
    gm.assert_same_answer(got, model[0], "search on the prepared graph")
    assert rp.graphSearchLast(ctx)[0] == model[1]


# ---------------------------------------------------------------- 7: refusals, degenerate sizes
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, k, kout = 1500, 16, 10, 12
    csr = gm.make_csr(12, n, d, 0.3)
    f = build(rp, ctx, csr, 30, 4, seed=7)
    ds = f.data
    graph = rp.knnGraphMetricSV(rp.metricCosine, k, f)
    good, stats = prepare(rp, ctx, "cosine", graph, ds, kout, 3)
    assert stats[0] > 0
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, data=ds, k_=k, kout_=kout, metric=COS, flags=3, gids=None, entry=None):
        gids = np.ascontiguousarray(graph[0] if gids is None else gids, dtype=np.int32)
        gdist = np.ascontiguousarray(graph[1])
        gcnt = np.ascontiguousarray(graph[2], dtype=np.int32)
        ids = np.full((n, 64), 12345, dtype=np.int32)
        dist = np.full((n, 64), 0.5)
        cnt = np.full(n, 77, dtype=np.int32)
        st = (entry or L.rpt_graph_prepare_csr_metric_host)(
            ctx._h, data._h, k_, C.c_void_p(gids.ctypes.data), C.c_void_p(gdist.ctypes.data),
            C.c_void_p(gcnt.ctypes.data), kout_, metric, flags, C.c_void_p(ids.ctypes.data),
            C.c_void_p(dist.ctypes.data), C.c_void_p(cnt.ctypes.data))
        assert st == code, (st, code)
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77)   # nothing was written
        assert rp.graphPrepareLast(ctx) == stats            # nothing was launched
        return msg

    for m in (COS | INN, REF, 2, INN | 1, -1):
        assert "metric" in refused(RPT_E_ARG, metric=m)
    for fl in (3 | COS, 3 | INN, 3 | REF, 4, -1):
        assert "flags" in refused(RPT_E_ARG, flags=fl)
    dense = rp.Dataset.dense(ctx, gm.densify(csr))
    for m in (0, COS, INN):
        assert "rpt_graph_prepare_*" in refused(RPT_E_ARG, data=dense, metric=m)     # names the dense entry point
    assert "k must" in refused(RPT_E_ARG, k_=65)
    assert "kout" in refused(RPT_E_ARG, kout_=0)
    bad = np.array(graph[0])
    bad[701, 0] = n
    assert graph[2][701] > 1 and "graph row 701: id" in refused(RPT_E_ARG, gids=bad)      # before any upload
    # the old entry points still refuse a metric, and say where it went
    for m in (COS, INN):
        msg = refused(RPT_E_UNSUPPORTED, metric=m, entry=L.rpt_graph_prepare_csr_host)
        assert "metric" in msg and "rpt_graph_prepare_csr_metric_*" in msg
        assert "rpt_graph_prepare_csr_metric_*" in refused(RPT_E_UNSUPPORTED, metric=m, entry=L.rpt_graph_prepare_host)
    with pytest.raises(rp.RPTError) as e:
        rp.graphPrepare(graph, ds, kout=kout, metric=rp.metricCosine)
    assert e.value.code == RPT_E_UNSUPPORTED and "rpt_graph_prepare_csr_metric_*" in str(e.value)
    with pytest.raises(ValueError):
        rp.graphPrepareMetricSV(rp.metricCosine, graph, ds, kout=65)
    with pytest.raises(NotImplementedError):
        rp.graphPrepareMetricSV(lambda u, v: 0.0, graph, ds)
    with pytest.raises(rp.RPTError) as e:
        rp.graphPrepareMetricSV(rp.metricInner, graph, dense)
    assert e.value.code == RPT_E_ARG
    again, st2 = prepare(rp, ctx, "cosine", graph, ds, kout, 3)
    pref.assert_same_answer(again, good, "after the refusals")
    assert st2 == stats
    assert rp.graphPrepareMetricSV(rp.metricCosine, graph, f)[0].shape == (n, 2 * k)


@pytest.mark.parametrize("metric", METRICS)
def test_no_points_and_one_point(rp, ctx, metric):
    d = 16
    csr = gm.make_csr(3, 20, d, 0.3)
    one = rp.Dataset.csr(ctx, *gm.from_rows(gm.rows_of(csr)[:1], d))
    g1 = (np.full((1, 3), -1, dtype=np.int32), np.full((1, 3), np.inf), np.zeros(1, dtype=np.int32))
    none = rp.Dataset.csr(ctx, *gm.from_rows([], d))
    g0 = (np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3)), np.zeros(0, dtype=np.int32))
    for fl in FLAGS:
        got, stats = prepare(rp, ctx, metric, g1, one, 2, fl)
        assert got[2].tolist() == [0] and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
        assert stats == (0, 0, 0)
        got, stats = prepare(rp, ctx, metric, g0, none, 5, fl)
        assert got[0].shape == (0, 5) and got[1].shape == (0, 5) and got[2].shape == (0,)
        assert stats == (0, 0, 0)
