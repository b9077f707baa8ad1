"""The search-graph preparation on SVector (CSR) rows on the device (rpt_graph_prepare_csr_host / _dev,
graph_diversify_csr_kernel in csrc/graph_prepare.hip): ids, counts, distance BITS and the three
statistics, no tolerance anywhere, against (a) the numpy restatement on the dense-ified rows
(tests/graph_prepare_ref.py) and (b) rp.graphPrepare on Dataset.dense of the dense-ified rows; where
named again with no point resident in LDS (graph_prepare_csr_resident = -1) and under a small cap."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_csr_ref as cref  # noqa: E402
import knn_graph_metric_ref as mref  # noqa: E402
import graph_prepare_ref as pref  # noqa: E402
import graph_search_csr_ref as scref  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
NP = {"f64": np.float64, "f32": np.float32}
FLAGS = (0, 1, 2, 3)
OPTION = "graph_prepare_csr_resident"


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


def build(rp, ctx, csr, minl, T, seed=1234):
    n, d = len(csr[0]) - 1, csr[3]
    cfg = rp.rpTreeCfg(minl, max(n, 2), d)
    return rp.forestBatch(seed, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, csr, ctx=ctx)


def prepare(rp, ctx, graph, ds, kout, flags, resident=0):
    with option(ctx, OPTION, resident):
        got = rp.graphPrepareSV(graph, ds, kout=kout, diversify=bool(flags & 1), reverse=bool(flags & 2))
        return got, rp.graphPrepareLast(ctx)


def check_all(rp, ctx, graph, ds, dense, D, kouts, tag, flags=FLAGS, residents=(0, -1)):
    """every flag value and every kout under every resident setting against (a) the restatement on D,
    the pair distances of the dense-ified rows, and (b) the dense entry point: bits and statistics"""
    for fl in flags:
        unions, (pairs, occluded) = pref.unions_of(graph, D, fl)
        for kout in kouts:
            want, capped = pref.cut_unions(unions, kout)
            for res in residents:
                got, stats = prepare(rp, ctx, graph, ds, kout, fl, res)
                t = "%s flags %d kout %d resident %d" % (tag, fl, kout, res)
                pref.assert_same_answer(got, want, t)
                assert stats == (pairs, occluded, capped), (t, stats)
            print("%s flags %d kout %d: pairs %d occluded %d capped %d" % (tag, fl, kout, pairs, occluded, capped))
            if dense is not None:
                t = "%s flags %d kout %d, dense entry point" % (tag, fl, kout)
                pref.assert_same_answer(rp.graphPrepare(graph, dense, kout=kout, diversify=bool(fl & 1),
                                                        reverse=bool(fl & 2)), want, t)
                assert rp.graphPrepareLast(ctx) == (pairs, occluded, capped), t


def neighbour_entries(csr, graph):
    """per point the entries its valid neighbours hold together: what the kernel compares with the cap"""
    lens = np.diff(csr[0])
    ids, _, cnt = graph
    return np.array([int(lens[ids[i, :cnt[i]]].sum()) for i in range(len(cnt))])


# ---------------------------------------------------------------- 1: the grid
_grid = {}


def grid_case(rp, ctx, dtype, d, density):
    """CSR rows, their forest, the pair distances and the dense twin; only the last key is kept"""
    key = (dtype, d, density)
    if key not in _grid:
        _grid.clear()
        n = 1500
        csr = cref.make_csr(d + int(100 * density), n, d, density, NP[dtype])
        f = build(rp, ctx, csr, 40, 3, seed=1234 + d)
        X64 = cref.densify(csr)
        _grid[key] = (csr, f, mref.metric_matrix(X64, "l2"), rp.Dataset.dense(ctx, X64.astype(NP[dtype])))
    return _grid[key]


@pytest.mark.parametrize("k", [1, 2, 10, 11, 12, 64])
@pytest.mark.parametrize("density", [0.05, 0.3])
@pytest.mark.parametrize("d", [24, 70, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_prepare_matches_the_dense_definition(rp, ctx, dtype, d, density, k):
    """k = 11 is the last with one pair per lane, 12 the first with two, 64 has 32; under a cap of 64
    entries some points are resident and some are not"""
    csr, f, D, dense = grid_case(rp, ctx, dtype, d, density)
    assert f.data.is_csr
    graph = rp.knnGraphSV(k, f)
    kouts = sorted({1, k, min(64, 2 * k), 64})
    tag = "%s d %d density %g k %d" % (dtype, d, density, k)
    check_all(rp, ctx, graph, f.data, dense, D, kouts, tag, residents=(0, -1, 64))
    if k == 10:
        if (d, density) == (24, 0.3):
            tot = neighbour_entries(csr, graph)
            assert (tot <= 64).sum() > 100 and (tot > 64).sum() > 100     # the cap of 64 divides this set
        # flags 0, kout = k: the input bit for bit; DIVERSIFY's output is a valid input again; with
        # REVERSE and a kout that cuts nothing the graph is symmetric
        same, _ = prepare(rp, ctx, graph, f.data, k, 0)
        pref.assert_same_answer(same, graph, "identity")
        once, _ = prepare(rp, ctx, graph, f.data, k, 1)
        twice, st = prepare(rp, ctx, once, f.data, k, 1)
        want, wst = pref.graph_prepare_ref(once, D, k, 1)
        pref.assert_same_answer(twice, want, "second pass")
        assert st == wst
        sym, st = prepare(rp, ctx, graph, f.data, 64, 3)
        if st[2] == 0:
            rows = [set(sym[0][i, :sym[2][i]].tolist()) for i in range(len(sym[2]))]
            assert all(i in rows[j] for i in range(len(rows)) for j in rows[i])


# ---------------------------------------------------------------- 2: cap and length edges
NNZ = (0, 1, 63, 64, 65, 127, 128, 129, 300)


def test_cap_and_length_edges(rp, ctx):
    """d = 300, rows of 0, 1, 63, 64, 65, 127, 128, 129 and 300 nonzeros (row i holds NNZ[i % 9]), a
    hand-made graph, a cap of 128 entries: graph rows whose neighbours total 127, 128 and 129 entries,
    and pairs whose supports are identical, wholly below / above each other and interleaved without
    meeting, each once under the cap (two neighbours) and once above it (all six in one row)"""
    d, n, k = 300, 300, 8
    rng = np.random.default_rng(1)
    rows = []
    for i in range(n):
        m = NNZ[i % len(NNZ)]
        rows.append((np.sort(rng.choice(d, size=m, replace=False)).astype(np.int32), rng.standard_normal(m)))
    block = lambda lo: np.arange(lo, lo + 64, dtype=np.int32)  # noqa: E731
    rows[3] = (block(0), rng.standard_normal(64))            # wholly below 12
    rows[12] = (block(236), rng.standard_normal(64))
    rows[21] = (block(100), rng.standard_normal(64))         # the support of 39
    rows[39] = (block(100), rng.standard_normal(64))
    rows[30] = (np.arange(101, 229, 2, dtype=np.int32), rng.standard_normal(64))   # interleaved with 48, disjoint
    rows[48] = (np.arange(100, 228, 2, dtype=np.int32), rng.standard_normal(64))
    csr = cref.from_rows(rows, d)
    lens = np.diff(csr[0])
    assert sorted(set(lens.tolist())) == sorted(NNZ)
    members = {i: rng.choice(n, k, replace=False).tolist() for i in range(n)}
    # ids by nonzeros: 0 -> 0, 1 -> 1, 2 -> 63, 4 -> 65, 5 -> 127, 6 -> 128, 57 -> 64
    members.update({100: [5, 0], 101: [5, 1], 102: [6, 1], 103: [2, 57], 104: [57, 66], 105: [4, 57],
                    106: [2, 57, 1], 107: [2, 4, 10], 110: [21, 39], 111: [3, 12], 112: [30, 48],
                    113: [3, 12, 21, 39, 30, 48], 114: [8, 17], 115: [8, 0]})
    D = mref.metric_matrix(cref.densify(csr), "l2")
    graph = mref.hand_graph(D, k, members)
    tot = neighbour_entries(csr, graph)
    assert [int(tot[i]) for i in (100, 101, 102, 103, 104, 105, 106, 107)] == [127, 128, 129, 127, 128, 129, 128, 129]
    assert tot[110] == tot[111] == tot[112] == 128 and tot[113] == 384 and tot[114] == 600
    ds = rp.Dataset.csr(ctx, *csr)
    dense = rp.Dataset.dense(ctx, cref.densify(csr))
    check_all(rp, ctx, graph, ds, dense, D, [4, 16], "edges", residents=(0, -1, 128))


# ---------------------------------------------------------------- 3: awkward values
def awkward_rows(d, dtype):
    """the awkward rows of test_gpu_knn_graph_csr.py (empty rows 3, 50, 51, 400, 599; 7 and 590 equal
    17; stored +0.0 and -0.0 in row 20; row 23 nothing but a stored -0.0) with an inf entry planted
    in row 40 and a NaN entry in row 41"""
    from test_gpu_knn_graph_csr import awkward_rows as base
    csr, empty = base(d, dtype)
    rows = cref.rows_of(csr)
    full = np.arange(d, dtype=np.int32)
    rng = np.random.default_rng(100 + d)
    vi, vn = rng.standard_normal(d).astype(NP[dtype]), rng.standard_normal(d).astype(NP[dtype])
    vi[0], vn[d - 1] = np.inf, np.nan
    rows[40], rows[41] = (full, vi), (full, vn)
    return cref.from_rows(rows, d, NP[dtype]), len(rows)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("d", [33, 32, 1])
def test_awkward_values(rp, ctx, d, dtype):
    csr, n = awkward_rows(d, dtype)
    k = 12
    rng = np.random.default_rng(d)
    special = ([3, 50, 51], [7, 17, 590], [40, 41, 20, 23], [11, 21, 22])
    members = {i: rng.choice(n, 6, replace=False).tolist() + special[i % 4] for i in range(n)}
    members[400] = [3, 50, 51, 599, 23]                      # an empty row lists rows without a nonzero
    members[17] = [7, 590, 100, 101]                         # duplicates of x_i itself
    D = mref.metric_matrix(cref.densify(csr), "l2")
    graph = mref.hand_graph(D, k, members)
    ds = rp.Dataset.csr(ctx, *csr)
    dense = rp.Dataset.dense(ctx, cref.densify(csr).astype(NP[dtype]))
    check_all(rp, ctx, graph, ds, dense, D, [k, 24], "awkward d %d %s" % (d, dtype), residents=(0, -1, 16))
    (ids, dist, cnt), _ = prepare(rp, ctx, graph, ds, k, 1)
    row = lambda i: ids[i, :cnt[i]].tolist()  # noqa: E731
    # two rows without nonzeros are at distance 0, and 0 < 0 is false: nothing in row 400 is occluded
    assert sorted(row(400)) == [3, 23, 50, 51, 599] and np.all(dist[400, :5] == 0.0)
    assert 7 in row(17) and 590 in row(17)                   # duplicates of x_17 itself: nothing is below 0
    # i % 4 == 1 lists 7, 17 and 590, equal rows: whatever keeps or occludes 7 occludes the other two
    dup_rows = [i for i in range(1, n, 4) if i not in (17, 41) and D[i, 7] > 0]
    assert (len(dup_rows) > 100 or d == 1) and all(17 not in row(i) and 590 not in row(i) for i in dup_rows)
    nan_rows = [i for i in range(2, n, 4) if i not in (40, 41)]
    assert all(41 in row(i) for i in nan_rows)               # a NaN distance is never occluded
    assert np.isnan(D[41, 40]) and cnt[41] == graph[2][41]   # ... and row 41, NaN against all, occludes nothing


# ---------------------------------------------------------------- 4: past any cap
def test_a_long_row_among_the_neighbours(rp, ctx):
    """d = 20 000: 200 rows of 12 nonzeros around five centres and one of 5 000, which every tenth
    graph row lists: 5 000 entries exceed the built-in cap, so those points walk global memory under
    every setting.  Restatement (a) folds the columns that any row uses (5 400 of the 20 000: a column
    of zeros adds +0.0 and changes no bit), (b) runs on all 20 000"""
    n, d, nnz, k = 200, 20000, 12, 8
    rng = np.random.default_rng(3)
    centres = np.array([40, 5000, 5100, 12345, d - 40])

    def short_row():
        c = rng.choice(centres, size=3, replace=False)
        cols = np.unique(np.clip(np.concatenate([cc + rng.integers(-40, 40, size=nnz) for cc in c]), 0, d - 1))
        return np.sort(rng.choice(cols, size=nnz, replace=False)).astype(np.int32), rng.standard_normal(nnz)

    rows = [short_row() for _ in range(n)]
    rows[123] = (np.sort(rng.choice(d, size=5000, replace=False)).astype(np.int32), rng.standard_normal(5000))
    csr = cref.from_rows(rows, d)
    X = cref.densify(csr)
    D = mref.metric_matrix(X[:, np.any(X != 0, axis=0)], "l2")
    exact = mref.exact_graph(D, k)
    members = {i: exact[0][i, :k - 1].tolist() + ([123] if i % 10 == 0 else [exact[0][i, k - 1]]) for i in range(n)}
    graph = mref.hand_graph(D, k, members)
    assert (graph[0] == 123).sum() >= 20
    check_all(rp, ctx, graph, rp.Dataset.csr(ctx, *csr), rp.Dataset.dense(ctx, X), D, [8, 16], "d 20000",
              flags=(1, 3))


def test_sixty_four_long_neighbours(rp, ctx):
    """k = 64 over rows of 300 nonzeros: 19 200 entries per point, 2 016 pairs, 32 per lane"""
    n, d, k = 130, 2000, 64
    rng = np.random.default_rng(9)
    rows = [(np.sort(rng.choice(d, size=300, replace=False)).astype(np.int32), rng.standard_normal(300))
            for _ in range(n)]
    rows[5] = rows[77]
    csr = cref.from_rows(rows, d)
    X = cref.densify(csr)
    D = mref.metric_matrix(X, "l2")
    graph = mref.exact_graph(D, k)
    assert neighbour_entries(csr, graph).min() == 19200
    check_all(rp, ctx, graph, rp.Dataset.csr(ctx, *csr), rp.Dataset.dense(ctx, X), D, [64], "k 64 x 300",
              flags=(1, 3))


# ---------------------------------------------------------------- 5: degenerate graphs and sets
def test_hub_empty_rows_and_tiny_sets(rp, ctx):
    """every row lists point 0: a reverse list of n - 1 against kout = 8; graph rows of count 0; n = 0
    and n = 1; a data set without any nonzero"""
    n, d, k = 1500, 16, 4
    csr = cref.make_csr(3, n, d, 0.3, empty=(9,))
    ds = rp.Dataset.csr(ctx, *csr)
    D = mref.metric_matrix(cref.densify(csr), "l2")
    rng = np.random.default_rng(4)
    rows = {i: [0] + rng.choice(n, 3, replace=False).tolist() for i in range(1, n)}
    rows[0] = [1, 2, 3]
    graph = mref.hand_graph(D, k, rows)
    for i in (7, 8, 900):                                   # empty rows: only reverse edges reach them
        graph[0][i], graph[1][i], graph[2][i] = -1, np.inf, 0
    check_all(rp, ctx, graph, ds, rp.Dataset.dense(ctx, cref.densify(csr)), D, [8, 64], "hub")
    got, stats = prepare(rp, ctx, graph, ds, 8, 2)
    assert got[2][0] == 8 and stats[2] >= n - 1 - 3 - 8
    # n = 1 and n = 0
    one = rp.Dataset.csr(ctx, *cref.from_rows(cref.rows_of(csr)[:1], d))
    g1 = (np.full((1, 3), -1, dtype=np.int32), np.full((1, 3), np.inf), np.zeros(1, dtype=np.int32))
    none = rp.Dataset.csr(ctx, *cref.from_rows([], d))
    g0 = (np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3)), np.zeros(0, dtype=np.int32))
    for fl in FLAGS:
        got, stats = prepare(rp, ctx, g1, one, 2, fl)
        assert got[2].tolist() == [0] and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
        assert stats == (0, 0, 0)
        got, stats = prepare(rp, ctx, g0, none, 5, fl)
        assert got[0].shape == (0, 5) and got[1].shape == (0, 5) and got[2].shape == (0,)
        assert stats == (0, 0, 0)
    # no nonzero at all: every distance is 0, nothing is below 0, nothing is occluded
    zeros = cref.make_csr(3, 20, d, 0.0)
    assert zeros[0][-1] == 0
    Dz = np.zeros((20, 20))
    gz = mref.exact_graph(Dz, 5)
    check_all(rp, ctx, gz, rp.Dataset.csr(ctx, *zeros), None, Dz, [5, 10], "no nonzeros", residents=(0, -1, 1))
    assert prepare(rp, ctx, gz, rp.Dataset.csr(ctx, *zeros), 5, 1)[1] == (200, 0, 0)


def test_inconsistent_distances_row_i_wins(rp, ctx):
    """row v lists 0 at another distance than row 0 lists v: each row keeps its own, also where the cap
    cuts the own entry off (the reverse copy must not come back in its place)"""
    n, d, k = 6, 5, 3
    csr = cref.make_csr(6, n, d, 0.6)
    ds = rp.Dataset.csr(ctx, *csr)
    D = mref.metric_matrix(cref.densify(csr), "l2")
    ids, dist, cnt = mref.hand_graph(D, k, {0: [1, 2, 3], 1: [0, 2], 2: [0, 3], 3: [0, 4], 4: [5], 5: [4]})
    v = int(ids[0, 2])                                      # the farthest of row 0: kout < 3 cuts it off
    c = int(cnt[v])
    s0 = ids[v, :c].tolist().index(0)
    order = [s0] + [x for x in range(c) if x != s0]
    ids[v, :c], dist[v, :c] = ids[v, order], dist[v, order]
    dist[v, 0] = 0.0                                        # row v says 0 is at distance 0, row 0 does not
    check_all(rp, ctx, (ids, dist, cnt), ds, rp.Dataset.dense(ctx, cref.densify(csr)), D, [1, 2, 8],
              "inconsistent", flags=(2, 3))


# ---------------------------------------------------------------- 6: determinism, device arrays
def test_two_calls_and_the_dev_entry_point_give_the_same_bits(rp, ctx):
    import torch
    n, d, k, kout = 2500, 64, 10, 16
    csr = cref.make_csr(13, n, d, 0.2)
    f = build(rp, ctx, csr, 50, 3, seed=8)
    graph = rp.knnGraphSV(k, f)
    a, sa = prepare(rp, ctx, graph, f.data, kout, 3)
    b, sb = prepare(rp, ctx, graph, f.data, kout, 3)
    pref.assert_same_answer(a, b, "second call")
    assert sa == sb and sa[0] > 0
    dev = torch.device("cuda", ctx.device)
    tx = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in csr[:3]]
    held = [x.clone() for x in tx]
    dx = rp.Dataset.csr_from_torch(ctx, tx[0], tx[1], tx[2], d)

    def on_device(g, fl):
        ti, td, tc = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in g)
        keep = (ti.clone(), td.clone(), tc.clone())
        oi = torch.empty((n, kout), dtype=torch.int32, device=dev)
        od = torch.empty((n, kout), dtype=torch.float64, device=dev)
        oc = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        rp.graphPrepareSVDev(k, dx, ti.data_ptr(), td.data_ptr(), tc.data_ptr(), kout, oi.data_ptr(), od.data_ptr(),
                             oc.data_ptr(), diversify=bool(fl & 1), reverse=bool(fl & 2))
        ctx.sync()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((ti, td, tc), keep))
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(tx, held))
        return (oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()), rp.graphPrepareLast(ctx)

    c, sc = on_device(graph, 3)
    pref.assert_same_answer(c, a, "dev against host")
    assert sc == sa
    # _dev does not validate: an id outside [0, n) is skipped, a count is clamped to [0, k]
    ids, dist, cnt = (np.array(x) for x in graph)
    ids[40, 1] = n + 5
    ids[41, 0] = -7
    ids[42, 3] = 2 ** 31 - 1
    full = int(np.argmax(cnt == k))
    cnt[full] = k + 3
    cnt[44] = -2
    D = mref.metric_matrix(cref.densify(csr), "l2")
    clean = pref.clean_graph((ids, dist, cnt), n)
    assert clean[2][40] == graph[2][40] - 1 and clean[2][full] == k and clean[2][44] == 0
    for fl in FLAGS:
        got, sg = on_device((ids, dist, cnt), fl)
        want, wst = pref.graph_prepare_ref(clean, D, kout, fl)
        pref.assert_same_answer(got, want, "planted graph, flags %d" % fl)
        assert sg == wst


# ---------------------------------------------------------------- 7: refusals
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, k, kout = 1500, 16, 10, 12
    csr = cref.make_csr(12, n, d, 0.3)
    f = build(rp, ctx, csr, 30, 4, seed=7)
    ds = f.data
    graph = rp.knnGraphSV(k, f)
    csrQ = cref.make_csr(13, 16, d, 0.3)
    knn0 = rp.knnBatch(5, f, csrQ)
    cand0 = C.c_int64(-1)
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(cand0)))
    good, stats = prepare(rp, ctx, graph, ds, kout, 3)
    assert stats[0] > 0
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, data=ds, k_=k, kout_=kout, metric=0, flags=3, gids=None, gcnt=None, entry=None):
        gids = np.ascontiguousarray(graph[0] if gids is None else gids, dtype=np.int32)
        gdist = np.ascontiguousarray(graph[1])
        gcnt = np.ascontiguousarray(graph[2] if gcnt is None else gcnt, dtype=np.int32)
        before = (gids.copy(), gdist.copy(), gcnt.copy())
        ids = np.full((n, 64), 12345, dtype=np.int32)
        dist = np.full((n, 64), 0.5)
        cnt = np.full(n, 77, dtype=np.int32)
        st = (entry or L.rpt_graph_prepare_csr_host)(
            ctx._h, data._h, k_, C.c_void_p(gids.ctypes.data), C.c_void_p(gdist.ctypes.data),
            C.c_void_p(gcnt.ctypes.data), kout_, metric, flags, C.c_void_p(ids.ctypes.data),
            C.c_void_p(dist.ctypes.data), C.c_void_p(cnt.ctypes.data))
        assert st == code, (st, code)
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77)   # nothing was written
        assert all(np.array_equal(x, y) for x, y in zip((gids, gdist, gcnt), before))
        assert rp.graphPrepareLast(ctx) == stats            # nothing was launched
        return msg

    dense = rp.Dataset.dense(ctx, cref.densify(csr))
    assert "rpt_graph_prepare_*" in refused(RPT_E_ARG, data=dense)       # names the dense entry point
    for m in (COS, INN):
        assert "metric" in refused(RPT_E_UNSUPPORTED, metric=m)
    for m in (COS | INN, REF, 2, INN | 1):
        assert "metric" in refused(RPT_E_ARG, metric=m)
    assert "k must" in refused(RPT_E_ARG, k_=0)
    assert "k must" in refused(RPT_E_ARG, k_=65)
    assert "kout" in refused(RPT_E_ARG, kout_=0)
    assert "kout" in refused(RPT_E_ARG, kout_=65)
    assert "flags" in refused(RPT_E_ARG, flags=4)
    assert "flags" in refused(RPT_E_ARG, flags=3 | COS)
    assert "flags" in refused(RPT_E_ARG, flags=-1)
    # _host names the row of the graph that is out of range, as the dense entry point does
    bad = np.array(graph[2])
    bad[700] = k + 1
    assert "graph row 700: count" in refused(RPT_E_ARG, gcnt=bad)
    bad[700] = -1
    assert "graph row 700: count" in refused(RPT_E_ARG, gcnt=bad)
    bad = np.array(graph[0])
    bad[701, 0] = n
    assert graph[2][701] > 1 and "graph row 701: id" in refused(RPT_E_ARG, gids=bad)
    bad[701, 0] = -1
    assert "graph row 701: id" in refused(RPT_E_ARG, gids=bad)
    bad[701, 0] = 701
    assert "graph row 701 holds its own id" in refused(RPT_E_ARG, gids=bad)
    bad[701, 0] = bad[701, 1]
    assert "graph row 701 holds id" in refused(RPT_E_ARG, gids=bad)
    # the dense entry point keeps refusing CSR data
    for m in (0, COS, INN):
        assert "CSR" in refused(RPT_E_UNSUPPORTED, metric=m, entry=L.rpt_graph_prepare_host)
    with pytest.raises(ValueError):
        rp.graphPrepareSV(graph, ds, kout=65)
    with pytest.raises(ValueError):
        rp.graphPrepareSV((graph[0][:5], graph[1][:5], graph[2][:5]), ds)
    with pytest.raises(rp.RPTError) as e:
        rp.graphPrepareSV(graph, dense)
    assert e.value.code == RPT_E_ARG
    again, st2 = prepare(rp, ctx, graph, ds, kout, 3)
    pref.assert_same_answer(again, good, "after the refusals")
    assert st2 == stats
    # kout defaults to min(64, 2 k); a forest stands for its data set; the kNN entry points answer as before
    assert rp.graphPrepareSV(graph, f)[0].shape == (n, 2 * k)
    cand = C.c_int64(-1)
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(cand)))
    assert cand.value == cand0.value
    for x, y in zip(knn0, rp.knnBatch(5, f, csrQ)):
        assert np.array_equal(x, y, equal_nan=True)


# ---------------------------------------------------------------- 8: end to end
def test_search_on_a_prepared_graph(rp, ctx):
    """knnGraphSV -> knnGraphRefineSV -> graphPrepareSV -> graphSearchSV with kg = kout: the search
    equals its restatement on the prepared graph, which equals the restatement of the preparation"""
    n, d, k, kout, nq = 2000, 32, 10, 16, 50
    csr = cref.make_csr(21, n, d, 0.3, np.float32)
    f = build(rp, ctx, csr, 60, 2, seed=9)
    graph = rp.knnGraphRefineSV(rp.knnGraphSV(k, f), f, iters=1)
    sg, stats = prepare(rp, ctx, graph, f.data, kout, 3)
    want, wst = pref.graph_prepare_ref(graph, mref.metric_matrix(cref.densify(csr), "l2"), kout, 3)
    pref.assert_same_answer(sg, want, "prepared")
    assert stats == wst
    rng = np.random.default_rng(8)
    rows = cref.rows_of(csr)
    csrQ = cref.from_rows([(rows[i][0], (rows[i][1] + 0.2 * rng.standard_normal(len(rows[i][1]))).astype(np.float32))
                           for i in rng.choice(n, nq)], d, np.float32)
    seeds = rng.integers(0, n, size=(nq, 4)).astype(np.int32)
    got = rp.graphSearchSV(sg, f.data, csrQ, 10, ef=32, seeds=seeds)
    model = scref.graph_search_csr_ref(csr, csrQ, sg[0], sg[2], seeds, 10, 32)
    scref.assert_same_answer(got, model[0], "search on the prepared graph")
    assert rp.graphSearchLast(ctx)[0] == model[1]


# ---------------------------------------------------------------- 9: the profile class, the C++ mirror
def test_prof_class_3_times_the_call(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    csr = cref.make_csr(14, 1000, 16, 0.3)
    ds = rp.Dataset.csr(ctx, *csr)
    graph = mref.exact_graph(mref.metric_matrix(cref.densify(csr), "l2"), 5)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        _lib.check(L.rpt_prof_reset(ctx._h))
        rp.graphPrepareSV(graph, ds, kout=8)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
        assert cnt.value == 1 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))


def test_cpp_example(tmp_path):
    """host/example_graph_prepare_sparse.cpp folds the pair distances that decide the keep rule again on
    the host over the union of the two supports and walks the rule for a sample of rows"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "example_graph_prepare_sparse")
    src = os.path.join(root, "rp-tree_amd", "host", "example_graph_prepare_sparse.cpp")
    lib = os.path.join(root, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "1200", "40", "60", "0.2", "3", "40", "8", "1", "5", "16"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and any(ln.startswith("recall@5 ") for ln in lines[-4:])
