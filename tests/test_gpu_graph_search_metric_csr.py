"""Best-first beam search over the kNN graph on SVector (CSR) rows under the cosine and inner-product
distances on the device (rpt_graph_search_csr_metric_host / _dev, csrc/graph_search_csr.hip): ids,
counts and distance BITS, no tolerance anywhere, against (a) the numpy restatement under dotS
(tests/graph_metric_csr_ref.py), (b) rp.graphSearch(metric=) on Dataset.dense of the dense-ified rows
and queries while every stored value is finite (tests/test_graph_metric_csr_host.py has the argument;
with a stored inf or NaN the two definitions part, and the test asserts that they do) and (c)
bruteKnn(metric=) on the CSR sets where named."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_metric_csr_ref as gm  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
NP = {"f64": np.float64, "f32": np.float32}
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


def dense_pair(rp, ctx, csrX, csrQ, dtype="f64"):
    """oracle (b)'s inputs: Dataset.dense of the dense-ified rows, the dense-ified queries"""
    return (rp.Dataset.dense(ctx, gm.densify(csrX).astype(NP[dtype])), gm.densify(csrQ).astype(NP[dtype]))


def search(rp, ctx, metric, graph, ds, csrQ, k, ef, seeds):
    got = rp.graphSearchMetricSV(distf_of(rp, metric), graph, ds, csrQ, k, ef=ef, seeds=seeds)
    return got, rp.graphSearchLast(ctx)


def check_padding(got, k):
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][pad] == -1) and np.all(np.isposinf(got[1][pad]))


def ring_graph(n, kg, rng=None):
    """every row lists its kg successors; with rng, slot 2 is a random chord (the ring alone is a long walk)"""
    gids = np.array([[(i + 1 + e) % n for e in range(kg)] for i in range(n)], dtype=np.int32)
    if rng is not None:
        gids[:, 2] = rng.integers(0, n, size=n)
    return gids, np.full(n, kg, dtype=np.int32)


def make_seeds(rng, nq, n, s):
    """random seeds with a repeated id in every row, -1 padding in every third; row 7 has none"""
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    seeds[:, 5] = seeds[:, 1]
    seeds[::3, 6:] = -1
    seeds[1, 0] = -1
    seeds[7, :] = -1
    return seeds


def all_ways(rp, ctx, metric, graph, ds, csrX, csrQ, k, ef, seeds, tag, D, dense=None):
    """the search against (a) and, with `dense`, (b), then under graph_search_nofilter and
    graph_search_csr_stream: the same answer and the same expansions every time"""
    want, exp, offered, upper = gm.graph_search_ref(csrX, csrQ, graph[0], graph[-1], seeds, k, ef, metric, D=D)
    got, (g_exp, g_eval) = search(rp, ctx, metric, graph, ds, csrQ, k, ef, seeds)
    print("%s: expansions %d, evaluated %d in [%d, %d]" % (tag, g_exp, g_eval, offered, upper))
    gm.assert_same_answer(got, want, tag + ", restatement")
    check_padding(got, k)
    assert g_exp == exp, tag
    assert offered <= g_eval <= upper, tag
    if dense is not None:
        dd, dq = dense
        twin = rp.graphSearch(graph, dd, dq, k, ef=ef, seeds=seeds, metric=distf_of(rp, metric))
        gm.assert_same_answer(got, twin, tag + ", dense entry point")
        assert rp.graphSearchLast(ctx) == (g_exp, g_eval), tag
    with option(ctx, "graph_search_nofilter", 1):
        got2, (n_exp, n_eval) = search(rp, ctx, metric, graph, ds, csrQ, k, ef, seeds)
    gm.assert_same_answer(got2, got, tag + ", graph_search_nofilter")
    assert n_exp == exp and g_eval <= n_eval <= upper, tag
    with option(ctx, "graph_search_csr_stream", 1):
        got3, stats3 = search(rp, ctx, metric, graph, ds, csrQ, k, ef, seeds)
    gm.assert_same_answer(got3, got, tag + ", graph_search_csr_stream")
    assert stats3 == (g_exp, g_eval), tag
    return got


# ---------------------------------------------------------------- 1: the grid
_grid = {}


def make_queries(csrX, seed, nq, density, dtype):
    """random sparse queries; the first are stored rows themselves, one is empty"""
    d = csrX[3]
    stored = gm.rows_of(csrX)
    rows = [(c.copy(), v.copy()) for c, v in gm.rows_of(gm.make_csr(seed, nq, d, density, NP[dtype]))]
    for i, j in enumerate((17, 5, 900)):
        rows[i] = stored[j]
    rows[3] = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=NP[dtype]))
    return gm.from_rows(rows, d, NP[dtype])


def grid_case(rp, ctx, dtype, d, density):
    """the sets, their forest and dense twins; only the last key is kept.  D and the graphs per distance"""
    key = (dtype, d, density)
    if key not in _grid:
        _grid.clear()
        n, nq = 1500, 48
        csrX = gm.make_csr(d + int(100 * density), n, d, density, NP[dtype])
        csrQ = make_queries(csrX, 1000 + d, nq, density, dtype)
        f = build(rp, ctx, csrX, 40, 4, seed=1234 + d)
        _grid[key] = (csrX, csrQ, f, dense_pair(rp, ctx, csrX, csrQ, dtype), {}, {})
    return _grid[key]


@pytest.mark.parametrize("kg,s", [(10, 8), (64, 8)])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("density", [0.05, 0.3])
@pytest.mark.parametrize("d", [24, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_search_matches_the_definition(rp, ctx, dtype, d, density, metric, kg, s):
    """d = 24 at density 0.05 leaves three rows in ten empty (cosine: NaN, by id); seeds with repeats,
    -1 padding and an all -1 row"""
    csrX, csrQ, f, dense, Ds, graphs = grid_case(rp, ctx, dtype, d, density)
    assert f.data.is_csr
    if metric not in Ds:
        Ds[metric] = gm.query_matrix(csrX, csrQ, metric)
    if (metric, kg) not in graphs:
        graphs[metric, kg] = rp.knnGraphMetricSV(distf_of(rp, metric), kg, f)
    seeds = make_seeds(np.random.default_rng(7 * s + kg), 48, 1500, s)
    got = all_ways(rp, ctx, metric, graphs[metric, kg], f.data, csrX, csrQ, 10, 32, seeds,
                   "%s %s d %d density %g kg %d s %d" % (metric, dtype, d, density, kg, s), Ds[metric], dense)
    assert got[2][7] == 0
    if metric == "cosine":
        assert np.isnan(got[1][3, :got[2][3]]).all() and got[2][3] == 10     # the empty query
        assert np.array_equal(np.sort(got[0][3]), got[0][3])


# ---------------------------------------------------------------- 2: piece edges
NNZ = (0, 1, 63, 64, 65, 127, 128, 129, 300)


def edge_rows(seed, count, d):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(count):
        m = NNZ[i % len(NNZ)]
        rows.append((np.sort(rng.choice(d, size=m, replace=False)).astype(np.int32), rng.standard_normal(m)))
    return rows, rng


@pytest.fixture(scope="module")
def edge_case(rp, ctx):
    """d = 300, n = 300: rows and queries of 0, 1, 63, 64, 65, 127, 128, 129 and 300 entries (one piece
    of a streamed query is 64 entries); among the 64s, supports wholly below the query's, wholly above
    it, identical, and interleaved with it without meeting"""
    d, n, nq = 300, 300, 36
    rows, rng = edge_rows(1, n, d)
    qrows, qrng = edge_rows(2, nq, d)
    block = lambda lo: np.arange(lo, lo + 64, dtype=np.int32)  # noqa: E731
    qrows[3] = (block(100), qrng.standard_normal(64))       # the query in the middle
    rows[3] = (block(0), rng.standard_normal(64))           # wholly below it
    rows[12] = (block(236), rng.standard_normal(64))        # wholly above it
    rows[21] = (block(100), rng.standard_normal(64))        # the same support
    qrows[12] = (np.arange(100, 228, 2, dtype=np.int32), qrng.standard_normal(64))
    rows[30] = (np.arange(101, 229, 2, dtype=np.int32), rng.standard_normal(64))   # interleaved, disjoint
    qrows[21] = rows[39]                                     # a stored row of 64 itself
    csrX, csrQ = gm.from_rows(rows, d), gm.from_rows(qrows, d)
    assert sorted(set(np.diff(csrX[0]).tolist())) == sorted(NNZ) == sorted(set(np.diff(csrQ[0]).tolist()))
    gids = np.stack([rng.permutation(np.delete(np.arange(n), i))[:64] for i in range(n)]).astype(np.int32)
    graph = (gids, np.full(n, 64, dtype=np.int32))
    seeds = np.stack([rng.permutation(n)[:64] for _ in range(nq)]).astype(np.int32)
    seeds[3, :4] = [3, 12, 21, 30]
    seeds[12, :4] = [3, 12, 21, 30]
    ds = rp.Dataset.csr(ctx, *csrX)
    Ds = {m: gm.query_matrix(csrX, csrQ, m) for m in METRICS}
    for q, v in ((3, 3), (3, 12), (12, 30)):                 # no shared column: inner -0.0, cosine exactly 1
        assert Ds["inner"][q, v] == 0.0 and np.signbit(Ds["inner"][q, v]) and Ds["cosine"][q, v] == 1.0
    assert Ds["inner"][3, 21] != 0.0
    return csrX, csrQ, graph, seeds, ds, Ds, dense_pair(rp, ctx, csrX, csrQ)


@pytest.mark.parametrize("k,ef", [(1, 1), (64, 256)])
@pytest.mark.parametrize("metric", METRICS)
def test_piece_edges(rp, ctx, edge_case, metric, k, ef):
    csrX, csrQ, graph, seeds, ds, Ds, dense = edge_case
    got = all_ways(rp, ctx, metric, graph, ds, csrX, csrQ, k, ef, seeds, "edges %s k %d ef %d" % (metric, k, ef),
                   Ds[metric], dense)
    if k == 64:                                              # the beam holds all 300 rows: the disjoint pairs are in
        for q, v in ((3, 3), (3, 12), (12, 30)):             # the answer with the bits of the definition
            at = np.flatnonzero(got[0][q] == v)
            if len(at):
                assert gm.bits(got[1][q, at[0]]) == gm.bits(Ds[metric][q, v])


# ---------------------------------------------------------------- 3: queries around the resident cap
@pytest.mark.parametrize("metric", METRICS)
def test_queries_around_the_resident_cap(rp, ctx, metric):
    """d = 6 000: 200 rows of 12 entries around five centres and one of 5 000; queries of 12, 2 048
    (the last that stays in LDS), 2 049 and 5 000 entries (streamed by their length), the long row
    itself.  Short rows against a long streamed query end the piece loop early"""
    n, d, nnz, k, ef = 200, 6000, 12, 8, 24
    rng = np.random.default_rng(3)
    centres = np.array([40, 1500, 1600, 4321, d - 40])

    def short_row():
        c = rng.choice(centres, size=3, replace=False)
        cols = np.unique(np.clip(np.concatenate([cc + rng.integers(-40, 40, size=nnz) for cc in c]), 0, d - 1))
        return np.sort(rng.choice(cols, size=nnz, replace=False)).astype(np.int32), rng.standard_normal(nnz)

    def long_row(m):
        return np.sort(rng.choice(d, size=m, replace=False)).astype(np.int32), rng.standard_normal(m)

    rows = [short_row() for _ in range(n)]
    rows[123] = long_row(5000)
    qrows = [short_row() for _ in range(3)] + [long_row(m) for m in (2048, 2049, 5000)] + [rows[123], rows[7]]
    csrX, csrQ = gm.from_rows(rows, d), gm.from_rows(qrows, d)
    graph = ring_graph(n, 6, rng)
    graph[0][::50, 0] = 123                                  # the long row is reached
    seeds = rng.integers(0, n, size=(len(qrows), 3)).astype(np.int32)
    seeds[6] = [123, 122, 5]
    ds = rp.Dataset.csr(ctx, *csrX)
    got = all_ways(rp, ctx, metric, graph, ds, csrX, csrQ, k, ef, seeds, "d 6000 " + metric,
                   gm.query_matrix(csrX, csrQ, metric), dense_pair(rp, ctx, csrX, csrQ))
    assert got[0][6, 0] == 123


# ---------------------------------------------------------------- 4: awkward values
def awkward_rows(d, dtype):
    """the awkward rows of test_gpu_knn_graph_csr.py (empty rows, duplicates, a full row, stored +0.0
    and -0.0, only column 0, only column d - 1, rows x 10) with an inf and a NaN entry planted"""
    from test_gpu_knn_graph_csr import awkward_rows as base
    csr, empty = base(d, dtype)
    rows = gm.rows_of(csr)
    full = np.arange(d, dtype=np.int32)
    rng = np.random.default_rng(100 + d)
    vi, vn = rng.standard_normal(d).astype(NP[dtype]), rng.standard_normal(d).astype(NP[dtype])
    vi[0], vn[d - 1] = np.inf, np.nan
    rows[40], rows[41] = (full, vi), (full, vn)
    return gm.from_rows(rows, d, NP[dtype]), rows


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("metric", METRICS)
def test_awkward_values(rp, ctx, metric, dtype):
    """held to the dotS restatement alone: a row that stores an inf where the query stores nothing takes
    no product there, the dense fold meets inf * 0 = NaN; the test asserts the dense answer differs"""
    d = 33
    csrX, rows = awkward_rows(d, dtype)
    n, k, ef = len(rows), 10, 32
    rng = np.random.default_rng(d)
    qrows = [(c.copy(), v.copy()) for c, v in gm.rows_of(gm.make_csr(50 + d, 24, d, 0.3, NP[dtype]))]
    full = np.arange(d, dtype=np.int32)
    qrows[0] = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=NP[dtype]))    # empty
    qrows[1] = rows[17]                                      # a stored row, which has duplicates
    qrows[2] = (full[::2], np.concatenate([[np.inf], rng.standard_normal(len(full[::2]) - 1)]).astype(NP[dtype]))
    qrows[3] = (full[1::2], np.concatenate([rng.standard_normal(len(full[1::2]) - 1), [np.nan]]).astype(NP[dtype]))
    qrows[4] = (np.array([0], dtype=np.int32), np.array([-0.0], dtype=NP[dtype]))   # nothing but a stored zero
    qrows[5] = rows[20]                                      # the row of stored +0.0 and -0.0
    qrows[6] = rows[40]                                      # the stored inf row
    csrQ = gm.from_rows(qrows, d, NP[dtype])
    graph = ring_graph(n, 7, rng)
    seeds = rng.integers(0, n, size=(24, 4)).astype(np.int32)
    seeds[1] = [17, 590, 7, 3]
    seeds[:, 0] = 40                                         # the inf row is offered to every query,
    seeds[::2, 1] = 41                                       # the NaN row to every other
    ds = rp.Dataset.csr(ctx, *csrX)
    D = gm.query_matrix(csrX, csrQ, metric)
    want, exp, offered, upper = gm.graph_search_ref(csrX, csrQ, graph[0], graph[1], seeds, k, ef, metric, D=D)
    for stream in (0, 1):
        with option(ctx, "graph_search_csr_stream", stream):
            got, stats = search(rp, ctx, metric, graph, ds, csrQ, k, ef, seeds)
        gm.assert_same_answer(got, want, "awkward %s %s stream %d" % (metric, dtype, stream))
        assert stats[0] == exp and offered <= stats[1] <= upper
    assert np.all(got[2] == k)
    if metric == "cosine":                                   # empty and all-zero queries: NaN from everything, by id
        for q in (0, 4):
            assert np.isnan(got[1][q]).all() and np.array_equal(np.sort(got[0][q]), got[0][q])
    else:
        assert np.all(got[1][0] == 0.0) and np.signbit(got[1][0]).all() and np.array_equal(np.sort(got[0][0]), got[0][0])
    # the case bites: the dense definition on the dense-ified sets answers otherwise
    dd, dq = dense_pair(rp, ctx, csrX, csrQ, dtype)
    twin = rp.graphSearch(graph, dd, dq, k, ef=ef, seeds=seeds, metric=distf_of(rp, metric))
    assert not (np.array_equal(twin[0], got[0]) and np.array_equal(gm.bits(twin[1]), gm.bits(got[1])))
    assert not np.array_equal(gm.bits(gm.dense_query_matrix(csrX, csrQ, metric)), gm.bits(D))


# ---------------------------------------------------------------- 5: the complete graph
@pytest.mark.parametrize("metric", METRICS)
def test_complete_graph_gives_the_brute_force_answer(rp, ctx, metric):
    """n = 65, every row lists all others (kg = 64: a full wave of candidates per offer), ef = 256,
    one seed: the beam ends up holding every point"""
    n, d, k, nq = 65, 40, 10, 16
    csrX = gm.make_csr(65, n, d, 0.25, empty=(9,))
    rows = gm.rows_of(csrX)
    rows[11] = rows[40]
    csrX = gm.from_rows(rows, d)
    csrQ = gm.from_rows(rows[:8] + gm.rows_of(gm.make_csr(66, 8, d, 0.25)), d)
    gids = np.array([[j for j in range(n) if j != i] for i in range(n)], dtype=np.int32)
    gcnt = np.full(n, n - 1, dtype=np.int32)
    seeds = np.random.default_rng(60).integers(0, n, size=(nq, 1)).astype(np.int32)
    ds = rp.Dataset.csr(ctx, *csrX)
    got, (exp, evaluated) = search(rp, ctx, metric, (gids, gcnt), ds, csrQ, k, 256, seeds)
    want, w_exp, offered, upper = gm.graph_search_ref(csrX, csrQ, gids, gcnt, seeds, k, 256, metric)
    gm.assert_same_answer(got, want, "restatement")
    bi, bd = rp.bruteKnn(ds, csrQ, k, metric=distf_of(rp, metric))
    assert np.array_equal(got[0], bi) and np.array_equal(gm.bits(got[1]), gm.bits(bd)) and np.all(got[2] == k)
    assert exp == w_exp == nq * n and offered == evaluated == nq * n


# ---------------------------------------------------------------- 6: repeat calls and entry points
@pytest.fixture(scope="module")
def plain_case(rp, ctx):
    n, d, nq = 2500, 64, 100
    csrX = gm.make_csr(13, n, d, 0.2)
    csrQ = gm.make_csr(14, nq, d, 0.2)
    f = build(rp, ctx, csrX, 50, 3, seed=8)
    seeds = np.random.default_rng(5).integers(0, n, size=(nq, 6)).astype(np.int32)
    return csrX, csrQ, f, seeds


@pytest.mark.parametrize("metric", METRICS)
def test_two_calls_and_the_dev_entry_point_give_the_same_bits(rp, ctx, plain_case, metric):
    import torch
    csrX, csrQ, f, seeds = plain_case
    n, d, kg, k, ef, s, nq = 2500, 64, 10, 10, 48, 6, 100
    ds = f.data
    graph = rp.knnGraphMetricSV(distf_of(rp, metric), kg, f)
    a, sa = search(rp, ctx, metric, graph, ds, csrQ, k, ef, seeds)
    b, sb = search(rp, ctx, metric, graph, ds, csrQ, k, ef, seeds)
    gm.assert_same_answer(a, b, "second call")
    assert sa == sb
    want, exp, offered, upper = gm.graph_search_ref(csrX, csrQ, graph[0], graph[2], seeds, k, ef, metric)
    gm.assert_same_answer(a, want, "restatement")
    dev = torch.device("cuda", ctx.device)
    tx = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in csrX[:3]]
    tq = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in csrQ[:3]]
    dx = rp.Dataset.csr_from_torch(ctx, tx[0], tx[1], tx[2], d)
    dq = rp.Dataset.csr_from_torch(ctx, tq[0], tq[1], tq[2], d)
    tg, tc, ts = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (graph[0], graph[2], seeds))
    ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
    dist = torch.empty((nq, k), dtype=torch.float64, device=dev)
    cnt = torch.empty(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.graphSearchMetricSVDev(distf_of(rp, metric), dx, dq, kg, tg.data_ptr(), tc.data_ptr(), s, ts.data_ptr(), k, ef,
                              ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    ctx.sync()
    gm.assert_same_answer((ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), a, "dev against host")
    assert rp.graphSearchLast(ctx) == sa


def test_metric_0_gives_the_bits_of_the_l2_entry_point(rp, ctx, plain_case):
    csrX, csrQ, f, seeds = plain_case
    graph = rp.knnGraphSV(10, f)
    want = rp.graphSearchSV(graph, f.data, csrQ, 10, ef=48, seeds=seeds)
    stats = rp.graphSearchLast(ctx)
    for distf in (None, rp.metricL2):
        got = rp.graphSearchMetricSV(distf, graph, f.data, csrQ, 10, ef=48, seeds=seeds)
        gm.assert_same_answer(got, want, "metric 0")
        assert rp.graphSearchLast(ctx) == stats
    with option(ctx, "graph_search_csr_stream", 1):
        gm.assert_same_answer(rp.graphSearchMetricSV(None, graph, f.data, csrQ, 10, ef=48, seeds=seeds), want,
                              "metric 0, streamed")


# ---------------------------------------------------------------- 7: seeds from a forest
@pytest.mark.parametrize("metric", METRICS)
def test_seeds_from_a_forest(rp, ctx, metric):
    n, d, kg, k = 3000, 32, 10, 10
    distf = distf_of(rp, metric)
    csrX = gm.make_csr(21, n, d, 0.3, np.float32)
    f = build(rp, ctx, csrX, 60, 2, seed=9)
    graph = rp.knnGraphRefineMetricSV(distf, rp.knnGraphMetricSV(distf, kg, f), f, iters=1)
    rng = np.random.default_rng(8)
    rows = gm.rows_of(csrX)
    csrQ = gm.from_rows([(rows[i][0], (rows[i][1] + 0.2 * rng.standard_normal(len(rows[i][1]))).astype(np.float32))
                         for i in rng.choice(n, 50)], d, np.float32)
    got = rp.graphSearchMetricSV(distf, graph, f, csrQ, k, ef=32, forest=f, seed_k=8)
    stats = rp.graphSearchLast(ctx)
    sid, _, scnt = rp.knnBatch(8, f, csrQ, dedup=True, metric=distf)
    seeds = np.where(np.arange(8)[None, :] < scnt[:, None], sid, -1).astype(np.int32)
    want = rp.graphSearchMetricSV(distf, graph, f.data, csrQ, k, ef=32, seeds=seeds)
    gm.assert_same_answer(got, want, "forest seeds")
    assert rp.graphSearchLast(ctx) == stats
    D = gm.query_matrix(csrX, csrQ, metric)
    model, exp, offered, upper = gm.graph_search_ref(csrX, csrQ, graph[0], graph[2], seeds, k, 32, metric, D=D)
    gm.assert_same_answer(got, model, "restatement")
    assert stats[0] == exp and offered <= stats[1] <= upper
    # ef = None means max(k, 32); SVectors as queries
    gm.assert_same_answer(rp.graphSearchMetricSV(distf, graph, f, csrQ, k, seeds=seeds), want, "default ef")
    svs = [rp.SVector(d, c, v) for c, v in gm.rows_of(csrQ)[:5]]
    few = rp.graphSearchMetricSV(distf, graph, f, svs, k, ef=32, seeds=seeds[:5])
    gm.assert_same_answer(few, tuple(x[:5] for x in want), "SVector queries")


# ---------------------------------------------------------------- 8: refusals, degenerate sizes
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, kg, k, s, nq = 1500, 16, 10, 10, 4, 16
    csrX = gm.make_csr(12, n, d, 0.3)
    csrQ = gm.make_csr(13, nq, d, 0.3)
    f = build(rp, ctx, csrX, 30, 4, seed=7)
    ds = f.data
    qd = rp.Dataset.csr(ctx, *csrQ)
    graph = rp.knnGraphMetricSV(rp.metricCosine, kg, f)
    seeds0 = np.random.default_rng(3).integers(0, n, size=(nq, s)).astype(np.int32)
    good = rp.graphSearchMetricSV(rp.metricCosine, graph, ds, qd, k, ef=32, seeds=seeds0)
    stats = rp.graphSearchLast(ctx)
    gm.assert_same_answer(good, gm.graph_search_ref(csrX, csrQ, graph[0], graph[2], seeds0, k, 32, "cosine")[0],
                          "before the refusals")
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, data=ds, queries=qd, kg_=kg, s_=s, k_=k, ef_=32, metric=COS, flags=0, gids=None, entry=None):
        gids = np.ascontiguousarray(graph[0] if gids is None else gids, dtype=np.int32)
        gcnt = np.ascontiguousarray(graph[2], dtype=np.int32)
        ids = np.full((nq, 64), 12345, dtype=np.int32)
        dist = np.full((nq, 64), 0.5)
        cnt = np.full(nq, 77, dtype=np.int32)
        st = (entry or L.rpt_graph_search_csr_metric_host)(
            ctx._h, data._h, queries._h, kg_, C.c_void_p(gids.ctypes.data), C.c_void_p(gcnt.ctypes.data), s_,
            C.c_void_p(seeds0.ctypes.data), k_, ef_, metric, flags, C.c_void_p(ids.ctypes.data),
            C.c_void_p(dist.ctypes.data), C.c_void_p(cnt.ctypes.data))
        assert st == code, (st, code)
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77)   # nothing was written
        assert rp.graphSearchLast(ctx) == stats            # nothing was launched
        return msg

    for m in (COS | INN, REF, 2, INN | 1, -1):
        assert "metric" in refused(RPT_E_ARG, metric=m)
    for fl in (COS, INN, REF, 1):
        assert "flags" in refused(RPT_E_ARG, flags=fl)
    dense = rp.Dataset.dense(ctx, gm.densify(csrX))
    qdense = rp.Dataset.dense(ctx, gm.densify(csrQ))
    for m in (0, COS, INN):
        assert "rpt_graph_search_*" in refused(RPT_E_ARG, data=dense, queries=qdense, metric=m)   # the dense entry point
    assert "both" in refused(RPT_E_ARG, queries=qdense)
    assert "ef" in refused(RPT_E_ARG, ef_=9)
    assert "kg" in refused(RPT_E_ARG, kg_=65)
    bad = np.array(graph[0])
    bad[701, 0] = n
    assert graph[2][701] > 0 and "graph row 701" in refused(RPT_E_ARG, gids=bad)     # before any upload
    # the old entry points still refuse a metric, and say where it went
    for m in (COS, INN):
        msg = refused(RPT_E_UNSUPPORTED, metric=m, entry=L.rpt_graph_search_csr_host)
        assert "metric" in msg and "rpt_graph_search_csr_metric_*" in msg
        assert "rpt_graph_search_csr_metric_*" in refused(RPT_E_UNSUPPORTED, metric=m, entry=L.rpt_graph_search_host)
    with pytest.raises(rp.RPTError) as e:
        rp.graphSearch(graph, ds, qd, k, ef=32, seeds=seeds0, metric=rp.metricCosine)
    assert e.value.code == RPT_E_UNSUPPORTED and "rpt_graph_search_csr_metric_*" in str(e.value)
    with pytest.raises(ValueError):
        rp.graphSearchMetricSV(rp.metricCosine, graph, ds, qd, k)     # neither seeds nor a forest
    with pytest.raises(NotImplementedError):
        rp.graphSearchMetricSV(lambda u, v: 0.0, graph, ds, qd, k, seeds=seeds0)
    again = rp.graphSearchMetricSV(rp.metricCosine, graph, ds, qd, k, ef=32, seeds=seeds0)
    gm.assert_same_answer(again, good, "after the refusals")
    assert rp.graphSearchLast(ctx) == stats


@pytest.mark.parametrize("metric", METRICS)
def test_no_queries_no_points_and_one_point(rp, ctx, metric):
    d = 8
    distf = distf_of(rp, metric)
    csrX = gm.make_csr(1, 50, d, 0.4)
    ds = rp.Dataset.csr(ctx, *csrX)
    graph = ring_graph(50, 3)
    none = gm.from_rows([], d)
    ids, dist, cnt = rp.graphSearchMetricSV(distf, graph, ds, none, 5, seeds=np.zeros((0, 2), dtype=np.int32))
    assert ids.shape == (0, 5) and dist.shape == (0, 5) and cnt.shape == (0,)
    assert rp.graphSearchLast(ctx) == (0, 0)
    csrQ = gm.make_csr(2, 4, d, 0.4)
    one_csr = gm.from_rows(gm.rows_of(csrX)[:1], d)
    one = rp.Dataset.csr(ctx, *one_csr)
    g1 = (np.full((1, 2), -1, dtype=np.int32), np.zeros(1, dtype=np.int32))
    seeds = np.array([[0], [-1], [0], [0]], dtype=np.int32)
    got = rp.graphSearchMetricSV(distf, g1, one, csrQ, 3, ef=3, seeds=seeds)
    gm.assert_same_answer(got, gm.graph_search_ref(one_csr, csrQ, g1[0], g1[1], seeds, 3, 3, metric)[0], "n = 1")
    assert got[2].tolist() == [1, 0, 1, 1] and rp.graphSearchLast(ctx) == (3, 3)
    empty = rp.Dataset.csr(ctx, *none)
    g0 = (np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int32))
    got = rp.graphSearchMetricSV(distf, g0, empty, csrQ, 3, seeds=np.full((4, 2), -1, dtype=np.int32))
    assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))


# ---------------------------------------------------------------- 9: the C++ mirror
def test_cpp_example(tmp_path):
    """host/example_graph_search_sparse_metric.cpp: build, refine, prepare and search under cosine, every
    reported distance folded again on the host over the shared columns and compared by its bits"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "example_graph_search_sparse_metric")
    src = os.path.join(root, "rp-tree_amd", "host", "example_graph_search_sparse_metric.cpp")
    lib = os.path.join(root, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "1200", "40", "60", "0.2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and any(ln.startswith("recall@") for ln in lines)
