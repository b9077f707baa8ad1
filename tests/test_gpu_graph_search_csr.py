"""Best-first beam search over the kNN graph on SVector (CSR) rows on the device
(rpt_graph_search_csr_host / _dev, csrc/graph_search_csr.hip): ids, counts and distance BITS, no
tolerance anywhere, against (a) the numpy restatement on the dense-ified sets
(tests/graph_search_csr_ref.py), (b) rp.graphSearch on Dataset.dense of the dense-ified rows and
queries and (c) bruteKnn on the CSR sets where named."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_csr_ref as cref  # noqa: E402
import graph_search_csr_ref as scref  # noqa: E402

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


def build(rp, ctx, csr, minl, T, seed=1234):
    n, d = len(csr[0]) - 1, csr[3]
    cfg = rp.rpTreeCfg(minl, max(n, 2), d)
    return rp.forestBatch(seed, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, csr, ctx=ctx)


def dense_pair(rp, ctx, csrX, csrQ, dtype="f64"):
    """oracle (b)'s inputs: Dataset.dense of the dense-ified rows, the dense-ified queries"""
    return (rp.Dataset.dense(ctx, cref.densify(csrX).astype(NP[dtype])), cref.densify(csrQ).astype(NP[dtype]))


def search(rp, ctx, graph, ds, csrQ, k, ef, seeds):
    got = rp.graphSearchSV(graph, ds, csrQ, k, ef=ef, seeds=seeds)
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
    """random seeds; with s = 8 a repeated id in every row, -1 padding in every third; row 7 has none"""
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    if s >= 8:
        seeds[:, 5] = seeds[:, 1]
        seeds[::3, 6:] = -1
        seeds[1, 0] = -1
    seeds[7, :] = -1
    return seeds


def all_ways(rp, ctx, graph, ds, csrX, csrQ, k, ef, seeds, tag, dtype="f64", D=None, dense=None):
    """the CSR search against (a) and (b), then under graph_search_nofilter and graph_search_csr_stream:
    the same answer and the same expansions every time"""
    want, exp, offered, upper = scref.graph_search_csr_ref(csrX, csrQ, graph[0], graph[-1], seeds, k, ef, D=D)
    got, (g_exp, g_eval) = search(rp, ctx, graph, ds, csrQ, k, ef, seeds)
    print("%s: expansions %d, evaluated %d in [%d, %d]" % (tag, g_exp, g_eval, offered, upper))
    scref.assert_same_answer(got, want, tag + ", restatement")
    check_padding(got, k)
    assert g_exp == exp, tag
    assert offered <= g_eval <= upper, tag
    dd, dq = dense if dense is not None else dense_pair(rp, ctx, csrX, csrQ, dtype)
    scref.assert_same_answer(got, rp.graphSearch(graph, dd, dq, k, ef=ef, seeds=seeds), tag + ", dense entry point")
    assert rp.graphSearchLast(ctx)[0] == exp
    with option(ctx, "graph_search_nofilter", 1):
        got2, (n_exp, n_eval) = search(rp, ctx, graph, ds, csrQ, k, ef, seeds)
    scref.assert_same_answer(got2, got, tag + ", graph_search_nofilter")
    assert n_exp == exp and g_eval <= n_eval <= upper, tag
    with option(ctx, "graph_search_csr_stream", 1):
        got3, (s_exp, s_eval) = search(rp, ctx, graph, ds, csrQ, k, ef, seeds)
    scref.assert_same_answer(got3, got, tag + ", graph_search_csr_stream")
    assert s_exp == exp and offered <= s_eval <= upper, tag
    return got


# ---------------------------------------------------------------- 1: the grid
_grid = {}


def make_queries(csrX, seed, nq, density, dtype):
    """random sparse queries; the first are stored rows themselves, one is empty"""
    d = csrX[3]
    stored = cref.rows_of(csrX)
    rows = [(c.copy(), v.copy()) for c, v in cref.rows_of(cref.make_csr(seed, nq, d, density, NP[dtype]))]
    for i, j in enumerate((17, 5, 900)):
        rows[i] = stored[j]
    rows[3] = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=NP[dtype]))
    return cref.from_rows(rows, d, NP[dtype])


def grid_case(rp, ctx, dtype, d, density):
    key = (dtype, d, density)
    if key not in _grid:
        n, nq = 1500, 48
        csrX = cref.make_csr(d + int(100 * density), n, d, density, NP[dtype])
        csrQ = make_queries(csrX, 1000 + d, nq, density, dtype)
        f = build(rp, ctx, csrX, 40, 4, seed=1234 + d)
        X64, Q64 = cref.densify(csrX), cref.densify(csrQ)
        D = scref.sref.query_matrix(X64, Q64, "l2")
        dense = (rp.Dataset.dense(ctx, X64.astype(NP[dtype])), Q64.astype(NP[dtype]))
        _grid[key] = (csrX, csrQ, f, D, dense, {})
    return _grid[key]


@pytest.mark.parametrize("kg,s", [(10, 1), (10, 8), (64, 8)])
@pytest.mark.parametrize("density", [0.05, 0.3])
@pytest.mark.parametrize("d", [24, 70, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_search_matches_the_dense_definition(rp, ctx, dtype, d, density, kg, s):
    csrX, csrQ, f, D, dense, graphs = grid_case(rp, ctx, dtype, d, density)
    assert f.data.is_csr
    if kg not in graphs:
        graphs[kg] = rp.knnGraphSV(kg, f)
    graph = graphs[kg]
    seeds = make_seeds(np.random.default_rng(7 * s + kg), 48, 1500, s)
    got = all_ways(rp, ctx, graph, f.data, csrX, csrQ, 10, 32, seeds,
                   "%s d %d density %g kg %d s %d" % (dtype, d, density, kg, s), dtype, D=D, dense=dense)
    assert got[2][7] == 0


# ---------------------------------------------------------------- 2: piece and cap edges
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
    """d = 300, n = 300: rows and queries of 0, 1, 63, 64, 65, 127, 128, 129 and 300 nonzeros (one
    piece of a streamed query is 64 entries; 300 = d is the resident cap here); among the 64s,
    supports wholly below the query's, wholly above it and interleaved with it without meeting"""
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
    csrX, csrQ = cref.from_rows(rows, d), cref.from_rows(qrows, d)
    assert sorted(set(np.diff(csrX[0]).tolist())) == sorted(NNZ) == sorted(set(np.diff(csrQ[0]).tolist()))
    gids = np.stack([rng.permutation(np.delete(np.arange(n), i))[:64] for i in range(n)]).astype(np.int32)
    graph = (gids, np.full(n, 64, dtype=np.int32))
    seeds = np.stack([rng.permutation(n)[:64] for _ in range(nq)]).astype(np.int32)
    seeds[3, :4] = [3, 12, 21, 30]
    seeds[12, :4] = [3, 12, 21, 30]
    ds = rp.Dataset.csr(ctx, *csrX)
    D = scref.sref.query_matrix(cref.densify(csrX), cref.densify(csrQ), "l2")
    return csrX, csrQ, graph, seeds, ds, D, dense_pair(rp, ctx, csrX, csrQ)


@pytest.mark.parametrize("k,ef", [(1, 1), (1, 256), (64, 64), (64, 256)])
def test_piece_and_cap_edges(rp, ctx, edge_case, k, ef):
    csrX, csrQ, graph, seeds, ds, D, dense = edge_case
    all_ways(rp, ctx, graph, ds, csrX, csrQ, k, ef, seeds, "edges k %d ef %d" % (k, ef), D=D, dense=dense)


# ---------------------------------------------------------------- 3: awkward values
def awkward_rows(d, dtype):
    """the awkward rows of test_gpu_knn_graph_csr.py (empty rows, duplicates, a full row, stored +0.0
    and -0.0, only column 0, only column d - 1, rows x 10) with an inf and a NaN entry planted"""
    from test_gpu_knn_graph_csr import awkward_rows as base
    csr, empty = base(d, dtype)
    rows = cref.rows_of(csr)
    full = np.arange(d, dtype=np.int32)
    rng = np.random.default_rng(100 + d)
    vi, vn = rng.standard_normal(d).astype(NP[dtype]), rng.standard_normal(d).astype(NP[dtype])
    vi[0], vn[d - 1] = np.inf, np.nan
    rows[40], rows[41] = (full, vi), (full, vn)
    return cref.from_rows(rows, d, NP[dtype]), rows


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("d", [33, 32, 1])
def test_awkward_values(rp, ctx, d, dtype):
    csrX, rows = awkward_rows(d, dtype)
    n, k, ef = len(rows), 10, 32
    rng = np.random.default_rng(d)
    qrows = [(c.copy(), v.copy()) for c, v in cref.rows_of(cref.make_csr(50 + d, 24, d, 0.3, NP[dtype]))]
    full = np.arange(d, dtype=np.int32)
    qrows[0] = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=NP[dtype]))    # empty
    qrows[1] = rows[17]                                      # a stored row: its duplicates 7 and 590 follow by id
    qrows[2] = (full, np.concatenate([[np.inf], rng.standard_normal(d - 1)]).astype(NP[dtype]))
    qrows[3] = (full, np.concatenate([rng.standard_normal(d - 1), [np.nan]]).astype(NP[dtype]))
    qrows[4] = (np.array([0], dtype=np.int32), np.array([-0.0], dtype=NP[dtype]))   # nothing but a stored zero
    qrows[5] = rows[20]                                      # the row of stored +0.0 and -0.0
    qrows[6] = rows[40]                                      # the stored inf row: inf - inf is NaN against itself
    csrQ = cref.from_rows(qrows, d, NP[dtype])
    graph = ring_graph(n, 7, rng)
    seeds = rng.integers(0, n, size=(24, 4)).astype(np.int32)
    seeds[1] = [17, 590, 7, 3]
    seeds[0, 0], seeds[4, 0] = 41, 40                        # the NaN row and the inf row are offered
    ds = rp.Dataset.csr(ctx, *csrX)
    want, exp, offered, upper = scref.graph_search_csr_ref(csrX, csrQ, graph[0], graph[1], seeds, k, ef)
    for stream in (0, 1):
        with option(ctx, "graph_search_csr_stream", stream):
            got, stats = search(rp, ctx, graph, ds, csrQ, k, ef, seeds)
        scref.assert_same_answer(got, want, "awkward d %d %s stream %d" % (d, dtype, stream))
        assert stats[0] == exp and offered <= stats[1] <= upper
    if d > 1:
        assert got[0][1, :3].tolist() == [7, 17, 590] and np.all(got[1][1, :3] == 0.0)
    assert np.all(np.isnan(got[1][3, :got[2][3]])) and got[2][3] == k
    assert np.array_equal(np.sort(got[0][3]), got[0][3])    # NaN distances rank by id


# ---------------------------------------------------------------- 4: a query above any possible cap
def test_queries_above_any_resident_cap(rp, ctx):
    """d = 20 000: 400 rows of 12 nonzeros around five centres and one of 5 000; queries of 12,
    2 048, 2 049, 3 000 and 5 000 nonzeros.  5 000 entries x 12 B x 4 waves exceed the LDS, so the
    streamed path is certain for the long ones; 2 048 / 2 049 straddle the resident cap"""
    n, d, nnz, k, ef = 400, 20000, 12, 8, 24
    rng = np.random.default_rng(3)
    centres = np.array([40, 5000, 5100, 12345, d - 40])

    def short_row():
        c = rng.choice(centres, size=3, replace=False)
        cols = np.unique(np.clip(np.concatenate([cc + rng.integers(-40, 40, size=nnz) for cc in c]), 0, d - 1))
        return np.sort(rng.choice(cols, size=nnz, replace=False)).astype(np.int32), rng.standard_normal(nnz)

    def long_row(m):
        return np.sort(rng.choice(d, size=m, replace=False)).astype(np.int32), rng.standard_normal(m)

    rows = [short_row() for _ in range(n)]
    rows[123] = long_row(5000)
    qrows = [short_row() for _ in range(4)] + [long_row(m) for m in (2048, 2049, 3000, 5000)] + [rows[123], rows[7]]
    csrX, csrQ = cref.from_rows(rows, d), cref.from_rows(qrows, d)
    graph = ring_graph(n, 6, rng)
    graph[0][::50, 0] = 123                                  # the long row is reached
    seeds = rng.integers(0, n, size=(len(qrows), 3)).astype(np.int32)
    seeds[8] = [123, 122, 5]
    ds = rp.Dataset.csr(ctx, *csrX)
    got = all_ways(rp, ctx, graph, ds, csrX, csrQ, k, ef, seeds, "d 20000")
    assert got[0][8, 0] == 123 and got[1][8, 0] == 0.0


# ---------------------------------------------------------------- 5: the complete graph
def test_complete_graph_gives_the_brute_force_answer(rp, ctx):
    """n = 65, every row lists all others (kg = 64: a full wave of candidates per offer), ef = 256,
    one seed: the beam ends up holding every point"""
    n, d, k, nq = 65, 40, 10, 16
    csrX = cref.make_csr(65, n, d, 0.25, empty=(9,))
    rows = cref.rows_of(csrX)
    rows[11] = rows[40]
    csrX = cref.from_rows(rows, d)
    csrQ = cref.from_rows(rows[:8] + cref.rows_of(cref.make_csr(66, 8, d, 0.25)), d)
    gids = np.array([[j for j in range(n) if j != i] for i in range(n)], dtype=np.int32)
    gcnt = np.full(n, n - 1, dtype=np.int32)
    seeds = np.random.default_rng(60).integers(0, n, size=(nq, 1)).astype(np.int32)
    ds = rp.Dataset.csr(ctx, *csrX)
    got, (exp, evaluated) = search(rp, ctx, (gids, gcnt), ds, csrQ, k, 256, seeds)
    want, w_exp, offered, upper = scref.graph_search_csr_ref(csrX, csrQ, gids, gcnt, seeds, k, 256)
    scref.assert_same_answer(got, want, "restatement")
    bi, bd = rp.bruteKnn(ds, csrQ, k)
    assert np.array_equal(got[0], bi) and np.all(got[2] == k)
    assert exp == w_exp == nq * n and offered == evaluated == nq * n


# ---------------------------------------------------------------- 6: degenerate sizes
def test_no_queries_no_points_one_point_and_no_seeds(rp, ctx):
    d = 8
    csrX = cref.make_csr(1, 50, d, 0.4)
    ds = rp.Dataset.csr(ctx, *csrX)
    graph = ring_graph(50, 3)
    none = cref.from_rows([], d)
    ids, dist, cnt = rp.graphSearchSV(graph, ds, none, 5, seeds=np.zeros((0, 2), dtype=np.int32))
    assert ids.shape == (0, 5) and dist.shape == (0, 5) and cnt.shape == (0,)
    assert rp.graphSearchLast(ctx) == (0, 0)
    csrQ = cref.make_csr(2, 4, d, 0.4)
    got = rp.graphSearchSV(graph, ds, csrQ, 5, seeds=np.full((4, 3), -1, dtype=np.int32))
    assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
    assert rp.graphSearchLast(ctx) == (0, 0)
    # n = 1
    one_csr = cref.from_rows(cref.rows_of(csrX)[:1], d)
    one = rp.Dataset.csr(ctx, *one_csr)
    g1 = (np.full((1, 2), -1, dtype=np.int32), np.zeros(1, dtype=np.int32))
    seeds = np.array([[0], [-1], [0], [0]], dtype=np.int32)
    got = rp.graphSearchSV(g1, one, csrQ, 3, ef=3, seeds=seeds)
    scref.assert_same_answer(got, scref.graph_search_csr_ref(one_csr, csrQ, g1[0], g1[1], seeds, 3, 3)[0], "n = 1")
    assert got[2].tolist() == [1, 0, 1, 1] and rp.graphSearchLast(ctx) == (3, 3)
    # n = 0: every count is 0
    empty = rp.Dataset.csr(ctx, *none)
    g0 = (np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int32))
    got = rp.graphSearchSV(g0, empty, csrQ, 3, seeds=np.full((4, 2), -1, dtype=np.int32))
    assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
    # rows and queries without nonzeros only
    zeros = cref.make_csr(3, 20, d, 0.0)
    zq = cref.make_csr(4, 3, d, 0.0)
    assert zeros[0][-1] == 0 and zq[0][-1] == 0
    gz = ring_graph(20, 3)
    sz = np.array([[4], [9], [19]], dtype=np.int32)
    got = rp.graphSearchSV(gz, rp.Dataset.csr(ctx, *zeros), zq, 5, ef=8, seeds=sz)
    scref.assert_same_answer(got, scref.graph_search_csr_ref(zeros, zq, gz[0], gz[1], sz, 5, 8)[0], "no nonzeros")
    assert np.all(got[1] == 0.0) and np.all(got[2] == 5)


def test_seed_with_an_empty_row_and_disconnected_halves(rp, ctx):
    n, d, k = 40, 12, 10
    csrX = cref.make_csr(2, n, d, 0.4)
    ds = rp.Dataset.csr(ctx, *csrX)
    # half A = ids 0 .. 5 (smaller than k), half B = the rest; graph rows 3 and 20 are empty
    gids = np.full((n, 6), -1, dtype=np.int32)
    gcnt = np.zeros(n, dtype=np.int32)
    for i in range(n):
        half = [j for j in (range(6) if i < 6 else range(6, n)) if j != i]
        row = half[:5] if i < 6 else [half[(i + e) % len(half)] for e in range(6)]
        row = sorted(set(row))
        gids[i, :len(row)], gcnt[i] = row, len(row)
    gcnt[3] = 0
    gcnt[20] = 0
    rows = cref.rows_of(csrX)
    csrQ = cref.from_rows([(rows[i][0], rows[i][1] + 0.05) for i in (0, 1, 2, 30, 31, 32)], d)
    seeds = np.array([[3, -1], [3, 4], [0, 0], [20, -1], [20, 21], [39, 7]], dtype=np.int32)
    got, stats = search(rp, ctx, (gids, gcnt), ds, csrQ, k, 16, seeds)
    want, exp, offered, upper = scref.graph_search_csr_ref(csrX, csrQ, gids, gcnt, seeds, k, 16)
    scref.assert_same_answer(got, want, "halves")
    assert stats[0] == exp and offered <= stats[1] <= upper
    assert got[2].tolist() == [1, 6, 6, 1, 10, 10]          # an empty row leads nowhere; A holds 6 points
    assert got[0][0, 0] == 3 and got[0][3, 0] == 20
    for i in range(6):
        c = got[2][i]
        assert np.all(got[0][i, :c] < 6) if i < 3 else np.all(got[0][i, :c] >= 6)
    check_padding(got, k)


# ---------------------------------------------------------------- 7: determinism, device arrays
def test_two_calls_and_the_dev_entry_point_give_the_same_bits(rp, ctx):
    import torch
    n, d, kg, k, ef, s, nq = 2500, 64, 10, 10, 48, 6, 100
    csrX = cref.make_csr(13, n, d, 0.2)
    csrQ = cref.make_csr(14, nq, d, 0.2)
    f = build(rp, ctx, csrX, 50, 3, seed=8)
    ds = f.data
    graph = rp.knnGraphSV(kg, f)
    rng = np.random.default_rng(5)
    seeds = rng.integers(0, n, size=(nq, s)).astype(np.int32)
    a, sa = search(rp, ctx, graph, ds, csrQ, k, ef, seeds)
    b, sb = search(rp, ctx, graph, ds, csrQ, k, ef, seeds)
    scref.assert_same_answer(a, b, "second call")
    assert sa == sb
    dev = torch.device("cuda", ctx.device)
    tx = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in csrX[:3]]
    tq = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in csrQ[:3]]
    dx = rp.Dataset.csr_from_torch(ctx, tx[0], tx[1], tx[2], d)
    dq = rp.Dataset.csr_from_torch(ctx, tq[0], tq[1], tq[2], d)

    def on_device(gids, gcnt, sd):
        tg, tc, ts = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (gids, gcnt, sd))
        ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
        dist = torch.empty((nq, k), dtype=torch.float64, device=dev)
        cnt = torch.empty(nq, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        rp.graphSearchSVDev(dx, dq, kg, tg.data_ptr(), tc.data_ptr(), s, ts.data_ptr(), k, ef, ids.data_ptr(),
                            dist.data_ptr(), cnt.data_ptr())
        ctx.sync()
        return (ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy()), rp.graphSearchLast(ctx)

    c, sc = on_device(graph[0], graph[2], seeds)
    scref.assert_same_answer(c, a, "dev against host")
    assert sc == sa
    # _dev does not validate: ids and seeds outside [0, n) and a count outside [0, kg] are skipped
    gids, gcnt, bad_seeds = np.array(graph[0]), np.array(graph[2]), seeds.copy()
    gids[int(a[0][0, 0]), 1] = n + 5                       # rows that the searches do reach
    gids[int(a[0][1, 0]), 0] = -7
    gcnt[int(a[0][2, 0])] = kg + 3
    gcnt[int(a[0][3, 0])] = -2
    gids[17, 0] = 2 ** 31 - 1
    bad_seeds[4, 0], bad_seeds[5, 1], bad_seeds[6, 2] = n, -9, 2 ** 31 - 1
    got, sg = on_device(gids, gcnt, bad_seeds)
    want, exp, offered, upper = scref.graph_search_csr_ref(csrX, csrQ, gids, gcnt, bad_seeds, k, ef)
    scref.assert_same_answer(got, want, "planted graph")
    assert sg[0] == exp and offered <= sg[1] <= upper
    clean_ids, clean_cnt = np.full_like(gids, -1), np.zeros_like(gcnt)
    for i in range(n):                                     # the cleaned arrays: what is skipped, removed
        row = [v for v in gids[i, :gcnt[i]].tolist() if 0 <= v < n] if 0 <= gcnt[i] <= kg else []
        clean_ids[i, :len(row)], clean_cnt[i] = row, len(row)
    clean_seeds = np.where((bad_seeds >= 0) & (bad_seeds < n), bad_seeds, -1)
    want2 = scref.graph_search_csr_ref(csrX, csrQ, clean_ids, clean_cnt, clean_seeds, k, ef)
    scref.assert_same_answer(got, want2[0], "cleaned arrays")
    assert want2[1] == exp


# ---------------------------------------------------------------- 8: refusals
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, kg, k, s, nq = 1500, 16, 10, 10, 4, 16
    csrX = cref.make_csr(12, n, d, 0.3)
    csrQ = cref.make_csr(13, nq, d, 0.3)
    f = build(rp, ctx, csrX, 30, 4, seed=7)
    ds = f.data
    qd = rp.Dataset.csr(ctx, *csrQ)
    graph = rp.knnGraphSV(kg, f)
    seeds0 = np.random.default_rng(3).integers(0, n, size=(nq, s)).astype(np.int32)
    before = rp.knnBatch(k, f, csrQ)
    cand0 = C.c_int64(-1)
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(cand0)))
    good = rp.graphSearchSV(graph, ds, qd, k, ef=32, seeds=seeds0)
    stats = rp.graphSearchLast(ctx)
    scref.assert_same_answer(good, scref.graph_search_csr_ref(csrX, csrQ, graph[0], graph[2], seeds0, k, 32)[0],
                             "before the refusals")
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(code, data=ds, queries=qd, kg_=kg, s_=s, k_=k, ef_=32, metric=0, flags=0, gids=None, gcnt=None,
                seeds=None, entry=None):
        gids = np.ascontiguousarray(graph[0] if gids is None else gids, dtype=np.int32)
        gcnt = np.ascontiguousarray(graph[2] if gcnt is None else gcnt, dtype=np.int32)
        seeds = np.ascontiguousarray(seeds0 if seeds is None else seeds, dtype=np.int32)
        ids = np.full((nq, 64), 12345, dtype=np.int32)
        dist = np.full((nq, 64), 0.5)
        cnt = np.full(nq, 77, dtype=np.int32)
        st = (entry or L.rpt_graph_search_csr_host)(
            ctx._h, data._h, queries._h, kg_, C.c_void_p(gids.ctypes.data), C.c_void_p(gcnt.ctypes.data), s_,
            C.c_void_p(seeds.ctypes.data), k_, ef_, metric, flags, C.c_void_p(ids.ctypes.data),
            C.c_void_p(dist.ctypes.data), C.c_void_p(cnt.ctypes.data))
        assert st == code, (st, code)
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77)   # nothing was written
        assert rp.graphSearchLast(ctx) == stats            # nothing was launched
        return msg

    dense = rp.Dataset.dense(ctx, cref.densify(csrX))
    qdense = rp.Dataset.dense(ctx, cref.densify(csrQ))
    assert "rpt_graph_search_*" in refused(RPT_E_ARG, data=dense, queries=qdense)   # names the dense entry point
    assert "both" in refused(RPT_E_ARG, queries=qdense)
    assert "both" in refused(RPT_E_ARG, data=dense)
    q_d = rp.Dataset.csr(ctx, csrQ[0], csrQ[1], csrQ[2], d + 1)
    assert "d or dtype" in refused(RPT_E_ARG, queries=q_d)
    q_32 = rp.Dataset.csr(ctx, csrQ[0], csrQ[1], csrQ[2].astype(np.float32), d)
    assert "d or dtype" in refused(RPT_E_ARG, queries=q_32)
    assert "kg" in refused(RPT_E_ARG, kg_=0)
    assert "kg" in refused(RPT_E_ARG, kg_=65)
    assert "s " in refused(RPT_E_ARG, s_=0)
    assert "s " in refused(RPT_E_ARG, s_=65)
    assert "k" in refused(RPT_E_ARG, k_=0)
    assert "k" in refused(RPT_E_ARG, k_=65, ef_=100)
    assert "ef" in refused(RPT_E_ARG, k_=10, ef_=9)
    assert "ef" in refused(RPT_E_ARG, ef_=257)
    assert "flags" in refused(RPT_E_ARG, flags=1)
    assert "flags" in refused(RPT_E_ARG, flags=COS)
    for m in (COS, INN):
        assert "metric" in refused(RPT_E_UNSUPPORTED, metric=m)
    for m in (COS | INN, REF, 2, INN | 1):
        assert "metric" in refused(RPT_E_ARG, metric=m)
    # _host names the row of the graph or of the seeds that is out of range, before any upload
    bad = np.array(graph[2])
    bad[700] = kg + 1
    assert "graph row 700" in refused(RPT_E_ARG, gcnt=bad)
    bad[700] = -1
    assert "graph row 700" in refused(RPT_E_ARG, gcnt=bad)
    bad = np.array(graph[0])
    bad[701, 0] = n
    assert graph[2][701] > 0 and "graph row 701" in refused(RPT_E_ARG, gids=bad)
    bad = seeds0.copy()
    bad[5, 2] = n
    assert "seeds row 5" in refused(RPT_E_ARG, seeds=bad)
    bad[5, 2] = -2
    assert "seeds row 5" in refused(RPT_E_ARG, seeds=bad)
    # the dense entry point keeps refusing CSR data
    for m in (0, COS, INN):
        assert "CSR" in refused(RPT_E_UNSUPPORTED, metric=m, entry=L.rpt_graph_search_host)
    with pytest.raises(rp.RPTError) as e:
        rp.graphSearchSV(graph, ds, qd, k, ef=5, seeds=seeds0)
    assert e.value.code == RPT_E_ARG
    with pytest.raises(ValueError):
        rp.graphSearchSV(graph, ds, qd, k)                  # neither seeds nor a forest
    # after the refusals: the same answer, and the kNN entry points answer as before
    again = rp.graphSearchSV(graph, ds, qd, k, ef=32, seeds=seeds0)
    scref.assert_same_answer(again, good, "after the refusals")
    assert rp.graphSearchLast(ctx) == stats
    cand = C.c_int64(-1)
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(cand)))
    assert cand.value == cand0.value
    for x, y in zip(before, rp.knnBatch(k, f, csrQ)):
        assert np.array_equal(x, y, equal_nan=True)


# ---------------------------------------------------------------- 9: seeds from a forest
def test_seeds_from_a_forest(rp, ctx):
    n, d, kg, k = 3000, 32, 10, 10
    csrX = cref.make_csr(21, n, d, 0.3, np.float32)
    f = build(rp, ctx, csrX, 60, 2, seed=9)
    graph = rp.knnGraphRefineSV(rp.knnGraphSV(kg, f), f, iters=1)
    rng = np.random.default_rng(8)
    rows = cref.rows_of(csrX)
    csrQ = cref.from_rows([(rows[i][0], (rows[i][1] + 0.2 * rng.standard_normal(len(rows[i][1]))).astype(np.float32))
                           for i in rng.choice(n, 50)], d, np.float32)
    got = rp.graphSearchSV(graph, f, csrQ, k, ef=32, forest=f, seed_k=8)
    stats = rp.graphSearchLast(ctx)
    sid, _, scnt = rp.knnBatch(8, f, csrQ, dedup=True)
    seeds = np.where(np.arange(8)[None, :] < scnt[:, None], sid, -1).astype(np.int32)
    want = rp.graphSearchSV(graph, f.data, csrQ, k, ef=32, seeds=seeds)
    scref.assert_same_answer(got, want, "forest seeds")
    assert rp.graphSearchLast(ctx) == stats
    D = scref.sref.query_matrix(cref.densify(csrX), cref.densify(csrQ), "l2")
    model, exp, offered, upper = scref.graph_search_csr_ref(csrX, csrQ, graph[0], graph[2], seeds, k, 32, D=D)
    scref.assert_same_answer(got, model, "restatement")
    assert stats[0] == exp and offered <= stats[1] <= upper
    for i in range(50):                                     # no worse than the seeds alone: 8 seeds at the most,
        sd = np.sort(D[i, seeds[i][seeds[i] >= 0]])         # so the m-th with m = min(k, valid seeds)
        m = min(k, len(sd))
        assert m > 0 and got[2][i] >= m and got[1][i, m - 1] <= sd[m - 1]
    # ef = None means max(k, 32); SVectors as queries
    scref.assert_same_answer(rp.graphSearchSV(graph, f, csrQ, k, seeds=seeds), want, "default ef")
    svs = [rp.SVector(d, c, v) for c, v in cref.rows_of(csrQ)[:5]]
    few = rp.graphSearchSV(graph, f, svs, k, ef=32, seeds=seeds[:5])
    scref.assert_same_answer(few, tuple(x[:5] for x in want), "SVector queries")


# ---------------------------------------------------------------- 10: the profile class
def test_prof_class_3_times_the_call(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    csrX = cref.make_csr(14, 1000, 16, 0.3)
    f = build(rp, ctx, csrX, 40, 2, seed=3)
    csrQ = cref.make_csr(15, 20, 16, 0.3)
    rp.knnBatch(5, f, csrQ)
    cand0 = C.c_int64(-1)
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(cand0)))
    graph = ring_graph(1000, 5)
    seeds = np.arange(40, dtype=np.int32).reshape(20, 2)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        _lib.check(L.rpt_prof_reset(ctx._h))
        rp.graphSearchSV(graph, f.data, csrQ, 5, ef=8, seeds=seeds)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
        assert cnt.value == 1 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))
    cand = C.c_int64(-1)
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(cand)))
    assert cand.value == cand0.value and cand.value > 0


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_example(tmp_path):
    """host/example_graph_search_sparse.cpp folds every reported distance again on the host over the
    union of the two supports and compares the bits"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "example_graph_search_sparse")
    src = os.path.join(root, "rp-tree_amd", "host", "example_graph_search_sparse.cpp")
    lib = os.path.join(root, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "1200", "40", "60", "0.2", "3", "40", "8", "1", "5", "16"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[-2].startswith("recall@5 ") and lines[0].startswith("query 0:")
