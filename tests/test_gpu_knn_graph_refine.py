"""NN-descent rounds over a kNN graph on the device (rpt_knn_graph_refine_host / _dev,
csrc/graph_refine.hip): ids, counts and distance BITS, and the statistics of the call, against the
numpy restatement of the definition in tests/knn_graph_refine_ref.py."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_graph_ref as ref  # noqa: E402
import knn_graph_refine_ref as rref  # noqa: E402

RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4


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


def make_rows(seed, n, d):
    """the recipe of test_gpu_knn_graph.py: finite rows with exact duplicates under other ids, a
    zero row and rows scaled x10"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    if n > 40:
        X[5] = X[17]
        X[n - 3] = X[17]
        X[31] = X[30]
        X[9] = 0.0
        X[20:28] *= 10.0
    return X


def as_dtype(rp, ctx, X, dtype):
    """-> (Dataset, the rows as the exactly widened doubles)"""
    if dtype == "f64":
        return rp.Dataset.dense(ctx, X), X
    if dtype == "f32":
        X32 = X.astype(np.float32)
        return rp.Dataset.dense(ctx, X32), X32.astype(np.float64)
    u = rp.to_bf16(X)
    return rp.Dataset.dense(ctx, u, dtype=rp.RPT_BF16), rp.from_bf16(u).astype(np.float64)


def leaves_of(f):
    return ref.leaf_slices(f.topology())


def hand_graph(X64, k, rows):
    """a graph from {i: member ids}: the fold distances, rows sorted by (distance, id)"""
    n = X64.shape[0]
    ids = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), np.inf)
    cnt = np.zeros(n, dtype=np.int32)
    for i, members in rows.items():
        m = np.array(sorted(set(members) - {i}), dtype=np.int32)
        dv = ref.fold_dist(X64[i], X64[m])
        o = np.lexsort((m, dv))[:k]
        ids[i, :len(o)], dist[i, :len(o)], cnt[i] = m[o], dv[o], len(o)
    return ids, dist, cnt


def check_against_ref(rp, ctx, ds, X64, g0, k, reverse, iters, tag, want=None, D=None):
    """the call under both kernel shapes against the restatement -> the device's graph"""
    if want is None:
        want = rref.refine_ref(X64, g0, k, reverse, iters, D)
    before = tuple(np.array(a) for a in g0)
    got = rp.knnGraphRefine(g0, ds, iters=iters, reverse=reverse)
    stats = rp.knnGraphRefineLast(ctx)
    for a, b in zip(before, g0):                           # the input tuple is not modified
        assert np.array_equal(a, b, equal_nan=True)
    ref.assert_same_graph(got, want[0], tag)
    print("%s: (rounds, updates, candidates) device %s restatement %s" % (tag, stats, want[1:]))
    assert stats == tuple(want[1:]), tag
    with option(ctx, "graph_refine_general", 1):
        gen = rp.knnGraphRefine(g0, ds, iters=iters, reverse=reverse)
        assert rp.knnGraphRefineLast(ctx) == stats
    ref.assert_same_graph(gen, got, tag + ", graph_refine_general")
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert np.all(got[0][pad] == -1) and np.all(np.isposinf(got[1][pad]))
    return got


# ---------------------------------------------------------------- the grid
_grid = {}


def grid_case(rp, ctx, dtype, d, k, reverse):
    """data set, forest graph and the restatement's first three rounds, built once per case"""
    key = (dtype, d, k, reverse)
    if key not in _grid:
        n, T, minl = 1500, 3, 40
        dkey = (dtype, d)
        if dkey not in _grid:
            ds, X64 = as_dtype(rp, ctx, make_rows(d, n, d), dtype)
            cfg = rp.rpTreeCfg(minl, n, d)
            f = rp.forestBatch(1234 + d, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
            _grid[dkey] = (ds, X64, f, rref.fold_matrix(X64))
        ds, X64, f, D = _grid[dkey]
        g0 = rp.knnGraph(k, f)
        ref.assert_same_graph(g0, ref.knn_graph_ref(X64, f.perm, leaves_of(f), k), "the forest's graph")
        rounds, g, tot, u = [], g0, [0, 0, 0], 1
        for _ in range(3):
            if u > 0:                                      # behind a round without updates nothing is applied
                g, r1, u, c = rref.refine_ref(X64, g, k, reverse, 1, D)
                tot = [tot[0] + r1, tot[1] + u, tot[2] + c]
            rounds.append((g,) + tuple(tot))
        _grid[key] = (ds, X64, g0, rounds)
    return _grid[key]


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("k,reverse", [(1, 0), (10, 10), (10, 3), (64, 64)])
@pytest.mark.parametrize("d", [24, 128, 200])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_refine_matches_the_definition(rp, ctx, dtype, d, k, reverse, iters):
    ds, X64, g0, rounds = grid_case(rp, ctx, dtype, d, k, reverse)
    got = check_against_ref(rp, ctx, ds, X64, g0, k, reverse, iters,
                            "%s d %d k %d r %d iters %d" % (dtype, d, k, reverse, iters), want=rounds[iters - 1])
    for i in range(X64.shape[0]):                          # never its own neighbour
        assert i not in got[0][i]


def test_two_calls_give_the_same_bits(rp, ctx):
    """the reverse lists are filled through an atomic cursor: their selection must not show it"""
    n, d, k = 3000, 32, 10
    ds, X64 = as_dtype(rp, ctx, make_rows(77, n, d), "f64")
    f = rp.forestBatch(5, 6, 60, 3, 0.5, d, ds, ctx=ctx)
    g0 = rp.knnGraph(k, f)
    a = rp.knnGraphRefine(g0, ds, iters=2, reverse=4)      # reverse < in-degree of many points
    sa = rp.knnGraphRefineLast(ctx)
    b = rp.knnGraphRefine(g0, f, iters=2, reverse=4)       # a forest stands for its data set
    assert rp.knnGraphRefineLast(ctx) == sa
    ref.assert_same_graph(a, b, "second call")
    want = rref.refine_ref(X64, g0, k, 4, 2)
    ref.assert_same_graph(a, want[0], "reverse 4")
    assert sa == tuple(want[1:])


# ---------------------------------------------------------------- short rows, tiny inputs, NaN
def test_short_and_empty_rows(rp, ctx):
    n, d, k = 700, 24, 5
    X = make_rows(n, n, d)
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(77, 12, 2, 1, 0.5, d, ds, ctx=ctx)  # leaves of one and two points
    g0 = rp.knnGraph(k, f)
    assert (g0[2] == 0).any() and (g0[2] == 1).any() and g0[2].max() < k
    for reverse, iters in ((0, 1), (5, 2), (2, 3)):
        check_against_ref(rp, ctx, ds, X, g0, k, reverse, iters, "tiny leaves r %d" % reverse)
    empty = (np.full((n, k), -1, dtype=np.int32), np.full((n, k), np.inf), np.zeros(n, dtype=np.int32))
    got = check_against_ref(rp, ctx, ds, X, empty, k, 5, 3, "empty graph")
    assert rp.knnGraphRefineLast(ctx) == (1, 0, 0) and np.all(got[2] == 0)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_data_sets(rp, ctx, n):
    d, k = 8, 3
    X = np.random.default_rng(n).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    g0 = hand_graph(X, k, {0: [1]} if n == 2 else {})
    got = rp.knnGraphRefine(g0, ds, iters=4)
    want = rref.refine_ref(X, g0, k, k, 4)
    ref.assert_same_graph(got, want[0], "n %d" % n)
    assert got[0].shape == (n, k) and rp.knnGraphRefineLast(ctx) == tuple(want[1:])
    if n == 2:                                             # the reverse neighbour completes row 1
        assert got[0][1, 0] == 0 and got[2].tolist() == [1, 1] and want[1] == 2


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nan_row_ranks_last_by_id(rp, ctx, dtype):
    n, d, k = 300, 24, 10
    X = make_rows(3, n, d)
    X[44, 7] = np.nan
    ds, X64 = as_dtype(rp, ctx, X, dtype)
    f = rp.forestBatch(5, 0, 10, 2, 0.5, d, ds, ctx=ctx)   # depth 0 projects nothing: NaN rows are allowed
    full = rp.knnGraph(k, f)
    assert np.all(np.isnan(full[1][44])) and full[0][44].tolist() == list(range(k))
    # the exact graph is a fixed point of the refinement
    check_against_ref(rp, ctx, ds, X64, full, k, k, 2, "depth 0 graph")
    # a sparse start: row 44 knows two far ids, the others a ring; the NaN row's list fills up by id
    rows = {i: [(i + 1) % n, (i + 7) % n] for i in range(n)}
    rows[44] = [250, 260]
    g0 = hand_graph(X64, k, rows)
    got = check_against_ref(rp, ctx, ds, X64, g0, k, k, 3, "ring with a NaN row")
    c = got[2][44]
    assert np.all(np.isnan(got[1][44, :c])) and got[0][44, :c].tolist() == sorted(got[0][44, :c].tolist())
    for i in [j for j in range(n) if 44 in got[0][j]]:     # NaN behind every number
        row = got[1][i, :got[2][i]]
        assert np.isnan(row[-1]) and not np.isnan(row[:-1]).any()


# ---------------------------------------------------------------- wide ties
def test_wide_ties_enter_by_id(rp, ctx):
    """the permuted-integer rows of test_wide_ties_order_by_id: 45 ids at exactly the same distance
    from the origin reach it through five far neighbours in one round; the first k by id stay"""
    k, d, m = 10, 24, 45
    rng = np.random.default_rng(8)
    base = np.zeros(d)
    base[:6] = [3, 1, 2, 5, 4, 7]
    rows = {tuple(rng.permutation(base)) for _ in range(4 * m)}
    tied = np.array(sorted(rows))[:m]
    assert len(tied) == m
    far = 50.0 + rng.standard_normal((30, d))
    X = np.concatenate([np.zeros((1, d)), far[:10], tied, far[10:]])
    order = rng.permutation(len(X))
    X = X[order]
    origin = int(np.nonzero(order == 0)[0][0])
    tied_ids = np.sort(np.nonzero((order >= 11) & (order < 11 + m))[0])
    far_ids = np.nonzero((order >= 1) & (order < 11))[0][:5]
    assert len(np.unique(ref.bits(ref.fold_dist(X[origin], X[tied_ids])))) == 1 and m > 3 * k
    graph = {origin: far_ids.tolist()}
    for a, fid in enumerate(far_ids):
        graph[int(fid)] = tied_ids[9 * a:9 * a + 9].tolist()
    ds = rp.Dataset.dense(ctx, X)
    g0 = hand_graph(X, k, graph)
    got = check_against_ref(rp, ctx, ds, X, g0, k, 0, 1, "ties")
    assert got[0][origin].tolist() == tied_ids[:k].tolist()
    got = check_against_ref(rp, ctx, ds, X, g0, k, k, 2, "ties, reverse")
    assert got[0][origin].tolist() == tied_ids[:k].tolist()


# ---------------------------------------------------------------- fixed point, both parities
def _ring(X, k):
    n = X.shape[0]
    return hand_graph(X, k, {i: [(i + 1) % n, (i + 2) % n] for i in range(n)})


def test_fixed_point_after_an_even_and_an_odd_number_of_rounds(rp, ctx):
    n, d, k = 120, 6, 4
    X = np.random.default_rng(1).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    g0 = _ring(X, k)
    parities = set()
    for reverse in (4, 0):
        want = rref.refine_ref(X, g0, k, reverse, 50)
        assert 1 < want[1] < 50
        parities.add(want[1] % 2)
        got = check_against_ref(rp, ctx, ds, X, g0, k, reverse, 50, "fixed point r %d" % reverse, want=want)
        again = rp.knnGraphRefine(got, ds, iters=1, reverse=reverse)
        assert rp.knnGraphRefineLast(ctx)[:2] == (1, 0)
        ref.assert_same_graph(again, got, "one more call")
        # stopping short of the round that changes nothing: the other parity of applied rounds
        short = rref.refine_ref(X, g0, k, reverse, want[1] - 1)
        assert short[1] == want[1] - 1
        check_against_ref(rp, ctx, ds, X, g0, k, reverse, want[1] - 1, "short r %d" % reverse, want=short)
    assert parities == {0, 1}, parities


# ---------------------------------------------------------------- accumulate keeps a refined graph
@pytest.mark.parametrize("iters", [1, 4])
def test_accumulating_the_forest_into_a_refined_graph_changes_nothing(rp, ctx, iters):
    n, d, k = 2000, 32, 10
    ds, X64 = as_dtype(rp, ctx, make_rows(2, n, d), "f32")
    cfg = rp.rpTreeCfg(50, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, 50, 4, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    refined = rp.knnGraphRefine(rp.knnGraph(k, f), f, iters=iters)
    ref.assert_same_graph(rp.knnGraph(k, f, accumulate=refined), refined, "accumulate")


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    n, d, T, minl, k = 1500, 16, 4, 30, 10
    X = np.random.default_rng(12).standard_normal((n, d))
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(7, 6, minl, T, 0.5, d, ds, ctx=ctx)
    g0 = rp.knnGraph(k, f)
    rp.knnGraphRefine(g0, ds)
    stats = rp.knnGraphRefineLast(ctx)

    def refused(code, data, kk, reverse, iters, flags, graph=g0):
        ids, dist, cnt = (np.array(a) for a in graph)
        keep = (ids.copy(), dist.copy(), cnt.copy())
        st = L.rpt_knn_graph_refine_host(ctx._h, data._h, kk, reverse, iters, flags, C.c_void_p(ids.ctypes.data),
                                         C.c_void_p(dist.ctypes.data), C.c_void_p(cnt.ctypes.data))
        assert st == code
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        for a, b in zip(keep, (ids, dist, cnt)):           # nothing was written
            assert np.array_equal(a, b)
        assert rp.knnGraphRefineLast(ctx) == stats         # nothing was launched
        return msg

    assert "k" in refused(RPT_E_ARG, ds, 0, 0, 1, 0)
    assert "k" in refused(RPT_E_ARG, ds, 65, 0, 1, 0)
    assert "reverse" in refused(RPT_E_ARG, ds, k, -1, 1, 0)
    assert "reverse" in refused(RPT_E_ARG, ds, k, 65, 1, 0)
    assert "iters" in refused(RPT_E_ARG, ds, k, k, 0, 0)
    assert "iters" in refused(RPT_E_ARG, ds, k, k, -2, 0)
    assert "flags" in refused(RPT_E_ARG, ds, k, k, 1, 1)
    for flag in (rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE):
        assert "metric" in refused(RPT_E_UNSUPPORTED, ds, k, k, 1, flag)
    rowptr = np.arange(n + 1, dtype=np.int64)
    csr = rp.Dataset.csr(ctx, rowptr, np.zeros(n, dtype=np.int32), np.ones(n), d)
    assert "CSR" in refused(RPT_E_UNSUPPORTED, csr, k, k, 1, 0)
    bad = tuple(np.array(a) for a in g0)
    bad[0][700, 2] = n
    assert "row 700" in refused(RPT_E_ARG, ds, k, k, 1, 0, bad)
    bad = tuple(np.array(a) for a in g0)
    bad[0][701, 0] = 701
    assert "row 701" in refused(RPT_E_ARG, ds, k, k, 1, 0, bad)
    bad = tuple(np.array(a) for a in g0)
    bad[2][702] = k + 1
    assert "row 702" in refused(RPT_E_ARG, ds, k, k, 1, 0, bad)
    bad = tuple(np.array(a) for a in g0)
    bad[0][703, 1] = bad[0][703, 0]
    assert "row 703" in refused(RPT_E_ARG, ds, k, k, 1, 0, bad)
    with pytest.raises(rp.RPTError) as e:
        rp.knnGraphRefine(g0, ds, iters=0)
    assert e.value.code == RPT_E_ARG

    # the context answers a knnGraph call right after
    ref.assert_same_graph(rp.knnGraph(k, f), ref.knn_graph_ref(X, f.perm, leaves_of(f), k), "after the refusals")


# ---------------------------------------------------------------- device arrays
@pytest.mark.parametrize("dtype", ["f64", "bf16"])
def test_dev_entry_point_with_torch_tensors(rp, ctx, dtype):
    import torch
    n, d, T, minl, k = 2500, 64, 3, 50, 10
    X = make_rows(13, n, d)
    dev = torch.device("cuda", ctx.device)
    t = torch.from_numpy(X).to(dev) if dtype == "f64" else torch.from_numpy(X).to(dev).to(torch.bfloat16)
    ds = rp.Dataset.from_torch(ctx, t)
    cfg = rp.rpTreeCfg(minl, n, d)
    f = rp.forestBatch(8, cfg.fpMaxTreeDepth, minl, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    g0 = rp.knnGraph(k, f)
    for iters, reverse in ((1, None), (2, 3), (3, 0)):
        ids = torch.from_numpy(g0[0]).to(dev)
        dist = torch.from_numpy(g0[1]).to(dev)
        cnt = torch.from_numpy(g0[2]).to(dev)
        torch.cuda.synchronize(dev)
        rp.knnGraphRefineDev(k, ds, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), iters=iters, reverse=reverse)
        ctx.sync()
        stats = rp.knnGraphRefineLast(ctx)
        got = (ids.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy())
        host = rp.knnGraphRefine(g0, ds, iters=iters, reverse=reverse)
        assert rp.knnGraphRefineLast(ctx) == stats and stats[0] == iters
        ref.assert_same_graph(got, host, "dev against host, iters %d" % iters)
    X64 = t.to(torch.float64).cpu().numpy()
    want = rref.refine_ref(X64, g0, k, 0, 3)
    ref.assert_same_graph(got, want[0], "dev")
    assert stats == tuple(want[1:])


def test_prof_class_3_times_the_call(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    X = make_rows(14, 1000, 16)
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(8, 4, 30, 3, 0.5, 16, ds, ctx=ctx)
    g0 = rp.knnGraph(5, f)
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        _lib.check(L.rpt_prof_reset(ctx._h))
        rp.knnGraphRefine(g0, ds, iters=2)
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(L.rpt_prof_get(ctx._h, 3, C.byref(ms), C.byref(cnt)))
        assert cnt.value == 1 and ms.value > 0.0
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_example(rp, ctx, tmp_path):
    n, d, T, minl, k, iters, reverse = 1200, 24, 3, 40, 8, 3, 5
    X = make_rows(15, n, d)
    data = tmp_path / "x.bin"
    data.write_bytes(np.array([n, d], dtype=np.int64).tobytes() + X.tobytes())
    exe = str(tmp_path / "example_knn_graph_refine")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_graph_refine.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = tmp_path / "graphs.bin"
    r = subprocess.run([exe, str(data), str(T), str(minl), str(k), str(iters), str(reverse), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok"
    raw = out.read_bytes()
    T2, L = np.frombuffer(raw[:8], dtype=np.int32)
    off = 8
    R = np.frombuffer(raw[off:off + T2 * L * d * 8], dtype=np.float64).reshape(T2, L, d)
    off += R.nbytes
    graphs = []
    for _ in range(2):
        ids = np.frombuffer(raw[off:off + n * k * 4], dtype=np.int32).reshape(n, k)
        off += ids.nbytes
        dist = np.frombuffer(raw[off:off + n * k * 8], dtype=np.float64).reshape(n, k)
        off += dist.nbytes
        cnt = np.frombuffer(raw[off:off + n * 4], dtype=np.int32)
        off += cnt.nbytes
        graphs.append((ids, dist, cnt))
    stats = tuple(int(v) for v in np.frombuffer(raw[off:off + 24], dtype=np.int64))
    # the same hyperplanes through the Python mirror: the same forest, the same graphs
    ds = rp.Dataset.dense(ctx, X)
    f = rp.forestBatch(0, int(L), minl, int(T2), 0.5, d, ds, ctx=ctx, hyperplanes=R)
    g0 = rp.knnGraph(k, f)
    ref.assert_same_graph(graphs[0], g0, "C++ example, the forest's graph")
    ref.assert_same_graph(graphs[1], rp.knnGraphRefine(g0, ds, iters=iters, reverse=reverse), "C++ example")
    assert rp.knnGraphRefineLast(ctx) == stats
    want = rref.refine_ref(X, g0, k, reverse, iters)
    ref.assert_same_graph(graphs[1], want[0], "C++ example, def")
    assert stats == tuple(want[1:])
