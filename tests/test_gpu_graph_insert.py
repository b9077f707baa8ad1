"""New rows into a kNN graph on the device (rpt_graph_insert_host / _dev; csrc/graph_insert.hip: the
chunk's searches through the existing launches, link_count / _scan / _fill / _merge_kernel): ids,
counts, distance BITS and the counters chunks / offered / accepted against the numpy restatement in
tests/graph_insert_ref.py, `evaluated` inside its defined bounds.  No tolerance anywhere.

The shapes are the smallest at which the kernels can still go wrong: 300 old and 100 new rows of the
golden sets, chunks that do not divide m, one chunk, a chunk larger than m, a hub that collects more
than two wave_merge pieces of offers, rows without a direction under cosine, and input rows that no
graph over the first n rows would hold."""
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
import knn_graph_metric_ref as mref  # noqa: E402
import graph_search_ref as sref  # noqa: E402
import graph_insert_ref as iref  # noqa: E402
import graph_metric_csr_ref as gm  # noqa: E402

RPT_E_ARG = -1
METRICS = ("l2", "cosine", "inner")
DENSE = ("f64", "f32", "bf16")
SPARSE = ("csr64", "csr32")
N_OLD, M_NEW = 300, 100


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
    return {"cosine": rp.metricCosine, "inner": rp.metricInner, "l2": rp.metricL2}[metric]


def golden_dense():
    return np.load(os.path.join(ROOT, "tests", "golden", "forest_dense_1000x16.npz"))["X"]


def golden_csr(rows):
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_sparse_600x12.npz"))
    rowptr = z["rowptr"][:rows + 1].astype(np.int64)
    return rowptr, z["col"][:rowptr[-1]].astype(np.int32), z["val"][:rowptr[-1]].astype(np.float64), int(z["d"])


def make_seeds(seed, n, m, s):
    """ids all over [0, N): old rows, rows of earlier chunks (followed) and of this or a later chunk
    (skipped); a repeated id per row, -1 padding in every third row, row 7 without a seed"""
    rng = np.random.default_rng(seed)
    seeds = rng.integers(0, n + m, size=(m, s)).astype(np.int32)
    seeds[:, 0] = rng.integers(0, max(n, 1), size=m)
    if s >= 4:
        seeds[:, 2] = seeds[:, 1]
        seeds[::3, s // 2:] = -1
    if m > 7:
        seeds[7, :] = -1
    return seeds


# ---------------------------------------------------------------- one case: the library against the restatement
_layout = {}


def layout_case(rp, layout, metric):
    """-> (what graphInsert is handed, D[N][N] of the exactly widened rows under the metric)"""
    if layout not in _layout:
        N = N_OLD + M_NEW
        if layout in DENSE:
            X = golden_dense()[:N]
            if layout == "f64":
                given, X64 = X, X
            elif layout == "f32":
                given = X.astype(np.float32)
                X64 = given.astype(np.float64)
            else:
                given = rp.to_bf16(X)
                X64 = rp.from_bf16(given).astype(np.float64)
            _layout[layout] = (given, X64, {})
        else:
            csr = golden_csr(N)
            if layout == "csr32":
                csr = (csr[0], csr[1], csr[2].astype(np.float32), csr[3])
            wide = (csr[0], csr[1], csr[2].astype(np.float64), csr[3])
            _layout[layout] = (csr, wide, {})
    given, wide, Ds = _layout[layout]
    if metric not in Ds:
        Ds[metric] = iref.pair_matrix(wide, metric) if layout in DENSE else iref.pair_matrix_csr(wide, metric)
    return given, Ds[metric]


def old_graph(D, n, kg):
    return mref.exact_graph(D[:n, :n], kg)


def check(rp, ctx, given, D, graph, m, seeds, ef, batch, metric, tag):
    """graphInsert against the restatement: the graph bit for bit, the three exact counters, `evaluated` in its bounds"""
    got = rp.graphInsert(graph, given, m, ef=ef, batch=batch, seeds=seeds, metric=distf(rp, metric), ctx=ctx)
    stats = rp.graphInsertLast(ctx)
    want = iref.graph_insert_ref(D, graph, m, seeds, ef, batch)
    ref, (chunks, offered, accepted), (lo, hi) = want
    iref.assert_same_graph(got, ref, tag)
    assert (stats[0], stats[2], stats[3]) == (chunks, offered, accepted), (tag, stats, want[1])
    assert lo <= stats[1] <= hi, (tag, stats, lo, hi)
    pad = np.arange(got[0].shape[1])[None, :] >= got[2][:, None]
    n = D.shape[0] - m
    assert np.all(got[0][n:][pad[n:]] == -1) and np.all(np.isposinf(got[1][n:][pad[n:]])), tag
    return got, stats


# ---------------------------------------------------------------- layouts and metrics
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("layout", DENSE + SPARSE)
def test_every_layout_and_metric_matches_the_definition(rp, ctx, layout, metric):
    given, D = layout_case(rp, layout, metric)
    n, m, kg = N_OLD, M_NEW, 10
    graph = old_graph(D, n, kg)
    seeds = make_seeds(5, n, m, 8)
    tag = "%s %s" % (layout, metric)
    got, stats = check(rp, ctx, given, D, graph, m, seeds, 32, 7, metric, tag)     # 14 chunks of 7 and one of 2
    assert stats[0] == 15 and got[2][n + 7] == 0 and 0 < stats[3] < stats[2]
    assert (got[0][n:] >= n).any()                                                  # rows of earlier chunks were found
    # the options change no bit of the graph, nor chunks / offered / accepted
    with option(ctx, "graph_search_nofilter", 1):
        again = rp.graphInsert(graph, given, m, ef=32, batch=7, seeds=seeds, metric=distf(rp, metric), ctx=ctx)
        bare = rp.graphInsertLast(ctx)
    iref.assert_same_graph(again, got, tag + ", graph_search_nofilter")
    assert (bare[0], bare[2], bare[3]) == (stats[0], stats[2], stats[3]) and bare[1] >= stats[1]
    if layout in SPARSE:
        with option(ctx, "graph_search_csr_stream", 1):
            again = rp.graphInsert(graph, given, m, ef=32, batch=7, seeds=seeds, metric=distf(rp, metric), ctx=ctx)
            assert rp.graphInsertLast(ctx) == stats
        iref.assert_same_graph(again, got, tag + ", graph_search_csr_stream")


# ---------------------------------------------------------------- kg, ef, batch, m
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("kg", [1, 10, 64])
def test_row_widths_beams_and_chunk_sizes(rp, ctx, kg, wide):
    given, D = layout_case(rp, "f64", "l2")
    n, m = N_OLD, M_NEW
    ef = 256 if wide else kg
    graph = old_graph(D, n, kg)
    seeds = make_seeds(kg, n, m, 8)
    for batch in (1, 7, m, m + 5):
        got, stats = check(rp, ctx, given, D, graph, m, seeds, ef, batch, "l2", "kg %d ef %d batch %d" % (kg, ef, batch))
        assert stats[0] == -(-m // batch)
        if batch >= m:                                      # one chunk: the new rows do not see each other
            assert (got[0][n:] < n).all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m", [0, 1, 65])
def test_no_new_row_one_and_a_chunk_plus_one(rp, ctx, m, metric):
    X = golden_dense()[:N_OLD + m]
    D = iref.pair_matrix(X, metric)
    graph = old_graph(D, N_OLD, 10)
    seeds = make_seeds(m, N_OLD, m, 3)
    got, stats = check(rp, ctx, X, D, graph, m, seeds, 16, 64, metric, "m %d %s" % (m, metric))
    assert stats[0] == (0, 1, 2)[(0, 1, 65).index(m)]
    if m == 0:
        iref.assert_same_graph(got, graph, "m = 0 copies the graph")
        assert stats == (0, 0, 0, 0)


def test_an_empty_graph_grows_from_nothing(rp, ctx):
    """n = 0: the first chunk finds nothing, later chunks find the earlier ones"""
    X = golden_dense()[:40]
    D = iref.pair_matrix(X, "l2")
    graph = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 4)), np.zeros(0, dtype=np.int32))
    seeds = np.stack([np.arange(i - 7, i - 4) for i in range(40)]).astype(np.int32)     # rows of earlier chunks
    seeds[seeds < 0] = -1
    got, stats = check(rp, ctx, X, D, graph, 40, seeds, 8, 5, "l2", "n = 0")
    first = got[0][:5]
    assert np.all(first[first >= 0] >= 5)                   # nothing to find; what they hold, later chunks brought
    assert np.all(got[2][5:] > 0) and stats[0] == 8


# ---------------------------------------------------------------- a hub
@pytest.mark.parametrize("batch", [150, 64])
@pytest.mark.parametrize("kg", [10, 64])
def test_a_hub_takes_far_more_than_64_offers(rp, ctx, kg, batch):
    """150 new rows that are copies or near-copies of old row 17: the copies tie at distance 0 with each
    other and with the row itself, the near-copies differ in ONE coordinate by a power of two, so all
    rows moved by the same amount are at bit-equal distances and the id decides"""
    n, m, t = N_OLD, 150, 17
    X = golden_dense()[:n]
    rng = np.random.default_rng(kg)
    new = np.repeat(X[t][None, :], m, axis=0)
    for i in range(40, m):
        new[i, rng.integers(0, X.shape[1])] += rng.choice([-1.0, 1.0]) * 2.0 ** -int(rng.integers(8, 11))
    new = new[rng.permutation(m)]
    XX = np.concatenate([X, new])
    D = iref.pair_matrix(XX, "l2")
    graph = old_graph(D, n, kg)
    seeds = rng.integers(0, n, size=(m, 4)).astype(np.int32)
    seeds[:, 1] = t
    got, stats = check(rp, ctx, XX, D, graph, m, seeds, max(kg, 32), batch, "l2", "hub kg %d batch %d" % (kg, batch))
    if batch >= m:                                          # one chunk: more than two pieces of 64 for row t
        assert (got[0][n:] == t).any(axis=1).sum() > 128
    row = got[0][t]
    assert (row[:min(kg, 40)] >= n).all() and np.all(got[1][t][:min(kg, 40)] == 0.0)       # the copies, by id
    assert np.all(np.diff(row[:min(kg, 40)]) > 0)
    assert stats[3] < stats[2]                              # most offers to the hub lose


# ---------------------------------------------------------------- cosine rows without a direction
def ragged(graph, seed):
    """every other row keeps only its first 3 .. kg - 1 entries: room for entries that rank last"""
    ids, dist, cnt = (a.copy() for a in graph)
    rng = np.random.default_rng(seed)
    for i in range(0, len(cnt), 2):
        c = int(rng.integers(3, ids.shape[1]))
        cnt[i] = c
        ids[i, c:] = -1
        dist[i, c:] = np.inf
    return ids, dist, cnt


@pytest.mark.parametrize("layout", ["f64", "csr64"])
def test_rows_without_a_direction_rank_last_by_id(rp, ctx, layout):
    """a zero dense row / an empty CSR row among the new rows under cosine: NaN from everything, so its
    answer is ordered by id, and the rows it names take it behind every number"""
    n, m = N_OLD, 60
    if layout == "f64":
        X = golden_dense()[:n + m].copy()
        X[[n + 3, n + 31]] = 0.0
        given, D = X, iref.pair_matrix(X, "cosine")
    else:
        rows = gm.rows_of(golden_csr(n + m))
        for i in (n + 3, n + 31):
            rows[i] = (np.zeros(0, dtype=np.int32), np.zeros(0))
        given = gm.from_rows(rows, 12)
        D = iref.pair_matrix_csr(given, "cosine")
    assert np.isnan(D[n + 3]).all()
    graph = ragged(old_graph(D, n, 10), 3)
    seeds = make_seeds(9, n, m, 8)
    got, stats = check(rp, ctx, given, D, graph, m, seeds, 32, 16, "cosine", "no direction, " + layout)
    assert np.isnan(got[1][n + 3][:got[2][n + 3]]).all() and np.all(np.diff(got[0][n + 3][:got[2][n + 3]]) > 0)
    assert np.isnan(got[1][:n]).any()                       # some old row took a NaN entry, behind its numbers


# ---------------------------------------------------------------- seeds
def test_seeds_of_earlier_chunks_are_followed_and_later_ones_skipped(rp, ctx):
    given, D = layout_case(rp, "f64", "l2")
    n, m, batch = N_OLD, M_NEW, 10
    graph = old_graph(D, n, 10)
    seeds = make_seeds(11, n, m, 4)
    seeds[5] = -1                                           # no seed at all
    seeds[25] = [n + 3, -1, -1, -1]                         # a row of an earlier chunk: followed
    seeds[26] = [n + 27, n + 95, n + 26, -1]                # its own chunk, a later chunk, itself: skipped
    got, _ = check(rp, ctx, given, D, graph, m, seeds, 16, batch, "l2", "seeds")
    assert got[2][n + 5] == 0 and got[2][n + 26] == 0 and got[2][n + 25] == 10
    assert not (got[0][:n] == n + 26).any() and not (got[0][:n] == n + 5).any()         # they link nothing


# ---------------------------------------------------------------- _dev: what the input rows may hold
def test_dev_copies_untouched_rows_verbatim_and_cleans_touched_ones(rp, ctx):
    import torch
    given, D = layout_case(rp, "f64", "l2")
    n, m, kg, s = N_OLD, M_NEW, 6, 4
    N = n + m
    ids, dist, cnt = (a.copy() for a in old_graph(D, n, kg))
    rng = np.random.default_rng(6)
    bad = rng.choice(n, 120, replace=False)
    for j, i in enumerate(bad):
        kind = j % 5
        if kind == 0:                                       # unsorted
            ids[i], dist[i] = ids[i, ::-1].copy(), dist[i, ::-1].copy()
        elif kind == 1:                                     # a gap inside the count
            ids[i, 2] = -1
        elif kind == 2:                                     # a count above kg
            cnt[i] = kg + 3
        elif kind == 3:                                     # an id outside [0, N)
            ids[i, 1] = N + 4
        else:                                               # the id of a NEW row, and an id twice
            ids[i, 0] = n + int(rng.integers(0, m))
            ids[i, 4] = ids[i, 3]
    seeds = make_seeds(2, n, m, s)
    ds = rp.Dataset.dense(ctx, given)
    dev = torch.device("cuda", ctx.device)
    for batch in (m, 9):
        want, (chunks, offered, accepted), (lo, hi) = iref.graph_insert_ref(D, (ids, dist, cnt), m, seeds, 16, batch)
        tg, td, tc, ts = (torch.from_numpy(a).to(dev) for a in (ids, dist, cnt, seeds))
        oi = torch.full((N, kg), 12345, dtype=torch.int32, device=dev)
        od = torch.full((N, kg), 0.5, dtype=torch.float64, device=dev)
        oc = torch.full((N,), 77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        rp.graphInsertDev(ds, kg, tg.data_ptr(), td.data_ptr(), tc.data_ptr(), m, s, ts.data_ptr(), 16, batch,
                          oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ctx.sync()
        got = (oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy())
        iref.assert_same_graph(got, want, "dev, batch %d" % batch)
        stats = rp.graphInsertLast(ctx)
        assert (stats[0], stats[2], stats[3]) == (chunks, offered, accepted) and lo <= stats[1] <= hi
        assert np.array_equal(tg.cpu().numpy(), ids) and np.array_equal(tc.cpu().numpy(), cnt)    # read only
        if batch == m:
            named = np.zeros(n, dtype=bool)
            named[got[0][n:][got[0][n:] >= 0]] = True
            same = np.array([np.array_equal(got[0][i], ids[i]) and got[2][i] == cnt[i] and
                             np.array_equal(sref.bits(got[1][i]), sref.bits(dist[i])) for i in range(n)])
            assert same[~named].all()                       # verbatim, whatever they hold
            assert (~named[bad]).sum() > 10 and named[bad].sum() > 10
            for i in bad[named[bad]]:                       # cleaned: sorted, inside [0, N), every id once
                c = int(got[2][i])
                assert 0 <= c <= kg and np.all((got[0][i, :c] >= 0) & (got[0][i, :c] < N)), i
                assert len(set(got[0][i, :c].tolist())) == c and np.all(got[0][i, c:] == -1), i
                keys = [sref.key(a, b) for a, b in zip(got[1][i, :c].tolist(), got[0][i, :c].tolist())]
                assert keys == sorted(keys), i


# ---------------------------------------------------------------- CSR against dense
@pytest.mark.parametrize("metric", METRICS)
def test_csr_rows_equal_the_dense_call_on_the_dense_ified_rows(rp, ctx, metric):
    csr, D = layout_case(rp, "csr64", metric)
    n, m = N_OLD, M_NEW
    graph = old_graph(D, n, 10)
    seeds = make_seeds(13, n, m, 8)
    a = rp.graphInsert(graph, csr, m, ef=32, batch=33, seeds=seeds, metric=distf(rp, metric), ctx=ctx)
    sa = rp.graphInsertLast(ctx)
    b = rp.graphInsert(graph, gm.densify(csr), m, ef=32, batch=33, seeds=seeds, metric=distf(rp, metric), ctx=ctx)
    sb = rp.graphInsertLast(ctx)
    iref.assert_same_graph(a, b, "csr against dense, " + metric)
    assert sa == sb and sa[0] == 4


# ---------------------------------------------------------------- (b) and (c) on the device
def test_one_chunk_is_graph_search_on_the_old_graph(rp, ctx):
    given, D = layout_case(rp, "f64", "l2")
    n, m, kg = N_OLD, M_NEW, 10
    graph = old_graph(D, n, kg)
    seeds = np.random.default_rng(1).integers(0, n, size=(m, 8)).astype(np.int32)
    got = rp.graphInsert(graph, given, m, ef=32, batch=m + 5, seeds=seeds, ctx=ctx)
    stats = rp.graphInsertLast(ctx)
    old = rp.Dataset.dense(ctx, given[:n])
    want = rp.graphSearch(graph, old, given[n:], kg, ef=32, seeds=seeds)
    sref.assert_same_answer(tuple(a[n:] for a in got), want, "batch >= m")
    assert stats[1] == rp.graphSearchLast(ctx)[1] and stats[2] == int(want[2].sum())


def test_one_call_is_the_sequence_of_single_chunk_calls(rp, ctx):
    given, D = layout_case(rp, "f64", "l2")
    n, m, b = N_OLD, M_NEW, 35                              # chunks of 35, 35 and 30 rows
    graph = old_graph(D, n, 10)
    seeds = make_seeds(17, n, m, 8)
    want = rp.graphInsert(graph, given, m, ef=32, batch=b, seeds=seeds, ctx=ctx)
    stats = rp.graphInsertLast(ctx)
    g, tot = graph, np.zeros(4, dtype=np.int64)
    for v in range(n, n + m, b):
        cnt = min(b, n + m - v)
        sd = seeds[v - n:v - n + cnt]
        sd = np.where(sd >= v + cnt, -1, sd)                # rows the prefix does not hold: skipped there, refused here
        g = rp.graphInsert(g, given[:v + cnt], cnt, ef=32, batch=cnt, seeds=sd, ctx=ctx)
        tot += rp.graphInsertLast(ctx)
    iref.assert_same_graph(g, want, "chunks of %d" % b)
    assert tuple(tot.tolist()) == stats


# ---------------------------------------------------------------- profiling
def test_the_link_kernels_have_a_profile_class_of_their_own(rp, ctx):
    """rpt_prof_*: one span of class 6 per linked chunk, the chunk's search stays class 3"""
    from rptree_amd import _lib
    L = _lib.lib()
    given, D = layout_case(rp, "f64", "l2")
    n, m = N_OLD, M_NEW
    graph = old_graph(D, n, 10)
    seeds = make_seeds(5, n, m, 8)
    _lib.check(L.rpt_prof_reset(ctx._h))
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        rp.graphInsert(graph, given, m, ef=32, batch=7, seeds=seeds, ctx=ctx)
        got = {}
        for which in (3, 6):
            ms, cnt = C.c_double(), C.c_int64()
            _lib.check(L.rpt_prof_get(ctx._h, which, C.byref(ms), C.byref(cnt)))
            got[which] = (ms.value, cnt.value)
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))
        _lib.check(L.rpt_prof_reset(ctx._h))
    assert got[3][1] == 15 and got[6][1] == 15 and got[3][0] > 0.0 and got[6][0] > 0.0, got
    ms, cnt = C.c_double(), C.c_int64()
    assert L.rpt_prof_get(ctx._h, 7, C.byref(ms), C.byref(cnt)) == RPT_E_ARG


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    given, D = layout_case(rp, "f64", "l2")
    n, m, kg, s = N_OLD, M_NEW, 10, 4
    N = n + m
    ds = rp.Dataset.dense(ctx, given)
    gids, gdist, gcnt = old_graph(D, n, kg)
    seeds0 = make_seeds(3, n, m, s)
    good = rp.graphInsert((gids, gdist, gcnt), ds, m, ef=32, batch=16, seeds=seeds0)
    stats = rp.graphInsertLast(ctx)
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(kg_=kg, m_=m, s_=s, ef_=32, batch_=16, metric=0, flags=0, g=None, c=None, sd=None):
        g = np.ascontiguousarray(gids if g is None else g, dtype=np.int32)
        c = np.ascontiguousarray(gcnt if c is None else c, dtype=np.int32)
        sd = np.ascontiguousarray(seeds0 if sd is None else sd, dtype=np.int32)
        ids = np.full((N, 64), 12345, dtype=np.int32)
        dist = np.full((N, 64), 0.5)
        cnt = np.full(N, 77, dtype=np.int32)
        st = L.rpt_graph_insert_host(ctx._h, ds._h, kg_, C.c_void_p(g.ctypes.data), C.c_void_p(gdist.ctypes.data),
                                     C.c_void_p(c.ctypes.data), m_, s_, C.c_void_p(sd.ctypes.data), ef_, batch_,
                                     metric, flags, C.c_void_p(ids.ctypes.data), C.c_void_p(dist.ctypes.data),
                                     C.c_void_p(cnt.ctypes.data))
        assert st == RPT_E_ARG, st
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77)   # nothing was written
        assert rp.graphInsertLast(ctx) == stats            # nothing was launched
        return msg

    assert "kg" in refused(kg_=0) and "kg" in refused(kg_=65, ef_=100)
    assert "s " in refused(s_=0) and "s " in refused(s_=65)
    assert "ef" in refused(ef_=9) and "ef" in refused(ef_=257)
    assert "batch" in refused(batch_=0) and "batch" in refused(batch_=-3)
    assert "m " in refused(m_=-1) and "m " in refused(m_=N + 1)
    for mt in (COS | INN, REF, 2, -1):
        assert "metric" in refused(metric=mt)
    for fl in (1, COS, REF):
        assert "flags" in refused(flags=fl)
    bad = np.array(gids)
    bad[201, 0] = n                                         # a graph over the first n rows holds no new id
    assert "graph row 201" in refused(g=bad)
    badc = np.array(gcnt)
    badc[17] = kg + 1
    assert "graph row 17" in refused(c=badc)
    bads = np.array(seeds0)
    bads[40, 1] = N
    assert "seeds row 40" in refused(sd=bads)
    bads[40, 1] = -2
    assert "seeds row 40" in refused(sd=bads)
    with pytest.raises(ValueError):
        rp.graphInsert((gids, gdist, gcnt), ds, m)                                  # neither seeds nor a forest
    with pytest.raises(ValueError):
        rp.graphInsert((gids, gdist, gcnt), ds, m - 1, seeds=seeds0[1:])            # the graph is not over N - m rows
    again = rp.graphInsert((gids, gdist, gcnt), ds, m, ef=32, batch=16, seeds=seeds0)
    iref.assert_same_graph(again, good, "after the refusals")
    assert rp.graphInsertLast(ctx) == stats


# ---------------------------------------------------------------- end to end
def test_insert_then_find_an_inserted_row(rp, ctx):
    """a forest and a graph over the old rows, graphInsert with the forest's seeds and the defaults, then
    graphSearch from a row that lists an inserted row: that row comes first, at distance 0"""
    n, m, d, kg = 1200, 200, 16, 10
    X = np.random.default_rng(31).standard_normal((n + m, d))
    old = rp.Dataset.dense(ctx, X[:n])
    cfg = rp.rpTreeCfg(40, n, d)
    f = rp.forestBatch(5, cfg.fpMaxTreeDepth, 40, 4, cfg.fpProjNzDensity, d, old, ctx=ctx)
    graph = rp.knnGraphRefine(rp.knnGraph(kg, f), f, iters=1)
    got = rp.graphInsert(graph, X, m, forest=f, ctx=ctx)                            # ef 32, batch min(m, 4096)
    stats = rp.graphInsertLast(ctx)
    sid, _, scnt = rp.knnBatch(8, f, X[n:], dedup=True)
    seeds = np.where(np.arange(8)[None, :] < scnt[:, None], sid, -1).astype(np.int32)
    want, (chunks, offered, accepted), (lo, hi) = iref.graph_insert_ref(iref.pair_matrix(X, "l2"), graph, m, seeds, 32, m)
    iref.assert_same_graph(got, want, "forest seeds, default ef and batch")
    assert (stats[0], stats[2], stats[3]) == (1, offered, accepted) and lo <= stats[1] <= hi and accepted > m
    # search the grown graph over all rows
    ds = rp.Dataset.dense(ctx, X)
    listed = [(o, p) for o in range(n) for p in got[0][o, :got[2][o]] if p >= n]
    assert len(listed) == accepted
    pick = listed[::max(1, len(listed) // 20)][:20]
    Q = X[[p for _, p in pick]]
    qseeds = np.array([[o] for o, _ in pick], dtype=np.int32)
    ids, dist, cnt = rp.graphSearch(got, ds, Q, 5, ef=32, seeds=qseeds)
    assert ids[:, 0].tolist() == [p for _, p in pick] and np.all(dist[:, 0] == 0.0) and np.all(cnt == 5)


# ---------------------------------------------------------------- the link's scratch, poisoned
POISON_NODES = ("test_every_layout_and_metric_matches_the_definition[f64-cosine]",
                "test_every_layout_and_metric_matches_the_definition[csr32-l2]",
                "test_a_hub_takes_far_more_than_64_offers[10-64]",
                "test_an_empty_graph_grows_from_nothing",
                "test_dev_copies_untouched_rows_verbatim_and_cleans_touched_ones")
_dead_child = None        # set by a child that died: no process is started after it


@pytest.mark.parametrize("byte", [255, 127])
def test_parity_on_poisoned_scratch(byte):
    """deg / toff / the touched list / the offers' segments come from the context's pool and only deg is
    cleared: with RPT_POOL_POISON (tests/test_gpu_pool_poison.py) every block is filled with `byte` before
    it is handed out, and the same bits must come back.  A child process, because the allocator reads the
    variable once; the probe of that file proves the child's allocator poisons."""
    global _dead_child
    if _dead_child is not None:
        pytest.fail("no child is started after a child that died: " + _dead_child)
    here = "tests/test_gpu_graph_insert.py::"
    env = dict(os.environ)
    env["RPT_POOL_POISON"] = str(byte)
    cmd = ["timeout", "-k", "10", "120", sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
           "tests/test_gpu_pool_poison.py::test_pool_probe_sees_the_poison"] + [here + n for n in POISON_NODES]
    try:
        pr = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=150)
    except subprocess.TimeoutExpired as e:
        _dead_child = "poison %d did not end within 150 s" % byte
        pytest.fail(_dead_child + "\n" + (e.stdout or b"").decode("utf-8", "replace")[-4000:])
    tail = pr.stdout.decode("utf-8", "replace")[-4000:]
    if pr.returncode < 0 or pr.returncode in (134, 139, 124, 137):
        _dead_child = "poison %d ended with status %d" % (byte, pr.returncode)
        pytest.fail(_dead_child + "\n" + tail)
    assert pr.returncode == 0, "poison %d: exit status %d\n%s" % (byte, pr.returncode, tail)
    summary = tail.strip().splitlines()[-1]
    assert "%d passed" % (len(POISON_NODES) + 1) in summary and "skipped" not in summary, summary


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_example(tmp_path):
    """host/example_graph_insert.cpp: a graph over n rows, m rows inserted, an inserted row found"""
    exe = str(tmp_path / "example_graph_insert")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_graph_insert.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "2000", "300", "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[0] == "inserted 300 rows into a graph of 2000"
    print(r.stdout)
