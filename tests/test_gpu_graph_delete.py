"""Rows out of a kNN graph on the device (rpt_graph_delete_host / _dev; csrc/graph_delete.hip:
delete_mark / _scan / _copy_kernel and delete_repair_kernel / delete_repair_csr_kernel): ids, counts,
distance BITS, newid and the four counters of rpt_graph_delete_last against the numpy restatement in
tests/graph_delete_ref.py, in both forms (old ids and compact).  No tolerance anywhere.

The shapes are the smallest at which the kernels can still go wrong: 333 rows (no multiple of 32, junk
bits behind the last id in the bitmap), d = 5 / 33 / 70 (one chunk of 32 columns, a chunk and one
column, two chunks and a rest; 5 and 33 columns of f64 or bf16 take the staging path without 16-byte
loads), CSR rows longer than a piece of 64 entries, kg = 64 (one row per workgroup), a row with more
than 64 candidates, rows that end short or empty, and input rows that no graph would hold."""
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
import graph_delete_ref as dref  # noqa: E402
import graph_metric_csr_ref as gm  # noqa: E402

RPT_E_ARG = -1
METRICS = ("l2", "cosine", "inner")
DENSE = ("f64", "f32", "bf16")
SPARSE = ("csr64", "csr32")
N = 333
DIM = {"f64": 33, "f32": 70, "bf16": 5}


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


def junk_words(rp, mask):
    """the bitmap of a bool mask with every bit behind the last id set"""
    n = len(mask)
    w = rp.allowBitmap(np.asarray(mask, dtype=bool), n).copy()
    if n % 32:
        w[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    return w


def random_mask(seed, n, deleted):
    return ~(np.random.default_rng(seed).random(n) < deleted)


_layout = {}


def layout_case(rp, layout, metric):
    """-> (what graphDelete is handed, D[n][n] of the exactly widened rows under the metric)"""
    if layout not in _layout:
        if layout in DENSE:
            X = np.random.default_rng(70 + DIM[layout]).standard_normal((N, DIM[layout]))
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
            # csr64: short rows, some empty; csr32: 150 columns at density 0.6, about 90 entries a row
            csr = gm.make_csr(5, N, 40, 0.3, empty=(3, 77, 200)) if layout == "csr64" else \
                gm.make_csr(6, N, 150, 0.6, dtype=np.float32)
            wide = (csr[0], csr[1], csr[2].astype(np.float64), csr[3])
            _layout[layout] = (csr, wide, {})
    given, wide, Ds = _layout[layout]
    if metric not in Ds:
        Ds[metric] = dref.pair_matrix(wide, metric) if layout in DENSE else dref.pair_matrix_csr(wide, metric)
    return given, Ds[metric]


def random_graph(D, kg, seed):
    """kg random ids per row (not the row itself, each once) with their true distances, in random order"""
    n = D.shape[0]
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.choice(np.delete(np.arange(n), i), kg, replace=False) for i in range(n)]).astype(np.int32)
    return ids, np.take_along_axis(D, ids.astype(np.int64), axis=1), np.full(n, kg, dtype=np.int32)


def check(rp, ctx, given, D, graph, keep, metric, tag, forms=(False, True)):
    """graphDelete against the restatement, both forms: the graph and newid bit for bit, the four counters"""
    out = {}
    for compact in forms:
        got, newid = rp.graphDelete(keep, graph, given, compact=compact, metric=distf(rp, metric), ctx=ctx)
        stats = rp.graphDeleteLast(ctx)
        want, wid, wstats = dref.graph_delete_ref(D, graph, keep, compact)
        t = "%s, %s" % (tag, "compact" if compact else "old ids")
        assert got[0].shape == want[0].shape, t
        dref.assert_same_graph(got, want, t)
        assert np.array_equal(newid, wid) and newid.dtype == np.int32, t
        assert stats == wstats, (t, stats, wstats)
        out[compact] = (got, newid, stats)
    return out


# ---------------------------------------------------------------- layouts and metrics
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("layout", DENSE + SPARSE)
def test_every_layout_and_metric_matches_the_definition(rp, ctx, layout, metric):
    given, D = layout_case(rp, layout, metric)
    graph = mref.exact_graph(D, 10)
    mask = random_mask(7, N, 0.3)
    tag = "%s %s" % (layout, metric)
    out = check(rp, ctx, given, D, graph, junk_words(rp, mask), metric, tag)
    (got, newid, stats) = out[False]
    assert stats[0] == int(mask.sum()) and 0 < stats[1] <= stats[0] and stats[2] > stats[3] > 0
    assert not np.isin(got[0], np.flatnonzero(~mask)).any()             # no entry names a deleted row
    assert np.all(got[2][~mask] == 0) and np.all(got[0][~mask] == -1) and np.all(np.isposinf(got[1][~mask]))
    # the compact form is the other form through newid
    (cg, cid, _) = out[True]
    kept = np.flatnonzero(mask)
    assert np.array_equal(cid[kept], np.arange(len(kept)))
    mapped = np.where(got[0][kept] >= 0, newid_map(cid, got[0][kept]), -1)
    assert np.array_equal(cg[0], mapped) and np.array_equal(sref.bits(cg[1]), sref.bits(got[1][kept]))
    assert np.array_equal(cg[2], got[2][kept])
    with option(ctx, "graph_delete_general", 1):                        # one row per workgroup: the same bits
        again, aid = rp.graphDelete(mask, graph, given, compact=False, metric=distf(rp, metric), ctx=ctx)
        assert rp.graphDeleteLast(ctx) == stats
    dref.assert_same_graph(again, got, tag + ", graph_delete_general")
    assert np.array_equal(aid, newid)


def newid_map(newid, ids):
    return newid[np.where(ids >= 0, ids, 0)]


# ---------------------------------------------------------------- kg and what is kept
def keeps(rp, n):
    one = np.zeros(n, dtype=bool)
    one[41] = True
    return {"all": np.ones(n, dtype=bool), "all but one": ~one, "one row": one, "nothing": np.zeros(n, dtype=bool),
            "NULL": None, "30 % deleted": junk_words(rp, random_mask(1, n, 0.3)), "90 % deleted": random_mask(2, n, 0.9)}


@pytest.mark.parametrize("kg", [1, 4, 10, 64])
def test_row_widths_and_keep_patterns(rp, ctx, kg):
    """kg = 64 on dense rows is the one-row-per-workgroup shape: four waves' shares do not fit 160 KB"""
    given, D = layout_case(rp, "f64", "l2")
    graph = mref.exact_graph(D, kg)
    for name, keep in keeps(rp, N).items():
        out = check(rp, ctx, given, D, graph, keep, "l2", "kg %d, %s" % (kg, name))
        got, newid, stats = out[False]
        if name in ("all", "NULL"):
            dref.assert_same_graph(got, graph, name + " is the identity")
            assert np.array_equal(newid, np.arange(N)) and stats == (N, 0, 0, 0)
            dref.assert_same_graph(out[True][0], graph, name + " is the identity, compact")
        if name == "nothing":
            assert stats == (0, 0, 0, 0) and out[True][0][0].shape == (0, kg) and np.all(newid == -1)
        if name == "one row":
            assert stats[0] == 1 and out[True][0][2].tolist() == [0]
    if kg <= 10:
        keep = keeps(rp, N)["30 % deleted"]
        with option(ctx, "graph_delete_general", 1):
            check(rp, ctx, given, D, graph, keep, "l2", "kg %d, graph_delete_general" % kg)


# ---------------------------------------------------------------- crafted graphs
def test_a_deleted_hub_touches_every_row(rp, ctx):
    given, D = layout_case(rp, "f64", "l2")
    h, kg = 100, 10
    ids, dist, cnt = (a.copy() for a in mref.exact_graph(D, kg))
    for i in range(N):
        if i != h and h not in ids[i]:
            ids[i, kg - 1], dist[i, kg - 1] = h, D[i, h]
    keep = np.ones(N, dtype=bool)
    keep[h] = False
    out = check(rp, ctx, given, D, (ids, dist, cnt), keep, "l2", "hub")
    assert out[False][2][:2] == (N - 1, N - 1) and out[False][2][3] == N - 1


def test_more_than_64_candidates_take_two_blocks(rp, ctx):
    """row 0 names rows 1 .. 10, of which 1 .. 8 are deleted and hold 80 different kept ids"""
    for layout in ("f32", "csr32"):
        given, D = layout_case(rp, layout, "l2")
        ids, dist, cnt = random_graph(D, 10, 12)
        keep = np.ones(N, dtype=bool)
        keep[1:9] = False
        ids[0] = np.arange(1, 11)
        for j in range(1, 9):
            ids[j] = 20 + 10 * (j - 1) + np.arange(10)
        dist = np.take_along_axis(D, ids.astype(np.int64), axis=1)
        out = check(rp, ctx, given, D, (ids, dist, cnt), keep, "l2", "two blocks, " + layout)
        C0 = set(range(20, 100))                            # 80 candidates: a block of 64 and one of 16
        best = sorted([(D[0, e], e) for e in C0 | {9, 10}])[:10]
        assert out[False][0][0][0].tolist() == [e for _, e in best]


def test_rows_whose_second_hop_is_gone_end_short(rp, ctx):
    """row 0 names 1, 2, 3; they name 4 .. 9; all of 1 .. 9 are deleted: row 0 ends empty.  Row 10 names
    1 and 11; row 1 names 4, 5, 6 (deleted): row 10 keeps one entry"""
    given, D = layout_case(rp, "f64", "cosine")
    ids, dist, cnt = random_graph(D, 6, 3)
    keep = np.ones(N, dtype=bool)
    keep[1:10] = False
    ids[0, :3], cnt[0] = [1, 2, 3], 3
    ids[1, :3], ids[2, :3], ids[3, :3] = [4, 5, 6], [6, 7, 8], [9, 4, 5]
    cnt[1:4] = 3
    ids[10, :2], cnt[10] = [1, 11], 2
    dist = np.take_along_axis(D, ids.astype(np.int64), axis=1)
    out = check(rp, ctx, given, D, (ids, dist, cnt), keep, "cosine", "short rows")
    got = out[False][0]
    assert got[2][0] == 0 and np.all(got[0][0] == -1) and got[2][10] == 1 and got[0][10, 0] == 11


@pytest.mark.parametrize("layout", ["f64", "csr64"])
def test_duplicate_rows_tie_by_id_and_nan_rows_rank_last_by_id(rp, ctx, layout):
    n = 200
    if layout == "f64":
        X = np.random.default_rng(8).standard_normal((n, 33))
        X[50:90] = X[10]                                    # 41 copies: bit-equal distances, the id decides
        X[[120, 121, 122]] = np.nan
        given, D = X, dref.pair_matrix(X, "l2")
        metric = "l2"
    else:
        rows = gm.rows_of(gm.make_csr(9, n, 40, 0.3))
        for i in range(50, 90):
            rows[i] = rows[10]
        for i in (120, 121, 122):                           # empty rows: NaN under cosine
            rows[i] = (np.zeros(0, dtype=np.int32), np.zeros(0))
        given = gm.from_rows(rows, 40)
        D, metric = dref.pair_matrix_csr(given, "cosine"), "cosine"
    assert np.isnan(D[120]).all()
    ids, dist, cnt = random_graph(D, 10, 4)
    ids[60, :4] = [10, 55, 120, 7]                          # a copy that names copies, a NaN row and a row to delete
    ids[7, :6] = [51, 52, 70, 121, 122, 11]
    dist = np.take_along_axis(D, ids.astype(np.int64), axis=1)
    keep = random_mask(5, n, 0.25)
    keep[[10, 51, 52, 55, 60, 70, 120, 121, 122]] = True
    keep[7] = False
    out = check(rp, ctx, given, D, (ids, dist, cnt), keep, metric, "ties and NaN, " + layout)
    got = out[False][0]
    row, d = got[0][60], got[1][60]
    zero = row[d == 0.0] if layout == "f64" else row[np.abs(d) < 1e-15]
    assert {10, 51, 52, 55, 70} <= set(zero.tolist()) and np.all(np.diff(zero) > 0)
    assert np.isnan(got[1]).any()


# ---------------------------------------------------------------- CSR against dense
@pytest.mark.parametrize("metric", METRICS)
def test_csr_rows_equal_the_dense_call_on_the_dense_ified_rows(rp, ctx, metric):
    csr, D = layout_case(rp, "csr64", metric)
    graph = mref.exact_graph(D, 10) if metric == "l2" else random_graph(D, 10, 2)
    keep = random_mask(3, N, 0.3)
    a, aid = rp.graphDelete(keep, graph, csr, metric=distf(rp, metric), ctx=ctx)
    sa = rp.graphDeleteLast(ctx)
    b, bid = rp.graphDelete(keep, graph, gm.densify(csr), metric=distf(rp, metric), ctx=ctx)
    assert sa == rp.graphDeleteLast(ctx) and np.array_equal(aid, bid)
    if metric == "cosine":                                  # the empty rows: NaN either way
        assert np.isnan(a[1]).any()
    dref.assert_same_graph(a, b, "csr against dense, " + metric)


@pytest.mark.parametrize("metric", ["cosine", "inner"])
def test_a_stored_inf_gets_the_answer_of_dots(rp, ctx, metric):
    """dotS takes the columns BOTH rows store, so a stored inf meets no absent column's 0: a number where
    the dense fold has NaN"""
    n = 120
    rows = gm.rows_of(gm.make_csr(11, n, 40, 0.3))
    for i in range(0, n, 3):
        c, v = rows[i]
        v = v.copy()
        v[0] = np.inf
        rows[i] = (c, v)
    csr = gm.from_rows(rows, 40)
    D = dref.pair_matrix_csr(csr, metric)
    graph = random_graph(D, 8, 6)
    keep = random_mask(4, n, 0.3)
    out = check(rp, ctx, csr, D, graph, keep, metric, "stored inf, " + metric, forms=(False,))
    dense, _ = rp.graphDelete(keep, graph, gm.densify(csr), compact=False, metric=distf(rp, metric), ctx=ctx)
    got = out[False][0]
    assert not np.array_equal(sref.bits(got[1]), sref.bits(dense[1]))


# ---------------------------------------------------------------- _dev: what the input rows may hold
def junk_graph(D, kg, seed):
    n = D.shape[0]
    ids, dist, cnt = (a.copy() for a in mref.exact_graph(D, kg))
    rng = np.random.default_rng(seed)
    bad = rng.choice(n, 150, replace=False)
    for j, i in enumerate(bad):
        kind = j % 6
        if kind == 0:                                       # unsorted
            ids[i], dist[i] = ids[i, ::-1].copy(), dist[i, ::-1].copy()
        elif kind == 1:                                     # a short count, ids of any kind behind it
            cnt[i] = 3
            ids[i, 4] = n + 9
        elif kind == 2:                                     # counts outside [0, kg]
            cnt[i] = kg + 3 if j % 12 == 2 else -2
        elif kind == 3:                                     # ids outside [0, n)
            ids[i, 1], ids[i, 2] = n + 4, -7
        elif kind == 4:                                     # an id twice
            ids[i, 4] = ids[i, 0]
        else:                                               # itself
            ids[i, 2] = i
    return (ids, dist, cnt), bad


def test_dev_copies_untouched_rows_verbatim_and_cleans_touched_ones(rp, ctx):
    import torch
    given, D = layout_case(rp, "f64", "l2")
    kg = 6
    (ids, dist, cnt), bad = junk_graph(D, kg, 6)
    mask = random_mask(9, N, 0.1)
    words = junk_words(rp, mask)
    ds = rp.Dataset.dense(ctx, given)
    dev = torch.device("cuda", ctx.device)
    tg, td, tc = (torch.from_numpy(a).to(dev) for a in (ids, dist, cnt))
    tw = torch.from_numpy(words.view(np.int32)).to(dev)
    for compact in (False, True):
        for with_newid in (True, False):
            want, wid, wstats = dref.graph_delete_ref(D, (ids, dist, cnt), mask, compact)
            oi = torch.full((N, kg), 12345, dtype=torch.int32, device=dev)
            od = torch.full((N, kg), 0.5, dtype=torch.float64, device=dev)
            oc = torch.full((N,), 77, dtype=torch.int32, device=dev)
            nid = torch.full((N,), 99, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            rp.graphDeleteDev(ds, kg, tg.data_ptr(), td.data_ptr(), tc.data_ptr(), tw.data_ptr(), oi.data_ptr(),
                              od.data_ptr(), oc.data_ptr(), nid.data_ptr() if with_newid else 0, compact=compact)
            ctx.sync()
            tag = "dev, compact %s, newid %s" % (compact, with_newid)
            got = (oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy())
            rows = want[0].shape[0]
            dref.assert_same_graph(tuple(a[:rows] for a in got), want, tag)
            assert rp.graphDeleteLast(ctx) == wstats, tag
            # behind the n' rows of the compact form nothing was written
            assert np.all(got[0][rows:] == 12345) and np.all(got[1][rows:] == 0.5) and np.all(got[2][rows:] == 77), tag
            assert np.array_equal(nid.cpu().numpy(), wid if with_newid else np.full(N, 99)), tag
            assert np.array_equal(tg.cpu().numpy(), ids) and np.array_equal(tc.cpu().numpy(), cnt)    # read only
            assert np.array_equal(sref.bits(td.cpu().numpy()), sref.bits(dist))
    # untouched rows are verbatim whatever they hold, touched rows are cleaned
    want, wid, wstats = dref.graph_delete_ref(D, (ids, dist, cnt), mask, False)
    gone = np.flatnonzero(~mask)
    touched = np.array([mask[i] and any(e in gone for _, e in dref.valid_entries(ids[i], dist[i], cnt[i], N, i))
                        for i in range(N)])
    assert touched.sum() == wstats[1] and touched[bad].sum() > 10 and (mask & ~touched)[bad].sum() > 10
    for i in np.flatnonzero(mask & ~touched):
        assert want[2][i] == cnt[i] and np.array_equal(sref.bits(want[1][i]), sref.bits(dist[i])), i
        inside = (ids[i] >= 0) & (ids[i] < N)
        assert np.array_equal(want[0][i][~inside], ids[i][~inside]), i
        assert np.array_equal(want[0][i][inside], np.where(mask[ids[i][inside]], ids[i][inside], -1)), i
    for i in np.flatnonzero(touched):
        c = int(want[2][i])
        row = want[0][i, :c]
        assert 0 <= c <= kg and np.all((row >= 0) & (row < N)) and i not in row and len(set(row.tolist())) == c, i
        keys = [sref.key(a, b) for a, b in zip(want[1][i, :c].tolist(), row.tolist())]
        assert keys == sorted(keys) and np.all(want[0][i, c:] == -1), i


# ---------------------------------------------------------------- delete, then search
def test_delete_then_search(rp, ctx):
    given, D = layout_case(rp, "f64", "l2")
    graph = mref.exact_graph(D, 10)
    mask = random_mask(21, N, 0.4)
    kept = np.flatnonzero(mask)
    # compact: the graph belongs to the compacted rows; every survivor is its own nearest neighbour
    (cg, newid) = rp.graphDelete(mask, graph, given, ctx=ctx)
    Xc = rp.compactRows(given, mask)
    assert np.array_equal(Xc, given[mask]) and np.array_equal(rp.compactRows(given, rp.allowBitmap(mask, N)), Xc)
    ds = rp.Dataset.dense(ctx, Xc)
    lister = {}                                             # a row that lists p, for every p that is listed
    for o in range(len(kept)):
        for p in cg[0][o, :cg[2][o]]:
            lister.setdefault(int(p), o)
    pick = sorted(lister)[::5]
    seeds = np.array([[lister[p]] for p in pick], dtype=np.int32)
    ids, dist, cnt = rp.graphSearch(cg, ds, Xc[pick], 5, ef=32, seeds=seeds)
    assert ids[:, 0].tolist() == pick and np.all(dist[:, 0] == 0.0)
    # old ids: the unchanged data set; from kept seeds no answer is a deleted row
    (og, oid) = rp.graphDelete(mask, graph, given, compact=False, ctx=ctx)
    full = rp.Dataset.dense(ctx, given)
    rng = np.random.default_rng(3)
    Q = given[rng.choice(N, 50, replace=False)] + 0.05 * rng.standard_normal((50, given.shape[1]))
    seeds = rng.choice(kept, size=(50, 6)).astype(np.int32)
    ids, dist, cnt = rp.graphSearch(og, full, Q, 10, ef=32, seeds=seeds)
    found = ids[ids >= 0]
    assert len(found) > 400 and mask[found].all()
    # CSR rows, compacted
    csr, Dc = layout_case(rp, "csr64", "l2")
    sub = rp.compactRows(csr, mask)
    want = gm.from_rows([r for r, k in zip(gm.rows_of(csr), mask) if k], csr[3])
    assert all(np.array_equal(a, b) for a, b in zip(sub[:3], want[:3])) and sub[3] == csr[3]


# ---------------------------------------------------------------- profiling
def test_the_delete_kernels_have_a_profile_class_of_their_own(rp, ctx):
    """rpt_prof_*: one span of class 8 per call; nothing of it is class 3 or 6"""
    from rptree_amd import _lib
    L = _lib.lib()
    given, D = layout_case(rp, "f64", "l2")
    graph = mref.exact_graph(D, 10)
    mask = random_mask(7, N, 0.3)
    _lib.check(L.rpt_prof_reset(ctx._h))
    _lib.check(L.rpt_prof_enable(ctx._h, 1))
    try:
        rp.graphDelete(mask, graph, given, ctx=ctx)
        rp.graphDelete(mask, graph, given, compact=False, ctx=ctx)
        got = {}
        for which in (3, 6, 8):
            ms, cnt = C.c_double(), C.c_int64()
            _lib.check(L.rpt_prof_get(ctx._h, which, C.byref(ms), C.byref(cnt)))
            got[which] = (ms.value, cnt.value)
    finally:
        _lib.check(L.rpt_prof_enable(ctx._h, 0))
        _lib.check(L.rpt_prof_reset(ctx._h))
    assert got[8][1] == 2 and got[8][0] > 0.0 and got[3][1] == 0 and got[6][1] == 0, got
    ms, cnt = C.c_double(), C.c_int64()
    assert L.rpt_prof_get(ctx._h, 9, C.byref(ms), C.byref(cnt)) == RPT_E_ARG


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(rp, ctx):
    from rptree_amd import _lib
    L = _lib.lib()
    given, D = layout_case(rp, "f64", "l2")
    kg = 10
    ds = rp.Dataset.dense(ctx, given)
    gids, gdist, gcnt = mref.exact_graph(D, kg)
    mask = random_mask(7, N, 0.3)
    words = rp.allowBitmap(mask, N)
    good = rp.graphDelete(words, (gids, gdist, gcnt), ds)
    stats = rp.graphDeleteLast(ctx)
    COS, INN, REF = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE

    def refused(kg_=kg, metric=0, flags=0, g=None, c=None):
        g = np.ascontiguousarray(gids if g is None else g, dtype=np.int32)
        c = np.ascontiguousarray(gcnt if c is None else c, dtype=np.int32)
        ids = np.full((N, 64), 12345, dtype=np.int32)
        dist = np.full((N, 64), 0.5)
        cnt = np.full(N, 77, dtype=np.int32)
        nid = np.full(N, 99, dtype=np.int32)
        st = L.rpt_graph_delete_host(ctx._h, ds._h, kg_, C.c_void_p(g.ctypes.data), C.c_void_p(gdist.ctypes.data),
                                     C.c_void_p(c.ctypes.data), C.c_void_p(words.ctypes.data), metric, flags,
                                     C.c_void_p(ids.ctypes.data), C.c_void_p(dist.ctypes.data),
                                     C.c_void_p(cnt.ctypes.data), C.c_void_p(nid.ctypes.data))
        assert st == RPT_E_ARG, st
        msg = L.rpt_last_error().decode()
        assert len(msg) > 8, msg
        assert np.all(ids == 12345) and np.all(dist == 0.5) and np.all(cnt == 77) and np.all(nid == 99)
        assert rp.graphDeleteLast(ctx) == stats            # nothing was launched
        return msg

    assert "kg" in refused(kg_=0) and "kg" in refused(kg_=65)
    for mt in (COS | INN, REF, 2, -1):
        assert "metric" in refused(metric=mt)
    for fl in (2, 3, COS, REF, -1):
        assert "flags" in refused(flags=fl)
    bad = np.array(gids)
    bad[201, 0] = N
    assert "graph row 201" in refused(g=bad)
    bad[201, 0] = -1
    assert "graph row 201" in refused(g=bad)
    badc = np.array(gcnt)
    badc[17] = kg + 1
    assert "graph row 17" in refused(c=badc)
    with pytest.raises(ValueError):
        rp.graphDelete(mask[:-1], (gids, gdist, gcnt), ds)                          # a mask of another length
    with pytest.raises(ValueError):
        rp.graphDelete(mask, (gids[:-1], gdist[:-1], gcnt[:-1]), ds)               # a graph over other rows
    with pytest.raises(ValueError):
        rp.graphDelete(np.flatnonzero(mask), (gids, gdist, gcnt), ds)               # ids are not a keep mask
    again = rp.graphDelete(words, (gids, gdist, gcnt), ds)
    dref.assert_same_graph(again[0], good[0], "after the refusals")
    assert np.array_equal(again[1], good[1]) and rp.graphDeleteLast(ctx) == stats


def test_an_empty_data_set_is_valid(rp, ctx):
    graph = (np.zeros((0, 4), dtype=np.int32), np.zeros((0, 4)), np.zeros(0, dtype=np.int32))
    for compact in (False, True):
        for keep in (None, np.zeros(0, dtype=bool)):
            got, newid = rp.graphDelete(keep, graph, np.zeros((0, 4)), compact=compact, ctx=ctx)
            assert got[0].shape == (0, 4) and got[2].shape == (0,) and newid.shape == (0,)
            assert rp.graphDeleteLast(ctx) == (0, 0, 0, 0)


# ---------------------------------------------------------------- the scratch, poisoned
POISON_NODES = ("test_every_layout_and_metric_matches_the_definition[f64-cosine]",
                "test_every_layout_and_metric_matches_the_definition[csr32-l2]",
                "test_row_widths_and_keep_patterns[64]",
                "test_more_than_64_candidates_take_two_blocks",
                "test_dev_copies_untouched_rows_verbatim_and_cleans_touched_ones")
_dead_child = None        # set by a child that died: no process is started after it


@pytest.mark.parametrize("byte", [255, 127])
def test_parity_on_poisoned_scratch(byte):
    """the flags, the touched list and newid come from the context's pool and nothing clears them: with
    RPT_POOL_POISON (tests/test_gpu_pool_poison.py) every block is filled with `byte` before it is handed
    out, and the same bits must come back.  A child process, because the allocator reads the variable
    once; the probe of that file proves the child's allocator poisons."""
    global _dead_child
    if _dead_child is not None:
        pytest.fail("no child is started after a child that died: " + _dead_child)
    here = "tests/test_gpu_graph_delete.py::"
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
    """host/example_graph_delete.cpp: a graph over n rows, a fifth of them deleted, the survivors searched"""
    exe = str(tmp_path / "example_graph_delete")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_graph_delete.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src, "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "2000", "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[0].startswith("deleted ") and lines[0].endswith(" of 2000 rows")
    print(r.stdout)
