"""An allow-list on the forest query and on the exhaustive kNN (rpt_knn_allow_*,
rpt_allow_candidates_host, rpt_brute_knn_allow_*, rpt_recall_hits_allow_host) on the device against
the numpy restatement tests/knn_allow_ref.py: the allowed lists under every mask and across the slice
seam, lists of ~16 000 candidates, every (layout, dtype, distance) cell under the three duplicate
rules, the exhaustive answer against bruteKnn over the allowed rows alone, recall, the device entry
points, the refusals and poisoned scratch."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_allow_ref as ref
import knn_metric_csr_ref as csrref
import test_gpu_brute_csr as brute_csr  # the rule of the true-L2 leg: check_l2, RTOL, ATOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPT_E_ARG, RPT_E_UNSUPPORTED = -1, -4
N, D, T, ML = 3000, 12, 6, 20


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


def masks(n):
    """name -> (what is passed as `allow`, the bool mask it means)"""
    draw = lambda f: np.random.default_rng(7).random(n) < f
    one = np.zeros(n, dtype=bool)
    one[n // 3] = True
    last = np.zeros(n, dtype=bool)
    last[((n - 1) // 32) * 32:] = True
    out = {"half": draw(0.5), "tenth": draw(0.1), "hundredth": draw(0.01), "all": np.ones(n, dtype=bool),
           "none": np.zeros(n, dtype=bool), "one": one, "last_word": last}
    out = {name: (m, m) for name, m in out.items()}
    out["tail_bits"] = (ref.bitmap(draw(0.5), tail=True), draw(0.5))     # the words, every bit behind n set
    return out


# ------------------------------------------------------------------ H. poisoned scratch (first: the
# child starts before this module's own GPU calls)
POISON_NODES = ["tests/test_gpu_pool_poison.py::test_pool_probe_sees_the_poison",
                "tests/test_gpu_knn_allow.py::test_lists[streamed-slice7]",
                "tests/test_gpu_knn_allow.py::test_long_lists"]


def test_no_slab_word_is_read_unwritten():
    """one case of A (sliced) and B in a fresh child whose allocator fills every block with 0xff: an
    unwritten id, range or count word read anywhere would be id -1 and change the answer"""
    env = dict(os.environ)
    env["RPT_POOL_POISON"] = "255"
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"]
    pr = subprocess.run(cmd + POISON_NODES, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                        timeout=180)
    tail = pr.stdout.decode("utf-8", "replace")[-4000:]
    assert pr.returncode == 0, "exit status %d\n%s" % (pr.returncode, tail)
    summary = tail.strip().splitlines()[-1]
    assert "3 passed" in summary and "skipped" not in summary, summary


# ------------------------------------------------------------------ forests
def dense_rows(oracle):
    X = oracle.data_normal_dense2(11, N, D)
    rng = np.random.default_rng(5)
    Q = np.concatenate([X[:30] * 1.002 + 0.004, rng.standard_normal((9, D)), np.full((1, D), 40.0)])
    return X, Q


def hyperplanes(oracle, n, d, ml, seed=13, trees=T):
    L, _, pnz = oracle.tree_cfg(ml, n, d)
    R, _ = oracle.forest_hyperplanes(seed, trees, L, pnz, d)
    return L, pnz, R


def sparse_rows():
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_sparse_600x12.npz"))
    data = (z["rowptr"], z["col"], z["val"])
    d = int(z["d"])
    rng = np.random.default_rng(6)
    fresh = csrref.random_csr(rng, 13, d, 0.3)
    lens = np.concatenate([np.diff(data[0])[:20], np.diff(fresh[0]), [0]])        # stored rows, fresh, an empty one
    col = np.concatenate([data[1][:data[0][20]], fresh[1]])
    val = np.concatenate([data[2][:data[0][20]], fresh[2]])
    return data, (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col.astype(np.int32), val), d


@pytest.fixture(scope="module")
def forests(rp, ctx, oracle):
    X, Q = dense_rows(oracle)
    L, pnz, R = hyperplanes(oracle, N, D, ML)
    out = {"dense": (rp.forestBatch(0, L, ML, T, pnz, D, X, ctx=ctx, hyperplanes=R, mode=rp.RPT_PROJ_EXACT), Q),
           # a chunk that does not divide n: empty Tips occur
           "streamed": (rp.forest(0, L, ML, T, 700, pnz, D, X, ctx=ctx, hyperplanes=R), Q)}
    data, queries, d = sparse_rows()
    cfg = rp.rpTreeCfg(ML, len(data[0]) - 1, d)
    out["csr"] = (rp.forestBatch(9, cfg.fpMaxTreeDepth, ML, T, cfg.fpProjNzDensity, d, data + (d,), ctx=ctx),
                  queries + (d,))
    yield out
    for f, _ in out.values():
        f.close()


# ------------------------------------------------------------------ A. lists
@pytest.mark.parametrize("mode", ["default", "slice7"])
@pytest.mark.parametrize("which", ["dense", "csr", "streamed"])
def test_lists(rp, ctx, forests, which, mode):
    """allowCandidates == numpy over candidatesBatch, offsets and ids, under every mask"""
    f, qs = forests[which]
    assert f.data.n % 32 != 0       # the tail word is a partial one
    off, cids = rp.candidatesBatch(f, qs)
    nq = (len(off) - 1) // T
    assert nq > 7 and nq % 7 != 0
    emptied = 0
    with option(ctx, "knn_allow_slice", 7 if mode == "slice7" else 0):
        ms = masks(f.data.n)
        hit = np.zeros(f.data.n, dtype=bool)         # one id that query 0 does reach
        hit[cids[0]] = True
        ms["one_reached"] = (hit, hit)
        for name, (allow, mask) in ms.items():
            woff, wids = ref.allowed_batch(off, cids, T, mask)
            goff, gids = rp.allowCandidates(allow, f, qs)
            assert np.array_equal(goff, woff), (name, np.flatnonzero(goff != woff)[:4])
            assert np.array_equal(gids, wids), name
            c, allowed, _ = rp.knnAllowLast(ctx)
            assert c == len(cids) and allowed == len(wids), name
            emptied += int((np.diff(woff) == 0).any() and len(wids) > 0)
        goff, gids = rp.allowCandidates(None, f, qs)
        assert np.array_equal(goff, off[::T]) and np.array_equal(gids, cids)
    if which == "dense":            # (the streamed forest's Tips are large: every list holds some allowed id)
        assert emptied > 0          # some query's list comes out empty next to non-empty ones


# ------------------------------------------------------------------ B. long lists
@pytest.fixture(scope="module")
def big(rp, ctx, oracle):
    n, d, trees, ml = 40000, 20, 13, 1500
    X = oracle.data_normal_dense2(11, n, d)
    Q = X[:64] * 1.002 + 0.004
    L, pnz, R = hyperplanes(oracle, n, d, ml, trees=trees)
    f = rp.forestBatch(0, L, ml, trees, pnz, d, X, ctx=ctx, hyperplanes=R, mode=rp.RPT_PROJ_EXACT)
    yield X, Q, f, trees
    f.close()


def test_long_lists(rp, ctx, big):
    """13 trees, leaves of 1 250: ~16 000 candidates per query, dozens of passes of the compaction's
    workgroup, ranges whose lengths are no multiple of 64; knnAllow against the restatement over
    candidatesBatch on metricDDL2's fold"""
    X, Q, f, trees = big
    off, cids = rp.candidatesBatch(f, Q)
    per_query = off[trees::trees] - off[:-1:trees]
    print("candidates per query: min %d median %d max %d" % (per_query.min(), np.median(per_query), per_query.max()))
    assert per_query.min() > 8 * 256 and (np.diff(off) % 64 != 0).any()
    ranked = []                     # every candidate entry of a query in (distance, position) order
    for i in range(len(Q)):
        c = cids[off[i * trees]:off[(i + 1) * trees]]
        dv = ref.l2_f64(X[c], Q[i])
        o = ref.rank(dv)
        ranked.append((c[o], dv[o]))
    ms = masks(len(X))
    for name, rule, k in (("half", ref.KEEP, 10), ("half", ref.EACH_ID_ONCE, 100), ("tenth", ref.EACH_ID_ONCE, 10),
                          ("hundredth", ref.ONE_PER_DISTANCE, 100), ("all", ref.KEEP, 100)):
        allow, mask = ms[name]
        ids, dist, cnt = rp.knnAllow(allow, k, f, Q, dedup=rule)
        for i, (ri, rd) in enumerate(ranked):
            wi, wd, wc = ref.from_ranked(ri, rd, mask, k, rule)
            assert cnt[i] == wc and np.array_equal(ids[i], wi), (name, rule, k, i)
            assert np.allclose(dist[i], wd, rtol=1e-12), (name, rule, k, i)
        c, allowed, _ = rp.knnAllowLast(ctx)
        assert c == per_query.sum() and allowed == int(mask[cids].sum()), name


# ------------------------------------------------------------------ C. every cell
RULE_ARG = {ref.KEEP: False, ref.EACH_ID_ONCE: True, ref.ONE_PER_DISTANCE: 2}


def check_cell(rp, ctx, f, qs, kw, k=10):
    """every id allowed: knnBatch's bits; 50 % / 10 %: the restatement over knnBatch(1024, dedup=False),
    the listing of every candidate entry with the cell's own distance bits in (distance, position) order"""
    assert rp.RPT_KNN_DEDUP_DISTANCE == RULE_ARG[ref.ONE_PER_DISTANCE]
    n = f.data.n
    off, _ = rp.candidatesBatch(f, qs)
    per_query = off[T::T] - off[:-1:T]
    assert per_query.max() <= 1024
    ms = masks(n)
    for rule, dedup in RULE_ARG.items():
        wi, wd, wc = rp.knnBatch(k, f, qs, dedup=dedup, **kw)
        for allow in (None, ms["all"][0], ref.bitmap(ms["all"][1], tail=True)):
            gi, gd, gc = rp.knnAllow(allow, k, f, qs, dedup=dedup, **kw)
            assert np.array_equal(gc, wc) and np.array_equal(gi, wi) and ref.same_bits(gd, wd), rule
    ai, ad, ac = rp.knnBatch(1024, f, qs, dedup=False, **kw)
    assert np.array_equal(ac, per_query)
    short = full = 0
    for name in ("half", "tenth"):
        allow, mask = ms[name]
        for rule, dedup in RULE_ARG.items():
            wi, wd, wc = ref.from_ranked_batch(ai, ad, ac, mask, k, rule)
            gi, gd, gc = rp.knnAllow(allow, k, f, qs, dedup=dedup, **kw)
            assert np.array_equal(gc, wc), (name, rule, np.flatnonzero(gc != wc)[:4])
            assert np.array_equal(gi, wi) and ref.same_bits(gd, wd), (name, rule)
            short += int((gc < k).sum())
            full += int((gc == k).sum())
    assert short > 0 and full > 0


def dense_cell(rp, ctx, oracle, dtype):
    """-> (device data set, what bruteKnn / compactRows take as host rows, queries)"""
    X, Q = dense_rows(oracle)
    if dtype == "f64":
        return rp.Dataset.dense(ctx, X), X, Q
    if dtype == "f32":
        X32 = X.astype(np.float32)
        return rp.Dataset.dense(ctx, X32), X32, Q.astype(np.float32)
    Xb = rp.to_bf16(X.astype(np.float32))
    return rp.Dataset.dense(ctx, Xb, dtype=rp.RPT_BF16), Xb, rp.from_bf16(rp.to_bf16(Q.astype(np.float32)))


def metric_kw(rp, metric):
    return {"l2": {}, "reference": {"reference_metric": True}, "cosine": {"metric": rp.metricCosine},
            "inner": {"metric": rp.metricInner}}[metric]


@pytest.mark.parametrize("metric", ["l2", "cosine", "inner"])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_dense_cells(rp, ctx, oracle, dtype, metric):
    ds, _, qs = dense_cell(rp, ctx, oracle, dtype)
    L, pnz, R = hyperplanes(oracle, N, D, ML)
    f = rp._build(ctx, ds, R.reshape(T, L, D), L, ML, rp.RPT_PROJ_AUTO)
    check_cell(rp, ctx, f, qs, metric_kw(rp, metric))
    f.close()
    ds.close()


@pytest.mark.parametrize("cell", ["l2", "reference", "cosine", "inner"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_csr_cells(rp, ctx, dtype, cell):
    rng = np.random.default_rng(55)
    n, d, nq = N, 24, 40
    data = csrref.random_csr(rng, n, d, 0.3, dtype)
    queries = tuple(a.copy() for a in csrref.random_csr(rng, nq, d, 0.3, dtype))
    cfg = rp.rpTreeCfg(ML, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, ML, T, cfg.fpProjNzDensity, d, data + (d,), ctx=ctx)
    check_cell(rp, ctx, f, queries + (d,), metric_kw(rp, cell))
    f.close()


# ------------------------------------------------------------------ D. exhaustive
def check_exhaustive(rp, ctx, ds, host_rows, qs, kw, k, names, bf16=False):
    """bruteKnnAllow == bruteKnn over compactRows(data, mask) with the ids mapped back: ids and bits"""
    n = ds.n
    ms = masks(n)
    wi, wd = rp.bruteKnn(ds, qs, k, **kw)
    gi, gd = rp.bruteKnnAllow(None, ds, qs, k, **kw)
    assert np.array_equal(gi, wi) and ref.same_bits(gd, wd)
    for name in names:
        allow, mask = ms[name]
        gi, gd = rp.bruteKnnAllow(allow, ds, qs, k, **kw)
        if not mask.any():
            assert (gi == -1).all() and np.isposinf(gd).all(), name
            continue
        sub = rp.compactRows(host_rows, mask)
        sds = (rp.Dataset.dense(ctx, sub, dtype=rp.RPT_BF16) if bf16 else
               rp.Dataset.csr(ctx, *sub) if isinstance(sub, tuple) else rp.Dataset.dense(ctx, sub))
        wi, wd = rp.bruteKnn(sds, qs, k, **kw)
        sds.close()
        assert np.array_equal(gi, ref.map_back(wi, mask)), (name, np.flatnonzero((gi != ref.map_back(wi, mask)).any(1))[:4])
        assert ref.same_bits(gd, wd), name
        m = min(k, int(mask.sum()))
        assert (gi[:, :m] >= 0).all() and (gi[:, m:] == -1).all() and np.isposinf(gd[:, m:]).all(), name


ALL_MASKS = ("half", "tenth", "hundredth", "all", "none", "one", "last_word", "tail_bits")


@pytest.mark.parametrize("metric", ["l2", "cosine", "inner"])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_exhaustive_dense(rp, ctx, oracle, dtype, metric):
    ds, host_rows, qs = dense_cell(rp, ctx, oracle, dtype)
    check_exhaustive(rp, ctx, ds, host_rows, qs, metric_kw(rp, metric), 10, ALL_MASKS, bf16=dtype == "bf16")
    ds.close()


def test_exhaustive_scan_over_several_workgroups(rp, ctx, big):
    """40 000 rows: 1 250 bitmap words, five blocks of the list kernels"""
    X, Q, f, _ = big
    for metric in ("l2", "inner"):
        check_exhaustive(rp, ctx, f.data, X, Q[:16], metric_kw(rp, metric), 10, ("half", "hundredth", "last_word", "tail_bits"))


@pytest.mark.parametrize("cell", ["reference", "cosine", "inner"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_exhaustive_csr(rp, ctx, dtype, cell):
    data, queries, d = sparse_rows()
    data = (data[0], data[1], data[2].astype(dtype))
    queries = (queries[0], queries[1], queries[2].astype(dtype))
    ds = rp.Dataset.csr(ctx, *data, d)
    check_exhaustive(rp, ctx, ds, data + (d,), queries + (d,), metric_kw(rp, cell), 10, ALL_MASKS)
    ds.close()


def left_out(Dm, k):
    """test_gpu_brute_csr's count of (query, position) pairs whose truth is not separated from both
    neighbours by more than 1e-9 relative, from the numpy truth alone"""
    nq, n = Dm.shape
    m = min(k, n)
    left = 0
    for i in range(nq):
        td = np.sort(Dm[i], kind="stable")[:m + 1]
        gap = np.diff(td) > 1e-9 * td[1:]
        right = np.ones(m, dtype=bool)
        right[:len(gap)] = gap[:m]
        leftn = np.ones(m, dtype=bool)
        leftn[1:] = gap[:m - 1]
        left += int((~(right & leftn)).sum())
    return left, nq * m


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_exhaustive_csr_true_l2(rp, ctx, oracle, dtype):
    """true L2 on CSR rows is the brute force's tolerance-mode distance (the tiled kernel behind its
    allow switch): held to tests/test_gpu_brute_csr.py's rule against numpy over the allowed rows,
    stored rows as queries included (distance exactly 0 where the row is allowed)"""
    n, d, density = 3000, 30, 0.3
    rowptr, col, val = oracle.data_normal_sparse2(5, n, d, density)
    val = val.astype(dtype)
    qr, qc, qv = brute_csr.queries_with_stored_rows(oracle, (rowptr, col, val), d, density, 64, 6)
    qv = qv.astype(dtype)
    Dall = brute_csr.true_distances(brute_csr.densify(rowptr, col, val, d), brute_csr.densify(qr, qc, qv, d))
    ds = rp.Dataset.csr(ctx, rowptr, col, val, d)
    for name, (allow, mask) in masks(n).items():
        allowed = np.flatnonzero(mask)
        newid = np.full(n + 1, -1, dtype=np.int64)          # (index -1 -> the last slot: -1 stays -1)
        newid[allowed] = np.arange(len(allowed))
        Dm = Dall[:, allowed]
        for k in (1, 10, 25):
            left, pairs = left_out(Dm, k)                   # before the device answer is looked at
            assert left <= 0.01 * pairs, (name, k, left, pairs)
            ids, dist = rp.bruteKnnAllow(allow, ds, (qr, qc, qv, d), k)
            assert (mask[ids[ids >= 0]]).all(), (name, k)
            got_left, got_pairs = brute_csr.check_l2(newid[ids].astype(np.int32), dist, Dm, k, (name, k))
            assert (got_left, got_pairs) == (left, pairs)
    ds.close()


# ------------------------------------------------------------------ E. recall
@pytest.mark.parametrize("which", ["dense", "csr"])
def test_recall(rp, ctx, forests, which):
    f, qs = forests[which]
    off, cids = rp.candidatesBatch(f, qs)
    nq = (len(off) - 1) // T
    k = 10
    distf = rp.metricL2 if which == "dense" else rp.metricInner
    for name in ("half", "tenth", "one", "none", "all"):
        allow, mask = masks(f.data.n)[name]
        truth, _ = rp.bruteKnnAllow(allow, f, qs, k, metric=distf)
        hits, got_truth = rp.recallHitsAllow(allow, distf, f, k, qs)
        assert np.array_equal(got_truth, truth), name
        want = np.array([[len(np.intersect1d(cids[off[i * T + t]:off[i * T + t + 1]], truth[i][truth[i] >= 0]))
                          for t in range(T)] for i in range(nq)], dtype=np.int32)
        assert np.array_equal(hits, want), name
        rec = rp.recallWithAllowBatch(allow, distf, f, k, qs)
        assert np.array_equal(rec, np.array([sum(h / k for h in row) / T for row in want.tolist()])), name
    hits, truth = rp.recallHitsAllow(None, distf, f, k, qs)
    whits, wtruth = rp.recallHits(distf, f, k, qs)
    assert np.array_equal(hits, whits) and np.array_equal(truth, wtruth)


# ------------------------------------------------------------------ F. device arrays
@pytest.mark.parametrize("which", ["dense", "csr"])
def test_dev_equals_host(rp, ctx, forests, which):
    import torch
    f, qs = forests[which]
    kw = {} if which == "dense" else {"metric": rp.metricInner}
    k = 7
    allow, mask = masks(f.data.n)["half"]
    words = ref.bitmap(mask)
    wi, wd, wc = rp.knnAllow(allow, k, f, qs, dedup=True, **kw)
    bi, bd = rp.bruteKnnAllow(allow, f, qs, k, **kw)
    dev = torch.device("cuda", 0)
    tw = torch.from_numpy(words.view(np.int32).copy()).to(dev)
    if which == "dense":
        tq = torch.from_numpy(np.ascontiguousarray(qs)).to(dev)
        qd = rp.Dataset.from_torch(ctx, tq)
        nq = len(qs)
    else:
        rowptr, col, val, d = qs
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rowptr, col, val)]
        qd = rp.Dataset.csr_from_torch(ctx, keep[0], keep[1], keep[2], d)
        nq = len(rowptr) - 1
    for ptr, (hi, hd, hc), (hbi, hbd) in ((tw.data_ptr(), (wi, wd, wc), (bi, bd)),
                                         (0, rp.knnAllow(None, k, f, qs, dedup=True, **kw),
                                          rp.bruteKnnAllow(None, f, qs, k, **kw))):
        ids = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
        dist = torch.zeros((nq, k), dtype=torch.float64, device=dev)
        cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rp.knnAllowDev(ptr, k, f, qd, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), dedup=True, **kw)
        ctx.sync()
        assert np.array_equal(cnt.cpu().numpy(), hc) and np.array_equal(ids.cpu().numpy(), hi)
        assert ref.same_bits(dist.cpu().numpy(), hd)
        ids.fill_(-7)
        dist.zero_()
        torch.cuda.synchronize()
        rp.bruteKnnAllowDev(ptr, f.data, qd, k, ids.data_ptr(), dist.data_ptr(), **kw)
        ctx.sync()
        assert np.array_equal(ids.cpu().numpy(), hbi) and ref.same_bits(dist.cpu().numpy(), hbd)


# ------------------------------------------------------------------ G. refusals
def test_refusals_leave_the_context_usable(rp, ctx, forests):
    from rptree_amd import _lib
    L = _lib.lib()
    f, Q = forests["dense"]
    fc, qc = forests["csr"]
    qd, nq = rp._query_dataset(ctx, f.data, Q)
    q32 = rp.Dataset.dense(ctx, Q.astype(np.float32))
    qcd, nqc = rp._query_dataset(ctx, fc.data, qc)
    k = 5
    ids = np.empty((max(nq, nqc), k), dtype=np.int32)
    dist = np.empty((max(nq, nqc), k))
    cnt = np.empty(max(nq, nqc), dtype=np.int32)
    hits = np.empty((max(nq, nqc), T), dtype=np.int32)

    def knn(forest, q, flags, kk=k):
        return L.rpt_knn_allow_host(ctx._h, forest._h, forest.data._h, q._h, None, kk, flags, rp._vp(ids), rp._vp(dist),
                                    rp._vp(cnt))

    def brute(forest, q, flags, kk=k):
        return L.rpt_brute_knn_allow_host(ctx._h, forest.data._h, q._h, None, kk, flags, rp._vp(ids), rp._vp(dist))

    def recall(forest, q, flags, kk=k):
        return L.rpt_recall_hits_allow_host(ctx._h, forest._h, forest.data._h, q._h, None, kk, flags, rp._vp(hits), None)
    cos, inn, refm = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE
    for forest, q, flags in ((f, qd, 2 << 8), (fc, qcd, inn | (3 << 8)), (f, qd, rp.RPT_KNN_DEDUP | (1 << 8))):
        assert knn(forest, q, flags) == RPT_E_UNSUPPORTED, hex(flags)      # a RPT_KNN_VOTE field
        assert L.rpt_last_error()
    bad = [(f, qd, refm), (f, qd, refm | 1),                              # the CSR metric on dense rows
           (f, qd, cos | inn), (fc, qcd, cos | refm), (fc, qcd, inn | refm),   # two metric bits
           (f, qd, 3), (fc, qcd, cos | 3),                                  # both duplicate bits
           (f, qcd, 0), (fc, qd, 0), (f, q32, 0)]                           # dense / CSR and f64 / f32 pairs
    for forest, q, flags in bad:
        assert knn(forest, q, flags) == RPT_E_ARG, hex(flags)
        assert L.rpt_last_error()
    assert knn(f, qd, 0, kk=1025) == RPT_E_ARG and knn(f, qd, 0, kk=0) == RPT_E_ARG
    for call in (brute, recall):
        for forest, q, flags in ((f, qd, refm), (f, qd, cos | inn), (fc, qcd, cos | refm), (f, qd, 1), (f, qd, 2 << 8),
                                 (f, qcd, 0), (fc, qd, 0), (f, q32, 0)):
            assert call(forest, q, flags) == RPT_E_ARG, (call.__name__, hex(flags))
        assert call(f, qd, 0, kk=1025) == RPT_E_ARG and call(f, qd, 0, kk=0) == RPT_E_ARG
    with pytest.raises(ValueError):
        rp.knnAllow(None, k, f, Q, reference_metric=True)
    with pytest.raises(ValueError):
        rp.bruteKnnAllow(None, fc, qc, k, metric=rp.metricCosine, reference_metric=True)
    with pytest.raises(ValueError):
        rp.knnAllow(np.ones(N + 1, dtype=bool), k, f, Q)
    # the context answers as before
    allow, mask = masks(N)["half"]
    off, cids = rp.candidatesBatch(f, Q)
    goff, gids = rp.allowCandidates(allow, f, Q)
    woff, wids = ref.allowed_batch(off, cids, T, mask)
    assert np.array_equal(goff, woff) and np.array_equal(gids, wids)
    assert knn(f, qd, 0) == 0 and knn(fc, qcd, refm | 1) == 0 and knn(fc, qcd, cos | 2) == 0
    assert brute(f, qd, inn) == 0 and brute(fc, qcd, refm) == 0 and brute(fc, qcd, cos) == 0 and recall(f, qd, 0) == 0
    tier, retries = _lib.C.c_int32(-1), _lib.C.c_int64(-1)
    assert knn(f, qd, 0) == 0
    assert L.rpt_knn_last_tier(ctx._h, _lib.C.byref(tier)) == 0 and tier.value == 0
    assert L.rpt_knn_last_retries(ctx._h, _lib.C.byref(retries)) == 0 and retries.value == 0


# ------------------------------------------------------------------ I. the C++ mirror
def test_cpp_knn_allow_example(tmp_path):
    """host/example_knn_allow.cpp: allowCandidates, knnAllow, bruteKnnAllow and recallHitsAllow of the C++
    mirror on SVector rows against its own host restatement"""
    exe = str(tmp_path / "example_knn_allow")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_allow.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src, "-L" + lib,
                           "-lrptree_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "3000", "40", "0.25", "6", "30", "12", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
