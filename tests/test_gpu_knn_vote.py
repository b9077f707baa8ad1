"""Vote-threshold kNN for every row layout and distance (rpt_knn_vote_*, rpt_vote_candidates_host)
on the device against the numpy restatement tests/knn_vote_ref.py: the voted lists on both paths of
the vote-select kernel and across the slice seam, queries above the old path's 16 384 candidates,
the old path's bits where it answers, every (layout, dtype, distance) cell, ties wider than k + 8,
the refusals, the device entry point and poisoned scratch."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_f32_ref as f32ref
import knn_metric_csr_ref as csrref
import knn_vote_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPT_E_ARG = -1
N, D, T, ML = 3000, 12, 6, 20
VS = (1, 2, 3, T, T + 1)


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


# ------------------------------------------------------------------ H. poisoned scratch (first: the
# children start before this module's own GPU calls)
POISON_NODES = ["tests/test_gpu_pool_poison.py::test_pool_probe_sees_the_poison",
                "tests/test_gpu_knn_vote.py::test_lists[dense-lds_median]",
                "tests/test_gpu_knn_vote.py::test_above_the_old_cap"]


def test_no_slab_word_is_read_unwritten():
    """one case of A (both paths of the kernel) and B (global slabs padded to 32 768) in a fresh
    child whose allocator fills every block with 0xff: an unwritten sort or id word read anywhere
    would be id -1 or sort last and change the lists"""
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
@pytest.mark.parametrize("mode", ["default", "lds_median", "slice7"])
@pytest.mark.parametrize("which", ["dense", "csr", "streamed"])
def test_lists(rp, ctx, forests, which, mode):
    """voteCandidates == numpy over candidatesBatch, ids and counts, for every threshold"""
    f, qs = forests[which]
    off, cids = rp.candidatesBatch(f, qs)
    nq = (len(off) - 1) // T
    per_query = off[T::T] - off[:-1:T]
    assert len(per_query) == nq
    name, value = "knn_vote_lds", 0
    if mode == "lds_median":
        value = int(np.median(per_query))
        assert (per_query <= value).any() and (per_query > value).any() and value >= 1
    elif mode == "slice7":
        name, value = "knn_vote_slice", 7
        assert nq > 7 and nq % 7 != 0
    emptied = 0
    with option(ctx, name, value):
        for v in VS:
            woff, wids, wcnt = ref.voted_batch(off, cids, T, v)
            goff, gids, gcnt = rp.voteCandidates(f, qs, v)
            assert np.array_equal(goff, woff), (v, np.flatnonzero(goff != woff)[:4])
            assert np.array_equal(gids, wids) and np.array_equal(gcnt, wcnt), v
            if v <= 3:
                emptied += int(woff[-1] == woff[-2])
            c, voted, _ = rp.knnVoteLast(ctx)
            assert c == len(cids) and voted == len(wids), v
    if which == "dense":
        assert emptied > 0          # the last query has no voted id at some v <= 3


# ------------------------------------------------------------------ B. above the old cap
@pytest.fixture(scope="module")
def big(rp, ctx, oracle):
    n, d, trees, ml = 40000, 20, 13, 1500
    X = oracle.data_normal_dense2(11, n, d)
    Q = X[:64] * 1.002 + 0.004
    L, pnz, R = hyperplanes(oracle, n, d, ml, trees=trees)
    f = rp.forestBatch(0, L, ml, trees, pnz, d, X, ctx=ctx, hyperplanes=R, mode=rp.RPT_PROJ_EXACT)
    ff = oracle.Forest(n, d, R, L, ml, f.perm, f.thr, f.mglo, f.mghi)   # the device's own forest
    yield X, Q, f, ff, trees
    f.close()


def test_above_the_old_cap(rp, ctx, oracle, big):
    """13 trees, leaves of 1 250: queries on both sides of 16 384 candidates in one batch; the old
    flag refuses the batch, the new entry point is the oracle's voting kNN, k = 100 included"""
    X, Q, f, ff, trees = big
    off, _ = rp.candidatesBatch(f, Q)
    per_query = off[trees::trees] - off[:-1:trees]
    print("candidates per query: min %d median %d max %d" % (per_query.min(), np.median(per_query), per_query.max()))
    assert (per_query <= 16384).any() and (per_query > 16384).any()
    with pytest.raises(rp.RPTError):
        rp.knnBatch(10, f, Q, vote=2)
    for k in (10, 100):
        ids, dist, cnt = rp.knnVote(k, f, Q, 2)
        wi, wd, wc = oracle.knn_dense_batch(ff, X, Q, k, vote_thr=2, threads=4)
        assert np.array_equal(cnt, wc) and np.array_equal(ids, wi), k
        assert np.allclose(dist, wd, rtol=1e-12), k
    c, voted, _ = rp.knnVoteLast(ctx)
    assert c == per_query.sum() and 0 < voted < c


# ------------------------------------------------------------------ C. the old path's bits
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_same_bits_as_the_old_flag(rp, ctx, oracle, dtype):
    n, d, trees, ml, k = 20000, 20, 12, 60, 10
    X = oracle.data_normal_dense2(11, n, d)
    Q = X[:100] * 1.002 + 0.004
    if dtype == "f32":
        X, Q = X.astype(np.float32), Q.astype(np.float32)
    L, pnz, R = hyperplanes(oracle, n, d, ml, trees=trees)
    f = rp.forestBatch(0, L, ml, trees, pnz, d, X, ctx=ctx, hyperplanes=R)
    for v in (1, 2, 3, 6):
        wi, wd, wc = rp.knnBatch(k, f, Q, vote=v)
        gi, gd, gc = rp.knnVote(k, f, Q, v)
        assert np.array_equal(gc, wc) and np.array_equal(gi, wi), v
        assert ref.same_bits(gd, wd), v
    f.close()


# ------------------------------------------------------------------ D. every cell
def lookup_restated(off, cids, trees, v, k, all_ids, all_dist, all_cnt):
    """the restatement over the numpy voted lists, every distance looked up in the answer of the
    cell's NON-voting entry point with k above the candidate count (each id once)"""
    def distance(i, ids):
        m = all_cnt[i]
        order = np.argsort(all_ids[i, :m])
        at = np.searchsorted(all_ids[i, :m][order], ids)
        assert np.array_equal(all_ids[i, :m][order][at], ids)
        return all_dist[i, :m][order][at]
    return ref.knn_vote_batch(off, cids, trees, v, distance, k)


def check_cell(rp, ctx, f, qs, kw, k=10):
    """v = 1 is knnBatch(dedup=True) of the cell; v = 2, 3 rank the numpy voted lists on that entry
    point's own distances -> the lists, for the cell's independent reference"""
    off, cids = rp.candidatesBatch(f, qs)
    per_query = off[T::T] - off[:-1:T]
    assert per_query.max() <= 1024
    wi, wd, wc = rp.knnBatch(k, f, qs, dedup=True, **kw)
    gi, gd, gc = rp.knnVote(k, f, qs, 1, **kw)
    assert np.array_equal(gc, wc) and np.array_equal(gi, wi)
    assert ref.same_bits(gd, wd)
    ai, ad, ac = rp.knnBatch(1024, f, qs, dedup=True, **kw)
    answers = {}
    for v in (2, 3):
        wi, wd, wc = lookup_restated(off, cids, T, v, k, ai, ad, ac)
        gi, gd, gc = rp.knnVote(k, f, qs, v, **kw)
        assert np.array_equal(gc, wc), v
        assert np.array_equal(gi, wi) and ref.same_bits(gd, wd), v
        assert (gc > 0).any()
        answers[v] = (gi, gd, gc)
    return off, cids, answers


@pytest.mark.parametrize("metric", ["l2", "cosine", "inner"])
@pytest.mark.parametrize("dtype", ["f64", "f32", "bf16"])
def test_dense_cells(rp, ctx, oracle, dtype, metric):
    X, Q = dense_rows(oracle)
    L, pnz, R = hyperplanes(oracle, N, D, ML)
    if dtype == "f64":
        Xh, Qh, ds, qs = X, Q, rp.Dataset.dense(ctx, X), Q
    elif dtype == "f32":
        qs = Q.astype(np.float32)
        Xh, Qh, ds = X.astype(np.float32).astype(np.float64), qs.astype(np.float64), rp.Dataset.dense(ctx, X.astype(np.float32))
    else:
        Xb = rp.to_bf16(X.astype(np.float32))
        qs = rp.from_bf16(rp.to_bf16(Q.astype(np.float32)))
        Xh, Qh = rp.from_bf16(Xb).astype(np.float64), qs.astype(np.float64)
        ds = rp.Dataset.dense(ctx, Xb, dtype=rp.RPT_BF16)
    f = rp._build(ctx, ds, R.reshape(T, L, D), L, ML, rp.RPT_PROJ_AUTO)
    kw = {} if metric == "l2" else {"metric": rp.metricCosine if metric == "cosine" else rp.metricInner}
    k = 10
    off, cids, answers = check_cell(rp, ctx, f, qs, kw, k)
    gi, gd, gc = answers[2]
    for i in range(len(Q)):
        vids, _ = ref.voted(cids[off[i * T]:off[(i + 1) * T]], 2)
        if metric != "l2":            # the left-fold dot of the exactly widened rows: ids and bits
            wi, wd, wc = ref.first_k(vids, ref.metric_dense(metric, Xh[vids], Qh[i]), k)
            assert gc[i] == wc and np.array_equal(gi[i], wi) and ref.same_bits(gd[i], wd), i
        elif dtype == "f64":
            wi, wd, wc = ref.first_k(vids, ref.l2_f64(Xh[vids], Qh[i]), k)
            assert gc[i] == wc and np.array_equal(gi[i], wi), i
            assert np.allclose(gd[i, :wc], wd[:wc], rtol=1e-12), i
        else:                         # the f32 sum: everything its bound and the definition imply
            f32ref.check_interval(vids, f32ref.exact_dist(Xh[vids], Qh[i]) if len(vids) else np.zeros(0),
                                  gi[i], gd[i], gc[i], k, f32ref.KEEP, D)
    f.close()
    ds.close()


@pytest.mark.parametrize("cell", ["l2", "reference", "cosine", "inner"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_csr_cells(rp, ctx, oracle, dtype, cell):
    rng = np.random.default_rng(55)
    n, d, nq, k = N, 24, 40, 10
    data = csrref.random_csr(rng, n, d, 0.3, dtype)
    queries = tuple(a.copy() for a in csrref.random_csr(rng, nq, d, 0.3, dtype))
    cfg = rp.rpTreeCfg(ML, n, d)
    f = rp.forestBatch(9, cfg.fpMaxTreeDepth, ML, T, cfg.fpProjNzDensity, d, data + (d,), ctx=ctx)
    kw = {"l2": {}, "reference": {"reference_metric": True}, "cosine": {"metric": rp.metricCosine},
          "inner": {"metric": rp.metricInner}}[cell]
    off, cids, answers = check_cell(rp, ctx, f, queries + (d,), kw, k)
    gi, gd, gc = answers[2]
    X, P = csrref.dense(*data, d)
    Qd, QP = csrref.dense(*queries, d)
    Xd = (X, P, csrref.self_dots(X, P))
    row = lambda c, i: (c[1][c[0][i]:c[0][i + 1]], c[2][c[0][i]:c[0][i + 1]])
    for i in range(nq):
        vids, _ = ref.voted(cids[off[i * T]:off[(i + 1) * T]], 2)
        if cell in ("cosine", "inner"):     # dotS: ids and bits (the ids are distinct and ascending)
            wi, wd, wc = csrref.knn_candidates(cell, Xd, vids, Qd[i], QP[i], k, 0)
            assert gc[i] == wc and np.array_equal(gi[i], wi) and ref.same_bits(gd[i], wd), i
        elif cell == "reference":           # the oracle's truncating metricSSL2, pair by pair: bits
            dv = np.array([oracle.metric_ss(*row(data, j), *row(queries, i)) for j in vids])
            wi, wd, wc = ref.first_k(vids, dv, k)
            assert gc[i] == wc and np.array_equal(gi[i], wi) and ref.same_bits(gd[i], wd), i
        else:                               # true L2: 1e-8 |q| absolute; ids where that separates them
            dv = np.sqrt(((X[vids] - Qd[i][None, :]) ** 2).sum(axis=1))
            wi, wd, wc = ref.first_k(vids, dv, k)
            tol = 1e-8 * max(np.linalg.norm(Qd[i]), 1.0)
            assert gc[i] == wc, i
            assert np.all(np.abs(gd[i, :wc] - wd[:wc]) <= tol), i
            sd = np.sort(dv)
            if wc and not (np.diff(sd[:wc + 1]) <= 2 * tol).any():
                assert np.array_equal(gi[i], wi), i
    f.close()


# ------------------------------------------------------------------ E. ties
def test_ties_wider_than_the_margin(rp, ctx):
    """rows in {0, 1}^4: 16 different rows, ~125 copies of each — far more than k + 8 rows tie at
    the cut; the answer is (distance, id) bit for bit and the exact kernel gave it; under cosine
    the zero rows are NaN and rank last by id"""
    rng = np.random.default_rng(3)
    n, d, k, trees = 2000, 4, 10, 4
    X = rng.integers(0, 2, (n, d)).astype(np.float64)
    Q = np.concatenate([X[:12], rng.integers(0, 2, (4, d)).astype(np.float64) + 0.5])
    f = rp.forestBatch(7, 3, 100, trees, 1.0, d, X, ctx=ctx)
    off, cids = rp.candidatesBatch(f, Q)
    for v in (1, 2):
        wi, wd, wc = ref.knn_vote_batch(off, cids, trees, v, lambda i, ids: ref.l2_f64(X[ids], Q[i]), k)
        gi, gd, gc = rp.knnVote(k, f, Q, v)
        unc = rp.knnVoteLast(ctx)[2]
        assert np.array_equal(gc, wc) and np.array_equal(gi, wi) and ref.same_bits(gd, wd), v
        assert unc > 0, v
    k = 1024                                 # every voted id is ranked: the NaN distances of the zero rows too
    wi, wd, wc = ref.knn_vote_batch(off, cids, trees, 1, lambda i, ids: ref.metric_dense("cosine", X[ids], Q[i]), k)
    gi, gd, gc = rp.knnVote(k, f, Q, 1, metric=rp.metricCosine)
    assert np.isnan(wd[np.arange(len(Q)), np.maximum(wc - 1, 0)]).any()
    assert np.array_equal(gc, wc) and np.array_equal(gi, wi) and ref.same_bits(gd, wd)
    f.close()


# ------------------------------------------------------------------ F. refusals
def test_refusals_leave_the_context_usable(rp, ctx, forests):
    from rptree_amd import _lib
    L = _lib.lib()
    f, Q = forests["dense"]
    fc, qc = forests["csr"]
    qd, nq = rp._query_dataset(ctx, f.data, Q)
    qcd, nqc = rp._query_dataset(ctx, fc.data, qc)
    k = 5
    ids = np.empty((max(nq, nqc), k), dtype=np.int32)
    dist = np.empty((max(nq, nqc), k))
    cnt = np.empty(max(nq, nqc), dtype=np.int32)

    def call(forest, q, v, flags, kk=k):
        return L.rpt_knn_vote_host(ctx._h, forest._h, forest.data._h, q._h, kk, v, flags, rp._vp(ids), rp._vp(dist),
                                   rp._vp(cnt))
    cos, inn, refm = rp.RPT_KNN_METRIC_COSINE, rp.RPT_KNN_METRIC_INNER, rp.RPT_KNN_METRIC_REFERENCE
    bad = [(f, qd, 0, 0), (f, qd, 65536, 0), (f, qd, -1, 0),                 # v out of [1, 65535]
           (f, qd, 2, cos | inn), (fc, qcd, 2, cos | refm), (fc, qcd, 2, inn | refm),   # two metric bits
           (f, qd, 2, refm),                                                  # the CSR metric on dense data
           (f, qd, 2, rp.RPT_KNN_DEDUP), (f, qd, 2, rp.RPT_KNN_DEDUP_DISTANCE), (fc, qcd, 2, cos | 1),
           (f, qd, 2, 2 << 8), (fc, qcd, 2, inn | (3 << 8)),                  # a RPT_KNN_VOTE field
           (f, qcd, 2, 0), (fc, qd, 2, 0)]                                    # a dense / CSR pair
    for forest, q, v, flags in bad:
        assert call(forest, q, v, flags) == RPT_E_ARG, (v, hex(flags))
        assert L.rpt_last_error()
    assert call(f, qd, 2, 0, kk=1025) == RPT_E_ARG and call(f, qd, 2, 0, kk=0) == RPT_E_ARG
    total = _lib.C.c_int64()
    assert L.rpt_vote_candidates_host(ctx._h, f._h, qd._h, 0, None, None, None, 0, _lib.C.byref(total)) == RPT_E_ARG
    with pytest.raises(ValueError):
        rp.knnVote(k, f, Q, 2, reference_metric=True)
    with pytest.raises(ValueError):
        rp.knnVote(k, fc, qc, 2, metric=rp.metricCosine, reference_metric=True)
    # the context answers as before
    off, cids = rp.candidatesBatch(f, Q)
    goff, gids, gcnt = rp.voteCandidates(f, Q, 2)
    woff, wids, wcnt = ref.voted_batch(off, cids, T, 2)
    assert np.array_equal(goff, woff) and np.array_equal(gids, wids) and np.array_equal(gcnt, wcnt)
    assert call(f, qd, 2, 0) == 0 and call(fc, qcd, 2, refm) == 0


# ------------------------------------------------------------------ G. device arrays
@pytest.mark.parametrize("which", ["dense", "csr"])
def test_dev_equals_host(rp, ctx, forests, which):
    import torch
    f, qs = forests[which]
    kw = {} if which == "dense" else {"metric": rp.metricInner}
    k = 7
    wi, wd, wc = rp.knnVote(k, f, qs, 2, **kw)
    dev = torch.device("cuda", 0)
    if which == "dense":
        tq = torch.from_numpy(np.ascontiguousarray(qs)).to(dev)
        qd = rp.Dataset.from_torch(ctx, tq)
        nq = len(qs)
    else:
        rowptr, col, val, d = qs
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rowptr, col, val)]
        qd = rp.Dataset.csr_from_torch(ctx, keep[0], keep[1], keep[2], d)
        nq = len(rowptr) - 1
    ids = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    dist = torch.zeros((nq, k), dtype=torch.float64, device=dev)
    cnt = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rp.knnVoteDev(k, f, qd, 2, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), **kw)
    ctx.sync()
    assert np.array_equal(cnt.cpu().numpy(), wc) and np.array_equal(ids.cpu().numpy(), wi)
    assert ref.same_bits(dist.cpu().numpy(), wd)


# ------------------------------------------------------------------ the C++ mirror
def test_cpp_knn_vote_example(tmp_path):
    """host/example_knn_vote.cpp: knnVote and voteCandidates of the C++ mirror on SVector rows against
    its own host restatement"""
    exe = str(tmp_path / "example_knn_vote")
    src = os.path.join(ROOT, "rp-tree_amd", "host", "example_knn_vote.cpp")
    lib = os.path.join(ROOT, "rp-tree_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src, "-L" + lib,
                           "-lrptree_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "3000", "40", "0.25", "6", "30", "12", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
