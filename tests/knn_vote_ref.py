"""numpy restatement of the vote-threshold kNN (include/rptree_hip.h, rpt_knn_vote_*), shared by
tests/test_knn_vote_host.py (no GPU) and tests/test_gpu_knn_vote.py.  Not a test module.

The definition: a query's candidates are the entries of all T trees' lists; count(id) = the number
of entries equal to id; the voted list = the ids with count >= v, ascending, each once (keepCounts'
order, RPTree.hs:464-478); the answer = the first k of the voted list by (distance, id), NaN last,
unused slots id -1 and distance +inf, count = min(k, number of voted ids)."""
import numpy as np


def voted(cands, v):
    """-> (ids ascending, counts) of the ids that at least v entries of cands carry"""
    ids, c = np.unique(np.asarray(cands, dtype=np.int64), return_counts=True)
    keep = c >= v
    return ids[keep].astype(np.int32), c[keep].astype(np.int32)


def voted_batch(off, cids, T, v):
    """candidatesBatch's (off[nq*T+1], ids) -> (off[nq+1], ids, counts) of the voted lists"""
    nq = (len(off) - 1) // T
    out_off = np.zeros(nq + 1, dtype=np.int64)
    parts_i, parts_c = [], []
    for i in range(nq):
        vi, vc = voted(cids[off[i * T]:off[(i + 1) * T]], v)
        parts_i.append(vi)
        parts_c.append(vc)
        out_off[i + 1] = out_off[i] + len(vi)
    cat = lambda p: np.concatenate(p) if p else np.zeros(0, dtype=np.int32)
    return out_off, cat(parts_i).astype(np.int32), cat(parts_c).astype(np.int32)


def first_k(ids, dist, k):
    """the first k of (ids ascending, their distances) by (distance, id), NaN last ->
    (ids[k], dist[k], count)"""
    ids = np.asarray(ids, dtype=np.int32)
    dist = np.asarray(dist, dtype=np.float64)
    assert ids.shape == dist.shape and np.all(np.diff(ids) > 0)
    nan = np.isnan(dist)
    order = np.lexsort((ids, np.where(nan, 0.0, dist), nan))[:k]
    cnt = len(order)
    oi = np.full(k, -1, dtype=np.int32)
    od = np.full(k, np.inf)
    oi[:cnt], od[:cnt] = ids[order], dist[order]
    return oi, od, cnt


def knn_vote(cands, v, distance, k):
    """one query: distance(ids) -> the distances of those rows to the query"""
    ids, _ = voted(cands, v)
    return first_k(ids, distance(ids) if len(ids) else np.zeros(0), k)


def knn_vote_batch(off, cids, T, v, distance, k):
    """distance(i, ids) -> distances of rows `ids` to query i; -> (ids[nq][k], dist[nq][k], count[nq])"""
    nq = (len(off) - 1) // T
    oi = np.empty((nq, k), dtype=np.int32)
    od = np.empty((nq, k))
    oc = np.empty(nq, dtype=np.int32)
    for i in range(nq):
        oi[i], od[i], oc[i] = knn_vote(cids[off[i * T]:off[(i + 1) * T]], v, lambda ids: distance(i, ids), k)
    return oi, od, oc


# ------------------------------------------------------------------ the distances of the cells
def l2_f64(X, q):
    """metricDDL2 (Internal.hs:384-388 restated): the left fold of the squared differences, sqrt"""
    t = np.asarray(X, dtype=np.float64) - np.asarray(q, dtype=np.float64)[None, :]
    P = np.concatenate([np.zeros((t.shape[0], 1)), t * t], axis=1)
    return np.sqrt(np.cumsum(P, axis=1)[:, -1])


def fold_dots(X, q):
    """innerDD: the left fold ((0 + x0 q0) + x1 q1) + ... of every row of X with q"""
    P = np.asarray(X, dtype=np.float64) * np.asarray(q, dtype=np.float64)[None, :]
    P = np.concatenate([np.zeros((P.shape[0], 1)), P], axis=1)
    return np.cumsum(P, axis=1)[:, -1]


def metric_dense(metric, X, q):
    """RPT_KNN_METRIC_INNER / _COSINE on exactly widened dense rows ("inner" / "cosine")"""
    dot = fold_dots(X, q)
    if metric == "inner":
        return -dot
    xx = np.array([fold_dots(x[None, :], x)[0] for x in np.asarray(X, dtype=np.float64)]) if len(X) else np.zeros(0)
    qq = fold_dots(np.asarray(q, dtype=np.float64)[None, :], q)[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return 1.0 - dot / (np.sqrt(xx) * np.sqrt(qq))


def same_bits(a, b):
    """bit-equal doubles; a NaN only has to be a NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64),
                                                                            b[~nb].view(np.uint64))
