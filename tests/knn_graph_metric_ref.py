"""numpy restatement of the kNN graph and its refinement under the cosine and inner-product
distances (include/rptree_hip.h, rpt_knn_graph_metric_* / rpt_knn_graph_refine_metric_*), shared by
tests/test_knn_graph_metric_host.py and the two GPU test modules.  Not a test module.

dot(a, b) = ((0 + a0 b0) + a1 b1) + ... in double, every product and sum rounded on its own;
inner: -dot(x_i, x_j); cosine: 1 - dot(x_i, x_j) / (sqrt(dot(x_i, x_i)) * sqrt(dot(x_j, x_j))).
Mates and the order (distance, id), NaN last, are knn_graph_ref's; a refinement round is
knn_graph_refine_ref.refine_round with the distance matrix handed in."""
import numpy as np

import knn_graph_ref as ref
import knn_graph_refine_ref as rref

METRICS = ("cosine", "inner")


def dot_fold(a, B):
    """dot(a, b) for every row b of B: np.cumsum adds in order, from the leading +0.0"""
    with np.errstate(invalid="ignore", over="ignore"):
        pr = a[None, :] * B
        z = np.concatenate([np.zeros((B.shape[0], 1)), pr], axis=1)
        return np.cumsum(z, axis=1)[:, -1]


def metric_dist(metric, a, B):
    """dist(a, b) for every row b of B, by the cumsum fold"""
    if metric == "l2":
        return ref.fold_dist(a, B)
    dt = dot_fold(a, B)
    if metric == "inner":
        return -dt
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        na = np.sqrt(dot_fold(a, a[None, :]))[0]
        nb = np.sqrt(np.array([dot_fold(b, b[None, :])[0] for b in B])) if len(B) else np.zeros(0)
        return 1.0 - dt / (na * nb)


def dot_matrix(X64):
    """dot_fold of every pair at once: the same sums, column by column (the accumulator starts at +0.0)"""
    n, d = X64.shape
    acc = np.zeros((n, n))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(d):
            acc = acc + X64[:, c][:, None] * X64[:, c][None, :]
    return acc


def metric_matrix(X64, metric):
    """dist(i, j) of every pair"""
    if metric == "l2":
        return rref.fold_matrix(X64)
    G = dot_matrix(X64)
    if metric == "inner":
        return -G
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.sqrt(np.diagonal(G).copy())
        return 1.0 - G / (s[:, None] * s[None, :])


def knn_graph_metric_ref(X64, perm, leaves, k, D, prior=None):
    """knn_graph_ref.knn_graph_ref with the distances read from D = metric_matrix(X64, metric)"""
    n = X64.shape[0]
    ids = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), np.inf, dtype=np.float64)
    cnt = np.zeros(n, dtype=np.int32)
    for i, m in enumerate(ref.mates_of(perm, leaves, n)):
        dv = D[i, m] if len(m) else np.zeros(0)
        if prior is not None:
            c = int(prior[2][i])
            pi, pd = prior[0][i, :c], prior[1][i, :c]
            new = ~np.isin(pi, m)
            m = np.concatenate([m, pi[new]])
            dv = np.concatenate([dv, pd[new]])
        order = np.lexsort((m, dv))[:k]
        c = len(order)
        ids[i, :c], dist[i, :c], cnt[i] = m[order], dv[order], c
    return ids, dist, cnt


def exact_graph(D, k):
    """the first k of all other points by (distance, id)"""
    n = D.shape[0]
    ids = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), np.inf, dtype=np.float64)
    cnt = np.zeros(n, dtype=np.int32)
    others = np.arange(n, dtype=np.int32)
    for i in range(n):
        m = others[others != i]
        dv = D[i, m]
        order = np.lexsort((m, dv))[:k]
        c = len(order)
        ids[i, :c], dist[i, :c], cnt[i] = m[order], dv[order], c
    return ids, dist, cnt


def hand_graph(D, k, rows):
    """a graph from {i: member ids}: the distances of D, rows sorted by (distance, id)"""
    n = D.shape[0]
    ids = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), np.inf)
    cnt = np.zeros(n, dtype=np.int32)
    for i, members in rows.items():
        m = np.array(sorted(set(members) - {i}), dtype=np.int32)
        dv = D[i, m]
        o = np.lexsort((m, dv))[:k]
        ids[i, :len(o)], dist[i, :len(o)], cnt[i] = m[o], dv[o], len(o)
    return ids, dist, cnt


def refine_ref(X64, graph, k, reverse, iters, D):
    """knn_graph_refine_ref.refine_ref under the metric of D"""
    return rref.refine_ref(X64, graph, k, reverse, iters, D)
