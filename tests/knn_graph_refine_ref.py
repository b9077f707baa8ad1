"""numpy restatement of the kNN graph refinement's definition (include/rptree_hip.h,
rpt_knn_graph_refine_*), shared by tests/test_knn_graph_refine_host.py and
tests/test_gpu_knn_graph_refine.py.  Not a test module.

One round: F(i) = the valid ids of row i; Rev_r(i) = the first r of {j : i in F(j)} by (the distance
stored with i in row j, j); B = F u Rev_r; C(i) = (B u U{F(v) : v in B}) minus i, a set; a member of
F(i) keeps its stored distance, any other gets knn_graph_ref.fold_dist; the new row is the first k
of C(i) by (distance, id), NaN last (np.lexsort keeps NaNs behind the numbers, in id order)."""
import numpy as np

from knn_graph_ref import fold_dist


def reverse_lists(ids, dist, cnt, r):
    """Rev_r of every point, as arrays of source ids"""
    n, k = ids.shape
    out = [np.zeros(0, dtype=np.int32) for _ in range(n)]
    if r == 0 or n == 0:
        return out
    valid = np.arange(k)[None, :] < cnt[:, None]
    src = np.repeat(np.arange(n, dtype=np.int32), k)[valid.ravel()]
    tgt = ids.ravel()[valid.ravel()]
    dd = dist.ravel()[valid.ravel()]
    order = np.lexsort((src, dd, tgt))                     # by target, then (stored distance, source)
    tgt, src = tgt[order], src[order]
    targets, first = np.unique(tgt, return_index=True)
    for t, a, b in zip(targets, first, list(first[1:]) + [len(tgt)]):
        out[int(t)] = src[a:min(b, a + r)]
    return out


def fold_matrix(X64):
    """fold_dist of every pair at once: the same sums, column by column (0 + x is x)"""
    n, d = X64.shape
    acc = np.zeros((n, n))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(d):
            t = X64[:, c][:, None] - X64[:, c][None, :]
            acc = acc + t * t
        return np.sqrt(acc)


def refine_round(X64, graph, k, r, D=None):
    """-> (R(graph), |F_new minus F_old| summed, |C minus F| summed); D: fold_matrix(X64), if at hand"""
    ids, dist, cnt = graph
    n = X64.shape[0]
    rev = reverse_lists(ids, dist, cnt, r)
    nids = np.full((n, k), -1, dtype=np.int32)
    ndist = np.full((n, k), np.inf, dtype=np.float64)
    ncnt = np.zeros(n, dtype=np.int32)
    updates = candidates = 0
    for i in range(n):
        F, Fd = ids[i, :cnt[i]], dist[i, :cnt[i]]
        B = np.union1d(F, rev[i])
        C = np.unique(np.concatenate([B] + [ids[v, :cnt[v]] for v in B])) if len(B) else B
        C = C[C != i]
        new = np.setdiff1d(C, F).astype(np.int32)
        candidates += len(new)
        m = np.concatenate([F, new])
        nd = np.zeros(0) if not len(new) else D[i, new] if D is not None else fold_dist(X64[i], X64[new])
        dv = np.concatenate([Fd, nd])
        order = np.lexsort((m, dv))[:k]
        c = len(order)
        nids[i, :c], ndist[i, :c], ncnt[i] = m[order], dv[order], c
        updates += int((~np.isin(m[order], F)).sum())
    return (nids, ndist, ncnt), updates, candidates


def refine_ref(X64, graph, k, reverse, iters, D=None):
    """-> (graph, rounds, updates, candidates) after up to `iters` rounds; a round that changes no
    row is the last one applied"""
    g = tuple(np.array(a) for a in graph)
    rounds = updates = candidates = 0
    for _ in range(iters):
        g, u, c = refine_round(X64, g, k, reverse, D)
        rounds += 1
        updates += u
        candidates += c
        if u == 0:
            break
    return g, rounds, updates, candidates


def exact_graph(X64, k):
    """the first k of all other points by (fold distance, id)"""
    n = X64.shape[0]
    ids = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), np.inf, dtype=np.float64)
    cnt = np.zeros(n, dtype=np.int32)
    others = np.arange(n, dtype=np.int32)
    for i in range(n):
        m = others[others != i]
        dv = fold_dist(X64[i], X64[m])
        order = np.lexsort((m, dv))[:k]
        c = len(order)
        ids[i, :c], dist[i, :c], cnt[i] = m[order], dv[order], c
    return ids, dist, cnt


def recall(graph, exact):
    """share of the exact graph's entries that the graph holds"""
    hit = tot = 0
    for i in range(exact[0].shape[0]):
        want = exact[0][i, :exact[2][i]]
        hit += int(np.isin(want, graph[0][i, :graph[2][i]]).sum())
        tot += len(want)
    return hit / max(tot, 1)
