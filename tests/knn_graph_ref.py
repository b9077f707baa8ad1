"""numpy restatement of the kNN graph's definition (include/rptree_hip.h, rpt_knn_graph_*), shared
by tests/test_knn_graph_host.py and tests/test_gpu_knn_graph.py.  Not a test module.

mates(i) = ids j != i sharing a leaf with i in some tree; dist = metricDDL2's left fold in double;
the answer = the first k of mates(i) by (distance, id), NaN last."""
import numpy as np


def leaf_slices(topo):
    """(offset, size) of the leaves of an rpt_topology table"""
    return [(int(o), int(s)) for (_, _, o, s, leaf) in topo if leaf]


def fold_dist(a, B):
    """sqrt(((0 + (a0 - b0)^2) + (a1 - b1)^2) + ...) for every row b of B: np.cumsum adds in order"""
    with np.errstate(invalid="ignore", over="ignore"):
        sq = (a[None, :] - B) ** 2
        z = np.concatenate([np.zeros((B.shape[0], 1)), sq], axis=1)
        return np.sqrt(np.cumsum(z, axis=1)[:, -1])


def mates_of(perm, leaves, n):
    """per point the sorted ids of its leaf mates over all trees, itself removed"""
    parts = [[] for _ in range(n)]
    for t in range(perm.shape[0]):
        for o, s in leaves:
            ids = perm[t, o:o + s]
            for i in ids:
                parts[i].append(ids)
    out = []
    for i in range(n):
        m = np.unique(np.concatenate(parts[i])) if parts[i] else np.zeros(0, dtype=np.int32)
        out.append(m[m != i].astype(np.int32))
    return out


def knn_graph_ref(X64, perm, leaves, k, prior=None):
    """-> (ids[n][k], dist[n][k], count[n]); prior = an earlier answer whose valid entries join the
    mates with their stored distances (RPT_GRAPH_ACCUMULATE)"""
    n = X64.shape[0]
    ids = np.full((n, k), -1, dtype=np.int32)
    dist = np.full((n, k), np.inf, dtype=np.float64)
    cnt = np.zeros(n, dtype=np.int32)
    for i, m in enumerate(mates_of(perm, leaves, n)):
        dv = fold_dist(X64[i], X64[m]) if len(m) else np.zeros(0)
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


def bits(a):
    """bit patterns; every NaN counts as the same value (IEEE leaves a NaN's payload open)"""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_graph(got, want, tag=""):
    """ids, counts and distance BITS"""
    gi, gd, gc = got
    wi, wd, wc = want
    assert np.array_equal(gc, wc), "%s: counts differ at rows %s" % (tag, np.nonzero(gc != wc)[0][:8])
    bad = np.nonzero((gi != wi).any(axis=1))[0]
    assert bad.size == 0, "%s: ids differ at rows %s: got %s want %s" % (
        tag, bad[:8], gi[bad[0]].tolist(), wi[bad[0]].tolist())
    bad = np.nonzero((bits(gd) != bits(wd)).any(axis=1))[0]
    assert bad.size == 0, "%s: distance bits differ at rows %s: got %s want %s" % (
        tag, bad[:8], gd[bad[0]].tolist(), wd[bad[0]].tolist())
