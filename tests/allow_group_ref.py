"""numpy restatement of the grouped allow-list (include/rptree_hip.h, rpt_*_allow_group_*), shared by
tests/test_allow_group_host.py (no GPU) and tests/test_gpu_allow_group.py.  Not a test module.

The definition adds nothing of its own: the answer of query q under (allow[G][words], group[nq]) is
the answer of the single-bitmap entry point for that query under bitmap allow[group[q]], or under no
bitmap for group[q] == -1.  So the restatement only COMPOSES the single-bitmap restatements
(graph_search_allow_ref, knn_allow_ref) query by query, and the statistics are sums."""
import numpy as np

import graph_search_allow_ref as aref
import knn_allow_ref as kref


def standing_group(nq):
    """group[q] = (5 q + 3) % 8 - 1: the values -1 .. 6, interleaved, nq / 8 queries each"""
    return ((5 * np.arange(nq) + 3) % 8 - 1).astype(np.int32)


def standing_masks(n):
    """seven masks: 50 % (seed 1), 50 % (seed 2), 10 % (seed 3), all ones, all zeros, only id n - 2 (in
    the last, partial word when n is no multiple of 32), 2 % (seed 4)"""
    draw = lambda seed, f: np.random.default_rng(seed).random(n) < f  # noqa: E731
    one = np.zeros(n, dtype=bool)
    one[n - 2] = True
    return [draw(1, 0.5), draw(2, 0.5), draw(3, 0.1), np.ones(n, dtype=bool), np.zeros(n, dtype=bool), one,
            draw(4, 0.02)]


def interleaved_group(nq, G):
    """every value of -1 .. G - 1, neighbours in different groups"""
    return ((5 * np.arange(nq) + 3) % (G + 1) - 1).astype(np.int32)


def mask_of_group(masks, g, n):
    """the bool mask query group g searches under; -1: every id; outside [-1, G): none"""
    if g == -1:
        return np.ones(n, dtype=bool)
    if 0 <= g < len(masks):
        return np.asarray(masks[g], dtype=bool)
    return np.zeros(n, dtype=bool)


def words_of_masks(masks, n, tail=False):
    """-> uint32[G][ceil(n / 32)], row g = the bitmap of masks[g] (tail: every bit behind n set too)"""
    out = np.zeros((len(masks), (n + 31) // 32), dtype=np.uint32)
    for g, m in enumerate(masks):
        out[g] = kref.bitmap(m, tail=tail)
    return out


def queries_of(group):
    """group value -> the (ascending) queries that carry it"""
    group = np.asarray(group)
    return {int(g): np.flatnonzero(group == g) for g in np.unique(group)}


def group_answers(X64, Q64, gids, gcount, seeds, k, ef, width, masks, group, metric="l2", D=None):
    """graph_search_allow_ref per query under the query's own mask -> ((ids, dist, count), expansions,
    offered, upper), the three statistics summed over the queries"""
    nq, n = Q64.shape[0], X64.shape[0]
    if D is None:
        D = aref.query_matrix(X64, Q64, metric)
    ids = np.full((nq, k), -1, dtype=np.int32)
    dist = np.full((nq, k), np.inf)
    cnt = np.zeros(nq, dtype=np.int32)
    tot = [0, 0, 0]
    seeds = np.asarray(seeds)
    for g, rows in queries_of(group).items():
        (gi, gd, gc), e, o, u = aref.graph_search_allow_ref(X64, Q64[rows], gids, gcount, seeds[rows], k, ef, width,
                                                            mask_of_group(masks, g, n), metric, D=D[rows])
        ids[rows], dist[rows], cnt[rows] = gi, gd, gc
        tot = [tot[0] + e, tot[1] + o, tot[2] + u]
    return (ids, dist, cnt), tot[0], tot[1], tot[2]


def knn_group_answers(all_ids, all_dist, all_cnt, masks, group, k, rule=kref.KEEP):
    """knn_allow_ref.from_ranked per query under the query's own mask; all_*: the ranked listing of
    every candidate entry (knnBatch with k = everything, duplicates kept) -> (ids, dist, count)"""
    nq = len(all_cnt)
    n = len(masks[0]) if len(masks) else int(all_ids.max()) + 1
    oi = np.empty((nq, k), dtype=np.int32)
    od = np.empty((nq, k))
    oc = np.empty(nq, dtype=np.int32)
    for i in range(nq):
        m = all_cnt[i]
        oi[i], od[i], oc[i] = kref.from_ranked(all_ids[i, :m], all_dist[i, :m], mask_of_group(masks, int(group[i]), n), k,
                                               rule)
    return oi, od, oc


def per_group_calls(call, masks, group, nq, shapes):
    """The route without the feature: one single-bitmap call per group over that group's queries.
    call(mask or None, rows) -> a tuple of arrays whose first axis is the rows; shapes: the trailing
    shape and dtype of each output.  -> the outputs scattered back to [nq]"""
    outs = [np.zeros((nq,) + tuple(sh), dtype=dt) for sh, dt in shapes]
    for g, rows in queries_of(group).items():
        got = call(None if g == -1 else masks[g], rows)
        for o, a in zip(outs, got):
            o[rows] = a
    return tuple(outs)
