"""numpy restatement of deleting rows from a kNN graph (include/rptree_hip.h, rpt_graph_delete_*), shared
by tests/test_graph_delete_host.py and tests/test_gpu_graph_delete.py.  Not a test module.

It sits on the pair matrices of graph_insert_ref.py: D[n][n] is dist(row p, row e) of the data set
under the layout's fold and the metric.  Two forms of the repair of a touched row, held against each
other by the host test:
  repair_literal  the definition at its word: the set C(p), the whole union K(p) u {(dist(p, e), e)},
                  sorted, its first kg
  repair_sorted   the way the device runs it: a bounded sorted list that starts as K(p); the rows of
                  D(p) are visited in a shuffled order (`rng`) and every id that has not been seen enters
                  at once"""
import bisect

import numpy as np

import graph_search_ref as sref
import graph_insert_ref as iref

key = sref.key
pair_matrix = iref.pair_matrix
pair_matrix_csr = iref.pair_matrix_csr
recall = iref.recall
assert_same_graph = iref.assert_same_graph


def keep_mask(keep, n):
    """keep as a bool array of n: None (every row stays), a bool array, or the uint32 words (id i = bit
    i & 31 of word i >> 5; bits at positions >= n are ignored)"""
    if keep is None:
        return np.ones(n, dtype=bool)
    k = np.asarray(keep)
    if k.dtype == np.uint32:
        assert k.shape == ((n + 31) // 32,)
        return np.unpackbits(np.ascontiguousarray(k).view(np.uint8), bitorder="little")[:n].astype(bool)
    assert k.dtype == np.bool_ and k.shape == (n,)
    return k


def valid_entries(ids_row, dist_row, count, n, j):
    """the valid entries of graph row j as [(distance, id)] in slot order: inside the count clamped to
    [0, kg], id in [0, n) and not j, an id once, at its first slot"""
    kg = len(ids_row)
    c = min(max(int(count), 0), kg)
    out, seen = [], set()
    for s in range(c):
        i = int(ids_row[s])
        if 0 <= i < n and i != j and i not in seen:
            seen.add(i)
            out.append((float(dist_row[s]), i))
    return out


def repair_literal(p, K, Dp, valid_of, keep, drow, kg):
    """-> (row as [(distance, id)], |C(p)|)"""
    held = {i for _, i in K}
    C = {e for j in Dp for _, e in valid_of(j) if keep[e] and e != p and e not in held}
    union = K + [(float(drow[e]), e) for e in C]
    return sorted(union, key=lambda e: key(*e))[:kg], len(C)


def repair_sorted(p, K, Dp, valid_of, keep, drow, kg, rng=None):
    """a sorted list of at most kg entries; what does not come before the last entry of a full list
    never enters; the rows of D(p) in any order"""
    lst = []

    def put(e):
        kv = key(*e)
        if len(lst) == kg:
            if not kv < lst[-1][0]:
                return
            lst.pop()
        bisect.insort(lst, (kv, e))

    for e in K:
        put(e)
    seen = {p} | {i for _, i in K}
    order = list(Dp)
    if rng is not None:
        order = [order[i] for i in rng.permutation(len(order))]
    evaluated = 0
    for j in order:
        cand = valid_of(j)
        if rng is not None:
            cand = [cand[i] for i in rng.permutation(len(cand))]
        for _, e in cand:
            if keep[e] and e not in seen:
                seen.add(e)
                evaluated += 1
                put((float(drow[e]), e))
    return [e for _, e in lst], evaluated


def graph_delete_ref(D, graph, keep, compact=False, literal=False, rng=None, repair=True):
    """-> (ids, dist, count), newid[n], (kept, touched, evaluated, dropped): rpt_graph_delete_*'s answer
    and rpt_graph_delete_last's four counters.  graph: (ids[n][kg], dist[n][kg], count[n]), not
    validated.  Without `compact` the arrays hold n rows in old ids; with it they hold the kept rows
    alone, renumbered through newid.  repair=False: touched rows keep K(p) alone (drop_only)."""
    gids, gdist, gcnt = (np.asarray(a) for a in graph)
    n, kg = gids.shape
    assert gdist.shape == (n, kg) and gcnt.shape == (n,)
    keep = keep_mask(keep, n)
    nkept = int(keep.sum())
    newid = np.where(keep, np.cumsum(keep) - 1 if compact else np.arange(n), -1).astype(np.int32)
    rows = nkept if compact else n
    oids = np.full((rows, kg), -1, dtype=np.int32)
    odist = np.full((rows, kg), np.inf)
    ocnt = np.zeros(rows, dtype=np.int32)
    cache = {}

    def valid_of(j):
        if j not in cache:
            cache[j] = valid_entries(gids[j], gdist[j], gcnt[j], n, j)
        return cache[j]

    touched = evaluated = dropped = 0
    for p in np.flatnonzero(keep).tolist():
        o = int(newid[p])
        V = valid_of(p)
        K = [(d, i) for d, i in V if keep[i]]
        Dp = [i for _, i in V if not keep[i]]
        if not Dp:                                          # untouched: slot for slot
            row = gids[p].astype(np.int64)
            inside = (row >= 0) & (row < n)
            oids[o] = np.where(inside, newid[np.where(inside, row, 0)], row)
            odist[o] = gdist[p]
            ocnt[o] = gcnt[p]
            continue
        touched += 1
        dropped += len(Dp)
        if not repair:
            row, m = sorted(K, key=lambda e: key(*e)), 0
        elif literal:
            row, m = repair_literal(p, K, Dp, valid_of, keep, D[p], kg)
        else:
            row, m = repair_sorted(p, K, Dp, valid_of, keep, D[p], kg, rng)
        evaluated += m
        ocnt[o] = len(row)
        for s, (d, i) in enumerate(row):
            oids[o, s], odist[o, s] = newid[i], d
    return (oids, odist, ocnt), newid, (nkept, touched, evaluated, dropped)


def drop_only(graph, keep, compact=False):
    """the yardstick of the recall table: dead entries removed, nothing put in their place"""
    n = np.asarray(graph[0]).shape[0]
    return graph_delete_ref(np.zeros((n, 0)), graph, keep, compact, repair=False)
