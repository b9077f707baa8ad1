"""numpy restatement of the search-graph preparation (include/rptree_hip.h, rpt_graph_prepare_*),
shared by tests/test_graph_prepare_host.py and tests/test_gpu_graph_prepare.py.  Not a test module.

Kept(i): the valid entries of row i; with DIVERSIFY, walking the row in stored order, entry e_m stays
unless an already kept e_l (l < m) has dist(e_l, e_m) < the distance stored with e_m in row i (a plain
<: NaN keeps, an equal distance keeps).  Union(i): Kept(i), with REVERSE joined by {j : i in Kept(j)}
at the distance stored with i in row j (an id in both keeps row i's distance).  Row i of the output:
the first kout of Union(i) by (distance, id), NaN behind every number.  The pair distances come from
D = knn_graph_metric_ref.metric_matrix(X64, metric)."""
import numpy as np

import knn_graph_ref as ref

bits = ref.bits
DIVERSIFY, REVERSE = 1, 2


def clean_graph(graph, n):
    """what the _dev entry point makes of an unvalidated graph: a count is clamped to [0, k], an id
    outside [0, n) is skipped; the rest of a row moves up in its order"""
    ids, dist, cnt = (np.asarray(a) for a in graph)
    k = ids.shape[1] if ids.ndim == 2 else 0
    oi = np.full((n, k), -1, dtype=np.int32)
    od = np.full((n, k), np.inf)
    oc = np.zeros(n, dtype=np.int32)
    for i in range(n):
        c = min(max(int(cnt[i]), 0), k)
        keep = [s for s in range(c) if 0 <= ids[i, s] < n]
        oc[i] = len(keep)
        oi[i, :len(keep)] = ids[i, keep]
        od[i, :len(keep)] = dist[i, keep]
    return oi, od, oc


def kept_of(ids_row, dist_row, D, diversify):
    """-> the slots of a (clean) row that stay, in stored order"""
    c = len(ids_row)
    if not diversify or c < 2:
        return list(range(c))
    r = np.asarray(ids_row, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        occ = D[np.ix_(r, r)] < np.asarray(dist_row)[None, :]   # occ[l, m]: e_l occludes e_m; NaN compares false
    kept = [0]
    for m in range(1, c):
        if not occ[kept, m].any():
            kept.append(m)
    return kept


def key(dv, i):
    """numbers by (distance, id), then NaN distances by id; -0.0 ties with +0.0"""
    nan = dv != dv
    return (nan, 0.0 if nan else dv, i)


def unions_of(graph, D, flags, n=None):
    """-> Union(i) for every i as a list of (distance, id) in the order of the answer, and (pairs,
    occluded); the part of the definition that does not depend on kout"""
    ids, dist, cnt = (np.asarray(a) for a in graph)
    n = len(cnt) if n is None else n
    ids, dist, cnt = clean_graph((ids, dist, cnt), n)
    div, rev = bool(flags & DIVERSIFY), bool(flags & REVERSE)
    pairs = occluded = 0
    union = []
    for i in range(n):
        c = int(cnt[i])
        kept = kept_of(ids[i, :c], dist[i, :c], D, div)
        if div:
            pairs += c * (c - 1) // 2
        occluded += c - len(kept)
        u = {}
        for s in kept:
            u.setdefault(int(ids[i, s]), dist[i, s])
        union.append(u)
    if rev:
        own = [list(u.items()) for u in union]
        for j in range(n):
            for t, dv in own[j]:
                union[t].setdefault(j, dv)       # an id that row t holds itself keeps row t's distance
    return [sorted(((dv, v) for v, dv in u.items()), key=lambda e: key(*e)) for u in union], (pairs, occluded)


def cut_unions(unions, kout):
    """-> (ids[n][kout], dist[n][kout], count[n]), capped"""
    n = len(unions)
    oi = np.full((n, kout), -1, dtype=np.int32)
    od = np.full((n, kout), np.inf)
    oc = np.zeros(n, dtype=np.int32)
    capped = 0
    for i, u in enumerate(unions):
        c = min(kout, len(u))
        capped += len(u) - c
        oc[i] = c
        oi[i, :c] = [e[1] for e in u[:c]]
        od[i, :c] = [e[0] for e in u[:c]]
    return (oi, od, oc), capped


def graph_prepare_ref(graph, D, kout, flags, n=None):
    """-> (ids[n][kout], dist[n][kout], count[n]), (pairs, occluded, capped)"""
    unions, (pairs, occluded) = unions_of(graph, D, flags, n)
    out, capped = cut_unions(unions, kout)
    return out, (pairs, occluded, capped)


def assert_same_answer(got, want, tag=""):
    """ids, counts and distance BITS"""
    ref.assert_same_graph(got, want, tag)
