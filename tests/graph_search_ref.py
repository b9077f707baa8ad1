"""numpy restatement of the beam search over a kNN graph (include/rptree_hip.h, rpt_graph_search_*),
shared by tests/test_graph_search_host.py and tests/test_gpu_graph_search.py.  Not a test module.

dist(q, v): the folds of knn_graph_ref / knn_graph_metric_ref with q in the place of x_i.  The beam
holds at most ef entries sorted by (distance, id), NaN behind every number; the valid seeds are
offered, then the graph row of the first unexpanded entry, until none is left; the answer is the
first k.  graph_search_ref offers a set one id at a time (an id that is rejected or evicted never
comes back, so the order inside a set plays no part); search_literal takes "the first ef of B u S"
at its word and is what the host test holds the fast form against."""
import bisect

import numpy as np

import knn_graph_ref as ref
import knn_graph_metric_ref as mref

bits = ref.bits


def row_norms(X64):
    """dot(x, x) of every row, the fold of mref.dot_fold"""
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.concatenate([np.zeros((X64.shape[0], 1)), X64 * X64], axis=1)
        return np.cumsum(z, axis=1)[:, -1]


def query_matrix(X64, Q64, metric):
    """dist(q, v) for every query q and every row v: [nq][n]"""
    nq, n = Q64.shape[0], X64.shape[0]
    D = np.empty((nq, n))
    if n == 0:
        return D
    rn = row_norms(X64) if metric == "cosine" else None
    for i in range(nq):
        q = Q64[i]
        if metric == "l2":
            D[i] = ref.fold_dist(q, X64)
            continue
        dt = mref.dot_fold(q, X64)
        if metric == "inner":
            D[i] = -dt
        else:
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                D[i] = 1.0 - dt / (np.sqrt(row_norms(q[None, :])[0]) * np.sqrt(rn))
    return D


def key(dv, i):
    """the order of the answer: numbers by (distance, id), then NaN distances by id; -0.0 ties with +0.0"""
    nan = dv != dv
    return (nan, 0.0 if nan else dv, i)


def row_of(gids, gcount, u, n):
    """the valid ids of graph row u; a count outside [0, kg] offers nothing"""
    kg = gids.shape[1]
    c = int(gcount[u])
    if c < 0 or c > kg:
        return [], 0
    return [v for v in gids[u, :c].tolist() if 0 <= v < n], c


def search_one(drow, gids, gcount, seeds_row, ef, visited=True):
    """-> (beam as [(distance, id)], expansions, offered, upper) of one query; drow[v] = dist(q, v)"""
    n = len(drow)
    beam, inbeam, expanded, seen, offered = [], set(), set(), set(), set()
    raw = {}

    def offer(S):
        for v in S:
            offered.add(v)
            if visited:
                if v in seen:
                    continue
                seen.add(v)
            if v in inbeam:
                continue
            kv = key(drow[v], v)
            if len(beam) == ef:
                if not kv < beam[-1]:
                    continue
                inbeam.discard(beam.pop()[2])
            bisect.insort(beam, kv)
            inbeam.add(v)
            raw[v] = drow[v]

    valid = [v for v in seeds_row if 0 <= v < n]
    upper = len(valid)
    offer(valid)
    while True:
        u = next((e[2] for e in beam if e[2] not in expanded), None)
        if u is None:
            break
        expanded.add(u)
        assert len(expanded) <= n
        S, c = row_of(gids, gcount, u, n)
        upper += c
        offer(S)
    return [(raw[e[2]], e[2]) for e in beam], len(expanded), len(offered), upper


def search_literal(drow, gids, gcount, seeds_row, ef):
    """the definition word for word: B <- the first ef of B u S -> (beam, expansions)"""
    n = len(drow)
    beam, expanded = [], set()

    def offer(S):
        ids = {e[2] for e in beam} | set(S)
        return sorted(key(drow[v], v) for v in ids)[:ef]

    beam = offer([v for v in seeds_row if 0 <= v < n])
    while True:
        u = next((e[2] for e in beam if e[2] not in expanded), None)
        if u is None:
            break
        expanded.add(u)
        beam = offer(row_of(gids, gcount, u, n)[0])
    return [(drow[e[2]], e[2]) for e in beam], len(expanded)


def graph_search_ref(X64, Q64, gids, gcount, seeds, k, ef, metric="l2", visited=True, D=None):
    """-> (ids[nq][k], dist[nq][k], count[nq]), expansions, offered, upper (sums over the queries).
    D: query_matrix(X64, Q64, metric), when the caller has it already."""
    nq = Q64.shape[0]
    if D is None:
        D = query_matrix(X64, Q64, metric)
    gids = np.asarray(gids)
    ids = np.full((nq, k), -1, dtype=np.int32)
    dist = np.full((nq, k), np.inf)
    cnt = np.zeros(nq, dtype=np.int32)
    tot = [0, 0, 0]
    for i in range(nq):
        beam, e, o, u = search_one(D[i].tolist(), gids, gcount, np.asarray(seeds[i]).tolist(), ef, visited)
        c = min(k, len(beam))
        cnt[i] = c
        ids[i, :c] = [b[1] for b in beam[:c]]
        dist[i, :c] = [b[0] for b in beam[:c]]
        tot = [tot[0] + e, tot[1] + o, tot[2] + u]
    return (ids, dist, cnt), tot[0], tot[1], tot[2]


def assert_same_answer(got, want, tag=""):
    """ids, counts and distance BITS"""
    ref.assert_same_graph(got, want, tag)
