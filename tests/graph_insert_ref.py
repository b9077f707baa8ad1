"""numpy restatement of inserting new rows into a kNN graph (include/rptree_hip.h, rpt_graph_insert_*),
shared by tests/test_graph_insert_host.py and tests/test_gpu_graph_insert.py.  Not a test module.

Built on graph_search_ref.search_one and the fold modules: D[N][N] is dist(row p as the query, row v)
of the data set of N = n + m rows, whose last m rows are the new ones.  With v rows visible, a chunk
P = [v, v + |P|) is searched (search_one over the first v rows and the graph so far, k = kg), the
answers become rows P, and every (d, o) of an answer A_p offers (d, p) to row o.  Two forms of the
link, held against each other by the host test:
  link_sorted   the chunk loop as the device runs it: a bounded sorted list per target, the offers
                entering one at a time in whatever order they arrive (`rng` shuffles them)
  link_literal  the definition at its word: the whole union per target, sorted, its first kg"""
import bisect

import numpy as np

import graph_search_ref as sref
import graph_metric_csr_ref as gm

key = sref.key


def pair_matrix(X64, metric):
    """dist(row p as the query, row v) for the dense folds: [N][N]"""
    return sref.query_matrix(X64, X64, metric)


def pair_matrix_csr(csr, metric):
    """the same for CSR rows: the union fold under L2 (= the fold over the dense-ified rows), dotS under
    cosine / inner product"""
    return gm.dense_query_matrix(csr, csr, "l2") if metric == "l2" else gm.query_matrix(csr, csr, metric)


def valid_entries(ids_row, dist_row, count, N):
    """the valid entries of a graph row as [(distance, id)] in slot order: inside the count clamped to
    [0, kg], id in [0, N), an id once, at its first slot"""
    kg = len(ids_row)
    c = min(max(int(count), 0), kg)
    out, seen = [], set()
    for j in range(c):
        i = int(ids_row[j])
        if 0 <= i < N and i not in seen:
            seen.add(i)
            out.append((float(dist_row[j]), i))
    return out


def link_literal(own, offers, kg):
    """the first kg by (distance, id) of own u offers; an offer whose id the row holds is dropped"""
    held = {i for _, i in own}
    union = own + [(d, p) for d, p in offers if p not in held]
    return sorted(union, key=lambda e: key(*e))[:kg]


def link_sorted(own, offers, kg, rng=None):
    """a sorted list of at most kg entries; what does not come before the last entry of a full list
    never enters"""
    held = {i for _, i in own}
    lst = []

    def put(e):
        kv = key(*e)
        if len(lst) == kg:
            if not kv < lst[-1][0]:
                return
            lst.pop()
        bisect.insort(lst, (kv, e))

    for e in own:
        put(e)
    offers = [e for e in offers if e[1] not in held]
    if rng is not None:
        offers = [offers[i] for i in rng.permutation(len(offers))]
    for e in offers:
        put(e)
    return [e for _, e in lst]


def graph_insert_ref(D, graph, m, seeds, ef, batch, literal=False, visited=True, rng=None):
    """-> (ids[N][kg], dist[N][kg], count[N]), (chunks, offered, accepted), (lo, hi): the graph after the
    last chunk, rpt_graph_insert_last's three exact counters and the bounds of `evaluated` (the sums of
    graph_search_ref's `offered` and `upper`).  graph: (ids[n][kg], dist[n][kg], count[n]) over the
    first n = N - m rows, not validated: rows nothing links to are copied as they are."""
    N = D.shape[0]
    n = N - m
    gids, gdist, gcnt = (np.asarray(a) for a in graph)
    kg = gids.shape[1]
    assert gids.shape == (n, kg) and gdist.shape == (n, kg) and gcnt.shape == (n,) and batch >= 1
    oids = np.full((N, kg), -1, dtype=np.int32)
    odist = np.full((N, kg), np.inf)
    ocnt = np.zeros(N, dtype=np.int32)
    oids[:n], odist[:n], ocnt[:n] = gids, gdist, gcnt
    seeds = np.asarray(seeds)
    assert seeds.ndim == 2 and seeds.shape[0] == m
    chunks = offered = accepted = lo = hi = 0
    v = n
    while v < N:
        cnt = min(batch, N - v)
        offers = {}
        answers = []
        for p in range(v, v + cnt):                      # every row of the chunk against the SAME graph
            beam, _, o, u = sref.search_one(D[p, :v].tolist(), oids[:v], ocnt[:v], seeds[p - n].tolist(), ef, visited)
            answers.append(beam[:kg])
            lo, hi = lo + o, hi + u
        for p, A in zip(range(v, v + cnt), answers):
            oids[p], odist[p], ocnt[p] = -1, np.inf, len(A)
            for j, (d, o) in enumerate(A):
                oids[p, j], odist[p, j] = o, d
                offers.setdefault(o, []).append((d, p))
                offered += 1
        for o, lst in offers.items():
            own = valid_entries(oids[o], odist[o], ocnt[o], N)
            row = link_literal(own, lst, kg) if literal else link_sorted(own, lst, kg, rng)
            oids[o], odist[o], ocnt[o] = -1, np.inf, len(row)
            for j, (d, i) in enumerate(row):
                oids[o, j], odist[o, j] = i, d
            held = {i for _, i in own}
            accepted += sum(v <= i < v + cnt and i not in held for _, i in row)
        v += cnt
        chunks += 1
    return (oids, odist, ocnt), (chunks, offered, accepted), (lo, hi)


def recall(ids, truth):
    """recall@k of ids[nq][k] against truth[nq][k] (every row full)"""
    return sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ids, truth)) / float(truth.size)


def assert_same_graph(got, want, tag=""):
    """ids, counts and distance BITS"""
    sref.assert_same_answer(got, want, tag)
