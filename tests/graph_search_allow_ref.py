"""numpy restatement of the beam search over an allow-list of ids (include/rptree_hip.h,
rpt_graph_search_allow_*), shared by tests/test_graph_search_allow_host.py and
tests/test_gpu_graph_search_allow.py.  Not a test module.  Built on graph_search_ref: the distance,
the order (key), the graph rows (row_of) and the seeds are that file's.

The beam is cut(everything offered so far): with the entries sorted by (distance, id), NaN behind
every number, it ends at its ef-th ALLOWED entry or at its width-th entry, whichever comes first.
Disallowed entries are expanded like any other; the answer is the first k allowed entries.  Three
forms: search_one offers a set one id at a time and keeps the count of allowed entries as the
kernel does (an id that is rejected or evicted never comes back, so the order inside a set plays no
part); the same with visited=False; search_literal takes "B <- cut(B u S)" at its word.
search_prefix is the tempting rule that is NOT the definition (the longest sorted prefix with at
most width entries and at most ef allowed ones): the host test shows where it goes wrong."""
import bisect

import numpy as np

import graph_search_ref as sref

bits = sref.bits
key = sref.key
row_of = sref.row_of
query_matrix = sref.query_matrix
assert_same_answer = sref.assert_same_answer


def words_of(mask):
    """a bool mask of n -> the ceil(n / 32) uint32 words: id i is bit i & 31 of word i >> 5"""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[0]
    w = np.zeros((n + 31) // 32, dtype=np.uint32)
    for i in np.flatnonzero(mask).tolist():
        w[i >> 5] |= np.uint32(1 << (i & 31))
    return w


def mask_of(words, n):
    """the first n bits of the words; bits at positions >= n are ignored; None = every id"""
    if words is None:
        return np.ones(n, dtype=bool)
    words = np.asarray(words, dtype=np.uint32)
    return np.array([bool((int(words[i >> 5]) >> (i & 31)) & 1) for i in range(n)], dtype=bool)


def cut(entries, allowed, ef, width):
    """entries: sorted keys (nan, distance, id) -> every entry that is not after min(t_a, t_w)"""
    out, na = [], 0
    for e in entries:
        out.append(e)
        na += bool(allowed[e[2]])
        if na == ef or len(out) == width:
            break
    return out


def search_one(drow, gids, gcount, seeds_row, ef, width, allowed, visited=True):
    """-> (beam as [(distance, id)], expansions, offered, upper) of one query; drow[v] = dist(q, v),
    allowed[v]: whether v is in the allow-list.  One id at a time, the way the kernel inserts."""
    n = len(drow)
    beam, inbeam, expanded, seen, offered = [], set(), set(), set(), set()
    na = [0]

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
            if na[0] == ef or len(beam) == width:       # full: the last entry is the threshold
                if not kv < beam[-1]:
                    continue
            bisect.insort(beam, kv)
            inbeam.add(v)
            na[0] += bool(allowed[v])
            if len(beam) > width:
                gone = beam.pop()[2]
                inbeam.discard(gone)
                na[0] -= bool(allowed[gone])
            if allowed[v] and na[0] >= ef:               # the beam ends at its ef-th allowed entry
                cnt, end = 0, None
                for p, e in enumerate(beam):
                    cnt += bool(allowed[e[2]])
                    if cnt == ef:
                        end = p + 1
                        break
                for e in beam[end:]:
                    inbeam.discard(e[2])
                del beam[end:]
                na[0] = ef

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
    return [(drow[e[2]], e[2]) for e in beam], len(expanded), len(offered), upper


def search_literal(drow, gids, gcount, seeds_row, ef, width, allowed):
    """the definition word for word: B <- cut(B u S) -> (beam, expansions)"""
    n = len(drow)
    beam, expanded = [], set()

    def offer(S):
        ids = {e[2] for e in beam} | set(S)
        return cut(sorted(key(drow[v], v) for v in ids), allowed, ef, width)

    beam = offer([v for v in seeds_row if 0 <= v < n])
    while True:
        u = next((e[2] for e in beam if e[2] not in expanded), None)
        if u is None:
            break
        expanded.add(u)
        beam = offer(row_of(gids, gcount, u, n)[0])
    return [(drow[e[2]], e[2]) for e in beam], len(expanded)


def prefix_rule(entries, allowed, ef, width):
    """NOT the definition: the longest sorted prefix with at most width entries and at most ef allowed"""
    out, na = [], 0
    for e in entries:
        if len(out) == width or na + bool(allowed[e[2]]) > ef:
            break
        out.append(e)
        na += bool(allowed[e[2]])
    return out


def search_prefix(drow, gids, gcount, seeds_row, ef, width, allowed, visited):
    """the search under prefix_rule, one id at a time -> (beam, expansions); it depends on `visited`"""
    n = len(drow)
    beam, expanded, seen = [], set(), set()

    def offer(S):
        nonlocal beam
        for v in S:
            if visited:
                if v in seen:
                    continue
                seen.add(v)
            if v in {e[2] for e in beam}:
                continue
            beam = prefix_rule(sorted(beam + [key(drow[v], v)]), allowed, ef, width)

    offer([v for v in seeds_row if 0 <= v < n])
    while True:
        u = next((e[2] for e in beam if e[2] not in expanded), None)
        if u is None or len(expanded) >= n:
            break
        expanded.add(u)
        offer(row_of(gids, gcount, u, n)[0])
    return [(drow[e[2]], e[2]) for e in beam], len(expanded)


def answer_of(beam, allowed, k):
    """the first k allowed entries of a beam -> (ids, dists)"""
    hit = [b for b in beam if allowed[b[1]]][:k]
    return [b[1] for b in hit], [b[0] for b in hit]


def graph_search_allow_ref(X64, Q64, gids, gcount, seeds, k, ef, width, allow=None, metric="l2", visited=True,
                           D=None):
    """-> (ids[nq][k], dist[nq][k], count[nq]), expansions, offered, upper (sums over the queries).
    allow: a bool mask of n, the uint32 words, or None (every id); D: query_matrix(X64, Q64, metric),
    when the caller has it already."""
    nq, n = Q64.shape[0], X64.shape[0]
    if D is None:
        D = query_matrix(X64, Q64, metric)
    allow = None if allow is None else np.asarray(allow)
    allowed = (mask_of(allow, n) if allow is None or allow.dtype == np.uint32 else allow.astype(bool)).tolist()
    gids = np.asarray(gids)
    ids = np.full((nq, k), -1, dtype=np.int32)
    dist = np.full((nq, k), np.inf)
    cnt = np.zeros(nq, dtype=np.int32)
    tot = [0, 0, 0]
    for i in range(nq):
        beam, e, o, u = search_one(D[i].tolist(), gids, gcount, np.asarray(seeds[i]).tolist(), ef, width, allowed,
                                   visited)
        hi, hd = answer_of(beam, allowed, k)
        cnt[i] = len(hi)
        ids[i, :len(hi)] = hi
        dist[i, :len(hi)] = hd
        tot = [tot[0] + e, tot[1] + o, tot[2] + u]
    return (ids, dist, cnt), tot[0], tot[1], tot[2]
