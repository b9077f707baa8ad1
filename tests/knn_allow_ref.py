"""numpy restatement of the allow-list on the forest query and on the exhaustive kNN
(include/rptree_hip.h, rpt_knn_allow_* / rpt_brute_knn_allow_*), shared by
tests/test_knn_allow_host.py (no GPU) and tests/test_gpu_knn_allow.py.  Not a test module.

The definition: a query's candidate list is rpt_candidates' (trees ascending, leaves left to right,
duplicates kept); the allowed list is that list without the entries whose id is not allowed, in the
same order; the answer is the k best of the allowed list by (distance, position), NaN last, under
the duplicate rule (0 = duplicates kept, 1 = each id once, 2 = one entry per distance), which is
applied AFTER the filter; count = min(k, entries the rule leaves); unused slots id -1, distance
+inf.  The exhaustive answer: the k best allowed rows by (distance, id), NaN last."""
import numpy as np

from knn_vote_ref import fold_dots, l2_f64, metric_dense, same_bits  # noqa: F401  (the cells' distances)

KEEP, EACH_ID_ONCE, ONE_PER_DISTANCE = 0, 1, 2
RULES = (KEEP, EACH_ID_ONCE, ONE_PER_DISTANCE)


# ------------------------------------------------------------------ the bitmap
def bitmap(mask, tail=False):
    """a bool mask of n -> ceil(n / 32) uint32 words (id i = bit i & 31 of word i >> 5); tail: every
    bit behind n set as well (they are ignored)"""
    mask = np.asarray(mask, dtype=bool)
    n = len(mask)
    bits = np.zeros(((n + 31) // 32) * 32, dtype=np.uint8)
    bits[:n] = mask
    if tail:
        bits[n:] = 1
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32))


# ------------------------------------------------------------------ the lists
def allowed_list(cands, mask):
    c = np.asarray(cands, dtype=np.int32)
    return c[np.asarray(mask, dtype=bool)[c]] if len(c) else c


def allowed_batch(off, cids, T, mask):
    """candidatesBatch's (off[nq*T+1], ids) -> (off[nq+1], ids) of the allowed lists"""
    nq = (len(off) - 1) // T
    out_off = np.zeros(nq + 1, dtype=np.int64)
    parts = []
    for i in range(nq):
        parts.append(allowed_list(cids[off[i * T]:off[(i + 1) * T]], mask))
        out_off[i + 1] = out_off[i] + len(parts[-1])
    return out_off, (np.concatenate(parts) if parts else np.zeros(0)).astype(np.int32)


# ------------------------------------------------------------------ rank, rule, cut
def rank(dist):
    """the order of a list's entries by (distance, position), NaN last"""
    dist = np.asarray(dist, dtype=np.float64)
    nan = np.isnan(dist)
    return np.lexsort((np.arange(len(dist)), np.where(nan, 0.0, dist), nan))


def rule_keeps(ids, dist, rule):
    """entries in RANK order -> the indices the duplicate rule keeps.  1: the first entry of every id;
    2: an entry is dropped when its distance equals the last kept one (knnPQ's nub; NaN equals nothing)"""
    if rule == KEEP:
        return np.arange(len(ids))
    kept, seen, last = [], set(), None
    for j, (i, dv) in enumerate(zip(np.asarray(ids).tolist(), np.asarray(dist, dtype=np.float64).tolist())):
        if rule == EACH_ID_ONCE:
            if i in seen:
                continue
            seen.add(i)
        elif kept and dv == last:
            continue
        kept.append(j)
        last = dv
    return np.asarray(kept, dtype=np.int64)


def cut(ids, dist, k):
    """the first k of ranked, rule-filtered entries -> (ids[k], dist[k], count)"""
    cnt = min(k, len(ids))
    oi = np.full(k, -1, dtype=np.int32)
    od = np.full(k, np.inf)
    oi[:cnt], od[:cnt] = ids[:cnt], dist[:cnt]
    return oi, od, cnt


def answer(ids, dist, k, rule):
    """a list (its ids and distances, in list order) -> the k best under the rule"""
    ids, dist = np.asarray(ids, dtype=np.int32), np.asarray(dist, dtype=np.float64)
    o = rank(dist)
    ids, dist = ids[o], dist[o]
    keep = rule_keeps(ids, dist, rule)
    return cut(ids[keep], dist[keep], k)


def knn_allow(cands, mask, distance, k, rule=KEEP):
    """filter, then rank: the definition.  distance(ids) -> the distances of those rows to the query"""
    lst = allowed_list(cands, mask)
    return answer(lst, distance(lst) if len(lst) else np.zeros(0), k, rule)


def knn_rank_then_filter(cands, mask, distance, k, rule=KEEP):
    """rank the WHOLE candidate list, drop the disallowed entries, then the rule and the cut: the same
    answer (a stable filter commutes with a stable sort)"""
    c = np.asarray(cands, dtype=np.int32)
    dist = distance(c) if len(c) else np.zeros(0)
    o = rank(dist)
    return from_ranked(c[o], dist[o], mask, k, rule)


def from_ranked(ids, dist, mask, k, rule=KEEP):
    """a ranked listing of every candidate entry -> drop the disallowed, the rule, the cut"""
    ids, dist = np.asarray(ids, dtype=np.int32), np.asarray(dist, dtype=np.float64)
    ok = np.asarray(mask, dtype=bool)[ids] if len(ids) else np.zeros(0, dtype=bool)
    ids, dist = ids[ok], dist[ok]
    keep = rule_keeps(ids, dist, rule)
    return cut(ids[keep], dist[keep], k)


def knn_rule_then_filter(cands, mask, distance, k, rule):
    """the WRONG order: the rule over the whole list, then the filter (what a caller gets who
    filters the answer of the unfiltered query with k = everything)"""
    c = np.asarray(cands, dtype=np.int32)
    dist = distance(c) if len(c) else np.zeros(0)
    o = rank(dist)
    ids, dist = c[o], dist[o]
    keep = rule_keeps(ids, dist, rule)
    ids, dist = ids[keep], dist[keep]
    ok = np.asarray(mask, dtype=bool)[ids] if len(ids) else np.zeros(0, dtype=bool)
    return cut(ids[ok], dist[ok], k)


def knn_take_k_then_filter(cands, mask, distance, k, rule=KEEP):
    """today's route: the unfiltered answer of k entries, the disallowed ones dropped afterwards"""
    c = np.asarray(cands, dtype=np.int32)
    oi, od, cnt = answer(c, distance(c) if len(c) else np.zeros(0), k, rule)
    ok = np.asarray(mask, dtype=bool)[oi[:cnt]]
    return cut(oi[:cnt][ok], od[:cnt][ok], k)


def batch(fn, off, cids, T, mask, distance, k, rule=KEEP):
    """fn: one of the per-query functions above; distance(i, ids) -> distances of rows `ids` to query i;
    -> (ids[nq][k], dist[nq][k], count[nq])"""
    nq = (len(off) - 1) // T
    oi = np.empty((nq, k), dtype=np.int32)
    od = np.empty((nq, k))
    oc = np.empty(nq, dtype=np.int32)
    for i in range(nq):
        oi[i], od[i], oc[i] = fn(cids[off[i * T]:off[(i + 1) * T]], mask, lambda ids: distance(i, ids), k, rule)
    return oi, od, oc


def from_ranked_batch(all_ids, all_dist, all_cnt, mask, k, rule=KEEP):
    nq = len(all_cnt)
    oi = np.empty((nq, k), dtype=np.int32)
    od = np.empty((nq, k))
    oc = np.empty(nq, dtype=np.int32)
    for i in range(nq):
        m = all_cnt[i]
        oi[i], od[i], oc[i] = from_ranked(all_ids[i, :m], all_dist[i, :m], mask, k, rule)
    return oi, od, oc


# ------------------------------------------------------------------ the exhaustive answer
def brute_allow(dist_all, mask, k):
    """the distances of ALL n rows to one query -> the k best allowed rows by (distance, id), NaN last"""
    ids = np.flatnonzero(np.asarray(mask, dtype=bool)).astype(np.int32)
    return answer(ids, np.asarray(dist_all, dtype=np.float64)[ids], k, KEEP)[:2]


def map_back(sub_ids, mask):
    """ids of bruteKnn over compactRows(data, mask) -> ids of the whole data set (-1 stays)"""
    allowed = np.flatnonzero(np.asarray(mask, dtype=bool)).astype(np.int32)
    sub_ids = np.asarray(sub_ids)
    out = np.full(sub_ids.shape, -1, dtype=np.int32)
    ok = sub_ids >= 0
    out[ok] = allowed[sub_ids[ok]]
    return out
