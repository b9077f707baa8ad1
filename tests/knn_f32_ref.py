"""numpy restatement of the L2 kNN on dense f32 / bf16 rows, the inputs it is tested on and the
rigorous check of an answer computed in rounded f32 arithmetic; shared by tests/test_knn_f32_host.py
(no GPU) and tests/test_gpu_knn_f32_l2.py.  Not a test module.

The definition (include/rptree_hip.h, rpt_knn_*; the selection rules restated from topk_from and
rpo_brute_knn_dense in oracle/rptree_oracle.cpp): one query's candidates in candidate order (tree
ascending, then leaf order), each with a distance, ranked by (distance, candidate position); the
duplicate rule; the first k.  On f32 / bf16 rows the distance the device ranks on is its own f32
squared distance, which the project bounds (rp-tree_amd/csrc/knn.hip, TierBounds, "f32 DATA",
Bf in TierBounds::make) against the true distance D of the exactly widened rows:

    |dist - D| <= (d + 2) 2^-24 D + sqrt(d) 4e-23

`check_interval` holds an answer to everything that bound and the definition imply together, for
every query and with no escape for near-ties; where f32 arithmetic is exact (the lattice rows below)
the answer is the definition's, bit for bit, and `knn_from_candidates` is compared directly."""
import math

import numpy as np

KEEP, DEDUP, DEDUP_DISTANCE = 0, 1, 2        # RPT_KNN_KEEP_DUPLICATES, RPT_KNN_DEDUP, RPT_KNN_DEDUP_DISTANCE

U32 = 2.0 ** -24                             # knn.hip, TierBounds::make: u = 5.9604644775390625e-08


def bound_rel(d):
    """knn.hip, TierBounds ("f32 DATA: ... within Bf = (d + 2) u of D"); the code carries the same
    value times 1.01 as slack of its own, the tests hold the kernels to the stated one"""
    return (d + 2) * U32


def bound_abs(d):
    """knn.hip, TierBounds::make (A of the f32 arithmetic): products in the f32 subnormal range"""
    return math.sqrt(d) * 4e-23


# ------------------------------------------------------------------ element types
def to_bf16(a):
    """float array -> bf16 bit patterns (uint16), round to nearest even: rptree_amd.to_bf16 restated,
    so that the host tests need no device library"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) >> 16).astype(np.uint16)


def from_bf16(u16):
    return (np.ascontiguousarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def as_dtype(a, dtype):
    """the float32 array holding `a` rounded to the element type ("f32" / "bf16")"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return from_bf16(to_bf16(a)) if dtype == "bf16" else a


# ------------------------------------------------------------------ the definition
def exact_dist(X64, q64):
    """sqrt(sum((x - q)^2)) in f64 of exactly widened f32 / bf16 rows.  Every difference is exact in
    f64 at the magnitudes the tests use (checked here against long double, 64 bits of mantissa); the
    sum of d squares is then within d 2^-53 relative, and exact wherever f32 arithmetic is."""
    X64 = np.asarray(X64, dtype=np.float64)
    q64 = np.asarray(q64, dtype=np.float64)
    t = X64 - q64[None, :]
    tl = X64.astype(np.longdouble) - q64.astype(np.longdouble)[None, :]
    assert np.array_equal(t.astype(np.longdouble), tl), "a difference is not exact in f64"
    return np.sqrt((t * t).sum(axis=1))


def ranked(cands, D, rule):
    """every entry the rule admits, in answer order -> (ids, distances); D[j] is the distance of
    cands[j].  KEEP: all of them by (distance, position).  DEDUP: each id once, at its first position
    (copies of an id have equal distances, so the first in rank order is the first in position).
    DEDUP_DISTANCE: knnPQ's nub on the distance values, the first entry of every value."""
    cands = np.asarray(cands)
    D = np.asarray(D, dtype=np.float64)
    assert cands.shape == D.shape and not np.isnan(D).any()
    order = np.lexsort((np.arange(len(D)), D))
    ids, val = cands[order], D[order]
    if rule == DEDUP:
        first = np.sort(np.unique(ids, return_index=True)[1])
        ids, val = ids[first], val[first]
    elif rule == DEDUP_DISTANCE:
        new = np.ones(len(val), dtype=bool)
        new[1:] = val[1:] != val[:-1]
        ids, val = ids[new], val[new]
    else:
        assert rule == KEEP
    return ids.astype(np.int32), val


def padded(ids, val, k):
    """the first k of a ranked list as the entry points return them: ids[k], dist[k], count"""
    cnt = min(k, len(ids))
    oi = np.full(k, -1, dtype=np.int32)
    od = np.full(k, np.inf)
    oi[:cnt], od[:cnt] = ids[:cnt], val[:cnt]
    return oi, od, cnt


def knn_from_candidates(cands, D, k, rule):
    """the k best of one query's candidates by (distance, candidate position) under the duplicate
    rule -> (ids[k], dist[k], count); unused slots hold -1 / +inf"""
    return padded(*ranked(cands, D, rule), k)


def brute_from_rows(X, q, k):
    """the k best of ALL rows by (distance, id) -> (ids[k], dist[k], count)"""
    return knn_from_candidates(np.arange(len(X), dtype=np.int32), exact_dist(X, q), k, KEEP)


def voted(cands, v):
    """the ids found at least v times, ascending (RPT_KNN_VOTE: the order of keepCounts)"""
    ids, c = np.unique(np.asarray(cands), return_counts=True)
    return ids[c >= v].astype(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------ the interval check
def interval_violation(cands, D, ids, dist, cnt, k, rule, d):
    """None, or what is wrong with one answer (ids[k], dist[k], cnt) to a query whose candidates,
    in candidate order, are cands with TRUE distances D (one per entry), when the answer is the k
    best by (a device value within rel D + abs_ of D, candidate position) under `rule`
    (KEEP or DEDUP).  Everything asserted follows from that contract; nothing is measured."""
    assert rule in (KEEP, DEDUP)
    cands = np.asarray(cands)
    D = np.asarray(D, dtype=np.float64)
    ids, dist, cnt = np.asarray(ids), np.asarray(dist, dtype=np.float64), int(cnt)
    rel, abs_ = bound_rel(d), bound_abs(d)
    order = np.argsort(cands, kind="stable")             # positions grouped by id, ascending inside
    uid, start, copies = np.unique(cands[order], return_index=True, return_counts=True)
    Did = D[order[start]]                                # copies of one id are one row: one distance
    assert np.array_equal(np.repeat(Did, copies), D[order])
    admitted = len(cands) if rule == KEEP else len(uid)
    if cnt != min(k, admitted):
        return "count %d, want %d" % (cnt, min(k, admitted))
    if not (np.all(ids[cnt:] == -1) and np.all(np.isposinf(dist[cnt:]))):
        return "padding"
    if cnt == 0:
        return None
    rid, rdist = ids[:cnt], dist[:cnt]
    slot = np.searchsorted(uid, rid)
    if np.any(slot >= len(uid)) or np.any(uid[np.minimum(slot, len(uid) - 1)] != rid):
        return "an id that is no candidate"
    taken = np.bincount(slot, minlength=len(uid))
    admits = copies if rule == KEEP else np.ones_like(copies)
    if np.any(taken > admits):
        return "id %d more often than the rule admits" % uid[np.argmax(taken - admits)]
    Dr = Did[slot]
    err = np.abs(rdist - Dr)
    if not np.all(err <= rel * Dr + abs_):               # (a NaN fails too)
        j = int(np.argmax(~(err <= rel * Dr + abs_)))
        return "distance %r of id %d at rank %d: the true one is %r, %.3g of the bound" % (
            rdist[j], rid[j], j, Dr[j], err[j] / (rel * Dr[j] + abs_))
    if np.any(np.diff(rdist) < 0):
        return "distances decrease at rank %d" % (int(np.argmax(np.diff(rdist) < 0)) + 1)
    # completeness: an entry left out has a device value >= the last one returned, and its device
    # value cannot exceed D (1 + rel) + abs_
    left = admits - taken
    low = (Did * (1.0 + rel) + abs_ < rdist[-1]) & (left > 0)
    if np.any(low):
        j = int(np.argmax(low))
        return "id %d (true distance %r, %d entries left out) belongs before the last one returned (%r)" % (
            uid[j], Did[j], left[j], rdist[-1])
    # copies and ties: the r-th returned copy of an id is its r-th position (equal values, ranked by
    # position: the returned copies are a prefix of the id's positions), copies of an id carry one
    # value, and entries with bit-equal values stand in ascending position
    nth = np.zeros(cnt, dtype=np.int64)                  # how many earlier slots hold the same id
    o2 = np.argsort(slot, kind="stable")
    s2 = slot[o2]
    run0 = np.concatenate([[0], np.flatnonzero(np.diff(s2)) + 1])
    nth[o2] = np.arange(cnt) - np.repeat(run0, np.diff(np.concatenate([run0, [cnt]])))
    first_val = rdist[o2][np.repeat(run0, np.diff(np.concatenate([run0, [cnt]])))]
    if np.any(rdist[o2].view(np.uint64) != first_val.view(np.uint64)):
        return "copies of one id with different distances"
    pos = order[start[slot] + nth]
    tie = rdist[1:].view(np.uint64) == rdist[:-1].view(np.uint64)
    if np.any(tie & (np.diff(pos) < 0)):
        j = int(np.argmax(tie & (np.diff(pos) < 0))) + 1
        return "equal distances at ranks %d, %d are not in candidate order" % (j - 1, j)
    return None


def check_interval(cands, D, ids, dist, cnt, k, rule, d):
    why = interval_violation(cands, D, ids, dist, cnt, k, rule, d)
    assert why is None, why


def worst_ratio(cands, D, ids, dist, cnt, d):
    """largest |dist - D| / (rel D + abs_) over the returned entries of one answer"""
    cands, D = np.asarray(cands), np.asarray(D, dtype=np.float64)
    if cnt == 0:
        return 0.0
    order = np.argsort(cands, kind="stable")
    Dr = D[order[np.searchsorted(cands[order], np.asarray(ids)[:cnt])]]
    return float(np.max(np.abs(np.asarray(dist)[:cnt] - Dr) / (bound_rel(d) * Dr + bound_abs(d))))


# ------------------------------------------------------------------ f32 kernels simulated in numpy
def sim_fold(Xc, q):
    """the squared distance as an f32 left fold: every difference, square and sum rounded to f32"""
    Xc, q = np.asarray(Xc, dtype=np.float32), np.asarray(q, dtype=np.float32)
    s = np.zeros(len(Xc), dtype=np.float32)
    for j in range(Xc.shape[1]):
        t = Xc[:, j] - q[j]
        s = s + t * t
    assert s.dtype == np.float32
    return s


def sim_lanes(Xc, q):
    """... as 64 lanes strided over the columns, each an f32 left fold, then an xor butterfly"""
    Xc, q = np.asarray(Xc, dtype=np.float32), np.asarray(q, dtype=np.float32)
    lanes = np.zeros((len(Xc), 64), dtype=np.float32)
    for j in range(Xc.shape[1]):
        t = Xc[:, j] - q[j]
        lanes[:, j % 64] = lanes[:, j % 64] + t * t
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    assert lanes.dtype == np.float32
    return lanes[:, 0]


def sim_expansion(Xc, q):
    """what the kernels must NOT do: |x|^2 + |q|^2 - 2 x.q, every operation in f32"""
    Xc, q = np.asarray(Xc, dtype=np.float32), np.asarray(q, dtype=np.float32)
    xx = np.zeros(len(Xc), dtype=np.float32)
    xq = np.zeros(len(Xc), dtype=np.float32)
    qq = np.float32(0)
    for j in range(Xc.shape[1]):
        xx = xx + Xc[:, j] * Xc[:, j]
        xq = xq + Xc[:, j] * q[j]
        qq = qq + q[j] * q[j]
    return np.maximum(xx + qq - np.float32(2) * xq, np.float32(0))


SIMS = {"fold": sim_fold, "lanes": sim_lanes}


def sim_knn(cands, Xc, q, k, rule, sq=sim_fold):
    """the kernels' rule with a simulated f32 sum: the k best by (f32 squared distance, position),
    the distance returned is sqrt((double)that)"""
    return knn_from_candidates(cands, np.sqrt(sq(Xc, q).astype(np.float64)), k, rule)


# ------------------------------------------------------------------ inputs
NQ = 48
KS = (1, 10, 24, 50)
FAMILIES = ("cont", "offset", "mixed", "self", "dups")
LATTICE_M = 8.0                              # |x| <= M, step 1/2

# (n, d, T, minLeaf): the smallest shapes that still reach each row layout and kernel
SHAPES_F32 = [
    (6000, 16, 12, 100),     # 4 sixteen-byte pieces, workgroup kernel
    (6000, 16, 4, 100),      # few candidates: wave / shard kernels
    (5000, 24, 6, 60),       # rows that are not 16 n bytes for the int8 shadow: half tier
    (4000, 208, 4, 200),     # 13 pieces
    (3000, 1040, 6, 200),    # long rows
    (3000, 37, 5, 50),       # odd length, unaligned rows
    (700, 8, 3, 400),        # leaves larger than a wave's list
]
SHAPES_BF16 = [SHAPES_F32[0], SHAPES_F32[3], SHAPES_F32[4], (3000, 72, 5, 50)]
BRUTE_SHAPES = [(3000, 16), (2000, 208), (1500, 37), (1000, 1040)]
BRUTE_KS = (1, 10, 64)


def lattice_is_exact(d, M=LATTICE_M):
    """rows and queries on the lattice of step 1/2 with |x| <= M: a difference is a multiple of 1/2
    below 2 M, its square a multiple of 1/4 below (2 M)^2, and every partial sum of d squares, in any
    order, a multiple of 1/4 below d (2 M)^2: an integer below 2^24 when counted in quarters, hence
    an f32 (and a bf16 difference widened to f32) with no rounding anywhere"""
    return d * (2 * M) ** 2 * 4 < 2 ** 24


def lattice_rows(rng, n, d):
    return np.clip(np.round(2.0 * rng.standard_normal((n, d))) / 2.0, -LATTICE_M, LATTICE_M).astype(np.float32)


def lattice_set(n, d, dtype="f32", seed=0, nq=NQ):
    """rows round(2 N(0,1)) / 2 clipped to |x| <= 8 (exact in bf16: 5 bits); queries: a third stored
    rows, a third stored rows with one coordinate moved by 1/2 (towards 0 at the clip), a third
    fresh lattice points -> (X, Q) as float32"""
    rng = np.random.default_rng([seed, n, d])
    X = lattice_rows(rng, n, d)
    Q = X[rng.integers(0, n, nq)].copy()
    for i in range(nq // 3, 2 * (nq // 3)):
        j = int(rng.integers(0, d))
        Q[i, j] += np.float32(-0.5 if Q[i, j] > 0 else 0.5)
    Q[2 * (nq // 3):] = lattice_rows(rng, nq - 2 * (nq // 3), d)
    assert np.array_equal(as_dtype(X, dtype), X) and np.array_equal(as_dtype(Q, dtype), Q)
    assert np.abs(X).max() <= LATTICE_M and np.abs(Q).max() <= LATTICE_M
    return X, Q


def family_set(kind, n, d, dtype="f32", seed=0, nq=NQ):
    """(X, Q) as float32 holding values of the element type; the queries are rounded to it as well
        cont    N(0,1), queries = rows + 0.003 (bf16: + 0.01, 0.003 is below half an ulp of most elements)
        offset  f32: 1000 + 0.01 N(0,1); bf16: 64 + lattice / 4: all the information in the low bits
        mixed   N(0,1), every other coordinate times 1e4: one kind of coordinate dominates the sum
        self    N(0,1), queries ARE stored rows: one copy per tree at distance exactly 0
        dups    N(0,1), every row stored 3 times under different ids"""
    rng = np.random.default_rng([seed, n, d, FAMILIES.index(kind)])
    step = 0.01 if dtype == "bf16" else 0.003
    if kind == "offset":
        if dtype == "bf16":
            X = 64.0 + lattice_rows(rng, n, d) / 4.0
            shift = 0.5 * np.round(rng.standard_normal((nq, d)))
        else:
            X = 1000.0 + 0.01 * rng.standard_normal((n, d))
            shift = step
    elif kind == "dups":
        m = n // 3
        B = rng.standard_normal((m, d))
        X = np.concatenate([B, B, B, rng.standard_normal((n - 3 * m, d))])
        shift = step
    else:
        X = rng.standard_normal((n, d))
        shift = 0.0 if kind == "self" else step
        if kind == "mixed":
            scale = np.where(np.arange(d) % 2 == 0, 1e4, 1.0)
            X, shift = X * scale, step * scale
    X = as_dtype(X, dtype)
    Q = as_dtype(X[rng.integers(0, n, nq)].astype(np.float64) + shift, dtype)
    return X, Q
