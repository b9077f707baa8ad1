"""numpy restatement of the L2 kNN's definition on dense f64 rows and the inputs that attack its
cut, shared by tests/test_knn_l2_cut_host.py and tests/test_gpu_knn_l2_cut.py.  Not a test module.

    dist(x, q) = sqrt(((0 + (x0 - q0)(x0 - q0)) + (x1 - q1)(x1 - q1)) + ...)     metricDDL2, in Double

every candidate ranked by (NaN last, value, candidate position), the duplicate rule on those values,
the first k (RPTree.hs:174-176).  The device ranks on a lane-parallel sum of the same products; the
builders below put many DIFFERENT rows with mathematically equal distances (coordinate permutations
of one row) around the k-th place, so that the two sums order them differently, and `model_sum` is
one such second order (not the device's) with which the host test shows that they do."""
import numpy as np

MARGIN = 8                  # entries the device keeps beyond k by its own sum (kLfMargin)
BAND_KS = (7, 8, 10, 15, 16, 17, 24, 31, 32, 33, 40, 50)     # cuts inside a band of 48 behind 6 rows
WIDE_KS = (63, 64, 70)      # ... and inside a band of 120: the fused kernels' largest k, and one beyond
COPY_TREES = (5, 12, 32)


# ------------------------------------------------------------------ the definition
def fold_l2(Xc, q):
    """metricDDL2 of every row of Xc to q: the left fold from +0.0 (np.cumsum adds in order), one sqrt"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = Xc - q[None, :]
        P = np.concatenate([np.zeros((Xc.shape[0], 1)), t * t], axis=1)
        return np.sqrt(np.cumsum(P, axis=1)[:, -1])


def model_sum(Xc, q):
    """a second summation order of the same products: 64 lanes strided over the columns, each a
    left fold, then an xor butterfly over the lanes (32, 16, ... 1), one sqrt"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = Xc - q[None, :]
        P = t * t
        n, d = P.shape
        lanes = np.zeros((n, 64))
        for j in range(d):
            lanes[:, j % 64] = lanes[:, j % 64] + P[:, j]
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ o]
        return np.sqrt(lanes[:, 0])


def select(ids, vals, k, dedup):
    """stable order by (NaN last, value, position); dedup 0 keeps copies, 1 each id once, 2 each
    VALUE once (knnPQ's nub: NaN equals nothing); the first k"""
    ids, vals = np.asarray(ids), np.asarray(vals, dtype=np.float64)
    nan = np.isnan(vals)
    order = np.lexsort((np.arange(len(vals)), np.where(nan, 0.0, vals), nan))
    out_i, out_v, seen, last = [], [], set(), None
    for j in order:
        i, v = int(ids[j]), vals[j]
        if dedup == 1:
            if i in seen:
                continue
            seen.add(i)
        elif dedup == 2 and out_v and v == last:
            continue
        out_i.append(i)
        out_v.append(v)
        last = v
        if len(out_i) == k:
            break
    return np.array(out_i, dtype=np.int32), np.array(out_v, dtype=np.float64)


def model_rule(ids, Xc, q, k, dedup=0):
    """the rule under test with model_sum in the device's place: keep the k + MARGIN best by
    (model sum, position), evaluate those as the fold, select the k best of THOSE"""
    ids = np.asarray(ids)
    ms = model_sum(Xc, q)
    nan = np.isnan(ms)
    keep = np.lexsort((np.arange(len(ms)), np.where(nan, 0.0, ms), nan))[:k + MARGIN]
    keep = np.sort(keep)                                   # back in candidate order
    return select(ids[keep], fold_l2(Xc[keep], q), k, dedup)


def same_bits(a, b):
    """bit-equal doubles; a NaN only has to be a NaN (its sign and payload are the platform's)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64),
                                                                            b[~nb].view(np.uint64))


def mismatch(ids, dist, cnt, want):
    """None when one device answer (k ids, k distances, a count) is the wanted one, else a reason"""
    wi, wv = want
    k = len(ids)
    if cnt != len(wi):
        return "count %d, want %d" % (cnt, len(wi))
    if not np.array_equal(ids[:cnt], wi):
        j = int(np.argmax(ids[:cnt] != wi))
        return "id %d at rank %d, want %d" % (ids[j], j, wi[j])
    if not same_bits(dist[:cnt], wv):
        return "distance bits"
    if not (np.all(ids[cnt:k] == -1) and np.all(np.isposinf(dist[cnt:k]))):
        return "padding"
    return None


# ------------------------------------------------------------------ adversarial data
def distinct_permutations(rng, b, count):
    """count pairwise different coordinate permutations of the row b"""
    rows, seen = [], set()
    while len(rows) < count:
        x = b[rng.permutation(len(b))]
        key = x.tobytes()
        if key not in seen:
            seen.add(key)
            rows.append(x)
    return rows


def band_set(d, B=48, near=6, far=50, seed=0):
    """B pairwise different coordinate permutations of one positive unit row (the band), `near`
    rows clearly nearer in front and `far` rows clearly farther behind, the row order shuffled.
    Queries: 0, and the constant vector -1/4 (for which (x_j - c)^2 is a permutation as well, and
    |s b - c 1|^2 = s^2 + s sum(b) / 2 + d / 16 grows with the scale s > 0, so the near rows stay
    nearer and the far rows farther).  Returns (X, Q, mask of the band's rows)."""
    rng = np.random.default_rng(seed)
    b = np.abs(rng.standard_normal(d)) + 1e-3
    b /= np.linalg.norm(b)
    rows = [b * (0.5 + 0.01 * j) for j in range(near)]
    rows += distinct_permutations(rng, b, B)
    rows += [b * (2.0 + 0.01 * j) for j in range(far)]
    p = rng.permutation(len(rows))
    X = np.ascontiguousarray(np.array(rows)[p])
    Q = np.zeros((2, d))
    Q[1] = -0.25
    return X, Q, np.isin(p, np.arange(near, near + B))


BANDS = {                   # name -> (arguments of band_set, the k whose cut lies in the band)
    "d37": (dict(d=37, seed=11), BAND_KS),
    "d64": (dict(d=64, seed=12), BAND_KS),        # 512-byte rows: the short-row layout
    "d128": (dict(d=128, seed=13), BAND_KS),
    "wide": (dict(d=128, B=120, seed=14), WIDE_KS),
}


# The band that reaches the prefilter's fallback under default options: more rows than the
# small-shard kernels take (2100 candidates), and a band wider than the 224 entries a ranking tier
# keeps on its second, wider attempt, so no tier can hold the band whole and certify behind it.
RERUN_BAND = dict(d=128, B=300, far=2400, seed=15)
RERUN_K = 10


def with_nonfinite_queries(Q):
    """the band's queries, then a NaN query and one whose squares overflow to +inf"""
    d = Q.shape[1]
    qn = np.full(d, 0.125)
    qn[d // 2] = np.nan
    qi = np.zeros(d)
    qi[d // 3] = 1e200
    return np.vstack([Q, qn[None, :], qi[None, :]])


def copies_set(d=128, npairs=12, nfar=300, seed=32):
    """npairs pairs (row, a permutation of it), pair j on the sphere of radius 1 + 1e-3 j around
    the query 0 (clearly beyond pair j - 1), then nfar far rows.  In a forest of T one-leaf trees
    every row is a candidate T times: the copies of a pair's two rows fill 2 T consecutive places.
    Returns (X, Q): pair j is rows 2 j and 2 j + 1."""
    rng = np.random.default_rng(seed)
    rows = []
    for j in range(npairs):
        x = rng.standard_normal(d)
        x *= (1.0 + 1e-3 * j) / np.linalg.norm(x)
        y = x[rng.permutation(d)]
        while np.array_equal(x, y):
            y = x[rng.permutation(d)]
        rows += [x, y]
    far = rng.standard_normal((nfar, d)) * 3.0
    return np.ascontiguousarray(np.vstack([np.array(rows), far])), np.zeros((1, d))


def copies_ks(npairs, T, kmax):
    """one k inside the copies of each row of each pair (candidates by distance: T copies of one
    row of pair 0, T of the other, T of pair 1's, ...), capped at kmax"""
    ks = set()
    for j in range(npairs):
        ks.add(min(2 * j * T + T // 2, kmax))
        ks.add(min(2 * j * T + T + T // 2, kmax))
    return sorted(k for k in ks if k >= 1)


def flat_candidates(n, T):
    """the candidate list of every query in a forest of T one-leaf trees over n points"""
    return np.tile(np.arange(n, dtype=np.int32), T)
