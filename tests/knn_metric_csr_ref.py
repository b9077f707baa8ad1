"""numpy restatement of the cosine / inner-product kNN on CSR rows (rpt_knn_csr_metric_*,
rpt_brute_knn_csr_metric_*), independent of the library:

    dotS(x, q): from +0.0, over the columns stored in BOTH rows in ascending order,
                acc = acc + x_j * q_j, every product and sum rounded on its own
    inner  = -dotS(x, q)
    cosine = 1 - dotS(x, q) / (sqrt(dotS(x, x)) * sqrt(dotS(q, q)))        NaN ranks last

A CSR matrix is (rowptr, col, val); `dense` below is its dense-ified value matrix in f64 with the
mask of the stored entries.  The folds run over the columns in ascending order, vectorised over the
rows: one numpy addition per column is one rounded addition per row.
"""
import numpy as np

COSINE, INNER = "cosine", "inner"
U = 2.0 ** -53
MARGIN = 8                       # the kernels keep the best k + 8 different ids before the fold


def dense(rowptr, col, val, d):
    """-> (X [n][d] f64, P [n][d] bool: the stored entries)"""
    rowptr = np.asarray(rowptr)
    n = len(rowptr) - 1
    X = np.zeros((n, d), dtype=np.float64)
    P = np.zeros((n, d), dtype=bool)
    r = np.repeat(np.arange(n), np.diff(rowptr))
    X[r, col] = np.asarray(val).astype(np.float64)
    P[r, col] = True
    return X, P


def dots(X, P, qx, qp):
    """dotS(x_i, q) of every row i"""
    acc = np.zeros(X.shape[0], dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in np.flatnonzero(qp):
            acc = np.where(P[:, j], acc + X[:, j] * qx[j], acc)
    return acc


def self_dots(X, P):
    """dotS(x_i, x_i) of every row i"""
    acc = np.zeros(X.shape[0], dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(X.shape[1]):
            acc = np.where(P[:, j], acc + X[:, j] * X[:, j], acc)
    return acc


def dot_pair(xi, xv, qi, qv):
    """dotS of one pair given as (ascending indices, values): the two-pointer merge, pure Python"""
    acc, a, b = 0.0, 0, 0
    xi, qi = [int(t) for t in xi], [int(t) for t in qi]
    xv, qv = [float(t) for t in xv], [float(t) for t in qv]
    while a < len(xi) and b < len(qi):
        if xi[a] == qi[b]:
            acc = acc + np.float64(xv[a]) * np.float64(qv[b])
            a += 1
            b += 1
        elif xi[a] < qi[b]:
            a += 1
        else:
            b += 1
    return float(acc)


def value(metric, dot, xx, qq):
    with np.errstate(all="ignore"):
        if metric == INNER:
            return -np.asarray(dot, dtype=np.float64)
        return 1.0 - np.asarray(dot, dtype=np.float64) / (np.sqrt(xx) * np.sqrt(np.float64(qq)))


def distances(metric, X, P, rn, qx, qp):
    """the distance of every row to one query; rn = self_dots(X, P)"""
    qq = self_dots(qx[None, :], qp[None, :])[0]
    return value(metric, dots(X, P, qx, qp), rn, qq)


def order_of(dist, pos):
    """indices by (distance, pos), NaN behind every number (by pos), -0.0 tying with +0.0"""
    nan = np.isnan(dist)
    return np.lexsort((pos, np.where(nan, 0.0, dist) + 0.0, nan))


def brute(metric, data, queries, d, k):
    """the k best of rows 0 .. n-1 by (distance, id) -> ids [nq][k], dist [nq][k]"""
    X, P = dense(*data, d)
    Q, QP = dense(*queries, d)
    rn = self_dots(X, P)
    n, nq = X.shape[0], Q.shape[0]
    ids = np.full((nq, k), -1, dtype=np.int32)
    dist = np.full((nq, k), np.inf)
    for i in range(nq):
        dv = distances(metric, X, P, rn, Q[i], QP[i])
        o = order_of(dv, np.arange(n))[:k]
        ids[i, :len(o)] = o
        dist[i, :len(o)] = dv[o]
    return ids, dist


def knn_candidates(metric, Xd, cand, qx, qp, k, dedup):
    """the k best of the candidate ids `cand` (in candidate order) by (distance, position) under
    the duplicate rule: 0 duplicates kept, 1 each id once, 2 each distance once (== : NaN equals
    nothing).  Xd = (X, P, rn).  -> ids [k], dist [k], count"""
    X, P, rn = Xd
    cand = np.asarray(cand, dtype=np.int64)
    uniq, inv = np.unique(cand, return_inverse=True)
    dv = distances(metric, X[uniq], P[uniq], rn[uniq], qx, qp)[inv] if len(cand) else np.zeros(0)
    ids = np.full(k, -1, dtype=np.int32)
    dist = np.full(k, np.inf)
    w, seen, last = 0, set(), None
    for j in order_of(dv, np.arange(len(cand))):
        if w == k:
            break
        c, v = int(cand[j]), dv[j]
        if dedup == 1:
            if c in seen:
                continue
            seen.add(c)
        elif dedup == 2 and w > 0 and v == last:
            continue
        ids[w], dist[w], last = c, v, v
        w += 1
    return ids, dist, w


def dot_lanes(xi, xv, qdense):
    """the lane-parallel dot of one CSR row with the dense-ified query: sixteen lanes, lane l takes
    the nonzeros 64 t + 4 l .. + 3 for t = 0, 1, .. and adds their products in index order, then
    the fixed butterfly (xor 8, 4, 2, 1) adds the sixteen partial sums"""
    s = np.zeros(16, dtype=np.float64)
    xv = np.asarray(xv).astype(np.float64)
    with np.errstate(all="ignore"):
        for t in range(0, len(xi), 64):
            for l in range(16):
                for e in range(4):
                    j = t + 4 * l + e
                    if j < len(xi):
                        s[l] = s[l] + xv[j] * qdense[xi[j]]
        for o in (8, 4, 2, 1):
            s = s + s[np.arange(16) ^ o]
    return float(s[0])


def slack(metric, d, qq, max_rn, out_of_range):
    """E of the certified cut (NaN: the query cannot be certified).  max_rn: the largest dotS(x, x)
    of the data; out_of_range: some row that is not all zeros has dotS(x, x) outside
    [2^-900, 2^900]."""
    with np.errstate(all="ignore"):
        if metric == COSINE:
            if out_of_range or not (2.0 ** -900 <= qq <= 2.0 ** 900):
                return float("nan")
            return (2.0 * d + 16.0) * U
        xb = np.sqrt(np.float64(max_rn)) + d * 2.0 ** -537
        qb = np.sqrt(np.float64(qq)) + d * 2.0 ** -537
        e = (2.0 * d + 8.0) * U * xb * qb + (2.0 * d + 8.0) * 2.0 ** -1074
        return float(e) if e <= 2.0 ** 960 else float("nan")


def row_stats(X, P, rn):
    """(max rn with NaN above inf, some non-zero row's rn outside [2^-900, 2^900])"""
    mx = float("nan") if np.isnan(rn).any() else (float(rn.max()) if len(rn) else 0.0)
    with np.errstate(invalid="ignore"):
        out = ~((rn >= 2.0 ** -900) & (rn <= 2.0 ** 900))
    nonzero = ((X != 0.0) & P).any(axis=1)
    return mx, bool((out & nonzero).any())


def certified(metric, dv, k, d, qq, max_rn, out_of_range):
    """the reference's own certificate for a brute-force query over the values dv (one per id): the
    k-th value strictly below the (k + MARGIN + 1)-th different id's value less E"""
    o = order_of(dv, np.arange(len(dv)))
    if len(o) <= k + MARGIN:
        return True
    e = slack(metric, d, qq, max_rn, out_of_range)
    with np.errstate(invalid="ignore"):
        return bool(dv[o[k - 1]] < dv[o[k + MARGIN]] - e)


# ---- fixtures shared by the CPU and the GPU tests ----
def random_csr(rng, n, d, density, dtype=np.float64, zeros=0.0):
    """rows with strictly ascending columns; a share `zeros` of the stored values is +-0.0"""
    mask = rng.random((n, d)) < density
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(mask.sum(axis=1))
    col = np.nonzero(mask)[1].astype(np.int32)
    val = rng.standard_normal(len(col)).astype(dtype)
    if zeros:
        z = rng.random(len(col)) < zeros
        val[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0).astype(dtype)
    return rowptr, col, val


def fixture_a(dtype=np.float64):
    """the brute-force fixture of the GPU test: 9 000 x 70, density 0.3, with an empty row, two
    duplicate rows, one full-length row and a last row whose length is no multiple of 4; 13 queries:
    four stored rows, an empty query, nine fresh ones"""
    rng = np.random.default_rng(21)
    n, d = 9000, 70
    mask = rng.random((n, d)) < 0.3
    mask[17] = False                                  # an empty row
    mask[40] = True                                   # a full-length row
    mask[n - 1] = False
    mask[n - 1, [2, 9, 30, 41, 66]] = True            # last row: 5 entries
    vals = rng.standard_normal((n, d)).astype(dtype)
    mask[101], vals[101] = mask[100], vals[100]       # two duplicate rows
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    col = np.nonzero(mask)[1].astype(np.int32)
    val = vals[mask]
    qmask = rng.random((13, d)) < 0.3
    qvals = rng.standard_normal((13, d)).astype(dtype)
    for i, r in enumerate((0, 100, 40, n - 1)):
        qmask[i], qvals[i] = mask[r], vals[r]
    qmask[4] = False                                  # an empty query
    qrowptr = np.concatenate([[0], np.cumsum(qmask.sum(axis=1))]).astype(np.int64)
    return ((rowptr, col, val), (qrowptr, np.nonzero(qmask)[1].astype(np.int32), qvals[qmask]), d)
