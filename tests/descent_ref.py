"""The descent of a query through a forest restated on the query's OWN keys (plain Python and
numpy, f64: neither the oracle nor the library is called).  Not a test module.

rpt_knn_* / rpt_candidates project the query batch once (Pq[T][L][nq], the forest's projection mode)
and then walk on Pq, thr, mglo, mghi and the topology alone, so given the keys the candidate list is
a pure function.  This file restates that function, RPTree.hs:299-314 as documented at `traverse`
in csrc/knn.hip, by RECURSION (the kernels are stackless or keep explicit stacks):

    node of n points at offset off, level l, heap slot h
      Tip  when l >= L or n <= min_leaf                      -> the range (off, n)
      Bin  proj = key[l] widened to f64, th = thr[h], dl = |mglo[h] - proj|, dr = |mghi[h] - proj|
           both children when (proj < th and dl > dr) or (proj > th and dl < dr), left first
           else the left child when proj < th, else the right one (proj == th goes right, and so
           does a NaN key: every comparison with it is false)
      the left child holds n // 2 points at off, the right one n - n // 2 at off + n // 2

`candidates_of_keys` walks the halving topology of a batch forest, `candidates_of_keys_x` an explicit
one (`kind` / `leaf_off` / `leaf_len` of RPStreamForest: 0 absent, 1 Bin, 2 Tip per heap slot; a Tip
may be empty and is a range all the same), `candidates_h_of_keys` / `candidates_h_of_keys_x` also
return every range's candidatesH priority (RPTree.hs:318-342: the smallest dl / dr met on the way
down, `p if p <= dl else dl`, +inf at the root), and `knn_h_select` is knnH's choice of buckets
(RPTree.hs:199-217 as `knn_h` in csrc/knn.hip states it).

Every call leaves a Trace in `last_trace` (and adds to the `trace` it is given): what the keys it
read were like, so that a test can assert that its inputs reach the edges they claim to reach."""
import numpy as np

INF = float("inf")


class Trace:
    """counts over the Bin nodes visited"""
    FIELDS = ("nodes", "key_eq_thr", "dl_eq_dr", "both", "nan_keys", "inf_keys")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, 0)

    def add(self, other):
        for f in self.FIELDS:
            setattr(self, f, getattr(self, f) + getattr(other, f))
        return self

    def __repr__(self):
        return "Trace(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f in self.FIELDS)


last_trace = Trace()


def _decide(key, th, lo, hi, tr):
    """one Bin node (RPTree.hs:303-314) -> (both, left, dl, dr)"""
    proj = float(key)
    dl = abs(lo - proj)
    dr = abs(hi - proj)
    both = (proj < th and dl > dr) or (proj > th and dl < dr)
    left = proj < th
    tr.nodes += 1
    tr.key_eq_thr += proj == th
    tr.dl_eq_dr += dl == dr
    tr.both += both
    tr.nan_keys += proj != proj
    tr.inf_keys += proj in (INF, -INF)
    return both, left, dl, dr


def _is_tip(level, n, L, min_leaf):
    return level >= L or n <= min_leaf


def _halves(n):
    nh = n // 2
    return nh, n - nh


def _walk(key, th, lo, hi, L, min_leaf, level, heap, off, n, p, out, tr):
    """the halving topology; appends (off, n, priority) left to right"""
    if _is_tip(level, n, L, min_leaf):
        out.append((off, n, p))
        return
    both, left, dl, dr = _decide(key[level], th[heap], lo[heap], hi[heap], tr)
    nl, nr = _halves(n)
    if both or left:
        _walk(key, th, lo, hi, L, min_leaf, level + 1, 2 * heap + 1, off, nl, p if p <= dl else dl, out, tr)
    if both or not left:
        _walk(key, th, lo, hi, L, min_leaf, level + 1, 2 * heap + 2, off + nl, nr, p if p <= dr else dr, out, tr)


def _walk_x(key, th, lo, hi, kind, leaf_off, leaf_len, level, heap, p, out, tr):
    """an explicit topology; an absent slot holds nothing"""
    if kind[heap] != 1:
        if kind[heap] == 2:
            out.append((int(leaf_off[heap]), int(leaf_len[heap]), p))
        return
    both, left, dl, dr = _decide(key[level], th[heap], lo[heap], hi[heap], tr)
    if both or left:
        _walk_x(key, th, lo, hi, kind, leaf_off, leaf_len, level + 1, 2 * heap + 1, p if p <= dl else dl, out, tr)
    if both or not left:
        _walk_x(key, th, lo, hi, kind, leaf_off, leaf_len, level + 1, 2 * heap + 2, p if p <= dr else dr, out, tr)


def _f64(a):
    return np.asarray(a).astype(np.float64)              # f32 keys widen exactly


def _finish(tr, trace):
    global last_trace
    last_trace = tr
    if trace is not None:
        trace.add(tr)


def candidates_h_of_keys(keys, thr, mglo, mghi, N, L, min_leaf, trace=None):
    """keys[T][L] of ONE query, thr / mglo / mghi [T][2^L - 1] -> per tree the list of
    (off, n, priority) of the leaves reached, left to right"""
    keys, thr, mglo, mghi = _f64(keys), _f64(thr), _f64(mglo), _f64(mghi)
    assert keys.ndim == 2 and keys.shape[1] == L and thr.shape == (keys.shape[0], (1 << L) - 1)
    tr, res = Trace(), []
    for t in range(keys.shape[0]):
        out = []
        _walk(keys[t].tolist(), thr[t].tolist(), mglo[t].tolist(), mghi[t].tolist(), L, min_leaf, 0, 0, 0, int(N),
              INF, out, tr)
        res.append(out)
    _finish(tr, trace)
    return res


def candidates_of_keys(keys, thr, mglo, mghi, N, L, min_leaf, trace=None):
    """-> per tree the list of (off, n) of the leaves reached, left to right"""
    return [[(o, n) for o, n, _ in tree]
            for tree in candidates_h_of_keys(keys, thr, mglo, mghi, N, L, min_leaf, trace)]


def _kind_of(kind, t):
    kind = np.asarray(kind)
    return (kind if kind.ndim == 1 else kind[t]).tolist()


def _rows_of(a, t):
    a = np.asarray(a)
    return (a if a.ndim == 1 else a[t]).tolist()


def candidates_h_of_keys_x(keys, thr, mglo, mghi, kind, leaf_off, leaf_len, trace=None):
    """the same over an explicit topology: kind / leaf_off / leaf_len per heap slot, one set for all
    trees ([S], RPStreamForest) or one per tree ([T][S], the oracle's StreamForest)"""
    keys, thr, mglo, mghi = _f64(keys), _f64(thr), _f64(mglo), _f64(mghi)
    tr, res = Trace(), []
    for t in range(keys.shape[0]):
        out = []
        _walk_x(keys[t].tolist(), thr[t].tolist(), mglo[t].tolist(), mghi[t].tolist(), _kind_of(kind, t),
                _rows_of(leaf_off, t), _rows_of(leaf_len, t), 0, 0, INF, out, tr)
        res.append(out)
    _finish(tr, trace)
    return res


def candidates_of_keys_x(keys, thr, mglo, mghi, kind, leaf_off, leaf_len, trace=None):
    return [[(o, n) for o, n, _ in tree]
            for tree in candidates_h_of_keys_x(keys, thr, mglo, mghi, kind, leaf_off, leaf_len, trace)]


def ids_of_ranges(perm, ranges):
    """perm[T][N] and the per-tree range lists -> per tree the candidate ids, left to right"""
    return [np.concatenate([perm[t, o:o + n] for o, n in ((r[0], r[1]) for r in tree)] +
                           [np.empty(0, dtype=perm.dtype)]) for t, tree in enumerate(ranges)]


def knn_h_select(ranges_h, k):
    """knnH's choice of buckets (RPTree.hs:199-217): the (off, n, priority) entries of all trees in
    (tree, left-to-right) order, stably sorted by priority; buckets are taken while the running count
    of POINTS stays <= k, but until at least one point is held; the bucket taken last comes first.
    -> [(tree, off, n)] in output order.  (Priorities must not be NaN: no order is defined then.)"""
    entries = [(p, t, o, n) for t, tree in enumerate(ranges_h) for o, n, p in tree]
    assert all(e[0] == e[0] for e in entries), "a NaN priority"
    order = sorted(range(len(entries)), key=lambda i: entries[i][0])         # stable
    taken, held = [], 0
    for i in order:
        _, t, o, n = entries[i]
        if n + held > k and held > 0:
            break
        taken.append((t, o, n))
        held += n
    return taken[::-1]


def knn_h_ids(perm, ranges_h, k):
    sel = knn_h_select(ranges_h, k)
    return np.concatenate([perm[t, o:o + n] for t, o, n in sel] + [np.empty(0, dtype=perm.dtype)])


# ------------------------------------------------------------------ inputs
def depth(n, min_leaf):
    """levels until every node holds at most min_leaf points"""
    L = 0
    while n > min_leaf:
        n, L = n - n // 2, L + 1
    return L


def lattice_rows(rng, n, d):
    """integers -3 .. 3: against hyperplanes of 0 / +-1 every key is a small integer in every
    arithmetic, so keys tie with thresholds and margins whatever kernel computed them"""
    return rng.integers(-3, 4, size=(n, d)).astype(np.float64)


def lattice_planes(rng, T, L, d):
    return rng.integers(-1, 2, size=(T, L, d)).astype(np.float64)


QUERY_KINDS = ("fresh", "gap", "stored", "mid", "x8", "near", "nan", "inf", "mixed")


def make_queries(kind, rng, X, nq):
    """-> Q[nq][d] float64 derived from the rows X:
        fresh   new points of the rows' kind (lattice rows: new lattice points, keys ON thresholds)
        gap     rows + 0.25 * integers in -2 .. 2 (lattice rows: keys in the gaps between the rows' keys)
        stored  rows as they are
        mid     midpoints of two rows (near many cuts: both children often)
        x8      rows * 8 (far outside the margins)
        near    rows * 1.001 + 0.003
        nan     a NaN in one coordinate of every query;  inf: +-inf there
        mixed   finite ("gap"), NaN and inf queries in turn"""
    n, d = X.shape
    X = np.asarray(X, dtype=np.float64)
    rows = X[rng.integers(0, n, nq)].copy()
    integral = bool(np.all(X == np.round(X)))
    if kind == "stored":
        return rows
    if kind == "fresh":
        return lattice_rows(rng, nq, d) if integral else rng.standard_normal((nq, d))
    if kind == "gap":
        return rows + 0.25 * rng.integers(-2, 3, size=(nq, d))
    if kind == "mid":
        return 0.5 * (rows + X[rng.integers(0, n, nq)])
    if kind == "x8":
        return rows * 8.0
    if kind == "near":
        return rows * 1.001 + 0.003
    col = rng.integers(0, d, nq)
    i = np.arange(nq)
    if kind == "nan":
        rows[i, col] = np.nan
        return rows
    if kind == "inf":
        rows[i, col] = np.where(rng.random(nq) < 0.5, np.inf, -np.inf)
        return rows
    assert kind == "mixed", kind
    Q = rows + 0.25 * rng.integers(-2, 3, size=(nq, d))
    Q[i[1::3], col[1::3]] = np.nan
    Q[i[2::3], col[2::3]] = np.where(rng.random(len(i[2::3])) < 0.5, np.inf, -np.inf)
    return Q


def axes_rows(rng, n, d):
    """coordinate l of row i is bit l of i (from the top) as -1 / +1, plus noise of 0.1: against
    `axes_planes` the points of a node at level l fall into two clusters around -1 and +1, which the
    median separates.  For the queries of `fan_queries`."""
    Lb = max(1, int(np.ceil(np.log2(n))))
    assert d >= Lb
    X = 0.1 * rng.standard_normal((n, d))
    X[:, :Lb] += ((np.arange(n)[:, None] >> np.arange(Lb)[::-1][None, :]) & 1) * 2.0 - 1.0
    return X


def axes_planes(rng, T, L, d):
    """level l's hyperplane is the l-th axis plus a small random vector (the trees differ)"""
    assert d >= L
    R = 0.05 * rng.standard_normal((T, L, d))
    R[:, np.arange(L), np.arange(L)] += 1.0
    return R


def fan_queries(rng, X, nq, m):
    """rows of `axes_rows` with m of the first coordinates set to 0.4: between the middle of the gap
    and the right cluster at those levels, where the rule takes both children in every tree, so a
    query reaches about 2^m leaves per tree"""
    n, d = X.shape
    Lb = max(1, int(np.ceil(np.log2(n))))
    Q = np.asarray(X, dtype=np.float64)[rng.integers(0, n, nq)].copy()
    for q in Q:
        q[rng.choice(Lb, m, replace=False)] = 0.4
    return Q
