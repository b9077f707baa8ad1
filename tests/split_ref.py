"""The split of a forest restated on the forest's OWN stored keys (numpy only: neither the oracle
nor the library is called).

The contract at the top of csrc/split.hip fixes perm, thr, mglo and mghi once the keys P[T][L][N] are
given, however those keys were computed: a node of n points in order o is split by the STABLE sort
of o by the level's key (so ties fall back on the earlier levels' keys and finally on the id), the
left child is the first nh = n div 2 points of the sorted order, thr = p'[nh] and the margins are
the sorted neighbours p'[nh-1], p'[nh+1] (n == 2: (p'[0], p'[1]); n == 1: p'[0] twice).  Keys compare
as IEEE numbers: -0.0 and +0.0 tie, and what is reported is the stored key at the sorted position,
sign of zero included.  f32 keys widen to f64 exactly, so everything is compared in f64.

What this does not check: the accuracy of the keys themselves (the projection tolerance tests do)."""
from collections import namedtuple

import numpy as np

Split = namedtuple("Split", "perm thr mglo mghi")


def topology(n, L, min_leaf):
    """DFS list of (level, heap, offset, size, is_leaf) of the halving rule: a node is a leaf when
    level >= L or n <= min_leaf, its children hold n // 2 and n - n // 2 points at heap indices
    2h + 1 and 2h + 2."""
    out = []

    def go(level, heap, off, m):
        leaf = level >= L or m <= min_leaf
        out.append((level, heap, off, m, int(leaf)))
        if not leaf:
            go(level + 1, 2 * heap + 1, off, m // 2)
            go(level + 1, 2 * heap + 2, off + m // 2, m - m // 2)

    go(0, 0, 0, int(n))
    return np.array(out, dtype=np.int64).reshape(-1, 5)


def forest_of_keys(P, L, min_leaf):
    """P[T][L][N] (f32 or f64) -> Split(perm[T][N] int32, thr, mglo, mghi [T][2^L - 1] f64, NaN where
    no split happened).  A key that the recursion reads must not be NaN (asserted); keys it never
    reads may be anything."""
    P = np.asarray(P)
    T, L2, N = P.shape
    assert L2 == L and P.dtype in (np.float32, np.float64)
    topo = topology(N, L, min_leaf)
    perm = np.tile(np.arange(N, dtype=np.int32), (T, 1))
    nodes = [np.full((T, (1 << L) - 1), np.nan) for _ in range(3)]
    for level in range(L):
        rows = topo[(topo[:, 0] == level) & (topo[:, 4] == 0)]
        if len(rows) == 0:
            break
        heap, off, m = rows[:, 1], rows[:, 2], rows[:, 3]
        start = np.cumsum(m) - m                               # of every node among the active positions
        seg = np.repeat(np.arange(len(rows)), m)
        pos = off[seg] + np.arange(int(m.sum())) - start[seg]   # ascending: DFS order is offset order
        nh = m // 2
        at = (start + nh, start + np.where(m >= 3, nh - 1, 0), start + np.where(m >= 3, nh + 1, m - 1))
        for t in range(T):
            ids = perm[t, pos]
            key = P[t, level, ids].astype(np.float64)
            assert not np.isnan(key).any(), "NaN key read at tree %d level %d" % (t, level)
            order = np.lexsort((key, seg))                     # stable: ties keep the order they came in
            perm[t, pos] = ids[order]
            key = key[order]
            for a, i in zip(nodes, at):
                a[t, heap] = key[i]
    return Split(perm, *nodes)


def same_bits(a, b):
    """NaN exactly where b has NaN, identical bits elsewhere (so -0.0 is not +0.0)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


def assert_same_bits(a, b, what=""):
    if same_bits(a, b):
        return
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, "%s: shapes %s and %s" % (what, a.shape, b.shape)
    bad = (np.isnan(a) != np.isnan(b)) | (~np.isnan(a) & ~np.isnan(b) &
                                          (a.view(np.int64) != b.view(np.int64)))
    i = tuple(int(v[0]) for v in np.nonzero(bad))
    raise AssertionError("%s: %d entries differ in their bits, the first at %s: %r (sign bit %d) != %r (sign bit %d)"
                         % (what, int(bad.sum()), i, float(a[i]), np.signbit(a[i]), float(b[i]), np.signbit(b[i])))


def assert_forest_bits_equal(f, g, what=""):
    """two forests (anything with perm, thr, mglo, mghi): perm equal, node arrays equal as bits"""
    assert np.array_equal(f.perm, g.perm), what + " perm"
    for name in ("thr", "mglo", "mghi"):
        assert_same_bits(getattr(f, name), getattr(g, name), (what + " " + name).strip())


def first_difference(got, ref, P, L, min_leaf):
    """None, or a description of the first node (by level, then heap index) at which `got` is not
    `ref`: tree, level, heap, node size, position, and whether the keys there tie."""
    T, _, N = P.shape
    topo = topology(N, L, min_leaf)
    topo = topo[np.lexsort((topo[:, 1], topo[:, 0]))]
    for t in range(T):
        for level, heap, off, m, leaf in (tuple(int(v) for v in r) for r in topo):
            if leaf:
                if level == 0 or np.array_equal(got.perm[t, off:off + m], ref.perm[t, off:off + m]):
                    continue
                # same points (the parent passed), another order: the sort of the parent's level
                i = int(np.argmax(got.perm[t, off:off + m] != ref.perm[t, off:off + m]))
                a, b = int(got.perm[t, off + i]), int(ref.perm[t, off + i])
                return ("tree %d, leaf at level %d, heap %d, %d points, position %d: id %d where the "
                        "reference has %d; their keys at level %d %s"
                        % (t, level, heap, m, off + i, a, b, level - 1,
                           "tie" if P[t, level - 1, a] == P[t, level - 1, b] else "differ"))
            nh = m // 2
            gl, rl = np.sort(got.perm[t, off:off + nh]), np.sort(ref.perm[t, off:off + nh])
            gr, rr = np.sort(got.perm[t, off + nh:off + m]), np.sort(ref.perm[t, off + nh:off + m])
            if not (np.array_equal(gl, rl) and np.array_equal(gr, rr)):
                extra = np.setdiff1d(gl, rl)
                missing = np.setdiff1d(rl, gl)
                if len(extra) == 0 or len(missing) == 0:
                    return ("tree %d, level %d, heap %d, %d points at position %d: not the points of "
                            "the reference's node" % (t, level, heap, m, off))
                a, b = int(extra[0]), int(missing[0])
                return ("tree %d, level %d, heap %d, %d points at position %d: %d points on the wrong "
                        "side of the cut, e.g. id %d left where the reference has id %d; their keys %s"
                        % (t, level, heap, m, off, len(extra), a, b,
                           "tie" if P[t, level, a] == P[t, level, b] else "differ"))
            for name in ("thr", "mglo", "mghi"):
                a, b = getattr(got, name)[t, heap], getattr(ref, name)[t, heap]
                if not same_bits(a, b):
                    keys = np.sort(P[t, level, ref.perm[t, off:off + m]].astype(np.float64))
                    lo, hi = max(nh - 1, 0), min(nh + 1, m - 1)
                    return ("tree %d, level %d, heap %d, %d points at position %d: %s = %r (sign bit %d), "
                            "the reference has %r (sign bit %d); the keys around the cut %s"
                            % (t, level, heap, m, off, name, float(a), np.signbit(a), float(b),
                               np.signbit(b), "tie" if keys[lo] == keys[nh] or keys[nh] == keys[hi]
                               else "differ"))
    for name in ("thr", "mglo", "mghi"):                    # a value at a node that never split
        if not same_bits(getattr(got, name), getattr(ref, name)):
            return name + " differs at a node that does not split"
    return None


def assert_split_of_keys(got, P, L, min_leaf, ref=None):
    """got (perm, thr, mglo, mghi) is the split of the keys P; -> the reference (for reuse)"""
    P = np.asarray(P)
    if ref is None:
        ref = forest_of_keys(P, L, min_leaf)
    ok = np.array_equal(got.perm, ref.perm) and all(
        same_bits(getattr(got, n), getattr(ref, n)) for n in ("thr", "mglo", "mghi"))
    if not ok:
        raise AssertionError("not the split of the stored keys: " +
                             str(first_difference(got, ref, P, L, min_leaf)))
    return ref


def assert_forest_is_split_of_keys(f, P=None, ref=None):
    """A built forest against the reference split of its own downloaded keys: perm exactly, thr /
    mglo / mghi NaN where the reference has NaN and identical bits elsewhere.  -> (P, reference)"""
    if P is None:
        P = f.proj()
    assert not np.isnan(P).any(), "the forest stores NaN keys"
    got = Split(f.perm, f.thr, f.mglo, f.mghi)
    assert got.perm.dtype == np.int32
    return P, assert_split_of_keys(got, P, f.L, f.min_leaf, ref)
