"""tests/split_ref.py (the split restated on stored keys) pinned to the CPU oracle, and shown to be
sharp: fed the oracle's own keys it gives the oracle's perm exactly and its thr / mglo / mghi bit
for bit, signed zeros included; and one wrong step a kernel could plausibly take (a tie broken the
wrong way, a margin from the wrong neighbour, a zero of the wrong sign, a flushed denormal, a cut
one position off) fails the comparison every time.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref  # noqa: E402
from split_ref import Split  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def unit_planes(T, L, d):
    R = np.zeros((T, L, d))
    for l in range(L):
        R[:, l, l % d] = 1.0
    return R


def dense_case(oracle, name):
    """-> X, R, min_leaf"""
    if name == "cont":                                   # 1000 x 16 continuous
        n, d, T, ml = 1000, 16, 3, 20
        X = oracle.data_normal_dense2(1234, n, d)
        L, _, pnz = oracle.tree_cfg(ml, n, d)
        R, _ = oracle.forest_hyperplanes(1235137, T, L, pnz, d)
    elif name == "round":                                # 20 000 x 8 rounded to 0.1: ties at every level
        n, d, T, ml = 20000, 8, 2, 30
        X = np.round(oracle.data_normal_dense2(31, n, d), 1)
        L, _, _ = oracle.tree_cfg(ml, n, d)
        R = np.round(oracle.forest_hyperplanes(8, T, L, 1.0, d)[0], 1)
    elif name == "zeros":                                # 777 x 6, columns of +-0.0
        n, d, T, ml, L = 777, 6, 3, 4, 6
        rng = np.random.default_rng(5)
        X = np.where(rng.random((n, d)) < 0.5, 0.0, -0.0)
        X[rng.random(n) < 0.2] = rng.standard_normal(d)
        R = unit_planes(T, L, d)
    elif name == "same":                                 # 5000 identical rows
        n, d, T, ml, L = 5000, 6, 2, 100, 5
        X = np.ones((n, d))
        R, _ = oracle.forest_hyperplanes(3, T, L, 0.9, d)
    elif name == "big":                                  # 140 001 x 16 rounded: the streamed sizes
        n, d, T, ml = 140001, 16, 1, 40
        X = np.round(oracle.data_normal_dense2(77, n, d), 1)
        L, _, pnz = oracle.tree_cfg(ml, n, d)
        R, _ = oracle.forest_hyperplanes(3, T, L, pnz, d)
    elif name == "mixed":                                # leaves at two depths: keys the oracle never computes
        n, d, T, ml, L = 257, 5, 2, 128, 3
        X = oracle.data_normal_dense2(1234, n, d)
        R, _ = oracle.forest_hyperplanes(1235137, T, L, 0.6, d)
    else:
        raise KeyError(name)
    return X, R, ml


_built = {}


def oracle_forest(oracle, name):
    if name not in _built:
        X, R, ml = dense_case(oracle, name)
        _built[name] = oracle.forest_build_dense(X, R, ml, want_proj=True)
    return _built[name]


def as_split(fo):
    return Split(fo.perm, fo.thr, fo.mglo, fo.mghi)


def check_against_oracle(fo):
    ref = split_ref.forest_of_keys(fo.proj, fo.L, fo.min_leaf)   # (asserts: no NaN key is ever read)
    assert ref.perm.dtype == np.int32 and np.array_equal(ref.perm, fo.perm)
    for name in ("thr", "mglo", "mghi"):
        split_ref.assert_same_bits(getattr(ref, name), getattr(fo, name), name)
    split_ref.assert_split_of_keys(as_split(fo), fo.proj, fo.L, fo.min_leaf, ref)
    return ref


def test_topology_is_the_oracles(oracle):
    for n, L, ml in ((1000, 6, 20), (257, 3, 128), (1, 2, 0), (3, 4, 0), (50, 5, 100), (64, 0, 1),
                     (140001, 12, 40)):
        assert np.array_equal(split_ref.topology(n, L, ml), np.asarray(oracle.topology(n, L, ml)).reshape(-1, 5))


@pytest.mark.parametrize("name", ["cont", "round", "zeros", "same", "big", "mixed"])
def test_reference_on_the_oracles_keys_is_the_oracles_forest(oracle, name):
    fo = oracle_forest(oracle, name)
    check_against_oracle(fo)
    if name == "mixed":
        assert np.isnan(fo.proj).any()                  # keys the oracle left out: never read (asserted inside)
    if name == "zeros":
        # innerSD adds every product to an accumulator that starts at +0.0: no projection is -0.0
        assert (fo.proj[~np.isnan(fo.proj)] == 0).any() and not np.signbit(fo.proj[fo.proj == 0]).any()
    if name in ("cont", "zeros", "mixed"):              # ... and the recursive restatement agrees
        for t in range(fo.T):
            w = tree_by_recursion(fo.proj[t], fo.proj[t], fo.L, fo.min_leaf)
            split_ref.assert_split_of_keys(w, fo.proj[t:t + 1], fo.L, fo.min_leaf)


def test_reference_on_the_golden_forests(oracle):
    g = np.load(os.path.join(G, "forest_dense_1000x16.npz"))
    fo = oracle.forest_build_dense(g["X"], g["R"], int(g["min_leaf"]), want_proj=True)
    ref = check_against_oracle(fo)
    assert np.array_equal(ref.perm, g["perm"])
    for name in ("thr", "mglo", "mghi"):
        split_ref.assert_same_bits(getattr(ref, name), g[name], name)
    g = np.load(os.path.join(G, "forest_sparse_600x12.npz"))
    fo = oracle.forest_build_csr(g["rowptr"], g["col"], g["val"], int(g["d"]), g["R"], int(g["min_leaf"]),
                                 want_proj=True)
    ref = check_against_oracle(fo)
    assert np.array_equal(ref.perm, g["perm"])
    for name in ("thr", "mglo", "mghi"):
        split_ref.assert_same_bits(getattr(ref, name), g[name], name)


def test_reference_on_a_csr_forest_with_exact_zero_projections(oracle):
    rowptr, col, val = oracle.data_normal_sparse2(1234, 6000, 12, 0.25)
    R, _ = oracle.forest_hyperplanes(7, 3, 6, 0.3, 12)
    fo = oracle.forest_build_csr(rowptr, col, val, 12, R, 10, want_proj=True)
    assert (fo.proj[0, 0] == 0).sum() > 500
    check_against_oracle(fo)


def check_node_by_node(oracle, P, L, min_leaf, ref):
    """every node of `ref` is oracle.partition_at_median of the node's keys in the order the node
    received them -> number of tied keys met"""
    T, _, N = P.shape
    ties = 0
    for t in range(T):
        def go(ids, level, heap, off):
            nonlocal ties
            m = len(ids)
            if level >= L or m <= min_leaf:
                assert np.array_equal(ref.perm[t, off:off + m], ids)
                return
            keys = P[t, level, ids]
            ties += len(keys) - len(np.unique(keys))
            nh, order, thr, lo, hi = oracle.partition_at_median(keys)
            assert nh == m // 2
            for a, b in ((ref.thr, thr), (ref.mglo, lo), (ref.mghi, hi)):
                split_ref.assert_same_bits(a[t, heap], b, "tree %d heap %d" % (t, heap))
            go(ids[order[:nh]], level + 1, 2 * heap + 1, off)
            go(ids[order[nh:]], level + 1, 2 * heap + 2, off + nh)
        go(np.arange(N, dtype=np.int32), 0, 0, 0)
    return ties


@pytest.mark.parametrize("name", ["cont", "round"])
def test_reference_on_keys_rounded_to_f32_node_by_node(oracle, name):
    """The oracle's keys rounded to f32 (far more ties) and widened again: every node of the reference
    is oracle.partition_at_median of the same keys in the order the node received."""
    fo = oracle_forest(oracle, name)
    P32 = fo.proj.astype(np.float32)
    P = P32.astype(np.float64)
    ref = split_ref.forest_of_keys(P32, fo.L, fo.min_leaf)
    ref64 = split_ref.forest_of_keys(P, fo.L, fo.min_leaf)
    split_ref.assert_split_of_keys(ref, P, fo.L, fo.min_leaf, ref64)      # f32 keys widen exactly
    ties = check_node_by_node(oracle, P, fo.L, fo.min_leaf, ref)
    assert ties > (100 if name == "round" else 0)


class KeyForest:
    """keys given directly (no projection), the reference split of them"""

    def __init__(self, P, L, min_leaf):
        self.proj, self.L, self.min_leaf = P, L, min_leaf
        self.T, _, self.N = P.shape
        self.perm, self.thr, self.mglo, self.mghi = split_ref.forest_of_keys(P, L, min_leaf)


def signed_zero_keys():
    """777 points, 6 levels: the key columns are +-0.0 with one point in five continuous (a
    projection cannot be -0.0, a stored key can: what the kernels are handed is the key block)"""
    n, T, L = 777, 3, 6
    rng = np.random.default_rng(5)
    P = np.where(rng.random((T, L, n)) < 0.5, 0.0, -0.0)
    cont = rng.random(n) < 0.2
    P[:, :, cont] = rng.standard_normal((T, L, int(cont.sum())))
    return P


_zero_forest = []


def zero_forest():
    if not _zero_forest:
        _zero_forest.append(KeyForest(signed_zero_keys(), 6, 4))
    return _zero_forest[0]


def test_reference_on_signed_zero_keys_node_by_node(oracle):
    kf = zero_forest()
    assert check_node_by_node(oracle, kf.proj, kf.L, kf.min_leaf, kf) > 1000
    for a in (kf.thr, kf.mglo, kf.mghi):
        z = a[~np.isnan(a)]
        z = z[z == 0]
        assert np.signbit(z).any() and not np.signbit(z).all()   # both zeros stand at cuts and beside them


# ------------------------------------------------------------------------------ mutations
def tree_by_recursion(P, order_keys, L, min_leaf, by_id=False):
    """One tree, node by node: the points are ordered by `order_keys` (what a kernel compares) and
    thr / margins are read from P (what is stored).  by_id: ties broken by the id alone."""
    N = P.shape[1]
    perm = np.empty((1, N), dtype=np.int32)
    nodes = [np.full((1, (1 << L) - 1), np.nan) for _ in range(3)]

    def go(ids, level, heap, off):
        m = len(ids)
        if level >= L or m <= min_leaf:
            perm[0, off:off + m] = ids
            return
        k = order_keys[level, ids]
        order = np.lexsort((ids, k)) if by_id else np.argsort(k, kind="stable")
        ids = ids[order]
        p = P[level, ids].astype(np.float64)
        nh = m // 2
        nodes[0][0, heap] = p[nh]
        nodes[1][0, heap] = p[nh - 1] if m >= 3 else p[0]
        nodes[2][0, heap] = p[nh + 1] if m >= 3 else p[m - 1]
        go(ids[:nh], level + 1, 2 * heap + 1, off)
        go(ids[nh:], level + 1, 2 * heap + 2, off + nh)

    go(np.arange(N, dtype=np.int32), 0, 0, 0)
    return Split(perm, *nodes)


def last_split_nodes(fo):
    """(level, heap, off, m, sorted keys of tree 0) of the split nodes whose children are both leaves:
    the final perm inside them is the sorted order of their own level"""
    topo = split_ref.topology(fo.N, fo.L, fo.min_leaf)
    leaf = {int(r[1]): bool(r[4]) for r in topo}
    for level, heap, off, m, lf in (tuple(int(v) for v in r) for r in topo):
        if not lf and leaf[2 * heap + 1] and leaf[2 * heap + 2]:
            yield level, heap, off, m, fo.proj[0, level, fo.perm[0, off:off + m]]


def must_fail(got, fo, needle):
    with pytest.raises(AssertionError, match="not the split of the stored keys") as e:
        split_ref.assert_split_of_keys(got, fo.proj, fo.L, fo.min_leaf)
    assert needle in str(e.value), str(e.value)


def mutable(fo, trees=slice(None)):
    return Split(*(getattr(fo, n)[trees].copy() for n in ("perm", "thr", "mglo", "mghi")))


def test_mutation_tied_ids_swapped_inside_a_child(oracle):
    fo = oracle_forest(oracle, "round")
    for level, heap, off, m, keys in last_split_nodes(fo):
        nh = m // 2
        i = [j for j in range(m - 1) if keys[j] == keys[j + 1] and j + 1 != nh]
        if i:
            got = mutable(fo)
            got.perm[0, [off + i[0], off + i[0] + 1]] = got.perm[0, [off + i[0] + 1, off + i[0]]]
            must_fail(got, fo, "tie")
            return
    pytest.fail("no tie inside a leaf")


def test_mutation_tied_ids_swapped_across_the_cut(oracle):
    fo = oracle_forest(oracle, "round")
    for level, heap, off, m, keys in last_split_nodes(fo):
        nh = m // 2
        if keys[nh - 1] == keys[nh]:
            got = mutable(fo)
            got.perm[0, [off + nh - 1, off + nh]] = got.perm[0, [off + nh, off + nh - 1]]
            must_fail(got, fo, "wrong side of the cut")
            return
    pytest.fail("no tie across a cut")


def test_mutation_mghi_taken_from_the_cut_itself(oracle):
    fo = oracle_forest(oracle, "cont")
    got = mutable(fo)
    heap = 2
    assert fo.mghi[1, heap] != fo.thr[1, heap]
    got.mghi[1, heap] = got.thr[1, heap]
    must_fail(got, fo, "mghi")


def test_mutation_thr_with_the_other_sign_of_zero(oracle):
    fo = zero_forest()
    t, heap = (int(v[0]) for v in np.nonzero(fo.thr == 0))
    got = mutable(fo)
    got.thr[t, heap] = -got.thr[t, heap]
    assert np.array_equal(got.thr, fo.thr, equal_nan=True)      # what np.array_equal cannot see
    must_fail(got, fo, "thr")


def test_mutation_negative_zero_ordered_before_positive_zero(oracle):
    fo = zero_forest()
    P = fo.proj[0]
    assert ((P == 0) & np.signbit(P)).any() and ((P == 0) & ~np.signbit(P)).any()
    order_keys = np.where((P == 0) & np.signbit(P), -5e-324, P)  # the order of an ordered-integer image
    got = tree_by_recursion(P, order_keys, fo.L, fo.min_leaf)
    with pytest.raises(AssertionError, match="not the split of the stored keys"):
        split_ref.assert_split_of_keys(got, fo.proj[:1], fo.L, fo.min_leaf)


def test_mutation_one_f32_denormal_key_treated_as_zero(oracle):
    fo = oracle_forest(oracle, "cont")
    P = (fo.proj[0] * 1e-40).astype(np.float32)                  # level 0 and below: f32 denormals
    L, ml = fo.L, fo.min_leaf
    ref = split_ref.forest_of_keys(P[None], L, ml)
    tiny = np.finfo(np.float32).tiny
    assert 0 < abs(ref.thr[0, 0]) < tiny
    order_keys = P.copy()
    # the root's extreme key on the far side of zero from the cut, flushed in the compare: it changes sides
    i = int(np.argmax(P[0]) if ref.thr[0, 0] > 0 else np.argmin(P[0]))
    assert 0 < abs(P[0, i]) < tiny and (P[0, i] > ref.thr[0, 0] > 0 or P[0, i] < ref.thr[0, 0] < 0)
    order_keys[0, i] = 0.0
    got = tree_by_recursion(P, order_keys, L, ml)
    with pytest.raises(AssertionError, match="not the split of the stored keys"):
        split_ref.assert_split_of_keys(got, P[None], L, ml, ref)
    split_ref.assert_split_of_keys(tree_by_recursion(P, P, L, ml), P[None], L, ml, ref)


def test_mutation_cut_at_n_plus_1_div_2(oracle):
    fo = oracle_forest(oracle, "cont")
    for level, heap, off, m, keys in last_split_nodes(fo):
        if m % 2 == 1 and m >= 5:
            nh = m // 2 + 1
            got = mutable(fo)
            got.thr[0, heap], got.mglo[0, heap], got.mghi[0, heap] = keys[nh], keys[nh - 1], keys[nh + 1]
            must_fail(got, fo, "thr")
            return
    pytest.fail("no odd node above two leaves")


def test_mutation_ties_broken_by_id_alone(oracle):
    fo = oracle_forest(oracle, "round")
    P = fo.proj[0]
    got = tree_by_recursion(P, P, fo.L, fo.min_leaf, by_id=True)
    with pytest.raises(AssertionError, match="not the split of the stored keys") as e:
        split_ref.assert_split_of_keys(got, fo.proj[:1], fo.L, fo.min_leaf)
    assert "tie" in str(e.value)
    split_ref.assert_split_of_keys(tree_by_recursion(P, P, fo.L, fo.min_leaf), fo.proj[:1], fo.L, fo.min_leaf)
