"""CPU proof that tests/knn_f32_ref.py, the reference tests/test_gpu_knn_f32_l2.py compares the device
with, is right (no GPU):

  * its selection rules equal the oracle's, ids and distance bits, under all three duplicate rules;
  * `check_interval` accepts honest f32 arithmetic (two summation orders simulated in numpy float32)
    on every input family, so the bound it holds the kernels to is satisfiable, and rejects each of
    six ways of being subtly wrong;
  * on the lattice rows f32 arithmetic is exact: the precondition of the bit-exact device tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_f32_ref as ref  # noqa: E402
import knn_l2_cut_ref as f64ref  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RULES = (ref.KEEP, ref.DEDUP, ref.DEDUP_DISTANCE)

# (n, d, T, minLeaf) of the host forests: the row lengths of the device shapes on fewer rows
HOST_SHAPES = [(1500, 16, 6, 60), (1200, 37, 4, 50), (900, 208, 3, 100), (600, 1040, 3, 100), (700, 8, 3, 400)]
HOST_NQ = 12


def forest_and_candidates(oracle, X, Q, T, min_leaf, seed=9):
    """an oracle forest over the rows X (float32 rows are widened exactly) and, per query, its
    candidate list in candidate order: tree ascending, then leaf order"""
    n, d = X.shape
    L, _, pnz = oracle.tree_cfg(min_leaf, n, d)
    R, _ = oracle.forest_hyperplanes(seed, T, L, pnz, d)
    fo = oracle.forest_build_dense(X, R, min_leaf)
    cands = [np.concatenate([oracle.candidates_dense(fo, q, t) for t in range(T)]) for q in Q]
    return fo, cands


# ------------------------------------------------------------------ the restatement equals the oracle
def lattice_golden():
    g = np.load(os.path.join(G, "forest_dense_1000x16.npz"))
    X = np.clip(np.round(2.0 * g["X"]) / 2.0, -ref.LATTICE_M, ref.LATTICE_M)
    Q = np.vstack([X[:4], np.clip(np.round(2.0 * g["Q"][:6]) / 2.0, -ref.LATTICE_M, ref.LATTICE_M)])
    return X, Q, g["R"], int(g["min_leaf"])


def continuous_f64(oracle):
    n, d, T, min_leaf = 800, 24, 5, 40
    X = oracle.data_normal_dense2(31, n, d)
    L, _, pnz = oracle.tree_cfg(min_leaf, n, d)
    R, _ = oracle.forest_hyperplanes(32, T, L, pnz, d)
    return X, np.vstack([X[:3], X[3:9] + 0.003]), R, min_leaf


@pytest.mark.parametrize("rows", ["lattice", "continuous"])
def test_selection_rules_equal_the_oracle(oracle, rows):
    """knn_from_candidates over the oracle's candidate lists == oracle.knn_dense and the rule of
    brute_from_rows == the oracle's brute force, ids, distance bits and counts.  Lattice rows: the
    distances are exact_dist (sums of quarters: every summation order gives the same bits).
    Continuous f64 rows: the distances are metricDDL2's left fold (knn_l2_cut_ref.fold_l2, which
    tests/test_knn_l2_cut_host.py pins to the oracle and which is pinned again here), since the
    order of an f64 sum shows in its last bits; the rules are the same code."""
    X, Q, R, min_leaf = lattice_golden() if rows == "lattice" else continuous_f64(oracle)
    n, T = len(X), R.shape[0]
    fo = oracle.forest_build_dense(X, R, min_leaf)
    dist = ref.exact_dist if rows == "lattice" else f64ref.fold_l2
    ties = 0
    for q in Q:
        cands = np.concatenate([oracle.candidates_dense(fo, q, t) for t in range(T)])
        D = dist(X[cands], q)
        assert ref.same_bits(D, [oracle.metric_dd(X[c], q) for c in cands])
        ties += len(D) - len(np.unique(D))
        for rule in RULES:
            for k in (1, 10, 50, len(cands) + 7):
                wi, wd = oracle.knn_dense(fo, X, q, k, dedup=rule)
                gi, gd, cnt = ref.knn_from_candidates(cands, D, k, rule)
                assert cnt == len(wi) and np.array_equal(gi[:cnt], wi) and ref.same_bits(gd[:cnt], wd), (rule, k)
                assert np.all(gi[cnt:] == -1) and np.all(np.isposinf(gd[cnt:]))
        Dall = dist(X, q)
        for k in (1, 10, 50, n + 7):
            wi, wd = oracle.brute_knn_dense(X, q, k)
            if rows == "lattice":
                gi, gd, cnt = ref.brute_from_rows(X, q, k)
            else:
                gi, gd, cnt = ref.knn_from_candidates(np.arange(n), Dall, k, ref.KEEP)
            assert cnt == len(wi) and np.array_equal(gi[:cnt], wi) and ref.same_bits(gd[:cnt], wd), k
    assert ties > 10 * len(Q)                # (copies across trees; on the lattice different rows too)


def test_rules_on_a_hand_made_list():
    cands = np.array([7, 3, 7, 5, 3, 9])
    D = np.array([2.0, 1.0, 2.0, 2.0, 1.0, 0.5])
    assert ref.knn_from_candidates(cands, D, 4, ref.KEEP)[0].tolist() == [9, 3, 3, 7]
    assert ref.knn_from_candidates(cands, D, 6, ref.DEDUP)[0].tolist() == [9, 3, 7, 5, -1, -1]
    i, v, c = ref.knn_from_candidates(cands, D, 4, ref.DEDUP_DISTANCE)
    assert i.tolist() == [9, 3, 7, -1] and v.tolist() == [0.5, 1.0, 2.0, np.inf] and c == 3
    assert ref.voted(cands, 2).tolist() == [3, 7]
    # KEEP order 9 3 3 7 7 5: the checker takes it, and refuses 5 in front of the second 7
    ok = ref.knn_from_candidates(cands, D, 6, ref.KEEP)
    assert ref.interval_violation(cands, D, *ok, 6, ref.KEEP, 4) is None
    bad = ok[0].copy()
    bad[4], bad[5] = 5, 7
    assert "candidate order" in ref.interval_violation(cands, D, bad, ok[1], ok[2], 6, ref.KEEP, 4)


# ------------------------------------------------------------------ exactness on the lattice
def all_device_shapes():
    return sorted(set((d, "f32") for _, d, _, _ in ref.SHAPES_F32) | set((d, "bf16") for _, d, _, _ in ref.SHAPES_BF16)
                  | set((d, t) for _, d in ref.BRUTE_SHAPES for t in ("f32", "bf16")))


def test_lattice_arithmetic_is_exact_in_f32():
    """d (2 M)^2 4 < 2^24 for every row length the device tests use, and both simulated f32 kernels
    return exact_dist bit for bit, also on the rows scaled by 2^40 and 2^-40 (f32)"""
    for d, dtype in all_device_shapes():
        assert ref.lattice_is_exact(d), d
        X, Q = ref.lattice_set(300, d, dtype, seed=1, nq=9)
        assert np.array_equal(ref.as_dtype(X, "bf16"), X)            # the lattice is exact in bf16
        for s in (1.0,) if dtype == "bf16" else (1.0, 2.0 ** 40, 2.0 ** -40):
            Xs, Qs = (X * np.float32(s)), (Q * np.float32(s))
            for q, q1 in zip(Qs, Q):
                D = ref.exact_dist(Xs, q)
                assert ref.same_bits(D, ref.exact_dist(X, q1) * s)   # scaled exactly
                for name, sq in ref.SIMS.items():
                    assert ref.same_bits(np.sqrt(sq(Xs, q).astype(np.float64)), D), (d, dtype, s, name)
    assert not ref.lattice_is_exact(4096 * 4)                        # (the bound is not vacuous)


# ------------------------------------------------------------------ the interval check has teeth
_sets = {}


def host_set(oracle, kind, shape, dtype):
    key = (kind, shape, dtype)
    if key not in _sets:
        n, d, T, min_leaf = shape
        X, Q = ref.family_set(kind, n, d, dtype, seed=3, nq=HOST_NQ)
        _, cands = forest_and_candidates(oracle, X, Q.astype(np.float64), T, min_leaf)
        D = [ref.exact_dist(X[c], q) for c, q in zip(cands, Q)]
        _sets[key] = (X, Q, cands, D)
    return _sets[key]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ref.FAMILIES)
def test_honest_f32_arithmetic_passes_the_interval_check(oracle, kind, dtype, record_property):
    """both summation orders, every host shape, every query, k and rule: accepted.  The largest
    |dist - D| / ((d + 2) 2^-24 D + sqrt(d) 4e-23) seen is printed (DESIGN 4.3 quotes it): measured
    against the f64 reference, not against a device."""
    worst = 0.0
    for shape in HOST_SHAPES:
        d = shape[1]
        X, Q, cands, D = host_set(oracle, kind, shape, dtype)
        for name, sq in ref.SIMS.items():
            for i, q in enumerate(Q):
                val = np.sqrt(sq(X[cands[i]], q).astype(np.float64))
                for rule in (ref.KEEP, ref.DEDUP):
                    rk = ref.ranked(cands[i], val, rule)
                    for k in ref.KS + (len(cands[i]) + 3,):
                        ans = ref.padded(*rk, k)
                        why = ref.interval_violation(cands[i], D[i], *ans, k, rule, d)
                        assert why is None, (kind, dtype, shape, name, i, rule, k, why)
                worst = max(worst, ref.worst_ratio(cands[i], D[i], *ref.padded(*rk, len(rk[0])), d))
        if kind == "self":                    # a stored row is at distance exactly 0 from itself
            assert all(np.sqrt(sq(X[c], q).astype(np.float64)).min() == 0.0
                       for c, q in zip(cands, Q) for sq in ref.SIMS.values())
    print("worst |dist - D| / bound, %s %s: %.3f" % (kind, dtype, worst))
    record_property("worst_ratio", worst)
    assert 0.0 <= worst < 1.0


def honest(oracle, kind="cont", shape=HOST_SHAPES[0], dtype="f32", k=10, rule=ref.KEEP, i=3, sq=ref.sim_fold):
    X, Q, cands, D = host_set(oracle, kind, shape, dtype)
    ids, dist, cnt = ref.sim_knn(cands[i], X[cands[i]], Q[i], k, rule, sq)
    assert ref.interval_violation(cands[i], D[i], ids, dist, cnt, k, rule, shape[1]) is None
    return X, Q[i], cands[i], D[i], ids, dist, cnt


def rejected(cands, D, ids, dist, cnt, k, rule, d):
    why = ref.interval_violation(cands, D, ids, dist, cnt, k, rule, d)
    with pytest.raises(AssertionError):
        ref.check_interval(cands, D, ids, dist, cnt, k, rule, d)
    return why


@pytest.mark.parametrize("rule", [ref.KEEP, ref.DEDUP])
def test_mutation_a_a_neighbour_replaced_by_a_farther_one(oracle, rule):
    """the true (k-1)-th neighbour is missing and the (k+3)-th stands at the end in its place: a
    sorted list of true distances of true candidates, wrong only in WHICH ones"""
    k, d = 10, HOST_SHAPES[0][1]
    X, q, cands, D, ids, dist, cnt = honest(oracle, k=k, rule=rule)
    fi, fd, _ = ref.sim_knn(cands, X[cands], q, k + 3, rule)
    assert fd[k + 2] > fd[k - 2] * (1 + 1e-3)
    ids2 = np.concatenate([ids[:k - 2], ids[k - 1:], fi[k + 2:]])
    dist2 = np.concatenate([dist[:k - 2], dist[k - 1:], fd[k + 2:]])
    assert "belongs before" in rejected(cands, D, ids2, dist2, cnt, k, rule, d)


def test_mutation_b_a_duplicate_copy_dropped(oracle):
    """duplicates kept, the query is a stored row found by all 6 trees: one of its copies is left
    out and the (k+1)-th entry moves up"""
    k, shape = 10, HOST_SHAPES[0]
    X, q, cands, D, ids, dist, cnt = honest(oracle, kind="self", k=k)
    assert (dist == 0).sum() >= 2 and len(set(ids[dist == 0].tolist())) == 1
    fi, fd, _ = ref.sim_knn(cands, X[cands], q, k + 1, ref.KEEP)
    why = rejected(cands, D, fi[1:], fd[1:], cnt, k, ref.KEEP, shape[1])
    assert "belongs before" in why


def test_mutation_c_two_entries_swapped(oracle):
    k, d = 10, HOST_SHAPES[0][1]
    _, _, cands, D, ids, dist, cnt = honest(oracle, k=k)
    assert dist[4] != dist[6]
    ids2, dist2 = ids.copy(), dist.copy()
    ids2[[4, 6]], dist2[[4, 6]] = ids[[6, 4]], dist[[6, 4]]
    assert "decrease" in rejected(cands, D, ids2, dist2, cnt, k, ref.KEEP, d)
    # ... and the ids alone, each under the other's distance
    assert "distance" in rejected(cands, D, ids2, dist, cnt, k, ref.KEEP, d)


def test_mutation_d_norm_expansion_on_offset_rows(oracle, dtype="f32"):
    """|x|^2 + |q|^2 - 2 x.q in f32 on rows near 1000: the squares are ten thousand million times the
    squared distance and their rounding swamps it.  (The bf16 offset rows, quarters near 64, are a
    lattice on which even the expansion is exact at d = 16: they attack the selection with ties,
    not the arithmetic.)"""
    k, shape = 10, HOST_SHAPES[0]
    bad = 0
    X, Q, cands, D = host_set(oracle, "offset", shape, dtype)
    for i in range(len(Q)):
        ans = ref.sim_knn(cands[i], X[cands[i]], Q[i], k, ref.KEEP, ref.sim_expansion)
        bad += ref.interval_violation(cands[i], D[i], *ans, k, ref.KEEP, shape[1]) is not None
        assert ref.interval_violation(cands[i], D[i], *ref.sim_knn(cands[i], X[cands[i]], Q[i], k, ref.KEEP),
                                      k, ref.KEEP, shape[1]) is None
    assert bad == len(Q), bad


@pytest.mark.parametrize("shape", [HOST_SHAPES[0], HOST_SHAPES[2]])
def test_mutation_e_the_last_elements_of_a_row_left_out(oracle, shape):
    """the last 4 elements (the last 16-byte piece of an f32 row) never reach the sum"""
    k, d = 10, shape[1]
    X, Q, cands, D = host_set(oracle, "cont", shape, "f32")
    bad = 0
    for i in range(len(Q)):
        ans = ref.knn_from_candidates(cands[i], np.sqrt(ref.sim_fold(X[cands[i]][:, :d - 4], Q[i][:d - 4])
                                                        .astype(np.float64)), k, ref.KEEP)
        bad += ref.interval_violation(cands[i], D[i], *ans, k, ref.KEEP, d) is not None
    assert bad == len(Q), bad


def test_mutation_f_count_one_short(oracle):
    k, d = 10, HOST_SHAPES[0][1]
    _, _, cands, D, ids, dist, cnt = honest(oracle, k=k)
    ids2, dist2 = ids.copy(), dist.copy()
    ids2[-1], dist2[-1] = -1, np.inf
    assert "count" in rejected(cands, D, ids2, dist2, cnt - 1, k, ref.KEEP, d)
    # more entries asked for than there are: the count is the number of entries the rule admits
    X, q = honest(oracle, k=k)[:2]
    kk = len(cands) + 5
    full = ref.sim_knn(cands, X[cands], q, kk, ref.DEDUP)
    assert full[2] == len(np.unique(cands))
    assert ref.interval_violation(cands, D, *full, kk, ref.DEDUP, d) is None
    assert "count" in rejected(cands, D, full[0], full[1], full[2] - 1, kk, ref.DEDUP, d)
