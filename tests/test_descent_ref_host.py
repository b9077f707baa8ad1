"""tests/descent_ref.py pinned to the oracle where the oracle's keys ARE the keys (no GPU).

With keys from oracle.inner_sd / inner_ss (the f64 innerSD / innerSS the oracle itself descends on)
the reference descent must list the ids of oracle.candidates_dense / candidates_sparse, of
stream_candidates_dense over an explicit topology, and the priorities and buckets of
candidates_h_dense / knn_h_dense: every query, every tree.  The inputs must reach the edges they
claim (asserted from the reference's trace), and every one-token mutant of the reference must change
at least one candidate list of these fixed inputs: the proof that they can see a subtly wrong kernel."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descent_ref as dr  # noqa: E402

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def keys_dense(oracle, R, q):
    """K[T][L]: the oracle's own key of q at every hyperplane (innerSD over R's nonzeros)"""
    T, L, _ = R.shape
    K = np.empty((T, L))
    for t in range(T):
        for l in range(L):
            idx = np.nonzero(R[t, l])[0]
            K[t, l] = oracle.inner_sd(idx, R[t, l, idx], q)
    return K


def keys_sparse(oracle, R, qi, qv):
    T, L, _ = R.shape
    K = np.empty((T, L))
    for t in range(T):
        for l in range(L):
            idx = np.nonzero(R[t, l])[0]
            K[t, l] = oracle.inner_ss(idx, R[t, l, idx], qi, qv)
    return K


class Dense:
    """an oracle forest over dense rows, query batches by kind, and the oracle's keys of every query"""

    def __init__(self, oracle, name, X, R, min_leaf, batches):
        self.name, self.X, self.R, self.min_leaf = name, X, R, min_leaf
        self.N, self.L = len(X), R.shape[1]
        self.f = oracle.forest_build_dense(X, R, min_leaf, threads=4)
        self.batches = batches                                          # {kind: Q}
        self.keys = {kind: [keys_dense(oracle, R, q) for q in Q] for kind, Q in batches.items()}

    def ranges(self, mod, kind, trace=None):
        f = self.f
        return [mod.candidates_of_keys(K, f.thr, f.mglo, f.mghi, self.N, self.L, self.min_leaf, trace=trace)
                for K in self.keys[kind]]


def generated(oracle, name, lattice, n, d, T, min_leaf, kinds, nq, L=None):
    rng = np.random.default_rng([n, d, T, min_leaf])
    L = L or dr.depth(n, min_leaf)
    if lattice:
        X, R = dr.lattice_rows(rng, n, d), dr.lattice_planes(rng, T, L, d)
    else:
        X = rng.standard_normal((n, d))
        R = rng.standard_normal((T, L, d)) * (rng.random((T, L, d)) < 0.6)
    return Dense(oracle, name, X, R, min_leaf, {k: dr.make_queries(k, rng, X, nq) for k in kinds})


ALL_KINDS = ("fresh", "gap", "stored", "mid", "x8", "nan", "inf")
_cases = {}


def cases(oracle):
    if not _cases:
        g = np.load(os.path.join(G, "forest_dense_1000x16.npz"))
        _cases["golden"] = Dense(oracle, "golden", g["X"], g["R"], int(g["min_leaf"]), {"golden": g["Q"]})
        _cases["lattice"] = generated(oracle, "lattice", True, 5000, 16, 3, 40, ("fresh", "gap", "stored"), 64)
        _cases["deep_lattice"] = generated(oracle, "deep_lattice", True, 1023, 16, 5, 1, ALL_KINDS, 32)
        _cases["deep_cont"] = generated(oracle, "deep_cont", False, 1023, 16, 5, 1, ALL_KINDS + ("near", "mixed"), 32)
        # 320 -> 160 -> 80 -> 40 points: nodes of exactly min_leaf points above the last level
        _cases["shallow"] = generated(oracle, "shallow", True, 320, 16, 3, 40, ("fresh", "gap", "mid"), 32, L=5)
    return _cases


# ------------------------------------------------------------------ the batch topology
def test_candidates_equal_the_oracle_every_query_every_tree(oracle):
    pairs = 0
    for c in cases(oracle).values():
        for kind, Q in c.batches.items():
            for q, rg in zip(Q, c.ranges(dr, kind)):
                ids = dr.ids_of_ranges(c.f.perm, rg)
                for t in range(c.f.T):
                    assert np.array_equal(ids[t], oracle.candidates_dense(c.f, q, t)), (c.name, kind, t)
                    pairs += 1
    print("%d (query, tree) pairs, 0 mismatches" % pairs)
    assert pairs >= 1664


def test_golden_candidate_list(oracle):
    """the committed candidate list of the golden forest, offsets and ids"""
    g = np.load(os.path.join(G, "forest_dense_1000x16.npz"))
    c = cases(oracle)["golden"]
    flat = [ids for rg in c.ranges(dr, "golden") for ids in dr.ids_of_ranges(c.f.perm, rg)]
    assert np.array_equal(np.concatenate([[0], np.cumsum([len(i) for i in flat])]), g["cand_off"])
    assert np.array_equal(np.concatenate(flat), g["cand_ids"])


def test_sparse_rows_equal_the_oracle(oracle):
    """the golden CSR forest, its own rows and perturbed rows as SVector queries (keys from innerSS)"""
    g = np.load(os.path.join(G, "forest_sparse_600x12.npz"))
    N, L, ml, R = int(g["n"]), int(g["L"]), int(g["min_leaf"]), g["R"]
    f = oracle.Forest(N, int(g["d"]), R, L, ml, g["perm"], g["thr"], g["mglo"], g["mghi"])
    rowptr, col, val = g["rowptr"], g["col"], g["val"]
    rng = np.random.default_rng(3)
    tr = dr.Trace()
    for i in rng.integers(0, N, 48):
        a, b = rowptr[i], rowptr[i + 1]
        for qv in (val[a:b], val[a:b] * 1.01 + 0.01, val[a:b] * 8.0):
            rg = dr.candidates_of_keys(keys_sparse(oracle, R, col[a:b], qv), f.thr, f.mglo, f.mghi, N, L, ml, trace=tr)
            ids = dr.ids_of_ranges(f.perm, rg)
            for t in range(f.T):
                assert np.array_equal(ids[t], oracle.candidates_sparse(f, col[a:b], qv, t)), (i, t)
    assert tr.key_eq_thr > 0                                            # (rows that store none of a hyperplane's indices)


# ------------------------------------------------------------------ the inputs hit what they claim
def test_trace_floors(oracle):
    cs = cases(oracle)
    tr = dr.Trace()
    cs["lattice"].ranges(dr, "fresh", trace=tr)
    print("lattice rows, fresh lattice queries:", tr)
    assert tr.key_eq_thr >= 20 and tr.dl_eq_dr >= 1000
    for name, kind in (("deep_cont", "mid"), ("deep_lattice", "gap")):
        tr = dr.Trace()
        nr = np.array([len(tree) for rg in cs[name].ranges(dr, kind, trace=tr) for tree in rg])
        print("%s, %s queries: %.2f of the (query, tree) pairs reach >= 2 ranges, %.2f >= 3; %s"
              % (name, kind, (nr >= 2).mean(), (nr >= 3).mean(), tr))
        assert (nr >= 2).mean() >= 0.25 and (nr >= 3).sum() >= 5 and tr.both >= 40
    for kind, field in (("nan", "nan_keys"), ("inf", "inf_keys")):
        tr = dr.Trace()
        cs["deep_cont"].ranges(dr, kind, trace=tr)
        assert getattr(tr, field) >= 100, tr
    tr = dr.Trace()
    cs["deep_lattice"].ranges(dr, "inf", trace=tr)
    assert tr.inf_keys >= 100 and tr.dl_eq_dr >= 100                    # inf - finite on both sides: dl == dr


# ------------------------------------------------------------------ an explicit topology
@pytest.mark.parametrize("n,chunk,min_leaf", [(1000, 128, 20), (777, 100, 5), (600, 600, 30)])
def test_streamed_forest_equals_the_oracle(oracle, n, chunk, min_leaf):
    rng = np.random.default_rng(n)
    d, T = 12, 3
    L = dr.depth(n, min_leaf)
    X = rng.standard_normal((n, d))
    R = rng.standard_normal((T, L, d)) * (rng.random((T, L, d)) < 0.6)
    sf = oracle.stream_forest_dense(X, R, min_leaf, chunk)
    tr, reached = dr.Trace(), 0
    for kind in ("mid", "near", "fresh", "nan"):
        for q in dr.make_queries(kind, rng, X, 24):
            K = keys_dense(oracle, R, q)
            rg = dr.candidates_of_keys_x(K, sf.thr, sf.mglo, sf.mghi, sf.kind, sf.leaf_off, sf.leaf_len, trace=tr)
            for t in range(T):
                ids = dr.ids_of_ranges(sf.leaf_ids, rg)[t]
                assert np.array_equal(ids, oracle.stream_candidates_dense(sf, R, q, t)), (kind, t)
                reached += len(rg[t])
    assert tr.both > 0 and reached > 0


# ------------------------------------------------------------------ priorities and knnH
def test_priorities_and_knn_h_equal_the_oracle(oracle):
    for name in ("golden", "deep_cont", "lattice"):
        c = cases(oracle)[name]
        f = c.f
        for kind in [k for k in c.batches if k in ("golden", "mid", "near", "gap", "fresh")]:
            for q, K in zip(c.batches[kind], c.keys[kind]):
                rh = dr.candidates_h_of_keys(K, f.thr, f.mglo, f.mghi, c.N, c.L, c.min_leaf)
                for t in range(f.T):
                    prio, off, ln = oracle.candidates_h_dense(f, q, t)
                    assert [r[0] for r in rh[t]] == off.tolist() and [r[1] for r in rh[t]] == ln.tolist()
                    assert np.array_equal(np.array([r[2] for r in rh[t]]).view(np.int64), prio.view(np.int64))
                for k in (1, 10, 100):
                    ids, _ = oracle.knn_h_dense(f, c.X, q, k)
                    assert np.array_equal(dr.knn_h_ids(f.perm, rh, k), ids), (name, kind, k)


# ------------------------------------------------------------------ mutants
MUTANTS = {
    # name: [(text of descent_ref.py, its replacement)]
    "threshold <= (the side)": [("left = proj < th", "left = proj <= th")],
    "threshold <= (the both rule)": [("(proj < th and dl > dr)", "(proj <= th and dl > dr)")],
    "threshold >= (the both rule)": [("(proj > th and dl < dr)", "(proj >= th and dl < dr)")],
    "left margin >=": [("and dl > dr)", "and dl >= dr)")],
    "right margin <=": [("and dl < dr)", "and dl <= dr)")],
    "dl / dr swapped": [("dl = abs(lo - proj)", "dl = abs(hi - proj)"), ("dr = abs(hi - proj)", "dr = abs(lo - proj)")],
    "n - n // 2 to the left child": [("nh = n // 2", "nh = n - n // 2")],
    "Tip test n < min_leaf": [("n <= min_leaf", "n < min_leaf")],
}


def mutant_module(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "descent_ref.py")
    with open(path) as fh:
        src = fh.read()
    for old, new in MUTANTS[name]:
        code = src.split('"""', 2)[2]                                   # (the docstring restates the rules)
        assert code.count(old) == 1, (name, old, code.count(old))
        src = src.replace(old, new)
    mod = types.ModuleType("descent_ref_mutant")
    exec(compile(src, path, "exec"), mod.__dict__)
    return mod


def test_the_unmutated_source_is_the_module():
    spec = importlib.util.find_spec("descent_ref")
    assert os.path.samefile(spec.origin, os.path.join(os.path.dirname(os.path.abspath(__file__)), "descent_ref.py"))


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_changes_a_candidate_list(oracle, name):
    mod = mutant_module(name)
    changed = 0
    for c in cases(oracle).values():
        for kind in c.batches:
            changed += sum(a != b for a, b in zip(c.ranges(dr, kind), c.ranges(mod, kind)))
    print("mutant %r: caught, %d candidate lists change" % (name, changed))
    assert changed > 0, "mutant %r goes unnoticed: the inputs are too tame" % name
