"""Every forest build against the reference split of its OWN stored keys (tests/split_ref.py).

The forest keeps all its keys (rpt_forest_get_proj, [T][L][N] in the key type), and given the keys
the contract of csrc/split.hip fixes perm, thr, mglo and mghi.  So whatever computed the keys — the
f64 MFMA projection, f32 rows, bf16 rows in any of their projection modes, CSR rows in exact or
tolerance mode — the build is held to an exact reference: perm identical, thr / mglo / mghi
identical bits (signed zeros included), every tree, every node, no tolerance and no flip rate.  What
this does not cover is the accuracy of the keys; that stays with the projection tolerance tests.

Sizes are the smallest at which each path of the split still runs: 131 080 / 131 075 points for the
streamed levels on 16-bit codes (divisible by 8 or not: pcode_kernel for bf16 / CSR rows or no
codes), 262 144 / 300 001 with stream_maxnodes 16 / 32 for csub_kernel, 70 000 with stream_big_node
1000 for the two-stage pick, and 5000 / 4097 / 1023 / 50 below the streamed levels.

The data kinds tie on the device whatever the order of summation: "dups" stores every row 2 to 4
times (equal rows, equal keys at every level: ties run through all earlier levels to the id),
"clump" holds 3000 identical rows, "lattice" is small integers against hyperplanes of 0 / +-1 (exact
in f32 and bf16), "zeros" has columns of +-0.0 and one all-zero hyperplane, "denormal" puts one
level's keys below the key type's smallest normal, "outlier" puts +-3e38 into one f32 column (keys
of +-inf, never NaN: one huge term per sum), "underflow" makes the sums of some rows underflow from
either side of zero on a streamed, a mid-size and a wave level (zeros at the cuts; the kernels give
+0.0 throughout, which every case asserts), "dupcluster" is "dups" with 3000 distinct rows that are
nearly equal in tree 0 alone (csub_kernel hands the node back for one tree while the others have
finished and counted it).  Each case asserts on the downloaded keys that the
data are what they claim."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MIN_LEAF = 40
SWITCHES = ("no_stream", "no_codes", "no_pcodes", "no_csub", "no_wsub", "no_wsort", "no_wpack", "no_wmid",
            "no_midselect")
TIE_KINDS = ("dups", "clump", "lattice", "zeros")


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


@pytest.fixture(scope="module")
def ctx(rp):
    return rp.default_context()


@contextlib.contextmanager
def options(ctx, **kw):
    old = {k: ctx.set_option(k, v) for k, v in kw.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


# --------------------------------------------------------------------------- data
def depth(n):
    """levels until every node holds at most MIN_LEAF points"""
    L = 0
    while n > MIN_LEAF:
        n, L = n - n // 2, L + 1
    return L


def make_rows(kind, rng, n, d, density=None):
    """-> X[n][d] float64.  density: the share of nonzero elements (CSR sources); copies of a row
    share its support."""
    def thin(B):
        return B if density is None else B * (rng.random(B.shape) < density)

    if kind in ("dups", "dupcluster"):
        reps = rng.integers(2, 5, size=n // 2 + 1)              # every base row 2 to 4 times
        idx = np.repeat(np.arange(len(reps)), reps)[:n]
        if n > 1 and idx[-1] != idx[-2]:
            idx[-1] = idx[-2]                                   # (the copy count cut off by n)
        rng.shuffle(idx)
        return thin(rng.standard_normal((len(reps), d)))[idx]
    if kind == "lattice":
        return thin(rng.integers(-3, 4, size=(n, d)).astype(np.float64))
    if kind == "zeros":
        X = np.where(rng.random((n, d)) < 0.5, 0.0, -0.0)
        some = rng.random(n) < 0.2
        X[some] = rng.standard_normal((int(some.sum()), d))
        return X
    X = thin(rng.standard_normal((n, d)))                       # cont, denormal, clump, outlier
    if kind == "clump":
        X[rng.choice(n, 3000, replace=False)] = thin(np.full((1, d), 0.5))
    elif kind == "outlier":
        rows = rng.choice(n, 20, replace=False)
        X[rows, 3] = np.where(rng.random(20) < 0.5, 3e38, -3e38)
    return X


def make_planes(kind, rng, T, L, d):
    if kind == "lattice":
        return rng.integers(-1, 2, size=(T, L, d)).astype(np.float64)
    if kind == "outlier":
        R = rng.standard_normal((T, L, d))                      # the huge column meets every hyperplane
        R[:, 0, 3] = 1.5                                        # ... and overflows at the root: +-inf keys
        return R
    R = rng.standard_normal((T, L, d)) * (rng.random((T, L, d)) < 0.6)
    if kind == "zeros" and L > 2:
        R[:, 2, :] = 0.0                                        # every key of that level is a zero
    return R


def to_csr(X):
    nz = X != 0
    rowptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    return rowptr, np.nonzero(nz)[1].astype(np.int32), X[nz]


# source -> (element type, projection mode, options of the build)
SOURCES = {
    "f64_mfma":         ("f64", "MFMA", {}),
    "f64_exact":        ("f64", "EXACT", {}),
    "f32":              ("f32", "AUTO", {}),
    "bf16":             ("bf16", "AUTO", {}),
    "bf16_terms3":      ("bf16", "AUTO", {"proj_bf16_terms": 3}),
    "bf16_f32":         ("bf16", "AUTO", {"proj_bf16_f32": 1}),
    "bf16_codes":       ("bf16", "AUTO", {"proj_bf16_codes": 1}),
    "csr_f64":          ("csr64", "EXACT", {}),
    "csr_f32":          ("csr32", "EXACT", {}),
    "csr_mfma":         ("csr64", "MFMA", {}),
    "csr_mfma_nodense": ("csr64", "MFMA", {"proj_csr_nodense": 1}),
}


class Case:
    def __init__(self, rp, src, kind, n, d, T, seed):
        self.src, self.kind, self.n, self.d, self.T = src, kind, n, d, T
        self.elem, mode, self.opts = SOURCES[src]
        self.mode = getattr(rp, "RPT_PROJ_" + mode)
        self.L = depth(n)
        rng = np.random.default_rng(seed)
        X = make_rows(kind, rng, n, d, density=0.2 if self.elem.startswith("csr") else None)
        R = make_planes(kind, rng, T, self.L, d)
        if kind == "denormal":
            # products of normal numbers that land below the key type's smallest normal, on level 1
            s = 1e-155 if self.elem == "f64" else 1e-20
            X *= s
            R[:, min(1, self.L - 1), :] *= s
        self.under = [l for l in (1, 7, 10) if l < self.L] or [self.L - 1]
        if kind == "underflow":
            # One row in 200 and the hyperplanes of a streamed, a mid-size and a wave level are scaled so
            # that every product of the two lies below half the smallest denormal of the arithmetic: the
            # sums underflow from either side of zero (IEEE rounding would give -0.0 as often as +0.0;
            # check_claims records what the kernels give).  The other rows' keys are symmetric about 0,
            # so the zeros sit at the cuts.
            s = 1e-200 if self.elem == "f64" else 1e-30
            X[rng.random(n) < max(0.005, 16.0 / n)] *= s
            R[:, self.under, :] *= s
        if kind == "dupcluster":
            # 3000 distinct rows c + t v + noise: v is orthogonal to every hyperplane of tree 0, whose
            # keys of the cluster are nearly equal at every level (one pivot code for more points than a
            # pool holds), and not to those of the other trees, which see ordinary rows there
            v = rng.standard_normal(d)
            q, _ = np.linalg.qr(R[0].T)
            v -= q @ (q.T @ v)
            rows = rng.choice(n, 3000, replace=False)
            X[rows] = (rng.standard_normal(d) + rng.standard_normal((3000, 1)) * v / np.linalg.norm(v)
                       + 1e-7 * rng.standard_normal((3000, d)))
        self.R = R
        if self.elem == "f32":
            X = X.astype(np.float32)
        self.X = X

    def build(self, rp, ctx, **extra):
        with options(ctx, **dict(self.opts, **extra)):
            if self.elem == "bf16":
                ds = rp.Dataset.dense(ctx, rp.to_bf16(self.X.astype(np.float32)), dtype=rp.RPT_BF16)
                f = rp._build(ctx, ds, self.R, self.L, MIN_LEAF, self.mode)
            else:
                src = self.X
                if self.elem.startswith("csr"):
                    rowptr, col, val = to_csr(self.X)
                    src = (rowptr, col, val.astype(np.float32 if self.elem == "csr32" else np.float64), self.d)
                f = rp.forestBatch(0, self.L, MIN_LEAF, self.T, 0, self.d, src, ctx=ctx, hyperplanes=self.R,
                                   mode=self.mode)
            back, bad = C.c_int64(-1), C.c_int64(-1)
            from rptree_amd import _lib
            _lib.check(_lib.lib().rpt_build_last_handed_back(ctx._h, C.byref(back), C.byref(bad)))
        return f, back.value, bad.value


def tied_positions(col):
    """positions of the sorted column whose key equals a neighbour's"""
    s = np.sort(col)
    eq = s[1:] == s[:-1]
    return int((np.concatenate([[False], eq]) | np.concatenate([eq, [False]])).sum())


def check_claims(case, f, P, ref):
    """the data are what the kind says, read off the downloaded keys (fixed by construction)"""
    assert not np.isnan(P).any()
    assert P.dtype == (np.float64 if case.elem in ("f64", "csr64") else np.float32)
    split_levels = sorted({int(r[0]) for r in f.topology() if not r[4]})
    if case.kind in ("dups", "dupcluster"):
        for t in range(case.T):
            for l in split_levels:
                assert tied_positions(P[t, l]) >= case.n // 2, (t, l)
    if case.kind == "clump":
        for t in range(case.T):
            assert tied_positions(P[t, 0]) >= 3000                # the clump is whole at the root
    # tie_nodes counts the cuts that straddle a tie, p'[nh - 1] == p'[nh]: each such node once, also
    # when a wave kernel handed the node back and it was split again (MIN_LEAF > 0: no node of one point)
    straddled = int((ref.mglo == ref.thr).sum())
    assert f.stats()["tie_nodes"] == straddled, (f.stats(), straddled)
    # (at n = 50 there is one cut per tree, and whether it falls on a tie is not fixed by construction:
    # the exact count above covers those cases, 0 included)
    if case.kind in TIE_KINDS and case.n >= 1000:
        assert straddled > 0
    # No projection kernel stores a -0.0 key.  The exact-order kernels add every product to an accumulator
    # that starts at +0.0; the matrix-pipe kernels were measured on the MI355X with sums that underflow
    # from either side ("underflow": f64, f32, bf16 and CSR tolerance mode) and give +0.0 there.  So both
    # zeros meet at a cut only through rpt_split_segments (test_split_segments_matches_partition_at_median);
    # this assertion fails, and says where, as soon as a kernel begins to produce one.
    negz = (P == 0) & np.signbit(P)
    assert not negz.any(), "a -0.0 key at (tree, level, id) %s" % (tuple(int(v[0]) for v in np.nonzero(negz)),)
    if case.kind == "underflow":
        for t in range(case.T):
            for l in case.under:
                assert (P[t, l] == 0).sum() >= 2, (t, l)         # the scaled rows' keys: zeros at the cut
    if case.kind == "outlier":
        assert np.isinf(P).any()
    if case.kind == "denormal":
        tiny = np.finfo(P.dtype).tiny
        assert ((P != 0) & (np.abs(P) < tiny)).any()


def run_case(rp, ctx, oracle, case, **extra):
    f, back, bad = case.build(rp, ctx, **extra)
    assert bad == 0
    P, ref = split_ref.assert_forest_is_split_of_keys(f)
    check_claims(case, f, P, ref)
    print("%s %s n=%d d=%d %s: stats %s, cuts on a tie %d, handed back %d"
          % (case.src, case.kind, case.n, case.d, dict(case.opts, **extra), f.stats(),
             int((ref.mglo == ref.thr).sum()), back))
    if case.src == "f64_exact":        # the whole arrangement once more: exact keys are the oracle's
        fo = oracle.forest_build_dense(case.X, case.R, MIN_LEAF, threads=case.T)
        split_ref.assert_forest_bits_equal(f, fo, "oracle")
    return f, back


# --------------------------------------------------------------------------- streamed levels on codes
STREAMED = [
    # source, kind, n, d
    ("f64_mfma", "cont", 131080, 16), ("f64_mfma", "dups", 131080, 16), ("f64_mfma", "denormal", 131080, 16),
    ("f64_mfma", "zeros", 131075, 16), ("f64_mfma", "lattice", 131075, 16),
    ("f64_exact", "dups", 131080, 16), ("f64_exact", "zeros", 131080, 16), ("f64_exact", "cont", 131075, 16),
    ("f32", "cont", 131080, 16), ("f32", "dups", 131080, 16), ("f32", "clump", 131080, 16),
    ("f32", "lattice", 131080, 16), ("f32", "zeros", 131080, 16), ("f32", "denormal", 131080, 16),
    ("f32", "outlier", 131080, 16), ("f32", "dups", 131075, 16), ("f32", "lattice", 131075, 16),
    ("bf16", "lattice", 131080, 64), ("bf16", "dups", 131080, 72), ("bf16", "dups", 131080, 264),
    ("bf16", "dups", 131075, 64), ("bf16", "cont", 131080, 64),
    ("bf16_terms3", "dups", 131080, 64), ("bf16_terms3", "lattice", 131080, 72),
    ("bf16_f32", "cont", 131080, 72), ("bf16_f32", "dups", 131080, 64),
    ("bf16_codes", "lattice", 131080, 64), ("bf16_codes", "dups", 131080, 72), ("bf16_codes", "clump", 131080, 264),
    ("csr_f64", "dups", 131080, 64), ("csr_f64", "cont", 131075, 64),
    ("csr_f32", "lattice", 131080, 64), ("csr_f32", "dups", 131080, 64),
    ("csr_mfma", "dups", 131080, 64), ("csr_mfma", "lattice", 131080, 64), ("csr_mfma", "cont", 131075, 64),
    ("csr_mfma_nodense", "dups", 131080, 64), ("csr_mfma_nodense", "lattice", 131080, 64),
    ("f64_mfma", "underflow", 131080, 16), ("f32", "underflow", 131080, 16), ("f32", "underflow", 131075, 16),
    ("bf16", "underflow", 131080, 64), ("csr_mfma", "underflow", 131080, 64),
]


@pytest.mark.parametrize("src,kind,n,d", STREAMED, ids=["-".join(map(str, c)) for c in STREAMED])
def test_streamed_levels(rp, ctx, oracle, src, kind, n, d):
    run_case(rp, ctx, oracle, Case(rp, src, kind, n, d, 2, seed=n + d))


# --------------------------------------------------------------------------- csub_kernel
CSUB = [
    ("f32", "cont", 262144, 16, 16), ("f32", "clump", 300001, 16, 32), ("f32", "dups", 300001, 16, 32),
    ("f64_mfma", "dups", 262144, 16, 16), ("f64_mfma", "clump", 300001, 16, 32),
    ("bf16", "lattice", 262144, 64, 16), ("bf16_codes", "clump", 300001, 64, 32),
    ("csr_mfma", "dups", 262144, 64, 16),
    # both zeros as keys of a level that csub_kernel splits (level 7)
    ("f64_mfma", "underflow", 300001, 16, 32), ("f32", "underflow", 262144, 16, 16),
    ("csr_mfma", "underflow", 262144, 64, 16),
    # a node handed back by ONE tree's block while the other trees' blocks finished it, cuts on ties included
    ("f64_mfma", "dupcluster", 300001, 16, 32), ("f32", "dupcluster", 300001, 16, 32),
]


@pytest.mark.parametrize("src,kind,n,d,maxnodes", CSUB, ids=["-".join(map(str, c)) for c in CSUB])
def test_mid_size_nodes_on_packed_codes(rp, ctx, oracle, src, kind, n, d, maxnodes):
    """stream_maxnodes caps the streamed levels: nodes of 4687 / 8192 points reach csub_kernel; a clump
    of 3000 equal keys overflows its pool and the node is handed back"""
    f, back = run_case(rp, ctx, oracle, Case(rp, src, kind, n, d, 2, seed=n + maxnodes), stream_maxnodes=maxnodes)
    if kind in ("clump", "dupcluster"):
        assert back > 0


# --------------------------------------------------------------------------- two-stage pick
BIG = [("f32", "dups"), ("f32", "lattice"), ("f64_mfma", "cont"), ("f64_mfma", "dups"), ("bf16", "lattice"),
       ("csr_f32", "dups")]


@pytest.mark.parametrize("src,kind", BIG, ids=["-".join(c) for c in BIG])
def test_two_stage_pick(rp, ctx, oracle, src, kind):
    d = 16 if src in ("f32", "f64_mfma") else 64
    run_case(rp, ctx, oracle, Case(rp, src, kind, 70000, d, 3, seed=7), stream_big_node=1000)


# --------------------------------------------------------------------------- below the streamed levels
SMALL = [("f64_mfma", "dups", 16), ("f64_mfma", "zeros", 16), ("f64_exact", "lattice", 16), ("f32", "dups", 16),
         ("f32", "lattice", 16), ("f32", "denormal", 16), ("f32", "outlier", 16), ("bf16", "dups", 64),
         ("bf16_terms3", "lattice", 72), ("bf16_f32", "dups", 72), ("csr_f64", "dups", 64), ("csr_f32", "lattice", 64),
         ("csr_mfma", "dups", 64), ("f64_mfma", "underflow", 16), ("f32", "underflow", 16)]


@pytest.mark.parametrize("no_stream", [0, 1])
@pytest.mark.parametrize("n", [5000, 4097, 1023, 50])
@pytest.mark.parametrize("src,kind,d", SMALL, ids=["-".join(map(str, c)) for c in SMALL])
def test_below_the_streamed_levels(rp, ctx, oracle, src, kind, d, n, no_stream):
    run_case(rp, ctx, oracle, Case(rp, src, kind, n, d, 3, seed=n), no_stream=no_stream)


# --------------------------------------------------------------------------- fallback switches
_default = {}


def default_build(rp, ctx, oracle, src, kind, d):
    """the default build of the switch cases and the one reference computed for it"""
    if (src, kind) not in _default:
        case = Case(rp, src, kind, 131080, d, 2, seed=99)
        f, back, bad = case.build(rp, ctx)
        P, ref = split_ref.assert_forest_is_split_of_keys(f)
        check_claims(case, f, P, ref)
        _default[src, kind] = (case, P, ref)
        f.close()
    return _default[src, kind]


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("src,kind,d", [("f32", "dups", 16), ("bf16", "lattice", 64)], ids=["f32-dups", "bf16-lattice"])
def test_fallback_switches(rp, ctx, oracle, src, kind, d, switch):
    """The switches do not touch the projection: the keys are the default build's bit for bit, and the
    forest is the one reference computed for the default build."""
    case, P, ref = default_build(rp, ctx, oracle, src, kind, d)
    f, back, bad = case.build(rp, ctx, **{switch: 1})
    assert bad == 0
    Q = f.proj()
    assert Q.dtype == P.dtype and np.array_equal(Q.view(np.int32), P.view(np.int32))
    split_ref.assert_forest_is_split_of_keys(f, P, ref)
    assert f.stats()["tie_nodes"] == int((ref.mglo == ref.thr).sum())      # on every path the same count
    print("%s %s %s=1: stats %s, cuts on a tie %d, handed back %d"
          % (src, kind, switch, f.stats(), int((ref.mglo == ref.thr).sum()), back))
