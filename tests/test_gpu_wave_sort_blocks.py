"""The sorting wave kernel (csrc/split.hip, wsort_kernel) keeps every node of depth d in an aligned
block of 1024 >> d positions, padded below and above its points so that the cut falls on the middle
of the block, and sorts only inside the blocks.  Every case here builds a small forest whose wave
kernel meets the node sizes and ties at which that padding rule can go wrong, and compares it, bit
for bit, with the oracle and with the same build under no_wsort = 1 (the histogram-select wave
kernel), with packed images (default) and without (no_wpack = 1).

The cases are checked on the CPU first (test_cases_are_what_they_claim, no GPU): the sizes of the
wave kernel's top nodes and of their descendants follow from N by the halving rule
(Internal.hs:495,503), the tie counts from the key columns."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref  # noqa: E402

K_CAP = 1024     # points a wave holds (kWCap)
K_LEVELS = 5     # levels per launch (kWRmax)
K_POOL = 128     # tied positions per level a wave orders exactly (kSPool)


# --------------------------------------------------------------------------- shapes
def wave_tops(n, L, ml, level=0):
    """(level, size) of the nodes the wave kernel starts from: the first split nodes of at most
    K_CAP points on every path from the root"""
    if level >= L or n <= ml:
        return []
    if n <= K_CAP:
        return [(level, n)]
    return wave_tops(n // 2, L, ml, level + 1) + wave_tops(n - n // 2, L, ml, level + 1)


def split_depth(n, level, L, ml):
    """levels a node goes on splitting for"""
    if level >= L or n <= ml:
        return 0
    return 1 + max(split_depth(n // 2, level + 1, L, ml), split_depth(n - n // 2, level + 1, L, ml))


def sizes_at(n, depth):
    out = [n]
    for _ in range(depth):
        out = [m for v in out for m in (v // 2, v - v // 2)]
    return out


# name: N, T, L, min_leaf, dtype, no_stream, data kind
SHAPES = {
    # three wave levels and N * T >= 65 536: the packed-image instantiation
    "n1024_pk":    (1024, 64, 3, 1, "f64", 1, "cont"),
    "n1023_pk":    (1023, 65, 3, 1, "f64", 1, "cont"),
    "n513_pk":     (513, 128, 3, 1, "f64", 1, "cont"),
    "n512_pk":     (512, 128, 3, 1, "f32", 1, "grid"),
    "n65536_pk":   (65536, 2, 9, 128, "f64", 0, "cont"),      # six streamed levels, then 1024 -> 128
    "n1023_f32":   (1023, 65, 3, 1, "f32", 1, "grid"),
    # all five levels of a launch, nodes left active for a second one
    "n1024_deep":  (1024, 4, 8, 1, "f64", 1, "cont"),
    "n1023_deep":  (1023, 4, 7, 2, "f32", 1, "grid"),         # children differ by one at every depth
    "n683_deep":   (683, 8, 6, 2, "f64", 1, "cont"),
    "n50":         (50, 4, 4, 3, "f64", 1, "cont"),
    "n50_pairs":   (50, 4, 8, 1, "f64", 1, "cont"),           # down to nodes of two points
    # a leaf beside a node that goes on splitting: 257 -> 128 | 129, 1028 -> ... -> 128 | 129
    "straddle257": (257, 4, 4, 128, "f64", 1, "cont"),
    "straddle1028": (1028, 4, 6, 128, "f32", 1, "grid"),
    "n2049":       (2049, 16, 9, 10, "f64", 0, "cont"),
    "n4097":       (4097, 16, 12, 4, "f64", 0, "cont"),
    "n2049_gen":   (2049, 4, 9, 10, "f64", 1, "cont"),
    "n70001":      (70001, 4, 16, 20, "f64", 0, "cont"),
    "n4096_f32":   (4096, 16, 8, 8, "f32", 0, "grid"),
    # ties
    "same":        (1024, 2, 6, 4, "f64", 1, "same"),
    "same_small":  (100, 2, 6, 4, "f32", 1, "same"),
    "two_values":  (1000, 3, 6, 4, "f64", 1, "two"),
    "signed_zero": (777, 3, 6, 4, "f64", 1, "zero"),
    "round1":      (5000, 4, 10, 8, "f64", 0, "round"),
    "pool_full":   (1024, 2, 3, 1, "f64", 1, "pool0"),        # exactly K_POOL tied positions
    "pool_over":   (1024, 2, 3, 1, "f64", 1, "pool1"),        # K_POOL + 1: the fallback
    "pool_full_pk": (1024, 64, 3, 1, "f64", 1, "pool0"),
    "pool_over_pk": (1024, 64, 3, 1, "f64", 1, "pool1"),
    "pool_over_d1": (1000, 2, 3, 1, "f64", 1, "pool1_d1"),    # ... inside one node of depth 1
}
D = 8


def unit_planes(T, L):
    """level l of every tree projects on coordinate l: the key columns are the data columns"""
    R = np.zeros((T, L, D))
    for l in range(L):
        R[:, l, l % D] = 1.0
    return R


def spread(rng, n):
    """n distinct values, evenly spaced (no two share a 21-bit image), in random order"""
    return rng.permutation(np.linspace(-1.0, 1.0, n))


def make(name):
    """-> X, R; seeded by the case's name"""
    N, T, L, ml, dtype, no_stream, kind = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if kind in ("cont", "round"):
        X = rng.standard_normal((N, D))
        if kind == "round":
            X = np.round(X, 1)
        R = rng.standard_normal((T, L, D)) * (rng.random((T, L, D)) < 0.6)
    elif kind == "grid":
        # projections that are exact in f32 in any order of summation (20 bits), so that the f32
        # build has the oracle's keys: multiples of 2^-14 below 8, hyperplanes of 0 / +-1
        X = np.clip(np.round(rng.standard_normal((N, D)) * 2.0 ** 14) / 2.0 ** 14, -7.0, 7.0)
        R = rng.integers(-1, 2, size=(T, L, D)).astype(np.float64)
    elif kind == "same":
        X = np.full((N, D), 0.375)
        R = unit_planes(T, L)
    elif kind == "two":
        X = np.where(rng.random((N, D)) < 0.45, -1.5, 2.25)
        R = unit_planes(T, L)
    elif kind == "zero":
        X = np.where(rng.random((N, D)) < 0.5, 0.0, -0.0)
        X[rng.random(N) < 0.2] = rng.standard_normal(D)
        R = unit_planes(T, L)
    else:
        X = np.stack([spread(rng, N) for _ in range(D)], axis=1)
        R = unit_planes(T, L)
        tied = K_POOL + (0 if kind == "pool0" else 1)
        if kind == "pool1_d1":
            # level 0 splits on column 0; the ties sit in column 1 among the points of the LEFT child
            left = np.argsort(X[:, 0], kind="stable")[:N // 2]
            X[left[:tied], 1] = 0.0625
        else:
            X[rng.permutation(N)[:tied], 0] = 0.0625
    if dtype == "f32":
        X = X.astype(np.float32)
    return np.ascontiguousarray(X), R


def tied_positions(col):
    """positions of the sorted column whose key equals a neighbour's"""
    s = np.sort(col)
    eq = s[1:] == s[:-1]
    return int((np.concatenate([[False], eq]) | np.concatenate([eq, [False]])).sum())


def test_cases_are_what_they_claim():
    tops = {k: wave_tops(v[0], v[2], v[3]) for k, v in SHAPES.items()}
    top_sizes = {n for t in tops.values() for _, n in t}
    assert {1024, 1023, 513, 512, 683, 257, 50, 1000, 777} <= top_sizes
    assert any(n < 64 for n in top_sizes)
    # N = 2049 / 4097: tops of 512, 513 and of 1024, 1025 -> 512, 513
    assert {n for _, n in tops["n2049"]} == {1024, 512, 513}
    assert {n for _, n in tops["n4097"]} == {1024, 512, 513}
    # children that differ by one at EVERY depth, down to the last level of a launch
    for d in range(1, K_LEVELS):
        s = sizes_at(1023, d)
        assert max(s) - min(s) == 1
    # packed images: at most three wave levels, one wave launch covers the points, N * T >= 2^16
    for k in ("n1024_pk", "n1023_pk", "n513_pk", "n512_pk", "n65536_pk", "n1023_f32", "pool_full_pk",
              "pool_over_pk"):
        N, T, L, ml = SHAPES[k][:4]
        assert N * T >= 1 << 16
        assert all(1 <= split_depth(n, lv, L, ml) <= 3 for lv, n in tops[k])
        assert sum(n for _, n in tops[k]) == N
    # five levels in one launch and nodes that stay active for a second one
    for k in ("n1024_deep", "n1023_deep", "n683_deep"):
        N, T, L, ml = SHAPES[k][:4]
        assert split_depth(N, 0, L, ml) > K_LEVELS
    # a leaf and a node that splits again, siblings in one wave
    for k in ("straddle257", "straddle1028"):
        N, T, L, ml = SHAPES[k][:4]
        depth = {257: 1, 1028: 3}[N]
        assert {128, 129} <= set(sizes_at(N, depth)) and ml == 128
        assert split_depth(128, depth, L, ml) == 0 and split_depth(129, depth, L, ml) >= 1
    # tie counts, on the key column of the level they are meant for
    X, _ = make("pool_full")
    assert tied_positions(X[:, 0]) == K_POOL and all(tied_positions(X[:, c]) == 0 for c in (1, 2))
    X, _ = make("pool_over")
    assert tied_positions(X[:, 0]) == K_POOL + 1
    X, _ = make("pool_over_pk")
    assert tied_positions(X[:, 0]) == K_POOL + 1
    X, _ = make("pool_over_d1")
    left = np.argsort(X[:, 0], kind="stable")[:500]
    assert tied_positions(X[:, 0]) == 0 and tied_positions(X[left, 1]) == K_POOL + 1
    X, _ = make("same")
    assert tied_positions(X[:, 0]) == 1024
    X, _ = make("two_values")
    assert len(np.unique(X[:, 0])) == 2
    X, _ = make("signed_zero")
    assert np.signbit(X[X[:, 0] == 0, 0]).any() and not np.signbit(X[X[:, 0] == 0, 0]).all()
    # f32 cases: the keys are exact in f32
    for k, v in SHAPES.items():
        if v[4] == "f32":
            X, R = make(k)
            assert X.dtype == np.float32
            P = np.abs(X.astype(np.float64)) @ np.abs(R.reshape(-1, D)).T
            assert P.max() < 64 and np.array_equal(X.astype(np.float64) * 2.0 ** 14 % 1, np.zeros(X.shape))


# --------------------------------------------------------------------------- GPU
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


@pytest.mark.gpu
@pytest.mark.parametrize("no_wpack", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forest_equals_the_oracle_and_the_select_kernel(rp, ctx, oracle, name, no_wpack):
    N, T, L, ml, dtype, no_stream, kind = SHAPES[name]
    X, R = make(name)
    fo = oracle.forest_build_dense(X.astype(np.float64), R, ml, threads=4)
    with options(ctx, no_stream=no_stream, no_wpack=no_wpack):
        f = rp.forestBatch(0, L, ml, T, 0.5, D, X, ctx=ctx, hyperplanes=R, mode=rp.RPT_PROJ_EXACT)
        with options(ctx, no_wsort=1):
            g = rp.forestBatch(0, L, ml, T, 0.5, D, X, ctx=ctx, hyperplanes=R, mode=rp.RPT_PROJ_EXACT)
    for t in range(T):
        assert np.array_equal(np.sort(f.perm[t]), np.arange(N)), "tree %d: not a permutation" % t
    # as bits (NaN where NaN): np.array_equal cannot tell the -0.0 of "signed_zero" from +0.0
    split_ref.assert_forest_bits_equal(f, g, "differs from no_wsort:")
    split_ref.assert_forest_bits_equal(f, fo, "differs from the oracle:")
    assert f.stats() == g.stats()
