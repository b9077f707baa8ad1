"""The numpy restatement of the L2 kNN's definition that tests/test_gpu_knn_l2_cut.py compares the
device with equals the oracle, and the inputs built for that test do what they are built for: a
"keep k + 8 by another summation order, then fold" rule answers them wrongly (no GPU)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_l2_cut_ref as ref  # noqa: E402


def all_builders():
    """name -> (rows, queries) of every input builder"""
    out = {}
    for name, (args, _) in ref.BANDS.items():
        X, Q, _ = ref.band_set(**args)
        out[name] = (X, Q)
    out["rerun"] = ref.band_set(**ref.RERUN_BAND)[:2]
    out["copies"] = ref.copies_set()
    return out


def test_fold_equals_the_oracle_bit_for_bit(oracle):
    for name, (X, Q) in all_builders().items():
        for q in Q:
            want = np.array([oracle.metric_dd(x, q) for x in X])
            assert ref.same_bits(ref.fold_l2(X, q), want), name


def test_fold_of_nonfinite_queries():
    X, Q, _ = ref.band_set(**ref.BANDS["d37"][0])
    Qn = ref.with_nonfinite_queries(Q)
    assert np.isnan(ref.fold_l2(X, Qn[2])).all()
    assert np.isposinf(ref.fold_l2(X, Qn[3])).all()
    # NaN last by position, +inf ties by position; nub: +inf once, NaN equals nothing
    for q in Qn[2:]:
        ids, _ = ref.select(np.arange(len(X)), ref.fold_l2(X, q), 9, 0)
        assert np.array_equal(ids, np.arange(9))
    assert len(ref.select(np.arange(len(X)), ref.fold_l2(X, Qn[2]), 9, 2)[0]) == 9
    assert len(ref.select(np.arange(len(X)), ref.fold_l2(X, Qn[3]), 9, 2)[0]) == 1


@pytest.mark.parametrize("T", [1, 3])
def test_select_equals_the_oracle(oracle, T):
    X, Q, _ = ref.band_set(**ref.BANDS["d37"][0])
    n, d = X.shape
    fo = oracle.forest_build_dense(X, np.zeros((T, 0, d)), 0)
    cands = np.asarray(fo.perm).reshape(-1)
    assert np.array_equal(cands, ref.flat_candidates(n, T))
    for q in Q:
        vals = ref.fold_l2(X[cands], q)
        for dedup in (0, 1):
            for k in (1,) + ref.BAND_KS + (n, n * T + 5):
                wi, wv = oracle.knn_dense(fo, X, q, k, dedup=bool(dedup))
                gi, gv = ref.select(cands, vals, k, dedup)
                assert np.array_equal(gi, wi) and ref.same_bits(gv, wv), (T, dedup, k)


def test_select_nub_keeps_one_entry_per_value():
    ids = np.array([4, 5, 6, 7, 8])
    vals = np.array([2.0, 1.0, 2.0, np.nan, 1.0])
    gi, gv = ref.select(ids, vals, 5, 2)
    assert gi.tolist() == [5, 4, 7] and gv[:2].tolist() == [1.0, 2.0] and np.isnan(gv[2])
    gi, _ = ref.select(np.array([1, 1, 2, 2]), np.array([3.0, 3.0, 1.0, 1.0]), 4, 1)
    assert gi.tolist() == [2, 1]


@pytest.mark.parametrize("name", list(ref.BANDS))
def test_bands_are_bands(name):
    args, ks = ref.BANDS[name]
    X, Q, band = ref.band_set(**args)
    B = int(band.sum())
    assert B == args.get("B", 48)
    assert len(np.unique(X, axis=0)) == len(X)                       # pairwise different rows
    assert np.array_equal(np.sort(X[band], axis=1), np.tile(np.sort(X[band][0]), (B, 1)))
    for q in Q:
        v = ref.fold_l2(X, q)
        assert len(np.unique(v[band])) >= 3                          # at least 3 different fold values
        # 6 rows clearly nearer, the others clearly farther: every listed k cuts inside the band
        assert v[~band].min() < v[band].min() * 0.9 and (v[~band] < v[band].min()).sum() == 6
        assert (v[~band] > v[band].max() * 1.1).sum() == len(X) - B - 6
        assert all(6 < k <= 6 + B for k in ks)


@pytest.mark.parametrize("name", list(ref.BANDS))
def test_bands_defeat_a_margin_of_eight(name):
    """keep k + 8 by the model sum, then fold: a wrong answer for at least half of the k"""
    args, ks = ref.BANDS[name]
    X, Q, _ = ref.band_set(**args)
    ids = np.arange(len(X))
    for q in Q:
        vals = ref.fold_l2(X, q)
        wrong = 0
        for k in ks:
            wi, wv = ref.select(ids, vals, k, 0)
            gi, gv = ref.model_rule(ids, X, q, k)
            wrong += not (np.array_equal(gi, wi) and ref.same_bits(gv, wv))
        assert 2 * wrong >= len(ks), (name, wrong, len(ks))


def test_rerun_band_is_wider_than_any_kept_set():
    X, Q, band = ref.band_set(**ref.RERUN_BAND)
    assert len(X) > 2100 and int(band.sum()) > 224 + 6 and len(np.unique(X, axis=0)) == len(X)
    ids = np.arange(len(X))
    for q in Q:
        v = ref.fold_l2(X, q)
        assert len(np.unique(v[band])) >= 3 and (v[~band] < v[band].min()).sum() == 6 < ref.RERUN_K
        wi, wv = ref.select(ids, v, ref.RERUN_K, 0)
        gi, gv = ref.model_rule(ids, X, q, ref.RERUN_K)
        assert not (np.array_equal(gi, wi) and ref.same_bits(gv, wv))


def test_copies_pairs_are_ordered_oppositely_by_the_two_sums():
    X, Q = ref.copies_set()
    f = ref.fold_l2(X[:24], Q[0])
    m = ref.model_sum(X[:24], Q[0])
    assert len(np.unique(X, axis=0)) == len(X)
    # pair j clearly beyond pair j - 1 under both sums, the far rows beyond all of them
    assert (np.minimum(f[2::2], f[3::2]) > np.maximum(f[0:-2:2], f[1:-2:2]) * (1 + 5e-4)).all()
    assert ref.fold_l2(X[24:], Q[0]).min() > 2.0
    # the member that comes first (ties: the lower position) differs between the two sums
    first_f = f[1::2] < f[0::2]
    first_m = m[1::2] < m[0::2]
    assert int((first_f != first_m).sum()) >= 3, (first_f, first_m)


def test_copies_defeat_a_margin_counted_in_copies():
    """with T >= 5 copies of every row, k + 8 kept COPIES by the model sum hold only one member of
    the pair at the cut: the rule fails wherever the two sums order that pair oppositely"""
    X, Q = ref.copies_set()
    wrong = 0
    for T in ref.COPY_TREES:
        cands = ref.flat_candidates(len(X), T)
        vals = ref.fold_l2(X[cands], Q[0])
        for k in ref.copies_ks(12, T, 1024):
            wi, wv = ref.select(cands, vals, k, 0)
            gi, gv = ref.model_rule(cands, X[cands], Q[0], k)
            wrong += not (np.array_equal(gi, wi) and ref.same_bits(gv, wv))
    assert wrong >= 3, wrong
