"""The cases of tests/test_gpu_knn_tier_bounds.py are what they claim (no GPU): asserted from the
emulation of the shadows and the float64 truth of tests/knn_tier_ref.py only.  The emulation is a
proxy of the kernels' ranking values, not their bits; nothing here checks the kernels."""
import numpy as np
import pytest

import knn_tier_ref as ref

N, NQ, NCAND = 6397, 48, 1200     # the GPU file's sweep shape; 1200 candidates: 12 trees x leaves of 100
DENSE_TIERS = ("f32", "half", "f32half")
DIMS = (16, 37, 128, 208)
KS = (1, 10, 24)


def _sweep(tier, d):
    """[(c, k, order differs with the kept set whole, kept set misses)] over the tier's ladder"""
    out = []
    for c in ref.LADDER[tier]:
        if tier in ("csr32", "ell"):
            X, Q, src = ref.offset_sweep_csr(c, N, 64, 16, NQ, 7)
        else:
            X, Q, src = ref.offset_sweep(tier, c, N, d, NQ, 7)
        cands = ref.proxy_candidates(src, N, NCAND)
        sh = ref.CsrShadow(tier, X) if tier in ("csr32", "ell") else ref.Shadow(tier, X)
        for k in (10, 24):
            differs, misses = ref.sweep_stats(tier, X, Q, k, cands, shadow=sh)
            out.append((c, k, differs, misses))
    return out


@pytest.mark.parametrize("tier,d", [("f32", 16), ("f32", 128), ("half", 16), ("half", 128), ("f32half", 37),
                                    ("int8", 16), ("int8", 128), ("csr32", 64), ("ell", 64)])
def test_every_sweep_crosses_from_misordered_to_missed(tier, d):
    """Every ladder has a step where the emulated top k is in another order than the exact one for at
    least a quarter of the queries while the kept set still holds every true neighbour (the tier's
    answer is right only because the kept rows are evaluated again), and a step where the kept set
    misses a true neighbour for at least a quarter of them (only the certificate and the exact
    fallback stand between that and a wrong answer)."""
    rows = _sweep(tier, d)
    for r in rows:
        print("%s d=%d c=%g k=%d: order differs (kept set whole) %d / %d, kept set misses %d / %d"
              % (tier, d, r[0], r[1], r[2], NQ, r[3], NQ))
    assert any(r[2] * 4 >= NQ for r in rows)
    assert any(r[3] * 4 >= NQ for r in rows)
    # the first step of the f32 and half ladders is the regime of the older tests: nothing is missed
    assert all(r[3] == 0 for r in rows if r[0] == ref.LADDER[tier][0])


ALIGNED = [(t, d, k, retry) for t in DENSE_TIERS for d in DIMS for k in KS for retry in (False, True)]


@pytest.mark.parametrize("tier,d,k,retry", ALIGNED)
def test_aligned_dense_cases_drop_every_true_neighbour(tier, d, k, retry):
    """The k true neighbours B are the float64 answer, separated from the (k+1)-th row by far more than
    1e-9; the first attempt keeps only decoys (all k dropped); in the retry variant so does the wider
    second attempt, whose cut then is the one the certificate decides.  The critical scale (F - dk) /
    err — the factor under which a smaller bound certifies the wrong cut — is at least 0.2: 0.31 on the
    f32 shadow (eta = 0.5 lifts it from the 0.24 of eta -> 0), 0.75 on the half shadows, where only the
    rows are rounded and the stated bound has little slack."""
    for place in ("first", "last", "middle"):
        case = ref.aligned_dense(tier, d, k, 301, place=place, retry=retry)
        rep = ref.aligned_report(case)
        print(tier, d, k, retry, place, "F %.6g dk %.6g err %.6g scale %.4f gap %.3g"
              % (rep["F"], rep["dk"], rep["bound"], rep["scale"], rep["gap"]))
        X = case["X"]
        assert len(X) % 2 == 1 and len(X) % 4 and len(X) % 64 and len(X) % 256
        assert rep["true_top_is_B"] and rep["gap"] > 1e-9
        assert rep["dropped_first"] == k and rep["dropped_deciding"] == k
        assert rep["scale"] >= 0.2
        A = X[case["ids_A"]]
        assert len(np.unique(A, axis=0)) == len(A)                         # the decoys are distinct
        n_dec = ref.kept_retry(tier, k) if retry else ref.kept(tier, k)
        assert len(A) == n_dec
        # ... and representable in the shadow, the block carries max_norm, every other row is tiny
        sh = ref.Shadow(tier, X)
        assert np.array_equal(sh.Xs[case["ids_A"]], A.astype(np.float64))
        block = np.concatenate([case["ids_A"], case["ids_B"]])
        norms = np.sqrt((X.astype(np.float64) ** 2).sum(1))
        rest = np.setdiff1d(np.arange(len(X)), block)
        assert norms[rest].max() < 1e-4 * norms[block].min()
        assert {"first": block.min() == 0, "last": block.max() == len(X) - 1,
                "middle": 0 < block.min() and block.max() < len(X) - 1}[place]


@pytest.mark.parametrize("k", KS)
def test_aligned_csr_cases(k):
    """CSR rows, offsets on the stored values only, the query on a column of its own.  The half table
    reaches 0.75 of its stated bound.  The (u16, f32) shadow does NOT reach 0.2: its bound E2 = (chain +
    8) u (2 xmax^2 + 4 |q|^2) carries seventeen roundings of headroom for the float32 arithmetic of the
    ranking value, and inputs rounded the worst way move the squared distance by two of them; the best
    this geometry reaches is 0.049 (measured here, asserted at 0.045), so a bound of an eighth survives
    on this tier and only one of about 1 / 32 would not.  A near query (x ~ q) reaches less still: there
    the rounding moves the squared distance in second order, far below the ranking value's own
    arithmetic, and the certificate never passes."""
    for tier, floor in (("csr32", 0.045), ("ell", 0.2)):
        for place in ("first", "last", "middle"):
            case = ref.aligned_csr(tier, k, 301, place=place)
            rep = ref.aligned_report(case)
            print(tier, k, place, "F %.9g dk %.9g bound %s scale %.4f gap %.3g"
                  % (rep["F"], rep["dk"], rep["bound"], rep["scale"], rep["gap"]))
            X = case["X"]
            assert X.ascending() and case["q"].ascending()
            assert rep["true_top_is_B"] and rep["gap"] > 1e-9
            assert rep["dropped_first"] == k
            assert rep["scale"] >= floor
            A = X.vals[case["ids_A"]]
            assert len(np.unique(A, axis=0)) == len(A) == ref.kept(tier, k)
            # the truth separates by far more than the header's 1e-8 |q| of the exact CSR distance
            qd = case["q"].dense()[0]
            ex = np.sort(ref.exact_csr(X, qd))
            assert ex[k] - ex[k - 1] > 100 * 1e-8 * np.sqrt((qd * qd).sum())


def test_int8_outlier_case_quantises_to_a_handful_of_codes():
    X, Q, src = ref.int8_outlier(6397, 128, 48, 3)
    sh = ref.Shadow("int8", X)
    codes = np.unique(sh.codes)
    print("int8 outlier: scale %.4g, codes %s, max row error %.4g" % (sh.s, codes.tolist(), sh.emax))
    assert len(codes) <= 4 and 127 in codes                      # 0, +-1 and the outlier's 127
    cands = ref.proxy_candidates(src, len(X), NCAND)
    tied = 0
    for i, idx in enumerate(cands):
        est = sh.estimate(Q[i], idx)
        tied += len(np.unique(est)) * 4 < len(est)               # ties everywhere in the ranking value
    assert tied == len(Q)
    inside = np.abs(Q).max(1) < 100.0
    assert inside.sum() >= len(Q) // 2 and (~inside).sum() >= len(Q) // 4
    # the kept set (k + 48 of 1200 tied candidates) misses true neighbours for most queries
    differs, misses = ref.sweep_stats("int8", X, Q, 10, cands, shadow=sh)
    print("int8 outlier: kept set misses a true neighbour for %d of %d queries" % (misses, len(Q)))
    assert misses * 4 >= len(Q)


def test_stated_bounds_agree_with_each_other():
    """The workgroup / one-wave expression and TierBounds are the same bound: err = A + Bt F on f64 rows,
    and on f32 rows (A + Bt F)(1 + Bf) + Bf F up to the second-order term."""
    for tier in DENSE_TIERS:
        for d in DIMS:
            f64 = tier != "f32half"
            xmax, qn, F = 4100.0 * np.sqrt(d), 4096.0 * np.sqrt(d), 3.0
            A, Bt, Bf = ref.tier_bounds(tier, f64, d, xmax, qn)
            err = ref.err_dense(tier, f64, d, xmax, qn, F)
            want = (A + Bt * F) * (1 + Bf) + Bf * F
            assert abs(err - want) <= 1e-9 * err
