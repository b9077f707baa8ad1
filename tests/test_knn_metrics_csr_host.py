"""Host side of the cosine / inner-product kNN on SVector (CSR) rows: the definition dotS (the left
fold over the columns both rows store) against the dense metrics on dense-ified rows, where a stored
inf / NaN makes the two differ, the rounding bound between the fold and the kernels' lane-parallel
sum, that the certificate holds on the GPU test's fixture, and the header / ctypes / Python surface.
No GPU needed."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import knn_metric_csr_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rptree_hip.h")).read()
ENTRY_POINTS = ("rpt_knn_csr_metric_host", "rpt_knn_csr_metric_dev", "rpt_brute_knn_csr_metric_host",
                "rpt_brute_knn_csr_metric_dev", "rpt_recall_hits_csr_metric_host")


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


def bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def same(a, b):
    return bits(a) == bits(b) or (a != a and b != b)


def sv(rp, csr, i, d):
    rowptr, col, val = csr
    a, b = rowptr[i], rowptr[i + 1]
    return rp.SVector(d, col[a:b], val[a:b])


def dense_row(csr, i, d):
    rowptr, col, val = csr
    x = np.zeros(d, dtype=np.float64)
    x[col[rowptr[i]:rowptr[i + 1]]] = val[rowptr[i]:rowptr[i + 1]].astype(np.float64)
    return x


def pairs(rp):
    """(csr, d, [(i, j)]): random rows with stored +-0.0, empty rows and duplicates (f64 and f32
    values), and the sparse 600 x 12 golden rows"""
    rng = np.random.default_rng(5)
    out = []
    for dtype in (np.float64, np.float32):
        rowptr, col, val = ref.random_csr(rng, 60, 40, 0.3, dtype, zeros=0.2)
        # rows 3 and 7 empty, row 11 a copy of row 10
        keep = np.ones(len(col), dtype=bool)
        for r in (3, 7):
            keep[rowptr[r]:rowptr[r + 1]] = False
        lens = np.diff(rowptr)
        lens[[3, 7]] = 0
        col, val = col[keep], val[keep]
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        a, b = rowptr[10], rowptr[11]
        a2, b2 = rowptr[11], rowptr[12]
        col = np.concatenate([col[:a2], col[a:b], col[b2:]])
        val = np.concatenate([val[:a2], val[a:b], val[b2:]])
        lens[11] = lens[10]
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ij = [(int(i), int(j)) for i, j in rng.integers(0, 60, (150, 2))]
        ij += [(3, 5), (5, 3), (3, 7), (10, 11), (11, 11), (0, 0)]
        out.append(((rowptr, col, val), 40, ij))
    z = np.load(os.path.join(ROOT, "tests", "golden", "forest_sparse_600x12.npz"))
    ij = [(int(i), int(j)) for i, j in rng.integers(0, 600, (150, 2))]
    out.append(((z["rowptr"], z["col"], z["val"]), int(z["d"]), ij))
    return out


def test_dots_equals_the_dense_metrics_on_dense_ified_rows(rp):
    """finite stored values: metricInner / metricCosine of two SVectors, the restatement (pair walk
    and column-vectorised) and the dense metrics of the dense-ified rows agree bit for bit"""
    checked = 0
    for csr, d, ij in pairs(rp):
        X, P = ref.dense(*csr, d)
        rn = ref.self_dots(X, P)
        for i, j in ij:
            xi, xj = dense_row(csr, i, d), dense_row(csr, j, d)
            u, v = sv(rp, csr, i, d), sv(rp, csr, j, d)
            want_i, want_c = rp.metricInner(xi, xj), rp.metricCosine(xi, xj)
            assert same(rp.metricInner(u, v), want_i), (i, j)
            assert same(rp.metricCosine(u, v), want_c), (i, j)
            assert same(-ref.dot_pair(u.svIdx, u.svVal, v.svIdx, v.svVal), want_i), (i, j)
            assert same(ref.distances(ref.INNER, X, P, rn, X[j], P[j])[i], want_i), (i, j)
            assert same(ref.distances(ref.COSINE, X, P, rn, X[j], P[j])[i], want_c), (i, j)
            checked += 1
    assert checked > 400
    # an empty row is NaN under cosine and -0.0 under the inner product, as a dense zero row is
    csr, d, _ = pairs(rp)[0]
    assert math.isnan(rp.metricCosine(sv(rp, csr, 3, d), sv(rp, csr, 5, d)))
    assert bits(rp.metricInner(sv(rp, csr, 3, d), sv(rp, csr, 5, d))) == bits(-0.0)
    with pytest.raises(TypeError):
        rp.metricInner(sv(rp, csr, 3, d), np.zeros(d))


def test_a_stored_inf_or_nan_counts_only_where_both_rows_store_the_column(rp):
    """one inf and one NaN stored on each side, in columns the other side lacks: the dense-ified fold
    meets inf * 0 = NaN, dotS does not — and that is what the reference's innerSS returns (two
    common columns: the right and the left fold add the same two products)"""
    d = 12
    x = rp.SVector(d, np.array([1, 3, 5, 8]), np.array([2.0, math.inf, -1.5, math.nan]))
    q = rp.SVector(d, np.array([1, 4, 5, 9]), np.array([0.5, math.nan, 4.0, -math.inf]))
    xd, qd = np.zeros(d), np.zeros(d)
    xd[x.svIdx], qd[q.svIdx] = x.svVal, q.svVal
    assert math.isnan(rp.metricInner(xd, qd))                       # the dense-ified fold
    want = (0.0 + 2.0 * 0.5) + (-1.5) * 4.0
    assert rp.metricInner(x, q) == -want == -rp.inner(x, q)         # innerSS visits common columns
    assert ref.dot_pair(x.svIdx, x.svVal, q.svIdx, q.svVal) == want
    X, P = ref.dense(np.array([0, 4]), x.svIdx, x.svVal, d)
    Q, QP = ref.dense(np.array([0, 4]), q.svIdx, q.svVal, d)
    assert ref.dots(X, P, Q[0], QP[0])[0] == want
    # cosine: the norms hold the non-finite squares, NaN either way
    assert math.isnan(rp.metricCosine(x, q))
    # a non-finite value in a COMMON column is a product like any other
    q2 = rp.SVector(d, np.array([1, 3]), np.array([0.5, 2.0]))
    assert rp.metricInner(x, q2) == -math.inf == -rp.inner(x, q2)
    q3 = rp.SVector(d, np.array([3, 8]), np.array([0.0, 1.0]))
    assert math.isnan(rp.metricInner(x, q3))                        # inf * 0 where BOTH store it


def hostile_pairs():
    """(name, x values, q values) on common columns 0 .. m-1"""
    rng = np.random.default_rng(8)
    out = []
    for m in (1, 63, 64, 65, 200):
        a = rng.standard_normal(m)
        out.append(("random%d" % m, a, rng.standard_normal(m)))
        b = np.ones(m)
        c = np.where(np.arange(m) % 2 == 0, 1.0, -1.0) * (1.0 + rng.random(m) * 1e-9)
        out.append(("cancel%d" % m, c * 1e8, b))                    # cancellation: dot << sum |p|
        out.append(("big%d" % m, a * 1e150, rng.standard_normal(m) * 1e150))
        out.append(("subnormal%d" % m, a * 1e-160, rng.standard_normal(m) * 1e-160))
    return out


@pytest.mark.parametrize("metric", [ref.INNER, ref.COSINE])
def test_fold_and_lane_parallel_sum_are_within_e(metric):
    """|fold - lane-parallel| <= E on hostile pairs, E = ref.slack for the pair's own norms; the
    cosine range rule makes E NaN where the norms leave [2^-900, 2^900]"""
    saw_nan = saw_bound = 0
    for name, a, b in hostile_pairs():
        m = len(a)
        idx = np.arange(m)
        fold = ref.dot_pair(idx, a, idx, b)
        lanes = ref.dot_lanes(idx, a, b)
        xx, qq = ref.dot_pair(idx, a, idx, a), ref.dot_pair(idx, b, idx, b)
        out_of_range = xx != 0.0 and not (2.0 ** -900 <= xx <= 2.0 ** 900)
        e = ref.slack(metric, m, qq, xx, out_of_range)
        vf, vl = ref.value(metric, fold, xx, qq), ref.value(metric, lanes, xx, qq)
        if metric == ref.COSINE and (name.startswith("big") and m > 1 or name.startswith("subnormal")):
            # |x|^2 ~ m 1e300 > 2^900 for m >= 2 / ~ 1e-320 < 2^-900: outside the range the bound needs
            assert math.isnan(e), name
            saw_nan += 1
            continue
        if math.isnan(e):
            assert metric == ref.COSINE and name == "big1" and out_of_range, name
            continue
        assert abs(float(vf) - float(vl)) <= e, (name, float(vf), float(vl), e)
        saw_bound += 1
    assert saw_bound >= 10 and (metric == ref.INNER or saw_nan >= 9)


@pytest.mark.parametrize("metric", [ref.INNER, ref.COSINE])
def test_the_fast_path_can_be_exercised_on_fixture_a(metric):
    """the reference's own certificate (k-th value strictly below the (k + 9)-th different value less
    E) holds for at least three quarters of fixture A's queries: the GPU test's bound on
    knn_last_uncertified is not vacuous"""
    data, queries, d = ref.fixture_a()
    X, P = ref.dense(*data, d)
    Q, QP = ref.dense(*queries, d)
    rn = ref.self_dots(X, P)
    max_rn, out = ref.row_stats(X, P, rn)
    assert not out and math.isfinite(max_rn)
    for k in (1, 10, 200):
        ok = 0
        for i in range(len(Q)):
            qq = ref.self_dots(Q[i][None], QP[i][None])[0]
            dv = ref.distances(metric, X, P, rn, Q[i], QP[i])
            ok += ref.certified(metric, dv, k, d, qq, max_rn, out)
        assert 4 * ok >= 3 * len(Q), (metric, k, ok)


def test_header_states_the_definition_and_the_refusals():
    assert "RPT_KNN_METRIC_COSINE / _INNER on CSR data: RPT_E_UNSUPPORTED." in HEADER
    for name in ENTRY_POINTS:
        assert re.search(r"int32_t\s+%s\s*\(" % name, HEADER), name
    flat = re.sub(r"\s*\n\s*\*\s*", " ", HEADER)
    for phrase in ("columns stored in BOTH rows in ascending column order",
                   "every product and sum rounded on its own, no FMA",
                   "Equal to the dense definition for finite values",
                   "Different with a stored inf or NaN",
                   "Not the reference's fold order",
                   "NaN behind every number",
                   "Neither bit or both: RPT_E_ARG",
                   "Dense data or a dense / CSR pair: RPT_E_ARG",
                   "RPT_KNN_METRIC_REFERENCE: RPT_E_ARG",
                   "RPT_KNN_VOTE: RPT_E_UNSUPPORTED"):
        assert phrase in flat, phrase
    assert re.search(r"#define RPT_ABI_VERSION 1\b", HEADER)


def test_ctypes_table_and_python_signatures(rp):
    from rptree_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["rpt_knn_csr_metric_host"] == _lib.SYMBOLS["rpt_knn_host"]
    assert _lib.SYMBOLS["rpt_knn_csr_metric_dev"] == _lib.SYMBOLS["rpt_knn_dev"]
    assert _lib.SYMBOLS["rpt_brute_knn_csr_metric_host"] == _lib.SYMBOLS["rpt_brute_knn_metric_host"]
    assert _lib.SYMBOLS["rpt_brute_knn_csr_metric_dev"] == _lib.SYMBOLS["rpt_brute_knn_dev"]
    assert _lib.SYMBOLS["rpt_recall_hits_csr_metric_host"] == _lib.SYMBOLS["rpt_recall_hits_host"]
    assert list(inspect.signature(rp.knnBatch).parameters) == ["k", "forest", "qs", "dedup", "vote",
                                                               "reference_metric", "metric"]
    assert list(inspect.signature(rp.bruteKnn).parameters) == ["forest_or_data", "qs", "k", "ctx", "metric",
                                                               "reference_metric"]
    assert list(inspect.signature(rp.recallHits).parameters) == ["distf", "forest", "k", "qs",
                                                                 "reference_metric"]
    for fn in (rp.metricInner, rp.metricCosine, rp.knnBatch, rp.bruteKnn, rp.recallHits):
        assert "SVector" in fn.__doc__, fn.__name__
