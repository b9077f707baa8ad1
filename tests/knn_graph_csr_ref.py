"""Helpers of the CSR kNN graph tests (include/rptree_hip.h, rpt_knn_graph_csr_* and
rpt_knn_graph_refine_csr_*), shared by tests/test_knn_graph_csr_host.py and
tests/test_gpu_knn_graph_csr.py.  Not a test module.

The definition is the dense one on dense(x): absent columns +0.0, f32 values widened exactly, a
stored zero a zero.  So the reference is knn_graph_ref / knn_graph_refine_ref on densify(...); the
union-of-supports fold here restates what the kernels do instead of visiting all d columns."""
import numpy as np

from knn_graph_ref import fold_dist, knn_graph_ref, leaf_slices, bits, assert_same_graph  # noqa: F401
from knn_graph_refine_ref import refine_ref, exact_graph, recall  # noqa: F401


def make_csr(seed, n, d, density, dtype=np.float64, empty=()):
    """-> (rowptr int64, col int32 strictly ascending per row, val, d); rows listed in `empty` hold
    nothing"""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, d)) < density
    mask[list(empty)] = False
    vals = rng.standard_normal((n, d)).astype(dtype)
    vals[vals == 0] = 1
    return from_dense_mask(vals, mask, d)


def from_dense_mask(vals, mask, d):
    """the entries of vals where mask holds, row by row with ascending columns"""
    n = vals.shape[0]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(mask.sum(axis=1))
    rows, cols = np.nonzero(mask)                          # row-major: columns ascend inside a row
    return rowptr, cols.astype(np.int32), np.ascontiguousarray(vals[rows, cols]), int(d)


def from_rows(rows, d, dtype=np.float64):
    """rows: a list of (columns, values) -> the CSR tuple"""
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(c) for c, _ in rows])
    col = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows] + [np.zeros(0, dtype=np.int32)])
    val = np.concatenate([np.asarray(v, dtype=dtype) for _, v in rows] + [np.zeros(0, dtype=dtype)])
    return rowptr, col, val, int(d)


def rows_of(csr):
    rowptr, col, val, _ = csr
    return [(col[rowptr[i]:rowptr[i + 1]], val[rowptr[i]:rowptr[i + 1]]) for i in range(len(rowptr) - 1)]


def densify(csr):
    """dense(x) of every row as doubles: absent columns +0.0, values widened exactly, stored zeros kept"""
    rowptr, col, val, d = csr
    n = len(rowptr) - 1
    X = np.zeros((n, d), dtype=np.float64)
    X[np.repeat(np.arange(n), np.diff(rowptr)), col] = val.astype(np.float64)
    return X


def union_fold(ca, va, cb, vb):
    """the fold over the ascending union of the two supports only: sqrt(((0 + (a_c - b_c)^2) + ...)),
    an absent entry being +0.0"""
    cols = np.union1d(ca, cb)
    a = np.zeros(len(cols))
    b = np.zeros(len(cols))
    a[np.searchsorted(cols, ca)] = np.asarray(va, dtype=np.float64)
    b[np.searchsorted(cols, cb)] = np.asarray(vb, dtype=np.float64)
    acc = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for x, y in zip(a, b):
            t = x - y
            acc = acc + t * t
        return np.sqrt(np.float64(acc))
