"""numpy restatement of the kNN graph and its refinement on SVector (CSR) rows under the cosine and
inner-product distances (include/rptree_hip.h, rpt_knn_graph_csr_metric_* /
rpt_knn_graph_refine_csr_metric_*), shared by tests/test_knn_graph_metric_csr_host.py and
tests/test_gpu_knn_graph_metric_csr.py.  Not a test module; no library code is used here.

dotS(x, y): from +0.0, over the columns stored in BOTH rows in ascending order, acc = acc + x_c * y_c,
every product and sum rounded on its own.  inner: -dotS(x_i, x_j); cosine:
1 - dotS(x_i, x_j) / (sqrt(dotS(x_i, x_i)) * sqrt(dotS(x_j, x_j))).  The matrix of all pairs is built
column by column on top of knn_metric_csr_ref.dense:

    acc = where(P_i & P_j, acc + X_i * X_j, acc)

Mates, the order (distance, id) with NaN last, accumulate and the rounds are
knn_graph_metric_ref.knn_graph_metric_ref / refine_ref with that matrix handed in."""
import numpy as np

import knn_graph_metric_ref as mref
import knn_metric_csr_ref as sref
from knn_graph_csr_ref import make_csr, from_rows, rows_of, densify  # noqa: F401
from knn_graph_ref import leaf_slices, bits, assert_same_graph  # noqa: F401
from knn_graph_refine_ref import recall  # noqa: F401

METRICS = ("cosine", "inner")


def dense(csr):
    """-> (X [n][d] f64, P [n][d] bool: the stored entries) of a (rowptr, col, val, d) tuple"""
    rowptr, col, val, d = csr
    return sref.dense(rowptr, col, val, d)


def dots_matrix(X, P):
    """dotS(x_i, x_j) of every ordered pair: the masked fold, column by column"""
    n, d = X.shape
    acc = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for c in range(d):
            both = P[:, c][:, None] & P[:, c][None, :]
            if both.any():
                acc = np.where(both, acc + X[:, c][:, None] * X[:, c][None, :], acc)
    return acc


def zero_filled_matrix(X):
    """what a fold over zero-filled rows gives: acc + X_i * X_j over every column, absent entries as +0.0"""
    return mref.dot_matrix(X)


def dist_matrix(metric, G):
    """dist(i, j) of every pair from G = dots_matrix(X, P); the norms are G's diagonal"""
    with np.errstate(all="ignore"):
        if metric == "inner":
            return -G
        s = np.sqrt(np.diagonal(G).copy())
        return 1.0 - G / (s[:, None] * s[None, :])


def metric_matrix(csr, metric):
    X, P = dense(csr)
    return dist_matrix(metric, dots_matrix(X, P))


def knn_graph_ref(X64, perm, leaves, k, D, prior=None):
    return mref.knn_graph_metric_ref(X64, perm, leaves, k, D, prior)


def refine_ref(X64, graph, k, reverse, iters, D):
    return mref.refine_ref(X64, graph, k, reverse, iters, D)


def exact_graph(D, k):
    return mref.exact_graph(D, k)


def hand_graph(D, k, rows):
    return mref.hand_graph(D, k, rows)


def dot_pair(ca, va, cb, vb):
    """dotS of one pair by the two-pointer merge (knn_metric_csr_ref.dot_pair)"""
    with np.errstate(all="ignore"):
        return sref.dot_pair(ca, va, cb, vb)
