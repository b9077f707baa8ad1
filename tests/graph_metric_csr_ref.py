"""Helpers of the tests of the graph search and the graph preparation on SVector (CSR) rows under the
cosine and inner-product distances (include/rptree_hip.h, rpt_graph_search_csr_metric_* /
rpt_graph_prepare_csr_metric_*), shared by tests/test_graph_metric_csr_host.py,
tests/test_gpu_graph_search_metric_csr.py and tests/test_gpu_graph_prepare_metric_csr.py.  Not a test
module; no library code is used here.

The distance is dotS's (knn_metric_csr_ref: from +0.0, over the columns stored in BOTH rows in
ascending order, acc = acc + x_c * y_c, every product and sum rounded on its own):
inner = -dotS(x, y), cosine = 1 - dotS(x, y) / (sqrt(dotS(x, x)) * sqrt(dotS(y, y))).  query_matrix
gives D[q][v] for a query set against the rows, rows_matrix D[i][j] among the rows
(knn_graph_metric_csr_ref.metric_matrix); the beam and the keep rule are graph_search_ref's and
graph_prepare_ref's with that matrix handed in.  dense_query_matrix / dense_rows_matrix are what the
dense entry points compute on the dense-ified rows (every column, absent entries as +0.0): the same
bits while every stored value is finite, other bits with a stored inf or NaN."""
import numpy as np

import graph_prepare_ref as pref
import graph_search_ref as gsref
import knn_graph_metric_csr_ref as mc
import knn_graph_metric_ref as mref
import knn_metric_csr_ref as sref
from knn_graph_csr_ref import make_csr, from_rows, rows_of, densify  # noqa: F401

METRICS = mc.METRICS
bits = mc.bits
assert_same_answer = gsref.assert_same_answer
DIVERSIFY, REVERSE = pref.DIVERSIFY, pref.REVERSE


def query_matrix(csrX, csrQ, metric):
    """dist(q, v) under dotS for every query q and every row v: [nq][n]"""
    X, P = mc.dense(csrX)
    Q, QP = mc.dense(csrQ)
    rn = sref.self_dots(X, P)
    qn = sref.self_dots(Q, QP)
    D = np.empty((Q.shape[0], X.shape[0]))
    for i in range(Q.shape[0]):
        D[i] = sref.value(metric, sref.dots(X, P, Q[i], QP[i]), rn, qn[i])
    return D


def rows_matrix(csr, metric):
    """dist(i, j) under dotS for every pair of rows: [n][n]"""
    return mc.metric_matrix(csr, metric)


def dense_query_matrix(csrX, csrQ, metric):
    """what rpt_graph_search_* computes on the dense-ified rows and queries"""
    return gsref.query_matrix(densify(csrX), densify(csrQ), metric)


def dense_rows_matrix(csr, metric):
    """what rpt_graph_prepare_* computes on the dense-ified rows"""
    return mref.metric_matrix(densify(csr), metric)


def graph_search_ref(csrX, csrQ, gids, gcount, seeds, k, ef, metric, visited=True, D=None):
    """-> (ids, dist, count), expansions, offered, upper"""
    if D is None:
        D = query_matrix(csrX, csrQ, metric)
    return gsref.graph_search_ref(densify(csrX), densify(csrQ), gids, gcount, seeds, k, ef, metric,
                                  visited=visited, D=D)


def graph_prepare_ref(graph, csr, kout, flags, metric, D=None):
    """-> (ids, dist, count), (pairs, occluded, capped)"""
    if D is None:
        D = rows_matrix(csr, metric)
    return pref.graph_prepare_ref(graph, D, kout, flags, len(csr[0]) - 1)


def exact_graph(D, k):
    """the exact k-NN graph of a [n][n] distance matrix, self excluded -> (ids, dist, count)"""
    return mc.exact_graph(D, k)
