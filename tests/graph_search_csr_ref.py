"""Helpers of the tests of the beam search on SVector (CSR) rows (include/rptree_hip.h,
rpt_graph_search_csr_*), shared by tests/test_graph_search_csr_host.py and
tests/test_gpu_graph_search_csr.py.  Not a test module.

The definition is the dense one on dense(q) and dense(x): absent columns +0.0, f32 values widened
exactly, a stored zero a zero.  So the reference is graph_search_ref on densify(...);
query_matrix_csr restates what the kernel does instead of visiting all d columns, the fold over the
union of the two supports only."""
import numpy as np

import graph_search_ref as sref
import knn_graph_csr_ref as cref

bits = sref.bits
assert_same_answer = sref.assert_same_answer


def query_matrix_csr(csrX, csrQ):
    """dist(q, v) for every query q and every row v by union_fold: [nq][n]"""
    X, Q = cref.rows_of(csrX), cref.rows_of(csrQ)
    D = np.empty((len(Q), len(X)))
    for i, (cq, vq) in enumerate(Q):
        for j, (cx, vx) in enumerate(X):
            D[i, j] = cref.union_fold(cq, vq, cx, vx)
    return D


def graph_search_csr_ref(csrX, csrQ, gids, gcount, seeds, k, ef, visited=True, D=None):
    """graph_search_ref on the dense-ified sets -> (ids, dist, count), expansions, offered, upper.
    D: the queries' distances to every row, when the caller has them already."""
    return sref.graph_search_ref(cref.densify(csrX), cref.densify(csrQ), gids, gcount, seeds, k, ef, "l2",
                                 visited=visited, D=D)
