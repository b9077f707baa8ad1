"""Exhaustive kNN over CSR rows (rpt_brute_knn_dev, brute_csr_kernel) at the C3 shape: 1 M x 784,
density 0.19, U(0,1] values, 1 000 queries, k = 10.  Per query tile (brute_csr_tile = 0 auto, 1, 2, 4,
8): ms per batch (median of REPS timed calls behind a warm-up, the stream synchronised inside the
timed region), the byte floor ceil(nq / Qt) * (12 nnz + 8 n) at 8 TB/s and the fraction of it reached;
and, for scale, one query on one CPU thread (numpy over the CSR arrays, the same formula).  Prints one
JSON line.

    python tools/brute_csr_times.py [reps] [n] [nq]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rp-tree_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rptree_amd as rp  # noqa: E402
from rptree_amd import _lib  # noqa: E402

PEAK = 8e12


def sparse_uniform(n, d, density, seed):
    rng = np.random.default_rng(seed)
    cols, counts = [], []
    for r0 in range(0, n, 50_000):
        m = rng.random((min(50_000, n - r0), d), dtype=np.float32) < density
        counts.append(m.sum(axis=1))
        cols.append(np.nonzero(m)[1].astype(np.int32))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.concatenate(counts))
    return rowptr, np.concatenate(cols), 1.0 - rng.random(int(rowptr[-1]))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    nq = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    d, k = 784, 10
    ctx = rp.default_context()
    rowptr, col, val = sparse_uniform(n, d, 0.19, 1234)
    qr, qc, qv = sparse_uniform(nq, d, 0.19, 4321)
    nnz = int(rowptr[-1])
    ds = rp.Dataset.csr(ctx, rowptr, col, val, d)
    qs = rp.Dataset.csr(ctx, qr, qc, qv, d)
    ids = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    L = _lib.lib()

    def once():
        _lib.check(L.rpt_brute_knn_dev(ctx._h, ds._h, qs._h, k, 0, C.c_void_p(ids.data_ptr()),
                                       C.c_void_p(dist.data_ptr())))
        ctx.sync()

    res = {"tool": "brute_csr_times", "device": torch.cuda.get_device_name(0), "reps": reps,
           "workload": "%d x %d CSR f64, nnz %d, %d queries, k=%d" % (n, d, nnz, nq, k), "tiles": {}}
    answers = {}
    for tile in (0, 8, 4, 2, 1):
        old = ctx.set_option("brute_csr_tile", tile)
        try:
            once()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                once()
                ts.append((time.perf_counter() - t0) * 1e3)
        finally:
            ctx.set_option("brute_csr_tile", old)
        ts.sort()
        ms = ts[len(ts) // 2]
        qt = tile if tile else 4          # the auto tile at this shape
        floor_ms = -(-nq // qt) * (12 * nnz + 8 * n) / PEAK * 1e3
        res["tiles"]["auto" if tile == 0 else str(tile)] = {
            "ms": round(ms, 2), "min_ms": round(ts[0], 2), "max_ms": round(ts[-1], 2), "Qt": qt,
            "byte_floor_ms": round(floor_ms, 2), "fraction_of_floor": round(floor_ms / ms, 3)}
        answers[tile] = (ids.cpu().numpy().copy(), dist.cpu().numpy().copy())
    res["tiles_agree_bitwise"] = all(np.array_equal(answers[t][0], answers[0][0]) and
                                     np.array_equal(answers[t][1].view(np.uint64), answers[0][1].view(np.uint64))
                                     for t in answers)
    res["auto_over_tile1"] = round(res["tiles"]["1"]["ms"] / res["tiles"]["auto"]["ms"], 2)
    # one query on one CPU thread, the same formula over the CSR arrays
    q = np.zeros(d)
    q[qc[qr[0]:qr[1]]] = qv[qr[0]:qr[1]]
    t0 = time.perf_counter()
    qj = q[col]
    term = (val - qj) ** 2 - qj ** 2
    s = np.add.reduceat(term, np.minimum(rowptr[:-1], nnz - 1))
    s[rowptr[1:] == rowptr[:-1]] = 0.0
    dd = np.sqrt(np.maximum(s + (q * q).sum(), 0.0))
    best = np.lexsort((np.arange(n), dd))[:k]
    res["cpu_one_thread_one_query_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["cpu_ids_equal_device"] = bool(np.array_equal(best.astype(np.int32), answers[0][0][0]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
