"""kNN time per query batch under L2 (default kernels), L2 on the all-f64 kernel (knn_no_pre32 = 1),
cosine and inner product (RPT_KNN_METRIC_COSINE / _INNER), at C2 (1 M x 128 f64, 32 trees) and on the
C4 shard (10 M x 128 f32, 8 of 64 trees, depth 17), for 10 000 and 100 000 queries.  Prints one JSON
line: ms per batch (median of REPS behind a warm-up), the candidates visited, and the row bytes
gathered (candidates x d x element size) / time as a fraction of 8 TB/s.

    python tools/knn_metric_times.py [c2,c4] [reps]
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

import torch  # noqa: E402

import rptree_amd as rp  # noqa: E402
from rptree_amd import _lib, gen  # noqa: E402

PEAK = 8e12


def time_batch(ctx, f, qs, k, flags, reps):
    nq = qs.n
    ids = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    dist = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    cnt = torch.empty((nq,), dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def once():
        _lib.check(L.rpt_knn_dev(ctx._h, f._h, f.data._h, qs._h, k, flags, ids.data_ptr(),
                                 dist.data_ptr(), cnt.data_ptr()))
        ctx.sync()

    once()                                        # warm-up (and the cosine row norms, once per dataset)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        once()
        ts.append((time.perf_counter() - t0) * 1e3)
    cand = C.c_int64()
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(cand)))
    ts.sort()
    return ts[len(ts) // 2], int(cand.value)


def leg(ctx, name, X, Qs, T, min_leaf, k, esize, reps):
    n, d = X.shape
    cfg = rp.rpTreeCfg(min_leaf, n, d)
    ds = rp.Dataset.from_torch(ctx, X)
    _, R = gen.forest_hyperplanes(1235137, T, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, d)
    f = rp._build(ctx, ds, R, cfg.fpMaxTreeDepth, min_leaf, rp.RPT_PROJ_AUTO)
    out = {"workload": "%s: %d x %d, %d trees, minLeaf %d, maxDepth %d, k=%d" %
                       (name, n, d, T, min_leaf, cfg.fpMaxTreeDepth, k)}
    cases = [("l2_default", 0, 0), ("l2_all_f64", 0, 1), ("cosine", rp.RPT_KNN_METRIC_COSINE, 0),
             ("inner", rp.RPT_KNN_METRIC_INNER, 0)]
    for nq, Q in Qs:
        qs = rp.Dataset.from_torch(ctx, Q)
        row = {}
        for label, flags, no_pre32 in cases:
            old = ctx.set_option("knn_no_pre32", no_pre32)
            try:
                ms, cand = time_batch(ctx, f, qs, k, flags, reps)
            finally:
                ctx.set_option("knn_no_pre32", old)
            row[label] = {"ms": round(ms, 3), "candidates": cand,
                          "gathered_GB": round(cand * d * esize / 1e9, 3),
                          "fraction_of_8TBs": round(cand * d * esize / (ms * 1e-3) / PEAK, 3)}
        base = row["l2_all_f64"]["ms"]
        row["cosine_over_l2_all_f64"] = round(row["cosine"]["ms"] / base, 3)
        row["inner_over_l2_all_f64"] = round(row["inner"]["ms"] / base, 3)
        out["nq%d" % nq] = row
        qs.close()
    f.close()
    ds.close()
    return out


def main():
    which = sys.argv[1].split(",") if len(sys.argv) > 1 else ["c2", "c4"]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda:0")
    ctx = rp.default_context()
    res = {"tool": "knn_metric_times", "device": torch.cuda.get_device_name(0), "reps": reps}
    if "c2" in which:
        X = gen.normal_dense2_torch(1234, 1_000_000, 128, dev)
        Qb = gen.normal_dense2_torch(4321, 100_000, 128, dev)
        torch.cuda.synchronize()
        res["c2"] = leg(ctx, "C2 f64", X, [(10_000, Qb[:10_000].contiguous()), (100_000, Qb)], 32, 128, 10, 8,
                        reps)
        del X, Qb
        torch.cuda.empty_cache()
    if "c4" in which:
        n, d = 10_000_000, 128
        g = torch.Generator(device=dev).manual_seed(1234)
        coin = (torch.rand(n, 1, device=dev, generator=g) < 0.5).float() * 2.0
        Xd = torch.randn(n, d, device=dev, dtype=torch.float32, generator=g) * 0.5 + coin
        del coin
        qi = torch.randint(0, n, (100_000,), device=dev, generator=g)
        Qd = (Xd[qi] * 1.001 + 0.003).contiguous()
        torch.cuda.synchronize()
        res["c4_shard"] = leg(ctx, "C4 shard f32 (8 of 64 trees)", Xd,
                              [(10_000, Qd[:10_000].contiguous()), (100_000, Qd)], 8, 128, 10, 4, reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
