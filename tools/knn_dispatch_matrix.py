"""Which fused kNN kernel answers which call, and with what: a walk over the rows of the host plan's
table (tests/knn_plan_check.cpp) that the public API reaches, at small shapes.  Per case and batch
one line: ranking tier, uncertified queries, in-kernel retries, candidates visited and a SHA-256 over
the ids, the distances' bits and the counts.  Run under tools/ktrace.sh, the per-kernel launch counts
(full template names) say which kernels ran; two builds that print the same lines and launch the same
kernels the same number of times dispatch alike.
usage: python tools/knn_dispatch_matrix.py"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rp-tree_amd", "python"))
import numpy as np
import rptree_amd as rp
from rptree_amd import _lib

NQ, MIN_LEAF = 64, 32
ctx = rp.default_context()
L_ = _lib.lib()


def last(name, ctype=C.c_int64):
    v = ctype(-1)
    _lib.check(getattr(L_, "rpt_knn_last_" + name)(ctx._h, C.byref(v)))
    return v.value


def dense(n, d, dtype, seed=7):
    X = np.random.default_rng(seed).standard_normal((n, d))
    if dtype == "f32":
        return X.astype(np.float32)
    if dtype == "bf16":
        return rp.to_bf16(X.astype(np.float32))
    return X


def sparse(n, d, dtype, seed=9, per_row=12):
    rng = np.random.default_rng(seed)
    col = np.concatenate([np.sort(rng.choice(d, per_row, replace=False)) for _ in range(n)]).astype(np.int32)
    val = rng.standard_normal(n * per_row).astype(np.float32 if dtype == "f32" else np.float64)
    return np.arange(n + 1, dtype=np.int64) * per_row, col, val, d


def rows(data, lo, hi):
    if isinstance(data, tuple):
        rowptr, col, val, d = data
        a, b = rowptr[lo], rowptr[hi]
        return rowptr[lo:hi + 1] - a, col[a:b], val[a:b], d
    return data[lo:hi]


def case(name, dtype, n, d, T, k, opts=None, csr=False, self_queries=False, batches=2, **knn):
    """A fresh dataset and forest (no shadows, no tier state), then `batches` batches of NQ queries."""
    data = sparse(n, d, dtype) if csr else dense(n, d, dtype)
    queries = data if self_queries else (sparse(NQ * batches, d, dtype, seed=21) if csr
                                         else dense(NQ * batches, d, dtype, seed=21))
    ds = rp.Dataset.csr(ctx, *data) if csr else rp.Dataset.dense(ctx, data, rp.RPT_BF16 if dtype == "bf16" else None)
    cfg = rp.rpTreeCfg(MIN_LEAF, n, d)
    f = rp.forestBatch(1235137, cfg.fpMaxTreeDepth, MIN_LEAF, T, cfg.fpProjNzDensity, d, ds, ctx=ctx)
    for o, v in (opts or {}).items():
        ctx.set_option(o, v)
    try:
        for b in range(batches):
            ids, dist, cnt = rp.knnBatch(k, f, rows(queries, b * NQ, (b + 1) * NQ), **knn)
            h = hashlib.sha256(ids.tobytes() + dist.tobytes() + cnt.tobytes()).hexdigest()
            print("%-44s batch %d  tier %d  uncertified %3d  retries %3d  candidates %7d  %s" % (
                name, b, last("tier", C.c_int32), last("uncertified"), last("retries"), last("candidates"), h),
                flush=True)
    finally:
        for o in (opts or {}):
            ctx.set_option(o, 0 if o != "knn_wave" else -1)
        f.close()
        ds.close()


def main():
    for dtype in ("f64", "f32", "bf16"):
        for d in ((32, 20) if dtype == "f64" else (32,)):
            for T in (2, 8, 40, 80):
                for k in (5, 50):
                    case("%s d%d T%d k%d" % (dtype, d, T, k), dtype, 4096, d, T, k)
    for T in (2, 8, 40):
        for opts in ({"knn_shard_old": 1}, {"knn_wave": 0}, {"knn_wave": 1}, {"knn_no_pre16": 1}, {"knn_no_pre32": 1},
                     {"knn_no_pre8": 1}, {"knn_shard_old": 1, "knn_no_pre8": 1},
                     {"knn_kp": 9, "knn_kp16": 12, "knn_kp8": 20}):
            tag = ",".join("%s=%d" % kv for kv in opts.items())
            case("f64 d32 T%d k5 %s" % (T, tag), "f64", 4096, 32, T, 5, opts)
            if "knn_kp" not in opts:
                case("f32 d32 T%d k5 %s" % (T, tag), "f32", 4096, 32, T, 5, opts)
    for T in (2, 40):
        case("bf16 d32 T%d k5 knn_kp8=58" % T, "bf16", 4096, 32, T, 5, {"knn_kp8": 58})
    case("f64 d32 T8 k5 dedup", "f64", 4096, 32, 8, 5, dedup=True)
    case("f64 d32 T8 k5 vote 2", "f64", 4096, 32, 8, 5, vote=2)
    case("f64 d32 T40 k5 vote 2", "f64", 4096, 32, 40, 5, vote=2)
    for dtype in ("f64", "f32"):
        case("csr %s d64 T8 k5" % dtype, dtype, 2000, 64, 8, 5, csr=True)
        case("csr %s d64 T8 k5 knn_csr_pre32" % dtype, dtype, 2000, 64, 8, 5, {"knn_csr_pre32": 1}, csr=True)
    case("csr f64 d64 T8 k5 knn_csr_pre32,knn_no_pre16", "f64", 2000, 64, 8, 5,
         {"knn_csr_pre32": 1, "knn_no_pre16": 1}, csr=True)
    # queries that are data points: one copy per tree ties at the cut (the int8 tier told to keep 13: fewer
    # than the copies on its wider second attempt too), cuts go uncertified, the exact kernel (f64 rows) /
    # the second launch (f32, CSR rows) answers and the forest drops its tiers
    for T in (40, 80):
        case("f64 d32 T%d k5 self knn_kp8=13" % T, "f64", 4096, 32, T, 5, {"knn_kp8": 13}, self_queries=True, batches=4)
        case("f32 d32 T%d k5 self knn_kp8=13" % T, "f32", 4096, 32, T, 5, {"knn_kp8": 13}, self_queries=True, batches=3)
    case("csr f64 d64 T40 k5 self", "f64", 2000, 64, 40, 5, csr=True, self_queries=True, batches=3)


if __name__ == "__main__":
    main()
