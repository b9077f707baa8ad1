"""kNN graph and one NN-descent round on SVector (CSR) rows under the cosine and inner-product
distances (rpt_knn_graph_csr_metric_dev, rpt_knn_graph_refine_csr_metric_dev, csrc/graph_csr.hip) at
the C3 shape: 1 M x 784, density 0.19, U(0,1] values, 32 trees, minLeaf 128, k = 10.

    python tools/knn_graph_metric_csr_times.py [reps] --parent-lib PATH [--out FILE] [--n N]

Three steps, each a fresh child process under a time limit of its own (a step that fails or runs out
of time ends the run; nothing is recorded then):
  csr     this build on the CSR rows: rpt_knn_graph_csr_dev (L2: the structurally equal kernel, the
          yardstick for the fold); rpt_knn_graph_csr_metric_dev under cosine and inner on the default
          path and again with graph_csr_masked = 1 (the price of the presence mask; the checksums
          must agree); one refinement round (k = reverse = 10) under each metric
  parent  the library built from the parent commit (PATH, loaded through RPTREE_HIP_LIB): the only
          device route it has to this answer, rpt_knn_csr_metric_dev over all points with
          RPT_KNN_DEDUP, k + 1, under each metric
  dense   this build: rpt_knn_graph_metric_dev and one refinement round on the dense-ified rows
          (6.3 GB more), under each metric
All steps draw the same rows and hyperplanes and must report the same perm checksum; the csr and
dense steps must report the same graph checksums (every stored value is finite: bit-equal).  Timing:
HIP events on the ctx stream, median of REPS behind a warm-up.  Writes
profiles/knn_graph_metric_csr_times.json.  No ratio is fixed in advance: the file holds the times.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rp-tree_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rptree_amd import gen  # noqa: E402  (no library call: the parent's library lacks the new symbols)

D, DENSITY, T, MINL, K, SEED = 784, 0.19, 32, 128, 10, 1234
RPT_F64, RPT_PROJ_AUTO, RPT_KNN_DEDUP = 0, 0, 1
RPT_KNN_METRIC_COSINE, RPT_KNN_METRIC_INNER = 1 << 25, 1 << 26
METRICS = ("cosine", "inner")
STEP_LIMIT_S = {"csr": 420, "parent": 420, "dense": 420}


def sparse_uniform_device(dev, n, d, density, seed):
    """bench.py's C3 rows: Bernoulli support + U(0,1] values, built on the device as CSR tensors"""
    g = torch.Generator(device=dev).manual_seed(seed)
    cols, counts = [], []
    for r0 in range(0, n, 100_000):
        m = torch.rand((min(100_000, n - r0), d), device=dev, generator=g) < density
        counts.append(m.sum(dim=1))
        cols.append(m.nonzero()[:, 1].to(torch.int32))
    col = torch.cat(cols)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.cat(counts), 0)
    val = 1.0 - torch.rand(col.numel(), dtype=torch.float64, device=dev, generator=g)
    return rowptr, col, val


def cfg_of(n):
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))            # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    return maxd, pnz


def event_ms(stream, fn, reps, before=None):
    """median HIP-event time of fn() on the ctx stream, behind one warm-up; before(): untimed set-up"""
    s = torch.cuda.ExternalStream(stream)
    if before:
        before()
    fn()
    s.synchronize()
    ts = []
    for _ in range(reps):
        if before:
            before()
            s.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts


def graph_crc(ids, dist, cnt):
    return zlib.crc32(cnt.cpu().numpy().tobytes(), zlib.crc32(dist.cpu().numpy().tobytes(),
                                                              zlib.crc32(ids.cpu().numpy().tobytes())))


# ------------------------------------------------------------------ this build, CSR or dense-ified rows
def step_this_build(dense, n, reps):
    import rptree_amd as rp
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    rowptr, col, val = sparse_uniform_device(dev, n, D, DENSITY, SEED)
    nnz = int(val.numel())
    maxd, pnz = cfg_of(n)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, D)
    if dense:
        X = torch.zeros((n, D), dtype=torch.float64, device=dev)
        rows = torch.repeat_interleave(torch.arange(n, device=dev), rowptr[1:] - rowptr[:-1])
        X[rows, col.long()] = val
        del rows
        torch.cuda.synchronize(dev)
        ds = rp.Dataset.from_torch(ctx, X)
        graph, refine = rp.knnGraphMetricDev, rp.knnGraphRefineMetricDev
    else:
        ds = rp.Dataset.csr_from_torch(ctx, rowptr, col, val, D)
        graph, refine = rp.knnGraphMetricSVDev, rp.knnGraphRefineMetricSVDev
    f = rp._build(ctx, ds, R, maxd, MINL, RPT_PROJ_AUTO)
    ids = torch.empty((n, K), dtype=torch.int32, device=dev)
    dist = torch.empty((n, K), dtype=torch.float64, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ptrs = (ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    leaves = [int(s) for (_, _, _, s, leaf) in f.topology() if leaf]
    res = {"n": n, "nnz": nnz, "maxDepth": maxd, "leaves": [min(leaves), max(leaves)],
           "perm_crc": zlib.crc32(f.perm.tobytes())}
    if not dense:                                               # the L2 kernel of the same build
        res["l2_graph_ms"], res["l2_graph_all_ms"] = event_ms(ctx.stream, lambda: rp.knnGraphSVDev(K, f, *ptrs), reps)
        ctx.sync()
    for name in METRICS:
        m = rp.metricCosine if name == "cosine" else rp.metricInner
        out = {}
        if not dense:                                           # the masked fold first: the default graph stays in the arrays
            old = ctx.set_option("graph_csr_masked", 1)
            out["masked_graph_ms"], out["masked_graph_all_ms"] = event_ms(ctx.stream, lambda: graph(m, K, f, *ptrs), reps)
            ctx.sync()
            ctx.set_option("graph_csr_masked", old)
            out["masked_graph_crc"] = graph_crc(ids, dist, cnt)
        out["graph_ms"], out["graph_all_ms"] = event_ms(ctx.stream, lambda: graph(m, K, f, *ptrs), reps)
        ctx.sync()
        out["pairs"] = rp.knnGraphLastPairs(ctx)
        out["graph_crc"] = graph_crc(ids, dist, cnt)
        keep = (ids.clone(), dist.clone(), cnt.clone())

        def restore():                                          # every timed round starts from the forest's graph
            ids.copy_(keep[0])
            dist.copy_(keep[1])
            cnt.copy_(keep[2])
            torch.cuda.synchronize(dev)

        out["refine_round_ms"], out["refine_round_all_ms"] = event_ms(
            ctx.stream, lambda: refine(m, K, ds, *ptrs, iters=1, reverse=K), reps, before=restore)
        ctx.sync()
        _, out["refine_updates"], out["refine_candidates"] = rp.knnGraphRefineLast(ctx)
        out["refined_crc"] = graph_crc(ids, dist, cnt)
        del keep
        res[name] = out
    return res


# ------------------------------------------------------------------ the parent commit's library
def step_parent(n, reps):
    """raw ctypes on the library RPTREE_HIP_LIB names"""
    L = C.CDLL(os.environ["RPTREE_HIP_LIB"])
    vp = C.c_void_p

    def call(fn, *a):
        f = getattr(L, fn)
        f.restype = C.c_int32
        if f(*a) != 0:
            L.rpt_last_error.restype = C.c_char_p
            raise SystemExit("%s: %s" % (fn, L.rpt_last_error().decode()))

    dev = torch.device("cuda", 0)
    rowptr, col, val = sparse_uniform_device(dev, n, D, DENSITY, SEED)
    maxd, pnz = cfg_of(n)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, D)
    R = np.ascontiguousarray(R, dtype=np.float64)
    ctx, ds, f, stream = vp(), vp(), vp(), vp()
    call("rpt_ctx_create", C.c_int32(0), C.byref(ctx))
    call("rpt_ctx_stream", ctx, C.byref(stream))
    torch.cuda.synchronize(dev)
    call("rpt_dataset_csr_dev", ctx, vp(rowptr.data_ptr()), vp(col.data_ptr()), vp(val.data_ptr()), C.c_int64(n),
         C.c_int32(D), C.c_int32(RPT_F64), C.c_int64(val.numel()), C.byref(ds))
    call("rpt_forest_build", ctx, ds, vp(R.ctypes.data), C.c_int32(T), C.c_int32(maxd), C.c_int32(MINL),
         C.c_int32(RPT_PROJ_AUTO), C.byref(f))
    perm = np.empty((T, n), dtype=np.int32)
    call("rpt_forest_get_perm", f, vp(perm.ctypes.data))
    ids = torch.empty((n, K + 1), dtype=torch.int32, device=dev)
    dist = torch.empty((n, K + 1), dtype=torch.float64, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    res = {"perm_crc": zlib.crc32(perm.tobytes())}
    for name, bit in zip(METRICS, (RPT_KNN_METRIC_COSINE, RPT_KNN_METRIC_INNER)):
        def once():
            call("rpt_knn_csr_metric_dev", ctx, f, ds, ds, C.c_int32(K + 1), C.c_int32(RPT_KNN_DEDUP | bit),
                 vp(ids.data_ptr()), vp(dist.data_ptr()), vp(cnt.data_ptr()))

        ms, all_ms = event_ms(stream.value, once, reps)
        call("rpt_ctx_sync", ctx)
        cand, unc = C.c_int64(), C.c_int64()
        call("rpt_knn_last_candidates", ctx, C.byref(cand))
        call("rpt_knn_last_uncertified", ctx, C.byref(unc))
        res[name] = {"self_query_ms": ms, "self_query_all_ms": all_ms, "self_query_candidates": int(cand.value),
                     "self_query_uncertified": int(unc.value)}
    return res


def run_step(name, n, reps, parent_lib):
    env = dict(os.environ)
    if name == "parent":
        env["RPTREE_HIP_LIB"] = os.path.abspath(parent_lib)
    try:
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(n), str(reps)], env=env,
                            capture_output=True, text=True, timeout=STEP_LIMIT_S[name])
    except subprocess.TimeoutExpired:
        raise SystemExit("step %s ran out of its %d s: nothing recorded" % (name, STEP_LIMIT_S[name]))
    if pr.returncode != 0:
        raise SystemExit("step %s failed (%d): nothing recorded\n%s%s" % (name, pr.returncode, pr.stdout, pr.stderr))
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, n, reps = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        res = step_parent(n, reps) if name == "parent" else step_this_build(name == "dense", n, reps)
        print(json.dumps(res))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    parent = opt("--parent-lib", None)
    out_path = opt("--out", os.path.join(ROOT, "profiles", "knn_graph_metric_csr_times.json"))
    n = int(opt("--n", 1_000_000))
    reps = int(args[0]) if args else 5
    if not parent:
        raise SystemExit("--parent-lib PATH is required: the comparison is to the parent commit's library")
    csr = run_step("csr", n, reps, parent)
    par = run_step("parent", n, reps, parent)
    den = run_step("dense", n, reps, parent)
    if not (csr["perm_crc"] == par["perm_crc"] == den["perm_crc"]):
        raise SystemExit("the steps built different forests")
    res = {"tool": "tools/knn_graph_metric_csr_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step",
           "workload": "C3: %d x %d CSR f64, density %.2f (%d nonzeros), %d trees, minLeaf %d, maxDepth %d, k = %d, "
                       "leaves of %d..%d points" % (n, D, DENSITY, csr["nnz"], T, MINL, csr["maxDepth"], K,
                                                    csr["leaves"][0], csr["leaves"][1]),
           "l2_graph_csr_ms": csr["l2_graph_ms"], "l2_graph_csr_all_ms": csr["l2_graph_all_ms"],
           "parent_library": "the parent commit's build, loaded through RPTREE_HIP_LIB in a child process",
           "bit_equal": "graph and refined graph: the CSR and the dense-ified arrays have the same checksum under "
                        "each metric; the default and the masked path have the same checksum"}
    for name in METRICS:
        c, p, d = csr[name], par[name], den[name]
        if c["graph_crc"] != d["graph_crc"] or c["refined_crc"] != d["refined_crc"]:
            raise SystemExit("%s: the CSR and the dense-ified graphs differ" % name)
        if c["graph_crc"] != c["masked_graph_crc"]:
            raise SystemExit("%s: the default and the masked path differ" % name)
        res[name] = {"graph_csr_ms": c["graph_ms"], "graph_csr_all_ms": c["graph_all_ms"],
                     "graph_csr_masked_ms": c["masked_graph_ms"], "graph_csr_masked_all_ms": c["masked_graph_all_ms"],
                     "pairs": c["pairs"],
                     "parent_self_query_ms": p["self_query_ms"], "parent_self_query_all_ms": p["self_query_all_ms"],
                     "parent_candidates": p["self_query_candidates"],
                     "parent_uncertified": p["self_query_uncertified"],
                     "graph_dense_ms": d["graph_ms"], "graph_dense_all_ms": d["graph_all_ms"],
                     "refine_round_csr_ms": c["refine_round_ms"], "refine_round_csr_all_ms": c["refine_round_all_ms"],
                     "refine_round_dense_ms": d["refine_round_ms"],
                     "refine_round_dense_all_ms": d["refine_round_all_ms"],
                     "refine_candidates": c["refine_candidates"], "refine_updates": c["refine_updates"]}
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
