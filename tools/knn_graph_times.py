"""kNN graph of the indexed points (rpt_knn_graph_dev, csrc/graph.hip) against the route it replaces:
rpt_knn_dev over all n stored points as queries with RPT_KNN_DEDUP and k + 1.

    python tools/knn_graph_times.py [c2[,c4,c5]] [reps] --parent-lib PATH [--out FILE]

C2 = the flagship shape (seeds of BASELINE configs[1]: 1 M x 128 f64, 32 trees, minLeaf 128, k = 10);
c4 / c5 = one GPU's shard of those configs (10 M x 128 f32, 8 trees / 1 M x 768 bf16, 16 trees,
k = 50: leaves above 128 points, the tiled kernel).  The graph call is timed with HIP events on the
ctx stream (median of REPS behind a warm-up), once before and once after the comparator.  The
comparator runs in a CHILD process whose RPTREE_HIP_LIB names the library built from the parent
commit (PATH), on the forest of the same seeds (the perm's checksum must agree), in the same run.
Writes profiles/knn_graph_times.json: both times, the pairs evaluated, the bytes of the model (every
leaf's rows once per tree for the graph, one row gather per candidate for the self-queries) and the
recall@10 of both answers against bruteKnn on 1 000 sampled points.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rp-tree_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rptree_amd import gen  # noqa: E402  (no library call: the child's library lacks the new symbols)

SHAPES = {  # name: n, d, dtype, trees, minLeaf, k, seed of the rows
    "c2": (1_000_000, 128, torch.float64, 32, 128, 10, 1234),
    "c4": (10_000_000, 128, torch.float32, 8, 128, 10, 1234),
    "c5": (1_000_000, 768, torch.bfloat16, 16, 256, 50, 99),
}
RPT_DT = {torch.float64: 0, torch.float32: 1, torch.bfloat16: 2}
RPT_PROJ_MFMA, RPT_KNN_DEDUP = 2, 1
SAMPLE = 1000


def rows_of(name, dev):
    n, d, dt, T, minl, k, seed = SHAPES[name]
    if name == "c2":
        X = gen.normal_dense2_torch(seed, n, d, dev)
    else:
        g = torch.Generator(device=dev).manual_seed(seed)
        X = torch.empty((n, d), dtype=dt, device=dev)
        for lo in range(0, n, 1_000_000):
            X[lo:lo + 1_000_000] = torch.randn(min(1_000_000, n - lo), d, device=dev, dtype=torch.float32,
                                               generator=g).to(dt)
    torch.cuda.synchronize(dev)
    return X


def cfg_of(name):
    import math
    n, d, dt, T, minl, k, seed = SHAPES[name]
    maxd = math.ceil(math.log(n / minl) / math.log(2.0))            # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(d) / math.log(10.0)), 1.0)
    return maxd, pnz


def event_ms(stream, fn, reps):
    """median HIP-event time of fn() on the ctx stream, behind one warm-up"""
    s = torch.cuda.ExternalStream(stream)
    fn()
    s.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts


def sample_ids(n):
    return np.sort(np.random.default_rng(7).choice(n, SAMPLE, replace=False)).astype(np.int64)


# ------------------------------------------------------------------ the comparator (child process)
def child(name, reps, out_path):
    """raw ctypes on the library RPTREE_HIP_LIB names: the parent commit's build"""
    L = C.CDLL(os.environ["RPTREE_HIP_LIB"])
    vp = C.c_void_p

    def call(fn, *a):
        f = getattr(L, fn)
        f.restype = C.c_int32
        if f(*a) != 0:
            L.rpt_last_error.restype = C.c_char_p
            raise SystemExit("%s: %s" % (fn, L.rpt_last_error().decode()))

    n, d, dt, T, minl, k, seed = SHAPES[name]
    maxd, pnz = cfg_of(name)
    dev = torch.device("cuda", 0)
    X = rows_of(name, dev)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, d)
    R = np.ascontiguousarray(R, dtype=np.float64)
    ctx, ds, f, stream = vp(), vp(), vp(), vp()
    call("rpt_ctx_create", C.c_int32(0), C.byref(ctx))
    call("rpt_ctx_stream", ctx, C.byref(stream))
    call("rpt_dataset_dense_dev", ctx, vp(X.data_ptr()), C.c_int64(n), C.c_int32(d), C.c_int32(RPT_DT[dt]),
         C.byref(ds))
    call("rpt_forest_build", ctx, ds, vp(R.ctypes.data), C.c_int32(T), C.c_int32(maxd), C.c_int32(minl),
         C.c_int32(RPT_PROJ_MFMA), C.byref(f))
    perm = np.empty((T, n), dtype=np.int32)
    call("rpt_forest_get_perm", f, vp(perm.ctypes.data))
    ids = torch.empty((n, k + 1), dtype=torch.int32, device=dev)
    dist = torch.empty((n, k + 1), dtype=torch.float64, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)

    def once():
        call("rpt_knn_dev", ctx, f, ds, ds, C.c_int32(k + 1), C.c_int32(RPT_KNN_DEDUP), vp(ids.data_ptr()),
             vp(dist.data_ptr()), vp(cnt.data_ptr()))

    ms, all_ms = event_ms(stream.value, once, reps)
    call("rpt_ctx_sync", ctx)
    cand = C.c_int64()
    call("rpt_knn_last_candidates", ctx, C.byref(cand))
    np.save(out_path, ids[torch.from_numpy(sample_ids(n)).to(dev)].cpu().numpy())
    print(json.dumps({"ms": ms, "all_ms": all_ms, "candidates": int(cand.value),
                      "perm_crc": zlib.crc32(perm.tobytes())}))


# ------------------------------------------------------------------ the graph (this build)
def leg(name, reps, parent_lib):
    import rptree_amd as rp
    from rptree_amd import _lib
    n, d, dt, T, minl, k, seed = SHAPES[name]
    maxd, pnz = cfg_of(name)
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    X = rows_of(name, dev)
    ds = rp.Dataset.from_torch(ctx, X)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, d)
    f = rp._build(ctx, ds, R, maxd, minl, rp.RPT_PROJ_MFMA)
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    dist = torch.empty((n, k), dtype=torch.float64, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    once = lambda: rp.knnGraphDev(k, f, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())  # noqa: E731
    ms_a, all_a = event_ms(ctx.stream, once, reps)
    ctx.sync()
    pairs = rp.knnGraphLastPairs(ctx)
    leaves = [int(s) for (_, _, _, s, leaf) in f.topology() if leaf]
    esize = X.element_size()
    out = {"workload": "%s: %d x %d %s, %d trees, minLeaf %d, maxDepth %d, k = %d, leaves of %d..%d points" %
                       (name, n, d, str(dt).split(".")[1], T, minl, maxd, k, min(leaves), max(leaves)),
           "kernel": "graph_tiled_kernel" if max(leaves) > 128 else "graph_leaf_kernel",
           "pairs": pairs, "pair_ops": pairs * d * 3,
           "model_bytes_graph": T * n * d * esize + 2 * T * n * k * 12}
    sel = sample_ids(n)
    truth, _ = rp.bruteKnn(ds, rp.Dataset.from_torch(ctx, X[torch.from_numpy(sel).to(dev)].contiguous()), k + 1)
    truth = [[j for j in row if j != i][:k] for i, row in zip(sel.tolist(), truth.tolist())]

    def recall(rows):
        return float(np.mean([len(set(t) & set(r)) / k for t, r in zip(truth, rows)]))

    got = ids[torch.from_numpy(sel).to(dev)].cpu().numpy()
    out["recall_graph"] = recall([[j for j in r if j >= 0] for r in got.tolist()])
    if parent_lib:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "self_ids.npy")
            env = dict(os.environ, RPTREE_HIP_LIB=os.path.abspath(parent_lib))
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(reps), path],
                                env=env, capture_output=True, text=True, timeout=900)
            if pr.returncode != 0:
                raise SystemExit("comparator failed:\n" + pr.stdout + pr.stderr)
            comp = json.loads(pr.stdout.strip().splitlines()[-1])
            self_ids = np.load(path)
        if comp["perm_crc"] != zlib.crc32(f.perm.tobytes()):
            raise SystemExit("the comparator's forest differs from this build's")
        out["recall_self_query"] = recall([[j for j in r if j != i and j >= 0][:k]
                                           for i, r in zip(sel.tolist(), self_ids.tolist())])
        out["self_query_ms"], out["self_query_all_ms"] = comp["ms"], comp["all_ms"]
        out["self_query_candidates"] = comp["candidates"]
        out["model_bytes_self_query"] = comp["candidates"] * d * esize
        out["self_query_library"] = "the parent commit's build, loaded through RPTREE_HIP_LIB in a child process"
    ms_b, all_b = event_ms(ctx.stream, once, reps)           # again, behind the comparator
    ctx.sync()
    out["graph_ms"] = min(ms_a, ms_b)
    out["graph_ms_before"], out["graph_ms_after"] = ms_a, ms_b
    out["graph_all_ms"] = all_a + all_b
    out["graph_pair_ops_per_s"] = out["pair_ops"] / (out["graph_ms"] * 1e-3)
    if parent_lib:
        out["speedup"] = out["self_query_ms"] / max(ms_a, ms_b)  # the slower graph series
    _lib.check(_lib.lib().rpt_ctx_trim(ctx._h))
    f.close()
    ds.close()
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    parent, out_path = None, os.path.join(ROOT, "profiles", "knn_graph_times.json")
    if "--parent-lib" in sys.argv:
        parent = sys.argv[sys.argv.index("--parent-lib") + 1]
        args.remove(parent)
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args.remove(out_path)
    names = (args[0] if args else "c2").split(",")
    reps = int(args[1]) if len(args) > 1 else 5
    res = {"tool": "tools/knn_graph_times.py", "reps": reps, "timing": "HIP events on the ctx stream, median",
           "legs": [leg(nm, reps, parent) for nm in names]}
    line = json.dumps(res)
    print(line)
    if parent:                      # without the comparator nothing is recorded
        with open(out_path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
