"""Beam search over the kNN graph on SVector (CSR) rows (rpt_graph_search_csr_dev,
csrc/graph_search_csr.hip) at the C3 shape: 1 M x 784, density 0.19, U(0,1] values, 32 trees,
minLeaf 128, k = 10, 10 000 queries of the same kind.

    python tools/graph_search_csr_times.py [reps] --parent-lib PATH [--out FILE] [--n N]

Three steps, each a fresh child process under a time limit of its own (a step that fails or runs out
of time ends the run; nothing is recorded then):
  csr     this build: the truth (bruteKnn on the CSR rows), rpt_knn_dev over all 32 trees with
          RPT_KNN_DEDUP, the graph (knnGraphSV of the 32 trees + 2 knnGraphRefineSV rounds), the seeds
          (rpt_knn_dev on the first 2 trees, 8 nearest, de-duplicated) and rpt_graph_search_csr_dev at
          ef = 16 / 32 / 64 / 128, resident queries and, once more, with graph_search_csr_stream = 1
  parent  the library built from the parent commit (PATH, loaded through RPTREE_HIP_LIB): its only
          device ANN route for sparse rows, rpt_knn_dev over all 32 trees with RPT_KNN_DEDUP
  dense   this build: rpt_graph_search_dev on the dense-ified rows (6.3 GB more) and queries with the
          graph and the seeds of the csr step
The csr step leaves the truth, the graph and the seeds in a scratch directory for the other two.  All
steps draw the same rows, queries and hyperplanes; the forests must report the same perm checksum,
and the dense search must report the checksums of the CSR search's answers (the contract: bit-equal).
Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  Writes
profiles/graph_search_csr_times.json.  No ratio is fixed in advance: the file holds what was measured.
"""
import ctypes as C
import json
import math
import os
import shutil
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

from rptree_amd import gen  # noqa: E402  (no library call: the parent's library lacks the new symbols)

D, DENSITY, T, MINL, K, KG, SEED, NQ, SEED_TREES, SEED_K = 784, 0.19, 32, 128, 10, 10, 1234, 10_000, 2, 8
EFS = (16, 32, 64, 128)
RPT_F64, RPT_PROJ_AUTO, RPT_KNN_DEDUP = 0, 0, 1
STEP_LIMIT_S = {"csr": 400, "parent": 300, "dense": 400}


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


def densify_device(dev, n, rowptr, col, val):
    X = torch.zeros((n, D), dtype=torch.float64, device=dev)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), rowptr[1:] - rowptr[:-1])
    X[rows, col.long()] = val
    return X


def cfg_of(n):
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))            # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    return maxd, pnz


def event_ms(stream, fn, reps):
    """median HIP-event time of fn() on the ctx stream, behind one warm-up"""
    s = torch.cuda.ExternalStream(stream)
    ts = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        if rep:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts


def recall_of(ids, truth):
    return float(np.mean([len(set(t) & set(r)) / K for t, r in zip(truth.tolist(), ids.tolist())]))


def answer_crc(ids, dist, cnt):
    return zlib.crc32(cnt.cpu().numpy().tobytes(), zlib.crc32(dist.cpu().numpy().tobytes(),
                                                              zlib.crc32(ids.cpu().numpy().tobytes())))


def outputs(dev):
    ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    dist = torch.empty((NQ, K), dtype=torch.float64, device=dev)
    cnt = torch.empty((NQ,), dtype=torch.int32, device=dev)
    return ids, dist, cnt


# ------------------------------------------------------------------ this build, the CSR rows
def step_csr(n, reps, scratch):
    import rptree_amd as rp
    from rptree_amd import _lib
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    rowptr, col, val = sparse_uniform_device(dev, n, D, DENSITY, SEED)
    qptr, qcol, qval = sparse_uniform_device(dev, NQ, D, DENSITY, SEED + 1)
    ds = rp.Dataset.csr_from_torch(ctx, rowptr, col, val, D)
    qd = rp.Dataset.csr_from_torch(ctx, qptr, qcol, qval, D)
    maxd, pnz = cfg_of(n)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, D)
    truth, _ = rp.bruteKnn(ds, qd, K)
    ids, dist, cnt = outputs(dev)
    torch.cuda.synchronize(dev)
    L, vp = _lib.lib(), _lib.vp

    def knn_dev(forest, k, o_ids, o_dist, o_cnt):
        _lib.check(L.rpt_knn_dev(ctx._h, forest._h, ds._h, qd._h, k, RPT_KNN_DEDUP, vp(o_ids.data_ptr()),
                                 vp(o_dist.data_ptr()), vp(o_cnt.data_ptr())))

    f = rp._build(ctx, ds, R, maxd, MINL, RPT_PROJ_AUTO)
    perm_crc = zlib.crc32(f.perm.tobytes())
    knn_ms, knn_all = event_ms(ctx.stream, lambda: knn_dev(f, K, ids, dist, cnt), reps)
    ctx.sync()
    knn_recall = recall_of(ids.cpu().numpy(), truth)

    # the graph: the 32-tree forest's, two NN-descent rounds
    gids = torch.empty((n, KG), dtype=torch.int32, device=dev)
    gdist = torch.empty((n, KG), dtype=torch.float64, device=dev)
    gcnt = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.knnGraphSVDev(KG, f, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr())
    rp.knnGraphRefineSVDev(KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), iters=2)
    ctx.sync()
    f.close()

    # the seeds: 8 nearest de-duplicated candidates of the first 2 trees
    f2 = rp._build(ctx, ds, R[:SEED_TREES], maxd, MINL, RPT_PROJ_AUTO)
    sids = torch.empty((NQ, SEED_K), dtype=torch.int32, device=dev)
    sdist = torch.empty((NQ, SEED_K), dtype=torch.float64, device=dev)
    scnt = torch.empty((NQ,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    seed_ms, seed_all = event_ms(ctx.stream, lambda: knn_dev(f2, SEED_K, sids, sdist, scnt), reps)
    ctx.sync()
    seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < scnt[:, None], sids,
                        torch.full_like(sids, -1)).contiguous()
    torch.cuda.synchronize(dev)
    seed_recall = recall_of(sids.cpu().numpy(), truth)
    np.save(os.path.join(scratch, "truth.npy"), truth)
    np.save(os.path.join(scratch, "gids.npy"), gids.cpu().numpy())
    np.save(os.path.join(scratch, "gcnt.npy"), gcnt.cpu().numpy())
    np.save(os.path.join(scratch, "seeds.npy"), seeds.cpu().numpy())

    rows = []
    for ef in EFS:
        def run():
            rp.graphSearchSVDev(ds, qd, KG, gids.data_ptr(), gcnt.data_ptr(), SEED_K, seeds.data_ptr(), K, ef,
                                ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        expansions, evaluated = rp.graphSearchLast(ctx)
        crc = answer_crc(ids, dist, cnt)
        recall = recall_of(ids.cpu().numpy(), truth)
        old = ctx.set_option("graph_search_csr_stream", 1)
        try:
            s_ms, s_all = event_ms(ctx.stream, run, reps)
            ctx.sync()
        finally:
            ctx.set_option("graph_search_csr_stream", old)
        if answer_crc(ids, dist, cnt) != crc or rp.graphSearchLast(ctx)[0] != expansions:
            raise SystemExit("graph_search_csr_stream changed the answer at ef %d" % ef)
        rows.append({"ef": ef, "ms": ms, "all_ms": all_ms, "streamed_ms": s_ms, "streamed_all_ms": s_all,
                     "seeds_plus_search_ms": seed_ms + ms, "recall_at_10": recall,
                     "evaluated_per_query": evaluated / NQ, "expansions_per_query": expansions / NQ, "crc": crc})
    return {"n": n, "nnz": int(val.numel()), "query_nnz": int(qval.numel()), "maxDepth": maxd, "perm_crc": perm_crc,
            "knn": {"ms": knn_ms, "all_ms": knn_all, "recall_at_10": knn_recall},
            "seeds": {"trees": SEED_TREES, "seed_k": SEED_K, "ms": seed_ms, "all_ms": seed_all,
                      "recall_at_10_of_the_seeds": seed_recall},
            "search": rows}


# ------------------------------------------------------------------ this build, the dense-ified rows
def step_dense(n, reps, scratch):
    import rptree_amd as rp
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    rowptr, col, val = sparse_uniform_device(dev, n, D, DENSITY, SEED)
    X = densify_device(dev, n, rowptr, col, val)
    del rowptr, col, val
    qptr, qcol, qval = sparse_uniform_device(dev, NQ, D, DENSITY, SEED + 1)
    Q = densify_device(dev, NQ, qptr, qcol, qval)
    torch.cuda.synchronize(dev)
    ds, qd = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, Q)
    gids, gcnt, seeds = (torch.from_numpy(np.load(os.path.join(scratch, name + ".npy"))).to(dev)
                         for name in ("gids", "gcnt", "seeds"))
    ids, dist, cnt = outputs(dev)
    torch.cuda.synchronize(dev)
    rows = []
    for ef in EFS:
        def run():
            rp.graphSearchDev(ds, qd, KG, gids.data_ptr(), gcnt.data_ptr(), SEED_K, seeds.data_ptr(), K, ef,
                              ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        expansions, evaluated = rp.graphSearchLast(ctx)
        rows.append({"ef": ef, "ms": ms, "all_ms": all_ms, "evaluated_per_query": evaluated / NQ,
                     "expansions_per_query": expansions / NQ, "crc": answer_crc(ids, dist, cnt)})
    return {"search": rows}


# ------------------------------------------------------------------ the parent commit's library
def step_parent(n, reps, scratch):
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
    qptr, qcol, qval = sparse_uniform_device(dev, NQ, D, DENSITY, SEED + 1)
    maxd, pnz = cfg_of(n)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, D)
    R = np.ascontiguousarray(R, dtype=np.float64)
    ctx, ds, qd, f, stream = vp(), vp(), vp(), vp(), vp()
    call("rpt_ctx_create", C.c_int32(0), C.byref(ctx))
    call("rpt_ctx_stream", ctx, C.byref(stream))
    torch.cuda.synchronize(dev)
    call("rpt_dataset_csr_dev", ctx, vp(rowptr.data_ptr()), vp(col.data_ptr()), vp(val.data_ptr()), C.c_int64(n),
         C.c_int32(D), C.c_int32(RPT_F64), C.c_int64(val.numel()), C.byref(ds))
    call("rpt_dataset_csr_dev", ctx, vp(qptr.data_ptr()), vp(qcol.data_ptr()), vp(qval.data_ptr()), C.c_int64(NQ),
         C.c_int32(D), C.c_int32(RPT_F64), C.c_int64(qval.numel()), C.byref(qd))
    call("rpt_forest_build", ctx, ds, vp(R.ctypes.data), C.c_int32(T), C.c_int32(maxd), C.c_int32(MINL),
         C.c_int32(RPT_PROJ_AUTO), C.byref(f))
    perm = np.empty((T, n), dtype=np.int32)
    call("rpt_forest_get_perm", f, vp(perm.ctypes.data))
    ids, dist, cnt = outputs(dev)
    torch.cuda.synchronize(dev)

    def once():
        call("rpt_knn_dev", ctx, f, ds, qd, C.c_int32(K), C.c_int32(RPT_KNN_DEDUP), vp(ids.data_ptr()),
             vp(dist.data_ptr()), vp(cnt.data_ptr()))

    ms, all_ms = event_ms(stream.value, once, reps)
    call("rpt_ctx_sync", ctx)
    truth = np.load(os.path.join(scratch, "truth.npy"))
    return {"perm_crc": zlib.crc32(perm.tobytes()), "ms": ms, "all_ms": all_ms,
            "recall_at_10": recall_of(ids.cpu().numpy(), truth)}


def run_step(name, n, reps, parent_lib, scratch):
    env = dict(os.environ)
    if name == "parent":
        env["RPTREE_HIP_LIB"] = os.path.abspath(parent_lib)
    limit = STEP_LIMIT_S[name]                              # the step ends at its own limit, whatever this process does
    pr = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                         str(n), str(reps), scratch], env=env, capture_output=True, text=True)
    if pr.returncode in (124, 137):
        raise SystemExit("step %s ran out of its %d s: nothing recorded" % (name, limit))
    if pr.returncode != 0:
        raise SystemExit("step %s failed (%d): nothing recorded\n%s%s" % (name, pr.returncode, pr.stdout, pr.stderr))
    print("step %s done" % name, file=sys.stderr, flush=True)
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, n, reps, scratch = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        step = {"csr": step_csr, "dense": step_dense, "parent": step_parent}[name]
        print(json.dumps(step(n, reps, scratch)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    parent = opt("--parent-lib", None)
    out_path = opt("--out", os.path.join(ROOT, "profiles", "graph_search_csr_times.json"))
    n = int(opt("--n", 1_000_000))
    reps = int(args[0]) if args else 5
    if not parent:
        raise SystemExit("--parent-lib PATH is required: the comparison is to the parent commit's library")
    scratch = tempfile.mkdtemp(prefix="graph_search_csr_")
    try:                                                    # a step that fails raises: nothing further starts
        csr = run_step("csr", n, reps, parent, scratch)
        par = run_step("parent", n, reps, parent, scratch)
        den = run_step("dense", n, reps, parent, scratch)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    if csr["perm_crc"] != par["perm_crc"]:
        raise SystemExit("the steps built different forests")
    for a, b in zip(csr["search"], den["search"]):
        if a["crc"] != b["crc"] or a["expansions_per_query"] != b["expansions_per_query"]:
            raise SystemExit("ef %d: the CSR and the dense-ified answers differ" % a["ef"])
        a["dense_ms"], a["dense_all_ms"] = b["ms"], b["all_ms"]
        a["dense_evaluated_per_query"] = b["evaluated_per_query"]
    res = {"tool": "tools/graph_search_csr_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step",
           "workload": "C3: %d x %d CSR f64, density %.2f (%d nonzeros), %d queries of the same kind (%d nonzeros), "
                       "minLeaf %d, maxDepth %d, k = %d, graph = knnGraphSV(%d trees, k = %d) + 2 refinement rounds, "
                       "seeds = %d nearest de-duplicated candidates of %d trees" %
                       (n, D, DENSITY, csr["nnz"], NQ, csr["query_nnz"], MINL, csr["maxDepth"], K, T, KG, SEED_K,
                        SEED_TREES),
           "seeds": csr["seeds"], "search": csr["search"],
           "bit_equal": "at every ef rpt_graph_search_dev on the dense-ified rows and queries gave the checksum of "
                        "rpt_graph_search_csr_dev's answer, and so did graph_search_csr_stream = 1",
           "knn_dedup_32_trees": [dict(csr["knn"], library="this build"),
                                  {"library": "the parent commit's build, loaded through RPTREE_HIP_LIB in a child "
                                              "process", "ms": par["ms"], "all_ms": par["all_ms"],
                                   "recall_at_10": par["recall_at_10"]}]}
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
