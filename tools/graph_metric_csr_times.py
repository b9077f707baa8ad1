"""Graph search and graph preparation on SVector (CSR) rows under the cosine and inner-product
distances (rpt_graph_search_csr_metric_dev, rpt_graph_prepare_csr_metric_dev; csrc/graph_search_csr.hip,
csrc/graph_prepare.hip) at the C3 shape: 1 M x 784, density 0.19, U(0,1] values, 32 trees, minLeaf 128,
k = 10, 10 000 queries of the same kind.

    python tools/graph_metric_csr_times.py [reps] --parent-lib PATH [--out FILE] [--n N]
                                           [--metrics cosine,inner] [--no-l2]

Steps, each a fresh child process under a time limit of its own (a step that fails or runs out of time
ends the run; nothing is recorded then).  Per distance:
  csr     this build: the truth (bruteKnn(metric=) on the CSR rows), the forest query
          rpt_knn_csr_metric_dev over all 32 trees with RPT_KNN_DEDUP, the graph (knnGraphMetricSV of the
          32 trees + 2 knnGraphRefineMetricSV rounds), the seeds (rpt_knn_csr_metric_dev on the first 2
          trees, 8 nearest, de-duplicated), rpt_graph_search_csr_metric_dev at ef = 16 / 32 / 64 / 128,
          resident queries and again with graph_search_csr_stream = 1, and
          rpt_graph_prepare_csr_metric_dev as diversify (kout 10) / reverse (kout 20) / both (kout 20),
          each again with graph_prepare_csr_resident = -1, with the search on each prepared graph
  parent  the library built from the parent commit (PATH, loaded through RPTREE_HIP_LIB): its only device
          route for these queries without a dense copy, rpt_knn_csr_metric_dev over all 32 trees with
          RPT_KNN_DEDUP
  dense   this build: rpt_graph_search_dev(metric) and rpt_graph_prepare_dev(metric) on the dense-ified
          rows (6.3 GB more) and queries with the graph and the seeds of the csr step
and once, unless --no-l2:
  l2      rpt_graph_search_csr_dev and rpt_graph_prepare_csr_dev under L2 through raw ctypes on this
          build's library and, in a second child, on the parent commit's: same rows, same forest, the
          graph each library builds itself (rpt_knn_graph_csr_dev + 2 rounds), same seeds.  The
          templates must not cost the L2 kernels anything: the answers' checksums must agree and the two
          timings are recorded side by side with all their repetitions
The csr step leaves the truth, the graph and the seeds in a scratch directory for the dense step.  All
steps draw the same rows, queries and hyperplanes; the forests must report the same perm checksum, and
the dense entry points must report the checksums of the CSR answers (finite values: bit-equal).
Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  Writes (or, for a subset of the
metrics, updates) profiles/graph_metric_csr_times.json.  No ratio is fixed in advance: the file holds
what was measured.
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
PREP_EF = 32
RPT_F64, RPT_PROJ_AUTO, RPT_KNN_DEDUP = 0, 0, 1
METRIC_BIT = {"cosine": 1 << 25, "inner": 1 << 26}
CONFIGS = {"diversify": (True, False, 10), "reverse": (False, True, 20), "both": (True, True, 20)}
STEP_LIMIT_S = {"csr": 420, "parent": 300, "dense": 420, "l2": 420}


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
    return (torch.empty((NQ, K), dtype=torch.int32, device=dev), torch.empty((NQ, K), dtype=torch.float64, device=dev),
            torch.empty((NQ,), dtype=torch.int32, device=dev))


def graph_outputs(dev, n, k):
    return (torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.float64, device=dev),
            torch.empty((n,), dtype=torch.int32, device=dev))


def distf_of(rp, metric):
    return {"cosine": rp.metricCosine, "inner": rp.metricInner}[metric]


# ------------------------------------------------------------------ this build, the CSR rows
def step_csr(n, reps, scratch, metric):
    import rptree_amd as rp
    from rptree_amd import _lib
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    distf, bit = distf_of(rp, metric), METRIC_BIT[metric]
    rowptr, col, val = sparse_uniform_device(dev, n, D, DENSITY, SEED)
    qptr, qcol, qval = sparse_uniform_device(dev, NQ, D, DENSITY, SEED + 1)
    ds = rp.Dataset.csr_from_torch(ctx, rowptr, col, val, D)
    qd = rp.Dataset.csr_from_torch(ctx, qptr, qcol, qval, D)
    maxd, pnz = cfg_of(n)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, D)
    truth, _ = rp.bruteKnn(ds, qd, K, metric=distf)
    ids, dist, cnt = outputs(dev)
    torch.cuda.synchronize(dev)
    L, vp = _lib.lib(), _lib.vp

    def knn_dev(forest, k, o_ids, o_dist, o_cnt):
        _lib.check(L.rpt_knn_csr_metric_dev(ctx._h, forest._h, ds._h, qd._h, k, RPT_KNN_DEDUP | bit,
                                            vp(o_ids.data_ptr()), vp(o_dist.data_ptr()), vp(o_cnt.data_ptr())))

    f = rp._build(ctx, ds, R, maxd, MINL, RPT_PROJ_AUTO)
    perm_crc = zlib.crc32(f.perm.tobytes())
    knn_ms, knn_all = event_ms(ctx.stream, lambda: knn_dev(f, K, ids, dist, cnt), reps)
    ctx.sync()
    knn_recall = recall_of(ids.cpu().numpy(), truth)

    # the graph: the 32-tree forest's, two NN-descent rounds, under the same distance
    gids, gdist, gcnt = graph_outputs(dev, n, KG)
    torch.cuda.synchronize(dev)
    rp.knnGraphMetricSVDev(distf, KG, f, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr())
    rp.knnGraphRefineMetricSVDev(distf, KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), iters=2)
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
    for name, t in (("gids", gids), ("gdist", gdist), ("gcnt", gcnt), ("seeds", seeds)):
        np.save(os.path.join(scratch, name + ".npy"), t.cpu().numpy())

    def search_rows(kg, g_ids, g_cnt, efs, streamed):
        rows = []
        for ef in efs:
            def run():
                rp.graphSearchMetricSVDev(distf, ds, qd, kg, g_ids.data_ptr(), g_cnt.data_ptr(), SEED_K,
                                          seeds.data_ptr(), K, ef, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            ms, all_ms = event_ms(ctx.stream, run, reps)
            ctx.sync()
            expansions, evaluated = rp.graphSearchLast(ctx)
            crc = answer_crc(ids, dist, cnt)
            row = {"ef": ef, "ms": ms, "all_ms": all_ms, "seeds_plus_search_ms": seed_ms + ms,
                   "recall_at_10": recall_of(ids.cpu().numpy(), truth), "evaluated_per_query": evaluated / NQ,
                   "expansions_per_query": expansions / NQ, "crc": crc}
            if streamed:
                old = ctx.set_option("graph_search_csr_stream", 1)
                try:
                    row["streamed_ms"], row["streamed_all_ms"] = event_ms(ctx.stream, run, reps)
                    ctx.sync()
                finally:
                    ctx.set_option("graph_search_csr_stream", old)
                if answer_crc(ids, dist, cnt) != crc or rp.graphSearchLast(ctx)[0] != expansions:
                    raise SystemExit("graph_search_csr_stream changed the answer at ef %d" % ef)
            rows.append(row)
        return rows

    res = {"n": n, "nnz": int(val.numel()), "query_nnz": int(qval.numel()), "maxDepth": maxd, "perm_crc": perm_crc,
           "knn": {"ms": knn_ms, "all_ms": knn_all, "recall_at_10": knn_recall},
           "seeds": {"trees": SEED_TREES, "seed_k": SEED_K, "ms": seed_ms, "all_ms": seed_all,
                     "recall_at_10_of_the_seeds": seed_recall},
           "search": search_rows(KG, gids, gcnt, EFS, True), "prepare": {}}
    for name, (div, rev, kout) in CONFIGS.items():
        oi, od, oc = graph_outputs(dev, n, kout)
        torch.cuda.synchronize(dev)

        def run():
            rp.graphPrepareMetricSVDev(distf, KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), kout,
                                       oi.data_ptr(), od.data_ptr(), oc.data_ptr(), diversify=div, reverse=rev)
        row = {"kout": kout}
        for tag, setting in (("resident", 0), ("global", -1)):
            old = ctx.set_option("graph_prepare_csr_resident", setting)
            try:
                ms, all_ms = event_ms(ctx.stream, run, reps)
                ctx.sync()
            finally:
                ctx.set_option("graph_prepare_csr_resident", old)
            stats, crc = list(rp.graphPrepareLast(ctx)), answer_crc(oi, od, oc)
            if tag == "global" and (crc != row["crc"] or stats != row["stats"]):
                raise SystemExit("graph_prepare_csr_resident = -1 changed the answer of %s" % name)
            row.update({tag + "_ms": ms, tag + "_all_ms": all_ms, "crc": crc, "stats": stats})
        row["mean_degree"] = float(oc.double().mean())
        row["search"] = search_rows(kout, oi, oc, (PREP_EF,), False)
        res["prepare"][name] = row
    return res


# ------------------------------------------------------------------ this build, the dense-ified rows
def step_dense(n, reps, scratch, metric):
    import rptree_amd as rp
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    distf = distf_of(rp, metric)
    rowptr, col, val = sparse_uniform_device(dev, n, D, DENSITY, SEED)
    X = densify_device(dev, n, rowptr, col, val)
    del rowptr, col, val
    qptr, qcol, qval = sparse_uniform_device(dev, NQ, D, DENSITY, SEED + 1)
    Q = densify_device(dev, NQ, qptr, qcol, qval)
    torch.cuda.synchronize(dev)
    ds, qd = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, Q)
    gids, gdist, gcnt, seeds = (torch.from_numpy(np.load(os.path.join(scratch, name + ".npy"))).to(dev)
                                for name in ("gids", "gdist", "gcnt", "seeds"))
    ids, dist, cnt = outputs(dev)
    torch.cuda.synchronize(dev)
    rows = []
    for ef in EFS:
        def run():
            rp.graphSearchDev(ds, qd, KG, gids.data_ptr(), gcnt.data_ptr(), SEED_K, seeds.data_ptr(), K, ef,
                              ids.data_ptr(), dist.data_ptr(), cnt.data_ptr(), metric=distf)
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        expansions, evaluated = rp.graphSearchLast(ctx)
        rows.append({"ef": ef, "ms": ms, "all_ms": all_ms, "evaluated_per_query": evaluated / NQ,
                     "expansions_per_query": expansions / NQ, "crc": answer_crc(ids, dist, cnt)})
    prep = {}
    for name, (div, rev, kout) in CONFIGS.items():
        oi, od, oc = graph_outputs(dev, n, kout)
        torch.cuda.synchronize(dev)

        def run():
            rp.graphPrepareDev(KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), kout, oi.data_ptr(),
                               od.data_ptr(), oc.data_ptr(), diversify=div, reverse=rev, metric=distf)
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        prep[name] = {"ms": ms, "all_ms": all_ms, "crc": answer_crc(oi, od, oc), "stats": list(rp.graphPrepareLast(ctx))}
    return {"search": rows, "prepare": prep}


# ------------------------------------------------------------------ raw ctypes on the library RPTREE_HIP_LIB names
class Raw:
    def __init__(self, n):
        self.L = C.CDLL(os.environ["RPTREE_HIP_LIB"])
        self.n = n
        vp = C.c_void_p
        self.dev = torch.device("cuda", 0)
        self.rowptr, self.col, self.val = sparse_uniform_device(self.dev, n, D, DENSITY, SEED)
        self.qptr, self.qcol, self.qval = sparse_uniform_device(self.dev, NQ, D, DENSITY, SEED + 1)
        self.maxd, pnz = cfg_of(n)
        _, R = gen.forest_hyperplanes(1235137, T, self.maxd, pnz, D)
        self.R = np.ascontiguousarray(R, dtype=np.float64)
        self.ctx, self.ds, self.qd, self.stream = vp(), vp(), vp(), vp()
        self.call("rpt_ctx_create", C.c_int32(0), C.byref(self.ctx))
        self.call("rpt_ctx_stream", self.ctx, C.byref(self.stream))
        torch.cuda.synchronize(self.dev)
        self.call("rpt_dataset_csr_dev", self.ctx, vp(self.rowptr.data_ptr()), vp(self.col.data_ptr()),
                  vp(self.val.data_ptr()), C.c_int64(n), C.c_int32(D), C.c_int32(RPT_F64), C.c_int64(self.val.numel()),
                  C.byref(self.ds))
        self.call("rpt_dataset_csr_dev", self.ctx, vp(self.qptr.data_ptr()), vp(self.qcol.data_ptr()),
                  vp(self.qval.data_ptr()), C.c_int64(NQ), C.c_int32(D), C.c_int32(RPT_F64),
                  C.c_int64(self.qval.numel()), C.byref(self.qd))

    def call(self, fn, *a):
        f = getattr(self.L, fn)
        f.restype = C.c_int32
        if f(*a) != 0:
            self.L.rpt_last_error.restype = C.c_char_p
            raise SystemExit("%s: %s" % (fn, self.L.rpt_last_error().decode()))

    def forest(self, trees):
        f = C.c_void_p()
        self.call("rpt_forest_build", self.ctx, self.ds, C.c_void_p(self.R.ctypes.data), C.c_int32(trees),
                  C.c_int32(self.maxd), C.c_int32(MINL), C.c_int32(RPT_PROJ_AUTO), C.byref(f))
        return f


def step_parent(n, reps, scratch, metric):
    r = Raw(n)
    vp = C.c_void_p
    f = r.forest(T)
    perm = np.empty((T, n), dtype=np.int32)
    r.call("rpt_forest_get_perm", f, vp(perm.ctypes.data))
    ids, dist, cnt = outputs(r.dev)
    torch.cuda.synchronize(r.dev)

    def once():
        r.call("rpt_knn_csr_metric_dev", r.ctx, f, r.ds, r.qd, C.c_int32(K), C.c_int32(RPT_KNN_DEDUP | METRIC_BIT[metric]),
               vp(ids.data_ptr()), vp(dist.data_ptr()), vp(cnt.data_ptr()))

    ms, all_ms = event_ms(r.stream.value, once, reps)
    r.call("rpt_ctx_sync", r.ctx)
    truth = np.load(os.path.join(scratch, "truth.npy"))
    return {"perm_crc": zlib.crc32(perm.tobytes()), "ms": ms, "all_ms": all_ms,
            "recall_at_10": recall_of(ids.cpu().numpy(), truth)}


def step_l2(n, reps, scratch, metric):
    """the L2 entry points of the library RPTREE_HIP_LIB names: graph, seeds, search sweep, preparation"""
    r = Raw(n)
    vp, i32 = C.c_void_p, C.c_int32
    f = r.forest(T)
    perm = np.empty((T, n), dtype=np.int32)
    r.call("rpt_forest_get_perm", f, vp(perm.ctypes.data))
    gids, gdist, gcnt = graph_outputs(r.dev, n, KG)
    torch.cuda.synchronize(r.dev)
    r.call("rpt_knn_graph_csr_dev", r.ctx, f, r.ds, i32(KG), i32(0), vp(gids.data_ptr()), vp(gdist.data_ptr()),
           vp(gcnt.data_ptr()))
    r.call("rpt_knn_graph_refine_csr_dev", r.ctx, r.ds, i32(KG), i32(KG), i32(2), i32(0), vp(gids.data_ptr()),
           vp(gdist.data_ptr()), vp(gcnt.data_ptr()))
    r.call("rpt_ctx_sync", r.ctx)
    r.call("rpt_forest_free", f)
    f2 = r.forest(SEED_TREES)
    sids = torch.empty((NQ, SEED_K), dtype=torch.int32, device=r.dev)
    sdist = torch.empty((NQ, SEED_K), dtype=torch.float64, device=r.dev)
    scnt = torch.empty((NQ,), dtype=torch.int32, device=r.dev)
    torch.cuda.synchronize(r.dev)
    r.call("rpt_knn_dev", r.ctx, f2, r.ds, r.qd, i32(SEED_K), i32(RPT_KNN_DEDUP), vp(sids.data_ptr()),
           vp(sdist.data_ptr()), vp(scnt.data_ptr()))
    r.call("rpt_ctx_sync", r.ctx)
    seeds = torch.where(torch.arange(SEED_K, device=r.dev)[None, :] < scnt[:, None], sids,
                        torch.full_like(sids, -1)).contiguous()
    ids, dist, cnt = outputs(r.dev)
    torch.cuda.synchronize(r.dev)
    res = {"perm_crc": zlib.crc32(perm.tobytes()), "graph_crc": answer_crc(gids, gdist, gcnt), "search": [], "prepare": {}}
    for ef in EFS:
        def run():
            r.call("rpt_graph_search_csr_dev", r.ctx, r.ds, r.qd, i32(KG), vp(gids.data_ptr()), vp(gcnt.data_ptr()),
                   i32(SEED_K), vp(seeds.data_ptr()), i32(K), i32(ef), i32(0), i32(0), vp(ids.data_ptr()),
                   vp(dist.data_ptr()), vp(cnt.data_ptr()))
        ms, all_ms = event_ms(r.stream.value, run, reps)
        r.call("rpt_ctx_sync", r.ctx)
        res["search"].append({"ef": ef, "ms": ms, "all_ms": all_ms, "crc": answer_crc(ids, dist, cnt)})
    for name, (div, rev, kout) in CONFIGS.items():
        oi, od, oc = graph_outputs(r.dev, n, kout)
        torch.cuda.synchronize(r.dev)

        def run():
            r.call("rpt_graph_prepare_csr_dev", r.ctx, r.ds, i32(KG), vp(gids.data_ptr()), vp(gdist.data_ptr()),
                   vp(gcnt.data_ptr()), i32(kout), i32(0), i32((1 if div else 0) | (2 if rev else 0)),
                   vp(oi.data_ptr()), vp(od.data_ptr()), vp(oc.data_ptr()))
        ms, all_ms = event_ms(r.stream.value, run, reps)
        r.call("rpt_ctx_sync", r.ctx)
        res["prepare"][name] = {"kout": kout, "ms": ms, "all_ms": all_ms, "crc": answer_crc(oi, od, oc)}
    return res


def run_step(name, n, reps, lib, scratch, metric):
    env = dict(os.environ)
    if lib:
        env["RPTREE_HIP_LIB"] = os.path.abspath(lib)
    limit = STEP_LIMIT_S[name]                              # the step ends at its own limit, whatever this process does
    pr = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                         str(n), str(reps), scratch, metric], env=env, capture_output=True, text=True)
    if pr.returncode in (124, 137):
        raise SystemExit("step %s (%s) ran out of its %d s: nothing recorded" % (name, metric, limit))
    if pr.returncode != 0:
        raise SystemExit("step %s (%s) failed (%d): nothing recorded\n%s%s" % (name, metric, pr.returncode, pr.stdout,
                                                                               pr.stderr))
    print("step %s (%s) done" % (name, metric), file=sys.stderr, flush=True)
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, n, reps, scratch, metric = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
        step = {"csr": step_csr, "dense": step_dense, "parent": step_parent, "l2": step_l2}[name]
        print(json.dumps(step(n, reps, scratch, metric)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    parent = opt("--parent-lib", None)
    out_path = opt("--out", os.path.join(ROOT, "profiles", "graph_metric_csr_times.json"))
    n = int(opt("--n", 1_000_000))
    metrics = [m for m in opt("--metrics", "cosine,inner").split(",") if m]
    no_l2 = "--no-l2" in args
    if no_l2:
        args.remove("--no-l2")
    reps = int(args[0]) if args else 5
    if not parent:
        raise SystemExit("--parent-lib PATH is required: the comparison is to the parent commit's library")
    this_lib = os.environ.get("RPTREE_HIP_LIB") or os.path.join(ROOT, "rp-tree_amd", "librptree_hip.so")
    res = {}
    if os.path.exists(out_path):                            # a run over a subset of the metrics keeps the rest
        with open(out_path) as fh:
            res = json.load(fh)
        if res.get("n") != n or res.get("reps") != reps:
            res = {}
    res.update({"tool": "tools/graph_metric_csr_times.py", "reps": reps, "n": n,
                "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step"})
    for metric in metrics:                                  # a step that fails raises: nothing further starts
        scratch = tempfile.mkdtemp(prefix="graph_metric_csr_")
        try:
            csr = run_step("csr", n, reps, None, scratch, metric)
            par = run_step("parent", n, reps, parent, scratch, metric)
            den = run_step("dense", n, reps, None, scratch, metric)
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
        if csr["perm_crc"] != par["perm_crc"]:
            raise SystemExit("the steps built different forests")
        for a, b in zip(csr["search"], den["search"]):
            if a["crc"] != b["crc"] or a["expansions_per_query"] != b["expansions_per_query"]:
                raise SystemExit("%s, ef %d: the CSR and the dense-ified answers differ" % (metric, a["ef"]))
            a["dense_ms"], a["dense_all_ms"] = b["ms"], b["all_ms"]
        for name, row in csr["prepare"].items():
            b = den["prepare"][name]
            if row["crc"] != b["crc"] or row["stats"] != b["stats"]:
                raise SystemExit("%s, %s: the CSR and the dense-ified prepared graphs differ" % (metric, name))
            row["dense_ms"], row["dense_all_ms"] = b["ms"], b["all_ms"]
        res["workload"] = ("C3: %d x %d CSR f64, density %.2f (%d nonzeros), %d queries of the same kind (%d nonzeros), "
                           "minLeaf %d, maxDepth %d, k = %d, graph = knnGraphMetricSV(%d trees, k = %d) + 2 refinement "
                           "rounds under the same distance, seeds = %d nearest de-duplicated candidates of %d trees"
                           % (n, D, DENSITY, csr["nnz"], NQ, csr["query_nnz"], MINL, csr["maxDepth"], K, T, KG, SEED_K,
                              SEED_TREES))
        res[metric] = {"seeds": csr["seeds"], "search": csr["search"], "prepare": csr["prepare"],
                       "bit_equal": "at every ef and for every preparation the dense entry point under the same metric "
                                    "gave the checksum (and the statistics) of the CSR entry point's answer, and so did "
                                    "graph_search_csr_stream = 1 and graph_prepare_csr_resident = -1",
                       "knn_dedup_32_trees": [dict(csr["knn"], library="this build"),
                                              {"library": "the parent commit's build, loaded through RPTREE_HIP_LIB in "
                                                          "a child process", "ms": par["ms"], "all_ms": par["all_ms"],
                                               "recall_at_10": par["recall_at_10"]}]}
    if not no_l2:
        scratch = tempfile.mkdtemp(prefix="graph_metric_csr_")
        try:
            mine = run_step("l2", n, reps, this_lib, scratch, "l2")
            theirs = run_step("l2", n, reps, parent, scratch, "l2")
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
        if mine["perm_crc"] != theirs["perm_crc"] or mine["graph_crc"] != theirs["graph_crc"]:
            raise SystemExit("the two libraries built different forests or L2 graphs")
        rows = []
        for a, b in zip(mine["search"], theirs["search"]):
            if a["crc"] != b["crc"]:
                raise SystemExit("L2, ef %d: this build's and the parent's answers differ" % a["ef"])
            rows.append({"entry": "rpt_graph_search_csr_dev", "ef": a["ef"], "this_ms": a["ms"], "this_all_ms": a["all_ms"],
                         "parent_ms": b["ms"], "parent_all_ms": b["all_ms"]})
        for name, a in mine["prepare"].items():
            b = theirs["prepare"][name]
            if a["crc"] != b["crc"]:
                raise SystemExit("L2, %s: this build's and the parent's prepared graphs differ" % name)
            rows.append({"entry": "rpt_graph_prepare_csr_dev", "config": name, "kout": a["kout"], "this_ms": a["ms"],
                         "this_all_ms": a["all_ms"], "parent_ms": b["ms"], "parent_all_ms": b["all_ms"]})
        res["l2_entry_points"] = rows
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
