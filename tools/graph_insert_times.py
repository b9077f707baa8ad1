"""New rows into a kNN graph (rpt_graph_insert_dev; csrc/graph_insert.hip) at C2: 1 M x 128 f64, minLeaf
128, k = 10.  The graph is knnGraph of 32 trees + 2 knnGraphRefine rounds over the first 90 % of the
rows; the last 10 % are inserted with seeds = the 8 nearest de-duplicated candidates of 2 trees of the
old rows' forest.

    python tools/graph_insert_times.py [reps] --parent-lib PATH [--out FILE] [--n N]

Steps, each a fresh child process under a time limit of its own (a step that fails or runs out of time
ends the run; nothing is recorded then):
  insert   this build: the old graph, the seeds, then rpt_graph_insert_dev at ef = 32 with batch 1024 /
           4096 / 16384 / m: ms, chunks / evaluated / offered / accepted, and from one profiled call
           (rpt_prof_*) the time of the link kernels (class 6) beside the searches (class 3).  The graph
           grown at batch 4096 is left in a scratch directory
  rebuild  the only route there was, through raw ctypes on the library RPTREE_HIP_LIB names, run on the
           parent commit's library (PATH) and on this build's: forest build (32 trees) +
           rpt_knn_graph_dev + 2 rpt_knn_graph_refine_dev rounds over ALL rows, each timed on its own.
           The parent's rebuilt graph is left in the scratch directory
  quality  this build: 10 000 queries, the exact answer (rpt_brute_knn_dev over all rows), and
           rpt_graph_search_dev at ef = 32 from the same seeds (8 nearest de-duplicated candidates of 2
           trees over the OLD rows) on the grown graph and on the rebuilt one: recall@10 overall and
           among the true neighbours that are new rows
Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  Writes
profiles/graph_insert_times.json.  No ratio is fixed in advance: the file holds what was measured.
--n N shrinks the data set (a rehearsal)."""
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

D, MINL, K, KG, SEED, NQ, TREES, SEED_TREES, SEED_K, ROUNDS = 128, 128, 10, 10, 1234, 10_000, 32, 2, 8, 2
EF = 32
KEEP_BATCH = 4096
RPT_F64, RPT_PROJ_MFMA, RPT_KNN_DEDUP = 0, 2, 1
STEP_LIMIT_S = {"insert": 540, "rebuild": 300, "quality": 420}


def batches(m):
    return sorted({min(b, m) for b in (1024, 4096, 16384, m)})


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


def shape(n):
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))           # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    return maxd, pnz


def triple(dev, rows, k):
    return (torch.empty((rows, k), dtype=torch.int32, device=dev), torch.empty((rows, k), dtype=torch.float64, device=dev),
            torch.empty((rows,), dtype=torch.int32, device=dev))


def graph_crc(ids, dist, cnt):
    return zlib.crc32(cnt.cpu().numpy().tobytes(), zlib.crc32(dist.cpu().numpy().tobytes(),
                                                              zlib.crc32(ids.cpu().numpy().tobytes())))


def forest_seeds(rp, _lib, ctx, dev, f2, ds, qd, nq):
    """the 8 nearest de-duplicated candidates of the forest f2 per row of qd, -1 behind the count"""
    sids, sdist, scnt = triple(dev, nq, SEED_K)
    torch.cuda.synchronize(dev)
    L, vp = _lib.lib(), _lib.vp
    _lib.check(L.rpt_knn_dev(ctx._h, f2._h, ds._h, qd._h, SEED_K, rp.RPT_KNN_DEDUP, vp(sids.data_ptr()),
                             vp(sdist.data_ptr()), vp(scnt.data_ptr())))
    ctx.sync()
    seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < scnt[:, None], sids,
                        torch.full_like(sids, -1)).contiguous()
    torch.cuda.synchronize(dev)
    return seeds


# ------------------------------------------------------------------ this build: the old graph, the seeds, the sweep
def step_insert(n, reps, scratch):
    import rptree_amd as rp
    from rptree_amd import _lib
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    m = n // 10
    n0 = n - m
    X = gen.normal_dense2_torch(SEED, n, D, dev)
    torch.cuda.synchronize(dev)
    ds, dold, dnew = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, X[:n0]), rp.Dataset.from_torch(ctx, X[n0:])
    maxd, pnz = shape(n0)
    _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)
    f = rp._build(ctx, dold, R, maxd, MINL, rp.RPT_PROJ_MFMA)
    g0 = triple(dev, n0, KG)
    torch.cuda.synchronize(dev)
    rp.knnGraphDev(KG, f, *(t.data_ptr() for t in g0))
    rp.knnGraphRefineDev(KG, dold, *(t.data_ptr() for t in g0), iters=ROUNDS)
    ctx.sync()
    f.close()
    f2 = rp._build(ctx, dold, R[:SEED_TREES], maxd, MINL, rp.RPT_PROJ_MFMA)
    seeds = forest_seeds(rp, _lib, ctx, dev, f2, dold, dnew, m)
    out = triple(dev, n, KG)
    torch.cuda.synchronize(dev)
    L = _lib.lib()
    rows = []
    for batch in batches(m):
        def run():
            rp.graphInsertDev(ds, KG, g0[0].data_ptr(), g0[1].data_ptr(), g0[2].data_ptr(), m, SEED_K, seeds.data_ptr(),
                              EF, batch, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        chunks, evaluated, offered, accepted = rp.graphInsertLast(ctx)
        _lib.check(L.rpt_prof_reset(ctx._h))
        _lib.check(L.rpt_prof_enable(ctx._h, 1))
        run()
        ctx.sync()
        prof = {}
        for name, which in (("search_ms", 3), ("link_ms", 6)):
            t, c = C.c_double(), C.c_int64()
            _lib.check(L.rpt_prof_get(ctx._h, which, C.byref(t), C.byref(c)))
            prof[name] = t.value
        _lib.check(L.rpt_prof_enable(ctx._h, 0))
        rows.append({"batch": batch, "ef": EF, "ms": ms, "all_ms": all_ms, "chunks": chunks,
                     "evaluated_per_new_row": evaluated / m, "offered": offered, "accepted": accepted,
                     "profiled_call": prof, "link_share_of_profiled": prof["link_ms"] / (prof["link_ms"] + prof["search_ms"]),
                     "mean_count_new": float(out[2][n0:].double().mean()), "crc": graph_crc(*out)})
        if batch == min(KEEP_BATCH, m):
            np.save(os.path.join(scratch, "grown_ids.npy"), out[0].cpu().numpy())
            np.save(os.path.join(scratch, "grown_cnt.npy"), out[2].cpu().numpy())
    return {"n": n, "m": m, "maxDepth_old_rows": maxd, "sweep": rows}


# ------------------------------------------------------------------ raw ctypes on the library RPTREE_HIP_LIB names
def step_rebuild(n, reps, scratch):
    L = C.CDLL(os.environ["RPTREE_HIP_LIB"])
    vp, i32 = C.c_void_p, C.c_int32
    dev = torch.device("cuda", 0)

    def call(fn, *a):
        f = getattr(L, fn)
        f.restype = C.c_int32
        if f(*a) != 0:
            L.rpt_last_error.restype = C.c_char_p
            raise SystemExit("%s: %s" % (fn, L.rpt_last_error().decode()))

    X = gen.normal_dense2_torch(SEED, n, D, dev)
    maxd, pnz = shape(n)
    _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)
    R = np.ascontiguousarray(R, dtype=np.float64)
    ctx, ds, stream = vp(), vp(), vp()
    call("rpt_ctx_create", i32(0), C.byref(ctx))
    call("rpt_ctx_stream", ctx, C.byref(stream))
    torch.cuda.synchronize(dev)
    call("rpt_dataset_dense_dev", ctx, vp(X.data_ptr()), C.c_int64(n), i32(D), i32(RPT_F64), C.byref(ds))
    g = triple(dev, n, KG)
    torch.cuda.synchronize(dev)
    held = {}

    def build():
        if held.get("f"):
            call("rpt_forest_free", held["f"])
        f = vp()
        call("rpt_forest_build", ctx, ds, vp(R.ctypes.data), i32(TREES), i32(maxd), i32(MINL), i32(RPT_PROJ_MFMA), C.byref(f))
        held["f"] = f

    def graph():
        call("rpt_knn_graph_dev", ctx, held["f"], ds, i32(KG), i32(0), vp(g[0].data_ptr()), vp(g[1].data_ptr()),
             vp(g[2].data_ptr()))

    def rounds():
        call("rpt_knn_graph_refine_dev", ctx, ds, i32(KG), i32(KG), i32(ROUNDS), i32(0), vp(g[0].data_ptr()),
             vp(g[1].data_ptr()), vp(g[2].data_ptr()))

    res = {}
    res["forest_build_ms"], res["forest_build_all_ms"] = event_ms(stream.value, build, reps)
    call("rpt_ctx_sync", ctx)
    # the rounds refine in place: every repetition of them follows a fresh rpt_knn_graph_dev
    res["knn_graph_ms"], res["knn_graph_all_ms"] = event_ms(stream.value, graph, reps)
    both_ms, both_all = event_ms(stream.value, lambda: (graph(), rounds()), reps)
    call("rpt_ctx_sync", ctx)
    res["knn_graph_plus_%d_rounds_ms" % ROUNDS], res["knn_graph_plus_rounds_all_ms"] = both_ms, both_all
    res["total_ms"] = res["forest_build_ms"] + both_ms
    res["crc"] = graph_crc(*g)
    np.save(os.path.join(scratch, "rebuilt_ids.npy"), g[0].cpu().numpy())
    np.save(os.path.join(scratch, "rebuilt_cnt.npy"), g[2].cpu().numpy())
    return res


# ------------------------------------------------------------------ this build: what the insertion costs in quality
def step_quality(n, reps, scratch):
    import rptree_amd as rp
    from rptree_amd import _lib
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    m = n // 10
    n0 = n - m
    X = gen.normal_dense2_torch(SEED, n, D, dev)
    Q = gen.normal_dense2_torch(SEED + 1, NQ, D, dev)
    torch.cuda.synchronize(dev)
    ds, dold, qd = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, X[:n0]), rp.Dataset.from_torch(ctx, Q)
    truth, _ = rp.bruteKnn(ds, qd, K)
    maxd, pnz = shape(n0)
    _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)
    f2 = rp._build(ctx, dold, R[:SEED_TREES], maxd, MINL, rp.RPT_PROJ_MFMA)
    seeds = forest_seeds(rp, _lib, ctx, dev, f2, dold, qd, NQ)
    new = truth >= n0
    res = {"true_neighbours_that_are_new_rows": int(new.sum()), "queries": NQ, "ef": EF}
    ids, dist, cnt = triple(dev, NQ, K)
    for name in ("grown", "rebuilt"):
        gids = torch.from_numpy(np.load(os.path.join(scratch, name + "_ids.npy"))).to(dev)
        gcnt = torch.from_numpy(np.load(os.path.join(scratch, name + "_cnt.npy"))).to(dev)
        torch.cuda.synchronize(dev)

        def run():
            rp.graphSearchDev(ds, qd, KG, gids.data_ptr(), gcnt.data_ptr(), SEED_K, seeds.data_ptr(), K, EF,
                              ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        got = ids.cpu().numpy()
        hit = np.array([[t in set(r) for t in tr] for tr, r in zip(truth.tolist(), got.tolist())])
        res[name] = {"search_ms": ms, "search_all_ms": all_ms, "recall_at_10": float(hit.mean()),
                     "recall_at_10_among_new_rows": float(hit[new].mean()) if new.any() else None,
                     "evaluated_per_query": rp.graphSearchLast(ctx)[1] / NQ}
    return res


STEPS = {"insert": step_insert, "rebuild": step_rebuild, "quality": step_quality}


def run_step(name, n, reps, lib, scratch):
    env = dict(os.environ)
    if lib:
        env["RPTREE_HIP_LIB"] = os.path.abspath(lib)
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
        print(json.dumps(STEPS[name](n, reps, scratch)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    parent = opt("--parent-lib", None)
    out_path = opt("--out", os.path.join(ROOT, "profiles", "graph_insert_times.json"))
    n = int(opt("--n", 1_000_000))
    reps = int(args[0]) if args else 5
    if not parent:
        raise SystemExit("--parent-lib PATH is required: the yardstick is the parent commit's rebuild")
    this_lib = os.environ.get("RPTREE_HIP_LIB") or os.path.join(ROOT, "rp-tree_amd", "librptree_hip.so")
    scratch = tempfile.mkdtemp(prefix="graph_insert_")
    try:                                                    # a step that fails raises: nothing further starts
        insert = run_step("insert", n, reps, None, scratch)
        mine = run_step("rebuild", n, reps, this_lib, scratch)
        theirs = run_step("rebuild", n, reps, parent, scratch)          # last: its graph is the one `quality` reads
        quality = run_step("quality", n, reps, None, scratch)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    if mine["crc"] != theirs["crc"]:
        raise SystemExit("this build's and the parent's rebuilt graphs differ")
    res = {"tool": "tools/graph_insert_times.py", "reps": reps, "n": n, "m": insert["m"],
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step",
           "workload": "C2: %d x %d float64, minLeaf %d, k = %d; graph = knnGraph(%d trees) + %d refinement rounds over the "
                       "first %d rows; the last %d rows inserted at ef = %d, seeds = %d nearest de-duplicated candidates of "
                       "%d trees over the old rows"
                       % (n, D, MINL, KG, TREES, ROUNDS, n - insert["m"], insert["m"], EF, SEED_K, SEED_TREES),
           "insert": insert["sweep"],
           "rebuild_all_rows": {"the parent commit's library": theirs, "this build": mine,
                                "one_checksum": "the two rebuilt graphs have one checksum"},
           "quality": quality,
           "note": "C2's rows are i.i.d. normal: they have no neighbourhoods, so the recall columns price the method on "
                   "the hardest case; tests/test_graph_insert_host.py holds the table on rows that have them"}
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
