"""Rows out of a kNN graph (rpt_graph_delete_dev; csrc/graph_delete.hip) at C2: 1 M x 128 f64, minLeaf
128, k = 10.  The graph is knnGraph of 32 trees + 2 knnGraphRefine rounds over all rows; a random 1 %,
10 % and 50 % of the rows are deleted (np.random.default_rng(7).random(n) < f).

    python tools/graph_delete_times.py [reps] --parent-lib PATH [--out FILE] [--n N]

Steps, each a fresh child process under a time limit of its own (a step that fails or runs out of time
ends the run; nothing is recorded then):
  delete   this build: the graph, then per fraction rpt_graph_delete_dev in old ids and compact: ms,
           kept / touched / evaluated / dropped, distances per touched row, and from one profiled call
           (rpt_prof_*) the time of the delete kernels (class 8); the same call with a bitmap that keeps
           every row runs the mark, scan and copy kernels alone, so what the fractions cost above it is
           the repair kernel's
  rebuild  yardstick (i), the only route to a graph without dead rows there was, through raw ctypes on
           the library RPTREE_HIP_LIB names, run on the parent commit's library (PATH) and on this
           build's: per fraction forest build (32 trees) + rpt_knn_graph_dev + 2 rpt_knn_graph_refine_dev
           rounds over the SURVIVORS
  search   yardstick (ii), living with the dead rows: 10 000 queries, per fraction the exact answer
           among the survivors (rpt_brute_knn_dev over them), rpt_graph_search_allow_dev on the UNREPAIRED
           graph with the keep bitmap at ef = 32 and width 4 ef / 8 ef, and rpt_graph_search_dev at ef = 32
           on the repaired, compacted graph over the compacted rows from the same seeds (8 nearest
           de-duplicated candidates of 2 trees over all rows; a dead seed is -1 on the compacted side):
           ms and recall@10
Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  Writes
profiles/graph_delete_times.json.  No ratio is fixed in advance: the file holds what was measured.
--n N shrinks the data set (a rehearsal)."""
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

D, MINL, K, KG, SEED, NQ, TREES, SEED_TREES, SEED_K, ROUNDS = 128, 128, 10, 10, 1234, 10_000, 32, 2, 8, 2
EF = 32
FRACTIONS = (0.01, 0.1, 0.5)
RPT_F64, RPT_PROJ_MFMA = 0, 2
STEP_LIMIT_S = {"delete": 420, "rebuild": 420, "search": 540}


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


def keep_mask(n, f):
    return ~(np.random.default_rng(7).random(n) < f)


def keep_words(mask):
    bits = np.zeros(((len(mask) + 31) // 32) * 32, dtype=np.uint8)
    bits[:len(mask)] = mask
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.int32)


def full_graph(rp, ctx, dev, ds, n):
    """knnGraph of 32 trees + 2 rounds over all n rows, on the device"""
    maxd, pnz = shape(n)
    _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)
    f = rp._build(ctx, ds, R, maxd, MINL, rp.RPT_PROJ_MFMA)
    g = triple(dev, n, KG)
    torch.cuda.synchronize(dev)
    rp.knnGraphDev(KG, f, *(t.data_ptr() for t in g))
    rp.knnGraphRefineDev(KG, ds, *(t.data_ptr() for t in g), iters=ROUNDS)
    ctx.sync()
    f.close()
    return g, R, maxd


# ------------------------------------------------------------------ this build: the deletions
def step_delete(n, reps):
    import rptree_amd as rp
    from rptree_amd import _lib
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    X = gen.normal_dense2_torch(SEED, n, D, dev)
    torch.cuda.synchronize(dev)
    ds = rp.Dataset.from_torch(ctx, X)
    g, _, _ = full_graph(rp, ctx, dev, ds, n)
    out = triple(dev, n, KG)
    newid = torch.empty((n,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    rows = []
    for f in (0.0,) + FRACTIONS:                            # 0.0: a bitmap that keeps every row, no row to repair
        mask = keep_mask(n, f)
        words = torch.from_numpy(keep_words(mask)).to(dev)
        torch.cuda.synchronize(dev)
        for compact in (False, True):
            def run():
                rp.graphDeleteDev(ds, KG, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), words.data_ptr(),
                                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), newid.data_ptr(),
                                  compact=compact)
            ms, all_ms = event_ms(ctx.stream, run, reps)
            ctx.sync()
            kept, touched, evaluated, dropped = rp.graphDeleteLast(ctx)
            _lib.check(L.rpt_prof_reset(ctx._h))
            _lib.check(L.rpt_prof_enable(ctx._h, 1))
            run()
            ctx.sync()
            t, c = C.c_double(), C.c_int64()
            _lib.check(L.rpt_prof_get(ctx._h, 8, C.byref(t), C.byref(c)))
            _lib.check(L.rpt_prof_enable(ctx._h, 0))
            rows_out = kept if compact else n
            rows.append({"deleted_fraction": f, "compact": compact, "ms": ms, "all_ms": all_ms, "kept": kept,
                         "touched": touched, "evaluated": evaluated, "dropped": dropped,
                         "distances_per_touched_row": evaluated / touched if touched else 0.0,
                         "class_8_ms_of_a_profiled_call": t.value, "class_8_spans": c.value,
                         "mean_count_kept_rows": float(out[2][:rows_out].double().sum()) / max(kept, 1),
                         "crc": graph_crc(out[0][:rows_out], out[1][:rows_out], out[2][:rows_out])})
    floor = {r["compact"]: r["ms"] for r in rows if r["deleted_fraction"] == 0.0}
    for r in rows:
        r["repair_share"] = max(0.0, 1.0 - floor[r["compact"]] / r["ms"]) if r["deleted_fraction"] else 0.0
    return {"n": n, "runs": rows}


# ------------------------------------------------------------------ raw ctypes on the library RPTREE_HIP_LIB names
def step_rebuild(n, reps):
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
    ctx, stream = vp(), vp()
    call("rpt_ctx_create", i32(0), C.byref(ctx))
    call("rpt_ctx_stream", ctx, C.byref(stream))
    res = {}
    for f in FRACTIONS:
        mask = keep_mask(n, f)
        Xs = X.index_select(0, torch.from_numpy(np.flatnonzero(mask)).to(dev)).contiguous()
        ns = Xs.shape[0]
        maxd, pnz = shape(ns)
        _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)
        R = np.ascontiguousarray(R, dtype=np.float64)
        ds = vp()
        torch.cuda.synchronize(dev)
        call("rpt_dataset_dense_dev", ctx, vp(Xs.data_ptr()), C.c_int64(ns), i32(D), i32(RPT_F64), C.byref(ds))
        g = triple(dev, ns, KG)
        torch.cuda.synchronize(dev)
        held = {}

        def build():
            if held.get("f"):
                call("rpt_forest_free", held["f"])
            fr = vp()
            call("rpt_forest_build", ctx, ds, vp(R.ctypes.data), i32(TREES), i32(maxd), i32(MINL), i32(RPT_PROJ_MFMA),
                 C.byref(fr))
            held["f"] = fr

        def graph():
            call("rpt_knn_graph_dev", ctx, held["f"], ds, i32(KG), i32(0), vp(g[0].data_ptr()), vp(g[1].data_ptr()),
                 vp(g[2].data_ptr()))

        def rounds():
            call("rpt_knn_graph_refine_dev", ctx, ds, i32(KG), i32(KG), i32(ROUNDS), i32(0), vp(g[0].data_ptr()),
                 vp(g[1].data_ptr()), vp(g[2].data_ptr()))

        r = {"survivors": ns}
        r["forest_build_ms"], r["forest_build_all_ms"] = event_ms(stream.value, build, reps)
        call("rpt_ctx_sync", ctx)
        # the rounds refine in place: every repetition of them follows a fresh rpt_knn_graph_dev
        both_ms, both_all = event_ms(stream.value, lambda: (graph(), rounds()), reps)
        call("rpt_ctx_sync", ctx)
        r["knn_graph_plus_%d_rounds_ms" % ROUNDS], r["knn_graph_plus_rounds_all_ms"] = both_ms, both_all
        r["total_ms"] = r["forest_build_ms"] + both_ms
        r["crc"] = graph_crc(*g)
        call("rpt_forest_free", held["f"])
        call("rpt_dataset_free", ds)
        res["%g" % f] = r
    return res


# ------------------------------------------------------------------ this build: searching with and without the repair
def step_search(n, reps):
    import rptree_amd as rp
    from rptree_amd import _lib
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    X = gen.normal_dense2_torch(SEED, n, D, dev)
    Q = gen.normal_dense2_torch(SEED + 1, NQ, D, dev)
    torch.cuda.synchronize(dev)
    ds, qd = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, Q)
    g, R, maxd = full_graph(rp, ctx, dev, ds, n)
    f2 = rp._build(ctx, ds, R[:SEED_TREES], maxd, MINL, rp.RPT_PROJ_MFMA)
    sids, sdist, scnt = triple(dev, NQ, SEED_K)
    torch.cuda.synchronize(dev)
    L, vp = _lib.lib(), _lib.vp
    _lib.check(L.rpt_knn_dev(ctx._h, f2._h, ds._h, qd._h, SEED_K, rp.RPT_KNN_DEDUP, vp(sids.data_ptr()),
                             vp(sdist.data_ptr()), vp(scnt.data_ptr())))
    ctx.sync()
    seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < scnt[:, None], sids,
                        torch.full_like(sids, -1)).contiguous()
    out = triple(dev, n, KG)
    newid = torch.empty((n,), dtype=torch.int32, device=dev)
    ids, dist, cnt = triple(dev, NQ, K)
    torch.cuda.synchronize(dev)
    res = {"queries": NQ, "ef": EF}

    def recall(truth, got):
        return float(np.mean([[t in set(r) for t in tr] for tr, r in zip(truth.tolist(), got.tolist())]))

    for f in FRACTIONS:
        mask = keep_mask(n, f)
        words = torch.from_numpy(keep_words(mask)).to(dev)
        Xs = X.index_select(0, torch.from_numpy(np.flatnonzero(mask)).to(dev)).contiguous()
        torch.cuda.synchronize(dev)
        dss = rp.Dataset.from_torch(ctx, Xs)
        truth, _ = rp.bruteKnn(dss, qd, K)                  # compact ids
        rp.graphDeleteDev(ds, KG, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), words.data_ptr(),
                          out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), newid.data_ptr(), compact=True)
        ctx.sync()
        nid = newid.cpu().numpy()
        cseeds = torch.where(seeds >= 0, newid[seeds.clamp(min=0).long()], seeds).contiguous()
        torch.cuda.synchronize(dev)
        r = {"survivors": int(mask.sum())}
        for width in (4 * EF, 8 * EF):
            def run():
                rp.graphSearchAllowDev(ds, qd, KG, g[0].data_ptr(), g[2].data_ptr(), SEED_K, seeds.data_ptr(),
                                       words.data_ptr(), K, EF, width, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            ms, all_ms = event_ms(ctx.stream, run, reps)
            ctx.sync()
            got = ids.cpu().numpy()
            got = np.where(got >= 0, nid[np.where(got >= 0, got, 0)], -1)
            r["allow_list_on_the_unrepaired_graph_width_%d" % width] = {
                "ms": ms, "all_ms": all_ms, "recall_at_10": recall(truth, got),
                "evaluated_per_query": rp.graphSearchLast(ctx)[1] / NQ}

        def run():
            rp.graphSearchDev(dss, qd, KG, out[0].data_ptr(), out[2].data_ptr(), SEED_K, cseeds.data_ptr(), K, EF,
                              ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        r["plain_search_on_the_repaired_compacted_graph"] = {
            "ms": ms, "all_ms": all_ms, "recall_at_10": recall(truth, ids.cpu().numpy()),
            "evaluated_per_query": rp.graphSearchLast(ctx)[1] / NQ}
        res["%g" % f] = r
    return res


STEPS = {"delete": step_delete, "rebuild": step_rebuild, "search": step_search}


def run_step(name, n, reps, lib):
    env = dict(os.environ)
    if lib:
        env["RPTREE_HIP_LIB"] = os.path.abspath(lib)
    limit = STEP_LIMIT_S[name]                              # the step ends at its own limit, whatever this process does
    pr = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                         str(n), str(reps)], env=env, capture_output=True, text=True)
    if pr.returncode in (124, 137):
        raise SystemExit("step %s ran out of its %d s: nothing recorded" % (name, limit))
    if pr.returncode != 0:
        raise SystemExit("step %s failed (%d): nothing recorded\n%s%s" % (name, pr.returncode, pr.stdout, pr.stderr))
    print("step %s done" % name, file=sys.stderr, flush=True)
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, n, reps = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        print(json.dumps(STEPS[name](n, reps)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    parent = opt("--parent-lib", None)
    out_path = opt("--out", os.path.join(ROOT, "profiles", "graph_delete_times.json"))
    n = int(opt("--n", 1_000_000))
    reps = int(args[0]) if args else 5
    if not parent:
        raise SystemExit("--parent-lib PATH is required: the yardstick is the parent commit's rebuild")
    this_lib = os.environ.get("RPTREE_HIP_LIB") or os.path.join(ROOT, "rp-tree_amd", "librptree_hip.so")
    # a step that fails raises: nothing further starts
    delete = run_step("delete", n, reps, None)
    mine = run_step("rebuild", n, reps, this_lib)
    theirs = run_step("rebuild", n, reps, parent)
    search = run_step("search", n, reps, None)
    for f in mine:
        if mine[f]["crc"] != theirs[f]["crc"]:
            raise SystemExit("this build's and the parent's rebuilt graphs differ at fraction " + f)
    res = {"tool": "tools/graph_delete_times.py", "reps": reps, "n": n,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step",
           "workload": "C2: %d x %d float64, minLeaf %d, k = %d; graph = knnGraph(%d trees) + %d refinement rounds over all "
                       "rows; deleted: np.random.default_rng(7).random(n) < f for f in %s"
                       % (n, D, MINL, KG, TREES, ROUNDS, list(FRACTIONS)),
           "delete": delete["runs"],
           "delete_note": "deleted_fraction 0 passes a bitmap that keeps every row: the mark, scan and copy kernels and "
                          "an empty repair launch; repair_share = 1 - that / ms",
           "rebuild_over_the_survivors": {"the parent commit's library": theirs, "this build": mine,
                                          "one_checksum": "per fraction the two rebuilt graphs have one checksum"},
           "search": search,
           "note": "C2's rows are i.i.d. normal: they have no neighbourhoods, so the recall columns price the method on "
                   "the hardest case; tests/test_graph_delete_host.py holds the table on rows that have them"}
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
