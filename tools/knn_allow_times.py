"""An allow-list on the forest query and on the exhaustive kNN (rpt_knn_allow_dev, rpt_brute_knn_allow_dev:
csrc/knn_allow.hip's compaction and list kernels + the general kernels) at the C2 shape: 1 M x 128 float64,
32 trees, minLeaf 128, k = 10, 10 000 queries, allowed 100 / 50 / 10 / 1 % (np.random.default_rng(7)).

    python tools/knn_allow_times.py [reps] --parent-lib PATH [--out FILE] [--n N] [--no-seeds]

Steps, each a fresh child process under a time limit of its own (a step that fails or runs out of time
ends the run; nothing is recorded then, except for the last step, which is recorded as not measured):
  allow    this build.  Per fraction: the truth among the allowed rows for the first 1 000 queries by
           rpt_brute_knn_allow_dev, against index_select of the allowed rows + rpt_brute_knn_dev on the
           copy (the copy timed on its own; the two answers must agree); rpt_knn_allow_dev |
           RPT_KNN_DEDUP: ms, the list kernel alone (rpt_prof_* class 5), allowed entries and answers
           per query, recall@10 among the allowed rows.  The unfiltered rpt_knn_dev | RPT_KNN_DEDUP.
  parent   the parent commit's library (PATH): rpt_knn_dev | RPT_KNN_DEDUP at k = 10 and k = 64, then
           a filter on the host: answers left per query and recall@10 among the allowed rows.  Its
           k = 10 checksum must be this build's.
  seeds    this build.  A graph (knnGraph of the 32 trees, 2 refinement rounds, graphPrepare with the
           reverse union, 20 columns); 8 seeds per query from 2 trees by rpt_knn_dev and by
           rpt_knn_allow_dev, each fed to rpt_graph_search_allow_dev at ef = 32, width 128.
Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  Writes
profiles/knn_allow_times.json.  No ratio is fixed in advance.
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

D, MINL, K, POST_K, SEED, NQ, NQ_TRUTH, TREES = 128, 128, 10, 64, 1234, 10_000, 1000, 32
KG, KOUT, SEED_TREES, SEED_K, EF, WIDTH = 10, 20, 2, 8, 32, 128
FRACS = (1.0, 0.5, 0.1, 0.01)
NEW_SYMBOLS = ("rpt_knn_allow_host", "rpt_knn_allow_dev", "rpt_allow_candidates_host", "rpt_brute_knn_allow_host",
               "rpt_brute_knn_allow_dev", "rpt_recall_hits_allow_host", "rpt_knn_allow_last")
STEP_LIMIT_S = {"allow": 420, "parent": 300, "seeds": 540}


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


def allow_mask(n, frac):
    return np.random.default_rng(7).random(n) < frac


def recall_of(ids, truth):
    """ids: [nq][*] with -1 padding; truth: [nq][K] with -1 padding where fewer than K rows are allowed"""
    hits = want = 0
    for t, r in zip(truth.tolist(), ids.tolist()):
        t = [v for v in t if v >= 0]
        want += len(t)
        hits += len(set(t) & set(r))
    return hits / max(want, 1)


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.cpu().numpy().tobytes(), c)
    return c


def setup(n, trees, parent_lib=""):
    """the package (on another build of the library, if named), rows, queries and the forest"""
    from rptree_amd import _lib
    if parent_lib:                   # the parent's library lacks the new symbols
        _lib.LIB_PATH = parent_lib
        for s in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(s)
    import rptree_amd as rp
    from rptree_amd import gen
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    X = gen.normal_dense2_torch(SEED, n, D, dev)
    Q = gen.normal_dense2_torch(SEED + 1, NQ, D, dev)
    torch.cuda.synchronize(dev)
    ds, qd = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, Q)
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))            # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)
    f = rp._build(ctx, ds, R[:trees], maxd, MINL, rp.RPT_PROJ_MFMA)
    return rp, _lib, ctx, dev, X, Q, ds, qd, f, R, maxd


def outputs(dev, nq, k):
    return (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float64, device=dev),
            torch.empty((nq,), dtype=torch.int32, device=dev))


def words_of(rp, mask, n, dev):
    w = torch.from_numpy(rp.allowBitmap(mask, n).view(np.int32).copy()).to(dev)
    torch.cuda.synchronize(dev)
    return w


# ------------------------------------------------------------------ this build: the filtered query and the truth
def step_allow(n, reps, scratch, _):
    rp, _lib, ctx, dev, X, Q, ds, qd, f, R, maxd = setup(n, TREES)
    L, vp = _lib.lib(), C.c_void_p
    qt = rp.Dataset.from_torch(ctx, Q[:NQ_TRUTH])
    ki, kd, kc = outputs(dev, NQ, K)
    ti, td, _ = outputs(dev, NQ_TRUTH, K)
    torch.cuda.synchronize(dev)
    out = {"n": n, "maxDepth": maxd, "perm_crc": zlib.crc32(f.perm.tobytes()), "by_allowed": {}}

    def unfiltered():
        _lib.check(L.rpt_knn_dev(ctx._h, f._h, ds._h, qd._h, K, rp.RPT_KNN_DEDUP, vp(ki.data_ptr()), vp(kd.data_ptr()),
                                 vp(kc.data_ptr())))
    ms, all_ms = event_ms(ctx.stream, unfiltered, reps)
    ctx.sync()
    out["knn_dev_dedup_k10"] = {"ms": ms, "all_ms": all_ms, "crc": crc(ki, kd, kc)}
    for frac in FRACS:
        mask = allow_mask(n, frac)
        words = words_of(rp, mask, n, dev)
        row = {"allowed_rows": int(mask.sum())}

        def brute():
            _lib.check(L.rpt_brute_knn_allow_dev(ctx._h, ds._h, qt._h, vp(words.data_ptr()), K, 0, vp(ti.data_ptr()),
                                                 vp(td.data_ptr())))
        ms, all_ms = event_ms(ctx.stream, brute, reps)
        ctx.sync()
        truth = ti.cpu().numpy().astype(np.int64)
        np.save(os.path.join(scratch, "truth_%g.npy" % frac), truth)
        row["brute_knn_allow_dev_1000q"] = {"ms": ms, "all_ms": all_ms}
        # the route that existed: copy the allowed rows, search the copy, map the ids back on the host
        idx = torch.from_numpy(np.flatnonzero(mask)).to(dev)
        cur = torch.cuda.current_stream(dev)
        copies = []
        for rep in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(cur)
            sub = X.index_select(0, idx)
            b.record(cur)
            b.synchronize()
            if rep:
                copies.append(a.elapsed_time(b))
        copies.sort()
        sds = rp.Dataset.from_torch(ctx, sub)
        si, sd, _ = outputs(dev, NQ_TRUTH, K)
        torch.cuda.synchronize(dev)

        def brute_copy():
            _lib.check(L.rpt_brute_knn_dev(ctx._h, sds._h, qt._h, K, 0, vp(si.data_ptr()), vp(sd.data_ptr())))
        ms, all_ms = event_ms(ctx.stream, brute_copy, reps)
        ctx.sync()
        got = si.cpu().numpy()
        back = np.where(got >= 0, np.flatnonzero(mask)[np.maximum(got, 0)], -1)
        row["index_select_then_brute_knn_dev_1000q"] = {
            "copy_ms": copies[len(copies) // 2], "copy_all_ms": copies, "copy_bytes": int(sub.numel()) * 8, "ms": ms,
            "all_ms": all_ms, "same_ids": bool(np.array_equal(back, truth)),
            "same_distance_bits": bool(np.array_equal(sd.cpu().numpy().view(np.uint64), td.cpu().numpy().view(np.uint64)))}
        sds.close()
        del sub, idx

        def filtered():
            _lib.check(L.rpt_knn_allow_dev(ctx._h, f._h, ds._h, qd._h, vp(words.data_ptr()), K, rp.RPT_KNN_DEDUP,
                                           vp(ki.data_ptr()), vp(kd.data_ptr()), vp(kc.data_ptr())))
        ms, all_ms = event_ms(ctx.stream, filtered, reps)
        ctx.sync()
        cand, allowed, unc = rp.knnAllowLast(ctx)
        got = ki.cpu().numpy()
        assert mask[got[got >= 0]].all()
        r = {"ms": ms, "all_ms": all_ms, "crc": crc(ki, kd, kc), "candidates_per_query": cand / NQ,
             "allowed_per_query": allowed / NQ, "answers_per_query": float(kc.double().mean()), "uncertified": unc,
             "recall_at_10_among_allowed": recall_of(got[:NQ_TRUTH], truth)}
        _lib.check(L.rpt_prof_enable(ctx._h, 1))
        ts = []
        for _ in range(reps):
            _lib.check(L.rpt_prof_reset(ctx._h))
            filtered()
            pms, launches = C.c_double(), C.c_int64()
            _lib.check(L.rpt_prof_get(ctx._h, 5, C.byref(pms), C.byref(launches)))
            ts.append(pms.value)
        _lib.check(L.rpt_prof_enable(ctx._h, 0))
        ts.sort()
        r["list_kernel_ms"] = ts[len(ts) // 2]
        row["knn_allow_dev_dedup_k10"] = r
        out["by_allowed"]["%g" % frac] = row
    return out


# ------------------------------------------------------------------ the parent commit's library: today's route
def step_parent(n, reps, scratch, parent_lib):
    rp, _lib, ctx, dev, X, Q, ds, qd, f, R, maxd = setup(n, TREES, parent_lib)
    L, vp = _lib.lib(), C.c_void_p
    out = {"perm_crc": zlib.crc32(f.perm.tobytes())}
    for k in (K, POST_K):
        ki, kd, kc = outputs(dev, NQ, k)
        torch.cuda.synchronize(dev)

        def run():
            _lib.check(L.rpt_knn_dev(ctx._h, f._h, ds._h, qd._h, k, rp.RPT_KNN_DEDUP, vp(ki.data_ptr()), vp(kd.data_ptr()),
                                     vp(kc.data_ptr())))
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        row = {"ms": ms, "all_ms": all_ms, "crc": crc(ki, kd, kc), "by_allowed": {},
               "note": "ms is the query alone: the copy of k answers per query to the host and the filter there are not in it"}
        got = ki.cpu().numpy()
        for frac in FRACS:
            mask = allow_mask(n, frac)
            kept = np.full((NQ, K), -1, dtype=np.int64)
            counts = []
            for i in range(NQ):
                r = [v for v in got[i].tolist() if v >= 0 and mask[v]][:K]
                kept[i, :len(r)] = r
                counts.append(len(r))
            truth = np.load(os.path.join(scratch, "truth_%g.npy" % frac))
            row["by_allowed"]["%g" % frac] = {"answers_per_query": float(np.mean(counts)),
                                              "recall_at_10_among_allowed": recall_of(kept[:NQ_TRUTH], truth)}
        out["knn_dev_dedup_k%d_then_host_filter" % k] = row
    return out


# ------------------------------------------------------------------ this build: seeds for the graph search
def step_seeds(n, reps, scratch, _):
    rp, _lib, ctx, dev, X, Q, ds, qd, f, R, maxd = setup(n, TREES)
    L, vp = _lib.lib(), C.c_void_p
    g0 = (torch.empty((n, KG), dtype=torch.int32, device=dev), torch.empty((n, KG), dtype=torch.float64, device=dev),
          torch.empty((n,), dtype=torch.int32, device=dev))
    gids = torch.empty((n, KOUT), dtype=torch.int32, device=dev)
    gdist = torch.empty((n, KOUT), dtype=torch.float64, device=dev)
    gcnt = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.knnGraphDev(KG, f, *(t.data_ptr() for t in g0))
    rp.knnGraphRefineDev(KG, ds, *(t.data_ptr() for t in g0), iters=2)
    rp.graphPrepareDev(KG, ds, *(t.data_ptr() for t in g0), KOUT, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(),
                       diversify=False, reverse=True)
    ctx.sync()
    f.close()
    f2 = rp._build(ctx, ds, R[:SEED_TREES], maxd, MINL, rp.RPT_PROJ_MFMA)
    si, sd, sc = outputs(dev, NQ, SEED_K)
    ids, dist, cnt = outputs(dev, NQ, K)
    torch.cuda.synchronize(dev)

    def seeds_of(words):
        def run():
            if words is None:
                _lib.check(L.rpt_knn_dev(ctx._h, f2._h, ds._h, qd._h, SEED_K, rp.RPT_KNN_DEDUP, vp(si.data_ptr()),
                                         vp(sd.data_ptr()), vp(sc.data_ptr())))
            else:
                _lib.check(L.rpt_knn_allow_dev(ctx._h, f2._h, ds._h, qd._h, vp(words.data_ptr()), SEED_K, rp.RPT_KNN_DEDUP,
                                               vp(si.data_ptr()), vp(sd.data_ptr()), vp(sc.data_ptr())))
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < sc[:, None], si, torch.full_like(si, -1)).contiguous()
        torch.cuda.synchronize(dev)
        return seeds, ms, all_ms

    out = {"mean_degree": float(gcnt.double().mean()), "by_allowed": {}}
    plain_seeds, plain_ms, plain_all = seeds_of(None)
    for frac in FRACS:
        mask = allow_mask(n, frac)
        words = words_of(rp, mask, n, dev)
        truth = np.load(os.path.join(scratch, "truth_%g.npy" % frac))
        row = {}
        for tag, (seeds, ms, all_ms) in (("seeds_from_knn_dev", (plain_seeds, plain_ms, plain_all)),
                                         ("seeds_from_knn_allow_dev", seeds_of(words))):
            def search():
                rp.graphSearchAllowDev(ds, qd, KOUT, gids.data_ptr(), gcnt.data_ptr(), SEED_K, seeds.data_ptr(),
                                       words.data_ptr(), K, EF, WIDTH, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            sms, sall = event_ms(ctx.stream, search, reps)
            ctx.sync()
            _, evaluated = rp.graphSearchLast(ctx)
            sh = seeds.cpu().numpy()
            usable = float(((sh >= 0) & mask[np.maximum(sh, 0)]).sum(axis=1).mean())
            row[tag] = {"seed_ms": ms, "seed_all_ms": all_ms, "usable_seeds_per_query": usable, "search_ms": sms,
                        "search_all_ms": sall, "evaluated_per_query": evaluated / NQ,
                        "recall_at_10_among_allowed": recall_of(ids.cpu().numpy()[:NQ_TRUTH], truth),
                        "answers_per_query": float(cnt.double().mean())}
        out["by_allowed"]["%g" % frac] = row
    return out


STEPS = {"allow": step_allow, "parent": step_parent, "seeds": step_seeds}


def run_step(name, n, reps, scratch, parent_lib):
    limit = STEP_LIMIT_S[name]                              # the step ends at its own limit, whatever this process does
    pr = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                         str(n), str(reps), scratch, parent_lib], capture_output=True, text=True)
    if pr.returncode in (124, 137):
        raise SystemExit("step %s ran out of its %d s: nothing recorded" % (name, limit))
    if pr.returncode != 0:
        raise SystemExit("step %s failed (%d): nothing recorded\n%s%s" % (name, pr.returncode, pr.stdout, pr.stderr))
    print("step %s done" % name, file=sys.stderr, flush=True)
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, n, reps, scratch, parent_lib = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
        print(json.dumps(STEPS[name](n, reps, scratch, parent_lib)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    parent = opt("--parent-lib", None)
    out_path = opt("--out", os.path.join(ROOT, "profiles", "knn_allow_times.json"))
    n = int(opt("--n", 1_000_000))
    seeds = "--no-seeds" not in args
    if not seeds:
        args.remove("--no-seeds")
    reps = int(args[0]) if args else 5
    if not parent:
        raise SystemExit("--parent-lib PATH is required: the yardsticks are the parent commit's library")
    parent = os.path.abspath(parent)
    scratch = tempfile.mkdtemp(prefix="knn_allow_")
    res = {"tool": "tools/knn_allow_times.py", "reps": reps, "n": n,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step; "
                     "list_kernel_ms: rpt_prof_* class 5 (the compaction kernel alone)",
           "workload": "C2: %d x %d float64, %d trees, minLeaf %d, k = %d, %d queries; allow = "
                       "np.random.default_rng(7).random(n) < fraction; recall@10 on the first %d queries against "
                       "rpt_brute_knn_allow_dev" % (n, D, TREES, MINL, K, NQ, NQ_TRUTH)}
    try:                                                    # a step that fails raises: nothing further starts
        res["this_build"] = run_step("allow", n, reps, scratch, "")
        res["parent_library"] = run_step("parent", n, reps, scratch, parent)
        if res["this_build"]["perm_crc"] != res["parent_library"]["perm_crc"]:
            raise SystemExit("this build and the parent's library built different forests")
        mine = res["this_build"]["knn_dev_dedup_k10"]["crc"]
        if mine != res["parent_library"]["knn_dev_dedup_k%d_then_host_filter" % K]["crc"]:
            raise SystemExit("this build's and the parent's unfiltered rpt_knn_dev answers differ")
        res["unfiltered_checksums_agree"] = True
        res["all_allowed_has_knn_dev_checksum"] = res["this_build"]["by_allowed"]["1"]["knn_allow_dev_dedup_k10"]["crc"] == mine
        if seeds:
            try:
                res["graph_seeds"] = run_step("seeds", n, reps, scratch, "")
            except SystemExit as e:                         # the last step: the rest stays recorded
                res["graph_seeds"] = "not measured: %s" % str(e).splitlines()[0]
        else:
            res["graph_seeds"] = "not measured"
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
