"""Beam search over an allow-list of ids (rpt_graph_search_allow_dev; the F switch of csrc/graph_dev.h's
beam, graph_search_allow_kernel) at C2: 1 M x 128 f64, 32 trees, minLeaf 128, k = 10, 10 000 queries.

    python tools/graph_search_allow_times.py [reps] --parent-lib PATH [--out FILE] [--n N]

Steps, each a fresh child process under a time limit of its own (a step that fails or runs out of time
ends the run; nothing is recorded then):
  allow   this build: the graph (knnGraph of the 32 trees + 2 knnGraphRefine rounds + graphPrepare with
          the reverse union, 20 columns), the seeds (rpt_knn_dev on the first 2 trees, 8 nearest,
          de-duplicated), per allowed fraction 1.0 / 0.5 / 0.1 / 0.01 (np.random.default_rng(7).random(n)
          < fraction) the exact answer among the allowed rows (bruteKnn on those rows alone), and
          rpt_graph_search_allow_dev at ef = 32 with width ef / 4 ef / 8 ef / 1024: ms, recall@10 against
          that answer, distances per query, a checksum.  Also the new entry point with a NULL bitmap at
          width = ef, which must give the unfiltered answer.  The graph and the seeds are left in a
          scratch directory for the other steps
  plain   rpt_graph_search_dev through raw ctypes on the library RPTREE_HIP_LIB names, run twice: on this
          build's library and on the parent commit's (PATH).  Same rows, queries, graph and seeds.
          (a) ef = 32, k = 10: the unfiltered cost, which the null-bitmap call above is held against and
          which the two libraries must agree on (one checksum);  (b) k = 64, ef = 256, the caps of the
          entry point, filtered on the host: the only filtered route there was, with its recall@10 per
          fraction against the same exact answers
Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  Writes
profiles/graph_search_allow_times.json.  No ratio is fixed in advance: the file holds what was measured.
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

D, MINL, K, KG, KOUT, SEED, NQ, TREES, SEED_TREES, SEED_K = 128, 128, 10, 10, 20, 1234, 10_000, 32, 2, 8
EF = 32
WIDTHS = (EF, 4 * EF, 8 * EF, 1024)
FRACS = (1.0, 0.5, 0.1, 0.01)
POST_K, POST_EF = 64, 256
RPT_F64 = 0
STEP_LIMIT_S = {"allow": 540, "plain": 300}


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
    return hits / want


def answer_crc(ids, dist, cnt):
    return zlib.crc32(cnt.cpu().numpy().tobytes(), zlib.crc32(dist.cpu().numpy().tobytes(),
                                                              zlib.crc32(ids.cpu().numpy().tobytes())))


def outputs(dev, k):
    return (torch.empty((NQ, k), dtype=torch.int32, device=dev), torch.empty((NQ, k), dtype=torch.float64, device=dev),
            torch.empty((NQ,), dtype=torch.int32, device=dev))


# ------------------------------------------------------------------ this build: the graph, the truth, the sweep
def step_allow(n, reps, scratch):
    import rptree_amd as rp
    from rptree_amd import _lib
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    X = gen.normal_dense2_torch(SEED, n, D, dev)
    Q = gen.normal_dense2_torch(SEED + 1, NQ, D, dev)
    torch.cuda.synchronize(dev)
    ds, qd = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, Q)
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))           # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)

    # the exact answer among the allowed rows, per fraction: brute force over those rows alone
    masks, truths = {}, {}
    for frac in FRACS:
        mask = allow_mask(n, frac)
        idx = np.flatnonzero(mask)
        sub = X[torch.from_numpy(idx).to(dev)].contiguous()
        torch.cuda.synchronize(dev)
        sds = rp.Dataset.from_torch(ctx, sub)
        tid, _ = rp.bruteKnn(sds, qd, min(K, len(idx)))
        truth = np.full((NQ, K), -1, dtype=np.int64)
        truth[:, :tid.shape[1]] = np.where(tid >= 0, idx[np.maximum(tid, 0)], -1)
        masks[frac], truths[frac] = mask, truth
        np.save(os.path.join(scratch, "truth_%g.npy" % frac), truth)
        sds.close()
        del sub

    f = rp._build(ctx, ds, R, maxd, MINL, rp.RPT_PROJ_MFMA)
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

    # the seeds: 8 nearest de-duplicated candidates of the first 2 trees
    f2 = rp._build(ctx, ds, R[:SEED_TREES], maxd, MINL, rp.RPT_PROJ_MFMA)
    sids, sdist, scnt = (torch.empty((NQ, SEED_K), dtype=torch.int32, device=dev),
                         torch.empty((NQ, SEED_K), dtype=torch.float64, device=dev),
                         torch.empty((NQ,), dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    L, vp = _lib.lib(), _lib.vp
    _lib.check(L.rpt_knn_dev(ctx._h, f2._h, ds._h, qd._h, SEED_K, rp.RPT_KNN_DEDUP, vp(sids.data_ptr()),
                             vp(sdist.data_ptr()), vp(scnt.data_ptr())))
    ctx.sync()
    seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < scnt[:, None], sids,
                        torch.full_like(sids, -1)).contiguous()
    torch.cuda.synchronize(dev)
    for name, t in (("gids", gids), ("gcnt", gcnt), ("seeds", seeds)):
        np.save(os.path.join(scratch, name + ".npy"), t.cpu().numpy())

    ids, dist, cnt = outputs(dev, K)
    torch.cuda.synchronize(dev)

    def timed(words, width):
        ptr = 0 if words is None else words.data_ptr()

        def run():
            rp.graphSearchAllowDev(ds, qd, KOUT, gids.data_ptr(), gcnt.data_ptr(), SEED_K, seeds.data_ptr(), ptr, K, EF,
                                   width, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        expansions, evaluated = rp.graphSearchLast(ctx)
        return {"ef": EF, "width": width, "ms": ms, "all_ms": all_ms, "evaluated_per_query": evaluated / NQ,
                "expansions_per_query": expansions / NQ, "crc": answer_crc(ids, dist, cnt)}

    null = timed(None, EF)
    null["recall_at_10"] = recall_of(ids.cpu().numpy(), truths[1.0])
    sweep = []
    for frac in FRACS:
        words = torch.from_numpy(rp.allowBitmap(masks[frac], n).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        for width in WIDTHS:
            row = timed(words, width)
            got = ids.cpu().numpy()
            assert masks[frac][got[got >= 0]].all()
            row.update({"allowed": frac, "allowed_rows": int(masks[frac].sum()),
                        "recall_at_10": recall_of(got, truths[frac]), "mean_count": float(cnt.double().mean())})
            sweep.append(row)
    return {"n": n, "maxDepth": maxd, "mean_degree": float(gcnt.double().mean()), "null_bitmap": null, "sweep": sweep}


# ------------------------------------------------------------------ raw ctypes on the library RPTREE_HIP_LIB names
def step_plain(n, reps, scratch):
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
    Q = gen.normal_dense2_torch(SEED + 1, NQ, D, dev)
    gids, gcnt, seeds = (torch.from_numpy(np.load(os.path.join(scratch, name + ".npy"))).to(dev)
                         for name in ("gids", "gcnt", "seeds"))
    ctx, ds, qd, stream = vp(), vp(), vp(), vp()
    call("rpt_ctx_create", i32(0), C.byref(ctx))
    call("rpt_ctx_stream", ctx, C.byref(stream))
    torch.cuda.synchronize(dev)
    call("rpt_dataset_dense_dev", ctx, vp(X.data_ptr()), C.c_int64(n), i32(D), i32(RPT_F64), C.byref(ds))
    call("rpt_dataset_dense_dev", ctx, vp(Q.data_ptr()), C.c_int64(NQ), i32(D), i32(RPT_F64), C.byref(qd))
    res = {}
    for tag, k, ef in (("unfiltered", K, EF), ("post_filter", POST_K, POST_EF)):
        ids, dist, cnt = outputs(dev, k)
        torch.cuda.synchronize(dev)

        def run():
            call("rpt_graph_search_dev", ctx, ds, qd, i32(KOUT), vp(gids.data_ptr()), vp(gcnt.data_ptr()), i32(SEED_K),
                 vp(seeds.data_ptr()), i32(k), i32(ef), i32(0), i32(0), vp(ids.data_ptr()), vp(dist.data_ptr()),
                 vp(cnt.data_ptr()))
        ms, all_ms = event_ms(stream.value, run, reps)
        call("rpt_ctx_sync", ctx)
        exp, ev = C.c_int64(), C.c_int64()
        call("rpt_graph_search_last", ctx, C.byref(exp), C.byref(ev))
        row = {"k": k, "ef": ef, "ms": ms, "all_ms": all_ms, "evaluated_per_query": ev.value / NQ,
               "crc": answer_crc(ids, dist, cnt)}
        got = ids.cpu().numpy()
        if tag == "unfiltered":
            row["recall_at_10"] = recall_of(got, np.load(os.path.join(scratch, "truth_1.npy")))
        else:                                              # the host keeps the first 10 allowed of the 64 answers
            row["recall_at_10_by_allowed"] = {}
            row["mean_count_by_allowed"] = {}
            for frac in FRACS:
                mask = allow_mask(n, frac)
                kept = np.full((NQ, K), -1, dtype=np.int64)
                counts = []
                for i in range(NQ):
                    r = [v for v in got[i].tolist() if v >= 0 and mask[v]][:K]
                    kept[i, :len(r)] = r
                    counts.append(len(r))
                row["recall_at_10_by_allowed"]["%g" % frac] = recall_of(kept, np.load(os.path.join(scratch, "truth_%g.npy" % frac)))
                row["mean_count_by_allowed"]["%g" % frac] = float(np.mean(counts))
        res[tag] = row
    return res


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
        print(json.dumps({"allow": step_allow, "plain": step_plain}[name](n, reps, scratch)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    parent = opt("--parent-lib", None)
    out_path = opt("--out", os.path.join(ROOT, "profiles", "graph_search_allow_times.json"))
    n = int(opt("--n", 1_000_000))
    reps = int(args[0]) if args else 5
    if not parent:
        raise SystemExit("--parent-lib PATH is required: both yardsticks are the parent commit's library")
    this_lib = os.environ.get("RPTREE_HIP_LIB") or os.path.join(ROOT, "rp-tree_amd", "librptree_hip.so")
    scratch = tempfile.mkdtemp(prefix="graph_search_allow_")
    try:                                                    # a step that fails raises: nothing further starts
        allow = run_step("allow", n, reps, None, scratch)
        mine = run_step("plain", n, reps, this_lib, scratch)
        theirs = run_step("plain", n, reps, parent, scratch)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    for tag in ("unfiltered", "post_filter"):
        if mine[tag]["crc"] != theirs[tag]["crc"]:
            raise SystemExit("%s: this build's and the parent's rpt_graph_search_dev answers differ" % tag)
    if allow["null_bitmap"]["crc"] != theirs["unfiltered"]["crc"]:
        raise SystemExit("a null bitmap gave another answer than the parent's rpt_graph_search_dev")
    res = {"tool": "tools/graph_search_allow_times.py", "reps": reps, "n": n,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step",
           "workload": "C2: %d x %d float64, minLeaf %d, maxDepth %d, k = %d, %d queries, graph = knnGraph(%d trees, k = %d) + "
                       "2 refinement rounds + graphPrepare(reverse union, %d columns; mean degree %.2f), seeds = %d nearest "
                       "de-duplicated candidates of %d trees; allow = np.random.default_rng(7).random(n) < fraction; "
                       "recall@10 against bruteKnn over the allowed rows alone"
                       % (n, D, MINL, allow["maxDepth"], K, NQ, TREES, KG, KOUT, allow["mean_degree"], SEED_K, SEED_TREES),
           "yardstick_a_unfiltered_cost": {
               "rpt_graph_search_dev, the parent commit's library": theirs["unfiltered"],
               "rpt_graph_search_dev, this build": mine["unfiltered"],
               "rpt_graph_search_allow_dev, null bitmap, width = ef, this build": allow["null_bitmap"],
               "one_checksum": "the three answers have one checksum"},
           "yardstick_b_post_filtering": {
               "rpt_graph_search_dev k = 64, ef = 256, filtered on the host, the parent commit's library": theirs["post_filter"],
               "the same, this build": mine["post_filter"],
               "note": "ms is the search alone: the copy of 64 answers per query to the host and the filter there are not in it"},
           "sweep": allow["sweep"]}
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
