"""The search-graph preparation (rpt_graph_prepare_dev, csrc/graph_prepare.hip) at C2, and the beam
search (rpt_graph_search_dev) on the raw against the prepared graphs.

    python tools/graph_prepare_times.py [reps] [--n N] [--out FILE] [--parent-lib LIB.so]

C2 = the flagship shape (seeds of BASELINE configs[1]: 1 M x 128 f64, rpTreeCfg depth, minLeaf 128),
k = 10, 10 000 queries.  The graph is knnGraph of the 32-tree forest plus two refinement rounds; the
seeds are those of tools/graph_search_times.py (the de-duplicated 8 nearest candidates of the forest's
first 2 trees).  Timed with HIP events on the ctx stream, median of REPS behind a warm-up:
  rpt_graph_prepare_dev for DIVERSIFY (kout = k), REVERSE (kout = 2 k) and both (kout = 2 k), with
      the call's statistics and the mean degree of the result;
  rpt_graph_search_dev on the raw and on each prepared graph with ef in {16, 32, 64, 128}: ms per
      batch, recall@10 against bruteKnn, distances evaluated per query.
The claim to check is search time at EQUAL RECALL: for every prepared graph and ef the report names
the raw graph's smallest ef whose recall is at least as high (none: the raw graph never gets there)
and its time.  With --parent-lib the raw graph's searches also run in a child process on another
build of the library (the parent commit's, started with RPTREE_HIP_LIB), as the other tools do.
Writes profiles/graph_prepare_times.json.  --n N shrinks the data set (a rehearsal; nothing is
written unless --out is given).
"""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rp-tree_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rptree_amd import _lib  # noqa: E402

RAW_ONLY = "--raw-only" in sys.argv
if RAW_ONLY:                                               # another build: it need not know the preparation yet
    for name in [s for s in _lib.SYMBOLS if s.startswith("rpt_graph_prepare")]:
        del _lib.SYMBOLS[name]

import rptree_amd as rp  # noqa: E402
from rptree_amd import gen  # noqa: E402

D, MINL, K, KG, SEED, NQ, TREES, SEED_TREES, SEED_K = 128, 128, 10, 10, 1234, 10_000, 32, 2, 8
EFS = (16, 32, 64, 128)
PREPARED = (("diversify", True, False, KG), ("reverse", False, True, 2 * KG), ("diversify + reverse", True, True, 2 * KG))


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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n, out_path, parent = 1_000_000, os.path.join(ROOT, "profiles", "graph_prepare_times.json"), None
    if "--n" in sys.argv:
        v = sys.argv[sys.argv.index("--n") + 1]
        n = int(v)
        args.remove(v)
        out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args.remove(out_path)
    if "--parent-lib" in sys.argv:
        parent = sys.argv[sys.argv.index("--parent-lib") + 1]
        args.remove(parent)
    reps = int(args[0]) if args else 5
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    X = gen.normal_dense2_torch(SEED, n, D, dev)
    Q = gen.normal_dense2_torch(SEED + 1, NQ, D, dev)
    torch.cuda.synchronize(dev)
    ds, qd = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, Q)
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))           # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)
    truth, _ = rp.bruteKnn(ds, qd, K)
    L = _lib.lib()
    vp = _lib.vp

    ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    dist = torch.empty((NQ, K), dtype=torch.float64, device=dev)
    cnt = torch.empty((NQ,), dtype=torch.int32, device=dev)

    # the graph: the 32-tree forest's, two NN-descent rounds
    f = rp._build(ctx, ds, R, maxd, MINL, rp.RPT_PROJ_MFMA)
    gids = torch.empty((n, KG), dtype=torch.int32, device=dev)
    gdist = torch.empty((n, KG), dtype=torch.float64, device=dev)
    gcnt = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    rp.knnGraphDev(KG, f, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr())
    rp.knnGraphRefineDev(KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), iters=2)
    ctx.sync()
    f.close()

    # the seeds: 8 nearest de-duplicated candidates of the first 2 trees
    f2 = rp._build(ctx, ds, R[:SEED_TREES], maxd, MINL, rp.RPT_PROJ_MFMA)
    sids = torch.empty((NQ, SEED_K), dtype=torch.int32, device=dev)
    sdist = torch.empty((NQ, SEED_K), dtype=torch.float64, device=dev)
    scnt = torch.empty((NQ,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _lib.check(L.rpt_knn_dev(ctx._h, f2._h, ds._h, qd._h, SEED_K, rp.RPT_KNN_DEDUP, vp(sids.data_ptr()),
                             vp(sdist.data_ptr()), vp(scnt.data_ptr())))
    ctx.sync()
    seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < scnt[:, None], sids,
                        torch.full_like(sids, -1)).contiguous()
    torch.cuda.synchronize(dev)

    def search_rows(kg, g_ids, g_cnt):
        rows = []
        for ef in EFS:
            def run():
                rp.graphSearchDev(ds, qd, kg, g_ids.data_ptr(), g_cnt.data_ptr(), SEED_K, seeds.data_ptr(), K, ef,
                                  ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            ms, all_ms = event_ms(ctx.stream, run, reps)
            ctx.sync()
            expansions, evaluated = rp.graphSearchLast(ctx)
            rows.append({"ef": ef, "ms": ms, "all_ms": all_ms, "recall_at_10": recall_of(ids.cpu().numpy(), truth),
                         "evaluated_per_query": evaluated / NQ, "expansions_per_query": expansions / NQ})
        return rows

    raw = {"graph": "raw", "library": os.path.basename(_lib.LIB_PATH), "kg": KG,
           "mean_degree": float(gcnt.double().mean().item()), "search": search_rows(KG, gids, gcnt)}
    if RAW_ONLY:
        print(json.dumps(raw))
        return

    prepared = []
    for name, diversify, reverse, kout in PREPARED:
        oids = torch.empty((n, kout), dtype=torch.int32, device=dev)
        odist = torch.empty((n, kout), dtype=torch.float64, device=dev)
        ocnt = torch.empty((n,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def run():
            rp.graphPrepareDev(KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), kout, oids.data_ptr(),
                               odist.data_ptr(), ocnt.data_ptr(), diversify=diversify, reverse=reverse)
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        pairs, occluded, capped = rp.graphPrepareLast(ctx)
        row = {"graph": name, "kout": kout, "prepare_ms": ms, "prepare_all_ms": all_ms, "pairs": pairs,
               "occluded": occluded, "capped": capped, "mean_degree": float(ocnt.double().mean().item()),
               "gather_bytes": (n * KG * D * 8) if diversify else 0, "search": search_rows(kout, oids, ocnt)}
        for s in row["search"]:                             # the raw graph's smallest ef with at least this recall
            match = next((r for r in raw["search"] if r["recall_at_10"] >= s["recall_at_10"]), None)
            s["raw_ef_at_equal_recall"] = match["ef"] if match else None
            s["raw_ms_at_equal_recall"] = match["ms"] if match else None
        prepared.append(row)
        del oids, odist, ocnt

    res = {"tool": "tools/graph_prepare_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median behind a warm-up",
           "workload": "c2: %d x %d float64, minLeaf %d, maxDepth %d, k = %d, %d queries, graph = knnGraph(%d trees, "
                       "k = %d) + 2 refinement rounds, seeds = %d nearest de-duplicated candidates of %d trees" %
                       (n, D, MINL, maxd, K, NQ, TREES, KG, SEED_K, SEED_TREES),
           "raw": [raw], "prepared": prepared}
    if parent:                                             # the raw graph's searches from another build, a fresh process
        cmd = [sys.executable, os.path.abspath(__file__), str(reps), "--raw-only"]
        if n != 1_000_000:
            cmd += ["--n", str(n)]
        pr = subprocess.run(cmd, env=dict(os.environ, RPTREE_HIP_LIB=os.path.abspath(parent)), stdout=subprocess.PIPE,
                            timeout=900)
        if pr.returncode != 0:
            raise SystemExit("the run on %s failed" % parent)
        row = json.loads(pr.stdout.decode().strip().splitlines()[-1])
        row["library"] = "parent commit (%s)" % os.path.basename(parent)
        res["raw"].append(row)
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
