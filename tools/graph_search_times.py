"""Beam search over the kNN graph (rpt_graph_search_dev, csrc/graph_search.hip) against the forest
query (rpt_knn_dev) at C2.

    python tools/graph_search_times.py [reps] [--n N] [--out FILE] [--parent-lib LIB.so]

C2 = the flagship shape (seeds of BASELINE configs[1]: 1 M x 128 f64, rpTreeCfg depth, minLeaf 128),
k = 10, 10 000 queries.  The graph is knnGraph of the 32-tree forest plus two refinement rounds; the
seeds are the de-duplicated 8 nearest candidates of the forest's FIRST 2 TREES (timed on their own);
the search runs with ef in {16, 32, 64, 128}.  Everything is timed with HIP events on the ctx stream,
median of REPS behind a warm-up.  profiles/graph_search_times.json gets, per ef: ms per batch,
recall@10 against bruteKnn and the distances evaluated per query; and, from the same run, ms and
recall@10 of rpt_knn_dev over all 32 trees with RPT_KNN_DEDUP, from this build and, with
--parent-lib, from another build of the library (the parent commit's: a child process started with
RPTREE_HIP_LIB, which runs only the forest query).
--n N shrinks the data set (a rehearsal; nothing is written unless --out is given).
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

KNN_ONLY = "--knn-only" in sys.argv
if KNN_ONLY:                                               # another build: it need not know the search yet
    for name in [s for s in _lib.SYMBOLS if s.startswith("rpt_graph_search")]:
        del _lib.SYMBOLS[name]

import rptree_amd as rp  # noqa: E402
from rptree_amd import gen  # noqa: E402

D, MINL, K, KG, SEED, NQ, TREES, SEED_TREES, SEED_K = 128, 128, 10, 10, 1234, 10_000, 32, 2, 8
EFS = (16, 32, 64, 128)


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
    n, out_path, parent = 1_000_000, os.path.join(ROOT, "profiles", "graph_search_times.json"), None
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

    ids = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    dist = torch.empty((NQ, K), dtype=torch.float64, device=dev)
    cnt = torch.empty((NQ,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    L = _lib.lib()
    vp = _lib.vp

    def knn_dev(forest, k, out_ids, out_dist, out_cnt):
        _lib.check(L.rpt_knn_dev(ctx._h, forest._h, ds._h, qd._h, k, rp.RPT_KNN_DEDUP, vp(out_ids.data_ptr()),
                                 vp(out_dist.data_ptr()), vp(out_cnt.data_ptr())))

    f = rp._build(ctx, ds, R, maxd, MINL, rp.RPT_PROJ_MFMA)
    knn_ms, knn_all = event_ms(ctx.stream, lambda: knn_dev(f, K, ids, dist, cnt), reps)
    ctx.sync()
    knn_row = {"library": os.path.basename(_lib.LIB_PATH), "trees": TREES, "ms": knn_ms, "all_ms": knn_all,
               "recall_at_10": recall_of(ids.cpu().numpy(), truth)}
    if KNN_ONLY:
        print(json.dumps(knn_row))
        return

    # the graph: the 32-tree forest's, two NN-descent rounds
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
    seed_ms, seed_all = event_ms(ctx.stream, lambda: knn_dev(f2, SEED_K, sids, sdist, scnt), reps)
    ctx.sync()
    seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < scnt[:, None], sids,
                        torch.full_like(sids, -1)).contiguous()
    torch.cuda.synchronize(dev)
    seed_recall = recall_of(sids.cpu().numpy(), truth)

    rows = []
    for ef in EFS:
        def run():
            rp.graphSearchDev(ds, qd, KG, gids.data_ptr(), gcnt.data_ptr(), SEED_K, seeds.data_ptr(), K, ef,
                              ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        expansions, evaluated = rp.graphSearchLast(ctx)
        rows.append({"ef": ef, "ms": ms, "all_ms": all_ms, "seeds_plus_search_ms": seed_ms + ms,
                     "recall_at_10": recall_of(ids.cpu().numpy(), truth),
                     "evaluated_per_query": evaluated / NQ, "expansions_per_query": expansions / NQ,
                     "gather_bytes": evaluated * D * 8})
    res = {"tool": "tools/graph_search_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median behind a warm-up",
           "workload": "c2: %d x %d float64, minLeaf %d, maxDepth %d, k = %d, %d queries, graph = knnGraph(%d trees, "
                       "k = %d) + 2 refinement rounds, seeds = %d nearest de-duplicated candidates of %d trees" %
                       (n, D, MINL, maxd, K, NQ, TREES, KG, SEED_K, SEED_TREES),
           "seeds": {"trees": SEED_TREES, "seed_k": SEED_K, "ms": seed_ms, "all_ms": seed_all,
                     "recall_at_10_of_the_seeds": seed_recall},
           "search": rows, "knn_dedup_32_trees": [knn_row]}
    if parent:                                             # the same forest query from another build, a fresh process
        cmd = [sys.executable, os.path.abspath(__file__), str(reps), "--knn-only"]
        if n != 1_000_000:
            cmd += ["--n", str(n)]
        pr = subprocess.run(cmd, env=dict(os.environ, RPTREE_HIP_LIB=os.path.abspath(parent)), stdout=subprocess.PIPE,
                            timeout=600)
        if pr.returncode != 0:
            raise SystemExit("the run on %s failed" % parent)
        row = json.loads(pr.stdout.decode().strip().splitlines()[-1])
        row["library"] = "parent commit (%s)" % os.path.basename(parent)
        res["knn_dedup_32_trees"].append(row)
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
