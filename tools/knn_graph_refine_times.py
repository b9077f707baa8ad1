"""NN-descent rounds over the kNN graph (rpt_knn_graph_refine_dev, csrc/graph_refine.hip) at C2.

    python tools/knn_graph_refine_times.py [reps] [--n N] [--out FILE]

C2 = the flagship shape (seeds of BASELINE configs[1]: 1 M x 128 f64, rpTreeCfg depth, minLeaf 128),
k = 10, reverse = 10.  Everything is timed with HIP events on the ctx stream, median of REPS behind a
warm-up.  Two tables go to profiles/knn_graph_refine_times.json:
  rounds   per refinement round over the 4-tree graph: ms, candidates (= distances evaluated), the
           bytes their gathers move (candidates x d x 8) and that as a fraction of the 4.85 TB/s the
           README reports for 128-byte gathers on this memory system
  recall   recall@10 against bruteKnn (k + 1, the point itself removed) on 10 000 sampled points and
           the total time, for knnGraph with 4 / 8 / 16 / 32 trees (unchanged code: the baseline, its
           32-tree time is the check that the run is comparable with the README's 129.3 ms) and for
           4 / 8 trees followed by 1, 2, 3 rounds
--n N shrinks the data set (a rehearsal; nothing is written unless --out is given).
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rp-tree_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rptree_amd as rp  # noqa: E402
from rptree_amd import _lib, gen  # noqa: E402

D, MINL, K, REVERSE, SEED, SAMPLE = 128, 128, 10, 10, 1234, 10_000
GATHER_RATE = 4.85e12  # bytes / s, 128-byte gathers (README)


def event_ms(stream, fn, reps, before=None):
    """median HIP-event time of fn() on the ctx stream, behind one warm-up; before() is not timed"""
    s = torch.cuda.ExternalStream(stream)
    ts = []
    for rep in range(reps + 1):
        if before:
            before()
            torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        if rep:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n, out_path = 1_000_000, os.path.join(ROOT, "profiles", "knn_graph_refine_times.json")
    rehearsal = "--n" in sys.argv
    if rehearsal:
        v = sys.argv[sys.argv.index("--n") + 1]
        n = int(v)
        args.remove(v)
        out_path = None
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args.remove(out_path)
    reps = int(args[0]) if args else 5
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    X = gen.normal_dense2_torch(SEED, n, D, dev)
    torch.cuda.synchronize(dev)
    ds = rp.Dataset.from_torch(ctx, X)
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))           # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    _, R = gen.forest_hyperplanes(1235137, 32, maxd, pnz, D)

    sel = np.sort(np.random.default_rng(7).choice(n, min(SAMPLE, n), replace=False)).astype(np.int64)
    sel_dev = torch.from_numpy(sel).to(dev)
    truth, _ = rp.bruteKnn(ds, rp.Dataset.from_torch(ctx, X[sel_dev].contiguous()), K + 1)
    truth = [[j for j in row if j != i][:K] for i, row in zip(sel.tolist(), truth.tolist())]

    ids = torch.empty((n, K), dtype=torch.int32, device=dev)
    dist = torch.empty((n, K), dtype=torch.float64, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    keep = [torch.empty_like(t) for t in (ids, dist, cnt)]
    torch.cuda.synchronize(dev)
    ptrs = (ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())

    def recall():
        rows = ids[sel_dev].cpu().numpy().tolist()
        return float(np.mean([len(set(t) & set(r)) / K for t, r in zip(truth, rows)]))

    def save():
        for a, b in zip(keep, (ids, dist, cnt)):
            a.copy_(b)

    def restore():
        for a, b in zip(keep, (ids, dist, cnt)):
            b.copy_(a)

    rounds_tab, recall_tab = [], []
    for T in (4, 8, 16, 32):
        f = rp._build(ctx, ds, R[:T], maxd, MINL, rp.RPT_PROJ_MFMA)
        graph_ms, graph_all = event_ms(ctx.stream, lambda: rp.knnGraphDev(K, f, *ptrs), reps)
        ctx.sync()
        recall_tab.append({"trees": T, "rounds": 0, "graph_ms": graph_ms, "refine_ms": 0.0, "total_ms": graph_ms,
                           "recall_at_10": recall(), "graph_all_ms": graph_all})
        if T <= 8:
            total = 0.0
            for rnd in (1, 2, 3):
                save()                                     # the graph this round starts from
                ms, all_ms = event_ms(ctx.stream, lambda: rp.knnGraphRefineDev(K, ds, *ptrs, iters=1,
                                                                              reverse=REVERSE), reps, before=restore)
                ctx.sync()
                _, updates, cands = rp.knnGraphRefineLast(ctx)
                total += ms
                recall_tab.append({"trees": T, "rounds": rnd, "graph_ms": graph_ms, "refine_ms": total,
                                   "total_ms": graph_ms + total, "recall_at_10": recall()})
                if T == 4:
                    nbytes = cands * D * 8
                    rounds_tab.append({"round": rnd, "ms": ms, "all_ms": all_ms, "candidates": cands,
                                       "candidates_per_point": cands / n, "updates": updates,
                                       "gather_bytes": nbytes,
                                       "fraction_of_gather_rate": nbytes / (ms * 1e-3) / GATHER_RATE})
        _lib.check(_lib.lib().rpt_ctx_trim(ctx._h))
        f.close()
    res = {"tool": "tools/knn_graph_refine_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median behind a warm-up",
           "workload": "c2: %d x %d float64, minLeaf %d, maxDepth %d, k = %d, reverse = %d, recall on %d sampled points" %
                       (n, D, MINL, maxd, K, REVERSE, len(sel)),
           "gather_rate_bytes_per_s": GATHER_RATE, "rounds": rounds_tab, "recall": recall_tab}
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
