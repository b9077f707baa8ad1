"""Preparing the kNN graph for the search on SVector (CSR) rows (rpt_graph_prepare_csr_dev,
graph_diversify_csr_kernel in csrc/graph_prepare.hip) at the C3 shape of tools/graph_search_csr_times.py:
1 M x 784, density 0.19, U(0,1] values, 32 trees, minLeaf 128, k = 10, 10 000 queries of the same kind.

    python tools/graph_prepare_csr_times.py [reps] [--out FILE] [--n N]

Two steps, each a fresh child process under a time limit of its own (a step that fails or runs out of
time ends the run; nothing is recorded then):
  csr     the truth (bruteKnn on the CSR rows), the graph (knnGraphSV of the 32 trees + 2
          knnGraphRefineSV rounds), the seeds (rpt_knn_dev on the first 2 trees, 8 nearest,
          de-duplicated); rpt_graph_prepare_csr_dev with diversify (kout 10), reverse (kout 20) and both
          (kout 20), each with graph_prepare_csr_resident = 0 and -1; rpt_graph_search_csr_dev at ef =
          16 / 32 / 64 / 128 on the raw graph and on each prepared graph
  dense   rpt_graph_prepare_dev on the dense-ified rows (6.3 GB more) and the graph of the csr step, the
          same three flag combinations
The csr step leaves the graph in a scratch directory for the other.  Both steps draw the same rows; the
dense preparation must report the checksums and the statistics of the CSR one (the contract:
bit-equal), and so must the CSR preparation with no point resident.  There is no earlier device route
for this step to compare against; the yardsticks are the dense kernel of the same run and the search on
the raw graph.  Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  Writes
profiles/graph_prepare_csr_times.json.  No ratio is fixed in advance: the file holds what was measured.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rp-tree_amd", "python"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graph_search_csr_times import (D, DENSITY, T, MINL, K, KG, SEED, NQ, SEED_TREES, SEED_K, EFS,  # noqa: E402
                                    RPT_PROJ_AUTO, RPT_KNN_DEDUP, sparse_uniform_device, densify_device, cfg_of,
                                    event_ms, recall_of, answer_crc, outputs)
from rptree_amd import gen  # noqa: E402

# name -> (diversify, reverse, kout)
CONFIGS = {"diversify": (True, False, 10), "reverse": (False, True, 20), "both": (True, True, 20)}
STEP_LIMIT_S = {"csr": 400, "dense": 300}


def graph_outputs(dev, n, kout):
    return (torch.empty((n, kout), dtype=torch.int32, device=dev), torch.empty((n, kout), dtype=torch.float64, device=dev),
            torch.empty((n,), dtype=torch.int32, device=dev))


# ------------------------------------------------------------------ the CSR rows
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
    L, vp = _lib.lib(), _lib.vp

    f = rp._build(ctx, ds, R, maxd, MINL, RPT_PROJ_AUTO)
    gids, gdist, gcnt = graph_outputs(dev, n, KG)
    torch.cuda.synchronize(dev)
    rp.knnGraphSVDev(KG, f, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr())
    rp.knnGraphRefineSVDev(KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), iters=2)
    ctx.sync()
    f.close()
    for name, t in (("gids", gids), ("gdist", gdist), ("gcnt", gcnt)):
        np.save(os.path.join(scratch, name + ".npy"), t.cpu().numpy())
    lens = (rowptr[1:] - rowptr[:-1])
    valid = torch.arange(KG, device=dev)[None, :] < gcnt[:, None]
    entries = (lens[gids.clamp(min=0).long()] * valid).sum(dim=1)   # per point: what the kernel compares with the cap

    # the seeds: 8 nearest de-duplicated candidates of the first 2 trees
    f2 = rp._build(ctx, ds, R[:SEED_TREES], maxd, MINL, RPT_PROJ_AUTO)
    sids, sdist, scnt = (torch.empty((NQ, SEED_K), dtype=torch.int32, device=dev),
                         torch.empty((NQ, SEED_K), dtype=torch.float64, device=dev),
                         torch.empty((NQ,), dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    _lib.check(L.rpt_knn_dev(ctx._h, f2._h, ds._h, qd._h, SEED_K, RPT_KNN_DEDUP, vp(sids.data_ptr()),
                             vp(sdist.data_ptr()), vp(scnt.data_ptr())))
    ctx.sync()
    seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < scnt[:, None], sids,
                        torch.full_like(sids, -1)).contiguous()
    torch.cuda.synchronize(dev)
    ids, dist, cnt = outputs(dev)

    def search_rows(kg, g_ids, g_cnt):
        rows = []
        for ef in EFS:
            def run():
                rp.graphSearchSVDev(ds, qd, kg, g_ids.data_ptr(), g_cnt.data_ptr(), SEED_K, seeds.data_ptr(), K, ef,
                                    ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            ms, all_ms = event_ms(ctx.stream, run, reps)
            ctx.sync()
            expansions, evaluated = rp.graphSearchLast(ctx)
            rows.append({"ef": ef, "ms": ms, "all_ms": all_ms, "recall_at_10": recall_of(ids.cpu().numpy(), truth),
                         "evaluated_per_query": evaluated / NQ, "expansions_per_query": expansions / NQ})
        return rows

    res = {"n": n, "nnz": int(val.numel()), "maxDepth": maxd,
           "neighbour_entries": {"mean": float(entries.double().mean()), "max": int(entries.max()),
                                 "share_resident_at_1536": float((entries <= 1536).double().mean())},
           "raw": {"mean_degree": float(gcnt.double().mean()), "search": search_rows(KG, gids, gcnt)}, "prepare": {}}
    for name, (div, rev, kout) in CONFIGS.items():
        oi, od, oc = graph_outputs(dev, n, kout)
        torch.cuda.synchronize(dev)

        def run():
            rp.graphPrepareSVDev(KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), kout, oi.data_ptr(),
                                 od.data_ptr(), oc.data_ptr(), diversify=div, reverse=rev)
        row = {"kout": kout}
        for tag, setting in (("resident", 0), ("global", -1)):
            old = ctx.set_option("graph_prepare_csr_resident", setting)
            try:
                ms, all_ms = event_ms(ctx.stream, run, reps)
                ctx.sync()
            finally:
                ctx.set_option("graph_prepare_csr_resident", old)
            stats, crc = rp.graphPrepareLast(ctx), answer_crc(oi, od, oc)
            if tag == "global" and (crc != row["crc"] or list(stats) != row["stats"]):
                raise SystemExit("graph_prepare_csr_resident = -1 changed the answer of %s" % name)
            row.update({tag + "_ms": ms, tag + "_all_ms": all_ms, "crc": crc, "stats": list(stats)})
        row["mean_degree"] = float(oc.double().mean())
        row["search"] = search_rows(kout, oi, oc)
        res["prepare"][name] = row
    return res


# ------------------------------------------------------------------ the dense-ified rows
def step_dense(n, reps, scratch):
    import rptree_amd as rp
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    rowptr, col, val = sparse_uniform_device(dev, n, D, DENSITY, SEED)
    X = densify_device(dev, n, rowptr, col, val)
    del rowptr, col, val
    torch.cuda.synchronize(dev)
    ds = rp.Dataset.from_torch(ctx, X)
    gids, gdist, gcnt = (torch.from_numpy(np.load(os.path.join(scratch, name + ".npy"))).to(dev)
                         for name in ("gids", "gdist", "gcnt"))
    res = {}
    for name, (div, rev, kout) in CONFIGS.items():
        oi, od, oc = graph_outputs(dev, n, kout)
        torch.cuda.synchronize(dev)

        def run():
            rp.graphPrepareDev(KG, ds, gids.data_ptr(), gdist.data_ptr(), gcnt.data_ptr(), kout, oi.data_ptr(),
                               od.data_ptr(), oc.data_ptr(), diversify=div, reverse=rev)
        ms, all_ms = event_ms(ctx.stream, run, reps)
        ctx.sync()
        res[name] = {"ms": ms, "all_ms": all_ms, "crc": answer_crc(oi, od, oc), "stats": list(rp.graphPrepareLast(ctx))}
    return res


def run_step(name, n, reps, scratch):
    limit = STEP_LIMIT_S[name]                              # the step ends at its own limit, whatever this process does
    pr = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                         str(n), str(reps), scratch], capture_output=True, text=True)
    if pr.returncode in (124, 137):
        raise SystemExit("step %s ran out of its %d s: nothing recorded" % (name, limit))
    if pr.returncode != 0:
        raise SystemExit("step %s failed (%d): nothing recorded\n%s%s" % (name, pr.returncode, pr.stdout, pr.stderr))
    print("step %s done" % name, file=sys.stderr, flush=True)
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, n, reps, scratch = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        print(json.dumps({"csr": step_csr, "dense": step_dense}[name](n, reps, scratch)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    out_path = opt("--out", os.path.join(ROOT, "profiles", "graph_prepare_csr_times.json"))
    n = int(opt("--n", 1_000_000))
    reps = int(args[0]) if args else 5
    scratch = tempfile.mkdtemp(prefix="graph_prepare_csr_")
    try:                                                    # a step that fails raises: nothing further starts
        csr = run_step("csr", n, reps, scratch)
        den = run_step("dense", n, reps, scratch)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    for name, row in csr["prepare"].items():
        if row["crc"] != den[name]["crc"] or row["stats"] != den[name]["stats"]:
            raise SystemExit("%s: the CSR and the dense-ified preparations differ" % name)
        row["dense_ms"], row["dense_all_ms"] = den[name]["ms"], den[name]["all_ms"]
    res = {"tool": "tools/graph_prepare_csr_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step",
           "workload": "C3: %d x %d CSR f64, density %.2f (%d nonzeros), %d queries of the same kind, minLeaf %d, "
                       "maxDepth %d, k = %d, graph = knnGraphSV(%d trees, k = %d) + 2 refinement rounds, seeds = %d "
                       "nearest de-duplicated candidates of %d trees" %
                       (n, D, DENSITY, csr["nnz"], NQ, MINL, csr["maxDepth"], K, T, KG, SEED_K, SEED_TREES),
           "neighbour_entries": csr["neighbour_entries"], "raw": csr["raw"], "prepare": csr["prepare"],
           "bit_equal": "for every flag combination rpt_graph_prepare_dev on the dense-ified rows gave the checksum "
                        "and the statistics of rpt_graph_prepare_csr_dev's answer, and so did "
                        "graph_prepare_csr_resident = -1"}
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
