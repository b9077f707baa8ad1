"""Cost of the certified L2 cut on dense f64 rows: rpt_knn_dev at C2 (1 M x 128 f64, 32 trees,
10 000 queries, k = 10) with flags 0 (the prefiltered path), with RPT_KNN_DEDUP (the all-f64 fused
kernel), with flags 0 under knn_no_pre32 (the all-f64 kernel, duplicates kept: the distinct-id keep)
and with knn_l2_exact (every query on the exact kernel), and the uncertified queries of each.
Timed with HIP events on the ctx stream, median of REPS behind a warm-up, alternating this build and
another build of the library (the parent commit's) in fresh child processes.

    python tools/knn_l2_cut_times.py PARENT_LIB [reps] [rounds]     -> profiles/knn_l2_cut_times.json
    python tools/knn_l2_cut_times.py --child [reps]                  (one library, one JSON line)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rp-tree_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, D, TREES, MINL, K, NQ = 1_000_000, 128, 32, 128, 10, 10_000


def child(reps):
    import torch
    import rptree_amd as rp
    from rptree_amd import _lib, gen

    dev = torch.device("cuda:0")
    ctx = rp.default_context()
    X = gen.normal_dense2_torch(1234, N, D, dev)
    Q = gen.normal_dense2_torch(4321, NQ, D, dev)
    torch.cuda.synchronize()
    cfg = rp.rpTreeCfg(MINL, N, D)
    ds = rp.Dataset.from_torch(ctx, X)
    qs = rp.Dataset.from_torch(ctx, Q)
    _, R = gen.forest_hyperplanes(1235137, TREES, cfg.fpMaxTreeDepth, cfg.fpProjNzDensity, D)
    f = rp._build(ctx, ds, R, cfg.fpMaxTreeDepth, MINL, rp.RPT_PROJ_AUTO)
    ids = torch.empty((NQ, K), dtype=torch.int32, device="cuda")
    dist = torch.empty((NQ, K), dtype=torch.float64, device="cuda")
    cnt = torch.empty((NQ,), dtype=torch.int32, device="cuda")
    L = _lib.lib()
    stream = torch.cuda.ExternalStream(ctx.stream)
    cases = [("flags_0", 0, {}), ("dedup", rp.RPT_KNN_DEDUP, {}), ("flags_0_no_pre32", 0, {"knn_no_pre32": 1}),
             ("flags_0_l2_exact", 0, {"knn_l2_exact": 1})]
    out = {}
    for label, flags, opts in cases:
        try:
            old = {name: ctx.set_option(name, v) for name, v in opts.items()}
        except Exception:                                  # (a build without the option)
            continue
        ts = []
        for rep in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            _lib.check(L.rpt_knn_dev(ctx._h, f._h, ds._h, qs._h, K, flags, ids.data_ptr(), dist.data_ptr(),
                                     cnt.data_ptr()))
            b.record(stream)
            b.synchronize()
            if rep:
                ts.append(a.elapsed_time(b))
        unc = rp.knn_last_uncertified(ctx)
        for name, v in old.items():
            ctx.set_option(name, v)
        out[label] = {"ms": sorted(ts)[len(ts) // 2], "all_ms": ts, "uncertified": int(unc),
                      "checksum": int(ids.to(torch.int64).sum().item())}
    print(json.dumps(out), flush=True)


def main():
    if sys.argv[1] == "--child":
        return child(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    parent = os.path.abspath(sys.argv[1])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    runs = {"this": [], "parent": []}
    for _ in range(rounds):
        for who in ("this", "parent"):
            env = dict(os.environ)
            if who == "parent":
                env["RPTREE_HIP_LIB"] = parent
            pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(reps)], env=env,
                                stdout=subprocess.PIPE, timeout=400)
            if pr.returncode != 0:
                raise SystemExit("the child on the %s library ended with status %d" % (who, pr.returncode))
            runs[who].append(json.loads(pr.stdout.decode().strip().splitlines()[-1]))
    res = {"tool": "tools/knn_l2_cut_times.py", "reps": reps, "rounds": rounds,
           "timing": "HIP events on the ctx stream around rpt_knn_dev, median behind a warm-up; child processes "
                     "alternate this build and the parent commit's library",
           "workload": "c2: %d x %d float64, %d trees, minLeaf %d, %d queries, k = %d" % (N, D, TREES, MINL, NQ, K),
           "runs": runs}
    print(json.dumps(res))
    with open(os.path.join(ROOT, "profiles", "knn_l2_cut_times.json"), "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
