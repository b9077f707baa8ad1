"""Allow-lists per query group (rpt_graph_search_allow_group_dev, rpt_knn_allow_group_dev,
rpt_brute_knn_allow_group_dev) at the C2 shape: 1 M x 128 float64, 32 trees, minLeaf 128, k = 10, 10 000
queries dealt to the groups round-robin; the graph and the seeds of tools/graph_search_allow_times.py.

    python tools/allow_group_times.py [reps] --parent-lib PATH [--parent-rev REV] [--out FILE] [--n N]
    python tools/allow_group_times.py --resources-only [--parent-rev REV]

Columns: G = 1, 16, 256 independent 10 % masks (np.random.default_rng(100 + g): the columns differ in the
number of bitmaps only) and 256 disjoint tenants that partition the rows.  Rows: graph search at ef 32 with
width 128 and 256, the forest query | RPT_KNN_DEDUP, the exhaustive kNN of the first 1 000 queries.
Steps, each a fresh child process under a time limit of its own; the run stops at the first non-zero exit:
  resources  no GPU: the compiler's register / LDS / scratch report (-Rpass-analysis=kernel-resource-usage,
             gfx950) of graph_search_allow_kernel, graph_search_csr_allow_kernel, allow_compact_kernel and
             brute_csr_kernel, from REV's sources (default HEAD~1) and from this tree's ->
             profiles/allow_group_resources.json
  prepare    this build: the graph and the seeds, left in a scratch directory
  grouped    this build: the grouped entry points, every row x column, and the single-bitmap entry point on
             the whole batch at G = 1 (yardstick b on this build)
  parent     the parent commit's library (PATH): (a) the per-group route, one single-bitmap call per group
             over that group's gathered queries, HIP events around all G calls; (b) the single-bitmap entry
             point on the whole batch at G = 1.  The checksums of (a), in query order, must be the grouped ones.
Timing: HIP events on the ctx stream, median of REPS behind a warm-up, all repetitions recorded.  Writes
profiles/allow_group_times.json.  No ratio is fixed in advance.
"""
import json
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rp-tree_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)

D, MINL, K, KG, KOUT, SEED, NQ, NQ_BRUTE, TREES, SEED_TREES, SEED_K = 128, 128, 10, 10, 20, 1234, 10_000, 1000, 32, 2, 8
EF, WIDTHS, FRAC = 32, (128, 256), 0.1
COLUMNS = (("G1", 1, "frac"), ("G16", 16, "frac"), ("G256", 256, "frac"), ("tenants256", 256, "tenants"))
NEW_SYMBOLS = ("rpt_graph_search_allow_group_dev", "rpt_graph_search_allow_group_host", "rpt_knn_allow_group_host",
               "rpt_knn_allow_group_dev", "rpt_allow_group_candidates_host", "rpt_brute_knn_allow_group_host",
               "rpt_brute_knn_allow_group_dev", "rpt_recall_hits_allow_group_host")
STEP_LIMIT_S = {"resources": 900, "prepare": 300, "grouped": 420, "parent": 540}
KERNELS = ("graph_search_allow_kernel", "graph_search_csr_allow_kernel", "allow_compact_kernel", "brute_csr_kernel")
SOURCES = ("graph_search.hip", "graph_search_csr.hip", "knn_allow.hip", "knn.hip")
FIELD = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
         "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds",
         "Occupancy [waves/SIMD]": "occupancy"}


# ------------------------------------------------------------------ the compiler's resource report (no GPU)
def resource_report(csrc):
    """kernel (demangled name) -> {sgprs, vgprs, agprs, scratch, lds, occupancy} of the SOURCES under csrc"""
    out = {}
    for src in SOURCES:
        pr = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                             "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                             os.path.join(csrc, src), "-o", os.devnull], capture_output=True, text=True)
        if pr.returncode != 0:
            raise SystemExit("hipcc failed on %s\n%s" % (src, pr.stderr[-2000:]))
        cur = None
        for ln in pr.stderr.splitlines():
            m = re.search(r"remark: (?:\S+: )?\s*(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|"
                          r"SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", ln)
            if not m:
                continue
            key, val = m.group(1), m.group(2)
            if key == "Function Name":
                name = subprocess.run(["c++filt", val], capture_output=True, text=True).stdout.strip() or val
                fam = [k for k in KERNELS if k + "<" in name or k + "(" in name]
                cur = None
                if fam:   # the kernel and its template arguments, without the parameter list; bool arguments as 0 / 1
                    at = name.find(fam[0])
                    short = name[at:name.find("(", at)].replace("true", "1").replace("false", "0")
                    cur = out.setdefault(short, {})
            elif cur is not None:
                cur[FIELD[key]] = int(val)
    return out


def step_resources(_n, _reps, _scratch, parent_rev):
    tmp = tempfile.mkdtemp(prefix="allow_group_src_")
    try:
        for rel in subprocess.run(["git", "-C", ROOT, "ls-tree", "-r", "--name-only", parent_rev, "rp-tree_amd/csrc",
                                   "include"], capture_output=True, text=True, check=True).stdout.split():
            dst = os.path.join(tmp, rel)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with open(dst, "wb") as fh:
                fh.write(subprocess.run(["git", "-C", ROOT, "show", "%s:%s" % (parent_rev, rel)], capture_output=True,
                                        check=True).stdout)
        before = resource_report(os.path.join(tmp, "rp-tree_amd", "csrc"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    after = resource_report(os.path.join(ROOT, "rp-tree_amd", "csrc"))
    fam = {}
    for k in KERNELS:
        b = {n: v for n, v in before.items() if k in n}
        a = {n: v for n, v in after.items() if k in n}
        keys = tuple(FIELD.values())
        fam[k] = {"instantiations_before": len(b), "instantiations_after": len(a),
                  "max_before": {x: max([v.get(x, 0) for v in b.values()] or [0]) for x in keys},
                  "max_after": {x: max([v.get(x, 0) for v in a.values()] or [0]) for x in keys},
                  "changed": {n: {"before": b[n], "after": a[n]} for n in sorted(b) if n in a and a[n] != b[n]},
                  "only_after": sorted(n for n in a if n not in b), "only_before": sorted(n for n in b if n not in a)}
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", parent_rev], capture_output=True, text=True).stdout.strip()
    return {"tool": "tools/allow_group_times.py --resources-only", "before": "sources of " + rev, "after": "this tree",
            "flags": "-O3 -ffp-contract=off --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage",
            "note": "instantiations are matched by kernel name and template arguments (bool arguments as 0 / 1: "
                    "brute_csr_kernel's ALLOW went from bool to int), without the parameter list; lds is the static "
                    "LDS, the search kernels' beam is dynamic; only_after: the new instantiations (brute_csr_kernel "
                    "with ALLOW = 2)",
            "families": fam}


# ------------------------------------------------------------------ the GPU steps
def event_ms(torch, stream, fn, reps):
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
    return sorted(ts)[len(ts) // 2], ts


def setup(n, trees, parent_lib=""):
    import torch
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
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    _, R = gen.forest_hyperplanes(1235137, TREES, maxd, pnz, D)
    f = rp._build(ctx, ds, R[:trees], maxd, MINL, rp.RPT_PROJ_MFMA)
    return torch, rp, ctx, dev, X, Q, ds, qd, f, R, maxd


def column_masks(np, kind, G, n):
    if kind == "tenants":
        owner = np.random.default_rng(9).integers(0, G, size=n)
        return [owner == g for g in range(G)]
    return [np.random.default_rng(100 + g).random(n) < FRAC for g in range(G)]


def outputs(torch, dev, nq, k):
    return (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float64, device=dev),
            torch.empty((nq,), dtype=torch.int32, device=dev))


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.cpu().numpy().tobytes(), c)
    return c


def step_prepare(n, reps, scratch, _):
    import numpy as np
    torch, rp, ctx, dev, X, Q, ds, qd, f, R, maxd = setup(n, TREES)
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
    f2 = rp._build(ctx, ds, R[:SEED_TREES], maxd, MINL, rp.RPT_PROJ_MFMA)
    sids, sdist, scnt = outputs(torch, dev, NQ, SEED_K)
    torch.cuda.synchronize(dev)
    rp.knnAllowDev(0, SEED_K, f2, qd, sids.data_ptr(), sdist.data_ptr(), scnt.data_ptr(), dedup=True)
    seeds = torch.where(torch.arange(SEED_K, device=dev)[None, :] < scnt[:, None], sids, torch.full_like(sids, -1))
    for name, t in (("gids", gids), ("gcnt", gcnt), ("seeds", seeds)):
        np.save(os.path.join(scratch, name + ".npy"), t.cpu().numpy())
    return {"n": n, "maxDepth": maxd, "mean_degree": float(gcnt.double().mean()), "perm_crc": zlib.crc32(f.perm.tobytes())}


def measure(n, reps, scratch, parent_lib):
    """both GPU steps: with parent_lib the per-group route (a) and G = 1 (b); without, the grouped entry points and (b)"""
    import numpy as np
    torch, rp, ctx, dev, X, Q, ds, qd, f, R, maxd = setup(n, TREES, parent_lib)
    gids, gcnt, seeds = (torch.from_numpy(np.load(os.path.join(scratch, name + ".npy"))).to(dev)
                         for name in ("gids", "gcnt", "seeds"))
    qb = rp.Dataset.from_torch(ctx, Q[:NQ_BRUTE])
    ids, dist, cnt = outputs(torch, dev, NQ, K)
    torch.cuda.synchronize(dev)
    out = {"perm_crc": zlib.crc32(f.perm.tobytes()), "columns": {}}

    def single(words_ptr, queries, sd, nq_, o, which):
        """one single-bitmap call on `queries` (a Dataset of nq_ rows) into the outputs o"""
        if which.startswith("graph"):
            rp.graphSearchAllowDev(ds, queries, KOUT, gids.data_ptr(), gcnt.data_ptr(), SEED_K, sd.data_ptr(), words_ptr, K,
                                   EF, int(which[5:]), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        elif which == "forest":
            rp.knnAllowDev(words_ptr, K, f, queries, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), dedup=True)
        else:
            rp.bruteKnnAllowDev(words_ptr, ds, queries, K, o[0].data_ptr(), o[1].data_ptr())

    rows = ["graph%d" % w for w in WIDTHS] + ["forest", "brute"]
    for col, G, kind in COLUMNS:
        masks = column_masks(np, kind, G, n)
        words = torch.from_numpy(rp.allowBitmaps(masks, n).view(np.int32).copy()).to(dev)
        group_h = (np.arange(NQ) % G).astype(np.int32)
        group = torch.from_numpy(group_h).to(dev)
        torch.cuda.synchronize(dev)
        res = {"G": G, "allowed_rows_per_bitmap": float(np.mean([m.sum() for m in masks]))}
        for which in rows:
            nq_ = NQ_BRUTE if which == "brute" else NQ
            queries = qb if which == "brute" else qd
            o = (ids[:nq_], dist[:nq_], cnt[:nq_])
            parts = o[:2] if which == "brute" else o
            r = {}
            if not parent_lib:
                def grouped():
                    if which.startswith("graph"):
                        rp.graphSearchAllowGroupDev(ds, queries, KOUT, gids.data_ptr(), gcnt.data_ptr(), SEED_K,
                                                    seeds.data_ptr(), words.data_ptr(), G, group.data_ptr(), K, EF,
                                                    int(which[5:]), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
                    elif which == "forest":
                        rp.knnAllowGroupDev(words.data_ptr(), G, group.data_ptr(), K, f, queries, o[0].data_ptr(),
                                            o[1].data_ptr(), o[2].data_ptr(), dedup=True)
                    else:
                        rp.bruteKnnAllowGroupDev(words.data_ptr(), G, group.data_ptr(), ds, queries, K, o[0].data_ptr(),
                                                 o[1].data_ptr())
                ms, all_ms = event_ms(torch, ctx.stream, grouped, reps)
                ctx.sync()
                r["grouped"] = {"ms": ms, "all_ms": all_ms, "crc": crc(*parts)}
            else:                                            # (a): the queries gathered by group, one call per group
                calls = []
                for g in range(G):
                    sel = torch.from_numpy(np.flatnonzero(group_h[:nq_] == g)).to(dev)
                    if len(sel) == 0:
                        continue
                    qg = Q[:nq_].index_select(0, sel).contiguous()
                    sg = seeds[:nq_].index_select(0, sel).contiguous()
                    og = outputs(torch, dev, len(sel), K)
                    calls.append((sel, qg, rp.Dataset.from_torch(ctx, qg), sg, og, words[g].data_ptr()))
                torch.cuda.synchronize(dev)

                def per_group():
                    for sel, qg, dq, sg, og, wp in calls:
                        single(wp, dq, sg, len(sel), og, which)
                ms, all_ms = event_ms(torch, ctx.stream, per_group, reps)
                ctx.sync()
                for sel, qg, dq, sg, og, wp in calls:
                    for dst, src in zip(parts, og):
                        dst.index_copy_(0, sel, src)
                torch.cuda.synchronize(dev)
                r["per_group_calls"] = {"ms": ms, "all_ms": all_ms, "calls": len(calls), "crc": crc(*parts),
                                        "note": "the gathers of queries and seeds are outside the timed region"}
                for c in calls:
                    c[2].close()
            if G == 1:                                       # (b): the single-bitmap entry point on the whole batch
                ms, all_ms = event_ms(torch, ctx.stream, lambda: single(words[0].data_ptr(), queries, seeds, nq_, o, which),
                                      reps)
                ctx.sync()
                r["single_bitmap_whole_batch"] = {"ms": ms, "all_ms": all_ms, "crc": crc(*parts)}
            res[which] = r
        out["columns"][col] = res
    return out


def step_grouped(n, reps, scratch, _):
    return measure(n, reps, scratch, "")


def step_parent(n, reps, scratch, parent_lib):
    return measure(n, reps, scratch, parent_lib)


STEPS = {"resources": step_resources, "prepare": step_prepare, "grouped": step_grouped, "parent": step_parent}


def run_step(name, n, reps, scratch, arg):
    limit = STEP_LIMIT_S[name]                              # the step ends at its own limit, whatever this process does
    pr = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
                         str(n), str(reps), scratch, arg], capture_output=True, text=True)
    if pr.returncode in (124, 137):
        raise SystemExit("step %s ran out of its %d s: nothing recorded" % (name, limit))
    if pr.returncode != 0:
        raise SystemExit("step %s failed (%d): nothing recorded\n%s%s" % (name, pr.returncode, pr.stdout[-3000:],
                                                                          pr.stderr[-3000:]))
    print("step %s done" % name, file=sys.stderr, flush=True)
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, n, reps, scratch, arg = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
        print(json.dumps(STEPS[name](n, reps, scratch, arg)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    parent = opt("--parent-lib", None)
    rev = opt("--parent-rev", "HEAD~1")
    out_path = opt("--out", os.path.join(ROOT, "profiles", "allow_group_times.json"))
    n = int(opt("--n", 1_000_000))
    only = "--resources-only" in args
    if only:
        args.remove("--resources-only")
    skip_resources = "--no-resources" in args
    if skip_resources:
        args.remove("--no-resources")
    reps = int(args[0]) if args else 5
    if not skip_resources:
        report = run_step("resources", 0, 0, "-", rev)
        with open(os.path.join(ROOT, "profiles", "allow_group_resources.json"), "w") as fh:
            fh.write(json.dumps(report, indent=1) + "\n")
    if only:
        return
    if not parent:
        raise SystemExit("--parent-lib PATH is required: the yardsticks are the parent commit's library")
    parent = os.path.abspath(parent)
    scratch = tempfile.mkdtemp(prefix="allow_group_")
    res = {"tool": "tools/allow_group_times.py", "reps": reps, "n": n,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up, all repetitions recorded; one child "
                     "process per step",
           "workload": "C2: %d x %d float64, %d trees, minLeaf %d, k = %d, %d queries dealt to the groups round-robin "
                       "(exhaustive kNN: the first %d); graph: knnGraph(%d) + 2 refinement rounds + graphPrepare(reverse "
                       "union, %d columns), seeds = %d nearest of %d trees; columns: G independent %g masks, or 256 "
                       "tenants that partition the rows" % (n, D, TREES, MINL, K, NQ, NQ_BRUTE, KG, KOUT, SEED_K,
                                                            SEED_TREES, FRAC)}
    try:                                                    # a step that fails raises: nothing further starts
        res["prepare"] = run_step("prepare", n, reps, scratch, "")
        res["this_build"] = run_step("grouped", n, reps, scratch, "")
        res["parent_library"] = run_step("parent", n, reps, scratch, parent)
        if len({res[s]["perm_crc"] for s in ("prepare", "this_build", "parent_library")}) != 1:
            raise SystemExit("this build and the parent's library built different forests")
        agree = {}
        for col, _, _ in COLUMNS:
            for which, r in res["this_build"]["columns"][col].items():
                if isinstance(r, dict) and "grouped" in r:
                    agree["%s %s" % (col, which)] = \
                        r["grouped"]["crc"] == res["parent_library"]["columns"][col][which]["per_group_calls"]["crc"]
        res["grouped_checksum_is_the_per_group_route_s"] = agree
        if not all(agree.values()):
            raise SystemExit("a grouped answer differs from the per-group route: %s" % [k for k, v in agree.items() if not v])
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
