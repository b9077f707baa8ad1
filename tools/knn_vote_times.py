"""Vote-threshold kNN (rpt_knn_vote_dev: csrc/knn_vote.hip vote_select_kernel + the general kernels) at
the C2 shape: 1 M x 128, 32 trees, minLeaf 128, k = 10, 10 000 queries, v in 1 .. 4.

    python tools/knn_vote_times.py [reps] [--out FILE] [--n N] [--parent-lib PATH]

Steps, each a fresh child process under a time limit of its own (a step that fails or runs out of time
ends the run; nothing is recorded then):
  f64         f64 rows under L2: rpt_knn_vote_dev, this build's rpt_knn_dev | RPT_KNN_VOTE(v) (the fused
              path; the same checksums expected), rpt_knn_dev without voting; recall@10 of each against
              rpt_brute_knn_dev on the first 1 000 queries; voted ids per query; the vote-select kernel
              alone (rpt_prof_* class 5) on its LDS path and, with knn_vote_lds = 1, on its global path
  f64_parent  --parent-lib only: the same rows through another build of the library (the parent commit's)
              on rpt_knn_dev | RPT_KNN_VOTE(v) and without voting: the yardstick of the cell that existed
  f32cos      f32 rows under cosine: rpt_knn_vote_dev against rpt_knn_dev | RPT_KNN_METRIC_COSINE
Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  Writes
profiles/knn_vote_times.json.  No ratio is fixed in advance.
"""
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

import torch  # noqa: E402

D, T, MINL, K, SEED, NQ, NQ_TRUTH = 128, 32, 128, 10, 1234, 10000, 1000
VS = (1, 2, 3, 4)
NEW_SYMBOLS = ("rpt_knn_vote_host", "rpt_knn_vote_dev", "rpt_vote_candidates_host", "rpt_knn_last_voted")
STEP_LIMIT_S = 400


def event_ms(stream, fn, reps):
    """median HIP-event time of fn() on the ctx stream, behind one warm-up"""
    s = torch.cuda.ExternalStream(stream)
    fn()
    s.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts


def crc(*tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.cpu().numpy().tobytes(), c)
    return c


def step(name, n, reps, parent_lib):
    from rptree_amd import _lib
    parent = name == "f64_parent"
    if parent:                       # another build of the library: it lacks the new symbols
        _lib.LIB_PATH = parent_lib
        for s in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(s)
    import rptree_amd as rp
    from rptree_amd import gen
    L = _lib.lib()
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    g = torch.Generator(device=dev).manual_seed(SEED)
    dt = torch.float32 if name == "f32cos" else torch.float64
    X = torch.randn((n, D), dtype=torch.float64, device=dev, generator=g).to(dt)
    Q = (X[:NQ].to(torch.float64) * 1.002 + 0.004 * torch.randn((NQ, D), dtype=torch.float64, device=dev,
                                                               generator=g)).to(dt)
    torch.cuda.synchronize(dev)
    ds, qs = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, Q)
    qt = rp.Dataset.from_torch(ctx, Q[:NQ_TRUTH])
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))            # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, D)
    f = rp._build(ctx, ds, R, maxd, MINL, rp.RPT_PROJ_AUTO)
    ki = torch.empty((NQ, K), dtype=torch.int32, device=dev)
    kd = torch.empty((NQ, K), dtype=torch.float64, device=dev)
    kc = torch.empty((NQ,), dtype=torch.int32, device=dev)
    ti = torch.empty((NQ_TRUTH, K), dtype=torch.int32, device=dev)
    td = torch.empty((NQ_TRUTH, K), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    vp = C.c_void_p
    metric = rp.RPT_KNN_METRIC_COSINE if name == "f32cos" else 0
    _lib.check(L.rpt_brute_knn_dev(ctx._h, ds._h, qt._h, K, metric, vp(ti.data_ptr()), vp(td.data_ptr())))
    ctx.sync()
    truth = ti.cpu().numpy()

    def recall():
        got = ki[:NQ_TRUTH].cpu().numpy()
        return float(sum(len(set(got[i]) & set(truth[i])) for i in range(NQ_TRUTH))) / (K * NQ_TRUTH)

    def old(flags):
        _lib.check(L.rpt_knn_dev(ctx._h, f._h, ds._h, qs._h, K, flags, vp(ki.data_ptr()), vp(kd.data_ptr()),
                                 vp(kc.data_ptr())))

    def new(v):
        _lib.check(L.rpt_knn_vote_dev(ctx._h, f._h, ds._h, qs._h, K, v, metric, vp(ki.data_ptr()), vp(kd.data_ptr()),
                                      vp(kc.data_ptr())))

    out = {"n": n, "maxDepth": maxd, "perm_crc": zlib.crc32(f.perm.tobytes())}

    def record(tag, fn):
        ms, all_ms = event_ms(ctx.stream, fn, reps)
        ctx.sync()
        out[tag] = {"ms": ms, "all_ms": all_ms, "crc": crc(ki, kd, kc), "recall_at_10": recall()}
        return out[tag]

    record("knn_no_vote", lambda: old(metric))
    cand = C.c_int64()
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(cand)))
    out["candidates_per_query"] = cand.value / NQ
    for v in VS:
        if name != "f32cos":
            record("knn_flag_v%d" % v, lambda: old(v << 8))
        if parent:
            continue
        r = record("knn_vote_v%d" % v, lambda: new(v))
        voted = C.c_int64()
        _lib.check(L.rpt_knn_last_voted(ctx._h, C.byref(voted)))
        r["voted_per_query"] = voted.value / NQ
        r["uncertified"] = rp.knn_last_uncertified(ctx)
        if name == "f64":            # the vote-select kernel alone, on both of its paths
            for lds in (0, 1):
                prev = ctx.set_option("knn_vote_lds", lds)
                new(v)
                _lib.check(L.rpt_prof_enable(ctx._h, 1))
                ts = []
                for _ in range(reps):
                    _lib.check(L.rpt_prof_reset(ctx._h))
                    new(v)
                    ms, launches = C.c_double(), C.c_int64()
                    _lib.check(L.rpt_prof_get(ctx._h, 5, C.byref(ms), C.byref(launches)))
                    ts.append(ms.value)
                _lib.check(L.rpt_prof_enable(ctx._h, 0))
                ctx.set_option("knn_vote_lds", prev)
                ts.sort()
                r["select_ms_lds" if lds == 0 else "select_ms_global"] = ts[len(ts) // 2]
    return out


def run_step(name, n, reps, parent_lib):
    try:
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(n), str(reps), parent_lib],
                            capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit("step %s ran out of its %d s: nothing recorded" % (name, STEP_LIMIT_S))
    if pr.returncode != 0:
        raise SystemExit("step %s failed (%d): nothing recorded\n%s%s" % (name, pr.returncode, pr.stdout, pr.stderr))
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        print(json.dumps(step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    out_path = opt("--out", os.path.join(ROOT, "profiles", "knn_vote_times.json"))
    n = int(opt("--n", 1_000_000))
    parent_lib = opt("--parent-lib", "")
    reps = int(args[0]) if args else 5
    res = {"tool": "tools/knn_vote_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step; "
                     "select_ms_*: rpt_prof_* class 5 (the vote-select kernel alone)",
           "workload": "C2: %d x %d, %d trees, minLeaf %d, k = %d, %d queries (recall@10 on the first %d against "
                       "the exhaustive search)" % (n, D, T, MINL, K, NQ, NQ_TRUTH)}
    res["f64"] = run_step("f64", n, reps, "")
    res["f64_parent"] = run_step("f64_parent", n, reps, parent_lib) if parent_lib else "not measured"
    res["f32cos"] = run_step("f32cos", n, reps, "")
    same = []
    for v in VS:
        crcs = {res["f64"]["knn_vote_v%d" % v]["crc"], res["f64"]["knn_flag_v%d" % v]["crc"]}
        if parent_lib and res["f64_parent"]["perm_crc"] == res["f64"]["perm_crc"]:
            crcs.add(res["f64_parent"]["knn_flag_v%d" % v]["crc"])
        same.append(len(crcs) == 1)
    res["bit_equal_f64"] = same            # rpt_knn_vote_dev against RPT_KNN_VOTE(v), per v
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
