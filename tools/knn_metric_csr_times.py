"""Cosine / inner-product kNN on SVector (CSR) rows (rpt_knn_csr_metric_dev, rpt_brute_knn_csr_metric_dev,
csrc/knn.hip knn_metric_csr_kernel) at the C3 shape: 1 M x 784, density 0.19, U(0,1] values, 32 trees,
minLeaf 128, k = 10; 1 000 queries for the exhaustive search, 10 000 for the forest query.

    python tools/knn_metric_csr_times.py [reps] [--out FILE] [--n N]

Two steps, each a fresh child process under a time limit of its own (a step that fails or runs out
of time ends the run; nothing is recorded then):
  csr     the CSR rows: the new exhaustive search and forest query under both metrics, default and
          with knn_metric_exact = 1, next to this build's L2 on the same rows (rpt_brute_knn_dev;
          rpt_knn_dev on the default fused path and with knn_general = 1, the structurally equal kernel)
  dense   the dense-ified rows (6.3 GB more): rpt_brute_knn_dev and rpt_knn_dev under the metrics
Both steps draw the same rows, queries and hyperplanes.  The exhaustive answers must have the same
checksum (ids and distance bits); so must the forest queries when the two forests have the same perm.
Timing: HIP events on the ctx stream, median of REPS behind a warm-up.  knn_last_uncertified is
recorded next to each time.  Writes profiles/knn_metric_csr_times.json.  No ratio is fixed in advance.
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

D, DENSITY, T, MINL, K, SEED = 784, 0.19, 32, 128, 10, 1234
NQ_BRUTE, NQ_KNN = 1000, 10000
RPT_PROJ_AUTO = 0
STEP_LIMIT_S = {"csr": 540, "dense": 540}


def sparse_uniform_device(dev, n, d, density, seed):
    """bench.py's C3 rows: Bernoulli support + U(0,1] values, built on the device as CSR tensors"""
    g = torch.Generator(device=dev).manual_seed(seed)
    cols, counts = [], []
    for r0 in range(0, n, 100_000):
        m = torch.rand((min(100_000, n - r0), d), device=dev, generator=g) < density
        counts.append(m.sum(dim=1))
        cols.append(m.nonzero()[:, 1].to(torch.int32))
    col = torch.cat(cols)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.cat(counts), 0)
    val = 1.0 - torch.rand(col.numel(), dtype=torch.float64, device=dev, generator=g)
    return rowptr, col, val


def densify(dev, rowptr, col, val, n):
    X = torch.zeros((n, D), dtype=torch.float64, device=dev)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), rowptr[1:] - rowptr[:-1])
    X[rows, col.long()] = val
    return X


def cfg_of(n):
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))            # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    return maxd, pnz


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


def step(dense, n, reps):
    import rptree_amd as rp
    from rptree_amd import _lib, gen
    L = _lib.lib()
    ctx = rp.default_context()
    dev = torch.device("cuda", ctx.device)
    rowptr, col, val = sparse_uniform_device(dev, n, D, DENSITY, SEED)
    qr, qc, qv = sparse_uniform_device(dev, NQ_KNN, D, DENSITY, SEED + 1)
    eb = int(qr[NQ_BRUTE])
    maxd, pnz = cfg_of(n)
    _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, D)
    if dense:
        X, Q = densify(dev, rowptr, col, val, n), densify(dev, qr, qc, qv, NQ_KNN)
        torch.cuda.synchronize(dev)
        ds, qk = rp.Dataset.from_torch(ctx, X), rp.Dataset.from_torch(ctx, Q)
        qb = rp.Dataset.from_torch(ctx, Q[:NQ_BRUTE])
        knn_metric, brute_metric = L.rpt_knn_dev, L.rpt_brute_knn_dev
    else:
        ds = rp.Dataset.csr_from_torch(ctx, rowptr, col, val, D)
        qk = rp.Dataset.csr_from_torch(ctx, qr, qc, qv, D)
        qb = rp.Dataset.csr_from_torch(ctx, qr[:NQ_BRUTE + 1].clone(), qc[:eb].clone(), qv[:eb].clone(), D)
        knn_metric, brute_metric = L.rpt_knn_csr_metric_dev, L.rpt_brute_knn_csr_metric_dev
    f = rp._build(ctx, ds, R, maxd, MINL, RPT_PROJ_AUTO)
    bi = torch.empty((NQ_BRUTE, K), dtype=torch.int32, device=dev)
    bd = torch.empty((NQ_BRUTE, K), dtype=torch.float64, device=dev)
    ki = torch.empty((NQ_KNN, K), dtype=torch.int32, device=dev)
    kd = torch.empty((NQ_KNN, K), dtype=torch.float64, device=dev)
    kc = torch.empty((NQ_KNN,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    vp = C.c_void_p

    def brute(entry, flags):
        _lib.check(entry(ctx._h, ds._h, qb._h, K, flags, vp(bi.data_ptr()), vp(bd.data_ptr())))

    def knn(entry, flags):
        _lib.check(entry(ctx._h, f._h, ds._h, qk._h, K, flags, vp(ki.data_ptr()), vp(kd.data_ptr()),
                         vp(kc.data_ptr())))

    out = {"n": n, "nnz": int(val.numel()), "maxDepth": maxd, "perm_crc": zlib.crc32(f.perm.tobytes())}

    def record(name, fn, crc_of, unc=True):
        ms, all_ms = event_ms(ctx.stream, fn, reps)
        ctx.sync()
        out[name] = {"ms": ms, "all_ms": all_ms, "crc": crc_of()}
        if unc:                                   # (the L2 brute force on CSR rows has no certificate)
            out[name]["uncertified"] = rp.knn_last_uncertified(ctx)

    for mname, flag in (("cosine", rp.RPT_KNN_METRIC_COSINE), ("inner", rp.RPT_KNN_METRIC_INNER)):
        for exact in (0, 1):
            old = ctx.set_option("knn_metric_exact", exact)
            tag = "_exact" if exact else ""
            record("brute_%s%s" % (mname, tag), lambda: brute(brute_metric, flag), lambda: crc(bi, bd))
            record("knn_%s%s" % (mname, tag), lambda: knn(knn_metric, flag), lambda: crc(ki, kd, kc))
            ctx.set_option("knn_metric_exact", old)
    if not dense:
        record("brute_l2", lambda: brute(L.rpt_brute_knn_dev, 0), lambda: crc(bi, bd), unc=False)
        record("knn_l2_fused", lambda: knn(L.rpt_knn_dev, 0), lambda: crc(ki, kd, kc))
        old = ctx.set_option("knn_general", 1)
        record("knn_l2_general", lambda: knn(L.rpt_knn_dev, 0), lambda: crc(ki, kd, kc))
        ctx.set_option("knn_general", old)
    v = C.c_int64()
    _lib.check(L.rpt_knn_last_candidates(ctx._h, C.byref(v)))
    out["knn_candidates"] = int(v.value)
    return out


def run_step(name, n, reps):
    try:
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, str(n), str(reps)],
                            capture_output=True, text=True, timeout=STEP_LIMIT_S[name])
    except subprocess.TimeoutExpired:
        raise SystemExit("step %s ran out of its %d s: nothing recorded" % (name, STEP_LIMIT_S[name]))
    if pr.returncode != 0:
        raise SystemExit("step %s failed (%d): nothing recorded\n%s%s" % (name, pr.returncode, pr.stdout, pr.stderr))
    return json.loads(pr.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, n, reps = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        print(json.dumps(step(name == "dense", n, reps)))
        return
    args = list(sys.argv[1:])

    def opt(flag, default):
        if flag not in args:
            return default
        v = args[args.index(flag) + 1]
        del args[args.index(flag):args.index(flag) + 2]
        return v

    out_path = opt("--out", os.path.join(ROOT, "profiles", "knn_metric_csr_times.json"))
    n = int(opt("--n", 1_000_000))
    reps = int(args[0]) if args else 5
    csr = run_step("csr", n, reps)
    den = run_step("dense", n, reps)
    same_forest = csr["perm_crc"] == den["perm_crc"]
    for m in ("cosine", "inner"):
        crcs = {csr["brute_" + m]["crc"], csr["brute_%s_exact" % m]["crc"], den["brute_" + m]["crc"]}
        if len(crcs) != 1:
            raise SystemExit("brute force under %s: the CSR, exact and dense-ified answers differ" % m)
        crcs = {csr["knn_" + m]["crc"], csr["knn_%s_exact" % m]["crc"]}
        if same_forest:
            crcs.add(den["knn_" + m]["crc"])
        if len(crcs) != 1:
            raise SystemExit("knn under %s: the CSR, exact and dense-ified answers differ" % m)
    res = {"tool": "tools/knn_metric_csr_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median of reps behind a warm-up; one child process per step",
           "workload": "C3: %d x %d CSR f64, density %.2f (%d nonzeros), %d trees, minLeaf %d, maxDepth %d, k = %d; "
                       "%d queries (brute force), %d queries (knn, %d candidates)"
                       % (n, D, DENSITY, csr["nnz"], T, MINL, csr["maxDepth"], K, NQ_BRUTE, NQ_KNN,
                          csr["knn_candidates"]),
           "same_forest_csr_and_dense": same_forest,
           "bit_equal": "brute force: CSR, CSR exact and dense-ified checksums agree; knn: CSR and CSR exact agree"
                        + (", and the dense-ified forest's" if same_forest else ""),
           "csr": {k: v for k, v in csr.items() if isinstance(v, dict)},
           "dense": {k: v for k, v in den.items() if isinstance(v, dict)}}
    print(json.dumps(res))
    with open(out_path, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
