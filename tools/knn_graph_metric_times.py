"""kNN graph and one NN-descent round under the cosine / inner-product distances
(rpt_knn_graph_metric_dev, rpt_knn_graph_refine_metric_dev) against the L2 entry points of this
build and of the parent commit, at C2.

    python tools/knn_graph_metric_times.py [reps] --parent-lib PATH [--n N] [--out FILE]

C2 = the flagship shape (seeds of BASELINE configs[1]: 1 M x 128 f64, 32 trees, minLeaf 128, k = 10).
Everything is timed with HIP events on the ctx stream, median of REPS behind a warm-up.  The parent
commit's library (PATH) runs in a fresh CHILD process through RPTREE_HIP_LIB, on the forest of the same
seeds (the perm's checksum must agree), in the same run.  profiles/knn_graph_metric_times.json gets:
  (a) rpt_knn_graph_metric_dev, cosine and inner product
  (b) this build's rpt_knn_graph_dev
  (c) the parent's rpt_knn_graph_dev
  (d) the parent's rpt_knn_dev over all points with RPT_KNN_METRIC_COSINE | RPT_KNN_DEDUP, k + 1: the
      route to a cosine graph before these entry points
  (e) one refinement round over the 32-tree graph, k = reverse = 10: L2 (this build and the parent's)
      and cosine
and the four expectations as booleans, each against the numbers of this one run:
  (b) within 10 % of (c); (a) no slower than (c) + 10 %; (a) faster than (d) (the ratio is reported);
  the cosine round of (e) within 10 % of the L2 round.
--n N shrinks the data set (a rehearsal; nothing is written unless --out is given).
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rptree_amd import gen  # noqa: E402  (no library call: the child's library lacks the new symbols)

D, T, MINL, K, REVERSE, SEED = 128, 32, 128, 10, 10, 1234
RPT_PROJ_MFMA, RPT_KNN_DEDUP, COSINE, INNER = 2, 1, 1 << 25, 1 << 26


def cfg_of(n):
    maxd = math.ceil(math.log(n / MINL) / math.log(2.0))            # rpTreeCfg, Conduit.hs:132-141
    pnz = min(1.0 / (math.log(D) / math.log(10.0)), 1.0)
    return maxd, pnz


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


class Raw:
    """raw ctypes on one library: the calls both builds have, and (this build only) the metric ones"""

    def __init__(self, path, n):
        self.L = C.CDLL(path)
        self.n = n
        vp = C.c_void_p
        self.dev = torch.device("cuda", 0)
        self.X = gen.normal_dense2_torch(SEED, n, D, self.dev)
        torch.cuda.synchronize(self.dev)
        maxd, pnz = cfg_of(n)
        _, R = gen.forest_hyperplanes(1235137, T, maxd, pnz, D)
        R = np.ascontiguousarray(R, dtype=np.float64)
        self.ctx, self.ds, self.f, stream = vp(), vp(), vp(), vp()
        self.call("rpt_ctx_create", C.c_int32(0), C.byref(self.ctx))
        self.call("rpt_ctx_stream", self.ctx, C.byref(stream))
        self.stream = stream.value
        self.call("rpt_dataset_dense_dev", self.ctx, vp(self.X.data_ptr()), C.c_int64(n), C.c_int32(D), C.c_int32(0),
                  C.byref(self.ds))
        self.call("rpt_forest_build", self.ctx, self.ds, vp(R.ctypes.data), C.c_int32(T), C.c_int32(maxd),
                  C.c_int32(MINL), C.c_int32(RPT_PROJ_MFMA), C.byref(self.f))
        perm = np.empty((T, n), dtype=np.int32)
        self.call("rpt_forest_get_perm", self.f, vp(perm.ctypes.data))
        self.perm_crc = zlib.crc32(perm.tobytes())

    def call(self, fn, *a):
        f = getattr(self.L, fn)
        f.restype = C.c_int32
        if f(*a) != 0:
            self.L.rpt_last_error.restype = C.c_char_p
            raise SystemExit("%s: %s" % (fn, self.L.rpt_last_error().decode()))

    def arrays(self, k):
        return (torch.empty((self.n, k), dtype=torch.int32, device=self.dev),
                torch.empty((self.n, k), dtype=torch.float64, device=self.dev),
                torch.empty((self.n,), dtype=torch.int32, device=self.dev))

    def graph(self, metric, reps):
        """metric None: rpt_knn_graph_dev; else rpt_knn_graph_metric_dev -> (ms, all, the arrays)"""
        ids, dist, cnt = self.arrays(K)
        vp = C.c_void_p
        ptrs = (vp(ids.data_ptr()), vp(dist.data_ptr()), vp(cnt.data_ptr()))
        if metric is None:
            once = lambda: self.call("rpt_knn_graph_dev", self.ctx, self.f, self.ds, C.c_int32(K), C.c_int32(0), *ptrs)  # noqa: E731
        else:
            once = lambda: self.call("rpt_knn_graph_metric_dev", self.ctx, self.f, self.ds, C.c_int32(K),  # noqa: E731
                                     C.c_int32(metric), C.c_int32(0), *ptrs)
        ms, all_ms = event_ms(self.stream, once, reps)
        self.call("rpt_ctx_sync", self.ctx)
        return ms, all_ms, (ids, dist, cnt)

    def round(self, metric, g, reps):
        """one refinement round over a copy of the graph g, restored (untimed) before every repetition"""
        ids, dist, cnt = (a.clone() for a in g)
        vp = C.c_void_p
        ptrs = (vp(ids.data_ptr()), vp(dist.data_ptr()), vp(cnt.data_ptr()))

        def restore():
            ids.copy_(g[0])
            dist.copy_(g[1])
            cnt.copy_(g[2])

        if metric is None:
            once = lambda: self.call("rpt_knn_graph_refine_dev", self.ctx, self.ds, C.c_int32(K), C.c_int32(REVERSE),  # noqa: E731
                                     C.c_int32(1), C.c_int32(0), *ptrs)
        else:
            once = lambda: self.call("rpt_knn_graph_refine_metric_dev", self.ctx, self.ds, C.c_int32(K),  # noqa: E731
                                     C.c_int32(REVERSE), C.c_int32(1), C.c_int32(metric), C.c_int32(0), *ptrs)
        ms, all_ms = event_ms(self.stream, once, reps, before=restore)
        r, u, c = C.c_int64(), C.c_int64(), C.c_int64()
        self.call("rpt_knn_graph_refine_last", self.ctx, C.byref(r), C.byref(u), C.byref(c))
        return ms, all_ms, int(c.value)

    def self_query(self, flags, reps):
        ids, dist, cnt = self.arrays(K + 1)
        vp = C.c_void_p
        once = lambda: self.call("rpt_knn_dev", self.ctx, self.f, self.ds, self.ds, C.c_int32(K + 1), C.c_int32(flags),  # noqa: E731
                                 vp(ids.data_ptr()), vp(dist.data_ptr()), vp(cnt.data_ptr()))
        ms, all_ms = event_ms(self.stream, once, reps)
        self.call("rpt_ctx_sync", self.ctx)
        return ms, all_ms


def child(n, reps):
    """the parent commit's library: (c), (d) and the L2 round of (e)"""
    lib = Raw(os.environ["RPTREE_HIP_LIB"], n)
    out = {"perm_crc": lib.perm_crc}
    out["graph_l2_ms"], out["graph_l2_all_ms"], g = lib.graph(None, reps)
    out["round_l2_ms"], out["round_l2_all_ms"], out["round_l2_candidates"] = lib.round(None, g, reps)
    out["self_query_cosine_ms"], out["self_query_cosine_all_ms"] = lib.self_query(COSINE | RPT_KNN_DEDUP, reps)
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n, out_path, parent = 1_000_000, os.path.join(ROOT, "profiles", "knn_graph_metric_times.json"), None
    if "--n" in sys.argv:
        v = sys.argv[sys.argv.index("--n") + 1]
        n, out_path = int(v), None
        args.remove(v)
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
        args.remove(out_path)
    if "--parent-lib" in sys.argv:
        parent = sys.argv[sys.argv.index("--parent-lib") + 1]
        args.remove(parent)
    if not parent:
        raise SystemExit("--parent-lib PATH (the library built from the parent commit) is required")
    reps = int(args[0]) if args else 5

    # the comparator first, in a process of its own that has gone before this one opens the device
    env = dict(os.environ, RPTREE_HIP_LIB=os.path.abspath(parent))
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(reps)], env=env,
                        capture_output=True, text=True, timeout=900)
    if pr.returncode != 0:
        raise SystemExit("comparator failed:\n" + pr.stdout + pr.stderr)
    par = json.loads(pr.stdout.strip().splitlines()[-1])

    from rptree_amd import _lib
    lib = Raw(_lib.LIB_PATH, n)
    if par["perm_crc"] != lib.perm_crc:
        raise SystemExit("the comparator's forest differs from this build's")
    maxd, _ = cfg_of(n)
    res = {"tool": "tools/knn_graph_metric_times.py", "reps": reps,
           "timing": "HIP events on the ctx stream, median behind a warm-up",
           "workload": "%d x %d f64, %d trees, minLeaf %d, maxDepth %d, k = %d, reverse = %d" % (n, D, T, MINL, maxd, K,
                                                                                               REVERSE),
           "parent_library": "the parent commit's build, loaded through RPTREE_HIP_LIB in a child process"}
    res["b_graph_l2_ms"], res["b_graph_l2_all_ms"], g_l2 = lib.graph(None, reps)
    res["a_graph_cosine_ms"], res["a_graph_cosine_all_ms"], g_cos = lib.graph(COSINE, reps)
    res["a_graph_inner_ms"], res["a_graph_inner_all_ms"], _ = lib.graph(INNER, reps)
    res["c_parent_graph_l2_ms"], res["c_parent_graph_l2_all_ms"] = par["graph_l2_ms"], par["graph_l2_all_ms"]
    res["d_parent_self_query_cosine_ms"] = par["self_query_cosine_ms"]
    res["d_parent_self_query_cosine_all_ms"] = par["self_query_cosine_all_ms"]
    res["e_round_l2_ms"], res["e_round_l2_all_ms"], res["e_round_l2_candidates"] = lib.round(None, g_l2, reps)
    res["e_round_cosine_ms"], res["e_round_cosine_all_ms"], res["e_round_cosine_candidates"] = lib.round(COSINE, g_cos,
                                                                                                      reps)
    res["e_parent_round_l2_ms"], res["e_parent_round_l2_all_ms"] = par["round_l2_ms"], par["round_l2_all_ms"]
    res["e_parent_round_l2_candidates"] = par["round_l2_candidates"]
    c = res["c_parent_graph_l2_ms"]
    worst_a = max(res["a_graph_cosine_ms"], res["a_graph_inner_ms"])
    res["ratio_b_over_c"] = res["b_graph_l2_ms"] / c
    res["ratio_a_cosine_over_c"] = res["a_graph_cosine_ms"] / c
    res["ratio_a_inner_over_c"] = res["a_graph_inner_ms"] / c
    res["speedup_a_cosine_over_d"] = res["d_parent_self_query_cosine_ms"] / res["a_graph_cosine_ms"]
    res["ratio_round_cosine_over_l2"] = res["e_round_cosine_ms"] / res["e_round_l2_ms"]
    res["ratio_round_l2_over_parent"] = res["e_round_l2_ms"] / res["e_parent_round_l2_ms"]
    res["expectations"] = {
        "b_within_10pct_of_c": abs(res["ratio_b_over_c"] - 1.0) <= 0.10,
        "a_no_slower_than_c_plus_10pct": worst_a <= 1.10 * c,
        "a_faster_than_d": worst_a < res["d_parent_self_query_cosine_ms"],
        "cosine_round_within_10pct_of_l2_round": abs(res["ratio_round_cosine_over_l2"] - 1.0) <= 0.10,
    }
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
