// graph_refine.hip — NN-descent rounds over a kNN graph (rpt_knn_graph_refine_*).
//
// One round maps the graph G (ids / dist / count, rpt_knn_graph_*'s layout) to R(G): row i becomes
// the first k, by (distance, id), of C(i) = (B(i) u U{F(v) : v in B(i)}) \ {i}, B(i) = F(i) u
// Rev_r(i), every set taken from G.  A round therefore reads the caller's arrays and writes a
// scratch graph, which a copy kernel then moves back: the caller's arrays hold the answer after
// every round, whatever the parity of the number of applied rounds.  All `iters` rounds are
// enqueued; a device-side flag (RefineState::active) is cleared by the first round that changed
// no row and every kernel of the later rounds exits at once on it.
//
// Kernels of a round, in stream order:
//   rev_zero_kernel        in-degrees and fill cursors to 0                          (reverse > 0)
//   rev_degree_kernel      in-degree of every target, vector atomics                 (reverse > 0)
//   rev_scan_kernel        exclusive scan of the in-degrees, one workgroup           (reverse > 0)
//   rev_fill_kernel        (source, stored distance) of every edge into its target's segment; the
//                          position inside a segment comes from an atomic cursor, so the ORDER of a
//                          segment depends on arrival — the join takes the first r of a segment by
//                          (stored distance, source), a total order, so Rev_r(i) does not
//   refine_join_kernel     one WAVE owns point i: its row into a sorted list held one entry per
//                          lane, Rev_r(i) by wave_merge over its segment, the ids of B(i) and of the
//                          rows F(v) into an LDS hash set (i and F(i) entered first, marked old), the
//                          set's new members compacted in place, their rows staged through LDS in
//                          chunks of 32 columns (a candidate per lane, columns ascending: the
//                          reference's fold), merged into the list with wave_merge, row i of the
//                          scratch graph written.  Four points per workgroup while four waves' LDS
//                          shares fit 160 KB, else (and with the option graph_refine_general) one
//                          point per workgroup.
//   refine_copy_kernel     scratch graph -> the caller's arrays
//   refine_end_kernel      the round's bookkeeping: rounds + 1, active = (some row changed)
// No atomics touch the lists; the counters (updates, candidates, changed rows) are sums, which do
// not depend on the order of their terms.
// RefineState, refine_begin / refine_end / refine_copy_kernel and the hash set's set_insert live in
// graph_refine_dev.h: the rounds over CSR rows (graph_csr.hip) run on the same ones.
#include <string.h>

#include <algorithm>

#include "graph_refine_dev.h"

namespace rpt {
namespace {

constexpr int kLdsMax = 160 * 1024;

// dynamic LDS, per wave (wave_bytes): 64 * kLS doubles (a chunk of 64 candidates' rows), kCW
// doubles (the chunk of x_i), H ints (the hash set, later the new candidates), k + r ints (B(i)).
// M: the distance (graph_dev.h); rn: the rows' dot(x, x) (cosine: x_i's once per point, a
// candidate's one 8-byte gather per new candidate)
template <class TD, int M>
__global__ __launch_bounds__(256) void refine_join_kernel(
    RefineState* st, const TD* __restrict__ X, int64_t n, int d, int k, int r, int vec, int H,
    int wave_bytes, const int32_t* __restrict__ ids, const double* __restrict__ dist,
    const int32_t* __restrict__ count, const int64_t* __restrict__ roff,
    const int32_t* __restrict__ rsrc, const double* __restrict__ rdist, int32_t* __restrict__ oids,
    double* __restrict__ odist, int32_t* __restrict__ ocount, const double* __restrict__ rn) {
  if (!st->active) return;
  extern __shared__ double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  double* buf = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * wave_bytes);
  double* xi = buf + 64 * kLS;
  int* tab = reinterpret_cast<int*>(xi + kCW);
  int* bl = tab + H;
  const int mask = H - 1, shift = 32 - (31 - __clz(H));
  const unsigned long long below = (1ULL << lane) - 1;
  unsigned long long n_upd = 0, n_cand = 0, n_chg = 0;

  for (int64_t i = (int64_t)blockIdx.x * W + wave; i < n; i += (int64_t)gridDim.x * W) {
    // row i, one entry per lane; an id outside [0, n) (never in a valid graph) is kept but not followed
    int c = count[i];
    c = c < 0 ? 0 : (c > k ? k : c);
    const int c_old = c;
    double ld = pos_inf();
    int lid = -1;
    if (lane < c) {
      ld = dist[i * k + lane];
      lid = ids[i * k + lane];
    }
    const int oid = lid;
    double ni = 0.0;
    if constexpr (M == kGraphCosine) ni = rn[i];

    // Rev_r(i): the first r of the segment by (stored distance, source)
    int rc = 0, rid = -1;
    if (r > 0) {
      const int64_t o0 = roff[i], deg = roff[i + 1] - o0;
      if (deg <= r) {  // all of them: a set, no order needed
        rc = (int)deg;
        if (lane < rc) rid = rsrc[o0 + lane];
      } else {
        double rd = pos_inf();
        for (int64_t b = 0; b < deg; b += 64) {
          const bool on = b + lane < deg;
          const double cd = on ? rdist[o0 + b + lane] : 0.0;
          const int ci = on ? rsrc[o0 + b + lane] : -1;
          wave_merge(rd, rid, rc, r, cd, ci, on, 0.0, -1, false);
        }
      }
    }

    for (int p = lane; p < H; p += 64) tab[p] = kEmpty;
    wave_sync();
    if (lane == 0) set_insert(tab, mask, shift, (int)i, ~(int)i);
    if (lane < c && (unsigned)lid < (unsigned long long)n) set_insert(tab, mask, shift, lid, ~lid);
    if (lane < c) bl[lane] = (unsigned)lid < (unsigned long long)n ? lid : -1;
    if (lane < rc) bl[c + lane] = rid;
    wave_sync();
    if (lane < rc) set_insert(tab, mask, shift, rid, rid);
    const int nb = c + rc;
    for (int p = lane; p < nb * k; p += 64) {
      const int b = p / k, e = p - b * k;
      const int v = bl[b];
      if (v < 0 || e >= count[v]) continue;
      const int cnd = ids[(int64_t)v * k + e];
      if ((unsigned)cnd < (unsigned long long)n) set_insert(tab, mask, shift, cnd, cnd);
    }
    wave_sync();

    // the new members, compacted to tab[0 .. m): a slot is read before anything is written at
    // or behind it (m <= base)
    int m = 0;
    for (int base = 0; base < H; base += 64) {
      const int v = tab[base + lane];
      const unsigned long long bal = __ballot(v >= 0);
      wave_sync();
      if (v >= 0) tab[m + __popcll(bal & below)] = v;
      m += __popcll(bal);
    }
    wave_sync();
    n_cand += (unsigned long long)m;

    bool changed = false;
    for (int b0 = 0; b0 < m; b0 += 64) {
      const int nrows = m - b0 < 64 ? m - b0 : 64;
      const int my = lane < nrows ? tab[b0 + lane] : -1;
      double acc = 0.0;
      for (int c0 = 0; c0 < d; c0 += kCW) {
        const int cw = d - c0 < kCW ? d - c0 : kCW;
        wave_sync();  // the last chunk has been read
        wave_stage<TD>(X, d, tab + b0, nrows, c0, cw, buf, vec != 0);
        if (lane < cw) xi[lane] = widen(X[(size_t)i * d + c0 + lane]);
        wave_sync();
        if (lane < nrows) {
          const double* row = buf + lane * kLS;
#pragma unroll 4
          for (int cc = 0; cc < cw; ++cc) acc = fold_step<M>(acc, xi[cc], row[cc]);
        }
      }
      double nj = 0.0;
      if constexpr (M == kGraphCosine) nj = lane < nrows ? rn[my] : 0.0;
      changed |= wave_merge(ld, lid, c, k, fold_finish<M>(acc, ni, nj), my, lane < nrows, 0.0, -1, false);
    }

    if (lane < k) {
      odist[i * k + lane] = lane < c ? ld : pos_inf();
      oids[i * k + lane] = lane < c ? lid : -1;
    }
    if (lane == 0) ocount[i] = c;
    if (changed) {  // |F_new(i) \ F_old(i)|
      bool was = false;
      for (int s = 0; s < c_old; ++s) was |= lid == __shfl(oid, s);
      const int fresh = __popcll(__ballot(lane < c && !was));
      n_upd += (unsigned long long)fresh;
      n_chg += fresh > 0 ? 1 : 0;
    }
  }
  if (lane == 0 && (n_cand | n_upd | n_chg)) {
    atomicAdd(&st->candidates, n_cand);
    atomicAdd(&st->updates, n_upd);
    if (n_chg) atomicAdd(&st->changed, n_chg);
  }
}

template <class TD, int M>
int32_t launch_join(rpt_ctx* ctx, RefineState* st, const rpt_dataset* data, int k, int r, int H,
                    int wave_bytes, int W, const int32_t* ids, const double* dist,
                    const int32_t* count, const int64_t* roff, const int32_t* rsrc,
                    const double* rdist, int32_t* oids, double* odist, int32_t* ocount) {
  const TD* X = static_cast<const TD*>(data->X);
  const int d = data->d;
  const int vec = ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && ((size_t)d * sizeof(TD)) % 16 == 0) ? 1 : 0;
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)refine_join_kernel<TD, M>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  const int64_t want = (data->n + W - 1) / W;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->n_cu * 16));
  hipLaunchKernelGGL((refine_join_kernel<TD, M>), dim3(grid), dim3(64 * W), (size_t)wave_bytes * W,
                     ctx->stream, st, X, data->n, d, k, r, vec, H, wave_bytes, ids, dist, count, roff,
                     rsrc, rdist, oids, odist, ocount, M == kGraphCosine ? data->sqnorm : nullptr);
  return RPT_OK;
}

template <class TD, class... A>
int32_t launch_join_metric(int m, A... a) {
  if (m == kGraphCosine) return launch_join<TD, kGraphCosine>(a...);
  if (m == kGraphInner) return launch_join<TD, kGraphInner>(a...);
  return launch_join<TD, kGraphL2>(a...);
}

}  // namespace

int32_t knn_graph_refine_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse,
                             int32_t iters, int32_t metric, int32_t* ids_dev, double* dist_dev,
                             int32_t* count_dev) {
  const int m = graph_metric_of(metric);
  if (m == kGraphCosine) RPT_TRY(ensure_sqnorm(ctx, data));  // the rows' dot(x, x), cached on the dataset
  if (!ctx->refine_state_dev) {
    hipError_t e = dev_alloc(&ctx->refine_state_dev, sizeof(RefineState));
    if (e != hipSuccess)
      return fail(RPT_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  }
  RefineState* st = static_cast<RefineState*>(ctx->refine_state_dev);
  const int64_t n = data->n;
  const int r = reverse;
  // the hash set holds at most 1 + (k + r)(k + 1) ids; half as many slots again keep the probes short
  const int64_t raw = 1 + (int64_t)(k + r) * (k + 1);
  int H = 64;
  while (H < raw + raw / 2) H <<= 1;
  const int wave_bytes = (int)(((size_t)(64 * kLS + kCW) * 8 + (size_t)(H + k + r) * 4 + 7) & ~(size_t)7);
  const int W = (ctx->opt.graph_refine_general == 0 && 4 * wave_bytes <= kLdsMax) ? 4 : 1;
  if (wave_bytes > kLdsMax) return fail(RPT_E_INTERNAL, "refine: the candidate set does not fit LDS");

  DevBuf<int32_t> sids, scount, deg, cur, rsrc;
  DevBuf<double> sdist, rdist;
  DevBuf<int64_t> roff;
  RPT_TRY(sids.alloc((size_t)n * k));
  RPT_TRY(sdist.alloc((size_t)n * k));
  RPT_TRY(scount.alloc((size_t)n));
  if (r > 0) {
    RPT_TRY(deg.alloc((size_t)n));
    RPT_TRY(cur.alloc((size_t)n));
    RPT_TRY(roff.alloc((size_t)n + 1));
    RPT_TRY(rsrc.alloc((size_t)n * k));
    RPT_TRY(rdist.alloc((size_t)n * k));
  }
  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  const int64_t cap = (int64_t)ctx->n_cu * 16;
  const unsigned grid_n = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap));
  const unsigned grid_e = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n * k + 255) / 256, cap));
  hipLaunchKernelGGL(refine_begin_kernel, dim3(1), dim3(64), 0, ctx->stream, st);
  for (int32_t it = 0; it < iters; ++it) {
    if (n > 0) {
      if (r > 0) {
        hipLaunchKernelGGL(rev_zero_kernel, dim3(grid_n), dim3(256), 0, ctx->stream, &st->active, n, deg.p, cur.p);
        hipLaunchKernelGGL(rev_degree_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, &st->active, n, k, ids_dev,
                           count_dev, deg.p);
        hipLaunchKernelGGL(rev_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, &st->active, n, deg.p,
                           roff.p);
        hipLaunchKernelGGL(rev_fill_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, &st->active, n, k, ids_dev,
                           dist_dev, count_dev, roff.p, cur.p, rsrc.p, rdist.p);
      }
      switch (data->dtype) {
        case RPT_F64:
          RPT_TRY(launch_join_metric<double>(m, ctx, st, data, k, r, H, wave_bytes, W, ids_dev, dist_dev,
                                              count_dev, roff.p, rsrc.p, rdist.p, sids.p, sdist.p, scount.p));
          break;
        case RPT_F32:
          RPT_TRY(launch_join_metric<float>(m, ctx, st, data, k, r, H, wave_bytes, W, ids_dev, dist_dev,
                                             count_dev, roff.p, rsrc.p, rdist.p, sids.p, sdist.p, scount.p));
          break;
        default:
          RPT_TRY(launch_join_metric<uint16_t>(m, ctx, st, data, k, r, H, wave_bytes, W, ids_dev, dist_dev,
                                                count_dev, roff.p, rsrc.p, rdist.p, sids.p, sdist.p, scount.p));
      }
      hipLaunchKernelGGL(refine_copy_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, st, n, k, sids.p,
                         sdist.p, scount.p, ids_dev, dist_dev, count_dev);
    }
    hipLaunchKernelGGL(refine_end_kernel, dim3(1), dim3(64), 0, ctx->stream, st);
    RPT_HIP(hipGetLastError());
  }
  return RPT_OK;
}

int32_t knn_graph_refine_last(rpt_ctx* ctx, int64_t* rounds, int64_t* updates, int64_t* candidates) {
  *rounds = *updates = *candidates = 0;
  if (!ctx->refine_state_dev) return RPT_OK;  // no call yet
  RPT_HIP(stream_sync(ctx->stream));
  RefineState h;
  RPT_HIP(hipMemcpy(&h, ctx->refine_state_dev, sizeof h, hipMemcpyDeviceToHost));
  *rounds = (int64_t)h.rounds;
  *updates = (int64_t)h.updates;
  *candidates = (int64_t)h.candidates;
  return RPT_OK;
}

}  // namespace rpt
