// graph_insert.hip — new rows into a kNN graph (rpt_graph_insert_*).
//
// The answer is the definition of include/rptree_hip.h.  The data set holds N = n + m rows, the last m
// of them new; the graph over the first n is copied into the output, and the new rows are taken in
// chunks of `batch`.  With v rows visible, a chunk P = [v, v + |P|)
//   is SEARCHED: the beam search of rpt_graph_search_* (graph_search.hip / graph_search_csr.hip, called
//     through graph_search_dev / graph_search_csr_dev with two non-owning views of `data`: its first
//     v rows as the data set, the rows of P as the queries) over the OUTPUT arrays as the graph, with
//     k = kg, its answers landing in place as rows P of the output;
//   and LINKED: every (d, o) of an answer A_p offers (d, p) to row o, and row o becomes the first kg
//     of its valid entries and its offers by (distance, id).
// The stream orders the link of a chunk before the search of the next.
//
// The link of a chunk works on the chunk's |P| * kg answer slots and the rows they name, never on all
// v rows:
//   link_count_kernel  a slot per thread: deg[o] += 1 (vector atomics); the slot that saw 0 appends o
//                      to the touched list
//   link_scan_kernel   one workgroup: the exclusive scan of the touched rows' degrees -> off[t], and
//                      toff[o] = off[t] for the fill
//   link_fill_kernel   a slot per thread: (d, p) into rsrc / rdist at toff[o] + (deg[o] -= 1), which
//                      leaves every deg[o] at 0 again for the next chunk
//   link_merge_kernel  one WAVE per touched row: the lanes hold row o one entry each (wave_merge of
//                      graph_dev.h), the offers enter in pieces of 64 (a hub with far more than 64
//                      offers is a longer loop), the row is written in place
// The position of an offer inside its segment comes from an atomic cursor, so the ORDER of a segment
// depends on arrival; the row is the first kg of a set under a total order, so the answer does not.  No
// atomics touch a row; the counters are sums.  deg[N] is zeroed once per call, toff[N] is written only
// where it is read.
#include <algorithm>

#include "graph_dev.h"

namespace rpt {
namespace {

struct InsertState {
  unsigned long long chunks, evaluated, offered, accepted;
  int32_t ntouched, pad;
};

__global__ void insert_begin_kernel(InsertState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->chunks = 0;
    st->evaluated = 0;
    st->offered = 0;
    st->accepted = 0;
    st->ntouched = 0;
    st->pad = 0;
  }
}

// behind the search of a chunk: its distances join the call's, the touched list starts empty
__global__ void insert_chunk_kernel(InsertState* st, const SearchState* ss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->chunks += 1;
    st->evaluated += ss->evaluated;
    st->ntouched = 0;
  }
}

// slot e = (row v + e / kg, column e % kg) of the chunk's answers: valid when the column lies inside
// the row's count and names a visible row (the search writes nothing else)
__device__ inline bool slot_of(int64_t e, int64_t total, int64_t v, int kg, const int32_t* oids,
                               const int32_t* ocount, int64_t& row, int& o) {
  if (e >= total) return false;
  const int64_t p = e / kg;
  const int j = (int)(e - p * kg);
  row = v + p;
  if (j >= ocount[row]) return false;
  o = oids[row * kg + j];
  return (unsigned)o < (unsigned long long)v;
}

__global__ __launch_bounds__(256) void link_count_kernel(InsertState* st, int64_t v, int64_t cnt, int kg,
                                                         const int32_t* __restrict__ oids,
                                                         const int32_t* __restrict__ ocount, int32_t* deg,
                                                         int32_t* __restrict__ touched) {
  const int64_t total = cnt * kg, stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long n_off = 0;
  for (int64_t e0 = (int64_t)blockIdx.x * blockDim.x; e0 < total; e0 += stride) {
    int64_t row;
    int o = -1;
    const bool on = slot_of(e0 + threadIdx.x, total, v, kg, oids, ocount, row, o);
    if (on && atomicAdd(&deg[o], 1) == 0) touched[atomicAdd(&st->ntouched, 1)] = o;
    n_off += (unsigned long long)__popcll(__ballot(on));
  }
  if ((threadIdx.x & 63) == 0 && n_off) atomicAdd(&st->offered, n_off);
}

// off[0 .. nt] = exclusive scan of deg[touched[0 .. nt)); toff[touched[t]] = off[t]
__global__ __launch_bounds__(kScanThreads) void link_scan_kernel(const InsertState* st,
                                                                 const int32_t* __restrict__ touched,
                                                                 const int32_t* __restrict__ deg,
                                                                 int64_t* __restrict__ off,
                                                                 int64_t* __restrict__ toff) {
  __shared__ int64_t part[kScanThreads];
  const int tid = threadIdx.x;
  const int64_t nt = st->ntouched;
  const int64_t per = (nt + kScanThreads - 1) / kScanThreads;
  const int64_t lo = std::min<int64_t>(nt, per * tid), hi = std::min<int64_t>(nt, lo + per);
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += deg[touched[i]];
  part[tid] = s;
  __syncthreads();
  for (int step = 1; step < kScanThreads; step <<= 1) {  // inclusive scan of the partial sums
    const int64_t add = tid >= step ? part[tid - step] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int64_t run = part[tid] - s;
  for (int64_t i = lo; i < hi; ++i) {
    const int o = touched[i];
    off[i] = run;
    toff[o] = run;
    run += deg[o];
  }
  if (tid == kScanThreads - 1) off[nt] = part[tid];
}

__global__ __launch_bounds__(256) void link_fill_kernel(int64_t v, int64_t cnt, int kg,
                                                        const int32_t* __restrict__ oids,
                                                        const double* __restrict__ odist,
                                                        const int32_t* __restrict__ ocount,
                                                        const int64_t* __restrict__ toff, int32_t* deg,
                                                        int32_t* __restrict__ rsrc,
                                                        double* __restrict__ rdist) {
  const int64_t total = cnt * kg, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    int64_t row;
    int o;
    if (!slot_of(e, total, v, kg, oids, ocount, row, o)) continue;
    const int64_t p = toff[o] + (atomicSub(&deg[o], 1) - 1);  // the last taker leaves deg[o] at 0
    rsrc[p] = (int32_t)row;
    rdist[p] = odist[e + v * kg];
  }
}

// Row o = touched[t] of the output, in place: its valid entries (inside the clamped count, id in
// [0, N), an id once, at its first slot), then its offers.  [v, v + cnt) are the chunk's rows.
__global__ __launch_bounds__(256) void link_merge_kernel(InsertState* st, int64_t N, int64_t v, int64_t cnt,
                                                         int kg, const int32_t* __restrict__ touched,
                                                         const int64_t* __restrict__ off,
                                                         const int32_t* __restrict__ rsrc,
                                                         const double* __restrict__ rdist, int32_t* oids,
                                                         double* odist, int32_t* ocount) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int64_t nt = st->ntouched;
  unsigned long long n_acc = 0;
  for (int64_t t = (int64_t)blockIdx.x * W + wave; t < nt; t += (int64_t)gridDim.x * W) {
    const int64_t o = touched[t];
    int c = ocount[o];
    c = c < 0 ? 0 : (c > kg ? kg : c);
    int kid = -1;
    double kd = pos_inf();
    if (lane < c) {
      kid = oids[o * kg + lane];
      kd = odist[o * kg + lane];
    }
    const bool ok = lane < c && (unsigned)kid < (unsigned long long)N;
    double ld = pos_inf();
    int lid = -1, lc = 0;
    wave_merge(ld, lid, lc, kg, kd, kid, ok, 0.0, -1, false);

    // an offer whose id the row holds already is dropped whether or not that entry is still in the
    // list (else the answer would depend on the order of arrival); a graph over rows that were visible
    // before this chunk holds no such id, and the loop is skipped
    const bool clash = __ballot(ok && kid >= v) != 0;
    const int64_t o0 = off[t], dg = off[t + 1] - o0;
    for (int64_t b = 0; b < dg; b += 64) {
      bool on = b + lane < dg;
      const double cd = on ? rdist[o0 + b + lane] : 0.0;
      const int ci = on ? rsrc[o0 + b + lane] : -2;
      if (clash)
        for (int e = 0; e < c; ++e) {
          const int kv = __shfl(kid, e);  // by every lane: a lane that is off may hold the entry asked for
          const bool kok = __shfl((int)ok, e) != 0;
          on = on && !(kok && ci == kv);
        }
      wave_merge(ld, lid, lc, kg, cd, ci, on, 0.0, -1, false);
    }

    if (lane < kg) {
      odist[o * kg + lane] = lane < lc ? ld : pos_inf();
      oids[o * kg + lane] = lane < lc ? lid : -1;
    }
    if (lane == 0) ocount[o] = lc;
    bool mine = lane < lc && lid >= v && lid < v + cnt;  // an offer that is in the row
    if (clash)
      for (int e = 0; e < c; ++e) {
        const int kv = __shfl(kid, e);
        const bool kok = __shfl((int)ok, e) != 0;
        mine = mine && !(kok && lid == kv);
      }
    n_acc += (unsigned long long)__popcll(__ballot(mine));
  }
  if (lane == 0 && n_acc) atomicAdd(&st->accepted, n_acc);
}

}  // namespace

int32_t graph_insert_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_dev,
                         const double* gdist_dev, const int32_t* gcount_dev, int64_t m, int32_t s,
                         const int32_t* seeds_dev, int32_t ef, int64_t batch, int32_t metric,
                         int32_t* oids_dev, double* odist_dev, int32_t* ocount_dev) {
  const int64_t N = data->n, n = N - m;
  const int mt = graph_metric_of(metric);
  if (mt == kGraphCosine && m > 0) RPT_TRY(ensure_sqnorm(ctx, data));  // the views below borrow it
  if (!ctx->insert_state_dev) {
    hipError_t e = dev_alloc(&ctx->insert_state_dev, sizeof(InsertState));
    if (e != hipSuccess)
      return fail(RPT_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  }
  InsertState* st = static_cast<InsertState*>(ctx->insert_state_dev);

  // the plan: scratch by (N, batch, kg)
  const int64_t B = std::min<int64_t>(batch, m);  // rows of the largest chunk
  const size_t slots = (size_t)B * kg;            // its answer slots: offers, and touched rows at most
  DevBuf<int32_t> deg, touched, rsrc;
  DevBuf<int64_t> toff, off;
  DevBuf<double> rdist;
  if (m > 0 && n + m - B > 0) {  // some chunk has a visible row to link to
    RPT_TRY(deg.alloc((size_t)N));
    RPT_TRY(toff.alloc((size_t)N));
    RPT_TRY(touched.alloc(slots));
    RPT_TRY(off.alloc(slots + 1));
    RPT_TRY(rsrc.alloc(slots));
    RPT_TRY(rdist.alloc(slots));
    RPT_HIP(hipMemsetAsync(deg.p, 0, (size_t)N * 4, ctx->stream));
  }

  hipLaunchKernelGGL(insert_begin_kernel, dim3(1), dim3(64), 0, ctx->stream, st);
  RPT_HIP(hipGetLastError());
  if (n > 0) {  // G_0: the caller's rows, verbatim
    RPT_HIP(hipMemcpyAsync(oids_dev, gids_dev, (size_t)n * kg * 4, hipMemcpyDeviceToDevice, ctx->stream));
    RPT_HIP(hipMemcpyAsync(odist_dev, gdist_dev, (size_t)n * kg * 8, hipMemcpyDeviceToDevice, ctx->stream));
    RPT_HIP(hipMemcpyAsync(ocount_dev, gcount_dev, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }

  const int64_t cap = (int64_t)ctx->n_cu * 16;
  for (int64_t v = n; v < N;) {
    const int64_t cnt = std::min<int64_t>(batch, N - v);
    // ---- the search of the chunk: the first v rows as the data set, rows [v, v + cnt) as the queries
    rpt_dataset dv = *data, qv = *data;
    dv.owns = qv.owns = false;
    dv.n = v;
    qv.n = cnt;
    if (data->csr) qv.rowptr = data->rowptr + v;
    else qv.X = static_cast<char*>(data->X) + (size_t)v * data->d * dtype_size(data->dtype);
    if (mt == kGraphCosine) qv.sqnorm = data->sqnorm + v;
    const int32_t* sd = seeds_dev + (size_t)(v - n) * s;
    if (data->csr)
      RPT_TRY(graph_search_csr_dev(ctx, &dv, &qv, kg, oids_dev, ocount_dev, s, sd, kg, ef, metric,
                                   oids_dev + (size_t)v * kg, odist_dev + (size_t)v * kg, ocount_dev + v));
    else
      RPT_TRY(graph_search_dev(ctx, &dv, &qv, kg, oids_dev, ocount_dev, s, sd, kg, ef, metric,
                               oids_dev + (size_t)v * kg, odist_dev + (size_t)v * kg, ocount_dev + v));
    hipLaunchKernelGGL(insert_chunk_kernel, dim3(1), dim3(64), 0, ctx->stream, st,
                       static_cast<const SearchState*>(ctx->search_state_dev));

    // ---- the link of the chunk
    if (v > 0) {
      ProfScope ps(ctx, RPT_PROF_GRAPH_LINK);
      const int64_t total = cnt * kg;
      const unsigned grid_e = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, cap));
      const int64_t rows = std::min<int64_t>(total, v);  // touched rows at most
      const unsigned grid_m = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, cap));
      hipLaunchKernelGGL(link_count_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, st, v, cnt, kg, oids_dev,
                         ocount_dev, deg.p, touched.p);
      hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, st, touched.p, deg.p,
                         off.p, toff.p);
      hipLaunchKernelGGL(link_fill_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, v, cnt, kg, oids_dev,
                         odist_dev, ocount_dev, toff.p, deg.p, rsrc.p, rdist.p);
      hipLaunchKernelGGL(link_merge_kernel, dim3(grid_m), dim3(256), 0, ctx->stream, st, N, v, cnt, kg,
                         touched.p, off.p, rsrc.p, rdist.p, oids_dev, odist_dev, ocount_dev);
    }
    RPT_HIP(hipGetLastError());
    v += cnt;
  }
  return RPT_OK;
}

int32_t graph_insert_last(rpt_ctx* ctx, int64_t* chunks, int64_t* evaluated, int64_t* offered,
                          int64_t* accepted) {
  *chunks = *evaluated = *offered = *accepted = 0;
  if (!ctx->insert_state_dev) return RPT_OK;  // no call yet
  RPT_HIP(stream_sync(ctx->stream));
  InsertState h;
  RPT_HIP(hipMemcpy(&h, ctx->insert_state_dev, sizeof h, hipMemcpyDeviceToHost));
  *chunks = (int64_t)h.chunks;
  *evaluated = (int64_t)h.evaluated;
  *offered = (int64_t)h.offered;
  *accepted = (int64_t)h.accepted;
  return RPT_OK;
}

}  // namespace rpt
