// graph_search.hip — best-first beam search over a kNN graph (rpt_graph_search_*).
//
// The answer is the definition of include/rptree_hip.h: a beam B of at most ef entries sorted by
// (distance, id), the valid seeds offered first, then, while B holds an unexpanded entry, the first
// such entry u marked expanded and the valid ids of graph row u offered.  Offering a set S makes B
// the first ef of B u S, every id once.  The beam's last entry only moves forward, so whatever was
// rejected or evicted once never enters later: a point is expanded at most once, and skipping an id
// that was evaluated before (the visited filter) changes no answer.
//
// graph_search_kernel: one WAVE owns a query, four queries per workgroup.  Per wave in LDS:
//   buf   R x kLS doubles    a chunk of kCW columns of up to R candidate rows (R = rows of one offer)
//   qv    d doubles          the query, widened once (d <= kQMax; beyond, kCW doubles per chunk)
//   bd/bi, tab, sid          the beam, the visited filter and the running offer's ids (graph_dev.h)
// An offer (graph_dev.h: beam_next_offer, beam_admit, beam_insert, shared with the CSR kernel of
// graph_search_csr.hip): a candidate per lane, dropped when the filter or the beam (exactly) holds
// it, the rest compacted, their rows staged chunk by chunk (wave_stage) and folded a candidate per
// lane, columns ascending (fold_step / fold_finish: the reference's fold), then inserted one by
// one: rank by ballot / popcount over the lanes' entries (lane l looks at positions l, l + 64, ...),
// the tail shifted by one in LDS.  No atomics touch the beam; the filter's atomics only decide what is
// evaluated twice.  The loops are bounded by the definition: ceil(s / R) seed offers, at most n
// expansions.
//
// graph_search_allow_kernel (rpt_graph_search_allow_*): the same search among the ids of an allow-list.
// The body of both kernels is graph_search_body; with its switch F on, the beam is the cut of
// graph_dev.h (up to `width` entries, ending at its ef-th allowed entry), the answer the first k allowed
// entries, and the workgroup 4, 2 or 1 waves, whichever keeps the most waves on a CU (search_waves), so
// that every valid shape launches.
#include <algorithm>

#include "graph_dev.h"

namespace rpt {
namespace {

constexpr int kLdsMax = 160 * 1024;
constexpr int kQMax = 1024;  // columns up to which the query stays in LDS whole

// The search of one workgroup; F and J are the beam's switches of graph_dev.h.  F off: the beam of
// rpt_graph_search_*.  F on: the beam of rpt_graph_search_allow_*, up to a.width entries with their
// allowed bytes `ba` behind the offer's ids.
template <class TD, int M, bool F, int J>
__device__ __forceinline__ void graph_search_body(const TD* __restrict__ X, const TD* __restrict__ Q,
                                                  const SearchArgs& a, double* smem) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int nj = ((F ? a.width : a.ef) + 63) >> 6, efp = nj * 64;
  const int d = a.d, ef = a.ef, R = a.R;
  double* buf = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * a.wave_bytes);
  double* qv = buf + R * kLS;
  double* bd = qv + (a.qres ? d : kCW);
  int* bi = reinterpret_cast<int*>(bd + efp);
  int* tab = bi + efp;
  int* sid = tab + a.H;
  unsigned char* ba = reinterpret_cast<unsigned char*>(sid + R);  // F only
  const bool filter = a.nofilter == 0;
  unsigned long long n_exp = 0, n_eval = 0;

  for (int64_t qi = (int64_t)blockIdx.x * W + wave; qi < a.nq; qi += (int64_t)gridDim.x * W) {
    const TD* qrow = Q + (size_t)qi * d;
    wave_sync();  // the last query's beam has been written out
    if (a.qres)
      for (int c = lane; c < d; c += 64) qv[c] = widen(qrow[c]);
    if (filter)
      for (int p = lane; p < a.H; p += 64) tab[p] = kEmpty;
    wave_sync();
    double qnorm = 0.0;
    if constexpr (M == kGraphCosine) qnorm = a.qn[qi];
    BeamAllow aw = {nullptr, false};  // F: the query's own bitmap
    if constexpr (F) aw = beam_allow_of(a, qi);

    int c = 0;   // entries of the beam
    int na = 0;  // F: the allowed ones among them
    int s0 = 0;
    int64_t expanded = 0;
    for (;;) {
      // ---- the next offer, without what is out of range, remembered by the filter or in the beam
      int cand;
      if (s0 >= a.s && expanded >= a.n) break;  // every point at most once
      if (!beam_next_offer(a, qi, bi, c, nj, lane, s0, expanded, cand)) break;
      const int nrows = beam_admit(a, bi, c, tab, sid, filter, lane, cand);
      if (nrows == 0) continue;
      n_eval += (unsigned long long)nrows;

      // ---- the distances: a candidate per lane, columns ascending
      const int my = lane < nrows ? sid[lane] : -1;
      double acc = 0.0;
      for (int c0 = 0; c0 < d; c0 += kCW) {
        const int cw = d - c0 < kCW ? d - c0 : kCW;
        wave_sync();  // the last chunk has been read
        wave_stage<TD>(X, d, sid, nrows, c0, cw, buf, a.vec != 0);
        if (!a.qres && lane < cw) qv[lane] = widen(qrow[c0 + lane]);
        wave_sync();
        if (lane < nrows) {
          const double* row = buf + lane * kLS;
          const double* qq = a.qres ? qv + c0 : qv;
#pragma unroll 4
          for (int cc = 0; cc < cw; ++cc) acc = fold_step<M>(acc, qq[cc], row[cc]);
        }
      }
      double nrm = 0.0;
      if constexpr (M == kGraphCosine) nrm = lane < nrows ? a.rn[my] : 0.0;
      const double cd = fold_finish<M>(acc, qnorm, nrm);

      // ---- into the beam, one at a time, by the order of before()
      if constexpr (F)
        beam_insert<true, J>(bd, bi, c, ef, nj, lane, nrows, cd, my, ba, a.width, &na, beam_allowed(aw, my));
      else
        beam_insert(bd, bi, c, ef, nj, lane, nrows, cd, my);
    }
    n_exp += (unsigned long long)expanded;
    if constexpr (F)
      beam_answer<true>(a, qi, bd, bi, c, lane, ba, na);
    else
      beam_answer(a, qi, bd, bi, c, lane);
  }
  if (lane == 0 && (n_exp | n_eval)) {
    atomicAdd(&a.st->expansions, n_exp);
    atomicAdd(&a.st->evaluated, n_eval);
  }
}

template <class TD, int M>
__global__ __launch_bounds__(256) void graph_search_kernel(const TD* __restrict__ X,
                                                           const TD* __restrict__ Q, SearchArgs a) {
  extern __shared__ double smem[];
  graph_search_body<TD, M, false, kBeamJ>(X, Q, a, smem);
}

// rpt_graph_search_allow_*: J = kBeamJ for a width up to 256, kBeamJWide beyond
template <class TD, int M, int J>
__global__ __launch_bounds__(256) void graph_search_allow_kernel(const TD* __restrict__ X,
                                                                 const TD* __restrict__ Q, SearchArgs a) {
  extern __shared__ double smem[];
  graph_search_body<TD, M, true, J>(X, Q, a, smem);
}

// J == 0: graph_search_kernel, four waves per workgroup; else graph_search_allow_kernel<J>, as many
// of 4, 2 or 1 as search_waves picks
template <class TD, int M, int J>
int32_t launch_search(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, SearchArgs a) {
  const TD* X = static_cast<const TD*>(data->X);
  const TD* Q = static_cast<const TD*>(queries->X);
  a.vec = ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && ((size_t)a.d * sizeof(TD)) % 16 == 0) ? 1 : 0;
  void (*kern)(const TD*, const TD*, SearchArgs);
  if constexpr (J == 0) kern = graph_search_kernel<TD, M>;
  else kern = graph_search_allow_kernel<TD, M, J>;
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  const int W = J == 0 ? 4 : search_waves(a.wave_bytes, kLdsMax);
  const int64_t want = (a.nq + W - 1) / W;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->n_cu * 64));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * W), (size_t)a.wave_bytes * W, ctx->stream, X, Q, a);
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

template <class TD, int J>
int32_t launch_search_metric(int m, rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                             const SearchArgs& a) {
  if (m == kGraphCosine) return launch_search<TD, kGraphCosine, J>(ctx, data, queries, a);
  if (m == kGraphInner) return launch_search<TD, kGraphInner, J>(ctx, data, queries, a);
  return launch_search<TD, kGraphL2, J>(ctx, data, queries, a);
}

template <class TD>
int32_t launch_search_beam(int m, rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                           const SearchArgs& a, bool allow) {
  if (!allow) return launch_search_metric<TD, 0>(m, ctx, data, queries, a);
  if (a.width <= 64 * kBeamJ) return launch_search_metric<TD, kBeamJ>(m, ctx, data, queries, a);
  return launch_search_metric<TD, kBeamJWide>(m, ctx, data, queries, a);
}

}  // namespace

int32_t graph_search_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, int32_t kg,
                         const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                         const int32_t* seeds_dev, int32_t k, int32_t ef, int32_t metric,
                         int32_t* ids_dev, double* dist_dev, int32_t* count_dev, int32_t width,
                         const AllowGroups& allow_dev) {
  const bool allow = width != 0;  // rpt_graph_search_allow_*
  const int m = graph_metric_of(metric);
  if (m == kGraphCosine) {  // the rows' dot(x, x), cached on the two datasets
    RPT_TRY(ensure_sqnorm(ctx, data));
    RPT_TRY(ensure_sqnorm(ctx, queries));
  }
  if (!ctx->search_state_dev) {
    hipError_t e = dev_alloc(&ctx->search_state_dev, sizeof(SearchState));
    if (e != hipSuccess)
      return fail(RPT_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  }
  SearchArgs a = {};
  a.n = data->n;
  a.nq = queries->n;
  a.d = data->d;
  a.kg = kg;
  a.s = s;
  a.k = k;
  a.ef = ef;
  a.width = allow ? width : ef;
  search_shape(a);
  a.qres = a.d <= kQMax ? 1 : 0;
  a.vec = 0;
  a.nofilter = ctx->opt.graph_search_nofilter != 0 ? 1 : 0;
  const int efp = ((a.width + 63) / 64) * 64;
  // an allow-list beam keeps a byte per entry behind the offer's ids
  a.wave_bytes = (int)(((size_t)(a.R * kLS + (a.qres ? a.d : kCW) + efp) * 8 +
                        (size_t)(efp + a.H + a.R) * 4 + (allow ? efp : 0) + 7) & ~(size_t)7);
  if (!allow && 4 * a.wave_bytes > kLdsMax)
    return fail(RPT_E_INTERNAL, "graph search: the beam does not fit LDS");
  a.gids = gids_dev;
  a.gcount = gcount_dev;
  a.seeds = seeds_dev;
  a.allow = allow_dev;
  a.rn = m == kGraphCosine ? data->sqnorm : nullptr;
  a.qn = m == kGraphCosine ? queries->sqnorm : nullptr;
  a.ids = ids_dev;
  a.dist = dist_dev;
  a.count = count_dev;
  a.st = static_cast<SearchState*>(ctx->search_state_dev);

  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  hipLaunchKernelGGL(search_begin_kernel, dim3(1), dim3(64), 0, ctx->stream, a.st);
  RPT_HIP(hipGetLastError());
  if (a.nq == 0) return RPT_OK;
  switch (data->dtype) {
    case RPT_F64:
      return launch_search_beam<double>(m, ctx, data, queries, a, allow);
    case RPT_F32:
      return launch_search_beam<float>(m, ctx, data, queries, a, allow);
    default:
      return launch_search_beam<uint16_t>(m, ctx, data, queries, a, allow);
  }
}

int32_t graph_search_last(rpt_ctx* ctx, int64_t* expansions, int64_t* evaluated) {
  *expansions = *evaluated = 0;
  if (!ctx->search_state_dev) return RPT_OK;  // no call yet
  RPT_HIP(stream_sync(ctx->stream));
  SearchState h;
  RPT_HIP(hipMemcpy(&h, ctx->search_state_dev, sizeof h, hipMemcpyDeviceToHost));
  *expansions = (int64_t)h.expansions;
  *evaluated = (int64_t)h.evaluated;
  return RPT_OK;
}

}  // namespace rpt
