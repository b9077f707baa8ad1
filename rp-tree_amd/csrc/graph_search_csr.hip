// graph_search_csr.hip — the beam search over a kNN graph on SVector (CSR) rows under L2
// (rpt_graph_search_csr_*) and under cosine / inner product (rpt_graph_search_csr_metric_*).
//
// The answer is the definition of include/rptree_hip.h for rpt_graph_search_* with dist(q, v) =
// metricDDL2's left fold over dense(q), dense(x_v) (graph_csr.hip: absent columns +0.0, f32 values
// widened exactly, a stored zero a zero).  A column where both hold +0.0 adds +0.0 to an accumulator
// that is never -0.0, so the fold over the ascending union of the two supports gives the bits of the
// fold over all d columns, and the answer is bit-equal to graph_search.hip's on the dense-ified rows
// and queries.
//
// graph_search_csr_kernel: one WAVE owns a query, four queries per workgroup; the beam, the visited
// filter and the offers are graph_search_kernel's (graph_dev.h: beam_next_offer, beam_admit,
// beam_insert).  Only the distance step differs: a candidate per lane walks its own CSR row
// two-pointer style against the query's (column, value) pairs, as refine_join_csr_kernel
// (graph_csr.hip) walks against x_i's: every step takes an entry of one side or of both, the absent
// side is 0.0, the candidate's tail is folded behind the query's last column.  No chunk of dense
// columns is staged.  Per wave in LDS:
//   qv/qc  qcap doubles / ints  the query's values, widened once, and its columns
//   bd/bi, tab, sid             the beam, the visited filter and the running offer's ids (graph_dev.h)
// Every offer of a search reads the query again, so a query of at most qcap entries stays in LDS for
// the whole search (resident); a longer one passes through qv/qc[0 .. kPiece) in pieces of kPiece
// entries per offer (streamed), and needs no more LDS than a short one.  The choice is per query and
// wave-uniform; the context option graph_search_csr_stream streams every query.  Both paths fold the
// same entries in the same order.
// Rows whose columns do not ascend strictly give an unspecified answer; a cursor never passes its
// row's end and every step of a walk advances one, so the kernel stays in bounds and terminates.
//
// Cosine / inner product (M != kGraphL2): the distance comes from dotS (rptree_hip.h), the left fold
// of x_c * y_c over the columns stored in BOTH rows, which is what the two-pointer walk meets when
// both cursors stand on one column.  So a step folds only then, a step that advances one side does no
// arithmetic, a lane stops when its candidate row or the query's entries are over, and there is no
// tail.  No zero stands in for an absent entry: a stored inf or NaN meets only what the other row
// stores.  Cosine reads dotS(q, q) once per query and dotS(x_v, x_v) in the epilogue, both from
// rpt_dataset::sqnorm (the same fold), as graph_search.hip does; LDS is what the L2 kernel takes.
//
// graph_search_csr_allow_kernel (rpt_graph_search_allow_* on CSR rows): the same search among the ids of
// an allow-list, as graph_search_allow_kernel is to graph_search_kernel: one body (graph_search_csr_body),
// the beam's switch F on, 4, 2 or 1 waves per workgroup by search_waves.
#include <algorithm>

#include "graph_dev.h"

namespace rpt {
namespace {

constexpr int kLdsMax = 160 * 1024;
constexpr int kNoCol = 0x7fffffff;  // a cursor at its row's end
constexpr int kPiece = 64;          // (column, value) pairs of a streamed query per LDS piece
// Entries up to which a query stays in LDS.  Four waves, each with an ef = 256 beam (256 x 12 B),
// the largest filter (2048 x 4 B) and 64 offer ids, take 4 x 11 520 B; what is left of 160 KB holds
// 4 x 2453 entries of 12 B.  2048 is the power of two below.
constexpr int kQCap = 2048;

// the candidate row of a lane: [jp, je), cj / vj its entry at jp (cj == kNoCol: the row is over)
struct RowWalk {
  int64_t jp, je;
  int cj;
  double vj;
};

// L2: folds the query entries pc/pv[0 .. np) and what the candidate holds up to the last of them.
// Cosine / inner product: folds the columns that pc[0 .. np) and the candidate both hold, and stops
// at the end of either.
template <class TV, int M>
__device__ __forceinline__ double merge_piece(double acc, const int* pc, const double* pv, int np, RowWalk& w,
                                              const int32_t* __restrict__ col, const TV* __restrict__ val) {
  int ii = 0;
  if constexpr (M != kGraphL2) {
    while (ii < np && w.jp < w.je) {  // every step advances the query, the candidate or both
      const int ci = pc[ii];
      const bool take_q = ci <= w.cj, take_j = w.cj <= ci;
      if (take_q && take_j) acc = fold_step<M>(acc, pv[ii], w.vj);
      if (take_q) ++ii;
      if (take_j) {
        ++w.jp;
        if (w.jp < w.je) {
          w.cj = col[w.jp];
          w.vj = widen(val[w.jp]);
        }
      }
    }
    return acc;
  }
  while (ii < np) {  // every step takes an entry of the query or of the candidate
    const int ci = pc[ii];
    const bool take_q = ci <= w.cj, take_j = w.cj <= ci;
    acc = fold_step<kGraphL2>(acc, take_q ? pv[ii] : 0.0, take_j ? w.vj : 0.0);
    if (take_q) ++ii;
    if (take_j) {
      ++w.jp;
      w.cj = kNoCol;
      if (w.jp < w.je) {
        w.cj = col[w.jp];
        w.vj = widen(val[w.jp]);
      }
    }
  }
  return acc;
}

// The search of one workgroup; F and J are the beam's switches of graph_dev.h, as in graph_search.hip:
// F on is the beam of rpt_graph_search_allow_*, with its allowed bytes `ba` behind the offer's ids.
template <class TV, int M, bool F, int J>
__device__ __forceinline__ void graph_search_csr_body(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const TV* __restrict__ val,
    const int64_t* __restrict__ qrowptr, const int32_t* __restrict__ qcol, const TV* __restrict__ qval,
    const SearchArgs& a, double* smem) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int nj = ((F ? a.width : a.ef) + 63) >> 6, efp = nj * 64;
  const int ef = a.ef;
  double* qv = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * a.wave_bytes);
  double* bd = qv + a.qcap;
  int* qc = reinterpret_cast<int*>(bd + efp);
  int* bi = qc + a.qcap;
  int* tab = bi + efp;
  int* sid = tab + a.H;
  unsigned char* ba = reinterpret_cast<unsigned char*>(sid + a.R);  // F only
  const bool filter = a.nofilter == 0;
  unsigned long long n_exp = 0, n_eval = 0;

  for (int64_t qi = (int64_t)blockIdx.x * W + wave; qi < a.nq; qi += (int64_t)gridDim.x * W) {
    const int64_t qb = qrowptr[qi], qe = qrowptr[qi + 1];
    const bool resident = a.stream == 0 && qe - qb <= (int64_t)a.qcap;  // wave-uniform
    wave_sync();  // the last query's beam has been written out
    if (resident)
      for (int64_t p = qb + lane; p < qe; p += 64) {
        qc[p - qb] = qcol[p];
        qv[p - qb] = widen(qval[p]);
      }
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

      // ---- the distances: a candidate per lane walks its row against the query's entries
      const int my = lane < nrows ? sid[lane] : -1;
      RowWalk w = {0, 0, kNoCol, 0.0};
      if (my >= 0) {
        w.jp = rowptr[my];
        w.je = rowptr[my + 1];
      }
      if (w.jp < w.je) {
        w.cj = col[w.jp];
        w.vj = widen(val[w.jp]);
      }
      double acc = 0.0;
      if (resident) {
        if (my >= 0) acc = merge_piece<TV, M>(acc, qc, qv, (int)(qe - qb), w, col, val);
      } else {
        for (int64_t p0 = qb; p0 < qe; p0 += kPiece) {
          if constexpr (M != kGraphL2) {  // wave-uniform: every candidate row of the offer is over
            if (!__ballot(w.jp < w.je)) break;
          }
          const int np = qe - p0 < kPiece ? (int)(qe - p0) : kPiece;
          wave_sync();  // the last piece has been read
          if (lane < np) {
            qc[lane] = qcol[p0 + lane];
            qv[lane] = widen(qval[p0 + lane]);
          }
          wave_sync();
          if (my >= 0) acc = merge_piece<TV, M>(acc, qc, qv, np, w, col, val);
        }
      }
      if constexpr (M == kGraphL2) {
        while (w.jp < w.je) {  // what the candidate holds behind the query's last column
          acc = fold_step<kGraphL2>(acc, 0.0, w.vj);
          ++w.jp;
          if (w.jp < w.je) w.vj = widen(val[w.jp]);
        }
      }
      double nrm = 0.0;
      if constexpr (M == kGraphCosine) nrm = my >= 0 ? a.rn[my] : 0.0;
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

template <class TV, int M>
__global__ __launch_bounds__(256) void graph_search_csr_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const TV* __restrict__ val,
    const int64_t* __restrict__ qrowptr, const int32_t* __restrict__ qcol, const TV* __restrict__ qval,
    SearchArgs a) {
  extern __shared__ double smem[];
  graph_search_csr_body<TV, M, false, kBeamJ>(rowptr, col, val, qrowptr, qcol, qval, a, smem);
}

// rpt_graph_search_allow_* on CSR rows: J = kBeamJ for a width up to 256, kBeamJWide beyond
template <class TV, int M, int J>
__global__ __launch_bounds__(256) void graph_search_csr_allow_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const TV* __restrict__ val,
    const int64_t* __restrict__ qrowptr, const int32_t* __restrict__ qcol, const TV* __restrict__ qval,
    SearchArgs a) {
  extern __shared__ double smem[];
  graph_search_csr_body<TV, M, true, J>(rowptr, col, val, qrowptr, qcol, qval, a, smem);
}

// J == 0: graph_search_csr_kernel, four waves per workgroup; else graph_search_csr_allow_kernel<J>, as
// many of 4, 2 or 1 as search_waves picks
template <class TV, int M, int J>
int32_t launch_search_csr(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                          const SearchArgs& a) {
  void (*kern)(const int64_t*, const int32_t*, const TV*, const int64_t*, const int32_t*, const TV*, SearchArgs);
  if constexpr (J == 0) kern = graph_search_csr_kernel<TV, M>;
  else kern = graph_search_csr_allow_kernel<TV, M, J>;
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  const int W = J == 0 ? 4 : search_waves(a.wave_bytes, kLdsMax);
  const int64_t want = (a.nq + W - 1) / W;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->n_cu * 64));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * W), (size_t)a.wave_bytes * W, ctx->stream, data->rowptr,
                     data->col, static_cast<const TV*>(data->val), queries->rowptr, queries->col,
                     static_cast<const TV*>(queries->val), a);
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

template <class TV, int J>
int32_t launch_search_csr_metric(int m, rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                 const SearchArgs& a) {
  if (m == kGraphCosine) return launch_search_csr<TV, kGraphCosine, J>(ctx, data, queries, a);
  if (m == kGraphInner) return launch_search_csr<TV, kGraphInner, J>(ctx, data, queries, a);
  return launch_search_csr<TV, kGraphL2, J>(ctx, data, queries, a);
}

template <class TV>
int32_t launch_search_csr_beam(int m, rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                               const SearchArgs& a, bool allow) {
  if (!allow) return launch_search_csr_metric<TV, 0>(m, ctx, data, queries, a);
  if (a.width <= 64 * kBeamJ) return launch_search_csr_metric<TV, kBeamJ>(m, ctx, data, queries, a);
  return launch_search_csr_metric<TV, kBeamJWide>(m, ctx, data, queries, a);
}

}  // namespace

int32_t graph_search_csr_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                             int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                             const int32_t* seeds_dev, int32_t k, int32_t ef, int32_t metric,
                             int32_t* ids_dev, double* dist_dev, int32_t* count_dev, int32_t width,
                             const AllowGroups& allow_dev) {
  const bool allow = width != 0;  // rpt_graph_search_allow_*
  const int m = graph_metric_of(metric);
  if (m == kGraphCosine) {  // the rows' dotS(x, x), cached on the two datasets
    RPT_TRY(ensure_sqnorm(ctx, data));
    RPT_TRY(ensure_sqnorm(ctx, queries));
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
  a.nofilter = ctx->opt.graph_search_nofilter != 0 ? 1 : 0;
  a.stream = ctx->opt.graph_search_csr_stream != 0 ? 1 : 0;
  // a row of ascending columns holds at most d entries: no more LDS than any query can fill
  a.qcap = std::max<int>(kPiece, std::min<int>(kQCap, a.d));
  const int efp = ((a.width + 63) / 64) * 64;
  // an allow-list beam keeps a byte per entry behind the offer's ids
  a.wave_bytes = (int)(((size_t)(a.qcap + efp) * 12 + (size_t)(a.H + a.R) * 4 + (allow ? efp : 0) + 7) &
                       ~(size_t)7);
  if (!allow && 4 * a.wave_bytes > kLdsMax) return fail(RPT_E_INTERNAL, "graph search: the beam does not fit LDS");
  if (!ctx->search_state_dev) {
    hipError_t e = dev_alloc(&ctx->search_state_dev, sizeof(SearchState));
    if (e != hipSuccess)
      return fail(RPT_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  }
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
  if (data->dtype == RPT_F64) return launch_search_csr_beam<double>(m, ctx, data, queries, a, allow);
  return launch_search_csr_beam<float>(m, ctx, data, queries, a, allow);
}

}  // namespace rpt
