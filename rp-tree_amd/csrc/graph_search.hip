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
//   bd/bi ef doubles / ints  the beam, sorted; bi holds id (unexpanded) or ~id (expanded)
//   tab   H ints             the visited filter: a hash of evaluated ids, kProbe slots per id, a
//                            full neighbourhood is overwritten (lossy)
//   sid   R ints             the ids of the running offer that are evaluated
// An offer: a candidate per lane, dropped when the filter or the beam (exactly) holds it, the rest
// compacted, their rows staged chunk by chunk (wave_stage) and folded a candidate per lane, columns
// ascending (fold_step / fold_finish: the reference's fold), then inserted one by one: rank by
// ballot / popcount over the lanes' entries (lane l looks at positions l, l + 64, ...), the tail
// shifted by one in LDS.  No atomics touch the beam; the filter's atomics only decide what is
// evaluated twice.  The loops are bounded by the definition: ceil(s / R) seed offers, at most n
// expansions.
#include <algorithm>

#include "graph_dev.h"

namespace rpt {
namespace {

constexpr int kEmpty = (int)0x80000000;  // free slot of the filter (never an id)
constexpr int kLdsMax = 160 * 1024;
constexpr int kQMax = 1024;  // columns up to which the query stays in LDS whole
constexpr int kProbe = 8;    // slots of the filter an id may take
constexpr int kBeamJ = RPT_GRAPH_SEARCH_MAX_EF / 64;  // beam entries a lane looks after

struct SearchState {
  unsigned long long expansions, evaluated;
};

struct SearchArgs {
  int64_t n, nq;
  int d, kg, s, k, ef;
  int R, H, qres, vec, nofilter, wave_bytes;
  const int32_t* gids;
  const int32_t* gcount;
  const int32_t* seeds;
  const double* rn;  // dot(x, x) of the data rows (cosine)
  const double* qn;  // ... of the queries
  int32_t* ids;
  double* dist;
  int32_t* count;
  SearchState* st;
};

__global__ void search_begin_kernel(SearchState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->expansions = 0;
    st->evaluated = 0;
  }
}

__device__ inline int beam_id(int v) { return v < 0 ? ~v : v; }

template <class TD, int M>
__global__ __launch_bounds__(256) void graph_search_kernel(const TD* __restrict__ X,
                                                           const TD* __restrict__ Q, SearchArgs a) {
  extern __shared__ double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int nj = (a.ef + 63) >> 6, efp = nj * 64;
  const int d = a.d, ef = a.ef, R = a.R;
  double* buf = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * a.wave_bytes);
  double* qv = buf + R * kLS;
  double* bd = qv + (a.qres ? d : kCW);
  int* bi = reinterpret_cast<int*>(bd + efp);
  int* tab = bi + efp;
  int* sid = tab + a.H;
  const int mask = a.H - 1, shift = 32 - (31 - __clz(a.H));
  const unsigned long long below = (1ULL << lane) - 1;
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

    int c = 0;  // entries of the beam
    int s0 = 0;
    int64_t expanded = 0;
    for (;;) {
      // ---- the next offer: a batch of seeds, then the row of the first unexpanded entry
      int cand = -1;
      if (s0 < a.s) {
        if (lane < R && s0 + lane < a.s) cand = a.seeds[qi * a.s + s0 + lane];
        s0 += R;
      } else {
        if (expanded >= a.n) break;  // every point at most once
        int pos = -1;
        for (int j = 0; j < nj && pos < 0; ++j) {
          const int p = j * 64 + lane;
          const unsigned long long bal = __ballot(p < c && bi[p] >= 0);
          if (bal) pos = j * 64 + __ffsll((long long)bal) - 1;
        }
        if (pos < 0) break;
        const int u = __builtin_amdgcn_readfirstlane(bi[pos]);
        wave_sync();
        if (lane == 0) bi[pos] = ~u;
        wave_sync();
        ++expanded;
        const int g = a.gcount[u];
        if (g >= 0 && g <= a.kg && lane < g) cand = a.gids[(int64_t)u * a.kg + lane];
      }

      // ---- drop what is outside [0, n), what the filter remembers, what the beam holds
      bool v = cand >= 0 && (int64_t)cand < a.n;
      const unsigned h = ((unsigned)cand * 2654435761u) >> shift;
      if (filter && v) {
        for (int pr = 0; pr < kProbe; ++pr) {
          const int t = tab[(h + pr) & (unsigned)mask];
          if (t == cand) v = false;
          if (t == cand || t == kEmpty) break;
        }
      }
      if (__ballot(v)) {
        for (int p = 0; p < c; ++p)
          if (beam_id(bi[p]) == cand) v = false;
      }
      const unsigned long long bal = __ballot(v);
      const int nrows = __popcll(bal);
      if (nrows == 0) continue;
      n_eval += (unsigned long long)nrows;
      if (filter && v) {
        bool done = false;
        for (int pr = 0; pr < kProbe && !done; ++pr) {
          const int old = atomicCAS(&tab[(h + pr) & (unsigned)mask], kEmpty, cand);
          done = old == kEmpty || old == cand;
        }
        if (!done) tab[h] = cand;  // a full neighbourhood: forget whoever sat at home
      }
      if (v) sid[__popcll(bal & below)] = cand;
      wave_sync();

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

      // ---- into the beam, one at a time
      v = lane < nrows;
      for (;;) {
        if (c == ef) {  // a full beam: only what comes before its last entry can enter
          const double td = bd[c - 1];
          const int ti = beam_id(bi[c - 1]);
          v = v && before(cd, my, td, ti);
        }
        const unsigned long long m = __ballot(v);
        if (!m) break;
        const int src = __ffsll((long long)m) - 1;
        const double nd = __shfl(cd, src);
        const int ni = __shfl(my, src);
        if (lane == src) v = false;
        double ed[kBeamJ];
        int ei[kBeamJ];
        int p = 0;
        bool dup = false;
#pragma unroll
        for (int j = 0; j < kBeamJ; ++j)
          if (j < nj) {
            const int pos = j * 64 + lane;
            const bool on = pos < c;
            ed[j] = on ? bd[pos] : 0.0;
            ei[j] = on ? bi[pos] : kEmpty;
            dup |= on && beam_id(ei[j]) == ni;
            p += __popcll(__ballot(on && before(ed[j], beam_id(ei[j]), nd, ni)));
          }
        if (__ballot(dup)) continue;  // the same id twice in one offer
        const int newc = c < ef ? c + 1 : c;
        wave_sync();  // every entry has been read
#pragma unroll
        for (int j = 0; j < kBeamJ; ++j)
          if (j < nj) {
            const int pos = j * 64 + lane;
            if (pos >= p && pos < c && pos + 1 < newc) {
              bd[pos + 1] = ed[j];
              bi[pos + 1] = ei[j];
            }
          }
        if (lane == 0) {
          bd[p] = nd;
          bi[p] = ni;
        }
        wave_sync();
        c = newc;
      }
    }
    n_exp += (unsigned long long)expanded;

    const int found = c < a.k ? c : a.k;
    if (lane < a.k) {
      const bool on = lane < found;
      a.ids[qi * a.k + lane] = on ? beam_id(bi[lane]) : -1;
      a.dist[qi * a.k + lane] = on ? bd[lane] : pos_inf();
    }
    if (lane == 0) a.count[qi] = found;
  }
  if (lane == 0 && (n_exp | n_eval)) {
    atomicAdd(&a.st->expansions, n_exp);
    atomicAdd(&a.st->evaluated, n_eval);
  }
}

template <class TD, int M>
int32_t launch_search(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, SearchArgs a) {
  const TD* X = static_cast<const TD*>(data->X);
  const TD* Q = static_cast<const TD*>(queries->X);
  a.vec = ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && ((size_t)a.d * sizeof(TD)) % 16 == 0) ? 1 : 0;
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)graph_search_kernel<TD, M>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  const int W = 4;
  const int64_t want = (a.nq + W - 1) / W;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->n_cu * 64));
  hipLaunchKernelGGL((graph_search_kernel<TD, M>), dim3(grid), dim3(64 * W), (size_t)a.wave_bytes * W,
                     ctx->stream, X, Q, a);
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

template <class TD>
int32_t launch_search_metric(int m, rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                             const SearchArgs& a) {
  if (m == kGraphCosine) return launch_search<TD, kGraphCosine>(ctx, data, queries, a);
  if (m == kGraphInner) return launch_search<TD, kGraphInner>(ctx, data, queries, a);
  return launch_search<TD, kGraphL2>(ctx, data, queries, a);
}

}  // namespace

int32_t graph_search_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, int32_t kg,
                         const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                         const int32_t* seeds_dev, int32_t k, int32_t ef, int32_t metric,
                         int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
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
  SearchArgs a;
  a.n = data->n;
  a.nq = queries->n;
  a.d = data->d;
  a.kg = kg;
  a.s = s;
  a.k = k;
  a.ef = ef;
  // an offer holds a graph row whole; seeds come in batches of the same size
  a.R = std::max<int>(kg, std::min<int>(s, 16));
  // the filter: eight slots per beam entry, 1 to 8 KB
  a.H = 256;
  while (a.H < 8 * ef && a.H < 2048) a.H <<= 1;
  a.qres = a.d <= kQMax ? 1 : 0;
  a.vec = 0;
  a.nofilter = ctx->opt.graph_search_nofilter != 0 ? 1 : 0;
  const int efp = ((ef + 63) / 64) * 64;
  a.wave_bytes = (int)(((size_t)(a.R * kLS + (a.qres ? a.d : kCW) + efp) * 8 +
                        (size_t)(efp + a.H + a.R) * 4 + 7) & ~(size_t)7);
  if (4 * a.wave_bytes > kLdsMax) return fail(RPT_E_INTERNAL, "graph search: the beam does not fit LDS");
  a.gids = gids_dev;
  a.gcount = gcount_dev;
  a.seeds = seeds_dev;
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
      return launch_search_metric<double>(m, ctx, data, queries, a);
    case RPT_F32:
      return launch_search_metric<float>(m, ctx, data, queries, a);
    default:
      return launch_search_metric<uint16_t>(m, ctx, data, queries, a);
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
