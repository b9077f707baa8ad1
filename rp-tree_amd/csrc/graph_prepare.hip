// graph_prepare.hip — a kNN graph made ready for the search (rpt_graph_prepare_*): occluded
// neighbours dropped (DIVERSIFY), reverse edges added (REVERSE), the degree capped at kout.
//
// Kept(i): the valid entries of row i; with DIVERSIFY, in stored order, e_m stays unless a kept
// e_l (l < m) has dist(e_l, e_m) < the distance stored with e_m.  Union(i): Kept(i) joined, with
// REVERSE, by {j : i in Kept(j)} at the distance stored in row j.  Row i of the output: the first
// kout of Union(i) by (distance, id).  The caller's graph is read only.
//
// Kernels, in stream order:
//   prep_begin_kernel      the call's counters to 0
//   graph_diversify_kernel (DIVERSIFY) one WAVE owns point i, four points per workgroup.  The row is
//                          compacted to its valid entries (LDS: ids, stored distances, dot(x, x)
//                          for cosine), their <= k data rows are staged chunk by chunk (32 columns,
//                          wave_stage), and the lanes own the pairs (l, m), l < m: pair p =
//                          m (m - 1) / 2 + l on lane p mod 64, NA = ceil(k (k - 1) / 128) of them
//                          per lane (a template argument: 1, 2, 4, 8, 16 or 32 accumulators carried
//                          through the chunks in registers).  After the last chunk one ballot per
//                          accumulator index gives the occlusion bits of 64 pairs; the pairs of an
//                          m are consecutive, so lane m cuts its word of m bits out of them and a
//                          loop of c - 1 wave-uniform steps resolves the serial keep rule.  Kept
//                          entries are compacted into a scratch graph.
//   rev_zero / _degree / _scan / _fill (REVERSE; graph_dev.h) the CSR of the reverse edges of Kept
//   prep_merge_kernel      one wave per point holds the output row one entry per lane: Kept(i)
//                          enters it (as it stands when it is sorted, else through wave_merge), then
//                          the reverse list in chunks of 64 through wave_merge, ids of Kept(i) taken
//                          out first (the distance stored in row i wins, also for an entry behind
//                          the cap).  The loop is bounded by the list's length.
// No atomics touch a list; the counters are sums.  The order inside a reverse list depends on the
// arrival of the fill's atomics, the answer is the first kout of a set under a total order.
#include <string.h>

#include <algorithm>

#include "graph_dev.h"

namespace rpt {
namespace {

constexpr int kLdsMax = 160 * 1024;

struct PrepState {
  unsigned long long pairs, occluded, capped;
  int32_t one;  // the `active` word of the rev_* kernels
  int32_t pad;
};

__global__ void prep_begin_kernel(PrepState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->pairs = 0;
    st->occluded = 0;
    st->capped = 0;
    st->one = 1;
    st->pad = 0;
  }
}

// pair p = m (m - 1) / 2 + l, l < m
__device__ inline void pair_of(int p, int& l, int& m) {
  m = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
  while (m * (m - 1) / 2 > p) --m;
  while ((m + 1) * m / 2 <= p) ++m;
  l = p - m * (m - 1) / 2;
}

// dynamic LDS, per wave (wave_bytes): k * kLS doubles (a chunk of the neighbours' rows), k doubles
// (stored distances), k doubles (dot(x, x), cosine), NA + 1 words (the ballots), k ints (ids)
template <class TD, int M, int NA>
__global__ __launch_bounds__(256) void graph_diversify_kernel(
    PrepState* st, const TD* __restrict__ X, int64_t n, int d, int k, int vec, int wave_bytes,
    const int32_t* __restrict__ ids, const double* __restrict__ dist,
    const int32_t* __restrict__ count, int32_t* __restrict__ kids, double* __restrict__ kdist,
    int32_t* __restrict__ kcount, const double* __restrict__ rn) {
  extern __shared__ double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  double* buf = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * wave_bytes);
  double* sd = buf + k * kLS;
  double* nr = sd + k;
  unsigned long long* bal = reinterpret_cast<unsigned long long*>(nr + k);
  int* sid = reinterpret_cast<int*>(bal + NA + 1);
  const unsigned long long below = (1ULL << lane) - 1;
  unsigned long long n_pairs = 0, n_occ = 0;

  for (int64_t i = (int64_t)blockIdx.x * W + wave; i < n; i += (int64_t)gridDim.x * W) {
    int c = count[i];
    c = c < 0 ? 0 : (c > k ? k : c);
    int id = -1;
    double dv = pos_inf();
    if (lane < c) {
      id = ids[i * k + lane];
      dv = dist[i * k + lane];
    }
    const bool ok = lane < c && (unsigned)id < (unsigned long long)n;
    const unsigned long long vm = __ballot(ok);
    const int cc = __popcll(vm);
    wave_sync();  // the last point's rows have been read
    if (ok) {
      const int pos = __popcll(vm & below);
      sid[pos] = id;
      sd[pos] = dv;
      if constexpr (M == kGraphCosine) nr[pos] = rn[id];
    }
    wave_sync();
    const int P = cc * (cc - 1) / 2;

    unsigned long long kept = cc > 0 ? 1ULL : 0ULL;
    if (P > 0) {
      int lm[NA];  // l | m << 8; pairs behind P read row 0 and are not looked at
      double acc[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int p = lane + 64 * a;
        int l = 0, m = 0;
        if (p < P) pair_of(p, l, m);
        lm[a] = l | (m << 8);
        acc[a] = 0.0;
      }
      for (int c0 = 0; c0 < d; c0 += kCW) {
        const int cw = d - c0 < kCW ? d - c0 : kCW;
        wave_sync();  // the last chunk has been read
        wave_stage<TD>(X, d, sid, cc, c0, cw, buf, vec != 0);
        wave_sync();
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          if (64 * a < P) {  // wave-uniform
            const double* ra = buf + (lm[a] & 255) * kLS;
            const double* rb = buf + (lm[a] >> 8) * kLS;
            double s = acc[a];
#pragma unroll 4
            for (int col = 0; col < cw; ++col) s = fold_step<M>(s, ra[col], rb[col]);
            acc[a] = s;
          }
        }
      }
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int l = lm[a] & 255, m = lm[a] >> 8;
        double ni = 0.0, nj = 0.0;
        if constexpr (M == kGraphCosine) {
          ni = nr[l];
          nj = nr[m];
        }
        const bool occ = lane + 64 * a < P && fold_finish<M>(acc[a], ni, nj) < sd[m];
        const unsigned long long b = __ballot(occ);
        if (lane == 0) bal[a] = b;
      }
      if (lane == 0) bal[NA] = 0;
      wave_sync();
      // lane m: bit l of `mine` = e_l occludes e_m
      unsigned long long mine = 0;
      if (lane >= 1 && lane < cc) {
        const int start = lane * (lane - 1) / 2, w = start >> 6, sh = start & 63;
        mine = bal[w] >> sh;
        if (sh + lane > 64) mine |= bal[w + 1] << (64 - sh);
        mine &= (1ULL << lane) - 1;
      }
      for (int m = 1; m < cc; ++m) {
        const unsigned long long om = __shfl(mine, m);
        if (!(om & kept)) kept |= 1ULL << m;
      }
    }
    const int kc = __popcll(kept);
    if (lane < cc && ((kept >> lane) & 1)) {
      const int pos = __popcll(kept & below);
      kids[i * k + pos] = sid[lane];
      kdist[i * k + pos] = sd[lane];
    }
    if (lane >= kc && lane < k) {
      kids[i * k + lane] = -1;
      kdist[i * k + lane] = pos_inf();
    }
    if (lane == 0) kcount[i] = kc;
    n_pairs += (unsigned long long)P;
    n_occ += (unsigned long long)(cc - kc);
  }
  if (lane == 0 && (n_pairs | n_occ)) {
    atomicAdd(&st->pairs, n_pairs);
    atomicAdd(&st->occluded, n_occ);
  }
}

// (ids, dist, count): Kept as the diversify kernel left it, or the caller's graph (entries out of
// range are skipped here); roff == nullptr: no reverse edges
__global__ __launch_bounds__(256) void prep_merge_kernel(
    PrepState* st, int64_t n, int k, int kout, const int32_t* __restrict__ ids,
    const double* __restrict__ dist, const int32_t* __restrict__ count,
    const int64_t* __restrict__ roff, const int32_t* __restrict__ rsrc,
    const double* __restrict__ rdist, int32_t* __restrict__ oids, double* __restrict__ odist,
    int32_t* __restrict__ ocount) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  unsigned long long n_cap = 0;
  for (int64_t i = (int64_t)blockIdx.x * W + wave; i < n; i += (int64_t)gridDim.x * W) {
    int c = count[i];
    c = c < 0 ? 0 : (c > k ? k : c);
    int kid = -1;
    double kd = pos_inf();
    if (lane < c) {
      kid = ids[i * k + lane];
      kd = dist[i * k + lane];
    }
    const bool ok = lane < c && (unsigned)kid < (unsigned long long)n;
    if (!ok) kid = -1;
    const unsigned long long vm = __ballot(ok);
    const int kc = __popcll(vm);

    // a row without gaps and in strict (distance, id) order enters as it stands
    const double pd = __shfl_up(kd, 1);
    const int pi = __shfl_up(kid, 1);
    const bool bad = ok && lane > 0 && !before(pd, pi, kd, kid);
    double ld = pos_inf();
    int lid = -1, lc = 0;
    if (vm == (c >= 64 ? ~0ULL : (1ULL << c) - 1) && !__ballot(bad)) {
      lc = kc < kout ? kc : kout;
      if (lane < lc) {
        ld = kd;
        lid = kid;
      }
    } else {
      wave_merge(ld, lid, lc, kout, kd, kid, ok, 0.0, -1, false);
    }

    int64_t extra = 0;  // |Union(i)| - |Kept(i)|
    if (roff) {
      const int64_t o0 = roff[i], deg = roff[i + 1] - o0;
      for (int64_t b = 0; b < deg; b += 64) {
        bool on = b + lane < deg;
        const double cd = on ? rdist[o0 + b + lane] : 0.0;
        const int ci = on ? rsrc[o0 + b + lane] : -2;
        for (int s = 0; s < c; ++s) {
          const int kv = __shfl(kid, s);  // by every lane: a lane that is off may hold the entry asked for
          on = on && ci != kv;
        }
        extra += __popcll(__ballot(on));
        wave_merge(ld, lid, lc, kout, cd, ci, on, 0.0, -1, false);
      }
    }

    if (lane < kout) {
      odist[i * kout + lane] = lane < lc ? ld : pos_inf();
      oids[i * kout + lane] = lane < lc ? lid : -1;
    }
    if (lane == 0) ocount[i] = lc;
    n_cap += (unsigned long long)(kc + extra - lc);
  }
  if (lane == 0 && n_cap) atomicAdd(&st->capped, n_cap);
}

struct DivArgs {
  rpt_ctx* ctx;
  PrepState* st;
  const rpt_dataset* data;
  int k, wave_bytes;
  const int32_t *ids, *count;
  const double* dist;
  int32_t *kids, *kcount;
  double* kdist;
};

template <class TD, int M, int NA>
int32_t launch_diversify(const DivArgs& a) {
  const TD* X = static_cast<const TD*>(a.data->X);
  const int d = a.data->d;
  const int vec = ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && ((size_t)d * sizeof(TD)) % 16 == 0) ? 1 : 0;
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(a.ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)graph_diversify_kernel<TD, M, NA>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  constexpr int W = 4;
  const int64_t want = (a.data->n + W - 1) / W;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)a.ctx->n_cu * 16));
  hipLaunchKernelGGL((graph_diversify_kernel<TD, M, NA>), dim3(grid), dim3(64 * W), (size_t)a.wave_bytes * W,
                     a.ctx->stream, a.st, X, a.data->n, d, a.k, vec, a.wave_bytes, a.ids, a.dist, a.count,
                     a.kids, a.kdist, a.kcount, M == kGraphCosine ? a.data->sqnorm : nullptr);
  return RPT_OK;
}

// accumulators per lane: pairs of a full row over 64 lanes, rounded up to a power of two
inline int pair_bucket(int k) {
  const int need = (k * (k - 1) / 2 + 63) / 64;
  int na = 1;
  while (na < need) na <<= 1;
  return na;
}

template <class TD, int M>
int32_t launch_diversify_na(int na, const DivArgs& a) {
  switch (na) {
    case 1: return launch_diversify<TD, M, 1>(a);
    case 2: return launch_diversify<TD, M, 2>(a);
    case 4: return launch_diversify<TD, M, 4>(a);
    case 8: return launch_diversify<TD, M, 8>(a);
    case 16: return launch_diversify<TD, M, 16>(a);
    default: return launch_diversify<TD, M, 32>(a);
  }
}

template <class TD>
int32_t launch_diversify_metric(int m, int na, const DivArgs& a) {
  if (m == kGraphCosine) return launch_diversify_na<TD, kGraphCosine>(na, a);
  if (m == kGraphInner) return launch_diversify_na<TD, kGraphInner>(na, a);
  return launch_diversify_na<TD, kGraphL2>(na, a);
}

}  // namespace

int32_t graph_prepare_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_dev,
                          const double* dist_dev, const int32_t* count_dev, int32_t kout, int32_t metric,
                          int32_t flags, int32_t* out_ids_dev, double* out_dist_dev,
                          int32_t* out_count_dev) {
  const int m = graph_metric_of(metric);
  const bool diversify = (flags & RPT_GRAPH_PREP_DIVERSIFY) != 0, reverse = (flags & RPT_GRAPH_PREP_REVERSE) != 0;
  if (diversify && m == kGraphCosine) RPT_TRY(ensure_sqnorm(ctx, data));
  if (!ctx->prepare_state_dev) {
    hipError_t e = dev_alloc(&ctx->prepare_state_dev, sizeof(PrepState));
    if (e != hipSuccess)
      return fail(RPT_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  }
  PrepState* st = static_cast<PrepState*>(ctx->prepare_state_dev);
  const int64_t n = data->n;
  const int na = pair_bucket(k);
  const int wave_bytes = (int)(((size_t)(k * kLS + 2 * k + na + 1) * 8 + (size_t)k * 4 + 7) & ~(size_t)7);
  if (4 * wave_bytes > kLdsMax) return fail(RPT_E_INTERNAL, "prepare: the neighbours' rows do not fit LDS");

  DevBuf<int32_t> kids, kcount, deg, cur, rsrc;
  DevBuf<double> kdist, rdist;
  DevBuf<int64_t> roff;
  if (diversify) {
    RPT_TRY(kids.alloc((size_t)n * k));
    RPT_TRY(kdist.alloc((size_t)n * k));
    RPT_TRY(kcount.alloc((size_t)n));
  }
  if (reverse) {
    RPT_TRY(deg.alloc((size_t)n));
    RPT_TRY(cur.alloc((size_t)n));
    RPT_TRY(roff.alloc((size_t)n + 1));
    RPT_TRY(rsrc.alloc((size_t)n * k));
    RPT_TRY(rdist.alloc((size_t)n * k));
  }
  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  hipLaunchKernelGGL(prep_begin_kernel, dim3(1), dim3(64), 0, ctx->stream, st);
  if (n > 0) {
    const int32_t* gi = ids_dev;
    const double* gd = dist_dev;
    const int32_t* gc = count_dev;
    if (diversify) {
      const DivArgs a{ctx, st, data, k, wave_bytes, ids_dev, count_dev, dist_dev, kids.p, kcount.p, kdist.p};
      switch (data->dtype) {
        case RPT_F64: RPT_TRY(launch_diversify_metric<double>(m, na, a)); break;
        case RPT_F32: RPT_TRY(launch_diversify_metric<float>(m, na, a)); break;
        default: RPT_TRY(launch_diversify_metric<uint16_t>(m, na, a));
      }
      gi = kids.p;
      gd = kdist.p;
      gc = kcount.p;
    }
    const int64_t cap = (int64_t)ctx->n_cu * 16;
    if (reverse) {
      const unsigned grid_n = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap));
      const unsigned grid_e = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n * k + 255) / 256, cap));
      hipLaunchKernelGGL(rev_zero_kernel, dim3(grid_n), dim3(256), 0, ctx->stream, &st->one, n, deg.p, cur.p);
      hipLaunchKernelGGL(rev_degree_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, &st->one, n, k, gi, gc, deg.p);
      hipLaunchKernelGGL(rev_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, &st->one, n, deg.p, roff.p);
      hipLaunchKernelGGL(rev_fill_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, &st->one, n, k, gi, gd, gc,
                         roff.p, cur.p, rsrc.p, rdist.p);
    }
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, cap));
    hipLaunchKernelGGL(prep_merge_kernel, dim3(grid), dim3(256), 0, ctx->stream, st, n, k, kout, gi, gd, gc,
                       reverse ? roff.p : nullptr, rsrc.p, rdist.p, out_ids_dev, out_dist_dev, out_count_dev);
  }
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

int32_t graph_prepare_last(rpt_ctx* ctx, int64_t* pairs, int64_t* occluded, int64_t* capped) {
  *pairs = *occluded = *capped = 0;
  if (!ctx->prepare_state_dev) return RPT_OK;  // no call yet
  RPT_HIP(stream_sync(ctx->stream));
  PrepState h;
  RPT_HIP(hipMemcpy(&h, ctx->prepare_state_dev, sizeof h, hipMemcpyDeviceToHost));
  *pairs = (int64_t)h.pairs;
  *occluded = (int64_t)h.occluded;
  *capped = (int64_t)h.capped;
  return RPT_OK;
}

}  // namespace rpt
