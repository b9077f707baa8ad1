// graph_prepare.hip — a kNN graph made ready for the search (rpt_graph_prepare_* on dense rows,
// rpt_graph_prepare_csr_* on SVector rows under L2, rpt_graph_prepare_csr_metric_* on SVector rows
// under cosine / inner product): occluded
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
//   graph_diversify_csr_kernel (DIVERSIFY, rpt_graph_prepare_csr_*: SVector rows under L2) the same
//                          frame: one wave per point, the compacted row, the pairs on the lanes, the
//                          ballots, the keep rule (div_row / div_keep / div_store below, one
//                          definition each).  Only the distance of a pair differs: a two-pointer merge
//                          over the two neighbours' (column, value) pairs (pair_fold), +0.0 for the
//                          absent side, which gives the bits of the dense fold over all d columns
//                          (graph_search_csr.hip has the argument).  Every neighbour row takes part in
//                          c - 1 pairs, so a point whose neighbours hold at most kResCap entries
//                          together has them packed into the wave's LDS first (resident: a wave prefix
//                          sum of the row lengths gives the offsets, the copy is coalesced row by row,
//                          values are widened once); any other point's lanes walk their two rows
//                          through global loads.  The choice is per point and wave-uniform, both paths
//                          fold the same entries in the same order.
//                          Under cosine / inner product (rpt_graph_prepare_csr_metric_*, M != kGraphL2)
//                          the distance of a pair comes from dotS (rptree_hip.h): a step folds only
//                          where both cursors stand on one column, and the walk ends with the shorter
//                          row.  Cosine takes the two neighbours' dotS(x, x) from a register of lane r
//                          (neighbour r) by two shuffles per pair: no LDS is added (kResCap below).
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

// ---- the frame of a diversify kernel, shared by graph_diversify_kernel (dense rows) and
// graph_diversify_csr_kernel (CSR rows).  All 64 lanes of the wave call these together.

// The entry of row i this lane looks at: false when it lies behind the clamped count or its id is no
// row.  The caller compacts the valid entries in stored order: sid/sd[0 .. cc), cc = popcount(vm).
__device__ __forceinline__ bool div_row(const int32_t* __restrict__ ids, const double* __restrict__ dist,
                                        const int32_t* __restrict__ count, int64_t i, int k, int64_t n,
                                        int lane, int& id, double& dv, unsigned long long& vm) {
  int c = count[i];
  c = c < 0 ? 0 : (c > k ? k : c);
  id = -1;
  dv = pos_inf();
  if (lane < c) {
    id = ids[i * k + lane];
    dv = dist[i * k + lane];
  }
  const bool ok = lane < c && (unsigned)id < (unsigned long long)n;
  vm = __ballot(ok);
  return ok;
}

// The serial keep rule.  bal: the occlusion bits of the pairs in pair order (bit p: e_l occludes
// e_m, p = m (m - 1) / 2 + l), one word more than the pairs fill.  The pairs of an m are consecutive,
// so lane m cuts its word of m bits out of them, and c - 1 wave-uniform steps walk the row: e_m stays
// unless a kept e_l occludes it.  -> the kept entries as a mask.
__device__ __forceinline__ unsigned long long div_keep(const unsigned long long* bal, int cc, int lane) {
  unsigned long long kept = 1ULL;
  unsigned long long mine = 0;  // lane m: bit l of `mine` = e_l occludes e_m
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
  return kept;
}

// Kept(i) compacted into row i of the scratch graph, the rest of the row padded.  -> |Kept(i)|
__device__ __forceinline__ int div_store(unsigned long long kept, int cc, const int* sid, const double* sd,
                                         int64_t i, int k, int lane, int32_t* __restrict__ kids,
                                         double* __restrict__ kdist, int32_t* __restrict__ kcount) {
  const int kc = __popcll(kept);
  if (lane < cc && ((kept >> lane) & 1)) {
    const int pos = __popcll(kept & ((1ULL << lane) - 1));
    kids[i * k + pos] = sid[lane];
    kdist[i * k + pos] = sd[lane];
  }
  if (lane >= kc && lane < k) {
    kids[i * k + lane] = -1;
    kdist[i * k + lane] = pos_inf();
  }
  if (lane == 0) kcount[i] = kc;
  return kc;
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
    int id;
    double dv;
    unsigned long long vm;
    const bool ok = div_row(ids, dist, count, i, k, n, lane, id, dv, vm);
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
      kept = div_keep(bal, cc, lane);
    }
    const int kc = div_store(kept, cc, sid, sd, i, k, lane, kids, kdist, kcount);
    n_pairs += (unsigned long long)P;
    n_occ += (unsigned long long)(cc - kc);
  }
  if (lane == 0 && (n_pairs | n_occ)) {
    atomicAdd(&st->pairs, n_pairs);
    atomicAdd(&st->occluded, n_occ);
  }
}

// ---- DIVERSIFY on SVector (CSR) rows ------------------------------------------------------------
constexpr int kNoCol = 0x7fffffff;  // a cursor at its row's end (a column is below d <= INT_MAX)
// Entries of a point's neighbours up to which they are staged in LDS, 12 B each (an int column, the
// value widened to double).  Two workgroups per CU get 80 KB each of the 160 KB, a wave 20 480 B.
// What a wave holds besides the entries is largest at k = 64: ids, stored distances, row lengths,
// row positions and 33 ballot words, 1 800 B.  That leaves 18 680 B = 1 556 entries; 1 536 = 3 x 512
// is the round number below, and a workgroup then takes 80 928 B at k = 64 (less for a smaller k:
// 74 752 B at k = 10).  The C3 point (k = 10, rows of 784 x 0.19 = 149 entries: 1 490 +- 35 per point
// if the neighbours were average rows) lies below the cap; measured there, neighbours are short
// rows, 1 245 entries per point on average and 1 404 at the most.
// Cosine needs dot(x, x) of the two neighbours of every pair.  k more doubles per wave would make the
// workgroup 80 928 + 4 x 512 = 82 976 B at k = 64, above the 81 920 B that two workgroups per CU may
// take each, and halve the occupancy.  So the norms stay out of LDS: lane r holds neighbour r's in a
// register and a pair fetches its two with __shfl.  The cosine kernel's workgroup is the L2 kernel's:
// 4 x ((1 536 + 2 x 64 + 33) x 8 + (1 536 + 2 x 64) x 4) = 4 x 20 232 = 80 928 B at k = 64.
constexpr int kResCap = 1536;

// where the rows of a pair are read: the entries staged in the wave's LDS, or the data set.
// kReadBoth: pair_fold reads the entries under both cursors in every step (below).
struct LdsRows {
  static constexpr bool kReadBoth = true;
  const int* c;
  const double* v;
  __device__ __forceinline__ int col(int p) const { return c[p]; }
  __device__ __forceinline__ double val(int p) const { return v[p]; }
};
template <class TV>
struct GlobalRows {
  static constexpr bool kReadBoth = false;
  const int32_t* __restrict__ c;
  const TV* __restrict__ v;
  __device__ __forceinline__ int col(int64_t p) const { return c[p]; }
  __device__ __forceinline__ double val(int64_t p) const { return widen(v[p]); }
};

// The L2 accumulator of the rows [ap, ae) and [bp, be): a two-pointer merge, the steps of merge_piece
// in graph_search_csr.hip.  Every step takes the entry of one side or of both (equal columns), the
// absent side is +0.0, and the tail of the longer row is folded the same way: a cursor at its row's
// end counts as column kNoCol.  A cursor is read only below its row's end and every step advances
// one, also for rows whose columns do not ascend.  The steps, and so the bits, do not depend on how
// the entries are fetched, which is chosen by what is cheap where they lie (C3, k = 10, ms of the
// whole DIVERSIFY call, both ways measured on both paths):
//   LDS     the entries under both cursors are read together at the top of every step, one round trip
//           a step instead of one per side that moved (17.2 against 24.8 ms); a finished cursor reads
//           entry 0, which exists whenever the loop runs, and its value is not used
//   global  the entries are carried in registers and only a side that moved loads its next one (32.8
//           against 44.0 ms: reading both every step doubles the loads)
// Cosine / inner product (M != kGraphL2): dotS of the two rows.  The same steps, but only a step
// that takes both sides folds, and the loop runs while both cursors are live: no tail, no entry 0 read
// for a finished cursor.
template <int M, class R, class I>
__device__ __forceinline__ double pair_fold(const R& r, I ap, I ae, I bp, I be) {
  double acc = 0.0;
  if constexpr (M != kGraphL2 && R::kReadBoth) {
    while (ap < ae && bp < be) {
      const int ca = r.col(ap), cb = r.col(bp);
      const double va = r.val(ap), vb = r.val(bp);
      const bool take_a = ca <= cb, take_b = cb <= ca;
      if (take_a && take_b) acc = fold_step<M>(acc, va, vb);
      ap += take_a ? 1 : 0;
      bp += take_b ? 1 : 0;
    }
  } else if constexpr (M != kGraphL2) {
    int ca = kNoCol, cb = kNoCol;
    double va = 0.0, vb = 0.0;
    if (ap < ae) {
      ca = r.col(ap);
      va = r.val(ap);
    }
    if (bp < be) {
      cb = r.col(bp);
      vb = r.val(bp);
    }
    while (ap < ae && bp < be) {
      const bool take_a = ca <= cb, take_b = cb <= ca;
      if (take_a && take_b) acc = fold_step<M>(acc, va, vb);
      if (take_a) {
        ++ap;
        if (ap < ae) {
          ca = r.col(ap);
          va = r.val(ap);
        }
      }
      if (take_b) {
        ++bp;
        if (bp < be) {
          cb = r.col(bp);
          vb = r.val(bp);
        }
      }
    }
  } else if constexpr (R::kReadBoth) {
    while (ap < ae || bp < be) {
      const bool ha = ap < ae, hb = bp < be;
      const I ia = ha ? ap : (I)0, ib = hb ? bp : (I)0;
      const int la = r.col(ia), lb = r.col(ib);
      const double va = r.val(ia), vb = r.val(ib);
      const int ca = ha ? la : kNoCol, cb = hb ? lb : kNoCol;
      const bool take_a = ca <= cb, take_b = cb <= ca;
      acc = fold_step<kGraphL2>(acc, take_a ? va : 0.0, take_b ? vb : 0.0);
      ap += take_a ? 1 : 0;
      bp += take_b ? 1 : 0;
    }
  } else {
    int ca = kNoCol, cb = kNoCol;
    double va = 0.0, vb = 0.0;
    if (ap < ae) {
      ca = r.col(ap);
      va = r.val(ap);
    }
    if (bp < be) {
      cb = r.col(bp);
      vb = r.val(bp);
    }
    while (ap < ae || bp < be) {
      const bool take_a = ca <= cb, take_b = cb <= ca;
      acc = fold_step<kGraphL2>(acc, take_a ? va : 0.0, take_b ? vb : 0.0);
      if (take_a) {
        ++ap;
        ca = kNoCol;
        if (ap < ae) {
          ca = r.col(ap);
          va = r.val(ap);
        }
      }
      if (take_b) {
        ++bp;
        cb = kNoCol;
        if (bp < be) {
          cb = r.col(bp);
          vb = r.val(bp);
        }
      }
    }
  }
  return acc;
}

// dynamic LDS, per wave (wave_bytes): cap doubles (staged values), k doubles (stored distances), k
// 64-bit row positions (into the staged entries when the point is resident, else into col / val),
// NA + 1 words (the ballots), cap ints (staged columns), k ints (ids), k ints (row lengths).
// rn: dot(x, x) of the data rows (cosine; kept in registers, not in LDS)
template <class TV, int M, int NA>
__global__ __launch_bounds__(256) void graph_diversify_csr_kernel(
    PrepState* st, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const TV* __restrict__ val, int64_t n, int k, int cap, int wave_bytes,
    const int32_t* __restrict__ ids, const double* __restrict__ dist,
    const int32_t* __restrict__ count, int32_t* __restrict__ kids, double* __restrict__ kdist,
    int32_t* __restrict__ kcount, const double* __restrict__ rn) {
  extern __shared__ double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  double* ev = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * wave_bytes);
  double* sd = ev + cap;
  long long* pos = reinterpret_cast<long long*>(sd + k);
  unsigned long long* bal = reinterpret_cast<unsigned long long*>(pos + k);
  int* ec = reinterpret_cast<int*>(bal + NA + 1);
  int* sid = ec + cap;
  int* rl = sid + k;
  const unsigned long long below = (1ULL << lane) - 1;
  unsigned long long n_pairs = 0, n_occ = 0;

  for (int64_t i = (int64_t)blockIdx.x * W + wave; i < n; i += (int64_t)gridDim.x * W) {
    int id;
    double dv;
    unsigned long long vm;
    const bool ok = div_row(ids, dist, count, i, k, n, lane, id, dv, vm);
    const int cc = __popcll(vm);
    wave_sync();  // the last point's rows have been read
    if (ok) {
      const int at = __popcll(vm & below);
      sid[at] = id;
      sd[at] = dv;
    }
    wave_sync();
    const int P = cc * (cc - 1) / 2;

    unsigned long long kept = cc > 0 ? 1ULL : 0ULL;
    if (P > 0) {
      // lane r < cc: the r-th neighbour's row; a wave prefix sum of the lengths (each clamped to
      // cap + 1, so that the sum fits an int) places the rows in the staged entries
      long long rb = 0;
      int len = 0;
      double nrm = 0.0;  // lane r: dot(x, x) of the r-th neighbour (cosine)
      if (lane < cc) {
        const int v = sid[lane];
        if constexpr (M == kGraphCosine) nrm = rn[v];
        rb = rowptr[v];
        const long long l64 = rowptr[v + 1] - rb;
        len = l64 < 0 ? 0 : (l64 > (long long)kNoCol ? kNoCol : (int)l64);
      }
      const int lc = len > cap ? cap + 1 : len;
      int incl = lc;
      for (int s = 1; s < 64; s <<= 1) {
        const int t = __shfl_up(incl, s);
        if (lane >= s) incl += t;
      }
      const int total = __shfl(incl, 63);
      const bool resident = total <= cap;  // wave-uniform; cap = 0: no point that has an entry to stage
      const int off = incl - lc;
      if (lane < cc) {
        pos[lane] = resident ? (long long)off : rb;
        rl[lane] = len;
      }
      if (resident) {
        for (int r = 0; r < cc; ++r) {  // row by row: consecutive lanes, consecutive entries
          const long long b = __shfl(rb, r);
          const int L = __shfl(len, r), o = __shfl(off, r);
          for (int p = lane; p < L; p += 64) {
            ec[o + p] = col[b + p];
            ev[o + p] = widen(val[b + p]);
          }
        }
      }
      wave_sync();
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int p = lane + 64 * a;
        int l = 0, m = 0;
        double acc = 0.0;
        if (p < P) {
          pair_of(p, l, m);
          if (resident) {
            const int pa = (int)pos[l], pb = (int)pos[m];
            acc = pair_fold<M>(LdsRows{ec, ev}, pa, pa + rl[l], pb, pb + rl[m]);
          } else {
            const long long pa = pos[l], pb = pos[m];
            acc = pair_fold<M>(GlobalRows<TV>{col, val}, pa, pa + rl[l], pb, pb + rl[m]);
          }
        }
        double n_l = 0.0, n_m = 0.0;
        if constexpr (M == kGraphCosine) {  // by all 64 lanes; a pair behind P asks for lane 0 twice
          n_l = __shfl(nrm, l);
          n_m = __shfl(nrm, m);
        }
        const bool occ = p < P && fold_finish<M>(acc, n_l, n_m) < sd[m];
        const unsigned long long b = __ballot(occ);
        if (lane == 0) bal[a] = b;
      }
      if (lane == 0) bal[NA] = 0;
      wave_sync();
      kept = div_keep(bal, cc, lane);
    }
    const int kc = div_store(kept, cc, sid, sd, i, k, lane, kids, kdist, kcount);
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
  int cap;  // CSR rows: entries of a point's neighbours that are staged in LDS (0: no point is resident)
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

template <class TV, int M, int NA>
int32_t launch_diversify_csr(const DivArgs& a) {
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(a.ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)graph_diversify_csr_kernel<TV, M, NA>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  constexpr int W = 4;
  const int64_t want = (a.data->n + W - 1) / W;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)a.ctx->n_cu * 16));
  hipLaunchKernelGGL((graph_diversify_csr_kernel<TV, M, NA>), dim3(grid), dim3(64 * W), (size_t)a.wave_bytes * W,
                     a.ctx->stream, a.st, a.data->rowptr, a.data->col, static_cast<const TV*>(a.data->val),
                     a.data->n, a.k, a.cap, a.wave_bytes, a.ids, a.dist, a.count, a.kids, a.kdist, a.kcount,
                     M == kGraphCosine ? a.data->sqnorm : nullptr);
  return RPT_OK;
}

// the distance of a launch: the kernel is instantiated per value type, metric and accumulator count
template <class TV, int NA>
int32_t launch_diversify_csr_metric(int m, const DivArgs& a) {
  if (m == kGraphCosine) return launch_diversify_csr<TV, kGraphCosine, NA>(a);
  if (m == kGraphInner) return launch_diversify_csr<TV, kGraphInner, NA>(a);
  return launch_diversify_csr<TV, kGraphL2, NA>(a);
}

template <class TV>
int32_t launch_diversify_csr_na(int m, int na, const DivArgs& a) {
  switch (na) {
    case 1: return launch_diversify_csr_metric<TV, 1>(m, a);
    case 2: return launch_diversify_csr_metric<TV, 2>(m, a);
    case 4: return launch_diversify_csr_metric<TV, 4>(m, a);
    case 8: return launch_diversify_csr_metric<TV, 8>(m, a);
    case 16: return launch_diversify_csr_metric<TV, 16>(m, a);
    default: return launch_diversify_csr_metric<TV, 32>(m, a);
  }
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
  int wave_bytes, cap = 0;
  if (data->csr) {
    // graph_prepare_csr_resident: 0 the built-in cap, n > 0 a smaller one, -1 no point resident.  Rows
    // of ascending columns hold at most d entries each: no more LDS than k of them can fill.
    const int64_t opt = ctx->opt.graph_prepare_csr_resident;
    const int64_t want = opt < 0 ? 0 : (opt == 0 ? kResCap : std::min<int64_t>(opt, kResCap));
    cap = (int)std::min<int64_t>(want, (int64_t)k * data->d);
    wave_bytes = (int)(((size_t)(cap + 2 * k + na + 1) * 8 + (size_t)(cap + 2 * k) * 4 + 7) & ~(size_t)7);
  } else {
    wave_bytes = (int)(((size_t)(k * kLS + 2 * k + na + 1) * 8 + (size_t)k * 4 + 7) & ~(size_t)7);
  }
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
      const DivArgs a{ctx, st, data, k, wave_bytes, cap, ids_dev, count_dev, dist_dev, kids.p, kcount.p, kdist.p};
      if (data->csr) {
        if (data->dtype == RPT_F64) RPT_TRY(launch_diversify_csr_na<double>(m, na, a));
        else RPT_TRY(launch_diversify_csr_na<float>(m, na, a));
      } else {
        switch (data->dtype) {
          case RPT_F64: RPT_TRY(launch_diversify_metric<double>(m, na, a)); break;
          case RPT_F32: RPT_TRY(launch_diversify_metric<float>(m, na, a)); break;
          default: RPT_TRY(launch_diversify_metric<uint16_t>(m, na, a));
        }
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
