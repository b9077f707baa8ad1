// graph_dev.h — device helpers shared by graph.hip (the graph, leaf by leaf), graph_refine.hip
// (its NN-descent rounds) and graph_search.hip (the beam search over it): the chunk geometry, the
// (distance, id) total order, the exact widening of f32 / bf16 elements, the metric's fold step
// and epilogue, the one-wave insertion into a sorted list, the one-wave staging of a chunk of
// rows, the CSR of a graph's reverse edges (graph_prepare.hip takes these too) and the beam of the
// search: its offers, its visited filter and its insertion, which graph_search.hip (dense rows) and
// graph_search_csr.hip (CSR rows) run around their own distance step.  The translation units are
// built with -ffp-contract=off.
#pragma once

#include <algorithm>

#include "common.h"

namespace rpt {
namespace {

constexpr int kCW = 32;         // columns of a staged chunk
constexpr int kLS = kCW + 1;    // its row stride in LDS, doubles (odd: no bank conflicts down a column)

// The distance the kernels are instantiated on.  L2: acc + (a - b)^2, then sqrt.  Cosine / inner
// product (rpt_knn_graph_metric_*): the left-fold dot acc + a * b (two rounded operations per
// element instead of three), then 1 - acc / (sqrt(n_i) * sqrt(n_j)) with the rows' cached
// dot(x, x) (rpt_dataset::sqnorm, the same fold) / -acc.  IEEE multiplication commutes and the
// columns ascend for both rows of a pair, so all three are symmetric bit for bit.
constexpr int kGraphL2 = 0, kGraphCosine = 1, kGraphInner = 2;

template <int M>
__device__ __forceinline__ double fold_step(double acc, double a, double b) {
  if constexpr (M == kGraphL2) {
    const double t = a - b;
    const double sq = t * t;
    return acc + sq;
  } else {
    const double pr = a * b;
    return acc + pr;
  }
}

// ni, nj: dot(x, x) of the two rows (cosine only)
template <int M>
__device__ __forceinline__ double fold_finish(double acc, double ni, double nj) {
  if constexpr (M == kGraphL2) return sqrt(acc);
  else if constexpr (M == kGraphInner) return -acc;
  else return 1.0 - acc / (sqrt(ni) * sqrt(nj));
}

// RPT_KNN_METRIC_COSINE / _INNER / 0 of the C ABI -> kGraph*
inline int graph_metric_of(int32_t metric) {
  return metric == RPT_KNN_METRIC_COSINE ? kGraphCosine : metric == RPT_KNN_METRIC_INNER ? kGraphInner : kGraphL2;
}

// the total order of the answer: numbers by (distance, id), then NaN distances by id
__device__ inline bool before(double da, int ia, double db, int ib) {
  const bool an = da != da, bn = db != db;
  if (an || bn) return an == bn ? ia < ib : bn;
  return da < db || (da == db && ia < ib);
}

__device__ inline double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// elements widen exactly; bf16 rows arrive as their bit patterns
__device__ inline double widen(double v) { return v; }
__device__ inline double widen(float v) { return (double)v; }
__device__ inline double widen(uint16_t v) { return (double)__uint_as_float((uint32_t)v << 16); }

template <class TD>
__device__ inline void widen16(const uint4& v, double* out);
template <>
__device__ inline void widen16<double>(const uint4& v, double* out) {
  out[0] = __longlong_as_double(((long long)v.y << 32) | v.x);
  out[1] = __longlong_as_double(((long long)v.w << 32) | v.z);
}
template <>
__device__ inline void widen16<float>(const uint4& v, double* out) {
  out[0] = (double)__uint_as_float(v.x);
  out[1] = (double)__uint_as_float(v.y);
  out[2] = (double)__uint_as_float(v.z);
  out[3] = (double)__uint_as_float(v.w);
}
template <>
__device__ inline void widen16<uint16_t>(const uint4& v, double* out) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    out[2 * i] = (double)__uint_as_float(w[i] << 16);
    out[2 * i + 1] = (double)__uint_as_float(w[i] & 0xffff0000u);
  }
}

// One wave merges up to two candidates per lane into a sorted list held one entry per lane
// (lanes [0, c) valid, c <= k <= 64).  Returns whether the list changed.
__device__ inline bool wave_merge(double& ld, int& lid, int& c, int k, double cd0, int ci0, bool v0,
                                  double cd1, int ci1, bool v1) {
  const int lane = threadIdx.x & 63;
  bool changed = false;
  for (;;) {
    if (c == k) {  // a full list: only what comes before its last entry can enter
      const double td = __shfl(ld, k - 1);
      const int ti = __shfl(lid, k - 1);
      v0 = v0 && before(cd0, ci0, td, ti);
      v1 = v1 && before(cd1, ci1, td, ti);
    }
    const unsigned long long m0 = __ballot(v0), m1 = __ballot(v1);
    if (!(m0 | m1)) break;
    const bool first = m0 != 0;
    const int src = __ffsll((long long)(first ? m0 : m1)) - 1;
    const double nd = __shfl(first ? cd0 : cd1, src);
    const int ni = __shfl(first ? ci0 : ci1, src);
    if (lane == src) {
      if (first) v0 = false;
      else v1 = false;
    }
    if (__ballot(lane < c && lid == ni)) continue;  // the same point, found by an earlier tree
    const int p = __popcll(__ballot(lane < c && before(ld, lid, nd, ni)));
    const double ud = __shfl_up(ld, 1);
    const int ui = __shfl_up(lid, 1);
    if (lane > p) {
      ld = ud;
      lid = ui;
    } else if (lane == p) {
      ld = nd;
      lid = ni;
    }
    if (c < k) ++c;
    changed = true;
  }
  return changed;
}

__device__ inline void wave_sync() {  // LDS writes of the wave visible to all its lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one wave: columns [c0, c0 + cw) of the rows sid[0 .. nrows) as doubles into buf[r * kLS + c],
// graph.hip's stage_chunk with a wave in place of the workgroup; four loads in flight per lane
template <class TD>
__device__ inline void wave_stage(const TD* __restrict__ X, int d, const int* sid, int nrows, int c0,
                                  int cw, double* buf, bool vec) {
  const int lane = threadIdx.x & 63;
  if (vec) {
    constexpr int E = 16 / (int)sizeof(TD);
    const int ppr = cw / E, total = nrows * ppr;
    for (int p0 = 0; p0 < total; p0 += 256) {
      uint4 v[4];
      int at[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * 64 + lane;
        at[u] = -1;
        if (p < total) {
          const int r = p / ppr, q = p - r * ppr;
          at[u] = r * kLS + q * E;
          v[u] = *reinterpret_cast<const uint4*>(X + (size_t)sid[r] * d + c0 + q * E);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (at[u] >= 0) {
          double w[E];
          widen16<TD>(v[u], w);
#pragma unroll
          for (int e = 0; e < E; ++e) buf[at[u] + e] = w[e];
        }
    }
  } else {
    for (int p = lane; p < nrows * cw; p += 64) {
      const int r = p / cw, c = p - r * cw;
      buf[r * kLS + c] = widen(X[(size_t)sid[r] * d + c0 + c]);
    }
  }
}

// ---- the beam of the graph search, shared by graph_search_kernel (graph_search.hip) and
// graph_search_csr_kernel (graph_search_csr.hip).  One wave owns a query; per wave in LDS:
//   bd/bi ef doubles / ints  the beam, sorted; bi holds id (unexpanded) or ~id (expanded)
//   tab   H ints             the visited filter: a hash of evaluated ids, kProbe slots per id, a
//                            full neighbourhood is overwritten (lossy)
//   sid   R ints             the ids of the running offer that are evaluated
// All 64 lanes of the wave call every function below together.
//
// The allow-list searches (rpt_graph_search_allow_*: graph_search_allow_kernel,
// graph_search_csr_allow_kernel) run the same functions with the compile-time switch F on.  Then
// the beam holds up to `width` entries (bd/bi of ceil(width / 64) * 64), a third array
//   ba    bytes, as many      1 where the entry's id is in the allow-list; ids use all 31 bits and
//                            ~id marks an expanded entry, so bi has no bit to spare
// stands beside them, `na` counts the allowed entries, and the beam is cut(everything offered) of
// include/rptree_hip.h: it ends at its ef-th allowed entry or at its width-th entry, whichever
// comes first.  With F off none of this is compiled and the functions are what they were.  J is
// the number of beam entries a lane looks after in beam_insert (ceil(width / 64) <= J).
constexpr int kEmpty = (int)0x80000000;  // free slot of a hash of ids in LDS (never an id): the
                                         // search's filter, the refinement's candidate set
constexpr int kProbe = 8;                // slots of the filter an id may take
constexpr int kBeamJ = RPT_GRAPH_SEARCH_MAX_EF / 64;  // beam entries a lane looks after
constexpr int kBeamJWide = RPT_GRAPH_SEARCH_MAX_WIDTH / 64;  // ... of an allow-list beam beyond 256

struct SearchState {
  unsigned long long expansions, evaluated;
};

struct SearchArgs {
  int64_t n, nq;
  int d, kg, s, k, ef;
  int R, H, qres, vec, nofilter, wave_bytes;
  int qcap, stream;  // CSR rows: entries of a query that stay in LDS, 1 = every query is streamed
  int width;         // entries the beam may hold, allowed or not (without an allow-list: ef)
  const int32_t* gids;
  const int32_t* gcount;
  const int32_t* seeds;
  AllowGroups allow;  // the allow-list: bit i & 31 of word i >> 5 of the query's row (F only); the group
                      // array and the row stride of rpt_graph_search_allow_group_*, or one bitmap
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

// What every search sizes the same way.  An offer holds a graph row whole and seeds come in batches
// of the same size; the filter has eight slots per beam entry, 1 to 8 KB.
inline void search_shape(SearchArgs& a) {
  a.R = std::max<int>(a.kg, std::min<int>(a.s, 16));
  a.H = 256;
  while (a.H < 8 * a.width && a.H < 2048) a.H <<= 1;
}

// Waves per workgroup of an allow-list search, which never refuses a shape: of 4, 2 and 1 the count
// that keeps the most waves on a CU, floor(lds / (W * wave_bytes)) workgroups of W waves each, the
// larger count on a tie.  One wave always fits (wave_bytes stays below 64 KB by the entry points'
// limits on kg, width and the resident query).
inline int search_waves(int wave_bytes, int lds) {
  int best = 1, waves = 0;
  for (int W = 4; W >= 1; W >>= 1) {
    const int r = (lds / (W * wave_bytes)) * W;
    if (r > waves) {
      waves = r;
      best = W;
    }
  }
  return best;
}

__device__ inline int beam_id(int v) { return v < 0 ? ~v : v; }

// The allow-list of the wave's query, resolved once before the seeds: `bits` is the query's bitmap
// (null: every id), `none` says that no id is allowed (a group value outside [-1, G)).  group[qi] is
// wave-uniform, so the row pointer is made from a scalar.
struct BeamAllow {
  const uint32_t* bits;
  bool none;
};

__device__ __forceinline__ BeamAllow beam_allow_of(const SearchArgs& a, int64_t qi) {
  BeamAllow r = {a.allow.bits, false};
  if (a.allow.group) {
    const int g = __builtin_amdgcn_readfirstlane(a.allow.group[qi]);
    r.bits = nullptr;
    if (g >= 0 && g < a.allow.G) r.bits = a.allow.bits + (int64_t)g * a.allow.stride;
    else r.none = g != -1;
  }
  return r;
}

// whether id v (in [0, n), or -1 on an idle lane) is in the allow-list: one 32-bit load
__device__ inline bool beam_allowed(const BeamAllow& w, int v) {
  if (v < 0 || w.none) return false;
  return w.bits == nullptr || ((w.bits[v >> 5] >> (v & 31)) & 1u) != 0;
}

// The next offer, a candidate per lane (-1: none): a batch of R seeds, then the graph row of the
// first unexpanded entry, which is marked expanded.  false: no unexpanded entry is left, the search
// is over.  The caller bounds the loop: once the seeds are through, at most n expansions.
__device__ __forceinline__ bool beam_next_offer(const SearchArgs& a, int64_t qi, int* bi, int c, int nj,
                                                int lane, int& s0, int64_t& expanded, int& cand) {
  cand = -1;
  if (s0 < a.s) {
    if (lane < a.R && s0 + lane < a.s) cand = a.seeds[qi * a.s + s0 + lane];
    s0 += a.R;
    return true;
  }
  int pos = -1;
  for (int j = 0; j < nj && pos < 0; ++j) {
    const int p = j * 64 + lane;
    const unsigned long long bal = __ballot(p < c && bi[p] >= 0);
    if (bal) pos = j * 64 + __ffsll((long long)bal) - 1;
  }
  if (pos < 0) return false;
  const int u = __builtin_amdgcn_readfirstlane(bi[pos]);
  wave_sync();
  if (lane == 0) bi[pos] = ~u;
  wave_sync();
  ++expanded;
  const int g = a.gcount[u];
  if (g >= 0 && g <= a.kg && lane < g) cand = a.gids[(int64_t)u * a.kg + lane];
  return true;
}

// Drops what is outside [0, n), what the filter remembers and what the beam holds; the rest is
// remembered by the filter and compacted into sid[0 .. nrows).  Returns nrows.
__device__ __forceinline__ int beam_admit(const SearchArgs& a, const int* bi, int c, int* tab, int* sid,
                                          bool filter, int lane, int cand) {
  const int mask = a.H - 1, shift = 32 - (31 - __clz(a.H));
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
  if (nrows == 0) return 0;
  if (filter && v) {
    bool done = false;
    for (int pr = 0; pr < kProbe && !done; ++pr) {
      const int old = atomicCAS(&tab[(h + pr) & (unsigned)mask], kEmpty, cand);
      done = old == kEmpty || old == cand;
    }
    if (!done) tab[h] = cand;  // a full neighbourhood: forget whoever sat at home
  }
  if (v) sid[__popcll(bal & ((1ULL << lane) - 1))] = cand;
  wave_sync();
  return nrows;
}

// The offer's entries (cd, my) of the lanes [0, nrows) into the beam of c entries, one at a time:
// rank by ballot / popcount over the lanes' entries (lane l looks at positions l, l + 64, ...), the
// tail shifted by one in LDS.
// F: al says whether `my` is allowed, ba / na are the beam's allowed bits and their count.  The beam
// is full when it holds ef allowed entries or `width` entries; either way its last entry is the
// threshold.  An insertion makes it min(c + 1, width) entries, and when an allowed entry came in and
// ef or more are allowed now, the beam ends at its ef-th allowed entry, found by ballot / popcount
// over the blocks of 64 positions: the old last entry and every disallowed one between it and the new
// ef-th go in one step.
template <bool F = false, int J = kBeamJ>
__device__ __forceinline__ void beam_insert(double* bd, int* bi, int& c, int ef, int nj, int lane, int nrows,
                                            double cd, int my, unsigned char* ba = nullptr, int width = 0,
                                            int* na_ = nullptr, bool al = false) {
  bool v = lane < nrows;
  const int cap = F ? width : ef;
  int na = 0;
  if constexpr (F) na = *na_;
  for (;;) {
    int gone = 0;  // F: the allowed bit of the entry a beam of `width` entries is about to lose
    if (F ? (na == ef || c == cap) : c == ef) {  // a full beam: only what comes before its last entry can enter
      const double td = bd[c - 1];
      const int ti = beam_id(bi[c - 1]);
      v = v && before(cd, my, td, ti);
      if constexpr (F) gone = c == cap ? (int)ba[c - 1] : 0;
    }
    const unsigned long long m = __ballot(v);
    if (!m) break;
    const int src = __ffsll((long long)m) - 1;
    const double nd = __shfl(cd, src);
    const int ni = __shfl(my, src);
    int nal = 0;
    if constexpr (F) nal = __shfl((int)al, src);
    if (lane == src) v = false;
    double ed[J];
    int ei[J];
    unsigned char ea[F ? J : 1];
    int p = 0;
    bool dup = false;
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (j < nj) {
        const int pos = j * 64 + lane;
        const bool on = pos < c;
        ed[j] = on ? bd[pos] : 0.0;
        ei[j] = on ? bi[pos] : kEmpty;
        if constexpr (F) ea[j] = on ? ba[pos] : (unsigned char)0;
        dup |= on && beam_id(ei[j]) == ni;
        p += __popcll(__ballot(on && before(ed[j], beam_id(ei[j]), nd, ni)));
      }
    if (__ballot(dup)) continue;  // the same id twice in one offer
    const int newc = c < cap ? c + 1 : c;
    wave_sync();  // every entry has been read
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (j < nj) {
        const int pos = j * 64 + lane;
        if (pos >= p && pos < c && pos + 1 < newc) {
          bd[pos + 1] = ed[j];
          bi[pos + 1] = ei[j];
          if constexpr (F) ba[pos + 1] = ea[j];
        }
      }
    if (lane == 0) {
      bd[p] = nd;
      bi[p] = ni;
      if constexpr (F) ba[p] = (unsigned char)nal;
    }
    wave_sync();
    c = newc;
    if constexpr (F) {
      na += nal - gone;
      if (nal && na >= ef) {  // the beam ends at its ef-th allowed entry
        int seen = 0;
        for (int j = 0; j < nj; ++j) {
          const int pos = j * 64 + lane;
          const unsigned long long am = __ballot(pos < c && ba[pos] != 0);
          const int cnt = __popcll(am);
          if (seen + cnt >= ef) {
            // the lane that holds the (ef - seen)-th set bit of am
            const bool hit = ((am >> lane) & 1ULL) && __popcll(am & ((2ULL << lane) - 1)) == ef - seen;
            c = j * 64 + __ffsll((long long)__ballot(hit));
            break;
          }
          seen += cnt;
        }
        na = ef;
      }
    }
  }
  if constexpr (F) *na_ = na;
}

// the answer of query qi: the first k of the beam, padded with id -1 and distance +inf
// F: the first k ALLOWED entries, compacted by ballot prefix over the blocks of 64 positions
template <bool F = false>
__device__ __forceinline__ void beam_answer(const SearchArgs& a, int64_t qi, const double* bd, const int* bi,
                                            int c, int lane, const unsigned char* ba = nullptr, int na = 0) {
  if constexpr (F) {
    const int found = na < a.k ? na : a.k;
    int seen = 0;
    for (int j = 0; j * 64 < c && seen < found; ++j) {
      const int pos = j * 64 + lane;
      const bool on = pos < c && ba[pos] != 0;
      const unsigned long long am = __ballot(on);
      const int r = seen + __popcll(am & ((1ULL << lane) - 1));
      if (on && r < found) {
        a.ids[qi * a.k + r] = beam_id(bi[pos]);
        a.dist[qi * a.k + r] = bd[pos];
      }
      seen += __popcll(am);
    }
    if (lane >= found && lane < a.k) {
      a.ids[qi * a.k + lane] = -1;
      a.dist[qi * a.k + lane] = pos_inf();
    }
    if (lane == 0) a.count[qi] = found;
    return;
  }
  const int found = c < a.k ? c : a.k;
  if (lane < a.k) {
    const bool on = lane < found;
    a.ids[qi * a.k + lane] = on ? beam_id(bi[lane]) : -1;
    a.dist[qi * a.k + lane] = on ? bd[lane] : pos_inf();
  }
  if (lane == 0) a.count[qi] = found;
}

// ---- the reverse edges of a graph as a CSR, shared by the refinement (graph_refine.hip, per round)
// and the preparation (graph_prepare.hip): zero, in-degrees (vector atomics), an exclusive scan by one
// workgroup, fill.  The position inside a target's segment comes from an atomic cursor, so the ORDER
// of a segment depends on arrival; both readers take a set or the first entries under a total order
// from it, so their answers do not.  `active`: a device-side flag, 0 = return at once.
constexpr int kScanThreads = 1024;

__global__ void rev_zero_kernel(const int32_t* active, int64_t n, int32_t* __restrict__ deg,
                                   int32_t* __restrict__ cur) {
  if (!*active) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    deg[i] = 0;
    cur[i] = 0;
  }
}

// edge e = (row j, slot s) of the graph: valid when s < count[j] and its target is a row
__device__ inline bool edge_of(int64_t e, int64_t n, int k, const int32_t* ids, const int32_t* count,
                               int64_t& j, int& t) {
  j = e / k;
  const int s = (int)(e - j * k);
  if (s >= count[j]) return false;
  t = ids[e];
  return (unsigned)t < (unsigned long long)n;
}

__global__ void rev_degree_kernel(const int32_t* active, int64_t n, int k,
                                     const int32_t* __restrict__ ids,
                                     const int32_t* __restrict__ count, int32_t* deg) {
  if (!*active) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * k; e += stride) {
    int64_t j;
    int t;
    if (edge_of(e, n, k, ids, count, j, t)) atomicAdd(&deg[t], 1);
  }
}

// off[0 .. n] = exclusive scan of deg[0 .. n): one workgroup, a contiguous run of rows per thread
__global__ __launch_bounds__(kScanThreads) void rev_scan_kernel(const int32_t* active, int64_t n,
                                                                   const int32_t* __restrict__ deg,
                                                                   int64_t* __restrict__ off) {
  if (!*active) return;
  __shared__ int64_t part[kScanThreads];
  const int tid = threadIdx.x;
  const int64_t per = (n + kScanThreads - 1) / kScanThreads;
  const int64_t lo = std::min<int64_t>(n, per * tid), hi = std::min<int64_t>(n, lo + per);
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += deg[i];
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
    off[i] = run;
    run += deg[i];
  }
  if (tid == kScanThreads - 1) off[n] = part[tid];
}

__global__ void rev_fill_kernel(const int32_t* active, int64_t n, int k,
                                   const int32_t* __restrict__ ids, const double* __restrict__ dist,
                                   const int32_t* __restrict__ count, const int64_t* __restrict__ off,
                                   int32_t* cur, int32_t* __restrict__ rsrc,
                                   double* __restrict__ rdist) {
  if (!*active) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * k; e += stride) {
    int64_t j;
    int t;
    if (!edge_of(e, n, k, ids, count, j, t)) continue;
    const int64_t p = off[t] + atomicAdd(&cur[t], 1);
    rsrc[p] = (int32_t)j;
    rdist[p] = dist[e];
  }
}

}  // namespace
}  // namespace rpt
