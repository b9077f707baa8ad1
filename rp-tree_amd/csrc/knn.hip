// knn.hip — query side of the hot path.
//
//   candidates (RPTree.hs:289-314): per tree a DFS from the root with the query's projection
//       on the level's hyperplane; the 4-way rule may descend both children; the leaf buckets
//       reached are concatenated left to right.
//   knn (RPTree.hs:168-176): concatenate the candidates of all trees in ascending tree key
//       (duplicates kept), distance of every candidate to the query (metricL2), stable sort
//       by distance, take k.  Equivalent total order: (distance, candidate position).
//
// Kernels (wave64, one workgroup per query):
//   count_kernel  : thread = tree; counts the leaf ranges / candidates each tree contributes
//   ranges_kernel : same traversal, writes (perm offset, length, candidate position) ranges
//   topk_kernel   : each wave streams candidate rows (whole-row coalesced gathers from HBM —
//                   this is the bandwidth-bound part, d*sizeof(x) bytes per candidate),
//                   wave-reduces the squared distance, and the block keeps the best k in LDS
//                   by bitonic-merging batches of candidates
//   expand_kernel : materialises candidate ids for rpt_candidates
#include <hip/hip_bf16.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "common.h"
#include <unordered_map>

#include "knn_allow.h"
#include "knn_vote.h"

namespace rpt {
namespace {

constexpr int kBuf = 2048;  // LDS entries of the top-k merge buffer (best k + batch)

struct Range {
  int64_t poff;  // absolute offset into perm ([T][N] flattened)
  int32_t n;
  int32_t pos;   // position of the range's first candidate in the query's candidate list
};

// ---- traversal ---------------------------------------------------------------------------
// emit(off, n) is called for every leaf reached, left to right.  Depth-first, left child first;
// the right children still to visit lie on the current path at distinct levels, so a 32-bit
// mask of those levels plus the current node's heap index is the whole stack: a pop takes the
// deepest pending level l, the ancestor of the current node at that level, its right child,
// and replays the l+1 halvings along that child's path for (off, n).  (Explicit stacks of
// (level, heap, off, n) cost 128 registers and held the fused kernels to 2 waves per SIMD.)
template <class TK, class Emit>
__device__ inline void traverse(const double* __restrict__ thr, const double* __restrict__ mglo,
                                const double* __restrict__ mghi, const TK* __restrict__ pq,
                                int64_t pq_stride, int L, int min_leaf, int64_t N, Emit emit) {
  unsigned int pending = 0, heap = 0;
  int level = 0, off = 0, n = (int)N;
  // Two levels per memory round trip (round 3): the walk is a chain of dependent node loads — 13 at
  // C2, a fifth of a query's life in the fused kernels — so a node's record is fetched together
  // with the records of BOTH its children (adjacent heap slots), and the child the decision picks
  // is decided on at once.  `last` clamps the children of the deepest Bin level into the arrays
  // (their records are never used: the level test comes first).
  const unsigned int last = L > 0 ? (1u << L) - 2u : 0u;
  auto step = [&](double th, double lo, double hi, double proj) {  // RPTree.hs:303-314
    const double dl = fabs(lo - proj);  // :306
    const double dr = fabs(hi - proj);  // :307
    const int nh = n / 2;
    const bool both = (proj < th && dl > dr) || (proj > th && dl < dr);  // :309-313
    if (both) {  // the right child waits, continue left
      pending |= 1u << level;
      heap = 2 * heap + 1;
      n = nh;
    } else if (proj < th) {  // :311
      heap = 2 * heap + 1;
      n = nh;
    } else {  // :314 (includes proj == thr)
      heap = 2 * heap + 2;
      off += nh;
      n = n - nh;
    }
    ++level;
  };
  for (;;) {
    for (;;) {
      if (level >= L || n <= min_leaf) {  // Tip (RPTree.hs:299)
        emit(off, n);
        break;
      }
      const unsigned int c0 = 2 * heap + 1 < last ? 2 * heap + 1 : last;
      const unsigned int c1 = 2 * heap + 2 < last ? 2 * heap + 2 : last;
      const int l1 = level + 1 < L ? level + 1 : level;
      const double proj = (double)pq[(int64_t)level * pq_stride];
      const double proj1 = (double)pq[(int64_t)l1 * pq_stride];
      const double th = thr[heap], lo = mglo[heap], hi = mghi[heap];
      const double th0 = thr[c0], lo0 = mglo[c0], hi0 = mghi[c0];
      const double th1 = thr[c1], lo1 = mglo[c1], hi1 = mghi[c1];
      step(th, lo, hi, proj);
      if (level >= L || n <= min_leaf) {
        emit(off, n);
        break;
      }
      const bool right = (heap & 1u) == 0u;  // heap = 2 h + 2
      step(right ? th1 : th0, right ? lo1 : lo0, right ? hi1 : hi0, proj1);
    }
    if (!pending) break;
    const int l = 31 - __clz((int)pending);
    pending &= ~(1u << l);
    heap = 2 * (((heap + 1) >> (level - l)) - 1) + 2;
    const unsigned int path = heap + 1;  // 1, then the l+1 decisions from the root down
    off = 0;
    n = (int)N;
    for (int i = l; i >= 0; --i) {
      const int nh = n / 2;
      if ((path >> i) & 1u) {
        off += nh;
        n -= nh;
      } else {
        n = nh;
      }
    }
    level = l + 1;
  }
}

// The same walk over an EXPLICIT topology (forests of the streaming build, common.h rpt_forest:
// kind 0 absent / 1 Bin / 2 Tip per heap slot, a Tip's range = (xoff, xlen)); same stackless
// scheme, nothing to replay on a pop.
template <class TK, class Emit>
__device__ inline void traverse_x(const double* __restrict__ thr, const double* __restrict__ mglo,
                                  const double* __restrict__ mghi, const int8_t* __restrict__ kind,
                                  const int64_t* __restrict__ xoff, const int64_t* __restrict__ xlen,
                                  const TK* __restrict__ pq, int64_t pq_stride, Emit emit) {
  unsigned int pending = 0, heap = 0;
  int level = 0;
  for (;;) {
    for (;;) {
      if (kind[heap] != 1) {  // Tip (RPTree.hs:299); an absent slot holds nothing
        if (kind[heap] == 2) emit((int)xoff[heap], (int)xlen[heap]);
        break;
      }
      const double proj = (double)pq[(int64_t)level * pq_stride];  // RPTree.hs:303-304
      const double th = thr[heap];
      const double dl = fabs(mglo[heap] - proj);
      const double dr = fabs(mghi[heap] - proj);
      const bool both = (proj < th && dl > dr) || (proj > th && dl < dr);
      if (both) {
        pending |= 1u << level;
        heap = 2 * heap + 1;
      } else if (proj < th) {
        heap = 2 * heap + 1;
      } else {
        heap = 2 * heap + 2;
      }
      ++level;
    }
    if (!pending) break;
    const int l = 31 - __clz((int)pending);
    pending &= ~(1u << l);
    heap = 2 * (((heap + 1) >> (level - l)) - 1) + 2;
    level = l + 1;
  }
}

template <class TK>
__global__ void count_x_kernel(const double* __restrict__ thr, const double* __restrict__ mglo,
                               const double* __restrict__ mghi, int64_t nodes,
                               const int8_t* __restrict__ kind, const int64_t* __restrict__ xoff,
                               const int64_t* __restrict__ xlen, const TK* Pq, int64_t nq, int T, int L,
                               int* __restrict__ cnt_cand, int* __restrict__ cnt_rng) {
  const int64_t q = blockIdx.x;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    int nc = 0, nr = 0;
    traverse_x<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, kind, xoff, xlen,
                   Pq + (int64_t)t * L * nq + q, nq, [&](int, int n) {
                     nc += n;
                     ++nr;
                   });
    cnt_cand[q * T + t] = nc;
    cnt_rng[q * T + t] = nr;
  }
}

template <class TK>
__global__ void ranges_x_kernel(const double* __restrict__ thr, const double* __restrict__ mglo,
                                const double* __restrict__ mghi, int64_t nodes,
                                const int8_t* __restrict__ kind, const int64_t* __restrict__ xoff,
                                const int64_t* __restrict__ xlen, const TK* Pq, int64_t nq, int T, int L,
                                int64_t N, const int64_t* __restrict__ cand_off,
                                const int64_t* __restrict__ rng_off, Range* __restrict__ ranges) {
  const int64_t q = blockIdx.x;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    int64_t r = rng_off[q * T + t];
    int64_t pos = cand_off[q * T + t] - cand_off[q * T];
    traverse_x<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, kind, xoff, xlen,
                   Pq + (int64_t)t * L * nq + q, nq, [&](int off, int n) {
                     ranges[r++] = Range{(int64_t)t * N + off, n, (int)pos};
                     pos += n;
                   });
  }
}

// per (query, tree) counts.  grid = nq blocks, blockDim >= T (multiple of 64).
template <class TK>
__global__ void count_kernel(const double* __restrict__ thr, const double* __restrict__ mglo,
                             const double* __restrict__ mghi, int64_t nodes, const TK* Pq,
                             int64_t nq, int T, int L, int min_leaf, int64_t N,
                             int* __restrict__ cnt_cand /*[nq][T]*/,
                             int* __restrict__ cnt_rng /*[nq][T]*/) {
  const int64_t q = blockIdx.x;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    int nc = 0, nr = 0;
    traverse<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, Pq + (int64_t)t * L * nq + q,
                 nq, L, min_leaf, N, [&](int, int n) {
                   nc += n;
                   ++nr;
                 });
    cnt_cand[q * T + t] = nc;
    cnt_rng[q * T + t] = nr;
  }
}

// exclusive scan of int32 counts into int64 offsets (single block; n is small: nq*T).
__global__ __launch_bounds__(1024) void scan_kernel(const int* __restrict__ in, int64_t n,
                                                    int64_t* __restrict__ out /*[n+1]*/) {
  __shared__ long long part[1024];
  __shared__ long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const long long v = i < n ? in[i] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      long long add = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < n) out[i] = carry + part[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += part[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[n] = carry;
}

template <class TK>
__global__ void ranges_kernel(const double* __restrict__ thr, const double* __restrict__ mglo,
                              const double* __restrict__ mghi, int64_t nodes, const TK* Pq,
                              int64_t nq, int T, int L, int min_leaf, int64_t N,
                              const int64_t* __restrict__ cand_off /*[nq*T+1]*/,
                              const int64_t* __restrict__ rng_off /*[nq*T+1]*/,
                              Range* __restrict__ ranges) {
  const int64_t q = blockIdx.x;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    int64_t r = rng_off[q * T + t];
    int64_t pos = cand_off[q * T + t] - cand_off[q * T];
    traverse<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, Pq + (int64_t)t * L * nq + q,
                 nq, L, min_leaf, N, [&](int off, int n) {
                   ranges[r++] = Range{(int64_t)t * N + off, n, (int)pos};
                   pos += n;
                 });
  }
}

// candidatesH (RPTree.hs:318-342): the same descent, every leaf reached carries the smallest
// margin distance met on the way down (`p min dl` towards the left child, `p min dr` towards
// the right one, +infinity at the root).  emit(off, n, priority), left to right.
template <class TK, class Emit>
__device__ inline void traverse_h(const double* __restrict__ thr, const double* __restrict__ mglo,
                                  const double* __restrict__ mghi, const TK* __restrict__ pq,
                                  int64_t pq_stride, int L, int min_leaf, int64_t N, Emit emit) {
  int s_level[32];
  unsigned int s_heap[32];
  int s_off[32], s_n[32];
  double s_p[32];
  int sp = 1;
  s_level[0] = 0;
  s_heap[0] = 0;
  s_off[0] = 0;
  s_n[0] = (int)N;
  s_p[0] = __longlong_as_double(0x7ff0000000000000LL);  // :320 infty = 1 / 0
  while (sp > 0) {
    --sp;
    int level = s_level[sp];
    unsigned int heap = s_heap[sp];
    int off = s_off[sp], n = s_n[sp];
    double p = s_p[sp];
    for (;;) {
      if (level >= L || n <= min_leaf) {  // :323 Tip
        emit(off, n, p);
        break;
      }
      const double proj = (double)pq[(int64_t)level * pq_stride];
      const double th = thr[heap];
      const double dl = fabs(mglo[heap] - proj);  // :330
      const double dr = fabs(mghi[heap] - proj);  // :331
      const double pl = p <= dl ? p : dl;         // :332
      const double pr = p <= dr ? p : dr;         // :333
      const int nh = n / 2;
      const bool both = (proj < th && dl > dr) || (proj > th && dl < dr);  // :335-339
      const bool left = proj < th;
      if (both) {  // push right, continue left
        s_level[sp] = level + 1;
        s_heap[sp] = 2 * heap + 2;
        s_off[sp] = off + nh;
        s_n[sp] = n - nh;
        s_p[sp] = pr;
        ++sp;
        heap = 2 * heap + 1;
        n = nh;
        p = pl;
      } else if (left) {
        heap = 2 * heap + 1;
        n = nh;
        p = pl;
      } else {
        heap = 2 * heap + 2;
        off += nh;
        n = n - nh;
        p = pr;
      }
      ++level;
    }
  }
}

// priorities of the leaf ranges, in the order ranges_kernel lists them
template <class TK>
__global__ void ranges_h_kernel(const double* __restrict__ thr, const double* __restrict__ mglo,
                                const double* __restrict__ mghi, int64_t nodes, const TK* Pq,
                                int64_t nq, int T, int L, int min_leaf, int64_t N,
                                const int64_t* __restrict__ rng_off /*[nq*T+1]*/,
                                double* __restrict__ prio) {
  const int64_t q = blockIdx.x;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    int64_t r = rng_off[q * T + t];
    traverse_h<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes,
                   Pq + (int64_t)t * L * nq + q, nq, L, min_leaf, N,
                   [&](int, int, double p) { prio[r++] = p; });
  }
}

// ... and over an EXPLICIT topology (streamed forests): candidatesH walks the RPT value whatever built
// it (RPTree.hs:318-342); a Tip's bucket may be empty, its entry is inserted all the same (:323)
template <class TK>
__global__ void ranges_hx_kernel(const double* __restrict__ thr, const double* __restrict__ mglo,
                                 const double* __restrict__ mghi, int64_t nodes,
                                 const int8_t* __restrict__ kind, const TK* Pq, int64_t nq, int T, int L,
                                 const int64_t* __restrict__ rng_off /*[nq*T+1]*/, double* __restrict__ prio) {
  const int64_t q = blockIdx.x;
  for (int t = threadIdx.x; t < T; t += blockDim.x) {
    int64_t r = rng_off[q * T + t];
    const double *th = thr + t * nodes, *lo = mglo + t * nodes, *hi = mghi + t * nodes;
    const TK* pq = Pq + (int64_t)t * L * nq + q;
    int s_level[32];
    unsigned int s_heap[32];
    double s_p[32];
    int sp = 1;
    s_level[0] = 0;
    s_heap[0] = 0;
    s_p[0] = __longlong_as_double(0x7ff0000000000000LL);  // :320 infty = 1 / 0
    while (sp > 0) {
      --sp;
      int level = s_level[sp];
      unsigned int heap = s_heap[sp];
      double p = s_p[sp];
      for (;;) {
        if (kind[heap] != 1) {  // :323 Tip (an absent slot holds nothing: the same test as traverse_x)
          if (kind[heap] == 2) prio[r++] = p;
          break;
        }
        const double proj = (double)pq[(int64_t)level * nq];
        const double dl = fabs(lo[heap] - proj), dr = fabs(hi[heap] - proj);  // :330-331
        const double pl = p <= dl ? p : dl, pr = p <= dr ? p : dr;            // :332-333
        const bool both = (proj < th[heap] && dl > dr) || (proj > th[heap] && dl < dr);  // :335-339
        if (both) {  // push right, continue left
          s_level[sp] = level + 1;
          s_heap[sp] = 2 * heap + 2;
          s_p[sp] = pr;
          ++sp;
          heap = 2 * heap + 1;
          p = pl;
        } else if (proj < th[heap]) {
          heap = 2 * heap + 1;
          p = pl;
        } else {
          heap = 2 * heap + 2;
          p = pr;
        }
        ++level;
      }
    }
  }
}

// candidate ids for rpt_candidates: one block per (query, tree) range list
__global__ void expand_kernel(const int32_t* __restrict__ perm, const Range* __restrict__ ranges,
                              const int64_t* __restrict__ rng_off, const int64_t* __restrict__ cand_off,
                              int T, int32_t* __restrict__ ids) {
  const int64_t q = blockIdx.x;
  const int64_t qbase = cand_off[q * T];
  for (int64_t r = rng_off[q * T]; r < rng_off[(q + 1) * T]; ++r) {
    const Range rg = ranges[r];
    for (int i = threadIdx.x; i < rg.n; i += blockDim.x)
      ids[qbase + rg.pos + i] = perm[rg.poff + i];
  }
}

// ---- distance + top-k --------------------------------------------------------------------
struct Entry {
  double dist;
  int pos;
  int id;
};
__device__ inline bool entry_less(const Entry& a, const Entry& b) {
  return a.dist < b.dist || (a.dist == b.dist && a.pos < b.pos);
}
// The total order of the metric kernels and of the multi-GPU merge, whatever the values are:
// numbers by (distance, position), then NaN distances by position (the rule finalize_leftfold
// applies), then unused slots (id -1) by position.  entry_less leaves NaN unordered.
__device__ inline int entry_class(const Entry& e) { return e.id < 0 ? 2 : (e.dist != e.dist ? 1 : 0); }
__device__ inline bool entry_less_total(const Entry& a, const Entry& b) {
  const int ca = entry_class(a), cb = entry_class(b);
  if (ca != cb) return ca < cb;
  if (ca == 0 && a.dist != b.dist) return a.dist < b.dist;
  return a.pos < b.pos;
}

template <bool TOTAL = false>
__device__ inline void bitonic_entries(Entry* e, int np) {
  for (int k = 2; k <= np; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (np >> 1); i += blockDim.x) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const int hi = lo | j;
        const bool up = (lo & k) == 0;
        const Entry a = e[lo], b = e[hi];
        if constexpr (TOTAL) {
          if (up ? entry_less_total(b, a) : entry_less_total(a, b)) {
            e[lo] = b;
            e[hi] = a;
          }
        } else if (up ? entry_less(b, a) : entry_less(a, b)) {
          e[lo] = b;
          e[hi] = a;
        }
      }
      __syncthreads();
    }
}

// Merge step: sort buf[0, np) and keep the best k (optionally unique ids) at the front.
// Returns the number of valid best entries.  All threads call; `scratch` is int[kBuf].
// dedup: 0 keep duplicates (knn), 1 each id once, 2 each DISTANCE once (knnPQ's `nub`)
// TOTAL: order by entry_less_total (NaN distances last); under dedup 1 two NaN distances of one id
// are one entry, under dedup 2 NaN equals nothing (`nub` compares with ==)
template <bool TOTAL = false>
__device__ int merge_best(Entry* buf, int filled, int k, int dedup, int* scratch) {
  int np = 1;
  while (np < filled) np <<= 1;
  for (int i = filled + threadIdx.x; i < np; i += blockDim.x)
    buf[i] = Entry{__longlong_as_double(0x7ff0000000000000LL), 0x7fffffff, -1};
  __syncthreads();
  bitonic_entries<TOTAL>(buf, np);
  if (!dedup) return filled < k ? filled : k;
  // same id => same distance (deterministic distance function): a duplicate sits in the run
  // of equal distances before it
  for (int i = threadIdx.x; i < filled; i += blockDim.x) {
    int dup = 0;
    if (dedup == 2) {
      dup = i > 0 && buf[i - 1].dist == buf[i].dist;
    } else {
      if constexpr (TOTAL) {
        const double di = buf[i].dist;
        for (int j = i - 1; j >= 0 && (buf[j].dist == di || (di != di && buf[j].dist != buf[j].dist)); --j)
          if (buf[j].id == buf[i].id) {
            dup = 1;
            break;
          }
      } else {
        for (int j = i - 1; j >= 0 && buf[j].dist == buf[i].dist; --j)
          if (buf[j].id == buf[i].id) {
            dup = 1;
            break;
          }
      }
    }
    scratch[i] = dup;
  }
  __syncthreads();
  // thread 0 compacts the first k unique entries (k is small; filled <= kBuf)
  __shared__ int s_kept;
  if (threadIdx.x == 0) {
    int w = 0;
    for (int i = 0; i < filled && w < k; ++i)
      if (!scratch[i]) {
        if (w != i) buf[w] = buf[i];
        ++w;
      }
    s_kept = w;
  }
  __syncthreads();
  return s_kept;
}

template <class TD>
struct AccOf { typedef float type; };
template <>
struct AccOf<double> { typedef double type; };

template <class TD>
__device__ inline typename AccOf<TD>::type ld(const TD* p) { return (typename AccOf<TD>::type)*p; }
template <>
__device__ inline float ld<__hip_bfloat16>(const __hip_bfloat16* p) { return __bfloat162float(*p); }

template <class TA>
__device__ inline TA wave_sum(TA v) {
  // fixed butterfly: the result does not depend on which wave computes it
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// metricDDL2 exactly as the reference evaluates it (Internal.hs:403-406): a LEFT FOLD of
// (u - v) ** 2 over the coordinates, then the root — one thread per row.  The batched distance
// passes reduce a row by a lane butterfly (same value to ~1 ulp, different last bits); the few
// rows that reach a result are evaluated again this way, so the distances that leave the
// library carry the reference's bits and their order is the order of those values.
__device__ inline double leftfold_distance(const double* __restrict__ x, const double* qs, int d) {
  double acc = 0.0;
  int j = 0;
  // one thread walks one row: the row's loads go out thirty-two elements at a time (sixteen 16-byte
  // loads in flight) so that the walk waits for HBM d / 32 times, not d / 4; the sum itself is the
  // reference's left fold whatever the grouping of the loads
  if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    typedef double d2 __attribute__((ext_vector_type(2), aligned(16)));
    for (; j + 32 <= d; j += 32) {
      d2 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = *reinterpret_cast<const d2*>(x + j + 2 * u);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const double t0 = v[u][0] - qs[j + 2 * u];
        acc = acc + t0 * t0;
        const double t1 = v[u][1] - qs[j + 2 * u + 1];
        acc = acc + t1 * t1;
      }
    }
  }
  for (; j < d; ++j) {
    const double t = x[j] - qs[j];
    acc = acc + t * t;
  }
  return sqrt(acc);
}

// The certified cut.  Both sums of a row add the SAME rounded, non-negative products p_j = t_j t_j,
// t_j = fl(x_j - q_j) (-ffp-contract=off: no FMA), from +0 in different orders.  Whatever the order,
// the d terms are merged by d - 1 additions that round (adding a zero is exact), so a term passes
// through at most d - 1 of them, and with no cancellation the computed sum is S (1 + t), S = sum p_j
// exactly, |t| <= g = (d - 1) u / (1 - (d - 1) u), u = 2^-53 (Higham, Accuracy and Stability, (4.4)).
// Underflow adds nothing: the products are the same numbers in both sums, an addition whose result
// is subnormal is exact, and so is the root's operand.  The root is correctly rounded: fold = sqrt(S
// (1 + t1)) (1 + e1), butterfly = sqrt(S (1 + t2)) (1 + e2), |e| <= u, hence
//     fold / butterfly >= sqrt((1 - g) / (1 + g)) (1 - u) / (1 + u) >= 1 - g - 2 g^2 - 2 u
//                      >= 1 - (d + 2) u            (d <= 2^20: g <= (d - 1) u + u / 2, 2 g^2 <= u / 2).
// With E = (d + 4) u, 1 - E is exact (a multiple of 2^-53 below 1) and the product b (1 - E) rounds
// once: fl(b (1 - E)) <= b (1 - (d + 3) u).  Every candidate left out of the kept set has a
// butterfly value >= b, the value of the LAST kept entry, so its fold is >= b (1 - (d + 2) u), which
// is above fl(b (1 - E)).  A query is certified when nothing was left out (copies of a kept id under
// a duplicate rule aside: one id, one value), or when k entries were written and the k-th of them,
// by the fold, is STRICTLY below fl(b (1 - E)): no candidate left out can belong to the answer nor,
// under dedup 2, equal a value in it.  b must be finite (+inf, also what a NaN is ranked as, orders
// nothing among those left out) and a NaN fold value fails the comparison: such a query is not certified.
__device__ inline bool l2_cut_certified(bool cut, int written, int k, double kth_fold, double b, int d) {
  if (!cut) return true;
  if (written != k || d > (1 << 20) || !(b < __longlong_as_double(0x7ff0000000000000LL))) return false;
  return kth_fold < b * (1.0 - (double)(d + 4) * 0x1p-53);
}

__device__ int merge_distinct(Entry* buf, int filled, int kk, int cap, bool ided, int* scratch, int* s_out);

// ---- cosine and inner-product metrics (RPT_KNN_METRIC_COSINE / _INNER) ----
// The reference's knn takes the distance as an argument (RPTree.hs:168-176); these two are
//     inner :  -dot(x, q)                                   knn (\x q -> negate (inner x q))
//     cosine:  1 - dot(x, q) / (sqrt(dot(x, x)) * sqrt(dot(q, q)))
// with dot = innerDD (Internal.hs:384-385), the left fold ((0 + x0 q0) + x1 q1) + ... in Double over
// the exactly widened elements, every product and sum rounded on its own (no FMA).  A zero row or
// query has cosine NaN.  Smaller is nearer for both.
constexpr int kMetricL2 = 0, kMetricCosine = 1, kMetricInner = 2;

template <int METRIC>
__device__ __forceinline__ double metric_value(double dot, double xx, double qq) {
  if constexpr (METRIC == kMetricL2) return dot;  // (the exact L2 kernel: the value is the fold itself)
  else if constexpr (METRIC == kMetricInner) return -dot;
  else return 1.0 - dot / (sqrt(xx) * sqrt(qq));
}

// innerDD as the reference folds it, one thread per row: eight 16-byte loads in flight, the sum a
// left fold whatever the grouping of the loads.  SELF: dot(x, x) (qs unused).
template <class TD, bool SELF = false>
__device__ inline double leftfold_dot(const TD* __restrict__ x, const double* qs, int d) {
  constexpr int V = 16 / (int)sizeof(TD);
  double acc = 0.0;
  int j = 0;
  if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    struct alignas(16) Raw { TD v[V]; };
    for (; j + 8 * V <= d; j += 8 * V) {
      Raw r[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) r[u] = *reinterpret_cast<const Raw*>(x + j + u * V);
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const double xv = (double)ld<TD>(&r[u].v[v]);
          acc = acc + xv * (SELF ? xv : qs[j + u * V + v]);
        }
    }
  }
  for (; j < d; ++j) {
    const double xv = (double)ld<TD>(x + j);
    acc = acc + xv * (SELF ? xv : qs[j]);
  }
  return acc;
}

// Final stage of those paths: m kept entries (ids / positions in bid / bpos, m <= capacity of lf
// and order) -> left-fold distances, order by (distance, position), the duplicate rule on the
// FINAL values (dedup 2 = knnPQ's nub: one entry per distance; dedup 1: the kept ids are distinct
// already), the first k written.  tid / nthr / sync: the threads that share the arrays.
// METRIC != L2: the rows are TX (f64 / f32 / bf16), the values metric_value of the left-fold dot,
// rn the rows' dot(x, x) (cosine), qq the query's.
template <class Sync>
__device__ inline void finalize_select(int m, int k, int dedup, const double* lf, int* order, const int* bid,
                                       const int* bpos, int tid, int nthr, Sync sync, int64_t q,
                                       int32_t* __restrict__ out_ids, double* __restrict__ out_dist,
                                       int32_t* __restrict__ out_cnt, int* s_w, double* s_last);

template <int METRIC = kMetricL2, class TX = double, class Sync>
__device__ inline void finalize_leftfold(const TX* __restrict__ X, int d, const double* qs, int m,
                                         int k, int dedup, double* lf, int* order, const int* bid,
                                         const int* bpos, int tid, int nthr, Sync sync, int64_t q,
                                         int32_t* __restrict__ out_ids, double* __restrict__ out_dist,
                                         int32_t* __restrict__ out_cnt,
                                         const double* __restrict__ rn = nullptr, double qq = 0.0,
                                         int* s_w = nullptr, double* s_last = nullptr) {
  for (int i = tid; i < m; i += nthr) {
    if constexpr (METRIC == kMetricL2)
      lf[i] = leftfold_distance(X + (int64_t)bid[i] * d, qs, d);
    else
      lf[i] = metric_value<METRIC>(leftfold_dot<TX>(X + (int64_t)bid[i] * d, qs, d),
                                   METRIC == kMetricCosine ? rn[bid[i]] : 0.0, qq);
  }
  sync();
  finalize_select(m, k, dedup, lf, order, bid, bpos, tid, nthr, sync, q, out_ids, out_dist, out_cnt, s_w, s_last);
}

// finalize_leftfold's selection, the values lf[0, m) given (knn_metric_csr_kernel computes its own)
template <class Sync>
__device__ inline void finalize_select(int m, int k, int dedup, const double* lf, int* order, const int* bid,
                                       const int* bpos, int tid, int nthr, Sync sync, int64_t q,
                                       int32_t* __restrict__ out_ids, double* __restrict__ out_dist,
                                       int32_t* __restrict__ out_cnt, int* s_w, double* s_last) {
  for (int i = tid; i < m; i += nthr) {
    const double di = lf[i];
    const int pi = bpos[i];
    int rank = 0;
    // a total order whatever the values are: NaN (a NaN query or row, inf - inf) ranks behind every
    // number, NaNs among themselves by position — the ranks are a permutation of 0 .. m - 1
    if (di == di)
      for (int j = 0; j < m; ++j) rank += lf[j] < di || (lf[j] == di && bpos[j] < pi);
    else
      for (int j = 0; j < m; ++j) rank += lf[j] == lf[j] || bpos[j] < pi;
    order[rank] = i;
  }
  sync();
  if (tid == 0) {
    int w = 0;
    double last = -1.0;
    for (int r = 0; r < m && w < k; ++r) {
      const int i = order[r];
      if (dedup == 2 && w > 0 && lf[i] == last) continue;
      out_ids[q * k + w] = bid[i];
      out_dist[q * k + w] = last = lf[i];
      ++w;
    }
    out_cnt[q] = w;
    if (s_w) {  // (the metric kernel's certificate: the count and the last value written)
      *s_w = w;
      *s_last = w > 0 ? last : 0.0;
    }
    for (; w < k; ++w) {
      out_ids[q * k + w] = -1;
      out_dist[q * k + w] = __longlong_as_double(0x7ff0000000000000LL);
    }
  }
}

// dense data.  One block (256 threads) per query.  Candidate list given as ranges.
// `identity`: the candidate list is the whole dataset in id order (brute force), perm unused.
template <class TD>
__global__ __launch_bounds__(256) void topk_dense_kernel(
    const TD* __restrict__ X, int d, const TD* __restrict__ Q, const int32_t* __restrict__ perm,
    const Range* __restrict__ ranges, const int64_t* __restrict__ rng_off, int T, int64_t N,
    int identity, int k, int dedup, int32_t* __restrict__ out_ids, double* __restrict__ out_dist,
    int32_t* __restrict__ out_cnt, int32_t* __restrict__ unc /* f64: the queries whose cut is not certified */,
    unsigned long long* __restrict__ unc_count) {
  typedef typename AccOf<TD>::type TA;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Entry* buf = reinterpret_cast<Entry*>(smem);                       // [kBuf]
  int* scratch = reinterpret_cast<int*>(smem + sizeof(Entry) * kBuf);  // [kBuf]
  TA* qs = reinterpret_cast<TA*>(smem + (sizeof(Entry) + 4) * kBuf);   // [d]
  __shared__ int s_merge[2], s_w;
  __shared__ double s_last;
  constexpr bool F64 = std::is_same<TD, double>::value;
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < d; j += blockDim.x) qs[j] = ld<TD>(Q + q * d + j);
  __syncthreads();

  int best = 0;    // valid best entries at buf[0, best)
  int filled = 0;  // entries in buf (block-uniform)
  const int cap = kBuf;
  // f64: the running list keeps the entries of k + kLfMargin different ids (see kLfMargin)
  const int kk = F64 ? (k + kLfMargin < kBuf / 2 ? k + kLfMargin : kBuf / 2) : k;
  bool cut = false;  // f64: some candidate was left out of the list (other than a same-id copy)
  auto merge = [&]() -> int {
    if constexpr (F64) {
      const int w = merge_distinct(buf, filled, kk, kBuf / 2, dedup != 0, scratch, s_merge);
      cut = cut || s_merge[1] != 0;
      return w;
    } else {
      return merge_best(buf, filled, kk, dedup, scratch);
    }
  };
  const int64_t r0 = identity ? 0 : rng_off[q * T];
  const int64_t r1 = identity ? 1 : rng_off[(q + 1) * T];
  for (int64_t r = r0; r < r1; ++r) {
    Range rg;
    if (identity) rg = Range{0, (int32_t)N, 0};
    else rg = ranges[r];
    int done = 0;
    while (done < rg.n) {
      int take = rg.n - done;
      if (take > cap - filled) take = cap - filled;
      // each wave handles candidates wave, wave+4, ... of this slice, four rows in flight
      for (int i0 = wave; i0 < take; i0 += 16) {
        int idv[4];
        TA s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + 4 * u;
          const int c = done + (i < take ? i : i0);
          idv[u] = identity ? c : perm[rg.poff + c];
          s[u] = (TA)0;
        }
        // f32 / bf16 rows: the value IS the answer's distance and what the candidates are ranked on,
        // so a row is summed in the order of batch_distances (the fused kernels): rows of whole
        // 16-byte pieces give every lane the pieces lane, lane + 64, ... and each piece a left fold,
        // other rows the elements lane, lane + 64, ...; then the same butterfly.  (The lanes beyond a
        // short row add +0.0, which changes nothing.)  A query then gets the same bits and the same
        // order of near-ties on this path, the brute force included, as on the fused ones.
        constexpr int V = 16 / (int)sizeof(TD);
        if (!F64 && (d % V) == 0) {
          struct alignas(16) Raw { TD v[V]; };
          for (int j = lane * V; j < d; j += 64 * V) {
            Raw x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const Raw*>(X + (int64_t)idv[u] * d + j);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int v = 0; v < V; ++v) {
                const TA df = ld<TD>(&x[u].v[v]) - qs[j + v];
                s[u] += df * df;
              }
          }
        } else
        for (int j = lane; j < d; j += 64) {
          const TA qj = qs[j];
          TA x[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) x[u] = ld<TD>(X + (int64_t)idv[u] * d + j);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const TA df = x[u] - qj;
            s[u] += df * df;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + 4 * u;
          const TA tot = wave_sum(s[u]);
          if (lane == 0 && i < take)
            buf[filled + i] = Entry{(double)sqrt((double)tot), rg.pos + done + i, idv[u]};
        }
      }
      filled += take;
      done += take;
      __syncthreads();
      if (filled == cap) {
        best = merge();
        filled = best;
        __syncthreads();
      }
    }
  }
  if (filled > best || best == 0) {
    best = merge();
    __syncthreads();
  }
  if constexpr (F64) {
    // the kept entries' distances again as the reference's left fold, the k best of those in the
    // order of those values (ties by candidate position): finalize_leftfold
    double* lf = reinterpret_cast<double*>(scratch);  // [kBuf] ints = kBuf / 2 doubles >= kk
    int* ids2 = reinterpret_cast<int*>(buf + kBuf / 2);  // the upper half of buf is free now:
    int* pos2 = ids2 + kBuf / 2;                          // 3 x kBuf / 2 ints fit its 16 KB
    int* order = pos2 + kBuf / 2;
    const double blast = best > 0 ? buf[best - 1].dist : 0.0;  // (buf's lower half stays)
    for (int i = threadIdx.x; i < best; i += blockDim.x) {
      ids2[i] = buf[i].id;
      pos2[i] = buf[i].pos;
    }
    __syncthreads();
    finalize_leftfold(reinterpret_cast<const double*>(X), d, reinterpret_cast<const double*>(qs), best, k,
                      dedup, lf, order, ids2, pos2, (int)threadIdx.x, (int)blockDim.x,
                      [] { __syncthreads(); }, q, out_ids, out_dist, out_cnt, nullptr, 0.0, &s_w, &s_last);
    // (thread 0 wrote the answer and s_w / s_last)
    if (threadIdx.x == 0 && !l2_cut_certified(cut, s_w, k, s_last, blast, d))
      unc[atomicAdd(unc_count, 1ULL)] = (int32_t)q;
    return;
  }
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const bool ok = i < best;
    out_ids[q * k + i] = ok ? buf[i].id : -1;
    out_dist[q * k + i] = ok ? buf[i].dist : __longlong_as_double(0x7ff0000000000000LL);
  }
  if (threadIdx.x == 0) out_cnt[q] = best;
}

// distances of the candidates [first, fill) of an LDS batch (ids in cid) to the query in qs,
// written to cdist.  The waves taking part are numbered slot = 0 .. nslots-1; every row is
// reduced by the same fixed butterfly whichever wave handles it, so the value does not depend
// on the kernel variant.  Each wave keeps EIGHT load instructions in flight.
// DOT (the cosine / inner-product kernel): the row's inner product with the query, sum of x * q,
// instead of its squared distance (use with SQRT = false); the loads and the reduction are the same.
template <class TD, class TA, int INFL = 8 /* load instructions in flight per wave */,
          bool SQRT = true /* false: leave the squared distance (a TA value) in cdist */,
          class TO = double /* element type of the batch values */, bool DOT = false>
__device__ __forceinline__ void batch_distances(const TD* __restrict__ X, int d, const int* cid,
                                       TO* cdist, const TA* qs, int first, int fill, int slot,
                                       int nslots, int lane) {
  constexpr int VV = 16 / (int)sizeof(TD);
  const int lpr = (d % VV) == 0 ? d / VV : 0;  // lanes one row needs with 16-byte loads
  if (lpr > 0 && lpr <= 32 && (lpr & (lpr - 1)) == 0) {
    // short rows (<= 512 B): 64 / lpr rows per load instruction, eight instructions in flight
    struct alignas(16) Raw { TD v[VV]; };
    const int rpw = 64 / lpr, sub = lane / lpr, jl = (lane % lpr) * VV;
    for (int i0 = first + slot * INFL * rpw; i0 < fill; i0 += nslots * INFL * rpw) {
      TA s[INFL];
      Raw x[INFL];
#pragma unroll
      for (int u = 0; u < INFL; ++u) {
        const int i = i0 + u * rpw + sub;
        x[u] = *reinterpret_cast<const Raw*>(X + (int64_t)cid[i < fill ? i : i0] * d + jl);
      }
#pragma unroll
      for (int u = 0; u < INFL; ++u) {
        s[u] = (TA)0;
#pragma unroll
        for (int v = 0; v < VV; ++v) {
          if constexpr (DOT) {
            s[u] += ld<TD>(&x[u].v[v]) * qs[jl + v];
          } else {
            const TA df = ld<TD>(&x[u].v[v]) - qs[jl + v];
            s[u] += df * df;
          }
        }
        for (int o = lpr >> 1; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o);  // fixed butterfly
        const int i = i0 + u * rpw + sub;
        if (jl == 0 && i < fill) cdist[i] = SQRT ? (TO)sqrt((double)s[u]) : (TO)s[u];
      }
    }
  } else
  // ---- long rows: one row per load instruction, 8 rows in flight per wave ----
  for (int i0 = first + slot * 8; i0 < fill; i0 += nslots * 8) {
    TA s[8];
    const TD* rows[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u < fill ? i0 + u : i0;
      rows[u] = X + (int64_t)cid[i] * d;
      s[u] = (TA)0;
    }
    constexpr int V = 16 / (int)sizeof(TD);
    if ((d % V) == 0) {
      struct alignas(16) Raw { TD v[V]; };
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      for (int j = lane * V; j < d; j += 64 * V) {
        // All eight row loads are issued before the first is used.  That has to be SAID: at the
        // register cap of several instantiations (168 VGPRs at three workgroups per CU) the scheduler
        // turned this loop into load / wait / load / wait — one or two rows in flight instead of eight
        // — which is the whole of round 3's "66 -> 119 ms" cliff of the bf16 kernel under the
        // consecutive-slot fill (the fill cost 3 registers, the gathers lost their memory
        // parallelism) and had silently hit the f32 / half-tier kernels on rows beyond 512 bytes.
        // The group barrier keeps the eight VMEM reads one scheduling group ahead of the arithmetic;
        // the waits stay progressive (vmcnt 7, 6, ... as the rows are consumed).
        u32x4 raw[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) raw[u] = *reinterpret_cast<const u32x4*>(rows[u] + j);
        __builtin_amdgcn_sched_group_barrier(0x020, 8, 0);          // eight VMEM reads ...
        __builtin_amdgcn_sched_group_barrier(0x002, 8 * V * (DOT ? 2 : 3), 0);  // ... then the VALU work on them
        Raw x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) __builtin_memcpy(&x[u], &raw[u], 16);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int v = 0; v < V; ++v) {
            if constexpr (DOT) {
              s[u] += ld<TD>(&x[u].v[v]) * qs[j + v];
            } else {
              const TA df = ld<TD>(&x[u].v[v]) - qs[j + v];
              s[u] += df * df;
            }
          }
      }
    } else {
      for (int j = lane; j < d; j += 64) {
        const TA qj = qs[j];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if constexpr (DOT) {
            s[u] += ld<TD>(rows[u] + j) * qj;
          } else {
            const TA df = ld<TD>(rows[u] + j) - qj;
            s[u] += df * df;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const TA tot = wave_sum(s[u]);
      if (lane == 0 && i0 + u < fill) cdist[i0 + u] = SQRT ? (TO)sqrt((double)tot) : (TO)tot;
    }
  }
}

// ---- cosine / inner-product kernel ---------------------------------------------------------
constexpr int kMB = 512;  // candidates per batch of knn_metric_kernel
constexpr int kMW = 64;   // leaf ranges it holds in LDS at a time

// The certified cut.  Both sums of a row, the left fold and the butterfly, add the SAME rounded
// products p_j = x_j q_j (-ffp-contract=off: no FMA) in different orders, so by the standard bound
// of a summation (Higham, Accuracy and Stability, (3.5): each term goes through at most d - 1
// additions, its product one more rounding) each is within gamma_d S of the exact dot, S = sum |p_j|
// <= |x| |q| (Cauchy-Schwarz), gamma_d = d u / (1 - d u), u = 2^-53; subnormal results add at most
// 2^-1075 per rounding, 2d - 1 roundings per sum.  Hence
//     |fold - butterfly| <= 2 gamma_d |x| |q| + 2d 2^-1074.
// inner:  the values are -dot.  With xb = sqrt(max rn) + d 2^-537 >= |x| (rn = fold(x.x) >= |x|^2 (1 -
//   gamma_d) - d 2^-1075: the squares that underflow) and qb the same for the query,
//   2 gamma_d |x||q| <= 2 d u (1 + 2 d u + 4 u) xb qb <= (2d + 1) u xb qb (d u <= 2^-30), one u xb qb
//   more for the rounding of b - E (|b| <= (1 + gamma_d) S), two more for the products that form E:
//     E = (2d + 8) u xb qb + (2d + 8) 2^-1074,
//   and only when E <= 2^960: then every partial sum stays below 2^1013, no sum overflows.
// cosine: the values are 1 - dot / D with ONE denominator D = sqrt(rn) sqrt(qq) for both sums.  When
//   every row's rn and the query's qq lie in [2^-900, 2^900] (zero rows are NaN in both sums: any
//   rn = 0 row must be all zeros), D >= |x||q| (1 - gamma_d)(1 - u)^3 and the underflow term is
//   below 2^-159 relative to D: |dot_f - dot_b| / D <= 2 d u + 2 u; the two divisions add u |dot/D|
//   <= 1.0001 u each, the two 1 - t add u |1 - t| <= 2.0002 u each, b - E is rounded once more
//   (<= 2.1 u):  2 d u + 10.3 u, rounded up:
//     E = (2d + 16) u.
// A query is certified when nothing was excluded from the kept set, or when k entries were written
// and the k-th (by the fold) is strictly below b - E, b the butterfly value of the LAST kept entry:
// every excluded candidate has butterfly >= b, so fold >= b - E > the k-th, and cannot belong to the
// answer (nor, under dedup 2, remove a value from it).  NaN anywhere in that test fails it.
// E for one query (NaN: the query cannot be certified).  stats: the dataset's row statistics
// (row_stats_kernel: [0] the largest rn as bits, NaN as the largest; [1] nonzero when some row's rn
// is outside the cosine range above).
template <int METRIC>
__device__ inline double metric_cut_slack(int d, double qq, const unsigned long long* stats) {
  const double u = 0x1p-53;
  if constexpr (METRIC == kMetricCosine) {
    if (stats[1] != 0 || !(qq >= 0x1p-900 && qq <= 0x1p900)) return __longlong_as_double(0x7ff8000000000000LL);
    return (2.0 * d + 16.0) * u;
  } else {
    const double xb = sqrt(__longlong_as_double((long long)stats[0])) + (double)d * 0x1p-537;
    const double qb = sqrt(qq) + (double)d * 0x1p-537;
    const double e = (2.0 * d + 8.0) * u * xb * qb + (2.0 * d + 8.0) * 0x1p-1074;
    return e <= 0x1p960 ? e : __longlong_as_double(0x7ff8000000000000LL);
  }
}

// dot(x, x) of every row as the left fold (the metrics' row norms, cached on the dataset) and the
// dataset's statistics for the certified cut (metric_cut_slack): stats[0] max over the rows of
// rn's bits (rn >= 0: the bits order as the values; a NaN, sign cleared, above +inf), stats[1] set
// when a row's rn lies outside [2^-900, 2^900] and the row is not all zeros.  stats zeroed before.
template <class TD>
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const TD* __restrict__ X, int64_t n, int d,
                                                         double* __restrict__ rn,
                                                         unsigned long long* __restrict__ stats) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long bits = 0, bad = 0;
  if (r < n) {
    const double v = leftfold_dot<TD, true>(X + r * d, nullptr, d);
    rn[r] = v;
    bits = (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffULL;
    if (!(v >= 0x1p-900 && v <= 0x1p900)) {
      bad = v != 0.0;
      for (int j = 0; j < d && !bad; ++j) bad = (double)ld<TD>(X + r * d + j) != 0.0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long ob = __shfl_xor(bits, o), oo = __shfl_xor(bad, o);
    bits = ob > bits ? ob : bits;
    bad |= oo;
  }
  if ((threadIdx.x & 63) == 0) {
    if (bits) atomicMax(&stats[0], bits);
    if (bad) atomicOr(&stats[1], bad);
  }
}

// knn_metric_kernel's merge: sort buf[0, filled) in the total order and keep a prefix that holds
// kk DIFFERENT ids (copies of one row, the same point found by several trees, have equal sums of
// both kinds and must not eat the margin), at most cap entries.  ided: the entries of one id are
// one entry (the first: the lowest position); the prefix is compacted.  Returns the kept count;
// *cut (block-uniform) is set when some entry was left out for the prefix (not a same-id copy).
__device__ int merge_distinct(Entry* buf, int filled, int kk, int cap, bool ided, int* scratch, int* s_out) {
  int np = 1;
  while (np < filled) np <<= 1;
  for (int i = filled + threadIdx.x; i < np; i += blockDim.x)
    buf[i] = Entry{__longlong_as_double(0x7ff0000000000000LL), 0x7fffffff, -1};
  __syncthreads();
  bitonic_entries<true>(buf, np);
  // same id => same value: a copy sits in the run of equal values before it
  for (int i = threadIdx.x; i < filled; i += blockDim.x) {
    const double di = buf[i].dist;
    int dup = 0;
    for (int j = i - 1; j >= 0 && (buf[j].dist == di || (di != di && buf[j].dist != buf[j].dist)); --j)
      if (buf[j].id == buf[i].id) {
        dup = 1;
        break;
      }
    scratch[i] = dup;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int w = 0, distinct = 0, i = 0, cut = 0;
    for (; i < filled; ++i) {
      if (!scratch[i]) {
        if (distinct == kk || w == cap) {
          cut = 1;
          break;
        }
        ++distinct;
      } else if (ided) {
        continue;
      } else if (w == cap) {
        cut = 1;
        break;
      }
      if (w != i) buf[w] = buf[i];
      ++w;
    }
    s_out[0] = w;
    s_out[1] = cut;
  }
  __syncthreads();
  return s_out[0];
}

// knn under the cosine or inner-product metric, dense rows of any dtype, values in f64.  One
// workgroup (four waves) per query over the plan's leaf ranges in candidate order (or, identity:
// the whole dataset in id order, the brute force).  Batches of kMB candidates: ids and positions
// gathered across ranges, the values, and only the entries that beat the current cut in the total
// order appended to buf; a merge keeps the best when the next batch might not fit.
//   EXACT = false (every query): the values from batch_distances (the butterfly f64 sum, 16-byte
// row loads, the short-row layout up to 512-byte rows); merge_distinct keeps the entries of the
// best k + kLfMargin different ids (same-id copies collapse under dedup 1 and 2: one id, one value
// in both sums); those are evaluated again as the left fold and selected in the finalize_leftfold
// order (NaN last, by position), the duplicate rule on the fold values.  Then the cut is certified
// (metric_cut_slack); when it is not, q is appended to the list unc (*unc_count entries).
//   EXACT = true (the queries of that list, grid-stride; unc == nullptr: all nq): every value is the left fold (one
// thread per row) and merge_best selects on those with no margin; the answer is the definition.
//   METRIC = kMetricL2 (f64 rows, EXACT only): the values are metricDDL2's fold, leftfold_distance.  It
// answers the queries whose cut no L2 path on dense f64 rows could certify (see kLfMargin), the
// prefilter tiers' among them, and every query under the option knn_l2_exact.
// LDS: buf [nbuf] entries (a power of two >= kk + kMB), scratch [nbuf] ints, the batch (kMB x 16 B),
// the query [d] doubles.
template <class TD, int METRIC, bool EXACT>
__global__ __launch_bounds__(256) void knn_metric_kernel(
    const TD* __restrict__ X, int d, const TD* __restrict__ Q, int64_t nq, const int32_t* __restrict__ perm,
    const Range* __restrict__ ranges, const int64_t* __restrict__ rng_off, int T, int64_t N,
    int identity, int nbuf, int k, int dedup, const double* __restrict__ rn,
    const unsigned long long* __restrict__ stats, int32_t* __restrict__ unc,
    unsigned long long* __restrict__ unc_count, int32_t* __restrict__ out_ids, double* __restrict__ out_dist,
    int32_t* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Entry* buf = reinterpret_cast<Entry*>(smem);                      // [nbuf]
  int* scratch = reinterpret_cast<int*>(smem + sizeof(Entry) * nbuf);  // [nbuf]
  double* cd = reinterpret_cast<double*>(scratch + nbuf);           // [kMB]
  int* cid = reinterpret_cast<int*>(cd + kMB);                      // [kMB]
  int* cpos = cid + kMB;                                            // [kMB]
  double* qs = reinterpret_cast<double*>(cpos + kMB);               // [d]
  __shared__ Range s_rng[kMW];
  __shared__ int s_fill, s_merge[2], s_w;
  __shared__ double s_qq, s_blast, s_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kk = EXACT ? k : (k + kLfMargin < nbuf / 2 ? k + kLfMargin : nbuf / 2);
  const int sdedup = EXACT ? dedup : (dedup ? 1 : 0);  // the fast path's rule while streaming
  const int64_t nw = EXACT && unc ? (int64_t)*unc_count : nq;  // the queries of this launch
  for (int64_t iw = blockIdx.x; iw < nw; iw += gridDim.x) {
    const int64_t q = EXACT && unc ? (int64_t)unc[iw] : iw;
    __syncthreads();  // (the previous query's finalize still reads the arrays)
    for (int j = threadIdx.x; j < d; j += blockDim.x) qs[j] = (double)ld<TD>(Q + q * d + j);
    if (threadIdx.x == 0) s_fill = 0;
    __syncthreads();
    // dot(q, q) (read after the first batch's barriers); the elements in LDS are the widened query
    if ((METRIC == kMetricCosine || !EXACT) && threadIdx.x == 0) s_qq = leftfold_dot<double, true>(qs, nullptr, d);

    int best = 0;
    bool cut = false;       // some candidate is not in buf (other than a same-id copy)
    Entry thr{0.0, 0, -1};  // the last kept entry after a cut; id -1: none yet, every entry enters
    const int64_t r0 = identity ? 0 : rng_off[q * T];
    const int64_t r1 = identity ? 1 : rng_off[(q + 1) * T];
    int64_t r = r0, w0 = r0, w1 = r0;  // next range; ranges [w0, w1) are in s_rng
    int done = 0;                      // candidates of range r already taken
    while (r < r1) {
      int nb = 0;
      while (nb < kMB && r < r1) {  // block-uniform
        if (r == w1) {
          __syncthreads();
          w0 = r;
          w1 = r + kMW < r1 ? r + kMW : r1;
          for (int i = threadIdx.x; i < w1 - w0; i += blockDim.x)
            s_rng[i] = identity ? Range{0, (int32_t)N, 0} : ranges[w0 + i];
          __syncthreads();
        }
        const Range rg = s_rng[r - w0];
        int take = rg.n - done;
        if (take > kMB - nb) take = kMB - nb;
        for (int i = threadIdx.x; i < take; i += blockDim.x) {
          const int c = done + i;
          cid[nb + i] = identity ? c : perm[rg.poff + c];
          cpos[nb + i] = rg.pos + c;
        }
        nb += take;
        done += take;
        if (done == rg.n) {
          ++r;
          done = 0;
        }
      }
      __syncthreads();
      if constexpr (METRIC == kMetricL2) {  // (f64 rows, EXACT only: metricDDL2 itself)
        static_assert(METRIC != kMetricL2 || (EXACT && std::is_same<TD, double>::value), "L2: the exact variant on f64 rows");
        for (int i = threadIdx.x; i < nb; i += blockDim.x)
          cd[i] = leftfold_distance(reinterpret_cast<const double*>(X) + (int64_t)cid[i] * d, qs, d);
      } else if constexpr (EXACT) {
        for (int i = threadIdx.x; i < nb; i += blockDim.x) cd[i] = leftfold_dot<TD>(X + (int64_t)cid[i] * d, qs, d);
      } else {
        batch_distances<TD, double, 8, false, double, true>(X, d, cid, cd, qs, 0, nb, wave, 4, lane);
      }
      __syncthreads();
      const double qq = METRIC == kMetricCosine ? s_qq : 0.0;
      // the order inside buf does not matter (the merges sort by value and position)
      for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        const Entry e{metric_value<METRIC>(cd[i], METRIC == kMetricCosine ? rn[cid[i]] : 0.0, qq), cpos[i],
                      cid[i]};
        if (entry_less_total(e, thr)) buf[atomicAdd(&s_fill, 1)] = e;
      }
      __syncthreads();
      const int filled = s_fill;
      if (filled + kMB > nbuf || r >= r1) {
        if constexpr (EXACT) {
          best = merge_best<true>(buf, filled, kk, sdedup, scratch);
          if (best == kk) thr = buf[kk - 1];
        } else {
          best = merge_distinct(buf, filled, kk, nbuf / 2, sdedup != 0, scratch, s_merge);
          if (s_merge[1]) {
            cut = true;
            thr = buf[best - 1];
          }
        }
        __syncthreads();
        if (threadIdx.x == 0) s_fill = best;
        __syncthreads();
      }
    }
    if (threadIdx.x == 0) s_blast = best > 0 ? buf[best - 1].dist : 0.0;  // (buf's lower half stays)
    double* lf = reinterpret_cast<double*>(scratch);        // nbuf / 2 doubles >= kk
    int* ids2 = reinterpret_cast<int*>(buf + nbuf / 2);     // the upper half of buf is free now:
    int* pos2 = ids2 + nbuf / 2;                            // 3 x nbuf / 2 ints fit its 8 x nbuf bytes
    int* order = pos2 + nbuf / 2;
    for (int i = threadIdx.x; i < best; i += blockDim.x) {
      ids2[i] = buf[i].id;
      pos2[i] = buf[i].pos;
    }
    __syncthreads();
    finalize_leftfold<METRIC>(X, d, qs, best, k, dedup, lf, order, ids2, pos2, (int)threadIdx.x,
                              (int)blockDim.x, [] { __syncthreads(); }, q, out_ids, out_dist, out_cnt, rn,
                              METRIC == kMetricCosine ? s_qq : 0.0, &s_w, &s_last);
    if (!EXACT && threadIdx.x == 0) {  // (the thread that wrote the answer and s_w / s_last)
      bool ok = !cut;
      if (!ok && s_w == k) ok = s_last < s_blast - metric_cut_slack<METRIC>(d, s_qq, stats);
      if (!ok) unc[atomicAdd(unc_count, 1ULL)] = (int32_t)q;
    }
  }
}

// ---- int8 ranking tier (round 3) ----------------------------------------------------------
// The dataset's int8 shadow holds c = rint(x / s) clamped to [-127, 127] with ONE scale s for the
// whole dataset, stored offset-binary (c + 128), rows of d bytes (d % 16 == 0): an eighth of the f64
// bytes, a 128-element row is one cache line.  The query is quantised SIXTEEN bits deep on the
// same grid, g = rint(256 q / s) clamped to the int16 range, kept as two byte planes (g = 256 H +
// Lo, H + 128 and Lo packed four to a word in LDS), and a candidate is ranked on the INTEGER
//     I = sum (g_j - 256 c_j)^2 = 65536 sum cu^2 - 131072 sum cu hu - 512 sum cu lo + K(query),
// cu = c + 128, hu = H + 128 (the sums of cu alone cancel), K = sum g^2 + 2^24 sum hu + 2^16 sum lo
// - 2^30 d: three v_dot4_u32_u8 per four elements, exact — no rounding anywhere in the ranking
// value (an 8-bit query doubled the uncertainty of the cut: at C2 17 candidates inside it instead of 9).
// By the triangle inequality the exact distance of a row x obeys
//     | |q - x| - (s / 256) sqrt(I) | <= |q - (s / 256) g| + |x - s c| <= eq + emax,
// eq computed per query in f64 (clipped elements included), emax = the dataset's largest
// |x - s c| (measured when the shadow is built), so a cut is certified exactly like the other
// tiers' (knn_fused_kernel), and an uncertified query is answered by the exact kernel.
struct Sh8 {
  double s, emax;  // scale, max row error; s == 0: the tier is not in use
};

// What a ranking tier knows about the exact distance D of a row from its estimate Dh (round 4):
//     lower(Dh) <= D <= upper(Dh),  lower(Dh) = (Dh - A - Bt Dh)(1 - Bf),  upper(Dh) = (Dh + A + Bt Dh)(1 + Bf)
//   f32 shadow : A = 2.1 u (xmax + |q|) + sqrt(d) 4e-23,             Bt = (d + 2) u   (rounded inputs,
//                differences, f32 accumulation, products in the subnormal range; knn_fused_kernel)
//   half shadow: A = 1.05 2^-11 xmax + 2.1 u |q| + sqrt(d) 3.1e-8,   Bt = (d + 2) u
//   int8 shadow: A = eq + emax (triangle inequality, Sh8), Bt = 0;  Dh = (s / 256) sqrt(I) and the
//                value kept is I rounded to f32 (rnd = 1.2e-7 covers it)
//   f32 DATA   : "exact" is the f32 distance the all-f32 kernel ranks on, within Bf = (d + 2) u of D
//                (every kernel that returns it is held to that bound, every query, by
//                tests/test_gpu_knn_f32_l2.py; tests/test_knn_f32_host.py: honest f32 sums reach 0.22 of it)
// The stored ranking value v is a non-negative float (a squared distance, or I); Dh = g sqrt(v).
struct TierBounds {
  double A, Bt, Bf, g, rnd;
  __device__ static TierBounds make(int tier /* 1 f32, 2 half, 3 int8 */, bool f64_data, int d, double xmax,
                                    double qnorm, double q8eq, Sh8 sh8) {
    const double u = 5.9604644775390625e-08;
    TierBounds b;
    b.A = tier == 3   ? (q8eq + sh8.emax) * (1.0 + 1e-12) + 1e-300
          : tier == 2 ? 1.05 * 4.8828125e-4 * xmax + 2.1 * u * qnorm + sqrt((double)d) * 3.1e-8
                      : 2.1 * u * (xmax + qnorm) + sqrt((double)d) * 4e-23;
    b.Bt = tier == 3 ? 0.0 : (double)(d + 2) * u;
    b.Bf = f64_data ? 0.0 : (double)(d + 2) * u * 1.01;
    b.g = tier == 3 ? sh8.s * (1.0 / 256.0) : 1.0;
    b.rnd = tier == 3 ? 1.2e-7 : 0.0;
    return b;
  }
  // the estimate of a stored value (its bits), rounded up
  __device__ double dh_up(unsigned int vb) const {
    return g * sqrt((double)__uint_as_float(vb) * (1.0 + rnd)) * (1.0 + 1e-15);
  }
  __device__ double upper(double dh) const { return (dh + A + Bt * dh) * (1.0 + Bf) * (1.0 + 1e-15); }
  // a row may be dropped against the bound Ulim on the exact k-th distance iff lower(Dh) > Ulim, i.e.
  // iff Dh > (Ulim / (1 - Bf) + A) / (1 - Bt); every stored value at or below the returned bits is KEPT
  __device__ unsigned int keep_bits(double Ulim) const {
    const double dstar = (Ulim / (1.0 - Bf) + A) / (1.0 - Bt) * (1.0 + 1e-15);
    const double t = (dstar / g) * (dstar / g) / (1.0 - rnd) * (1.0 + 1e-15);
    if (!(t < 3.0e38)) return 0x7fc00000u;  // inf / NaN: keep everything that is a number
    float tf = (float)t;
    if ((double)tf < t) tf = __uint_as_float(__float_as_uint(tf) + 1u);  // round up (t >= 0)
    return __float_as_uint(tf);
  }
  // may a row whose stored value is vb be dropped against Ulim?  (the certificate of a fixed cut)
  __device__ bool dropped_ok(unsigned int vb, double Ulim) const { return vb > keep_bits(Ulim); }
};

// quantised query -> planes[0 .. d/4) = hu words, planes[d/4 .. d/2) = lo words; the caller sums
// kq (this thread's share of K without the - 2^30 d term) and e2 (its share of eq^2) over its threads
__device__ inline void quantise_query(const double* qsrc_d, const float* qsrc_f, int d, double s,
                                      unsigned int* planes, int tid, int nthr, double& kq, double& e2) {
  kq = 0.0;
  e2 = 0.0;
  const double inv = 256.0 / s, g2x = s / 256.0;
  const int nw = d / 4;
  for (int w = tid; w < nw; w += nthr) {
    unsigned int wh = 0, wl = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const double v = qsrc_d ? qsrc_d[4 * w + b] : (double)qsrc_f[4 * w + b];
      double c = rint(v * inv);
      c = c < -32768.0 ? -32768.0 : (c > 32767.0 ? 32767.0 : c);  // NaN stays NaN: e2 turns NaN, no certificate
      const int g = c == c ? (int)c : 0;
      const double e = v - g2x * (double)g;
      e2 += e * e;
      const unsigned int hu = (unsigned int)((g >> 8) + 128), lo = (unsigned int)(g & 255);
      kq += (double)g * (double)g + 16777216.0 * (double)hu + 65536.0 * (double)lo;  // exact: < 2^53
      wh |= hu << (8 * b);
      wl |= lo << (8 * b);
    }
    planes[w] = wh;
    planes[nw + w] = wl;
  }
}

// number of keys of an LDS list below `mine`: the loads go out eight at a time (one load, one
// compare per turn left every iteration waiting out an LDS round trip: 14 k cycles for 150 keys)
__device__ __forceinline__ int count_below(const unsigned long long* lkey, int n, unsigned long long mine) {
  int rank = 0, j = 0;
  for (; j + 8 <= n; j += 8) {
    unsigned long long a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = lkey[j + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) rank += a[u] < mine;
  }
  for (; j < n; ++j) rank += lkey[j] < mine;
  return rank;
}
// ... and of (distance, position) pairs below (di, pi)
__device__ __forceinline__ int count_below2(const double* dd, const int* pp, int m, double di, int pi) {
  int rank = 0, j = 0;
  if (di != di) {  // NaN ranks behind every number, NaNs by position (a total order: no two equal ranks)
    for (; j < m; ++j) rank += dd[j] == dd[j] || pp[j] < pi;
    return rank;
  }
  for (; j + 8 <= m; j += 8) {
    double a[8];
    int b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a[u] = dd[j + u];
      b[u] = pp[j + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) rank += a[u] < di || (a[u] == di && b[u] < pi);
  }
  for (; j < m; ++j) rank += dd[j] < di || (dd[j] == di && pp[j] < pi);
  return rank;
}

// integer squared distances (see above) of the candidates [first, fill) -> cdist (exact integers
// as doubles, in units of (s / 256)^2)
template <int INFL = 16, class TO = double>
__device__ __forceinline__ void batch_distances_i8(const uint8_t* __restrict__ X8, int d, const int* cid,
                                                   TO* cdist, const unsigned int* planes, double kq,
                                                   int first, int fill, int slot, int nslots, int lane) {
  const int lpr = d / 16;  // lanes one row needs with 16-byte loads
  const int nw = d / 4;
  if (lpr <= 32 && (lpr & (lpr - 1)) == 0) {
    const int rpw = 64 / lpr, sub = lane / lpr, piece = lane % lpr;
    const uint4 hv = reinterpret_cast<const uint4*>(planes)[piece];
    const uint4 lv = reinterpret_cast<const uint4*>(planes + nw)[piece];
    const unsigned int hw[4] = {hv.x, hv.y, hv.z, hv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
    for (int i0 = first + slot * INFL * rpw; i0 < fill; i0 += nslots * INFL * rpw) {
      uint4 x[INFL];
#pragma unroll
      for (int u = 0; u < INFL; ++u) {
        const int i = i0 + u * rpw + sub;
        x[u] = *reinterpret_cast<const uint4*>(X8 + (int64_t)cid[i < fill ? i : i0] * d + piece * 16);
      }
#pragma unroll
      for (int u = 0; u < INFL; ++u) {
        const unsigned int xw[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
        unsigned int a = 0, b = 0, cc = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          a = __builtin_amdgcn_udot4(xw[w], hw[w], a, false);
          b = __builtin_amdgcn_udot4(xw[w], lw[w], b, false);
          cc = __builtin_amdgcn_udot4(xw[w], xw[w], cc, false);
        }
        for (int o = lpr >> 1; o > 0; o >>= 1) {
          a += __shfl_xor(a, o);
          b += __shfl_xor(b, o);
          cc += __shfl_xor(cc, o);
        }
        const int i = i0 + u * rpw + sub;
        if (piece == 0 && i < fill)
          cdist[i] = (TO)(65536.0 * (double)cc - 131072.0 * (double)a - 512.0 * (double)b + kq);
      }
    }
    return;
  }
  if (lpr <= 64) {
    // rows of up to 1024 bytes: one row per load instruction (lanes beyond the row idle), SIXTEEN rows
    // in flight — with eight a 768-byte row kept half the bytes of the bf16 kernel's rows in flight
    // and the pass was no faster than reading the bf16 rows themselves (C5: 82 against 68 ms)
    constexpr int RF = 16;
    const bool on = lane < lpr;
    uint4 hv = uint4{0u, 0u, 0u, 0u}, lv = hv;
    if (on) {
      hv = reinterpret_cast<const uint4*>(planes)[lane];
      lv = reinterpret_cast<const uint4*>(planes + nw)[lane];
    }
    const unsigned int hw[4] = {hv.x, hv.y, hv.z, hv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
    for (int i0 = first + slot * RF; i0 < fill; i0 += nslots * RF) {
      uint4 x[RF];
#pragma unroll
      for (int u = 0; u < RF; ++u) {
        x[u] = uint4{0u, 0u, 0u, 0u};
        if (on) x[u] = *reinterpret_cast<const uint4*>(X8 + (int64_t)cid[i0 + u < fill ? i0 + u : i0] * d + lane * 16);
      }
#pragma unroll
      for (int u = 0; u < RF; ++u) {
        const unsigned int xw[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
        unsigned int a = 0, b = 0, cc = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          a = __builtin_amdgcn_udot4(xw[w], hw[w], a, false);
          b = __builtin_amdgcn_udot4(xw[w], lw[w], b, false);
          cc = __builtin_amdgcn_udot4(xw[w], xw[w], cc, false);
        }
        for (int o = 32; o > 0; o >>= 1) {
          a += __shfl_xor(a, o);
          b += __shfl_xor(b, o);
          cc += __shfl_xor(cc, o);
        }
        if (lane == 0 && i0 + u < fill)
          cdist[i0 + u] = (TO)(65536.0 * (double)cc - 131072.0 * (double)a - 512.0 * (double)b + kq);
      }
    }
    return;
  }
  // longer rows: one row per load instruction and 1024-byte piece, eight rows in flight
  for (int i0 = first + slot * 8; i0 < fill; i0 += nslots * 8) {
    unsigned int a[8], b[8], cc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = b[u] = cc[u] = 0;
    for (int p = lane; p < lpr; p += 64) {
      const uint4 hv = reinterpret_cast<const uint4*>(planes)[p];
      const uint4 lv = reinterpret_cast<const uint4*>(planes + nw)[p];
      const unsigned int hw[4] = {hv.x, hv.y, hv.z, hv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
      uint4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        x[u] = *reinterpret_cast<const uint4*>(X8 + (int64_t)cid[i0 + u < fill ? i0 + u : i0] * d + p * 16);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const unsigned int xw[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          a[u] = __builtin_amdgcn_udot4(xw[w], hw[w], a[u], false);
          b[u] = __builtin_amdgcn_udot4(xw[w], lw[w], b[u], false);
          cc[u] = __builtin_amdgcn_udot4(xw[w], xw[w], cc[u], false);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      unsigned int ta = a[u], tb = b[u], tc = cc[u];
      for (int o = 32; o > 0; o >>= 1) {
        ta += __shfl_xor(ta, o);
        tb += __shfl_xor(tb, o);
        tc += __shfl_xor(tc, o);
      }
      if (lane == 0 && i0 + u < fill)
        cdist[i0 + u] = (TO)(65536.0 * (double)tc - 131072.0 * (double)ta - 512.0 * (double)tb + kq);
    }
  }
}

// CSR data for the fused kernel (SVector rows, Internal.hs:92-93): data rows and query rows
struct CsrPtrs {
  const int64_t* rowptr;
  const int32_t* col;
  const void* val;
  int64_t nnz;
  const int64_t* qrowptr;
  const int32_t* qcol;
  const void* qval;
  // f32 prefilter (f64 rows, d <= 65536): the rows again as (u16 column, f32 value), 6 instead of
  // 12 bytes per nonzero; the longest row (bounds the f32 summation chains)
  const uint16_t* col16;
  const float* val32;
  int64_t max_rowlen;
  // half tier: the rows as a fixed-width table of (u16 column | half value << 16) slots
  const uint32_t* ell;
  int ell_w;
};

// Squared-distance sums of U CSR rows per 16-lane group against the dense-ified query qs (LDS):
// s[u] = sum over the row's nonzeros of ((x_j - q_j)^2 - q_j^2); the true Euclidean distance is
// sqrt(|q|^2 + s).  Lane l of the group takes the nonzeros ra + 64 t + 4 l .. + 3 for t = 0, 1, ..
// with one 16-byte column load and one 16/32-byte value load (4-byte aligned addresses), sums
// them in index order and the group adds its sixteen partial sums by a fixed butterfly: a
// row's value does not depend on the kernel or the slot it is computed in (the fused kernel and
// the general path call this same function).  All loads of a step — U rows — are issued before
// the first is used: the walk of a row is a chain of dependent loads (id -> rowptr -> col / val
// -> qs[col]), and issuing them row by row left the kernels latency-bound (C3: 2.2 TB/s).
// DOT: the term is the product x_j q_j instead (the lane-parallel dot of knn_metric_csr_kernel).
template <class TD, int U, bool DOT = false>
__device__ __forceinline__ void csr_rows_dist2(const int32_t* __restrict__ col,
                                               const TD* __restrict__ val, int64_t nnz,
                                               const int64_t (&ra)[U], const int64_t (&rb)[U],
                                               const double* qs, int l16, double (&s)[U]) {
  struct __attribute__((packed, aligned(4))) C4 { int v[4]; };
  struct __attribute__((packed, aligned(4))) V4 { TD v[4]; };
#pragma unroll
  for (int u = 0; u < U; ++u) s[u] = 0.0;
  for (int64_t t = 4 * l16;; t += 64) {
    C4 c[U];
    V4 v[U];
    bool more = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = ra[u] + t;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c[u].v[e] = 0;
        v[u].v[e] = (TD)0;
      }
      if (j < rb[u]) {
        if (j + 4 <= nnz) {  // may run past the row's end (masked below), never past the arrays'
          c[u] = *reinterpret_cast<const C4*>(col + j);
          v[u] = *reinterpret_cast<const V4*>(val + j);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j + e < rb[u]) {
              c[u].v[e] = col[j + e];
              v[u].v[e] = val[j + e];
            }
        }
      }
      more = more || j + 64 < rb[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = ra[u] + t;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = j + e < rb[u];
        const double qj = qs[ok ? c[u].v[e] : 0];
        if constexpr (DOT) {
          const double term = (double)v[u].v[e] * qj;
          s[u] += ok ? term : 0.0;
        } else {
          const double df = (double)v[u].v[e] - qj;
          const double term = df * df - qj * qj;
          s[u] += ok ? term : 0.0;
        }
      }
    }
    if (!__any(more)) break;
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    for (int o = 8; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o);  // fixed butterfly inside the group
}

// distances of the CSR candidates [first, fill) of an LDS batch: sixteen rows of a wave in flight
// (four row slots per 16-lane group)
template <class TD, bool DOT = false /* cdist: the rows' lane-parallel dots with qs, qn2 unused */>
__device__ __forceinline__ void batch_distances_csr(const int64_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col,
                                                    const TD* __restrict__ val, int64_t nnz,
                                                    const int* cid, double* cdist, const double* qs,
                                                    double qn2, int first, int fill, int wave,
                                                    int lane) {
  constexpr int U = 4;
  const int grp = lane >> 4, l16 = lane & 15;
  for (int i0 = first + wave * 4 * U; i0 < fill; i0 += 4 * 4 * U) {
    int64_t ra[U], rb[U];
    double s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * 4 + grp;
      const bool ok = i < fill;
      const int id = cid[ok ? i : first];
      ra[u] = rowptr[id];
      rb[u] = ok ? rowptr[id + 1] : ra[u];
    }
    csr_rows_dist2<TD, U, DOT>(col, val, nnz, ra, rb, qs, l16, s);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double t = s[u] + qn2;
      const int i = i0 + u * 4 + grp;
      if constexpr (DOT) {
        if (l16 == 0 && i < fill) cdist[i] = s[u];
      } else if (l16 == 0 && i < fill) cdist[i] = sqrt(t > 0 ? t : 0.0);
    }
  }
}

// The same walk over the (u16 column, f32 value) shadow of the rows, in f32 arithmetic: the
// RANKING pass of the CSR prefilter (knn_fused_kernel<.., PRE32, CSR>).  No FMA contraction in
// this translation unit: the error bound of the refine step counts one rounding per operation.
template <int U>
__device__ __forceinline__ void csr_rows_dist2_f32(const uint16_t* __restrict__ col16,
                                                   const float* __restrict__ val32, int64_t nnz,
                                                   const int64_t (&ra)[U], const int64_t (&rb)[U],
                                                   const float* qs32, int l16, float (&s)[U]) {
  struct __attribute__((packed, aligned(2))) C4 { uint16_t v[4]; };
  struct __attribute__((packed, aligned(4))) V4 { float v[4]; };
#pragma unroll
  for (int u = 0; u < U; ++u) s[u] = 0.f;
  for (int64_t t = 4 * l16;; t += 64) {
    C4 c[U];
    V4 v[U];
    bool more = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = ra[u] + t;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c[u].v[e] = 0;
        v[u].v[e] = 0.f;
      }
      if (j < rb[u]) {
        if (j + 4 <= nnz) {
          c[u] = *reinterpret_cast<const C4*>(col16 + j);
          v[u] = *reinterpret_cast<const V4*>(val32 + j);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j + e < rb[u]) {
              c[u].v[e] = col16[j + e];
              v[u].v[e] = val32[j + e];
            }
        }
      }
      more = more || j + 64 < rb[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = ra[u] + t;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = j + e < rb[u];
        const float qj = qs32[ok ? (int)c[u].v[e] : 0];
        const float df = v[u].v[e] - qj;
        const float term = df * df - qj * qj;
        s[u] += ok ? term : 0.f;
      }
    }
    if (!__any(more)) break;
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    for (int o = 8; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o);
}

// f32 SQUARED distances (clamped at 0) of the CSR candidates [first, fill) from the shadow
__device__ __forceinline__ void batch_distances_csr32(const int64_t* __restrict__ rowptr,
                                                      const uint16_t* __restrict__ col16,
                                                      const float* __restrict__ val32, int64_t nnz,
                                                      const int* cid, double* cdist,
                                                      const float* qs32, float qn2, int first,
                                                      int fill, int wave, int lane) {
  constexpr int U = 4;
  const int grp = lane >> 4, l16 = lane & 15;
  for (int i0 = first + wave * 4 * U; i0 < fill; i0 += 4 * 4 * U) {
    int64_t ra[U], rb[U];
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * 4 + grp;
      const bool ok = i < fill;
      const int id = cid[ok ? i : first];
      ra[u] = rowptr[id];
      rb[u] = ok ? rowptr[id + 1] : ra[u];
    }
    csr_rows_dist2_f32<U>(col16, val32, nnz, ra, rb, qs32, l16, s);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float t = qn2 + s[u];
      const int i = i0 + u * 4 + grp;
      if (l16 == 0 && i < fill) cdist[i] = (double)(t > 0.f ? t : 0.f);
    }
  }
}

// f32 SQUARED distances (clamped at 0) of the CSR candidates [first, fill) from the fixed-width
// half shadow (rpt_dataset::shadow_ell): row id -> id * W slots, no rowptr step; sixteen lanes
// per row, a lane takes the 16-byte chunks l16, l16 + 16, .. (four slots each), the chunks of all
// four row slots of the group and of up to four steps are loaded before the first is used (W <=
// 256: ONE round of loads per sixteen rows of the wave).  A slot adds x (x - 2 q_col) = (x - q)^2
// - q^2 with two roundings (explicit FMAs); an absent slot (column 0, x = 0) adds 0.
__device__ __forceinline__ void batch_distances_ell16(const uint32_t* __restrict__ ell, int W,
                                                      const int* cid, double* cdist,
                                                      const float* qs32, float qn2, int first,
                                                      int fill, int wave, int lane) {
  constexpr int U = 4, S = 4;
  const int grp = lane >> 4, l16 = lane & 15;
  const int chunks = W >> 2;
  for (int i0 = first + wave * 4 * U; i0 < fill; i0 += 4 * 4 * U) {
    const uint4* row[U];
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * 4 + grp;
      const int id = cid[i < fill ? i : first];
      row[u] = reinterpret_cast<const uint4*>(ell + (int64_t)id * W);
      s[u] = 0.f;
    }
    for (int c0 = 0; c0 < chunks; c0 += 16 * S) {
      uint4 v[U][S];
#pragma unroll
      for (int st = 0; st < S; ++st) {
        const int c = c0 + st * 16 + l16;
#pragma unroll
        for (int u = 0; u < U; ++u) v[u][st] = c < chunks ? row[u][c] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int st = 0; st < S; ++st) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const unsigned int w4[4] = {v[u][st].x, v[u][st].y, v[u][st].z, v[u][st].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const unsigned short hb = (unsigned short)(w4[e] >> 16);
            _Float16 h;
            __builtin_memcpy(&h, &hb, 2);
            const float x = (float)h;
            const float qj = qs32[w4[e] & 0xffffu];
            s[u] = __builtin_fmaf(x, __builtin_fmaf(-2.f, qj, x), s[u]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      for (int o = 8; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o);
      const float t = qn2 + s[u];
      const int i = i0 + u * 4 + grp;
      if (l16 == 0 && i < fill) cdist[i] = (double)(t > 0.f ? t : 0.f);
    }
  }
}

// ---------------------------------------------------------------------------------------
// fused query kernel (dense data): one workgroup per query does everything after the query
// projections — traversal of every tree (thread = tree, twice: count, then emit ranges in
// tree order), candidate ids gathered into LDS, distances (each wave keeps EIGHT whole rows in
// flight, 16-byte loads, butterfly reduction), top-k.  No global scan, no range list in HBM.
// Batches of kFC candidates; the running best k re-enter the next batch at the front with
// their original candidate positions, so the order (distance, position) is global.
// k <= kFK: k rounds of block-wide arg-min; larger k or a range list that does not fit the
// LDS slab -> the query is flagged and the host falls back to the general path.
// (kFC, kFR, kFK, kBK, kVoteCap: knn_plan.h)
// ---------------------------------------------------------------------------------------
#ifndef RPT_CONSEC_FILL
#define RPT_CONSEC_FILL 0
#endif
constexpr bool kConsecFill = RPT_CONSEC_FILL != 0;  // consecutive-slot fill in the non-WIDE instantiations too
constexpr int kSelList = 512;  // select_packed's candidate list (in the idle distance slab)

template <class TD, class TK, bool PRE32, bool CSR = false, bool I8 = false /* PRE32 on the int8 shadow */>
// (three workgroups per CU is what the 52 KB slab allows: keep the registers at that occupancy)
__global__ __launch_bounds__(256, 3) void knn_fused_kernel(
    const TD* __restrict__ X, int d, const TD* __restrict__ Q, const int32_t* __restrict__ perm,
    const double* __restrict__ thr, const double* __restrict__ mglo,
    const double* __restrict__ mghi, int64_t nodes, const TK* __restrict__ Pq, int64_t nq, int T,
    int L, int min_leaf, int64_t N, int k, int dedup_vote /* duplicate rule | vote threshold << 8 */,
    int32_t* __restrict__ out_ids,
    double* __restrict__ out_dist, int32_t* __restrict__ out_cnt, unsigned int* ovf_flags,
    unsigned int* ovf_count, unsigned long long* cand_total,
    const void* __restrict__ Xf /* PRE32: f32 (or, sh16, IEEE half) shadow of X */,
    double xmax /* max row norm */,
    int k1 /* PRE32: entries kept by the shadow pass, the last one = the first excluded */,
    CsrPtrs csr /* CSR: X / Q are null, rows and queries are SVectors */, int sh16 = 0,
    Sh8 sh8 = Sh8{0.0, 0.0} /* s > 0: Xf is the int8 shadow (see Sh8) */,
    unsigned long long* dbg = nullptr /* debug_stamps: phase clocks of one workgroup */) {
  int dbgi = 0;
#define KSTAMP() do { if (dbg && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0 && dbgi < 60) dbg[dbgi++] = clock64(); } while (0)
  KSTAMP();
  typedef typename AccOf<TD>::type TA;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // Dense prefilter instantiations (round 3): the batch values are f32 (what their packed keys hold
  // anyway) and a candidate's position is computed, not stored, so the same 32 KB hold TWICE the
  // candidates — C2's 3922 per query in ONE batch: one fill, one selection.
  constexpr bool WIDE = PRE32 && !CSR;
  constexpr int FC = WIDE ? 2 * kFC : kFC;   // candidates per batch
  typedef typename std::conditional<WIDE, float, double>::type TB;
  TB* cval = reinterpret_cast<TB*>(smem);                          // [FC] batch values
  double* cdist = reinterpret_cast<double*>(smem);                 // the same slab as doubles: [kFC]
                                                                   // (exact paths, refine, slots, lists)
  int* cid = reinterpret_cast<int*>(cdist + kFC);                  // [FC] (WIDE) / [kFC]
  int* cpos = WIDE ? cid + 1024 : cid + kFC;                       // [kFC]; WIDE: only the refine
                                                                   // stage's <= kBKx positions
  int64_t* rpoff = reinterpret_cast<int64_t*>(cid + 2 * kFC);      // [kFR]
  int* rn = reinterpret_cast<int*>(rpoff + kFR);                   // [kFR]
  int* tcnt = rn + kFR;                                            // [1024] per-tree counts
  int* trng = tcnt + 1024;                                         // [1024]
  double* bdist = reinterpret_cast<double*>(trng + 1024);          // [kBKx]
  int* bid = reinterpret_cast<int*>(bdist + kBKx);                 // [kBKx]
  int* bpos = bid + kBKx;                                          // [kBKx]
  TA* qs = reinterpret_cast<TA*>(bpos + kBKx);                     // [d]
  float* qs32 = reinterpret_cast<float*>(qs + d);                  // [d] (PRE32)
  // voting mode (dedup_vote >> 8 = v > 0, RPTree.hs:464-478 counts / keepCounts): all candidate
  // ids of the query, sorted, so that the ids found in at least v trees can be picked out
  int* vid = reinterpret_cast<int*>(
      (reinterpret_cast<uintptr_t>(qs32 + d) + 15) & ~(uintptr_t)15);  // [kVoteCap]
  __shared__ int s_nr, s_nc;
  __shared__ double s_qn;
  __shared__ int s_fw;         // finalize_leftfold: entries written ...
  __shared__ double s_flast;   // ... and the last of them (the certificate of the f64 L2 cut)
  __shared__ double s_red_d[8];
  __shared__ int s_red_p[8], s_red_i[8];
  __shared__ int s_wk[4];
  __shared__ double s_q8e[4], s_q8k[4];  // int8 tier: the waves' shares of eq^2 and of K (see Sh8)
  __shared__ unsigned int s_mm[4], s_lcnt;  // select_packed: the waves' thresholds, the list length
  const int vote = PRE32 ? 0 : (dedup_vote >> 8);
  const int dedup = vote > 0 ? 0 : (dedup_vote & 3);  // kept ids are distinct

  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool rerun = !PRE32 && k1 == -1;  // second pass: only the queries the prefilter gave up on
  if (rerun && ovf_flags[q] != 2u) return;
  // f32 / bf16 data with duplicates kept: the distances are f32 values, so the squared distance is
  // ranked through the packed key as well and the root is taken once, on output (same bits)
  const bool pack32 = !PRE32 && !CSR && sizeof(TA) == 4 && dedup == 0;
  double* qsd = reinterpret_cast<double*>(qs);  // CSR: the dense-ified query, d doubles (the
                                                // slab holds d * (sizeof(TA) + 4) >= 8 d bytes)
  if constexpr (CSR) {
    for (int j = tid; j < d; j += 256) qsd[j] = 0.0;
    __syncthreads();
    const TD* qv = static_cast<const TD*>(csr.qval);
    for (int64_t j = csr.qrowptr[q] + tid; j < csr.qrowptr[q + 1]; j += 256)
      qsd[csr.qcol[j]] = (double)qv[j];
    __syncthreads();
    if (PRE32)  // the slab holds d * 12 bytes: d doubles, then d floats
      for (int j = tid; j < d; j += 256) reinterpret_cast<float*>(qsd + d)[j] = (float)qsd[j];
    if (wave == 0) {
      double sq = 0.0;
      for (int j = lane; j < d; j += 64) sq += qsd[j] * qsd[j];
      sq = wave_sum(sq);
      if (lane == 0) s_qn = sq;  // |q|^2 (the dense variants keep |q| here, PRE32 only)
    }
  } else {
    for (int j = tid; j < d; j += 256) qs[j] = ld<TD>(Q + q * d + j);
    if constexpr (I8) {  // int8 tier: the quantised query's byte planes in the f32 copy's place
      __syncthreads();
      double kqp, e2p;
      if constexpr (sizeof(TA) == 8)
        quantise_query(reinterpret_cast<const double*>(qs), nullptr, d, sh8.s,
                       reinterpret_cast<unsigned int*>(qs32), tid, 256, kqp, e2p);
      else
        quantise_query(nullptr, reinterpret_cast<const float*>(qs), d, sh8.s,
                       reinterpret_cast<unsigned int*>(qs32), tid, 256, kqp, e2p);
      for (int o = 32; o > 0; o >>= 1) {
        kqp += __shfl_xor(kqp, o);  // integer-valued doubles below 2^53: exact in any order
        e2p += __shfl_xor(e2p, o);
      }
      if (lane == 0) {
        s_q8k[wave] = kqp;
        s_q8e[wave] = e2p;
      }
    } else if (PRE32)
      for (int j = tid; j < d; j += 256) qs32[j] = (float)ld<TD>(Q + q * d + j);
  }

  // ---- traversal: ONE pass in the usual case.  Thread = tree; the leaf ranges a tree reaches go
  // to its S slots (in the batch slab, idle until the first fill) and are counted in any case;
  // after the scan over the trees they are compacted in tree order.  A tree that outgrows its
  // slots (or T > kFR) sends the workgroup through the second, emitting traversal.  (Round 3: two
  // traversals of 13 dependent node loads each were a fifth of a C2 query's life.) ----
  const int S = T <= kFR ? kFR / T : 0;
  int64_t* spoff = reinterpret_cast<int64_t*>(cdist);  // [kFR]
  int* sn = reinterpret_cast<int*>(cdist + kFR);       // [kFR]
  int slots_short = 0;
  for (int t = tid; t < T; t += 256) {
    int nc = 0, nr = 0;
    traverse<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, Pq + (int64_t)t * L * nq + q,
                 nq, L, min_leaf, N, [&](int off, int n) {
                   if (nr < S) {
                     spoff[t * S + nr] = (int64_t)t * N + off;
                     sn[t * S + nr] = n;
                   }
                   nc += n;
                   ++nr;
                 });
    tcnt[t] = nc;
    trng[t] = nr;
    slots_short |= nr > S;
  }
  const int second_pass = __syncthreads_or(slots_short);
  if (tid == 0) {  // exclusive scans over <= 1024 trees
    int c = 0, r = 0;
    for (int t = 0; t < T; ++t) {
      const int a = tcnt[t], b = trng[t];
      tcnt[t] = c;
      trng[t] = r;
      c += a;
      r += b;
    }
    s_nc = c;
    s_nr = r;
  }
  __syncthreads();
  KSTAMP();  // 1: query + traversal + scan
  const int nr_tot = s_nr, nc_tot = s_nc;
  constexpr bool i8 = I8;
  static_assert(!I8 || (PRE32 && !CSR), "the int8 tier is a dense prefilter");
  const double q8k = i8 ? s_q8k[0] + s_q8k[1] + s_q8k[2] + s_q8k[3] - 1073741824.0 * (double)d : 0.0;
  const double q8eq = i8 ? sqrt(s_q8e[0] + s_q8e[1] + s_q8e[2] + s_q8e[3]) : 0.0;
  if (nr_tot > kFR) {  // too many leaf ranges for the slab: general path
    if (tid == 0) {
      ovf_flags[q] = 1u;
      atomicAdd(ovf_count, 1u);
    }
    return;
  }
  if (tid == 0 && !rerun) atomicAdd(cand_total, (unsigned long long)nc_tot);
  // ---- ranges in tree order + rstart[r] = candidates before range r (the batches are filled by
  // position: a binary search over rstart, every load of a batch in flight at once).  rstart takes
  // tcnt's place: a thread reads its trees' scan values before anyone overwrites them ----
  int* rstart = tcnt;  // [nr_tot + 1] <= kFR + 1
  {
    int r0[4], r1[4], c0[4];  // T <= 1024: at most four trees per thread
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = tid + 256 * u;
      r0[u] = t < T ? trng[t] : 0;
      r1[u] = t < T ? (t + 1 < T ? trng[t + 1] : nr_tot) : 0;
      c0[u] = t < T ? tcnt[t] : 0;
    }
    __syncthreads();
    for (int u = 0; u < 4; ++u) {
      const int t = tid + 256 * u;
      if (t >= T) break;
      int r = r0[u], c = c0[u];
      if (!second_pass) {
        for (int i2 = 0; r < r1[u]; ++i2, ++r) {
          const int n = sn[t * S + i2];
          rpoff[r] = spoff[t * S + i2];
          rn[r] = n;
          rstart[r] = c;
          c += n;
        }
      } else {
        traverse<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, Pq + (int64_t)t * L * nq + q,
                     nq, L, min_leaf, N, [&](int off, int n) {
                       rpoff[r] = (int64_t)t * N + off;
                       rn[r] = n;
                       rstart[r] = c;
                       c += n;
                       ++r;
                     });
      }
    }
    if (tid == 0) rstart[nr_tot] = nc_tot;
  }
  __syncthreads();

  // ---- voting mode: every candidate id into LDS, ascending (the order of M.foldrWithKey in
  // keepCounts); an id found in c trees is a run of c equal entries ----
  if (vote > 0) {
    if (nc_tot > kVoteCap) {  // more candidates than the slab counts: reported, not answered
      if (tid == 0) {
        ovf_flags[q] = 3u;
        atomicAdd(ovf_count, 1u);
      }
      return;
    }
    int pos = 0;
    for (int r = 0; r < nr_tot; ++r) {  // every thread walks the same range list
      const int n = rn[r];
      for (int i = tid; i < n; i += 256) vid[pos + i] = perm[rpoff[r] + i];
      pos += n;
    }
    int np = 1;
    while (np < nc_tot) np <<= 1;
    for (int i = nc_tot + tid; i < np; i += 256) vid[i] = 0x7fffffff;
    __syncthreads();
    for (int kk = 2; kk <= np; kk <<= 1)
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < (np >> 1); i += 256) {
          const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
          const bool up = (lo & kk) == 0;
          const int a = vid[lo], b = vid[hi];
          if (up ? b < a : a < b) {
            vid[lo] = b;
            vid[hi] = a;
          }
        }
        __syncthreads();
      }
  }
  int vsrc = 0;  // voting mode: next entry of vid to look at

  // ---- selection: ksel rounds of block-wide arg-min by (distance, position) over the batch
  // entries [0, fill); the winners go to bdist / bid / bpos.  A thread keeps its eight entries
  // in registers (a consumed one gets position -1), a round costs one arg-min over them, a
  // butterfly, four LDS words and ONE barrier (the per-wave results alternate between two
  // buffers) ----
  // The f32 pass ranks SQUARED f32 distances (exact float values): (value bits << 32 | position)
  // is one 64-bit key whose unsigned order is the (distance, position) order — half the
  // cross-lane traffic per round, and the owner of the winner writes it out itself.
  // Round 3: the ksel rounds are WAVE-local (shuffles only, no LDS, no barrier): every wave takes
  // the ksel smallest of its own quarter of the batch, the four lists meet in LDS and the ksel
  // smallest of those 4 x ksel keys — the batch's ksel smallest are among them — are ranked by
  // counting.  Two barriers per batch instead of one per round (C2: 17 rounds per 2048 entries).
  // Round 3 (late): the ksel smallest through a THRESHOLD instead of ksel rounds.  The value half of
  // a key is the bit pattern of a non-negative float, monotone as an unsigned integer.  An upper
  // bound tau of the ksel-th smallest value: once a full list exists, the value of its last entry
  // (the list sits at the front of the batch); before that, every wave takes the ceil(ksel / 4)-th
  // smallest of its 64 per-thread minima (ranked by counting over lane reads) and tau is the largest
  // of the four — at least ksel entries lie at or below it.  The entries <= tau (ksel plus a few)
  // are compacted into a list and ranked by counting on the full keys: three barriers per batch
  // whatever ksel is (the rounds cost 0.03 ms per kept entry and 10 000 queries at C2).  A list of
  // more than 256 entries (values tied by the hundred) falls back to the rounds.
  auto select_packed = [&](int fill, int ksel, int have /* entries of a list from earlier batches */,
                           int pb0 /* WIDE: position of the batch's first NEW candidate */) -> int {
    constexpr int E = FC / 256;
    unsigned long long key[E];
    unsigned int vmin = ~0u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = tid + 256 * e;
      unsigned int pos;
      if constexpr (WIDE) pos = (unsigned int)(i < have ? bpos[i < kBKx ? i : 0] : pb0 + (i - have));
      else pos = (unsigned int)cpos[i < kFC ? i : 0];
      key[e] = i < fill ? ((unsigned long long)__float_as_uint((float)cval[i]) << 32) | pos : ~0ULL;
      const unsigned int v = (unsigned int)(key[e] >> 32);
      if (i < fill) vmin = v < vmin ? v : vmin;
    }
    unsigned int tau;
    if (have == ksel) {
      tau = __float_as_uint((float)bdist[ksel - 1]);
    } else {
      const int r = (ksel + 3) / 4;
      int cnt = 0;
#pragma unroll
      for (int j2 = 0; j2 < 64; ++j2) {  // (constant lane: v_readlane, not an LDS permute)
        const unsigned int o = (unsigned int)__builtin_amdgcn_readlane((int)vmin, j2);
        cnt += (o < vmin || (o == vmin && j2 < lane)) ? 1 : 0;
      }
      const unsigned long long hit = __ballot(cnt == r - 1);
      tau = __shfl(vmin, __ffsll((long long)hit) - 1);  // ~0u when the wave holds fewer than r entries
      if (lane == 0) s_mm[wave] = tau;
    }
    if (tid == 0) s_lcnt = 0u;
    KSTAMP();  // sel: keys + threshold
    __syncthreads();  // (every thread has read its cdist entries: the list below reuses that slab)
    KSTAMP();  // sel: barrier
    if (have != ksel) {
      tau = s_mm[0];
#pragma unroll
      for (int w = 1; w < 4; ++w) tau = s_mm[w] > tau ? s_mm[w] : tau;
    }
    unsigned long long* lkey = reinterpret_cast<unsigned long long*>(cdist);  // [kSelList]
    int* lidx = reinterpret_cast<int*>(cdist + kSelList);                      // [kSelList]
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (key[e] != ~0ULL && (unsigned int)(key[e] >> 32) <= tau) {
        const unsigned int slot = atomicAdd(&s_lcnt, 1u);
        if (slot < (unsigned int)kSelList) {
          lkey[slot] = key[e];
          lidx[slot] = tid + 256 * e;
        }
      }
    KSTAMP();  // sel: compaction
    __syncthreads();
    KSTAMP();  // sel: barrier
    const int n = (int)s_lcnt;
    if (n <= kSelList) {
      for (int t2 = tid; t2 < n; t2 += 256) {
        const unsigned long long mine = lkey[t2];
        const int rank = count_below(lkey, n, mine);
        if (rank < ksel) {
          bdist[rank] = (double)__uint_as_float((unsigned int)(mine >> 32));
          bid[rank] = cid[lidx[t2]];
          bpos[rank] = (int)(unsigned int)mine;
        }
      }
      __syncthreads();
      return n < ksel ? n : ksel;
    }
    // (the winners' lists of the fallback live in the same idle slab: 4 x kBKx keys, then ids)
    unsigned long long (*wb_key)[kBKx] = reinterpret_cast<unsigned long long (*)[kBKx]>(cdist);
    int (*wb_id)[kBKx] = reinterpret_cast<int (*)[kBKx]>(cdist + 4 * kBKx);
    // ---- fallback: ksel wave-local rounds, the four lists merged by rank counting ----
    for (int r = 0; r < ksel; ++r) {
      unsigned long long m = key[0];
#pragma unroll
      for (int e = 1; e < E; ++e) m = key[e] < m ? key[e] : m;
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t2 = __shfl_xor(m, o);
        m = t2 < m ? t2 : m;
      }
      if (m == ~0ULL) {  // this wave's entries are exhausted (wave-uniform)
        if (lane == 0)
          for (int r2 = r; r2 < ksel; ++r2) wb_key[wave][r2] = ~0ULL;
        break;
      }
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (key[e] == m) {  // keys are unique (positions are): exactly one owner
          key[e] = ~0ULL;
          wb_key[wave][r] = m;
          wb_id[wave][r] = cid[tid + 256 * e];
        }
    }
    __syncthreads();
    const int tot = 4 * ksel;
    int myvalid = 0;
    for (int t2 = tid; t2 < tot; t2 += 256) {
      const unsigned long long mine = wb_key[t2 / ksel][t2 % ksel];
      if (mine == ~0ULL) continue;
      ++myvalid;
      int rank = 0;
      for (int w = 0; w < 4; ++w)
        for (int r = 0; r < ksel; ++r) rank += wb_key[w][r] < mine;
      if (rank < ksel) {
        bdist[rank] = (double)__uint_as_float((unsigned int)(mine >> 32));
        bid[rank] = wb_id[t2 / ksel][t2 % ksel];
        bpos[rank] = (int)(unsigned int)mine;
      }
    }
    // entries in all = the valid keys of the four lists, at most ksel are kept
    for (int o = 32; o > 0; o >>= 1) myvalid += __shfl_xor(myvalid, o);
    if (lane == 0) s_mm[wave] = (unsigned int)myvalid;
    __syncthreads();
    const int nvalid = (int)(s_mm[0] + s_mm[1] + s_mm[2] + s_mm[3]);
    __syncthreads();  // s_mm is the next batch's threshold exchange
    return nvalid < ksel ? nvalid : ksel;
  };
  // kdist > 0 (dense f64 rows, see kLfMargin): keep the entries of the best kdist DIFFERENT ids, at
  // most ksel entries; l2cut is set when a candidate is left out for that (a same-id copy under a
  // duplicate rule is not one; a full list counts as a cut: the batch may hold more)
  bool l2cut = false;
  auto select = [&](int fill, int ksel, int dedup, int kdist) -> int {
    constexpr int E = kFC / 256;
    double dd[E];
    int pp[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = tid + 256 * e;
      dd[e] = i < fill ? cdist[i] : __longlong_as_double(0x7ff0000000000000LL);
      // NaN (a NaN query or row, inf - inf) ranks with +inf, by position: a total order, every entry
      // can be selected (a NaN would lose every comparison and end the rounds with nothing chosen)
      if (dd[e] != dd[e]) dd[e] = __longlong_as_double(0x7ff0000000000000LL);
      pp[e] = i < fill ? cpos[i] : -1;
    }
    int nb = 0, par = 0, nd = 0;
    double last_d = -1.0;
    while (nb < ksel) {
      double bd = __longlong_as_double(0x7ff0000000000000LL);
      int bp = 0x7fffffff, bi = -1;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (pp[e] >= 0 && (dd[e] < bd || (dd[e] == bd && pp[e] < bp))) {
          bd = dd[e];
          bp = pp[e];
          bi = tid + 256 * e;
        }
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o);
        const int op = __shfl_xor(bp, o), oi = __shfl_xor(bi, o);
        if (od < bd || (od == bd && op < bp)) {
          bd = od;
          bp = op;
          bi = oi;
        }
      }
      if (lane == 0) {
        s_red_d[par * 4 + wave] = bd;
        s_red_p[par * 4 + wave] = bp;
        s_red_i[par * 4 + wave] = bi;
      }
      __syncthreads();
      bd = s_red_d[par * 4];
      bp = s_red_p[par * 4];
      bi = s_red_i[par * 4];
      for (int w = 1; w < 4; ++w)
        if (s_red_d[par * 4 + w] < bd || (s_red_d[par * 4 + w] == bd && s_red_p[par * 4 + w] < bp)) {
          bd = s_red_d[par * 4 + w];
          bp = s_red_p[par * 4 + w];
          bi = s_red_i[par * 4 + w];
        }
      par ^= 1;
      if (bi < 0) break;  // candidates exhausted
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (bi == tid + 256 * e) pp[e] = -1;  // consumed
      bool keep = true, copy = false;
      if (dedup == 2 && nb > 0 && bd == last_d) keep = false;  // knnPQ: one per distance
      else if ((dedup || kdist > 0) && bd == last_d)  // same id => same distance: duplicates are among equal dist
        for (int j = nb - 1; j >= 0 && bdist[j] == bd; --j)
          if (bid[j] == cid[bi]) copy = true;
      if (dedup && copy) keep = false;
      if (keep && kdist > 0 && !copy) {
        if (nd == kdist) {  // one different id more than the kept set holds (uniform)
          l2cut = true;
          break;
        }
        ++nd;
      }
      if (keep) {
        if (tid == 0) {
          bdist[nb] = bd;
          bid[nb] = cid[bi];
          bpos[nb] = bp;
        }
        ++nb;
        last_d = bd;
      }
    }
    if (kdist > 0 && nb == ksel) l2cut = true;
    __syncthreads();  // the winners are visible; cdist / cid / cpos may be refilled
    return nb;
  };

  // A dense prefilter cut that cannot be certified is tried ONCE more, by the same workgroup, with
  // three times the kept entries (the other workgroups keep the chip busy meanwhile); only then is
  // the query left to the host's second launch of the exact kernel (two such queries of C2's 10 000
  // cost that launch 0.4 ms: they run alone on an empty chip)
  const int k1_retry = (PRE32 && !CSR) ? (3 * k1 < kBK ? 3 * k1 : kBK) : k1;
retry_wider:
  int best = 0;       // entries of the running best list
  int pos_base = 0;   // candidate position of the next unconsumed candidate
  while ((vote > 0 ? vsrc < nc_tot : pos_base < nc_tot) || best == 0) {
    // ---- fill the batch: best list first (keeps its positions), then new candidates ----
    for (int i = tid; i < best; i += 256) {
      cval[i] = (TB)bdist[i];
      cid[i] = bid[i];
      if constexpr (!WIDE) cpos[i] = bpos[i];
    }
    int fill = best;
    const int first_new = fill;
    const int pb0 = pos_base;
    // voting mode: the heads of the runs of at least `vote` equal ids, 256 entries of vid per
    // round, compacted into the batch with their index in vid as position (ascending id order)
    while (!WIDE && vote > 0 && vsrc < nc_tot && fill + 256 <= kFC) {
      const int i = vsrc + tid;
      int keep = 0;
      if (i < nc_tot && (i == 0 || vid[i] != vid[i - 1])) {
        int c = 1;
        while (c < vote && i + c < nc_tot && vid[i + c] == vid[i]) ++c;
        keep = c >= vote;
      }
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) s_wk[wave] = __popcll(bal);
      __syncthreads();
      int base = fill;
      for (int w = 0; w < wave; ++w) base += s_wk[w];
      if (keep) {
        const int slot = base + __popcll(bal & ((1ULL << lane) - 1ULL));
        cid[slot] = vid[i];
        cpos[slot] = i;
      }
      fill += s_wk[0] + s_wk[1] + s_wk[2] + s_wk[3];
      vsrc += 256;
      __syncthreads();  // s_wk is rewritten by the next round
    }
    // the batch's new candidates by position: slot s holds candidate pos_base + s, whose range is
    // found by a fixed nine-step search over rstart; a thread's (up to) eight perm loads are all
    // issued before the first is used (walking the ranges one after the other, a dependent global
    // load per range, was a sixth of a C2 query's life)
    if (vote == 0) {
      int take = nc_tot - pos_base;
      if (take > FC - fill) take = FC - fill;
      constexpr int EF = FC / 256;
      // a thread takes EF CONSECUTIVE slots: one search for the first, then a walk along rstart (a
      // leaf range holds ~100 candidates: a boundary or two per thread) — sixteen independent
      // nine-step searches per thread were 13 % of a C2 query's life
      int64_t addr[EF];
      constexpr bool CONSEC = WIDE || kConsecFill;
      if constexpr (!CONSEC) {
#pragma unroll
        for (int e = 0; e < EF; ++e) {
          const int s2 = tid + 256 * e;
          const int c = pos_base + (s2 < take ? s2 : 0);
          int lo = 0;
#pragma unroll
          for (int step = kFR / 2; step > 0; step >>= 1) {
            const int m = lo + step;
            if (m < nr_tot && rstart[m] <= c) lo = m;
          }
          addr[e] = rpoff[lo] + (c - rstart[lo]);
        }
      } else {
        const int s0 = tid * EF;
        const int c0 = pos_base + (s0 < take ? s0 : 0);
        int lo = 0;
#pragma unroll
        for (int step = kFR / 2; step > 0; step >>= 1) {
          const int m = lo + step;
          if (m < nr_tot && rstart[m] <= c0) lo = m;
        }
        int rs = rstart[lo], re = rstart[lo + 1];
        int64_t rbase = rpoff[lo];
#pragma unroll
        for (int e = 0; e < EF; ++e) {
          const int c = c0 + e;
          if (s0 + e < take) {
            while (c >= re) {  // (c < nc_tot = rstart[nr_tot]: ends; empty ranges are stepped over)
              ++lo;
              rs = re;
              re = rstart[lo + 1];
              rbase = rpoff[lo];
            }
          }
          addr[e] = rbase + (c - rs);
        }
      }
      int32_t idv[EF];
#pragma unroll
      for (int e = 0; e < EF; ++e) idv[e] = (CONSEC ? tid * EF + e : tid + 256 * e) < take ? perm[addr[e]] : 0;
#pragma unroll
      for (int e = 0; e < EF; ++e) {
        const int s2 = CONSEC ? tid * EF + e : tid + 256 * e;
        if (s2 < take) {
          cid[fill + s2] = idv[e];
          if constexpr (!WIDE) cpos[fill + s2] = pos_base + s2;
        }
      }
      fill += take;
      pos_base += take;
    }
    __syncthreads();
    KSTAMP();  // batch fill
    // ---- distances of the new candidates ----
    if constexpr (CSR && PRE32) {
      if (sh16)
        batch_distances_ell16(csr.ell, csr.ell_w, cid, cdist, reinterpret_cast<const float*>(qsd + d),
                              (float)s_qn, first_new, fill, wave, lane);
      else
        batch_distances_csr32(csr.rowptr, csr.col16, csr.val32, csr.nnz, cid, cdist,
                              reinterpret_cast<const float*>(qsd + d), (float)s_qn, first_new, fill,
                              wave, lane);
    } else if constexpr (CSR)
      batch_distances_csr<TD>(csr.rowptr, csr.col, static_cast<const TD*>(csr.val), csr.nnz, cid,
                              cdist, qsd, s_qn, first_new, fill, wave, lane);
    else if constexpr (PRE32) {
      if constexpr (I8)  // int8 rows: an eighth of the f64 bytes, integer ranking values
        batch_distances_i8<16, TB>(static_cast<const uint8_t*>(Xf), d, cid, cval,
                                   reinterpret_cast<const unsigned int*>(qs32), q8k, first_new, fill, wave, 4,
                                   lane);
      else if (sh16)  // half rows: a quarter of the f64 bytes (the query stays f32)
        batch_distances<_Float16, float, 16, false, TB>(static_cast<const _Float16*>(Xf), d, cid, cval, qs32,
                                                        first_new, fill, wave, 4, lane);
      else
        batch_distances<float, float, 16, false, TB>(static_cast<const float*>(Xf), d, cid, cval, qs32,
                                                     first_new, fill, wave, 4, lane);
    } else if (pack32)
      batch_distances<TD, TA, (sizeof(TD) < 8 ? 16 : 8), false>(X, d, cid, cdist, qs, first_new, fill, wave, 4, lane);
    else
      batch_distances<TD, TA, (sizeof(TD) < 8 ? 16 : 8)>(X, d, cid, cdist, qs, first_new, fill, wave, 4, lane);
    __syncthreads();
    KSTAMP();  // distances
    // dense f64 rows ranked on butterfly sums keep the entries of k + kLfMargin different ids (see
    // kLfMargin; duplicates kept: as many entries as the list holds): the duplicate rule while
    // streaming is "each id once" (dedup 2 collapses on the FOLD values, in finalize_leftfold).
    // Voting mode: the ids are distinct, the margin is the uncertified one (no exact variant votes).
    constexpr bool L2F64 = !PRE32 && !CSR && std::is_same<TD, double>::value;
    const int kdist = L2F64 && vote == 0 ? k + kLfMargin : 0;
    const int ksel = L2F64 ? (kdist > 0 && dedup == 0 ? kBKx : k + kLfMargin) : k;
    const int nb = PRE32 ? select_packed(fill, k1, best, pb0) : pack32 ? select_packed(fill, k, best, pb0)
                                                                    : select(fill, ksel, kdist > 0 && dedup ? 1 : dedup, kdist);
    best = nb;
    KSTAMP();  // selection
    if (vote > 0 ? vsrc >= nc_tot : pos_base >= nc_tot) break;
  }
  if constexpr (PRE32 && CSR) {
    // ---- refine (CSR): exact distances of the kept entries; certify the cut on SQUARED distances.
    // Error of the f32 squared distance of a row x (u = 2^-24, one rounding per operation, inputs
    // rounded to f32): a term (x_j - q_j)^2 - q_j^2 is off by at most 6.2 u T_j, T_j = (|x_j| +
    // |q_j|)^2 + q_j^2; the sum of n terms, the butterfly and the |q|^2 term pass through chains of
    // at most m = 4 ceil(n / 64) + 5 additions: (m + 1) u (sum T_j + |q|^2); sum T_j <= 2 |x|^2 +
    // 3 |q|^2.  Together E2 <= (m + 8) u (2 xmax^2 + 4 |q|^2) (clamping at 0 only moves the value
    // towards the true one).  Every dropped candidate therefore has an exact squared distance
    // >= F2 - E2, F2 = the smallest dropped f32 value.
    const bool cut = best == k1;
    const double F2 = cut ? bdist[k1 - 1] : 0.0;
    const int m = cut ? k1 - 1 : best;
    for (int i = tid; i < m; i += 256) {
      cid[i] = bid[i];
      cpos[i] = bpos[i];
    }
    __syncthreads();
    batch_distances_csr<TD>(csr.rowptr, csr.col, static_cast<const TD*>(csr.val), csr.nnz, cid,
                            cdist, qsd, s_qn, 0, m, wave, lane);
    __syncthreads();
    best = select(m, k, 0, 0);
    if (cut && best > 0) {
      const double u = 5.9604644775390625e-08;
      const double chain = (double)(4 * ((csr.max_rowlen + 63) / 64) + 5);
      const double E2 = (chain + 8.0) * u * (2.0 * xmax * xmax + 4.0 * s_qn) * 1.01 + 1e-37;
      const double dk = bdist[best - 1];
      bool certified = (s_qn < 1e36) && (F2 < 1e37) && (F2 - E2 > dk * dk * (1.0 + 1e-14));
      if (sh16) {
        // half shadow: E2 (taken at the norm of the rounded rows, <= 1.001 xmax) bounds the f32
        // value against the squared distance of the ROUNDED row x_h; |x - x_h| <= 2^-11 |x| (+ 2^-25
        // per element in the half subnormal range; 1.05: the f64 -> f32 -> half double rounding), so
        // the exact distance of every dropped row is >= sqrt(F2 - E2') - emax
        const double E2h = E2 * 1.003;
        const double emax = 1.05 * 4.8828125e-4 * xmax + sqrt((double)csr.max_rowlen) * 3.1e-8;
        const double lo = F2 - E2h;
        certified = (s_qn < 1e36) && (F2 < 1e37) && lo > 0.0 && sqrt(lo) - emax > dk * (1.0 + 1e-13);
      }
      if (!certified) {
        if (tid == 0) {  // flag 2: the host re-runs this query with exact distances only
          ovf_flags[q] = 2u;
          atomicAdd(cand_total + 1, 1ULL);
        }
        return;
      }
    }
  } else if constexpr (PRE32) {
    // ---- refine: exact distances of the entries the f32 pass kept; certify the cut ----
    // (Round 4, measured and dropped HERE: the shard kernel's two-round refinement — exact distances
    // first for the entries near the k-th estimate, then for those a bound U on the k-th exact distance
    // cannot exclude: ~ 20 rows instead of 58 at C2.  The 58 rows are one lane-parallel round trip of a
    // workgroup that waits at barriers either way; the second round and its counting passes cost more
    // than the 35 KB they save: 1.288 against 1.274 ms per 10 000 queries on one box.)
    // The f32 distance of a row differs from the exact one by at most
    //   err(x) = 2.1 u (|x| + |q|) + (d + 2) u dist32,  u = 2^-24
    // (inputs rounded to f32, the differences, the f32 accumulation), so every candidate the
    // f32 pass dropped has an exact distance >= F - err(F), F = the smallest dropped f32
    // distance.  If that is not above the exact k-th distance the query goes to the exact path.
    const bool cut = best == k1;                    // something was dropped
    // the f32 pass keeps squared distances; the int8 pass integers, rounded to f32 in the packed
    // key (2^-24 relative, taken off here): F = s sqrt(I) bounds every dropped row from below
    const double F = !cut ? 0.0
                     : i8 ? sh8.s * (1.0 / 256.0) * sqrt(bdist[k1 - 1] * (1.0 - 1.2e-7))
                          : sqrt(bdist[k1 - 1]);
    const int m = cut ? k1 - 1 : best;
    if (wave == 0) {
      double qn = 0.0;
      for (int j = lane; j < d; j += 64) qn += (double)qs[j] * (double)qs[j];
      for (int o = 32; o > 0; o >>= 1) qn += __shfl_xor(qn, o);
      if (lane == 0) s_qn = sqrt(qn);
    }
    for (int i = tid; i < m; i += 256) {
      cid[i] = bid[i];
      cpos[i] = bpos[i];
    }
    __syncthreads();
    if constexpr (std::is_same<TD, double>::value) {
      for (int i = tid; i < m; i += 256)  // the reference's own arithmetic for the kept rows
        cdist[i] = leftfold_distance(X + (int64_t)cid[i] * d, qs, d);
    } else {
      batch_distances<TD, TA>(X, d, cid, cdist, qs, 0, m, wave, 4, lane);
    }
    __syncthreads();
    KSTAMP();  // refine: exact distances
    {  // the k best of the m <= 63 refined entries by (distance, position): rank by counting
      const bool mine = tid < m;
      const double di = mine ? cdist[tid] : 0.0;
      const int pi = mine ? cpos[tid] : 0, ii = mine ? cid[tid] : -1;
      int rank = 0;
      if (mine)
        rank = count_below2(cdist, cpos, m, di, pi);
      if (mine && rank < k) {
        bdist[rank] = di;
        bid[rank] = ii;
        bpos[rank] = pi;
      }
      __syncthreads();
      best = m < k ? m : k;
    }
    if (cut && best > 0) {
      const double u = 5.9604644775390625e-08;
      // + sqrt(d) * 4e-23: products in the f32 subnormal range lose relative accuracy
      // (absolute error 2^-150 each; |sqrt a - sqrt b| <= sqrt |a - b|)
      // half shadow: |x~ - x| <= 2^-11 |x| + sqrt(d) 2^-25 (subnormal halves), the query and the
      // arithmetic stay f32
      const double err = sh16 ? 1.05 * 4.8828125e-4 * xmax + 2.1 * u * s_qn + (double)(d + 2) * u * F +
                                    sqrt((double)d) * 3.1e-8
                              : 2.1 * u * (xmax + s_qn) + (double)(d + 2) * u * F + sqrt((double)d) * 4e-23;
      // (norms whose squares leave the f32 range — inf - inf = NaN entries are never ranked —
      // fail the test through s_qn; the dataset side is checked when the shadow is built)
      // F must be finite: an overflowed f32 sum (inf) orders nothing among the dropped
      // f32 DATA ranked on their half shadow: what the cut is compared with is the f32 distance the
      // all-f32 kernel ranks on, itself within (d + 2) u dist of the exact one
      double err2 = std::is_same<TD, double>::value ? err : err + (double)(d + 2) * u * (F + err) * 1.01;
      if (i8) {  // triangle inequality (Sh8): exact distance of a dropped row >= F - eq - emax
        const double e8 = (q8eq + sh8.emax) * (1.0 + 1e-12) + 1e-300;
        err2 = std::is_same<TD, double>::value ? e8 : e8 + (double)(d + 2) * u * F * 1.01;
        if (!(q8eq == q8eq)) err2 = F + 1.0;  // NaN in the query: never certified
      }
      if (!(s_qn < 1e18) || !(F < 1e30) || !(F - err2 > bdist[best - 1])) {
        if (k1 < k1_retry) {  // (uniform: shared values decide)
          k1 = k1_retry;
          // (counted: a forest whose batches retry often gets a wider first attempt, knn_dev)
          if (tid == 0 && !rerun) atomicAdd(reinterpret_cast<unsigned int*>(cand_total) + 4, 1u);
          __syncthreads();
          goto retry_wider;
        }
        if (tid == 0) {  // flag 2: the host answers this query again exactly (f64 rows: the exact
                         // kernel over the plan, see kLfMargin; f32 rows: the all-exact fused kernel)
          ovf_flags[q] = 2u;
          atomicAdd(cand_total + 1, 1ULL);
        }
        return;
      }
    }
  }
  if constexpr (!PRE32 && !CSR && std::is_same<TD, double>::value) {
    // f64 rows ranked on butterfly sums: the k + kLfMargin kept entries again as the reference's
    // left fold, the k best of THOSE in the order of those values (finalize_leftfold)
    __syncthreads();
    const double blast = best > 0 ? bdist[best - 1] : 0.0;  // the butterfly value of the last kept entry
    finalize_leftfold(reinterpret_cast<const double*>(X), d, reinterpret_cast<const double*>(qs), best, k,
                      dedup, cdist, cpos, bid, bpos, tid, 256, [] { __syncthreads(); }, q, out_ids,
                      out_dist, out_cnt, nullptr, 0.0, &s_fw, &s_flast);
    // (thread 0 wrote the answer, s_fw and s_flast.)  Flag 2: the host answers this query again
    // with the exact kernel (l2_cut_certified)
    if (tid == 0 && vote == 0 && !l2_cut_certified(l2cut, s_fw, k, s_flast, blast, d)) {
      ovf_flags[q] = 2u;
      atomicAdd(cand_total + 1, 1ULL);
    }
    return;
  }
  for (int i = tid; i < k; i += 256) {
    const bool ok = i < best;
    out_ids[q * k + i] = ok ? bid[i] : -1;
    out_dist[q * k + i] = ok ? (pack32 ? (double)sqrt(bdist[i]) : bdist[i])
                             : __longlong_as_double(0x7ff0000000000000LL);
  }
  if (tid == 0) out_cnt[q] = best;
  KSTAMP();  // final ranking, certificate, output
#undef KSTAMP
}

// ---------------------------------------------------------------------------------------
// fused query kernel, wave variant: ONE WAVE per query, four independent queries per
// workgroup and no workgroup barrier anywhere.  For small shards (a few trees per GPU, a few
// hundred candidates per query) the workgroup variant spends most of a query's life in its
// serial phases — traversal by T threads, range scan, k selection rounds with two barriers
// each — while the other waves of the CU can only cover for it if they belong to other
// queries; here every wave is its own query, so 12 queries per CU are in flight and their
// traversal latencies overlap the others' row gathers.  Lane = tree in the traversal (one
// pass: the leaf ranges go to per-tree slots and are compacted after a shuffle scan; a second
// pass only if a tree outgrew its slots), batches of kWC candidates, the wave's own entries of
// the batch in registers during the k arg-min rounds.  Same total order (distance, candidate
// position) and the same distance reduction as the workgroup variant: identical results.
// (kWC, kWR, kWT and the LDS bytes of a wave, fused_wave_bytes: knn_plan.h)
// ---------------------------------------------------------------------------------------
__device__ inline void wave_sync() {  // LDS writes of the wave visible to all its lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <class TD, class TK, bool PRE32, bool I8 = false /* PRE32 on the int8 shadow */>
__global__ __launch_bounds__(256, 3) void knn_fused_wave_kernel(
    const TD* __restrict__ X, int d, const TD* __restrict__ Q, const int32_t* __restrict__ perm,
    const double* __restrict__ thr, const double* __restrict__ mglo,
    const double* __restrict__ mghi, int64_t nodes, const TK* __restrict__ Pq, int64_t nq, int T,
    int L, int min_leaf, int64_t N, int k, int dedup, int32_t* __restrict__ out_ids,
    double* __restrict__ out_dist, int32_t* __restrict__ out_cnt, unsigned int* ovf_flags,
    unsigned int* ovf_count, unsigned long long* cand_total,
    const void* __restrict__ Xf, double xmax, int k1 /* PRE32: see knn_fused_kernel */,
    unsigned long long* dbg /* debug_stamps: phase clocks of one wave */, int sh16 = 0,
    Sh8 sh8 = Sh8{0.0, 0.0} /* s > 0: Xf is the int8 shadow (see Sh8) */) {
  typedef typename AccOf<TD>::type TA;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  if (q >= nq) return;  // no workgroup barrier below
  int dbgi = 0;
#define KSTAMP() do { if (dbg && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0 && dbgi < 60) dbg[dbgi++] = clock64(); } while (0)
  KSTAMP();
  const bool rerun = !PRE32 && k1 == -1;  // second pass: only the queries the prefilter gave up on
  if (rerun && ovf_flags[q] != 2u) return;
  const bool pack32 = !PRE32 && sizeof(TA) == 4 && dedup == 0;  // see knn_fused_kernel
  unsigned char* base = smem + (size_t)wave * fused_wave_bytes(d, sizeof(TA));
  double* cdist = reinterpret_cast<double*>(base);                 // [kWC]
  double* bdist = cdist + kWC;                                     // [kFKx]
  int64_t* rpoff = reinterpret_cast<int64_t*>(bdist + kFKx);       // [kWR] compact, tree order
  int64_t* spoff = rpoff + kWR;                                    // [kWR] per-tree slots
  TA* qs = reinterpret_cast<TA*>(spoff + kWR);                     // [d]
  int* cid = reinterpret_cast<int*>(base + (size_t)kWC * 8 + (size_t)kFKx * 8 + (size_t)kWR * 16 +
                                    (((size_t)d * sizeof(TA) + 7) & ~(size_t)7));  // [kWC]
  int* rn = cid + kWC;                                             // [kWR]
  int* sn = rn + kWR;                                              // [kWR]
  int* bid = sn + kWR;                                             // [kFKx]
  int* bpos = bid + kFKx;                                          // [kFKx]
  float* qs32 = reinterpret_cast<float*>(bpos + kFKx);             // [d] (PRE32)

  for (int j = lane; j < d; j += 64) qs[j] = ld<TD>(Q + q * d + j);
  constexpr bool i8 = I8;
  static_assert(!I8 || PRE32, "the int8 tier is a prefilter");
  double q8k = 0.0, q8eq = 0.0;
  if constexpr (I8) {  // int8 tier: the quantised query's byte planes in the f32 copy's place (see Sh8)
    wave_sync();
    if constexpr (sizeof(TA) == 8)
      quantise_query(reinterpret_cast<const double*>(qs), nullptr, d, sh8.s,
                     reinterpret_cast<unsigned int*>(qs32), lane, 64, q8k, q8eq);
    else
      quantise_query(nullptr, reinterpret_cast<const float*>(qs), d, sh8.s,
                     reinterpret_cast<unsigned int*>(qs32), lane, 64, q8k, q8eq);
    for (int o = 32; o > 0; o >>= 1) {
      q8k += __shfl_xor(q8k, o);
      q8eq += __shfl_xor(q8eq, o);
    }
    q8k -= 1073741824.0 * (double)d;
    q8eq = sqrt(q8eq);
    wave_sync();
  } else if (PRE32)
    for (int j = lane; j < d; j += 64) qs32[j] = (float)ld<TD>(Q + q * d + j);

  // ---- traversal: lane = tree; ranges into the tree's S slots, counted in any case ----
  const int S = kWR / T;
  int my_nc = 0, my_nr = 0;
  if (lane < T) {
    const int t = lane;
    traverse<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, Pq + (int64_t)t * L * nq + q,
                 nq, L, min_leaf, N, [&](int off, int n) {
                   if (my_nr < S) {
                     spoff[t * S + my_nr] = (int64_t)t * N + off;
                     sn[t * S + my_nr] = n;
                   }
                   my_nc += n;
                   ++my_nr;
                 });
  }
  int inc_c = my_nc, inc_r = my_nr;  // inclusive scans over the trees
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(inc_c, o), b = __shfl_up(inc_r, o);
    if (lane >= o) {
      inc_c += a;
      inc_r += b;
    }
  }
  const int nc_tot = __shfl(inc_c, 63), nr_tot = __shfl(inc_r, 63);
  KSTAMP();  // 1: traversal
  if (nr_tot > kWR) {  // too many leaf ranges for the slab: general path
    if (lane == 0) {
      ovf_flags[q] = 1u;
      atomicAdd(ovf_count, 1u);
    }
    return;
  }
  if (lane == 0 && !rerun) atomicAdd(cand_total, (unsigned long long)nc_tot);
  if (__ballot(my_nr > S) == 0ULL) {  // the usual case: compact the slots (a lane reads its own)
    if (lane < T) {
      const int r0 = inc_r - my_nr;
      for (int r = 0; r < my_nr; ++r) {
        rpoff[r0 + r] = spoff[lane * S + r];
        rn[r0 + r] = sn[lane * S + r];
      }
    }
  } else if (lane < T) {  // some tree reached more leaves than its slots hold: second pass
    const int t = lane;
    int r = inc_r - my_nr;
    traverse<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, Pq + (int64_t)t * L * nq + q,
                 nq, L, min_leaf, N, [&](int off, int n) {
                   rpoff[r] = (int64_t)t * N + off;
                   rn[r] = n;
                   ++r;
                 });
  }
  wave_sync();
  // rstart[r] = candidates before range r (the batches are filled by position, see
  // knn_fused_kernel), in the slot slab the compaction has just emptied: lane l scans ranges 2l, 2l + 1
  int* rstart = reinterpret_cast<int*>(spoff);  // [nr_tot + 1] <= kWR + 1 ints in kWR int64
  {
    const int a = 2 * lane < nr_tot ? rn[2 * lane] : 0, b = 2 * lane + 1 < nr_tot ? rn[2 * lane + 1] : 0;
    int incl = a + b;
    for (int o = 1; o < 64; o <<= 1) {
      const int t2 = __shfl_up(incl, o);
      if (lane >= o) incl += t2;
    }
    const int excl = incl - (a + b);
    if (2 * lane <= nr_tot) rstart[2 * lane] = excl;
    if (2 * lane + 1 <= nr_tot) rstart[2 * lane + 1] = excl + a;
    if (lane == 63) rstart[nr_tot] = incl;  // = nc_tot (the only writer of entry kWR when all slots are in use)
  }
  wave_sync();

  constexpr int E = kWC / 64;  // batch entries a lane owns: lane, lane + 64, ...
  const double kInf = __longlong_as_double(0x7ff0000000000000LL);
  // ---- selection over the batch entries [0, fill): entries below first_new are the running
  // best list (positions in bpos), the others are new candidates at positions pb0, pb0 + 1, ...;
  // ksel rounds of wave-wide arg-min by (distance, position); winners to bdist / bid / bpos ----
  // f32 pass: squared f32 distance bits << 32 | position as one key (see knn_fused_kernel)
  auto wselect_packed = [&](int fill, int first_new, int pb0, int ksel) -> int {
    unsigned long long key[E];
    unsigned int vlo = ~0u;  // the lane's smallest value
#pragma unroll
    for (int s2 = 0; s2 < E; ++s2) {
      const int i = lane + 64 * s2;
      const unsigned int pos = i < first_new ? (unsigned int)bpos[i < kFKx ? i : 0] : (unsigned int)(pb0 + (i - first_new));
      key[s2] = i < fill ? ((unsigned long long)__float_as_uint((float)cdist[i]) << 32) | pos : ~0ULL;
      if (i < fill) {
        const unsigned int v = (unsigned int)(key[s2] >> 32);
        vlo = v < vlo ? v : vlo;
      }
    }
    wave_sync();  // bpos is rewritten below, cdist becomes the list slab
    // a threshold instead of ksel rounds (see knn_fused_kernel's select_packed): the value of the
    // list's last entry once it is full, else the ksel-th smallest of the 64 per-lane minima
    unsigned int tau;
    if (first_new == ksel) {
      tau = __float_as_uint((float)bdist[ksel - 1]);
    } else {
      int cnt = 0;
#pragma unroll
      for (int j2 = 0; j2 < 64; ++j2) {  // (constant lane: v_readlane, not an LDS permute)
        const unsigned int o = (unsigned int)__builtin_amdgcn_readlane((int)vlo, j2);
        cnt += (o < vlo || (o == vlo && j2 < lane)) ? 1 : 0;
      }
      const unsigned long long hit = __ballot(cnt == ksel - 1);
      tau = __shfl(vlo, __ffsll((long long)hit) - 1);  // ~0u with fewer than ksel occupied lanes
    }
    unsigned long long* lkey = reinterpret_cast<unsigned long long*>(cdist);      // [128]
    int* lidx = reinterpret_cast<int*>(cdist + 128);                               // [128]
    unsigned int* lcnt = reinterpret_cast<unsigned int*>(cdist + 192);
    if (lane == 0) *lcnt = 0u;
    wave_sync();
#pragma unroll
    for (int s2 = 0; s2 < E; ++s2)
      if (key[s2] != ~0ULL && (unsigned int)(key[s2] >> 32) <= tau) {
        const unsigned int slot = atomicAdd(lcnt, 1u);
        if (slot < 128u) {
          lkey[slot] = key[s2];
          lidx[slot] = lane + 64 * s2;
        }
      }
    wave_sync();
    const int n = (int)*lcnt;
    if (n <= 128) {
      for (int t = lane; t < n; t += 64) {
        const unsigned long long mine = lkey[t];
        const int rank = count_below(lkey, n, mine);
        if (rank < ksel) {
          bdist[rank] = (double)__uint_as_float((unsigned int)(mine >> 32));
          bid[rank] = cid[lidx[t]];
          bpos[rank] = (int)(unsigned int)mine;
        }
      }
      wave_sync();
      return n < ksel ? n : ksel;
    }
    // fallback (values tied by the hundred): ksel rounds of wave-wide arg-min
    int nb = 0;
    while (nb < ksel) {
      unsigned long long m = key[0];
#pragma unroll
      for (int s2 = 1; s2 < E; ++s2) m = key[s2] < m ? key[s2] : m;
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t2 = __shfl_xor(m, o);
        m = t2 < m ? t2 : m;
      }
      if (m == ~0ULL) break;
#pragma unroll
      for (int s2 = 0; s2 < E; ++s2)
        if (key[s2] == m) {
          key[s2] = ~0ULL;
          bdist[nb] = (double)__uint_as_float((unsigned int)(m >> 32));
          bid[nb] = cid[lane + 64 * s2];
          bpos[nb] = (int)(unsigned int)m;
        }
      ++nb;
    }
    wave_sync();
    return nb;
  };
  // kdist > 0: the entries of the best kdist different ids, l2cut (knn_fused_kernel's select)
  bool l2cut = false;
  auto wselect = [&](int fill, int first_new, int pb0, int ksel, int dedup, int kdist) -> int {
    // ---- the lane's entries: distance and candidate position (-1 = none / consumed) ----
    double dd[E];
    int pp[E];
#pragma unroll
    for (int s = 0; s < E; ++s) {
      const int i = lane + 64 * s;
      dd[s] = i < fill ? cdist[i] : kInf;
      if (dd[s] != dd[s]) dd[s] = kInf;  // NaN ranks with +inf, by position (see knn_fused_kernel's select)
      pp[s] = i < fill ? (i < first_new ? bpos[i] : pb0 + (i - first_new)) : -1;
    }
    wave_sync();  // bpos is rewritten below
    // ---- selection: k rounds of wave-wide arg-min by (distance, position) ----
    int nb = 0, nd = 0;
    double last_d = -1.0;
    while (nb < ksel) {
      double bd = kInf;
      int bp = 0x7fffffff, bi = -1;
#pragma unroll
      for (int s = 0; s < E; ++s)
        if (pp[s] >= 0 && (dd[s] < bd || (dd[s] == bd && pp[s] < bp))) {
          bd = dd[s];
          bp = pp[s];
          bi = lane + 64 * s;
        }
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o);
        const int op = __shfl_xor(bp, o), oi = __shfl_xor(bi, o);
        if (od < bd || (od == bd && op < bp)) {
          bd = od;
          bp = op;
          bi = oi;
        }
      }
      if (bi < 0) break;  // candidates exhausted
#pragma unroll
      for (int s = 0; s < E; ++s)
        if (bi == lane + 64 * s) pp[s] = -1;  // consumed
      bool keep = true, copy = false;
      if (dedup == 2 && nb > 0 && bd == last_d) keep = false;  // knnPQ: one per distance
      else if ((dedup || kdist > 0) && bd == last_d)  // same id => same distance: duplicates are among equal dist
        for (int j = nb - 1; j >= 0 && bdist[j] == bd; --j)
          if (bid[j] == cid[bi]) copy = true;
      if (dedup && copy) keep = false;
      if (keep && kdist > 0 && !copy) {
        if (nd == kdist) {  // one different id more than the kept set holds (wave-uniform)
          l2cut = true;
          break;
        }
        ++nd;
      }
      if (keep) {
        if (lane == 0) {
          bdist[nb] = bd;
          bid[nb] = cid[bi];
          bpos[nb] = bp;
        }
        wave_sync();
        ++nb;
        last_d = bd;
      }
    }
    if (kdist > 0 && nb == ksel) l2cut = true;
    return nb;
  };

  int best = 0, pos_base = 0;
  while (pos_base < nc_tot || best == 0) {
    // ---- fill the batch: best list first (keeps its positions), then new candidates ----
    for (int i = lane; i < best; i += 64) {
      cdist[i] = bdist[i];
      cid[i] = bid[i];
    }
    int fill = best;
    const int first_new = best, pb0 = pos_base;
    {  // by position: a seven-step search over rstart, the lane's perm loads all in flight at once
      int take = nc_tot - pos_base;
      if (take > kWC - fill) take = kWC - fill;
      int64_t addr[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int s2 = lane + 64 * e;
        const int c = pos_base + (s2 < take ? s2 : 0);
        int lo = 0;
#pragma unroll
        for (int step = kWR / 2; step > 0; step >>= 1) {
          const int m = lo + step;
          if (m < nr_tot && rstart[m] <= c) lo = m;
        }
        addr[e] = rpoff[lo] + (c - rstart[lo]);
      }
      int32_t idv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) idv[e] = lane + 64 * e < take ? perm[addr[e]] : 0;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (lane + 64 * e < take) cid[fill + lane + 64 * e] = idv[e];
      fill += take;
      pos_base += take;
    }
    wave_sync();
    KSTAMP();  // batch filled
    if constexpr (PRE32) {
      if constexpr (I8)
        batch_distances_i8<16>(static_cast<const uint8_t*>(Xf), d, cid, cdist,
                              reinterpret_cast<const unsigned int*>(qs32), q8k, first_new, fill, 0, 1, lane);
      else if (sh16)
        batch_distances<_Float16, float, 16, false>(static_cast<const _Float16*>(Xf), d, cid, cdist, qs32,
                                                    first_new, fill, 0, 1, lane);
      else
        batch_distances<float, float, 16, false>(static_cast<const float*>(Xf), d, cid, cdist, qs32,
                                                 first_new, fill, 0, 1, lane);
    } else if (pack32)
      batch_distances<TD, TA, (sizeof(TD) < 8 ? 16 : 8), false>(X, d, cid, cdist, qs, first_new, fill, 0, 1, lane);
    else
      batch_distances<TD, TA, (sizeof(TD) < 8 ? 16 : 8)>(X, d, cid, cdist, qs, first_new, fill, 0, 1, lane);
    wave_sync();
    KSTAMP();  // distances
    // f64 rows: the entries of k + kLfMargin different ids, as many as the list holds when duplicates
    // are kept; "each id once" while streaming (see knn_fused_kernel and kLfMargin)
    constexpr bool L2F64 = !PRE32 && std::is_same<TD, double>::value;
    const int kdist = L2F64 ? k + kLfMargin : 0;
    const int ksel = L2F64 ? (dedup == 0 ? kFKx : k + kLfMargin) : k;
    const int nb = PRE32 ? wselect_packed(fill, first_new, pb0, k1)
                 : pack32 ? wselect_packed(fill, first_new, pb0, k)
                          : wselect(fill, first_new, pb0, ksel, L2F64 && dedup ? 1 : dedup, kdist);
    best = nb;
    KSTAMP();  // selection
    if (pos_base >= nc_tot) break;
  }
  if constexpr (PRE32) {  // exact distances of the kept entries + certified cut (knn_fused_kernel)
    const bool cut = best == k1;
    // the f32 pass keeps squared distances, the int8 pass integers (knn_fused_kernel)
    const double F = !cut ? 0.0
                     : i8 ? sh8.s * (1.0 / 256.0) * sqrt(bdist[k1 - 1] * (1.0 - 1.2e-7))
                          : sqrt(bdist[k1 - 1]);
    const int m = cut ? k1 - 1 : best;
    double qn = 0.0;
    for (int j = lane; j < d; j += 64) qn += (double)qs[j] * (double)qs[j];
    for (int o = 32; o > 0; o >>= 1) qn += __shfl_xor(qn, o);
    for (int i = lane; i < m; i += 64) cid[i] = bid[i];
    wave_sync();
    if constexpr (std::is_same<TD, double>::value) {
      for (int i = lane; i < m; i += 64)  // the reference's own arithmetic (leftfold_distance)
        cdist[i] = leftfold_distance(X + (int64_t)cid[i] * d, qs, d);
    } else {
      batch_distances<TD, TA>(X, d, cid, cdist, qs, 0, m, 0, 1, lane);
    }
    wave_sync();
    KSTAMP();  // refine distances
    {  // the k best of the m <= 63 refined entries by (distance, position): every lane ranks its
       // own entry by counting (no selection rounds), the winners go to bdist / bid / bpos
      const bool mine = lane < m;
      const double di = mine ? cdist[lane] : kInf;
      const int pi = mine ? bpos[lane] : 0x7fffffff, ii = mine ? bid[lane] : -1;
      int rank = 0;
      rank = count_below2(cdist, bpos, m, di, pi);
      wave_sync();
      if (mine && rank < k) {
        bdist[rank] = di;
        bid[rank] = ii;
        bpos[rank] = pi;
      }
      wave_sync();
      best = m < k ? m : k;
    }
    KSTAMP();  // final selection
    if (cut && best > 0) {
      const double u = 5.9604644775390625e-08;
      const double err = sh16 ? 1.05 * 4.8828125e-4 * xmax + 2.1 * u * sqrt(qn) + (double)(d + 2) * u * F +
                                    sqrt((double)d) * 3.1e-8
                              : 2.1 * u * (xmax + sqrt(qn)) + (double)(d + 2) * u * F + sqrt((double)d) * 4e-23;
      double err2 = std::is_same<TD, double>::value ? err : err + (double)(d + 2) * u * (F + err) * 1.01;
      if (i8) {  // triangle inequality (Sh8)
        const double e8 = (q8eq + sh8.emax) * (1.0 + 1e-12) + 1e-300;
        err2 = std::is_same<TD, double>::value ? e8 : e8 + (double)(d + 2) * u * F * 1.01;
        if (!(q8eq == q8eq)) err2 = F + 1.0;  // NaN in the query: never certified
      }
      if (!(sqrt(qn) < 1e18) || !(F < 1e30) || !(F - err2 > bdist[best - 1])) {
        if (lane == 0) {
          ovf_flags[q] = 2u;
          atomicAdd(cand_total + 1, 1ULL);
        }
        return;
      }
    }
  }
  if constexpr (!PRE32 && std::is_same<TD, double>::value) {  // see knn_fused_kernel
    wave_sync();
    const double blast = best > 0 ? bdist[best - 1] : 0.0;  // the butterfly value of the last kept entry
    int fw = 0;         // (lane 0's: it writes the answer)
    double flast = 0.0;
    finalize_leftfold(reinterpret_cast<const double*>(X), d, reinterpret_cast<const double*>(qs), best, k,
                      dedup, cdist, cid, bid, bpos, lane, 64, [] { wave_sync(); }, q, out_ids, out_dist,
                      out_cnt, nullptr, 0.0, &fw, &flast);
    // flag 2: the host answers this query again with the exact kernel (l2_cut_certified)
    if (lane == 0 && !l2_cut_certified(l2cut, fw, k, flast, blast, d)) {
      ovf_flags[q] = 2u;
      atomicAdd(cand_total + 1, 1ULL);
    }
    return;
  }
  for (int i = lane; i < k; i += 64) {
    const bool ok = i < best;
    out_ids[q * k + i] = ok ? bid[i] : -1;
    out_dist[q * k + i] = ok ? (pack32 ? (double)sqrt(bdist[i]) : bdist[i]) : kInf;
  }
  if (lane == 0) out_cnt[q] = best;
  KSTAMP();
#undef KSTAMP
}

// ---------------------------------------------------------------------------------------
// Small tree shards, round 4 (what one of G GPUs holds: a few trees, a few hundred candidates per
// query).  Two changes against knn_fused_wave_kernel's prefiltered instantiations, same answers:
//
// (1) The traversal is its own launch.  In the fused kernel it was 28 % of a query's life (47 k of
//     165 k cycles at a 4-tree C2 shard) with 4 of 64 lanes at work on a chain of dependent loads,
//     inside a wave that holds 168 registers and 12 KB of LDS for the phases that follow.
//     shard_ranges_kernel walks with lane = (query, tree) — 64 / T queries per wave, every lane
//     busy, a dozen registers — and leaves each query's leaf ranges compacted in tree order
//     (RPTree.hs:289-314 per tree, :176 the concatenation).
//
// (2) The rows that get an exact distance are chosen by VALUE, not by count.  The ranking tiers
//     bound a candidate's exact distance D by its ranking value: lower(Dh) <= D <= upper(Dh), Dh the
//     tier's distance estimate (the int8 tier: triangle inequality, Sh8; f32 / half: the rounding
//     analysis in knn_fused_kernel).  So
//       * the k-th smallest exact distance d_k is at most upper(Dh_(k)), Dh_(k) the k-th smallest
//         estimate seen so far: a candidate with lower(Dh) > upper(Dh_(k)) can be dropped at once and
//         for good (the bound only tightens as batches arrive) — the carried list;
//       * once the first entries of the list have their exact distances, U = the k-th smallest of
//         those is an upper bound of d_k too, and only list entries with lower(Dh) <= U need an exact
//         distance at all.
//     Every candidate without an exact distance is strictly farther than d_k, so the k best by
//     (exact distance, position) of the refined ones are the reference's answer (RPTree.hs:174-176) —
//     certified by construction: no fixed k' (the one-wave kernel kept k + 37 rows for every query to
//     certify the worst of ten thousand: 48 KB of f64 rows per query against 63 KB of int8 rows; the
//     band at the cut holds ~ 9), no uncertified re-runs except a list that outgrows its 128 slots.
// (kSKmax, the largest k the shard kernel serves, and shard_wave_bytes: knn_plan.h)

template <class TK>
__global__ __launch_bounds__(256) void shard_ranges_kernel(
    const double* __restrict__ thr, const double* __restrict__ mglo, const double* __restrict__ mghi,
    int64_t nodes, const TK* __restrict__ Pq, int64_t nq, int T, int L, int min_leaf, int64_t N,
    int2* __restrict__ hdr /* [nq] (leaf ranges, candidates) */, int64_t* __restrict__ rng_off /* [nq][kWR] */,
    int* __restrict__ rng_n /* [nq][kWR] */, unsigned int* ovf_flags, unsigned int* ovf_count,
    unsigned long long* cand_total) {
  const int lane = threadIdx.x & 63;
  const int qpw = 64 / T;  // queries per wave (T <= 64)
  const int64_t wave_g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int ql = lane / T, t = lane - ql * T;
  const int64_t q = wave_g * qpw + ql;
  const bool on = ql < qpw && q < nq;
  int nr = 0, nc = 0, o0 = 0, n0 = 0, o1 = 0, n1 = 0;
  if (on)
    traverse<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, Pq + (int64_t)t * L * nq + q, nq, L,
                 min_leaf, N, [&](int off, int n) {
                   if (nr == 0) {
                     o0 = off;
                     n0 = n;
                   } else if (nr == 1) {
                     o1 = off;
                     n1 = n;
                   }
                   nc += n;
                   ++nr;
                 });
  int ir = nr, ic = nc;  // inclusive scans over the wave, made segment-relative below
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(ir, o), b = __shfl_up(ic, o);
    if (lane >= o) {
      ir += a;
      ic += b;
    }
  }
  const int seg0 = ql * T, seg1 = seg0 + T - 1 < 63 ? seg0 + T - 1 : 63;
  const int pr = __shfl(ir, seg0 > 0 ? seg0 - 1 : 0), pc = __shfl(ic, seg0 > 0 ? seg0 - 1 : 0);
  const int er = __shfl(ir, seg1), ec = __shfl(ic, seg1);
  const int before_r = seg0 > 0 ? pr : 0, before_c = seg0 > 0 ? pc : 0;
  const int nr_tot = er - before_r, nc_tot = ec - before_c;
  const int base = ir - nr - before_r;  // this tree's first slot in the query's compact list
  unsigned long long visited = 0;
  if (on) {
    if (t == 0) hdr[q] = make_int2(nr_tot, nc_tot);
    if (nr_tot > kWR) {  // too many leaf ranges for the consumer's slab: general path
      if (t == 0) {
        ovf_flags[q] = 1u;
        atomicAdd(ovf_count, 1u);
      }
    } else {
      if (t == 0) visited = (unsigned long long)nc_tot;
      int64_t* ro = rng_off + q * kWR + base;
      int* rn = rng_n + q * kWR + base;
      if (nr >= 1) {
        ro[0] = (int64_t)t * N + o0;
        rn[0] = n0;
      }
      if (nr >= 2) {
        ro[1] = (int64_t)t * N + o1;
        rn[1] = n1;
      }
      if (nr > 2) {  // rare (both children at two nodes of one tree): walk again for the rest
        int i = 0;
        traverse<TK>(thr + t * nodes, mglo + t * nodes, mghi + t * nodes, Pq + (int64_t)t * L * nq + q, nq,
                     L, min_leaf, N, [&](int off, int n) {
                       if (i >= 2) {
                         ro[i] = (int64_t)t * N + off;
                         rn[i] = n;
                       }
                       ++i;
                     });
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) visited += __shfl_xor(visited, o);
  if (lane == 0 && visited) atomicAdd(cand_total, visited);
}

// TIER: 1 = f32 shadow, 2 = IEEE-half shadow, 3 = int8 shadow (Sh8)
// kSL: slots of the carried list (a multiple of 64); MINB: workgroups per CU the register budget allows.
// Two shapes are instantiated: (128, 4) for shards whose candidates are one batch, (256, 3) beyond
// (the first batch's threshold comes from per-lane minima and lets more of a 980-candidate query
// through than 128 slots hold: 1.6 % of the queries of an 8-tree C2 shard).  WC = candidates per
// batch: 512, and 640 in the second shape — a C4 shard's 610 candidates per query are one batch
// instead of 512 + 98 (a batch costs a fill and a list update whatever it holds).
template <class TD, int TIER, int kSL, int MINB, int WC>
__global__ __launch_bounds__(256, MINB) void knn_shard_wave_kernel(
    const TD* __restrict__ X, int d, const TD* __restrict__ Q, const int32_t* __restrict__ perm, int64_t nq,
    int k, const int2* __restrict__ hdr, const int64_t* __restrict__ rng_off, const int* __restrict__ rng_n,
    int32_t* __restrict__ out_ids, double* __restrict__ out_dist, int32_t* __restrict__ out_cnt,
    unsigned int* ovf_flags, unsigned long long* cand_total, const void* __restrict__ Xf, double xmax, Sh8 sh8,
    int r1_pct /* first refinement round: estimates up to Dh_(k) + r1_pct % of the error bound */,
    unsigned long long* dbg) {
  typedef typename AccOf<TD>::type TA;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  if (q >= nq) return;  // no workgroup barrier below
  int dbgi = 0;
#define KSTAMP() do { if (dbg && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0 && dbgi < 60) dbg[dbgi++] = clock64(); } while (0)
  KSTAMP();
  const int2 h = hdr[q];
  const int nr_tot = h.x, nc_tot = h.y;
  if (nr_tot > kWR) return;  // flagged by shard_ranges_kernel: the general path answers it
  constexpr int kSLpl = kSL / 64;  // list entries per lane
  unsigned char* base = smem + (size_t)wave * shard_wave_bytes(d, sizeof(TA), kSL, WC);
  unsigned long long* lkey = reinterpret_cast<unsigned long long*>(base);           // [kSL] (value bits << 32 | position)
  double* rdist = reinterpret_cast<double*>(lkey + kSL);                              // [kSL] exact distances
  int64_t* rpoff = reinterpret_cast<int64_t*>(rdist + kSL);                           // [kWR]
  TA* qs = reinterpret_cast<TA*>(rpoff + kWR);                                        // [d]
  float* cval = reinterpret_cast<float*>(base + (size_t)kSL * 16 + (size_t)kWR * 8 +
                                         (((size_t)d * sizeof(TA) + 15) & ~(size_t)15));  // [WC] ranking values
  int* cid = reinterpret_cast<int*>(cval + WC);                                       // [WC]
  int* rstart = cid + WC;                                                            // [kWR + 1]
  int* lid = rstart + kWR + 4;                                                        // [kSL]
  unsigned int* lcnt = reinterpret_cast<unsigned int*>(lid + kSL);                    // [4]
  float* qs32 = reinterpret_cast<float*>(lcnt + 4);                                   // [d] f32 copy / byte planes

  // ---- the query's leaf ranges (tree order) and rstart[r] = candidates before range r ----
  for (int r = lane; r < nr_tot; r += 64) rpoff[r] = rng_off[q * kWR + r];
  {
    const int a = 2 * lane < nr_tot ? rng_n[q * kWR + 2 * lane] : 0;
    const int b = 2 * lane + 1 < nr_tot ? rng_n[q * kWR + 2 * lane + 1] : 0;
    int incl = a + b;
    for (int o = 1; o < 64; o <<= 1) {
      const int t2 = __shfl_up(incl, o);
      if (lane >= o) incl += t2;
    }
    const int excl = incl - (a + b);
    if (2 * lane <= nr_tot) rstart[2 * lane] = excl;
    if (2 * lane + 1 <= nr_tot) rstart[2 * lane + 1] = excl + a;
  }
  // ---- the query: exact copy, ranking copy, norm ----
  double qn = 0.0;
  for (int j = lane; j < d; j += 64) {
    const TA v = ld<TD>(Q + q * d + j);
    qs[j] = v;
    qn += (double)v * (double)v;
    if constexpr (TIER != 3) qs32[j] = (float)v;
  }
  for (int o = 32; o > 0; o >>= 1) qn += __shfl_xor(qn, o);
  const double qnorm = sqrt(qn);
  double q8k = 0.0, q8eq = 0.0;
  if constexpr (TIER == 3) {
    wave_sync();
    if constexpr (sizeof(TA) == 8)
      quantise_query(reinterpret_cast<const double*>(qs), nullptr, d, sh8.s, reinterpret_cast<unsigned int*>(qs32),
                     lane, 64, q8k, q8eq);
    else
      quantise_query(nullptr, reinterpret_cast<const float*>(qs), d, sh8.s, reinterpret_cast<unsigned int*>(qs32),
                     lane, 64, q8k, q8eq);
    for (int o = 32; o > 0; o >>= 1) {
      q8k += __shfl_xor(q8k, o);
      q8eq += __shfl_xor(q8eq, o);
    }
    q8k -= 1073741824.0 * (double)d;
    q8eq = sqrt(q8eq);
  }
  wave_sync();
  KSTAMP();  // 1: ranges + query

  // ---- the tier's bounds (TierBounds) ----
  const TierBounds tb = TierBounds::make(TIER, std::is_same<TD, double>::value, d, xmax, qnorm, q8eq, sh8);
  const double A = tb.A, Bt = tb.Bt, Bf = tb.Bf;
  // squares outside the f32 range, NaN: no bound holds — the exact kernel answers (as before)
  if (!(qnorm < 1e18) || !(A == A)) {
    if (lane == 0) {
      ovf_flags[q] = 2u;
      atomicAdd(cand_total + 1, 1ULL);
    }
    return;
  }
  auto dh_up = [&](unsigned int vb) -> double { return tb.dh_up(vb); };
  auto keep_bits = [&](double Ulim) -> unsigned int { return tb.keep_bits(Ulim); };
  auto upper = [&](double dh) -> double { return tb.upper(dh); };

  constexpr int E = WC / 64;
  int n_list = 0, pos_base = 0;
  while (pos_base < nc_tot) {
    // ---- fill: candidate s of the batch by position (a search over rstart, the perm loads in flight together)
    const int take = nc_tot - pos_base < WC ? nc_tot - pos_base : WC;
    {
      int64_t addr[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int s2 = lane + 64 * e;
        const int c = pos_base + (s2 < take ? s2 : 0);
        int lo = 0;
#pragma unroll
        for (int step = kWR / 2; step > 0; step >>= 1) {
          const int m = lo + step;
          if (m < nr_tot && rstart[m] <= c) lo = m;
        }
        addr[e] = rpoff[lo] + (c - rstart[lo]);
      }
      int32_t idv[E];
#pragma unroll
      for (int e = 0; e < E; ++e) idv[e] = lane + 64 * e < take ? perm[addr[e]] : 0;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (lane + 64 * e < take) cid[lane + 64 * e] = idv[e];
    }
    wave_sync();
    KSTAMP();  // batch filled
    if constexpr (TIER == 3)
      batch_distances_i8<16, float>(static_cast<const uint8_t*>(Xf), d, cid, cval,
                                    reinterpret_cast<const unsigned int*>(qs32), q8k, 0, take, 0, 1, lane);
    else if constexpr (TIER == 2)
      batch_distances<_Float16, float, 16, false, float>(static_cast<const _Float16*>(Xf), d, cid, cval, qs32, 0,
                                                         take, 0, 1, lane);
    else
      batch_distances<float, float, 16, false, float>(static_cast<const float*>(Xf), d, cid, cval, qs32, 0, take,
                                                      0, 1, lane);
    wave_sync();
    KSTAMP();  // ranking values
    // ---- the batch against the carried list ----
    unsigned long long key[E];
    unsigned int vlo = ~0u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = lane + 64 * e;
      key[e] = i < take ? ((unsigned long long)__float_as_uint(cval[i]) << 32) | (unsigned int)(pos_base + i) : ~0ULL;
      const unsigned int v = (unsigned int)(key[e] >> 32);
      vlo = v < vlo ? v : vlo;
    }
    // an upper bound of the k-th smallest value seen: the list's k-th entry, or (first batch) the
    // k-th smallest of the 64 per-lane minima
    unsigned int tau;
    if (n_list >= k) {
      tau = (unsigned int)(lkey[k - 1] >> 32);
    } else {
      int cnt = 0;
#pragma unroll
      for (int j2 = 0; j2 < 64; ++j2) {
        const unsigned int o = (unsigned int)__builtin_amdgcn_readlane((int)vlo, j2);
        cnt += (o < vlo || (o == vlo && j2 < lane)) ? 1 : 0;
      }
      const unsigned long long hit = __ballot(cnt == k - 1);
      tau = __shfl(vlo, __ffsll((long long)hit) - 1);  // ~0u with fewer than k occupied lanes
    }
    const unsigned int thr0 = tau >= 0x7f800000u ? 0x7fc00000u : keep_bits(upper(dh_up(tau)));
    if (lane == 0) *lcnt = (unsigned int)n_list;
    wave_sync();
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (key[e] != ~0ULL && (unsigned int)(key[e] >> 32) <= thr0) {
        const unsigned int slot = atomicAdd(lcnt, 1u);
        if (slot < (unsigned int)kSL) {
          lkey[slot] = key[e];
          lid[slot] = cid[lane + 64 * e];
        }
      }
    wave_sync();
    const int n = (int)*lcnt;
    if (n > kSL) {  // more candidates inside the band than the list holds (values tied by the hundred)
      if (lane == 0) {
        ovf_flags[q] = 2u;
        atomicAdd(cand_total + 1, 1ULL);
      }
      return;
    }
    {  // order the list by (value, position): rank by counting, kSLpl entries per lane
      unsigned long long mk[kSLpl];
      int mi[kSLpl], mr[kSLpl];
#pragma unroll
      for (int w = 0; w < kSLpl; ++w) {
        const int i = lane + 64 * w;
        mk[w] = i < n ? lkey[i] : ~0ULL;
        mi[w] = i < n ? lid[i] : 0;
      }
#pragma unroll
      for (int w = 0; w < kSLpl; ++w) mr[w] = lane + 64 * w < n ? count_below(lkey, n, mk[w]) : 0;
      wave_sync();
#pragma unroll
      for (int w = 0; w < kSLpl; ++w)
        if (lane + 64 * w < n) {
          lkey[mr[w]] = mk[w];
          lid[mr[w]] = mi[w];
        }
      wave_sync();
    }
    n_list = n;
    if (n > k) {  // trim to the band of the (now exact) k-th smallest value: a prefix of the ordered list
      const unsigned int vk = (unsigned int)(lkey[k - 1] >> 32);
      const unsigned int thr1 = vk >= 0x7f800000u ? 0x7fc00000u : keep_bits(upper(dh_up(vk)));
      int c = 0;
#pragma unroll
      for (int w = 0; w < kSLpl; ++w)
        c += __popcll(__ballot(lane + 64 * w < n && (unsigned int)(lkey[lane + 64 * w] >> 32) <= thr1));
      n_list = c;
    }
    pos_base += take;
    KSTAMP();  // list updated
  }

  // ---- exact distances, first round: the entries whose estimate is within r1_pct % of the error bound
  // above the k-th estimate (the k-th exact distance is about the k-th estimate: what lies beyond
  // that is what the second round would have to add)
  auto exact = [&](int from, int to) {
    if constexpr (std::is_same<TD, double>::value) {
      for (int i = from + lane; i < to; i += 64)  // the reference's own arithmetic (leftfold_distance)
        rdist[i] = leftfold_distance(reinterpret_cast<const double*>(X) + (int64_t)lid[i] * d,
                                     reinterpret_cast<const double*>(qs), d);
    } else {
      batch_distances<TD, TA>(X, d, lid, rdist, qs, from, to, 0, 1, lane);
    }
  };
  auto prefix_le = [&](unsigned int tb) -> int {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kSLpl; ++w)
      c += __popcll(__ballot(lane + 64 * w < n_list && (unsigned int)(lkey[lane + 64 * w] >> 32) <= tb));
    return c;
  };
  // rank of entry (di, pi) among the refined entries [0, m) by (exact distance, position); NaN behind
  // every number, NaNs by position
  auto rank_of = [&](int m, double di, unsigned int pi) -> int {
    int rank = 0;
    if (di != di) {
      for (int j = 0; j < m; ++j) rank += rdist[j] == rdist[j] || (unsigned int)lkey[j] < pi;
      return rank;
    }
    int j = 0;
    for (; j + 8 <= m; j += 8) {
      double a[8];
      unsigned int b[8];
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        a[w] = rdist[j + w];
        b[w] = (unsigned int)lkey[j + w];
      }
#pragma unroll
      for (int w = 0; w < 8; ++w) rank += a[w] < di || (a[w] == di && b[w] < pi);
    }
    for (; j < m; ++j) rank += rdist[j] < di || (rdist[j] == di && (unsigned int)lkey[j] < pi);
    return rank;
  };
  int m = n_list;
  if (n_list > k) {
    const double dk = dh_up((unsigned int)(lkey[k - 1] >> 32));
    int r1 = prefix_le(keep_bits((dk + (A + Bt * dk) * (0.01 * (double)r1_pct) - A) * (1.0 - Bf)));
    // (keep_bits(U) keeps Dh <= (U / (1 - Bf) + A) / (1 - Bt): with the U above that is about
    // Dh <= dk + r1_pct % of the bound)
    r1 = r1 < k ? k : r1;
    exact(0, r1);
    wave_sync();
    KSTAMP();  // first round
    m = r1;
    if (r1 < n_list) {
      // U = the k-th smallest exact distance so far; entries beyond r1 with lower(Dh) <= U follow
      double U = 0.0;
      {
        double dv[kSLpl];
        unsigned long long hit[kSLpl];
#pragma unroll
        for (int w = 0; w < kSLpl; ++w) {
          const int i = lane + 64 * w;
          dv[w] = i < r1 ? rdist[i] : 0.0;
          const int rk = i < r1 ? rank_of(r1, dv[w], (unsigned int)lkey[i]) : -1;
          hit[w] = __ballot(rk == k - 1);
        }
#pragma unroll
        for (int w = 0; w < kSLpl; ++w)
          if (hit[w]) U = __shfl(dv[w], __ffsll((long long)hit[w]) - 1);  // (uniform: exactly one hit)
      }
      const int r2 = U == U ? prefix_le(keep_bits(U)) : n_list;
      if (r2 > r1) {
        exact(r1, r2);
        wave_sync();
        m = r2;
      }
      KSTAMP();  // second round
    }
  } else {
    exact(0, n_list);
    wave_sync();
    KSTAMP();
  }
  // ---- the k best of the m refined entries by (exact distance, position) ----
  {
#pragma unroll
    for (int w = 0; w < kSLpl; ++w) {
      const int i = lane + 64 * w;
      if (i < m) {
        const double di = rdist[i];
        const int rk = rank_of(m, di, (unsigned int)lkey[i]);
        if (rk < k) {
          out_ids[q * k + rk] = lid[i];
          out_dist[q * k + rk] = di;
        }
      }
    }
    const int best = m < k ? m : k;
    for (int i = best + lane; i < k; i += 64) {
      out_ids[q * k + i] = -1;
      out_dist[q * k + i] = __longlong_as_double(0x7ff0000000000000LL);
    }
    if (lane == 0) out_cnt[q] = best;
  }
  KSTAMP();
#undef KSTAMP
}

// CSR data and CSR queries: the query is densified into LDS; distance of a sparse row x:
// d^2 = |q|^2 + sum_{j in nz(x)} ((x_j - q_j)^2 - q_j^2)   (true Euclidean distance)
template <class TD>
__global__ __launch_bounds__(256) void topk_csr_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const TD* __restrict__ val, int64_t nnz, int d, const int64_t* __restrict__ qrowptr,
    const int32_t* __restrict__ qcol, const TD* __restrict__ qval,
    const int32_t* __restrict__ perm, const Range* __restrict__ ranges,
    const int64_t* __restrict__ rng_off, int T, int k, int dedup, int refm /* RPT_KNN_METRIC_REFERENCE */,
    int32_t* __restrict__ out_ids, double* __restrict__ out_dist, int32_t* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Entry* buf = reinterpret_cast<Entry*>(smem);
  int* scratch = reinterpret_cast<int*>(smem + sizeof(Entry) * kBuf);
  double* qs = reinterpret_cast<double*>(smem + (sizeof(Entry) + 4) * kBuf);  // [d]
  __shared__ double s_qn2;
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < d; j += blockDim.x) qs[j] = 0.0;
  __syncthreads();
  for (int64_t j = qrowptr[q] + threadIdx.x; j < qrowptr[q + 1]; j += blockDim.x)
    qs[qcol[j]] = (double)qval[j];
  __syncthreads();
  if (threadIdx.x < 64) {
    double s = 0;
    for (int j = lane; j < d; j += 64) s += qs[j] * qs[j];
    s = wave_sum(s);
    if (lane == 0) s_qn2 = s;
  }
  __syncthreads();
  const double qn2 = s_qn2;
  int best = 0, filled = 0;
  const int cap = kBuf;
  for (int64_t r = rng_off[q * T]; r < rng_off[(q + 1) * T]; ++r) {
    const Range rg = ranges[r];
    int done = 0;
    while (done < rg.n) {
      int take = rg.n - done;
      if (take > cap - filled) take = cap - filled;
      // RPT_KNN_METRIC_REFERENCE: metricSSL2 (Internal.hs:389-393) as the reference evaluates it —
      // diffSS = binSS (-) 0 (:435-450), a merge of the two index lists that STOPS when either is
      // exhausted (the tail of the longer one is dropped), the squares summed by a left fold in
      // merge order.  One thread per candidate: the walk is sequential by definition.
      if (refm) {
        const int64_t qa = qrowptr[q], qb = qrowptr[q + 1];
        for (int i = threadIdx.x; i < take; i += blockDim.x) {
          const int id = perm[rg.poff + done + i];
          int64_t i1 = rowptr[id];
          const int64_t b1 = rowptr[id + 1];
          int64_t i2 = qa;
          double acc = 0.0;
          while (i1 < b1 && i2 < qb) {
            const int il = col[i1], ir = qcol[i2];
            double df;
            if (il == ir) {
              df = (double)val[i1] - (double)qval[i2];
              ++i1;
              ++i2;
            } else if (il < ir) {
              df = (double)val[i1] - 0.0;
              ++i1;
            } else {
              df = 0.0 - (double)qval[i2];
              ++i2;
            }
            acc = acc + df * df;
          }
          buf[filled + i] = Entry{sqrt(acc), rg.pos + done + i, id};
        }
      } else
      // sixteen lanes per candidate row, sixteen rows per wave in flight (csr_rows_dist2)
      for (int i0 = wave * 16; i0 < take; i0 += 64) {
        constexpr int U = 4;
        int64_t ra[U], rb[U];
        int id[U];
        double s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * 4 + (lane >> 4);
          const bool ok = i < take;
          id[u] = perm[rg.poff + done + (ok ? i : 0)];
          ra[u] = rowptr[id[u]];
          rb[u] = ok ? rowptr[id[u] + 1] : ra[u];
        }
        csr_rows_dist2<TD, U>(col, val, nnz, ra, rb, qs, lane & 15, s);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * 4 + (lane >> 4);
          const double t = s[u] + qn2;
          if ((lane & 15) == 0 && i < take)
            buf[filled + i] = Entry{sqrt(t > 0 ? t : 0.0), rg.pos + done + i, id[u]};
        }
      }
      filled += take;
      done += take;
      __syncthreads();
      if (filled == cap) {
        best = merge_best(buf, filled, k, dedup, scratch);
        filled = best;
        __syncthreads();
      }
    }
  }
  if (filled > best || best == 0) {
    best = merge_best(buf, filled, k, dedup, scratch);
    __syncthreads();
  }
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const bool ok = i < best;
    out_ids[q * k + i] = ok ? buf[i].id : -1;
    out_dist[q * k + i] = ok ? buf[i].dist : __longlong_as_double(0x7ff0000000000000LL);
  }
  if (threadIdx.x == 0) out_cnt[q] = best;
}

// ---- cosine / inner product on CSR rows (rpt_knn_csr_metric_*, rpt_brute_knn_csr_metric_*) ----
// dotS(x, q) of two CSR rows (strictly ascending columns, values widened exactly): from +0.0, over the
// columns stored in BOTH rows in ascending order, acc = acc + x_j * q_j, every product and sum
// rounded on its own.  inner = -dotS(x, q), cosine = 1 - dotS(x, q) / (sqrt(dotS(x, x)) sqrt(dotS(q,
// q))).  With finite stored values these are the dense metrics' bits on the dense-ified rows: a
// column one side lacks would add x * (+0.0) = +-0.0 to an acc that is never -0.0.  A stored inf or
// NaN meets no 0 of the other side: the column counts only where both rows store it.
// One thread walks the row x (nonzeros [a, b)) against the dense-ified query qs; pres holds one bit
// per column the query stores.  Eight loads in flight; the sum is the fold whatever their grouping.
template <class TD>
__device__ inline double leftfold_dot_csr(const int32_t* __restrict__ col, const TD* __restrict__ val,
                                          int64_t a, int64_t b, const double* qs, const unsigned int* pres) {
  double acc = 0.0;
  int64_t j = a;
  for (; j + 8 <= b; j += 8) {
    int c[8];
    TD v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      c[u] = col[j + u];
      v[u] = val[j + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if ((pres[c[u] >> 5] >> (c[u] & 31)) & 1u) acc = acc + (double)v[u] * qs[c[u]];
  }
  for (; j < b; ++j) {
    const int c = col[j];
    if ((pres[c >> 5] >> (c & 31)) & 1u) acc = acc + (double)val[j] * qs[c];
  }
  return acc;
}

// row_sqnorm_kernel for CSR rows: rn[i] = dotS(x_i, x_i), the fold of the row's stored squares, and
// the same two statistics (a row is all zeros when every stored value equals 0)
template <class TD>
__global__ __launch_bounds__(256) void row_sqnorm_csr_kernel(const int64_t* __restrict__ rowptr,
                                                             const TD* __restrict__ val, int64_t n,
                                                             double* __restrict__ rn,
                                                             unsigned long long* __restrict__ stats) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long bits = 0, bad = 0;
  if (r < n) {
    double v = 0.0;
    bool nz = false;
    for (int64_t j = rowptr[r]; j < rowptr[r + 1]; ++j) {
      const double x = (double)val[j];
      v = v + x * x;
      nz = nz || x != 0.0;
    }
    rn[r] = v;
    bits = (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffULL;
    if (!(v >= 0x1p-900 && v <= 0x1p900)) bad = nz;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long ob = __shfl_xor(bits, o), oo = __shfl_xor(bad, o);
    bits = ob > bits ? ob : bits;
    bad |= oo;
  }
  if ((threadIdx.x & 63) == 0) {
    if (bits) atomicMax(&stats[0], bits);
    if (bad) atomicOr(&stats[1], bad);
  }
}

// knn_metric_kernel for CSR rows and CSR queries: the same batches, merges, margin and certificate
// (metric_cut_slack with d: a row pair has at most d products, fewer only tighten the bound), one
// workgroup per query over the plan's leaf ranges or, identity, rows 0 .. N - 1 (the brute force).
// The query is dense-ified into LDS (qs, and pres: a bit per stored column); qq = dotS(q, q) is
// folded by one thread over the query's stored values.
//   EXACT = false: the values are csr_rows_dist2's lane-parallel dot (sixteen lanes per row, four
// rows per group in flight); it reads qs alone — with finite values the columns the query lacks add
// exact zeros, and a stored inf / NaN makes stats or qq non-finite, which fails the certificate of
// every query that left a candidate out.  The kept entries are evaluated again as the fold WITH the
// presence test, so a query that left nothing out is the definition whatever the values are.
//   EXACT = true: every value is leftfold_dot_csr, merge_best selects with no margin.
// LDS: knn_metric_kernel's, then pres [(d + 31) / 32] words.
template <class TD, int METRIC, bool EXACT>
__global__ __launch_bounds__(256) void knn_metric_csr_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const TD* __restrict__ val, int64_t nnz,
    int d, const int64_t* __restrict__ qrowptr, const int32_t* __restrict__ qcol, const TD* __restrict__ qval,
    int64_t nq, const int32_t* __restrict__ perm, const Range* __restrict__ ranges,
    const int64_t* __restrict__ rng_off, int T, int64_t N, int identity, int nbuf, int k, int dedup,
    const double* __restrict__ rn, const unsigned long long* __restrict__ stats, int32_t* __restrict__ unc,
    unsigned long long* __restrict__ unc_count, int32_t* __restrict__ out_ids, double* __restrict__ out_dist,
    int32_t* __restrict__ out_cnt) {
  static_assert(METRIC == kMetricCosine || METRIC == kMetricInner, "cosine or inner product");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Entry* buf = reinterpret_cast<Entry*>(smem);                         // [nbuf]
  int* scratch = reinterpret_cast<int*>(smem + sizeof(Entry) * nbuf);  // [nbuf]
  double* cd = reinterpret_cast<double*>(scratch + nbuf);              // [kMB]
  int* cid = reinterpret_cast<int*>(cd + kMB);                         // [kMB]
  int* cpos = cid + kMB;                                               // [kMB]
  double* qs = reinterpret_cast<double*>(cpos + kMB);                  // [d]
  unsigned int* pres = reinterpret_cast<unsigned int*>(qs + d);        // [(d + 31) / 32]
  __shared__ Range s_rng[kMW];
  __shared__ int s_fill, s_merge[2], s_w;
  __shared__ double s_qq, s_blast, s_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kk = EXACT ? k : (k + kLfMargin < nbuf / 2 ? k + kLfMargin : nbuf / 2);
  const int sdedup = EXACT ? dedup : (dedup ? 1 : 0);  // the fast path's rule while streaming
  const int64_t nw = EXACT && unc ? (int64_t)*unc_count : nq;  // the queries of this launch
  for (int64_t iw = blockIdx.x; iw < nw; iw += gridDim.x) {
    const int64_t q = EXACT && unc ? (int64_t)unc[iw] : iw;
    __syncthreads();  // (the previous query's finalize still reads the arrays)
    for (int j = threadIdx.x; j < d; j += blockDim.x) qs[j] = 0.0;
    for (int j = threadIdx.x; j < (d + 31) / 32; j += blockDim.x) pres[j] = 0u;
    if (threadIdx.x == 0) s_fill = 0;
    __syncthreads();
    const int64_t qa = qrowptr[q], qb = qrowptr[q + 1];
    for (int64_t j = qa + threadIdx.x; j < qb; j += blockDim.x) {
      const int c = qcol[j];
      qs[c] = (double)qval[j];
      atomicOr(&pres[c >> 5], 1u << (c & 31));
    }
    if (threadIdx.x == 0) {  // dotS(q, q)
      double acc = 0.0;
      for (int64_t j = qa; j < qb; ++j) {
        const double v = (double)qval[j];
        acc = acc + v * v;
      }
      s_qq = acc;
    }
    __syncthreads();
    const double qq = METRIC == kMetricCosine ? s_qq : 0.0;

    int best = 0;
    bool cut = false;       // some candidate is not in buf (other than a same-id copy)
    Entry thr{0.0, 0, -1};  // the last kept entry after a cut; id -1: none yet, every entry enters
    const int64_t r0 = identity ? 0 : rng_off[q * T];
    const int64_t r1 = identity ? 1 : rng_off[(q + 1) * T];
    int64_t r = r0, w0 = r0, w1 = r0;  // next range; ranges [w0, w1) are in s_rng
    int done = 0;                      // candidates of range r already taken
    while (r < r1) {
      int nb = 0;
      while (nb < kMB && r < r1) {  // block-uniform
        if (r == w1) {
          __syncthreads();
          w0 = r;
          w1 = r + kMW < r1 ? r + kMW : r1;
          for (int i = threadIdx.x; i < w1 - w0; i += blockDim.x)
            s_rng[i] = identity ? Range{0, (int32_t)N, 0} : ranges[w0 + i];
          __syncthreads();
        }
        const Range rg = s_rng[r - w0];
        int take = rg.n - done;
        if (take > kMB - nb) take = kMB - nb;
        for (int i = threadIdx.x; i < take; i += blockDim.x) {
          const int c = done + i;
          cid[nb + i] = identity ? c : perm[rg.poff + c];
          cpos[nb + i] = rg.pos + c;
        }
        nb += take;
        done += take;
        if (done == rg.n) {
          ++r;
          done = 0;
        }
      }
      __syncthreads();
      if constexpr (EXACT) {
        for (int i = threadIdx.x; i < nb; i += blockDim.x)
          cd[i] = leftfold_dot_csr<TD>(col, val, rowptr[cid[i]], rowptr[cid[i] + 1], qs, pres);
      } else {
        batch_distances_csr<TD, true>(rowptr, col, val, nnz, cid, cd, qs, 0.0, 0, nb, wave, lane);
      }
      __syncthreads();
      // the order inside buf does not matter (the merges sort by value and position)
      for (int i = threadIdx.x; i < nb; i += blockDim.x) {
        const Entry e{metric_value<METRIC>(cd[i], METRIC == kMetricCosine ? rn[cid[i]] : 0.0, qq), cpos[i],
                      cid[i]};
        if (entry_less_total(e, thr)) buf[atomicAdd(&s_fill, 1)] = e;
      }
      __syncthreads();
      const int filled = s_fill;
      if (filled + kMB > nbuf || r >= r1) {
        if constexpr (EXACT) {
          best = merge_best<true>(buf, filled, kk, sdedup, scratch);
          if (best == kk) thr = buf[kk - 1];
        } else {
          best = merge_distinct(buf, filled, kk, nbuf / 2, sdedup != 0, scratch, s_merge);
          if (s_merge[1]) {
            cut = true;
            thr = buf[best - 1];
          }
        }
        __syncthreads();
        if (threadIdx.x == 0) s_fill = best;
        __syncthreads();
      }
    }
    if (threadIdx.x == 0) s_blast = best > 0 ? buf[best - 1].dist : 0.0;  // (buf's lower half stays)
    double* lf = reinterpret_cast<double*>(scratch);     // nbuf / 2 doubles >= kk
    int* ids2 = reinterpret_cast<int*>(buf + nbuf / 2);  // the upper half of buf is free now:
    int* pos2 = ids2 + nbuf / 2;                         // 3 x nbuf / 2 ints fit its 8 x nbuf bytes
    int* order = pos2 + nbuf / 2;
    for (int i = threadIdx.x; i < best; i += blockDim.x) {
      const int id = buf[i].id;
      ids2[i] = id;
      pos2[i] = buf[i].pos;
      lf[i] = metric_value<METRIC>(leftfold_dot_csr<TD>(col, val, rowptr[id], rowptr[id + 1], qs, pres),
                                   METRIC == kMetricCosine ? rn[id] : 0.0, qq);
    }
    __syncthreads();
    finalize_select(best, k, dedup, lf, order, ids2, pos2, (int)threadIdx.x, (int)blockDim.x,
                    [] { __syncthreads(); }, q, out_ids, out_dist, out_cnt, &s_w, &s_last);
    if (!EXACT && threadIdx.x == 0) {  // (the thread that wrote the answer and s_w / s_last)
      bool ok = !cut;
      if (!ok && s_w == k) ok = s_last < s_blast - metric_cut_slack<METRIC>(d, s_qq, stats);
      if (!ok) unc[atomicAdd(unc_count, 1ULL)] = (int32_t)q;
    }
  }
}

// knnH: distances of the points of the selected leaf ranges, written in result order
// (sel[r].pos = position of the range's first point in the query's result).  One block per
// query, one wave per point.
template <class TD>
__global__ __launch_bounds__(256) void dist_sel_dense_kernel(
    const TD* __restrict__ X, int d, const TD* __restrict__ Q, const int32_t* __restrict__ perm,
    const Range* __restrict__ sel, const int64_t* __restrict__ sel_off,
    const int64_t* __restrict__ out_off, int32_t* __restrict__ out_ids,
    double* __restrict__ out_dist) {
  typedef typename AccOf<TD>::type TA;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  TA* qs = reinterpret_cast<TA*>(smem);
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < d; j += blockDim.x) qs[j] = ld<TD>(Q + q * d + j);
  __syncthreads();
  if constexpr (std::is_same<TD, double>::value) {
    // knnH returns whole buckets: every point's distance as metricDDL2's left fold (one thread per
    // point; see leftfold_distance)
    for (int64_t r = sel_off[q]; r < sel_off[q + 1]; ++r) {
      const Range rg = sel[r];
      for (int i = threadIdx.x; i < rg.n; i += blockDim.x) {
        const int id = perm[rg.poff + i];
        out_ids[out_off[q] + rg.pos + i] = id;
        out_dist[out_off[q] + rg.pos + i] = leftfold_distance(X + (int64_t)id * d, qs, d);
      }
    }
    return;
  }
  for (int64_t r = sel_off[q]; r < sel_off[q + 1]; ++r) {
    const Range rg = sel[r];
    for (int i = wave; i < rg.n; i += 4) {
      const int id = perm[rg.poff + i];
      TA s = (TA)0;
      for (int j = lane; j < d; j += 64) {
        const TA df = ld<TD>(X + (int64_t)id * d + j) - qs[j];
        s += df * df;
      }
      const TA tot = wave_sum(s);
      if (lane == 0) {
        out_ids[out_off[q] + rg.pos + i] = id;
        out_dist[out_off[q] + rg.pos + i] = (double)sqrt((double)tot);
      }
    }
  }
}

template <class TD>
__global__ __launch_bounds__(256) void dist_sel_csr_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const TD* __restrict__ val, int d, const int64_t* __restrict__ qrowptr,
    const int32_t* __restrict__ qcol, const TD* __restrict__ qval,
    const int32_t* __restrict__ perm, const Range* __restrict__ sel,
    const int64_t* __restrict__ sel_off, const int64_t* __restrict__ out_off,
    int32_t* __restrict__ out_ids, double* __restrict__ out_dist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* qs = reinterpret_cast<double*>(smem);  // [d] densified query
  __shared__ double s_qn2;
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < d; j += blockDim.x) qs[j] = 0.0;
  __syncthreads();
  for (int64_t j = qrowptr[q] + threadIdx.x; j < qrowptr[q + 1]; j += blockDim.x)
    qs[qcol[j]] = (double)qval[j];
  __syncthreads();
  if (threadIdx.x < 64) {
    double s = 0;
    for (int j = lane; j < d; j += 64) s += qs[j] * qs[j];
    s = wave_sum(s);
    if (lane == 0) s_qn2 = s;
  }
  __syncthreads();
  const double qn2 = s_qn2;
  for (int64_t r = sel_off[q]; r < sel_off[q + 1]; ++r) {
    const Range rg = sel[r];
    for (int i = wave; i < rg.n; i += 4) {
      const int id = perm[rg.poff + i];
      double s = 0;
      for (int64_t j = rowptr[id] + lane; j < rowptr[id + 1]; j += 64) {
        const double qj = qs[col[j]];
        const double df = (double)val[j] - qj;
        s += df * df - qj * qj;  // same formula as topk_csr_kernel: true Euclidean distance
      }
      s = wave_sum(s) + qn2;
      if (lane == 0) {
        out_ids[out_off[q] + rg.pos + i] = id;
        out_dist[out_off[q] + rg.pos + i] = sqrt(s > 0 ? s : 0.0);
      }
    }
  }
}

// multi-GPU merge: G shard results per query; shard g's [nq][k] ids / distances and [nq] counts
// start g * sstride BYTES after the base pointers (shard-major arrays: sstride = the array's
// own size; one packed exchange record per shard: sstride = the record size)
__global__ __launch_bounds__(256) void merge_kernel(const int32_t* __restrict__ ids,
                                                    const double* __restrict__ dist,
                                                    const int32_t* __restrict__ cnt,
                                                    int64_t ids_stride, int64_t dist_stride,
                                                    int64_t cnt_stride, int G, int64_t nq, int k,
                                                    int dedup, int32_t* __restrict__ out_ids,
                                                    double* __restrict__ out_dist,
                                                    int32_t* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int total = G * k;
  int np = 1;
  while (np < total) np <<= 1;
  Entry* buf = reinterpret_cast<Entry*>(smem);
  int* scratch = reinterpret_cast<int*>(smem + sizeof(Entry) * np);
  const int64_t q = blockIdx.x;
  auto shard_cnt = [&](int g) {
    return reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(cnt) + g * cnt_stride)[q];
  };
  // invalid slots sort last: dist = +inf, pos keeps shard order
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int g = i / k, r = i % k;
    const bool ok = r < shard_cnt(g);
    const int64_t src = q * k + r;
    const double* dg =
        reinterpret_cast<const double*>(reinterpret_cast<const char*>(dist) + g * dist_stride);
    const int32_t* ig =
        reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(ids) + g * ids_stride);
    buf[i] = Entry{ok ? dg[src] : __longlong_as_double(0x7ff0000000000000LL), i, ok ? ig[src] : -1};
  }
  __syncthreads();
  int valid = 0;
  for (int g = 0; g < G; ++g) valid += shard_cnt(g);
  // the total order: NaN distances (a NaN query, a zero row under the cosine metric) rank behind
  // every number and among themselves by shard position, as on one device; negative distances
  // (the inner-product metric) are ordinary numbers
  int best = merge_best<true>(buf, total, k, dedup, scratch);
  // merge_best counted +inf padding as entries: clamp to the valid ones (dedup can only
  // shrink further; invalid entries have id -1 and sort last)
  __syncthreads();
  int m = 0;
  for (int i = 0; i < best; ++i) m += buf[i].id >= 0;  // every thread computes the same
  best = m < valid ? m : valid;
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const bool ok = i < best;
    out_ids[q * k + i] = ok ? buf[i].id : -1;
    out_dist[q * k + i] = ok ? buf[i].dist : __longlong_as_double(0x7ff0000000000000LL);
  }
  if (threadIdx.x == 0) out_cnt[q] = best;
}

// ---- host side ----------------------------------------------------------------------------
struct QueryPlan {
  DevBuf<char> Pq;  // [T][L][nq] projections of the queries
  DevBuf<int> cnt_cand, cnt_rng;
  DevBuf<int64_t> cand_off, rng_off;
  DevBuf<Range> ranges;
  int64_t total_cand = 0, total_rng = 0;
};

template <class TK>
int32_t make_plan_t(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* q, QueryPlan& pl) {
  const int64_t nq = q->n;
  const int T = f->T, L = f->L;
  hipStream_t st = ctx->stream;
  ProfScope ps(ctx, RPT_PROF_KNN_PLAN);
  RPT_TRY(pl.Pq.alloc((size_t)T * L * nq * sizeof(TK) + 16));
  if (L > 0 && nq > 0) RPT_TRY(project_columns(ctx, q, f->R.p, T * L, f->mode, pl.Pq.p));
  const int64_t m = nq * T;
  RPT_TRY(pl.cnt_cand.alloc((size_t)m));
  RPT_TRY(pl.cnt_rng.alloc((size_t)m));
  RPT_TRY(pl.cand_off.alloc((size_t)m + 1));
  RPT_TRY(pl.rng_off.alloc((size_t)m + 1));
  if (nq == 0) return RPT_OK;
  const int threads = T <= 64 ? 64 : (T <= 128 ? 128 : 256);
  const TK* Pq = reinterpret_cast<const TK*>(pl.Pq.p);
  if (f->xtopo)
    hipLaunchKernelGGL(count_x_kernel<TK>, dim3((unsigned)nq), dim3(threads), 0, st, f->thr.p,
                       f->mglo.p, f->mghi.p, f->nodes, (const int8_t*)f->xkind.p,
                       (const int64_t*)f->xoff.p, (const int64_t*)f->xlen.p, Pq, nq, T, L,
                       pl.cnt_cand.p, pl.cnt_rng.p);
  else
    hipLaunchKernelGGL(count_kernel<TK>, dim3((unsigned)nq), dim3(threads), 0, st, f->thr.p,
                       f->mglo.p, f->mghi.p, f->nodes, Pq, nq, T, L, f->min_leaf, f->n,
                       pl.cnt_cand.p, pl.cnt_rng.p);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, pl.cnt_cand.p, m, pl.cand_off.p);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, pl.cnt_rng.p, m, pl.rng_off.p);
  RPT_HIP(hipGetLastError());
  int64_t tot[2];
  RPT_HIP(hipMemcpyAsync(&tot[0], pl.cand_off.p + m, 8, hipMemcpyDeviceToHost, st));
  RPT_HIP(hipMemcpyAsync(&tot[1], pl.rng_off.p + m, 8, hipMemcpyDeviceToHost, st));
  RPT_HIP(stream_sync(st));
  pl.total_cand = tot[0];
  pl.total_rng = tot[1];
  RPT_TRY(pl.ranges.alloc((size_t)pl.total_rng));
  if (f->xtopo)
    hipLaunchKernelGGL(ranges_x_kernel<TK>, dim3((unsigned)nq), dim3(threads), 0, st, f->thr.p,
                       f->mglo.p, f->mghi.p, f->nodes, (const int8_t*)f->xkind.p,
                       (const int64_t*)f->xoff.p, (const int64_t*)f->xlen.p, Pq, nq, T, L, f->n,
                       pl.cand_off.p, pl.rng_off.p, pl.ranges.p);
  else
    hipLaunchKernelGGL(ranges_kernel<TK>, dim3((unsigned)nq), dim3(threads), 0, st, f->thr.p,
                       f->mglo.p, f->mghi.p, f->nodes, Pq, nq, T, L, f->min_leaf, f->n,
                       pl.cand_off.p, pl.rng_off.p, pl.ranges.p);
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

int32_t make_plan(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* q, QueryPlan& pl) {
  RPT_ARG(proj_dtype(q->dtype) == f->pdtype,
          "query dtype must have the forest's projection type (f64 vs f32/bf16)");
  if (f->pdtype == RPT_F64) return make_plan_t<double>(ctx, f, q, pl);
  return make_plan_t<float>(ctx, f, q, pl);
}

size_t topk_smem(int d, size_t acc_size) { return (sizeof(Entry) + 4) * kBuf + (size_t)d * acc_size; }

}  // namespace

int32_t candidates(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* q, int64_t* off_host,
                   int32_t* ids_host, int64_t cap, int64_t* total) {
  QueryPlan pl;
  RPT_TRY(make_plan(ctx, f, q, pl));
  *total = pl.total_cand;
  const int64_t m = q->n * f->T;
  if (off_host) {
    if (m > 0) RPT_HIP(hipMemcpy(off_host, pl.cand_off.p, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost));
    else off_host[0] = 0;
  }
  if (ids_host && pl.total_cand > 0) {
    RPT_ARG(cap >= pl.total_cand, "ids capacity too small");
    DevBuf<int32_t> ids;
    RPT_TRY(ids.alloc((size_t)pl.total_cand));
    hipLaunchKernelGGL(expand_kernel, dim3((unsigned)q->n), dim3(128), 0, ctx->stream,
                       f->perm.p, pl.ranges.p, pl.rng_off.p, pl.cand_off.p, f->T, ids.p);
    RPT_HIP(hipGetLastError());
    RPT_HIP(stream_sync(ctx->stream));
    RPT_HIP(hipMemcpy(ids_host, ids.p, (size_t)pl.total_cand * 4, hipMemcpyDeviceToHost));
  }
  return RPT_OK;
}

template <class TD>
static int32_t launch_topk_dense(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                                 const int32_t* perm, const Range* ranges, const int64_t* rng_off,
                                 int T, int identity, int k, int dedup, int32_t* ids,
                                 double* dist, int32_t* cnt, int32_t* unc = nullptr,
                                 unsigned long long* unc_count = nullptr /* f64: see launch_l2_f64 */) {
  typedef typename AccOf<TD>::type TA;
  const size_t smem = topk_smem(data->d, sizeof(TA));
  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  RPT_HIP(launch_dyn(topk_dense_kernel<TD>, dim3((unsigned)q->n), dim3(256), smem, ctx->stream,
                     (const TD*)data->X, data->d, (const TD*)q->X, perm, ranges, rng_off, T,
                     data->n, identity, k, dedup, ids, dist, cnt, unc, unc_count));
  return RPT_OK;
}

constexpr int kMergeMax = 4096;  // entries of one merge launch (LDS)

// f32 shadow of a dense f64 dataset + its largest row norm (one wave per row)
__global__ __launch_bounds__(256) void shadow32_kernel(const double* __restrict__ X, int64_t n, int d,
                                                       float* __restrict__ Xf,
                                                       unsigned long long* __restrict__ max_bits) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  double mx = 0.0;
  for (int64_t r = row0; r < n; r += (int64_t)gridDim.x * 4) {
    double s = 0.0;
    for (int j = lane; j < d; j += 64) {
      const double v = X[r * d + j];
      Xf[r * d + j] = (float)v;
      s += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (!(s <= mx)) mx = s == s ? s : __longlong_as_double(0x7ff0000000000000LL);  // NaN row -> +inf
  }
  if (lane == 0) atomicMax(max_bits, (unsigned long long)__double_as_longlong(mx));  // mx >= 0
}

// Builds the f32 shadow once per dataset.  The shadow is an optimisation: whenever it cannot be
// had (no memory for it, a failed launch or copy, rows whose squares leave the f32 range, NaN
// rows) the dataset is marked "tried, unusable" (max_norm = -2) and the caller continues on the
// all-f64 path — never an error.
static int32_t ensure_shadow(rpt_ctx* ctx, const rpt_dataset* data) {
  if (data->shadow32 || data->max_norm == -2.0) return RPT_OK;
  void* p = nullptr;
  DevBuf<unsigned long long> mb;
  unsigned long long bits = 0;
  auto give_up = [&]() {
    if (p) dev_free(p);
    (void)hipGetLastError();       // the exact path starts from a clean error state
    data->max_norm = -2.0;
    return RPT_OK;
  };
  if (dev_alloc(&p, (size_t)data->n * data->d * sizeof(float)) != hipSuccess) {
    p = nullptr;
    return give_up();
  }
  if (mb.alloc(1) != RPT_OK) return give_up();
  if (hipMemsetAsync(mb.p, 0, 8, ctx->stream) != hipSuccess) return give_up();
  int64_t blocks = (data->n + 3) / 4;
  if (blocks > (int64_t)ctx->n_cu * 16) blocks = (int64_t)ctx->n_cu * 16;
  hipLaunchKernelGGL(shadow32_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                     (const double*)data->X, data->n, data->d, (float*)p, mb.p);
  if (hipGetLastError() != hipSuccess) return give_up();
  if (hipMemcpyAsync(&bits, mb.p, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    return give_up();
  if (stream_sync(ctx->stream) != hipSuccess) return give_up();
  double m2;
  std::memcpy(&m2, &bits, 8);
  data->max_norm = std::sqrt(m2) * (1.0 + 1e-12);
  // squares would leave the f32 range, or a row holds a NaN (the kernel folds a NaN sum into
  // +inf, see shadow32_kernel): no shadow
  if (!(data->max_norm < 1e18)) return give_up();
  data->shadow32 = (float*)p;
  return RPT_OK;
}

// IEEE-half shadow of a dense f64 dataset (one wave per row) + the largest |element| (bits in
// max_bits[0]); built after the f32 shadow, whose row norm it shares
template <class TIn>
__global__ __launch_bounds__(256) void shadow16_kernel(const TIn* __restrict__ X, int64_t n, int d,
                                                       _Float16* __restrict__ Xh,
                                                       unsigned long long* __restrict__ max_bits) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  double mx = 0.0, mn2 = 0.0;  // largest |element|, largest squared row norm
  for (int64_t r = row0; r < n; r += (int64_t)gridDim.x * 4) {
    double s2 = 0.0;
    for (int j = lane; j < d; j += 64) {
      const double v = (double)X[r * d + j];
      Xh[r * d + j] = (_Float16)(float)v;
      const double a = fabs(v);
      if (!(a <= mx)) mx = a == a ? a : __longlong_as_double(0x7ff0000000000000LL);
      s2 += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
    if (!(s2 <= mn2)) mn2 = s2 == s2 ? s2 : __longlong_as_double(0x7ff0000000000000LL);
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(mx, o);
    mx = t > mx ? t : mx;
  }
  if (lane == 0) {
    atomicMax(max_bits, (unsigned long long)__double_as_longlong(mx));
    atomicMax(max_bits + 1, (unsigned long long)__double_as_longlong(mn2));
  }
}

// The half shadow, once per dataset: allowed to fail like the f32 one (no memory, elements outside
// the half range): the f32 tier then ranks.
static int32_t ensure_shadow16(rpt_ctx* ctx, const rpt_dataset* data) {
  if (data->shadow16_state != 0) return RPT_OK;
  data->shadow16_state = -1;
  void* p = nullptr;
  DevBuf<unsigned long long> mb;
  unsigned long long bits[2] = {0, 0};
  auto give_up = [&]() {
    if (p) dev_free(p);
    (void)hipGetLastError();
    return RPT_OK;
  };
  if (data->dtype == RPT_BF16 || data->csr) return RPT_OK;
  if (dev_alloc(&p, (size_t)data->n * data->d * 2 + 16) != hipSuccess) {
    p = nullptr;
    return give_up();
  }
  if (mb.alloc(2) != RPT_OK) return give_up();
  if (hipMemsetAsync(mb.p, 0, 16, ctx->stream) != hipSuccess) return give_up();
  int64_t blocks = (data->n + 3) / 4;
  if (blocks > (int64_t)ctx->n_cu * 16) blocks = (int64_t)ctx->n_cu * 16;
  if (data->dtype == RPT_F64)
    hipLaunchKernelGGL(shadow16_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       (const double*)data->X, data->n, data->d, (_Float16*)p, mb.p);
  else
    hipLaunchKernelGGL(shadow16_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       (const float*)data->X, data->n, data->d, (_Float16*)p, mb.p);
  if (hipGetLastError() != hipSuccess) return give_up();
  if (hipMemcpyAsync(bits, mb.p, 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return give_up();
  if (stream_sync(ctx->stream) != hipSuccess) return give_up();
  double mabs, mn2;
  std::memcpy(&mabs, &bits[0], 8);
  std::memcpy(&mn2, &bits[1], 8);
  if (!(mabs < 6.0e4)) return give_up();  // beyond the half range (or NaN / inf)
  if (data->max_norm < 0.0) {             // f32 data: no f32 shadow pass has measured the norms
    if (data->max_norm == -2.0) return give_up();
    data->max_norm = std::sqrt(mn2) * (1.0 + 1e-12);
    if (!(data->max_norm < 1e18)) return give_up();
  }
  data->shadow16 = (uint16_t*)p;
  data->shadow16_state = 1;
  return RPT_OK;
}

// int8 shadow (Sh8): pass 1 = the largest |element| (bits in max_bits[0]; NaN / inf -> +inf)
template <class TIn>
__global__ __launch_bounds__(256) void maxabs_kernel(const TIn* __restrict__ X, int64_t count,
                                                     unsigned long long* __restrict__ max_bits) {
  double mx = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const double a = fabs((double)ld<TIn>(X + i));
    if (!(a <= mx)) mx = a == a ? a : __longlong_as_double(0x7ff0000000000000LL);
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(mx, o);
    mx = t > mx ? t : mx;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(max_bits, (unsigned long long)__double_as_longlong(mx));
}
// pass 2 = the rows (one wave per row) and the largest squared row error |x - s c|^2 (max_bits[1])
template <class TIn>
__global__ __launch_bounds__(256) void shadow8_kernel(const TIn* __restrict__ X, int64_t n, int d, double s,
                                                      int8_t* __restrict__ X8,
                                                      unsigned long long* __restrict__ max_bits) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const double inv = 1.0 / s;
  double mx = 0.0;
  for (int64_t r = row0; r < n; r += (int64_t)gridDim.x * 4) {
    double e2 = 0.0;
    for (int j = lane; j < d; j += 64) {
      const double v = (double)ld<TIn>(X + r * d + j);
      double c = rint(v * inv);
      c = c < -127.0 ? -127.0 : (c > 127.0 ? 127.0 : c);
      X8[r * d + j] = (int8_t)(uint8_t)((int)c + 128);  // offset binary
      const double e = v - s * c;
      e2 += e * e;
    }
    for (int o = 32; o > 0; o >>= 1) e2 += __shfl_xor(e2, o);
    if (!(e2 <= mx)) mx = e2 == e2 ? e2 : __longlong_as_double(0x7ff0000000000000LL);
  }
  if (lane == 0) atomicMax(max_bits + 1, (unsigned long long)__double_as_longlong(mx));
}

// The int8 shadow, once per dataset; allowed to fail like the others (no memory, rows that are not a
// multiple of 16 elements, non-finite or all-zero data): the half tier then ranks.
static int32_t ensure_shadow8(rpt_ctx* ctx, const rpt_dataset* data) {
  if (data->shadow8_state != 0) return RPT_OK;
  data->shadow8_state = -1;
  void* p = nullptr;
  DevBuf<unsigned long long> mb;
  unsigned long long bits[2] = {0, 0};
  auto give_up = [&](const char* why = "") {
    if (ctx->opt.debug_host) fprintf(stderr, "int8 shadow: not built (%s)\n", why);
    if (p) dev_free(p);
    (void)hipGetLastError();
    return RPT_OK;
  };
  if (data->csr || data->n == 0 || (data->d % 16) != 0 || data->d > 16384)
    return give_up("CSR rows, or rows that are not a multiple of 16 elements");
  if (dev_alloc(&p, (size_t)data->n * data->d + 16) != hipSuccess) {
    p = nullptr;
    return give_up("no memory");
  }
  if (mb.alloc(2) != RPT_OK) return give_up();
  if (hipMemsetAsync(mb.p, 0, 16, ctx->stream) != hipSuccess) return give_up();
  const int64_t count = data->n * data->d;
  int64_t b1 = (count + 255) / 256;
  if (b1 > (int64_t)ctx->n_cu * 16) b1 = (int64_t)ctx->n_cu * 16;
  if (data->dtype == RPT_F64)
    hipLaunchKernelGGL(maxabs_kernel<double>, dim3((unsigned)b1), dim3(256), 0, ctx->stream,
                       (const double*)data->X, count, mb.p);
  else if (data->dtype == RPT_F32)
    hipLaunchKernelGGL(maxabs_kernel<float>, dim3((unsigned)b1), dim3(256), 0, ctx->stream,
                       (const float*)data->X, count, mb.p);
  else
    hipLaunchKernelGGL(maxabs_kernel<__hip_bfloat16>, dim3((unsigned)b1), dim3(256), 0, ctx->stream,
                       (const __hip_bfloat16*)data->X, count, mb.p);
  if (hipGetLastError() != hipSuccess) return give_up();
  if (hipMemcpyAsync(bits, mb.p, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return give_up();
  if (stream_sync(ctx->stream) != hipSuccess) return give_up();
  double mabs;
  std::memcpy(&mabs, &bits[0], 8);
  if (!(mabs > 0.0) || !(mabs < 1e150)) return give_up("max |x| is zero, huge or not finite");  // all zeros, NaN / inf, or no range left
  const double s = mabs / 127.0;
  if (!(s > 0.0) || !(1.0 / s < 1e300)) return give_up();
  int64_t blocks = (data->n + 3) / 4;
  if (blocks > (int64_t)ctx->n_cu * 16) blocks = (int64_t)ctx->n_cu * 16;
  if (data->dtype == RPT_F64)
    hipLaunchKernelGGL(shadow8_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       (const double*)data->X, data->n, data->d, s, (int8_t*)p, mb.p);
  else if (data->dtype == RPT_F32)
    hipLaunchKernelGGL(shadow8_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       (const float*)data->X, data->n, data->d, s, (int8_t*)p, mb.p);
  else
    hipLaunchKernelGGL(shadow8_kernel<__hip_bfloat16>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       (const __hip_bfloat16*)data->X, data->n, data->d, s, (int8_t*)p, mb.p);
  if (hipGetLastError() != hipSuccess) return give_up();
  if (hipMemcpyAsync(bits, mb.p, 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return give_up();
  if (stream_sync(ctx->stream) != hipSuccess) return give_up();
  double e2;
  std::memcpy(&e2, &bits[1], 8);
  if (!(e2 < 1e300)) return give_up("row error not finite");
  data->s8_scale = s;
  data->s8_emax = std::sqrt(e2) * (1.0 + 1e-9);  // (the butterfly sum of squares: a few ulp)
  data->shadow8 = (int8_t*)p;
  data->shadow8_state = 1;
  if (ctx->opt.debug_host)
    fprintf(stderr, "int8 shadow: scale %.6g (max |x| %.6g), max row error %.6g\n", s, mabs, data->s8_emax);
  return RPT_OK;
}

// The metrics' row norms dot(x, x), once per dataset (8 bytes per row, freed with it), followed by
// the two statistics of row_sqnorm_kernel (the certified cut's bound).  Unlike the shadows this is
// not optional: without it the metric cannot be evaluated or its cut certified.  Declared in
// common.h: the cosine kNN graph and its refinement (graph.hip, graph_refine.hip) read it too.
int32_t ensure_sqnorm(rpt_ctx* ctx, const rpt_dataset* data) {
  if (data->sqnorm) return RPT_OK;
  DevBuf<double> rn;
  RPT_TRY(rn.alloc((size_t)data->n + 2));
  unsigned long long* stats = reinterpret_cast<unsigned long long*>(rn.p + data->n);
  RPT_HIP(hipMemsetAsync(stats, 0, 16, ctx->stream));
  const unsigned blocks = (unsigned)((data->n + 255) / 256);
  if (blocks > 0) {
    if (data->csr && data->dtype == RPT_F64)  // (CSR rows: dotS(x, x), f64 or f32 values)
      hipLaunchKernelGGL(row_sqnorm_csr_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream, data->rowptr,
                         (const double*)data->val, data->n, rn.p, stats);
    else if (data->csr)
      hipLaunchKernelGGL(row_sqnorm_csr_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream, data->rowptr,
                         (const float*)data->val, data->n, rn.p, stats);
    else if (data->dtype == RPT_F64)
      hipLaunchKernelGGL(row_sqnorm_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream,
                         (const double*)data->X, data->n, data->d, rn.p, stats);
    else if (data->dtype == RPT_F32)
      hipLaunchKernelGGL(row_sqnorm_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream,
                         (const float*)data->X, data->n, data->d, rn.p, stats);
    else
      hipLaunchKernelGGL(row_sqnorm_kernel<__hip_bfloat16>, dim3(blocks), dim3(256), 0, ctx->stream,
                         (const __hip_bfloat16*)data->X, data->n, data->d, rn.p, stats);
    RPT_HIP(hipGetLastError());
  }
  data->sqnorm = rn.p;
  rn.p = nullptr;  // owned by the dataset now
  return RPT_OK;
}

static size_t metric_smem(int nbuf, int d) {
  return (sizeof(Entry) + 4) * (size_t)nbuf + (size_t)kMB * 16 + (size_t)d * 8;
}

// The metric kernels' list of uncertified queries (unc, [nq] ints, the caller's) and the context's
// count of them (read lazily by rpt_knn_last_uncertified: no read-back here)
static int32_t metric_unc_count(rpt_ctx* ctx, unsigned long long** p) {
  if (!ctx->metric_unc_dev) RPT_HIP(dev_alloc((void**)&ctx->metric_unc_dev, 8));
  *p = ctx->metric_unc_dev;
  return RPT_OK;
}

template <class TD, int METRIC, bool EXACT>
static int32_t launch_metric_v(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                               const int32_t* perm, const Range* ranges, const int64_t* rng_off, int T,
                               int identity, int k, int dedup, int32_t* unc, unsigned long long* unc_count,
                               int32_t* ids, double* dist, int32_t* cnt) {
  // buf holds the kept kk = k + kLfMargin (at most nbuf / 2) and one batch
  const int nbuf = k + kLfMargin + kMB <= 1024 ? 1024 : kBuf;
  const size_t smem = metric_smem(nbuf, data->d);
  RPT_ARG(smem <= 150 * 1024, "d too large");
  // the exact variant strides over its list of queries (blocks beyond its length return at once)
  int64_t grid = q->n;
  if (EXACT && grid > (int64_t)ctx->n_cu * 4) grid = (int64_t)ctx->n_cu * 4;
  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  RPT_HIP(launch_dyn(knn_metric_kernel<TD, METRIC, EXACT>, dim3((unsigned)grid), dim3(256), smem,
                     ctx->stream, (const TD*)data->X, data->d, (const TD*)q->X, q->n, perm, ranges, rng_off, T,
                     data->n, identity, nbuf, k, dedup, METRIC == kMetricL2 ? nullptr : (const double*)data->sqnorm,
                     METRIC == kMetricL2 ? nullptr
                                         : reinterpret_cast<const unsigned long long*>(data->sqnorm + data->n),
                     unc, unc_count, ids, dist, cnt));
  return RPT_OK;
}

// the fast kernel, then the exact one over the queries it could not certify (all of them with
// knn_metric_exact); ctx->last_uncertified follows
template <class TD, int METRIC>
static int32_t launch_metric_t(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                               const int32_t* perm, const Range* ranges, const int64_t* rng_off, int T,
                               int identity, int k, int dedup, int32_t* unc, int32_t* ids, double* dist,
                               int32_t* cnt) {
  unsigned long long* uc = nullptr;
  RPT_TRY(metric_unc_count(ctx, &uc));
  if (ctx->opt.knn_metric_exact) {
    unc = nullptr;  // every query
    ctx->last_uncertified = q->n;
    ctx->metric_unc_pending = false;
  } else {
    RPT_HIP(hipMemsetAsync(uc, 0, 8, ctx->stream));
    RPT_TRY((launch_metric_v<TD, METRIC, false>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup, unc,
                                                uc, ids, dist, cnt)));
    ctx->metric_unc_pending = true;
  }
  return launch_metric_v<TD, METRIC, true>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup, unc, uc,
                                           ids, dist, cnt);
}

// Dense f64 rows under L2 over a query plan or, with identity, the whole dataset (the brute force):
// topk_dense_kernel ranks on butterfly sums and lists the queries whose cut it cannot certify, the
// exact kernel answers those again (all of them, alone, with knn_l2_exact).  The count is read
// lazily (rpt_knn_last_uncertified).  unc: [q->n] ints of device scratch that lives until the kernels are done.
static int32_t launch_l2_f64(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, const int32_t* perm,
                             const Range* ranges, const int64_t* rng_off, int T, int identity, int k, int dedup,
                             int32_t* unc, int32_t* ids, double* dist, int32_t* cnt) {
  unsigned long long* uc = nullptr;
  RPT_TRY(metric_unc_count(ctx, &uc));
  if (ctx->opt.knn_l2_exact) {
    unc = nullptr;  // every query
    ctx->last_uncertified = q->n;
    ctx->metric_unc_pending = false;
  } else {
    RPT_HIP(hipMemsetAsync(uc, 0, 8, ctx->stream));
    RPT_TRY(launch_topk_dense<double>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup, ids, dist, cnt,
                                      unc, uc));
    ctx->metric_unc_pending = true;
  }
  return launch_metric_v<double, kMetricL2, true>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup, unc,
                                                  uc, ids, dist, cnt);
}

// the queries a fused launch flagged 2 (a cut that could not be certified), as the exact kernel's list
__global__ __launch_bounds__(256) void collect_flagged_kernel(const unsigned int* __restrict__ flags, int64_t nq,
                                                              int32_t* __restrict__ unc,
                                                              unsigned long long* __restrict__ unc_count) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < nq && flags[q] == 2u) unc[atomicAdd(unc_count, 1ULL)] = (int32_t)q;
}

template <class TD>
static int32_t launch_metric_td(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                                const int32_t* perm, const Range* ranges, const int64_t* rng_off, int T,
                                int identity, int k, int dedup, int metric, int32_t* unc, int32_t* ids,
                                double* dist, int32_t* cnt) {
  if (metric == RPT_KNN_METRIC_COSINE)
    return launch_metric_t<TD, kMetricCosine>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup,
                                              unc, ids, dist, cnt);
  return launch_metric_t<TD, kMetricInner>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup, unc,
                                           ids, dist, cnt);
}

// the cosine / inner-product kernels over the query plan (batch and streamed forests alike) or, with
// identity, over the whole dataset (brute force; ties by id).  unc: [q->n] ints of device scratch
// that lives until the kernels are done.
static int32_t launch_metric(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                             const int32_t* perm, const Range* ranges, const int64_t* rng_off, int T,
                             int identity, int k, int dedup, int metric, int32_t* unc, int32_t* ids,
                             double* dist, int32_t* cnt) {
  RPT_TRY(ensure_sqnorm(ctx, data));
  if (data->dtype == RPT_F64)
    return launch_metric_td<double>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup, metric, unc,
                                    ids, dist, cnt);
  if (data->dtype == RPT_F32)
    return launch_metric_td<float>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup, metric, unc,
                                   ids, dist, cnt);
  return launch_metric_td<__hip_bfloat16>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup,
                                          metric, unc, ids, dist, cnt);
}

static int32_t knn_metric(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q,
                          int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  ctx->last_uncertified = 0;
  ctx->metric_unc_pending = false;
  ctx->last_retries = 0;
  ctx->last_tier = 0;
  QueryPlan pl;
  RPT_TRY(make_plan(ctx, f, q, pl));
  ctx->last_candidates = pl.total_cand;
  if (q->n == 0) return RPT_OK;
  DevBuf<int32_t> unc;
  RPT_TRY(unc.alloc((size_t)q->n));
  RPT_TRY(launch_metric(ctx, data, q, f->perm.p, pl.ranges.p, pl.rng_off.p, f->T, 0, k, flags & 3,
                        flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER), unc.p, ids_dev, dist_dev,
                        count_dev));
  RPT_HIP(stream_sync(ctx->stream));  // the plan's buffers are released on return
  return RPT_OK;
}

// ---- cosine / inner product on CSR rows: knn_metric_csr_kernel's launchers (as launch_metric_*) ----
template <class TD, int METRIC, bool EXACT>
static int32_t launch_metric_csr_v(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                                   const int32_t* perm, const Range* ranges, const int64_t* rng_off, int T,
                                   int identity, int k, int dedup, int32_t* unc, unsigned long long* unc_count,
                                   int32_t* ids, double* dist, int32_t* cnt) {
  const int nbuf = k + kLfMargin + kMB <= 1024 ? 1024 : kBuf;
  const size_t smem = metric_smem(nbuf, data->d) + (size_t)((data->d + 31) / 32) * 4;
  RPT_ARG(smem <= 150 * 1024, "d too large");
  int64_t grid = q->n;
  if (EXACT && grid > (int64_t)ctx->n_cu * 4) grid = (int64_t)ctx->n_cu * 4;
  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  RPT_HIP(launch_dyn(knn_metric_csr_kernel<TD, METRIC, EXACT>, dim3((unsigned)grid), dim3(256), smem, ctx->stream,
                     data->rowptr, data->col, (const TD*)data->val, data->nnz, data->d, q->rowptr, q->col,
                     (const TD*)q->val, q->n, perm, ranges, rng_off, T, data->n, identity, nbuf, k, dedup,
                     (const double*)data->sqnorm,
                     reinterpret_cast<const unsigned long long*>(data->sqnorm + data->n), unc, unc_count, ids,
                     dist, cnt));
  return RPT_OK;
}

template <class TD, int METRIC>
static int32_t launch_metric_csr_t(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                                   const int32_t* perm, const Range* ranges, const int64_t* rng_off, int T,
                                   int identity, int k, int dedup, int32_t* unc, int32_t* ids, double* dist,
                                   int32_t* cnt) {
  unsigned long long* uc = nullptr;
  RPT_TRY(metric_unc_count(ctx, &uc));
  if (ctx->opt.knn_metric_exact) {
    unc = nullptr;  // every query
    ctx->last_uncertified = q->n;
    ctx->metric_unc_pending = false;
  } else {
    RPT_HIP(hipMemsetAsync(uc, 0, 8, ctx->stream));
    RPT_TRY((launch_metric_csr_v<TD, METRIC, false>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup,
                                                    unc, uc, ids, dist, cnt)));
    ctx->metric_unc_pending = true;
  }
  return launch_metric_csr_v<TD, METRIC, true>(ctx, data, q, perm, ranges, rng_off, T, identity, k, dedup, unc, uc,
                                               ids, dist, cnt);
}

// CSR rows and CSR queries under RPT_KNN_METRIC_COSINE / _INNER over the query plan or, identity, the
// whole dataset (the brute force: ties by id).  unc: [q->n] ints of device scratch, as launch_metric's.
static int32_t launch_metric_csr(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                                 const int32_t* perm, const Range* ranges, const int64_t* rng_off, int T,
                                 int identity, int k, int dedup, int metric, int32_t* unc, int32_t* ids,
                                 double* dist, int32_t* cnt) {
  RPT_ARG(data->n <= 0x7fffffff, "too many rows");
  RPT_TRY(ensure_sqnorm(ctx, data));
  const bool cosine = metric == RPT_KNN_METRIC_COSINE;
  if (data->dtype == RPT_F64)
    return cosine ? launch_metric_csr_t<double, kMetricCosine>(ctx, data, q, perm, ranges, rng_off, T, identity, k,
                                                               dedup, unc, ids, dist, cnt)
                  : launch_metric_csr_t<double, kMetricInner>(ctx, data, q, perm, ranges, rng_off, T, identity, k,
                                                              dedup, unc, ids, dist, cnt);
  return cosine ? launch_metric_csr_t<float, kMetricCosine>(ctx, data, q, perm, ranges, rng_off, T, identity, k,
                                                            dedup, unc, ids, dist, cnt)
                : launch_metric_csr_t<float, kMetricInner>(ctx, data, q, perm, ranges, rng_off, T, identity, k,
                                                           dedup, unc, ids, dist, cnt);
}

// (u16 column, f32 value) shadow of a CSR f64 dataset, its largest squared row norm and longest row
__global__ __launch_bounds__(256) void shadow_csr_kernel(const int64_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const double* __restrict__ val, int64_t n,
                                                         int64_t nnz, uint16_t* __restrict__ col16,
                                                         float* __restrict__ val32,
                                                         unsigned long long* __restrict__ max_bits) {
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = gtid; j < nnz; j += gsz) {
    col16[j] = (uint16_t)col[j];
    val32[j] = (float)val[j];
  }
  double mx = 0.0;
  long long ml = 0;
  for (int64_t r = gtid; r < n; r += gsz) {  // rows are short (SVectors): one thread per row
    const int64_t a = rowptr[r], b = rowptr[r + 1];
    double s2 = 0.0;
    for (int64_t j = a; j < b; ++j) s2 += val[j] * val[j];
    if (!(s2 <= mx)) mx = s2 == s2 ? s2 : __longlong_as_double(0x7ff0000000000000LL);  // NaN -> +inf
    if (b - a > ml) ml = b - a;
  }
  atomicMax(max_bits, (unsigned long long)__double_as_longlong(mx));  // mx >= 0
  atomicMax(max_bits + 1, (unsigned long long)ml);
}

// Built once per dataset, like the dense shadow: an optimisation that is allowed to fail (no
// memory, NaN rows, squares outside the f32 range): the dataset is then marked and the exact
// kernel answers.
static int32_t ensure_shadow_csr(rpt_ctx* ctx, const rpt_dataset* data) {
  if (data->shadow_col16 || data->max_norm == -2.0) return RPT_OK;
  void *pc = nullptr, *pv = nullptr;
  DevBuf<unsigned long long> mb;
  unsigned long long bits[2] = {0, 0};
  auto give_up = [&]() {
    if (pc) dev_free(pc);
    if (pv) dev_free(pv);
    (void)hipGetLastError();
    data->max_norm = -2.0;
    return RPT_OK;
  };
  const size_t nz = (size_t)(data->nnz > 0 ? data->nnz : 1);
  if (dev_alloc(&pc, nz * 2 + 16) != hipSuccess) {
    pc = nullptr;
    return give_up();
  }
  if (dev_alloc(&pv, nz * 4 + 16) != hipSuccess) {
    pv = nullptr;
    return give_up();
  }
  if (mb.alloc(2) != RPT_OK) return give_up();
  if (hipMemsetAsync(mb.p, 0, 16, ctx->stream) != hipSuccess) return give_up();
  hipLaunchKernelGGL(shadow_csr_kernel, dim3((unsigned)ctx->n_cu * 8), dim3(256), 0, ctx->stream,
                     data->rowptr, data->col, (const double*)data->val, data->n, data->nnz,
                     (uint16_t*)pc, (float*)pv, mb.p);
  if (hipGetLastError() != hipSuccess) return give_up();
  if (hipMemcpyAsync(bits, mb.p, 16, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    return give_up();
  if (stream_sync(ctx->stream) != hipSuccess) return give_up();
  double m2;
  std::memcpy(&m2, &bits[0], 8);
  data->max_norm = std::sqrt(m2) * (1.0 + 1e-12);
  if (!(data->max_norm < 1e18)) return give_up();
  data->max_rowlen = (int64_t)bits[1];
  data->shadow32 = (float*)pv;
  data->shadow_col16 = (uint16_t*)pc;
  return RPT_OK;
}

// CSR f64 rows: largest squared row norm, longest row, largest |value| (one thread per row)
__global__ __launch_bounds__(256) void csr_stats_kernel(const int64_t* __restrict__ rowptr,
                                                        const double* __restrict__ val, int64_t n,
                                                        unsigned long long* __restrict__ max_bits) {
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double mx = 0.0, ma = 0.0;
  long long ml = 0;
  for (int64_t r = gtid; r < n; r += gsz) {
    const int64_t a = rowptr[r], b = rowptr[r + 1];
    double s2 = 0.0;
    for (int64_t j = a; j < b; ++j) {
      const double v = val[j], av = fabs(v);
      s2 += v * v;
      if (!(av <= ma)) ma = av == av ? av : inf;
    }
    if (!(s2 <= mx)) mx = s2 == s2 ? s2 : inf;  // NaN -> +inf
    if (b - a > ml) ml = b - a;
  }
  atomicMax(max_bits, (unsigned long long)__double_as_longlong(mx));
  atomicMax(max_bits + 1, (unsigned long long)ml);
  atomicMax(max_bits + 2, (unsigned long long)__double_as_longlong(ma));
}

// the fixed-width half table: sixteen lanes per row, a lane writes whole 16-byte chunks
__global__ __launch_bounds__(256) void ell_fill_kernel(const int64_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col,
                                                       const double* __restrict__ val, int64_t n,
                                                       int W, uint32_t* __restrict__ ell) {
  const int l16 = threadIdx.x & 15;
  const int chunks = W >> 2;
  for (int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); r < n; r += (int64_t)gridDim.x * 16) {
    const int64_t a = rowptr[r], b = rowptr[r + 1];
    uint4* out = reinterpret_cast<uint4*>(ell + r * W);
    for (int c = l16; c < chunks; c += 16) {
      unsigned int w4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t j = a + 4 * (int64_t)c + e;
        w4[e] = 0u;
        if (j < b) {
          const _Float16 h = (_Float16)(float)val[j];
          unsigned short hb;
          __builtin_memcpy(&hb, &h, 2);
          w4[e] = (unsigned int)col[j] | ((unsigned int)hb << 16);
        }
      }
      out[c] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    }
  }
}

// The half tier's table of a CSR f64 dataset, once per dataset; allowed to fail (no memory, values
// beyond the half range, rows so uneven that the padding would exceed twice the nonzeros).
static int32_t ensure_shadow_ell(rpt_ctx* ctx, const rpt_dataset* data) {
  if (data->ell_state != 0) return RPT_OK;
  data->ell_state = -1;
  if (!data->csr || data->dtype != RPT_F64 || data->d > 65536 || data->n == 0 ||
      data->max_norm == -2.0)
    return RPT_OK;
  void* p = nullptr;
  DevBuf<unsigned long long> mb;
  unsigned long long bits[3] = {0, 0, 0};
  auto give_up = [&]() {
    if (p) dev_free(p);
    (void)hipGetLastError();
    return RPT_OK;
  };
  if (mb.alloc(3) != RPT_OK) return give_up();
  if (hipMemsetAsync(mb.p, 0, 24, ctx->stream) != hipSuccess) return give_up();
  hipLaunchKernelGGL(csr_stats_kernel, dim3((unsigned)ctx->n_cu * 8), dim3(256), 0, ctx->stream,
                     data->rowptr, (const double*)data->val, data->n, mb.p);
  if (hipGetLastError() != hipSuccess) return give_up();
  if (hipMemcpyAsync(bits, mb.p, 24, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return give_up();
  if (stream_sync(ctx->stream) != hipSuccess) return give_up();
  double m2, mabs;
  std::memcpy(&m2, &bits[0], 8);
  std::memcpy(&mabs, &bits[2], 8);
  const double mn = std::sqrt(m2) * (1.0 + 1e-12);
  if (!(mn < 1e18) || !(mabs < 6.0e4)) return give_up();
  const int64_t W = (((int64_t)bits[1] + 3) & ~(int64_t)3) > 4 ? (((int64_t)bits[1] + 3) & ~(int64_t)3) : 4;
  if (W > 4096 || (double)data->n * (double)W > 3.0 * (double)data->nnz + 1048576.0) return give_up();
  if (dev_alloc(&p, (size_t)data->n * (size_t)W * 4 + 16) != hipSuccess) {
    p = nullptr;
    return give_up();
  }
  int64_t blocks = (data->n + 15) / 16;
  if (blocks > (int64_t)ctx->n_cu * 32) blocks = (int64_t)ctx->n_cu * 32;
  hipLaunchKernelGGL(ell_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, data->rowptr,
                     data->col, (const double*)data->val, data->n, (int)W, (uint32_t*)p);
  if (hipGetLastError() != hipSuccess) return give_up();
  if (stream_sync(ctx->stream) != hipSuccess) return give_up();
  if (data->max_norm < 0.0) data->max_norm = mn;
  if (data->max_rowlen == 0) data->max_rowlen = (int64_t)bits[1];
  data->shadow_ell = (uint32_t*)p;
  data->ell_w = (int)W;
  data->ell_state = 1;
  return RPT_OK;
}

// what fused_shadows_wanted and fused_plan read of a call (knn_plan.h)
static void fused_input_shadows(FusedIn& in, const rpt_dataset* data) {
  in.shadow8 = data->shadow8 != nullptr;
  in.shadow16 = data->shadow16 != nullptr;
  in.shadow32 = data->shadow32 != nullptr;
  in.shadow_col16 = data->shadow_col16 != nullptr;
  in.shadow_ell = data->shadow_ell != nullptr;
}

static FusedIn fused_input(const rpt_ctx* ctx, const rpt_forest* f, const rpt_dataset* data, int k, int dedup,
                           int vote) {
  const auto elem = [](int32_t dt) { return dt == RPT_F64 ? Elem::F64 : dt == RPT_F32 ? Elem::F32 : Elem::BF16; };
  FusedIn in;
  in.elem = elem(data->dtype);
  in.proj = elem(f->pdtype);
  in.csr = data->csr;
  in.d = data->d;
  in.k = k;
  in.dedup = dedup;
  in.vote = vote;
  in.T = f->T;
  in.L = f->L;
  in.min_leaf = f->min_leaf;
  in.n = f->n;
  in.tiers = f->tiers;
  fused_input_options(in, ctx->opt);
  fused_input_shadows(in, data);
  return in;
}

// launches what the plan says: one kernel (the shard family: its traversal kernel first)
template <class TD, class TK>
static int32_t launch_fused(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q,
                            const void* Pq, const FusedIn& in, const FusedPlan& p, int32_t* ids, double* dist,
                            int32_t* cnt, unsigned int* ovf, unsigned long long* cand_total) {
  constexpr bool kF64 = std::is_same<TD, double>::value, kBf16 = std::is_same<TD, __hip_bfloat16>::value;
  const int k = in.k, dedup = in.dedup | in.vote << 8;  // (the kernels take the vote threshold with the duplicate rule)
  // debug_stamps: phase clocks of one wave of the wave kernel, printed after the launch
  DevBuf<unsigned long long> dbgdev;
  unsigned long long* dbg = nullptr;
  if (ctx->opt.debug_stamps && dbgdev.alloc(64) == RPT_OK) {
    (void)hipMemsetAsync(dbgdev.p, 0, 64 * 8, ctx->stream);
    dbg = dbgdev.p;
  }
  struct DbgPrint {
    rpt_ctx* ctx;
    unsigned long long* p;
    ~DbgPrint() {
      if (!p) return;
      unsigned long long hs[64];
      (void)stream_sync(ctx->stream);
      if (hipMemcpy(hs, p, sizeof(hs), hipMemcpyDeviceToHost) != hipSuccess) return;
      for (int i = 1; i < 64 && hs[i]; ++i) fprintf(stderr, "knn wave stamp %d: +%llu\n", i, hs[i] - hs[i - 1]);
    }
  } dbgprint{ctx, nullptr};
  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  // what a dense tier ranks on (CSR rows: see CsrPtrs) and what its certificate reads
  const void* shadow = data->csr || p.tier == 0 ? nullptr
                       : p.tier == 3            ? (const void*)data->shadow8
                       : p.tier == 2            ? (const void*)data->shadow16
                                                : (const void*)data->shadow32;
  const double xmax = p.tier > 0 ? data->max_norm : 0.0;
  const Sh8 s8 = p.tier == 3 ? Sh8{data->s8_scale, data->s8_emax} : Sh8{0.0, 0.0};
  const dim3 block(256);
  // (the if constexpr guards: which instantiations exist — bf16 rows have no wave or shard tiers and
  // no CSR form, f32 rows no CSR shadow; the plan never asks for one of those)
  switch (p.family) {
    case Family::Shard:
      // round 4: traversal as its own launch, exact distances for an adaptive certified set
      // (shard_ranges_kernel / knn_shard_wave_kernel)
      if constexpr (!kBf16) {
        const int64_t nq = q->n;
        DevBuf<int2> hdr;
        DevBuf<int64_t> roff;
        DevBuf<int> rlen;
        RPT_TRY(hdr.alloc((size_t)nq));
        RPT_TRY(roff.alloc((size_t)nq * kWR));
        RPT_TRY(rlen.alloc((size_t)nq * kWR));
        const int qpw = 64 / f->T;
        hipLaunchKernelGGL(shard_ranges_kernel<TK>, dim3((unsigned)((nq + 4 * qpw - 1) / (4 * qpw))), block, 0,
                           ctx->stream, f->thr.p, f->mglo.p, f->mghi.p, f->nodes, (const TK*)Pq, nq, f->T, f->L,
                           f->min_leaf, f->n, hdr.p, roff.p, rlen.p, ovf + 1, ovf, cand_total);
        RPT_HIP(hipGetLastError());
        auto kern = p.tier == 3   ? (p.one_batch ? knn_shard_wave_kernel<TD, 3, 128, 4, 512> : knn_shard_wave_kernel<TD, 3, 256, 3, 640>)
                    : p.tier == 2 ? (p.one_batch ? knn_shard_wave_kernel<TD, 2, 128, 4, 512> : knn_shard_wave_kernel<TD, 2, 256, 3, 640>)
                                  : (p.one_batch ? knn_shard_wave_kernel<TD, 1, 128, 4, 512> : knn_shard_wave_kernel<TD, 1, 256, 3, 640>);
        const int r1_pct = 110;  // (100 / 110 / 130 measured: 0.281 / 0.279 / 0.283 ms per 10 000 queries)
        dbgprint.p = dbg;
        RPT_HIP(launch_dyn(kern, dim3((unsigned)((nq + 3) / 4)), block, p.smem, ctx->stream, (const TD*)data->X,
                           data->d, (const TD*)q->X, f->perm.p, nq, k, hdr.p, roff.p, rlen.p, ids, dist, cnt,
                           ovf + 1, cand_total, shadow, xmax, s8, r1_pct, dbg));
        return RPT_OK;
      }
      break;
    case Family::Wave: {
      decltype(&knn_fused_wave_kernel<TD, TK, false>) kern = nullptr;
      if constexpr (!kBf16) {
        if (p.tier > 0) kern = p.tier == 3 ? knn_fused_wave_kernel<TD, TK, true, true> : knn_fused_wave_kernel<TD, TK, true, false>;
      }
      if (p.tier == 0) kern = knn_fused_wave_kernel<TD, TK, false>;
      if (!kern) break;
      dbgprint.p = dbg;
      RPT_HIP(launch_dyn(kern, dim3((unsigned)((q->n + 3) / 4)), block, p.smem, ctx->stream, (const TD*)data->X,
                         data->d, (const TD*)q->X, f->perm.p, f->thr.p, f->mglo.p, f->mghi.p, f->nodes,
                         (const TK*)Pq, q->n, f->T, f->L, f->min_leaf, f->n, k, dedup, ids, dist, cnt, ovf + 1, ovf,
                         cand_total, shadow, xmax, p.k1, dbg, p.sh16 ? 1 : 0, s8));
      return RPT_OK;
    }
    case Family::Workgroup: {
      // dense rows, every distance exact; or ranked on a shadow (f32 rows: their half / int8 one, bf16
      // rows: their int8 one); SVector rows: the same kernel, distances over CSR rows, exact or ranked
      // on their half table / (u16, f32) shadow
      decltype(&knn_fused_kernel<TD, TK, false>) kern = nullptr;
      if constexpr (kF64) {
        if (data->csr && p.tier > 0) kern = knn_fused_kernel<TD, TK, true, true>;
      }
      if (!data->csr && p.tier > 0)
        kern = p.tier == 3 ? knn_fused_kernel<TD, TK, true, false, true> : knn_fused_kernel<TD, TK, true, false, false>;
      if constexpr (!kBf16) {
        if (data->csr && p.tier == 0) kern = knn_fused_kernel<TD, TK, false, true>;
      }
      if (!data->csr && p.tier == 0) kern = knn_fused_kernel<TD, TK, false>;
      if (!kern) break;
      const CsrPtrs cp = data->csr ? CsrPtrs{data->rowptr, data->col, data->val, data->nnz, q->rowptr, q->col, q->val,
                                             data->shadow_col16, data->shadow32,
                                             p.csr_rank == CsrRank::Ell ? (int64_t)data->ell_w : data->max_rowlen,
                                             data->shadow_ell, data->ell_w}
                                   : CsrPtrs{};
      // (the stamps of the workgroup kernel: dense f64 rows on a ranking tier)
      unsigned long long* wdbg = kF64 && !data->csr && p.tier > 0 ? dbg : nullptr;
      dbgprint.p = wdbg;
      RPT_HIP(launch_dyn(kern, dim3((unsigned)q->n), block, p.smem, ctx->stream, (const TD*)data->X, data->d,
                         (const TD*)q->X, f->perm.p, f->thr.p, f->mglo.p, f->mghi.p, f->nodes, (const TK*)Pq, q->n,
                         f->T, f->L, f->min_leaf, f->n, k, dedup, ids, dist, cnt, ovf + 1, ovf, cand_total, shadow,
                         xmax, p.k1, cp, p.sh16 ? 1 : 0, s8, wdbg));
      return RPT_OK;
    }
  }
  return fail(RPT_E_UNSUPPORTED, "fused kNN: no kernel for the plan");
}

static int32_t knn_general(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                           const rpt_dataset* q, int32_t k, int32_t flags, int32_t* ids_dev,
                           double* dist_dev, int32_t* count_dev) {
  QueryPlan pl;
  RPT_TRY(make_plan(ctx, f, q, pl));
  ctx->last_candidates = pl.total_cand;
  if (q->n == 0) return RPT_OK;
  const int dedup = flags & 3;
  const int refm = (flags & RPT_KNN_METRIC_REFERENCE) ? 1 : 0;
  DevBuf<int32_t> unc;  // dense f64 rows: the queries the exact kernel answers again (launch_l2_f64)
  if (data->csr) {
    const size_t smem = topk_smem(data->d, 8);
    ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
    if (data->dtype == RPT_F64) {
      RPT_HIP(launch_dyn(topk_csr_kernel<double>, dim3((unsigned)q->n), dim3(256), smem,
                         ctx->stream, data->rowptr, data->col, (const double*)data->val, data->nnz, data->d,
                         q->rowptr, q->col, (const double*)q->val, f->perm.p, pl.ranges.p,
                         pl.rng_off.p, f->T, k, dedup, refm, ids_dev, dist_dev, count_dev));
    } else {
      RPT_HIP(launch_dyn(topk_csr_kernel<float>, dim3((unsigned)q->n), dim3(256), smem,
                         ctx->stream, data->rowptr, data->col, (const float*)data->val, data->nnz, data->d,
                         q->rowptr, q->col, (const float*)q->val, f->perm.p, pl.ranges.p,
                         pl.rng_off.p, f->T, k, dedup, refm, ids_dev, dist_dev, count_dev));
    }
  } else if (data->dtype == RPT_F64) {
    RPT_TRY(unc.alloc((size_t)q->n));
    RPT_TRY(launch_l2_f64(ctx, data, q, f->perm.p, pl.ranges.p, pl.rng_off.p, f->T, 0, k, dedup, unc.p, ids_dev,
                          dist_dev, count_dev));
  } else if (data->dtype == RPT_F32) {
    RPT_TRY(launch_topk_dense<float>(ctx, data, q, f->perm.p, pl.ranges.p, pl.rng_off.p, f->T, 0,
                                     k, dedup, ids_dev, dist_dev, count_dev));
  } else {
    RPT_TRY(launch_topk_dense<__hip_bfloat16>(ctx, data, q, f->perm.p, pl.ranges.p, pl.rng_off.p,
                                              f->T, 0, k, dedup, ids_dev, dist_dev, count_dev));
  }
  RPT_HIP(stream_sync(ctx->stream));  // the plan's buffers are released on return
  return RPT_OK;
}

// ---- what the list routes (rpt_knn_vote_*, rpt_knn_allow_*, rpt_brute_knn_allow_*) share ----
// queries q0 .. q0 + ns - 1 as a dataset of their own (a view: nothing is owned, no cache is read)
static rpt_dataset query_view(const rpt_dataset* q, int64_t q0, int64_t ns) {
  rpt_dataset qv = *q;
  qv.owns = false;
  qv.n = ns;
  if (q->csr) qv.rowptr = q->rowptr + q0;  // (rowptr holds absolute offsets into col / val)
  else qv.X = static_cast<char*>(q->X) + (size_t)q0 * q->d * dtype_size(q->dtype);
  return qv;
}

// The general launcher of the (row layout, dtype, distance) cell over lists made by a list step:
// `lists` takes perm's place, every query has one range (T := 1).  dedup: the duplicate rule (0 .. 2);
// metric: 0 or RPT_KNN_METRIC_COSINE / _INNER; refm: CSR rows under the reference's metricSSL2.
// unc: [q->n] ints of device scratch.  ctx->last_uncertified / metric_unc_pending follow the launch.
static int32_t launch_lists(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, const int32_t* lists,
                            const Range* rg, const int64_t* ro, int k, int dedup, int metric, int refm,
                            int32_t* unc, int32_t* ids, double* dist, int32_t* cnt) {
  ctx->last_uncertified = 0;
  ctx->metric_unc_pending = false;
  if (data->csr && metric) return launch_metric_csr(ctx, data, q, lists, rg, ro, 1, 0, k, dedup, metric, unc, ids, dist, cnt);
  if (data->csr) {
    const size_t smem = topk_smem(data->d, 8);
    ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
    if (data->dtype == RPT_F64)
      RPT_HIP(launch_dyn(topk_csr_kernel<double>, dim3((unsigned)q->n), dim3(256), smem, ctx->stream, data->rowptr,
                         data->col, (const double*)data->val, data->nnz, data->d, q->rowptr, q->col,
                         (const double*)q->val, lists, rg, ro, 1, k, dedup, refm, ids, dist, cnt));
    else
      RPT_HIP(launch_dyn(topk_csr_kernel<float>, dim3((unsigned)q->n), dim3(256), smem, ctx->stream, data->rowptr,
                         data->col, (const float*)data->val, data->nnz, data->d, q->rowptr, q->col,
                         (const float*)q->val, lists, rg, ro, 1, k, dedup, refm, ids, dist, cnt));
    return RPT_OK;
  }
  if (metric) return launch_metric(ctx, data, q, lists, rg, ro, 1, 0, k, dedup, metric, unc, ids, dist, cnt);
  if (data->dtype == RPT_F64) return launch_l2_f64(ctx, data, q, lists, rg, ro, 1, 0, k, dedup, unc, ids, dist, cnt);
  if (data->dtype == RPT_F32) return launch_topk_dense<float>(ctx, data, q, lists, rg, ro, 1, 0, k, dedup, ids, dist, cnt);
  return launch_topk_dense<__hip_bfloat16>(ctx, data, q, lists, rg, ro, 1, 0, k, dedup, ids, dist, cnt);
}

// the launchers count uncertified queries per launch: a sliced call adds its slices up
static int32_t add_uncertified(rpt_ctx* ctx, int64_t& uncertified) {
  if (ctx->metric_unc_pending) {
    unsigned long long n = 0;
    RPT_HIP(hipMemcpyAsync(&n, ctx->metric_unc_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
    RPT_HIP(stream_sync(ctx->stream));
    uncertified += (int64_t)n;
  } else {
    uncertified += ctx->last_uncertified;
  }
  return RPT_OK;
}

// ---- the vote threshold over the general kernels (rpt_knn_vote_*, rpt_vote_candidates_host) ----
// make_plan, then knn_vote.hip's vote-select step turns every query's leaf ranges into ONE range of
// a scratch id array (the ids at least v trees propose, ascending), then the launcher of the (row
// layout, dtype, distance) ranks those lists as it ranks any plan: perm := the voted ids, T := 1, no
// duplicate rule (the ids are distinct, so candidate position order is id order).
static_assert(sizeof(Range) == sizeof(VoteRange) && offsetof(Range, poff) == offsetof(VoteRange, poff) &&
                  offsetof(Range, n) == offsetof(VoteRange, n) && offsetof(Range, pos) == offsetof(VoteRange, pos),
              "knn_vote.h restates Range");

// Words of id and sort slabs one slice may hold (1 GiB; a single query above it is a slice of its
// own).  Fixed: scratch is sized from the plan and the options, never from the free memory.
constexpr int64_t kVoteBudgetWords = (int64_t)1 << 28;

struct VoteWork {
  QueryPlan pl;
  std::vector<int64_t> starts;    // [nq + 1] cand_off[q * T] on the host
  std::vector<VoteSlice> slices;
  DevBuf<int64_t> sort_off;       // [nq]: a large query's first word in the slice's sort slab
  DevBuf<int32_t> ids, counts, sort;
  DevBuf<Range> vranges;
  DevBuf<int64_t> vrng_off;
  DevBuf<unsigned long long> total;
  int lds_cap = kVoteLds;
};

static int64_t vote_pow2(int64_t n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// the plan, the slices and their scratch (sized for the largest slice)
static int32_t vote_prepare(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* q, bool want_counts, VoteWork& w) {
  RPT_TRY(make_plan(ctx, f, q, w.pl));
  const int64_t nq = q->n;
  RPT_TRY(w.total.alloc(1));
  RPT_HIP(hipMemsetAsync(w.total.p, 0, 8, ctx->stream));
  if (nq == 0) return RPT_OK;
  w.lds_cap = ctx->opt.knn_vote_lds > 0 && ctx->opt.knn_vote_lds < kVoteLds ? (int)ctx->opt.knn_vote_lds : kVoteLds;
  const int64_t max_q = ctx->opt.knn_vote_slice > 0 ? ctx->opt.knn_vote_slice : 0x7fffffff;
  DevBuf<int64_t> starts_dev;
  RPT_TRY(starts_dev.alloc((size_t)nq + 1));
  RPT_TRY(vote_query_starts(ctx, w.pl.cand_off.p, f->T, nq, starts_dev.p));
  w.starts.resize((size_t)nq + 1);
  RPT_HIP(hipMemcpyAsync(w.starts.data(), starts_dev.p, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  RPT_HIP(stream_sync(ctx->stream));
  std::vector<int64_t> so((size_t)nq, 0);
  VoteSlice cur;
  int64_t max_cand = 1, max_sort = 1, max_ns = 1;
  auto close = [&]() {
    if (cur.ns == 0) return;
    w.slices.push_back(cur);
    max_cand = std::max(max_cand, cur.cand_words);
    max_sort = std::max(max_sort, cur.sort_words);
    max_ns = std::max(max_ns, cur.ns);
  };
  for (int64_t i = 0; i < nq; ++i) {
    const int64_t nc = w.starts[i + 1] - w.starts[i];
    RPT_ARG(nc <= 0x7fffffff, "a query has more candidates than an int32 holds");
    const int64_t sw = nc > w.lds_cap ? vote_pow2(nc) : 0;
    if (cur.ns > 0 && (cur.ns >= max_q || cur.cand_words + cur.sort_words + nc + sw > kVoteBudgetWords)) {
      close();
      cur = VoteSlice();
    }
    if (cur.ns == 0) cur.q0 = i;
    so[i] = cur.sort_words;
    cur.ns += 1;
    cur.cand_words += nc;
    cur.sort_words += sw;
    if (sw == 0 && nc > 0) cur.lds_words = std::max(cur.lds_words, (int)vote_pow2(nc));
  }
  close();
  RPT_TRY(w.sort_off.alloc((size_t)nq));
  RPT_HIP(hipMemcpyAsync(w.sort_off.p, so.data(), (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
  RPT_HIP(stream_sync(ctx->stream));  // (so is a local)
  RPT_TRY(w.ids.alloc((size_t)max_cand));
  if (want_counts) RPT_TRY(w.counts.alloc((size_t)max_cand));
  RPT_TRY(w.sort.alloc((size_t)max_sort));
  RPT_TRY(w.vranges.alloc((size_t)max_ns));
  RPT_TRY(w.vrng_off.alloc((size_t)max_ns + 1));
  return RPT_OK;
}

static int32_t vote_slice_select(rpt_ctx* ctx, rpt_forest* f, VoteWork& w, const VoteSlice& sl, int v,
                                 bool want_counts) {
  ProfScope ps(ctx, RPT_PROF_KNN_VOTE);
  return vote_select(ctx, f->perm.p, reinterpret_cast<const VoteRange*>(w.pl.ranges.p), w.pl.rng_off.p,
                     w.pl.cand_off.p, f->T, sl, v, w.lds_cap, w.sort_off.p, w.sort.p, w.ids.p,
                     want_counts ? w.counts.p : nullptr, reinterpret_cast<VoteRange*>(w.vranges.p), w.vrng_off.p,
                     w.total.p);
}

static int32_t vote_read_total(rpt_ctx* ctx, VoteWork& w) {
  unsigned long long t = 0;
  RPT_HIP(hipMemcpyAsync(&t, w.total.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  RPT_HIP(stream_sync(ctx->stream));
  ctx->last_voted = (int64_t)t;
  return RPT_OK;
}

int32_t knn_vote_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q, int32_t k,
                     int32_t v, int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  RPT_ARG(k <= kBuf / 2, "k too large for the LDS merge buffer");
  RPT_ARG((size_t)data->d * 8 + (sizeof(Entry) + 4) * kBuf <= 150 * 1024, "d too large");
  ctx->last_uncertified = 0;
  ctx->metric_unc_pending = false;
  ctx->last_retries = 0;
  ctx->last_tier = 0;
  ctx->last_voted = 0;
  VoteWork w;
  RPT_TRY(vote_prepare(ctx, f, q, false, w));
  ctx->last_candidates = w.pl.total_cand;
  if (q->n == 0) return RPT_OK;
  const int metric = flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER);
  const int refm = (flags & RPT_KNN_METRIC_REFERENCE) ? 1 : 0;
  DevBuf<int32_t> unc;  // the queries the exact kernels answer again
  size_t max_ns = 1;
  for (const VoteSlice& sl : w.slices) max_ns = std::max(max_ns, (size_t)sl.ns);
  RPT_TRY(unc.alloc(max_ns));
  int64_t uncertified = 0;
  for (size_t si = 0; si < w.slices.size(); ++si) {
    const VoteSlice& sl = w.slices[si];
    RPT_TRY(vote_slice_select(ctx, f, w, sl, v, false));
    const rpt_dataset qv = query_view(q, sl.q0, sl.ns);
    RPT_TRY(launch_lists(ctx, data, &qv, w.ids.p, w.vranges.p, w.vrng_off.p, k, 0, metric, refm, unc.p,
                         ids_dev + sl.q0 * k, dist_dev + sl.q0 * k, count_dev + sl.q0));
    if (w.slices.size() > 1) RPT_TRY(add_uncertified(ctx, uncertified));
  }
  if (w.slices.size() > 1) {
    ctx->last_uncertified = uncertified;
    ctx->metric_unc_pending = false;
  }
  return vote_read_total(ctx, w);  // synchronises: the scratch is released on return
}

int32_t vote_candidates(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* q, int32_t v, int64_t* off_host,
                        int32_t* ids_host, int32_t* counts_host, int64_t cap, int64_t* total) {
  const bool fill = ids_host != nullptr;
  const bool want_counts = fill && counts_host != nullptr;
  ctx->last_voted = 0;
  VoteWork w;
  RPT_TRY(vote_prepare(ctx, f, q, want_counts, w));
  ctx->last_candidates = w.pl.total_cand;
  std::vector<Range> hr;
  std::vector<int32_t> hids, hcnt;
  int64_t at = 0;
  if (off_host) off_host[0] = 0;
  for (const VoteSlice& sl : w.slices) {
    RPT_TRY(vote_slice_select(ctx, f, w, sl, v, want_counts));
    hr.resize((size_t)sl.ns);
    RPT_HIP(hipMemcpyAsync(hr.data(), w.vranges.p, (size_t)sl.ns * sizeof(Range), hipMemcpyDeviceToHost, ctx->stream));
    if (fill && sl.cand_words > 0) {
      hids.resize((size_t)sl.cand_words);
      RPT_HIP(hipMemcpyAsync(hids.data(), w.ids.p, (size_t)sl.cand_words * 4, hipMemcpyDeviceToHost, ctx->stream));
      if (want_counts) {
        hcnt.resize((size_t)sl.cand_words);
        RPT_HIP(hipMemcpyAsync(hcnt.data(), w.counts.p, (size_t)sl.cand_words * 4, hipMemcpyDeviceToHost,
                               ctx->stream));
      }
    }
    RPT_HIP(stream_sync(ctx->stream));
    for (int64_t i = 0; i < sl.ns; ++i) {
      const Range& r = hr[(size_t)i];
      if (fill && r.n > 0) {
        RPT_ARG(at + r.n <= cap, "ids capacity too small");
        std::memcpy(ids_host + at, hids.data() + r.poff, (size_t)r.n * 4);
        if (want_counts) std::memcpy(counts_host + at, hcnt.data() + r.poff, (size_t)r.n * 4);
      }
      at += r.n;
      if (off_host) off_host[sl.q0 + i + 1] = at;
    }
  }
  *total = at;
  return vote_read_total(ctx, w);
}

// ---- an allow-list on the forest query and on the exhaustive kNN (rpt_knn_allow_*, rpt_brute_knn_allow_*) ----
// The forest query: make_plan, then knn_allow.hip's compaction turns every query's leaf ranges into
// ONE range of a scratch id slab (the candidate list without the disallowed entries, order and
// duplicates kept), then launch_lists ranks it with the call's duplicate rule: the rule sees the
// allowed list only.  A null bitmap takes the same route with every bit read as set.  Scratch: the
// vote route's fixed budget (kVoteBudgetWords), queries sliced against it or by knn_allow_slice.
// The exhaustive kNN: the bitmap as ONE ascending id list that every query ranks; position order is
// id order, so (distance, position) is (distance, id).
struct AllowWork {
  QueryPlan pl;
  std::vector<int64_t> starts;  // [nq + 1] cand_off[q * T] on the host
  std::vector<AllowSlice> slices;
  DevBuf<int32_t> ids, counts;
  DevBuf<Range> vranges;
  DevBuf<int64_t> vrng_off;
  DevBuf<unsigned long long> total;
  int64_t max_ns = 1;
};

static int32_t allow_prepare(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* q, AllowWork& w) {
  RPT_TRY(make_plan(ctx, f, q, w.pl));
  const int64_t nq = q->n;
  RPT_TRY(w.total.alloc(1));
  RPT_HIP(hipMemsetAsync(w.total.p, 0, 8, ctx->stream));
  if (nq == 0) return RPT_OK;
  const int64_t max_q = ctx->opt.knn_allow_slice > 0 ? ctx->opt.knn_allow_slice : 0x7fffffff;
  DevBuf<int64_t> starts_dev;
  RPT_TRY(starts_dev.alloc((size_t)nq + 1));
  RPT_TRY(vote_query_starts(ctx, w.pl.cand_off.p, f->T, nq, starts_dev.p));
  w.starts.resize((size_t)nq + 1);
  RPT_HIP(hipMemcpyAsync(w.starts.data(), starts_dev.p, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  RPT_HIP(stream_sync(ctx->stream));
  AllowSlice cur;
  int64_t max_cand = 1;
  auto close = [&]() {
    if (cur.ns == 0) return;
    w.slices.push_back(cur);
    max_cand = std::max(max_cand, cur.cand_words);
    w.max_ns = std::max(w.max_ns, cur.ns);
  };
  for (int64_t i = 0; i < nq; ++i) {
    const int64_t nc = w.starts[i + 1] - w.starts[i];
    RPT_ARG(nc <= 0x7fffffff, "a query has more candidates than an int32 holds");
    if (cur.ns > 0 && (cur.ns >= max_q || cur.cand_words + nc > kVoteBudgetWords)) {
      close();
      cur = AllowSlice();
    }
    if (cur.ns == 0) cur.q0 = i;
    cur.ns += 1;
    cur.cand_words += nc;
  }
  close();
  RPT_TRY(w.ids.alloc((size_t)max_cand));
  RPT_TRY(w.counts.alloc((size_t)w.max_ns));
  RPT_TRY(w.vranges.alloc((size_t)w.max_ns));
  RPT_TRY(w.vrng_off.alloc((size_t)w.max_ns + 1));
  return RPT_OK;
}

static int32_t allow_slice_compact(rpt_ctx* ctx, rpt_forest* f, AllowWork& w, const AllowSlice& sl,
                                   const AllowGroups& allow_dev) {
  ProfScope ps(ctx, RPT_PROF_KNN_VOTE);  // class 5: the candidate-list step
  return allow_compact(ctx, f->perm.p, reinterpret_cast<const VoteRange*>(w.pl.ranges.p), w.pl.rng_off.p,
                       w.pl.cand_off.p, f->T, sl, allow_dev, w.ids.p, reinterpret_cast<VoteRange*>(w.vranges.p),
                       w.vrng_off.p, w.counts.p, w.total.p);
}

static int32_t allow_read_total(rpt_ctx* ctx, AllowWork& w) {
  unsigned long long t = 0;
  RPT_HIP(hipMemcpyAsync(&t, w.total.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  RPT_HIP(stream_sync(ctx->stream));
  ctx->last_allowed = (int64_t)t;
  return RPT_OK;
}

int32_t knn_allow_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q,
                      const AllowGroups& allow_dev, int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev,
                      int32_t* count_dev) {
  RPT_ARG(k <= kBuf / 2, "k too large for the LDS merge buffer");
  RPT_ARG((size_t)data->d * 8 + (sizeof(Entry) + 4) * kBuf <= 150 * 1024, "d too large");
  ctx->last_uncertified = 0;
  ctx->metric_unc_pending = false;
  ctx->last_retries = 0;
  ctx->last_tier = 0;
  ctx->last_allowed = 0;
  AllowWork w;
  RPT_TRY(allow_prepare(ctx, f, q, w));
  ctx->last_candidates = w.pl.total_cand;
  if (q->n == 0) return RPT_OK;
  const int metric = flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER);
  const int refm = (flags & RPT_KNN_METRIC_REFERENCE) ? 1 : 0;
  DevBuf<int32_t> unc;  // the queries the exact kernels answer again
  RPT_TRY(unc.alloc((size_t)w.max_ns));
  int64_t uncertified = 0;
  for (const AllowSlice& sl : w.slices) {
    RPT_TRY(allow_slice_compact(ctx, f, w, sl, allow_dev));
    const rpt_dataset qv = query_view(q, sl.q0, sl.ns);
    RPT_TRY(launch_lists(ctx, data, &qv, w.ids.p, w.vranges.p, w.vrng_off.p, k, flags & 3, metric, refm, unc.p,
                         ids_dev + sl.q0 * k, dist_dev + sl.q0 * k, count_dev + sl.q0));
    if (w.slices.size() > 1) RPT_TRY(add_uncertified(ctx, uncertified));
  }
  if (w.slices.size() > 1) {
    ctx->last_uncertified = uncertified;
    ctx->metric_unc_pending = false;
  }
  return allow_read_total(ctx, w);  // synchronises: the scratch is released on return
}

int32_t allow_candidates(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* q, const AllowGroups& allow_dev,
                         int64_t* off_host, int32_t* ids_host, int64_t cap, int64_t* total) {
  const bool fill = ids_host != nullptr;
  ctx->last_allowed = 0;
  AllowWork w;
  RPT_TRY(allow_prepare(ctx, f, q, w));
  ctx->last_candidates = w.pl.total_cand;
  std::vector<Range> hr;
  std::vector<int32_t> hids;
  int64_t at = 0;
  if (off_host) off_host[0] = 0;
  for (const AllowSlice& sl : w.slices) {
    RPT_TRY(allow_slice_compact(ctx, f, w, sl, allow_dev));
    hr.resize((size_t)sl.ns);
    RPT_HIP(hipMemcpyAsync(hr.data(), w.vranges.p, (size_t)sl.ns * sizeof(Range), hipMemcpyDeviceToHost, ctx->stream));
    if (fill && sl.cand_words > 0) {
      hids.resize((size_t)sl.cand_words);
      RPT_HIP(hipMemcpyAsync(hids.data(), w.ids.p, (size_t)sl.cand_words * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    RPT_HIP(stream_sync(ctx->stream));
    for (int64_t i = 0; i < sl.ns; ++i) {
      const Range& r = hr[(size_t)i];
      if (fill && r.n > 0) {  // (a piece's first r.n words are the list; the rest was never written)
        RPT_ARG(at + r.n <= cap, "ids capacity too small");
        std::memcpy(ids_host + at, hids.data() + r.poff, (size_t)r.n * 4);
      }
      at += r.n;
      if (off_host) off_host[sl.q0 + i + 1] = at;
    }
  }
  *total = at;
  return allow_read_total(ctx, w);
}

int32_t knn_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q,
                int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  ctx->metric_unc_pending = false;
  RPT_ARG(data->dtype == q->dtype, "data and query dtype must match");
  RPT_ARG(k <= kBuf / 2, "k too large for the LDS merge buffer");
  RPT_ARG((size_t)data->d * 8 + (sizeof(Entry) + 4) * kBuf <= 150 * 1024, "d too large");
  RPT_ARG(proj_dtype(q->dtype) == f->pdtype,
          "query dtype must have the forest's projection type (f64 vs f32/bf16)");
  const int vote = (flags >> 8) & 0xffff;  // RPT_KNN_VOTE(v)
  if (flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER)) {
    if (data->csr)
      return fail(RPT_E_UNSUPPORTED, "RPT_KNN_METRIC_COSINE / _INNER: dense data only");
    if (vote > 0) return fail(RPT_E_UNSUPPORTED, "RPT_KNN_METRIC_COSINE / _INNER: no voting (RPT_KNN_VOTE)");
    return knn_metric(ctx, f, data, q, k, flags, ids_dev, dist_dev, count_dev);
  }
  // (the fused kernels walk the implicit batch topology: streamed forests take the general path;
  // so do SVector rows under the reference's own truncating metric)
  const bool refm = data->csr && (flags & RPT_KNN_METRIC_REFERENCE);
  ctx->last_uncertified = 0;
  // (knn_l2_exact: every query of dense f64 rows on the exact kernel, which the general path launches)
  const bool l2_exact = ctx->opt.knn_l2_exact && data->dtype == RPT_F64 && !data->csr && vote == 0;
  const bool fused = k <= kFK && f->T <= 1024 && ((!ctx->opt.knn_general && !l2_exact) || vote > 0) &&
                     (size_t)data->d * 8 <= 32 * 1024 && !f->xtopo && !refm;
  if (vote > 0 && (!fused || data->csr))
    return fail(RPT_E_UNSUPPORTED, "RPT_KNN_VOTE: dense data, k <= 64 and at most 1024 trees");
  if (!fused || q->n == 0) return knn_general(ctx, f, data, q, k, flags, ids_dev, dist_dev, count_dev);
  const int64_t nq = q->n;
  DevBuf<char> Pq;
  // one control block, one memset, one read-back: u64 candidates visited, u64 queries whose
  // prefilter cut was not certified, u32 queries that overflowed the range slab, pad, flags[nq]
  DevBuf<unsigned int> ctl;
  const size_t esz = f->pdtype == RPT_F64 ? 8 : 4;
  RPT_TRY(Pq.alloc((size_t)f->T * f->L * nq * esz + 16));
  RPT_TRY(ctl.alloc((size_t)nq + 6));
  RPT_HIP(hipMemsetAsync(ctl.p, 0, ((size_t)nq + 6) * 4, ctx->stream));
  unsigned int* ovf_p = ctl.p + 5;  // launch_fused: the count at ovf_p[0], the flags from ovf_p + 1
  unsigned long long* ctot_p = reinterpret_cast<unsigned long long*>(ctl.p);
  {
    ProfScope ps(ctx, RPT_PROF_KNN_PLAN);
    if (f->L > 0) RPT_TRY(project_columns(ctx, q, f->R.p, f->T * f->L, f->mode, Pq.p));
  }
  // the shadows the call ranks on, each built once per dataset (an ensure_* may leave its shadow absent)
  FusedIn in = fused_input(ctx, f, data, k, flags & 3, vote);
  for (unsigned tried = 0, want; (want = fused_shadows_wanted(in, tried)) != 0; tried |= want) {
    if (want & kShadow8) RPT_TRY(ensure_shadow8(ctx, data));
    if (want & kShadow32) RPT_TRY(ensure_shadow(ctx, data));
    if (want & kShadow16) RPT_TRY(ensure_shadow16(ctx, data));
    if (want & kShadowCsr32) RPT_TRY(ensure_shadow_csr(ctx, data));
    if (want & kShadowEll) RPT_TRY(ensure_shadow_ell(ctx, data));
    fused_input_shadows(in, data);
  }
  int tier = 0;
  auto launch = [&](bool rerun) -> int32_t {
    in.rerun = rerun;
    const FusedPlan p = fused_plan(in);
    if (!rerun) tier = p.tier;
    if (f->pdtype == RPT_F64)
      return launch_fused<double, double>(ctx, f, data, q, Pq.p, in, p, ids_dev, dist_dev, count_dev, ovf_p, ctot_p);
    if (data->dtype == RPT_F32)
      return launch_fused<float, float>(ctx, f, data, q, Pq.p, in, p, ids_dev, dist_dev, count_dev, ovf_p, ctot_p);
    return launch_fused<__hip_bfloat16, float>(ctx, f, data, q, Pq.p, in, p, ids_dev, dist_dev, count_dev, ovf_p,
                                               ctot_p);
  };
  RPT_TRY(launch(false));
  // (read back into the pinned arena: a pageable destination makes the copy a staged, blocking one)
  unsigned int hctl_stack[6] = {0, 0, 0, 0, 0, 0};
  unsigned int* hctl = reinterpret_cast<unsigned int*>(pin_alloc(ctx, 32));
  if (!hctl) hctl = hctl_stack;
  RPT_HIP(hipMemcpyAsync(hctl, ctl.p, 24, hipMemcpyDeviceToHost, ctx->stream));
  RPT_HIP(stream_sync(ctx->stream));
  const unsigned int novf = hctl[5];
  unsigned long long tot[2];
  std::memcpy(tot, hctl, 16);
  ctx->last_candidates = (int64_t)tot[0];
  ctx->last_uncertified = (int64_t)tot[1];
  ctx->last_retries = 0;
  if (novf && vote > 0)
    return fail(RPT_E_UNSUPPORTED,
                "RPT_KNN_VOTE: a query reaches more than 16384 candidates or 512 leaves");
  if (novf)  // some query reached more leaf ranges than the LDS slab holds: general path
    return knn_general(ctx, f, data, q, k, flags, ids_dev, dist_dev, count_dev);
  ctx->last_tier = tier;
  ctx->last_retries = (int64_t)hctl[4];
  fused_after_batch(f->tiers, tier, (uint64_t)nq, tot[1], hctl[4]);
  if (tot[1] && data->dtype == RPT_F64 && !data->csr) {
    // dense f64 rows whose cut no kernel could certify (different rows that tie at the cut, to the
    // last bits or exactly): the exact kernel over the query plan, them only — the definition
    QueryPlan pl;
    RPT_TRY(make_plan(ctx, f, q, pl));
    DevBuf<int32_t> unc;
    RPT_TRY(unc.alloc((size_t)nq));
    unsigned long long* uc = nullptr;
    RPT_TRY(metric_unc_count(ctx, &uc));
    RPT_HIP(hipMemsetAsync(uc, 0, 8, ctx->stream));
    hipLaunchKernelGGL(collect_flagged_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream,
                       ovf_p + 1, nq, unc.p, uc);
    RPT_HIP(hipGetLastError());
    RPT_TRY((launch_metric_v<double, kMetricL2, true>(ctx, data, q, f->perm.p, pl.ranges.p, pl.rng_off.p, f->T, 0,
                                                      k, flags & 3, unc.p, uc, ids_dev, dist_dev, count_dev)));
    RPT_HIP(stream_sync(ctx->stream));  // the plan, unc and ovf are released on return
  } else if (tot[1]) {  // f32 / CSR rows with equal distances at the prefilter's cut: the exact kernel, them only
    RPT_TRY(launch(true));
    RPT_HIP(stream_sync(ctx->stream));  // Pq / ovf are released on return
  }
  return RPT_OK;
}

// knnH (RPTree.hs:199-217): the union of the trees' candidatesH heaps is popped in increasing
// priority; buckets are taken while the running count stays <= k — but at least one —, each new
// bucket in FRONT of the ones taken before; the result is every point of those buckets with its
// distance, neither sorted nor cut to k.  Equal priorities keep (tree, DFS) order (the reference's
// order among ties depends on the shape of its heap).
// Device: query projections, traversal with priorities, distances.  Host: the per-query
// selection over a few dozen (priority, leaf) entries.
int32_t knn_h(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q,
              int32_t k, int64_t* off_host, int32_t* ids_host, double* dist_host, int64_t cap,
              int64_t* total) {
  RPT_ARG(data->dtype == q->dtype && data->csr == q->csr, "data and query must have one layout");
  const int64_t nq = q->n;
  const int T = f->T;
  *total = 0;
  if (off_host) off_host[0] = 0;
  if (nq == 0) return RPT_OK;
  QueryPlan pl;
  RPT_TRY(make_plan(ctx, f, q, pl));
  hipStream_t st = ctx->stream;
  DevBuf<double> prio;
  RPT_TRY(prio.alloc((size_t)pl.total_rng));
  const int threads = T <= 64 ? 64 : (T <= 128 ? 128 : 256);
  if (f->xtopo) {  // streamed forest: the same walk over the stored topology (ranges in traverse_x's order)
    if (f->pdtype == RPT_F64)
      hipLaunchKernelGGL(ranges_hx_kernel<double>, dim3((unsigned)nq), dim3(threads), 0, st, f->thr.p, f->mglo.p,
                         f->mghi.p, f->nodes, f->xkind.p, (const double*)pl.Pq.p, nq, T, f->L, pl.rng_off.p, prio.p);
    else
      hipLaunchKernelGGL(ranges_hx_kernel<float>, dim3((unsigned)nq), dim3(threads), 0, st, f->thr.p, f->mglo.p,
                         f->mghi.p, f->nodes, f->xkind.p, (const float*)pl.Pq.p, nq, T, f->L, pl.rng_off.p, prio.p);
  } else if (f->pdtype == RPT_F64)
    hipLaunchKernelGGL(ranges_h_kernel<double>, dim3((unsigned)nq), dim3(threads), 0, st, f->thr.p,
                       f->mglo.p, f->mghi.p, f->nodes, (const double*)pl.Pq.p, nq, T, f->L,
                       f->min_leaf, f->n, pl.rng_off.p, prio.p);
  else
    hipLaunchKernelGGL(ranges_h_kernel<float>, dim3((unsigned)nq), dim3(threads), 0, st, f->thr.p,
                       f->mglo.p, f->mghi.p, f->nodes, (const float*)pl.Pq.p, nq, T, f->L,
                       f->min_leaf, f->n, pl.rng_off.p, prio.p);
  RPT_HIP(hipGetLastError());
  RPT_HIP(stream_sync(st));
  std::vector<Range> hr((size_t)pl.total_rng);
  std::vector<double> hp((size_t)pl.total_rng);
  std::vector<int64_t> hoff((size_t)nq * T + 1);
  RPT_HIP(hipMemcpy(hr.data(), pl.ranges.p, hr.size() * sizeof(Range), hipMemcpyDeviceToHost));
  RPT_HIP(hipMemcpy(hp.data(), prio.p, hp.size() * 8, hipMemcpyDeviceToHost));
  RPT_HIP(hipMemcpy(hoff.data(), pl.rng_off.p, hoff.size() * 8, hipMemcpyDeviceToHost));
  std::vector<Range> sel;
  std::vector<int64_t> sel_off((size_t)nq + 1, 0), out_off((size_t)nq + 1, 0);
  std::vector<int64_t> order, taken;
  for (int64_t qi = 0; qi < nq; ++qi) {
    const int64_t r0 = hoff[(size_t)qi * T], r1 = hoff[(size_t)(qi + 1) * T];
    order.resize((size_t)(r1 - r0));
    for (int64_t r = r0; r < r1; ++r) order[(size_t)(r - r0)] = r;
    std::stable_sort(order.begin(), order.end(),
                     [&](int64_t a, int64_t b) { return hp[(size_t)a] < hp[(size_t)b]; });
    taken.clear();
    int64_t n = 0;
    for (int64_t r : order) {  // :209-217
      const int64_t ntot = hr[(size_t)r].n + n;
      // `not (null acc)` (:216) is about the POINTS taken so far: an empty bucket (streamed trees can
      // hold one) does not count as "at least one"
      if (ntot > k && n > 0) break;
      taken.push_back(r);
      n = ntot;
    }
    int64_t pos = 0;
    for (size_t i = taken.size(); i-- > 0;) {  // `xsh <> acc`: the bucket taken last comes first
      Range rg = hr[(size_t)taken[i]];
      rg.pos = (int32_t)pos;
      pos += rg.n;
      sel.push_back(rg);
    }
    sel_off[(size_t)qi + 1] = (int64_t)sel.size();
    out_off[(size_t)qi + 1] = out_off[(size_t)qi] + pos;
  }
  *total = out_off[(size_t)nq];
  if (off_host) std::memcpy(off_host, out_off.data(), out_off.size() * 8);
  if (!ids_host || !dist_host || *total == 0) return RPT_OK;
  RPT_ARG(cap >= *total, "result capacity too small");
  DevBuf<Range> dsel;
  DevBuf<int64_t> dsel_off, dout_off;
  DevBuf<int32_t> ids;
  DevBuf<double> dist;
  RPT_TRY(dsel.alloc(sel.size()));
  RPT_TRY(dsel_off.alloc(sel_off.size()));
  RPT_TRY(dout_off.alloc(out_off.size()));
  RPT_TRY(ids.alloc((size_t)*total));
  RPT_TRY(dist.alloc((size_t)*total));
  RPT_HIP(hipMemcpy(dsel.p, sel.data(), sel.size() * sizeof(Range), hipMemcpyHostToDevice));
  RPT_HIP(hipMemcpy(dsel_off.p, sel_off.data(), sel_off.size() * 8, hipMemcpyHostToDevice));
  RPT_HIP(hipMemcpy(dout_off.p, out_off.data(), out_off.size() * 8, hipMemcpyHostToDevice));
  if (data->csr) {
    const size_t smem = (size_t)data->d * 8;
    RPT_ARG(smem <= 150 * 1024, "d too large");
    if (data->dtype == RPT_F64) {
      RPT_HIP(launch_dyn(dist_sel_csr_kernel<double>, dim3((unsigned)nq), dim3(256), smem, st,
                         data->rowptr, data->col, (const double*)data->val, data->d, q->rowptr,
                         q->col, (const double*)q->val, f->perm.p, dsel.p, dsel_off.p, dout_off.p,
                         ids.p, dist.p));
    } else {
      RPT_HIP(launch_dyn(dist_sel_csr_kernel<float>, dim3((unsigned)nq), dim3(256), smem, st,
                         data->rowptr, data->col, (const float*)data->val, data->d, q->rowptr,
                         q->col, (const float*)q->val, f->perm.p, dsel.p, dsel_off.p, dout_off.p,
                         ids.p, dist.p));
    }
  } else {
    const size_t smem = (size_t)data->d * (data->dtype == RPT_F64 ? 8 : 4);
    RPT_ARG(smem <= 150 * 1024, "d too large");
#define RPT_DIST_SEL(TD)                                                                      \
  RPT_HIP(launch_dyn(dist_sel_dense_kernel<TD>, dim3((unsigned)nq), dim3(256), smem, st,      \
                     (const TD*)data->X, data->d, (const TD*)q->X, f->perm.p, dsel.p,         \
                     dsel_off.p, dout_off.p, ids.p, dist.p))
    if (data->dtype == RPT_F64) RPT_DIST_SEL(double);
    else if (data->dtype == RPT_F32) RPT_DIST_SEL(float);
    else RPT_DIST_SEL(__hip_bfloat16);
#undef RPT_DIST_SEL
  }
  RPT_HIP(stream_sync(st));
  RPT_HIP(hipMemcpy(ids_host, ids.p, (size_t)*total * 4, hipMemcpyDeviceToHost));
  RPT_HIP(hipMemcpy(dist_host, dist.p, (size_t)*total * 8, hipMemcpyDeviceToHost));
  return RPT_OK;
}

static int32_t launch_merge(rpt_ctx* ctx, const int32_t* ids, const double* dist,
                            const int32_t* cnt, int64_t is, int64_t ds, int64_t cs, int32_t G,
                            int64_t nq, int32_t k, int32_t flags, int32_t* out_ids,
                            double* out_dist, int32_t* out_count) {
  int np = 1;
  while (np < G * k) np <<= 1;
  const size_t smem = (sizeof(Entry) + 4) * (size_t)np;
  RPT_HIP(launch_dyn(merge_kernel, dim3((unsigned)nq), dim3(256), smem, ctx->stream, ids, dist,
                     cnt, is, ds, cs, G, nq, k, flags & 3, out_ids, out_dist, out_count));
  return RPT_OK;
}

int32_t knn_merge_dev(rpt_ctx* ctx, const int32_t* ids_dev, const double* dist_dev,
                      const int32_t* count_dev, int64_t shard_stride, int32_t G, int64_t nq,
                      int32_t k, int32_t flags, int32_t* out_ids, double* out_dist,
                      int32_t* out_count) {
  if (nq == 0) return RPT_OK;
  // shard_stride 0: three shard-major arrays [G][nq][k], [G][nq][k], [G][nq]
  const int64_t is = shard_stride ? shard_stride : nq * k * 4, ds = shard_stride ? shard_stride : nq * k * 8,
                cs = shard_stride ? shard_stride : nq * 4;
  // one launch holds all G * k entries of a query in LDS (20 bytes each: 4096 entries = 80 KB)
  if ((int64_t)G * k <= kMergeMax)
    return launch_merge(ctx, ids_dev, dist_dev, count_dev, is, ds, cs, G, nq, k, flags, out_ids,
                        out_dist, out_count);
  // larger merges (e.g. 8 shards x k = 1024) fold the shards in one at a time: the running
  // result (shards < g, already in the final order) against shard g is a 2-way merge of 2k
  // entries, and ties still prefer the earlier shard, so the order is that of the G-way merge.
  // The kernel addresses "shard 1" as base + stride, so the pair need not be adjacent.
  DevBuf<int32_t> ti[2], tc[2];
  DevBuf<double> td[2];
  for (int b = 0; b < 2 && G > 2; ++b) {
    RPT_TRY(ti[b].alloc((size_t)nq * k));
    RPT_TRY(td[b].alloc((size_t)nq * k));
    RPT_TRY(tc[b].alloc((size_t)nq));
  }
  const char *ai = (const char*)ids_dev, *ad = (const char*)dist_dev, *ac = (const char*)count_dev;
  for (int g = 1; g < G; ++g) {
    const bool last = g == G - 1;
    int32_t* oi = last ? out_ids : ti[g & 1].p;
    double* od = last ? out_dist : td[g & 1].p;
    int32_t* oc = last ? out_count : tc[g & 1].p;
    const char *gi = (const char*)ids_dev + g * is, *gd = (const char*)dist_dev + g * ds,
               *gc = (const char*)count_dev + g * cs;
    RPT_TRY(launch_merge(ctx, (const int32_t*)ai, (const double*)ad, (const int32_t*)ac, gi - ai,
                         gd - ad, gc - ac, 2, nq, k, flags, oi, od, oc));
    ai = (const char*)oi;
    ad = (const char*)od;
    ac = (const char*)oc;
  }
  return RPT_OK;
}

namespace {
// ---- brute force over CSR rows, query-tiled ---------------------------------
// One workgroup answers a TILE of QT queries against a block of consecutive rows: the queries
// are dense-ified into LDS interleaved (qs[j * QT + i] = coordinate j of query i, so the QT values
// a nonzero meets are one contiguous LDS read), the rows are streamed ONCE per tile — sixteen
// lanes per row, kBcU rows per group in flight, the coalesced 16-byte column / value loads of
// csr_rows_dist2 — and every nonzero is evaluated against all QT queries from registers.  A
// row's sum is added in csr_rows_dist2's order (four nonzeros per lane in index order, then the
// fixed butterfly of the group), so a distance does not depend on QT or on the row block.
// Selection: per query an LDS buffer of `cap` entries, the best k so far at its front.  An entry
// is appended only if it beats the k-th best so far (rows arrive in ascending id order, so an
// equal distance loses), and the buffer is sorted (merge_best, total order: NaN behind every
// number) when the next batch of rows might not fit.
// RPT_KNN_METRIC_REFERENCE: the truncating merge of metricSSL2 (topk_csr_kernel's refm branch),
// one thread per (row, query) pair.
// Grid: x = query tile, y = row block; block y writes its lists at out_*[y][nq][k].
constexpr int kBcThreads = 512;
constexpr int kBcU = 4;                              // rows per 16-lane group in flight
constexpr int kBcGroups = kBcThreads / 16;
constexpr int kBcRows = kBcGroups * kBcU;            // rows per batch
static_assert((kBcRows & (kBcRows - 1)) == 0 && kBcThreads % kBcRows == 0, "batch shape");

// ALLOW: only the rows whose bit of `allow` is set are offered (rpt_brute_knn_allow_*); a compile-time
// switch, off (0) in the unfiltered instantiation, whose code it leaves as it was.  1: one bitmap for
// every query.  2 (rpt_brute_knn_allow_group_*): tile query i's own bitmap, resolved once per tile into
// LDS (allow_row: a row of ag.bits, every id, or none).
template <class TD, int QT, int ALLOW = 0>
__global__ __launch_bounds__(kBcThreads) void brute_csr_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const TD* __restrict__ val, int64_t nnz, int64_t n, int d,
    const int64_t* __restrict__ qrowptr, const int32_t* __restrict__ qcol,
    const TD* __restrict__ qval, int64_t nq, int k, int cap, int64_t rows_per_block, int refm,
    int32_t* __restrict__ out_ids, double* __restrict__ out_dist, int32_t* __restrict__ out_cnt,
    AllowGroups ag /* ALLOW only: ceil(n / 32) words per bitmap */) {
  const uint32_t* __restrict__ allow = ag.bits;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* qs = reinterpret_cast<double*>(smem);                                   // [d][QT]
  Entry* bufs = reinterpret_cast<Entry*>(smem + (size_t)d * QT * sizeof(double));  // [QT][cap]
  __shared__ double s_qn2[QT], s_thr[QT];
  __shared__ int s_fill[QT], s_have[QT];
  __shared__ const uint32_t* s_abits[ALLOW == 2 ? QT : 1];  // ALLOW == 2: query i's bitmap (null: every id)
  __shared__ int s_anone[ALLOW == 2 ? QT : 1];              // ... 1: no id is allowed
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * QT;
  const int nqt = nq - q0 < QT ? (int)(nq - q0) : QT;
  if constexpr (ALLOW == 2) {
    if (tid < QT) {  // (read behind the first barrier below)
      bool none = true;
      s_abits[tid] = tid < nqt ? allow_row(ag, q0 + tid, none) : nullptr;
      s_anone[tid] = none ? 1 : 0;
    }
  }
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int j = tid; j < d * QT; j += kBcThreads) qs[j] = 0.0;
  if (tid < QT) {
    s_fill[tid] = 0;
    s_have[tid] = 0;
    s_thr[tid] = 0.0;
    s_qn2[tid] = 0.0;
  }
  __syncthreads();
  if (!refm) {
    for (int i = 0; i < nqt; ++i)
      for (int64_t j = qrowptr[q0 + i] + tid; j < qrowptr[q0 + i + 1]; j += kBcThreads)
        qs[(int64_t)qcol[j] * QT + i] = (double)qval[j];
    __syncthreads();
    // |q|^2 over the query's nonzero list in the order a ROW's sum is added (four nonzeros per
    // lane of a 16-lane group, then the butterfly): against a row that equals the query every term
    // is -(q_j^2) exactly, the row's sum is -|q|^2 to the bit, and a stored row's distance to
    // itself (and to its copies) is exactly 0 instead of the rounding noise of two summation orders
    for (int i = wave; i < nqt; i += kBcThreads / 64) {
      const int64_t a = qrowptr[q0 + i], b = qrowptr[q0 + i + 1];
      double s = 0.0;
      for (int64_t j = a + 4 * (lane & 15); j < b; j += 64)
        for (int e = 0; e < 4; ++e)
          if (j + e < b) {
            const double v = (double)qval[j + e];
            s += v * v;
          }
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) s_qn2[i] = s;
    }
    __syncthreads();
  }
  auto push = [&](int i, double dist, int row) {
    if constexpr (ALLOW == 1) {
      if (!((allow[row >> 5] >> (row & 31)) & 1u)) return;
    }
    if constexpr (ALLOW == 2) {
      const uint32_t* ab = s_abits[i];
      if (s_anone[i] || (ab && !((ab[row >> 5] >> (row & 31)) & 1u))) return;
    }
    if (!s_have[i] || (dist == dist && !(dist >= s_thr[i])))
      bufs[i * cap + atomicAdd(&s_fill[i], 1)] = Entry{dist, row, row};
  };
  // sorts query i's buffer, keeps the best k in front; every thread calls
  auto settle = [&](int i) {
    Entry* buf = bufs + i * cap;
    const int best = merge_best<true>(buf, s_fill[i], k, 0, nullptr);
    __syncthreads();
    if (tid == 0) {
      s_fill[i] = best;
      if (best == k) {
        s_have[i] = 1;
        s_thr[i] = buf[k - 1].dist;
      }
    }
    __syncthreads();
    return best;
  };
  for (int64_t b0 = r0; b0 < r1; b0 += kBcRows) {
    if (refm) {
      const int64_t row = b0 + (tid & (kBcRows - 1));
      if (row < r1) {
        const int64_t a1 = rowptr[row], b1 = rowptr[row + 1];
        for (int i = tid / kBcRows; i < nqt; i += kBcThreads / kBcRows) {
          int64_t i1 = a1, i2 = qrowptr[q0 + i];
          const int64_t b2 = qrowptr[q0 + i + 1];
          double acc = 0.0;
          while (i1 < b1 && i2 < b2) {
            const int il = col[i1], ir = qcol[i2];
            double df;
            if (il == ir) {
              df = (double)val[i1] - (double)qval[i2];
              ++i1;
              ++i2;
            } else if (il < ir) {
              df = (double)val[i1] - 0.0;
              ++i1;
            } else {
              df = 0.0 - (double)qval[i2];
              ++i2;
            }
            acc = acc + df * df;
          }
          push(i, sqrt(acc), (int)row);
        }
      }
    } else {
      struct __attribute__((packed, aligned(4))) C4 { int v[4]; };
      struct __attribute__((packed, aligned(4))) V4 { TD v[4]; };
      const int grp = tid >> 4, l16 = tid & 15;
      int64_t ra[kBcU], rb[kBcU];
      double s[kBcU][QT];
#pragma unroll
      for (int u = 0; u < kBcU; ++u) {
        const int64_t row = b0 + u * kBcGroups + grp;
        const bool ok = row < r1;
        ra[u] = rowptr[ok ? row : r0];
        rb[u] = ok ? rowptr[row + 1] : ra[u];
#pragma unroll
        for (int i = 0; i < QT; ++i) s[u][i] = 0.0;
      }
      for (int64_t t = 4 * l16;; t += 64) {
        C4 c[kBcU];
        V4 v[kBcU];
        bool more = false;
#pragma unroll
        for (int u = 0; u < kBcU; ++u) {
          const int64_t j = ra[u] + t;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            c[u].v[e] = 0;
            v[u].v[e] = (TD)0;
          }
          if (j < rb[u]) {
            if (j + 4 <= nnz) {  // may run past the row's end (masked below), never past the arrays'
              c[u] = *reinterpret_cast<const C4*>(col + j);
              v[u] = *reinterpret_cast<const V4*>(val + j);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (j + e < rb[u]) {
                  c[u].v[e] = col[j + e];
                  v[u].v[e] = val[j + e];
                }
            }
          }
          more = more || j + 64 < rb[u];
        }
#pragma unroll
        for (int u = 0; u < kBcU; ++u) {
          const int64_t j = ra[u] + t;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = j + e < rb[u];
            const double* qp = qs + (int64_t)(ok ? c[u].v[e] : 0) * QT;
            const double x = (double)v[u].v[e];
#pragma unroll
            for (int i = 0; i < QT; ++i) {
              const double qj = qp[i];
              const double df = x - qj;
              const double term = df * df - qj * qj;
              s[u][i] += ok ? term : 0.0;
            }
          }
        }
        if (!__any(more)) break;
      }
#pragma unroll
      for (int u = 0; u < kBcU; ++u) {
        const int64_t row = b0 + u * kBcGroups + grp;
#pragma unroll
        for (int i = 0; i < QT; ++i) {
          double a = s[u][i];
          for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o);  // csr_rows_dist2's butterfly
          if (l16 == 0 && row < r1 && i < nqt) {
            const double t = a + s_qn2[i];
            push(i, sqrt(t > 0 ? t : 0.0), (int)row);
          }
        }
      }
    }
    __syncthreads();
    // a batch appends at most kBcRows entries to a buffer: sort the ones the next might overflow
    unsigned need = 0;
    for (int i = 0; i < nqt; ++i) need |= (s_fill[i] > cap - kBcRows ? 1u : 0u) << i;
    __syncthreads();
    for (int i = 0; i < nqt; ++i)
      if (need >> i & 1) settle(i);
  }
  for (int i = 0; i < nqt; ++i) {
    const int best = settle(i);
    const Entry* buf = bufs + i * cap;
    const int64_t o = (int64_t)blockIdx.y * nq + q0 + i;
    for (int r = tid; r < k; r += kBcThreads) {
      const bool ok = r < best;
      out_ids[o * k + r] = ok ? buf[r].id : -1;
      out_dist[o * k + r] = ok ? buf[r].dist : __longlong_as_double(0x7ff0000000000000LL);
    }
    if (tid == 0) out_cnt[o] = best;
    __syncthreads();
  }
}

static inline int brute_csr_cap(int k) {
  int cap = 256;
  while (cap < k + kBcRows) cap <<= 1;
  return cap;
}
static inline size_t brute_csr_smem(int d, int qt, int k) {
  return (size_t)d * qt * sizeof(double) + (size_t)qt * brute_csr_cap(k) * sizeof(Entry);
}
constexpr size_t kBcLds = 150 * 1024;  // the budget the other query kernels keep (of 160 KB)

template <class TD, int QT>
static int32_t launch_brute_csr_t(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int k,
                                  int refm, int64_t rows_per_block, int nblk, int32_t* ids,
                                  double* dist, int32_t* cnt, const AllowGroups& allow) {
  const size_t smem = brute_csr_smem(data->d, QT, k);
  const int64_t tiles = (q->n + QT - 1) / QT;
  RPT_HIP(launch_dyn(allow.group  ? brute_csr_kernel<TD, QT, 2>
                     : allow.bits ? brute_csr_kernel<TD, QT, 1>
                                  : brute_csr_kernel<TD, QT, 0>,
                     dim3((unsigned)tiles, (unsigned)nblk),
                     dim3(kBcThreads), smem, ctx->stream, data->rowptr, data->col,
                     (const TD*)data->val, data->nnz, data->n, data->d, q->rowptr, q->col,
                     (const TD*)q->val, q->n, k, brute_csr_cap(k), rows_per_block, refm, ids, dist,
                     cnt, allow));
  return RPT_OK;
}

template <class TD>
static int32_t launch_brute_csr(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int k,
                                int refm, int qt, int64_t rows_per_block, int nblk, int32_t* ids,
                                double* dist, int32_t* cnt, const AllowGroups& allow) {
  switch (qt) {
    case 8: return launch_brute_csr_t<TD, 8>(ctx, data, q, k, refm, rows_per_block, nblk, ids, dist, cnt, allow);
    case 4: return launch_brute_csr_t<TD, 4>(ctx, data, q, k, refm, rows_per_block, nblk, ids, dist, cnt, allow);
    case 2: return launch_brute_csr_t<TD, 2>(ctx, data, q, k, refm, rows_per_block, nblk, ids, dist, cnt, allow);
    default: return launch_brute_csr_t<TD, 1>(ctx, data, q, k, refm, rows_per_block, nblk, ids, dist, cnt, allow);
  }
}

// queries per workgroup: the option brute_csr_tile (rounded down to 1, 2, 4 or 8), else the
// largest tile up to 4 the batch can use (measured at C3, 1 000 queries: 240 / 154 / 120 / 127 ms
// for QT = 1 / 2 / 4 / 8 — from QT = 4 on the kernel is bound by its arithmetic and LDS reads, not
// by the bytes it streams); halved until the tile's LDS fits (QT = 1 fits whenever the
// `d too large` rule of the query kernels holds)
static int brute_csr_tile(const rpt_ctx* ctx, int d, int k, int64_t nq) {
  int qt = 8;
  if (ctx->opt.brute_csr_tile > 0) {
    while (qt > ctx->opt.brute_csr_tile) qt >>= 1;
  } else {
    qt = 4;
    while (qt > 1 && qt / 2 >= nq) qt >>= 1;
  }
  while (qt > 1 && brute_csr_smem(d, qt, k) > kBcLds) qt >>= 1;
  return qt;
}

// exhaustive kNN of CSR queries over CSR rows 0 .. n-1, k best by (distance, id), into device
// arrays [nq][k]; cnt: [nq] ints of device scratch.  allow: empty, the one bitmap of the rows offered
// (allow.bits), or with allow.group every query's own.
// Enqueues only.
static int32_t brute_csr(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int k, int refm,
                         int32_t* ids_dev, double* dist_dev, int32_t* cnt_dev,
                         const AllowGroups& allow = AllowGroups()) {
  RPT_ARG((size_t)data->d * 8 + (sizeof(Entry) + 4) * kBuf <= 150 * 1024, "d too large");
  RPT_ARG(data->n <= 0x7fffffff, "too many rows");
  const int64_t nq = q->n, n = data->n;
  const int qt = brute_csr_tile(ctx, data->d, k, nq);
  // few query tiles: split the rows over enough workgroups for two per CU, each with at least
  // 4096 rows, at most as many as one merge launch takes; the row blocks are "shards" in ascending
  // id order for merge_kernel, whose (distance, shard, rank) order is then (distance, id)
  const int64_t tiles = (nq + qt - 1) / qt;
  int64_t nblk = (2 * (int64_t)ctx->n_cu + tiles - 1) / tiles;
  nblk = std::min(nblk, std::min<int64_t>(kMergeMax / k, n / 4096));
  nblk = std::max<int64_t>(nblk, 1);
  int64_t rows = (n + nblk - 1) / nblk;
  rows = std::max<int64_t>((rows + kBcRows - 1) / kBcRows * kBcRows, kBcRows);
  nblk = std::max<int64_t>((n + rows - 1) / rows, 1);
  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  if (nblk == 1) {
    if (data->dtype == RPT_F64)
      return launch_brute_csr<double>(ctx, data, q, k, refm, qt, rows, 1, ids_dev, dist_dev, cnt_dev, allow);
    return launch_brute_csr<float>(ctx, data, q, k, refm, qt, rows, 1, ids_dev, dist_dev, cnt_dev, allow);
  }
  DevBuf<int32_t> pi, pc;
  DevBuf<double> pd;
  RPT_TRY(pi.alloc((size_t)nblk * nq * k));
  RPT_TRY(pd.alloc((size_t)nblk * nq * k));
  RPT_TRY(pc.alloc((size_t)nblk * nq));
  if (data->dtype == RPT_F64)
    RPT_TRY(launch_brute_csr<double>(ctx, data, q, k, refm, qt, rows, (int)nblk, pi.p, pd.p, pc.p, allow));
  else
    RPT_TRY(launch_brute_csr<float>(ctx, data, q, k, refm, qt, rows, (int)nblk, pi.p, pd.p, pc.p, allow));
  // (the partial lists are released on return: the allocator hands a block out again only after
  // the stream it was freed on has been synchronised)
  return knn_merge_dev(ctx, pi.p, pd.p, pc.p, 0, (int32_t)nblk, nq, k, 0, ids_dev, dist_dev, cnt_dev);
}

// ---- brute force over CSR rows under the cosine / inner-product metrics, query-tiled ------------
// brute_csr_kernel's stream with the per-nonzero term x * q_j: a tile of QT queries (dense-ified
// interleaved, plus one byte per column whose bit i says query i stores it) against a block of rows
// read once.  Each (query, row block) keeps the best kk = k + kLfMargin rows by the lane-parallel
// value (rows arrive in ascending id order and are distinct: merge_best is merge_distinct here),
// evaluates those again as the fold dotS (leftfold_dot_csr's walk, one thread per kept row, the
// presence test on), writes its k best by (fold value, id) — finalize_leftfold's order — and
// certifies its own cut as knn_metric_csr_kernel does; a query with an uncertified block is flagged
// 2 and answered again, whole, by knn_metric_csr_kernel<.., EXACT = true> in identity mode.
// LDS: qs [d][QT] doubles, bufs [QT][cap] entries (cap >= kk + kBcRows), the finalize arrays
// (kk x 20 bytes, one query at a time), pres [d] bytes.
static inline size_t brute_csr_metric_smem(int d, int qt, int kk) {
  return (size_t)d * qt * sizeof(double) + (size_t)qt * brute_csr_cap(kk) * sizeof(Entry) +
         (((size_t)kk * 20 + 15) & ~(size_t)15) + (((size_t)d + 15) & ~(size_t)15);
}

template <class TD, int QT, int METRIC>
__global__ __launch_bounds__(kBcThreads) void brute_csr_metric_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const TD* __restrict__ val, int64_t nnz,
    int64_t n, int d, const int64_t* __restrict__ qrowptr, const int32_t* __restrict__ qcol,
    const TD* __restrict__ qval, int64_t nq, int k, int kk, int cap, int64_t rows_per_block,
    const double* __restrict__ rn, const unsigned long long* __restrict__ stats, unsigned int* __restrict__ flags,
    int32_t* __restrict__ out_ids, double* __restrict__ out_dist, int32_t* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* qs = reinterpret_cast<double*>(smem);                                   // [d][QT]
  Entry* bufs = reinterpret_cast<Entry*>(smem + (size_t)d * QT * sizeof(double));  // [QT][cap]
  double* lf = reinterpret_cast<double*>(bufs + (size_t)QT * cap);                // [kk]
  int* order = reinterpret_cast<int*>(lf + kk);                                   // [kk]
  int* ids2 = order + kk;                                                         // [kk]
  int* pos2 = ids2 + kk;                                                          // [kk]
  unsigned char* pres = smem + (size_t)d * QT * sizeof(double) + (size_t)QT * cap * sizeof(Entry) +
                        (((size_t)kk * 20 + 15) & ~(size_t)15);                   // [d]
  __shared__ double s_qq[QT], s_last;
  __shared__ Entry s_thr[QT];
  __shared__ int s_fill[QT], s_have[QT], s_cut[QT], s_w;
  const int tid = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * QT;
  const int nqt = nq - q0 < QT ? (int)(nq - q0) : QT;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int j = tid; j < d * QT; j += kBcThreads) qs[j] = 0.0;
  for (int j = tid; j < d; j += kBcThreads) pres[j] = 0;
  if (tid < QT) {
    s_fill[tid] = 0;
    s_have[tid] = 0;
    s_cut[tid] = 0;
    s_qq[tid] = 0.0;
  }
  __syncthreads();
  // (a column's byte is shared by the tile's queries: one query at a time, a barrier between them)
  for (int i = 0; i < nqt; ++i) {
    for (int64_t j = qrowptr[q0 + i] + tid; j < qrowptr[q0 + i + 1]; j += kBcThreads) {
      qs[(int64_t)qcol[j] * QT + i] = (double)qval[j];
      pres[qcol[j]] |= (unsigned char)(1u << i);
    }
    __syncthreads();
  }
  if (tid < nqt) {  // dotS(q, q)
    double acc = 0.0;
    for (int64_t j = qrowptr[q0 + tid]; j < qrowptr[q0 + tid + 1]; ++j) {
      const double v = (double)qval[j];
      acc = acc + v * v;
    }
    s_qq[tid] = acc;
  }
  __syncthreads();
  // rows arrive in ascending id order: an entry enters only if it beats the kk-th best so far in
  // the total order (an equal value, or a NaN behind a NaN, loses to the smaller id)
  auto push = [&](int i, double dist, int row) {
    const Entry e{dist, row, row};
    if (!s_have[i] || entry_less_total(e, s_thr[i])) bufs[i * cap + atomicAdd(&s_fill[i], 1)] = e;
    else s_cut[i] = 1;
  };
  // sorts query i's buffer, keeps the best kk in front; every thread calls
  auto settle = [&](int i) {
    Entry* buf = bufs + i * cap;
    const int filled = s_fill[i];
    const int best = merge_best<true>(buf, filled, kk, 0, nullptr);
    __syncthreads();
    if (tid == 0) {
      s_fill[i] = best;
      if (filled > best) s_cut[i] = 1;
      if (best == kk) {
        s_have[i] = 1;
        s_thr[i] = buf[kk - 1];
      }
    }
    __syncthreads();
    return best;
  };
  for (int64_t b0 = r0; b0 < r1; b0 += kBcRows) {
    struct __attribute__((packed, aligned(4))) C4 { int v[4]; };
    struct __attribute__((packed, aligned(4))) V4 { TD v[4]; };
    const int grp = tid >> 4, l16 = tid & 15;
    int64_t ra[kBcU], rb[kBcU];
    double s[kBcU][QT];
#pragma unroll
    for (int u = 0; u < kBcU; ++u) {
      const int64_t row = b0 + u * kBcGroups + grp;
      const bool ok = row < r1;
      ra[u] = rowptr[ok ? row : r0];
      rb[u] = ok ? rowptr[row + 1] : ra[u];
#pragma unroll
      for (int i = 0; i < QT; ++i) s[u][i] = 0.0;
    }
    for (int64_t t = 4 * l16;; t += 64) {
      C4 c[kBcU];
      V4 v[kBcU];
      bool more = false;
#pragma unroll
      for (int u = 0; u < kBcU; ++u) {
        const int64_t j = ra[u] + t;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c[u].v[e] = 0;
          v[u].v[e] = (TD)0;
        }
        if (j < rb[u]) {
          if (j + 4 <= nnz) {  // may run past the row's end (masked below), never past the arrays'
            c[u] = *reinterpret_cast<const C4*>(col + j);
            v[u] = *reinterpret_cast<const V4*>(val + j);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (j + e < rb[u]) {
                c[u].v[e] = col[j + e];
                v[u].v[e] = val[j + e];
              }
          }
        }
        more = more || j + 64 < rb[u];
      }
#pragma unroll
      for (int u = 0; u < kBcU; ++u) {
        const int64_t j = ra[u] + t;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool ok = j + e < rb[u];
          const double* qp = qs + (int64_t)(ok ? c[u].v[e] : 0) * QT;
          const double x = (double)v[u].v[e];
#pragma unroll
          for (int i = 0; i < QT; ++i) {
            const double term = x * qp[i];
            s[u][i] += ok ? term : 0.0;
          }
        }
      }
      if (!__any(more)) break;
    }
#pragma unroll
    for (int u = 0; u < kBcU; ++u) {
      const int64_t row = b0 + u * kBcGroups + grp;
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        double a = s[u][i];
        for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o);  // csr_rows_dist2's butterfly
        if (l16 == 0 && row < r1 && i < nqt)
          push(i, metric_value<METRIC>(a, METRIC == kMetricCosine ? rn[row] : 0.0, s_qq[i]), (int)row);
      }
    }
    __syncthreads();
    // a batch appends at most kBcRows entries to a buffer: sort the ones the next might overflow
    unsigned need = 0;
    for (int i = 0; i < nqt; ++i) need |= (s_fill[i] > cap - kBcRows ? 1u : 0u) << i;
    __syncthreads();
    for (int i = 0; i < nqt; ++i)
      if (need >> i & 1) settle(i);
  }
  for (int i = 0; i < nqt; ++i) {
    const int best = settle(i);
    const Entry* buf = bufs + i * cap;
    const int64_t o = (int64_t)blockIdx.y * nq + q0 + i;
    const double qq = METRIC == kMetricCosine ? s_qq[i] : 0.0;
    for (int r = tid; r < best; r += kBcThreads) {  // the kept rows again as the fold
      const int id = buf[r].id;
      ids2[r] = id;
      pos2[r] = id;
      double acc = 0.0;
      for (int64_t j = rowptr[id]; j < rowptr[id + 1]; ++j) {
        const int c = col[j];
        if ((pres[c] >> i) & 1) acc = acc + (double)val[j] * qs[(int64_t)c * QT + i];
      }
      lf[r] = metric_value<METRIC>(acc, METRIC == kMetricCosine ? rn[id] : 0.0, qq);
    }
    __syncthreads();
    finalize_select(best, k, 0, lf, order, ids2, pos2, tid, kBcThreads, [] { __syncthreads(); }, o, out_ids,
                    out_dist, out_cnt, &s_w, &s_last);
    if (tid == 0) {  // (the thread that wrote the answer and s_w / s_last)
      bool ok = !s_cut[i];
      if (!ok && s_w == k && best > 0)
        ok = s_last < buf[best - 1].dist - metric_cut_slack<METRIC>(d, s_qq[i], stats);
      if (!ok) flags[q0 + i] = 2u;
    }
    __syncthreads();
  }
}

template <class TD, int QT, int METRIC>
static int32_t launch_brute_csr_metric_t(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int k,
                                         int64_t rows_per_block, int nblk, unsigned int* flags, int32_t* ids,
                                         double* dist, int32_t* cnt) {
  const int kk = k + kLfMargin;
  const int64_t tiles = (q->n + QT - 1) / QT;
  RPT_HIP(launch_dyn(brute_csr_metric_kernel<TD, QT, METRIC>, dim3((unsigned)tiles, (unsigned)nblk),
                     dim3(kBcThreads), brute_csr_metric_smem(data->d, QT, kk), ctx->stream, data->rowptr, data->col,
                     (const TD*)data->val, data->nnz, data->n, data->d, q->rowptr, q->col, (const TD*)q->val, q->n,
                     k, kk, brute_csr_cap(kk), rows_per_block, (const double*)data->sqnorm,
                     reinterpret_cast<const unsigned long long*>(data->sqnorm + data->n), flags, ids, dist, cnt));
  return RPT_OK;
}

template <class TD, int METRIC>
static int32_t launch_brute_csr_metric(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int k, int qt,
                                       int64_t rows, int nblk, unsigned int* flags, int32_t* ids, double* dist,
                                       int32_t* cnt) {
  switch (qt) {
    case 8: return launch_brute_csr_metric_t<TD, 8, METRIC>(ctx, data, q, k, rows, nblk, flags, ids, dist, cnt);
    case 4: return launch_brute_csr_metric_t<TD, 4, METRIC>(ctx, data, q, k, rows, nblk, flags, ids, dist, cnt);
    case 2: return launch_brute_csr_metric_t<TD, 2, METRIC>(ctx, data, q, k, rows, nblk, flags, ids, dist, cnt);
    default: return launch_brute_csr_metric_t<TD, 1, METRIC>(ctx, data, q, k, rows, nblk, flags, ids, dist, cnt);
  }
}

// exhaustive kNN of CSR queries over CSR rows under RPT_KNN_METRIC_COSINE / _INNER into device arrays
// [nq][k]: the tiled stream (brute_csr's tile and row blocks, merged by knn_merge_dev), then the
// exact kernel over the flagged queries — or alone over all of them with knn_metric_exact.
// cnt: [nq] ints of device scratch.  Enqueues only; ctx->last_uncertified follows lazily.
static int32_t brute_csr_metric(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int k, int metric,
                                int32_t* ids_dev, double* dist_dev, int32_t* cnt_dev) {
  RPT_ARG(data->n <= 0x7fffffff, "too many rows");
  RPT_TRY(ensure_sqnorm(ctx, data));
  const int64_t nq = q->n, n = data->n;
  const bool cosine = metric == RPT_KNN_METRIC_COSINE;
  unsigned long long* uc = nullptr;
  RPT_TRY(metric_unc_count(ctx, &uc));
  DevBuf<int32_t> unc;
  RPT_TRY(unc.alloc((size_t)nq));
  auto exact = [&](int32_t* list) -> int32_t {
    if (data->dtype == RPT_F64)
      return cosine ? launch_metric_csr_v<double, kMetricCosine, true>(ctx, data, q, nullptr, nullptr, nullptr, 1, 1,
                                                                       k, 0, list, uc, ids_dev, dist_dev, cnt_dev)
                    : launch_metric_csr_v<double, kMetricInner, true>(ctx, data, q, nullptr, nullptr, nullptr, 1, 1,
                                                                      k, 0, list, uc, ids_dev, dist_dev, cnt_dev);
    return cosine ? launch_metric_csr_v<float, kMetricCosine, true>(ctx, data, q, nullptr, nullptr, nullptr, 1, 1, k,
                                                                    0, list, uc, ids_dev, dist_dev, cnt_dev)
                  : launch_metric_csr_v<float, kMetricInner, true>(ctx, data, q, nullptr, nullptr, nullptr, 1, 1, k,
                                                                   0, list, uc, ids_dev, dist_dev, cnt_dev);
  };
  if (ctx->opt.knn_metric_exact) {
    ctx->last_uncertified = nq;
    ctx->metric_unc_pending = false;
    return exact(nullptr);
  }
  const int kk = k + kLfMargin;
  int qt = brute_csr_tile(ctx, data->d, kk, nq);
  while (qt > 1 && brute_csr_metric_smem(data->d, qt, kk) > kBcLds) qt >>= 1;
  // (a d near the `d too large` limit with k near 1024: one query does not fit next to the finalize
  // arrays — the forest kernel pair in identity mode, one workgroup per query, has the same answer)
  if (brute_csr_metric_smem(data->d, qt, kk) > kBcLds)
    return launch_metric_csr(ctx, data, q, nullptr, nullptr, nullptr, 1, 1, k, 0, metric, unc.p, ids_dev, dist_dev,
                             cnt_dev);
  // the row blocks of brute_csr
  const int64_t tiles = (nq + qt - 1) / qt;
  int64_t nblk = (2 * (int64_t)ctx->n_cu + tiles - 1) / tiles;
  nblk = std::min(nblk, std::min<int64_t>(kMergeMax / k, n / 4096));
  nblk = std::max<int64_t>(nblk, 1);
  int64_t rows = (n + nblk - 1) / nblk;
  rows = std::max<int64_t>((rows + kBcRows - 1) / kBcRows * kBcRows, kBcRows);
  nblk = std::max<int64_t>((n + rows - 1) / rows, 1);
  DevBuf<unsigned int> flags;
  RPT_TRY(flags.alloc((size_t)nq));
  RPT_HIP(hipMemsetAsync(flags.p, 0, (size_t)nq * 4, ctx->stream));
  RPT_HIP(hipMemsetAsync(uc, 0, 8, ctx->stream));
  DevBuf<int32_t> pi, pc;
  DevBuf<double> pd;
  int32_t* oi = ids_dev;
  double* od = dist_dev;
  int32_t* oc = cnt_dev;
  if (nblk > 1) {
    RPT_TRY(pi.alloc((size_t)nblk * nq * k));
    RPT_TRY(pd.alloc((size_t)nblk * nq * k));
    RPT_TRY(pc.alloc((size_t)nblk * nq));
    oi = pi.p;
    od = pd.p;
    oc = pc.p;
  }
  {
    ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
    if (data->dtype == RPT_F64)
      RPT_TRY(cosine ? (launch_brute_csr_metric<double, kMetricCosine>(ctx, data, q, k, qt, rows, (int)nblk, flags.p,
                                                                       oi, od, oc))
                     : (launch_brute_csr_metric<double, kMetricInner>(ctx, data, q, k, qt, rows, (int)nblk, flags.p,
                                                                      oi, od, oc)));
    else
      RPT_TRY(cosine ? (launch_brute_csr_metric<float, kMetricCosine>(ctx, data, q, k, qt, rows, (int)nblk, flags.p,
                                                                      oi, od, oc))
                     : (launch_brute_csr_metric<float, kMetricInner>(ctx, data, q, k, qt, rows, (int)nblk, flags.p, oi,
                                                                     od, oc)));
  }
  if (nblk > 1)
    RPT_TRY(knn_merge_dev(ctx, pi.p, pd.p, pc.p, 0, (int32_t)nblk, nq, k, 0, ids_dev, dist_dev, cnt_dev));
  hipLaunchKernelGGL(collect_flagged_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, flags.p,
                     nq, unc.p, uc);
  RPT_HIP(hipGetLastError());
  ctx->metric_unc_pending = true;
  return exact(unc.p);
}

// ---- recallWith on the device: |candidates(tree t, query i) ∩ truth_i| --------------------------
// One workgroup per (query, tree): the k truth ids are sorted in LDS, every candidate id of the
// tree's leaf ranges is looked up by bisection and MARKS the truth slot it equals; the marked slots
// are counted.  Marking makes the count a set intersection whatever the ranges hold (the reference
// intersects sets, RPTree.hs:276-282) — and the ranges of one tree are disjoint anyway: a batch
// tree's perm row is a permutation cut into leaves, and a streamed tree's Tips are disjoint slices
// [xoff, xoff + xlen) of its perm row, every inserted point stored in exactly one Tip.
__global__ __launch_bounds__(256) void recall_hits_kernel(const int32_t* __restrict__ truth, int k,
                                                          const int32_t* __restrict__ perm,
                                                          const Range* __restrict__ ranges,
                                                          const int64_t* __restrict__ rng_off, int T,
                                                          int32_t* __restrict__ hits) {
  __shared__ int s_id[1024];
  __shared__ int s_hit[1024];
  __shared__ int s_cnt;
  const int64_t qt = blockIdx.x, q = qt / T;
  int np = 1;
  while (np < k) np <<= 1;
  for (int i = threadIdx.x; i < np; i += blockDim.x) {
    const int id = i < k ? truth[q * k + i] : -1;
    s_id[i] = id < 0 ? 0x7fffffff : id;  // unused slots sort last and equal no candidate
    s_hit[i] = 0;
  }
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  for (int kk = 2; kk <= np; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (np >> 1); i += blockDim.x) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const bool up = (lo & kk) == 0;
        const int a = s_id[lo], b = s_id[hi];
        if (up ? b < a : a < b) {
          s_id[lo] = b;
          s_id[hi] = a;
        }
      }
      __syncthreads();
    }
  for (int64_t r = rng_off[qt]; r < rng_off[qt + 1]; ++r) {
    const Range rg = ranges[r];
    for (int i = threadIdx.x; i < rg.n; i += blockDim.x) {
      const int id = perm[rg.poff + i];
      int lo = 0, hi = np;  // first slot with s_id >= id
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_id[mid] < id) lo = mid + 1;
        else hi = mid;
      }
      if (lo < np && s_id[lo] == id) s_hit[lo] = 1;
    }
  }
  __syncthreads();
  int c = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x) c += s_hit[i];
  if (c) atomicAdd(&s_cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) hits[qt] = s_cnt;
}

}  // namespace

// exhaustive kNN into device arrays [nq][k] (k best by (distance, id); unused slots id -1, +inf):
// dense data under L2 (flags 0) or RPT_KNN_METRIC_COSINE / _INNER through the identity mode of the
// query kernels, CSR data under the true L2 or RPT_KNN_METRIC_REFERENCE through brute_csr_kernel.
// Enqueues on the ctx stream, does not synchronise.
int32_t brute_knn_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int32_t k,
                      int32_t flags, int32_t* ids_dev, double* dist_dev) {
  RPT_ARG(k <= kBuf / 2, "k too large");
  const int64_t nq = q->n;
  if (nq == 0) return RPT_OK;
  DevBuf<int32_t> cnt;
  RPT_TRY(cnt.alloc((size_t)nq));
  if (data->csr)
    return brute_csr(ctx, data, q, k, (flags & RPT_KNN_METRIC_REFERENCE) ? 1 : 0, ids_dev, dist_dev,
                     cnt.p);
  const int32_t metric = flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER);
  if (metric) {
    ctx->last_uncertified = 0;
    ctx->metric_unc_pending = false;
    DevBuf<int32_t> unc;
    RPT_TRY(unc.alloc((size_t)nq));
    return launch_metric(ctx, data, q, nullptr, nullptr, nullptr, 1, 1, k, 0, metric, unc.p, ids_dev,
                         dist_dev, cnt.p);
  }
  if (data->dtype == RPT_F64) {
    ctx->last_uncertified = 0;
    ctx->metric_unc_pending = false;
    DevBuf<int32_t> unc;
    RPT_TRY(unc.alloc((size_t)nq));
    return launch_l2_f64(ctx, data, q, nullptr, nullptr, nullptr, 1, 1, k, 0, unc.p, ids_dev, dist_dev, cnt.p);
  }
  if (data->dtype == RPT_F32)
    return launch_topk_dense<float>(ctx, data, q, nullptr, nullptr, nullptr, 1, 1, k, 0, ids_dev,
                                    dist_dev, cnt.p);
  return launch_topk_dense<__hip_bfloat16>(ctx, data, q, nullptr, nullptr, nullptr, 1, 1, k, 0,
                                           ids_dev, dist_dev, cnt.p);
}

int32_t brute_knn_metric(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int32_t k,
                         int32_t metric, int32_t* ids_host, double* dist_host) {
  const int64_t nq = q->n;
  if (nq == 0) return RPT_OK;
  DevBuf<int32_t> ids;
  DevBuf<double> dist;
  RPT_TRY(ids.alloc((size_t)nq * k));
  RPT_TRY(dist.alloc((size_t)nq * k));
  RPT_TRY(brute_knn_dev(ctx, data, q, k, metric, ids.p, dist.p));
  RPT_HIP(stream_sync(ctx->stream));
  RPT_HIP(hipMemcpy(ids_host, ids.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
  RPT_HIP(hipMemcpy(dist_host, dist.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
  return RPT_OK;
}

int32_t brute_knn(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int32_t k,
                  int32_t* ids_host, double* dist_host) {
  return brute_knn_metric(ctx, data, q, k, 0, ids_host, dist_host);
}

// recallWith (RPTree.hs:276-282) for a query batch, the division left to the caller:
// hits[i][t] = |candidates(tree t, query i) ∩ truth_i|, truth_i = the brute force under `flags`
// ---- cosine / inner product on CSR rows (rpt_knn_csr_metric_*, rpt_brute_knn_csr_metric_*) ----
// arguments checked by the caller: CSR data and queries of one dtype, exactly one metric bit
int32_t knn_csr_metric_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q,
                           int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  RPT_ARG(k <= kBuf / 2, "k too large for the LDS merge buffer");
  RPT_ARG((size_t)data->d * 8 + (sizeof(Entry) + 4) * kBuf <= 150 * 1024, "d too large");
  ctx->last_uncertified = 0;
  ctx->metric_unc_pending = false;
  ctx->last_retries = 0;
  ctx->last_tier = 0;
  QueryPlan pl;
  RPT_TRY(make_plan(ctx, f, q, pl));
  ctx->last_candidates = pl.total_cand;
  if (q->n == 0) return RPT_OK;
  DevBuf<int32_t> unc;
  RPT_TRY(unc.alloc((size_t)q->n));
  RPT_TRY(launch_metric_csr(ctx, data, q, f->perm.p, pl.ranges.p, pl.rng_off.p, f->T, 0, k, flags & 3,
                            flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER), unc.p, ids_dev, dist_dev,
                            count_dev));
  RPT_HIP(stream_sync(ctx->stream));  // the plan's buffers are released on return
  return RPT_OK;
}

// exhaustive: brute_csr_metric_kernel's tiled stream, the exact kernel over the flagged queries.
// Enqueues only.
int32_t brute_knn_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, int32_t k,
                                 int32_t metric, int32_t* ids_dev, double* dist_dev) {
  RPT_ARG(k <= kBuf / 2, "k too large");
  RPT_ARG((size_t)data->d * 8 + (sizeof(Entry) + 4) * kBuf <= 150 * 1024, "d too large");
  ctx->last_uncertified = 0;
  ctx->metric_unc_pending = false;
  const int64_t nq = q->n;
  if (nq == 0) return RPT_OK;
  DevBuf<int32_t> cnt;
  RPT_TRY(cnt.alloc((size_t)nq));
  return brute_csr_metric(ctx, data, q, k, metric, ids_dev, dist_dev, cnt.p);
}

int32_t recall_hits(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q,
                    int32_t k, int32_t flags, int32_t* hits_host, int32_t* truth_ids_host) {
  const int64_t nq = q->n;
  if (nq == 0) return RPT_OK;
  DevBuf<int32_t> ids, hits;
  DevBuf<double> dist;
  RPT_TRY(ids.alloc((size_t)nq * k));
  RPT_TRY(dist.alloc((size_t)nq * k));
  RPT_TRY(hits.alloc((size_t)nq * f->T));
  if (data->csr && (flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER)))  // (rpt_recall_hits_csr_metric_host)
    RPT_TRY(brute_knn_csr_metric_dev(ctx, data, q, k, flags, ids.p, dist.p));
  else
    RPT_TRY(brute_knn_dev(ctx, data, q, k, flags, ids.p, dist.p));
  QueryPlan pl;
  RPT_TRY(make_plan(ctx, f, q, pl));
  hipLaunchKernelGGL(recall_hits_kernel, dim3((unsigned)(nq * f->T)), dim3(256), 0, ctx->stream,
                     ids.p, k, f->perm.p, pl.ranges.p, pl.rng_off.p, f->T, hits.p);
  RPT_HIP(hipGetLastError());
  RPT_HIP(stream_sync(ctx->stream));
  RPT_HIP(hipMemcpy(hits_host, hits.p, (size_t)nq * f->T * 4, hipMemcpyDeviceToHost));
  if (truth_ids_host)
    RPT_HIP(hipMemcpy(truth_ids_host, ids.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
  return RPT_OK;
}

// The exhaustive kNN among the allowed rows into device arrays [nq][k] (unused slots -1 / +inf);
// flags: 0, RPT_KNN_METRIC_COSINE / _INNER, or RPT_KNN_METRIC_REFERENCE (CSR rows).  CSR rows under
// flags 0 (the true L2) stay on the tiled brute_csr_kernel behind its ALLOW switch: its distance is
// the brute force's own (a stored row at exactly 0 from itself), which the list route's
// topk_csr_kernel matches only to 1e-8 |q|.  Every other cell ranks the one list.  Enqueues, then
// synchronises (the list is scratch of this call).
int32_t brute_knn_allow_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q, const uint32_t* allow_dev,
                            int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev) {
  RPT_ARG(k <= kBuf / 2, "k too large");
  RPT_ARG((size_t)data->d * 8 + (sizeof(Entry) + 4) * kBuf <= 150 * 1024, "d too large");
  RPT_ARG(data->n <= 0x7fffffff, "too many rows");
  ctx->last_uncertified = 0;
  ctx->metric_unc_pending = false;
  const int64_t nq = q->n;
  if (nq == 0) return RPT_OK;
  DevBuf<int32_t> list, cnt, unc;
  DevBuf<int64_t> block_off, ro;
  DevBuf<Range> rg;
  if (data->csr && flags == 0) {
    RPT_TRY(cnt.alloc((size_t)nq));
    AllowGroups one;
    one.bits = allow_dev;
    RPT_TRY(brute_csr(ctx, data, q, k, 0, ids_dev, dist_dev, cnt.p, one));
    RPT_HIP(stream_sync(ctx->stream));
    return RPT_OK;
  }
  RPT_TRY(list.alloc((size_t)std::max<int64_t>(data->n, 1)));
  RPT_TRY(block_off.alloc((size_t)allow_list_blocks(data->n) + 1));
  RPT_TRY(rg.alloc((size_t)nq));
  RPT_TRY(ro.alloc((size_t)nq + 1));
  RPT_TRY(cnt.alloc((size_t)nq));
  RPT_TRY(unc.alloc((size_t)nq));
  {
    ProfScope ps(ctx, RPT_PROF_KNN_VOTE);  // class 5: the candidate-list step
    RPT_TRY(allow_list(ctx, allow_dev, data->n, block_off.p, list.p, nq, reinterpret_cast<VoteRange*>(rg.p), ro.p));
  }
  RPT_TRY(launch_lists(ctx, data, q, list.p, rg.p, ro.p, k, 0, flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER),
                       (flags & RPT_KNN_METRIC_REFERENCE) ? 1 : 0, unc.p, ids_dev, dist_dev, cnt.p));
  RPT_HIP(stream_sync(ctx->stream));
  return RPT_OK;
}

namespace {
// rows [q][k] of a pass's scratch answer into the call's, for the queries whose list slot[q] the pass
// built (slots s0 .. s1 - 1); `none` also takes the queries without a list (slot -1: no id allowed)
__global__ void allow_pass_copy_kernel(const int32_t* __restrict__ slot, int32_t s0, int32_t s1, int none, int64_t nq,
                                       int k, const int32_t* __restrict__ si, const double* __restrict__ sd,
                                       int32_t* __restrict__ oi, double* __restrict__ od) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nq * k) return;
  const int32_t sl = slot[e / k];
  if ((sl >= s0 && sl < s1) || (none && sl < 0)) {
    oi[e] = si[e];
    od[e] = sd[e];
  }
}
}  // namespace

// The exhaustive kNN under a grouped allow-list (allow.group non-null).  CSR rows under flags 0 stay on
// brute_csr_kernel, whose tile queries test their own bitmaps.  Every other cell ranks lists: ONE
// ascending id list per group that a query names (and one of all ids when a query is unfiltered),
// concatenated in a slab; query q's single range is {start, length, 0} of its group's list.  The lists
// are sized from their popcounts against a fixed budget of ids per pass (knn_allow_group_budget, else
// the 1 GiB of the other list routes; a list above it is a pass of its own).  More than one pass: each
// pass ranks every query, the queries of other passes over an empty range, into scratch, and its own
// queries' rows are copied out; a query's answer is a function of its list alone, so the budget changes
// no bit.  Returns synchronised.
int32_t brute_knn_allow_group_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* q,
                                  const AllowGroups& allow, int32_t k, int32_t flags, int32_t* ids_dev,
                                  double* dist_dev) {
  RPT_ARG(k <= kBuf / 2, "k too large");
  RPT_ARG((size_t)data->d * 8 + (sizeof(Entry) + 4) * kBuf <= 150 * 1024, "d too large");
  RPT_ARG(data->n <= 0x7fffffff, "too many rows");
  ctx->last_uncertified = 0;
  ctx->metric_unc_pending = false;
  const int64_t nq = q->n, n = data->n;
  if (nq == 0) return RPT_OK;
  DevBuf<int32_t> cnt;
  RPT_TRY(cnt.alloc((size_t)nq));
  if (data->csr && flags == 0) {
    RPT_TRY(brute_csr(ctx, data, q, k, 0, ids_dev, dist_dev, cnt.p, allow));
    RPT_HIP(stream_sync(ctx->stream));
    return RPT_OK;
  }
  // the lists the batch names, in the order of their first query
  // (the map holds at most nq groups whatever G is: the _dev entry point does not validate G)
  std::vector<int32_t> hg((size_t)nq), slot((size_t)nq), sel;
  std::unordered_map<int32_t, int32_t> slot_of;
  RPT_HIP(hipMemcpyAsync(hg.data(), allow.group, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
  RPT_HIP(stream_sync(ctx->stream));
  int32_t all_slot = -1;
  for (int64_t i = 0; i < nq; ++i) {
    const int32_t g = hg[(size_t)i];
    int32_t* at = nullptr;
    if (g == -1) at = &all_slot;
    else if (g >= 0 && g < allow.G) at = &slot_of.emplace(g, -1).first->second;
    if (at && *at < 0) {
      *at = (int32_t)sel.size();
      sel.push_back(g);
    }
    slot[(size_t)i] = at ? *at : -1;
  }
  const int64_t R = (int64_t)sel.size(), nblk = allow_list_blocks(n);
  DevBuf<int32_t> sel_dev, slot_dev, list, unc, si;
  DevBuf<int64_t> block_off, list_off_dev, ro;
  DevBuf<double> sd;
  DevBuf<Range> rg;
  std::vector<int64_t> len((size_t)R, 0), list_off((size_t)R, 0);
  if (R > 0) {
    RPT_TRY(sel_dev.alloc((size_t)R));
    RPT_TRY(block_off.alloc((size_t)(R * (nblk + 1))));
    RPT_TRY(list_off_dev.alloc((size_t)R));
    RPT_HIP(hipMemcpyAsync(sel_dev.p, sel.data(), (size_t)R * 4, hipMemcpyHostToDevice, ctx->stream));
    {
      ProfScope ps(ctx, RPT_PROF_KNN_VOTE);  // class 5: the candidate-list step
      RPT_TRY(allow_group_count(ctx, allow.bits, allow.stride, n, sel_dev.p, R, block_off.p));
    }
    RPT_HIP(hipMemcpy2DAsync(len.data(), 8, block_off.p + nblk, (size_t)(nblk + 1) * 8, 8, (size_t)R,
                             hipMemcpyDeviceToHost, ctx->stream));
    RPT_HIP(stream_sync(ctx->stream));
  }
  // passes: consecutive lists while their ids fit the budget
  const int64_t budget = ctx->opt.knn_allow_group_budget > 0 ? ctx->opt.knn_allow_group_budget : kVoteBudgetWords;
  std::vector<int32_t> pass_end;  // one past the last list of each pass
  int64_t fill = 0, slab = 1;
  for (int64_t r = 0; r < R; ++r) {
    if (r > 0 && fill > 0 && fill + len[(size_t)r] > budget) {
      pass_end.push_back((int32_t)r);
      fill = 0;
    }
    list_off[(size_t)r] = fill;
    fill += len[(size_t)r];
    slab = std::max(slab, fill);
  }
  pass_end.push_back((int32_t)R);  // (no list at all: one pass of empty ranges)
  const bool multi = pass_end.size() > 1;
  RPT_TRY(list.alloc((size_t)slab));
  RPT_TRY(rg.alloc((size_t)nq));
  RPT_TRY(ro.alloc((size_t)nq + 1));
  RPT_TRY(unc.alloc((size_t)nq));
  if (R > 0) RPT_HIP(hipMemcpyAsync(list_off_dev.p, list_off.data(), (size_t)R * 8, hipMemcpyHostToDevice, ctx->stream));
  std::vector<int64_t> hro((size_t)nq + 1);
  for (int64_t i = 0; i <= nq; ++i) hro[(size_t)i] = i;
  RPT_HIP(hipMemcpyAsync(ro.p, hro.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (multi) {
    RPT_TRY(si.alloc((size_t)nq * k));
    RPT_TRY(sd.alloc((size_t)nq * k));
    RPT_TRY(slot_dev.alloc((size_t)nq));
    RPT_HIP(hipMemcpyAsync(slot_dev.p, slot.data(), (size_t)nq * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  RPT_HIP(stream_sync(ctx->stream));  // (the host vectors above may go)
  std::vector<Range> hr((size_t)nq);
  int64_t uncertified = 0;
  int32_t s0 = 0;
  for (size_t p = 0; p < pass_end.size(); ++p) {
    const int32_t s1 = pass_end[p];
    if (s1 > s0) {
      ProfScope ps(ctx, RPT_PROF_KNN_VOTE);
      RPT_TRY(allow_group_scatter(ctx, allow.bits, allow.stride, n, sel_dev.p + s0, s1 - s0,
                                  block_off.p + (int64_t)s0 * (nblk + 1), list_off_dev.p + s0, list.p));
    }
    for (int64_t i = 0; i < nq; ++i) {
      const int32_t sl = slot[(size_t)i];
      const bool mine = sl >= s0 && sl < s1;
      hr[(size_t)i] = Range{mine ? list_off[(size_t)sl] : 0, mine ? (int32_t)len[(size_t)sl] : 0, 0};
    }
    RPT_HIP(hipMemcpyAsync(rg.p, hr.data(), (size_t)nq * sizeof(Range), hipMemcpyHostToDevice, ctx->stream));
    RPT_HIP(stream_sync(ctx->stream));  // (hr is written again by the next pass)
    RPT_TRY(launch_lists(ctx, data, q, list.p, rg.p, ro.p, k, 0, flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER),
                         (flags & RPT_KNN_METRIC_REFERENCE) ? 1 : 0, unc.p, multi ? si.p : ids_dev,
                         multi ? sd.p : dist_dev, cnt.p));
    if (multi) {
      // The statistic is a sum over the queries, so a pass counts its OWN queries only (the others rank an
      // empty range here and their real list in another pass): the launch's list of uncertified queries
      // (unc[0 .. count), query numbers) is read back, or, where a launch reports every query (the
      // *_exact options), the pass's own queries are taken for it.
      const bool first = p == 0;
      auto own = [&](int64_t i) {
        const int32_t sl = slot[(size_t)i];
        return (sl >= s0 && sl < s1) || (first && sl < 0);
      };
      if (ctx->metric_unc_pending) {
        unsigned long long nu = 0;
        RPT_HIP(hipMemcpyAsync(&nu, ctx->metric_unc_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
        RPT_HIP(stream_sync(ctx->stream));
        nu = std::min<unsigned long long>(nu, (unsigned long long)nq);
        std::vector<int32_t> hu((size_t)nu);
        if (nu) RPT_HIP(hipMemcpy(hu.data(), unc.p, (size_t)nu * 4, hipMemcpyDeviceToHost));
        for (const int32_t i : hu) uncertified += i >= 0 && i < nq && own(i) ? 1 : 0;
      } else if (ctx->last_uncertified == nq) {
        for (int64_t i = 0; i < nq; ++i) uncertified += own(i) ? 1 : 0;
      } else {
        uncertified += ctx->last_uncertified;
      }
      const int64_t el = nq * k;
      hipLaunchKernelGGL(allow_pass_copy_kernel, dim3((unsigned)((el + 255) / 256)), dim3(256), 0, ctx->stream,
                         slot_dev.p, s0, s1, p == 0 ? 1 : 0, nq, k, si.p, sd.p, ids_dev, dist_dev);
      RPT_HIP(hipGetLastError());
      RPT_HIP(stream_sync(ctx->stream));  // the slab and the ranges are written again by the next pass
    }
    s0 = s1;
  }
  if (multi) {
    ctx->last_uncertified = uncertified;
    ctx->metric_unc_pending = false;
  }
  RPT_HIP(stream_sync(ctx->stream));
  return RPT_OK;
}

// recall_hits with the truth taken among the allowed rows (brute_knn_allow_dev).  The truth holds
// allowed rows only, so the trees' unfiltered candidates intersect it as the allowed ones would.
int32_t recall_hits_allow(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* q,
                          const AllowGroups& allow, int32_t k, int32_t flags, int32_t* hits_host,
                          int32_t* truth_ids_host) {
  const int64_t nq = q->n;
  if (nq == 0) return RPT_OK;
  DevBuf<int32_t> ids, hits;
  DevBuf<double> dist;
  RPT_TRY(ids.alloc((size_t)nq * k));
  RPT_TRY(dist.alloc((size_t)nq * k));
  RPT_TRY(hits.alloc((size_t)nq * f->T));
  if (allow.group) RPT_TRY(brute_knn_allow_group_dev(ctx, data, q, allow, k, flags, ids.p, dist.p));
  else RPT_TRY(brute_knn_allow_dev(ctx, data, q, allow.bits, k, flags, ids.p, dist.p));
  QueryPlan pl;
  RPT_TRY(make_plan(ctx, f, q, pl));
  hipLaunchKernelGGL(recall_hits_kernel, dim3((unsigned)(nq * f->T)), dim3(256), 0, ctx->stream, ids.p, k,
                     f->perm.p, pl.ranges.p, pl.rng_off.p, f->T, hits.p);
  RPT_HIP(hipGetLastError());
  RPT_HIP(stream_sync(ctx->stream));
  RPT_HIP(hipMemcpy(hits_host, hits.p, (size_t)nq * f->T * 4, hipMemcpyDeviceToHost));
  if (truth_ids_host) RPT_HIP(hipMemcpy(truth_ids_host, ids.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
  return RPT_OK;
}

}  // namespace rpt
