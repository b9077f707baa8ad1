// graph_csr.hip — the kNN graph of the indexed points and its NN-descent rounds on SVector (CSR)
// rows under L2 (rpt_knn_graph_csr_*, rpt_knn_graph_refine_csr_*) and under the cosine / inner-product
// distances (rpt_knn_graph_csr_metric_*, rpt_knn_graph_refine_csr_metric_*; behind the L2 notes).
//
// dist(i, j) is graph.hip's: metricDDL2 as a left fold in double over dense(x_i), dense(x_j), the
// rows with every absent column as +0.0.  A column where both rows hold +0.0 adds (+0.0 - +0.0)^2 =
// +0.0 to an accumulator that starts at +0.0 and is a sum of squares, so never -0.0: acc + (+0.0)
// is acc, bit for bit.  The fold over ANY ascending set of columns that contains the union of the
// two supports therefore gives the bits of the fold over all d columns, and no kernel here visits
// all d columns.  The translation unit is built with -ffp-contract=off.
//
//   graph_csr_leaf_kernel   graph.hip's graph_leaf_kernel (one workgroup per leaf of up to 128
//                           rows, every pair once) with another staging: a chunk is a WINDOW of 32
//                           columns [c0, c0 + 32); the P x kLS buffer is zeroed and every row
//                           scatters its nonzeros of the window into it.  Two lanes own a row (its
//                           cursor lives in their registers; the columns ascend, so a cursor only
//                           moves forward).  The next c0 is the smallest column any cursor of the
//                           leaf points at: windows in which the leaf holds nothing are never
//                           staged or folded.
//   graph_csr_tiled_kernel  graph.hip's graph_tiled_kernel (64 rows of a leaf against the leaf in
//                           blocks of 64, any leaf size) with the same windows over the 64 + 64
//                           rows of the two blocks.
//   refine_join_csr_kernel  graph_refine.hip's refine_join_kernel (one wave per point, the hash
//                           set, wave_merge) with the distances of the new candidates by a
//                           two-pointer merge: a candidate per lane walks its own row against
//                           x_i's (column, value) pairs, which pass through LDS in pieces of 64, so
//                           a long row needs no more LDS than a short one.
// Rows whose columns do not ascend strictly give an unspecified answer; every access stays inside
// the row (a cursor never passes its row's end, a scatter checks its window) and every loop
// advances a cursor, so the kernels stay in bounds and terminate.
//
// Cosine / inner product: the same three kernels instantiated on the distance (M), as graph.hip's.
// dist(i, j) comes from dotS(x_i, x_j): the left fold acc + x_c * y_c from +0.0 over the columns
// stored in BOTH rows, ascending (rptree_hip.h).  Under cosine the rows' cached dotS(x, x)
// (rpt_dataset::sqnorm) travel next to the ids.
//   Zero-filled windows give dotS while every stored value is finite: a column one row lacks adds
//   x * (+0.0) = +-0.0, and an acc that starts at +0.0 is never -0.0 (a sum is -0.0 only when both
//   operands are), so acc + (+-0.0) is acc.  This is the path that is timed.
//   A stored inf or NaN breaks that (inf * 0 = NaN where dotS takes no product at all).  The leaf
//   kernels therefore read the data set's statistic stats[0] (knn.hip row_sqnorm_csr_kernel: the
//   largest dotS(x, x), as bits; finite exactly when every stored value is finite and no square
//   overflows) on the device and branch uniformly: when it is not finite, or with the context option
//   graph_csr_masked, every staged row also leaves a 32-bit presence word (bit c: the row stores
//   column c0 + c) and a product is folded only where both rows' bits are set.  Nothing is read
//   back to the host, and the answer does not depend on the path.
//   The join's two-pointer merge needs no mask: under a metric it folds a step only when both sides
//   take (ci == cj), and nothing is left to fold behind x_i's last column.
#include <string.h>

#include <algorithm>

#include "graph_refine_dev.h"

namespace rpt {
namespace {

constexpr int kLeafMax = 128;   // largest leaf of graph_csr_leaf_kernel
constexpr int kTB = 64;         // rows / columns of a block of graph_csr_tiled_kernel
constexpr int kThreads = 256;
constexpr int kLdsMax = 160 * 1024;
constexpr int kNoCol = 0x7fffffff;  // a cursor at its row's end
constexpr int kPiece = 64;      // (column, value) pairs of x_i per LDS piece of the join

struct GBlock {  // graph.hip's: rows [row0, row0 + 64) (tiled) or all rows (leaf kernel) of a leaf
  int64_t off;
  int32_t n;
  int32_t row0;
};

// graph.hip's tile_fold: 4 x 4 pairs over cw columns
template <int M>
__device__ inline void tile_fold(const double* bufA, int ra, int sa, const double* bufB, int rb,
                                 int sb, int cw, double (&acc)[16]) {
  const double* pa = bufA + ra * kLS;
  const double* pb = bufB + rb * kLS;
#pragma unroll 2
  for (int c = 0; c < cw; ++c) {
    double a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = pa[u * sa * kLS + c];
#pragma unroll
    for (int v = 0; v < 4; ++v) b[v] = pb[v * sb * kLS + c];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u * 4 + v] = fold_step<M>(acc[u * 4 + v], a[u], b[v]);
  }
}

// tile_fold under a metric with presence words (pmA / pmB: one per buffer row, bit c = the row
// stores column c of the window): a product enters only where both rows store the column, and a
// column that no pair of the tile shares is not read at all
template <int M>
__device__ inline void tile_fold_masked(const double* bufA, int ra, int sa, const unsigned* pmA,
                                        const double* bufB, int rb, int sb, const unsigned* pmB,
                                        int cw, double (&acc)[16]) {
  const double* pa = bufA + ra * kLS;
  const double* pb = bufB + rb * kLS;
  unsigned ma[4], mb[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) ma[u] = pmA[ra + u * sa];
#pragma unroll
  for (int v = 0; v < 4; ++v) mb[v] = pmB[rb + v * sb];
  unsigned todo = (ma[0] | ma[1] | ma[2] | ma[3]) & (mb[0] | mb[1] | mb[2] | mb[3]);
  if (cw < 32) todo &= (1u << cw) - 1u;
  while (todo) {  // ascending columns
    const int c = __ffs((int)todo) - 1;
    todo &= todo - 1u;
    double a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = pa[u * sa * kLS + c];
#pragma unroll
    for (int v = 0; v < 4; ++v) b[v] = pb[v * sb * kLS + c];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if ((ma[u] & mb[v]) >> c & 1u) acc[u * 4 + v] = fold_step<M>(acc[u * 4 + v], a[u], b[v]);
  }
}

// whether the metric kernels take the presence-masked fold: forced, or the largest dotS(x, x) of the
// data set (stats[0], its bits with the sign cleared) is inf or NaN
__device__ inline bool masked_fold(const unsigned long long* __restrict__ stats, int force) {
  return force != 0 || stats[0] >= 0x7ff0000000000000ULL;
}

__global__ void graph_csr_init_kernel(int64_t n, int k, int32_t* __restrict__ ids,
                                      double* __restrict__ dist, int32_t* __restrict__ count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * k; i += stride) {
    ids[i] = -1;
    dist[i] = pos_inf();
    if (i < n) count[i] = 0;
  }
}

// The cursor of one row, held by the two lanes 2 r and 2 r + 1 of a wave (h = lane & 1): pos is
// the row's first entry no window has taken yet, next its column (kNoCol at the end).
struct RowCursor {
  int64_t pos, end;
  int next;
};

template <class TV>
__device__ inline void cursor_open(RowCursor& rc, int id, const int64_t* __restrict__ rowptr,
                                   const int32_t* __restrict__ col) {
  rc.pos = rc.end = 0;
  rc.next = kNoCol;
  if (id >= 0) {
    rc.pos = rowptr[id];
    rc.end = rowptr[id + 1];
    if (rc.pos < rc.end) rc.next = col[rc.pos];
  }
}

// smallest `next` of the workgroup (all kThreads threads call it; wmin: 4 ints of LDS).  The
// barrier inside also ends the reads of the last window's buffer.
__device__ inline int block_min_col(int v, int* wmin) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = v;
  __syncthreads();
  const int a = wmin[0] < wmin[1] ? wmin[0] : wmin[1], b = wmin[2] < wmin[3] ? wmin[2] : wmin[3];
  return a < b ? a : b;
}

// The window [c0, c0 + cw) of one row into brow[0 .. cw): the row's two lanes zero it, then scatter
// the row's entries of the window, one taking the even and one the odd entries from the cursor on.
// Both lanes of a pair call it together (live == the pair owns a buffer row).  kMask: returns the
// presence bits of the entries THIS lane scattered (bit c: column c0 + c), else 0.
template <class TV, bool kMask = false>
__device__ inline unsigned stage_window(RowCursor& rc, bool live, int h, int c0, int cw, double* brow,
                                        const int32_t* __restrict__ col, const TV* __restrict__ val) {
  [[maybe_unused]] unsigned bits = 0;
  if (live)
    for (int c = h; c < cw; c += 2) brow[c] = 0.0;
  wave_sync();  // the pair's zeros are in place before either lane scatters
  int64_t at = rc.pos + h;
  const int c1 = c0 + cw;
  while (at < rc.end) {
    const int c = col[at];
    if (c >= c1) break;
    if (live && c >= c0) {
      brow[c - c0] = widen(val[at]);
      if constexpr (kMask) bits |= 1u << (c - c0);
    }
    at += 2;
  }
  const int64_t other = __shfl_xor(at, 1);
  int64_t np = at < other ? at : other;  // the first entry at or behind the window's end
  if (np > rc.end) np = rc.end;
  rc.pos = np;
  rc.next = np < rc.end ? col[np] : kNoCol;
  return bits;
}

// ---- leaves of up to 128 points: one workgroup per leaf, every pair once ----------------------
// dynamic LDS: lds_doubles = max(4 ng (4 ng + 1), 4 ng * kLS) doubles (the window, later the
// distance matrix), then 4 ng ints (the leaf's ids) and 4 ints (the waves' smallest columns).
// Cosine: 4 ng more doubles, the rows' norms rn[id], at the END of the doubles (graph.hip's place).
// Cosine / inner: 4 ng more ints behind the others, the presence words of the staged rows.
template <class TV, int M>
__global__ __launch_bounds__(kThreads) void graph_csr_leaf_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const TV* __restrict__ val,
    int d, const int32_t* __restrict__ perm_t, const GBlock* __restrict__ blocks, int k,
    int lds_doubles, int32_t* __restrict__ ids, double* __restrict__ dist,
    int32_t* __restrict__ count, const double* __restrict__ rn,
    const unsigned long long* __restrict__ stats, int force_masked) {
  extern __shared__ double smem[];
  double* buf = smem;
  int* sid = reinterpret_cast<int*>(smem + lds_doubles);
  const GBlock blk = blocks[blockIdx.x];
  const int s = blk.n;
  if (s < 2) return;  // no mates in this tree
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ng = (s + 3) >> 2;  // row groups: group g holds the rows g, g + ng, g + 2 ng, g + 3 ng
  const int P = 4 * ng;
  int* wmin = sid + P;
  [[maybe_unused]] unsigned* pmask = reinterpret_cast<unsigned*>(wmin + 4);
  [[maybe_unused]] double* snorm = smem + lds_doubles - P;
  bool masked = false;  // L2: a constant, the masked branch is not instantiated
  if constexpr (M != kGraphL2) masked = masked_fold(stats, force_masked);
  for (int r = tid; r < P; r += kThreads) {
    const int id = r < s ? perm_t[blk.off + r] : -1;
    sid[r] = id;
    if constexpr (M == kGraphCosine) snorm[r] = id >= 0 ? rn[id] : 0.0;
  }

  // tiles (gi <= gj) of the upper triangle, row-major; up to three per lane
  const int ntiles = ng * (ng + 1) / 2;
  int gi[3], gj[3];
  double acc[3][16];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    int t = tid + u * kThreads;
    int g = 0;
    if (t < ntiles) {
      while (t >= ng - g) {
        t -= ng - g;
        ++g;
      }
      gi[u] = g;
      gj[u] = g + t;
    } else {
      gi[u] = -1;
      gj[u] = -1;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[u][e] = 0.0;
  }

  // the row of this lane pair (P <= 128: every row has its pair)
  const int myrow = tid >> 1, h = tid & 1;
  const bool live = myrow < P;
  RowCursor rc;
  cursor_open<TV>(rc, live && myrow < s ? perm_t[blk.off + myrow] : -1, rowptr, col);
  for (;;) {
    const int c0 = block_min_col(rc.next, wmin);  // ... and the last window has been read
    if (c0 == kNoCol) break;
    const int cw = d - c0 < kCW ? d - c0 : kCW;
    if (!masked) {
      stage_window<TV>(rc, live, h, c0, cw, buf + myrow * kLS, col, val);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 3; ++u)
        if (gi[u] >= 0) tile_fold<M>(buf, gi[u], ng, buf, gj[u], ng, cw, acc[u]);
    } else if constexpr (M != kGraphL2) {
      unsigned bits = stage_window<TV, true>(rc, live, h, c0, cw, buf + myrow * kLS, col, val);
      bits |= __shfl_xor(bits, 1);
      if (live && h == 0) pmask[myrow] = bits;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 3; ++u)
        if (gi[u] >= 0) tile_fold_masked<M>(buf, gi[u], ng, pmask, buf, gj[u], ng, pmask, cw, acc[u]);
    }
  }
  __syncthreads();

  // the distances, both ways, into the matrix D[P][SD]
  const int SD = P + 1;
  double* D = smem;
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (gi[u] >= 0) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int ri = gi[u] + ng * a, rj = gj[u] + ng * b;
          double v;
          if constexpr (M == kGraphCosine) v = fold_finish<M>(acc[u][a * 4 + b], snorm[ri], snorm[rj]);
          else v = fold_finish<M>(acc[u][a * 4 + b], 0.0, 0.0);
          D[ri * SD + rj] = v;
          D[rj * SD + ri] = v;
        }
    }
  __syncthreads();

  // one wave per row, four rows' lists in flight
  for (int r0 = wave; r0 < s; r0 += 16) {
    double ld[4];
    int lid[4], lc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + 4 * u;
      lc[u] = 0;
      ld[u] = pos_inf();
      lid[u] = -1;
      if (r < s) {
        const int64_t g = sid[r];
        int c = count[g];
        c = c < 0 ? 0 : (c > k ? k : c);
        lc[u] = c;
        if (lane < c) {
          ld[u] = dist[g * k + lane];
          lid[u] = ids[g * k + lane];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + 4 * u;
      if (r >= s) break;
      const int me = sid[r];
      const int j0 = lane, j1 = lane + 64;
      const int ci0 = j0 < s ? sid[j0] : -1, ci1 = j1 < s ? sid[j1] : -1;
      const bool v0 = j0 < s && j0 != r && ci0 != me, v1 = j1 < s && j1 != r && ci1 != me;
      const double cd0 = j0 < P ? D[r * SD + j0] : 0.0, cd1 = j1 < P ? D[r * SD + j1] : 0.0;
      int c = lc[u];
      if (wave_merge(ld[u], lid[u], c, k, cd0, ci0, v0, cd1, ci1, v1)) {
        const int64_t g = me;
        if (lane < k) {
          dist[g * k + lane] = lane < c ? ld[u] : pos_inf();
          ids[g * k + lane] = lane < c ? lid[u] : -1;
        }
        if (lane == 0) count[g] = c;
      }
    }
  }
}

// ---- any leaf: 64 rows of a leaf per workgroup against the leaf in blocks of 64 ---------------
// dynamic LDS: 2 * 64 * kLS doubles (the windows of the two blocks, rows 0 .. 63 and 64 .. 127 of
// one buffer; later the 64 x 65 distance block), 64 k doubles (the rows' lists), then ints: 64 k
// list ids, 64 counts, 64 changed flags, 64 + 64 row ids, 4 smallest columns.  Cosine: 64 + 64 more
// doubles behind the lists' (the norms of the two blocks' rows).  Cosine / inner: 64 + 64 more ints
// at the end, the presence words of the staged rows.
template <class TV, int M>
__global__ __launch_bounds__(kThreads) void graph_csr_tiled_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const TV* __restrict__ val,
    int d, const int32_t* __restrict__ perm_t, const GBlock* __restrict__ blocks, int k,
    int32_t* __restrict__ ids, double* __restrict__ dist, int32_t* __restrict__ count,
    const double* __restrict__ rn, const unsigned long long* __restrict__ stats, int force_masked) {
  extern __shared__ double smem[];
  constexpr int kNorms = M == kGraphCosine ? 2 * kTB : 0;
  double* bufA = smem;
  double* bufB = smem + kTB * kLS;
  double* lst_d = smem + 2 * kTB * kLS;
  [[maybe_unused]] double* nrmA = lst_d + kTB * k;
  [[maybe_unused]] double* nrmB = nrmA + kTB;
  int* lst_i = reinterpret_cast<int*>(lst_d + kTB * k + kNorms);
  int* lst_c = lst_i + kTB * k;
  int* lst_ch = lst_c + kTB;
  int* sidA = lst_ch + kTB;
  int* sidB = sidA + kTB;
  int* wmin = sidB + kTB;
  [[maybe_unused]] unsigned* pmask = reinterpret_cast<unsigned*>(wmin + 4);
  const GBlock blk = blocks[blockIdx.x];
  const int s = blk.n;
  if (s < 2) return;
  bool masked = false;  // L2: a constant, the masked branch is not instantiated
  if constexpr (M != kGraphL2) masked = masked_fold(stats, force_masked);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nr = s - blk.row0 < kTB ? s - blk.row0 : kTB;
  if (tid < kTB) {
    const int g = tid < nr ? perm_t[blk.off + blk.row0 + tid] : -1;
    sidA[tid] = g;
    if constexpr (M == kGraphCosine) nrmA[tid] = g >= 0 ? rn[g] : 0.0;
    int c = g >= 0 ? count[g] : 0;
    lst_c[tid] = c < 0 ? 0 : (c > k ? k : c);
    lst_ch[tid] = 0;
  }
  __syncthreads();
  for (int p = tid; p < nr * k; p += kThreads) {
    const int r = p / k, e = p - r * k;
    if (e < lst_c[r]) {
      const int64_t g = sidA[r];
      lst_d[p] = dist[g * k + e];
      lst_i[p] = ids[g * k + e];
    }
  }
  const int gi = tid >> 4, gj = tid & 15;  // rows gi + 16 u against columns gj + 16 v
  constexpr int SD = kTB + 1;
  const int myrow = tid >> 1, h = tid & 1;  // 0 .. 63: the block's rows, 64 .. 127: the leaf's points

  for (int cb = 0; cb < s; cb += kTB) {
    const int nc = s - cb < kTB ? s - cb : kTB;
    __syncthreads();  // the last block's selection is over
    if (tid < kTB) {
      const int g = tid < nc ? perm_t[blk.off + cb + tid] : -1;
      sidB[tid] = g;
      if constexpr (M == kGraphCosine) nrmB[tid] = g >= 0 ? rn[g] : 0.0;
    }
    RowCursor rc;
    {
      int id = -1;
      if (myrow < kTB) {
        if (myrow < nr) id = perm_t[blk.off + blk.row0 + myrow];
      } else if (myrow - kTB < nc) {
        id = perm_t[blk.off + cb + myrow - kTB];
      }
      cursor_open<TV>(rc, id, rowptr, col);
    }
    double acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
    for (;;) {
      const int c0 = block_min_col(rc.next, wmin);
      if (c0 == kNoCol) break;
      const int cw = d - c0 < kCW ? d - c0 : kCW;
      if (!masked) {
        stage_window<TV>(rc, true, h, c0, cw, smem + myrow * kLS, col, val);
        __syncthreads();
        tile_fold<M>(bufA, gi, 16, bufB, gj, 16, cw, acc);
      } else if constexpr (M != kGraphL2) {
        unsigned bits = stage_window<TV, true>(rc, true, h, c0, cw, smem + myrow * kLS, col, val);
        bits |= __shfl_xor(bits, 1);
        if (h == 0) pmask[myrow] = bits;
        __syncthreads();
        tile_fold_masked<M>(bufA, gi, 16, pmask, bufB, gj, 16, pmask + kTB, cw, acc);
      }
    }
    __syncthreads();
    double* D = smem;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        double v;
        if constexpr (M == kGraphCosine) v = fold_finish<M>(acc[a * 4 + b], nrmA[gi + 16 * a], nrmB[gj + 16 * b]);
        else v = fold_finish<M>(acc[a * 4 + b], 0.0, 0.0);
        D[(gi + 16 * a) * SD + gj + 16 * b] = v;
      }
    __syncthreads();
    for (int r = wave; r < nr; r += 4) {
      const int me = sidA[r];
      int c = lst_c[r];
      double ld = lane < c ? lst_d[r * k + lane] : pos_inf();
      int lid = lane < c ? lst_i[r * k + lane] : -1;
      const int ci0 = sidB[lane];
      const bool v0 = lane < nc && cb + lane != blk.row0 + r && ci0 != me;
      if (wave_merge(ld, lid, c, k, D[r * SD + lane], ci0, v0, 0.0, -1, false)) {
        if (lane < c) {
          lst_d[r * k + lane] = ld;
          lst_i[r * k + lane] = lid;
        }
        if (lane == 0) {
          lst_c[r] = c;
          lst_ch[r] = 1;
        }
      }
    }
  }
  __syncthreads();
  for (int p = tid; p < nr * k; p += kThreads) {
    const int r = p / k, e = p - r * k;
    if (!lst_ch[r]) continue;
    const int64_t g = sidA[r];
    const bool on = e < lst_c[r];
    dist[g * k + e] = on ? lst_d[p] : pos_inf();
    ids[g * k + e] = on ? lst_i[p] : -1;
    if (e == 0) count[g] = lst_c[r];
  }
}

template <class TV, int M>
int32_t launch_graph_csr(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                         bool general, int smax, const GBlock* blocks_dev, int64_t nblocks,
                         int32_t* ids, double* dist, int32_t* count) {
  const TV* val = static_cast<const TV*>(data->val);
  const int d = data->d;
  // the norms, and behind them the statistics (ensure_sqnorm); L2 reads neither
  const double* rn = M == kGraphL2 ? nullptr : data->sqnorm;
  const unsigned long long* stats =
      M == kGraphL2 ? nullptr : reinterpret_cast<const unsigned long long*>(data->sqnorm + data->n);
  const int force = ctx->opt.graph_csr_masked != 0;
  static DeviceOnce attr_once[2];
  if (!general) {
    const int ng = (smax + 3) / 4, P = 4 * ng;
    const int lds_doubles = std::max(P * (P + 1), P * kLS) + (M == kGraphCosine ? P : 0);
    const size_t smem = (size_t)lds_doubles * 8 + (size_t)(P + 4 + (M == kGraphL2 ? 0 : P)) * 4;
    RPT_TRY(attr_once[0].run(ctx->device, [&]() -> int32_t {
      RPT_HIP(hipFuncSetAttribute((const void*)graph_csr_leaf_kernel<TV, M>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
      return RPT_OK;
    }));
    for (int32_t t = 0; t < f->T; ++t)
      hipLaunchKernelGGL((graph_csr_leaf_kernel<TV, M>), dim3((unsigned)nblocks), dim3(kThreads), smem,
                         ctx->stream, data->rowptr, data->col, val, d,
                         f->perm.p + (int64_t)t * f->n, blocks_dev, k, lds_doubles, ids, dist, count,
                         rn, stats, force);
  } else {
    const size_t smem = (size_t)(2 * kTB * kLS + kTB * k + (M == kGraphCosine ? 2 * kTB : 0)) * 8 +
                        (size_t)(kTB * k + 4 * kTB + 4 + (M == kGraphL2 ? 0 : 2 * kTB)) * 4;
    RPT_TRY(attr_once[1].run(ctx->device, [&]() -> int32_t {
      RPT_HIP(hipFuncSetAttribute((const void*)graph_csr_tiled_kernel<TV, M>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
      return RPT_OK;
    }));
    for (int32_t t = 0; t < f->T; ++t)
      hipLaunchKernelGGL((graph_csr_tiled_kernel<TV, M>), dim3((unsigned)nblocks), dim3(kThreads), smem,
                         ctx->stream, data->rowptr, data->col, val, d,
                         f->perm.p + (int64_t)t * f->n, blocks_dev, k, ids, dist, count, rn, stats,
                         force);
  }
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

template <class TV>
int32_t launch_graph_csr_metric(int m, rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                bool general, int smax, const GBlock* blocks_dev, int64_t nblocks,
                                int32_t* ids, double* dist, int32_t* count) {
  if (m == kGraphCosine)
    return launch_graph_csr<TV, kGraphCosine>(ctx, f, data, k, general, smax, blocks_dev, nblocks, ids, dist, count);
  if (m == kGraphInner)
    return launch_graph_csr<TV, kGraphInner>(ctx, f, data, k, general, smax, blocks_dev, nblocks, ids, dist, count);
  return launch_graph_csr<TV, kGraphL2>(ctx, f, data, k, general, smax, blocks_dev, nblocks, ids, dist, count);
}

// dynamic LDS, per wave (wave_bytes): kPiece doubles and kPiece ints (a piece of x_i's values and
// columns), H ints (the hash set, later the new candidates), k + r ints (B(i)).  rn: the rows'
// dotS(x, x) (cosine only).
template <class TV, int M>
__global__ __launch_bounds__(256) void refine_join_csr_kernel(
    RefineState* st, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const TV* __restrict__ val, int64_t n, int k, int r, int H, int wave_bytes,
    const int32_t* __restrict__ ids, const double* __restrict__ dist,
    const int32_t* __restrict__ count, const int64_t* __restrict__ roff,
    const int32_t* __restrict__ rsrc, const double* __restrict__ rdist, int32_t* __restrict__ oids,
    double* __restrict__ odist, int32_t* __restrict__ ocount, const double* __restrict__ rn) {
  if (!st->active) return;
  extern __shared__ double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  double* pv = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * wave_bytes);
  int* pc = reinterpret_cast<int*>(pv + kPiece);
  int* tab = pc + kPiece;
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

    const int64_t ib = rowptr[i], ie = rowptr[i + 1];
    [[maybe_unused]] double ni = 0.0;
    if constexpr (M == kGraphCosine) ni = rn[i];
    bool changed = false;
    for (int b0 = 0; b0 < m; b0 += 64) {
      const int nrows = m - b0 < 64 ? m - b0 : 64;
      const int my = lane < nrows ? tab[b0 + lane] : -1;
      // this lane's candidate row: [jp, je), cj / vj its entry at jp (kNoCol: the row is over)
      int64_t jp = 0, je = 0;
      if (my >= 0) {
        jp = rowptr[my];
        je = rowptr[my + 1];
      }
      int cj = kNoCol;
      double vj = 0.0;
      if (jp < je) {
        cj = col[jp];
        vj = widen(val[jp]);
      }
      double acc = 0.0;
      for (int64_t p0 = ib; p0 < ie; p0 += kPiece) {
        const int np = ie - p0 < kPiece ? (int)(ie - p0) : kPiece;
        wave_sync();  // the last piece has been read
        if (lane < np) {
          pc[lane] = col[p0 + lane];
          pv[lane] = widen(val[p0 + lane]);
        }
        wave_sync();
        if (my >= 0) {
          int ii = 0;
          while (ii < np) {  // every step takes an entry of x_i or of the candidate
            const int ci = pc[ii];
            const bool take_i = ci <= cj, take_j = cj <= ci;
            if constexpr (M == kGraphL2) {
              acc = fold_step<kGraphL2>(acc, take_i ? pv[ii] : 0.0, take_j ? vj : 0.0);
            } else {  // dotS: only a column both rows store
              if (take_i && take_j) acc = fold_step<M>(acc, pv[ii], vj);
            }
            if (take_i) ++ii;
            if (take_j) {
              ++jp;
              cj = kNoCol;
              if (jp < je) {
                cj = col[jp];
                vj = widen(val[jp]);
              }
            }
          }
        }
      }
      if constexpr (M == kGraphL2) {
        while (jp < je) {  // what the candidate holds behind x_i's last column
          acc = fold_step<kGraphL2>(acc, 0.0, vj);
          ++jp;
          if (jp < je) vj = widen(val[jp]);
        }
      }
      double dv;
      if constexpr (M == kGraphL2) dv = fold_finish<kGraphL2>(acc, 0.0, 0.0);
      else if constexpr (M == kGraphCosine) dv = fold_finish<M>(acc, ni, my >= 0 ? rn[my] : 0.0);
      else dv = fold_finish<M>(acc, 0.0, 0.0);
      changed |= wave_merge(ld, lid, c, k, dv, my, lane < nrows, 0.0, -1, false);
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

template <class TV, int M>
int32_t launch_join_csr(rpt_ctx* ctx, RefineState* st, const rpt_dataset* data, int k, int r, int H,
                        int wave_bytes, int W, const int32_t* ids, const double* dist,
                        const int32_t* count, const int64_t* roff, const int32_t* rsrc,
                        const double* rdist, int32_t* oids, double* odist, int32_t* ocount) {
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)refine_join_csr_kernel<TV, M>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  const int64_t want = (data->n + W - 1) / W;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->n_cu * 16));
  hipLaunchKernelGGL((refine_join_csr_kernel<TV, M>), dim3(grid), dim3(64 * W), (size_t)wave_bytes * W,
                     ctx->stream, st, data->rowptr, data->col, static_cast<const TV*>(data->val),
                     data->n, k, r, H, wave_bytes, ids, dist, count, roff, rsrc, rdist, oids, odist,
                     ocount, M == kGraphCosine ? data->sqnorm : nullptr);
  return RPT_OK;
}

template <class TV, class... A>
int32_t launch_join_csr_metric(int m, A&&... a) {
  if (m == kGraphCosine) return launch_join_csr<TV, kGraphCosine>(a...);
  if (m == kGraphInner) return launch_join_csr<TV, kGraphInner>(a...);
  return launch_join_csr<TV, kGraphL2>(a...);
}

}  // namespace

int32_t knn_graph_csr_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                          int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                          int32_t* count_dev) {
  ctx->last_graph_pairs = 0;
  if (f->n == 0) return RPT_OK;
  const int m = graph_metric_of(metric);
  // the rows' dotS(x, x) and their statistics, cached on the dataset: the inner product reads the
  // statistics too (which fold the leaf kernels take)
  if (m != kGraphL2) RPT_TRY(ensure_sqnorm(ctx, data));
  // the leaf table: the same for every tree (Internal.hs:289,495,503)
  std::vector<Node> nodes;
  enumerate_topology(f->n, f->L, f->min_leaf, nodes);
  int64_t smax = 0;
  for (const Node& nd : nodes)
    if (nd.leaf) smax = std::max(smax, nd.n);
  const bool general = ctx->opt.graph_general != 0 || smax > kLeafMax;
  std::vector<GBlock> blocks;
  int64_t pairs = 0;
  for (const Node& nd : nodes) {
    if (!nd.leaf || nd.n < 2) continue;
    RPT_ARG(nd.n <= 0x7fffffff, "leaf too large");
    if (general) {
      for (int64_t r0 = 0; r0 < nd.n; r0 += kTB) blocks.push_back({nd.off, (int32_t)nd.n, (int32_t)r0});
      pairs += nd.n * (nd.n - 1);      // every ordered pair
    } else {
      blocks.push_back({nd.off, (int32_t)nd.n, 0});
      pairs += nd.n * (nd.n - 1) / 2;  // every pair once
    }
  }
  RPT_ARG(blocks.size() <= 0x7fffffffu, "too many leaf blocks for one launch");
  if (!(flags & RPT_GRAPH_ACCUMULATE)) {
    const int64_t want = (f->n * k + 255) / 256;
    const unsigned grid = (unsigned)std::min<int64_t>(want, (int64_t)ctx->n_cu * 16);
    hipLaunchKernelGGL(graph_csr_init_kernel, dim3(grid), dim3(256), 0, ctx->stream, f->n, k, ids_dev,
                       dist_dev, count_dev);
    RPT_HIP(hipGetLastError());
  }
  ctx->last_graph_pairs = pairs * f->T;
  if (blocks.empty()) return RPT_OK;
  DevBuf<GBlock> bdev;
  RPT_TRY(bdev.alloc(blocks.size()));
  RPT_TRY(upload_async(ctx, bdev.p, blocks.data(), blocks.size() * sizeof(GBlock)));
  ProfScope ps(ctx, RPT_PROF_KNN_TOPK);
  const int64_t nb = (int64_t)blocks.size();
  if (data->dtype == RPT_F64)
    return launch_graph_csr_metric<double>(m, ctx, f, data, k, general, (int)smax, bdev.p, nb, ids_dev, dist_dev, count_dev);
  return launch_graph_csr_metric<float>(m, ctx, f, data, k, general, (int)smax, bdev.p, nb, ids_dev, dist_dev, count_dev);
}

int32_t knn_graph_refine_csr_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse,
                                 int32_t iters, int32_t metric, int32_t* ids_dev, double* dist_dev,
                                 int32_t* count_dev) {
  const int m = graph_metric_of(metric);
  if (m == kGraphCosine) RPT_TRY(ensure_sqnorm(ctx, data));  // the join needs no mask, so no statistics
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
  const int wave_bytes = (int)(((size_t)kPiece * 12 + (size_t)(H + k + r) * 4 + 7) & ~(size_t)7);
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
      if (data->dtype == RPT_F64)
        RPT_TRY(launch_join_csr_metric<double>(m, ctx, st, data, k, r, H, wave_bytes, W, ids_dev, dist_dev,
                                               count_dev, roff.p, rsrc.p, rdist.p, sids.p, sdist.p, scount.p));
      else
        RPT_TRY(launch_join_csr_metric<float>(m, ctx, st, data, k, r, H, wave_bytes, W, ids_dev, dist_dev,
                                              count_dev, roff.p, rsrc.p, rdist.p, sids.p, sdist.p, scount.p));
      hipLaunchKernelGGL(refine_copy_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, st, n, k, sids.p,
                         sdist.p, scount.p, ids_dev, dist_dev, count_dev);
    }
    hipLaunchKernelGGL(refine_end_kernel, dim3(1), dim3(64), 0, ctx->stream, st);
    RPT_HIP(hipGetLastError());
  }
  return RPT_OK;
}

}  // namespace rpt
