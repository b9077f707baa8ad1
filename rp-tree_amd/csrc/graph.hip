// graph.hip — kNN graph of the indexed points, built leaf by leaf (rpt_knn_graph_*).
//
// knn (RPTree.hs:174-176) with every stored point as the query ranks, per tree, the points of
// the leaf the query falls into.  All points of a leaf have the same leaf mates, so the leaf's
// rows are read ONCE per tree and every pair of the leaf is evaluated once, instead of one
// candidate gather per point.  The distance is metricDDL2 (Internal.hs:403-406) as a left fold in
// double for every dtype: acc = acc + (a - b) * (a - b), columns ascending, no FMA (the
// translation unit is built with -ffp-contract=off), then one correctly rounded sqrt.  The fold
// is symmetric bit for bit, so dist(i, j) serves both rows.
//
// One launch per tree, the trees in stream order.  Within a tree a point lies in exactly one
// leaf, so exactly one workgroup (leaf kernel) or one workgroup per 64-row block (tiled kernel)
// owns point i's running list [k] in global memory: no atomics, no races, one result.
//   graph_leaf_kernel   leaves of up to 128 points: one workgroup per leaf; the pair accumulators
//                       of the leaf's upper triangle live in registers (4 x 4 pairs per tile, up
//                       to three tiles per lane), the rows pass through LDS in chunks of 32
//                       columns (row stride 33 doubles: column reads are conflict-free), the
//                       distances go to an LDS matrix and one wave per row merges them into the
//                       row's list.
//   graph_tiled_kernel  any leaf: a workgroup owns 64 rows of a leaf and meets the leaf's points
//                       in blocks of 64, one 4 x 4 tile per lane, the same chunks and the same
//                       fold (the accumulators carry over the chunks), the lists of its rows in
//                       LDS until the end.  It evaluates every ordered pair: twice the work.
// The selection is an insertion into a sorted list held one entry per lane: candidates not
// before the list's last entry are dropped by a ballot, the others are inserted one at a time,
// an id that the list already holds (the same point found by an earlier tree) is skipped.
#include <string.h>

#include <algorithm>

#include "graph_dev.h"

namespace rpt {
namespace {

constexpr int kLeafMax = 128;   // largest leaf of graph_leaf_kernel
constexpr int kTB = 64;         // rows / columns of a block of graph_tiled_kernel
constexpr int kThreads = 256;

// one workgroup's share of a tree: rows [row0, row0 + 64) (tiled) or all rows (leaf kernel) of
// the leaf perm[t][off .. off + n)
struct GBlock {
  int64_t off;
  int32_t n;
  int32_t row0;
};

// columns [c0, c0 + cw) of the rows sid[0 .. nrows) (id < 0: no row, the slot keeps what it held
// and nothing reads its results) as doubles into buf[r * kLS + c].  vec: rows are 16-byte
// granular (base and pitch), so a row's chunk is whole 16-byte pieces.
template <class TD>
__device__ inline void stage_chunk(const TD* __restrict__ X, int d, const int* sid, int nrows,
                                   int c0, int cw, double* buf, bool vec) {
  if (vec) {
    constexpr int E = 16 / (int)sizeof(TD);
    const int ppr = cw / E;
    for (int p = threadIdx.x; p < nrows * ppr; p += kThreads) {
      const int r = p / ppr, q = p - r * ppr;
      const int id = sid[r];
      if (id < 0) continue;
      const uint4 v = *reinterpret_cast<const uint4*>(X + (size_t)id * d + c0 + q * E);
      double w[E];
      widen16<TD>(v, w);
#pragma unroll
      for (int e = 0; e < E; ++e) buf[r * kLS + q * E + e] = w[e];
    }
  } else {
    for (int p = threadIdx.x; p < nrows * cw; p += kThreads) {
      const int r = p / cw, c = p - r * cw;
      const int id = sid[r];
      if (id < 0) continue;
      buf[r * kLS + c] = widen(X[(size_t)id * d + c0 + c]);
    }
  }
}

// 4 x 4 pairs over cw columns: rows ra + u * sa of bufA against rows rb + v * sb of bufB.  The
// reference's fold: every difference, square and sum (L2) / every product and sum (the dot of the
// cosine and inner-product distances) rounded on its own.
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

__global__ void graph_init_kernel(int64_t n, int k, int32_t* __restrict__ ids,
                                  double* __restrict__ dist, int32_t* __restrict__ count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * k; i += stride) {
    ids[i] = -1;
    dist[i] = pos_inf();
    if (i < n) count[i] = 0;
  }
}

// ---- leaves of up to 128 points: one workgroup per leaf, every pair once ----------------------
// dynamic LDS: lds_doubles doubles, then 4 ng ints (the leaf's ids); ng = ceil(largest leaf / 4).
// lds_doubles = max(4 ng (4 ng + 1), 4 ng * kLS) (the chunk, later the distance matrix), for the
// cosine distance 4 ng more: the rows' norms rn[id] at the END of the doubles (behind the matrix of
// the largest leaf, so of every leaf).
template <class TD, int M>
__global__ __launch_bounds__(kThreads) void graph_leaf_kernel(
    const TD* __restrict__ X, int d, const int32_t* __restrict__ perm_t,
    const GBlock* __restrict__ blocks, int k, int lds_doubles, int vec, int32_t* __restrict__ ids,
    double* __restrict__ dist, int32_t* __restrict__ count, const double* __restrict__ rn) {
  extern __shared__ double smem[];
  double* buf = smem;
  int* sid = reinterpret_cast<int*>(smem + lds_doubles);
  const GBlock blk = blocks[blockIdx.x];
  const int s = blk.n;
  if (s < 2) return;  // no mates in this tree
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ng = (s + 3) >> 2;  // row groups: group g holds the rows g, g + ng, g + 2 ng, g + 3 ng
  const int P = 4 * ng;
  [[maybe_unused]] double* snorm = smem + lds_doubles - P;
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

  for (int c0 = 0; c0 < d; c0 += kCW) {
    const int cw = d - c0 < kCW ? d - c0 : kCW;
    __syncthreads();  // the ids are there / the last chunk has been read
    stage_chunk<TD>(X, d, sid, P, c0, cw, buf, vec != 0);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 3; ++u)
      if (gi[u] >= 0) tile_fold<M>(buf, gi[u], ng, buf, gj[u], ng, cw, acc[u]);
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
// dynamic LDS: 2 * 64 * kLS doubles (two chunks, later the 64 x 65 distance block), 64 k doubles
// (the rows' lists), for the cosine distance 64 + 64 doubles (the norms of the rows and of the
// block's points), then ints: 64 k list ids, 64 counts, 64 changed flags, 64 + 64 row ids
template <class TD, int M>
__global__ __launch_bounds__(kThreads) void graph_tiled_kernel(
    const TD* __restrict__ X, int d, const int32_t* __restrict__ perm_t,
    const GBlock* __restrict__ blocks, int k, int vec, int32_t* __restrict__ ids,
    double* __restrict__ dist, int32_t* __restrict__ count, const double* __restrict__ rn) {
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
  const GBlock blk = blocks[blockIdx.x];
  const int s = blk.n;
  if (s < 2) return;
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

  for (int cb = 0; cb < s; cb += kTB) {
    const int nc = s - cb < kTB ? s - cb : kTB;
    __syncthreads();  // the last block's selection is over
    if (tid < kTB) {
      const int g = tid < nc ? perm_t[blk.off + cb + tid] : -1;
      sidB[tid] = g;
      if constexpr (M == kGraphCosine) nrmB[tid] = g >= 0 ? rn[g] : 0.0;
    }
    double acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
    for (int c0 = 0; c0 < d; c0 += kCW) {
      const int cw = d - c0 < kCW ? d - c0 : kCW;
      __syncthreads();
      stage_chunk<TD>(X, d, sidA, kTB, c0, cw, bufA, vec != 0);
      stage_chunk<TD>(X, d, sidB, kTB, c0, cw, bufB, vec != 0);
      __syncthreads();
      tile_fold<M>(bufA, gi, 16, bufB, gj, 16, cw, acc);
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

template <class TD, int M>
int32_t launch_graph(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k, bool general,
                     int smax, const GBlock* blocks_dev, int64_t nblocks, int32_t* ids, double* dist,
                     int32_t* count) {
  const TD* X = static_cast<const TD*>(data->X);
  const double* rn = M == kGraphCosine ? data->sqnorm : nullptr;
  const int d = data->d;
  // 16-byte pieces need a 16-byte base and pitch
  const int vec = ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && ((size_t)d * sizeof(TD)) % 16 == 0) ? 1 : 0;
  constexpr int kLdsMax = 160 * 1024;
  static DeviceOnce attr_once[2];
  if (!general) {
    const int ng = (smax + 3) / 4, P = 4 * ng;
    const int lds_doubles = std::max(P * (P + 1), P * kLS) + (M == kGraphCosine ? P : 0);
    const size_t smem = (size_t)lds_doubles * 8 + (size_t)P * 4;
    RPT_TRY(attr_once[0].run(ctx->device, [&]() -> int32_t {
      RPT_HIP(hipFuncSetAttribute((const void*)graph_leaf_kernel<TD, M>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
      return RPT_OK;
    }));
    for (int32_t t = 0; t < f->T; ++t)
      hipLaunchKernelGGL((graph_leaf_kernel<TD, M>), dim3((unsigned)nblocks), dim3(kThreads), smem,
                         ctx->stream, X, d, f->perm.p + (int64_t)t * f->n, blocks_dev, k,
                         lds_doubles, vec, ids, dist, count, rn);
  } else {
    const size_t smem = (size_t)(2 * kTB * kLS + kTB * k + (M == kGraphCosine ? 2 * kTB : 0)) * 8 +
                        (size_t)(kTB * k + 4 * kTB) * 4;
    RPT_TRY(attr_once[1].run(ctx->device, [&]() -> int32_t {
      RPT_HIP(hipFuncSetAttribute((const void*)graph_tiled_kernel<TD, M>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
      return RPT_OK;
    }));
    for (int32_t t = 0; t < f->T; ++t)
      hipLaunchKernelGGL((graph_tiled_kernel<TD, M>), dim3((unsigned)nblocks), dim3(kThreads), smem,
                         ctx->stream, X, d, f->perm.p + (int64_t)t * f->n, blocks_dev, k, vec, ids,
                         dist, count, rn);
  }
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

template <class TD>
int32_t launch_graph_metric(int m, rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                            bool general, int smax, const GBlock* blocks_dev, int64_t nblocks,
                            int32_t* ids, double* dist, int32_t* count) {
  if (m == kGraphCosine)
    return launch_graph<TD, kGraphCosine>(ctx, f, data, k, general, smax, blocks_dev, nblocks, ids, dist, count);
  if (m == kGraphInner)
    return launch_graph<TD, kGraphInner>(ctx, f, data, k, general, smax, blocks_dev, nblocks, ids, dist, count);
  return launch_graph<TD, kGraphL2>(ctx, f, data, k, general, smax, blocks_dev, nblocks, ids, dist, count);
}

}  // namespace

int32_t knn_graph_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                      int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                      int32_t* count_dev) {
  ctx->last_graph_pairs = 0;
  if (f->n == 0) return RPT_OK;
  const int m = graph_metric_of(metric);
  if (m == kGraphCosine) RPT_TRY(ensure_sqnorm(ctx, data));  // the rows' dot(x, x), cached on the dataset
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
    hipLaunchKernelGGL(graph_init_kernel, dim3(grid), dim3(256), 0, ctx->stream, f->n, k, ids_dev,
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
  switch (data->dtype) {
    case RPT_F64:
      return launch_graph_metric<double>(m, ctx, f, data, k, general, (int)smax, bdev.p, nb, ids_dev, dist_dev, count_dev);
    case RPT_F32:
      return launch_graph_metric<float>(m, ctx, f, data, k, general, (int)smax, bdev.p, nb, ids_dev, dist_dev, count_dev);
    default:
      return launch_graph_metric<uint16_t>(m, ctx, f, data, k, general, (int)smax, bdev.p, nb, ids_dev, dist_dev, count_dev);
  }
}

}  // namespace rpt
