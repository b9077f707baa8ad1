// graph_delete.hip — rows out of a kNN graph (rpt_graph_delete_*).
//
// The answer is the definition of include/rptree_hip.h: the deleted rows are dropped, every kept row
// that named one (a TOUCHED row) is repaired from the deleted rows' own neighbours, one hop, and with
// RPT_GRAPH_DELETE_COMPACT the survivors are renumbered densely.  The caller's graph is read only.
//
// Kernels, in stream order:
//   delete_mark_kernel    one WAVE per row, an entry per lane: flag[p] = 0 (deleted), 1 (kept, names no
//                         deleted row) or 2 (touched); the valid entries that name a deleted row are
//                         counted (one ballot per row)
//   delete_scan_kernel    one workgroup, a contiguous run of rows per thread (rev_scan_kernel's shape):
//                         the exclusive scans of "kept" and of "touched" -> newid[] and the touched list
//   delete_copy_kernel    a slot per thread: untouched rows slot for slot with their ids mapped through
//                         newid, deleted rows emptied (without COMPACT) or skipped (with it)
//   delete_repair_kernel  (dense rows) / delete_repair_csr_kernel (CSR rows), templates on (TD or TV, M)
//                         like refine_join_kernel / refine_join_csr_kernel, whose helpers they reuse:
//                         one WAVE owns a touched row p.  Its kept valid entries K(p) enter a sorted
//                         list held one entry per lane (wave_merge) with their STORED distances; p and
//                         K(p) enter the LDS hash set marked old; the kept valid ids of the rows of D(p)
//                         enter as new; the new members are compacted in place, their distances to p
//                         evaluated in blocks of 64 (a candidate per lane; dense rows staged through LDS
//                         in chunks of kCW columns, CSR rows by the two-pointer merge against x_p passing
//                         through LDS in pieces), merged into the list, and the row is written with its
//                         ids mapped through newid.  Four rows per workgroup while four waves' LDS shares
//                         fit 160 KB, else (and with the option graph_delete_general) one.
// The slots of the hash set depend on the order of arrival; the row is the first kg of a set under a
// total order and every distance is a function of its pair, so the answer does not.  No atomics touch a
// row; the counters are sums.  Scratch: flag[n], the touched list [n] and, when the caller passes no
// newid, newid[n]: 8 n or 12 n bytes.
#include <algorithm>
#include <type_traits>

#include "graph_refine_dev.h"

namespace rpt {
namespace {

constexpr int kLdsMax = 160 * 1024;
constexpr int kNoCol = 0x7fffffff;  // a cursor at its row's end
constexpr int kPiece = 64;          // (column, value) pairs of x_p per LDS piece

struct DeleteState {
  unsigned long long kept, touched, evaluated, dropped;
};

__global__ void delete_begin_kernel(DeleteState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->kept = 0;
    st->touched = 0;
    st->evaluated = 0;
    st->dropped = 0;
  }
}

// whether id v (in [0, n)) stays: bit v & 31 of word v >> 5; a null bitmap keeps every row
__device__ inline bool kept_id(const uint32_t* keep, int v) {
  return keep == nullptr || ((keep[v >> 5] >> (v & 31)) & 1u) != 0;
}

// Row j of the graph, an entry per lane: lid / ld are the lane's slot (id -1 at or beyond the clamped
// count).  Returns whether the lane's entry is VALID: inside the count, id in [0, n), not j itself,
// and the first slot of the row that holds this id.  All 64 lanes call it together.
__device__ inline bool load_row(int64_t j, int64_t n, int kg, const int32_t* ids, const double* dist,
                                const int32_t* count, int lane, int& lid, double& ld) {
  int c = count[j];
  c = c < 0 ? 0 : (c > kg ? kg : c);
  lid = -1;
  ld = pos_inf();
  if (lane < c) {
    lid = ids[j * kg + lane];
    if (dist) ld = dist[j * kg + lane];
  }
  bool ok = lane < c && (unsigned)lid < (unsigned long long)n && lid != (int)j;
  for (int e = 0; e + 1 < c; ++e) {  // an id twice: the later slot does not count
    const int ev = __shfl(lid, e);
    if (e < lane && ev == lid) ok = false;
  }
  return ok;
}

__global__ __launch_bounds__(256) void delete_mark_kernel(DeleteState* st, int64_t n, int kg,
                                                          const int32_t* __restrict__ ids,
                                                          const int32_t* __restrict__ count,
                                                          const uint32_t* __restrict__ keep,
                                                          int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  unsigned long long n_drop = 0;
  for (int64_t p = (int64_t)blockIdx.x * W + wave; p < n; p += (int64_t)gridDim.x * W) {
    if (!kept_id(keep, (int)p)) {
      if (lane == 0) flag[p] = 0;
      continue;
    }
    int lid;
    double ld;
    const bool ok = load_row(p, n, kg, ids, nullptr, count, lane, lid, ld);
    const int gone = __popcll(__ballot(ok && !kept_id(keep, lid)));
    if (lane == 0) flag[p] = gone ? 2 : 1;
    n_drop += (unsigned long long)gone;
  }
  if (lane == 0 && n_drop) atomicAdd(&st->dropped, n_drop);
}

// newid[i] = -1 (deleted), the number of kept rows below i (compact) or i; list[0 .. touched) = the
// touched rows, ascending
__global__ __launch_bounds__(kScanThreads) void delete_scan_kernel(DeleteState* st, int64_t n, int compact,
                                                                   const int32_t* __restrict__ flag,
                                                                   int32_t* __restrict__ newid,
                                                                   int32_t* __restrict__ list) {
  __shared__ int64_t part_k[kScanThreads];
  __shared__ int64_t part_t[kScanThreads];
  const int tid = threadIdx.x;
  const int64_t per = (n + kScanThreads - 1) / kScanThreads;
  const int64_t lo = std::min<int64_t>(n, per * tid), hi = std::min<int64_t>(n, lo + per);
  int64_t sk = 0, stc = 0;
  for (int64_t i = lo; i < hi; ++i) {
    const int f = flag[i];
    sk += f != 0;
    stc += f == 2;
  }
  part_k[tid] = sk;
  part_t[tid] = stc;
  __syncthreads();
  for (int step = 1; step < kScanThreads; step <<= 1) {  // inclusive scans of the partial sums
    const int64_t ak = tid >= step ? part_k[tid - step] : 0;
    const int64_t at = tid >= step ? part_t[tid - step] : 0;
    __syncthreads();
    part_k[tid] += ak;
    part_t[tid] += at;
    __syncthreads();
  }
  int64_t rk = part_k[tid] - sk, rt = part_t[tid] - stc;
  for (int64_t i = lo; i < hi; ++i) {
    const int f = flag[i];
    newid[i] = f == 0 ? -1 : (int32_t)(compact ? rk : i);
    if (f == 2) list[rt++] = (int32_t)i;
    rk += f != 0;
  }
  if (tid == kScanThreads - 1) {
    st->kept = (unsigned long long)part_k[tid];
    st->touched = (unsigned long long)part_t[tid];
  }
}

__global__ __launch_bounds__(256) void delete_copy_kernel(int64_t n, int kg, int compact,
                                                          const int32_t* __restrict__ ids,
                                                          const unsigned long long* __restrict__ dist,
                                                          const int32_t* __restrict__ count,
                                                          const int32_t* __restrict__ flag,
                                                          const int32_t* __restrict__ newid,
                                                          int32_t* __restrict__ oids,
                                                          unsigned long long* __restrict__ odist,
                                                          int32_t* __restrict__ ocount) {
  const int64_t total = n * kg, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const int64_t p = e / kg;
    const int s = (int)(e - p * kg);
    const int f = flag[p];
    if (f == 2) continue;  // the repair writes it
    if (f == 0) {
      if (!compact) {
        oids[e] = -1;
        odist[e] = 0x7ff0000000000000ULL;
        if (s == 0) ocount[p] = 0;
      }
      continue;
    }
    const int64_t o = newid[p];
    const int id = ids[e];
    oids[o * kg + s] = (unsigned)id < (unsigned long long)n ? newid[id] : id;
    odist[o * kg + s] = dist[e];  // the bits
    if (s == 0) ocount[o] = count[p];
  }
}

// What the two repair kernels share in front of their distances: row p into the sorted list (ld, lid,
// c) of its kept valid entries, the hash set filled, its new members compacted to tab[0 .. m).  bl:
// kg ints.  Returns m = |C(p)|.
__device__ inline int repair_gather(int64_t p, int64_t n, int kg, int H, const int32_t* ids, const double* dist,
                                    const int32_t* count, const uint32_t* keep, int* tab, int* bl, int lane,
                                    double& ld, int& lid, int& c) {
  const int mask = H - 1, shift = 32 - (31 - __clz(H));
  const unsigned long long below = (1ULL << lane) - 1;
  int rid;
  double rd;
  const bool ok = load_row(p, n, kg, ids, dist, count, lane, rid, rd);
  const bool stays = ok && kept_id(keep, rid);
  const bool gone = ok && !stays;
  ld = pos_inf();
  lid = -1;
  c = 0;
  wave_merge(ld, lid, c, kg, rd, rid, stays, 0.0, -1, false);  // K(p), sorted

  for (int q = lane; q < H; q += 64) tab[q] = kEmpty;
  const unsigned long long gm = __ballot(gone);
  const int nd = __popcll(gm);
  if (gone) bl[__popcll(gm & below)] = rid;  // D(p)
  wave_sync();
  if (lane == 0) set_insert(tab, mask, shift, (int)p, ~(int)p);
  if (stays) set_insert(tab, mask, shift, rid, ~rid);
  wave_sync();
  for (int q = lane; q < nd * kg; q += 64) {
    const int b = q / kg, e = q - b * kg;
    const int v = bl[b];
    if (e >= count[v]) continue;
    const int cnd = ids[(int64_t)v * kg + e];
    if ((unsigned)cnd < (unsigned long long)n && cnd != v && kept_id(keep, cnd))
      set_insert(tab, mask, shift, cnd, cnd);
  }
  wave_sync();

  // the new members, compacted to tab[0 .. m): a slot is read before anything is written at or
  // behind it (m <= base)
  int m = 0;
  for (int base = 0; base < H; base += 64) {
    const int v = tab[base + lane];
    const unsigned long long bal = __ballot(v >= 0);
    wave_sync();
    if (v >= 0) tab[m + __popcll(bal & below)] = v;
    m += __popcll(bal);
  }
  wave_sync();
  return m;
}

// row p of the answer: sorted, ids through newid, unused slots id -1 and distance +inf
__device__ inline void repair_write(int64_t p, int kg, const int32_t* newid, int lane, double ld, int lid,
                                    int c, int32_t* oids, double* odist, int32_t* ocount) {
  const int64_t o = newid[p];
  if (lane < kg) {
    odist[o * kg + lane] = lane < c ? ld : pos_inf();
    oids[o * kg + lane] = lane < c ? newid[lid] : -1;
  }
  if (lane == 0) ocount[o] = c;
}

// dynamic LDS, per wave (wave_bytes): 64 * kLS doubles (a block of 64 candidates' rows), kCW doubles
// (the chunk of x_p), H ints (the hash set, later the candidates), kg ints (D(p)).  rn: the rows'
// dot(x, x) (cosine only).
template <class TD, int M>
__global__ __launch_bounds__(256) void delete_repair_kernel(
    DeleteState* st, const TD* __restrict__ X, int64_t n, int d, int kg, int vec, int H, int wave_bytes,
    const int32_t* __restrict__ ids, const double* __restrict__ dist, const int32_t* __restrict__ count,
    const uint32_t* __restrict__ keep, const int32_t* __restrict__ list, const int32_t* __restrict__ newid,
    int32_t* __restrict__ oids, double* __restrict__ odist, int32_t* __restrict__ ocount,
    const double* __restrict__ rn) {
  extern __shared__ double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  double* buf = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * wave_bytes);
  double* xp = buf + 64 * kLS;
  int* tab = reinterpret_cast<int*>(xp + kCW);
  int* bl = tab + H;
  const int64_t nt = (int64_t)st->touched;
  unsigned long long n_eval = 0;

  for (int64_t t = (int64_t)blockIdx.x * W + wave; t < nt; t += (int64_t)gridDim.x * W) {
    const int64_t p = list[t];
    double ld;
    int lid, c;
    const int m = repair_gather(p, n, kg, H, ids, dist, count, keep, tab, bl, lane, ld, lid, c);
    n_eval += (unsigned long long)m;
    double np = 0.0;
    if constexpr (M == kGraphCosine) np = rn[p];

    for (int b0 = 0; b0 < m; b0 += 64) {
      const int nrows = m - b0 < 64 ? m - b0 : 64;
      const int my = lane < nrows ? tab[b0 + lane] : -1;
      double acc = 0.0;
      for (int c0 = 0; c0 < d; c0 += kCW) {
        const int cw = d - c0 < kCW ? d - c0 : kCW;
        wave_sync();  // the last chunk has been read
        wave_stage<TD>(X, d, tab + b0, nrows, c0, cw, buf, vec != 0);
        if (lane < cw) xp[lane] = widen(X[(size_t)p * d + c0 + lane]);
        wave_sync();
        if (lane < nrows) {
          const double* row = buf + lane * kLS;
#pragma unroll 4
          for (int cc = 0; cc < cw; ++cc) acc = fold_step<M>(acc, xp[cc], row[cc]);
        }
      }
      double nj = 0.0;
      if constexpr (M == kGraphCosine) nj = lane < nrows ? rn[my] : 0.0;
      wave_merge(ld, lid, c, kg, fold_finish<M>(acc, np, nj), my, lane < nrows, 0.0, -1, false);
    }
    repair_write(p, kg, newid, lane, ld, lid, c, oids, odist, ocount);
    wave_sync();  // tab and bl are the next row's
  }
  if (lane == 0 && n_eval) atomicAdd(&st->evaluated, n_eval);
}

// dynamic LDS, per wave (wave_bytes): kPiece doubles and kPiece ints (a piece of x_p's values and
// columns), H ints, kg ints.  rn: the rows' dotS(x, x) (cosine only).
template <class TV, int M>
__global__ __launch_bounds__(256) void delete_repair_csr_kernel(
    DeleteState* st, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const TV* __restrict__ val, int64_t n, int kg, int H, int wave_bytes, const int32_t* __restrict__ ids,
    const double* __restrict__ dist, const int32_t* __restrict__ count, const uint32_t* __restrict__ keep,
    const int32_t* __restrict__ list, const int32_t* __restrict__ newid, int32_t* __restrict__ oids,
    double* __restrict__ odist, int32_t* __restrict__ ocount, const double* __restrict__ rn) {
  extern __shared__ double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  double* pv = reinterpret_cast<double*>(reinterpret_cast<char*>(smem) + (size_t)wave * wave_bytes);
  int* pc = reinterpret_cast<int*>(pv + kPiece);
  int* tab = pc + kPiece;
  int* bl = tab + H;
  const int64_t nt = (int64_t)st->touched;
  unsigned long long n_eval = 0;

  for (int64_t t = (int64_t)blockIdx.x * W + wave; t < nt; t += (int64_t)gridDim.x * W) {
    const int64_t p = list[t];
    double ld;
    int lid, c;
    const int m = repair_gather(p, n, kg, H, ids, dist, count, keep, tab, bl, lane, ld, lid, c);
    n_eval += (unsigned long long)m;
    const int64_t ib = rowptr[p], ie = rowptr[p + 1];
    [[maybe_unused]] double np = 0.0;
    if constexpr (M == kGraphCosine) np = rn[p];

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
        const int npc = ie - p0 < kPiece ? (int)(ie - p0) : kPiece;
        wave_sync();  // the last piece has been read
        if (lane < npc) {
          pc[lane] = col[p0 + lane];
          pv[lane] = widen(val[p0 + lane]);
        }
        wave_sync();
        if (my >= 0) {
          int ii = 0;
          while (ii < npc) {  // every step takes an entry of x_p or of the candidate
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
        while (jp < je) {  // what the candidate holds behind x_p's last column
          acc = fold_step<kGraphL2>(acc, 0.0, vj);
          ++jp;
          if (jp < je) vj = widen(val[jp]);
        }
      }
      double dv;
      if constexpr (M == kGraphL2) dv = fold_finish<kGraphL2>(acc, 0.0, 0.0);
      else if constexpr (M == kGraphCosine) dv = fold_finish<M>(acc, np, my >= 0 ? rn[my] : 0.0);
      else dv = fold_finish<M>(acc, 0.0, 0.0);
      wave_merge(ld, lid, c, kg, dv, my, lane < nrows, 0.0, -1, false);
    }
    repair_write(p, kg, newid, lane, ld, lid, c, oids, odist, ocount);
    wave_sync();  // tab and bl are the next row's
  }
  if (lane == 0 && n_eval) atomicAdd(&st->evaluated, n_eval);
}

struct RepairArgs {
  DeleteState* st;
  int kg, H, wave_bytes, W;
  const int32_t* ids;
  const double* dist;
  const int32_t* count;
  const uint32_t* keep;
  const int32_t* list;
  const int32_t* newid;
  int32_t* oids;
  double* odist;
  int32_t* ocount;
};

inline unsigned repair_grid(rpt_ctx* ctx, int64_t n, int W) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + W - 1) / W, (int64_t)ctx->n_cu * 16));
}

template <class TD, int M>
int32_t launch_repair(rpt_ctx* ctx, const rpt_dataset* data, const RepairArgs& a) {
  const TD* X = static_cast<const TD*>(data->X);
  const int d = data->d;
  const int vec = ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && ((size_t)d * sizeof(TD)) % 16 == 0) ? 1 : 0;
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)delete_repair_kernel<TD, M>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  hipLaunchKernelGGL((delete_repair_kernel<TD, M>), dim3(repair_grid(ctx, data->n, a.W)), dim3(64 * a.W),
                     (size_t)a.wave_bytes * a.W, ctx->stream, a.st, X, data->n, d, a.kg, vec, a.H, a.wave_bytes,
                     a.ids, a.dist, a.count, a.keep, a.list, a.newid, a.oids, a.odist, a.ocount,
                     M == kGraphCosine ? data->sqnorm : nullptr);
  return RPT_OK;
}

template <class TV, int M>
int32_t launch_repair_csr(rpt_ctx* ctx, const rpt_dataset* data, const RepairArgs& a) {
  static DeviceOnce attr_once;
  RPT_TRY(attr_once.run(ctx->device, [&]() -> int32_t {
    RPT_HIP(hipFuncSetAttribute((const void*)delete_repair_csr_kernel<TV, M>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax));
    return RPT_OK;
  }));
  hipLaunchKernelGGL((delete_repair_csr_kernel<TV, M>), dim3(repair_grid(ctx, data->n, a.W)), dim3(64 * a.W),
                     (size_t)a.wave_bytes * a.W, ctx->stream, a.st, data->rowptr, data->col,
                     static_cast<const TV*>(data->val), data->n, a.kg, a.H, a.wave_bytes, a.ids, a.dist, a.count,
                     a.keep, a.list, a.newid, a.oids, a.odist, a.ocount,
                     M == kGraphCosine ? data->sqnorm : nullptr);
  return RPT_OK;
}

template <class T>
int32_t launch_repair_metric(int m, bool csr, rpt_ctx* ctx, const rpt_dataset* data, const RepairArgs& a) {
  if constexpr (!std::is_same<T, uint16_t>::value) {
    if (csr) {
      if (m == kGraphCosine) return launch_repair_csr<T, kGraphCosine>(ctx, data, a);
      if (m == kGraphInner) return launch_repair_csr<T, kGraphInner>(ctx, data, a);
      return launch_repair_csr<T, kGraphL2>(ctx, data, a);
    }
  }
  if (m == kGraphCosine) return launch_repair<T, kGraphCosine>(ctx, data, a);
  if (m == kGraphInner) return launch_repair<T, kGraphInner>(ctx, data, a);
  return launch_repair<T, kGraphL2>(ctx, data, a);
}

}  // namespace

int32_t graph_delete_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_dev,
                         const double* gdist_dev, const int32_t* gcount_dev, const uint32_t* keep_dev,
                         int32_t metric, int32_t flags, int32_t* oids_dev, double* odist_dev,
                         int32_t* ocount_dev, int32_t* newid_dev) {
  const int64_t n = data->n;
  const int mt = graph_metric_of(metric);
  const int compact = (flags & RPT_GRAPH_DELETE_COMPACT) ? 1 : 0;
  if (mt == kGraphCosine && n > 0) RPT_TRY(ensure_sqnorm(ctx, data));  // the rows' dot(x, x), cached on the dataset
  if (!ctx->delete_state_dev) {
    hipError_t e = dev_alloc(&ctx->delete_state_dev, sizeof(DeleteState));
    if (e != hipSuccess)
      return fail(RPT_E_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  }
  DeleteState* st = static_cast<DeleteState*>(ctx->delete_state_dev);

  // the plan: the hash set holds at most 1 + kg + kg^2 ids; half as many slots again keep the probes short
  const int64_t raw = 1 + (int64_t)kg + (int64_t)kg * kg;
  int H = 64;
  while (H < raw + raw / 2) H <<= 1;
  const size_t stage = data->csr ? (size_t)kPiece * 12 : (size_t)(64 * kLS + kCW) * 8;
  const int wave_bytes = (int)((stage + (size_t)(H + kg) * 4 + 7) & ~(size_t)7);
  const int W = (ctx->opt.graph_delete_general == 0 && 4 * wave_bytes <= kLdsMax) ? 4 : 1;
  if (wave_bytes > kLdsMax) return fail(RPT_E_INTERNAL, "delete: the candidate set does not fit LDS");

  DevBuf<int32_t> flag, list, nid;
  if (n > 0) {
    RPT_TRY(flag.alloc((size_t)n));
    RPT_TRY(list.alloc((size_t)n));
    if (!newid_dev) {
      RPT_TRY(nid.alloc((size_t)n));
      newid_dev = nid.p;
    }
  }

  ProfScope ps(ctx, RPT_PROF_GRAPH_DELETE);
  hipLaunchKernelGGL(delete_begin_kernel, dim3(1), dim3(64), 0, ctx->stream, st);
  if (n > 0) {
    const int64_t cap = (int64_t)ctx->n_cu * 16;
    const unsigned grid_r = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, cap));
    const unsigned grid_e = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n * kg + 255) / 256, cap));
    hipLaunchKernelGGL(delete_mark_kernel, dim3(grid_r), dim3(256), 0, ctx->stream, st, n, kg, gids_dev,
                       gcount_dev, keep_dev, flag.p);
    hipLaunchKernelGGL(delete_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, st, n, compact, flag.p,
                       newid_dev, list.p);
    hipLaunchKernelGGL(delete_copy_kernel, dim3(grid_e), dim3(256), 0, ctx->stream, n, kg, compact, gids_dev,
                       reinterpret_cast<const unsigned long long*>(gdist_dev), gcount_dev, flag.p, newid_dev,
                       oids_dev, reinterpret_cast<unsigned long long*>(odist_dev), ocount_dev);
    if (keep_dev) {  // without a bitmap no row is touched
      const RepairArgs a{st, kg, H, wave_bytes, W, gids_dev, gdist_dev, gcount_dev, keep_dev, list.p, newid_dev,
                         oids_dev, odist_dev, ocount_dev};
      const bool csr = data->csr;
      if (data->dtype == RPT_F64) RPT_TRY(launch_repair_metric<double>(mt, csr, ctx, data, a));
      else if (data->dtype == RPT_F32) RPT_TRY(launch_repair_metric<float>(mt, csr, ctx, data, a));
      else RPT_TRY(launch_repair_metric<uint16_t>(mt, false, ctx, data, a));
    }
  }
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

int32_t graph_delete_last(rpt_ctx* ctx, int64_t* kept, int64_t* touched, int64_t* evaluated,
                          int64_t* dropped) {
  *kept = *touched = *evaluated = *dropped = 0;
  if (!ctx->delete_state_dev) return RPT_OK;  // no call yet
  RPT_HIP(stream_sync(ctx->stream));
  DeleteState h;
  RPT_HIP(hipMemcpy(&h, ctx->delete_state_dev, sizeof h, hipMemcpyDeviceToHost));
  *kept = (int64_t)h.kept;
  *touched = (int64_t)h.touched;
  *evaluated = (int64_t)h.evaluated;
  *dropped = (int64_t)h.dropped;
  return RPT_OK;
}

}  // namespace rpt
