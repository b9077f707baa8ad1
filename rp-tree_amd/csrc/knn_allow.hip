// knn_allow.hip — an allow-list (a bitmap of n bits: id i = bit i & 31 of word i >> 5) as a list step
// of its own, in front of the general kNN kernels, which rank any list of ids:
//
//   allow_compact_kernel: one workgroup of 256 threads (four waves) per query.  The query's
//     candidate list (its leaf ranges, trees ascending, leaves left to right) is walked 256
//     positions at a time.  A thread finds the range of its position by bisection over the ranges'
//     `pos` (a prefix sum; empty ranges share the `pos` of the range behind them and are never the
//     last with pos <= position), loads perm[poff + i] (neighbouring threads: neighbouring words,
//     except across a range boundary), tests the id's bit, and the kept entries are written in order
//     at kept-so-far + the workgroup prefix: a ballot per wave, four wave totals in LDS.  No atomic
//     cursor: the order is the answer (the duplicate rules rank by position).  The wave totals are
//     double-buffered, so a pass costs one barrier.
//   allow_count_kernel / allow_scan_kernel / allow_scatter_kernel: the bitmap as the ascending list
//     of its ids.  A thread takes a word (the tail word masked at n); a block of 256 words counts
//     its bits; one workgroup scans the block totals, however many; the blocks then scatter: a
//     block-wide exclusive prefix of the popcounts gives every word its first slot, and the thread
//     writes the word's ids by clearing the lowest set bit.
//   allow_ranges_kernel: nq copies of the range {0, total, 0}.
//   One list per group (rpt_brute_knn_allow_group_*: allow_group_count / allow_group_scatter): the count,
//     scan and scatter kernels take the list as a second grid dimension; sel[y] names the bitmap row of
//     list y (-1: every id), the tail mask is applied per row, list y keeps its own nblk + 1 words of
//     block offsets and is written from list_off[y] on.  The host sizes the slab from the lists' lengths.
//
// LDS: a few dozen bytes.  Every output word that is read later is written here: a query's slab
// piece holds `count` ids and its range says so; the words behind them are never read.
#include "knn_allow.h"

#include <algorithm>

#include "common.h"

namespace rpt {
namespace {

__global__ __launch_bounds__(256) void allow_compact_kernel(
    const int32_t* __restrict__ perm, const VoteRange* __restrict__ ranges, const int64_t* __restrict__ rng_off,
    const int64_t* __restrict__ cand_off, int T, int64_t q0, AllowGroups ag,
    int32_t* __restrict__ out_ids, VoteRange* __restrict__ vranges, int64_t* __restrict__ vrng_off,
    int32_t* __restrict__ counts, unsigned long long* __restrict__ allowed_total) {
  __shared__ int s_w[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x, q = q0 + b;
  const int64_t c0 = cand_off[q * T], nc = cand_off[(q + 1) * T] - c0;
  const int64_t ostart = c0 - cand_off[q0 * T];
  const int64_t r0 = rng_off[q * T], r1 = rng_off[(q + 1) * T];
  int32_t* out = out_ids + ostart;
  bool none;  // the query's own bitmap, block-uniform
  const uint32_t* __restrict__ allow = allow_row(ag, q, none);
  int kept = 0;  // block-uniform
  int buf = 0;
  for (int64_t p0 = 0; p0 < nc; p0 += 256, buf ^= 1) {
    const int64_t p = p0 + threadIdx.x;
    bool keep = false;
    int32_t id = 0;
    if (p < nc) {
      int64_t lo = r0, hi = r1;  // the last range with pos <= p (the first range's pos is 0)
      while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)ranges[mid].pos <= p) lo = mid;
        else hi = mid;
      }
      const VoteRange rg = ranges[lo];
      const int64_t i = p - rg.pos;
      if (i < rg.n) {
        id = perm[rg.poff + i];
        keep = !none && (!allow || ((allow[id >> 5] >> (id & 31)) & 1u));
      }
    }
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ULL << lane) - 1ULL));
    if (lane == 0) s_w[buf][wave] = __popcll(m);
    __syncthreads();  // (the next pass writes the other half of s_w; this half is written again only behind
                      // the next pass's barrier, which every thread reaches after the reads below)
    int pre = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
      const int c = s_w[buf][w];
      if (w < wave) pre += c;
      tot += c;
    }
    if (keep) out[kept + pre + before] = id;
    kept += tot;
  }
  if (threadIdx.x == 0) {
    vranges[b] = VoteRange{ostart, kept, 0};
    vrng_off[b] = b;
    if (b == 0) vrng_off[gridDim.x] = gridDim.x;
    counts[b] = kept;
    if (kept) atomicAdd(allowed_total, (unsigned long long)kept);
  }
}

// word w of the bitmap with the bits at positions >= n cleared (null bitmap: every id)
__device__ inline uint32_t allow_word(const uint32_t* __restrict__ allow, int64_t w, int64_t words, int64_t n) {
  if (w >= words) return 0u;
  uint32_t v = allow ? allow[w] : 0xffffffffu;
  const int64_t left = n - w * 32;  // >= 1
  if (left < 32) v &= (1u << (int)left) - 1u;
  return v;
}

// the inclusive prefix of v over the workgroup's 256 threads and the workgroup's total
__device__ inline int allow_block_scan(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_w[wave] = x;
  __syncthreads();
  int pre = 0, tot = 0;
  for (int w = 0; w < 4; ++w) {
    const int c = s_w[w];
    if (w < wave) pre += c;
    tot += c;
  }
  __syncthreads();  // s_w may be written again
  *total = tot;
  return x + pre;
}

// The bitmap of the list blockIdx.y builds.  sel null: the one bitmap `bits` (null: every id).  Else
// sel[blockIdx.y] names a row of `stride` words (the host passes rows in [0, G) only), -1: every id.
__device__ inline const uint32_t* allow_list_row(const uint32_t* __restrict__ bits, int64_t stride,
                                                 const int32_t* __restrict__ sel) {
  if (!sel) return bits;
  const int32_t g = sel[blockIdx.y];
  return g < 0 ? nullptr : bits + (int64_t)g * stride;
}

// grid: x = block of 256 words, y = list; list y keeps its gridDim.x + 1 words of block_cnt
__global__ __launch_bounds__(256) void allow_count_kernel(const uint32_t* __restrict__ bits, int64_t stride,
                                                          const int32_t* __restrict__ sel, int64_t words, int64_t n,
                                                          int64_t* __restrict__ block_cnt) {
  __shared__ int s_w[4];
  const uint32_t* __restrict__ allow = allow_list_row(bits, stride, sel);
  const int64_t w = (int64_t)blockIdx.x * kAllowListWords + threadIdx.x;
  int tot = 0;
  allow_block_scan(__popc(allow_word(allow, w, words, n)), s_w, &tot);
  if (threadIdx.x == 0) block_cnt[(int64_t)blockIdx.y * (gridDim.x + 1) + blockIdx.x] = tot;
}

// in place: block_off[i] := the sum of block_off[0 .. i), block_off[nblk] := the total; one workgroup
// per list, list x at block_off + x * (nblk + 1)
__global__ __launch_bounds__(256) void allow_scan_kernel(int64_t* __restrict__ block_off, int64_t nblk) {
  __shared__ long long s_w[4];
  block_off += (int64_t)blockIdx.x * (nblk + 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long base = 0;  // block-uniform
  for (int64_t i0 = 0; i0 < nblk; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    const long long v = i < nblk ? (long long)block_off[i] : 0;
    long long x = v;
    for (int o = 1; o < 64; o <<= 1) {
      const long long y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    long long pre = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
      const long long c = s_w[w];
      if (w < wave) pre += c;
      tot += c;
    }
    __syncthreads();
    if (i < nblk) block_off[i] = (int64_t)(base + pre + x - v);
    base += tot;
  }
  if (threadIdx.x == 0) block_off[nblk] = (int64_t)base;
}

// grid as allow_count_kernel's; list y starts at out_ids + list_off[y] (null: 0)
__global__ __launch_bounds__(256) void allow_scatter_kernel(const uint32_t* __restrict__ bits, int64_t stride,
                                                            const int32_t* __restrict__ sel, int64_t words,
                                                            int64_t n, const int64_t* __restrict__ block_off,
                                                            const int64_t* __restrict__ list_off,
                                                            int32_t* __restrict__ out_ids) {
  __shared__ int s_w[4];
  const uint32_t* __restrict__ allow = allow_list_row(bits, stride, sel);
  const int64_t w = (int64_t)blockIdx.x * kAllowListWords + threadIdx.x;
  uint32_t v = allow_word(allow, w, words, n);
  const int c = __popc(v);
  int tot = 0;
  const int incl = allow_block_scan(c, s_w, &tot);
  // behind the list's start: < its popcount, which the host sized the slab from
  int64_t o = (list_off ? list_off[blockIdx.y] : 0) + block_off[(int64_t)blockIdx.y * (gridDim.x + 1) + blockIdx.x] +
              (incl - c);
  const int32_t id0 = (int32_t)(w * 32);
  while (v) {
    out_ids[o++] = id0 + (__ffs(v) - 1);
    v &= v - 1;
  }
}

__global__ __launch_bounds__(256) void allow_ranges_kernel(const int64_t* __restrict__ total, int64_t nq,
                                                           VoteRange* __restrict__ vranges,
                                                           int64_t* __restrict__ vrng_off) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < nq) vranges[q] = VoteRange{0, (int32_t)*total, 0};
  if (q <= nq) vrng_off[q] = q;
}

}  // namespace

int32_t allow_compact(rpt_ctx* ctx, const int32_t* perm, const VoteRange* ranges, const int64_t* rng_off,
                      const int64_t* cand_off, int T, const AllowSlice& sl, const AllowGroups& allow,
                      int32_t* out_ids, VoteRange* vranges, int64_t* vrng_off, int32_t* counts,
                      unsigned long long* allowed_total) {
  if (sl.ns == 0) return RPT_OK;
  RPT_ARG(sl.ns <= 0x7fffffff, "too many queries for one allow-compaction launch");
  hipLaunchKernelGGL(allow_compact_kernel, dim3((unsigned)sl.ns), dim3(256), 0, ctx->stream, perm, ranges, rng_off,
                     cand_off, T, sl.q0, allow, out_ids, vranges, vrng_off, counts, allowed_total);
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

int32_t allow_list(rpt_ctx* ctx, const uint32_t* allow, int64_t n, int64_t* block_off, int32_t* out_ids,
                   int64_t nq, VoteRange* vranges, int64_t* vrng_off) {
  RPT_ARG(n >= 0 && n <= 0x7fffffff, "too many rows for an allow-list");
  const int64_t words = (n + 31) / 32, nblk = allow_list_blocks(n);
  RPT_ARG(nblk <= 0x7fffffff && nq <= (int64_t)0x7fffffff * 128, "too many blocks for one launch");
  if (nblk > 0) {
    hipLaunchKernelGGL(allow_count_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, allow, (int64_t)0,
                       (const int32_t*)nullptr, words, n, block_off);
    RPT_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(allow_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, block_off, nblk);
  RPT_HIP(hipGetLastError());
  if (nblk > 0) {
    hipLaunchKernelGGL(allow_scatter_kernel, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, allow, (int64_t)0,
                       (const int32_t*)nullptr, words, n, block_off, (const int64_t*)nullptr, out_ids);
    RPT_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(allow_ranges_kernel, dim3((unsigned)((nq + 1 + 255) / 256)), dim3(256), 0, ctx->stream,
                     block_off + nblk, nq, vranges, vrng_off);
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

// the lists of one launch: the y dimension of a grid
constexpr int64_t kAllowListRows = 65535;

int32_t allow_group_count(rpt_ctx* ctx, const uint32_t* bits, int64_t stride, int64_t n, const int32_t* sel,
                          int64_t R, int64_t* block_off) {
  RPT_ARG(n >= 0 && n <= 0x7fffffff, "too many rows for an allow-list");
  const int64_t words = (n + 31) / 32, nblk = allow_list_blocks(n);
  RPT_ARG(nblk <= 0x7fffffff, "too many blocks for one launch");
  for (int64_t r0 = 0; r0 < R; r0 += kAllowListRows) {
    const unsigned nr = (unsigned)std::min<int64_t>(kAllowListRows, R - r0);
    int64_t* bo = block_off + r0 * (nblk + 1);
    if (nblk > 0) {
      hipLaunchKernelGGL(allow_count_kernel, dim3((unsigned)nblk, nr), dim3(256), 0, ctx->stream, bits, stride,
                         sel + r0, words, n, bo);
      RPT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(allow_scan_kernel, dim3(nr), dim3(256), 0, ctx->stream, bo, nblk);
    RPT_HIP(hipGetLastError());
  }
  return RPT_OK;
}

int32_t allow_group_scatter(rpt_ctx* ctx, const uint32_t* bits, int64_t stride, int64_t n, const int32_t* sel,
                            int64_t R, const int64_t* block_off, const int64_t* list_off, int32_t* out_ids) {
  const int64_t words = (n + 31) / 32, nblk = allow_list_blocks(n);
  if (nblk == 0) return RPT_OK;
  for (int64_t r0 = 0; r0 < R; r0 += kAllowListRows) {
    const unsigned nr = (unsigned)std::min<int64_t>(kAllowListRows, R - r0);
    hipLaunchKernelGGL(allow_scatter_kernel, dim3((unsigned)nblk, nr), dim3(256), 0, ctx->stream, bits, stride,
                       sel + r0, words, n, block_off + r0 * (nblk + 1), list_off + r0, out_ids);
    RPT_HIP(hipGetLastError());
  }
  return RPT_OK;
}

}  // namespace rpt
