// knn_vote.hip — the vote threshold (MRPT) as a step of its own: from a query plan's leaf ranges to
// the list of ids that at least v trees propose, ascending, each once (keepCounts' order,
// RPTree.hs:464-478), as ONE range per query that every general kNN kernel can rank.
//
//   vote_select_kernel: one workgroup of 256 threads (four waves) per query.
//     1. the ranges' ids are copied into the sort array and padded to a power of two with
//        0x7fffffff (ids are row numbers < 2^31 - 1, so the padding sorts last and equals no id);
//     2. the bitonic network sorts it;
//     3. position i heads a run when S[i - 1] != S[i], and the run has at least v entries exactly
//        when S[i + v - 1] == S[i] (the array is sorted): one more read, no run lengths;
//     4. the kept heads are compacted in ascending order by a block-wide prefix sum (a ballot per
//        wave, four wave totals in LDS).  No atomic counter: the order is the answer.
//   The sort array is LDS (up to kVoteLds ids) or, for a query with more candidates, a slab of
//   global memory of the next power of two: the same network, the same code, any candidate count an
//   int32 holds.  Every word of a sort array is written before it is read, padding included.
//
// LDS: 4 bytes per id of the slice's largest LDS sort, 64 KB at the bound, which leaves two
// workgroups per CU.  The network's lanes take j consecutive words and skip j; 4-byte LDS accesses
// bank on the word address mod 32 within a 32-lane half.  For j <= 16 a half's 32 `lo` words lie in
// 64 consecutive ones and word w is taken together with w + 32 (a 2-way conflict); from j = 32 on a
// half reads 32 consecutive words (none).
#include "knn_vote.h"

#include "common.h"

namespace rpt {
namespace {

constexpr int32_t kVotePad = 0x7fffffff;

// S[0 .. np), np a power of two; I: int for the LDS array, int64_t for a global slab
template <class I>
__device__ inline void vote_bitonic(int32_t* S, I np) {
  for (I k = 2; k <= np; k <<= 1) {
    for (I j = k >> 1; j > 0; j >>= 1) {
      for (I i = threadIdx.x; i < (np >> 1); i += 256) {
        const I lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        const I hi = lo | j;
        const bool up = (lo & k) == 0;
        const int32_t a = S[lo], b = S[hi];
        if ((a > b) == up) {
          S[lo] = b;
          S[hi] = a;
        }
      }
      __syncthreads();
    }
    if (k > (np >> 1)) break;  // (k <<= 1 would overflow I at np = 2^(bits - 2) .. : leave first)
  }
}

template <class I>
__device__ inline int vote_query(int32_t* S, I nc, I np, const int32_t* __restrict__ perm,
                                 const VoteRange* __restrict__ ranges, int64_t r0, int64_t r1, int v,
                                 int32_t* __restrict__ out_ids, int32_t* __restrict__ out_counts, int* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = r0; r < r1; ++r) {
    const VoteRange rg = ranges[r];
    for (int i = threadIdx.x; i < rg.n; i += 256) S[(I)rg.pos + i] = perm[rg.poff + i];
  }
  for (I i = nc + threadIdx.x; i < np; i += 256) S[i] = kVotePad;
  __syncthreads();
  vote_bitonic<I>(S, np);
  int kept = 0;  // block-uniform
  for (I c0 = 0; c0 < nc; c0 += 256) {
    const I i = c0 + threadIdx.x;
    bool keep = false;
    int32_t id = 0;
    const int64_t last = (int64_t)i + (v - 1);  // the run's v-th entry, if it has one
    if (i < nc) {
      id = S[i];
      keep = (i == 0 || S[i - 1] != id) && last < (int64_t)nc && S[(I)last] == id;
    }
    const unsigned long long b = __ballot(keep);
    const int before = __popcll(b & ((1ULL << lane) - 1ULL));
    if (lane == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int pre = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
      const int c = s_w[w];
      if (w < wave) pre += c;
      tot += c;
    }
    if (keep) {
      const int o = kept + pre + before;
      out_ids[o] = id;
      if (out_counts) {  // the run's end: the first entry after `last` that differs (binary search)
        I a = (I)last, e = nc;  // S[a] == id, S[e] != id (e == nc: past the end)
        while (e - a > 1) {
          const I m = a + ((e - a) >> 1);
          if (S[m] == id) a = m;
          else e = m;
        }
        out_counts[o] = (int32_t)(e - i);
      }
    }
    kept += tot;
    __syncthreads();  // s_w is written again
  }
  return kept;
}

__global__ __launch_bounds__(256) void vote_select_kernel(
    const int32_t* __restrict__ perm, const VoteRange* __restrict__ ranges, const int64_t* __restrict__ rng_off,
    const int64_t* __restrict__ cand_off, int T, int64_t q0, int v, int lds_cap, int lds_words,
    const int64_t* __restrict__ sort_off, int32_t* __restrict__ sort_slab, int32_t* __restrict__ out_ids,
    int32_t* __restrict__ out_counts, VoteRange* __restrict__ vranges, int64_t* __restrict__ vrng_off,
    unsigned long long* __restrict__ voted_total) {
  extern __shared__ __attribute__((aligned(16))) int32_t s_ids[];  // [lds_words]
  __shared__ int s_w[4];
  const int64_t b = blockIdx.x, q = q0 + b;
  const int64_t c0 = cand_off[q * T], nc = cand_off[(q + 1) * T] - c0;
  const int64_t ostart = c0 - cand_off[q0 * T];
  const int64_t r0 = rng_off[q * T], r1 = rng_off[(q + 1) * T];
  int32_t* oc = out_counts ? out_counts + ostart : nullptr;
  int kept = 0;
  if (nc > 0 && nc <= (int64_t)lds_cap && nc <= (int64_t)lds_words) {
    int np = 1;
    while (np < (int)nc) np <<= 1;  // <= lds_words, itself a power of two
    kept = vote_query<int>(s_ids, (int)nc, np, perm, ranges, r0, r1, v, out_ids + ostart, oc, s_w);
  } else if (nc > 0) {
    int64_t np = 1;
    while (np < nc) np <<= 1;
    kept = vote_query<int64_t>(sort_slab + sort_off[q], nc, np, perm, ranges, r0, r1, v, out_ids + ostart, oc,
                               s_w);
  }
  if (threadIdx.x == 0) {
    vranges[b] = VoteRange{ostart, kept, 0};
    vrng_off[b] = b;
    if (b == 0) vrng_off[gridDim.x] = gridDim.x;
    if (kept) atomicAdd(voted_total, (unsigned long long)kept);
  }
}

__global__ __launch_bounds__(256) void vote_starts_kernel(const int64_t* __restrict__ cand_off, int T, int64_t nq,
                                                          int64_t* __restrict__ starts) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q <= nq) starts[q] = cand_off[q * T];
}

}  // namespace

int32_t vote_select(rpt_ctx* ctx, const int32_t* perm, const VoteRange* ranges, const int64_t* rng_off,
                    const int64_t* cand_off, int T, const VoteSlice& sl, int v, int lds_cap,
                    const int64_t* sort_off, int32_t* sort_slab, int32_t* out_ids, int32_t* out_counts,
                    VoteRange* vranges, int64_t* vrng_off, unsigned long long* voted_total) {
  if (sl.ns == 0) return RPT_OK;
  RPT_ARG(sl.ns <= 0x7fffffff, "too many queries for one vote-select launch");
  RPT_ARG(lds_cap >= 1 && lds_cap <= kVoteLds && sl.lds_words >= 1 && sl.lds_words <= kVoteLds &&
              (sl.lds_words & (sl.lds_words - 1)) == 0,
          "vote-select: LDS bound out of range");
  RPT_HIP(launch_dyn(vote_select_kernel, dim3((unsigned)sl.ns), dim3(256), (size_t)sl.lds_words * 4, ctx->stream,
                     perm, ranges, rng_off, cand_off, T, sl.q0, v, lds_cap, sl.lds_words, sort_off, sort_slab,
                     out_ids, out_counts, vranges, vrng_off, voted_total));
  return RPT_OK;
}

int32_t vote_query_starts(rpt_ctx* ctx, const int64_t* cand_off, int T, int64_t nq, int64_t* starts) {
  hipLaunchKernelGGL(vote_starts_kernel, dim3((unsigned)((nq + 1 + 255) / 256)), dim3(256), 0, ctx->stream,
                     cand_off, T, nq, starts);
  RPT_HIP(hipGetLastError());
  return RPT_OK;
}

}  // namespace rpt
