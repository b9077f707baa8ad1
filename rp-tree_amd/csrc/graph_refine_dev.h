// graph_refine_dev.h — what the NN-descent rounds over dense rows (graph_refine.hip) and over CSR
// rows (graph_csr.hip) share besides graph_dev.h: the round's device-side state, its bookkeeping
// kernels and the LDS hash set of a point's candidates.
#pragma once

#include "graph_dev.h"

namespace rpt {
namespace {

// the hash set: a free slot is kEmpty (graph_dev.h); a member c is stored as c (new) or ~c (i itself
// and F(i): never a candidate)

struct RefineState {
  int32_t active;  // 0: an earlier round changed no row, the kernels of this round return at once
  int32_t pad;
  unsigned long long changed;  // rows the running round changed
  unsigned long long rounds, updates, candidates;
};

__global__ void refine_begin_kernel(RefineState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->active = 1;
    st->pad = 0;
    st->changed = 0;
    st->rounds = 0;
    st->updates = 0;
    st->candidates = 0;
  }
}

__global__ void refine_end_kernel(RefineState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && st->active) {
    st->rounds += 1;
    if (st->changed == 0) st->active = 0;
    st->changed = 0;
  }
}

__global__ void refine_copy_kernel(const RefineState* st, int64_t n, int k,
                                   const int32_t* __restrict__ sids, const double* __restrict__ sdist,
                                   const int32_t* __restrict__ scount, int32_t* __restrict__ ids,
                                   double* __restrict__ dist, int32_t* __restrict__ count) {
  if (!st->active) return;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * k; e += stride) {
    ids[e] = sids[e];
    dist[e] = sdist[e];
    if (e < n) count[e] = scount[e];
  }
}

// c joins the set unless it is there (as old or new); `stored` is c or ~c
__device__ inline void set_insert(int* tab, int mask, int shift, int c, int stored) {
  unsigned h = ((unsigned)c * 2654435761u) >> shift;
  for (;;) {
    const int old = atomicCAS(&tab[h], kEmpty, stored);
    if (old == kEmpty || old == c || old == ~c) return;
    h = (h + 1) & (unsigned)mask;
  }
}
}  // namespace
}  // namespace rpt
