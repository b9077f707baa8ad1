// knn_vote.h — the vote-select step of rpt_knn_vote_* / rpt_vote_candidates_host (knn_vote.hip),
// called by knn.hip's knn_vote / vote_candidates.
#pragma once

#include <stdint.h>

struct rpt_ctx;

namespace rpt {

// knn.hip's Range, member for member (knn.hip asserts the layout): candidates perm[poff .. poff + n),
// the first of them at position `pos` of the query's candidate list
struct VoteRange {
  int64_t poff;
  int32_t n;
  int32_t pos;
};

constexpr int kVoteLds = 16384;  // ids one workgroup sorts in LDS (64 KB: two workgroups per CU)

// What one launch of the vote-select kernel works on: queries q0 .. q0 + ns - 1 of a query plan.
struct VoteSlice {
  int64_t q0 = 0, ns = 0;
  int64_t cand_words = 0;  // candidates of the slice = words of its id slabs
  int64_t sort_words = 0;  // words of the global sort slabs (queries over the LDS bound)
  int lds_words = 1;       // power of two: the largest LDS sort of the slice
};

// The voted list of every query of the slice: the ids that at least v of the query's candidate
// entries carry, ascending, each once, written to out_ids from word cand_off[q * T] - cand_off[q0 * T]
// on (out_counts, unless null, holds each id's number of entries at the same place), and described by
// vranges[q - q0] = {that word, the number of voted ids, 0}, vrng_off[i] = i for i in 0 .. ns.
// sort_off[q]: the query's first word in sort_slab (a power of two >= its candidates, for queries with
// more than lds_cap candidates), ignored for the others.  *voted_total grows by the slice's voted ids.
// Enqueues on the ctx stream; every pointer is device memory.
int32_t vote_select(rpt_ctx* ctx, const int32_t* perm, const VoteRange* ranges, const int64_t* rng_off,
                    const int64_t* cand_off, int T, const VoteSlice& sl, int v, int lds_cap,
                    const int64_t* sort_off, int32_t* sort_slab, int32_t* out_ids, int32_t* out_counts,
                    VoteRange* vranges, int64_t* vrng_off, unsigned long long* voted_total);

// cand_off[q * T] for q in 0 .. nq, packed ([nq + 1] on the device); enqueues on the ctx stream
int32_t vote_query_starts(rpt_ctx* ctx, const int64_t* cand_off, int T, int64_t nq, int64_t* starts);

}  // namespace rpt
