// knn_allow.h — the list steps of rpt_knn_allow_* / rpt_allow_candidates_host / rpt_brute_knn_allow_*
// (knn_allow.hip), called by knn.hip's knn_allow_dev / allow_candidates / brute_knn_allow_dev.
#pragma once

#include <stdint.h>

#include "common.h"
#include "knn_vote.h"

struct rpt_ctx;

namespace rpt {

// What one launch of the compaction kernel works on: queries q0 .. q0 + ns - 1 of a query plan.
struct AllowSlice {
  int64_t q0 = 0, ns = 0;
  int64_t cand_words = 0;  // candidates of the slice = words of its id slab
};

// The allowed list of every query of the slice: the query's candidate list (trees ascending, leaves
// left to right, duplicates kept) without the entries whose id is not allowed, in the same order,
// written to out_ids from word cand_off[q * T] - cand_off[q0 * T] on and described by
// vranges[q - q0] = {that word, the number of kept entries, 0}, vrng_off[i] = i for i in 0 .. ns,
// counts[q - q0] = the number of kept entries.  allow: query q's own bitmap (common.h: AllowGroups,
// indexed by the query's number in the whole batch, so a slice may hold any mix of groups) of
// ceil(n / 32) words, id i = bit i & 31 of word i >> 5; null = every id.  Candidate ids are rows of the forest (< n), so no bit at or behind n is
// ever read.  *allowed_total grows by the slice's kept entries.  Enqueues on the ctx stream; every
// pointer is device memory.
int32_t allow_compact(rpt_ctx* ctx, const int32_t* perm, const VoteRange* ranges, const int64_t* rng_off,
                      const int64_t* cand_off, int T, const AllowSlice& sl, const AllowGroups& allow,
                      int32_t* out_ids, VoteRange* vranges, int64_t* vrng_off, int32_t* counts,
                      unsigned long long* allowed_total);

// words a block of the list kernels takes (one per thread)
constexpr int kAllowListWords = 256;
inline int64_t allow_list_blocks(int64_t n) {
  const int64_t words = (n + 31) / 32;
  return (words + kAllowListWords - 1) / kAllowListWords;
}

// The ascending list of the allowed ids in [0, n): out_ids[0 .. total), n <= 2^31 - 1 of them at most
// (out_ids holds n words).  allow as above (null = every id); the tail word is masked at n.
// block_off: [allow_list_blocks(n) + 1] words of scratch; block_off[allow_list_blocks(n)] = total
// afterwards.  Then nq ranges {0, total, 0} with vrng_off[i] = i for i in 0 .. nq: every query ranks
// the one list.  Enqueues on the ctx stream.
int32_t allow_list(rpt_ctx* ctx, const uint32_t* allow, int64_t n, int64_t* block_off, int32_t* out_ids,
                   int64_t nq, VoteRange* vranges, int64_t* vrng_off);

// One list per group (rpt_brute_knn_allow_group_*).  sel[r], r in 0 .. R - 1, names the bitmap of list
// r: a row of `bits` (`stride` words each; the caller passes rows that exist only) or -1 = every id.
// allow_group_count: block_off is [R][allow_list_blocks(n) + 1] words; afterwards row r holds the
// exclusive scan of list r's block popcounts (the tail word masked at n) and, in its last word, the
// list's length.  allow_group_scatter: list r, ascending, to out_ids[list_off[r] ..), for the rows of
// `sel`, `block_off` and `list_off` it is given (a pass hands in pointers to its first list).  The
// caller sizes out_ids from the lengths.  Both enqueue on the ctx stream.
int32_t allow_group_count(rpt_ctx* ctx, const uint32_t* bits, int64_t stride, int64_t n, const int32_t* sel,
                          int64_t R, int64_t* block_off);
int32_t allow_group_scatter(rpt_ctx* ctx, const uint32_t* bits, int64_t stride, int64_t n, const int32_t* sel,
                            int64_t R, const int64_t* block_off, const int64_t* list_off, int32_t* out_ids);

}  // namespace rpt
