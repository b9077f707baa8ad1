// knn_plan.h — the host-side plan of a fused kNN call: which kernel family answers it, on which
// ranking tier, how many entries the tier keeps, how much LDS the launch needs and which shadows of
// the dataset are built first.  Plain C++17 (no HIP headers): knn.hip launches what fused_plan says,
// and tests/test_knn_plan_host.py pins these rules on the CPU.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RPT_HD __host__ __device__
#else
#define RPT_HD
#endif

namespace rpt {

// Dense f64 rows under L2: the batched distance passes RANK on butterfly sums, the answer is defined
// on the reference's left fold (RPTree.hs:174 ranks ALL candidates on the fold).  A ranking path
// keeps the entries of the best k + kLfMargin DIFFERENT ids by (butterfly distance, position) — copies
// of one id, the same point found by several trees, have one value under either sum and must not
// use the margin up — at most the capacity of its list; those are evaluated again as the fold and
// the k best of THOSE by (fold distance, position) are written.  Then the cut is CERTIFIED per query
// (l2_cut_certified); a query that is not certified is answered again by the exact kernel
// (knn_metric_kernel<double, kMetricL2, true>: every candidate on the fold, no margin), so the
// answer is the definition however many different rows tie at the k-th distance.
constexpr int kLfMargin = 8;

// ---- the workgroup kernel (knn_fused_kernel) ---------------------------------------------
constexpr int kFC = 2048;     // candidates per batch
constexpr int kFR = 512;      // leaf ranges per query in LDS
constexpr int kFK = 64;       // largest k served by the arg-min selection
constexpr int kFKx = kFK + kLfMargin;  // capacity of the running best list (see kLfMargin)
// the workgroup kernel's prefilter tiers may keep more than that: the threshold selection costs
// the same whatever it keeps, and the int8 tier needs a wide margin at the cut (see Sh8)
constexpr int kBK = 224;
constexpr int kBKx = kBK + kLfMargin;
constexpr int kVoteCap = 16384;  // candidates of one query the voting mode can count (64 KB of LDS)

// ---- the one-wave kernel (knn_fused_wave_kernel) -----------------------------------------
constexpr int kWC = 512;  // candidates per batch of one wave
constexpr int kWR = 128;  // leaf ranges per query
constexpr int kWT = 64;   // trees (lane = tree)
// the variant is chosen when trees x minLeaf (~ candidates per query) is at most this
// (round 3: trees x the leaf size the topology gives, at most 700 — it was trees x minLeaf <= 1024.
// With the threshold selection, the single traversal and the in-kernel retry the workgroup kernel
// answers an 8-tree shard of C2 (8 x 122 candidates) in 0.67 ms, this one in 0.96; the 8 x 76 of a
// C4 shard stay here: 3.2 against 5.9 ms per 100 000 queries)
constexpr int64_t kWaveCandidates = 700;
constexpr int64_t kShardCandidates = 2100;  // ... and the round-4 shard kernels (see fused_plan)
// (the one-wave kernel takes its int8 threshold from the 64 per-lane minima: beyond the 48th of them
// the candidate list outgrows its 128 slots)
constexpr int kWaveKeep8 = 48;

constexpr int kSKmax = 48;  // largest k the shard kernel serves (the carried list must hold k and its band)

// ---- dynamic LDS of the three kernel families ---------------------------------------------
RPT_HD inline size_t fused_wave_bytes(int d, size_t acc_size) {  // one wave of knn_fused_wave_kernel
  const size_t b = (size_t)kWC * 12 + (size_t)kWR * 24 + (size_t)kFKx * 16 + (size_t)d * (acc_size + 4);
  return (b + 15) & ~(size_t)15;
}

RPT_HD inline size_t shard_wave_bytes(int d, size_t acc_size, int kSL, int WC) {  // ... of knn_shard_wave_kernel
  const size_t b = (size_t)WC * 8 + (size_t)kWR * 8 + (size_t)(kWR + 4) * 4 + (size_t)kSL * 20 + 16 +
                   (((size_t)d * acc_size + 15) & ~(size_t)15) + (size_t)d * 4;
  return (b + 15) & ~(size_t)15;
}

inline size_t fused_block_bytes(int d, size_t acc_size, bool vote) {  // a workgroup of knn_fused_kernel
  return (size_t)kFC * 16 + (size_t)kFR * 12 + 2048 * 4 + (size_t)kBKx * 16 + (size_t)d * (acc_size + 4) + 64 +
         (vote ? (size_t)kVoteCap * 4 + 16 : 0);
}

inline int prefilter_keep(int k) { return k + (k / 2 > 6 ? k / 2 : 6); }

// ---- what the decision depends on ---------------------------------------------------------
enum class Elem { F64, F32, BF16 };

// what a forest has learnt from its earlier query batches (fused_after_batch)
struct TierState {
  // set when a query batch had more than a quarter of its f32-prefilter cuts uncertified (many
  // equal distances: e.g. the queries are data points, found once per tree): later batches on this
  // forest go straight to the all-f64 kernel
  bool prefilter_off = false;
  bool pre8_off = false;   // ... and one more: the int8 shadow failed too many cuts here
  bool pre16_off = false;  // ... the same one tier up: the f16 shadow failed too many cuts here
  double kp8_boost = 1.0;  // int8 tier: factor on the kept entries, raised when a batch retried often
};

struct FusedIn {
  Elem elem = Elem::F64, proj = Elem::F64;  // rows; projections (F64 or F32)
  bool csr = false;
  int d = 0, k = 0;
  int dedup = 0;  // duplicate rule of the call
  int vote = 0;   // vote threshold (0: no voting)
  bool rerun = false;  // the second launch of a call: the uncertified queries, exact distances only
  int T = 0, L = 0, min_leaf = 0;  // the forest
  int64_t n = 0;
  TierState tiers;
  // options (rpt_options), by value
  int64_t knn_wave = -1, knn_kp = 0, knn_kp16 = 0, knn_kp8 = 0;
  bool knn_no_pre32 = false, knn_no_pre16 = false, knn_no_pre8 = false, knn_csr_pre32 = false,
       knn_shard_old = false;
  // the dataset's shadows that exist
  bool shadow8 = false, shadow16 = false, shadow32 = false, shadow_col16 = false, shadow_ell = false;
};

// Every ranking tier wants duplicates kept and no voting; the half tier (and the ELL table) can be
// switched off by option or by the forest, and the int8 tier stands on the half tier's switches too
inline bool tiers_allowed(const FusedIn& in) { return in.dedup == 0 && in.vote == 0 && !in.knn_no_pre32; }
inline bool half_allowed(const FusedIn& in) {
  return tiers_allowed(in) && !in.knn_no_pre16 && !in.tiers.pre16_off;
}
inline bool int8_allowed(const FusedIn& in) {
  return half_allowed(in) && !in.knn_no_pre8 && !in.tiers.pre8_off;
}

// ---- the shadows a call builds first ------------------------------------------------------
enum : unsigned { kShadow8 = 1, kShadow32 = 2, kShadow16 = 4, kShadowCsr32 = 8, kShadowEll = 16 };

// The ensure_shadow* calls knn_dev makes next, given those it has made for this call (`tried`) and
// what they left (in.shadow*: an ensure_* may leave its shadow absent — no memory, rows that are not
// a multiple of 16 elements, a value out of range); 0: none, launch.  (No shadow when voting or
// under a duplicate rule: nothing ranks on one then.)
inline unsigned fused_shadows_wanted(const FusedIn& in, unsigned tried) {
  if (!tiers_allowed(in)) return 0;
  const bool half_on = half_allowed(in), int8_on = int8_allowed(in);
  const bool pre32_on = in.proj == Elem::F64 && prefilter_keep(in.k) < kFK && !in.tiers.prefilter_off;
  if (in.csr) {
    // CSR rows: the (u16, f32) shadow halves the bytes of the ranking pass but NOT its time — at C3
    // the exact kernel already gathers rows at 6.4 TB/s and the f32 pass, with its 17 selection
    // rounds per batch, is bound by its serial phases (14.3 ms against 13.8 ms per 10 000 queries):
    // opt-in (knn_csr_pre32), kept for bandwidth-poorer configurations and pinned by a test
    if (!pre32_on || in.elem != Elem::F64 || in.d > 65536) return 0;
    return ((in.knn_csr_pre32 ? kShadowCsr32 : 0u) | (half_on ? kShadowEll : 0u)) & ~tried;
  }
  // bf16 rows: the int8 tier exists (identical answers, tested) but is OPT-IN (knn_kp8 > 0): at C5
  // (10 M x 768, k = 50) the cut needs 200 kept rows to certify 99 % of the queries and the pass is
  // then no faster than the plain bf16 kernel (82 against 68 ms per 100 000 queries) — its 768-byte
  // rows keep half the bytes in flight per wave — while the shadow costs 7.7 GB
  if (in.elem == Elem::BF16)
    return (in.knn_kp8 > 0 && int8_on && !in.tiers.prefilter_off ? kShadow8 : 0u) & ~tried;
  if (in.elem == Elem::F64 ? !pre32_on : !half_on) return 0;
  // the int8 shadow first; the f32 and half ones (+75 % of the dataset) only when it cannot rank
  // this call: rows that are not a multiple of 16 elements, k beyond what the tier keeps in the
  // one-wave kernel, no memory, or a forest that has dropped the tier (once per dataset each)
  if (int8_on && !(tried & kShadow8)) return kShadow8;
  if (int8_on && in.shadow8 && in.k + 8 <= kWaveKeep8 - 1) return 0;
  if (in.elem == Elem::F32) return kShadow16 & ~tried;  // (f32 rows: the half shadow is the only other tier)
  if (!(tried & kShadow32)) return kShadow32;
  return (in.shadow32 && half_on ? kShadow16 : 0u) & ~tried;
}

// ---- the launch ---------------------------------------------------------------------------
enum class Family { Workgroup, Wave, Shard };  // knn_fused_kernel; knn_fused_wave_kernel;
                                               // shard_ranges_kernel + knn_shard_wave_kernel
enum class CsrRank { Plain, Shadow32, Ell };   // CSR rows: ranked on themselves, their (u16, f32) shadow, their half table

struct FusedPlan {
  Family family = Family::Workgroup;
  bool one_batch = false;  // Shard: a query's candidates are one batch (<TD, tier, 128, 4, 512>, else <.., 256, 3, 640>)
  int tier = 0;            // 0 exact, 1 f32 shadow, 2 half shadow / ELL table, 3 int8 shadow
  CsrRank csr_rank = CsrRank::Plain;
  int k1 = 0;         // entries the tier keeps + 1; tier 0: -1 for the rerun, else 0
  bool sh16 = false;  // the kernels' sh16 argument: a half shadow / the ELL table is there to rank on
  size_t smem = 0;    // dynamic LDS bytes of the launch
  int64_t est_cand = 0;  // candidates per query the topology promises: trees x leaf size
};

inline FusedPlan fused_plan(const FusedIn& in) {
  FusedPlan p;
  const bool f64 = in.elem == Elem::F64, f32 = in.elem == Elem::F32, bf16 = in.elem == Elem::BF16;
  const size_t acc = f64 ? 8 : 4;
  const int k = in.k;
  // small shards (few trees => a few hundred candidates per query): one wave per query
  const size_t wbytes = fused_wave_bytes(in.d, acc);
  int64_t leaf = in.n;  // the size splitting stops at: the first level's node size <= minLeaf, or depth L
  for (int l = 0; l < in.L && leaf > (int64_t)in.min_leaf; ++l) leaf -= leaf / 2;
  const int64_t est_cand = p.est_cand = (int64_t)in.T * (leaf > 0 ? leaf : 1);
  const bool lanes = in.T >= 1 && in.T <= kWT;
  bool wave = lanes && wbytes <= 16 * 1024 && est_cand <= kWaveCandidates;
  // the round-4 shard kernels (traversal as its own launch, adaptive certified set) stay ahead of the
  // workgroup kernel for longer: an 8-tree C2 shard (980 candidates) 0.42 against 0.65 ms per 10 000
  // queries, 16 trees (1950) 0.73 against 0.86 (5.7 against 7.9 ms per 100 000); at 32 trees the
  // workgroup kernel is level or ahead
  bool wave_shard = lanes && wbytes <= 16 * 1024 && est_cand <= kShardCandidates;
  if (in.knn_wave >= 0) wave = wave_shard = in.knn_wave == 1 && lanes && wbytes <= 40 * 1024;
  if (in.vote > 0 || in.csr) wave = wave_shard = false;  // voting mode: the workgroup kernel, all-exact distances

  // ---- the tier (none in the second launch of a call)
  const bool ranked = tiers_allowed(in) && !in.rerun;
  const bool half_on = half_allowed(in) && !in.rerun;
  // f64 data, duplicates kept, small k: rank the candidates on the f32 shadow (half the row
  // bytes), exact distances for the best k' only, cut certified per query (see the kernels)
  // entries the f32 pass keeps: every one costs a selection round per batch (16 of them: 0.75 ms
  // per 10 000 queries at C2), too few and cuts fail their certificate (re-run per query): k + 6
  // certifies 10 000 of 10 000 C2 queries
  const int kp_env = (int)in.knn_kp, kp16_env = (int)in.knn_kp16, kp8_env = (int)in.knn_kp8;
  int kp = kp_env > k && kp_env < kFK ? kp_env : prefilter_keep(k);
  const bool pre32 = f64 && ranked && kp + 1 <= kFK && in.shadow32 && !in.tiers.prefilter_off &&
                     (!in.csr || in.shadow_col16);
  // first tier: rank on the HALF shadow (a quarter of the f64 bytes); its rounding is coarser, so it
  // keeps a few more entries for the exact pass: k + max(8, k / 2) (C2: 10 000 of 10 000 queries
  // certified with 18 kept, 2.55 ms per batch against 4.10 ms on the f32 shadow; 26 kept 2.70 ms)
  const int kp16 = kp16_env > k && kp16_env < kFK ? kp16_env : k + (k / 2 > 8 ? k / 2 : 8);
  // (f32 data: the half shadow is the only ranking tier; the kept rows are refined with the very
  // f32 distance the all-f32 kernel ranks on, so the answers are identical)
  const bool sh16 = !in.csr && in.shadow16 && half_on && kp16 + 1 <= kFK && (pre32 || f32);
  // SVector rows: the fixed-width half table is their first tier (the f32 CSR shadow is opt-in)
  const bool ell = f64 && in.csr && in.shadow_ell && half_on && kp16 + 1 <= kFK && !in.tiers.prefilter_off;
  if (sh16 || ell) kp = kp16;
  // ... or, before that, on the INT8 shadow (an eighth of the f64 bytes; integer ranking values, the
  // cut certified through the triangle inequality, see Sh8): coarser again, k + max(48, k) kept
  const int kcap8 = wave ? kWaveKeep8 : kBK;
  // (the width of the band at the cut grows with the square root of the row length: sqrt(d / 128)
  // times the margin that certifies C2's 128-element rows)
  // ... and with the number of candidates (the band holds a share of them: 48 certify C2's 3922 and a
  // C4 forest's 3686 per query, not the 4915 of C4's 64 trees, where most queries took the in-kernel
  // retry — a second pass over all candidates: 3.5 ms per 10 000 queries against 2.0 with 100 kept),
  // and with what the forest's earlier batches reported (kp8_boost: retries counted by the kernel)
  const double cand_scale = est_cand > 4000 ? (double)est_cand / 4000.0 : 1.0;
  const int margin8 = (int)((k > 48 ? k : 48) * (in.d > 128 ? std::sqrt((double)in.d / 128.0) : 1.0) *
                            cand_scale * in.tiers.kp8_boost);
  int kp8 = kp8_env > k && kp8_env < kcap8 ? kp8_env : k + margin8;
  if (kp8 > kcap8 - 1) kp8 = kcap8 - 1;
  const bool sh8 = !in.csr && in.shadow8 && int8_allowed(in) && !in.rerun && kp8 >= k + 8 &&
                   !in.tiers.prefilter_off && !(bf16 && wave);  // (bf16: the workgroup kernel only)
  if (sh8) kp = kp8;
  p.tier = sh8 ? 3 : (sh16 || ell) ? 2 : pre32 ? 1 : 0;
  p.csr_rank = ell ? CsrRank::Ell : pre32 && in.csr ? CsrRank::Shadow32 : CsrRank::Plain;
  p.sh16 = sh16 || ell;
  p.k1 = p.tier > 0 ? kp + 1 : in.rerun ? -1 : 0;

  // ---- the kernel family.  Only the prefiltered f64 / f32 instantiations have the shard kernels
  // (knn_shard_old = 1 keeps the round-3 one-wave kernel); a forced wave variant on very long rows:
  // the shard kernels' slab must fit the CU's LDS
  if (wave_shard && !bf16 && p.tier > 0 && k <= kSKmax && !in.knn_shard_old &&
      4 * shard_wave_bytes(in.d, acc, 256, 640) <= 160 * 1024) {
    p.family = Family::Shard;
    p.one_batch = est_cand <= kWC;
    p.smem = 4 * (p.one_batch ? shard_wave_bytes(in.d, acc, 128, 512) : shard_wave_bytes(in.d, acc, 256, 640));
  } else if (wave) {
    p.family = Family::Wave;
    p.smem = 4 * wbytes;
  } else {
    p.smem = fused_block_bytes(in.d, acc, in.vote > 0);
  }
  return p;
}

// ---- after a batch ------------------------------------------------------------------------
// What the forest learns from a batch of nq queries that ran on `tier`: `uncertified` cuts failed
// their certificate, `retries` queries took the in-kernel wider second attempt.
inline void fused_after_batch(TierState& st, int tier, uint64_t nq, uint64_t uncertified, uint64_t retries) {
  // too many uncertified cuts: one tier down for the later batches on this forest (half -> f32
  // shadow -> all-f64)
  if (uncertified * 4 > nq) {
    if (tier == 3) st.pre8_off = true;
    else if (tier == 2) st.pre16_off = true;
    else if (tier == 1) st.prefilter_off = true;  // (tier 0: the count is the f64 kernels' own)
  }
  // a batch in which more than an eighth of the queries needed the wider second attempt: the next
  // batches on this forest start wider (the int8 tier's kept entries; capped by the kernel's list)
  if (tier == 3 && retries * 8 > nq && st.kp8_boost < 4.0) st.kp8_boost *= 1.5;
}

}  // namespace rpt
