// Table test of rp-tree_amd/csrc/knn_plan.h: inputs of a fused kNN call against the plan the host code
// must make of them.  The expected values are worked out by hand from the rules (and the LDS sizes from
// the kernels' slab layouts), not with the header's own functions.  Built and run by
// tests/test_knn_plan_host.py; exit status 0 = every row holds.
#include <cstdio>

#include "knn_plan.h"

using namespace rpt;

static int failures = 0;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d (row %s): %s\n", __FILE__, __LINE__, row, #cond); \
      ++failures;                                                           \
    }                                                                       \
  } while (0)

// C2's forest: n = 1 000 000, L = 13, minLeaf 128 -> leaves of 123 points; f64 rows of 128 elements, k = 10
static FusedIn base(int T) {
  FusedIn in;
  in.d = 128;
  in.k = 10;
  in.T = T;
  in.L = 13;
  in.min_leaf = 128;
  in.n = 1000000;
  return in;
}
static FusedIn with8(int T) {
  FusedIn in = base(T);
  in.shadow8 = true;
  return in;
}
static FusedIn with_all(int T) {
  FusedIn in = with8(T);
  in.shadow16 = in.shadow32 = true;
  return in;
}

static void expect(const char* row, const FusedIn& in, Family family, int tier, int k1, size_t smem) {
  const FusedPlan p = fused_plan(in);
  CHECK(p.family == family);
  CHECK(p.tier == tier);
  CHECK(p.k1 == k1);
  CHECK(p.smem == smem);
  if (p.family != family || p.tier != tier || p.k1 != k1 || p.smem != smem)
    std::printf("  got family %d tier %d k1 %d smem %zu est_cand %lld\n", (int)p.family, p.tier, p.k1, p.smem,
                (long long)p.est_cand);
}

// the ensure_* calls in order, each leaving its shadow present unless `fail` names it
static unsigned walk_shadows(FusedIn in, unsigned fail, unsigned* steps) {
  unsigned tried = 0, n = 0;
  for (unsigned w; (w = fused_shadows_wanted(in, tried)) != 0 && n < 8; tried |= w) {
    steps[n++] = w;
    const unsigned got = w & ~fail;
    if (got & kShadow8) in.shadow8 = true;
    if (got & kShadow32) in.shadow32 = true;
    if (got & kShadow16) in.shadow16 = true;
    if (got & kShadowCsr32) in.shadow32 = in.shadow_col16 = true;
    if (got & kShadowEll) in.shadow_ell = true;
  }
  for (unsigned i = n; i < 8; ++i) steps[i] = 0;
  return n;
}
static void expect_shadows(const char* row, const FusedIn& in, unsigned fail, unsigned s0, unsigned s1 = 0,
                           unsigned s2 = 0) {
  unsigned st[8];
  const unsigned n = walk_shadows(in, fail, st);
  CHECK(n == (s0 ? 1u : 0u) + (s1 ? 1u : 0u) + (s2 ? 1u : 0u));
  CHECK(st[0] == s0 && st[1] == s1 && st[2] == s2);
}

// LDS bytes from the slab layouts (d = 128, f64 accumulators unless said otherwise)
constexpr size_t kBlock128 = 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 128 * 12 + 64;  // 52416
constexpr size_t kWave128 = 4 * (512 * 12 + 128 * 24 + 72 * 16 + 128 * 12);            // 4 x 11904
constexpr size_t kShardOne128 = 4 * (512 * 8 + 128 * 8 + 132 * 4 + 128 * 20 + 16 + 128 * 8 + 128 * 4);  // 4 x 9760
constexpr size_t kShardTwo128 = 4 * (640 * 8 + 128 * 8 + 132 * 4 + 256 * 20 + 16 + 128 * 8 + 128 * 4);  // 4 x 13344

int main() {
  const char* row = "0";
  {
    FusedIn in = base(32);
    CHECK(fused_plan(in).est_cand == 32 * 123);
    in.T = 8;
    CHECK(fused_plan(in).est_cand == 984);
    in.T = 4;
    CHECK(fused_plan(in).est_cand == 492);
    CHECK(prefilter_keep(10) == 16 && prefilter_keep(50) == 75);
  }
  // 1-3: the three kernel families by the candidates per query; the int8 tier keeps k + 48, 47 in a wave
  expect("1", with8(32), Family::Workgroup, 3, 59, kBlock128);
  expect_shadows("1", base(32), 0, kShadow8);
  expect("2", with8(8), Family::Shard, 3, 59, kShardTwo128);
  CHECK(!fused_plan(with8(8)).one_batch);
  expect("3", with8(4), Family::Shard, 3, 48, kShardOne128);
  CHECK(fused_plan(with8(4)).one_batch);
  {  // 4: k = 50 in a wave: no tier keeps few enough entries
    FusedIn in = with_all(4);
    in.k = 50;
    expect("4", in, Family::Wave, 0, 0, kWave128);
    expect_shadows("4", in, 0, 0);
    in.T = 32;  // (the workgroup kernel's int8 tier keeps k + 50 of a shadow an earlier call built)
    expect("4b", in, Family::Workgroup, 3, 101, kBlock128);
    in = base(32);
    in.k = 40;  // k + 8 beyond the one-wave kernel's 47: the f32 and half shadows are built as well
    expect_shadows("4c", in, 0, kShadow8, kShadow32, kShadow16);
  }
  {  // 5, 6: knn_shard_old: the prefiltered one-wave kernel where the wave rule holds, else the workgroup kernel
    FusedIn in = with8(4);
    in.knn_shard_old = true;
    expect("5", in, Family::Wave, 3, 48, kWave128);
    in.T = 8;
    expect("6", in, Family::Workgroup, 3, 59, kBlock128);
  }
  {  // 7: knn_wave forces the family; forced, a wave's slab may take 40 KB instead of 16 KB
    FusedIn in = with8(4);
    in.knn_wave = 0;
    expect("7a", in, Family::Workgroup, 3, 59, kBlock128);
    in = with8(32);
    in.knn_wave = 1;
    expect("7b", in, Family::Shard, 3, 48, kShardTwo128);
    in = with8(4);
    in.d = 640;  // a wave's slab: 10368 + 12 d = 18048 bytes; margin 48 sqrt(5) = 107
    expect("7c", in, Family::Workgroup, 3, 118, 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 640 * 12 + 64);
    in.knn_wave = 1;
    expect("7d", in, Family::Shard, 3, 48, 4 * (512 * 8 + 128 * 8 + 132 * 4 + 128 * 20 + 16 + 640 * 8 + 640 * 4));
    in.d = 2560;  // 41088 bytes
    expect("7e", in, Family::Workgroup, 3, 224, 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 2560 * 12 + 64);
  }
  {  // 8: d = 2496: a forced wave's slab fits (40320 bytes), four shard slabs of 41760 do not fit 160 KB
    FusedIn in = with8(4);
    in.knn_wave = 1;
    in.d = 2496;
    expect("8", in, Family::Wave, 3, 48, 4 * 40320);
  }
  {  // 9: d = 20: no int8 shadow
    FusedIn in = base(32);
    in.d = 20;
    expect_shadows("9", in, kShadow8, kShadow8, kShadow32, kShadow16);
    in.shadow32 = in.shadow16 = true;
    expect("9", in, Family::Workgroup, 2, 19, 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 20 * 12 + 64);
    CHECK(fused_plan(in).sh16);
    in = base(32);  // (no memory for the f32 shadow either: no half shadow, tier 0)
    in.d = 20;
    expect_shadows("9b", in, kShadow8 | kShadow32, kShadow8, kShadow32);
    expect("9b", in, Family::Workgroup, 0, 0, 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 20 * 12 + 64);
  }
  {  // 10-12: the options that switch tiers off
    FusedIn in = base(32);
    in.knn_no_pre16 = true;
    expect_shadows("10", in, 0, kShadow32);
    in.shadow8 = in.shadow16 = in.shadow32 = true;
    expect("10", in, Family::Workgroup, 1, 17, kBlock128);
    CHECK(!fused_plan(in).sh16);
    in = with_all(32);
    in.knn_no_pre32 = true;
    expect_shadows("11", in, 0, 0);
    expect("11", in, Family::Workgroup, 0, 0, kBlock128);
    in = base(32);
    in.knn_no_pre8 = true;
    expect_shadows("12", in, 0, kShadow32, kShadow16);
    in.shadow8 = in.shadow16 = in.shadow32 = true;
    expect("12", in, Family::Workgroup, 2, 19, kBlock128);
  }
  {  // 13: a forest that dropped its tiers one after another; all three shadows: the kept entries are the int8 tier's
    FusedIn in = with_all(32);
    expect("13", in, Family::Workgroup, 3, 59, kBlock128);
    CHECK(fused_plan(in).sh16);
    in.tiers.pre8_off = true;
    expect("13a", in, Family::Workgroup, 2, 19, kBlock128);
    expect_shadows("13a", in, 0, kShadow32, kShadow16);
    in.tiers.pre16_off = true;
    expect("13b", in, Family::Workgroup, 1, 17, kBlock128);
    expect_shadows("13b", in, 0, kShadow32);
    in.tiers.prefilter_off = true;
    expect("13c", in, Family::Workgroup, 0, 0, kBlock128);
    expect_shadows("13c", in, 0, 0);
  }
  {  // 14: f32 rows: the int8 and the half tier, never the f32 one
    const size_t block32 = 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 128 * 8 + 64;
    FusedIn in = base(32);
    in.elem = in.proj = Elem::F32;
    expect_shadows("14", in, 0, kShadow8);
    expect_shadows("14", in, kShadow8, kShadow8, kShadow16);
    expect("14", in, Family::Workgroup, 0, 0, block32);
    in.shadow32 = true;
    expect("14a", in, Family::Workgroup, 0, 0, block32);
    in.shadow16 = true;
    expect("14b", in, Family::Workgroup, 2, 19, block32);
    in.shadow8 = true;
    expect("14c", in, Family::Workgroup, 3, 59, block32);
    in.T = 8;  // the shard kernels serve f32 rows too: slabs with f32 accumulators
    expect("14d", in, Family::Shard, 3, 59, 4 * (640 * 8 + 128 * 8 + 132 * 4 + 256 * 20 + 16 + 128 * 4 + 128 * 4));
  }
  {  // 15, 16: bf16 rows: the int8 tier is opt-in and the workgroup kernel's only
    const size_t block32 = 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 128 * 8 + 64;
    FusedIn in = base(32);
    in.elem = Elem::BF16;
    in.proj = Elem::F32;
    expect_shadows("15", in, 0, 0);
    expect("15", in, Family::Workgroup, 0, 0, block32);
    in.knn_kp8 = 58;
    expect_shadows("16", in, 0, kShadow8);
    in.shadow8 = true;
    expect("16", in, Family::Workgroup, 3, 59, block32);
    in.T = 4;
    expect("16a", in, Family::Wave, 0, 0, 4 * (512 * 12 + 128 * 24 + 72 * 16 + 128 * 8));
    in.T = 8;  // (no shard kernels for bf16 rows)
    expect("16b", in, Family::Workgroup, 3, 59, block32);
  }
  {  // 17-19: SVector rows
    const size_t block64 = 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 64 * 12 + 64;
    FusedIn in = base(4);
    in.csr = true;
    in.d = 64;
    expect_shadows("17", in, 0, kShadowEll);
    in.shadow_ell = true;
    expect("17", in, Family::Workgroup, 2, 19, block64);
    CHECK(fused_plan(in).csr_rank == CsrRank::Ell && fused_plan(in).sh16);
    in.shadow_ell = false;
    in.knn_csr_pre32 = true;
    expect_shadows("18", in, kShadowEll, kShadowCsr32 | kShadowEll);
    in.shadow32 = in.shadow_col16 = true;
    expect("18", in, Family::Workgroup, 1, 17, block64);
    CHECK(fused_plan(in).csr_rank == CsrRank::Shadow32 && !fused_plan(in).sh16);
    in.shadow_col16 = false;  // (the f32 values without the u16 columns rank nothing)
    expect("18a", in, Family::Workgroup, 0, 0, block64);
    in.knn_no_pre16 = true;
    expect_shadows("18b", in, 0, kShadowCsr32);
    in = base(4);
    in.csr = true;
    in.d = 64;
    in.elem = in.proj = Elem::F32;
    in.shadow32 = in.shadow_col16 = in.shadow_ell = true;
    expect_shadows("19", in, 0, 0);
    expect("19", in, Family::Workgroup, 0, 0, 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 64 * 8 + 64);
    CHECK(fused_plan(in).csr_rank == CsrRank::Plain);
  }
  {  // 20-22: a duplicate rule, voting, the second launch: every distance exact
    FusedIn in = with_all(32);
    in.dedup = 1;
    expect_shadows("20", in, 0, 0);
    expect("20", in, Family::Workgroup, 0, 0, kBlock128);
    in = with_all(4);
    in.vote = 2;
    expect_shadows("21", in, 0, 0);
    expect("21", in, Family::Workgroup, 0, 0, kBlock128 + 16384 * 4 + 16);
    in = with_all(32);
    in.rerun = true;
    expect("22", in, Family::Workgroup, 0, -1, kBlock128);
    in.T = 4;
    expect("22a", in, Family::Wave, 0, -1, kWave128);
  }
  {  // 23-25: the int8 tier's margin: x sqrt(d / 128), x candidates / 4000, x the forest's boost
    FusedIn in = with8(32);
    in.d = 256;  // 48 sqrt(2) = 67.9
    expect("23", in, Family::Workgroup, 3, 78, 2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 256 * 12 + 64);
    in = with8(5);
    in.L = 0;
    in.n = 983;  // 5 x 983 = 4915 candidates: 48 x 1.22875 = 58.98
    CHECK(fused_plan(in).est_cand == 4915);
    expect("24", in, Family::Workgroup, 3, 69, kBlock128);
    in = with8(32);
    in.tiers.kp8_boost = 1.5;
    expect("25", in, Family::Workgroup, 3, 83, kBlock128);
    in.knn_kp = 20;  // the options that set the kept entries
    in.knn_kp16 = 30;
    in.knn_kp8 = 40;
    expect("25a", in, Family::Workgroup, 3, 41, kBlock128);
    in.shadow8 = false;
    in.shadow16 = in.shadow32 = true;
    expect("25b", in, Family::Workgroup, 2, 31, kBlock128);
    in.shadow16 = false;
    expect("25c", in, Family::Workgroup, 1, 21, kBlock128);
  }
  {  // 26: more than a quarter of the queries uncertified: the tier that ran is dropped
    row = "26";
    for (int tier = 0; tier <= 3; ++tier) {
      TierState st;
      fused_after_batch(st, tier, 64, 16, 0);  // a quarter exactly: nothing
      CHECK(!st.pre8_off && !st.pre16_off && !st.prefilter_off && st.kp8_boost == 1.0);
      fused_after_batch(st, tier, 64, 17, 0);
      CHECK(st.pre8_off == (tier == 3) && st.pre16_off == (tier == 2) && st.prefilter_off == (tier == 1));
      CHECK(st.kp8_boost == 1.0);
    }
    // 27, 28: more than an eighth retried on the int8 tier: the boost x 1.5, until it has reached 4
    row = "27";
    TierState st;
    fused_after_batch(st, 3, 64, 0, 8);
    CHECK(st.kp8_boost == 1.0);
    fused_after_batch(st, 2, 64, 0, 9);
    CHECK(st.kp8_boost == 1.0);
    fused_after_batch(st, 3, 64, 0, 9);
    CHECK(st.kp8_boost == 1.5 && !st.pre8_off);
    row = "28";
    st.kp8_boost = 3.375;
    fused_after_batch(st, 3, 64, 0, 64);
    CHECK(st.kp8_boost == 5.0625);
    fused_after_batch(st, 3, 64, 0, 64);
    CHECK(st.kp8_boost == 5.0625);
    st.kp8_boost = 4.0;
    fused_after_batch(st, 3, 64, 0, 64);
    CHECK(st.kp8_boost == 4.0);
  }
  {  // 29-33: the shapes of tests/test_gpu_knn_tier_bounds.py reach the kernel and the tier they are meant for
    row = "29-33";
    // sweeps: n = 6397, L = 6, minLeaf 100 -> leaves of 100; the shadows are those the call's own walk builds
    auto sweep = [](int T, int d, int k) {
      FusedIn in;
      in.d = d;
      in.k = k;
      in.T = T;
      in.L = 6;
      in.min_leaf = 100;
      in.n = 6397;
      return in;
    };
    auto walked = [](FusedIn in) {  // rows that are not a multiple of 16 elements get no int8 shadow
      unsigned st[8];
      walk_shadows(in, in.d % 16 ? kShadow8 : 0u, st);
      for (unsigned i = 0; i < 8; ++i) {
        const unsigned got = st[i] & ~(in.d % 16 ? kShadow8 : 0u);
        if (got & kShadow8) in.shadow8 = true;
        if (got & kShadow32) in.shadow32 = true;
        if (got & kShadow16) in.shadow16 = true;
        if (got & kShadowCsr32) in.shadow32 = in.shadow_col16 = true;
        if (got & kShadowEll) in.shadow_ell = true;
      }
      return in;
    };
    auto block = [](int d, size_t acc) { return (size_t)(2048 * 16 + 512 * 12 + 8192 + 232 * 16 + 64) + (size_t)d * (acc + 4); };
    CHECK(fused_plan(sweep(12, 16, 10)).est_cand == 1200);
    // 29: the workgroup kernel (12 x 100 candidates would be the shard kernels': knn_wave = 0)
    FusedIn in = sweep(12, 16, 10);
    in.knn_wave = 0;
    in.knn_no_pre16 = true;
    expect("29a", walked(in), Family::Workgroup, 1, 17, block(16, 8));
    in = sweep(12, 208, 24);
    in.knn_wave = 0;
    in.knn_no_pre8 = true;
    expect("29b", walked(in), Family::Workgroup, 2, 37, block(208, 8));
    in.knn_no_pre8 = false;  // int8: margin 48 sqrt(208 / 128) = 61
    expect("29c", walked(in), Family::Workgroup, 3, 86, block(208, 8));
    in = sweep(12, 208, 1);
    in.knn_wave = 0;
    in.elem = in.proj = Elem::F32;
    in.knn_no_pre8 = true;
    expect("29d", walked(in), Family::Workgroup, 2, 10, block(208, 4));
    // 30: the one-wave kernel: 6 x 100, knn_wave = 1 and knn_shard_old = 1
    in = sweep(6, 37, 10);
    in.knn_wave = 1;
    in.knn_shard_old = true;
    in.knn_no_pre8 = true;  // (d = 37: no int8 shadow either way)
    expect("30a", walked(in), Family::Wave, 2, 19, 4 * 10816);  // 512 * 12 + 128 * 24 + 72 * 16 + 37 * 12 = 10812
    in.knn_no_pre8 = false;
    in.knn_no_pre16 = true;
    expect("30b", walked(in), Family::Wave, 1, 17, 4 * 10816);
    in = sweep(6, 128, 24);
    in.knn_wave = 1;
    in.knn_shard_old = true;
    expect("30c", walked(in), Family::Wave, 3, 48, kWave128);
    // 31: the shard kernels: 4 x 100 is one batch, 8 x 100 several
    in = sweep(4, 128, 1);
    in.knn_no_pre16 = true;
    expect("31a", walked(in), Family::Shard, 1, 8, kShardOne128);
    CHECK(fused_plan(walked(in)).one_batch);
    in = sweep(8, 16, 24);
    in.knn_no_pre8 = true;
    expect("31b", walked(in), Family::Shard, 2, 37, 4 * (640 * 8 + 128 * 8 + 132 * 4 + 256 * 20 + 16 + 16 * 8 + 16 * 4));
    CHECK(!fused_plan(walked(in)).one_batch);
    in = sweep(8, 208, 10);
    in.elem = in.proj = Elem::F32;
    in.knn_no_pre8 = true;
    expect("31c", walked(in), Family::Shard, 2, 19, 4 * (640 * 8 + 128 * 8 + 132 * 4 + 256 * 20 + 16 + 208 * 4 + 208 * 4));
    in = sweep(4, 37, 10);
    in.knn_no_pre8 = true;
    // (the query's 37 * 8 = 296 bytes are padded to 304: 4096 + 1024 + 528 + 2560 + 16 + 304 + 148 = 8676 -> 8688)
    expect("31d", walked(in), Family::Shard, 2, 19, 4 * 8688);
    // 32: the aligned cases: ONE tree of depth 0, every row a candidate (301 rows; 1301: several batches)
    auto leaf = [](int n, int d, int k) {
      FusedIn in;
      in.d = d;
      in.k = k;
      in.T = 1;
      in.L = 0;
      in.min_leaf = 0;
      in.n = n;
      return in;
    };
    in = leaf(301, 16, 10);
    in.knn_no_pre16 = true;
    CHECK(fused_plan(in).est_cand == 301);
    expect("32a", walked(in), Family::Shard, 1, 17, 4 * (512 * 8 + 128 * 8 + 132 * 4 + 128 * 20 + 16 + 16 * 8 + 16 * 4));
    CHECK(fused_plan(walked(in)).one_batch);
    in.knn_wave = 0;
    expect("32b", walked(in), Family::Workgroup, 1, 17, block(16, 8));
    in.knn_wave = 1;
    in.knn_shard_old = true;
    expect("32c", walked(in), Family::Wave, 1, 17, 4 * (512 * 12 + 128 * 24 + 72 * 16 + 16 * 12));
    in = leaf(1301, 128, 24);
    in.knn_no_pre8 = true;
    expect("32d", walked(in), Family::Shard, 2, 37, kShardTwo128);
    CHECK(!fused_plan(walked(in)).one_batch);
    in = leaf(301, 37, 1);
    in.elem = in.proj = Elem::F32;
    in.knn_wave = 0;
    expect("32e", walked(in), Family::Workgroup, 2, 10, block(37, 4));
    // 33: SVector rows: the workgroup kernel whatever the shape; the half table by default, the (u16, f32)
    // shadow under knn_csr_pre32 + knn_no_pre16
    in = leaf(301, 64, 10);
    in.csr = true;
    expect("33a", walked(in), Family::Workgroup, 2, 19, block(64, 8));
    CHECK(fused_plan(walked(in)).csr_rank == CsrRank::Ell);
    in.knn_csr_pre32 = in.knn_no_pre16 = true;
    expect("33b", walked(in), Family::Workgroup, 1, 17, block(64, 8));
    CHECK(fused_plan(walked(in)).csr_rank == CsrRank::Shadow32);
    in = sweep(12, 64, 24);
    in.csr = true;
    expect("33c", walked(in), Family::Workgroup, 2, 37, block(64, 8));
    in.knn_csr_pre32 = in.knn_no_pre16 = true;
    expect("33d", walked(in), Family::Workgroup, 1, 37, block(64, 8));
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("knn_plan: all rows hold\n");
  return 0;
}
