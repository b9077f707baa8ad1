// One tenant's rows through the C++ host mirror: an allow-list on the forest query and on the
// exhaustive kNN.  Draws argv[1] sparse rows of dimension argv[2] with nonzero density argv[3], builds
// a forest (argv[4] trees, minLeaf argv[5]) and allows every argv[7]-th row.  For a stored row and a
// fresh one it takes allowCandidates, knnAllow (k = argv[6], each id once, the inner-product distance),
// bruteKnnAllow and recallHitsAllow.  The allowed list must be the trees' candidate lists in order
// without the disallowed ids; every knnAllow entry must be an allowed candidate whose distance is the
// host's left fold over the indices both vectors store, bit for bit, in (distance, position) order;
// the exhaustive answer must be the host's (distance, id) order over the allowed rows; the hits must
// be the trees' candidates found in that truth.  Prints the list sizes and "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "rptree.hpp"
using namespace rptree;

static double dotS(const SVector& a, const SVector& b) {
  size_t i = 0, j = 0;
  double acc = 0.0;
  while (i < a.svVec.size() && j < b.svVec.size()) {
    if (a.svVec[i].first == b.svVec[j].first) {
      volatile double p = a.svVec[i].second * b.svVec[j].second;  // rounded on its own: no contraction
      acc = acc + p;
      ++i;
      ++j;
    } else if (a.svVec[i].first < b.svVec[j].first) {
      ++i;
    } else {
      ++j;
    }
  }
  return acc;
}

static bool sameBits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

int main(int argc, char** argv) {
  if (argc < 8) return std::printf("usage: %s n d density ntrees minleaf k every\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]);
  const int d = std::atoi(argv[2]);
  const double density = std::atof(argv[3]);
  const int ntrees = std::atoi(argv[4]), minLeaf = std::atoi(argv[5]), k = std::atoi(argv[6]);
  const int every = std::atoi(argv[7]);
  try {
    SMGen gen(2026);
    std::vector<SVector> xs;
    for (int64_t i = 0; i < n; ++i) xs.push_back(sparse(gen, density, d));
    const std::vector<SVector> queries{xs[3], sparse(gen, density, d)};
    std::vector<bool> mask((size_t)n);
    for (int64_t i = 0; i < n; ++i) mask[(size_t)i] = i % every == 0;
    const std::vector<uint32_t> allow = allowBitmap(mask);
    Context ctx(0);
    Dataset dats(ctx, xs, d);
    Dataset qs(ctx, queries, d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, d, dats);
    std::vector<int64_t> off;
    const std::vector<int32_t> lists = allowCandidates(tts, allow, qs, &off);
    const KnnResult nn = knnAllow(tts, allow, k, qs, RPT_KNN_DEDUP, Metric::Inner);
    const BruteResult truth = bruteKnnAllow(ctx, dats, allow, qs, k, Metric::Inner);
    std::vector<int32_t> tids;
    const std::vector<int32_t> hits = recallHitsAllow(tts, allow, k, qs, Metric::Inner, 0, &tids);
    int64_t bad = 0;
    for (size_t qi = 0; qi < queries.size(); ++qi) {
      std::vector<int32_t> want;  // the allowed list
      std::vector<std::set<int32_t>> per_tree((size_t)ntrees);
      for (int t = 0; t < ntrees; ++t)
        for (int32_t c : candidates(tts, t, queries[qi])) {
          per_tree[(size_t)t].insert(c);
          if (mask[(size_t)c]) want.push_back(c);
        }
      const std::vector<int32_t> got(lists.begin() + off[qi], lists.begin() + off[qi + 1]);
      bad += got != want;
      const std::set<int32_t> distinct(want.begin(), want.end());
      const int cnt = nn.count[qi];
      bad += cnt != (int)std::min(distinct.size(), (size_t)k);
      for (int s = 0; s < cnt; ++s) {
        const int32_t id = nn.ids[qi * (size_t)k + s];
        const double dv = nn.dist[qi * (size_t)k + s];
        bad += !distinct.count(id);
        bad += !sameBits(dv, -dotS(xs[(size_t)id], queries[qi]));
        if (s > 0) bad += dv < nn.dist[qi * (size_t)k + s - 1];
      }
      // the exhaustive answer among the allowed rows: (distance, id)
      std::vector<std::pair<double, int32_t>> all;
      for (int64_t i = 0; i < n; ++i)
        if (mask[(size_t)i]) all.push_back({-dotS(xs[(size_t)i], queries[qi]), (int32_t)i});
      std::sort(all.begin(), all.end());
      for (int s = 0; s < k; ++s) {
        const bool used = (size_t)s < all.size();
        bad += truth.ids[qi * (size_t)k + s] != (used ? all[(size_t)s].second : -1);
        if (used) bad += !sameBits(truth.dist[qi * (size_t)k + s], all[(size_t)s].first);
        bad += tids[qi * (size_t)k + s] != truth.ids[qi * (size_t)k + s];
      }
      for (int t = 0; t < ntrees; ++t) {
        int h = 0;
        for (int s = 0; s < k; ++s) h += per_tree[(size_t)t].count(truth.ids[qi * (size_t)k + s]) ? 1 : 0;
        bad += hits[qi * (size_t)ntrees + t] != h;
      }
      std::printf("query %zu: %zu allowed candidate entries, %zu ids, %d returned\n", qi, want.size(),
                  distinct.size(), cnt);
    }
    if (bad) return std::printf("FAIL %lld checks\n", (long long)bad), 1;
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
