// The vote threshold on SVector rows through the C++ host mirror.  Draws argv[1] sparse rows of
// dimension argv[2] with nonzero density argv[3], builds a forest (argv[4] trees, minLeaf argv[5])
// and, for a stored row and a fresh one, takes voteCandidates and knnVote (k = argv[6], v = argv[7])
// under the inner-product distance.  The voted list must be the ids that at least v of the trees'
// candidate lists hold, ascending, with their counts; every knnVote entry must be a voted id whose
// distance is the host's left fold over the indices both vectors store, bit for bit, in (distance,
// id) order.  Prints the list sizes and "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

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
  if (argc < 8) return std::printf("usage: %s n d density ntrees minleaf k v\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]);
  const int d = std::atoi(argv[2]);
  const double density = std::atof(argv[3]);
  const int ntrees = std::atoi(argv[4]), minLeaf = std::atoi(argv[5]), k = std::atoi(argv[6]), v = std::atoi(argv[7]);
  try {
    SMGen gen(2025);
    std::vector<SVector> xs;
    for (int64_t i = 0; i < n; ++i) xs.push_back(sparse(gen, density, d));
    const std::vector<SVector> queries{xs[3], sparse(gen, density, d)};
    Context ctx(0);
    Dataset dats(ctx, xs, d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, d, dats);
    int64_t bad = 0;
    for (size_t qi = 0; qi < queries.size(); ++qi) {
      std::map<int32_t, int32_t> count;
      for (int t = 0; t < ntrees; ++t)
        for (int32_t c : candidates(tts, t, queries[qi])) ++count[c];
      std::vector<std::pair<int32_t, int32_t>> want;
      for (const auto& e : count)
        if (e.second >= v) want.push_back(e);
      const auto got = voteCandidates(tts, v, queries[qi]);
      bad += got != want;
      const auto nn = knnVote(tts, k, v, queries[qi], Metric::Inner);
      bad += nn.size() != std::min(want.size(), (size_t)k);
      for (size_t s = 0; s < nn.size(); ++s) {
        bad += !count.count(nn[s].second) || count[nn[s].second] < v;
        bad += !sameBits(nn[s].first, -dotS(xs[(size_t)nn[s].second], queries[qi]));
        if (s > 0)
          bad += nn[s].first < nn[s - 1].first || (nn[s].first == nn[s - 1].first && nn[s].second <= nn[s - 1].second);
      }
      std::printf("query %zu: %zu candidates ids, %zu with %d votes, %zu returned\n", qi, count.size(), want.size(), v,
                  nn.size());
    }
    if (bad) return std::printf("FAIL %lld checks\n", (long long)bad), 1;
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
