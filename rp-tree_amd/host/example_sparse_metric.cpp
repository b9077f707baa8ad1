// Cosine and inner-product kNN on SVector rows through the C++ host mirror.  Draws argv[1] sparse
// rows of dimension argv[2] with nonzero density argv[3], builds a forest (argv[4] trees, minLeaf
// argv[5]) and, for both metrics, takes bruteKnn, knn and recallWith for k = argv[6] of a stored row
// and of a fresh one.  Every distance is folded again on the host over the indices both vectors
// store (the left fold, every product and sum rounded on its own) and must agree bit for bit; the
// brute force must be sorted by (distance, id) and every knn entry must be a candidate.  Prints the
// recalls and "ok".
#include <cmath>
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

static double distance(Metric m, const SVector& x, const SVector& q) {
  if (m == Metric::Inner) return -dotS(x, q);
  return 1.0 - dotS(x, q) / (std::sqrt(dotS(x, x)) * std::sqrt(dotS(q, q)));
}

static bool sameBits(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (a != a && b != b); }

int main(int argc, char** argv) {
  if (argc < 7) return std::printf("usage: %s n d density ntrees minleaf k\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]);
  const int d = std::atoi(argv[2]);
  const double density = std::atof(argv[3]);
  const int ntrees = std::atoi(argv[4]), minLeaf = std::atoi(argv[5]), k = std::atoi(argv[6]);
  try {
    SMGen gen(2025);
    std::vector<SVector> xs;
    for (int64_t i = 0; i < n; ++i) xs.push_back(sparse(gen, density, d));
    const std::vector<SVector> queries{xs[3], sparse(gen, density, d)};
    Context ctx(0);
    Dataset dats(ctx, xs, d);
    Dataset qs(ctx, queries, d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, d, dats);
    int64_t bad = 0;
    for (Metric m : {Metric::Cosine, Metric::Inner}) {
      const BruteResult br = bruteKnn(ctx, dats, qs, k, m);
      for (size_t qi = 0; qi < queries.size(); ++qi) {
        for (int s = 0; s < k; ++s) {
          const int32_t id = br.ids[qi * (size_t)k + (size_t)s];
          const double got = br.dist[qi * (size_t)k + (size_t)s];
          if (id < 0) continue;
          bad += !sameBits(got, distance(m, xs[(size_t)id], queries[qi]));
          if (s > 0 && br.ids[qi * (size_t)k + (size_t)s - 1] >= 0) {
            const double prev = br.dist[qi * (size_t)k + (size_t)s - 1];
            bad += got < prev || (got == prev && id < br.ids[qi * (size_t)k + (size_t)s - 1]);
          }
        }
        std::set<int32_t> cand;
        for (int t = 0; t < ntrees; ++t)
          for (int32_t c : candidates(tts, t, queries[qi])) cand.insert(c);
        for (const auto& e : knn(tts, k, queries[qi], m)) {
          bad += !cand.count(e.second);
          bad += !sameBits(e.first, distance(m, xs[(size_t)e.second], queries[qi]));
        }
        for (const auto& e : knnPQ(tts, k, queries[qi], m))
          bad += !sameBits(e.first, distance(m, xs[(size_t)e.second], queries[qi]));
        std::printf("%s query %zu recall %.4f\n", m == Metric::Cosine ? "cosine" : "inner", qi,
                    recallWith(tts, k, queries[qi], m));
      }
    }
    if (bad) return std::printf("FAIL %lld entries differ from the host fold or its order\n", (long long)bad), 1;
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
