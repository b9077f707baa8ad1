// Answering queries with the kNN graph of SVector rows through the C++ host mirror: forest ->
// knnGraphSV -> knnGraphRefineSV -> graphSearchSV.  Draws argv[1] sparse rows and argv[2] sparse
// queries of dimension argv[3] with nonzero density argv[4], builds a forest (argv[5] trees, minLeaf
// argv[6]), its kNN graph for kg = argv[7] refined by argv[8] NN-descent rounds, then searches it
// for k = argv[9] with a beam of ef = argv[10] from the forest's 8 nearest candidates per query.
// Every distance of the answer is folded again on the host over the union of the two supports
// (metricDDL2's left fold, absent entries +0.0) and must agree bit for bit.  Prints the first
// query's answer, the statistics of the search, recall@k against the exhaustive answer and "ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rptree.hpp"
using namespace rptree;

static double unionFold(const SVector& a, const SVector& b) {
  size_t i = 0, j = 0;
  double acc = 0.0;
  while (i < a.svVec.size() || j < b.svVec.size()) {
    const int ci = i < a.svVec.size() ? a.svVec[i].first : a.svDim;
    const int cj = j < b.svVec.size() ? b.svVec[j].first : b.svDim;
    const double x = ci <= cj ? a.svVec[i].second : 0.0, y = cj <= ci ? b.svVec[j].second : 0.0;
    volatile double t = x - y;  // every difference, square and sum rounded on its own: no contraction
    volatile double sq = t * t;
    acc = acc + sq;
    if (ci <= cj) ++i;
    if (cj <= ci) ++j;
  }
  return std::sqrt(acc);
}

int main(int argc, char** argv) {
  if (argc < 11) return std::printf("usage: %s n nq d density ntrees minleaf kg iters k ef\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]), nq = std::atoll(argv[2]);
  const int d = std::atoi(argv[3]);
  const double density = std::atof(argv[4]);
  const int ntrees = std::atoi(argv[5]), minLeaf = std::atoi(argv[6]), kg = std::atoi(argv[7]);
  const int iters = std::atoi(argv[8]), k = std::atoi(argv[9]), ef = std::atoi(argv[10]);
  try {
    SMGen gen(2025);
    std::vector<SVector> xs, qv;
    for (int64_t i = 0; i < n; ++i) xs.push_back(sparse(gen, density, d));
    for (int64_t i = 0; i < nq; ++i) qv.push_back(sparse(gen, density, d));
    Context ctx(0);
    Dataset dats(ctx, xs, d), qs(ctx, qv, d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, d, dats);
    GraphResult g = knnGraphSV(tts, kg);
    if (iters > 0) g = knnGraphRefineSV(ctx, dats, g, iters);
    SearchStats st;
    const KnnResult got = graphSearchSV(tts, g, qs, k, ef, 8, &st);
    const BruteResult truth = bruteKnn(ctx, dats, qs, k);
    int64_t hits = 0, want = 0, bad = 0;
    for (int64_t i = 0; i < nq; ++i) {
      for (int a = 0; a < k; ++a) {
        const int32_t t = truth.ids[(size_t)i * k + a];
        if (t < 0) continue;
        ++want;
        for (int b = 0; b < got.count[(size_t)i]; ++b) hits += got.ids[(size_t)i * k + b] == t;
      }
      for (int b = 0; b < got.count[(size_t)i]; ++b) {
        const double db = got.dist[(size_t)i * k + b];
        const double fold = unionFold(qv[(size_t)i], xs[(size_t)got.ids[(size_t)i * k + b]]);
        bad += std::memcmp(&fold, &db, 8) != 0;
        if (b > 0 && db < got.dist[(size_t)i * k + b - 1]) return std::printf("FAIL query %" PRId64 " is not sorted\n", i), 1;
      }
    }
    if (bad) return std::printf("FAIL %" PRId64 " distances differ from the host fold\n", bad), 1;
    if (nq > 0) {
      std::printf("query 0:");
      for (int b = 0; b < got.count[0]; ++b) std::printf(" %d (%.6f)", got.ids[(size_t)b], got.dist[(size_t)b]);
      std::printf("\n");
    }
    std::printf("expansions %" PRId64 " evaluated %" PRId64 " (%.1f distances per query)\n", st.expansions,
                st.evaluated, nq ? (double)st.evaluated / (double)nq : 0.0);
    std::printf("recall@%d %.4f\n", k, want ? (double)hits / (double)want : 1.0);
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
