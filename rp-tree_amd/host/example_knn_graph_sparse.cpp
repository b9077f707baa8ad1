// The kNN graph of SVector rows and its refinement through the C++ host mirror.  Draws argv[1]
// sparse rows of dimension argv[2] with nonzero density argv[3], builds a forest (argv[4] trees,
// minLeaf argv[5]), takes the kNN graph for k = argv[6] with knnGraphSV and applies argv[7]
// NN-descent rounds with knnGraphRefineSV.  Every distance of both graphs is then folded again on
// the host over the union of the two rows' supports (metricDDL2's left fold, absent entries +0.0)
// and must agree bit for bit.  Prints the statistics and "ok".
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

static int64_t check_graph(const std::vector<SVector>& xs, const GraphResult& g) {
  int64_t bad = 0;
  for (size_t i = 0; i < xs.size(); ++i)
    for (int s = 0; s < g.count[i]; ++s) {
      const double want = unionFold(xs[i], xs[(size_t)g.ids[i * (size_t)g.k + (size_t)s]]);
      bad += std::memcmp(&want, &g.dist[i * (size_t)g.k + (size_t)s], 8) != 0;
    }
  return bad;
}

int main(int argc, char** argv) {
  if (argc < 8) return std::printf("usage: %s n d density ntrees minleaf k iters\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]);
  const int d = std::atoi(argv[2]);
  const double density = std::atof(argv[3]);
  const int ntrees = std::atoi(argv[4]), minLeaf = std::atoi(argv[5]), k = std::atoi(argv[6]);
  const int iters = std::atoi(argv[7]);
  try {
    SMGen gen(2024);
    std::vector<SVector> xs;
    for (int64_t i = 0; i < n; ++i) xs.push_back(sparse(gen, density, d));
    Context ctx(0);
    Dataset dats(ctx, xs, d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, d, dats);
    const GraphResult g = knnGraphSV(tts, k);
    RefineStats st;
    const GraphResult refined = knnGraphRefineSV(ctx, dats, g, iters, -1, &st);
    const int64_t bad = check_graph(xs, g) + check_graph(xs, refined);
    if (bad) return std::printf("FAIL %" PRId64 " distances differ from the host fold\n", bad), 1;
    std::printf("rounds %" PRId64 " updates %" PRId64 " candidates %" PRId64 "\n", st.rounds, st.updates,
                st.candidates);
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
