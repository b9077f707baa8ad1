// Preparing the kNN graph for the search through the C++ host mirror: forest -> knnGraph ->
// knnGraphRefine -> graphPrepare -> graphSearch -> recall against bruteKnn, on the raw and on the
// prepared graph.  Reads dense f64 rows from the file named by argv[1] (int64 n, int64 d, X[n][d]
// double) and queries of the same layout from argv[2], builds a forest (argv[3] trees, minLeaf
// argv[4]), its kNN graph for kg = argv[5] refined by argv[6] NN-descent rounds, prepares it
// (diversify + reverse union, degree <= argv[7]) and searches both graphs for k = argv[8] with a beam
// of ef = argv[9] from the forest's 8 nearest candidates per query.  Prints the statistics of the
// preparation, both recalls and "ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "rptree.hpp"
using namespace rptree;

static bool read_rows(const char* path, std::vector<DVector>& xs, int64_t& n, int64_t& d) {
  FILE* fp = std::fopen(path, "rb");
  if (!fp) return false;
  bool ok = std::fread(&n, 8, 1, fp) == 1 && std::fread(&d, 8, 1, fp) == 1 && n > 0 && d > 0;
  xs.assign((size_t)(ok ? n : 0), DVector{std::vector<double>((size_t)(ok ? d : 0))});
  for (int64_t i = 0; ok && i < n; ++i) ok = std::fread(xs[(size_t)i].dvVec.data(), 8, (size_t)d, fp) == (size_t)d;
  std::fclose(fp);
  return ok;
}

static double recall(const KnnResult& got, const BruteResult& truth, int64_t nq, int k) {
  int64_t hits = 0, want = 0;
  for (int64_t i = 0; i < nq; ++i)
    for (int a = 0; a < k; ++a) {
      const int32_t t = truth.ids[(size_t)i * k + a];
      if (t < 0) continue;
      ++want;
      for (int b = 0; b < got.count[(size_t)i]; ++b) hits += got.ids[(size_t)i * k + b] == t;
    }
  return want ? (double)hits / (double)want : 1.0;
}

int main(int argc, char** argv) {
  if (argc < 10) return std::printf("usage: %s data.bin queries.bin ntrees minleaf kg iters kout k ef\n", argv[0]), 2;
  const int ntrees = std::atoi(argv[3]), minLeaf = std::atoi(argv[4]), kg = std::atoi(argv[5]);
  const int iters = std::atoi(argv[6]), kout = std::atoi(argv[7]), k = std::atoi(argv[8]), ef = std::atoi(argv[9]);
  std::vector<DVector> xs, qv;
  int64_t n = 0, d = 0, nq = 0, dq = 0;
  if (!read_rows(argv[1], xs, n, d)) return std::printf("FAIL cannot read %s\n", argv[1]), 2;
  if (!read_rows(argv[2], qv, nq, dq) || dq != d) return std::printf("FAIL cannot read %s\n", argv[2]), 2;
  try {
    Context ctx(0);
    Dataset dats(ctx, xs), qs(ctx, qv);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, (int)d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, (int)d, dats);
    GraphResult g = knnGraph(tts, kg);
    if (iters > 0) g = knnGraphRefine(ctx, dats, g, iters);
    PrepareStats ps;
    const GraphResult sg = graphPrepare(ctx, dats, g, kout, true, true, &ps);
    // the prepared graph: rows sorted by (distance, id), within the cap, and symmetric where no row was cut
    int64_t edges = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int c = sg.count[(size_t)i];
      if (c < 0 || c > kout) return std::printf("FAIL row %" PRId64 ": count %d\n", i, c), 1;
      edges += c;
      for (int b = 1; b < c; ++b)
        if (sg.dist[(size_t)i * kout + b] < sg.dist[(size_t)i * kout + b - 1])
          return std::printf("FAIL row %" PRId64 " is not sorted\n", i), 1;
    }
    if (ps.capped == 0)
      for (int64_t i = 0; i < n; ++i)
        for (int b = 0; b < sg.count[(size_t)i]; ++b) {
          const int32_t j = sg.ids[(size_t)i * kout + b];
          bool back = false;
          for (int a = 0; a < sg.count[(size_t)j]; ++a) back = back || sg.ids[(size_t)j * kout + a] == i;
          if (!back) return std::printf("FAIL edge %" PRId64 " -> %d has no reverse\n", i, j), 1;
        }
    const BruteResult truth = bruteKnn(ctx, dats, qs, k);
    const KnnResult raw = graphSearch(tts, g, qs, k, ef), got = graphSearch(tts, sg, qs, k, ef);
    std::printf("pairs %" PRId64 " occluded %" PRId64 " capped %" PRId64 " (mean degree %.2f)\n", ps.pairs, ps.occluded,
                ps.capped, n ? (double)edges / (double)n : 0.0);
    std::printf("recall@%d raw %.4f prepared %.4f\n", k, recall(raw, truth, nq, k), recall(got, truth, nq, k));
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
