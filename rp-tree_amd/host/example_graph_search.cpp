// Answering queries with the kNN graph through the C++ host mirror: forest -> knnGraph ->
// knnGraphRefine -> graphSearch -> recall against bruteKnn.  Reads dense f64 rows from the file named
// by argv[1] (int64 n, int64 d, X[n][d] double) and queries of the same layout from argv[2], builds a
// forest (argv[3] trees, minLeaf argv[4]), its kNN graph for kg = argv[5] refined by argv[6]
// NN-descent rounds, then searches it for k = argv[7] with a beam of ef = argv[8] from the forest's
// 8 nearest candidates per query.  Prints the statistics of the search, recall@k against the
// exhaustive answer and "ok".
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

int main(int argc, char** argv) {
  if (argc < 9) return std::printf("usage: %s data.bin queries.bin ntrees minleaf kg iters k ef\n", argv[0]), 2;
  const int ntrees = std::atoi(argv[3]), minLeaf = std::atoi(argv[4]), kg = std::atoi(argv[5]);
  const int iters = std::atoi(argv[6]), k = std::atoi(argv[7]), ef = std::atoi(argv[8]);
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
    SearchStats st;
    const KnnResult got = graphSearch(tts, g, qs, k, ef, Metric::L2, 8, &st);
    const BruteResult truth = bruteKnn(ctx, dats, qs, k);
    int64_t hits = 0, want = 0;
    for (int64_t i = 0; i < nq; ++i)
      for (int a = 0; a < k; ++a) {
        const int32_t t = truth.ids[(size_t)i * k + a];
        if (t < 0) continue;
        ++want;
        for (int b = 0; b < got.count[(size_t)i]; ++b) hits += got.ids[(size_t)i * k + b] == t;
      }
    // the answer is sorted by (distance, id) and never beats the exhaustive one
    for (int64_t i = 0; i < nq; ++i)
      for (int b = 0; b < got.count[(size_t)i]; ++b) {
        const double db = got.dist[(size_t)i * k + b];
        if (b > 0 && db < got.dist[(size_t)i * k + b - 1]) return std::printf("FAIL query %" PRId64 " is not sorted\n", i), 1;
        if (db < truth.dist[(size_t)i * k + b]) return std::printf("FAIL query %" PRId64 " beats brute force\n", i), 1;
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
