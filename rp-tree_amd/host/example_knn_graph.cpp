// kNN graph of a data set through the C++ host mirror.  Reads dense f64 rows from the file named
// by argv[1] (int64 n, int64 d, X[n][d] double), builds a forest (argv[2] trees, minLeaf argv[3]),
// takes its kNN graph for k = argv[4] — once from the whole forest, once by accumulating the trees
// one at a time in reverse order, which must give the same arrays — and writes to argv[5]: int32 T,
// int32 L, the dense-ified hyperplanes R[T][L][d] double, ids[n][k] int32, dist[n][k] double,
// count[n] int32.  Prints the first rows and "ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "rptree.hpp"
using namespace rptree;

int main(int argc, char** argv) {
  if (argc < 6) return std::printf("usage: %s data.bin ntrees minleaf k out.bin\n", argv[0]), 2;
  const int ntrees = std::atoi(argv[2]), minLeaf = std::atoi(argv[3]), k = std::atoi(argv[4]);
  FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return std::printf("FAIL cannot open %s\n", argv[1]), 2;
  int64_t n = 0, d = 0;
  bool ok = std::fread(&n, 8, 1, fp) == 1 && std::fread(&d, 8, 1, fp) == 1 && n > 0 && d > 0;
  std::vector<DVector> xs((size_t)(ok ? n : 0), DVector{std::vector<double>((size_t)(ok ? d : 0))});
  for (int64_t i = 0; ok && i < n; ++i)
    ok = std::fread(xs[(size_t)i].dvVec.data(), 8, (size_t)d, fp) == (size_t)d;
  std::fclose(fp);
  if (!ok) return std::printf("FAIL short file\n"), 2;
  try {
    Context ctx(0);
    Dataset dats(ctx, xs);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, (int)d);
    const int L = cfg.fpMaxTreeDepth;
    RPForest tts = forestBatch(ctx, 7, L, minLeaf, ntrees, cfg.fpProjNzDensity, (int)d, dats);
    const GraphResult g = knnGraph(tts, k);

    // the same graph from one-tree forests folded in, last tree first
    GraphResult acc;
    for (int t = ntrees - 1; t >= 0; --t) {
      RPForest one(ctx, dats, {tts.rpVectors[(size_t)t]}, L, minLeaf);
      acc = knnGraph(one, k, t == ntrees - 1 ? nullptr : &acc);
    }
    if (acc.ids != g.ids || acc.dist != g.dist || acc.count != g.count)
      return std::printf("FAIL accumulating the trees one by one gives another graph\n"), 1;

    for (int64_t i = 0; i < n && i < 3; ++i) {
      std::printf("row %" PRId64 " (%d):", i, g.count[(size_t)i]);
      for (int j = 0; j < g.count[(size_t)i]; ++j)
        std::printf(" %d:%.6g", g.ids[(size_t)i * k + j], g.dist[(size_t)i * k + j]);
      std::printf("\n");
    }
    std::vector<double> R((size_t)ntrees * L * d, 0.0);
    for (int t = 0; t < ntrees; ++t)
      for (int l = 0; l < L; ++l)
        for (auto& iv : tts.rpVectors[(size_t)t][(size_t)l].svVec)
          R[((size_t)t * L + l) * d + (size_t)iv.first] = iv.second;
    FILE* out = std::fopen(argv[5], "wb");
    if (!out) return std::printf("FAIL cannot write %s\n", argv[5]), 2;
    const int32_t hdr[2] = {ntrees, L};
    std::fwrite(hdr, 4, 2, out);
    std::fwrite(R.data(), 8, R.size(), out);
    std::fwrite(g.ids.data(), 4, g.ids.size(), out);
    std::fwrite(g.dist.data(), 8, g.dist.size(), out);
    std::fwrite(g.count.data(), 4, g.count.size(), out);
    std::fclose(out);
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
