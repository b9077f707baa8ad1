// knn under the cosine distance through the C++ host mirror: `knn distf k forest q` with
// distf = Metric::Cosine.  Reads a dense f64 dataset and one query from the file named by argv[1]
// (int64 n, int32 d, n x d doubles, d doubles), builds a forest (argv[2] trees, minLeaf argv[3])
// and prints every tree's candidates, the k = argv[4] answers with their distances' bits, "ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rptree.hpp"
using namespace rptree;

int main(int argc, char** argv) {
  if (argc < 5) return std::printf("usage: %s data.bin ntrees minleaf k\n", argv[0]), 2;
  const int ntrees = std::atoi(argv[2]), minLeaf = std::atoi(argv[3]), k = std::atoi(argv[4]);
  FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return std::printf("FAIL cannot open %s\n", argv[1]), 2;
  int64_t n = 0;
  int32_t d = 0;
  bool ok = std::fread(&n, 8, 1, fp) == 1 && std::fread(&d, 4, 1, fp) == 1 && n > 0 && d > 0;
  std::vector<DVector> xs;
  std::vector<double> row((size_t)(ok ? d : 0));
  for (int64_t i = 0; ok && i < n; ++i) {
    ok = std::fread(row.data(), 8, (size_t)d, fp) == (size_t)d;
    xs.push_back(fromListDv(row));
  }
  ok = ok && std::fread(row.data(), 8, (size_t)d, fp) == (size_t)d;
  std::fclose(fp);
  if (!ok) return std::printf("FAIL short file\n"), 2;
  const DVector q = fromListDv(row);
  try {
    Context ctx(0);
    Dataset dats(ctx, xs);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, 1.0, d, dats);
    for (int t = 0; t < ntrees; ++t) {
      std::printf("cand %d:", t);
      for (int32_t id : candidates(tts, t, q)) std::printf(" %d", id);
      std::printf("\n");
    }
    auto hits = knn(tts, k, q, Metric::Cosine);
    std::printf("knn:");
    for (auto& h : hits) {
      uint64_t bits;
      std::memcpy(&bits, &h.first, 8);
      std::printf(" %d:%016" PRIx64, h.second, bits);
    }
    std::printf("\nok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
