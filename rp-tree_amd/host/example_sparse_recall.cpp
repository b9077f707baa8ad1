// recallWith on SVector data through the C++ host mirror.  Reads a CSR f64 dataset and one query
// from the file named by argv[1] (int64 n, int32 d, int64 nnz, rowptr[n + 1] int64, col[nnz] int32,
// val[nnz] double; then int32 qnz, qcol[qnz] int32, qval[qnz] double), builds a forest (argv[2]
// trees, minLeaf argv[3]) and prints every tree's candidates, the k = argv[4] true neighbours, the
// per-tree hits, the recall's bits — under the true Euclidean distance and under the reference's
// truncating metricSSL2 — and "ok".
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
  int64_t n = 0, nnz = 0;
  int32_t d = 0, qnz = 0;
  bool ok = std::fread(&n, 8, 1, fp) == 1 && std::fread(&d, 4, 1, fp) == 1 &&
            std::fread(&nnz, 8, 1, fp) == 1 && n > 0 && d > 0 && nnz >= 0;
  std::vector<int64_t> rowptr((size_t)(ok ? n + 1 : 1));
  std::vector<int32_t> col((size_t)(ok ? nnz : 0) + 1);
  std::vector<double> val((size_t)(ok ? nnz : 0) + 1);
  ok = ok && std::fread(rowptr.data(), 8, (size_t)n + 1, fp) == (size_t)n + 1 &&
       std::fread(col.data(), 4, (size_t)nnz, fp) == (size_t)nnz &&
       std::fread(val.data(), 8, (size_t)nnz, fp) == (size_t)nnz && std::fread(&qnz, 4, 1, fp) == 1 && qnz >= 0;
  std::vector<int32_t> qcol((size_t)(ok ? qnz : 0) + 1);
  std::vector<double> qval((size_t)(ok ? qnz : 0) + 1);
  ok = ok && std::fread(qcol.data(), 4, (size_t)qnz, fp) == (size_t)qnz &&
       std::fread(qval.data(), 8, (size_t)qnz, fp) == (size_t)qnz;
  std::fclose(fp);
  if (!ok) return std::printf("FAIL short file\n"), 2;
  std::vector<SVector> xs((size_t)n, SVector{d, {}});
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = rowptr[(size_t)i]; j < rowptr[(size_t)i + 1]; ++j)
      xs[(size_t)i].svVec.push_back({col[(size_t)j], val[(size_t)j]});
  SVector q{d, {}};
  for (int j = 0; j < qnz; ++j) q.svVec.push_back({qcol[(size_t)j], qval[(size_t)j]});
  try {
    Context ctx(0);
    Dataset dats(ctx, xs, d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, d, dats);
    for (int t = 0; t < ntrees; ++t) {
      std::printf("cand %d:", t);
      for (int32_t id : candidates(tts, t, q)) std::printf(" %d", id);
      std::printf("\n");
    }
    std::vector<SVector> qv{q};
    Dataset qs(ctx, qv, d);
    for (int ref = 0; ref < 2; ++ref) {
      const int32_t flags = ref ? RPT_KNN_METRIC_REFERENCE : 0;
      std::vector<int32_t> truth;
      const std::vector<int32_t> hits = recallHits(tts, k, qs, flags, &truth);
      const BruteResult br = bruteKnn(ctx, dats, qs, k, flags);
      if (br.ids != truth) return std::printf("FAIL bruteKnn and recallHits disagree on the truth\n"), 1;
      std::printf("truth %d:", ref);
      for (int32_t id : truth) std::printf(" %d", id);
      std::printf("\nhits %d:", ref);
      for (int32_t h : hits) std::printf(" %d", h);
      const double r = recallWith(tts, k, q, ref != 0);
      uint64_t bits;
      std::memcpy(&bits, &r, 8);
      std::printf("\nrecall %d: %016" PRIx64 "\n", ref, bits);
    }
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
