// Deleting rows without rebuilding anything, through the C++ host mirror: forest -> knnGraph ->
// knnGraphRefine -> graphPrepare once, then a tombstone bitmap and graphSearchAllow.  Reads dense f64
// rows from the file named by argv[1] (int64 n, int64 d, X[n][d] double) and queries of the same
// layout from argv[2], builds a forest (argv[3] trees, minLeaf argv[4]) and its kNN graph for kg =
// argv[5] refined by one NN-descent round and prepared, deletes every argv[9]-th row (row i with
// i % argv[9] == 0; 0 deletes nothing) and searches for k = argv[6] with ef = argv[7] allowed beam
// entries and a frontier of width = argv[8] from the forest's 8 nearest candidates per query, deleted
// or not.  Checks that no deleted row is answered, that every distance is the surviving row's, that
// with nothing deleted and with no bitmap at all the answer is graphSearch's bit for bit, and prints
// the statistics, recall@k against the exhaustive answer among the surviving rows and "ok".
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

static bool same_bits(const KnnResult& a, const KnnResult& b) {
  return a.ids == b.ids && a.count == b.count && a.dist.size() == b.dist.size() &&
         std::memcmp(a.dist.data(), b.dist.data(), 8 * a.dist.size()) == 0;
}

// the left fold of the library: every operation rounded on its own
static double l2(const DVector& a, const DVector& b) {
  double acc = 0.0;
  for (size_t c = 0; c < a.dvVec.size(); ++c) {
    volatile double t = a.dvVec[c] - b.dvVec[c];
    volatile double sq = t * t;
    acc = acc + sq;
  }
  return std::sqrt(acc);
}

int main(int argc, char** argv) {
  if (argc < 10) return std::printf("usage: %s data.bin queries.bin ntrees minleaf kg k ef width every\n", argv[0]), 2;
  const int ntrees = std::atoi(argv[3]), minLeaf = std::atoi(argv[4]), kg = std::atoi(argv[5]);
  const int k = std::atoi(argv[6]), ef = std::atoi(argv[7]), width = std::atoi(argv[8]), every = std::atoi(argv[9]);
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
    g = knnGraphRefine(ctx, dats, g, 1);
    const GraphResult sg = graphPrepare(ctx, dats, g, 2 * kg);
    // nothing deleted: graphSearch's bits, with every bit set and with no bitmap at all
    const KnnResult plain = graphSearch(tts, sg, qs, k, ef);
    std::vector<bool> alive((size_t)n, true);
    if (!same_bits(plain, graphSearchAllow(tts, sg, qs, allowBitmap(alive), k, ef, width)))
      return std::printf("FAIL an all-ones bitmap gives another answer than graphSearch\n"), 1;
    if (!same_bits(plain, graphSearchAllow(tts, sg, qs, {}, k, ef, width)))
      return std::printf("FAIL no bitmap gives another answer than graphSearch\n"), 1;
    // the tombstones
    int64_t deleted = 0;
    for (int64_t i = 0; every > 0 && i < n; i += every) alive[(size_t)i] = false, ++deleted;
    SearchStats st;
    const KnnResult got = graphSearchAllow(tts, sg, qs, allowBitmap(alive), k, ef, width, Metric::L2, 8, &st);
    int64_t hits = 0, want = 0;
    for (int64_t i = 0; i < nq; ++i) {
      std::vector<std::pair<double, int32_t>> all;
      for (int64_t j = 0; j < n; ++j)
        if (alive[(size_t)j]) all.emplace_back(l2(qv[(size_t)i], xs[(size_t)j]), (int32_t)j);
      const size_t top = std::min<size_t>((size_t)k, all.size());
      std::partial_sort(all.begin(), all.begin() + (long)top, all.end());
      want += (int64_t)top;
      for (int b = 0; b < got.count[(size_t)i]; ++b) {
        const int32_t id = got.ids[(size_t)i * k + b];
        const double db = got.dist[(size_t)i * k + b];
        if (id < 0 || id >= n || !alive[(size_t)id]) return std::printf("FAIL query %" PRId64 " answers a deleted row\n", i), 1;
        const double fold = l2(qv[(size_t)i], xs[(size_t)id]);
        if (std::memcmp(&fold, &db, 8) != 0) return std::printf("FAIL query %" PRId64 ": not the row's distance\n", i), 1;
        if (b > 0 && db < got.dist[(size_t)i * k + b - 1]) return std::printf("FAIL query %" PRId64 " is not sorted\n", i), 1;
        for (size_t a = 0; a < top; ++a) hits += all[a].second == id;
      }
    }
    std::printf("deleted %" PRId64 " of %" PRId64 " rows\n", deleted, n);
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
