// Growing an index without rebuilding anything, through the C++ host mirror: forest -> knnGraph ->
// knnGraphRefine over the first n rows once, then graphInsert of m further rows and graphSearch on the
// grown graph.  Draws n = argv[1] old and m = argv[2] new rows of d = argv[3] standard normal columns,
// builds a forest of 4 trees over the old rows and their 10-NN graph refined by one NN-descent round,
// inserts the new rows at ef = 32 with the forest's 8 nearest candidates as seeds in chunks of 128, and
// checks: the old part of a graph grown by nothing is the graph; every new row is sorted, names rows
// that were visible to its chunk and stores the rows' distance; every old row that took a new id
// stores the distance the new row stores for it; and a search that starts at an old row which lists
// an inserted row finds that row first, at distance 0.  Prints the statistics and "ok".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rptree.hpp"
using namespace rptree;

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
  if (argc < 4) return std::printf("usage: %s n m d\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]), m = std::atoll(argv[2]);
  const int d = std::atoi(argv[3]), kg = 10, ef = 32, minLeaf = 40;
  const int64_t batch = 128;
  if (n < 100 || m < 1 || d < 1) return std::printf("FAIL n >= 100, m >= 1, d >= 1\n"), 2;
  SMGen gen(2026);
  std::vector<DVector> all((size_t)(n + m), DVector{std::vector<double>((size_t)d)});
  for (auto& x : all)
    for (auto& v : x.dvVec) v = gen.normal(0.0, 1.0);
  const std::vector<DVector> olds(all.begin(), all.begin() + (long)n), news(all.begin() + (long)n, all.end());
  try {
    Context ctx(0);
    Dataset dold(ctx, olds), dnew(ctx, news), dall(ctx, all);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, 4, cfg.fpProjNzDensity, d, dold);
    GraphResult g = knnGraph(tts, kg);
    g = knnGraphRefine(ctx, dold, g, 1);

    // nothing to insert: the graph comes back as it is
    const GraphResult same = graphInsert(ctx, dold, g, 0, ef, batch, {}, 8);
    if (same.ids != g.ids || same.count != g.count || std::memcmp(same.dist.data(), g.dist.data(), 8 * g.dist.size()))
      return std::printf("FAIL m = 0 does not copy the graph\n"), 1;

    InsertStats st;
    const GraphResult big = graphInsert(tts, dall, dnew, g, ef, batch, Metric::L2, 8, &st);
    if ((int64_t)big.count.size() != n + m) return std::printf("FAIL the grown graph has another size\n"), 1;
    for (int64_t p = n; p < n + m; ++p) {
      const int64_t visible = n + (p - n) / batch * batch;  // the rows its chunk saw
      for (int b = 0; b < big.count[(size_t)p]; ++b) {
        const int32_t id = big.ids[(size_t)p * kg + b];
        const double db = big.dist[(size_t)p * kg + b];
        // rows of later chunks may have joined this row since: they are not its own answer
        if (id < 0 || id >= n + m || id == p) return std::printf("FAIL row %" PRId64 " names %d\n", p, id), 1;
        const double fold = l2(all[(size_t)p], all[(size_t)id]);
        if (std::memcmp(&fold, &db, 8) != 0) return std::printf("FAIL row %" PRId64 ": not the rows' distance\n", p), 1;
        if (b > 0 && db < big.dist[(size_t)p * kg + b - 1]) return std::printf("FAIL row %" PRId64 " is not sorted\n", p), 1;
        if (id >= visible && id < visible + batch) return std::printf("FAIL row %" PRId64 " names a row of its own chunk\n", p), 1;
      }
    }
    // reverse links: old rows that took a new id, at the distance of the pair
    std::vector<DVector> qv;
    std::vector<int32_t> seeds, want;
    int64_t links = 0;
    for (int64_t o = 0; o < n; ++o)
      for (int b = 0; b < big.count[(size_t)o]; ++b) {
        const int32_t id = big.ids[(size_t)o * kg + b];
        if (id < n) continue;
        ++links;
        const double fold = l2(all[(size_t)o], all[(size_t)id]), db = big.dist[(size_t)o * kg + b];
        if (std::memcmp(&fold, &db, 8) != 0) return std::printf("FAIL row %" PRId64 ": not the pair's distance\n", o), 1;
        if (qv.size() < 32 && links % 7 == 1) {
          qv.push_back(all[(size_t)id]);
          seeds.push_back((int32_t)o);
          want.push_back(id);
        }
      }
    if (links == 0) return std::printf("FAIL no old row links to a new one\n"), 1;
    // an inserted row is found from a row that lists it
    Dataset qs(ctx, qv);
    const KnnResult found = graphSearch(ctx, dall, big, qs, 5, ef, seeds, 1);
    for (size_t i = 0; i < want.size(); ++i)
      if (found.ids[i * 5] != want[i] || found.dist[i * 5] != 0.0)
        return std::printf("FAIL inserted row %d is not found first at distance 0\n", want[i]), 1;
    std::printf("inserted %" PRId64 " rows into a graph of %" PRId64 "\n", m, n);
    std::printf("chunks %" PRId64 " evaluated %" PRId64 " (%.1f distances per new row) offered %" PRId64
                " accepted %" PRId64 "\n", st.chunks, st.evaluated, (double)st.evaluated / (double)m, st.offered,
                st.accepted);
    std::printf("old rows that list a new row: %" PRId64 " entries; %zu inserted rows searched for and found\n",
                links, want.size());
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
