// Shrinking an index without rebuilding anything, through the C++ host mirror: forest -> knnGraph ->
// knnGraphRefine over n rows once, then graphDelete of a fifth of them and graphSearch on what is left.
// Draws n = argv[1] rows of d = argv[2] standard normal columns, builds a forest of 4 trees and the
// 10-NN graph refined by one NN-descent round, deletes every row whose id is 2 mod 5 with the tombstone
// bitmap graphSearchAllow would take, and checks: keeping every row gives the graph back; no row of the
// result names a deleted row; every row is sorted and stores its rows' distance, kept entries and new
// ones alike; the compact form is the other form through newid; and a search over the compacted rows
// that starts at a row which lists a survivor finds that survivor first, at distance 0.  Prints the
// statistics and "ok".
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
  if (argc < 3) return std::printf("usage: %s n d\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]);
  const int d = std::atoi(argv[2]), kg = 10, ef = 32, minLeaf = 40;
  if (n < 100 || d < 1) return std::printf("FAIL n >= 100, d >= 1\n"), 2;
  SMGen gen(2026);
  std::vector<DVector> all((size_t)n, DVector{std::vector<double>((size_t)d)});
  for (auto& x : all)
    for (auto& v : x.dvVec) v = gen.normal(0.0, 1.0);
  std::vector<bool> mask((size_t)n);
  std::vector<DVector> left;
  for (int64_t i = 0; i < n; ++i) {
    mask[(size_t)i] = i % 5 != 2;
    if (mask[(size_t)i]) left.push_back(all[(size_t)i]);
  }
  const std::vector<uint32_t> keep = allowBitmap(mask);
  try {
    Context ctx(0);
    Dataset data(ctx, all), rest(ctx, left);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, 4, cfg.fpProjNzDensity, d, data);
    GraphResult g = knnGraph(tts, kg);
    g = knnGraphRefine(ctx, data, g, 1);

    // nothing to delete: the graph comes back as it is
    const DeleteResult same = graphDelete(ctx, data, g, {}, false);
    if (same.graph.ids != g.ids || same.graph.count != g.count ||
        std::memcmp(same.graph.dist.data(), g.dist.data(), 8 * g.dist.size()))
      return std::printf("FAIL keeping every row does not copy the graph\n"), 1;

    DeleteStats st;
    const DeleteResult old = graphDelete(ctx, data, g, keep, false, &st);
    const DeleteResult tight = graphDelete(ctx, data, g, keep, true);
    const int64_t nk = (int64_t)left.size();
    if (st.kept != nk || (int64_t)tight.graph.count.size() != nk || (int64_t)old.graph.count.size() != n)
      return std::printf("FAIL the result has another size\n"), 1;
    int64_t fresh = 0;
    for (int64_t p = 0; p < n; ++p) {
      const int32_t np = old.newid[(size_t)p];
      if (!mask[(size_t)p]) {
        if (np != -1 || old.graph.count[(size_t)p] != 0 || tight.newid[(size_t)p] != -1)
          return std::printf("FAIL deleted row %" PRId64 " is not empty\n", p), 1;
        continue;
      }
      const int32_t q = tight.newid[(size_t)p];
      if (np != p || q < 0 || old.graph.count[(size_t)p] != tight.graph.count[(size_t)q])
        return std::printf("FAIL newid of row %" PRId64 "\n", p), 1;
      for (int b = 0; b < old.graph.count[(size_t)p]; ++b) {
        const int32_t id = old.graph.ids[(size_t)p * kg + b];
        const double db = old.graph.dist[(size_t)p * kg + b];
        if (id < 0 || id >= n || id == p || !mask[(size_t)id])
          return std::printf("FAIL row %" PRId64 " names %d\n", p, id), 1;
        const double fold = l2(all[(size_t)p], all[(size_t)id]);
        if (std::memcmp(&fold, &db, 8) != 0) return std::printf("FAIL row %" PRId64 ": not the rows' distance\n", p), 1;
        if (b > 0 && db < old.graph.dist[(size_t)p * kg + b - 1]) return std::printf("FAIL row %" PRId64 " is not sorted\n", p), 1;
        if (tight.graph.ids[(size_t)q * kg + b] != tight.newid[(size_t)id] ||
            std::memcmp(&tight.graph.dist[(size_t)q * kg + b], &db, 8) != 0)
          return std::printf("FAIL row %" PRId64 ": the compact form differs\n", p), 1;
        bool was = false;
        for (int e = 0; e < g.count[(size_t)p]; ++e) was |= g.ids[(size_t)p * kg + e] == id;
        fresh += !was;
      }
    }
    if (st.touched == 0 || fresh == 0) return std::printf("FAIL no row was repaired\n"), 1;
    // a survivor is found from a row that lists it, over the compacted rows
    std::vector<DVector> qv;
    std::vector<int32_t> seeds, want;
    for (int64_t o = 0; o < nk && qv.size() < 32; o += 11) {
      if (tight.graph.count[(size_t)o] == 0) continue;
      const int32_t id = tight.graph.ids[(size_t)o * kg];
      qv.push_back(left[(size_t)id]);
      seeds.push_back((int32_t)o);
      want.push_back(id);
    }
    Dataset qs(ctx, qv);
    const KnnResult found = graphSearch(ctx, rest, tight.graph, qs, 5, ef, seeds, 1);
    for (size_t i = 0; i < want.size(); ++i)
      if (found.ids[i * 5] != want[i] || found.dist[i * 5] != 0.0)
        return std::printf("FAIL survivor %d is not found first at distance 0\n", want[i]), 1;
    std::printf("deleted %" PRId64 " of %" PRId64 " rows\n", n - nk, n);
    std::printf("kept %" PRId64 " touched %" PRId64 " evaluated %" PRId64 " (%.1f distances per touched row) dropped %"
                PRId64 "\n", st.kept, st.touched, st.evaluated, (double)st.evaluated / (double)st.touched, st.dropped);
    std::printf("entries the repair brought in: %" PRId64 "; %zu survivors searched for and found\n", fresh, want.size());
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
