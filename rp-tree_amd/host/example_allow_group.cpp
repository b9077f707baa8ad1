// Three tenants served from one batch, through the C++ host mirror: row i belongs to tenant i % 3 and
// query q to tenant q % 3, except that every seventh query is unfiltered (group -1).  Reads dense f64
// rows from the file named by argv[1] (int64 n, int64 d, X[n][d] double) and queries of the same
// layout from argv[2], builds a forest (argv[3] trees, minLeaf argv[4]) and its kNN graph for kg =
// argv[5], refined by one NN-descent round and prepared, and answers k = argv[6] in ONE call each of
// graphSearchAllowGroup (ef = argv[7], width = argv[8], seeds from the forest), knnAllowGroup and
// bruteKnnAllowGroup under the three tenants' bitmaps.  Checks every grouped answer bit for bit against
// one single-bitmap call per tenant over that tenant's queries (the only route before), that no answer
// leaves its tenant, and prints per query "graph|forest|brute <q> tenant <t>: id:distance ..." and "ok".
#include <cinttypes>
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

// row q of a grouped answer against row r of a per-tenant answer: ids and distance bits
static bool same_row(const int32_t* ia, const double* da, const int32_t* ib, const double* db, int k) {
  return std::memcmp(ia, ib, 4 * (size_t)k) == 0 && std::memcmp(da, db, 8 * (size_t)k) == 0;
}

static void print_row(const char* what, int64_t q, int t, const int32_t* ids, const double* dist, int k) {
  std::printf("%s %" PRId64 " tenant %d:", what, q, t);
  for (int b = 0; b < k; ++b) std::printf(" %d:%.17g", ids[b], dist[b]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 9) return std::printf("usage: %s data.bin queries.bin ntrees minleaf kg k ef width\n", argv[0]), 2;
  const int ntrees = std::atoi(argv[3]), minLeaf = std::atoi(argv[4]), kg = std::atoi(argv[5]);
  const int k = std::atoi(argv[6]), ef = std::atoi(argv[7]), width = std::atoi(argv[8]);
  const int G = 3;
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
    // the tenants' bitmaps, one after the other, and every query's tenant
    std::vector<std::vector<bool>> owns((size_t)G, std::vector<bool>((size_t)n, false));
    for (int64_t i = 0; i < n; ++i) owns[(size_t)(i % G)][(size_t)i] = true;
    const std::vector<uint32_t> allow = allowBitmaps(owns);
    std::vector<int32_t> group((size_t)nq);
    for (int64_t q = 0; q < nq; ++q) group[(size_t)q] = q % 7 == 6 ? -1 : (int32_t)(q % G);
    // one call each for the whole batch
    const KnnResult graph = graphSearchAllowGroup(tts, sg, qs, allow, G, group, k, ef, width);
    const KnnResult forest = knnAllowGroup(tts, allow, G, group, k, qs, RPT_KNN_DEDUP);
    const BruteResult brute = bruteKnnAllowGroup(ctx, dats, allow, G, group, qs, k);
    // the route without groups: the queries gathered by tenant, one call per tenant
    for (int t = -1; t < G; ++t) {
      std::vector<int64_t> rows;
      std::vector<DVector> sub;
      for (int64_t q = 0; q < nq; ++q)
        if (group[(size_t)q] == t) rows.push_back(q), sub.push_back(qv[(size_t)q]);
      if (rows.empty()) continue;
      Dataset sq(ctx, sub);
      const std::vector<uint32_t> one = t < 0 ? std::vector<uint32_t>() : allowBitmap(owns[(size_t)t]);
      const KnnResult wg = graphSearchAllow(tts, sg, sq, one, k, ef, width);
      const KnnResult wf = knnAllow(tts, one, k, sq, RPT_KNN_DEDUP);
      const BruteResult wb = bruteKnnAllow(ctx, dats, one, sq, k);
      for (size_t r = 0; r < rows.size(); ++r) {
        const size_t q = (size_t)rows[r];
        if (graph.count[q] != wg.count[r] || !same_row(&graph.ids[q * k], &graph.dist[q * k], &wg.ids[r * k], &wg.dist[r * k], k))
          return std::printf("FAIL graph search: query %zu differs from its tenant's own call\n", q), 1;
        if (forest.count[q] != wf.count[r] || !same_row(&forest.ids[q * k], &forest.dist[q * k], &wf.ids[r * k], &wf.dist[r * k], k))
          return std::printf("FAIL forest query: query %zu differs from its tenant's own call\n", q), 1;
        if (!same_row(&brute.ids[q * k], &brute.dist[q * k], &wb.ids[r * k], &wb.dist[r * k], k))
          return std::printf("FAIL exhaustive kNN: query %zu differs from its tenant's own call\n", q), 1;
      }
    }
    for (int64_t q = 0; q < nq; ++q) {
      const int t = group[(size_t)q];
      for (int b = 0; b < k; ++b)
        for (const int32_t id : {graph.ids[(size_t)q * k + b], forest.ids[(size_t)q * k + b], brute.ids[(size_t)q * k + b]})
          if (id >= 0 && t >= 0 && id % G != t) return std::printf("FAIL query %" PRId64 " answers another tenant's row\n", q), 1;
      print_row("graph", q, t, &graph.ids[(size_t)q * k], &graph.dist[(size_t)q * k], k);
      print_row("forest", q, t, &forest.ids[(size_t)q * k], &forest.dist[(size_t)q * k], k);
      print_row("brute", q, t, &brute.ids[(size_t)q * k], &brute.dist[(size_t)q * k], k);
    }
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
