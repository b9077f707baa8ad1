// Preparing the kNN graph of SVector rows for the search through the C++ host mirror: forest ->
// knnGraphSV -> knnGraphRefineSV -> graphPrepareSV -> graphSearchSV.  Draws argv[1] sparse rows and
// argv[2] sparse queries of dimension argv[3] with nonzero density argv[4], builds a forest (argv[5]
// trees, minLeaf argv[6]) and its kNN graph for kg = argv[7] refined by argv[8] NN-descent rounds.
// For a sample of rows the keep rule of DIVERSIFY is walked again on the host, every pair distance
// that decides it folded over the union of the two supports (metricDDL2's left fold, absent entries
// +0.0): the kept ids and the stored distances must agree with graphPrepareSV(diversify only) bit for
// bit.  Then the graph is prepared with both steps (kout = 2 kg) and searched for k = argv[9] with a
// beam of ef = argv[10] from the forest's 8 nearest candidates per query, next to the raw graph.
// Prints the statistics of the preparation, recall@k of both graphs against the exhaustive answer
// and "ok".
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

static double recallOf(const KnnResult& got, const BruteResult& truth, int64_t nq, int k) {
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
  if (argc < 11) return std::printf("usage: %s n nq d density ntrees minleaf kg iters k ef\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]), nq = std::atoll(argv[2]);
  const int d = std::atoi(argv[3]);
  const double density = std::atof(argv[4]);
  const int ntrees = std::atoi(argv[5]), minLeaf = std::atoi(argv[6]), kg = std::atoi(argv[7]);
  const int iters = std::atoi(argv[8]), k = std::atoi(argv[9]), ef = std::atoi(argv[10]);
  try {
    SMGen gen(2025);
    std::vector<SVector> xs, qv;
    for (int64_t i = 0; i < n; ++i) xs.push_back(sparse(gen, density, d));
    for (int64_t i = 0; i < nq; ++i) qv.push_back(sparse(gen, density, d));
    Context ctx(0);
    Dataset dats(ctx, xs, d), qs(ctx, qv, d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, d, dats);
    GraphResult g = knnGraphSV(tts, kg);
    if (iters > 0) g = knnGraphRefineSV(ctx, dats, g, iters);

    // DIVERSIFY alone, kout = kg: row i of the answer is Kept(i) (the rows of g are sorted already)
    PrepareStats ds;
    const GraphResult kept = graphPrepareSV(ctx, dats, g, kg, true, false, &ds);
    const int64_t step = n > 64 ? n / 64 : 1;
    int64_t rows = 0, folds = 0;
    for (int64_t i = 0; i < n; i += step, ++rows) {
      const int c = g.count[(size_t)i];
      std::vector<int> mine;  // the slots that stay
      for (int m = 0; m < c; ++m) {
        bool occluded = false;
        for (int l : mine) {
          ++folds;
          const double dlm = unionFold(xs[(size_t)g.ids[(size_t)i * kg + l]], xs[(size_t)g.ids[(size_t)i * kg + m]]);
          if (dlm < g.dist[(size_t)i * kg + m]) {
            occluded = true;
            break;
          }
        }
        if (!occluded) mine.push_back(m);
      }
      if ((int)mine.size() != kept.count[(size_t)i])
        return std::printf("FAIL row %" PRId64 ": %d kept, the host walk keeps %zu\n", i, kept.count[(size_t)i], mine.size()), 1;
      for (size_t a = 0; a < mine.size(); ++a) {
        const size_t src = (size_t)i * kg + (size_t)mine[a], dst = (size_t)i * kg + a;
        if (kept.ids[dst] != g.ids[src] || std::memcmp(&kept.dist[dst], &g.dist[src], 8) != 0)
          return std::printf("FAIL row %" PRId64 " slot %zu differs from the host walk\n", i, a), 1;
      }
    }
    std::printf("diversify: pairs %" PRId64 " occluded %" PRId64 "; %" PRId64 " rows walked on the host (%" PRId64
                " pair folds)\n", ds.pairs, ds.occluded, rows, folds);

    PrepareStats ps;
    const GraphResult sg = graphPrepareSV(tts, g, -1, true, true, &ps);
    std::printf("prepared: kout %d, pairs %" PRId64 " occluded %" PRId64 " capped %" PRId64 "\n", sg.k, ps.pairs,
                ps.occluded, ps.capped);
    const BruteResult truth = bruteKnn(ctx, dats, qs, k);
    const KnnResult raw = graphSearchSV(tts, g, qs, k, ef), got = graphSearchSV(tts, sg, qs, k, ef);
    std::printf("raw graph recall@%d %.4f\n", k, recallOf(raw, truth, nq, k));
    std::printf("recall@%d %.4f\n", k, recallOf(got, truth, nq, k));
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
