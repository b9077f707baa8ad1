// The kNN graph under the cosine distance through the C++ host mirror.  Reads dense f64 rows from
// the file named by argv[1] (int64 n, int64 d, X[n][d] double), builds a forest (argv[2] trees,
// minLeaf argv[3]), takes its kNN graph for k = argv[4] under Metric::Cosine, applies argv[5]
// NN-descent rounds with argv[6] reverse neighbours under the same metric, prints the recall of both
// graphs against bruteKnn under that metric (k + 1 nearest, the point itself dropped) and writes to
// argv[7]: int32 T, int32 L, the dense-ified hyperplanes R[T][L][d] double, then both graphs (the
// forest's, the refined one), each ids[n][k] int32, dist[n][k] double, count[n] int32, then int64
// rounds, updates, candidates, then the two recalls as doubles.  Prints "ok" last.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "rptree.hpp"
using namespace rptree;

static void put(FILE* out, const GraphResult& g) {
  std::fwrite(g.ids.data(), 4, g.ids.size(), out);
  std::fwrite(g.dist.data(), 8, g.dist.size(), out);
  std::fwrite(g.count.data(), 4, g.count.size(), out);
}

// share of the exact neighbours (the brute-force k + 1 without the point itself, cut to k) that the graph holds
static double recall(const GraphResult& g, const BruteResult& truth, int64_t n, int k) {
  int64_t hit = 0, tot = 0;
  for (int64_t i = 0; i < n; ++i) {
    int taken = 0;
    for (int s = 0; s <= k && taken < k; ++s) {
      const int32_t want = truth.ids[(size_t)i * (k + 1) + s];
      if (want < 0 || want == i) continue;
      ++taken;
      ++tot;
      for (int e = 0; e < g.count[(size_t)i]; ++e)
        if (g.ids[(size_t)i * k + e] == want) {
          ++hit;
          break;
        }
    }
  }
  return tot ? (double)hit / (double)tot : 1.0;
}

int main(int argc, char** argv) {
  if (argc < 8) return std::printf("usage: %s data.bin ntrees minleaf k iters reverse out.bin\n", argv[0]), 2;
  const int ntrees = std::atoi(argv[2]), minLeaf = std::atoi(argv[3]), k = std::atoi(argv[4]);
  const int iters = std::atoi(argv[5]), reverse = std::atoi(argv[6]);
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
    const GraphResult g = knnGraph(tts, k, Metric::Cosine);
    RefineStats st;
    const GraphResult refined = knnGraphRefine(ctx, dats, g, Metric::Cosine, iters, reverse, &st);
    // Metric::L2 through the metric overloads: the bits of the entry points without a metric
    const GraphResult l2 = knnGraph(tts, k), l2m = knnGraph(tts, k, Metric::L2);
    if (l2.ids != l2m.ids || l2.dist != l2m.dist || l2.count != l2m.count)
      return std::printf("FAIL Metric::L2 gives another graph than knnGraph\n"), 1;

    const BruteResult truth = bruteKnn(ctx, dats, dats, k + 1, metric_flags(Metric::Cosine));
    const double r0 = recall(g, truth, n, k), r1 = recall(refined, truth, n, k);
    std::printf("rounds %" PRId64 " updates %" PRId64 " candidates %" PRId64 "\n", st.rounds, st.updates,
                st.candidates);
    std::printf("cosine recall@%d against bruteKnn: forest graph %.4f, refined %.4f\n", k, r0, r1);
    if (r1 < r0) return std::printf("FAIL the refinement lowered the recall\n"), 1;

    std::vector<double> R((size_t)ntrees * L * d, 0.0);
    for (int t = 0; t < ntrees; ++t)
      for (int l = 0; l < L; ++l)
        for (auto& iv : tts.rpVectors[(size_t)t][(size_t)l].svVec)
          R[((size_t)t * L + l) * d + (size_t)iv.first] = iv.second;
    FILE* out = std::fopen(argv[7], "wb");
    if (!out) return std::printf("FAIL cannot write %s\n", argv[7]), 2;
    const int32_t hdr[2] = {ntrees, L};
    std::fwrite(hdr, 4, 2, out);
    std::fwrite(R.data(), 8, R.size(), out);
    put(out, g);
    put(out, refined);
    const int64_t tail[3] = {st.rounds, st.updates, st.candidates};
    std::fwrite(tail, 8, 3, out);
    const double rec[2] = {r0, r1};
    std::fwrite(rec, 8, 2, out);
    std::fclose(out);
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
