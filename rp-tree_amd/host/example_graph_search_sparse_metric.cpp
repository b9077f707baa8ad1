// Answering cosine queries with the kNN graph of SVector rows through the C++ host mirror: forest ->
// knnGraphSV -> knnGraphRefineSV -> graphPrepareSV -> graphSearchSV, all under Metric::Cosine.  Draws
// argv[1] sparse rows and argv[2] sparse queries of dimension argv[3] with nonzero density argv[4],
// builds a forest (3 trees, minLeaf 40), its 8-NN graph refined by one NN-descent round, prepares it
// (diversify, reverse union, 16 columns) and searches it for k = 5 with a beam of ef = 16 from the
// forest's 8 nearest candidates per query.  Every distance of the answer is evaluated again on the
// host from dotS (the left fold of the products of the columns both vectors store, from +0.0) and must
// agree bit for bit; Metric::L2 through the overloads must give graphPrepareSV's and graphSearchSV's
// bits.  Prints the statistics, recall@k against the exhaustive answer under the same metric and "ok".
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rptree.hpp"
using namespace rptree;

static double dotS(const SVector& a, const SVector& b) {
  size_t i = 0, j = 0;
  double acc = 0.0;
  while (i < a.svVec.size() && j < b.svVec.size()) {
    const int ci = a.svVec[i].first, cj = b.svVec[j].first;
    if (ci == cj) {
      volatile double pr = a.svVec[i].second * b.svVec[j].second;  // product and sum rounded on their own
      acc = acc + pr;
    }
    if (ci <= cj) ++i;
    if (cj <= ci) ++j;
  }
  return acc;
}

static double cosine(const SVector& a, const SVector& b) {
  const double ab = dotS(a, b);
  volatile double den = std::sqrt(dotS(a, a)) * std::sqrt(dotS(b, b));
  volatile double q = ab / den;
  return 1.0 - q;
}

template <class R>
static bool same_bits(const R& a, const R& b) {
  return a.ids == b.ids && a.count == b.count && a.dist.size() == b.dist.size() &&
         std::memcmp(a.dist.data(), b.dist.data(), 8 * a.dist.size()) == 0;
}

int main(int argc, char** argv) {
  if (argc < 5) return std::printf("usage: %s n nq d density\n", argv[0]), 2;
  const int64_t n = std::atoll(argv[1]), nq = std::atoll(argv[2]);
  const int d = std::atoi(argv[3]);
  const double density = std::atof(argv[4]);
  const int ntrees = 3, minLeaf = 40, kg = 8, kout = 16, k = 5, ef = 16;
  const Metric m = Metric::Cosine;
  try {
    SMGen gen(2025);
    std::vector<SVector> xs, qv;
    for (int64_t i = 0; i < n; ++i) xs.push_back(sparse(gen, density, d));
    for (int64_t i = 0; i < nq; ++i) qv.push_back(sparse(gen, density, d));
    Context ctx(0);
    Dataset dats(ctx, xs, d), qs(ctx, qv, d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, d, dats);
    // Metric::L2 through the new overloads: the bits of the L2 functions
    const GraphResult l2 = knnGraphSV(tts, kg);
    const GraphResult l2p = graphPrepareSV(ctx, dats, l2, kout);
    if (!same_bits(l2p, graphPrepareSV(ctx, dats, l2, Metric::L2, kout)))
      return std::printf("FAIL Metric::L2 gives another graph than graphPrepareSV\n"), 1;
    if (!same_bits(graphSearchSV(tts, l2p, qs, k, ef), graphSearchSV(tts, l2p, qs, Metric::L2, k, ef)))
      return std::printf("FAIL Metric::L2 gives another answer than graphSearchSV\n"), 1;
    // build -> refine -> prepare -> search under cosine
    GraphResult g = knnGraphSV(tts, kg, m);
    g = knnGraphRefineSV(ctx, dats, g, m, 1);
    PrepareStats ps;
    const GraphResult sg = graphPrepareSV(tts, g, m, kout, true, true, &ps);
    SearchStats st;
    const KnnResult got = graphSearchSV(tts, sg, qs, m, k, ef, 8, &st);
    const BruteResult truth = bruteKnn(ctx, dats, qs, k, m);
    int64_t hits = 0, want = 0, bad = 0;
    for (int64_t i = 0; i < n; ++i)
      for (int b = 0; b < sg.count[(size_t)i]; ++b) {
        const double db = sg.dist[(size_t)i * kout + b];
        const double fold = cosine(xs[(size_t)i], xs[(size_t)sg.ids[(size_t)i * kout + b]]);
        if (fold != fold && db != db) continue;  // NaN (a vector without nonzeros): the payload is not compared
        bad += std::memcmp(&fold, &db, 8) != 0;
      }
    for (int64_t i = 0; i < nq; ++i) {
      for (int a = 0; a < k; ++a) {
        const int32_t t = truth.ids[(size_t)i * k + a];
        if (t < 0) continue;
        ++want;
        for (int b = 0; b < got.count[(size_t)i]; ++b) hits += got.ids[(size_t)i * k + b] == t;
      }
      for (int b = 0; b < got.count[(size_t)i]; ++b) {
        const double db = got.dist[(size_t)i * k + b];
        const double fold = cosine(qv[(size_t)i], xs[(size_t)got.ids[(size_t)i * k + b]]);
        if (fold != fold && db != db) continue;
        bad += std::memcmp(&fold, &db, 8) != 0;
        if (b > 0 && db < got.dist[(size_t)i * k + b - 1]) return std::printf("FAIL query %" PRId64 " is not sorted\n", i), 1;
      }
    }
    if (bad) return std::printf("FAIL %" PRId64 " distances differ from the host dotS\n", bad), 1;
    std::printf("prepare: pairs %" PRId64 " occluded %" PRId64 " capped %" PRId64 "\n", ps.pairs, ps.occluded, ps.capped);
    std::printf("search: expansions %" PRId64 " evaluated %" PRId64 " (%.1f distances per query)\n", st.expansions,
                st.evaluated, nq ? (double)st.evaluated / (double)nq : 0.0);
    std::printf("recall@%d %.4f\n", k, want ? (double)hits / (double)want : 1.0);
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
