// The kNN graph of SVector rows and its refinement under the cosine and inner-product distances
// through the C++ host mirror.  Reads CSR rows of f64 values from the file named by argv[1] (int64
// n, int64 d, rowptr[n + 1] int64, col[nnz] int32, val[nnz] double), builds a forest with seed 7
// (argv[2] trees, minLeaf argv[3]) and, under Metric::Cosine and then Metric::Inner, takes the kNN
// graph for k = argv[4] with knnGraphSV and applies argv[5] NN-descent rounds with argv[6] reverse
// neighbours with knnGraphRefineSV.  Every distance of the four graphs is evaluated again on the
// host from dotS (the left fold of the products of the columns both rows store, from +0.0) and must
// agree bit for bit; Metric::L2 through the overloads must give knnGraphSV's bits.  Prints per
// metric the statistics and a checksum of the two graphs (what a caller with the same rows and the
// same forest compares), then "ok".
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

static double distance(Metric m, const SVector& a, const SVector& b) {
  const double ab = dotS(a, b);
  if (m == Metric::Inner) return -ab;
  volatile double den = std::sqrt(dotS(a, a)) * std::sqrt(dotS(b, b));
  volatile double q = ab / den;
  return 1.0 - q;
}

static int64_t check_graph(Metric m, const std::vector<SVector>& xs, const GraphResult& g) {
  int64_t bad = 0;
  for (size_t i = 0; i < xs.size(); ++i)
    for (int s = 0; s < g.count[i]; ++s) {
      const double want = distance(m, xs[i], xs[(size_t)g.ids[i * (size_t)g.k + (size_t)s]]);
      const double got = g.dist[i * (size_t)g.k + (size_t)s];
      if (want != want && got != got) continue;  // NaN (a zero row under cosine): the payload is not compared
      bad += std::memcmp(&want, &got, 8) != 0;
    }
  return bad;
}

// sum over the slots p of (bits(dist[p]) ^ id[p] * G) * (2 p + 1), plus sum over the rows i of
// count[i] * (2 i + 1) * G, in 64-bit wrapping arithmetic
static uint64_t checksum(const GraphResult& g) {
  const uint64_t G = 0x9E3779B97F4A7C15ULL;
  uint64_t h = 0;
  for (size_t p = 0; p < g.ids.size(); ++p) {
    uint64_t bits;
    std::memcpy(&bits, &g.dist[p], 8);
    h += (bits ^ ((uint64_t)(uint32_t)g.ids[p] * G)) * (2 * (uint64_t)p + 1);
  }
  for (size_t i = 0; i < g.count.size(); ++i) h += (uint64_t)(uint32_t)g.count[i] * (2 * (uint64_t)i + 1) * G;
  return h;
}

int main(int argc, char** argv) {
  if (argc < 7) return std::printf("usage: %s rows.bin ntrees minleaf k iters reverse\n", argv[0]), 2;
  const int ntrees = std::atoi(argv[2]), minLeaf = std::atoi(argv[3]), k = std::atoi(argv[4]);
  const int iters = std::atoi(argv[5]), reverse = std::atoi(argv[6]);
  FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return std::printf("FAIL cannot open %s\n", argv[1]), 2;
  int64_t n = 0, d = 0;
  bool ok = std::fread(&n, 8, 1, fp) == 1 && std::fread(&d, 8, 1, fp) == 1 && n > 0 && d > 0;
  std::vector<int64_t> rowptr((size_t)(ok ? n + 1 : 0));
  ok = ok && std::fread(rowptr.data(), 8, rowptr.size(), fp) == rowptr.size() && rowptr[0] == 0;
  for (int64_t i = 0; ok && i < n; ++i) ok = rowptr[(size_t)i] <= rowptr[(size_t)i + 1];
  const size_t nnz = ok ? (size_t)rowptr[(size_t)n] : 0;
  std::vector<int32_t> col(nnz);
  std::vector<double> val(nnz);
  ok = ok && std::fread(col.data(), 4, nnz, fp) == nnz && std::fread(val.data(), 8, nnz, fp) == nnz;
  std::fclose(fp);
  if (!ok) return std::printf("FAIL short or malformed file\n"), 2;
  std::vector<SVector> xs;
  for (int64_t i = 0; i < n; ++i) {
    SVector v{(int)d, {}};
    for (int64_t p = rowptr[(size_t)i]; p < rowptr[(size_t)i + 1]; ++p)
      v.svVec.push_back({col[(size_t)p], val[(size_t)p]});
    xs.push_back(std::move(v));
  }
  try {
    Context ctx(0);
    Dataset dats(ctx, xs, (int)d);
    const RPTreeConfig cfg = rpTreeCfg(minLeaf, n, (int)d);
    RPForest tts = forestBatch(ctx, 7, cfg.fpMaxTreeDepth, minLeaf, ntrees, cfg.fpProjNzDensity, (int)d, dats);
    const GraphResult l2 = knnGraphSV(tts, k), l2m = knnGraphSV(tts, k, Metric::L2);
    if (l2.ids != l2m.ids || std::memcmp(l2.dist.data(), l2m.dist.data(), 8 * l2.dist.size()) != 0 ||
        l2.count != l2m.count)
      return std::printf("FAIL Metric::L2 gives another graph than knnGraphSV\n"), 1;
    const GraphResult l2r = knnGraphRefineSV(ctx, dats, l2, iters, reverse),
                      l2rm = knnGraphRefineSV(ctx, dats, l2, Metric::L2, iters, reverse);
    if (l2r.ids != l2rm.ids || std::memcmp(l2r.dist.data(), l2rm.dist.data(), 8 * l2r.dist.size()) != 0 ||
        l2r.count != l2rm.count)
      return std::printf("FAIL Metric::L2 gives another refinement than knnGraphRefineSV\n"), 1;
    for (Metric m : {Metric::Cosine, Metric::Inner}) {
      const char* name = m == Metric::Cosine ? "cosine" : "inner";
      const GraphResult g = knnGraphSV(tts, k, m);
      RefineStats st;
      const GraphResult refined = knnGraphRefineSV(ctx, dats, g, m, iters, reverse, &st);
      const int64_t bad = check_graph(m, xs, g) + check_graph(m, xs, refined);
      if (bad) return std::printf("FAIL %s: %" PRId64 " distances differ from the host dotS\n", name, bad), 1;
      std::printf("%s rounds %" PRId64 " updates %" PRId64 " candidates %" PRId64 " checksum %016" PRIx64
                  " %016" PRIx64 "\n",
                  name, st.rounds, st.updates, st.candidates, checksum(g), checksum(refined));
    }
    std::printf("ok\n");
  } catch (const RPTError& e) {
    std::printf("RPTError: %s\n", e.what());
    return 2;
  }
  return 0;
}
