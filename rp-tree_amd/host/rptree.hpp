// rptree.hpp — header-only C++ host mirror of the Data.RPTree API surface for the hot path,
// over the C ABI of include/rptree_hip.h.  The reference host language is Haskell (no GHC in
// the build image), so this mirror keeps the reference's names, argument order and error
// behaviour in C++ (the Python mirror is rp-tree_amd/python/rptree_amd).
//
//   forestBatch / treeBatch   Batch.hs:29-63          knn          RPTree.hs:168-176
//   candidates                RPTree.hs:289-314        recallWith   RPTree.hs:259-282
//   knnH / knnPQ              RPTree.hs:181-217,318-342
//   rpTreeCfg / RPTreeConfig  Conduit.hs:123-141       SVector/DVector/Embed  Internal.hs:56-133
//   sparse / stdNormal / sample: host-side hyperplane sampling, Batch.hs:59-61, Gen.hs:148-195
//   (SplitMix64 + Box-Muller restated from the published algorithm: self-consistent, not
//   verified against Hackage's splitmix-distributions — a Haskell host keeps its own generator).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rptree_hip.h"

namespace rptree {

struct RPTError : std::runtime_error {  // next to Internal.hs:66-72
  int code;
  RPTError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int32_t s) {
  if (s != RPT_OK) throw RPTError(s, rpt_last_error());
}

// ---- vector types, Internal.hs:92-133 ----
struct SVector {
  int svDim;
  std::vector<std::pair<int, double>> svVec;  // ascending indices (unchecked in the reference)
};
struct DVector {
  std::vector<double> dvVec;
};
inline SVector fromListSv(int n, std::vector<std::pair<int, double>> ll) { return {n, std::move(ll)}; }
inline DVector fromListDv(std::vector<double> ll) { return {std::move(ll)}; }
template <class V, class X>
struct Embed {
  V eEmbed;
  X eData;
};

// Inner SVector DVector / metricL2 with the reference's summation order (Internal.hs:369-406)
inline double inner(const SVector& u, const DVector& v) {
  double acc = 0.0;
  size_t m = u.svVec.size() < v.dvVec.size() ? u.svVec.size() : v.dvVec.size();
  for (size_t j = m; j-- > 0;) acc = u.svVec[j].second * v.dvVec[(size_t)u.svVec[j].first] + acc;
  return acc;
}
inline double metricL2(const DVector& u, const DVector& v) {
  double acc = 0.0;
  for (size_t j = 0; j < u.dvVec.size() && j < v.dvVec.size(); ++j)
    acc = acc + std::pow(u.dvVec[j] - v.dvVec[j], 2.0);
  return std::sqrt(acc);
}

// ---- parameters, Conduit.hs:123-141 ----
struct RPTreeConfig {
  int fpMaxTreeDepth;
  int64_t fpDataChunkSize;
  double fpProjNzDensity;
};
inline RPTreeConfig rpTreeCfg(int minl, int64_t n, int d) {
  const double maxd = std::ceil(std::log((double)n / (double)minl) / std::log(2.0));
  const double pnzMin = 1.0 / (std::log((double)d) / std::log(10.0));
  return {(int)maxd, (int64_t)std::ceil((double)n / 100.0), pnzMin < 1.0 ? pnzMin : 1.0};
}

// ---- host-side random generation (stays on the host), Gen.hs:148-195 ----
class SMGen {
  uint64_t seed_, gamma_;
  static uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 33)) * 0xff51afd7ed558ccdULL;
    z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53ULL;
    return z ^ (z >> 33);
  }
  static uint64_t mixGamma(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z = (z ^ (z >> 31)) | 1ULL;
    return __builtin_popcountll(z ^ (z >> 1)) >= 24 ? z : z ^ 0xaaaaaaaaaaaaaaaaULL;
  }

 public:
  explicit SMGen(uint64_t s) : seed_(mix64(s)), gamma_(mixGamma(s + 0x9e3779b97f4a7c15ULL)) {}
  uint64_t nextWord64() {
    seed_ += gamma_;
    return mix64(seed_);
  }
  double nextDouble() { return (double)(nextWord64() >> 11) * 0x1.0p-53; }
  bool bernoulli(double p) { return nextDouble() < p; }
  double normal(double mu, double sig) {
    const double u1 = nextDouble(), u2 = nextDouble();
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2) * sig + mu;
  }
  double uniformR(double lo, double hi) { return nextDouble() * (hi - lo) + lo; }
};
// `sparse pnz dim stdNormal`
inline SVector sparse(SMGen& g, double pnz, int dim) {
  SVector v{dim, {}};
  for (int i = 0; i < dim; ++i)
    if (g.bernoulli(pnz)) v.svVec.push_back({i, g.normal(0.0, 1.0)});
  return v;
}

// ---- handles ----
class Context {
  rpt_ctx* h_ = nullptr;

 public:
  explicit Context(int device = 0) { check(rpt_ctx_create(device, &h_)); }
  ~Context() { rpt_ctx_destroy(h_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  rpt_ctx* get() const { return h_; }
};

class Dataset {
  rpt_dataset* h_ = nullptr;

 public:
  int64_t n = 0;
  int d = 0;
  bool csr = false;  // SVector rows
  Dataset(Context& ctx, const std::vector<DVector>& xs) {
    n = (int64_t)xs.size();
    d = n ? (int)xs[0].dvVec.size() : 1;
    std::vector<double> flat((size_t)n * d);
    for (int64_t i = 0; i < n; ++i)
      for (int j = 0; j < d; ++j) flat[(size_t)i * d + j] = xs[(size_t)i].dvVec[(size_t)j];
    check(rpt_dataset_dense_host(ctx.get(), flat.data(), n, d, RPT_F64, &h_));
  }
  // SVector rows as CSR (rowptr / col / val); `dim` is the rows' svDim
  Dataset(Context& ctx, const std::vector<SVector>& xs, int dim) {
    n = (int64_t)xs.size();
    d = dim;
    csr = true;
    std::vector<int64_t> rowptr{0};
    std::vector<int32_t> col;
    std::vector<double> val;
    for (auto& x : xs) {
      for (auto& iv : x.svVec) {
        col.push_back(iv.first);
        val.push_back(iv.second);
      }
      rowptr.push_back((int64_t)col.size());
    }
    col.push_back(0);  // non-NULL pointers for an all-empty batch
    val.push_back(0.0);
    check(rpt_dataset_csr_host(ctx.get(), rowptr.data(), col.data(), val.data(), n, d, RPT_F64, &h_));
  }
  ~Dataset() { rpt_dataset_free(h_); }
  Dataset(const Dataset&) = delete;
  Dataset& operator=(const Dataset&) = delete;
  rpt_dataset* get() const { return h_; }
};

// `RPForest d a` (Internal.hs:182): trees keyed 0..T-1, held flat in HBM.
class RPForest {
  rpt_forest* h_ = nullptr;

 public:
  Context* ctx;
  const Dataset* data;
  std::vector<std::vector<SVector>> rpVectors;  // _rpVectors of every tree (one per level)
  int T, L, minLeaf;
  bool streamed = false;  // built by the chunk fold of `forest` (explicit topology)
  // chunk == 0: the batch build (createMulti); chunk > 0: the streaming build, `insert` folded over
  // chunks of `chunk` points (Conduit.hs:147-176 over Internal.hs:245-297)
  RPForest(Context& c, const Dataset& ds, std::vector<std::vector<SVector>> rvss, int maxd,
           int minl, int64_t chunk = 0)
      : ctx(&c), data(&ds), rpVectors(std::move(rvss)), T((int)rpVectors.size()), L(maxd),
        minLeaf(minl) {
    std::vector<double> R((size_t)T * L * ds.d, 0.0);  // dense-ified [T][L][d]
    for (int t = 0; t < T; ++t)
      for (int l = 0; l < L; ++l)
        for (auto& iv : rpVectors[(size_t)t][(size_t)l].svVec)
          R[((size_t)t * L + l) * ds.d + (size_t)iv.first] = iv.second;
    if (chunk > 0) {
      check(rpt_forest_stream_build(c.get(), ds.get(), R.data(), T, L, minl, chunk, RPT_PROJ_AUTO, &h_));
      streamed = true;
    } else {
      check(rpt_forest_build(c.get(), ds.get(), R.data(), T, L, minl, RPT_PROJ_AUTO, &h_));
    }
  }
  ~RPForest() { rpt_forest_free(h_); }
  RPForest(const RPForest&) = delete;
  RPForest& operator=(const RPForest&) = delete;
  rpt_forest* get() const { return h_; }
  std::vector<int32_t> perm() const {
    std::vector<int32_t> p((size_t)T * data->n);
    check(rpt_forest_get_perm(h_, p.data()));
    return p;
  }
  // treeSize (RPTree.hs:362-363): sum of the leaf sizes of tree t
  int64_t treeSize(int) const {
    if (streamed) {  // points held by the Tips (less than n after the data-loss branch, :277)
      int64_t held = 0;
      check(rpt_forest_get_topology(h_, nullptr, nullptr, nullptr, nullptr, &held, nullptr));
      return held;
    }
    int64_t cnt = 0, nrec = 0;
    check(rpt_topology(data->n, L, minLeaf, nullptr, 0, &nrec));
    std::vector<int64_t> rec((size_t)nrec * 5);
    check(rpt_topology(data->n, L, minLeaf, rec.data(), nrec, &nrec));
    for (int64_t i = 0; i < nrec; ++i)
      if (rec[(size_t)i * 5 + 4]) cnt += rec[(size_t)i * 5 + 3];
    return cnt;
  }
};

// forestBatch :: Word64 -> Int -> Int -> Int -> Double -> Int -> data -> RPForest  (Batch.hs:48-63)
inline RPForest forestBatch(Context& ctx, uint64_t seed, int maxd, int minl, int ntrees, double pnz,
                            int dim, const Dataset& src) {
  if (dim != src.d) throw RPTError(RPT_E_ARG, "projection vector dimension != data dimension");
  SMGen g(seed);  // `sample seed`: one generator, trees outermost, levels inner (Batch.hs:59-61)
  std::vector<std::vector<SVector>> rvss((size_t)ntrees);
  for (int t = 0; t < ntrees; ++t)
    for (int l = 0; l < maxd; ++l) rvss[(size_t)t].push_back(sparse(g, pnz, dim));
  return RPForest(ctx, src, std::move(rvss), maxd, minl);
}
inline RPForest treeBatch(Context& ctx, uint64_t seed, int maxDepth, int minLeaf, double pnz, int dim,
                          const Dataset& src) {
  return forestBatch(ctx, seed, maxDepth, minLeaf, 1, pnz, dim, src);
}
// forest :: Word64 -> Int -> Int -> Int -> Int -> Double -> Int -> source -> RPForest
// (Conduit.hs:104-121): seed, max depth, min leaf, trees, CHUNK SIZE, density, dimension, data —
// the reference's streaming semantics (same hyperplane draw order, Conduit.hs:116-118)
inline RPForest forest(Context& ctx, uint64_t seed, int maxd, int minl, int ntrees, int64_t chunksize,
                       double pnz, int dim, const Dataset& src) {
  if (dim != src.d) throw RPTError(RPT_E_ARG, "projection vector dimension != data dimension");
  if (chunksize < 1) throw RPTError(RPT_E_ARG, "chunk size must be >= 1");
  SMGen g(seed);
  std::vector<std::vector<SVector>> rvss((size_t)ntrees);
  for (int t = 0; t < ntrees; ++t)
    for (int l = 0; l < maxd; ++l) rvss[(size_t)t].push_back(sparse(g, pnz, dim));
  return RPForest(ctx, src, std::move(rvss), maxd, minl, chunksize);
}

// The distance `knn` ranks by (the reference's distf argument): metricL2, or the cosine / negated
// inner-product distances of RPT_KNN_METRIC_COSINE / RPT_KNN_METRIC_INNER (include/rptree_hip.h:
// every value in double, the dots a left fold).  On SVector data Cosine / Inner go to the
// rpt_*_csr_metric_* entry points: the fold runs over the indices both vectors store, in ascending
// order — the dense value of the dense-ified vectors when the stored values are finite, and a
// stored inf / NaN counts only where both store the index.
enum class Metric { L2, Cosine, Inner };

inline int32_t metric_flags(Metric m) {
  return m == Metric::Cosine ? RPT_KNN_METRIC_COSINE : m == Metric::Inner ? RPT_KNN_METRIC_INNER : 0;
}

// knn distf k forest q  (RPTree.hs:168-176): (distance, point id), duplicates kept
inline std::vector<std::pair<double, int32_t>> knn(const RPForest& tts, int k, const DVector& q,
                                                   Metric metric = Metric::L2) {
  std::vector<DVector> qv{q};
  Dataset qs(*tts.ctx, qv);
  std::vector<int32_t> ids((size_t)k);
  std::vector<double> dist((size_t)k);
  int32_t cnt = 0;
  check(rpt_knn_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), k,
                     RPT_KNN_KEEP_DUPLICATES | metric_flags(metric), ids.data(), dist.data(), &cnt));
  std::vector<std::pair<double, int32_t>> out;
  for (int i = 0; i < cnt; ++i) out.push_back({dist[(size_t)i], ids[(size_t)i]});
  return out;
}

// knnPQ distf k forest q  (RPTree.hs:181-194): like knn, one entry per distance (`nub`)
inline std::vector<std::pair<double, int32_t>> knnPQ(const RPForest& tts, int k, const DVector& q,
                                                     Metric metric = Metric::L2) {
  std::vector<DVector> qv{q};
  Dataset qs(*tts.ctx, qv);
  std::vector<int32_t> ids((size_t)k);
  std::vector<double> dist((size_t)k);
  int32_t cnt = 0;
  check(rpt_knn_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), k,
                     RPT_KNN_DEDUP_DISTANCE | metric_flags(metric), ids.data(), dist.data(), &cnt));
  std::vector<std::pair<double, int32_t>> out;
  for (int i = 0; i < cnt; ++i) out.push_back({dist[(size_t)i], ids[(size_t)i]});
  return out;
}

// ... and for an SVector forest; Metric::Cosine / Inner: rpt_knn_csr_metric_host
inline std::vector<std::pair<double, int32_t>> knnSV(const RPForest& tts, int k, const SVector& q, Metric metric,
                                                     int32_t dedup) {
  std::vector<SVector> qv{q};
  Dataset qs(*tts.ctx, qv, tts.data->d);
  std::vector<int32_t> ids((size_t)k);
  std::vector<double> dist((size_t)k);
  int32_t cnt = 0;
  check((metric == Metric::L2 ? rpt_knn_host : rpt_knn_csr_metric_host)(
      tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), k, dedup | metric_flags(metric), ids.data(), dist.data(),
      &cnt));
  std::vector<std::pair<double, int32_t>> out;
  for (int i = 0; i < cnt; ++i) out.push_back({dist[(size_t)i], ids[(size_t)i]});
  return out;
}
inline std::vector<std::pair<double, int32_t>> knn(const RPForest& tts, int k, const SVector& q,
                                                   Metric metric = Metric::L2) {
  return knnSV(tts, k, q, metric, RPT_KNN_KEEP_DUPLICATES);
}
inline std::vector<std::pair<double, int32_t>> knnPQ(const RPForest& tts, int k, const SVector& q,
                                                     Metric metric = Metric::L2) {
  return knnSV(tts, k, q, metric, RPT_KNN_DEDUP_DISTANCE);
}

// knnH metricL2 k forest q  (RPTree.hs:199-217): whole buckets of the leaves with the smallest
// margin priority, NOT sorted by distance and NOT cut to k (as the reference)
inline std::vector<std::pair<double, int32_t>> knnH(const RPForest& tts, int k, const DVector& q) {
  std::vector<DVector> qv{q};
  Dataset qs(*tts.ctx, qv);
  int64_t off[2] = {0, 0}, total = 0;
  check(rpt_knnh_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), k, off, nullptr,
                      nullptr, 0, &total));
  std::vector<int32_t> ids((size_t)(total > 0 ? total : 1));
  std::vector<double> dist((size_t)(total > 0 ? total : 1));
  check(rpt_knnh_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), k, off, ids.data(),
                      dist.data(), total, &total));
  std::vector<std::pair<double, int32_t>> out;
  for (int64_t i = 0; i < total; ++i) out.push_back({dist[(size_t)i], ids[(size_t)i]});
  return out;
}

// candidates tree q (RPTree.hs:289-314): ids of the leaf buckets reached in tree t
inline std::vector<int32_t> candidates(const RPForest& tts, int t, const DVector& q) {
  std::vector<DVector> qv{q};
  Dataset qs(*tts.ctx, qv);
  std::vector<int64_t> off((size_t)tts.T + 1);
  int64_t total = 0;
  check(rpt_candidates(tts.ctx->get(), tts.get(), qs.get(), off.data(), nullptr, 0, &total));
  std::vector<int32_t> ids((size_t)(total > 0 ? total : 1));
  check(rpt_candidates(tts.ctx->get(), tts.get(), qs.get(), off.data(), ids.data(), total, &total));
  return std::vector<int32_t>(ids.begin() + off[(size_t)t], ids.begin() + off[(size_t)t + 1]);
}

inline std::vector<int32_t> candidates(const RPForest& tts, int t, const SVector& q) {
  std::vector<SVector> qv{q};
  Dataset qs(*tts.ctx, qv, tts.data->d);
  std::vector<int64_t> off((size_t)tts.T + 1);
  int64_t total = 0;
  check(rpt_candidates(tts.ctx->get(), tts.get(), qs.get(), off.data(), nullptr, 0, &total));
  std::vector<int32_t> ids((size_t)(total > 0 ? total : 1));
  check(rpt_candidates(tts.ctx->get(), tts.get(), qs.get(), off.data(), ids.data(), total, &total));
  return std::vector<int32_t>(ids.begin() + off[(size_t)t], ids.begin() + off[(size_t)t + 1]);
}

// ---- the vote threshold (rpt_knn_vote_host, rpt_vote_candidates_host) ----
// knnVote: only the ids that at least v trees propose are ranked, each once, by (distance, id) ->
// (distance, point id).  Every row layout and Metric, batch and streamed forests, any number of
// trees and of candidates, k up to 1024; the distances are knn's for the same data and metric.
// reference_metric (SVector rows, Metric::L2): the reference's truncating metricSSL2.
template <class Q>
inline std::vector<std::pair<double, int32_t>> knnVoteVia(const RPForest& tts, const Q& qs, int k, int v,
                                                          int32_t flags) {
  std::vector<int32_t> ids((size_t)k);
  std::vector<double> dist((size_t)k);
  int32_t cnt = 0;
  check(rpt_knn_vote_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), k, v, flags, ids.data(),
                          dist.data(), &cnt));
  std::vector<std::pair<double, int32_t>> out;
  for (int i = 0; i < cnt; ++i) out.push_back({dist[(size_t)i], ids[(size_t)i]});
  return out;
}
inline std::vector<std::pair<double, int32_t>> knnVote(const RPForest& tts, int k, int v, const DVector& q,
                                                       Metric metric = Metric::L2) {
  std::vector<DVector> qv{q};
  Dataset qs(*tts.ctx, qv);
  return knnVoteVia(tts, qs, k, v, metric_flags(metric));
}
inline std::vector<std::pair<double, int32_t>> knnVote(const RPForest& tts, int k, int v, const SVector& q,
                                                       Metric metric = Metric::L2, bool reference_metric = false) {
  std::vector<SVector> qv{q};
  Dataset qs(*tts.ctx, qv, tts.data->d);
  return knnVoteVia(tts, qs, k, v, metric_flags(metric) | (reference_metric ? RPT_KNN_METRIC_REFERENCE : 0));
}

// voteCandidates: (id, number of trees that propose it) of the ids with at least v votes, ascending
// (the reference's commented-out counts / keepCounts, RPTree.hs:464-478)
template <class Q>
inline std::vector<std::pair<int32_t, int32_t>> voteCandidatesVia(const RPForest& tts, const Q& qs, int v) {
  int64_t off[2] = {0, 0}, total = 0;
  check(rpt_vote_candidates_host(tts.ctx->get(), tts.get(), qs.get(), v, off, nullptr, nullptr, 0, &total));
  std::vector<int32_t> ids((size_t)(total > 0 ? total : 1)), counts(ids.size());
  check(rpt_vote_candidates_host(tts.ctx->get(), tts.get(), qs.get(), v, off, ids.data(), counts.data(), total,
                                 &total));
  std::vector<std::pair<int32_t, int32_t>> out;
  for (int64_t i = 0; i < total; ++i) out.push_back({ids[(size_t)i], counts[(size_t)i]});
  return out;
}
inline std::vector<std::pair<int32_t, int32_t>> voteCandidates(const RPForest& tts, int v, const DVector& q) {
  std::vector<DVector> qv{q};
  Dataset qs(*tts.ctx, qv);
  return voteCandidatesVia(tts, qs, v);
}
inline std::vector<std::pair<int32_t, int32_t>> voteCandidates(const RPForest& tts, int v, const SVector& q) {
  std::vector<SVector> qv{q};
  Dataset qs(*tts.ctx, qv, tts.data->d);
  return voteCandidatesVia(tts, qs, v);
}

// ---- evaluation: exhaustive kNN and recallWith (RPTree.hs:259-282), dense and SVector data ----
// flags: 0, metric_flags(Metric::Cosine / Inner) on dense data, RPT_KNN_METRIC_REFERENCE (the
// reference's truncating metricSSL2) on SVector data
// kNN graph of the forest's own points (rpt_knn_graph_host): knn (RPTree.hs:174-176) with every
// stored point as the query, built leaf by leaf.  Row i of ids / dist holds the first k, by
// (distance, id), of the points j != i that share a leaf with i in some tree; count[i] entries are
// valid, the rest are id -1, distance +inf.  Distances are metricDDL2's left fold (Internal.hs:403-406).
// accumulate: an earlier result over the same data set and k (another forest, a tree shard) whose
// entries join the candidates (RPT_GRAPH_ACCUMULATE); the order of folding does not matter.
struct GraphResult {
  int k = 0;
  std::vector<int32_t> ids;    // [n][k]
  std::vector<double> dist;    // [n][k]
  std::vector<int32_t> count;  // [n]
};
// knnGraph / knnGraphSV around their _host entry point: call(flags, ids, dist, count)
template <class Call>
inline GraphResult knnGraphVia(Call call, const RPForest& tts, int k, const GraphResult* accumulate) {
  const size_t n = (size_t)tts.data->n;
  GraphResult g;
  if (accumulate) {
    if (accumulate->k != k || accumulate->count.size() != n)
      throw RPTError(RPT_E_ARG, "accumulate: a result of another data set or k");
    g = *accumulate;
  }
  g.k = k;
  g.ids.resize(n * (size_t)(k > 0 ? k : 0) + 1);  // + 1: non-NULL pointers for an empty data set
  g.dist.resize(n * (size_t)(k > 0 ? k : 0) + 1);
  g.count.resize(n + 1);
  check(call(accumulate ? RPT_GRAPH_ACCUMULATE : 0, g.ids.data(), g.dist.data(), g.count.data()));
  g.ids.resize(n * (size_t)k);
  g.dist.resize(n * (size_t)k);
  g.count.resize(n);
  return g;
}
inline GraphResult knnGraph(const RPForest& tts, int k, const GraphResult* accumulate = nullptr) {
  return knnGraphVia(
      [&](int32_t flags, int32_t* ids, double* dist, int32_t* count) {
        return rpt_knn_graph_host(tts.ctx->get(), tts.get(), tts.data->get(), k, flags, ids, dist, count);
      },
      tts, k, accumulate);
}

// ... under another distance (rpt_knn_graph_metric_host): Metric::Cosine / Metric::Inner, the
// distances of RPT_KNN_METRIC_COSINE / _INNER bit for bit (the left-fold dot in double); Metric::L2
// gives knnGraph's bits.  accumulate must be a result under the same metric (not detected).
inline GraphResult knnGraph(const RPForest& tts, int k, Metric metric, const GraphResult* accumulate = nullptr) {
  return knnGraphVia(
      [&](int32_t flags, int32_t* ids, double* dist, int32_t* count) {
        return rpt_knn_graph_metric_host(tts.ctx->get(), tts.get(), tts.data->get(), k, metric_flags(metric), flags,
                                         ids, dist, count);
      },
      tts, k, accumulate);
}

// NN-descent rounds over a kNN graph (rpt_knn_graph_refine_host) -> the refined graph; `g` is not
// modified.  One round gives row i the first k, by (distance, id), of its neighbours, up to
// `reverse` of the points that list i (-1 = k, 0 = none) and all of their neighbours; a round
// that changes nothing ends the sequence.  Deterministic.  stats (optional): rounds applied, ids
// that entered a row, distances evaluated (rpt_knn_graph_refine_last).
struct RefineStats {
  int64_t rounds = 0, updates = 0, candidates = 0;
};
// knnGraphRefine / knnGraphRefineSV around their _host entry point: call(reverse, flags, ids, dist, count),
// reverse already resolved (-1 -> k)
template <class Call>
inline GraphResult knnGraphRefineVia(Call call, const char* who, Context& ctx, const Dataset& data,
                                     const GraphResult& g, int reverse, RefineStats* stats) {
  const size_t n = (size_t)data.n;
  if (g.count.size() != n || g.ids.size() != n * (size_t)(g.k > 0 ? g.k : 0) || g.dist.size() != g.ids.size())
    throw RPTError(RPT_E_ARG, std::string(who) + ": a graph of another data set or k");
  GraphResult out = g;
  out.ids.resize(out.ids.size() + 1);  // + 1: non-NULL pointers for an empty data set
  out.dist.resize(out.dist.size() + 1);
  out.count.resize(n + 1);
  check(call(reverse < 0 ? g.k : reverse, 0, out.ids.data(), out.dist.data(), out.count.data()));
  out.ids.resize(n * (size_t)g.k);
  out.dist.resize(n * (size_t)g.k);
  out.count.resize(n);
  if (stats) check(rpt_knn_graph_refine_last(ctx.get(), &stats->rounds, &stats->updates, &stats->candidates));
  return out;
}
inline GraphResult knnGraphRefine(Context& ctx, const Dataset& data, const GraphResult& g, int iters = 1,
                                  int reverse = -1, RefineStats* stats = nullptr) {
  return knnGraphRefineVia(
      [&](int32_t rev, int32_t flags, int32_t* ids, double* dist, int32_t* count) {
        return rpt_knn_graph_refine_host(ctx.get(), data.get(), g.k, rev, iters, flags, ids, dist, count);
      },
      "knnGraphRefine", ctx, data, g, reverse, stats);
}

// ... under another distance (rpt_knn_graph_refine_metric_host); the graph's stored distances must
// be that metric's (knnGraph's under the same Metric; another is not detected)
inline GraphResult knnGraphRefine(Context& ctx, const Dataset& data, const GraphResult& g, Metric metric,
                                  int iters = 1, int reverse = -1, RefineStats* stats = nullptr) {
  return knnGraphRefineVia(
      [&](int32_t rev, int32_t flags, int32_t* ids, double* dist, int32_t* count) {
        return rpt_knn_graph_refine_metric_host(ctx.get(), data.get(), g.k, rev, iters, metric_flags(metric), flags,
                                                ids, dist, count);
      },
      "knnGraphRefine", ctx, data, g, reverse, stats);
}

// knnGraph of a forest over SVector rows (rpt_knn_graph_csr_host).  The distances are metricDDL2's
// left fold over the dense-ified rows (absent columns +0.0), so the arrays are bit-equal to
// knnGraph's on the dense-ified data set with the same forest; the kernels visit only the 32-column
// windows in which a leaf holds a nonzero.  The rows' indices must ascend strictly.  L2 only.
inline GraphResult knnGraphSV(const RPForest& tts, int k, const GraphResult* accumulate = nullptr) {
  return knnGraphVia(
      [&](int32_t flags, int32_t* ids, double* dist, int32_t* count) {
        return rpt_knn_graph_csr_host(tts.ctx->get(), tts.get(), tts.data->get(), k, flags, ids, dist, count);
      },
      tts, k, accumulate);
}

// knnGraphRefine over SVector rows (rpt_knn_graph_refine_csr_host): the same rounds, the same
// statistics, bit-equal to knnGraphRefine on the dense-ified data set
inline GraphResult knnGraphRefineSV(Context& ctx, const Dataset& data, const GraphResult& g, int iters = 1,
                                    int reverse = -1, RefineStats* stats = nullptr) {
  return knnGraphRefineVia(
      [&](int32_t rev, int32_t flags, int32_t* ids, double* dist, int32_t* count) {
        return rpt_knn_graph_refine_csr_host(ctx.get(), data.get(), g.k, rev, iters, flags, ids, dist, count);
      },
      "knnGraphRefineSV", ctx, data, g, reverse, stats);
}

// knnGraphSV under another distance (rpt_knn_graph_csr_metric_host): Metric::Cosine / Metric::Inner
// over the indices both rows store (the left fold of the shared columns' products from +0.0, the
// definition knnBatch uses on SVector data); Metric::L2 gives knnGraphSV's bits.  While every stored
// value is finite that is knnGraph(tts, k, metric) on the dense-ified rows bit for bit; with a stored
// inf or NaN it is not, and the answer is this definition.  accumulate must be a result under the
// same metric (not detected).
inline GraphResult knnGraphSV(const RPForest& tts, int k, Metric metric, const GraphResult* accumulate = nullptr) {
  return knnGraphVia(
      [&](int32_t flags, int32_t* ids, double* dist, int32_t* count) {
        return rpt_knn_graph_csr_metric_host(tts.ctx->get(), tts.get(), tts.data->get(), k, metric_flags(metric),
                                             flags, ids, dist, count);
      },
      tts, k, accumulate);
}

// knnGraphRefineSV under another distance (rpt_knn_graph_refine_csr_metric_host); the graph's stored
// distances must be that metric's (knnGraphSV's under the same Metric; another is not detected)
inline GraphResult knnGraphRefineSV(Context& ctx, const Dataset& data, const GraphResult& g, Metric metric,
                                    int iters = 1, int reverse = -1, RefineStats* stats = nullptr) {
  return knnGraphRefineVia(
      [&](int32_t rev, int32_t flags, int32_t* ids, double* dist, int32_t* count) {
        return rpt_knn_graph_refine_csr_metric_host(ctx.get(), data.get(), g.k, rev, iters, metric_flags(metric),
                                                    flags, ids, dist, count);
      },
      "knnGraphRefineSV", ctx, data, g, reverse, stats);
}

// A kNN graph made ready for graphSearch (rpt_graph_prepare_host) -> a graph of kout columns; `g`
// is not modified.  diversify: walking a row in stored order, a neighbour is dropped when an
// already kept neighbour of the row is nearer to it than the point itself is (a plain <, the
// metric's fold bit for bit); reverse: every point that lists i after that joins row i at the
// distance stored there; the row is the first kout (-1 = min(64, 2 k)) of that set by (distance,
// id).  The metric must be the one the graph was built under; under Metric::Inner, which is no
// metric, diversify costs recall.  stats (optional): pair distances evaluated, entries dropped by
// diversify, entries cut off by kout (rpt_graph_prepare_last).
struct PrepareStats {
  int64_t pairs = 0, occluded = 0, capped = 0;
};
// graphPrepare / graphPrepareSV around their _host entry point
using GraphPrepareEntry = int32_t (*)(rpt_ctx*, const rpt_dataset*, int32_t, const int32_t*, const double*,
                                      const int32_t*, int32_t, int32_t, int32_t, int32_t*, double*, int32_t*);
inline GraphResult graphPrepareVia(GraphPrepareEntry entry, const char* who, Context& ctx, const Dataset& data,
                                   const GraphResult& g, int32_t metric, int kout, bool diversify, bool reverse,
                                   PrepareStats* stats) {
  const size_t n = (size_t)data.n;
  if (g.count.size() != n || g.ids.size() != n * (size_t)(g.k > 0 ? g.k : 0) || g.dist.size() != g.ids.size())
    throw RPTError(RPT_E_ARG, std::string(who) + ": a graph of another data set or k");
  if (kout < 0) kout = 2 * g.k < RPT_GRAPH_MAX_K ? 2 * g.k : RPT_GRAPH_MAX_K;
  if (kout < 1 || kout > RPT_GRAPH_MAX_K) throw RPTError(RPT_E_ARG, std::string(who) + ": kout must be in [1,64]");
  const int32_t none = -1;  // non-NULL pointers for an empty data set
  const double nod = 0.0;
  GraphResult out;
  out.k = kout;
  out.ids.resize(n * (size_t)kout + 1);
  out.dist.resize(n * (size_t)kout + 1);
  out.count.resize(n + 1);
  check(entry(ctx.get(), data.get(), g.k, n ? g.ids.data() : &none, n ? g.dist.data() : &nod,
              n ? g.count.data() : &none, kout, metric,
              (diversify ? RPT_GRAPH_PREP_DIVERSIFY : 0) | (reverse ? RPT_GRAPH_PREP_REVERSE : 0), out.ids.data(),
              out.dist.data(), out.count.data()));
  out.ids.resize(n * (size_t)kout);
  out.dist.resize(n * (size_t)kout);
  out.count.resize(n);
  if (stats) check(rpt_graph_prepare_last(ctx.get(), &stats->pairs, &stats->occluded, &stats->capped));
  return out;
}
inline GraphResult graphPrepare(Context& ctx, const Dataset& data, const GraphResult& g, Metric metric,
                                int kout = -1, bool diversify = true, bool reverse = true,
                                PrepareStats* stats = nullptr) {
  return graphPrepareVia(rpt_graph_prepare_host, "graphPrepare", ctx, data, g, metric_flags(metric), kout,
                         diversify, reverse, stats);
}
inline GraphResult graphPrepare(Context& ctx, const Dataset& data, const GraphResult& g, int kout = -1,
                                bool diversify = true, bool reverse = true, PrepareStats* stats = nullptr) {
  return graphPrepare(ctx, data, g, Metric::L2, kout, diversify, reverse, stats);
}

// graphPrepare over SVector rows under L2 (rpt_graph_prepare_csr_host): data is a CSR data set.  The
// pair distances of diversify are metricDDL2's left fold over the dense-ified rows, so the graph and
// the statistics are bit-equal to graphPrepare's on the dense-ified data set with the same graph.
// The rows' indices must ascend strictly.
inline GraphResult graphPrepareSV(Context& ctx, const Dataset& data, const GraphResult& g, int kout = -1,
                                  bool diversify = true, bool reverse = true, PrepareStats* stats = nullptr) {
  return graphPrepareVia(rpt_graph_prepare_csr_host, "graphPrepareSV", ctx, data, g, 0, kout, diversify, reverse,
                         stats);
}
// ... over the data set of a forest
inline GraphResult graphPrepareSV(const RPForest& tts, const GraphResult& g, int kout = -1, bool diversify = true,
                                  bool reverse = true, PrepareStats* stats = nullptr) {
  return graphPrepareSV(*tts.ctx, *tts.data, g, kout, diversify, reverse, stats);
}

// graphPrepareSV under another distance (rpt_graph_prepare_csr_metric_host): Metric::Cosine /
// Metric::Inner over the indices both rows store, as knnGraphSV(tts, k, metric) defines them, which
// must be the metric the graph's distances were computed under; Metric::L2 gives graphPrepareSV's
// bits.  While every stored value is finite that is graphPrepare(ctx, data, g, metric, ...) on the
// dense-ified rows bit for bit.  Under Metric::Inner diversify costs recall.
inline GraphResult graphPrepareSV(Context& ctx, const Dataset& data, const GraphResult& g, Metric metric,
                                  int kout = -1, bool diversify = true, bool reverse = true,
                                  PrepareStats* stats = nullptr) {
  return graphPrepareVia(rpt_graph_prepare_csr_metric_host, "graphPrepareSV", ctx, data, g, metric_flags(metric),
                         kout, diversify, reverse, stats);
}
// ... over the data set of a forest
inline GraphResult graphPrepareSV(const RPForest& tts, const GraphResult& g, Metric metric, int kout = -1,
                                  bool diversify = true, bool reverse = true, PrepareStats* stats = nullptr) {
  return graphPrepareSV(*tts.ctx, *tts.data, g, metric, kout, diversify, reverse, stats);
}

// Query a kNN graph: best-first beam search (rpt_graph_search_host).  g: a graph over `data`
// (knnGraph's, knnGraphRefine's; only ids and count are read), qs: dense queries of the data's d,
// seeds: [nq][s] start ids (s <= 64, -1 = unused slot), ef: entries of the beam (k <= ef <= 256).
// The seeds are offered to the beam, then the graph row of its first unexpanded entry, until none
// is left; the answer is the first k of the beam by (distance, id), unused slots id -1, distance
// +inf.  Distances are the metric's left fold in double (Metric::Cosine / Inner bit-equal to
// bruteKnn's).  stats (optional): entries expanded, distances computed (rpt_graph_search_last).
struct KnnResult {
  int k = 0;
  std::vector<int32_t> ids;    // [nq][k]
  std::vector<double> dist;    // [nq][k]
  std::vector<int32_t> count;  // [nq]
};
struct SearchStats {
  int64_t expansions = 0, evaluated = 0;
};
// graphSearch / graphSearchSV around their _host entry point: call(graph ids, graph count, seeds, flags,
// ids, dist, count)
template <class Call>
inline KnnResult graphSearchVia(Call call, const char* who, Context& ctx, const Dataset& data, const GraphResult& g,
                                const Dataset& qs, int k, const std::vector<int32_t>& seeds, int s,
                                SearchStats* stats) {
  const size_t n = (size_t)data.n, nq = (size_t)qs.n;
  if (g.count.size() != n || g.ids.size() != n * (size_t)(g.k > 0 ? g.k : 0))
    throw RPTError(RPT_E_ARG, std::string(who) + ": a graph of another data set");
  if (s < 1 || seeds.size() != nq * (size_t)s) throw RPTError(RPT_E_ARG, std::string(who) + ": seeds must be [nq][s]");
  const int32_t none = -1;  // non-NULL pointers for empty inputs
  KnnResult r;
  r.k = k;
  r.ids.resize(nq * (size_t)(k > 0 ? k : 0) + 1);
  r.dist.resize(nq * (size_t)(k > 0 ? k : 0) + 1);
  r.count.resize(nq + 1);
  check(call(n ? g.ids.data() : &none, n ? g.count.data() : &none, nq ? seeds.data() : &none, 0, r.ids.data(),
             r.dist.data(), r.count.data()));
  r.ids.resize(nq * (size_t)k);
  r.dist.resize(nq * (size_t)k);
  r.count.resize(nq);
  if (stats) check(rpt_graph_search_last(ctx.get(), &stats->expansions, &stats->evaluated));
  return r;
}
// the seeds a forest gives: the ids of its de-duplicated seed_k nearest candidates (entry: rpt_knn_host or
// rpt_knn_csr_metric_host, with RPT_KNN_DEDUP in flags), slots beyond that answer's count -1
inline std::vector<int32_t> forestSeeds(const RPForest& tts, const Dataset& qs, int seed_k, decltype(&rpt_knn_host) entry,
                                        int32_t flags, const char* who) {
  const size_t nq = (size_t)qs.n;
  if (seed_k < 1) throw RPTError(RPT_E_ARG, std::string(who) + ": seed_k must be at least 1");
  std::vector<int32_t> seeds(nq * (size_t)seed_k + 1), cnt(nq + 1);
  std::vector<double> dist(nq * (size_t)seed_k + 1);
  check(entry(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), seed_k, flags, seeds.data(), dist.data(),
              cnt.data()));
  seeds.resize(nq * (size_t)seed_k);
  for (size_t i = 0; i < nq; ++i)
    for (int e = cnt[i]; e < seed_k; ++e) seeds[i * (size_t)seed_k + (size_t)e] = -1;
  return seeds;
}
inline KnnResult graphSearch(Context& ctx, const Dataset& data, const GraphResult& g, const Dataset& qs, int k,
                             int ef, const std::vector<int32_t>& seeds, int s, Metric metric,
                             SearchStats* stats = nullptr) {
  return graphSearchVia(
      [&](const int32_t* gids, const int32_t* gcount, const int32_t* sd, int32_t flags, int32_t* ids, double* dist,
          int32_t* count) {
        return rpt_graph_search_host(ctx.get(), data.get(), qs.get(), g.k, gids, gcount, s, sd, k, ef,
                                     metric_flags(metric), flags, ids, dist, count);
      },
      "graphSearch", ctx, data, g, qs, k, seeds, s, stats);
}
inline KnnResult graphSearch(Context& ctx, const Dataset& data, const GraphResult& g, const Dataset& qs, int k,
                             int ef, const std::vector<int32_t>& seeds, int s, SearchStats* stats = nullptr) {
  return graphSearch(ctx, data, g, qs, k, ef, seeds, s, Metric::L2, stats);
}
// ... the seeds taken from a forest: the ids of its de-duplicated seed_k nearest candidates
// (rpt_knn_host with RPT_KNN_DEDUP under the same metric), slots beyond that answer's count -1
inline KnnResult graphSearch(const RPForest& tts, const GraphResult& g, const Dataset& qs, int k, int ef,
                             Metric metric = Metric::L2, int seed_k = 8, SearchStats* stats = nullptr) {
  return graphSearch(*tts.ctx, *tts.data, g, qs, k, ef,
                     forestSeeds(tts, qs, seed_k, rpt_knn_host, RPT_KNN_DEDUP | metric_flags(metric), "graphSearch"),
                     seed_k, metric, stats);
}

// graphSearch over SVector rows under L2 (rpt_graph_search_csr_host): data and qs are CSR data sets
// of one d and dtype.  The distances are metricDDL2's left fold over the dense-ified query and row,
// so the answer and the statistics are bit-equal to graphSearch's on the dense-ified data set and
// queries with the same graph and seeds.  The rows' indices must ascend strictly.
inline KnnResult graphSearchSV(Context& ctx, const Dataset& data, const GraphResult& g, const Dataset& qs, int k,
                               int ef, const std::vector<int32_t>& seeds, int s, SearchStats* stats = nullptr) {
  return graphSearchVia(
      [&](const int32_t* gids, const int32_t* gcount, const int32_t* sd, int32_t flags, int32_t* ids, double* dist,
          int32_t* count) {
        return rpt_graph_search_csr_host(ctx.get(), data.get(), qs.get(), g.k, gids, gcount, s, sd, k, ef, 0, flags,
                                         ids, dist, count);
      },
      "graphSearchSV", ctx, data, g, qs, k, seeds, s, stats);
}
// ... the seeds taken from a batch forest over the CSR set, as graphSearch takes them
inline KnnResult graphSearchSV(const RPForest& tts, const GraphResult& g, const Dataset& qs, int k, int ef,
                               int seed_k = 8, SearchStats* stats = nullptr) {
  return graphSearchSV(*tts.ctx, *tts.data, g, qs, k, ef,
                       forestSeeds(tts, qs, seed_k, rpt_knn_host, RPT_KNN_DEDUP, "graphSearchSV"), seed_k, stats);
}

// graphSearchSV under another distance (rpt_graph_search_csr_metric_host): Metric::Cosine /
// Metric::Inner over the indices both the query and the row store, as knnGraphSV(tts, k, metric)
// defines them (bit-equal to bruteKnn(ctx, data, qs, k, metric)'s); Metric::L2 gives graphSearchSV's
// bits.  While every stored value is finite that is graphSearch(..., metric) on the dense-ified data
// set and queries bit for bit.  A query without nonzeros is NaN from everything under Metric::Cosine
// and gets its answers ordered by id.
inline KnnResult graphSearchSV(Context& ctx, const Dataset& data, const GraphResult& g, const Dataset& qs,
                               Metric metric, int k, int ef, const std::vector<int32_t>& seeds, int s,
                               SearchStats* stats = nullptr) {
  return graphSearchVia(
      [&](const int32_t* gids, const int32_t* gcount, const int32_t* sd, int32_t flags, int32_t* ids, double* dist,
          int32_t* count) {
        return rpt_graph_search_csr_metric_host(ctx.get(), data.get(), qs.get(), g.k, gids, gcount, s, sd, k, ef,
                                                metric_flags(metric), flags, ids, dist, count);
      },
      "graphSearchSV", ctx, data, g, qs, k, seeds, s, stats);
}
// ... the seeds taken from a batch forest over the CSR set under the same metric (Metric::Cosine /
// Inner: rpt_knn_csr_metric_host with RPT_KNN_DEDUP)
inline KnnResult graphSearchSV(const RPForest& tts, const GraphResult& g, const Dataset& qs, Metric metric, int k,
                               int ef, int seed_k = 8, SearchStats* stats = nullptr) {
  return graphSearchSV(*tts.ctx, *tts.data, g, qs, metric, k, ef,
                       forestSeeds(tts, qs, seed_k, metric == Metric::L2 ? rpt_knn_host : rpt_knn_csr_metric_host,
                                   RPT_KNN_DEDUP | metric_flags(metric), "graphSearchSV"),
                       seed_k, stats);
}

// graphSearch among SOME of the points (rpt_graph_search_allow_host): `allow` holds ceil(n / 32)
// words, id i allowed when bit i & 31 of word i >> 5 is set (allowBitmap packs a mask); an empty
// vector allows every id.  data and qs are both dense or both CSR, under any Metric.  ef counts
// ALLOWED beam entries only; width in [ef, 1024] is the most entries the beam may hold, allowed or
// not (0 = min(1024, 8 * ef)); a beam with ef allowed entries ends at its ef-th allowed entry, and
// disallowed entries are expanded like any other.  The answer is the first k allowed entries.  With
// every id allowed it is graphSearch's / graphSearchSV's bit for bit; with width = ef it is the allowed
// entries of the unfiltered beam.
inline std::vector<uint32_t> allowBitmap(const std::vector<bool>& mask) {
  std::vector<uint32_t> words((mask.size() + 31) / 32, 0u);
  for (size_t i = 0; i < mask.size(); ++i)
    if (mask[i]) words[i >> 5] |= 1u << (i & 31);
  return words;
}
inline KnnResult graphSearchAllow(Context& ctx, const Dataset& data, const GraphResult& g, const Dataset& qs,
                                  const std::vector<uint32_t>& allow, int k, int ef, int width,
                                  const std::vector<int32_t>& seeds, int s, Metric metric = Metric::L2,
                                  SearchStats* stats = nullptr) {
  if (!allow.empty() && allow.size() != ((size_t)data.n + 31) / 32)
    throw RPTError(RPT_E_ARG, "graphSearchAllow: allow must hold ceil(n / 32) words (or none)");
  if (width == 0) width = std::min(RPT_GRAPH_SEARCH_MAX_WIDTH, 8 * ef);
  return graphSearchVia(
      [&](const int32_t* gids, const int32_t* gcount, const int32_t* sd, int32_t flags, int32_t* ids, double* dist,
          int32_t* count) {
        return rpt_graph_search_allow_host(ctx.get(), data.get(), qs.get(), g.k, gids, gcount, s, sd,
                                           allow.empty() ? nullptr : allow.data(), k, ef, width,
                                           metric_flags(metric), flags, ids, dist, count);
      },
      "graphSearchAllow", ctx, data, g, qs, k, seeds, s, stats);
}
// ... the seeds taken from a forest under the same metric, as graphSearch / graphSearchSV take them;
// seeds need not be allowed
inline KnnResult graphSearchAllow(const RPForest& tts, const GraphResult& g, const Dataset& qs,
                                  const std::vector<uint32_t>& allow, int k, int ef, int width = 0,
                                  Metric metric = Metric::L2, int seed_k = 8, SearchStats* stats = nullptr) {
  const bool csr_metric = tts.data->csr && metric != Metric::L2;
  return graphSearchAllow(*tts.ctx, *tts.data, g, qs, allow, k, ef, width,
                          forestSeeds(tts, qs, seed_k, csr_metric ? rpt_knn_csr_metric_host : rpt_knn_host,
                                      RPT_KNN_DEDUP | metric_flags(metric), "graphSearchAllow"),
                          seed_k, metric, stats);
}

// New rows into a kNN graph (rpt_graph_insert_host): `data` holds N = n + m rows whose LAST m are the
// new ones, g is a graph over the first n (its distances ARE read), dense or CSR rows under any Metric
// (the one g was built under).  The new rows are taken in chunks of `batch`; every row of a chunk is
// answered by graphSearch with k = g.k and this ef over the rows visible so far (the first n and the
// chunks before it, not its own chunk), the answer becomes the new row, and every row it names takes
// the new id at the same distance when that is among its first g.k by (distance, id).  seeds[m][s]
// (-1 = unused; a seed may name a row of an earlier chunk).  The result is a pure function of its
// inputs, bit for bit; m = 0 copies the graph.  A smaller batch links more (rows of one chunk do not
// see each other; knnGraphRefine afterwards links them), a larger one fills the device.
struct InsertStats {
  int64_t chunks = 0, evaluated = 0, offered = 0, accepted = 0;
};
inline GraphResult graphInsert(Context& ctx, const Dataset& data, const GraphResult& g, int64_t m, int ef,
                               int64_t batch, const std::vector<int32_t>& seeds, int s, Metric metric = Metric::L2,
                               InsertStats* stats = nullptr) {
  const size_t N = (size_t)data.n, n = N - (size_t)m;
  if (m < 0 || (size_t)m > N || g.count.size() != n || g.ids.size() != n * (size_t)(g.k > 0 ? g.k : 0) ||
      g.dist.size() != g.ids.size())
    throw RPTError(RPT_E_ARG, "graphInsert: the graph must be over the first n = N - m rows of data");
  if (s < 1 || seeds.size() != (size_t)m * (size_t)s) throw RPTError(RPT_E_ARG, "graphInsert: seeds must be [m][s]");
  const int32_t none = -1;  // non-NULL pointers for empty inputs
  const double nod = 0.0;
  const size_t k = (size_t)(g.k > 0 ? g.k : 0);
  GraphResult r;
  r.k = g.k;
  r.ids.resize(N * k + 1);
  r.dist.resize(N * k + 1);
  r.count.resize(N + 1);
  check(rpt_graph_insert_host(ctx.get(), data.get(), g.k, n ? g.ids.data() : &none, n ? g.dist.data() : &nod,
                              n ? g.count.data() : &none, m, s, m ? seeds.data() : &none, ef, batch,
                              metric_flags(metric), 0, r.ids.data(), r.dist.data(), r.count.data()));
  r.ids.resize(N * k);
  r.dist.resize(N * k);
  r.count.resize(N);
  if (stats)
    check(rpt_graph_insert_last(ctx.get(), &stats->chunks, &stats->evaluated, &stats->offered, &stats->accepted));
  return r;
}
// ... the seeds taken from a forest over the OLD n rows: `fresh` holds the m new rows alone (the last
// m rows of data once more), batch 0 = min(m, 4096) (kept after tools/graph_insert_times.py's sweep)
inline GraphResult graphInsert(const RPForest& old, const Dataset& data, const Dataset& fresh, const GraphResult& g,
                               int ef, int64_t batch = 0, Metric metric = Metric::L2, int seed_k = 8,
                               InsertStats* stats = nullptr) {
  const bool csr_metric = old.data->csr && metric != Metric::L2;
  if (batch == 0) batch = std::max<int64_t>(1, std::min<int64_t>(fresh.n, 4096));
  return graphInsert(*old.ctx, data, g, fresh.n, ef, batch,
                     forestSeeds(old, fresh, seed_k, csr_metric ? rpt_knn_csr_metric_host : rpt_knn_host,
                                 RPT_KNN_DEDUP | metric_flags(metric), "graphInsert"),
                     seed_k, metric, stats);
}

// Rows out of a kNN graph (rpt_graph_delete_host): `keep` holds the ceil(n / 32) words of allowBitmap (a
// set bit = the row STAYS; the tombstone bitmap graphSearchAllow takes, unchanged; empty = every row
// stays), g is a graph over data's n rows (its distances ARE read), dense or CSR rows under any Metric
// (the one g was built under).  The deleted rows are dropped; a kept row that named one becomes the
// first g.k by (distance, id) of its kept entries, at their stored distances, and the kept neighbours of
// its deleted neighbours, at their distance to the row (one hop: a row whose neighbours and all their
// neighbours are gone ends short, and knnGraphRefine afterwards repairs it).  compact: the survivors are
// renumbered densely, newid[i] = the number of kept rows below i or -1, and the result has popcount(keep)
// rows; otherwise it has n rows in old ids, deleted rows empty, newid[i] = i or -1, and is searchable
// with the unchanged data set.  A pure function of its inputs, bit for bit.
struct DeleteStats {
  int64_t kept = 0, touched = 0, evaluated = 0, dropped = 0;
};
struct DeleteResult {
  GraphResult graph;
  std::vector<int32_t> newid;  // [n]
};
inline DeleteResult graphDelete(Context& ctx, const Dataset& data, const GraphResult& g,
                                const std::vector<uint32_t>& keep, bool compact, Metric metric,
                                DeleteStats* stats = nullptr) {
  const size_t n = (size_t)data.n, k = (size_t)(g.k > 0 ? g.k : 0);
  if (g.count.size() != n || g.ids.size() != n * k || g.dist.size() != g.ids.size())
    throw RPTError(RPT_E_ARG, "graphDelete: the graph must be over the n rows of data");
  if (!keep.empty() && keep.size() != (n + 31) / 32)
    throw RPTError(RPT_E_ARG, "graphDelete: keep must hold ceil(n / 32) words (or none)");
  DeleteResult r;
  r.graph.k = g.k;
  r.graph.ids.resize(n * k + 1);
  r.graph.dist.resize(n * k + 1);
  r.graph.count.resize(n + 1);
  r.newid.resize(n + 1);
  check(rpt_graph_delete_host(ctx.get(), data.get(), g.k, g.ids.data(), g.dist.data(), g.count.data(),
                              keep.empty() ? nullptr : keep.data(), metric_flags(metric),
                              compact ? RPT_GRAPH_DELETE_COMPACT : 0, r.graph.ids.data(), r.graph.dist.data(),
                              r.graph.count.data(), r.newid.data()));
  r.newid.resize(n);
  size_t rows = n;
  if (compact) {
    rows = 0;
    for (int32_t v : r.newid) rows += v >= 0;
  }
  r.graph.ids.resize(rows * k);
  r.graph.dist.resize(rows * k);
  r.graph.count.resize(rows);
  if (stats)
    check(rpt_graph_delete_last(ctx.get(), &stats->kept, &stats->touched, &stats->evaluated, &stats->dropped));
  return r;
}
inline DeleteResult graphDelete(Context& ctx, const Dataset& data, const GraphResult& g,
                                const std::vector<uint32_t>& keep, bool compact = true,
                                DeleteStats* stats = nullptr) {
  return graphDelete(ctx, data, g, keep, compact, Metric::L2, stats);
}

struct BruteResult {
  std::vector<int32_t> ids;  // [nq][k], -1 = unused slot
  std::vector<double> dist;  // [nq][k]
};
inline BruteResult bruteKnn(Context& ctx, const Dataset& data, const Dataset& qs, int k, int32_t flags = 0) {
  BruteResult r{std::vector<int32_t>((size_t)qs.n * k + 1), std::vector<double>((size_t)qs.n * k + 1)};
  check(rpt_brute_knn_metric_host(ctx.get(), data.get(), qs.get(), k, flags, r.ids.data(), r.dist.data()));
  r.ids.resize((size_t)qs.n * k);
  r.dist.resize((size_t)qs.n * k);
  return r;
}
// ... under a Metric, dense or SVector data (SVector rows under Cosine / Inner:
// rpt_brute_knn_csr_metric_host, the distance over the indices both vectors store)
inline BruteResult bruteKnn(Context& ctx, const Dataset& data, const Dataset& qs, int k, Metric metric) {
  if (!data.csr || metric == Metric::L2) return bruteKnn(ctx, data, qs, k, metric_flags(metric));
  BruteResult r{std::vector<int32_t>((size_t)qs.n * k + 1), std::vector<double>((size_t)qs.n * k + 1)};
  check(rpt_brute_knn_csr_metric_host(ctx.get(), data.get(), qs.get(), k, metric_flags(metric), r.ids.data(),
                                      r.dist.data()));
  r.ids.resize((size_t)qs.n * k);
  r.dist.resize((size_t)qs.n * k);
  return r;
}
// hits[i][t] = |candidates(tree t, query i) n true kNN of query i|, truth (optional) [nq][k]
inline std::vector<int32_t> recallHits(const RPForest& tts, int k, const Dataset& qs, int32_t flags = 0,
                                       std::vector<int32_t>* truth = nullptr) {
  std::vector<int32_t> hits((size_t)qs.n * tts.T + 1);
  if (truth) truth->assign((size_t)qs.n * k + 1, -1);
  check(rpt_recall_hits_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), k, flags, hits.data(),
                             truth ? truth->data() : nullptr));
  hits.resize((size_t)qs.n * tts.T);
  if (truth) truth->resize((size_t)qs.n * k);
  return hits;
}
// per query: mean over the trees of hits / k, summed in tree order (RPTree.hs:276-282)
inline std::vector<double> recallWithBatch(const RPForest& tts, int k, const Dataset& qs, int32_t flags = 0) {
  const std::vector<int32_t> hits = recallHits(tts, k, qs, flags);
  std::vector<double> out((size_t)qs.n);
  for (int64_t i = 0; i < qs.n; ++i) {
    double acc = 0.0;
    for (int t = 0; t < tts.T; ++t) acc += (double)hits[(size_t)i * tts.T + t] / (double)k;
    out[(size_t)i] = acc / (double)tts.T;
  }
  return out;
}
// ... under a Metric, dense or SVector forests (SVector rows under Cosine / Inner:
// rpt_recall_hits_csr_metric_host)
inline std::vector<int32_t> recallHits(const RPForest& tts, int k, const Dataset& qs, Metric metric,
                                       std::vector<int32_t>* truth = nullptr) {
  if (!tts.data->csr || metric == Metric::L2) return recallHits(tts, k, qs, metric_flags(metric), truth);
  std::vector<int32_t> hits((size_t)qs.n * tts.T + 1);
  if (truth) truth->assign((size_t)qs.n * k + 1, -1);
  check(rpt_recall_hits_csr_metric_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(), k,
                                        metric_flags(metric), hits.data(), truth ? truth->data() : nullptr));
  hits.resize((size_t)qs.n * tts.T);
  if (truth) truth->resize((size_t)qs.n * k);
  return hits;
}
inline std::vector<double> recallWithBatch(const RPForest& tts, int k, const Dataset& qs, Metric metric) {
  const std::vector<int32_t> hits = recallHits(tts, k, qs, metric);
  std::vector<double> out((size_t)qs.n);
  for (int64_t i = 0; i < qs.n; ++i) {
    double acc = 0.0;
    for (int t = 0; t < tts.T; ++t) acc += (double)hits[(size_t)i * tts.T + t] / (double)k;
    out[(size_t)i] = acc / (double)tts.T;
  }
  return out;
}
inline double recallWith(const RPForest& tts, int k, const SVector& q, Metric metric) {
  std::vector<SVector> qv{q};
  Dataset qs(*tts.ctx, qv, tts.data->d);
  return recallWithBatch(tts, k, qs, metric)[0];
}
inline double recallWith(const RPForest& tts, int k, const DVector& q, Metric metric = Metric::L2) {
  std::vector<DVector> qv{q};
  Dataset qs(*tts.ctx, qv);
  return recallWithBatch(tts, k, qs, metric_flags(metric))[0];
}
inline double recallWith(const RPForest& tts, int k, const SVector& q, bool reference_metric = false) {
  std::vector<SVector> qv{q};
  Dataset qs(*tts.ctx, qv, tts.data->d);
  return recallWithBatch(tts, k, qs, reference_metric ? RPT_KNN_METRIC_REFERENCE : 0)[0];
}

// ---- an allow-list on the forest query and on the exhaustive kNN (rpt_knn_allow_host,
// rpt_allow_candidates_host, rpt_brute_knn_allow_host, rpt_recall_hits_allow_host) ----
// `allow`: the ceil(n / 32) words of allowBitmap (an empty vector allows every id); one list serves
// every query.  A query's candidate list loses its disallowed entries, order and duplicates kept, and
// is ranked as knn ranks it, the duplicate rule (dedup: RPT_KNN_KEEP_DUPLICATES, RPT_KNN_DEDUP,
// RPT_KNN_DEDUP_DISTANCE) seeing allowed entries only.  Every row layout and Metric; flags may add
// RPT_KNN_METRIC_REFERENCE on SVector rows under Metric::L2.
inline const uint32_t* allowWords(const std::vector<uint32_t>& allow, int64_t n, const char* who) {
  if (!allow.empty() && allow.size() != ((size_t)n + 31) / 32)
    throw RPTError(RPT_E_ARG, std::string(who) + ": allow must hold ceil(n / 32) words (or none)");
  return allow.empty() ? nullptr : allow.data();
}
inline KnnResult knnAllow(const RPForest& tts, const std::vector<uint32_t>& allow, int k, const Dataset& qs,
                          int32_t dedup = RPT_KNN_KEEP_DUPLICATES, Metric metric = Metric::L2, int32_t flags = 0) {
  KnnResult r{k, std::vector<int32_t>((size_t)qs.n * k + 1), std::vector<double>((size_t)qs.n * k + 1),
              std::vector<int32_t>((size_t)qs.n + 1)};
  check(rpt_knn_allow_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(),
                           allowWords(allow, tts.data->n, "knnAllow"), k, dedup | metric_flags(metric) | flags,
                           r.ids.data(), r.dist.data(), r.count.data()));
  r.ids.resize((size_t)qs.n * k);
  r.dist.resize((size_t)qs.n * k);
  r.count.resize((size_t)qs.n);
  return r;
}
// the allowed lists themselves: list i = ids[off[i] .. off[i + 1])
inline std::vector<int32_t> allowCandidates(const RPForest& tts, const std::vector<uint32_t>& allow,
                                            const Dataset& qs, std::vector<int64_t>* off = nullptr) {
  const uint32_t* w = allowWords(allow, tts.data->n, "allowCandidates");
  std::vector<int64_t> o((size_t)qs.n + 1);
  int64_t total = 0;
  check(rpt_allow_candidates_host(tts.ctx->get(), tts.get(), qs.get(), w, o.data(), nullptr, 0, &total));
  std::vector<int32_t> ids((size_t)(total > 0 ? total : 1));
  check(rpt_allow_candidates_host(tts.ctx->get(), tts.get(), qs.get(), w, o.data(), ids.data(), total, &total));
  ids.resize((size_t)total);
  if (off) *off = o;
  return ids;
}
// the k best ALLOWED rows by (distance, id); flags: RPT_KNN_METRIC_REFERENCE on SVector rows, or 0
inline BruteResult bruteKnnAllow(Context& ctx, const Dataset& data, const std::vector<uint32_t>& allow,
                                 const Dataset& qs, int k, Metric metric = Metric::L2, int32_t flags = 0) {
  BruteResult r{std::vector<int32_t>((size_t)qs.n * k + 1), std::vector<double>((size_t)qs.n * k + 1)};
  check(rpt_brute_knn_allow_host(ctx.get(), data.get(), qs.get(), allowWords(allow, data.n, "bruteKnnAllow"), k,
                                 metric_flags(metric) | flags, r.ids.data(), r.dist.data()));
  r.ids.resize((size_t)qs.n * k);
  r.dist.resize((size_t)qs.n * k);
  return r;
}
// recallHits with the truth taken among the allowed rows (bruteKnnAllow's ids)
inline std::vector<int32_t> recallHitsAllow(const RPForest& tts, const std::vector<uint32_t>& allow, int k,
                                            const Dataset& qs, Metric metric = Metric::L2, int32_t flags = 0,
                                            std::vector<int32_t>* truth = nullptr) {
  std::vector<int32_t> hits((size_t)qs.n * tts.T + 1);
  if (truth) truth->assign((size_t)qs.n * k + 1, -1);
  check(rpt_recall_hits_allow_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(),
                                   allowWords(allow, tts.data->n, "recallHitsAllow"), k, metric_flags(metric) | flags,
                                   hits.data(), truth ? truth->data() : nullptr));
  hits.resize((size_t)qs.n * tts.T);
  if (truth) truth->resize((size_t)qs.n * k);
  return hits;
}

// ---- allow-lists per query group (rpt_*_allow_group_host): many tenants in one batch ----
// graphSearchAllowGroup, knnAllowGroup, allowGroupCandidates, bruteKnnAllowGroup and recallHitsAllowGroup
// take (allow, G, group) where graphSearchAllow, knnAllow, ... take `allow`: G bitmaps of
// ceil(n / 32) words each, one after the other (allowBitmaps packs masks), and one group entry per
// query; query q is answered under bitmap group[q], -1 = every id.  The answer of query q is what the
// single-bitmap function gives that query under its bitmap, bit for bit.  A group entry outside
// [-1, G) is refused (RPT_E_ARG).
inline std::vector<uint32_t> allowBitmaps(const std::vector<std::vector<bool>>& masks) {
  std::vector<uint32_t> words;
  for (const std::vector<bool>& m : masks) {
    const std::vector<uint32_t> w = allowBitmap(m);
    words.insert(words.end(), w.begin(), w.end());
  }
  return words;
}
inline const uint32_t* allowGroupWords(const std::vector<uint32_t>& allow, int G, const std::vector<int32_t>& group,
                                       int64_t n, int64_t nq, const char* who) {
  if (G < 0 || allow.size() != (size_t)G * (((size_t)n + 31) / 32))
    throw RPTError(RPT_E_ARG, std::string(who) + ": allow must hold G rows of ceil(n / 32) words");
  if (group.size() != (size_t)nq) throw RPTError(RPT_E_ARG, std::string(who) + ": group must hold one entry per query");
  static const uint32_t no_rows = 0;  // G bitmaps of no words (n = 0) are still not a null allow
  return G == 0 ? nullptr : allow.empty() ? &no_rows : allow.data();
}
inline KnnResult graphSearchAllowGroup(Context& ctx, const Dataset& data, const GraphResult& g, const Dataset& qs,
                                  const std::vector<uint32_t>& allow, int G, const std::vector<int32_t>& group, int k,
                                  int ef, int width, const std::vector<int32_t>& seeds, int s,
                                  Metric metric = Metric::L2, SearchStats* stats = nullptr) {
  const uint32_t* w = allowGroupWords(allow, G, group, data.n, qs.n, "graphSearchAllowGroup");
  if (width == 0) width = std::min(RPT_GRAPH_SEARCH_MAX_WIDTH, 8 * ef);
  return graphSearchVia(
      [&](const int32_t* gids, const int32_t* gcount, const int32_t* sd, int32_t flags, int32_t* ids, double* dist,
          int32_t* count) {
        return rpt_graph_search_allow_group_host(ctx.get(), data.get(), qs.get(), g.k, gids, gcount, s, sd, w, G,
                                                 group.data(), k, ef, width, metric_flags(metric), flags, ids, dist,
                                                 count);
      },
      "graphSearchAllowGroup", ctx, data, g, qs, k, seeds, s, stats);
}
// ... the seeds taken from a forest under the same metric (unfiltered: seeds need not be allowed)
inline KnnResult graphSearchAllowGroup(const RPForest& tts, const GraphResult& g, const Dataset& qs,
                                  const std::vector<uint32_t>& allow, int G, const std::vector<int32_t>& group, int k,
                                  int ef, int width = 0, Metric metric = Metric::L2, int seed_k = 8,
                                  SearchStats* stats = nullptr) {
  const bool csr_metric = tts.data->csr && metric != Metric::L2;
  return graphSearchAllowGroup(*tts.ctx, *tts.data, g, qs, allow, G, group, k, ef, width,
                          forestSeeds(tts, qs, seed_k, csr_metric ? rpt_knn_csr_metric_host : rpt_knn_host,
                                      RPT_KNN_DEDUP | metric_flags(metric), "graphSearchAllowGroup"),
                          seed_k, metric, stats);
}
inline KnnResult knnAllowGroup(const RPForest& tts, const std::vector<uint32_t>& allow, int G,
                          const std::vector<int32_t>& group, int k, const Dataset& qs,
                          int32_t dedup = RPT_KNN_KEEP_DUPLICATES, Metric metric = Metric::L2, int32_t flags = 0) {
  KnnResult r{k, std::vector<int32_t>((size_t)qs.n * k + 1), std::vector<double>((size_t)qs.n * k + 1),
              std::vector<int32_t>((size_t)qs.n + 1)};
  check(rpt_knn_allow_group_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(),
                                 allowGroupWords(allow, G, group, tts.data->n, qs.n, "knnAllowGroup"), G, group.data(), k,
                                 dedup | metric_flags(metric) | flags, r.ids.data(), r.dist.data(), r.count.data()));
  r.ids.resize((size_t)qs.n * k);
  r.dist.resize((size_t)qs.n * k);
  r.count.resize((size_t)qs.n);
  return r;
}
inline std::vector<int32_t> allowGroupCandidates(const RPForest& tts, const std::vector<uint32_t>& allow, int G,
                                            const std::vector<int32_t>& group, const Dataset& qs,
                                            std::vector<int64_t>* off = nullptr) {
  const uint32_t* w = allowGroupWords(allow, G, group, tts.data->n, qs.n, "allowGroupCandidates");
  std::vector<int64_t> o((size_t)qs.n + 1);
  int64_t total = 0;
  check(rpt_allow_group_candidates_host(tts.ctx->get(), tts.get(), qs.get(), w, G, group.data(), o.data(), nullptr, 0,
                                        &total));
  std::vector<int32_t> ids((size_t)(total > 0 ? total : 1));
  check(rpt_allow_group_candidates_host(tts.ctx->get(), tts.get(), qs.get(), w, G, group.data(), o.data(), ids.data(),
                                        total, &total));
  ids.resize((size_t)total);
  if (off) *off = o;
  return ids;
}
inline BruteResult bruteKnnAllowGroup(Context& ctx, const Dataset& data, const std::vector<uint32_t>& allow, int G,
                                 const std::vector<int32_t>& group, const Dataset& qs, int k,
                                 Metric metric = Metric::L2, int32_t flags = 0) {
  BruteResult r{std::vector<int32_t>((size_t)qs.n * k + 1), std::vector<double>((size_t)qs.n * k + 1)};
  check(rpt_brute_knn_allow_group_host(ctx.get(), data.get(), qs.get(),
                                       allowGroupWords(allow, G, group, data.n, qs.n, "bruteKnnAllowGroup"), G,
                                       group.data(), k, metric_flags(metric) | flags, r.ids.data(), r.dist.data()));
  r.ids.resize((size_t)qs.n * k);
  r.dist.resize((size_t)qs.n * k);
  return r;
}
inline std::vector<int32_t> recallHitsAllowGroup(const RPForest& tts, const std::vector<uint32_t>& allow, int G,
                                            const std::vector<int32_t>& group, int k, const Dataset& qs,
                                            Metric metric = Metric::L2, int32_t flags = 0,
                                            std::vector<int32_t>* truth = nullptr) {
  std::vector<int32_t> hits((size_t)qs.n * tts.T + 1);
  if (truth) truth->assign((size_t)qs.n * k + 1, -1);
  check(rpt_recall_hits_allow_group_host(tts.ctx->get(), tts.get(), tts.data->get(), qs.get(),
                                         allowGroupWords(allow, G, group, tts.data->n, qs.n, "recallHitsAllowGroup"), G,
                                         group.data(), k, metric_flags(metric) | flags, hits.data(),
                                         truth ? truth->data() : nullptr));
  hits.resize((size_t)qs.n * tts.T);
  if (truth) truth->resize((size_t)qs.n * k);
  return hits;
}

}  // namespace rptree
