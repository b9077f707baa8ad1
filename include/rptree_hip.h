/*
 * rptree_hip.h — C ABI of the MI355X (gfx950) implementation of rp-tree's random-projection
 * hot path.  This is the drop-in boundary: the entry points are what a Haskell
 * `foreign import ccall` layer under the unchanged Data.RPTree API binds.
 *
 * The reference (ocramz/rp-tree v0.7.1) is closed pure Haskell with no FFI or plugin
 * interface; each entry point therefore names the reference FUNCTION it
 * replaces (file:line relative to the reference checkout).
 *
 * Conventions
 *   - Plain C: opaque handles, raw pointers, sizes.  No torch / C++ types.
 *   - Every function returns an int32 status: 0 = ok, negative = error (RPT_E_*).
 *     rpt_last_error() returns a message for the calling thread.  Nothing throws or aborts
 *     across the ABI: every entry point catches C++ exceptions of its host-side planners
 *     (std::bad_alloc -> RPT_E_NOMEM, anything else -> RPT_E_INTERNAL).  There is NO CPU fallback: without a usable HIP device every compute
 *     entry point fails with RPT_E_HIP.
 *   - Ownership: the caller owns every host buffer it passes or receives.  The library owns
 *     device memory behind the opaque handles; release it with the matching *_free.
 *   - Pointers named *_host are host memory, *_dev are device (HBM) addresses of the ctx's
 *     device, e.g. torch tensor .data_ptr() values.
 *   - Threading: re-entrant per rpt_ctx (one ctx = one device + one stream); a ctx is not
 *     thread-safe.  All work of a ctx is enqueued on its stream; entry points that return
 *     host data synchronise that stream, *_dev entry points do not (call rpt_ctx_sync).
 *
 * Flat forest layout (identical to oracle/rptree_oracle.h):
 *   perm[T][N]  int32   point ids; per tree the concatenation of the leaf buckets in
 *                       left-to-right order, each bucket in the reference's order
 *                       (Internal.hs:495,504-505: children inherit the stably sorted order).
 *   thr, mglo, mghi  double [T][2^L-1], heap order (root 0, children 2h+1, 2h+2); NaN where
 *                       the slot is not a Bin.  = _rpThreshold / _rpMargin of `RPT`
 *                       (Internal.hs:139-145), values per Internal.hs:496-501.
 *   The topology (Bin vs Tip, every node's offset and size) is a pure function of
 *   (N, minLeaf, maxDepth): Internal.hs:289 and :495,503; rpt_topology() enumerates it.
 */
#ifndef RPTREE_HIP_H
#define RPTREE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPT_ABI_VERSION 1

/* status codes */
#define RPT_OK 0
#define RPT_E_ARG (-1)      /* invalid argument */
#define RPT_E_HIP (-2)      /* HIP runtime / device error (incl. no device) */
#define RPT_E_NOMEM (-3)    /* host or device allocation failed */
#define RPT_E_UNSUPPORTED (-4)
#define RPT_E_INTERNAL (-5)

/* element types of datasets / queries */
#define RPT_F64 0           /* the reference's only type (Double) */
#define RPT_F32 1           /* build extension */
#define RPT_BF16 2          /* build extension */

/* projection modes (rpt_project, rpt_forest_build flags) */
#define RPT_PROJ_AUTO 0     /* f64 data: EXACT; f32/bf16 data: MFMA */
#define RPT_PROJ_EXACT 1    /* f64 VALU, the reference's summation order and no FMA
                               (Internal.hs:382): bit-identical to innerSD/innerSS */
#define RPT_PROJ_MFMA 2     /* MFMA tiles (f64/f32/bf16 inputs), k-ordered fma chain:
                               within 1e-5*|x||r| of the reference value.  CSR rows: dense-ified
                               as two bf16 terms on the bf16 matrix pipe (from 65 536 rows on,
                               d % 8 == 0), else the exact-order kernel with ONE fused
                               multiply-add per term instead of the reference's two roundings
                               (same tolerance) */

/* knn flags */
#define RPT_KNN_KEEP_DUPLICATES 0 /* the reference: RPTree.hs:174-176 never de-duplicates */
#define RPT_KNN_DEDUP 1           /* extension: each point id at most once */
#define RPT_KNN_DEDUP_DISTANCE 2  /* knnPQ (RPTree.hs:181-194): `nub` keeps one entry per DISTANCE */
/* Voting (the MRPT vote threshold; the reference carries it as the commented-out `counts` /
 * `keepCounts` sketch, RPTree.hs:464-478): only the points found in at least v of the trees'
 * candidate lists get a distance; they are taken in ascending id order (the order of
 * M.foldrWithKey in keepCounts), each once, and the k best by (distance, id) are returned.
 * Dense data, k <= 64; or-ed into the knn flags: RPT_KNN_VOTE(v), v in [1, 65535]. */
#define RPT_KNN_VOTE(v) ((int32_t)(v) << 8)
/* SVector (CSR) data: distances by the reference's own metricSSL2 (Internal.hs:389-393 over diffSS /
 * binSS :435-450) — the merge of the two index lists STOPS when either vector is exhausted, so the
 * tail of the longer one is silently dropped — instead of the true Euclidean
 * distance, for results identical to `knn metricL2` of the reference on SVector data.  Bit-exact
 * (left fold in merge order); one thread per candidate, general query path.  Ignored for dense
 * data (metricDDL2 is what they get anyway). */
#define RPT_KNN_METRIC_REFERENCE (1 << 24)
/* Cosine and inner-product distances (the reference's `knn distf` with another distf, RPTree.hs:
 * 168-176; the forest only decides which points are candidates, the metric only ranks them).  Dense
 * data (f64, f32, bf16 rows); every quantity in double, f32 / bf16 elements widened exactly; with
 * dot(x, q) = innerDD (Internal.hs:384-385), the left fold ((0 + x0 q0) + x1 q1) + ... from +0.0,
 * every product and sum rounded on its own (no FMA):
 *   RPT_KNN_METRIC_INNER : dist = -dot(x, q)                          (maximum inner product)
 *   RPT_KNN_METRIC_COSINE: dist = 1 - dot(x, q) / (sqrt(dot(x, x)) * sqrt(dot(q, q)))
 * with correctly rounded sqrt and division; smaller is nearer; a zero row or query gives NaN, and
 * NaN ranks behind every number, NaNs among themselves by candidate position.  The answer is
 * exactly that definition: ALL candidates ranked by (distance, candidate position), the duplicate
 * rule applied to those distances, the first k.  Candidates are ranked first on a lane-parallel f64
 * dot; the entries of the best k + 8 different rows are evaluated again as the fold, and the cut is
 * certified with a rounding bound of the two sums (within (2d + 16) u of each other for cosine,
 * (2d + 8) u |q| max|x| for the inner product, u = 2^-53).  A query whose cut cannot be certified
 * (ties or cancellation near the k-th distance, a zero or NaN query, k near 1024) is answered again
 * by an exact kernel that evaluates every candidate as the fold; rpt_knn_last_uncertified counts
 * those queries, the context option knn_metric_exact sends every query there.  Unlike L2 on f32 /
 * bf16 rows the values are f64 for every dtype.  Or-ed into the knn flags; at most one of the two, not with
 * RPT_KNN_METRIC_REFERENCE (RPT_E_ARG); CSR data and RPT_KNN_VOTE: RPT_E_UNSUPPORTED.  Not for
 * knnH (rpt_knnh_host has no flags).
 * Memory note: the first cosine or inner-product call on a dataset caches its rows' dot(x, x) on the
 * device, 8 bytes per row, freed with the dataset (a dataset borrowed with rpt_dataset_dense_dev must not change
 * while the library holds it). */
#define RPT_KNN_METRIC_COSINE (1 << 25)
#define RPT_KNN_METRIC_INNER (1 << 26)

typedef struct rpt_ctx rpt_ctx;
typedef struct rpt_dataset rpt_dataset;
typedef struct rpt_forest rpt_forest;

/* ---- library / context ---- */
int32_t rpt_abi_version(void);
const char* rpt_last_error(void);
int32_t rpt_device_count(int32_t* count);
int32_t rpt_ctx_create(int32_t device, rpt_ctx** out);
int32_t rpt_ctx_destroy(rpt_ctx* ctx);
int32_t rpt_ctx_sync(rpt_ctx* ctx);
/* device buffers released by the library are cached for reuse (multi-GB hipMalloc/hipFree per
 * build is slow); rpt_ctx_trim returns the cache to the driver (rpt_ctx_destroy does too). */
int32_t rpt_ctx_trim(rpt_ctx* ctx);
/* Allocator debugging aid.  RPT_POOL_POISON=<byte> in the environment (read once, at library load)
 * fills every block the library's device allocator hands out with that byte, so that a kernel
 * reading scratch nobody wrote computes garbage instead of passing by luck; RPT_NO_POOL wins over
 * it.  The probe allocates nbytes (> 0) the way the kernels' scratch is allocated, copies them to
 * out_host, frees the block and synchronises; *poison is the byte in force, -1 when poison is off. */
int32_t rpt_debug_pool_probe(rpt_ctx* ctx, int64_t nbytes, uint8_t* out_host, int32_t* poison);
/* the hipStream_t all work of this ctx is enqueued on (for HIP-event timing by the caller) */
int32_t rpt_ctx_stream(rpt_ctx* ctx, void** hip_stream);

/* Algorithm switches of a context.  They exist for the parity tests of the fallback paths and
 * for A/B timing; every default is the tuned path and results never depend on them (beyond the
 * documented tolerances of the MFMA projections).  rpt_ctx_create seeds them ONCE from the
 * environment (RPT_<NAME>, upper case); no entry point reads the environment afterwards.
 *   no_stream, stream_maxnodes, stream_minper, no_wmid, no_midselect, stream_big_node, no_wsub,
 *   no_wsort, no_wpack, no_csub, no_codes, no_pcodes
 *       median split: which regime handles which level
 *   proj_narrow, proj_bf16_f32     projection: 32 hyperplanes per pass only / bf16 rows on the f32 pipe
 *   proj_bf16_terms (3), proj_bf16_codes, proj_csr_nodense
 *       bf16 rows meet every hyperplane as TWO bf16 terms (|error| <= 2^-17 |x||r| by construction,
 *       inside RPT_PROJ_MFMA's 1e-5); 3 keeps a third term (f32-level agreement, a third more
 *       matrix-pipe work) / codes from the bf16 kernel's epilogue / CSR rows stay on the segmented kernel
 *   knn_wave (-1 auto, 0, 1), knn_kp, knn_kp16, knn_kp8, knn_no_pre32, knn_no_pre16, knn_no_pre8,
 *   knn_csr_pre32, knn_general
 *       query kernels; knn_kp8 > 0 also opts bf16 datasets into the int8 ranking tier
 *   graph_general (0 / 1)          kNN graph: every leaf on the tiled kernel (rpt_knn_graph_*)
 *   graph_refine_general (0 / 1)   kNN graph refinement: one point per workgroup for every k and
 *                                  reverse (rpt_knn_graph_refine_*)
 *   graph_delete_general (0 / 1)   rpt_graph_delete_*: one touched row per workgroup for every kg
 *   graph_csr_masked (0 / 1)       kNN graph on CSR rows under cosine / inner product: the
 *                                  presence-masked fold for every call, not only for data that stores
 *                                  an inf or NaN (rpt_knn_graph_csr_metric_*)
 *   graph_search_nofilter (0 / 1)  graph search: no visited filter, only the beam itself is checked
 *                                  before a distance is computed (rpt_graph_search_*)
 *   graph_search_csr_stream (0 / 1)  graph search on CSR rows: every query passes through LDS in
 *                                  pieces, none stays resident (rpt_graph_search_csr_*,
 *                                  rpt_graph_search_csr_metric_*)
 *   graph_prepare_csr_resident (0, n, -1)  graph preparation on CSR rows: a point's neighbours are
 *                                  staged in LDS when they hold at most this many entries together
 *                                  (0 = the built-in cap of 1536, n > 0 = min(n, 1536), -1 = no point
 *                                  is resident; rpt_graph_prepare_csr_*,
 *                                  rpt_graph_prepare_csr_metric_*)
 *   brute_csr_tile (0 auto, n)     brute force over CSR rows: queries per workgroup (1, 2, 4 or 8; other
 *                                  values round down; halved while the tile does not fit LDS; auto
 *                                  takes up to 4)
 *   knn_vote_lds (0, n)            rpt_knn_vote_*: ids one workgroup sorts in LDS (0 = 16 384, n > 0 =
 *                                  min(n, 16 384)); queries with more candidates sort in a global slab;
 *                                  the answer does not depend on it
 *   knn_vote_slice (0 auto, n)     rpt_knn_vote_*: at most n queries per vote-select slice (auto: by a
 *                                  fixed scratch budget); the answer does not depend on it
 *   knn_allow_group_budget (0 auto, n)  rpt_brute_knn_allow_group_*: at most n ids of group lists per pass
 *   knn_allow_slice (0 auto, n)    rpt_knn_allow_* / rpt_allow_candidates_host: at most n queries per
 *                                  compaction slice (auto: by the same fixed scratch budget); the answer
 *                                  does not depend on it
 *   comm_force_exchange           sharded kNN on a ONE-rank communicator still runs record ->
 *                                  ncclAllGather -> merge (set on the communicator's first ctx)
 *   comm_inject_failure            test hook: the device's shard reports a failure (see "Failures"
 *                                  under the multi-GPU entry points)
 *   debug_host, debug_stamps       stderr diagnostics
 * Unknown names: RPT_E_ARG. */
int32_t rpt_ctx_set_option(rpt_ctx* ctx, const char* name, int64_t value);
int32_t rpt_ctx_get_option(rpt_ctx* ctx, const char* name, int64_t* value);

/* ---- kernel timing (bench.py roofline): HIP events recorded on the ctx stream around every
 * launch of a kernel class while enabled.  which: 0 = projection batch kernels (one launch =
 * one pass over the whole point set for up to 96 hyperplanes), 1 = split work,
 * 2 = query plan (query projections + traversal), 3 = distance/top-k kernel, 4 = the wide
 * (> 32 hyperplanes per pass) MFMA projection launches alone (they are also part of class 0),
 * 5 = the candidate-list step: the vote-select kernel of rpt_knn_vote_* / rpt_vote_candidates_host and
 * the compaction and list kernels of rpt_knn_allow_* / rpt_brute_knn_allow_*, 6 = the link kernels of
 * rpt_graph_insert_* (one launch = the link of one chunk; its searches are class 3), 8 = the mark,
 * scan, copy and repair kernels of rpt_graph_delete_* (one launch = one call).  7 is not a class:
 * rpt_prof_get answers RPT_E_ARG for it.
 * rpt_prof_get synchronises the stream and returns the accumulated ms and launch count. */
int32_t rpt_prof_enable(rpt_ctx* ctx, int32_t on);
int32_t rpt_prof_reset(rpt_ctx* ctx);
int32_t rpt_prof_get(rpt_ctx* ctx, int32_t which, double* total_ms, int64_t* launches);

/* ---- datasets: Embed / DVector / SVector carriers (Internal.hs:56-59,92-93,122) ----
 * dense: row-major X[n][d] (`V.Vector (Embed DVector Double x)` packed once at the boundary).
 * csr:   SVector rows: rowptr[n+1] (int64), col[nnz] (int32, ascending per row, < d), val.
 * *_host variants copy to HBM; *_dev variants borrow device memory that must outlive the
 * handle.  Query batches use the same handle type.
 * Stream order of borrowed memory: the ctx stream is a non-blocking stream of its own, nothing
 * orders it against the stream that PRODUCED the borrowed arrays.  The producer must have
 * finished (synchronise its stream, or make it wait on an event of it via rpt_ctx_stream) before
 * the first rpt_* call that reads the memory; the same holds for output buffers of the *_dev
 * query entry points that another stream initialises.  (rptree_amd.Dataset.from_torch and
 * ShardedForest synchronise torch's current stream for exactly this reason.) */
int32_t rpt_dataset_dense_host(rpt_ctx* ctx, const void* X_host, int64_t n, int32_t d,
                               int32_t dtype, rpt_dataset** out);
int32_t rpt_dataset_dense_dev(rpt_ctx* ctx, const void* X_dev, int64_t n, int32_t d,
                              int32_t dtype, rpt_dataset** out);
int32_t rpt_dataset_csr_host(rpt_ctx* ctx, const int64_t* rowptr_host, const int32_t* col_host,
                             const void* val_host, int64_t n, int32_t d, int32_t dtype,
                             rpt_dataset** out);
/* borrow CSR arrays that already live in HBM (they must outlive the handle; NOT validated:
 * rowptr non-decreasing from 0 to nnz, every column index in [0, d), as the host variant checks) */
int32_t rpt_dataset_csr_dev(rpt_ctx* ctx, const int64_t* rowptr_dev, const int32_t* col_dev,
                            const void* val_dev, int64_t n, int32_t d, int32_t dtype, int64_t nnz,
                            rpt_dataset** out);
int32_t rpt_dataset_free(rpt_dataset* ds);
int32_t rpt_dataset_info(const rpt_dataset* ds, int64_t* n, int32_t* d, int32_t* dtype,
                         int32_t* is_csr, int64_t* nnz);

/* ---- topology: Internal.hs:289 (leaf test), :495,503 (cut at n div 2) ----
 * Enumerates the nodes in DFS (pre-)order.  Each record is 5 int64:
 * {level, heap, offset, size, is_leaf}.  Pass out=NULL to get the count only. */
int32_t rpt_topology(int64_t n, int32_t max_depth, int32_t min_leaf, int64_t* out,
                     int64_t cap_records, int64_t* n_records);

/* ---- projection batch: replaces the N `inner` calls of Internal.hs:504 ----
 * P[c][i] = R[c] `inner` x_i  for C hyperplanes R_host[C][d] (dense-ified SVectors; zeros are
 * skipped exactly like the sparse representation skips them).  Output in the compute type:
 * double for F64 data, float for F32/BF16 data.  P_host / P_dev is [C][n]. */
int32_t rpt_project_host(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t C,
                         int32_t mode, void* P_host);
int32_t rpt_project_dev(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t C,
                        int32_t mode, void* P_dev);

/* ---- forest build: replaces createMulti/create/insert/partitionAtMedian/sortByVG
 * (Internal.hs:217-297,486-512) under forestBatch / treeBatch (Batch.hs:29-63) ----
 * R_host[T][L][d]: the hyperplanes sampled by the HOST (Batch.hs:59-61), dense-ified.
 * L = maxDepth.  flags: RPT_PROJ_* mode. */
int32_t rpt_forest_build(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t T,
                         int32_t L, int32_t min_leaf, int32_t flags, rpt_forest** out);
int32_t rpt_forest_free(rpt_forest* f);
int32_t rpt_forest_info(const rpt_forest* f, int64_t* n, int32_t* d, int32_t* T, int32_t* L,
                        int32_t* min_leaf);
/* copy-out accessors so the host can rebuild ordinary `RPT` values (Internal.hs:139-149) */
int32_t rpt_forest_get_perm(rpt_forest* f, int32_t* perm_host /*[T][N]*/);
int32_t rpt_forest_get_nodes(rpt_forest* f, double* thr_host, double* mglo_host,
                             double* mghi_host /* each [T][2^L-1] */);
/* projections computed during the build, [T][L][N] in the compute type (parity tests) */
int32_t rpt_forest_get_proj(rpt_forest* f, void* proj_host);
/* ---- streaming build: `forest` / `tree` (Conduit.hs:58-121) = chunkedAccum (Conduit.hs:169-176)
 * folding insertMulti / insert (Internal.hs:245-297) over chunks of `chunk` points (the last one may
 * be shorter, C.chunksOf).  The reference's semantics, including its quirks: a chunk part that
 * reaches a Bin is split at ITS OWN median and the thresholds are averaged ((thr0 + thr) / 2,
 * Internal.hs:281), margins fold by (max, min) (:280, :86-87); an EMPTY part reaching a Bin replaces
 * the subtree by an empty Tip (:277) — the points stored below it are lost (rpt_forest_get_topology
 * reports how many).  With chunk >= n the result is the batch forest.  Dense rows only.
 * The shape of a streamed tree depends on (n, chunk, minLeaf, maxDepth): such a forest carries an
 * EXPLICIT topology — heap slots 0 .. 2^(maxDepth+1)-2, kind 0 absent / 1 Bin / 2 Tip, the points of
 * Tip h = perm[t][leaf_off[h] .. leaf_off[h] + leaf_len[h]) — the same for every tree.
 * rpt_forest_get_perm / _get_nodes return [T][n] ids (the first `held` of a row are valid) and
 * [T][slots] node arrays; rpt_candidates / rpt_knn_* work on the handle (general query path). */
int32_t rpt_forest_stream_build(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t T,
                                int32_t L, int32_t min_leaf, int64_t chunk, int32_t flags,
                                rpt_forest** out);
/* any output pointer may be NULL; kind / leaf_off / leaf_len hold *slots entries */
int32_t rpt_forest_get_topology(rpt_forest* f, int64_t* slots, int8_t* kind_host,
                                int64_t* leaf_off_host, int64_t* leaf_len_host, int64_t* held,
                                int64_t* dropped);
/* import a forest built elsewhere (e.g. deserialiseRPForest, Internal.hs:191-196) */
int32_t rpt_forest_import(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t T,
                          int32_t L, int32_t min_leaf, const int32_t* perm_host,
                          const double* thr_host, const double* mglo_host,
                          const double* mghi_host, rpt_forest** out);
/* projection mode the forest's thresholds were computed with; queries project in the same mode,
 * with a kernel chosen by the batch's shape and the context's options at the time of the call (so a
 * stored row sent back as a query gets the build's key bit for bit in RPT_PROJ_EXACT, and a key
 * within twice the mode's tolerance of it otherwise: e.g. RPT_PROJ_MFMA on CSR rows builds on the
 * dense-ified bf16 path from 65 536 rows on, while a small query batch stays on the segmented
 * kernel; proj_bf16_terms, proj_bf16_f32 and proj_csr_nodense are not stored in the forest).  A forest imported with rpt_forest_import starts as RPT_PROJ_AUTO: restore the
 * builder's mode with rpt_forest_set_mode (the flat on-disk format stores it). */
int32_t rpt_forest_get_mode(const rpt_forest* f, int32_t* mode);
int32_t rpt_forest_set_mode(rpt_forest* f, int32_t mode);
/* statistics of the batch build.  tie_nodes: nodes (of at least two points, over all trees) whose
 * cut falls on a tie, p'[nh - 1] == p'[nh]; every such node counts once, whichever kernels split it */
int32_t rpt_forest_stats(rpt_forest* f, int64_t* tie_nodes, int64_t* big_mid_nodes);

/* ---- split of one level on caller-supplied projections: partitionAtMedian
 * (Internal.hs:486-505) for every node of a segment list, for integer parity on IDENTICAL
 * projection inputs.  key_host[n]: projections indexed by point id.  seg_off/seg_len[S]:
 * disjoint segments of perm_io_host[n] (ids).  On return every segment is stably sorted by
 * key (ties: previous position), thr_mg_host[S][3] = {thr, mglo, mghi}. */
int32_t rpt_split_segments(rpt_ctx* ctx, const double* key_host, int64_t n,
                           int32_t* perm_io_host, const int64_t* seg_off_host,
                           const int64_t* seg_len_host, int32_t S, double* thr_mg_host);

/* ---- queries ----
 * candidates (RPTree.hs:289-314): for every (query, tree) the leaf buckets reached, in
 * left-to-right order.  Output is CSR-like: off_host[nq*T + 1] (int64) into ids_host.
 * Two-call protocol: ids_host = NULL -> only *total is written. */
int32_t rpt_candidates(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* queries,
                       int64_t* off_host, int32_t* ids_host, int64_t cap, int64_t* total);

/* knnH (RPTree.hs:199-217 over candidatesH :318-342) with distf = metricL2: per query the
 * buckets of the leaves with the smallest margin priority, taken while the running count stays
 * <= k (always at least one), the bucket taken last FIRST, every point with its distance — as in
 * the reference the result is neither sorted by distance nor cut to k.  Equal priorities keep
 * (tree, DFS) order (the reference's order among ties depends on its heap's shape).
 * Output is CSR-like: off_host[nq + 1] into ids_host / dist_host.  Two-call protocol:
 * ids_host = NULL -> only off_host and *total are written. */
int32_t rpt_knnh_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                      const rpt_dataset* queries, int32_t k, int64_t* off_host, int32_t* ids_host,
                      double* dist_host, int64_t cap, int64_t* total);

/* Dense f64 data: the distances returned are metricDDL2's left fold of (u - v)^2 (Internal.hs:
 * 403-406) with every square correctly rounded, and the results are selected and ordered on those
 * values, on every query path: the answer is the k best of ALL candidates by (fold distance, NaN
 * last, candidate position) under the duplicate rule, ids and distance bits.
 * How: candidates are RANKED on a lane-parallel sum of the same squares (the same value to a few
 * ulp).  The entries of the best k + 8 DIFFERENT ids by that value (copies of one id, the same point
 * found by several trees, do not count against the 8; at most as many entries as the kernel's list
 * holds), or the kept entries of a prefilter tier, are evaluated again as the fold and the k best of
 * those are written.  Then the cut is certified per query: both sums add the same d non-negative
 * products, so they differ by less than (d + 4) 2^-53 relative, and when the k-th fold distance is
 * strictly below the lane-parallel value of the last kept entry less that bound, no candidate left
 * out can belong to the answer.  A query that is not certified (more different rows tie at the
 * cut than were kept, +inf or NaN at the cut) is answered again by an exact kernel that ranks every
 * candidate on the fold itself, one thread per row, with no margin; so is a query whose prefilter
 * cut could not be certified.  rpt_knn_last_uncertified counts both; the context option
 * knn_l2_exact sends every query to the exact kernel.  rpt_brute_knn_*, the truth of
 * rpt_recall_hits_host included, follow the same rule.  RPT_KNN_VOTE alone keeps the uncertified
 * margin of 8 (the exact kernel does not vote).
 * `(** 2)` is libm's pow in a GHC build: where pow(t, 2) is correctly rounded these are its bits;
 * glibc >= 2.28 returns a neighbouring double for about 9 arguments in 10 000, which moves the last
 * bit of about one distance in a thousand (tests/test_oracle_kat.py measures it on the test box).
 * RPT_KNN_DEDUP_DISTANCE collapses entries whose FOLD distances are equal (knnPQ's nub on the values
 * returned): k entries when the candidates hold k different values, strictly ascending. */
/* knn (RPTree.hs:168-176) with distf = metricL2 (Internal.hs:318, metricDDL2 :403-406 /
 * true Euclidean distance for CSR data, evaluated as |q|^2 + sum over the row's nonzeros of
 * ((x_j - q_j)^2 - q_j^2): absolute error about 1e-8 |q|): per query the k best (distance, id), stable in
 * candidate order (tree ascending, then leaf order).  ids/dist are [nq][k]; count[nq] is the
 * number of valid entries (< k when fewer candidates).  Unused slots: id -1, dist +inf. */
/* Memory note: the first rpt_knn_* call with duplicates kept (flags 0) and k <= 42 on a dense
 * f64 dataset builds an int8 copy of it on the device (+12.5 % of the dataset's size, freed with the
 * dataset; one scale for the whole dataset, rows of a multiple of 16 elements).  Only when that copy
 * cannot rank the call (other row lengths, k >= 40 on small tree shards, no memory, or a forest that
 * has dropped the tier) an f32 copy (+50 %) and an IEEE-half copy (+25 %, elements within the half
 * range) are built as well; f32 datasets likewise get the int8 copy first, the half copy when
 * needed: candidates are ranked on the int8 copy (k + max(48, k) kept; the ranking
 * value is an exact integer, the cut is certified through the triangle inequality with the
 * quantisation errors of the query and of the worst row), the half copy (k + max(8, k/2) kept) or
 * the f32 copy (k + max(6, k/2) kept), exact f64 distances are computed for the kept ones, and a
 * per-query error bound certifies the cut (a query that fails it is tried once more with three
 * times the kept entries, then takes the all-f64 path).
 * Results are identical either way.  A dataset borrowed with rpt_dataset_dense_dev must not be
 * modified while the library holds it.
 * Dense f32 / bf16 rows under L2: the elements are widened to f32 exactly and every difference,
 * square and sum is rounded to f32 (no FMA); the answer is the k best of ALL candidates by (that f32
 * squared distance, candidate position) under the duplicate rule, and the distance returned is
 * sqrt((double)it).  Every returned distance lies within (d + 2) 2^-24 relative, plus sqrt(d) 4e-23
 * for products in the f32 subnormal range, of the true Euclidean distance of the widened rows (the
 * bound the ranking tiers' certificates on f32 data rely on), and the answer is the definition's bit
 * for bit wherever f32 arithmetic is exact.  A row is summed in one fixed order on every query path,
 * rpt_brute_knn_* and the truth of rpt_recall_hits_host included, so neither the bits nor the order
 * of near-tied candidates depend on the path.  tests/test_gpu_knn_f32_l2.py holds every path to both
 * statements against an f64 reference (tests/knn_f32_ref.py), every query. */
int32_t rpt_knn_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                     const rpt_dataset* queries, int32_t k, int32_t flags, int32_t* ids_host,
                     double* dist_host, int32_t* count_host);
int32_t rpt_knn_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                    const rpt_dataset* queries, int32_t k, int32_t flags, int32_t* ids_dev,
                    double* dist_dev, int32_t* count_dev);
/* statistics of the last rpt_knn_* call: total candidates visited (sum over queries) */
int32_t rpt_knn_last_candidates(rpt_ctx* ctx, int64_t* total);
/* ... and how many of its queries were answered again exactly because their cut could not be
 * certified: on dense f64 rows under L2 the queries of a prefilter tier (equal distances at its
 * cut) and of the all-f64 kernels (different rows that tie at the cut) that the exact kernel answered
 * (every query with the option knn_l2_exact); on f32 / CSR rows the prefilter's, answered by the
 * all-exact kernel.  After an RPT_KNN_METRIC_COSINE / _INNER call: the queries the metric's exact
 * kernel answered (all of them with the option knn_metric_exact).  This may read the count from
 * the device, so it waits for the call's kernels to finish */
int32_t rpt_knn_last_uncertified(rpt_ctx* ctx, int64_t* total);
/* ... and how many took the in-kernel second attempt (a cut the first, narrower selection could not
 * certify, retried with three times the kept entries by the same workgroup).  Telemetry: a forest whose
 * batches retry often starts its later batches wider. */
int32_t rpt_knn_last_retries(rpt_ctx* ctx, int64_t* total);
/* ... and the shadow its candidates were ranked on: 0 = none (all-f64 distances), 1 = the f32 copy
 * of the dataset, 2 = its IEEE-half copy (round 3: a quarter of the f64 bytes; keeps k + max(8, k / 2)
 * entries for the exact pass, same certificate with the half rounding in the error bound), 3 = its
 * int8 copy (an eighth of the f64 bytes).  A forest on which more than a quarter of a batch cannot
 * be certified drops one tier for its later batches (int8 -> half -> f32 -> none). */
int32_t rpt_knn_last_tier(rpt_ctx* ctx, int32_t* tier);
/* diagnostics of the last rpt_forest_build on this context: split nodes of 1025 .. 8192 points that
 * the packed-code kernel handed back to the general kernels (heavy ties: more than 1024 points of a
 * node share the 16-bit code of its median; the result does not depend on it), and how many of those
 * because a code histogram contradicted the node sizes (a defect if ever non-zero; tested to be 0) */
int32_t rpt_build_last_handed_back(rpt_ctx* ctx, int64_t* nodes, int64_t* inconsistent);

/* ---- kNN graph of the indexed points: knn (RPTree.hs:174-176) with EVERY STORED POINT as the
 * query, distf = metricL2 (metricDDL2, Internal.hs:403-406), built leaf by leaf ----
 * `f` is a batch forest (built or imported) over the dense data set `data`, rows 0 .. n-1.  For a
 * point i:
 *   mates(i)   the ids j != i that share a leaf with i in at least one tree.  A point is never its
 *              own neighbour; a different id holding an equal row is an ordinary neighbour at
 *              distance 0.
 *   dist(i, j) sqrt(((0 + (x_i0 - x_j0)^2) + (x_i1 - x_j1)^2) + ...) in double: metricDDL2's left
 *              fold, every difference, square and sum rounded on its own, no FMA; f32 and bf16
 *              elements are widened exactly first.  The values are doubles and bit-exact against
 *              this definition for all three dtypes (as the cosine / inner-product metrics are, and
 *              unlike rpt_knn_*, whose L2 on f32 / bf16 rows is f32 arithmetic within a stated
 *              bound of the true distance, see rpt_knn_host).  The fold is
 *              symmetric bit for bit, dist(i, j) == dist(j, i): a pair is evaluated once.
 *   answer     the first k of mates(i) ordered by (distance, id); NaN ranks behind every number,
 *              NaNs among themselves by id.  count[i] = min(k, |mates(i)|); unused slots hold
 *              id -1 and distance +inf.
 * The forest decides only the membership of mates(i): the margin rule of `candidates`
 * (RPTree.hs:289-314), which sends a query near a cut into both children, plays no part.  The
 * graph is therefore NOT defined as the de-duplicated self-query rpt_knn_*; the two differ on the
 * few points that rule sends both ways (3 of 3 000 entries in a trial of 6 000 points).
 * No ranking shadow, certificate or fallback: every distance is the fold itself, so ties of any
 * width and duplicate rows are ranked exactly, and rpt_knn_last_tier and the forest's ranking
 * tiers are untouched.
 * RPT_GRAPH_ACCUMULATE: the output arrays are also an input.  The valid entries already there
 * (count[i] of them per row, sorted by (distance, id), free of i) join mates(i) with their stored
 * distances; duplicate ids collapse to one entry.  The order is total and the union is a set, so
 * folding forests over one data set (tree shards, several forests) in any order gives the same
 * arrays.  Without the flag the arrays are output only.
 * One launch per tree in stream order; within a tree one workgroup owns a point's list: no atomics,
 * a deterministic result.  Leaves of up to 128 points take a one-workgroup kernel that evaluates
 * every pair once; larger leaves (a depth cap, maxDepth 0 = all pairs) take a tiled kernel that
 * evaluates every ordered pair; the context option graph_general sends every leaf there; the
 * answer does not depend on it.  rpt_knn_graph_last_pairs: distances the last call evaluated,
 * T * sum over leaves of s (s - 1) / 2 (one-workgroup kernel) or s (s - 1) (tiled kernel), s the
 * leaf size (the padding lanes of a tile are not counted).
 * Errors: k outside [1, RPT_GRAPH_MAX_K], data that is not the forest's data set shape (n, d,
 * dtype), other flag bits: RPT_E_ARG.  CSR data, a streamed forest (explicit topology), the
 * RPT_KNN_METRIC_* flags: RPT_E_UNSUPPORTED.  n = 0 and forests of depth 0 are valid.  An imported
 * forest's perm rows must be permutations of 0 .. n-1 (rpt_forest_import checks the range only).
 * _dev enqueues on the ctx stream and does not synchronise (rpt_ctx_sync before reading); _host
 * synchronises.  ids / dist are [n][k], count is [n].  Timed under rpt_prof_* class 3. */
#define RPT_GRAPH_ACCUMULATE 1
#define RPT_GRAPH_MAX_K 64
int32_t rpt_knn_graph_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                          int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev);
int32_t rpt_knn_graph_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                           int32_t flags, int32_t* ids_host, double* dist_host,
                           int32_t* count_host);
int32_t rpt_knn_graph_last_pairs(rpt_ctx* ctx, int64_t* pairs);

/* ---- NN-descent rounds over a kNN graph: "a neighbour of my neighbour is probably my neighbour" ----
 * Input: the dense data set `data` (f64, f32 or bf16 rows; rows 0 .. n-1) and a graph in
 * rpt_knn_graph_*'s layout: ids[n][k], dist[n][k], count[n], row i holding count[i] valid entries
 * sorted by (distance, id), free of i, ids in [0, n), no id twice.  The arrays are input AND
 * output.  No forest takes part: any graph over the data set will do (rpt_knn_graph_*'s, a
 * brute-force one, one from elsewhere whose distances are the fold below).
 * One round maps a graph G to R(G).  For a point i, every set taken from G (never from rows the
 * round has already rewritten: a round reads the old graph and writes a new one):
 *   F(i)      the valid ids of row i
 *   Rev_r(i)  the first r, ordered by (the distance stored with i in row j, j), of {j : i in F(j)};
 *             r = `reverse`, 0 = none
 *   B(i)      F(i) u Rev_r(i)
 *   C(i)      (B(i) u U{F(v) : v in B(i)}) \ {i}, a SET: every id once
 *   dist      c in F(i): the distance stored in row i.  Any other c: metricDDL2's left fold in
 *             double exactly as rpt_knn_graph_* defines it (elements widened exactly, every
 *             difference, square and sum rounded on its own, no FMA, one sqrt), bit-exact for all
 *             three dtypes
 *   row i of R(G)   the first k of C(i) by (distance, id), NaN behind every number, NaNs among
 *             themselves by id; count = min(k, |C(i)|); unused slots hold id -1 and distance +inf
 * `iters` rounds are applied; a round that changes no row ends the sequence (R is deterministic,
 * later rounds would be the identity).  F(i) is a subset of C(i), so every slot of a row only ever
 * moves forward in the (distance, id) order.  The result is a pure function of (data, G, k,
 * reverse, iters): no sampling, no atomics on the lists, no dependence on the launch shape; two
 * calls give the same bits.  NN-descent's new / old flags and rho-sampling are deliberately left
 * out (they trade this determinism for fewer evaluations).
 * rpt_knn_graph_refine_last (synchronises the stream), statistics of the last call on ctx:
 *   rounds      rounds applied, up to and including the first one that changed nothing (or iters)
 *   updates     sum over the applied rounds and i of |F_new(i) \ F_old(i)|
 *   candidates  sum over the applied rounds and i of |C(i) \ F(i)|: the distances evaluated
 * A point is owned by one wave (four points per workgroup) while (k + reverse)(k + 1) ids fit its
 * share of LDS, by a workgroup of its own beyond; the context option graph_refine_general sends
 * every point there; the answer does not depend on it.
 * Errors: k outside [1, RPT_GRAPH_MAX_K], reverse outside [0, RPT_GRAPH_MAX_K], iters < 1, flags
 * other than 0: RPT_E_ARG.  CSR data, any RPT_KNN_METRIC_* bit: RPT_E_UNSUPPORTED.  Scratch (a
 * second graph, the reverse lists: about 24 k + 20 bytes per point) comes from the context's
 * pool: RPT_E_NOMEM.  n = 0 and n = 1 are valid.
 * _host checks the graph BEFORE anything is uploaded (count in [0, k], ids in [0, n), id != i, no
 * id twice in a row) and returns RPT_E_ARG naming the row; it synchronises.  _dev borrows device
 * arrays and, like rpt_dataset_csr_dev, does NOT validate them: a count or an id out of range is
 * skipped, but the result is then unspecified.  _dev enqueues ALL `iters` rounds on the ctx
 * stream and does not synchronise (rpt_ctx_sync before reading); the kernels of the rounds behind
 * the first one that changed nothing return at once on a device-side flag.  The caller's arrays
 * hold the answer for every number of applied rounds.  Timed under rpt_prof_* class 3. */
int32_t rpt_knn_graph_refine_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse,
                                 int32_t iters, int32_t flags, int32_t* ids_dev, double* dist_dev,
                                 int32_t* count_dev);
int32_t rpt_knn_graph_refine_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse,
                                  int32_t iters, int32_t flags, int32_t* ids_host, double* dist_host,
                                  int32_t* count_host);
int32_t rpt_knn_graph_refine_last(rpt_ctx* ctx, int64_t* rounds, int64_t* updates,
                                  int64_t* candidates);

/* ---- the kNN graph and its refinement under the cosine and inner-product distances ----
 * rpt_knn_graph_metric_* and rpt_knn_graph_refine_metric_* are rpt_knn_graph_* and
 * rpt_knn_graph_refine_* with one more argument, `metric`: 0, RPT_KNN_METRIC_COSINE or
 * RPT_KNN_METRIC_INNER.  `flags` keeps its meaning (RPT_GRAPH_ACCUMULATE or 0 for the graph, 0 for
 * the refinement).  Everything stated above carries over word for word: mates(i), the sets F /
 * Rev_r / B / C, the order (distance, id) with NaN behind every number and NaNs among themselves by
 * id, counts, unused slots (id -1, distance +inf), one owner per list, no atomics on the lists, a
 * deterministic result, _dev enqueues and does not synchronise / _host synchronises, the context
 * options graph_general and graph_refine_general, rpt_prof_* class 3, rpt_knn_graph_last_pairs,
 * rpt_knn_graph_refine_last, and the validation of the graph by the _host refinement.  The one
 * thing that changes is dist(i, j).  With dot(a, b) the left fold ((0 + a0 b0) + a1 b1) + ... in
 * double from +0.0, f32 / bf16 elements widened exactly, every product and sum rounded on its own,
 * no FMA (the dot of the RPT_KNN_METRIC_* definition above, with q = x_i):
 *   metric == 0            sqrt of the fold of squared differences, as rpt_knn_graph_* defines it;
 *                          the same bits as the entry points without `metric`
 *   RPT_KNN_METRIC_INNER   dist(i, j) = -dot(x_i, x_j)
 *   RPT_KNN_METRIC_COSINE  dist(i, j) = 1 - dot(x_i, x_j) / (sqrt(dot(x_i, x_i)) * sqrt(dot(x_j, x_j)))
 *                          with correctly rounded sqrt, product and division; a zero row gives NaN
 *                          against everything (and so ranks last, by id, in every list)
 * No ranking shadow, certificate or fallback here either: every distance is that fold.
 *   Symmetry     both distances are symmetric bit for bit, dist(i, j) == dist(j, i): IEEE
 *                multiplication commutes and the fold visits the same products in the same order,
 *                so a pair is still evaluated once.
 *   Signed zero  -dot can be -0.0.  The order compares numbers, so -0.0 ties with +0.0 and the id
 *                decides; the stored bits are the computed ones.
 *   Inner product  it is not a metric and a point may be "nearer" to others than to itself.
 *                Nothing in the definition cares: i is excluded by id, as above.
 *   Mixing metrics  accumulating into, or refining, arrays that were built under another metric is
 *                the caller's error and is NOT detected: stored distances are taken as stored.
 * Errors: any other `metric` value, both metric bits together, RPT_KNN_METRIC_REFERENCE: RPT_E_ARG
 * (a metric bit in `flags` too: flags must be 0 / RPT_GRAPH_ACCUMULATE).  CSR data and streamed
 * forests: RPT_E_UNSUPPORTED.  Everything else as the entry points without `metric`.
 * Memory note: the cosine distance reads the rows' dot(x, x) cached on the dataset by the first
 * cosine or inner-product call of any kind, 8 bytes per row, freed with the dataset (a dataset
 * borrowed with rpt_dataset_dense_dev must not change while the library holds it). */
int32_t rpt_knn_graph_metric_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                 int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                                 int32_t* count_dev);
int32_t rpt_knn_graph_metric_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                  int32_t metric, int32_t flags, int32_t* ids_host,
                                  double* dist_host, int32_t* count_host);
int32_t rpt_knn_graph_refine_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                        int32_t reverse, int32_t iters, int32_t metric, int32_t flags,
                                        int32_t* ids_dev, double* dist_dev, int32_t* count_dev);
int32_t rpt_knn_graph_refine_metric_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                         int32_t reverse, int32_t iters, int32_t metric, int32_t flags,
                                         int32_t* ids_host, double* dist_host, int32_t* count_host);

/* ---- the kNN graph and its NN-descent rounds on SVector (CSR) rows, under L2 ----
 * rpt_knn_graph_csr_* and rpt_knn_graph_refine_csr_* are rpt_knn_graph_* and rpt_knn_graph_refine_*
 * for a CSR data set (rpt_dataset_csr_*, f64 or f32 values); `f` is a batch forest over it.  Let
 * dense(x) be the row of d doubles that a CSR row stands for: absent columns are +0.0, f32 values
 * are widened exactly, and a stored zero is a zero.  Everything stated for the dense entry points
 * carries over word for word with dist(i, j) = metricDDL2's left fold over dense(x_i), dense(x_j):
 * mates(i), the sets F / Rev_r / B / C, the order (distance, id) with NaN behind every number and
 * NaNs among themselves by id, counts and unused slots (id -1, distance +inf),
 * RPT_GRAPH_ACCUMULATE, one owner per list and no atomics on a list, a round that changes nothing
 * ends the sequence, _dev enqueues and does not synchronise / _host validates the graph (the
 * refinement) and synchronises, the context options graph_general and graph_refine_general,
 * rpt_knn_graph_last_pairs, rpt_knn_graph_refine_last, rpt_prof_* class 3.
 *   Bit-equal to the dense entry points  The kernels do not visit all d columns and need not.  A
 *                column where both rows hold +0.0 contributes acc + (+0.0), which is acc for every
 *                acc the fold can hold: it starts at +0.0 and, a sum of squares, never becomes
 *                -0.0.  A pair's fold over any ascending superset of the union of the two supports
 *                therefore gives the same bits, and the answer is bit-equal to what
 *                rpt_knn_graph_* / rpt_knn_graph_refine_* give on the dense-ified rows with the same
 *                perm.  The fold stays symmetric bit for bit: a pair of a leaf is still evaluated
 *                once.  Two rows without nonzeros are at distance 0.
 *   Ascending columns  A row's columns must ascend strictly (the SVector invariant;
 *                rpt_dataset_csr_host checks only col < d).  For rows that break the invariant the
 *                answer is unspecified, but the kernels stay in bounds and terminate.
 * There is no limit on a row's length or on d: the leaf kernels stage windows of 32 columns (only
 * the windows in which the leaf holds a nonzero), the refinement merges a candidate's row against
 * x_i's, which passes through LDS in pieces of bounded size.
 * Errors: a dense data set: RPT_E_ARG (the message names rpt_knn_graph_* / rpt_knn_graph_refine_*);
 * a data set of another shape than the forest's (n, d, dtype), k outside [1, RPT_GRAPH_MAX_K],
 * reverse outside [0, RPT_GRAPH_MAX_K], iters < 1, other flag bits: RPT_E_ARG.  A streamed forest,
 * any RPT_KNN_METRIC_* bit: RPT_E_UNSUPPORTED.  n = 0, n = 1, depth 0 and rows with no nonzeros are
 * valid. */
int32_t rpt_knn_graph_csr_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                              int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev);
int32_t rpt_knn_graph_csr_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                               int32_t flags, int32_t* ids_host, double* dist_host,
                               int32_t* count_host);
int32_t rpt_knn_graph_refine_csr_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                     int32_t reverse, int32_t iters, int32_t flags, int32_t* ids_dev,
                                     double* dist_dev, int32_t* count_dev);
int32_t rpt_knn_graph_refine_csr_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                      int32_t reverse, int32_t iters, int32_t flags,
                                      int32_t* ids_host, double* dist_host, int32_t* count_host);

/* ---- the kNN graph and its NN-descent rounds on SVector (CSR) rows, under cosine / inner product ----
 * rpt_knn_graph_csr_metric_* and rpt_knn_graph_refine_csr_metric_* are rpt_knn_graph_csr_* and
 * rpt_knn_graph_refine_csr_* with one more argument, `metric` (before `flags`): 0,
 * RPT_KNN_METRIC_COSINE or RPT_KNN_METRIC_INNER.  Everything stated for those entry points carries
 * over word for word (mates, the order (distance, id), the layout, unused slots, k <= 64,
 * RPT_GRAPH_ACCUMULATE, batch forests only, the refinement round and rpt_knn_graph_refine_last,
 * rpt_knn_graph_last_pairs, the options graph_general / graph_refine_general); the one thing that
 * changes is dist(i, j), and it is the definition rpt_knn_csr_metric_* uses, word for word:
 * dotS(x, y) starts at +0.0, takes the columns stored in BOTH rows in ascending column order and
 * folds acc = acc + x_c * y_c, every product and sum rounded on its own, f32 values widened
 * exactly, no FMA.
 *   metric == 0            the bits of rpt_knn_graph_csr_* / rpt_knn_graph_refine_csr_*
 *   RPT_KNN_METRIC_INNER   dist(i, j) = -dotS(x_i, x_j)
 *   RPT_KNN_METRIC_COSINE  dist(i, j) = 1 - dotS(x_i, x_j) / (sqrt(dotS(x_i, x_i)) * sqrt(dotS(x_j, x_j)))
 *                          with the norms cached on the data set; an empty or all-zero row is at NaN
 *                          from everything and ranks last, by id
 * NaN ranks behind every number, NaNs among themselves by id; -0.0 (the inner distance of two rows
 * that share no column) ties with +0.0, the id decides and the stored bits are the computed ones.
 * Both distances are symmetric bit for bit, so a pair of a leaf is still evaluated once.
 *   Stored inf and NaN  While every stored value is finite, this is the dense definition
 *                (rpt_knn_graph_metric_* on the dense-ified rows with the same perm) bit for bit: a
 *                column only one row stores would add x * (+0.0) = +-0.0 to an accumulator that is
 *                never -0.0.  With a stored inf or NaN it is not: the dense fold meets inf * 0 = NaN
 *                where dotS takes no product (dotS of {0: inf} and {1: 1.0} is +0.0).  The answer
 *                is dotS in both cases.  The leaf kernels stage zero-filled windows; they read the
 *                data set's cached statistic (the largest dotS(x, x)) on the device, and when it is
 *                not finite they keep a presence word per staged row and fold a product only where
 *                both rows store the column.  The context option graph_csr_masked = 1 sends every
 *                call down that path; the answer does not depend on it.
 *   Ascending columns  as above: unspecified answer, in bounds, terminates.
 * Errors: any other `metric` value, both metric bits together, RPT_KNN_METRIC_REFERENCE: RPT_E_ARG
 * (a metric bit in `flags` too).  Dense data: RPT_E_ARG.  A streamed forest: RPT_E_UNSUPPORTED.
 * Everything else as rpt_knn_graph_csr_* / rpt_knn_graph_refine_csr_*; an error leaves the context
 * usable.  The graph under either metric (the inner product for the statistic alone) and the
 * refinement under cosine cache the rows' dotS(x, x) and their statistics on the data set, 8 bytes
 * per row, on their first call.  Such a graph is prepared and searched by
 * rpt_graph_prepare_csr_metric_* and rpt_graph_search_csr_metric_* (below); rpt_graph_search_csr_* and
 * rpt_graph_prepare_csr_* themselves keep refusing a metric (RPT_E_UNSUPPORTED).  Not built:
 * streamed forests, the reference's right-fold innerSS order. */
int32_t rpt_knn_graph_csr_metric_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                     int32_t metric, int32_t flags, int32_t* ids_dev,
                                     double* dist_dev, int32_t* count_dev);
int32_t rpt_knn_graph_csr_metric_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                      int32_t metric, int32_t flags, int32_t* ids_host,
                                      double* dist_host, int32_t* count_host);
int32_t rpt_knn_graph_refine_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                            int32_t reverse, int32_t iters, int32_t metric,
                                            int32_t flags, int32_t* ids_dev, double* dist_dev,
                                            int32_t* count_dev);
int32_t rpt_knn_graph_refine_csr_metric_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                             int32_t reverse, int32_t iters, int32_t metric,
                                             int32_t flags, int32_t* ids_host, double* dist_host,
                                             int32_t* count_host);

/* ---- query the kNN graph: best-first beam search from given seeds ----
 * Input: the dense data set `data` (n rows of f64, f32 or bf16), the dense `queries` (the same d and
 * element type, as rpt_knn_* requires), a graph over the data set in rpt_knn_graph_*'s layout of
 * which ONLY gids[n][kg] and gcount[n] are read (the stored distances play no part; kg in
 * [1, RPT_GRAPH_MAX_K]), seeds[nq][s] (s in [1, 64]; -1 marks an unused slot, the same id twice
 * counts once), k in [1, 64], ef in [k, RPT_GRAPH_SEARCH_MAX_EF] and `metric`: 0 (L2),
 * RPT_KNN_METRIC_COSINE or RPT_KNN_METRIC_INNER.  The result is a pure function of these.
 *   dist(q, v)  exactly the distance of rpt_knn_graph_metric_* with q in the place of x_i: a left
 *               fold in double, columns ascending, elements widened exactly, every operation
 *               rounded on its own, no FMA; L2 takes one sqrt; cosine uses the cached dot(x, x) of
 *               the row and the same fold for dot(q, q).  So it is bit-equal to
 *               rpt_brute_knn_metric_host for cosine and inner product on all three dtypes, and to
 *               rpt_brute_knn_host (L2) on f64 rows.
 *   Order       entries are ordered by (distance, id), NaN behind every number, NaNs among
 *               themselves by id.
 *   Beam        B holds at most ef entries, sorted, each flagged expanded or not.  Offering a set S
 *               to B means B <- the first ef of B u {(dist(q, v), v) : v in S}, every id once; new
 *               entries start unexpanded.
 *   Search      1. offer the valid seeds (ids in [0, n)).  2. repeat: let u be the first unexpanded
 *               entry of B in the order; if there is none, stop; otherwise mark u expanded and
 *               offer the valid ids of graph row u (slots < gcount[u], ids in [0, n); a row whose
 *               gcount lies outside [0, kg] offers nothing).
 *   Answer      the first k of B, count = min(k, |B|); unused slots hold id -1 and distance +inf.  A
 *               query whose seeds are all -1 has count 0.
 * Termination: an entry that is evicted, or an id that is rejected against a full beam, can never
 * enter later, because the beam's last entry only moves forward.  So a point is expanded at most
 * once and the loop ends after at most n expansions (the kernel's loop has exactly that bound).
 * Visited set: for the same reason, remembering which ids were already evaluated only saves work:
 * the answer is the same with an exact visited set, a lossy one, or none.  The kernel keeps a
 * small lossy hash of evaluated ids per query and checks the beam itself exactly; the context
 * option graph_search_nofilter switches the hash off; the answer and `expansions` do not depend
 * on it, only `evaluated` does.  One wave answers a query; nothing is shared between queries and
 * no atomics touch a beam, so the same input gives the same bits whatever the launch shape.
 * rpt_graph_search_last (synchronises the stream), sums over the last call's queries:
 *   expansions  entries marked expanded (defined by the text above)
 *   evaluated   distances the kernel really computed: at least the number of distinct ids offered,
 *               at most the valid seed slots plus gcount[u] over the expanded u
 * Errors: k, ef, s or kg out of range, ef < k, flags other than 0, queries whose d or dtype differ
 * from the data's, a dense / CSR pair, any other `metric` value, both metric bits together,
 * RPT_KNN_METRIC_REFERENCE: RPT_E_ARG.  CSR data: RPT_E_UNSUPPORTED.  nq = 0 and n = 0 are valid;
 * with n = 0 every count is 0.  Scratch comes from the context's pool: RPT_E_NOMEM.  Timed under
 * rpt_prof_* class 3.  A call leaves rpt_knn_last_* and the forests' ranking tiers untouched.
 * _dev borrows device arrays, enqueues on the ctx stream, does not synchronise and does NOT validate
 * the arrays: a graph id or seed outside [0, n) and a gcount outside [0, kg] are skipped, never
 * followed.  _host checks BEFORE anything is uploaded that every gcount is in [0, kg], every valid
 * graph id in [0, n) and every seed -1 or in [0, n), and returns RPT_E_ARG naming the row; it
 * synchronises. */
#define RPT_GRAPH_SEARCH_MAX_EF 256
int32_t rpt_graph_search_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                             int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                             const int32_t* seeds_dev, int32_t k, int32_t ef, int32_t metric,
                             int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev);
int32_t rpt_graph_search_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                              int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                              int32_t s, const int32_t* seeds_host, int32_t k, int32_t ef,
                              int32_t metric, int32_t flags, int32_t* ids_host, double* dist_host,
                              int32_t* count_host);
int32_t rpt_graph_search_last(rpt_ctx* ctx, int64_t* expansions, int64_t* evaluated);

/* ---- query the kNN graph over an allow-list of ids ----
 * rpt_graph_search_allow_* is the beam search of rpt_graph_search_* among SOME of the points: a
 * tombstone bitmap after deletions, the rows of one tenant.  The parameter list is
 * rpt_graph_search_*'s with `allow` behind the seeds and `width` behind ef.  One pair of entry
 * points serves dense data (f64, f32, bf16; dist as rpt_graph_search_*) and CSR data (f64, f32; dist
 * as rpt_graph_search_csr_metric_*, whose metric 0 is rpt_graph_search_csr_*) under `metric` 0,
 * RPT_KNN_METRIC_COSINE and RPT_KNN_METRIC_INNER; data and queries are both dense or both CSR.
 *   allow       a bitmap of n bits in ceil(n / 32) 32-bit words: id i is allowed when bit i & 31 of
 *               word i >> 5 is set.  Bits at positions >= n are ignored.  A null pointer means every
 *               id is allowed.  One bitmap serves the whole batch.
 *   width       in [ef, RPT_GRAPH_SEARCH_MAX_WIDTH]: the most entries the beam may hold, allowed or
 *               not.
 *   ef          in [k, RPT_GRAPH_SEARCH_MAX_EF], as before; it now counts ALLOWED entries only.
 * The distance, the total order ((distance, id), NaN behind every number, NaNs among themselves by
 * id), the seeds, the offers and "the first unexpanded entry" are word for word those of
 * rpt_graph_search_*.  Three things change.
 *   Cut         For a set U of (distance, id) entries sorted in the order, t_a is the ef-th allowed
 *               entry of U, if it has one, and t_w the width-th entry of U, if it has one.  cut(U)
 *               is every entry of U that is not after min(t_a, t_w); with neither, cut(U) = U.  So
 *               a beam with ef allowed entries ENDS at its ef-th allowed entry, disallowed entries
 *               behind it go too, and a beam with fewer allowed entries holds up to `width`
 *               entries, mostly disallowed ones: the frontier it walks through.
 *   Offer       B <- cut(B u {(dist(q, v), v) : v in S}), every id once, new entries unexpanded.
 *               Disallowed entries are expanded like any other: the traversal walks through them.
 *               Seeds need not be allowed.
 *   Answer      the first k allowed entries of B, count = min(k, allowed entries of B); unused slots
 *               hold id -1 and distance +inf.
 * Three properties:
 *   Consistency  cut(cut(A) u S) = cut(A u S): the entry at min(t_a, t_w) is itself in the beam and
 *               witnesses the limit, and both limits only tighten as entries are added.  Hence B is
 *               always cut of everything offered so far: an id rejected or evicted once can never
 *               enter later, a point is expanded at most once, the loop ends after at most n
 *               expansions, and the visited filter (an exact visited set, a lossy one, or none;
 *               graph_search_nofilter) changes no answer and not `expansions`.  (The rule "the
 *               longest sorted prefix with at most width entries and at most ef allowed ones" is
 *               NOT this one: it forgets a rejected allowed entry and lets later, farther entries
 *               in, so its answer depends on the visited set.)
 *   Identity    With every id allowed (a null bitmap or all ones) t_a is the ef-th entry and
 *               width >= ef, so B is the first ef: the ids, the distance bits, the counts and
 *               `expansions` are those of rpt_graph_search_* / _csr_* / _csr_metric_* on the same
 *               inputs, whatever `width` is.  `evaluated` keeps its defined bounds; it is equal too
 *               under graph_search_nofilter = 1 (the hash is sized by width).
 *   width = ef  is post-filtering: the answer is the allowed entries of the unfiltered beam.
 * One wave answers a query and no atomics touch a beam: the same bits whatever the launch shape and
 * whatever graph_search_nofilter and graph_search_csr_stream are set to.  Every valid combination of
 * arguments launches: the beam, the filter, the offer's rows and the resident query take up to about
 * 46 KB of LDS per wave, and a workgroup is 4, 2 or 1 waves, whichever keeps the most waves on a
 * compute unit.  rpt_graph_search_last reports these calls too.
 * Errors: those of rpt_graph_search_* (a dense / CSR pair, any other `metric` value, both metric bits
 * together, RPT_KNN_METRIC_REFERENCE, k, ef, s or kg out of range, flags other than 0: RPT_E_ARG), and
 * width outside [ef, RPT_GRAPH_SEARCH_MAX_WIDTH]: RPT_E_ARG.  CSR data is NOT refused here.  Always
 * valid: n = 0, nq = 0, an all-zero bitmap (every count is 0), a null bitmap.  _host validates the
 * graph and the seeds as rpt_graph_search_host does, reads and uploads ceil(n / 32) words of
 * allow_host, and synchronises; _dev borrows device arrays, does not synchronise and does NOT
 * validate.  A refused call leaves the context usable. */
#define RPT_GRAPH_SEARCH_MAX_WIDTH 1024
int32_t rpt_graph_search_allow_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                   int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev,
                                   int32_t s, const int32_t* seeds_dev, const uint32_t* allow_dev,
                                   int32_t k, int32_t ef, int32_t width, int32_t metric, int32_t flags,
                                   int32_t* ids_dev, double* dist_dev, int32_t* count_dev);
int32_t rpt_graph_search_allow_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                    int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                                    int32_t s, const int32_t* seeds_host, const uint32_t* allow_host,
                                    int32_t k, int32_t ef, int32_t width, int32_t metric, int32_t flags,
                                    int32_t* ids_host, double* dist_host, int32_t* count_host);

/* ---- insert new rows into a kNN graph ----
 * rpt_graph_insert_* grows a graph: the rows that were added to a data set find their neighbours
 * with the beam search and are linked in both directions, and nothing is rebuilt.  With the allow-list
 * (deletions) this makes the graph a dynamic index.  One pair of entry points serves dense data (f64,
 * f32, bf16) and CSR data (f64, f32) under `metric` 0, RPT_KNN_METRIC_COSINE and RPT_KNN_METRIC_INNER.
 * Inputs:
 *   data        a data set of N = n + m rows; its LAST m rows are the new ones.
 *   gids, gdist, gcount   a graph over the first n rows in rpt_knn_graph_*'s layout: ids[n][kg],
 *               dist[n][kg], count[n], kg in [1, RPT_GRAPH_MAX_K].  The stored distances ARE read
 *               here.  The caller's graph is read only.
 *   m           >= 0, at most data.n.
 *   seeds       seeds[m][s], s in [1, 64], -1 an unused slot: where the search of new row n + i starts.
 *   ef          in [kg, RPT_GRAPH_SEARCH_MAX_EF].
 *   batch       >= 1: new rows per chunk.
 *   flags       0.
 * Output: oids[N][kg], odist[N][kg], ocount[N].
 * State.  G_0 is the input graph followed by m empty rows; v_0 = n rows are visible.  Chunk c is the
 * rows P_c = [v_c, min(v_c + batch, N)).
 *   Search      For every p in P_c, A_p is the answer of rpt_graph_search_*'s definition, word for word,
 *               with the query = row p of data, the graph = G_c, n replaced by v_c (seeds and graph
 *               ids outside [0, v_c) are skipped: a seed naming a row of an EARLIER chunk is valid, a
 *               seed naming a row of this or a later chunk is not), k = kg, this ef and this metric.
 *               The distance is the one the graph code uses for this layout and metric: the dense
 *               folds, the union fold for CSR rows under L2, dotS for CSR rows under cosine / inner
 *               product, with the cached norms for cosine.  All of them are symmetric bit for bit, so
 *               the distance found with p as the query is the distance a graph row of the other
 *               endpoint would store for p.
 *   Link        Row p of G_{c+1} is A_p: sorted by (distance, id), count = |A_p|, unused slots hold id
 *               -1 and distance +inf.  For every o < v_c named by at least one A_p of this chunk, row
 *               o of G_{c+1} is the first kg by (distance, id) (the order of the search: NaN behind
 *               every number, NaNs among themselves by id) of
 *                 (valid entries of row o of G_c) u {(d, p) : p in P_c, (d, o) in A_p}.
 *               Rows that no A_p names are carried over unchanged.  v_{c+1} = v_c + |P_c|.
 * The result is G after the last chunk: a pure function of (data, graph, m, seeds, ef, batch, metric).
 * The order in which reverse offers arrive plays no part: the row is the first kg of a set under a
 * total order.  Stated properties:
 *   Rows of one chunk do not see each other: the price of searching a chunk in parallel; `batch` is
 *               the knob, and a rpt_knn_graph_refine_* round afterwards links them.
 *   m = 0 copies the graph.
 *   A new row whose seeds are all invalid gets count 0 and links nothing.
 *   Untouched rows are copied verbatim by _dev, whatever they hold.
 *   Touched rows come out sorted with invalid entries dropped: slots at or beyond the count clamped to
 *               [0, kg], ids outside [0, N), and an id the row holds twice counts once, at its first
 *               slot (an offer whose id the row holds already is dropped too; neither happens in a
 *               graph over the first n rows).
 * No atomics touch a row and one wave writes it: the same bits whatever the launch shape and whatever
 * graph_search_nofilter and graph_search_csr_stream are set to.  The link of a chunk costs O(|P_c| kg)
 * whatever n is.  Scratch is sized by (N, batch, kg): 12 N + 24 min(batch, m) kg bytes.
 * rpt_graph_insert_last: chunks = the number of chunks; evaluated = the distances the searches
 * computed (bounds as rpt_graph_search_last's, summed); offered = reverse entries offered (the sum of
 * |A_p|); accepted = reverse entries that are in their target's row when that row is written.
 * rpt_graph_search_last then reports the last chunk's search.
 * Errors: kg, s or ef out of range, batch < 1, m < 0 or m > data.n, flags other than 0, any other
 * `metric` value, both metric bits together, RPT_KNN_METRIC_REFERENCE: RPT_E_ARG; no room for the
 * scratch: RPT_E_NOMEM.  _host validates the counts, ids in [0, n) and seeds in {-1} u [0, N) before
 * anything is uploaded, as rpt_graph_search_host does, names the offending row, and synchronises;
 * _dev borrows device arrays, does NOT validate and does not synchronise.  A refused call leaves the
 * context usable. */
int32_t rpt_graph_insert_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_dev,
                             const double* gdist_dev, const int32_t* gcount_dev, int64_t m, int32_t s,
                             const int32_t* seeds_dev, int32_t ef, int64_t batch, int32_t metric,
                             int32_t flags, int32_t* oids_dev, double* odist_dev, int32_t* ocount_dev);
int32_t rpt_graph_insert_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_host,
                              const double* gdist_host, const int32_t* gcount_host, int64_t m, int32_t s,
                              const int32_t* seeds_host, int32_t ef, int64_t batch, int32_t metric,
                              int32_t flags, int32_t* oids_host, double* odist_host, int32_t* ocount_host);
int32_t rpt_graph_insert_last(rpt_ctx* ctx, int64_t* chunks, int64_t* evaluated, int64_t* offered,
                              int64_t* accepted);

/* ---- delete rows from a kNN graph ----
 * rpt_graph_delete_* is the other half of a dynamic index: rows leave the graph without a rebuild.  A
 * tombstone bitmap (rpt_graph_search_allow_*) only hides rows; here the deleted rows are dropped,
 * every list that named one is repaired from the deleted row's own neighbours (the delete
 * consolidation of FreshDiskANN, adapted to graphs that store distances, order rows by (distance, id)
 * and answer bit for bit), and the survivors are optionally renumbered densely.  One pair of entry
 * points serves dense data (f64, f32, bf16) and CSR data (f64, f32) under `metric` 0,
 * RPT_KNN_METRIC_COSINE and RPT_KNN_METRIC_INNER.
 * Inputs:
 *   data        a data set of n rows.
 *   gids, gdist, gcount   a graph in rpt_knn_graph_*'s layout: ids[n][kg], dist[n][kg], count[n], kg in
 *               [1, RPT_GRAPH_MAX_K].  The stored distances ARE read.  The caller's graph is read
 *               only; the output arrays overlap none of the inputs.
 *   keep        the bitmap format of rpt_graph_search_allow_*: ceil(n / 32) uint32_t words, id i = bit
 *               i & 31 of word i >> 5, bits at positions >= n ignored, NULL = every row stays.  A set
 *               bit means the row STAYS: a tombstone bitmap a caller searches with is passed
 *               unchanged.
 *   flags       0 or RPT_GRAPH_DELETE_COMPACT.
 * Outputs: oids[n][kg], odist[n][kg], ocount[n] (sized for n rows) and newid[n] (int32; may be NULL).
 * Definition.  Ids are old ids throughout.  The VALID entries of row j are, as rpt_graph_insert_*
 * states for touched rows: the slots below the count clamped to [0, kg], whose id is in [0, n) and is
 * not j; an id the row holds twice counts once, at its first slot.  For a kept row p, K(p) is the
 * valid entries of row p whose id is kept, with their STORED distances, and D(p) is the ids of the
 * valid entries of row p that are deleted.
 *   Untouched row (D(p) is empty): copied slot for slot, whatever it holds, the distance bits verbatim;
 *               an id in [0, n) is replaced by newid of it, any other id is left as it is; the count
 *               is verbatim.
 *   Touched row (D(p) is not empty): with
 *                 C(p) = { e : e is the id of a valid entry of row j for some j in D(p), e is kept,
 *                          e != p, e is not an id of K(p) }, each id once,
 *               row p becomes the first kg, by the order of the search ((distance, id); NaN behind
 *               every number, NaNs among themselves by id; -0.0 ties with +0.0), of
 *                 K(p) u { (dist(p, e), e) : e in C(p) }.
 *               It is written sorted, the count is the size of the result, unused slots hold id -1 and
 *               distance +inf.  dist is the graph code's distance for the layout and metric: the dense
 *               folds, the union fold for CSR rows under L2, dotS for CSR rows under cosine / inner
 *               product, with the cached norms for cosine.  Those distances are symmetric bit for
 *               bit, so a new entry holds exactly the bits rpt_knn_graph_* or a refinement round would
 *               store for that pair.
 *   One hop only  A deleted neighbour's deleted neighbours are not followed: a row whose neighbours and
 *               all their neighbours are gone ends with fewer than kg entries, or none.  A
 *               rpt_knn_graph_refine_* round afterwards repairs such rows.
 *   Without RPT_GRAPH_DELETE_COMPACT  the output has n rows in old ids; a deleted row has count 0, ids
 *               -1 and distances +inf; newid[i] is i, or -1 for a deleted row.  The result is
 *               searchable with the unchanged data set: no kept row names a deleted one, so only
 *               seeds can reach one.
 *   With RPT_GRAPH_DELETE_COMPACT  newid[i] is the number of kept rows below i, or -1; the output has
 *               n' = popcount rows; row newid[p] is row p of the other form with every id mapped
 *               through newid; rows n' .. n of the output arrays are not written.  Compacting the
 *               data set is the caller's business.
 * The result is a pure function of (data, graph, keep, metric, flags): the same bits on every call and
 * every launch shape.  No atomics touch a row and one wave writes it.  Touched rows are repaired four
 * to a workgroup while four waves' shares of LDS fit, one to a workgroup beyond (dense rows at kg =
 * 64); the context option graph_delete_general sends every row there; the answer does not depend on
 * it.  Scratch is sized by n alone: 8 n bytes, 12 n when newid is NULL.
 * rpt_graph_delete_last: kept = the kept rows; touched = the touched rows; evaluated = the sum of
 * |C(p)|, the distances evaluated; dropped = the sum of |D(p)|, the valid entries of kept rows that
 * named a deleted row.  All four are sums.
 * Errors: kg out of range, flag bits other than RPT_GRAPH_DELETE_COMPACT, any other `metric` value,
 * both metric bits together, RPT_KNN_METRIC_REFERENCE: RPT_E_ARG; no room for the scratch:
 * RPT_E_NOMEM.  _host validates the counts and ids in [0, n) before anything is uploaded, as
 * rpt_graph_insert_host does, names the offending row, and synchronises; with COMPACT it writes the n'
 * rows of the answer and leaves the rest of the caller's arrays as they were.  _dev borrows device
 * arrays, does NOT validate and does not synchronise: with junk rows it stays in bounds and
 * terminates, untouched rows verbatim and touched rows cleaned.  n = 0, keep = nothing and keep =
 * everything are valid.  A refused call leaves the context usable. */
#define RPT_GRAPH_DELETE_COMPACT 1
int32_t rpt_graph_delete_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_dev,
                             const double* gdist_dev, const int32_t* gcount_dev, const uint32_t* keep_dev,
                             int32_t metric, int32_t flags, int32_t* oids_dev, double* odist_dev,
                             int32_t* ocount_dev, int32_t* newid_dev);
int32_t rpt_graph_delete_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_host,
                              const double* gdist_host, const int32_t* gcount_host, const uint32_t* keep_host,
                              int32_t metric, int32_t flags, int32_t* oids_host, double* odist_host,
                              int32_t* ocount_host, int32_t* newid_host);
int32_t rpt_graph_delete_last(rpt_ctx* ctx, int64_t* kept, int64_t* touched, int64_t* evaluated,
                              int64_t* dropped);

/* ---- query the kNN graph on SVector (CSR) rows, under L2 ----
 * rpt_graph_search_csr_* is rpt_graph_search_* for a CSR data set and CSR queries (rpt_dataset_csr_*,
 * f64 or f32 values, the same d and the same dtype); the parameter lists are the dense ones.  With
 * dense(x) as rpt_knn_graph_csr_* defines it (absent columns are +0.0, f32 values are widened
 * exactly, a stored zero is a zero), everything stated for rpt_graph_search_* carries over word for
 * word with dist(q, v) = metricDDL2's left fold over dense(q), dense(x_v), no FMA, one sqrt: the
 * beam, the offers, the order (distance, id) with NaN behind every number and NaNs among themselves
 * by id, the answer, counts and unused slots (id -1, distance +inf), termination after at most n
 * expansions, the visited filter that only saves work (graph_search_nofilter), _dev skipping ids
 * and counts out of range without validating, _host validating the graph and the seeds before
 * anything is uploaded (the same messages) and synchronising, rpt_prof_* class 3, rpt_knn_last_*
 * untouched.  rpt_graph_search_last serves both pairs of entry points: it reports the last call of
 * either.
 *   Bit-equal to the dense entry points  The kernel visits the union of the two supports only: a
 *                column where both hold +0.0 contributes acc + (+0.0), which is acc for every acc
 *                the fold can hold (it starts at +0.0 and, a sum of squares, never becomes -0.0).
 *                The fold over any ascending superset of the union of the two supports gives the
 *                same bits, so the answer and both statistics' definitions are bit-equal to
 *                rpt_graph_search_* on the dense-ified data and queries with the same graph and
 *                seeds.  A query and a row without nonzeros are at distance 0.
 *   metric       must be 0.  RPT_KNN_METRIC_COSINE and RPT_KNN_METRIC_INNER: RPT_E_UNSUPPORTED (the
 *                parameter is there so that they need no new symbol); any other value, both bits
 *                together, RPT_KNN_METRIC_REFERENCE: RPT_E_ARG.  The two distances are served by
 *                rpt_graph_search_csr_metric_* (below), which the message names.
 *   The query in LDS  A candidate's row is merged against the query's (column, value) pairs.  A
 *                query of at most min(d, 2048) entries stays in LDS for its whole search; a longer
 *                one passes through LDS in pieces of 64 per offer.  The context option
 *                graph_search_csr_stream = 1 sends every query down the second path; the answer and
 *                both statistics do not depend on it.  There is no limit on a row's length or on d.
 *   Ascending columns  A row's columns must ascend strictly; for rows or queries that break the
 *                invariant the answer is unspecified, but the kernel stays in bounds and terminates.
 * Errors, all RPT_E_ARG: a dense data set (the message names rpt_graph_search_*), a dense / CSR
 * pair, d or dtype differing between data and queries, kg, s or k outside [1, 64], ef outside
 * [k, RPT_GRAPH_SEARCH_MAX_EF], flags other than 0.  n = 0, nq = 0, n = 1, rows and queries without
 * nonzeros are valid.  A refused call writes nothing and leaves the statistics and the context
 * usable.  rpt_graph_search_* keeps refusing CSR data (RPT_E_UNSUPPORTED). */
int32_t rpt_graph_search_csr_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                 int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                                 const int32_t* seeds_dev, int32_t k, int32_t ef, int32_t metric,
                                 int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev);
int32_t rpt_graph_search_csr_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                  int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                                  int32_t s, const int32_t* seeds_host, int32_t k, int32_t ef,
                                  int32_t metric, int32_t flags, int32_t* ids_host, double* dist_host,
                                  int32_t* count_host);

/* ---- prepare the kNN graph for the search: diversify, reverse union, degree cap ----
 * What PyNNDescent does between building a graph and searching it.  Input: the dense data set `data`
 * (f64, f32 or bf16 rows), a graph ids[n][k], dist[n][k], count[n] in rpt_knn_graph_*'s layout (k in
 * [1, RPT_GRAPH_MAX_K]), kout in [1, RPT_GRAPH_MAX_K], `metric`: 0 (L2), RPT_KNN_METRIC_COSINE or
 * RPT_KNN_METRIC_INNER, and `flags`: an or of RPT_GRAPH_PREP_DIVERSIFY and RPT_GRAPH_PREP_REVERSE.
 * Output: a second graph out_ids[n][kout], out_dist[n][kout], out_count[n]; the input arrays are
 * const and are never written.  For a point i:
 *   Kept(i)   without DIVERSIFY: the valid entries of row i.  With DIVERSIFY: walk row i in stored
 *             order e_0, e_1, ...; e_m is kept unless some ALREADY KEPT e_l (l < m) has
 *             dist(e_l, e_m) < the distance stored with e_m in row i ("e_l occludes e_m").  A plain
 *             <: a comparison with NaN is false, so NaN keeps; ids do not break ties, an equal
 *             distance does not occlude.  e_0 is always kept.
 *   dist(e_l, e_m)  the fold of rpt_knn_graph_metric_*: a left fold in double over ascending
 *             columns, elements widened exactly, every operation rounded on its own, no FMA, the
 *             cached dot(x, x) of the rows for cosine.  It is symmetric bit for bit, so each
 *             unordered pair of a row is evaluated once.  The metric must be the one the stored
 *             distances were computed under (not detected).
 *   Union(i)  without REVERSE: Kept(i).  With REVERSE: Kept(i) u {j : i in Kept(j)}, a SET.  A
 *             reverse entry j carries the distance stored with i in row j; if j is in Kept(i) too,
 *             the distance stored in row i wins (this only matters for an inconsistent input).
 *   row i of the output   the first kout of Union(i) by (distance, id), NaN behind every number,
 *             NaNs among themselves by id; out_count[i] = min(kout, |Union(i)|); unused slots hold
 *             id -1 and distance +inf.
 * Consequences.  A duplicate of a kept neighbour (another id, an equal row) is dropped: it lies at
 * distance 0 from it.  Duplicates of x_i itself (stored distance 0) are all kept: nothing is below
 * 0.  A zero row under cosine is NaN against everything, so it is never occluded and never
 * occludes.  flags = 0 with kout = k reproduces a graph with sorted rows bit for bit.  The output of
 * DIVERSIFY alone is a valid input again (PyNNDescent's second pass is a second call).  With
 * REVERSE and kout >= every |Union(i)| the output is symmetric: j in row i <=> i in row j.
 * The two steps are separate switches on purpose: the occlusion rule assumes a metric.  Under the
 * inner product, which is none, DIVERSIFY costs recall and is not recommended; REVERSE still helps.
 * The result is a pure function of the inputs, the same bits on every call, whatever the launch
 * shape: one wave owns a row, no atomics touch a list.  The reverse lists are built with atomics
 * (as the refinement's), so the order inside one depends on arrival; the answer is the first kout
 * of a set under a total order and does not.
 * rpt_graph_prepare_last (synchronises the stream), three sums over i of the last call on ctx:
 *   pairs     c_i (c_i - 1) / 2 with DIVERSIFY, c_i the valid entries of row i, else 0: the
 *             distances evaluated, every pair of a row once
 *   occluded  c_i - |Kept(i)|
 *   capped    |Union(i)| - out_count[i]
 * Errors: k or kout outside [1, RPT_GRAPH_MAX_K], other flag bits, any other `metric` value, both
 * metric bits together, RPT_KNN_METRIC_REFERENCE: RPT_E_ARG.  CSR data: RPT_E_UNSUPPORTED.  Scratch
 * (the kept graph and the reverse lists: about 24 k + 20 bytes per point) comes from the context's
 * pool: RPT_E_NOMEM.  n = 0 and n = 1 are valid.  A refused call writes nothing and leaves the
 * statistics as they were.
 * _host checks the graph BEFORE anything is uploaded, with the checks and messages of
 * rpt_knn_graph_refine_host (count in [0, k], ids in [0, n), id != i, no id twice in a row;
 * RPT_E_ARG naming the row); it synchronises.  _dev borrows device arrays, enqueues on the ctx
 * stream, does not synchronise (rpt_ctx_sync before reading) and does NOT validate: a count is
 * clamped to [0, k] and an id outside [0, n) is skipped, as if the entry were not in the row.  Timed
 * under rpt_prof_* class 3.  A call leaves rpt_knn_last_* and the forests' ranking tiers untouched. */
#define RPT_GRAPH_PREP_DIVERSIFY 1
#define RPT_GRAPH_PREP_REVERSE 2
int32_t rpt_graph_prepare_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_dev,
                              const double* dist_dev, const int32_t* count_dev, int32_t kout,
                              int32_t metric, int32_t flags, int32_t* out_ids_dev, double* out_dist_dev,
                              int32_t* out_count_dev);
int32_t rpt_graph_prepare_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_host,
                               const double* dist_host, const int32_t* count_host, int32_t kout,
                               int32_t metric, int32_t flags, int32_t* out_ids_host, double* out_dist_host,
                               int32_t* out_count_host);
int32_t rpt_graph_prepare_last(rpt_ctx* ctx, int64_t* pairs, int64_t* occluded, int64_t* capped);

/* ---- prepare the kNN graph for the search on SVector (CSR) rows, under L2 ----
 * rpt_graph_prepare_csr_* is rpt_graph_prepare_* for a CSR data set (rpt_dataset_csr_*, f64 or f32
 * values); the parameter lists are the dense ones, `metric` included.  With dense(x) as
 * rpt_knn_graph_csr_* defines it (absent columns are +0.0, f32 values are widened exactly, a stored
 * zero is a zero), everything stated for rpt_graph_prepare_* carries over word for word with
 * dist(e_l, e_m) = metricDDL2's left fold over dense(x_l), dense(x_m), no FMA, one sqrt: Kept(i) and
 * its plain <, Union(i), the first kout by (distance, id) with NaN behind every number, unused slots
 * (id -1, distance +inf), the three statistics, _host validating the graph before anything is
 * uploaded (the same checks and messages) and synchronising, _dev clamping a count to [0, k] and
 * skipping ids out of range without validating, the scratch from the context's pool (RPT_E_NOMEM),
 * rpt_prof_* class 3, rpt_knn_last_* untouched, n = 0 and n = 1 valid.  rpt_graph_prepare_last serves
 * both pairs of entry points: it reports the last call of either.
 *   Bit-equal to the dense entry points  Only DIVERSIFY reads data rows.  Its kernel visits the
 *                union of two neighbours' supports only: a column where both hold +0.0 contributes
 *                acc + (+0.0), which is acc for every acc the fold can hold (it starts at +0.0 and,
 *                a sum of squares, never becomes -0.0).  The fold over any ascending superset of the
 *                union of the two supports gives the same bits, so the output and all three
 *                statistics are bit-equal to rpt_graph_prepare_* on the dense-ified rows with the
 *                same graph.  Two rows without nonzeros are at distance 0 (0 < 0 is false: kept).
 *   metric       must be 0.  RPT_KNN_METRIC_COSINE and RPT_KNN_METRIC_INNER: RPT_E_UNSUPPORTED (the
 *                parameter is there so that they need no new symbol); any other value, both bits
 *                together, RPT_KNN_METRIC_REFERENCE: RPT_E_ARG.  The two distances are served by
 *                rpt_graph_prepare_csr_metric_* (below), which the message names.
 *   The neighbours in LDS  A pair's distance is a two-pointer merge over the two rows' (column,
 *                value) pairs.  Every neighbour row takes part in c - 1 pairs, so a point whose
 *                neighbours hold at most 1536 entries together (12 bytes each: two workgroups of
 *                four points fit a CU's 160 KB for every k) has them copied into LDS once, values
 *                widened once, and its pairs merge out of LDS (resident); any other point's pairs
 *                walk their rows through global loads, which needs no LDS per entry.  The choice is
 *                per point, both paths fold the same entries in the same order.  The context option
 *                graph_prepare_csr_resident lowers the cap (n > 0) or sends every point down the
 *                second path (-1); the output and the statistics do not depend on it.  There is no
 *                limit on a row's length or on d.
 *   Ascending columns  A row's columns must ascend strictly; for rows that break the invariant the
 *                answer is unspecified, but the kernel stays in bounds and terminates.
 * Errors: a dense data set: RPT_E_ARG (the message names rpt_graph_prepare_*); k or kout outside
 * [1, RPT_GRAPH_MAX_K], other flag bits: RPT_E_ARG, as the dense entry points.  A refused call writes
 * nothing and leaves the statistics and the context usable.  rpt_graph_prepare_* keeps refusing CSR
 * data (RPT_E_UNSUPPORTED). */
int32_t rpt_graph_prepare_csr_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_dev,
                                  const double* dist_dev, const int32_t* count_dev, int32_t kout,
                                  int32_t metric, int32_t flags, int32_t* out_ids_dev, double* out_dist_dev,
                                  int32_t* out_count_dev);
int32_t rpt_graph_prepare_csr_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_host,
                                   const double* dist_host, const int32_t* count_host, int32_t kout,
                                   int32_t metric, int32_t flags, int32_t* out_ids_host, double* out_dist_host,
                                   int32_t* out_count_host);

/* ---- query and prepare the kNN graph on SVector (CSR) rows, under cosine / inner product ----
 * rpt_graph_search_csr_metric_* and rpt_graph_prepare_csr_metric_* are rpt_graph_search_csr_* and
 * rpt_graph_prepare_csr_* with the same parameter lists, word for word (`metric` already stands before
 * `flags`), and with `metric` honoured: 0, RPT_KNN_METRIC_COSINE or RPT_KNN_METRIC_INNER.  They
 * prepare and search the graph that rpt_knn_graph_csr_metric_* / rpt_knn_graph_refine_csr_metric_*
 * build.  Everything stated for the L2 entry points carries over word for word (the beam, the offers
 * and the seeds, Kept(i) and its plain <, Union(i), the order (distance, id), counts and unused slots,
 * termination after at most n expansions, _host validating before anything is uploaded, _dev skipping
 * what is out of range, n = 0 / 1 and nq = 0, rpt_prof_* class 3, the options graph_search_nofilter,
 * graph_search_csr_stream and graph_prepare_csr_resident, on none of which the answer depends);
 * rpt_graph_search_last and rpt_graph_prepare_last serve these calls too.  The one thing that changes
 * is the distance, and it is the definition rpt_knn_csr_metric_* and rpt_knn_graph_csr_metric_* use,
 * word for word: dotS(x, y) starts at +0.0, takes the columns stored in BOTH rows in ascending
 * column order and folds acc = acc + x_c * y_c, every product and sum rounded on its own, f32
 * values widened exactly, no FMA.
 *   metric == 0            the bits of rpt_graph_search_csr_* / rpt_graph_prepare_csr_*
 *   RPT_KNN_METRIC_INNER   dist(x, y) = -dotS(x, y)
 *   RPT_KNN_METRIC_COSINE  dist(x, y) = 1 - dotS(x, y) / (sqrt(dotS(x, x)) * sqrt(dotS(y, y))), the
 *                          norms cached on the data set and, for the search, on the query set (8
 *                          bytes per row, on the first call); an empty or all-zero row or query is
 *                          at NaN from everything
 * NaN ranks behind every number, NaNs among themselves by id, so a query without nonzeros under
 * cosine still gets min(k, what the search reached) answers, ordered by id; -0.0 (the inner distance
 * of two rows that share no column) ties with +0.0, the id decides and the stored bits are the
 * computed ones.  In the preparation a NaN never occludes and is never occluded (a plain <).
 *   The merge    For dotS the two-pointer merge of the L2 kernels is the definition itself: a product
 *                is taken only where both cursors stand on one column, a step that advances one side
 *                does no arithmetic, and the walk ends with the shorter row: no tail, no zero-filled
 *                window, no presence word.
 *   Stored inf and NaN  While every stored value is finite, the answers are those of
 *                rpt_graph_search_* / rpt_graph_prepare_* under the same metric on the dense-ified
 *                rows bit for bit (a column only one row stores would add x * (+0.0) = +-0.0 to an
 *                accumulator that is never -0.0).  With a stored inf or NaN they are not: the dense
 *                fold meets inf * 0 = NaN where dotS takes no product.  The answer is dotS in both
 *                cases.
 *   LDS          What the L2 kernels take.  The cosine preparation keeps the neighbours' norms in
 *                registers (lane r: neighbour r) and fetches a pair's two by shuffle, so a workgroup
 *                stays at 80 928 B at k = 64 and two share a CU.
 *   Ascending columns  as above: unspecified answer, in bounds, terminates.
 * Errors: any other `metric` value, both metric bits together, RPT_KNN_METRIC_REFERENCE: RPT_E_ARG
 * (a metric bit in `flags` too).  Dense data: RPT_E_ARG, the message names rpt_graph_search_* /
 * rpt_graph_prepare_*, which keep refusing CSR data (RPT_E_UNSUPPORTED).  Everything else as
 * rpt_graph_search_csr_* / rpt_graph_prepare_csr_*; an error leaves the context usable.  Not built:
 * streamed forests, the reference's right-fold innerSS order. */
int32_t rpt_graph_search_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                        int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev,
                                        int32_t s, const int32_t* seeds_dev, int32_t k, int32_t ef,
                                        int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                                        int32_t* count_dev);
int32_t rpt_graph_search_csr_metric_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                         int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                                         int32_t s, const int32_t* seeds_host, int32_t k, int32_t ef,
                                         int32_t metric, int32_t flags, int32_t* ids_host, double* dist_host,
                                         int32_t* count_host);
int32_t rpt_graph_prepare_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                         const int32_t* ids_dev, const double* dist_dev,
                                         const int32_t* count_dev, int32_t kout, int32_t metric,
                                         int32_t flags, int32_t* out_ids_dev, double* out_dist_dev,
                                         int32_t* out_count_dev);
int32_t rpt_graph_prepare_csr_metric_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                          const int32_t* ids_host, const double* dist_host,
                                          const int32_t* count_host, int32_t kout, int32_t metric,
                                          int32_t flags, int32_t* out_ids_host, double* out_dist_host,
                                          int32_t* out_count_host);

/* multi-GPU merge: G per-shard results (shard g holds trees [g*T/G, (g+1)*T/G)), gathered
 * shard-major as ids_dev[G][nq][k] etc. (e.g. by an RCCL all-gather), merged into the
 * global top-k with the reference's stable order (shard ascending = tree ascending).
 * Any G >= 1 and k <= 1024: up to 4096 entries per query merge in one launch, larger merges
 * fold the shards in one at a time (same order). */
int32_t rpt_knn_merge_dev(rpt_ctx* ctx, const int32_t* ids_dev, const double* dist_dev,
                          const int32_t* count_dev, int32_t G, int64_t nq, int32_t k,
                          int32_t flags, int32_t* out_ids_dev, double* out_dist_dev,
                          int32_t* out_count_dev);
/* the same merge over G packed exchange records (ONE all-gather instead of three): a shard
 * writes its rpt_knn_dev results into one record — distances at off_dist, ids at off_ids,
 * counts at off_count, then ONE int32 status word (0 = the shard answered; anything else = it
 * failed and its lists are void), `bytes` in all (rpt_knn_record_layout; a multiple of 16) — the records
 * of all shards are gathered back to back (record_bytes apart, shard-major), and
 * rpt_knn_merge_records_dev merges them exactly like rpt_knn_merge_dev. */
int32_t rpt_knn_record_layout(int64_t nq, int32_t k, int64_t* bytes, int64_t* off_dist,
                              int64_t* off_ids, int64_t* off_count);
int32_t rpt_knn_merge_records_dev(rpt_ctx* ctx, const void* records_dev, int64_t record_bytes,
                                  int32_t G, int64_t nq, int32_t k, int32_t flags,
                                  int32_t* out_ids_dev, double* out_dist_dev,
                                  int32_t* out_count_dev);

/* ---- multi-GPU: tree shards per device, ONE RCCL all-gather per query batch ----
 * Reference contract: the trees of a forest are independent (createMulti maps create over the
 * IntMap, Internal.hs:234-240) and knn concatenates the per-tree candidates in key order before
 * one stable sort (RPTree.hs:174-176).  Rank r of G holds the contiguous tree block
 * [r*T/G, (r+1)*T/G) and a replica of the point set; the build needs no communication; a query
 * batch is answered per shard into one exchange record (rpt_knn_record_layout), the records are
 * all-gathered over xGMI (ncclAllGather on the ctx streams, librccl) and merged on every device
 * in (distance, shard, rank) order = the reference's order.  The result is identical to
 * rpt_knn_* on the whole forest on one device.
 *
 * A communicator is formed either by ONE process for n devices (rpt_comm_init: ncclCommInitAll,
 * one rpt_ctx and one host worker thread per device; the ctxs are owned by the communicator)
 * or by one process PER device (rpt_comm_init_rank with the caller's ctx; rank 0 makes the id
 * with rpt_comm_unique_id and the host distributes its RPT_COMM_UID_BYTES bytes, e.g. through
 * the launcher's store).  Per-device arguments (ds, data, queries, outputs) are arrays of
 * `nlocal` entries, entry g living on the device of rpt_comm_ctx(comm, g): n entries after
 * rpt_comm_init(n), one after rpt_comm_init_rank.
 *
 * Failures.  With one process per device a rank's error code is invisible to its peers, so a rank
 * whose query kernels fail still joins the all-gather — its record's status word set — and returns
 * its own error; every rank scans the gathered status words after the merge: if one is set, all
 * counts of the answer are -1 and the next rpt_comm_sync (rpt_knn_sharded calls it) returns
 * RPT_E_INTERNAL naming the rank.  A rank that cannot join at all (no memory for its record, the
 * collective cannot be enqueued) aborts its communicator (ncclCommAbort): peers see a failed
 * collective instead of a hang, and every later call on the communicator returns RPT_E_INTERNAL. */
#define RPT_COMM_UID_BYTES 128
typedef struct rpt_comm rpt_comm;
typedef struct rpt_sharded_forest rpt_sharded_forest;
int32_t rpt_comm_init(int32_t n_gpus, rpt_comm** out);
int32_t rpt_comm_unique_id(void* uid_out /*[RPT_COMM_UID_BYTES]*/);
int32_t rpt_comm_init_rank(rpt_ctx* ctx, int32_t nranks, int32_t rank,
                           const void* uid /*[RPT_COMM_UID_BYTES]*/, rpt_comm** out);
int32_t rpt_comm_destroy(rpt_comm* comm);
int32_t rpt_comm_info(const rpt_comm* comm, int32_t* nranks, int32_t* nlocal, int32_t* first_rank);
int32_t rpt_comm_ctx(rpt_comm* comm, int32_t local_index, rpt_ctx** ctx);   /* borrowed */
int32_t rpt_comm_sync(rpt_comm* comm);                    /* rpt_ctx_sync of every local ctx */
/* createMulti (Internal.hs:234-240) sharded: R_host is the WHOLE forest's [T][L][d] block (every
 * rank passes the same); local device g builds the trees of rank first_rank + g.  T >= nranks. */
int32_t rpt_forest_build_sharded(rpt_comm* comm, const rpt_dataset* const* ds,
                                 const double* R_host, int32_t T, int32_t L, int32_t min_leaf,
                                 int32_t flags, rpt_sharded_forest** out);
int32_t rpt_sharded_forest_free(rpt_sharded_forest* sf);
/* the shard of local device g as an ordinary forest handle (borrowed) and its tree block */
int32_t rpt_sharded_forest_local(rpt_sharded_forest* sf, int32_t local_index, rpt_forest** f,
                                 int32_t* first_tree, int32_t* n_trees);
/* knn (RPTree.hs:168-176) over the sharded forest.  _dev: every local device receives the merged
 * answer in its own output buffers ([nq][k] ids / distances, [nq] counts), enqueued on the ctx
 * streams (rpt_comm_sync before reading).  rpt_knn_sharded copies device 0's answer to the host. */
int32_t rpt_knn_sharded_dev(rpt_comm* comm, rpt_sharded_forest* sf,
                            const rpt_dataset* const* data, const rpt_dataset* const* queries,
                            int32_t k, int32_t flags, int32_t* const* ids_dev,
                            double* const* dist_dev, int32_t* const* count_dev);
int32_t rpt_knn_sharded(rpt_comm* comm, rpt_sharded_forest* sf, const rpt_dataset* const* data,
                        const rpt_dataset* const* queries, int32_t k, int32_t flags,
                        int32_t* ids_host, double* dist_host, int32_t* count_host);

/* brute-force exact kNN on the device (evaluation of recall; ties by ascending id) */
int32_t rpt_brute_knn_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                           int32_t k, int32_t* ids_host, double* dist_host);
/* ... under the metric of `flags`: 0 (L2, as rpt_brute_knn_host), RPT_KNN_METRIC_COSINE or
 * RPT_KNN_METRIC_INNER (the distances defined with those flags; ties by ascending id) */
int32_t rpt_brute_knn_metric_host(rpt_ctx* ctx, const rpt_dataset* data,
                                  const rpt_dataset* queries, int32_t k, int32_t flags,
                                  int32_t* ids_host, double* dist_host);
/* Both entry points take SVector (CSR) data with CSR queries too (same d, same dtype, f64 or f32
 * values; a dense / CSR pair is RPT_E_ARG).  The candidates are the rows 0 .. n-1; the answer is
 * the k best by (distance, id), NaN behind every number; with fewer than k rows the unused slots
 * are id -1, distance +inf.  Two distances, the two rpt_knn_* has on CSR data:
 *   flags 0                   the true Euclidean distance, evaluated as rpt_knn_* evaluates it:
 *                             sqrt(max(0, |q|^2 + sum over the row's nonzeros of ((x_j - q_j)^2 -
 *                             q_j^2))) in double, within about 1e-8 |q| absolute (|q|^2 is summed
 *                             in a row's order: a query that is a stored row is at distance
 *                             exactly 0 from it and from its copies)
 *   RPT_KNN_METRIC_REFERENCE  (rpt_brute_knn_metric_host) the reference's truncating metricSSL2
 *                             (Internal.hs:389-393 over binSS :435-450), bit-exact: what
 *                             `recallWith metricL2` of the reference computes on SVector rows.
 *                             Dense data: RPT_E_ARG, as before.
 * RPT_KNN_METRIC_COSINE / _INNER on CSR data: RPT_E_UNSUPPORTED.
 * (Those two distances on CSR data have entry points of their own: rpt_knn_csr_metric_*,
 * rpt_brute_knn_csr_metric_* and rpt_recall_hits_csr_metric_host, below.)
 * One workgroup answers a tile of queries (dense-ified in LDS) against a block of rows streamed
 * once; the option brute_csr_tile sets the tile, the answer does not depend on it. */
/* ... and into device arrays ids_dev / dist_dev [nq][k], for dense data (flags 0,
 * RPT_KNN_METRIC_COSINE, RPT_KNN_METRIC_INNER) and CSR data (flags 0, RPT_KNN_METRIC_REFERENCE):
 * enqueued on the ctx stream, not synchronised (rpt_ctx_sync before reading). */
int32_t rpt_brute_knn_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                          int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev);

/* recallWith (RPTree.hs:259-282) for a query batch, on the device, the division of :276-282 left
 * to the caller: hits_host[i][t] = | set(candidates(tree t, query i)) n set(truth_i) |, where
 * truth_i are the valid ids of the brute force of query i under `flags` (as rpt_brute_knn_dev: 0,
 * RPT_KNN_METRIC_COSINE / _INNER on dense data, RPT_KNN_METRIC_REFERENCE on CSR data); the
 * reference's value is the mean over t of hits[i][t] / k.  hits_host is [nq][T];
 * truth_ids_host, if not NULL, receives the truth ids [nq][k] (-1 = unused slot).  Dense and CSR
 * forests, batch and streamed.  A point counts once per tree.  The rpt_knn_last_* statistics are
 * untouched (but RPT_KNN_METRIC_COSINE / _INNER reset rpt_knn_last_uncertified, as
 * rpt_brute_knn_metric_host does). */
int32_t rpt_recall_hits_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                             const rpt_dataset* queries, int32_t k, int32_t flags,
                             int32_t* hits_host /*[nq][T]*/,
                             int32_t* truth_ids_host /*[nq][k], may be NULL*/);

/* ---- cosine and inner-product kNN on SVector (CSR) rows ----
 * rpt_knn_*, rpt_brute_knn_* and rpt_recall_hits_host for CSR data with CSR queries (same d, same
 * dtype, f64 or f32 values widened exactly) under RPT_KNN_METRIC_COSINE / _INNER.  The definition:
 * for two CSR rows with strictly ascending columns, dotS(x, q) starts at +0.0, takes the columns
 * stored in BOTH rows in ascending column order, and for each acc = acc + x_j * q_j: a left fold,
 * every product and sum rounded on its own, no FMA.
 *   RPT_KNN_METRIC_INNER : dist = -dotS(x, q)
 *   RPT_KNN_METRIC_COSINE: dist = 1 - dotS(x, q) / (sqrt(dotS(x, x)) * sqrt(dotS(q, q))), NaN for an
 *                          empty or all-zero row or query; NaN ranks last.
 * Equal to the dense definition for finite values: when every stored value of both rows is finite
 * this is RPT_KNN_METRIC_INNER / _COSINE of the dense-ified rows bit for bit (a column one side
 * lacks would add x * (+0.0) = +-0.0 to an acc that is never -0.0), so rpt_knn_* and
 * rpt_brute_knn_metric_* on the dense-ified data give the same ids and distance bits.
 * Different with a stored inf or NaN: the dense-ified fold meets inf * 0 = NaN, this one does not —
 * a column counts only where both rows store it, which is what the reference's innerSS
 * (Internal.hs:323) visits.  Not the reference's fold order: innerSS adds the same products from the
 * right, x0 q0 + (x1 q1 + (... + 0)), which differs in the last bits and is not built; the left fold
 * is chosen so that CSR and dense-ified data give one answer.
 * Selection: rpt_brute_knn_csr_metric_*: the k best of rows 0 .. n-1 by (distance, id).
 * rpt_knn_csr_metric_*: the k best of all candidates by (distance, candidate position) under the
 * duplicate rule of `flags`.  Both: NaN behind every number, unused slots id -1 and distance +inf,
 * -0.0 ties with +0.0 and the stored bits are the computed ones.
 * `flags`: the duplicate rule (rpt_knn_csr_metric_* only) or-ed with exactly one of
 * RPT_KNN_METRIC_COSINE / _INNER.  Neither bit or both: RPT_E_ARG (the L2 distance on CSR rows is
 * rpt_knn_* / rpt_brute_knn_*).  Dense data or a dense / CSR pair: RPT_E_ARG (dense rows under the
 * metrics are rpt_knn_* / rpt_brute_knn_metric_*).  RPT_KNN_METRIC_REFERENCE: RPT_E_ARG.
 * RPT_KNN_VOTE: RPT_E_UNSUPPORTED.  A dtype mismatch, or queries whose projection type is not the
 * forest's: RPT_E_ARG.
 * Candidates are ranked on a lane-parallel f64 dot; the entries of the best k + 8 different rows are
 * evaluated again as the fold and the cut is certified with RPT_KNN_METRIC_*'s rounding bound (a row
 * pair has at most d products); a query whose cut cannot be certified (ties, NaN or inf at the cut,
 * the cosine range rule) is answered again by an exact kernel.  rpt_knn_last_candidates and
 * rpt_knn_last_uncertified are served, rpt_knn_last_tier and rpt_knn_last_retries read 0; the option
 * knn_metric_exact sends every query to the exact kernel.  The exhaustive search streams the rows
 * as rpt_brute_knn_* does on CSR data: a tile of queries (option brute_csr_tile; the answer does
 * not depend on it) against a block of rows read once, every (query, row block) certifying its own
 * cut; a query with an uncertified block is answered again, whole, by the exact kernel.  The
 * first call caches the rows' dotS(x, x) on the dataset, 8 bytes per row.  The _dev variants
 * enqueue on the ctx stream as rpt_knn_dev / rpt_brute_knn_dev do. */
int32_t rpt_knn_csr_metric_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                const rpt_dataset* queries, int32_t k, int32_t flags,
                                int32_t* ids_host, double* dist_host, int32_t* count_host);
int32_t rpt_knn_csr_metric_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                               const rpt_dataset* queries, int32_t k, int32_t flags, int32_t* ids_dev,
                               double* dist_dev, int32_t* count_dev);
int32_t rpt_brute_knn_csr_metric_host(rpt_ctx* ctx, const rpt_dataset* data,
                                      const rpt_dataset* queries, int32_t k, int32_t flags,
                                      int32_t* ids_host, double* dist_host);
int32_t rpt_brute_knn_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data,
                                     const rpt_dataset* queries, int32_t k, int32_t flags,
                                     int32_t* ids_dev, double* dist_dev);
int32_t rpt_recall_hits_csr_metric_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                        const rpt_dataset* queries, int32_t k, int32_t flags,
                                        int32_t* hits_host /*[nq][T]*/,
                                        int32_t* truth_ids_host /*[nq][k], may be NULL*/);

/* ---- vote-threshold kNN for every row layout and distance, no candidate cap ----
 * The RPT_KNN_VOTE flag of rpt_knn_* keeps its fused path and its caps (dense rows under L2, k <= 64,
 * at most 1024 trees, a batch forest, at most 16384 candidates and 512 leaves per query); these
 * entry points serve the same definition everywhere else.
 * The definition: for a query, take the candidates of all T trees (rpt_candidates' lists);
 * count(id) is the number of entries equal to id (leaves of one tree are disjoint: the number of
 * trees that propose id).  The voted list is the ids with count >= v, ascending, each once
 * (keepCounts' order).  The answer is the first k of the voted list by (distance, id); NaN ranks
 * last; unused slots are id -1 and distance +inf; count[q] = min(k, number of voted ids).
 * The distance is exactly the one the non-voting entry point of the same (row layout, dtype, flag)
 * returns, with its fold order, certificate and exact rerun:
 *   dense f64, flags 0           metricDDL2's fold: certified cut + exact kernel (rpt_knn_* on f64 rows);
 *                                a tie wider than k + 8 at the cut is answered by the exact kernel
 *   dense f32 / bf16, flags 0    the f32 sum in its one fixed order
 *   dense, _COSINE / _INNER      the left-fold dot of RPT_KNN_METRIC_*
 *   CSR, flags 0                 the true Euclidean distance of rpt_knn_* on CSR rows
 *   CSR, _REFERENCE              the reference's truncating metricSSL2
 *   CSR, _COSINE / _INNER        dotS of rpt_knn_csr_metric_*
 * v in [1, 65535] (else RPT_E_ARG); k in [1, 1024]; any number of trees; dense f64 / f32 / bf16 and
 * CSR f64 / f32 data with queries of the same layout and dtype; batch and streamed forests.
 * `flags` is 0 or exactly one of RPT_KNN_METRIC_COSINE / _INNER / _REFERENCE.  RPT_E_ARG: two of
 * those bits together, RPT_KNN_METRIC_REFERENCE on dense data, any duplicate-rule bit (the voted
 * ids are distinct), a RPT_KNN_VOTE field (the threshold is the argument).  An error leaves the
 * context usable.
 * No query is refused for its candidate count: a workgroup per query sorts the candidate ids in LDS
 * (up to 16384 of them; option knn_vote_lds lowers the bound) or, above that, in a slab of global
 * memory, and compacts the runs of at least v in ascending order.  Scratch is sized from the query
 * plan and a fixed budget; a batch above it is processed in slices of queries (option
 * knn_vote_slice bounds a slice).  The answer does not depend on either option.
 * rpt_knn_last_voted: the voted ids of the last call over all queries = the distances evaluated.
 * rpt_knn_last_candidates and rpt_knn_last_uncertified are served, rpt_knn_last_tier and
 * rpt_knn_last_retries read 0.  The _dev variant takes device outputs and returns synchronised.
 * rpt_vote_candidates_host: the voted lists themselves (the reference's commented-out `counts` /
 * `keepCounts`), with rpt_candidates' two-call protocol: ids_host NULL returns *total (and
 * off_host[nq + 1], if given); the second call fills ids_host[cap >= total] and, unless NULL,
 * counts_host with count(id) of every voted id. */
int32_t rpt_knn_vote_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                          const rpt_dataset* queries, int32_t k, int32_t v, int32_t flags,
                          int32_t* ids_host, double* dist_host, int32_t* count_host);
int32_t rpt_knn_vote_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                         const rpt_dataset* queries, int32_t k, int32_t v, int32_t flags,
                         int32_t* ids_dev, double* dist_dev, int32_t* count_dev);
int32_t rpt_vote_candidates_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* queries, int32_t v,
                                 int64_t* off_host /*[nq+1], may be NULL*/, int32_t* ids_host,
                                 int32_t* counts_host /*may be NULL*/, int64_t cap, int64_t* total);
int32_t rpt_knn_last_voted(rpt_ctx* ctx, int64_t* total);

/* ---- an allow-list on the forest query and on the exhaustive kNN ----
 * `allow` is the bitmap of rpt_graph_search_allow_*, unchanged: ceil(n / 32) uint32 words; id i is bit
 * i & 31 of word i >> 5; bits at positions >= n are ignored; NULL means every id; one bitmap serves
 * the batch.
 * The forest query (rpt_knn_allow_*).  The candidate list of a query is rpt_candidates' list: trees
 * ascending, leaves left to right, duplicates kept.  The allowed list is that list with every entry
 * whose id is not allowed removed, in the same order.  The answer is what rpt_knn_* would answer if
 * the allowed list were the candidate list: the k best by (distance, position in the allowed list)
 * under the duplicate rule; NaN ranks last; count = min(k, entries the rule leaves); unused slots are
 * id -1, distance +inf.  The duplicate rule applies after the filter (RPT_KNN_DEDUP_DISTANCE before
 * the filter could keep a disallowed row and lose the allowed row at the same distance).  The
 * distances, fold orders, certificates and exact reruns are those of the existing general kernels of
 * the (row layout, dtype, distance) cell: with every id allowed the answer is rpt_knn_*'s, bit for
 * bit (ids, distance bits, counts); with any bitmap it equals "rank the whole candidate list, then
 * drop disallowed entries, then apply the rule and cut to k".
 * The exhaustive kNN (rpt_brute_knn_allow_*).  The answer is the k best allowed rows by (distance,
 * id), NaN last, unused slots -1 / +inf.  Distances are rpt_brute_knn_*'s for the cell: in every cell
 * except true L2 on CSR rows the answer is bit-equal to the brute force over the allowed rows alone
 * with ids mapped back through the ascending allowed ids; true L2 on CSR rows (flags 0) is the
 * tolerance-mode distance of rpt_brute_knn_* there (rtol 1e-9, atol 1e-12; a stored row is at exactly
 * 0 from itself), from the same tiled kernel behind a compile-time allow switch.
 * Recall (rpt_recall_hits_allow_host): hits[i][t] = the number of ids of truth_i among the candidates of
 * (tree t, query i), as rpt_recall_hits_host counts them, truth_i being the exhaustive answer among the allowed rows (unused slots -1).
 * One entry point routes every cell: dense f64 / f32 / bf16 and CSR f64 / f32 rows with queries of
 * the same layout and dtype; L2 (no metric bit), RPT_KNN_METRIC_COSINE, RPT_KNN_METRIC_INNER, and
 * RPT_KNN_METRIC_REFERENCE on CSR rows; batch and streamed forests; k in [1, 1024]; any number of
 * trees and of candidates.  Flags of rpt_knn_allow_*: the duplicate-rule bits (0, RPT_KNN_DEDUP,
 * RPT_KNN_DEDUP_DISTANCE) or-ed with at most one metric bit.  Refused with RPT_E_ARG, as rpt_knn_*
 * refuses them: both duplicate bits, RPT_KNN_METRIC_COSINE with _INNER, a metric with
 * RPT_KNN_METRIC_REFERENCE, unknown bits; also RPT_KNN_METRIC_REFERENCE on dense rows, k outside
 * [1, 1024], data and queries of different layout or dtype.  A RPT_KNN_VOTE field is
 * RPT_E_UNSUPPORTED.  rpt_brute_knn_allow_* / rpt_recall_hits_allow_host take a metric bit only (any
 * other bit: RPT_E_ARG).  An error leaves the context usable.
 * How: a compaction kernel writes each query's allowed list into a scratch slab (a workgroup per
 * query, a ballot and a workgroup prefix: stable), and the cell's general kernel ranks it as one
 * range; the exhaustive kNN ranks one ascending list of the allowed ids (popcount, scan, scatter),
 * except the true L2 on CSR rows, whose tiled kernel skips the rows whose bit is clear.
 * Scratch is sized from the query plan against a fixed 1 GiB budget, never from the free memory; a
 * batch above it is processed in slices of queries (option knn_allow_slice bounds a slice; the answer
 * does not depend on it).  The _host variants validate before anything is uploaded and upload the
 * ceil(n / 32) words; the _dev variants take device pointers (allow_dev too) and return synchronised.
 * rpt_allow_candidates_host: the allowed lists themselves, with rpt_candidates' two-call protocol:
 * ids_host NULL returns *total (and off_host[nq + 1], if given); the second call fills
 * ids_host[cap >= total].
 * rpt_knn_allow_last: the candidate entries and the allowed entries (= distances evaluated) of the
 * last rpt_knn_allow_* / rpt_allow_candidates_host call, summed over its queries.
 * rpt_knn_last_uncertified serves these calls; rpt_knn_last_tier / _retries read 0.
 * Not built: a bitmap per query in THESE entry points (a bitmap per query or per tenant is the
 * rpt_*_allow_group_* entry points below); the vote route (rpt_knn_vote_*, RPT_KNN_VOTE) under a filter; the
 * fused kernels under a filter (this route is the general path, as rpt_knn_vote_* is); sharded /
 * multi-GPU queries; rpt_knnh_host. */
int32_t rpt_knn_allow_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                           const rpt_dataset* queries, const uint32_t* allow_host, int32_t k, int32_t flags,
                           int32_t* ids_host, double* dist_host, int32_t* count_host);
int32_t rpt_knn_allow_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                          const rpt_dataset* queries, const uint32_t* allow_dev, int32_t k, int32_t flags,
                          int32_t* ids_dev, double* dist_dev, int32_t* count_dev);
int32_t rpt_allow_candidates_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* queries,
                                  const uint32_t* allow_host, int64_t* off_host /*[nq+1], may be NULL*/,
                                  int32_t* ids_host, int64_t cap, int64_t* total);
int32_t rpt_brute_knn_allow_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                 const uint32_t* allow_host, int32_t k, int32_t flags, int32_t* ids_host,
                                 double* dist_host);
int32_t rpt_brute_knn_allow_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                const uint32_t* allow_dev, int32_t k, int32_t flags, int32_t* ids_dev,
                                double* dist_dev);
int32_t rpt_recall_hits_allow_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                   const rpt_dataset* queries, const uint32_t* allow_host, int32_t k,
                                   int32_t flags, int32_t* hits_host /*[nq][T]*/,
                                   int32_t* truth_ids_host /*[nq][k], may be NULL*/);
int32_t rpt_knn_allow_last(rpt_ctx* ctx, int64_t* candidates, int64_t* allowed);

/* ---- allow-lists per query group: many tenants in one batch ----
 * Every rpt_*_allow_* entry point above takes ONE bitmap for the whole batch.  The rpt_*_allow_group_*
 * entry points take a GROUPED allow-list where `allow` stands there, three arguments:
 *   allow   G bitmaps of words = ceil(n / 32) uint32 each, row g at allow + g * words (the row stride
 *           is `words`, not n / 32).  The bit layout is the one above; bits at or behind n are ignored
 *           in every row.  May be NULL only when G == 0.
 *   G       >= 0.
 *   group   [nq] int32: query q searches under bitmap group[q]; -1 = every id is allowed (the null
 *           bitmap above).  NULL = every query is -1.
 * G tenants with many queries each, a bitmap per query (G = nq, group = 0 .. nq - 1) and a mix with
 * unfiltered queries are all this one shape.
 * Definition: the answer for query q is the answer of the single-bitmap entry point for that query
 * under bitmap allow[group[q]] (the null bitmap for -1), bit for bit: ids, distance bits, counts, the
 * padding -1 / +inf, in every cell those entry points serve (row layouts, dtypes, distances, the CSR
 * reference metric, batch and streamed forests, the duplicate rules, every k, ef and width).  The call
 * statistics (rpt_graph_search_last, rpt_knn_allow_last, rpt_knn_last_uncertified) are the sums over
 * the queries of what the per-bitmap calls report; `evaluated` under the lossy visited filter keeps
 * its bounds and is equal under graph_search_nofilter = 1.
 * Errors: every refusal of the single-bitmap entry point, with its code; G < 0, a NULL allow with
 * G > 0: RPT_E_ARG.  The _host variants also check group[q] in [-1, G) before anything is uploaded
 * (RPT_E_ARG), then upload G * words words and nq group entries.  The _dev variants borrow device
 * pointers and do not validate; they stay in bounds whatever group holds: a value outside [-1, G) is
 * DEFINED as "no id allowed" (count 0, padding only).  An error leaves the context usable.
 * How: every wave of the graph search, every workgroup of the compaction kernel and every tile query
 * of the CSR true-L2 kernel resolves its own bitmap row once.  The exhaustive kNN builds one ascending
 * id list per group that a query names (popcount, scan and scatter over a second grid dimension; a
 * group nobody names costs nothing), concatenated, and query q ranks the range of its group's list.
 * The lists are sized from their popcounts against the fixed 1 GiB budget; lists that do not fit
 * together are built and ranked in passes (option knn_allow_group_budget = ids per pass, for tests;
 * the answer does not depend on it).  Slicing of the forest query stays by queries (knn_allow_slice);
 * a slice may hold any mix of groups.
 * Not built: the vote route under a filter, the fused kernels under a filter, sharded queries,
 * rpt_knnh_host, a frontier beyond RPT_GRAPH_SEARCH_MAX_WIDTH. */
int32_t rpt_graph_search_allow_group_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                         int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev,
                                         int32_t s, const int32_t* seeds_dev, const uint32_t* allow_dev,
                                         int32_t G, const int32_t* group_dev, int32_t k, int32_t ef,
                                         int32_t width, int32_t metric, int32_t flags, int32_t* ids_dev,
                                         double* dist_dev, int32_t* count_dev);
int32_t rpt_graph_search_allow_group_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                          int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                                          int32_t s, const int32_t* seeds_host, const uint32_t* allow_host,
                                          int32_t G, const int32_t* group_host, int32_t k, int32_t ef,
                                          int32_t width, int32_t metric, int32_t flags, int32_t* ids_host,
                                          double* dist_host, int32_t* count_host);
int32_t rpt_knn_allow_group_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                 const rpt_dataset* queries, const uint32_t* allow_host, int32_t G,
                                 const int32_t* group_host, int32_t k, int32_t flags, int32_t* ids_host,
                                 double* dist_host, int32_t* count_host);
int32_t rpt_knn_allow_group_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                const rpt_dataset* queries, const uint32_t* allow_dev, int32_t G,
                                const int32_t* group_dev, int32_t k, int32_t flags, int32_t* ids_dev,
                                double* dist_dev, int32_t* count_dev);
int32_t rpt_allow_group_candidates_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* queries,
                                        const uint32_t* allow_host, int32_t G, const int32_t* group_host,
                                        int64_t* off_host /*[nq+1], may be NULL*/, int32_t* ids_host,
                                        int64_t cap, int64_t* total);
int32_t rpt_brute_knn_allow_group_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                       const uint32_t* allow_host, int32_t G, const int32_t* group_host,
                                       int32_t k, int32_t flags, int32_t* ids_host, double* dist_host);
int32_t rpt_brute_knn_allow_group_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                      const uint32_t* allow_dev, int32_t G, const int32_t* group_dev,
                                      int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev);
int32_t rpt_recall_hits_allow_group_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                         const rpt_dataset* queries, const uint32_t* allow_host, int32_t G,
                                         const int32_t* group_host, int32_t k, int32_t flags,
                                         int32_t* hits_host /*[nq][T]*/,
                                         int32_t* truth_ids_host /*[nq][k], may be NULL*/);

#ifdef __cplusplus
}
#endif
#endif
