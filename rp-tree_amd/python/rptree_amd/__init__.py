"""rptree_amd — host-side mirror of the Data.RPTree API surface over the MI355X C ABI.

The reference host language is Haskell (no GHC in this image), so this Python layer plays the
role the Haskell `Data.RPTree` wrapper would play: same function names, argument order and
meaning as the reference, calling the C ABI of include/rptree_hip.h.  Reference citations are
file:line in ocramz/rp-tree v0.7.1.

    forestBatch / treeBatch   Batch.hs:29-63
    knn                       RPTree.hs:168-176
    candidates                RPTree.hs:289-314
    recallWith                RPTree.hs:259-282
    rpTreeCfg / RPTreeConfig  Conduit.hs:123-141
    SVector / DVector / Embed Internal.hs:56-59,92-133
    leaves / levels / points / treeSize / leafSizes   Internal.hs:199-208, RPTree.hs:362-367
"""
import atexit
import ctypes as C
import math
import weakref
from collections import namedtuple

import numpy as np

from . import gen
from ._lib import (RPT_BF16, RPT_F32, RPT_F64, RPT_GRAPH_ACCUMULATE, RPT_GRAPH_MAX_K, RPT_GRAPH_SEARCH_MAX_EF,
                   RPT_GRAPH_SEARCH_MAX_WIDTH, RPT_GRAPH_DELETE_COMPACT, RPT_GRAPH_PREP_DIVERSIFY, RPT_GRAPH_PREP_REVERSE,
                   RPT_KNN_DEDUP, RPT_KNN_DEDUP_DISTANCE,
                   RPT_KNN_KEEP_DUPLICATES, RPT_KNN_METRIC_COSINE, RPT_KNN_METRIC_INNER,
                   RPT_KNN_METRIC_REFERENCE,
                   RPT_PROJ_AUTO, RPT_PROJ_EXACT, RPT_PROJ_MFMA, RPTError, check, lib)

__all__ = [
    "Context", "Dataset", "RPForest", "RPTree", "SVector", "DVector", "Embed", "fromListSv",
    "fromVectorSv", "fromListDv", "fromVectorDv", "forestBatch", "treeBatch", "knn", "knnBatch",
    "candidates", "recallWith", "rpTreeCfg", "RPTreeConfig", "leaves", "levels", "points",
    "treeSize", "leafSizes", "metricL2", "inner", "project", "splitSegments", "topology",
    "bruteKnn", "RPTError", "forest", "tree", "saveForest", "loadForest", "importForest",
    "knnH", "knnHBatch", "knnPQ", "candidatesBatch", "to_bf16", "from_bf16", "RPStreamForest",
    "metricCosine", "metricInner", "recallWithBatch", "recallHits",
    "knnGraph", "knnGraphDev", "knnGraphLastPairs",
    "knnGraphRefine", "knnGraphRefineDev", "knnGraphRefineLast",
    "knnGraphMetric", "knnGraphMetricDev", "knnGraphRefineMetric", "knnGraphRefineMetricDev",
    "knnGraphSV", "knnGraphSVDev", "knnGraphRefineSV", "knnGraphRefineSVDev",
    "knnGraphMetricSV", "knnGraphMetricSVDev", "knnGraphRefineMetricSV", "knnGraphRefineMetricSVDev",
    "graphSearch", "graphSearchDev", "graphSearchLast", "graphSearchSV", "graphSearchSVDev",
    "graphSearchAllow", "graphSearchAllowDev", "allowBitmap",
    "graphInsert", "graphInsertDev", "graphInsertLast",
    "graphDelete", "graphDeleteDev", "graphDeleteLast", "compactRows",
    "graphPrepare", "graphPrepareDev", "graphPrepareLast", "graphPrepareSV", "graphPrepareSVDev",
    "graphSearchMetricSV", "graphSearchMetricSVDev", "graphPrepareMetricSV", "graphPrepareMetricSVDev",
    "knnVote", "knnVoteDev", "voteCandidates", "knnVoteLast",
    "knnAllow", "knnAllowDev", "allowCandidates", "knnAllowLast", "bruteKnnAllow", "bruteKnnAllowDev",
    "recallHitsAllow", "recallWithAllowBatch",
    "allowBitmaps", "graphSearchAllowGroup", "graphSearchAllowGroupDev", "knnAllowGroup", "knnAllowGroupDev",
    "allowGroupCandidates", "bruteKnnAllowGroup", "bruteKnnAllowGroupDev", "recallHitsAllowGroup",
    "recallWithAllowGroupBatch",
]

_DT = {np.dtype(np.float64): RPT_F64, np.dtype(np.float32): RPT_F32}


def to_bf16(a):
    """float array -> bf16 bit patterns (uint16), round to nearest even (numpy has no bf16)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    out = ((u + r) >> 16).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    out[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return out


def from_bf16(u16):
    """bf16 bit patterns (uint16) -> float32 (exact)."""
    return (np.ascontiguousarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


# ---------------------------------------------------------------------------------------
# vector types (Internal.hs:92-133)
# ---------------------------------------------------------------------------------------
class SVector(namedtuple("SVector", "svDim svIdx svVal")):
    """Sparse vector: dimension + (index, value) components, indices ascending (unchecked in
    the reference, Internal.hs:99-105)."""
    __slots__ = ()


class DVector(namedtuple("DVector", "dvVec")):
    __slots__ = ()


Embed = namedtuple("Embed", "eEmbed eData")           # Internal.hs:56-59


def fromListSv(n, ll):                                # Internal.hs:106-107
    idx = np.array([i for i, _ in ll], dtype=np.int32)
    val = np.array([x for _, x in ll], dtype=np.float64)
    return SVector(int(n), idx, val)


def fromVectorSv(n, idx, val):                        # Internal.hs:116-119
    return SVector(int(n), np.asarray(idx, dtype=np.int32), np.asarray(val, dtype=np.float64))


def fromListDv(ll):                                   # Internal.hs:128-129
    return DVector(np.array(ll, dtype=np.float64))


fromVectorDv = fromListDv                             # Internal.hs:130-131


# ---------------------------------------------------------------------------------------
# parameters (Conduit.hs:123-141)
# ---------------------------------------------------------------------------------------
RPTreeConfig = namedtuple("RPTreeConfig", "fpMaxTreeDepth fpDataChunkSize fpProjNzDensity")


def rpTreeCfg(minl, n, d):
    """Conduit.hs:132-141: maxd = ceiling(logBase 2 (n/minl)); chunk = ceiling(n/100);
    pnz = min 1 (1/logBase 10 d)."""
    maxd = math.ceil(math.log(n / minl) / math.log(2.0))
    nchunk = math.ceil(n / 100)
    with np.errstate(divide="ignore"):
        pnz_min = 1.0 / (math.log(d) / math.log(10.0)) if d != 1 else math.inf
    return RPTreeConfig(int(maxd), int(nchunk), min(pnz_min, 1.0))


# ---------------------------------------------------------------------------------------
# handles
# ---------------------------------------------------------------------------------------
# Handles still alive when the interpreter exits (e.g. kept by a traceback) are released HERE,
# forests before datasets before contexts, while the HIP runtime is still up; a __del__ that
# ran during interpreter teardown would call into a runtime whose static state is gone.
_live = weakref.WeakSet()


def _close_all():
    objs = list(_live)
    for kind in ("ShardedForest", "RPForest", "Dataset", "Comm", "Context"):
        for o in objs:
            if type(o).__name__ == kind:
                try:
                    o.close()
                except Exception:
                    pass


atexit.register(_close_all)


class Context:
    """One MI355X device + stream (rpt_ctx).  Raises if there is no usable HIP device."""

    def __init__(self, device=0):
        h = C.c_void_p()
        check(lib().rpt_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._owns = True
        _live.add(self)

    @classmethod
    def _borrowed(cls, handle, device):
        """Wrap a ctx owned by someone else (rpt_comm_ctx): never destroyed from here."""
        self = cls.__new__(cls)
        self._h, self.device, self._owns = handle, int(device), False
        return self

    def sync(self):
        check(lib().rpt_ctx_sync(self._h))

    def set_option(self, name, value):
        """Algorithm switch of this context (rpt_ctx_set_option); returns the previous value."""
        old = self.get_option(name)
        check(lib().rpt_ctx_set_option(self._h, name.encode(), int(value)))
        return old

    def get_option(self, name):
        v = C.c_int64()
        check(lib().rpt_ctx_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def pool_probe(self, nbytes):
        """(bytes, poison): what a fresh nbytes block of the device allocator holds, and the
        RPT_POOL_POISON byte in force (-1 when poison is off) (rpt_debug_pool_probe)."""
        buf = (C.c_uint8 * int(nbytes))()
        poison = C.c_int32()
        check(lib().rpt_debug_pool_probe(self._h, int(nbytes), buf, C.byref(poison)))
        return bytes(buf), poison.value

    @property
    def stream(self):
        s = C.c_void_p()
        check(lib().rpt_ctx_stream(self._h, C.byref(s)))
        return s.value

    def close(self):
        if self._h is not None:
            if self._owns:
                lib().rpt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class Dataset:
    """Point set / query batch resident in HBM (rpt_dataset)."""

    def __init__(self, ctx, handle, n, d, dtype, is_csr, keep=None):
        self.ctx, self._h, self.n, self.d, self.dtype, self.is_csr = ctx, handle, n, d, dtype, is_csr
        self._keep = keep
        self._host = None
        _live.add(self)

    @staticmethod
    def dense(ctx, X, dtype=None):
        """Row-major host array -> HBM.  float64 / float32 arrays keep their type; a uint16 array
        with dtype=RPT_BF16 holds bf16 bit patterns (see to_bf16)."""
        X = np.ascontiguousarray(X)
        if X.ndim != 2:
            raise ValueError("dense data must be a 2-D array [n][d]")
        if dtype == RPT_BF16:
            if X.dtype != np.uint16:
                X = to_bf16(X)
            dt = RPT_BF16
        else:
            if X.dtype not in _DT:
                X = X.astype(np.float64)
            dt = _DT[X.dtype]
        h = C.c_void_p()
        check(lib().rpt_dataset_dense_host(ctx._h, _vp(X), X.shape[0], X.shape[1], dt, C.byref(h)))
        ds = Dataset(ctx, h, X.shape[0], X.shape[1], dt, False)
        ds._host = X if dt == RPT_F64 else None     # recallWith's value semantics read rows back
        return ds

    @staticmethod
    def dense_device(ctx, ptr, n, d, dtype, keep=None):
        """Borrow device memory (e.g. a torch tensor's data_ptr()); `keep` pins the owner.
        The ctx stream is NOT ordered against whatever stream produced that memory: the caller
        must have synchronised the producer (Dataset.from_torch does)."""
        h = C.c_void_p()
        check(lib().rpt_dataset_dense_dev(ctx._h, C.c_void_p(ptr), n, d, dtype, C.byref(h)))
        return Dataset(ctx, h, n, d, dtype, False, keep)

    @staticmethod
    def from_torch(ctx, t):
        """Borrow a contiguous 2-D torch tensor on ctx's device (float64 / float32 / bfloat16).
        torch's current stream is synchronised first: the library enqueues on its own
        non-blocking stream, which nothing else orders behind the kernels that filled `t`."""
        import torch
        dt = {torch.float64: RPT_F64, torch.float32: RPT_F32, torch.bfloat16: RPT_BF16}[t.dtype]
        if t.dim() != 2 or not t.is_contiguous() or t.device.index != ctx.device:
            raise ValueError("need a contiguous 2-D tensor on cuda:%d" % ctx.device)
        torch.cuda.current_stream(t.device).synchronize()
        return Dataset.dense_device(ctx, t.data_ptr(), t.shape[0], t.shape[1], dt, keep=t)

    @staticmethod
    def csr(ctx, rowptr, col, val, d):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val)
        if val.dtype not in _DT:
            val = val.astype(np.float64)
        h = C.c_void_p()
        check(lib().rpt_dataset_csr_host(ctx._h, _vp(rowptr), _vp(col), _vp(val), len(rowptr) - 1,
                                         int(d), _DT[val.dtype], C.byref(h)))
        return Dataset(ctx, h, len(rowptr) - 1, int(d), _DT[val.dtype], True)

    @staticmethod
    def csr_from_torch(ctx, rowptr, col, val, d):
        """Borrow CSR arrays held in torch tensors on ctx's device (int64 rowptr, int32 col,
        float64 / float32 val).  Not validated (see rpt_dataset_csr_dev); torch's current stream
        is synchronised first."""
        import torch
        dt = {torch.float64: RPT_F64, torch.float32: RPT_F32}[val.dtype]
        if rowptr.dtype != torch.int64 or col.dtype != torch.int32:
            raise ValueError("rowptr must be int64 and col int32")
        torch.cuda.current_stream(val.device).synchronize()
        n = rowptr.numel() - 1
        h = C.c_void_p()
        check(lib().rpt_dataset_csr_dev(ctx._h, C.c_void_p(rowptr.data_ptr()), C.c_void_p(col.data_ptr()),
                                        C.c_void_p(val.data_ptr()), n, int(d), dt, val.numel(),
                                        C.byref(h)))
        return Dataset(ctx, h, n, int(d), dt, True, keep=(rowptr, col, val))

    @staticmethod
    def of(ctx, data):
        """Pack `V.Vector (Embed v Double x)`-like input once at the boundary.  Accepts a
        Dataset, a 2-D array, (rowptr, col, val, d), a scipy CSR matrix, or a sequence of
        Embed / DVector / SVector values."""
        if isinstance(data, Dataset):
            return data
        if isinstance(data, np.ndarray):
            return Dataset.dense(ctx, data)
        if isinstance(data, tuple) and len(data) == 4 and not isinstance(data, (SVector,)):
            return Dataset.csr(ctx, *data)
        if hasattr(data, "indptr") and hasattr(data, "indices"):
            return Dataset.csr(ctx, data.indptr, data.indices, data.data, data.shape[1])
        vs = [x.eEmbed if isinstance(x, Embed) else x for x in data]
        if not vs:
            raise ValueError("empty dataset")
        if isinstance(vs[0], DVector):
            return Dataset.dense(ctx, np.stack([np.asarray(v.dvVec, dtype=np.float64) for v in vs]))
        if isinstance(vs[0], SVector):
            rowptr = np.zeros(len(vs) + 1, dtype=np.int64)
            rowptr[1:] = np.cumsum([len(v.svIdx) for v in vs])
            col = np.concatenate([v.svIdx for v in vs]).astype(np.int32)
            val = np.concatenate([v.svVal for v in vs]).astype(np.float64)
            return Dataset.csr(ctx, rowptr, col, val, vs[0].svDim)
        return Dataset.dense(ctx, np.asarray(vs, dtype=np.float64))

    def close(self):
        if self._h is not None:
            lib().rpt_dataset_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _query_dataset(ctx, like, q):
    """One query or a batch -> Dataset with the layout (dense/CSR) and dtype of `like`."""
    if isinstance(q, Dataset):
        return q, q.n
    npdt = np.float64 if like.dtype == RPT_F64 else np.float32
    if like.is_csr:
        if isinstance(q, SVector):
            q = [q]
        if isinstance(q, tuple) and len(q) == 4:
            return Dataset.csr(ctx, q[0], q[1], np.asarray(q[2], dtype=npdt), q[3]), len(q[0]) - 1
        rowptr = np.zeros(len(q) + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum([len(v.svIdx) for v in q])
        col = (np.concatenate([v.svIdx for v in q]) if len(q) else np.zeros(0)).astype(np.int32)
        val = (np.concatenate([v.svVal for v in q]) if len(q) else np.zeros(0)).astype(npdt)
        return Dataset.csr(ctx, rowptr, col, val, like.d), len(q)
    if isinstance(q, DVector):
        q = q.dvVec
    if like.dtype == RPT_BF16:       # data and queries share one element type on the device
        a = np.asarray(q)
        if a.dtype != np.uint16:
            a = to_bf16(a)
        if a.ndim == 1:
            a = a[None, :]
        return Dataset.dense(ctx, a, dtype=RPT_BF16), a.shape[0]
    a = np.asarray(q, dtype=npdt)
    if a.ndim == 1:
        a = a[None, :]
    return Dataset.dense(ctx, a), a.shape[0]


# ---------------------------------------------------------------------------------------
# forest (Internal.hs:139-182)
# ---------------------------------------------------------------------------------------
class RPTree:
    """View of one tree of a flat forest: `RPTree d l a` (Internal.hs:172-175)."""

    def __init__(self, forest, t):
        self.forest, self.t = forest, t

    @property
    def _rpVectors(self):
        R = self.forest.R[self.t]
        out = []
        for l in range(R.shape[0]):
            idx = np.nonzero(R[l])[0].astype(np.int32)
            out.append(SVector(R.shape[1], idx, R[l, idx]))
        return out


class RPForest:
    """`RPForest d a` = IntMap of trees keyed 0..T-1 (Internal.hs:182), held in HBM in the flat
    layout of include/rptree_hip.h; `perm`, `thr`, `mglo`, `mghi` copy it out."""

    def __init__(self, ctx, handle, data, R, max_depth, min_leaf, owns=True):
        self.ctx, self._h, self.data = ctx, handle, data
        self._owns = owns           # False: a shard borrowed from an rpt_sharded_forest
        self.R = R
        self.T, self.L, self.d = R.shape
        assert self.L == max_depth
        self.min_leaf = int(min_leaf)
        self.N = data.n
        self._perm = self._nodes = None
        _live.add(self)

    # IntMap-like access
    def __len__(self):
        return self.T

    def __getitem__(self, t):
        if not 0 <= t < self.T:
            raise KeyError(t)
        return RPTree(self, t)

    def __iter__(self):
        return (RPTree(self, t) for t in range(self.T))

    def keys(self):
        return range(self.T)

    @property
    def perm(self):
        if self._perm is None:
            p = np.empty((self.T, self.N), dtype=np.int32)
            check(lib().rpt_forest_get_perm(self._h, _vp(p)))
            self._perm = p
        return self._perm

    def _get_nodes(self):
        if self._nodes is None:
            nodes = (1 << self.L) - 1
            a = [np.empty((self.T, nodes), dtype=np.float64) for _ in range(3)]
            check(lib().rpt_forest_get_nodes(self._h, _vp(a[0]), _vp(a[1]), _vp(a[2])))
            self._nodes = a
        return self._nodes

    thr = property(lambda self: self._get_nodes()[0])
    mglo = property(lambda self: self._get_nodes()[1])
    mghi = property(lambda self: self._get_nodes()[2])

    def proj(self):
        dt = np.float64 if self.data.dtype == RPT_F64 else np.float32
        p = np.empty((self.T, self.L, self.N), dtype=dt)
        check(lib().rpt_forest_get_proj(self._h, _vp(p)))
        return p

    @property
    def mode(self):
        m = C.c_int32()
        check(lib().rpt_forest_get_mode(self._h, C.byref(m)))
        return m.value

    def stats(self):
        a, b = C.c_int64(), C.c_int64()
        check(lib().rpt_forest_stats(self._h, C.byref(a), C.byref(b)))
        return {"tie_nodes": a.value, "big_mid_nodes": b.value}

    def topology(self):
        return topology(self.N, self.L, self.min_leaf)

    def close(self):
        if self._h is not None:
            if self._owns:
                lib().rpt_forest_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def topology(n, max_depth, min_leaf):
    """DFS list of (level, heap, offset, size, is_leaf) — Internal.hs:289,495,503."""
    cnt = C.c_int64()
    check(lib().rpt_topology(n, max_depth, min_leaf, None, 0, C.byref(cnt)))
    out = np.empty((cnt.value, 5), dtype=np.int64)
    check(lib().rpt_topology(n, max_depth, min_leaf, _vp(out), cnt.value, C.byref(cnt)))
    return out


def _build(ctx, ds, R, maxd, minl, mode):
    R = np.ascontiguousarray(R, dtype=np.float64)
    T, L, d = R.shape
    if L != maxd:
        raise ValueError("hyperplane block has %d levels, maxDepth is %d" % (L, maxd))
    h = C.c_void_p()
    check(lib().rpt_forest_build(ctx._h, ds._h, _vp(R), T, L, int(minl), int(mode), C.byref(h)))
    return RPForest(ctx, h, ds, R, maxd, minl)


def forestBatch(seed, maxd, minl, ntrees, pnz, dim, src, *, ctx=None, mode=RPT_PROJ_AUTO,
                hyperplanes=None):
    """Batch.hs:48-63.  seed, max tree depth, min leaf size, number of trees, nonzero density of
    the projection vectors, their dimension, dataset.  The hyperplanes are sampled on the host
    exactly where the reference samples them (Batch.hs:59-61) unless `hyperplanes` (a dense
    [T][L][dim] block, e.g. produced by the real Haskell generator) is supplied."""
    ctx = ctx or default_context()
    ds = Dataset.of(ctx, src)
    if hyperplanes is None:
        _, R = gen.forest_hyperplanes(seed, ntrees, maxd, pnz, dim)
    else:
        R = np.asarray(hyperplanes, dtype=np.float64)
    if R.shape[2] != ds.d:
        # the reference never checks `dim` against the data; HBM indexing must
        raise ValueError("projection vector dimension %d != data dimension %d" % (R.shape[2], ds.d))
    return _build(ctx, ds, R, maxd, minl, mode)


def treeBatch(seed, maxDepth, minLeaf, pnz, dim, src, **kw):
    """Batch.hs:29-41 (= forestBatch with one tree: same draw order for a single tree)."""
    return forestBatch(seed, maxDepth, minLeaf, 1, pnz, dim, src, **kw)


class RPStreamForest(RPForest):
    """A forest built by the streaming insert (rpt_forest_stream_build): its trees have the
    EXPLICIT topology the fold over chunks produced — `kind[h]` 0 absent / 1 Bin / 2 Tip per heap
    slot (2^(L+1)-1 of them), a Tip's points = perm[t][leaf_off[h] : leaf_off[h] + leaf_len[h]] —
    the same for every tree.  `held` = points stored per tree (< N after the reference's data-loss
    branch, Internal.hs:277), `dropped` = how many that branch discarded (counted over the fold)."""

    def __init__(self, ctx, handle, data, R, max_depth, min_leaf):
        super().__init__(ctx, handle, data, R, max_depth, min_leaf)
        n = C.c_int64()
        check(lib().rpt_forest_get_topology(handle, C.byref(n), None, None, None, None, None))
        self.slots = n.value
        self.kind = np.empty(self.slots, dtype=np.int8)
        self.leaf_off = np.empty(self.slots, dtype=np.int64)
        self.leaf_len = np.empty(self.slots, dtype=np.int64)
        held, dropped = C.c_int64(), C.c_int64()
        check(lib().rpt_forest_get_topology(handle, C.byref(n), _vp(self.kind), _vp(self.leaf_off),
                                            _vp(self.leaf_len), C.byref(held), C.byref(dropped)))
        self.held, self.dropped = held.value, dropped.value

    def _get_nodes(self):
        if self._nodes is None:
            a = [np.empty((self.T, self.slots), dtype=np.float64) for _ in range(3)]
            check(lib().rpt_forest_get_nodes(self._h, _vp(a[0]), _vp(a[1]), _vp(a[2])))
            self._nodes = a
        return self._nodes

    thr = property(lambda self: self._get_nodes()[0])
    mglo = property(lambda self: self._get_nodes()[1])
    mghi = property(lambda self: self._get_nodes()[2])

    def topology(self):
        raise TypeError("a streamed forest has an explicit topology: kind / leaf_off / leaf_len")

    def tips(self, t):
        """{heap: ids} of tree t's Tips, heap order"""
        return {int(h): self.perm[t, self.leaf_off[h]:self.leaf_off[h] + self.leaf_len[h]]
                for h in np.nonzero(self.kind == 2)[0]}


def forest(seed, maxd, minl, ntrees, chunksize, pnz, dim, src, *, ctx=None, mode=RPT_PROJ_AUTO,
           hyperplanes=None):
    """Conduit.hs:104-121 `forest`: the streaming build with the reference's semantics — the source
    is cut into chunks of `chunksize` points (C.chunksOf: the last may be shorter) and every chunk
    is folded into every tree with `insert` (Internal.hs:245-297): a chunk part that meets a Bin is
    split at its OWN median and averaged into the threshold, a part that meets a Tip is put in
    front of its points, an empty part that meets a Bin drops the subtree (the reference's
    data-loss quirk, kept; `dropped` counts it).  Hyperplanes are sampled exactly like
    forestBatch's (same draw order, Conduit.hs:116-118).  Dense rows or SVector rows (a (rowptr, col,
    val, dim) tuple: `forest` is polymorphic in `Inner SVector v`, Conduit.hs:104-113).  With chunksize >= the
    number of points the result is forestBatch's forest (as a streamed-forest handle)."""
    ctx = ctx or default_context()
    xs = src if isinstance(src, (np.ndarray, Dataset, tuple)) else list(src)    # (tuple: CSR arrays + dim)
    ds = Dataset.of(ctx, xs)
    if hyperplanes is None:
        _, R = gen.forest_hyperplanes(seed, ntrees, maxd, pnz, dim)
    else:
        R = np.asarray(hyperplanes, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    if R.shape[2] != ds.d:
        raise ValueError("projection vector dimension %d != data dimension %d" % (R.shape[2], ds.d))
    T, L, _ = R.shape
    if L != maxd:
        raise ValueError("hyperplane block has %d levels, maxDepth is %d" % (L, maxd))
    h = C.c_void_p()
    check(lib().rpt_forest_stream_build(ctx._h, ds._h, _vp(R), T, L, int(minl), int(chunksize),
                                        int(mode), C.byref(h)))
    return RPStreamForest(ctx, h, ds, R, maxd, minl)


def tree(seed, maxDepth, minLeaf, chunksize, pnz, dim, src, **kw):
    """Conduit.hs:58-72 `tree`: see `forest`."""
    return forest(seed, maxDepth, minLeaf, 1, chunksize, pnz, dim, src, **kw)


def saveForest(path, forest_):
    """Flat on-disk format: hyperplanes, perm and node arrays in one .npz —
    a 10M-point forest needs no boxed `Embed`s.  The counterpart of serialiseRPForest
    (Internal.hs:185-188) for the flat layout; the data itself is not stored."""
    np.savez_compressed(path, R=forest_.R, min_leaf=forest_.min_leaf, N=forest_.N,
                        perm=forest_.perm, thr=forest_.thr, mglo=forest_.mglo, mghi=forest_.mghi,
                        mode=forest_.mode)


def loadForest(path, data, ctx=None):
    """deserialiseRPForest (Internal.hs:191-196) for the flat format: back into HBM via
    rpt_forest_import.  `data` is the point set the forest was built on."""
    ctx = ctx or (data.ctx if isinstance(data, Dataset) else default_context())
    z = np.load(path)
    ds = Dataset.of(ctx, data)
    if int(z["N"]) != ds.n:
        raise ValueError("forest was built on %d points, data has %d" % (int(z["N"]), ds.n))
    mode = int(z["mode"]) if "mode" in z.files else RPT_PROJ_AUTO
    return importForest(ctx, ds, z["R"], int(z["min_leaf"]), z["perm"], z["thr"], z["mglo"],
                        z["mghi"], mode=mode)


def importForest(ctx, data, R, min_leaf, perm, thr, mglo, mghi, mode=RPT_PROJ_AUTO):
    """Rebuild a device forest from flat arrays (e.g. after deserialiseRPForest).  mode: the
    projection mode the thresholds were computed with (queries project the same way)."""
    ds = Dataset.of(ctx, data)
    R = np.ascontiguousarray(R, dtype=np.float64)
    T, L, _ = R.shape
    h = C.c_void_p()
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (thr, mglo, mghi)]
    check(lib().rpt_forest_import(ctx._h, ds._h, _vp(R), T, L, int(min_leaf), _vp(perm),
                                  _vp(a[0]), _vp(a[1]), _vp(a[2]), C.byref(h)))
    check(lib().rpt_forest_set_mode(h, int(mode)))
    return RPForest(ctx, h, ds, R, L, min_leaf)


# ---- accessors (Internal.hs:199-208, RPTree.hs:362-367) ----
def leaves(tree):
    """All leaf buckets of a tree, left to right (ids)."""
    f, t = tree.forest, tree.t
    if isinstance(f, RPStreamForest):
        return _stream_leaves(f, t)
    topo = f.topology()
    return [f.perm[t, o:o + n] for (_, _, o, n, leaf) in topo if leaf]


def levels(tree):
    return tree.forest.L


def points(tree):
    if isinstance(tree.forest, RPStreamForest):
        return tree.forest.perm[tree.t, :tree.forest.held]
    return tree.forest.perm[tree.t]


def _stream_leaves(f, t):
    """Tips of a streamed tree in left-to-right (DFS) order"""
    out, stack = [], [0]
    while stack:
        h = stack.pop()
        if f.kind[h] == 2:
            out.append(f.perm[t, f.leaf_off[h]:f.leaf_off[h] + f.leaf_len[h]])
        elif f.kind[h] == 1:
            stack.append(2 * h + 2)
            stack.append(2 * h + 1)
    return out


def leafSizes(tree):
    if isinstance(tree.forest, RPStreamForest):
        return [len(x) for x in _stream_leaves(tree.forest, tree.t)]
    return [int(n) for (_, _, _, n, leaf) in tree.forest.topology() if leaf]


def treeSize(tree):
    return sum(leafSizes(tree))


# ---- algebra helpers on the host (single pairs; the batch lives on the device) ----
def inner(u, v):
    """Inner SVector DVector / SVector SVector / DVector DVector (Internal.hs:322-341) with the
    reference's summation order."""
    if isinstance(u, SVector) and isinstance(v, DVector):
        acc = 0.0
        m = min(len(u.svIdx), len(v.dvVec))
        for j in range(m - 1, -1, -1):
            acc = float(u.svVal[j]) * float(v.dvVec[u.svIdx[j]]) + acc
        return acc
    if isinstance(u, SVector) and isinstance(v, SVector):
        prods, a, b = [], 0, 0
        while a < len(u.svIdx) and b < len(v.svIdx):
            if u.svIdx[a] == v.svIdx[b]:
                prods.append(float(u.svVal[a]) * float(v.svVal[b]))
                a += 1
                b += 1
            elif u.svIdx[a] < v.svIdx[b]:
                a += 1
            else:
                b += 1
        acc = 0.0
        for p in reversed(prods):
            acc = p + acc
        return acc
    acc = 0.0
    for x, y in zip(u.dvVec, v.dvVec):
        acc = acc + float(x) * float(y)
    return acc


def metricL2(u, v):
    """metricDDL2 (Internal.hs:403-406) for dense pairs; the device kernels use the same
    definition (true Euclidean distance)."""
    a = np.asarray(u.dvVec if isinstance(u, DVector) else u, dtype=np.float64)
    b = np.asarray(v.dvVec if isinstance(v, DVector) else v, dtype=np.float64)
    return float(np.sqrt(np.sum((a - b) ** 2)))


def _dense_f64(u):
    # f32 elements (and bf16 ones, given as their float values: from_bf16) widen exactly
    return np.asarray(u.dvVec if isinstance(u, DVector) else u).astype(np.float64).ravel().tolist()


def _dot_fold(a, b):
    """innerDD (Internal.hs:384-385): ((0 + a0 b0) + a1 b1) + ..., each product and sum rounded."""
    acc = 0.0
    for x, y in zip(a, b):
        acc = acc + x * y
    return acc


def _dot_sv(u, v):
    """dotS of two SVectors (strictly ascending indices): from +0.0, over the indices stored in BOTH,
    in ascending order, acc = acc + u_j * v_j, each product and sum rounded.  The products inner()
    adds from the right (the reference's innerSS order), added from the left: the order that makes
    SVector and dense-ified rows agree bit for bit when the stored values are finite."""
    acc, a, b = 0.0, 0, 0
    ui, vi = np.asarray(u.svIdx).tolist(), np.asarray(v.svIdx).tolist()
    ux = np.asarray(u.svVal).astype(np.float64).tolist()
    vx = np.asarray(v.svVal).astype(np.float64).tolist()
    while a < len(ui) and b < len(vi):
        if ui[a] == vi[b]:
            acc = acc + ux[a] * vx[b]
            a += 1
            b += 1
        elif ui[a] < vi[b]:
            a += 1
        else:
            b += 1
    return acc


def _metric_dots(u, v):
    # (u.v, u.u, v.v): dotS for two SVectors, the dense left fold otherwise
    if isinstance(u, SVector) or isinstance(v, SVector):
        if not (isinstance(u, SVector) and isinstance(v, SVector)):
            raise TypeError("metricInner / metricCosine: two SVectors or two dense vectors")
        return _dot_sv(u, v), _dot_sv(u, u), _dot_sv(v, v)
    a, b = _dense_f64(u), _dense_f64(v)
    return _dot_fold(a, b), _dot_fold(a, a), _dot_fold(b, b)


def metricInner(u, v):
    """-(inner u v): the inner-product distance of the device's RPT_KNN_METRIC_INNER (maximum
    inner-product search; smaller is nearer), the dot a left fold in Double from +0.0.
    Two SVectors: the fold runs over the indices stored in both, in ascending order (what
    rpt_knn_csr_metric_* evaluates): the dense value of the dense-ified vectors when the stored
    values are finite; a stored inf / NaN counts only where both vectors store the index."""
    return -_metric_dots(u, v)[0]


def metricCosine(u, v):
    """1 - inner u v / (sqrt (inner u u) * sqrt (inner v v)): the cosine distance of the device's
    RPT_KNN_METRIC_COSINE, every dot a left fold in Double; NaN when u or v is zero.
    Two SVectors: every dot as metricInner's (NaN for an empty or all-zero vector)."""
    uv, uu, vv = _metric_dots(u, v)
    den = np.float64(math.sqrt(uu)) * np.float64(math.sqrt(vv))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return float(1.0 - np.float64(uv) / den)


_METRIC_FLAGS = {metricL2: 0, metricCosine: RPT_KNN_METRIC_COSINE, metricInner: RPT_KNN_METRIC_INNER}


def _metric_flag(metric):
    """None / metricL2 / metricCosine / metricInner -> the knn flag bits of the device metric."""
    if metric is None:
        return 0
    try:
        return _METRIC_FLAGS[metric]
    except (KeyError, TypeError):
        raise NotImplementedError(
            "the device evaluates metricL2, metricCosine and metricInner only") from None


# ---------------------------------------------------------------------------------------
# queries
# ---------------------------------------------------------------------------------------
def candidates(tree, q):
    """RPTree.hs:289-314: ids of the leaf buckets reached by q in this tree, left to right."""
    f = tree.forest
    off, ids = candidatesBatch(f, q)
    t = tree.t
    return ids[off[t]:off[t + 1]]


def candidatesBatch(forest, qs):
    """-> (off[nq*T+1], ids): candidates of (query i, tree t) = ids[off[i*T+t]:off[i*T+t+1]]"""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    total = C.c_int64()
    off = np.empty(nq * forest.T + 1, dtype=np.int64)
    check(lib().rpt_candidates(ctx._h, forest._h, qd._h, _vp(off), None, 0, C.byref(total)))
    ids = np.empty(max(total.value, 1), dtype=np.int32)
    check(lib().rpt_candidates(ctx._h, forest._h, qd._h, _vp(off), _vp(ids), total.value,
                               C.byref(total)))
    return off, ids[:total.value]


def knnBatch(k, forest, qs, dedup=False, vote=0, reference_metric=False, metric=None):
    """knn for a batch of queries -> (ids[nq][k], dist[nq][k], count[nq]).
    dedup: False = the reference's knn (duplicates kept), True = each id once,
    RPT_KNN_DEDUP_DISTANCE = knnPQ's `nub` (one entry per distance).
    vote = v > 0: only points found by at least v trees are ranked (RPT_KNN_VOTE; the
    reference's commented-out counts / keepCounts, RPTree.hs:464-478), ties by ascending id.
    reference_metric: SVector data are ranked by the reference's own metricSSL2 (Internal.hs:
    389-393: the merge of the index lists stops at the shorter vector's end) instead of the true
    Euclidean distance.
    metric: None / metricL2, metricCosine or metricInner (RPT_KNN_METRIC_COSINE / _INNER: every
    value in f64, bit-exact to those host functions).  On SVector data the two are evaluated over
    the indices both vectors store (rpt_knn_csr_metric_host; see metricInner): the answer of the
    dense-ified data when the stored values are finite; not with reference_metric (ValueError)."""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    cnt = np.empty(nq, dtype=np.int32)
    flags = (RPT_KNN_DEDUP_DISTANCE if dedup == RPT_KNN_DEDUP_DISTANCE
             else RPT_KNN_DEDUP if dedup else RPT_KNN_KEEP_DUPLICATES)
    flags |= int(vote) << 8                       # RPT_KNN_VOTE(v)
    if reference_metric:                          # SVector data: the truncating metricSSL2
        flags |= RPT_KNN_METRIC_REFERENCE
    mflag = _metric_flag(metric)
    if mflag and reference_metric and forest.data.is_csr:
        raise ValueError("reference_metric is an L2 metric: not with metricCosine / metricInner")
    flags |= mflag
    # SVector data under metricCosine / metricInner: the entry point of their own (the distance over
    # the indices both vectors store, see metricInner); vote stays an error there
    entry = lib().rpt_knn_csr_metric_host if mflag and forest.data.is_csr else lib().rpt_knn_host
    check(entry(ctx._h, forest._h, forest.data._h, qd._h, int(k), flags, _vp(ids), _vp(dist), _vp(cnt)))
    return ids, dist, cnt


def _vote_flags(forest, metric, reference_metric):
    mflag = _metric_flag(metric)
    if mflag and reference_metric:
        raise ValueError("reference_metric is an L2 metric: not with metricCosine / metricInner")
    if reference_metric and not forest.data.is_csr:
        raise ValueError("reference_metric is the SVector rows' metric")
    return mflag | (RPT_KNN_METRIC_REFERENCE if reference_metric else 0)


def knnVote(k, forest, qs, v, metric=None, reference_metric=False):
    """Vote-threshold knn for a batch of queries -> (ids[nq][k], dist[nq][k], count[nq])
    (rpt_knn_vote_host): only the ids that at least v trees propose are ranked, each once, by
    (distance, id).  Every row layout (dense f64 / f32 / bf16, SVector f64 / f32), every distance
    (metric: None / metricL2, metricCosine, metricInner; reference_metric: SVector rows by the
    reference's truncating metricSSL2), batch and streamed forests, any number of trees and of
    candidates, k up to 1024.  The distances are those of knnBatch for the same data and metric.
    qs: as knnBatch's (arrays, SVectors, a CSR tuple, a Dataset)."""
    ctx = forest.ctx
    flags = _vote_flags(forest, metric, reference_metric)
    qd, nq = _query_dataset(ctx, forest.data, qs)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    cnt = np.empty(nq, dtype=np.int32)
    check(lib().rpt_knn_vote_host(ctx._h, forest._h, forest.data._h, qd._h, int(k), int(v), flags,
                                  _vp(ids), _vp(dist), _vp(cnt)))
    return ids, dist, cnt


def knnVoteDev(k, forest, queries, v, ids_ptr, dist_ptr, count_ptr, metric=None, reference_metric=False):
    """knnVote on device arrays (rpt_knn_vote_dev): queries is a Dataset, the outputs (int32 [nq][k],
    float64 [nq][k], int32 [nq]) device addresses.  Returns synchronised; whatever filled the
    queries must have finished (see Dataset.dense_device)."""
    ctx = forest.ctx
    flags = _vote_flags(forest, metric, reference_metric)
    check(lib().rpt_knn_vote_dev(ctx._h, forest._h, forest.data._h, queries._h, int(k), int(v), flags,
                                 C.c_void_p(ids_ptr), C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def voteCandidates(forest, qs, v):
    """-> (off[nq+1], ids, counts): the voted list of query i = ids[off[i]:off[i+1]], the ids that at
    least v trees propose, ascending, each once; counts: the number of trees that propose each (the
    reference's commented-out counts / keepCounts, RPTree.hs:464-478; rpt_vote_candidates_host)."""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    total = C.c_int64()
    off = np.empty(nq + 1, dtype=np.int64)
    check(lib().rpt_vote_candidates_host(ctx._h, forest._h, qd._h, int(v), _vp(off), None, None, 0,
                                         C.byref(total)))
    ids = np.empty(max(total.value, 1), dtype=np.int32)
    counts = np.empty(max(total.value, 1), dtype=np.int32)
    check(lib().rpt_vote_candidates_host(ctx._h, forest._h, qd._h, int(v), _vp(off), _vp(ids), _vp(counts),
                                         total.value, C.byref(total)))
    return off, ids[:total.value], counts[:total.value]


def knnVoteLast(ctx=None):
    """(candidates, voted, uncertified) of the last knnVote / knnVoteDev call: the candidate entries
    of all trees, the voted ids (= distances evaluated), the queries answered again by an exact
    kernel."""
    ctx = ctx or default_context()
    c, v, u = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().rpt_knn_last_candidates(ctx._h, C.byref(c)))
    check(lib().rpt_knn_last_voted(ctx._h, C.byref(v)))
    check(lib().rpt_knn_last_uncertified(ctx._h, C.byref(u)))
    return int(c.value), int(v.value), int(u.value)


def _allow_words(allow, n):
    """allow as graphSearchAllow takes it -> (the uint32 words or None, their address or None)"""
    if allow is None:
        return None, None
    words = allowBitmap(allow, n)
    return words, _vp(words)


def _allow_group_args(allow, group, n, nq):
    """(allow, group) of a grouped call (graphSearchAllowGroup, knnAllowGroup, ...) -> (words[G][ceil(n / 32)], their address or None, G, group as
    int32[nq], its address).  allow: what allowBitmaps takes, or its result; None or empty = no bitmap
    (G = 0: every group entry must be -1).  group None is the C ABI's null group: every query unfiltered."""
    g = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    if g is not None and g.shape != (nq,):
        raise ValueError("group must hold one int per query (nq = %d)" % nq)
    words = allowBitmaps([] if allow is None else allow, n)
    G = int(words.shape[0])
    return words, (_vp(words) if G else None), G, g, _vp(g)


def _dedup_flag(dedup):
    return (RPT_KNN_DEDUP_DISTANCE if dedup == RPT_KNN_DEDUP_DISTANCE
            else RPT_KNN_DEDUP if dedup else RPT_KNN_KEEP_DUPLICATES)


def knnAllow(allow, k, forest, qs, dedup=False, metric=None, reference_metric=False):
    """knnBatch among SOME of the points (rpt_knn_allow_host) -> (ids[nq][k], dist[nq][k], count[nq]).
    allow: a bool array of n (True = allowed), the uint32 words of allowBitmap, or None (every id);
    one list serves the batch.  A query's candidate list loses its disallowed entries, order and
    duplicates kept, and is then ranked as knnBatch ranks: by (distance, position) under the duplicate
    rule (dedup as knnBatch's), which therefore sees allowed entries only; count = min(k, entries
    left), unused slots are id -1 and distance +inf.  Every row layout (dense f64 / f32 / bf16,
    SVector f64 / f32), every distance (metric: None / metricL2, metricCosine, metricInner;
    reference_metric: SVector rows by the reference's truncating metricSSL2), batch and streamed
    forests, k up to 1024.  With every id allowed the answer is knnBatch's bit for bit.  The seeds of
    graphSearchAllow under the same list: knnAllow(allow, seed_k, forest, qs, dedup=True, metric=metric)[0]
    (unused slots are -1 already).  A bitmap per tenant or per query: knnAllowGroup."""
    ctx = forest.ctx
    flags = _dedup_flag(dedup) | _vote_flags(forest, metric, reference_metric)
    qd, nq = _query_dataset(ctx, forest.data, qs)
    words, wp = _allow_words(allow, forest.data.n)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    cnt = np.empty(nq, dtype=np.int32)
    check(lib().rpt_knn_allow_host(ctx._h, forest._h, forest.data._h, qd._h, wp, int(k), flags, _vp(ids),
                                   _vp(dist), _vp(cnt)))
    return ids, dist, cnt


def knnAllowGroup(allow, group, k, forest, qs, dedup=False, metric=None, reference_metric=False):
    """knnAllow with a bitmap per query group (rpt_knn_allow_group_host) -> (ids[nq][k], dist[nq][k],
    count[nq]).  allow: what allowBitmaps takes, or its result (G bitmaps); group: int[nq], query q is
    answered under bitmap group[q], -1 = every id.  The answer of query q is what knnAllow(allow[group[q]],
    ...) gives it, bit for bit; knnAllowLast's numbers are the sums over the queries."""
    ctx = forest.ctx
    flags = _dedup_flag(dedup) | _vote_flags(forest, metric, reference_metric)
    qd, nq = _query_dataset(ctx, forest.data, qs)
    words, wp, G, g, gp = _allow_group_args(allow, group, forest.data.n, nq)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    cnt = np.empty(nq, dtype=np.int32)
    check(lib().rpt_knn_allow_group_host(ctx._h, forest._h, forest.data._h, qd._h, wp, G, gp, int(k), flags,
                                         _vp(ids), _vp(dist), _vp(cnt)))
    return ids, dist, cnt


def knnAllowGroupDev(allow_ptr, G, group_ptr, k, forest, queries, ids_ptr, dist_ptr, count_ptr, dedup=False,
                     metric=None, reference_metric=False):
    """knnAllowGroup on device arrays (rpt_knn_allow_group_dev): allow_ptr is the device address of
    G rows of ceil(n / 32) uint32 words, group_ptr that of nq int32 (0 = every query unfiltered); the
    rest as knnAllowDev.  Nothing is validated: a group value outside [-1, G) means no id is allowed."""
    ctx = forest.ctx
    flags = _dedup_flag(dedup) | _vote_flags(forest, metric, reference_metric)
    check(lib().rpt_knn_allow_group_dev(ctx._h, forest._h, forest.data._h, queries._h, C.c_void_p(allow_ptr),
                                        int(G), C.c_void_p(group_ptr), int(k), flags, C.c_void_p(ids_ptr),
                                        C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def knnAllowDev(allow_ptr, k, forest, queries, ids_ptr, dist_ptr, count_ptr, dedup=False, metric=None,
                reference_metric=False):
    """knnAllow on device arrays (rpt_knn_allow_dev): allow_ptr is the device address of the
    ceil(n / 32) uint32 words (0 = every id), queries a Dataset, the outputs (int32 [nq][k], float64
    [nq][k], int32 [nq]) device addresses.  Returns synchronised; whatever filled the queries and the
    words must have finished (see Dataset.dense_device)."""
    ctx = forest.ctx
    flags = _dedup_flag(dedup) | _vote_flags(forest, metric, reference_metric)
    check(lib().rpt_knn_allow_dev(ctx._h, forest._h, forest.data._h, queries._h, C.c_void_p(allow_ptr), int(k),
                                  flags, C.c_void_p(ids_ptr), C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def allowCandidates(allow, forest, qs):
    """-> (off[nq+1], ids): the allowed list of query i = ids[off[i]:off[i+1]], its candidates of all
    trees (trees ascending, leaves left to right, duplicates kept) without the entries whose id the
    allow-list excludes (rpt_allow_candidates_host)."""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    words, wp = _allow_words(allow, forest.data.n)
    total = C.c_int64()
    off = np.empty(nq + 1, dtype=np.int64)
    check(lib().rpt_allow_candidates_host(ctx._h, forest._h, qd._h, wp, _vp(off), None, 0, C.byref(total)))
    ids = np.empty(max(total.value, 1), dtype=np.int32)
    check(lib().rpt_allow_candidates_host(ctx._h, forest._h, qd._h, wp, _vp(off), _vp(ids), total.value,
                                          C.byref(total)))
    return off, ids[:total.value]


def allowGroupCandidates(allow, group, forest, qs):
    """allowCandidates with every query under its own bitmap (rpt_allow_group_candidates_host; allow and
    group as knnAllowGroup's) -> (off[nq+1], ids)."""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    words, wp, G, g, gp = _allow_group_args(allow, group, forest.data.n, nq)
    total = C.c_int64()
    off = np.empty(nq + 1, dtype=np.int64)
    check(lib().rpt_allow_group_candidates_host(ctx._h, forest._h, qd._h, wp, G, gp, _vp(off), None, 0,
                                                C.byref(total)))
    ids = np.empty(max(total.value, 1), dtype=np.int32)
    check(lib().rpt_allow_group_candidates_host(ctx._h, forest._h, qd._h, wp, G, gp, _vp(off), _vp(ids), total.value,
                                                C.byref(total)))
    return off, ids[:total.value]


def knnAllowLast(ctx=None):
    """(candidates, allowed, uncertified) of the last knnAllow / knnAllowDev / allowCandidates call:
    the candidate entries of all trees, the allowed ones among them (= distances evaluated), the
    queries answered again by an exact kernel."""
    ctx = ctx or default_context()
    c, a, u = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().rpt_knn_allow_last(ctx._h, C.byref(c), C.byref(a)))
    check(lib().rpt_knn_last_uncertified(ctx._h, C.byref(u)))
    return int(c.value), int(a.value), int(u.value)


def _graph_flag(accumulate):
    return RPT_GRAPH_ACCUMULATE if accumulate else 0


def _knn_graph(entry, k, forest, accumulate, metric_flag=None):
    """knnGraph / knnGraphMetric / knnGraphSV / knnGraphMetricSV around their _host entry point;
    metric_flag None: the entry point takes no metric word"""
    ctx, n = forest.ctx, forest.N
    if accumulate is None:
        ids = np.empty((n, k), dtype=np.int32)
        dist = np.empty((n, k), dtype=np.float64)
        cnt = np.empty(n, dtype=np.int32)
    else:                                         # copies: the caller's arrays are not modified
        ids = np.array(accumulate[0], dtype=np.int32, order="C")
        dist = np.array(accumulate[1], dtype=np.float64, order="C")
        cnt = np.array(accumulate[2], dtype=np.int32, order="C")
        if ids.shape != (n, k) or dist.shape != (n, k) or cnt.shape != (n,):
            raise ValueError("accumulate must be (ids[n][k], dist[n][k], count[n]) of this forest's n and k")
    metric = () if metric_flag is None else (metric_flag,)
    check(entry(ctx._h, forest._h, forest.data._h, int(k), *metric, _graph_flag(accumulate is not None),
                _vp(ids), _vp(dist), _vp(cnt)))
    return ids, dist, cnt


def knnGraph(k, forest, accumulate=None):
    """kNN graph of the forest's own points (rpt_knn_graph_host): knn (RPTree.hs:174-176) with every
    stored point as the query, built leaf by leaf -> (ids[n][k], dist[n][k], count[n]).  Row i holds
    the first k, by (distance, id), of the points j != i that share a leaf with i in some tree;
    the distances are metricDDL2's left fold (Internal.hs:403-406) in double for every dtype;
    unused slots are id -1, distance +inf.  accumulate: an earlier (ids, dist, count) over the
    same data set and k (another forest, a tree shard) whose entries join the candidates; the
    result does not depend on the order forests are folded in.  Dense batch forests, k <= 64."""
    return _knn_graph(lib().rpt_knn_graph_host, k, forest, accumulate)


def knnGraphDev(k, forest, ids_ptr, dist_ptr, count_ptr, accumulate=False):
    """knnGraph into device arrays (rpt_knn_graph_dev): int32 [n][k], float64 [n][k], int32 [n]
    given as device addresses (e.g. torch tensors' data_ptr()).  Enqueued on the ctx stream, not
    synchronised (forest.ctx.sync() before reading); with accumulate the arrays are an input too
    and whatever filled them must have finished (see Dataset.dense_device)."""
    check(lib().rpt_knn_graph_dev(forest.ctx._h, forest._h, forest.data._h, int(k),
                                  _graph_flag(accumulate), C.c_void_p(ids_ptr),
                                  C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def knnGraphMetric(distf, k, forest, accumulate=None):
    """knnGraph under another distance (rpt_knn_graph_metric_host).  distf: None / metricL2 (the same
    bits as knnGraph), metricCosine or metricInner; the distances are those host functions bit for
    bit (the left-fold dot in double for every dtype), a zero row is NaN under metricCosine and
    ranks last.  accumulate: an earlier answer UNDER THE SAME distf (another is not detected: the
    stored distances are taken as stored).  Everything else as knnGraph.  Dense data only: SVector
    (CSR) rows are refused, knnGraphMetricSV takes them."""
    return _knn_graph(lib().rpt_knn_graph_metric_host, k, forest, accumulate, _metric_flag(distf))


def knnGraphMetricDev(distf, k, forest, ids_ptr, dist_ptr, count_ptr, accumulate=False):
    """knnGraphMetric into device arrays (rpt_knn_graph_metric_dev); the arrays and the
    synchronisation as knnGraphDev's."""
    metric = _metric_flag(distf)
    check(lib().rpt_knn_graph_metric_dev(forest.ctx._h, forest._h, forest.data._h, int(k),
                                         metric, _graph_flag(accumulate),
                                         C.c_void_p(ids_ptr), C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def knnGraphSV(k, forest, accumulate=None):
    """knnGraph of a forest over SVector (CSR) rows (rpt_knn_graph_csr_host) -> (ids[n][k],
    dist[n][k], count[n]).  The distances are metricDDL2's left fold over the dense-ified rows
    (absent columns +0.0, f32 values widened exactly), so the answer is bit-equal to knnGraph on
    the dense-ified data set with the same forest; the kernels visit only the 32-column windows in
    which a leaf holds a nonzero.  Rows must have strictly ascending columns.  accumulate as
    knnGraph's.  Batch forests over CSR data (f64 or f32 values), L2 only, k <= 64."""
    return _knn_graph(lib().rpt_knn_graph_csr_host, k, forest, accumulate)


def knnGraphSVDev(k, forest, ids_ptr, dist_ptr, count_ptr, accumulate=False):
    """knnGraphSV into device arrays (rpt_knn_graph_csr_dev); the arrays and the synchronisation
    as knnGraphDev's."""
    check(lib().rpt_knn_graph_csr_dev(forest.ctx._h, forest._h, forest.data._h, int(k),
                                      _graph_flag(accumulate), C.c_void_p(ids_ptr),
                                      C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def knnGraphMetricSV(distf, k, forest, accumulate=None):
    """knnGraphSV under another distance (rpt_knn_graph_csr_metric_host).  distf: None / metricL2
    (the same bits as knnGraphSV), metricCosine or metricInner, evaluated over the indices both rows
    store (see metricInner; the definition knnBatch uses on SVector data): the left fold of the
    products of the shared columns from +0.0, in double.  While every stored value is finite that
    is knnGraphMetric on the dense-ified rows bit for bit; with a stored inf or NaN it is not (the
    dense fold meets inf * 0), and the answer is this definition either way.  An empty or all-zero
    row is NaN under metricCosine and ranks last, by id; two rows that share no index are at
    metricInner distance -0.0, which ties with +0.0.  accumulate: an earlier answer UNDER THE SAME
    distf.  Everything else as knnGraphSV.  (knnGraphMetric itself takes dense data only.)"""
    return _knn_graph(lib().rpt_knn_graph_csr_metric_host, k, forest, accumulate, _metric_flag(distf))


def knnGraphMetricSVDev(distf, k, forest, ids_ptr, dist_ptr, count_ptr, accumulate=False):
    """knnGraphMetricSV into device arrays (rpt_knn_graph_csr_metric_dev); the arrays and the
    synchronisation as knnGraphDev's."""
    metric = _metric_flag(distf)
    check(lib().rpt_knn_graph_csr_metric_dev(forest.ctx._h, forest._h, forest.data._h, int(k),
                                             metric, _graph_flag(accumulate),
                                             C.c_void_p(ids_ptr), C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def knnGraphLastPairs(ctx=None):
    """distances the last knnGraph call on ctx evaluated (rpt_knn_graph_last_pairs)"""
    ctx = ctx or default_context()
    v = C.c_int64()
    check(lib().rpt_knn_graph_last_pairs(ctx._h, C.byref(v)))
    return int(v.value)


def _refine_data(data):
    return data if isinstance(data, Dataset) else data.data


def _knn_graph_refine(entry, graph, data, iters, reverse, ctx, metric_flag=None):
    """knnGraphRefine / -SV / -Metric / -MetricSV around their _host entry point; metric_flag None:
    the entry point takes no metric word"""
    ds = _refine_data(data)
    ctx = ctx or ds.ctx
    ids = np.array(graph[0], dtype=np.int32, order="C")       # copies: refined in place, returned
    dist = np.array(graph[1], dtype=np.float64, order="C")
    cnt = np.array(graph[2], dtype=np.int32, order="C")
    if ids.ndim != 2 or ids.shape[0] != ds.n or dist.shape != ids.shape or cnt.shape != (ds.n,):
        raise ValueError("graph must be (ids[n][k], dist[n][k], count[n]) over the data set's n rows")
    k = ids.shape[1]
    metric = () if metric_flag is None else (metric_flag,)
    check(entry(ctx._h, ds._h, int(k), int(k if reverse is None else reverse), int(iters), *metric, 0,
                _vp(ids), _vp(dist), _vp(cnt)))
    return ids, dist, cnt

def knnGraphRefine(graph, data, iters=1, reverse=None, ctx=None):
    """NN-descent rounds over a kNN graph (rpt_knn_graph_refine_host) -> new (ids, dist, count); the
    input tuple is not modified.  graph: (ids[n][k], dist[n][k], count[n]) over `data`, e.g.
    knnGraph's; data: a dense Dataset, or a forest (its .data is used; no forest takes part).
    One round gives row i the first k, by (distance, id), of its neighbours, up to `reverse` of
    the points that list i (None = k, 0 = none; the nearest by (distance, id)) and all of THEIR
    neighbours; distances not already in row i are metricDDL2's left fold in double, bit-exact for
    every dtype.  A round that changes nothing ends the sequence.  Deterministic: the same input
    gives the same bits.  k and reverse <= 64."""
    return _knn_graph_refine(lib().rpt_knn_graph_refine_host, graph, data, iters, reverse, ctx)


def knnGraphRefineDev(k, data, ids_ptr, dist_ptr, count_ptr, iters=1, reverse=None):
    """knnGraphRefine on device arrays in place (rpt_knn_graph_refine_dev): int32 [n][k], float64
    [n][k], int32 [n] given as device addresses.  The arrays are NOT validated.  All `iters` rounds
    are enqueued on the ctx stream, not synchronised (ctx.sync() before reading); whatever filled
    the arrays must have finished (see Dataset.dense_device)."""
    ds = _refine_data(data)
    check(lib().rpt_knn_graph_refine_dev(ds.ctx._h, ds._h, int(k), int(k if reverse is None else reverse),
                                         int(iters), 0, C.c_void_p(ids_ptr), C.c_void_p(dist_ptr),
                                         C.c_void_p(count_ptr)))


def knnGraphRefineSV(graph, data, iters=1, reverse=None, ctx=None):
    """knnGraphRefine over SVector (CSR) rows (rpt_knn_graph_refine_csr_host) -> new (ids, dist,
    count).  data: a CSR Dataset, or a forest over one.  The distances are metricDDL2's left fold
    over the dense-ified rows, so the answer (and knnGraphRefineLast's numbers) is bit-equal to
    knnGraphRefine on the dense-ified data set.  Everything else as knnGraphRefine."""
    return _knn_graph_refine(lib().rpt_knn_graph_refine_csr_host, graph, data, iters, reverse, ctx)


def knnGraphRefineSVDev(k, data, ids_ptr, dist_ptr, count_ptr, iters=1, reverse=None):
    """knnGraphRefineSV on device arrays in place (rpt_knn_graph_refine_csr_dev); the arrays and
    the synchronisation as knnGraphRefineDev's."""
    ds = _refine_data(data)
    check(lib().rpt_knn_graph_refine_csr_dev(ds.ctx._h, ds._h, int(k), int(k if reverse is None else reverse),
                                             int(iters), 0, C.c_void_p(ids_ptr), C.c_void_p(dist_ptr),
                                             C.c_void_p(count_ptr)))


def knnGraphRefineMetric(distf, graph, data, iters=1, reverse=None, ctx=None):
    """knnGraphRefine under another distance (rpt_knn_graph_refine_metric_host).  distf: None /
    metricL2 (the same bits as knnGraphRefine), metricCosine or metricInner; distances not already
    in row i are those host functions bit for bit.  The graph's stored distances must be distf's
    (knnGraphMetric's under the same distf; another metric is not detected).  Everything else as
    knnGraphRefine.  Dense data only: SVector (CSR) rows are refused, knnGraphRefineMetricSV takes
    them."""
    return _knn_graph_refine(lib().rpt_knn_graph_refine_metric_host, graph, data, iters, reverse, ctx,
                             _metric_flag(distf))


def knnGraphRefineMetricDev(distf, k, data, ids_ptr, dist_ptr, count_ptr, iters=1, reverse=None):
    """knnGraphRefineMetric on device arrays in place (rpt_knn_graph_refine_metric_dev); the arrays
    and the synchronisation as knnGraphRefineDev's."""
    metric = _metric_flag(distf)
    ds = _refine_data(data)
    check(lib().rpt_knn_graph_refine_metric_dev(ds.ctx._h, ds._h, int(k), int(k if reverse is None else reverse),
                                                int(iters), metric, 0, C.c_void_p(ids_ptr),
                                                C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def knnGraphRefineMetricSV(distf, graph, data, iters=1, reverse=None, ctx=None):
    """knnGraphRefineSV under another distance (rpt_knn_graph_refine_csr_metric_host).  distf: None /
    metricL2 (the same bits as knnGraphRefineSV), metricCosine or metricInner over the indices both
    rows store, as knnGraphMetricSV defines them.  The graph's stored distances must be distf's
    (knnGraphMetricSV's under the same distf; another metric is not detected).  Everything else as
    knnGraphRefineSV.  (knnGraphRefineMetric itself takes dense data only.)"""
    return _knn_graph_refine(lib().rpt_knn_graph_refine_csr_metric_host, graph, data, iters, reverse, ctx,
                             _metric_flag(distf))


def knnGraphRefineMetricSVDev(distf, k, data, ids_ptr, dist_ptr, count_ptr, iters=1, reverse=None):
    """knnGraphRefineMetricSV on device arrays in place (rpt_knn_graph_refine_csr_metric_dev); the
    arrays and the synchronisation as knnGraphRefineDev's."""
    metric = _metric_flag(distf)
    ds = _refine_data(data)
    check(lib().rpt_knn_graph_refine_csr_metric_dev(ds.ctx._h, ds._h, int(k), int(k if reverse is None else reverse),
                                                    int(iters), metric, 0, C.c_void_p(ids_ptr),
                                                    C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def knnGraphRefineLast(ctx=None):
    """(rounds, updates, candidates) of the last knnGraphRefine call on ctx
    (rpt_knn_graph_refine_last; synchronises): rounds applied up to and including the first that
    changed nothing, ids that entered a row, distances evaluated."""
    ctx = ctx or default_context()
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().rpt_knn_graph_refine_last(ctx._h, C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def _graph_search(entry, who, graph, data, qs, k, ef, seeds, forest, seed_k, metric_flag, seed_metric, ctx,
                  allow=None, width=None, filtered=False, group=None, grouped=False):
    """graphSearch / graphSearchSV / graphSearchMetricSV / graphSearchAllow around their _host entry
    point; seed_metric: the metric of the knnBatch that takes seeds from `forest`; filtered: the entry
    point takes the allow-list's words behind the seeds and `width` behind ef"""
    ds = _refine_data(data)
    ctx = ctx or ds.ctx
    gids = np.ascontiguousarray(graph[0], dtype=np.int32)
    gcnt = np.ascontiguousarray(graph[-1], dtype=np.int32)
    if gids.ndim != 2 or gids.shape[0] != ds.n or gcnt.shape != (ds.n,):
        raise ValueError("graph must be (ids[n][kg], dist[n][kg], count[n]) over the data set's n rows")
    if ef is None:
        ef = max(int(k), 32)
    if seeds is None and forest is None:
        raise ValueError(who + " needs seeds or a forest to take them from")
    qd, nq = _query_dataset(ctx, ds, qs)
    if seeds is None:
        sid, _, scnt = knnBatch(int(seed_k), forest, qd, dedup=True, metric=seed_metric)
        seeds = np.where(np.arange(sid.shape[1])[None, :] < scnt[:, None], sid, -1)
    seeds = np.ascontiguousarray(seeds, dtype=np.int32)
    if seeds.ndim != 2 or seeds.shape[0] != nq:
        raise ValueError("seeds must be [nq][s]")
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    cnt = np.empty(nq, dtype=np.int32)
    head = (ctx._h, ds._h, qd._h, int(gids.shape[1]), _vp(gids), _vp(gcnt), int(seeds.shape[1]), _vp(seeds))
    beam = (int(k), int(ef))
    if filtered and grouped:  # the entry point takes (allow, G, group) where allow stands
        words, wp, G, g, gp = _allow_group_args(allow, group, ds.n, nq)
        head += (wp, G, gp)
    elif filtered:
        words = None if allow is None else allowBitmap(allow, ds.n)
        head += (None if words is None else _vp(words),)
    if filtered:
        beam += (min(RPT_GRAPH_SEARCH_MAX_WIDTH, 8 * int(ef)) if width is None else int(width),)
    check(entry(*head, *beam, metric_flag, 0, _vp(ids), _vp(dist), _vp(cnt)))
    return ids, dist, cnt


def graphSearch(graph, data, qs, k, ef=None, seeds=None, forest=None, seed_k=8, metric=None, ctx=None):
    """Best-first beam search over a kNN graph (rpt_graph_search_host) -> (ids[nq][k], dist[nq][k],
    count[nq]).  graph: (ids[n][kg], dist[n][kg], count[n]) over `data`, e.g. knnGraph's or
    knnGraphRefine's (the distances are not read; a pair (ids, count) will do); data: a dense Dataset,
    or a forest (its .data is used).  The beam holds ef entries (None = max(k, 32), at most 256); the
    search starts from seeds[nq][s] (s <= 64, -1 = unused slot) or, with `forest`, from the ids of
    knnBatch(seed_k, forest, qs, dedup=True, metric=metric), and repeatedly offers the graph row of
    the beam's first unexpanded entry until none is left.  The answer is the first k of the beam
    by (distance, id); metric: None / metricL2, metricCosine or metricInner, the distances those
    host functions bit for bit (L2: on f64 rows).  Unused slots are id -1, distance +inf.  SVector
    (CSR) data is refused here: graphSearchSV (L2), graphSearchMetricSV (any of the three)."""
    return _graph_search(lib().rpt_graph_search_host, "graphSearch", graph, data, qs, k, ef, seeds, forest,
                         seed_k, _metric_flag(metric), metric, ctx)


def graphSearchDev(data, queries, kg, gids_ptr, gcount_ptr, s, seeds_ptr, k, ef, ids_ptr, dist_ptr, count_ptr,
                   metric=None):
    """graphSearch on device arrays (rpt_graph_search_dev): data and queries are Datasets, the graph
    (int32 [n][kg], int32 [n]), the seeds (int32 [nq][s]) and the outputs (int32 [nq][k], float64
    [nq][k], int32 [nq]) device addresses.  The arrays are NOT validated: entries out of range are
    skipped.  Enqueued on the ctx stream, not synchronised (ctx.sync() before reading); whatever
    filled the arrays must have finished (see Dataset.dense_device)."""
    metric_flag = _metric_flag(metric)
    ds = _refine_data(data)
    check(lib().rpt_graph_search_dev(ds.ctx._h, ds._h, queries._h, int(kg), C.c_void_p(gids_ptr),
                                     C.c_void_p(gcount_ptr), int(s), C.c_void_p(seeds_ptr), int(k), int(ef),
                                     metric_flag, 0, C.c_void_p(ids_ptr), C.c_void_p(dist_ptr),
                                     C.c_void_p(count_ptr)))


def graphSearchSV(graph, data, qs, k, ef=None, seeds=None, forest=None, seed_k=8, ctx=None):
    """graphSearch over SVector (CSR) rows under L2 (rpt_graph_search_csr_host) -> (ids[nq][k],
    dist[nq][k], count[nq]).  data: a CSR Dataset, or a forest over one; qs: SVectors, a CSR tuple
    (rowptr, col, val, d) or a CSR Dataset of the same d and dtype.  The distances are metricDDL2's
    left fold over the dense-ified query and row, so the answer (and graphSearchLast's numbers) is
    bit-equal to graphSearch on the dense-ified data set and queries with the same graph and seeds.
    With `forest` (a batch forest over the CSR set) the seeds are the ids of knnBatch(seed_k, forest,
    qs, dedup=True).  Everything else as graphSearch."""
    return _graph_search(lib().rpt_graph_search_csr_host, "graphSearchSV", graph, data, qs, k, ef, seeds,
                         forest, seed_k, 0, None, ctx)


def graphSearchSVDev(data, queries, kg, gids_ptr, gcount_ptr, s, seeds_ptr, k, ef, ids_ptr, dist_ptr, count_ptr):
    """graphSearchSV on device arrays (rpt_graph_search_csr_dev): data and queries are CSR Datasets;
    the arrays and the synchronisation as graphSearchDev's."""
    ds = _refine_data(data)
    check(lib().rpt_graph_search_csr_dev(ds.ctx._h, ds._h, queries._h, int(kg), C.c_void_p(gids_ptr),
                                         C.c_void_p(gcount_ptr), int(s), C.c_void_p(seeds_ptr), int(k), int(ef),
                                         0, 0, C.c_void_p(ids_ptr), C.c_void_p(dist_ptr),
                                         C.c_void_p(count_ptr)))


def graphSearchMetricSV(distf, graph, data, qs, k, ef=None, seeds=None, forest=None, seed_k=8, ctx=None):
    """graphSearchSV under another distance (rpt_graph_search_csr_metric_host) -> (ids[nq][k],
    dist[nq][k], count[nq]).  distf: None / metricL2 (the same bits as graphSearchSV), metricCosine or
    metricInner over the indices both the query and the row store, as knnGraphMetricSV defines them
    (those host functions on SVectors bit for bit); while every stored value is finite the answer is
    graphSearch(metric=distf) on the dense-ified data set and queries bit for bit.  An empty or
    all-zero query is NaN from everything under metricCosine: it still gets its answers, ordered by
    id.  graph: e.g. knnGraphMetricSV's, knnGraphRefineMetricSV's or graphPrepareMetricSV's under the
    same distf.  With `forest` the seeds are the ids of knnBatch(seed_k, forest, qs, dedup=True,
    metric=distf).  Everything else as graphSearchSV.  (graphSearch(metric=) itself takes dense data
    only.)"""
    return _graph_search(lib().rpt_graph_search_csr_metric_host, "graphSearchMetricSV", graph, data, qs, k, ef,
                         seeds, forest, seed_k, _metric_flag(distf), distf, ctx)


def graphSearchMetricSVDev(distf, data, queries, kg, gids_ptr, gcount_ptr, s, seeds_ptr, k, ef, ids_ptr, dist_ptr,
                           count_ptr):
    """graphSearchMetricSV on device arrays (rpt_graph_search_csr_metric_dev): data and queries are CSR
    Datasets; the arrays and the synchronisation as graphSearchDev's."""
    metric = _metric_flag(distf)
    ds = _refine_data(data)
    check(lib().rpt_graph_search_csr_metric_dev(ds.ctx._h, ds._h, queries._h, int(kg), C.c_void_p(gids_ptr),
                                                C.c_void_p(gcount_ptr), int(s), C.c_void_p(seeds_ptr), int(k),
                                                int(ef), metric, 0, C.c_void_p(ids_ptr), C.c_void_p(dist_ptr),
                                                C.c_void_p(count_ptr)))


def allowBitmaps(masks, n):
    """G allow-lists as uint32[G][ceil(n / 32)], row g being allowBitmap(masks[g], n): the bitmaps of a
    grouped call (graphSearchAllow / knnAllow / bruteKnnAllow / ... with group=).  masks: a sequence
    whose entries are each what allowBitmap takes (a bool mask of n, integer ids, or ceil(n / 32)
    uint32 words), or the result of this function (returned as it is).  The row stride is
    ceil(n / 32) words."""
    n = int(n)
    nw = (n + 31) // 32
    if isinstance(masks, np.ndarray) and masks.dtype == np.uint32 and masks.ndim == 2:
        if masks.shape[1] != nw:
            raise ValueError("every allow-list row must hold ceil(n / 32) = %d uint32" % nw)
        return np.ascontiguousarray(masks)
    out = np.zeros((len(masks), nw), dtype=np.uint32)
    for g, m in enumerate(masks):
        out[g] = allowBitmap(m, n)
    return out


def allowBitmap(mask_or_ids, n):
    """The allow-list of graphSearchAllow as ceil(n / 32) uint32 words: id i is allowed when bit i & 31
    of word i >> 5 is set.  mask_or_ids: a bool array of n (True = allowed), an integer array of the
    allowed ids (each in [0, n)), or the uint32 words themselves (returned as they are)."""
    n = int(n)
    nw = (n + 31) // 32
    a = np.asarray(mask_or_ids)
    if a.dtype == np.uint32:
        if a.shape != (nw,):
            raise ValueError("the allow-list's words must be ceil(n / 32) = %d uint32" % nw)
        return np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        if a.shape != (n,):
            raise ValueError("the allow mask must hold n = %d bools" % n)
        mask = a
    else:
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("allow must be a bool mask of n, integer ids or uint32 words")
        ids = a.astype(np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            raise ValueError("an allowed id lies outside [0, n)")
        mask = np.zeros(n, dtype=bool)
        mask[ids] = True
    bits = np.zeros(nw * 32, dtype=np.uint8)
    bits[:n] = mask
    return np.ascontiguousarray(np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32))


def graphSearchAllow(allow, graph, data, qs, k, ef=None, width=None, seeds=None, forest=None, seed_k=8, metric=None,
                     ctx=None):
    """graphSearch among SOME of the points (rpt_graph_search_allow_host) -> (ids[nq][k], dist[nq][k],
    count[nq]): the rows a tombstone bitmap has not deleted, the rows of one tenant.  allow: a bool
    array of n (True = allowed), the uint32 words of allowBitmap, or None (every id); one list serves
    the whole batch.  data: a dense or an SVector (CSR) Dataset, or a forest over one; qs as graphSearch
    / graphSearchSV take them; metric: None / metricL2, metricCosine or metricInner on either layout.
    ef (None = max(k, 32), at most 256) counts ALLOWED beam entries only; width (None = min(1024,
    8 * ef), in [ef, 1024]) is the most entries the beam may hold, allowed or not: the frontier the
    search walks through, disallowed entries being expanded like any other.  A beam with ef allowed
    entries ends at its ef-th allowed entry.  The answer is the first k allowed entries by (distance,
    id).  With every id allowed it is graphSearch's / graphSearchSV's / graphSearchMetricSV's bit for
    bit, whatever the width; with width = ef it is the allowed entries of the unfiltered beam.  With
    `forest` the seeds are the ids of knnBatch(seed_k, forest, qs, dedup=True, metric=metric); seeds
    need not be allowed.  A bitmap per tenant or per query: graphSearchAllowGroup."""
    return _graph_search(lib().rpt_graph_search_allow_host, "graphSearchAllow", graph, data, qs, k, ef, seeds,
                         forest, seed_k, _metric_flag(metric), metric, ctx, allow, width, True)


def graphSearchAllowGroup(allow, group, graph, data, qs, k, ef=None, width=None, seeds=None, forest=None, seed_k=8,
                          metric=None, ctx=None):
    """graphSearchAllow with a bitmap per query group (rpt_graph_search_allow_group_host) ->
    (ids[nq][k], dist[nq][k], count[nq]).  allow: what allowBitmaps takes, or its result (G bitmaps);
    group: int[nq], query q searches under bitmap group[q], -1 = every id (None: every query -1).  Many tenants in one batch, a
    bitmap per query (group = arange(nq)) or a mix with unfiltered queries.  The answer of query q is
    graphSearchAllow(allow[group[q]], ...)'s for that query, bit for bit, and graphSearchLast's
    expansions are the sum over the queries.  A group entry outside [-1, G) is refused."""
    return _graph_search(lib().rpt_graph_search_allow_group_host, "graphSearchAllowGroup", graph, data, qs, k, ef,
                         seeds, forest, seed_k, _metric_flag(metric), metric, ctx, allow, width, True, group, True)


def graphSearchAllowGroupDev(data, queries, kg, gids_ptr, gcount_ptr, s, seeds_ptr, allow_ptr, G, group_ptr, k, ef,
                             width, ids_ptr, dist_ptr, count_ptr, metric=None):
    """graphSearchAllowGroup on device arrays (rpt_graph_search_allow_group_dev): allow_ptr the
    device address of G rows of ceil(n / 32) uint32 words, group_ptr that of nq int32 (0 = every query
    unfiltered); the rest as graphSearchAllowDev.  Nothing is validated: a group value outside
    [-1, G) means no id is allowed (count 0)."""
    metric_flag = _metric_flag(metric)
    ds = _refine_data(data)
    check(lib().rpt_graph_search_allow_group_dev(ds.ctx._h, ds._h, queries._h, int(kg), C.c_void_p(gids_ptr),
                                                 C.c_void_p(gcount_ptr), int(s), C.c_void_p(seeds_ptr),
                                                 C.c_void_p(allow_ptr), int(G), C.c_void_p(group_ptr), int(k),
                                                 int(ef), int(width), metric_flag, 0, C.c_void_p(ids_ptr),
                                                 C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def graphSearchAllowDev(data, queries, kg, gids_ptr, gcount_ptr, s, seeds_ptr, allow_ptr, k, ef, width, ids_ptr,
                        dist_ptr, count_ptr, metric=None):
    """graphSearchAllow on device arrays (rpt_graph_search_allow_dev): data and queries are Datasets
    (both dense or both CSR), allow_ptr the device address of the ceil(n / 32) uint32 words (0 = every
    id); the other arrays and the synchronisation as graphSearchDev's."""
    metric_flag = _metric_flag(metric)
    ds = _refine_data(data)
    check(lib().rpt_graph_search_allow_dev(ds.ctx._h, ds._h, queries._h, int(kg), C.c_void_p(gids_ptr),
                                           C.c_void_p(gcount_ptr), int(s), C.c_void_p(seeds_ptr),
                                           C.c_void_p(allow_ptr), int(k), int(ef), int(width), metric_flag, 0,
                                           C.c_void_p(ids_ptr), C.c_void_p(dist_ptr), C.c_void_p(count_ptr)))


def graphSearchLast(ctx=None):
    """(expansions, evaluated) of the last graphSearch / graphSearchSV / graphSearchAllow call on ctx
    (rpt_graph_search_last; synchronises): beam entries expanded and distances computed, summed over
    the queries."""
    ctx = ctx or default_context()
    a, b = C.c_int64(), C.c_int64()
    check(lib().rpt_graph_search_last(ctx._h, C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def _insert_rows(data, n):
    """the new rows of graphInsert's `data` as knnBatch takes queries: the rows from n on"""
    if isinstance(data, Dataset):
        if data._host is None:
            raise ValueError("graphInsert takes seeds from a forest only when it is handed the rows themselves "
                             "(an array or a CSR tuple, or a Dataset made from float64 rows): pass seeds")
        return data._host[n:]
    if isinstance(data, tuple):
        rowptr = np.asarray(data[0], dtype=np.int64)
        lo, hi = int(rowptr[n]), int(rowptr[-1])
        return rowptr[n:] - lo, np.asarray(data[1])[lo:hi], np.asarray(data[2])[lo:hi], data[3]
    return np.asarray(data)[n:]


def graphInsert(graph, data, m, ef=None, batch=None, seeds=None, forest=None, seed_k=8, metric=None, ctx=None):
    """New rows into a kNN graph (rpt_graph_insert_host) -> (ids[N][kg], dist[N][kg], count[N]): the
    graph grows, nothing is rebuilt.  data: the data set of N = n + m rows whose LAST m rows are the new
    ones, as a 2-D array (float64, float32, or uint16 bf16 patterns), a CSR tuple (rowptr, col, val, d)
    or a dense or CSR Dataset; graph: (ids[n][kg], dist[n][kg], count[n]) over the first n rows
    (knnGraph's, knnGraphRefine's; the distances ARE read); metric: None / metricL2, metricCosine or
    metricInner, the one the graph was built under, on either layout.  The new rows are taken in
    chunks of `batch`.  Every row of a chunk is answered by graphSearch with k = kg and this ef (None
    = max(kg, 32)) over the rows visible so far: the first n and the chunks before it, not its own
    chunk.  The answer becomes the new row, and every row it names takes the new id at the same
    distance when that is among its first kg by (distance, id).  Rows of one chunk do not see each
    other (knnGraphRefine afterwards links them): a smaller batch links more, a larger one fills the
    device.  batch None = min(m, 4096): kept after the sweep of tools/graph_insert_times.py at 1 M x 128
    (74 / 25 / 19 / 14 ms at batch 1024 / 4096 / 16384 / m = 100 000: one chunk is the fastest, and its
    rows are linked to old rows only).  seeds[m][s] (s <= 64, -1 = unused; a seed may name a row of an earlier chunk)
    or, with `forest`, a forest over the OLD n rows, the ids of knnBatch(seed_k, forest, new rows,
    dedup=True, metric=metric).  The result is a pure function of its inputs, bit for bit; m = 0
    copies the graph."""
    metric_flag = _metric_flag(metric)
    ctx = ctx or (data.ctx if isinstance(data, Dataset) else default_context())
    if isinstance(data, np.ndarray) and data.dtype == np.uint16:
        ds = Dataset.dense(ctx, data, dtype=RPT_BF16)
    else:
        ds = Dataset.of(ctx, data)
    m = int(m)
    N, n = ds.n, ds.n - m
    gids = np.ascontiguousarray(graph[0], dtype=np.int32)
    gdist = np.ascontiguousarray(graph[1], dtype=np.float64)
    gcnt = np.ascontiguousarray(graph[2], dtype=np.int32)
    if m < 0 or n < 0 or gids.ndim != 2 or gids.shape[0] != n or gdist.shape != gids.shape or gcnt.shape != (n,):
        raise ValueError("graph must be (ids[n][kg], dist[n][kg], count[n]) over the first n = N - m rows of data")
    kg = int(gids.shape[1])
    if ef is None:
        ef = max(kg, 32)
    if batch is None:
        batch = max(1, min(m, 4096))
    if seeds is None:
        if forest is None:
            raise ValueError("graphInsert needs seeds or a forest over the old rows to take them from")
        if m:
            sid, _, scnt = knnBatch(int(seed_k), forest, _insert_rows(data, n), dedup=True, metric=metric)
            seeds = np.where(np.arange(sid.shape[1])[None, :] < scnt[:, None], sid, -1)
        else:
            seeds = np.zeros((0, int(seed_k)), dtype=np.int32)
    seeds = np.ascontiguousarray(seeds, dtype=np.int32)
    if seeds.ndim != 2 or seeds.shape[0] != m:
        raise ValueError("seeds must be [m][s]")
    ids = np.empty((N, kg), dtype=np.int32)
    dist = np.empty((N, kg), dtype=np.float64)
    cnt = np.empty(N, dtype=np.int32)
    check(lib().rpt_graph_insert_host(ctx._h, ds._h, kg, _vp(gids), _vp(gdist), _vp(gcnt), m, int(seeds.shape[1]),
                                      _vp(seeds), int(ef), int(batch), metric_flag, 0, _vp(ids), _vp(dist),
                                      _vp(cnt)))
    return ids, dist, cnt


def graphInsertDev(data, kg, gids_ptr, gdist_ptr, gcount_ptr, m, s, seeds_ptr, ef, batch, oids_ptr, odist_ptr,
                   ocount_ptr, metric=None):
    """graphInsert on device arrays (rpt_graph_insert_dev): data is the Dataset of N = n + m rows, the
    graph (int32 [n][kg], float64 [n][kg], int32 [n]), the seeds (int32 [m][s]) and the outputs (int32
    [N][kg], float64 [N][kg], int32 [N]) device addresses.  The input graph is read only and NOT
    validated: rows nothing links to are copied as they are, touched rows come out sorted without
    their invalid entries.  Enqueued on the ctx stream, not synchronised (ctx.sync() before reading);
    whatever filled the arrays must have finished (see Dataset.dense_device)."""
    metric_flag = _metric_flag(metric)
    ds = _refine_data(data)
    check(lib().rpt_graph_insert_dev(ds.ctx._h, ds._h, int(kg), C.c_void_p(gids_ptr), C.c_void_p(gdist_ptr),
                                     C.c_void_p(gcount_ptr), int(m), int(s), C.c_void_p(seeds_ptr), int(ef),
                                     int(batch), metric_flag, 0, C.c_void_p(oids_ptr), C.c_void_p(odist_ptr),
                                     C.c_void_p(ocount_ptr)))


def graphInsertLast(ctx=None):
    """(chunks, evaluated, offered, accepted) of the last graphInsert call on ctx (rpt_graph_insert_last;
    synchronises): chunks searched and linked, distances the searches computed, reverse entries offered
    to the rows the answers name, and those that were in their row when it was written."""
    ctx = ctx or default_context()
    a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().rpt_graph_insert_last(ctx._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return int(a.value), int(b.value), int(c.value), int(d.value)


def compactRows(data, keep):
    """The kept rows of a host data set, for graphDelete's compact form: data is a 2-D array or a CSR
    tuple (rowptr, col, val, d), keep a bool array of n (True = the row stays) or the uint32 words of
    allowBitmap.  Row newid[p] of the result is row p of data."""
    n = (len(data[0]) - 1) if isinstance(data, tuple) else len(data)
    k = np.asarray(keep)
    if k.dtype == np.uint32:
        k = np.unpackbits(allowBitmap(k, n).view(np.uint8), bitorder="little")[:n].astype(bool)
    if k.dtype != np.bool_ or k.shape != (n,):
        raise ValueError("keep must be a bool mask of n = %d or its uint32 words" % n)
    if not isinstance(data, tuple):
        return np.ascontiguousarray(np.asarray(data)[k])
    rowptr = np.asarray(data[0], dtype=np.int64)
    length = (rowptr[1:] - rowptr[:-1])[k]
    out = np.zeros(length.size + 1, dtype=np.int64)
    out[1:] = np.cumsum(length)
    take = np.repeat(k, rowptr[1:] - rowptr[:-1])
    return out, np.asarray(data[1])[take], np.asarray(data[2])[take], data[3]


def graphDelete(keep, graph, data, compact=True, metric=None, ctx=None):
    """Rows out of a kNN graph (rpt_graph_delete_host) -> ((ids, dist, count), newid): the deleted rows
    are dropped and every list that named one is repaired from the deleted row's own neighbours, one
    hop; nothing is rebuilt.  keep: a bool array of n (True = the row STAYS), the uint32 words of
    allowBitmap (the tombstone bitmap graphSearchAllow takes, unchanged) or None (every row stays).
    graph: (ids[n][kg], dist[n][kg], count[n]) over data's n rows (the distances ARE read); data: a 2-D
    array (float64, float32, or uint16 bf16 patterns), a CSR tuple (rowptr, col, val, d), a dense or CSR
    Dataset, or a forest over one; metric: None / metricL2, metricCosine or metricInner, the one the
    graph was built under.  A kept row that named no deleted row is copied; a row that did becomes the
    first kg by (distance, id) of its kept entries, at their stored distances, and the kept neighbours
    of its deleted neighbours, at their distance to the row.  compact=True: the survivors are
    renumbered densely, newid[i] = the number of kept rows below i or -1, the graph has popcount(keep)
    rows and belongs to compactRows(data, keep).  compact=False: n rows in old ids, deleted rows empty,
    newid[i] = i or -1; searchable with the unchanged data.  A row whose neighbours and all their
    neighbours are gone ends short: knnGraphRefine afterwards repairs it.  A pure function of its inputs,
    bit for bit."""
    metric_flag = _metric_flag(metric)
    if not isinstance(data, (Dataset, np.ndarray, tuple)) and hasattr(data, "data"):
        data = data.data                                  # a forest
    ctx = ctx or (data.ctx if isinstance(data, Dataset) else default_context())
    if isinstance(data, np.ndarray) and data.dtype == np.uint16:
        ds = Dataset.dense(ctx, data, dtype=RPT_BF16)
    else:
        ds = Dataset.of(ctx, data)
    n = ds.n
    gids = np.ascontiguousarray(graph[0], dtype=np.int32)
    gdist = np.ascontiguousarray(graph[1], dtype=np.float64)
    gcnt = np.ascontiguousarray(graph[2], dtype=np.int32)
    if gids.ndim != 2 or gids.shape[0] != n or gdist.shape != gids.shape or gcnt.shape != (n,):
        raise ValueError("graph must be (ids[n][kg], dist[n][kg], count[n]) over the data set's n rows")
    kg = int(gids.shape[1])
    words = None
    if keep is not None:
        k = np.asarray(keep)
        if k.dtype != np.uint32 and k.dtype != np.bool_:
            raise ValueError("keep must be a bool mask of n, its uint32 words or None")
        words = allowBitmap(k, n)
    ids = np.empty((n, kg), dtype=np.int32)
    dist = np.empty((n, kg), dtype=np.float64)
    cnt = np.empty(n, dtype=np.int32)
    newid = np.empty(n, dtype=np.int32)
    check(lib().rpt_graph_delete_host(ctx._h, ds._h, kg, _vp(gids), _vp(gdist), _vp(gcnt),
                                      None if words is None else _vp(words), metric_flag,
                                      RPT_GRAPH_DELETE_COMPACT if compact else 0, _vp(ids), _vp(dist), _vp(cnt),
                                      _vp(newid)))
    rows = int(np.count_nonzero(newid >= 0)) if compact else n
    return (ids[:rows], dist[:rows], cnt[:rows]), newid


def graphDeleteDev(data, kg, gids_ptr, gdist_ptr, gcount_ptr, keep_ptr, oids_ptr, odist_ptr, ocount_ptr,
                   newid_ptr=0, compact=True, metric=None):
    """graphDelete on device arrays (rpt_graph_delete_dev): data is the Dataset (or a forest over it),
    the graph (int32 [n][kg], float64 [n][kg], int32 [n]), keep (ceil(n / 32) uint32 words, 0 = every
    row stays), the outputs (sized for n rows; with compact only the first popcount rows are written)
    and newid (int32 [n], 0 = not wanted) device addresses; the outputs overlap no input.  The graph is
    read only and NOT validated: untouched rows are copied as they are, touched rows come out sorted
    without their invalid entries.  Enqueued on the ctx stream, not synchronised (ctx.sync() before
    reading); whatever filled the arrays must have finished (see Dataset.dense_device)."""
    metric_flag = _metric_flag(metric)
    ds = _refine_data(data)
    check(lib().rpt_graph_delete_dev(ds.ctx._h, ds._h, int(kg), C.c_void_p(gids_ptr), C.c_void_p(gdist_ptr),
                                     C.c_void_p(gcount_ptr), C.c_void_p(keep_ptr), metric_flag,
                                     RPT_GRAPH_DELETE_COMPACT if compact else 0, C.c_void_p(oids_ptr),
                                     C.c_void_p(odist_ptr), C.c_void_p(ocount_ptr), C.c_void_p(newid_ptr)))


def graphDeleteLast(ctx=None):
    """(kept, touched, evaluated, dropped) of the last graphDelete call on ctx (rpt_graph_delete_last;
    synchronises): kept rows, kept rows that named a deleted row, distances evaluated for them, and the
    valid entries of kept rows that named a deleted row."""
    ctx = ctx or default_context()
    a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().rpt_graph_delete_last(ctx._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return int(a.value), int(b.value), int(c.value), int(d.value)


def _prepare_flags(diversify, reverse):
    return (RPT_GRAPH_PREP_DIVERSIFY if diversify else 0) | (RPT_GRAPH_PREP_REVERSE if reverse else 0)


def _graph_prepare(entry, graph, data, kout, diversify, reverse, metric_flag, ctx):
    """graphPrepare / graphPrepareSV around their _host entry point"""
    ds = _refine_data(data)
    ctx = ctx or ds.ctx
    ids = np.ascontiguousarray(graph[0], dtype=np.int32)
    dist = np.ascontiguousarray(graph[1], dtype=np.float64)
    cnt = np.ascontiguousarray(graph[2], dtype=np.int32)
    if ids.ndim != 2 or ids.shape[0] != ds.n or dist.shape != ids.shape or cnt.shape != (ds.n,):
        raise ValueError("graph must be (ids[n][k], dist[n][k], count[n]) over the data set's n rows")
    k = ids.shape[1]
    if kout is None:
        kout = min(RPT_GRAPH_MAX_K, 2 * k)
    kout = int(kout)
    if kout < 1 or kout > RPT_GRAPH_MAX_K:   # before the outputs are sized by it
        raise ValueError("kout must be in [1,64]")
    oids = np.empty((ds.n, kout), dtype=np.int32)
    odist = np.empty((ds.n, kout), dtype=np.float64)
    ocnt = np.empty(ds.n, dtype=np.int32)
    check(entry(ctx._h, ds._h, int(k), _vp(ids), _vp(dist), _vp(cnt), kout, metric_flag,
                _prepare_flags(diversify, reverse), _vp(oids), _vp(odist), _vp(ocnt)))
    return oids, odist, ocnt


def graphPrepare(graph, data, kout=None, diversify=True, reverse=True, metric=None, ctx=None):
    """A kNN graph made ready for graphSearch (rpt_graph_prepare_host) -> new (ids[n][kout],
    dist[n][kout], count[n]); the input tuple is not modified.  graph: (ids[n][k], dist[n][k],
    count[n]) over `data`, e.g. knnGraph's or knnGraphRefine's; data: a dense Dataset, or a forest
    (its .data is used).  diversify: walking a row in stored order, a neighbour is dropped when an
    already kept neighbour of the row is nearer to it than the point itself is (a plain <; the pair
    distance is metric's fold, bit for bit).  reverse: every point that lists i after that joins row
    i, at the distance stored there.  The row is the first kout (None = min(64, 2 k)) of that set by
    (distance, id); unused slots are id -1, distance +inf.  metric: None / metricL2, metricCosine or
    metricInner, the one the graph was built under.  Under metricInner, which is no metric,
    diversify costs recall: pass diversify=False there.  Deterministic; k and kout <= 64.  SVector
    (CSR) data is refused here: graphPrepareSV (L2), graphPrepareMetricSV (any of the three)."""
    return _graph_prepare(lib().rpt_graph_prepare_host, graph, data, kout, diversify, reverse,
                          _metric_flag(metric), ctx)


def graphPrepareDev(k, data, ids_ptr, dist_ptr, count_ptr, kout, out_ids_ptr, out_dist_ptr, out_count_ptr,
                    diversify=True, reverse=True, metric=None):
    """graphPrepare on device arrays (rpt_graph_prepare_dev): the graph (int32 [n][k], float64 [n][k],
    int32 [n]; read only) and the outputs (int32 [n][kout], float64 [n][kout], int32 [n]) given as
    device addresses.  The arrays are NOT validated: a count is clamped to [0, k], an id outside
    [0, n) is skipped.  Enqueued on the ctx stream, not synchronised (ctx.sync() before reading);
    whatever filled the arrays must have finished (see Dataset.dense_device)."""
    metric_flag = _metric_flag(metric)
    ds = _refine_data(data)
    check(lib().rpt_graph_prepare_dev(ds.ctx._h, ds._h, int(k), C.c_void_p(ids_ptr), C.c_void_p(dist_ptr),
                                      C.c_void_p(count_ptr), int(kout), metric_flag,
                                      _prepare_flags(diversify, reverse), C.c_void_p(out_ids_ptr),
                                      C.c_void_p(out_dist_ptr), C.c_void_p(out_count_ptr)))


def graphPrepareSV(graph, data, kout=None, diversify=True, reverse=True, ctx=None):
    """graphPrepare over SVector (CSR) rows under L2 (rpt_graph_prepare_csr_host) -> new (ids[n][kout],
    dist[n][kout], count[n]).  data: a CSR Dataset, or a forest over one; graph: e.g. knnGraphSV's or
    knnGraphRefineSV's.  The pair distances of diversify are metricDDL2's left fold over the
    dense-ified rows, so the answer (and graphPrepareLast's numbers) is bit-equal to graphPrepare on
    the dense-ified data set with the same graph.  kout: None = min(64, 2 k).  Everything else as
    graphPrepare."""
    return _graph_prepare(lib().rpt_graph_prepare_csr_host, graph, data, kout, diversify, reverse, 0, ctx)


def graphPrepareSVDev(k, data, ids_ptr, dist_ptr, count_ptr, kout, out_ids_ptr, out_dist_ptr, out_count_ptr,
                      diversify=True, reverse=True):
    """graphPrepareSV on device arrays (rpt_graph_prepare_csr_dev): data is a CSR Dataset; the arrays
    and the synchronisation as graphPrepareDev's."""
    ds = _refine_data(data)
    check(lib().rpt_graph_prepare_csr_dev(ds.ctx._h, ds._h, int(k), C.c_void_p(ids_ptr), C.c_void_p(dist_ptr),
                                          C.c_void_p(count_ptr), int(kout), 0,
                                          _prepare_flags(diversify, reverse), C.c_void_p(out_ids_ptr),
                                          C.c_void_p(out_dist_ptr), C.c_void_p(out_count_ptr)))


def graphPrepareMetricSV(distf, graph, data, kout=None, diversify=True, reverse=True, ctx=None):
    """graphPrepareSV under another distance (rpt_graph_prepare_csr_metric_host) -> new (ids[n][kout],
    dist[n][kout], count[n]).  distf: None / metricL2 (the same bits as graphPrepareSV), metricCosine
    or metricInner over the indices both rows store, as knnGraphMetricSV defines them; it must be the
    one the graph's stored distances were computed under (knnGraphMetricSV's, knnGraphRefineMetricSV's;
    not detected).  While every stored value is finite the answer (and graphPrepareLast's numbers) is
    graphPrepare(metric=distf) on the dense-ified data set bit for bit.  Under metricInner diversify
    costs recall: pass diversify=False there.  Everything else as graphPrepareSV.
    (graphPrepare(metric=) itself takes dense data only.)"""
    return _graph_prepare(lib().rpt_graph_prepare_csr_metric_host, graph, data, kout, diversify, reverse,
                          _metric_flag(distf), ctx)


def graphPrepareMetricSVDev(distf, k, data, ids_ptr, dist_ptr, count_ptr, kout, out_ids_ptr, out_dist_ptr,
                            out_count_ptr, diversify=True, reverse=True):
    """graphPrepareMetricSV on device arrays (rpt_graph_prepare_csr_metric_dev): data is a CSR Dataset;
    the arrays and the synchronisation as graphPrepareDev's."""
    metric = _metric_flag(distf)
    ds = _refine_data(data)
    check(lib().rpt_graph_prepare_csr_metric_dev(ds.ctx._h, ds._h, int(k), C.c_void_p(ids_ptr),
                                                 C.c_void_p(dist_ptr), C.c_void_p(count_ptr), int(kout), metric,
                                                 _prepare_flags(diversify, reverse), C.c_void_p(out_ids_ptr),
                                                 C.c_void_p(out_dist_ptr), C.c_void_p(out_count_ptr)))


def graphPrepareLast(ctx=None):
    """(pairs, occluded, capped) of the last graphPrepare / graphPrepareSV call on ctx (rpt_graph_prepare_last;
    synchronises): pair distances evaluated by diversify, entries it dropped, entries of the unions
    that the cap kout cut off, summed over the rows."""
    ctx = ctx or default_context()
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().rpt_graph_prepare_last(ctx._h, C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def knn_last_uncertified(ctx=None):
    """queries of the last knn call whose cut could not be certified and were answered again
    exactly: the f32 prefilter's (L2), or, after a metricCosine / metricInner call, the metric
    kernel's (answered by its exact variant; every query with the option knn_metric_exact)"""
    ctx = ctx or default_context()
    v = C.c_int64()
    check(lib().rpt_knn_last_uncertified(ctx._h, C.byref(v)))
    return int(v.value)


def knn(distf, k, tts, q, dedup=False):
    """RPTree.hs:168-176: `knn distf k forest q` -> [(distance, point id)] in increasing
    distance order, duplicates across trees kept (the reference never de-duplicates).
    distf = metricL2, metricCosine or metricInner (the metric is evaluated on the device)."""
    _metric_flag(distf)                           # anything else: NotImplementedError
    ids, dist, cnt = knnBatch(k, tts, q, dedup=dedup, metric=distf)
    return [(float(dist[0, i]), int(ids[0, i])) for i in range(int(cnt[0]))]


def knnPQ(distf, k, tts, q):
    """RPTree.hs:181-194: like knn, but the heap's `nub` keeps ONE entry per distance value
    (the first in candidate order here; the reference's pick among ties depends on the heap).
    distf = metricL2, metricCosine or metricInner."""
    _metric_flag(distf)
    ids, dist, cnt = knnBatch(k, tts, q, dedup=RPT_KNN_DEDUP_DISTANCE, metric=distf)
    return [(float(dist[0, i]), int(ids[0, i])) for i in range(int(cnt[0]))]


def knnHBatch(k, forest, qs):
    """knnH for a batch of queries -> (off[nq+1], ids, dist): the result of query i is
    ids[off[i]:off[i+1]] with its distances."""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    total = C.c_int64()
    off = np.empty(nq + 1, dtype=np.int64)
    check(lib().rpt_knnh_host(ctx._h, forest._h, forest.data._h, qd._h, int(k), _vp(off), None,
                              None, 0, C.byref(total)))
    ids = np.empty(max(total.value, 1), dtype=np.int32)
    dist = np.empty(max(total.value, 1), dtype=np.float64)
    check(lib().rpt_knnh_host(ctx._h, forest._h, forest.data._h, qd._h, int(k), _vp(off),
                              _vp(ids), _vp(dist), total.value, C.byref(total)))
    return off, ids[:total.value], dist[:total.value]


def knnH(distf, k, tts, q):
    """RPTree.hs:199-217: leaves are visited in increasing margin priority (candidatesH
    :318-342); whole buckets are taken while the running count stays <= k (at least one), the
    bucket taken last first.  As in the reference the result is NOT sorted by distance and NOT
    cut to k: [(distance, point id)]."""
    if distf is not metricL2:
        raise NotImplementedError("the device path evaluates metricL2 only")
    off, ids, dist = knnHBatch(k, tts, q)
    return [(float(dist[i]), int(ids[i])) for i in range(int(off[0]), int(off[1]))]


def _brute_flags(data, metric, reference_metric):
    flags = _metric_flag(metric)
    if reference_metric and data.is_csr:          # dense rows: metricDDL2 is what they get anyway
        if flags:
            raise ValueError("reference_metric is an L2 metric: not with metricCosine / metricInner")
        flags |= RPT_KNN_METRIC_REFERENCE
    return flags


def bruteKnn(forest_or_data, qs, k, ctx=None, metric=None, reference_metric=False):
    """exhaustive kNN on the device, the k best by (distance, id); metric: None / metricL2,
    metricCosine or metricInner.  SVector (CSR) data: the true Euclidean distance, or with
    reference_metric the reference's truncating metricSSL2 (Internal.hs:389-393), bit-exact; under
    metricCosine / metricInner the distance over the indices both vectors store
    (rpt_brute_knn_csr_metric_host; see metricInner), NaN behind every number."""
    data = forest_or_data.data if isinstance(forest_or_data, RPForest) else forest_or_data
    ctx = ctx or data.ctx
    qd, nq = _query_dataset(ctx, data, qs)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    flags = _brute_flags(data, metric, reference_metric)
    if data.is_csr and flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER):
        check(lib().rpt_brute_knn_csr_metric_host(ctx._h, data._h, qd._h, int(k), flags, _vp(ids),
                                                  _vp(dist)))
    elif flags:
        check(lib().rpt_brute_knn_metric_host(ctx._h, data._h, qd._h, int(k), flags, _vp(ids),
                                              _vp(dist)))
    else:
        check(lib().rpt_brute_knn_host(ctx._h, data._h, qd._h, int(k), _vp(ids), _vp(dist)))
    return ids, dist


def recallHits(distf, forest, k, qs, reference_metric=False):
    """-> (hits[nq][T], truth[nq][k]): hits[i][t] = |candidates(tree t, query i) ∩ true kNN of
    query i|, the truth by brute force under distf, both on the device (rpt_recall_hits_host;
    SVector data under metricCosine / metricInner: rpt_recall_hits_csr_metric_host, the truth
    bruteKnn's under that distf)."""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    hits = np.empty((nq, forest.T), dtype=np.int32)
    truth = np.empty((nq, k), dtype=np.int32)
    flags = _brute_flags(forest.data, distf, reference_metric)
    csr_metric = forest.data.is_csr and flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER)
    entry = lib().rpt_recall_hits_csr_metric_host if csr_metric else lib().rpt_recall_hits_host
    check(entry(ctx._h, forest._h, forest.data._h, qd._h, int(k), flags, _vp(hits), _vp(truth)))
    return hits, truth


def recallWithBatch(distf, forest, k, qs, reference_metric=False):
    """recallWith for a batch of queries -> recall[nq]: per query the mean over trees of
    |candidates(tree, q) ∩ true kNN| / k (RPTree.hs:276-282), summed in tree order.  Dense and
    SVector forests, batch and streamed; reference_metric: the truth of SVector data under the
    reference's own metricSSL2."""
    hits, _ = recallHits(distf, forest, k, qs, reference_metric)
    out = np.empty(hits.shape[0], dtype=np.float64)
    for i, row in enumerate(hits.tolist()):
        out[i] = sum(h / k for h in row) / len(row)
    return out


def _brute_allow_flags(data, metric, reference_metric):
    flags = _metric_flag(metric)
    if reference_metric:
        if flags:
            raise ValueError("reference_metric is an L2 metric: not with metricCosine / metricInner")
        if not data.is_csr:
            raise ValueError("reference_metric is the SVector rows' metric")
        flags |= RPT_KNN_METRIC_REFERENCE
    return flags


def bruteKnnAllow(allow, forest_or_data, qs, k, ctx=None, metric=None, reference_metric=False):
    """bruteKnn among SOME of the rows (rpt_brute_knn_allow_host) -> (ids[nq][k], dist[nq][k]): the k
    best allowed rows by (distance, id), NaN last, unused slots id -1 and distance +inf.  allow as
    knnAllow's.  Every row layout and distance; the answer is bruteKnn's over compactRows(data, allow)
    with the ids mapped back, bit for bit; the true Euclidean distance on SVector rows is bruteKnn's
    tolerance-mode distance (rtol 1e-9, atol 1e-12), from the same tiled kernel.  A bitmap per tenant
    or per query: bruteKnnAllowGroup."""
    data = forest_or_data.data if isinstance(forest_or_data, RPForest) else forest_or_data
    ctx = ctx or data.ctx
    qd, nq = _query_dataset(ctx, data, qs)
    words, wp = _allow_words(allow, data.n)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    check(lib().rpt_brute_knn_allow_host(ctx._h, data._h, qd._h, wp, int(k),
                                         _brute_allow_flags(data, metric, reference_metric), _vp(ids), _vp(dist)))
    return ids, dist


def bruteKnnAllowGroup(allow, group, forest_or_data, qs, k, ctx=None, metric=None, reference_metric=False):
    """bruteKnnAllow with a bitmap per query group (rpt_brute_knn_allow_group_host; allow and group as
    knnAllowGroup's) -> (ids[nq][k], dist[nq][k]): query q ranks the rows of bitmap group[q] (-1 = every
    row); its answer is bruteKnnAllow(allow[group[q]], ...)'s, bit for bit.  One ascending id list is
    built per group that a query names, never per query."""
    data = forest_or_data.data if isinstance(forest_or_data, RPForest) else forest_or_data
    ctx = ctx or data.ctx
    qd, nq = _query_dataset(ctx, data, qs)
    words, wp, G, g, gp = _allow_group_args(allow, group, data.n, nq)
    ids = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    check(lib().rpt_brute_knn_allow_group_host(ctx._h, data._h, qd._h, wp, G, gp, int(k),
                                               _brute_allow_flags(data, metric, reference_metric), _vp(ids),
                                               _vp(dist)))
    return ids, dist


def bruteKnnAllowGroupDev(allow_ptr, G, group_ptr, data, queries, k, ids_ptr, dist_ptr, metric=None,
                          reference_metric=False):
    """bruteKnnAllowGroup on device arrays (rpt_brute_knn_allow_group_dev): allow_ptr the device
    address of G rows of ceil(n / 32) uint32 words, group_ptr that of nq int32 (0 = every query
    unfiltered); the rest as bruteKnnAllowDev.  A group value outside [-1, G) means no row is allowed."""
    check(lib().rpt_brute_knn_allow_group_dev(data.ctx._h, data._h, queries._h, C.c_void_p(allow_ptr), int(G),
                                              C.c_void_p(group_ptr), int(k),
                                              _brute_allow_flags(data, metric, reference_metric),
                                              C.c_void_p(ids_ptr), C.c_void_p(dist_ptr)))


def bruteKnnAllowDev(allow_ptr, data, queries, k, ids_ptr, dist_ptr, metric=None, reference_metric=False):
    """bruteKnnAllow on device arrays (rpt_brute_knn_allow_dev): allow_ptr the device address of the
    ceil(n / 32) uint32 words (0 = every id), data and queries Datasets, the outputs (int32 [nq][k],
    float64 [nq][k]) device addresses.  Returns synchronised."""
    check(lib().rpt_brute_knn_allow_dev(data.ctx._h, data._h, queries._h, C.c_void_p(allow_ptr), int(k),
                                        _brute_allow_flags(data, metric, reference_metric),
                                        C.c_void_p(ids_ptr), C.c_void_p(dist_ptr)))


def recallHitsAllow(allow, distf, forest, k, qs, reference_metric=False):
    """recallHits with the truth taken among the allowed rows (rpt_recall_hits_allow_host) ->
    (hits[nq][T], truth[nq][k]): truth = bruteKnnAllow's ids (unused slots -1), hits[i][t] =
    |candidates(tree t, query i) ∩ truth_i|.  The truth holds allowed rows only, so the trees'
    candidates need no filter."""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    words, wp = _allow_words(allow, forest.data.n)
    hits = np.empty((nq, forest.T), dtype=np.int32)
    truth = np.empty((nq, k), dtype=np.int32)
    check(lib().rpt_recall_hits_allow_host(ctx._h, forest._h, forest.data._h, qd._h, wp, int(k),
                                           _brute_allow_flags(forest.data, distf, reference_metric), _vp(hits),
                                           _vp(truth)))
    return hits, truth


def recallHitsAllowGroup(allow, group, distf, forest, k, qs, reference_metric=False):
    """recallHitsAllow with a bitmap per query group (rpt_recall_hits_allow_group_host; allow and group as
    knnAllowGroup's) -> (hits[nq][T], truth[nq][k]), truth = bruteKnnAllowGroup's ids."""
    ctx = forest.ctx
    qd, nq = _query_dataset(ctx, forest.data, qs)
    words, wp, G, g, gp = _allow_group_args(allow, group, forest.data.n, nq)
    hits = np.empty((nq, forest.T), dtype=np.int32)
    truth = np.empty((nq, k), dtype=np.int32)
    check(lib().rpt_recall_hits_allow_group_host(ctx._h, forest._h, forest.data._h, qd._h, wp, G, gp, int(k),
                                                 _brute_allow_flags(forest.data, distf, reference_metric),
                                                 _vp(hits), _vp(truth)))
    return hits, truth


def recallWithAllowBatch(allow, distf, forest, k, qs, reference_metric=False):
    """recallWithBatch among the allowed rows -> recall[nq]: per query the mean over trees of
    |candidates(tree, q) ∩ the k nearest allowed rows| / k, summed in tree order."""
    hits, _ = recallHitsAllow(allow, distf, forest, k, qs, reference_metric)
    out = np.empty(hits.shape[0], dtype=np.float64)
    for i, row in enumerate(hits.tolist()):
        out[i] = sum(h / k for h in row) / len(row)
    return out


def recallWithAllowGroupBatch(allow, group, distf, forest, k, qs, reference_metric=False):
    """recallWithAllowBatch with a bitmap per query group -> recall[nq]."""
    hits, _ = recallHitsAllowGroup(allow, group, distf, forest, k, qs, reference_metric)
    out = np.empty(hits.shape[0], dtype=np.float64)
    for i, row in enumerate(hits.tolist()):
        out[i] = sum(h / k for h in row) / len(row)
    return out


def recallWith(distf, tt, k, q, reference_metric=False):
    """RPTree.hs:259-282: mean over trees of |candidates(tree, q) ∩ true kNN| / k, the truth by
    brute force over all points under distf (metricL2, metricCosine or metricInner): the one-query
    case of recallWithBatch."""
    return float(recallWithBatch(distf, tt, k, q, reference_metric)[0])


# ---------------------------------------------------------------------------------------
# stand-alone kernels (parity tests)
# ---------------------------------------------------------------------------------------
def project(data, R, mode=RPT_PROJ_AUTO, ctx=None):
    """P[c][i] = R[c] `inner` x_i (the N inner products of Internal.hs:504 as one batch)."""
    ctx = ctx or (data.ctx if isinstance(data, Dataset) else default_context())
    ds = Dataset.of(ctx, data)
    R = np.ascontiguousarray(R, dtype=np.float64)
    Cn = R.shape[0]
    dt = np.float64 if ds.dtype == RPT_F64 else np.float32
    P = np.empty((Cn, ds.n), dtype=dt)
    check(lib().rpt_project_host(ctx._h, ds._h, _vp(R), Cn, int(mode), _vp(P)))
    return P


def splitSegments(keys, perm, seg_off, seg_len, ctx=None):
    """partitionAtMedian (Internal.hs:486-505) of every segment on caller-supplied projections.
    Returns (perm sorted per segment, thr_mg[S][3])."""
    ctx = ctx or default_context()
    keys = np.ascontiguousarray(keys, dtype=np.float64)
    perm = np.array(perm, dtype=np.int32)
    so = np.ascontiguousarray(seg_off, dtype=np.int64)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    out = np.empty((len(so), 3), dtype=np.float64)
    check(lib().rpt_split_segments(ctx._h, _vp(keys), len(keys), _vp(perm), _vp(so), _vp(sl),
                                   len(so), _vp(out)))
    return perm, out
