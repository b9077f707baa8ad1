{-# LANGUAGE ForeignFunctionInterface #-}
{-# LANGUAGE FlexibleContexts #-}
-- | Binding of the MI355X hot path (include/rptree_hip.h) under the unchanged Data.RPTree API.
--
-- WRITTEN BLIND: there is no GHC in the build image, so this module has not been compiled.
-- It shows the binding a maintainer would add next to src/Data/RPTree/Batch.hs; the tested
-- mirrors of exactly this call sequence are rp-tree_amd/python/rptree_amd/__init__.py and
-- rp-tree_amd/host/rptree.hpp.
module Data.RPTree.HIP (forestBatchHIP, forestBatchHIPWith, forestHIP, withDeviceData, withDeviceForest,
                        withDeviceForestOn, knnHIP, knnMetricHIP, knnGraphHIP, knnGraphRefineHIP, knnGraphMetricHIP, knnGraphRefineMetricHIP, knnGraphSVHIP, knnGraphRefineSVHIP, knnGraphMetricSVHIP, knnGraphRefineMetricSVHIP, graphSearchHIP, graphSearchAllowHIP, graphInsertHIP, graphDeleteHIP, graphSearchSVHIP, graphPrepareHIP, graphPrepareSVHIP, graphSearchMetricSVHIP, graphPrepareMetricSVHIP, recallWithHIP, knnMetricSVHIP, recallWithMetricSVHIP, knnVoteHIP, voteCandidatesHIP, knnAllowHIP, bruteKnnAllowHIP, recallWithAllowHIP, graphSearchAllowGroupHIP, graphSearchAllowGroupDevHIP, knnAllowGroupHIP, knnAllowGroupDevHIP, allowGroupCandidatesHIP, bruteKnnAllowGroupHIP, bruteKnnAllowGroupDevHIP, recallWithAllowGroupHIP, withDeviceDataSV, Metric(..), ProjMode(..), FlatForest(..),
                        DeviceForest(..), DeviceData(..)) where

import Control.Exception (Exception, bracket, throwIO)
import Control.Monad (when)
import Data.Int (Int8, Int32, Int64)
import Data.Word (Word32, Word64)
import Foreign.C.String (CString, peekCString)
import Foreign.Marshal.Alloc (alloca)
import Foreign.Ptr (Ptr, nullPtr)
import Foreign.Storable (peek)
import System.IO.Unsafe (unsafePerformIO)
import qualified Data.IntMap.Strict as IM
import qualified Data.Vector as V
import qualified Data.Vector.Storable as VS
import qualified Data.Vector.Storable.Mutable as VSM
import qualified Data.Vector.Unboxed as VU

import System.Random.SplitMix.Distributions (sample, stdNormal)
import Data.RPTree.Gen (sparse)
import Data.RPTree.Internal (Embed(..), DVector(..), SVector(..), RPForest, RPTree(..), RPT(..), Margin(..))
import Data.Semigroup (Max(..), Min(..))

data Ctx; data Dataset; data Forest; data Comm; data ShardedForest

-- `safe`: every call may launch kernels and synchronise; do not block the RTS.
foreign import ccall safe "rpt_ctx_create"          c_ctx_create     :: Int32 -> Ptr (Ptr Ctx) -> IO Int32
foreign import ccall safe "rpt_ctx_destroy"         c_ctx_destroy    :: Ptr Ctx -> IO Int32
foreign import ccall safe "rpt_dataset_dense_host"  c_dataset_dense  :: Ptr Ctx -> Ptr Double -> Int64 -> Int32 -> Int32 -> Ptr (Ptr Dataset) -> IO Int32
foreign import ccall safe "rpt_dataset_free"        c_dataset_free   :: Ptr Dataset -> IO Int32
foreign import ccall safe "rpt_forest_build"        c_forest_build   :: Ptr Ctx -> Ptr Dataset -> Ptr Double -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr (Ptr Forest) -> IO Int32
foreign import ccall safe "rpt_forest_free"         c_forest_free    :: Ptr Forest -> IO Int32
foreign import ccall safe "rpt_forest_get_perm"     c_forest_perm    :: Ptr Forest -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_forest_get_nodes"    c_forest_nodes   :: Ptr Forest -> Ptr Double -> Ptr Double -> Ptr Double -> IO Int32
-- forest / tree (Conduit.hs:58-121): the fold of insert over chunks, Internal.hs:245-297
foreign import ccall safe "rpt_forest_stream_build" c_stream_build   :: Ptr Ctx -> Ptr Dataset -> Ptr Double -> Int32 -> Int32 -> Int32 -> Int64 -> Int32 -> Ptr (Ptr Forest) -> IO Int32
foreign import ccall safe "rpt_forest_get_topology" c_forest_topo    :: Ptr Forest -> Ptr Int64 -> Ptr Int8 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> IO Int32
foreign import ccall safe "rpt_knn_host"            c_knn_host       :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
-- knnH (RPTree.hs:199-217): two calls, the first with null outputs returns the result size
foreign import ccall safe "rpt_knnh_host"           c_knnh_host      :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int32 -> Ptr Int64 -> Ptr Int32 -> Ptr Double -> Int64 -> Ptr Int64 -> IO Int32
foreign import ccall safe "rpt_dataset_csr_host"    c_dataset_csr    :: Ptr Ctx -> Ptr Int64 -> Ptr Int32 -> Ptr Double -> Int64 -> Int32 -> Int32 -> Ptr (Ptr Dataset) -> IO Int32
foreign import ccall safe "rpt_recall_hits_host"    c_recall_hits    :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int32 -> Int32 -> Ptr Int32 -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_graph_host"      c_knn_graph_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_graph_refine_host" c_knn_graph_refine_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_graph_metric_host" c_knn_graph_metric_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_graph_refine_metric_host" c_knn_graph_refine_metric_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_graph_csr_host" c_knn_graph_csr_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_graph_refine_csr_host" c_knn_graph_refine_csr_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_graph_csr_metric_host" c_knn_graph_csr_metric_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_graph_refine_csr_metric_host" c_knn_graph_refine_csr_metric_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_search_host" c_graph_search_host :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Int32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_search_allow_host" c_graph_search_allow_host :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Int32 -> Int32 -> Ptr Int32 -> Ptr Word32 -> Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_insert_host" c_graph_insert_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> Int64 -> Int32 -> Ptr Int32 -> Int32 -> Int64 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_delete_host" c_graph_delete_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> Ptr Word32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_search_csr_host" c_graph_search_csr_host :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Int32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_prepare_host" c_graph_prepare_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_prepare_csr_host" c_graph_prepare_csr_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_search_csr_metric_host" c_graph_search_csr_metric_host :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Int32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_prepare_csr_metric_host" c_graph_prepare_csr_metric_host :: Ptr Ctx -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_csr_metric_host" c_knn_csr_metric_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_recall_hits_csr_metric_host" c_recall_hits_csr_metric :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int32 -> Int32 -> Ptr Int32 -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_vote_host" c_knn_vote_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_allow_host" c_knn_allow_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Ptr Word32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_brute_knn_allow_host" c_brute_knn_allow_host :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Ptr Word32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> IO Int32
foreign import ccall safe "rpt_recall_hits_allow_host" c_recall_hits_allow_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Ptr Word32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Int32 -> IO Int32
-- the grouped allow-list: (allow, G, group) where allow stands above
foreign import ccall safe "rpt_graph_search_allow_group_host" c_graph_search_allow_group_host :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Int32 -> Int32 -> Ptr Int32 -> Ptr Word32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_graph_search_allow_group_dev" c_graph_search_allow_group_dev :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Int32 -> Ptr Int32 -> Ptr Int32 -> Int32 -> Ptr Int32 -> Ptr Word32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_allow_group_host" c_knn_allow_group_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Ptr Word32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_knn_allow_group_dev" c_knn_allow_group_dev :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Ptr Word32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32
foreign import ccall safe "rpt_allow_group_candidates_host" c_allow_group_candidates_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Word32 -> Int32 -> Ptr Int32 -> Ptr Int64 -> Ptr Int32 -> Int64 -> Ptr Int64 -> IO Int32
foreign import ccall safe "rpt_brute_knn_allow_group_host" c_brute_knn_allow_group_host :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Ptr Word32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> IO Int32
foreign import ccall safe "rpt_brute_knn_allow_group_dev" c_brute_knn_allow_group_dev :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Ptr Word32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> IO Int32
foreign import ccall safe "rpt_recall_hits_allow_group_host" c_recall_hits_allow_group_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Ptr Word32 -> Int32 -> Ptr Int32 -> Int32 -> Int32 -> Ptr Int32 -> Ptr Int32 -> IO Int32
-- two calls, the first with null outputs returns the total
foreign import ccall safe "rpt_vote_candidates_host" c_vote_candidates_host :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int32 -> Ptr Int64 -> Ptr Int32 -> Ptr Int32 -> Int64 -> Ptr Int64 -> IO Int32
foreign import ccall unsafe "rpt_last_error"        c_last_error     :: IO CString
-- multi-GPU (csrc/comm.hip on librccl): one process drives n devices; per-device arguments are
-- arrays with one entry per device (Foreign.Marshal.Array.withArray)
foreign import ccall safe "rpt_comm_init"            c_comm_init      :: Int32 -> Ptr (Ptr Comm) -> IO Int32
foreign import ccall safe "rpt_comm_destroy"         c_comm_destroy   :: Ptr Comm -> IO Int32
foreign import ccall safe "rpt_comm_ctx"             c_comm_ctx       :: Ptr Comm -> Int32 -> Ptr (Ptr Ctx) -> IO Int32
foreign import ccall safe "rpt_forest_build_sharded" c_build_sharded  :: Ptr Comm -> Ptr (Ptr Dataset) -> Ptr Double -> Int32 -> Int32 -> Int32 -> Int32 -> Ptr (Ptr ShardedForest) -> IO Int32
foreign import ccall safe "rpt_sharded_forest_free"  c_sharded_free   :: Ptr ShardedForest -> IO Int32
foreign import ccall safe "rpt_knn_sharded"          c_knn_sharded    :: Ptr Comm -> Ptr ShardedForest -> Ptr (Ptr Dataset) -> Ptr (Ptr Dataset) -> Int32 -> Int32 -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO Int32

-- | Projection kernel of a build (include/rptree_hip.h RPT_PROJ_*).  'ProjAuto' on Double data is the
-- exact-order kernel (separate multiply and add in innerSD's order, Internal.hs:369-382: leaf
-- assignments identical to the pure library's); 'ProjMfma' is the matrix-core kernel bench.py times
-- (projection values within 1e-5 |x||r|, a handful of leaf flips per million points at most).
data ProjMode = ProjAuto | ProjExact | ProjMfma deriving (Eq, Show)

projFlag :: ProjMode -> Int32
projFlag ProjAuto = 0
projFlag ProjExact = 1
projFlag ProjMfma = 2

newtype RPTHipError = RPTHipError String deriving Show
instance Exception RPTHipError          -- next to RPTError (Internal.hs:66-72)

check :: Int32 -> IO ()
check 0 = pure ()
check _ = c_last_error >>= peekCString >>= throwIO . RPTHipError

-- | The flat forest of include/rptree_hip.h, copied out so ordinary 'RPTree' values can be rebuilt.
data FlatForest = FlatForest
  { ffPerm :: VS.Vector Int32, ffThr, ffLo, ffHi :: VS.Vector Double
  , ffN, ffTrees, ffDepth, ffMinLeaf :: Int }

-- | Dense-ify one hyperplane in O(d + nnz): zeros where the sparse vector has no component.
denseOf :: Int -> SVector Double -> VS.Vector Double
denseOf dim (SV _ vv) = VS.replicate dim 0 VS.// VU.toList vv

-- | Drop-in for 'Data.RPTree.Batch.forestBatch' (Batch.hs:48-63) on dense data.  Everything the
-- result needs is copied out, so the device objects are released before returning (bracket:
-- also when a call fails) — nothing is left to finalisers.
forestBatchHIP :: Word64 -> Int -> Int -> Int -> Double -> Int
               -> V.Vector (Embed DVector Double x)
               -> RPForest Double (V.Vector (Embed DVector Double x))
forestBatchHIP = forestBatchHIPWith ProjAuto

-- | ... with the projection kernel chosen by the caller ('ProjMfma' = the timed one).  One context and
-- one upload per call: a host that builds several forests over the same points, or queries the
-- forest afterwards, uses 'withDeviceData' / 'withDeviceForestOn' instead and pays the upload once.
forestBatchHIPWith :: ProjMode -> Word64 -> Int -> Int -> Int -> Double -> Int
                   -> V.Vector (Embed DVector Double x)
                   -> RPForest Double (V.Vector (Embed DVector Double x))
forestBatchHIPWith mode seed maxd minl ntrees pnz dim src = unsafePerformIO $ do
  -- hyperplanes: sampled by the HOST exactly as Batch.hs:59-61 does
  let rvss = sample seed $ V.replicateM ntrees (V.replicateM maxd (sparse pnz dim stdNormal))
      rflat = VS.concat [ denseOf dim r | rvs <- V.toList rvss, r <- V.toList rvs ]     -- R[T][L][d]
      xflat = VS.concat [ VS.convert v | Embed (DV v) _ <- V.toList src ]                -- X[N][d]
      n = V.length src
      nodes = 2 ^ maxd - 1
      acquire mk = alloca $ \pp -> mk pp >>= check >> peek pp
  ff <- bracket (acquire (c_ctx_create 0)) c_ctx_destroy $ \ctx ->
        bracket (acquire (\pp -> VS.unsafeWith xflat (\px -> c_dataset_dense ctx px (fromIntegral n) (fromIntegral dim) 0 pp)))
                c_dataset_free $ \ds ->
        bracket (acquire (\pp -> VS.unsafeWith rflat (\pr -> c_forest_build ctx ds pr (fromIntegral ntrees) (fromIntegral maxd) (fromIntegral minl) (projFlag mode) pp)))
                c_forest_free $ \f -> do
          perm <- VSM.new (ntrees * n); thr <- VSM.new (ntrees * nodes); lo <- VSM.new (ntrees * nodes); hi <- VSM.new (ntrees * nodes)
          VSM.unsafeWith perm (c_forest_perm f) >>= check
          VSM.unsafeWith thr (\a -> VSM.unsafeWith lo (\b -> VSM.unsafeWith hi (c_forest_nodes f a b))) >>= check
          FlatForest <$> VS.freeze perm <*> VS.freeze thr <*> VS.freeze lo <*> VS.freeze hi
                     <*> pure n <*> pure ntrees <*> pure maxd <*> pure minl
  pure $ IM.fromList [ (t, RPTree (rvss V.! t) (rebuild ff src t)) | t <- [0 .. ntrees - 1] ]

-- | Rebuild the lazy 'RPT' (Internal.hs:139-149) of tree t from the flat arrays: topology is a
-- pure function of (N, minLeaf, maxDepth) (Internal.hs:289,495,503).
rebuild :: FlatForest -> V.Vector a -> Int -> RPT Double () (V.Vector a)
rebuild ff src t = go 0 0 0 (ffN ff)
  where
    nodes = 2 ^ ffDepth ff - 1
    go lev h off m
      | lev >= ffDepth ff || m <= ffMinLeaf ff =
          Tip () (V.generate m (\i -> src V.! fromIntegral (ffPerm ff VS.! (t * ffN ff + off + i))))
      | otherwise =
          let nh = m `div` 2; ix = t * nodes + h
          in Bin () (ffThr ff VS.! ix) (Margin (Max (ffLo ff VS.! ix)) (Min (ffHi ff VS.! ix)))
                 (go (lev + 1) (2 * h + 1) off nh) (go (lev + 1) (2 * h + 2) (off + nh) (m - nh))

-- | Drop-in for 'Data.RPTree.Conduit.forest' (Conduit.hs:104-121) on dense data once the conduit
-- has been sunk into a vector (@src <- runConduit (source .| C.sinkVector)@): the reference's fold
-- of 'insert' over chunks of @chunk@ points runs on the device (rpt_forest_stream_build) and the
-- explicit topology it returns (kind 1 = Bin, 2 = Tip per heap slot, the same for every tree) is
-- turned back into ordinary 'RPT' values.
forestHIP :: Word64 -> Int -> Int -> Int -> Int -> Double -> Int
          -> V.Vector (Embed DVector Double x)
          -> RPForest Double (V.Vector (Embed DVector Double x))
forestHIP seed maxd minl ntrees chunk pnz dim src = unsafePerformIO $ do
  let rvss = sample seed $ V.replicateM ntrees (V.replicateM maxd (sparse pnz dim stdNormal))  -- Conduit.hs:116-118
      rflat = VS.concat [ denseOf dim r | rvs <- V.toList rvss, r <- V.toList rvs ]
      xflat = VS.concat [ VS.convert v | Embed (DV v) _ <- V.toList src ]
      n = V.length src
      slots = 2 ^ (maxd + 1) - 1
      acquire mk = alloca $ \pp -> mk pp >>= check >> peek pp
  (perm, thr, lo, hi, kind, loff, llen) <-
    bracket (acquire (c_ctx_create 0)) c_ctx_destroy $ \ctx ->
    bracket (acquire (\pp -> VS.unsafeWith xflat (\px -> c_dataset_dense ctx px (fromIntegral n) (fromIntegral dim) 0 pp)))
            c_dataset_free $ \ds ->
    bracket (acquire (\pp -> VS.unsafeWith rflat (\pr -> c_stream_build ctx ds pr (fromIntegral ntrees) (fromIntegral maxd) (fromIntegral minl) (fromIntegral chunk) 0 pp)))
            c_forest_free $ \f -> do
      perm <- VSM.new (ntrees * n); thr <- VSM.new (ntrees * slots); lo <- VSM.new (ntrees * slots); hi <- VSM.new (ntrees * slots)
      kind <- VSM.new slots; loff <- VSM.new slots; llen <- VSM.new slots
      VSM.unsafeWith perm (c_forest_perm f) >>= check
      VSM.unsafeWith thr (\a -> VSM.unsafeWith lo (\b -> VSM.unsafeWith hi (c_forest_nodes f a b))) >>= check
      alloca $ \ps -> alloca $ \ph -> alloca $ \pd ->
        VSM.unsafeWith kind (\k -> VSM.unsafeWith loff (\o -> VSM.unsafeWith llen (\l -> c_forest_topo f ps k o l ph pd))) >>= check
      (,,,,,,) <$> VS.freeze perm <*> VS.freeze thr <*> VS.freeze lo <*> VS.freeze hi
               <*> VS.freeze kind <*> VS.freeze loff <*> VS.freeze llen
  let tree t = go 0
        where
          go h | kind VS.! h == 1 =
                   let ix = t * slots + h
                   in Bin () (thr VS.! ix) (Margin (Max (lo VS.! ix)) (Min (hi VS.! ix))) (go (2 * h + 1)) (go (2 * h + 2))
               | otherwise =            -- Tip (kind 2; an absent slot never hangs below a Bin)
                   Tip () (V.generate (fromIntegral (llen VS.! h))
                             (\i -> src V.! fromIntegral (perm VS.! (t * n + fromIntegral (loff VS.! h) + i))))
  pure $ IM.fromList [ (t, RPTree (rvss V.! t) (tree t)) | t <- [0 .. ntrees - 1] ]

-- | A forest that STAYS on the device, for hosts that build once and query many times (what the
-- north star means by "host code stays Haskell": the handle is the currency, as 'RPForest' is in
-- the reference).  The context, the packed dataset and the forest live for the extent of the
-- callback; queries go through 'knnHIP' without re-uploading anything.
data DeviceForest = DeviceForest { dfCtx :: Ptr Ctx, dfData :: Ptr Dataset, dfForest :: Ptr Forest }

-- | A context and the packed point set on the device, for the extent of the callback: the upload
-- (1 GB at C2: 18 ms over PCIe against a 5 ms build) is paid once however many forests are built.
data DeviceData = DeviceData { ddCtx :: Ptr Ctx, ddData :: Ptr Dataset, ddDim :: Int }

withDeviceData :: Int -> V.Vector (Embed DVector Double x) -> (DeviceData -> IO a) -> IO a
withDeviceData dim src act = do
  let xflat = VS.concat [ VS.convert v | Embed (DV v) _ <- V.toList src ]
      acquire mk = alloca $ \pp -> mk pp >>= check >> peek pp
  bracket (acquire (c_ctx_create 0)) c_ctx_destroy $ \ctx ->
    bracket (acquire (\pp -> VS.unsafeWith xflat (\px -> c_dataset_dense ctx px (fromIntegral (V.length src)) (fromIntegral dim) 0 pp)))
            c_dataset_free $ \ds -> act (DeviceData ctx ds dim)

-- | One forest over device-resident points (any number of these per 'withDeviceData').
withDeviceForestOn :: DeviceData -> ProjMode -> Word64 -> Int -> Int -> Int -> Double
                   -> (DeviceForest -> IO a) -> IO a
withDeviceForestOn (DeviceData ctx ds dim) mode seed maxd minl ntrees pnz act = do
  let rvss = sample seed $ V.replicateM ntrees (V.replicateM maxd (sparse pnz dim stdNormal))
      rflat = VS.concat [ denseOf dim r | rvs <- V.toList rvss, r <- V.toList rvs ]
      acquire mk = alloca $ \pp -> mk pp >>= check >> peek pp
  bracket (acquire (\pp -> VS.unsafeWith rflat (\pr -> c_forest_build ctx ds pr (fromIntegral ntrees) (fromIntegral maxd) (fromIntegral minl) (projFlag mode) pp)))
          c_forest_free $ \f -> act (DeviceForest ctx ds f)

withDeviceForest :: Word64 -> Int -> Int -> Int -> Double -> Int -> V.Vector (Embed DVector Double x)
                 -> (DeviceForest -> IO a) -> IO a
withDeviceForest seed maxd minl ntrees pnz dim src act =
  withDeviceData dim src $ \dd -> withDeviceForestOn dd ProjAuto seed maxd minl ntrees pnz act

-- | 'knn metricL2 k' (RPTree.hs:168-176) for a batch of dense queries: ids and distances.
knnHIP :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int -> Int -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnHIP ctx f ds qs nq k = knnMetricHIP MetricL2 ctx f ds qs nq k

-- | The distances the device can rank by.  A Haskell closure cannot run on the device, so 'knn''s
-- distf is one of these: 'MetricL2' = metricL2; 'MetricCosine' = @\x q -> 1 - inner x q / (sqrt (inner x x)
-- * sqrt (inner q q))@; 'MetricInner' = @\x q -> negate (inner x q)@ — with inner = innerDD's left
-- fold in Double (Internal.hs:384-385), bit for bit (RPT_KNN_METRIC_COSINE / _INNER).
data Metric = MetricL2 | MetricCosine | MetricInner deriving (Eq, Show)

metricFlag :: Metric -> Int32
metricFlag MetricL2 = 0
metricFlag MetricCosine = 33554432   -- RPT_KNN_METRIC_COSINE (1 << 25)
metricFlag MetricInner = 67108864    -- RPT_KNN_METRIC_INNER (1 << 26)

-- | 'knn distf k' (RPTree.hs:168-176) under one of the device metrics, for a batch of dense queries.
knnMetricHIP :: Metric -> Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int -> Int -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnMetricHIP m ctx f ds qs nq k = do
  ids <- VSM.new (nq * k); dist <- VSM.new (nq * k); cnt <- VSM.new nq
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_host ctx f ds qs (fromIntegral k) (metricFlag m) a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | The kNN graph of the forest's own points: 'knn metricL2 k' (RPTree.hs:174-176) with every stored
-- point as the query, built leaf by leaf (rpt_knn_graph_host).  Row i holds the first k, by
-- (distance, id), of the points j /= i that share a leaf with i in some tree, with metricDDL2's
-- left fold (Internal.hs:403-406) as the distance; count[i] entries are valid, the rest are
-- id -1, distance +Infinity.  @Just earlier@ folds an earlier answer over the same data set and k
-- in (RPT_GRAPH_ACCUMULATE = 1: another forest, a tree shard); the order of folding does not matter.
-- Dense batch forests, k <= 64; n = number of stored points.
knnGraphHIP :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int -> Int
            -> Maybe (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
            -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnGraphHIP ctx f ds n k earlier = do
  (ids, dist, cnt, flags) <- case earlier of
    Nothing -> (,,,) <$> VSM.new (n * k) <*> VSM.new (n * k) <*> VSM.new n <*> pure 0
    Just (i0, d0, c0) -> (,,,) <$> VS.thaw i0 <*> VS.thaw d0 <*> VS.thaw c0 <*> pure 1
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_graph_host ctx f ds (fromIntegral k) flags a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | NN-descent rounds over a kNN graph of the data set (rpt_knn_graph_refine_host): one round gives
-- row i the first k, by (distance, id), of its neighbours, up to @reverse@ of the points that list i
-- (0 = none) and all of their neighbours, with metricDDL2's left fold as the distance of every new
-- entry; @iters@ rounds, ended early by a round that changes nothing.  Deterministic; no forest
-- takes part.  The input vectors are not modified.  k and reverse <= 64; n = number of stored points.
knnGraphRefineHIP :: Ptr Ctx -> Ptr Dataset -> Int -> Int -> Int -> Int
                  -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                  -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnGraphRefineHIP ctx ds _n k reverse iters (i0, d0, c0) = do
  ids <- VS.thaw i0
  dist <- VS.thaw d0
  cnt <- VS.thaw c0
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_graph_refine_host ctx ds (fromIntegral k) (fromIntegral reverse) (fromIntegral iters) 0 a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'knnGraphHIP' for a forest over SVector rows ('withDeviceDataSV'; rpt_knn_graph_csr_host).  The
-- distance is metricDDL2's left fold over the dense-ified rows (absent entries +0.0), so the answer
-- is bit-equal to 'knnGraphHIP' on the dense-ified data set with the same forest; the kernels visit
-- only the 32-column windows in which a leaf holds a nonzero.  Indices must ascend strictly.
knnGraphSVHIP :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int -> Int
              -> Maybe (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
              -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnGraphSVHIP ctx f ds n k earlier = do
  (ids, dist, cnt, flags) <- case earlier of
    Nothing -> (,,,) <$> VSM.new (n * k) <*> VSM.new (n * k) <*> VSM.new n <*> pure 0
    Just (i0, d0, c0) -> (,,,) <$> VS.thaw i0 <*> VS.thaw d0 <*> VS.thaw c0 <*> pure 1
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_graph_csr_host ctx f ds (fromIntegral k) flags a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'knnGraphRefineHIP' over SVector rows (rpt_knn_graph_refine_csr_host): the same rounds, bit-equal
-- to 'knnGraphRefineHIP' on the dense-ified data set.
knnGraphRefineSVHIP :: Ptr Ctx -> Ptr Dataset -> Int -> Int -> Int -> Int
                    -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                    -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnGraphRefineSVHIP ctx ds _n k reverse iters (i0, d0, c0) = do
  ids <- VS.thaw i0
  dist <- VS.thaw d0
  cnt <- VS.thaw c0
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_graph_refine_csr_host ctx ds (fromIntegral k) (fromIntegral reverse) (fromIntegral iters) 0 a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'knnGraphHIP' under another distance (rpt_knn_graph_metric_host): 'MetricCosine' / 'MetricInner'
-- are the distances of 'knnMetricHIP' (the left-fold dot in Double for every dtype, bit-exact; a zero
-- row is NaN under the cosine distance and ranks last); 'MetricL2' gives 'knnGraphHIP''s bits.
-- @Just earlier@ must be an answer under the same metric (another is not detected: stored distances
-- are taken as stored).
knnGraphMetricHIP :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Metric -> Int -> Int
                  -> Maybe (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                  -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnGraphMetricHIP ctx f ds m n k earlier = do
  (ids, dist, cnt, flags) <- case earlier of
    Nothing -> (,,,) <$> VSM.new (n * k) <*> VSM.new (n * k) <*> VSM.new n <*> pure 0
    Just (i0, d0, c0) -> (,,,) <$> VS.thaw i0 <*> VS.thaw d0 <*> VS.thaw c0 <*> pure 1
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_graph_metric_host ctx f ds (fromIntegral k) (metricFlag m) flags a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'knnGraphRefineHIP' under another distance (rpt_knn_graph_refine_metric_host); the graph's stored
-- distances must be that metric's ('knnGraphMetricHIP' under the same 'Metric').
knnGraphRefineMetricHIP :: Ptr Ctx -> Ptr Dataset -> Metric -> Int -> Int -> Int -> Int
                        -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                        -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnGraphRefineMetricHIP ctx ds m _n k reverse iters (i0, d0, c0) = do
  ids <- VS.thaw i0
  dist <- VS.thaw d0
  cnt <- VS.thaw c0
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_graph_refine_metric_host ctx ds (fromIntegral k) (fromIntegral reverse) (fromIntegral iters) (metricFlag m) 0 a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'knnGraphSVHIP' under another distance (rpt_knn_graph_csr_metric_host): 'MetricCosine' /
-- 'MetricInner' over the indices both rows store, the distances of 'knnMetricSVHIP' (the left fold
-- of the shared indices' products from +0.0, in Double).  While every stored value is finite that
-- is 'knnGraphMetricHIP' on the dense-ified rows bit for bit; with a stored infinity or NaN it is
-- not (the dense fold meets inf * 0), and the answer is this definition.  'MetricL2' gives
-- 'knnGraphSVHIP''s bits.  @Just earlier@ must be an answer under the same metric.
knnGraphMetricSVHIP :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Metric -> Int -> Int
                    -> Maybe (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                    -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnGraphMetricSVHIP ctx f ds m n k earlier = do
  (ids, dist, cnt, flags) <- case earlier of
    Nothing -> (,,,) <$> VSM.new (n * k) <*> VSM.new (n * k) <*> VSM.new n <*> pure 0
    Just (i0, d0, c0) -> (,,,) <$> VS.thaw i0 <*> VS.thaw d0 <*> VS.thaw c0 <*> pure 1
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_graph_csr_metric_host ctx f ds (fromIntegral k) (metricFlag m) flags a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'knnGraphRefineSVHIP' under another distance (rpt_knn_graph_refine_csr_metric_host); the graph's
-- stored distances must be that metric's ('knnGraphMetricSVHIP' under the same 'Metric').
knnGraphRefineMetricSVHIP :: Ptr Ctx -> Ptr Dataset -> Metric -> Int -> Int -> Int -> Int
                          -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                          -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnGraphRefineMetricSVHIP ctx ds m _n k reverse iters (i0, d0, c0) = do
  ids <- VS.thaw i0
  dist <- VS.thaw d0
  cnt <- VS.thaw c0
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (c_knn_graph_refine_csr_metric_host ctx ds (fromIntegral k) (fromIntegral reverse) (fromIntegral iters) (metricFlag m) 0 a b))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | Query a kNN graph: best-first beam search (rpt_graph_search_host).  @(gids, gcount)@ is a graph
-- over the data set with @kg@ slots per row ('knnGraphHIP' \/ 'knnGraphRefineHIP', the distances are
-- not read); @seeds@ holds @s@ start ids per query (-1 = unused slot, s <= 64).  The seeds are
-- offered to a beam of at most @ef@ entries sorted by (distance, id), then the graph row of the
-- beam's first unexpanded entry, until none is left; the answer is the first k of the beam, unused
-- slots id -1, distance +Infinity.  Distances are the metric's left fold in Double ('MetricCosine' \/
-- 'MetricInner' bit-equal to the exhaustive answer).  k <= 64, k <= ef <= 256; nq = number of queries.
graphSearchHIP :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Metric -> Int -> Int
               -> (VS.Vector Int32, VS.Vector Int32) -> Int -> VS.Vector Int32 -> Int -> Int
               -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphSearchHIP ctx ds qs m nq kg (gids, gcount) s seeds k ef = do
  ids <- VSM.new (nq * k); dist <- VSM.new (nq * k); cnt <- VSM.new nq
  VS.unsafeWith gids (\pg -> VS.unsafeWith gcount (\pc -> VS.unsafeWith seeds (\ps ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_search_host ctx ds qs (fromIntegral kg) pg pc (fromIntegral s) ps (fromIntegral k) (fromIntegral ef) (metricFlag m) 0 a b)))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'graphSearchHIP' over SVector rows under L2 (rpt_graph_search_csr_host): @ds@ and @qs@ are CSR data
-- sets ('withDeviceDataSV') of one dimension and element type.  The distances are metricDDL2's left
-- fold over the dense-ified query and row (absent entries +0.0), so the answer is bit-equal to
-- 'graphSearchHIP' with 'MetricL2' on the dense-ified data set and queries with the same graph and
-- seeds.  The rows' indices must ascend strictly.
graphSearchSVHIP :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Int -> Int
                 -> (VS.Vector Int32, VS.Vector Int32) -> Int -> VS.Vector Int32 -> Int -> Int
                 -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphSearchSVHIP ctx ds qs nq kg (gids, gcount) s seeds k ef = do
  ids <- VSM.new (nq * k); dist <- VSM.new (nq * k); cnt <- VSM.new nq
  VS.unsafeWith gids (\pg -> VS.unsafeWith gcount (\pc -> VS.unsafeWith seeds (\ps ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_search_csr_host ctx ds qs (fromIntegral kg) pg pc (fromIntegral s) ps (fromIntegral k) (fromIntegral ef) 0 0 a b)))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'graphSearchSVHIP' under another distance (rpt_graph_search_csr_metric_host): 'MetricCosine' /
-- 'MetricInner' over the indices both the query and the row store (the left fold of the shared
-- indices' products from +0.0, as 'knnGraphMetricSVHIP' defines them); 'MetricL2' gives
-- 'graphSearchSVHIP's bits.  While every stored value is finite the answer is 'graphSearchHIP' under
-- the same 'Metric' on the dense-ified data set and queries bit for bit.  A query without nonzeros is
-- NaN from everything under 'MetricCosine' and gets its answers ordered by id.
graphSearchMetricSVHIP :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Metric -> Int -> Int
                       -> (VS.Vector Int32, VS.Vector Int32) -> Int -> VS.Vector Int32 -> Int -> Int
                       -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphSearchMetricSVHIP ctx ds qs m nq kg (gids, gcount) s seeds k ef = do
  ids <- VSM.new (nq * k); dist <- VSM.new (nq * k); cnt <- VSM.new nq
  VS.unsafeWith gids (\pg -> VS.unsafeWith gcount (\pc -> VS.unsafeWith seeds (\ps ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_search_csr_metric_host ctx ds qs (fromIntegral kg) pg pc (fromIntegral s) ps (fromIntegral k) (fromIntegral ef) (metricFlag m) 0 a b)))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'graphSearchHIP' among SOME of the points (rpt_graph_search_allow_host): @allow@ holds
-- ceil(n \/ 32) words, id i allowed when bit (i .&. 31) of word (i `shiftR` 5) is set; 'Nothing' allows
-- every id.  @ds@ and @qs@ are both dense or both CSR, under any 'Metric'.  @ef@ counts ALLOWED beam
-- entries only; @width@ in [ef, 1024] is the most entries the beam may hold, allowed or not; a beam
-- with ef allowed entries ends at its ef-th allowed entry and disallowed entries are expanded like any
-- other.  The answer is the first k allowed entries.  With every id allowed it is 'graphSearchHIP's \/
-- 'graphSearchMetricSVHIP's bit for bit; with width = ef it is the allowed entries of the unfiltered beam.
graphSearchAllowHIP :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Metric -> Int -> Int
                    -> (VS.Vector Int32, VS.Vector Int32) -> Int -> VS.Vector Int32 -> Maybe (VS.Vector Word32)
                    -> Int -> Int -> Int -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphSearchAllowHIP ctx ds qs m nq kg (gids, gcount) s seeds allow k ef width = do
  ids <- VSM.new (nq * k); dist <- VSM.new (nq * k); cnt <- VSM.new nq
  let withAllow f = maybe (f nullPtr) (`VS.unsafeWith` f) allow
  VS.unsafeWith gids (\pg -> VS.unsafeWith gcount (\pc -> VS.unsafeWith seeds (\ps -> withAllow (\pa ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_search_allow_host ctx ds qs (fromIntegral kg) pg pc (fromIntegral s) ps pa (fromIntegral k) (fromIntegral ef) (fromIntegral width) (metricFlag m) 0 a b))))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | New rows into a kNN graph (rpt_graph_insert_host): @ds@ holds N = n + m rows whose LAST m are the
-- new ones (dense or CSR, under any 'Metric'), the graph is over the first n and its distances ARE
-- read.  The new rows are taken in chunks of @batch@; every row of a chunk is answered by
-- 'graphSearchHIP' with k = kg and this @ef@ over the rows visible so far (the first n and the chunks
-- before it, not its own chunk), the answer becomes the new row, and every row it names takes the new
-- id at the same distance when that is among its first kg by (distance, id).  @seeds@ is [m][s], -1
-- an unused slot; a seed may name a row of an earlier chunk.  The result (ids[N][kg], dist[N][kg],
-- count[N]) is a pure function of its inputs, bit for bit; m = 0 copies the graph.
graphInsertHIP :: Ptr Ctx -> Ptr Dataset -> Metric -> Int -> Int -> Int
               -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32) -> Int -> VS.Vector Int32 -> Int -> Int
               -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphInsertHIP ctx ds metric n m kg (gids, gdist, gcount) s seeds ef batch = do
  let total = n + m
  ids <- VSM.new (total * kg); dist <- VSM.new (total * kg); cnt <- VSM.new total
  VS.unsafeWith gids (\pg -> VS.unsafeWith gdist (\pd -> VS.unsafeWith gcount (\pc -> VS.unsafeWith seeds (\ps ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_insert_host ctx ds (fromIntegral kg) pg pd pc (fromIntegral m) (fromIntegral s) ps (fromIntegral ef) (fromIntegral batch) (metricFlag metric) 0 a b))))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | Rows out of a kNN graph (rpt_graph_delete_host): @keep@ holds the ceil(n / 32) words of the tombstone
-- bitmap 'graphSearchAllowHIP' takes, unchanged (a set bit = the row STAYS; 'Nothing' = every row
-- stays); the graph is over the n rows of @ds@ (dense or CSR, under any 'Metric') and its distances ARE
-- read.  The deleted rows are dropped; a kept row that named one becomes the first kg by (distance, id)
-- of its kept entries, at their stored distances, and the kept neighbours of its deleted neighbours,
-- at their distance to the row (one hop; 'knnGraphRefineHIP' afterwards repairs rows that end short).
-- @compact@: the survivors are renumbered densely and the result has popcount rows; otherwise n rows
-- in old ids with the deleted rows empty.  Returns the graph and newid[n] (the new id, or -1).  A pure
-- function of its inputs, bit for bit.
graphDeleteHIP :: Ptr Ctx -> Ptr Dataset -> Metric -> Int -> Int
               -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32) -> Maybe (VS.Vector Word32) -> Bool
               -> IO ((VS.Vector Int32, VS.Vector Double, VS.Vector Int32), VS.Vector Int32)
graphDeleteHIP ctx ds metric n kg (gids, gdist, gcount) keep compact = do
  ids <- VSM.new (n * kg); dist <- VSM.new (n * kg); cnt <- VSM.new n; newid <- VSM.new n
  let withKeep f = maybe (f nullPtr) (\w -> VS.unsafeWith w f) keep
  VS.unsafeWith gids (\pg -> VS.unsafeWith gdist (\pd -> VS.unsafeWith gcount (\pc -> withKeep (\pk ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (\c -> VSM.unsafeWith newid (
      c_graph_delete_host ctx ds (fromIntegral kg) pg pd pc pk (metricFlag metric) (if compact then 1 else 0) a b c)))))))) >>= check
  nid <- VS.freeze newid
  let rows = if compact then VS.length (VS.filter (>= 0) nid) else n
  i <- VS.freeze ids; d <- VS.freeze dist; c <- VS.freeze cnt
  pure ((VS.take (rows * kg) i, VS.take (rows * kg) d, VS.take rows c), nid)

-- | A kNN graph made ready for 'graphSearchHIP' (rpt_graph_prepare_host), PyNNDescent's search graph.
-- @diversify@: walking a row in stored order, a neighbour is dropped when an already kept neighbour
-- of the row is nearer to it than the point itself is (a plain <; the pair distance is the metric's
-- left fold in Double, bit-exact).  @reverse@: every point that lists i after that joins row i at the
-- distance stored there.  Row i of the answer is the first @kout@ of that set by (distance, id),
-- unused slots id -1, distance +Infinity.  The metric must be the one the graph was built under;
-- under 'MetricInner', which is no metric, @diversify@ costs recall.  The input vectors are not
-- modified.  k and kout <= 64; n = number of stored points.
graphPrepareHIP :: Ptr Ctx -> Ptr Dataset -> Metric -> Int -> Int -> Int -> Bool -> Bool
                -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphPrepareHIP ctx ds m n k kout diversify reverse (i0, d0, c0) = do
  ids <- VSM.new (n * kout); dist <- VSM.new (n * kout); cnt <- VSM.new n
  let flags = (if diversify then 1 else 0) + (if reverse then 2 else 0)
  VS.unsafeWith i0 (\pi -> VS.unsafeWith d0 (\pd -> VS.unsafeWith c0 (\pc ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_prepare_host ctx ds (fromIntegral k) pi pd pc (fromIntegral kout) (metricFlag m) flags a b)))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'graphPrepareHIP' over SVector rows under L2 (rpt_graph_prepare_csr_host): @ds@ is a CSR data set
-- ('withDeviceDataSV'), the graph e.g. 'knnGraphSVHIP's or 'knnGraphRefineSVHIP's.  The pair distances
-- of @diversify@ are metricDDL2's left fold over the dense-ified rows, so the answer is bit-equal to
-- 'graphPrepareHIP' with 'MetricL2' on the dense-ified data set and the same graph.
graphPrepareSVHIP :: Ptr Ctx -> Ptr Dataset -> Int -> Int -> Int -> Bool -> Bool
                  -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                  -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphPrepareSVHIP ctx ds n k kout diversify reverse (i0, d0, c0) = do
  ids <- VSM.new (n * kout); dist <- VSM.new (n * kout); cnt <- VSM.new n
  let flags = (if diversify then 1 else 0) + (if reverse then 2 else 0)
  VS.unsafeWith i0 (\pi -> VS.unsafeWith d0 (\pd -> VS.unsafeWith c0 (\pc ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_prepare_csr_host ctx ds (fromIntegral k) pi pd pc (fromIntegral kout) 0 flags a b)))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | 'graphPrepareSVHIP' under another distance (rpt_graph_prepare_csr_metric_host): the pair distances
-- of @diversify@ are 'MetricCosine' / 'MetricInner' over the indices both rows store, the metric the
-- graph's stored distances must have been computed under ('knnGraphMetricSVHIP',
-- 'knnGraphRefineMetricSVHIP'); 'MetricL2' gives 'graphPrepareSVHIP's bits.  Under 'MetricInner'
-- @diversify@ costs recall.
graphPrepareMetricSVHIP :: Ptr Ctx -> Ptr Dataset -> Metric -> Int -> Int -> Int -> Bool -> Bool
                        -> (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
                        -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphPrepareMetricSVHIP ctx ds m n k kout diversify reverse (i0, d0, c0) = do
  ids <- VSM.new (n * kout); dist <- VSM.new (n * kout); cnt <- VSM.new n
  let flags = (if diversify then 1 else 0) + (if reverse then 2 else 0)
  VS.unsafeWith i0 (\pi -> VS.unsafeWith d0 (\pd -> VS.unsafeWith c0 (\pc ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_prepare_csr_metric_host ctx ds (fromIntegral k) pi pd pc (fromIntegral kout) (metricFlag m) flags a b)))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | SVector rows as a CSR dataset on the device (rpt_dataset_csr_host), for the extent of the
-- callback on an existing context: the point set of an SVector forest, or a batch of SVector queries.
withDeviceDataSV :: Ptr Ctx -> Int -> V.Vector (SVector Double) -> (Ptr Dataset -> IO a) -> IO a
withDeviceDataSV ctx dim rows act = do
  let ixs = [ VU.toList ix | SV _ ix _ <- V.toList rows ]
      rowptr = VS.fromList (scanl (+) 0 (map (fromIntegral . length) ixs)) :: VS.Vector Int64
      -- (one slot of padding: the pointers of an all-empty batch stay valid)
      col = VS.fromList (map fromIntegral (concat ixs) ++ [0]) :: VS.Vector Int32
      val = VS.fromList (concat [ VU.toList vs | SV _ _ vs <- V.toList rows ] ++ [0]) :: VS.Vector Double
      acquire mk = alloca $ \pp -> mk pp >>= check >> peek pp
  bracket (acquire (\pp -> VS.unsafeWith rowptr (\pr -> VS.unsafeWith col (\pc -> VS.unsafeWith val (\pv ->
             c_dataset_csr ctx pr pc pv (fromIntegral (V.length rows)) (fromIntegral dim) 0 pp)))))
          c_dataset_free act

-- | 'recallWith metricL2 forest k' (RPTree.hs:259-282) for a batch of SVector queries over an SVector
-- forest on the device: per query the mean over the trees of
-- @|candidates tree q `intersection` true kNN| / k@, truth and intersection both on the device
-- (rpt_recall_hits_host; the division of :276-282 here, in tree order).  @refMetric@ ranks the truth
-- by the reference's own truncating metricSSL2 (RPT_KNN_METRIC_REFERENCE: the value 'recallWith
-- metricL2' of the reference itself has on SVector rows) instead of the true Euclidean distance.
-- @ds@ is the forest's point set ('withDeviceDataSV'), @ntrees@ its number of trees.
recallWithHIP :: Bool -> Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int -> Int -> Int
              -> V.Vector (SVector Double) -> IO (V.Vector Double)
recallWithHIP refMetric ctx f ds ntrees dim k qs =
  withDeviceDataSV ctx dim qs $ \qd -> do
    let nq = V.length qs
        flags = if refMetric then 16777216 else 0     -- RPT_KNN_METRIC_REFERENCE (1 << 24)
    hits <- VSM.new (max 1 (nq * ntrees)); truth <- VSM.new (max 1 (nq * k))
    VSM.unsafeWith hits (\a -> VSM.unsafeWith truth (c_recall_hits ctx f ds qd (fromIntegral k) flags a)) >>= check
    hs <- VS.freeze hits
    let rec i = sum [ fromIntegral (hs VS.! (i * ntrees + t)) / fromIntegral k | t <- [0 .. ntrees - 1] ]
                / fromIntegral ntrees
    pure (V.generate nq rec)

-- | 'knn distf k' (RPTree.hs:168-176) over an SVector forest under 'MetricCosine' / 'MetricInner', for
-- a batch of SVector queries (rpt_knn_csr_metric_host).  The dot is a LEFT fold from +0.0 over the
-- indices stored in both vectors, in ascending order, every product and sum rounded on its own: the
-- products innerSS (Internal.hs:323) adds from the right, added from the left, so that the answer is
-- the one 'knnMetricHIP' gives on the dense-ified rows whenever the stored values are finite; a stored
-- Infinity / NaN counts only where both vectors store the index.  NaN (an empty or all-zero vector
-- under 'MetricCosine') ranks last.  'MetricL2' is refused here (RPT_E_ARG): that is 'knnHIP' on the
-- SVector forest.  @ds@ is the forest's point set ('withDeviceDataSV').
knnMetricSVHIP :: Metric -> Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int -> Int
               -> V.Vector (SVector Double) -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnMetricSVHIP m ctx f ds dim k qs =
  withDeviceDataSV ctx dim qs $ \qd -> do
    let nq = V.length qs
    ids <- VSM.new (max 1 (nq * k)); dist <- VSM.new (max 1 (nq * k)); cnt <- VSM.new (max 1 nq)
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt
      (c_knn_csr_metric_host ctx f ds qd (fromIntegral k) (metricFlag m) a b))) >>= check
    (,,) <$> (VS.take (nq * k) <$> VS.freeze ids) <*> (VS.take (nq * k) <$> VS.freeze dist)
         <*> (VS.take nq <$> VS.freeze cnt)

-- | 'recallWith distf forest k' (RPTree.hs:259-282) for a batch of SVector queries over an SVector
-- forest under 'MetricCosine' / 'MetricInner' (rpt_recall_hits_csr_metric_host): the truth is the
-- exhaustive search under 'knnMetricSVHIP''s distance, by (distance, id).
recallWithMetricSVHIP :: Metric -> Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int -> Int -> Int
                      -> V.Vector (SVector Double) -> IO (V.Vector Double)
recallWithMetricSVHIP m ctx f ds ntrees dim k qs =
  withDeviceDataSV ctx dim qs $ \qd -> do
    let nq = V.length qs
    hits <- VSM.new (max 1 (nq * ntrees)); truth <- VSM.new (max 1 (nq * k))
    VSM.unsafeWith hits (\a -> VSM.unsafeWith truth
      (c_recall_hits_csr_metric ctx f ds qd (fromIntegral k) (metricFlag m) a)) >>= check
    hs <- VS.freeze hits
    let rec i = sum [ fromIntegral (hs VS.! (i * ntrees + t)) / fromIntegral k | t <- [0 .. ntrees - 1] ]
                / fromIntegral ntrees
    pure (V.generate nq rec)

-- | The vote threshold (the reference's commented-out @counts@ / @keepCounts@, RPTree.hs:464-478) for
-- every row layout and distance (rpt_knn_vote_host): of a query's candidates only the ids that at least
-- @v@ trees propose are ranked, each once, by (distance, id); the distance is the one 'knnHIP' /
-- 'knnMetricHIP' / 'knnMetricSVHIP' give for the same data and metric.  @refMetric@ (SVector rows,
-- 'MetricL2'): the reference's truncating metricSSL2.  @ds@ is the forest's point set, @qd@ the @nq@
-- queries in the same layout ('withDeviceData' / 'withDeviceDataSV').  Any number of trees and of
-- candidates, k up to 1024, batch and streamed forests.
knnVoteHIP :: Metric -> Bool -> Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Ptr Dataset -> Int -> Int -> Int
           -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnVoteHIP m refMetric ctx f ds qd nq k v = do
  let flags = metricFlag m + (if refMetric then 16777216 else 0)     -- RPT_KNN_METRIC_REFERENCE (1 << 24)
  ids <- VSM.new (max 1 (nq * k)); dist <- VSM.new (max 1 (nq * k)); cnt <- VSM.new (max 1 nq)
  VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt
    (c_knn_vote_host ctx f ds qd (fromIntegral k) (fromIntegral v) flags a b))) >>= check
  (,,) <$> (VS.take (nq * k) <$> VS.freeze ids) <*> (VS.take (nq * k) <$> VS.freeze dist)
       <*> (VS.take nq <$> VS.freeze cnt)

-- | The voted lists themselves (rpt_vote_candidates_host): @(off, ids, counts)@, the list of query i
-- is @ids[off i .. off (i + 1))@, ascending, @counts@ the number of trees that propose each id.
voteCandidatesHIP :: Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int -> Int
                  -> IO (VS.Vector Int64, VS.Vector Int32, VS.Vector Int32)
voteCandidatesHIP ctx f qd nq v = do
  off <- VSM.new (nq + 1)
  total <- alloca $ \pt -> do
    VSM.unsafeWith off (\po -> c_vote_candidates_host ctx f qd (fromIntegral v) po nullPtr nullPtr 0 pt) >>= check
    peek pt
  let m = max 1 (fromIntegral total)
  ids <- VSM.new m; cnt <- VSM.new m
  alloca $ \pt -> VSM.unsafeWith off (\po -> VSM.unsafeWith ids (\a -> VSM.unsafeWith cnt (\b ->
    c_vote_candidates_host ctx f qd (fromIntegral v) po a b total pt))) >>= check
  (,,) <$> VS.freeze off <*> (VS.take (fromIntegral total) <$> VS.freeze ids)
       <*> (VS.take (fromIntegral total) <$> VS.freeze cnt)

-- | 'knnHIP' / 'knnMetricHIP' / 'knnMetricSVHIP' among SOME of the points (rpt_knn_allow_host): @allow@ is
-- the bitmap 'graphSearchAllowHIP' takes, unchanged (ceil(n / 32) words, id i = bit @i .&. 31@ of word
-- @i `shiftR` 5@; 'Nothing' = every id).  A query's candidate list loses its disallowed entries, order
-- and duplicates kept, and is ranked by (distance, position) under the duplicate rule @dedup@ (0
-- duplicates kept, 1 each id once, 2 one entry per distance), which sees allowed entries only.  With
-- every id allowed the answer is the unfiltered one bit for bit.  @refMetric@ (SVector rows, 'MetricL2'):
-- the reference's truncating metricSSL2.  @ds@ is the forest's point set, @qd@ the @nq@ queries in the
-- same layout.  The ids seed 'graphSearchAllowHIP' under the same bitmap (@dedup@ = 1).
knnAllowHIP :: Metric -> Bool -> Int -> Maybe (VS.Vector Word32) -> Ptr Ctx -> Ptr Forest -> Ptr Dataset
            -> Ptr Dataset -> Int -> Int -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnAllowHIP m refMetric dedup allow ctx f ds qd nq k = do
  let flags = fromIntegral dedup + metricFlag m + (if refMetric then 16777216 else 0)   -- RPT_KNN_METRIC_REFERENCE
      withAllow g = maybe (g nullPtr) (`VS.unsafeWith` g) allow
  ids <- VSM.new (max 1 (nq * k)); dist <- VSM.new (max 1 (nq * k)); cnt <- VSM.new (max 1 nq)
  withAllow (\pa -> VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt
    (c_knn_allow_host ctx f ds qd pa (fromIntegral k) flags a b)))) >>= check
  (,,) <$> (VS.take (nq * k) <$> VS.freeze ids) <*> (VS.take (nq * k) <$> VS.freeze dist)
       <*> (VS.take nq <$> VS.freeze cnt)

-- | The exhaustive kNN among the allowed rows (rpt_brute_knn_allow_host): the k best allowed rows by
-- (distance, id), NaN last, unused slots id -1 and distance +Infinity.
bruteKnnAllowHIP :: Metric -> Bool -> Maybe (VS.Vector Word32) -> Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Int -> Int
                 -> IO (VS.Vector Int32, VS.Vector Double)
bruteKnnAllowHIP m refMetric allow ctx ds qd nq k = do
  let flags = metricFlag m + (if refMetric then 16777216 else 0)
      withAllow g = maybe (g nullPtr) (`VS.unsafeWith` g) allow
  ids <- VSM.new (max 1 (nq * k)); dist <- VSM.new (max 1 (nq * k))
  withAllow (\pa -> VSM.unsafeWith ids (\a -> VSM.unsafeWith dist
    (c_brute_knn_allow_host ctx ds qd pa (fromIntegral k) flags a))) >>= check
  (,) <$> (VS.take (nq * k) <$> VS.freeze ids) <*> (VS.take (nq * k) <$> VS.freeze dist)

-- | 'recallWith' (RPTree.hs:259-282) with the truth taken among the allowed rows
-- (rpt_recall_hits_allow_host): per query the mean over the trees of
-- |candidates(tree, q) `intersect` the k nearest allowed rows| / k.
recallWithAllowHIP :: Metric -> Bool -> Maybe (VS.Vector Word32) -> Ptr Ctx -> Ptr Forest -> Ptr Dataset
                   -> Ptr Dataset -> Int -> Int -> Int -> IO (V.Vector Double)
recallWithAllowHIP m refMetric allow ctx f ds qd nq ntrees k = do
  let flags = metricFlag m + (if refMetric then 16777216 else 0)
      withAllow g = maybe (g nullPtr) (`VS.unsafeWith` g) allow
  hits <- VSM.new (max 1 (nq * ntrees)); truth <- VSM.new (max 1 (nq * k))
  withAllow (\pa -> VSM.unsafeWith hits (\a -> VSM.unsafeWith truth
    (c_recall_hits_allow_host ctx f ds qd pa (fromIntegral k) flags a))) >>= check
  hs <- VS.freeze hits
  let rec i = sum [ fromIntegral (hs VS.! (i * ntrees + t)) / fromIntegral k | t <- [0 .. ntrees - 1] ]
              / fromIntegral ntrees
  pure (V.generate nq rec)

-- ---- allow-lists per query group (rpt_*_allow_group_*) ----
-- A grouped allow-list is @(allow, g, group)@: @allow@ holds @g@ bitmaps of ceil(n \/ 32) words each, one
-- after the other (row stride ceil(n \/ 32)); @group@ holds one entry per query, query q being answered
-- under bitmap @group ! q@, -1 = every id.  The answer of query q is the single-bitmap function's for that
-- query under its bitmap, bit for bit.  The host variants refuse a group entry outside [-1, g).

-- | the two arrays of a grouped allow-list as pointers (an empty @allow@ is the null pointer)
withGroups :: VS.Vector Word32 -> VS.Vector Int32 -> (Ptr Word32 -> Ptr Int32 -> IO a) -> IO a
withGroups allow group f
  | VS.null allow = VS.unsafeWith group (f nullPtr)
  | otherwise = VS.unsafeWith allow (\pa -> VS.unsafeWith group (f pa))

-- | 'graphSearchAllowHIP' with a bitmap per query group (rpt_graph_search_allow_group_host).
graphSearchAllowGroupHIP :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Metric -> Int -> Int
                         -> (VS.Vector Int32, VS.Vector Int32) -> Int -> VS.Vector Int32
                         -> VS.Vector Word32 -> Int -> VS.Vector Int32
                         -> Int -> Int -> Int -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
graphSearchAllowGroupHIP ctx ds qs m nq kg (gids, gcount) s seeds allow g group k ef width = do
  ids <- VSM.new (nq * k); dist <- VSM.new (nq * k); cnt <- VSM.new nq
  VS.unsafeWith gids (\pg -> VS.unsafeWith gcount (\pc -> VS.unsafeWith seeds (\ps -> withGroups allow group (\pa pgr ->
    VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt (
      c_graph_search_allow_group_host ctx ds qs (fromIntegral kg) pg pc (fromIntegral s) ps pa (fromIntegral g) pgr (fromIntegral k) (fromIntegral ef) (fromIntegral width) (metricFlag m) 0 a b))))))) >>= check
  (,,) <$> VS.freeze ids <*> VS.freeze dist <*> VS.freeze cnt

-- | The same on device arrays (rpt_graph_search_allow_group_dev): every pointer is device memory, nothing
-- is validated (a group entry outside [-1, g) means no id is allowed), the call is enqueued only.
graphSearchAllowGroupDevHIP :: Ptr Ctx -> Ptr Dataset -> Ptr Dataset -> Metric -> Int -> Ptr Int32 -> Ptr Int32 -> Int
                            -> Ptr Int32 -> Ptr Word32 -> Int -> Ptr Int32 -> Int -> Int -> Int
                            -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO ()
graphSearchAllowGroupDevHIP ctx ds qs m kg pg pc s ps pa g pgr k ef width a b c =
  c_graph_search_allow_group_dev ctx ds qs (fromIntegral kg) pg pc (fromIntegral s) ps pa (fromIntegral g) pgr (fromIntegral k) (fromIntegral ef) (fromIntegral width) (metricFlag m) 0 a b c >>= check

-- | 'knnAllowHIP' with a bitmap per query group (rpt_knn_allow_group_host).
knnAllowGroupHIP :: Metric -> Bool -> Int -> VS.Vector Word32 -> Int -> VS.Vector Int32 -> Ptr Ctx -> Ptr Forest
                 -> Ptr Dataset -> Ptr Dataset -> Int -> Int -> IO (VS.Vector Int32, VS.Vector Double, VS.Vector Int32)
knnAllowGroupHIP m refMetric dedup allow g group ctx f ds qd nq k = do
  let flags = fromIntegral dedup + metricFlag m + (if refMetric then 16777216 else 0)   -- RPT_KNN_METRIC_REFERENCE
  ids <- VSM.new (max 1 (nq * k)); dist <- VSM.new (max 1 (nq * k)); cnt <- VSM.new (max 1 nq)
  withGroups allow group (\pa pgr -> VSM.unsafeWith ids (\a -> VSM.unsafeWith dist (\b -> VSM.unsafeWith cnt
    (c_knn_allow_group_host ctx f ds qd pa (fromIntegral g) pgr (fromIntegral k) flags a b)))) >>= check
  (,,) <$> (VS.take (nq * k) <$> VS.freeze ids) <*> (VS.take (nq * k) <$> VS.freeze dist)
       <*> (VS.take nq <$> VS.freeze cnt)

-- | The same on device arrays (rpt_knn_allow_group_dev); returns synchronised.
knnAllowGroupDevHIP :: Metric -> Bool -> Int -> Ptr Word32 -> Int -> Ptr Int32 -> Ptr Ctx -> Ptr Forest -> Ptr Dataset
                    -> Ptr Dataset -> Int -> Ptr Int32 -> Ptr Double -> Ptr Int32 -> IO ()
knnAllowGroupDevHIP m refMetric dedup pa g pgr ctx f ds qd k a b c =
  c_knn_allow_group_dev ctx f ds qd pa (fromIntegral g) pgr (fromIntegral k)
    (fromIntegral dedup + metricFlag m + (if refMetric then 16777216 else 0)) a b c >>= check

-- | The allowed lists themselves, every query under its own bitmap (rpt_allow_group_candidates_host):
-- (off[nq+1], ids).
allowGroupCandidatesHIP :: VS.Vector Word32 -> Int -> VS.Vector Int32 -> Ptr Ctx -> Ptr Forest -> Ptr Dataset -> Int
                        -> IO (VS.Vector Int64, VS.Vector Int32)
allowGroupCandidatesHIP allow g group _ctx f qd nq = do
  off <- VSM.new (nq + 1)
  total <- withGroups allow group (\pa pgr -> VSM.unsafeWith off (\po -> alloca (\pt -> do
    c_allow_group_candidates_host _ctx f qd pa (fromIntegral g) pgr po nullPtr 0 pt >>= check
    peek pt)))
  ids <- VSM.new (max 1 (fromIntegral total))
  withGroups allow group (\pa pgr -> VSM.unsafeWith off (\po -> VSM.unsafeWith ids (\pi -> alloca (\pt ->
    c_allow_group_candidates_host _ctx f qd pa (fromIntegral g) pgr po pi total pt)))) >>= check
  (,) <$> VS.freeze off <*> (VS.take (fromIntegral total) <$> VS.freeze ids)

-- | 'bruteKnnAllowHIP' with a bitmap per query group (rpt_brute_knn_allow_group_host).
bruteKnnAllowGroupHIP :: Metric -> Bool -> VS.Vector Word32 -> Int -> VS.Vector Int32 -> Ptr Ctx -> Ptr Dataset
                      -> Ptr Dataset -> Int -> Int -> IO (VS.Vector Int32, VS.Vector Double)
bruteKnnAllowGroupHIP m refMetric allow g group ctx ds qd nq k = do
  let flags = metricFlag m + (if refMetric then 16777216 else 0)
  ids <- VSM.new (max 1 (nq * k)); dist <- VSM.new (max 1 (nq * k))
  withGroups allow group (\pa pgr -> VSM.unsafeWith ids (\a -> VSM.unsafeWith dist
    (c_brute_knn_allow_group_host ctx ds qd pa (fromIntegral g) pgr (fromIntegral k) flags a))) >>= check
  (,) <$> (VS.take (nq * k) <$> VS.freeze ids) <*> (VS.take (nq * k) <$> VS.freeze dist)

-- | The same on device arrays (rpt_brute_knn_allow_group_dev); returns synchronised.
bruteKnnAllowGroupDevHIP :: Metric -> Bool -> Ptr Word32 -> Int -> Ptr Int32 -> Ptr Ctx -> Ptr Dataset -> Ptr Dataset
                         -> Int -> Ptr Int32 -> Ptr Double -> IO ()
bruteKnnAllowGroupDevHIP m refMetric pa g pgr ctx ds qd k a b =
  c_brute_knn_allow_group_dev ctx ds qd pa (fromIntegral g) pgr (fromIntegral k)
    (metricFlag m + (if refMetric then 16777216 else 0)) a b >>= check

-- | 'recallWithAllowHIP' with a bitmap per query group (rpt_recall_hits_allow_group_host).
recallWithAllowGroupHIP :: Metric -> Bool -> VS.Vector Word32 -> Int -> VS.Vector Int32 -> Ptr Ctx -> Ptr Forest
                        -> Ptr Dataset -> Ptr Dataset -> Int -> Int -> Int -> IO (V.Vector Double)
recallWithAllowGroupHIP m refMetric allow g group ctx f ds qd nq ntrees k = do
  let flags = metricFlag m + (if refMetric then 16777216 else 0)
  hits <- VSM.new (max 1 (nq * ntrees)); truth <- VSM.new (max 1 (nq * k))
  withGroups allow group (\pa pgr -> VSM.unsafeWith hits (\a -> VSM.unsafeWith truth
    (c_recall_hits_allow_group_host ctx f ds qd pa (fromIntegral g) pgr (fromIntegral k) flags a))) >>= check
  hs <- VS.freeze hits
  let rec i = sum [ fromIntegral (hs VS.! (i * ntrees + t)) / fromIntegral k | t <- [0 .. ntrees - 1] ]
              / fromIntegral ntrees
  pure (V.generate nq rec)
