// api.hip — C-ABI entry points (include/rptree_hip.h): contexts, datasets, topology,
// forest accessors and the thin wrappers around the kernels in project/split/knn.hip.
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <new>

#include "common.h"

namespace rpt {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int32_t fail(int32_t code, const std::string& msg) {
  g_err = msg;
  return code;
}

// ---- caching device allocator ------------------------------------------------------------
namespace {
struct Block {
  void* p;
  size_t bytes;
};
std::mutex g_pool_mu;
std::map<int, std::vector<Block>> g_pool_free;            // device -> cached blocks
std::map<void*, std::pair<int, size_t>> g_pool_live;      // ptr -> (device, bytes)
struct Pending {
  void* p;
  size_t bytes;
  int dev;
  hipStream_t stream;
};
std::vector<Pending> g_pool_pending;                      // freed, stream not yet synchronised
thread_local hipStream_t tl_stream = nullptr;
size_t round_bytes(size_t b) {
  const size_t g = b >= ((size_t)1 << 20) ? ((size_t)2 << 20) : 256;
  return (b + g - 1) / g * g;
}
}  // namespace

static hipError_t dev_alloc_impl(void** p, size_t bytes);
// allocator debugging aids, read from the environment ONCE per process (library load):
// RPT_NO_POOL = plain hipMalloc/hipFree, RPT_POOL_POISON=<byte> = fill every block handed out
// (finds reads of uninitialised memory: tests/test_gpu_pool_poison.py); RPT_NO_POOL wins
static const bool g_no_pool = getenv("RPT_NO_POOL") != nullptr;
static const int g_poison = getenv("RPT_POOL_POISON") ? atoi(getenv("RPT_POOL_POISON")) : -1;
hipError_t dev_alloc(void** p, size_t bytes) {
  if (g_no_pool) return hipMalloc(p, bytes ? bytes : 1);
  const hipError_t e = dev_alloc_impl(p, bytes);
  if (e == hipSuccess && g_poison >= 0) {
    // the whole block that is handed out, not just the request: a block is rounded up and a
    // recycled one may be a quarter larger, and the "+ 16" slack reads land in that tail
    size_t block = bytes ? bytes : 1;
    {
      std::lock_guard<std::mutex> lk(g_pool_mu);
      auto it = g_pool_live.find(*p);
      if (it != g_pool_live.end()) block = it->second.second;
    }
    (void)hipDeviceSynchronize();
    (void)hipMemset(*p, g_poison, block);
    (void)hipDeviceSynchronize();
  }
  return e;
}
static int dev_pool_poison() { return g_no_pool ? -1 : g_poison; }  // rpt_debug_pool_probe
static hipError_t dev_alloc_impl(void** p, size_t bytes) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const size_t want = round_bytes(bytes ? bytes : 1);
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    std::vector<Block>& fl = g_pool_free[dev];
    int best = -1;
    for (int i = 0; i < (int)fl.size(); ++i)
      if (fl[i].bytes >= want && fl[i].bytes <= want + want / 4 &&
          (best < 0 || fl[i].bytes < fl[best].bytes))
        best = i;
    if (best >= 0) {
      *p = fl[best].p;
      g_pool_live[*p] = {dev, fl[best].bytes};
      fl.erase(fl.begin() + best);
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(p, want);
  if (e != hipSuccess) {  // give the cache back to the driver and retry once
    dev_trim();
    e = hipMalloc(p, want);
  }
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_live[*p] = {dev, want};
  }
  return e;
}

void dev_free(void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  auto it = g_pool_live.find(p);
  if (it == g_pool_live.end()) {
    (void)hipFree(p);
    return;
  }
  g_pool_pending.push_back(Pending{p, it->second.second, it->second.first, tl_stream});
  g_pool_live.erase(it);
}

void dev_set_stream(hipStream_t s) { tl_stream = s; }

hipError_t stream_sync(hipStream_t s) {
  const hipError_t e = hipStreamSynchronize(s);
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (size_t i = 0; i < g_pool_pending.size();) {
    if (g_pool_pending[i].stream == s) {
      g_pool_free[g_pool_pending[i].dev].push_back(Block{g_pool_pending[i].p, g_pool_pending[i].bytes});
      g_pool_pending[i] = g_pool_pending.back();
      g_pool_pending.pop_back();
    } else {
      ++i;
    }
  }
  return e;
}

constexpr size_t kPinBytes = 8u << 20;

void* pin_alloc(rpt_ctx* ctx, size_t bytes) {
  bytes = (bytes + 63) & ~(size_t)63;
  if (bytes > kPinBytes) return nullptr;
  if (!ctx->pin) {
    if (hipHostMalloc((void**)&ctx->pin, kPinBytes, hipHostMallocDefault) != hipSuccess) {
      ctx->pin = nullptr;
      return nullptr;
    }
    ctx->pin_cap = kPinBytes;
    ctx->pin_off = 0;
  }
  if (ctx->pin_off + bytes > ctx->pin_cap) (void)ctx_sync(ctx);  // in-flight copies drain first
  void* r = ctx->pin + ctx->pin_off;
  ctx->pin_off += bytes;
  return r;
}

int32_t upload_async(rpt_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
  if (bytes == 0) return RPT_OK;
  void* stage = pin_alloc(ctx, bytes);
  if (!stage) {
    RPT_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    RPT_HIP(stream_sync(ctx->stream));
    return RPT_OK;
  }
  std::memcpy(stage, src_host, bytes);
  RPT_HIP(hipMemcpyAsync(dst_dev, stage, bytes, hipMemcpyHostToDevice, ctx->stream));
  return RPT_OK;
}

hipError_t ctx_sync(rpt_ctx* ctx) {
  const hipError_t e = stream_sync(ctx->stream);
  ctx->pin_off = 0;
  return e;
}

// Returns the cache of the CURRENT device to the driver: after hipDeviceSynchronize every stream
// of that device has drained, so its cached blocks and its blocks waiting for a stream
// synchronisation are all idle.  Other devices (other contexts, possibly driven by other host
// threads: rpt_comm_init) are not touched — their streams were not synchronised here.
void dev_trim() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceSynchronize();
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (size_t i = 0; i < g_pool_pending.size();) {
    if (g_pool_pending[i].dev == dev) {
      (void)hipFree(g_pool_pending[i].p);
      g_pool_pending[i] = g_pool_pending.back();
      g_pool_pending.pop_back();
    } else {
      ++i;
    }
  }
  auto it = g_pool_free.find(dev);
  if (it != g_pool_free.end()) {
    for (Block& b : it->second) (void)hipFree(b.p);
    it->second.clear();
  }
}

void enumerate_topology(int64_t N, int32_t L, int32_t min_leaf, std::vector<Node>& out) {
  // iterative DFS, pre-order (left before right): Internal.hs:289 leaf test, :495,503 halves
  struct Item { int32_t level; int64_t heap, off, n; };
  std::vector<Item> stack;
  stack.push_back({0, 0, 0, N});
  while (!stack.empty()) {
    Item it = stack.back();
    stack.pop_back();
    bool leaf = is_leaf(it.level, it.n, L, min_leaf);
    out.push_back({it.level, it.heap, it.off, it.n, leaf});
    if (!leaf) {
      int64_t nh = it.n / 2;
      stack.push_back({it.level + 1, 2 * it.heap + 2, it.off + nh, it.n - nh});
      stack.push_back({it.level + 1, 2 * it.heap + 1, it.off, nh});
    }
  }
}

}  // namespace rpt

using namespace rpt;

static void prof_resolve(rpt_ctx* ctx);

// ---- context options ---------------------------------------------------------------------
namespace {
struct OptDesc {
  const char* name;
  int64_t rpt_options::*field;
};
const OptDesc kOptions[] = {
    {"no_stream", &rpt_options::no_stream},
    {"stream_maxnodes", &rpt_options::stream_maxnodes},
    {"stream_minper", &rpt_options::stream_minper},
    {"no_wmid", &rpt_options::no_wmid},
    {"no_midselect", &rpt_options::no_midselect},
    {"stream_big_node", &rpt_options::stream_big_node},
    {"no_wsub", &rpt_options::no_wsub},
    {"no_wsort", &rpt_options::no_wsort},
    {"no_wpack", &rpt_options::no_wpack},
    {"no_csub", &rpt_options::no_csub},
    {"no_codes", &rpt_options::no_codes},
    {"no_pcodes", &rpt_options::no_pcodes},
    {"proj_narrow", &rpt_options::proj_narrow},
    {"proj_bf16_f32", &rpt_options::proj_bf16_f32},
    {"proj_bf16_terms", &rpt_options::proj_bf16_terms},
    {"proj_bf16_codes", &rpt_options::proj_bf16_codes},
    {"proj_csr_nodense", &rpt_options::proj_csr_nodense},
    {"knn_wave", &rpt_options::knn_wave},
    {"knn_kp", &rpt_options::knn_kp},
    {"knn_no_pre32", &rpt_options::knn_no_pre32},
    {"knn_no_pre16", &rpt_options::knn_no_pre16},
    {"knn_kp16", &rpt_options::knn_kp16},
    {"knn_no_pre8", &rpt_options::knn_no_pre8},
    {"knn_kp8", &rpt_options::knn_kp8},
    {"knn_l2_exact", &rpt_options::knn_l2_exact},
    {"knn_metric_exact", &rpt_options::knn_metric_exact},
    {"knn_csr_pre32", &rpt_options::knn_csr_pre32},
    {"knn_general", &rpt_options::knn_general},
    {"knn_vote_lds", &rpt_options::knn_vote_lds},
    {"knn_vote_slice", &rpt_options::knn_vote_slice},
    {"knn_allow_slice", &rpt_options::knn_allow_slice},
    {"knn_allow_group_budget", &rpt_options::knn_allow_group_budget},
    {"graph_general", &rpt_options::graph_general},
    {"graph_refine_general", &rpt_options::graph_refine_general},
    {"graph_delete_general", &rpt_options::graph_delete_general},
    {"graph_csr_masked", &rpt_options::graph_csr_masked},
    {"graph_search_nofilter", &rpt_options::graph_search_nofilter},
    {"graph_search_csr_stream", &rpt_options::graph_search_csr_stream},
    {"graph_prepare_csr_resident", &rpt_options::graph_prepare_csr_resident},
    {"knn_shard_old", &rpt_options::knn_shard_old},
    {"brute_csr_tile", &rpt_options::brute_csr_tile},
    {"comm_force_exchange", &rpt_options::comm_force_exchange},
    {"comm_inject_failure", &rpt_options::comm_inject_failure},
    {"comm_timeout_ms", &rpt_options::comm_timeout_ms},
    {"comm_stall_test", &rpt_options::comm_stall_test},
    {"tune0", &rpt_options::tune0},
    {"tune1", &rpt_options::tune1},
    {"tune2", &rpt_options::tune2},
    {"tune3", &rpt_options::tune3},
    {"debug_host", &rpt_options::debug_host},
    {"debug_stamps", &rpt_options::debug_stamps},
};
const OptDesc* find_option(const char* name) {
  if (!name) return nullptr;
  for (const OptDesc& o : kOptions)
    if (std::strcmp(o.name, name) == 0) return &o;
  return nullptr;
}
// RPT_<NAME> in the environment seeds an option when a context is created (a variable that is
// set but holds no number means 1); nothing reads the environment after that.
void options_from_env(rpt_options& opt) {
  for (const OptDesc& o : kOptions) {
    std::string env = "RPT_";
    for (const char* c = o.name; *c; ++c) env += (char)std::toupper((unsigned char)*c);
    if (const char* v = getenv(env.c_str())) {
      char* end = nullptr;
      const long long x = std::strtoll(v, &end, 10);
      opt.*(o.field) = (end && end != v) ? (int64_t)x : 1;
    }
  }
}

// No exception leaves the library (the header's promise): the host-side planners use
// std::vector / std::string / std::map, whose failures would otherwise terminate the caller.
template <class F>
int32_t guarded(F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    try {
      return fail(RPT_E_NOMEM, "out of host memory");
    } catch (...) {
      return RPT_E_NOMEM;
    }
  } catch (const std::exception& e) {
    try {
      return fail(RPT_E_INTERNAL, std::string("internal error: ") + e.what());
    } catch (...) {
      return RPT_E_INTERNAL;
    }
  } catch (...) {
    return RPT_E_INTERNAL;
  }
}
}  // namespace

extern "C" {

int32_t rpt_abi_version(void) { return RPT_ABI_VERSION; }
const char* rpt_last_error(void) { return g_err.c_str(); }

int32_t rpt_device_count(int32_t* count) {
  return guarded([&]() -> int32_t {
    RPT_ARG(count, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
      *count = 0;
      return fail(RPT_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = c;
    return RPT_OK;
  });
}

int32_t rpt_ctx_create(int32_t device, rpt_ctx** out) {
  return guarded([&]() -> int32_t {
    RPT_ARG(out, "out is NULL");
    *out = nullptr;
    int c = 0;
    RPT_HIP(hipGetDeviceCount(&c));
    if (c <= 0) return fail(RPT_E_HIP, "no HIP device available (there is no CPU fallback)");
    RPT_ARG(device >= 0 && device < c, "device index out of range");
    RPT_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    RPT_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return fail(RPT_E_UNSUPPORTED,
                  std::string("this library is built for gfx950 only, device is ") +
                      prop.gcnArchName);
    rpt_ctx* ctx = new (std::nothrow) rpt_ctx();
    if (!ctx) return fail(RPT_E_NOMEM, "out of host memory");
    ctx->device = device;
    options_from_env(ctx->opt);
    ctx->n_cu = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete ctx;
      return fail(RPT_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = ctx;
    return RPT_OK;
  });
}

int32_t rpt_ctx_destroy(rpt_ctx* ctx) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    if (!ctx) return RPT_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) {
      (void)stream_sync(ctx->stream);
      prof_resolve(ctx);
      for (hipEvent_t e : ctx->prof_events) (void)hipEventDestroy(e);
      ctx->prof_events.clear();
      (void)hipStreamDestroy(ctx->stream);
    }
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    if (ctx->metric_unc_dev) dev_free(ctx->metric_unc_dev);
    if (ctx->refine_state_dev) dev_free(ctx->refine_state_dev);
    if (ctx->search_state_dev) dev_free(ctx->search_state_dev);
    if (ctx->prepare_state_dev) dev_free(ctx->prepare_state_dev);
    if (ctx->insert_state_dev) dev_free(ctx->insert_state_dev);
    if (ctx->delete_state_dev) dev_free(ctx->delete_state_dev);
    dev_trim();
    delete ctx;
    return RPT_OK;
  });
}

int32_t rpt_ctx_sync(rpt_ctx* ctx) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx, "ctx is NULL");
    RPT_HIP(hipSetDevice(ctx->device));
    RPT_HIP(stream_sync(ctx->stream));
    return RPT_OK;
  });
}

int32_t rpt_ctx_trim(rpt_ctx* ctx) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx, "ctx is NULL");
    RPT_HIP(hipSetDevice(ctx->device));
    RPT_HIP(stream_sync(ctx->stream));
    dev_trim();
    return RPT_OK;
  });
}

int32_t rpt_debug_pool_probe(rpt_ctx* ctx, int64_t nbytes, uint8_t* out_host, int32_t* poison) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && out_host && poison, "NULL argument");
    RPT_ARG(nbytes > 0, "nbytes must be positive");
    RPT_HIP(hipSetDevice(ctx->device));
    *poison = dev_pool_poison();
    void* p = nullptr;
    RPT_HIP(dev_alloc(&p, (size_t)nbytes));
    const hipError_t e = hipMemcpyAsync(out_host, p, (size_t)nbytes, hipMemcpyDeviceToHost, ctx->stream);
    dev_free(p);
    RPT_HIP(e);
    RPT_HIP(stream_sync(ctx->stream));   // the copy has landed; the block is reusable from here
    return RPT_OK;
  });
}

int32_t rpt_ctx_stream(rpt_ctx* ctx, void** hip_stream) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && hip_stream, "NULL argument");
    *hip_stream = (void*)ctx->stream;
    return RPT_OK;
  });
}

int32_t rpt_ctx_set_option(rpt_ctx* ctx, const char* name, int64_t value) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && name, "NULL argument");
    const OptDesc* o = find_option(name);
    if (!o) return fail(RPT_E_ARG, std::string("unknown option: ") + name);
    ctx->opt.*(o->field) = value;
    return RPT_OK;
  });
}

int32_t rpt_ctx_get_option(rpt_ctx* ctx, const char* name, int64_t* value) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && name && value, "NULL argument");
    const OptDesc* o = find_option(name);
    if (!o) return fail(RPT_E_ARG, std::string("unknown option: ") + name);
    *value = ctx->opt.*(o->field);
    return RPT_OK;
  });
}

// ---- kernel timing ----------------------------------------------------------------------
static void prof_resolve(rpt_ctx* ctx) {
  for (rpt_prof_span& sp : ctx->spans) {
    float ms = 0.f;
    if (hipEventSynchronize(sp.b) == hipSuccess &&
        hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
      ctx->prof_ms[sp.which] += (double)ms;
      ctx->prof_n[sp.which] += 1;
      if (sp.which == RPT_PROF_PROJECT_WIDE) {  // the wide launches are projection launches too
        ctx->prof_ms[RPT_PROF_PROJECT] += (double)ms;
        ctx->prof_n[RPT_PROF_PROJECT] += 1;
      }
    }
    if (hipEventQuery(sp.b) == hipSuccess) {  // both have completed: free for the next span
      ctx->prof_events.push_back(sp.a);
      ctx->prof_events.push_back(sp.b);
    } else {
      (void)hipGetLastError();
      (void)hipEventDestroy(sp.a);
      (void)hipEventDestroy(sp.b);
    }
  }
  ctx->spans.clear();
}

int32_t rpt_prof_enable(rpt_ctx* ctx, int32_t on) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx, "ctx is NULL");
    ctx->prof = on != 0;
    return RPT_OK;
  });
}

int32_t rpt_prof_reset(rpt_ctx* ctx) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx, "ctx is NULL");
    RPT_HIP(hipSetDevice(ctx->device));
    prof_resolve(ctx);
    for (int i = 0; i < RPT_PROF_CLASSES; ++i) {
      ctx->prof_ms[i] = 0;
      ctx->prof_n[i] = 0;
    }
    return RPT_OK;
  });
}

int32_t rpt_prof_get(rpt_ctx* ctx, int32_t which, double* total_ms, int64_t* launches) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && total_ms && launches, "NULL argument");
    RPT_ARG(which >= 0 && which < RPT_PROF_CLASSES && which != 7, "unknown kernel class");
    RPT_HIP(hipSetDevice(ctx->device));
    RPT_HIP(stream_sync(ctx->stream));
    prof_resolve(ctx);
    *total_ms = ctx->prof_ms[which];
    *launches = ctx->prof_n[which];
    return RPT_OK;
  });
}

// ---- datasets -------------------------------------------------------------------------
static int32_t check_dtype(int32_t dt) {
  RPT_ARG(dt == RPT_F64 || dt == RPT_F32 || dt == RPT_BF16, "unknown dtype");
  return RPT_OK;
}

int32_t rpt_dataset_dense_host(rpt_ctx* ctx, const void* X_host, int64_t n, int32_t d,
                               int32_t dtype, rpt_dataset** out) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && out, "NULL argument");
    *out = nullptr;
    RPT_TRY(check_dtype(dtype));
    RPT_ARG(n >= 0 && d >= 1, "n must be >= 0 and d >= 1");
    RPT_ARG(n < (int64_t)0x7fffffff, "n must fit int32 point ids");
    RPT_ARG(n == 0 || X_host, "X_host is NULL");
    RPT_HIP(hipSetDevice(ctx->device));
    rpt_dataset* ds = new (std::nothrow) rpt_dataset();
    if (!ds) return fail(RPT_E_NOMEM, "out of host memory");
    ds->ctx = ctx;
    ds->n = n;
    ds->d = d;
    ds->dtype = dtype;
    ds->owns = true;
    size_t bytes = (size_t)n * d * dtype_size(dtype);
    hipError_t e = dev_alloc(&ds->X, bytes ? bytes : 16);
    if (e != hipSuccess) {
      delete ds;
      return fail(RPT_E_NOMEM, std::string("hipMalloc dataset: ") + hipGetErrorString(e));
    }
    if (bytes) {
      e = hipMemcpyAsync(ds->X, X_host, bytes, hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess) e = stream_sync(ctx->stream);
      if (e != hipSuccess) {
        dev_free(ds->X);
        delete ds;
        return fail(RPT_E_HIP, std::string("H2D copy: ") + hipGetErrorString(e));
      }
    }
    *out = ds;
    return RPT_OK;
  });
}

int32_t rpt_dataset_dense_dev(rpt_ctx* ctx, const void* X_dev, int64_t n, int32_t d,
                              int32_t dtype, rpt_dataset** out) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && out, "NULL argument");
    *out = nullptr;
    RPT_TRY(check_dtype(dtype));
    RPT_ARG(n >= 0 && d >= 1, "n must be >= 0 and d >= 1");
    RPT_ARG(n < (int64_t)0x7fffffff, "n must fit int32 point ids");
    RPT_ARG(n == 0 || X_dev, "X_dev is NULL");
    RPT_ARG(((uintptr_t)X_dev & 15) == 0, "X_dev must be 16-byte aligned");
    rpt_dataset* ds = new (std::nothrow) rpt_dataset();
    if (!ds) return fail(RPT_E_NOMEM, "out of host memory");
    ds->ctx = ctx;
    ds->n = n;
    ds->d = d;
    ds->dtype = dtype;
    ds->owns = false;
    ds->X = const_cast<void*>(X_dev);
    *out = ds;
    return RPT_OK;
  });
}

int32_t rpt_dataset_csr_host(rpt_ctx* ctx, const int64_t* rowptr_host, const int32_t* col_host,
                             const void* val_host, int64_t n, int32_t d, int32_t dtype,
                             rpt_dataset** out) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && out, "NULL argument");
    *out = nullptr;
    RPT_TRY(check_dtype(dtype));
    RPT_ARG(dtype != RPT_BF16, "CSR datasets are f64 or f32");
    RPT_ARG(n >= 0 && d >= 1 && rowptr_host, "bad CSR arguments");
    RPT_ARG(n < (int64_t)0x7fffffff, "n must fit int32 point ids");
    RPT_ARG(rowptr_host[0] == 0, "rowptr[0] must be 0");
    int64_t nnz = rowptr_host[n];
    RPT_ARG(nnz >= 0, "rowptr[n] negative");
    for (int64_t i = 0; i < n; ++i)
      RPT_ARG(rowptr_host[i + 1] >= rowptr_host[i], "rowptr must be non-decreasing");
    RPT_ARG(nnz == 0 || (col_host && val_host), "col/val NULL");
    // SVector invariants (Internal.hs:99-105) are unchecked in the reference; the kernels
    // index a dense hyperplane by col, so col < d is validated here to keep HBM accesses in
    // bounds.
    for (int64_t j = 0; j < nnz; ++j)
      RPT_ARG(col_host[j] >= 0 && col_host[j] < d, "CSR column index out of range");
    RPT_HIP(hipSetDevice(ctx->device));
    rpt_dataset* ds = new (std::nothrow) rpt_dataset();
    if (!ds) return fail(RPT_E_NOMEM, "out of host memory");
    ds->ctx = ctx;
    ds->n = n;
    ds->d = d;
    ds->dtype = dtype;
    ds->csr = true;
    ds->owns = true;
    ds->nnz = nnz;
    size_t vb = (size_t)nnz * dtype_size(dtype);
    hipError_t e = dev_alloc((void**)&ds->rowptr, (size_t)(n + 1) * 8);
    if (e == hipSuccess) e = dev_alloc((void**)&ds->col, nnz ? (size_t)nnz * 4 : 16);
    if (e == hipSuccess) e = dev_alloc(&ds->val, vb ? vb : 16);
    if (e == hipSuccess)
      e = hipMemcpyAsync(ds->rowptr, rowptr_host, (size_t)(n + 1) * 8, hipMemcpyHostToDevice,
                         ctx->stream);
    if (e == hipSuccess && nnz)
      e = hipMemcpyAsync(ds->col, col_host, (size_t)nnz * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && nnz)
      e = hipMemcpyAsync(ds->val, val_host, vb, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = stream_sync(ctx->stream);
    if (e != hipSuccess) {
      rpt_dataset_free(ds);
      return fail(RPT_E_HIP, std::string("CSR upload: ") + hipGetErrorString(e));
    }
    *out = ds;
    return RPT_OK;
  });
}

int32_t rpt_dataset_csr_dev(rpt_ctx* ctx, const int64_t* rowptr_dev, const int32_t* col_dev,
                            const void* val_dev, int64_t n, int32_t d, int32_t dtype, int64_t nnz,
                            rpt_dataset** out) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && out, "NULL argument");
    *out = nullptr;
    RPT_TRY(check_dtype(dtype));
    RPT_ARG(dtype != RPT_BF16, "CSR datasets are f64 or f32");
    RPT_ARG(n >= 0 && d >= 1 && nnz >= 0 && rowptr_dev, "bad CSR arguments");
    RPT_ARG(n < (int64_t)0x7fffffff, "n must fit int32 point ids");
    RPT_ARG(nnz == 0 || (col_dev && val_dev), "col/val NULL");
    // borrowed device arrays are NOT validated (that would be a pass over them): rowptr must be
    // non-decreasing from 0 to nnz and every column index in [0, d), as rpt_dataset_csr_host checks
    rpt_dataset* ds = new (std::nothrow) rpt_dataset();
    if (!ds) return fail(RPT_E_NOMEM, "out of host memory");
    ds->ctx = ctx;
    ds->n = n;
    ds->d = d;
    ds->dtype = dtype;
    ds->csr = true;
    ds->owns = false;
    ds->nnz = nnz;
    ds->rowptr = const_cast<int64_t*>(rowptr_dev);
    ds->col = const_cast<int32_t*>(col_dev);
    ds->val = const_cast<void*>(val_dev);
    *out = ds;
    return RPT_OK;
  });
}

int32_t rpt_dataset_free(rpt_dataset* ds) {
  return guarded([&]() -> int32_t {
    if (ds) dev_set_stream(ds->ctx->stream);
    if (!ds) return RPT_OK;
    if (ds->shadow32) dev_free(ds->shadow32);
    if (ds->shadow16) dev_free(ds->shadow16);
    if (ds->shadow8) dev_free(ds->shadow8);
    if (ds->sqnorm) dev_free(ds->sqnorm);
    if (ds->shadow_col16) dev_free(ds->shadow_col16);
    if (ds->shadow_ell) dev_free(ds->shadow_ell);
    if (ds->csr_split) dev_free(ds->csr_split);
    if (ds->csr_dense) dev_free(ds->csr_dense);
    if (ds->owns) {
      (void)hipSetDevice(ds->ctx->device);
      (void)stream_sync(ds->ctx->stream);
      if (ds->X) dev_free(ds->X);
      if (ds->rowptr) dev_free(ds->rowptr);
      if (ds->col) dev_free(ds->col);
      if (ds->val) dev_free(ds->val);
    }
    delete ds;
    return RPT_OK;
  });
}

int32_t rpt_dataset_info(const rpt_dataset* ds, int64_t* n, int32_t* d, int32_t* dtype,
                         int32_t* is_csr, int64_t* nnz) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ds, "ds is NULL");
    if (n) *n = ds->n;
    if (d) *d = ds->d;
    if (dtype) *dtype = ds->dtype;
    if (is_csr) *is_csr = ds->csr ? 1 : 0;
    if (nnz) *nnz = ds->csr ? ds->nnz : ds->n * ds->d;
    return RPT_OK;
  });
}

// ---- topology -------------------------------------------------------------------------
int32_t rpt_topology(int64_t n, int32_t max_depth, int32_t min_leaf, int64_t* out,
                     int64_t cap_records, int64_t* n_records) {
  return guarded([&]() -> int32_t {
    RPT_ARG(n >= 0 && max_depth >= 0 && max_depth <= 30, "bad topology arguments");
    RPT_ARG(n_records, "n_records is NULL");
    std::vector<Node> nodes;
    enumerate_topology(n, max_depth, min_leaf, nodes);
    *n_records = (int64_t)nodes.size();
    if (out) {
      for (int64_t i = 0; i < (int64_t)nodes.size() && i < cap_records; ++i) {
        out[5 * i + 0] = nodes[i].level;
        out[5 * i + 1] = nodes[i].heap;
        out[5 * i + 2] = nodes[i].off;
        out[5 * i + 3] = nodes[i].n;
        out[5 * i + 4] = nodes[i].leaf ? 1 : 0;
      }
    }
    return RPT_OK;
  });
}

// ---- projection -----------------------------------------------------------------------
static int32_t upload_R(rpt_ctx* ctx, const double* R_host, size_t count, DevBuf<double>& buf) {
  RPT_TRY(buf.alloc(count));
  return upload_async(ctx, buf.p, R_host, count * 8);
}

int32_t rpt_project_dev(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t C,
                        int32_t mode, void* P_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && ds && R_host && P_dev, "NULL argument");
    RPT_ARG(C >= 1, "C must be >= 1");
    RPT_HIP(hipSetDevice(ctx->device));
    DevBuf<double> Rd;
    RPT_TRY(upload_R(ctx, R_host, (size_t)C * ds->d, Rd));
    RPT_TRY(project_columns(ctx, ds, Rd.p, C, mode, P_dev));
    RPT_HIP(stream_sync(ctx->stream));  // Rd is released on return
    return RPT_OK;
  });
}

int32_t rpt_project_host(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t C,
                         int32_t mode, void* P_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && ds && R_host && P_host, "NULL argument");
    RPT_ARG(C >= 1, "C must be >= 1");
    RPT_HIP(hipSetDevice(ctx->device));
    size_t esz = dtype_size(proj_dtype(ds->dtype));
    DevBuf<char> P;
    RPT_TRY(P.alloc((size_t)C * ds->n * esz));
    RPT_TRY(rpt_project_dev(ctx, ds, R_host, C, mode, P.p));
    if (ds->n)
      RPT_HIP(hipMemcpy(P_host, P.p, (size_t)C * ds->n * esz, hipMemcpyDeviceToHost));
    return RPT_OK;
  });
}

// ---- forest ---------------------------------------------------------------------------
static int32_t forest_alloc(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t T,
                            int32_t L, int32_t min_leaf, rpt_forest** out) {
  RPT_ARG(ctx && ds && R_host && out, "NULL argument");
  RPT_ARG(T >= 1, "T must be >= 1");
  RPT_ARG(L >= 0 && L <= 30, "maxDepth must be in [0,30]");
  RPT_ARG(min_leaf >= 0, "minLeaf must be >= 0");
  RPT_ARG(ds->ctx == ctx, "dataset belongs to another context");
  RPT_ARG((int64_t)T * ds->n < ((int64_t)1 << 40), "forest too large");
  RPT_HIP(hipSetDevice(ctx->device));
  rpt_forest* f = new (std::nothrow) rpt_forest();
  if (!f) return fail(RPT_E_NOMEM, "out of host memory");
  f->ctx = ctx;
  f->n = ds->n;
  f->d = ds->d;
  f->T = T;
  f->L = L;
  f->min_leaf = min_leaf;
  f->pdtype = proj_dtype(ds->dtype);
  f->dtype = ds->dtype;
  f->nodes = ((int64_t)1 << L) - 1;
  int32_t s = f->perm.alloc((size_t)T * f->n);
  if (s == RPT_OK) s = f->thr.alloc((size_t)T * f->nodes);
  if (s == RPT_OK) s = f->mglo.alloc((size_t)T * f->nodes);
  if (s == RPT_OK) s = f->mghi.alloc((size_t)T * f->nodes);
  if (s == RPT_OK) s = upload_R(ctx, R_host, (size_t)T * L * f->d, f->R);
  if (s != RPT_OK) {
    delete f;
    return s;
  }
  *out = f;
  return RPT_OK;
}

int32_t rpt_forest_build(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t T,
                         int32_t L, int32_t min_leaf, int32_t flags, rpt_forest** out) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(out, "out is NULL");
    *out = nullptr;
    rpt_forest* f = nullptr;
    RPT_TRY(forest_alloc(ctx, ds, R_host, T, L, min_leaf, &f));
    int32_t s = build_forest(ctx, ds, f, flags);
    if (s != RPT_OK) {
      delete f;
      return s;
    }
    *out = f;
    return RPT_OK;
  });
}

int32_t rpt_forest_stream_build(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t T,
                                int32_t L, int32_t min_leaf, int64_t chunk, int32_t flags,
                                rpt_forest** out) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(out, "out is NULL");
    *out = nullptr;
    RPT_ARG(ctx && ds && R_host, "NULL argument");
    RPT_ARG(T >= 1, "T must be >= 1");
    RPT_ARG(L >= 0 && L <= 24, "maxDepth of a streamed forest must be in [0,24]");
    RPT_ARG(min_leaf >= 0, "minLeaf must be >= 0");
    RPT_ARG(chunk >= 1, "chunk size must be >= 1");
    RPT_ARG(ds->ctx == ctx, "dataset belongs to another context");
    RPT_HIP(hipSetDevice(ctx->device));
    rpt_forest* f = new (std::nothrow) rpt_forest();
    if (!f) return fail(RPT_E_NOMEM, "out of host memory");
    f->ctx = ctx;
    f->n = ds->n;
    f->d = ds->d;
    f->T = T;
    f->L = L;
    f->min_leaf = min_leaf;
    f->pdtype = proj_dtype(ds->dtype);
    f->dtype = ds->dtype;
    f->nodes = ((int64_t)1 << (L + 1)) - 1;
    int32_t s = f->perm.alloc((size_t)T * f->n);
    if (s == RPT_OK) s = f->thr.alloc((size_t)T * f->nodes);
    if (s == RPT_OK) s = f->mglo.alloc((size_t)T * f->nodes);
    if (s == RPT_OK) s = f->mghi.alloc((size_t)T * f->nodes);
    if (s == RPT_OK) s = upload_R(ctx, R_host, (size_t)T * L * f->d, f->R);
    if (s == RPT_OK) s = stream_build_forest(ctx, ds, f, chunk, flags);
    if (s != RPT_OK) {
      delete f;
      return s;
    }
    *out = f;
    return RPT_OK;
  });
}

int32_t rpt_forest_get_topology(rpt_forest* f, int64_t* slots, int8_t* kind_host,
                                int64_t* leaf_off_host, int64_t* leaf_len_host, int64_t* held,
                                int64_t* dropped) {
  return guarded([&]() -> int32_t {
    RPT_ARG(f, "forest is NULL");
    RPT_ARG(f->xtopo, "this forest has the implicit batch topology (rpt_topology enumerates it)");
    if (slots) *slots = f->nodes;
    if (kind_host) std::memcpy(kind_host, f->xkind_h.data(), (size_t)f->nodes);
    if (leaf_off_host) std::memcpy(leaf_off_host, f->xoff_h.data(), (size_t)f->nodes * 8);
    if (leaf_len_host) std::memcpy(leaf_len_host, f->xlen_h.data(), (size_t)f->nodes * 8);
    if (held) *held = f->held;
    if (dropped) *dropped = f->dropped;
    return RPT_OK;
  });
}

int32_t rpt_forest_import(rpt_ctx* ctx, const rpt_dataset* ds, const double* R_host, int32_t T,
                          int32_t L, int32_t min_leaf, const int32_t* perm_host,
                          const double* thr_host, const double* mglo_host,
                          const double* mghi_host, rpt_forest** out) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(out, "out is NULL");
    *out = nullptr;
    RPT_ARG(perm_host && thr_host && mglo_host && mghi_host, "NULL argument");
    rpt_forest* f = nullptr;
    RPT_TRY(forest_alloc(ctx, ds, R_host, T, L, min_leaf, &f));
    for (int64_t i = 0; i < (int64_t)T * f->n; ++i)
      if (perm_host[i] < 0 || perm_host[i] >= f->n) {
        delete f;
        return fail(RPT_E_ARG, "perm entry out of range");
      }
    hipError_t e = hipSuccess;
    if (f->n) e = hipMemcpy(f->perm.p, perm_host, (size_t)T * f->n * 4, hipMemcpyHostToDevice);
    size_t nb = (size_t)T * f->nodes * 8;
    if (e == hipSuccess && nb) e = hipMemcpy(f->thr.p, thr_host, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess && nb) e = hipMemcpy(f->mglo.p, mglo_host, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess && nb) e = hipMemcpy(f->mghi.p, mghi_host, nb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      delete f;
      return fail(RPT_E_HIP, std::string("forest import: ") + hipGetErrorString(e));
    }
    *out = f;
    return RPT_OK;
  });
}

int32_t rpt_forest_free(rpt_forest* f) {
  return guarded([&]() -> int32_t {
    if (f) dev_set_stream(f->ctx->stream);
    if (!f) return RPT_OK;
    (void)hipSetDevice(f->ctx->device);
    (void)stream_sync(f->ctx->stream);
    delete f;
    return RPT_OK;
  });
}

int32_t rpt_forest_info(const rpt_forest* f, int64_t* n, int32_t* d, int32_t* T, int32_t* L,
                        int32_t* min_leaf) {
  return guarded([&]() -> int32_t {
    RPT_ARG(f, "forest is NULL");
    if (n) *n = f->n;
    if (d) *d = f->d;
    if (T) *T = f->T;
    if (L) *L = f->L;
    if (min_leaf) *min_leaf = f->min_leaf;
    return RPT_OK;
  });
}

int32_t rpt_forest_get_perm(rpt_forest* f, int32_t* perm_host) {
  return guarded([&]() -> int32_t {
    if (f) dev_set_stream(f->ctx->stream);
    RPT_ARG(f && perm_host, "NULL argument");
    RPT_HIP(hipSetDevice(f->ctx->device));
    RPT_HIP(stream_sync(f->ctx->stream));
    if (f->n)
      RPT_HIP(hipMemcpy(perm_host, f->perm.p, (size_t)f->T * f->n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
  });
}

int32_t rpt_forest_get_nodes(rpt_forest* f, double* thr_host, double* mglo_host,
                             double* mghi_host) {
  return guarded([&]() -> int32_t {
    if (f) dev_set_stream(f->ctx->stream);
    RPT_ARG(f && thr_host && mglo_host && mghi_host, "NULL argument");
    RPT_HIP(hipSetDevice(f->ctx->device));
    RPT_HIP(stream_sync(f->ctx->stream));
    size_t nb = (size_t)f->T * f->nodes * 8;
    if (nb) {
      RPT_HIP(hipMemcpy(thr_host, f->thr.p, nb, hipMemcpyDeviceToHost));
      RPT_HIP(hipMemcpy(mglo_host, f->mglo.p, nb, hipMemcpyDeviceToHost));
      RPT_HIP(hipMemcpy(mghi_host, f->mghi.p, nb, hipMemcpyDeviceToHost));
    }
    return RPT_OK;
  });
}

int32_t rpt_forest_get_proj(rpt_forest* f, void* proj_host) {
  return guarded([&]() -> int32_t {
    if (f) dev_set_stream(f->ctx->stream);
    RPT_ARG(f && proj_host, "NULL argument");
    RPT_ARG(f->proj.p, "this forest holds no projections (imported forest)");
    RPT_HIP(hipSetDevice(f->ctx->device));
    RPT_HIP(stream_sync(f->ctx->stream));
    size_t nb = (size_t)f->T * f->L * f->n * dtype_size(f->pdtype);
    if (nb) RPT_HIP(hipMemcpy(proj_host, f->proj.p, nb, hipMemcpyDeviceToHost));
    return RPT_OK;
  });
}

int32_t rpt_forest_stats(rpt_forest* f, int64_t* tie_nodes, int64_t* big_mid_nodes) {
  return guarded([&]() -> int32_t {
    RPT_ARG(f, "forest is NULL");
    if (tie_nodes) *tie_nodes = f->tie_nodes;
    if (big_mid_nodes) *big_mid_nodes = f->big_mid_nodes;
    return RPT_OK;
  });
}

int32_t rpt_forest_get_mode(const rpt_forest* f, int32_t* mode) {
  return guarded([&]() -> int32_t {
    RPT_ARG(f && mode, "NULL argument");
    *mode = f->mode;
    return RPT_OK;
  });
}

int32_t rpt_forest_set_mode(rpt_forest* f, int32_t mode) {
  return guarded([&]() -> int32_t {
    RPT_ARG(f, "forest is NULL");
    RPT_ARG(mode == RPT_PROJ_AUTO || mode == RPT_PROJ_EXACT || mode == RPT_PROJ_MFMA,
            "unknown projection mode");
    f->mode = mode;
    return RPT_OK;
  });
}

int32_t rpt_split_segments(rpt_ctx* ctx, const double* key_host, int64_t n,
                           int32_t* perm_io_host, const int64_t* seg_off_host,
                           const int64_t* seg_len_host, int32_t S, double* thr_mg_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && key_host && perm_io_host && seg_off_host && seg_len_host && thr_mg_host,
            "NULL argument");
    RPT_ARG(n >= 1 && S >= 1, "n and S must be >= 1");
    RPT_HIP(hipSetDevice(ctx->device));
    return split_segments(ctx, key_host, n, perm_io_host, seg_off_host, seg_len_host, S,
                          thr_mg_host);
  });
}

// ---- queries --------------------------------------------------------------------------
static int32_t check_query(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* q) {
  RPT_ARG(ctx && f && q, "NULL argument");
  RPT_ARG(f->ctx == ctx && q->ctx == ctx, "handles belong to another context");
  RPT_ARG(q->d == f->d, "query dimension differs from the forest's");
  RPT_HIP(hipSetDevice(ctx->device));
  return RPT_OK;
}

int32_t rpt_candidates(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* queries,
                       int64_t* off_host, int32_t* ids_host, int64_t cap, int64_t* total) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(total, "total is NULL");
    return candidates(ctx, f, queries, off_host, ids_host, cap, total);
  });
}

int32_t rpt_knnh_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                      const rpt_dataset* queries, int32_t k, int64_t* off_host, int32_t* ids_host,
                      double* dist_host, int64_t cap, int64_t* total) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(data && data->ctx == ctx, "bad data handle");
    RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
    RPT_ARG(data->csr == queries->csr, "data and queries must both be dense or both CSR");
    RPT_ARG(k >= 1, "k must be >= 1");
    RPT_ARG(total, "total is NULL");
    return knn_h(ctx, f, data, queries, k, off_host, ids_host, dist_host, cap, total);
  });
}

}  // extern "C"

namespace {
// the knn flags: dedup rule (0 .. 2), RPT_KNN_VOTE(v), RPT_KNN_METRIC_REFERENCE, one of
// RPT_KNN_METRIC_COSINE / _INNER (not with the reference metric)
int32_t check_knn_flags(int32_t flags) {
  const int32_t metric = flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER);
  RPT_ARG(flags >= 0 && (flags & ~(0x1ffff03 | RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER)) == 0 &&
              (flags & 3) != 3,
          "unknown knn flags");
  RPT_ARG(metric != (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER),
          "RPT_KNN_METRIC_COSINE and RPT_KNN_METRIC_INNER are exclusive");
  RPT_ARG(!metric || !(flags & RPT_KNN_METRIC_REFERENCE),
          "RPT_KNN_METRIC_REFERENCE is an L2 metric: not with RPT_KNN_METRIC_COSINE / _INNER");
  return RPT_OK;
}
}  // namespace

extern "C" {

int32_t rpt_knn_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                    const rpt_dataset* queries, int32_t k, int32_t flags, int32_t* ids_dev,
                    double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(data && data->ctx == ctx, "bad data handle");
    RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
    RPT_ARG(data->csr == queries->csr, "data and queries must both be dense or both CSR");
    RPT_ARG(k >= 1 && k <= 1024, "k must be in [1,1024]");
    RPT_TRY(check_knn_flags(flags));
    RPT_ARG(ids_dev && dist_dev && count_dev, "NULL output");
    return knn_dev(ctx, f, data, queries, k, flags, ids_dev, dist_dev, count_dev);
  });
}

int32_t rpt_knn_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                     const rpt_dataset* queries, int32_t k, int32_t flags, int32_t* ids_host,
                     double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(ids_host && dist_host && count_host, "NULL output");
    RPT_ARG(k >= 1 && k <= 1024, "k must be in [1,1024]");
    RPT_TRY(check_knn_flags(flags));
    int64_t nq = queries->n;
    DevBuf<int32_t> ids, cnt;
    DevBuf<double> dist;
    RPT_TRY(ids.alloc((size_t)nq * k));
    RPT_TRY(dist.alloc((size_t)nq * k));
    RPT_TRY(cnt.alloc((size_t)nq));
    RPT_TRY(rpt_knn_dev(ctx, f, data, queries, k, flags, ids.p, dist.p, cnt.p));
    RPT_HIP(stream_sync(ctx->stream));
    if (nq) {
      RPT_HIP(hipMemcpy(ids_host, ids.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
      RPT_HIP(hipMemcpy(dist_host, dist.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
      RPT_HIP(hipMemcpy(count_host, cnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    }
    return RPT_OK;
  });
}

int32_t rpt_knn_last_candidates(rpt_ctx* ctx, int64_t* total) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && total, "NULL argument");
    *total = ctx->last_candidates;
    return RPT_OK;
  });
}

int32_t rpt_knn_last_uncertified(rpt_ctx* ctx, int64_t* total) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && total, "NULL argument");
    if (ctx->metric_unc_pending) {  // the last call was a cosine / inner-product kNN
      unsigned long long n = 0;
      RPT_HIP(stream_sync(ctx->stream));
      RPT_HIP(hipMemcpy(&n, ctx->metric_unc_dev, 8, hipMemcpyDeviceToHost));
      ctx->last_uncertified = (int64_t)n;
      ctx->metric_unc_pending = false;
    }
    *total = ctx->last_uncertified;
    return RPT_OK;
  });
}

int32_t rpt_knn_last_retries(rpt_ctx* ctx, int64_t* total) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && total, "NULL argument");
    *total = ctx->last_retries;
    return RPT_OK;
  });
}

int32_t rpt_build_last_handed_back(rpt_ctx* ctx, int64_t* nodes, int64_t* inconsistent) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && nodes && inconsistent, "NULL argument");
    *nodes = ctx->last_csub_redo;
    *inconsistent = ctx->last_csub_bad;
    return RPT_OK;
  });
}

int32_t rpt_knn_last_tier(rpt_ctx* ctx, int32_t* tier) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && tier, "NULL argument");
    *tier = ctx->last_tier;
    return RPT_OK;
  });
}

// ---- kNN graph of the indexed points ------------------------------------------------------
namespace {
// metric of the rpt_knn_graph_metric_* / rpt_knn_graph_refine_metric_* entry points
int32_t check_graph_metric(int32_t metric) {
  RPT_ARG(metric != (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER),
          "metric: RPT_KNN_METRIC_COSINE and RPT_KNN_METRIC_INNER are exclusive");
  RPT_ARG(metric == 0 || metric == RPT_KNN_METRIC_COSINE || metric == RPT_KNN_METRIC_INNER,
          "metric must be 0, RPT_KNN_METRIC_COSINE or RPT_KNN_METRIC_INNER");
  return RPT_OK;
}

// the (ids[n][k], dist[n][k], count[n]) arrays of a _host entry point, staged on the device
struct Triple {
  DevBuf<int32_t> ids, cnt;
  DevBuf<double> dist;
  size_t n = 0, k = 0;
  int32_t alloc(int64_t rows, int32_t cols) {
    n = (size_t)rows, k = (size_t)cols;
    RPT_TRY(ids.alloc(n * k));
    RPT_TRY(dist.alloc(n * k));
    return cnt.alloc(n);
  }
  int32_t upload(const int32_t* ids_host, const double* dist_host, const int32_t* count_host) {
    if (!n) return RPT_OK;
    RPT_HIP(hipMemcpy(ids.p, ids_host, n * k * 4, hipMemcpyHostToDevice));
    RPT_HIP(hipMemcpy(dist.p, dist_host, n * k * 8, hipMemcpyHostToDevice));
    RPT_HIP(hipMemcpy(cnt.p, count_host, n * 4, hipMemcpyHostToDevice));
    return RPT_OK;
  }
  int32_t download(int32_t* ids_host, double* dist_host, int32_t* count_host) {
    if (!n) return RPT_OK;
    RPT_HIP(hipMemcpy(ids_host, ids.p, n * k * 4, hipMemcpyDeviceToHost));
    RPT_HIP(hipMemcpy(dist_host, dist.p, n * k * 8, hipMemcpyDeviceToHost));
    RPT_HIP(hipMemcpy(count_host, cnt.p, n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
  }
};

// the entry points a call came through: rpt_x_* (dense rows), rpt_x_csr_* (CSR rows, L2 only) or
// rpt_x_csr_metric_* (CSR rows under every metric); graph search and preparation
enum class Rows { Dense, Csr, CsrMetric };

// rpt_knn_graph_dev (has_metric false: the metric bits in flags are refused) and
// rpt_knn_graph_metric_dev; csr: rpt_knn_graph_csr_dev and rpt_knn_graph_csr_metric_dev
int32_t graph_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k, bool has_metric,
                  int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                  int32_t* count_dev, bool csr = false) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_ARG(ctx && f && data, "NULL argument");
  RPT_ARG(f->ctx == ctx && data->ctx == ctx, "handles belong to another context");
  if (has_metric)
    RPT_TRY(check_graph_metric(metric));
  else if (flags > 0 && (flags & (RPT_KNN_METRIC_REFERENCE | RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER)))
    return fail(RPT_E_UNSUPPORTED, "the kNN graph is built under metricL2 only (no metric flags)");
  RPT_ARG((flags & ~RPT_GRAPH_ACCUMULATE) == 0, "flags must be 0 or RPT_GRAPH_ACCUMULATE");
  if (csr) RPT_ARG(data->csr, "rpt_knn_graph_csr_* takes CSR data only (dense rows: rpt_knn_graph_*)");
  else if (data->csr) return fail(RPT_E_UNSUPPORTED, "the kNN graph takes dense data only (not CSR rows: rpt_knn_graph_csr_*, rpt_knn_graph_csr_metric_*)");
  if (f->xtopo)
    return fail(RPT_E_UNSUPPORTED, "the kNN graph takes batch forests only (not a streamed forest)");
  RPT_ARG(data->n == f->n && data->d == f->d && data->dtype == f->dtype,
          "data is not the forest's data set (n, d, dtype)");
  RPT_ARG(k >= 1 && k <= RPT_GRAPH_MAX_K, "k must be in [1,64] (RPT_GRAPH_MAX_K)");
  RPT_ARG(f->n <= 0x7fffffff, "graph too large");
  RPT_ARG(f->n == 0 || (ids_dev && dist_dev && count_dev), "NULL output");
  RPT_HIP(hipSetDevice(ctx->device));
  if (csr) return knn_graph_csr_dev(ctx, f, data, k, metric, flags, ids_dev, dist_dev, count_dev);
  return knn_graph_dev(ctx, f, data, k, metric, flags, ids_dev, dist_dev, count_dev);
}

int32_t graph_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k, bool has_metric,
                   int32_t metric, int32_t flags, int32_t* ids_host, double* dist_host,
                   int32_t* count_host, bool csr = false) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_ARG(ctx && f && data, "NULL argument");
  RPT_ARG(k >= 1 && k <= RPT_GRAPH_MAX_K, "k must be in [1,64] (RPT_GRAPH_MAX_K)");
  const int64_t n = f->n;
  RPT_ARG(n == 0 || (ids_host && dist_host && count_host), "NULL output");
  Triple g;
  RPT_TRY(g.alloc(n, k));
  if (flags == RPT_GRAPH_ACCUMULATE)  // the arrays are an input too
    RPT_TRY(g.upload(ids_host, dist_host, count_host));
  RPT_TRY(graph_dev(ctx, f, data, k, has_metric, metric, flags, g.ids.p, g.dist.p, g.cnt.p, csr));
  RPT_HIP(stream_sync(ctx->stream));
  return g.download(ids_host, dist_host, count_host);
}
}  // namespace

int32_t rpt_knn_graph_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                          int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return graph_dev(ctx, f, data, k, false, 0, flags, ids_dev, dist_dev, count_dev);
  });
}

int32_t rpt_knn_graph_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                           int32_t flags, int32_t* ids_host, double* dist_host,
                           int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return graph_host(ctx, f, data, k, false, 0, flags, ids_host, dist_host, count_host);
  });
}

int32_t rpt_knn_graph_metric_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                 int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                                 int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return graph_dev(ctx, f, data, k, true, metric, flags, ids_dev, dist_dev, count_dev);
  });
}

int32_t rpt_knn_graph_metric_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                  int32_t metric, int32_t flags, int32_t* ids_host,
                                  double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return graph_host(ctx, f, data, k, true, metric, flags, ids_host, dist_host, count_host);
  });
}

int32_t rpt_knn_graph_csr_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                              int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return graph_dev(ctx, f, data, k, false, 0, flags, ids_dev, dist_dev, count_dev, true);
  });
}

int32_t rpt_knn_graph_csr_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                               int32_t flags, int32_t* ids_host, double* dist_host,
                               int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return graph_host(ctx, f, data, k, false, 0, flags, ids_host, dist_host, count_host, true);
  });
}

int32_t rpt_knn_graph_csr_metric_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                     int32_t metric, int32_t flags, int32_t* ids_dev,
                                     double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return graph_dev(ctx, f, data, k, true, metric, flags, ids_dev, dist_dev, count_dev, true);
  });
}

int32_t rpt_knn_graph_csr_metric_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, int32_t k,
                                      int32_t metric, int32_t flags, int32_t* ids_host,
                                      double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return graph_host(ctx, f, data, k, true, metric, flags, ids_host, dist_host, count_host, true);
  });
}

int32_t rpt_knn_graph_last_pairs(rpt_ctx* ctx, int64_t* pairs) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && pairs, "NULL argument");
    *pairs = ctx->last_graph_pairs;
    return RPT_OK;
  });
}

// ---- NN-descent rounds over a kNN graph ----------------------------------------------------
namespace {
// has_metric false (rpt_knn_graph_refine_*): the metric bits in flags are refused
int32_t check_refine(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse,
                     int32_t iters, bool has_metric, int32_t metric, int32_t flags, bool csr) {
  RPT_ARG(ctx && data, "NULL argument");
  RPT_ARG(data->ctx == ctx, "handles belong to another context");
  if (has_metric)
    RPT_TRY(check_graph_metric(metric));
  else if (flags > 0 && (flags & (RPT_KNN_METRIC_REFERENCE | RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER)))
    return fail(RPT_E_UNSUPPORTED, "the kNN graph is refined under metricL2 only (no metric flags)");
  RPT_ARG(flags == 0, "flags must be 0");
  if (csr) RPT_ARG(data->csr, "rpt_knn_graph_refine_csr_* takes CSR data only (dense rows: rpt_knn_graph_refine_*)");
  else if (data->csr) return fail(RPT_E_UNSUPPORTED, "the kNN graph refinement takes dense data only (not CSR rows: rpt_knn_graph_refine_csr_*, rpt_knn_graph_refine_csr_metric_*)");
  RPT_ARG(k >= 1 && k <= RPT_GRAPH_MAX_K, "k must be in [1,64] (RPT_GRAPH_MAX_K)");
  RPT_ARG(reverse >= 0 && reverse <= RPT_GRAPH_MAX_K, "reverse must be in [0,64] (RPT_GRAPH_MAX_K)");
  RPT_ARG(iters >= 1, "iters must be at least 1");
  RPT_ARG(data->n <= 0x7fffffff, "graph too large");
  return RPT_OK;
}

// the graph a _host entry point is given (rpt_knn_graph_refine_*, rpt_graph_prepare_*), checked
// before anything is uploaded: the kernels follow its ids
int32_t check_graph_rows(int64_t n, int32_t k, const int32_t* ids_host, const int32_t* count_host) {
  std::vector<int32_t> seen((size_t)n, -1);  // seen[id] = the last row that held id
  for (int64_t i = 0; i < n; ++i) {
    const int32_t c = count_host[i];
    if (c < 0 || c > k)
      return fail(RPT_E_ARG, "graph row " + std::to_string(i) + ": count " + std::to_string(c) +
                                 " outside [0, k]");
    for (int32_t s = 0; s < c; ++s) {
      const int32_t id = ids_host[i * k + s];
      if (id < 0 || id >= n)
        return fail(RPT_E_ARG, "graph row " + std::to_string(i) + ": id " + std::to_string(id) +
                                   " outside [0, n)");
      if (id == i) return fail(RPT_E_ARG, "graph row " + std::to_string(i) + " holds its own id");
      if (seen[id] == (int32_t)i)
        return fail(RPT_E_ARG, "graph row " + std::to_string(i) + " holds id " + std::to_string(id) + " twice");
      seen[id] = (int32_t)i;
    }
  }
  return RPT_OK;
}
}  // namespace

namespace {
int32_t refine_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse, int32_t iters,
                   bool has_metric, int32_t metric, int32_t flags, int32_t* ids_dev,
                   double* dist_dev, int32_t* count_dev, bool csr = false) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_TRY(check_refine(ctx, data, k, reverse, iters, has_metric, metric, flags, csr));
  RPT_ARG(data->n == 0 || (ids_dev && dist_dev && count_dev), "NULL graph arrays");
  RPT_HIP(hipSetDevice(ctx->device));
  if (csr) return knn_graph_refine_csr_dev(ctx, data, k, reverse, iters, metric, ids_dev, dist_dev, count_dev);
  return knn_graph_refine_dev(ctx, data, k, reverse, iters, metric, ids_dev, dist_dev, count_dev);
}

int32_t refine_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse, int32_t iters,
                    bool has_metric, int32_t metric, int32_t flags, int32_t* ids_host,
                    double* dist_host, int32_t* count_host, bool csr = false) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_TRY(check_refine(ctx, data, k, reverse, iters, has_metric, metric, flags, csr));
  const int64_t n = data->n;
  RPT_ARG(n == 0 || (ids_host && dist_host && count_host), "NULL graph arrays");
  RPT_TRY(check_graph_rows(n, k, ids_host, count_host));  // before anything is uploaded
  RPT_HIP(hipSetDevice(ctx->device));
  Triple g;
  RPT_TRY(g.alloc(n, k));
  RPT_TRY(g.upload(ids_host, dist_host, count_host));
  RPT_TRY(refine_dev(ctx, data, k, reverse, iters, has_metric, metric, flags, g.ids.p, g.dist.p, g.cnt.p, csr));
  RPT_HIP(stream_sync(ctx->stream));
  return g.download(ids_host, dist_host, count_host);
}
}  // namespace

int32_t rpt_knn_graph_refine_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse,
                                 int32_t iters, int32_t flags, int32_t* ids_dev, double* dist_dev,
                                 int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return refine_dev(ctx, data, k, reverse, iters, false, 0, flags, ids_dev, dist_dev, count_dev);
  });
}

int32_t rpt_knn_graph_refine_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t reverse,
                                  int32_t iters, int32_t flags, int32_t* ids_host, double* dist_host,
                                  int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return refine_host(ctx, data, k, reverse, iters, false, 0, flags, ids_host, dist_host, count_host);
  });
}

int32_t rpt_knn_graph_refine_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                        int32_t reverse, int32_t iters, int32_t metric, int32_t flags,
                                        int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return refine_dev(ctx, data, k, reverse, iters, true, metric, flags, ids_dev, dist_dev, count_dev);
  });
}

int32_t rpt_knn_graph_refine_metric_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                         int32_t reverse, int32_t iters, int32_t metric, int32_t flags,
                                         int32_t* ids_host, double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return refine_host(ctx, data, k, reverse, iters, true, metric, flags, ids_host, dist_host, count_host);
  });
}

int32_t rpt_knn_graph_refine_csr_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                     int32_t reverse, int32_t iters, int32_t flags, int32_t* ids_dev,
                                     double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return refine_dev(ctx, data, k, reverse, iters, false, 0, flags, ids_dev, dist_dev, count_dev, true);
  });
}

int32_t rpt_knn_graph_refine_csr_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                      int32_t reverse, int32_t iters, int32_t flags,
                                      int32_t* ids_host, double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return refine_host(ctx, data, k, reverse, iters, false, 0, flags, ids_host, dist_host, count_host, true);
  });
}

int32_t rpt_knn_graph_refine_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                            int32_t reverse, int32_t iters, int32_t metric,
                                            int32_t flags, int32_t* ids_dev, double* dist_dev,
                                            int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return refine_dev(ctx, data, k, reverse, iters, true, metric, flags, ids_dev, dist_dev, count_dev, true);
  });
}

int32_t rpt_knn_graph_refine_csr_metric_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                             int32_t reverse, int32_t iters, int32_t metric,
                                             int32_t flags, int32_t* ids_host, double* dist_host,
                                             int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return refine_host(ctx, data, k, reverse, iters, true, metric, flags, ids_host, dist_host, count_host, true);
  });
}

int32_t rpt_knn_graph_refine_last(rpt_ctx* ctx, int64_t* rounds, int64_t* updates,
                                  int64_t* candidates) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && rounds && updates && candidates, "NULL argument");
    RPT_HIP(hipSetDevice(ctx->device));
    return knn_graph_refine_last(ctx, rounds, updates, candidates);
  });
}

// ---- the (allow, G, group) of the rpt_*_allow_group_* entry points ------------------------------
extern "C++" {
namespace {
// the single bitmap of the rpt_*_allow_* entry points (null: every id)
AllowGroups one_bitmap(const uint32_t* allow_dev) {
  AllowGroups a;
  a.bits = allow_dev;
  return a;
}

int32_t check_group_args(const uint32_t* allow, int32_t G) {
  RPT_ARG(G >= 0, "G (the number of bitmaps) must not be negative");
  RPT_ARG(allow || G == 0, "allow is NULL with G > 0");
  return RPT_OK;
}

// device arrays as they are: a null group is every query unfiltered, whatever allow holds
AllowGroups groups_dev(const uint32_t* allow_dev, int32_t G, const int32_t* group_dev, int64_t n) {
  AllowGroups a;
  if (!group_dev) return a;
  a.bits = allow_dev;
  a.group = group_dev;
  a.G = G;
  a.stride = (n + 31) / 32;
  return a;
}

// host arrays: group[q] in [-1, G) checked before anything is uploaded, then G * ceil(n / 32) words and
// nq group entries on the device
int32_t upload_groups(const uint32_t* allow_host, int32_t G, const int32_t* group_host, int64_t n, int64_t nq,
                      DevBuf<uint32_t>& bitmap, DevBuf<int32_t>& grp, AllowGroups* out) {
  *out = AllowGroups();
  if (!group_host) return RPT_OK;
  for (int64_t q = 0; q < nq; ++q)
    if (group_host[q] < -1 || group_host[q] >= G)
      return fail(RPT_E_ARG, "group[" + std::to_string(q) + "] = " + std::to_string(group_host[q]) +
                                 " outside [-1, G)");
  const size_t words = (size_t)G * (size_t)((n + 31) / 32);
  if (words) {
    RPT_TRY(bitmap.alloc(words));
    RPT_HIP(hipMemcpy(bitmap.p, allow_host, words * 4, hipMemcpyHostToDevice));
  }
  RPT_TRY(grp.alloc((size_t)std::max<int64_t>(nq, 1)));
  if (nq) RPT_HIP(hipMemcpy(grp.p, group_host, (size_t)nq * 4, hipMemcpyHostToDevice));
  *out = groups_dev(words ? bitmap.p : nullptr, G, grp.p, n);
  return RPT_OK;
}
}  // namespace
}  // extern "C++"

// ---- beam search over a kNN graph -------------------------------------------------------------
namespace {
// Rows::Csr: the rpt_graph_search_csr_* entry points (CSR data and queries, L2 only); Rows::CsrMetric:
// the rpt_graph_search_csr_metric_* ones (the same, under every metric).  allow: the
// rpt_graph_search_allow_* ones, which take dense and CSR data alike under every metric (the caller
// passes the Rows of the data set) and a beam of `width` entries
int32_t check_search(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, int32_t kg,
                     int32_t s, int32_t k, int32_t ef, int32_t metric, int32_t flags, Rows rows,
                     bool allow = false, int32_t width = 0) {
  RPT_ARG(ctx && data && queries, "NULL argument");
  RPT_ARG(data->ctx == ctx && queries->ctx == ctx, "handles belong to another context");
  RPT_TRY(check_graph_metric(metric));
  if (rows == Rows::Csr && metric != 0)
    return fail(RPT_E_UNSUPPORTED, "the graph search on CSR rows is built under metricL2 only (metric must be 0) "
                                   "by rpt_graph_search_csr_*; cosine / inner product: rpt_graph_search_csr_metric_*");
  RPT_ARG(flags == 0, "flags must be 0");
  RPT_ARG(data->csr == queries->csr, "data and queries must both be dense or both CSR");
  if (rows == Rows::CsrMetric)
    RPT_ARG(data->csr, "rpt_graph_search_csr_metric_* takes CSR data only (dense rows: rpt_graph_search_*)");
  else if (rows == Rows::Csr)
    RPT_ARG(data->csr, "rpt_graph_search_csr_* takes CSR data only (dense rows: rpt_graph_search_*)");
  else if (data->csr)
    return fail(RPT_E_UNSUPPORTED, "the graph search takes dense data only (not CSR rows: rpt_graph_search_csr_*, "
                                   "rpt_graph_search_csr_metric_*)");
  RPT_ARG(data->d == queries->d && data->dtype == queries->dtype,
          "queries differ from the data set in d or dtype");
  RPT_ARG(kg >= 1 && kg <= RPT_GRAPH_MAX_K, "kg must be in [1,64] (RPT_GRAPH_MAX_K)");
  RPT_ARG(s >= 1 && s <= 64, "s (seeds per query) must be in [1,64]");
  RPT_ARG(k >= 1 && k <= 64, "k must be in [1,64]");
  RPT_ARG(ef >= k, "ef must be at least k");
  RPT_ARG(ef <= RPT_GRAPH_SEARCH_MAX_EF, "ef must be at most 256 (RPT_GRAPH_SEARCH_MAX_EF)");
  RPT_ARG(data->n <= 0x7fffffff, "graph too large");
  if (allow)
    RPT_ARG(width >= ef && width <= RPT_GRAPH_SEARCH_MAX_WIDTH,
            "width must be in [ef, 1024] (RPT_GRAPH_SEARCH_MAX_WIDTH)");
  return RPT_OK;
}

// the graph and the seeds a _host entry point is given, checked before anything is uploaded
int32_t check_search_arrays(int64_t n, int64_t nq, int32_t kg, const int32_t* gids_host,
                            const int32_t* gcount_host, int32_t s, const int32_t* seeds_host) {
  for (int64_t i = 0; i < n; ++i) {
    const int32_t c = gcount_host[i];
    if (c < 0 || c > kg)
      return fail(RPT_E_ARG, "graph row " + std::to_string(i) + ": count " + std::to_string(c) +
                                 " outside [0, kg]");
    for (int32_t e = 0; e < c; ++e) {
      const int32_t id = gids_host[i * kg + e];
      if (id < 0 || id >= n)
        return fail(RPT_E_ARG, "graph row " + std::to_string(i) + ": id " + std::to_string(id) +
                                   " outside [0, n)");
    }
  }
  for (int64_t q = 0; q < nq; ++q)
    for (int32_t e = 0; e < s; ++e) {
      const int32_t id = seeds_host[q * s + e];
      if (id != -1 && (id < 0 || id >= n))
        return fail(RPT_E_ARG, "seeds row " + std::to_string(q) + ": id " + std::to_string(id) +
                                   " is neither -1 nor in [0, n)");
    }
  return RPT_OK;
}

int32_t search_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, int32_t kg,
                   const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s, const int32_t* seeds_dev,
                   int32_t k, int32_t ef, int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                   int32_t* count_dev, Rows rows, bool allow = false, int32_t width = 0,
                   const AllowGroups& allow_dev = AllowGroups()) {
  if (ctx) dev_set_stream(ctx->stream);
  if (allow && data) rows = data->csr ? Rows::CsrMetric : Rows::Dense;
  RPT_TRY(check_search(ctx, data, queries, kg, s, k, ef, metric, flags, rows, allow, width));
  RPT_ARG(data->n == 0 || (gids_dev && gcount_dev), "NULL graph arrays");
  RPT_ARG(queries->n == 0 || (seeds_dev && ids_dev && dist_dev && count_dev), "NULL seeds or output");
  RPT_HIP(hipSetDevice(ctx->device));
  if (rows != Rows::Dense)
    return graph_search_csr_dev(ctx, data, queries, kg, gids_dev, gcount_dev, s, seeds_dev, k, ef, metric,
                                ids_dev, dist_dev, count_dev, allow ? width : 0, allow_dev);
  return graph_search_dev(ctx, data, queries, kg, gids_dev, gcount_dev, s, seeds_dev, k, ef, metric,
                          ids_dev, dist_dev, count_dev, allow ? width : 0, allow_dev);
}

int32_t search_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, int32_t kg,
                    const int32_t* gids_host, const int32_t* gcount_host, int32_t s,
                    const int32_t* seeds_host, int32_t k, int32_t ef, int32_t metric, int32_t flags,
                    int32_t* ids_host, double* dist_host, int32_t* count_host, Rows rows, bool allow = false,
                    int32_t width = 0, const uint32_t* allow_host = nullptr, bool grouped = false, int32_t G = 0,
                    const int32_t* group_host = nullptr) {
  if (ctx) dev_set_stream(ctx->stream);
  if (allow && data) rows = data->csr ? Rows::CsrMetric : Rows::Dense;
  RPT_TRY(check_search(ctx, data, queries, kg, s, k, ef, metric, flags, rows, allow, width));
  if (grouped) RPT_TRY(check_group_args(allow_host, G));
  const int64_t n = data->n, nq = queries->n;
  RPT_ARG(n == 0 || (gids_host && gcount_host), "NULL graph arrays");
  RPT_ARG(nq == 0 || (seeds_host && ids_host && dist_host && count_host), "NULL seeds or output");
  RPT_TRY(check_search_arrays(n, nq, kg, gids_host, gcount_host, s, seeds_host));
  RPT_HIP(hipSetDevice(ctx->device));
  DevBuf<uint32_t> gbits;
  DevBuf<int32_t> ggrp;
  AllowGroups ag;  // validated here, before anything is uploaded
  if (grouped) RPT_TRY(upload_groups(allow_host, G, group_host, n, nq, gbits, ggrp, &ag));
  DevBuf<int32_t> gids, gcnt, seeds;
  Triple out;
  RPT_TRY(gids.alloc((size_t)n * kg));
  RPT_TRY(gcnt.alloc((size_t)n));
  RPT_TRY(seeds.alloc((size_t)nq * s));
  RPT_TRY(out.alloc(nq, k));
  if (n) {
    RPT_HIP(hipMemcpy(gids.p, gids_host, (size_t)n * kg * 4, hipMemcpyHostToDevice));
    RPT_HIP(hipMemcpy(gcnt.p, gcount_host, (size_t)n * 4, hipMemcpyHostToDevice));
  }
  if (nq) RPT_HIP(hipMemcpy(seeds.p, seeds_host, (size_t)nq * s * 4, hipMemcpyHostToDevice));
  DevBuf<uint32_t> bitmap;  // the allow-list's ceil(n / 32) words
  const size_t words = allow_host && !grouped ? (size_t)((n + 31) / 32) : 0;
  if (words) {
    RPT_TRY(bitmap.alloc(words));
    RPT_HIP(hipMemcpy(bitmap.p, allow_host, words * 4, hipMemcpyHostToDevice));
  }
  if (!grouped) ag = one_bitmap(words ? bitmap.p : nullptr);
  RPT_TRY(search_dev(ctx, data, queries, kg, gids.p, gcnt.p, s, seeds.p, k, ef, metric, flags, out.ids.p,
                     out.dist.p, out.cnt.p, rows, allow, width, ag));
  RPT_HIP(stream_sync(ctx->stream));
  return out.download(ids_host, dist_host, count_host);
}
}  // namespace

int32_t rpt_graph_search_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                             int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                             const int32_t* seeds_dev, int32_t k, int32_t ef, int32_t metric,
                             int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return search_dev(ctx, data, queries, kg, gids_dev, gcount_dev, s, seeds_dev, k, ef, metric, flags,
                      ids_dev, dist_dev, count_dev, Rows::Dense);
  });
}

int32_t rpt_graph_search_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                              int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                              int32_t s, const int32_t* seeds_host, int32_t k, int32_t ef,
                              int32_t metric, int32_t flags, int32_t* ids_host, double* dist_host,
                              int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return search_host(ctx, data, queries, kg, gids_host, gcount_host, s, seeds_host, k, ef, metric, flags,
                       ids_host, dist_host, count_host, Rows::Dense);
  });
}

int32_t rpt_graph_search_csr_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                 int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                                 const int32_t* seeds_dev, int32_t k, int32_t ef, int32_t metric,
                                 int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return search_dev(ctx, data, queries, kg, gids_dev, gcount_dev, s, seeds_dev, k, ef, metric, flags,
                      ids_dev, dist_dev, count_dev, Rows::Csr);
  });
}

int32_t rpt_graph_search_csr_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                  int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                                  int32_t s, const int32_t* seeds_host, int32_t k, int32_t ef,
                                  int32_t metric, int32_t flags, int32_t* ids_host, double* dist_host,
                                  int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return search_host(ctx, data, queries, kg, gids_host, gcount_host, s, seeds_host, k, ef, metric, flags,
                       ids_host, dist_host, count_host, Rows::Csr);
  });
}

int32_t rpt_graph_search_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                        int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev,
                                        int32_t s, const int32_t* seeds_dev, int32_t k, int32_t ef,
                                        int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                                        int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return search_dev(ctx, data, queries, kg, gids_dev, gcount_dev, s, seeds_dev, k, ef, metric, flags,
                      ids_dev, dist_dev, count_dev, Rows::CsrMetric);
  });
}

int32_t rpt_graph_search_csr_metric_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                         int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                                         int32_t s, const int32_t* seeds_host, int32_t k, int32_t ef,
                                         int32_t metric, int32_t flags, int32_t* ids_host, double* dist_host,
                                         int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return search_host(ctx, data, queries, kg, gids_host, gcount_host, s, seeds_host, k, ef, metric, flags,
                       ids_host, dist_host, count_host, Rows::CsrMetric);
  });
}

int32_t rpt_graph_search_allow_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                   int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                                   const int32_t* seeds_dev, const uint32_t* allow_dev, int32_t k, int32_t ef,
                                   int32_t width, int32_t metric, int32_t flags, int32_t* ids_dev,
                                   double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    return search_dev(ctx, data, queries, kg, gids_dev, gcount_dev, s, seeds_dev, k, ef, metric, flags,
                      ids_dev, dist_dev, count_dev, Rows::Dense, true, width, one_bitmap(allow_dev));
  });
}

int32_t rpt_graph_search_allow_group_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                         int32_t kg, const int32_t* gids_dev, const int32_t* gcount_dev, int32_t s,
                                         const int32_t* seeds_dev, const uint32_t* allow_dev, int32_t G,
                                         const int32_t* group_dev, int32_t k, int32_t ef, int32_t width,
                                         int32_t metric, int32_t flags, int32_t* ids_dev, double* dist_dev,
                                         int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    RPT_TRY(check_group_args(allow_dev, G));
    return search_dev(ctx, data, queries, kg, gids_dev, gcount_dev, s, seeds_dev, k, ef, metric, flags,
                      ids_dev, dist_dev, count_dev, Rows::Dense, true, width,
                      groups_dev(allow_dev, G, group_dev, data ? data->n : 0));
  });
}

int32_t rpt_graph_search_allow_group_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                          int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                                          int32_t s, const int32_t* seeds_host, const uint32_t* allow_host,
                                          int32_t G, const int32_t* group_host, int32_t k, int32_t ef,
                                          int32_t width, int32_t metric, int32_t flags, int32_t* ids_host,
                                          double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return search_host(ctx, data, queries, kg, gids_host, gcount_host, s, seeds_host, k, ef, metric, flags,
                       ids_host, dist_host, count_host, Rows::Dense, true, width, allow_host, true, G, group_host);
  });
}

int32_t rpt_graph_search_allow_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                    int32_t kg, const int32_t* gids_host, const int32_t* gcount_host,
                                    int32_t s, const int32_t* seeds_host, const uint32_t* allow_host,
                                    int32_t k, int32_t ef, int32_t width, int32_t metric, int32_t flags,
                                    int32_t* ids_host, double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    return search_host(ctx, data, queries, kg, gids_host, gcount_host, s, seeds_host, k, ef, metric, flags,
                       ids_host, dist_host, count_host, Rows::Dense, true, width, allow_host);
  });
}

int32_t rpt_graph_search_last(rpt_ctx* ctx, int64_t* expansions, int64_t* evaluated) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && expansions && evaluated, "NULL argument");
    RPT_HIP(hipSetDevice(ctx->device));
    return graph_search_last(ctx, expansions, evaluated);
  });
}

// ---- a kNN graph made ready for the search -------------------------------------------------------
namespace {
// Rows::Csr: the rpt_graph_prepare_csr_* entry points (CSR data, L2 only); Rows::CsrMetric: the
// rpt_graph_prepare_csr_metric_* ones (the same, under every metric)
int32_t check_prepare(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, int32_t kout, int32_t metric,
                      int32_t flags, Rows rows) {
  RPT_ARG(ctx && data, "NULL argument");
  RPT_ARG(data->ctx == ctx, "handles belong to another context");
  RPT_TRY(check_graph_metric(metric));
  if (rows == Rows::Csr && metric != 0)
    return fail(RPT_E_UNSUPPORTED,
                "the graph preparation on CSR rows is built under metricL2 only (metric must be 0) by "
                "rpt_graph_prepare_csr_*; cosine / inner product: rpt_graph_prepare_csr_metric_*");
  RPT_ARG((flags & ~(RPT_GRAPH_PREP_DIVERSIFY | RPT_GRAPH_PREP_REVERSE)) == 0,
          "flags must be an or of RPT_GRAPH_PREP_DIVERSIFY and RPT_GRAPH_PREP_REVERSE");
  if (rows == Rows::CsrMetric)
    RPT_ARG(data->csr, "rpt_graph_prepare_csr_metric_* takes CSR data only (dense rows: rpt_graph_prepare_*)");
  else if (rows == Rows::Csr)
    RPT_ARG(data->csr, "rpt_graph_prepare_csr_* takes CSR data only (dense rows: rpt_graph_prepare_*)");
  else if (data->csr)
    return fail(RPT_E_UNSUPPORTED, "the graph preparation takes dense data only (not CSR rows: "
                                   "rpt_graph_prepare_csr_*, rpt_graph_prepare_csr_metric_*)");
  RPT_ARG(k >= 1 && k <= RPT_GRAPH_MAX_K, "k must be in [1,64] (RPT_GRAPH_MAX_K)");
  RPT_ARG(kout >= 1 && kout <= RPT_GRAPH_MAX_K, "kout must be in [1,64] (RPT_GRAPH_MAX_K)");
  RPT_ARG(data->n <= 0x7fffffff, "graph too large");
  return RPT_OK;
}

int32_t prepare_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_dev,
                    const double* dist_dev, const int32_t* count_dev, int32_t kout, int32_t metric,
                    int32_t flags, int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev,
                    Rows rows) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_TRY(check_prepare(ctx, data, k, kout, metric, flags, rows));
  RPT_ARG(data->n == 0 || (ids_dev && dist_dev && count_dev), "NULL graph arrays");
  RPT_ARG(data->n == 0 || (out_ids_dev && out_dist_dev && out_count_dev), "NULL output");
  RPT_HIP(hipSetDevice(ctx->device));
  return graph_prepare_dev(ctx, data, k, ids_dev, dist_dev, count_dev, kout, metric, flags, out_ids_dev,
                           out_dist_dev, out_count_dev);
}

int32_t prepare_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_host,
                     const double* dist_host, const int32_t* count_host, int32_t kout, int32_t metric,
                     int32_t flags, int32_t* out_ids_host, double* out_dist_host, int32_t* out_count_host,
                     Rows rows) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_TRY(check_prepare(ctx, data, k, kout, metric, flags, rows));
  const int64_t n = data->n;
  RPT_ARG(n == 0 || (ids_host && dist_host && count_host), "NULL graph arrays");
  RPT_ARG(n == 0 || (out_ids_host && out_dist_host && out_count_host), "NULL output");
  RPT_TRY(check_graph_rows(n, k, ids_host, count_host));  // before anything is uploaded
  RPT_HIP(hipSetDevice(ctx->device));
  Triple g, out;
  RPT_TRY(g.alloc(n, k));
  RPT_TRY(out.alloc(n, kout));
  RPT_TRY(g.upload(ids_host, dist_host, count_host));
  RPT_TRY(prepare_dev(ctx, data, k, g.ids.p, g.dist.p, g.cnt.p, kout, metric, flags, out.ids.p, out.dist.p,
                      out.cnt.p, rows));
  RPT_HIP(stream_sync(ctx->stream));
  return out.download(out_ids_host, out_dist_host, out_count_host);
}
}  // namespace

int32_t rpt_graph_prepare_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_dev,
                              const double* dist_dev, const int32_t* count_dev, int32_t kout,
                              int32_t metric, int32_t flags, int32_t* out_ids_dev, double* out_dist_dev,
                              int32_t* out_count_dev) {
  return guarded([&]() -> int32_t {
    return prepare_dev(ctx, data, k, ids_dev, dist_dev, count_dev, kout, metric, flags, out_ids_dev,
                       out_dist_dev, out_count_dev, Rows::Dense);
  });
}

int32_t rpt_graph_prepare_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_host,
                               const double* dist_host, const int32_t* count_host, int32_t kout,
                               int32_t metric, int32_t flags, int32_t* out_ids_host, double* out_dist_host,
                               int32_t* out_count_host) {
  return guarded([&]() -> int32_t {
    return prepare_host(ctx, data, k, ids_host, dist_host, count_host, kout, metric, flags, out_ids_host,
                        out_dist_host, out_count_host, Rows::Dense);
  });
}

int32_t rpt_graph_prepare_csr_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k, const int32_t* ids_dev,
                                  const double* dist_dev, const int32_t* count_dev, int32_t kout,
                                  int32_t metric, int32_t flags, int32_t* out_ids_dev,
                                  double* out_dist_dev, int32_t* out_count_dev) {
  return guarded([&]() -> int32_t {
    return prepare_dev(ctx, data, k, ids_dev, dist_dev, count_dev, kout, metric, flags, out_ids_dev,
                       out_dist_dev, out_count_dev, Rows::Csr);
  });
}

int32_t rpt_graph_prepare_csr_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                   const int32_t* ids_host, const double* dist_host,
                                   const int32_t* count_host, int32_t kout, int32_t metric, int32_t flags,
                                   int32_t* out_ids_host, double* out_dist_host, int32_t* out_count_host) {
  return guarded([&]() -> int32_t {
    return prepare_host(ctx, data, k, ids_host, dist_host, count_host, kout, metric, flags, out_ids_host,
                        out_dist_host, out_count_host, Rows::Csr);
  });
}

int32_t rpt_graph_prepare_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                         const int32_t* ids_dev, const double* dist_dev,
                                         const int32_t* count_dev, int32_t kout, int32_t metric,
                                         int32_t flags, int32_t* out_ids_dev, double* out_dist_dev,
                                         int32_t* out_count_dev) {
  return guarded([&]() -> int32_t {
    return prepare_dev(ctx, data, k, ids_dev, dist_dev, count_dev, kout, metric, flags, out_ids_dev,
                       out_dist_dev, out_count_dev, Rows::CsrMetric);
  });
}

int32_t rpt_graph_prepare_csr_metric_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t k,
                                          const int32_t* ids_host, const double* dist_host,
                                          const int32_t* count_host, int32_t kout, int32_t metric,
                                          int32_t flags, int32_t* out_ids_host, double* out_dist_host,
                                          int32_t* out_count_host) {
  return guarded([&]() -> int32_t {
    return prepare_host(ctx, data, k, ids_host, dist_host, count_host, kout, metric, flags, out_ids_host,
                        out_dist_host, out_count_host, Rows::CsrMetric);
  });
}

int32_t rpt_graph_prepare_last(rpt_ctx* ctx, int64_t* pairs, int64_t* occluded, int64_t* capped) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && pairs && occluded && capped, "NULL argument");
    RPT_HIP(hipSetDevice(ctx->device));
    return graph_prepare_last(ctx, pairs, occluded, capped);
  });
}

// ---- new rows into a kNN graph -------------------------------------------------------------------
namespace {
// one pair of entry points for dense and CSR data under every metric
int32_t check_insert(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, int64_t m, int32_t s, int32_t ef,
                     int64_t batch, int32_t metric, int32_t flags) {
  RPT_ARG(ctx && data, "NULL argument");
  RPT_ARG(data->ctx == ctx, "handles belong to another context");
  RPT_TRY(check_graph_metric(metric));
  RPT_ARG(flags == 0, "flags must be 0");
  RPT_ARG(kg >= 1 && kg <= RPT_GRAPH_MAX_K, "kg must be in [1,64] (RPT_GRAPH_MAX_K)");
  RPT_ARG(s >= 1 && s <= 64, "s (seeds per new row) must be in [1,64]");
  RPT_ARG(ef >= kg, "ef must be at least kg");
  RPT_ARG(ef <= RPT_GRAPH_SEARCH_MAX_EF, "ef must be at most 256 (RPT_GRAPH_SEARCH_MAX_EF)");
  RPT_ARG(batch >= 1, "batch must be at least 1");
  RPT_ARG(m >= 0 && m <= data->n, "m must be in [0, data.n]: the new rows are the data set's last m");
  RPT_ARG(data->n <= 0x7fffffff, "graph too large");
  RPT_ARG(std::min<int64_t>(batch, m) * kg <= 0x7fffffff, "a chunk of min(batch, m) rows holds 2^31 or more entries");
  return RPT_OK;
}

int32_t insert_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_dev,
                   const double* gdist_dev, const int32_t* gcount_dev, int64_t m, int32_t s,
                   const int32_t* seeds_dev, int32_t ef, int64_t batch, int32_t metric, int32_t flags,
                   int32_t* oids_dev, double* odist_dev, int32_t* ocount_dev) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_TRY(check_insert(ctx, data, kg, m, s, ef, batch, metric, flags));
  RPT_ARG(data->n == m || (gids_dev && gdist_dev && gcount_dev), "NULL graph arrays");
  RPT_ARG(m == 0 || seeds_dev, "NULL seeds");
  RPT_ARG(data->n == 0 || (oids_dev && odist_dev && ocount_dev), "NULL output");
  RPT_HIP(hipSetDevice(ctx->device));
  return graph_insert_dev(ctx, data, kg, gids_dev, gdist_dev, gcount_dev, m, s, seeds_dev, ef, batch, metric,
                          oids_dev, odist_dev, ocount_dev);
}

int32_t insert_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_host,
                    const double* gdist_host, const int32_t* gcount_host, int64_t m, int32_t s,
                    const int32_t* seeds_host, int32_t ef, int64_t batch, int32_t metric, int32_t flags,
                    int32_t* oids_host, double* odist_host, int32_t* ocount_host) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_TRY(check_insert(ctx, data, kg, m, s, ef, batch, metric, flags));
  const int64_t N = data->n, n = N - m;
  RPT_ARG(n == 0 || (gids_host && gdist_host && gcount_host), "NULL graph arrays");
  RPT_ARG(m == 0 || seeds_host, "NULL seeds");
  RPT_ARG(N == 0 || (oids_host && odist_host && ocount_host), "NULL output");
  // before anything is uploaded: the graph's counts and ids, then the seeds, which may name new rows
  RPT_TRY(check_search_arrays(n, 0, kg, gids_host, gcount_host, s, nullptr));
  for (int64_t q = 0; q < m; ++q)
    for (int32_t e = 0; e < s; ++e) {
      const int32_t id = seeds_host[q * s + e];
      if (id != -1 && (id < 0 || id >= N))
        return fail(RPT_E_ARG, "seeds row " + std::to_string(q) + ": id " + std::to_string(id) +
                                   " is neither -1 nor in [0, N)");
    }
  RPT_HIP(hipSetDevice(ctx->device));
  Triple g, out;
  DevBuf<int32_t> seeds;
  RPT_TRY(g.alloc(n, kg));
  RPT_TRY(out.alloc(N, kg));
  RPT_TRY(seeds.alloc((size_t)m * s));
  RPT_TRY(g.upload(gids_host, gdist_host, gcount_host));
  if (m) RPT_HIP(hipMemcpy(seeds.p, seeds_host, (size_t)m * s * 4, hipMemcpyHostToDevice));
  RPT_TRY(insert_dev(ctx, data, kg, g.ids.p, g.dist.p, g.cnt.p, m, s, seeds.p, ef, batch, metric, flags,
                     out.ids.p, out.dist.p, out.cnt.p));
  RPT_HIP(stream_sync(ctx->stream));
  return out.download(oids_host, odist_host, ocount_host);
}
}  // namespace

int32_t rpt_graph_insert_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_dev,
                             const double* gdist_dev, const int32_t* gcount_dev, int64_t m, int32_t s,
                             const int32_t* seeds_dev, int32_t ef, int64_t batch, int32_t metric,
                             int32_t flags, int32_t* oids_dev, double* odist_dev, int32_t* ocount_dev) {
  return guarded([&]() -> int32_t {
    return insert_dev(ctx, data, kg, gids_dev, gdist_dev, gcount_dev, m, s, seeds_dev, ef, batch, metric, flags,
                      oids_dev, odist_dev, ocount_dev);
  });
}

int32_t rpt_graph_insert_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_host,
                              const double* gdist_host, const int32_t* gcount_host, int64_t m, int32_t s,
                              const int32_t* seeds_host, int32_t ef, int64_t batch, int32_t metric,
                              int32_t flags, int32_t* oids_host, double* odist_host, int32_t* ocount_host) {
  return guarded([&]() -> int32_t {
    return insert_host(ctx, data, kg, gids_host, gdist_host, gcount_host, m, s, seeds_host, ef, batch, metric,
                       flags, oids_host, odist_host, ocount_host);
  });
}

int32_t rpt_graph_insert_last(rpt_ctx* ctx, int64_t* chunks, int64_t* evaluated, int64_t* offered,
                              int64_t* accepted) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && chunks && evaluated && offered && accepted, "NULL argument");
    RPT_HIP(hipSetDevice(ctx->device));
    return graph_insert_last(ctx, chunks, evaluated, offered, accepted);
  });
}

// ---- rows out of a kNN graph ---------------------------------------------------------------------
namespace {
// one pair of entry points for dense and CSR data under every metric
int32_t check_delete(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, int32_t metric, int32_t flags) {
  RPT_ARG(ctx && data, "NULL argument");
  RPT_ARG(data->ctx == ctx, "handles belong to another context");
  RPT_TRY(check_graph_metric(metric));
  RPT_ARG((flags & ~RPT_GRAPH_DELETE_COMPACT) == 0, "flags must be 0 or RPT_GRAPH_DELETE_COMPACT");
  RPT_ARG(kg >= 1 && kg <= RPT_GRAPH_MAX_K, "kg must be in [1,64] (RPT_GRAPH_MAX_K)");
  RPT_ARG(data->n <= 0x7fffffff, "graph too large");
  return RPT_OK;
}

int32_t delete_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_dev,
                   const double* gdist_dev, const int32_t* gcount_dev, const uint32_t* keep_dev, int32_t metric,
                   int32_t flags, int32_t* oids_dev, double* odist_dev, int32_t* ocount_dev, int32_t* newid_dev) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_TRY(check_delete(ctx, data, kg, metric, flags));
  RPT_ARG(data->n == 0 || (gids_dev && gdist_dev && gcount_dev), "NULL graph arrays");
  RPT_ARG(data->n == 0 || (oids_dev && odist_dev && ocount_dev), "NULL output");
  RPT_HIP(hipSetDevice(ctx->device));
  return graph_delete_dev(ctx, data, kg, gids_dev, gdist_dev, gcount_dev, keep_dev, metric, flags, oids_dev,
                          odist_dev, ocount_dev, newid_dev);
}

int32_t delete_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_host,
                    const double* gdist_host, const int32_t* gcount_host, const uint32_t* keep_host,
                    int32_t metric, int32_t flags, int32_t* oids_host, double* odist_host, int32_t* ocount_host,
                    int32_t* newid_host) {
  if (ctx) dev_set_stream(ctx->stream);
  RPT_TRY(check_delete(ctx, data, kg, metric, flags));
  const int64_t n = data->n;
  RPT_ARG(n == 0 || (gids_host && gdist_host && gcount_host), "NULL graph arrays");
  RPT_ARG(n == 0 || (oids_host && odist_host && ocount_host), "NULL output");
  RPT_TRY(check_search_arrays(n, 0, kg, gids_host, gcount_host, 0, nullptr));  // before anything is uploaded
  RPT_HIP(hipSetDevice(ctx->device));
  Triple g, out;
  DevBuf<uint32_t> bitmap;
  DevBuf<int32_t> newid;
  RPT_TRY(g.alloc(n, kg));
  RPT_TRY(out.alloc(n, kg));
  RPT_TRY(newid.alloc((size_t)n));
  const size_t words = keep_host ? (size_t)((n + 31) / 32) : 0;
  RPT_TRY(bitmap.alloc(words));
  RPT_TRY(g.upload(gids_host, gdist_host, gcount_host));
  if (words) RPT_HIP(hipMemcpy(bitmap.p, keep_host, words * 4, hipMemcpyHostToDevice));
  RPT_TRY(delete_dev(ctx, data, kg, g.ids.p, g.dist.p, g.cnt.p, words ? bitmap.p : nullptr, metric, flags,
                     out.ids.p, out.dist.p, out.cnt.p, newid.p));
  int64_t kept = 0, touched = 0, evaluated = 0, dropped = 0;
  RPT_TRY(graph_delete_last(ctx, &kept, &touched, &evaluated, &dropped));  // synchronises
  // the compact form has `kept` rows; what lies behind them in the caller's arrays is left as it was
  const size_t rows = (size_t)((flags & RPT_GRAPH_DELETE_COMPACT) ? kept : n);
  if (rows) {
    RPT_HIP(hipMemcpy(oids_host, out.ids.p, rows * kg * 4, hipMemcpyDeviceToHost));
    RPT_HIP(hipMemcpy(odist_host, out.dist.p, rows * kg * 8, hipMemcpyDeviceToHost));
    RPT_HIP(hipMemcpy(ocount_host, out.cnt.p, rows * 4, hipMemcpyDeviceToHost));
  }
  if (newid_host && n) RPT_HIP(hipMemcpy(newid_host, newid.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return RPT_OK;
}
}  // namespace

int32_t rpt_graph_delete_dev(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_dev,
                             const double* gdist_dev, const int32_t* gcount_dev, const uint32_t* keep_dev,
                             int32_t metric, int32_t flags, int32_t* oids_dev, double* odist_dev,
                             int32_t* ocount_dev, int32_t* newid_dev) {
  return guarded([&]() -> int32_t {
    return delete_dev(ctx, data, kg, gids_dev, gdist_dev, gcount_dev, keep_dev, metric, flags, oids_dev, odist_dev,
                      ocount_dev, newid_dev);
  });
}

int32_t rpt_graph_delete_host(rpt_ctx* ctx, const rpt_dataset* data, int32_t kg, const int32_t* gids_host,
                              const double* gdist_host, const int32_t* gcount_host, const uint32_t* keep_host,
                              int32_t metric, int32_t flags, int32_t* oids_host, double* odist_host,
                              int32_t* ocount_host, int32_t* newid_host) {
  return guarded([&]() -> int32_t {
    return delete_host(ctx, data, kg, gids_host, gdist_host, gcount_host, keep_host, metric, flags, oids_host,
                       odist_host, ocount_host, newid_host);
  });
}

int32_t rpt_graph_delete_last(rpt_ctx* ctx, int64_t* kept, int64_t* touched, int64_t* evaluated,
                              int64_t* dropped) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && kept && touched && evaluated && dropped, "NULL argument");
    RPT_HIP(hipSetDevice(ctx->device));
    return graph_delete_last(ctx, kept, touched, evaluated, dropped);
  });
}

int32_t rpt_knn_merge_dev(rpt_ctx* ctx, const int32_t* ids_dev, const double* dist_dev,
                          const int32_t* count_dev, int32_t G, int64_t nq, int32_t k,
                          int32_t flags, int32_t* out_ids_dev, double* out_dist_dev,
                          int32_t* out_count_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && ids_dev && dist_dev && count_dev && out_ids_dev && out_dist_dev &&
                out_count_dev,
            "NULL argument");
    RPT_ARG(G >= 1 && nq >= 0 && k >= 1 && k <= 1024, "bad merge arguments");
    RPT_HIP(hipSetDevice(ctx->device));
    return knn_merge_dev(ctx, ids_dev, dist_dev, count_dev, 0, G, nq, k, flags, out_ids_dev,
                         out_dist_dev, out_count_dev);
  });
}

int32_t rpt_knn_record_layout(int64_t nq, int32_t k, int64_t* bytes, int64_t* off_dist,
                              int64_t* off_ids, int64_t* off_count) {
  return guarded([&]() -> int32_t {
    RPT_ARG(bytes && off_dist && off_ids && off_count, "NULL argument");
    RPT_ARG(nq >= 0 && k >= 1, "bad record arguments");
    *off_dist = 0;
    *off_ids = nq * k * 8;
    *off_count = nq * k * 12;
    // + the shard's status word (int32 behind the counts, 0 = ok), rounded to 16 bytes
    *bytes = (nq * k * 12 + nq * 4 + 4 + 15) & ~(int64_t)15;
    return RPT_OK;
  });
}

int32_t rpt_knn_merge_records_dev(rpt_ctx* ctx, const void* records_dev, int64_t record_bytes,
                                  int32_t G, int64_t nq, int32_t k, int32_t flags,
                                  int32_t* out_ids_dev, double* out_dist_dev,
                                  int32_t* out_count_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ctx && records_dev && out_ids_dev && out_dist_dev && out_count_dev, "NULL argument");
    RPT_ARG(G >= 1 && nq >= 0 && k >= 1 && k <= 1024, "bad merge arguments");
    int64_t bytes, od, oi, oc;
    RPT_TRY(rpt_knn_record_layout(nq, k, &bytes, &od, &oi, &oc));
    RPT_ARG(record_bytes >= bytes && record_bytes % 8 == 0,
            "record_bytes smaller than rpt_knn_record_layout's size or not a multiple of 8");
    RPT_HIP(hipSetDevice(ctx->device));
    const char* base = static_cast<const char*>(records_dev);
    return knn_merge_dev(ctx, reinterpret_cast<const int32_t*>(base + oi),
                         reinterpret_cast<const double*>(base + od),
                         reinterpret_cast<const int32_t*>(base + oc), record_bytes, G, nq, k, flags,
                         out_ids_dev, out_dist_dev, out_count_dev);
  });
}

}  // extern "C"

namespace {
// the brute-force entry points: dense data with dense queries under 0 / RPT_KNN_METRIC_COSINE /
// _INNER, CSR data with CSR queries under 0 / RPT_KNN_METRIC_REFERENCE
int32_t check_brute(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, int32_t k,
                    int32_t flags) {
  RPT_ARG(ctx && data && queries, "NULL argument");
  RPT_ARG(data->ctx == ctx && queries->ctx == ctx, "handles belong to another context");
  RPT_ARG(data->csr == queries->csr, "data and queries must both be dense or both CSR");
  RPT_ARG(data->d == queries->d && data->dtype == queries->dtype, "shape/dtype mismatch");
  RPT_ARG(k >= 1 && k <= 1024, "k must be in [1,1024]");
  if (data->csr) {
    if (flags == RPT_KNN_METRIC_COSINE || flags == RPT_KNN_METRIC_INNER)
      return fail(RPT_E_UNSUPPORTED, "RPT_KNN_METRIC_COSINE / _INNER: dense data only");
    RPT_ARG(flags == 0 || flags == RPT_KNN_METRIC_REFERENCE,
            "flags must be 0 or RPT_KNN_METRIC_REFERENCE for CSR data");
  } else {
    RPT_ARG(flags == 0 || flags == RPT_KNN_METRIC_COSINE || flags == RPT_KNN_METRIC_INNER,
            "flags must be 0, RPT_KNN_METRIC_COSINE or RPT_KNN_METRIC_INNER");
  }
  RPT_HIP(hipSetDevice(ctx->device));
  return RPT_OK;
}
}  // namespace

extern "C" {

int32_t rpt_brute_knn_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                           int32_t k, int32_t* ids_host, double* dist_host) {
  return rpt_brute_knn_metric_host(ctx, data, queries, k, 0, ids_host, dist_host);
}

int32_t rpt_brute_knn_metric_host(rpt_ctx* ctx, const rpt_dataset* data,
                                  const rpt_dataset* queries, int32_t k, int32_t flags,
                                  int32_t* ids_host, double* dist_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ids_host && dist_host, "NULL argument");
    RPT_TRY(check_brute(ctx, data, queries, k, flags));
    return brute_knn_metric(ctx, data, queries, k, flags, ids_host, dist_host);
  });
}

int32_t rpt_brute_knn_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                          int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ids_dev && dist_dev, "NULL output");
    RPT_TRY(check_brute(ctx, data, queries, k, flags));
    return brute_knn_dev(ctx, data, queries, k, flags, ids_dev, dist_dev);
  });
}

int32_t rpt_recall_hits_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                             const rpt_dataset* queries, int32_t k, int32_t flags,
                             int32_t* hits_host, int32_t* truth_ids_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(hits_host, "NULL output");
    RPT_TRY(check_brute(ctx, data, queries, k, flags));
    RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
    RPT_ARG(queries->n * (int64_t)f->T <= 0x7fffffff, "too many (query, tree) pairs for one call");
    return recall_hits(ctx, f, data, queries, k, flags, hits_host, truth_ids_host);
  });
}

}  // extern "C"

// ---- cosine / inner product on CSR rows -----------------------------------------------------
namespace {
// the rpt_*_csr_metric_* entry points: CSR data with CSR queries, exactly one metric bit in `flags`
// next to `allowed` (the duplicate rule of the forest query; 0 for the brute force)
int32_t check_csr_metric(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, int32_t k,
                         int32_t flags, int32_t allowed, const char* l2_entry, const char* dense_entry) {
  RPT_ARG(ctx && data && queries, "NULL argument");
  RPT_ARG(data->ctx == ctx && queries->ctx == ctx, "handles belong to another context");
  const int32_t metric = flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER);
  if (!data->csr || !queries->csr) return fail(RPT_E_ARG, dense_entry);
  RPT_ARG(!(flags & RPT_KNN_METRIC_REFERENCE),
          "RPT_KNN_METRIC_REFERENCE is an L2 metric: not with RPT_KNN_METRIC_COSINE / _INNER");
  if (metric != RPT_KNN_METRIC_COSINE && metric != RPT_KNN_METRIC_INNER) return fail(RPT_E_ARG, l2_entry);
  if (allowed && ((flags >> 8) & 0xffff) != 0)
    return fail(RPT_E_UNSUPPORTED, "RPT_KNN_METRIC_COSINE / _INNER: no voting (RPT_KNN_VOTE)");
  RPT_ARG(flags >= 0 && (flags & ~(metric | allowed)) == 0 && (flags & 3) != 3, "unknown knn flags");
  RPT_ARG(data->d == queries->d && data->dtype == queries->dtype, "data and query shape / dtype must match");
  RPT_ARG(k >= 1 && k <= 1024, "k must be in [1,1024]");
  RPT_HIP(hipSetDevice(ctx->device));
  return RPT_OK;
}
const char kCsrMetricKnnL2[] =
    "rpt_knn_csr_metric_*: exactly one of RPT_KNN_METRIC_COSINE / _INNER (L2 on CSR rows: rpt_knn_*)";
const char kCsrMetricKnnDense[] =
    "rpt_knn_csr_metric_*: CSR data and CSR queries (dense rows under the metrics: rpt_knn_*)";
const char kCsrMetricBruteL2[] =
    "rpt_brute_knn_csr_metric_*: exactly one of RPT_KNN_METRIC_COSINE / _INNER (L2 on CSR rows: rpt_brute_knn_*)";
const char kCsrMetricBruteDense[] =
    "rpt_brute_knn_csr_metric_*: CSR data and CSR queries (dense rows under the metrics: "
    "rpt_brute_knn_metric_*)";
}  // namespace

extern "C" {

int32_t rpt_knn_csr_metric_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                               const rpt_dataset* queries, int32_t k, int32_t flags, int32_t* ids_dev,
                               double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_TRY(check_csr_metric(ctx, data, queries, k, flags, 3, kCsrMetricKnnL2, kCsrMetricKnnDense));
    RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
    RPT_ARG(proj_dtype(queries->dtype) == f->pdtype,
            "query dtype must have the forest's projection type (f64 vs f32/bf16)");
    RPT_ARG(ids_dev && dist_dev && count_dev, "NULL output");
    return knn_csr_metric_dev(ctx, f, data, queries, k, flags, ids_dev, dist_dev, count_dev);
  });
}

int32_t rpt_knn_csr_metric_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                const rpt_dataset* queries, int32_t k, int32_t flags, int32_t* ids_host,
                                double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_TRY(check_csr_metric(ctx, data, queries, k, flags, 3, kCsrMetricKnnL2, kCsrMetricKnnDense));
    RPT_ARG(ids_host && dist_host && count_host, "NULL output");
    Triple out;
    RPT_TRY(out.alloc(queries->n, k));
    RPT_TRY(rpt_knn_csr_metric_dev(ctx, f, data, queries, k, flags, out.ids.p, out.dist.p, out.cnt.p));
    RPT_HIP(stream_sync(ctx->stream));
    return out.download(ids_host, dist_host, count_host);
  });
}

int32_t rpt_brute_knn_csr_metric_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                     int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_csr_metric(ctx, data, queries, k, flags, 0, kCsrMetricBruteL2, kCsrMetricBruteDense));
    RPT_ARG(ids_dev && dist_dev, "NULL output");
    return brute_knn_csr_metric_dev(ctx, data, queries, k, flags, ids_dev, dist_dev);
  });
}

int32_t rpt_brute_knn_csr_metric_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                      int32_t k, int32_t flags, int32_t* ids_host, double* dist_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_csr_metric(ctx, data, queries, k, flags, 0, kCsrMetricBruteL2, kCsrMetricBruteDense));
    RPT_ARG(ids_host && dist_host, "NULL output");
    const int64_t nq = queries->n;
    if (nq == 0) return RPT_OK;
    DevBuf<int32_t> ids;
    DevBuf<double> dist;
    RPT_TRY(ids.alloc((size_t)nq * k));
    RPT_TRY(dist.alloc((size_t)nq * k));
    RPT_TRY(brute_knn_csr_metric_dev(ctx, data, queries, k, flags, ids.p, dist.p));
    RPT_HIP(stream_sync(ctx->stream));
    RPT_HIP(hipMemcpy(ids_host, ids.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    RPT_HIP(hipMemcpy(dist_host, dist.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    return RPT_OK;
  });
}

int32_t rpt_recall_hits_csr_metric_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                        const rpt_dataset* queries, int32_t k, int32_t flags,
                                        int32_t* hits_host, int32_t* truth_ids_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_TRY(check_csr_metric(ctx, data, queries, k, flags, 0, kCsrMetricBruteL2, kCsrMetricBruteDense));
    RPT_ARG(hits_host, "NULL output");
    RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
    RPT_ARG(proj_dtype(queries->dtype) == f->pdtype,
            "query dtype must have the forest's projection type (f64 vs f32/bf16)");
    RPT_ARG(queries->n * (int64_t)f->T <= 0x7fffffff, "too many (query, tree) pairs for one call");
    return recall_hits(ctx, f, data, queries, k, flags, hits_host, truth_ids_host);
  });
}

}  // extern "C"

// ---- the vote threshold for every row layout and distance --------------------------------------
namespace {
int32_t check_knn_vote(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries, int32_t k,
                       int32_t v, int32_t flags) {
  RPT_TRY(check_query(ctx, f, queries));
  RPT_ARG(data && data->ctx == ctx, "bad data handle");
  RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
  RPT_ARG(data->csr == queries->csr, "data and queries must both be dense or both CSR");
  RPT_ARG(data->dtype == queries->dtype, "data and query dtype must match");
  RPT_ARG(proj_dtype(queries->dtype) == f->pdtype,
          "query dtype must have the forest's projection type (f64 vs f32/bf16)");
  RPT_ARG(k >= 1 && k <= 1024, "k must be in [1,1024]");
  RPT_ARG(v >= 1 && v <= 65535, "rpt_knn_vote_*: v must be in [1, 65535]");
  RPT_ARG(flags == 0 || flags == RPT_KNN_METRIC_COSINE || flags == RPT_KNN_METRIC_INNER ||
              flags == RPT_KNN_METRIC_REFERENCE,
          "rpt_knn_vote_*: flags is 0 or exactly one of RPT_KNN_METRIC_COSINE / _INNER / _REFERENCE (the threshold "
          "is the argument v, the voted ids are distinct: no duplicate rule)");
  RPT_ARG(!(flags & RPT_KNN_METRIC_REFERENCE) || data->csr,
          "rpt_knn_vote_*: RPT_KNN_METRIC_REFERENCE is the CSR rows' metric");
  return RPT_OK;
}
}  // namespace

extern "C" {

int32_t rpt_knn_vote_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries,
                         int32_t k, int32_t v, int32_t flags, int32_t* ids_dev, double* dist_dev,
                         int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_knn_vote(ctx, f, data, queries, k, v, flags));
    RPT_ARG(ids_dev && dist_dev && count_dev, "NULL output");
    return knn_vote_dev(ctx, f, data, queries, k, v, flags, ids_dev, dist_dev, count_dev);
  });
}

int32_t rpt_knn_vote_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries,
                          int32_t k, int32_t v, int32_t flags, int32_t* ids_host, double* dist_host,
                          int32_t* count_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_knn_vote(ctx, f, data, queries, k, v, flags));
    RPT_ARG(ids_host && dist_host && count_host, "NULL output");
    Triple out;
    RPT_TRY(out.alloc(queries->n, k));
    RPT_TRY(knn_vote_dev(ctx, f, data, queries, k, v, flags, out.ids.p, out.dist.p, out.cnt.p));
    RPT_HIP(stream_sync(ctx->stream));
    return out.download(ids_host, dist_host, count_host);
  });
}

int32_t rpt_vote_candidates_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* queries, int32_t v,
                                 int64_t* off_host, int32_t* ids_host, int32_t* counts_host, int64_t cap,
                                 int64_t* total) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(total, "total is NULL");
    RPT_ARG(v >= 1 && v <= 65535, "rpt_vote_candidates_host: v must be in [1, 65535]");
    return vote_candidates(ctx, f, queries, v, off_host, ids_host, counts_host, cap, total);
  });
}

int32_t rpt_knn_last_voted(rpt_ctx* ctx, int64_t* total) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && total, "NULL argument");
    *total = ctx->last_voted;
    return RPT_OK;
  });
}

}  // extern "C"

// ---- an allow-list on the forest query and on the exhaustive kNN ----------------------------------
namespace {
// the metric part of the rpt_*_allow_* flags: 0 or exactly one of RPT_KNN_METRIC_COSINE / _INNER /
// _REFERENCE, the last on CSR rows only
int32_t check_allow_metric(const rpt_dataset* data, int32_t flags) {
  const int32_t metric = flags & (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER);
  RPT_ARG(metric != (RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER),
          "RPT_KNN_METRIC_COSINE and RPT_KNN_METRIC_INNER are exclusive");
  RPT_ARG(!metric || !(flags & RPT_KNN_METRIC_REFERENCE),
          "RPT_KNN_METRIC_REFERENCE is an L2 metric: not with RPT_KNN_METRIC_COSINE / _INNER");
  RPT_ARG(!(flags & RPT_KNN_METRIC_REFERENCE) || data->csr, "RPT_KNN_METRIC_REFERENCE is the CSR rows' metric");
  return RPT_OK;
}

int32_t check_knn_allow(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries, int32_t k,
                        int32_t flags) {
  RPT_TRY(check_query(ctx, f, queries));
  RPT_ARG(data && data->ctx == ctx, "bad data handle");
  RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
  RPT_ARG(data->csr == queries->csr, "data and queries must both be dense or both CSR");
  RPT_ARG(data->dtype == queries->dtype, "data and query dtype must match");
  RPT_ARG(proj_dtype(queries->dtype) == f->pdtype,
          "query dtype must have the forest's projection type (f64 vs f32/bf16)");
  RPT_ARG(k >= 1 && k <= 1024, "k must be in [1,1024]");
  RPT_TRY(check_knn_flags(flags));  // rpt_knn_*'s own refusals, with their codes
  if ((flags >> 8) & 0xffff)
    return fail(RPT_E_UNSUPPORTED, "rpt_knn_allow_*: no voting (RPT_KNN_VOTE) under an allow-list");
  return check_allow_metric(data, flags);
}

int32_t check_brute_allow(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries, int32_t k,
                          int32_t flags) {
  RPT_ARG(ctx && data && queries, "NULL argument");
  RPT_ARG(data->ctx == ctx && queries->ctx == ctx, "handles belong to another context");
  RPT_ARG(data->csr == queries->csr, "data and queries must both be dense or both CSR");
  RPT_ARG(data->d == queries->d && data->dtype == queries->dtype, "shape/dtype mismatch");
  RPT_ARG(k >= 1 && k <= 1024, "k must be in [1,1024]");
  RPT_ARG(flags >= 0 && (flags & ~(RPT_KNN_METRIC_COSINE | RPT_KNN_METRIC_INNER | RPT_KNN_METRIC_REFERENCE)) == 0,
          "rpt_brute_knn_allow_*: flags is 0 or one of RPT_KNN_METRIC_COSINE / _INNER / _REFERENCE");
  RPT_TRY(check_allow_metric(data, flags));
  RPT_HIP(hipSetDevice(ctx->device));
  return RPT_OK;
}

// the ceil(n / 32) words of a host bitmap on the device (null stays null: every id)
int32_t upload_allow(const uint32_t* allow_host, int64_t n, DevBuf<uint32_t>& bitmap, const uint32_t** allow_dev) {
  *allow_dev = nullptr;
  const size_t words = allow_host ? (size_t)((n + 31) / 32) : 0;
  if (!words) return RPT_OK;
  RPT_TRY(bitmap.alloc(words));
  RPT_HIP(hipMemcpy(bitmap.p, allow_host, words * 4, hipMemcpyHostToDevice));
  *allow_dev = bitmap.p;
  return RPT_OK;
}
}  // namespace

extern "C" {

int32_t rpt_knn_allow_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries,
                          const uint32_t* allow_dev, int32_t k, int32_t flags, int32_t* ids_dev, double* dist_dev,
                          int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_knn_allow(ctx, f, data, queries, k, flags));
    RPT_ARG(ids_dev && dist_dev && count_dev, "NULL output");
    return knn_allow_dev(ctx, f, data, queries, one_bitmap(allow_dev), k, flags, ids_dev, dist_dev, count_dev);
  });
}

int32_t rpt_knn_allow_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries,
                           const uint32_t* allow_host, int32_t k, int32_t flags, int32_t* ids_host,
                           double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_knn_allow(ctx, f, data, queries, k, flags));
    RPT_ARG(ids_host && dist_host && count_host, "NULL output");
    DevBuf<uint32_t> bitmap;
    const uint32_t* allow_dev = nullptr;
    RPT_TRY(upload_allow(allow_host, data->n, bitmap, &allow_dev));
    Triple out;
    RPT_TRY(out.alloc(queries->n, k));
    RPT_TRY(knn_allow_dev(ctx, f, data, queries, one_bitmap(allow_dev), k, flags, out.ids.p, out.dist.p, out.cnt.p));
    RPT_HIP(stream_sync(ctx->stream));
    return out.download(ids_host, dist_host, count_host);
  });
}

int32_t rpt_allow_candidates_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* queries,
                                  const uint32_t* allow_host, int64_t* off_host, int32_t* ids_host, int64_t cap,
                                  int64_t* total) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(total, "total is NULL");
    DevBuf<uint32_t> bitmap;
    const uint32_t* allow_dev = nullptr;
    RPT_TRY(upload_allow(allow_host, f->n, bitmap, &allow_dev));
    return allow_candidates(ctx, f, queries, one_bitmap(allow_dev), off_host, ids_host, cap, total);
  });
}

int32_t rpt_brute_knn_allow_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                const uint32_t* allow_dev, int32_t k, int32_t flags, int32_t* ids_dev,
                                double* dist_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ids_dev && dist_dev, "NULL output");
    RPT_TRY(check_brute_allow(ctx, data, queries, k, flags));
    return brute_knn_allow_dev(ctx, data, queries, allow_dev, k, flags, ids_dev, dist_dev);
  });
}

int32_t rpt_brute_knn_allow_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                 const uint32_t* allow_host, int32_t k, int32_t flags, int32_t* ids_host,
                                 double* dist_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ids_host && dist_host, "NULL output");
    RPT_TRY(check_brute_allow(ctx, data, queries, k, flags));
    const int64_t nq = queries->n;
    if (nq == 0) return RPT_OK;
    DevBuf<uint32_t> bitmap;
    const uint32_t* allow_dev = nullptr;
    RPT_TRY(upload_allow(allow_host, data->n, bitmap, &allow_dev));
    DevBuf<int32_t> ids;
    DevBuf<double> dist;
    RPT_TRY(ids.alloc((size_t)nq * k));
    RPT_TRY(dist.alloc((size_t)nq * k));
    RPT_TRY(brute_knn_allow_dev(ctx, data, queries, allow_dev, k, flags, ids.p, dist.p));
    RPT_HIP(hipMemcpy(ids_host, ids.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    RPT_HIP(hipMemcpy(dist_host, dist.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    return RPT_OK;
  });
}

int32_t rpt_recall_hits_allow_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries,
                                   const uint32_t* allow_host, int32_t k, int32_t flags, int32_t* hits_host,
                                   int32_t* truth_ids_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(hits_host, "NULL output");
    RPT_TRY(check_brute_allow(ctx, data, queries, k, flags));
    RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
    RPT_ARG(proj_dtype(queries->dtype) == f->pdtype,
            "query dtype must have the forest's projection type (f64 vs f32/bf16)");
    RPT_ARG(queries->n * (int64_t)f->T <= 0x7fffffff, "too many (query, tree) pairs for one call");
    DevBuf<uint32_t> bitmap;
    const uint32_t* allow_dev = nullptr;
    RPT_TRY(upload_allow(allow_host, data->n, bitmap, &allow_dev));
    return recall_hits_allow(ctx, f, data, queries, one_bitmap(allow_dev), k, flags, hits_host, truth_ids_host);
  });
}

// ---- the same entry points under a grouped allow-list: (allow, G, group) where allow stands above ----
int32_t rpt_knn_allow_group_dev(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries,
                                const uint32_t* allow_dev, int32_t G, const int32_t* group_dev, int32_t k,
                                int32_t flags, int32_t* ids_dev, double* dist_dev, int32_t* count_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_knn_allow(ctx, f, data, queries, k, flags));
    RPT_ARG(ids_dev && dist_dev && count_dev, "NULL output");
    RPT_TRY(check_group_args(allow_dev, G));
    return knn_allow_dev(ctx, f, data, queries, groups_dev(allow_dev, G, group_dev, data->n), k, flags, ids_dev,
                         dist_dev, count_dev);
  });
}

int32_t rpt_knn_allow_group_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data, const rpt_dataset* queries,
                                 const uint32_t* allow_host, int32_t G, const int32_t* group_host, int32_t k,
                                 int32_t flags, int32_t* ids_host, double* dist_host, int32_t* count_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_knn_allow(ctx, f, data, queries, k, flags));
    RPT_ARG(ids_host && dist_host && count_host, "NULL output");
    RPT_TRY(check_group_args(allow_host, G));
    DevBuf<uint32_t> bitmap;
    DevBuf<int32_t> grp;
    AllowGroups ag;
    RPT_TRY(upload_groups(allow_host, G, group_host, data->n, queries->n, bitmap, grp, &ag));
    Triple out;
    RPT_TRY(out.alloc(queries->n, k));
    RPT_TRY(knn_allow_dev(ctx, f, data, queries, ag, k, flags, out.ids.p, out.dist.p, out.cnt.p));
    RPT_HIP(stream_sync(ctx->stream));
    return out.download(ids_host, dist_host, count_host);
  });
}

int32_t rpt_allow_group_candidates_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* queries,
                                        const uint32_t* allow_host, int32_t G, const int32_t* group_host,
                                        int64_t* off_host, int32_t* ids_host, int64_t cap, int64_t* total) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(total, "total is NULL");
    RPT_TRY(check_group_args(allow_host, G));
    DevBuf<uint32_t> bitmap;
    DevBuf<int32_t> grp;
    AllowGroups ag;
    RPT_TRY(upload_groups(allow_host, G, group_host, f->n, queries->n, bitmap, grp, &ag));
    return allow_candidates(ctx, f, queries, ag, off_host, ids_host, cap, total);
  });
}

int32_t rpt_brute_knn_allow_group_dev(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                      const uint32_t* allow_dev, int32_t G, const int32_t* group_dev, int32_t k,
                                      int32_t flags, int32_t* ids_dev, double* dist_dev) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ids_dev && dist_dev, "NULL output");
    RPT_TRY(check_brute_allow(ctx, data, queries, k, flags));
    RPT_TRY(check_group_args(allow_dev, G));
    if (!group_dev) return brute_knn_allow_dev(ctx, data, queries, nullptr, k, flags, ids_dev, dist_dev);
    return brute_knn_allow_group_dev(ctx, data, queries, groups_dev(allow_dev, G, group_dev, data->n), k, flags,
                                     ids_dev, dist_dev);
  });
}

int32_t rpt_brute_knn_allow_group_host(rpt_ctx* ctx, const rpt_dataset* data, const rpt_dataset* queries,
                                       const uint32_t* allow_host, int32_t G, const int32_t* group_host, int32_t k,
                                       int32_t flags, int32_t* ids_host, double* dist_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_ARG(ids_host && dist_host, "NULL output");
    RPT_TRY(check_brute_allow(ctx, data, queries, k, flags));
    RPT_TRY(check_group_args(allow_host, G));
    const int64_t nq = queries->n;
    DevBuf<uint32_t> bitmap;
    DevBuf<int32_t> grp;
    AllowGroups ag;
    RPT_TRY(upload_groups(allow_host, G, group_host, data->n, nq, bitmap, grp, &ag));
    if (nq == 0) return RPT_OK;
    DevBuf<int32_t> ids;
    DevBuf<double> dist;
    RPT_TRY(ids.alloc((size_t)nq * k));
    RPT_TRY(dist.alloc((size_t)nq * k));
    if (!ag.group) RPT_TRY(brute_knn_allow_dev(ctx, data, queries, nullptr, k, flags, ids.p, dist.p));
    else RPT_TRY(brute_knn_allow_group_dev(ctx, data, queries, ag, k, flags, ids.p, dist.p));
    RPT_HIP(hipMemcpy(ids_host, ids.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    RPT_HIP(hipMemcpy(dist_host, dist.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    return RPT_OK;
  });
}

int32_t rpt_recall_hits_allow_group_host(rpt_ctx* ctx, rpt_forest* f, const rpt_dataset* data,
                                         const rpt_dataset* queries, const uint32_t* allow_host, int32_t G,
                                         const int32_t* group_host, int32_t k, int32_t flags, int32_t* hits_host,
                                         int32_t* truth_ids_host) {
  return guarded([&]() -> int32_t {
    if (ctx) dev_set_stream(ctx->stream);
    RPT_TRY(check_query(ctx, f, queries));
    RPT_ARG(hits_host, "NULL output");
    RPT_TRY(check_brute_allow(ctx, data, queries, k, flags));
    RPT_ARG(data->n == f->n && data->d == f->d, "data shape differs from the forest's");
    RPT_ARG(proj_dtype(queries->dtype) == f->pdtype,
            "query dtype must have the forest's projection type (f64 vs f32/bf16)");
    RPT_ARG(queries->n * (int64_t)f->T <= 0x7fffffff, "too many (query, tree) pairs for one call");
    RPT_TRY(check_group_args(allow_host, G));
    DevBuf<uint32_t> bitmap;
    DevBuf<int32_t> grp;
    AllowGroups ag;
    RPT_TRY(upload_groups(allow_host, G, group_host, data->n, queries->n, bitmap, grp, &ag));
    return recall_hits_allow(ctx, f, data, queries, ag, k, flags, hits_host, truth_ids_host);
  });
}

int32_t rpt_knn_allow_last(rpt_ctx* ctx, int64_t* candidates, int64_t* allowed) {
  return guarded([&]() -> int32_t {
    RPT_ARG(ctx && candidates && allowed, "NULL argument");
    *candidates = ctx->last_candidates;
    *allowed = ctx->last_allowed;
    return RPT_OK;
  });
}

}  // extern "C"
