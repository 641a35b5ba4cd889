// pislam_dist.inc — multi-GPU entry points of the C ABI (include/pislam_hip.h, "pislam_dist_*").
// Included by pislam_hip.hip (needs pislam_ctx, fail(), HIPCHK, PISLAM_EXPORT).
//
// One process per GPU; every rank owns a contiguous shard of the batch of independent pyramids
// (SURVEY.md §8e — the reference has no cross-frame state, demo.cpp:77-101 is a pure per-frame loop), so the
// data path needs no collective.  The ONE exchange is the all-gather of the per-pyramid keypoint counts
// (what a consumer needs to place every rank's keypoints in a global list): ncclAllGather over RCCL/xGMI,
// 4 bytes per pyramid, latency-bound.  It runs on the context's own collective stream, ordered after the
// work already enqueued on the context stream, so that it overlaps the next batch call.
//
// RCCL is bound at run time (dlopen "librccl.so.1"): a process that already carries an RCCL (PyTorch
// bundles one with the same soname) keeps exactly one copy, and a single-GPU user never loads it.

#include <chrono>
#include <dlfcn.h>
#include <mutex>
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>   // types and enum values only; no link-time dependency
#else
// A ROCm install without the RCCL development headers still builds the library (a single-GPU user never needs
// RCCL): the few types and constants of the public NCCL ABI that the entry points below use.
extern "C" {
typedef struct ncclComm *ncclComm_t;
#define NCCL_UNIQUE_ID_BYTES 128
typedef struct { char internal[NCCL_UNIQUE_ID_BYTES]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclUint32 = 3, ncclFloat64 = 8 } ncclDataType_t;
typedef enum { ncclMax = 2 } ncclRedOp_t;
}
#endif

namespace {

struct RcclApi {
  void *handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  std::string why;
};

// Bound once per process, thread-safe (contexts are per-thread and may initialise concurrently).
bool rccl_bind(RcclApi &api);
RcclApi *rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] { (void)rccl_bind(api); });
  return api.handle ? &api : nullptr;
}
bool rccl_bind(RcclApi &api) {
  const char *env = getenv("PISLAM_RCCL_LIB");
  const char *names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char *n : names) {
    if (!n || !*n) continue;
    api.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (api.handle) break;
    api.why = dlerror();
  }
  if (!api.handle) return false;
#define PISLAM_RCCL_SYM(field, name)                                   \
  api.field = (decltype(api.field))dlsym(api.handle, name);            \
  if (!api.field) {                                                    \
    api.why = std::string("missing symbol ") + name;                   \
    dlclose(api.handle);                                               \
    api.handle = nullptr;                                              \
    return false;                                                      \
  }
  PISLAM_RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
  PISLAM_RCCL_SYM(CommInitRank, "ncclCommInitRank")
  PISLAM_RCCL_SYM(CommDestroy, "ncclCommDestroy")
  PISLAM_RCCL_SYM(CommCount, "ncclCommCount")
  PISLAM_RCCL_SYM(AllGather, "ncclAllGather")
  PISLAM_RCCL_SYM(AllReduce, "ncclAllReduce")
  PISLAM_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef PISLAM_RCCL_SYM
  return true;
}

int fail_rccl(pislam_ctx *c, const char *what, RcclApi *api, ncclResult_t r) {
  std::string m = what;
  m += ": ";
  m += api && api->GetErrorString ? api->GetErrorString(r) : "RCCL error";
  return fail(c, PISLAM_ERR_DIST, m.c_str());
}

}  // namespace

struct pislam_dist_state {
  int rank = 0, world = 1;
  ncclComm_t comm = nullptr;
  hipStream_t cstream = nullptr;          // the collective stream
  hipEvent_t ready = nullptr;             // ctx stream -> collective stream ordering
  static constexpr int RING = 16;
  hipEvent_t done[RING] = {};             // completion of the last RING collectives
  unsigned long long issued = 0;
  void *scratch = nullptr;                // one double for pislam_dist_allreduce_max
  // PISLAM_DIST_TRACE=1: host microseconds spent inside the four calls of one exchange (record, wait, collective,
  // record), printed by pislam_dist_finalize — a diagnostic for "which call blocks the launch thread"
  bool trace = false;
  double t_host[4] = {0, 0, 0, 0};
};

static inline double dist_now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

PISLAM_EXPORT int pislam_dist_shard(int global_batch, int rank, int world, int *first, int *count) {
  if (global_batch < 0 || world < 1 || rank < 0 || rank >= world || !first || !count) return PISLAM_ERR_INVALID;
  const int base = global_batch / world, rem = global_batch % world;   // the first `rem` ranks take one more
  *first = rank * base + std::min(rank, rem);
  *count = base + (rank < rem ? 1 : 0);
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_dist_get_unique_id(uint8_t id[PISLAM_DIST_ID_BYTES]) {
  static_assert(PISLAM_DIST_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
  if (!id) return PISLAM_ERR_INVALID;
  RcclApi *api = rccl_api();
  if (!api) return PISLAM_ERR_DIST;
  ncclUniqueId u;
  if (api->GetUniqueId(&u) != ncclSuccess) return PISLAM_ERR_DIST;
  memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_dist_finalize(pislam_ctx *c) {
  if (!c) return PISLAM_ERR_INVALID;
  pislam_dist_state *d = c->dist;
  if (!d) return PISLAM_OK;
  (void)hipSetDevice(c->device);
  if (d->cstream) (void)hipStreamSynchronize(d->cstream);
  if (d->trace && d->issued)
    fprintf(stderr, "[pislam_dist rank %d] %llu exchanges, host us per call: hipEventRecord(launch stream) %.1f, "
                    "hipStreamWaitEvent(collective stream) %.1f, collective %.1f, hipEventRecord(collective stream) %.1f\n",
            d->rank, d->issued, d->t_host[0] / d->issued, d->t_host[1] / d->issued, d->t_host[2] / d->issued,
            d->t_host[3] / d->issued);
  if (d->comm) {
    RcclApi *api = rccl_api();
    if (api) (void)api->CommDestroy(d->comm);
  }
  if (d->ready) (void)hipEventDestroy(d->ready);
  for (auto &e : d->done)
    if (e) (void)hipEventDestroy(e);
  if (d->cstream) (void)hipStreamDestroy(d->cstream);
  if (d->scratch) (void)hipFree(d->scratch);
  delete d;
  c->dist = nullptr;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_dist_init(pislam_ctx *c, const uint8_t id[PISLAM_DIST_ID_BYTES], int rank, int world) {
  if (!c) return PISLAM_ERR_INVALID;
  if (world < 1 || rank < 0 || rank >= world) return fail(c, PISLAM_ERR_INVALID, "bad rank / world");
  if ((world > 1 || c->opt.dist_rccl_single) && !id) return fail(c, PISLAM_ERR_INVALID, "null unique id");
  if (c->dist) PCHK(pislam_dist_finalize(c));
  HIPCHK(c, hipSetDevice(c->device));
  pislam_dist_state *d = new pislam_dist_state();
  d->rank = rank;
  d->world = world;
  d->trace = getenv("PISLAM_DIST_TRACE") != nullptr;
  c->dist = d;
  hipError_t e = hipStreamCreateWithFlags(&d->cstream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ready, hipEventDisableTiming);
  for (int i = 0; i < pislam_dist_state::RING && e == hipSuccess; i++)
    e = hipEventCreateWithFlags(&d->done[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&d->scratch, 2 * sizeof(double));
  if (e != hipSuccess) {
    (void)pislam_dist_finalize(c);
    return fail(c, PISLAM_ERR_HIP, "pislam_dist_init: stream / event creation", e);
  }
  // degrades to a single GPU without touching RCCL (SURVEY §8e); the test hook "dist_rccl_single" keeps the
  // RCCL path (a 1-rank communicator) so that it can be exercised on a 1-GPU box
  if (world == 1 && !c->opt.dist_rccl_single) return PISLAM_OK;
  RcclApi *api = rccl_api();
  if (!api) {
    (void)pislam_dist_finalize(c);
    return fail(c, PISLAM_ERR_DIST, "RCCL (librccl.so.1) could not be loaded");
  }
  ncclUniqueId u;
  memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  const ncclResult_t r = api->CommInitRank(&d->comm, world, u, rank);
  if (r != ncclSuccess) {
    d->comm = nullptr;
    (void)pislam_dist_finalize(c);
    return fail_rccl(c, "ncclCommInitRank", api, r);
  }
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_dist_rank(const pislam_ctx *c) { return c && c->dist ? c->dist->rank : 0; }
PISLAM_EXPORT int pislam_dist_world(const pislam_ctx *c) { return c && c->dist ? c->dist->world : 1; }

// What RCCL itself says (ncclCommCount), not what the caller passed in: 0 without a communicator (single GPU,
// or pislam_dist_init not called), negative on an RCCL error.
PISLAM_EXPORT int pislam_dist_comm_count(pislam_ctx *c) {
  if (!c) return PISLAM_ERR_INVALID;
  pislam_dist_state *d = c->dist;
  if (!d || !d->comm) return 0;
  RcclApi *api = rccl_api();
  int n = 0;
  const ncclResult_t r = api->CommCount(d->comm, &n);
  if (r != ncclSuccess) return fail_rccl(c, "ncclCommCount", api, r);
  return n;
}

PISLAM_EXPORT int pislam_dist_allgather_counts_on(pislam_ctx *c, void *producer_stream, const uint32_t *local_counts,
                                                  size_t n, uint32_t *all_counts) {
  if (!c) return PISLAM_ERR_INVALID;
  pislam_dist_state *d = c->dist;
  if (!d) return fail(c, PISLAM_ERR_INVALID, "pislam_dist_init has not been called on this context");
  if (n == 0) return PISLAM_OK;
  if (!local_counts || !all_counts) return fail(c, PISLAM_ERR_INVALID, "null pointer");
  if (!is_device_ptr(local_counts) || !is_device_ptr(all_counts))
    return fail(c, PISLAM_ERR_INVALID, "the count all-gather takes device pointers only");
  HIPCHK(c, hipSetDevice(c->device));
  // ordered after everything the producer stream holds so far (the batch call that produces the counts)
  double t0 = d->trace ? dist_now_us() : 0, t1;
  auto lap = [&](int k) {
    if (!d->trace) return;
    t1 = dist_now_us();
    d->t_host[k] += t1 - t0;
    t0 = t1;
  };
  HIPCHK(c, hipEventRecord(d->ready, (hipStream_t)producer_stream));
  lap(0);
  HIPCHK(c, hipStreamWaitEvent(d->cstream, d->ready, 0));
  lap(1);
  if (!d->comm) {
    if (all_counts != local_counts)
      HIPCHK(c, hipMemcpyAsync(all_counts, local_counts, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, d->cstream));
  } else {
    RcclApi *api = rccl_api();
    const ncclResult_t r = api->AllGather(local_counts, all_counts, n, ncclUint32, d->comm, d->cstream);
    if (r != ncclSuccess) return fail_rccl(c, "ncclAllGather", api, r);
  }
  lap(2);
  HIPCHK(c, hipEventRecord(d->done[d->issued % pislam_dist_state::RING], d->cstream));
  lap(3);
  d->issued++;
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_dist_allgather_counts(pislam_ctx *c, const uint32_t *local_counts, size_t n,
                                               uint32_t *all_counts) {
  if (!c) return PISLAM_ERR_INVALID;
  return pislam_dist_allgather_counts_on(c, (void *)c->stream, local_counts, n, all_counts);
}

PISLAM_EXPORT int pislam_dist_fence_on(pislam_ctx *c, int back, void *consumer_stream) {
  if (!c) return PISLAM_ERR_INVALID;
  pislam_dist_state *d = c->dist;
  if (!d) return fail(c, PISLAM_ERR_INVALID, "pislam_dist_init has not been called on this context");
  if (back < 1) return fail(c, PISLAM_ERR_INVALID, "back must be >= 1");
  if (d->issued < (unsigned long long)back) return PISLAM_OK;          // nothing that old was ever issued
  // The collective stream is in order: a collective issued later than the one asked for completes after it, so
  // when that one's event slot has been reused (back > RING) waiting for the oldest kept event still covers it.
  back = std::min(back, (int)pislam_dist_state::RING);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamWaitEvent((hipStream_t)consumer_stream, d->done[(d->issued - back) % pislam_dist_state::RING], 0));
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_dist_fence(pislam_ctx *c, int back) {
  if (!c) return PISLAM_ERR_INVALID;
  return pislam_dist_fence_on(c, back, (void *)c->stream);
}

PISLAM_EXPORT int pislam_dist_synchronize(pislam_ctx *c) {
  if (!c) return PISLAM_ERR_INVALID;
  pislam_dist_state *d = c->dist;
  if (!d) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(d->cstream));
  return PISLAM_OK;
}

PISLAM_EXPORT int pislam_dist_allreduce_max(pislam_ctx *c, double *value) {
  if (!c || !value) return PISLAM_ERR_INVALID;
  pislam_dist_state *d = c->dist;
  if (!d) return fail(c, PISLAM_ERR_INVALID, "pislam_dist_init has not been called on this context");
  if (!d->comm) return PISLAM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  RcclApi *api = rccl_api();
  double *s = (double *)d->scratch;
  HIPCHK(c, hipMemcpyAsync(s, value, sizeof(double), hipMemcpyHostToDevice, d->cstream));
  const ncclResult_t r = api->AllReduce(s, s + 1, 1, ncclFloat64, ncclMax, d->comm, d->cstream);
  if (r != ncclSuccess) return fail_rccl(c, "ncclAllReduce", api, r);
  HIPCHK(c, hipMemcpyAsync(value, s + 1, sizeof(double), hipMemcpyDeviceToHost, d->cstream));
  HIPCHK(c, hipStreamSynchronize(d->cstream));
  return PISLAM_OK;
}
