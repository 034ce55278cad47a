// rrtmg_abi.hip -- extern "C" surface of librrtmg_hip.so (declared in include/rrtmg_hip.h).
#include <dlfcn.h>
#include <pthread.h>

#include <cstring>
#include <mutex>

#include <atomic>
#include <condition_variable>
#include <memory>

#include <cstddef>

#include "rrtmg_ctx.h"

namespace rrtmg {

const char *status_message(int code) {
  switch (code) {
    case RRTMG_OK: return "ok";
    case RRTMG_ERR_HIP: return "HIP runtime error";
    case RRTMG_ERR_NOT_INITIALISED: return "not initialised";
    case RRTMG_ERR_TABLES: return "table blob error";
    case RRTMG_ERR_ARG: return "bad argument";
    case RRTMG_ERR_PARTIAL_CLOUD: return "PARTIAL CLOUD NOT ALLOWED";
    case RRTMG_ERR_ICE_RADIUS: return "ICE RADIUS OUT OF BOUNDS";
    case RRTMG_ERR_LIQ_RADIUS: return "LIQUID EFFECTIVE RADIUS OUT OF BOUNDS";
    case RRTMG_ERR_KISS_PRESSURE: return "MCICA_SUBCOL: KISSVEC SEED GENERATOR REQUIRES PMID FROM BOTTOM FOUR LAYERS.";
    case RRTMG_ERR_ICLD: return "MCICA_SUBCOL: INVALID ICLD";
    case RRTMG_ERR_INFLAG1_MCICA: return "INFLAG = 1 OPTION NOT AVAILABLE WITH MCICA";
    case RRTMG_ERR_ICE_GEN_SIZE: return "ICE GENERALIZED EFFECTIVE SIZE OUT OF BOUNDS";
    case RRTMG_ERR_ICE_RADIUS_SMALL: return "ICE RADIUS TOO SMALL";
    case RRTMG_ERR_UNSUPPORTED: return "option not supported by RRTMG";
    case RRTMG_ERR_ICE_EXT_NEG: return "ICE EXTINCTION LESS THAN 0.0";
    case RRTMG_ERR_ICE_SSA_GT1: return "ICE SSA GRTR THAN 1.0";
    case RRTMG_ERR_ICE_SSA_NEG: return "ICE SSA LESS THAN 0.0";
    case RRTMG_ERR_ICE_ASYM_GT1: return "ICE ASYM GRTR THAN 1.0";
    case RRTMG_ERR_ICE_ASYM_NEG: return "ICE ASYM LESS THAN 0.0";
    case RRTMG_ERR_FDELTA_NEG: return "FDELTA LESS THAN 0.0";
    case RRTMG_ERR_FDELTA_GT1: return "FDELTA GT THAN 1.0";
    case RRTMG_ERR_LIQ_EXT_NEG: return "LIQUID EXTINCTION LESS THAN 0.0";
    case RRTMG_ERR_LIQ_SSA_GT1: return "LIQUID SSA GRTR THAN 1.0";
    case RRTMG_ERR_LIQ_SSA_NEG: return "LIQUID SSA LESS THAN 0.0";
    case RRTMG_ERR_LIQ_ASYM_GT1: return "LIQUID ASYM GRTR THAN 1.0";
    case RRTMG_ERR_LIQ_ASYM_NEG: return "LIQUID ASYM LESS THAN 0.0";
    default: return "unknown error";
  }
}

int ctx_prepare_device(rrtmg_ctx *ctx) {
  RRTMG_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!ctx->stream) RRTMG_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  if (!ctx->stream_lw) RRTMG_HIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->stream_lw, hipStreamNonBlocking));
  if (!ctx->hint) {
    RRTMG_HIP_CHECK(ctx, hipHostMalloc((void **)&ctx->hint, 2 * sizeof(rrtmg_ctx::CallHint) + 2 * sizeof(int), hipHostMallocDefault));   // (+ rrtmg_ctx::night_host)
    for (int w = 0; w < 2; ++w) { ctx->hint[w].ntile = -1; ctx->hint[w].nlay = -1; ctx->hint[w].ncloudy = -1; }
    ctx->night_host()[0] = 0; ctx->night_host()[1] = 0;
    RRTMG_HIP_CHECK(ctx, hipMalloc((void **)&ctx->ncloudy_dev, 4 * sizeof(int)));
    RRTMG_HIP_CHECK(ctx, hipMemset(ctx->ncloudy_dev, 0, 4 * sizeof(int)));
  }
  if (!ctx->flag_host) {
    RRTMG_HIP_CHECK(ctx, hipHostMalloc((void **)&ctx->flag_host, 2 * sizeof(int), hipHostMallocDefault));
    ctx->flag_host[0] = ctx->flag_host[1] = 0;
  }
  if (!ctx->err_dev) {
    RRTMG_HIP_CHECK(ctx, hipMalloc((void **)&ctx->err_dev, 64));
    RRTMG_HIP_CHECK(ctx, hipMemset(ctx->err_dev, 0, 64));
  }
  for (int w = 0; w < 2; ++w)
    for (int k = 0; k < 2; ++k)
      if (!ctx->kiss_ev[w][k]) RRTMG_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->kiss_ev[w][k], hipEventDisableTiming));
  for (int w = 0; w < 2; ++w)
    if (!ctx->sync_ev[w]) RRTMG_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->sync_ev[w], hipEventDisableTiming));
  for (int w = 0; w < 2; ++w)
    if (!ctx->share_ev[w]) RRTMG_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->share_ev[w], hipEventDisableTiming));
  for (int w = 0; w < 2; ++w)
    if (!ctx->alpha_ev[w]) RRTMG_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->alpha_ev[w], hipEventDisableTiming));
  return RRTMG_OK;
}

int copy_out_enqueue(rrtmg_ctx *ctx, hipStream_t s, const OutCopy *o, int count, int *herr_dev, PendingOut &po, int slot) {
  // A destination that is page-locked memory the runtime knows (hipHostMalloc / hipHostRegister: the components' output pool
  // hands such arrays out) takes its copy directly; the others go through the staging buffer.
  if (count > kMaxOut) return ctx->fail(RRTMG_ERR_ARG, "copy_out: %d output arrays (at most %d)", count, kMaxOut);
  // A float32-boundary call (ctx->f32): ONE narrow launch on s for all the outputs, into a float staging buffer of the device;
  // what comes down, and what the caller's arrays hold, are 4 n bytes each.
  const size_t elem = ctx->f32 ? sizeof(float) : sizeof(double);
  po.count = count; po.total = 0; po.herr = 0; po.slot = slot; po.has_flag = herr_dev != nullptr; po.enqueued = false; po.elem = elem;
  size_t all = 0;
  for (int i = 0; i < count; ++i) {
    hipPointerAttribute_t at;
    po.oc[i] = o[i];
    po.direct[i] = hipPointerGetAttributes(&at, o[i].host) == hipSuccess && at.type == hipMemoryTypeHost;
    if (!po.direct[i]) po.total += o[i].n * elem;
    all += (o[i].n + 3) / 4 * 4;   // (every output starts 16-byte aligned in the float staging buffer)
  }
  (void)hipGetLastError();   // (an unknown pointer is an error code of the query, not of this call)
  if (po.total > ctx->pinned_cap[slot]) {
    if (ctx->pinned[slot]) (void)hipHostFree(ctx->pinned[slot]);
    ctx->pinned[slot] = nullptr; ctx->pinned_cap[slot] = 0;
    RRTMG_HIP_CHECK(ctx, hipHostMalloc(&ctx->pinned[slot], po.total, hipHostMallocDefault));
    ctx->pinned_cap[slot] = po.total;
  }
  char *p = (char *)ctx->pinned[slot];
  if (herr_dev) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(&ctx->flag_host[slot], herr_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  const float *narrow = nullptr;
  if (ctx->f32 && all) {
    float *q = (float *)ctx->buf(slot == 0 ? "out.f32.0" : "out.f32.1", all * sizeof(float));
    if (!q) return ctx->status;
    PrecisionBatch nb(s, false);
    size_t at = 0;
    for (int i = 0; i < count; ++i) { nb.add(o[i].dev, q + at, o[i].n); at += (o[i].n + 3) / 4 * 4; }
    nb.flush();
    narrow = q;
  }
  size_t off = 0, at = 0;
  for (int i = 0; i < count; ++i) {
    const void *dev = narrow ? (const void *)(narrow + at) : (const void *)o[i].dev;
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(po.direct[i] ? (char *)o[i].host : p + off, dev, o[i].n * elem, hipMemcpyDeviceToHost, s));
    if (!po.direct[i]) off += o[i].n * elem;
    at += (o[i].n + 3) / 4 * 4;
  }
  po.enqueued = true;
  return RRTMG_OK;
}

void copy_out_complete(rrtmg_ctx *ctx, PendingOut &po) {
  po.enqueued = false;
  if (po.has_flag) po.herr = ctx->flag_host[po.slot];
  const size_t total = po.total;
  const int count = po.count;
  const OutCopy *o = po.oc;
  const bool *direct = po.direct;
  const char *p = (const char *)ctx->pinned[po.slot];
  if (total == 0) return;
  // pinned staging -> the caller's arrays, in slices on a few host threads (first touch of fresh pages dominates)
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt == 0 ? 1 : (nt > 8 ? 8 : nt);
  if (total < (size_t)4 << 20) nt = 1;
  std::vector<std::thread> th;
  auto work = [&](unsigned t) {
    size_t off2 = 0;
    for (int i = 0; i < count; ++i) {
      if (direct[i]) continue;
      const size_t bytes = o[i].n * po.elem, per = (bytes / nt + 4095) & ~(size_t)4095;
      const size_t lo = (size_t)t * per, hi = lo + per < bytes ? lo + per : bytes;
      if (lo < bytes) memcpy((char *)o[i].host + lo, p + off2 + lo, hi - lo);
      off2 += bytes;
    }
  };
  for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
  work(0);
  for (auto &x : th) x.join();
}

int copy_out(rrtmg_ctx *ctx, hipStream_t s, const OutCopy *o, int count, int *herr_dev, int *herr_host) {
  PendingOut po;
  if (const int rc = copy_out_enqueue(ctx, s, o, count, herr_dev, po, 0)) return rc;
  RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  copy_out_complete(ctx, po);
  if (herr_dev) *herr_host = po.herr;
  return RRTMG_OK;
}

// ---- host-pointer inputs (rrtmg_host_inputs.h) ---------------------------------------------------------------------------
namespace {
// A few persistent host threads that scan input arrays (created on first use, never joined: they sleep between calls and
// end with the process).  The caller of wait() works its OWN batch's queue too, so a batch completes even in a process whose
// pool has no workers, and never pays for another context's batch.  fork(): the child gets a fresh pool (pthread_atfork child
// handler: new mutex, empty queue, workers started on first use) -- the parent's may have been locked by a thread that does
// not exist in the child.
struct ScanJob {
  const uint64_t *q = nullptr;
  size_t n = 0;
  uint64_t first = 0;
  std::atomic<bool> differs{false};
};
constexpr size_t kSliceWords = (size_t)1 << 16;   // 512 KB per task
class HostPool {
 public:
  struct Task { ScanJob *job; size_t lo; };
  // A batch owns its slices: `next` is a cursor into `tasks` (both under the pool's mutex), so the waiter takes from its OWN
  // batch and a worker from the newest batch that has any left in O(1) -- no scan of, and no erase from, a queue shared by
  // every context while the workers need the same lock.
  struct Batch { std::atomic<long> open{0}; std::vector<Task> tasks; size_t next = 0; };
  static HostPool &get() {
    HostPool *p = g_pool.load(std::memory_order_acquire);
    if (p) return *p;
    static std::once_flag atfork_once;
    std::call_once(atfork_once, [] { pthread_atfork(nullptr, nullptr, [] { g_pool.store(nullptr, std::memory_order_release); }); });
    HostPool *fresh = new HostPool();   // (no threads yet: a pool that loses the race below is simply deleted)
    HostPool *expected = nullptr;
    if (g_pool.compare_exchange_strong(expected, fresh, std::memory_order_acq_rel)) { fresh->start_workers(); return *fresh; }
    delete fresh;
    return *expected;
  }
  void start(ScanJob *jobs, int njobs, Batch &b) {
    std::lock_guard<std::mutex> lk(m_);
    for (int j = 0; j < njobs; ++j)
      for (size_t lo = 0; lo < jobs[j].n; lo += kSliceWords) b.tasks.push_back(Task{&jobs[j], lo});
    b.open.store((long)b.tasks.size(), std::memory_order_release);
    if (!b.tasks.empty()) { active_.push_back(&b); cv_.notify_all(); }
  }
  void wait(Batch &b) {
    for (;;) {   // help with THIS batch's slices until none is left to hand out ...
      Task t;
      {
        std::lock_guard<std::mutex> lk(m_);
        if (!take(&b, t)) break;
      }
      run(t, b);
    }
    std::unique_lock<std::mutex> lk(m_);   // ... then sleep until the workers have handed in the slices they still hold
    done_.wait(lk, [&b] { return b.open.load(std::memory_order_acquire) <= 0; });
  }

 private:
  HostPool() = default;
  // (m_ held) the batch's next slice; a batch that has handed out its last one leaves active_ at once -- it is in there only
  // while it has slices (active_ holds one entry per context that is scanning right now)
  bool take(Batch *b, Task &t) {
    if (b->next >= b->tasks.size()) return false;
    t = b->tasks[b->next++];
    if (b->next >= b->tasks.size())
      for (size_t i = active_.size(); i-- > 0;)
        if (active_[i] == b) { active_.erase(active_.begin() + (long)i); break; }
    return true;
  }
  void start_workers() {
    unsigned n = std::thread::hardware_concurrency();
    n = n <= 2 ? 1 : (n / 2 > 16 ? 16 : n / 2);
    if (const char *env = getenv("RRTMG_HIP_HOST_THREADS")) { const int v = atoi(env); if (v >= 0 && v <= 64) n = (unsigned)v; }
    for (unsigned i = 0; i < n; ++i) std::thread([this] { loop(); }).detach();
  }
  void loop() {
    for (;;) {
      Task t;
      Batch *b;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return !active_.empty(); });
        b = active_.back();
        if (!take(b, t)) continue;   // (cannot happen: a batch is in active_ only while it has slices)
      }
      run(t, *b);
    }
  }
  void run(const Task &t, Batch &b) {
    ScanJob &j = *t.job;
    const size_t hi = t.lo + kSliceWords < j.n ? t.lo + kSliceWords : j.n;
    for (size_t i = t.lo; i < hi && !j.differs.load(std::memory_order_relaxed); i += 4096) {
      const size_t e = i + 4096 < hi ? i + 4096 : hi;
      uint64_t acc = 0;
      for (size_t k = i; k < e; ++k) acc |= j.q[k] ^ j.first;
      if (acc) j.differs.store(true, std::memory_order_relaxed);
    }
    if (b.open.fetch_sub(1, std::memory_order_acq_rel) == 1) {   // the batch's last slice: wake its waiter (b is not touched again)
      std::lock_guard<std::mutex> lk(m_);
      done_.notify_all();
    }
  }
  static std::atomic<HostPool *> g_pool;
  std::mutex m_;
  std::condition_variable cv_, done_;
  std::vector<Batch *> active_;
};
std::atomic<HostPool *> HostPool::g_pool{nullptr};
}  // namespace

void HostInputs::add(const double **slot, const double *host, size_t n, const char *name, bool required, InPolicy policy, double mul, double div) {
  *slot = nullptr;
  if (!host) {
    if (required) { ctx_->fail(RRTMG_ERR_ARG, "required array '%s' is NULL", name); ok_ = false; }
    return;
  }
  if (memspace_ == 1) { *slot = host; return; }   // device pointers are used as they are
  Entry e{slot, host, n, name, policy, mul, div};
  e.f32 = f32_;
  entries_.push_back(e);
}

bool HostInputs::upload(const Entry &e) {
  const std::string key = std::string(prefix_) + e.name;
  double *dp = (double *)ctx_->buf(key, e.n * sizeof(double));
  if (!dp) return false;
  ctx_->bufs[key].uniform = false;
  if (e.f32) {   // 4 n bytes up into the staging buffer; widened, with the unit factor, by the batch's one launch (finish)
    float *st = (float *)ctx_->buf(key + ".f32", e.n * sizeof(float));
    if (!st) return false;
    if (hipMemcpyAsync(st, e.host, e.n * sizeof(float), hipMemcpyHostToDevice, s_) != hipSuccess) { ctx_->fail(RRTMG_ERR_HIP, "H2D copy of '%s' failed", e.name); return false; }
    widen_.add(st, dp, e.n, e.mul, e.div);
    *e.slot = dp;
    resolved(e, dp, e.n * sizeof(float));
    return true;
  }
  if (hipMemcpyAsync(dp, e.host, e.n * sizeof(double), hipMemcpyHostToDevice, s_) != hipSuccess) { ctx_->fail(RRTMG_ERR_HIP, "H2D copy of '%s' failed", e.name); return false; }
  if (e.mul != 0.0) launch_scale(s_, dp, e.n, e.mul, e.div);
  *e.slot = dp;
  resolved(e, dp, e.n * sizeof(double));
  return true;
}

bool HostInputs::fill(const Entry &e, double host_value) {
  // the value numpy would have formed on the host: one rounding per operation
  volatile double v = host_value;
  if (e.mul != 0.0) { v = v * e.mul; if (e.div != 0.0) v = v / e.div; }
  const double value = v;
  const std::string key = std::string(prefix_) + e.name;
  double *dp = (double *)ctx_->buf(key, e.n * sizeof(double));
  if (!dp) return false;
  DevBuf &b = ctx_->bufs[key];
  if (!(b.uniform && b.uni_n == e.n && memcmp(&b.uni_value, &value, sizeof value) == 0)) {
    launch_fill(s_, dp, e.n, value);
    b.uniform = true; b.uni_value = value; b.uni_n = e.n;
  }
  *e.slot = dp;
  resolved(e, dp, 0);
  return true;
}

bool HostInputs::finish() {
  if (!ok_) return false;
  // a joint call's table first: what it already holds, or what an earlier input of this batch is about to bring, is taken below
  bool brought = false;
  if (share_)
    for (Entry &e : entries_) {
      e.taken = share_->acquire(share_key(e.host, e.n, e.mul, e.div, (int)e.policy, e.f32 ? 4 : 8), owner_, &e.share) != ShareTable::Found::New;
      if (!e.taken) brought = true;
    }
  std::unique_ptr<ScanJob[]> jobs(new ScanJob[entries_.size() + 1]);
  int njobs = 0;
  for (Entry &e : entries_) {
    if (e.taken || e.n < kScanMin) continue;
    const uint64_t *q = (const uint64_t *)e.host;
    size_t nq = e.n;
    uint64_t w0;
    uint64_t acc = 0;
    if (e.f32) {
      // 4-byte patterns, compared two at a time: the words from the first 8-byte aligned element on, against the first
      // element's pattern twice; the odd element behind them on its own
      const uint32_t *f = (const uint32_t *)e.host;
      const size_t skip = ((uintptr_t)f & 7) ? 1 : 0;
      q = (const uint64_t *)(f + skip); nq = (e.n - skip) / 2;
      w0 = (uint64_t)f[0] | (uint64_t)f[0] << 32;
      if ((e.n - skip) & 1) acc |= f[e.n - 1] ^ f[0];
    } else {
      w0 = q[0];
    }
    for (size_t i = 0; i < 2048; ++i) acc |= q[i] ^ w0;                       // the head ...
    for (size_t k = 1; k <= 16; ++k) acc |= q[(nq - 1) / 16 * k] ^ w0;         // ... and sixteen places further on
    if (acc) continue;                                                         // certainly not uniform: goes up at once
    e.job = njobs;
    jobs[njobs].q = q; jobs[njobs].n = nq; jobs[njobs].first = w0;
    ++njobs;
  }
  HostPool::Batch batch;
  if (njobs) HostPool::get().start(jobs.get(), njobs, batch);
  for (const Entry &e : entries_)
    if (!e.taken && e.job < 0 && !upload(e)) ok_ = false;
  if (njobs) HostPool::get().wait(batch);
  for (const Entry &e : entries_) {
    if (e.job < 0) continue;
    const ScanJob &j = jobs[e.job];
    if (j.differs.load()) { if (!upload(e)) ok_ = false; continue; }
    if (e.policy == InPolicy::ZeroAbsent && j.first == 0) { *e.slot = nullptr; resolved(e, nullptr, 0); continue; }   // all +0.0 (+0.0f): the "array absent" path adds the same
    double v;
    if (e.f32) { float f; memcpy(&f, &j.first, sizeof f); v = (double)f; }   // (exact: fill() applies the factors to it as to a double)
    else memcpy(&v, &j.first, sizeof v);
    if (!fill(e, v)) ok_ = false;
  }
  widen_.flush();   // behind every upload of the batch, in front of what the call enqueues next and of the table's event
  if (!share_) return ok_;
  // One event behind the last write of this batch into a buffer the table names; a batch that takes what the OTHER spectrum's
  // stream wrote waits for that spectrum's event on its own stream (what its own stream wrote is ordered already).
  if (brought && hipEventRecord(ctx_->share_ev[owner_], s_) != hipSuccess) { ctx_->fail(RRTMG_ERR_HIP, "hipEventRecord failed (shared inputs)"); ok_ = false; }
  bool wait_other = false;
  for (const Entry &e : entries_) {
    if (!e.taken) continue;
    if (!share_->resolved(e.share)) { ok_ = false; continue; }   // (its first upload failed: ctx says why)
    *e.slot = share_->take(e.share);
    if (share_->owner_of(e.share) != owner_) wait_other = true;
  }
  if (wait_other && hipStreamWaitEvent(s_, ctx_->share_ev[1 - owner_], 0) != hipSuccess) { ctx_->fail(RRTMG_ERR_HIP, "hipStreamWaitEvent failed (shared inputs)"); ok_ = false; }
  share_->drop_unresolved();
  return ok_;
}

std::string default_blob_path(const char *which) {
  if (const char *env = getenv(strcmp(which, "sw") == 0 ? "RRTMG_HIP_SW_DATA" : "RRTMG_HIP_LW_DATA")) return env;
  Dl_info info;
  std::string dir = ".";
  if (dladdr((void *)&default_blob_path, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    size_t k = p.rfind('/');
    dir = (k == std::string::npos) ? "." : p.substr(0, k);
  }
  return dir + "/../data/rrtmg_" + which + "_data.bin";
}

}  // namespace rrtmg

using namespace rrtmg;

// The caller's struct is copied into one of the library's own.  struct_size must be sizeof(Args) of THIS header; anything else
// -- 0 included: that slot was `reserved0` in two earlier layouts, one that ended with the outputs and one that already carried
// the unit factors, and the library cannot tell which of them a zero comes from -- was built against another header and is
// refused, so that no caller ever gets RRTMG_OK with fields dropped or read past its struct.  Unit factors: host arrays only.
template <class Args, class Impl>
static int checked_call(rrtmg_ctx *ctx, const Args *a, const char *what, Impl impl) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!a) return ctx->fail(RRTMG_ERR_ARG, "%s: NULL argument struct", what);
  if ((size_t)a->struct_size != sizeof(Args))
    return ctx->fail(RRTMG_ERR_ARG, "%s: struct_size %d is not sizeof(%s_args) = %zu of this library (ABI version %d): set it to sizeof of the struct and rebuild the caller against include/rrtmg_hip.h",
                     what, (int)a->struct_size, what, sizeof(Args), RRTMG_HIP_ABI_VERSION);
  Args own = *a;
  if (own.memspace == 1 && (own.pressure_scale != 0.0 || own.water_path_scale != 0.0 || own.h2o_mul != 0.0 || own.h2o_div != 0.0))
    return ctx->fail(RRTMG_ERR_ARG, "%s: unit factors (pressure_scale, water_path_scale, h2o_mul, h2o_div) apply to host arrays only (memspace 0)", what);
  return impl(ctx, &own);
}

// The optional structs of the flux calls are checked before anything is enqueued: 0, or the status ctx->fail returned.
template <class S>
static int check_struct(rrtmg_ctx *ctx, const S *p, const char *name) {
  if (p && (size_t)p->struct_size != sizeof(S))
    return ctx->fail(RRTMG_ERR_ARG, "%s: struct_size %d is not sizeof(%s) = %zu of this library: set it to sizeof of the struct", name, (int)p->struct_size, name, sizeof(S));
  return 0;
}
template <class S>
static int check_band_struct(rrtmg_ctx *ctx, const S *b, const char *name) {
  if (int rc = check_struct(ctx, b, name)) return rc;
  if (b && b->levels != 0 && b->levels != 1) return ctx->fail(RRTMG_ERR_ARG, "%s: levels %d is neither 0 (all interface levels) nor 1 (surface and top)", name, (int)b->levels);
  return 0;
}

// Every shortwave flux entry point: sf, then b (size, then levels), then c; a struct without a member set is the call without it.
static int sw_optional_checked(rrtmg_ctx *ctx, const rrtmg_sw_surface *&sf, const rrtmg_sw_components *&c, const rrtmg_sw_band_fluxes *&b) {
  if (int rc = check_struct(ctx, sf, "rrtmg_sw_surface")) return rc;
  if (sf && !(sf->albdir || sf->albdif)) sf = nullptr;
  if (int rc = check_band_struct(ctx, b, "rrtmg_sw_band_fluxes")) return rc;
  if (b && !(b->up || b->dn || b->upc || b->dnc || b->dndir || b->dndirc)) b = nullptr;
  if (int rc = check_struct(ctx, c, "rrtmg_sw_components")) return rc;
  if (c && !(c->dirdflx || c->difdflx || c->dirdnuv || c->difdnuv || c->dirdnir || c->difdnir || c->dirdflxc || c->difdflxc)) c = nullptr;
  return 0;
}
// (f32: the float32 boundary, rrtmg_precision.h -- the same checks in the same order, then the driver behind the boundary)
static int sw_fluxes_checked(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_surface *sf, const rrtmg_sw_components *c, const rrtmg_sw_band_fluxes *b, bool f32 = false) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (int rc = sw_optional_checked(ctx, sf, c, b)) return rc;
  return checked_call(ctx, a, "rrtmg_sw", [sf, c, b, f32](rrtmg_ctx *x, const rrtmg_sw_args *y) { return f32 ? sw_fluxes_f32_impl(x, y, sf, c, b) : sw_fluxes_impl(x, y, sf, c, b); });
}
// the longwave's band struct, likewise
static int lw_optional_checked(rrtmg_ctx *ctx, const rrtmg_lw_band_fluxes *&b) {
  if (int rc = check_band_struct(ctx, b, "rrtmg_lw_band_fluxes")) return rc;
  if (b && !(b->up || b->dn || b->upc || b->dnc)) b = nullptr;
  return 0;
}

extern "C" {

#ifndef RRTMG_SRC_HASH
#define RRTMG_SRC_HASH "unknown"
#endif
// "... src:<hash>": sha256 over climt_amd/csrc + include/rrtmg_hip.h at build time (climt_amd/build.py::source_hash)
const char *rrtmg_hip_version(void) { return "rrtmg-hip 0.2 (gfx950) src:" RRTMG_SRC_HASH; }

int rrtmg_hip_create(rrtmg_ctx **out, int device_ordinal) {
  if (!out) return RRTMG_ERR_ARG;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  rrtmg_ctx *c = new rrtmg_ctx();
  c->device = device_ordinal;
  if (const char *env = getenv("RRTMG_HIP_CHUNK_TILES")) { const int v = atoi(env); if (v > 0) { c->chunk_tiles = v; c->chunk_auto = false; } }
  if (const char *env = getenv("RRTMG_HIP_SORT_COLUMNS")) c->sort_columns = atoi(env) != 0;
  if (const char *env = getenv("RRTMG_HIP_MAX_SCRATCH_BYTES")) { const long long v = atoll(env); if (v > 0) c->max_scratch_bytes = (size_t)v; }
  *out = c;
  if (e != hipSuccess || n <= 0)
    return c->fail(RRTMG_ERR_HIP, "no HIP device available (%s): librrtmg_hip has no CPU path", hipGetErrorString(e));
  if (device_ordinal < 0 || device_ordinal >= n) return c->fail(RRTMG_ERR_ARG, "device ordinal %d out of range (%d devices)", device_ordinal, n);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) c->device_mem = prop.totalGlobalMem;
  }
  return ctx_prepare_device(c);
}

void rrtmg_hip_destroy(rrtmg_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (auto &kv : ctx->bufs)
    if (kv.second.p) (void)hipFree(kv.second.p);
  if (ctx->sw_tab_dev) (void)hipFree(ctx->sw_tab_dev);
  if (ctx->lw_tab_dev) (void)hipFree(ctx->lw_tab_dev);
  if (ctx->err_dev) (void)hipFree(ctx->err_dev);
  if (ctx->ncloudy_dev) (void)hipFree(ctx->ncloudy_dev);
  if (ctx->hint) (void)hipHostFree((void *)ctx->hint);
  if (ctx->flag_host) (void)hipHostFree(ctx->flag_host);
  for (int w = 0; w < 2; ++w)
    if (ctx->pinned[w]) (void)hipHostFree(ctx->pinned[w]);
  for (int w = 0; w < 4; ++w)
    for (hipEvent_t e : ctx->ev[w])
      if (e) (void)hipEventDestroy(e);
  for (int w = 0; w < 2; ++w)
    for (int k = 0; k < 2; ++k)
      if (ctx->kiss_ev[w][k]) (void)hipEventDestroy(ctx->kiss_ev[w][k]);
  for (int w = 0; w < 2; ++w)
    if (ctx->sync_ev[w]) (void)hipEventDestroy(ctx->sync_ev[w]);
  for (int w = 0; w < 2; ++w)
    if (ctx->share_ev[w]) (void)hipEventDestroy(ctx->share_ev[w]);
  for (int w = 0; w < 2; ++w)
    if (ctx->alpha_ev[w]) (void)hipEventDestroy(ctx->alpha_ev[w]);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->stream_lw) (void)hipStreamDestroy(ctx->stream_lw);
  rrtmg::free_sw_desc(ctx);
  rrtmg::free_lw_desc(ctx);
  rrtmg::free_cork_tables(ctx);
  delete ctx;
}

const char *rrtmg_hip_last_error(const rrtmg_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }
void *rrtmg_hip_stream(rrtmg_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
int rrtmg_hip_kernel_ms(rrtmg_ctx *ctx, int which, double *ms) {
  if (!ctx || which < 0 || which > 3 || !ms || ctx->ev_chunks[which] <= 0) return RRTMG_ERR_ARG;
  double sum = 0.0;
  for (int c = 0; c < ctx->ev_chunks[which]; ++c) {
    float f = 0.f;
    RRTMG_HIP_CHECK(ctx, hipEventElapsedTime(&f, ctx->ev[which][2 * c], ctx->ev[which][2 * c + 1]));
    sum += (double)f;
  }
  *ms = sum;
  return RRTMG_OK;
}
int rrtmg_hip_kernel_launches(rrtmg_ctx *ctx, int which) { return (!ctx || which < 0 || which > 3) ? -1 : ctx->ev_chunks[which]; }
int rrtmg_hip_synchronize(rrtmg_ctx *ctx) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (ctx->stream) RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->stream_lw) RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream_lw));
  // deferred calls: collect the device-side error flags now (the former Fortran `stop` conditions).  Deferred calls do
  // not clear their flag (atomicMax accumulates over every call enqueued since the last collection); it is cleared here.
  if (ctx->pending[0] || ctx->pending[1]) {
    int herr[2] = {0, 0};
    const int zero[2] = {0, 0};
    RRTMG_HIP_CHECK(ctx, hipMemcpy(herr, ctx->err_dev, sizeof herr, hipMemcpyDeviceToHost));
    RRTMG_HIP_CHECK(ctx, hipMemcpy(ctx->err_dev, zero, sizeof zero, hipMemcpyHostToDevice));
    const bool p0 = ctx->pending[0], p1 = ctx->pending[1];
    ctx->pending[0] = ctx->pending[1] = false;
    const int e0 = p0 ? herr[0] : 0, e1 = p1 ? herr[1] : 0;
    if (e0 && e1) return ctx->fail(e0, "shortwave: %s; longwave (status %d): %s", status_message(e0), e1, status_message(e1));
    if (e0) return ctx->fail(e0, "shortwave: %s", status_message(e0));
    if (e1) return ctx->fail(e1, "longwave: %s", status_message(e1));
  }
  return RRTMG_OK;
}
int rrtmg_hip_stream_wait(rrtmg_ctx *ctx, void *other_stream) {
  if (!ctx || !ctx->stream || !ctx->stream_lw) return RRTMG_ERR_ARG;
  hipStream_t o = (hipStream_t)other_stream;
  RRTMG_HIP_CHECK(ctx, hipEventRecord(ctx->sync_ev[0], ctx->stream));
  RRTMG_HIP_CHECK(ctx, hipEventRecord(ctx->sync_ev[1], ctx->stream_lw));
  RRTMG_HIP_CHECK(ctx, hipStreamWaitEvent(o, ctx->sync_ev[0], 0));
  RRTMG_HIP_CHECK(ctx, hipStreamWaitEvent(o, ctx->sync_ev[1], 0));
  return RRTMG_OK;
}
int rrtmg_hip_set_deferred(rrtmg_ctx *ctx, int on) {
  if (!ctx) return RRTMG_ERR_ARG;
  int rc = rrtmg_hip_synchronize(ctx);
  ctx->deferred = on != 0;
  return rc;
}

int rrtmg_hip_set_column_sort(rrtmg_ctx *ctx, int on) {
  if (!ctx) return RRTMG_ERR_ARG;
  ctx->sort_columns = on != 0;
  return RRTMG_OK;
}

int rrtmg_hip_set_sw_night_skip(rrtmg_ctx *ctx, int on) {
  if (!ctx) return RRTMG_ERR_ARG;
  ctx->sw_night_skip = on != 0;
  return RRTMG_OK;
}
int rrtmg_hip_set_sw_night_pack(rrtmg_ctx *ctx, int on) {
  if (!ctx) return RRTMG_ERR_ARG;
  ctx->sw_night_pack = on != 0;
  return RRTMG_OK;
}
int rrtmg_hip_set_sw_clear_sky(rrtmg_ctx *ctx, int on) {
  if (!ctx) return RRTMG_ERR_ARG;
  ctx->sw_clear_sky = on != 0;
  return RRTMG_OK;
}
int rrtmg_hip_set_lw_clear_sky(rrtmg_ctx *ctx, int on) {
  if (!ctx) return RRTMG_ERR_ARG;
  ctx->lw_clear_sky = on != 0;
  return RRTMG_OK;
}
// The rank correlations of exponential overlap, copied into the context (rrtmg_ctx::alpha).  Host memory: the copy is complete
// on return.  Every mask step that reads the buffer first has its stream wait for alpha_ev (mcica_mask_launch, mcica_mask_impl).  Device memory: the copy goes on the stream the spectrum's device-resident calls run on -- the longwave's own
// stream first waits for what the main stream holds, where rrtmg_hip_overlap_alpha runs -- in front of every later call.
int rrtmg_hip_set_mcica_overlap_alpha(rrtmg_ctx *ctx, int which, int ncol, int nlay, int memspace, const double *alpha) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (which < 0 || which > 2) return ctx->fail(RRTMG_ERR_ARG, "set_mcica_overlap_alpha: which must be 0 (shortwave), 1 (longwave) or 2 (both)");
  if (!alpha) {
    for (int w = 0; w < 2; ++w)
      if (which == 2 || which == w) ctx->alpha[w] = rrtmg_ctx::OverlapAlpha();
    return RRTMG_OK;
  }
  if (ncol <= 0 || nlay <= 0 || nlay > 256 || (memspace != 0 && memspace != 1)) return ctx->fail(RRTMG_ERR_ARG, "set_mcica_overlap_alpha: bad argument");
  if (int rc = ctx_prepare_device(ctx)) return rc;
  const size_t bytes = (size_t)ncol * nlay * sizeof(double);
  for (int w = 0; w < 2; ++w) {
    if (which != 2 && which != w) continue;
    ctx->alpha[w] = rrtmg_ctx::OverlapAlpha();
    double *dev = (double *)ctx->buf(w == 0 ? "sw.alpha" : "lw.alpha", bytes);
    if (!dev) return ctx->status;
    if (memspace == 0) {
      // (calls still in flight from deferred mode may read the buffer: they are waited for, as a synchronous call does)
      if (ctx->pending[0] || ctx->pending[1]) { if (const int prc = rrtmg_hip_synchronize(ctx)) return prc; }
      RRTMG_HIP_CHECK(ctx, hipEventSynchronize(ctx->alpha_ev[w]));   // (an earlier copy from device memory into the same buffer may still be in flight)
      RRTMG_HIP_CHECK(ctx, hipMemcpy(dev, alpha, bytes, hipMemcpyHostToDevice));
    } else {
      hipStream_t s = (w == 1 && ctx->deferred) ? ctx->stream_lw : ctx->stream;
      if (s != ctx->stream) {
        RRTMG_HIP_CHECK(ctx, hipEventRecord(ctx->alpha_ev[w], ctx->stream));
        RRTMG_HIP_CHECK(ctx, hipStreamWaitEvent(s, ctx->alpha_ev[w], 0));
      }
      RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(dev, alpha, bytes, hipMemcpyDeviceToDevice, s));
      RRTMG_HIP_CHECK(ctx, hipEventRecord(ctx->alpha_ev[w], s));
      if (!ctx->deferred) RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
    }
    ctx->alpha[w].dev = dev; ctx->alpha[w].ncol = ncol; ctx->alpha[w].nlay = nlay;
  }
  return RRTMG_OK;
}
int rrtmg_hip_sw_night_last(rrtmg_ctx *ctx, int *night_tiles, int *night_columns) {
  if (!ctx || !night_tiles || !night_columns) return RRTMG_ERR_ARG;
  const volatile int *n = ctx->sw_night_reported ? ctx->night_host() : nullptr;
  *night_tiles = n ? n[0] : 0;
  *night_columns = n ? n[1] : 0;
  return RRTMG_OK;
}

int rrtmg_hip_set_constants(rrtmg_ctx *ctx, double pi, double grav, double planck, double boltz, double clight,
                            double avogad, double alosmt, double gascon, double sbcnst, double secdy) {
  if (!ctx) return RRTMG_ERR_ARG;
  Constants &k = ctx->k;
  k.pi = pi; k.grav = grav; k.planck = planck; k.boltz = boltz; k.clight = clight; k.avogad = avogad;
  k.alosmt = alosmt; k.gascon = gascon; k.sbcnst = sbcnst; k.secdy = secdy;
  k.radcn1 = 2. * planck * clight * clight * 1.e-07;
  k.radcn2 = planck * clight / boltz;
  ctx->have_constants = true;
  return RRTMG_OK;
}

int rrtmg_hip_sw_init(rrtmg_ctx *ctx, double cpdair, const char *blob_path) { return ctx ? sw_init_impl(ctx, cpdair, blob_path) : RRTMG_ERR_ARG; }
int rrtmg_hip_lw_init(rrtmg_ctx *ctx, double cpdair, const char *blob_path) { return ctx ? lw_init_impl(ctx, cpdair, blob_path) : RRTMG_ERR_ARG; }
int rrtmg_hip_lw_tables_synthetic(const rrtmg_ctx *ctx) { return ctx && ctx->lw_ts.synthetic ? 1 : 0; }

long rrtmg_hip_get_table(rrtmg_ctx *ctx, const char *name, double *out, long capacity) {
  if (!ctx || !name) return -1;
  const TableSet &ts = (strncmp(name, "sw/", 3) == 0) ? ctx->sw_ts : ctx->lw_ts;
  auto it = ts.reg.find(name);
  if (it == ts.reg.end()) return -1;
  const long n = it->second.n;
  if (out) {
    if (capacity < n) return -2;
    memcpy(out, ts.flat.data() + it->second.off, (size_t)n * sizeof(double));
  }
  return n;
}

int rrtmg_hip_sw_fluxes(rrtmg_ctx *ctx, const rrtmg_sw_args *a) { return sw_fluxes_checked(ctx, a, nullptr, nullptr, nullptr); }
int rrtmg_hip_lw_fluxes(rrtmg_ctx *ctx, const rrtmg_lw_args *a) { return checked_call(ctx, a, "rrtmg_lw", [](rrtmg_ctx *x, const rrtmg_lw_args *y) { return lw_fluxes_impl(x, y); }); }
int rrtmg_hip_sw_fluxes_components(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_components *c) { return sw_fluxes_checked(ctx, a, nullptr, c, nullptr); }
int rrtmg_hip_sw_fluxes_bands(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_components *c, const rrtmg_sw_band_fluxes *b) { return sw_fluxes_checked(ctx, a, nullptr, c, b); }
int rrtmg_hip_sw_fluxes_surface(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_surface *sf, const rrtmg_sw_components *c, const rrtmg_sw_band_fluxes *b) { return sw_fluxes_checked(ctx, a, sf, c, b); }
int rrtmg_hip_lw_fluxes_bands(rrtmg_ctx *ctx, const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *b) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (int rc = lw_optional_checked(ctx, b)) return rc;
  if (!b) return rrtmg_hip_lw_fluxes(ctx, a);
  return checked_call(ctx, a, "rrtmg_lw", [b](rrtmg_ctx *x, const rrtmg_lw_args *y) { return lw_fluxes_impl(x, y, b); });
}
// Both spectra of one host state (radiation_fluxes_impl; rrtmg_call.h: joint_run).  Every check of the separate entry points, through the same helpers,
// and the three of the joint call, before anything is enqueued.
static int radiation_fluxes_checked(rrtmg_ctx *ctx, const rrtmg_radiation_call *call, bool f32) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!call) return ctx->fail(RRTMG_ERR_ARG, "rrtmg_radiation_call: NULL argument struct");
  if (int rc = check_struct(ctx, call, "rrtmg_radiation_call")) return rc;
  const rrtmg_sw_surface *sf = call->sw_surface; const rrtmg_sw_components *c = call->sw_components; const rrtmg_sw_band_fluxes *b = call->sw_bands;
  const rrtmg_lw_band_fluxes *lb = call->lw_bands;
  if (int rc = sw_optional_checked(ctx, sf, c, b)) return rc;
  if (int rc = lw_optional_checked(ctx, lb)) return rc;
  return checked_call(ctx, call->sw, "rrtmg_sw", [=](rrtmg_ctx *, const rrtmg_sw_args *sw) {
    return checked_call(ctx, call->lw, "rrtmg_lw", [=](rrtmg_ctx *, const rrtmg_lw_args *lw) {
      if (sw->memspace != 0 || lw->memspace != 0)
        return ctx->fail(RRTMG_ERR_ARG, "rrtmg_hip_radiation_fluxes: host arrays only (memspace 0 in both structs); device-resident callers have deferred mode");
      if (sw->ncol != lw->ncol || sw->nlay != lw->nlay)
        return ctx->fail(RRTMG_ERR_ARG, "rrtmg_hip_radiation_fluxes: the shortwave has %d x %d columns x layers, the longwave %d x %d", (int)sw->ncol, (int)sw->nlay, (int)lw->ncol, (int)lw->nlay);
      if (sw->shard_col0 != lw->shard_col0 || sw->shard_ncol != lw->shard_ncol)
        return ctx->fail(RRTMG_ERR_ARG, "rrtmg_hip_radiation_fluxes: shard_col0 / shard_ncol differ between the two structs");
      ctx->f32 = f32;   // (host pointers: both drivers upload and download 4-byte reals for the duration of the call)
      const int rc = radiation_fluxes_impl(ctx, sw, sf, c, b, lw, lb);
      ctx->f32 = false;
      return rc;
    });
  });
}
int rrtmg_hip_radiation_fluxes(rrtmg_ctx *ctx, const rrtmg_radiation_call *call) { return radiation_fluxes_checked(ctx, call, false); }
// The float32 boundary (rrtmg_precision.h): the entry point chooses the precision of ITS call
int rrtmg_hip_sw_fluxes_f32(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_surface *surface, const rrtmg_sw_components *c, const rrtmg_sw_band_fluxes *b) {
  return sw_fluxes_checked(ctx, a, surface, c, b, true);
}
int rrtmg_hip_lw_fluxes_f32(rrtmg_ctx *ctx, const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *b) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (int rc = lw_optional_checked(ctx, b)) return rc;
  return checked_call(ctx, a, "rrtmg_lw", [b](rrtmg_ctx *x, const rrtmg_lw_args *y) { return lw_fluxes_f32_impl(x, y, b); });
}
int rrtmg_hip_radiation_fluxes_f32(rrtmg_ctx *ctx, const rrtmg_radiation_call *call) { return radiation_fluxes_checked(ctx, call, true); }
int rrtmg_hip_radiation_last(rrtmg_ctx *ctx, int *arrays_shared, long long *bytes_uploaded, long long *bytes_shared) {
  if (!ctx || !arrays_shared || !bytes_uploaded || !bytes_shared || !ctx->joint_seen) return RRTMG_ERR_ARG;
  *arrays_shared = ctx->joint_arrays_shared; *bytes_uploaded = ctx->joint_bytes_uploaded; *bytes_shared = ctx->joint_bytes_shared;
  return RRTMG_OK;
}
// band limits, cm^-1: shortwave bands 16..29 (wavenum1 / wavenum2 of rrtmg_sw_init.f90, band 29 last), longwave bands 1..16
// (rrtmg_lw_init.f90:196-204; hi - lo == delwave)
int rrtmg_hip_band_limits(int spectrum, double *lo, double *hi) {
  static const double sw_lo[14] = {2600., 3250., 4000., 4650., 5150., 6150., 7700., 8050., 12850., 16000., 22650., 29000., 38000., 820.};
  static const double sw_hi[14] = {3250., 4000., 4650., 5150., 6150., 7700., 8050., 12850., 16000., 22650., 29000., 38000., 50000., 2600.};
  static const double lw_lo[16] = {10., 350., 500., 630., 700., 820., 980., 1080., 1180., 1390., 1480., 1800., 2080., 2250., 2380., 2600.};
  static const double lw_hi[16] = {350., 500., 630., 700., 820., 980., 1080., 1180., 1390., 1480., 1800., 2080., 2250., 2380., 2600., 3250.};
  if (spectrum != 0 && spectrum != 1) return -1;
  const int n = spectrum ? 16 : 14;
  for (int i = 0; i < n; ++i) {
    if (lo) lo[i] = spectrum ? lw_lo[i] : sw_lo[i];
    if (hi) hi[i] = spectrum ? lw_hi[i] : sw_hi[i];
  }
  return n;
}
int rrtmg_hip_abi_version(void) { return RRTMG_HIP_ABI_VERSION; }

int rrtmg_hip_mcica_mask(rrtmg_ctx *ctx, int which, int ncol, int nlay, int icld, int permuteseed, int irng,
                         const double *play, const double *cldfrac, double *cldfmcl) {
  return ctx ? mcica_mask_impl(ctx, which, ncol, nlay, icld, permuteseed, irng, play, cldfrac, cldfmcl) : RRTMG_ERR_ARG;
}

}  // extern "C"
