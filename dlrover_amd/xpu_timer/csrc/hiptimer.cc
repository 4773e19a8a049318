// libhiptimer.so — LD_PRELOAD interposition profiler for the MI355X stack.
//
// MI355X-native rebuild of the reference's xpu_timer hook library
// (ref: xpu_timer/xpu_timer/nvidia/hook.cc + common/manager.cc — CUDA/cuBLAS/
// NCCL interposition with cudaEvent timing, hang detection, Prometheus).
//
// Interposed symbols (the HIP/ROCm analogs of SURVEY.md §2.3's table):
//   hipLaunchKernel / hipExtModuleLaunchKernel / hipModuleLaunchKernel
//   hipblasLtMatmul (hipBLASLt GEMMs — torch linear layers)
//   ncclAllReduce/ncclAllGather/ncclReduceScatter/ncclBroadcast/
//   ncclSend/ncclRecv  (librccl exports the nccl* names)
//   hipMalloc / hipFree / hipMemcpyAsync / hipHostMalloc (traffic counters)
//
// Each async op gets a pooled hipEvent pair recorded on ITS stream; a poller
// thread retires completed pairs into per-category latency/byte counters and
// tracks hang state: outstanding work with no completion for
// HIPTIMER_HANG_SECS (default 60) sets hang=1. Metrics are exported as
// Prometheus text to HIPTIMER_METRICS_DIR/hiptimer_<rank>.prom every
// HIPTIMER_DUMP_INTERVAL seconds (default 5) — the agent-side collector
// ships them to the master's hang diagnostician.
//
// Overhead: two event records + one pool pop per op; poller does the rest
// off the hot path (reference targets <=0.5%: xpu_timer/README.md:20).

#include <dlfcn.h>
#include <execinfo.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <errno.h>
#include <signal.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <deque>
#include <map>
#include <set>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

// nccl typedefs (we only pass pointers through; avoid needing rccl headers)
typedef void* ncclComm_t;
typedef struct
{
  char internal[128];
} ncclUniqueId_dummy;
typedef int ncclResult_t;
typedef int ncclDataType_t;
typedef int ncclRedOp_t;

namespace hiptimer {

using real_fn_t = void*;

// Map an interposed symbol to the library that actually provides it. Needed
// because torch dlopen()s its backend libs WITHOUT RTLD_GLOBAL, so
// dlsym(RTLD_NEXT, ...) from this preloaded lib cannot see them — calling the
// nil result was a segfault. dlsym on an explicit dlopen handle bypasses the
// search-order problem (and cannot find OUR interposer, unlike RTLD_DEFAULT).
static const char* provider_of(const char* name) {
  if (strncmp(name, "nccl", 4) == 0) return "librccl.so";
  if (strncmp(name, "hipblasLt", 9) == 0) return "libhipblaslt.so";
  return "libamdhip64.so";
}

static void* real(const char* name) {
  static std::mutex m;
  static std::map<std::string, void*> cache;
  std::lock_guard<std::mutex> g(m);
  auto it = cache.find(name);
  if (it != cache.end()) return it->second;
  void* fn = dlsym(RTLD_NEXT, name);
  if (fn == nullptr) {
    static std::map<std::string, void*> handles;
    const char* lib = provider_of(name);
    void*& h = handles[lib];
    if (h == nullptr) h = dlopen(lib, RTLD_LAZY | RTLD_LOCAL);
    if (h != nullptr) fn = dlsym(h, name);
  }
  if (getenv("HIPTIMER_DEBUG")) {
    fprintf(stderr, "[hiptimer] resolve %s -> %p\n", name, fn);
    fflush(stderr);
  }
  cache[name] = fn;
  return fn;
}

void install_crash_trace(const std::string& dir, int rank);

enum Category : int {
  CAT_KERNEL = 0,
  CAT_GEMM = 1,
  CAT_COMM = 2,
  CAT_MEMCPY = 3,
  CAT_COUNT = 4
};

static const char* kCatNames[CAT_COUNT] = {"kernel", "gemm", "comm", "memcpy"};

struct PendingOp {
  hipEvent_t start;
  hipEvent_t stop;
  Category cat;
  double bytes;
  double enqueue_ts;
  const char* name;  // owned by the HIP runtime (kernel symbol) or static
  double busbytes;   // collective bus-bytes (bytes x op/world factor)
  double flops;      // GEMM flops for TFLOPS attribution
};

// one retired op in the bounded kernel-trace ring (timeline dump)
struct TraceEvent {
  const char* name;
  int cat;
  double ts;      // host enqueue time (s)
  double dur_ms;  // GPU duration
};

struct CatStats {
  std::atomic<long> count{0};
  std::atomic<double> total_ms{0.0};
  std::atomic<double> max_ms{0.0};
  std::atomic<double> bytes{0.0};
};

class Manager {
 public:
  static Manager& inst() {
    static Manager m;
    return m;
  }

  bool enabled() const { return enabled_; }

  void record_begin(hipStream_t stream, Category cat, double bytes,
                    hipEvent_t* start, hipEvent_t* stop) {
    *start = nullptr;
    *stop = nullptr;
    if (!enabled_) return;
    // exact counting is cheap and unconditional …
    launched_.fetch_add(1);
    stats_[cat].count.fetch_add(1);
    if (bytes != 0) atomic_add(stats_[cat].bytes, bytes);
    if (no_events_) return;
    // … but hipEvent pairs cost ~10 us per launch (record + pool lock), which
    // measured 15.7% of step time on small_1b. Sample the timing instead:
    // every sample_-th launch gets events; drain() re-weights by sample_.
    // Collectives are always timed — they are the hang-detection signal and
    // arrive at bucket frequency, not kernel frequency.
    if (cat != CAT_COMM && sample_ > 1 &&
        (sample_ctr_.fetch_add(1) % sample_) != 0)
      return;
    std::lock_guard<std::mutex> g(pool_mu_);
    if (pool_.size() < 2) {
      for (int i = 0; i < 16; ++i) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, 0) != hipSuccess) return;
        pool_.push_back(e);
      }
    }
    *start = pool_.back();
    pool_.pop_back();
    *stop = pool_.back();
    pool_.pop_back();
    (void)hipEventRecord(*start, stream);
  }

  void record_end(hipStream_t stream, Category cat, double bytes,
                  hipEvent_t start, hipEvent_t stop,
                  const char* name = nullptr, double busbytes = 0,
                  double flops = 0) {
    if (!enabled_ || start == nullptr) return;
    (void)hipEventRecord(stop, stream);
    std::lock_guard<std::mutex> g(q_mu_);
    pending_.push_back({start, stop, cat, bytes, now(), name, busbytes, flops});
  }

  // stable owned name strings (per-GEMM-shape labels outlive the call)
  const char* intern(const std::string& s) {
    std::lock_guard<std::mutex> g(intern_mu_);
    return interned_.insert(s).first->c_str();
  }

  void count_gemm_flops(double flops) { atomic_add(gemm_flops_, flops); }

  // ---- RCCL communicator introspection (ref behavior: the reference's
  // nccl_parser extracts comm world size/rank + per-comm traffic so the
  // diagnostician can name WHICH process group a hang or imbalance is in) --
  struct CommInfo {
    int nranks = 0;
    int rank = 0;
    long calls = 0;
    double bytes = 0;
    bool alive = true;
  };

  void register_comm(void* c, int nranks, int rank) {
    std::lock_guard<std::mutex> g(comm_mu_);
    CommInfo& ci = comms_[c];
    ci.nranks = nranks;
    ci.rank = rank;
    ci.alive = true;
  }

  void unregister_comm(void* c) {
    std::lock_guard<std::mutex> g(comm_mu_);
    auto it = comms_.find(c);
    if (it != comms_.end()) it->second.alive = false;  // keep stats visible
  }

  int comm_nranks(void* c) {
    std::lock_guard<std::mutex> g(comm_mu_);
    auto it = comms_.find(c);
    return it != comms_.end() ? it->second.nranks : 0;
  }

  void count_comm_call(void* c, double bytes) {
    std::lock_guard<std::mutex> g(comm_mu_);
    CommInfo& ci = comms_[c];
    ci.calls += 1;
    ci.bytes += bytes;
  }

  void count_alloc(long bytes) { alloc_bytes_ += bytes; }
  void count_free() { free_count_ += 1; }
  void count_host_alloc(long bytes) { host_alloc_bytes_ += bytes; }

  static double now() {
    return std::chrono::duration<double>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
  }

 private:
  Manager() {
    const char* dis = getenv("HIPTIMER_DISABLE");
    enabled_ = !(dis && dis[0] == '1');
    const char* noev = getenv("HIPTIMER_NO_EVENTS");
    no_events_ = noev && noev[0] == '1';
    const char* nopoll = getenv("HIPTIMER_NO_POLLER");
    no_poller_ = nopoll && nopoll[0] == '1';
    const char* dbg = getenv("HIPTIMER_DEBUG");
    debug_ = dbg && dbg[0] == '1';
    hang_secs_ = getenv("HIPTIMER_HANG_SECS")
                     ? atof(getenv("HIPTIMER_HANG_SECS"))
                     : 60.0;
    dump_interval_ = getenv("HIPTIMER_DUMP_INTERVAL")
                         ? atof(getenv("HIPTIMER_DUMP_INTERVAL"))
                         : 5.0;
    sample_ = getenv("HIPTIMER_SAMPLE") ? atoi(getenv("HIPTIMER_SAMPLE")) : 32;
    if (sample_ < 1) sample_ = 1;
    const char* dir = getenv("HIPTIMER_METRICS_DIR");
    metrics_dir_ = dir ? dir : "/tmp/hiptimer";
    const char* rank = getenv("RANK");
    rank_ = rank ? atoi(rank) : 0;
    if (mkdir(metrics_dir_.c_str(), 0755) != 0 && errno != EEXIST)
      enabled_ = false;
    last_completion_ = now();
    if (enabled_ && getenv("HIPTIMER_NO_CRASH_TRACE") == nullptr)
      install_crash_trace(metrics_dir_, rank_);
    if (enabled_ && !no_poller_)
      pthread_create(&poller_, nullptr, &Manager::poll_entry, this);
  }

  static void* poll_entry(void* self) {
    static_cast<Manager*>(self)->poll_loop();
    return nullptr;
  }

  void poll_loop() {
    double last_dump = 0;
    while (true) {
      usleep(20000);  // 20 ms
      drain();
      double t = now();
      if (t - last_dump > dump_interval_) {
        dump_metrics();
        last_dump = t;
      }
      maybe_dump_timeline();
    }
  }

  void drain() {
    std::deque<PendingOp> done;
    {
      std::lock_guard<std::mutex> g(q_mu_);
      // events complete in stream order per stream; scan the front
      while (!pending_.empty()) {
        PendingOp& op = pending_.front();
        if (hipEventQuery(op.stop) != hipSuccess) break;
        done.push_back(op);
        pending_.pop_front();
      }
    }
    for (auto& op : done) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, op.start, op.stop) == hipSuccess) {
        // timing is sampled 1-in-sample_ for non-comm ops: re-weight so the
        // exported ms totals estimate wall contribution (counts and bytes
        // are exact — accumulated at launch time in record_begin)
        long w = (op.cat == CAT_COMM) ? 1 : sample_;
        auto& s = stats_[op.cat];
        atomic_add(s.total_ms, (double)ms * w);
        atomic_max(s.max_ms, (double)ms);
        if (op.name != nullptr) {
          // per-kernel attribution (poller thread only: no lock needed)
          auto& e = kernel_stats_[op.name];
          e.first += w;
          e.second += (double)ms * w;
        }
        if (op.cat == CAT_COMM && op.busbytes > 0) {
          atomic_add(comm_busbytes_, op.busbytes);
          comm_busms_ += (double)ms;
        }
        if (op.cat == CAT_GEMM) {
          gemm_ms_timed_ += (double)ms * w;
        }
        // bounded kernel-trace ring (timeline dump, ref manager.h:50-62)
        trace_ring_[trace_head_ % kTraceRing] = {
            op.name ? op.name : kCatNames[op.cat], op.cat, op.enqueue_ts,
            (double)ms};
        trace_head_ += 1;
      }
      last_completion_ = now();
      {
        std::lock_guard<std::mutex> g(pool_mu_);
        pool_.push_back(op.start);
        pool_.push_back(op.stop);
      }
    }
  }

  static void atomic_add(std::atomic<double>& a, double v) {
    double cur = a.load();
    while (!a.compare_exchange_weak(cur, cur + v)) {
    }
  }
  static void atomic_max(std::atomic<double>& a, double v) {
    double cur = a.load();
    while (cur < v && !a.compare_exchange_weak(cur, v)) {
    }
  }

  bool is_hang(double* since) {
    size_t outstanding;
    {
      std::lock_guard<std::mutex> g(q_mu_);
      outstanding = pending_.size();
      if (!pending_.empty()) {
        const PendingOp& f = pending_.front();
        oldest_name_ = f.name ? f.name : kCatNames[f.cat];
        oldest_cat_ = f.cat;
        oldest_enqueue_ = f.enqueue_ts;
      } else {
        oldest_name_ = nullptr;
      }
      outstanding_ = outstanding;
    }
    double idle = now() - last_completion_;
    if (outstanding > 0 && idle > hang_secs_) {
      *since = last_completion_.load();
      return true;
    }
    *since = 0;
    return false;
  }

  void dump_metrics() {
    char path[512], tmp[520];
    snprintf(path, sizeof(path), "%s/hiptimer_%d.prom", metrics_dir_.c_str(),
             rank_);
    snprintf(tmp, sizeof(tmp), "%s.tmp", path);
    FILE* f = fopen(tmp, "w");
    if (!f) return;
    double since = 0;
    int hang = is_hang(&since) ? 1 : 0;
    // metric names mirror the reference xpu_timer exposition so the
    // collector/diagnostician logic carries over (XPU_TIMER_COMMON_HANG)
    fprintf(f, "XPU_TIMER_COMMON_HANG %d\n", hang);
    fprintf(f, "hiptimer_hang_since_seconds %.3f\n", since);
    fprintf(f, "hiptimer_outstanding_ops %zu\n", outstanding_);
    if (oldest_name_ != nullptr) {
      // the op the device has been sitting on: a stuck ncclAllReduce names
      // the wedged collective directly (ref hang dossier quality bar)
      std::string nm = std::string(oldest_name_).substr(0, 120);
      for (auto& c : nm)
        if (c == '"' || c == '\\' || c == '\n') c = '_';
      fprintf(f,
              "hiptimer_oldest_pending{name=\"%s\",cat=\"%s\"} %.3f\n",
              nm.c_str(), kCatNames[oldest_cat_], now() - oldest_enqueue_);
    }
    fprintf(f, "hiptimer_wall_seconds %.3f\n", now());
    fprintf(f, "hiptimer_launched_total %ld\n", launched_.load());
    fprintf(f, "hiptimer_sample_interval %d\n", sample_);
    for (int c = 0; c < CAT_COUNT; ++c) {
      auto& s = stats_[c];
      fprintf(f, "hiptimer_op_count{cat=\"%s\"} %ld\n", kCatNames[c],
              s.count.load());
      fprintf(f, "hiptimer_op_ms_total{cat=\"%s\"} %.3f\n", kCatNames[c],
              s.total_ms.load());
      fprintf(f, "hiptimer_op_ms_max{cat=\"%s\"} %.3f\n", kCatNames[c],
              s.max_ms.load());
      fprintf(f, "hiptimer_op_bytes_total{cat=\"%s\"} %.0f\n", kCatNames[c],
              s.bytes.load());
    }
    // top kernels by total time (reference exposes per-kernel latency too)
    {
      std::vector<std::pair<std::string, std::pair<long, double>>> top(
          kernel_stats_.begin(), kernel_stats_.end());
      std::sort(top.begin(), top.end(), [](const auto& a, const auto& b) {
        return a.second.second > b.second.second;
      });
      int n = 0;
      for (auto& kv : top) {
        if (++n > 20) break;
        std::string nm = kv.first.substr(0, 120);
        for (auto& c : nm)
          if (c == '"' || c == '\\' || c == '\n') c = '_';
        fprintf(f, "hiptimer_kernel_count{name=\"%s\"} %ld\n", nm.c_str(),
                kv.second.first);
        fprintf(f, "hiptimer_kernel_ms_total{name=\"%s\"} %.3f\n",
                nm.c_str(), kv.second.second);
      }
    }
    {
      std::lock_guard<std::mutex> g(comm_mu_);
      for (auto& kv : comms_) {
        fprintf(f,
                "hiptimer_comm_calls{comm=\"%p\",nranks=\"%d\",rank=\"%d\","
                "alive=\"%d\"} %ld\n",
                kv.first, kv.second.nranks, kv.second.rank,
                kv.second.alive ? 1 : 0, kv.second.calls);
        fprintf(f,
                "hiptimer_comm_elems{comm=\"%p\",nranks=\"%d\",rank=\"%d\","
                "alive=\"%d\"} %.0f\n",
                kv.first, kv.second.nranks, kv.second.rank,
                kv.second.alive ? 1 : 0, kv.second.bytes);
      }
    }
    // derived throughput metrics
    {
      double bus = comm_busbytes_.load();
      double bms = comm_busms_;
      fprintf(f, "hiptimer_comm_busbytes_total %.0f\n", bus);
      fprintf(f, "hiptimer_comm_busbw_gbs %.3f\n",
              bms > 0 ? bus / (bms / 1e3) / 1e9 : 0.0);
      double gf = gemm_flops_.load();
      double gms = gemm_ms_timed_;
      fprintf(f, "hiptimer_gemm_flops_total %.0f\n", gf);
      fprintf(f, "hiptimer_gemm_tflops %.2f\n",
              gms > 0 ? gf / (gms / 1e3) / 1e12 : 0.0);
    }
    fprintf(f, "hiptimer_device_alloc_bytes %.0f\n", (double)alloc_bytes_.load());
    fprintf(f, "hiptimer_device_free_total %ld\n", free_count_.load());
    fprintf(f, "hiptimer_host_alloc_bytes %.0f\n",
            (double)host_alloc_bytes_.load());
    fclose(f);
    rename(tmp, path);
  }

  // timeline: dump the trace ring as chrome-trace JSON (perfetto-loadable)
  // when <metrics_dir>/dump_timeline_<rank> appears, or automatically on the
  // first hang detection (ref: KernelTraceManager ring + gen_trace_timeline)
  void maybe_dump_timeline() {
    char flag[512], all_flag[512];
    snprintf(flag, sizeof(flag), "%s/dump_timeline_%d", metrics_dir_.c_str(),
             rank_);
    snprintf(all_flag, sizeof(all_flag), "%s/dump_timeline_all",
             metrics_dir_.c_str());
    double since;
    bool hang_now = is_hang(&since);
    bool flagged = access(flag, F_OK) == 0;
    // shared fan-out flag (every local rank dumps once per touch): edge-
    // triggered on mtime so no rank has to unlink it out from under peers
    bool all_flagged = false;
    struct stat st;
    if (stat(all_flag, &st) == 0 && st.st_mtime != last_all_flag_mtime_) {
      last_all_flag_mtime_ = st.st_mtime;
      all_flagged = true;
    }
    if (!flagged && !all_flagged && !(hang_now && !hang_dumped_)) return;
    if (hang_now) hang_dumped_ = true;
    if (flagged) unlink(flag);
    dump_timeline();
  }

  void dump_timeline() {
    char path[512];
    snprintf(path, sizeof(path), "%s/timeline_%d.json", metrics_dir_.c_str(),
             rank_);
    FILE* f = fopen(path, "w");
    if (!f) return;
    fprintf(f, "{\"traceEvents\":[\n");
    long n = trace_head_ < (long)kTraceRing ? trace_head_ : (long)kTraceRing;
    long first = trace_head_ - n;
    for (long i = 0; i < n; ++i) {
      const TraceEvent& e = trace_ring_[(first + i) % kTraceRing];
      std::string nm = e.name ? std::string(e.name).substr(0, 160) : "?";
      for (auto& c : nm)
        if (c == '"' || c == '\\' || c == '\n') c = '_';
      fprintf(f,
              "%s{\"name\":\"%s\",\"cat\":\"%s\",\"ph\":\"X\","
              "\"ts\":%.1f,\"dur\":%.1f,\"pid\":%d,\"tid\":%d}",
              i ? ",\n" : "", nm.c_str(), kCatNames[e.cat], e.ts * 1e6,
              e.dur_ms * 1e3, rank_, e.cat);
    }
    fprintf(f, "\n]}\n");
    fclose(f);
  }

 public:
 private:
  bool enabled_ = false;
  bool no_events_ = false;
  bool no_poller_ = false;
  bool debug_ = false;
  double hang_secs_ = 60.0;
  double dump_interval_ = 5.0;
  std::string metrics_dir_;
  int rank_ = 0;
  pthread_t poller_;
  std::mutex pool_mu_;
  std::vector<hipEvent_t> pool_;
  std::mutex q_mu_;
  std::deque<PendingOp> pending_;
  std::mutex comm_mu_;
  std::map<void*, CommInfo> comms_;
  CatStats stats_[CAT_COUNT];
  std::map<std::string, std::pair<long, double>> kernel_stats_;
  std::atomic<long> launched_{0};
  int sample_ = 32;
  std::atomic<long> sample_ctr_{0};
  std::atomic<long> alloc_bytes_{0};
  std::atomic<long> free_count_{0};
  std::atomic<long> host_alloc_bytes_{0};
  std::atomic<double> last_completion_{0};
  std::mutex intern_mu_;
  std::set<std::string> interned_;
  std::atomic<double> gemm_flops_{0};
  double gemm_ms_timed_ = 0;        // poller thread only
  std::atomic<double> comm_busbytes_{0};
  double comm_busms_ = 0;           // poller thread only
  static constexpr size_t kTraceRing = 8192;
  TraceEvent trace_ring_[kTraceRing] = {};
  long trace_head_ = 0;             // poller thread only
  bool hang_dumped_ = false;
  long last_all_flag_mtime_ = 0;
  size_t outstanding_ = 0;        // poller thread only
  const char* oldest_name_ = nullptr;
  int oldest_cat_ = 0;
  double oldest_enqueue_ = 0;
};

// ---- fatal-signal backtrace (ref: common/signal_handler.cc) --------------
// On SIGSEGV/SIGABRT/SIGBUS/SIGFPE: write a native backtrace of the faulting
// thread to <metrics_dir>/crash_<rank>.txt (async-signal-safe: backtrace_*_fd
// + write), then re-raise with the default handler so the exit code and core
// behavior are unchanged. Round-1's driver bench died with an unattributed
// GPU memory fault — this leaves a host-side trace next time.
class SignalBacktrace {
 public:
  static void install(const std::string& dir, int rank) {
    static SignalBacktrace inst;
    inst.path_ = dir + "/crash_" + std::to_string(rank) + ".txt";
    int sigs[] = {SIGSEGV, SIGABRT, SIGBUS, SIGFPE};
    for (int s : sigs) {
      struct sigaction sa;
      memset(&sa, 0, sizeof(sa));
      sa.sa_sigaction = &SignalBacktrace::on_signal;
      sa.sa_flags = SA_SIGINFO | SA_RESETHAND;
      sigaction(s, &sa, &inst.prev_[s]);
    }
    self() = &inst;
  }

 private:
  static SignalBacktrace*& self() {
    static SignalBacktrace* p = nullptr;
    return p;
  }

  static void on_signal(int sig, siginfo_t* info, void*) {
    SignalBacktrace* s = self();
    if (s != nullptr) {
      int fd = open(s->path_.c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0644);
      if (fd >= 0) {
        char head[128];
        int n = snprintf(head, sizeof(head),
                         "signal %d at addr %p; native backtrace:\n", sig,
                         info ? info->si_addr : nullptr);
        if (n > 0) {
          ssize_t w = write(fd, head, (size_t)n);
          (void)w;
        }
        void* frames[64];
        int depth = backtrace(frames, 64);
        backtrace_symbols_fd(frames, depth, fd);
        close(fd);
      }
    }
    raise(sig);  // SA_RESETHAND restored the default handler
  }

  std::string path_;
  struct sigaction prev_[64] = {};
};

void install_crash_trace(const std::string& dir, int rank) {
  SignalBacktrace::install(dir, rank);
}

struct Scoped {
  hipEvent_t start = nullptr, stop = nullptr;
  hipStream_t stream;
  Category cat;
  double bytes;
  const char* name = nullptr;
  double busbytes = 0;
  double flops = 0;
  Scoped(hipStream_t s, Category c, double b, const char* n = nullptr,
         double bus = 0, double fl = 0)
      : stream(s), cat(c), bytes(b), name(n), busbytes(bus), flops(fl) {
    Manager::inst().record_begin(s, c, b, &start, &stop);
  }
  void finish() {
    Manager::inst().record_end(stream, cat, bytes, start, stop, name,
                               busbytes, flops);
  }
};

}  // namespace hiptimer

using hiptimer::CAT_COMM;
using hiptimer::CAT_GEMM;
using hiptimer::CAT_KERNEL;
using hiptimer::CAT_MEMCPY;
using hiptimer::Manager;
using hiptimer::real;

extern "C" {

// ---- kernel launches -------------------------------------------------------

hipError_t hipLaunchKernel(const void* function_address, dim3 numBlocks,
                           dim3 dimBlocks, void** args, size_t sharedMemBytes,
                           hipStream_t stream) {
  using fn_t = hipError_t (*)(const void*, dim3, dim3, void**, size_t,
                              hipStream_t);
  static fn_t fn = (fn_t)real("hipLaunchKernel");
  using name_fn_t = const char* (*)(const void*, hipStream_t);
  static name_fn_t name_fn = (name_fn_t)real("hipKernelNameRefByPtr");
  const char* kname =
      name_fn != nullptr ? name_fn(function_address, stream) : nullptr;
  hiptimer::Scoped sc(stream, CAT_KERNEL, 0, kname);
  hipError_t rc =
      fn(function_address, numBlocks, dimBlocks, args, sharedMemBytes, stream);
  sc.finish();
  return rc;
}

hipError_t hipModuleLaunchKernel(hipFunction_t f, unsigned gx, unsigned gy,
                                 unsigned gz, unsigned bx, unsigned by,
                                 unsigned bz, unsigned sharedMemBytes,
                                 hipStream_t stream, void** params,
                                 void** extra) {
  using fn_t = hipError_t (*)(hipFunction_t, unsigned, unsigned, unsigned,
                              unsigned, unsigned, unsigned, unsigned,
                              hipStream_t, void**, void**);
  static fn_t fn = (fn_t)real("hipModuleLaunchKernel");
  hiptimer::Scoped sc(stream, CAT_KERNEL, 0);
  hipError_t rc =
      fn(f, gx, gy, gz, bx, by, bz, sharedMemBytes, stream, params, extra);
  sc.finish();
  return rc;
}

hipError_t hipExtModuleLaunchKernel(hipFunction_t f, unsigned gx, unsigned gy,
                                    unsigned gz, unsigned bx, unsigned by,
                                    unsigned bz, size_t sharedMemBytes,
                                    hipStream_t stream, void** params,
                                    void** extra, hipEvent_t startEvent,
                                    hipEvent_t stopEvent, unsigned flags) {
  using fn_t = hipError_t (*)(hipFunction_t, unsigned, unsigned, unsigned,
                              unsigned, unsigned, unsigned, size_t,
                              hipStream_t, void**, void**, hipEvent_t,
                              hipEvent_t, unsigned);
  static fn_t fn = (fn_t)real("hipExtModuleLaunchKernel");
  hiptimer::Scoped sc(stream, CAT_KERNEL, 0);
  hipError_t rc = fn(f, gx, gy, gz, bx, by, bz, sharedMemBytes, stream, params,
                     extra, startEvent, stopEvent, flags);
  sc.finish();
  return rc;
}

// ---- hipBLASLt GEMM --------------------------------------------------------

// hipblasLtMatmul(handle, desc, alpha, A, Adesc, B, Bdesc, beta, C, Cdesc,
//                 D, Ddesc, algo, workspace, wsSize, stream)
// layout attribute query (hipblaslt.h): BATCH_COUNT=0, ROWS=4, COLS=5
//
// Current hipBLASLt answers the ROWS/COLS queries with INVALID_VALUE (only
// the batch attributes are readable), so rows/cols are remembered when the
// layout is created and the query is only the fallback.
static std::mutex g_layout_mu;
static std::map<void*, std::pair<uint64_t, uint64_t>> g_layout_dims;

int hipblasLtMatrixLayoutCreate(void** layout, int type, uint64_t rows,
                                uint64_t cols, int64_t ld) {
  using fn_t = int (*)(void**, int, uint64_t, uint64_t, int64_t);
  static fn_t fn = (fn_t)real("hipblasLtMatrixLayoutCreate");
  int rc = fn(layout, type, rows, cols, ld);
  if (rc == 0 && layout != nullptr && *layout != nullptr) {
    std::lock_guard<std::mutex> g(g_layout_mu);
    g_layout_dims[*layout] = {rows, cols};
  }
  return rc;
}

int hipblasLtMatrixLayoutDestroy(void* layout) {
  using fn_t = int (*)(void*);
  static fn_t fn = (fn_t)real("hipblasLtMatrixLayoutDestroy");
  {
    std::lock_guard<std::mutex> g(g_layout_mu);
    g_layout_dims.erase(layout);
  }
  return fn(layout);
}

static void layout_dims(void* layout, long long* rows, long long* cols,
                        int* batch) {
  using get_t = int (*)(void*, int, void*, size_t, size_t*);
  static get_t get = (get_t)real("hipblasLtMatrixLayoutGetAttribute");
  *rows = *cols = 0;
  *batch = 1;
  if (get == nullptr || layout == nullptr) return;
  unsigned long long r = 0, c = 0;
  int32_t b = 1;
  size_t written = 0;
  bool known = false;
  {
    std::lock_guard<std::mutex> g(g_layout_mu);
    auto it = g_layout_dims.find(layout);
    if (it != g_layout_dims.end()) {
      r = it->second.first;
      c = it->second.second;
      known = true;
    }
  }
  if (!known) {
    get(layout, 4, &r, sizeof(r), &written);
    get(layout, 5, &c, sizeof(c), &written);
  }
  get(layout, 0, &b, sizeof(b), &written);
  *rows = (long long)r;
  *cols = (long long)c;
  *batch = b > 0 ? b : 1;
}

int hipblasLtMatmul(void* handle, void* matmulDesc, const void* alpha,
                    const void* A, void* Adesc, const void* B, void* Bdesc,
                    const void* beta, const void* C, void* Cdesc, void* D,
                    void* Ddesc, const void* algo, void* workspace,
                    size_t workspaceSizeInBytes, hipStream_t stream) {
  using fn_t = int (*)(void*, void*, const void*, const void*, void*,
                       const void*, void*, const void*, const void*, void*,
                       void*, void*, const void*, void*, size_t, hipStream_t);
  static fn_t fn = (fn_t)real("hipblasLtMatmul");
  // per-GEMM m/n/k/batch -> flops + a per-shape label (ref hook.cc:253-322)
  long long m = 0, n = 0, ar = 0, ac = 0;
  int batch = 1, abatch = 1;
  layout_dims(Ddesc, &m, &n, &batch);
  layout_dims(Adesc, &ar, &ac, &abatch);
  const long long kdim = (ar == m) ? ac : ar;
  const double flops = 2.0 * m * n * kdim * batch;
  const char* label = nullptr;
  if (m > 0 && n > 0 && kdim > 0) {
    char buf[96];
    snprintf(buf, sizeof(buf), "gemm_m%lld_n%lld_k%lld_b%d", m, n, kdim,
             batch);
    label = Manager::inst().intern(buf);
    Manager::inst().count_gemm_flops(flops);
  }
  hiptimer::Scoped sc(stream, CAT_GEMM, 0, label, 0, flops);
  int rc = fn(handle, matmulDesc, alpha, A, Adesc, B, Bdesc, beta, C, Cdesc, D,
              Ddesc, algo, workspace, workspaceSizeInBytes, stream);
  sc.finish();
  return rc;
}

// ---- RCCL collectives (librccl exports nccl* names) --------------------------

// ncclDataType_t element sizes (nccl.h ordering; RCCL matches upstream)
static int nccl_dtype_bytes(int dt) {
  switch (dt) {
    case 0: case 1: return 1;               // int8/uint8
    case 2: case 3: return 4;               // int32/uint32
    case 4: case 5: return 8;               // int64/uint64
    case 6: return 2;                       // float16
    case 7: return 4;                       // float32
    case 8: return 8;                       // float64
    case 9: return 2;                       // bfloat16
    default: return 1;                      // fp8 variants / unknown
  }
}

// bus-bytes per DLRover/nccl-tests busbw convention (node_check utils.py):
// allreduce 2(n-1)/n x data; all-gather/reduce-scatter (n-1)/n x total data
static double busbw_factor_allreduce(int n) {
  return n > 0 ? 2.0 * (n - 1) / n : 0.0;
}
static double busbw_factor_ag_rs(int n) {
  return n > 0 ? (double)(n - 1) / n : 0.0;
}

#define HIPTIMER_NCCL_COLL(NAME, BUS_FACTOR)                                   \
  ncclResult_t NAME(const void* sendbuff, void* recvbuff, size_t count,        \
                    ncclDataType_t dt, ncclRedOp_t op, ncclComm_t comm,        \
                    hipStream_t stream) {                                      \
    using fn_t = ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t,  \
                                  ncclRedOp_t, ncclComm_t, hipStream_t);       \
    static fn_t fn = (fn_t)real(#NAME);                                        \
    const double bytes = (double)count * nccl_dtype_bytes((int)dt);            \
    const int nr = Manager::inst().comm_nranks(comm);                          \
    Manager::inst().count_comm_call(comm, bytes);                              \
    hiptimer::Scoped sc(stream, CAT_COMM, bytes, #NAME,                        \
                        bytes * (BUS_FACTOR));                                 \
    ncclResult_t rc = fn(sendbuff, recvbuff, count, dt, op, comm, stream);     \
    sc.finish();                                                               \
    return rc;                                                                 \
  }

// comm lifecycle: record {comm -> (nranks, rank)} so metrics can attribute
// traffic to a specific process group (DP vs TP vs PP)
ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks,
                              ncclUniqueId_dummy commId, int rank) {
  using fn_t = ncclResult_t (*)(ncclComm_t*, int, ncclUniqueId_dummy, int);
  static fn_t fn = (fn_t)real("ncclCommInitRank");
  ncclResult_t rc = fn(comm, nranks, commId, rank);
  if (rc == 0 && comm != nullptr)
    Manager::inst().register_comm(*comm, nranks, rank);
  return rc;
}

ncclResult_t ncclCommInitRankConfig(ncclComm_t* comm, int nranks,
                                    ncclUniqueId_dummy commId, int rank,
                                    void* config) {
  using fn_t =
      ncclResult_t (*)(ncclComm_t*, int, ncclUniqueId_dummy, int, void*);
  static fn_t fn = (fn_t)real("ncclCommInitRankConfig");
  ncclResult_t rc = fn(comm, nranks, commId, rank, config);
  if (rc == 0 && comm != nullptr)
    Manager::inst().register_comm(*comm, nranks, rank);
  return rc;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  using fn_t = ncclResult_t (*)(ncclComm_t);
  static fn_t fn = (fn_t)real("ncclCommDestroy");
  Manager::inst().unregister_comm(comm);
  return fn(comm);
}

ncclResult_t ncclCommAbort(ncclComm_t comm) {
  using fn_t = ncclResult_t (*)(ncclComm_t);
  static fn_t fn = (fn_t)real("ncclCommAbort");
  Manager::inst().unregister_comm(comm);
  return fn(comm);
}

HIPTIMER_NCCL_COLL(ncclAllReduce, busbw_factor_allreduce(nr))
HIPTIMER_NCCL_COLL(ncclReduce, 1.0)

ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff,
                           size_t sendcount, ncclDataType_t dt, ncclComm_t comm,
                           hipStream_t stream) {
  using fn_t = ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t,
                                ncclComm_t, hipStream_t);
  static fn_t fn = (fn_t)real("ncclAllGather");
  const int nr = Manager::inst().comm_nranks(comm);
  const double bytes = (double)sendcount * nccl_dtype_bytes((int)dt) * (nr > 0 ? nr : 1);
  Manager::inst().count_comm_call(comm, bytes);
  hiptimer::Scoped sc(stream, CAT_COMM, bytes, "ncclAllGather",
                      bytes * busbw_factor_ag_rs(nr));
  ncclResult_t rc = fn(sendbuff, recvbuff, sendcount, dt, comm, stream);
  sc.finish();
  return rc;
}

ncclResult_t ncclReduceScatter(const void* sendbuff, void* recvbuff,
                               size_t recvcount, ncclDataType_t dt,
                               ncclRedOp_t op, ncclComm_t comm,
                               hipStream_t stream) {
  using fn_t = ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t,
                                ncclRedOp_t, ncclComm_t, hipStream_t);
  static fn_t fn = (fn_t)real("ncclReduceScatter");
  const int nr = Manager::inst().comm_nranks(comm);
  const double bytes = (double)recvcount * nccl_dtype_bytes((int)dt) * (nr > 0 ? nr : 1);
  Manager::inst().count_comm_call(comm, bytes);
  hiptimer::Scoped sc(stream, CAT_COMM, bytes, "ncclReduceScatter",
                      bytes * busbw_factor_ag_rs(nr));
  ncclResult_t rc = fn(sendbuff, recvbuff, recvcount, dt, op, comm, stream);
  sc.finish();
  return rc;
}

ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count,
                           ncclDataType_t dt, int root, ncclComm_t comm,
                           hipStream_t stream) {
  using fn_t = ncclResult_t (*)(const void*, void*, size_t, ncclDataType_t,
                                int, ncclComm_t, hipStream_t);
  static fn_t fn = (fn_t)real("ncclBroadcast");
  const double bytes = (double)count * nccl_dtype_bytes((int)dt);
  Manager::inst().count_comm_call(comm, bytes);
  hiptimer::Scoped sc(stream, CAT_COMM, bytes, "ncclBroadcast", bytes);
  ncclResult_t rc = fn(sendbuff, recvbuff, count, dt, root, comm, stream);
  sc.finish();
  return rc;
}

ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t dt,
                      int peer, ncclComm_t comm, hipStream_t stream) {
  using fn_t =
      ncclResult_t (*)(const void*, size_t, ncclDataType_t, int, ncclComm_t,
                       hipStream_t);
  static fn_t fn = (fn_t)real("ncclSend");
  const double bytes = (double)count * nccl_dtype_bytes((int)dt);
  Manager::inst().count_comm_call(comm, bytes);
  hiptimer::Scoped sc(stream, CAT_COMM, bytes, "ncclSend", bytes);
  ncclResult_t rc = fn(sendbuff, count, dt, peer, comm, stream);
  sc.finish();
  return rc;
}

ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t dt, int peer,
                      ncclComm_t comm, hipStream_t stream) {
  using fn_t = ncclResult_t (*)(void*, size_t, ncclDataType_t, int, ncclComm_t,
                                hipStream_t);
  static fn_t fn = (fn_t)real("ncclRecv");
  const double bytes = (double)count * nccl_dtype_bytes((int)dt);
  Manager::inst().count_comm_call(comm, bytes);
  hiptimer::Scoped sc(stream, CAT_COMM, bytes, "ncclRecv", bytes);
  ncclResult_t rc = fn(recvbuff, count, dt, peer, comm, stream);
  sc.finish();
  return rc;
}

// ---- memory traffic ----------------------------------------------------------

hipError_t hipMalloc(void** ptr, size_t size) {
  using fn_t = hipError_t (*)(void**, size_t);
  static fn_t fn = (fn_t)real("hipMalloc");
  hipError_t rc = fn(ptr, size);
  if (rc == hipSuccess) Manager::inst().count_alloc((long)size);
  return rc;
}

hipError_t hipFree(void* ptr) {
  using fn_t = hipError_t (*)(void*);
  static fn_t fn = (fn_t)real("hipFree");
  Manager::inst().count_free();
  return fn(ptr);
}

hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int flags) {
  using fn_t = hipError_t (*)(void**, size_t, unsigned int);
  static fn_t fn = (fn_t)real("hipHostMalloc");
  hipError_t rc = fn(ptr, size, flags);
  if (rc == hipSuccess) Manager::inst().count_host_alloc((long)size);
  return rc;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t sizeBytes,
                          hipMemcpyKind kind, hipStream_t stream) {
  using fn_t =
      hipError_t (*)(void*, const void*, size_t, hipMemcpyKind, hipStream_t);
  static fn_t fn = (fn_t)real("hipMemcpyAsync");
  hiptimer::Scoped sc(stream, CAT_MEMCPY, (double)sizeBytes);
  hipError_t rc = fn(dst, src, sizeBytes, kind, stream);
  sc.finish();
  return rc;
}

}  // extern "C"
