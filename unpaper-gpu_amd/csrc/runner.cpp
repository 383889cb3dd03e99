// runner.cpp — multi-device batch scheduler: the MI355X peer of the reference's
// lib/batch_worker.c + lib/threadpool.c + the decode/encode queues
// (lib/decode_queue.c, lib/encode_queue.c) and the pinned per-stream staging of
// src/pipeline/image_pipeline.c:226-376.
//
// Reference: batch_process_parallel (batch_worker.c:273) submits every job to
// a thread pool; each worker binds a CUDA stream from the pool
// (batch_worker.c:197-212) and runs process_sheet on one sheet.  Jobs are
// independent (fresh SheetProcessState per job, sheet_process.c:29-84), so
// pages shard across devices with no collective.
//
// Here: one host thread per device, each owning K batches (= K HIP streams,
// K in-flight launch sequences of S sheets).  Jobs are pulled in chunks of S
// from one shared counter (BatchQueue peer), so a faster device takes more.
// Host-fed runs move every chunk through a slot's pinned staging:
//   load (host pool: source -> pinned in)   [decode queue peer]
//   H2D + pipeline + D2H on the slot stream [DMA engines + CUs]
//   store (host pool: pinned out -> sink)   [encode queue peer]
// with K slots per device in flight, so the host work of one slot overlaps the
// device work of the others.
//
// This file: the host pool, placement, create/destroy and the two run loops
// (runner_internal.h names the other files).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <thread>

#include "runner_internal.h"

using Clock = std::chrono::steady_clock;

namespace uph {

// Fixed-size host thread pool with a blocking parallel-for; the calling
// thread works too, so a pool shared by several device threads cannot
// deadlock.
class HostPool {
 public:
  // aff: the CPUs the workers run on (a device's NUMA node), or null
  explicit HostPool(int n, const cpu_set_t* aff = nullptr) {
    if (aff) {
      aff_ = *aff;
      pinned_ = true;
    }
    for (int i = 0; i < n; i++) th_.emplace_back([this] { loop(); });
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  int size() const { return (int)th_.size(); }
  // fire-and-forget task (the caller tracks completion itself)
  void submit(std::function<void()> f) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      q_.push_back(std::move(f));
    }
    cv_.notify_one();
  }
  void parallel_for(int n, const std::function<void(int)>& fn) {
    if (n <= 0) return;
    struct Group {
      std::atomic<int> next{0};
      std::atomic<int> left;
      std::mutex mu;
      std::condition_variable cv;
    };
    auto g = std::make_shared<Group>();
    g->left = n;
    auto body = [g, n, &fn] {
      for (;;) {
        const int i = g->next.fetch_add(1);
        if (i >= n) return;
        fn(i);
        if (g->left.fetch_sub(1) == 1) {
          std::lock_guard<std::mutex> lk(g->mu);
          g->cv.notify_all();
        }
      }
    };
    const int helpers = std::min<int>(n - 1, (int)th_.size());
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (int i = 0; i < helpers; i++) q_.push_back(body);
    }
    cv_.notify_all();
    body();
    std::unique_lock<std::mutex> lk(g->mu);
    g->cv.wait(lk, [&] { return g->left.load() == 0; });
    // queued helpers that start after this point find no index left and
    // return without touching `fn`
  }

 private:
  void loop() {
    if (pinned_) pthread_setaffinity_np(pthread_self(), sizeof(aff_), &aff_);
    for (;;) {
      std::function<void()> t;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
        if (stop_ && q_.empty()) return;
        t = std::move(q_.front());
        q_.pop_front();
      }
      t();
    }
  }
  std::vector<std::thread> th_;
  std::deque<std::function<void()>> q_;
  std::mutex mu_;
  std::condition_variable cv_;
  bool stop_ = false;
  cpu_set_t aff_;
  bool pinned_ = false;
};

namespace {

double secs(Clock::time_point a, Clock::time_point b) {
  return std::chrono::duration<double>(b - a).count();
}

// The CPUs of a device's NUMA node (sysfs via its PCI bus id), within the
// CPUs this process may use.  False when the node is unknown (no NUMA, a
// virtual device) or shares no CPU with the process.
bool device_node_cpus(int device, int* node, cpu_set_t* cpus) {
  *node = -1;
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, device) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  for (char* c = bus; *c; c++) *c = (char)tolower((unsigned char)*c);
  char path[256];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
  FILE* f = fopen(path, "r");
  if (!f) return false;
  const bool got = fscanf(f, "%d", node) == 1;
  fclose(f);
  if (!got || *node < 0) return false;
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", *node);
  f = fopen(path, "r");
  if (!f) return false;
  char list[4096] = {0};
  const bool read = fgets(list, sizeof(list), f) != nullptr;
  fclose(f);
  if (!read) return false;
  cpu_set_t allowed;
  CPU_ZERO(cpus);
  if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return false;
  for (char* p = list; *p && *p != '\n';) {  // "a-b,c,d-e"
    char* e;
    const long a = strtol(p, &e, 10);
    long b = a;
    if (e == p) break;
    if (*e == '-') b = strtol(e + 1, &e, 10);
    for (long c = a; c <= b && c < CPU_SETSIZE; c++)
      if (c >= 0 && CPU_ISSET(c, &allowed)) CPU_SET(c, cpus);
    p = *e == ',' ? e + 1 : e;
  }
  return CPU_COUNT(cpus) > 0;
}

}  // namespace
}  // namespace uph

using namespace uph;

namespace {

// per-sheet device status after a finished run: a failing wait names the
// sheets through their reports
void collect_failures(Slot& sl) {
  sl.failed.assign((size_t)sl.count, 0);
  if (uphip_batch_wait(sl.b) == 0) return;
  uphip_clear_error();
  for (int s = 0; s < sl.count; s++) {
    UphipSheetReport rep;
    if (uphip_batch_get_report(sl.b, s, &rep) != 0 || rep.flags) sl.failed[(size_t)s] = 1;
  }
}

// Sheets per batch when the caller leaves it to the runner: the sheet's
// input pages plus its two working planes (GRAY8 for gray inputs, RGB24
// otherwise, as the batch plans them) within 2 GiB, at most 64 (the batch
// size the A4 measurements use) and at least 1.
int32_t auto_capacity(const UphipOptions& o, const UphipBatchGeometry& g) {
  const int64_t w = g.page_width, h = g.page_height;
  const int n_in = o.input_count > 0 ? o.input_count : 1;
  const bool gray = g.page_format == UPHIP_FMT_GRAY8 || g.page_format == UPHIP_FMT_MONOWHITE ||
                    g.page_format == UPHIP_FMT_MONOBLACK;
  const int64_t in = round_pitch(row_bytes((int32_t)w, g.page_format)) * h * n_in;
  const int64_t plane = (gray ? 1 : 3) * w * n_in * h;
  const int64_t per_sheet = std::max<int64_t>(in + 2 * plane, 1);
  return (int32_t)std::max<int64_t>(1, std::min<int64_t>(64, (2ll << 30) / per_sheet));
}

// The devices' results of a finished run into the runner's stats; the number
// of failed jobs, the first error recorded.
int fold_stats(UphipRunner* r, Clock::time_point t0, double load_s, double store_s) {
  memset(&r->stats, 0, sizeof(r->stats));
  std::string err;
  for (size_t i = 0; i < r->dev.size(); i++) {
    DeviceCtx& dc = r->dev[i];
    r->stats.jobs_done += dc.done;
    r->stats.jobs_failed += dc.failed;
    if (i < UPHIP_RUNNER_MAX_DEVICES) r->stats.jobs_per_device[i] = dc.done;
    if (err.empty() && !dc.error.empty()) err = dc.error;
  }
  r->stats.load_s = load_s;
  r->stats.store_s = store_s;
  r->stats.wall_s = secs(t0, Clock::now());
  if (!err.empty()) fail("runner: %s", err.c_str());
  return (int)std::min<int64_t>(r->stats.jobs_failed, 1 << 30);
}

// Pinned staging per slot, laid out like the batch's input slots: each
// device's from a thread on its node (hipHostMalloc places pinned memory on
// the node nearest the current device; the thread's binding makes any
// first-touch local too).  All or nothing: a later call allocates afresh.
bool ensure_staging(UphipRunner* r) {
  if (r->staged) return true;
  const size_t in = (size_t)(r->in_page_stride * r->geo.capacity * r->opts.input_count);
  const size_t out = (size_t)(r->out_sheet_stride * r->geo.capacity);
  std::atomic<bool> ok{true};
  std::vector<std::thread> th;
  for (DeviceCtx& dc : r->dev)
    th.emplace_back([&ok, in, out, pdc = &dc] {
      pdc->bind();
      uphip_set_device(pdc->device);
      for (Slot& sl : pdc->slots)
        if (!sl.hin.reserve(in) || !sl.hout.reserve(out)) ok = false;
      if (!ok) uphip_clear_error();  // reported below from this thread
    });
  for (auto& t : th) t.join();
  if (!ok) {
    fail("runner: pinned staging allocation failed");
    for (DeviceCtx& dc : r->dev)
      for (Slot& sl : dc.slots) {
        sl.hin.release();
        sl.hout.release();
      }
  }
  return r->staged = ok;
}

// The dense device chunk a direct memory source is copied into, per slot.
bool ensure_direct_input(UphipRunner* r, size_t bytes) {
  const int caller_dev = uphip_get_device();
  bool ok = true;
  for (DeviceCtx& dc : r->dev) {
    uphip_set_device(dc.device);
    for (Slot& sl : dc.slots) ok &= sl.din.reserve(bytes);
  }
  uphip_set_device(caller_dev);
  return ok;
}

// What the device threads of one host-fed run share.
struct HostRun {
  UphipRunner* r;
  int64_t njobs;
  UphipSource* src;
  UphipSink* sink;
  // Direct paths: a memory source whose pages all exist is copied H2D from
  // the caller's (registered) buffer into a dense device chunk that the batch
  // reads in place (uphip_batch_run_device takes any pitch); a memory sink
  // laid out like the batch's output rows receives the D2H copy itself.
  bool dsrc = false, dsnk = false;
  int64_t in_extent = 0;  // bytes from a source page's first to its last
  std::atomic<int64_t> next{0};  // the first job no slot has taken
  std::atomic<int64_t> load_ns{0}, store_ns{0};
};

enum : int { FREE = 0, LOADING, LOADED, RUNNING, DRAINING, STORING };

// A fixed-sheet run: the first npages pages of the slot's chunk placed by
// their own sizes, every other input slot of the batch (all of them for a
// source without sizes) back at the geometry's: no size outlives its chunk.
bool place_pages(UphipRunner* r, Slot* sl, int npages) {
  if (!r->fixed_sheet) return true;
  for (int q = 0; q < r->geo.capacity * r->opts.input_count; q++) {
    const PageSize ps = q < npages ? sl->psize[(size_t)q] : PageSize{};
    const bool full = ps.w == r->geo.page_width && ps.h == r->geo.page_height;
    if (uphip_batch_set_page_size(sl->b, q, full ? 0 : ps.w, full ? 0 : ps.h) != 0) return false;
  }
  return true;
}

// One device thread's slots in a host-fed run.  A slot moves FREE -> LOADING
// (page tasks on the host pool) -> LOADED (last task) -> RUNNING (H2D +
// pipeline queued on its stream) -> DRAINING (status read, D2H queued) ->
// STORING (sheet tasks on the pool) -> FREE (last task).  The device thread
// only moves slots along and never does host copies itself, so decode, DMA,
// kernels and encode of different slots overlap.  `state` is what the pool
// tasks and the device thread share, `phase` the device thread's own view:
// a slot FREE in state and STORING in phase has a chunk to account.
struct SlotLoop {
  HostRun& run;
  DeviceCtx& dc;
  UphipRunner* const r;
  const UphipSink* const sink;
  const int K, S, nin;
  std::unique_ptr<std::atomic<int>[]> state, pend;
  std::vector<int> phase;
  std::deque<int> inflight;  // RUNNING / DRAINING slots in submission order
  bool jobs_left = true;

  SlotLoop(HostRun& hr, DeviceCtx& d)
      : run(hr), dc(d), r(hr.r), sink(hr.sink), K((int)d.slots.size()), S(hr.r->geo.capacity),
        nin(hr.r->opts.input_count), state(new std::atomic<int>[K]), pend(new std::atomic<int>[K]), phase(K, FREE) {
    for (int k = 0; k < K; k++) {
      state[k] = FREE;
      pend[k] = 0;
    }
  }
  Slot* slot(int k) { return &dc.slots[(size_t)k]; }

  void note(const char* what) {
    if (dc.error.empty()) dc.error = uphip_last_error() ? uphip_last_error() : what;
    uphip_clear_error();
  }

  // every sheet of the chunk failed on the device: accounted on the next pass
  void fail_chunk(int k, const char* what) {
    Slot* sl = slot(k);
    note(what);
    for (int s = 0; s < sl->count; s++) sl->failed[(size_t)s] |= 1;
    phase[k] = STORING;
    state[k] = FREE;
  }

  // stored (or failed): count the chunk's sheets
  void account_chunk(int k) {
    Slot* sl = slot(k);
    for (int s = 0; s < sl->count; s++) {
      if (sl->failed[(size_t)s]) {
        dc.failed++;
        if ((sl->failed[(size_t)s] & 2) && dc.error.empty()) dc.error = "a sheet could not be stored";
        if ((sl->failed[(size_t)s] & 4) && dc.error.empty()) {
          const std::string& why = sl->load_error[(size_t)s];
          dc.error = why.empty() ? "a page could not be loaded" : "a page could not be loaded: " + why;
        }
      } else {
        dc.done++;
      }
    }
    phase[k] = FREE;
  }

  // A free slot takes the next chunk of jobs: a direct source's goes to the
  // device at once, any other's pages to the pool's load tasks.  False when
  // no jobs are left.
  bool begin_chunk(int k) {
    Slot* sl = slot(k);
    const int64_t first = run.next.fetch_add(S);
    if (first >= run.njobs) return jobs_left = false;
    sl->first = first;
    sl->jdev = false;
    sl->tdev = false;
    sl->count = (int32_t)std::min<int64_t>(S, run.njobs - first);
    sl->failed.assign((size_t)sl->count, 0);
    sl->load_error.assign((size_t)sl->count, std::string());
    sl->psize.assign((size_t)(sl->count * nin), PageSize{});
    sl->last_first = first;
    sl->last_count = sl->count;
    if (run.dsrc) {
      submit_chunk(k);
      return true;
    }
    if (sl->jpg.size() < (size_t)(sl->count * nin)) sl->jpg.resize((size_t)(sl->count * nin));
    for (JpegPage& jp : sl->jpg) jp.on = false;
    if (sl->tif.size() < (size_t)(sl->count * nin)) sl->tif.resize((size_t)(sl->count * nin));
    for (TiffPage& tp : sl->tif) tp.on = false;
    pend[k] = sl->count;
    state[k] = LOADING;
    phase[k] = LOADING;
    for (int s = 0; s < sl->count; s++) dc.pool->submit([this, sl, k, s] { load_sheet(sl, k, s); });
    return true;
  }

  // pool task: the input pages of sheet s into the slot's staging
  void load_sheet(Slot* sl, int k, int s) {
    const auto a = Clock::now();
    for (int j = 0; j < nin; j++) {
      uint8_t* dst = sl->hin.as() + ((int64_t)s * nin + j) * r->in_page_stride;
      const size_t q = (size_t)(s * nin + j);
      if (!load_page(r, dc.device, run.src, sl->first + s, j, dst, &sl->jpg[q], &sl->tif[q], &sl->psize[q])) {
        sl->jpg[q].on = sl->tif[q].on = false;
        sl->psize[q] = PageSize{};  // the blank page below is of the geometry's size
        sl->failed[(size_t)s] |= 4;
        if (uphip_last_error() && sl->load_error[(size_t)s].empty()) sl->load_error[(size_t)s] = uphip_last_error();
        uphip_clear_error();
        // the slot still runs: a blank (white) page, cheap and
        // deterministic, instead of stale staging bytes
        memset(dst, r->geo.page_format == UPHIP_FMT_MONOWHITE ? 0x00 : 0xFF, (size_t)r->in_page_stride);
      }
    }
    run.load_ns += (int64_t)(secs(a, Clock::now()) * 1e9);
    if (pend[k].fetch_sub(1) == 1) state[k] = LOADED;
  }

  // The chunk's pages to the device (a direct source: one DMA copy from the
  // caller's pages; else the staging and the pages' device decode), the run,
  // then the sink's encode, all queued on the slot's stream.
  void submit_chunk(int k) {
    Slot* sl = slot(k);
    const UphipSource* src = run.src;
    const int npages = sl->count * nin;
    bool ok;
    if (run.dsrc) {
      const size_t bytes = (size_t)((npages - 1) * src->page_stride + run.in_extent);
      ok = place_pages(r, sl, 0) && UPH_HIP(hipMemcpyAsync(sl->din.as(), src->base + sl->first * nin * src->page_stride, bytes,
                                  hipMemcpyHostToDevice, (hipStream_t)uphip_batch_stream(sl->b))) &&
           uphip_batch_run_device(sl->b, sl->count, sl->din.as(), src->linesize, src->page_stride) == 0;
    } else {
      ok = place_pages(r, sl, npages) && upload_staging(r, sl, npages) && jpeg_submit(sl, npages) &&
           tiff_submit(sl, npages) && uphip_batch_run(sl->b, sl->count) == 0;
    }
    const PackedCodec* pc = packed_codec(sink, r->out_fmt);
    if (!ok || (pc && pc->encode(sl->b, sink) != 0)) return fail_chunk(k, "run failed");
    phase[k] = RUNNING;
    state[k] = RUNNING;
    inflight.push_back(k);
  }

  // a finished run's per-sheet status (the stream is idle: a status read only)
  void read_status(Slot* sl) {
    std::vector<char> pre = sl->failed;
    collect_failures(*sl);
    for (size_t s = 0; s < pre.size(); s++) sl->failed[s] |= pre[s];
    // pages whose entropy-coded data, or whose TIFF strips, the device found corrupt
    std::vector<int32_t> jst((size_t)(sl->count * nin), 0);
    auto page_status = [&](bool any, const Buffer& dst, const char* what) {
      if (!any) return;
      if (!UPH_HIP(hipMemcpy(jst.data(), dst.as(), 4 * jst.size(), hipMemcpyDeviceToHost)))
        jst.assign(jst.size(), 1);
      for (size_t q = 0; q < jst.size(); q++)
        if (jst[q]) {
          sl->failed[q / (size_t)nin] |= 4;
          if (dc.error.empty()) dc.error = what;
        }
    };
    page_status(sl->jdev, sl->djst, "corrupt JPEG entropy-coded data (device decode)");
    page_status(sl->tdev, sl->dtst, "corrupt TIFF strip (device decode)");
  }

  // A finished run: its status, then its D2H queued -- the sheets, or what
  // the sink's codec made of them.  False when the chunk failed instead.
  bool drain_chunk(int k) {
    Slot* sl = slot(k);
    read_status(sl);
    // straight into a memory sink unless a sheet failed (its slot in the
    // sink stays untouched, as with the store tasks)
    bool clean = true;
    for (int s = 0; s < sl->count; s++) clean &= !sl->failed[(size_t)s];
    sl->direct_out = run.dsnk && clean;
    bool queued;
    if (const PackedCodec* pc = packed_codec(sink, r->out_fmt)) {
      // only the encoded files come back: sizes (already on the host), then
      // one copy of the packed files
      const int npg = sl->count * r->oc;
      sl->jsize.assign((size_t)npg, -1);
      sl->joff.assign((size_t)npg, 0);
      const int64_t total = pc->sizes(sl->b, sl->jsize.data(), npg);
      int64_t o = 0;
      for (int i = 0; i < npg; i++) {
        sl->joff[(size_t)i] = o;
        if (sl->jsize[(size_t)i] > 0) o += sl->jsize[(size_t)i];
      }
      queued = total >= 0 && sl->hjpg.reserve((size_t)total, (size_t)total / 2 + 4096) &&
               pc->download(sl->b, sl->hjpg.as(), (int64_t)sl->hjpg.capacity()) == 0;
    } else if (sink->codec == UphipSink::Codec::Jp2) {
      // the chunk's pages coded on the device; the store tasks write
      queued = jp2_chunk_submit(r, sl, sl->count * r->oc);
    } else {
      uint8_t* dst = sl->direct_out ? sink->base + sl->first * sink->sheet_stride : sl->hout.as();
      queued = uphip_batch_download_async(sl->b, dst, r->out_linesize, r->out_sheet_stride) == 0;
    }
    if (!queued) return fail_chunk(k, "download failed"), false;
    phase[k] = DRAINING;
    state[k] = DRAINING;
    return true;
  }

  // The D2H is done: the chunk's good sheets to the pool's store tasks.
  void store_chunk(int k) {
    Slot* sl = slot(k);
    int nstore = 0;
    for (int s = 0; s < sl->count; s++) nstore += !sl->failed[(size_t)s];
    phase[k] = STORING;
    if (sl->direct_out || nstore == 0) {  // the copy went straight into the sink, or nothing to store
      state[k] = FREE;
      return;
    }
    pend[k] = nstore;
    state[k] = STORING;
    for (int s = 0; s < sl->count; s++) {
      if (sl->failed[(size_t)s]) continue;
      dc.pool->submit([this, sl, k, s] {
        const auto a = Clock::now();
        bool good = true;
        store_chunk_sheet(r, sink, dc.device, sl, s, &good);
        if (!good) {
          sl->failed[(size_t)s] |= 2;
          uphip_clear_error();
        }
        run.store_ns += (int64_t)(secs(a, Clock::now()) * 1e9);
        if (pend[k].fetch_sub(1) == 1) state[k] = FREE;
      });
    }
  }

  void loop() {
    for (;;) {
      bool progress = false;
      for (int k = 0; k < K; k++) {
        const int st = state[k].load();
        if (st == FREE && phase[k] == STORING) {
          account_chunk(k);
          progress = true;
        }
        if (st == FREE && phase[k] == FREE && jobs_left) progress |= begin_chunk(k);
        if (st == LOADED && phase[k] == LOADING) {
          submit_chunk(k);
          progress = true;
        }
      }
      // the oldest slots on the GPU: a finished run -> its D2H; a finished
      // D2H -> the sink, in submission order
      for (size_t q = 0; q < inflight.size();) {
        const int k = inflight[q];
        if (uphip_batch_query(slot(k)->b) != 1) break;
        progress = true;
        if (phase[k] == RUNNING && drain_chunk(k)) {
          q++;  // stays in flight until its copy is done
          continue;
        }
        inflight.erase(inflight.begin() + (long)q);
        if (phase[k] == DRAINING) store_chunk(k);  // else the drain failed the chunk
      }
      bool idle = !jobs_left;
      for (int k = 0; k < K && idle; k++) idle = state[k].load() == FREE && phase[k] == FREE;
      if (idle) break;
      if (!progress) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  }
};

}  // namespace

extern "C" {

UphipRunner* uphip_runner_create(const UphipOptions* options, const UphipBatchGeometry* geometry,
                                 const UphipRunnerConfig* config) {
  if (!options || !geometry || !config) return fail("runner_create: null argument"), nullptr;
  if (!runtime_ready()) return fail("runner_create: no HIP device"), nullptr;
  const int ndev_all = uphip_device_count();
  if (config->ndevices <= 0 || geometry->page_width <= 0 || geometry->page_height <= 0)
    return fail("runner_create: invalid configuration"), nullptr;
  UphipRunner* r = new UphipRunner();
  r->opts = *options;
  r->geo = *geometry;
  r->fixed_sheet = options->sheet_size.width != -1 && options->sheet_size.height != -1 && options->pre_rotate == 0;
  r->cfg = *config;
  r->oc = options->output_count < 1 ? 1 : options->output_count;
  if (r->geo.capacity <= 0) r->geo.capacity = auto_capacity(*options, *geometry);
  for (int i = 0; i < config->ndevices; i++) {
    const int d = config->devices ? config->devices[i] : i;
    if (d < 0 || d >= ndev_all) {
      delete r;
      return fail("runner_create: device %d out of range (%d devices)", d, ndev_all), nullptr;
    }
    r->devices.push_back(d);
  }
  const int caller_dev = uphip_get_device();
  r->dev.resize(r->devices.size());
  bool ok = true;
  for (size_t i = 0; ok && i < r->devices.size(); i++) {
    DeviceCtx& dc = r->dev[i];
    dc.device = r->devices[i];
    if (uphip_set_device(dc.device) != 0) {
      ok = false;
      break;
    }
    // the first batch measures the footprint the auto layout divides by
    if (i == 0) {
      UphipBatch* b = uphip_batch_create(options, &r->geo);
      if (!b) {
        ok = false;
        break;
      }
      int64_t bb = 0;
      uphip_batch_device_bytes(b, &bb);
      r->batch_bytes = bb;
      if (config->batches_per_device <= 0) {
        // per slot: the batch, plus the dense input chunk a direct memory
        // source is copied into (allocated at the first host run)
        int64_t ip = 0;
        uphip_batch_input_ptr(b, 0, &ip);
        const int64_t din = ip * r->geo.page_height * r->geo.capacity *
                            (options->input_count > 0 ? options->input_count : 1);
        size_t fr = 0, tot = 0;
        int n = 1;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && bb > 0)
          n = 1 + (int)std::min<int64_t>((int64_t)(fr / 2) / (bb + din), 15);
        r->cfg.batches_per_device = n;
      }
      dc.slots.resize((size_t)r->cfg.batches_per_device);
      dc.slots[0].b = b;
    } else {
      dc.slots.resize((size_t)r->cfg.batches_per_device);
    }
    for (Slot& sl : dc.slots) {
      if (!sl.b) sl.b = uphip_batch_create(options, &r->geo);
      if (!sl.b) {
        ok = false;
        break;
      }
      if (config->timing) uphip_batch_set_timing(sl.b, 1);
    }
  }
  uphip_set_device(caller_dev);
  if (!ok) {
    uphip_runner_destroy(r);
    return nullptr;
  }
  UphipBatch* b0 = r->dev[0].slots[0].b;
  int64_t bytes = 0;
  uphip_batch_output_info(b0, &r->out_w, &r->out_h, &r->out_fmt, &bytes);
  uphip_batch_input_ptr(b0, 0, &r->in_pitch);
  r->in_page_stride = r->in_pitch * r->geo.page_height;
  // output staging laid out like the batch's output rows, so a batch's
  // sheets come back as linear DMA copies
  {
    int64_t op = 0;
    UphipBatch* bb = r->dev[0].slots[0].b;
    r->out_linesize = round_pitch(row_bytes(r->out_w, r->out_fmt));
    if (uphip_batch_output_pitch(bb, &op) == 0 && op >= row_bytes(r->out_w, r->out_fmt))
      r->out_linesize = op;
  }
  r->out_sheet_stride = r->out_linesize * r->out_h;
  // load/store pools: one per device, its share of the host threads, on the
  // device's NUMA node (the decode/encode queues' workers, lib/decode_queue.c)
  const int nd = (int)r->devices.size();
  const int ht = config->host_threads > 0 ? config->host_threads : 4 * nd;
  for (int i = 0; i < nd; i++) {
    DeviceCtx& dc = r->dev[(size_t)i];
    dc.pinned = device_node_cpus(dc.device, &dc.numa, &dc.cpus);
    const int share = std::max(1, ht / nd + (i < ht % nd ? 1 : 0));
    dc.pool = new HostPool(share, dc.pinned ? &dc.cpus : nullptr);
  }
  return r;
}

void uphip_runner_destroy(UphipRunner* r) {
  if (!r) return;
  for (DeviceCtx& dc : r->dev) {
    delete dc.pool;
    dc.pool = nullptr;
  }
  for (DeviceCtx& dc : r->dev) {
    uphip_set_device(dc.device);
    for (Slot& sl : dc.slots)
      if (sl.b) uphip_batch_destroy(sl.b);
    dc.slots.clear();  // the slots' buffers free themselves, on their device
  }
  delete r;
}

int uphip_runner_layout(UphipRunner* r, int32_t* batches_per_device, int32_t* capacity,
                        int64_t* batch_bytes) {
  if (!r) return fail("runner_layout: null runner"), -1;
  if (batches_per_device) *batches_per_device = r->cfg.batches_per_device;
  if (capacity) *capacity = r->geo.capacity;
  if (batch_bytes) *batch_bytes = r->batch_bytes;
  return 0;
}

int uphip_runner_placement(UphipRunner* r, int32_t device_index, int32_t* numa_node,
                           int32_t* ncpus, int32_t* pool_threads) {
  if (!r || device_index < 0 || device_index >= (int)r->dev.size())
    return fail("runner_placement: bad device index"), -1;
  const DeviceCtx& dc = r->dev[(size_t)device_index];
  if (numa_node) *numa_node = dc.pinned ? dc.numa : -1;
  if (ncpus) *ncpus = dc.pinned ? CPU_COUNT(&dc.cpus) : 0;
  if (pool_threads) *pool_threads = dc.pool ? dc.pool->size() : 0;
  return 0;
}

int64_t uphip_runner_slot_chunk(UphipRunner* r, int32_t device_index, int32_t slot,
                                int32_t* count) {
  if (!r || device_index < 0 || device_index >= (int)r->dev.size() || slot < 0 ||
      slot >= (int)r->dev[(size_t)device_index].slots.size())
    return fail("runner_slot_chunk: bad arguments"), -1;
  const Slot& sl = r->dev[(size_t)device_index].slots[(size_t)slot];
  if (count) *count = sl.last_first >= 0 ? sl.last_count : 0;
  return sl.last_first;
}

UphipBatch* uphip_runner_batch(UphipRunner* r, int32_t device_index, int32_t slot) {
  if (!r || device_index < 0 || device_index >= (int)r->dev.size() || slot < 0 ||
      slot >= (int)r->dev[(size_t)device_index].slots.size())
    return nullptr;
  return r->dev[(size_t)device_index].slots[(size_t)slot].b;
}

int uphip_runner_run_device(UphipRunner* r, const UphipDevicePages* shards, int32_t passes) {
  if (!r || !shards || passes < 1) return fail("runner_run_device: bad arguments"), -1;
  const auto t0 = Clock::now();
  const int S = r->geo.capacity;
  std::vector<std::thread> th;
  for (size_t i = 0; i < r->dev.size(); i++) {
    th.emplace_back([r, i, S, shards, passes] {
      DeviceCtx& dc = r->dev[i];
      dc.done = dc.failed = 0;
      dc.error.clear();
      const auto a = Clock::now();
      dc.bind();
      uphip_set_device(dc.device);
      const UphipDevicePages& sh = shards[i];
      const int64_t nin = r->opts.input_count;
      const size_t ns = dc.slots.size();
      std::vector<int32_t> used(ns, 0);
      // Each chunk goes to a slot whose stream is idle (the first batches to
      // the slots in order, then to whichever finishes first), so a slow
      // chunk -- a sheet whose blackfilter replay runs long -- delays only its
      // own slot: a fixed chunk -> slot mapping would queue every later chunk
      // of that slot, pass after pass, behind it.
      size_t next_fresh = 0;
      auto idle_slot = [&]() -> size_t {
        if (next_fresh < ns) return next_fresh++;
        for (;;) {
          for (size_t s = 0; s < ns; s++)
            if (uphip_batch_query(dc.slots[s].b) != 0) return s;  // idle, or failed (run reports)
          std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
      };
      for (int32_t pass = 0; pass < passes; pass++)
      for (int64_t first = 0; first < sh.count; first += S) {
        const int32_t n = (int32_t)std::min<int64_t>(S, sh.count - first);
        const size_t k = idle_slot();
        Slot& sl = dc.slots[k];
        if (!place_pages(r, &sl, 0) ||
            uphip_batch_run_device(sl.b, n, (const uint8_t*)sh.pages + first * nin * sh.page_stride,
                                   sh.pitch, sh.page_stride) != 0) {
          if (dc.error.empty()) dc.error = uphip_last_error() ? uphip_last_error() : "run failed";
          uphip_clear_error();
          dc.failed += n;
          continue;
        }
        used[k] = n;
        sl.last_first = first;
        sl.last_count = n;
        dc.done += n;
      }
      for (size_t s = 0; s < dc.slots.size(); s++) {
        if (!used[s]) continue;
        if (uphip_batch_wait(dc.slots[s].b) != 0) {
          if (dc.error.empty()) dc.error = uphip_last_error() ? uphip_last_error() : "wait failed";
          uphip_clear_error();
          dc.failed += 1;  // at least one sheet; the sticky status does not say how many
        }
      }
      dc.busy_s = secs(a, Clock::now());
    });
  }
  for (auto& t : th) t.join();
  return fold_stats(r, t0, 0, 0);
}

int uphip_runner_run_host(UphipRunner* r, int64_t njobs, UphipSource* src, UphipSink* sink) {
  if (!r || !src || !sink || njobs < 0) return fail("runner_run_host: bad arguments"), -1;
  if (sink->codec == UphipSink::Codec::G4 && r->out_fmt != UPHIP_FMT_MONOWHITE)
    return fail("runner_run_host: a Group 4 sink takes bilevel sheets and this runner's leave in format %d: "
                "set output_pixel_format to UPHIP_FMT_MONOWHITE", r->out_fmt), -1;
  // the batch saves Y400A sheets as GRAY8 (saveImage's mapping); a PDF asked
  // for gray with alpha would silently lose the alpha, so it is refused
  if (sink->codec == UphipSink::Codec::Png && sink->pdfw &&
      (r->opts.output_pixel_format == UPHIP_FMT_NONE ? r->geo.page_format : r->opts.output_pixel_format) ==
          UPHIP_FMT_Y400A)
    return fail("runner_run_host: a lossless PDF sink cannot take Y400A sheets (PDF images carry no alpha "
                "sample): set output_pixel_format to another format"), -1;
  if (!ensure_staging(r)) return -1;
  const int S = r->geo.capacity;
  const int nin = r->opts.input_count;
  HostRun run{r, njobs, src, sink};
  // The direct source needs pages the batch can read in place: rows at least
  // a row long and pages that do not overlap (page_stride 0, a repeated page,
  // or overlapping pages take the staged path, which copies page by page).
  const int64_t in_row = row_bytes(r->geo.page_width, r->geo.page_format);
  run.in_extent = (int64_t)(r->geo.page_height - 1) * src->linesize + in_row;
  run.dsrc = src->base && !src->load && src->npages >= njobs * nin && njobs > 0 &&
             src->linesize >= in_row && src->page_stride >= run.in_extent &&
             src->reg.ensure(src->base, (size_t)((src->npages - 1) * src->page_stride + run.in_extent));
  const int64_t out_extent =
      (int64_t)(r->out_h - 1) * r->out_linesize + row_bytes(r->out_w, r->out_fmt);
  run.dsnk = sink->base && !sink->store && r->oc == 1 && sink->nsheets >= njobs && njobs > 0 &&
             sink->linesize == r->out_linesize && sink->sheet_stride == r->out_sheet_stride &&
             sink->reg.ensure(sink->base, (size_t)((sink->nsheets - 1) * sink->sheet_stride + out_extent));
  if (run.dsrc && !ensure_direct_input(r, (size_t)(src->page_stride * S * nin))) return -1;
  const auto t0 = Clock::now();
  std::vector<std::thread> th;
  for (DeviceCtx& dc : r->dev)
    th.emplace_back([&run, pdc = &dc] {
      pdc->done = pdc->failed = 0;
      pdc->error.clear();
      pdc->bind();
      uphip_set_device(pdc->device);
      SlotLoop(run, *pdc).loop();
    });
  for (auto& t : th) t.join();
  return fold_stats(r, t0, run.load_ns.load() * 1e-9, run.store_ns.load() * 1e-9);
}

int uphip_runner_get_stats(UphipRunner* r, UphipRunnerStats* out) {
  if (!r || !out) return -1;
  *out = r->stats;
  return 0;
}

int uphip_runner_output_info(UphipRunner* r, int32_t* width, int32_t* height, int32_t* format,
                             int64_t* linesize) {
  if (!r) return -1;
  if (width) *width = r->out_w;
  if (height) *height = r->out_h;
  if (format) *format = r->out_fmt;
  if (linesize) *linesize = r->out_linesize;
  return 0;
}

}  // extern "C"
