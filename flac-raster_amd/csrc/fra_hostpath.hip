// fra_hostpath.hip -- the host pipeline: fra_plan_encode_host, _progress and _ring.  Row bands of a host raster go
// H2D while earlier bands are analysed (fra_exec.hip run_host_band), and each band's frames come back D2H as soon
// as they are assembled.  No kernels here.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <ctime>
#include <deque>
#include <thread>

#include "fra_plan.h"

using namespace fra;

// the host raster of an encode: image row r of channel c at row r % rows of plane c.  A whole raster never wraps
// (rows = INT64_MAX, planes a band stride apart); the bounded-memory ring of fra_plan_encode_ring does (planes of
// `rows` rows), and its completed copies are published in rows_done
struct HostRows {
  const uint8_t* base;
  int64_t rows;
  int64_t plane;  // elements between the channels of a band-planar raster
  volatile int64_t* rows_done;
};
// the copies below move rows as runs: one run per channel for band-planar rasters (band_stride >= row_stride), one
// run holding every channel for pixel- and line-interleaved ones
static bool planar_runs(const fra_job& j) { return j.channels > 1 && j.band_stride >= j.row_stride; }
// rows the plan's windows reach ([0, rows)) and the elements one such row spans from its first element: up to the
// last window column, in a run of every channel up to the last channel's
static void row_extent(const fra_plan* p, int64_t* rows, int64_t* span) {
  const fra_job& j = p->job;
  int64_t nr = 0, cols = 0;
  for (const fra_window& w : p->windows)
    if (w.height > 0 && w.width > 0) {
      nr = std::max<int64_t>(nr, (int64_t)w.row_off + w.height);
      cols = std::max<int64_t>(cols, (int64_t)w.col_off + w.width);
    }
  *rows = nr;
  *span = cols ? (cols - 1) * j.col_stride + (planar_runs(j) ? 0 : (int64_t)(j.channels - 1) * j.band_stride) + 1 : 0;
}
// H2D of raster rows [r0, r1) of every band (channel) of the job: one contiguous run per channel for band-planar
// rasters, one run for interleaved ones -- split where a ring wraps --, clamped to the plan's extent (the last row
// of the last channel may end before row_stride does).  A run ends with its last row (`span`, <= row_stride
// unless the raster has one row only: encode_host refuses rows that overlap)
static int copy_rows_h2d(fra_plan* p, const HostRows& h, int64_t span, int64_t r0, int64_t r1, hipStream_t st) {
  const fra_job& j = p->job;
  const int es = elem_size(j.dtype);
  const int64_t extent = (int64_t)(p->raster_bytes / es);
  const bool planar = planar_runs(j);
  const int nrun = planar ? j.channels : 1;
  for (int c = 0; c < nrun; c++) {
    const int64_t dbase = (int64_t)c * (planar ? j.band_stride : 0);
    const int64_t hbase = (int64_t)c * (planar ? h.plane : 0);
    for (int64_t r = r0; r < r1;) {
      const int64_t rr = r % h.rows, n = std::min(r1 - r, h.rows - rr);
      const int64_t a = dbase + r * j.row_stride;
      const int64_t b = std::min(extent, dbase + (r + n - 1) * j.row_stride + std::max(j.row_stride, span));
      if (b > a)
        HIPCHK(hipMemcpyAsync((uint8_t*)p->d_raster_owned + a * es, h.base + (hbase + rr * j.row_stride) * es,
                              (size_t)(b - a) * es, hipMemcpyHostToDevice, st));
      r += n;
    }
  }
  return FRA_OK;
}

// page-locked (hipHostMalloc'd or registered) host memory: an async copy to it returns at once
static bool host_pinned(const void* ptr) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeHost;
}
// encode_host's D2H copies into a pageable output, on threads of their own (`out` null: off, the caller copies
// itself).  The runtime's own copy into pageable memory stages through one pinned buffer and copies out on the
// calling thread, page faults of a lazily committed buffer included: about 17 GB/s, so C5's 22.4 GB of frames
// outlasted the 34 GB raster's H2D by 0.6 s (profiles/r05_ring_timeline.txt).  Here each of n threads owns a
// 64 MiB piece of page-locked staging: DMA the piece into it at the link rate, then copy it out on that thread,
// so the copy-outs and their page faults run n-wide beside the DMA.  push() takes a byte range whose frames are
// complete on the device.
struct D2HWorker {
  static constexpr uint64_t kPiece = 64ull << 20;
  D2HWorker(int device, uint8_t* out, const uint8_t* dev, uint8_t* stage, const std::vector<hipStream_t>& st)
      : out_(out), dev_(dev) {
    if (!out_) return;
    for (size_t i = 0; i < st.size(); i++)
      th_.emplace_back([this, device, stage, i, s = st[i]]() { run(device, stage + (uint64_t)i * kPiece, s); });
  }
  ~D2HWorker() { finish(); }
  bool on() const { return out_ != nullptr; }
  void push(uint64_t a, uint64_t b) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (uint64_t x = a; x < b; x += kPiece) q_.emplace_back(x, std::min(b, x + kPiece));
    }
    cv_.notify_all();
  }
  // wait for every pushed copy; false if one failed (error())
  bool finish() {
    if (!th_.empty()) {
      { std::lock_guard<std::mutex> lk(mu_); end_ = true; }
      cv_.notify_all();
      for (auto& t : th_) t.join();
      th_.clear();
    }
    return err_.empty();
  }
  const std::string& error() const { return err_; }

 private:
  void run(int device, uint8_t* stage, hipStream_t st) {
    hipError_t e = hipSetDevice(device);
    for (;;) {
      std::pair<uint64_t, uint64_t> r;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return !q_.empty() || end_; });
        if (q_.empty()) break;
        r = q_.front();
        q_.pop_front();
      }
      if (e != hipSuccess) continue;  // drain the queue after a failure
      const size_t n = (size_t)(r.second - r.first);
      e = hipMemcpyAsync(stage, dev_ + r.first, n, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e == hipSuccess) memcpy(out_ + r.first, stage, n);
    }
    if (e != hipSuccess) {
      std::lock_guard<std::mutex> lk(mu_);
      if (err_.empty()) err_ = hipGetErrorString(e);
    }
  }
  uint8_t* out_;
  const uint8_t* dev_;
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::pair<uint64_t, uint64_t>> q_;
  bool end_ = false;
  std::string err_;  // read after the joins
};

// the context's staging and streams for D2HWorker (FRA_D2H_THREADS workers, default 4), made at its first use.
// Built in an arena of its own and committed to the context only when every piece exists (a half-built
// staging set would leave a worker pool with no threads that reports success without copying)
static int ctx_staging(fra_ctx* cx) {
  if (cx->stage) return FRA_OK;
  const int n = env_d2h_threads();
  HipArena made;
  uint8_t* stage = nullptr;
  std::vector<hipStream_t> sts(n);
  hipError_t he = made.pinned(&stage, D2HWorker::kPiece * n, hipHostMallocPortable);
  for (int i = 0; he == hipSuccess && i < n; i++) he = made.stream(&sts[i]);
  if (he != hipSuccess) return set_err(FRA_E_HIP, "D2H staging: %s", hipGetErrorString(he));
  cx->stage_res = std::move(made);
  cx->stage = stage;
  cx->stage_st = std::move(sts);
  return FRA_OK;
}

// the plan's streams, events and offset mirror of the host pipeline, made at its first use
static int plan_host_pipeline(fra_plan* p) {
  const size_t nb = p->hbands.size();
  if (!p->h2d) HIPCHK(p->res.stream(&p->h2d));
  if (!p->d2h) HIPCHK(p->res.stream(&p->d2h));
  if (!p->hev_start) HIPCHK(p->res.event(&p->hev_start));
  while (p->hev.size() < 2 * nb) {
    hipEvent_t e = nullptr;
    HIPCHK(p->res.event(&e));
    p->hev.push_back(e);
  }
  if (!p->h_gbase) {
    HIPCHK(p->res.pinned(&p->h_gbase, sizeof(unsigned long long) * (nb + 1),
                         hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void**)&p->d_gbase_mirror, p->h_gbase, 0));
  }
  return FRA_OK;
}

// wait (host) until the producer has published rows [0, r1) of the raster; false if it reported failure.
// `poll` runs on every spin (the ring path publishes finished H2D copies there, which the producer may need
// before it can publish r1)
template <typename F>
static bool wait_rows(const volatile int64_t* rows_ready, int64_t r1, F&& poll) {
  if (!rows_ready) return true;
  for (int spin = 0;; spin++) {
    const int64_t r = __atomic_load_n(const_cast<const int64_t*>(rows_ready), __ATOMIC_ACQUIRE);
    if (r < 0) return false;
    if (r >= r1) return true;
    poll();
    if (spin < 64) continue;
    struct timespec ts = {0, spin < 1024 ? 2000 : 50000};
    nanosleep(&ts, nullptr);
  }
}

// `ring_rows` 0: host_raster is the whole raster
static int encode_host(fra_plan* p, const void* host_raster, uint8_t* host_out, uint64_t capacity,
                       uint64_t* total_bytes, const volatile int64_t* rows_ready, int64_t ring_rows,
                       volatile int64_t* rows_done) {
  if (!p || (!host_raster && p->raster_bytes) || (!host_out && capacity)) return set_err(FRA_E_INVALID, "null argument");
  // rows go H2D as whole runs of row_stride elements, band after band: a raster whose rows overlap (a zero row
  // stride, a sliding view) would be encoded from rows that have not arrived.  Refused here, before any GPU work
  int64_t nrows = 0, span = 0;
  row_extent(p, &nrows, &span);
  if (nrows > 1 && p->job.row_stride < span)
    return set_err(FRA_E_INVALID,
                   "host raster layout: rows overlap (row_stride %lld < the %lld elements a row spans); the host "
                   "paths copy whole rows -- encode such a raster device-resident (fra_plan_execute)",
                   (long long)p->job.row_stride, (long long)span);
  const bool ring = ring_rows > 0;
  const HostRows host{(const uint8_t*)host_raster, ring ? ring_rows : INT64_MAX,
                      ring ? ring_rows * p->job.row_stride : p->job.band_stride, rows_done};
  (void)hipSetDevice(p->ctx->device);
  hipStream_t s = p->ctx->stream;
  const int nb = (int)p->hbands.size();
  if (total_bytes) *total_bytes = 0;
  if (nb == 0) {  // no windows
    p->executed = true;
    return FRA_OK;
  }
  if (int rc = drain_pipeline(p)) return rc;  // the bands below use buffer set 0 on the plan's stream
  if (int rc = plan_own_raster(p)) return rc;
  p->d_raster = p->d_raster_owned;
  p->args.raster = p->d_raster;
  p->job.raster = host_raster;
  p->job.raster_on_device = 0;
  set_vec8(p);
  const ExecEnv env = env_exec();
  if (int rc = plan_host_pipeline(p)) return rc;
  // H2D runs at most one band ahead of the oldest band whose D2H is not yet issued (unlimited measured
  // slower on C4: 22.2 vs 21.3 ms)
  constexpr int ahead = 1;
  // the copies must not overwrite the device raster while earlier work of this plan still reads it
  HIPCHK(hipEventRecord(p->hev_start, s));
  HIPCHK(hipStreamWaitEvent(p->h2d, p->hev_start, 0));
  HIPCHK(hipStreamWaitEvent(p->d2h, p->hev_start, 0));
  // ring path: bands whose H2D copy is enqueued / known complete; completed bands free their ring rows
  int copies = 0, copied = 0;
  auto publish = [&]() {
    if (!ring) return;
    int64_t done = -1;
    while (copied < copies && hipEventQuery(p->hev[2 * copied]) == hipSuccess) done = p->hbands[copied++].r1;
    if (done >= 0) __atomic_store_n(const_cast<int64_t*>(host.rows_done), done, __ATOMIC_RELEASE);
  };
  auto enqueue_copy = [&](int b) -> int {
    const auto& hb = p->hbands[b];
    if (!wait_rows(rows_ready, hb.r1, publish))
      return set_err(FRA_E_STATE, "the raster producer failed (rows_ready < 0)");
    if (hb.r1 > hb.r0)
      if (int rc = copy_rows_h2d(p, host, span, hb.r0, hb.r1, p->h2d)) return rc;
    HIPCHK(hipEventRecord(p->hev[2 * b], p->h2d));
    copies = b + 1;
    publish();
    return FRA_OK;
  };
  uint64_t beg = 0;
  int issued = 0;  // bands whose D2H has been enqueued
  bool over = false;
  // a pageable output (the ring path's lazily committed frames): a D2H into it returns only once the runtime has
  // staged the whole copy, which would hold this loop -- and with it the next band's H2D and the producer's ring
  // rows -- for every band's frames; those copies go to worker threads instead
  // (the context's staging and streams, held for this call -- a concurrent encode on the same context copies
  // through the runtime instead)
  fra_ctx* cx = p->ctx;
  std::unique_lock<std::mutex> stage_lk(cx->stage_mu, std::defer_lock);
  const bool out_pageable = capacity > 0 && !host_pinned(host_out) && stage_lk.try_lock();
  if (out_pageable)
    if (int rc = ctx_staging(cx)) return rc;
  D2HWorker dw(cx->device, out_pageable ? host_out : nullptr, p->d_out, cx->stage, cx->stage_st);
  auto enqueue_d2h = [&](int b) -> int {
    const uint64_t end = p->h_gbase[b + 1];
    if (end > capacity) over = true;
    if (!over && end > beg) {
      if (dw.on()) {
        dw.push(beg, end);
      } else {
        HIPCHK(hipStreamWaitEvent(p->d2h, p->hev[2 * b + 1], 0));
        HIPCHK(hipMemcpyAsync(host_out + beg, p->d_out + beg, (size_t)(end - beg), hipMemcpyDeviceToHost, p->d2h));
      }
    }
    beg = end;
    return FRA_OK;
  };
  // an error after work was enqueued (a failed producer, a HIP error): drain the three streams (and the D2H
  // worker) before returning, so no copy still reads or writes the caller's buffers
  auto drained = [&](int code) -> int {
    KeepError keep;
    dw.finish();
    (void)hipStreamSynchronize(p->h2d);
    (void)hipStreamSynchronize(s);
    (void)hipStreamSynchronize(p->d2h);
    return code;
  };
  // (a HIP error once copies are in flight also drains: the caller may free or refill its ring on return)
#define HIPCHK_D(x)                                                                                         \
  do {                                                                                                      \
    hipError_t _e = (x);                                                                                    \
    if (_e != hipSuccess)                                                                                   \
      return drained(set_err(FRA_E_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__)); \
  } while (0)
  int rc = enqueue_copy(0);
  if (rc) return drained(rc);
  for (int b = 0; b < nb; b++) {
    if (b + 1 < nb) {  // the next band's rows go over PCIe meanwhile
      while (ahead > 0 && b + 1 - issued > ahead) {
        HIPCHK_D(hipEventSynchronize(p->hev[2 * issued + 1]));
        if ((rc = enqueue_d2h(issued++))) return drained(rc);
      }
      if ((rc = enqueue_copy(b + 1))) return drained(rc);
    }
    HIPCHK_D(hipStreamWaitEvent(s, p->hev[2 * b], 0));
    if ((rc = run_host_band(p, b, env))) return drained(rc);
    HIPCHK_D(hipEventRecord(p->hev[2 * b + 1], s));
    // bands already assembled: their D2H can start now (pageable sources make the H2D enqueue blocking)
    while (issued <= b && hipEventQuery(p->hev[2 * issued + 1]) == hipSuccess)
      if ((rc = enqueue_d2h(issued++))) return drained(rc);
    publish();
  }
  while (issued < nb) {
    HIPCHK_D(hipEventSynchronize(p->hev[2 * issued + 1]));
    if ((rc = enqueue_d2h(issued++))) return drained(rc);
  }
  if (!dw.finish()) return drained(set_err(FRA_E_HIP, "frames D2H: %s", dw.error().c_str()));
  HIPCHK_D(hipStreamSynchronize(p->d2h));
  HIPCHK_D(hipStreamSynchronize(s));
  HIPCHK_D(hipStreamSynchronize(p->h2d));
#undef HIPCHK_D
  publish();
  p->executed = true;
  // a frame the assembly skipped or a frame-scan desync (the device error word) fails the call: the copied
  // frames are not a valid stream
  if ((rc = check_dev_err(p))) return rc;
  if (total_bytes) *total_bytes = beg;
  if (over)
    return set_err(FRA_E_SPACE, "output needs %llu bytes, capacity %llu (frames stay on the device)",
                   (unsigned long long)beg, (unsigned long long)capacity);
  return FRA_OK;
}

extern "C" {

int fra_plan_encode_host(fra_plan* p, const void* host_raster, uint8_t* host_out, uint64_t capacity,
                         uint64_t* total_bytes) {
  return encode_host(p, host_raster, host_out, capacity, total_bytes, nullptr, 0, nullptr);
}
int fra_plan_encode_host_progress(fra_plan* p, const void* host_raster, uint8_t* host_out, uint64_t capacity,
                                  uint64_t* total_bytes, const volatile int64_t* rows_ready) {
  if (!rows_ready) return set_err(FRA_E_INVALID, "null rows_ready");
  return encode_host(p, host_raster, host_out, capacity, total_bytes, rows_ready, 0, nullptr);
}
int fra_plan_encode_ring(fra_plan* p, const void* ring, int64_t ring_rows, uint8_t* host_out, uint64_t capacity,
                         uint64_t* total_bytes, const volatile int64_t* rows_ready, volatile int64_t* rows_done) {
  if (!p || !ring || !rows_ready || !rows_done) return set_err(FRA_E_INVALID, "null argument");
  int64_t mx = 0;
  fra_plan_host_band_rows(p, &mx);
  if (ring_rows < mx || ring_rows < 1)
    return set_err(FRA_E_INVALID, "ring of %lld rows < the tallest host band (%lld rows)", (long long)ring_rows,
                   (long long)mx);
  return encode_host(p, ring, host_out, capacity, total_bytes, rows_ready, ring_rows, rows_done);
}

}  // extern "C"
