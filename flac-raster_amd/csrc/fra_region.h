// fra_region.h -- the host scaffold of the units over a raster or a decoded region on the device: five reduce it
// (fra_decimate.hip, fra_resample.hip with its nodata-aware reads, fra_compare.hip, fra_stats.hip, fra_zonal.hip), two map it
// (fra_calc.hip and fra_focal.hip, whose output has a dtype, a size or a band count of its own: Dst, run_raster_to,
// run_region_to) and one transforms it as a whole (fra_proximity.hip, with two outputs of its own: stage_in, stage_out,
// run_region_src), as does the one that labels its connected components (fra_regions.hip, three outputs and a table);
// fra_warp.hip and fra_rasterize.hip use its staging.  Once each:
//   * the refusals they share: a bad dtype or raster layout (check_raster), items that do not cover the region
//     (check_cover), and what is left to the windowed read, which refuses it with its own message
//     (left_to_window_read, left_to_window_read_no_dst, refer_to_window_read);
//   * the dtype dispatch (with_dtype), the extent of a strided raster (extent_of) and the test for aligned 16-byte
//     row loads (aligned16);
//   * a call's stream and arena (Call: it lives in fra_host.h, where the device decoder finds it too), the staging
//     of host buffers (stage_in, stage_out, copy_back), the kernels' time between two events (timed), and the two
//     frames around a unit's kernels: a raster job (run_raster) and a region decoded by the windowed read
//     (fra_decode_device_window, called as any caller would: same kernels, refusals and messages) into a per-call
//     device buffer (decode; run_region_src without a destination, run_region_to and run_region with one).
//   * device code: the vector access and the conversion of a result the mapping units share (VecOf, to_out), and the
//     workgroup's sum of a count (wg_sum: the resampling, the warp, the proximity, the rasterizer).
// The scan of a raster in chunks of rows and slots, which four of the units share, is in fra_scan.h.
// Every function is inline: the units are separate translation units of one library and of one check program.
#pragma once
#include <algorithm>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"

namespace fra_region {

struct Strides { int64_t band, row, col; };  // in elements

// elements addressed from element 0 by a (channels, rows, cols) raster of the given strides
inline int64_t extent_of(int64_t channels, int64_t rows, int64_t cols, const Strides& s) {
  return (channels - 1) * s.band + (rows - 1) * s.row + (cols - 1) * s.col + 1;
}

// 16-byte row loads are aligned: column stride 1; base, row and band strides multiples of 16 bytes
inline bool aligned16(const void* p, const Strides& s, size_t es) {
  return s.col == 1 && ((uintptr_t)p % 16) == 0 && (((uint64_t)s.row * es) % 16) == 0 &&
         (((uint64_t)s.band * es) % 16) == 0;
}

// FRA_E_INVALID for a dtype outside fra_dtype, then for a (channels, h, w) raster without a pixel or a negative
// stride in either of two layouts (a unit with one layout passes it twice)
inline int check_raster(int dtype, int32_t channels, int32_t h, int32_t w, const Strides& a, const Strides& b) {
  if (dtype < FRA_U8 || dtype > FRA_F64) return fra_internal_set_error(FRA_E_INVALID, "bad dtype %d", dtype);
  if (channels < 1 || h < 1 || w < 1 || a.band < 0 || a.row < 0 || a.col < 0 || b.band < 0 || b.row < 0 || b.col < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d x %d x %d)", channels, h, w);
  return FRA_OK;
}

// f(T{}) for the element type T of a checked dtype
template <typename F>
inline void with_dtype(int dtype, F&& f) {
  switch (dtype) {
    case FRA_U8: f(uint8_t{}); break;
    case FRA_I8: f(int8_t{}); break;
    case FRA_U16: f(uint16_t{}); break;
    case FRA_I16: f(int16_t{}); break;
    case FRA_U32: f(uint32_t{}); break;
    case FRA_I32: f(int32_t{}); break;
    case FRA_F32: f(float{}); break;
    case FRA_F64: f(double{}); break;
  }
}

// a second, read-only raster of labels beside the values (fra_zonal.hip): the integer dtypes, and f(Z{}) for one
inline bool is_int_dtype(int dtype) { return dtype >= FRA_U8 && dtype <= FRA_I32; }
template <typename F>
inline void with_int_dtype(int dtype, F&& f) {
  switch (dtype) {
    case FRA_U8: f(uint8_t{}); break;
    case FRA_I8: f(int8_t{}); break;
    case FRA_U16: f(uint16_t{}); break;
    case FRA_I16: f(int16_t{}); break;
    case FRA_U32: f(uint32_t{}); break;
    case FRA_I32: f(int32_t{}); break;
  }
}

// FRA_E_INVALID unless the intersections of the items with roi add up to roi's area (the item windows and roi are
// non-negative: the caller has left everything else to the windowed read)
inline int check_cover(const fra_decode_job* job, const fra_window* roi) {
  const int64_t h = roi->height, w = roi->width;
  int64_t covered = 0;
  for (int i = 0; i < job->nitems; i++) {
    const fra_window& t = job->items[i].window;
    const int64_t ra = std::max<int64_t>(t.row_off, roi->row_off);
    const int64_t rb = std::min<int64_t>((int64_t)t.row_off + t.height, (int64_t)roi->row_off + h);
    const int64_t ca = std::max<int64_t>(t.col_off, roi->col_off);
    const int64_t cb = std::min<int64_t>((int64_t)t.col_off + t.width, (int64_t)roi->col_off + w);
    if (rb > ra && cb > ca) covered += (rb - ra) * (cb - ca);
  }
  if (covered != h * w)
    return fra_internal_set_error(FRA_E_INVALID, "the items do not cover the region (%lld of its %lld pixels)",
                                  (long long)covered, (long long)(h * w));
  return FRA_OK;
}

// a non-negative item window everywhere (what is not is the windowed read's to refuse)
inline bool item_windows_ok(const fra_decode_job* job) {
  for (int i = 0; i < job->nitems; i++) {
    const fra_window& w = job->items[i].window;
    if (w.height < 0 || w.width < 0 || w.row_off < 0 || w.col_off < 0) return false;
  }
  return true;
}

// What the windowed read refuses at once (before any GPU work, with its own message) is left to it: a unit that finds
// one of these refers the call to it (refer_to_window_read).  The part that does not depend on a destination ...
inline bool region_left_to_window_read(const fra_decode_job* job, const fra_window* roi) {
  return roi->height <= 0 || roi->width <= 0 || roi->row_off < 0 || roi->col_off < 0 || job->nitems < 0 ||
         (job->nitems && !job->items) || job->dst_dtype < FRA_U8 || job->dst_dtype > FRA_F64 || job->channels < 1 ||
         job->channels > 8 || (job->flags & FRA_DECODE_CONCAT) || !item_windows_ok(job);
}
// ... for a read into the job's destination (the decimated and resampled reads)
inline bool left_to_window_read(const fra_decode_job* job, const fra_window* roi) {
  return region_left_to_window_read(job, roi) || !job->dst || job->band_stride < 0 || job->row_stride < 0 ||
         job->col_stride < 0;
}
// ... and for a read that ignores the job's destination and strides (the comparison and the statistics)
inline bool left_to_window_read_no_dst(const fra_decode_job* job, const fra_window* roi) {
  return region_left_to_window_read(job, roi) || (!job->data && job->len) || job->denorm < FRA_DENORM_NONE ||
         job->denorm > FRA_DENORM_PCM16 ||
         (job->denorm == FRA_DENORM_NONE && job->dst_dtype != FRA_I16 && job->dst_dtype != FRA_I32);
}

// the windowed read's code for a call that was left to it, or "bad arguments"; `needs_dummy_dst`: the job's own dst
// and strides are ignored
inline int refer_to_window_read(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, fra_decoded* infos,
                                bool needs_dummy_dst) {
  fra_decode_job inner = *job;
  if (needs_dummy_dst) {
    inner.dst = (void*)infos;  // any non-null pointer: the call returns before it is looked at
    inner.dst_on_device = 1;
    inner.band_stride = 0, inner.row_stride = 0, inner.col_stride = 1;
  }
  const int rc = fra_decode_device_window(ctx, &inner, roi, infos);
  return rc ? rc : fra_internal_set_error(FRA_E_INVALID, "bad arguments");
}

#ifdef __HIPCC__
using ::Call;  // (fra_host.h)

// a host raster copied to the device from its element 0 to the last one addressed; a device raster as it is
inline int stage_in(Call& c, const void* p, int on_device, size_t bytes, const void** d) {
  *d = p;
  if (on_device) return FRA_OK;
  void* q = nullptr;
  HIPCHK(c.sc.alloc(&q, bytes));
  HIPCHK(hipMemcpyAsync(q, p, bytes, hipMemcpyHostToDevice, c.s));
  *d = q;
  return FRA_OK;
}

// A destination the kernels write through `dev`.  A host destination is staged whole, so that the elements between
// the outputs keep the caller's values, and copied back whole after the kernels.
struct StagedOut {
  void* dev = nullptr;
  void* host = nullptr;  // null: a device destination, nothing to copy back
  size_t bytes = 0;
};
inline int stage_out(Call& c, void* p, int on_device, size_t bytes, StagedOut* o) {
  *o = StagedOut{p, nullptr, bytes};
  if (on_device) return FRA_OK;
  o->host = p;
  HIPCHK(c.sc.alloc(&o->dev, bytes));
  HIPCHK(hipMemcpyAsync(o->dev, p, bytes, hipMemcpyHostToDevice, c.s));
  return FRA_OK;
}
inline int copy_back(Call& c, const StagedOut& o) {
  if (o.host) HIPCHK(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c.s));
  return FRA_OK;
}

// `enqueue` (the kernels) between two events of the call's arena, then `after` (the copies to the host), then the
// stream is waited for; *ms: the kernels' time.  Both return a code and enqueue only.
template <typename Enqueue, typename After>
inline int timed(Call& c, float* ms, Enqueue&& enqueue, After&& after) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(c.sc.event(&e0, hipEventDefault));
  HIPCHK(c.sc.event(&e1, hipEventDefault));
  HIPCHK(hipEventRecord(e0, c.s));
  if (const int rc = enqueue()) return rc;
  HIPCHK(hipEventRecord(e1, c.s));
  if (const int rc = after()) return rc;
  HIPCHK(hipStreamSynchronize(c.s));
  float t = 0.f;
  (void)hipEventElapsedTime(&t, e0, e1);
  *ms = t;
  return FRA_OK;
}

// roi at full resolution in job->dst_dtype into device memory of `sc`: band-planar, rows of *row_stride elements that
// start on 16-byte boundaries (for the vector loads of the kernel that follows), bands of roi->height rows.  The job's
// own dst and strides are not looked at.  Synchronous; the windowed read's scratch is gone on return.
inline int decode(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, fra_decoded* infos, HipArena& sc,
                  void** d_region, int64_t* row_stride) {
  const int64_t h = roi->height, w = roi->width;
  const size_t es = (size_t)elem_size(job->dst_dtype);
  const int64_t vlen = 16 / (int64_t)es;
  const int64_t rs = (w + vlen - 1) / vlen * vlen;
  HIPCHK(sc.alloc(d_region, (size_t)job->channels * (size_t)(h * rs) * es));
  fra_decode_job inner = *job;
  inner.dst = *d_region;
  inner.dst_on_device = 1;
  inner.band_stride = h * rs;
  inner.row_stride = rs;
  inner.col_stride = 1;
  *row_stride = rs;
  return fra_decode_device_window(ctx, &inner, roi, infos);
}

// a checked raster job: a (channels, h, w) source and a (channels, oh, ow) destination of one dtype
struct RasterJob {
  const void* src;
  int32_t src_on_device, dtype, channels, h, w;
  Strides ss;
  void* dst;
  int32_t dst_on_device, oh, ow;
  Strides ds;
};
// the fields fra_decimate_job and fra_resample_job share; the unit works out the output size
template <typename Job>
inline RasterJob raster_job(const Job& j) {
  return RasterJob{j.src, j.src_on_device, j.dtype, j.channels, j.height, j.width,
                   Strides{j.src_band_stride, j.src_row_stride, j.src_col_stride},
                   j.dst, j.dst_on_device, 0, 0, Strides{j.dst_band_stride, j.dst_row_stride, j.dst_col_stride}};
}
inline int check_raster(const RasterJob& j) { return check_raster(j.dtype, j.channels, j.h, j.w, j.ss, j.ds); }

// what a unit's kernels work on: a device source and a destination, with their strides
struct Io {
  const void* src;
  Strides ss;
  StagedOut out;
  Strides ds;
};

// a destination raster with a dtype and a band count of its own (a (channels, oh, ow) raster through its strides)
struct Dst {
  void* p;
  int32_t on_device, dtype, channels, oh, ow;
  Strides s;
};

// A (channels, h, w) source of `dtype` and a destination from the staging of their host buffers on: body(call, io)
// plans and runs the unit's kernels (timed) and copies the destination back (copy_back).
template <typename Body>
inline int run_raster_to(fra_ctx* ctx, const void* src, int32_t src_on_device, int32_t dtype, int32_t channels, int32_t h,
                         int32_t w, const Strides& ss, const Dst& d, Body&& body) {
  Call c(ctx);
  Io io{nullptr, ss, {}, d.s};
  if (const int rc = stage_in(c, src, src_on_device, (size_t)extent_of(channels, h, w, ss) * (size_t)elem_size(dtype), &io.src))
    return rc;
  if (const int rc = stage_out(c, d.p, d.on_device, (size_t)extent_of(d.channels, d.oh, d.ow, d.s) * (size_t)elem_size(d.dtype),
                               &io.out))
    return rc;
  return body(c, io);
}
// ... for a raster job, whose destination has the source's dtype and band count
template <typename Body>
inline int run_raster(fra_ctx* ctx, const RasterJob& j, Body&& body) {
  return run_raster_to(ctx, j.src, j.src_on_device, j.dtype, j.channels, j.h, j.w, j.ss,
                       Dst{j.dst, j.dst_on_device, j.dtype, j.channels, j.oh, j.ow, j.ds}, body);
}

// A region without a destination (the reducing units): decoded into a per-call buffer, body(call, d_region, strides).
template <typename Body>
inline int run_region_src(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, fra_decoded* infos, Body&& body) {
  Call c(ctx);
  void* d_region = nullptr;  // the region at full resolution: band-planar, in dst_dtype, rows on 16-byte boundaries
  int64_t rs = 0;
  if (const int rc = decode(ctx, job, roi, infos, c.sc, &d_region, &rs)) return rc;
  return body(c, (const void*)d_region, Strides{(int64_t)roi->height * rs, rs, 1});
}
// The same as run_raster_to for a region: the decoded region is the body's source.
template <typename Body>
inline int run_region_to(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, fra_decoded* infos, const Dst& d,
                         Body&& body) {
  return run_region_src(ctx, job, roi, infos, [&](Call& c, const void* d_region, const Strides& ss) -> int {
    Io io{d_region, ss, {}, d.s};
    if (const int rc = stage_out(c, d.p, d.on_device,
                                 (size_t)extent_of(d.channels, d.oh, d.ow, d.s) * (size_t)elem_size(d.dtype), &io.out))
      return rc;
    return body(c, io);
  });
}
// ... into the job's dst and strides, the (channels, oh, ow) destination in dst_dtype
template <typename Body>
inline int run_region(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, fra_decoded* infos, int32_t oh,
                      int32_t ow, Body&& body) {
  return run_region_to(ctx, job, roi, infos,
                       Dst{job->dst, job->dst_on_device, job->dst_dtype, job->channels, oh, ow,
                           {job->band_stride, job->row_stride, job->col_stride}},
                       body);
}

// Device code the mapping units (fra_calc.hip, fra_focal.hip) share: P neighbouring elements as one vector access,
// and the rule's conversion of an f64 result (include/flac_raster_amd.h, band math: Output).
template <typename T, int P>
struct alignas(sizeof(T) * P < 16 ? sizeof(T) * P : 16) VecOf { T v[P]; };

__device__ inline double sat(double x, double lo, double hi) { return x != x ? 0.0 : (x < lo ? lo : (x > hi ? hi : x)); }

template <typename D>
__device__ inline D to_out(double x) {
  if constexpr (std::is_floating_point<D>::value) {
    return (D)(x != x ? __longlong_as_double(0x7ff8000000000000ll) : x);
  } else {
    return (D)sat(rint(x), (double)std::numeric_limits<D>::lowest(), (double)std::numeric_limits<D>::max());
  }
}

// Device code every unit that counts per workgroup shares: the sum of `v` (a 32- or 64-bit unsigned) over the 256
// threads of a workgroup, to thread 0 alone (the others get 0).  Lane exchanges within each wave, four words of LDS,
// one barrier: every thread of the workgroup calls it, once per kernel.  What becomes of the total is the caller's.
template <typename S>
__device__ inline S wg_sum(S v) {
  static_assert(std::is_unsigned<S>::value && (sizeof(S) == 4 || sizeof(S) == 8), "a 32- or 64-bit count");
  using X = std::conditional_t<sizeof(S) == 4, int, long long>;  // what the lane exchange takes
  __shared__ S s_part[4];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (S)__shfl_xor((X)v, m, 64);
  if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  return threadIdx.x == 0 ? (S)(s_part[0] + s_part[1] + s_part[2] + s_part[3]) : (S)0;
}
#endif

}  // namespace fra_region
