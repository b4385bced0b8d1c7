// fra_decimate.hip -- decimated reads: a raster at 1/k resolution (fra_decimate), and a region of a set of tile
// streams decoded and decimated without the full-resolution region leaving the GPU (fra_decode_device_decimated).
//
// The rule (include/flac_raster_amd.h): the region h x w is cut into k x k blocks anchored at its origin (edge blocks
// are smaller, n = rows x columns pixels each); the output is ceil(h/k) x ceil(w/k).
//   nearest  out[R, C] = in[min(R k + k/2, h-1), min(C k + k/2, w-1)]
//   average  integer dtypes: S = exact sum of the block, out = rint((double)S / (double)n), half to even
//            float dtypes:   every element as f64; a block row is padded with +0.0 to k elements and summed by the
//                            adjacent-pair tree; the row sums are added top to bottom; out = (T)(acc / (double)n)
//
// k_decimate<T, 1>: a thread owns V = 16 / sizeof(T) consecutive elements of a source row (one 16-byte load when the
// layout allows, guarded scalar loads otherwise), a wave 64 V consecutive elements, a workgroup 256 V.  The pair tree
// runs over the thread's V values in registers for min(log2 k, log2 V) levels; when k > V the k / V lanes of a block
// finish it with __shfl_xor butterflies (lane l and l ^ 1, then l ^ 2, ...: exactly the adjacent-pair tree, f64
// addition being commutative); when k < V a thread holds V / k blocks.  The row loop then adds the row sums in order.
// Every source element is read once, nothing is shared between workgroups, there are no atomics.  A workgroup is one
// (band, block row, column segment); all indices are 64-bit.
// k_decimate<T, 0>: one thread per output element, one load each.
//
// fra_decode_device_decimated calls the windowed read (fra_decode_device_window) as any caller would, with a device
// buffer of the region as its destination: same kernels, same refusals, same messages.  fra_decode_dev.hip knows
// nothing of this unit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"

extern "C" void fra_internal_ctx_stream(fra_ctx* ctx, int* device, hipStream_t* stream);

namespace {

struct DecimArgs {
  const void* src;
  void* dst;
  int64_t sbs, srs, scs;  // source element strides: band, row, column
  int64_t dbs, drs, dcs;  // destination element strides
  int32_t h, w, oh, ow;
  int32_t k, logk;
  int32_t nseg;  // workgroups per block row (average) / per output row (nearest)
  int32_t vec;   // 16-byte row loads are aligned (scs == 1; base, row and band strides multiples of 16 bytes)
};

template <typename T>
struct AccOf { using type = std::conditional_t<std::is_floating_point<T>::value, double, long long>; };

template <typename A>
__device__ inline A lane_xor(A v, int m) {
  if constexpr (std::is_same<A, double>::value) return __shfl_xor(v, m, 64);
  else return (A)__shfl_xor((long long)v, m, 64);
}

template <typename T, int MODE>
__global__ void __launch_bounds__(256) k_decimate(DecimArgs a) {
  const T* __restrict__ src = (const T*)a.src;
  T* __restrict__ dst = (T*)a.dst;
  const uint32_t seg = blockIdx.x % (uint32_t)a.nseg;
  const uint32_t rest = blockIdx.x / (uint32_t)a.nseg;
  const int32_t R = (int32_t)(rest % (uint32_t)a.oh);
  const int64_t b = (int64_t)(rest / (uint32_t)a.oh);
  const int k = a.k;
  if constexpr (MODE == 0) {
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C >= a.ow) return;
    const int64_t r = min((int64_t)R * k + (k >> 1), (int64_t)a.h - 1);
    const int64_t c = min(C * k + (k >> 1), (int64_t)a.w - 1);
    dst[b * a.dbs + (int64_t)R * a.drs + C * a.dcs] = src[b * a.sbs + r * a.srs + c * a.scs];
  } else {
    using A = typename AccOf<T>::type;
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int LOGV = V == 16 ? 4 : (V == 8 ? 3 : (V == 4 ? 2 : 1));
    struct alignas(16) Vec { T v[V]; };
    const int logk = a.logk;
    const int64_t col0 = ((int64_t)seg * 256 + threadIdx.x) * V;  // first source column of this thread
    const int64_t row0 = (int64_t)R * k;
    const int rows = (int)min((int64_t)k, (int64_t)a.h - row0);
    const int64_t left = (int64_t)a.w - col0;  // columns from col0 to the row's end (<= 0: none; the lane still
                                               // takes part in the butterflies, with +0.0)
    const bool whole = a.vec && left >= V;
    const T* p = src + (b * a.sbs + row0 * a.srs + col0 * a.scs);
    constexpr int NOUT = V / 2;  // most blocks a thread holds (k = 2)
    A acc[NOUT];
    // this thread's V elements of one row; the columns past the row's end are +0.0
    auto load_row = [&](const T* q) {
      Vec v;
      if (whole) {
        v = *(const Vec*)q;
      } else {
#pragma unroll
        for (int i = 0; i < V; i++) v.v[i] = i < left ? q[(int64_t)i * a.scs] : (T)0;
      }
      return v;
    };
    Vec next = load_row(p);
    for (int r = 0; r < rows; r++) {
      const Vec cur = next;
      p += a.srs;
      if (r + 1 < rows) next = load_row(p);  // in flight while this row is summed
      A x[V];
#pragma unroll
      for (int i = 0; i < V; i++) x[i] = (A)cur.v[i];
      // the adjacent-pair tree inside the thread: min(logk, LOGV) levels
#pragma unroll
      for (int l = 0; l < LOGV; l++) {
        if (l < logk) {
#pragma unroll
          for (int i = 0; i < (V >> (l + 1)); i++) x[i] = x[2 * i] + x[2 * i + 1];
        }
      }
      // ... and across the k / V lanes of a block
      for (int l = LOGV; l < logk; l++) x[0] = x[0] + lane_xor<A>(x[0], 1 << (l - LOGV));
      // row sums, top to bottom
#pragma unroll
      for (int i = 0; i < NOUT; i++) acc[i] = r == 0 ? x[i] : acc[i] + x[i];
    }
    if (left <= 0) return;
    const int nout = logk < LOGV ? V >> logk : 1;  // blocks of this thread
    if (logk > LOGV && ((threadIdx.x & ((1u << (logk - LOGV)) - 1)) != 0)) return;  // a block's first lane stores
    const int64_t C0 = col0 >> logk;
#pragma unroll
    for (int i = 0; i < NOUT; i++) {
      const int64_t C = C0 + i;
      if (i < nout && C < a.ow) {
        const int64_t cols = min((int64_t)k, (int64_t)a.w - C * k);
        const double n = (double)((int64_t)rows * cols);
        T o;
        if constexpr (std::is_floating_point<T>::value) o = (T)(acc[i] / n);
        else o = (T)(long long)rint((double)acc[i] / n);
        dst[b * a.dbs + (int64_t)R * a.drs + C * a.dcs] = o;
      }
    }
  }
}

thread_local float g_decimate_ms = 0.f;

template <typename T>
void launch_t(int mode, unsigned grid, hipStream_t s, const DecimArgs& a) {
  if (mode == FRA_RESAMPLE_NEAREST) hipLaunchKernelGGL((k_decimate<T, 0>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_decimate<T, 1>), dim3(grid), dim3(256), 0, s, a);
}

int log2_factor(int k) {
  for (int l = 1; l <= 6; l++)
    if (k == (1 << l)) return l;
  return 0;
}

// k_decimate over device buffers between two events; enqueues only
int launch_decimate(int dtype, int mode, int channels, DecimArgs a, const void* d_src, void* d_dst, hipEvent_t e0,
                    hipEvent_t e1, hipStream_t s) {
  const size_t es = (size_t)elem_size(dtype);
  a.src = d_src;
  a.dst = d_dst;
  a.vec = a.scs == 1 && ((uintptr_t)d_src % 16) == 0 && (((uint64_t)a.srs * es) % 16) == 0 &&
          (((uint64_t)a.sbs * es) % 16) == 0;
  const int64_t per_row = mode == FRA_RESAMPLE_NEAREST ? a.ow : ((int64_t)a.w + (16 / (int64_t)es) - 1) / (16 / (int64_t)es);
  a.nseg = (int32_t)((per_row + 255) / 256);
  const int64_t grid = (int64_t)channels * a.oh * a.nseg;
  if (grid > INT32_MAX) return fra_internal_set_error(FRA_E_INVALID, "the raster is too large for one decimation");
  HIPCHK(hipEventRecord(e0, s));
  switch (dtype) {
    case FRA_U8: launch_t<uint8_t>(mode, (unsigned)grid, s, a); break;
    case FRA_I8: launch_t<int8_t>(mode, (unsigned)grid, s, a); break;
    case FRA_U16: launch_t<uint16_t>(mode, (unsigned)grid, s, a); break;
    case FRA_I16: launch_t<int16_t>(mode, (unsigned)grid, s, a); break;
    case FRA_U32: launch_t<uint32_t>(mode, (unsigned)grid, s, a); break;
    case FRA_I32: launch_t<int32_t>(mode, (unsigned)grid, s, a); break;
    case FRA_F32: launch_t<float>(mode, (unsigned)grid, s, a); break;
    case FRA_F64: launch_t<double>(mode, (unsigned)grid, s, a); break;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e1, s));
  return FRA_OK;
}

int check_factor(int32_t factor, int32_t resampling) {
  if (!log2_factor(factor))
    return fra_internal_set_error(FRA_E_INVALID, "the decimation factor must be 2, 4, 8, 16, 32 or 64 (got %d)", factor);
  if (resampling != FRA_RESAMPLE_NEAREST && resampling != FRA_RESAMPLE_AVERAGE)
    return fra_internal_set_error(FRA_E_INVALID, "unknown resampling %d (0 nearest, 1 average)", resampling);
  return FRA_OK;
}

// elements addressed from element 0 by a (channels, rows, cols) raster of the given strides
int64_t extent_of(int64_t channels, int64_t rows, int64_t cols, int64_t bs, int64_t rs, int64_t cs) {
  return (channels - 1) * bs + (rows - 1) * rs + (cols - 1) * cs + 1;
}

}  // namespace

extern "C" {

FRA_API int fra_decimate_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_decimate_ms;
  return FRA_OK;
}

FRA_API int fra_decimate(fra_ctx* ctx, const fra_decimate_job* job) {
  if (!ctx || !job || !job->src || !job->dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (const int rc = check_factor(job->factor, job->resampling)) return rc;
  if (job->dtype < FRA_U8 || job->dtype > FRA_F64) return fra_internal_set_error(FRA_E_INVALID, "bad dtype %d", job->dtype);
  if (job->channels < 1 || job->height < 1 || job->width < 1 || job->src_band_stride < 0 || job->src_row_stride < 0 ||
      job->src_col_stride < 0 || job->dst_band_stride < 0 || job->dst_row_stride < 0 || job->dst_col_stride < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d x %d x %d)", job->channels, job->height,
                                  job->width);
  const int k = job->factor;
  DecimArgs a{};
  a.sbs = job->src_band_stride, a.srs = job->src_row_stride, a.scs = job->src_col_stride;
  a.dbs = job->dst_band_stride, a.drs = job->dst_row_stride, a.dcs = job->dst_col_stride;
  a.h = job->height, a.w = job->width;
  a.oh = (int32_t)(((int64_t)a.h + k - 1) / k), a.ow = (int32_t)(((int64_t)a.w + k - 1) / k);
  a.k = k, a.logk = log2_factor(k);

  int device = 0;
  hipStream_t s = nullptr;
  fra_internal_ctx_stream(ctx, &device, &s);
  (void)hipSetDevice(device);
  HipArena sc;  // staging buffers and events of this call, released on every path
  const size_t es = (size_t)elem_size(job->dtype);
  const size_t src_bytes = (size_t)extent_of(job->channels, a.h, a.w, a.sbs, a.srs, a.scs) * es;
  const size_t dst_bytes = (size_t)extent_of(job->channels, a.oh, a.ow, a.dbs, a.drs, a.dcs) * es;
  const void* d_src = job->src;
  void* d_dst = job->dst;
  if (!job->src_on_device) {
    void* p = nullptr;
    HIPCHK(sc.alloc(&p, src_bytes));
    HIPCHK(hipMemcpyAsync(p, job->src, src_bytes, hipMemcpyHostToDevice, s));
    d_src = p;
  }
  if (!job->dst_on_device) {  // staged whole, so that the elements between the outputs keep the caller's values
    HIPCHK(sc.alloc(&d_dst, dst_bytes));
    HIPCHK(hipMemcpyAsync(d_dst, job->dst, dst_bytes, hipMemcpyHostToDevice, s));
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(sc.event(&e0, hipEventDefault));
  HIPCHK(sc.event(&e1, hipEventDefault));
  if (const int rc = launch_decimate(job->dtype, job->resampling, job->channels, a, d_src, d_dst, e0, e1, s)) return rc;
  if (!job->dst_on_device) HIPCHK(hipMemcpyAsync(job->dst, d_dst, dst_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  g_decimate_ms = ms;
  return FRA_OK;
}

FRA_API int fra_decode_device_decimated(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, int32_t factor,
                                        int32_t resampling, fra_decoded* infos) {
  if (!ctx || !job || !roi || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (const int rc = check_factor(factor, resampling)) return rc;
  // what the windowed read refuses at once is left to it (it does so before any GPU work, with its own message)
  const bool refer = roi->height <= 0 || roi->width <= 0 || roi->row_off < 0 || roi->col_off < 0 || job->nitems < 0 ||
                     (job->nitems && !job->items) || !job->dst || job->dst_dtype < FRA_U8 || job->dst_dtype > FRA_F64 ||
                     job->channels < 1 || job->channels > 8 || job->band_stride < 0 || job->row_stride < 0 ||
                     job->col_stride < 0 || (job->flags & FRA_DECODE_CONCAT) || !fra_region::item_windows_ok(job);
  if (refer) {
    const int rc = fra_decode_device_window(ctx, job, roi, infos);
    return rc ? rc : fra_internal_set_error(FRA_E_INVALID, "bad arguments");
  }
  const int64_t h = roi->height, w = roi->width;
  if (const int rc = fra_region::check_cover(job, roi)) return rc;

  int device = 0;
  hipStream_t s = nullptr;
  fra_internal_ctx_stream(ctx, &device, &s);
  (void)hipSetDevice(device);
  HipArena sc;  // the region buffer, the staged output and the events: released on every path
  void* d_region = nullptr;  // the region at full resolution: band-planar, in dst_dtype, rows on 16-byte boundaries
  int64_t rs = 0;
  if (const int rc = fra_region::decode(ctx, job, roi, infos, sc, &d_region, &rs)) return rc;

  const int k = factor;
  DecimArgs a{};
  const size_t es = (size_t)elem_size(job->dst_dtype);
  a.sbs = h * rs, a.srs = rs, a.scs = 1;
  a.dbs = job->band_stride, a.drs = job->row_stride, a.dcs = job->col_stride;
  a.h = (int32_t)h, a.w = (int32_t)w;
  a.oh = (int32_t)((h + k - 1) / k), a.ow = (int32_t)((w + k - 1) / k);
  a.k = k, a.logk = log2_factor(k);

  const size_t dst_bytes = (size_t)extent_of(job->channels, a.oh, a.ow, a.dbs, a.drs, a.dcs) * es;
  void* d_dst = job->dst;
  if (!job->dst_on_device) {
    HIPCHK(sc.alloc(&d_dst, dst_bytes));
    HIPCHK(hipMemcpyAsync(d_dst, job->dst, dst_bytes, hipMemcpyHostToDevice, s));
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(sc.event(&e0, hipEventDefault));
  HIPCHK(sc.event(&e1, hipEventDefault));
  if (const int rc = launch_decimate(job->dst_dtype, resampling, job->channels, a, d_region, d_dst, e0, e1, s)) return rc;
  if (!job->dst_on_device) HIPCHK(hipMemcpyAsync(job->dst, d_dst, dst_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  g_decimate_ms = ms;
  return FRA_OK;
}

}  // extern "C"
