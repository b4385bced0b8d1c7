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
// This unit holds the kernel, its launch and the order of its entries' refusals.  Shared: the host scaffold of the
// five region-reducing units (fra_region.h: the dtype and layout refusal, what is left to the windowed read, staging,
// the region decoded by fra_decode_device_window as any caller would, the timed launch), and with the resampling
// units AccOf, log2_factor and check_factor (fra_resample.h).  fra_decode_dev.hip knows nothing of this unit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"
#include "fra_resample.h"

namespace {

using namespace fra_region;
using fra_rs::AccOf;

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

// k_decimate by `factor` over `io`, timed, and the destination copied back (`r` holds the sizes)
int launch_decimate(Call& c, const Io& io, int dtype, int mode, int channels, const fra_rs::ResampleArgs& r, int factor) {
  const int64_t V = 16 / (int64_t)elem_size(dtype);
  DecimArgs a{};
  a.src = io.src, a.dst = io.out.dev;
  a.sbs = io.ss.band, a.srs = io.ss.row, a.scs = io.ss.col;
  a.dbs = io.ds.band, a.drs = io.ds.row, a.dcs = io.ds.col;
  a.h = r.h, a.w = r.w, a.oh = r.oh, a.ow = r.ow;
  a.k = factor, a.logk = fra_rs::log2_factor(factor);
  a.vec = aligned16(io.src, io.ss, (size_t)elem_size(dtype));
  const int64_t per_row = mode == FRA_RESAMPLE_NEAREST ? a.ow : ((int64_t)a.w + V - 1) / V;
  a.nseg = (int32_t)((per_row + 255) / 256);
  const int64_t grid = (int64_t)channels * a.oh * a.nseg;
  if (grid > INT32_MAX) return fra_internal_set_error(FRA_E_INVALID, "the raster is too large for one decimation");
  return timed(
      c, &g_decimate_ms,
      [&]() -> int {
        with_dtype(dtype, [&](auto t) { launch_t<decltype(t)>(mode, (unsigned)grid, c.s, a); });
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&] { return copy_back(c, io.out); });
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
  RasterJob r = raster_job(*job);
  fra_rs::ResampleArgs sizes{};
  if (const int rc = fra_rs::check_factor(r.h, r.w, job->factor, job->resampling, &sizes)) return rc;
  if (const int rc = check_raster(r)) return rc;
  r.oh = sizes.oh, r.ow = sizes.ow;
  return run_raster(ctx, r, [&](Call& c, const Io& io) {
    return launch_decimate(c, io, r.dtype, job->resampling, r.channels, sizes, job->factor);
  });
}

FRA_API int fra_decode_device_decimated(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, int32_t factor,
                                        int32_t resampling, fra_decoded* infos) {
  if (!ctx || !job || !roi || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  fra_rs::ResampleArgs sizes{};
  if (const int rc = fra_rs::check_factor(roi->height, roi->width, factor, resampling, &sizes)) return rc;
  if (left_to_window_read(job, roi)) return refer_to_window_read(ctx, job, roi, infos, false);
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region(ctx, job, roi, infos, sizes.oh, sizes.ow, [&](Call& c, const Io& io) {
    return launch_decimate(c, io, job->dst_dtype, resampling, job->channels, sizes, factor);
  });
}

}  // extern "C"
