// fra_resample.hip -- resampled reads: a raster at any output size (fra_resample), and a region of a set of tile
// streams decoded and resampled without the full-resolution region leaving the GPU (fra_decode_device_resampled).
//
// The rule (include/flac_raster_amd.h): each axis alone, g = gcd(w, ow), w' = w / g, ow' = ow / g; integer
// coordinates only; every f64 operation rounded on its own (the library is built with -ffp-contract=off).
//   centre   num = (2 C + 1) w' - ow', den = 2 ow', i0 = floor(num / den), t = (double)(num - i0 den) / (double)den
//   nearest  out[R, C] = in[min((2 R + 1) h' / (2 oh'), h - 1), min((2 C + 1) w' / (2 ow'), w - 1)]
//   bilinear taps i0, i0 + 1, weights [1 - t, t];  cubic  taps i0 - 1 .. i0 + 2, Catmull-Rom; tap indices clamped;
//            vertically first (top to bottom) for every tap column, then left to right; integers: rint, clamped
//   average  integer area weights vx_i, vy_j (units of 1 / ow', 1 / oh' of a source pixel), n = h' w';
//            integers: S exact in int64, rint((double)S / (double)n); floats: c_i = sum_j (double)vy_j x[j][i] top to
//            bottom, acc = sum_i (double)vx_i c_i left to right, (T)(acc / (double)n)
//
// k_resample<T, 0 | 2 | 3>: one thread per output element; a workgroup is 256 consecutive output columns of one
// output row of one band, so the row's taps and weights are wave-uniform and the column's are computed once per thread.
// k_resample<T, 1>: a workgroup is (band, output row, `per` consecutive output columns), `per` chosen by the host so
// that their source columns fit the workgroup's 256 V (V = 16 / sizeof(T)).  A thread owns V adjacent source columns
// (one 16-byte load per row when the layout allows, guarded element loads otherwise -- k_decimate's two paths) and
// accumulates them down the output row's source rows, four rows requested at once with the next four in flight; the column sums go to LDS
// once, and the threads that own an output sum their taps from there left to right.  When one output column spans more
// than 256 V source columns (per = 1) the workgroup walks its span in chunks of 256 V and thread 0 carries the sum.
// For 8- and 16-bit integers whose column sums fit 32 bits (h' 2^(8 itemsize) <= 2^31) the columns are accumulated with
// 24-bit multiplies in 32 bits (NARROW); the output's sum is 64-bit always.
// No atomics, nothing shared between workgroups; all indices are 64-bit.
//
// This unit holds the kernel and its launch.  Shared with fra_resample_masked.hip (fra_resample.h): the kernel's
// arguments, udiv, centre, tap_weights, from_f64, the refusals of the sizes and the grid of a launch; with all five
// region-reducing units (fra_region.h): the dtype and layout refusal, what is left to the windowed read, staging, the
// decoded region and the timed launch.
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
using namespace fra_rs;

template <typename T, int MODE, bool NARROW = false>
__global__ void __launch_bounds__(256) k_resample(ResampleArgs a) {
  const T* __restrict__ src = (const T*)a.src;
  T* __restrict__ dst = (T*)a.dst;
  const uint32_t seg = blockIdx.x % (uint32_t)a.nseg;
  const uint32_t rest = blockIdx.x / (uint32_t)a.nseg;
  const int64_t R = (int64_t)(rest % (uint32_t)a.oh);
  const int64_t b = (int64_t)(rest / (uint32_t)a.oh);
  const int64_t h = a.h, w = a.w;
  if constexpr (MODE == FRA_RESAMPLE_NEAREST) {
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C >= a.ow) return;
    const int64_t r = min(udiv((2 * R + 1) * a.hr, 2 * a.ohr), h - 1);
    const int64_t c = min(udiv((2 * C + 1) * a.wr, 2 * a.owr), w - 1);
    dst[b * a.dbs + R * a.drs + C * a.dcs] = src[b * a.sbs + r * a.srs + c * a.scs];
  } else if constexpr (MODE == FRA_RESAMPLE_BILINEAR || MODE == FRA_RESAMPLE_CUBIC) {
    constexpr int NT = MODE == FRA_RESAMPLE_BILINEAR ? 2 : 4;
    constexpr int OFF = MODE == FRA_RESAMPLE_BILINEAR ? 0 : -1;
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C >= a.ow) return;
    int64_t i0y, i0x;
    double ty, tx, wy[NT], wx[NT];
    centre(R, a.hr, a.ohr, &i0y, &ty);  // wave-uniform
    centre(C, a.wr, a.owr, &i0x, &tx);
    tap_weights<MODE>(ty, wy);
    tap_weights<MODE>(tx, wx);
    const T* rows[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) rows[j] = src + (b * a.sbs + min(max(i0y + OFF + j, (int64_t)0), h - 1) * a.srs);
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < NT; i++) {
      const int64_t co = min(max(i0x + OFF + i, (int64_t)0), w - 1) * a.scs;
      double c = (double)rows[0][co] * wy[0];  // vertically, top to bottom
#pragma unroll
      for (int j = 1; j < NT; j++) c = c + (double)rows[j][co] * wy[j];
      v = i == 0 ? c * wx[0] : v + c * wx[i];  // then left to right
    }
    dst[b * a.dbs + R * a.drs + C * a.dcs] = from_f64<T>(v);
  } else {
    using A = typename AccOf<T>::type;                  // an output's sum, as the rule has it
    using CA = std::conditional_t<NARROW, int32_t, A>;  // a column's sum (NARROW: it fits 32 bits, says the host)
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int64_t SPAN = 256 * V;  // source columns of a workgroup per chunk
    constexpr int G = 4;               // source rows requested at once by 16-byte loads
    struct alignas(16) Vec { T v[V]; };
    __shared__ CA cs[V * 256];  // column sums, element i of thread t at [i * 256 + t] (conflict-free stores)
    const int tid = (int)threadIdx.x;
    const int64_t Ca = (int64_t)seg * a.per, Cb = min(Ca + (int64_t)a.per, (int64_t)a.ow);
    // the workgroup's source columns [c_lo, c_hi), walked from a multiple of V so that the vector loads stay aligned
    const int64_t c_lo = udiv(Ca * a.wr, a.owr) / V * V;
    const int64_t c_hi = min(udiv(Cb * a.wr + a.owr - 1, a.owr), w);
    // the output row's source rows [j_lo, j_hi)
    const int64_t j_lo = udiv(R * a.hr, a.ohr);
    const int64_t j_hi = min(udiv((R + 1) * a.hr + a.ohr - 1, a.ohr), h);
    const int64_t y_lo = R * a.hr, y_hi = (R + 1) * a.hr;
    const double n = (double)(a.hr * a.wr);
    A run = 0;  // the running sum of a thread's output (carried over the chunks when per == 1)
    for (int64_t base = c_lo; base < c_hi; base += SPAN) {
      const int64_t col0 = base + (int64_t)tid * V;  // first source column of this thread
      const int64_t left = col0 < c_hi ? w - col0 : 0;  // columns from col0 to the row's end; 0 past the span's end
      const bool whole = a.vec && left >= V;
      const T* p = src + (b * a.sbs + j_lo * a.srs + col0 * a.scs);
      CA acc[V];
      // the thread's columns down the rows [j_lo, j_hi), top to bottom: GR rows are requested at once and the next GR
      // are in flight while these are added; a row's V elements stay packed in four registers until then
      auto down = [&](auto gr, auto load_row) {
        constexpr int GR = decltype(gr)::value;
        uint4 next[GR];
#pragma unroll
        for (int g = 0; g < GR; g++) next[g] = j_lo + g < j_hi ? load_row(p + g * a.srs) : uint4{};
        int64_t edge = j_lo * a.ohr;  // where source row j begins, in units of 1 / oh' of a source row
        for (int64_t j0 = j_lo; j0 < j_hi; j0 += GR) {
          uint4 cur[GR];
#pragma unroll
          for (int g = 0; g < GR; g++) cur[g] = next[g];
          p += GR * a.srs;
#pragma unroll
          for (int g = 0; g < GR; g++)
            if (j0 + GR + g < j_hi) next[g] = load_row(p + g * a.srs);
#pragma unroll
          for (int g = 0; g < GR; g++) {
            if (j0 + g < j_hi) {
              const int64_t top = max(edge, y_lo);
              edge += a.ohr;
              const int64_t vy = min(edge, y_hi) - top;  // wave-uniform, 1 .. min(h', oh')
              Vec x;
              __builtin_memcpy(&x, &cur[g], 16);
#pragma unroll
              for (int i = 0; i < V; i++) {
                CA term;
                if constexpr (NARROW) term = __mul24((int)vy, (int)x.v[i]);  // both within 24 bits
                else term = (CA)vy * (CA)x.v[i];
                acc[i] = (g == 0 && j0 == j_lo) ? term : acc[i] + term;
              }
            }
          }
        }
      };
      if (whole) {
        down(std::integral_constant<int, G>{}, [](const T* q) { return *(const uint4*)q; });
      } else {  // the row's end, or a layout without aligned rows: element by element, one row ahead
        down(std::integral_constant<int, 1>{}, [&](const T* q) {
          Vec v;
#pragma unroll
          for (int i = 0; i < V; i++) v.v[i] = i < left ? q[(int64_t)i * a.scs] : (T)0;
          uint4 r;
          __builtin_memcpy(&r, &v, 16);
          return r;
        });
      }
      if (base != c_lo) __syncthreads();  // the previous chunk's sums have been read
#pragma unroll
      for (int i = 0; i < V; i++) cs[i * 256 + tid] = acc[i];
      __syncthreads();
      const int64_t lim = min(base + SPAN, c_hi);
      for (int64_t C = Ca + tid; C < Cb; C += 256) {
        const int64_t x_lo = C * a.wr, x_hi = (C + 1) * a.wr;
        const int64_t t_lo = udiv(x_lo, a.owr), t_hi = min(udiv(x_hi + a.owr - 1, a.owr), w);  // the output's taps
        const bool first = t_lo >= base;  // the output starts in this chunk
        A s = first ? (A)0 : run;
        const int64_t i_lo = max(t_lo, base), i_hi = min(t_hi, lim);
        int64_t xe = i_lo * a.owr;  // where source column i begins, in units of 1 / ow' of a source column
        for (int64_t i = i_lo; i < i_hi; i++) {
          const int64_t lft = max(xe, x_lo);
          xe += a.owr;
          const A vx = (A)(min(xe, x_hi) - lft);
          const uint32_t rel = (uint32_t)(i - base);
          const A term = vx * (A)cs[(rel % V) * 256 + rel / V];
          s = (first && i == t_lo) ? term : s + term;
        }
        run = s;
        if (t_hi <= lim) {
          T o;
          if constexpr (std::is_floating_point<T>::value) o = (T)(s / n);
          else o = (T)(long long)rint((double)s / n);
          dst[b * a.dbs + R * a.drs + C * a.dcs] = o;
        }
      }
    }
  }
}

thread_local float g_resample_ms = 0.f;

template <typename T>
void launch_t(int mode, unsigned grid, hipStream_t s, const ResampleArgs& a) {
  switch (mode) {
    case FRA_RESAMPLE_NEAREST: hipLaunchKernelGGL((k_resample<T, 0>), dim3(grid), dim3(256), 0, s, a); break;
    case FRA_RESAMPLE_AVERAGE:
      if constexpr (std::is_integral<T>::value && sizeof(T) <= 2) {
        if (a.narrow) {
          hipLaunchKernelGGL((k_resample<T, 1, true>), dim3(grid), dim3(256), 0, s, a);
          break;
        }
      }
      hipLaunchKernelGGL((k_resample<T, 1>), dim3(grid), dim3(256), 0, s, a);
      break;
    case FRA_RESAMPLE_BILINEAR: hipLaunchKernelGGL((k_resample<T, 2>), dim3(grid), dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((k_resample<T, 3>), dim3(grid), dim3(256), 0, s, a); break;
  }
}

// k_resample over `io`, timed, and the destination copied back (`a` holds the sizes)
int launch_resample(Call& c, const Io& io, int dtype, int mode, int channels, ResampleArgs a) {
  unsigned grid = 0;
  if (const int rc = plan_grid(&a, io, dtype, channels, &mode, true, false, &grid)) return rc;
  return timed(
      c, &g_resample_ms,
      [&]() -> int {
        with_dtype(dtype, [&](auto t) { launch_t<decltype(t)>(mode, grid, c.s, a); });
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&] { return copy_back(c, io.out); });
}

}  // namespace

extern "C" {

FRA_API int fra_resample_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_resample_ms;
  return FRA_OK;
}

FRA_API int fra_resample(fra_ctx* ctx, const fra_resample_job* job) {
  if (!ctx || !job || !job->src || !job->dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  RasterJob r = raster_job(*job);
  if (const int rc = check_raster(r)) return rc;
  ResampleArgs a{};
  if (const int rc = check_sizes(r.h, r.w, job->out_height, job->out_width, job->resampling, r.dtype, &a)) return rc;
  r.oh = a.oh, r.ow = a.ow;
  return run_raster(ctx, r, [&](Call& c, const Io& io) {
    return launch_resample(c, io, r.dtype, job->resampling, r.channels, a);
  });
}

FRA_API int fra_decode_device_resampled(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                        int32_t out_height, int32_t out_width, int32_t resampling, fra_decoded* infos) {
  if (!ctx || !job || !roi || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  ResampleArgs a{};
  if (left_to_window_read(job, roi)) {
    if (const int rc = check_sizes(1, 1, out_height, out_width, resampling, FRA_U8, &a)) return rc;
    return refer_to_window_read(ctx, job, roi, infos, false);
  }
  if (const int rc = check_sizes(roi->height, roi->width, out_height, out_width, resampling, job->dst_dtype, &a)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region(ctx, job, roi, infos, a.oh, a.ow, [&](Call& c, const Io& io) {
    return launch_resample(c, io, job->dst_dtype, resampling, job->channels, a);
  });
}

}  // extern "C"
