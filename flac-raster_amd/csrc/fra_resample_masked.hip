// fra_resample_masked.hip -- nodata-aware resampled and decimated reads: fra_resample_masked, fra_decimate_masked and
// the two reads behind the decoder (fra_decode_device_resampled_masked, fra_decode_device_decimated_masked).
//
// The rule (include/flac_raster_amd.h, "Nodata-aware reads"): coordinates, taps and weights are those of the unmasked
// resampling; a pixel x is invalid when (double)x == nd or, in a float dtype, when it is NaN; the fill is (T)nd.
//   average  down the rows c_i = sum of vy_j x[j][i] over the valid pixels (floats: the first valid term initialises)
//            and u_i = sum of vy_j over them; left to right over the columns with u_i > 0  S = sum vx_i c_i,
//            W = sum vx_i u_i; W == 0 gives the fill, else rint((double)S / (double)W) or (T)(acc / (double)W)
//   bilinear, cubic  all taps valid: the unmasked formula; else the masked bilinear of the same centre
//   nearest  picks its pixel, invalid or not
// The decimation by k is the same arithmetic with h' = w' = k and oh' = ow' = 1 (every weight 1, the tap ranges clipped
// at the raster's edge): only the reduced sizes the host hands over differ.
//
// k_resample_masked<T, 1> has the shape of k_resample<T, 1> (fra_resample.hip): a workgroup is (band, output row, `per`
// output columns), a thread owns V = 16 / sizeof(T) adjacent source columns (16-byte row loads when the layout allows,
// guarded element loads otherwise), four rows are requested at once with the next four in flight, the column sums go
// to LDS once and each output's taps are summed left to right from there.  New: the valid weight u_i travels beside
// c_i, in registers (32 bits: u_i <= h' <= 2^31; NARROW: 16) and in LDS; the compare's constant is wave-uniform.  When one output
// spans more than 256 V source columns the workgroup walks its span in chunks and the thread carries S and W.
// NARROW (8- and 16-bit integers with h' 2^(8 itemsize) <= 2^31 and h' < 2^16): c_i in 32 bits, u_i in 16 bits.
// k_resample_masked<T, 0 | 2 | 3>: one thread per output element.
// The count of fill outputs per band (optional): summed within each wave by lane exchanges, then one atomicAdd per
// workgroup into a zeroed array of `channels` 64-bit words; no atomic in a loop.  All indices are 64-bit.
//
// This unit holds the kernel and its launch with the fill counts.  Shared with fra_resample.hip (fra_resample.h): the
// nodata refusal (check_nodata, which fra_warp.hip takes too); MaskedArgs is ResampleArgs and two fields; udiv, centre,
// tap_weights, from_f64, the refusals of the sizes and of a factor, the grid of a launch (NARROW with the extra
// h' < 2^16 here only); with all five region-reducing units (fra_region.h): the dtype and layout refusal, what is left to the windowed read, staging, the
// decoded region and the timed launch.
#include <hip/hip_runtime.h>

#include <cfloat>
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

// (double)x == nd (nd = (T)nodata is exact, says the host; a NaN nd equals nothing), or a NaN pixel
template <typename T>
__device__ inline bool invalid(T x, T nd) {
  if constexpr (std::is_floating_point<T>::value) return x == nd || x != x;
  else return x == nd;
}

// The workgroup's count of fill outputs into its band's word: every thread calls it with its own count.
__device__ inline void count_fill(unsigned long long* filled, int64_t b, uint32_t mine) {
  if (!filled) return;  // uniform
  __shared__ uint32_t wave_sum[4];
  uint32_t v = mine;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long total = (unsigned long long)wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    if (total) atomicAdd(&filled[b], total);
  }
}

// (the NARROW average of 8-bit integers is held to 3 waves per SIMD, what k_resample<T, 1, true> reaches: left alone
// it comes out one register over)
template <typename T, int MODE, bool NARROW = false>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(MODE == 1 && NARROW && sizeof(T) == 1 ? 3 : 1))) k_resample_masked(MaskedArgs a) {
  const T* __restrict__ src = (const T*)a.src;
  T* __restrict__ dst = (T*)a.dst;
  const uint32_t seg = blockIdx.x % (uint32_t)a.nseg;
  const uint32_t rest = blockIdx.x / (uint32_t)a.nseg;
  const int64_t R = (int64_t)(rest % (uint32_t)a.oh);
  const int64_t b = (int64_t)(rest / (uint32_t)a.oh);
  const int64_t h = a.h, w = a.w;
  const T nd = (T)a.nodata;  // the compare's constant and the fill
  uint32_t nfill = 0;        // this thread's outputs that no valid pixel reached
  if constexpr (MODE == FRA_RESAMPLE_NEAREST) {
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C < a.ow) {
      const int64_t r = min(udiv((2 * R + 1) * a.hr, 2 * a.ohr), h - 1);
      const int64_t c = min(udiv((2 * C + 1) * a.wr, 2 * a.owr), w - 1);
      const T x = src[b * a.sbs + r * a.srs + c * a.scs];
      dst[b * a.dbs + R * a.drs + C * a.dcs] = x;
      nfill = invalid(x, nd) ? 1u : 0u;
    }
  } else if constexpr (MODE == FRA_RESAMPLE_BILINEAR || MODE == FRA_RESAMPLE_CUBIC) {
    constexpr int NT = MODE == FRA_RESAMPLE_BILINEAR ? 2 : 4;
    constexpr int OFF = MODE == FRA_RESAMPLE_BILINEAR ? 0 : -1;
    constexpr int M = -OFF;  // where the bilinear taps i0, i0 + 1 lie among the NT
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C < a.ow) {
      int64_t i0y, i0x;
      double ty, tx;
      centre(R, a.hr, a.ohr, &i0y, &ty);  // wave-uniform
      centre(C, a.wr, a.owr, &i0x, &tx);
      T x[NT][NT];  // [j][i]: tap row j, tap column i
      bool all = true;
#pragma unroll
      for (int j = 0; j < NT; j++) {
        const T* row = src + (b * a.sbs + min(max(i0y + OFF + j, (int64_t)0), h - 1) * a.srs);
#pragma unroll
        for (int i = 0; i < NT; i++) {
          x[j][i] = row[min(max(i0x + OFF + i, (int64_t)0), w - 1) * a.scs];
          all = all && !invalid(x[j][i], nd);
        }
      }
      T o;
      if (all) {  // the unmasked formula
        double wy[NT], wx[NT];
        if constexpr (MODE == FRA_RESAMPLE_BILINEAR) {
          wy[0] = 1.0 - ty, wy[1] = ty, wx[0] = 1.0 - tx, wx[1] = tx;
        } else {
          tap_weights<FRA_RESAMPLE_CUBIC>(ty, wy);
          tap_weights<FRA_RESAMPLE_CUBIC>(tx, wx);
        }
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < NT; i++) {
          double c = (double)x[0][i] * wy[0];  // vertically, top to bottom
#pragma unroll
          for (int j = 1; j < NT; j++) c = c + (double)x[j][i] * wy[j];
          v = i == 0 ? c * wx[0] : v + c * wx[i];  // then left to right
        }
        o = from_f64<T>(v);
      } else {  // the masked bilinear of the same centre
        const double wy[2] = {1.0 - ty, ty}, wx[2] = {1.0 - tx, tx};
        double v = 0.0, wt = 0.0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < 2; i++) {
          double c = 0.0, u = 0.0;
          bool have = false;
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const T xv = x[M + j][M + i];
            if (!invalid(xv, nd)) {
              const double term = (double)xv * wy[j];
              c = have ? c + term : term;
              u = have ? u + wy[j] : wy[j];
              have = true;
            }
          }
          if (have) {
            const double cv = c * wx[i], cu = u * wx[i];
            v = any ? v + cv : cv;
            wt = any ? wt + cu : cu;
            any = true;
          }
        }
        if (!any || wt <= 0.0) {
          o = nd;
          nfill = 1;
        } else {
          o = from_f64<T>(v / wt);
        }
      }
      dst[b * a.dbs + R * a.drs + C * a.dcs] = o;
    }
  } else {
    using A = typename AccOf<T>::type;                  // an output's sum, as the rule has it
    using CA = std::conditional_t<NARROW, int32_t, A>;  // a column's sum (NARROW: it fits 32 bits, says the host)
    using UA = std::conditional_t<NARROW, uint16_t, uint32_t>;  // a column's valid weight in LDS
    constexpr bool FLT = std::is_floating_point<T>::value;
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int64_t SPAN = 256 * V;  // source columns of a workgroup per chunk
    constexpr int G = 4;               // source rows requested at once by 16-byte loads
    struct alignas(16) Vec { T v[V]; };
    struct Col { CA c; UA u; };  // a column's sum and its valid weight, read together by the taps
    __shared__ Col cols[V * 256];  // element i of thread t at [i * 256 + t] (conflict-free stores)
    const int tid = (int)threadIdx.x;
    const int64_t Ca = (int64_t)seg * a.per, Cb = min(Ca + (int64_t)a.per, (int64_t)a.ow);
    // the workgroup's source columns [c_lo, c_hi), walked from a multiple of V so that the vector loads stay aligned
    const int64_t c_lo = udiv(Ca * a.wr, a.owr) / V * V;
    const int64_t c_hi = min(udiv(Cb * a.wr + a.owr - 1, a.owr), w);
    // the output row's source rows [j_lo, j_hi)
    const int64_t j_lo = udiv(R * a.hr, a.ohr);
    const int64_t j_hi = min(udiv((R + 1) * a.hr + a.ohr - 1, a.ohr), h);
    const int64_t y_lo = R * a.hr, y_hi = (R + 1) * a.hr;
    A run = 0;         // the running S of a thread's output (carried over the chunks when per == 1)
    int64_t run_w = 0;  // ... and its W
    for (int64_t base = c_lo; base < c_hi; base += SPAN) {
      const int64_t col0 = base + (int64_t)tid * V;  // first source column of this thread
      const int64_t left = col0 < c_hi ? w - col0 : 0;  // columns from col0 to the row's end; 0 past the span's end
      const bool whole = a.vec && left >= V;
      const T* p = src + (b * a.sbs + j_lo * a.srs + col0 * a.scs);
      CA acc[V];
      constexpr int UP = NARROW ? 2 : 1;  // NARROW: two columns' valid weights (< 2^16 each) share a register
      uint32_t u[V / UP];
#pragma unroll
      for (int i = 0; i < V; i++) acc[i] = 0, u[i / UP] = 0;
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
                const bool ok = !invalid(x.v[i], nd);
                if constexpr (FLT) {
                  const CA term = (CA)vy * (CA)x.v[i];
                  acc[i] = ok ? (u[i] == 0 ? term : acc[i] + term) : acc[i];  // the first valid term initialises
                  u[i] += ok ? (uint32_t)vy : 0u;
                } else {  // an invalid pixel weighs 0 in both sums
                  const int m = ok ? (int)vy : 0;
                  if constexpr (NARROW) acc[i] += __mul24(m, (int)x.v[i]);  // both within 24 bits
                  else acc[i] += (CA)m * (CA)x.v[i];
                  u[i / UP] += (uint32_t)m << (16 * (i % UP));
                }
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
      for (int i = 0; i < V; i++) cols[i * 256 + tid] = Col{acc[i], (UA)(u[i / UP] >> (16 * (i % UP)))};
      __syncthreads();
      const int64_t lim = min(base + SPAN, c_hi);
      for (int64_t C = Ca + tid; C < Cb; C += 256) {
        const int64_t x_lo = C * a.wr, x_hi = (C + 1) * a.wr;
        const int64_t t_lo = udiv(x_lo, a.owr), t_hi = min(udiv(x_hi + a.owr - 1, a.owr), w);  // the output's taps
        const bool first = t_lo >= base;  // the output starts in this chunk
        A s = first ? (A)0 : run;
        int64_t wsum = first ? 0 : run_w;
        const int64_t i_lo = max(t_lo, base), i_hi = min(t_hi, lim);
        int64_t xe = i_lo * a.owr;  // where source column i begins, in units of 1 / ow' of a source column
        for (int64_t i = i_lo; i < i_hi; i++) {
          const int64_t lft = max(xe, x_lo);
          xe += a.owr;
          const int64_t vx = min(xe, x_hi) - lft;
          const uint32_t rel = (uint32_t)(i - base);
          const Col col = cols[(rel % V) * 256 + rel / V];
          const int64_t ui = (int64_t)col.u;
          if constexpr (FLT) {
            if (ui != 0) {  // a column without a valid pixel is skipped; the first other one initialises
              const A term = (A)vx * col.c;
              s = wsum == 0 ? term : s + term;
              wsum += vx * ui;
            }
          } else {  // (such a column's sum and weight are 0: adding them skips it)
            s += (A)vx * (A)col.c;
            wsum += vx * ui;
          }
        }
        run = s;
        run_w = wsum;
        if (t_hi <= lim) {
          T o;
          if (wsum == 0) {
            o = nd;
            nfill++;
          } else if constexpr (FLT) {
            o = (T)(s / (double)wsum);
          } else {
            o = (T)(long long)rint((double)s / (double)wsum);
          }
          dst[b * a.dbs + R * a.drs + C * a.dcs] = o;
        }
      }
    }
  }
  count_fill(a.filled, b, nfill);
}

thread_local float g_masked_ms = 0.f;

template <typename T>
void launch_t(int mode, unsigned grid, hipStream_t s, const MaskedArgs& a) {
  switch (mode) {
    case FRA_RESAMPLE_NEAREST: hipLaunchKernelGGL((k_resample_masked<T, 0>), dim3(grid), dim3(256), 0, s, a); break;
    case FRA_RESAMPLE_AVERAGE:
      if constexpr (std::is_integral<T>::value && sizeof(T) <= 2) {
        if (a.narrow) {
          hipLaunchKernelGGL((k_resample_masked<T, 1, true>), dim3(grid), dim3(256), 0, s, a);
          break;
        }
      }
      hipLaunchKernelGGL((k_resample_masked<T, 1>), dim3(grid), dim3(256), 0, s, a);
      break;
    case FRA_RESAMPLE_BILINEAR: hipLaunchKernelGGL((k_resample_masked<T, 2>), dim3(grid), dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((k_resample_masked<T, 3>), dim3(grid), dim3(256), 0, s, a); break;
  }
}

// k_resample_masked over `io`, timed, the fill counts into `filled` (host, channels words; may be null) and the
// destination copied back (`a` holds the sizes; `same_size_copies`: fra_resample.h, plan_grid)
int launch_masked(Call& c, const Io& io, int dtype, int mode, int channels, MaskedArgs a, bool same_size_copies,
                  double nodata, uint64_t* filled) {
  unsigned grid = 0;
  if (const int rc = plan_grid(&a, io, dtype, channels, &mode, same_size_copies, true, &grid)) return rc;
  const size_t filled_bytes = (size_t)channels * sizeof(unsigned long long);
  a.nodata = nodata;
  a.filled = nullptr;
  if (filled) {
    HIPCHK(c.sc.alloc(&a.filled, filled_bytes));
    HIPCHK(hipMemsetAsync(a.filled, 0, filled_bytes, c.s));
  }
  return timed(
      c, &g_masked_ms,
      [&]() -> int {
        with_dtype(dtype, [&](auto t) { launch_t<decltype(t)>(mode, grid, c.s, a); });
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&]() -> int {
        if (filled) HIPCHK(hipMemcpyAsync(filled, a.filled, filled_bytes, hipMemcpyDeviceToHost, c.s));
        return copy_back(c, io.out);
      });
}

}  // namespace

extern "C" {

FRA_API int fra_resample_masked_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_masked_ms;
  return FRA_OK;
}

FRA_API int fra_resample_masked(fra_ctx* ctx, const fra_resample_job* job, double nodata, uint64_t* filled) {
  if (!ctx || !job || !job->src || !job->dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  RasterJob r = raster_job(*job);
  if (const int rc = check_raster(r)) return rc;
  MaskedArgs a{};
  if (const int rc = check_sizes(r.h, r.w, job->out_height, job->out_width, job->resampling, r.dtype, &a)) return rc;
  if (const int rc = check_nodata(nodata, r.dtype)) return rc;
  r.oh = a.oh, r.ow = a.ow;
  return run_raster(ctx, r, [&](Call& c, const Io& io) {
    return launch_masked(c, io, r.dtype, job->resampling, r.channels, a, true, nodata, filled);
  });
}

FRA_API int fra_decimate_masked(fra_ctx* ctx, const fra_decimate_job* job, double nodata, uint64_t* filled) {
  if (!ctx || !job || !job->src || !job->dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  RasterJob r = raster_job(*job);
  MaskedArgs a{};
  if (const int rc = check_factor(r.h, r.w, job->factor, job->resampling, &a)) return rc;
  if (const int rc = check_raster(r)) return rc;
  if (const int rc = check_nodata(nodata, r.dtype)) return rc;
  r.oh = a.oh, r.ow = a.ow;
  return run_raster(ctx, r, [&](Call& c, const Io& io) {
    return launch_masked(c, io, r.dtype, job->resampling, r.channels, a, false, nodata, filled);
  });
}

FRA_API int fra_decode_device_resampled_masked(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                               int32_t out_height, int32_t out_width, int32_t resampling,
                                               fra_decoded* infos, double nodata, uint64_t* filled) {
  if (!ctx || !job || !roi || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  MaskedArgs a{};
  if (left_to_window_read(job, roi)) {
    if (const int rc = check_sizes(1, 1, out_height, out_width, resampling, FRA_U8, &a)) return rc;
    return refer_to_window_read(ctx, job, roi, infos, false);
  }
  if (const int rc = check_sizes(roi->height, roi->width, out_height, out_width, resampling, job->dst_dtype, &a)) return rc;
  if (const int rc = check_nodata(nodata, job->dst_dtype)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region(ctx, job, roi, infos, a.oh, a.ow, [&](Call& c, const Io& io) {
    return launch_masked(c, io, job->dst_dtype, resampling, job->channels, a, true, nodata, filled);
  });
}

FRA_API int fra_decode_device_decimated_masked(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                               int32_t factor, int32_t resampling, fra_decoded* infos, double nodata,
                                               uint64_t* filled) {
  if (!ctx || !job || !roi || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  MaskedArgs a{};
  if (const int rc = check_factor(roi->height, roi->width, factor, resampling, &a)) return rc;
  if (left_to_window_read(job, roi)) return refer_to_window_read(ctx, job, roi, infos, false);
  if (const int rc = check_nodata(nodata, job->dst_dtype)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region(ctx, job, roi, infos, a.oh, a.ow, [&](Call& c, const Io& io) {
    return launch_masked(c, io, job->dst_dtype, resampling, job->channels, a, false, nodata, filled);
  });
}

}  // extern "C"
