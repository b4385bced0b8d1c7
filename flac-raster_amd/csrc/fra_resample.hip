// fra_resample.hip -- resampled reads: a raster at any output size (fra_resample), a region of a set of tile streams
// decoded and resampled without the full-resolution region leaving the GPU (fra_decode_device_resampled), and the
// nodata-aware reads: fra_resample_masked, fra_decimate_masked and the two behind the decoder
// (fra_decode_device_resampled_masked, fra_decode_device_decimated_masked).
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
// With a nodata value ("Nodata-aware reads"): coordinates, taps and weights are the same; a pixel x is invalid when
// (double)x == nd or, in a float dtype, when it is NaN; the fill is (T)nd.
//   average  down the rows c_i = sum of vy_j x[j][i] over the valid pixels (floats: the first valid term initialises)
//            and u_i = sum of vy_j over them; left to right over the columns with u_i > 0  S = sum vx_i c_i,
//            W = sum vx_i u_i; W == 0 gives the fill, else rint((double)S / (double)W) or (T)(acc / (double)W)
//   bilinear, cubic  all taps valid: the unmasked formula; else the masked bilinear of the same centre
//   nearest  picks its pixel, invalid or not
// The decimation by k is the same arithmetic with h' = w' = k and oh' = ow' = 1 (every weight 1, the tap ranges clipped
// at the raster's edge): only the reduced sizes the host hands over differ.
//
// k_resample<T, MODE, MASKED, NARROW> is the one kernel of all of them; "k_resample_masked" in the documents names its
// MASKED instantiations.
// MODE 0 | 2 | 3: one thread per output element; a workgroup is 256 consecutive output columns of one output row of one
// band, so the row's taps and weights are wave-uniform and the column's are computed once per thread.
// MODE 1: a workgroup is (band, output row, `per` consecutive output columns), `per` chosen by the host so that their
// source columns fit the workgroup's 256 V (V = 16 / sizeof(T)).  A thread owns V adjacent source columns (one 16-byte
// load per row when the layout allows, guarded element loads otherwise -- k_decimate's two paths) and accumulates them
// down the output row's source rows, four rows requested at once with the next four in flight; the column sums go to
// LDS once, and the threads that own an output sum their taps from there left to right.  When one output column spans
// more than 256 V source columns (per = 1) the workgroup walks its span in chunks of 256 V and the thread carries the sum.
// For 8- and 16-bit integers whose column sums fit 32 bits (h' 2^(8 itemsize) <= 2^31) the columns are accumulated with
// 24-bit multiplies in 32 bits (NARROW); the output's sum is 64-bit always.
// MASKED adds, under `if constexpr`: the valid weight u_i beside c_i, in registers (32 bits: u_i <= h' <= 2^31; NARROW,
// which then also needs h' < 2^16: two columns' 16-bit weights share a register) and in LDS; W beside S, carried over
// the chunks like it; and the count of fill outputs per band (optional), summed over the workgroup (fra_region.h:
// wg_sum) and added by one atomicAdd per workgroup that has any into a zeroed array of `channels` 64-bit words.  How a
// sum starts differs on purpose: an unmasked sum is initialised by its first term and a masked float sum by its first
// valid term (a sum started at +0.0 would turn a raster of -0.0 into +0.0); masked integer sums start at 0 and an
// invalid pixel weighs 0.  Nothing else is shared between workgroups; all indices are 64-bit.
//
// This unit holds the kernel, its launch and the entries.  Shared with fra_warp.hip (fra_resample.h): invalid and
// combine_taps; with fra_decimate.hip: AccOf and the refusal of a factor; with all the units over fra_region.h: the
// dtype and layout refusal, what is left to the windowed read, staging, the decoded region, the timed launch and the
// workgroup's sum.
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

// (the masked NARROW average of 8-bit integers is held to 3 waves per SIMD, what its unmasked instance reaches: left
// alone it comes out one register over)
template <typename T, int MODE, bool MASKED, bool NARROW = false>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(MASKED && MODE == 1 && NARROW && sizeof(T) == 1 ? 3 : 1))) k_resample(ResampleArgs a) {
  const T* __restrict__ src = (const T*)a.src;
  T* __restrict__ dst = (T*)a.dst;
  const uint32_t seg = blockIdx.x % (uint32_t)a.nseg;
  const uint32_t rest = blockIdx.x / (uint32_t)a.nseg;
  const int64_t R = (int64_t)(rest % (uint32_t)a.oh);
  const int64_t b = (int64_t)(rest / (uint32_t)a.oh);
  const int64_t h = a.h, w = a.w;
  [[maybe_unused]] const T nd = (T)a.nodata;  // MASKED: the compare's constant and the fill
  [[maybe_unused]] uint32_t nfill = 0;        // MASKED: this thread's outputs that no valid pixel reached
  if constexpr (MODE == FRA_RESAMPLE_NEAREST) {
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C < a.ow) {
      const int64_t r = min(udiv((2 * R + 1) * a.hr, 2 * a.ohr), h - 1);
      const int64_t c = min(udiv((2 * C + 1) * a.wr, 2 * a.owr), w - 1);
      const T x = src[b * a.sbs + r * a.srs + c * a.scs];
      dst[b * a.dbs + R * a.drs + C * a.dcs] = x;
      if constexpr (MASKED) nfill = invalid(x, nd) ? 1u : 0u;
    }
  } else if constexpr (MODE == FRA_RESAMPLE_BILINEAR || MODE == FRA_RESAMPLE_CUBIC) {
    constexpr int NT = kTaps<MODE>;
    constexpr int OFF = MODE == FRA_RESAMPLE_BILINEAR ? 0 : -1;
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C < a.ow) {
      int64_t i0y, i0x;
      double ty, tx;
      centre(R, a.hr, a.ohr, &i0y, &ty);  // wave-uniform
      centre(C, a.wr, a.owr, &i0x, &tx);
      T x[NT][NT];  // [j][i]: tap row j, tap column i
#pragma unroll
      for (int j = 0; j < NT; j++) {
        const T* row = src + (b * a.sbs + min(max(i0y + OFF + j, (int64_t)0), h - 1) * a.srs);
#pragma unroll
        for (int i = 0; i < NT; i++) x[j][i] = row[min(max(i0x + OFF + i, (int64_t)0), w - 1) * a.scs];
      }
      dst[b * a.dbs + R * a.drs + C * a.dcs] = combine_taps<T, MODE, MASKED, from_f64<T>>(x, ty, tx, nd, nd, &nfill);
    }
  } else {
    using A = typename AccOf<T>::type;                  // an output's sum, as the rule has it
    using CA = std::conditional_t<NARROW, int32_t, A>;  // a column's sum (NARROW: it fits 32 bits, says the host)
    using UA = std::conditional_t<NARROW, uint16_t, uint32_t>;  // MASKED: a column's valid weight in LDS
    constexpr bool FLT = std::is_floating_point<T>::value;
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int64_t SPAN = 256 * V;  // source columns of a workgroup per chunk
    constexpr int G = 4;               // source rows requested at once by 16-byte loads
    struct alignas(16) Vec { T v[V]; };
    struct Sum { CA c; };               // a column's sum ...
    struct SumW { CA c; UA u; };        // ... MASKED: and its valid weight, read together by the taps
    using Col = std::conditional_t<MASKED, SumW, Sum>;
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
    [[maybe_unused]] const double n = (double)(a.hr * a.wr);
    A run = 0;  // the running S of a thread's output (carried over the chunks when per == 1)
    [[maybe_unused]] int64_t run_w = 0;  // MASKED: ... and its W
    // a weight times a pixel as a column's term (NARROW: both within 24 bits)
    auto times = [](int64_t wgt, T xv) -> CA {
      if constexpr (NARROW) return __mul24((int)wgt, (int)xv);
      else return (CA)wgt * (CA)xv;
    };
    for (int64_t base = c_lo; base < c_hi; base += SPAN) {
      const int64_t col0 = base + (int64_t)tid * V;  // first source column of this thread
      const int64_t left = col0 < c_hi ? w - col0 : 0;  // columns from col0 to the row's end; 0 past the span's end
      const bool whole = a.vec && left >= V;
      const T* p = src + (b * a.sbs + j_lo * a.srs + col0 * a.scs);
      CA acc[V];
      constexpr int UP = NARROW ? 2 : 1;  // MASKED NARROW: two columns' valid weights (< 2^16 each) share a register
      [[maybe_unused]] uint32_t u[V / UP];
      if constexpr (MASKED) {
#pragma unroll
        for (int i = 0; i < V; i++) acc[i] = 0, u[i / UP] = 0;
      }
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
                if constexpr (!MASKED) {  // the first term initialises
                  const CA term = times(vy, x.v[i]);
                  acc[i] = (g == 0 && j0 == j_lo) ? term : acc[i] + term;
                } else if constexpr (FLT) {  // the first valid term initialises
                  const bool ok = !invalid(x.v[i], nd);
                  const CA term = times(vy, x.v[i]);
                  acc[i] = ok ? (u[i] == 0 ? term : acc[i] + term) : acc[i];
                  u[i] += ok ? (uint32_t)vy : 0u;
                } else {  // an invalid pixel weighs 0 in both sums
                  const int m = invalid(x.v[i], nd) ? 0 : (int)vy;
                  acc[i] += times(m, x.v[i]);
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
      for (int i = 0; i < V; i++) {
        if constexpr (MASKED) cols[i * 256 + tid] = Col{acc[i], (UA)(u[i / UP] >> (16 * (i % UP)))};
        else cols[i * 256 + tid] = Col{acc[i]};
      }
      __syncthreads();
      const int64_t lim = min(base + SPAN, c_hi);
      for (int64_t C = Ca + tid; C < Cb; C += 256) {
        const int64_t x_lo = C * a.wr, x_hi = (C + 1) * a.wr;
        const int64_t t_lo = udiv(x_lo, a.owr), t_hi = min(udiv(x_hi + a.owr - 1, a.owr), w);  // the output's taps
        const bool first = t_lo >= base;  // the output starts in this chunk
        A s = first ? (A)0 : run;
        [[maybe_unused]] int64_t wsum = first ? 0 : run_w;
        const int64_t i_lo = max(t_lo, base), i_hi = min(t_hi, lim);
        int64_t xe = i_lo * a.owr;  // where source column i begins, in units of 1 / ow' of a source column
        for (int64_t i = i_lo; i < i_hi; i++) {
          const int64_t lft = max(xe, x_lo);
          xe += a.owr;
          const int64_t vx = min(xe, x_hi) - lft;
          const uint32_t rel = (uint32_t)(i - base);
          const Col col = cols[(rel % V) * 256 + rel / V];
          const A term = (A)vx * (A)col.c;
          if constexpr (!MASKED) {
            s = (first && i == t_lo) ? term : s + term;
          } else if constexpr (FLT) {
            if (col.u != 0) {  // a column without a valid pixel is skipped; the first other one initialises
              s = wsum == 0 ? term : s + term;
              wsum += vx * (int64_t)col.u;
            }
          } else {  // (a column without a valid pixel has sum and weight 0: adding them skips it)
            s += term;
            wsum += vx * (int64_t)col.u;
          }
        }
        run = s;
        if constexpr (MASKED) run_w = wsum;
        if (t_hi <= lim) {
          double den;
          if constexpr (MASKED) den = (double)wsum;
          else den = n;
          T o;
          if (MASKED && wsum == 0) {
            o = nd;
            nfill++;
          } else if constexpr (FLT) {
            o = (T)(s / den);
          } else {
            o = (T)(long long)rint((double)s / den);
          }
          dst[b * a.dbs + R * a.drs + C * a.dcs] = o;
        }
      }
    }
  }
  if constexpr (MASKED) {
    if (a.filled) {  // uniform
      const uint32_t total = wg_sum(nfill);
      if (threadIdx.x == 0 && total) atomicAdd(&a.filled[b], (unsigned long long)total);
    }
  }
}

thread_local float g_resample_ms = 0.f;  // the last unmasked launch
thread_local float g_masked_ms = 0.f;    // the last masked one

template <typename T, bool MASKED>
void launch_t(int mode, unsigned grid, hipStream_t s, const ResampleArgs& a) {
  switch (mode) {
    case FRA_RESAMPLE_NEAREST: hipLaunchKernelGGL((k_resample<T, 0, MASKED>), dim3(grid), dim3(256), 0, s, a); break;
    case FRA_RESAMPLE_AVERAGE:
      if constexpr (std::is_integral<T>::value && sizeof(T) <= 2) {
        if (a.narrow) {
          hipLaunchKernelGGL((k_resample<T, 1, MASKED, true>), dim3(grid), dim3(256), 0, s, a);
          break;
        }
      }
      hipLaunchKernelGGL((k_resample<T, 1, MASKED>), dim3(grid), dim3(256), 0, s, a);
      break;
    case FRA_RESAMPLE_BILINEAR: hipLaunchKernelGGL((k_resample<T, 2, MASKED>), dim3(grid), dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((k_resample<T, 3, MASKED>), dim3(grid), dim3(256), 0, s, a); break;
  }
}

// what a read asks for beside its source and destination: an output size, or a decimation factor (factor != 0: the
// nodata-aware decimation; the unmasked one is fra_decimate.hip); a nodata value or none (null); where the fill counts
// go (host, channels words; null: not counted; masked only)
struct Want {
  int32_t oh, ow, factor, resampling;
  const double* nodata;
  uint64_t* filled;
};

// k_resample over `io`, timed, the fill counts and the destination copied back (`a` holds the sizes).  An output of
// the input's size is the input for a resampling; the decimation has no such case (plan_grid).
int launch_resample(Call& c, const Io& io, int dtype, int channels, ResampleArgs a, const Want& w) {
  const bool masked = w.nodata != nullptr, counted = masked && w.filled;
  int mode = w.resampling;
  unsigned grid = 0;
  if (const int rc = plan_grid(&a, io, dtype, channels, &mode, w.factor == 0, masked, &grid)) return rc;
  const size_t filled_bytes = (size_t)channels * sizeof(unsigned long long);
  if (masked) a.nodata = *w.nodata;
  if (counted) {
    HIPCHK(c.sc.alloc(&a.filled, filled_bytes));
    HIPCHK(hipMemsetAsync(a.filled, 0, filled_bytes, c.s));
  }
  return timed(
      c, masked ? &g_masked_ms : &g_resample_ms,
      [&]() -> int {
        with_dtype(dtype, [&](auto t) {
          if (masked) launch_t<decltype(t), true>(mode, grid, c.s, a);
          else launch_t<decltype(t), false>(mode, grid, c.s, a);
        });
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&]() -> int {
        if (counted) HIPCHK(hipMemcpyAsync(w.filled, a.filled, filled_bytes, hipMemcpyDeviceToHost, c.s));
        return copy_back(c, io.out);
      });
}

// A raster job.  The order of the refusals is each entry's own and is kept: a resampling refuses the raster, then the
// sizes; the decimation its factor, then the raster; the nodata value comes last.
int read_raster(fra_ctx* ctx, RasterJob r, const Want& w) {
  ResampleArgs a{};
  if (w.factor)
    if (const int rc = check_factor(r.h, r.w, w.factor, w.resampling, &a)) return rc;
  if (const int rc = check_raster(r)) return rc;
  if (!w.factor)
    if (const int rc = check_sizes(r.h, r.w, w.oh, w.ow, w.resampling, r.dtype, &a)) return rc;
  if (w.nodata)
    if (const int rc = check_nodata(*w.nodata, r.dtype)) return rc;
  r.oh = a.oh, r.ow = a.ow;
  return run_raster(ctx, r, [&](Call& c, const Io& io) { return launch_resample(c, io, r.dtype, r.channels, a, w); });
}

// A region of a set of tile streams.  Before what is left to the windowed read comes what does not need the region:
// the decimation's factor and code, or the resampling's output size and code (through a 1 x 1 probe); after it the
// sizes of the region, the nodata value and the cover.
int read_region(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, fra_decoded* infos, const Want& w) {
  ResampleArgs a{};
  const bool left = left_to_window_read(job, roi);
  if (w.factor) {
    if (const int rc = check_factor(roi->height, roi->width, w.factor, w.resampling, &a)) return rc;
  } else if (left) {
    if (const int rc = check_sizes(1, 1, w.oh, w.ow, w.resampling, FRA_U8, &a)) return rc;
  }
  if (left) return refer_to_window_read(ctx, job, roi, infos, false);
  if (!w.factor)
    if (const int rc = check_sizes(roi->height, roi->width, w.oh, w.ow, w.resampling, job->dst_dtype, &a)) return rc;
  if (w.nodata)
    if (const int rc = check_nodata(*w.nodata, job->dst_dtype)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region(ctx, job, roi, infos, a.oh, a.ow, [&](Call& c, const Io& io) {
    return launch_resample(c, io, job->dst_dtype, job->channels, a, w);
  });
}

int null_argument() { return fra_internal_set_error(FRA_E_INVALID, "null argument"); }

}  // namespace

extern "C" {

FRA_API int fra_resample_timing(float* ms) {
  if (!ms) return null_argument();
  *ms = g_resample_ms;
  return FRA_OK;
}

FRA_API int fra_resample_masked_timing(float* ms) {
  if (!ms) return null_argument();
  *ms = g_masked_ms;
  return FRA_OK;
}

FRA_API int fra_resample(fra_ctx* ctx, const fra_resample_job* job) {
  if (!ctx || !job || !job->src || !job->dst) return null_argument();
  return read_raster(ctx, raster_job(*job), Want{job->out_height, job->out_width, 0, job->resampling, nullptr, nullptr});
}

FRA_API int fra_resample_masked(fra_ctx* ctx, const fra_resample_job* job, double nodata, uint64_t* filled) {
  if (!ctx || !job || !job->src || !job->dst) return null_argument();
  return read_raster(ctx, raster_job(*job), Want{job->out_height, job->out_width, 0, job->resampling, &nodata, filled});
}

FRA_API int fra_decimate_masked(fra_ctx* ctx, const fra_decimate_job* job, double nodata, uint64_t* filled) {
  if (!ctx || !job || !job->src || !job->dst) return null_argument();
  return read_raster(ctx, raster_job(*job), Want{0, 0, job->factor, job->resampling, &nodata, filled});
}

FRA_API int fra_decode_device_resampled(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                        int32_t out_height, int32_t out_width, int32_t resampling, fra_decoded* infos) {
  if (!ctx || !job || !roi || !infos) return null_argument();
  return read_region(ctx, job, roi, infos, Want{out_height, out_width, 0, resampling, nullptr, nullptr});
}

FRA_API int fra_decode_device_resampled_masked(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                               int32_t out_height, int32_t out_width, int32_t resampling,
                                               fra_decoded* infos, double nodata, uint64_t* filled) {
  if (!ctx || !job || !roi || !infos) return null_argument();
  return read_region(ctx, job, roi, infos, Want{out_height, out_width, 0, resampling, &nodata, filled});
}

FRA_API int fra_decode_device_decimated_masked(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                               int32_t factor, int32_t resampling, fra_decoded* infos, double nodata,
                                               uint64_t* filled) {
  if (!ctx || !job || !roi || !infos) return null_argument();
  return read_region(ctx, job, roi, infos, Want{0, 0, factor, resampling, &nodata, filled});
}

}  // extern "C"
