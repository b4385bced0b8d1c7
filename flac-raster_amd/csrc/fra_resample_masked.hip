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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"

extern "C" void fra_internal_ctx_stream(fra_ctx* ctx, int* device, hipStream_t* stream);

namespace {

struct MaskedArgs {
  const void* src;
  void* dst;
  int64_t sbs, srs, scs;  // source element strides: band, row, column
  int64_t dbs, drs, dcs;  // destination element strides
  int32_t h, w, oh, ow;
  int64_t hr, ohr, wr, owr;  // h', oh', w', ow'
  int32_t nseg;              // workgroups per output row
  int32_t per;               // average: output columns of a workgroup
  int32_t vec;  // average: 16-byte row loads are aligned (scs == 1; base, row and band strides multiples of 16 bytes)
  int32_t narrow;  // average of 8- and 16-bit integers: a column's sum fits 32 bits and its valid weight 16
  double nodata;
  unsigned long long* filled;  // one word per band, zeroed by the host; null: not counted
};

template <typename T>
struct AccOf { using type = std::conditional_t<std::is_floating_point<T>::value, double, long long>; };

// a / b for a >= 0, b > 0; the 32-bit division when both fit
__device__ inline int64_t udiv(int64_t a, int64_t b) {
  if ((((uint64_t)a | (uint64_t)b) >> 32) == 0) return (int64_t)((uint32_t)a / (uint32_t)b);
  return (int64_t)((uint64_t)a / (uint64_t)b);
}

// i0 and t of output index C along an axis of reduced sizes (nr source, onr output)
__device__ inline void centre(int64_t C, int64_t nr, int64_t onr, int64_t* i0, double* t) {
  const int64_t num = (2 * C + 1) * nr - onr, den = 2 * onr;  // num > -den: the floor of a negative num is -1
  *i0 = num < 0 ? -1 : udiv(num, den);
  *t = (double)(num - *i0 * den) / (double)den;
}

__device__ inline void cubic_weights(double t, double* wt) {
  wt[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
  wt[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
  wt[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
  wt[3] = ((0.5 * t - 0.5) * t) * t;
}

template <typename T>
__device__ inline T from_f64(double v) {
  if constexpr (std::is_floating_point<T>::value) {
    return (T)v;
  } else {
    constexpr double lo = std::is_signed<T>::value ? -(double)(1ull << (8 * sizeof(T) - 1)) : 0.0;
    constexpr double hi = (double)((1ull << (8 * sizeof(T) - (std::is_signed<T>::value ? 1 : 0))) - 1);
    return (T)(long long)fmin(fmax(rint(v), lo), hi);
  }
}

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
          cubic_weights(ty, wy);
          cubic_weights(tx, wx);
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

// FRA_E_INVALID unless nd is a nodata value of the dtype (the rule): an integer inside an integer dtype's range; NaN,
// or finite and exact in a float dtype
int check_nodata(double nd, int dtype) {
  bool ok;
  if (dtype == FRA_F64) {
    ok = std::isnan(nd) || std::isfinite(nd);
  } else if (dtype == FRA_F32) {
    ok = std::isnan(nd) || (std::isfinite(nd) && std::fabs(nd) <= (double)FLT_MAX && (double)(float)nd == nd);
  } else {
    const int bits = 8 * elem_size(dtype);
    const bool sgn = dtype == FRA_I8 || dtype == FRA_I16 || dtype == FRA_I32;
    const double lo = sgn ? -std::ldexp(1.0, bits - 1) : 0.0, hi = std::ldexp(1.0, sgn ? bits - 1 : bits) - 1.0;
    ok = std::isfinite(nd) && nd == std::floor(nd) && nd >= lo && nd <= hi;
  }
  if (!ok)
    return fra_internal_set_error(FRA_E_INVALID,
                                  "nodata %.17g is not a value of the dtype (an integer in range; for floats NaN, or "
                                  "finite and exact)", nd);
  return FRA_OK;
}

// the sizes of a resampling into `a`; FRA_E_INVALID for an output size, a code or an average the rule refuses
int check_sizes(int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t resampling, int dtype, MaskedArgs* a) {
  if (oh < 1 || oh > FRA_RESAMPLE_MAX_OUT || ow < 1 || ow > FRA_RESAMPLE_MAX_OUT)
    return fra_internal_set_error(FRA_E_INVALID, "the output size must be 1 .. %d in each dimension (got %d x %d)",
                                  FRA_RESAMPLE_MAX_OUT, oh, ow);
  if (resampling < FRA_RESAMPLE_NEAREST || resampling > FRA_RESAMPLE_CUBIC)
    return fra_internal_set_error(FRA_E_INVALID, "unknown resampling %d (0 nearest, 1 average, 2 bilinear, 3 cubic)",
                                  resampling);
  const int64_t gh = std::gcd((int64_t)h, (int64_t)oh), gw = std::gcd((int64_t)w, (int64_t)ow);
  a->h = h, a->w = w, a->oh = oh, a->ow = ow;
  a->hr = h / gh, a->ohr = oh / gh, a->wr = w / gw, a->owr = ow / gw;
  if (resampling == FRA_RESAMPLE_AVERAGE) {
    const int64_t n = a->hr * a->wr;  // < 2^62
    const bool is_float = dtype == FRA_F32 || dtype == FRA_F64;
    if (is_float ? n > ((int64_t)1 << 53) : n > ((int64_t)1 << (63 - 8 * elem_size(dtype))))
      return fra_internal_set_error(FRA_E_INVALID,
                                    "average: %d x %d -> %d x %d has n = %lld weights per output pixel, more than the "
                                    "rule's exact arithmetic holds",
                                    h, w, oh, ow, (long long)n);
  }
  return FRA_OK;
}

int log2_factor(int k) {
  for (int l = 1; l <= 6; l++)
    if (k == (1 << l)) return l;
  return 0;
}

// the sizes of a decimation by `factor` into `a`: h' = w' = k, oh' = ow' = 1
int check_factor(int32_t h, int32_t w, int32_t factor, int32_t resampling, MaskedArgs* a) {
  if (!log2_factor(factor))
    return fra_internal_set_error(FRA_E_INVALID, "the decimation factor must be 2, 4, 8, 16, 32 or 64 (got %d)", factor);
  if (resampling != FRA_RESAMPLE_NEAREST && resampling != FRA_RESAMPLE_AVERAGE)
    return fra_internal_set_error(FRA_E_INVALID, "unknown resampling %d (0 nearest, 1 average)", resampling);
  a->h = h, a->w = w;
  a->oh = (int32_t)(((int64_t)h + factor - 1) / factor), a->ow = (int32_t)(((int64_t)w + factor - 1) / factor);
  a->hr = a->wr = factor, a->ohr = a->owr = 1;
  return FRA_OK;
}

// k_resample_masked over device buffers between two events, and the fill counts into `filled` (host, channels words;
// may be null); enqueues only.  `same_size_copies`: an output of the input's size is the input (the resampling's rule;
// the decimation has no such case).
int launch_masked(int dtype, int mode, int channels, MaskedArgs a, bool same_size_copies, const void* d_src, void* d_dst,
                  double nodata, uint64_t* filled, HipArena& sc, hipEvent_t e0, hipEvent_t e1, hipStream_t s) {
  const size_t es = (size_t)elem_size(dtype);
  a.src = d_src;
  a.dst = d_dst;
  a.nodata = nodata;
  a.filled = nullptr;
  if (same_size_copies && a.oh == a.h && a.ow == a.w) mode = FRA_RESAMPLE_NEAREST;
  a.vec = a.scs == 1 && ((uintptr_t)d_src % 16) == 0 && (((uint64_t)a.srs * es) % 16) == 0 &&
          (((uint64_t)a.sbs * es) % 16) == 0;
  a.per = 1;
  if (mode == FRA_RESAMPLE_AVERAGE) {
    // `per` consecutive outputs cover at most ceil(per w / ow) + 1 source columns, V - 1 more from the aligned start
    const int64_t V = 16 / (int64_t)es, room = 256 * V - V - 1;
    a.per = (int32_t)std::min<int64_t>(std::max<int64_t>(room * a.owr / a.wr, 1), a.ow);
    a.nseg = (int32_t)(((int64_t)a.ow + a.per - 1) / a.per);
    a.per = (int32_t)(((int64_t)a.ow + a.nseg - 1) / a.nseg);  // the same workgroups, evenly filled
    // the weights of a column's rows sum to h' and each is at most min(h', oh') <= 65536
    a.narrow = dtype <= FRA_I16 && a.hr <= ((int64_t)1 << (31 - 8 * (int)es)) && a.hr < 65536;
  } else {
    a.nseg = (int32_t)(((int64_t)a.ow + 255) / 256);
  }
  const int64_t grid = (int64_t)channels * a.oh * a.nseg;
  if (grid > INT32_MAX) return fra_internal_set_error(FRA_E_INVALID, "the raster is too large for one resampling");
  if (filled) {
    HIPCHK(sc.alloc(&a.filled, (size_t)channels * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(a.filled, 0, (size_t)channels * sizeof(unsigned long long), s));
  }
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
  if (filled) HIPCHK(hipMemcpyAsync(filled, a.filled, (size_t)channels * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  return FRA_OK;
}

// elements addressed from element 0 by a (channels, rows, cols) raster of the given strides
int64_t extent_of(int64_t channels, int64_t rows, int64_t cols, int64_t bs, int64_t rs, int64_t cs) {
  return (channels - 1) * bs + (rows - 1) * rs + (cols - 1) * cs + 1;
}

// what fra_resample_job and fra_decimate_job share, once the sizes are in `a`
struct RasterJob {
  const void* src;
  int32_t src_on_device, dtype, channels;
  void* dst;
  int32_t dst_on_device;
};

// a raster job from the staging of its host buffers to the kernel's time
int run_raster(fra_ctx* ctx, const RasterJob& job, int mode, const MaskedArgs& a, bool same_size_copies, double nodata,
               uint64_t* filled) {
  int device = 0;
  hipStream_t s = nullptr;
  fra_internal_ctx_stream(ctx, &device, &s);
  (void)hipSetDevice(device);
  HipArena sc;  // staging buffers, the counts and the events of this call, released on every path
  const size_t es = (size_t)elem_size(job.dtype);
  const size_t src_bytes = (size_t)extent_of(job.channels, a.h, a.w, a.sbs, a.srs, a.scs) * es;
  const size_t dst_bytes = (size_t)extent_of(job.channels, a.oh, a.ow, a.dbs, a.drs, a.dcs) * es;
  const void* d_src = job.src;
  void* d_dst = job.dst;
  if (!job.src_on_device) {
    void* p = nullptr;
    HIPCHK(sc.alloc(&p, src_bytes));
    HIPCHK(hipMemcpyAsync(p, job.src, src_bytes, hipMemcpyHostToDevice, s));
    d_src = p;
  }
  if (!job.dst_on_device) {  // staged whole, so that the elements between the outputs keep the caller's values
    HIPCHK(sc.alloc(&d_dst, dst_bytes));
    HIPCHK(hipMemcpyAsync(d_dst, job.dst, dst_bytes, hipMemcpyHostToDevice, s));
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(sc.event(&e0, hipEventDefault));
  HIPCHK(sc.event(&e1, hipEventDefault));
  if (const int rc = launch_masked(job.dtype, mode, job.channels, a, same_size_copies, d_src, d_dst, nodata, filled, sc,
                                   e0, e1, s))
    return rc;
  if (!job.dst_on_device) HIPCHK(hipMemcpyAsync(job.dst, d_dst, dst_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  g_masked_ms = ms;
  return FRA_OK;
}

// what the windowed read refuses at once (it does so before any GPU work, with its own message)
bool left_to_window_read(const fra_decode_job* job, const fra_window* roi) {
  return roi->height <= 0 || roi->width <= 0 || roi->row_off < 0 || roi->col_off < 0 || job->nitems < 0 ||
         (job->nitems && !job->items) || !job->dst || job->dst_dtype < FRA_U8 || job->dst_dtype > FRA_F64 ||
         job->channels < 1 || job->channels > 8 || job->band_stride < 0 || job->row_stride < 0 ||
         job->col_stride < 0 || (job->flags & FRA_DECODE_CONCAT) || !fra_region::item_windows_ok(job);
}

// the region decoded into a per-call buffer, then the kernel over it (the sizes are in `a`)
int run_region(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, int mode, MaskedArgs a,
               bool same_size_copies, double nodata, uint64_t* filled, fra_decoded* infos) {
  int device = 0;
  hipStream_t s = nullptr;
  fra_internal_ctx_stream(ctx, &device, &s);
  (void)hipSetDevice(device);
  HipArena sc;  // the region buffer, the staged output, the counts and the events: released on every path
  void* d_region = nullptr;  // the region at full resolution: band-planar, in dst_dtype, rows on 16-byte boundaries
  int64_t rs = 0;
  if (const int rc = fra_region::decode(ctx, job, roi, infos, sc, &d_region, &rs)) return rc;

  const size_t es = (size_t)elem_size(job->dst_dtype);
  a.sbs = (int64_t)roi->height * rs, a.srs = rs, a.scs = 1;
  a.dbs = job->band_stride, a.drs = job->row_stride, a.dcs = job->col_stride;
  const size_t dst_bytes = (size_t)extent_of(job->channels, a.oh, a.ow, a.dbs, a.drs, a.dcs) * es;
  void* d_dst = job->dst;
  if (!job->dst_on_device) {
    HIPCHK(sc.alloc(&d_dst, dst_bytes));
    HIPCHK(hipMemcpyAsync(d_dst, job->dst, dst_bytes, hipMemcpyHostToDevice, s));
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(sc.event(&e0, hipEventDefault));
  HIPCHK(sc.event(&e1, hipEventDefault));
  if (const int rc = launch_masked(job->dst_dtype, mode, job->channels, a, same_size_copies, d_region, d_dst, nodata,
                                   filled, sc, e0, e1, s))
    return rc;
  if (!job->dst_on_device) HIPCHK(hipMemcpyAsync(job->dst, d_dst, dst_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  g_masked_ms = ms;
  return FRA_OK;
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
  if (job->dtype < FRA_U8 || job->dtype > FRA_F64) return fra_internal_set_error(FRA_E_INVALID, "bad dtype %d", job->dtype);
  if (job->channels < 1 || job->height < 1 || job->width < 1 || job->src_band_stride < 0 || job->src_row_stride < 0 ||
      job->src_col_stride < 0 || job->dst_band_stride < 0 || job->dst_row_stride < 0 || job->dst_col_stride < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d x %d x %d)", job->channels, job->height,
                                  job->width);
  MaskedArgs a{};
  if (const int rc = check_sizes(job->height, job->width, job->out_height, job->out_width, job->resampling, job->dtype, &a))
    return rc;
  if (const int rc = check_nodata(nodata, job->dtype)) return rc;
  a.sbs = job->src_band_stride, a.srs = job->src_row_stride, a.scs = job->src_col_stride;
  a.dbs = job->dst_band_stride, a.drs = job->dst_row_stride, a.dcs = job->dst_col_stride;
  const RasterJob r{job->src, job->src_on_device, job->dtype, job->channels, job->dst, job->dst_on_device};
  return run_raster(ctx, r, job->resampling, a, true, nodata, filled);
}

FRA_API int fra_decimate_masked(fra_ctx* ctx, const fra_decimate_job* job, double nodata, uint64_t* filled) {
  if (!ctx || !job || !job->src || !job->dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  MaskedArgs a{};
  if (const int rc = check_factor(job->height, job->width, job->factor, job->resampling, &a)) return rc;
  if (job->dtype < FRA_U8 || job->dtype > FRA_F64) return fra_internal_set_error(FRA_E_INVALID, "bad dtype %d", job->dtype);
  if (job->channels < 1 || job->height < 1 || job->width < 1 || job->src_band_stride < 0 || job->src_row_stride < 0 ||
      job->src_col_stride < 0 || job->dst_band_stride < 0 || job->dst_row_stride < 0 || job->dst_col_stride < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d x %d x %d)", job->channels, job->height,
                                  job->width);
  if (const int rc = check_nodata(nodata, job->dtype)) return rc;
  a.sbs = job->src_band_stride, a.srs = job->src_row_stride, a.scs = job->src_col_stride;
  a.dbs = job->dst_band_stride, a.drs = job->dst_row_stride, a.dcs = job->dst_col_stride;
  const RasterJob r{job->src, job->src_on_device, job->dtype, job->channels, job->dst, job->dst_on_device};
  return run_raster(ctx, r, job->resampling, a, false, nodata, filled);
}

FRA_API int fra_decode_device_resampled_masked(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                               int32_t out_height, int32_t out_width, int32_t resampling,
                                               fra_decoded* infos, double nodata, uint64_t* filled) {
  if (!ctx || !job || !roi || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  MaskedArgs a{};
  if (left_to_window_read(job, roi)) {
    if (const int rc = check_sizes(1, 1, out_height, out_width, resampling, FRA_U8, &a)) return rc;
    const int rc = fra_decode_device_window(ctx, job, roi, infos);
    return rc ? rc : fra_internal_set_error(FRA_E_INVALID, "bad arguments");
  }
  if (const int rc = check_sizes(roi->height, roi->width, out_height, out_width, resampling, job->dst_dtype, &a)) return rc;
  if (const int rc = check_nodata(nodata, job->dst_dtype)) return rc;
  if (const int rc = fra_region::check_cover(job, roi)) return rc;
  return run_region(ctx, job, roi, resampling, a, true, nodata, filled, infos);
}

FRA_API int fra_decode_device_decimated_masked(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                               int32_t factor, int32_t resampling, fra_decoded* infos, double nodata,
                                               uint64_t* filled) {
  if (!ctx || !job || !roi || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  MaskedArgs a{};
  if (const int rc = check_factor(roi->height, roi->width, factor, resampling, &a)) return rc;
  if (left_to_window_read(job, roi)) {
    const int rc = fra_decode_device_window(ctx, job, roi, infos);
    return rc ? rc : fra_internal_set_error(FRA_E_INVALID, "bad arguments");
  }
  if (const int rc = check_nodata(nodata, job->dst_dtype)) return rc;
  if (const int rc = fra_region::check_cover(job, roi)) return rc;
  return run_region(ctx, job, roi, resampling, a, false, nodata, filled, infos);
}

}  // extern "C"
