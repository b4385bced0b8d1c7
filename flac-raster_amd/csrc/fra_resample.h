// fra_resample.h -- what the units that sample a raster share (fra_resample.hip with its nodata-aware reads and
// fra_warp.hip; fra_decimate.hip takes AccOf, log2_factor and check_factor): the resampling kernel's arguments, the
// device helpers of the rule (include/flac_raster_amd.h: centres, tap weights, the conversion of a result, what an
// invalid pixel is, and the value of a bilinear or cubic pixel from its taps: combine_taps, the one place that holds
// "all taps valid: the unmasked formula; else the masked bilinear of the same centre"), the refusals of an output size,
// a resampling code, an average the rule's exact arithmetic does not hold, a decimation factor and a nodata value, and
// the grid of a launch.  The host scaffold around the kernels is fra_region.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"

namespace fra_rs {

struct ResampleArgs {
  const void* src;
  void* dst;
  int64_t sbs, srs, scs;  // source element strides: band, row, column
  int64_t dbs, drs, dcs;  // destination element strides
  int32_t h, w, oh, ow;
  int64_t hr, ohr, wr, owr;  // h', oh', w', ow'
  int32_t nseg;              // workgroups per output row
  int32_t per;               // average: output columns of a workgroup
  int32_t vec;  // average: 16-byte row loads are aligned (scs == 1; base, row and band strides multiples of 16 bytes)
  int32_t narrow;  // average of 8- and 16-bit integers: a column's sum fits 32 bits (h' 2^(8 itemsize) <= 2^31); masked:
                   // and its valid weight 16
  double nodata;               // the masked instantiations only
  unsigned long long* filled;  // ... one word per band, zeroed by the host; null: not counted
};
static_assert(sizeof(ResampleArgs) == 144, "the kernel's arguments, without padding");

template <typename T>
struct AccOf { using type = std::conditional_t<std::is_floating_point<T>::value, double, long long>; };

// a / b for a >= 0, b > 0; the 32-bit division when both fit (the 64-bit one is several times as long)
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

template <int MODE>
__device__ inline void tap_weights(double t, double* wt) {
  if constexpr (MODE == FRA_RESAMPLE_BILINEAR) {
    wt[0] = 1.0 - t;
    wt[1] = t;
  } else {
    wt[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    wt[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
    wt[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    wt[3] = ((0.5 * t - 0.5) * t) * t;
  }
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

// taps per axis of a mode that interpolates
template <int MODE>
constexpr int kTaps = MODE == FRA_RESAMPLE_BILINEAR ? 2 : 4;

// The value of a bilinear or cubic pixel from its taps x[j][i] (tap row j, tap column i, already fetched and clamped)
// and the fractions ty, tx of its centre: the rule's formula, vertically (top to bottom) then left to right, converted
// by CONV.  MASKED: that formula when every tap is valid, else the masked bilinear of the same centre over the valid
// ones of its four taps; a pixel none of them reaches gets `fillv` and raises *nfill.
template <typename T, int MODE, bool MASKED, T (*CONV)(double)>
__device__ inline T combine_taps(const T (&x)[kTaps<MODE>][kTaps<MODE>], double ty, double tx, T nd, T fillv,
                                 uint32_t* nfill) {
  constexpr int NT = kTaps<MODE>;
  if constexpr (MASKED) {
    bool all = true;
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int i = 0; i < NT; i++) all = all && !invalid(x[j][i], nd);
    if (!all) {
      constexpr int M = MODE == FRA_RESAMPLE_CUBIC ? 1 : 0;  // where the bilinear taps i0, i0 + 1 lie among the NT
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
        *nfill += 1u;
        return fillv;
      }
      return CONV(v / wt);
    }
  }
  double wy[NT], wx[NT];
  tap_weights<MODE>(ty, wy);
  tap_weights<MODE>(tx, wx);
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < NT; i++) {
    double c = (double)x[0][i] * wy[0];  // vertically, top to bottom
#pragma unroll
    for (int j = 1; j < NT; j++) c = c + (double)x[j][i] * wy[j];
    v = i == 0 ? c * wx[0] : v + c * wx[i];  // then left to right
  }
  return CONV(v);
}

// the sizes of a resampling into `a`; FRA_E_INVALID for an output size, a code or an average the rule refuses
inline int check_sizes(int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t resampling, int dtype, ResampleArgs* a) {
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

inline int log2_factor(int k) {
  for (int l = 1; l <= 6; l++)
    if (k == (1 << l)) return l;
  return 0;
}

// the sizes of a decimation by `factor` into `a`: h' = w' = k, oh' = ow' = 1; FRA_E_INVALID for a factor or a code
inline int check_factor(int32_t h, int32_t w, int32_t factor, int32_t resampling, ResampleArgs* a) {
  if (!log2_factor(factor))
    return fra_internal_set_error(FRA_E_INVALID, "the decimation factor must be 2, 4, 8, 16, 32 or 64 (got %d)", factor);
  if (resampling != FRA_RESAMPLE_NEAREST && resampling != FRA_RESAMPLE_AVERAGE)
    return fra_internal_set_error(FRA_E_INVALID, "unknown resampling %d (0 nearest, 1 average)", resampling);
  a->h = h, a->w = w;
  a->oh = (int32_t)(((int64_t)h + factor - 1) / factor), a->ow = (int32_t)(((int64_t)w + factor - 1) / factor);
  a->hr = a->wr = factor, a->ohr = a->owr = 1;
  return FRA_OK;
}

// FRA_E_INVALID unless nd is a nodata value of the dtype (the rule): an integer inside an integer dtype's range; NaN,
// or finite and exact in a float dtype (`what`: the argument's name in the message)
inline int check_nodata(double nd, int dtype, const char* what = "nodata") {
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
                                  "%s %.17g is not a value of the dtype (an integer in range; for floats NaN, or "
                                  "finite and exact)", what, nd);
  return FRA_OK;
}

// The launch of k_resample over `io` into `a` (its sizes are set), *mode and *grid.
// `same_size_copies`: an output of the input's size is the input, in every mode (the resampling's rule; the decimation
// has no such case).  `masked`: the kernel keeps a column's valid weight in 16 bits beside its NARROW sum.
inline int plan_grid(ResampleArgs* a, const fra_region::Io& io, int dtype, int channels, int* mode, bool same_size_copies,
                     bool masked, unsigned* grid) {
  const size_t es = (size_t)elem_size(dtype);
  a->src = io.src, a->dst = io.out.dev;
  a->sbs = io.ss.band, a->srs = io.ss.row, a->scs = io.ss.col;
  a->dbs = io.ds.band, a->drs = io.ds.row, a->dcs = io.ds.col;
  if (same_size_copies && a->oh == a->h && a->ow == a->w) *mode = FRA_RESAMPLE_NEAREST;
  a->vec = fra_region::aligned16(io.src, io.ss, es);
  a->per = 1;
  if (*mode == FRA_RESAMPLE_AVERAGE) {
    // `per` consecutive outputs cover at most ceil(per w / ow) + 1 source columns, V - 1 more from the aligned start
    const int64_t V = 16 / (int64_t)es, room = 256 * V - V - 1;
    a->per = (int32_t)std::min<int64_t>(std::max<int64_t>(room * a->owr / a->wr, 1), a->ow);
    a->nseg = (int32_t)(((int64_t)a->ow + a->per - 1) / a->per);
    a->per = (int32_t)(((int64_t)a->ow + a->nseg - 1) / a->nseg);  // the same workgroups, evenly filled
    // the weights of a column's rows sum to h' and each is at most min(h', oh') <= 65536
    a->narrow = dtype <= FRA_I16 && a->hr <= ((int64_t)1 << (31 - 8 * (int)es)) && (!masked || a->hr < 65536);
  } else {
    a->nseg = (int32_t)(((int64_t)a->ow + 255) / 256);
  }
  const int64_t n = (int64_t)channels * a->oh * a->nseg;
  if (n > INT32_MAX) return fra_internal_set_error(FRA_E_INVALID, "the raster is too large for one resampling");
  *grid = (unsigned)n;
  return FRA_OK;
}

}  // namespace fra_rs
