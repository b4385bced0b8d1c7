// fra_proximity.h -- the host arithmetic of the proximity unit (fra_proximity.hip) that needs no GPU: the refusals of a
// job in the header's order, the reach threshold (the greatest squared distance whose f64 distance is within max_dist),
// the conversion of a fill to an output's bits, and the launch plan of the two phases (include/flac_raster_amd.h,
// "Proximity").  tools/decode_host_check.cpp checks all of it in the stand-alone program.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"

namespace fra_px {

constexpr int32_t kMaxSide = 32768;
constexpr int64_t kMaxD2 = 2ll * 32767 * 32767;  // 2147352578 < 2^31: the greatest squared distance inside a region
constexpr int kChunkRows = 64;                   // rows of a column in one target mask
constexpr int kThreads = 256;                    // of every workgroup of the unit
constexpr int kSub = 8;                          // lanes that share a pixel's short candidate range in k_prox_rows
constexpr int kLong = 64;                        // a range of more candidates goes to a whole wave
constexpr int32_t kTeamWidth = 512;              // up to this region width a workgroup solves four rows, a wave each
constexpr uint16_t kNone = 1;                    // the 16-bit intermediate is g << 1 | below; g == 0 is never below

// d <= max_dist for the squared distance d2, as the rule states it
inline bool within(int64_t d2, double scale, double max_dist) { return std::sqrt((double)d2) * scale <= max_dist; }

// The greatest d2 in 0 .. kMaxD2 within reach.  sqrt and the product by a positive scale are monotone, so the predicate
// holds up to one d2 and a bisection finds it; it holds at 0 because max_dist >= 0.
inline int64_t reach_threshold(bool has_max_dist, double scale, double max_dist) {
  if (!has_max_dist || within(kMaxD2, scale, max_dist)) return kMaxD2;
  int64_t lo = 0, hi = kMaxD2;  // within(lo), !within(hi)
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    (within(mid, scale, max_dist) ? lo : hi) = mid;
  }
  return lo;
}

// floor(sqrt(t)) for 0 <= t < 2^31: no vertical distance beyond it is within reach
inline int32_t isqrt(int64_t t) {
  int64_t g = (int64_t)std::sqrt((double)t);
  while (g * g > t) g--;
  while ((g + 1) * (g + 1) <= t) g++;
  return (int32_t)g;
}

// the bits of to_out<D>(x) (fra_region.h) for a dtype, in the low bytes of the word: the fills are converted here
inline uint64_t out_bits(int dtype, double x) {
  uint64_t bits = 0;
  fra_region::with_dtype(dtype, [&](auto t) {
    using D = decltype(t);
    D v;
    if constexpr (std::is_floating_point<D>::value) {
      v = (D)(x != x ? std::numeric_limits<double>::quiet_NaN() : x);
      if (x != x) {  // the quiet NaN 0x7ff8000000000000 and its f32 cast, whatever the sign of the host's constant
        const uint64_t q64 = 0x7ff8000000000000ull;
        const uint32_t q32 = 0x7fc00000u;
        if constexpr (sizeof(D) == 8) std::memcpy(&v, &q64, 8); else std::memcpy(&v, &q32, 4);
      }
    } else {
      const double lo = (double)std::numeric_limits<D>::lowest(), hi = (double)std::numeric_limits<D>::max();
      const double r = std::nearbyint(x);  // half to even in the default rounding mode, as rint on the device
      v = (D)(x != x ? 0.0 : (r < lo ? lo : (r > hi ? hi : r)));
    }
    std::memcpy(&bits, &v, sizeof(D));
  });
  return bits;
}

#ifdef __HIPCC__
// the rule's target predicate (the regions unit's foreground is the same one): nvalues == 0: non-zero and not NaN
template <typename T>
__device__ inline bool is_target(T v, int32_t nvalues, const double* values) {
  if (nvalues == 0) return v != (T)0 && v == v;
  const double x = (double)v;
  bool hit = false;
  for (int i = 0; i < nvalues; i++) hit |= x == values[i];
  return hit;
}
#endif

// FRA_E_INVALID for what the rule refuses, in the header's order (after the null arguments): a (channels, h, w) source
// of `dtype` with the strides ss, and the options
inline int check_job(int dtype, int32_t channels, int32_t h, int32_t w, const fra_region::Strides& ss, const fra_proximity_opts* o) {
  if (const int rc = fra_region::check_raster(dtype, channels, std::max(h, 1), std::max(w, 1), ss, ss)) return rc;
  if (channels > 255) return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d bands, more than 255)", channels);
  if (o->dist.dst) {
    if (o->dist.dtype < FRA_U8 || o->dist.dtype > FRA_F64) return fra_internal_set_error(FRA_E_INVALID, "bad dist dtype %d", o->dist.dtype);
    if (o->dist.band_stride < 0 || o->dist.row_stride < 0 || o->dist.col_stride < 0)
      return fra_internal_set_error(FRA_E_INVALID, "bad dist layout (a negative stride)");
  }
  if (o->alloc.dst && (o->alloc.band_stride < 0 || o->alloc.row_stride < 0 || o->alloc.col_stride < 0))
    return fra_internal_set_error(FRA_E_INVALID, "bad alloc layout (a negative stride)");
  if (h < 1 || h > kMaxSide || w < 1 || w > kMaxSide)
    return fra_internal_set_error(FRA_E_INVALID, "the region must be 1 .. %d in each dimension (got %d x %d)", kMaxSide, h, w);
  if (o->nvalues < 0 || o->nvalues > 16)
    return fra_internal_set_error(FRA_E_INVALID, "nvalues: %d target values (0 .. 16)", o->nvalues);
  for (int i = 0; i < o->nvalues; i++)
    if (!std::isfinite(o->values[i])) return fra_internal_set_error(FRA_E_INVALID, "values: target value %d is not finite", i);
  if (!std::isfinite(o->scale) || !(o->scale > 0.0))
    return fra_internal_set_error(FRA_E_INVALID, "scale: %g is not finite and positive", o->scale);
  if (o->has_max_dist && !(o->max_dist >= 0.0))  // (a NaN fails the comparison)
    return fra_internal_set_error(FRA_E_INVALID, "max_dist: %g is NaN or negative", o->max_dist);
  if (o->out_height < 1 || o->out_width < 1 || o->out_row_off < 0 || o->out_col_off < 0 ||
      (int64_t)o->out_row_off + o->out_height > h || (int64_t)o->out_col_off + o->out_width > w)
    return fra_internal_set_error(FRA_E_INVALID, "the output window (%d, %d, %d x %d) is empty or not inside the region (%d x %d)",
                                  o->out_row_off, o->out_col_off, o->out_height, o->out_width, h, w);
  if (!o->dist.dst && !o->alloc.dst) return fra_internal_set_error(FRA_E_INVALID, "neither dist nor alloc is given");
  return FRA_OK;
}

// The launch plan of a checked job.
//   Columns: the region's rows in chunks of 64, one target mask per (chunk, column); the chunks k0 .. k1 hold the output
//   window's rows; every grid is col_blocks workgroups wide.
//   Rows: a team of team_threads threads solves one output row; rows_per_wg teams share a workgroup.  levels = the bit
//   length of out_width: level L solves the pixels (2 i + 1) * 2^(levels - 1 - L) - 1.  Per team the LDS holds the row's
//   intermediate (w words of 16 bits), the argmins (out_width words), the queue of the pixels with a long range and its
//   two counters.
struct Plan {
  int32_t nchunks, k0, k1, col_blocks;
  int32_t rows_per_wg, team_threads, levels, row_wgs;
  uint32_t g_off, opt_off, queue_off, count_off;  // bytes, inside a team's slice
  uint32_t queue_cap, team_bytes, lds_bytes;
};
inline int32_t bit_length(uint32_t x) {
  int32_t n = 0;
  for (; x; x >>= 1) n++;
  return n;
}
inline Plan make_plan(int32_t h, int32_t w, const fra_proximity_opts& o) {
  Plan p{};
  p.nchunks = (h + kChunkRows - 1) / kChunkRows;
  p.k0 = o.out_row_off / kChunkRows, p.k1 = (o.out_row_off + o.out_height - 1) / kChunkRows;
  p.col_blocks = (w + kThreads - 1) / kThreads;
  p.rows_per_wg = w <= kTeamWidth ? 4 : 1;
  p.team_threads = kThreads / p.rows_per_wg;
  p.levels = bit_length((uint32_t)o.out_width);
  p.row_wgs = (o.out_height + p.rows_per_wg - 1) / p.rows_per_wg;
  // Neighbouring ranges of a level share an end point, so their lengths add up to at most w + (pixels of the level) and
  // fewer than (w + out_width) / 64 of them are longer than 64.
  p.queue_cap = (uint32_t)((w + o.out_width) / kLong + 1);
  auto up4 = [](uint32_t b) { return (b + 3u) & ~3u; };
  p.g_off = 0;
  p.opt_off = up4(2u * (uint32_t)w);
  p.queue_off = p.opt_off + up4(2u * (uint32_t)o.out_width);
  p.count_off = p.queue_off + up4(2u * p.queue_cap);
  p.team_bytes = p.count_off + 8u;
  p.lds_bytes = p.team_bytes * (uint32_t)p.rows_per_wg;
  return p;
}

}  // namespace fra_px
