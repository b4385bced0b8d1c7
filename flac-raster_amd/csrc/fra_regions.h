// fra_regions.h -- the host arithmetic of the regions unit (fra_regions.hip) that needs no GPU: the refusals of a job in
// the header's order, the launch plan of the tile and seam kernels and of the two prefix sums, and the FRA_E_SPACE
// decisions once a band's count of kept components is known (include/flac_raster_amd.h, "Regions").
// tools/decode_host_check.cpp checks all of it in the stand-alone program.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_proximity.h"  // out_bits, the target predicate
#include "fra_region.h"

namespace fra_rg {

constexpr int32_t kMaxSide = 32768;
constexpr int kTile = 64;                      // side of the tile a workgroup labels in LDS
constexpr int kThreads = 256;                  // of every workgroup of the unit
constexpr int kRun = kTile * kTile / kThreads; // pixels of a tile row one thread walks: 16
constexpr int kScanItems = 16;                 // items per thread of a prefix-sum block
constexpr int kScanBlock = kThreads * kScanItems;
constexpr uint32_t kBackground = 0xffffffffu;  // the parent of a background pixel
constexpr uint32_t kRootBit = 0x80000000u;     // parent of a numbered root: kRootBit | its component index

// the bits of a pixel's link byte
constexpr unsigned kFg = 1u, kW = 2u, kN = 4u, kNW = 8u, kNE = 16u;

// the greatest N a labels dtype holds
inline int64_t label_max(int dtype) {
  int64_t m = 0;
  fra_region::with_int_dtype(dtype, [&](auto t) {
    using Z = decltype(t);
    m = (int64_t)std::numeric_limits<Z>::max();
  });
  return m;
}

// FRA_E_INVALID for what the rule refuses, in the header's order (after the null arguments)
inline int check_job(int dtype, int32_t channels, int32_t h, int32_t w, const fra_region::Strides& ss, const fra_regions_opts* o) {
  if (const int rc = fra_region::check_raster(dtype, channels, std::max(h, 1), std::max(w, 1), ss, ss)) return rc;
  if (channels > 255) return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d bands, more than 255)", channels);
  if (o->labels.dst && !fra_region::is_int_dtype(o->labels.dtype))
    return fra_internal_set_error(FRA_E_INVALID, "bad labels dtype %d (an integer dtype is needed)", o->labels.dtype);
  auto bad_layout = [](const fra_calc_dst& d) { return d.band_stride < 0 || d.row_stride < 0 || d.col_stride < 0; };
  if (o->labels.dst && bad_layout(o->labels)) return fra_internal_set_error(FRA_E_INVALID, "bad labels layout (a negative stride)");
  if (o->area.dst) {
    if (o->area.dtype < FRA_U8 || o->area.dtype > FRA_F64) return fra_internal_set_error(FRA_E_INVALID, "bad area dtype %d", o->area.dtype);
    if (bad_layout(o->area)) return fra_internal_set_error(FRA_E_INVALID, "bad area layout (a negative stride)");
  }
  if (o->sieved.dst && bad_layout(o->sieved)) return fra_internal_set_error(FRA_E_INVALID, "bad sieved layout (a negative stride)");
  if (h < 1 || h > kMaxSide || w < 1 || w > kMaxSide)
    return fra_internal_set_error(FRA_E_INVALID, "the region must be 1 .. %d in each dimension (got %d x %d)", kMaxSide, h, w);
  if (o->nvalues < 0 || o->nvalues > 16)
    return fra_internal_set_error(FRA_E_INVALID, "nvalues: %d foreground values (0 .. 16)", o->nvalues);
  for (int i = 0; i < o->nvalues; i++)
    if (!std::isfinite(o->values[i])) return fra_internal_set_error(FRA_E_INVALID, "values: foreground value %d is not finite", i);
  if (o->connectivity != 4 && o->connectivity != 8)
    return fra_internal_set_error(FRA_E_INVALID, "connectivity: %d is neither 4 nor 8", o->connectivity);
  if (o->min_size < 1) return fra_internal_set_error(FRA_E_INVALID, "min_size: %d is below 1", o->min_size);
  if (o->table_cap < 0) return fra_internal_set_error(FRA_E_INVALID, "table_cap: %d is negative", o->table_cap);
  if (!o->labels.dst && !o->area.dst && !o->sieved.dst && !o->table)
    return fra_internal_set_error(FRA_E_INVALID, "none of labels, area, sieved and table is given");
  return FRA_OK;
}

// FRA_E_SPACE when the N kept components of `band` do not fit the labels dtype or the table
inline int check_space(int32_t band, int64_t n, const fra_regions_opts* o) {
  if (o->labels.dst && n > label_max(o->labels.dtype))
    return fra_internal_set_error(FRA_E_SPACE, "band %d has %lld components, more than the labels dtype holds (%lld)", band, (long long)n,
                                  (long long)label_max(o->labels.dtype));
  if (o->table && n > (int64_t)o->table_cap)
    return fra_internal_set_error(FRA_E_SPACE, "band %d has %lld components, more than the table holds (%d)", band, (long long)n,
                                  o->table_cap);
  return FRA_OK;
}

// Whether a call can end in FRA_E_SPACE at all: with more than one band such a call counts every band before it writes
inline bool may_lack_space(int32_t h, int32_t w, const fra_regions_opts* o) {
  const int64_t most = (int64_t)h * w;  // no band has more components than pixels
  return (o->labels.dst && most > label_max(o->labels.dtype)) || (o->table && most > (int64_t)o->table_cap);
}

// The launch plan of a checked job.
//   Tiles: tiles_x x tiles_y workgroups, each over kTile x kTile pixels (the last ones cut by the region's edge).
//   Seams: one thread per pixel of the first row of every tile row but the first (its N, NW, NE links cross the border)
//   and one per row of every tile column but the first (the W and NW links of its first pixel and the NE link of the
//   pixel left of it; on the first row of a tile only W: the row threads have the others).
//   Scans: blocks of kScanBlock items, one workgroup each, and one workgroup that adds up the block sums.
struct Plan {
  int32_t tiles_x, tiles_y;
  int64_t npix;
  int64_t seam_row_threads, seam_col_threads;
  uint32_t link_wgs, seam_wgs, pixel_scan_blocks;
};
inline uint32_t scan_blocks(int64_t n) { return (uint32_t)((n + kScanBlock - 1) / kScanBlock); }
inline Plan make_plan(int32_t h, int32_t w) {
  Plan p{};
  p.tiles_x = (w + kTile - 1) / kTile, p.tiles_y = (h + kTile - 1) / kTile;
  p.npix = (int64_t)h * w;
  p.seam_row_threads = (int64_t)(p.tiles_y - 1) * w;
  p.seam_col_threads = (int64_t)(p.tiles_x - 1) * h;
  p.link_wgs = (uint32_t)((p.npix + kThreads - 1) / kThreads);
  p.seam_wgs = (uint32_t)((p.seam_row_threads + p.seam_col_threads + kThreads - 1) / kThreads);
  p.pixel_scan_blocks = scan_blocks(p.npix);
  return p;
}

}  // namespace fra_rg
