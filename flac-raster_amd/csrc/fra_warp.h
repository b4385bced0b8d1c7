// fra_warp.h -- the host arithmetic of the warped reads (fra_warp.hip) that needs no GPU: the refusals of an output
// size, a resampling code, the flags and a map, and the source window a map touches (include/flac_raster_amd.h, "Warped
// reads").  tools/decode_host_check.cpp checks all of it in the stand-alone program.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"

namespace fra_wp {

// FRA_E_INVALID for an output size, a resampling code or flags the rule refuses
inline int check_out(int32_t oh, int32_t ow, int32_t resampling, int32_t flags) {
  if (oh < 1 || oh > FRA_RESAMPLE_MAX_OUT || ow < 1 || ow > FRA_RESAMPLE_MAX_OUT)
    return fra_internal_set_error(FRA_E_INVALID, "the output size must be 1 .. %d in each dimension (got %d x %d)",
                                  FRA_RESAMPLE_MAX_OUT, oh, ow);
  if (resampling == FRA_RESAMPLE_AVERAGE)
    return fra_internal_set_error(FRA_E_INVALID,
                                  "a warp takes point samples: the average is not offered (read an overview, then warp it)");
  if (resampling != FRA_RESAMPLE_NEAREST && resampling != FRA_RESAMPLE_BILINEAR && resampling != FRA_RESAMPLE_CUBIC)
    return fra_internal_set_error(FRA_E_INVALID, "unknown resampling %d (0 nearest, 2 bilinear, 3 cubic)", resampling);
  if (flags & ~FRA_WARP_NODATA) return fra_internal_set_error(FRA_E_INVALID, "unknown warp flags 0x%x", (unsigned)flags);
  return FRA_OK;
}

// FRA_E_INVALID for a map the rule refuses for an oh x ow output (whose size has been checked)
inline int check_map(const fra_warp_map* m, int32_t oh, int32_t ow) {
  if (m->kind == FRA_WARP_AFFINE) {
    for (int k = 0; k < 6; k++)
      if (!std::isfinite(m->affine[k]))
        return fra_internal_set_error(FRA_E_INVALID, "affine coefficient %d of the map is not finite", k);
    return FRA_OK;
  }
  if (m->kind != FRA_WARP_GRID) return fra_internal_set_error(FRA_E_INVALID, "unknown map kind %d (0 affine, 1 grid)", m->kind);
  if (m->step < 1) return fra_internal_set_error(FRA_E_INVALID, "the grid step must be at least 1 (got %d)", m->step);
  const int64_t gh = ((int64_t)oh + m->step - 1) / m->step + 1, gw = ((int64_t)ow + m->step - 1) / m->step + 1;
  if (m->gh != gh || m->gw != gw)
    return fra_internal_set_error(FRA_E_INVALID, "a %d x %d output at step %d takes a grid of %lld x %lld nodes (got %d x %d)", oh,
                                  ow, m->step, (long long)gh, (long long)gw, m->gh, m->gw);
  if (!m->gx || !m->gy) return fra_internal_set_error(FRA_E_INVALID, "null grid");
  return FRA_OK;
}

constexpr int kMargin = 3;  // pixels the window grows by per side: the cubic's taps reach 2.5 from a coordinate

// The source window a checked map touches in an H x W raster: the hull of the coordinates (AFFINE: of the four corner
// pixel centres; GRID: of the nodes where both planes are finite), from floor(min) - 3 to floor(max) + 3 per axis,
// clipped to the raster.  false, and nothing written, when the hull misses [0, W) x [0, H) by more than a pixel (or
// has no finite node): no pixel is inside then, with a pixel to spare for the rounding of a pixel's own coordinate.
inline bool source_window(const fra_warp_map& m, int32_t H, int32_t W, int32_t oh, int32_t ow, fra_window* win) {
  double xmin = HUGE_VAL, xmax = -HUGE_VAL, ymin = HUGE_VAL, ymax = -HUGE_VAL;
  auto take = [&](double x, double y) {
    if (!std::isfinite(x) || !std::isfinite(y)) return;
    xmin = std::min(xmin, x), xmax = std::max(xmax, x), ymin = std::min(ymin, y), ymax = std::max(ymax, y);
  };
  if (m.kind == FRA_WARP_AFFINE) {
    const double* k = m.affine;
    for (double v : {0.5, (double)oh - 0.5})
      for (double u : {0.5, (double)ow - 0.5}) take((k[0] * u + k[1] * v) + k[2], (k[3] * u + k[4] * v) + k[5]);
  } else {
    const int64_t n = (int64_t)m.gh * m.gw;
    for (int64_t i = 0; i < n; i++) take(m.gx[i], m.gy[i]);
  }
  if (!(xmax >= -1.0 && xmin < (double)W + 1.0 && ymax >= -1.0 && ymin < (double)H + 1.0)) return false;
  const double c0 = std::max(std::floor(xmin) - kMargin, 0.0), c1 = std::min(std::floor(xmax) + kMargin, (double)W - 1.0);
  const double r0 = std::max(std::floor(ymin) - kMargin, 0.0), r1 = std::min(std::floor(ymax) + kMargin, (double)H - 1.0);
  win->row_off = (int32_t)r0, win->col_off = (int32_t)c0;
  win->height = (int32_t)(r1 - r0) + 1, win->width = (int32_t)(c1 - c0) + 1;
  return true;
}

}  // namespace fra_wp
