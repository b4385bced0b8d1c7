// fra_rasterize.h -- the host arithmetic of the polygon rasterizer (fra_rasterize.hip) that needs no GPU: the refusals
// of a job, the edge table (rings closed, level edges dropped, every edge oriented y0 < y1, a feature index per edge),
// the per-feature x-extent, and the binning of the edges into one list per band of 16 output rows
// (include/flac_raster_amd.h, "Rasterizing polygons").  tools/decode_host_check.cpp checks all of it in the stand-alone
// program.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <new>
#include <vector>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"

namespace fra_rz {

constexpr int kBandRows = 16;                  // output rows per band: the height of a tile of k_rasterize
constexpr int32_t kMaxSide = 65536;            // of the output window, per axis
constexpr int32_t kMaxFeatures = 1 << 24;
constexpr int64_t kMaxVerts = (int64_t)1 << 28;
constexpr double kMaxCoord = 4503599627370496.0;  // 2^52: a pixel centre is exact up to here
constexpr int64_t kMaxBinned = ((int64_t)1 << 31) - 1;  // entries of all the band lists together

struct Edge { double x0, y0, x1, y1; };   // y0 < y1
struct Extent { double lo, hi; };         // of a feature's x, widened by the rounding of xi (see extents)

// the least and the greatest value of an integer dtype of a zone raster
inline void int_range(int dtype, int64_t* lo, int64_t* hi) {
  fra_region::with_int_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    *lo = (int64_t)std::numeric_limits<T>::lowest(), *hi = (int64_t)std::numeric_limits<T>::max();
  });
}

// FRA_E_INVALID for a job the rule refuses, in the header's order (after the null arguments)
inline int check_job(const fra_rasterize_job* j) {
  if (!fra_region::is_int_dtype(j->dtype))
    return fra_internal_set_error(FRA_E_INVALID, "bad output dtype %d (an integer dtype of at most 32 bits)", j->dtype);
  if (j->height < 1 || j->height > kMaxSide || j->width < 1 || j->width > kMaxSide)
    return fra_internal_set_error(FRA_E_INVALID, "the output size must be 1 .. %d in each dimension (got %d x %d)", kMaxSide,
                                  j->height, j->width);
  if (j->row_stride < 0 || j->col_stride < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad output layout (strides %lld, %lld)", (long long)j->row_stride,
                                  (long long)j->col_stride);
  if (j->nfeatures < 0 || j->nrings < 0 || j->nverts < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad geometry tables (%d features, %lld rings, %lld vertices)", j->nfeatures,
                                  (long long)j->nrings, (long long)j->nverts);
  if (j->nfeatures) {
    const int64_t* fr = j->feature_ring_start;
    bool ok = fr[0] == 0 && fr[j->nfeatures] == j->nrings;
    for (int32_t f = 0; f < j->nfeatures && ok; f++) ok = fr[f] <= fr[f + 1];
    if (!ok) return fra_internal_set_error(FRA_E_INVALID, "bad geometry tables (feature_ring_start is not 0 ... nrings, ascending)");
  } else if (j->nrings) {
    return fra_internal_set_error(FRA_E_INVALID, "bad geometry tables (%lld rings of no feature)", (long long)j->nrings);
  }
  if (j->nrings) {
    const int64_t* rs = j->ring_start;
    bool ok = rs[0] == 0 && rs[j->nrings] <= j->nverts;
    for (int64_t r = 0; r < j->nrings && ok; r++) ok = rs[r] <= rs[r + 1];
    if (!ok) return fra_internal_set_error(FRA_E_INVALID, "bad geometry tables (ring_start is not ascending from 0 within the vertices)");
    for (int64_t r = 0; r < j->nrings; r++)
      if (rs[r + 1] - rs[r] < 3)
        return fra_internal_set_error(FRA_E_INVALID, "ring %lld has %lld vertices (at least 3 are needed)", (long long)r,
                                      (long long)(rs[r + 1] - rs[r]));
    for (int64_t i = 0, n = 2 * rs[j->nrings]; i < n; i++)
      if (!(std::fabs(j->xy[i]) <= kMaxCoord))  // (a NaN fails every comparison)
        return fra_internal_set_error(FRA_E_INVALID, "coordinate %lld is not finite or above 2^52 in magnitude", (long long)i);
  }
  int64_t lo = 0, hi = 0;
  int_range(j->dtype, &lo, &hi);
  for (int32_t f = 0; f < j->nfeatures; f++)
    if (j->values[f] < lo || j->values[f] > hi)
      return fra_internal_set_error(FRA_E_INVALID, "burn value %lld of feature %d is not a value of the output dtype",
                                    (long long)j->values[f], f);
  if (j->fill < lo || j->fill > hi)
    return fra_internal_set_error(FRA_E_INVALID, "fill %lld is not a value of the output dtype", (long long)j->fill);
  if (j->nfeatures > kMaxFeatures)
    return fra_internal_set_error(FRA_E_INVALID, "%d features: at most 2^24 go into one call", j->nfeatures);
  if (j->nverts > kMaxVerts)
    return fra_internal_set_error(FRA_E_INVALID, "%lld vertices: at most 2^28 go into one call", (long long)j->nverts);
  return FRA_OK;
}

// the canonical edges of a checked job, in feature, ring and vertex order, and the feature of each
inline void build_edges(const fra_rasterize_job* j, std::vector<Edge>* edges, std::vector<int32_t>* feat) {
  edges->clear(), feat->clear();
  for (int32_t f = 0; f < j->nfeatures; f++)
    for (int64_t r = j->feature_ring_start[f]; r < j->feature_ring_start[f + 1]; r++) {
      const int64_t a = j->ring_start[r], n = j->ring_start[r + 1] - a;
      for (int64_t i = 0; i < n; i++) {
        const double* p = j->xy + 2 * (a + i);
        const double* q = j->xy + 2 * (a + (i + 1 == n ? 0 : i + 1));  // the ring closes on its first vertex
        if (p[1] == q[1]) continue;                                      // level, or of no length
        edges->push_back(p[1] < q[1] ? Edge{p[0], p[1], q[0], q[1]} : Edge{q[0], q[1], p[0], p[1]});
        feat->push_back(f);
      }
    }
}

// Per feature, an interval that holds every xi of its edges: the hull of their x, widened by 2^-50 of its larger
// magnitude.  (xi = x0 + t (x1 - x0) with 0 <= t <= 1 lies between x0 and fl(x0 + fl(x1 - x0)) by the monotonicity of
// rounding, and that is within 2^-51 max(|x0|, |x1|) of x1.)  A feature without an edge gets [inf, -inf].
inline void extents(const std::vector<Edge>& edges, const std::vector<int32_t>& feat, int32_t nfeatures, std::vector<Extent>* ext) {
  ext->assign((size_t)nfeatures, Extent{HUGE_VAL, -HUGE_VAL});
  for (size_t k = 0; k < edges.size(); k++) {
    Extent& e = (*ext)[(size_t)feat[k]];
    e.lo = std::min(e.lo, std::min(edges[k].x0, edges[k].x1));
    e.hi = std::max(e.hi, std::max(edges[k].x0, edges[k].x1));
  }
  for (Extent& e : *ext)
    if (e.lo <= e.hi) {
      const double m = std::max(std::fabs(e.lo), std::fabs(e.hi)) * 0x1p-50;
      e.lo -= m, e.hi += m;
    }
}

// The rows of the window whose centres an edge's [y0, y1) contains, as [*first, *last] relative to the window; false
// when there is none.  Row R has the centre R + 0.5, so y0 <= R + 0.5 < y1 is ceil(y0 - 0.5) <= R <= ceil(y1 - 0.5) - 1
// (y - 0.5 is exact up to 2^52).
inline bool edge_rows(const Edge& e, int64_t row_off, int32_t h, int64_t* first, int64_t* last) {
  const double lo = std::max(std::ceil(e.y0 - 0.5), (double)row_off);
  const double hi = std::min(std::ceil(e.y1 - 0.5) - 1.0, (double)row_off + (double)(h - 1));
  if (!(lo <= hi)) return false;
  *first = (int64_t)(lo - (double)row_off), *last = (int64_t)(hi - (double)row_off);
  return true;
}

// The edges of every band of kBandRows output rows as one list in the edges' own order: band b holds
// binned[band_start[b] .. band_start[b + 1]).  FRA_E_NOMEM when the lists together pass kMaxBinned entries.
struct Bins {
  std::vector<uint32_t> band_start;  // nbands + 1
  std::vector<Edge> edges;
  std::vector<int32_t> feat;
};
inline int bin_edges(const std::vector<Edge>& edges, const std::vector<int32_t>& feat, int64_t row_off, int32_t h, Bins* b) {
  const int64_t nbands = ((int64_t)h + kBandRows - 1) / kBandRows;
  std::vector<int64_t> count((size_t)nbands + 1, 0);
  for (const Edge& e : edges) {
    int64_t r0, r1;
    if (!edge_rows(e, row_off, h, &r0, &r1)) continue;
    for (int64_t k = r0 / kBandRows; k <= r1 / kBandRows; k++) count[(size_t)k + 1]++;
  }
  for (int64_t k = 0; k < nbands; k++) count[(size_t)k + 1] += count[(size_t)k];
  if (count[(size_t)nbands] > kMaxBinned)
    return fra_internal_set_error(FRA_E_NOMEM, "the band lists hold %lld edges (at most 2^31 - 1)", (long long)count[(size_t)nbands]);
  b->band_start.assign(count.begin(), count.end());
  b->edges.resize((size_t)count[(size_t)nbands]);
  b->feat.resize((size_t)count[(size_t)nbands]);
  std::vector<int64_t> at(count.begin(), count.end() - 1);
  for (size_t i = 0; i < edges.size(); i++) {
    int64_t r0, r1;
    if (!edge_rows(edges[i], row_off, h, &r0, &r1)) continue;
    for (int64_t k = r0 / kBandRows; k <= r1 / kBandRows; k++) {
      const size_t slot = (size_t)at[(size_t)k]++;
      b->edges[slot] = edges[i], b->feat[slot] = feat[i];
    }
  }
  return FRA_OK;
}

// everything the kernel takes from a checked job; FRA_E_NOMEM when the host runs out of memory
struct Prepared {
  Bins bins;
  std::vector<Extent> ext;
  std::vector<uint32_t> values;  // the low 32 bits of every burn value: the output dtype's own bits
};
inline int prepare(const fra_rasterize_job* j, Prepared* p) {
  try {
    std::vector<Edge> edges;
    std::vector<int32_t> feat;
    build_edges(j, &edges, &feat);
    extents(edges, feat, j->nfeatures, &p->ext);
    p->values.resize((size_t)j->nfeatures);
    for (int32_t f = 0; f < j->nfeatures; f++) p->values[(size_t)f] = (uint32_t)(uint64_t)j->values[f];
    return bin_edges(edges, feat, j->row_off, j->height, &p->bins);
  } catch (const std::bad_alloc&) {
    return fra_internal_set_error(FRA_E_NOMEM, "out of host memory for the edge table");
  }
}

}  // namespace fra_rz
