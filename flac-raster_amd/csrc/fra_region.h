// fra_region.h -- what the reads that reduce a decoded region on the device share (fra_decimate.hip, fra_resample.hip,
// fra_compare.hip, fra_stats.hip): the check that the items cover the region, and the windowed read (fra_decode_device_window, called as
// any caller would: same kernels, refusals and messages) into a per-call device buffer of the region.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"

namespace fra_region {

// FRA_E_INVALID unless the intersections of the items with roi add up to roi's area (the item windows and roi are
// non-negative: the caller has left everything else to the windowed read)
inline int check_cover(const fra_decode_job* job, const fra_window* roi) {
  const int64_t h = roi->height, w = roi->width;
  int64_t covered = 0;
  for (int i = 0; i < job->nitems; i++) {
    const fra_window& t = job->items[i].window;
    const int64_t ra = std::max<int64_t>(t.row_off, roi->row_off);
    const int64_t rb = std::min<int64_t>((int64_t)t.row_off + t.height, (int64_t)roi->row_off + h);
    const int64_t ca = std::max<int64_t>(t.col_off, roi->col_off);
    const int64_t cb = std::min<int64_t>((int64_t)t.col_off + t.width, (int64_t)roi->col_off + w);
    if (rb > ra && cb > ca) covered += (rb - ra) * (cb - ca);
  }
  if (covered != h * w)
    return fra_internal_set_error(FRA_E_INVALID, "the items do not cover the region (%lld of its %lld pixels)",
                                  (long long)covered, (long long)(h * w));
  return FRA_OK;
}

// a non-negative item window everywhere (what is not is the windowed read's to refuse)
inline bool item_windows_ok(const fra_decode_job* job) {
  for (int i = 0; i < job->nitems; i++) {
    const fra_window& w = job->items[i].window;
    if (w.height < 0 || w.width < 0 || w.row_off < 0 || w.col_off < 0) return false;
  }
  return true;
}

#ifdef __HIPCC__
// roi at full resolution in job->dst_dtype into device memory of `sc`: band-planar, rows of *row_stride elements that
// start on 16-byte boundaries (for the vector loads of the kernel that follows), bands of roi->height rows.  The job's
// own dst and strides are not looked at.  Synchronous; the windowed read's scratch is gone on return.
inline int decode(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, fra_decoded* infos, HipArena& sc,
                  void** d_region, int64_t* row_stride) {
  const int64_t h = roi->height, w = roi->width;
  const size_t es = (size_t)elem_size(job->dst_dtype);
  const int64_t vlen = 16 / (int64_t)es;
  const int64_t rs = (w + vlen - 1) / vlen * vlen;
  HIPCHK(sc.alloc(d_region, (size_t)job->channels * (size_t)(h * rs) * es));
  fra_decode_job inner = *job;
  inner.dst = *d_region;
  inner.dst_on_device = 1;
  inner.band_stride = h * rs;
  inner.row_stride = rs;
  inner.col_stride = 1;
  *row_stride = rs;
  return fra_decode_device_window(ctx, &inner, roi, infos);
}
#endif

}  // namespace fra_region
