// fra_verify.h -- the verify entry of the device decoder (fra_decode_dev.hip), shared with fra_plan.hip, which builds
// its arguments from a plan (fra_plan_verify), and with tools/decode_host_check.cpp.  Host only; not part of the ABI.
#pragma once
#include <cstdint>

#include "../../include/flac_raster_amd.h"

static_assert(sizeof(fra_verify_report) == 32, "fra_verify_report is 32 bytes in the ABI");

// the raster the decoded samples are compared with, on the device
struct fra_verify_source {
  const void* raster;  // element (band 0, row 0, col 0)
  int32_t dtype;       // fra_dtype
  int32_t norm;        // fra_job.norm: 0 raw int16 / int32 samples, 16 / 24 normalize_to_audio
  int64_t band_stride, row_stride, col_stride;  // elements
  const void* norm_rows;  // device, one fra::NormDev per item (the plan's own rows of its last execute)
};

// Decodes the items' frames as fra_decode_device does on the offsets path (every item needs frame_offsets, `data` is
// a device pointer) and compares every sample with the normalised source element of its window position
// (k_dec_verify) instead of storing it.  first_frames (may be null: 0 everywhere): the stream's frame number of item
// i's first frame -- frame f of the item holds samples from (first_frames[i] + f) * blocksize of the window.
// reports[i] / *bad_windows as fra_plan_verify.  Arguments are validated before any GPU work.
extern "C" int fra_internal_verify_device(fra_ctx* ctx, const uint8_t* data, uint64_t len, const fra_decode_item* items,
                                          int32_t nitems, int32_t channels, const fra_verify_source* src,
                                          const int32_t* first_frames, fra_verify_report* reports,
                                          int32_t* bad_windows);
