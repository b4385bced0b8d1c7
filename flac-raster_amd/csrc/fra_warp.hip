// fra_warp.hip -- warped reads: a raster onto an output grid of its own through an affine map or a coordinate grid
// (fra_warp), and a set of tile streams likewise, only the source window the map touches being decoded and nothing but
// the output leaving the GPU (fra_decode_device_warped).  The third unit over fra_region.h that maps a raster, and the
// first whose reads depend on data: a 2-D gather.
//
// The rule (include/flac_raster_amd.h, "Warped reads"; flac_raster/warp.py: warp_arrays is the reference the kernel is
// checked against bit for bit): u = C + 0.5, v = R + 0.5; AFFINE x = (a u + b v) + c, y = (d u + e v) + f; GRID the
// bilinear patch of the cell (min(C / step, gw - 2), min(R / step, gh - 2)); inside when 0 <= x < W and 0 <= y < H, else
// fill; nearest in[floor(y)][floor(x)]; bilinear and cubic about px = x - 0.5 with the resampling rule's taps, weights,
// clamping, order and conversion; with a nodata value the nodata-aware rule's masked bilinear (fra_resample.h:
// combine_taps, which the resampling kernel calls too; the conversion of a NaN and the fill are the warp's own).
//
// k_warp<T, MODE, MASKED>: a workgroup owns a tile of kTH x kTW = 16 x 64 output pixels of one band; wave w owns the tile
// rows w, w + 4, w + 8, w + 12 and a lane one column, so a wave stores 64 neighbouring pixels and, under a map close to a
// translation, its lanes read neighbouring source pixels.  Every thread computes the source coordinates of its pixels
// and reads its taps straight from global memory: the gather.  Neighbouring pixels share their taps through the vector
// L1 and the L2, and that is enough: a second path that reduced the tile's bounding box of taps, staged it in LDS with
// coalesced 16-byte row loads and read every tap from there was built, measured and deleted -- over the 4 x 10980^2
// uint16 scene it took 2.22 ms against 1.94 ms for a 10 degree rotation (bilinear), and lost for a shift, for the
// Mercator grid and for the nearest as well (DESIGN 6c has the table).
//   The counters.  The fill count as k_resample_masked's: summed over the workgroup (fra_region.h: wg_sum), one
//   atomicAdd per workgroup that has any into the band's word.  One 64-bit vector atomic add per workgroup into the gathered counter, which is kept in
//   kShards words on lines of their own and summed by the host: with one word the 472,656 adds of that scene took 3.8 of
//   the kernel's 6.0 ms (a word takes about 88 adds per microsecond).  fra_warp_paths reports 0 staged workgroups.
// Memory safety does not rest on the host's window arithmetic: a tap index is clamped to the region after it is
// clamped to the raster, so no coordinate, finite or not, leads outside the source.  All offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"
#include "fra_resample.h"
#include "fra_warp.h"

static_assert(sizeof(fra_warp_map) == 80 && sizeof(fra_warp_job) == 208, "the warp's structures, as the header says");

namespace {

using namespace fra_region;
using namespace fra_rs;
using namespace fra_wp;

constexpr int kTH = 16, kTW = 64;  // the tile: 4 waves x 4 rows of 64 pixels
constexpr int kP = 4;              // pixels of a thread, 4 tile rows apart
constexpr int kShards = 256;       // words of the workgroup counter
constexpr int kShardStride = 16;   // ... 128 bytes apart

struct WarpArgs {
  const void* src;  // the region's element (band 0, row 0, col 0)
  void* dst;
  int64_t sbs, srs, scs;  // source element strides: band, row, column
  int64_t dbs, drs, dcs;  // destination element strides
  const double* gx;       // GRID: the planes on the device
  const double* gy;
  unsigned long long* filled;  // one word per band, zeroed by the host
  unsigned long long* gathered;  // the workgroups: kShards words, kShardStride apart, zeroed by the host
  double m[6];                 // AFFINE
  double nodata, fill;
  double inv_step;             // GRID: 1 / step when step is a power of two (exact), else 0
  int32_t H, W;                // the whole raster
  int32_t row0, col0, rh, rw;  // the region of it the source holds
  int32_t oh, ow;
  int32_t kind, step, gh, gw;
  uint32_t tiles_x, ntiles;    // tiles across the output, and in all
};

// tap i along an axis of n raster pixels as an index into the region [off, off + len) of it: clamped to the raster (the
// rule), then to the region (which holds every tap when the host's window is right; memory safety when it is not)
__device__ inline int32_t tap_at(int32_t i, int32_t n, int32_t off, int32_t len) {
  return min(max(min(max(i, 0), n - 1) - off, 0), len - 1);
}

// the source coordinates of output pixel (R, C)
__device__ inline void coords(const WarpArgs& a, int32_t R, int32_t C, double* x, double* y) {
  const double u = (double)C + 0.5, v = (double)R + 0.5;
  if (a.kind == FRA_WARP_AFFINE) {
    *x = (a.m[0] * u + a.m[1] * v) + a.m[2];
    *y = (a.m[3] * u + a.m[4] * v) + a.m[5];
  } else {
    const int32_t cj = min(C / a.step, a.gw - 2), ci = min(R / a.step, a.gh - 2);
    // (a power-of-two step, fit_grid's kind: the product with its reciprocal is the quotient, bit for bit, and several
    // times shorter than an f64 division; the branch is uniform)
    const double du = u - (double)(cj * a.step), dv = v - (double)(ci * a.step);
    const double fx = a.inv_step != 0.0 ? du * a.inv_step : du / (double)a.step;
    const double fy = a.inv_step != 0.0 ? dv * a.inv_step : dv / (double)a.step;
    const int64_t at = (int64_t)ci * a.gw + cj;
    auto patch = [&](const double* __restrict__ g) {
      const double g00 = g[at], g01 = g[at + 1], g10 = g[at + a.gw], g11 = g[at + a.gw + 1];
      const double top = g00 + (g01 - g00) * fx;
      const double bot = g10 + (g11 - g10) * fx;
      return top + (bot - top) * fy;
    };
    *x = patch(a.gx);
    *y = patch(a.gy);
  }
}

// the rule's conversion of a result: the resampling's (fra_resample.h: from_f64), a NaN as the canonical quiet NaN
template <typename T>
__device__ inline T result_of(double v) {
  if constexpr (std::is_floating_point<T>::value) return (T)(v != v ? __longlong_as_double(0x7ff8000000000000ll) : v);
  else return from_f64<T>(v);
}

// the first tap and the fraction along one axis: nearest floor(x), t unused; else i0 = floor(x - 0.5), t = (x - 0.5) - i0
template <int MODE>
__device__ inline int32_t first_tap(double x, double* t) {
  if constexpr (MODE == FRA_RESAMPLE_NEAREST) {
    *t = 0.0;
    return (int32_t)floor(x);
  } else {
    const double p = x - 0.5, f = floor(p);
    *t = p - f;
    return (int32_t)f + (MODE == FRA_RESAMPLE_CUBIC ? -1 : 0);
  }
}

// The value of an inside pixel at (x, y); fetch(r, c) reads region element (r, c).  *nfill is raised when the pixel is
// to be counted (it got the fill, or the nearest picked an invalid pixel).
template <typename T, int MODE, bool MASKED, typename Fetch>
__device__ inline T sample(const WarpArgs& a, double x, double y, T nd, T fillv, Fetch&& fetch, uint32_t* nfill) {
  double ty, tx;
  const int32_t fy = first_tap<MODE>(y, &ty), fx = first_tap<MODE>(x, &tx);
  if constexpr (MODE == FRA_RESAMPLE_NEAREST) {
    const T v = fetch(tap_at(fy, a.H, a.row0, a.rh), tap_at(fx, a.W, a.col0, a.rw));
    if constexpr (MASKED) *nfill += invalid(v, nd) ? 1u : 0u;
    return v;
  } else {
    constexpr int NT = kTaps<MODE>;
    T xv[NT][NT];  // [j][i]: tap row j, tap column i
    int32_t cols[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) cols[i] = tap_at(fx + i, a.W, a.col0, a.rw);
#pragma unroll
    for (int j = 0; j < NT; j++) {
      const int32_t r = tap_at(fy + j, a.H, a.row0, a.rh);
#pragma unroll
      for (int i = 0; i < NT; i++) xv[j][i] = fetch(r, cols[i]);
    }
    return combine_taps<T, MODE, MASKED, result_of<T>>(xv, ty, tx, nd, fillv, nfill);
  }
}

template <typename T, int MODE, bool MASKED>
__global__ void __launch_bounds__(256) k_warp(WarpArgs a) {
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t band = blockIdx.y;
  const uint32_t tile_id = blockIdx.z * gridDim.x + blockIdx.x;
  if (tile_id >= a.ntiles) return;  // (the whole workgroup: the last slice of the grid)
  const int32_t orow0 = (int32_t)(tile_id / a.tiles_x) * kTH;  // the tile's origin in the output
  const int32_t ocol0 = (int32_t)(tile_id % a.tiles_x) * kTW;
  const T* __restrict__ const ps = (const T*)a.src + (int64_t)band * a.sbs;
  T* __restrict__ const pd = (T*)a.dst + (int64_t)band * a.dbs;
  const T nd = (T)a.nodata, fillv = (T)a.fill;
  const int32_t C = ocol0 + (int32_t)lane;
  auto fetch = [&](int32_t r, int32_t c) { return ps[(int64_t)r * a.srs + (int64_t)c * a.scs]; };
  uint32_t nfill = 0;
#pragma unroll
  for (int p = 0; p < kP; p++) {
    const int32_t R = orow0 + (int32_t)wave + 4 * p;
    if (R < a.oh && C < a.ow) {
      double x, y;
      coords(a, R, C, &x, &y);
      T o = fillv;
      if (x >= 0.0 && x < (double)a.W && y >= 0.0 && y < (double)a.H) o = sample<T, MODE, MASKED>(a, x, y, nd, fillv, fetch, &nfill);
      else nfill++;
      pd[(int64_t)R * a.drs + (int64_t)C * a.dcs] = o;
    }
  }
  // the counters: the workgroup's fill count into its band's word, and the workgroup itself into its shard
  const uint32_t total = wg_sum(nfill);
  if (tid == 0) {
    if (total) atomicAdd(&a.filled[band], (unsigned long long)total);
    atomicAdd(&a.gathered[((tile_id + band) % (uint32_t)kShards) * kShardStride], 1ull);
  }
}

thread_local float g_warp_ms = 0.f;
thread_local uint64_t g_warp_paths[2] = {0, 0};

template <typename T>
void launch_t(int mode, bool masked, dim3 grid, hipStream_t s, const WarpArgs& a) {
  switch (mode) {
    case FRA_RESAMPLE_NEAREST:
      if (masked) hipLaunchKernelGGL((k_warp<T, 0, true>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_warp<T, 0, false>), grid, dim3(256), 0, s, a);
      break;
    case FRA_RESAMPLE_BILINEAR:
      if (masked) hipLaunchKernelGGL((k_warp<T, 2, true>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_warp<T, 2, false>), grid, dim3(256), 0, s, a);
      break;
    default:
      if (masked) hipLaunchKernelGGL((k_warp<T, 3, true>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_warp<T, 3, false>), grid, dim3(256), 0, s, a);
      break;
  }
}

// what a warp asks for beside its source and destination, checked
struct WarpSpec {
  const fra_warp_map* map;
  int32_t oh, ow, resampling, flags;
  double nodata, fill;
};

// k_warp over `io`, whose source is the `region` of an H x W raster (a null source: no pixel is inside), timed; the
// fill counts to `filled` (channels words, may be null) and the destination copied back
int run_warp(Call& c, const Io& io, int dtype, int32_t channels, int32_t H, int32_t W, const fra_window& region,
             const WarpSpec& w, uint64_t* filled) {
  WarpArgs a{};
  a.src = io.src, a.dst = io.out.dev;
  a.sbs = io.ss.band, a.srs = io.ss.row, a.scs = io.ss.col;
  a.dbs = io.ds.band, a.drs = io.ds.row, a.dcs = io.ds.col;
  a.nodata = w.nodata, a.fill = w.fill;
  a.H = H, a.W = W;
  a.row0 = region.row_off, a.col0 = region.col_off, a.rh = region.height, a.rw = region.width;
  a.oh = w.oh, a.ow = w.ow;
  a.kind = w.map->kind;
  if (a.kind == FRA_WARP_AFFINE) {
    std::memcpy(a.m, w.map->affine, sizeof(a.m));
  } else {
    a.step = w.map->step, a.gh = w.map->gh, a.gw = w.map->gw;
    a.inv_step = (a.step & (a.step - 1)) == 0 ? 1.0 / (double)a.step : 0.0;
    const size_t plane = (size_t)a.gh * (size_t)a.gw * sizeof(double);
    double* d = nullptr;
    HIPCHK(c.sc.alloc(&d, 2 * plane));
    HIPCHK(hipMemcpyAsync(d, w.map->gx, plane, hipMemcpyHostToDevice, c.s));
    HIPCHK(hipMemcpyAsync((char*)d + plane, w.map->gy, plane, hipMemcpyHostToDevice, c.s));
    a.gx = d, a.gy = (const double*)((const char*)d + plane);
  }
  constexpr size_t kPathWords = (size_t)kShards * kShardStride;
  const size_t head = ((size_t)channels + kShardStride - 1) / kShardStride * kShardStride;  // the shards start on a line of their own
  const size_t words = head + kPathWords;
  HIPCHK(c.sc.alloc(&a.filled, words * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(a.filled, 0, words * sizeof(unsigned long long), c.s));
  a.gathered = a.filled + head;
  const int64_t tiles_x = ((int64_t)w.ow + kTW - 1) / kTW, tiles_y = ((int64_t)w.oh + kTH - 1) / kTH;
  // at most 2^32 output pixels: 2^22 tiles, in slices of 2^20 so that a grid dimension's threads stay in 32 bits
  const int64_t ntiles = tiles_x * tiles_y, slice = std::min<int64_t>(ntiles, (int64_t)1 << 20);
  a.tiles_x = (uint32_t)tiles_x, a.ntiles = (uint32_t)ntiles;
  const dim3 grid((unsigned)slice, (unsigned)channels, (unsigned)((ntiles + slice - 1) / slice));
  const bool masked = (w.flags & FRA_WARP_NODATA) != 0;
  std::vector<unsigned long long> counts(words);
  const int rc = timed(
      c, &g_warp_ms,
      [&]() -> int {
        with_dtype(dtype, [&](auto t) { launch_t<decltype(t)>(w.resampling, masked, grid, c.s, a); });
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&]() -> int {
        HIPCHK(hipMemcpyAsync(counts.data(), a.filled, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.s));
        return copy_back(c, io.out);
      });
  if (rc) return rc;
  if (filled)
    for (int k = 0; k < channels; k++) filled[k] = (uint64_t)counts[k];
  uint64_t n = 0;
  for (int i = 0; i < kShards; i++) n += (uint64_t)counts[head + (size_t)i * kShardStride];
  g_warp_paths[0] = 0, g_warp_paths[1] = n;  // (no workgroup stages its taps: see the top of the file)
  return FRA_OK;
}

// the refusals that need the dtype: nodata (under FRA_WARP_NODATA) and fill
int check_values(int32_t flags, double nodata, double fill, int dtype) {
  if (flags & FRA_WARP_NODATA)
    if (const int rc = check_nodata(nodata, dtype)) return rc;
  return check_nodata(fill, dtype, "fill");
}

}  // namespace

extern "C" {

FRA_API int fra_warp_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_warp_ms;
  return FRA_OK;
}

FRA_API int fra_warp_paths(uint64_t counts[2]) {
  if (!counts) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  counts[0] = g_warp_paths[0], counts[1] = g_warp_paths[1];
  return FRA_OK;
}

FRA_API int fra_warp_source_window(const fra_warp_map* map, int32_t raster_h, int32_t raster_w, int32_t out_h, int32_t out_w,
                                   fra_window* window) {
  if (!map || !window) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (const int rc = check_out(out_h, out_w, FRA_RESAMPLE_NEAREST, 0)) return rc;
  if (const int rc = check_map(map, out_h, out_w)) return rc;
  if (raster_h < 1 || raster_w < 1) return fra_internal_set_error(FRA_E_INVALID, "bad raster size (%d x %d)", raster_h, raster_w);
  return source_window(*map, raster_h, raster_w, out_h, out_w, window) ? 1 : 0;
}

FRA_API int fra_warp(fra_ctx* ctx, const fra_warp_job* job, uint64_t* filled) {
  if (!ctx || !job || !job->src || !job->dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  RasterJob r = raster_job(*job);
  if (const int rc = check_raster(r)) return rc;
  if (r.channels > 255) return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d bands, more than 255)", r.channels);
  const WarpSpec w{&job->map, job->out_height, job->out_width, job->resampling, job->flags, job->nodata, job->fill};
  if (const int rc = check_out(w.oh, w.ow, w.resampling, w.flags)) return rc;
  if (const int rc = check_map(w.map, w.oh, w.ow)) return rc;
  if (const int rc = check_values(w.flags, w.nodata, w.fill, r.dtype)) return rc;
  r.oh = w.oh, r.ow = w.ow;
  return run_raster(ctx, r, [&](Call& c, const Io& io) {
    return run_warp(c, io, r.dtype, r.channels, r.h, r.w, fra_window{0, 0, r.h, r.w}, w, filled);
  });
}

FRA_API int fra_decode_device_warped(fra_ctx* ctx, const fra_decode_job* job, int32_t raster_h, int32_t raster_w,
                                     const fra_warp_map* map, int32_t out_h, int32_t out_w, int32_t resampling, int32_t flags,
                                     double nodata, double fill, fra_decoded* infos, uint64_t* filled) {
  if (!ctx || !job || !map || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  const WarpSpec w{map, out_h, out_w, resampling, flags, nodata, fill};
  if (const int rc = check_out(out_h, out_w, resampling, flags)) return rc;
  if (const int rc = check_map(map, out_h, out_w)) return rc;
  if (raster_h < 1 || raster_w < 1) return fra_internal_set_error(FRA_E_INVALID, "bad raster size (%d x %d)", raster_h, raster_w);
  fra_window roi{0, 0, 1, 1};  // (what the windowed read's refusals are asked about when nothing is to be decoded)
  const bool touches = source_window(*map, raster_h, raster_w, out_h, out_w, &roi);
  if (left_to_window_read(job, &roi)) return refer_to_window_read(ctx, job, &roi, infos, false);
  if (const int rc = check_values(flags, nodata, fill, job->dst_dtype)) return rc;
  if (!touches) {  // every pixel is outside: the kernel reads no source
    for (int i = 0; i < job->nitems; i++) infos[i] = fra_decoded{};
    Call c(ctx);
    Io io{nullptr, Strides{0, 0, 1}, {}, Strides{job->band_stride, job->row_stride, job->col_stride}};
    if (const int rc = stage_out(c, job->dst, job->dst_on_device,
                                 (size_t)extent_of(job->channels, out_h, out_w, io.ds) * (size_t)elem_size(job->dst_dtype), &io.out))
      return rc;
    return run_warp(c, io, job->dst_dtype, job->channels, raster_h, raster_w, fra_window{0, 0, 1, 1}, w, filled);
  }
  if (const int rc = check_cover(job, &roi)) return rc;
  return run_region(ctx, job, &roi, infos, out_h, out_w, [&](Call& c, const Io& io) {
    return run_warp(c, io, job->dst_dtype, job->channels, raster_h, raster_w, roi, w, filled);
  });
}

}  // extern "C"
