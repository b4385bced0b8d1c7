// fra_rasterize.hip -- polygon features burned into an integer raster on the GPU (fra_rasterize): zones and masks from
// vector geometry, born on the device so that they can go to k_zonal without visiting the host.  The tenth unit over
// fra_region.h, and the first whose input is not a raster.
//
// The rule (include/flac_raster_amd.h, "Rasterizing polygons"; flac_raster/rasterize.py: rasterize_arrays is the
// reference the kernel is checked against byte for byte).  All arithmetic is IEEE f64, every operation rounded on its
// own.  Pixel (r, c) of the window has the centre xc = (double)(col_off + c) + 0.5, yc = (double)(row_off + r) + 0.5.
// A ring is closed implicitly; an edge with y0 == y1 is dropped; every other edge is oriented y0 < y1 before any
// arithmetic.  An edge crosses the scanline of yc when y0 <= yc && yc < y1; then t = (yc - y0) / (y1 - y0),
// xi = x0 + t * (x1 - x0), and it counts for the pixel when xi > xc.  A feature covers the pixel when an odd number of
// its edges count, over all its rings; the pixel gets the burn value of the covering feature with the highest index,
// or the fill.  *burned: the pixels covered by any feature.
//
// The host (fra_rasterize.h) builds the edge table and one list of edges per band of 16 output rows, in the edges' own
// order, and a widened x-extent per feature.  k_rasterize<T>: one 256-thread workgroup per 16 x 64 output tile; thread
// t owns the 4 neighbouring pixels (t & 15) * 4 ... of tile row t >> 4.  The workgroup walks its band's list in chunks
// of kChunk edges.  Phase A: the threads compute xi once per (edge of the chunk, row of the tile) into LDS, -inf where
// the edge does not cross the row -- the f64 division is the dear instruction and is not repeated per pixel; an edge
// of a feature whose extent lies wholly left of the tile's centres counts for none of them and one wholly right for
// all of them, an even number of times per row, so both get -inf without the division.  Phase B: every thread walks
// its row's xi and toggles 4 parity bits by xi > xc (the 16 lanes of a row read the same word: a broadcast; the rows
// of a wave lie kRowStride doubles apart, 4 banks from one another), four edges per round of LDS reads, and tests its
// least centre first: a wave skips the edges that do not concern it.  Where the feature index changes -- the same
// place for every thread -- the pixels of odd parity take the feature's value and the parity is cleared; parity,
// values and the pending feature live in registers across the chunks.  A band without edges: the loop does not run
// and the tile is the fill.  The covered pixels are counted per workgroup into a word of its own, and k_rasterize_fold
// adds 4096 of those per workgroup for the host to finish: no word is shared by the workgroups.
// Memory safety: a tile reads band_start[its band .. + 1] and the entries between them; ext and values are indexed by
// the feature indices the host wrote; stores are guarded by the window.  All offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_rasterize.h"
#include "fra_region.h"

static_assert(sizeof(fra_rasterize_job) == 128, "the rasterizer's job, as the header says");

namespace {

using namespace fra_region;
using namespace fra_rz;

constexpr int kTH = kBandRows, kTW = 64;  // the tile: 16 rows of 16 threads x 4 pixels
constexpr int kPix = 4;
#ifndef FRA_RZ_CHUNK
#define FRA_RZ_CHUNK 128
#endif
// edges per chunk: 16 x kChunk x 8 bytes of LDS, 16.5 KiB at 128, so that 8 workgroups share a CU; 256 halves that and
// measured 1.6 times slower, 64 the same
constexpr int kChunk = FRA_RZ_CHUNK;
constexpr int kRowStride = kChunk + 2;    // doubles between the rows of s_xi: 16-byte aligned, 4 banks apart
constexpr int kFold = 4096;               // partial counts a workgroup of the fold adds
static_assert(kChunk >= 16 && (kChunk & (kChunk - 1)) == 0, "kChunk is a power of two");

struct RzArgs {
  const Edge* edges;            // the band lists
  const int32_t* feat;          // ... the feature of every entry
  const uint32_t* band_start;   // nbands + 1
  const Extent* ext;            // per feature
  const uint32_t* values;       // per feature: the output dtype's bits
  void* dst;
  uint32_t* partial;            // one word per tile
  int64_t row_off, col_off, drs, dcs;
  int32_t h, w;
  uint32_t fill;
  int32_t vec;                  // rows of 4-pixel vector stores are aligned
};

template <typename T>
__global__ void __launch_bounds__(256) k_rasterize(RzArgs a) {
  __shared__ alignas(16) double s_xi[kTH * kRowStride];
  __shared__ alignas(16) int32_t s_feat[kChunk];
  const uint32_t tid = threadIdx.x;
  const int32_t trow = (int32_t)(tid >> 4), r0 = (int32_t)blockIdx.y * kTH, c0 = (int32_t)blockIdx.x * kTW;
  const int32_t R = r0 + trow, C = c0 + (int32_t)(tid & 15u) * kPix;
  const uint32_t e_lo = a.band_start[blockIdx.y], e_hi = a.band_start[blockIdx.y + 1];
  double xc[kPix];
#pragma unroll
  for (int p = 0; p < kPix; p++) xc[p] = (double)(a.col_off + C + p) + 0.5;
  const double xc_first = (double)(a.col_off + c0) + 0.5;
  const double xc_last = (double)(a.col_off + min(c0 + kTW, a.w) - 1) + 0.5;
  uint32_t par = 0, cov = 0, val[kPix] = {0, 0, 0, 0};
  int32_t cur = -1;  // the feature the parity belongs to
  auto commit = [&]() {
    if (par) {
      const uint32_t v = a.values[cur];
#pragma unroll
      for (int p = 0; p < kPix; p++) val[p] = (par >> p & 1u) ? v : val[p];
      cov |= par;
      par = 0;
    }
  };
  for (uint32_t e0 = e_lo; e0 < e_hi; e0 += (uint32_t)kChunk) {
    const uint32_t n = min((uint32_t)kChunk, e_hi - e0);
    // phase A: xi of every (edge, row) once; G groups of threads share the rows when the chunk is shorter than 256
    constexpr int G = kChunk >= 256 ? 1 : 256 / kChunk, RPG = kTH / G;
    for (uint32_t i = tid; i < (uint32_t)(kChunk * G); i += 256u) {
      const uint32_t j = i % (uint32_t)kChunk, g = i / (uint32_t)kChunk;
      if (j < n) {
        const Edge e = a.edges[e0 + j];
        const int32_t f = a.feat[e0 + j];
        const Extent x = a.ext[f];
        const bool live = x.hi > xc_first && !(x.lo > xc_last);
        const double dy = e.y1 - e.y0, dx = e.x1 - e.x0;
        if (g == 0) s_feat[j] = f;
#pragma unroll 4
        for (int k = 0; k < RPG; k++) {
          const int32_t rr = (int32_t)g * RPG + k;
          const double yc = (double)(a.row_off + r0 + rr) + 0.5;
          double xi = -HUGE_VAL;
          if (live && e.y0 <= yc && yc < e.y1) xi = e.x0 + ((yc - e.y0) / dy) * dx;
          s_xi[rr * kRowStride + (int32_t)j] = xi;
        }
      }
    }
    __syncthreads();
    // phase B: the row's crossings against the thread's 4 centres, four edges per round of LDS reads (a read per edge
    // followed by the branch on its feature left the loop waiting for the LDS once per edge: DESIGN 6c)
    const double* __restrict__ row = s_xi + trow * kRowStride;
    auto step = [&](int32_t f, double xi) {
      if (f != cur) {  // (the same edge for every thread)
        commit();
        cur = f;
      }
      if (xi > xc[0]) {  // else none of the thread's centres, xc[0] being the least: a wave skips the edges that do not
        par ^= 1u;       // cross its rows or lie left of its pixels, most of a long list
#pragma unroll
        for (int p = 1; p < kPix; p++) par ^= (xi > xc[p] ? 1u : 0u) << p;
      }
    };
    uint32_t j = 0;
    for (; j + 4 <= n; j += 4) {
      const int4 f4 = *reinterpret_cast<const int4*>(s_feat + j);
      const double2 xa = *reinterpret_cast<const double2*>(row + j), xb = *reinterpret_cast<const double2*>(row + j + 2);
      step(f4.x, xa.x), step(f4.y, xa.y), step(f4.z, xb.x), step(f4.w, xb.y);
    }
    for (; j < n; j++) step(s_feat[j], row[j]);
    __syncthreads();
  }
  commit();
  uint32_t cnt = 0;
  if (R < a.h && C < a.w) {
    T o[kPix];
#pragma unroll
    for (int p = 0; p < kPix; p++) o[p] = (T)((cov >> p & 1u) ? val[p] : a.fill);
    T* const d = (T*)a.dst + (int64_t)R * a.drs + (int64_t)C * a.dcs;
    if (a.vec && C + kPix <= a.w) {
      VecOf<T, kPix> v;
#pragma unroll
      for (int p = 0; p < kPix; p++) v.v[p] = o[p];
      *(VecOf<T, kPix>*)d = v;
      cnt = (uint32_t)__popc(cov);
    } else {
#pragma unroll
      for (int p = 0; p < kPix; p++)
        if (C + p < a.w) {
          d[(int64_t)p * a.dcs] = o[p];
          cnt += cov >> p & 1u;
        }
    }
  }
  // the workgroup's covered pixels into its own word
  const uint32_t total = wg_sum(cnt);
  if (tid == 0) a.partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// out[workgroup] = the sum of its kFold partial counts
__global__ void __launch_bounds__(256) k_rasterize_fold(const uint32_t* __restrict__ partial, uint32_t n, unsigned long long* __restrict__ out) {
  const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)kFold;
  unsigned long long s = 0;
  for (uint32_t i = tid; i < (uint32_t)kFold && base + i < n; i += 256u) s += partial[base + i];
  const unsigned long long total = wg_sum(s);
  if (tid == 0) out[blockIdx.x] = total;
}

thread_local float g_rasterize_ms = 0.f;

// f(U{}) for the unsigned type of an integer dtype's size: the kernel moves bit patterns
template <typename F>
void with_bits(int dtype, F&& f) {
  switch (elem_size(dtype)) {
    case 1: f(uint8_t{}); break;
    case 2: f(uint16_t{}); break;
    default: f(uint32_t{}); break;
  }
}

// a host table on the device, in the call's arena
template <typename T>
int upload(Call& c, const std::vector<T>& v, const T** d) {
  T* p = nullptr;
  HIPCHK(c.sc.alloc(&p, v.size() * sizeof(T)));
  if (!v.empty()) HIPCHK(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c.s));
  *d = p;
  return FRA_OK;
}

}  // namespace

extern "C" {

FRA_API int fra_rasterize_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_rasterize_ms;
  return FRA_OK;
}

FRA_API int fra_rasterize(fra_ctx* ctx, const fra_rasterize_job* job, uint64_t* burned) {
  if (!ctx || !job || !job->dst || (job->nfeatures > 0 && (!job->feature_ring_start || !job->values)) ||
      (job->nrings > 0 && (!job->ring_start || !job->xy)))
    return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (const int rc = check_job(job)) return rc;
  Prepared p;
  if (const int rc = prepare(job, &p)) return rc;
  Call c(ctx);
  const size_t es = (size_t)elem_size(job->dtype);
  const Strides ds{0, job->row_stride, job->col_stride};
  StagedOut out;
  if (const int rc = stage_out(c, job->dst, job->dst_on_device, (size_t)extent_of(1, job->height, job->width, ds) * es, &out))
    return rc;
  RzArgs a{};
  if (const int rc = upload(c, p.bins.edges, &a.edges)) return rc;
  if (const int rc = upload(c, p.bins.feat, &a.feat)) return rc;
  if (const int rc = upload(c, p.bins.band_start, &a.band_start)) return rc;
  if (const int rc = upload(c, p.ext, &a.ext)) return rc;
  if (const int rc = upload(c, p.values, &a.values)) return rc;
  const uint32_t tiles_x = (uint32_t)((job->width + kTW - 1) / kTW), tiles_y = (uint32_t)((job->height + kTH - 1) / kTH);
  const uint32_t ntiles = tiles_x * tiles_y, nfold = (ntiles + (uint32_t)kFold - 1) / (uint32_t)kFold;  // at most 2^22 and 2^10
  unsigned long long* d_sums = nullptr;
  HIPCHK(c.sc.alloc(&a.partial, (size_t)ntiles * sizeof(uint32_t)));
  HIPCHK(c.sc.alloc(&d_sums, (size_t)nfold * sizeof(unsigned long long)));
  a.dst = out.dev;
  a.row_off = job->row_off, a.col_off = job->col_off, a.drs = ds.row, a.dcs = ds.col;
  a.h = job->height, a.w = job->width;
  a.fill = (uint32_t)(uint64_t)job->fill;
  a.vec = ds.col == 1 && ((uintptr_t)out.dev % (kPix * es)) == 0 && (ds.row % kPix) == 0;
  std::vector<unsigned long long> sums(nfold);
  const int rc = timed(
      c, &g_rasterize_ms,
      [&]() -> int {
        with_bits(job->dtype, [&](auto t) {
          hipLaunchKernelGGL((k_rasterize<decltype(t)>), dim3(tiles_x, tiles_y), dim3(256), 0, c.s, a);
        });
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_rasterize_fold, dim3(nfold), dim3(256), 0, c.s, a.partial, ntiles, d_sums);
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&]() -> int {
        HIPCHK(hipMemcpyAsync(sums.data(), d_sums, (size_t)nfold * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.s));
        return copy_back(c, out);
      });
  if (rc) return rc;
  if (burned) {
    uint64_t n = 0;
    for (unsigned long long s : sums) n += (uint64_t)s;
    *burned = n;
  }
  return FRA_OK;
}

}  // extern "C"
