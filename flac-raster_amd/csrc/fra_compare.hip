// fra_compare.hip -- exact comparison of two rasters (fra_compare), and of a region of a set of tile streams with a
// reference raster without the decoded region leaving the GPU (fra_decode_device_compare).
//
// The rule (include/flac_raster_amd.h), one report per band of two (channels, h, w) rasters a and b of one dtype:
//   integer dtypes  d = (int64)a - (int64)b, never wrapping; differing = pixels with d != 0; first = the first of them in
//                   row-major order; max |d|, sum |d| (uint64), sum d^2 (128 bits), min / max of a and of b: all exact.
//   f32 / f64       every element as f64.  Both numbers: equal iff a == b, d = 0.0 when equal else a - b, |d| goes to
//                   max_abs and fsum_abs, d * d to fsum_sq.  Both NaN: unordered only.  One NaN: unordered and differing.
//                   Minima and maxima skip NaN.
//
// k_compare<T>: the row-chunk scan of fra_scan.h over two rasters, slots of V = 16 / sizeof(T) elements, vector loads
// when both layouts allow, the pipelined row-major walk (scan_row_major).  The thread's record goes through the fixed
// tree of block_reduce to one partial per workgroup.  Nothing else is written, there are no atomics.
// k_compare_fold: one workgroup per band.  Counts, extremes and the integer sums are folded by the same tree (they do not
// depend on the order); the two f64 sums are added strictly in partial order.  Equal inputs and layout give equal bytes.
//
// This unit holds the kernels and their launch.  Shared with the other units over a region (fra_region.h): the dtype
// and layout refusal, what is left to the windowed read (the variant that ignores the job's destination), the staging
// of host rasters, the region decoded by fra_decode_device_window as any caller would, and the timed launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"
#include "fra_scan.h"

static_assert(sizeof(fra_compare_band) == 128, "fra_compare_band is 128 bytes");

namespace {

using namespace fra_region;

constexpr uint64_t kNone = ~0ull;  // no differing pixel

struct Partial {  // a thread's, a wave's, a workgroup's and, folded, a band's record
  uint64_t differing, unordered, first /* band-linear index, kNone */, sum_abs, sq_lo, sq_hi;
  double max_abs, fsum_abs, fsum_sq, a_min, a_max, b_min, b_max;
};

struct CmpArgs {
  const void* a;
  const void* b;
  int64_t abs_, ars, acs;  // element strides of a: band, row, column
  int64_t bbs, brs, bcs;   // ... of b
  Partial* partials;       // channels x nchunks
  int32_t h, w;
  ChunkPlan plan;
  int32_t vec;  // 16-byte loads are aligned in both rasters (column stride 1; base, row and band strides multiples of 16 bytes)
};

// x then y: the f64 sums are x + y in this order
__device__ inline void combine(Partial& x, const Partial& y) {
  x.differing += y.differing;
  x.unordered += y.unordered;
  x.first = y.first < x.first ? y.first : x.first;
  x.sum_abs += y.sum_abs;
  x.sq_lo += y.sq_lo;
  x.sq_hi += y.sq_hi + (x.sq_lo < y.sq_lo);
  x.max_abs = y.max_abs > x.max_abs ? y.max_abs : x.max_abs;
  x.fsum_abs = x.fsum_abs + y.fsum_abs;
  x.fsum_sq = x.fsum_sq + y.fsum_sq;
  x.a_min = y.a_min < x.a_min ? y.a_min : x.a_min;
  x.a_max = y.a_max > x.a_max ? y.a_max : x.a_max;
  x.b_min = y.b_min < x.b_min ? y.b_min : x.b_min;
  x.b_max = y.b_max > x.b_max ? y.b_max : x.b_max;
}

template <typename T, bool FLT = std::is_floating_point<T>::value>
struct Acc;

// integers: |d| <= 2^32 - 1 fits 32 bits, d^2 64; the thread's sums cannot leave 64 / 128 bits
template <typename T>
struct Acc<T, false> {
  static constexpr int V = 16 / (int)sizeof(T);
  uint64_t differing = 0, first = kNone, sum_abs = 0, sq_lo = 0, sq_hi = 0;
  uint32_t mx = 0;
  T amin = std::numeric_limits<T>::max(), amax = std::numeric_limits<T>::lowest();
  T bmin = std::numeric_limits<T>::max(), bmax = std::numeric_limits<T>::lowest();

  template <bool FULL>
  __device__ inline void slot(const T* a, const T* b, int n, uint64_t lin) {
    uint32_t mask = 0;
    uint64_t sabs = 0, ssq = 0;  // (narrow types: the compiler keeps what fits in 32 bits there)
#pragma unroll
    for (int i = 0; i < V; i++) {
      if (FULL || i < n) {
        const T x = a[i], y = b[i];
        // the difference modulo 2^32 of the larger and the smaller is their true distance
        const uint32_t ad = x > y ? (uint32_t)x - (uint32_t)y : (uint32_t)y - (uint32_t)x;
        mask |= (ad != 0 ? 1u : 0u) << i;
        mx = ad > mx ? ad : mx;
        amin = x < amin ? x : amin, amax = x > amax ? x : amax;
        bmin = y < bmin ? y : bmin, bmax = y > bmax ? y : bmax;
        if constexpr (sizeof(T) < 4) {
          sabs += ad;
          ssq += ad * ad;  // < 2^32
        } else {
          sum_abs += ad;
          const uint64_t q = (uint64_t)ad * ad;
          sq_lo += q;
          sq_hi += sq_lo < q;
        }
      }
    }
    if constexpr (sizeof(T) < 4) {
      sum_abs += sabs;
      sq_lo += ssq;
      sq_hi += sq_lo < ssq;
    }
    if (mask) {
      differing += (uint32_t)__popc(mask);
      if (first == kNone) first = lin + (uint32_t)(__ffs((int)mask) - 1);  // the thread meets its slots in row-major order
    }
  }
  __device__ inline Partial partial() const {
    Partial p;
    p.differing = differing, p.unordered = 0, p.first = first, p.sum_abs = sum_abs, p.sq_lo = sq_lo, p.sq_hi = sq_hi;
    p.max_abs = (double)mx, p.fsum_abs = 0.0, p.fsum_sq = 0.0;
    p.a_min = (double)amin, p.a_max = (double)amax, p.b_min = (double)bmin, p.b_max = (double)bmax;
    return p;
  }
};

template <typename T>
struct Acc<T, true> {
  static constexpr int V = 16 / (int)sizeof(T);
  uint64_t differing = 0, unordered = 0, first = kNone;
  double mx = 0.0, fsum_abs = 0.0, fsum_sq = 0.0;
  double amin = HUGE_VAL, amax = -HUGE_VAL, bmin = HUGE_VAL, bmax = -HUGE_VAL;

  template <bool FULL>
  __device__ inline void slot(const T* a, const T* b, int n, uint64_t lin) {
    uint32_t mask = 0, umask = 0;
#pragma unroll
    for (int i = 0; i < V; i++) {
      if (FULL || i < n) {
        const double x = (double)a[i], y = (double)b[i];
        const bool xn = x != x, yn = y != y;
        const bool un = xn || yn;
        const double d = (un || x == y) ? 0.0 : x - y;  // never NaN: inf - inf of one sign is the equal case
        const double ad = fabs(d);
        mask |= ((xn != yn) || (!un && x != y) ? 1u : 0u) << i;
        umask |= (un ? 1u : 0u) << i;
        mx = ad > mx ? ad : mx;
        fsum_abs = fsum_abs + ad;  // (+0.0 for a pixel that contributes nothing: the sums are never -0.0)
        fsum_sq = fsum_sq + d * d;
        amin = x < amin ? x : amin, amax = x > amax ? x : amax;  // a NaN compares false: skipped
        bmin = y < bmin ? y : bmin, bmax = y > bmax ? y : bmax;
      }
    }
    unordered += (uint32_t)__popc(umask);
    if (mask) {
      differing += (uint32_t)__popc(mask);
      if (first == kNone) first = lin + (uint32_t)(__ffs((int)mask) - 1);
    }
  }
  __device__ inline Partial partial() const {
    Partial p;
    p.differing = differing, p.unordered = unordered, p.first = first, p.sum_abs = 0, p.sq_lo = 0, p.sq_hi = 0;
    p.max_abs = mx, p.fsum_abs = fsum_abs, p.fsum_sq = fsum_sq;
    p.a_min = amin, p.a_max = amax, p.b_min = bmin, p.b_max = bmax;
    return p;
  }
};

template <typename T>
__global__ void __launch_bounds__(256) k_compare(CmpArgs g) {
  constexpr int V = 16 / (int)sizeof(T);
  struct Pair { VecOf<T, V> a, b; };
  __shared__ Partial sh[4];
  const Chunk c = chunk_of(g.plan, g.h, blockIdx.x);
  const T* __restrict__ pa = (const T*)g.a + (c.band * g.abs_ + c.row0 * g.ars);
  const T* __restrict__ pb = (const T*)g.b + (c.band * g.bbs + c.row0 * g.brs);
  const bool vec = g.vec != 0;
  Acc<T> acc;
  scan_row_major<V>(
      g.plan, c.rows, g.w,
      [&](uint32_t row, uint32_t cv, int n) {
        return Pair{load_slot<T, V>(pa + ((int64_t)row * g.ars + (int64_t)cv * V * g.acs), g.acs, vec, n),
                    load_slot<T, V>(pb + ((int64_t)row * g.brs + (int64_t)cv * V * g.bcs), g.bcs, vec, n)};
      },
      [&](const Pair& s, int n, uint32_t row, uint32_t cv) {
        const uint64_t lin = (uint64_t)(c.row0 + row) * (uint64_t)g.w + (uint64_t)cv * V;
        if (n == V) acc.template slot<true>(s.a.v, s.b.v, n, lin);
        else acc.template slot<false>(s.a.v, s.b.v, n, lin);
      });
  const Partial p = block_reduce(acc.partial(), sh, combine);
  if (threadIdx.x == 0) g.partials[blockIdx.x] = p;
}

__global__ void __launch_bounds__(256) k_compare_fold(const Partial* __restrict__ partials, uint32_t nchunks, int32_t h,
                                                      int32_t w, int32_t is_float, fra_compare_band* __restrict__ out) {
  __shared__ Partial sh[4];
  __shared__ double s_f[2][256];
  const Partial* p = partials + (size_t)blockIdx.x * nchunks;
  Partial acc;
  acc.differing = acc.unordered = acc.sum_abs = acc.sq_lo = acc.sq_hi = 0, acc.first = kNone;
  acc.max_abs = acc.fsum_abs = acc.fsum_sq = 0.0;
  acc.a_min = acc.b_min = HUGE_VAL, acc.a_max = acc.b_max = -HUGE_VAL;
  for (uint32_t i = threadIdx.x; i < nchunks; i += 256) combine(acc, p[i]);
  acc = block_reduce(acc, sh, combine);  // everything but the two f64 sums, which follow in partial order
  double fsum[2];
  sum_in_order(p, nchunks, {&Partial::fsum_abs, &Partial::fsum_sq}, s_f, fsum);
  if (threadIdx.x != 0) return;
  fra_compare_band r;
  r.count = (uint64_t)h * (uint64_t)w;
  r.differing = acc.differing, r.unordered = acc.unordered;
  r.first_row = acc.first == kNone ? -1 : (int64_t)(acc.first / (uint64_t)w);
  r.first_col = acc.first == kNone ? -1 : (int64_t)(acc.first % (uint64_t)w);
  r.sum_abs = acc.sum_abs, r.sum_sq_lo = acc.sq_lo, r.sum_sq_hi = acc.sq_hi;
  r.max_abs = acc.max_abs;
  r.fsum_abs = is_float ? fsum[0] : 0.0, r.fsum_sq = is_float ? fsum[1] : 0.0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool no_a = is_float && acc.a_min > acc.a_max, no_b = is_float && acc.b_min > acc.b_max;  // no number in the band
  r.a_min = no_a ? nan : acc.a_min, r.a_max = no_a ? nan : acc.a_max;
  r.b_min = no_b ? nan : acc.b_min, r.b_max = no_b ? nan : acc.b_max;
  r.reserved = 0;
  out[blockIdx.x] = r;
}

thread_local float g_compare_ms = 0.f;

constexpr const char* kNot = "compared in one call";  // (too_many_pixels; sum_abs stays inside 64 bits)

// k_compare + k_compare_fold over two (channels, h, w) device rasters, timed, and the reports to `bands` on the host
// (the partials and the device reports belong to the call)
int run_compare(Call& c, int dtype, int channels, int32_t h, int32_t w, const void* d_a, const Strides& sa,
                const void* d_b, const Strides& sb, fra_compare_band* bands) {
  const size_t es = (size_t)elem_size(dtype);
  const int64_t V = 16 / (int64_t)es;
  CmpArgs g{};
  g.a = d_a, g.b = d_b;
  g.abs_ = sa.band, g.ars = sa.row, g.acs = sa.col;
  g.bbs = sb.band, g.brs = sb.row, g.bcs = sb.col;
  g.h = h, g.w = w;
  g.vec = aligned16(d_a, sa, es) && aligned16(d_b, sb, es);
  // (a chunk's slots are counted in 32 bits)
  if (const int rc = plan_chunks(&g.plan, V, h, w, channels, (int64_t)1 << 31, 0, "comparison")) return rc;
  const unsigned grid = g.plan.grid;
  HIPCHK(c.sc.alloc(&g.partials, (size_t)grid * sizeof(Partial)));
  fra_compare_band* d_bands = nullptr;
  HIPCHK(c.sc.alloc(&d_bands, (size_t)channels * sizeof(fra_compare_band)));
  return timed(
      c, &g_compare_ms,
      [&]() -> int {
        with_dtype(dtype, [&](auto t) {
          hipLaunchKernelGGL(k_compare<decltype(t)>, dim3(grid), dim3(256), 0, c.s, g);
        });
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_compare_fold, dim3((unsigned)channels), dim3(256), 0, c.s, (const Partial*)g.partials,
                           g.plan.nchunks, g.h, g.w, (int32_t)(dtype == FRA_F32 || dtype == FRA_F64), d_bands);
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&]() -> int {
        HIPCHK(hipMemcpyAsync(bands, d_bands, (size_t)channels * sizeof(fra_compare_band), hipMemcpyDeviceToHost, c.s));
        return FRA_OK;
      });
}

}  // namespace

extern "C" {

FRA_API int fra_compare_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_compare_ms;
  return FRA_OK;
}

FRA_API int fra_compare(fra_ctx* ctx, const fra_compare_job* job, fra_compare_band* bands) {
  if (!ctx || !job || !bands || !job->a || !job->b) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  const Strides sa{job->a_band_stride, job->a_row_stride, job->a_col_stride};
  const Strides sb{job->b_band_stride, job->b_row_stride, job->b_col_stride};
  const int32_t ch = job->channels, h = job->height, w = job->width;
  if (const int rc = check_raster(job->dtype, ch, h, w, sa, sb)) return rc;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  Call c(ctx);
  const size_t es = (size_t)elem_size(job->dtype);
  const void *d_a = nullptr, *d_b = nullptr;
  if (const int rc = stage_in(c, job->a, job->a_on_device, (size_t)extent_of(ch, h, w, sa) * es, &d_a)) return rc;
  if (const int rc = stage_in(c, job->b, job->b_on_device, (size_t)extent_of(ch, h, w, sb) * es, &d_b)) return rc;
  return run_compare(c, job->dtype, ch, h, w, d_a, sa, d_b, sb, bands);
}

FRA_API int fra_decode_device_compare(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, const void* ref,
                                      int32_t ref_on_device, int64_t ref_band_stride, int64_t ref_row_stride,
                                      int64_t ref_col_stride, fra_compare_band* bands, fra_decoded* infos) {
  if (!ctx || !job || !roi || !ref || !bands || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (ref_band_stride < 0 || ref_row_stride < 0 || ref_col_stride < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad reference layout (strides %lld, %lld, %lld)",
                                  (long long)ref_band_stride, (long long)ref_row_stride, (long long)ref_col_stride);
  if (left_to_window_read_no_dst(job, roi)) return refer_to_window_read(ctx, job, roi, infos, true);
  const int32_t h = roi->height, w = roi->width;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region_src(ctx, job, roi, infos, [&](Call& c, const void* d_region, const Strides& sa) -> int {
    const Strides sb{ref_band_stride, ref_row_stride, ref_col_stride};
    const void* d_ref = nullptr;
    if (const int rc = stage_in(c, ref, ref_on_device,
                                (size_t)extent_of(job->channels, h, w, sb) * (size_t)elem_size(job->dst_dtype), &d_ref))
      return rc;
    return run_compare(c, job->dst_dtype, job->channels, h, w, d_region, sa, d_ref, sb, bands);
  });
}

}  // extern "C"
