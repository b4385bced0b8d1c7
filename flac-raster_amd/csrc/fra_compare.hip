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
// k_compare<T>: a workgroup is one (band, chunk of rows); the chunk is cut into slots of V = 16 / sizeof(T) consecutive
// elements of a row, and thread t owns slots t, t + 256, ... of the chunk: one 16-byte load per raster and slot when both
// layouts allow, guarded element loads otherwise (any layout; the slots are the same, so the result does not depend on
// which loads were used).  The next slot's loads are in flight while the current one is accumulated.  The thread's
// record goes through a fixed wave tree (__shfl_down) and, through LDS, the block's four waves in order, to one partial
// per workgroup.  Nothing else is written, there are no atomics.
// k_compare_fold: one workgroup per band.  Counts, extremes and the integer sums are folded by the same tree (they do not
// depend on the order); the two f64 sums are added strictly in partial order.  Equal inputs and layout give equal bytes.
//
// This unit holds the kernels, their launch and the 2^32-pixel refusal.  Shared with the other region-reducing units
// (fra_region.h): the dtype and layout refusal, what is left to the windowed read (the variant that ignores the job's
// destination), the staging of host rasters, the region decoded by fra_decode_device_window as any caller would, and
// the timed launch.
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
  uint32_t nvec;       // slots per row: ceil(w / V)
  uint32_t rpb;        // rows per workgroup
  uint32_t nchunks;    // workgroups per band: ceil(h / rpb)
  uint32_t step_rows;  // 256 / nvec and 256 % nvec: a thread's way from one of its slots to the next
  uint32_t step_vecs;
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

__device__ inline uint64_t down(uint64_t v, int off) { return (uint64_t)__shfl_down((unsigned long long)v, off, 64); }
__device__ inline double down(double v, int off) { return __shfl_down(v, off, 64); }

// the block's record in thread 0: lane tree inside each wave, then the waves in order
__device__ inline Partial block_reduce(Partial p, Partial* sh /* [4] */) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    Partial q;
    q.differing = down(p.differing, off), q.unordered = down(p.unordered, off), q.first = down(p.first, off);
    q.sum_abs = down(p.sum_abs, off), q.sq_lo = down(p.sq_lo, off), q.sq_hi = down(p.sq_hi, off);
    q.max_abs = down(p.max_abs, off), q.fsum_abs = down(p.fsum_abs, off), q.fsum_sq = down(p.fsum_sq, off);
    q.a_min = down(p.a_min, off), q.a_max = down(p.a_max, off), q.b_min = down(p.b_min, off), q.b_max = down(p.b_max, off);
    combine(p, q);  // (lanes past 64 - off fold their own value in; lane 0 never reads them)
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    p = sh[0];
    for (int k = 1; k < 4; k++) combine(p, sh[k]);
  }
  return p;
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
  struct alignas(16) Vec { T v[V]; };
  __shared__ Partial sh[4];
  const uint32_t chunk = blockIdx.x % g.nchunks;
  const int64_t band = (int64_t)(blockIdx.x / g.nchunks);
  const int64_t row0 = (int64_t)chunk * g.rpb;
  const uint32_t rows = (uint32_t)min((int64_t)g.rpb, (int64_t)g.h - row0);
  const T* __restrict__ pa = (const T*)g.a + (band * g.abs_ + row0 * g.ars);
  const T* __restrict__ pb = (const T*)g.b + (band * g.bbs + row0 * g.brs);
  const bool vec = g.vec != 0;
  // slot (row, cv) of the chunk: elements [cv V, cv V + n) of its row
  auto count = [&](uint32_t cv) { return (int)min((int64_t)V, (int64_t)g.w - (int64_t)cv * V); };
  auto load = [&](const T* p, int64_t cs, int n) {
    Vec v;
    if (vec && n == V) {
      v = *(const Vec*)p;
    } else {
#pragma unroll
      for (int i = 0; i < V; i++) v.v[i] = i < n ? p[(int64_t)i * cs] : (T)0;
    }
    return v;
  };
  Acc<T> acc;
  uint32_t row = threadIdx.x / g.nvec, cv = threadIdx.x % g.nvec;
  Vec na{}, nb{};
  int nn = 0;
  bool have = row < rows;
  if (have) {
    nn = count(cv);
    na = load(pa + ((int64_t)row * g.ars + (int64_t)cv * V * g.acs), g.acs, nn);
    nb = load(pb + ((int64_t)row * g.brs + (int64_t)cv * V * g.bcs), g.bcs, nn);
  }
  while (have) {
    const Vec ca = na, cb = nb;
    const int cn = nn;
    const uint64_t lin = (uint64_t)(row0 + row) * (uint64_t)g.w + (uint64_t)cv * V;
    row += g.step_rows, cv += g.step_vecs;
    if (cv >= g.nvec) cv -= g.nvec, row++;
    have = row < rows;
    if (have) {  // in flight while the current slot is accumulated
      nn = count(cv);
      na = load(pa + ((int64_t)row * g.ars + (int64_t)cv * V * g.acs), g.acs, nn);
      nb = load(pb + ((int64_t)row * g.brs + (int64_t)cv * V * g.bcs), g.bcs, nn);
    }
    if (cn == V) acc.template slot<true>(ca.v, cb.v, cn, lin);
    else acc.template slot<false>(ca.v, cb.v, cn, lin);
  }
  const Partial p = block_reduce(acc.partial(), sh);
  if (threadIdx.x == 0) g.partials[blockIdx.x] = p;
}

__global__ void __launch_bounds__(256) k_compare_fold(const Partial* __restrict__ partials, uint32_t nchunks, int32_t h,
                                                      int32_t w, int32_t is_float, fra_compare_band* __restrict__ out) {
  __shared__ Partial sh[4];
  __shared__ double s_abs[256], s_sq[256];
  __shared__ double s_total_sq;
  const Partial* p = partials + (size_t)blockIdx.x * nchunks;
  Partial acc;
  acc.differing = acc.unordered = acc.sum_abs = acc.sq_lo = acc.sq_hi = 0, acc.first = kNone;
  acc.max_abs = acc.fsum_abs = acc.fsum_sq = 0.0;
  acc.a_min = acc.b_min = HUGE_VAL, acc.a_max = acc.b_max = -HUGE_VAL;
  for (uint32_t i = threadIdx.x; i < nchunks; i += 256) combine(acc, p[i]);
  acc = block_reduce(acc, sh);  // everything but the two f64 sums, which follow in partial order
  double fa = 0.0, fs = 0.0;
  for (uint32_t base = 0; base < nchunks; base += 256) {
    const uint32_t i = base + threadIdx.x;
    s_abs[threadIdx.x] = i < nchunks ? p[i].fsum_abs : 0.0;
    s_sq[threadIdx.x] = i < nchunks ? p[i].fsum_sq : 0.0;
    __syncthreads();
    const uint32_t n = min(256u, nchunks - base);
    if (threadIdx.x == 0)
      for (uint32_t j = 0; j < n; j++) fa = fa + s_abs[j];
    if (threadIdx.x == 64)  // (another wave)
      for (uint32_t j = 0; j < n; j++) fs = fs + s_sq[j];
    __syncthreads();
  }
  if (threadIdx.x == 64) s_total_sq = fs;
  __syncthreads();
  if (threadIdx.x != 0) return;
  fra_compare_band r;
  r.count = (uint64_t)h * (uint64_t)w;
  r.differing = acc.differing, r.unordered = acc.unordered;
  r.first_row = acc.first == kNone ? -1 : (int64_t)(acc.first / (uint64_t)w);
  r.first_col = acc.first == kNone ? -1 : (int64_t)(acc.first % (uint64_t)w);
  r.sum_abs = acc.sum_abs, r.sum_sq_lo = acc.sq_lo, r.sum_sq_hi = acc.sq_hi;
  r.max_abs = acc.max_abs;
  r.fsum_abs = is_float ? fa : 0.0, r.fsum_sq = is_float ? s_total_sq : 0.0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool no_a = is_float && acc.a_min > acc.a_max, no_b = is_float && acc.b_min > acc.b_max;  // no number in the band
  r.a_min = no_a ? nan : acc.a_min, r.a_max = no_a ? nan : acc.a_max;
  r.b_min = no_b ? nan : acc.b_min, r.b_max = no_b ? nan : acc.b_max;
  r.reserved = 0;
  out[blockIdx.x] = r;
}

thread_local float g_compare_ms = 0.f;

constexpr int64_t kMaxPixels = (int64_t)1 << 32;  // per band: sum_abs stays inside 64 bits
constexpr int64_t kBlocks = 4096;                 // workgroups aimed at: 16 per CU
constexpr int64_t kMinSlots = 1024;               // slots of a workgroup, at least (4 per thread), rows permitting

int too_many_pixels(int64_t h, int64_t w) {
  if (h * w <= kMaxPixels) return FRA_OK;
  return fra_internal_set_error(FRA_E_INVALID, "more than 2^32 pixels per band (%lld x %lld) are not compared in one call",
                                (long long)h, (long long)w);
}

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
  const int64_t nvec = ((int64_t)g.w + V - 1) / V;
  int64_t rpb = std::max<int64_t>(((int64_t)g.h * channels + kBlocks - 1) / kBlocks, (kMinSlots + nvec - 1) / nvec);
  rpb = std::min<int64_t>(rpb, std::max<int64_t>(1, ((int64_t)1 << 31) / nvec));  // a chunk's slots are counted in 32 bits
  rpb = std::min<int64_t>(rpb, g.h);
  const int64_t nchunks = ((int64_t)g.h + rpb - 1) / rpb;
  const int64_t grid = nchunks * channels;
  if (grid > INT32_MAX) return fra_internal_set_error(FRA_E_INVALID, "the raster is too large for one comparison");
  g.nvec = (uint32_t)nvec, g.rpb = (uint32_t)rpb, g.nchunks = (uint32_t)nchunks;
  g.step_rows = (uint32_t)(256 / nvec), g.step_vecs = (uint32_t)(256 % nvec);
  HIPCHK(c.sc.alloc(&g.partials, (size_t)grid * sizeof(Partial)));
  fra_compare_band* d_bands = nullptr;
  HIPCHK(c.sc.alloc(&d_bands, (size_t)channels * sizeof(fra_compare_band)));
  return timed(
      c, &g_compare_ms,
      [&]() -> int {
        with_dtype(dtype, [&](auto t) {
          hipLaunchKernelGGL(k_compare<decltype(t)>, dim3((unsigned)grid), dim3(256), 0, c.s, g);
        });
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_compare_fold, dim3((unsigned)channels), dim3(256), 0, c.s, (const Partial*)g.partials,
                           g.nchunks, g.h, g.w, (int32_t)(dtype == FRA_F32 || dtype == FRA_F64), d_bands);
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
  if (const int rc = too_many_pixels(h, w)) return rc;
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
  if (const int rc = too_many_pixels(h, w)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  Call c(ctx);
  void* d_region = nullptr;  // the region at full resolution: band-planar, in dst_dtype, rows on 16-byte boundaries
  int64_t rs = 0;
  if (const int rc = decode(ctx, job, roi, infos, c.sc, &d_region, &rs)) return rc;
  const Strides sa{(int64_t)h * rs, rs, 1}, sb{ref_band_stride, ref_row_stride, ref_col_stride};
  const void* d_ref = nullptr;
  if (const int rc = stage_in(c, ref, ref_on_device,
                              (size_t)extent_of(job->channels, h, w, sb) * (size_t)elem_size(job->dst_dtype), &d_ref))
    return rc;
  return run_compare(c, job->dst_dtype, job->channels, h, w, d_region, sa, d_ref, sb, bands);
}

}  // extern "C"
