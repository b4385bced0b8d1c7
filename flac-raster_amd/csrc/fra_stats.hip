// fra_stats.hip -- band statistics and histograms of a raster (fra_stats), and of a region of a set of tile streams
// without the decoded region leaving the GPU (fra_decode_device_stats).
//
// The rule (include/flac_raster_amd.h), one report per band of a (channels, h, w) raster of any dtype, every element as
// f64: nan / nodata / valid counts; min, max and their finite forms over the valid pixels; for integers the exact
// 128-bit sums of x and x^2; for floats fsum, mean = fsum / valid and fm2 = sum (x - mean)^2 with the mean of the
// first pass; a histogram of `bins` bins over an explicit range or over [fin_min, fin_max] of the band, with the pixels
// outside it counted in below / above.
//
// k_stats<T, PASS, HMODE>: the row-chunk scan of fra_scan.h over one raster, slots of V = 16 / sizeof(T) elements, the
// pipelined row-major walk (scan_row_major).
//   PASS 1 accumulates the counts, extremes and sums; PASS 2 reads the band's record (mean, histogram range and scale)
//   from device memory -- no host round trip -- and accumulates fm2 (floats) and the histogram.  Pass 2 runs for floats,
//   and for integers only for a histogram over the automatic range; integers with an explicit range count their
//   histogram in pass 1.
//   HMODE 0: no histogram.  HMODE 1: the workgroup counts a window of at most kLdsBins bins, [bin0, bin0 + nbins), into
//   a private uint32 histogram in LDS with LDS atomics -- equal neighbouring bins of a slot merged first, so a constant
//   raster issues one atomic per slot, not one per pixel -- and adds its non-zero bins to the band's uint64 histogram
//   with 64-bit integer atomics at its end.  Integer atomics do not depend on the order: the counts are deterministic.
//   More than kLdsBins bins (up to 65536) are counted window by window, one more launch of the pass-2 kernel over the
//   raster per window (at most 8): pixels of other windows are skipped, and the partials of these launches are not
//   folded.  (Global atomics per pixel run were measured first: 50 ms for the 65536-bin histogram of a 964 MB uint16
//   scene and 354 ms for a constant one, against 0.5 - 0.8 ms per LDS window.)
//   The thread's record goes through the fixed tree of block_reduce to one partial per workgroup.
// k_stats_fold / k_stats_fold2: one workgroup per band.  Counts, extremes and the integer sums by the same tree, the f64
// sum strictly in partial order; the band's record is written to (pass 1) and completed in (pass 2) device memory.
//
// kLdsBins = 8192: 32 KiB of LDS per workgroup, so the 160 KiB of a CU still hold four workgroups of 256 threads (16
// waves), which a bandwidth-bound loop needs; a uint32 bin per 4-byte bank, so lanes that hit different bins conflict
// only on equal banks and lanes that hit one bin serialise -- which the merge above bounds per slot.
//
// This unit holds the kernels, their launch and the refusals of the options.  Shared with the other units over a region
// (fra_region.h): the dtype and layout refusal, what is left to the windowed read (the variant that ignores the job's
// destination), the staging of a host raster, the decoded region and the timed launch.
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

static_assert(sizeof(fra_stats_band) == 160, "fra_stats_band is 160 bytes");

namespace {

using namespace fra_region;

constexpr int kLdsBins = 8192;   // bins a workgroup counts in LDS (32 KiB)
constexpr int kMaxBins = 65536;

struct Partial {  // a thread's, a wave's, a workgroup's and, folded, a band's record
  uint64_t valid, nan, nodata, below, above, sum_lo, sum_hi /* two's complement */, sq_lo, sq_hi;
  double mn, mx, fmn, fmx;
  double fsum;  // pass 1: sum x; pass 2: sum (x - mean)^2
};

struct StatsArgs {
  const void* src;
  int64_t bs, rs, cs;      // element strides: band, row, column
  Partial* partials;       // channels x nchunks
  fra_stats_band* bands;   // the bands' records in device memory
  unsigned long long* hist;  // channels x bins in device memory
  double lo, hi, scale;    // the explicit range (pass 1 with a histogram)
  double nodata;
  int32_t h, w;
  ChunkPlan plan;
  int32_t vec;  // 16-byte loads are aligned (column stride 1; base, row and band strides multiples of 16 bytes)
  int32_t bins, flags;
  int32_t bin0, nbins;  // the window of bins this launch counts (HMODE 1)
};

// x then y: the f64 sum is x + y in this order
__device__ inline void combine(Partial& x, const Partial& y) {
  x.valid += y.valid, x.nan += y.nan, x.nodata += y.nodata, x.below += y.below, x.above += y.above;
  x.sum_lo += y.sum_lo;
  x.sum_hi += y.sum_hi + (x.sum_lo < y.sum_lo);
  x.sq_lo += y.sq_lo;
  x.sq_hi += y.sq_hi + (x.sq_lo < y.sq_lo);
  x.mn = y.mn < x.mn ? y.mn : x.mn, x.mx = y.mx > x.mx ? y.mx : x.mx;
  x.fmn = y.fmn < x.fmn ? y.fmn : x.fmn, x.fmx = y.fmx > x.fmx ? y.fmx : x.fmx;
  x.fsum = x.fsum + y.fsum;
}

__device__ inline Partial empty_partial() {
  Partial p;
  p.valid = p.nan = p.nodata = p.below = p.above = p.sum_lo = p.sum_hi = p.sq_lo = p.sq_hi = 0;
  p.mn = p.fmn = HUGE_VAL, p.mx = p.fmx = -HUGE_VAL;
  p.fsum = 0.0;
  return p;
}

// the bin of lo <= x <= hi by the rule's f64 operation sequence (x - lo >= 0 and never NaN; the fmax keeps the index
// inside the bins whatever the product is)
__device__ inline int32_t bin_of(double x, double lo, double scale, double top) {
  const double d = x - lo;
  const double t = d * scale;
  return scale == 0.0 ? 0 : (int32_t)fmax(0.0, fmin(top, floor(t)));
}

// a thread's share of the histogram: the bin of a valid pixel by the rule's f64 operation sequence, runs of one bin
// inside a slot merged into one atomic
template <int HMODE>
struct Hist {
  double lo = 0.0, hi = 0.0, scale = 0.0, top = 0.0;  // top = bins - 1
  bool on = false;
  bool unit = false;  // scale == 1.0 and an integral lo: an integer x lies in bin x - lo, exactly what the f64 sequence gives
  int64_t ilo = 0;
  uint32_t* lds = nullptr;  // the workgroup's bins: nbins from bin0
  int32_t bin0 = 0;
  uint32_t nbins = 0;
  uint64_t below = 0, above = 0;
  uint32_t cur = 0;  // window-relative
  uint32_t run = 0;

  __device__ inline void flush() {
    if constexpr (HMODE != 0) {
      if (run) {
        atomicAdd(&lds[cur], run);
        run = 0;
      }
    }
  }
  __device__ inline void set_range(double lo_, double hi_, double scale_, int32_t bins) {
    lo = lo_, hi = hi_, scale = scale_, top = (double)(bins - 1);
    on = lo_ == lo_;  // NaN: the band has no range
    unit = scale_ == 1.0 && lo_ == floor(lo_) && fabs(lo_) < 9007199254740992.0;
    ilo = unit ? (int64_t)lo_ : 0;
  }
  __device__ inline void count(int32_t i) {
    const uint32_t j = (uint32_t)(i - bin0);
    if (j < nbins) {  // (a bin of another window: counted by that window's launch)
      if (j != cur) flush(), cur = j;
      run++;
    }
  }
  __device__ inline void put(double x) {
    if constexpr (HMODE != 0) {
      if (!on) return;
      if (x < lo) below++;
      else if (x > hi) above++;
      else count(bin_of(x, lo, scale, top));
    }
  }
  // an integer pixel (|x| < 2^32)
  __device__ inline void put_int(int64_t xi) {
    if constexpr (HMODE != 0) {
      if (!on) return;
      const double x = (double)xi;
      if (x < lo) below++;
      else if (x > hi) above++;
      else if (unit) count((int32_t)min(xi - ilo, (int64_t)top));  // 0 <= x - lo <= hi - lo = bins
      else count(bin_of(x, lo, scale, top));
    }
  }
};

template <typename T, int PASS, int HMODE>
struct Acc {
  static constexpr bool FLT = std::is_floating_point<T>::value;
  static constexpr int V = 16 / (int)sizeof(T);
  using M = std::conditional_t<FLT, double, T>;  // extremes and the nodata value
  using S = std::conditional_t<FLT, double, std::conditional_t<std::is_signed<T>::value, int64_t, uint64_t>>;
  uint64_t valid = 0, nan = 0, nodata = 0, sq_lo = 0, sq_hi = 0;
  S sum = 0;  // integers: |x| <= 2^31 over fewer than 2^32 / 256 + V pixels; floats: sum x (pass 1), sum (x - mean)^2 (pass 2)
  M mn = FLT ? (M)HUGE_VAL : std::numeric_limits<M>::max(), mx = FLT ? (M)-HUGE_VAL : std::numeric_limits<M>::lowest();
  double fmn = HUGE_VAL, fmx = -HUGE_VAL;  // floats
  Nodata<T> nodata_of;
  double mean = 0.0;
  Hist<HMODE> hist;

  template <bool FULL>
  __device__ inline void slot(const T* v, int n) {
    int32_t ssum = 0;   // one- and two-byte integers: the slot's sums stay inside 32 and 64 bits without a carry
    uint64_t ssq = 0;
#pragma unroll
    for (int i = 0; i < V; i++) {
      if (FULL || i < n) {
        const M x = (M)v[i];
        if constexpr (FLT) {
          if (x != x) {
            nan++;
            continue;
          }
        }
        if (nodata_of.is(x)) {
          nodata++;
          continue;
        }
        if constexpr (PASS == 1) {
          valid++;
          mn = x < mn ? x : mn, mx = x > mx ? x : mx;
          if constexpr (FLT) {
            if (fabs(x) < HUGE_VAL) fmn = x < fmn ? x : fmn, fmx = x > fmx ? x : fmx;
            sum = sum + x;
          } else if constexpr (sizeof(T) < 4) {
            const int32_t xs = (int32_t)x;
            ssum += xs;  // |x| < 2^16, at most 16 of them
            const uint32_t ax = (uint32_t)(xs < 0 ? -xs : xs);
            ssq += ax * ax;  // < 2^32
          } else {
            sum += (S)x;
            const int64_t xs = (int64_t)x;
            const uint64_t ax = xs < 0 ? (uint64_t)-xs : (uint64_t)xs;  // <= 2^32 - 1 (2^31 for int32)
            const uint64_t q = ax * ax;
            sq_lo += q;
            sq_hi += sq_lo < q;
          }
        } else if constexpr (FLT) {
          const double d = x - mean;
          sum = sum + d * d;
        }
        if constexpr (FLT) hist.put((double)x);
        else hist.put_int((int64_t)x);
      }
    }
    if constexpr (PASS == 1 && !FLT && sizeof(T) < 4) {
      sum += (S)ssum;
      sq_lo += ssq;  // a thread's pixels (fewer than 2^32 / 256 + V) x 2^30: no carry
    }
    hist.flush();
  }

  __device__ inline Partial partial() const {
    Partial p = empty_partial();
    p.below = hist.below, p.above = hist.above;
    if constexpr (PASS == 1) {
      p.valid = valid, p.nan = nan, p.nodata = nodata;
      if (valid) p.mn = (double)mn, p.mx = (double)mx;
      if constexpr (FLT) {
        p.fmn = fmn, p.fmx = fmx, p.fsum = sum;
      } else {
        p.fmn = p.mn, p.fmx = p.mx;
        p.sum_lo = (uint64_t)sum;
        if constexpr (std::is_signed<T>::value) p.sum_hi = sum < 0 ? ~0ull : 0ull;
        p.sq_lo = sq_lo, p.sq_hi = sq_hi;
      }
    } else if constexpr (FLT) {
      p.fsum = sum;
    }
    return p;
  }
};

template <typename T, int PASS, int HMODE>
__global__ void __launch_bounds__(256) k_stats(StatsArgs g) {
  constexpr int V = 16 / (int)sizeof(T);
  extern __shared__ uint32_t s_hist[];  // HMODE 1: the workgroup's bins (nbins x 4 bytes of dynamic LDS)
  __shared__ Partial sh[4];
  const Chunk c = chunk_of(g.plan, g.h, blockIdx.x);
  const int64_t band = c.band;
  const T* __restrict__ ps = (const T*)g.src + (band * g.bs + c.row0 * g.rs);
  const bool vec = g.vec != 0;
  unsigned long long* const band_hist = HMODE != 0 ? g.hist + (band * (int64_t)g.bins + g.bin0) : nullptr;

  Acc<T, PASS, HMODE> acc;
  acc.nodata_of.set((g.flags & FRA_STATS_NODATA) != 0, g.nodata);
  if constexpr (HMODE != 0) {
    if constexpr (PASS == 1) {
      acc.hist.set_range(g.lo, g.hi, g.scale, g.bins);
    } else {
      const fra_stats_band* r = g.bands + band;
      acc.hist.set_range(r->hist_lo, r->hist_hi, r->hist_scale, g.bins);
    }
    acc.hist.lds = s_hist, acc.hist.bin0 = g.bin0, acc.hist.nbins = (uint32_t)g.nbins;
  }
  if constexpr (PASS == 2) acc.mean = g.bands[band].mean;
  if constexpr (PASS == 2 && HMODE == 1) {
    // a further window (its partial is not folded) that the band's finite valid pixels cannot reach -- the bin is
    // monotonic in x -- has nothing to count: the whole workgroup leaves before it reads a pixel
    if (g.bin0 > 0) {
      const fra_stats_band* r = g.bands + band;
      const double xa = fmax(r->fin_min, acc.hist.lo), xb = fmin(r->fin_max, acc.hist.hi);
      if (!acc.hist.on || !(xa <= xb)) return;
      const int32_t ba = bin_of(xa, acc.hist.lo, acc.hist.scale, acc.hist.top);
      const int32_t bb = bin_of(xb, acc.hist.lo, acc.hist.scale, acc.hist.top);
      if (bb < g.bin0 || ba >= g.bin0 + g.nbins) return;
    }
  }
  if constexpr (HMODE == 1) {
    for (int i = threadIdx.x; i < g.nbins; i += 256) s_hist[i] = 0;
    __syncthreads();
  }

  scan_row_major<V>(
      g.plan, c.rows, g.w,
      [&](uint32_t row, uint32_t cv, int n) {
        return load_slot<T, V>(ps + ((int64_t)row * g.rs + (int64_t)cv * V * g.cs), g.cs, vec, n);
      },
      [&](const VecOf<T, V>& x, int n, uint32_t, uint32_t) {
        if (n == V) acc.template slot<true>(x.v, n);
        else acc.template slot<false>(x.v, n);
      });
  const Partial p = block_reduce(acc.partial(), sh, combine);  // (its barrier also ends the workgroup's LDS counting)
  if (threadIdx.x == 0) g.partials[blockIdx.x] = p;
  if constexpr (HMODE == 1) {
    for (int i = threadIdx.x; i < g.nbins; i += 256) {
      const uint32_t c = s_hist[i];
      if (c) atomicAdd(&band_hist[i], (unsigned long long)c);
    }
  }
}

// a band's partials folded into thread 0's record; the f64 sum, added strictly in partial order, into *fsum
__device__ inline Partial fold_partials(const Partial* p, uint32_t nchunks, Partial* sh, double (&s_f)[1][256],
                                        double* fsum) {
  Partial acc = empty_partial();
  for (uint32_t i = threadIdx.x; i < nchunks; i += 256) combine(acc, p[i]);
  acc = block_reduce(acc, sh, combine);  // everything but the f64 sum, which follows in partial order
  double f[1];
  sum_in_order(p, nchunks, {&Partial::fsum}, s_f, f);
  *fsum = f[0];
  return acc;
}

__global__ void __launch_bounds__(256) k_stats_fold(StatsArgs g, int32_t is_float, int32_t fused_hist) {
  __shared__ Partial sh[4];
  __shared__ double s_f[1][256];
  double fsum = 0.0;
  const Partial a = fold_partials(g.partials + (size_t)blockIdx.x * g.plan.nchunks, g.plan.nchunks, sh, s_f, &fsum);
  if (threadIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  fra_stats_band r;
  r.count = (uint64_t)g.h * (uint64_t)g.w;
  r.valid = a.valid, r.nan = a.nan, r.nodata = a.nodata;
  r.below = fused_hist ? a.below : 0, r.above = fused_hist ? a.above : 0;
  r.sum_lo = a.sum_lo, r.sum_hi = (int64_t)a.sum_hi, r.sq_lo = a.sq_lo, r.sq_hi = a.sq_hi;
  const bool none = a.valid == 0, no_fin = a.fmn > a.fmx;
  r.min = none ? nan : a.mn, r.max = none ? nan : a.mx;
  r.fin_min = no_fin ? nan : a.fmn, r.fin_max = no_fin ? nan : a.fmx;
  r.fsum = is_float ? fsum : 0.0;
  r.mean = is_float ? fsum / (double)a.valid : 0.0;  // 0.0 / 0.0 = NaN for a band without a valid pixel
  r.fm2 = 0.0;
  r.hist_lo = r.hist_hi = r.hist_scale = 0.0;
  if (g.bins > 0) {
    const bool automatic = (g.flags & FRA_STATS_AUTO_RANGE) != 0;
    if (automatic && no_fin) {
      r.hist_lo = r.hist_hi = nan;
    } else {
      r.hist_lo = automatic ? r.fin_min : g.lo, r.hist_hi = automatic ? r.fin_max : g.hi;
      const double span = r.hist_hi - r.hist_lo;
      double scale = r.hist_hi > r.hist_lo ? (double)g.bins / span : 0.0;
      if (!(fabs(scale) < HUGE_VAL)) scale = 0.0;
      r.hist_scale = scale;
    }
  }
  g.bands[blockIdx.x] = r;
}

__global__ void __launch_bounds__(256) k_stats_fold2(StatsArgs g, int32_t is_float) {
  __shared__ Partial sh[4];
  __shared__ double s_f[1][256];
  double fsum = 0.0;
  const Partial a = fold_partials(g.partials + (size_t)blockIdx.x * g.plan.nchunks, g.plan.nchunks, sh, s_f, &fsum);
  if (threadIdx.x != 0) return;
  fra_stats_band* r = g.bands + blockIdx.x;
  r->below = a.below, r->above = a.above;
  if (is_float) r->fm2 = fsum;
}

thread_local float g_stats_ms = 0.f;

constexpr const char* kNot = "described in one call";  // (too_many_pixels)

template <typename T, int PASS, int HMODE>
void launch_one(unsigned grid, size_t lds, hipStream_t s, const StatsArgs& g) {
  hipLaunchKernelGGL((k_stats<T, PASS, HMODE>), dim3(grid), dim3(256), lds, s, g);
}

template <typename T>
void launch_pass(int pass, int hmode, unsigned grid, size_t lds, hipStream_t s, const StatsArgs& g) {
  constexpr bool FLT = std::is_floating_point<T>::value;
  if (pass == 1) {
    if constexpr (FLT) {
      launch_one<T, 1, 0>(grid, 0, s, g);  // floats count their histogram in pass 2
    } else {
      if (hmode == 0) launch_one<T, 1, 0>(grid, 0, s, g);
      else launch_one<T, 1, 1>(grid, lds, s, g);
    }
  } else {
    if (hmode == 1) launch_one<T, 2, 1>(grid, lds, s, g);
    else if constexpr (FLT) launch_one<T, 2, 0>(grid, 0, s, g);
  }
}

void launch_dtype(int dtype, int pass, int hmode, unsigned grid, size_t lds, hipStream_t s, const StatsArgs& g) {
  with_dtype(dtype, [&](auto t) { launch_pass<decltype(t)>(pass, hmode, grid, lds, s, g); });
}

// the statistics kernels over a (channels, h, w) device raster, timed, the reports to `bands` and the counts to `hist`
// on the host (the partials, the device reports and the device histogram belong to the call)
int run_stats(Call& c, int dtype, int channels, int32_t h, int32_t w, const void* d_src, const Strides& ss,
              const fra_stats_opts& o, fra_stats_band* bands, uint64_t* hist) {
  hipStream_t s = c.s;
  HipArena& sc = c.sc;
  StatsArgs g{};
  g.bs = ss.band, g.rs = ss.row, g.cs = ss.col;
  g.h = h, g.w = w;
  const size_t es = (size_t)elem_size(dtype);
  const int64_t V = 16 / (int64_t)es;
  const bool is_float = dtype == FRA_F32 || dtype == FRA_F64;
  const bool automatic = (o.flags & FRA_STATS_AUTO_RANGE) != 0;
  g.src = d_src;
  g.vec = aligned16(d_src, ss, es);
  g.bins = o.bins, g.flags = o.flags, g.nodata = o.nodata;
  g.lo = g.hi = g.scale = 0.0;
  if (o.bins > 0 && !automatic) {
    g.lo = o.hist_lo, g.hi = o.hist_hi;
    const double span = g.hi - g.lo;
    g.scale = g.hi > g.lo ? (double)o.bins / span : 0.0;
    if (!std::isfinite(g.scale)) g.scale = 0.0;
  }
  // (a chunk's slots are counted in 32 bits, and its pixels in an LDS bin)
  if (const int rc = plan_chunks(&g.plan, V, h, w, channels, (int64_t)1 << 31, ((int64_t)1 << 32) - 1, "statistics call"))
    return rc;
  const unsigned grid = g.plan.grid;
  HIPCHK(sc.alloc(&g.partials, (size_t)grid * sizeof(Partial)));
  HIPCHK(sc.alloc(&g.bands, (size_t)channels * sizeof(fra_stats_band)));
  const size_t hist_bytes = (size_t)channels * (size_t)o.bins * sizeof(uint64_t);
  g.hist = nullptr;
  if (o.bins > 0) {
    HIPCHK(sc.alloc(&g.hist, hist_bytes));
    HIPCHK(hipMemsetAsync(g.hist, 0, hist_bytes, s));
  }
  const int hmode = o.bins == 0 ? 0 : 1;
  const bool second = is_float || (o.bins > 0 && automatic);
  const bool fused = o.bins > 0 && !second;  // integers, explicit range: the first window is counted in pass 1
  // the window of bins a launch counts, and its LDS bytes
  auto window = [&](int bin0) {
    g.bin0 = bin0, g.nbins = std::min(kLdsBins, o.bins - bin0);
    return (size_t)g.nbins * sizeof(uint32_t);
  };
  return timed(
      c, &g_stats_ms,
      [&]() -> int {
        {
          const size_t lds = fused ? window(0) : 0;
          launch_dtype(dtype, 1, fused ? hmode : 0, grid, lds, s, g);
          HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_stats_fold, dim3((unsigned)channels), dim3(256), 0, s, g, (int32_t)is_float, (int32_t)fused);
        HIPCHK(hipGetLastError());
        // pass 2 reads the records k_stats_fold wrote: once for fm2, below / above and the first window (then folded),
        // and once more per further window of bins, for its counts alone
        for (int bin0 = fused ? kLdsBins : 0; bin0 == 0 ? second : bin0 < o.bins; bin0 += kLdsBins) {
          const size_t lds = hmode ? window(bin0) : 0;
          launch_dtype(dtype, 2, hmode, grid, lds, s, g);
          HIPCHK(hipGetLastError());
          if (bin0 == 0) {
            hipLaunchKernelGGL(k_stats_fold2, dim3((unsigned)channels), dim3(256), 0, s, g, (int32_t)is_float);
            HIPCHK(hipGetLastError());
          }
          if (!hmode) break;
        }
        return FRA_OK;
      },
      [&]() -> int {
        HIPCHK(hipMemcpyAsync(bands, g.bands, (size_t)channels * sizeof(fra_stats_band), hipMemcpyDeviceToHost, s));
        if (o.bins > 0) HIPCHK(hipMemcpyAsync(hist, g.hist, hist_bytes, hipMemcpyDeviceToHost, s));
        return FRA_OK;
      });
}

int check_opts(const fra_stats_opts* o, const uint64_t* hist) {
  if (o->bins < 0 || o->bins > kMaxBins)
    return fra_internal_set_error(FRA_E_INVALID, "bins %d outside 0 ... %d", o->bins, kMaxBins);
  if (o->flags & ~(FRA_STATS_AUTO_RANGE | FRA_STATS_NODATA))
    return fra_internal_set_error(FRA_E_INVALID, "unknown statistics flags 0x%x", (unsigned)o->flags);
  if (o->bins > 0 && !(o->flags & FRA_STATS_AUTO_RANGE) &&
      !(std::isfinite(o->hist_lo) && std::isfinite(o->hist_hi) && o->hist_lo <= o->hist_hi))
    return fra_internal_set_error(FRA_E_INVALID, "bad histogram range [%g, %g]: finite bounds with lo <= hi are needed",
                                  o->hist_lo, o->hist_hi);
  if (o->bins > 0 && !hist) return fra_internal_set_error(FRA_E_INVALID, "null histogram with %d bins", o->bins);
  return FRA_OK;
}

}  // namespace

extern "C" {

FRA_API int fra_stats_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_stats_ms;
  return FRA_OK;
}

FRA_API int fra_stats(fra_ctx* ctx, const fra_stats_job* job, fra_stats_band* bands, uint64_t* hist) {
  if (!ctx || !job || !bands || !job->src) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  const Strides ss{job->band_stride, job->row_stride, job->col_stride};
  const int32_t ch = job->channels, h = job->height, w = job->width;
  if (const int rc = check_raster(job->dtype, ch, h, w, ss, ss)) return rc;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  if (const int rc = check_opts(&job->opts, hist)) return rc;
  Call c(ctx);
  const void* d_src = nullptr;
  if (const int rc = stage_in(c, job->src, job->src_on_device,
                              (size_t)extent_of(ch, h, w, ss) * (size_t)elem_size(job->dtype), &d_src))
    return rc;
  return run_stats(c, job->dtype, ch, h, w, d_src, ss, job->opts, bands, hist);
}

FRA_API int fra_decode_device_stats(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                    const fra_stats_opts* opts, fra_stats_band* bands, uint64_t* hist,
                                    fra_decoded* infos) {
  if (!ctx || !job || !roi || !opts || !bands || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (const int rc = check_opts(opts, hist)) return rc;
  if (left_to_window_read_no_dst(job, roi)) return refer_to_window_read(ctx, job, roi, infos, true);
  const int32_t h = roi->height, w = roi->width;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region_src(ctx, job, roi, infos, [&](Call& c, const void* d_region, const Strides& ss) {
    return run_stats(c, job->dst_dtype, job->channels, h, w, d_region, ss, *opts, bands, hist);
  });
}

}  // extern "C"
