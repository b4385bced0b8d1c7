// fra_zonal.hip -- zonal statistics: per-zone band statistics of a raster against a zone raster (fra_zonal), and of a
// region of a set of tile streams without the decoded region leaving the GPU (fra_decode_device_zonal).
//
// The rule (include/flac_raster_amd.h): a value raster (channels, h, w) of any dtype and a zone raster (h, w) of an
// integer dtype; a pixel belongs to zone k = z - zone_lo when 0 <= k < nzones (and z is not the ignored label), else it
// is outside; one record per (band, zone) with the counts, extremes and sums of fra_stats over the zone's pixels.
//
// k_zonal<T, Z, PASS>: the chunks and the slot loads of fra_scan.h (the load choice for each raster separately): a
// workgroup is one (band, chunk of rows), a slot is V = 16 / sizeof(T) pixels, the values as one 16-byte load and their
// V zone labels as one load of V * sizeof(Z) bytes (in 16-byte pieces) where the raster allows it, element by element
// otherwise, the next slot in flight while this one is accumulated.  The threads lie on neighbouring slots of a row
// (256 of them, or on several rows of a narrow raster), and each walks down the chunk's rows in its column of slots
// before it moves 256 slots on: unlike the row-major walk of fra_scan.h this keeps a thread inside one zone for as long
// as the zone goes on downwards.  The zone raster is read once per (band, chunk) workgroup, so `channels` times per launch; a
// workgroup over all bands of a chunk would need channels tables in LDS.
//   Runs.  A thread merges the neighbouring pixels of one zone in registers (counts, sum, sq, min, max) and touches
//   shared state once per run; a run goes on from one slot of the thread to its next, so a constant zone raster costs
//   one update per thread, not one per pixel, and a raster of large zones one per slot at the most.
//   The table.  A workgroup owns a table of a window of zones, [win0, win0 + nwin), in LDS: per zone eight uint64 words
//   (valid, nan, nodata, sum, sq_a, sq_b, min, max), stored word by word (word * nwin + zone, so that neighbouring
//   zones lie in neighbouring banks) and updated with LDS atomics: 64-bit adds for the counts and the sum (two's
//   complement: |sum| < 2^63 below 2^32 pixels); unsigned min / max on an order-preserving integer image of the value
//   (integers: sign bit flipped; doubles: all bits flipped when negative, else the sign bit set), so that floats take
//   the same path; x^2 < 2^64 as sq_a += q & 0xffffffff and sq_b += q >> 32, neither of which can wrap below 2^32
//   pixels (dtypes of <= 16 bits have q < 2^32 and add to sq_a alone); floats add x to the f64 sum with an LDS f64
//   atomic.  At its end the workgroup adds its non-empty entries to the call's table in device memory with 64-bit
//   global atomics.  Integer atomics do not depend on the order: everything but fsum / fm2 is exact and deterministic.
//   Windows.  k_zonal_range reads the zone raster once before the passes: per chunk of rows the smallest and the
//   largest zone that occurs in it, and the call's `outside`.  A workgroup's window starts at its own chunk's smallest
//   zone, so zones that are spatially coherent (fields, catchments: a chunk of a few rows meets few of them, whatever
//   nzones is) take one launch; a chunk whose zones span more than a window takes one more launch per window, in
//   which every workgroup whose chunk is done leaves before it reads a pixel.  The host cannot know the widest chunk
//   without a round trip, so it enqueues ceil(nzones / kLdsZones) launches.  (First built with one window position per
//   launch for the whole raster: 1849 zones in blocks of 256 x 256 pixels over the 964 MB scene took four launches that
//   all read the raster, 2.52 ms)
//   PASS 2 (floats): the window's means are copied from the device table into LDS, a run reads its zone's mean there
//   and adds (x - mean)^2 in f64, flushed with an LDS f64 atomic: two words per zone, so a window of 4 x as many zones.
// k_zonal_init fills the table, k_zonal_mean writes mean = fsum / valid per (band, zone) between the passes -- no host
// round trip --, k_zonal_finish turns the table into fra_zonal_rec (NaN extremes for valid == 0, the 128-bit encoding).
//
// kLdsZones = 512: 8 words x 8 bytes x 512 = 32 KiB of LDS per workgroup and no static LDS beside it, so the 160 KiB
// of a CU hold five workgroups of 256 threads (20 waves, 5 per SIMD; the registers, 36 - 104 VGPRs, allow 4 - 8):
// a bandwidth-bound loop with one slot in flight per thread needs at least the four that kLdsBins of fra_stats.hip
// argues for, and an entry here is sixteen times a bin.  kLdsZones2 = 2048 is the same 32 KiB for the second pass.
// Measured numbers and the many-zones decision: DESIGN.md 6c.
//
// Shared with the other units over fra_region.h: the dtype and layout refusal, what is left to the windowed read, the
// staging of host rasters, the decoded region and the timed launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"
#include "fra_scan.h"

static_assert(sizeof(fra_zonal_rec) == 112, "fra_zonal_rec is 112 bytes");
static_assert(sizeof(fra_zonal_opts) == 32, "fra_zonal_opts is 32 bytes");

namespace {

using namespace fra_region;

constexpr int kLdsZones = 512;    // zones a workgroup keeps in LDS in pass 1 (32 KiB)
constexpr int kLdsZones2 = 2048;  // ... and in pass 2 (mean and fm2 per zone: 32 KiB)
constexpr int kMaxZones = 65536;

using u64 = unsigned long long;

enum : int { W_VALID = 0, W_NAN, W_NODATA, W_SUM, W_SQA, W_SQB, W_MIN, W_MAX, kWords };
constexpr int W_FM2 = W_SQA, W_MEAN = W_SQB;  // floats have no integer squares: their table keeps fm2 and the mean there
constexpr u64 kMsb = 0x8000000000000000ull;

struct ZonalArgs {
  const void* src;
  const void* zones;
  int64_t bs, rs, cs;  // element strides of the values: band, row, column
  int64_t zrs, zcs;    // ... and of the zone raster: row, column
  u64* table;          // channels x nzones x kWords
  const uint2* ranges; // per chunk of rows: the smallest and the largest zone that occurs in it (k_zonal_range)
  int64_t zone_lo, ignore_zone;
  double nodata;
  int32_t h, w;
  ChunkPlan plan;               // (its row-major steps are not used: the column walk below)
  uint32_t cols, rstep;         // a workgroup's threads lie on `rstep` rows of `cols` neighbouring slots: cols x rstep <= 256
  int32_t vec, zvec;  // aligned 16-byte loads of the values / aligned vector loads of the zones
  int32_t flags, nzones;
  int32_t wini, wcap;  // this launch keeps window `wini` of `wcap` zones, counted from the chunk's smallest zone
};

// order-preserving images: a < b as values <=> key(a) < key(b) as unsigned integers
__device__ inline u64 key_of(int64_t x) { return (u64)x ^ kMsb; }
__device__ inline u64 key_of(double x) {
  const u64 b = (u64)__double_as_longlong(x);
  return (b & kMsb) ? ~b : (b | kMsb);
}
__device__ inline double value_of_key(u64 k, bool is_float) {
  if (!is_float) return (double)(int64_t)(k ^ kMsb);
  return __longlong_as_double((long long)((k & kMsb) ? (k ^ kMsb) : ~k));
}

__device__ inline void add_f64(u64* word, double v) { unsafeAtomicAdd((double*)word, v); }

// a thread's run: neighbouring pixels of one zone of a slot, merged in registers
template <typename T, int PASS>
struct Run {
  static constexpr bool FLT = std::is_floating_point<T>::value;
  static constexpr int V = 16 / (int)sizeof(T);
  using M = std::conditional_t<FLT, double, int64_t>;
  using S = std::conditional_t<FLT, double, u64>;  // integers: the two's-complement sum, wrapping
  u64* tab = nullptr;  // the workgroup's table in LDS
  uint32_t nwin = 0;
  uint32_t cur = ~0u;  // the run's zone, relative to the window; ~0u: no run
  uint32_t valid = 0, nan = 0, nodata = 0;
  S sum = 0;           // pass 1: sum x; pass 2: sum (x - mean)^2
  u64 sqa = 0, sqb = 0;
  M mn = 0, mx = 0;    // of the valid pixels (set by the first)
  double mean = 0.0;   // pass 2
  Nodata<T> nodata_of;

  __device__ inline void flush() {
    if (cur == ~0u) return;
    if constexpr (PASS == 1) {
      if (valid) {
        atomicAdd(&tab[W_VALID * nwin + cur], (u64)valid);
        if constexpr (FLT) {
          add_f64(&tab[W_SUM * nwin + cur], sum);
        } else {
          atomicAdd(&tab[W_SUM * nwin + cur], sum);
          atomicAdd(&tab[W_SQA * nwin + cur], sqa);
          if constexpr (sizeof(T) == 4) atomicAdd(&tab[W_SQB * nwin + cur], sqb);
        }
        atomicMin(&tab[W_MIN * nwin + cur], key_of(mn));
        atomicMax(&tab[W_MAX * nwin + cur], key_of(mx));
      }
      if constexpr (FLT) {
        if (nan) atomicAdd(&tab[W_NAN * nwin + cur], (u64)nan);
      }
      if (nodata) atomicAdd(&tab[W_NODATA * nwin + cur], (u64)nodata);
    } else {
      if (valid) add_f64(&tab[cur], sum);
    }
    cur = ~0u, valid = nan = nodata = 0, sum = 0, sqa = sqb = 0;
  }

  // a pixel of zone j (window-relative)
  __device__ inline void put(uint32_t j, T v) {
    if (j != cur) {
      flush();
      cur = j;
      if constexpr (PASS == 2) mean = __longlong_as_double((long long)tab[nwin + j]);
    }
    const M x = (M)v;
    if constexpr (FLT) {
      if (x != x) {
        nan++;
        return;
      }
    }
    if (nodata_of.is(x)) {
      nodata++;
      return;
    }
    if constexpr (PASS == 1) {
      mn = (!valid || x < mn) ? x : mn, mx = (!valid || x > mx) ? x : mx;
      if constexpr (FLT) {
        sum = sum + x;
      } else {
        sum += (u64)x;
        const u64 ax = x < 0 ? (u64)-x : (u64)x;  // <= 2^32 - 1
        const u64 q = ax * ax;
        if constexpr (sizeof(T) == 4) sqa += q & 0xffffffffull, sqb += q >> 32;
        else sqa += q;  // q < 2^32
      }
    } else {
      const double d = x - mean;
      sum = sum + d * d;
    }
    valid++;
  }
};

template <typename T, typename Z, int PASS>
__global__ void __launch_bounds__(256) k_zonal(ZonalArgs g) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr bool FLT = std::is_floating_point<T>::value;
  static_assert(PASS == 1 || FLT, "the second pass is the floats'");
  using Vec = VecOf<T, V>;
  using ZVec = VecOf<Z, V>;
  extern __shared__ u64 s_tab[];  // pass 1: kWords x nwin; pass 2: fm2 and the mean, 2 x nwin
  const Chunk c = chunk_of(g.plan, g.h, blockIdx.x);
  const int64_t band = c.band;
  const uint32_t chunk = c.chunk, rows = c.rows;
  const T* __restrict__ ps = (const T*)g.src + (band * g.bs + c.row0 * g.rs);
  const Z* __restrict__ pz = (const Z*)g.zones + c.row0 * g.zrs;
  const bool vec = g.vec != 0, zvec = g.zvec != 0;
  // the window of this launch: `wcap` zones from the chunk's smallest zone on, cut at its largest.  A window that no
  // zone of the chunk reaches has nothing to add: the whole workgroup leaves before it reads a pixel
  const uint2 range = g.ranges[chunk];
  const u64 first = (u64)range.x + (u64)g.wini * (u64)g.wcap;
  if (range.x > range.y || first > range.y) return;
  const uint32_t win0 = (uint32_t)first, nwin = min((uint32_t)g.wcap, range.y - win0 + 1);
  u64* const entries = g.table + ((band * (int64_t)g.nzones + win0) * kWords);
  if constexpr (PASS == 1) {
    for (int wd = 0; wd < kWords; wd++)
      for (uint32_t j = threadIdx.x; j < nwin; j += 256) s_tab[wd * nwin + j] = wd == W_MIN ? ~0ull : 0ull;
  } else {
    for (uint32_t j = threadIdx.x; j < nwin; j += 256) s_tab[j] = 0ull, s_tab[nwin + j] = entries[(size_t)j * kWords + W_MEAN];
  }
  __syncthreads();

  Run<T, PASS> run;
  run.tab = s_tab, run.nwin = nwin;
  run.nodata_of.set((g.flags & FRA_ZONAL_NODATA) != 0, g.nodata);
  const bool ignore = (g.flags & FRA_ZONAL_IGNORE) != 0;

  auto slot = [&](const Vec& x, const ZVec& z, int n) {
#pragma unroll
    for (int i = 0; i < V; i++) {
      if (i < n) {
        const int64_t zi = (int64_t)z.v[i];
        if (ignore && zi == g.ignore_zone) continue;
        // the difference modulo 2^64: inside the window (which lies inside the zones) exactly when j < nwin
        const u64 j = (u64)zi - (u64)g.zone_lo - (u64)win0;
        if (j < (u64)nwin) run.put((uint32_t)j, x.v[i]);  // (outside, or a zone of another window: that window's launch)
      }
    }
  };

  // A thread's slots: it walks down the rows of the chunk in one column of slots, then in the next column `cols`
  // further on, so that its run goes on from row to row where the zones do.  (A wave still reads neighbouring slots
  // of a row.)  The threads past cols x rstep have no slot.
  const uint32_t rl = threadIdx.x / g.cols;
  uint32_t row = rl, cv = threadIdx.x % g.cols;  // (cols <= nvec: the first column exists)
  Vec nx{};
  ZVec nz{};
  int nn = 0;
  auto issue = [&]() {  // the loads of slot (row, cv) of the chunk: pixels [cv V, cv V + nn) of its row
    nn = slot_count<V>(g.w, cv);
    nx = load_slot<T, V>(ps + ((int64_t)row * g.rs + (int64_t)cv * V * g.cs), g.cs, vec, nn);
    nz = load_slot<Z, V>(pz + ((int64_t)row * g.zrs + (int64_t)cv * V * g.zcs), g.zcs, zvec, nn);
  };
  bool have = rl < g.rstep && rl < rows;
  if (have) issue();
  while (have) {
    const Vec cx = nx;
    const ZVec cz = nz;
    const int cn = nn;
    row += g.rstep;
    if (row >= rows) row = rl, cv += g.cols;
    have = cv < g.plan.nvec;
    if (have) issue();  // in flight while the current slot is accumulated
    slot(cx, cz, cn);
  }
  run.flush();      // a run goes on from one slot of the thread to its next: a constant zone raster, one update per thread
  __syncthreads();  // the workgroup's table is complete
  for (uint32_t j = threadIdx.x; j < nwin; j += 256) {
    u64* const e = entries + (size_t)j * kWords;
    if constexpr (PASS == 1) {
      const u64 valid = s_tab[W_VALID * nwin + j], nan = s_tab[W_NAN * nwin + j], nodata = s_tab[W_NODATA * nwin + j];
      if (valid) {
        atomicAdd(&e[W_VALID], valid);
        if constexpr (FLT) {
          add_f64(&e[W_SUM], __longlong_as_double((long long)s_tab[W_SUM * nwin + j]));
        } else {
          atomicAdd(&e[W_SUM], s_tab[W_SUM * nwin + j]);
          atomicAdd(&e[W_SQA], s_tab[W_SQA * nwin + j]);
          if constexpr (sizeof(T) == 4) atomicAdd(&e[W_SQB], s_tab[W_SQB * nwin + j]);
        }
        atomicMin(&e[W_MIN], s_tab[W_MIN * nwin + j]);
        atomicMax(&e[W_MAX], s_tab[W_MAX * nwin + j]);
      }
      if (nan) atomicAdd(&e[W_NAN], nan);
      if (nodata) atomicAdd(&e[W_NODATA], nodata);
    } else {
      const double f = __longlong_as_double((long long)s_tab[j]);
      if (f != 0.0) add_f64(&e[W_FM2], f);  // (NaN != 0.0)
    }
  }
}

// The zone raster alone, before the passes: `parts` workgroups per chunk of rows (the chunks of k_zonal) find the
// smallest and the largest zone that occurs in it (kmin > kmax: none) and add its pixels that lie in no zone to
// *outside.  Slots of 16 bytes, thread t of part p owns slots p 256 + t, + parts x 256, ... of the chunk.
template <typename Z>
__global__ void __launch_bounds__(256) k_zonal_range(ZonalArgs g, uint2* ranges, u64* outside, uint32_t parts) {
  constexpr int VZ = 16 / (int)sizeof(Z);
  using ZVec = VecOf<Z, VZ>;
  __shared__ uint32_t s_min, s_max;
  __shared__ u64 s_out;
  const uint32_t chunk = blockIdx.x / parts, part = blockIdx.x % parts;
  const Chunk c = chunk_at(g.plan, g.h, chunk);
  const uint32_t rows = c.rows;
  const Z* __restrict__ pz = (const Z*)g.zones + c.row0 * g.zrs;
  const bool ignore = (g.flags & FRA_ZONAL_IGNORE) != 0, zvec = g.zvec != 0;
  if (threadIdx.x == 0) s_min = ~0u, s_max = 0, s_out = 0;
  __syncthreads();
  const u64 nvz = ((u64)g.w + VZ - 1) / VZ, total = nvz * rows;
  uint32_t kmin = ~0u, kmax = 0;
  u64 out = 0;
  for (u64 idx = (u64)part * 256 + threadIdx.x; idx < total; idx += (u64)parts * 256) {
    const u64 r = idx / nvz, cv = idx % nvz;
    const int n = slot_count<VZ>(g.w, (uint32_t)cv);
    const ZVec v = load_slot<Z, VZ>(pz + ((int64_t)r * g.zrs + (int64_t)cv * VZ * g.zcs), g.zcs, zvec, n);
#pragma unroll
    for (int i = 0; i < VZ; i++) {
      if (i < n) {
        const int64_t zi = (int64_t)v.v[i];
        const u64 k = (u64)zi - (u64)g.zone_lo;  // modulo 2^64: in range exactly when 0 <= z - zone_lo < nzones
        if ((ignore && zi == g.ignore_zone) || k >= (u64)g.nzones) out++;
        else kmin = min(kmin, (uint32_t)k), kmax = max(kmax, (uint32_t)k);
      }
    }
  }
  if (out) atomicAdd(&s_out, out);
  if (kmin <= kmax) atomicMin(&s_min, kmin), atomicMax(&s_max, kmax);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_min <= s_max) atomicMin(&ranges[chunk].x, s_min), atomicMax(&ranges[chunk].y, s_max);
    if (s_out) atomicAdd(outside, s_out);
  }
}

// the call's table, the chunks' ranges and the counter before the first launch
__global__ void __launch_bounds__(256) k_zonal_init(u64* table, u64* misc, uint32_t entries, uint2* ranges, uint32_t nchunks) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) misc[0] = 0ull;
  if (i < nchunks) ranges[i] = make_uint2(~0u, 0u);
  if (i >= entries) return;
  u64* e = table + (size_t)i * kWords;
  for (int wd = 0; wd < kWords; wd++) e[wd] = wd == W_MIN ? ~0ull : 0ull;
}

// floats, between the passes: mean = fsum / valid of every (band, zone), one IEEE division (0 / 0 = NaN)
__global__ void __launch_bounds__(256) k_zonal_mean(u64* table, uint32_t entries) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= entries) return;
  u64* e = table + (size_t)i * kWords;
  const double mean = __longlong_as_double((long long)e[W_SUM]) / (double)e[W_VALID];
  e[W_MEAN] = (u64)__double_as_longlong(mean);
}

__global__ void __launch_bounds__(256) k_zonal_finish(const u64* table, const u64* misc, uint32_t entries, int32_t is_float,
                                                      int32_t is_signed, fra_zonal_rec* recs, uint64_t* outside) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *outside = misc[0];
  if (i >= entries) return;
  const u64* e = table + (size_t)i * kWords;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  fra_zonal_rec r;
  r.valid = e[W_VALID], r.nan = e[W_NAN], r.nodata = e[W_NODATA];
  r.count = r.valid + r.nan + r.nodata;
  r.min = r.valid ? value_of_key(e[W_MIN], is_float != 0) : nan;
  r.max = r.valid ? value_of_key(e[W_MAX], is_float != 0) : nan;
  if (is_float) {
    r.sum_lo = 0, r.sum_hi = 0, r.sq_lo = r.sq_hi = 0;
    r.fsum = __longlong_as_double((long long)e[W_SUM]);
    r.mean = __longlong_as_double((long long)e[W_MEAN]);
    r.fm2 = __longlong_as_double((long long)e[W_FM2]);
  } else {
    r.sum_lo = e[W_SUM];
    r.sum_hi = is_signed && (int64_t)e[W_SUM] < 0 ? -1 : 0;  // |sum| < 2^63 (signed), sum < 2^64 (unsigned)
    const u64 a = e[W_SQA], b = e[W_SQB];  // sq = a + b 2^32
    r.sq_lo = a + (b << 32);
    r.sq_hi = (b >> 32) + (r.sq_lo < a);
    r.fsum = r.mean = r.fm2 = 0.0;
  }
  r.reserved = 0;
  recs[i] = r;
}

thread_local float g_zonal_ms = 0.f;

constexpr const char* kNot = "described in one zonal call";  // (too_many_pixels)
constexpr int64_t kMaxRecords = (int64_t)1 << 24;  // (band, zone) records of a call: a table of 1 GiB

template <typename T, typename Z>
void launch_pass(int pass, unsigned grid, size_t lds, hipStream_t s, const ZonalArgs& g) {
  if (pass == 1) {
    hipLaunchKernelGGL((k_zonal<T, Z, 1>), dim3(grid), dim3(256), lds, s, g);
  } else if constexpr (std::is_floating_point<T>::value) {
    hipLaunchKernelGGL((k_zonal<T, Z, 2>), dim3(grid), dim3(256), lds, s, g);
  }
}

void launch_dtypes(int dtype, int zdtype, int pass, unsigned grid, size_t lds, hipStream_t s, const ZonalArgs& g) {
  with_dtype(dtype, [&](auto t) {
    with_int_dtype(zdtype, [&](auto z) { launch_pass<decltype(t), decltype(z)>(pass, grid, lds, s, g); });
  });
}

// the zonal kernels over a (channels, h, w) device raster and an (h, w) device zone raster, timed, the records to
// `recs` and the count to `outside` on the host (the table and the device records belong to the call)
int run_zonal(Call& c, int dtype, int channels, int32_t h, int32_t w, const void* d_src, const Strides& ss, int zdtype,
              const void* d_zones, int64_t zrs, int64_t zcs, const fra_zonal_opts& o, fra_zonal_rec* recs,
              uint64_t* outside) {
  hipStream_t s = c.s;
  HipArena& sc = c.sc;
  ZonalArgs g{};
  g.src = d_src, g.zones = d_zones;
  g.bs = ss.band, g.rs = ss.row, g.cs = ss.col, g.zrs = zrs, g.zcs = zcs;
  g.h = h, g.w = w;
  g.zone_lo = o.zone_lo, g.ignore_zone = o.ignore_zone, g.nodata = o.nodata, g.flags = o.flags, g.nzones = o.nzones;
  const size_t es = (size_t)elem_size(dtype), zes = (size_t)elem_size(zdtype);
  const int64_t V = 16 / (int64_t)es;
  const bool is_float = dtype == FRA_F32 || dtype == FRA_F64;
  const bool is_signed = dtype == FRA_I8 || dtype == FRA_I16 || dtype == FRA_I32;
  g.vec = aligned16(d_src, ss, es);
  g.zvec = aligned16(d_zones, Strides{0, zrs, zcs}, zes);
  // (a chunk's slots are counted in 32 bits)
  if (const int rc = plan_chunks(&g.plan, V, h, w, channels, (int64_t)1 << 31, 0, "zonal call")) return rc;
  const unsigned grid = g.plan.grid;
  const int64_t nchunks = g.plan.nchunks;
  g.cols = std::min<uint32_t>(g.plan.nvec, 256), g.rstep = 256 / g.cols;
  const uint32_t entries = (uint32_t)channels * (uint32_t)o.nzones;  // (checked: too_many_records)
  HIPCHK(sc.alloc(&g.table, (size_t)entries * kWords * sizeof(u64)));
  u64* d_misc = nullptr;  // the pixels outside every zone
  uint2* d_ranges = nullptr;
  HIPCHK(sc.alloc(&d_misc, sizeof(u64)));
  HIPCHK(sc.alloc(&d_ranges, (size_t)nchunks * sizeof(uint2)));
  g.ranges = d_ranges;
  fra_zonal_rec* d_recs = nullptr;
  uint64_t* d_outside = nullptr;
  HIPCHK(sc.alloc(&d_recs, (size_t)entries * sizeof(fra_zonal_rec)));
  HIPCHK(sc.alloc(&d_outside, sizeof(uint64_t)));
  const unsigned egrid = (entries + 255) / 256;
  const unsigned igrid = (std::max(entries, (uint32_t)nchunks) + 255) / 256;
  const uint32_t parts = (uint32_t)std::max<int64_t>(1, (kBlocks + nchunks - 1) / nchunks);  // of a chunk, for k_zonal_range
  return timed(
      c, &g_zonal_ms,
      [&]() -> int {
        hipLaunchKernelGGL(k_zonal_init, dim3(igrid), dim3(256), 0, s, g.table, d_misc, entries, d_ranges, (uint32_t)nchunks);
        HIPCHK(hipGetLastError());
        with_int_dtype(zdtype, [&](auto z) {
          hipLaunchKernelGGL(k_zonal_range<decltype(z)>, dim3((unsigned)nchunks * parts), dim3(256), 0, s, g, d_ranges, d_misc,
                             parts);
        });
        HIPCHK(hipGetLastError());
        // a chunk's zones, from its smallest to its largest, take one launch per window: as many launches as the
        // widest chunk could need; in the others its workgroups leave at once
        g.wcap = std::min(kLdsZones, o.nzones);
        for (g.wini = 0; g.wini * kLdsZones < o.nzones; g.wini++) {
          launch_dtypes(dtype, zdtype, 1, grid, (size_t)g.wcap * kWords * sizeof(u64), s, g);
          HIPCHK(hipGetLastError());
        }
        if (is_float) {
          hipLaunchKernelGGL(k_zonal_mean, dim3(egrid), dim3(256), 0, s, g.table, entries);
          HIPCHK(hipGetLastError());
          g.wcap = std::min(kLdsZones2, o.nzones);
          for (g.wini = 0; g.wini * kLdsZones2 < o.nzones; g.wini++) {
            launch_dtypes(dtype, zdtype, 2, grid, (size_t)g.wcap * 2 * sizeof(u64), s, g);
            HIPCHK(hipGetLastError());
          }
        }
        hipLaunchKernelGGL(k_zonal_finish, dim3(egrid), dim3(256), 0, s, (const u64*)g.table, (const u64*)d_misc, entries,
                           (int32_t)is_float, (int32_t)is_signed, d_recs, d_outside);
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&]() -> int {
        HIPCHK(hipMemcpyAsync(recs, d_recs, (size_t)entries * sizeof(fra_zonal_rec), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(outside, d_outside, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        return FRA_OK;
      });
}

int too_many_records(int64_t channels, int64_t nzones) {
  if (channels * nzones <= kMaxRecords) return FRA_OK;
  return fra_internal_set_error(FRA_E_INVALID, "%lld bands x %lld zones are more than 2^24 records in one zonal call",
                                (long long)channels, (long long)nzones);
}

int check_zones(int zone_dtype, int64_t zrs, int64_t zcs) {
  if (!is_int_dtype(zone_dtype))
    return fra_internal_set_error(FRA_E_INVALID, "bad zone dtype %d: an integer dtype of at most 32 bits is needed", zone_dtype);
  if (zrs < 0 || zcs < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad zone layout (strides %lld, %lld)", (long long)zrs, (long long)zcs);
  return FRA_OK;
}

int check_opts(const fra_zonal_opts* o) {
  if (o->nzones < 1 || o->nzones > kMaxZones)
    return fra_internal_set_error(FRA_E_INVALID, "nzones %d outside 1 ... %d", o->nzones, kMaxZones);
  if (o->flags & ~(FRA_ZONAL_NODATA | FRA_ZONAL_IGNORE))
    return fra_internal_set_error(FRA_E_INVALID, "unknown zonal flags 0x%x", (unsigned)o->flags);
  return FRA_OK;
}

}  // namespace

extern "C" {

FRA_API int fra_zonal_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_zonal_ms;
  return FRA_OK;
}

FRA_API int fra_zonal(fra_ctx* ctx, const fra_zonal_job* job, fra_zonal_rec* recs, uint64_t* outside) {
  if (!ctx || !job || !recs || !outside || !job->src || !job->zones)
    return fra_internal_set_error(FRA_E_INVALID, "null argument");
  const Strides ss{job->band_stride, job->row_stride, job->col_stride};
  const int32_t ch = job->channels, h = job->height, w = job->width;
  if (const int rc = check_raster(job->dtype, ch, h, w, ss, ss)) return rc;
  if (const int rc = check_zones(job->zone_dtype, job->zone_row_stride, job->zone_col_stride)) return rc;
  if (const int rc = check_opts(&job->opts)) return rc;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  if (const int rc = too_many_records(ch, job->opts.nzones)) return rc;
  Call c(ctx);
  const void *d_src = nullptr, *d_zones = nullptr;
  if (const int rc = stage_in(c, job->src, job->src_on_device,
                              (size_t)extent_of(ch, h, w, ss) * (size_t)elem_size(job->dtype), &d_src))
    return rc;
  const Strides zs{0, job->zone_row_stride, job->zone_col_stride};
  if (const int rc = stage_in(c, job->zones, job->zones_on_device,
                              (size_t)extent_of(1, h, w, zs) * (size_t)elem_size(job->zone_dtype), &d_zones))
    return rc;
  return run_zonal(c, job->dtype, ch, h, w, d_src, ss, job->zone_dtype, d_zones, zs.row, zs.col, job->opts, recs, outside);
}

FRA_API int fra_decode_device_zonal(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, const void* zones,
                                    int32_t zones_on_device, int32_t zone_dtype, int64_t zone_row_stride,
                                    int64_t zone_col_stride, const fra_zonal_opts* opts, fra_zonal_rec* recs,
                                    uint64_t* outside, fra_decoded* infos) {
  if (!ctx || !job || !roi || !zones || !opts || !recs || !outside || !infos)
    return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (const int rc = check_zones(zone_dtype, zone_row_stride, zone_col_stride)) return rc;
  if (const int rc = check_opts(opts)) return rc;
  if (left_to_window_read_no_dst(job, roi)) return refer_to_window_read(ctx, job, roi, infos, true);
  const int32_t h = roi->height, w = roi->width;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region_src(ctx, job, roi, infos, [&](Call& c, const void* d_region, const Strides& ss) -> int {
    const Strides zs{0, zone_row_stride, zone_col_stride};
    const void* d_zones = nullptr;
    if (const int rc = stage_in(c, zones, zones_on_device, (size_t)extent_of(1, h, w, zs) * (size_t)elem_size(zone_dtype),
                                &d_zones))
      return rc;
    return run_zonal(c, job->dst_dtype, job->channels, h, w, d_region, ss, zone_dtype, d_zones, zs.row, zs.col, *opts, recs,
                     outside);
  });
}

}  // extern "C"
