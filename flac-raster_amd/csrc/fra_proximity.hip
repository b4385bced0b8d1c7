// fra_proximity.hip -- the exact Euclidean distance transform and nearest-target allocation over a raster or a decoded
// region (include/flac_raster_amd.h, "Proximity"; the rule in numpy: flac_raster/proximity.py).  The transform is
// separable, and every band goes through two phases on one band's 16-bit intermediate:
//
//   Columns.  k_prox_mask reads the source once: a thread takes 64 rows of one column (lanes on adjacent columns, so a
//   wave reads whole rows) into a 64-bit target mask and the workgroup's target count goes to a word of its own.
//   k_prox_carry walks the masks of a column down and up and leaves, per chunk of the output window's rows, the last
//   target row before the chunk and the first one after it.  k_prox_cols combines both with the mask by bit scans: per
//   pixel the vertical distance g to the nearest target of its column, above winning a tie, "none" beyond the reach.
//
//   Rows.  k_prox_rows holds an output row's intermediate in LDS and finds, per output pixel c, the leftmost column j
//   that minimises g[j]^2 + (c - j)^2.  That argmin does not decrease with c (the costs are Monge, and a "none" column
//   costs more than any other), so level L of a divide and conquer solves the pixels (2 i + 1) 2^(levels - 1 - L) - 1
//   between the argmins of their solved neighbours.  A short range is scanned by 8 lanes, a long one is queued and
//   scanned by a whole wave; a level's ranges overlap in end points only, so a level costs w + (its pixels) candidates
//   whatever the content.  The last pass turns every argmin into d2, the distance and the allocated value.
//
// Shared with the other units over fra_region.h: the layout refusal, what is left to the windowed read, staging, the
// decode of a region and to_out.  The refusals, the reach threshold and the launch plan are in fra_proximity.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "fra_proximity.h"

namespace {

using namespace fra_region;
using namespace fra_px;

struct ProxArgs {
  const void* src;           // element (row 0, col 0) of the band
  int64_t srs, scs;          // of the source, in elements
  int32_t h, w;              // the region
  int32_t r0, c0, oh, ow;    // the output window
  int32_t k0, k1, nchunks;   // chunks of 64 rows: those of the output window's rows, and all
  int32_t nvalues;
  double values[16];
  uint32_t t2, gmax;         // the greatest d2 within reach and floor(sqrt) of it
  unsigned long long* mask;  // nchunks x w
  int32_t* up;               // (k1 - k0 + 1) x w: the last target row before the chunk, -1 without one
  int32_t* dn;               // ... the first target row after it, -1 without one
  uint16_t* g;               // oh x w: g << 1 | below, kNone
  uint32_t* targets;         // per workgroup of k_prox_mask
  uint32_t* reached;         // per workgroup of k_prox_rows
  // the outputs of the band (null: not wanted), the fills as the output's bits
  void* dist; int32_t ddtype; int64_t drs, dcs; double scale, fixed; int32_t has_fixed; unsigned long long dist_fill;
  void* alloc; int64_t ars, acs; unsigned long long alloc_fill;
  Plan plan;
};

// the workgroup's sum of `v` into out[its index]: a word of its own
__device__ inline void wg_sum_to(uint32_t v, uint32_t* out, uint32_t index) {
  const uint32_t total = wg_sum(v);
  if (threadIdx.x == 0) out[index] = total;
}

// grid (col_blocks, nchunks): the target mask of 64 rows of a column per thread
template <typename T>
__global__ void __launch_bounds__(256) k_prox_mask(ProxArgs a) {
  const int32_t c = (int32_t)(blockIdx.x * 256u + threadIdx.x), k = (int32_t)blockIdx.y;
  unsigned long long m = 0;
  if (c < a.w) {
    const int32_t ra = k * kChunkRows, n = min(kChunkRows, a.h - ra);
    const T* p = (const T*)a.src + (int64_t)ra * a.srs + (int64_t)c * a.scs;
    for (int32_t i = 0; i < n; i++) m |= (unsigned long long)is_target(p[(int64_t)i * a.srs], a.nvalues, a.values) << i;
    a.mask[(int64_t)k * a.w + c] = m;
  }
  wg_sum_to((uint32_t)__popcll(m), a.targets, blockIdx.y * gridDim.x + blockIdx.x);
}

// grid (col_blocks): a thread per column walks the chunks down, then up
__global__ void __launch_bounds__(256) k_prox_carry(ProxArgs a) {
  const int32_t c = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (c >= a.w) return;
  int32_t last = -1;
  for (int32_t k = 0; k <= a.k1; k++) {
    if (k >= a.k0) a.up[(int64_t)(k - a.k0) * a.w + c] = last;
    const unsigned long long m = a.mask[(int64_t)k * a.w + c];
    if (m) last = k * kChunkRows + 63 - __clzll((long long)m);
  }
  int32_t next = -1;
  for (int32_t k = a.nchunks - 1; k >= a.k0; k--) {
    if (k <= a.k1) a.dn[(int64_t)(k - a.k0) * a.w + c] = next;
    const unsigned long long m = a.mask[(int64_t)k * a.w + c];
    if (m) next = k * kChunkRows + __ffsll((long long)m) - 1;
  }
}

// grid (col_blocks, k1 - k0 + 1): the intermediate of the chunk's rows inside the output window
__global__ void __launch_bounds__(256) k_prox_cols(ProxArgs a) {
  const int32_t c = (int32_t)(blockIdx.x * 256u + threadIdx.x), kk = (int32_t)blockIdx.y, k = a.k0 + kk;
  if (c >= a.w) return;
  const unsigned long long m = a.mask[(int64_t)k * a.w + c];
  const int32_t u = a.up[(int64_t)kk * a.w + c], d = a.dn[(int64_t)kk * a.w + c];
  const int32_t ia = max(0, a.r0 - k * kChunkRows), ib = min(kChunkRows, a.r0 + a.oh - k * kChunkRows);
  constexpr int32_t kFar = 0x7fffffff;
  for (int32_t i = ia; i < ib; i++) {
    const int32_t r = k * kChunkRows + i;
    const unsigned long long ma = m & (~0ull >> (63 - i)), mb = m >> i;  // the targets at or above row r, at or below it
    const int32_t ga = ma ? i - (63 - __clzll((long long)ma)) : (u >= 0 ? r - u : kFar);
    const int32_t gb = mb ? __ffsll((long long)mb) - 1 : (d >= 0 ? d - r : kFar);
    const int32_t g = min(ga, gb);
    a.g[(int64_t)(r - a.r0) * a.w + c] = (uint32_t)g > a.gmax ? kNone : (uint16_t)(g << 1 | (gb < ga));
  }
}

// the least key of `width` neighbouring lanes (a power of two), in all of them
__device__ inline unsigned long long min_over(unsigned long long key, int width) {
  for (int m = width >> 1; m >= 1; m >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, m, 64);
    key = o < key ? o : key;
  }
  return key;
}

// The least cost << 16 | column over the columns j0, j0 + stride, ... <= hi of the row's intermediate for the pixel of
// region column c; a range of "none" columns gives the key of lo at the greatest cost.
__device__ inline unsigned long long scan_range(const uint16_t* sg, int32_t c, int32_t lo, int32_t j0, int32_t hi, int32_t stride) {
  unsigned long long key = 0xffffffffull << 16 | (unsigned long long)lo;
  for (int32_t j = j0; j <= hi; j += stride) {
    const uint32_t gv = sg[j];
    if (gv == kNone) continue;
    const uint32_t g = gv >> 1, dx = (uint32_t)abs(c - j);
    const unsigned long long k2 = (unsigned long long)(g * g + dx * dx) << 16 | (unsigned long long)j;
    key = k2 < key ? k2 : key;
  }
  return key;
}

// grid (row_wgs): rows_per_wg output rows per workgroup, a team of team_threads threads each.  U moves the bits of a
// source element to the allocation output.
template <typename U>
__global__ void __launch_bounds__(256) k_prox_rows(ProxArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  const Plan& pl = a.plan;
  const int32_t ts = pl.team_threads, tid = (int32_t)threadIdx.x, team = tid / ts, tl = tid % ts;
  const int32_t row = (int32_t)blockIdx.x * pl.rows_per_wg + team;  // of the output window
  const bool live = row < a.oh;
  unsigned char* const base = lds + (size_t)team * pl.team_bytes;
  uint16_t* const sg = (uint16_t*)(base + pl.g_off);
  uint16_t* const so = (uint16_t*)(base + pl.opt_off);
  uint16_t* const sq = (uint16_t*)(base + pl.queue_off);
  uint32_t* const qn = (uint32_t*)(base + pl.count_off);  // two counters: a level's, and the next level's being reset
  const int32_t w = a.w, ow = a.ow;

  for (int32_t j = tl; j < w; j += ts) sg[j] = live ? a.g[(int64_t)row * w + j] : kNone;
  if (tl < 2) qn[tl] = 0;
  __syncthreads();

  const int32_t sub = tl / kSub, sl = tl % kSub, lane = tl & 63, wave = tl >> 6, nwaves = ts >> 6;
  for (int32_t L = 0; L < pl.levels; L++) {
    const int32_t step = 1 << (pl.levels - 1 - L), npix = (ow / step + 1) / 2;
    uint32_t* const cnt = qn + (L & 1);
    // short ranges: 8 lanes per pixel
    for (int32_t b = 0; b < npix; b += ts / kSub) {
      const int32_t i = b + sub, p = (2 * i + 1) * step - 1;
      bool scan = false;
      int32_t lo = 0, hi = -1;
      if (i < npix) {
        lo = p - step >= 0 ? (int32_t)so[p - step] : 0;
        hi = p + step < ow ? (int32_t)so[p + step] : w - 1;
        scan = hi - lo < kLong;
        if (!scan && sl == 0) {
          const uint32_t slot = atomicAdd(cnt, 1u);
          if (slot < pl.queue_cap) sq[slot] = (uint16_t)i;
        }
      }
      unsigned long long key = ~0ull;
      if (scan) key = scan_range(sg, a.c0 + p, lo, lo + sl, hi, kSub);
      key = min_over(key, kSub);
      if (scan && sl == 0) so[p] = (uint16_t)key;
    }
    __syncthreads();
    // long ranges: a wave per pixel
    const int32_t nq = (int32_t)min(*cnt, pl.queue_cap);
    if (tl == 0) qn[(L + 1) & 1] = 0;
    for (int32_t q = wave; q < nq; q += nwaves) {
      const int32_t i = sq[q], p = (2 * i + 1) * step - 1;
      const int32_t lo = p - step >= 0 ? (int32_t)so[p - step] : 0;
      const int32_t hi = p + step < ow ? (int32_t)so[p + step] : w - 1;
      const unsigned long long key = min_over(scan_range(sg, a.c0 + p, lo, lo + lane, hi, 64), 64);
      if (lane == 0) so[p] = (uint16_t)key;
    }
    __syncthreads();
  }

  // every argmin into the outputs
  uint32_t nreach = 0;
  if (live) {
    const int32_t r = a.r0 + row;
    for (int32_t p = tl; p < ow; p += ts) {
      const int32_t j = so[p], c = a.c0 + p;
      const uint32_t gv = sg[j], g = gv >> 1, dx = (uint32_t)abs(c - j), d2 = g * g + dx * dx;
      const bool reach = gv != kNone && d2 <= a.t2;
      nreach += reach;
      if (a.dist) {
        const double d = a.has_fixed ? a.fixed : sqrt((double)d2) * a.scale;
        const int64_t off = (int64_t)row * a.drs + (int64_t)p * a.dcs;
        const unsigned long long f = a.dist_fill;
        switch (a.ddtype) {
          case FRA_U8: ((uint8_t*)a.dist)[off] = reach ? to_out<uint8_t>(d) : (uint8_t)f; break;
          case FRA_I8: ((int8_t*)a.dist)[off] = reach ? to_out<int8_t>(d) : (int8_t)(uint8_t)f; break;
          case FRA_U16: ((uint16_t*)a.dist)[off] = reach ? to_out<uint16_t>(d) : (uint16_t)f; break;
          case FRA_I16: ((int16_t*)a.dist)[off] = reach ? to_out<int16_t>(d) : (int16_t)(uint16_t)f; break;
          case FRA_U32: ((uint32_t*)a.dist)[off] = reach ? to_out<uint32_t>(d) : (uint32_t)f; break;
          case FRA_I32: ((int32_t*)a.dist)[off] = reach ? to_out<int32_t>(d) : (int32_t)(uint32_t)f; break;
          case FRA_F32: ((float*)a.dist)[off] = reach ? to_out<float>(d) : __uint_as_float((uint32_t)f); break;
          default: ((double*)a.dist)[off] = reach ? to_out<double>(d) : __longlong_as_double((long long)f); break;
        }
      }
      if (a.alloc) {
        const int32_t tr = (gv & 1u) ? r + (int32_t)g : r - (int32_t)g;  // the nearest target's row
        const U v = reach ? ((const U*)a.src)[(int64_t)tr * a.srs + (int64_t)j * a.scs] : (U)a.alloc_fill;
        ((U*)a.alloc)[(int64_t)row * a.ars + (int64_t)p * a.acs] = v;
      }
    }
  }
  wg_sum_to(nreach, a.reached, blockIdx.x);
}

// out[x] = the sum of the n words of list x (one workgroup each)
__global__ void __launch_bounds__(256) k_prox_fold(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb, unsigned long long* out) {
  const uint32_t tid = threadIdx.x, n = blockIdx.x ? nb : na;
  const uint32_t* const p = blockIdx.x ? b : a;
  unsigned long long s = 0;
  for (uint32_t i = tid; i < n; i += 256u) s += p[i];
  const unsigned long long total = wg_sum(s);
  if (tid == 0) out[blockIdx.x] = total;
}

thread_local float g_prox_ms[2] = {0.f, 0.f};

// f(U{}) for the unsigned type of an element size
template <typename F>
void with_bits(size_t es, F&& f) {
  switch (es) {
    case 1: f(uint8_t{}); break;
    case 2: f(uint16_t{}); break;
    case 4: f(uint32_t{}); break;
    default: f(uint64_t{}); break;
  }
}

// Both phases over every band of a (channels, h, w) device source of `sdtype` into the staged outputs, then the counts.
int run_proximity(Call& c, const fra_proximity_opts& o, int sdtype, int32_t channels, int32_t h, int32_t w, const void* src,
                  const Strides& ss, const StagedOut& dist, const StagedOut& alloc, uint64_t* counts) {
  const Plan pl = make_plan(h, w, o);
  const size_t es = (size_t)elem_size(sdtype);
  ProxArgs a{};
  a.srs = ss.row, a.scs = ss.col, a.h = h, a.w = w;
  a.r0 = o.out_row_off, a.c0 = o.out_col_off, a.oh = o.out_height, a.ow = o.out_width;
  a.k0 = pl.k0, a.k1 = pl.k1, a.nchunks = pl.nchunks;
  a.nvalues = o.nvalues;
  std::memcpy(a.values, o.values, sizeof(a.values));
  const int64_t t2 = reach_threshold(o.has_max_dist != 0, o.scale, o.max_dist);
  a.t2 = (uint32_t)t2, a.gmax = (uint32_t)isqrt(t2);
  a.scale = o.scale, a.fixed = o.fixed, a.has_fixed = o.has_fixed != 0;
  a.ddtype = o.dist.dtype, a.drs = o.dist.row_stride, a.dcs = o.dist.col_stride;
  a.ars = o.alloc.row_stride, a.acs = o.alloc.col_stride;
  if (dist.dev) a.dist_fill = out_bits(o.dist.dtype, o.fill);
  if (alloc.dev) a.alloc_fill = out_bits(sdtype, o.alloc_fill);
  a.plan = pl;

  const int64_t kchunks = pl.k1 - pl.k0 + 1;
  const uint32_t nmask = (uint32_t)pl.col_blocks * (uint32_t)pl.nchunks, nrows = (uint32_t)pl.row_wgs;  // workgroups per band
  uint32_t *d_targets = nullptr, *d_reached = nullptr;
  unsigned long long* d_sums = nullptr;
  HIPCHK(c.sc.alloc(&a.mask, (size_t)pl.nchunks * (size_t)w * sizeof(unsigned long long)));
  HIPCHK(c.sc.alloc(&a.up, (size_t)kchunks * (size_t)w * sizeof(int32_t)));
  HIPCHK(c.sc.alloc(&a.dn, (size_t)kchunks * (size_t)w * sizeof(int32_t)));
  HIPCHK(c.sc.alloc(&a.g, (size_t)o.out_height * (size_t)w * sizeof(uint16_t)));
  HIPCHK(c.sc.alloc(&d_targets, (size_t)channels * nmask * sizeof(uint32_t)));
  HIPCHK(c.sc.alloc(&d_reached, (size_t)channels * nrows * sizeof(uint32_t)));
  HIPCHK(c.sc.alloc(&d_sums, 2 * sizeof(unsigned long long)));
  if (pl.lds_bytes > 65536u) {
    hipError_t e = hipSuccess;
    with_bits(es, [&](auto u) {
      e = hipFuncSetAttribute((const void*)k_prox_rows<decltype(u)>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
    });
    HIPCHK(e);
  }

  std::vector<hipEvent_t> ev((size_t)channels * 3);
  for (hipEvent_t& e : ev) HIPCHK(c.sc.event(&e, hipEventDefault));
  const dim3 blk(256), grid_mask((unsigned)pl.col_blocks, (unsigned)pl.nchunks), grid_cols((unsigned)pl.col_blocks, (unsigned)kchunks);
  for (int32_t b = 0; b < channels; b++) {
    a.src = (const unsigned char*)src + (size_t)((int64_t)b * ss.band) * es;
    a.dist = dist.dev ? (unsigned char*)dist.dev + (size_t)((int64_t)b * o.dist.band_stride) * (size_t)elem_size(o.dist.dtype) : nullptr;
    a.alloc = alloc.dev ? (unsigned char*)alloc.dev + (size_t)((int64_t)b * o.alloc.band_stride) * es : nullptr;
    a.targets = d_targets + (size_t)b * nmask, a.reached = d_reached + (size_t)b * nrows;
    HIPCHK(hipEventRecord(ev[(size_t)b * 3], c.s));
    with_dtype(sdtype, [&](auto t) { hipLaunchKernelGGL((k_prox_mask<decltype(t)>), grid_mask, blk, 0, c.s, a); });
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_prox_carry, dim3((unsigned)pl.col_blocks), blk, 0, c.s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_prox_cols, grid_cols, blk, 0, c.s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[(size_t)b * 3 + 1], c.s));
    with_bits(es, [&](auto u) { hipLaunchKernelGGL((k_prox_rows<decltype(u)>), dim3(nrows), blk, pl.lds_bytes, c.s, a); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[(size_t)b * 3 + 2], c.s));
  }
  hipLaunchKernelGGL(k_prox_fold, dim3(2), blk, 0, c.s, d_targets, (uint32_t)channels * nmask, d_reached, (uint32_t)channels * nrows, d_sums);
  HIPCHK(hipGetLastError());
  unsigned long long sums[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, c.s));
  if (const int rc = copy_back(c, dist)) return rc;
  if (const int rc = copy_back(c, alloc)) return rc;
  HIPCHK(hipStreamSynchronize(c.s));
  g_prox_ms[0] = g_prox_ms[1] = 0.f;
  for (int32_t b = 0; b < channels; b++)
    for (int ph = 0; ph < 2; ph++) {
      float t = 0.f;
      (void)hipEventElapsedTime(&t, ev[(size_t)b * 3 + ph], ev[(size_t)b * 3 + ph + 1]);
      g_prox_ms[ph] += t;
    }
  if (counts) {
    counts[0] = (uint64_t)sums[0], counts[1] = (uint64_t)sums[1];
    counts[2] = (uint64_t)channels * (uint64_t)o.out_height * (uint64_t)o.out_width - counts[1];
  }
  return FRA_OK;
}

// the outputs of a call staged (a host output whole, so that the elements between the outputs keep their values)
int stage_outputs(Call& c, const fra_proximity_opts& o, int sdtype, int32_t channels, StagedOut* dist, StagedOut* alloc) {
  *dist = StagedOut{}, *alloc = StagedOut{};
  if (o.dist.dst) {
    const Strides s{o.dist.band_stride, o.dist.row_stride, o.dist.col_stride};
    if (const int rc = stage_out(c, o.dist.dst, o.dist.dst_on_device,
                                 (size_t)extent_of(channels, o.out_height, o.out_width, s) * (size_t)elem_size(o.dist.dtype), dist))
      return rc;
  }
  if (o.alloc.dst) {
    const Strides s{o.alloc.band_stride, o.alloc.row_stride, o.alloc.col_stride};
    if (const int rc = stage_out(c, o.alloc.dst, o.alloc.dst_on_device,
                                 (size_t)extent_of(channels, o.out_height, o.out_width, s) * (size_t)elem_size(sdtype), alloc))
      return rc;
  }
  return FRA_OK;
}

}  // namespace

extern "C" {

FRA_API int fra_proximity_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  ms[0] = g_prox_ms[0], ms[1] = g_prox_ms[1];
  return FRA_OK;
}

FRA_API int fra_proximity(fra_ctx* ctx, const fra_proximity_job* job, uint64_t* counts) {
  if (!ctx || !job || !job->src) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  const Strides ss{job->band_stride, job->row_stride, job->col_stride};
  const int32_t h = job->height, w = job->width;
  if (const int rc = check_job(job->dtype, job->channels, h, w, ss, &job->opts)) return rc;
  Call c(ctx);
  const void* src = nullptr;
  if (const int rc = stage_in(c, job->src, job->src_on_device,
                              (size_t)extent_of(job->channels, h, w, ss) * (size_t)elem_size(job->dtype), &src))
    return rc;
  StagedOut dist, alloc;
  if (const int rc = stage_outputs(c, job->opts, job->dtype, job->channels, &dist, &alloc)) return rc;
  return run_proximity(c, job->opts, job->dtype, job->channels, h, w, src, ss, dist, alloc, counts);
}

FRA_API int fra_decode_device_proximity(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, const fra_proximity_opts* opts,
                                        fra_decoded* infos, uint64_t* counts) {
  if (!ctx || !job || !roi || !opts || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (left_to_window_read_no_dst(job, roi)) return refer_to_window_read(ctx, job, roi, infos, true);
  const int32_t h = roi->height, w = roi->width;
  if (const int rc = check_job(job->dst_dtype, job->channels, h, w, Strides{0, 0, 1}, opts)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region_src(ctx, job, roi, infos, [&](Call& c, const void* d_region, const Strides& ss) -> int {
    StagedOut dist, alloc;
    if (const int rc = stage_outputs(c, *opts, job->dst_dtype, job->channels, &dist, &alloc)) return rc;
    return run_proximity(c, *opts, job->dst_dtype, job->channels, h, w, d_region, ss, dist, alloc, counts);
  });
}

}  // extern "C"
