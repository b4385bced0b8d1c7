// fra_focal.hip -- focal operations: a kh x kw window around every pixel of every band of a raster (fra_focal), and of
// a region of a set of tile streams without the decoded region leaving the GPU (fra_decode_device_focal).  The second
// unit over fra_region.h that maps a raster, and the first whose pixels share their inputs.
//
// The rule (include/flac_raster_amd.h): every value an f64, every step one IEEE f64 operation, the taps in row-major
// order; flac_raster/focal.py: focal_arrays is the reference the kernel is checked against bit for bit.
//
// k_focal<S>: a workgroup owns a tile of kTH x kTW = 16 x 64 output pixels of one band; thread (ty, tx) = (tid / 16,
// tid % 16) owns the 4 neighbouring pixels 4 tx ... 4 tx + 3 of row ty, so that it stores them as one vector.
//   The halo tile.  The (kTH + kh - 1) x (kTW + kw - 1) source elements under the tile, the columns widened to whole
//   16-byte vectors of the source, are read from global memory once per workgroup -- a 16-byte load where the vector
//   lies inside the row and aligned16 holds, element by element otherwise (the raster's borders, any other layout) --
//   and kept in LDS in the source's own type, one validity byte per element beside them (inside the source or clamped
//   to it, not NaN, not nodata): the 30 x 80 f64 elements of a 15 x 15 window take 18.8 + 5.6 KiB, six workgroups (24
//   waves) of a CU's 160 KiB; a 3 x 3 window over uint16 takes 6.8 KiB, and the 8 workgroups a CU's 32 waves allow
//   fit.  The edge mode is applied here: a clamped tap is loaded from the pixel it stands for.  The loop over the
//   tile's vectors has one trip count per workgroup; lanes past the end load nothing.  (Tiles of 32 and 64 rows, and
//   one LDS read per row element shared by the thread's four pixels, were measured and were no faster: DESIGN 6c.)
//   LDS layout.  Column c of a tile row lives at (c % 4) * qp + c / 4: four phase sub-rows.  For a tap (dy, dx) and
//   its pixel p a thread reads column 4 tx + (off + p + dx), whose phase is the same for every lane and whose index is
//   tx + const: the 16 lanes of a tile row read 16 consecutive elements.  The row pitch is 64 mod 128 bytes (128 mod 256
//   for 8-byte elements, whose bank is taken mod 64), so the two tile rows of a 32-lane group fall on disjoint banks:
//   reads along a row are free of bank conflicts for every element size; the validity bytes likewise.
//   All valid.  The barrier after the load is a __syncthreads_or of "I have written an invalid element": a workgroup
//   whose halo tile is all valid (the interior of an integer raster without nodata) never reads the validity bytes.
//   The op is dispatched once per workgroup on scalar values (the spec travels by value in the kernel's arguments, the
//   weights are scalar loads); the destination dtype is dispatched at the store alone, so there is one instance per
//   source type.  A thread whose pixels lie past the rectangle computes and stores nothing; a ragged slot stores
//   element by element.  left_out: one wave reduction and one 64-bit vector atomic add per wave, into the band's
//   counter.
//   MEDIAN counts, for every valid tap, the valid taps that order before it (by value, equal values by tap order): at
//   most 25 x 25 LDS reads per pixel and no per-lane array, which would live in private memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"
#include "fra_scan.h"

static_assert(sizeof(fra_focal_spec) == 1904, "fra_focal_spec is 1904 bytes");

namespace {

using namespace fra_region;

constexpr int kTH = 16, kTW = 64;  // the tile: 256 threads x 4 pixels
constexpr int kP = 4;              // pixels of a thread, neighbours in a row

struct FocalArgs {
  const void* src;
  void* dst;
  int64_t sbs, srs, scs;  // source element strides: band, row, column
  int64_t dbs, drs, dcs;  // destination element strides
  unsigned long long* left;  // per band: the pixels that got fill, zeroed by the host
  double nodata, fill;
  int32_t h, w;            // the source
  int32_t r0, c0, oh, ow;  // the output rectangle
  int32_t op, kh, kw, clamp, flags;
  int32_t use_nd;          // FRA_FOCAL_NODATA with a nodata that is not NaN
  int32_t svec, dvec;      // vector accesses are aligned (fra_region.h: aligned16)
  int32_t ddtype;
  uint32_t tiles_x, ntiles;  // tiles across the rectangle, and in all
  uint32_t qp, pitch, vpitch, val_off;  // a phase sub-row and a tile row in elements; a validity row and the validity's start in bytes
  double params[8];
  double weights[FRA_FOCAL_MAX_SIZE * FRA_FOCAL_MAX_SIZE];
};

__device__ inline double neg_zero() { return __longlong_as_double((long long)0x8000000000000000ull); }
__device__ inline double pos_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// where a thread finds its taps: tile row ty + dy starts at row0 + dy * pitch (values) and vrow0 + dy * vpitch (validity),
// its column 4 tx + q at (q & 3) * qp + (q >> 2) from there
template <typename S>
struct Taps {
  const S* tile;
  const uint8_t* val;
  uint32_t row0, vrow0, pitch, vpitch, qp;
  __device__ inline uint32_t col(uint32_t q) const { return (q & 3u) * qp + (q >> 2); }
  __device__ inline double x(uint32_t dy, uint32_t q) const { return (double)tile[row0 + dy * pitch + col(q)]; }
  __device__ inline bool ok(uint32_t dy, uint32_t q) const { return val[vrow0 + dy * vpitch + col(q)] != 0; }
};

// SUM, MEAN, MIN, MAX, COUNT and CONVOLVE of the thread's kP pixels: one walk over the taps in row-major order.  AV: every
// element of the halo tile is valid.  A sum starts at -0.0, which is x for every first x (-0.0 + x == x bit for bit,
// x = +-0.0 included), a minimum at +inf and a maximum at -inf likewise.  Bit p of the result: pixel p gets fill.
template <typename S, int OP, bool AV>
__device__ inline uint32_t reduce_taps(const FocalArgs& g, const Taps<S>& t, uint32_t off, double* out) {
  double acc[kP], ws[kP];
  uint32_t n[kP];
#pragma unroll
  for (int p = 0; p < kP; p++) {
    acc[p] = OP == FRA_FOCAL_MIN ? pos_inf() : (OP == FRA_FOCAL_MAX ? -pos_inf() : neg_zero());
    ws[p] = neg_zero();
    n[p] = 0;
  }
  for (uint32_t dy = 0; dy < (uint32_t)g.kh; dy++) {
    for (uint32_t dx = 0; dx < (uint32_t)g.kw; dx++) {
      const double wt = OP == FRA_FOCAL_CONVOLVE ? g.weights[dy * (uint32_t)g.kw + dx] : 0.0;
#pragma unroll
      for (int p = 0; p < kP; p++) {
        const uint32_t q = off + (uint32_t)p + dx;
        const bool v = AV ? true : t.ok(dy, q);
        const double x = t.x(dy, q);
        if constexpr (OP == FRA_FOCAL_SUM || OP == FRA_FOCAL_MEAN) {
          acc[p] = v ? acc[p] + x : acc[p];
        } else if constexpr (OP == FRA_FOCAL_MIN) {
          acc[p] = (v && x < acc[p]) ? x : acc[p];
        } else if constexpr (OP == FRA_FOCAL_MAX) {
          acc[p] = (v && x > acc[p]) ? x : acc[p];
        } else if constexpr (OP == FRA_FOCAL_CONVOLVE) {
          const double prod = x * wt;
          acc[p] = v ? acc[p] + prod : acc[p];
          ws[p] = v ? ws[p] + wt : ws[p];
        }
        n[p] += v ? 1u : 0u;
      }
    }
  }
  uint32_t fill = 0;
#pragma unroll
  for (int p = 0; p < kP; p++) {
    double r = acc[p];
    bool f = n[p] == 0;
    if constexpr (OP == FRA_FOCAL_MEAN) r = acc[p] / (double)n[p];
    if constexpr (OP == FRA_FOCAL_COUNT) r = (double)n[p], f = false;
    if constexpr (OP == FRA_FOCAL_CONVOLVE) {
      if (g.flags & FRA_FOCAL_NORMALIZE) r = acc[p] / ws[p], f = f || ws[p] == 0.0;
    }
    out[p] = r;
    fill |= (uint32_t)f << p;
  }
  return fill;
}

// MEDIAN: the valid tap with exactly (n - 1) / 2 valid taps ordered before it
template <typename S>
__device__ inline uint32_t median_taps(const FocalArgs& g, const Taps<S>& t, uint32_t off, double* out) {
  uint32_t fill = 0;
  const uint32_t kh = (uint32_t)g.kh, kw = (uint32_t)g.kw;
#pragma unroll
  for (int p = 0; p < kP; p++) {
    uint32_t n = 0;
    for (uint32_t dy = 0; dy < kh; dy++)
      for (uint32_t dx = 0; dx < kw; dx++) n += t.ok(dy, off + (uint32_t)p + dx) ? 1u : 0u;
    const uint32_t rank = n ? (n - 1u) / 2u : 0u;
    double r = 0.0;
    for (uint32_t iy = 0; iy < kh; iy++) {
      for (uint32_t ix = 0; ix < kw; ix++) {
        const uint32_t qi = off + (uint32_t)p + ix;
        const double xi = t.x(iy, qi);
        const bool vi = t.ok(iy, qi);
        uint32_t before = 0;
        for (uint32_t jy = 0; jy < kh; jy++) {
          for (uint32_t jx = 0; jx < kw; jx++) {
            const uint32_t qj = off + (uint32_t)p + jx;
            const double xj = t.x(jy, qj);
            const bool earlier = jy * kw + jx < iy * kw + ix;
            before += (t.ok(jy, qj) && (xj < xi || (xj == xi && earlier))) ? 1u : 0u;
          }
        }
        r = (vi && before == rank) ? xi : r;
      }
    }
    out[p] = r;
    fill |= (uint32_t)(n == 0) << p;
  }
  return fill;
}

// SLOPE and HILLSHADE: Horn's gradient over the nine taps, every one of which must be valid
template <typename S, int OP, bool AV>
__device__ inline uint32_t terrain_taps(const FocalArgs& g, const Taps<S>& t, uint32_t off, double* out) {
  uint32_t fill = 0;
#pragma unroll
  for (int p = 0; p < kP; p++) {
    double z[9];
    bool all = true;
#pragma unroll
    for (uint32_t k = 0; k < 9; k++) {
      const uint32_t q = off + (uint32_t)p + k % 3u;
      z[k] = t.x(k / 3u, q);
      if (!AV) all = all && t.ok(k / 3u, q);
    }
    const double a = z[0], b = z[1], c = z[2], d = z[3], f = z[5], gg = z[6], hh = z[7], i = z[8];
    const double zx = ((c + (f + f)) + i) - ((a + (d + d)) + gg);
    const double zy = ((a + (b + b)) + c) - ((gg + (hh + hh)) + i);
    const double pp = zx * g.params[0], qq = zy * g.params[1];
    double r;
    if constexpr (OP == FRA_FOCAL_SLOPE) {
      r = sqrt(pp * pp + qq * qq) * g.params[2];
    } else {
      double s = ((g.params[4] - pp * g.params[2]) - qq * g.params[3]) / sqrt((1.0 + pp * pp) + qq * qq);
      s = s > 0.0 ? s : 0.0;
      r = s * g.params[5];
    }
    out[p] = r;
    fill |= (uint32_t)!all << p;
  }
  return fill;
}

template <typename S, bool AV>
__device__ inline uint32_t apply_op(const FocalArgs& g, const Taps<S>& t, uint32_t off, double* out) {
  switch (g.op) {
    case FRA_FOCAL_SUM: return reduce_taps<S, FRA_FOCAL_SUM, AV>(g, t, off, out);
    case FRA_FOCAL_MEAN: return reduce_taps<S, FRA_FOCAL_MEAN, AV>(g, t, off, out);
    case FRA_FOCAL_MIN: return reduce_taps<S, FRA_FOCAL_MIN, AV>(g, t, off, out);
    case FRA_FOCAL_MAX: return reduce_taps<S, FRA_FOCAL_MAX, AV>(g, t, off, out);
    case FRA_FOCAL_COUNT: return reduce_taps<S, FRA_FOCAL_COUNT, AV>(g, t, off, out);
    case FRA_FOCAL_CONVOLVE: return reduce_taps<S, FRA_FOCAL_CONVOLVE, AV>(g, t, off, out);
    case FRA_FOCAL_SLOPE: return terrain_taps<S, FRA_FOCAL_SLOPE, AV>(g, t, off, out);
    case FRA_FOCAL_HILLSHADE: return terrain_taps<S, FRA_FOCAL_HILLSHADE, AV>(g, t, off, out);
    default: return median_taps<S>(g, t, off, out);  // (the host has checked the op)
  }
}

// the thread's n <= kP pixels, converted, to p[0], p[cs], ...
template <typename D>
__device__ inline void store_px(D* p, int64_t cs, bool vec, int n, const double* x) {
  if (vec && n == kP) {
    VecOf<D, kP> v;
#pragma unroll
    for (int i = 0; i < kP; i++) v.v[i] = to_out<D>(x[i]);
    *(VecOf<D, kP>*)p = v;
  } else {
#pragma unroll
    for (int i = 0; i < kP; i++)
      if (i < n) p[(int64_t)i * cs] = to_out<D>(x[i]);
  }
}

template <typename S>
__global__ void __launch_bounds__(256) k_focal(FocalArgs g) {
  constexpr int V = 16 / (int)sizeof(S);  // elements of a 16-byte vector
  extern __shared__ __align__(16) unsigned char s_focal[];
  S* const tile = (S*)s_focal;
  uint8_t* const val = s_focal + g.val_off;
  const uint32_t tid = threadIdx.x;
  const uint32_t band = blockIdx.y;
  const uint32_t tile_id = blockIdx.z * gridDim.x + blockIdx.x;
  if (tile_id >= g.ntiles) return;  // (the whole workgroup: the last slice of the grid)
  const int32_t orow0 = (int32_t)(tile_id / g.tiles_x) * kTH;  // the tile's origin in the rectangle
  const int32_t ocol0 = (int32_t)(tile_id % g.tiles_x) * kTW;
  const int32_t trows = min(kTH, g.oh - orow0), tcols = min(kTW, g.ow - ocol0);
  const int32_t srow0 = g.r0 + orow0 - g.kh / 2;  // the source pixel under the first tap of the tile's first pixel
  const int32_t scol0 = g.c0 + ocol0 - g.kw / 2;
  const int32_t lcol0 = (scol0 >= 0 ? scol0 / V : -((-scol0 + V - 1) / V)) * V;  // ... rounded down to a whole vector
  const uint32_t off = (uint32_t)(scol0 - lcol0);
  const uint32_t nrows = (uint32_t)(trows + g.kh - 1);
  const uint32_t cpr = (off + (uint32_t)(tcols + g.kw - 1) + V - 1) / V;  // vectors per tile row
  const uint32_t nvec = nrows * cpr;
  const uint32_t niter = (nvec + 255u) / 256u;
  const S* __restrict__ const ps = (const S*)g.src + (int64_t)band * g.sbs;

  int bad = 0;  // this thread has written an invalid element
  for (uint32_t it = 0; it < niter; it++) {
    const uint32_t ch = it * 256u + tid;
    if (ch < nvec) {
      const uint32_t lr = ch / cpr, cc = ch - lr * cpr;
      int32_t sr = srow0 + (int32_t)lr;
      const int32_t col0 = lcol0 + (int32_t)cc * V;
      bool row_ok = sr >= 0 && sr < g.h;
      if (g.clamp) sr = min(max(sr, 0), g.h - 1), row_ok = true;
      const S* const prow = ps + (int64_t)(row_ok ? sr : 0) * g.srs;
      S x[V];
      uint32_t okm = 0;  // bit j: element j is a source pixel (its own or the one it is clamped to)
      if (row_ok && g.svec && col0 >= 0 && col0 + V <= g.w) {
        const VecOf<S, V> v = *(const VecOf<S, V>*)(prow + col0);
#pragma unroll
        for (int j = 0; j < V; j++) x[j] = v.v[j];
        okm = (1u << V) - 1u;
      } else {
#pragma unroll
        for (int j = 0; j < V; j++) {
          int32_t c = col0 + j;
          bool ok = row_ok && c >= 0 && c < g.w;
          if (g.clamp) c = min(max(c, 0), g.w - 1), ok = row_ok;
          x[j] = ok ? prow[(int64_t)c * g.scs] : (S)0;
          okm |= (uint32_t)ok << j;
        }
      }
#pragma unroll
      for (int j = 0; j < V; j++) {
        const double xd = (double)x[j];
        const bool valid = (okm >> j & 1u) && !(xd != xd) && !(g.use_nd && xd == g.nodata);
        const uint32_t lc = cc * V + (uint32_t)j;
        const uint32_t at = (lc & 3u) * g.qp + (lc >> 2);
        tile[lr * g.pitch + at] = x[j];
        val[lr * g.vpitch + at] = valid ? 1 : 0;
        bad |= !valid;
      }
    }
  }
  const bool all_valid = __syncthreads_or(bad) == 0;

  const uint32_t ty = tid / (kTW / kP), tx = tid % (kTW / kP);
  const int n = (int)ty < trows ? min(kP, max(0, tcols - (int)tx * kP)) : 0;  // the thread's pixels inside the rectangle
  uint32_t nleft = 0;
  if (n > 0) {
    const Taps<S> t{tile, val, ty * g.pitch + tx, ty * g.vpitch + tx, g.pitch, g.vpitch, g.qp};
    double out[kP];
    uint32_t fill = all_valid ? apply_op<S, true>(g, t, off, out) : apply_op<S, false>(g, t, off, out);
    if ((g.flags & FRA_FOCAL_KEEP_MASK) && !all_valid) {
#pragma unroll
      for (int p = 0; p < kP; p++) fill |= (uint32_t)!t.ok((uint32_t)g.kh / 2u, off + (uint32_t)p + (uint32_t)g.kw / 2u) << p;
    }
    fill &= (1u << n) - 1u;
    nleft = (uint32_t)__popc(fill);
#pragma unroll
    for (int p = 0; p < kP; p++) out[p] = (fill >> p & 1u) ? g.fill : out[p];
    const int64_t doff = (int64_t)band * g.dbs + (int64_t)(orow0 + (int32_t)ty) * g.drs + (int64_t)(ocol0 + (int32_t)tx * kP) * g.dcs;
    const bool dvec = g.dvec != 0;
    switch (g.ddtype) {
      case FRA_U8: store_px((uint8_t*)g.dst + doff, g.dcs, dvec, n, out); break;
      case FRA_I8: store_px((int8_t*)g.dst + doff, g.dcs, dvec, n, out); break;
      case FRA_U16: store_px((uint16_t*)g.dst + doff, g.dcs, dvec, n, out); break;
      case FRA_I16: store_px((int16_t*)g.dst + doff, g.dcs, dvec, n, out); break;
      case FRA_U32: store_px((uint32_t*)g.dst + doff, g.dcs, dvec, n, out); break;
      case FRA_I32: store_px((int32_t*)g.dst + doff, g.dcs, dvec, n, out); break;
      case FRA_F32: store_px((float*)g.dst + doff, g.dcs, dvec, n, out); break;
      default: store_px((double*)g.dst + doff, g.dcs, dvec, n, out); break;
    }
  }

  uint32_t s = nleft;
#pragma unroll
  for (int o = 32; o; o >>= 1) s += __shfl_down(s, o, 64);
  if ((tid & 63u) == 0 && s) atomicAdd(g.left + band, (unsigned long long)s);
}

thread_local float g_focal_ms = 0.f;

constexpr const char* kNot = "mapped in one call";  // (too_many_pixels)

// the smallest b >= bytes with b % mod == mod / 2
int64_t half_odd(int64_t bytes, int64_t mod) { return (bytes + mod / 2 - 1) / mod * mod + mod / 2; }

// k_focal over the rectangle `r` of a (channels, h, w) device raster into a device raster, timed; the fill counts to
// `left_out` (channels words)
int run_focal(Call& c, const fra_focal_spec& sp, int sdtype, int32_t channels, int32_t h, int32_t w, const fra_window& r,
              const Io& io, int ddtype, uint64_t* left_out) {
  FocalArgs g{};
  g.src = io.src, g.dst = io.out.dev;
  g.sbs = io.ss.band, g.srs = io.ss.row, g.scs = io.ss.col;
  g.dbs = io.ds.band, g.drs = io.ds.row, g.dcs = io.ds.col;
  g.nodata = sp.nodata, g.fill = sp.fill;
  g.h = h, g.w = w;
  g.r0 = r.row_off, g.c0 = r.col_off, g.oh = r.height, g.ow = r.width;
  g.op = sp.op, g.kh = sp.kh, g.kw = sp.kw, g.clamp = sp.edge == FRA_FOCAL_EDGE_CLAMP, g.flags = sp.flags;
  g.use_nd = (sp.flags & FRA_FOCAL_NODATA) && sp.nodata == sp.nodata;
  const int64_t es = elem_size(sdtype), V = 16 / es;
  g.svec = aligned16(io.src, io.ss, (size_t)es);
  g.dvec = aligned16(io.out.dev, io.ds, (size_t)elem_size(ddtype));
  g.ddtype = ddtype;
  std::memcpy(g.params, sp.params, sizeof(g.params));
  std::memcpy(g.weights, sp.weights, sizeof(g.weights));
  // the halo tile in LDS: columns widened to whole vectors (and to the four phases), rows on disjoint banks
  const int64_t unit = std::max<int64_t>(V, 4);
  const int64_t lw = (kTW + sp.kw - 1 + (V - 1) + unit - 1) / unit * unit;
  const int64_t rows = kTH + sp.kh - 1;
  const int64_t pitch = half_odd(lw * es, es == 8 ? 256 : 128) / es;
  const int64_t vpitch = half_odd(lw, 128);
  const int64_t val_off = (rows * pitch * es + 15) / 16 * 16;
  const size_t lds = (size_t)(val_off + rows * vpitch);
  g.qp = (uint32_t)(lw / 4), g.pitch = (uint32_t)pitch, g.vpitch = (uint32_t)vpitch, g.val_off = (uint32_t)val_off;
  const int64_t tiles_x = ((int64_t)r.width + kTW - 1) / kTW, tiles_y = ((int64_t)r.height + kTH - 1) / kTH;
  // at most 2^32 pixels per band: fewer than 2^29 tiles, in slices of 2^20 so that a grid dimension's threads stay in 32 bits
  const int64_t ntiles = tiles_x * tiles_y, slice = std::min<int64_t>(ntiles, (int64_t)1 << 20);
  g.tiles_x = (uint32_t)tiles_x, g.ntiles = (uint32_t)ntiles;
  HIPCHK(c.sc.alloc(&g.left, sizeof(unsigned long long) * (size_t)channels));
  HIPCHK(hipMemsetAsync(g.left, 0, sizeof(unsigned long long) * (size_t)channels, c.s));
  unsigned long long left[255] = {};
  const int rc = timed(
      c, &g_focal_ms,
      [&]() -> int {
        with_dtype(sdtype, [&](auto s) {
          hipLaunchKernelGGL((k_focal<decltype(s)>), dim3((unsigned)slice, (unsigned)channels, (unsigned)((ntiles + slice - 1) / slice)),
                             dim3(256), lds, c.s, g);
        });
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&]() -> int {
        HIPCHK(hipMemcpyAsync(left, g.left, sizeof(unsigned long long) * (size_t)channels, hipMemcpyDeviceToHost, c.s));
        return copy_back(c, io.out);
      });
  if (rc) return rc;
  if (left_out)
    for (int k = 0; k < channels; k++) left_out[k] = (uint64_t)left[k];
  return FRA_OK;
}

int check_spec(const fra_focal_spec* s) {
  if (!s) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (s->op < FRA_FOCAL_SUM || s->op > FRA_FOCAL_HILLSHADE) return fra_internal_set_error(FRA_E_INVALID, "op: unknown focal op %d", s->op);
  if (s->edge != FRA_FOCAL_EDGE_SKIP && s->edge != FRA_FOCAL_EDGE_CLAMP)
    return fra_internal_set_error(FRA_E_INVALID, "edge: unknown edge mode %d", s->edge);
  if (s->flags & ~(FRA_FOCAL_NODATA | FRA_FOCAL_NORMALIZE | FRA_FOCAL_KEEP_MASK))
    return fra_internal_set_error(FRA_E_INVALID, "flags: unknown focal flags 0x%x", (unsigned)s->flags);
  if (s->kh < 1 || s->kh > FRA_FOCAL_MAX_SIZE || !(s->kh & 1))
    return fra_internal_set_error(FRA_E_INVALID, "kh: window height %d is not odd and in 1 ... %d", s->kh, FRA_FOCAL_MAX_SIZE);
  if (s->kw < 1 || s->kw > FRA_FOCAL_MAX_SIZE || !(s->kw & 1))
    return fra_internal_set_error(FRA_E_INVALID, "kw: window width %d is not odd and in 1 ... %d", s->kw, FRA_FOCAL_MAX_SIZE);
  if (s->op == FRA_FOCAL_MEDIAN && s->kh * s->kw > FRA_FOCAL_MAX_MEDIAN)
    return fra_internal_set_error(FRA_E_INVALID, "kh, kw: a median of %d x %d taps, more than %d", s->kh, s->kw, FRA_FOCAL_MAX_MEDIAN);
  if ((s->op == FRA_FOCAL_SLOPE || s->op == FRA_FOCAL_HILLSHADE) && (s->kh != 3 || s->kw != 3))
    return fra_internal_set_error(FRA_E_INVALID, "kh, kw: slope and hillshade take a 3 x 3 window, not %d x %d", s->kh, s->kw);
  if ((s->flags & FRA_FOCAL_NORMALIZE) && s->op != FRA_FOCAL_CONVOLVE)
    return fra_internal_set_error(FRA_E_INVALID, "flags: FRA_FOCAL_NORMALIZE goes with FRA_FOCAL_CONVOLVE alone (op %d)", s->op);
  return FRA_OK;
}

// the layout of a (channels, h, w) source and of the destination (whose size is the rectangle's, checked after it)
int check_layouts(int sdtype, int32_t channels, int32_t h, int32_t w, const Strides& ss, const fra_calc_dst* o) {
  if (const int rc = check_raster(sdtype, channels, h, w, ss, ss)) return rc;
  const Strides ds{o->band_stride, o->row_stride, o->col_stride};
  if (const int rc = check_raster(o->dtype, channels, h, w, ds, ds)) return rc;
  if (channels > 255) return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d bands, more than 255)", channels);
  return FRA_OK;
}

// FRA_E_INVALID unless r is a rectangle of at least one pixel inside h x w
int check_rect(const fra_window& r, int32_t h, int32_t w, const char* what, const char* in) {
  if (r.height < 1 || r.width < 1 || r.row_off < 0 || r.col_off < 0 || (int64_t)r.row_off + r.height > h ||
      (int64_t)r.col_off + r.width > w)
    return fra_internal_set_error(FRA_E_INVALID, "%s (%d, %d, %d x %d) is empty or not inside %s (%d x %d)", what, r.row_off,
                                  r.col_off, r.height, r.width, in, h, w);
  return FRA_OK;
}

}  // namespace

extern "C" {

FRA_API int fra_focal_check(const fra_focal_spec* spec) { return check_spec(spec); }

FRA_API int fra_focal_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_focal_ms;
  return FRA_OK;
}

FRA_API int fra_focal(fra_ctx* ctx, const fra_focal_job* job, uint64_t* left_out) {
  if (!ctx || !job || !job->src || !job->out.dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (const int rc = check_spec(&job->spec)) return rc;
  const Strides ss{job->band_stride, job->row_stride, job->col_stride};
  const int32_t h = job->height, w = job->width;
  const fra_calc_dst& o = job->out;
  if (const int rc = check_layouts(job->dtype, job->channels, h, w, ss, &o)) return rc;
  if (const int rc = check_rect(job->rect, h, w, "the output rectangle", "the source")) return rc;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  return run_raster_to(ctx, job->src, job->src_on_device, job->dtype, job->channels, h, w, ss,
                       Dst{o.dst, o.dst_on_device, o.dtype, job->channels, job->rect.height, job->rect.width,
                           {o.band_stride, o.row_stride, o.col_stride}},
                       [&](Call& c, Io& io) {
                         return run_focal(c, job->spec, job->dtype, job->channels, h, w, job->rect, io, o.dtype, left_out);
                       });
}

FRA_API int fra_decode_device_focal(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, const fra_focal_spec* spec,
                                    const fra_window* inner, const fra_calc_dst* out, uint64_t* left_out, fra_decoded* infos) {
  if (!ctx || !job || !roi || !spec || !inner || !out || !out->dst || !infos)
    return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (left_to_window_read_no_dst(job, roi)) return refer_to_window_read(ctx, job, roi, infos, true);
  if (const int rc = check_spec(spec)) return rc;
  const int32_t h = roi->height, w = roi->width;
  if (const int rc = check_layouts(job->dst_dtype, job->channels, h, w, Strides{0, 0, 1}, out)) return rc;
  if (const int rc = check_rect(*inner, h, w, "the inner rectangle", "the region")) return rc;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region_to(ctx, job, roi, infos,
                       Dst{out->dst, out->dst_on_device, out->dtype, job->channels, inner->height, inner->width,
                           {out->band_stride, out->row_stride, out->col_stride}},
                       [&](Call& c, Io& io) {
                         return run_focal(c, *spec, job->dst_dtype, job->channels, h, w, *inner, io, out->dtype, left_out);
                       });
}

}  // extern "C"
