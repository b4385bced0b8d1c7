// fra_calc.hip -- band math: a per-pixel expression program over the bands of a raster (fra_calc), and over a region of
// a set of tile streams without the decoded region leaving the GPU (fra_decode_device_calc).  The one unit over
// fra_region.h that maps a raster; its output has a dtype and a band count of its own.
//
// The rule (include/flac_raster_amd.h): a stack program in reverse Polish notation, every value an f64, every op one
// IEEE f64 operation; flac_raster/calc.py: calc_arrays is the reference the kernel is checked against bit for bit.
//
// k_calc<S, D>: an interpreter.  The program travels by value in the kernel's arguments, so the fetch of a word, the
// dispatch on its op and the stack pointer are scalar loads, scalar branches and a scalar register: the program is the
// same for every lane.  A lane evaluates P = 8 or 4 neighbouring pixels of a row (a slot) per word, which spreads a
// word's dispatch, and the latency of a BAND word's load, over the wave's 512 or 256 pixels (P = 8: 21 - 38 % less time
// than P = 4 on the measured expressions; the host picks it while the LDS below stays within 32 KiB).
// Grid, slots and cursor of fra_scan.h, with no band in the grid: a workgroup is a chunk of rows, thread t owns slots
// t, t + 256, ... of it, and the loop over a chunk's slots has one trip count for the whole workgroup (lanes past the
// end evaluate nothing they load or store), so no branch of the interpreter diverges.
//   The stack.  A per-lane array indexed by the stack pointer would live in private memory.  Instead the top of the
//   stack is P registers and the values below it are in LDS, lane-major: value s of pixel p of thread t at
//   ((s * P + p) * 256 + t) * 8 bytes, so a wave reads and writes 512 contiguous bytes (no bank conflict), and nobody
//   but thread t ever touches its column (no barrier).  The host has simulated the stack (fra_calc.h) and asks for
//   (deepest - 1) * P * 2 KiB of dynamic LDS: NDVI takes 32 KiB at P = 8, the deepest program 56 KiB at P = 4.
//   Loads and stores.  A slot of a row is read as one vector of P elements (4 to 64 bytes: up to four 16-byte
//   accesses) when the source's column stride is 1 and its base and strides are multiples of 16 bytes, element by
//   element otherwise (a ragged last slot always); stores likewise, judged on the destination.  A BAND word loads where it stands: what hides the
//   latency is the occupancy (up to 32 waves per CU), not a prefetch.
//   Nodata.  A first walk over the program's BAND words marks the left-out pixels of the slot (P bits); their second
//   load, by the word itself, comes from the cache.  The count goes through one wave reduction and one 64-bit vector
//   atomic add per wave, at the kernel's end, into one device counter: a pixel is left out for all outputs at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_calc.h"
#include "fra_host.h"
#include "fra_region.h"
#include "fra_scan.h"

static_assert(sizeof(fra_calc_program) == 544, "fra_calc_program is 544 bytes");

namespace {

using namespace fra_region;

// P, the pixels of a lane per word, is 8 while the stack below the top then fits kWideLds bytes of LDS (depth <= 3: the
// copy, NDVI, a stretch), and 4 for deeper programs (at most 56 KiB).  (-1: always 4, the A/B build of DESIGN 6c)
#ifndef FRA_CALC_WIDE_LDS
#define FRA_CALC_WIDE_LDS 32768
#endif
constexpr int64_t kWideLds = FRA_CALC_WIDE_LDS;

struct CalcArgs {
  const void* src;
  void* dst;
  int64_t sbs, srs, scs;  // source element strides: band, row, column
  int64_t dbs, drs, dcs;  // destination element strides
  unsigned long long* left;  // the left-out pixels, zeroed by the host
  double nodata, fill;
  int32_t h, w;
  ChunkPlan plan;      // for slots of P pixels, P the instance's; one band
  int32_t svec, dvec;  // vector accesses are aligned (column stride 1; base, row and band strides multiples of 16 bytes)
  int32_t use_nd;      // FRA_CALC_NODATA with a nodata that is not NaN ... (1) or that is (2: NaN pixels alone are left out)
  int32_t ncode;
  uint16_t code[FRA_CALC_MAX_CODE];
  double consts[FRA_CALC_MAX_CONST];
};

// elements [0, n) of a slot as f64 (the others 0.0)
template <typename S, int P>
__device__ inline void load_f64(const S* p, int64_t cs, bool vec, int n, double* x) {
  auto widen = [&](const VecOf<S, P>& v) {
#pragma unroll
    for (int i = 0; i < P; i++) x[i] = (double)v.v[i];
  };
  // (each path converts what it loaded: one conversion after the paths have met costs the interpreter more branches)
  if (vec && n == P) widen(load_slot<S, P>(p, cs, true, P));
  else widen(load_slot<S, P>(p, cs, false, n));
}

template <typename D, int P>
__device__ inline void store_slot(D* p, int64_t cs, bool vec, int n, const double* x) {
  if (vec && n == P) {
    VecOf<D, P> v;
#pragma unroll
    for (int i = 0; i < P; i++) v.v[i] = to_out<D>(x[i]);
    *(VecOf<D, P>*)p = v;
  } else {
#pragma unroll
    for (int i = 0; i < P; i++)
      if (i < n) p[(int64_t)i * cs] = to_out<D>(x[i]);
  }
}

template <typename S, typename D, int P>
__global__ void __launch_bounds__(256) k_calc(CalcArgs g) {
  static_assert(P == 4 || P == 8, "a slot's left-out bits and vector accesses are written for 4 or 8 pixels");
  extern __shared__ double s_stack[];  // (deepest - 1) x P x 256 values: what lies below the top of the stack
  const uint32_t tid = threadIdx.x;
  const Chunk c = chunk_at(g.plan, g.h, blockIdx.x);
  const uint32_t rows = c.rows;
  const uint32_t nslots = rows * g.plan.nvec;  // (the host keeps a chunk's slots inside 31 bits)
  const uint32_t niter = (nslots + 255u) / 256u;
  const S* __restrict__ const ps = (const S*)g.src + c.row0 * g.srs;
  D* __restrict__ const pd = (D*)g.dst + c.row0 * g.drs;
  const bool svec = g.svec != 0, dvec = g.dvec != 0;
  Cursor at(g.plan, tid);
  uint32_t nleft = 0;  // (a thread's slots x P stay far below 2^32)

  for (uint32_t it = 0; it < niter; it++) {
    const bool active = at.row < rows;
    const int n = active ? slot_count<P>(g.w, at.cv) : 0;
    const int64_t soff = (int64_t)at.row * g.srs + (int64_t)at.cv * P * g.scs;
    const int64_t doff = (int64_t)at.row * g.drs + (int64_t)at.cv * P * g.dcs;
    uint32_t mask = 0;  // bit i: pixel i of the slot is left out
    if (g.use_nd) {
      for (int pc = 0; pc < g.ncode; pc++) {
        const uint32_t word = g.code[pc];
        if ((word & 0xffu) != FRA_CALC_BAND) continue;
        double x[P];
        load_f64<S, P>(ps + ((int64_t)(word >> 8) * g.sbs + soff), g.scs, svec, n, x);
#pragma unroll
        for (int i = 0; i < P; i++) mask |= (uint32_t)(x[i] != x[i] || (g.use_nd == 1 && x[i] == g.nodata)) << i;
      }
      mask &= (1u << n) - 1u;
      nleft += (uint32_t)__popc(mask);
    }

    double tos[P];  // the top of the stack; the sp - 1 values below it are in LDS
#pragma unroll
    for (int i = 0; i < P; i++) tos[i] = 0.0;
    uint32_t sp = 0;
    // value s (from the bottom) of pixel i
    auto slot = [&](uint32_t s, int i) -> double& { return s_stack[(s * P + i) * 256u + tid]; };
    auto push = [&]() {  // makes room on top
      if (sp > 0) {
#pragma unroll
        for (int i = 0; i < P; i++) slot(sp - 1, i) = tos[i];
      }
      sp++;
    };
    for (int pc = 0; pc < g.ncode; pc++) {
      const uint32_t word = g.code[pc];
      const uint32_t op = word & 0xffu, arg = word >> 8;
      if (op == FRA_CALC_CONST) {
        push();
        const double c = g.consts[arg];
#pragma unroll
        for (int i = 0; i < P; i++) tos[i] = c;
      } else if (op == FRA_CALC_BAND) {
        push();
        load_f64<S, P>(ps + ((int64_t)arg * g.sbs + soff), g.scs, svec, n, tos);
      } else if (op == FRA_CALC_STORE) {
        double x[P];
#pragma unroll
        for (int i = 0; i < P; i++) x[i] = (mask >> i & 1u) ? g.fill : tos[i];
        store_slot<D, P>(pd + ((int64_t)arg * g.dbs + doff), g.dcs, dvec, n, x);
        sp--;
        if (sp > 0) {
#pragma unroll
          for (int i = 0; i < P; i++) tos[i] = slot(sp - 1, i);
        }
      } else if (op == FRA_CALC_NEG || op == FRA_CALC_ABS || op == FRA_CALC_SQRT || op == FRA_CALC_FLOOR ||
                 op == FRA_CALC_NOT) {
#pragma unroll
        for (int i = 0; i < P; i++) {
          const double x = tos[i];
          double r;
          switch (op) {
            case FRA_CALC_NEG: r = -x; break;
            case FRA_CALC_ABS: r = fabs(x); break;
            case FRA_CALC_SQRT: r = sqrt(x); break;
            case FRA_CALC_FLOOR: r = floor(x); break;
            default: r = x != 0.0 ? 0.0 : 1.0; break;
          }
          tos[i] = r;
        }
      } else if (op == FRA_CALC_SELECT) {
#pragma unroll
        for (int i = 0; i < P; i++) {
          const double c = slot(sp - 3, i), a = slot(sp - 2, i);
          tos[i] = c != 0.0 ? a : tos[i];
        }
        sp -= 2;
      } else {  // the binary ops: a below the top, b on top
        double a[P];
#pragma unroll
        for (int i = 0; i < P; i++) a[i] = slot(sp - 2, i);
        sp--;
        switch (op) {
#define FRA_CALC_BIN(OP, EXPR)                \
  case OP:                                    \
    _Pragma("unroll") for (int i = 0; i < P; i++) { \
      const double x = a[i], y = tos[i];      \
      tos[i] = (EXPR);                        \
    }                                         \
    break;
          FRA_CALC_BIN(FRA_CALC_ADD, x + y)
          FRA_CALC_BIN(FRA_CALC_SUB, x - y)
          FRA_CALC_BIN(FRA_CALC_MUL, x * y)
          FRA_CALC_BIN(FRA_CALC_DIV, x / y)
          FRA_CALC_BIN(FRA_CALC_MIN, x < y ? x : y)
          FRA_CALC_BIN(FRA_CALC_MAX, x > y ? x : y)
          FRA_CALC_BIN(FRA_CALC_LT, x < y ? 1.0 : 0.0)
          FRA_CALC_BIN(FRA_CALC_LE, x <= y ? 1.0 : 0.0)
          FRA_CALC_BIN(FRA_CALC_GT, x > y ? 1.0 : 0.0)
          FRA_CALC_BIN(FRA_CALC_GE, x >= y ? 1.0 : 0.0)
          FRA_CALC_BIN(FRA_CALC_EQ, x == y ? 1.0 : 0.0)
          FRA_CALC_BIN(FRA_CALC_NE, x != y ? 1.0 : 0.0)
          FRA_CALC_BIN(FRA_CALC_AND, ((x != 0.0) & (y != 0.0)) ? 1.0 : 0.0)
          FRA_CALC_BIN(FRA_CALC_OR, ((x != 0.0) | (y != 0.0)) ? 1.0 : 0.0)
#undef FRA_CALC_BIN
          default: break;  // (the host has checked every op)
        }
      }
    }
    at.next(g.plan);
  }

  if (g.use_nd) {
    uint32_t s = nleft;  // a wave's slots x P stay below 2^32 as well
#pragma unroll
    for (int off = 32; off; off >>= 1) s += __shfl_down(s, off, 64);
    if ((tid & 63u) == 0 && s) atomicAdd(g.left, (unsigned long long)s);
  }
}

thread_local float g_calc_ms = 0.f;

constexpr const char* kNot = "mapped in one call";  // (too_many_pixels)

// k_calc over a (channels, h, w) device raster into a device raster, timed; the left-out count to `left_out` (nout words)
int run_calc(Call& c, const fra_calc_program& p, int deepest, int sdtype, int32_t h, int32_t w, const Io& io, int ddtype,
             uint64_t* left_out) {
  CalcArgs g{};
  g.src = io.src, g.dst = io.out.dev;
  g.sbs = io.ss.band, g.srs = io.ss.row, g.scs = io.ss.col;
  g.dbs = io.ds.band, g.drs = io.ds.row, g.dcs = io.ds.col;
  g.nodata = p.nodata, g.fill = p.fill;
  g.h = h, g.w = w;
  g.svec = aligned16(io.src, io.ss, (size_t)elem_size(sdtype));
  g.dvec = aligned16(io.out.dev, io.ds, (size_t)elem_size(ddtype));
  g.use_nd = (p.flags & FRA_CALC_NODATA) ? (p.nodata == p.nodata ? 1 : 2) : 0;
  g.ncode = p.ncode;
  std::memcpy(g.code, p.code, sizeof(g.code));
  std::memcpy(g.consts, p.consts, sizeof(g.consts));
  const int below = std::max(0, deepest - 1);  // the values the LDS holds per pixel
  const int P = (int64_t)below * 8 * 256 * (int64_t)sizeof(double) <= kWideLds ? 8 : 4;
  // (a chunk's pixels are counted in 32 bits: 2^29 slots of 8)
  if (const int rc = plan_chunks(&g.plan, P, h, w, 1, (int64_t)1 << 29, 0, "band math call")) return rc;
  const unsigned grid = g.plan.grid;
  const size_t lds = (size_t)below * P * 256 * sizeof(double);
  HIPCHK(c.sc.alloc(&g.left, sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(g.left, 0, sizeof(unsigned long long), c.s));
  unsigned long long left = 0;
  const int rc = timed(
      c, &g_calc_ms,
      [&]() -> int {
        with_dtype(sdtype, [&](auto s) {
          with_dtype(ddtype, [&](auto d) {
            if (P == 8) hipLaunchKernelGGL((k_calc<decltype(s), decltype(d), 8>), dim3(grid), dim3(256), lds, c.s, g);
            else hipLaunchKernelGGL((k_calc<decltype(s), decltype(d), 4>), dim3(grid), dim3(256), lds, c.s, g);
          });
        });
        HIPCHK(hipGetLastError());
        return FRA_OK;
      },
      [&]() -> int {
        HIPCHK(hipMemcpyAsync(&left, g.left, sizeof(left), hipMemcpyDeviceToHost, c.s));
        return copy_back(c, io.out);
      });
  if (rc) return rc;
  if (left_out)
    for (int k = 0; k < p.nout; k++) left_out[k] = (uint64_t)left;
  return FRA_OK;
}

// the destination's dtype and layout, for an output of p's bands
int check_dst(const fra_calc_program* p, const fra_calc_dst* o, int32_t h, int32_t w) {
  const Strides ds{o->band_stride, o->row_stride, o->col_stride};
  return check_raster(o->dtype, p->nout, h, w, ds, ds);
}

}  // namespace

extern "C" {

FRA_API int fra_calc_check(const fra_calc_program* program, int32_t channels) {
  return fra_calcp::check_program(program, channels, nullptr);
}

FRA_API int fra_calc_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_calc_ms;
  return FRA_OK;
}

FRA_API int fra_calc(fra_ctx* ctx, const fra_calc_job* job, uint64_t* left_out) {
  if (!ctx || !job || !job->src || !job->out.dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  const fra_calc_program& p = job->program;
  int deepest = 0;
  if (const int rc = fra_calcp::check_program(&p, job->channels, &deepest)) return rc;
  const Strides ss{job->band_stride, job->row_stride, job->col_stride};
  const int32_t h = job->height, w = job->width;
  if (const int rc = check_raster(job->dtype, job->channels, h, w, ss, ss)) return rc;
  if (const int rc = check_dst(&p, &job->out, h, w)) return rc;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  const fra_calc_dst& o = job->out;
  return run_raster_to(ctx, job->src, job->src_on_device, job->dtype, job->channels, h, w, ss,
                       Dst{o.dst, o.dst_on_device, o.dtype, p.nout, h, w, {o.band_stride, o.row_stride, o.col_stride}},
                       [&](Call& c, Io& io) { return run_calc(c, p, deepest, job->dtype, h, w, io, o.dtype, left_out); });
}

FRA_API int fra_decode_device_calc(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                   const fra_calc_program* program, const fra_calc_dst* out, uint64_t* left_out,
                                   fra_decoded* infos) {
  if (!ctx || !job || !roi || !program || !out || !out->dst || !infos)
    return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (left_to_window_read_no_dst(job, roi)) return refer_to_window_read(ctx, job, roi, infos, true);
  int deepest = 0;
  if (const int rc = fra_calcp::check_program(program, job->channels, &deepest)) return rc;
  const int32_t h = roi->height, w = roi->width;
  if (const int rc = check_dst(program, out, h, w)) return rc;
  if (const int rc = too_many_pixels(h, w, kNot)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region_to(
      ctx, job, roi, infos,
      Dst{out->dst, out->dst_on_device, out->dtype, program->nout, h, w, {out->band_stride, out->row_stride, out->col_stride}},
      [&](Call& c, Io& io) { return run_calc(c, *program, deepest, job->dst_dtype, h, w, io, out->dtype, left_out); });
}

}  // extern "C"
