// fra_resample.hip -- resampled reads: a raster at any output size (fra_resample), and a region of a set of tile
// streams decoded and resampled without the full-resolution region leaving the GPU (fra_decode_device_resampled).
//
// The rule (include/flac_raster_amd.h): each axis alone, g = gcd(w, ow), w' = w / g, ow' = ow / g; integer
// coordinates only; every f64 operation rounded on its own (the library is built with -ffp-contract=off).
//   centre   num = (2 C + 1) w' - ow', den = 2 ow', i0 = floor(num / den), t = (double)(num - i0 den) / (double)den
//   nearest  out[R, C] = in[min((2 R + 1) h' / (2 oh'), h - 1), min((2 C + 1) w' / (2 ow'), w - 1)]
//   bilinear taps i0, i0 + 1, weights [1 - t, t];  cubic  taps i0 - 1 .. i0 + 2, Catmull-Rom; tap indices clamped;
//            vertically first (top to bottom) for every tap column, then left to right; integers: rint, clamped
//   average  integer area weights vx_i, vy_j (units of 1 / ow', 1 / oh' of a source pixel), n = h' w';
//            integers: S exact in int64, rint((double)S / (double)n); floats: c_i = sum_j (double)vy_j x[j][i] top to
//            bottom, acc = sum_i (double)vx_i c_i left to right, (T)(acc / (double)n)
//
// k_resample<T, 0 | 2 | 3>: one thread per output element; a workgroup is 256 consecutive output columns of one
// output row of one band, so the row's taps and weights are wave-uniform and the column's are computed once per thread.
// k_resample<T, 1>: a workgroup is (band, output row, `per` consecutive output columns), `per` chosen by the host so
// that their source columns fit the workgroup's 256 V (V = 16 / sizeof(T)).  A thread owns V adjacent source columns
// (one 16-byte load per row when the layout allows, guarded element loads otherwise -- k_decimate's two paths) and
// accumulates them down the output row's source rows, four rows requested at once with the next four in flight; the column sums go to LDS
// once, and the threads that own an output sum their taps from there left to right.  When one output column spans more
// than 256 V source columns (per = 1) the workgroup walks its span in chunks of 256 V and thread 0 carries the sum.
// For 8- and 16-bit integers whose column sums fit 32 bits (h' 2^(8 itemsize) <= 2^31) the columns are accumulated with
// 24-bit multiplies in 32 bits (NARROW); the output's sum is 64-bit always.
// No atomics, nothing shared between workgroups; all indices are 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <type_traits>

#include "../../include/flac_raster_amd.h"
#include "fra_host.h"
#include "fra_region.h"

extern "C" void fra_internal_ctx_stream(fra_ctx* ctx, int* device, hipStream_t* stream);

namespace {

struct ResampleArgs {
  const void* src;
  void* dst;
  int64_t sbs, srs, scs;  // source element strides: band, row, column
  int64_t dbs, drs, dcs;  // destination element strides
  int32_t h, w, oh, ow;
  int64_t hr, ohr, wr, owr;  // h', oh', w', ow'
  int32_t nseg;              // workgroups per output row
  int32_t per;               // average: output columns of a workgroup
  int32_t vec;  // average: 16-byte row loads are aligned (scs == 1; base, row and band strides multiples of 16 bytes)
  int32_t narrow;  // average of 8- and 16-bit integers: a column's sum fits 32 bits (h' 2^(8 itemsize) <= 2^31)
};

template <typename T>
struct AccOf { using type = std::conditional_t<std::is_floating_point<T>::value, double, long long>; };

// a / b for a >= 0, b > 0; the 32-bit division when both fit (the 64-bit one is several times as long)
__device__ inline int64_t udiv(int64_t a, int64_t b) {
  if ((((uint64_t)a | (uint64_t)b) >> 32) == 0) return (int64_t)((uint32_t)a / (uint32_t)b);
  return (int64_t)((uint64_t)a / (uint64_t)b);
}

// i0 and t of output index C along an axis of reduced sizes (nr source, onr output)
__device__ inline void centre(int64_t C, int64_t nr, int64_t onr, int64_t* i0, double* t) {
  const int64_t num = (2 * C + 1) * nr - onr, den = 2 * onr;  // num > -den: the floor of a negative num is -1
  *i0 = num < 0 ? -1 : udiv(num, den);
  *t = (double)(num - *i0 * den) / (double)den;
}

template <int MODE>
__device__ inline void tap_weights(double t, double* wt) {
  if constexpr (MODE == FRA_RESAMPLE_BILINEAR) {
    wt[0] = 1.0 - t;
    wt[1] = t;
  } else {
    wt[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    wt[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
    wt[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    wt[3] = ((0.5 * t - 0.5) * t) * t;
  }
}

template <typename T>
__device__ inline T from_f64(double v) {
  if constexpr (std::is_floating_point<T>::value) {
    return (T)v;
  } else {
    constexpr double lo = std::is_signed<T>::value ? -(double)(1ull << (8 * sizeof(T) - 1)) : 0.0;
    constexpr double hi = (double)((1ull << (8 * sizeof(T) - (std::is_signed<T>::value ? 1 : 0))) - 1);
    return (T)(long long)fmin(fmax(rint(v), lo), hi);
  }
}

template <typename T, int MODE, bool NARROW = false>
__global__ void __launch_bounds__(256) k_resample(ResampleArgs a) {
  const T* __restrict__ src = (const T*)a.src;
  T* __restrict__ dst = (T*)a.dst;
  const uint32_t seg = blockIdx.x % (uint32_t)a.nseg;
  const uint32_t rest = blockIdx.x / (uint32_t)a.nseg;
  const int64_t R = (int64_t)(rest % (uint32_t)a.oh);
  const int64_t b = (int64_t)(rest / (uint32_t)a.oh);
  const int64_t h = a.h, w = a.w;
  if constexpr (MODE == FRA_RESAMPLE_NEAREST) {
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C >= a.ow) return;
    const int64_t r = min(udiv((2 * R + 1) * a.hr, 2 * a.ohr), h - 1);
    const int64_t c = min(udiv((2 * C + 1) * a.wr, 2 * a.owr), w - 1);
    dst[b * a.dbs + R * a.drs + C * a.dcs] = src[b * a.sbs + r * a.srs + c * a.scs];
  } else if constexpr (MODE == FRA_RESAMPLE_BILINEAR || MODE == FRA_RESAMPLE_CUBIC) {
    constexpr int NT = MODE == FRA_RESAMPLE_BILINEAR ? 2 : 4;
    constexpr int OFF = MODE == FRA_RESAMPLE_BILINEAR ? 0 : -1;
    const int64_t C = (int64_t)seg * 256 + threadIdx.x;
    if (C >= a.ow) return;
    int64_t i0y, i0x;
    double ty, tx, wy[NT], wx[NT];
    centre(R, a.hr, a.ohr, &i0y, &ty);  // wave-uniform
    centre(C, a.wr, a.owr, &i0x, &tx);
    tap_weights<MODE>(ty, wy);
    tap_weights<MODE>(tx, wx);
    const T* rows[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) rows[j] = src + (b * a.sbs + min(max(i0y + OFF + j, (int64_t)0), h - 1) * a.srs);
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < NT; i++) {
      const int64_t co = min(max(i0x + OFF + i, (int64_t)0), w - 1) * a.scs;
      double c = (double)rows[0][co] * wy[0];  // vertically, top to bottom
#pragma unroll
      for (int j = 1; j < NT; j++) c = c + (double)rows[j][co] * wy[j];
      v = i == 0 ? c * wx[0] : v + c * wx[i];  // then left to right
    }
    dst[b * a.dbs + R * a.drs + C * a.dcs] = from_f64<T>(v);
  } else {
    using A = typename AccOf<T>::type;                  // an output's sum, as the rule has it
    using CA = std::conditional_t<NARROW, int32_t, A>;  // a column's sum (NARROW: it fits 32 bits, says the host)
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int64_t SPAN = 256 * V;  // source columns of a workgroup per chunk
    constexpr int G = 4;               // source rows requested at once by 16-byte loads
    struct alignas(16) Vec { T v[V]; };
    __shared__ CA cs[V * 256];  // column sums, element i of thread t at [i * 256 + t] (conflict-free stores)
    const int tid = (int)threadIdx.x;
    const int64_t Ca = (int64_t)seg * a.per, Cb = min(Ca + (int64_t)a.per, (int64_t)a.ow);
    // the workgroup's source columns [c_lo, c_hi), walked from a multiple of V so that the vector loads stay aligned
    const int64_t c_lo = udiv(Ca * a.wr, a.owr) / V * V;
    const int64_t c_hi = min(udiv(Cb * a.wr + a.owr - 1, a.owr), w);
    // the output row's source rows [j_lo, j_hi)
    const int64_t j_lo = udiv(R * a.hr, a.ohr);
    const int64_t j_hi = min(udiv((R + 1) * a.hr + a.ohr - 1, a.ohr), h);
    const int64_t y_lo = R * a.hr, y_hi = (R + 1) * a.hr;
    const double n = (double)(a.hr * a.wr);
    A run = 0;  // the running sum of a thread's output (carried over the chunks when per == 1)
    for (int64_t base = c_lo; base < c_hi; base += SPAN) {
      const int64_t col0 = base + (int64_t)tid * V;  // first source column of this thread
      const int64_t left = col0 < c_hi ? w - col0 : 0;  // columns from col0 to the row's end; 0 past the span's end
      const bool whole = a.vec && left >= V;
      const T* p = src + (b * a.sbs + j_lo * a.srs + col0 * a.scs);
      CA acc[V];
      // the thread's columns down the rows [j_lo, j_hi), top to bottom: GR rows are requested at once and the next GR
      // are in flight while these are added; a row's V elements stay packed in four registers until then
      auto down = [&](auto gr, auto load_row) {
        constexpr int GR = decltype(gr)::value;
        uint4 next[GR];
#pragma unroll
        for (int g = 0; g < GR; g++) next[g] = j_lo + g < j_hi ? load_row(p + g * a.srs) : uint4{};
        int64_t edge = j_lo * a.ohr;  // where source row j begins, in units of 1 / oh' of a source row
        for (int64_t j0 = j_lo; j0 < j_hi; j0 += GR) {
          uint4 cur[GR];
#pragma unroll
          for (int g = 0; g < GR; g++) cur[g] = next[g];
          p += GR * a.srs;
#pragma unroll
          for (int g = 0; g < GR; g++)
            if (j0 + GR + g < j_hi) next[g] = load_row(p + g * a.srs);
#pragma unroll
          for (int g = 0; g < GR; g++) {
            if (j0 + g < j_hi) {
              const int64_t top = max(edge, y_lo);
              edge += a.ohr;
              const int64_t vy = min(edge, y_hi) - top;  // wave-uniform, 1 .. min(h', oh')
              Vec x;
              __builtin_memcpy(&x, &cur[g], 16);
#pragma unroll
              for (int i = 0; i < V; i++) {
                CA term;
                if constexpr (NARROW) term = __mul24((int)vy, (int)x.v[i]);  // both within 24 bits
                else term = (CA)vy * (CA)x.v[i];
                acc[i] = (g == 0 && j0 == j_lo) ? term : acc[i] + term;
              }
            }
          }
        }
      };
      if (whole) {
        down(std::integral_constant<int, G>{}, [](const T* q) { return *(const uint4*)q; });
      } else {  // the row's end, or a layout without aligned rows: element by element, one row ahead
        down(std::integral_constant<int, 1>{}, [&](const T* q) {
          Vec v;
#pragma unroll
          for (int i = 0; i < V; i++) v.v[i] = i < left ? q[(int64_t)i * a.scs] : (T)0;
          uint4 r;
          __builtin_memcpy(&r, &v, 16);
          return r;
        });
      }
      if (base != c_lo) __syncthreads();  // the previous chunk's sums have been read
#pragma unroll
      for (int i = 0; i < V; i++) cs[i * 256 + tid] = acc[i];
      __syncthreads();
      const int64_t lim = min(base + SPAN, c_hi);
      for (int64_t C = Ca + tid; C < Cb; C += 256) {
        const int64_t x_lo = C * a.wr, x_hi = (C + 1) * a.wr;
        const int64_t t_lo = udiv(x_lo, a.owr), t_hi = min(udiv(x_hi + a.owr - 1, a.owr), w);  // the output's taps
        const bool first = t_lo >= base;  // the output starts in this chunk
        A s = first ? (A)0 : run;
        const int64_t i_lo = max(t_lo, base), i_hi = min(t_hi, lim);
        int64_t xe = i_lo * a.owr;  // where source column i begins, in units of 1 / ow' of a source column
        for (int64_t i = i_lo; i < i_hi; i++) {
          const int64_t lft = max(xe, x_lo);
          xe += a.owr;
          const A vx = (A)(min(xe, x_hi) - lft);
          const uint32_t rel = (uint32_t)(i - base);
          const A term = vx * (A)cs[(rel % V) * 256 + rel / V];
          s = (first && i == t_lo) ? term : s + term;
        }
        run = s;
        if (t_hi <= lim) {
          T o;
          if constexpr (std::is_floating_point<T>::value) o = (T)(s / n);
          else o = (T)(long long)rint((double)s / n);
          dst[b * a.dbs + R * a.drs + C * a.dcs] = o;
        }
      }
    }
  }
}

thread_local float g_resample_ms = 0.f;

template <typename T>
void launch_t(int mode, unsigned grid, hipStream_t s, const ResampleArgs& a) {
  switch (mode) {
    case FRA_RESAMPLE_NEAREST: hipLaunchKernelGGL((k_resample<T, 0>), dim3(grid), dim3(256), 0, s, a); break;
    case FRA_RESAMPLE_AVERAGE:
      if constexpr (std::is_integral<T>::value && sizeof(T) <= 2) {
        if (a.narrow) {
          hipLaunchKernelGGL((k_resample<T, 1, true>), dim3(grid), dim3(256), 0, s, a);
          break;
        }
      }
      hipLaunchKernelGGL((k_resample<T, 1>), dim3(grid), dim3(256), 0, s, a);
      break;
    case FRA_RESAMPLE_BILINEAR: hipLaunchKernelGGL((k_resample<T, 2>), dim3(grid), dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((k_resample<T, 3>), dim3(grid), dim3(256), 0, s, a); break;
  }
}

// the sizes of a job into `a`; FRA_E_INVALID for an output size, a code or an average the rule refuses
int check_sizes(int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t resampling, int dtype, ResampleArgs* a) {
  if (oh < 1 || oh > FRA_RESAMPLE_MAX_OUT || ow < 1 || ow > FRA_RESAMPLE_MAX_OUT)
    return fra_internal_set_error(FRA_E_INVALID, "the output size must be 1 .. %d in each dimension (got %d x %d)",
                                  FRA_RESAMPLE_MAX_OUT, oh, ow);
  if (resampling < FRA_RESAMPLE_NEAREST || resampling > FRA_RESAMPLE_CUBIC)
    return fra_internal_set_error(FRA_E_INVALID, "unknown resampling %d (0 nearest, 1 average, 2 bilinear, 3 cubic)",
                                  resampling);
  const int64_t gh = std::gcd((int64_t)h, (int64_t)oh), gw = std::gcd((int64_t)w, (int64_t)ow);
  a->h = h, a->w = w, a->oh = oh, a->ow = ow;
  a->hr = h / gh, a->ohr = oh / gh, a->wr = w / gw, a->owr = ow / gw;
  if (resampling == FRA_RESAMPLE_AVERAGE) {
    const int64_t n = a->hr * a->wr;  // < 2^62
    const bool is_float = dtype == FRA_F32 || dtype == FRA_F64;
    if (is_float ? n > ((int64_t)1 << 53) : n > ((int64_t)1 << (63 - 8 * elem_size(dtype))))
      return fra_internal_set_error(FRA_E_INVALID,
                                    "average: %d x %d -> %d x %d has n = %lld weights per output pixel, more than the "
                                    "rule's exact arithmetic holds",
                                    h, w, oh, ow, (long long)n);
  }
  return FRA_OK;
}

// k_resample over device buffers between two events; enqueues only
int launch_resample(int dtype, int mode, int channels, ResampleArgs a, const void* d_src, void* d_dst, hipEvent_t e0,
                    hipEvent_t e1, hipStream_t s) {
  const size_t es = (size_t)elem_size(dtype);
  a.src = d_src;
  a.dst = d_dst;
  if (a.oh == a.h && a.ow == a.w) mode = FRA_RESAMPLE_NEAREST;  // the input itself, in every mode
  a.vec = a.scs == 1 && ((uintptr_t)d_src % 16) == 0 && (((uint64_t)a.srs * es) % 16) == 0 &&
          (((uint64_t)a.sbs * es) % 16) == 0;
  a.per = 1;
  if (mode == FRA_RESAMPLE_AVERAGE) {
    // `per` consecutive outputs cover at most ceil(per w / ow) + 1 source columns, V - 1 more from the aligned start
    const int64_t V = 16 / (int64_t)es, room = 256 * V - V - 1;
    a.per = (int32_t)std::min<int64_t>(std::max<int64_t>(room * a.owr / a.wr, 1), a.ow);
    a.nseg = (int32_t)(((int64_t)a.ow + a.per - 1) / a.per);
    a.per = (int32_t)(((int64_t)a.ow + a.nseg - 1) / a.nseg);  // the same workgroups, evenly filled
    // the weights of a column's rows sum to h' and each is at most min(h', oh') <= 65536
    a.narrow = dtype <= FRA_I16 && a.hr <= ((int64_t)1 << (31 - 8 * (int)es));
  } else {
    a.nseg = (int32_t)(((int64_t)a.ow + 255) / 256);
  }
  const int64_t grid = (int64_t)channels * a.oh * a.nseg;
  if (grid > INT32_MAX) return fra_internal_set_error(FRA_E_INVALID, "the raster is too large for one resampling");
  HIPCHK(hipEventRecord(e0, s));
  switch (dtype) {
    case FRA_U8: launch_t<uint8_t>(mode, (unsigned)grid, s, a); break;
    case FRA_I8: launch_t<int8_t>(mode, (unsigned)grid, s, a); break;
    case FRA_U16: launch_t<uint16_t>(mode, (unsigned)grid, s, a); break;
    case FRA_I16: launch_t<int16_t>(mode, (unsigned)grid, s, a); break;
    case FRA_U32: launch_t<uint32_t>(mode, (unsigned)grid, s, a); break;
    case FRA_I32: launch_t<int32_t>(mode, (unsigned)grid, s, a); break;
    case FRA_F32: launch_t<float>(mode, (unsigned)grid, s, a); break;
    case FRA_F64: launch_t<double>(mode, (unsigned)grid, s, a); break;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e1, s));
  return FRA_OK;
}

// elements addressed from element 0 by a (channels, rows, cols) raster of the given strides
int64_t extent_of(int64_t channels, int64_t rows, int64_t cols, int64_t bs, int64_t rs, int64_t cs) {
  return (channels - 1) * bs + (rows - 1) * rs + (cols - 1) * cs + 1;
}

}  // namespace

extern "C" {

FRA_API int fra_resample_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  *ms = g_resample_ms;
  return FRA_OK;
}

FRA_API int fra_resample(fra_ctx* ctx, const fra_resample_job* job) {
  if (!ctx || !job || !job->src || !job->dst) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (job->dtype < FRA_U8 || job->dtype > FRA_F64) return fra_internal_set_error(FRA_E_INVALID, "bad dtype %d", job->dtype);
  if (job->channels < 1 || job->height < 1 || job->width < 1 || job->src_band_stride < 0 || job->src_row_stride < 0 ||
      job->src_col_stride < 0 || job->dst_band_stride < 0 || job->dst_row_stride < 0 || job->dst_col_stride < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad raster layout (%d x %d x %d)", job->channels, job->height,
                                  job->width);
  ResampleArgs a{};
  if (const int rc = check_sizes(job->height, job->width, job->out_height, job->out_width, job->resampling, job->dtype, &a))
    return rc;
  a.sbs = job->src_band_stride, a.srs = job->src_row_stride, a.scs = job->src_col_stride;
  a.dbs = job->dst_band_stride, a.drs = job->dst_row_stride, a.dcs = job->dst_col_stride;

  int device = 0;
  hipStream_t s = nullptr;
  fra_internal_ctx_stream(ctx, &device, &s);
  (void)hipSetDevice(device);
  HipArena sc;  // staging buffers and events of this call, released on every path
  const size_t es = (size_t)elem_size(job->dtype);
  const size_t src_bytes = (size_t)extent_of(job->channels, a.h, a.w, a.sbs, a.srs, a.scs) * es;
  const size_t dst_bytes = (size_t)extent_of(job->channels, a.oh, a.ow, a.dbs, a.drs, a.dcs) * es;
  const void* d_src = job->src;
  void* d_dst = job->dst;
  if (!job->src_on_device) {
    void* p = nullptr;
    HIPCHK(sc.alloc(&p, src_bytes));
    HIPCHK(hipMemcpyAsync(p, job->src, src_bytes, hipMemcpyHostToDevice, s));
    d_src = p;
  }
  if (!job->dst_on_device) {  // staged whole, so that the elements between the outputs keep the caller's values
    HIPCHK(sc.alloc(&d_dst, dst_bytes));
    HIPCHK(hipMemcpyAsync(d_dst, job->dst, dst_bytes, hipMemcpyHostToDevice, s));
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(sc.event(&e0, hipEventDefault));
  HIPCHK(sc.event(&e1, hipEventDefault));
  if (const int rc = launch_resample(job->dtype, job->resampling, job->channels, a, d_src, d_dst, e0, e1, s)) return rc;
  if (!job->dst_on_device) HIPCHK(hipMemcpyAsync(job->dst, d_dst, dst_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  g_resample_ms = ms;
  return FRA_OK;
}

FRA_API int fra_decode_device_resampled(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                        int32_t out_height, int32_t out_width, int32_t resampling, fra_decoded* infos) {
  if (!ctx || !job || !roi || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  // what the windowed read refuses at once is left to it (it does so before any GPU work, with its own message)
  const bool refer = roi->height <= 0 || roi->width <= 0 || roi->row_off < 0 || roi->col_off < 0 || job->nitems < 0 ||
                     (job->nitems && !job->items) || !job->dst || job->dst_dtype < FRA_U8 || job->dst_dtype > FRA_F64 ||
                     job->channels < 1 || job->channels > 8 || job->band_stride < 0 || job->row_stride < 0 ||
                     job->col_stride < 0 || (job->flags & FRA_DECODE_CONCAT) || !fra_region::item_windows_ok(job);
  if (refer) {
    ResampleArgs unused{};
    if (const int rc = check_sizes(1, 1, out_height, out_width, resampling, FRA_U8, &unused)) return rc;
    const int rc = fra_decode_device_window(ctx, job, roi, infos);
    return rc ? rc : fra_internal_set_error(FRA_E_INVALID, "bad arguments");
  }
  ResampleArgs a{};
  if (const int rc = check_sizes(roi->height, roi->width, out_height, out_width, resampling, job->dst_dtype, &a)) return rc;
  const int64_t h = roi->height;
  if (const int rc = fra_region::check_cover(job, roi)) return rc;

  int device = 0;
  hipStream_t s = nullptr;
  fra_internal_ctx_stream(ctx, &device, &s);
  (void)hipSetDevice(device);
  HipArena sc;  // the region buffer, the staged output and the events: released on every path
  void* d_region = nullptr;  // the region at full resolution: band-planar, in dst_dtype, rows on 16-byte boundaries
  int64_t rs = 0;
  if (const int rc = fra_region::decode(ctx, job, roi, infos, sc, &d_region, &rs)) return rc;

  const size_t es = (size_t)elem_size(job->dst_dtype);
  a.sbs = h * rs, a.srs = rs, a.scs = 1;
  a.dbs = job->band_stride, a.drs = job->row_stride, a.dcs = job->col_stride;
  const size_t dst_bytes = (size_t)extent_of(job->channels, a.oh, a.ow, a.dbs, a.drs, a.dcs) * es;
  void* d_dst = job->dst;
  if (!job->dst_on_device) {
    HIPCHK(sc.alloc(&d_dst, dst_bytes));
    HIPCHK(hipMemcpyAsync(d_dst, job->dst, dst_bytes, hipMemcpyHostToDevice, s));
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(sc.event(&e0, hipEventDefault));
  HIPCHK(sc.event(&e1, hipEventDefault));
  if (const int rc = launch_resample(job->dst_dtype, resampling, job->channels, a, d_region, d_dst, e0, e1, s)) return rc;
  if (!job->dst_on_device) HIPCHK(hipMemcpyAsync(job->dst, d_dst, dst_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  g_resample_ms = ms;
  return FRA_OK;
}

}  // extern "C"
