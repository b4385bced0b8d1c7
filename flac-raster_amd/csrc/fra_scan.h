// fra_scan.h -- the row-chunk scan of the units that read a (bands, h, w) raster slot by slot: fra_compare.hip,
// fra_stats.hip, fra_zonal.hip and fra_calc.hip.  A workgroup of 256 threads is one (band, chunk of rows); a chunk is cut
// into slots of V neighbouring elements of a row; a slot is one aligned vector load where the layout allows and guarded
// element loads otherwise (the slots are the same, so a result does not depend on which loads were used).  Once each:
//   * host: the 2^32-pixel refusal (too_many_pixels) and the chunk arithmetic (ChunkPlan, plan_chunks);
//   * device: the workgroup's chunk (chunk_of, chunk_at), a slot's element count and load (slot_count, load_slot), a
//     thread's row-major way through its slots (Cursor) and the walk that keeps the next slot's loads in flight while the
//     current one is accumulated (scan_row_major), the block's record through a fixed tree (block_reduce), f64 fields of
//     a band's partials added strictly in partial order (sum_in_order) and the nodata predicate (Nodata).
// The host part compiles without __HIPCC__, like the top of fra_region.h.
#pragma once
#include <cmath>

#include "fra_region.h"

namespace fra_region {

constexpr int64_t kMaxPixels = (int64_t)1 << 32;  // per band: the integer sums stay inside 64 (|x|), 65 (x) and 96 (x^2) bits
constexpr int64_t kBlocks = 4096;                 // workgroups aimed at: 16 per CU
constexpr int64_t kMinSlots = 1024;               // slots of a workgroup, at least (4 per thread), rows permitting
constexpr int64_t kThreads = 256;                 // of a workgroup: a thread owns slots t, t + 256, ... of its chunk

// `what`: the unit's phrase after "are not"
inline int too_many_pixels(int64_t h, int64_t w, const char* what) {
  if (h * w <= kMaxPixels) return FRA_OK;
  return fra_internal_set_error(FRA_E_INVALID, "more than 2^32 pixels per band (%lld x %lld) are not %s", (long long)h,
                                (long long)w, what);
}

// how a (bands, h, w) raster is cut into workgroups, and a thread's way from one of its slots to the next
struct ChunkPlan {
  uint32_t nvec;       // slots per row: ceil(w / V)
  uint32_t rpb;        // rows per workgroup
  uint32_t nchunks;    // workgroups per band: ceil(h / rpb)
  uint32_t step_rows;  // 256 / nvec and 256 % nvec: row-major, 256 slots on
  uint32_t step_vecs;
  uint32_t grid;       // nchunks x bands
};

// The plan for slots of V elements: `bands` x h rows spread over kBlocks workgroups of at least kMinSlots slots, a chunk
// of at most `slot_cap` slots (they are counted in 32 bits) and, where `pixel_cap` is not 0, of at most that many pixels.
// `bands` is 1 for a unit whose workgroup reads every band of its chunk.  FRA_E_INVALID ("... too large for one
// <noun>") for a grid past INT32_MAX.
inline int plan_chunks(ChunkPlan* p, int64_t V, int64_t h, int64_t w, int64_t bands, int64_t slot_cap, int64_t pixel_cap,
                       const char* noun) {
  const int64_t nvec = (w + V - 1) / V;
  int64_t rpb = std::max<int64_t>((h * bands + kBlocks - 1) / kBlocks, (kMinSlots + nvec - 1) / nvec);
  rpb = std::min<int64_t>(rpb, std::max<int64_t>(1, slot_cap / nvec));
  if (pixel_cap) rpb = std::min<int64_t>(rpb, std::max<int64_t>(1, pixel_cap / w));
  rpb = std::min<int64_t>(rpb, h);
  const int64_t nchunks = (h + rpb - 1) / rpb;
  if (nchunks * bands > INT32_MAX) return fra_internal_set_error(FRA_E_INVALID, "the raster is too large for one %s", noun);
  *p = ChunkPlan{(uint32_t)nvec, (uint32_t)rpb, (uint32_t)nchunks, (uint32_t)(kThreads / nvec), (uint32_t)(kThreads % nvec),
                 (uint32_t)(nchunks * bands)};
  return FRA_OK;
}

#ifdef __HIPCC__
// chunk `chunk` of a band: its first row and its rows
struct Chunk {
  int64_t band, row0;
  uint32_t chunk, rows;
};
__device__ inline Chunk chunk_at(const ChunkPlan& p, int32_t h, uint32_t chunk) {
  const int64_t row0 = (int64_t)chunk * p.rpb;
  return Chunk{0, row0, chunk, (uint32_t)min((int64_t)p.rpb, (int64_t)h - row0)};
}
// ... of workgroup `block` of a grid of nchunks x bands
__device__ inline Chunk chunk_of(const ChunkPlan& p, int32_t h, uint32_t block) {
  Chunk c = chunk_at(p, h, block % p.nchunks);
  c.band = (int64_t)(block / p.nchunks);
  return c;
}

// slot cv of a row of w elements: elements [cv V, cv V + n)
template <int V>
__device__ inline int slot_count(int32_t w, uint32_t cv) {
  return (int)min((int64_t)V, (int64_t)w - (int64_t)cv * V);
}
// ... loaded from p, its first element: one aligned vector load when `vec` and the slot is whole, else guarded element
// loads with zeros past n
template <typename T, int V>
__device__ inline VecOf<T, V> load_slot(const T* p, int64_t col_stride, bool vec, int n) {
  VecOf<T, V> v;
  if (vec && n == V) {
    v = *(const VecOf<T, V>*)p;
  } else {
#pragma unroll
    for (int i = 0; i < V; i++) v.v[i] = i < n ? p[(int64_t)i * col_stride] : (T)0;
  }
  return v;
}

// a thread's slot (row, cv) of its chunk, in row-major order
struct Cursor {
  uint32_t row, cv;
  __device__ inline Cursor(const ChunkPlan& p, uint32_t tid) : row(tid / p.nvec), cv(tid % p.nvec) {}
  __device__ inline void next(const ChunkPlan& p) {
    row += p.step_rows, cv += p.step_vecs;
    if (cv >= p.nvec) cv -= p.nvec, row++;
  }
};

// body(slot, n, row, cv) for every slot of the thread in a chunk of `rows` rows of w elements, slot = load(row, cv, n):
// the next slot's loads are issued before body runs on the current one
template <int V, typename Load, typename Body>
__device__ inline void scan_row_major(const ChunkPlan& p, uint32_t rows, int32_t w, Load&& load, Body&& body) {
  Cursor c(p, threadIdx.x);
  decltype(load(0u, 0u, 0)) next{};
  int nn = 0;
  bool have = c.row < rows;
  if (have) nn = slot_count<V>(w, c.cv), next = load(c.row, c.cv, nn);
  while (have) {
    const auto cur = next;
    const int cn = nn;
    const uint32_t row = c.row, cv = c.cv;
    c.next(p);
    have = c.row < rows;
    if (have) nn = slot_count<V>(w, c.cv), next = load(c.row, c.cv, nn);  // in flight while the current slot is accumulated
    body(cur, cn, row, cv);
  }
}

// The block's record in thread 0: a lane tree inside each wave (the record moves word by word), then the four waves in
// order through sh[4].  combine(x, y) is "x then y".
template <typename P, typename Combine>
__device__ inline P block_reduce(P p, P* sh, Combine&& combine) {
  static_assert(sizeof(P) % 8 == 0 && std::is_trivially_copyable<P>::value, "a record of 8-byte fields");
  constexpr int N = (int)(sizeof(P) / 8);
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    unsigned long long wd[N];
    __builtin_memcpy(wd, &p, sizeof(P));
#pragma unroll
    for (int i = 0; i < N; i++) wd[i] = __shfl_down(wd[i], off, 64);
    P q;
    __builtin_memcpy(&q, wd, sizeof(P));
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

// out[k], in thread 0: the f64 field f[k] of p[0 .. n) added strictly in the order of the partials, by one thread (of
// wave k) per field.  The whole workgroup calls it.
template <typename P, int N>
__device__ inline void sum_in_order(const P* p, uint32_t n, double P::*const (&f)[N], double (&s)[N][256], double (&out)[N]) {
  static_assert(N <= 4, "a wave per field");
  const uint32_t k = threadIdx.x >> 6;
  const bool adds = (threadIdx.x & 63) == 0 && k < (uint32_t)N;
  double acc = 0.0;
  for (uint32_t base = 0; base < n; base += 256) {
    const uint32_t i = base + threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; j++) s[j][threadIdx.x] = i < n ? p[i].*f[j] : 0.0;
    __syncthreads();
    const uint32_t m = min(256u, n - base);
    if (adds)
      for (uint32_t j = 0; j < m; j++) acc = acc + s[k][j];
  }
  __syncthreads();
  if (adds) s[k][0] = acc;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; j++) out[j] = s[j][0];
}

// the nodata predicate of a raster of T: x == v as f64, which for an integer T holds only for an integral v inside
// T's range (`on`: the caller's flag)
template <typename T>
struct Nodata {
  static constexpr bool FLT = std::is_floating_point<T>::value;
  std::conditional_t<FLT, double, T> nd = 0;
  bool use = false;
  __device__ inline void set(bool on, double v) {
    if (!on) return;
    if constexpr (FLT) {
      use = v == v, nd = v;
    } else {
      use = v >= (double)std::numeric_limits<T>::lowest() && v <= (double)std::numeric_limits<T>::max() && v == floor(v);
      nd = use ? (T)v : (T)0;
    }
  }
  template <typename X>
  __device__ inline bool is(X x) const { return use && x == (X)nd; }
};
#endif

}  // namespace fra_region
