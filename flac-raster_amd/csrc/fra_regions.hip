// fra_regions.hip -- connected components of a raster's foreground, their areas and boxes, and the sieve
// (include/flac_raster_amd.h, "Regions"; the rule in numpy: flac_raster/regions.py).  A band goes through four phases
// on two scratch arrays, a link byte and a 32-bit parent per pixel:
//
//   Links.  k_reg_links reads the source (the only kernel templated on its dtype) and writes per pixel the foreground
//   bit and the link bits towards W, N, NW and NE.  Everything below reads these bytes alone.
//
//   Tiles.  k_reg_tile labels a tile of 64 x 64 pixels in LDS: a thread walks 16 pixels of a tile row, starts every
//   pixel at the first pixel of its run inside those 16, and unites across the links that are left (a link whose two
//   ends are joined by two other links of the same 2 x 2 block is skipped).  Every pixel then finds its root and
//   writes it, as a pixel index of the region, to the parent array; a background pixel gets kBackground.
//
//   Seams.  k_reg_seam takes the links that cross a tile border, one thread per border pixel, and unites their ends on
//   the parent array.
//
//   Flatten, count, number, write.  k_reg_flatten points every pixel at its root.  A root is the smallest pixel index
//   of its component -- its first pixel -- so a prefix sum over the roots in raster order (k_reg_scan_*) numbers the
//   components before the sieve in the rule's order; the root's parent word becomes kRootBit | that index.
//   k_reg_accum adds up areas and boxes per component with integer atomics, after merging a thread's runs and, in
//   LDS, what the workgroup has of its dominant component.  A second prefix sum over the components that pass the
//   sieve gives the final numbers, and k_reg_write / k_reg_table write the outputs.
//
// The union-find.  parent[x] <= x always: a tile writes the least index of a tile component, and afterwards a word is
// only ever lowered, by an atomic min.  So a find walks strictly downwards and ends, and a union that loses a race
// retries from the strictly smaller index the atomic returned.  No kernel waits for another workgroup: the order between
// phases is the order of the kernels.  Only integer min, max and add atomics are used, whose results do not depend on
// the order of arrival, so a result is the same from run to run.
//
// Shared with the other units over fra_region.h: the layout refusal, what is left to the windowed read, staging, the
// decode of a region and to_out.  The refusals, the FRA_E_SPACE decisions and the launch plan are in fra_regions.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "fra_regions.h"

namespace {

using namespace fra_region;
using namespace fra_rg;
using fra_px::is_target;
using fra_px::out_bits;

struct RegArgs {
  const void* src;           // element (row 0, col 0) of the band
  int64_t srs, scs;          // of the source, in elements
  int32_t h, w;
  int32_t nvalues, invert, by_value, conn8;
  double values[16];
  uint8_t* link;             // h x w
  uint32_t* parent;          // h x w
  uint32_t* fg_part;         // per tile: its foreground pixels
  // the components before the sieve, in the order of their first pixels
  uint32_t ncomp;
  uint32_t* root;            // the first pixel
  uint32_t* area;
  int32_t* box;              // rmin, cmin, rmax, cmax
  uint32_t* number;          // 1 .. N for a kept one, 0 for a removed one
  uint32_t min_size;
  int32_t need_area, need_box;
  uint32_t* blk;             // the block sums of a prefix sum, then their exclusive prefix
  uint32_t* blk_area;        // ... and the kept pixels per block (second scan)
  uint32_t* res;             // foreground pixels, components, kept components, kept pixels
  // the outputs of the band (null: not wanted)
  void* labels; int32_t ldtype; int64_t lrs, lcs;
  void* area_out; int32_t adtype; int64_t ars, acs;
  void* sieved; int64_t vrs, vcs; unsigned long long sieve_fill;
  fra_region_rec* table;
};

// a forest in LDS or in global memory: the parent of x, and min(parent of x, v) returning what was there
struct LdsForest {
  uint32_t* p;
  __device__ uint32_t load(uint32_t x) const { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ uint32_t lower(uint32_t x, uint32_t v) const { return __hip_atomic_fetch_min(p + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
// Agent scope for every access of k_reg_seam: the min is carried out at the memory side, on the one true word.  The
// load may be served by this XCD's L2 with an older value of the word; every older value is an ancestor of x that was
// its parent once, so the walk stays inside x's component and above its root, and what it ends at is only a proposal
// that the atomic min then checks against the true word.
struct GlobalForest {
  uint32_t* p;
  __device__ uint32_t load(uint32_t x) const { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ uint32_t lower(uint32_t x, uint32_t v) const { return __hip_atomic_fetch_min(p + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

template <typename F>
__device__ inline uint32_t find(const F& f, uint32_t x) {
  // ends: a parent that differs from x is smaller than x, so x strictly decreases
  for (;;) {
    const uint32_t p = f.load(x);
    if (p >= x) return x;  // (a root; never above x: see the head of the file)
    x = p;
  }
}

template <typename F>
__device__ inline void unite(const F& f, uint32_t a, uint32_t b) {
  // ends: every round either returns or replaces a by a strictly smaller index (old < a, as a parent that is not the
  // index itself is smaller), and b never grows
  for (;;) {
    a = find(f, a), b = find(f, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = f.lower(a, b);  // a > b: the larger root goes below the smaller
    if (old == a) return;                // a was a root and is now linked
    a = old;                             // somebody linked a to old first: old and b are still to be united
  }
}

// grid (link_wgs): a pixel per thread
template <typename T>
__global__ void __launch_bounds__(kThreads) k_reg_links(RegArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)a.h * a.w) return;
  const int32_t r = (int32_t)(i / a.w), c = (int32_t)(i % a.w);
  const T* const s = (const T*)a.src;
  auto at = [&](int32_t rr, int32_t cc) { return s[(int64_t)rr * a.srs + (int64_t)cc * a.scs]; };
  auto fg = [&](T v) { return v == v && (is_target(v, a.nvalues, a.values) != (a.invert != 0)); };
  const T v = at(r, c);
  unsigned bits = 0;
  if (fg(v)) {
    bits = kFg;
    auto linked = [&](int32_t rr, int32_t cc) {
      if (rr < 0 || cc < 0 || cc >= a.w) return false;
      const T u = at(rr, cc);
      return fg(u) && (!a.by_value || u == v);
    };
    if (linked(r, c - 1)) bits |= kW;
    if (linked(r - 1, c)) bits |= kN;
    if (a.conn8) {
      if (linked(r - 1, c - 1)) bits |= kNW;
      if (linked(r - 1, c + 1)) bits |= kNE;
    }
  }
  a.link[i] = (uint8_t)bits;
}

// grid (tiles_x, tiles_y): thread t has the pixels t % 4 * 16 .. + 15 of tile row t / 4
__global__ void __launch_bounds__(kThreads) k_reg_tile(RegArgs a) {
  __shared__ uint32_t lab[kTile * kTile];
  __shared__ uint8_t lk[kTile * kTile];
  const int32_t t = (int32_t)threadIdx.x, lr = t / (kTile / kRun), lc0 = t % (kTile / kRun) * kRun;
  const int32_t r = (int32_t)blockIdx.y * kTile + lr, c0 = (int32_t)blockIdx.x * kTile + lc0;
  const uint32_t p0 = (uint32_t)(lr * kTile + lc0);
  const LdsForest f{lab};

  // the link bytes, without the links that leave the tile; every pixel starts at the first pixel of its run
  uint32_t nfg = 0, start = p0;
  for (int32_t j = 0; j < kRun; j++) {
    const int32_t lc = lc0 + j, c = c0 + j;
    unsigned bits = (r < a.h && c < a.w) ? a.link[(int64_t)r * a.w + c] : 0u;
    if (lc == 0) bits &= ~(kW | kNW);
    if (lr == 0) bits &= ~(kN | kNW | kNE);
    if (lc == kTile - 1) bits &= ~kNE;
    if (j == 0 || !(bits & kW)) start = p0 + (uint32_t)j;
    lk[p0 + j] = (uint8_t)bits;
    lab[p0 + j] = (bits & kFg) ? start : kBackground;
    nfg += bits & kFg;
  }
  __syncthreads();

  // the links that the runs do not hold
  for (int32_t j = 0; j < kRun; j++) {
    const uint32_t p = p0 + (uint32_t)j;
    const unsigned bits = lk[p];
    if (j == 0 && (bits & kW)) unite(f, p, p - 1);
    if (bits & kN) {
      // p ~ p-1 ~ p-1-kTile ~ p-kTile already
      const bool implied = (bits & kW) && (lk[p - 1] & kN) && (lk[p - kTile] & kW);
      if (!implied) unite(f, p, p - kTile);
    }
    if (bits & kNW) {
      const bool implied = ((bits & kN) && (lk[p - kTile] & kW)) || ((bits & kW) && (lk[p - 1] & kN));
      if (!implied) unite(f, p, p - kTile - 1);
    }
    if (bits & kNE) {
      const bool implied = (bits & kN) && (lk[p - kTile + 1] & kW);
      if (!implied) unite(f, p, p - kTile + 1);
    }
  }
  __syncthreads();

  // The first pixel of every run to its root.  The other pixels of a run point at it and are never roots, so a union
  // never touched them: one walk per run instead of one per pixel (in a full tile the walks are 64 steps long).  A store
  // lowers a word to an ancestor, which the walks of the other threads may meet or miss alike.
  for (int32_t j = 0; j < kRun; j++) {
    const uint32_t p = p0 + (uint32_t)j;
    const unsigned bits = lk[p];
    if ((bits & kFg) && (j == 0 || !(bits & kW))) {
      const uint32_t root = find(f, p);
      __hip_atomic_store(lab + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();

  // the root of every pixel as an index of the region: the least local index is the least one of the region too
  for (int32_t j = 0; j < kRun; j++) {
    const int32_t c = c0 + j;
    if (r >= a.h || c >= a.w) continue;
    const uint32_t p = p0 + (uint32_t)j;
    uint32_t out = kBackground;
    if (lk[p] & kFg) {
      const uint32_t first = (j == 0 || !(lk[p] & kW)) ? p : lab[p];  // of the pixel's run
      const uint32_t root = lab[first];
      out = (uint32_t)(((int32_t)blockIdx.y * kTile + (int32_t)(root / kTile)) * a.w + (int32_t)blockIdx.x * kTile + (int32_t)(root % kTile));
    }
    a.parent[(int64_t)r * a.w + c] = out;
  }
  const uint32_t total = wg_sum(nfg);
  if (t == 0) a.fg_part[blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// grid (seam_wgs): the links across the tile borders (fra_regions.h, Plan)
__global__ void __launch_bounds__(kThreads) k_reg_seam(RegArgs a, int64_t nrow, int64_t ncol) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const GlobalForest f{a.parent};
  const uint32_t w = (uint32_t)a.w;
  if (idx < nrow) {
    const int32_t r = (int32_t)(idx / a.w + 1) * kTile, c = (int32_t)(idx % a.w);
    const uint32_t p = (uint32_t)r * w + (uint32_t)c;
    const unsigned bits = a.link[p];
    // As in a tile, a link whose ends two other links of its 2 x 2 block join is skipped: those links are united in a
    // tile, or by another thread of this kernel, or are skipped for the same reason one pixel further left.  Along a
    // border between two full tiles one union is left of 64.
    if (bits & kN) {
      const bool implied = (bits & kW) && (a.link[p - 1] & kN) && (a.link[p - w] & kW);
      if (!implied) unite(f, p, p - w);
    }
    if (bits & kNW) {
      const bool implied = ((bits & kN) && (a.link[p - w] & kW)) || ((bits & kW) && (a.link[p - 1] & kN));
      if (!implied) unite(f, p, p - w - 1);
    }
    if (bits & kNE) {
      const bool implied = (bits & kN) && (a.link[p - w + 1] & kW);
      if (!implied) unite(f, p, p - w + 1);
    }
  } else if (idx < nrow + ncol) {
    const int64_t j = idx - nrow;
    const int32_t c = (int32_t)(j / a.h + 1) * kTile, r = (int32_t)(j % a.h);
    const uint32_t p = (uint32_t)r * w + (uint32_t)c;
    const unsigned bits = a.link[p];
    if (bits & kW) {
      // p ~ p-w ~ p-w-1 ~ p-1 already.  Not at a four-tile corner: there the N link of p is a seam link too, which is
      // skipped for the sake of this one, and one of the two has to be united.
      const bool implied = r % kTile != 0 && (bits & kN) && (a.link[p - w] & kW) && (a.link[p - 1] & kN);
      if (!implied) unite(f, p, p - 1);
    }
    if (r % kTile != 0) {
      if (bits & kNW) {
        const bool implied = ((bits & kN) && (a.link[p - w] & kW)) || ((bits & kW) && (a.link[p - 1] & kN));
        if (!implied) unite(f, p, p - w - 1);
      }
      const unsigned left = a.link[p - 1];
      if (left & kNE) {
        const bool implied = (left & kN) && (a.link[p - w] & kW);
        if (!implied) unite(f, p - 1, p - w);
      }
    }
  }
}

// grid (link_wgs): every pixel to its root, a pixel per thread, so that the walks of a wave -- dependent loads, mostly
// of the same few words -- run side by side (folded into the counting pass below, sixteen pixels per thread one after
// the other, the same work took 0.7 ms longer over the benchmark's grid).  Other threads lower other words meanwhile,
// each to its own root: whatever a load returns is an ancestor, and the walk ends at the root, which no thread changes.
__global__ void __launch_bounds__(kThreads) k_reg_flatten(RegArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)a.h * a.w) return;
  const uint32_t p = a.parent[i];
  if (p == kBackground || p == (uint32_t)i) return;
  const uint32_t root = find(GlobalForest{a.parent}, p);
  if (root != p) a.parent[i] = root;
}

// the exclusive prefix of v over the workgroup's threads, and the total
__device__ inline uint32_t wg_excl_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t s[kThreads];
  const uint32_t t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < (uint32_t)kThreads; d <<= 1) {
    const uint32_t x = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  const uint32_t incl = s[t];
  *total = s[kThreads - 1];
  __syncthreads();
  return incl - v;
}

// The two prefix sums.  kRoots: over the pixels, an item is a root (its parent is itself).  kKept: over the components
// before the sieve, an item passes the sieve.
enum ScanMode { kRoots = 0, kKept = 1 };
template <int MODE>
__device__ inline bool scan_flag(const RegArgs& a, int64_t i) {
  if (MODE == kRoots) return a.parent[i] == (uint32_t)i;
  return !a.need_area || a.area[i] >= a.min_size;
}

// grid (blocks): the items of a block that count, and in kKept their pixels
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_reg_scan_count(RegArgs a, int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * kScanBlock + (int64_t)threadIdx.x * kScanItems;
  uint32_t cnt = 0, px = 0;
  for (int j = 0; j < kScanItems; j++) {
    const int64_t i = base + j;
    if (i < n && scan_flag<MODE>(a, i)) {
      cnt++;
      if (MODE == kKept && a.need_area) px += a.area[i];
    }
  }
  const uint32_t total = wg_sum(cnt);
  if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
  if (MODE == kKept) {
    __syncthreads();  // (wg_sum's LDS words are read by thread 0 above)
    const uint32_t tpx = wg_sum(px);
    if (threadIdx.x == 0) a.blk_area[blockIdx.x] = tpx;
  }
}

// one workgroup: the block sums become their exclusive prefix; res[slot] = the total, and in kKept res[slot + 1] = the
// pixels.  In kRoots it also adds up the tiles' foreground counts into res[0].
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_reg_scan_blocks(RegArgs a, uint32_t nb, uint32_t ntiles) {
  const uint32_t t = threadIdx.x, per = (nb + kThreads - 1) / kThreads;
  const uint32_t lo = min(nb, t * per), hi = min(nb, lo + per);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += a.blk[i];
  uint32_t total = 0;
  uint32_t run = wg_excl_scan(sum, &total);
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t v = a.blk[i];
    a.blk[i] = run;
    run += v;
  }
  uint32_t other = 0;
  if (MODE == kRoots) {
    for (uint32_t i = t; i < ntiles; i += kThreads) other += a.fg_part[i];
  } else {
    for (uint32_t i = t; i < nb; i += kThreads) other += a.blk_area[i];
  }
  const uint32_t tother = wg_sum(other);
  if (t == 0) {
    if (MODE == kRoots) a.res[0] = tother, a.res[1] = total;
    else a.res[2] = total, a.res[3] = tother;
  }
}

// grid (blocks): kRoots: component k's first pixel, and the root's parent word becomes kRootBit | k (a thread reads and
// writes the words of its own items only).  kKept: the final number of component k.
template <int MODE>
__global__ void __launch_bounds__(kThreads) k_reg_scan_write(RegArgs a, int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * kScanBlock + (int64_t)threadIdx.x * kScanItems;
  uint32_t flags = 0, cnt = 0;
  for (int j = 0; j < kScanItems; j++) {
    const int64_t i = base + j;
    if (i < n && scan_flag<MODE>(a, i)) flags |= 1u << j, cnt++;
  }
  uint32_t total = 0;
  uint32_t pos = a.blk[blockIdx.x] + wg_excl_scan(cnt, &total);
  for (int j = 0; j < kScanItems; j++) {
    const int64_t i = base + j;
    if (i >= n) break;
    const bool on = (flags >> j) & 1u;
    if (MODE == kRoots) {
      if (on) {
        if (pos < a.ncomp) a.root[pos] = (uint32_t)i;  // (always: the table was sized by this very count)
        a.parent[i] = kRootBit | pos;
      }
    } else {
      a.number[i] = on ? pos + 1 : 0u;
    }
    pos += on;
  }
}

// grid (blocks over ncomp): empty areas and boxes
__global__ void __launch_bounds__(kThreads) k_reg_init(RegArgs a) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= a.ncomp) return;
  a.area[k] = 0;
  if (a.need_box) {
    a.box[4 * (size_t)k + 0] = 0x7fffffff, a.box[4 * (size_t)k + 1] = 0x7fffffff;
    a.box[4 * (size_t)k + 2] = -1, a.box[4 * (size_t)k + 3] = -1;
  }
}

// the component index of a pixel after the numbering of the roots, kBackground for a background pixel
__device__ inline uint32_t comp_of(const RegArgs& a, int64_t i) {
  const uint32_t p = a.parent[i];
  if (p == kBackground) return p;
  const uint32_t k = (p & kRootBit) ? (p & ~kRootBit) : (a.parent[p] & ~kRootBit);
  return k < a.ncomp ? k : kBackground;  // (always below: the bound of every table access that follows)
}

// grid (tiles_x, tiles_y), the threads as in k_reg_tile: areas and boxes.  A thread merges its 16 pixels into runs of
// one component; the workgroup's dominant component -- that of the longest run, the greater index on a tie -- is
// merged in LDS and reaches the memory once per workgroup, every other run with one atomic per word.
__global__ void __launch_bounds__(kThreads) k_reg_accum(RegArgs a) {
  __shared__ unsigned long long s_dom;
  __shared__ uint32_t s_area;
  __shared__ int32_t s_box[4];
  const int32_t t = (int32_t)threadIdx.x, lr = t / (kTile / kRun), lc0 = t % (kTile / kRun) * kRun;
  const int32_t r = (int32_t)blockIdx.y * kTile + lr, c0 = (int32_t)blockIdx.x * kTile + lc0;
  if (t == 0) {
    s_dom = 0ull, s_area = 0;
    s_box[0] = s_box[1] = 0x7fffffff, s_box[2] = s_box[3] = -1;
  }
  __syncthreads();
  uint32_t ks[kRun];
  uint32_t best_len = 0, best_k = 0, len = 0;
#pragma unroll
  for (int j = 0; j < kRun; j++) {
    const int32_t c = c0 + j;
    ks[j] = (r < a.h && c < a.w) ? comp_of(a, (int64_t)r * a.w + c) : kBackground;
    len = (j > 0 && ks[j] == ks[j - 1]) ? len + 1 : 1;
    if (ks[j] != kBackground && len >= best_len) best_len = len, best_k = ks[j];
  }
  if (best_len) atomicMax(&s_dom, (unsigned long long)best_len << 32 | best_k);
  __syncthreads();
  const unsigned long long dom = s_dom;
  const uint32_t dom_k = dom ? (uint32_t)dom : kBackground;
  auto flush = [&](uint32_t k, uint32_t n, int32_t ca, int32_t cb) {
    if (k == dom_k) {
      atomicAdd(&s_area, n);
      if (a.need_box) atomicMin(&s_box[0], r), atomicMin(&s_box[1], ca), atomicMax(&s_box[2], r), atomicMax(&s_box[3], cb);
    } else {
      atomicAdd(&a.area[k], n);
      if (a.need_box) {
        int32_t* const b = a.box + 4 * (size_t)k;
        atomicMin(b + 0, r), atomicMin(b + 1, ca), atomicMax(b + 2, r), atomicMax(b + 3, cb);
      }
    }
  };
  int32_t from = 0;
#pragma unroll
  for (int j = 1; j <= kRun; j++) {
    if (j == kRun || ks[j] != ks[j - 1]) {
      if (ks[j - 1] != kBackground) flush(ks[j - 1], (uint32_t)(j - from), c0 + from, c0 + j - 1);
      from = j;
    }
  }
  __syncthreads();
  if (t == 0 && s_area) {
    atomicAdd(&a.area[dom_k], s_area);
    if (a.need_box) {
      int32_t* const b = a.box + 4 * (size_t)dom_k;
      atomicMin(b + 0, s_box[0]), atomicMin(b + 1, s_box[1]), atomicMax(b + 2, s_box[2]), atomicMax(b + 3, s_box[3]);
    }
  }
}

// grid (link_wgs): a pixel per thread into the outputs.  U moves the bits of a source element to `sieved`.
template <typename U>
__global__ void __launch_bounds__(kThreads) k_reg_write(RegArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)a.h * a.w) return;
  const int32_t r = (int32_t)(i / a.w), c = (int32_t)(i % a.w);
  const uint32_t k = comp_of(a, i);
  const uint32_t n = k == kBackground ? 0u : a.number[k];
  if (a.labels) {
    const int64_t off = (int64_t)r * a.lrs + (int64_t)c * a.lcs;
    switch (a.ldtype) {
      case FRA_U8: ((uint8_t*)a.labels)[off] = (uint8_t)n; break;
      case FRA_I8: ((int8_t*)a.labels)[off] = (int8_t)n; break;
      case FRA_U16: ((uint16_t*)a.labels)[off] = (uint16_t)n; break;
      case FRA_I16: ((int16_t*)a.labels)[off] = (int16_t)n; break;
      case FRA_U32: ((uint32_t*)a.labels)[off] = n; break;
      default: ((int32_t*)a.labels)[off] = (int32_t)n; break;
    }
  }
  if (a.area_out) {
    const double x = n ? (double)a.area[k] : 0.0;
    const int64_t off = (int64_t)r * a.ars + (int64_t)c * a.acs;
    switch (a.adtype) {
      case FRA_U8: ((uint8_t*)a.area_out)[off] = to_out<uint8_t>(x); break;
      case FRA_I8: ((int8_t*)a.area_out)[off] = to_out<int8_t>(x); break;
      case FRA_U16: ((uint16_t*)a.area_out)[off] = to_out<uint16_t>(x); break;
      case FRA_I16: ((int16_t*)a.area_out)[off] = to_out<int16_t>(x); break;
      case FRA_U32: ((uint32_t*)a.area_out)[off] = to_out<uint32_t>(x); break;
      case FRA_I32: ((int32_t*)a.area_out)[off] = to_out<int32_t>(x); break;
      case FRA_F32: ((float*)a.area_out)[off] = to_out<float>(x); break;
      default: ((double*)a.area_out)[off] = to_out<double>(x); break;
    }
  }
  if (a.sieved) {
    const bool removed = k != kBackground && n == 0;
    const U v = removed ? (U)a.sieve_fill : ((const U*)a.src)[(int64_t)r * a.srs + (int64_t)c * a.scs];
    ((U*)a.sieved)[(int64_t)r * a.vrs + (int64_t)c * a.vcs] = v;
  }
}

// grid (blocks over ncomp): record number - 1 of every kept component
__global__ void __launch_bounds__(kThreads) k_reg_table(RegArgs a) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= a.ncomp) return;
  const uint32_t n = a.number[k];
  if (!n) return;
  const int32_t* const b = a.box + 4 * (size_t)k;
  a.table[n - 1] = fra_region_rec{a.root[k], a.area[k], b[0], b[1], b[2], b[3]};
}

thread_local float g_reg_ms[4] = {0.f, 0.f, 0.f, 0.f};

template <typename F>
void with_bits(size_t es, F&& f) {
  switch (es) {
    case 1: f(uint8_t{}); break;
    case 2: f(uint16_t{}); break;
    case 4: f(uint32_t{}); break;
    default: f(uint64_t{}); break;
  }
}

struct Outputs { StagedOut labels, area, sieved; };

// what a call keeps over its bands: the pixel scratch, the events and the plan
struct Run {
  Plan plan;
  RegArgs a;
  int sdtype;
  size_t es;
  hipEvent_t ev[10];
};

// One band through the four phases.  counts4: the band's four counts.  With `write` the outputs and the table are
// written, unless the band's N does not fit (FRA_E_SPACE, before anything is written).
int run_band(Call& c, Run& R, const fra_regions_opts& o, int32_t band, bool write, uint64_t* counts4) {
  RegArgs& a = R.a;
  const Plan& pl = R.plan;
  HipArena tab;  // the band's component tables
  const dim3 blk(kThreads), tiles((unsigned)pl.tiles_x, (unsigned)pl.tiles_y);
  const uint32_t ntiles = (uint32_t)pl.tiles_x * (uint32_t)pl.tiles_y;
  uint32_t res[4] = {0, 0, 0, 0};

  HIPCHK(hipEventRecord(R.ev[0], c.s));
  with_dtype(R.sdtype, [&](auto t) { hipLaunchKernelGGL((k_reg_links<decltype(t)>), dim3(pl.link_wgs), blk, 0, c.s, a); });
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(R.ev[1], c.s));
  hipLaunchKernelGGL(k_reg_tile, tiles, blk, 0, c.s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(R.ev[2], c.s));
  if (pl.seam_wgs) {
    hipLaunchKernelGGL(k_reg_seam, dim3(pl.seam_wgs), blk, 0, c.s, a, pl.seam_row_threads, pl.seam_col_threads);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(R.ev[3], c.s));
  // flatten, then the roots counted per block: the number of components is needed before their tables can be made
  hipLaunchKernelGGL(k_reg_flatten, dim3(pl.link_wgs), blk, 0, c.s, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL((k_reg_scan_count<kRoots>), dim3(pl.pixel_scan_blocks), blk, 0, c.s, a, pl.npix);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL((k_reg_scan_blocks<kRoots>), dim3(1), blk, 0, c.s, a, pl.pixel_scan_blocks, ntiles);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(R.ev[4], c.s));
  HIPCHK(hipMemcpyAsync(res, a.res, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s));
  HIPCHK(hipStreamSynchronize(c.s));

  a.ncomp = res[1];
  const uint32_t comp_blocks = scan_blocks(a.ncomp), comp_wgs = (a.ncomp + kThreads - 1) / kThreads;
  a.need_area = o.min_size > 1 || o.area.dst || o.table;
  a.need_box = o.table != nullptr;
  HIPCHK(tab.alloc(&a.root, (size_t)a.ncomp * sizeof(uint32_t)));
  HIPCHK(tab.alloc(&a.area, (size_t)a.ncomp * sizeof(uint32_t)));
  HIPCHK(tab.alloc(&a.box, (size_t)a.ncomp * 4 * sizeof(int32_t)));
  HIPCHK(tab.alloc(&a.number, (size_t)a.ncomp * sizeof(uint32_t)));
  HIPCHK(tab.alloc(&a.blk_area, (size_t)(comp_blocks ? comp_blocks : 1) * sizeof(uint32_t)));
  HIPCHK(hipEventRecord(R.ev[5], c.s));
  if (a.ncomp) {
    hipLaunchKernelGGL((k_reg_scan_write<kRoots>), dim3(pl.pixel_scan_blocks), blk, 0, c.s, a, pl.npix);
    HIPCHK(hipGetLastError());
    if (a.need_area) {
      hipLaunchKernelGGL(k_reg_init, dim3(comp_wgs), blk, 0, c.s, a);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(k_reg_accum, tiles, blk, 0, c.s, a);
      HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL((k_reg_scan_count<kKept>), dim3(comp_blocks), blk, 0, c.s, a, (int64_t)a.ncomp);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_reg_scan_blocks<kKept>), dim3(1), blk, 0, c.s, a, comp_blocks, 0u);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL((k_reg_scan_write<kKept>), dim3(comp_blocks), blk, 0, c.s, a, (int64_t)a.ncomp);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(R.ev[6], c.s));
  if (a.ncomp) {
    HIPCHK(hipMemcpyAsync(res + 2, a.res + 2, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s));
    HIPCHK(hipStreamSynchronize(c.s));
    if (!a.need_area) res[3] = res[0];  // nothing is removed
  }
  for (int k = 0; k < 4; k++) counts4[k] = res[k];

  int rc = FRA_OK;
  HIPCHK(hipEventRecord(R.ev[7], c.s));
  if (write) rc = check_space(band, (int64_t)res[2], &o);
  if (write && rc == FRA_OK) {
    fra_region_rec* d_table = nullptr;
    if (o.table && res[2]) {
      if (o.table_on_device) d_table = o.table + (size_t)band * (size_t)o.table_cap;
      else HIPCHK(tab.alloc(&d_table, (size_t)res[2] * sizeof(fra_region_rec)));
    }
    a.table = d_table;
    if (a.labels || a.area_out || a.sieved) {
      with_bits(R.es, [&](auto u) { hipLaunchKernelGGL((k_reg_write<decltype(u)>), dim3(pl.link_wgs), blk, 0, c.s, a); });
      HIPCHK(hipGetLastError());
    }
    if (d_table) {
      hipLaunchKernelGGL(k_reg_table, dim3(comp_wgs), blk, 0, c.s, a);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(R.ev[8], c.s));
    if (d_table && !o.table_on_device)
      HIPCHK(hipMemcpyAsync(o.table + (size_t)band * (size_t)o.table_cap, d_table, (size_t)res[2] * sizeof(fra_region_rec),
                            hipMemcpyDeviceToHost, c.s));
  } else {
    HIPCHK(hipEventRecord(R.ev[8], c.s));
  }
  HIPCHK(hipStreamSynchronize(c.s));  // the band's tables go with `tab`
  const int seg[6][3] = {{0, 1, 0}, {1, 2, 1}, {2, 3, 2}, {3, 4, 3}, {5, 6, 3}, {7, 8, 3}};
  for (const auto& s : seg) {
    float t = 0.f;
    (void)hipEventElapsedTime(&t, R.ev[s[0]], R.ev[s[1]]);
    g_reg_ms[s[2]] += t;
  }
  return rc;
}

// every band of a (channels, h, w) device source of `sdtype` into the staged outputs
int run_regions(Call& c, const fra_regions_opts& o, int sdtype, int32_t channels, int32_t h, int32_t w, const void* src,
                const Strides& ss, const Outputs& out, uint64_t* counts) {
  Run R{};
  R.plan = make_plan(h, w);
  R.sdtype = sdtype, R.es = (size_t)elem_size(sdtype);
  const Plan& pl = R.plan;
  RegArgs& a = R.a;
  a.srs = ss.row, a.scs = ss.col, a.h = h, a.w = w;
  a.nvalues = o.nvalues, a.invert = o.invert != 0, a.by_value = o.by_value != 0, a.conn8 = o.connectivity == 8;
  std::memcpy(a.values, o.values, sizeof(a.values));
  a.min_size = (uint32_t)o.min_size;
  a.ldtype = o.labels.dtype, a.lrs = o.labels.row_stride, a.lcs = o.labels.col_stride;
  a.adtype = o.area.dtype, a.ars = o.area.row_stride, a.acs = o.area.col_stride;
  a.vrs = o.sieved.row_stride, a.vcs = o.sieved.col_stride;
  if (out.sieved.dev) a.sieve_fill = out_bits(sdtype, o.sieve_fill);
  const uint32_t ntiles = (uint32_t)pl.tiles_x * (uint32_t)pl.tiles_y;
  HIPCHK(c.sc.alloc(&a.link, (size_t)pl.npix));
  HIPCHK(c.sc.alloc(&a.parent, (size_t)pl.npix * sizeof(uint32_t)));
  HIPCHK(c.sc.alloc(&a.fg_part, (size_t)ntiles * sizeof(uint32_t)));
  HIPCHK(c.sc.alloc(&a.blk, (size_t)pl.pixel_scan_blocks * sizeof(uint32_t)));  // (no more components than pixels)
  HIPCHK(c.sc.alloc(&a.res, 4 * sizeof(uint32_t)));
  for (hipEvent_t& e : R.ev) HIPCHK(c.sc.event(&e, hipEventDefault));
  for (float& t : g_reg_ms) t = 0.f;

  std::vector<uint64_t> cnt((size_t)channels * 4, 0);
  auto set_band = [&](int32_t b) {
    a.src = (const unsigned char*)src + (size_t)((int64_t)b * ss.band) * R.es;
    a.labels = out.labels.dev ? (unsigned char*)out.labels.dev + (size_t)((int64_t)b * o.labels.band_stride) * (size_t)elem_size(o.labels.dtype) : nullptr;
    a.area_out = out.area.dev ? (unsigned char*)out.area.dev + (size_t)((int64_t)b * o.area.band_stride) * (size_t)elem_size(o.area.dtype) : nullptr;
    a.sieved = out.sieved.dev ? (unsigned char*)out.sieved.dev + (size_t)((int64_t)b * o.sieved.band_stride) * R.es : nullptr;
  };
  auto give_counts = [&]() { if (counts) std::memcpy(counts, cnt.data(), cnt.size() * sizeof(uint64_t)); };
  // With more than one band a call that may lack space counts every band first: nothing is written before every N is known.
  if (channels > 1 && may_lack_space(h, w, &o)) {
    for (int32_t b = 0; b < channels; b++) {
      set_band(b);
      if (const int rc = run_band(c, R, o, b, false, &cnt[(size_t)b * 4])) return rc;
    }
    give_counts();
    for (int32_t b = 0; b < channels; b++)
      if (const int rc = check_space(b, (int64_t)cnt[(size_t)b * 4 + 2], &o)) return rc;
  }
  for (int32_t b = 0; b < channels; b++) {
    set_band(b);
    const int rc = run_band(c, R, o, b, true, &cnt[(size_t)b * 4]);
    if (rc == FRA_E_SPACE) give_counts();  // (one band, or the first round has passed: the counts are complete)
    if (rc) return rc;
  }
  give_counts();
  if (const int rc = copy_back(c, out.labels)) return rc;
  if (const int rc = copy_back(c, out.area)) return rc;
  if (const int rc = copy_back(c, out.sieved)) return rc;
  HIPCHK(hipStreamSynchronize(c.s));
  return FRA_OK;
}

// the outputs of a call staged (a host output whole, so that the elements between the outputs keep their values)
int stage_outputs(Call& c, const fra_regions_opts& o, int sdtype, int32_t channels, int32_t h, int32_t w, Outputs* out) {
  *out = Outputs{};
  auto one = [&](const fra_calc_dst& d, int dtype, StagedOut* s) -> int {
    if (!d.dst) return FRA_OK;
    const Strides st{d.band_stride, d.row_stride, d.col_stride};
    return stage_out(c, d.dst, d.dst_on_device, (size_t)extent_of(channels, h, w, st) * (size_t)elem_size(dtype), s);
  };
  if (const int rc = one(o.labels, o.labels.dtype, &out->labels)) return rc;
  if (const int rc = one(o.area, o.area.dtype, &out->area)) return rc;
  return one(o.sieved, sdtype, &out->sieved);
}

}  // namespace

extern "C" {

FRA_API int fra_regions_timing(float* ms) {
  if (!ms) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  for (int k = 0; k < 4; k++) ms[k] = g_reg_ms[k];
  return FRA_OK;
}

FRA_API int fra_regions(fra_ctx* ctx, const fra_regions_job* job, uint64_t* counts) {
  if (!ctx || !job || !job->src) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  const Strides ss{job->band_stride, job->row_stride, job->col_stride};
  const int32_t h = job->height, w = job->width;
  if (const int rc = check_job(job->dtype, job->channels, h, w, ss, &job->opts)) return rc;
  Call c(ctx);
  const void* src = nullptr;
  if (const int rc = stage_in(c, job->src, job->src_on_device,
                              (size_t)extent_of(job->channels, h, w, ss) * (size_t)elem_size(job->dtype), &src))
    return rc;
  Outputs out;
  if (const int rc = stage_outputs(c, job->opts, job->dtype, job->channels, h, w, &out)) return rc;
  return run_regions(c, job->opts, job->dtype, job->channels, h, w, src, ss, out, counts);
}

FRA_API int fra_decode_device_regions(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi, const fra_regions_opts* opts,
                                      fra_decoded* infos, uint64_t* counts) {
  if (!ctx || !job || !roi || !opts || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (left_to_window_read_no_dst(job, roi)) return refer_to_window_read(ctx, job, roi, infos, true);
  const int32_t h = roi->height, w = roi->width;
  if (const int rc = check_job(job->dst_dtype, job->channels, h, w, Strides{0, 0, 1}, opts)) return rc;
  if (const int rc = check_cover(job, roi)) return rc;
  return run_region_src(ctx, job, roi, infos, [&](Call& c, const void* d_region, const Strides& ss) -> int {
    Outputs out;
    if (const int rc = stage_outputs(c, *opts, job->dst_dtype, job->channels, h, w, &out)) return rc;
    return run_regions(c, *opts, job->dst_dtype, job->channels, h, w, d_region, ss, out, counts);
  });
}

}  // extern "C"
