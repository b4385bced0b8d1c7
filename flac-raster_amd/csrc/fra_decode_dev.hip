// fra_decode_dev.hip -- batched FLAC decode on the GPU: tile streams -> raster (fra_decode_device).
//
// FLAC gives a decoder three serial chains (a frame's end is known only after decoding it, subframe c+1 starts
// where c ends, every sample depends on the previous `order` ones), so there is no parallelism inside a
// subframe; a scene has 10^4..10^5 frames and that is where the parallelism lies:
//
//   host        candidates = the caller's frame offsets, or every sync position 0xFFF8/9 whose header parses and
//               whose CRC-8 holds (threads over byte ranges, at most 16; no speculative decode on the host)
//   k_dec_parse one lane per candidate: walks the frame's bits (subframe headers, warm-up, LPC parameters,
//               partitioned Rice/Rice2 residual with escapes, VERBATIM, CONSTANT) through a three-word bit window,
//               writes residuals / verbatim samples as int32 into scratch laid out in groups of 64 frames
//               ((c * blocksize + i) * 64 + lane inside a group: a wave's stores of sample i are one 256-byte run),
//               a descriptor per subframe, and per frame its byte length, sample count and status after the
//               CRC-16 from the frame's start to its decoded end.  Every read is bounded by the stream's end and
//               every loop by the block size and the unary cap, so a false candidate ends as "not a frame"
//   host        frame table D2H, chain start -> end exactly as fra_decode (fLaC at a break = next stream)
//   k_dec_restore one lane per chained (frame, channel): inverts FIXED 0-4 (registers) and LPC 1-32 (coefficients
//               and a 32-entry history ring per lane in LDS) in place with 64-bit sums, checks every sample
//               against the subframe's width
//   k_dec_scatter per (group, 64 samples): wasted-bits shift, stereo undo, optional denormalisation, an LDS
//               transpose so that scratch reads (lane-major) and raster writes (sample-major) are both contiguous
//
// fra_decode_device_window runs the same kernels over the frames that hold samples of a region of interest: the
// host selects them by frame number (fixed-blocksize streams: frame f starts at sample f * blocksize), k_dec_parse
// and k_dec_restore see only those, and k_dec_scatter clips to the region at the granularity of a frame's
// 64-sample run.  Damage in a frame that was not selected is not detected: that frame is never read.
//
// fra_internal_verify_device (fra_plan_verify) runs k_dec_parse and k_dec_restore over a plan's own frames and then
// k_dec_verify in k_dec_scatter's place: same grid and transpose, but it loads the source raster element instead of
// storing to it, normalises it anew and compares.  Nothing is written but a mismatch count and the first mismatch.
//
// On the host the three entries are one scaffold (struct Decode) and what is particular to each.  Shared: the call's
// stream and arena, the host's view of a device-resident input, opening an item (the parameters beside its frame
// offsets, or STREAMINFO and the candidate search), the layout (DecItem, groups of 64 frames, scratch, the slots'
// byte positions), staging and uploads, the launches with their five events, the infos, the copy back and the scan of
// the failure flags.  An entry adds its own refusals, where a host input lies on the device (fra_decode_device
// uploads it whole; the windowed read uploads the spans of the selected frames, so its slots are positions of that
// upload and its messages carry item-relative bytes; the verify entry takes device memory), its candidates and its
// chain: chain_stream with concatenation and capacity windows, chain_window, or the verify entry's position check.
//
// Not covered (refused, never decoded differently): 33-bit samples (side channel of a 32-bps stream); by the
// windowed read also FRA_DECODE_CONCAT, capacity windows and variable-blocksize streams.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/flac_raster_amd.h"
#include "fra_decode_host.h"
#include "fra_device.h"
#include "fra_host.h"
#include "fra_verify.h"

namespace {

using fra_dec::FrameHdr;
using fra_dec::HostCand;
using fra_dec::StreamParams;
using fra_dec::ST_NONE;
using fra_dec::ST_OK;
using fra_dec::ST_UNSUPPORTED;

constexpr int kLanes = 64;  // frames per group = lanes of a wave
constexpr uint64_t kNoFrame = ~0ull;
constexpr uint32_t kMaxUnary = 1u << 28;
enum : uint32_t { SF_CONSTANT = 0, SF_VERBATIM = 1, SF_FIXED = 2, SF_LPC = 3 };

struct DecItem {
  uint64_t end;  // absolute byte end of the item: no read goes past it
  int32_t channels, bps, sample_rate, bs_stride;
  int32_t row_off, col_off, width, height;  // the tile; row_off / col_off = destination position of its first pixel
                                             // (windowed read: below zero when the region starts inside the tile)
  double dmin, span;
};
// per item of a windowed read (the kClip instances of k_dec_restore / k_dec_scatter)
struct DecClip {
  int32_t r0, r1, c0, c1;  // tile-relative rows / columns that are written
  int64_t p_lo, p_hi;      // tile samples that are needed
};
struct DecGroup {
  uint64_t base;  // first scratch element of the group
  int32_t item, count;
};
using FrameOut = fra_dec::FrameRec;
struct DecArgs {
  const uint8_t* data;
  const DecItem* items;
  const DecGroup* groups;
  const uint64_t* starts;  // [ngroups * 64] absolute byte of every candidate (kNoFrame: empty slot)
  FrameOut* fout;          // [ngroups * 64]
  uint32_t* sdesc;         // [ngroups * 64 * 8]: kind | order << 8 | wasted << 16 | shift << 24
  int32_t* coefs;          // [ngroups * 64 * 8 * 32]
  int32_t* scratch;
  const int64_t* samp0;    // [ngroups * 64]: item-relative first sample of a chained frame, -1 otherwise
  uint32_t* fail;          // [ngroups * 64]: a reconstructed sample left the subframe's width
  void* dst;
  int64_t band_stride, row_stride, col_stride;
  int32_t dst_dtype, denorm;
  const DecClip* clips;    // [nitems], windowed read only
};

// ------------------------------------------------------------------------------------------ device bit reader
// MSB-first over data[.., end); bits past `end` read as zeros and set `bad` (as the host's Bits)
struct DBits {
  const uint8_t* d;
  uint64_t end;  // absolute byte bound
  // a three-word window over bytes [cb, cb + 24): cw and nw are in use, fw was requested one refill ahead so that its
  // load latency is covered by the ~64 bits of work in between; the read position is bit `o` (< 64) of cw
  uint64_t cb, cw, nw, fw;
  uint32_t o;
  bool bad;  // the window moved past `end` (the frame cannot be one: its end is checked against `end` as well)
  __device__ uint64_t ld(uint64_t byte) const {
    if (byte + 8 <= end) {
      uint64_t w;
      __builtin_memcpy(&w, d + byte, 8);
      return __builtin_bswap64(w);
    }
    uint64_t w = 0;
    for (uint64_t i = 0; i < 8; i++) w = (w << 8) | (byte + i < end ? (uint64_t)d[byte + i] : 0ull);
    return w;
  }
  __device__ void init(const uint8_t* data, uint64_t e, uint64_t byte) {
    d = data; end = e; cb = byte; o = 0; bad = false;
    cw = ld(byte); nw = ld(byte + 8); fw = ld(byte + 16);
  }
  __device__ uint64_t pos() const { return cb * 8 + o; }  // absolute bit position
  __device__ uint64_t peek() const { return o ? (cw << o) | (nw >> (64 - o)) : cw; }
  __device__ void skip(uint32_t n) {  // n <= 64
    o += n;
    if (o >= 64) {
      o -= 64;
      cb += 8;
      cw = nw;
      nw = fw;
      fw = ld(cb + 16);
      if (cb > end) bad = true;
    }
  }
  __device__ uint32_t get(int n) {  // n <= 32
    if (n == 0) return 0;
    const uint32_t v = (uint32_t)(peek() >> (64 - n));
    skip((uint32_t)n);
    return v;
  }
  __device__ int32_t sget(int n) {
    if (n == 0) return 0;
    const uint32_t v = get(n);
    return n == 32 ? (int32_t)v : (int32_t)(v << (32 - n)) >> (32 - n);
  }
  __device__ uint32_t unary() {  // zeros before a one; a run that reaches the end or the cap is bad
    uint32_t z = 0;
    for (;;) {
      const uint64_t w = peek();
      if (w) {
        const int lz = __builtin_clzll(w);
        skip((uint32_t)lz + 1);
        return z + (uint32_t)lz;
      }
      skip(64);
      z += 64;
      if (bad || z > kMaxUnary + 64) { bad = true; return z; }
    }
  }
};

__device__ inline bool side_channel(int assign, int c) {
  return (assign == 8 && c == 1) || (assign == 9 && c == 0) || (assign == 10 && c == 1);
}

// one candidate frame; returns its status
__device__ int parse_frame(const DecArgs& a, const DecItem& it, const DecGroup& grp, int slot, int lane, uint64_t st,
                           const uint16_t* crct, FrameOut& fo) {
  FrameHdr h;
  if (st >= it.end || !fra_dec::parse_header(a.data + st, a.data + it.end, it.sample_rate, it.bps, h)) return ST_NONE;
  if (h.channels != it.channels || h.blocksize > it.bs_stride) return ST_NONE;
  DBits br;
  br.init(a.data, it.end, st + (uint64_t)h.hdr_len);
  const int n = h.blocksize;
  for (int c = 0; c < h.channels; c++) {
    const int bps = h.bps + (side_channel(h.chan_assign, c) ? 1 : 0);
    if (br.get(1) != 0) return ST_NONE;
    const int type = (int)br.get(6);
    int wasted = 0;
    if (br.get(1)) wasted = (int)br.unary() + 1;
    if (br.bad || wasted >= bps) return ST_NONE;
    const int eb = bps - wasted;
    uint32_t kind;
    int order = 0;
    if (type == 0) kind = SF_CONSTANT;
    else if (type == 1) kind = SF_VERBATIM;
    else if (type >= 8 && type <= 12) { kind = SF_FIXED; order = type - 8; }
    else if (type >= 32) { kind = SF_LPC; order = type - 31; }
    else return ST_NONE;
    if (order > n) return ST_NONE;
    if (eb > 32) return ST_UNSUPPORTED;  // 33-bit side channel of a 32-bps stream
    int32_t* out = a.scratch + grp.base + (uint64_t)c * (uint64_t)it.bs_stride * kLanes + lane;
    int shift = 0;
    // CONSTANT keeps its value at sample 0; VERBATIM and the warm-up are eb-bit samples
    const int plain = kind == SF_CONSTANT ? 1 : (kind == SF_VERBATIM ? n : order);
    for (int i = 0; i < plain; i++) {
      out[(uint64_t)i * kLanes] = br.sget(eb);
      if (br.bad) return ST_NONE;
    }
    if (kind == SF_LPC) {
      const int prec = (int)br.get(4) + 1;
      if (prec == 16) return ST_NONE;
      shift = br.sget(5);
      if (shift < 0) return ST_NONE;
      int32_t* cf = a.coefs + ((uint64_t)slot * 8 + c) * 32;
      for (int j = 0; j < order; j++) cf[j] = br.sget(prec);
    }
    if (kind >= SF_FIXED) {
      const uint32_t method = br.get(2);
      if (method > 1) return ST_NONE;
      const int pbits = method == 0 ? 4 : 5;
      const uint32_t esc = method == 0 ? 15u : 31u;
      const int porder = (int)br.get(4);
      if (n & ((1 << porder) - 1)) return ST_NONE;
      const int psz = n >> porder;
      if (psz < order) return ST_NONE;
      uint32_t k = br.get(pbits);
      int raw = k == esc ? (int)br.get(5) : -1;
      int left = psz - order;
      for (int i = order; i < n; i++) {
        if (left == 0) {  // next partition (psz >= 1: at most one per sample)
          k = br.get(pbits);
          raw = k == esc ? (int)br.get(5) : -1;
          left = psz;
        }
        left--;
        int32_t v;
        if (raw >= 0) {
          v = br.sget(raw);
        } else {
          const uint32_t q = br.unary();
          if (br.bad || q > kMaxUnary) return ST_NONE;
          const uint64_t u = ((uint64_t)q << k) | (k ? (uint64_t)br.get((int)k) : 0ull);
          const int64_t w = (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
          if (w < INT32_MIN || w > INT32_MAX) return ST_NONE;
          v = (int32_t)w;
        }
        if (br.bad) return ST_NONE;
        out[(uint64_t)i * kLanes] = v;
      }
    }
    if (br.bad) return ST_NONE;
    a.sdesc[(uint64_t)slot * 8 + c] = kind | ((uint32_t)order << 8) | ((uint32_t)wasted << 16) | ((uint32_t)shift << 24);
  }
  const uint64_t body_end = (br.pos() + 7) >> 3;  // absolute byte after the padded subframes
  if (body_end + 2 > it.end) return ST_NONE;
  uint32_t crc = 0;
  uint64_t p = st;
  for (; p + 8 <= body_end; p += 8) {
    uint64_t w;
    __builtin_memcpy(&w, a.data + p, 8);
    w = __builtin_bswap64(w);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      crc = ((crc << 8) ^ crct[((crc >> 8) ^ (uint32_t)(w >> 56)) & 0xFF]) & 0xFFFF;
      w <<= 8;
    }
  }
  for (; p < body_end; p++) crc = ((crc << 8) ^ crct[((crc >> 8) ^ a.data[p]) & 0xFF]) & 0xFFFF;
  if (crc != (((uint32_t)a.data[body_end] << 8) | a.data[body_end + 1])) return ST_NONE;
  fo.len = (uint32_t)(body_end + 2 - st);
  fo.n = n;
  fo.assign = (uint8_t)h.chan_assign;
  fo.bps = (uint8_t)h.bps;
  return ST_OK;
}

__global__ __launch_bounds__(kLanes) void k_dec_parse(DecArgs a) {
  __shared__ uint16_t crct[256];
  for (int v = threadIdx.x; v < 256; v += kLanes) {
    uint32_t d = (uint32_t)v << 8;
    for (int b = 0; b < 8; b++) d = (d & 0x8000u) ? ((d << 1) ^ 0x8005u) : (d << 1);
    crct[v] = (uint16_t)d;
  }
  __syncthreads();
  const int g = blockIdx.x, lane = threadIdx.x, slot = g * kLanes + lane;
  const DecGroup grp = a.groups[g];
  const DecItem it = a.items[grp.item];
  FrameOut fo{0, 0, 0, 0, 0, 0};
  const uint64_t st = lane < grp.count ? a.starts[slot] : kNoFrame;
  if (st != kNoFrame) fo.status = (uint8_t)parse_frame(a, it, grp, slot, lane, st, crct, fo);
  a.fout[slot] = fo;
}

// ------------------------------------------------------------------------------------------ restore
// kClip: the windowed read, which stops at a frame's last needed sample
template <bool kClip>
__global__ __launch_bounds__(kLanes) void k_dec_restore(DecArgs a) {
  __shared__ int32_t s_coef[32 * kLanes];  // [j][lane]: a lane's column, conflict-free
  __shared__ int32_t s_hist[32 * kLanes];  // history ring, sample i at row i & 31
  const int g = blockIdx.x, c = blockIdx.y, lane = threadIdx.x, slot = g * kLanes + lane;
  const DecGroup grp = a.groups[g];
  const DecItem it = a.items[grp.item];
  if (c >= it.channels || lane >= grp.count || a.samp0[slot] < 0) return;
  const FrameOut fo = a.fout[slot];
  const uint32_t d = a.sdesc[(uint64_t)slot * 8 + c];
  const uint32_t kind = d & 0xFF;
  const int order = (int)((d >> 8) & 0xFF), wasted = (int)((d >> 16) & 0xFF), shift = (int)(d >> 24);
  if (kind < SF_FIXED) return;
  const int n = kClip ? (int)std::min<int64_t>(fo.n, a.clips[grp.item].p_hi - a.samp0[slot]) : fo.n;
  const int eb = (int)fo.bps + (side_channel(fo.assign, c) ? 1 : 0) - wasted;  // <= 32 (parse refused 33)
  // samples within eb bits keep every predictor sum below 2^53: no int64 overflow (as the host decoder)
  const int64_t lo = -((int64_t)1 << (eb - 1)), hi = ((int64_t)1 << (eb - 1)) - 1;
  int32_t* s = a.scratch + grp.base + (uint64_t)c * (uint64_t)it.bs_stride * kLanes + lane;
  bool bad = false;
  if (kind == SF_FIXED) {
    int64_t s1 = 0, s2 = 0, s3 = 0, s4 = 0;  // s[i-1] .. s[i-4]
    for (int i = 0; i < order; i++) { s4 = s3; s3 = s2; s2 = s1; s1 = s[(uint64_t)i * kLanes]; }
    for (int i0 = order; i0 < n; i0 += 8) {
      int32_t r[8];
#pragma unroll
      for (int u = 0; u < 8; u++) r[u] = i0 + u < n ? s[(uint64_t)(i0 + u) * kLanes] : 0;
#pragma unroll
      for (int u = 0; u < 8; u++) {
        if (i0 + u < n) {
          int64_t p = 0;
          switch (order) {
            case 1: p = s1; break;
            case 2: p = 2 * s1 - s2; break;
            case 3: p = 3 * s1 - 3 * s2 + s3; break;
            case 4: p = 4 * s1 - 6 * s2 + 4 * s3 - s4; break;
          }
          const int64_t v = p + r[u];
          if (v < lo || v > hi) bad = true;
          s[(uint64_t)(i0 + u) * kLanes] = (int32_t)v;
          s4 = s3; s3 = s2; s2 = s1; s1 = (int32_t)v;
        }
      }
      if (bad) break;
    }
  } else {
    const int32_t* cf = a.coefs + ((uint64_t)slot * 8 + c) * 32;
    for (int j = 0; j < order; j++) s_coef[j * kLanes + lane] = cf[j];
    for (int i = 0; i < order; i++) s_hist[(i & 31) * kLanes + lane] = s[(uint64_t)i * kLanes];
    for (int i0 = order; i0 < n; i0 += 8) {
      int32_t r[8];
#pragma unroll
      for (int u = 0; u < 8; u++) r[u] = i0 + u < n ? s[(uint64_t)(i0 + u) * kLanes] : 0;
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int i = i0 + u;
        if (i < n) {
          int64_t acc = 0;
          for (int j = 0; j < order; j++)
            acc += (int64_t)s_coef[j * kLanes + lane] * (int64_t)s_hist[((i - 1 - j) & 31) * kLanes + lane];
          const int64_t v = (acc >> shift) + r[u];
          if (v < lo || v > hi) bad = true;
          s_hist[(i & 31) * kLanes + lane] = (int32_t)v;
          s[(uint64_t)i * kLanes] = (int32_t)v;
        }
      }
      if (bad) break;
    }
  }
  if (bad) a.fail[slot] = 1;
}

// ------------------------------------------------------------------------------------------ scatter
__device__ inline double sat(double x, double lo, double hi) {
  return x != x ? 0.0 : (x < lo ? lo : (x > hi ? hi : x));
}

// one decoded sample -> the destination element (every f64 operation separate, in normalization.py's order)
__device__ inline void put_sample(const DecArgs& a, const DecItem& it, int64_t e, int32_t s) {
  if (a.denorm == FRA_DENORM_NONE) {
    if (a.dst_dtype == FRA_I16) ((int16_t*)a.dst)[e] = (int16_t)s;
    else ((int32_t*)a.dst)[e] = s;
    return;
  }
  double y;
  if (a.denorm == FRA_DENORM_INT) y = (double)s / (it.bps <= 16 ? 32767.0 : 8388607.0);
  else y = (double)(it.bps <= 16 ? s : (s >> 16)) / 32768.0;
  double x = y + 1.0;
  x = x / 2.0;
  x = x * it.span;
  x = x + it.dmin;
  switch (a.dst_dtype) {
    case FRA_U8: ((uint8_t*)a.dst)[e] = (uint8_t)sat(rint(x), 0.0, 255.0); break;
    case FRA_I8: ((int8_t*)a.dst)[e] = (int8_t)sat(rint(x), -128.0, 127.0); break;
    case FRA_U16: ((uint16_t*)a.dst)[e] = (uint16_t)sat(rint(x), 0.0, 65535.0); break;
    case FRA_I16: ((int16_t*)a.dst)[e] = (int16_t)sat(rint(x), -32768.0, 32767.0); break;
    case FRA_U32: ((uint32_t*)a.dst)[e] = (uint32_t)sat(rint(x), 0.0, 4294967295.0); break;
    case FRA_I32: ((int32_t*)a.dst)[e] = (int32_t)sat(rint(x), -2147483648.0, 2147483647.0); break;
    case FRA_F32: ((float*)a.dst)[e] = (float)x; break;
    default: ((double*)a.dst)[e] = x; break;
  }
}

// kClip: the windowed read, which writes only the item's clip rectangle and skips every 64-sample run outside it
template <bool kClip>
__global__ __launch_bounds__(256) void k_dec_scatter(DecArgs a) {
  __shared__ int32_t tile[kLanes][kLanes + 1];
  const int g = blockIdx.x, i0 = blockIdx.y * kLanes, t = threadIdx.x;
  const DecGroup grp = a.groups[g];
  const DecItem it = a.items[grp.item];
  if (i0 >= it.bs_stride) return;
  const int lane = t & 63, q = t >> 6;
  const int slot = g * kLanes + lane;
  const bool live = lane < grp.count && a.samp0[slot] >= 0;
  FrameOut fo{0, 0, 0, 0, 0, 0};
  if (live) fo = a.fout[slot];
  const uint32_t d0 = live ? a.sdesc[(uint64_t)slot * 8] : 0u;
  const uint32_t d1 = live && it.channels > 1 ? a.sdesc[(uint64_t)slot * 8 + 1] : 0u;
  const int32_t* sc = a.scratch + grp.base + lane;
  const uint64_t cstride = (uint64_t)it.bs_stride * kLanes;
  const uint32_t nsamp = (uint32_t)it.width * (uint32_t)it.height;
  // does this frame's 64-sample run hold a sample inside the clip?  Runs that do not are neither loaded (phase 1)
  // nor stored (phase 2); a block without any such run returns before touching scratch
  __shared__ uint8_t s_need[kLanes];
  bool need = live;
  DecClip cl{};
  if constexpr (kClip) {
    cl = a.clips[grp.item];
    need = false;
    if (live && i0 < fo.n && it.width > 0) {
      const int64_t s0 = a.samp0[slot];
      const int64_t pa = std::max<int64_t>(s0 + i0, cl.p_lo), pb = std::min<int64_t>(s0 + std::min(fo.n, i0 + kLanes), cl.p_hi);
      if (pa < pb) {
        const int32_t col = (int32_t)(pa % it.width);
        if (col >= cl.c0 && col < cl.c1) need = true;
        else need = pa + (col < cl.c0 ? cl.c0 - col : it.width - col + cl.c0) < pb;
      }
    }
    if (q == 0) s_need[lane] = need;
    if (!__syncthreads_or(need)) return;
  }
  for (int c = 0; c < it.channels; c++) {
    __syncthreads();
    if (need) {
      const uint32_t dc = c == 0 ? d0 : (c == 1 ? d1 : a.sdesc[(uint64_t)slot * 8 + c]);
      for (int k = 0; k < 16; k++) {
        const int i = i0 + q + 4 * k;
        if (i >= fo.n) break;
        int32_t v;
        if (fo.assign >= 8 && c < 2) {
          const int64_t x0 = (int64_t)((uint64_t)(int64_t)sc[(uint64_t)((d0 & 0xFF) ? i : 0) * kLanes] << ((d0 >> 16) & 0xFF));
          const int64_t x1 =
              (int64_t)((uint64_t)(int64_t)sc[cstride + (uint64_t)((d1 & 0xFF) ? i : 0) * kLanes] << ((d1 >> 16) & 0xFF));
          int64_t l, r;
          if (fo.assign == 8) { l = x0; r = x0 - x1; }        // L/S
          else if (fo.assign == 9) { l = x0 + x1; r = x1; }   // S/R
          else {                                              // M/S
            const int64_t m = (x0 * 2) | (x1 & 1);
            l = (m + x1) >> 1;
            r = (m - x1) >> 1;
          }
          v = (int32_t)(c == 0 ? l : r);
        } else {
          const int64_t x = (int64_t)sc[(uint64_t)c * cstride + (uint64_t)((dc & 0xFF) ? i : 0) * kLanes];
          v = (int32_t)(int64_t)((uint64_t)x << ((dc >> 16) & 0xFF));
        }
        tile[lane][i - i0] = v;
      }
    }
    __syncthreads();
    for (int k = 0; k < 16; k++) {
      const int f = q + 4 * k;  // frame of the group; lane = sample within the 64-sample run
      if (f >= grp.count) break;
      const int fs = g * kLanes + f;
      const int64_t s0 = a.samp0[fs];
      if (s0 < 0 || (kClip && !s_need[f])) continue;
      const int i = i0 + lane;
      if (i >= a.fout[fs].n) continue;
      const uint64_t p = (uint64_t)s0 + (uint64_t)i;
      if (p >= nsamp) continue;  // (the host checked the chain's sample count against the window)
      const uint32_t row = (uint32_t)p / (uint32_t)it.width, col = (uint32_t)p % (uint32_t)it.width;
      if (kClip && ((int32_t)row < cl.r0 || (int32_t)row >= cl.r1 || (int32_t)col < cl.c0 || (int32_t)col >= cl.c1))
        continue;
      const int64_t e = (int64_t)c * a.band_stride + ((int64_t)it.row_off + row) * a.row_stride +
                        ((int64_t)it.col_off + col) * a.col_stride;
      put_sample(a, it, e, tile[f][lane]);
    }
  }
}

// ------------------------------------------------------------------------------------------ verify
struct VerArgs {
  const void* src;           // the source raster; DecArgs' strides and the items' windows address it
  const fra::NormDev* nd;    // [nitems] min / max keys of the encode
  unsigned long long* res;   // [nitems][2]: mismatch count, smallest mismatching key (p << 3) | channel
  int32_t* vals;             // [nitems][2]: expected and decoded sample at that key (pass 1)
  int32_t norm, pass;
};

// k_dec_scatter<false>'s grid and phases, but phase 2 loads the source element the scatter would store to, normalises
// it by the plain f64 sequence (no table) and compares.  Pass 0 counts the mismatches of the group's item and keeps
// the smallest key; pass 1, launched only when an item has mismatches, writes both samples at that key.
template <int SRC>
__global__ __launch_bounds__(256) void k_dec_verify(DecArgs a, VerArgs v) {
  __shared__ int32_t tile[kLanes][kLanes + 1];
  const int g = blockIdx.x, i0 = blockIdx.y * kLanes, t = threadIdx.x;
  const DecGroup grp = a.groups[g];
  const DecItem it = a.items[grp.item];
  if (i0 >= it.bs_stride) return;
  unsigned long long* res = v.res + 2 * (size_t)grp.item;
  unsigned long long first = 0;
  if (v.pass) {  // (uniform over the block)
    if (res[0] == 0) return;
    first = res[1];
  }
  const int lane = t & 63, q = t >> 6;
  const int slot = g * kLanes + lane;
  const bool live = lane < grp.count && a.samp0[slot] >= 0;
  FrameOut fo{0, 0, 0, 0, 0, 0};
  if (live) fo = a.fout[slot];
  const uint32_t d0 = live ? a.sdesc[(uint64_t)slot * 8] : 0u;
  const uint32_t d1 = live && it.channels > 1 ? a.sdesc[(uint64_t)slot * 8 + 1] : 0u;
  const int32_t* sc = a.scratch + grp.base + lane;
  const uint64_t cstride = (uint64_t)it.bs_stride * kLanes;
  const uint32_t nsamp = (uint32_t)it.width * (uint32_t)it.height;
  const fra::NormParams np = fra::norm_params(v.norm, v.nd[grp.item]);
  unsigned long long nbad = 0, kmin = ~0ull;
  for (int c = 0; c < it.channels; c++) {
    __syncthreads();
    if (live) {
      const uint32_t dc = c == 0 ? d0 : (c == 1 ? d1 : a.sdesc[(uint64_t)slot * 8 + c]);
      for (int k = 0; k < 16; k++) {
        const int i = i0 + q + 4 * k;
        if (i >= fo.n) break;
        int32_t s;
        if (fo.assign >= 8 && c < 2) {
          const int64_t x0 = (int64_t)((uint64_t)(int64_t)sc[(uint64_t)((d0 & 0xFF) ? i : 0) * kLanes] << ((d0 >> 16) & 0xFF));
          const int64_t x1 =
              (int64_t)((uint64_t)(int64_t)sc[cstride + (uint64_t)((d1 & 0xFF) ? i : 0) * kLanes] << ((d1 >> 16) & 0xFF));
          int64_t l, r;
          if (fo.assign == 8) { l = x0; r = x0 - x1; }        // L/S
          else if (fo.assign == 9) { l = x0 + x1; r = x1; }   // S/R
          else {                                              // M/S
            const int64_t m = (x0 * 2) | (x1 & 1);
            l = (m + x1) >> 1;
            r = (m - x1) >> 1;
          }
          s = (int32_t)(c == 0 ? l : r);
        } else {
          const int64_t x = (int64_t)sc[(uint64_t)c * cstride + (uint64_t)((dc & 0xFF) ? i : 0) * kLanes];
          s = (int32_t)(int64_t)((uint64_t)x << ((dc >> 16) & 0xFF));
        }
        tile[lane][i - i0] = s;
      }
    }
    __syncthreads();
    for (int k = 0; k < 16; k++) {
      const int f = q + 4 * k;  // frame of the group; lane = sample within the 64-sample run
      if (f >= grp.count) break;
      const int fs = g * kLanes + f;
      const int64_t s0 = a.samp0[fs];
      if (s0 < 0) continue;
      const int i = i0 + lane;
      if (i >= a.fout[fs].n) continue;
      const uint64_t p = (uint64_t)s0 + (uint64_t)i;
      if (p >= nsamp) continue;  // (the host checked every frame's samples against the window)
      const uint32_t row = (uint32_t)p / (uint32_t)it.width, col = (uint32_t)p % (uint32_t)it.width;
      const int64_t e = (int64_t)c * a.band_stride + ((int64_t)it.row_off + row) * a.row_stride +
                        ((int64_t)it.col_off + col) * a.col_stride;
      const int32_t want = fra::fetch_sample<SRC>(v.src, e, np), got = tile[f][lane];
      if (want != got) {
        const unsigned long long key = (p << 3) | (unsigned)c;
        if (!v.pass) {
          nbad++;
          kmin = key < kmin ? key : kmin;
        } else if (key == first) {
          v.vals[2 * (size_t)grp.item] = want;
          v.vals[2 * (size_t)grp.item + 1] = got;
        }
      }
    }
  }
  if (nbad) {
    atomicAdd(&res[0], nbad);
    atomicMin(&res[1], kmin);
  }
}

// ------------------------------------------------------------------------------------------ host side
struct ItemPlan {
  bool search = false;
  StreamParams sp;
  uint64_t audio = 0;           // item-relative first audio byte (search path)
  std::vector<HostCand> cand;   // sorted by start
  size_t n = 0;                 // frames laid out: slots first_group * 64 + [0, n)
  int32_t first_group = 0;
};
struct Range { uint64_t at, bytes; };             // of the input
struct Rect { int64_t row0, col0, rows, cols; };  // of the destination, from its origin

thread_local float g_last_ms[4] = {0, 0, 0, 0};

const char kUnsupported[] = "33-bit samples (side channel of a 32-bps stream) are not supported on the device";

// the kernel times of a finished call (events: parse start / end, restore start, scatter start / end)
void keep_times(const hipEvent_t* ev) {
  float ms[4] = {0, 0, 0, 0};
  (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
  (void)hipEventElapsedTime(&ms[1], ev[2], ev[3]);
  (void)hipEventElapsedTime(&ms[2], ev[3], ev[4]);
  (void)hipEventElapsedTime(&ms[3], ev[0], ev[4]);
  memcpy(g_last_ms, ms, sizeof(ms));
}

// what both decode entries check of a job before any GPU work
int check_job(const fra_ctx* ctx, const fra_decode_job* job, const fra_decoded* infos) {
  if (!ctx || !job || !infos) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  const int ni = job->nitems;
  if (ni < 0 || (ni && !job->items) || (!job->data && job->len) || !job->dst)
    return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (job->dst_dtype < FRA_U8 || job->dst_dtype > FRA_F64)
    return fra_internal_set_error(FRA_E_INVALID, "bad dst_dtype %d", job->dst_dtype);
  if (job->denorm < FRA_DENORM_NONE || job->denorm > FRA_DENORM_PCM16)
    return fra_internal_set_error(FRA_E_INVALID, "bad denorm %d", job->denorm);
  if (job->denorm == FRA_DENORM_NONE && job->dst_dtype != FRA_I16 && job->dst_dtype != FRA_I32)
    return fra_internal_set_error(FRA_E_INVALID, "FRA_DENORM_NONE needs dst_dtype FRA_I16 or FRA_I32");
  if (job->channels < 1 || job->channels > 8 || job->band_stride < 0 || job->row_stride < 0 || job->col_stride < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad destination layout (channels %d)", job->channels);
  return FRA_OK;
}

// ... and all three entries of item i of `len` bytes of data
int check_item(const fra_decode_item& it, int i, uint64_t len) {
  if (it.offset > len || it.bytes > len - it.offset)
    return fra_internal_set_error(FRA_E_INVALID, "item %d lies outside the data", i);
  const fra_window& w = it.window;
  if (w.row_off < 0 || w.col_off < 0 || w.width < 0 || (w.height < 0 && w.width != 1) || w.height == INT32_MIN)
    return fra_internal_set_error(FRA_E_INVALID, "item %d: bad window", i);
  if ((int64_t)std::abs(w.height) * w.width > INT32_MAX)
    return fra_internal_set_error(FRA_E_INVALID, "item %d: a window of more than 2^31 - 1 samples is not supported "
                                                 "on the device", i);
  if (it.frame_offsets) {
    if (it.nframes < 0 || it.channels < 1 || it.channels > 8 || it.bps < 4 || it.bps > 32 || it.blocksize < 1 ||
        it.blocksize > 65536)
      return fra_internal_set_error(FRA_E_INVALID, "item %d: bad stream parameters", i);
    for (int f = 0; f < it.nframes; f++)
      if (it.frame_offsets[f + 1] < it.frame_offsets[f])
        return fra_internal_set_error(FRA_E_INVALID, "item %d: frame offsets are not ascending", i);
    if (it.frame_offsets[it.nframes] > it.bytes)
      return fra_internal_set_error(FRA_E_INVALID, "item %d: frame offsets run past the item", i);
  }
  return FRA_OK;
}

// what both decode entries refuse of an opened item: its channel count, then 32-bps samples into FRA_I16
int check_stream(const fra_decode_job* job, int i, const StreamParams& sp) {
  if (sp.channels != job->channels)
    return fra_internal_set_error(FRA_E_INVALID, "item %d has %d channels, the destination %d", i, sp.channels,
                                  job->channels);
  if (job->denorm == FRA_DENORM_NONE && job->dst_dtype == FRA_I16 && sp.bps > 16)
    return fra_internal_set_error(FRA_E_INVALID, "item %d: a %d-bps stream needs dst_dtype FRA_I32", i, sp.bps);
  return FRA_OK;
}

void fill_info(fra_decoded& inf, const ItemPlan& ip, int64_t nframes, uint64_t nsamples, int nstreams) {
  inf.sample_rate = ip.sp.sample_rate;
  inf.channels = ip.sp.channels;
  inf.bps = ip.sp.bps;
  inf.blocksize = ip.sp.max_bs;
  inf.nframes = nframes;
  inf.nsamples = nsamples;
  inf.nstreams = nstreams;
  inf.audio_offset = ip.audio;
}

// the per-group and per-slot tables and the scratch of one call, owned by `sc`
int alloc_tables(HipArena& sc, DecArgs& a, size_t ni, size_t ng, uint64_t scratch_elems) {
  const size_t nslots = ng * kLanes;
  void *d_items, *d_groups, *d_starts, *d_fout, *d_sdesc, *d_coefs, *d_scratch, *d_samp0, *d_fail;
  HIPCHK(sc.alloc(&d_items, sizeof(DecItem) * ni));
  HIPCHK(sc.alloc(&d_groups, sizeof(DecGroup) * ng));
  HIPCHK(sc.alloc(&d_starts, sizeof(uint64_t) * nslots));
  HIPCHK(sc.alloc(&d_fout, sizeof(FrameOut) * nslots));
  HIPCHK(sc.alloc(&d_sdesc, sizeof(uint32_t) * nslots * 8));
  HIPCHK(sc.alloc(&d_coefs, sizeof(int32_t) * nslots * 8 * 32));
  HIPCHK(sc.alloc(&d_scratch, sizeof(int32_t) * (size_t)scratch_elems));
  HIPCHK(sc.alloc(&d_samp0, sizeof(int64_t) * nslots));
  HIPCHK(sc.alloc(&d_fail, sizeof(uint32_t) * nslots));
  a.items = (const DecItem*)d_items;
  a.groups = (const DecGroup*)d_groups;
  a.starts = (const uint64_t*)d_starts;
  a.fout = (FrameOut*)d_fout;
  a.sdesc = (uint32_t*)d_sdesc;
  a.coefs = (int32_t*)d_coefs;
  a.scratch = (int32_t*)d_scratch;
  a.samp0 = (const int64_t*)d_samp0;
  a.fail = (uint32_t*)d_fail;
  return FRA_OK;
}

// k_dec_verify's instance of the source dtype, over k_dec_scatter's grid
void launch_verify(int dtype, dim3 grid, hipStream_t s, const DecArgs& a, const VerArgs& v) {
  switch (dtype) {
#define FRA_VERIFY_CASE(DT, ST) \
  case DT: hipLaunchKernelGGL(k_dec_verify<fra::ST>, grid, dim3(256), 0, s, a, v); break;
    FRA_VERIFY_CASE(FRA_U8, ST_U8)
    FRA_VERIFY_CASE(FRA_I8, ST_I8)
    FRA_VERIFY_CASE(FRA_U16, ST_U16)
    FRA_VERIFY_CASE(FRA_I16, ST_I16)
    FRA_VERIFY_CASE(FRA_U32, ST_U32)
    FRA_VERIFY_CASE(FRA_I32, ST_I32)
    FRA_VERIFY_CASE(FRA_F32, ST_F32)
    FRA_VERIFY_CASE(FRA_F64, ST_F64)
#undef FRA_VERIFY_CASE
  }
}

// One call of any of the three entries: its stream and arena (Call), the five events of keep_times, the host's view
// of the input, and the tables the kernels read, on the host and on the device (`a`).  The members are the steps the
// entries share, in the order they take them; between them an entry puts its own checks, candidates and chain, and it
// sets a.data itself: where the input lies on the device differs from entry to entry.
struct Decode : Call {
  hipEvent_t ev[5] = {};
  const uint8_t* hdata = nullptr;  // the input as the host reads it (search path)
  std::unique_ptr<uint8_t[]> hcopy;
  std::vector<ItemPlan> plan;
  std::vector<fra_dec::ScanUnit> units;
  std::vector<DecItem> h_items;  // (an item that is not laid out stays zeroed and has no groups)
  std::vector<DecGroup> h_groups;
  std::vector<uint64_t> h_starts;
  std::vector<FrameOut> h_fout;
  std::vector<int64_t> h_samp0;
  std::vector<uint32_t> h_fail;
  uint64_t scratch_elems = 0;
  int bs_max = 1;
  size_t ng = 0, nslots = 0;
  DecArgs a{};
  size_t dst_bytes = 0;
  bool by_window = false;  // a host destination comes back rectangle by rectangle

  Decode(fra_ctx* ctx, int ni) : Call(ctx), plan((size_t)ni), h_items((size_t)ni) {}

  // the host's view of the input: host memory as it is; of device memory a copy of `read` (the candidate search and
  // the chain read the bytes on the host), none when `read` is empty
  int host_view(const fra_decode_job* job, const std::vector<Range>& read) {
    hdata = job->data_on_device ? nullptr : job->data;
    if (read.empty() || !job->data_on_device) return FRA_OK;
    hcopy.reset(new (std::nothrow) uint8_t[(size_t)job->len + 1]);  // (only the ranges copied below are touched)
    if (!hcopy) return fra_internal_set_error(FRA_E_NOMEM, "out of host memory");
    for (const Range& r : read)
      if (r.bytes) HIPCHK(hipMemcpy(hcopy.get() + r.at, job->data + r.at, (size_t)r.bytes, hipMemcpyDeviceToHost));
    hdata = hcopy.get();
    return FRA_OK;
  }

  // item i's stream parameters: from the item beside its frame offsets, else from its STREAMINFO, and then its bytes
  // from the first audio byte on are queued for the candidate search in units of 1 MiB
  int open_item(const fra_decode_item& it, int i) {
    ItemPlan& ip = plan[(size_t)i];
    if (it.frame_offsets) {
      ip.sp.sample_rate = 0;
      ip.sp.channels = it.channels;
      ip.sp.bps = it.bps;
      ip.sp.max_bs = it.blocksize;
      return FRA_OK;
    }
    ip.search = true;
    const uint8_t* d = hdata + it.offset;
    const size_t at = fra_dec::skip_id3(d, (size_t)it.bytes);
    if (at == SIZE_MAX) return fra_internal_set_error(FRA_E_INVALID, "item %d: ID3v2 tag runs past the end of the data", i);
    ip.audio = fra_dec::parse_metadata(d, (size_t)it.bytes, at, ip.sp);
    if (!ip.audio) return fra_internal_set_error(FRA_E_INVALID, "item %d: not a FLAC stream (bad fLaC/STREAMINFO)", i);
    if (ip.sp.channels < 1 || ip.sp.channels > 8 || ip.sp.bps < 4 || ip.sp.bps > 32)
      return fra_internal_set_error(FRA_E_INVALID, "unsupported STREAMINFO (channels %d, bps %d)", ip.sp.channels,
                                    ip.sp.bps);
    for (uint64_t b = ip.audio; b < it.bytes; b += (1u << 20))
      units.push_back({i, d, it.bytes, b, std::min<uint64_t>(it.bytes, b + (1u << 20)), &ip.sp, {}});
    return FRA_OK;
  }

  // the queued search: every candidate of a searched item in its `cand`; true when anything was queued
  bool scan() {
    if (units.empty()) return false;
    fra_dec::scan_units(units);
    for (auto& u : units) {
      auto& c = plan[(size_t)u.item].cand;
      c.insert(c.end(), u.found.begin(), u.found.end());  // units are in byte order
    }
    return true;
  }

  // item i as the kernels see it: its bytes end at `end` of a.data and its tile lies at `at` of the destination;
  // n candidate frames in groups of 64 (a group never spans items), `stride` scratch samples per frame and channel
  void lay_out(int i, size_t n, int stride, uint64_t end, const fra_window& at, double dmin, double span) {
    ItemPlan& ip = plan[(size_t)i];
    bs_max = std::max(bs_max, stride);
    DecItem& di = h_items[(size_t)i];
    di.end = end;
    di.channels = ip.sp.channels;
    di.bps = ip.sp.bps;
    di.sample_rate = ip.sp.sample_rate;
    di.bs_stride = stride;
    di.row_off = at.row_off;
    di.col_off = at.col_off;
    di.width = at.width;
    di.height = at.height;
    di.dmin = dmin;
    di.span = span;
    ip.first_group = (int32_t)h_groups.size();
    ip.n = n;
    for (size_t k = 0; k < n; k += kLanes) {
      h_groups.push_back({scratch_elems, i, (int32_t)std::min<size_t>(kLanes, n - k)});
      scratch_elems += (uint64_t)ip.sp.channels * (uint64_t)stride * kLanes;
    }
  }

  // the slots of the groups laid out: start_of(i, k) is where frame k of item i starts in a.data
  template <typename StartOf>
  int slots(const char* too_many, StartOf&& start_of) {
    ng = h_groups.size();
    if (ng > (size_t)INT32_MAX / kLanes) return fra_internal_set_error(FRA_E_INVALID, "%s", too_many);
    nslots = ng * kLanes;
    h_starts.assign(std::max<size_t>(1, nslots), kNoFrame);
    for (size_t i = 0; i < plan.size(); i++)
      for (size_t k = 0; k < plan[i].n; k++) h_starts[(size_t)plan[i].first_group * kLanes + k] = start_of((int)i, k);
    return FRA_OK;
  }

  // the device side of the tables (and of `clips`, a windowed read's), the job's destination (none: the verify
  // entry) -- device memory as it is; host memory staged, and copied in unless it comes back by_window, so that
  // elements between the windows keep the caller's values either way -- the events, the uploads, cleared failure flags
  int stage(const fra_decode_job* job, int64_t extent, const std::vector<DecClip>* clips) {
    const size_t ni = h_items.size();
    if (const int rc = alloc_tables(sc, a, ni, ng, scratch_elems)) return rc;
    void* d_clips = nullptr;
    if (clips) {
      HIPCHK(sc.alloc(&d_clips, sizeof(DecClip) * ni));
      a.clips = (const DecClip*)d_clips;
    }
    if (job) {
      a.band_stride = job->band_stride;
      a.row_stride = job->row_stride;
      a.col_stride = job->col_stride;
      a.dst_dtype = job->dst_dtype;
      a.denorm = job->denorm;
      dst_bytes = (size_t)extent * (size_t)elem_size(job->dst_dtype);
      by_window = !job->dst_on_device && job->col_stride == 1;
      a.dst = job->dst;
      if (!job->dst_on_device) {
        HIPCHK(sc.alloc(&a.dst, dst_bytes));
        if (dst_bytes && !by_window) HIPCHK(hipMemcpyAsync(a.dst, job->dst, dst_bytes, hipMemcpyHostToDevice, s));
      }
    }
    for (auto& e : ev) HIPCHK(sc.event(&e, hipEventDefault));
    HIPCHK(hipMemcpyAsync((void*)a.items, h_items.data(), sizeof(DecItem) * ni, hipMemcpyHostToDevice, s));
    if (clips) HIPCHK(hipMemcpyAsync(d_clips, clips->data(), sizeof(DecClip) * ni, hipMemcpyHostToDevice, s));
    if (ng) {
      HIPCHK(hipMemcpyAsync((void*)a.groups, h_groups.data(), sizeof(DecGroup) * ng, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync((void*)a.starts, h_starts.data(), sizeof(uint64_t) * nslots, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemsetAsync(a.fail, 0, sizeof(uint32_t) * nslots, s));
    }
    return FRA_OK;
  }

  // k_dec_parse over every slot, the frame table back to the host in h_fout (ev[0], ev[1] around the kernel);
  // synchronises.  h_samp0 is then the entry's chain to fill: the first sample of every chained frame
  int parse_candidates() {
    h_fout.resize(std::max<size_t>(1, nslots));
    HIPCHK(hipEventRecord(ev[0], s));
    if (ng) {
      hipLaunchKernelGGL(k_dec_parse, dim3((unsigned)ng), dim3(kLanes), 0, s, a);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ev[1], s));
    if (ng) HIPCHK(hipMemcpyAsync(h_fout.data(), a.fout, sizeof(FrameOut) * nslots, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    h_samp0.assign(std::max<size_t>(1, nslots), -1);
    return FRA_OK;
  }

  // k_dec_scatter's grid: (group, 64 samples of the largest block)
  dim3 grid() const { return dim3((unsigned)ng, (unsigned)((bs_max + kLanes - 1) / kLanes)); }

  // the chain's first samples to the device, `restore` (an instance of k_dec_restore) over the chained frames, then
  // second(): the kernel that consumes them, over grid() (ev[2..4]), the failure flags back; enqueues only
  template <typename Second>
  int restore_and(void (*restore)(DecArgs), int channels, Second&& second) {
    h_fail.assign(std::max<size_t>(1, nslots), 0);
    if (ng) {
      HIPCHK(hipMemcpyAsync((void*)a.samp0, h_samp0.data(), sizeof(int64_t) * nslots, hipMemcpyHostToDevice, s));
      HIPCHK(hipEventRecord(ev[2], s));
      hipLaunchKernelGGL(restore, dim3((unsigned)ng, (unsigned)channels), dim3(kLanes), 0, s, a);
      HIPCHK(hipGetLastError());
    }
    else HIPCHK(hipEventRecord(ev[2], s));
    HIPCHK(hipEventRecord(ev[3], s));
    if (ng) {
      second();
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ev[4], s));
    if (ng) HIPCHK(hipMemcpyAsync(h_fail.data(), a.fail, sizeof(uint32_t) * nslots, hipMemcpyDeviceToHost, s));
    return FRA_OK;
  }
  template <bool kClip>
  int restore_and_scatter(int channels) {
    void (*const restore)(DecArgs) = k_dec_restore<kClip>;  // (named before k_dec_scatter: the code object's order)
    return restore_and(restore, channels, [&] { hipLaunchKernelGGL(k_dec_scatter<kClip>, grid(), dim3(256), 0, s, a); });
  }

  // the stream waited for; FRA_E_INVALID for the first frame with a failure flag, named by its byte in `bytes`
  int wait_and_check(const uint64_t* bytes) {
    HIPCHK(hipStreamSynchronize(s));
    for (size_t k = 0; k < nslots; k++)
      if (h_fail[k])
        return fra_internal_set_error(FRA_E_INVALID, "frame decode failed: a reconstructed sample leaves the sample range "
                                                     "(frame at byte %llu)", (unsigned long long)bytes[k]);
    return FRA_OK;
  }

  // the end of a decode: a host destination back -- by_window the rectangles of every band, else the whole extent --
  // then wait_and_check, and the kernel times kept on success
  int finish(const fra_decode_job* job, const std::vector<Rect>& rects, const uint64_t* bytes) {
    if (by_window) {
      const size_t es = (size_t)elem_size(job->dst_dtype);
      for (const Rect& r : rects)
        for (int c = 0; c < job->channels; c++) {
          const size_t off = ((size_t)c * (size_t)job->band_stride + (size_t)r.row0 * (size_t)job->row_stride +
                              (size_t)r.col0) * es;
          if (job->row_stride == 0 || r.rows == 1)
            HIPCHK(hipMemcpyAsync((uint8_t*)job->dst + off, (const uint8_t*)a.dst + off, (size_t)r.cols * es,
                                  hipMemcpyDeviceToHost, s));
          else
            HIPCHK(hipMemcpy2DAsync((uint8_t*)job->dst + off, (size_t)job->row_stride * es, (const uint8_t*)a.dst + off,
                                    (size_t)job->row_stride * es, (size_t)r.cols * es, (size_t)r.rows,
                                    hipMemcpyDeviceToHost, s));
        }
    } else if (!job->dst_on_device && dst_bytes) {
      HIPCHK(hipMemcpyAsync(job->dst, a.dst, dst_bytes, hipMemcpyDeviceToHost, s));
    }
    if (const int rc = wait_and_check(bytes)) return rc;
    keep_times(ev);
    return FRA_OK;
  }
};

}  // namespace

extern "C" {

FRA_API int fra_decode_device_timing(float* ms4) {
  if (!ms4) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  memcpy(ms4, g_last_ms, sizeof(g_last_ms));
  return FRA_OK;
}

FRA_API int fra_decode_device(fra_ctx* ctx, const fra_decode_job* job, fra_decoded* infos) {
  if (const int rc = check_job(ctx, job, infos)) return rc;
  const int ni = job->nitems;
  memset(infos, 0, sizeof(fra_decoded) * (size_t)ni);
  if (ni == 0) return FRA_OK;

  std::vector<Range> read;  // what the host reads of the input: all of it when any item is searched
  int64_t extent = 0;       // elements of dst addressed, from element 0
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = job->items[i];
    if (const int rc = check_item(it, i, job->len)) return rc;
    const fra_window& w = it.window;
    if (!it.frame_offsets && read.empty()) read.push_back({0, job->len});
    if (w.height != 0 && w.width > 0)
      extent = std::max<int64_t>(extent, (int64_t)(job->channels - 1) * job->band_stride +
                                             ((int64_t)w.row_off + std::abs(w.height) - 1) * job->row_stride +
                                             ((int64_t)w.col_off + w.width - 1) * job->col_stride + 1);
  }

  Decode c(ctx, ni);
  if (const int rc = c.host_view(job, read)) return rc;
  c.a.data = job->data;  // a host input is uploaded whole, so every entry of h_starts is a byte of job->data
  if (!job->data_on_device) {
    void* p = nullptr;
    HIPCHK(c.sc.alloc(&p, (size_t)job->len));
    if (job->len) HIPCHK(hipMemcpyAsync(p, job->data, (size_t)job->len, hipMemcpyHostToDevice, c.s));
    c.a.data = (const uint8_t*)p;
  }

  // ---- candidates: every frame of the offsets, every sync position of a searched stream
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = job->items[i];
    if (const int rc = c.open_item(it, i)) return rc;
    if (!it.frame_offsets) continue;
    auto& cand = c.plan[(size_t)i].cand;
    cand.reserve((size_t)it.nframes);
    for (int f = 0; f < it.nframes; f++) cand.push_back({it.frame_offsets[f], it.blocksize});
  }
  c.scan();

  // ---- scratch of the largest candidate block size per frame; a capacity window is rows of one sample
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = job->items[i];
    const ItemPlan& ip = c.plan[(size_t)i];
    if (const int rc = check_stream(job, i, ip.sp)) return rc;
    int stride = 1;
    for (const HostCand& k : ip.cand) stride = std::max(stride, k.bs);
    c.lay_out(i, ip.cand.size(), stride, it.offset + it.bytes,
              {it.window.row_off, it.window.col_off, std::abs(it.window.height), it.window.width}, it.data_min,
              it.data_max - it.data_min);
  }
  if (const int rc = c.slots("too many candidate frames",
                             [&](int i, size_t k) { return job->items[i].offset + c.plan[(size_t)i].cand[k].start; }))
    return rc;
  if (const int rc = c.stage(job, extent, nullptr)) return rc;
  if (const int rc = c.parse_candidates()) return rc;

  // ---- chain (item-relative byte positions, the host decoder's wording)
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = job->items[i];
    const ItemPlan& ip = c.plan[(size_t)i];
    const size_t s0 = (size_t)ip.first_group * kLanes;
    uint64_t nsamp = 0;
    int64_t nframes = 0;
    int nstreams = 1;
    if (!ip.search) {
      for (size_t k = 0; k < ip.cand.size(); k++) {
        const FrameOut& fo = c.h_fout[s0 + k];
        if (fo.status == ST_UNSUPPORTED) return fra_internal_set_error(FRA_E_INVALID, "item %d: %s", i, kUnsupported);
        if (fo.status != ST_OK || fo.len != it.frame_offsets[k + 1] - it.frame_offsets[k])
          return fra_internal_set_error(FRA_E_INVALID, "lost sync / corrupt frame at byte %llu",
                                        (unsigned long long)it.frame_offsets[k]);
        c.h_samp0[s0 + k] = (int64_t)nsamp;
        nsamp += (uint64_t)fo.n;
        nframes++;
      }
    } else {
      const fra_dec::ChainResult cr = fra_dec::chain_stream(c.hdata + it.offset, it.bytes, ip.audio, ip.sp,
                                                            (job->flags & FRA_DECODE_CONCAT) != 0, ip.cand,
                                                            c.h_fout.data() + s0, c.h_samp0.data() + s0);
      if (cr.code == fra_dec::CHAIN_UNSUPPORTED) return fra_internal_set_error(FRA_E_INVALID, "item %d: %s", i, kUnsupported);
      if (cr.code == fra_dec::CHAIN_CONCAT_FORMAT)
        return fra_internal_set_error(FRA_E_INVALID, "concatenated stream at byte %llu has a different format",
                                      (unsigned long long)cr.byte);
      if (cr.code == fra_dec::CHAIN_LOST_SYNC)
        return fra_internal_set_error(FRA_E_INVALID, "lost sync / corrupt frame at byte %llu",
                                      (unsigned long long)cr.byte);
      nsamp = cr.nsamp;
      nframes = cr.nframes;
      nstreams = cr.nstreams;
    }
    if (it.window.height < 0) {
      if (nsamp > (uint64_t)(-(int64_t)it.window.height)) {
        infos[i].channels = ip.sp.channels;
        infos[i].bps = ip.sp.bps;
        infos[i].nsamples = nsamp;
        return fra_internal_set_error(FRA_E_SPACE, "item %d: the stream has %llu samples per channel, room for %lld", i,
                                      (unsigned long long)nsamp, -(long long)it.window.height);
      }
    } else if (nsamp != (uint64_t)it.window.height * (uint64_t)it.window.width)
      return fra_internal_set_error(FRA_E_INVALID, "item %d: the stream has %llu samples per channel, its window %d x %d",
                                    i, (unsigned long long)nsamp, it.window.height, it.window.width);
    fill_info(infos[i], ip, nframes, nsamp, nstreams);
  }

  // ---- restore and scatter the chained frames; a host destination with contiguous rows comes back window by window
  if (const int rc = c.restore_and_scatter<false>(job->channels)) return rc;
  std::vector<Rect> rects;
  for (int i = 0; c.by_window && i < ni; i++) {
    const fra_window& w = job->items[i].window;
    const int64_t rows = w.height < 0 ? (int64_t)infos[i].nsamples : w.height;
    if (rows > 0 && w.width > 0) rects.push_back({w.row_off, w.col_off, rows, w.width});
  }
  return c.finish(job, rects, c.h_starts.data());
}

// The windowed read: as fra_decode_device, for the frames that hold samples of `roi` only.  Tables, scratch and
// the uploaded bytes follow the selection: an item outside the region costs nothing, an item inside it costs its
// selected frames (the search path uploads a stream from its first selected candidate to its end, because a
// frame's length is known only after k_dec_parse).
FRA_API int fra_decode_device_window(fra_ctx* ctx, const fra_decode_job* job, const fra_window* roi,
                                     fra_decoded* infos) {
  if (!roi) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (const int rc = check_job(ctx, job, infos)) return rc;
  if (roi->height <= 0 || roi->width <= 0 || roi->row_off < 0 || roi->col_off < 0)
    return fra_internal_set_error(FRA_E_INVALID, "the region of interest needs height > 0, width > 0 and an origin "
                                                 ">= 0 (%d x %d at %d, %d)", roi->height, roi->width, roi->row_off,
                                  roi->col_off);
  if (job->flags & FRA_DECODE_CONCAT)
    return fra_internal_set_error(FRA_E_INVALID, "FRA_DECODE_CONCAT is not supported by the windowed read");
  const int ni = job->nitems;
  memset(infos, 0, sizeof(fra_decoded) * (size_t)ni);
  if (ni == 0) return FRA_OK;

  std::vector<fra_dec::FrameSel> sel((size_t)ni);
  std::vector<Range> read;  // what the host reads of the input: the searched items that the region hits
  int64_t extent = 0;       // elements of dst addressed, from element 0 (= the region's first pixel)
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = job->items[i];
    if (const int rc = check_item(it, i, job->len)) return rc;
    const fra_window& w = it.window;
    if (w.height < 0)
      return fra_internal_set_error(FRA_E_INVALID, "item %d: a capacity window (height < 0) is not supported by the "
                                                   "windowed read", i);
    fra_dec::FrameSel& sl = sel[(size_t)i];
    sl = fra_dec::select_samples(w.row_off, w.col_off, w.height, w.width, roi->row_off, roi->col_off, roi->height,
                                 roi->width);
    if (!sl.hit) continue;
    if (it.frame_offsets) sl.set_blocksize(it.blocksize);
    else read.push_back({it.offset, it.bytes});
    extent = std::max<int64_t>(extent, (int64_t)(job->channels - 1) * job->band_stride +
                                           ((int64_t)sl.rb - 1 - roi->row_off) * job->row_stride +
                                           ((int64_t)sl.cb - 1 - roi->col_off) * job->col_stride + 1);
  }

  Decode c(ctx, ni);
  if (const int rc = c.host_view(job, read)) return rc;

  // ---- candidates of the selected frames
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = job->items[i];
    ItemPlan& ip = c.plan[(size_t)i];
    fra_dec::FrameSel& sl = sel[(size_t)i];
    if (!sl.hit) continue;
    if (const int rc = c.open_item(it, i)) return rc;
    if (it.frame_offsets) {
      if (sl.f_hi >= it.nframes) return fra_internal_set_error(FRA_E_INVALID, "item %d: the stream ends before the window", i);
      // frame f is entry f of the offsets and starts at sample f * blocksize (header numbers are not consulted)
      for (int64_t f = sl.f_lo; f <= sl.f_hi; f++) ip.cand.push_back({it.frame_offsets[f], it.blocksize, 0, (uint64_t)f});
      continue;
    }
    if (ip.sp.min_bs != ip.sp.max_bs || ip.sp.max_bs < 1)
      return fra_internal_set_error(FRA_E_INVALID, "item %d: the windowed read needs a fixed-blocksize stream "
                                                   "(STREAMINFO block sizes %d .. %d)", i, ip.sp.min_bs, ip.sp.max_bs);
    sl.set_blocksize(ip.sp.max_bs);
    if (ip.sp.total_samples && (uint64_t)sl.p_hi > ip.sp.total_samples)
      return fra_internal_set_error(FRA_E_INVALID, "item %d: the stream ends before the window", i);
  }
  std::vector<std::vector<HostCand>> all((size_t)ni);  // search path: every candidate of the stream
  if (c.scan())
    for (int i = 0; i < ni; i++) {
      ItemPlan& ip = c.plan[(size_t)i];
      if (!ip.search) continue;
      all[(size_t)i].swap(ip.cand);
      const auto& found = all[(size_t)i];
      if (!found.empty() && found.front().start == ip.audio && found.front().variable)
        return fra_internal_set_error(FRA_E_INVALID, "item %d: the windowed read needs a fixed-blocksize stream "
                                                     "(variable-blocksize frame header)", i);
      fra_dec::filter_candidates(found, sel[(size_t)i].f_lo, sel[(size_t)i].f_hi, ip.cand);
    }

  // ---- where each item's bytes lie on the device: a host input is uploaded as the spans that hold the selected
  //      frames, one after the other; scratch of the stream's block size per frame; the tile relative to the region
  std::vector<DecClip> h_clips((size_t)ni);
  std::vector<uint64_t> dev_base((size_t)ni, 0), span_a((size_t)ni, 0), span_b((size_t)ni, 0);
  uint64_t upload = 0;
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = job->items[i];
    const ItemPlan& ip = c.plan[(size_t)i];
    const fra_dec::FrameSel& sl = sel[(size_t)i];
    if (!sl.hit) continue;
    if (const int rc = check_stream(job, i, ip.sp)) return rc;
    if (!ip.cand.empty()) {
      span_a[(size_t)i] = ip.cand.front().start;
      span_b[(size_t)i] = ip.search ? it.bytes : it.frame_offsets[sl.f_hi + 1];
    }
    if (job->data_on_device) {
      dev_base[(size_t)i] = it.offset;
      span_b[(size_t)i] = it.bytes;
    } else {
      dev_base[(size_t)i] = upload - span_a[(size_t)i];  // (modulo 2^64; only dev_base + [span_a, span_b) is addressed)
      upload += span_b[(size_t)i] - span_a[(size_t)i];
    }
    c.lay_out(i, ip.cand.size(), ip.sp.max_bs, dev_base[(size_t)i] + span_b[(size_t)i],
              {it.window.row_off - roi->row_off, it.window.col_off - roi->col_off, it.window.height, it.window.width},
              it.data_min, it.data_max - it.data_min);
    h_clips[(size_t)i] = {sl.ra - it.window.row_off, sl.rb - it.window.row_off, sl.ca - it.window.col_off,
                          sl.cb - it.window.col_off, sl.p_lo, sl.p_hi};
  }
  if (const int rc = c.slots("too many candidate frames",
                             [&](int i, size_t k) { return dev_base[(size_t)i] + c.plan[(size_t)i].cand[k].start; }))
    return rc;
  std::vector<uint64_t> h_rel(std::max<size_t>(1, c.nslots), 0);  // item-relative, for messages
  for (int i = 0; i < ni; i++) {
    const ItemPlan& ip = c.plan[(size_t)i];
    for (size_t k = 0; k < ip.cand.size(); k++) h_rel[(size_t)ip.first_group * kLanes + k] = ip.cand[k].start;
  }
  c.a.data = job->data;
  if (!job->data_on_device) {
    void* p = nullptr;
    HIPCHK(c.sc.alloc(&p, (size_t)upload));
    for (int i = 0; i < ni; i++)
      if (span_b[(size_t)i] > span_a[(size_t)i])
        HIPCHK(hipMemcpyAsync((uint8_t*)p + (dev_base[(size_t)i] + span_a[(size_t)i]),
                              job->data + job->items[i].offset + span_a[(size_t)i],
                              (size_t)(span_b[(size_t)i] - span_a[(size_t)i]), hipMemcpyHostToDevice, c.s));
    c.a.data = (const uint8_t*)p;
  }
  if (const int rc = c.stage(job, extent, &h_clips)) return rc;
  if (const int rc = c.parse_candidates()) return rc;

  // ---- the selected frames: CRC-16 (status), byte-contiguous, full blocks, reaching the last needed sample
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = job->items[i];
    const ItemPlan& ip = c.plan[(size_t)i];
    const fra_dec::FrameSel& sl = sel[(size_t)i];
    if (!sl.hit) continue;
    const size_t s0 = (size_t)ip.first_group * kLanes;
    const int64_t bs = ip.sp.max_bs;
    int64_t nframes = 0;
    if (!ip.search) {
      for (size_t k = 0; k < ip.cand.size(); k++) {
        const FrameOut& fo = c.h_fout[s0 + k];
        const int64_t f = sl.f_lo + (int64_t)k;
        if (fo.status == ST_UNSUPPORTED) return fra_internal_set_error(FRA_E_INVALID, "item %d: %s", i, kUnsupported);
        if (fo.status != ST_OK || fo.len != it.frame_offsets[f + 1] - it.frame_offsets[f] ||
            (fo.n != bs && f != it.nframes - 1))
          return fra_internal_set_error(FRA_E_INVALID, "lost sync / corrupt frame at byte %llu",
                                        (unsigned long long)it.frame_offsets[f]);
        c.h_samp0[s0 + k] = f * bs;
        nframes++;
      }
      if (sl.f_hi * bs + c.h_fout[s0 + ip.cand.size() - 1].n < sl.p_hi)
        return fra_internal_set_error(FRA_E_INVALID, "item %d: the stream ends before the window", i);
    } else {
      const fra_dec::ChainResult cr = fra_dec::chain_window(it.bytes, ip.audio, bs, sl, all[(size_t)i], ip.cand,
                                                            c.h_fout.data() + s0, c.h_samp0.data() + s0);
      if (cr.code == fra_dec::CHAIN_UNSUPPORTED) return fra_internal_set_error(FRA_E_INVALID, "item %d: %s", i, kUnsupported);
      if (cr.code == fra_dec::CHAIN_ENDS_EARLY)
        return fra_internal_set_error(FRA_E_INVALID, "item %d: the stream ends before the window", i);
      if (cr.code != fra_dec::CHAIN_OK)
        return fra_internal_set_error(FRA_E_INVALID, "lost sync / corrupt frame at byte %llu",
                                      (unsigned long long)cr.byte);
      nframes = cr.nframes;
    }
    fill_info(infos[i], ip, nframes, (uint64_t)(sl.rb - sl.ra) * (uint64_t)(sl.cb - sl.ca), 1);
  }

  // ---- restore and scatter; a host destination with contiguous rows comes back intersection by intersection
  if (const int rc = c.restore_and_scatter<true>(job->channels)) return rc;
  std::vector<Rect> rects;
  for (int i = 0; c.by_window && i < ni; i++) {
    const fra_dec::FrameSel& sl = sel[(size_t)i];
    if (sl.hit) rects.push_back({sl.ra - roi->row_off, sl.ca - roi->col_off, sl.rb - sl.ra, sl.cb - sl.ca});
  }
  return c.finish(job, rects, h_rel.data());
}

// The verify entry (fra_verify.h): fra_decode_device's offsets path up to k_dec_restore, then k_dec_verify against
// the source raster.  Hidden: fra_plan_verify is the public way in.
int fra_internal_verify_device(fra_ctx* ctx, const uint8_t* data, uint64_t len, const fra_decode_item* items,
                               int32_t nitems, int32_t channels, const fra_verify_source* src,
                               const int32_t* first_frames, fra_verify_report* reports, int32_t* bad_windows) {
  if (!ctx || !src || !reports || !bad_windows || nitems < 0 || (nitems && !items) || (!data && len))
    return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (nitems && (!src->raster || !src->norm_rows)) return fra_internal_set_error(FRA_E_INVALID, "null argument");
  if (src->dtype < FRA_U8 || src->dtype > FRA_F64) return fra_internal_set_error(FRA_E_INVALID, "bad dtype %d", src->dtype);
  if (src->norm != 0 && src->norm != 16 && src->norm != 24)
    return fra_internal_set_error(FRA_E_INVALID, "norm must be 0, 16 or 24");
  if (src->norm == 0 && src->dtype != FRA_I16 && src->dtype != FRA_I32)
    return fra_internal_set_error(FRA_E_INVALID, "norm == 0 needs int16 or int32 samples");
  if (channels < 1 || channels > 8 || src->band_stride < 0 || src->row_stride < 0 || src->col_stride < 0)
    return fra_internal_set_error(FRA_E_INVALID, "bad source layout (channels %d)", channels);
  const int ni = nitems;
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = items[i];
    if (const int rc = check_item(it, i, len)) return rc;
    if (!it.frame_offsets) return fra_internal_set_error(FRA_E_INVALID, "item %d: verify needs frame offsets", i);
    if (it.window.height < 0) return fra_internal_set_error(FRA_E_INVALID, "item %d: bad window", i);
    if (it.channels != channels)
      return fra_internal_set_error(FRA_E_INVALID, "item %d has %d channels, the source %d", i, it.channels, channels);
    const int64_t nsamp = (int64_t)it.window.height * it.window.width;
    const int64_t nfr_all = (nsamp + it.blocksize - 1) / it.blocksize;
    const int64_t first = first_frames ? first_frames[i] : 0;
    if (first < 0 || first > nfr_all || it.nframes > nfr_all - first)
      return fra_internal_set_error(FRA_E_INVALID, "item %d: frames %lld + %d lie past the window's %lld frames", i,
                                    (long long)first, it.nframes, (long long)nfr_all);
    if (!first_frames && it.nframes != nfr_all)
      return fra_internal_set_error(FRA_E_INVALID, "item %d: %d frames, its window %d x %d holds %lld", i, it.nframes,
                                    it.window.height, it.window.width, (long long)nfr_all);
  }
  memset(reports, 0, sizeof(fra_verify_report) * (size_t)ni);
  for (int i = 0; i < ni; i++) reports[i].first_sample = -1;
  *bad_windows = 0;
  if (ni == 0) return FRA_OK;

  // ---- every frame of the offsets, scratch of the item's block size per frame; the source stands where a decode has
  //      its destination
  Decode c(ctx, ni);
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = items[i];
    (void)c.open_item(it, i);  // (the offsets branch: it refuses nothing)
    c.lay_out(i, (size_t)it.nframes, it.blocksize, it.offset + it.bytes, it.window, 0.0, 0.0);
  }
  if (const int rc = c.slots("too many frames",
                             [&](int i, size_t k) { return items[i].offset + items[i].frame_offsets[k]; }))
    return rc;
  c.a.data = data;
  c.a.band_stride = src->band_stride;
  c.a.row_stride = src->row_stride;
  c.a.col_stride = src->col_stride;
  if (const int rc = c.stage(nullptr, 0, nullptr)) return rc;
  VerArgs v{};
  v.src = src->raster;
  v.nd = (const fra::NormDev*)src->norm_rows;
  v.norm = src->norm;
  HIPCHK(c.sc.alloc(&v.res, sizeof(unsigned long long) * 2 * (size_t)ni));
  HIPCHK(c.sc.alloc(&v.vals, sizeof(int32_t) * 2 * (size_t)ni));
  std::vector<unsigned long long> h_res(2 * (size_t)ni);
  for (int i = 0; i < ni; i++) {
    h_res[2 * (size_t)i] = 0;
    h_res[2 * (size_t)i + 1] = ~0ull;
  }
  HIPCHK(hipMemcpyAsync(v.res, h_res.data(), sizeof(unsigned long long) * 2 * (size_t)ni, hipMemcpyHostToDevice, c.s));
  HIPCHK(hipMemsetAsync(v.vals, 0, sizeof(int32_t) * 2 * (size_t)ni, c.s));

  // ---- parse every frame; each must be one, of its offsets' length and of its position's sample count
  if (const int rc = c.parse_candidates()) return rc;
  for (int i = 0; i < ni; i++) {
    const fra_decode_item& it = items[i];
    const size_t g0 = (size_t)c.plan[(size_t)i].first_group * kLanes;
    const int64_t nsamp = (int64_t)it.window.height * it.window.width;
    int64_t at = (int64_t)(first_frames ? first_frames[i] : 0) * it.blocksize;
    for (int f = 0; f < it.nframes; f++) {
      const FrameOut& fo = c.h_fout[g0 + (size_t)f];
      if (fo.status == ST_UNSUPPORTED) return fra_internal_set_error(FRA_E_INVALID, "item %d: %s", i, kUnsupported);
      if (fo.status != ST_OK || fo.len != it.frame_offsets[f + 1] - it.frame_offsets[f] ||
          fo.n != std::min<int64_t>(it.blocksize, nsamp - at))
        return fra_internal_set_error(FRA_E_INVALID, "lost sync / corrupt frame at byte %llu",
                                      (unsigned long long)it.frame_offsets[f]);
      c.h_samp0[g0 + (size_t)f] = at;
      at += fo.n;
    }
    reports[i].nframes = it.nframes;
  }

  // ---- restore, compare
  if (const int rc = c.restore_and(k_dec_restore<false>, channels,
                                   [&] { launch_verify(src->dtype, c.grid(), c.s, c.a, v); }))
    return rc;
  if (c.ng)
    HIPCHK(hipMemcpyAsync(h_res.data(), v.res, sizeof(unsigned long long) * 2 * (size_t)ni, hipMemcpyDeviceToHost, c.s));
  if (const int rc = c.wait_and_check(c.h_starts.data())) return rc;
  int bad = 0;
  for (int i = 0; i < ni; i++) bad += h_res[2 * (size_t)i] != 0;
  if (bad) {  // the rare path: both samples at every bad item's first mismatch
    std::vector<int32_t> h_vals(2 * (size_t)ni);
    v.pass = 1;
    launch_verify(src->dtype, c.grid(), c.s, c.a, v);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_vals.data(), v.vals, sizeof(int32_t) * 2 * (size_t)ni, hipMemcpyDeviceToHost, c.s));
    HIPCHK(hipStreamSynchronize(c.s));
    for (int i = 0; i < ni; i++) {
      if (!h_res[2 * (size_t)i]) continue;
      fra_verify_report& r = reports[i];
      r.mismatches = h_res[2 * (size_t)i];
      r.first_sample = (int64_t)(h_res[2 * (size_t)i + 1] >> 3);
      r.first_channel = (int32_t)(h_res[2 * (size_t)i + 1] & 7);
      r.expected = h_vals[2 * (size_t)i];
      r.got = h_vals[2 * (size_t)i + 1];
    }
  }
  *bad_windows = bad;
  keep_times(c.ev);
  return FRA_OK;
}

}  // extern "C"
