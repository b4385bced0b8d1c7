// fra_decode_host.h -- the host-side pieces of the device decoder (fra_decode_dev.hip): the candidate search, the
// frame chain and, for the windowed read (fra_decode_device_window), the frame-range arithmetic, the candidate
// filter and the local chain.  Plain C++ without any HIP, so a stand-alone program can run them under host
// sanitizers (tools/decode_host_check.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "fra_frame_header.h"

namespace fra_dec {

enum : int32_t { ST_NONE = 0, ST_OK = 1, ST_UNSUPPORTED = 2 };

struct HostCand {
  uint64_t start;  // stream-relative byte
  int32_t bs;      // block size of its header
  int32_t variable = 0;  // its header's blocking-strategy bit
  uint64_t number = 0;   // its header's frame number (first sample when variable)
};

// what k_dec_parse reports per candidate
struct FrameRec {
  uint32_t len;  // bytes, CRC-16 included
  int32_t n;     // samples per channel
  uint8_t status, assign, bps, pad;
};

// every sync position of data[b0, b1) whose header parses (CRC-8) and has the stream's channel count
inline void scan_range(const uint8_t* data, uint64_t len, uint64_t b0, uint64_t b1, const StreamParams& sp,
                       std::vector<HostCand>& out) {
  uint64_t q = b0;
  b1 = std::min(b1, len);
  while (q < b1 && q + 1 < len) {
    const void* hit = memchr(data + q, 0xFF, (size_t)(b1 - q));
    if (!hit) break;
    q = (uint64_t)((const uint8_t*)hit - data);
    if (q + 1 < len && (data[q + 1] & 0xFE) == 0xF8) {
      FrameHdr h;
      if (parse_header(data + q, data + len, sp.sample_rate, sp.bps, h) && h.channels == sp.channels)
        out.push_back({q, h.blocksize, h.variable ? 1 : 0, h.number});
    }
    q++;
  }
}

struct ScanUnit {
  int item;
  const uint8_t* data;  // the stream
  uint64_t len, b0, b1;
  const StreamParams* sp;
  std::vector<HostCand> found;
};

// the units on at most 16 threads (never sized by the machine's core count alone)
inline void scan_units(std::vector<ScanUnit>& units) {
  if (units.empty()) return;
  unsigned nt = std::thread::hardware_concurrency();
  nt = std::max(1u, std::min({nt, 16u, (unsigned)units.size()}));
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (;;) {
      const size_t u = next.fetch_add(1);
      if (u >= units.size()) return;
      ScanUnit& x = units[u];
      scan_range(x.data, x.len, x.b0, x.b1, *x.sp, x.found);
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
}

enum ChainCode { CHAIN_OK = 0, CHAIN_LOST_SYNC, CHAIN_UNSUPPORTED, CHAIN_CONCAT_FORMAT, CHAIN_ENDS_EARLY };
struct ChainResult {
  ChainCode code = CHAIN_OK;
  uint64_t byte = 0;  // stream-relative position of the failure
  uint64_t nsamp = 0;
  int64_t nframes = 0;
  int nstreams = 1;
};

// Follow start -> end from the first audio byte through the candidate table, exactly as fra_decode: a false
// candidate inside a frame is never reached, "fLaC" at a break starts the next stream when `concat`.  samp0[k]
// receives the first sample of chained candidate k (the caller presets -1).
inline ChainResult chain_stream(const uint8_t* d, uint64_t len, uint64_t audio, const StreamParams& sp, bool concat,
                                const std::vector<HostCand>& cand, const FrameRec* rec, int64_t* samp0) {
  ChainResult r;
  uint64_t pos = audio;
  while (pos < len) {
    auto c = std::lower_bound(cand.begin(), cand.end(), pos,
                              [](const HostCand& x, uint64_t v) { return x.start < v; });
    if (c != cand.end() && c->start == pos) {
      const size_t k = (size_t)(c - cand.begin());
      if (rec[k].status == ST_UNSUPPORTED) { r.code = CHAIN_UNSUPPORTED; r.byte = pos; return r; }
      if (rec[k].status == ST_OK && rec[k].len > 0) {
        samp0[k] = (int64_t)r.nsamp;
        r.nsamp += (uint64_t)rec[k].n;
        r.nframes++;
        pos += rec[k].len;
        continue;
      }
    }
    if (concat && len - pos >= 4 && memcmp(d + pos, "fLaC", 4) == 0) {
      StreamParams sp2;
      const size_t a2 = parse_metadata(d, (size_t)len, (size_t)pos, sp2);
      if (!a2 || sp2.channels != sp.channels || sp2.bps != sp.bps) { r.code = CHAIN_CONCAT_FORMAT; r.byte = pos; return r; }
      pos = a2;
      r.nstreams++;
      continue;
    }
    r.code = CHAIN_LOST_SYNC;
    r.byte = pos;
    return r;
  }
  return r;
}

// ------------------------------------------------------------------------------------------ windowed read
// What a region of interest needs of one tile: the tile (r0, c0, H, W) and the region (rr, rc, rh, rw) are in
// raster coordinates.  The needed samples of the tile's stream are [p_lo, p_hi): from the first pixel of the
// intersection's first row to the last pixel of its last row.
struct FrameSel {
  bool hit = false;
  int32_t ra = 0, rb = 0, ca = 0, cb = 0;  // intersection rows [ra, rb) and columns [ca, cb), raster coordinates
  int64_t p_lo = 0, p_hi = 0;
  int64_t f_lo = 0, f_hi = -1;             // needed frames of a fixed-blocksize stream (set_blocksize)
  void set_blocksize(int64_t bs) {
    f_lo = p_lo / bs;
    f_hi = (p_hi - 1) / bs;
  }
};

inline FrameSel select_samples(int32_t r0, int32_t c0, int32_t H, int32_t W, int32_t rr, int32_t rc, int32_t rh,
                               int32_t rw) {
  FrameSel s;
  const int64_t ra = std::max<int64_t>(r0, rr), rb = std::min<int64_t>((int64_t)r0 + H, (int64_t)rr + rh);
  const int64_t ca = std::max<int64_t>(c0, rc), cb = std::min<int64_t>((int64_t)c0 + W, (int64_t)rc + rw);
  if (ra >= rb || ca >= cb) return s;
  s.hit = true;
  s.ra = (int32_t)ra; s.rb = (int32_t)rb; s.ca = (int32_t)ca; s.cb = (int32_t)cb;
  s.p_lo = (ra - r0) * W + (ca - c0);
  s.p_hi = (rb - 1 - r0) * W + (cb - c0);
  return s;
}

// the candidates whose header carries a fixed-blocksize frame number in [f_lo, f_hi], in byte order
inline void filter_candidates(const std::vector<HostCand>& all, int64_t f_lo, int64_t f_hi, std::vector<HostCand>& out) {
  for (const HostCand& c : all)
    if (!c.variable && c.number >= (uint64_t)f_lo && c.number <= (uint64_t)f_hi) out.push_back(c);
}

// The local chain over the filtered candidates `cand` (byte order; rec[k] = what k_dec_parse reports for cand[k]):
// start at the first audio byte when f_lo == 0, otherwise at each candidate numbered f_lo in byte order; a chain is
// valid when every step pos += len lands on a candidate with status OK and the next consecutive number, through
// f_hi.  The first valid chain wins; samp0[k] of its frames receives number * bs (the caller presets -1) and
// nframes their count.  Every frame but the stream's last (the one that ends at `len`) must hold exactly bs
// samples, and the last selected frame must reach p_hi (else CHAIN_ENDS_EARLY).  `all` is the unfiltered list: it
// tells a stream that ends before frame f_lo from one that lost frame f_lo.
inline ChainResult chain_window(uint64_t len, uint64_t audio, int64_t bs, const FrameSel& sel,
                                const std::vector<HostCand>& all, const std::vector<HostCand>& cand,
                                const FrameRec* rec, int64_t* samp0) {
  ChainResult fail;
  fail.code = CHAIN_LOST_SYNC;
  fail.byte = audio;
  int64_t fail_depth = -1;
  std::vector<size_t> chosen;
  for (size_t k0 = 0; k0 < cand.size(); k0++) {
    if (cand[k0].number != (uint64_t)sel.f_lo) continue;
    if (sel.f_lo == 0 && cand[k0].start != audio) continue;
    uint64_t pos = cand[k0].start;
    ChainResult r;
    chosen.clear();
    for (int64_t f = sel.f_lo; f <= sel.f_hi; f++) {
      if (pos >= len) { r.code = CHAIN_ENDS_EARLY; r.byte = pos; break; }
      auto c = std::lower_bound(cand.begin(), cand.end(), pos, [](const HostCand& x, uint64_t v) { return x.start < v; });
      const size_t k = (size_t)(c - cand.begin());
      const bool here = c != cand.end() && c->start == pos && c->number == (uint64_t)f;
      if (here && rec[k].status == ST_UNSUPPORTED) { r.code = CHAIN_UNSUPPORTED; r.byte = pos; return r; }
      if (!here || rec[k].status != ST_OK || rec[k].len == 0 || rec[k].len > len - pos || rec[k].n > bs ||
          (rec[k].n != bs && pos + rec[k].len != len)) {
        r.code = CHAIN_LOST_SYNC;
        r.byte = pos;
        break;
      }
      chosen.push_back(k);
      pos += rec[k].len;
    }
    if (r.code == CHAIN_OK) {
      const size_t kl = chosen.back();
      if ((int64_t)cand[kl].number * bs + rec[kl].n < sel.p_hi) { r.code = CHAIN_ENDS_EARLY; r.byte = pos; }
    }
    if (r.code == CHAIN_OK) {
      for (size_t k : chosen) samp0[k] = (int64_t)cand[k].number * bs;
      r.nframes = (int64_t)chosen.size();
      return r;
    }
    // a chain of good frames that runs into the stream's end is the answer; otherwise keep the deepest failure
    if (r.code == CHAIN_ENDS_EARLY && !chosen.empty()) return r;
    if ((int64_t)chosen.size() > fail_depth) { fail = r; fail_depth = (int64_t)chosen.size(); }
  }
  if (fail_depth < 0 && sel.f_lo > 0) {  // nothing carries the number f_lo
    bool later = false;
    for (const HostCand& c : all) {
      if (c.variable) continue;
      if (c.number >= (uint64_t)sel.f_lo) later = true;
      else if (c.number == (uint64_t)sel.f_lo - 1) fail.byte = c.start;  // (the frame before the lost one)
    }
    if (!later) { fail.code = CHAIN_ENDS_EARLY; fail.byte = len; }
  }
  return fail;
}

}  // namespace fra_dec
