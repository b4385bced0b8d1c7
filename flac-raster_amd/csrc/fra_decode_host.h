// fra_decode_host.h -- the host-side pieces of the device decoder (fra_decode_dev.hip): the candidate search and
// the frame chain.  Plain C++ without any HIP, so a stand-alone program can run them under host sanitizers
// (tools/decode_host_check.cpp).
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
        out.push_back({q, h.blocksize});
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

enum ChainCode { CHAIN_OK = 0, CHAIN_LOST_SYNC, CHAIN_UNSUPPORTED, CHAIN_CONCAT_FORMAT };
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

}  // namespace fra_dec
