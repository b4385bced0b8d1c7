// fra_frame_header.h -- FLAC frame-header and STREAMINFO parsing shared by the host decoder (fra_decode.cpp)
// and the device decoder (fra_decode_dev.hip: host candidate search and k_dec_parse).  Plain C++, no tables: the
// CRC-8 of the few header bytes is computed bit by bit so the same code runs on the host and in a kernel.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define FRA_HDR_HD __host__ __device__ inline
#else
#define FRA_HDR_HD inline
#endif

namespace fra_dec {

struct StreamParams {
  int sample_rate = 0, channels = 0, bps = 0, min_bs = 0, max_bs = 0;
  uint64_t total_samples = 0;
};

struct FrameHdr {
  int blocksize = 0, sample_rate = 0, chan_assign = 0, channels = 0, bps = 0;
  uint64_t number = 0;  // frame number (fixed) or first sample (variable)
  bool variable = false;
  int hdr_len = 0;
};

FRA_HDR_HD uint32_t crc8_update(uint32_t c, uint32_t byte) {
  c ^= byte;
  for (int b = 0; b < 8; b++) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
  return c;
}

// RFC 9639 9.1; 0 values of sample rate / bps (code 0) take the STREAMINFO ones (sp_rate / sp_bps).
FRA_HDR_HD bool parse_header(const uint8_t* p, const uint8_t* end, int sp_rate, int sp_bps, FrameHdr& h) {
  if (end - p < 6) return false;
  if (p[0] != 0xFF || (p[1] & 0xFE) != 0xF8) return false;
  h.variable = p[1] & 1;
  const int bsc = p[2] >> 4, src = p[2] & 15, ca = p[3] >> 4, bpc = (p[3] >> 1) & 7;
  if ((p[3] & 1) || bsc == 0 || src == 15 || ca > 10 || bpc == 3) return false;
  const uint8_t* q = p + 4;
  // UTF-8-like coded number
  uint64_t v = *q++;
  int extra = 0;
  if (!(v & 0x80)) extra = 0;
  else if ((v & 0xE0) == 0xC0) { v &= 0x1F; extra = 1; }
  else if ((v & 0xF0) == 0xE0) { v &= 0x0F; extra = 2; }
  else if ((v & 0xF8) == 0xF0) { v &= 0x07; extra = 3; }
  else if ((v & 0xFC) == 0xF8) { v &= 0x03; extra = 4; }
  else if ((v & 0xFE) == 0xFC) { v &= 0x01; extra = 5; }
  else if (v == 0xFE) { v = 0; extra = 6; }
  else return false;
  if (!h.variable && extra > 5) return false;
  if (end - q < extra + 1) return false;
  for (int i = 0; i < extra; i++) {
    if ((*q & 0xC0) != 0x80) return false;
    v = (v << 6) | (*q++ & 0x3F);
  }
  h.number = v;
  if (bsc == 1) h.blocksize = 192;
  else if (bsc <= 5) h.blocksize = 576 << (bsc - 2);
  else if (bsc == 6) { if (end - q < 2) return false; h.blocksize = *q++ + 1; }
  else if (bsc == 7) { if (end - q < 3) return false; h.blocksize = ((q[0] << 8) | q[1]) + 1; q += 2; }
  else h.blocksize = 256 << (bsc - 8);
  if (src == 0) h.sample_rate = sp_rate;
  else if (src < 12) {
    switch (src) {
      case 1: h.sample_rate = 88200; break;
      case 2: h.sample_rate = 176400; break;
      case 3: h.sample_rate = 192000; break;
      case 4: h.sample_rate = 8000; break;
      case 5: h.sample_rate = 16000; break;
      case 6: h.sample_rate = 22050; break;
      case 7: h.sample_rate = 24000; break;
      case 8: h.sample_rate = 32000; break;
      case 9: h.sample_rate = 44100; break;
      case 10: h.sample_rate = 48000; break;
      default: h.sample_rate = 96000; break;
    }
  }
  else if (src == 12) { if (end - q < 2) return false; h.sample_rate = *q++ * 1000; }
  else if (src == 13) { if (end - q < 3) return false; h.sample_rate = (q[0] << 8) | q[1]; q += 2; }
  else { if (end - q < 3) return false; h.sample_rate = ((q[0] << 8) | q[1]) * 10; q += 2; }
  switch (bpc) {
    case 0: h.bps = sp_bps; break;
    case 1: h.bps = 8; break;
    case 2: h.bps = 12; break;
    case 4: h.bps = 16; break;
    case 5: h.bps = 20; break;
    case 6: h.bps = 24; break;
    default: h.bps = 32; break;
  }
  if (h.bps < 4 || h.bps > 32) return false;
  h.chan_assign = ca;
  h.channels = ca < 8 ? ca + 1 : 2;
  if (end - q < 1) return false;
  uint32_t c8 = 0;
  for (const uint8_t* r = p; r < q; r++) c8 = crc8_update(c8, *r);
  if (c8 != *q) return false;
  h.hdr_len = (int)(q - p) + 1;
  return true;
}

// ID3v2 prefix (mutagen may leave one): offset of the byte after it, 0 when there is none, SIZE_MAX when the tag
// runs past the end
inline size_t skip_id3(const uint8_t* data, size_t len) {
  if (len >= 10 && memcmp(data, "ID3", 3) == 0) {
    const size_t at = 10 + (((size_t)data[6] & 0x7F) << 21 | ((size_t)data[7] & 0x7F) << 14 |
                            ((size_t)data[8] & 0x7F) << 7 | ((size_t)data[9] & 0x7F));
    return at > len ? SIZE_MAX : at;
  }
  return 0;
}

// "fLaC" + metadata blocks; returns the offset of the first audio byte (0 on error)
inline size_t parse_metadata(const uint8_t* d, size_t len, size_t at, StreamParams& sp) {
  if (at > len || len - at < 8 || memcmp(d + at, "fLaC", 4) != 0) return 0;
  size_t q = at + 4;
  bool have_si = false;
  for (;;) {
    if (len - q < 4) return 0;
    const bool last = d[q] & 0x80;
    const int type = d[q] & 0x7F;
    const size_t bl = ((size_t)d[q + 1] << 16) | ((size_t)d[q + 2] << 8) | d[q + 3];
    q += 4;
    if (len - q < bl) return 0;
    if (type == 0) {
      if (bl < 34) return 0;
      const uint8_t* s = d + q;
      sp.min_bs = (s[0] << 8) | s[1];
      sp.max_bs = (s[2] << 8) | s[3];
      sp.sample_rate = (s[10] << 12) | (s[11] << 4) | (s[12] >> 4);
      sp.channels = ((s[12] >> 1) & 7) + 1;
      sp.bps = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
      sp.total_samples = ((uint64_t)(s[13] & 15) << 32) | ((uint64_t)s[14] << 24) | ((uint64_t)s[15] << 16) |
                         ((uint64_t)s[16] << 8) | s[17];
      have_si = true;
    }
    q += bl;
    if (last) break;
  }
  return have_si ? q : 0;
}

}  // namespace fra_dec
