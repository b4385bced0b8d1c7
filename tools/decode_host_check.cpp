// decode_host_check.cpp -- stand-alone check of the host-side pieces of the device decoder, meant to be built with
// host sanitizers (make -C flac-raster_amd/csrc hostcheck) and run without a GPU:
//   * the candidate search (fra_decode_host.h scan_units) and the chain (chain_stream) over the files given on the
//     command line and over corrupted / truncated variants of them; the per-candidate frame lengths that k_dec_parse
//     would report come from the host decoder's own validate-only frame decode, and the chain's verdict and sample
//     count must agree with fra_decode on the same bytes;
//   * the windowed read's frame selection (select_samples / filter_candidates / chain_window): for a few frame
//     ranges of every file (first frame only, a middle range, through the last frame) the selected frames and their
//     first samples must equal what the full chain assigns to the same frames, and a bit-flipped variant must fail
//     exactly when the flipped byte lies in a selected frame;
//   * the argument validation of fra_decode_device, fra_decode_device_window, the verify entry behind
//     fra_plan_verify (fra_internal_verify_device: null arguments, a first frame past the stream), the decimated and resampled reads,
//     their nodata-aware entries (fra_resample.hip: a nodata value the dtype does not admit included),
//     the comparison (fra_compare, fra_decode_device_compare), the statistics (fra_stats, fra_decode_device_stats),
//     the band math (fra_calc, fra_decode_device_calc, and every refusal of its program validator, fra_calc_check),
//     the focal operations (fra_focal, fra_decode_device_focal, and every refusal of their spec validator,
//     fra_focal_check), the zonal statistics (fra_zonal, fra_decode_device_zonal), the warped reads (fra_warp,
//     fra_decode_device_warped, fra_warp_source_window), the polygon rasterizer (fra_rasterize) and the proximity unit
//     (fra_proximity, fra_decode_device_proximity), which return before any GPU work, and the order of these refusals
//     (inputs that break two rules at once);
//   * the proximity unit's reach threshold against the f64 predicate at and around perfect squares, the conversion of
//     its fills and the arithmetic of its launch plan (fra_proximity.h);
//   * the regions unit's refusals in the header's order (fra_regions, fra_decode_device_regions), its FRA_E_SPACE
//     decisions and the arithmetic of its tile, seam and scan plan (fra_regions.h);
//   * the rasterizer's edge table, x-extents and band lists (fra_rasterize.h): closed rings, dropped and oriented
//     edges, an empty band, a feature spanning all bands, a ring with a repeated closing vertex, and that every
//     (edge, row) crossing of the rule is in the row's band list, in the edges' order;
//   * the source-window arithmetic of the warped reads (fra_warp.h source_window): pinned windows, footprints that
//     miss the raster, non-finite grid nodes, and that every tap of every inside pixel lies in the window;
//   * the chunk arithmetic of the row-chunk scan (fra_scan.h plan_chunks): invariants and pinned values.
// usage: decode_host_check [--concat] file.flac ...
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../flac-raster_amd/csrc/fra_decode.cpp"  // the host decoder's frame validation (internal linkage)
#include "../flac-raster_amd/csrc/fra_decode_host.h"
#include "../flac-raster_amd/csrc/fra_scan.h"
#include "../flac-raster_amd/csrc/fra_proximity.h"
#include "../flac-raster_amd/csrc/fra_regions.h"
#include "../flac-raster_amd/csrc/fra_rasterize.h"
#include "../flac-raster_amd/csrc/fra_warp.h"

static std::string g_msg;
extern "C" int fra_internal_set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_msg = buf;
  return code;
}
#ifdef WITH_DEVICE_ENTRY
#include "../flac-raster_amd/csrc/fra_verify.h"
typedef struct ihipStream_t* hipStream_t;
extern "C" void fra_internal_ctx_stream(fra_ctx*, int* device, hipStream_t* stream) { *device = 0; *stream = nullptr; }
#endif

static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// search + chain with host-computed frame records; returns 0 when the chain succeeds
static int search_and_chain(const std::vector<uint8_t>& v, bool concat, uint64_t* nsamp, int64_t* nframes, int* nstreams,
                            uint64_t* bad_byte) {
  const uint8_t* d = v.data();
  const size_t len = v.size();
  const size_t at = fra_dec::skip_id3(d, len);
  if (at == SIZE_MAX) return -1;
  fra_dec::StreamParams sp;
  const size_t audio = fra_dec::parse_metadata(d, len, at, sp);
  if (!audio || sp.channels < 1 || sp.channels > 8 || sp.bps < 4 || sp.bps > 32) return -1;
  std::vector<fra_dec::ScanUnit> units;
  for (uint64_t b = audio; b < len; b += 4096)  // small units: many range seams
    units.push_back({0, d, len, b, std::min<uint64_t>(len, b + 4096), &sp, {}});
  fra_dec::scan_units(units);
  std::vector<fra_dec::HostCand> cand;
  for (auto& u : units) cand.insert(cand.end(), u.found.begin(), u.found.end());
  std::vector<fra_dec::FrameRec> rec(cand.size() + 1);
  Scratch sc;
  for (size_t k = 0; k < cand.size(); k++) {
    FrameHdr h;
    size_t fl = 0;
    if (parse_header(d + cand[k].start, d + len, sp, h)) fl = decode_frame(d + cand[k].start, d + len, sp, h, nullptr, sp.channels, sc);
    rec[k] = {(uint32_t)fl, h.blocksize, (uint8_t)(fl ? fra_dec::ST_OK : fra_dec::ST_NONE), (uint8_t)h.chan_assign, (uint8_t)h.bps, 0};
  }
  std::vector<int64_t> samp0(cand.size() + 1, -1);
  const fra_dec::ChainResult r = fra_dec::chain_stream(d, len, audio, sp, concat, cand, rec.data(), samp0.data());
  *nsamp = r.nsamp; *nframes = r.nframes; *nstreams = r.nstreams; *bad_byte = r.byte;
  return r.code == fra_dec::CHAIN_OK ? 0 : -1;
}

// every candidate of a stream with the frame records the host decoder gives them
struct Scanned {
  fra_dec::StreamParams sp;
  size_t audio = 0;
  std::vector<fra_dec::HostCand> cand;
  std::vector<fra_dec::FrameRec> rec;
};
static bool scan_with_records(const std::vector<uint8_t>& v, Scanned& s) {
  const uint8_t* d = v.data();
  const size_t len = v.size();
  const size_t at = fra_dec::skip_id3(d, len);
  if (at == SIZE_MAX) return false;
  s.audio = fra_dec::parse_metadata(d, len, at, s.sp);
  if (!s.audio || s.sp.channels < 1 || s.sp.channels > 8 || s.sp.bps < 4 || s.sp.bps > 32) return false;
  fra_dec::scan_range(d, len, s.audio, len, s.sp, s.cand);
  s.rec.assign(s.cand.size() + 1, fra_dec::FrameRec{0, 0, 0, 0, 0, 0});
  Scratch sc;
  for (size_t k = 0; k < s.cand.size(); k++) {
    FrameHdr h;
    size_t fl = 0;
    if (parse_header(d + s.cand[k].start, d + len, s.sp, h)) fl = decode_frame(d + s.cand[k].start, d + len, s.sp, h, nullptr, s.sp.channels, sc);
    s.rec[k] = {(uint32_t)fl, h.blocksize, (uint8_t)(fl ? fra_dec::ST_OK : fra_dec::ST_NONE), (uint8_t)h.chan_assign, (uint8_t)h.bps, 0};
  }
  return true;
}

// the local chain of frames [f_lo, f_hi] of `v`; returns the chain's code and fills (start, first sample) pairs
static fra_dec::ChainCode window_chain(const std::vector<uint8_t>& v, int64_t f_lo, int64_t f_hi, int64_t p_hi,
                                       std::vector<std::pair<uint64_t, int64_t>>& got) {
  Scanned s;
  if (!scan_with_records(v, s) || s.sp.min_bs != s.sp.max_bs) return fra_dec::CHAIN_LOST_SYNC;
  fra_dec::FrameSel sel;
  sel.hit = true;
  sel.f_lo = f_lo; sel.f_hi = f_hi;
  sel.p_lo = f_lo * s.sp.max_bs; sel.p_hi = p_hi;
  std::vector<fra_dec::HostCand> kept;
  fra_dec::filter_candidates(s.cand, f_lo, f_hi, kept);
  std::vector<fra_dec::FrameRec> rec(kept.size() + 1);
  for (size_t k = 0, j = 0; k < kept.size(); k++) {  // both lists are in byte order
    while (s.cand[j].start != kept[k].start) j++;
    rec[k] = s.rec[j];
  }
  std::vector<int64_t> samp0(kept.size() + 1, -1);
  const fra_dec::ChainResult r = fra_dec::chain_window(v.size(), s.audio, s.sp.max_bs, sel, s.cand, kept, rec.data(), samp0.data());
  got.clear();
  for (size_t k = 0; k < kept.size(); k++)
    if (samp0[k] >= 0) got.push_back({kept[k].start, samp0[k]});
  if (r.code == fra_dec::CHAIN_OK) EXPECT(r.nframes == (int64_t)got.size(), "chain_window counts %lld frames, marks %zu", (long long)r.nframes, got.size());
  return r.code;
}

static void check_ranges(const char* what, const std::vector<uint8_t>& v) {
  Scanned s;
  if (!scan_with_records(v, s)) { EXPECT(false, "%s: not a stream", what); return; }
  std::vector<int64_t> samp0(s.cand.size() + 1, -1);
  const fra_dec::ChainResult full = fra_dec::chain_stream(v.data(), v.size(), s.audio, s.sp, false, s.cand, s.rec.data(), samp0.data());
  EXPECT(full.code == fra_dec::CHAIN_OK && full.nframes > 0 && s.sp.min_bs == s.sp.max_bs, "%s: no fixed-blocksize chain", what);
  if (g_fail) return;
  struct Fr { uint64_t start, len; int64_t samp0; };
  std::vector<Fr> fr;
  for (size_t k = 0; k < s.cand.size(); k++)
    if (samp0[k] >= 0) fr.push_back({s.cand[k].start, s.rec[k].len, samp0[k]});
  const int64_t F = (int64_t)fr.size(), bs = s.sp.max_bs;
  const int64_t ranges[3][2] = {{0, 0}, {F / 3, std::max(F / 3, 2 * F / 3 - 1)}, {std::max<int64_t>(0, F - 2), F - 1}};
  for (auto& rg : ranges) {
    const int64_t f_lo = rg[0], f_hi = rg[1];
    const int64_t p_hi = std::min<int64_t>((f_hi + 1) * bs, (int64_t)full.nsamp);
    std::vector<std::pair<uint64_t, int64_t>> got;
    const fra_dec::ChainCode code = window_chain(v, f_lo, f_hi, p_hi, got);
    bool same = code == fra_dec::CHAIN_OK && (int64_t)got.size() == f_hi - f_lo + 1;
    for (int64_t f = f_lo; same && f <= f_hi; f++)
      same = got[(size_t)(f - f_lo)].first == fr[(size_t)f].start && got[(size_t)(f - f_lo)].second == fr[(size_t)f].samp0;
    EXPECT(same, "%s: frames %lld..%lld differ from the full chain (code %d)", what, (long long)f_lo, (long long)f_hi, (int)code);
    EXPECT(window_chain(v, f_lo, f_hi, p_hi + 1, got) != fra_dec::CHAIN_OK || p_hi < (int64_t)full.nsamp,
           "%s: a window past the last frame's samples accepted", what);
    // bit flips before, inside and after the range
    const uint64_t a = fr[(size_t)f_lo].start, b = fr[(size_t)f_hi].start + fr[(size_t)f_hi].len;
    const uint64_t flips[] = {s.audio + 9, a > s.audio ? a - 1 : a, a, a + 5, (a + b) / 2, b - 1, b, b + 7, v.size() - 3};
    for (uint64_t pos : flips) {
      if (pos < s.audio || pos >= v.size()) continue;
      std::vector<uint8_t> e(v);
      e[(size_t)pos] ^= 0x04;
      const bool inside = pos >= a && pos < b;
      const bool ok = window_chain(e, f_lo, f_hi, p_hi, got) == fra_dec::CHAIN_OK;
      EXPECT(ok == !inside, "%s: frames %lld..%lld (bytes %llu..%llu), bit flipped at %llu: chain %s", what, (long long)f_lo,
             (long long)f_hi, (unsigned long long)a, (unsigned long long)b, (unsigned long long)pos, ok ? "succeeds" : "fails");
      if (ok) {
        bool eq = (int64_t)got.size() == f_hi - f_lo + 1;
        for (int64_t f = f_lo; eq && f <= f_hi; f++) eq = got[(size_t)(f - f_lo)].first == fr[(size_t)f].start;
        EXPECT(eq, "%s: frames %lld..%lld move under a flip at %llu", what, (long long)f_lo, (long long)f_hi, (unsigned long long)pos);
      }
    }
  }
  printf("%-40s %lld frames, 3 frame ranges checked\n", what, (long long)F);
}

static void check_bytes(const char* what, const std::vector<uint8_t>& v, bool concat) {
  fra_decoded info;
  int32_t* smp = nullptr;
  const int rc = fra_decode(v.data(), v.size(), concat ? FRA_DECODE_CONCAT : 0, &info, &smp);
  const std::string host_msg = g_msg;
  uint64_t nsamp = 0, bad = 0; int64_t nfr = 0; int nst = 0;
  const int rc2 = search_and_chain(v, concat, &nsamp, &nfr, &nst, &bad);
  // (a frame whose samples leave the range passes the host's validation and fails its second pass: not a chain matter)
  const bool host_chain_ok = rc == 0 || host_msg.find("pass 2") != std::string::npos;
  EXPECT((rc2 == 0) == host_chain_ok, "%s: chain verdict %d, host decoder %d (%s)", what, rc2, rc, host_msg.c_str());
  if (rc == 0 && rc2 == 0)
    EXPECT(nsamp == info.nsamples && nfr == info.nframes && nst == info.nstreams, "%s: %llu samples / %lld frames / %d streams, host %llu / %lld / %d",
           what, (unsigned long long)nsamp, (long long)nfr, nst, (unsigned long long)info.nsamples, (long long)info.nframes, info.nstreams);
  if (rc != 0 && rc2 != 0 && host_msg.find("lost sync") != std::string::npos) {
    char want[64];
    snprintf(want, sizeof(want), "at byte %llu", (unsigned long long)bad);
    EXPECT(host_msg.find(want) != std::string::npos, "%s: chain breaks at byte %llu, host says: %s", what, (unsigned long long)bad, host_msg.c_str());
  }
  printf("%-40s host rc %d, chain rc %d, %llu samples\n", what, rc, rc2, (unsigned long long)nsamp);
  free(smp);
}

int main(int argc, char** argv) {
  bool concat = false;
  for (int i = 1; i < argc; i++) {
    if (std::string(argv[i]) == "--concat") { concat = true; continue; }
    FILE* f = fopen(argv[i], "rb");
    if (!f) { printf("cannot open %s\n", argv[i]); return 2; }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    check_bytes(argv[i], v, concat);
    if (concat) check_bytes("  without the concat flag", v, false);
    {  // the windowed read takes one stream: of a concatenated file, the first
      std::vector<uint8_t> one(v);
      uint64_t nsamp = 0, bad = 0; int64_t nfr = 0; int nst = 0;
      if (concat && search_and_chain(v, false, &nsamp, &nfr, &nst, &bad) != 0 && bad < v.size()) one.resize((size_t)bad);
      check_ranges("  frame ranges", one);
    }
    const size_t flips[] = {200, 50000, v.size() - 3, v.size() / 2, v.size() / 3};
    for (size_t pos : flips) {
      if (pos >= v.size()) continue;
      std::vector<uint8_t> e(v);
      e[pos] ^= 0x04;
      char what[64];
      snprintf(what, sizeof(what), "  bit flipped at byte %zu", pos);
      check_bytes(what, e, concat);
    }
    for (size_t cut : {(size_t)100, (size_t)1, v.size() / 2}) {
      if (cut >= v.size()) continue;
      std::vector<uint8_t> e(v.begin(), v.end() - (long)cut);
      char what[64];
      snprintf(what, sizeof(what), "  last %zu bytes cut", cut);
      check_bytes(what, e, concat);
    }
  }
#ifdef WITH_DEVICE_ENTRY
  // argument validation of fra_decode_device: every call returns FRA_E_INVALID before any GPU work
  fra_ctx* ctx = (fra_ctx*)(uintptr_t)16;  // never dereferenced on these paths
  fra_decoded inf[2];
  uint8_t data[64] = {0};
  int32_t dst[64];
  fra_decode_item it{};
  it.offset = 0; it.bytes = 64; it.window = {0, 0, 1, 8};
  fra_decode_job job{};
  job.data = data; job.len = 64; job.items = &it; job.nitems = 1; job.dst = dst; job.dst_dtype = FRA_I32;
  job.channels = 1; job.band_stride = 64; job.row_stride = 8; job.col_stride = 1;
  auto bad = [&](const char* what, fra_decode_job j, fra_decode_item x) {
    j.items = &x;
    EXPECT(fra_decode_device(ctx, &j, inf) == FRA_E_INVALID, "%s accepted", what);
  };
  EXPECT(fra_decode_device(nullptr, &job, inf) == FRA_E_INVALID, "null ctx accepted");
  EXPECT(fra_decode_device(ctx, nullptr, inf) == FRA_E_INVALID, "null job accepted");
  EXPECT(fra_decode_device(ctx, &job, nullptr) == FRA_E_INVALID, "null infos accepted");
  { auto j = job; j.dst = nullptr; bad("null dst", j, it); }
  { auto j = job; j.dst_dtype = 9; bad("dtype 9", j, it); }
  { auto j = job; j.denorm = 3; bad("denorm 3", j, it); }
  { auto j = job; j.dst_dtype = FRA_F32; bad("float dst without denorm", j, it); }
  { auto j = job; j.channels = 9; bad("9 channels", j, it); }
  { auto j = job; j.row_stride = -1; bad("negative stride", j, it); }
  { auto j = job; j.nitems = -1; bad("negative item count", j, it); }
  { auto x = it; x.offset = 60; x.bytes = 8; bad("item past the data", job, x); }
  { auto x = it; x.offset = ~0ull; x.bytes = 2; bad("item offset overflow", job, x); }
  { auto x = it; x.window.row_off = -1; bad("negative window", job, x); }
  { auto x = it; x.window = {0, 0, 65536, 65536}; bad("2^32-sample window", job, x); }
  { auto x = it; x.window = {0, 0, -8, 2}; bad("capacity window wider than 1", job, x); }
  uint64_t fo[3] = {0, 40, 20};
  { auto x = it; x.frame_offsets = fo; x.nframes = 2; x.channels = 1; x.bps = 16; x.blocksize = 16; bad("descending offsets", job, x); }
  fo[2] = 80;
  { auto x = it; x.frame_offsets = fo; x.nframes = 2; x.channels = 1; x.bps = 16; x.blocksize = 16; bad("offsets past the item", job, x); }
  fo[2] = 60;
  { auto x = it; x.frame_offsets = fo; x.nframes = 2; x.channels = 0; x.bps = 16; x.blocksize = 16; bad("0 channels", job, x); }
  { auto j = job; j.nitems = 0; EXPECT(fra_decode_device(ctx, &j, inf) == FRA_OK, "empty job refused"); }
  // ... and of fra_decode_device_window
  const fra_window roi{0, 0, 1, 8};
  auto badw = [&](const char* what, fra_decode_job j, fra_decode_item x, const fra_window* r) {
    j.items = &x;
    EXPECT(fra_decode_device_window(ctx, &j, r, inf) == FRA_E_INVALID, "window read: %s accepted", what);
  };
  badw("null roi", job, it, nullptr);
  EXPECT(fra_decode_device_window(nullptr, &job, &roi, inf) == FRA_E_INVALID, "window read: null ctx accepted");
  { fra_window r = roi; r.height = 0; badw("zero-height roi", job, it, &r); }
  { fra_window r = roi; r.width = 0; badw("zero-width roi", job, it, &r); }
  { fra_window r = roi; r.width = -3; badw("negative-width roi", job, it, &r); }
  { fra_window r = roi; r.row_off = -1; badw("negative roi origin", job, it, &r); }
  { auto j = job; j.flags = FRA_DECODE_CONCAT; badw("FRA_DECODE_CONCAT", j, it, &roi); }
  { auto x = it; x.window = {0, 0, -8, 1}; badw("capacity window", job, x, &roi); }
  { auto j = job; j.dst_dtype = 9; badw("dtype 9", j, it, &roi); }
  { auto x = it; x.offset = 60; x.bytes = 8; x.window = {100, 100, 1, 8}; badw("item past the data, outside the roi", job, x, &roi); }
  { auto j = job; j.nitems = 0; EXPECT(fra_decode_device_window(ctx, &j, &roi, inf) == FRA_OK, "window read: empty job refused"); }
  // the order of the refusals: inputs that break two rules at once, and the message that wins
  {
    auto says = [&](int rc, const char* part) { return rc == FRA_E_INVALID && g_msg.find(part) != std::string::npos; };
    auto x_past = it; x_past.offset = 60; x_past.bytes = 8;
    { auto j = job; j.dst_dtype = 9; j.denorm = 3; EXPECT(says(fra_decode_device(ctx, &j, inf), "bad dst_dtype"), "dtype 9 with denorm 3: %s", g_msg.c_str()); }
    { auto j = job; j.dst_dtype = FRA_F32; j.denorm = FRA_DENORM_NONE; j.channels = 9; EXPECT(says(fra_decode_device(ctx, &j, inf), "FRA_DENORM_NONE needs"), "float dst without denorm with 9 channels: %s", g_msg.c_str()); }
    {
      fra_decode_item two[2] = {x_past, it};
      two[1].window.row_off = -1;
      auto j = job; j.items = two; j.nitems = 2;
      EXPECT(says(fra_decode_device(ctx, &j, inf), "item 0 lies outside the data"), "item 0 past the data with a bad window of item 1: %s", g_msg.c_str());
    }
    { auto j = job; j.dst_dtype = 9; EXPECT(says(fra_decode_device_window(ctx, &j, nullptr, inf), "null argument"), "window read: null roi with dtype 9: %s", g_msg.c_str()); }
    { auto j = job; j.dst_dtype = 9; fra_window r = roi; r.width = 0; EXPECT(says(fra_decode_device_window(ctx, &j, &r, inf), "bad dst_dtype"), "window read: dtype 9 with a zero-width roi: %s", g_msg.c_str()); }
    { auto j = job; j.flags = FRA_DECODE_CONCAT; fra_window r = roi; r.width = 0; EXPECT(says(fra_decode_device_window(ctx, &j, &r, inf), "region of interest"), "window read: zero-width roi with FRA_DECODE_CONCAT: %s", g_msg.c_str()); }
    { auto j = job; j.flags = FRA_DECODE_CONCAT; j.items = &x_past; EXPECT(says(fra_decode_device_window(ctx, &j, &roi, inf), "FRA_DECODE_CONCAT is not supported"), "window read: FRA_DECODE_CONCAT with an item past the data: %s", g_msg.c_str()); }
    { auto x = x_past; x.window = {100, 100, 1, 8}; auto j = job; j.items = &x; EXPECT(says(fra_decode_device_window(ctx, &j, &roi, inf), "item 0 lies outside the data"), "window read: item past the data, outside the roi: %s", g_msg.c_str()); }
  }
  // ... and of the verify entry (fra_plan_verify's driver): an item over frame offsets, a source raster, reports
  {
    uint64_t vo[3] = {0, 30, 64};  // two frames of 16 samples: an 8 x 4 window
    fra_decode_item vi{};
    vi.offset = 0; vi.bytes = 64; vi.window = {0, 0, 8, 4};
    vi.frame_offsets = vo; vi.nframes = 2; vi.channels = 1; vi.bps = 16; vi.blocksize = 16;
    int16_t raster[32] = {0};
    double rows[5] = {0};  // stands in for one device NormDev; never read on these paths
    fra_verify_source vs{};
    vs.raster = raster; vs.dtype = FRA_I16; vs.norm = 16; vs.band_stride = 32; vs.row_stride = 4; vs.col_stride = 1;
    vs.norm_rows = rows;
    fra_verify_report rep[1];
    int32_t nbad = 0, ff = 0;
    auto ver = [&](fra_ctx* c, const uint8_t* d, const fra_decode_item* x, int n, int ch, const fra_verify_source* sr,
                   const int32_t* f0, fra_verify_report* r, int32_t* b) {
      return fra_internal_verify_device(c, d, 64, x, n, ch, sr, f0, r, b);
    };
    EXPECT(ver(nullptr, data, &vi, 1, 1, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: null ctx accepted");
    EXPECT(ver(ctx, nullptr, &vi, 1, 1, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: null data accepted");
    EXPECT(ver(ctx, data, nullptr, 1, 1, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: null items accepted");
    EXPECT(ver(ctx, data, &vi, 1, 1, nullptr, &ff, rep, &nbad) == FRA_E_INVALID, "verify: null source accepted");
    EXPECT(ver(ctx, data, &vi, 1, 1, &vs, &ff, nullptr, &nbad) == FRA_E_INVALID, "verify: null reports accepted");
    EXPECT(ver(ctx, data, &vi, 1, 1, &vs, &ff, rep, nullptr) == FRA_E_INVALID, "verify: null bad_windows accepted");
    { auto s2 = vs; s2.raster = nullptr; EXPECT(ver(ctx, data, &vi, 1, 1, &s2, &ff, rep, &nbad) == FRA_E_INVALID, "verify: null raster accepted"); }
    { auto s2 = vs; s2.norm_rows = nullptr; EXPECT(ver(ctx, data, &vi, 1, 1, &s2, &ff, rep, &nbad) == FRA_E_INVALID, "verify: null norm rows accepted"); }
    { auto s2 = vs; s2.dtype = 8; EXPECT(ver(ctx, data, &vi, 1, 1, &s2, &ff, rep, &nbad) == FRA_E_INVALID, "verify: dtype 8 accepted"); }
    { auto s2 = vs; s2.norm = 8; EXPECT(ver(ctx, data, &vi, 1, 1, &s2, &ff, rep, &nbad) == FRA_E_INVALID, "verify: norm 8 accepted"); }
    { auto s2 = vs; s2.dtype = FRA_U16; s2.norm = 0; EXPECT(ver(ctx, data, &vi, 1, 1, &s2, &ff, rep, &nbad) == FRA_E_INVALID, "verify: norm 0 of uint16 accepted"); }
    { auto s2 = vs; s2.col_stride = -1; EXPECT(ver(ctx, data, &vi, 1, 1, &s2, &ff, rep, &nbad) == FRA_E_INVALID, "verify: negative stride accepted"); }
    EXPECT(ver(ctx, data, &vi, 1, 2, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: channel count unlike the item's accepted");
    EXPECT(ver(ctx, data, &vi, -1, 1, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: negative item count accepted");
    { auto x = vi; x.frame_offsets = nullptr; EXPECT(ver(ctx, data, &x, 1, 1, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: item without frame offsets accepted"); }
    { auto x = vi; x.bytes = 60; EXPECT(ver(ctx, data, &x, 1, 1, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: offsets past the item accepted"); }
    { auto x = vi; x.offset = 8; EXPECT(ver(ctx, data, &x, 1, 1, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: item past the data accepted"); }
    { auto x = vi; x.window = {0, 0, -32, 1}; EXPECT(ver(ctx, data, &x, 1, 1, &vs, &ff, rep, &nbad) == FRA_E_INVALID, "verify: capacity window accepted"); }
    // a per-item first frame: the window has 2 frames, so (1, 2 frames), (2, 1 frame), 3 and -1 lie past the stream
    for (int32_t f0 : {1, 3, -1}) EXPECT(ver(ctx, data, &vi, 1, 1, &vs, &f0, rep, &nbad) == FRA_E_INVALID, "verify: first frame %d accepted", f0);
    { auto x = vi; x.nframes = 1; x.bytes = 30; int32_t f0 = 2; EXPECT(ver(ctx, data, &x, 1, 1, &vs, &f0, rep, &nbad) == FRA_E_INVALID, "verify: one frame from frame 2 of 2 accepted"); }
    { auto x = vi; x.nframes = 1; x.bytes = 30; EXPECT(ver(ctx, data, &x, 1, 1, &vs, nullptr, rep, &nbad) == FRA_E_INVALID, "verify: 1 of 2 frames without a first frame accepted"); }
    // two rules broken at once: the message that wins
    { auto s2 = vs; s2.dtype = 8; s2.norm = 8; EXPECT(ver(ctx, data, &vi, 1, 1, &s2, &ff, rep, &nbad) == FRA_E_INVALID && g_msg.find("bad dtype") != std::string::npos, "verify: dtype 8 with norm 8: %s", g_msg.c_str()); }
    { auto x = vi; x.frame_offsets = nullptr; EXPECT(ver(ctx, data, &x, 1, 2, &vs, &ff, rep, &nbad) == FRA_E_INVALID && g_msg.find("verify needs frame offsets") != std::string::npos, "verify: no frame offsets with a channel mismatch: %s", g_msg.c_str()); }
    nbad = 7;
    EXPECT(ver(ctx, data, &vi, 0, 1, &vs, &ff, rep, &nbad) == FRA_OK && nbad == 0, "verify: empty job refused");
  }
  // ... and of the decimated reads (fra_decimate.hip): refused before any GPU work
  {
    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;
    dj.items = &di;
    const fra_window r48{0, 0, 4, 8};
    auto dec = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, int k, int mode, fra_decoded* o) {
      return fra_decode_device_decimated(c, j, r, k, mode, o);
    };
    EXPECT(dec(nullptr, &dj, &r48, 2, 1, inf) == FRA_E_INVALID, "decimated read: null ctx accepted");
    EXPECT(dec(ctx, nullptr, &r48, 2, 1, inf) == FRA_E_INVALID, "decimated read: null job accepted");
    EXPECT(dec(ctx, &dj, nullptr, 2, 1, inf) == FRA_E_INVALID, "decimated read: null roi accepted");
    EXPECT(dec(ctx, &dj, &r48, 2, 1, nullptr) == FRA_E_INVALID, "decimated read: null infos accepted");
    for (int k : {0, 1, 3, 128, -2}) EXPECT(dec(ctx, &dj, &r48, k, 1, inf) == FRA_E_INVALID, "decimated read: factor %d accepted", k);
    for (int m : {2, -1}) EXPECT(dec(ctx, &dj, &r48, 2, m, inf) == FRA_E_INVALID, "decimated read: resampling %d accepted", m);
    { fra_window r = r48; r.height = 5; EXPECT(dec(ctx, &dj, &r, 2, 1, inf) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "decimated read: uncovered row accepted"); }
    { auto x = di; x.window.width = 7; auto j = dj; j.items = &x; EXPECT(dec(ctx, &j, &r48, 2, 1, inf) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "decimated read: uncovered column accepted"); }
    { auto j = dj; j.nitems = 0; EXPECT(dec(ctx, &j, &r48, 2, 1, inf) == FRA_E_INVALID, "decimated read: empty job accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(dec(ctx, &dj, &r, 2, 1, inf) == FRA_E_INVALID && g_msg.find("region of interest") != std::string::npos, "decimated read: zero-width roi accepted"); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(dec(ctx, &j, &r48, 2, 1, inf) == FRA_E_INVALID, "decimated read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.dst = nullptr; EXPECT(dec(ctx, &j, &r48, 2, 1, inf) == FRA_E_INVALID, "decimated read: null dst accepted"); }
    { auto j = dj; j.dst_dtype = 9; EXPECT(dec(ctx, &j, &r48, 2, 1, inf) == FRA_E_INVALID, "decimated read: dtype 9 accepted"); }
    { auto x = di; x.window = {0, 0, -8, 1}; auto j = dj; j.items = &x; EXPECT(dec(ctx, &j, &r48, 2, 1, inf) == FRA_E_INVALID, "decimated read: capacity window accepted"); }
    int32_t out[16];
    fra_decimate_job mj{};
    mj.src = dst; mj.dtype = FRA_I32; mj.channels = 1; mj.height = 8; mj.width = 8;
    mj.src_band_stride = 64; mj.src_row_stride = 8; mj.src_col_stride = 1;
    mj.factor = 2; mj.resampling = FRA_RESAMPLE_AVERAGE;
    mj.dst = out; mj.dst_band_stride = 16; mj.dst_row_stride = 4; mj.dst_col_stride = 1;
    EXPECT(fra_decimate(nullptr, &mj) == FRA_E_INVALID, "decimate: null ctx accepted");
    EXPECT(fra_decimate(ctx, nullptr) == FRA_E_INVALID, "decimate: null job accepted");
    { auto j = mj; j.src = nullptr; EXPECT(fra_decimate(ctx, &j) == FRA_E_INVALID, "decimate: null src accepted"); }
    { auto j = mj; j.dst = nullptr; EXPECT(fra_decimate(ctx, &j) == FRA_E_INVALID, "decimate: null dst accepted"); }
    for (int k : {0, 1, 3, 128}) { auto j = mj; j.factor = k; EXPECT(fra_decimate(ctx, &j) == FRA_E_INVALID, "decimate: factor %d accepted", k); }
    { auto j = mj; j.resampling = 2; EXPECT(fra_decimate(ctx, &j) == FRA_E_INVALID, "decimate: resampling 2 accepted"); }
    { auto j = mj; j.dtype = 8; EXPECT(fra_decimate(ctx, &j) == FRA_E_INVALID, "decimate: dtype 8 accepted"); }
    { auto j = mj; j.height = 0; EXPECT(fra_decimate(ctx, &j) == FRA_E_INVALID, "decimate: zero height accepted"); }
    { auto j = mj; j.dst_row_stride = -1; EXPECT(fra_decimate(ctx, &j) == FRA_E_INVALID, "decimate: negative stride accepted"); }
    EXPECT(fra_decimate_timing(nullptr) == FRA_E_INVALID, "decimate timing: null accepted");
  }
  // ... and of the resampled reads (fra_resample.hip): refused before any GPU work
  {
    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;
    dj.items = &di;
    const fra_window r48{0, 0, 4, 8};
    auto rs = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, int oh, int ow, int mode, fra_decoded* o) {
      return fra_decode_device_resampled(c, j, r, oh, ow, mode, o);
    };
    EXPECT(rs(nullptr, &dj, &r48, 3, 5, 1, inf) == FRA_E_INVALID, "resampled read: null ctx accepted");
    EXPECT(rs(ctx, nullptr, &r48, 3, 5, 1, inf) == FRA_E_INVALID, "resampled read: null job accepted");
    EXPECT(rs(ctx, &dj, nullptr, 3, 5, 1, inf) == FRA_E_INVALID, "resampled read: null roi accepted");
    EXPECT(rs(ctx, &dj, &r48, 3, 5, 1, nullptr) == FRA_E_INVALID, "resampled read: null infos accepted");
    for (int n : {0, -1, 65537}) {
      EXPECT(rs(ctx, &dj, &r48, n, 5, 1, inf) == FRA_E_INVALID && g_msg.find("output size") != std::string::npos, "resampled read: out height %d accepted", n);
      EXPECT(rs(ctx, &dj, &r48, 3, n, 1, inf) == FRA_E_INVALID && g_msg.find("output size") != std::string::npos, "resampled read: out width %d accepted", n);
    }
    for (int m : {4, -1}) EXPECT(rs(ctx, &dj, &r48, 3, 5, m, inf) == FRA_E_INVALID && g_msg.find("resampling") != std::string::npos, "resampled read: resampling %d accepted", m);
    for (int m : {0, 1, 2, 3}) { fra_window r = r48; r.height = 5; EXPECT(rs(ctx, &dj, &r, 3, 5, m, inf) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "resampled read: uncovered row accepted (mode %d)", m); }
    { auto x = di; x.window.width = 7; auto j = dj; j.items = &x; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "resampled read: uncovered column accepted"); }
    { auto j = dj; j.nitems = 0; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf) == FRA_E_INVALID, "resampled read: empty job accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(rs(ctx, &dj, &r, 3, 5, 1, inf) == FRA_E_INVALID && g_msg.find("region of interest") != std::string::npos, "resampled read: zero-width roi accepted"); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf) == FRA_E_INVALID, "resampled read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.dst = nullptr; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf) == FRA_E_INVALID, "resampled read: null dst accepted"); }
    { auto j = dj; j.dst_dtype = 9; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf) == FRA_E_INVALID, "resampled read: dtype 9 accepted"); }
    int32_t out[16];
    fra_resample_job mj{};
    mj.src = dst; mj.dtype = FRA_I32; mj.channels = 1; mj.height = 8; mj.width = 8;
    mj.src_band_stride = 64; mj.src_row_stride = 8; mj.src_col_stride = 1;
    mj.out_height = 3; mj.out_width = 5; mj.resampling = FRA_RESAMPLE_AVERAGE;
    mj.dst = out; mj.dst_band_stride = 15; mj.dst_row_stride = 5; mj.dst_col_stride = 1;
    EXPECT(fra_resample(nullptr, &mj) == FRA_E_INVALID, "resample: null ctx accepted");
    EXPECT(fra_resample(ctx, nullptr) == FRA_E_INVALID, "resample: null job accepted");
    { auto j = mj; j.src = nullptr; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID, "resample: null src accepted"); }
    { auto j = mj; j.dst = nullptr; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID, "resample: null dst accepted"); }
    for (int n : {0, -1, 65537}) {
      { auto j = mj; j.out_height = n; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID, "resample: out height %d accepted", n); }
      { auto j = mj; j.out_width = n; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID, "resample: out width %d accepted", n); }
    }
    for (int m : {4, -1}) { auto j = mj; j.resampling = m; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID, "resample: resampling %d accepted", m); }
    { auto j = mj; j.dtype = 8; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID, "resample: dtype 8 accepted"); }
    { auto j = mj; j.height = 0; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID, "resample: zero height accepted"); }
    { auto j = mj; j.dst_row_stride = -1; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID, "resample: negative stride accepted"); }
    // the overflow bounds of the average: n = h' w'; n 2^(8 itemsize) > 2^63 (integers), n > 2^53 (floats)
    { auto j = mj; j.height = 65537; j.width = 65537; j.out_height = 1; j.out_width = 1; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID && g_msg.find("average") != std::string::npos, "resample: int32 average of 2^32 weights accepted"); }
    { auto j = mj; j.dtype = FRA_U8; j.height = (1 << 28) + 1; j.width = (1 << 27) + 1; j.out_height = 2; j.out_width = 2; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID && g_msg.find("average") != std::string::npos, "resample: uint8 average of 2^55 weights accepted"); }
    { auto j = mj; j.dtype = FRA_F64; j.height = (1 << 27) + 1; j.width = (1 << 26) + 1; j.out_height = 2; j.out_width = 2; EXPECT(fra_resample(ctx, &j) == FRA_E_INVALID && g_msg.find("average") != std::string::npos, "resample: f64 average of 2^53 weights accepted"); }
    EXPECT(fra_resample_timing(nullptr) == FRA_E_INVALID, "resample timing: null accepted");
  }
  // ... and of the nodata-aware reads (fra_resample.hip): the unmasked refusals, and a nodata value the dtype
  // does not admit, before any GPU work
  {
    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;  // dst_dtype int32
    dj.items = &di;
    const fra_window r48{0, 0, 4, 8};
    const double qnan = std::nan(""), inf_v = HUGE_VAL;
    uint64_t filled[8];
    auto bad_nodata = [&](int rc) { return rc == FRA_E_INVALID && g_msg.find("nodata") != std::string::npos; };
    auto rs = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, int oh, int ow, int mode, fra_decoded* o, double nd) {
      return fra_decode_device_resampled_masked(c, j, r, oh, ow, mode, o, nd, filled);
    };
    EXPECT(rs(nullptr, &dj, &r48, 3, 5, 1, inf, 0.0) == FRA_E_INVALID, "masked resampled read: null ctx accepted");
    EXPECT(rs(ctx, nullptr, &r48, 3, 5, 1, inf, 0.0) == FRA_E_INVALID, "masked resampled read: null job accepted");
    EXPECT(rs(ctx, &dj, nullptr, 3, 5, 1, inf, 0.0) == FRA_E_INVALID, "masked resampled read: null roi accepted");
    EXPECT(rs(ctx, &dj, &r48, 3, 5, 1, nullptr, 0.0) == FRA_E_INVALID, "masked resampled read: null infos accepted");
    for (int n : {0, -1, 65537}) {
      EXPECT(rs(ctx, &dj, &r48, n, 5, 1, inf, 0.0) == FRA_E_INVALID && g_msg.find("output size") != std::string::npos, "masked resampled read: out height %d accepted", n);
      EXPECT(rs(ctx, &dj, &r48, 3, n, 1, inf, 0.0) == FRA_E_INVALID && g_msg.find("output size") != std::string::npos, "masked resampled read: out width %d accepted", n);
    }
    for (int m : {4, -1}) EXPECT(rs(ctx, &dj, &r48, 3, 5, m, inf, 0.0) == FRA_E_INVALID && g_msg.find("resampling") != std::string::npos, "masked resampled read: resampling %d accepted", m);
    for (double nd : {0.5, 2147483648.0, -2147483649.0, qnan, inf_v, -inf_v})
      for (int m : {0, 1, 2, 3}) EXPECT(bad_nodata(rs(ctx, &dj, &r48, 3, 5, m, inf, nd)), "masked resampled read: nodata %g of int32 accepted (mode %d)", nd, m);
    for (int m : {0, 1, 2, 3}) { fra_window r = r48; r.height = 5; EXPECT(rs(ctx, &dj, &r, 3, 5, m, inf, 0.0) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "masked resampled read: uncovered row accepted (mode %d)", m); }
    { auto x = di; x.window.width = 7; auto j = dj; j.items = &x; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf, 0.0) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "masked resampled read: uncovered column accepted"); }
    { auto j = dj; j.nitems = 0; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf, 0.0) == FRA_E_INVALID, "masked resampled read: empty job accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(rs(ctx, &dj, &r, 3, 5, 1, inf, 0.0) == FRA_E_INVALID && g_msg.find("region of interest") != std::string::npos, "masked resampled read: zero-width roi accepted"); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf, 0.0) == FRA_E_INVALID, "masked resampled read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.dst = nullptr; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf, 0.0) == FRA_E_INVALID, "masked resampled read: null dst accepted"); }
    { auto j = dj; j.dst_dtype = 9; EXPECT(rs(ctx, &j, &r48, 3, 5, 1, inf, 0.0) == FRA_E_INVALID, "masked resampled read: dtype 9 accepted"); }
    auto dec = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, int k, int mode, fra_decoded* o, double nd) {
      return fra_decode_device_decimated_masked(c, j, r, k, mode, o, nd, filled);
    };
    EXPECT(dec(nullptr, &dj, &r48, 2, 1, inf, 0.0) == FRA_E_INVALID, "masked decimated read: null ctx accepted");
    EXPECT(dec(ctx, nullptr, &r48, 2, 1, inf, 0.0) == FRA_E_INVALID, "masked decimated read: null job accepted");
    EXPECT(dec(ctx, &dj, nullptr, 2, 1, inf, 0.0) == FRA_E_INVALID, "masked decimated read: null roi accepted");
    EXPECT(dec(ctx, &dj, &r48, 2, 1, nullptr, 0.0) == FRA_E_INVALID, "masked decimated read: null infos accepted");
    for (int k : {0, 1, 3, 128, -2}) EXPECT(dec(ctx, &dj, &r48, k, 1, inf, 0.0) == FRA_E_INVALID, "masked decimated read: factor %d accepted", k);
    for (int m : {2, -1}) EXPECT(dec(ctx, &dj, &r48, 2, m, inf, 0.0) == FRA_E_INVALID, "masked decimated read: resampling %d accepted", m);
    for (double nd : {0.5, 2147483648.0, qnan, inf_v}) EXPECT(bad_nodata(dec(ctx, &dj, &r48, 2, 1, inf, nd)), "masked decimated read: nodata %g of int32 accepted", nd);
    { fra_window r = r48; r.height = 5; EXPECT(dec(ctx, &dj, &r, 2, 1, inf, 0.0) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "masked decimated read: uncovered row accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(dec(ctx, &dj, &r, 2, 1, inf, 0.0) == FRA_E_INVALID && g_msg.find("region of interest") != std::string::npos, "masked decimated read: zero-width roi accepted"); }
    { auto j = dj; j.dst = nullptr; EXPECT(dec(ctx, &j, &r48, 2, 1, inf, 0.0) == FRA_E_INVALID, "masked decimated read: null dst accepted"); }
    { auto x = di; x.window = {0, 0, -8, 1}; auto j = dj; j.items = &x; EXPECT(dec(ctx, &j, &r48, 2, 1, inf, 0.0) == FRA_E_INVALID, "masked decimated read: capacity window accepted"); }
    int32_t out[16];
    fra_resample_job mj{};
    mj.src = dst; mj.dtype = FRA_I32; mj.channels = 1; mj.height = 8; mj.width = 8;
    mj.src_band_stride = 64; mj.src_row_stride = 8; mj.src_col_stride = 1;
    mj.out_height = 3; mj.out_width = 5; mj.resampling = FRA_RESAMPLE_AVERAGE;
    mj.dst = out; mj.dst_band_stride = 15; mj.dst_row_stride = 5; mj.dst_col_stride = 1;
    EXPECT(fra_resample_masked(nullptr, &mj, 0.0, filled) == FRA_E_INVALID, "masked resample: null ctx accepted");
    EXPECT(fra_resample_masked(ctx, nullptr, 0.0, filled) == FRA_E_INVALID, "masked resample: null job accepted");
    { auto j = mj; j.src = nullptr; EXPECT(fra_resample_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked resample: null src accepted"); }
    { auto j = mj; j.dst = nullptr; EXPECT(fra_resample_masked(ctx, &j, 0.0, nullptr) == FRA_E_INVALID, "masked resample: null dst accepted"); }
    for (int n : {0, -1, 65537}) { auto j = mj; j.out_height = n; EXPECT(fra_resample_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked resample: out height %d accepted", n); }
    for (int m : {4, -1}) { auto j = mj; j.resampling = m; EXPECT(fra_resample_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked resample: resampling %d accepted", m); }
    { auto j = mj; j.dtype = 8; EXPECT(fra_resample_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked resample: dtype 8 accepted"); }
    { auto j = mj; j.height = 0; EXPECT(fra_resample_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked resample: zero height accepted"); }
    { auto j = mj; j.dst_row_stride = -1; EXPECT(fra_resample_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked resample: negative stride accepted"); }
    { auto j = mj; j.height = 65537; j.width = 65537; j.out_height = 1; j.out_width = 1; EXPECT(fra_resample_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID && g_msg.find("average") != std::string::npos, "masked resample: int32 average of 2^32 weights accepted"); }
    // a nodata value per dtype: outside the range, fractional, inexact in f32, infinite; NaN for an integer dtype
    struct { int dtype; double nd; } bad[] = {
        {FRA_U8, 256.0}, {FRA_U8, -1.0}, {FRA_I8, 128.0}, {FRA_I8, -129.0}, {FRA_U16, 65536.0}, {FRA_I16, -32769.0},
        {FRA_U32, 4294967296.0}, {FRA_I32, 2147483648.0}, {FRA_U16, 0.5}, {FRA_I32, qnan}, {FRA_U8, inf_v},
        {FRA_F32, 0.1}, {FRA_F32, 16777217.0}, {FRA_F32, 1e300}, {FRA_F32, inf_v}, {FRA_F64, -inf_v}};
    for (const auto& c : bad) {
      auto j = mj; j.dtype = c.dtype;
      EXPECT(bad_nodata(fra_resample_masked(ctx, &j, c.nd, filled)), "masked resample: nodata %g of dtype %d accepted", c.nd, c.dtype);
      fra_decimate_job k{};
      k.src = dst; k.dtype = c.dtype; k.channels = 1; k.height = 8; k.width = 8;
      k.src_band_stride = 64; k.src_row_stride = 8; k.src_col_stride = 1;
      k.factor = 2; k.resampling = FRA_RESAMPLE_AVERAGE;
      k.dst = out; k.dst_band_stride = 16; k.dst_row_stride = 4; k.dst_col_stride = 1;
      EXPECT(bad_nodata(fra_decimate_masked(ctx, &k, c.nd, nullptr)), "masked decimate: nodata %g of dtype %d accepted", c.nd, c.dtype);
    }
    fra_decimate_job kj{};
    kj.src = dst; kj.dtype = FRA_I32; kj.channels = 1; kj.height = 8; kj.width = 8;
    kj.src_band_stride = 64; kj.src_row_stride = 8; kj.src_col_stride = 1;
    kj.factor = 2; kj.resampling = FRA_RESAMPLE_AVERAGE;
    kj.dst = out; kj.dst_band_stride = 16; kj.dst_row_stride = 4; kj.dst_col_stride = 1;
    EXPECT(fra_decimate_masked(nullptr, &kj, 0.0, filled) == FRA_E_INVALID, "masked decimate: null ctx accepted");
    EXPECT(fra_decimate_masked(ctx, nullptr, 0.0, filled) == FRA_E_INVALID, "masked decimate: null job accepted");
    { auto j = kj; j.src = nullptr; EXPECT(fra_decimate_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked decimate: null src accepted"); }
    for (int k : {0, 1, 3, 128}) { auto j = kj; j.factor = k; EXPECT(fra_decimate_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked decimate: factor %d accepted", k); }
    { auto j = kj; j.resampling = 2; EXPECT(fra_decimate_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked decimate: resampling 2 accepted"); }
    { auto j = kj; j.dtype = 8; EXPECT(fra_decimate_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked decimate: dtype 8 accepted"); }
    { auto j = kj; j.height = 0; EXPECT(fra_decimate_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked decimate: zero height accepted"); }
    { auto j = kj; j.dst_row_stride = -1; EXPECT(fra_decimate_masked(ctx, &j, 0.0, filled) == FRA_E_INVALID, "masked decimate: negative stride accepted"); }
    EXPECT(fra_resample_masked_timing(nullptr) == FRA_E_INVALID, "masked resample timing: null accepted");
  }
  // ... and of the comparison (fra_compare.hip): refused before any GPU work
  {
    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;
    dj.items = &di;
    dj.dst = nullptr;  // ignored by the compared read, as are the job's strides
    dj.band_stride = dj.row_stride = dj.col_stride = -1;
    const fra_window r48{0, 0, 4, 8};
    static int32_t ref[64];
    fra_compare_band bands[1];
    auto cmp = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, const void* rf, int64_t bs, int64_t rs,
                   int64_t cs, fra_compare_band* b, fra_decoded* o) {
      return fra_decode_device_compare(c, j, r, rf, 0, bs, rs, cs, b, o);
    };
    EXPECT(cmp(nullptr, &dj, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: null ctx accepted");
    EXPECT(cmp(ctx, nullptr, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: null job accepted");
    EXPECT(cmp(ctx, &dj, nullptr, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: null roi accepted");
    EXPECT(cmp(ctx, &dj, &r48, nullptr, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: null ref accepted");
    EXPECT(cmp(ctx, &dj, &r48, ref, 32, 8, 1, nullptr, inf) == FRA_E_INVALID, "compared read: null bands accepted");
    EXPECT(cmp(ctx, &dj, &r48, ref, 32, 8, 1, bands, nullptr) == FRA_E_INVALID, "compared read: null infos accepted");
    EXPECT(cmp(ctx, &dj, &r48, ref, -1, 8, 1, bands, inf) == FRA_E_INVALID && g_msg.find("layout") != std::string::npos, "compared read: negative band stride accepted");
    EXPECT(cmp(ctx, &dj, &r48, ref, 32, -8, 1, bands, inf) == FRA_E_INVALID, "compared read: negative row stride accepted");
    EXPECT(cmp(ctx, &dj, &r48, ref, 32, 8, -1, bands, inf) == FRA_E_INVALID, "compared read: negative column stride accepted");
    { fra_window r = r48; r.height = 5; EXPECT(cmp(ctx, &dj, &r, ref, 40, 8, 1, bands, inf) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "compared read: uncovered row accepted"); }
    { auto x = di; x.window.width = 7; auto j = dj; j.items = &x; EXPECT(cmp(ctx, &j, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "compared read: uncovered column accepted"); }
    { auto j = dj; j.nitems = 0; EXPECT(cmp(ctx, &j, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: empty job accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(cmp(ctx, &dj, &r, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID && g_msg.find("region of interest") != std::string::npos, "compared read: zero-width roi accepted"); }
    { fra_window r{0, 0, 65537, 65536}; EXPECT(cmp(ctx, &dj, &r, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID && g_msg.find("2^32 pixels") != std::string::npos, "compared read: more than 2^32 pixels accepted"); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(cmp(ctx, &j, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.dst_dtype = 9; EXPECT(cmp(ctx, &j, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID && g_msg.find("dtype") != std::string::npos, "compared read: dtype 9 accepted"); }
    { auto j = dj; j.denorm = 7; EXPECT(cmp(ctx, &j, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: denorm 7 accepted"); }
    { auto j = dj; j.channels = 0; EXPECT(cmp(ctx, &j, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: no channels accepted"); }
    { auto x = di; x.window = {0, 0, -8, 1}; auto j = dj; j.items = &x; EXPECT(cmp(ctx, &j, &r48, ref, 32, 8, 1, bands, inf) == FRA_E_INVALID, "compared read: capacity window accepted"); }
    fra_compare_job cj{};
    cj.a = dst; cj.b = ref; cj.dtype = FRA_I32; cj.channels = 1; cj.height = 8; cj.width = 8;
    cj.a_band_stride = cj.b_band_stride = 64; cj.a_row_stride = cj.b_row_stride = 8; cj.a_col_stride = cj.b_col_stride = 1;
    EXPECT(fra_compare(nullptr, &cj, bands) == FRA_E_INVALID, "compare: null ctx accepted");
    EXPECT(fra_compare(ctx, nullptr, bands) == FRA_E_INVALID, "compare: null job accepted");
    EXPECT(fra_compare(ctx, &cj, nullptr) == FRA_E_INVALID, "compare: null bands accepted");
    { auto j = cj; j.a = nullptr; EXPECT(fra_compare(ctx, &j, bands) == FRA_E_INVALID, "compare: null a accepted"); }
    { auto j = cj; j.b = nullptr; EXPECT(fra_compare(ctx, &j, bands) == FRA_E_INVALID, "compare: null b accepted"); }
    { auto j = cj; j.dtype = 8; EXPECT(fra_compare(ctx, &j, bands) == FRA_E_INVALID && g_msg.find("dtype") != std::string::npos, "compare: dtype 8 accepted"); }
    { auto j = cj; j.width = 0; EXPECT(fra_compare(ctx, &j, bands) == FRA_E_INVALID && g_msg.find("layout") != std::string::npos, "compare: zero width accepted"); }
    { auto j = cj; j.channels = 0; EXPECT(fra_compare(ctx, &j, bands) == FRA_E_INVALID, "compare: no channels accepted"); }
    { auto j = cj; j.b_row_stride = -8; EXPECT(fra_compare(ctx, &j, bands) == FRA_E_INVALID, "compare: negative stride accepted"); }
    { auto j = cj; j.height = 65537; j.width = 65536; EXPECT(fra_compare(ctx, &j, bands) == FRA_E_INVALID && g_msg.find("2^32 pixels") != std::string::npos, "compare: more than 2^32 pixels accepted"); }
    EXPECT(fra_compare_timing(nullptr) == FRA_E_INVALID, "compare timing: null accepted");
  }
  // ... and of the statistics (fra_stats.hip): refused before any GPU work
  {
    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;
    dj.items = &di;
    dj.dst = nullptr;  // ignored, as are the job's strides
    dj.band_stride = dj.row_stride = dj.col_stride = -1;
    const fra_window r48{0, 0, 4, 8};
    fra_stats_band bands[1];
    uint64_t hist[8];
    fra_stats_opts none{};
    fra_stats_opts eight{};
    eight.bins = 8; eight.hist_lo = 0.0; eight.hist_hi = 1.0;
    auto st = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, const fra_stats_opts* o, fra_stats_band* b,
                  uint64_t* h, fra_decoded* d) { return fra_decode_device_stats(c, j, r, o, b, h, d); };
    EXPECT(st(nullptr, &dj, &r48, &none, bands, hist, inf) == FRA_E_INVALID, "statistics read: null ctx accepted");
    EXPECT(st(ctx, nullptr, &r48, &none, bands, hist, inf) == FRA_E_INVALID, "statistics read: null job accepted");
    EXPECT(st(ctx, &dj, nullptr, &none, bands, hist, inf) == FRA_E_INVALID, "statistics read: null roi accepted");
    EXPECT(st(ctx, &dj, &r48, nullptr, bands, hist, inf) == FRA_E_INVALID, "statistics read: null options accepted");
    EXPECT(st(ctx, &dj, &r48, &none, nullptr, hist, inf) == FRA_E_INVALID, "statistics read: null bands accepted");
    EXPECT(st(ctx, &dj, &r48, &none, bands, hist, nullptr) == FRA_E_INVALID, "statistics read: null infos accepted");
    EXPECT(st(ctx, &dj, &r48, &eight, bands, nullptr, inf) == FRA_E_INVALID && g_msg.find("null histogram") != std::string::npos, "statistics read: null histogram with bins accepted");
    for (int b : {-1, 65537}) { auto o = eight; o.bins = b; EXPECT(st(ctx, &dj, &r48, &o, bands, hist, inf) == FRA_E_INVALID && g_msg.find("bins") != std::string::npos, "statistics read: %d bins accepted", b); }
    { auto o = eight; o.flags = 4; EXPECT(st(ctx, &dj, &r48, &o, bands, hist, inf) == FRA_E_INVALID && g_msg.find("flags") != std::string::npos, "statistics read: flag 4 accepted"); }
    { auto o = eight; o.hist_lo = 2.0; EXPECT(st(ctx, &dj, &r48, &o, bands, hist, inf) == FRA_E_INVALID && g_msg.find("range") != std::string::npos, "statistics read: inverted range accepted"); }
    { auto o = eight; o.hist_hi = HUGE_VAL; EXPECT(st(ctx, &dj, &r48, &o, bands, hist, inf) == FRA_E_INVALID && g_msg.find("range") != std::string::npos, "statistics read: infinite range accepted"); }
    { fra_window r = r48; r.height = 5; EXPECT(st(ctx, &dj, &r, &none, bands, hist, inf) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "statistics read: uncovered row accepted"); }
    { auto x = di; x.window.width = 7; auto j = dj; j.items = &x; EXPECT(st(ctx, &j, &r48, &none, bands, hist, inf) == FRA_E_INVALID && g_msg.find("do not cover") != std::string::npos, "statistics read: uncovered column accepted"); }
    { auto j = dj; j.nitems = 0; EXPECT(st(ctx, &j, &r48, &none, bands, hist, inf) == FRA_E_INVALID, "statistics read: empty job accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(st(ctx, &dj, &r, &none, bands, hist, inf) == FRA_E_INVALID && g_msg.find("region of interest") != std::string::npos, "statistics read: zero-width roi accepted"); }
    { fra_window r{0, 0, 65537, 65536}; EXPECT(st(ctx, &dj, &r, &none, bands, hist, inf) == FRA_E_INVALID && g_msg.find("2^32 pixels") != std::string::npos, "statistics read: more than 2^32 pixels accepted"); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(st(ctx, &j, &r48, &none, bands, hist, inf) == FRA_E_INVALID, "statistics read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.dst_dtype = 9; EXPECT(st(ctx, &j, &r48, &none, bands, hist, inf) == FRA_E_INVALID && g_msg.find("dtype") != std::string::npos, "statistics read: dtype 9 accepted"); }
    { auto j = dj; j.denorm = 7; EXPECT(st(ctx, &j, &r48, &none, bands, hist, inf) == FRA_E_INVALID, "statistics read: denorm 7 accepted"); }
    { auto j = dj; j.channels = 0; EXPECT(st(ctx, &j, &r48, &none, bands, hist, inf) == FRA_E_INVALID, "statistics read: no channels accepted"); }
    { auto x = di; x.window = {0, 0, -8, 1}; auto j = dj; j.items = &x; EXPECT(st(ctx, &j, &r48, &none, bands, hist, inf) == FRA_E_INVALID, "statistics read: capacity window accepted"); }
    fra_stats_job sj{};
    sj.src = dst; sj.dtype = FRA_I32; sj.channels = 1; sj.height = 8; sj.width = 8;
    sj.band_stride = 64; sj.row_stride = 8; sj.col_stride = 1;
    EXPECT(fra_stats(nullptr, &sj, bands, hist) == FRA_E_INVALID, "statistics: null ctx accepted");
    EXPECT(fra_stats(ctx, nullptr, bands, hist) == FRA_E_INVALID, "statistics: null job accepted");
    EXPECT(fra_stats(ctx, &sj, nullptr, hist) == FRA_E_INVALID, "statistics: null bands accepted");
    { auto j = sj; j.src = nullptr; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID, "statistics: null src accepted"); }
    { auto j = sj; j.dtype = 8; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID && g_msg.find("dtype") != std::string::npos, "statistics: dtype 8 accepted"); }
    { auto j = sj; j.width = 0; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID && g_msg.find("layout") != std::string::npos, "statistics: zero width accepted"); }
    { auto j = sj; j.channels = 0; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID, "statistics: no channels accepted"); }
    { auto j = sj; j.row_stride = -8; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID, "statistics: negative stride accepted"); }
    { auto j = sj; j.height = 65537; j.width = 65536; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID && g_msg.find("2^32 pixels") != std::string::npos, "statistics: more than 2^32 pixels accepted"); }
    { auto j = sj; j.opts = eight; EXPECT(fra_stats(ctx, &j, bands, nullptr) == FRA_E_INVALID && g_msg.find("null histogram") != std::string::npos, "statistics: null histogram with bins accepted"); }
    for (int b : {-1, 65537}) { auto j = sj; j.opts = eight; j.opts.bins = b; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID && g_msg.find("bins") != std::string::npos, "statistics: %d bins accepted", b); }
    { auto j = sj; j.opts.flags = 8; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID && g_msg.find("flags") != std::string::npos, "statistics: flag 8 accepted"); }
    { auto j = sj; j.opts = eight; j.opts.hist_hi = -1.0; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID && g_msg.find("range") != std::string::npos, "statistics: inverted range accepted"); }
    { auto j = sj; j.opts = eight; j.opts.hist_lo = -HUGE_VAL; EXPECT(fra_stats(ctx, &j, bands, hist) == FRA_E_INVALID && g_msg.find("range") != std::string::npos, "statistics: infinite range accepted"); }
    EXPECT(fra_stats_timing(nullptr) == FRA_E_INVALID, "statistics timing: null accepted");
  }
  // ... and of the band math (fra_calc.hip): the program validator (fra_calc.h), which needs no context, and the
  // argument refusals of both entries, before any GPU work
  {
    auto says = [&](int rc, const char* what) { return rc == FRA_E_INVALID && g_msg.find(what) != std::string::npos; };
    auto word = [](int op, int arg = 0) { return (uint16_t)(op | arg << 8); };
    fra_calc_program ndvi{};  // (b1 - b0) / (b1 + b0)
    const uint16_t code[] = {word(FRA_CALC_BAND, 1), word(FRA_CALC_BAND, 0), word(FRA_CALC_SUB), word(FRA_CALC_BAND, 1),
                             word(FRA_CALC_BAND, 0), word(FRA_CALC_ADD), word(FRA_CALC_DIV), word(FRA_CALC_STORE, 0)};
    memcpy(ndvi.code, code, sizeof(code));
    ndvi.ncode = 8; ndvi.nout = 1;
    EXPECT(fra_calc_check(&ndvi, 2) == FRA_OK, "calc check: NDVI refused: %s", g_msg.c_str());
    EXPECT(fra_calc_check(nullptr, 2) == FRA_E_INVALID, "calc check: null program accepted");
    EXPECT(says(fra_calc_check(&ndvi, 1), "word 0: band 1 of 1"), "calc check: band past the channels: %s", g_msg.c_str());
    for (int ch : {0, 256}) EXPECT(says(fra_calc_check(&ndvi, ch), "source bands"), "calc check: %d channels accepted", ch);
    for (int n : {0, -1, 129}) { auto p = ndvi; p.ncode = n; EXPECT(says(fra_calc_check(&p, 2), "words outside"), "calc check: %d words accepted", n); }
    for (int n : {-1, 33}) { auto p = ndvi; p.nconst = n; EXPECT(says(fra_calc_check(&p, 2), "constants outside"), "calc check: %d constants accepted", n); }
    for (int n : {0, 9}) { auto p = ndvi; p.nout = n; EXPECT(says(fra_calc_check(&p, 2), "outputs outside"), "calc check: %d outputs accepted", n); }
    { auto p = ndvi; p.flags = 2; EXPECT(says(fra_calc_check(&p, 2), "flags"), "calc check: flag 2 accepted"); }
    { auto p = ndvi; p.flags = FRA_CALC_NODATA; p.nodata = NAN; p.fill = HUGE_VAL; EXPECT(fra_calc_check(&p, 2) == FRA_OK, "calc check: NaN nodata and infinite fill refused"); }
    { auto p = ndvi; p.code[2] = word(23); EXPECT(says(fra_calc_check(&p, 2), "word 2: unknown op 23"), "calc check: op 23: %s", g_msg.c_str()); }
    { auto p = ndvi; p.code[2] = word(255, 255); EXPECT(says(fra_calc_check(&p, 2), "word 2: unknown op 255"), "calc check: op 255: %s", g_msg.c_str()); }
    { auto p = ndvi; p.code[2] = word(FRA_CALC_SUB, 1); EXPECT(says(fra_calc_check(&p, 2), "word 2: op 4 takes no argument"), "calc check: SUB with an argument: %s", g_msg.c_str()); }
    { auto p = ndvi; p.code[1] = word(FRA_CALC_CONST, 0); EXPECT(says(fra_calc_check(&p, 2), "word 1: constant 0 of 0"), "calc check: constant past nconst: %s", g_msg.c_str()); }
    { auto p = ndvi; p.code[1] = word(FRA_CALC_CONST, 31); p.nconst = 32; p.consts[31] = NAN; EXPECT(fra_calc_check(&p, 2) == FRA_OK, "calc check: a NaN constant refused"); }
    { auto p = ndvi; p.code[0] = word(FRA_CALC_NEG); EXPECT(says(fra_calc_check(&p, 2), "word 0: stack underflow"), "calc check: underflow: %s", g_msg.c_str()); }
    { auto p = ndvi; p.code[3] = word(FRA_CALC_SELECT); EXPECT(says(fra_calc_check(&p, 2), "word 3: stack underflow"), "calc check: SELECT of one value: %s", g_msg.c_str()); }
    { auto p = ndvi; p.code[7] = word(FRA_CALC_STORE, 1); EXPECT(says(fra_calc_check(&p, 2), "word 7: output 1 of 1"), "calc check: output past nout: %s", g_msg.c_str()); }
    { auto p = ndvi; p.nout = 2; EXPECT(says(fra_calc_check(&p, 2), "word 7: output 1 is never stored"), "calc check: missing output: %s", g_msg.c_str()); }
    { auto p = ndvi; p.ncode = 7; EXPECT(says(fra_calc_check(&p, 2), "word 6: 1 values left"), "calc check: values left: %s", g_msg.c_str()); }
    { auto p = ndvi; p.code[8] = word(FRA_CALC_BAND, 0); p.code[9] = word(FRA_CALC_STORE, 0); p.ncode = 10; EXPECT(says(fra_calc_check(&p, 2), "word 9: output 0 stored twice"), "calc check: stored twice: %s", g_msg.c_str()); }
    { fra_calc_program p{}; for (int i = 0; i < 9; i++) p.code[i] = word(FRA_CALC_BAND, 0); p.ncode = 9; p.nout = 1; EXPECT(says(fra_calc_check(&p, 2), "word 8: stack deeper than 8"), "calc check: depth 9: %s", g_msg.c_str()); }
    { fra_calc_program p{}; for (int i = 0; i < 128; i++) p.code[i] = word(i % 2 ? FRA_CALC_NEG : FRA_CALC_ABS); p.code[0] = word(FRA_CALC_BAND, 254); p.code[127] = word(FRA_CALC_STORE, 0); p.ncode = 128; p.nout = 1; EXPECT(fra_calc_check(&p, 255) == FRA_OK, "calc check: 128 words over band 254 refused: %s", g_msg.c_str()); }
    // every word of every value: the validator reads nothing outside the program
    { fra_calc_program p{}; p.ncode = 1; p.nout = 1; for (int w = 0; w < 65536; w++) { p.code[0] = (uint16_t)w; EXPECT(fra_calc_check(&p, 255) == FRA_E_INVALID, "calc check: the lone word %d accepted", w); } }

    static float out[64];
    fra_calc_job cj{};
    cj.src = dst; cj.dtype = FRA_I32; cj.channels = 2; cj.height = 4; cj.width = 8;
    cj.band_stride = 32; cj.row_stride = 8; cj.col_stride = 1;
    cj.program = ndvi;
    cj.out.dst = out; cj.out.dtype = FRA_F32; cj.out.band_stride = 32; cj.out.row_stride = 8; cj.out.col_stride = 1;
    uint64_t left[8];
    EXPECT(fra_calc(nullptr, &cj, left) == FRA_E_INVALID, "calc: null ctx accepted");
    EXPECT(fra_calc(ctx, nullptr, left) == FRA_E_INVALID, "calc: null job accepted");
    { auto j = cj; j.src = nullptr; EXPECT(fra_calc(ctx, &j, left) == FRA_E_INVALID, "calc: null src accepted"); }
    { auto j = cj; j.out.dst = nullptr; EXPECT(fra_calc(ctx, &j, nullptr) == FRA_E_INVALID, "calc: null dst accepted"); }
    { auto j = cj; j.channels = 1; EXPECT(says(fra_calc(ctx, &j, left), "word 0: band 1 of 1"), "calc: band past the channels: %s", g_msg.c_str()); }
    { auto j = cj; j.program.code[7] = word(FRA_CALC_ADD); EXPECT(says(fra_calc(ctx, &j, left), "word 7"), "calc: invalid program: %s", g_msg.c_str()); }
    { auto j = cj; j.dtype = 8; EXPECT(says(fra_calc(ctx, &j, left), "bad dtype"), "calc: source dtype 8: %s", g_msg.c_str()); }
    { auto j = cj; j.out.dtype = -1; EXPECT(says(fra_calc(ctx, &j, left), "bad dtype"), "calc: destination dtype -1: %s", g_msg.c_str()); }
    { auto j = cj; j.width = 0; EXPECT(says(fra_calc(ctx, &j, left), "bad raster layout"), "calc: zero width: %s", g_msg.c_str()); }
    { auto j = cj; j.row_stride = -8; EXPECT(says(fra_calc(ctx, &j, left), "bad raster layout"), "calc: negative source stride: %s", g_msg.c_str()); }
    { auto j = cj; j.out.col_stride = -1; EXPECT(says(fra_calc(ctx, &j, left), "bad raster layout"), "calc: negative destination stride: %s", g_msg.c_str()); }
    { auto j = cj; j.height = 65537; j.width = 65536; EXPECT(says(fra_calc(ctx, &j, left), "2^32 pixels"), "calc: more than 2^32 pixels: %s", g_msg.c_str()); }
    // the order: the program, then the source, then the destination, then the size
    { auto j = cj; j.program.ncode = 0; j.dtype = 8; EXPECT(says(fra_calc(ctx, &j, left), "words outside"), "calc: no words and dtype 8: %s", g_msg.c_str()); }
    { auto j = cj; j.dtype = 8; j.out.dtype = 8; j.width = 0; EXPECT(says(fra_calc(ctx, &j, left), "bad dtype"), "calc: dtype 8 and zero width: %s", g_msg.c_str()); }
    { auto j = cj; j.out.row_stride = -1; j.height = 65537; j.width = 65536; EXPECT(says(fra_calc(ctx, &j, left), "bad raster layout"), "calc: negative stride and 2^32 pixels: %s", g_msg.c_str()); }
    EXPECT(fra_calc_timing(nullptr) == FRA_E_INVALID, "calc timing: null accepted");

    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;
    dj.items = &di;
    dj.dst = nullptr;  // ignored, as are the job's strides
    dj.band_stride = dj.row_stride = dj.col_stride = -1;
    dj.channels = 2;
    const fra_window r48{0, 0, 4, 8};
    const fra_calc_dst od = cj.out;
    auto rc = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, const fra_calc_program* p, const fra_calc_dst* o,
                  fra_decoded* d) { return fra_decode_device_calc(c, j, r, p, o, left, d); };
    EXPECT(rc(nullptr, &dj, &r48, &ndvi, &od, inf) == FRA_E_INVALID, "calc read: null ctx accepted");
    EXPECT(rc(ctx, nullptr, &r48, &ndvi, &od, inf) == FRA_E_INVALID, "calc read: null job accepted");
    EXPECT(rc(ctx, &dj, nullptr, &ndvi, &od, inf) == FRA_E_INVALID, "calc read: null roi accepted");
    EXPECT(rc(ctx, &dj, &r48, nullptr, &od, inf) == FRA_E_INVALID, "calc read: null program accepted");
    EXPECT(rc(ctx, &dj, &r48, &ndvi, nullptr, inf) == FRA_E_INVALID, "calc read: null destination accepted");
    EXPECT(rc(ctx, &dj, &r48, &ndvi, &od, nullptr) == FRA_E_INVALID, "calc read: null infos accepted");
    { auto o = od; o.dst = nullptr; EXPECT(rc(ctx, &dj, &r48, &ndvi, &o, inf) == FRA_E_INVALID, "calc read: null dst accepted"); }
    { auto j = dj; j.channels = 1; EXPECT(says(rc(ctx, &j, &r48, &ndvi, &od, inf), "word 0: band 1 of 1"), "calc read: band past the channels: %s", g_msg.c_str()); }
    { auto p = ndvi; p.nout = 9; EXPECT(says(rc(ctx, &dj, &r48, &p, &od, inf), "outputs outside"), "calc read: 9 outputs: %s", g_msg.c_str()); }
    { auto o = od; o.dtype = 8; EXPECT(says(rc(ctx, &dj, &r48, &ndvi, &o, inf), "bad dtype"), "calc read: destination dtype 8: %s", g_msg.c_str()); }
    { auto o = od; o.band_stride = -1; EXPECT(says(rc(ctx, &dj, &r48, &ndvi, &o, inf), "bad raster layout"), "calc read: negative destination stride: %s", g_msg.c_str()); }
    { fra_window r = r48; r.height = 5; EXPECT(says(rc(ctx, &dj, &r, &ndvi, &od, inf), "do not cover"), "calc read: uncovered row: %s", g_msg.c_str()); }
    { auto x = di; x.window.width = 7; auto j = dj; j.items = &x; EXPECT(says(rc(ctx, &j, &r48, &ndvi, &od, inf), "do not cover"), "calc read: uncovered column: %s", g_msg.c_str()); }
    { auto j = dj; j.nitems = 0; EXPECT(rc(ctx, &j, &r48, &ndvi, &od, inf) == FRA_E_INVALID, "calc read: empty job accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(says(rc(ctx, &dj, &r, &ndvi, &od, inf), "region of interest"), "calc read: zero-width roi: %s", g_msg.c_str()); }
    { fra_window r{0, 0, 65537, 65536}; EXPECT(says(rc(ctx, &dj, &r, &ndvi, &od, inf), "2^32 pixels"), "calc read: more than 2^32 pixels: %s", g_msg.c_str()); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(rc(ctx, &j, &r48, &ndvi, &od, inf) == FRA_E_INVALID, "calc read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.dst_dtype = 9; EXPECT(says(rc(ctx, &j, &r48, &ndvi, &od, inf), "dtype"), "calc read: dtype 9: %s", g_msg.c_str()); }
    { auto j = dj; j.denorm = 7; EXPECT(rc(ctx, &j, &r48, &ndvi, &od, inf) == FRA_E_INVALID, "calc read: denorm 7 accepted"); }
    { auto j = dj; j.channels = 0; EXPECT(rc(ctx, &j, &r48, &ndvi, &od, inf) == FRA_E_INVALID, "calc read: no channels accepted"); }
    // the windowed read's refusals come first, then the program, then the destination, then the cover
    { fra_window r = r48; r.width = 0; auto p = ndvi; p.ncode = 0; EXPECT(says(rc(ctx, &dj, &r, &p, &od, inf), "region of interest"), "calc read: zero-width roi and no words: %s", g_msg.c_str()); }
    { fra_window r = r48; r.height = 5; auto p = ndvi; p.ncode = 0; EXPECT(says(rc(ctx, &dj, &r, &p, &od, inf), "words outside"), "calc read: uncovered row and no words: %s", g_msg.c_str()); }

    // ... and of the focal operations (fra_focal.hip): the spec validator, which needs no context, and the two entries
    fra_focal_spec mean3{};
    mean3.op = FRA_FOCAL_MEAN; mean3.kh = 3; mean3.kw = 3; mean3.edge = FRA_FOCAL_EDGE_SKIP;
    EXPECT(fra_focal_check(&mean3) == FRA_OK, "focal check: a 3 x 3 mean refused: %s", g_msg.c_str());
    EXPECT(fra_focal_check(nullptr) == FRA_E_INVALID, "focal check: null spec accepted");
    for (int op : {-1, 9}) { auto s = mean3; s.op = op; EXPECT(says(fra_focal_check(&s), "op: unknown focal op"), "focal check: op %d: %s", op, g_msg.c_str()); }
    for (int e : {-1, 2}) { auto s = mean3; s.edge = e; EXPECT(says(fra_focal_check(&s), "edge: unknown edge mode"), "focal check: edge %d: %s", e, g_msg.c_str()); }
    { auto s = mean3; s.flags = 8; EXPECT(says(fra_focal_check(&s), "flags: unknown focal flags"), "focal check: flag 8: %s", g_msg.c_str()); }
    for (int k : {0, 2, 17, -3}) { auto s = mean3; s.kh = k; EXPECT(says(fra_focal_check(&s), "kh: window height"), "focal check: kh %d: %s", k, g_msg.c_str()); }
    for (int k : {0, 4, 17, -1}) { auto s = mean3; s.kw = k; EXPECT(says(fra_focal_check(&s), "kw: window width"), "focal check: kw %d: %s", k, g_msg.c_str()); }
    { auto s = mean3; s.kh = s.kw = 15; s.flags = FRA_FOCAL_NODATA | FRA_FOCAL_KEEP_MASK; s.nodata = NAN; s.fill = HUGE_VAL; EXPECT(fra_focal_check(&s) == FRA_OK, "focal check: 15 x 15, NaN nodata and infinite fill refused: %s", g_msg.c_str()); }
    { auto s = mean3; s.op = FRA_FOCAL_MEDIAN; s.kh = 5; s.kw = 5; EXPECT(fra_focal_check(&s) == FRA_OK, "focal check: a 5 x 5 median refused"); s.kw = 7; EXPECT(says(fra_focal_check(&s), "a median of 5 x 7 taps"), "focal check: a 5 x 7 median: %s", g_msg.c_str()); }
    for (int op : {FRA_FOCAL_SLOPE, FRA_FOCAL_HILLSHADE}) { auto s = mean3; s.op = op; EXPECT(fra_focal_check(&s) == FRA_OK, "focal check: 3 x 3 terrain op refused"); s.kh = 5; EXPECT(says(fra_focal_check(&s), "take a 3 x 3 window"), "focal check: 5 x 3 terrain op: %s", g_msg.c_str()); }
    { auto s = mean3; s.flags = FRA_FOCAL_NORMALIZE; EXPECT(says(fra_focal_check(&s), "FRA_FOCAL_NORMALIZE goes with"), "focal check: a normalised mean: %s", g_msg.c_str()); s.op = FRA_FOCAL_CONVOLVE; s.weights[4] = NAN; EXPECT(fra_focal_check(&s) == FRA_OK, "focal check: a normalised convolution with a NaN weight refused"); }

    fra_focal_job fj{};
    fj.src = dst; fj.dtype = FRA_I32; fj.channels = 2; fj.height = 4; fj.width = 8;
    fj.band_stride = 32; fj.row_stride = 8; fj.col_stride = 1;
    fj.rect = {0, 0, 4, 8};
    fj.spec = mean3;
    fj.out = cj.out;
    EXPECT(fra_focal(nullptr, &fj, left) == FRA_E_INVALID, "focal: null ctx accepted");
    EXPECT(fra_focal(ctx, nullptr, left) == FRA_E_INVALID, "focal: null job accepted");
    { auto j = fj; j.src = nullptr; EXPECT(fra_focal(ctx, &j, left) == FRA_E_INVALID, "focal: null src accepted"); }
    { auto j = fj; j.out.dst = nullptr; EXPECT(fra_focal(ctx, &j, nullptr) == FRA_E_INVALID, "focal: null dst accepted"); }
    { auto j = fj; j.spec.kw = 2; EXPECT(says(fra_focal(ctx, &j, left), "kw: window width"), "focal: even window: %s", g_msg.c_str()); }
    { auto j = fj; j.dtype = 8; EXPECT(says(fra_focal(ctx, &j, left), "bad dtype"), "focal: source dtype 8: %s", g_msg.c_str()); }
    { auto j = fj; j.out.dtype = -1; EXPECT(says(fra_focal(ctx, &j, left), "bad dtype"), "focal: destination dtype -1: %s", g_msg.c_str()); }
    { auto j = fj; j.width = 0; EXPECT(says(fra_focal(ctx, &j, left), "bad raster layout"), "focal: zero width: %s", g_msg.c_str()); }
    { auto j = fj; j.row_stride = -8; EXPECT(says(fra_focal(ctx, &j, left), "bad raster layout"), "focal: negative source stride: %s", g_msg.c_str()); }
    { auto j = fj; j.out.col_stride = -1; EXPECT(says(fra_focal(ctx, &j, left), "bad raster layout"), "focal: negative destination stride: %s", g_msg.c_str()); }
    { auto j = fj; j.channels = 256; EXPECT(says(fra_focal(ctx, &j, left), "more than 255"), "focal: 256 bands: %s", g_msg.c_str()); }
    for (fra_window r : {fra_window{0, 0, 0, 8}, fra_window{0, 0, 4, 0}, fra_window{-1, 0, 4, 8}, fra_window{0, -1, 4, 8}, fra_window{1, 0, 4, 8}, fra_window{0, 1, 4, 8}, fra_window{0, 0, 2147483647, 8}, fra_window{2147483647, 0, 1, 8}}) {
      auto j = fj; j.rect = r; EXPECT(says(fra_focal(ctx, &j, left), "the output rectangle"), "focal: rectangle (%d, %d, %d x %d): %s", r.row_off, r.col_off, r.height, r.width, g_msg.c_str());
    }
    { auto j = fj; j.height = 65537; j.width = 65536; EXPECT(says(fra_focal(ctx, &j, left), "2^32 pixels"), "focal: more than 2^32 pixels: %s", g_msg.c_str()); }
    // the order: the spec, then the layouts, then the rectangle, then the size
    { auto j = fj; j.spec.op = 9; j.dtype = 8; EXPECT(says(fra_focal(ctx, &j, left), "op: unknown"), "focal: op 9 and dtype 8: %s", g_msg.c_str()); }
    { auto j = fj; j.out.dtype = 8; j.rect.width = 9; EXPECT(says(fra_focal(ctx, &j, left), "bad dtype"), "focal: dtype 8 and a wide rectangle: %s", g_msg.c_str()); }
    { auto j = fj; j.rect.width = 0; j.height = 65537; j.width = 65536; EXPECT(says(fra_focal(ctx, &j, left), "the output rectangle"), "focal: empty rectangle and 2^32 pixels: %s", g_msg.c_str()); }
    EXPECT(fra_focal_timing(nullptr) == FRA_E_INVALID, "focal timing: null accepted");

    const fra_window in48{0, 0, 4, 8};
    auto rf = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, const fra_focal_spec* s, const fra_window* in,
                  const fra_calc_dst* o, fra_decoded* d) { return fra_decode_device_focal(c, j, r, s, in, o, left, d); };
    EXPECT(rf(nullptr, &dj, &r48, &mean3, &in48, &od, inf) == FRA_E_INVALID, "focal read: null ctx accepted");
    EXPECT(rf(ctx, nullptr, &r48, &mean3, &in48, &od, inf) == FRA_E_INVALID, "focal read: null job accepted");
    EXPECT(rf(ctx, &dj, nullptr, &mean3, &in48, &od, inf) == FRA_E_INVALID, "focal read: null roi accepted");
    EXPECT(rf(ctx, &dj, &r48, nullptr, &in48, &od, inf) == FRA_E_INVALID, "focal read: null spec accepted");
    EXPECT(rf(ctx, &dj, &r48, &mean3, nullptr, &od, inf) == FRA_E_INVALID, "focal read: null inner rectangle accepted");
    EXPECT(rf(ctx, &dj, &r48, &mean3, &in48, nullptr, inf) == FRA_E_INVALID, "focal read: null destination accepted");
    EXPECT(rf(ctx, &dj, &r48, &mean3, &in48, &od, nullptr) == FRA_E_INVALID, "focal read: null infos accepted");
    { auto o = od; o.dst = nullptr; EXPECT(rf(ctx, &dj, &r48, &mean3, &in48, &o, inf) == FRA_E_INVALID, "focal read: null dst accepted"); }
    { auto s = mean3; s.kh = 4; EXPECT(says(rf(ctx, &dj, &r48, &s, &in48, &od, inf), "kh: window height"), "focal read: even window: %s", g_msg.c_str()); }
    { auto o = od; o.dtype = 8; EXPECT(says(rf(ctx, &dj, &r48, &mean3, &in48, &o, inf), "bad dtype"), "focal read: destination dtype 8: %s", g_msg.c_str()); }
    { auto o = od; o.band_stride = -1; EXPECT(says(rf(ctx, &dj, &r48, &mean3, &in48, &o, inf), "bad raster layout"), "focal read: negative destination stride: %s", g_msg.c_str()); }
    for (fra_window in : {fra_window{0, 0, 0, 8}, fra_window{0, 0, 5, 8}, fra_window{0, 1, 4, 8}, fra_window{-1, 0, 2, 2}}) {
      EXPECT(says(rf(ctx, &dj, &r48, &mean3, &in, &od, inf), "the inner rectangle"), "focal read: inner (%d, %d, %d x %d): %s", in.row_off, in.col_off, in.height, in.width, g_msg.c_str());
    }
    { fra_window r = r48; r.height = 5; EXPECT(says(rf(ctx, &dj, &r, &mean3, &in48, &od, inf), "do not cover"), "focal read: uncovered row: %s", g_msg.c_str()); }
    { auto j = dj; j.nitems = 0; EXPECT(rf(ctx, &j, &r48, &mean3, &in48, &od, inf) == FRA_E_INVALID, "focal read: empty job accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(says(rf(ctx, &dj, &r, &mean3, &in48, &od, inf), "region of interest"), "focal read: zero-width roi: %s", g_msg.c_str()); }
    { fra_window r{0, 0, 65537, 65536}; EXPECT(says(rf(ctx, &dj, &r, &mean3, &in48, &od, inf), "2^32 pixels"), "focal read: more than 2^32 pixels: %s", g_msg.c_str()); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(rf(ctx, &j, &r48, &mean3, &in48, &od, inf) == FRA_E_INVALID, "focal read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.dst_dtype = 9; EXPECT(says(rf(ctx, &j, &r48, &mean3, &in48, &od, inf), "dtype"), "focal read: dtype 9: %s", g_msg.c_str()); }
    { auto j = dj; j.channels = 0; EXPECT(rf(ctx, &j, &r48, &mean3, &in48, &od, inf) == FRA_E_INVALID, "focal read: no channels accepted"); }
    // the windowed read's refusals come first, then the spec, then the destination, then the inner rectangle, then the cover
    { fra_window r = r48; r.width = 0; auto s = mean3; s.op = 9; EXPECT(says(rf(ctx, &dj, &r, &s, &in48, &od, inf), "region of interest"), "focal read: zero-width roi and op 9: %s", g_msg.c_str()); }
    { fra_window r = r48; r.height = 5; fra_window in{0, 0, 6, 8}; EXPECT(says(rf(ctx, &dj, &r, &mean3, &in, &od, inf), "the inner rectangle"), "focal read: uncovered row and a tall inner rectangle: %s", g_msg.c_str()); }
  }
  // ... and of the zonal statistics (fra_zonal.hip): refused before any GPU work, in the order the header gives
  {
    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;
    dj.items = &di;
    dj.dst = nullptr;  // ignored, as are the job's strides
    dj.band_stride = dj.row_stride = dj.col_stride = -1;
    const fra_window r48{0, 0, 4, 8};
    auto says = [&](int rc, const char* what) { return rc == FRA_E_INVALID && g_msg.find(what) != std::string::npos; };
    static uint16_t zones[64];
    fra_zonal_rec recs[4];
    uint64_t outside = 0;
    fra_zonal_opts four{};
    four.nzones = 4;
    fra_zonal_job zj{};
    zj.src = dst; zj.dtype = FRA_I32; zj.channels = 1; zj.height = 8; zj.width = 8;
    zj.band_stride = 64; zj.row_stride = 8; zj.col_stride = 1;
    zj.zones = zones; zj.zone_dtype = FRA_U16; zj.zone_row_stride = 8; zj.zone_col_stride = 1;
    zj.opts = four;
    EXPECT(fra_zonal(nullptr, &zj, recs, &outside) == FRA_E_INVALID, "zonal: null ctx accepted");
    EXPECT(fra_zonal(ctx, nullptr, recs, &outside) == FRA_E_INVALID, "zonal: null job accepted");
    EXPECT(fra_zonal(ctx, &zj, nullptr, &outside) == FRA_E_INVALID, "zonal: null records accepted");
    EXPECT(fra_zonal(ctx, &zj, recs, nullptr) == FRA_E_INVALID, "zonal: null outside accepted");
    { auto j = zj; j.src = nullptr; EXPECT(fra_zonal(ctx, &j, recs, &outside) == FRA_E_INVALID, "zonal: null src accepted"); }
    { auto j = zj; j.zones = nullptr; EXPECT(fra_zonal(ctx, &j, recs, &outside) == FRA_E_INVALID, "zonal: null zones accepted"); }
    { auto j = zj; j.dtype = 8; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad dtype"), "zonal: dtype 8: %s", g_msg.c_str()); }
    { auto j = zj; j.width = 0; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad raster layout"), "zonal: zero width: %s", g_msg.c_str()); }
    { auto j = zj; j.row_stride = -8; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad raster layout"), "zonal: negative stride: %s", g_msg.c_str()); }
    for (int z : {-1, (int)FRA_F32, (int)FRA_F64, 8}) { auto j = zj; j.zone_dtype = z; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad zone dtype"), "zonal: zone dtype %d: %s", z, g_msg.c_str()); }
    { auto j = zj; j.zone_row_stride = -8; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad zone layout"), "zonal: negative zone row stride: %s", g_msg.c_str()); }
    { auto j = zj; j.zone_col_stride = -1; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad zone layout"), "zonal: negative zone column stride: %s", g_msg.c_str()); }
    for (int n : {0, -1, 65537}) { auto j = zj; j.opts.nzones = n; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "nzones"), "zonal: nzones %d: %s", n, g_msg.c_str()); }
    { auto j = zj; j.opts.flags = 4; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "unknown zonal flags"), "zonal: flag 4: %s", g_msg.c_str()); }
    { auto j = zj; j.height = 65537; j.width = 65536; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "2^32 pixels"), "zonal: more than 2^32 pixels: %s", g_msg.c_str()); }
    { auto j = zj; j.channels = 257; j.opts.nzones = 65536; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "2^24 records"), "zonal: 257 bands x 65536 zones: %s", g_msg.c_str()); }
    // ... the order: the first broken rule speaks
    { auto j = zj; j.dtype = 8; j.zone_dtype = 7; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad dtype"), "zonal: dtype 8 and zone dtype 7: %s", g_msg.c_str()); }
    { auto j = zj; j.zone_dtype = 7; j.zone_row_stride = -1; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad zone dtype"), "zonal: zone dtype 7 and a negative zone stride: %s", g_msg.c_str()); }
    { auto j = zj; j.zone_col_stride = -1; j.opts.nzones = 0; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "bad zone layout"), "zonal: negative zone stride and no zones: %s", g_msg.c_str()); }
    { auto j = zj; j.opts.nzones = 0; j.opts.flags = 4; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "nzones"), "zonal: no zones and flag 4: %s", g_msg.c_str()); }
    { auto j = zj; j.opts.flags = 4; j.height = 65537; j.width = 65536; EXPECT(says(fra_zonal(ctx, &j, recs, &outside), "unknown zonal flags"), "zonal: flag 4 and 2^32 pixels: %s", g_msg.c_str()); }
    EXPECT(fra_zonal_timing(nullptr) == FRA_E_INVALID, "zonal timing: null accepted");
    auto zr = [&](fra_ctx* c, const fra_decode_job* j, const fra_window* r, const void* z, int zd, int64_t zrs, int64_t zcs,
                  const fra_zonal_opts* o, fra_zonal_rec* rc, uint64_t* out, fra_decoded* d) {
      return fra_decode_device_zonal(c, j, r, z, 0, zd, zrs, zcs, o, rc, out, d);
    };
    EXPECT(zr(nullptr, &dj, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, inf) == FRA_E_INVALID, "zonal read: null ctx accepted");
    EXPECT(zr(ctx, nullptr, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, inf) == FRA_E_INVALID, "zonal read: null job accepted");
    EXPECT(zr(ctx, &dj, nullptr, zones, FRA_U16, 8, 1, &four, recs, &outside, inf) == FRA_E_INVALID, "zonal read: null roi accepted");
    EXPECT(zr(ctx, &dj, &r48, nullptr, FRA_U16, 8, 1, &four, recs, &outside, inf) == FRA_E_INVALID, "zonal read: null zones accepted");
    EXPECT(zr(ctx, &dj, &r48, zones, FRA_U16, 8, 1, nullptr, recs, &outside, inf) == FRA_E_INVALID, "zonal read: null options accepted");
    EXPECT(zr(ctx, &dj, &r48, zones, FRA_U16, 8, 1, &four, nullptr, &outside, inf) == FRA_E_INVALID, "zonal read: null records accepted");
    EXPECT(zr(ctx, &dj, &r48, zones, FRA_U16, 8, 1, &four, recs, nullptr, inf) == FRA_E_INVALID, "zonal read: null outside accepted");
    EXPECT(zr(ctx, &dj, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, nullptr) == FRA_E_INVALID, "zonal read: null infos accepted");
    for (int z : {-1, (int)FRA_F32, 8}) EXPECT(says(zr(ctx, &dj, &r48, zones, z, 8, 1, &four, recs, &outside, inf), "bad zone dtype"), "zonal read: zone dtype %d: %s", z, g_msg.c_str());
    EXPECT(says(zr(ctx, &dj, &r48, zones, FRA_U16, -8, 1, &four, recs, &outside, inf), "bad zone layout"), "zonal read: negative zone stride: %s", g_msg.c_str());
    for (int n : {0, 65537}) { auto o = four; o.nzones = n; EXPECT(says(zr(ctx, &dj, &r48, zones, FRA_U16, 8, 1, &o, recs, &outside, inf), "nzones"), "zonal read: nzones %d: %s", n, g_msg.c_str()); }
    { auto o = four; o.flags = 8; EXPECT(says(zr(ctx, &dj, &r48, zones, FRA_U16, 8, 1, &o, recs, &outside, inf), "unknown zonal flags"), "zonal read: flag 8: %s", g_msg.c_str()); }
    { fra_window r = r48; r.height = 5; EXPECT(says(zr(ctx, &dj, &r, zones, FRA_U16, 8, 1, &four, recs, &outside, inf), "do not cover"), "zonal read: uncovered row: %s", g_msg.c_str()); }
    { auto x = di; x.window.width = 7; auto j = dj; j.items = &x; EXPECT(says(zr(ctx, &j, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, inf), "do not cover"), "zonal read: uncovered column: %s", g_msg.c_str()); }
    { auto j = dj; j.nitems = 0; EXPECT(zr(ctx, &j, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, inf) == FRA_E_INVALID, "zonal read: empty job accepted"); }
    { fra_window r = r48; r.width = 0; EXPECT(says(zr(ctx, &dj, &r, zones, FRA_U16, 8, 1, &four, recs, &outside, inf), "region of interest"), "zonal read: zero-width roi: %s", g_msg.c_str()); }
    { fra_window r{0, 0, 65537, 65536}; EXPECT(says(zr(ctx, &dj, &r, zones, FRA_U16, 8, 1, &four, recs, &outside, inf), "2^32 pixels"), "zonal read: more than 2^32 pixels: %s", g_msg.c_str()); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(zr(ctx, &j, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, inf) == FRA_E_INVALID, "zonal read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.dst_dtype = 9; EXPECT(says(zr(ctx, &j, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, inf), "dtype"), "zonal read: dtype 9: %s", g_msg.c_str()); }
    { auto j = dj; j.denorm = 7; EXPECT(zr(ctx, &j, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, inf) == FRA_E_INVALID, "zonal read: denorm 7 accepted"); }
    { auto j = dj; j.channels = 0; EXPECT(zr(ctx, &j, &r48, zones, FRA_U16, 8, 1, &four, recs, &outside, inf) == FRA_E_INVALID, "zonal read: no channels accepted"); }
    { fra_window r = r48; r.width = 0; auto o = four; o.nzones = 0; EXPECT(says(zr(ctx, &dj, &r, zones, FRA_U16, 8, 1, &o, recs, &outside, inf), "nzones"), "zonal read: no zones and zero-width roi: %s", g_msg.c_str()); }
  }
  // ... and of the warped reads (fra_warp.hip): refused before any GPU work, in the order the header gives
  {
    auto says = [&](int rc, const char* what) { return rc == FRA_E_INVALID && g_msg.find(what) != std::string::npos; };
    static int32_t wsrc[64];
    int32_t wout[15];
    uint64_t wfilled[1];
    fra_warp_job wj{};
    wj.src = wsrc; wj.dtype = FRA_I32; wj.channels = 1; wj.height = 8; wj.width = 8;
    wj.src_band_stride = 64; wj.src_row_stride = 8; wj.src_col_stride = 1;
    wj.out_height = 3; wj.out_width = 5; wj.resampling = FRA_RESAMPLE_BILINEAR;
    wj.dst = wout; wj.dst_band_stride = 15; wj.dst_row_stride = 5; wj.dst_col_stride = 1;
    wj.map.kind = FRA_WARP_AFFINE;
    wj.map.affine[0] = wj.map.affine[4] = 1.0;
    EXPECT(fra_warp(nullptr, &wj, wfilled) == FRA_E_INVALID, "warp: null ctx accepted");
    EXPECT(fra_warp(ctx, nullptr, wfilled) == FRA_E_INVALID, "warp: null job accepted");
    { auto j = wj; j.src = nullptr; EXPECT(fra_warp(ctx, &j, wfilled) == FRA_E_INVALID, "warp: null src accepted"); }
    { auto j = wj; j.dst = nullptr; EXPECT(fra_warp(ctx, &j, nullptr) == FRA_E_INVALID, "warp: null dst accepted"); }
    { auto j = wj; j.dtype = 8; EXPECT(says(fra_warp(ctx, &j, wfilled), "bad dtype"), "warp: dtype 8: %s", g_msg.c_str()); }
    { auto j = wj; j.height = 0; EXPECT(says(fra_warp(ctx, &j, wfilled), "bad raster layout"), "warp: zero height: %s", g_msg.c_str()); }
    { auto j = wj; j.dst_row_stride = -5; EXPECT(says(fra_warp(ctx, &j, wfilled), "bad raster layout"), "warp: negative stride: %s", g_msg.c_str()); }
    { auto j = wj; j.channels = 256; EXPECT(says(fra_warp(ctx, &j, wfilled), "more than 255"), "warp: 256 bands: %s", g_msg.c_str()); }
    for (int n : {0, -1, 65537}) {
      { auto j = wj; j.out_height = n; EXPECT(says(fra_warp(ctx, &j, wfilled), "output size"), "warp: out height %d: %s", n, g_msg.c_str()); }
      { auto j = wj; j.out_width = n; EXPECT(says(fra_warp(ctx, &j, wfilled), "output size"), "warp: out width %d: %s", n, g_msg.c_str()); }
    }
    { auto j = wj; j.resampling = FRA_RESAMPLE_AVERAGE; EXPECT(says(fra_warp(ctx, &j, wfilled), "point samples"), "warp: average: %s", g_msg.c_str()); }
    for (int r : {-1, 4}) { auto j = wj; j.resampling = r; EXPECT(says(fra_warp(ctx, &j, wfilled), "unknown resampling"), "warp: resampling %d: %s", r, g_msg.c_str()); }
    { auto j = wj; j.flags = 2; EXPECT(says(fra_warp(ctx, &j, wfilled), "unknown warp flags"), "warp: flag 2: %s", g_msg.c_str()); }
    for (int k : {-1, 2}) { auto j = wj; j.map.kind = k; EXPECT(says(fra_warp(ctx, &j, wfilled), "unknown map kind"), "warp: kind %d: %s", k, g_msg.c_str()); }
    for (int k = 0; k < 6; k++)
      for (double bad : {(double)NAN, (double)HUGE_VAL, -(double)HUGE_VAL}) {
        auto j = wj; j.map.affine[k] = bad; EXPECT(says(fra_warp(ctx, &j, wfilled), "is not finite"), "warp: coefficient %d = %g: %s", k, bad, g_msg.c_str());
      }
    double plane[12] = {0};
    fra_warp_job gj = wj;
    gj.map.kind = FRA_WARP_GRID; gj.map.step = 2; gj.map.gh = 3; gj.map.gw = 4; gj.map.gx = gj.map.gy = plane;
    for (int st : {0, -2}) { auto j = gj; j.map.step = st; EXPECT(says(fra_warp(ctx, &j, wfilled), "grid step"), "warp: step %d: %s", st, g_msg.c_str()); }
    { auto j = gj; j.map.gw = 5; EXPECT(says(fra_warp(ctx, &j, wfilled), "takes a grid of 3 x 4 nodes"), "warp: gw 5: %s", g_msg.c_str()); }
    { auto j = gj; j.map.gh = 2; EXPECT(says(fra_warp(ctx, &j, wfilled), "takes a grid of 3 x 4 nodes"), "warp: gh 2: %s", g_msg.c_str()); }
    { auto j = gj; j.map.step = 1; EXPECT(says(fra_warp(ctx, &j, wfilled), "takes a grid of 4 x 6 nodes"), "warp: step 1 with 3 x 4 nodes: %s", g_msg.c_str()); }
    { auto j = gj; j.map.gx = nullptr; EXPECT(says(fra_warp(ctx, &j, wfilled), "null grid"), "warp: null gx: %s", g_msg.c_str()); }
    { auto j = gj; j.map.gy = nullptr; EXPECT(says(fra_warp(ctx, &j, wfilled), "null grid"), "warp: null gy: %s", g_msg.c_str()); }
    { auto j = wj; j.flags = FRA_WARP_NODATA; j.nodata = 0.5; EXPECT(says(fra_warp(ctx, &j, wfilled), "nodata 0.5 is not a value"), "warp: nodata 0.5: %s", g_msg.c_str()); }
    { auto j = wj; j.nodata = 0.5; j.fill = 0.5; EXPECT(says(fra_warp(ctx, &j, wfilled), "fill 0.5 is not a value"), "warp: fill 0.5 (and an unused nodata): %s", g_msg.c_str()); }
    { auto j = wj; j.fill = 2147483648.0; EXPECT(says(fra_warp(ctx, &j, wfilled), "fill"), "warp: fill 2^31: %s", g_msg.c_str()); }
    { auto j = wj; j.dtype = FRA_F32; j.fill = 0.1; EXPECT(says(fra_warp(ctx, &j, wfilled), "fill"), "warp: an inexact float32 fill: %s", g_msg.c_str()); }
    { auto j = wj; j.dtype = FRA_F64; j.fill = HUGE_VAL; EXPECT(says(fra_warp(ctx, &j, wfilled), "fill"), "warp: an infinite fill: %s", g_msg.c_str()); }
    // ... the order: the layout, the sizes, the resampling, the flags, the map, nodata, fill
    { auto j = wj; j.dtype = 8; j.out_height = 0; EXPECT(says(fra_warp(ctx, &j, wfilled), "bad dtype"), "warp: dtype 8 and out height 0: %s", g_msg.c_str()); }
    { auto j = wj; j.out_height = 0; j.resampling = 1; EXPECT(says(fra_warp(ctx, &j, wfilled), "output size"), "warp: out height 0 and the average: %s", g_msg.c_str()); }
    { auto j = wj; j.resampling = 1; j.flags = 2; EXPECT(says(fra_warp(ctx, &j, wfilled), "point samples"), "warp: the average and flag 2: %s", g_msg.c_str()); }
    { auto j = gj; j.flags = 2; j.map.step = 0; EXPECT(says(fra_warp(ctx, &j, wfilled), "unknown warp flags"), "warp: flag 2 and step 0: %s", g_msg.c_str()); }
    { auto j = gj; j.map.step = 0; j.map.gx = nullptr; EXPECT(says(fra_warp(ctx, &j, wfilled), "grid step"), "warp: step 0 and a null grid: %s", g_msg.c_str()); }
    { auto j = wj; j.map.affine[2] = NAN; j.fill = 0.5; EXPECT(says(fra_warp(ctx, &j, wfilled), "is not finite"), "warp: a NaN coefficient and fill 0.5: %s", g_msg.c_str()); }
    { auto j = wj; j.flags = 1; j.nodata = 0.5; j.fill = 0.5; EXPECT(says(fra_warp(ctx, &j, wfilled), "nodata"), "warp: nodata 0.5 and fill 0.5: %s", g_msg.c_str()); }
    EXPECT(fra_warp_timing(nullptr) == FRA_E_INVALID, "warp timing: null accepted");
    EXPECT(fra_warp_paths(nullptr) == FRA_E_INVALID, "warp paths: null accepted");
    { uint64_t c[2] = {7, 7}; EXPECT(fra_warp_paths(c) == FRA_OK && c[0] == 0 && c[1] == 0, "warp paths: not zero before any call"); }
    // the read behind the decoder: an identity over a 4 x 8 raster of one item
    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;  // dst_dtype int32, a destination with strides
    dj.items = &di;
    auto rd = [&](fra_ctx* c, const fra_decode_job* j, int32_t rh, int32_t rw, const fra_warp_map* m, int32_t oh, int32_t ow, int32_t mode,
                  int32_t flags, double nd, double fl, fra_decoded* d) {
      return fra_decode_device_warped(c, j, rh, rw, m, oh, ow, mode, flags, nd, fl, d, wfilled);
    };
    const fra_warp_map& id = wj.map;
    EXPECT(rd(nullptr, &dj, 4, 8, &id, 3, 5, 2, 0, 0.0, 0.0, inf) == FRA_E_INVALID, "warped read: null ctx accepted");
    EXPECT(rd(ctx, nullptr, 4, 8, &id, 3, 5, 2, 0, 0.0, 0.0, inf) == FRA_E_INVALID, "warped read: null job accepted");
    EXPECT(rd(ctx, &dj, 4, 8, nullptr, 3, 5, 2, 0, 0.0, 0.0, inf) == FRA_E_INVALID, "warped read: null map accepted");
    EXPECT(rd(ctx, &dj, 4, 8, &id, 3, 5, 2, 0, 0.0, 0.0, nullptr) == FRA_E_INVALID, "warped read: null infos accepted");
    EXPECT(says(rd(ctx, &dj, 4, 8, &id, 0, 5, 2, 0, 0.0, 0.0, inf), "output size"), "warped read: out height 0: %s", g_msg.c_str());
    EXPECT(says(rd(ctx, &dj, 4, 8, &id, 3, 5, 1, 0, 0.0, 0.0, inf), "point samples"), "warped read: average: %s", g_msg.c_str());
    EXPECT(says(rd(ctx, &dj, 4, 8, &id, 3, 5, 2, 4, 0.0, 0.0, inf), "unknown warp flags"), "warped read: flag 4: %s", g_msg.c_str());
    EXPECT(says(rd(ctx, &dj, 4, 8, &gj.map, 3, 7, 2, 0, 0.0, 0.0, inf), "takes a grid of"), "warped read: a grid for another size: %s", g_msg.c_str());
    EXPECT(says(rd(ctx, &dj, 0, 8, &id, 3, 5, 2, 0, 0.0, 0.0, inf), "bad raster size"), "warped read: raster height 0: %s", g_msg.c_str());
    EXPECT(says(rd(ctx, &dj, 4, 8, &id, 3, 5, 2, 1, 0.5, 0.0, inf), "nodata"), "warped read: nodata 0.5: %s", g_msg.c_str());
    EXPECT(says(rd(ctx, &dj, 4, 8, &id, 3, 5, 2, 0, 0.0, 0.5, inf), "fill"), "warped read: fill 0.5: %s", g_msg.c_str());
    EXPECT(says(rd(ctx, &dj, 9, 8, &id, 3, 5, 2, 0, 0.0, 0.0, inf), "do not cover"), "warped read: a window of six rows over an item of four: %s", g_msg.c_str());
    { auto j = dj; j.dst_dtype = 9; EXPECT(says(rd(ctx, &j, 4, 8, &id, 3, 5, 2, 0, 0.0, 0.5, inf), "dtype"), "warped read: dtype 9 and fill 0.5: %s", g_msg.c_str()); }
    { auto j = dj; j.dst = nullptr; EXPECT(rd(ctx, &j, 4, 8, &id, 3, 5, 2, 0, 0.0, 0.0, inf) == FRA_E_INVALID, "warped read: null dst accepted"); }
    { auto j = dj; j.flags = FRA_DECODE_CONCAT; EXPECT(rd(ctx, &j, 4, 8, &id, 3, 5, 2, 0, 0.0, 0.0, inf) == FRA_E_INVALID, "warped read: FRA_DECODE_CONCAT accepted"); }
    { auto j = dj; j.channels = 0; EXPECT(rd(ctx, &j, 4, 8, &id, 3, 5, 2, 0, 0.0, 0.0, inf) == FRA_E_INVALID, "warped read: no channels accepted"); }
    { auto j = dj; j.row_stride = -1; fra_warp_map out = id; out.affine[2] = 100.0;  // nothing to decode: the job is still checked
      EXPECT(rd(ctx, &j, 4, 8, &out, 3, 5, 2, 0, 0.0, 0.0, inf) == FRA_E_INVALID, "warped read: negative stride with a map that misses the raster accepted"); }
    // the source window
    fra_window win{};
    EXPECT(fra_warp_source_window(nullptr, 4, 8, 3, 5, &win) == FRA_E_INVALID, "source window: null map accepted");
    EXPECT(fra_warp_source_window(&id, 4, 8, 3, 5, nullptr) == FRA_E_INVALID, "source window: null window accepted");
    EXPECT(says(fra_warp_source_window(&id, 4, 8, 0, 5, &win), "output size"), "source window: out height 0: %s", g_msg.c_str());
    EXPECT(says(fra_warp_source_window(&id, 0, 8, 3, 5, &win), "bad raster size"), "source window: raster height 0: %s", g_msg.c_str());
    auto window_is = [&](const fra_warp_map& m, int32_t H, int32_t W, int32_t oh, int32_t ow, int r, int c, int h, int w) {
      fra_window x{-1, -1, -1, -1};
      return fra_warp_source_window(&m, H, W, oh, ow, &x) == 1 && x.row_off == r && x.col_off == c && x.height == h && x.width == w;
    };
    auto misses = [&](const fra_warp_map& m, int32_t H, int32_t W, int32_t oh, int32_t ow) {
      fra_window x{-1, -1, -1, -1};
      return fra_warp_source_window(&m, H, W, oh, ow, &x) == 0 && x.row_off == -1;
    };
    auto affine = [&](double a, double b, double c, double d, double e, double f) {
      fra_warp_map m{};
      m.kind = FRA_WARP_AFFINE;
      const double k[6] = {a, b, c, d, e, f};
      memcpy(m.affine, k, sizeof(k));
      return m;
    };
    EXPECT(window_is(id, 300, 500, 300, 500, 0, 0, 300, 500), "source window: the identity is not the raster");
    EXPECT(window_is(id, 9, 8, 3, 5, 0, 0, 6, 8), "source window: the identity of 3 x 5 over 9 x 8");
    EXPECT(window_is(affine(1, 0, 100, 0, 1, 50), 300, 500, 10, 20, 47, 97, 16, 26), "source window: a shift by (100, 50)");
    EXPECT(window_is(affine(1, 0, -2.5, 0, 1, 0), 300, 500, 5, 3, 0, 0, 8, 4), "source window: a shift that leaves one column inside");
    EXPECT(misses(affine(1, 0, -4.5, 0, 1, 0), 300, 500, 5, 3), "source window: two pixels left of the raster");
    EXPECT(window_is(affine(1, 0, 0, 0, 1, 299.75), 300, 500, 7, 7, 297, 0, 3, 10), "source window: within a pixel below the raster");
    EXPECT(misses(affine(1, 0, 0, 0, 1, 300.5), 300, 500, 7, 7), "source window: a pixel below the raster");
    EXPECT(misses(affine(1, 0, 600, 0, 1, 0), 300, 500, 5, 5), "source window: right of the raster");
    EXPECT(misses(affine(1, 0, 0, 0, 1, -50), 300, 500, 9, 9), "source window: above the raster");
    EXPECT(window_is(affine(1e6, 0, -1e9, 0, 1e6, -1e9), 300, 500, 65536, 65536, 0, 0, 300, 500), "source window: a huge footprint is clipped");
    {  // a grid: the nodes' hull; non-finite nodes are left out; none finite misses
      double gx[12], gy[12];
      for (int i = 0; i < 3; i++)
        for (int k = 0; k < 4; k++) gx[i * 4 + k] = 10.0 + 2.5 * k, gy[i * 4 + k] = 20.0 + 1.5 * i;
      fra_warp_map g = gj.map;
      g.gx = gx; g.gy = gy;
      EXPECT(window_is(g, 300, 500, 3, 5, 17, 7, 10, 14), "source window: a grid's hull");
      gx[5] = NAN; gy[0] = HUGE_VAL; gx[11] = 4000.0; gy[11] = NAN;
      EXPECT(window_is(g, 300, 500, 3, 5, 17, 7, 10, 14), "source window: non-finite nodes are left out");
      for (double& v : gx) v = NAN;
      EXPECT(misses(g, 300, 500, 3, 5), "source window: no finite node");
    }
    // every tap of every inside pixel lies in the window: rotations and scales about the raster, the cubic's reach
    for (int deg = 0; deg < 360; deg += 17)
      for (double scale : {0.3, 1.0, 1.9, 7.5}) {
        const int H = 300, W = 500, oh = 70, ow = 300;
        const double c = scale * std::cos(deg * M_PI / 180.0), s = scale * std::sin(deg * M_PI / 180.0);
        const fra_warp_map m = affine(c, -s, 250.0 - (c * 150 - s * 35), s, c, 150.0 - (s * 150 + c * 35));
        fra_window x{};
        const int rc = fra_warp_source_window(&m, H, W, oh, ow, &x);
        bool ok = rc == 0 || (rc == 1 && x.row_off >= 0 && x.col_off >= 0 && x.height >= 1 && x.width >= 1 && x.row_off + x.height <= H && x.col_off + x.width <= W);
        for (int R = 0; R < oh && ok; R++)
          for (int C = 0; C < ow && ok; C++) {
            const double u = C + 0.5, v = R + 0.5;
            const double px = (m.affine[0] * u + m.affine[1] * v) + m.affine[2], py = (m.affine[3] * u + m.affine[4] * v) + m.affine[5];
            if (!(px >= 0 && px < W && py >= 0 && py < H)) continue;
            const int i0 = (int)std::floor(px - 0.5), j0 = (int)std::floor(py - 0.5);
            ok = rc == 1 && std::max(i0 - 1, 0) >= x.col_off && std::min(i0 + 2, W - 1) < x.col_off + x.width &&
                 std::max(j0 - 1, 0) >= x.row_off && std::min(j0 + 2, H - 1) < x.row_off + x.height;
          }
        EXPECT(ok, "source window: rotation %d, scale %g: a tap lies outside (%d, %d, %d x %d)", deg, scale, x.row_off, x.col_off, x.height, x.width);
      }
  }
  // ... and of the polygon rasterizer (fra_rasterize.hip): refused before any GPU work, in the order the header gives
  {
    auto says = [&](int rc, const char* what) { return rc == FRA_E_INVALID && g_msg.find(what) != std::string::npos; };
    // feature 0: a square with a repeated closing vertex; feature 1: a triangle and a second ring
    const double xy[] = {1, 1, 9, 1, 9, 9, 1, 9, 1, 1, /**/ 2, 20, 30, 22, 4, 40, /**/ 10, 3, 12, 3, 11, 5};
    const int64_t ring_start[] = {0, 5, 8, 11}, feat_start[] = {0, 1, 3}, values[] = {7, -2};
    int16_t rout[48 * 40];
    uint64_t burned = 99;
    fra_rasterize_job rj{};
    rj.xy = xy; rj.nverts = 11; rj.ring_start = ring_start; rj.nrings = 3; rj.feature_ring_start = feat_start; rj.nfeatures = 2;
    rj.values = values; rj.dtype = FRA_I16; rj.height = 48; rj.width = 40; rj.fill = -1;
    rj.dst = rout; rj.row_stride = 40; rj.col_stride = 1;
    EXPECT(fra_rasterize(nullptr, &rj, &burned) == FRA_E_INVALID, "rasterize: null ctx accepted");
    EXPECT(fra_rasterize(ctx, nullptr, &burned) == FRA_E_INVALID, "rasterize: null job accepted");
    { auto j = rj; j.dst = nullptr; EXPECT(says(fra_rasterize(ctx, &j, &burned), "null argument"), "rasterize: null dst: %s", g_msg.c_str()); }
    { auto j = rj; j.xy = nullptr; EXPECT(says(fra_rasterize(ctx, &j, &burned), "null argument"), "rasterize: null xy: %s", g_msg.c_str()); }
    { auto j = rj; j.ring_start = nullptr; EXPECT(says(fra_rasterize(ctx, &j, &burned), "null argument"), "rasterize: null ring_start: %s", g_msg.c_str()); }
    { auto j = rj; j.feature_ring_start = nullptr; EXPECT(says(fra_rasterize(ctx, &j, &burned), "null argument"), "rasterize: null feature_ring_start: %s", g_msg.c_str()); }
    { auto j = rj; j.values = nullptr; EXPECT(says(fra_rasterize(ctx, &j, &burned), "null argument"), "rasterize: null values: %s", g_msg.c_str()); }
    for (int d : {-1, (int)FRA_F32, (int)FRA_F64, 8}) { auto j = rj; j.dtype = d; EXPECT(says(fra_rasterize(ctx, &j, &burned), "bad output dtype"), "rasterize: dtype %d: %s", d, g_msg.c_str()); }
    for (int n : {0, -3, 65537}) {
      { auto j = rj; j.height = n; EXPECT(says(fra_rasterize(ctx, &j, &burned), "output size"), "rasterize: height %d: %s", n, g_msg.c_str()); }
      { auto j = rj; j.width = n; EXPECT(says(fra_rasterize(ctx, &j, &burned), "output size"), "rasterize: width %d: %s", n, g_msg.c_str()); }
    }
    { auto j = rj; j.row_stride = -40; EXPECT(says(fra_rasterize(ctx, &j, &burned), "bad output layout"), "rasterize: negative row stride: %s", g_msg.c_str()); }
    { auto j = rj; j.col_stride = -1; EXPECT(says(fra_rasterize(ctx, &j, &burned), "bad output layout"), "rasterize: negative column stride: %s", g_msg.c_str()); }
    { auto j = rj; j.nfeatures = -1; EXPECT(says(fra_rasterize(ctx, &j, &burned), "bad geometry tables"), "rasterize: -1 features: %s", g_msg.c_str()); }
    { auto j = rj; j.nrings = -1; EXPECT(says(fra_rasterize(ctx, &j, &burned), "bad geometry tables"), "rasterize: -1 rings: %s", g_msg.c_str()); }
    { auto j = rj; j.nverts = -1; EXPECT(says(fra_rasterize(ctx, &j, &burned), "bad geometry tables"), "rasterize: -1 vertices: %s", g_msg.c_str()); }
    { auto j = rj; j.nfeatures = 0; EXPECT(says(fra_rasterize(ctx, &j, &burned), "rings of no feature"), "rasterize: rings without features: %s", g_msg.c_str()); }
    { const int64_t fs[] = {0, 2, 1}; auto j = rj; j.feature_ring_start = fs; EXPECT(says(fra_rasterize(ctx, &j, &burned), "feature_ring_start"), "rasterize: descending feature table: %s", g_msg.c_str()); }
    { const int64_t fs[] = {1, 1, 3}; auto j = rj; j.feature_ring_start = fs; EXPECT(says(fra_rasterize(ctx, &j, &burned), "feature_ring_start"), "rasterize: feature table from 1: %s", g_msg.c_str()); }
    { const int64_t fs[] = {0, 1, 2}; auto j = rj; j.feature_ring_start = fs; EXPECT(says(fra_rasterize(ctx, &j, &burned), "feature_ring_start"), "rasterize: feature table short of the rings: %s", g_msg.c_str()); }
    { const int64_t rs[] = {0, 8, 5, 11}; auto j = rj; j.ring_start = rs; EXPECT(says(fra_rasterize(ctx, &j, &burned), "ring_start"), "rasterize: descending ring table: %s", g_msg.c_str()); }
    { const int64_t rs[] = {0, 5, 8, 12}; auto j = rj; j.ring_start = rs; EXPECT(says(fra_rasterize(ctx, &j, &burned), "ring_start"), "rasterize: rings past the vertices: %s", g_msg.c_str()); }
    { const int64_t rs[] = {0, 5, 9, 11}; auto j = rj; j.ring_start = rs; EXPECT(says(fra_rasterize(ctx, &j, &burned), "ring 2 has 2 vertices"), "rasterize: a ring of 2: %s", g_msg.c_str()); }
    { const int64_t rs[] = {0, 5, 5, 11}; auto j = rj; j.ring_start = rs; EXPECT(says(fra_rasterize(ctx, &j, &burned), "ring 1 has 0 vertices"), "rasterize: an empty ring: %s", g_msg.c_str()); }
    for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY, 9007199254740992.0, -4503599627370497.0}) {
      double v[22]; memcpy(v, xy, sizeof(v)); v[13] = bad;
      auto j = rj; j.xy = v; EXPECT(says(fra_rasterize(ctx, &j, &burned), "coordinate 13"), "rasterize: coordinate %g: %s", bad, g_msg.c_str());
    }
    { const int64_t v[] = {7, 32768}; auto j = rj; j.values = v; EXPECT(says(fra_rasterize(ctx, &j, &burned), "burn value 32768 of feature 1"), "rasterize: burn 32768 in int16: %s", g_msg.c_str()); }
    { auto j = rj; j.dtype = FRA_U8; EXPECT(says(fra_rasterize(ctx, &j, &burned), "burn value -2"), "rasterize: burn -2 in uint8: %s", g_msg.c_str()); }
    { auto j = rj; j.fill = -32769; EXPECT(says(fra_rasterize(ctx, &j, &burned), "fill -32769"), "rasterize: fill -32769 in int16: %s", g_msg.c_str()); }
    { auto j = rj; j.dtype = FRA_U32; j.fill = (int64_t)1 << 32; const int64_t v[] = {7, 4294967295ll}; j.values = v; EXPECT(says(fra_rasterize(ctx, &j, &burned), "fill 4294967296"), "rasterize: fill 2^32 in uint32: %s", g_msg.c_str()); }
    {  // more than 2^24 features: empty ones, the tables are still walked
      std::vector<int64_t> fs((size_t)(1 << 24) + 2, 0), vs((size_t)(1 << 24) + 1, 1);
      auto j = rj; j.nfeatures = (1 << 24) + 1; j.nrings = 0; j.nverts = 0; j.feature_ring_start = fs.data(); j.values = vs.data();
      EXPECT(says(fra_rasterize(ctx, &j, &burned), "2^24"), "rasterize: 2^24 + 1 features: %s", g_msg.c_str());
    }
    { auto j = rj; j.nverts = ((int64_t)1 << 28) + 1; EXPECT(says(fra_rasterize(ctx, &j, &burned), "2^28"), "rasterize: 2^28 + 1 vertices: %s", g_msg.c_str()); }
    // the order: an input that breaks two rules gets the message of the first
    { auto j = rj; j.dtype = 8; j.height = 0; EXPECT(says(fra_rasterize(ctx, &j, &burned), "bad output dtype"), "rasterize: dtype 8 and height 0: %s", g_msg.c_str()); }
    { auto j = rj; j.width = 0; j.col_stride = -1; EXPECT(says(fra_rasterize(ctx, &j, &burned), "output size"), "rasterize: width 0 and a negative stride: %s", g_msg.c_str()); }
    { auto j = rj; j.row_stride = -1; j.nrings = -1; EXPECT(says(fra_rasterize(ctx, &j, &burned), "bad output layout"), "rasterize: a negative stride and -1 rings: %s", g_msg.c_str()); }
    { const int64_t rs[] = {0, 5, 9, 11}; double v[22]; memcpy(v, xy, sizeof(v)); v[0] = NAN; auto j = rj; j.ring_start = rs; j.xy = v; EXPECT(says(fra_rasterize(ctx, &j, &burned), "ring 2 has 2"), "rasterize: a ring of 2 and a NaN: %s", g_msg.c_str()); }
    { double v[22]; memcpy(v, xy, sizeof(v)); v[3] = NAN; auto j = rj; j.xy = v; j.fill = 1 << 20; EXPECT(says(fra_rasterize(ctx, &j, &burned), "coordinate 3"), "rasterize: a NaN and a fill out of range: %s", g_msg.c_str()); }
    { const int64_t v[] = {70000, 1}; auto j = rj; j.values = v; j.fill = 1 << 20; EXPECT(says(fra_rasterize(ctx, &j, &burned), "burn value 70000"), "rasterize: a burn value and a fill out of range: %s", g_msg.c_str()); }
    EXPECT(burned == 99, "rasterize: a refusal wrote the burned count");
    EXPECT(fra_rasterize_timing(nullptr) == FRA_E_INVALID, "rasterize timing: null accepted");
    // the edge table: rings closed on their first vertex, level edges and the one of no length dropped, y0 < y1
    EXPECT(fra_rz::check_job(&rj) == FRA_OK, "rasterize: the sample job is refused: %s", g_msg.c_str());
    std::vector<fra_rz::Edge> edges;
    std::vector<int32_t> feat;
    fra_rz::build_edges(&rj, &edges, &feat);
    // the square: 2 level edges and the closing one dropped -> 2; the triangle 3; the small ring: 1 level -> 2
    EXPECT(edges.size() == 7 && feat == std::vector<int32_t>({0, 0, 1, 1, 1, 1, 1}), "rasterize: %zu edges", edges.size());
    bool oriented = true;
    for (const auto& e : edges) oriented = oriented && e.y0 < e.y1;
    EXPECT(oriented, "rasterize: an edge is not oriented");
    EXPECT(edges.size() == 7 && edges[0].x0 == 9 && edges[0].y0 == 1 && edges[0].y1 == 9 && edges[1].x0 == 1 && edges[1].y0 == 1 && edges[1].x1 == 1 && edges[1].y1 == 9,
           "rasterize: the square's edges");  // (9,1)->(9,9) as it is, (1,9)->(1,1) turned
    EXPECT(edges.size() == 7 && edges[2].x0 == 2 && edges[2].y1 == 22 && edges[4].x0 == 2 && edges[4].y0 == 20 && edges[4].x1 == 4 && edges[4].y1 == 40,
           "rasterize: the triangle's edges");  // (2,20)->(30,22) as it is, (4,40)->(2,20) turned
    std::vector<fra_rz::Extent> ext;
    fra_rz::extents(edges, feat, 2, &ext);
    EXPECT(ext.size() == 2 && ext[0].lo <= 1 && ext[0].lo > 0.999 && ext[0].hi >= 9 && ext[0].hi < 9.001 && ext[1].lo <= 2 && ext[1].hi >= 30,
           "rasterize: extents");
    { std::vector<fra_rz::Extent> none; fra_rz::extents({}, {}, 1, &none); EXPECT(none.size() == 1 && none[0].lo > none[0].hi, "rasterize: the extent of a feature without edges"); }
    // the band lists of a 48-row window: band 0 (rows 0..15) the square and the small ring, band 1 the triangle,
    // band 2 the triangle's lower part; from row 16 on a window of 16 rows holds the triangle alone
    fra_rz::Bins bins;
    EXPECT(fra_rz::bin_edges(edges, feat, 0, 48, &bins) == FRA_OK && bins.band_start.size() == 4, "rasterize: bins");
    EXPECT(bins.band_start == std::vector<uint32_t>({0, 4, 7, 9}), "rasterize: band starts %u %u %u %u", bins.band_start[0], bins.band_start[1], bins.band_start[2], bins.band_start[3]);
    EXPECT(bins.feat == std::vector<int32_t>({0, 0, 1, 1, 1, 1, 1, 1, 1}), "rasterize: the features of the band lists");
    fra_rz::Bins empty;  // below every edge: bands without an edge
    EXPECT(fra_rz::bin_edges(edges, feat, 48, 40, &empty) == FRA_OK && empty.band_start == std::vector<uint32_t>({0, 0, 0, 0}), "rasterize: empty bands");
    {  // a feature that spans all the bands of a tall window is in every list once per edge, and keeps its place
      const double tall[] = {5, -10, 8, 5000, 2, 4000, /**/ 3, 100, 6, 100, 4, 120};
      const int64_t rs[] = {0, 3, 6}, fs[] = {0, 1, 2}, vs[] = {1, 2};
      fra_rasterize_job tj = rj;
      tj.xy = tall; tj.nverts = 6; tj.ring_start = rs; tj.nrings = 2; tj.feature_ring_start = fs; tj.values = vs; tj.height = 330;
      fra_rz::Prepared p;
      EXPECT(fra_rz::check_job(&tj) == FRA_OK && fra_rz::prepare(&tj, &p) == FRA_OK, "rasterize: the tall job: %s", g_msg.c_str());
      const size_t nb = (330 + 15) / 16;
      bool ok = p.bins.band_start.size() == nb + 1 && p.values == std::vector<uint32_t>({1, 2});
      for (size_t b = 0; b < nb && ok; b++) {
        const uint32_t a = p.bins.band_start[b], z = p.bins.band_start[b + 1];
        // (5,-10)-(8,5000) and (5,-10)-(2,4000) cross every row of the window; the small triangle rows 100 .. 119
        const uint32_t want = 2 + ((b == 6 || b == 7) ? 2 : 0);
        ok = z - a == want && p.bins.feat[a] == 0 && p.bins.feat[a + 1] == 0 && (want == 2 || (p.bins.feat[a + 2] == 1 && p.bins.feat[a + 3] == 1));
      }
      EXPECT(ok, "rasterize: the lists of a feature that spans all bands");
    }
    {  // every crossing of the rule is in its row's band list, for windows at several offsets
      bool ok = true;
      for (int64_t off : {(int64_t)0, (int64_t)3, (int64_t)17, (int64_t)-5})
        for (int32_t hh : {1, 16, 17, 45}) {
          fra_rz::Bins b;
          ok = ok && fra_rz::bin_edges(edges, feat, off, hh, &b) == FRA_OK;
          for (int32_t r = 0; r < hh && ok; r++) {
            const double yc = (double)(off + r) + 0.5;
            std::vector<int> want, got;
            for (size_t k = 0; k < edges.size(); k++) if (edges[k].y0 <= yc && yc < edges[k].y1) want.push_back((int)k);
            for (uint32_t k = b.band_start[(size_t)r / 16]; k < b.band_start[(size_t)r / 16 + 1]; k++)
              if (b.edges[k].y0 <= yc && yc < b.edges[k].y1)
                for (size_t q = 0; q < edges.size(); q++) if (!memcmp(&edges[q], &b.edges[k], sizeof(fra_rz::Edge)) && feat[q] == b.feat[k]) { got.push_back((int)q); break; }
            ok = want == got;
          }
        }
      EXPECT(ok, "rasterize: a crossing is missing from its band list, or out of order");
    }
  }
  // ... and of the proximity unit (fra_proximity.hip): refused before any GPU work, in the order the header gives
  {
    auto says = [&](int rc, const char* what) { return rc == FRA_E_INVALID && g_msg.find(what) != std::string::npos; };
    static uint8_t psrc[3 * 40 * 50];
    static float pdist[3 * 40 * 50];
    static uint8_t palloc[3 * 40 * 50];
    uint64_t counts[3] = {9, 9, 9};
    fra_proximity_job pj{};
    pj.src = psrc; pj.dtype = FRA_U8; pj.channels = 3; pj.height = 40; pj.width = 50;
    pj.band_stride = 2000; pj.row_stride = 50; pj.col_stride = 1;
    pj.opts.scale = 1.0; pj.opts.out_height = 40; pj.opts.out_width = 50;
    pj.opts.dist.dst = pdist; pj.opts.dist.dtype = FRA_F32; pj.opts.dist.band_stride = 2000; pj.opts.dist.row_stride = 50; pj.opts.dist.col_stride = 1;
    pj.opts.alloc.dst = palloc; pj.opts.alloc.band_stride = 2000; pj.opts.alloc.row_stride = 50; pj.opts.alloc.col_stride = 1;
    const fra_region::Strides pss{2000, 50, 1};
    EXPECT(fra_px::check_job(FRA_U8, 3, 40, 50, pss, &pj.opts) == FRA_OK, "proximity: the sample job is refused: %s", g_msg.c_str());
    EXPECT(fra_proximity(nullptr, &pj, counts) == FRA_E_INVALID, "proximity: null ctx accepted");
    EXPECT(fra_proximity(ctx, nullptr, counts) == FRA_E_INVALID, "proximity: null job accepted");
    { auto j = pj; j.src = nullptr; EXPECT(says(fra_proximity(ctx, &j, counts), "null argument"), "proximity: null src: %s", g_msg.c_str()); }
    for (int d : {-1, 8}) { auto j = pj; j.dtype = d; EXPECT(says(fra_proximity(ctx, &j, counts), "bad dtype"), "proximity: dtype %d: %s", d, g_msg.c_str()); }
    { auto j = pj; j.channels = 0; EXPECT(says(fra_proximity(ctx, &j, counts), "bad raster layout"), "proximity: no band: %s", g_msg.c_str()); }
    { auto j = pj; j.channels = 256; EXPECT(says(fra_proximity(ctx, &j, counts), "more than 255"), "proximity: 256 bands: %s", g_msg.c_str()); }
    { auto j = pj; j.row_stride = -50; EXPECT(says(fra_proximity(ctx, &j, counts), "bad raster layout"), "proximity: negative source stride: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.dist.dtype = 8; EXPECT(says(fra_proximity(ctx, &j, counts), "bad dist dtype"), "proximity: dist dtype 8: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.dist.col_stride = -1; EXPECT(says(fra_proximity(ctx, &j, counts), "bad dist layout"), "proximity: negative dist stride: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.alloc.band_stride = -1; EXPECT(says(fra_proximity(ctx, &j, counts), "bad alloc layout"), "proximity: negative alloc stride: %s", g_msg.c_str()); }
    for (int n : {0, -3, 32769}) {
      { auto j = pj; j.height = n; EXPECT(says(fra_proximity(ctx, &j, counts), "1 .. 32768"), "proximity: height %d: %s", n, g_msg.c_str()); }
      { auto j = pj; j.width = n; EXPECT(says(fra_proximity(ctx, &j, counts), "1 .. 32768"), "proximity: width %d: %s", n, g_msg.c_str()); }
    }
    for (int n : {-1, 17}) { auto j = pj; j.opts.nvalues = n; EXPECT(says(fra_proximity(ctx, &j, counts), "nvalues"), "proximity: %d values: %s", n, g_msg.c_str()); }
    for (double v : {(double)NAN, (double)INFINITY}) { auto j = pj; j.opts.nvalues = 2; j.opts.values[1] = v; EXPECT(says(fra_proximity(ctx, &j, counts), "target value 1 is not finite"), "proximity: value %g: %s", v, g_msg.c_str()); }
    for (double v : {0.0, -1.0, (double)NAN, (double)INFINITY}) { auto j = pj; j.opts.scale = v; EXPECT(says(fra_proximity(ctx, &j, counts), "scale"), "proximity: scale %g: %s", v, g_msg.c_str()); }
    for (double v : {-0.5, (double)NAN}) { auto j = pj; j.opts.has_max_dist = 1; j.opts.max_dist = v; EXPECT(says(fra_proximity(ctx, &j, counts), "max_dist"), "proximity: max_dist %g: %s", v, g_msg.c_str()); }
    { auto o = pj.opts; o.max_dist = NAN; EXPECT(fra_px::check_job(FRA_U8, 3, 40, 50, pss, &o) == FRA_OK, "proximity: max_dist looked at without has_max_dist"); }
    { auto o = pj.opts; o.has_max_dist = 1; o.max_dist = INFINITY; EXPECT(fra_px::check_job(FRA_U8, 3, 40, 50, pss, &o) == FRA_OK, "proximity: an infinite max_dist refused"); }
    { auto j = pj; j.opts.out_height = 0; EXPECT(says(fra_proximity(ctx, &j, counts), "output window"), "proximity: empty window: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.out_col_off = 1; EXPECT(says(fra_proximity(ctx, &j, counts), "output window"), "proximity: window past the right edge: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.out_row_off = -1; EXPECT(says(fra_proximity(ctx, &j, counts), "output window"), "proximity: negative window offset: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.dist.dst = nullptr; j.opts.alloc.dst = nullptr; EXPECT(says(fra_proximity(ctx, &j, counts), "neither dist nor alloc"), "proximity: no output: %s", g_msg.c_str()); }
    // two rules broken at once: the message of the first
    { auto j = pj; j.dtype = 8; j.height = 0; EXPECT(says(fra_proximity(ctx, &j, counts), "bad dtype"), "proximity: dtype 8 and height 0: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.dist.dtype = -1; j.width = 40000; EXPECT(says(fra_proximity(ctx, &j, counts), "bad dist dtype"), "proximity: dist dtype and width: %s", g_msg.c_str()); }
    { auto j = pj; j.height = 0; j.opts.nvalues = 17; EXPECT(says(fra_proximity(ctx, &j, counts), "1 .. 32768"), "proximity: height 0 and 17 values: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.nvalues = 17; j.opts.scale = 0.0; EXPECT(says(fra_proximity(ctx, &j, counts), "nvalues"), "proximity: 17 values and scale 0: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.scale = 0.0; j.opts.has_max_dist = 1; j.opts.max_dist = -1.0; EXPECT(says(fra_proximity(ctx, &j, counts), "scale"), "proximity: scale 0 and max_dist -1: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.has_max_dist = 1; j.opts.max_dist = -1.0; j.opts.out_width = 0; EXPECT(says(fra_proximity(ctx, &j, counts), "max_dist"), "proximity: max_dist -1 and an empty window: %s", g_msg.c_str()); }
    { auto j = pj; j.opts.out_width = 0; j.opts.dist.dst = nullptr; j.opts.alloc.dst = nullptr; EXPECT(says(fra_proximity(ctx, &j, counts), "output window"), "proximity: an empty window and no output: %s", g_msg.c_str()); }
    EXPECT(counts[0] == 9 && counts[1] == 9 && counts[2] == 9, "proximity: a refusal wrote the counts");
    EXPECT(fra_proximity_timing(nullptr) == FRA_E_INVALID, "proximity timing: null accepted");
    // the read over a region: what the windowed read refuses is referred to it; the options as above
    {
      fra_decode_item di = it;
      di.window = {0, 0, 4, 8};
      fra_decode_job dj = job;
      dj.items = &di;
      const fra_window r48{0, 0, 4, 8};
      fra_window r40 = r48;
      r40.width = 0;
      auto o = pj.opts;
      o.out_height = 4; o.out_width = 8;
      EXPECT(fra_decode_device_proximity(ctx, &dj, &r48, nullptr, inf, counts) == FRA_E_INVALID && g_msg == "null argument", "proximity read: null options: %s", g_msg.c_str());
      EXPECT(fra_decode_device_proximity(ctx, &dj, nullptr, &o, inf, counts) == FRA_E_INVALID, "proximity read: null roi accepted");
      EXPECT(says(fra_decode_device_proximity(ctx, &dj, &r40, &o, inf, counts), "region of interest"), "proximity read: zero-width roi: %s", g_msg.c_str());
      { auto q = o; q.scale = 0.0; EXPECT(says(fra_decode_device_proximity(ctx, &dj, &r40, &q, inf, counts), "region of interest"), "proximity read: zero-width roi and scale 0: %s", g_msg.c_str()); }
      { auto q = o; q.scale = 0.0; EXPECT(says(fra_decode_device_proximity(ctx, &dj, &r48, &q, inf, counts), "scale"), "proximity read: scale 0: %s", g_msg.c_str()); }
      { auto q = o; q.out_width = 9; EXPECT(says(fra_decode_device_proximity(ctx, &dj, &r48, &q, inf, counts), "output window"), "proximity read: window past the region: %s", g_msg.c_str()); }
      { fra_window r = r48; r.height = 5; auto q = o; q.out_height = 5; EXPECT(says(fra_decode_device_proximity(ctx, &dj, &r, &q, inf, counts), "do not cover"), "proximity read: uncovered row: %s", g_msg.c_str()); }
    }
    // the reach threshold against the f64 predicate, at and around perfect squares
    for (double scale : {1.0, 0.1, 10.0, 30.0}) {
      bool ok = true;
      for (int64_t k : {0, 1, 2, 3, 7, 100, 1000, 12345, 32767, 46339})
        for (int64_t off : {-2, -1, 0, 1, 2}) {
          const int64_t d2 = k * k + off;
          if (d2 < 0 || d2 > fra_px::kMaxD2) continue;
          const double md = std::sqrt((double)d2) * scale;  // exactly the distance of d2: d2 is within reach, d2 + 1 is not
          const int64_t t = fra_px::reach_threshold(true, scale, md);
          ok = ok && t == d2 && fra_px::within(t, scale, md) && (t == fra_px::kMaxD2 || !fra_px::within(t + 1, scale, md));
          const double below = std::nextafter(md, 0.0);
          if (d2 > 0) ok = ok && fra_px::reach_threshold(true, scale, below) == d2 - 1;
          const int64_t ta = fra_px::reach_threshold(true, scale, (double)k * scale);  // a radius of k pixels
          ok = ok && fra_px::within(ta, scale, (double)k * scale) && (ta == fra_px::kMaxD2 || !fra_px::within(ta + 1, scale, (double)k * scale));
        }
      EXPECT(ok, "proximity: the reach threshold disagrees with the predicate at scale %g", scale);
    }
    EXPECT(fra_px::reach_threshold(false, 1.0, 0.0) == fra_px::kMaxD2 && fra_px::reach_threshold(true, 1.0, INFINITY) == fra_px::kMaxD2, "proximity: no limit");
    EXPECT(fra_px::reach_threshold(true, 1.0, 0.0) == 0 && fra_px::reach_threshold(true, 30.0, 29.0) == 0 && fra_px::reach_threshold(true, 1.0, 5.0) == 25, "proximity: pinned thresholds");
    EXPECT(fra_px::isqrt(0) == 0 && fra_px::isqrt(24) == 4 && fra_px::isqrt(25) == 5 && fra_px::isqrt(fra_px::kMaxD2) == 46339, "proximity: isqrt");
    // the fills as the output holds them
    EXPECT(fra_px::out_bits(FRA_F32, NAN) == 0x7fc00000u && fra_px::out_bits(FRA_F64, -NAN) == 0x7ff8000000000000ull, "proximity: a NaN fill");
    EXPECT(fra_px::out_bits(FRA_U8, 300.0) == 255 && fra_px::out_bits(FRA_U8, -3.0) == 0 && fra_px::out_bits(FRA_I8, -7.0) == 0xf9 && fra_px::out_bits(FRA_U16, 2.5) == 2 &&
               fra_px::out_bits(FRA_U16, 3.5) == 4 && fra_px::out_bits(FRA_I32, NAN) == 0 && fra_px::out_bits(FRA_I16, -1e9) == 0x8000, "proximity: integer fills");
    // the launch plan
    {
      struct Case { int32_t h, w, r0, c0, oh, ow; };
      const Case cases[] = {{1, 1, 0, 0, 1, 1}, {7, 19, 0, 0, 7, 19}, {200, 70, 60, 3, 75, 60}, {130, 517, 17, 29, 90, 333}, {9, 512, 0, 0, 9, 512},
                            {9, 513, 0, 0, 9, 513}, {3, 32768, 0, 0, 3, 32768}, {32768, 3, 0, 0, 32768, 3}, {10980, 10980, 0, 0, 10980, 10980}};
      for (const Case& c : cases) {
        fra_proximity_opts o{};
        o.out_row_off = c.r0; o.out_col_off = c.c0; o.out_height = c.oh; o.out_width = c.ow;
        const fra_px::Plan p = fra_px::make_plan(c.h, c.w, o);
        bool ok = (int64_t)p.nchunks * 64 >= c.h && (int64_t)(p.nchunks - 1) * 64 < c.h && p.k0 * 64 <= c.r0 && c.r0 < (p.k0 + 1) * 64 &&
                  p.k1 * 64 <= c.r0 + c.oh - 1 && c.r0 + c.oh - 1 < (p.k1 + 1) * 64 && p.k1 < p.nchunks &&
                  (int64_t)p.col_blocks * 256 >= c.w && (int64_t)(p.col_blocks - 1) * 256 < c.w;
        ok = ok && p.rows_per_wg * p.team_threads == 256 && p.team_threads % 64 == 0 && (p.rows_per_wg == 4) == (c.w <= 512) &&
             (int64_t)p.row_wgs * p.rows_per_wg >= c.oh && (int64_t)(p.row_wgs - 1) * p.rows_per_wg < c.oh;
        ok = ok && (1 << (p.levels - 1)) <= c.ow && c.ow < (1ll << p.levels);
        // every output pixel belongs to exactly one level
        int64_t pixels = 0;
        for (int L = 0; L < p.levels; L++) pixels += (c.ow / (1 << (p.levels - 1 - L)) + 1) / 2;
        ok = ok && pixels == c.ow;
        ok = ok && p.opt_off >= 2u * (uint32_t)c.w && p.queue_off >= p.opt_off + 2u * (uint32_t)c.ow && p.count_off >= p.queue_off + 2u * p.queue_cap &&
             p.opt_off % 4 == 0 && p.count_off % 4 == 0 && p.team_bytes == p.count_off + 8 && p.lds_bytes == p.team_bytes * (uint32_t)p.rows_per_wg &&
             (int64_t)p.queue_cap * 64 > c.w + c.ow && p.lds_bytes + 64 <= 160 * 1024;
        EXPECT(ok, "proximity: the plan of %d x %d, window (%d, %d, %d x %d)", c.h, c.w, c.r0, c.c0, c.oh, c.ow);
      }
      fra_proximity_opts o{};
      o.out_height = 3; o.out_width = 32768;
      const fra_px::Plan wide = fra_px::make_plan(3, 32768, o);
      EXPECT(wide.levels == 16 && wide.rows_per_wg == 1 && wide.queue_cap == 1025 && wide.lds_bytes == 133132 && wide.row_wgs == 3 && wide.col_blocks == 128, "proximity: the widest plan: %d levels, %u bytes", wide.levels, wide.lds_bytes);
      o.out_row_off = 60; o.out_col_off = 3; o.out_height = 75; o.out_width = 60;
      const fra_px::Plan seam = fra_px::make_plan(200, 70, o);
      EXPECT(seam.nchunks == 4 && seam.k0 == 0 && seam.k1 == 2 && seam.rows_per_wg == 4 && seam.row_wgs == 19 && seam.levels == 6, "proximity: the plan of the seam shape");
    }
  }
  // ... and of the regions unit (fra_regions.hip): refused before any GPU work, in the order the header gives
  {
    auto says = [&](int rc, const char* what) { return rc == FRA_E_INVALID && g_msg.find(what) != std::string::npos; };
    static uint8_t rsrc[3 * 40 * 50];
    static int32_t rlab[3 * 40 * 50];
    static float rarea[3 * 40 * 50];
    static uint8_t rsieved[3 * 40 * 50];
    static fra_region_rec rtab[3 * 10];
    uint64_t counts[12];
    for (uint64_t& v : counts) v = 9;
    fra_regions_job rj{};
    rj.src = rsrc; rj.dtype = FRA_U8; rj.channels = 3; rj.height = 40; rj.width = 50;
    rj.band_stride = 2000; rj.row_stride = 50; rj.col_stride = 1;
    rj.opts.connectivity = 4; rj.opts.min_size = 1; rj.opts.table = rtab; rj.opts.table_cap = 10;
    rj.opts.labels.dst = rlab; rj.opts.labels.dtype = FRA_I32; rj.opts.labels.band_stride = 2000; rj.opts.labels.row_stride = 50; rj.opts.labels.col_stride = 1;
    rj.opts.area.dst = rarea; rj.opts.area.dtype = FRA_F32; rj.opts.area.band_stride = 2000; rj.opts.area.row_stride = 50; rj.opts.area.col_stride = 1;
    rj.opts.sieved.dst = rsieved; rj.opts.sieved.band_stride = 2000; rj.opts.sieved.row_stride = 50; rj.opts.sieved.col_stride = 1;
    const fra_region::Strides rss{2000, 50, 1};
    EXPECT(fra_rg::check_job(FRA_U8, 3, 40, 50, rss, &rj.opts) == FRA_OK, "regions: the sample job is refused: %s", g_msg.c_str());
    EXPECT(fra_regions(nullptr, &rj, counts) == FRA_E_INVALID, "regions: null ctx accepted");
    EXPECT(fra_regions(ctx, nullptr, counts) == FRA_E_INVALID, "regions: null job accepted");
    { auto j = rj; j.src = nullptr; EXPECT(says(fra_regions(ctx, &j, counts), "null argument"), "regions: null src: %s", g_msg.c_str()); }
    for (int d : {-1, 8}) { auto j = rj; j.dtype = d; EXPECT(says(fra_regions(ctx, &j, counts), "bad dtype"), "regions: dtype %d: %s", d, g_msg.c_str()); }
    { auto j = rj; j.channels = 0; EXPECT(says(fra_regions(ctx, &j, counts), "bad raster layout"), "regions: no band: %s", g_msg.c_str()); }
    { auto j = rj; j.channels = 256; EXPECT(says(fra_regions(ctx, &j, counts), "more than 255"), "regions: 256 bands: %s", g_msg.c_str()); }
    { auto j = rj; j.col_stride = -1; EXPECT(says(fra_regions(ctx, &j, counts), "bad raster layout"), "regions: negative source stride: %s", g_msg.c_str()); }
    for (int d : {-1, (int)FRA_F32, (int)FRA_F64, 8}) { auto j = rj; j.opts.labels.dtype = d; EXPECT(says(fra_regions(ctx, &j, counts), "bad labels dtype"), "regions: labels dtype %d: %s", d, g_msg.c_str()); }
    { auto j = rj; j.opts.labels.row_stride = -1; EXPECT(says(fra_regions(ctx, &j, counts), "bad labels layout"), "regions: negative labels stride: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.area.dtype = 8; EXPECT(says(fra_regions(ctx, &j, counts), "bad area dtype"), "regions: area dtype 8: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.area.band_stride = -1; EXPECT(says(fra_regions(ctx, &j, counts), "bad area layout"), "regions: negative area stride: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.sieved.col_stride = -1; EXPECT(says(fra_regions(ctx, &j, counts), "bad sieved layout"), "regions: negative sieved stride: %s", g_msg.c_str()); }
    { auto o = rj.opts; o.labels.dst = nullptr; o.labels.dtype = FRA_F32; o.area.dst = nullptr; o.area.dtype = 8; o.sieved.dtype = 99;
      EXPECT(fra_rg::check_job(FRA_U8, 3, 40, 50, rss, &o) == FRA_OK, "regions: the dtype of an output that is not given was looked at: %s", g_msg.c_str()); }
    for (int n : {0, -3, 32769}) {
      { auto j = rj; j.height = n; EXPECT(says(fra_regions(ctx, &j, counts), "1 .. 32768"), "regions: height %d: %s", n, g_msg.c_str()); }
      { auto j = rj; j.width = n; EXPECT(says(fra_regions(ctx, &j, counts), "1 .. 32768"), "regions: width %d: %s", n, g_msg.c_str()); }
    }
    for (int n : {-1, 17}) { auto j = rj; j.opts.nvalues = n; EXPECT(says(fra_regions(ctx, &j, counts), "nvalues"), "regions: %d values: %s", n, g_msg.c_str()); }
    for (double v : {(double)NAN, (double)INFINITY}) { auto j = rj; j.opts.nvalues = 2; j.opts.values[1] = v; EXPECT(says(fra_regions(ctx, &j, counts), "foreground value 1 is not finite"), "regions: value %g: %s", v, g_msg.c_str()); }
    for (int n : {0, 6, -4, 16}) { auto j = rj; j.opts.connectivity = n; EXPECT(says(fra_regions(ctx, &j, counts), "connectivity"), "regions: connectivity %d: %s", n, g_msg.c_str()); }
    for (int n : {0, -7}) { auto j = rj; j.opts.min_size = n; EXPECT(says(fra_regions(ctx, &j, counts), "min_size"), "regions: min_size %d: %s", n, g_msg.c_str()); }
    { auto j = rj; j.opts.table_cap = -1; EXPECT(says(fra_regions(ctx, &j, counts), "table_cap"), "regions: table_cap -1: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.labels.dst = nullptr; j.opts.area.dst = nullptr; j.opts.sieved.dst = nullptr; j.opts.table = nullptr;
      EXPECT(says(fra_regions(ctx, &j, counts), "none of labels, area, sieved and table"), "regions: no output: %s", g_msg.c_str()); }
    { auto o = rj.opts; o.labels.dst = nullptr; o.area.dst = nullptr; o.sieved.dst = nullptr; o.table_cap = 0;
      EXPECT(fra_rg::check_job(FRA_U8, 3, 40, 50, rss, &o) == FRA_OK, "regions: a table alone refused: %s", g_msg.c_str()); }
    // the order: an input that breaks two rules gets the message of the first
    { auto j = rj; j.dtype = 8; j.height = 0; EXPECT(says(fra_regions(ctx, &j, counts), "bad dtype"), "regions: dtype 8 and height 0: %s", g_msg.c_str()); }
    { auto j = rj; j.channels = 256; j.opts.labels.dtype = FRA_F32; EXPECT(says(fra_regions(ctx, &j, counts), "more than 255"), "regions: 256 bands and float labels: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.labels.dtype = FRA_F64; j.opts.area.dtype = -1; EXPECT(says(fra_regions(ctx, &j, counts), "bad labels dtype"), "regions: labels and area dtypes: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.area.dtype = -1; j.width = 40000; EXPECT(says(fra_regions(ctx, &j, counts), "bad area dtype"), "regions: area dtype and width: %s", g_msg.c_str()); }
    { auto j = rj; j.height = 0; j.opts.nvalues = 17; EXPECT(says(fra_regions(ctx, &j, counts), "1 .. 32768"), "regions: height 0 and 17 values: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.nvalues = 17; j.opts.connectivity = 5; EXPECT(says(fra_regions(ctx, &j, counts), "nvalues"), "regions: 17 values and connectivity 5: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.connectivity = 5; j.opts.min_size = 0; EXPECT(says(fra_regions(ctx, &j, counts), "connectivity"), "regions: connectivity 5 and min_size 0: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.min_size = 0; j.opts.table_cap = -1; EXPECT(says(fra_regions(ctx, &j, counts), "min_size"), "regions: min_size 0 and table_cap -1: %s", g_msg.c_str()); }
    { auto j = rj; j.opts.table_cap = -1; j.opts.labels.dst = nullptr; j.opts.area.dst = nullptr; j.opts.sieved.dst = nullptr; j.opts.table = nullptr;
      EXPECT(says(fra_regions(ctx, &j, counts), "table_cap"), "regions: table_cap -1 and no output: %s", g_msg.c_str()); }
    bool untouched = true;
    for (uint64_t v : counts) untouched = untouched && v == 9;
    EXPECT(untouched, "regions: a refusal wrote the counts");
    EXPECT(fra_regions_timing(nullptr) == FRA_E_INVALID, "regions timing: null accepted");
    // the read over a region: what the windowed read refuses is referred to it; the options as above
    {
      fra_decode_item di = it;
      di.window = {0, 0, 4, 8};
      fra_decode_job dj = job;
      dj.items = &di;
      const fra_window r48{0, 0, 4, 8};
      fra_window r40 = r48;
      r40.width = 0;
      auto o = rj.opts;
      EXPECT(fra_decode_device_regions(ctx, &dj, &r48, nullptr, inf, counts) == FRA_E_INVALID && g_msg == "null argument", "regions read: null options: %s", g_msg.c_str());
      EXPECT(fra_decode_device_regions(ctx, &dj, nullptr, &o, inf, counts) == FRA_E_INVALID, "regions read: null roi accepted");
      EXPECT(says(fra_decode_device_regions(ctx, &dj, &r40, &o, inf, counts), "region of interest"), "regions read: zero-width roi: %s", g_msg.c_str());
      { auto q = o; q.min_size = 0; EXPECT(says(fra_decode_device_regions(ctx, &dj, &r40, &q, inf, counts), "region of interest"), "regions read: zero-width roi and min_size 0: %s", g_msg.c_str()); }
      { auto q = o; q.min_size = 0; EXPECT(says(fra_decode_device_regions(ctx, &dj, &r48, &q, inf, counts), "min_size"), "regions read: min_size 0: %s", g_msg.c_str()); }
      { auto q = o; q.labels.dtype = FRA_F32; EXPECT(says(fra_decode_device_regions(ctx, &dj, &r48, &q, inf, counts), "bad labels dtype"), "regions read: float labels: %s", g_msg.c_str()); }
      { fra_window r = r48; r.height = 5; EXPECT(says(fra_decode_device_regions(ctx, &dj, &r, &o, inf, counts), "do not cover"), "regions read: uncovered row: %s", g_msg.c_str()); }
    }
    // the FRA_E_SPACE decisions: N against the labels dtype, then against the table
    {
      auto space = [&](int rc, const char* what) { return rc == FRA_E_SPACE && g_msg.find(what) != std::string::npos; };
      EXPECT(fra_rg::label_max(FRA_U8) == 255 && fra_rg::label_max(FRA_I8) == 127 && fra_rg::label_max(FRA_U16) == 65535 && fra_rg::label_max(FRA_I16) == 32767 &&
                 fra_rg::label_max(FRA_U32) == 4294967295ll && fra_rg::label_max(FRA_I32) == 2147483647ll, "regions: the greatest label of a dtype");
      auto o = rj.opts;
      o.labels.dtype = FRA_U8; o.table_cap = 300;
      EXPECT(fra_rg::check_space(1, 255, &o) == FRA_OK, "regions: 255 components refused for uint8 labels: %s", g_msg.c_str());
      EXPECT(space(fra_rg::check_space(1, 256, &o), "band 1 has 256 components, more than the labels dtype holds (255)"), "regions: 256 components in uint8 labels: %s", g_msg.c_str());
      o.labels.dtype = FRA_I8;
      EXPECT(fra_rg::check_space(0, 127, &o) == FRA_OK && space(fra_rg::check_space(0, 128, &o), "labels dtype holds (127)"), "regions: int8 labels: %s", g_msg.c_str());
      o.labels.dtype = FRA_I32;
      EXPECT(fra_rg::check_space(2, 300, &o) == FRA_OK, "regions: a full table refused: %s", g_msg.c_str());
      EXPECT(space(fra_rg::check_space(2, 301, &o), "band 2 has 301 components, more than the table holds (300)"), "regions: 301 components in a table of 300: %s", g_msg.c_str());
      o.labels.dtype = FRA_U8;  // both: the labels dtype is named
      EXPECT(space(fra_rg::check_space(2, 301, &o), "labels dtype"), "regions: both limits: %s", g_msg.c_str());
      o.labels.dst = nullptr; o.table = nullptr; o.table_cap = 0;
      EXPECT(fra_rg::check_space(0, 1 << 30, &o) == FRA_OK, "regions: limits of outputs that are not given: %s", g_msg.c_str());
      o = rj.opts;  // int32 labels, a table of 10
      EXPECT(fra_rg::may_lack_space(40, 50, &o), "regions: a table of 10 for 2000 pixels cannot lack space");
      o.table_cap = 2000;
      EXPECT(!fra_rg::may_lack_space(40, 50, &o), "regions: a table of a record per pixel can lack space");
      o.table = nullptr; o.labels.dtype = FRA_U16;
      EXPECT(!fra_rg::may_lack_space(40, 50, &o) && fra_rg::may_lack_space(256, 257, &o) && !fra_rg::may_lack_space(255, 257, &o), "regions: uint16 labels and the pixel count");
      o.labels.dtype = FRA_I32;
      EXPECT(!fra_rg::may_lack_space(32768, 32768, &o), "regions: int32 labels hold 2^30 components");
    }
    // the launch plan: tiles of 64, a seam thread per border pixel, scan blocks of 4096
    {
      EXPECT(fra_rg::kRun == 16 && fra_rg::kScanBlock == 4096 && (fra_rg::kRootBit & 0x40000000u) == 0 && (int64_t)fra_rg::kMaxSide * fra_rg::kMaxSide <= (int64_t)fra_rg::kRootBit >> 1, "regions: the constants");
      const struct { int h, w, tx, ty; long long rows, cols; unsigned links, seams, blocks; } cases[] = {
          {1, 1, 1, 1, 0, 0, 1, 0, 1},       {64, 64, 1, 1, 0, 0, 16, 0, 1},        {65, 65, 2, 2, 65, 65, 17, 1, 2},
          {130, 191, 3, 3, 382, 260, 97, 3, 7}, {5, 1100, 18, 1, 0, 85, 22, 1, 2}, {520, 520, 9, 9, 4160, 4160, 1057, 33, 67},
          {3, 32768, 512, 1, 0, 1533, 384, 6, 24}, {32768, 3, 1, 512, 1533, 0, 384, 6, 24}};
      for (const auto& c : cases) {
        const fra_rg::Plan p = fra_rg::make_plan(c.h, c.w);
        EXPECT(p.tiles_x == c.tx && p.tiles_y == c.ty && p.npix == (int64_t)c.h * c.w && p.seam_row_threads == c.rows && p.seam_col_threads == c.cols &&
                   p.link_wgs == c.links && p.seam_wgs == c.seams && p.pixel_scan_blocks == c.blocks,
               "regions: the plan of %d x %d: %d x %d tiles, %lld + %lld seam threads, %u / %u / %u workgroups", c.h, c.w, p.tiles_x, p.tiles_y,
               (long long)p.seam_row_threads, (long long)p.seam_col_threads, p.link_wgs, p.seam_wgs, p.pixel_scan_blocks);
      }
      const fra_rg::Plan big = fra_rg::make_plan(32768, 32768);
      EXPECT(big.npix == (1ll << 30) && big.link_wgs == (1u << 22) && big.pixel_scan_blocks == (1u << 18) && big.seam_row_threads == 511ll * 32768 && big.seam_wgs == 130816u, "regions: the greatest plan");
      EXPECT(fra_rg::scan_blocks(0) == 0 && fra_rg::scan_blocks(1) == 1 && fra_rg::scan_blocks(4096) == 1 && fra_rg::scan_blocks(4097) == 2, "regions: scan blocks");
    }
  }
  // ... and the order of the refusals of these five units: an input that breaks two rules gets the message of the first
  {
    fra_decode_item di = it;
    di.window = {0, 0, 4, 8};
    fra_decode_job dj = job;  // dst_dtype int32
    dj.items = &di;
    const fra_window r48{0, 0, 4, 8};
    fra_window r40 = r48;
    r40.width = 0;
    auto says = [&](int rc, const char* what) { return rc == FRA_E_INVALID && g_msg.find(what) != std::string::npos; };
    int32_t out[16];
    static int32_t ref[64];
    uint64_t filled[8], hist[8];
    fra_decimate_job kj{};
    kj.src = dst; kj.dtype = FRA_I32; kj.channels = 1; kj.height = 8; kj.width = 8;
    kj.src_band_stride = 64; kj.src_row_stride = 8; kj.src_col_stride = 1;
    kj.factor = 2; kj.resampling = FRA_RESAMPLE_AVERAGE;
    kj.dst = out; kj.dst_band_stride = 16; kj.dst_row_stride = 4; kj.dst_col_stride = 1;
    fra_resample_job mj{};
    mj.src = dst; mj.dtype = FRA_I32; mj.channels = 1; mj.height = 8; mj.width = 8;
    mj.src_band_stride = 64; mj.src_row_stride = 8; mj.src_col_stride = 1;
    mj.out_height = 3; mj.out_width = 5; mj.resampling = FRA_RESAMPLE_AVERAGE;
    mj.dst = out; mj.dst_band_stride = 15; mj.dst_row_stride = 5; mj.dst_col_stride = 1;
    { auto j = kj; j.factor = 3; j.dtype = 8; EXPECT(says(fra_decimate(ctx, &j), "decimation factor"), "decimate: factor 3 and dtype 8: %s", g_msg.c_str()); }
    { auto j = kj; j.dtype = 8; j.height = 0; EXPECT(says(fra_decimate(ctx, &j), "bad dtype"), "decimate: dtype 8 and zero height: %s", g_msg.c_str()); }
    { auto j = kj; j.factor = 3; EXPECT(says(fra_decimate_masked(ctx, &j, 0.5, filled), "decimation factor"), "masked decimate: factor 3 and nodata 0.5: %s", g_msg.c_str()); }
    { auto j = kj; j.dtype = 8; EXPECT(says(fra_decimate_masked(ctx, &j, 0.5, filled), "bad dtype"), "masked decimate: dtype 8 and nodata 0.5: %s", g_msg.c_str()); }
    { auto j = kj; j.dst_row_stride = -1; EXPECT(says(fra_decimate_masked(ctx, &j, 0.5, filled), "bad raster layout"), "masked decimate: negative stride and nodata 0.5: %s", g_msg.c_str()); }
    { auto j = mj; j.dtype = 8; j.width = 0; EXPECT(says(fra_resample(ctx, &j), "bad dtype"), "resample: dtype 8 and zero width: %s", g_msg.c_str()); }
    { auto j = mj; j.src_col_stride = -1; j.out_width = 0; EXPECT(says(fra_resample(ctx, &j), "bad raster layout"), "resample: negative stride and out width 0: %s", g_msg.c_str()); }
    { auto j = mj; j.out_height = 0; EXPECT(says(fra_resample_masked(ctx, &j, 0.5, filled), "output size"), "masked resample: out height 0 and nodata 0.5: %s", g_msg.c_str()); }
    { auto j = mj; j.dst_row_stride = -1; EXPECT(says(fra_resample_masked(ctx, &j, 0.5, filled), "bad raster layout"), "masked resample: negative stride and nodata 0.5: %s", g_msg.c_str()); }
    { auto j = mj; j.dst_row_stride = -1; j.out_height = 0; EXPECT(says(fra_resample_masked(ctx, &j, 0.0, filled), "bad raster layout"), "masked resample: negative stride and out height 0: %s", g_msg.c_str()); }
    EXPECT(says(fra_decode_device_resampled(ctx, &dj, &r40, 0, 5, 1, inf), "output size"), "resampled read: zero-width roi and out height 0: %s", g_msg.c_str());
    EXPECT(says(fra_decode_device_resampled_masked(ctx, &dj, &r40, 0, 5, 1, inf, 0.0, filled), "output size"), "masked resampled read: zero-width roi and out height 0: %s", g_msg.c_str());
    EXPECT(says(fra_decode_device_resampled_masked(ctx, &dj, &r40, 3, 5, 1, inf, 0.5, filled), "region of interest"), "masked resampled read: zero-width roi and nodata 0.5: %s", g_msg.c_str());
    EXPECT(says(fra_decode_device_resampled_masked(ctx, &dj, &r48, 0, 5, 1, inf, 0.5, filled), "output size"), "masked resampled read: out height 0 and nodata 0.5: %s", g_msg.c_str());
    { fra_window r = r48; r.height = 5; EXPECT(says(fra_decode_device_resampled_masked(ctx, &dj, &r, 3, 5, 1, inf, 0.5, filled), "nodata"), "masked resampled read: uncovered row and nodata 0.5: %s", g_msg.c_str()); }
    EXPECT(says(fra_decode_device_decimated(ctx, &dj, &r40, 3, 1, inf), "decimation factor"), "decimated read: factor 3 and zero-width roi: %s", g_msg.c_str());
    EXPECT(says(fra_decode_device_decimated_masked(ctx, &dj, &r40, 3, 1, inf, 0.0, filled), "decimation factor"), "masked decimated read: factor 3 and zero-width roi: %s", g_msg.c_str());
    EXPECT(says(fra_decode_device_decimated_masked(ctx, &dj, &r40, 2, 1, inf, 0.5, filled), "region of interest"), "masked decimated read: zero-width roi and nodata 0.5: %s", g_msg.c_str());
    { fra_window r = r48; r.height = 5; EXPECT(says(fra_decode_device_decimated_masked(ctx, &dj, &r, 2, 1, inf, 0.5, filled), "nodata"), "masked decimated read: uncovered row and nodata 0.5: %s", g_msg.c_str()); }
    fra_stats_band sbands[1];
    fra_stats_opts eight{};
    eight.bins = 8; eight.hist_lo = 0.0; eight.hist_hi = 1.0;
    { auto o = eight; o.bins = -1; EXPECT(says(fra_decode_device_stats(ctx, &dj, &r40, &o, sbands, hist, inf), "bins"), "statistics read: bins -1 and zero-width roi: %s", g_msg.c_str()); }
    { fra_window r{0, 0, 65537, 65536}; auto j = dj; j.nitems = 0; EXPECT(says(fra_decode_device_stats(ctx, &j, &r, &eight, sbands, hist, inf), "2^32 pixels"), "statistics read: 2^32 pixels and no items: %s", g_msg.c_str()); }
    fra_stats_job sj{};
    sj.src = dst; sj.dtype = FRA_I32; sj.channels = 1; sj.height = 8; sj.width = 8;
    sj.band_stride = 64; sj.row_stride = 8; sj.col_stride = 1;
    { auto j = sj; j.dtype = 8; j.width = 0; EXPECT(says(fra_stats(ctx, &j, sbands, hist), "bad dtype"), "statistics: dtype 8 and zero width: %s", g_msg.c_str()); }
    { auto j = sj; j.row_stride = -8; j.opts = eight; j.opts.bins = -1; EXPECT(says(fra_stats(ctx, &j, sbands, hist), "bad raster layout"), "statistics: negative stride and bins -1: %s", g_msg.c_str()); }
    { auto j = sj; j.height = 65537; j.width = 65536; j.opts = eight; j.opts.bins = -1; EXPECT(says(fra_stats(ctx, &j, sbands, hist), "2^32 pixels"), "statistics: 2^32 pixels and bins -1: %s", g_msg.c_str()); }
    fra_compare_band cbands[1];
    EXPECT(says(fra_decode_device_compare(ctx, &dj, &r40, ref, 0, 32, -8, 1, cbands, inf), "bad reference layout"), "compared read: negative reference stride and zero-width roi: %s", g_msg.c_str());
    { fra_window r{0, 0, 65537, 65536}; auto j = dj; j.nitems = 0; EXPECT(says(fra_decode_device_compare(ctx, &j, &r, ref, 0, 32, 8, 1, cbands, inf), "2^32 pixels"), "compared read: 2^32 pixels and no items: %s", g_msg.c_str()); }
    fra_compare_job cj{};
    cj.a = dst; cj.b = ref; cj.dtype = FRA_I32; cj.channels = 1; cj.height = 8; cj.width = 8;
    cj.a_band_stride = cj.b_band_stride = 64; cj.a_row_stride = cj.b_row_stride = 8; cj.a_col_stride = cj.b_col_stride = 1;
    { auto j = cj; j.dtype = 8; j.b_row_stride = -8; EXPECT(says(fra_compare(ctx, &j, cbands), "bad dtype"), "compare: dtype 8 and negative stride: %s", g_msg.c_str()); }
    { auto j = cj; j.height = 65537; j.width = 65536; j.a_col_stride = -1; EXPECT(says(fra_compare(ctx, &j, cbands), "bad raster layout"), "compare: negative stride and 2^32 pixels: %s", g_msg.c_str()); }
  }
  printf("argument validation checked\n");
#endif
  // the chunk arithmetic of the row-chunk scan (fra_scan.h plan_chunks): its invariants over every element size and a
  // set of shapes (one slot, short last slots, more than 256 slots per row, one column, 2^32 pixels, the benchmark
  // scene), as the reducing units call it (slots of 16 bytes, with and without the statistics' pixel cap) and as the
  // band math does (slots of 4 and 8 pixels, one band), and pinned values
  {
    using fra_region::ChunkPlan;
    using fra_region::plan_chunks;
    struct Shape { int64_t h, w, bands; };
    const Shape shapes[] = {{1, 1, 1}, {5, 511, 1}, {3, 4113, 1}, {130, 517, 1}, {(int64_t)1 << 20, 1, 1}, {65536, 65536, 1},
                            {10980, 10980, 4}};
    auto check = [&](int64_t V, const Shape& s, int64_t bands, int64_t slot_cap, int64_t pixel_cap) {
      ChunkPlan p{};
      EXPECT(plan_chunks(&p, V, s.h, s.w, bands, slot_cap, pixel_cap, "check") == FRA_OK, "plan V %lld %lld x %lld refused: %s",
             (long long)V, (long long)s.h, (long long)s.w, g_msg.c_str());
      const int64_t nvec = p.nvec, rpb = p.rpb, nchunks = p.nchunks;
      const bool ok = nvec == (s.w + V - 1) / V && rpb >= 1 && (nchunks - 1) * rpb < s.h && s.h <= nchunks * rpb &&
                      rpb * nvec <= slot_cap && (!pixel_cap || rpb * s.w <= pixel_cap) &&
                      (int64_t)p.step_rows * nvec + p.step_vecs == 256 && (int64_t)p.step_vecs < nvec &&
                      (int64_t)p.grid == nchunks * bands;
      EXPECT(ok, "plan V %lld %lld x %lld x %lld cap %lld / %lld: nvec %u rpb %u nchunks %u step %u + %u grid %u", (long long)V,
             (long long)s.h, (long long)s.w, (long long)bands, (long long)slot_cap, (long long)pixel_cap, p.nvec, p.rpb, p.nchunks,
             p.step_rows, p.step_vecs, p.grid);
    };
    for (int64_t es : {1, 2, 4, 8})
      for (const Shape& s : shapes) {
        check(16 / es, s, s.bands, (int64_t)1 << 31, 0);
        check(16 / es, s, s.bands, (int64_t)1 << 31, ((int64_t)1 << 32) - 1);
      }
    for (int64_t P : {4, 8})
      for (const Shape& s : shapes) check(P, s, 1, (int64_t)1 << 29, 0);
    auto pin = [&](const char* what, int64_t V, const Shape& s, int64_t slot_cap, int64_t pixel_cap, ChunkPlan want) {
      ChunkPlan p{};
      plan_chunks(&p, V, s.h, s.w, s.bands, slot_cap, pixel_cap, "check");
      EXPECT(p.nvec == want.nvec && p.rpb == want.rpb && p.nchunks == want.nchunks && p.step_rows == want.step_rows &&
                 p.step_vecs == want.step_vecs && p.grid == want.grid,
             "plan %s: nvec %u rpb %u nchunks %u step %u + %u grid %u", what, p.nvec, p.rpb, p.nchunks, p.step_rows, p.step_vecs,
             p.grid);
    };
    pin("benchmark scene, 2-byte elements", 8, {10980, 10980, 4}, (int64_t)1 << 31, 0, {1373, 11, 999, 0, 256, 3996});
    pin("3 x 4113, 8-byte elements", 2, {3, 4113, 1}, (int64_t)1 << 31, 0, {2057, 1, 3, 0, 256, 3});
    pin("2^20 x 1, 4-byte elements", 4, {(int64_t)1 << 20, 1, 1}, (int64_t)1 << 31, 0, {1, 1024, 1024, 256, 0, 1024});
    pin("65536 x 65536 x 4, 1-byte elements, pixel cap", 16, {65536, 65536, 4}, (int64_t)1 << 31, ((int64_t)1 << 32) - 1,
        {4096, 64, 1024, 0, 256, 4096});
    pin("130 x 517, band math with 8 pixels", 8, {130, 517, 1}, (int64_t)1 << 29, 0, {65, 16, 9, 3, 61, 9});
    { ChunkPlan p{}; EXPECT(plan_chunks(&p, 16, INT32_MAX, 1, 2, 1, 0, "check") == FRA_E_INVALID && g_msg == "the raster is too large for one check", "plan: a grid past INT32_MAX: %s", g_msg.c_str()); }
    printf("chunk plans checked\n");
  }
  printf(g_fail ? "%d FAILED\n" : "host check ok\n", g_fail);
  return g_fail ? 1 : 0;
}
