// decode_host_check.cpp -- stand-alone check of the host-side pieces of the device decoder, meant to be built with
// host sanitizers (make -C flac-raster_amd/csrc hostcheck) and run without a GPU:
//   * the candidate search (fra_decode_host.h scan_units) and the chain (chain_stream) over the files given on the
//     command line and over corrupted / truncated variants of them; the per-candidate frame lengths that k_dec_parse
//     would report come from the host decoder's own validate-only frame decode, and the chain's verdict and sample
//     count must agree with fra_decode on the same bytes;
//   * the argument validation of fra_decode_device, which returns before any GPU work.
// usage: decode_host_check [--concat] file.flac ...
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../flac-raster_amd/csrc/fra_decode.cpp"  // the host decoder's frame validation (internal linkage)
#include "../flac-raster_amd/csrc/fra_decode_host.h"

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
  printf("argument validation checked\n");
#endif
  printf(g_fail ? "%d FAILED\n" : "host check ok\n", g_fail);
  return g_fail ? 1 : 0;
}
