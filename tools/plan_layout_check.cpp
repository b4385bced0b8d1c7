// plan_layout_check.cpp -- stand-alone check of the plan layout (flac-raster_amd/csrc/fra_layout.h): the pure host
// arithmetic behind fra_plan_create, built with g++ and host sanitizers (make -C flac-raster_amd/csrc plancheck)
// and run without a GPU.  It lays out a handful of jobs -- an empty window, edge tiles, a small block size, ranged
// plans, windows out of row order, a plan large enough for several host bands and frame groups -- and checks the
// invariants the kernels and the host pipeline rely on.  It also pins layout_loads: for raster layouts of every kind
// (padded rows and bands, interleaved, zero and overlapping strides, rows 2^29 elements apart) the vector width and
// row block of the min/max pass, the 8-byte sample vectors, the 32-bit offsets and the wave kernel's eligibility,
// against values worked out by hand.
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../flac-raster_amd/csrc/fra_layout.h"

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

static int g_fail = 0;
static const char* g_what = "";
#define EXPECT(c, ...) do { if (!(c)) { g_fail++; printf("FAIL %s:%d [%s] %s: ", __FILE__, __LINE__, g_what, #c); printf(__VA_ARGS__); printf("\n"); } } while (0)

using namespace fra;

static std::vector<fra_window> tiles(int H, int W, int tile) {
  std::vector<fra_window> w;
  for (int r = 0; r < H; r += tile)
    for (int c = 0; c < W; c += tile) w.push_back({r, c, std::min(tile, H - r), std::min(tile, W - c)});
  return w;
}

// a uint16 band-planar H x W job at level 5, normalised to 16 bits (mid-side with two channels)
static fra_job job_u16(int H, int W, int channels, int blocksize, const std::vector<fra_window>& w) {
  fra_job j{};
  j.dtype = FRA_U16;
  j.channels = channels;
  j.band_stride = (int64_t)H * W;
  j.row_stride = W;
  j.col_stride = 1;
  j.windows = w.data();
  j.nwindows = (int)w.size();
  j.level = 5;
  j.blocksize = blocksize;
  j.norm = 16;
  return j;
}

// groups (or the host bands' groups) partition windows and frames contiguously and in order
static void check_partition(const PlanLayout& L, const std::vector<Group>& gs) {
  int w = 0, f = 0;
  for (const Group& g : gs) {
    EXPECT(g.w0 == w && g.f0 == f && g.w1 >= g.w0 && g.f1 >= g.f0, "group (%d,%d,%d,%d) after window %d frame %d",
           g.w0, g.w1, g.f0, g.f1, w, f);
    int nf = 0;
    for (int k = g.w0; k < g.w1 && k < (int)L.streams.size(); k++) nf += L.streams[k].nframes;
    EXPECT(g.f1 - g.f0 == nf, "group of %d frames, its windows have %d", g.f1 - g.f0, nf);
    w = g.w1;
    f = g.f1;
  }
  EXPECT(w == (int)L.streams.size() && f == (int)L.frames.size(), "groups end at window %d frame %d", w, f);
}

static void check_layout(const char* what, const fra_job& j, const int32_t* franges, int groups, bool monotone) {
  g_what = what;
  PlanLayout L;
  const int rc = build_layout(j, j.windows, franges, groups, L);
  EXPECT(rc == FRA_OK, "build_layout: %d (%s)", rc, g_msg.c_str());
  if (rc) return;
  const int ns = (int)L.streams.size(), nfr = (int)L.frames.size(), bs = j.blocksize;
  EXPECT(ns == j.nwindows, "%d streams", ns);
  EXPECT(L.mid_side == (j.channels == 2) && L.cmax == (L.mid_side ? 4 : j.channels) && !L.b32, "channel layout");

  // streams and frames
  int first = 0;
  size_t verbatim = 0;
  for (int w = 0, g = 0; w < ns; w++) {
    const StreamDev& st = L.streams[w];
    EXPECT(st.first_frame == first, "window %d: first_frame %d, prefix sum %d", w, st.first_frame, first);
    EXPECT(st.nsamples == (int64_t)j.windows[w].width * j.windows[w].height, "window %d: nsamples", w);
    const int64_t nfr_all = (st.nsamples + bs - 1) / bs;
    int64_t fa = 0, want = nfr_all;
    if (franges) {  // frames [first, first + count) of the stream, the count clipped to its end (-1: to the end)
      fa = franges[2 * w];
      want = franges[2 * w + 1] < 0 ? nfr_all - fa : std::min<int64_t>(franges[2 * w + 1], nfr_all - fa);
    }
    EXPECT(st.nframes == want, "window %d: %d frames, expected %lld", w, st.nframes, (long long)want);
    int64_t sum = 0;
    for (int k = 0; k < st.nframes && g < nfr; k++, g++) {
      const FrameDev& fr = L.frames[g];
      EXPECT(fr.stream == w && fr.index == fa + k, "frame %d: stream %d index %d", g, fr.stream, fr.index);
      EXPECT(fr.n > 0 && fr.n <= bs, "frame %d: n = %d", g, fr.n);
      EXPECT((int64_t)fr.row0 * st.width + fr.col0 == (int64_t)fr.index * bs, "frame %d: starts at (%d, %d)", g, fr.row0,
             fr.col0);
      EXPECT(fr.win >= 0 && fr.win < (int)L.win_sizes.size() && L.win_sizes[fr.win] == fr.n, "frame %d: window table", g);
      sum += fr.n;
      // a VERBATIM frame: header (<= 16 bytes with its CRC-8), per channel a subframe header byte and n samples --
      // the side channel of a mid-side pair carries one bit more --, padding, CRC-16
      const size_t bits = (size_t)j.channels * (8 + (size_t)fr.n * 16) + (L.mid_side ? fr.n : 0);
      verbatim += 16 + (bits + 7) / 8 + 2;
    }
    if (!franges) EXPECT(sum == st.nsamples, "window %d: its frames hold %lld of %lld samples", w, (long long)sum,
                         (long long)st.nsamples);
    first += st.nframes;
  }
  EXPECT(first == nfr, "%d frames, the windows' counts sum to %d", nfr, first);
  EXPECT(L.out_cap >= verbatim, "capacity %zu < %zu bytes of VERBATIM frames", L.out_cap, verbatim);

  // groups and host bands
  check_partition(L, L.groups);
  EXPECT(L.all.w0 == 0 && L.all.w1 == ns && L.all.f0 == 0 && L.all.f1 == nfr, "the whole-plan group");
  EXPECT((int)L.groups.size() == (nfr < 4096 ? 1 : std::max(1, std::min(8, groups))), "%zu groups", L.groups.size());
  std::vector<Group> bg;
  for (const HBand& hb : L.hbands) bg.push_back(hb.g);
  if (ns) check_partition(L, bg);
  else EXPECT(L.hbands.empty(), "bands without windows");
  if (!monotone) EXPECT(L.hbands.size() == 1, "%zu bands for windows out of row order", L.hbands.size());
  if (nfr >= 2048 && monotone) EXPECT(L.hbands.size() > 1, "%zu bands for %d frames", L.hbands.size(), nfr);
  int64_t prev = 0;
  for (size_t b = 0; b < L.hbands.size(); b++) {
    const HBand& hb = L.hbands[b];
    EXPECT(hb.r0 <= hb.r1 && (b == 0 || hb.r0 >= prev), "band %zu: rows [%lld, %lld) after %lld", b, (long long)hb.r0,
           (long long)hb.r1, (long long)prev);
    prev = hb.r1;
    // every row of the band's non-empty windows: copied by exactly one band, this one or an earlier one
    for (int k = hb.g.w0; k < hb.g.w1; k++) {
      if (L.streams[k].nsamples == 0) continue;
      for (int64_t r = j.windows[k].row_off; r < (int64_t)j.windows[k].row_off + j.windows[k].height; r++) {
        int n = 0;
        for (size_t c = 0; c <= b; c++) n += r >= L.hbands[c].r0 && r < L.hbands[c].r1;
        EXPECT(n == 1, "row %lld of window %d is copied %d times by bands 0..%zu", (long long)r, k, n, b);
        if (n != 1) break;
      }
    }
  }

  // the partial list: exactly the ascending (frame * 8 + channel) entries with n < blocksize
  EXPECT(L.wave_ok == (bs == kMaxBlock), "wave_ok %d", (int)L.wave_ok);
  std::vector<int32_t> part;
  if (L.wave_ok)
    for (int g = 0; g < nfr; g++)
      for (int c = 0; L.frames[g].n < bs && c < j.channels; c++) part.push_back(g * 8 + c);
  EXPECT(part == L.part, "partial list of %zu entries, expected %zu", L.part.size(), part.size());

  // window tables
  const int nw = std::max(1, L.nwin), nt = (int)std::max<size_t>(1, L.win_sizes.size());
  EXPECT(L.nwin == num_windows(level_cfg(j.level).nsub), "nwin %d", L.nwin);
  EXPECT(L.wtab.size() == (size_t)nt * nw * bs + 64 && L.wrange.size() == 2 * (size_t)nt * nw &&
             L.wplat.size() == L.wrange.size(), "table sizes");
  for (int t = 0; t < (int)L.win_sizes.size(); t++)
    for (int w = 0; w < L.nwin; w++) {
      const size_t i = (size_t)t * nw + w;
      const int n = L.win_sizes[t], lo = L.wrange[2 * i], hi = L.wrange[2 * i + 1];
      const int plo = L.wplat[2 * i], phi = L.wplat[2 * i + 1];
      EXPECT(0 <= lo && lo <= hi && hi <= n, "table %d window %d: [%d, %d) of %d", t, w, lo, hi, n);
      EXPECT(plo <= phi && (plo == phi || (lo <= plo && phi <= hi)), "table %d window %d: plateau [%d, %d) outside [%d, %d)",
             t, w, plo, phi, lo, hi);
      const float* o = L.wtab.data() + i * bs;
      bool ones = true, zeros = true;
      for (int k = plo; k < phi; k++) ones = ones && o[k] == 1.0f;
      for (int k = 0; k < bs; k++)
        if (k < lo || k >= hi) zeros = zeros && o[k] == 0.0f;
      EXPECT(ones, "table %d window %d: a plateau coefficient is not 1.0f", t, w);
      EXPECT(zeros, "table %d window %d: a coefficient outside [%d, %d) is not zero", t, w, lo, hi);
    }
  printf("%-44s %3d windows %5d frames %zu groups %2zu bands %4zu partial, capacity %zu\n", what, ns, nfr, L.groups.size(),
         L.hbands.size(), L.part.size(), L.out_cap);
}

// ---- layout_loads: which load paths a layout allows.  Every expectation below is worked out by hand from the rule
// in fra_layout.h (V = vector bytes / itemsize; every window start, width, row stride and -- with more than one
// channel -- band stride a multiple of V; col_stride 1; the two 2^32 bounds of the min/max pass; the 2^31-byte span
// of a frame's rows for 32-bit lane offsets) and written out as numbers.
struct Loads {
  int mm_vec, mm_rows;
  bool vec8, off32, wave_ok;
};
struct LoadJob {
  int dtype, channels, level, norm;
  int64_t band, row, col;
  int blocksize = 4096;
};
static void check_loads(const char* what, const LoadJob& q, const std::vector<fra_window>& w, const Loads& want) {
  g_what = what;
  fra_job j{};
  j.dtype = q.dtype;
  j.channels = q.channels;
  j.band_stride = q.band;
  j.row_stride = q.row;
  j.col_stride = q.col;
  j.windows = w.data();
  j.nwindows = (int)w.size();
  j.level = q.level;
  j.blocksize = q.blocksize;
  j.norm = q.norm;
  PlanLayout L;
  const int rc = build_layout(j, j.windows, nullptr, 1, L);
  EXPECT(rc == FRA_OK, "build_layout: %d (%s)", rc, g_msg.c_str());
  if (rc) return;
  EXPECT(L.mm_vec == want.mm_vec, "mm_vec %d, expected %d", L.mm_vec, want.mm_vec);
  EXPECT(L.mm_rows == want.mm_rows, "mm_rows %d, expected %d", L.mm_rows, want.mm_rows);
  EXPECT(L.ld_vec8 == want.vec8, "ld_vec8 %d, expected %d", (int)L.ld_vec8, (int)want.vec8);
  EXPECT(L.ld_off32 == want.off32, "ld_off32 %d, expected %d", (int)L.ld_off32, (int)want.off32);
  EXPECT(L.wave_ok == want.wave_ok, "wave_ok %d, expected %d", (int)L.wave_ok, (int)want.wave_ok);
  int tallest = 0;
  for (const fra_window& x : w) tallest = std::max(tallest, x.height);
  if (L.mm_vec) EXPECT(L.mm_max_rows == tallest, "mm_max_rows %d, tallest window %d", L.mm_max_rows, tallest);
  printf("%-58s mm_vec %2d rows %2d vec8 %d off32 %d wave_ok %d\n", what, L.mm_vec, L.mm_rows, (int)L.ld_vec8,
         (int)L.ld_off32, (int)L.wave_ok);
}

static void check_load_paths() {
  // a 72 x 264 raster; the aligned windows start at elements 0 and 8 * row + 16 and are 264 and 128 wide, the
  // unaligned ones start at 3 * row + 5 (131 wide) and 0 (1 wide)
  const int H = 72, W = 264;
  const std::vector<fra_window> al = {{0, 0, 72, 264}, {8, 16, 40, 128}}, un = {{3, 5, 33, 131}, {0, 0, 1, 1}};
  const int64_t P = (int64_t)H * W;  // 19008 = 16 * 1188
  // min/max rows per workgroup = min(64, 2048 / (264 / V)): V 8 -> 33 vectors -> 62; V 4 -> 66 -> 31; V 2 -> 132 -> 15

  // uint16 (V = 8 for 16 bytes, 4 for 8 bytes), 3 bands, level 5, norm 16: the wave kernel's plans
  const auto u16 = [](int64_t b, int64_t r, int64_t c) { return LoadJob{FRA_U16, 3, 5, 16, b, r, c}; };
  check_loads("u16 planar", u16(P, W, 1), al, {16, 62, true, true, true});            // 264, 19008, 2128 % 8 == 0
  check_loads("u16 planar, unaligned windows", u16(P, W, 1), un, {0, 1, false, true, true});  // 797 and width 131 odd
  check_loads("u16 rows + 16 bytes", u16(72 * 272, 272, 1), al, {16, 62, true, true, true});  // 272 % 8 == 0
  check_loads("u16 rows + 8 bytes", u16(72 * 268, 268, 1), al, {8, 31, true, true, true});    // 268 % 8 == 4, % 4 == 0
  check_loads("u16 rows + 13 elements", u16(72 * 277, 277, 1), al, {0, 1, false, true, true});  // 277 odd
  check_loads("u16 bands + 8 bytes", u16(P + 4, W, 1), al, {8, 31, true, true, true});        // 19012 % 8 == 4
  check_loads("u16 bands + 1 element", u16(P + 1, W, 1), al, {0, 1, false, true, true});      // 19009 odd
  check_loads("u16 pixel-interleaved", u16(1, 3 * W, 3), al, {0, 1, false, true, true});      // col_stride 3
  check_loads("u16 line-interleaved", u16(W, 3 * W, 1), al, {16, 62, true, true, true});      // 792 % 8 == 0, band 264
  check_loads("u16 band_stride 0", u16(0, W, 1), al, {16, 62, true, true, true});
  check_loads("u16 row_stride 0", u16(W, 0, 1), al, {16, 62, true, true, true});              // starts 0 and 16
  check_loads("u16 row_stride 8", u16(832, 8, 1), al, {16, 62, true, true, true});            // starts 0 and 80
  check_loads("u16 row_stride 8, unaligned windows", u16(832, 8, 1), un, {0, 1, false, true, true});  // start 29
  // ... one band: the band stride does not matter
  check_loads("u16 one band, odd band stride", LoadJob{FRA_U16, 1, 5, 16, P + 1, W, 1}, al, {16, 62, true, true, true});
  // level 8 leaves the wave kernel's levels (3..6); a block size that is not 4096 too, and 4090 % 4 != 0 stops
  // the 8-byte sample vectors (the min/max pass does not look at the block size)
  check_loads("u16 planar, level 8", LoadJob{FRA_U16, 3, 8, 16, P, W, 1}, al, {16, 62, true, true, false});
  check_loads("u16 planar, block 4090", LoadJob{FRA_U16, 3, 5, 16, P, W, 1, 4090}, al, {16, 62, false, true, false});

  // uint8 (V = 16 / 8), 2 bands, level 5: 264 % 16 == 8, so never 16-byte vectors at this width
  const auto u8 = [](int64_t b, int64_t r, int64_t c) { return LoadJob{FRA_U8, 2, 5, 16, b, r, c}; };
  check_loads("u8 planar", u8(P, W, 1), al, {8, 62, true, true, true});
  check_loads("u8 rows + 16 bytes", u8(72 * 280, 280, 1), al, {8, 62, true, true, true});     // 280 % 16 == 8
  check_loads("u8 rows + 8 bytes", u8(72 * 272, 272, 1), al, {8, 62, true, true, true});      // 272 % 16 == 0, widths not
  check_loads("u8 rows + 13 elements", u8(72 * 277, 277, 1), al, {0, 1, false, true, true});
  check_loads("u8 bands + 8 bytes", u8(P + 8, W, 1), al, {8, 62, true, true, true});
  check_loads("u8 line-interleaved", u8(W, 2 * W, 1), al, {8, 62, true, true, true});         // band 264 % 16 == 8
  check_loads("u8 pixel-interleaved", u8(1, 2 * W, 2), al, {0, 1, false, true, true});
  {  // 16-byte vectors once everything is a multiple of 16; a window of more than 65535 vectors has none
    const std::vector<fra_window> w16 = {{0, 0, 40, 256}, {8, 16, 20, 64}};
    check_loads("u8 256 wide", u8(72 * 256, 256, 1), w16, {16, 64, true, true, true});        // 16 vectors: min(64, 128)
    const std::vector<fra_window> wide = {{0, 0, 1, 1 << 20}};
    check_loads("u8 2^20 wide", LoadJob{FRA_U8, 1, 5, 16, 1 << 20, 1 << 20, 1}, wide, {0, 1, true, true, true});
  }

  // float32 (V = 4 / 2), 2 bands, level 8, norm 24: a 32-bps plan of the levels the layout marks for a wave kernel
  // (levels >= 7), which no execute takes
  const auto f32 = [](int64_t b, int64_t r, int64_t c) { return LoadJob{FRA_F32, 2, 8, 24, b, r, c}; };
  check_loads("f32 planar", f32(P, W, 1), al, {16, 31, true, true, true});
  check_loads("f32 rows + 8 bytes", f32(72 * 266, 266, 1), al, {8, 15, true, true, true});    // 266 % 4 == 2
  check_loads("f32 bands + 8 bytes", f32(P + 2, W, 1), al, {8, 15, true, true, true});
  check_loads("f32 bands + 1 element", f32(P + 1, W, 1), al, {0, 1, false, true, true});
  check_loads("f32 pixel-interleaved", f32(1, 2 * W, 2), al, {0, 1, false, true, true});
  check_loads("f32 planar, level 5", LoadJob{FRA_F32, 2, 5, 24, P, W, 1}, al, {16, 31, true, true, false});

  // int16 raw samples (norm 0): no min/max pass at all, sample vectors as for uint16, no wave kernel
  check_loads("i16 norm 0 planar", LoadJob{FRA_I16, 2, 5, 0, P, W, 1}, al, {0, 1, true, true, false});
  check_loads("i16 norm 0 rows + 13", LoadJob{FRA_I16, 2, 5, 0, 72 * 277, 277, 1}, al, {0, 1, false, true, false});
  // float64: no vector path
  check_loads("f64 planar", LoadJob{FRA_F64, 1, 5, 24, P, W, 1}, al, {0, 1, false, true, false});
  check_loads("f64 rows + 16 bytes", LoadJob{FRA_F64, 1, 5, 24, 72 * 266, 266, 1}, al, {0, 1, false, true, false});
  check_loads("f64 pixel-interleaved", LoadJob{FRA_F64, 1, 5, 24, 1, W, 1}, al, {0, 1, false, true, false});

  // pixel-interleaved uint16 with col_stride 2, windows 1..257 wide (the scalar loader's width classes)
  {
    const std::vector<fra_window> w = {{0, 0, 40, 256}, {40, 0, 36, 255}, {76, 0, 36, 257}, {112, 0, 9000, 1}};
    check_loads("u16 col_stride 2", LoadJob{FRA_U16, 2, 5, 16, 1, 2 * 4104, 2}, w, {0, 1, false, true, true});
  }

  // the two 2^32 bounds and the 2^31-byte span, uint16, one band, the window 3 x 8192: 1024 16-byte vectors a
  // row -> 2 rows per workgroup; a frame spans ceil(4096 / 8192) + 1 = 2 rows
  const std::vector<fra_window> big = {{0, 0, 3, 8192}};
  const auto huge = [](int64_t r) { return LoadJob{FRA_U16, 1, 5, 16, 0, r, 1}; };
  const int64_t R29 = int64_t(1) << 29;
  // (2 * 2^29 + 8192) * 2 bytes = 2^31 + 16384: 64-bit offsets; 2 rows * 2^29 * 2 bytes = 2^31 < 2^32: vectors stay
  check_loads("u16 row_stride 2^29", huge(R29), big, {16, 2, true, false, true});
  // (2 * (2^29 - 8192) + 8192) * 2 = 2^31 - 16384
  check_loads("u16 row_stride 2^29 - 8192", huge(R29 - 8192), big, {16, 2, true, true, true});
  // (2 * (2^29 - 4096) + 8192) * 2 = 2^31 exactly: not below it
  check_loads("u16 row_stride 2^29 - 4096", huge(R29 - 4096), big, {16, 2, true, false, true});
  // 2 rows * 2^30 * 2 bytes = 2^32: no 16-byte vectors; 8-byte ones take 1 row of 2048 vectors: 2^31 bytes
  check_loads("u16 row_stride 2^30", huge(2 * R29), big, {8, 1, true, false, true});
  // 1 row * 2^31 * 2 bytes = 2^32: scalar min/max
  check_loads("u16 row_stride 2^31", huge(4 * R29), big, {0, 1, true, false, true});
}

int main() {
  check_load_paths();
  {
    const std::vector<fra_window> w = {{0, 0, 0, 0}};
    check_layout("an empty window", job_u16(64, 64, 1, 4096, w), nullptr, 1, true);
    const std::vector<fra_window> w2 = {{0, 0, 64, 64}, {0, 0, 0, 0}, {64, 0, 30, 50}};
    check_layout("an empty window between two", job_u16(100, 64, 1, 4096, w2), nullptr, 1, true);
    check_layout("no windows", job_u16(64, 64, 1, 4096, {}), nullptr, 1, true);
  }
  const std::vector<fra_window> edge = tiles(1800, 2500, 1000);
  for (int ch = 1; ch <= 2; ch++)
    for (int bs : {4096, 16}) {
      char what[64];
      snprintf(what, sizeof(what), "2500x1800 in tiles of 1000, %d ch, block %d", ch, bs);
      check_layout(what, job_u16(1800, 2500, ch, bs, edge), nullptr, 1, true);
    }
  {  // ranged: to the end from frame 0, nothing from the frame count on, a count past the end (clipped), a middle run
    const fra_job j = job_u16(1800, 2500, 2, 4096, edge);
    std::vector<int32_t> fr;
    for (size_t w = 0; w < edge.size(); w++) {
      const int nfr = (int)(((int64_t)edge[w].height * edge[w].width + 4095) / 4096);
      switch (w % 4) {
        case 0: fr.insert(fr.end(), {0, -1}); break;
        case 1: fr.insert(fr.end(), {nfr, -1}); break;
        case 2: fr.insert(fr.end(), {nfr - 3, 1000}); break;
        default: fr.insert(fr.end(), {5, 7}); break;
      }
    }
    check_layout("ranged plan", j, fr.data(), 1, true);
  }
  {
    std::vector<fra_window> w = tiles(4096, 4096, 512);  // (enough frames for several bands)
    std::reverse(w.begin(), w.end());
    check_layout("windows in descending row order", job_u16(4096, 4096, 1, 4096, w), nullptr, 1, false);
    w = tiles(4096, 4096, 512);
    std::swap(w[3], w[60]);
    check_layout("two windows out of row order", job_u16(4096, 4096, 1, 4096, w), nullptr, 1, false);
  }
  const std::vector<fra_window> big = tiles(4096, 4096, 512);  // 64 tiles in 8 rows, 4096 frames
  check_layout("64 tiles of 512x512", job_u16(4096, 4096, 1, 4096, big), nullptr, 1, true);
  check_layout("64 tiles of 512x512, 4 groups", job_u16(4096, 4096, 2, 4096, big), nullptr, 4, true);
  check_layout("64 tiles of 512x512, 99 groups", job_u16(4096, 4096, 1, 4096, big), nullptr, 99, true);
  printf(g_fail ? "%d FAILED\n" : "plan layout ok\n", g_fail);
  return g_fail ? 1 : 0;
}
