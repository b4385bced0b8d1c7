// fra_layout.h -- the layout of a plan as pure host arithmetic: streams and frames of a job (ranged plans
// included), output capacity, vector-load eligibility, window tables, frame groups, host bands and the
// partial-subframe list.  No HIP: plan_build (fra_plan.hip) computes a layout, allocates and uploads;
// tools/plan_layout_check.cpp exercises it without a GPU.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <map>
#include <vector>

#include "fra_host.h"
#include "fra_internal.h"

namespace fra {

// frame groups: contiguous window runs [w0, w1) with frames [f0, f1)
struct Group { int w0, w1, f0, f1; };
// host pipeline (fra_plan_encode_host): row bands of windows; band b copies raster rows [r0, r1)
// before its kernels run (rows already copied by earlier bands are not copied again)
struct HBand { Group g; int64_t r0, r1; };

struct PlanLayout {
  int src = 0;
  bool b32 = false;
  bool mid_side = false;  // mid-side: four virtual channels (L, R, M, S) analysed per frame
  int nwin = 0;
  int cmax = 1;
  std::vector<StreamDev> streams;
  std::vector<FrameDev> frames;
  int max_segs = 0;
  int mm_vec = 0, mm_rows = 1, mm_max_rows = 0;  // vectorised k_minmax shape (0 = scalar path)
  bool ld_vec8 = false;  // k_analyze 8-byte sample vectors possible (pointer alignment checked at execute)
  bool ld_off32 = false;  // k_analyze 32-bit lane offsets (JobArgs::off32)
  size_t raster_bytes = 0;
  size_t out_cap = 0;
  // window tables [ntables][max(1, nwin)][blocksize] (one table set per distinct block size, + 64 entries of
  // slack), the nonzero extent [lo, hi) of every window and its longest run of coefficients exactly 1.0f
  std::vector<int> win_sizes;
  std::vector<float> wtab;
  std::vector<int32_t> wrange, wplat;
  std::vector<Group> groups;  // FRA_GROUPS execution (size 1 = serial)
  Group all{0, 0, 0, 0};      // the whole plan as one group (timing mode)
  std::vector<HBand> hbands;
  // wave-path plans: the partial subframes k_analyze takes beside k_analyze_w (frame * 8 + channel, ascending;
  // a launch over frames [f0, f1) passes the entries in [8 f0, 8 f1))
  bool wave_ok = false;
  std::vector<int32_t> part;
  int64_t tmp_stride = 0;  // words per encoded-subframe slot
  int64_t lut_stride = 0;  // normalisation table entries per stream (0: no table)
};

// normalization.py:108-120 (calculate_audio_params, total_pixels = H*W of the encode unit)
inline int sample_rate_for_pixels(int64_t px) {
  if (px < 1000000) return 44100;
  if (px < 10000000) return 48000;
  if (px < 100000000) return 96000;
  return 192000;
}
// tukey(p) window as defined in DESIGN.md 3.4 (same formula as the oracle, computed on the host)
inline void tukey(float* w, int N, double p) {
  for (int i = 0; i < N; i++) w[i] = 1.0f;
  int Np = (int)(p / 2.0 * (double)N) - 1;
  if (Np > 0) {
    for (int n = 0; n <= Np; n++) {
      w[n] = (float)(0.5 - 0.5 * cos(M_PI * (double)n / (double)Np));
      w[N - Np - 1 + n] = (float)(0.5 - 0.5 * cos(M_PI * (double)(n + Np) / (double)Np));
    }
  }
}
inline void window_set(float* w, int N, int stride, int nsub) {
  if (nsub <= 0) return;
  tukey(w, N, 0.5);
  int idx = 1;
  for (int m = 2; m <= nsub; m++)
    for (int j = 0; j < m; j++, idx++) {
      float* o = w + (size_t)idx * stride;
      const int a = (int)((int64_t)j * N / m), b = (int)((int64_t)(j + 1) * N / m);
      for (int i = 0; i < N; i++) o[i] = 0.0f;
      if (b - a > 0) tukey(o + a, b - a, 0.5);
    }
}

// streams, frames and the output capacity; frame f of a window covers samples [f, f + 1) * blocksize of its stream
inline int layout_frames(const fra_job& j, const fra_window* windows, const int32_t* franges, PlanLayout& L) {
  L.src = j.dtype;
  int bps;
  if (j.norm == 16) bps = 16;
  else if (j.norm == 24) bps = 32;  // int32 audio -> 32-bps FLAC
  else bps = (j.dtype == FRA_I16 || j.dtype == FRA_U8 || j.dtype == FRA_I8) ? 16 : 32;
  L.b32 = bps == 32;
  // FRA-1 3.1b mid-side for 2-channel 16-bps streams at the levels whose libFLAC preset enables it:
  // four virtual channels (L, R, M, S) are analysed per frame, k_frame_scan keeps the cheapest pair
  L.mid_side = j.channels == 2 && bps == 16 && level_cfg(j.level).ms;
  L.cmax = L.mid_side ? 4 : j.channels;
  const int sbps_max = L.mid_side ? bps + 1 : bps;  // side samples carry one more bit
  std::map<int, int> win_index;  // block size -> window table index
  int64_t nf_total = 0;
  int64_t max_extent = 0;
  size_t out_cap = 0;
  for (int w = 0; w < j.nwindows; w++) {
    const fra_window& wd = windows[w];
    StreamDev st{};
    st.base_off = (int64_t)wd.row_off * j.row_stride + (int64_t)wd.col_off * j.col_stride;
    st.band_stride = j.band_stride;
    st.row_stride = j.row_stride;
    st.col_stride = j.col_stride;
    st.width = wd.width;
    st.height = wd.height;
    st.channels = j.channels;
    st.bps = bps;
    st.norm = j.norm;
    st.nsamples = (int64_t)wd.width * wd.height;
    st.sample_rate = j.sample_rate > 0 ? j.sample_rate : sample_rate_for_pixels(st.nsamples);
    st.first_frame = (int32_t)nf_total;
    st.frame_number0 = (uint32_t)j.first_frame;
    st.ms = L.mid_side ? 1 : 0;
    const int64_t nfr_all = (st.nsamples + j.blocksize - 1) / j.blocksize;
    // frame range of this window (fra_plan_create_ranged): frames [fa, fa + nfr) of its stream; the
    // normalisation still spans the whole window, frame numbers stay those of the whole stream
    int64_t fa = 0, nfr = nfr_all;
    if (franges) {
      fa = std::min<int64_t>(franges[2 * w], nfr_all);
      nfr = franges[2 * w + 1] < 0 ? nfr_all - fa : std::min<int64_t>(franges[2 * w + 1], nfr_all - fa);
    }
    st.nframes = (int32_t)nfr;
    if (st.nsamples > 0) {
      int64_t ext = st.base_off + (int64_t)(j.channels - 1) * j.band_stride + (int64_t)(wd.height - 1) * j.row_stride +
                    (int64_t)(wd.width - 1) * j.col_stride + 1;
      max_extent = std::max(max_extent, ext);
      const int segs = (wd.width + 4095) / 4096;
      L.max_segs = (int)std::max<int64_t>(L.max_segs, (int64_t)segs * wd.height);
    }
    for (int64_t f = fa; f < fa + nfr; f++) {
      FrameDev fr{};
      fr.stream = w;
      fr.index = (int32_t)f;
      const int64_t first = f * j.blocksize;
      fr.n = (int32_t)std::min<int64_t>(j.blocksize, st.nsamples - first);
      fr.row0 = (int32_t)(first / wd.width);
      fr.col0 = (int32_t)(first % wd.width);
      auto it = win_index.find(fr.n);
      if (it == win_index.end()) {
        int idx = (int)L.win_sizes.size();
        win_index[fr.n] = idx;
        L.win_sizes.push_back(fr.n);
        fr.win = idx;
      } else fr.win = it->second;
      L.frames.push_back(fr);
      out_cap += 16 + 2 + (size_t)j.channels * ((size_t)fr.n * sbps_max / 8 + 8);
    }
    nf_total += nfr;
    L.streams.push_back(st);
  }
  if (nf_total > INT32_MAX / 2)
    return fra_internal_set_error(FRA_E_INVALID, "too many frames (%lld)", (long long)nf_total);
  L.raster_bytes = (size_t)max_extent * elem_size(j.dtype);
  L.out_cap = out_cap + 64;
  // per-subframe slots for the encoded subframes (k_analyze -> k_assemble)
  L.tmp_stride = ((int64_t)j.blocksize * sbps_max + 64 + 31) / 32 + 4;
  // normalisation tables for <= 16-bit integer rasters (k_norm_lut -> gathered by k_analyze)
  if (j.norm != 0 && (j.dtype == FRA_U8 || j.dtype == FRA_I8 || j.dtype == FRA_U16 || j.dtype == FRA_I16) &&
      !L.streams.empty())
    L.lut_stride = elem_size(j.dtype) == 1 ? 256 : 65536;
  return FRA_OK;
}

// which vector loads the job's strides and windows allow (the raster pointer's alignment is checked at execute)
inline void layout_loads(const fra_job& j, PlanLayout& L) {
  // vectorised min/max: every window start, row, band and width a multiple of V = vec/itemsize
  L.mm_vec = 0;
  if (j.norm != 0 && j.col_stride == 1 && elem_size(j.dtype) <= 4) {
    for (int vb : {16, 8}) {
      const int64_t V = vb / elem_size(j.dtype);
      bool ok = V >= 2 && j.row_stride % V == 0 && (j.channels == 1 || j.band_stride % V == 0);
      int64_t max_nv = 1;
      for (int w = 0; ok && w < j.nwindows; w++) {
        const StreamDev& st = L.streams[w];
        if (st.nsamples == 0) continue;
        ok = st.base_off % V == 0 && st.width % V == 0 && st.width / V <= 65535;
        max_nv = std::max<int64_t>(max_nv, st.width / V);
      }
      if (!ok) continue;
      const int64_t rows = std::max<int64_t>(1, std::min<int64_t>(64, 2048 / max_nv));
      if (rows * max_nv * max_nv >= (int64_t(1) << 32)) continue;
      if (rows * j.row_stride * elem_size(j.dtype) >= (int64_t(1) << 32)) continue;  // 32-bit byte offsets
      L.mm_vec = vb;
      L.mm_rows = (int)rows;
      L.mm_max_rows = 0;
      for (const StreamDev& st : L.streams) L.mm_max_rows = std::max(L.mm_max_rows, (int)st.height);
      break;
    }
  }
  // k_analyze 8-byte sample vectors: V = 8/itemsize samples never straddle a row and stay aligned
  const int64_t V = 8 / std::max(1, elem_size(j.dtype));
  bool ok = elem_size(j.dtype) <= 4 && j.col_stride == 1 && j.blocksize % V == 0 && j.row_stride % V == 0 &&
            (j.channels == 1 || j.band_stride % V == 0);
  for (int w = 0; ok && w < j.nwindows; w++) {
    const StreamDev& st = L.streams[w];
    if (st.nsamples) ok = st.base_off % V == 0 && st.width % V == 0;
  }
  L.ld_vec8 = ok;
  // 32-bit lane offsets of the fast load path: a frame's rows of one channel span < 2^31 bytes
  bool o32 = j.row_stride >= 0;
  for (int w = 0; o32 && w < j.nwindows; w++) {
    const StreamDev& st = L.streams[w];
    if (!st.nsamples) continue;
    const int64_t rows = (j.blocksize + st.width - 1) / st.width + 1;
    o32 = (rows * j.row_stride + st.width) * elem_size(j.dtype) < (int64_t(1) << 31);
  }
  L.ld_off32 = o32;
}

inline void layout_windows(const fra_job& j, PlanLayout& L) {
  const int nsub = level_cfg(j.level).nsub;
  L.nwin = num_windows(nsub);
  const int nw = std::max(1, L.nwin), nt = (int)std::max<size_t>(1, L.win_sizes.size());
  const size_t wn = (size_t)nt * nw * j.blocksize;
  // exact size: k_analyze reads entries [0, n) of the table of block size n only (load_window)
  // + slack: k_analyze_w reads a whole chunk's look-ahead of coefficients without a bound (its samples past n
  // are zero), which may run 16 + MAXLAG entries past the last row
  L.wtab.assign(wn + 64, 0.0f);
  for (size_t t = 0; t < L.win_sizes.size(); t++)
    window_set(L.wtab.data() + t * nw * j.blocksize, L.win_sizes[t], j.blocksize, nsub);
  // nonzero extent [lo, hi) of every window (k_analyze: waves outside it skip the autocorrelation)
  L.wrange.assign(2 * (size_t)nt * nw, 0);
  // longest run of coefficients exactly 1.0f (the tukey plateau): its products are the samples themselves
  L.wplat.assign(2 * (size_t)nt * nw, 0);
  for (int t = 0; t < nt; t++)
    for (int w = 0; w < nw; w++) {
      const float* o = L.wtab.data() + ((size_t)t * nw + w) * j.blocksize;
      int lo = j.blocksize, hi = 0;
      int best = 0, blo = 0, run = 0;
      for (int i = 0; i < j.blocksize; i++) {
        if (o[i] != 0.0f) { lo = std::min(lo, i); hi = i + 1; }
        run = o[i] == 1.0f ? run + 1 : 0;
        if (run > best) { best = run; blo = i + 1 - run; }
      }
      L.wrange[2 * ((size_t)t * nw + w)] = lo < hi ? lo : 0;
      L.wrange[2 * ((size_t)t * nw + w) + 1] = lo < hi ? hi : 0;
      L.wplat[2 * ((size_t)t * nw + w)] = blo;
      L.wplat[2 * ((size_t)t * nw + w) + 1] = blo + best;
    }
}

// frame groups: `want` (FRA_GROUPS, default 1: measured no gain on C4) contiguous
// window runs of about equal frame count; one group for small plans, where launch latency dominates
inline void layout_groups(int want, PlanLayout& L) {
  const int ns = (int)L.streams.size(), nfr = (int)L.frames.size();
  const int G = nfr < 4096 ? 1 : std::max(1, std::min(8, want));
  L.all = {0, ns, 0, nfr};
  L.groups.clear();
  int w = 0, f = 0;
  for (int g = 0; g < G && w < ns; g++) {
    const int64_t target = (int64_t)nfr * (g + 1) / G;
    Group gr{w, w, f, f};
    while (w < ns && (g == G - 1 || f < target || gr.f1 == gr.f0)) {
      f += L.streams[w].nframes;
      w++;
      gr.w1 = w;
      gr.f1 = f;
    }
    L.groups.push_back(gr);
  }
  if (L.groups.empty()) L.groups.push_back(L.all);
  L.groups.back().w1 = ns;
  L.groups.back().f1 = nfr;
}

// Row bands for the host pipeline: runs of windows sharing a row offset (a row of tiles), merged until a
// band holds >= 1/16 of the frames (one band for small plans, where launch latency dominates).  Band b
// copies the raster rows its windows cover that no earlier band copied; if the windows' row ranges are
// not monotone the plan falls back to one band covering every row.
inline void layout_host_bands(const fra_window* windows, PlanLayout& L) {
  L.hbands.clear();
  const int ns = (int)L.streams.size(), nfr = (int)L.frames.size();
  if (ns == 0) return;
  const int64_t min_frames = nfr < 2048 ? (int64_t)nfr + 1 : std::max<int64_t>(1, nfr / 16);
  std::vector<Group> bands;
  int w = 0, f = 0;
  while (w < ns) {
    Group g{w, w, f, f};
    while (w < ns && (g.f1 - g.f0 < min_frames || g.w1 == g.w0)) {
      const int r = windows[w].row_off;
      while (w < ns && windows[w].row_off == r) {  // a whole row of windows
        f += L.streams[w].nframes;
        w++;
      }
      g.w1 = w;
      g.f1 = f;
    }
    bands.push_back(g);
  }
  if (bands.size() > 1 && bands.back().f1 - bands.back().f0 < min_frames / 2) {  // fold a small tail band
    bands[bands.size() - 2].w1 = bands.back().w1;
    bands[bands.size() - 2].f1 = bands.back().f1;
    bands.pop_back();
  }
  int64_t lo_all = INT64_MAX, hi_all = 0, prev_lo = -1, hi = 0;
  bool mono = true;
  for (const auto& g : bands) {
    int64_t lo = INT64_MAX, hb = 0;
    for (int k = g.w0; k < g.w1; k++)
      if (L.streams[k].nsamples > 0) {
        lo = std::min<int64_t>(lo, windows[k].row_off);
        hb = std::max<int64_t>(hb, (int64_t)windows[k].row_off + windows[k].height);
      }
    if (lo == INT64_MAX) { lo = hi; hb = hi; }
    if (lo < prev_lo) mono = false;
    prev_lo = lo;
    lo_all = std::min(lo_all, lo);
    hi_all = std::max(hi_all, hb);
    L.hbands.push_back({g, std::max(lo, hi), std::max(std::max(lo, hi), hb)});
    hi = std::max(hi, hb);
  }
  if (!mono) {
    L.hbands.clear();
    L.hbands.push_back({L.all, lo_all == INT64_MAX ? 0 : lo_all, hi_all});
  }
}

// plans k_analyze_w may take (wave_path decides per execute), and their partial subframes (frame * 8 + channel,
// ascending): k_analyze's share of a wave-path launch
inline void layout_wave(const fra_job& j, PlanLayout& L) {
  L.part.clear();
  L.wave_ok = j.blocksize == kMaxBlock &&
              ((!L.b32 && j.level >= 3 && j.level <= 6 && j.norm != 0 && elem_size(j.dtype) <= 2 && j.dtype != FRA_F64) ||
               (L.b32 && j.level >= 7 && j.norm == 24 && j.dtype == FRA_F32 && j.channels == L.cmax));
  if (!L.wave_ok) return;
  for (int g = 0; g < (int)L.frames.size(); g++) {
    const FrameDev& fr = L.frames[g];
    if (fr.n == j.blocksize) continue;
    const StreamDev& st = L.streams[fr.stream];
    for (int c = 0; c < (st.ms ? 2 : st.channels); c++) L.part.push_back(g * 8 + c);
  }
}

// the layout of a validated job (plan_create); franges null, or [2 w] first frame and [2 w + 1] count (-1: to the
// end) of window w; `groups` = the frame groups wanted (FRA_GROUPS)
inline int build_layout(const fra_job& j, const fra_window* windows, const int32_t* franges, int groups,
                        PlanLayout& L) {
  L = PlanLayout{};
  if (int rc = layout_frames(j, windows, franges, L)) return rc;
  layout_loads(j, L);
  layout_windows(j, L);
  layout_groups(groups, L);
  layout_host_bands(windows, L);
  layout_wave(j, L);
  return FRA_OK;
}

}  // namespace fra
