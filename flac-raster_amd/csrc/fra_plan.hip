// fra_plan.hip -- the plan: create (validate, lay out, allocate, upload), destroy, set_raster and the queries.
// No kernels here.  Per-job launch sequence (fra_exec.hip -> fra_kernels.hip):
//   k_norm_init, k_minmax, k_norm_finalize  (skipped when norm == 0)
//   k_analyze  [frames x channels]
//   k_frame_scan (frame sizes + decoupled look-back scan; k_group_offsets after a previous group)
//   k_assemble [frames]
#include <algorithm>
#include <new>

#include "fra_plan.h"
#include "fra_verify.h"

namespace fra {
int frame_scan_blocks(int nframes);

// CRC-16 (poly x^16+x^15+x^2+1) tables for k_crc16: slice-by-4 byte tables T[k][v] = CRC of v
// followed by k zero bytes, and M[i][0|1][b] = b * x^(8*2^i) (resp. b*x^8*x^(8*2^i)) mod P.
static uint32_t gf16_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 15; i >= 0; i--) {
    r <<= 1;
    if (r & 0x10000u) r ^= 0x18005u;
    if ((b >> i) & 1u) r ^= a;
  }
  return r & 0xFFFFu;
}
static std::vector<uint16_t> crc16_tables() {
  std::vector<uint16_t> tab(kCrcT16Off + 16 * 256);
  for (int v = 0; v < 256; v++) {
    uint32_t d = (uint32_t)v << 8;
    for (int b = 0; b < 8; b++) d = (d & 0x8000u) ? ((d << 1) ^ 0x8005u) : (d << 1);
    tab[v] = (uint16_t)d;
  }
  for (int k = 1; k < 4; k++)
    for (int v = 0; v < 256; v++) {
      const uint32_t p = tab[(k - 1) * 256 + v];
      tab[k * 256 + v] = (uint16_t)(((p << 8) & 0xFFFFu) ^ tab[p >> 8]);
    }
  for (int k = 0; k < 16; k++)  // slice-by-16 (k_assemble): T16[k] = T[k] for k < 4
    for (int v = 0; v < 256; v++) {
      if (k == 0) { tab[kCrcT16Off + v] = tab[v]; continue; }
      const uint32_t p = tab[kCrcT16Off + (k - 1) * 256 + v];
      tab[kCrcT16Off + k * 256 + v] = (uint16_t)(((p << 8) & 0xFFFFu) ^ tab[p >> 8]);
    }
  uint32_t X = 0x100;  // x^8
  for (int i = 0; i < 24; i++) {
    for (int b = 0; b < 256; b++) {
      tab[1024 + i * 512 + b] = (uint16_t)gf16_mul((uint32_t)b, X);
      tab[1024 + i * 512 + 256 + b] = (uint16_t)gf16_mul(gf16_mul((uint32_t)b, 0x100), X);
    }
    X = gf16_mul(X, X);
  }
  return tab;
}

template <typename T>
static hipError_t upload_vec(HipArena& res, const T** d, const std::vector<T>& v) {
  return res.upload(const_cast<T**>(d), v.data(), sizeof(T) * v.size());
}

static int plan_build(fra_plan* p) {
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p->ctx->device) == hipSuccess && ncu > 0)
      p->ncu = ncu;
  }
  const fra_job& j = p->job;
  PlanLayout& L = *p;
  if (int rc = build_layout(j, p->windows.data(), p->franges.empty() ? nullptr : p->franges.data(), env_groups(), L))
    return rc;
  const int nfr = (int)p->frames.size();
  const size_t nst = std::max<size_t>(1, p->streams.size());
  const size_t nsf = (size_t)std::max(1, nfr) * p->cmax;
  HipArena& res = p->res;
  JobArgs& a = p->args;
  (void)hipSetDevice(p->ctx->device);
  // a slot set / a norm set (a plan that is not pipelined has one of each)
  auto make_slots = [&](SlotSet& s) -> int {
    HIPCHK(res.alloc(&s.sf, sizeof(SfDesc) * nsf));
    HIPCHK(res.alloc(&s.fbytes, sizeof(unsigned long long) * (nfr + 1)));
    HIPCHK(res.alloc(&s.foff, sizeof(unsigned long long) * (nfr + 1)));
    HIPCHK(res.alloc(&s.tmp, sizeof(uint32_t) * (size_t)p->tmp_stride * nsf));
    HIPCHK(res.alloc(&s.fmeta, sizeof(uint32_t) * kMetaWords * std::max(1, nfr)));
    return FRA_OK;
  };
  auto make_norm = [&](NormSet& n) -> int {
    HIPCHK(res.alloc_zero(&n.norm, sizeof(NormDev) * nst));
    if (p->lut_stride) HIPCHK(res.alloc(&n.lut, sizeof(int32_t) * (size_t)p->lut_stride * nst));
    return FRA_OK;
  };
  if (int rc = make_slots(p->slot[0])) return rc;
  if (int rc = make_norm(p->nset[0])) return rc;
  HIPCHK(res.alloc(&p->d_out, p->out_cap));
  // the job's tables
  HIPCHK(res.upload(&p->d_streams, p->streams.data(), sizeof(StreamDev) * p->streams.size()));
  a.streams = p->d_streams;
  HIPCHK(upload_vec(res, &a.frames, p->frames));
  HIPCHK(upload_vec(res, &a.win, p->wtab));
  HIPCHK(upload_vec(res, &a.wrange, p->wrange));
  HIPCHK(upload_vec(res, &a.wplat, p->wplat));
  std::vector<float>().swap(p->wtab);  // (the device holds it now)
  {  // per-frame analysis descriptors (WaveDev: the load phase's metadata in one scalar load)
    std::vector<WaveDev> wv(std::max(1, nfr));
    for (int g = 0; g < nfr; g++) {
      const FrameDev& fr = p->frames[g];
      const StreamDev& st = p->streams[fr.stream];
      WaveDev& w = wv[g];
      w.off0 = st.base_off + (int64_t)fr.row0 * st.row_stride;
      w.band_stride = st.band_stride;
      w.row_stride = (uint32_t)st.row_stride;
      w.width = (uint32_t)st.width;
      w.col0 = (uint32_t)fr.col0;
      w.stream = fr.stream;
      w.n = fr.n;
      w.win = fr.win;
      w.bps = st.bps;
      w.nch = st.ms ? 2 : st.channels;
      w.channels = st.channels;
      w.ms = st.ms;
      w.norm = st.norm;
    }
    HIPCHK(upload_vec(res, &a.wave, wv));
  }
  HIPCHK(upload_vec(res, &a.crctab, crc16_tables()));
  {
    // look-back words (zero: no tag yet) and tickets of every scan slot, sized for the whole plan
    const size_t nscan = p->groups.size();
    // any group of <= nfr frames needs <= 256 words by default, or nfr's count (one frame per thread when forced)
    p->look_stride = std::max({256, frame_scan_blocks(nfr), (nfr + 255) / 256});
    HIPCHK(res.alloc_zero(&p->d_look, sizeof(unsigned long long) * (size_t)p->look_stride * 2 * nscan));
    HIPCHK(res.alloc_zero(&p->d_ticket, sizeof(unsigned long long) * nscan));
    HIPCHK(res.alloc_zero(&p->d_err, sizeof(uint32_t)));
    HIPCHK(res.alloc(&p->d_gbase, sizeof(unsigned long long) * (std::max(p->groups.size(), p->hbands.size()) + 1)));
    p->aux.resize(p->groups.size() - 1);
    for (auto& st : p->aux) HIPCHK(res.stream(&st));
    p->gev.resize(1 + 2 * p->groups.size());
    for (auto& e : p->gev) HIPCHK(res.event(&e));
  }
  int prio_lo = 0, prio_hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  if (p->wave_ok) {
    HIPCHK(res.upload(&p->d_part, p->part.data(), sizeof(int32_t) * p->part.size()));
    if (!p->part.empty()) {
      HIPCHK(res.stream(&p->pside, prio_hi));
      HIPCHK(res.event(&p->ev_pfork));
      HIPCHK(res.event(&p->ev_pjoin));
    }
  }
  a.out = p->d_out;
  a.err = p->d_err;
  a.out_cap = p->out_cap;
  a.tmp_stride = p->tmp_stride;
  a.lut_stride = p->lut_stride;
  a.nframes_total = nfr;
  a.cmax = p->cmax;
  a.blocksize = j.blocksize;
  a.level = j.level;
  a.nwin = std::max(1, p->nwin);
  a.off32 = p->ld_off32 ? 1 : 0;
  use_buffers(p, 0, 0);
  for (auto& e : p->ev) HIPCHK(res.event(&e, hipEventDefault));
  // cross-execute pipelining: more slot and norm sets.  Large plans only (>= 1024 frames: a C4 scene split 8 ways,
  // ~3.7k frames per rank, stays pipelined); small ones (the pyflac shim, single tiles) execute once per plan
  const bool want = env_pipe() && p->groups.size() == 1 && nfr >= env_pipe_min_frames();
  const size_t extra = sizeof(SfDesc) * nsf + sizeof(uint32_t) * (size_t)p->tmp_stride * nsf +
                       sizeof(uint32_t) * kMetaWords * nfr + 2 * sizeof(unsigned long long) * (nfr + 1) +
                       (fra_plan::kNormSets - 1) * (sizeof(NormDev) * nst + sizeof(int32_t) * (size_t)p->lut_stride * nst);
  size_t freeb = 0, totalb = 0;
  if (!(want && hipMemGetInfo(&freeb, &totalb) == hipSuccess && extra <= freeb / 3)) return FRA_OK;
  p->pipe = true;
  for (int n = 1; n < fra_plan::kNormSets; n++)
    if (int rc = make_norm(p->nset[n])) return rc;
  for (auto& n : p->nset) HIPCHK(res.event(&n.ev_free));
  // background streams at the lowest priority (the plan's stream is created at the highest)
  HIPCHK(res.stream(&p->nstream, prio_lo));
  HIPCHK(res.event(&p->ev_raster));
  // three slot sets (r05: with the 16-bit k_analyze_w instance C4 neutral, its 8-way share -4.6 %, C3 -2.3 %, C5
  // quarter -0.7 %, profiles/r05_ab_background.txt) when twice the extra set fits a third of the free memory,
  // else two
  p->nslot = (hipMemGetInfo(&freeb, &totalb) == hipSuccess && 2 * extra <= freeb / 3) ? 3 : 2;
  for (int b = 1; b < p->nslot; b++)
    if (int rc = make_slots(p->slot[b])) return rc;
  HIPCHK(res.stream(&p->pack, prio_lo));
  // 16-bit plans: C4 -1.2 %, C3 -2.4 % (r03 v14); 32-bps plans too since the background assembly that the
  // early start displaced is gone (r03: C5 +5 % with it; r04: C5 106.50 -> 106.24 ms,
  // profiles/r04_ab_dual_streams_32bps.txt)
  for (auto& st : p->astream) HIPCHK(res.stream(&st, prio_hi));
  if (p->wave_ok) {  // the k_analyze_w instance counters (fra_plan::kCnt ring)
    HIPCHK(res.alloc_zero(&p->d_cnt17, sizeof(uint32_t) * fra_plan::kCnt));
    HIPCHK(res.pinned(&p->h_cnt17, sizeof(uint32_t) * fra_plan::kCnt, hipHostMallocPortable));
    for (auto& c : p->cnt) HIPCHK(res.event(&c.ev));
  }
  for (auto& s : p->slot) {
    HIPCHK(res.event(&s.ev_scan));
    HIPCHK(res.event(&s.ev_pack));
    HIPCHK(res.event(&s.ev_norm));
    HIPCHK(res.event(&s.ev_ana));
    HIPCHK(res.event(&s.ev_part));
  }
  return FRA_OK;
}

void use_buffers(fra_plan* p, int b, int nb) {
  const SlotSet& s = p->slot[b];
  const NormSet& n = p->nset[nb];
  JobArgs& a = p->args;
  a.sf = s.sf; a.tmp = s.tmp; a.fmeta = s.fmeta;
  a.frame_bytes = s.fbytes; a.frame_off = s.foff;
  a.norm = n.norm; a.lut = n.lut;
  p->cur = b;
  p->curn = nb;
}
// make the plan's stream wait for every k_assemble still running on the pack stream, then use set 0
int drain_pipeline(fra_plan* p) {
  if (!p->pipe) return FRA_OK;
  for (auto& s : p->slot) {
    if (s.pack_pending) {
      HIPCHK(hipStreamWaitEvent(p->ctx->stream, s.ev_pack, 0));
      s.pack_pending = false;
    }
    // (an analysis on its stream is followed by its chain + assembly on the pack stream: covered above;
    // the wait below also orders a pipelined execute's analysis before the serial work that follows)
    if (s.ana_pending) HIPCHK(hipStreamWaitEvent(p->ctx->stream, s.ev_ana, 0));
    s.ana_pending = false;  // (covered by the resync below)
  }
  for (auto& n : p->nset) {  // (norm stream: its partial-subframe lists)
    if (n.free_pending) HIPCHK(hipStreamWaitEvent(p->ctx->stream, n.ev_free, 0));
    n.free_pending = false;
  }
  // serial executes and host raster copies now go onto the plan's stream; when pipelining resumes, the
  // first background norm stage waits for ALL of it (an event recorded on the plan's stream at that
  // point): a pipelined analysis still reading a norm set or a raster copy queued before this drain
  // cannot be overtaken
  p->resync = true;
  p->raster_dirty = false;
  use_buffers(p, 0, 0);
  return FRA_OK;
}
// device-detected inconsistencies (JobArgs::err): bit 0 a frame-scan ticket past its grid, bit 1 a frame the
// assembly did not write because its sizes left the output or its slots -- the stream is not handed back.  The
// word is sticky: once set, every later sync / result / host encode of the plan reports it (call after the work
// that may set it has completed)
int check_dev_err(fra_plan* p) {
  uint32_t e = 0;
  HIPCHK(hipMemcpy(&e, p->d_err, sizeof(e), hipMemcpyDeviceToHost));
  if (e) return set_err(FRA_E_STATE, "device error word 0x%x (%s%s)", e, (e & 1u) ? "frame-scan ticket desync " : "",
                        (e & 2u) ? "frame outside its output/slot bounds" : "");
  return FRA_OK;
}
int plan_sync_all(fra_plan* p) {
  if (p->pipe) {
    for (auto& st : p->astream) HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipStreamSynchronize(p->nstream));
    HIPCHK(hipStreamSynchronize(p->pack));
  }
  HIPCHK(hipStreamSynchronize(p->ctx->stream));
  return check_dev_err(p);
}
int plan_own_raster(fra_plan* p) {
  if (!p->d_raster_owned && p->raster_bytes) HIPCHK(p->res.alloc(&p->d_raster_owned, p->raster_bytes));
  return FRA_OK;
}

void collect_times(fra_plan* p) {
  if (!p->pending_times) return;
  (void)hipEventSynchronize(p->ev[4]);
  for (int k = 0; k < 4; k++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p->ev[k], p->ev[k + 1]) == hipSuccess) p->ms[k] += ms;
  }
  p->nexec++;
  p->pending_times = false;
}

static int plan_create(fra_ctx* ctx, const fra_job* job, const int32_t* franges, fra_plan** out) {
  if (!ctx || !job || !out) return set_err(FRA_E_INVALID, "null argument");
  if (job->channels < 1 || job->channels > 8) return set_err(FRA_E_INVALID, "channels must be 1..8 (got %d)", job->channels);
  if (job->blocksize < 16 || job->blocksize > kMaxBlock)
    return set_err(FRA_E_INVALID, "blocksize must be 16..%d (got %d)", kMaxBlock, job->blocksize);
  if (job->level < 0 || job->level > 8) return set_err(FRA_E_INVALID, "level must be 0..8 (got %d)", job->level);
  if (job->dtype < FRA_U8 || job->dtype > FRA_F64) return set_err(FRA_E_INVALID, "bad dtype %d", job->dtype);
  if (job->norm != 0 && job->norm != 16 && job->norm != 24) return set_err(FRA_E_INVALID, "norm must be 0, 16 or 24");
  if (job->norm == 0 && job->dtype != FRA_I16 && job->dtype != FRA_I32)
    return set_err(FRA_E_INVALID, "norm == 0 (pre-normalised audio) needs int16 or int32 samples");
  if (job->nwindows < 0 || (job->nwindows > 0 && !job->windows)) return set_err(FRA_E_INVALID, "bad windows");
  if (job->first_frame < 0) return set_err(FRA_E_INVALID, "first_frame must be >= 0");
  // (the analysis descriptors hold the row stride in 32 bits: WaveDev)
  if (job->band_stride < 0 || job->row_stride < 0 || job->col_stride < 1 || job->row_stride > (int64_t)UINT32_MAX)
    return set_err(FRA_E_INVALID, "strides must be >= 0 (col_stride >= 1) with row_stride < 2^32 elements");
  for (int w = 0; w < job->nwindows; w++) {
    const fra_window& wd = job->windows[w];
    if (wd.height < 0 || wd.width < 0 || wd.row_off < 0 || wd.col_off < 0 || (wd.height > 0) != (wd.width > 0))
      return set_err(FRA_E_INVALID, "window %d invalid (%d,%d,%d,%d)", w, wd.row_off, wd.col_off, wd.height, wd.width);
  }
  if (franges) {
    // a range must start inside its window's stream (a count past the end is clipped to it): a first frame past
    // the end or a negative count other than -1 (to the end) is a malformed work item of a multi-GPU split
    // 
    for (int w = 0; w < job->nwindows; w++) {
      const fra_window& wd = job->windows[w];
      const int64_t nfr_all = ((int64_t)wd.width * wd.height + job->blocksize - 1) / job->blocksize;
      const int32_t f0 = franges[2 * w], n = franges[2 * w + 1];
      if (f0 < 0 || f0 > nfr_all || n < -1)
        return set_err(FRA_E_INVALID, "window %d: frame range (%d, %d) outside its %lld frames", w, f0, n,
                       (long long)nfr_all);
    }
  }
  fra_plan* p = new (std::nothrow) fra_plan();
  if (!p) return set_err(FRA_E_NOMEM, "out of host memory");
  p->ctx = ctx;
  p->job = *job;
  p->windows.assign(job->windows, job->windows + job->nwindows);
  p->job.windows = p->windows.data();
  if (franges) p->franges.assign(franges, franges + 2 * (size_t)job->nwindows);
  int rc = plan_build(p);
  if (rc == FRA_OK && job->raster) rc = fra_plan_set_raster(p, job->raster, job->raster_on_device);
  if (rc != FRA_OK) {
    KeepError keep;
    fra_plan_destroy(p);  // releases whatever was made
    return rc;
  }
  *out = p;
  return FRA_OK;
}

}  // namespace fra

using namespace fra;

extern "C" {

int fra_plan_create(fra_ctx* ctx, const fra_job* job, fra_plan** out) { return plan_create(ctx, job, nullptr, out); }
int fra_plan_create_ranged(fra_ctx* ctx, const fra_job* job, const int32_t* frame_ranges, fra_plan** out) {
  if (!frame_ranges) return set_err(FRA_E_INVALID, "null frame_ranges");
  return plan_create(ctx, job, frame_ranges, out);
}

void fra_plan_destroy(fra_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  delete p;
}

int fra_plan_set_raster(fra_plan* p, const void* raster, int32_t on_device) {
  if (!p) return set_err(FRA_E_INVALID, "null plan");
  (void)hipSetDevice(p->ctx->device);
  if (on_device) {
    p->d_raster = raster;
  } else {
    if (int rc = plan_own_raster(p)) return rc;
    // the copy must not overtake a pipelined analysis (its own stream) still reading the old rows
    for (auto& s : p->slot)
      if (s.ana_pending) HIPCHK(hipStreamWaitEvent(p->ctx->stream, s.ev_ana, 0));
    if (p->raster_bytes) {
      HIPCHK(hipMemcpyAsync(p->d_raster_owned, raster, p->raster_bytes, hipMemcpyHostToDevice, p->ctx->stream));
      if (p->pipe) {  // the next pipelined norm stage (norm stream) reads the new raster after this copy
        HIPCHK(hipEventRecord(p->ev_raster, p->ctx->stream));
        p->raster_dirty = true;
      }
    }
    p->d_raster = p->d_raster_owned;
  }
  p->args.raster = p->d_raster;
  p->job.raster = raster;
  p->job.raster_on_device = on_device;
  return FRA_OK;
}

int fra_plan_sync(fra_plan* p) {
  if (!p) return set_err(FRA_E_INVALID, "null plan");
  (void)hipSetDevice(p->ctx->device);
  if (int rc = plan_sync_all(p)) return rc;
  if (p->timing) collect_times(p);
  return FRA_OK;
}

int fra_plan_result(fra_plan* p, fra_stream_info* infos, uint64_t* total) {
  if (!p) return set_err(FRA_E_INVALID, "null plan");
  if (!p->executed) return set_err(FRA_E_STATE, "plan not executed");
  (void)hipSetDevice(p->ctx->device);
  if (int rc = plan_sync_all(p)) return rc;
  const int nfr = p->args.nframes_total;
  std::vector<unsigned long long> off(nfr + 1);
  HIPCHK(hipMemcpy(off.data(), p->args.frame_off, sizeof(unsigned long long) * (nfr + 1), hipMemcpyDeviceToHost));
  // exclusive scan of [bytes..., 0]: off[nfr] = total
  if (total) *total = off[nfr];
  if (infos) {
    std::vector<NormDev> nd(p->streams.size());
    if (!nd.empty())
      HIPCHK(hipMemcpy(nd.data(), p->args.norm, sizeof(NormDev) * nd.size(), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < p->streams.size(); s++) {
      const StreamDev& st = p->streams[s];
      fra_stream_info& in = infos[s];
      in.offset = off[st.first_frame];
      in.frame_bytes = off[st.first_frame + st.nframes] - off[st.first_frame];
      in.data_min = p->job.norm ? nd[s].mn : 0.0;
      in.data_max = p->job.norm ? nd[s].mx : 0.0;
      in.sample_rate = st.sample_rate;
      in.bps = st.bps;
      in.channels = st.channels;
      in.nframes = st.nframes;
    }
  }
  return FRA_OK;
}

int fra_plan_download(fra_plan* p, uint8_t* host_out, uint64_t capacity) {
  uint64_t total = 0;
  int rc = fra_plan_result(p, nullptr, &total);
  if (rc) return rc;
  if (capacity < total) return set_err(FRA_E_INVALID, "capacity %llu < %llu", (unsigned long long)capacity,
                                       (unsigned long long)total);
  if (total) HIPCHK(hipMemcpy(host_out, p->d_out, total, hipMemcpyDeviceToHost));
  return FRA_OK;
}

int fra_plan_frame_offsets(fra_plan* p, uint64_t* offsets, uint64_t n) {
  if (!p || !offsets) return set_err(FRA_E_INVALID, "null argument");
  if (!p->executed) return set_err(FRA_E_STATE, "plan not executed");
  const uint64_t nfr = (uint64_t)p->args.nframes_total;
  if (n != nfr + 1) return set_err(FRA_E_INVALID, "frame offsets: n = %llu, plan has %llu frames + 1",
                                   (unsigned long long)n, (unsigned long long)nfr);
  (void)hipSetDevice(p->ctx->device);
  if (int rc = plan_sync_all(p)) return rc;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64");
  HIPCHK(hipMemcpy(offsets, p->args.frame_off, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
  return FRA_OK;
}

int fra_plan_device_output(fra_plan* p, const uint8_t** dev_ptr, uint64_t* capacity) {
  if (!p) return set_err(FRA_E_INVALID, "null plan");
  *dev_ptr = p->d_out;
  *capacity = p->out_cap;
  return FRA_OK;
}

int fra_plan_verify(fra_plan* p, fra_verify_report* reports, int32_t* bad_windows) {
  if (!p || !reports || !bad_windows) return set_err(FRA_E_INVALID, "null argument");
  if (!p->executed) return set_err(FRA_E_STATE, "plan not executed");
  (void)hipSetDevice(p->ctx->device);
  if (int rc = plan_sync_all(p)) return rc;
  // the last execute's frames: its slot set's offsets, relative to each window's first frame
  const size_t nfr = (size_t)p->args.nframes_total, nst = p->streams.size();
  std::vector<uint64_t> off(nfr + 1);
  HIPCHK(hipMemcpy(off.data(), p->args.frame_off, sizeof(uint64_t) * (nfr + 1), hipMemcpyDeviceToHost));
  std::vector<uint64_t> rel(nfr + nst + 1);
  std::vector<fra_decode_item> items(nst);
  std::vector<int32_t> first(nst, 0);
  for (size_t s = 0; s < nst; s++) {
    const StreamDev& st = p->streams[s];
    uint64_t* r = rel.data() + st.first_frame + s;
    for (int f = 0; f <= st.nframes; f++) r[f] = off[(size_t)st.first_frame + f] - off[st.first_frame];
    fra_decode_item& it = items[s];
    it = fra_decode_item{};
    it.offset = off[st.first_frame];
    it.bytes = r[st.nframes];
    it.window = p->windows[s];
    it.frame_offsets = r;
    it.nframes = st.nframes;
    it.channels = st.channels;
    it.bps = st.bps;
    it.blocksize = p->job.blocksize;
    if (st.nframes) first[s] = p->frames[st.first_frame].index;  // (a ranged plan's first frame of the stream)
  }
  fra_verify_source src{};
  src.raster = p->d_raster;
  src.dtype = p->job.dtype;
  src.norm = p->job.norm;
  src.band_stride = p->job.band_stride;
  src.row_stride = p->job.row_stride;
  src.col_stride = p->job.col_stride;
  src.norm_rows = p->nset[p->curn].norm;  // the last execute's min / max keys, read on the device
  return fra_internal_verify_device(p->ctx, p->d_out, off[nfr], items.data(), (int32_t)nst, p->job.channels, &src,
                                    first.data(), reports, bad_windows);
}

int fra_plan_enable_timing(fra_plan* p, int32_t on) {
  if (!p) return set_err(FRA_E_INVALID, "null plan");
  p->timing = on != 0;
  for (float& m : p->ms) m = 0;
  p->nexec = 0;
  p->pending_times = false;
  return FRA_OK;
}

int fra_plan_timing(fra_plan* p, float* ms4, int32_t* n) {
  if (!p) return set_err(FRA_E_INVALID, "null plan");
  collect_times(p);
  for (int k = 0; k < 4; k++) ms4[k] = p->ms[k];
  *n = p->nexec;
  return FRA_OK;
}

int fra_plan_set_first_frame(fra_plan* p, int32_t first_frame) {
  if (!p || first_frame < 0) return set_err(FRA_E_INVALID, "bad argument");
  (void)hipSetDevice(p->ctx->device);
  // pipelined executes still in flight read frame_number0 on the analysis / pack streams (k_frame_scan):
  // let them finish before the table changes under them
  if (int rc = plan_sync_all(p)) return rc;
  p->job.first_frame = first_frame;
  for (auto& st : p->streams) st.frame_number0 = (uint32_t)first_frame;
  if (!p->streams.empty())  // complete before this call returns, so every later execute reads it
    HIPCHK(hipMemcpyAsync(p->d_streams, p->streams.data(), sizeof(StreamDev) * p->streams.size(),
                          hipMemcpyHostToDevice, p->ctx->stream));
  HIPCHK(hipStreamSynchronize(p->ctx->stream));  // the host array may change again before it is read
  return FRA_OK;
}

int fra_plan_flags(fra_plan* p, int32_t* flags) {
  if (!p || !flags) return set_err(FRA_E_INVALID, "null argument");
  // (vector loads as an execute will decide them: the device raster's alignment, or hipMalloc's for host rasters)
  set_vec8(p);
  const ExecEnv env = env_exec();
  const int k17 = env.keep17 >= 0 ? env.keep17 : p->k17;
  const int mv = p->job.norm != 0 ? minmax_vec(p) : 0;
  *flags = (p->pipe ? FRA_PLAN_PIPELINED : 0) | (wave_path(p, env) ? FRA_PLAN_WAVE : 0) | (k17 ? FRA_PLAN_KEEP17 : 0) |
           (p->args.vec8 ? FRA_PLAN_LOAD_VEC8 : 0) | (mv == 16 ? FRA_PLAN_MINMAX_VEC16 : 0) |
           (mv == 8 ? FRA_PLAN_MINMAX_VEC8 : 0) | (p->args.off32 ? FRA_PLAN_OFF32 : 0);
  return FRA_OK;
}

int fra_plan_capacity(fra_plan* p, uint64_t* capacity, int32_t* host_bands) {
  if (!p) return set_err(FRA_E_INVALID, "null plan");
  if (capacity) *capacity = p->out_cap;
  if (host_bands) *host_bands = (int32_t)p->hbands.size();
  return FRA_OK;
}

int fra_plan_host_band_rows(fra_plan* p, int64_t* max_rows) {
  if (!p || !max_rows) return set_err(FRA_E_INVALID, "null argument");
  int64_t m = 0;
  for (const auto& hb : p->hbands) m = std::max(m, hb.r1 - hb.r0);
  *max_rows = m;
  return FRA_OK;
}

}  // extern "C"
