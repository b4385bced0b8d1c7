// fra_exec.hip -- fra_plan_execute: the stages of a frame group (norm stage, partial-subframe list, choice of the
// k_analyze_w instance, analysis, frame scan + group offsets, assembly) and the four schedules that order them on
// streams: serial / timing, FRA_GROUPS frame groups, one host band, and the cross-execute pipeline.  No kernels
// here (fra_kernels.hip, fra_analyze.hip launch them).
#include <algorithm>

#include "fra_plan.h"

namespace fra {
hipError_t launch_minmax(int src, const JobArgs& a, int nstreams, int max_segs, int vec_bytes, int rows, int max_rows,
                         hipStream_t s, int max_blocks);
hipError_t launch_norm_finalize(const JobArgs& a, int nstreams, hipStream_t s);
hipError_t launch_norm_lut(int src, const JobArgs& a, int nstreams, hipStream_t s);
hipError_t launch_analyze(int src, bool b32, bool ms, const JobArgs& a, hipStream_t s, bool wave, const int32_t* part,
                          int npart, int max_part_blocks, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join);
hipError_t launch_analyze_part(int src, bool b32, const JobArgs& a, const int32_t* part, int npart, int max_part_blocks,
                               hipStream_t s);
hipError_t launch_frame_scan(const JobArgs& a, unsigned long long* gbase, int grp, int last, int add_base,
                             unsigned long long* host_mirror, unsigned long long* look2, int look_stride,
                             unsigned long long* ctl, hipStream_t s);
hipError_t launch_assemble(const JobArgs& a, hipStream_t s);
hipError_t launch_group_offsets(unsigned long long* frame_off, const unsigned long long* frame_bytes,
                                unsigned long long* gbase, int grp, int f0, int n, int last, int nframes,
                                hipStream_t s, unsigned long long* host_mirror = nullptr);

// k_analyze_w (one subframe per wave, fra_analyze_w.hip) takes the full frames of 16-bit plans normalised
// through the per-tile table with 8-byte sample vectors at levels 3-6 (the partial frames' subframes go to
// k_analyze as a list); FRA_ANALYZE_WG=1 keeps every frame on the workgroup kernel (tests compare both)
bool wave_path(const fra_plan* p, const ExecEnv& env) {
  if (env.analyze_wg || !p->wave_ok || !p->args.vec8 || !p->args.off32 || p->job.blocksize != kMaxBlock) return false;
  // (32-bps plans stay on k_analyze: a one-subframe-per-wave 32-bps kernel, r05's k_analyze_w32, was measured
  // slower -- C5 quarter 28.5 against 22.8 ms of analysis, profiles/r05_ab_w32_c5q.txt -- and removed in r06)
  if (p->b32) return false;
  return p->args.lut && p->job.level >= 3 && p->job.level <= 6;  // k_analyze_w
}

// ------------------------------------------------------------------------------------------------ stages
// One frame group of an execute: group gi of ng, its frames as kernel arguments, and its analysis path
struct GroupJob {
  Group gr;
  int gi, ng;
  JobArgs ga;
  // wave path: k_analyze_w for the full frames, k_analyze for the group's partial subframes `part`
  bool wave = false;
  const int32_t* part = nullptr;
  int npart = 0;
  int nf() const { return gr.f1 - gr.f0; }
};

// norm stage of the group's windows on stream s: minmax, finalize, table
static int stage_norm(fra_plan* p, const Group& gr, hipStream_t s) {
  const JobArgs& a = p->args;
  const int nst = gr.w1 - gr.w0;
  // the minmax family indexes streams by blockIdx.y: launched per chunk of <= kMaxGridY windows, with the
  // stream/norm/LUT pointers offset to the chunk (grid Y is limited to 65535 on the device)
  constexpr int kMaxGridY = 65535;
  for (int c0 = 0; p->job.norm != 0 && p->max_segs > 0 && c0 < nst; c0 += kMaxGridY) {
    const int nc = std::min(kMaxGridY, nst - c0);
    JobArgs ma = a;
    ma.streams += gr.w0 + c0;
    ma.norm += gr.w0 + c0;
    if (ma.lut) ma.lut += (int64_t)(gr.w0 + c0) * a.lut_stride;
    const int vec = minmax_vec(p);  // pointer alignment
    // the full grid (max_blocks 0), one workgroup per row block, in pipelined executes as in serial ones --
    // measured against one workgroup per CU striding over the blocks: C4 step 1.666 -> 1.626 ms, 8-way share
    // 0.292 -> 0.274 ms, 4-way 0.505 -> 0.488 ms, C5 neutral, C3 1.089 -> 1.101
    // (profiles/r04_ab_assemble_fpw_minmax_grid.txt, r04_ab_minmax_grid_shards.txt)
    HIPCHK(launch_minmax(p->src, ma, nc, p->max_segs, vec, p->mm_rows, p->mm_max_rows, s, 0));
    HIPCHK(launch_norm_finalize(ma, nc, s));
    HIPCHK(launch_norm_lut(p->src, ma, nc, s));
  }
  return FRA_OK;
}

// the group's kernel arguments, its analysis path and its share of the partial-subframe list
static int group_job(fra_plan* p, const Group& gr, int gi, int ng, const ExecEnv& env, GroupJob& job) {
  job.gr = gr;
  job.gi = gi;
  job.ng = ng;
  job.ga = p->args;
  job.ga.frame_base = gr.f0;
  job.ga.frame_count = job.nf();
  job.wave = wave_path(p, env);
  if (env.require_wave && !job.wave && job.nf() > 0)
    return set_err(FRA_E_STATE, "FRA_REQUIRE_WAVE: the plan does not take k_analyze_w");
  const auto plo = std::lower_bound(p->part.begin(), p->part.end(), gr.f0 * 8);
  const auto phi = std::lower_bound(p->part.begin(), p->part.end(), gr.f1 * 8);
  job.npart = job.wave ? (int)(phi - plo) : 0;
  job.part = job.wave ? p->d_part + (plo - p->part.begin()) : nullptr;
  return FRA_OK;
}

// the k_analyze_w instance of this launch, from the counter snapshots that have arrived, and (count: the group is
// the whole plan) the ring entry it counts into
static void pick_instance(fra_plan* p, GroupJob& job, const ExecEnv& env, bool count) {
  p->cnt_cur = -1;  // (count_out copies the count out after everything the execute timed or waits on)
  if (!job.wave) return;
  // the snapshots that have arrived (newest wins): 17 bits when more than 1/32 of its waves needed bit 16 -- a wave
  // that does on the 16-bit instance re-derives its residuals from the samples (the sample path)
  for (int j = 0; j < fra_plan::kCnt; j++) {
    CntSlot& c = p->cnt[j];
    if (!c.pending || hipEventQuery(c.ev) != hipSuccess) continue;
    c.pending = false;
    const uint32_t n17 = p->h_cnt17[j] - c.base;
    c.base = p->h_cnt17[j];
    if (c.seq >= p->cnt_newest) {
      p->cnt_newest = c.seq;
      p->k17 = n17 > c.sub / 32 ? 1 : 0;
    }
  }
  job.ga.k17 = env.keep17 >= 0 ? env.keep17 : p->k17;  // (tests / A/B: FRA_KEEP17 forces the instance)
  const int j = (int)(p->cnt_next % fra_plan::kCnt);
  if (p->d_cnt17 && !p->cnt[j].pending && job.nf() > 0 && count) {
    p->cnt_cur = j;
    job.ga.cnt17 = p->d_cnt17 + j;
  }
}

// the analysis on stream s; a partial list still in the job runs beside k_analyze_w on the side stream
static int stage_analyze(fra_plan* p, const GroupJob& job, hipStream_t s) {
  HIPCHK(launch_analyze(p->src, p->b32, p->cmax == 4 && p->job.channels == 2, job.ga, s, job.wave, job.part, job.npart,
                        8 * p->ncu, p->pside, p->ev_pfork, p->ev_pjoin));
  if (p->cnt_cur >= 0) p->cnt[p->cnt_cur].sub = (uint32_t)job.nf() * (uint32_t)p->cmax;
  return FRA_OK;
}

// frame sizes and offsets within the group: one k_frame_scan on scan slot `slot`; add_base: the group's base is
// already ordered (first / only group, host bands on one stream), so it writes the final offsets itself
static int stage_scan(fra_plan* p, const GroupJob& job, int slot, bool add_base, unsigned long long* host_mirror,
                      hipStream_t s) {
  if (job.nf() > 0)
    HIPCHK(launch_frame_scan(job.ga, p->d_gbase, job.gi, job.gi == job.ng - 1, add_base ? 1 : 0, host_mirror,
                             p->d_look + (size_t)slot * 2 * p->look_stride, p->look_stride, p->d_ticket + slot, s));
  return FRA_OK;
}
// ... else k_group_offsets adds the base once the previous group has published it (and passes the base on for a
// group without frames)
static int stage_group_offsets(fra_plan* p, const GroupJob& job, unsigned long long* host_mirror, hipStream_t s) {
  HIPCHK(launch_group_offsets(job.ga.frame_off, job.ga.frame_bytes, p->d_gbase, job.gi, job.gr.f0, job.nf(),
                              job.gi == job.ng - 1, p->args.nframes_total, s, host_mirror));
  return FRA_OK;
}

// after an execute: copy its k_analyze_w count (fra_plan::d_cnt17 entry) to page-locked memory on the analysis
// stream s, behind everything the execute's frame scan, assembly and timing events wait for
static int count_out(fra_plan* p, hipStream_t s) {
  const int cj = p->cnt_cur;
  if (cj < 0) return FRA_OK;
  p->cnt_cur = -1;
  HIPCHK(hipMemcpyAsync(p->h_cnt17 + cj, p->d_cnt17 + cj, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(p->cnt[cj].ev, s));
  p->cnt[cj].pending = true;
  p->cnt[cj].seq = p->cnt_next++;
  return FRA_OK;
}

// ------------------------------------------------------------------------------------------------ schedules
// serial: the whole plan as one group on the plan's stream; in timing mode events bracket each kernel phase
static int run_serial(fra_plan* p, const ExecEnv& env) {
  const hipStream_t s = p->ctx->stream;
  GroupJob job;
  if (p->timing) HIPCHK(hipEventRecord(p->ev[0], s));
  if (int rc = stage_norm(p, p->all, s)) return rc;
  if (int rc = group_job(p, p->all, 0, 1, env, job)) return rc;
  if (p->timing) HIPCHK(hipEventRecord(p->ev[1], s));
  pick_instance(p, job, env, true);
  if (int rc = stage_analyze(p, job, s)) return rc;
  if (p->timing) HIPCHK(hipEventRecord(p->ev[2], s));
  if (int rc = stage_scan(p, job, 0, true, nullptr, s)) return rc;
  if (job.nf() == 0)
    if (int rc = stage_group_offsets(p, job, nullptr, s)) return rc;
  if (p->timing) HIPCHK(hipEventRecord(p->ev[3], s));
  HIPCHK(launch_assemble(job.ga, s));
  if (p->timing) {
    HIPCHK(hipEventRecord(p->ev[4], s));
    p->pending_times = true;
  }
  return count_out(p, s);
}

// FRA_GROUPS: group g on its own stream (group 0 on the plan's), each with its own scan slot; a group's offsets
// follow the previous group's (event ordered), so one group's minmax / assembly overlaps another's analysis
static int run_groups(fra_plan* p, const ExecEnv& env) {
  const hipStream_t s = p->ctx->stream;
  const int ng = (int)p->groups.size();
  HIPCHK(hipEventRecord(p->gev[0], s));
  for (int g = 1; g < ng; g++) HIPCHK(hipStreamWaitEvent(p->aux[g - 1], p->gev[0], 0));
  for (int g = 0; g < ng; g++) {
    const hipStream_t st = g == 0 ? s : p->aux[g - 1];
    GroupJob job;
    if (int rc = stage_norm(p, p->groups[g], st)) return rc;
    if (int rc = group_job(p, p->groups[g], g, ng, env, job)) return rc;
    pick_instance(p, job, env, false);
    if (int rc = stage_analyze(p, job, st)) return rc;
    // the first group's scan writes final offsets; a later one's are relative until the previous group has
    // published its end
    if (int rc = stage_scan(p, job, g, g == 0, nullptr, st)) return rc;
    if (g) HIPCHK(hipStreamWaitEvent(st, p->gev[1 + 2 * (g - 1)], 0));
    if (g || job.nf() == 0)
      if (int rc = stage_group_offsets(p, job, nullptr, st)) return rc;
    HIPCHK(hipEventRecord(p->gev[1 + 2 * g], st));  // offsets published
    HIPCHK(launch_assemble(job.ga, st));
    if (g) HIPCHK(hipEventRecord(p->gev[2 + 2 * g], st));
  }
  for (int g = 1; g < ng; g++) HIPCHK(hipStreamWaitEvent(s, p->gev[2 + 2 * g], 0));
  return FRA_OK;
}

// host band b of fra_plan_encode_host, on the plan's stream (every band on scan slot 0).  The band's end offset
// reaches h_gbase by a kernel store (k_frame_scan / k_group_offsets), not by a copy-engine command that would
// queue behind the H2D copies
int run_host_band(fra_plan* p, int b, const ExecEnv& env) {
  const hipStream_t s = p->ctx->stream;
  const Group& gr = p->hbands[b].g;
  const int nb = (int)p->hbands.size();
  GroupJob job;
  if (int rc = stage_norm(p, gr, s)) return rc;
  if (int rc = group_job(p, gr, b, nb, env, job)) return rc;
  pick_instance(p, job, env, nb == 1);
  if (int rc = stage_analyze(p, job, s)) return rc;
  if (int rc = stage_scan(p, job, 0, true, p->d_gbase_mirror, s)) return rc;
  if (job.nf() == 0)
    if (int rc = stage_group_offsets(p, job, p->d_gbase_mirror, s)) return rc;
  HIPCHK(launch_assemble(job.ga, s));
  return FRA_OK;
}

// cross-execute pipelining: execute k's norm stage (and partial subframes) on the norm stream, its analysis on an
// analysis stream, its frame scan and assembly on the pack stream, each into / out of slot set k % nslot and
// the next norm set, so that this execute's analysis overlaps the previous execute's k_assemble
static int run_pipelined(fra_plan* p, const ExecEnv& env) {
  const hipStream_t s = p->ctx->stream;
  const int b = (p->cur + 1) % p->nslot;
  SlotSet& ss = p->slot[b];
  const hipStream_t as = p->astream[p->exec_n++ & 1u];  // this execute's analysis stream
  if (ss.pack_pending) HIPCHK(hipStreamWaitEvent(as, ss.ev_pack, 0));  // execute k-nslot is done with set b
  // one background kernel at a time beside k_analyze: this norm stage after k_assemble of execute k-2
  // (which runs under the analysis of execute k-1) -- 32-bps plans (C5 quarter +0.4 % without); 16-bit plans: the
  // norm stage runs beside that assembly and the analysis of execute k-1 (C4 step 1.526 -> 1.497-1.504 ms, its
  // 8-way shares -4 %, C3 -0.8 %, profiles/r05_ab_bg_serial.txt) and only the partial-subframe list launch
  // after the norm stage waits for that assembly (it rewrites the slots; the norm stage writes only this set's
  // NormDev / table, which execute k-2's analysis and partial list -- both earlier on this stream or waited
  // for below -- read)
  const bool bg_serial = p->b32;
  if (ss.pack_pending && bg_serial) HIPCHK(hipStreamWaitEvent(p->nstream, ss.ev_pack, 0));
  const int nb = (p->curn + 1) % fra_plan::kNormSets;
  NormSet& ns = p->nset[nb];
  use_buffers(p, b, nb);
  // norm stage of this execute on the norm stream: after the last analysis that read norm set nb (execute
  // k-3), and after a host raster copy enqueued on the plan's stream since the last
  // execute.  (That analysis's partial-subframe list ran earlier on the norm stream itself.)
  if (ns.free_pending) HIPCHK(hipStreamWaitEvent(p->nstream, ns.ev_free, 0));
  if (p->resync) {  // first pipelined execute after serial ones: after everything on the plan's stream
    HIPCHK(hipEventRecord(p->ev_raster, s));
    for (auto& st : p->astream) HIPCHK(hipStreamWaitEvent(st, p->ev_raster, 0));
    p->raster_dirty = true;
    p->resync = false;
  }
  if (p->raster_dirty) {
    HIPCHK(hipStreamWaitEvent(p->nstream, p->ev_raster, 0));
    p->raster_dirty = false;
  }
  GroupJob job;
  if (int rc = stage_norm(p, p->groups[0], p->nstream)) return rc;
  if (int rc = group_job(p, p->groups[0], 0, 1, env, job)) return rc;
  HIPCHK(hipEventRecord(ss.ev_norm, p->nstream));
  HIPCHK(hipStreamWaitEvent(as, ss.ev_norm, 0));
  // the partial subframes on the norm stream right after the norm stage (a whole execute before the frame scan
  // that waits for them) instead of beside k_analyze_w
  const bool parts = job.npart > 0;
  if (parts) {
    // (these slots: execute k-2's assembly read them -- the norm stream waited for it above, or does here)
    if (!bg_serial && ss.pack_pending) HIPCHK(hipStreamWaitEvent(p->nstream, ss.ev_pack, 0));
    HIPCHK(launch_analyze_part(p->src, p->b32, job.ga, job.part, job.npart, 8 * p->ncu, p->nstream));
    HIPCHK(hipEventRecord(ss.ev_part, p->nstream));
    job.part = nullptr;
    job.npart = 0;
  }
  pick_instance(p, job, env, true);
  if (int rc = stage_analyze(p, job, as)) return rc;
  HIPCHK(hipEventRecord(ss.ev_ana, as));
  // the frame-size chain (k_frame_scan) only feeds this execute's assembly, so it goes onto the pack stream
  // with it and the analysis stream proceeds straight to the next execute's analysis
  HIPCHK(hipEventRecord(ss.ev_scan, as));
  HIPCHK(hipStreamWaitEvent(p->pack, ss.ev_scan, 0));
  if (parts) HIPCHK(hipStreamWaitEvent(p->pack, ss.ev_part, 0));  // the partial subframes (norm stream) are done
  if (int rc = stage_scan(p, job, 0, true, nullptr, p->pack)) return rc;
  if (job.nf() == 0)
    if (int rc = stage_group_offsets(p, job, nullptr, p->pack)) return rc;
  HIPCHK(launch_assemble(job.ga, p->pack));
  if (int rc = count_out(p, as)) return rc;
  ss.ana_pending = true;
  HIPCHK(hipEventRecord(ns.ev_free, as));  // (the analysis was the last work on `as`): the norm set is free for
  ns.free_pending = true;                  // the norm stage of the execute kNormSets later
  HIPCHK(hipEventRecord(ss.ev_pack, p->pack));
  ss.pack_pending = true;
  return FRA_OK;
}

}  // namespace fra

using namespace fra;

extern "C" int fra_plan_execute(fra_plan* p) {
  if (!p) return set_err(FRA_E_INVALID, "null plan");
  if (!p->d_raster && !p->streams.empty()) return set_err(FRA_E_STATE, "plan has no raster");
  (void)hipSetDevice(p->ctx->device);
  if (p->timing) collect_times(p);
  set_vec8(p);
  const ExecEnv env = env_exec();
  int rc;
  if (p->pipe && !p->timing) {
    rc = run_pipelined(p, env);
  } else {
    if ((rc = drain_pipeline(p))) return rc;
    rc = (p->timing || p->groups.size() == 1) ? run_serial(p, env) : run_groups(p, env);
  }
  if (rc == FRA_OK) p->executed = true;
  return rc;
}
