// fra_plan.h -- fra_ctx and fra_plan (host only), the environment switches, and what the translation units of the
// host side share: fra_plan.hip (create / build / destroy / set_raster / queries), fra_exec.hip (stages and
// schedules of an execute), fra_hostpath.hip (fra_plan_encode_host and kin), fra_api.hip (the rest of the C ABI).
#pragma once
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "fra_host.h"
#include "fra_layout.h"

#define set_err fra_internal_set_error

struct fra_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  HipArena res;  // owns the stream
  // encode_host's D2H workers for pageable outputs: page-locked staging (one 64 MiB piece per worker) and one
  // stream per worker, kept across plans (the file path builds a plan per call); one encode at a time holds them
  std::mutex stage_mu;
  HipArena stage_res;  // owns the staging and its streams
  uint8_t* stage = nullptr;
  std::vector<hipStream_t> stage_st;
};

namespace fra {

// ---- environment switches, each read here only.  When a plan is made:
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline int env_groups() { return env_int("FRA_GROUPS", 1); }  // frame groups of plans of >= 4096 frames (1..8)
inline bool env_pipe() { return env_int("FRA_PIPE", 1) != 0; }  // cross-execute pipelining
inline int env_pipe_min_frames() {  // ... of plans of at least this many frames (read once per process)
  static const int v = env_int("FRA_PIPE_MIN_FRAMES", 1024);
  return v;
}
// when a context's D2H staging is made (its first encode into a pageable output): worker threads, 1..16
inline int env_d2h_threads() { return std::min(std::max(env_int("FRA_D2H_THREADS", 4), 1), 16); }
// at every execute (tests compare the paths these select):
struct ExecEnv {
  bool analyze_wg;    // FRA_ANALYZE_WG=1 keeps every frame on the workgroup kernel
  bool require_wave;  // FRA_REQUIRE_WAVE=1 makes a plan that would not take the wave path fail instead
  int keep17;         // FRA_KEEP17=0/1 forces the k_analyze_w instance (-1: the plan's own choice)
};
inline ExecEnv env_exec() {
  const char* ek = getenv("FRA_KEEP17");
  return {env_int("FRA_ANALYZE_WG", 0) == 1, env_int("FRA_REQUIRE_WAVE", 0) == 1,
          (ek && ek[0] == '0') ? 0 : (ek && ek[0] == '1') ? 1 : -1};
}

// one slot set: descriptors, encoded-subframe slots, frame meta, sizes and offsets of an execute, with the events
// a pipelined execute into it records
struct SlotSet {
  SfDesc* sf = nullptr;
  uint32_t* tmp = nullptr;
  uint32_t* fmeta = nullptr;
  unsigned long long* fbytes = nullptr;
  unsigned long long* foff = nullptr;
  hipEvent_t ev_norm = nullptr;  // its norm stage is done (norm stream)
  hipEvent_t ev_part = nullptr;  // its partial subframes are done (norm stream)
  hipEvent_t ev_ana = nullptr;   // its analysis is done
  hipEvent_t ev_scan = nullptr;  // hands the execute over from the analysis stream to the pack stream
  hipEvent_t ev_pack = nullptr;  // its assembly is done (pack stream)
  bool ana_pending = false, pack_pending = false;
};
// one norm set: NormDev + table of every stream
struct NormSet {
  NormDev* norm = nullptr;
  int32_t* lut = nullptr;
  hipEvent_t ev_free = nullptr;  // the last analysis (+ partial list) reading the set is done
  bool free_pending = false;
};
// one entry of the k_analyze_w instance counter ring: the counter never resets, an execute's count is its snapshot
// (page-locked h_cnt17[j], valid once `ev` has completed) minus the entry's previous one
struct CntSlot {
  uint32_t base = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;
  uint64_t seq = 0;
  uint32_t sub = 0;  // subframes counted
};

}  // namespace fra

// A plan owns every device buffer a job needs (raster copy if host-resident, stream/frame tables, window tables,
// subframe descriptors, frame sizes/offsets, output, scan workspace), so that fra_plan_execute() only enqueues
// kernels and events: no allocation, no host sync.  Everything is made through `res` and released with it; the
// pointers and handles below are views.
struct fra_plan : fra::PlanLayout {
  fra_ctx* ctx = nullptr;
  fra_job job{};
  std::vector<fra_window> windows;
  std::vector<int32_t> franges;  // fra_plan_create_ranged: [2 w] first frame, [2 w + 1] count (-1: to the end)
  int ncu = 256;  // compute units of the device (background grids)
  HipArena res;
  void* d_raster_owned = nullptr;
  const void* d_raster = nullptr;
  fra::StreamDev* d_streams = nullptr;
  int32_t* d_part = nullptr;    // PlanLayout::part
  hipStream_t pside = nullptr;  // the partial subframes' stream (beside k_analyze_w) and its fork / join
  hipEvent_t ev_pfork = nullptr, ev_pjoin = nullptr;
  // k_analyze_w instance (r05): kept residuals up to 17 bits or 16 (JobArgs::k17), picked per execute from how many
  // waves of an earlier execute needed bit 16.  Pipelined plans count into d_cnt17[j] (ring entry j) and copy the
  // counter into page-locked h_cnt17[j] after the analysis; the host reads a snapshot once its event has completed
  // (no sync)
  static constexpr int kCnt = 4;
  uint32_t* d_cnt17 = nullptr;
  uint32_t* h_cnt17 = nullptr;
  fra::CntSlot cnt[kCnt];
  uint64_t cnt_next = 0, cnt_newest = 0;
  int cnt_cur = -1;  // the ring entry the last analysis counted into (-1: none)
  int k17 = 1;  // start with 17 bits: never slower than the sample path by more than its VGPR cost
  uint8_t* d_out = nullptr;
  // k_frame_scan look-back words and tickets per scan slot (frame group g: slot g; host bands and the
  // timing pass: slot 0) and, on the host, each slot's ticket base and launch tag (launches on one slot
  // are stream-ordered)
  unsigned long long* d_look = nullptr;
  uint32_t* d_err = nullptr;  // JobArgs::err (plan_sync_all)
  unsigned long long* d_ticket = nullptr;  // per scan slot: [63:32] epoch, [31:0] next ticket (k_frame_scan)
  int look_stride = 0;
  // kernel arguments: the plan's tables, and the slot / norm set chosen by use_buffers
  fra::JobArgs args{};
  // frame groups: group g > 0 runs on aux[g - 1] (group 0 on the context stream) so one group's minmax/assemble
  // overlaps another's k_analyze
  std::vector<hipStream_t> aux;
  std::vector<hipEvent_t> gev;          // [0] start, then per group: offsets-published, done
  unsigned long long* d_gbase = nullptr;  // [max(groups, host bands) + 1] byte offset of each group's first frame
  // host pipeline (fra_plan_encode_host), made at its first call
  hipStream_t h2d = nullptr, d2h = nullptr;
  std::vector<hipEvent_t> hev;          // per band: rows copied, frames assembled (+ end offset mirrored)
  hipEvent_t hev_start = nullptr;
  unsigned long long* h_gbase = nullptr;  // page-locked mirror of d_gbase[1..bands]
  unsigned long long* d_gbase_mirror = nullptr;  // its device address
  // cross-execute pipelining (FRA_PIPE, default on when a second buffer set fits in a third of the free
  // device memory, single frame group): execute k analyses into slot set k % nslot on an analysis stream
  // while the frame-size chain + assembly of earlier executes (reading the other sets) run on the pack stream.
  // A plan that is not pipelined has one slot set and one norm set.
  bool pipe = false;
  // slot sets: nslot = 3 (execute k's analysis waits for the assembly of execute k-3), or 2 when memory is short;
  // the analysis streams alternate by execute
  static constexpr int kSlotSets = 3;
  int nslot = 1;
  int cur = 0;  // slot set of the last execute
  unsigned exec_n = 0;
  fra::SlotSet slot[kSlotSets];
  hipStream_t pack = nullptr;
  // execute k's analysis runs on astream[k % 2] (highest priority): execute k+1's is queued on the other stream
  // than execute k's, so its first waves fill the CUs that execute k's tail leaves idle instead of waiting for
  // that kernel to end
  hipStream_t astream[2] = {};
  // ... and the normalisation stage (k_minmax -> k_norm_finalize -> k_norm_lut) of execute k+1 runs on
  // the norm stream under k_analyze of execute k.  k_analyze_w (4 waves of 8 KiB and 97 VGPRs per SIMD) leaves
  // 32 KiB of LDS and 96 VGPRs per SIMD beside it for the norm stage and the assembly; the 32-bps k_analyze (5
  // workgroups of 31.6 KiB) leaves none, so there they run in the gaps between analysis waves
  // norm sets (NormDev + table) cycle over kNormSets executes, the slot sets above over nslot (r05): execute k+1's norm
  // stage waits for execute k-2's analysis, not k-1's, so the norm stream runs up to a whole execute ahead and
  // execute k+1's table is ready before execute k's analysis drains (its waves fill that grid's last, partly empty
  // generation instead of waiting behind a k_minmax_vec that runs ~1.1 ms beside the analysis)
  static constexpr int kNormSets = 3;
  fra::NormSet nset[kNormSets];
  int curn = 0;  // norm set of the last execute
  hipStream_t nstream = nullptr;
  hipEvent_t ev_raster = nullptr;
  bool raster_dirty = false;  // a host raster copy on the plan's stream the norm stream must wait for
  bool resync = false;        // serial work was queued on the plan's stream since the last pipelined execute
  // timing
  bool timing = false;
  hipEvent_t ev[5] = {};
  float ms[4] = {0, 0, 0, 0};
  int nexec = 0;
  bool pending_times = false;
  bool executed = false;
};

namespace fra {
// fra_plan.hip
void use_buffers(fra_plan* p, int b, int nb);  // point the kernel arguments at slot set b and norm set nb
int drain_pipeline(fra_plan* p);
int check_dev_err(fra_plan* p);
int plan_sync_all(fra_plan* p);
void collect_times(fra_plan* p);  // timing mode: add the last execute's phase times once it has finished
int plan_own_raster(fra_plan* p);  // the plan's own device raster (host-resident jobs), made on first use
// 8-byte sample vectors as an execute decides them: the device raster's alignment (hipMalloc's for host rasters)
inline void set_vec8(fra_plan* p) { p->args.vec8 = (p->ld_vec8 && (uintptr_t)p->d_raster % 8 == 0) ? 1 : 0; }
// bytes per load of the min/max pass as an execute decides them: the layout's vector width when the device raster
// is aligned to it, else 0 (scalar k_minmax; a 16-byte layout does not fall back to 8-byte vectors)
inline int minmax_vec(const fra_plan* p) { return (p->mm_vec && (uintptr_t)p->d_raster % p->mm_vec == 0) ? p->mm_vec : 0; }
// fra_exec.hip
bool wave_path(const fra_plan* p, const ExecEnv& env);
int run_host_band(fra_plan* p, int b, const ExecEnv& env);
// keeps the calling thread's error message across clean-up calls that may set their own
struct KeepError {
  std::string msg = fra_last_error();
  ~KeepError() { set_err(0, "%s", msg.c_str()); }
};
}  // namespace fra
