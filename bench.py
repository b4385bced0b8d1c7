#!/usr/bin/env python3
"""bench.py -- FLAC raster encode throughput on MI355X (driver contract: one JSON line on rank 0).

Workload (default ``--config c4``, the north-star configuration of BASELINE.json):
  C4  Sentinel-2 L1C-like 10980 x 10980 x 4 uint16 raster, ``--streaming --tile-size 1024``,
      ``-c 5``: 121 tiles -> 121 independent FLAC streams (100 x 1024^2, 20 x 1024x740, 1 x 740^2).
A *step* = one pass of the encode hot path over the whole scene: device-resident raster in HBM ->
per-tile nanmin/nanmax -> normalize_to_audio -> FLAC analysis -> bit-packed frames of every tile
in HBM (the bytes the reference's pyflac/libFLAC calls produce per tile, cli.py:553-622).

Multi-GPU (one process per GPU): under torch.distributed.run, or ``--gpus N`` alone, which starts the N rank
processes itself before touching the GPU.  STRONG scaling by default -- BASELINE's C4/C5 are ONE scene split
over the GPUs into (tile, frame range) items of equal cost (``--split frames``: frames, plus a fixed charge for
partial frames), no
collective on the data path; ``value`` = scene pixels / max-over-ranks time; per-rank times and the imbalance
are reported.  ``--scaling weak`` instead gives every rank its own scene (seed + rank).

A plain run (``--gpus 1 --steps N --warmup W``) does what the headline needs and nothing else: set-up (scene, plan,
the settle executes), W warmup steps, the N timed steps, ``--dump-outputs DIR`` if asked (the last timed step's
stream table and a fixed sample of its frame bytes as .npy, see ``dump_outputs``), and the result line (``value``,
``ms_per_step``, ``config``, ``per_rank``, ``analysis_instance``).

Every other leg runs only with ``--full`` (rank 0; each still has its ``--no-*`` switch), and adds to the line:
* ``analysis_instance.ms_per_step_forced_17bit``: the same steps forced onto the 17-bit k_analyze_w instance;
* ``roofline`` of the dominant kernel: HIP events on the plan's stream; algorithmic bytes = input raster
  bytes + emitted frame bytes of the units one launch processes; ``traffic`` / ``valu_issue_frac`` from
  in-run rocprofv3 PMC passes of this same build (``--no-pmc`` falls back to the committed profile
  file of the same kernel sources, else null); ``bound`` = the larger of the HBM and VALU-issue fractions;
* ``cpu_baseline``: the CPU oracle (oracle/, C port of the path, 1 thread) on a bounded sample of the
  same scene, bytes checked against the GPU's; ``cpu_baseline_mp``: the same port fanned over the
  host's core share (BASELINE.md B-mp);
* ``e2e``: the PCIe-inclusive path (host raster -> pipelined H2D / kernels / D2H -> host frames);
* ``size_ratio_vs_libflac_c2``, ``pyflac_shim_c2``: the C2 raster's size against libFLAC's and the shim's latency;
* ``kernel_stats``: a rocprofv3 kernel trace of a child run of the same steps.
A ``--shard R/N`` projection line is made of the per-kernel times, so it runs that leg without ``--full``.
"""

from __future__ import annotations

import argparse
import csv
import hashlib
import json
import os
import platform
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "flac-raster_amd"))

CONFIGS = {
    "c3": dict(kind=3, bands=1, H=16384, W=16384, dtype=np.int16, tile=512, level=5, norm=16,
               workload="C3 synthetic DEM 16384x16384x1 int16, --streaming --tile-size 512, -c 5"),
    "c4": dict(kind=4, bands=4, H=10980, W=10980, dtype=np.uint16, tile=1024, level=5, norm=16,
               workload="C4 Sentinel-2 L1C-like 10980x10980x4 uint16, --streaming --tile-size 1024, -c 5"),
    "c5": dict(kind=5, bands=8, H=32768, W=32768, dtype=np.float32, tile=512, level=8, norm=24,
               workload="C5 multispectral 32768x32768x8 float32 (normalize->int32, 32-bps), --streaming "
                        "--tile-size 512, -c 8"),
    # profiling / A/B subset of C5 (a quarter of the scene, the same tiles, level and per-subframe work); never the
    # bench line's workload
    "c5q": dict(kind=5, bands=8, H=16384, W=16384, dtype=np.float32, tile=512, level=8, norm=24,
                workload="C5 quarter (16384x16384x8 float32, tiles 512, -c 8): profiling subset"),
}
SEED = 20260227
HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md chip-level parameters)
SIMDS = 256 * 4          # 256 CUs x 4 SIMD-32
VALU_CYC = 2             # SIMD cycles per wave64 VALU instruction on a SIMD-32 (MI355X_MICROARCH.md)
XCDS = 8                 # GRBM_GUI_ACTIVE sums the busy cycles of the 8 XCDs
SETTLE = 16              # untimed executes of plan set-up, before the --warmup steps (reported as settle_executes)


def tiles(H, W, t):
    return [(r, c, min(t, H - r), min(t, W - c)) for r in range(0, H, t) for c in range(0, W, t)]


def lpt_shard(wins, nranks):
    """Longest-processing-time static assignment of tiles to ranks (deterministic; == dist.shard)."""
    order = sorted(range(len(wins)), key=lambda i: (-(wins[i][2] * wins[i][3]), i))
    load = [0] * nranks
    owner = [0] * len(wins)
    for i in order:
        r = min(range(nranks), key=lambda k: (load[k], k))
        owner[i] = r
        load[r] += wins[i][2] * wins[i][3]
    return owner


def sources_sha():
    """Hash of the kernel sources: a committed profile file is only valid for the build it measured."""
    h = hashlib.sha256()
    for p in sorted((ROOT / "flac-raster_amd" / "csrc").glob("*")):
        if p.suffix in (".hip", ".h", ".cpp"):
            h.update(p.name.encode())
            h.update(p.read_bytes())
    return h.hexdigest()[:16]


# ------------------------------------------------------------------------------------- --dump-outputs
DUMP_SAMPLE_BYTES = 8 << 20  # frame bytes kept in frames_sample.npy (as float32: 32 MiB of the 64 MB allowed)


def dump_outputs(out_dir, ctx, plan, prefix=""):
    """What a caller of the timed path holds after the last timed execute -- the stream table of ``plan.result()``
    and the frame bytes in the plan's device output -- as float .npy files, so two builds can be compared:

    * ``streams.npy``  float64 (nstreams, 8): offset, frame_bytes, data_min, data_max, sample_rate, bps, channels,
      nframes of every stream (the integers are exact in float64);
    * ``frames_sample.npy``  float32 (nstreams, chunk), chunk = DUMP_SAMPLE_BYTES // nstreams: ``chunk`` consecutive
      frame bytes of EVERY stream, starting at a position inside the stream drawn by a generator seeded with SEED
      (the whole stream, zero padded, when it is shorter than ``chunk``) -- the frames themselves are 0.5-22 GB;
    * ``frames_sample_start.npy``  float64 (nstreams,): that position, in bytes from the stream's first byte.
    """
    out_dir.mkdir(parents=True, exist_ok=True)
    infos, total = plan.result()
    dev_out, _ = plan.device_output()
    n = len(infos)
    table = np.array([[s.offset, s.frame_bytes, s.data_min, s.data_max, s.sample_rate, s.bps, s.channels, s.nframes]
                      for s in infos], dtype=np.float64).reshape(n, 8)
    chunk = max(1, DUMP_SAMPLE_BYTES // max(1, n))
    u = np.random.default_rng(SEED).random(n)
    start = np.zeros(n, np.float64)
    sample = np.zeros((n, chunk), np.float32)
    for i, s in enumerate(infos):
        size = int(s.frame_bytes)
        take = min(size, chunk)
        first = int(u[i] * (size - take + 1))
        if s.offset + first + take > total:
            raise RuntimeError(f"stream {i}: offset {s.offset} + {size} bytes exceeds the output's {total}")
        buf = np.empty(max(1, take), np.uint8)
        if take:
            ctx.d2h(buf[:take], dev_out + int(s.offset) + first)
        sample[i, :take] = buf[:take]
        start[i] = first
    np.save(out_dir / f"{prefix}streams.npy", table)
    np.save(out_dir / f"{prefix}frames_sample.npy", sample)
    np.save(out_dir / f"{prefix}frames_sample_start.npy", start)


# ------------------------------------------------------------------------------------- CPU baselines
def _oracle():
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle as O  # test / baseline infrastructure only (never on the product path)
    return O


def _encode_tile_cpu(O, cfg, tile):
    B = cfg["bands"]
    h, w = tile.shape[1], tile.shape[2]
    inter = tile.transpose(1, 2, 0).reshape(-1, B)
    audio, _, _ = O.normalize(inter, 16 if cfg["norm"] == 16 else 24)
    return O.encode(audio, O.sample_rate_for_pixels(h * w), level=cfg["level"], with_header=False)


def cpu_baseline(cfg, wins, gpu_tile_bytes, budget_s):
    """Time the CPU oracle (C port of the encode path, 1 thread) on the first tiles of the scene
    until ~budget_s of CPU work; verify its bytes equal the GPU's for those tiles."""
    O = _oracle()
    from flac_raster.synth import synth_window

    px = 0
    t_cpu = 0.0
    checked = 0
    mismatches = 0
    for idx, (r0, c0, h, w) in enumerate(wins):
        tile = synth_window(cfg["kind"], SEED, cfg["bands"], cfg["H"], cfg["W"], r0, c0, h, w)
        t0 = time.perf_counter()
        frames = _encode_tile_cpu(O, cfg, tile)
        t_cpu += time.perf_counter() - t0
        px += h * w
        got = gpu_tile_bytes(idx)
        if got is not None:
            checked += 1
            if got != frames:
                mismatches += 1
        if t_cpu >= budget_s:
            break
    return dict(value=px / t_cpu / 1e6, seconds=t_cpu, pixels=px, tiles=idx + 1, checked=checked,
                mismatches=mismatches)


def _mp_worker(args):
    cfg_name, level, tile_ids, barrier = args
    cfg = dict(CONFIGS[cfg_name], level=level)
    O = _oracle()
    from flac_raster.synth import synth_window

    wins = tiles(cfg["H"], cfg["W"], cfg["tile"])
    data = [synth_window(cfg["kind"], SEED, cfg["bands"], cfg["H"], cfg["W"], *wins[i]) for i in tile_ids]
    barrier.wait()
    t0 = time.perf_counter()
    nbytes = 0
    for t in data:
        nbytes += len(_encode_tile_cpu(O, cfg, t))
    t1 = time.perf_counter()
    return t0, t1, sum(wins[i][2] * wins[i][3] for i in tile_ids), nbytes


def cpu_mp_child(cfg_name, procs, ntiles, level=None):
    """B-mp: the oracle on the first ``ntiles`` tiles fanned over ``procs`` processes (its own process
    tree, started by the bench as a child so no GPU state is forked); prints one JSON line."""
    import multiprocessing as mp

    cfg = CONFIGS[cfg_name]
    level = cfg["level"] if level is None else level
    wins = tiles(cfg["H"], cfg["W"], cfg["tile"])[:ntiles]
    order = sorted(range(len(wins)), key=lambda i: -(wins[i][2] * wins[i][3]))
    share = [[] for _ in range(procs)]
    load = [0] * procs
    for i in order:
        k = min(range(procs), key=lambda j: load[j])
        share[k].append(i)
        load[k] += wins[i][2] * wins[i][3]
    share = [s for s in share if s]
    ctx = mp.get_context("fork")
    mgr = ctx.Manager()
    barrier = mgr.Barrier(len(share))
    with ctx.Pool(len(share)) as pool:
        res = pool.map(_mp_worker, [(cfg_name, level, s, barrier) for s in share])
    t0 = min(r[0] for r in res)
    t1 = max(r[1] for r in res)
    px = sum(r[2] for r in res)
    print(json.dumps({"value": px / (t1 - t0) / 1e6, "seconds": t1 - t0, "pixels": px, "tiles": len(wins),
                      "procs": len(share)}), flush=True)


# ------------------------------------------------------------------------------------- in-run PMC
def _short(name):
    return name.replace("void ", "").split("(")[0].replace("fra::", "").split("<")[0]


def pmc_pass(args, counters, tag):
    """One rocprofv3 counter pass over a 1-step child run of this bench (same config, same build).
    Returns {kernel: {counter: [values per launch]}} or None."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    out = tempfile.mkdtemp(prefix=f"fra_pmc_{tag}_", dir="/tmp")
    cmd = [prof, "--pmc", *counters, "--output-format", "csv", "-d", out, "-o", "run", "--",
           sys.executable, str(ROOT / "bench.py"), "--config", args.config, "--steps", "1", "--warmup", "1",
           "--child"]
    if args.level is not None:
        cmd += ["--level", str(args.level)]
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       timeout=float(os.environ.get("FRA_PMC_TIMEOUT", "150")), check=True)
    except (subprocess.SubprocessError, OSError):
        shutil.rmtree(out, ignore_errors=True)
        return None
    f = next(Path(out).rglob("*counter_collection.csv"), None)
    acc = {}
    if f is not None:
        for r in csv.DictReader(open(f)):
            acc.setdefault(_short(r["Kernel_Name"]), {}).setdefault(r["Counter_Name"], []).append(
                float(r["Counter_Value"]))
    shutil.rmtree(out, ignore_errors=True)
    return acc or None


def _med(v):
    v = sorted(v or [0.0])
    return v[len(v) // 2]


def inrun_pmc(args, kernel):
    """HBM traffic (FETCH_SIZE x2 + WRITE_SIZE, MI355X_MICROARCH.md gfx950 correction; KiB), VALU
    instruction counts and the wave-cycle split of ``kernel``'s median launch, from separate passes.
    SQ_WAVE_CYCLES = SQ_WAIT_ANY (parked at s_waitcnt / s_barrier) + SQ_WAIT_INST_ANY (ready, not issued)
    + SQ_ACTIVE_INST_ANY (issuing), all in quad-cycles (MI355X_MICROARCH.md "rocprofv3 PMC slots")."""
    res = {"source": "in-run rocprofv3 --pmc passes of this build (bench.py --child, 1 step)"}
    fe = pmc_pass(args, ["FETCH_SIZE"], "fetch")
    wr = pmc_pass(args, ["WRITE_SIZE"], "write")
    va = pmc_pass(args, ["SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY",
                         "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU"], "valu")
    gr = pmc_pass(args, ["SQ_WAVES", "SQ_INSTS_LDS", "SQ_WAIT_INST_LDS", "SQ_LDS_BANK_CONFLICT",
                         "GRBM_GUI_ACTIVE"], "grbm")
    # the analysis phase is k_analyze_w (full frames, one subframe per wave) + k_analyze (partial frames)
    # on 16-bit LUT plans, k_analyze alone otherwise: traffic summed over the phase's kernels, the per-wave
    # counters of the larger one
    group = [kernel]
    if kernel == "k_analyze" and va and "k_analyze_w" in va:
        group = ["k_analyze_w", "k_analyze"]
        kernel = "k_analyze_w"
        res["kernels"] = group
    if fe and wr and all(k in fe and k in wr for k in group if k in fe):
        res["traffic"] = int(sum(2 * _med(fe[k]["FETCH_SIZE"]) * 1024 + _med(wr[k]["WRITE_SIZE"]) * 1024
                                 for k in group if k in fe and k in wr))
        res["traffic_by_kernel"] = {k: int(2 * _med(fe[k].get("FETCH_SIZE")) * 1024 +
                                           _med(wr.get(k, {}).get("WRITE_SIZE")) * 1024) for k in fe}
    if va and kernel in va:
        v = va[kernel]
        waves = _med(v.get("SQ_WAVES"))
        res["waves"] = int(waves)
        res["valu_insts"] = int(_med(v.get("SQ_INSTS_VALU")))
        res["valu_per_wave"] = round(res["valu_insts"] / waves, 1) if waves else None
        res["salu_per_wave"] = round(_med(v.get("SQ_INSTS_SALU")) / waves, 1) if waves else None
        wc = _med(v.get("SQ_WAVE_CYCLES"))
        if wc:
            st = {"wave_quad_cycles_per_wave": round(wc / waves, 1),
                  "parked_waitcnt_or_barrier": round(_med(v.get("SQ_WAIT_ANY")) / wc, 4),
                  "ready_not_issued": round(_med(v.get("SQ_WAIT_INST_ANY")) / wc, 4),
                  "issuing": round(_med(v.get("SQ_ACTIVE_INST_ANY")) / wc, 4),
                  "issuing_valu": round(_med(v.get("SQ_ACTIVE_INST_VALU")) / wc, 4)}
            st["dominant"] = max(("parked_waitcnt_or_barrier", "ready_not_issued", "issuing"), key=lambda k: st[k])
            res["stalls"] = st
    if gr and kernel in gr:
        g = gr[kernel]
        res["busy_cycles_per_xcd"] = int(_med(g.get("GRBM_GUI_ACTIVE")) / XCDS)
        waves = _med(g.get("SQ_WAVES"))
        if waves:
            res["lds_per_wave"] = round(_med(g.get("SQ_INSTS_LDS")) / waves, 1)
            res["lds_issue_stall_quad_cycles_per_wave"] = round(_med(g.get("SQ_WAIT_INST_LDS")) / waves, 1)
            res["lds_bank_conflict_cycles_per_wave"] = round(_med(g.get("SQ_LDS_BANK_CONFLICT")) / waves, 1)
    return res


def analysis_kernel(cfg, dt, wave, k17=True):
    """(label, mangled-name prefix) of the analysis kernel a plan of this config launches: k_analyze_w when the plan
    reports FRA_PLAN_WAVE (``wave``: full frames one subframe per wave, the partial-frame list on k_analyze beside
    it) for a <= 16-bit raster, else the k_analyze instance of the sample width and the level's lag."""
    lvl = cfg["level"]
    if wave and np.dtype(dt).itemsize <= 2:
        pcap = {3: 4, 4: 4, 5: 5, 6: 6}[lvl]
        return ("k_analyze_w (+ k_analyze over the partial-frame list, same phase)",
                f"_ZN3fra11k_analyze_wILi8ELi{pcap}ELb{1 if k17 else 0}E")
    b32 = 1 if cfg["norm"] == 24 or np.dtype(dt).itemsize > 2 else 0
    lag = 12 if lvl >= 7 else (8 if lvl >= 3 else 0)
    return "k_analyze", f"_ZN3fra9k_analyzeILb{b32}ELi{lag}E"


def codegen_stats(kernel, prefix=None):
    """code bytes, VGPRs, SGPRs and spill counts of ``kernel`` (the instance whose mangled name starts with
    ``prefix`` when given) in the loaded library's gfx950 code object (tools/codeobj_stats.py), so codegen
    regressions show up in the bench record."""
    try:
        sys.path.insert(0, str(ROOT / "tools"))
        import codeobj_stats
        rows = [r for r in codeobj_stats.stats(str(N_LIB_PATH()), kernel)
                if (r["kernel"].startswith(prefix) if prefix else
                    (r["kernel"].split("I")[0].endswith(kernel) or f"{len(kernel)}{kernel}" in r["kernel"]))]
        if not rows:
            return None
        r = max(rows, key=lambda r: r["code_bytes"])
        return {k: r.get(k) for k in ("kernel", "code_bytes", "vgpr", "sgpr", "sgpr_spill", "vgpr_spill", "lds",
                                      "scratch", "s_nop", "writelane", "readlane")}
    except Exception as e:  # reported, never fatal
        return {"error": f"{type(e).__name__}: {e}"}


def N_LIB_PATH():
    from flac_raster import _native
    return _native._LIB_PATH


def inrun_kernel_stats(args, out_dir):
    """rocprofv3 --kernel-trace --stats over a child run that executes ONLY the plan (``--child``: the
    warmup + timed executes of this config, no parity launches, no CPU / e2e legs) in the roofline's serial
    timing mode (each kernel alone, as the HIP events of ``roofline.achieved`` measure it), so the
    per-kernel averages are those launches.  The stats CSV is copied to ``out_dir`` (tagged with the
    kernel-source hash); returns {kernel: {calls, avg_ms, min_ms, max_ms}}."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    tmp = tempfile.mkdtemp(prefix="fra_kt_", dir="/tmp")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--",
           sys.executable, str(ROOT / "bench.py"), "--config", args.config, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--child", "--child-serial"]
    if args.level is not None:
        cmd += ["--level", str(args.level)]
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       timeout=float(os.environ.get("FRA_PMC_TIMEOUT", "150")), check=True)
    except (subprocess.SubprocessError, OSError):
        shutil.rmtree(tmp, ignore_errors=True)
        return None
    f = next(Path(tmp).rglob("*kernel_stats.csv"), None)
    out = {}
    if f is not None:
        for r in csv.DictReader(open(f)):
            # (two instances of one kernel -- k_analyze_w's 17- and 16-bit -- keep the one with the most calls: the
            # instance the plan settled on; the settle execute's is in the committed CSV)
            if _short(r["Name"]) in out and out[_short(r["Name"])]["calls"] >= int(r["Calls"]):
                continue
            out[_short(r["Name"])] = {"calls": int(r["Calls"]), "avg_ms": round(float(r["AverageNs"]) / 1e6, 5),
                                     "min_ms": round(float(r["MinNs"]) / 1e6, 5),
                                     "max_ms": round(float(r["MaxNs"]) / 1e6, 5)}
        if out_dir:
            try:
                Path(out_dir).mkdir(parents=True, exist_ok=True)
                shutil.copy(f, Path(out_dir) / f"{args.config}_n1_{sources_sha()}_timed_kernel_stats.csv")
            except OSError:
                pass
    shutil.rmtree(tmp, ignore_errors=True)
    return out or None


def reference_cpu_probe():
    """the reference's own CPU path is pyflac (libFLAC 1.4.3) or the ``flac`` CLI on
    the node.  Probed, never installed; absent here, so the CPU baseline stays the oracle port."""
    import importlib.util
    pyflac = importlib.util.find_spec("pyflac") is not None
    cli = shutil.which("flac")
    return {"pyflac_importable": pyflac, "flac_cli": cli, "libflac_on_node": bool(pyflac or cli)}


def committed_profile(args, cfg, kernel):
    f = ROOT / "profiles" / f"traffic_{args.config}.json"
    if not f.exists():
        return {"source": "none"}
    try:
        d = json.loads(f.read_text())
    except ValueError:
        return {"source": "unreadable"}
    if d.get("sources_sha") != sources_sha():
        return {"source": f"{d.get('source')} is STALE (kernel sources changed since it was measured)"}
    out = {"source": d.get("source"), "traffic": d.get(kernel)}
    for k in ("waves", "valu_insts", "valu_per_wave", "busy_cycles_per_xcd"):
        if f"{kernel}:{k}" in d:
            out[k] = d[f"{kernel}:{k}"]
    return out


# ------------------------------------------------------------------------------------- rank launcher
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_gpus():
    """GPUs this process may use, counted WITHOUT initialising HIP (torch.cuda.device_count() reads the
    KFD topology on this image; no HIP call), so the launcher can still start fresh rank processes."""
    try:
        import torch
        return int(torch.cuda.device_count())
    except Exception:
        return 0


def launch_ranks(n, argv):
    """``bench.py --gpus N`` without a launcher (no WORLD_SIZE): start N fresh rank processes of this script,
    one per GPU (RANK = LOCAL_RANK = r, WORLD_SIZE = N, MASTER_ADDR 127.0.0.1), before this process touches the
    GPU; relay rank 0's JSON line and fail if any rank fails.  More ranks than visible GPUs is refused unless
    FRA_DIST_BACKEND=gloo asks for a rehearsal (ranks share GPUs; the line is labelled ``rehearsal``)."""
    ndev = visible_gpus()
    env0 = dict(os.environ)
    if n > ndev:
        if env0.get("FRA_DIST_BACKEND") != "gloo" or ndev < 1:
            raise SystemExit(f"bench.py --gpus {n}: only {ndev} GPU(s) visible (set FRA_DIST_BACKEND=gloo to "
                             f"rehearse {n} ranks on fewer GPUs)")
    port = _free_port()
    outs, procs = [], []
    for r in range(n):
        env = dict(env0, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), FRA_BENCH_LAUNCHED="1")
        out = tempfile.TemporaryFile(mode="w+")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve()), *argv], env=env,
                                      stdout=out, stderr=None))
    failed = None
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad and failed is None:
            failed = bad
            for p in procs:  # our own children, by PID: a rank that died leaves the others at a barrier
                if p.poll() is None:
                    p.terminate()
        if all(c is not None for c in codes):
            break
        time.sleep(0.2)
    for r, out in enumerate(outs):
        out.seek(0)
        text = out.read()
        out.close()
        if r == 0:
            sys.stdout.write(text)
            sys.stdout.flush()
        elif text.strip():
            sys.stderr.write(f"[rank {r}] {text}")
    if failed is not None:
        raise SystemExit(f"bench.py --gpus {n}: rank(s) failed: " +
                         ", ".join(f"rank {r} exit {c}" for r, c in failed))


# ------------------------------------------------------------------------------------- main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="GPUs (one rank process each); without a launcher N > 1 starts the N ranks itself")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c4", choices=sorted(CONFIGS))
    ap.add_argument("--level", type=int, default=None)
    ap.add_argument("--cpu-budget", type=float, default=12.0, help="seconds of 1-core CPU oracle work (rank 0)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--scaling", default="strong", choices=["weak", "strong"])
    ap.add_argument("--shard", default=None, metavar="R/N",
                    help="time rank R's share (--split) of the scene for an N-GPU strong-scaling run, on this one GPU "
                         "(projection of the multi-GPU step; DESIGN.md section 7)")
    ap.add_argument("--split", default="frames", choices=["frames", "strided", "lpt"],
                    help="strong scaling: (tile, frame range) work items of equal cost per rank (default; "
                         "fra_plan_create_ranged), the same over the tiles in strided order, or whole tiles by LPT")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="skip the in-run rocprofv3 counter passes")
    ap.add_argument("--no-trace", action="store_true", help="skip the in-run rocprofv3 kernel-trace pass")
    ap.add_argument("--prof-dir", default=os.environ.get("FRA_PROF_DIR", str(ROOT / "gpurun_out" / "bench_prof")),
                    help="where the timed-launch kernel-stats CSV of the in-run trace pass is copied")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg (forced-17-bit steps, per-kernel times and "
                         "roofline, CPU baselines, e2e, C2 size ratio and shim latency, rocprofv3 trace and counter "
                         "passes; each still subject to its --no-* switch).  Without it the run is set-up, warmup, "
                         "the timed steps and the result line only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last one computed (stream table, sampled frame bytes) "
                         "as DIR/<name>.npy")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)  # PMC child: steps only
    ap.add_argument("--child-serial", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-mp-child", nargs=2, type=int, metavar=("PROCS", "TILES"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cpu_mp_child:
        cpu_mp_child(args.config, *args.cpu_mp_child, level=args.level)
        return
    cfg = dict(CONFIGS[args.config])
    if args.level is not None:
        cfg["level"] = args.level

    if "WORLD_SIZE" not in os.environ:
        if args.gpus is not None and args.gpus > 1 and not (args.child or args.shard):
            launch_ranks(args.gpus, sys.argv[1:])  # N fresh rank processes; this one never touches the GPU
            return
        if args.gpus is not None and args.gpus < 1:
            raise SystemExit("--gpus must be >= 1")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" in os.environ and args.gpus is not None and args.gpus != world:
        raise SystemExit(f"bench.py --gpus {args.gpus} under a launcher with WORLD_SIZE={world}")
    rehearsal = None
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist_mod
        # RCCL over xGMI on a GPU node; FRA_DIST_BACKEND=gloo rehearses several ranks on one GPU
        backend = os.environ.get("FRA_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        ndev = torch.cuda.device_count()
        if world > ndev:
            if backend != "gloo":
                raise SystemExit(f"{world} ranks but {ndev} GPU(s): FRA_DIST_BACKEND=gloo rehearses ranks sharing GPUs")
            rehearsal = f"{world} ranks on {ndev} GPU(s)"
        if backend == "nccl":
            torch.cuda.set_device(local)
        dist_mod.init_process_group(backend=backend)
        dist = dist_mod

    from flac_raster import _native as N

    def barrier():
        if dist is not None:
            dist.barrier()

    def allgather(vals):
        if dist is None:
            return [list(vals)]
        import torch
        dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor(list(vals), dtype=torch.float64, device=dev)
        out = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(out, t)
        return [o.cpu().tolist() for o in out]

    ctx = N.Context(local if N.device_count() > local else 0)
    B, H, W = cfg["bands"], cfg["H"], cfg["W"]
    dt = np.dtype(cfg["dtype"])
    raster_bytes = B * H * W * dt.itemsize
    dev_raster = ctx.alloc(raster_bytes)
    weak = args.scaling == "weak"
    ctx.synth(cfg["kind"], SEED + (rank if weak else 0), B, H, W, dev_raster)
    wins = tiles(H, W, cfg["tile"])
    shard_of = None
    if args.shard:
        sr, sn = (int(x) for x in args.shard.split("/"))
        if world != 1 or not 0 <= sr < sn:
            raise SystemExit("--shard R/N needs a single process and 0 <= R < N")
        shard_of = (sr, sn)
    nparts = shard_of[1] if shard_of is not None else (1 if weak else world)
    if shard_of is not None:
        rank = shard_of[0]
    if args.split in ("frames", "strided") or nparts == 1:
        from flac_raster.tiles import frame_split
        items = frame_split(wins, nparts, stride=nparts if args.split == "strided" else 1)[rank if nparts > 1 else 0]
    else:
        owner = lpt_shard(wins, nparts)
        items = [(i, 0, -(-(wins[i][2] * wins[i][3]) // 4096)) for i in range(len(wins)) if owner[i] == rank]
    mine = [i for i, _, _ in items]
    my_wins = [wins[i] for i in mine]
    full = all(f0 == 0 and n * 4096 >= wins[i][2] * wins[i][3] for i, f0, n in items)
    ranges = None if full else [(f0, n) for _, f0, n in items]
    plan = N.Plan(ctx, dev_raster, True, dt, B, (H * W, W, 1), my_wins, cfg["level"], 4096, cfg["norm"],
                  frame_ranges=ranges)
    wave_plan = bool(plan.flags() & 4)  # FRA_PLAN_WAVE: full frames on k_analyze_w
    k17_plan = True

    if args.child:  # rocprofv3 child: the plan's launches only
        if args.child_serial:  # the roofline's mode: serial executes, each kernel alone on the device
            plan.enable_timing(True)
        # settle the k_analyze_w instance as the timed run's synced warmup does (FRA_PLAN_KEEP17 follows the first
        # execute's count; that execute ran on the 17-bit instance and shows as its own kernel name in the trace)
        plan.execute()
        plan.sync()
        for _ in range(args.warmup + args.steps):
            plan.execute()
        plan.sync()
        plan.close()
        ctx.free(dev_raster)
        return

    # (untimed: settles the k_analyze_w instance, FRA_PLAN_KEEP17, even at --warmup 0).  A plan's first execute
    # has no count yet and runs the 17-bit instance: its synced time is reported as first_execute_ms (cold: it
    # also pays the first launch of every kernel)
    t0 = time.perf_counter()
    plan.execute()
    plan.sync()
    first_ms = (time.perf_counter() - t0) * 1e3
    first_inst = (17 if plan.flags() & 8 else 16) if wave_plan else None
    # plan set-up, before the W warmup steps: SETTLE executes bring the device to its steady state (r06,
    # profiles/r06_keep17_order.txt: after 4 executes the next 20 still ran ~3-4 % slower than later segments of 20)
    for _ in range(SETTLE):
        plan.execute()
    plan.sync()
    for _ in range(args.warmup):
        plan.execute()
    plan.sync()
    barrier()
    plan.sync()
    inst = []  # the k_analyze_w instance each timed execute ran (flags() & 8 right after it: the one it launched)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        plan.execute()
        inst.append(plan.flags() & 8)
    plan.sync()
    t1 = time.perf_counter()
    barrier()
    dt_s = t1 - t0
    inst = [17 if f else 16 for f in inst] if wave_plan else None
    if args.dump_outputs:
        dump_outputs(Path(args.dump_outputs), ctx, plan, f"rank{rank}_" if world > 1 else "")
    # the legs below re-run the steps: only under --full (and for a --shard projection line, which is made of them)
    extra = args.full or shard_of is not None
    # the same pipelined steps forced onto the 17-bit instance (what a plan runs before its count arrives, and on
    # data where more than 1/32 of the waves need bit 16): the adaptive pick's worth, reported beside ms_per_step
    k17_ms = None
    if extra and wave_plan and os.environ.get("FRA_KEEP17") is None:
        os.environ["FRA_KEEP17"] = "1"  # read by every execute (getenv)
        try:
            plan.execute()
            plan.sync()
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                plan.execute()
            plan.sync()
            k17_ms = (time.perf_counter() - t0) / args.steps * 1e3
            barrier()
        finally:
            del os.environ["FRA_KEEP17"]
    # per-kernel launch times (roofline): the same steps again, serial, HIP events between kernels
    kms, nexec = [0.0] * 4, 0
    if extra:
        plan.enable_timing(True)
        for _ in range(args.steps):
            plan.execute()
        plan.sync()
        kms, nexec = plan.timing()
        plan.enable_timing(False)
    infos, total = plan.result()
    # the k_analyze_w instance the plan settled on (FRA_PLAN_KEEP17: kept residuals up to 17 bits, else 16)
    k17_plan = bool(plan.flags() & 8)
    # pixels of this rank's frames (a partial tile counts its frame range only)
    my_px = sum(min(wins[i][2] * wins[i][3], (f0 + n) * 4096) - f0 * 4096 for i, f0, n in items)
    my_in_bytes = my_px * B * dt.itemsize
    per_launch_ms = [k / max(1, nexec) for k in kms]
    ranks = allgather([dt_s, per_launch_ms[1], sum(per_launch_ms), len(my_wins), my_px, total])
    T = max(r[0] for r in ranks)
    out_bytes_all = sum(r[5] for r in ranks)

    # dominant kernel: the larger of analyze (1) and pack (3); algorithmic bytes per launch =
    # input bytes + frame bytes of the units this rank's launch processes
    dom = 1 if per_launch_ms[1] >= per_launch_ms[3] else 3
    dom_name = {1: "k_analyze", 3: "k_assemble"}[dom]
    alg_bytes = my_in_bytes + total
    step_ms_local = sum(per_launch_ms)
    achieved = path_gbps = None  # (no per-kernel times without the serial leg above)
    if extra:
        achieved = alg_bytes / (per_launch_ms[dom] * 1e-3) / 1e9
        path_gbps = alg_bytes / (step_ms_local * 1e-3) / 1e9

    if shard_of is not None:  # projection line: this rank's share only, not a job throughput
        sh = {"shard": f"{shard_of[0]}/{shard_of[1]}", "config": cfg["workload"], "tiles": len(my_wins),
              "pixels": my_px, "ms_per_step": round(T / args.steps * 1e3, 4),
              "kernel_ms_per_launch": {"minmax": round(per_launch_ms[0], 4), "analyze": round(per_launch_ms[1], 4),
                                       "frame_scan": round(per_launch_ms[2], 4),
                                       "pack": round(per_launch_ms[3], 4)},
              "fixed_ms_per_step": round(T / args.steps * 1e3 - per_launch_ms[1], 4),
              "projected_job_mpix_s": round(H * W / (T / args.steps) / 1e6, 2),
              "split": args.split, "frames": sum(n for _, _, n in items),
              "note": "projected, unmeasured on hardware: one GPU runs this rank's share of the scene ("
                      + {"frames": "equal frame ranges", "strided": "equal frame ranges over strided tiles",
                         "lpt": "LPT tiles"}[args.split]
                      + "); the N-GPU step is the slowest rank's step"}
        print(json.dumps(sh), flush=True)
        plan.close()
        ctx.free(dev_raster)
        return
    result = None
    if rank == 0:
        scene_px = H * W
        job_px = scene_px * (world if weak else 1)
        value = job_px * args.steps / T / 1e6
        cpu = cpu_mp = None
        if args.full and not args.no_cpu and world == 1:
            gi = {i: infos[j] for j, i in enumerate(mine)}
            dev_out, _ = plan.device_output()

            def tile_bytes(idx):  # this tile's frames, copied D2H on demand
                if idx not in gi:
                    return None
                buf = np.empty(max(1, gi[idx].frame_bytes), np.uint8)
                N.load().fra_memcpy_d2h(ctx.h, buf.ctypes.data, dev_out + gi[idx].offset, gi[idx].frame_bytes)
                return buf[:gi[idx].frame_bytes].tobytes()
            cb = cpu_baseline(cfg, wins, tile_bytes, args.cpu_budget)
            cpu = {"value": round(cb["value"], 3), "unit": "MPix/s", "cores": 1, "kind": "port",
                   "sample": f"first {cb['tiles']} tiles ({cb['pixels']} px, {cb['seconds']:.1f} s) of the same "
                             f"scene through oracle/fr_oracle.c normalize+encode (FRA-1, 1 thread, "
                             f"{platform.processor() or platform.machine()}, os.cpu_count()={os.cpu_count()}); "
                             f"bytes equal to GPU for {cb['checked'] - cb['mismatches']}/{cb['checked']} tiles. "
                             f"Plain scalar C restatement of FRA-1, slower than the reference's numpy "
                             f"normalisation alone (19.3 MPix/s per C4 tile, BASELINE.md 1): not a proxy for "
                             f"libFLAC or the reference CPU path (measurable only if `reference_cpu` finds pyflac / flac)"}
            # B-mp: the same port over the host's core share (OMP_NUM_THREADS on the box = its CPU share)
            procs = int(os.environ.get("OMP_NUM_THREADS") or 0) or min(16, os.cpu_count() or 1)
            px_per_tile = cb["pixels"] / max(1, cb["tiles"])
            ntiles = int(min(len(wins), max(procs, cb["value"] * 1e6 * 6.0 * procs / max(1.0, px_per_tile))))
            try:
                r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--config", args.config,
                                    "--cpu-mp-child", str(procs), str(ntiles)] +
                                   (["--level", str(args.level)] if args.level is not None else []),
                                   capture_output=True, text=True, timeout=240, check=True)
                mp = json.loads(r.stdout.strip().splitlines()[-1])
                cpu_mp = {"value": round(mp["value"], 3), "unit": "MPix/s", "cores": mp["procs"], "kind": "port",
                          "sample": f"first {mp['tiles']} tiles ({mp['pixels']} px) over {mp['procs']} processes, "
                                    f"{mp['seconds']:.2f} s wall (BASELINE.md B-mp)"}
            except (subprocess.SubprocessError, OSError, ValueError, KeyError, IndexError) as e:
                cpu_mp = {"value": None, "error": type(e).__name__}
        # PCIe-inclusive end-to-end (not `value`): host raster -> pipelined H2D / kernels / D2H -> host frames
        e2e = None
        if args.full and not args.no_e2e and world == 1:
            if raster_bytes <= (8 << 30):
                e2e = measure_e2e(N, ctx, cfg, dt, B, H, W, my_wins, my_px, dev_raster, plan)
            else:  # the whole raster is never page-locked: the bounded ring path (fra_plan_encode_ring)
                try:
                    e2e = measure_e2e_ring(N, ctx, cfg, dt, B, H, W, my_wins, my_px, dev_raster, plan)
                except Exception as e:  # reported, never fatal for the headline line
                    e2e = {"value": None, "error": f"{type(e).__name__}: {e}"}
        # size vs libFLAC: only pinned for C2 (sample_rgb, 178,857 frame bytes at -c 5)
        size_c2 = None
        if args.full:
            try:
                from flac_raster.tiff import read_geotiff
                rgb, _ = read_geotiff(ROOT / "tests" / "golden" / "sample_rgb.tif")
                _, fr = N.encode_windows(rgb, [(0, 0, 256, 256)], level=5, norm=16, device=ctx.device)
                size_c2 = round(len(fr) / 178857.0, 5)
            except Exception:
                size_c2 = None
        # pyflac-shim latency per stream on C2 (sample_rgb, 65,536 x 3 int16 samples; the reference's
        # per-tile call shape: StreamEncoder(...).process(audio); finish())
        shim = None
        if args.full:
            try:
                shim = measure_shim_c2(N)
            except Exception as e:  # reported, never fatal for the headline line
                shim = {"error": f"{type(e).__name__}: {e}"}
        # counters of the dominant kernel: in-run passes (this build), else the committed file if current.
        # The passes run in a child process: release this process's device buffers first.
        plan.close()
        ctx.free(dev_raster)
        plan = dev_raster = None
        kstats = None
        if args.full and not args.no_trace and world == 1:
            kstats = inrun_kernel_stats(args, args.prof_dir)
        pm = None
        if args.full and not args.no_pmc and world == 1:
            pm = inrun_pmc(args, dom_name)
            if "traffic" not in pm and "valu_insts" not in pm:
                pm = None
        # roofline of the dominant kernel (--full: it needs the per-kernel times and the counters)
        if args.full:
            if pm is None:
                pm = committed_profile(args, cfg, dom_name)
            # the kernel the analysis phase's HIP events time: k_analyze_w (+ the partial-frame k_analyze list beside
            # it) on 16-bit LUT plans at levels 3-6, k_analyze otherwise -- from the config, so lines without in-run
            # counters (N > 1) name it too
            dom_label = dom_name
            codegen = codegen_stats(dom_name)
            if dom_name == "k_analyze":
                dom_label, prefix = analysis_kernel(cfg, dt, wave_plan, k17_plan)
                codegen = codegen_stats(prefix.split("ILb")[0].split("ILi")[0].rsplit("fra", 1)[1].lstrip("0123456789"),
                                        prefix)
            hbm_frac = achieved / HBM_PEAK_GBPS
            valu_frac = None
            if pm.get("valu_insts") and pm.get("busy_cycles_per_xcd"):
                valu_frac = pm["valu_insts"] * VALU_CYC / (SIMDS * pm["busy_cycles_per_xcd"])
            bound = "hbm" if valu_frac is None or hbm_frac >= valu_frac else "valu"
        per_rank = [{"rank": k, "ms_per_step": round(r[0] / args.steps * 1e3, 4),
                     "analyze_ms": round(r[1], 4) if args.full else None,
                     "serial_ms": round(r[2], 4) if args.full else None, "tiles": int(r[3]), "pixels": int(r[4]),
                     "frame_bytes": int(r[5])} for k, r in enumerate(ranks)]
        mean_t = sum(r[0] for r in ranks) / len(ranks)
        result = {
            "metric": "raster MPixels/sec encoded at -c 5 + size ratio vs libFLAC, 1/2/4/8 GPU",
            "value": round(value, 2),
            "unit": "MPix/s",
            "n_gpus": world,
            **({"rehearsal": rehearsal} if rehearsal else {}),
            "steps": args.steps,
            "warmup": args.warmup,
            "settle_executes": 1 + SETTLE,
            "ms_per_step": round(T / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": ("u16->i16 (int32 analysis, exact integer autocorrelation on i8 MFMA)" if cfg["norm"] == 16
                      else "f32->i32 (int64 analysis, f32 chunk partials + f64 autocorrelation tree)"),
            "data": "synthetic (flac_raster.synth, seed 20260227; device-generated, integer-exact numpy mirror)",
            "config": {"workload": cfg["workload"], "level": cfg["level"], "tiles": len(wins),
                       "raster_bytes": raster_bytes, "compressed_bytes": int(out_bytes_all),
                       "compression_ratio": round(raster_bytes * (world if weak else 1) / max(1.0, out_bytes_all), 4),
                       "msamples_per_s": round(job_px * B * args.steps / T / 1e6, 1),
                       "parallelism": (f"{world} scene(s), one per GPU, no collective" if weak else
                                       "one scene over {} GPU(s), no collective: {}".format(world, {
                                           "frames": "(tile, frame range) items of equal cost per rank (frames + partial-frame charge)",
                                           "strided": "(tile, frame range) items of equal cost per rank, "
                                                      "tiles in strided order",
                                           "lpt": "whole tiles by LPT on pixel count"}[args.split])),
                       "split": args.split,
                       "serial_ms_per_step": round(step_ms_local, 4) if args.full else None},
            "per_rank": per_rank,
            "imbalance": round(T / mean_t, 4) if mean_t > 0 else None,
            "analysis_instance": ({
                "timed_executes": {str(b): inst.count(b) for b in sorted(set(inst))},
                "first_execute": first_inst, "first_execute_ms": round(first_ms, 4),
                "ms_per_step_forced_17bit": round(k17_ms, 4) if k17_ms is not None else None,
                "note": "k_analyze_w keeps residuals up to 17 or 16 bits; a plan picks per execute from an earlier "
                        "execute's count of waves that needed bit 16 (FRA_PLAN_KEEP17). The timed executes re-encode "
                        "the same scene, so they run the instance the settle execute's count chose; bytes are equal "
                        "either way. first_execute_ms is the plan's first (17-bit, cold) execute, synced alone"}
                if inst is not None else None),
        }
        if args.full:
            result.update({
                "roofline": {"bound": bound, "kernel": dom_label, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS,
                             "unit": "GB/s", "frac": round(hbm_frac, 5), "traffic": pm.get("traffic"),
                             "valu_issue_frac": round(valu_frac, 4) if valu_frac is not None else None,
                             # whole path: algorithmic bytes of the step over the TIMED (pipelined) step, and over the
                             # serial sum of the kernels (each alone, HIP events)
                             "whole_path_frac": round(
                                 out_bytes_all / max(1e-12, T / args.steps) / 1e9 / HBM_PEAK_GBPS
                                 + raster_bytes * (world if weak else 1) / max(1e-12, T / args.steps)
                                 / 1e9 / HBM_PEAK_GBPS, 5),
                             "whole_path_frac_serial": round(path_gbps / HBM_PEAK_GBPS, 5),
                             "whole_path_gbps_serial": round(path_gbps, 2),
                             "codegen": codegen,
                             "alg_bytes_per_launch": int(alg_bytes),
                             "kernel_ms_per_launch": {"minmax": round(per_launch_ms[0], 4),
                                                      "analyze": round(per_launch_ms[1], 4),
                                                      "frame_scan": round(per_launch_ms[2], 4),
                                                      "pack": round(per_launch_ms[3], 4)},
                             "counters": pm,
                             "valu_note": f"valu_issue_frac = SQ_INSTS_VALU x {VALU_CYC} cyc / ({SIMDS} SIMDs x "
                                          "GRBM_GUI_ACTIVE/8) of the same launch"},
                "kernel_stats": ({"source": "rocprofv3 --kernel-trace --stats over bench.py --child --child-serial "
                                            f"(the plan's {args.warmup}+{args.steps} executes only, serial as the "
                                            "roofline's HIP events, no parity launches), CSV "
                                            f"{args.config}_n1_{sources_sha()}_timed_kernel_stats.csv",
                                  "sources_sha": sources_sha(), "kernels": kstats} if kstats else None),
                "reference_cpu": reference_cpu_probe(),
                "cpu_baseline": cpu,
                "cpu_baseline_mp": cpu_mp,
                "size_ratio_vs_libflac_c2": size_c2,
                "pyflac_shim_c2": shim,
                "e2e": e2e,
            })
        print(json.dumps(result), flush=True)
    if plan is not None:
        plan.close()
        ctx.free(dev_raster)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def measure_shim_c2(N):
    from flac_raster.encoder import StreamEncoder
    from flac_raster.normalization import normalize_to_audio
    from flac_raster.tiff import read_geotiff

    rgb, _ = read_geotiff(ROOT / "tests" / "golden" / "sample_rgb.tif")
    audio, _ = normalize_to_audio(rgb.transpose(1, 2, 0).reshape(-1, 3), 16)
    out = []

    def one(enc):
        enc.process(audio)
        enc.finish()

    N.release_pinned_pool()
    t0 = time.perf_counter()
    one(StreamEncoder(44100, lambda b, n, s, f: out.append(n), compression_level=5, blocksize=4096))  # cold
    t_cold = time.perf_counter() - t0
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        one(StreamEncoder(44100, lambda b, n, s, f: out.append(n), compression_level=5, blocksize=4096))
    t_new = (time.perf_counter() - t0) / reps
    return {"ms_first_stream": round(t_cold * 1e3, 3), "ms_per_stream": round(t_new * 1e3, 3),
            "what": "StreamEncoder(...).process(65,536 x 3 int16) + finish() incl. 19 write callbacks, a new encoder "
                    "per stream (the reference's per-tile shape); the first stream builds the GPU plan, later "
                    "ones of the same shape take it from the process-wide plan pool"}


def measure_e2e(N, ctx, cfg, dt, B, H, W, my_wins, my_px, dev_raster, dev_plan):
    """Host raster -> frames in host memory through the pipelined ``fra_plan_encode_host`` (row bands:
    H2D of band b+1 || kernels of band b || D2H of band b-1).  Page-locked buffers (what
    ``GeoTIFF.read(pinned=True)`` delivers; allocated once, outside the timed region) and, for reference,
    pageable numpy buffers.  Also the bare PCIe copy times of the same bytes."""
    host = N.pinned_empty((B, H, W), dt)
    ctx.d2h(host, dev_raster)
    plan = N.Plan(ctx, None, False, dt, B, (H * W, W, 1), my_wins, cfg["level"], 4096, cfg["norm"])
    cap, nbands = plan.capacity()
    out = N.pinned_empty(cap, np.uint8)
    total = plan.encode_host(host, out)  # warm-up
    ref = dev_plan.download()[1]
    equal = bytes(out[:total]) == ref
    del ref
    reps = 3
    t0 = time.perf_counter()
    for _ in range(reps):
        total = plan.encode_host(host, out)
    te = (time.perf_counter() - t0) / reps
    # bare copies of the same bytes (pinned): the PCIe floor of this path
    dev_out, _ = plan.device_output()
    t0 = time.perf_counter()
    ctx.h2d(dev_raster, host)
    t_h2d = time.perf_counter() - t0
    t0 = time.perf_counter()
    N.load().fra_memcpy_d2h(ctx.h, out.ctypes.data, dev_out, total)
    t_d2h = time.perf_counter() - t0
    res = {"value": round(my_px / te / 1e6, 2), "unit": "MPix/s", "ms": round(te * 1e3, 2), "bands": nbands,
           "what": "page-locked host raster -> pipelined row-band H2D / kernels / D2H -> page-locked host frames (1 GPU)",
           "bytes_equal_device_path": bool(equal),
           "h2d_ms_alone": round(t_h2d * 1e3, 2), "d2h_ms_alone": round(t_d2h * 1e3, 2),
           "pcie_floor_ms": round(max(t_h2d, t_d2h) * 1e3, 2)}
    # pageable variant (a plain numpy raster and output buffer)
    hp = np.empty((B, H, W), dt)
    hp[...] = host
    op = np.empty(cap, np.uint8)
    plan.encode_host(hp, op)
    t0 = time.perf_counter()
    plan.encode_host(hp, op)
    tp = time.perf_counter() - t0
    res["pageable"] = {"value": round(my_px / tp / 1e6, 2), "ms": round(tp * 1e3, 2)}
    plan.close()
    del out, hp, op
    if os.environ.get("FRA_E2E_FILE", "1") != "0" and len(my_wins) == len(tiles(H, W, cfg["tile"])):
        try:
            res["e2e_file"] = measure_e2e_file(N, cfg, host, dev_plan, res["pcie_floor_ms"])
        except Exception as e:  # reported, never fatal for the headline line
            res["e2e_file"] = {"error": f"{type(e).__name__}: {e}"}
    del host
    return res


def measure_e2e_ring(N, ctx, cfg, dt, B, H, W, my_wins, my_px, dev_raster, dev_plan):
    """Host raster -> frames in host memory with BOUNDED page-locked memory (``fra_plan_encode_ring``): the
    scene sits in pageable host memory (copied there untimed, standing in for the source file's pages), a
    producer copies its row bands into a page-locked ring of two host bands + a step (16 threads), and the
    pipelined encoder copies each band H2D once the producer published it and releases its ring rows after
    the copy; frames land in a lazily committed pageable buffer.  The PCIe floor is the raster's H2D at the
    page-locked rate measured on the ring itself."""
    from concurrent.futures import ThreadPoolExecutor

    host = np.empty((B, H, W), dt)  # pageable: the source
    ctx.d2h(host, dev_raster)
    nthreads = min(16, int(os.environ.get("OMP_NUM_THREADS") or 0) or (os.cpu_count() or 4))
    pool = ThreadPoolExecutor(nthreads)

    def fill(dst, r0, r1):  # rows split over the threads (numpy copies release the GIL)
        n = r1 - r0
        k = max(1, min(nthreads, n))
        cuts = [r0 + n * i // k for i in range(k + 1)]
        list(pool.map(lambda i: np.copyto(dst[:, cuts[i] - r0:cuts[i + 1] - r0, :], host[:, cuts[i]:cuts[i + 1], :]),
                      range(k)))

    def run():
        return N.encode_windows_ring((B, H, W), dt, my_wins, fill, cfg["level"], 4096, cfg["norm"],
                                     device=ctx.device)

    ref_i, ref_total = dev_plan.result()
    dev_out, _ = dev_plan.device_output()
    infos, frames, R = run()  # warm-up (pinned pool)
    ref = np.empty(ref_total, np.uint8)
    N.load().fra_memcpy_d2h(ctx.h, ref.ctypes.data, dev_out, ref_total)
    equal = len(frames) == ref_total and bool(np.array_equal(frames, ref))
    del ref, frames
    t0 = time.perf_counter()
    infos, frames, R = run()
    te = time.perf_counter() - t0
    total = len(frames)
    del frames
    # page-locked H2D rate on a ring-sized buffer -> the floor for the whole raster
    ring = N.pinned_empty((B, R, W), dt)
    ring[...] = host[:, :R, :]
    t0 = time.perf_counter()
    ctx.h2d(dev_raster, ring)
    t_h2d = time.perf_counter() - t0
    h2d_gbs = ring.nbytes / t_h2d / 1e9
    t0 = time.perf_counter()
    fill(ring, 0, R)
    t_fill = time.perf_counter() - t0
    fill_gbs = ring.nbytes / t_fill / 1e9
    floor_ms = host.nbytes / (h2d_gbs * 1e9) * 1e3
    res = {"value": round(my_px / te / 1e6, 2), "unit": "MPix/s", "ms": round(te * 1e3, 2),
           "what": "pageable host raster -> producer copies into a page-locked ring of 2 host bands + a step "
                   f"({nthreads} threads) -> pipelined row-band H2D / kernels / D2H -> lazily committed host frames "
                   "(fra_plan_encode_ring, 1 GPU)",
           "ring_rows": int(R), "ring_bytes": int(ring.nbytes), "raster_bytes": int(host.nbytes),
           "frame_bytes": int(total), "bytes_equal_device_path": equal,
           "h2d_pinned_gbs": round(h2d_gbs, 2), "producer_copy_gbs": round(fill_gbs, 2),
           "pcie_floor_ms": round(floor_ms, 2), "ratio_vs_pcie_floor": round(te * 1e3 / floor_ms, 3)}
    del ring, host
    pool.shutdown()
    return res


def measure_e2e_file(N, cfg, host, dev_plan, pcie_floor_ms):
    """File -> container bytes in memory (cli.py:553-602): the scene written once as a
    tiled deflate and once as a tiled LZW GeoTIFF (tile 512, predictor 2, native writer), then
    ``encode_geotiff_streaming`` -- the decode of row band b+1 on a producer thread into the bounded ring,
    overlapped with the H2D / kernels / D2H of band b (fra_plan_encode_ring, r05) -- plus the container
    assembly.
    Decode alone (the same threaded decoder into page-locked memory) is timed separately."""
    from flac_raster.geo import Affine
    from flac_raster.streaming import encode_geotiff_streaming, streaming_parts
    from flac_raster.tiff import GeoTIFF, write_geotiff

    ref = dev_plan.download()[1]
    out = {"what": "tiled GeoTIFF file (page cache) -> decode || H2D || kernels || D2H -> container bytes "
                   "in memory; decode_ms = the same threaded decode alone"}
    tmpd = tempfile.mkdtemp(prefix="fra_e2e_", dir="/tmp")
    try:
        B, H, W = host.shape
        for comp in ("deflate", "lzw"):
            p = Path(tmpd) / f"scene_{comp}.tif"
            write_geotiff(p, host, compression=comp, tile=512, predictor=2, level=6)
            g = GeoTIFF(p)
            dec = N.pinned_empty(host.shape, host.dtype)
            t0 = time.perf_counter()
            g.read_window_into(dec, 0, 0, H, W)
            t_dec = time.perf_counter() - t0
            g.close()
            same_raster = bool(np.array_equal(dec, host))
            del dec
            encode_geotiff_streaming(p, cfg["tile"], cfg["level"])  # warm-up (plan pool, pinned pool)
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                tl, streams, shape, dtype, info = encode_geotiff_streaming(p, cfg["tile"], cfg["level"])
                parts = streaming_parts(tl, streams, shape, dtype, Affine(*info.transform), info.crs, cfg["tile"])
                te = time.perf_counter() - t0
                best = te if best is None else min(best, te)
            equal = b"".join(bytes(ts.body) for ts in streams) == ref
            floor = max(t_dec * 1e3, pcie_floor_ms)
            out[comp] = {"file_bytes": p.stat().st_size, "ms": round(best * 1e3, 2),
                         "mpix_s": round(H * W / best / 1e6, 2), "decode_ms": round(t_dec * 1e3, 2),
                         "decode_mpix_s": round(H * W / t_dec / 1e6, 2),
                         "ratio_vs_max_decode_pcie": round(best * 1e3 / floor, 3),
                         "bytes_equal_device_path": bool(equal), "decoded_raster_equal": same_raster,
                         "container_bytes": int(sum(len(x) for x in parts))}
            del streams, parts
            p.unlink()
    finally:
        shutil.rmtree(tmpd, ignore_errors=True)
    return out


if __name__ == "__main__":
    main()
