"""bench.py's options around the timed steps: ``--dump-outputs`` writes what the last timed step computed (checked
here against the plan's own download), a plain run prints the headline line only, and ``--full`` adds the other legs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bench
from flac_raster import _native as N
from flac_raster.synth import synth_window

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("offset", "frame_bytes", "data_min", "data_max", "sample_rate", "bps", "channels", "nframes")


def _run_bench(*args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "FRA_DIST_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--config", "c3", "--steps", "3",
                        "--warmup", "1", *args], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1  # one JSON result line, nothing else on stdout
    return json.loads(lines[0])


def test_dump_outputs_equal_the_plans_download(tmp_path, monkeypatch):
    """Streams shorter and longer than the sampled chunk (an odd 700 x 900 raster in 256-tiles: 12 streams, edge
    tiles included): the table equals plan.result(), every sampled run of bytes equals the same bytes of
    plan.download(), and a second dump of the same execute is identical."""
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 12 * 150000)  # chunk 150000: edge streams shorter, others longer
    r = synth_window(4, 7, 3, 700, 900).astype(np.uint16)
    B, H, W = r.shape
    ctx = N.default_context(0)
    dev = ctx.alloc(r.nbytes)
    plan = None
    try:
        ctx.h2d(dev, r)
        wins = bench.tiles(H, W, 256)
        plan = N.Plan(ctx, dev, True, r.dtype, B, (H * W, W, 1), wins, 5, 4096, 16)
        plan.execute()
        plan.sync()
        bench.dump_outputs(tmp_path / "a", ctx, plan)
        bench.dump_outputs(tmp_path / "b", ctx, plan, prefix="rank1_")
        infos, frames = plan.download()
    finally:
        if plan is not None:
            plan.close()
        ctx.free(dev)
    names = ("streams", "frames_sample", "frames_sample_start")
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    for n in names:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"rank1_{n}.npy"))
        assert a[n].dtype in (np.float32, np.float64)
    assert a["streams"].shape == (len(wins), 8) and a["streams"].dtype == np.float64
    for i, s in enumerate(infos):
        assert a["streams"][i].tolist() == [float(getattr(s, f)) for f in FIELDS]
    chunk = a["frames_sample"].shape[1]
    assert chunk == 150000 and a["frames_sample"].shape[0] == len(wins)
    sizes = [int(s.frame_bytes) for s in infos]
    assert min(sizes) < chunk < max(sizes)  # both branches of the sampler
    raw = np.frombuffer(frames, np.uint8)
    for i, s in enumerate(infos):
        take = min(sizes[i], chunk)
        first = int(a["frames_sample_start"][i])
        assert 0 <= first <= sizes[i] - take and (first == 0 or sizes[i] > chunk)
        lo = int(s.offset) + first
        assert np.array_equal(a["frames_sample"][i, :take], raw[lo:lo + take].astype(np.float32))
        assert not a["frames_sample"][i, take:].any()
    assert any(a["frames_sample_start"] > 0)


def test_plain_run_prints_the_headline_and_dumps(tmp_path):
    d = _run_bench("--dump-outputs", str(tmp_path / "dump"))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and d["unit"] == "MPix/s" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(16384 * 16384 / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    for k in ("roofline", "kernel_stats", "cpu_baseline", "cpu_baseline_mp", "e2e", "pyflac_shim_c2"):
        assert k not in d
    assert d["analysis_instance"]["ms_per_step_forced_17bit"] is None
    files = sorted(p.name for p in (tmp_path / "dump").iterdir())
    assert files == ["frames_sample.npy", "frames_sample_start.npy", "streams.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "dump").iterdir()) <= 64_000_000
    streams = np.load(tmp_path / "dump" / "streams.npy")
    assert streams.shape == (1024, 8)
    assert int(streams[:, 1].sum()) == d["config"]["compressed_bytes"]
    assert np.array_equal(streams[1:, 0], np.cumsum(streams[:-1, 1]))  # the streams tile the output
    sample = np.load(tmp_path / "dump" / "frames_sample.npy")
    assert sample.dtype == np.float32 and sample.shape == (1024, bench.DUMP_SAMPLE_BYTES // 1024)
    assert sample.min() >= 0 and sample.max() <= 255 and np.array_equal(sample, np.floor(sample))
    assert len(np.unique(sample[:, :64])) > 64  # frame bytes, not a cleared buffer


def test_full_run_adds_the_other_legs():
    d = _run_bench("--full", "--no-cpu", "--no-e2e", "--no-pmc", "--no-trace")
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    k = d["roofline"]["kernel_ms_per_launch"]
    assert all(k[n] > 0 for n in ("minmax", "analyze", "frame_scan", "pack"))
    assert d["config"]["serial_ms_per_step"] == pytest.approx(sum(k.values()), abs=1e-3)
    assert d["analysis_instance"]["ms_per_step_forced_17bit"] > 0
    assert d["size_ratio_vs_libflac_c2"] == pytest.approx(0.99001, abs=1e-5)
    assert d["pyflac_shim_c2"]["ms_per_stream"] > 0
    assert d["cpu_baseline"] is None and d["e2e"] is None and d["kernel_stats"] is None
