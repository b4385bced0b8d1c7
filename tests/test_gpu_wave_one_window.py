"""k_analyze_w with its window count fixed per instance, the Levinson-Durbin recursion that stops per lane, and the
scalar row walk of its load phase.

Small tiles of full 4,096-sample frames only, so every subframe goes through the wave kernel (FRA_REQUIRE_WAVE=1),
with both of its instances (FRA_KEEP17=0 / 1), at levels 3, 4, 5 (one apodization window: the instances without a
window loop; level 3 has max_lpc = 6, so orders 7 and 8 of the recursion stay unused) and 6 (three windows: the
instance that keeps the runtime count).  The bytes are compared with the CPU oracle and with the workgroup kernel
(FRA_ANALYZE_WG=1).

One 768-wide, three-band raster per dtype holds every tile (the odd band mirrors the signal):

 * nine 64 x 192 tiles (3 frames per band), four abreast, so each is a tile inside a wider raster and its frames
   start at columns 0, 64 and 128 of the tile: the per-lane row walk.  Frame 0 is a full-range ramp that gives the
   tile its range, frames 1 and 2 hold one signal chosen for the Levinson-Durbin recursion and the order choice:
     - band-limited noise of three bandwidths (different orders win),
     - a two-valued pattern of period 2, 3 and 4 (autocorrelation of rank 2-3 but for the window's taper and its
       rounding: the prediction error falls to 1e-9 of R[0] after a few steps and the later steps divide by it),
     - a linear ramp with +-1 dither (near-singular autocorrelation),
     - an exact AR(1) decay,
     - white noise;
 * row-walk tiles of two frames of band-limited noise:
     - 32 x 256 at column 0 and the same samples at column 256 (row stride > width, the tile not at the raster's
       first column): every lane of a uint16 load lies in one row, the scalar walk; for uint8 (512 samples per load)
       these are per-lane walks with two rows per load,
     - 16 x 512: the scalar walk for uint8 as well (one row per load) and for uint16 (two loads per row),
     - 32 x 256 at column 64: rows that start 128 (64) bytes into the raster's rows.
   A frame starts at a multiple of 4,096 samples of its tile, so for a width that is a multiple of the samples of one
   load its first column is one too: the first-column condition of the scalar walk holds whenever the width's does
   (the kernel checks both).

The recursion's early exit (an error <= 0) is not reached by these signals, nor by any found: a windowed integer
frame's autocorrelation stays positive definite in f64 (smallest error seen: 1e-10 of R[0]).  What the signals do
reach is the recursion's divisions by a tiny error, and rows of every lane's order that the order choice and the
quantiser then read.
"""
import functools

import numpy as np
import pytest

import oracle as O
from flac_raster import _native as N

pytestmark = pytest.mark.gpu

FRAME = 4096
WIDTH = 768
SIG_TILE = (64, 192)  # 3 frames per band


def _to_raw(frac, dtype):
    """Map [0, 1] to the dtype's full range (0 -> min, 1 -> max)."""
    info = np.iinfo(dtype)
    return np.round(info.min + np.clip(frac, 0.0, 1.0) * (float(info.max) - float(info.min))).astype(dtype)


def _band_noise(rng, n, taps):
    w = rng.standard_normal(n + 2 * taps)
    sm = np.convolve(w, np.hanning(taps), mode="same")[taps:taps + n]
    return (sm - sm.min()) / (sm.max() - sm.min())


def _signals(dtype, rng):
    """[(name, 2 * FRAME samples in [0, 1] or raw)] -- frames 1 and 2 of a signal tile."""
    info = np.iinfo(dtype)
    n = 2 * FRAME
    t = np.arange(n)
    span = float(info.max) - float(info.min)
    out = []
    for taps in (5, 17, 65):
        out.append((f"noise-{taps}", _to_raw(_band_noise(rng, n, taps), dtype)))
    two = _to_raw(np.array([0.3, 0.7]), dtype)
    out.append(("period-2", two[t & 1]))
    out.append(("period-3", two[(t % 3 == 0).astype(int)]))
    out.append(("period-4", two[((t & 3) < 2).astype(int)]))
    # a ramp over a quarter of the range, +-1 raw unit of dither
    ramp = np.round(info.min + span * (0.25 + 0.25 * (t % FRAME) / (FRAME - 1.0))) + rng.choice([-1, 1], n)
    out.append(("ramp-dither", ramp.astype(dtype)))
    # x[k] = mid + amp * rho^k from each frame's start
    decay = 0.5 + 0.45 * 0.995 ** (t % FRAME)
    out.append(("ar1-decay", _to_raw(decay, dtype)))
    out.append(("white", rng.integers(info.min, int(info.max) + 1, n).astype(dtype)))
    return out


@functools.lru_cache(maxsize=None)
def _raster(dtype, bands):
    """(raster [bands, rows, WIDTH], windows, names)"""
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    rng = np.random.default_rng(20260917)
    sigs = _signals(dt, rng)
    h, w = SIG_TILE
    per_row = WIDTH // w
    sig_rows = -(-len(sigs) // per_row) * h
    rows = sig_rows + 32 + 32 + 16
    r = np.zeros((bands, rows, WIDTH), dtype=dt)
    wins, names = [], []

    def put(name, r0, c0, hh, ww, x):
        for b in range(bands):
            xb = x if not (b & 1) else (int(info.max) + int(info.min) - x.astype(np.int64)).astype(dt)
            r[b, r0:r0 + hh, c0:c0 + ww] = xb.reshape(hh, ww)
        wins.append((r0, c0, hh, ww))
        names.append(name)

    range_frame = _to_raw(np.arange(FRAME) / (FRAME - 1.0), dt)
    for i, (name, x) in enumerate(sigs):
        put(name, (i // per_row) * h, (i % per_row) * w, h, w, np.concatenate([range_frame, x]))
    walk = _to_raw(_band_noise(rng, 2 * FRAME, 9), dt)
    put("walk-256-col0", sig_rows, 0, 32, 256, walk)
    put("walk-256-col256", sig_rows, 256, 32, 256, walk)
    put("walk-256-col64", sig_rows + 32, 64, 32, 256, walk)
    put("walk-512", sig_rows + 64, 0, 16, 512, walk)
    r.setflags(write=False)
    return r, tuple(wins), tuple(names)


@functools.lru_cache(maxsize=None)
def _oracle_frames(dtype, bands, level):
    r, wins, _ = _raster(dtype, bands)
    out = []
    for (r0, c0, h, w) in wins:
        tile = r[:, r0:r0 + h, c0:c0 + w]
        inter = tile.transpose(1, 2, 0).reshape(-1, bands)
        audio, _, _ = O.normalize(inter, 16)
        out.append(O.encode(audio, O.sample_rate_for_pixels(h * w), level=level, with_header=False))
    return tuple(out)


def _gpu_frames(r, wins, level):
    infos, frames = N.encode_windows(r, list(wins), level=level, norm=16)
    return [frames[i.offset: i.offset + i.frame_bytes] for i in infos]


def test_tiles_are_what_they_are_for():
    """Whole frames only, both row walks present for each dtype, the signals as named (no GPU work)."""
    for dtype in ("uint16", "uint8"):
        r, wins, names = _raster(dtype, 1)
        per_load = 64 * (8 // np.dtype(dtype).itemsize)
        scalar = [n for n, (_, _, h, w) in zip(names, wins) if w % per_load == 0]
        vector = [n for n, (_, _, h, w) in zip(names, wins) if w % per_load != 0]
        assert "walk-512" in scalar and "noise-5" in vector
        assert ("walk-256-col256" in scalar) == (dtype == "uint16")
        for name, (r0, c0, h, w) in zip(names, wins):
            assert (h * w) % FRAME == 0 and 2 <= h * w // FRAME <= 3
            x = r[0, r0:r0 + h, c0:c0 + w].reshape(-1).astype(np.int64)
            if name.startswith("period-"):
                p = int(name[-1])
                assert np.unique(x[FRAME:]).size == 2 and np.array_equal(x[FRAME + p:], x[FRAME:-p])
            if name == "ramp-dither":
                slope = 0.25 * float(np.iinfo(dtype).max - np.iinfo(dtype).min) / (FRAME - 1.0)
                assert np.abs(np.diff(x[FRAME:2 * FRAME])).max() <= slope + 3  # (rounding + the two dithers)
        a, b = wins[names.index("walk-256-col0")], wins[names.index("walk-256-col256")]
        assert np.array_equal(r[:, a[0]:a[0] + a[2], a[1]:a[1] + a[3]], r[:, b[0]:b[0] + b[2], b[1]:b[1] + b[3]])


@pytest.mark.parametrize("level", [3, 4, 5, 6])
@pytest.mark.parametrize("dtype", ["uint16", "uint8"])
def test_wave_one_window_exact(monkeypatch, dtype, level):
    bands = 3  # (not 2: two channels are coded mid-side at levels 4-6, and with a mirrored band M / S always win)
    r, wins, names = _raster(dtype, bands)
    exp = _oracle_frames(dtype, bands, level)
    monkeypatch.setenv("FRA_REQUIRE_WAVE", "1")
    for keep17 in ("0", "1"):
        monkeypatch.setenv("FRA_KEEP17", keep17)
        got = _gpu_frames(r, wins, level)
        for name, g, e in zip(names, got, exp):
            assert g == e, f"{name} ({dtype}, level {level}, keep17={keep17}): wave kernel != oracle"
    monkeypatch.delenv("FRA_REQUIRE_WAVE")
    monkeypatch.delenv("FRA_KEEP17")
    monkeypatch.setenv("FRA_ANALYZE_WG", "1")
    wg = _gpu_frames(r, wins, level)
    for name, g, e in zip(names, wg, exp):
        assert g == e, f"{name} ({dtype}, level {level}): workgroup kernel != oracle"
