"""k_analyze_w on inputs chosen for its integer arithmetic: packed sums, biased differences, the three-operand dot
chains, the zig-zag sums of the keep pass and the bit positions of the encoder.

Small rasters of full 4,096-sample frames only (tiles of 64 x 192 = 3 frames and 128 x 64 = 2 frames per band), so
every subframe goes through the wave kernel (FRA_REQUIRE_WAVE=1), with both of its instances (FRA_KEEP17=0 / 1) at
levels 3, 5 and 6.  The bytes are compared with the CPU oracle and with the workgroup kernel (FRA_ANALYZE_WG=1).

The cases, one tile each (every band of a tile holds the same kind of signal):
 1. raw values alternating the tile's min and max: audio alternating -32767 / +32767, the largest differences
    and sums of every FIXED order and of the 32-bit accumulators;
 2. a ramp and a parabola: FIXED orders 1 and 2 win, encoded through the sample path;
 3. band-limited noise: an LPC model wins and its kept residuals are encoded;
 4. a sparse spike train between the extremes: residuals of 2^16 and more (17-bit keep, or the sample path on the
    16-bit instance);
 5. white noise over the full range: VERBATIM;
 6. full-range noise in a frame's first quarter before a slow ramp: the encoded bits overrun the LDS bit buffer;
 7. a constant frame and a two-valued frame (beside frames that give the tile its range);
 8. a frame whose audio values are all multiples of 4 while the tile's extremes lie in another frame: wasted bits;
 9. a frame that starts with the largest warm-up samples before a smooth rest.
"""
import functools

import numpy as np
import pytest

import oracle as O
from flac_raster import _native as N

pytestmark = pytest.mark.gpu

FRAME = 4096
TILE_A = (64, 192)   # 3 frames per band
TILE_B = (128, 64)   # 2 frames per band
WIDTH = 192


def _to_raw(frac, dtype):
    """Map [0, 1] to the dtype's full range (0 -> min, 1 -> max)."""
    info = np.iinfo(dtype)
    return np.round(info.min + np.clip(frac, 0.0, 1.0) * (float(info.max) - float(info.min))).astype(dtype)


def _multiples_of_4(dtype):
    """Raw values whose audio value is a multiple of 4 when the tile spans the dtype's whole range (the oracle's
    own normalisation of every raw value)."""
    info = np.iinfo(dtype)
    raws = np.arange(info.min, info.max + 1, dtype=np.int64).astype(dtype)
    audio, _, _ = O.normalize(raws.reshape(-1, 1), 16)
    a = np.asarray(audio).reshape(-1).astype(np.int64)
    sel = raws[(a % 4 == 0) & (a != 0)]
    assert sel.size >= 8
    return sel


def _cases(dtype, seed):
    """[(name, tile shape, 1-D raw samples of one band)]"""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    nA, nB = TILE_A[0] * TILE_A[1], TILE_B[0] * TILE_B[1]
    t = np.arange(nA, dtype=np.float64)
    out = []
    # 1. alternating extremes
    alt = np.where(np.arange(nA) & 1, info.max, info.min).astype(dtype)
    out.append(("alternate", TILE_A, alt))
    out.append(("alternate-2f", TILE_B, alt[:nB].copy()))
    # 2. ramp / parabola (with the extremes, so that the steps are not lost in the normalisation)
    out.append(("ramp", TILE_A, _to_raw(t / (nA - 1), dtype)))
    out.append(("parabola", TILE_B, _to_raw((np.arange(nB) / (nB - 1.0)) ** 2, dtype)))
    # 3. band-limited noise
    w = rng.standard_normal(nA + 64)
    sm = np.convolve(w, np.hanning(33), mode="same")[32:32 + nA]
    sm = (sm - sm.min()) / (sm.max() - sm.min())
    out.append(("lpc-noise", TILE_A, _to_raw(sm, dtype)))
    # 4. sparse spikes between the extremes
    sp = np.full(nA, info.min, dtype=dtype)
    sp[rng.choice(nA, nA // 97, replace=False)] = info.max
    sp[5::389] = info.max
    out.append(("spikes", TILE_A, sp))
    # 5. white noise
    out.append(("white", TILE_B, rng.integers(info.min, int(info.max) + 1, nB).astype(dtype)))
    # 6. noisy quarter before a slow ramp, every frame
    ov = np.empty(nA, dtype=dtype)
    for f in range(nA // FRAME):
        ov[FRAME * f: FRAME * f + 1024] = rng.integers(info.min, int(info.max) + 1, 1024).astype(dtype)
        ov[FRAME * f + 1024: FRAME * (f + 1)] = _to_raw(0.3 + 0.1 * f + np.arange(3072) / 3072.0 * 0.05, dtype)
    out.append(("overrun", TILE_A, ov))
    # 7. constant frame, two-valued frame, a frame with the range
    c7 = np.empty(nA, dtype=dtype)
    c7[:FRAME] = _to_raw(np.array([0.37]), dtype)[0]
    two = _to_raw(np.array([0.25, 0.75]), dtype)
    c7[FRAME:2 * FRAME] = two[(rng.random(FRAME) < 0.3).astype(int)]
    c7[2 * FRAME:] = _to_raw(np.arange(FRAME) / (FRAME - 1.0), dtype)
    out.append(("constant-two", TILE_A, c7))
    # 8. multiples of 4 in frame 0, the extremes in frame 1
    m4 = _multiples_of_4(dtype)
    c8 = np.empty(nA, dtype=dtype)
    walk = np.cumsum(rng.integers(-2, 3, FRAME)) + m4.size // 2
    c8[:FRAME] = m4[np.clip(walk, 0, m4.size - 1)]
    c8[FRAME:2 * FRAME] = _to_raw(np.arange(FRAME) / (FRAME - 1.0), dtype)
    c8[2 * FRAME:] = m4[rng.integers(0, m4.size, FRAME)]
    out.append(("wasted-bits", TILE_A, c8))
    # 9. the largest warm-up samples, then smooth
    c9 = _to_raw(0.5 + 0.2 * np.sin(np.arange(nB) / 40.0), dtype)
    for f in range(nB // FRAME):
        c9[FRAME * f: FRAME * f + 8] = info.max if f == 0 else info.min
    out.append(("warm-up", TILE_B, c9))
    return out


@functools.lru_cache(maxsize=None)
def _raster(dtype, bands):
    """All cases stacked into one raster (tiles one below the other) + their windows.  Odd bands mirror the
    signal (max + min - raw): the same kind of signal, other values -- except the wasted-bits case, whose bands
    are equal (its audio values must stay multiples of 4)."""
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    cases = _cases(dt, 20260301 + bands)
    rows = sum(shape[0] for _, shape, _ in cases)
    r = np.zeros((bands, rows, WIDTH), dtype=dt)
    wins, r0 = [], 0
    for name, (h, w), x in cases:
        for b in range(bands):
            xb = x
            if name != "wasted-bits" and (b & 1):
                xb = (int(info.max) + int(info.min) - x.astype(np.int64)).astype(dt)
            r[b, r0:r0 + h, :w] = xb.reshape(h, w)
        wins.append((r0, 0, h, w))
        r0 += h
    r.setflags(write=False)
    return r, tuple(wins)


@functools.lru_cache(maxsize=None)
def _oracle_frames(dtype, bands, level):
    r, wins = _raster(dtype, bands)
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


def test_cases_reach_what_they_are_for():
    """The inputs do what their names say, read from the oracle's normalisation (no GPU work)."""
    for dtype in ("uint16", "int16", "uint8"):
        r, wins = _raster(dtype, 1)
        names = [c[0] for c in _cases(np.dtype(dtype), 0)]
        for name, (r0, c0, h, w) in zip(names, wins):
            audio, _, _ = O.normalize(r[:, r0:r0 + h, c0:c0 + w].transpose(1, 2, 0).reshape(-1, 1), 16)
            a = np.asarray(audio).reshape(-1).astype(np.int64)
            if name.startswith("alternate"):
                assert set(np.unique(a)) == {-32767, 32767} and np.all(a[1:] != a[:-1])
            if name == "wasted-bits":
                assert np.all(a[:FRAME] % 4 == 0) and np.any(a[:FRAME] % 8 != 0) and np.any(a[FRAME:2 * FRAME] & 1)
            if name == "constant-two":
                assert np.unique(a[:FRAME]).size == 1 and np.unique(a[FRAME:2 * FRAME]).size == 2
            if name == "warm-up":
                assert np.all(a[:8] == 32767)
            if name == "spikes":
                assert a.min() == -32767 and a.max() == 32767


@pytest.mark.parametrize("level", [3, 5, 6])
@pytest.mark.parametrize("bands", [1, 2, 4])
@pytest.mark.parametrize("dtype", ["uint16", "int16", "uint8"])
def test_wave_kernel_exact(monkeypatch, dtype, bands, level):
    r, wins = _raster(dtype, bands)
    exp = _oracle_frames(dtype, bands, level)
    names = [c[0] for c in _cases(np.dtype(dtype), 0)]
    monkeypatch.setenv("FRA_REQUIRE_WAVE", "1")
    for keep17 in ("0", "1"):
        monkeypatch.setenv("FRA_KEEP17", keep17)
        got = _gpu_frames(r, wins, level)
        for name, g, e in zip(names, got, exp):
            assert g == e, f"{name} ({dtype} x{bands}, level {level}, keep17={keep17}): wave kernel != oracle"
    monkeypatch.delenv("FRA_REQUIRE_WAVE")
    monkeypatch.delenv("FRA_KEEP17")
    monkeypatch.setenv("FRA_ANALYZE_WG", "1")
    wg = _gpu_frames(r, wins, level)
    for name, g, e in zip(names, wg, exp):
        assert g == e, f"{name} ({dtype} x{bands}, level {level}): workgroup kernel != oracle"
