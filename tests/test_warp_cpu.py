"""CPU tests of the warped reads (no GPU needed).

* ``warp.warp_arrays`` is the rule: it equals, bit for bit, ``warp.warp_pixel``, a per-pixel loop over Python floats,
  for 8 dtypes x 3 modes x with / without nodata x two rasters x four maps.
* The rule's three consequences (identity, integer shift, power-of-two scales = ``resample.resample``), and a step-1
  grid of a dyadic affine = that affine.
* The new C ABI names are declared, exported and bound; the structures have the header's sizes; every refusal arrives
  before any GPU work; the source window of the library is the one of ``warp.source_window``.
* ``crs.py``: round trips, the central meridian, the meridian arc against a numerical integral, unknown CRSs.
* ``fit_grid``, ``suggested_grid``, the command line with ``--cpu``.
"""
import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import crs, resample, warp
from flac_raster.geo import Affine

ROOT = Path(__file__).resolve().parents[1]
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
MODES = ("nearest", "bilinear", "cubic")
NEW = ("fra_warp", "fra_decode_device_warped", "fra_warp_source_window", "fra_warp_timing", "fra_warp_paths")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ, first at {i}: got {got[i]!r} "
                             f"({int(g[i]):#x}), want {want[i]!r} ({int(w[i]):#x})")


def _raster(dt, shape, rng):
    """Half small values (7 = the nodata of the tests), half the full range; floats with NaN, +-inf and -0.0."""
    dt = np.dtype(dt)
    small = rng.integers(0, 9, size=shape)
    if dt.kind != "f":
        info = np.iinfo(dt)
        full = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64)
        return np.where(rng.random(shape) < 0.5, small, full).astype(dt)
    full = rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 6, size=shape)
    a = np.where(rng.random(shape) < 0.5, small.astype(np.float64), full).astype(dt)
    flat = a.reshape(-1)
    if flat.size > 16:
        k = rng.choice(flat.size, size=max(4, flat.size // 50), replace=False)
        flat[k] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], dt), size=k.size)
    return a


def _same_but_nan_signs(got, want, what=""):
    """Bit-exact equality, except that a NaN need only be a NaN at the same place: the resampling leaves the sign of a
    NaN result to the hardware, the warp writes the canonical one."""
    if got.dtype.kind == "f":
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        got, want = np.where(np.isnan(got), 0, got).astype(got.dtype), np.where(np.isnan(want), 0, want).astype(want.dtype)
    _same(got, want, what)


def _rotation(deg, scale, cx, cy, ox, oy):
    """Output pixel (ox, oy) lands on source (cx, cy); rotated by ``deg``, ``scale`` source pixels per output pixel."""
    c, s = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    return warp.affine_coefficients((c, -s, cx - (c * ox - s * oy), s, c, cy - (s * ox + c * oy)))


def _maps(shape, out_shape):
    h, w = shape
    oh, ow = out_shape
    return {
        "identity": warp.affine_coefficients(IDENTITY),
        "shift": warp.affine_coefficients((1.0, 0.0, -2.3, 0.0, 1.0, 1.7)),  # part of the output is outside
        "rotation": _rotation(30.0, 0.7, w / 2.0, h / 2.0, ow / 2.0, oh / 2.0),
        "grid": warp.grid_map(lambda c, r: (c * (w / ow) + 0.004 * r * r - 0.7, r * (h / oh) + 0.003 * c * c - 0.4),
                              out_shape, 4),
    }


# ------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_warp_arrays_equals_the_per_pixel_loop(dt):
    rng = np.random.default_rng(70 + np.dtype(dt).num)
    for shape, out_shape in (((7, 19), (9, 13)), ((33, 67), (11, 23))):
        a = _raster(dt, (2,) + shape, rng)
        assert (a == 7).any()  # the nodata value occurs
        for name, m in _maps(shape, out_shape).items():
            for mode in MODES:
                for nodata, fill in ((None, None), (7.0, None), (7.0, 3.0)):
                    got, filled = warp.warp_arrays(a, out_shape, m, mode, nodata, fill)
                    want, wfilled = warp.warp_pixel(a, out_shape, m, mode, nodata, fill)
                    _same(got, want, f"{name} {mode} nodata {nodata} {shape}")
                    assert filled.tolist() == wfilled.tolist() and filled.dtype == np.uint64
                    if name == "shift":
                        assert (filled > 0).all()


def test_the_identity_returns_the_input():
    rng = np.random.default_rng(1)
    for dt in DTYPES:
        a = _raster(dt, (2, 33, 67), rng)
        got, filled = warp.warp_arrays(a, (33, 67), warp.affine_coefficients(IDENTITY), "nearest")
        _same(got, a, "nearest")  # every bit, NaN and -0.0 included
        assert filled.tolist() == [0, 0]
        finite = np.where(np.isfinite(a.astype(np.float64)), a, 1).astype(dt)  # the other taps weigh 0.0: inf * 0 is NaN
        for mode in ("bilinear", "cubic"):
            got, filled = warp.warp_arrays(finite, (33, 67), warp.affine_coefficients(IDENTITY), mode)
            assert np.array_equal(got, finite) and filled.tolist() == [0, 0], (dt, mode)
            got, filled = warp.warp_arrays(finite, (33, 67), warp.affine_coefficients(IDENTITY), mode, nodata=7.0)
            assert np.array_equal(got[finite != 7], finite[finite != 7])


def test_an_integer_shift_is_a_crop_with_fill():
    rng = np.random.default_rng(2)
    for dt in (np.uint16, np.float32):
        a = _raster(dt, (3, 33, 67), rng)
        a = np.where(np.isfinite(a.astype(np.float64)), a, 2).astype(dt)
        m = warp.affine_coefficients((1.0, 0.0, 60.0, 0.0, 1.0, -5.0))  # output (R, C) is source (R - 5, C + 60)
        want = np.full((3, 20, 30), 9, dt)
        want[:, 5:, :7] = a[:, :15, 60:]
        for mode in MODES:
            got, filled = warp.warp_arrays(a, (20, 30), m, mode, fill=9)
            assert np.array_equal(got, want), (dt, mode)
            assert filled.tolist() == [20 * 30 - 15 * 7] * 3


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_power_of_two_scales_equal_the_resampling(dt):
    rng = np.random.default_rng(3 + np.dtype(dt).num)
    a = _raster(dt, (2, 16, 24), rng)
    for scale in (2.0, 4.0, 0.5, 0.25):
        out_shape = (int(16 / scale), int(24 / scale))
        m = warp.affine_coefficients((scale, 0.0, 0.0, 0.0, scale, 0.0))
        for mode in MODES:
            _same_but_nan_signs(warp.warp_arrays(a, out_shape, m, mode)[0], resample.resample(a, out_shape, mode), f"{scale} {mode}")
            got, filled = warp.warp_arrays(a, out_shape, m, mode, nodata=7.0)
            want = resample.resample(a, out_shape, mode, nodata=7.0)
            _same_but_nan_signs(got, want, f"{scale} {mode} nodata")
            if mode == "nearest":  # the picked pixels that are invalid
                assert filled.tolist() == np.count_nonzero(~resample.valid_mask(want, 7.0), axis=(1, 2)).tolist()


def test_a_step_1_grid_of_a_dyadic_affine_is_that_affine():
    rng = np.random.default_rng(4)
    a = _raster(np.float64, (2, 33, 67), rng)
    k = (0.875, -0.25, 3.125, 0.375, 1.125, -2.5)  # multiples of 1 / 8: every operation of both maps is exact
    m = warp.affine_coefficients(k)
    g = warp.grid_map(lambda c, r: (k[0] * c + k[1] * r + k[2], k[3] * c + k[4] * r + k[5]), (21, 40), 1)
    xa, ya = warp.map_coords(m, (21, 40))
    xg, yg = warp.map_coords(g, (21, 40))
    assert np.array_equal(xa, xg) and np.array_equal(ya, yg)
    for mode in MODES:
        for nodata in (None, 7.0):
            got, filled = warp.warp_arrays(a, (21, 40), g, mode, nodata)
            want, wfilled = warp.warp_arrays(a, (21, 40), m, mode, nodata)
            _same(got, want, mode)
            assert filled.tolist() == wfilled.tolist()


def test_python_refusals():
    a = np.zeros((1, 4, 4), np.int16)
    ident = warp.affine_coefficients(IDENTITY)
    with pytest.raises(ValueError, match="point samples"):
        warp.warp_arrays(a, (2, 2), ident, "average")
    with pytest.raises(ValueError, match="resampling must be"):
        warp.warp_arrays(a, (2, 2), ident, "lanczos")
    with pytest.raises(ValueError, match="out_shape"):
        warp.warp_arrays(a, (0, 2), ident)
    with pytest.raises(ValueError, match="finite"):
        warp.affine_coefficients((1, 0, math.nan, 0, 1, 0))
    with pytest.raises(ValueError, match="fill"):
        warp.warp_arrays(a, (2, 2), ident, fill=0.5)
    with pytest.raises(ValueError, match="nodata"):
        warp.warp_arrays(a, (2, 2), ident, nodata=1e9)
    with pytest.raises(ValueError, match="step"):
        warp.grid_map(lambda c, r: (c, r), (4, 4), 0)
    g = warp.grid_map(lambda c, r: (c, r), (4, 4), 2)
    with pytest.raises(ValueError, match="planes"):
        warp.warp_arrays(a, (9, 9), g)
    with pytest.raises(ValueError, match="no inverse"):
        warp.affine_map(IDENTITY, (1.0, 2.0, 0.0, 2.0, 4.0, 0.0))
    m = warp.affine_map(Affine(20.0, 0.0, 500100.0, 0.0, -20.0, 4099900.0), Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0))
    assert m.affine == (2.0, 0.0, 10.0, 0.0, 2.0, 10.0)


# ------------------------------------------------------------------------------- the ABI
def test_abi_names_and_layout():
    header = (ROOT / "include" / "flac_raster_amd.h").read_text()
    L = N.load()
    for name in NEW:
        assert name in N.EXPORTS and re.search(rf"FRA_API int {name}\(", header) and hasattr(L, name), name
    for name in ("fra_warp_map", "fra_warp_job", "#define FRA_WARP_AFFINE 0", "#define FRA_WARP_GRID 1",
                 "#define FRA_WARP_NODATA 1", "#define FRA_ABI_VERSION 3"):
        assert name in header, name
    assert L.fra_abi_version() == 3
    assert C.sizeof(N.WarpMap) == 80 and N.WarpMap.affine.offset == 16 and N.WarpMap.gx.offset == 64
    assert C.sizeof(N.WarpJob) == 208 and N.WarpJob.dst.offset == 72 and N.WarpJob.nodata.offset == 112
    assert N.WarpJob.map.offset == 128
    assert "80 bytes" in header and "208 bytes" in header
    assert (warp.AFFINE, warp.GRID, warp.FLAG_NODATA, warp.MARGIN) == (N.WARP_AFFINE, N.WARP_GRID, N.WARP_NODATA, 3)
    for name in ("warp", "decode_device_warped", "warp_timing", "warp_paths"):
        assert hasattr(N.Context, name)
    ms = C.c_float(-1.0)
    assert L.fra_warp_timing(C.byref(ms)) == 0 and ms.value >= 0.0
    assert L.fra_warp_timing(None) == -1 and L.fra_warp_paths(None) == -1
    counts = (C.c_uint64 * 2)(5, 5)
    assert L.fra_warp_paths(counts) == 0 and list(counts) == [0, 0]
    make = (ROOT / "flac-raster_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^UNITS = [^#]*\bfra_warp\b", make, re.M | re.S)
    assert re.search(r"^HOSTCHECK_UNITS = [^#]*fra_warp\.hip", make, re.M | re.S)


def _warp_job():
    src = np.zeros((1, 8, 8), np.int32)
    dst = np.zeros((1, 3, 5), np.int32)
    job = N.WarpJob()
    job.src, job.dtype, job.channels, job.height, job.width = C.c_void_p(src.ctypes.data), N.DTYPE_CODES[np.dtype(np.int32)], 1, 8, 8
    job.src_band_stride, job.src_row_stride, job.src_col_stride = 64, 8, 1
    job.out_height, job.out_width, job.resampling = 3, 5, N.RESAMPLE_BILINEAR
    job.dst = C.c_void_p(dst.ctypes.data)
    job.dst_band_stride, job.dst_row_stride, job.dst_col_stride = 15, 5, 1
    job.map.kind = N.WARP_AFFINE
    for k, v in enumerate(IDENTITY):
        job.map.affine[k] = v
    return job, (src, dst)


def test_every_refusal_arrives_before_any_gpu_work():
    L = N.load()
    ctx = C.c_void_p(16)  # never dereferenced on these paths
    job, keep = _warp_job()
    filled = (C.c_uint64 * 1)()

    def refused(j, word):
        return L.fra_warp(ctx, C.byref(j), filled) == -1 and word in L.fra_last_error()

    def variant(**kw):
        j, _ = _warp_job()
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    assert L.fra_warp(None, C.byref(job), filled) == -1 and b"null" in L.fra_last_error()
    assert L.fra_warp(ctx, None, filled) == -1 and b"null" in L.fra_last_error()
    assert refused(variant(src=None), b"null") and refused(variant(dst=None), b"null")
    assert refused(variant(dtype=8), b"bad dtype") and refused(variant(dtype=-1), b"bad dtype")
    assert refused(variant(width=0), b"bad raster layout") and refused(variant(src_row_stride=-1), b"bad raster layout")
    assert refused(variant(dst_col_stride=-1), b"bad raster layout") and refused(variant(channels=256), b"more than 255")
    for oh, ow in ((0, 5), (3, 0), (65537, 5), (3, 65537), (-1, 5)):
        assert refused(variant(out_height=oh, out_width=ow), b"output size"), (oh, ow)
    assert refused(variant(resampling=N.RESAMPLE_AVERAGE), b"point samples")
    assert refused(variant(resampling=4), b"unknown resampling") and refused(variant(resampling=-1), b"unknown resampling")
    assert refused(variant(flags=2), b"unknown warp flags")
    for kind in (-1, 2):
        j = variant()
        j.map.kind = kind
        assert refused(j, b"unknown map kind")
    for k in range(6):
        for bad in (math.nan, math.inf, -math.inf):
            j = variant()
            j.map.affine[k] = bad
            assert refused(j, b"is not finite"), (k, bad)
    plane = np.zeros((3, 4), np.float64)
    pd = plane.ctypes.data_as(C.POINTER(C.c_double))

    def grid(step, gh, gw, gx=pd, gy=pd):
        j = variant()
        j.map.kind, j.map.step, j.map.gh, j.map.gw, j.map.gx, j.map.gy = N.WARP_GRID, step, gh, gw, gx, gy
        return j

    assert refused(grid(0, 3, 4), b"grid step") and refused(grid(-2, 3, 4), b"grid step")
    assert refused(grid(2, 3, 5), b"takes a grid of 3 x 4 nodes") and refused(grid(2, 2, 4), b"takes a grid of 3 x 4 nodes")
    assert refused(grid(1, 3, 4), b"takes a grid of 4 x 6 nodes")
    assert refused(grid(2, 3, 4, gx=None), b"null grid") and refused(grid(2, 3, 4, gy=None), b"null grid")
    assert refused(variant(flags=N.WARP_NODATA, nodata=0.5), b"nodata 0.5 is not a value")
    assert refused(variant(flags=N.WARP_NODATA, nodata=math.nan), b"nodata")
    assert refused(variant(fill=0.5), b"fill 0.5 is not a value") and refused(variant(fill=2.0**31), b"fill")
    assert refused(variant(dtype=N.DTYPE_CODES[np.dtype(np.float32)], fill=0.1), b"fill")
    assert refused(variant(dtype=N.DTYPE_CODES[np.dtype(np.float32)], fill=math.inf), b"fill")
    # the order: the layout, the sizes, the map, the values
    assert refused(variant(dtype=8, out_height=0), b"bad dtype") and refused(variant(out_height=0, fill=0.5), b"output size")
    assert refused(variant(resampling=1, flags=2), b"point samples") and refused(grid(0, 3, 4, gx=None), b"grid step")
    # the read behind the decoder
    items = (N.DecodeItem * 1)()
    items[0].bytes, items[0].window = 64, N.Window(0, 0, 4, 8)
    data = np.zeros(64, np.uint8)
    out = np.zeros(64, np.int32)
    dj = N.DecodeJob()
    dj.data, dj.len, dj.items, dj.nitems = C.c_void_p(data.ctypes.data), 64, items, 1
    dj.dst, dj.dst_dtype, dj.channels = C.c_void_p(out.ctypes.data), N.DTYPE_CODES[np.dtype(np.int32)], 1
    dj.band_stride, dj.row_stride, dj.col_stride = 15, 5, 1
    infos = (N.Decoded * 1)()
    ident = N.warp_map(warp.affine_coefficients(IDENTITY))[0]

    def read(j=dj, c=ctx, H=4, W=8, m=ident, oh=3, ow=5, mode=2, flags=0, nd=0.0, fl=0.0, inf=infos):
        return L.fra_decode_device_warped(c, C.byref(j) if j is not None else None, H, W, C.byref(m) if m is not None else None,
                                          oh, ow, mode, flags, nd, fl, inf, filled)

    def says(rc, word):
        return rc == -1 and word in L.fra_last_error()

    assert says(read(c=None), b"null") and says(read(j=None), b"null") and says(read(m=None), b"null")
    assert says(read(inf=None), b"null")
    assert says(read(oh=0), b"output size") and says(read(mode=1), b"point samples") and says(read(flags=4), b"unknown warp flags")
    assert says(read(H=0), b"bad raster size") and says(read(W=-3), b"bad raster size")
    bad = N.warp_map(warp.affine_coefficients(IDENTITY))[0]
    bad.affine[2] = math.nan
    assert says(read(m=bad), b"is not finite")
    assert says(read(flags=1, nd=0.5), b"nodata") and says(read(fl=0.5), b"fill")
    assert says(read(H=9), b"do not cover")  # the identity over rows 0 .. 3 + 3 of a 9-row raster: the item has four
    wrong = N.DecodeJob.from_buffer_copy(dj)
    wrong.dst_dtype = 9
    assert says(read(j=wrong, fl=0.5), b"dtype")  # the windowed read's refusals come before the values'
    wrong = N.DecodeJob.from_buffer_copy(dj)
    wrong.flags = N.DECODE_CONCAT
    assert read(j=wrong) == -1
    del keep


def test_the_source_window_is_the_one_python_predicts():
    rng = np.random.default_rng(6)
    H, W = 300, 500
    cases = [(warp.affine_coefficients(IDENTITY), (300, 500)), (warp.affine_coefficients((1, 0, 600, 0, 1, 0)), (5, 5)),
             (warp.affine_coefficients((1, 0, -4.5, 0, 1, 0)), (5, 3)), (warp.affine_coefficients((1, 0, 0, 0, 1, 300.5)), (7, 7)),
             (_rotation(30.0, 0.7, 250, 150, 35, 150), (70, 300)), (_rotation(200.0, 1.9, 100, 100, 10, 10), (33, 67))]
    for _ in range(20):
        k = rng.normal(0, 1.5, 6) * (1, 1, 300, 1, 1, 300)
        cases.append((warp.affine_coefficients(k), (int(rng.integers(1, 90)), int(rng.integers(1, 90)))))
    g = warp.grid_map(lambda c, r: (c * 1.3 + 0.002 * r * r - 20.0, r * 0.8 + 0.001 * c * c + 40.0), (70, 300), 16)
    holes = warp.Map(warp.GRID, step=16, gx=g.gx.copy(), gy=g.gy.copy())
    holes.gx[1, 2] = np.nan
    holes.gy[0, 0] = np.inf
    nothing = warp.Map(warp.GRID, step=16, gx=np.full_like(g.gx, np.nan), gy=g.gy)
    cases += [(g, (70, 300)), (holes, (70, 300)), (nothing, (70, 300))]
    seen = set()
    for m, out_shape in cases:
        win = warp.source_window(m, (H, W), out_shape)
        assert N.warp_source_window(m, (H, W), out_shape) == win, (m.affine, out_shape)
        seen.add(win is None)
        if win is None:
            continue
        r0, c0, h, w = win
        assert 0 <= r0 and 0 <= c0 and h >= 1 and w >= 1 and r0 + h <= H and c0 + w <= W
        # every tap of every inside pixel lies in the window (the cubic's reach is the widest)
        x, y = warp.map_coords(m, out_shape)
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        if inside.any():
            cols = np.clip(np.floor(x[inside] - 0.5)[:, None] + np.arange(-1, 3), 0, W - 1)
            rows = np.clip(np.floor(y[inside] - 0.5)[:, None] + np.arange(-1, 3), 0, H - 1)
            assert cols.min() >= c0 and cols.max() < c0 + w and rows.min() >= r0 and rows.max() < r0 + h
    assert seen == {True, False}
    assert warp.source_window(warp.affine_coefficients(IDENTITY), (H, W), (H, W)) == (0, 0, H, W)
    assert warp.source_window(warp.affine_coefficients((1, 0, 100, 0, 1, 50)), (H, W), (10, 20)) == (47, 97, 16, 26)
    with pytest.raises(N.NativeError, match="output size"):
        N.warp_source_window(warp.affine_coefficients(IDENTITY), (H, W), (0, 5))


def test_a_window_of_the_source_gives_the_whole_rasters_result():
    rng = np.random.default_rng(8)
    a = _raster(np.float32, (2, 60, 90), rng)
    for m, out_shape in ((_rotation(30.0, 0.7, 45, 30, 20, 12), (24, 40)), (warp.affine_coefficients((1, 0, 80.5, 0, 1, -3.25)), (12, 30))):
        r0, c0, h, w = warp.source_window(m, (60, 90), out_shape)
        for mode in MODES:
            for nodata in (None, 7.0):
                want, wfilled = warp.warp_arrays(a, out_shape, m, mode, nodata)
                got, filled = warp.warp_arrays(a[:, r0:r0 + h, c0:c0 + w], out_shape, m, mode, nodata, origin=(r0, c0),
                                               raster_shape=(60, 90))
                _same(got, want, mode)
                assert filled.tolist() == wfilled.tolist()
    with pytest.raises(ValueError, match="does not hold"):
        warp.warp_arrays(a[:, 10:20, 10:20], (24, 40), _rotation(30.0, 0.7, 45, 30, 20, 12), origin=(10, 10), raster_shape=(60, 90))


# ------------------------------------------------------------------------------- crs.py
def test_utm_and_mercator_round_trips():
    lat, dlon = np.meshgrid(np.linspace(-80.0, 80.0, 41), np.linspace(-3.5, 3.5, 29))
    for zone, south in ((1, False), (33, False), (60, False), (18, True), (33, True)):
        lon = (6.0 * zone - 183.0) + dlon
        e, n = crs.utm_forward(lon, lat, zone, south)
        lon2, lat2 = crs.utm_inverse(e, n, zone, south)
        assert np.abs(lon2 - lon).max() <= 1e-11 and np.abs(lat2 - lat).max() <= 1e-11
        e2, n2 = crs.utm_forward(lon2, lat2, zone, south)
        assert np.abs(e2 - e).max() <= 1e-6 and np.abs(n2 - n).max() <= 1e-6
        f = crs.transformer("EPSG:4326", f"EPSG:{32700 + zone if south else 32600 + zone}")
        fe, fn = f(lon, lat)
        assert np.array_equal(fe, e) and np.array_equal(fn, n)
    lon, lat = np.meshgrid(np.linspace(-180.0, 180.0, 37), np.linspace(-85.0, 85.0, 35))
    x, y = crs.mercator_forward(lon, lat)
    lon2, lat2 = crs.mercator_inverse(x, y)
    assert np.abs(lon2 - lon).max() <= 1e-11 and np.abs(lat2 - lat).max() <= 1e-11
    x2, y2 = crs.mercator_forward(lon2, lat2)
    assert np.abs(x2 - x).max() <= 1e-6 and np.abs(y2 - y).max() <= 1e-6
    assert abs(x[0, -1] - math.pi * crs.A_WGS84) < 1e-6
    # through the composition: UTM -> 3857 -> UTM
    e, n = crs.utm_forward(15.0 + np.linspace(-3, 3, 13), np.linspace(-70, 70, 13), 33)
    mx, my = crs.transformer("EPSG:32633", "EPSG:3857")(e, n)
    e2, n2 = crs.transformer("EPSG:3857", "EPSG:32633")(mx, my)
    assert np.abs(e2 - e).max() <= 1e-6 and np.abs(n2 - n).max() <= 1e-6


def test_the_central_meridian():
    for zone in (1, 33, 60):
        lon0 = 6.0 * zone - 183.0
        for lat in (-75.0, -10.0, 0.0, 33.0, 80.0):
            assert crs.utm_forward(lon0, lat, zone, lat < 0)[0] == 500000.0
        assert tuple(float(v) for v in crs.utm_forward(lon0, 0.0, zone)) == (500000.0, 0.0)
        assert tuple(float(v) for v in crs.utm_forward(lon0, 0.0, zone, True)) == (500000.0, 10000000.0)


def test_the_northing_is_the_scaled_meridian_arc():
    e2 = crs.F_WGS84 * (2.0 - crs.F_WGS84)
    n = 100000  # composite Simpson
    for lat in (15.0, 45.0, 75.0):
        phi = np.linspace(0.0, math.radians(lat), n + 1)
        y = crs.A_WGS84 * (1.0 - e2) * (1.0 - e2 * np.sin(phi) ** 2) ** -1.5
        arc = (phi[1] - phi[0]) / 3.0 * (y[0] + y[-1] + 4.0 * y[1:-1:2].sum() + 2.0 * y[2:-1:2].sum())
        assert abs(float(crs.utm_forward(15.0, lat, 33)[1]) - 0.9996 * arc) <= 1e-4
        assert abs(float(crs.utm_forward(15.0, -lat, 33, True)[1]) - (10000000.0 - 0.9996 * arc)) <= 1e-4


def test_an_unknown_crs_is_refused():
    for bad in ("EPSG:2154", "EPSG:32661", "EPSG:32600", "+proj=lcc", None):
        with pytest.raises(ValueError, match=r"pass coords=.*pyproj.*--like / --transform"):
            crs.transformer(bad, "EPSG:4326")
        with pytest.raises(ValueError, match="pass coords="):
            crs.transformer("EPSG:3857", bad)
    x, y = crs.transformer("epsg:4326", "EPSG:4326")(3.0, 4.0)
    assert (float(x), float(y)) == (3.0, 4.0)


# ------------------------------------------------------------------------------- grids
def test_fit_grid_reaches_the_threshold():
    # a Sentinel-2 tile (10980 x 10980 at 10 m, UTM 33 N) onto its suggested Web Mercator grid
    st = Affine(10.0, 0.0, 399960.0, 0.0, -10.0, 4600020.0)
    dt, (oh, ow) = crs.suggested_grid(st, (10980, 10980), crs.transformer("EPSG:32633", "EPSG:3857"))
    assert abs(oh - 10980) < 400 and abs(ow - 10980) < 400 and dt.a == -dt.e and dt.b == 0.0
    back = crs.transformer("EPSG:3857", "EPSG:32633")

    def pixel(cols, rows):
        x, y = back(dt.a * cols + dt.c, dt.e * rows + dt.f)
        return (x - st.c) / st.a, (y - st.f) / st.e

    m, err = warp.fit_grid(pixel, (oh, ow))
    assert err <= 0.125 and m.step in (1, 2, 4, 8, 16) and m.gx.shape == warp.grid_shape((oh, ow), m.step)
    # the error it reports is the true maximum at the cell centres, through the rule's own interpolation
    gh, gw = m.gx.shape
    cc, rr = np.meshgrid((np.arange(gw - 1) + 0.5) * m.step, (np.arange(gh - 1) + 0.5) * m.step)
    tx, ty = pixel(cc, rr)
    def mid(g):
        top = g[:-1, :-1] + (g[:-1, 1:] - g[:-1, :-1]) * 0.5
        bot = g[1:, :-1] + (g[1:, 1:] - g[1:, :-1]) * 0.5
        return top + (bot - top) * 0.5

    assert err == float(np.hypot(mid(m.gx) - tx, mid(m.gy) - ty).max())
    if m.step < 16:  # the step above missed the threshold
        assert warp.centre_error(warp.grid_map(pixel, (oh, ow), 2 * m.step), pixel) > 0.125
    # an affine is reproduced by the coarsest grid
    k = (0.7, -0.4, 12.5, 0.4, 0.7, -3.25)
    m, err = warp.fit_grid(lambda c, r: (k[0] * c + k[1] * r + k[2], k[3] * c + k[4] * r + k[5]), (500, 700))
    assert m.step == 16 and err < 1e-9


def test_suggested_grid_of_the_identity_is_the_source_grid():
    for t, shape in (((10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0), (300, 500)), ((1.0, 0.0, 0.0, 0.0, -1.0, 0.0), (7, 19)),
                     ((0.25, 0.0, -3.0, 0.0, -0.25, 9.0), (1098, 1098))):
        got, gshape = crs.suggested_grid(t, shape, lambda x, y: (x, y))
        assert gshape == shape
        assert np.allclose(tuple(got)[:6], t, rtol=4 * np.finfo(np.float64).eps, atol=0.0)  # hypot / hypot: a few ulps


# ------------------------------------------------------------------------------- the command line
H, W, TILE = 40, 52, 32
TRANSFORM = (10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)


def _scene():
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([1000 + 60 * np.sin(yy / 5.0) + 40 * np.cos(xx / 7.0) + rng.integers(0, 5, (H, W)),
                  500 + 3 * yy + 2 * xx + rng.integers(0, 9, (H, W))]).astype(np.uint16)
    a[0, 10:12, 20:23] = 0
    return a


def test_cli_writes_the_rule(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli
    from flac_raster.streaming import assemble_streaming, read_window, warp_window
    from flac_raster.tiff import read_geotiff, write_geotiff
    from flac_raster.tiles import calculate_tiles
    from oracle_tiles import oracle_encode_tiles

    a = _scene()
    tif = tmp_path / "scene.tif"
    write_geotiff(tif, a, transform=TRANSFORM, crs="EPSG:32633")
    flac = tmp_path / "scene_streaming.flac"
    tiles = calculate_tiles(H, W, TILE)
    data = assemble_streaming(tiles, oracle_encode_tiles(a, tiles, level=5), a.shape, a.dtype, Affine(*TRANSFORM), "EPSG:32633", TILE)
    flac.write_bytes(data)
    decoded = read_window(data, window=(0, 0, H, W), device=None)[0]
    monkeypatch.setattr(cli, "_gpu_present", lambda: False)
    app, run = cli.app, CliRunner()
    out = tmp_path / "out.tif"
    # --like: another raster's grid, rotated and finer, in the same CRS
    like_t = (4.0, 3.0, 500050.0, 3.0, -4.0, 4099900.0)
    like = tmp_path / "like.tif"
    write_geotiff(like, np.zeros((1, 30, 45), np.uint8), transform=like_t, crs="EPSG:32633")
    m = warp.affine_map(like_t, TRANSFORM)
    for src, ref in ((tif, a), (flac, decoded)):
        res = run.invoke(app, ["warp", str(src), "-o", str(out), "--like", str(like), "--resampling", "cubic", "--nodata", "0", "--cpu"])
        assert res.exit_code == 0 and "source window" in res.output and "filled" in res.output, res.output
        got, info = read_geotiff(out)
        want, filled = warp.warp_arrays(ref, (30, 45), m, "cubic", 0.0)
        _same(got, want, f"--like, {src.name}")
        assert tuple(info.transform)[:6] == like_t and str(info.crs) == "EPSG:32633" and info.nodata == 0
        # --transform: a shifted, coarser grid partly outside
        res = run.invoke(app, ["warp", str(src), "-o", str(out), "--transform", "20,0,499900,0,-20,4100100", "--out-shape", "12,20",
                               "--resampling", "nearest", "--fill", "9", "--cpu"])
        assert res.exit_code == 0, res.output
        got, info = read_geotiff(out)
        m2 = warp.affine_map((20.0, 0.0, 499900.0, 0.0, -20.0, 4100100.0), TRANSFORM)
        want, filled = warp.warp_arrays(ref, (12, 20), m2, "nearest", None, 9)
        _same(got, want, f"--transform, {src.name}")
        assert filled[0] > 0 and tuple(info.transform)[:6] == (20.0, 0.0, 499900.0, 0.0, -20.0, 4100100.0)
        # --dst-crs: Web Mercator through a fitted grid
        res = run.invoke(app, ["warp", str(src), "-o", str(out), "--dst-crs", "EPSG:3857", "--cpu"])
        assert res.exit_code == 0 and "coordinate grid: step" in res.output, res.output
        got, info = read_geotiff(out)
        dt, dshape = crs.suggested_grid(TRANSFORM, (H, W), crs.transformer("EPSG:32633", "EPSG:3857"))
        assert got.shape == (2,) + dshape and str(info.crs) == "EPSG:3857"
        assert np.allclose(tuple(info.transform)[:6], tuple(dt)[:6], rtol=1e-15)
        if src == flac:
            wout, wt, wcrs, winfo = warp_window(data, tuple(dt)[:6], dshape, "EPSG:3857", cpu=True)
            _same(got, wout, "--dst-crs against warp_window")
            assert wcrs == "EPSG:3857" and winfo["grid_error"] <= 0.125 and winfo["source_window"] == (0, 0, H, W)
            # the pixels the grid puts well inside the source hold the source's values range
            assert got[1].max() <= decoded[1].max() and (got[1][got[1] > 0].min() >= decoded[1].min())
    # exactly one of the three; their companions
    for args in ([], ["--like", str(like), "--dst-crs", "EPSG:3857"], ["--transform", "1,0,0,0,1,0"], ["--out-shape", "3,3", "--like", str(like)],
                 ["--like", str(like), "--res", "5"], ["--dst-crs", "EPSG:3857", "--res", "5", "--size", "4,4"],
                 ["--dst-crs", "EPSG:2154"], ["--like", str(like), "--resampling", "average"]):
        res = run.invoke(app, ["warp", str(tif), "-o", str(out), "--cpu"] + args)
        assert res.exit_code == 1 and "Error" in res.output, (args, res.output)
    res = run.invoke(app, ["warp", str(tif), "-o", str(out), "--dst-crs", "EPSG:4326", "--size", "20,30", "--cpu"])
    assert res.exit_code == 0 and read_geotiff(out)[0].shape == (2, 20, 30), res.output
    # a grid wholly outside: all fill, no source window
    wout, _, _, winfo = warp_window(data, (10.0, 0.0, 900000.0, 0.0, -10.0, 4100000.0), (5, 6), fill=3, cpu=True)
    assert (wout == 3).all() and winfo["source_window"] is None and winfo["shares"] == [1.0, 1.0]


def test_hostcheck_covers_the_warp_refusals():
    """make hostcheck: the argument validation of the warp entries and the source-window arithmetic in the stand-alone
    program under AddressSanitizer + UBSan; no GPU."""
    csrc = ROOT / "flac-raster_amd" / "csrc"
    if not shutil.which("make") or not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("no make / hipcc")
    text = (ROOT / "tools" / "decode_host_check.cpp").read_text()
    for name in ("fra_warp(", "fra_decode_device_warped", "fra_warp_source_window", "fra_warp_timing", "fra_warp_paths"):
        assert name in text, name
    subprocess.run(["make", "-C", str(csrc), "hostcheck"], check=True, capture_output=True)
    run = subprocess.run([str(csrc / "build" / "decode_host_check"), str(ROOT / "tests" / "golden" / "sample_rgb.flac")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "argument validation checked" in run.stdout and "host check ok" in run.stdout, \
        run.stdout[-4000:] + run.stderr[-4000:]
