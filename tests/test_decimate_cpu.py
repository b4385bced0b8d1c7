"""CPU tests of the decimated reads (no GPU needed).

* the new C ABI names are declared, exported and bound; ``fra_decimate`` and ``fra_decode_device_decimated`` refuse a
  null argument, a factor outside 2 .. 64, an unknown resampling code and items that do not cover the region before
  any GPU work.
* ``resample.decimate`` is the rule: ``nearest`` against the index formula, integer ``average`` against exact
  ``fractions.Fraction`` arithmetic rounded half to even, float ``average`` against ``np.mean`` within the worst-case
  bound of k^2 same-sign additions, and its summation order (the pair tree, not left to right).
* host ``read_window(decimate=k)`` / ``read_overview`` equal ``decimate`` of the full-resolution read; the ``window
  --decimate`` and ``overview`` CLI commands on the host path.
"""
import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import resample
from flac_raster.geo import Affine
from flac_raster.resample import decimate, decimated_shape, decimated_transform
from flac_raster.streaming import assemble_streaming, read_overview, read_window, streaming_to_raster
from flac_raster.tiff import read_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TILE = 300, 420, 128  # the container of test_window_cpu: 3 x 4 tiles, ragged right and bottom

# (row_off, col_off, height, width) as asked -> the same clipped to the raster (test_window_cpu's table)
WINDOWS = {
    "inside one tile": ((10, 140, 50, 60), (10, 140, 50, 60)),
    "four-tile corner": ((100, 230, 60, 50), (100, 230, 60, 50)),
    "single pixel": ((299, 419, 1, 1), (299, 419, 1, 1)),
    "full row band": ((120, 0, 20, 420), (120, 0, 20, 420)),
    "whole raster": ((0, 0, 300, 420), (0, 0, 300, 420)),
    "over the edge": ((250, 380, 100, 100), (250, 380, 50, 40)),
}
NEW = ("fra_decimate", "fra_decode_device_decimated", "fra_decimate_timing")


@pytest.fixture(scope="module")
def container():
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (1000 + 60 * np.sin(yy / 23.0) + 40 * np.cos(xx / 31.0)).astype(np.int64)
    r = np.stack([base + b * 7 + rng.integers(0, 50, size=(H, W)) for b in range(3)]).astype(np.uint16)
    tiles = calculate_tiles(H, W, TILE)
    streams = oracle_encode_tiles(r, tiles, level=5)
    data = assemble_streaming(tiles, streams, r.shape, r.dtype, TRANSFORM, "EPSG:32633", TILE)
    full = {sem: streaming_to_raster(data, device=None, semantics=sem)[0] for sem in ("pcm16", "int")}
    for a in full.values():
        a.setflags(write=False)
    return data, full


# ------------------------------------------------------------------------------- 1. names and refusals
def test_new_names_exported_declared_and_bound():
    hdr = (ROOT / "include" / "flac_raster_amd.h").read_text()
    decl = set(re.findall(r"FRA_API\s+[^;(]*?\b(fra_\w+)\s*\(", hdr))
    L = N.load()
    for name in NEW:
        assert name in decl and name in N.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+FRA_RESAMPLE_NEAREST\s+0\b", hdr) and re.search(r"#define\s+FRA_RESAMPLE_AVERAGE\s+1\b", hdr)
    assert "fra_decimate_job" in hdr and (N.RESAMPLE_NEAREST, N.RESAMPLE_AVERAGE) == (0, 1)
    assert resample.RESAMPLING == {"nearest": 0, "average": 1} and resample.FACTORS == (2, 4, 8, 16, 32, 64)
    assert hasattr(N.Context, "decimate") and hasattr(N.Context, "decode_device_decimated")
    assert L.fra_abi_version() == 3
    from flac_raster import streaming, tiles
    import inspect

    for fn in (streaming.read_window, streaming.window_to_tiff, tiles.read_window_on_device):
        p = inspect.signature(fn).parameters
        assert p["decimate"].default == 1 and p["resampling"].default == "nearest", fn
    assert inspect.signature(streaming.read_overview).parameters["resampling"].default == "average"


def _decode_job():
    data = (C.c_uint8 * 64)()
    dst = (C.c_int32 * 64)()
    item = N.DecodeItem()
    item.offset, item.bytes, item.window = 0, 64, N.Window(0, 0, 4, 8)
    job = N.DecodeJob()
    job.data, job.len, job.items, job.nitems = C.cast(data, C.c_void_p), 64, C.pointer(item), 1
    job.dst, job.dst_dtype, job.channels = C.cast(dst, C.c_void_p), N.DTYPE_CODES[np.dtype(np.int32)], 1
    job.band_stride, job.row_stride, job.col_stride = 8, 4, 1
    return job, item, (data, dst)


def test_decimated_decode_refuses_before_any_gpu_work():
    """Every call returns FRA_E_INVALID before the context is looked at, so a stand-in pointer serves."""
    L = N.load()
    ctx = C.c_void_p(16)
    job, item, _keep = _decode_job()
    infos = (N.Decoded * 1)()
    roi = N.Window(0, 0, 4, 8)

    def call(ctx=ctx, job=job, roi=roi, k=2, mode=1, infos=infos):
        return L.fra_decode_device_decimated(ctx, C.byref(job) if job is not None else None,
                                             C.byref(roi) if roi is not None else None, k, mode, infos)

    for kw in ({"ctx": None}, {"job": None}, {"roi": None}, {"infos": None}):
        assert call(**kw) == -1 and b"null" in L.fra_last_error(), kw
    for k in (0, 1, 3, 128, -2, 6):
        assert call(k=k) == -1 and b"factor" in L.fra_last_error() and str(k).encode() in L.fra_last_error()
    assert call(mode=2) == -1 and b"resampling" in L.fra_last_error()
    assert call(mode=-1) == -1 and b"resampling" in L.fra_last_error()
    # the item covers rows 0..3 of columns 0..7; a region one row taller has an uncovered strip
    assert call(roi=N.Window(0, 0, 5, 8)) == -1 and b"do not cover the region" in L.fra_last_error()
    item.window = N.Window(0, 0, 4, 7)  # an uncovered column
    assert call() == -1 and b"do not cover the region" in L.fra_last_error()
    job.nitems = 0
    assert call() == -1 and b"do not cover the region" in L.fra_last_error()
    job.nitems = 1
    item.window = N.Window(0, 0, 4, 8)
    # what the windowed read refuses is refused in its words
    assert call(roi=N.Window(0, 0, 0, 8)) == -1 and b"region of interest" in L.fra_last_error()
    job.flags = N.DECODE_CONCAT
    assert call() == -1 and b"CONCAT" in L.fra_last_error()


def test_decimate_entry_refuses_before_any_gpu_work():
    L = N.load()
    ctx = C.c_void_p(16)
    src = (C.c_int32 * 64)()
    dst = (C.c_int32 * 64)()
    job = N.DecimateJob()
    job.src, job.dst, job.dtype = C.cast(src, C.c_void_p), C.cast(dst, C.c_void_p), N.DTYPE_CODES[np.dtype(np.int32)]
    job.channels, job.height, job.width = 1, 8, 8
    job.src_band_stride, job.src_row_stride, job.src_col_stride = 64, 8, 1
    job.dst_band_stride, job.dst_row_stride, job.dst_col_stride = 16, 4, 1
    job.factor, job.resampling = 2, 0
    assert L.fra_decimate(None, C.byref(job)) == -1 and b"null" in L.fra_last_error()
    assert L.fra_decimate(ctx, None) == -1 and b"null" in L.fra_last_error()
    job.src = None
    assert L.fra_decimate(ctx, C.byref(job)) == -1 and b"null" in L.fra_last_error()
    job.src = C.cast(src, C.c_void_p)
    job.dst = None
    assert L.fra_decimate(ctx, C.byref(job)) == -1 and b"null" in L.fra_last_error()
    job.dst = C.cast(dst, C.c_void_p)
    for k in (0, 1, 3, 128):
        job.factor = k
        assert L.fra_decimate(ctx, C.byref(job)) == -1 and b"factor" in L.fra_last_error()
    job.factor, job.resampling = 2, 2
    assert L.fra_decimate(ctx, C.byref(job)) == -1 and b"resampling" in L.fra_last_error()
    job.resampling, job.dtype = 1, 8
    assert L.fra_decimate(ctx, C.byref(job)) == -1 and b"dtype" in L.fra_last_error()
    job.dtype, job.width = 5, 0
    assert L.fra_decimate(ctx, C.byref(job)) == -1 and b"layout" in L.fra_last_error()
    assert L.fra_decimate_timing(None) == -1
    with pytest.raises(ValueError):
        resample.check_factor(3)
    with pytest.raises(ValueError):
        resample.resampling_code("cubic")


# ------------------------------------------------------------------------------- 2. the numpy rule
SHAPES = lambda k: [(1, 1), (k - 1, k + 1), (2 * k + 1, 3 * k - 1), (5, max(1, k // 2))]  # noqa: E731  (the last: w < k)


def test_shape_and_transform():
    assert decimated_shape(300, 420, 8) == (38, 53) and decimated_shape(1, 1, 64) == (1, 1)
    assert decimated_shape(16, 17, 4) == (4, 5)
    t = (10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
    assert decimated_transform(t, (100, 230, 60, 50), 4) == (40.0, 0.0, 502300.0, 0.0, -40.0, 4099000.0)
    r = (2.0, 0.5, 7.0, -0.25, -3.0, 11.0)  # rotation terms scale and shift too
    assert decimated_transform(r, (3, 5), 2) == (4.0, 1.0, 7.0 + 5 * 2.0 + 3 * 0.5, -0.5, -6.0, 11.0 + 5 * -0.25 + 3 * -3.0)


@pytest.mark.parametrize("k", [2, 8, 64])
def test_nearest_is_the_index_formula(k):
    rng = np.random.default_rng(k)
    for h, w in SHAPES(k):
        a = rng.integers(-30000, 30000, size=(2, h, w)).astype(np.int16)
        got = decimate(a, k, "nearest")
        oh, ow = decimated_shape(h, w, k)
        assert got.shape == (2, oh, ow) and got.dtype == a.dtype
        for R in range(oh):
            for Cc in range(ow):
                assert np.array_equal(got[:, R, Cc], a[:, min(R * k + k // 2, h - 1), min(Cc * k + k // 2, w - 1)])
    assert np.array_equal(decimate(a[0], k, "nearest"), got[0])  # the (h, w) form


def _exact_average(a, k):
    """Block means by exact rational arithmetic, rounded half to even."""
    h, w = a.shape
    oh, ow = decimated_shape(h, w, k)
    out = np.zeros((oh, ow), a.dtype)
    for R in range(oh):
        for Cc in range(ow):
            blk = a[R * k:R * k + k, Cc * k:Cc * k + k]
            out[R, Cc] = round(Fraction(int(blk.astype(object).sum()), blk.size))  # round(): half to even
    return out


@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.int16, np.uint32, np.int32], ids=lambda d: np.dtype(d).name)
def test_integer_average_is_exact_and_rounds_half_to_even(dt):
    dt = np.dtype(dt)
    # ties: block sums of n/2 mod n, both towards an even and an odd neighbour
    ties = np.array([[1, 2, 3, 4, 0, 1], [1, 2, 4, 3, 1, 0], [5, 5, 7, 7, 2, 3]], dt)  # blocks 1.5, 3.5, 0.5; edge row
    assert np.array_equal(decimate(ties, 2, "average"), np.array([[2, 4, 0], [5, 7, 2]], dt))
    assert np.array_equal(decimate(ties, 2, "average"), _exact_average(ties, 2))
    rng = np.random.default_rng(dt.itemsize)
    info = np.iinfo(dt)
    for k in (2, 4, 16):
        for h, w in SHAPES(k):
            a = rng.integers(info.min, int(info.max) + 1, size=(h, w), dtype=np.int64).astype(dt)
            a[0, 0], a[-1, -1] = info.max, info.min
            assert np.array_equal(decimate(a, k, "average"), _exact_average(a, k)), (k, h, w)
    full = np.full((64, 64), info.max, dt)  # the largest sum: 4096 * max
    assert decimate(full, 64, "average")[0, 0] == info.max


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_average_is_within_the_bound_of_k2_additions(dt):
    rng = np.random.default_rng(9)
    for k in (2, 8, 64):
        for h, w in SHAPES(k):
            a = rng.uniform(0.5, 1000.0, size=(h, w)).astype(dt)
            got = decimate(a, k, "average")
            oh, ow = decimated_shape(h, w, k)
            assert got.shape == (oh, ow) and got.dtype == dt
            for R in range(oh):
                for Cc in range(ow):
                    want = np.mean(a[R * k:R * k + k, Cc * k:Cc * k + k].astype(np.float64))
                    tol = k * k * 2.0 ** -53 * want
                    if dt == np.float32:  # the result is then rounded to f32 once, and rounding is monotonic
                        assert np.float32(want - tol) <= got[R, Cc] <= np.float32(want + tol), (k, h, w, R, Cc)
                    else:
                        assert abs(got[R, Cc] - want) <= tol, (k, h, w, R, Cc)


def test_float_average_follows_the_pair_tree_and_plain_ieee():
    row = np.array([[1e16, 1.0, -1e16, 1.0]])
    assert ((1e16 + 1.0) + -1e16) + 1.0 == 1.0  # left to right
    assert (1e16 + 1.0) + (-1e16 + 1.0) == 0.0  # the tree
    assert decimate(row, 4, "average")[0, 0] == 0.0
    # rows are accumulated top to bottom: (1e16 + 1) + -1e16 = 0, not 1e16 + (1 + -1e16)
    col = np.array([[1e16, 0.0], [1.0, 0.0], [-1e16, 0.0], [1.0, 0.0]])
    assert decimate(col, 4, "average")[0, 0] == 1.0 / 8.0
    # an edge block is padded with +0.0 in its rows, and rows it does not have are not added: -0.0 stays -0.0 only
    # where nothing was added to it
    z = np.full((1, 2), -0.0)
    assert np.signbit(decimate(z, 2, "average")[0, 0])  # (-0.0 + -0.0) / 2, one row
    assert not np.signbit(decimate(z[:, :1], 2, "average")[0, 0])  # -0.0 + (+0.0 pad)
    assert np.signbit(decimate(np.full((3, 2), -0.0), 2, "average")[1, 0])  # the missing row is not added
    a = np.ones((2, 4), np.float32)
    a[0, 1], a[1, 2] = np.nan, np.inf
    got = decimate(a, 2, "average")
    assert np.isnan(got[0, 0]) and got[0, 1] == np.inf
    a[0, 3] = -np.inf
    assert np.isnan(decimate(a, 2, "average")[0, 1])
    big = np.full((2, 2), np.finfo(np.float32).max, np.float32)  # the f64 sum does not overflow
    assert decimate(big, 2, "average")[0, 0] == np.finfo(np.float32).max
    with pytest.raises(TypeError):
        decimate(np.zeros((2, 2), np.int64), 2)
    with pytest.raises(ValueError):
        decimate(np.zeros((2, 2), np.int16), 2, "cubic")
    with pytest.raises(ValueError):
        decimate(np.zeros((2, 2), np.int16), 3)


# ------------------------------------------------------------------------------- 3. the container on the host
@pytest.mark.parametrize("mode", ["nearest", "average"])
@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("name", list(WINDOWS))
def test_host_read_window_decimated_equals_decimate_of_the_window(container, name, k, mode):
    data, full = container
    asked, (r, c, h, w) = WINDOWS[name]
    got, win, index = read_window(data, window=asked, device=None, decimate=k, resampling=mode)
    plain, win1, _ = read_window(data, window=asked, device=None)
    assert tuple(win) == tuple(win1) == (r, c, h, w) and index["height"] == H
    assert got.dtype == np.uint16 and got.shape == (3,) + decimated_shape(h, w, k)
    assert np.array_equal(got, decimate(plain, k, mode))
    assert np.array_equal(got, decimate(full["pcm16"][:, r:r + h, c:c + w], k, mode))


def test_host_read_overview_and_bad_arguments(container):
    data, full = container
    for sem in ("pcm16", "int"):
        got, index = read_overview(data, 4, device=None, semantics=sem)  # average by default
        assert index["width"] == W and np.array_equal(got, decimate(full[sem], 4, "average"))
    got, _ = read_overview(data, 16, "nearest")
    assert np.array_equal(got, decimate(full["pcm16"], 16, "nearest"))
    with pytest.raises(ValueError):
        read_window(data, window=(0, 0, 8, 8), decimate=3)
    with pytest.raises(ValueError):
        read_window(data, window=(0, 0, 8, 8), decimate=2, resampling="cubic")
    with pytest.raises(ValueError):
        read_overview(data, 1)


def test_cli_on_the_host(container, tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli

    data, full = container
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    monkeypatch.setattr(cli, "_gpu_present", lambda: False)  # the host path, wherever this runs
    out = tmp_path / "win.tif"
    res = CliRunner().invoke(cli.app, ["window", str(src), "-o", str(out), "--window", "100,230,60,50", "--decimate", "4"])
    assert res.exit_code == 0, res.output
    px, info = read_geotiff(out)
    assert px.shape == (3, 15, 13) and np.array_equal(px, decimate(full["pcm16"][:, 100:160, 230:280], 4, "nearest"))
    assert tuple(info.transform)[:6] == (40.0, 0.0, 500000.0 + 230 * 10.0, 0.0, -40.0, 4100000.0 - 100 * 10.0)
    assert "32633" in str(info.crs)
    out2 = tmp_path / "win_avg.tif"
    res = CliRunner().invoke(cli.app, ["window", str(src), "-o", str(out2), "--bbox",
                                       "501403.5,4099400.1,501999.0,4099899.0", "--decimate", "4", "--resampling",
                                       "average"])
    assert res.exit_code == 0, res.output
    px2, info2 = read_geotiff(out2)
    assert np.array_equal(px2, decimate(full["pcm16"][:, 10:60, 140:200], 4, "average"))
    assert tuple(info2.transform)[:6] == (40.0, 0.0, 501400.0, 0.0, -40.0, 4099900.0)
    out3 = tmp_path / "preview.tif"
    res = CliRunner().invoke(cli.app, ["overview", str(src), "-o", str(out3), "--factor", "4"])
    assert res.exit_code == 0, res.output
    px3, info3 = read_geotiff(out3)
    assert px3.shape == (3, 75, 105) and np.array_equal(px3, decimate(full["pcm16"], 4, "average"))
    assert tuple(info3.transform)[:6] == (40.0, 0.0, 500000.0, 0.0, -40.0, 4100000.0) and "32633" in str(info3.crs)
    res = CliRunner().invoke(cli.app, ["overview", str(src), "-o", str(tmp_path / "n.tif"), "--factor", "8",
                                       "--resampling", "nearest"])
    assert res.exit_code == 0, res.output
    assert np.array_equal(read_geotiff(tmp_path / "n.tif")[0], decimate(full["pcm16"], 8, "nearest"))
    # a region is still required, and a bad factor is an error
    assert CliRunner().invoke(cli.app, ["window", str(src), "-o", str(tmp_path / "x.tif"), "--decimate", "4"]).exit_code == 1
    assert CliRunner().invoke(cli.app, ["window", str(src), "-o", str(tmp_path / "x.tif"), "--window", "0,0,8,8",
                                        "--decimate", "3"]).exit_code == 1
    assert CliRunner().invoke(cli.app, ["overview", str(src), "-o", str(tmp_path / "x.tif"), "--factor", "5"]).exit_code == 1
