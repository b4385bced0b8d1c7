"""GPU tests of the warped reads (``k_warp`` alone through ``fra_warp``, and behind the windowed read through
``fra_decode_device_warped`` and ``streaming.warp_window``).

The expectation is never the kernel: it is ``warp.warp_arrays`` -- the rule in numpy, checked on the CPU against a
per-pixel loop -- applied to the raster itself or to the full host decode.  The comparison is bit for bit for every
dtype: the coordinates and the values are IEEE f64 operations in a fixed order, so there is no tolerance to choose.
The shapes are the smallest at which each of these can go wrong (the tile is 16 x 64 output pixels): a footprint larger
than the raster ((1, 1), (7, 19) sources), a ragged tile and a one-workgroup grid ((5, 3), (33, 67) outputs), several
tiles with ragged tails and a grid cell spanning tiles ((70, 300) outputs, step 16), a tile whose footprint is the whole
source (the shrink of (130, 517) to (4, 13)) and footprints around 16 KiB (scales around 1.9 for 4-byte elements).
"""
import functools
import math

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import resample, warp
from flac_raster.geo import Affine

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
MODES = ("nearest", "bilinear", "cubic")
PAIRS = [((1, 1), (5, 3)), ((7, 19), (1, 1)), ((7, 19), (33, 67)), ((33, 67), (5, 3)), ((33, 67), (70, 300)),
         ((130, 517), (33, 67)), ((130, 517), (70, 300))]
B = 3
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _ctx():
    return N.default_context(0)


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


def _padded(a, pad_cols, fill=77):
    """``a`` (B, h, w) as a view of a larger array: ``pad_cols`` spare columns per row and one spare row per band."""
    nb, h, w = a.shape
    big = np.full((nb, h + 1, w + pad_cols), fill, a.dtype)
    big[:, :h, :w] = a
    return big, big[:, :h, :w]


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

    def bent(c, r):
        return c * (w / ow) + 0.0004 * r * r - 0.7, r * (h / oh) + 0.0003 * c * c - 0.4

    return {
        "identity": warp.affine_coefficients(IDENTITY),
        "shift partly outside": warp.affine_coefficients((1.0, 0.0, -2.3, 0.0, 1.0, 1.7)),
        "wholly outside": warp.affine_coefficients((1.0, 0.0, w + 50.0, 0.0, 1.0, 0.0)),
        "rotation 30 x 0.7": _rotation(30.0, 0.7, w / 2.0, h / 2.0, ow / 2.0, oh / 2.0),
        "rotation 200 x 1.9": _rotation(200.0, 1.9, w / 2.0, h / 2.0, ow / 2.0, oh / 2.0),
        "grid step 4": warp.grid_map(bent, out_shape, 4),
        "grid step 16": warp.grid_map(bent, out_shape, 16),
        "grid step 3": warp.grid_map(bent, out_shape, 3),  # not a power of two: the kernel divides
    }


def _check(ctx, a, out_shape, m, mode, nodata, fill, what):
    want, wfilled = warp.warp_arrays(a, out_shape, m, mode, nodata, fill)
    got, filled = ctx.warp(a, out_shape, m, mode, nodata=nodata, fill=fill)
    _same(got, want, what)
    assert filled.tolist() == wfilled.tolist(), (what, filled, wfilled)
    return got, filled


# ------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_dtype(dt):
    rng = np.random.default_rng(500 + np.dtype(dt).num)
    ctx = _ctx()
    a = _raster(dt, (B, 33, 67), rng)
    m = _rotation(30.0, 0.7, 33.5, 16.5, 33.5, 16.5)
    for mode in MODES:
        for nodata, fill in ((None, None), (7.0, None), (7.0, 3.0), (None, 5.0)):
            _check(ctx, a, (33, 67), m, mode, nodata, fill, f"{mode} nodata {nodata} fill {fill}")
    assert ctx.warp_timing() >= 0.0 and ctx.warp_paths() == (0, 3 * 2 * B)  # 3 x 2 tiles per band, all gathered


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_maps_and_shapes(dt):
    rng = np.random.default_rng(600 + np.dtype(dt).num)
    ctx = _ctx()
    for shape, out_shape in PAIRS:
        a = _raster(dt, (B,) + shape, rng)
        for name, m in _maps(shape, out_shape).items():
            for mode in MODES:
                for nodata in (None, 7.0):
                    got, filled = _check(ctx, a, out_shape, m, mode, nodata, None, f"{name} {mode} nodata {nodata} {shape} -> {out_shape}")
                    if name == "wholly outside":
                        assert filled.tolist() == [out_shape[0] * out_shape[1]] * B
                    if name == "identity" and mode == "nearest" and shape == (130, 517) and out_shape == (70, 300):
                        _same(got, np.ascontiguousarray(a[:, :70, :300]), "the identity is a copy")


def test_footprints_of_every_size_and_the_workgroup_count():
    """The identity's small footprints, a shrink whose one tile reads the whole source, and footprints around 16 KiB (the
    size at which a staged path, measured slower and not built, would have given way to the gather): every workgroup is
    counted as gathered, none as staged."""
    rng = np.random.default_rng(7)
    ctx = _ctx()
    a = _raster(np.uint16, (B, 130, 517), rng)
    for mode in MODES:
        _check(ctx, a, (130, 517), warp.affine_coefficients(IDENTITY), mode, None, None, f"identity {mode}")
        assert ctx.warp_paths() == (0, 9 * 9 * B), mode
    d = _raster(np.float64, (B, 130, 517), rng)
    shrink = warp.affine_coefficients((517 / 13.0, 0.0, 0.0, 0.0, 130 / 4.0, 0.0))
    for mode in MODES:
        for nodata in (None, 7.0):
            _check(ctx, d, (4, 13), shrink, mode, nodata, None, f"shrink {mode} {nodata}")
            assert ctx.warp_paths() == (0, B), mode  # one tile: 130 x 517 x 8 bytes
    f = _raster(np.float32, (B, 130, 517), rng)
    for scale in (1.6, 1.8, 2.0, 2.2):
        m = _rotation(3.0, scale, 258.0, 65.0, 150.0, 35.0)
        for mode in MODES:
            _check(ctx, f, (70, 300), m, mode, 7.0, None, f"scale {scale} {mode}")
            assert ctx.warp_paths() == (0, 5 * 5 * B)


@pytest.mark.parametrize("dt", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_power_of_two_scales_equal_the_resampling_on_the_device(dt):
    rng = np.random.default_rng(8 + np.dtype(dt).num)
    ctx = _ctx()
    for shape, scale in (((33, 67), 0.5), ((33, 67), 0.25), ((32, 68), 2.0), ((32, 68), 4.0)):
        a = _raster(dt, (B,) + shape, rng)
        out_shape = (int(shape[0] / scale), int(shape[1] / scale))
        m = warp.affine_coefficients((scale, 0.0, 0.0, 0.0, scale, 0.0))
        for mode in MODES:
            got, _ = ctx.warp(a, out_shape, m, mode)
            _same_but_nan_signs(got, ctx.resample(a, out_shape, mode), f"{shape} x {scale} {mode}: fra_resample")
            _same_but_nan_signs(got, resample.resample(a, out_shape, mode), f"{shape} x {scale} {mode}: the rule")
            got, _ = ctx.warp(a, out_shape, m, mode, nodata=7.0)
            _same_but_nan_signs(got, ctx.resample(a, out_shape, mode, nodata=7.0), f"{shape} x {scale} {mode}: fra_resample_masked")


# ------------------------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("dt", [np.uint16, np.float64, np.uint8], ids=lambda d: np.dtype(d).name)
def test_layouts(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(70 + dt.num)
    ctx = _ctx()
    h, w = 33, 67
    oh, ow = 33, 67
    a = _raster(dt, (B, h, w), rng)
    V = 16 // dt.itemsize
    for m, mode, nodata in ((_rotation(30.0, 0.7, 33.5, 16.5, 33.5, 16.5), "cubic", 7.0),
                            (warp.affine_coefficients((1.0, 0.0, -2.3, 0.0, 1.0, 1.7)), "bilinear", None),
                            (warp.grid_map(lambda c, r: (c * 0.9 + 0.001 * r * r, r * 1.1 - 0.5), (oh, ow), 16), "nearest", 7.0)):
        want, wfilled = warp.warp_arrays(a, (oh, ow), m, mode, nodata)
        abig16, av16 = _padded(a, -w % V + V)   # rows 16-byte aligned: vector loads
        abig5, av5 = _padded(a, 5)              # rows not 16-byte aligned: element loads
        wide = np.full((B, h, 2 * w), 77, dt)
        wide[:, :, ::2] = a
        keep = abig16.tobytes(), abig5.tobytes(), wide.tobytes()
        for view in (av16, av5, wide[:, :, ::2]):
            got, filled = ctx.warp(view, (oh, ow), m, mode, nodata=nodata)
            _same(got, want, f"{mode} source view {view.strides}")
            assert filled.tolist() == wfilled.tolist()
        assert (abig16.tobytes(), abig5.tobytes(), wide.tobytes()) == keep  # nothing is written to the source
        # host destinations: the caller's values between the outputs stay
        for pad in (-ow % V + V, 5):
            obig = np.full((B, oh + 1, ow + pad), 77, dt)
            ctx.warp(a, (oh, ow), m, mode, dst=obig[:, :oh, :ow], nodata=nodata)
            _same(obig[:, :oh, :ow], want, f"{mode} padded destination {pad}")
            assert (obig[:, oh] == 77).all() and (obig[:, :, ow:] == 77).all()
        owide = np.full((B, oh, 2 * ow), 77, dt)
        ctx.warp(av5, (oh, ow), m, mode, dst=owide[:, :, ::2], nodata=nodata)
        _same(owide[:, :, ::2], want, f"{mode} column stride 2")
        assert (owide[:, :, 1::2] == 77).all()
        # device source and destination
        rs, ors = w + (-w % V), ow + (-ow % V) + V
        sa = np.full((B, h, rs), 77, dt)
        sa[:, :, :w] = a
        so = np.full((B, oh, ors), 77, dt)
        d_a, d_o = ctx.alloc(sa.nbytes), ctx.alloc(so.nbytes)
        try:
            ctx.h2d(d_a, sa)
            ctx.h2d(d_o, so)
            _, filled = ctx.warp(d_a, (oh, ow), m, mode, dst=d_o, nodata=nodata, dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1),
                                 dst_strides=(oh * ors, ors, 1))
            back = np.empty_like(so)
            ctx.d2h(back, d_o)
            _same(np.ascontiguousarray(back[:, :, :ow]), want, f"{mode} device to device")
            assert (back[:, :, ow:] == 77).all() and filled.tolist() == wfilled.tolist()
            got, _ = ctx.warp(d_a, (oh, ow), m, mode, nodata=nodata, dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1))
            _same(got, want, f"{mode} device to host")
            src_back = np.empty_like(sa)
            ctx.d2h(src_back, d_a)
            assert src_back.tobytes() == sa.tobytes()
        finally:
            ctx.free(d_a)
            ctx.free(d_o)


def test_refusals_leave_everything_untouched_and_the_context_goes_on():
    ctx = _ctx()
    a = np.arange(3 * 7 * 19, dtype=np.uint16).reshape(3, 7, 19)
    ident = warp.affine_coefficients(IDENTITY)
    ctx.warp(a, (7, 19), ident)
    before, paths = ctx.warp_timing(), ctx.warp_paths()
    dst = np.full((3, 7, 19), 5, np.uint16)
    g = warp.grid_map(lambda c, r: (c, r), (7, 19), 4)
    bad_grid = warp.Map(warp.GRID, step=4, gx=g.gx[:, :-1].copy(), gy=g.gy[:, :-1].copy())
    nan_map = warp.Map(warp.AFFINE, (1.0, 0.0, math.nan, 0.0, 1.0, 0.0))
    for msg, m in (("takes a grid of", bad_grid), ("is not finite", nan_map), ("unknown map kind", warp.Map(5))):
        with pytest.raises(N.NativeError, match=msg) as e:
            ctx.warp(a, (7, 19), m, dst=dst)
        assert "error -1" in str(e.value)
    with pytest.raises(ValueError, match="point samples"):
        ctx.warp(a, (7, 19), ident, "average", dst=dst)
    with pytest.raises(ValueError, match="fill"):
        ctx.warp(a, (7, 19), ident, dst=dst, fill=0.5)
    d = ctx.alloc(16)
    try:
        with pytest.raises(N.NativeError, match="bad raster layout"):
            ctx.warp(a, (7, 19), ident, dst=d, dst_strides=(0, -1, 1))
    finally:
        ctx.free(d)
    assert (dst == 5).all() and ctx.warp_timing() == before and ctx.warp_paths() == paths
    got, _ = ctx.warp(a, (7, 19), ident, "nearest")
    _same(got, a, "after the refusals")


# ------------------------------------------------------------------------------- 3. behind the decoder
H, W, TILE = 300, 500, 128  # 3 x 4 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 399960.0, 0.0, -10.0, 4600020.0)
CRS = "EPSG:32633"


@functools.lru_cache(maxsize=None)
def _container():
    from flac_raster.streaming import build_streaming, read_window

    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    src = np.stack([(3000 + 2000 * np.sin(yy / 17.0 + b) + 800 * np.cos(xx / 23.0) + rng.integers(0, 40, (H, W)))
                    for b in range(B)]).astype(np.uint16)
    data = build_streaming(src, TRANSFORM, CRS, TILE)
    host = read_window(data, window=(0, 0, H, W), device=None)[0]  # what the container holds: the source of the rule
    host.setflags(write=False)
    return data, host


def test_the_warped_read_equals_the_rule_over_the_full_decode():
    from flac_raster.streaming import _tile_items, warp_window

    data, host = _container()
    ctx = _ctx()
    nd = float(host[1, 150, 250])
    # a rotation whose footprint crosses tile borders and the raster's edge
    rot = _rotation(25.0, 0.8, 440.0, 250.0, 100.0, 60.0)
    dst_t = tuple(Affine(*tuple(TRANSFORM)[:6]) * Affine(*rot.affine))[:6]  # source transform o map
    for mode in MODES:
        for nodata in (None, nd):
            want, wfilled = warp.warp_arrays(host, (120, 200), rot, mode, nodata)
            got, t, crs_, info = warp_window(data, dst_t, (120, 200), resampling=mode, nodata=nodata, device=0)
            m = info["map"]
            want2, _ = warp.warp_arrays(host, (120, 200), m, mode, nodata)  # the composed coefficients, rounded
            _same(got, want2, f"rotation {mode} nodata {nodata}")
            assert info["filled"].tolist() == warp.warp_arrays(host, (120, 200), m, mode, nodata)[1].tolist()
            assert (info["filled"] > 0).all() and crs_ == CRS
            win = warp.source_window(m, (H, W), (120, 200))
            assert info["source_window"] == win == N.warp_source_window(m, (H, W), (120, 200))
            assert win[0] + win[2] == H and win[1] + win[3] == W and win[0] > 0 and win[1] > TILE  # the edge; not every tile
            cpu, _, _, cinfo = warp_window(data, dst_t, (120, 200), resampling=mode, nodata=nodata, cpu=True)
            _same(cpu, got, f"rotation {mode} nodata {nodata}: host path")
            assert cinfo["filled"].tolist() == info["filled"].tolist()
    # the entry itself, with the exact map, every item handed over, into a strided host destination
    _, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    big = np.full((B, 121, 210), 77, np.uint16)
    infos, filled = ctx.decode_device_warped(blob, items, big, np.uint16, B, (121 * 210, 210, 1), (H, W), (120, 200), rot, "cubic",
                                             denorm=N.DENORM_PCM16, nodata=nd)
    want, wfilled = warp.warp_arrays(host, (120, 200), rot, "cubic", nd)
    _same(np.ascontiguousarray(big[:, :120, :200]), want, "the entry, strided destination")
    assert (big[:, 120] == 77).all() and (big[:, :, 200:] == 77).all() and filled.tolist() == wfilled.tolist()
    decoded = [k for k, i in enumerate(infos) if i.nframes > 0]
    win = warp.source_window(rot, (H, W), (120, 200))
    hit = [k for k, it in enumerate(items) if it["window"][0] < win[0] + win[2] and it["window"][0] + it["window"][2] > win[0]
           and it["window"][1] < win[1] + win[3] and it["window"][1] + it["window"][3] > win[1]]
    assert decoded == hit and 0 < len(hit) < len(items)
    assert len(ctx.decode_timing()) == 4 and ctx.warp_timing() >= 0.0
    # a shift wholly outside: nothing is decoded
    out = np.zeros((B, 9, 11), np.uint16)
    infos, filled = ctx.decode_device_warped(blob, items, out, np.uint16, B, (99, 11, 1), (H, W), (9, 11),
                                             warp.affine_coefficients((1.0, 0.0, 0.0, 0.0, 1.0, H + 20.0)), "bilinear",
                                             denorm=N.DENORM_PCM16, fill=9)
    assert (out == 9).all() and filled.tolist() == [99] * B and all(i.nframes == 0 for i in infos)
    got, _, _, info = warp_window(data, (10.0, 0.0, 900000.0, 0.0, -10.0, 4600020.0), (9, 11), fill=4, device=0)
    assert (got == 4).all() and info["source_window"] is None and info["shares"] == [1.0] * B
    # the items must cover the source window
    with pytest.raises(N.NativeError, match="do not cover"):
        ctx.decode_device_warped(blob, [it for k, it in enumerate(items) if k != hit[-1]], big, np.uint16, B, (121 * 210, 210, 1),
                                 (H, W), (120, 200), rot, denorm=N.DENORM_PCM16)
    got, _ = ctx.warp(np.asarray(host), (9, 11), warp.affine_coefficients(IDENTITY), "nearest")  # the context goes on
    _same(got, np.ascontiguousarray(host[:, :9, :11]), "after the refusal")


def test_utm_to_web_mercator_through_a_fitted_grid():
    from flac_raster import crs
    from flac_raster.streaming import warp_window

    data, host = _container()
    dst_t, (oh, ow) = crs.suggested_grid(TRANSFORM, (H, W), crs.transformer(CRS, "EPSG:3857"))
    for mode, nodata in (("bilinear", None), ("cubic", float(host[0, 10, 10])), ("nearest", None)):
        got, t, crs_, info = warp_window(data, dst_t, (oh, ow), "EPSG:3857", resampling=mode, nodata=nodata, device=0)
        m = info["map"]
        assert m.kind == warp.GRID and info["grid_error"] <= 0.125 and crs_ == "EPSG:3857" and t == tuple(dst_t)[:6]
        want, wfilled = warp.warp_arrays(host, (oh, ow), m, mode, nodata)
        _same(got, want, f"mercator {mode}")
        assert info["filled"].tolist() == wfilled.tolist() and 0 < info["shares"][0] < 0.2  # the tilted tile's corners
        assert info["source_window"] == warp.source_window(m, (H, W), (oh, ow)) == (0, 0, H, W)
        cpu, _, _, cinfo = warp_window(data, dst_t, (oh, ow), "EPSG:3857", resampling=mode, nodata=nodata, cpu=True)
        _same(cpu, got, f"mercator {mode}: host path")


def test_warp_cli_on_the_device(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.tiff import read_geotiff, write_geotiff

    data, host = _container()
    flac = tmp_path / "scene_streaming.flac"
    flac.write_bytes(data)
    dev, cpu = tmp_path / "dev.tif", tmp_path / "cpu.tif"
    res = CliRunner().invoke(app, ["warp", str(flac), "-o", str(dev), "--dst-crs", "EPSG:3857", "--device", "0"])
    assert res.exit_code == 0 and "GPU 0" in res.output and "coordinate grid" in res.output, res.output
    res = CliRunner().invoke(app, ["warp", str(flac), "-o", str(cpu), "--dst-crs", "EPSG:3857", "--cpu"])
    assert res.exit_code == 0 and "host" in res.output, res.output
    assert dev.read_bytes() == cpu.read_bytes()
    tif, like = tmp_path / "a.tif", tmp_path / "c.tif"
    write_geotiff(tif, np.asarray(host), transform=tuple(TRANSFORM)[:6], crs=CRS)
    write_geotiff(like, np.zeros((1, 80, 90), np.uint8), transform=(23.0, 7.0, 400500.0, 7.0, -23.0, 4599500.0), crs=CRS)
    res = CliRunner().invoke(app, ["warp", str(tif), "-o", str(dev), "--like", str(like), "--resampling", "cubic", "--device", "0"])
    assert res.exit_code == 0 and "GPU 0" in res.output, res.output
    res = CliRunner().invoke(app, ["warp", str(tif), "-o", str(cpu), "--like", str(like), "--resampling", "cubic", "--cpu"])
    assert res.exit_code == 0, res.output
    assert dev.read_bytes() == cpu.read_bytes()
    got, info = read_geotiff(dev)
    m = warp.affine_map((23.0, 7.0, 400500.0, 7.0, -23.0, 4599500.0), tuple(TRANSFORM)[:6])
    _same(got, warp.warp_arrays(np.asarray(host), (80, 90), m, "cubic")[0], "cli, --like")
    assert tuple(info.transform)[:6] == (23.0, 7.0, 400500.0, 7.0, -23.0, 4599500.0)
