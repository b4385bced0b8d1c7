"""GPU tests of the resampled reads (``k_resample`` alone through ``fra_resample``, and behind the windowed read through
``fra_decode_device_resampled``).

Every comparison is bit-exact (floats: the same NaN positions and the same bits elsewhere, so a lost ``-0.0`` shows).
The expectation is never the kernel: it is ``resample.resample`` -- the rule in numpy, checked on the CPU against a
per-pixel loop in exact coordinates -- applied to the source raster or to the host ``read_window``.  The shape pairs are
the smallest at which the mapping can go wrong: a single pixel, up and down by coprime sizes, negative first taps, the
identity, long vertical spans, more than one workgroup along a row, output columns whose source span exceeds a wave's
columns and, for the widest elements, a workgroup's.
"""
import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.resample import resample, resampled_transform
from flac_raster.tiff import read_geotiff

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
MODES = ("nearest", "average", "bilinear", "cubic")
PAIRS = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((5, 7), (3, 4)), ((5, 7), (11, 13)), ((9, 6), (9, 6)),
         ((13, 17), (2, 1)), ((2, 3), (7, 1)), ((300, 5), (2, 3)), ((3, 4100), (2, 1025)), ((3, 4100), (2, 37))]


def _ctx():
    return N.default_context(0)


def _same(got, want):
    """Bit-exact equality; NaNs need only be NaNs at the same places."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(np.ascontiguousarray(got).view(u)[~gn],
                                                     np.ascontiguousarray(want).view(u)[~wn])


def _sentinel(dt):
    return np.dtype(dt).type(77)


def _raster(dt, shape, rng):
    """Full-range integers; floats with cancelling magnitudes (a wrong summation order shows) and, where there is
    room, a NaN, both infinities and negative zeros (a skipped or reordered special shows)."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        a = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
        a.flat[0] = info.max
        return a
    pick = rng.integers(0, 6, size=shape)
    a = np.choose(pick, [np.full(shape, 1e16), np.full(shape, -1e16), np.ones(shape), rng.normal(0.0, 3.0, size=shape),
                         np.full(shape, -0.0), rng.uniform(0.0, 1e-3, size=shape)]).astype(dt)
    if a.size >= 30:
        for v in (np.nan, np.inf, -np.inf, np.inf):  # (two +inf: inf + inf stays inf, inf + -inf is NaN)
            a.flat[int(rng.integers(0, a.size))] = v
    return a


def _padded(a, pad_cols, fill):
    """``a`` (B, h, w) as a view of a larger array: ``pad_cols`` spare columns per row and one spare row per band."""
    B, h, w = a.shape
    big = np.full((B, h + 1, w + pad_cols), fill, a.dtype)
    big[:, :h, :w] = a
    return big, big[:, :h, :w]


def _check_padding(big, h, w, fill):
    assert _same(big[:, h, :], np.full_like(big[:, h, :], fill)) and _same(big[:, :, w:], np.full_like(big[:, :, w:], fill))


# ------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_alone_equals_the_numpy_rule(dt, mode):
    dt = np.dtype(dt)
    rng = np.random.default_rng(200 + dt.num)
    ctx = _ctx()
    fill = _sentinel(dt)
    V = 16 // dt.itemsize
    specials = False
    for (h, w), (oh, ow) in PAIRS:
        a = _raster(dt, (3, h, w), rng)
        specials |= dt.kind == "f" and bool(np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
                                            and (np.signbit(a) & (a == 0)).any() and (np.abs(a) == dt.type(1e16)).any())
        want = resample(a, (oh, ow), mode)
        assert want.shape == (3, oh, ow)
        # host source, rows not 16-byte aligned (element loads) and aligned (16-byte loads), padded destination
        for pad in (5, -w % V + V):
            sbig, src = _padded(a, pad, fill)
            dbig, dst = _padded(np.full((3, oh, ow), fill, dt), 2, fill)
            assert ctx.resample(src, (oh, ow), mode, dst) is dst
            assert _same(dst, want), (h, w, oh, ow, pad)
            _check_padding(dbig, oh, ow, fill)
            _check_padding(sbig, h, w, fill)
            assert _same(sbig[:, :h, :w], a)
        assert _same(ctx.resample(a, (oh, ow), mode), want), (h, w, oh, ow)  # contiguous, a new array comes back
        assert ctx.resample_timing() >= 0.0
        # pixel-interleaved source
        inter = np.ascontiguousarray(a.transpose(1, 2, 0))  # (h, w, 3)
        assert _same(ctx.resample(inter.transpose(2, 0, 1), (oh, ow), mode), want), (h, w, oh, ow, "interleaved")
        # device-resident source (aligned rows) and destination (padded)
        rs = w + (-w % V)
        staged = np.full((3, h, rs), fill, dt)
        staged[:, :, :w] = a
        d_src, d_dst = ctx.alloc(staged.nbytes), ctx.alloc(3 * (oh + 1) * (ow + 2) * dt.itemsize)
        try:
            ctx.h2d(d_src, staged)
            dbig = np.full((3, oh + 1, ow + 2), fill, dt)
            ctx.h2d(d_dst, dbig)
            ctx.resample(d_src, (oh, ow), mode, d_dst, dtype=dt, shape=(3, h, w), strides=(h * rs, rs, 1),
                         dst_strides=((oh + 1) * (ow + 2), ow + 2, 1))
            ctx.d2h(dbig, d_dst)
        finally:
            ctx.free(d_src)
            ctx.free(d_dst)
        assert _same(dbig[:, :oh, :ow], want), (h, w, oh, ow, "device")
        _check_padding(dbig, oh, ow, fill)
    assert specials or dt.kind != "f"  # the float data held a NaN, both infinities, -0.0 and cancelling magnitudes


def test_kernel_order_clamp_and_wide_spans():
    """The order-visible and cubic clamp cases of the CPU tests on the device, and an output column whose source span
    is wider than a workgroup's columns (the chunked walk)."""
    ctx = _ctx()
    rng = np.random.default_rng(8)
    col = np.array([[[1e16], [1.0], [-1e16], [1.0]]])
    assert ctx.resample(col, (1, 1), "average")[0, 0, 0] == 0.25  # top to bottom; a pairwise tree gives 0.0
    assert ctx.resample(np.ascontiguousarray(col.transpose(0, 2, 1)), (1, 1), "average")[0, 0, 0] == 0.25
    sq = np.array([[[1e16, 1.0], [-1e16, 1.0]]])
    assert ctx.resample(sq, (1, 1), "average")[0, 0, 0] == 0.5  # vertically first
    z = np.full((1, 2, 2), -0.0, np.float32)
    assert np.signbit(ctx.resample(z, (1, 1), "average")[0, 0, 0])
    ties = np.array([[[1, 2, 3, 4, 0, 1], [1, 2, 4, 3, 1, 0]]], np.int16)  # 1.5, 3.5, 0.5: half to even
    assert np.array_equal(ctx.resample(ties, (1, 3), "average"), [[[2, 4, 0]]])
    step = np.array([[[0, 0, 255, 255, 0, 0]]], np.uint8)
    exact = resample(step.astype(np.float64), (1, 24), "cubic")
    assert exact.max() > 255.0 and exact.min() < 0.0  # the exact values leave the range
    got = ctx.resample(step, (1, 24), "cubic")
    assert _same(got, resample(step, (1, 24), "cubic")) and got.max() == 255 and got.min() == 0
    assert _same(ctx.resample(step.astype(np.float64), (1, 24), "cubic"), exact)
    # 32771 > 2^15 rows into one: the column sums of uint16 no longer fit 32 bits (the other accumulators), 32768 do
    for h in (32771, 32768):
        tall = np.full((1, h, 3), 65535, np.uint16)
        tall[0, ::7, 1] = rng.integers(0, 65536, size=len(tall[0, ::7, 1]))
        assert _same(ctx.resample(tall, (1, 2), "average"), resample(tall, (1, 2), "average")), h
    # f64: a workgroup holds 512 columns, f32 1024; one output column of 1500 spans three and two chunks
    for dt in (np.float64, np.float32, np.int32):
        wide = _raster(dt, (2, 3, 1500), rng)
        if np.dtype(dt).kind == "f":
            wide[np.isnan(wide) | np.isinf(wide)] = 1.0  # (one special would be all there is to see in one output)
        for out_shape in ((2, 1), (1, 2)):
            assert _same(ctx.resample(wide, out_shape, "average"), resample(wide, out_shape, "average")), (dt, out_shape)


# ------------------------------------------------------------------------------- 2. behind the decoder
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TILE = 80, 90, 48  # 2 x 2 tiles of 48 pixels, ragged right and bottom
WINDOWS = [(0, 0, H, W), (30, 41, 37, 29)]  # the whole raster, and a window off the tile grid over all four tiles
OUT_SHAPES = [(37, 53), (200, 150)]


@pytest.fixture(scope="module", params=[np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def container(request):
    from flac_raster.streaming import build_streaming, read_window

    dt = np.dtype(request.param)
    rng = np.random.default_rng(12 + dt.itemsize)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(20000 + 9000 * np.sin(yy / 11.0 + b) + 8000 * np.cos(xx / 13.0) + rng.integers(0, 400, (H, W)))
                  for b in range(3)])
    r = (r / 7.0).astype(dt) if dt.kind == "f" else r.astype(dt)
    data = build_streaming(r, TRANSFORM, "EPSG:32633", TILE)
    host = {w: read_window(data, window=w, device=None)[0] for w in WINDOWS}  # the expectation's input, read once
    for a in host.values():
        a.setflags(write=False)
    return data, dt, host


@pytest.mark.parametrize("mode", MODES)
def test_container_reads_equal_the_rule_of_the_host_read(container, mode):
    from flac_raster.streaming import read_overview, read_window

    data, dt, host = container
    for wdw in WINDOWS:
        for out_shape in OUT_SHAPES:
            want = resample(host[wdw], out_shape, mode)
            dev, dw, idx = read_window(data, window=wdw, device=0, out_shape=out_shape, resampling=mode)
            assert dw == wdw and len(idx["frames"]) == 4 and dev.dtype == dt
            assert _same(dev, want), (wdw, out_shape)
            got, hw, _ = read_window(data, window=wdw, device=None, out_shape=out_shape, resampling=mode)
            assert hw == wdw and _same(got, want), (wdw, out_shape, "host")
    assert _same(read_overview(data, out_shape=(37, 53), resampling=mode, device=0)[0], resample(host[WINDOWS[0]], (37, 53), mode))
    assert _ctx().resample_timing() >= 0.0 and len(_ctx().decode_timing()) == 4


def test_container_refusals_and_max_size(container):
    from flac_raster.streaming import _window_items, read_overview, read_window

    data, dt, host = container
    with pytest.raises(ValueError, match="not both"):
        read_window(data, window=WINDOWS[1], device=0, decimate=2, out_shape=(8, 8))
    got, _ = read_overview(data, max_size=45, device=0)  # the longest side becomes 45, average by default
    assert got.shape == (3, 40, 45) and _same(got, resample(host[WINDOWS[0]], (40, 45), "average"))
    # items that do not cover the region: the cover message, and the destination is left alone
    index, win, blob, items = _window_items(data, WINDOWS[1], None)
    assert len(items) == 4
    dst = np.full((3, 8, 8), 77, dt)
    ctx = _ctx()
    for mode in MODES:
        with pytest.raises(N.NativeError, match="do not cover the region"):
            ctx.decode_device_resampled(np.frombuffer(blob, dtype=np.uint8), items[:3], dst, dt, 3, (64, 8, 1), win,
                                        (8, 8), mode, N.DENORM_PCM16)
    assert _same(dst, np.full((3, 8, 8), 77, dt))
    # a padded destination: only the outputs are written
    big = np.full((3, 9, 10), 77, dt)
    ctx.decode_device_resampled(np.frombuffer(blob, dtype=np.uint8), items, big, dt, 3, (90, 10, 1), win, (8, 8),
                                "bilinear", N.DENORM_PCM16)
    assert _same(big[:, :8, :8], resample(host[WINDOWS[1]], (8, 8), "bilinear"))
    _check_padding(big, 8, 8, dt.type(77))


def test_plan_output_resampled_on_device():
    """``tiles.read_window_on_device(out_shape=)``: device to device through the plan's frame offsets, equal to the
    rule of the full-resolution read of the same window."""
    from flac_raster.tiles import read_window_on_device

    rng = np.random.default_rng(11)
    B, Hh, Ww = 2, 60, 130
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    r = np.stack([(3000 + 900 * np.sin(yy / 17.0 + b) + 700 * np.cos(xx / 29.0) + rng.integers(0, 60, (Hh, Ww)))
                  for b in range(B)]).astype(np.uint16)
    tiles = [(0, 0, 60, 64), (0, 64, 60, 66)]
    ctx = _ctx()
    plan = N.Plan(ctx, r.ctypes.data, False, r.dtype, B, (Hh * Ww, Ww, 1), tiles, 5, 4096, 16, keepalive=r)
    wdw = (7, 30, 41, 77)
    dev = ctx.alloc(B * 41 * 77 * 2)
    try:
        plan.execute()
        plan.sync()
        read_window_on_device(plan, wdw, dev)
        full = np.empty((B, 41, 77), np.int16)
        ctx.d2h(full, dev)
        for mode in MODES:
            read_window_on_device(plan, wdw, dev, out_shape=(19, 50), resampling=mode)
            got = np.empty((B, 19, 50), np.int16)
            ctx.d2h(got, dev)
            assert np.array_equal(got, resample(full, (19, 50), mode)), mode
        with pytest.raises(ValueError, match="not both"):
            read_window_on_device(plan, wdw, dev, decimate=2, out_shape=(19, 50))
    finally:
        ctx.free(dev)
        plan.close()


# ------------------------------------------------------------------------------- 3. CLI
def test_cli_writes_the_rule_and_its_transform(container, tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app

    data, dt, host = container
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    out = tmp_path / "win.tif"
    res = CliRunner().invoke(app, ["window", str(src), "-o", str(out), "--window", "30,41,37,29", "--device", "0",
                                   "--out-shape", "20,58", "--resampling", "cubic"])
    assert res.exit_code == 0, res.output
    px, info = read_geotiff(out)
    assert _same(px, resample(host[WINDOWS[1]], (20, 58), "cubic")) and "32633" in str(info.crs)
    assert tuple(info.transform)[:6] == resampled_transform(tuple(TRANSFORM)[:6], WINDOWS[1], (20, 58))
    assert tuple(info.transform)[:6] == (5.0, 0.0, 500410.0, 0.0, -18.5, 4099700.0)
    out2 = tmp_path / "preview.tif"
    res = CliRunner().invoke(app, ["overview", str(src), "-o", str(out2), "--size", "45", "--device", "0"])
    assert res.exit_code == 0, res.output
    px2, info2 = read_geotiff(out2)
    assert _same(px2, resample(host[WINDOWS[0]], (40, 45), "average"))  # average by default
    assert tuple(info2.transform)[:6] == (20.0, 0.0, 500000.0, 0.0, -20.0, 4100000.0)
