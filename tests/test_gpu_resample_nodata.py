"""GPU tests of the nodata-aware reads (``k_resample_masked`` alone through ``fra_resample_masked`` and
``fra_decimate_masked``, and behind the windowed read through the two ``fra_decode_device_*_masked`` entries).

Every comparison is bit-exact (floats: the same NaN positions and the same bits elsewhere).  The expectation is never
the kernel: it is ``resample.resample(..., nodata=)`` / ``resample.decimate(..., nodata=)`` -- the rule in numpy, checked
on the CPU against a per-pixel loop -- applied to the source raster or to the host ``read_window``.  The shape pairs
are those of ``test_gpu_resample.py``.

Two kinds of input: full-range data (integers over the whole dtype, floats with cancelling magnitudes, NaN, both
infinities and negative zeros) with about 30 % of the pixels invalid, in every layout; and bounded data (100 .. 200, the
nodata value far below, so that neither an average of valid pixels nor a cubic overshoot can land on it) under every
mask, where the kernel's per-band count of fill outputs must equal ``out == fill`` counted by numpy.
"""
import ctypes as C

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.resample import FACTORS, decimate, decimated_shape, resample
from flac_raster.tiff import read_geotiff

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
IDS = [np.dtype(d).name for d in DTYPES]
MODES = ("average", "bilinear", "cubic")
PAIRS = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((5, 7), (3, 4)), ((5, 7), (11, 13)), ((9, 6), (9, 6)),
         ((13, 17), (2, 1)), ((2, 3), (7, 1)), ((300, 5), (2, 3)), ((3, 4100), (2, 1025)), ((3, 4100), (2, 37))]
MASKS = ("random", "row", "column", "all", "none")


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


def _fill(dt, nd):
    dt = np.dtype(dt)
    return dt.type(nd) if dt.kind == "f" else dt.type(int(nd))


def _nodata_of(dt):
    dt = np.dtype(dt)
    return -9999.0 if dt.kind == "f" else float({1: 7, 2: 1000, 4: 100000}[dt.itemsize])


def _full_range(dt, shape, rng, nd):
    """Full-range integers; floats with cancelling magnitudes and, where there is room, a NaN, both infinities and
    negative zeros among the valid pixels; about 30 % of the pixels are ``nd``."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        a = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
        a.flat[0] = info.max
    else:
        pick = rng.integers(0, 6, size=shape)
        a = np.choose(pick, [np.full(shape, 1e16), np.full(shape, -1e16), np.ones(shape), rng.normal(0.0, 3.0, size=shape),
                             np.full(shape, -0.0), rng.uniform(0.0, 1e-3, size=shape)]).astype(dt)
    a[rng.random(shape) < 0.3] = _fill(dt, nd)
    if dt.kind == "f" and a.size >= 30:
        for v in (np.nan, np.inf, -np.inf, np.inf):
            a.flat[int(rng.integers(0, a.size))] = v
    return a


def _bounded(dt, shape, rng, nd, mask):
    """Values in 100 .. 200 (int8: 20 .. 100) and ``nd`` where ``mask`` says so."""
    dt = np.dtype(dt)
    lo, hi = (20, 100) if dt == np.int8 else (100, 200)
    a = rng.uniform(lo, hi, size=shape).astype(dt) if dt.kind == "f" else rng.integers(lo, hi + 1, size=shape).astype(dt)
    fill = _fill(dt, nd)
    if mask == "random":
        a[rng.random(shape) < 0.3] = fill
    elif mask == "row":
        a[:, shape[1] // 2, :] = fill
    elif mask == "column":
        a[:, :, shape[2] // 2] = fill
    elif mask == "all":
        a[...] = fill
    return a


def _count_fill(out, nd):
    return (np.isnan(out) if nd != nd else out == _fill(out.dtype, nd)).reshape(out.shape[0], -1).sum(axis=1).astype(np.uint64)


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
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_kernel_alone_equals_the_numpy_rule(dt, mode):
    dt = np.dtype(dt)
    rng = np.random.default_rng(900 + dt.num)
    ctx = _ctx()
    sent = dt.type(77)
    V = 16 // dt.itemsize
    nd = _nodata_of(dt)
    specials = False
    for (h, w), (oh, ow) in PAIRS:
        a = _full_range(dt, (3, h, w), rng, nd)
        specials |= dt.kind == "f" and bool(np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
                                            and (np.signbit(a) & (a == 0)).any())
        want = resample(a, (oh, ow), mode, nodata=nd)
        # host source, rows not 16-byte aligned (element loads) and aligned (16-byte loads), padded destination
        for pad in (5, -w % V + V):
            sbig, src = _padded(a, pad, sent)
            dbig, dst = _padded(np.full((3, oh, ow), sent, dt), 2, sent)
            assert ctx.resample(src, (oh, ow), mode, dst, nodata=nd) is dst
            assert _same(dst, want), (h, w, oh, ow, pad)
            _check_padding(dbig, oh, ow, sent)
            _check_padding(sbig, h, w, sent)
            assert _same(sbig[:, :h, :w], a)
        assert _same(ctx.resample(a, (oh, ow), mode, nodata=nd), want), (h, w, oh, ow)  # contiguous
        assert ctx.resample_masked_timing() >= 0.0
        inter = np.ascontiguousarray(a.transpose(1, 2, 0))  # pixel-interleaved source
        assert _same(ctx.resample(inter.transpose(2, 0, 1), (oh, ow), mode, nodata=nd), want), (h, w, oh, ow, "interleaved")
        # device-resident source (aligned rows) and destination (padded)
        rs = w + (-w % V)
        staged = np.full((3, h, rs), sent, dt)
        staged[:, :, :w] = a
        d_src, d_dst = ctx.alloc(staged.nbytes), ctx.alloc(3 * (oh + 1) * (ow + 2) * dt.itemsize)
        try:
            ctx.h2d(d_src, staged)
            dbig = np.full((3, oh + 1, ow + 2), sent, dt)
            ctx.h2d(d_dst, dbig)
            ctx.resample(d_src, (oh, ow), mode, d_dst, dtype=dt, shape=(3, h, w), strides=(h * rs, rs, 1),
                         dst_strides=((oh + 1) * (ow + 2), ow + 2, 1), nodata=nd)
            ctx.d2h(dbig, d_dst)
        finally:
            ctx.free(d_src)
            ctx.free(d_dst)
        assert _same(dbig[:, :oh, :ow], want), (h, w, oh, ow, "device")
        _check_padding(dbig, oh, ow, sent)
        # bounded data under every mask: the rule, and the count of fill outputs
        for nd_b in {"i": (-100.0,), "u": (0.0,), "f": (-9999.0, np.nan)}[dt.kind]:
            for mask in MASKS:
                b = _bounded(dt, (3, h, w), rng, nd_b, mask)
                want_b = resample(b, (oh, ow), mode, nodata=nd_b)
                filled = np.full(3, 99, np.uint64)
                got = ctx.resample(b, (oh, ow), mode, nodata=nd_b, filled=filled)
                assert _same(got, want_b), (h, w, oh, ow, mask, nd_b)
                assert np.array_equal(filled, _count_fill(got, nd_b)), (h, w, oh, ow, mask, nd_b, filled)
                if mask == "all":
                    assert filled.tolist() == [oh * ow] * 3
                if mask == "none":  # no invalid pixel: the unmasked kernel's bits
                    assert _same(got, ctx.resample(b, (oh, ow), mode)) and not filled.any()
    assert specials or dt.kind != "f"  # the float data held a NaN, both infinities and -0.0 among the valid pixels


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_kernel_nearest_no_invalid_and_wide_spans(dt):
    """``nearest`` with a nodata value is the unmasked result; full-range data without an invalid pixel gives the
    unmasked kernel's bits in every mode (``-0.0`` included); an output column whose source span is wider than a
    workgroup's columns carries both sums over the chunks."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(950 + dt.num)
    ctx = _ctx()
    nd = _nodata_of(dt)
    a = _full_range(dt, (2, 13, 17), rng, nd)
    assert _same(ctx.resample(a, (5, 4), "nearest", nodata=nd), resample(a, (5, 4), "nearest"))
    clean = a.copy()
    clean[(clean == _fill(dt, nd)) | (np.isnan(clean) if dt.kind == "f" else False)] = dt.type(-0.0 if dt.kind == "f" else 3)
    for mode in ("nearest",) + MODES:
        for out_shape in ((5, 4), (20, 31)):
            filled = np.full(2, 99, np.uint64)
            got = ctx.resample(clean, out_shape, mode, nodata=nd, filled=filled)
            assert _same(got, ctx.resample(clean, out_shape, mode)) and not filled.any(), (mode, out_shape)
    # 1500 columns into one or two: f64 walks three chunks of 512 columns, f32 two of 1024
    wide = _full_range(dt, (2, 3, 1500), rng, nd)
    if dt.kind == "f":
        wide[np.isnan(wide) | np.isinf(wide)] = 1.0  # (one special would be all there is to see in one output)
    wide[:, :, 500:1100] = _fill(dt, nd)  # a whole chunk of f64 without a valid pixel
    for out_shape in ((2, 1), (1, 2), (1, 3)):
        assert _same(ctx.resample(wide, out_shape, "average", nodata=nd), resample(wide, out_shape, "average", nodata=nd)), out_shape
    if dt == np.uint16:
        # 32771 > 2^15 rows into one: the column sums of uint16 no longer fit 32 bits (the other accumulators)
        for h in (32771, 32768):
            tall = np.full((1, h, 3), 65535, np.uint16)
            tall[0, ::7, 1] = rng.integers(0, 65536, size=len(tall[0, ::7, 1]))
            tall[0, ::5, 2] = 1000
            assert _same(ctx.resample(tall, (1, 2), "average", nodata=nd), resample(tall, (1, 2), "average", nodata=nd)), h


@pytest.mark.parametrize("h", (65535, 65536, 65539))
@pytest.mark.parametrize("dt", (np.uint8, np.int8), ids=("uint8", "int8"))
def test_kernel_wide_masked_average_of_8_bit(dt, h):
    """The masked average of an 8-bit dtype keeps a column's valid weight in 16 bits while h' < 65536 and takes the wide
    instance from there on: h rows into one row are h' = h (narrow, wide, wide), into two h' = 65535, 32768, 65539
    (narrow, narrow, wide).  65536 valid pixels of a column are the sharp case: a weight of 16 bits wraps to 0 and the
    output becomes the fill."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(970 + dt.num + h)
    ctx = _ctx()
    info = np.iinfo(dt)
    a = np.full((1, h, 3), info.max, dt)
    a[0, rng.random(h) < 0.3, 0] = 7
    vals = rng.integers(info.min, int(info.max), size=len(a[0, ::7, 1]), dtype=np.int64)  # the range without one value ...
    a[0, ::7, 1] = (vals + (vals >= 7)).astype(dt)  # ... which is 7: the column is valid throughout
    a[0, ::5, 2] = 7
    assert (a[0, :, 1] != 7).all() and (a[0, :, 0] == 7).any()  # u_i = h in column 1: 65536 does not fit 16 bits
    for out_shape in ((1, 2), (2, 2)):
        want = resample(a, out_shape, "average", nodata=7.0)
        filled = np.full(1, 99, np.uint64)
        got = ctx.resample(a, out_shape, "average", nodata=7.0, filled=filled)
        assert _same(got, want), (h, out_shape, got.tolist(), want.tolist())
        assert np.array_equal(filled, _count_fill(want, 7.0)), (h, out_shape, filled)


# ------------------------------------------------------------------------------- 2. the decimate geometry
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_decimate_geometry_equals_the_numpy_rule(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(1000 + dt.num)
    ctx = _ctx()
    V = 16 // dt.itemsize
    nd = _nodata_of(dt)
    nd_b = -9999.0 if dt.kind == "f" else -100.0 if dt.kind == "i" else 0.0
    sent = dt.type(77)
    for k in FACTORS:
        for h, w in ((13, 17), (64, 64), (3, 4100)):
            oh, ow = decimated_shape(h, w, k)
            a = _full_range(dt, (2, h, w), rng, nd)
            want = decimate(a, k, "average", nodata=nd)
            assert _same(ctx.decimate(a, k, "average", nodata=nd), want), (k, h, w)
            sbig, src = _padded(a, -w % V + V, sent)  # rows on 16-byte boundaries
            dbig, dst = _padded(np.full((2, oh, ow), sent, dt), 2, sent)
            assert ctx.decimate(src, k, "average", dst, nodata=nd) is dst and _same(dst, want), (k, h, w, "aligned")
            _check_padding(dbig, oh, ow, sent)
            assert _same(ctx.decimate(a, k, "nearest", nodata=nd), decimate(a, k, "nearest")), (k, h, w)
            b = _bounded(dt, (2, h, w), rng, nd_b, "random")
            filled = np.full(2, 99, np.uint64)
            got = ctx.decimate(b, k, "average", nodata=nd_b, filled=filled)
            assert _same(got, decimate(b, k, "average", nodata=nd_b)), (k, h, w, "bounded")
            assert np.array_equal(filled, _count_fill(got, nd_b)), (k, h, w, filled)
    z = np.full((1, 1, 1), _fill(dt, nd), dt)  # a single invalid pixel: the decimation fills, there is no identity size
    assert _same(ctx.decimate(z, 2, "average", nodata=nd), decimate(z, 2, "average", nodata=nd))


# ------------------------------------------------------------------------------- 3. behind the decoder
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TILE = 150, 170, 64  # 3 x 3 tiles of 64 pixels, ragged right and bottom
MARGIN = 21  # rows and columns of nodata around the data
WINDOWS = [(0, 0, H, W), (9, 11, 97, 110)]  # the whole raster, and a window off the tile grid over four tiles
OUT_SHAPES = [(37, 53), (200, 230)]


@pytest.fixture(scope="module", params=[np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def container(request):
    from flac_raster.streaming import build_streaming, read_window

    dt = np.dtype(request.param)
    rng = np.random.default_rng(31 + dt.itemsize)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(20000 + 9000 * np.sin(yy / 11.0 + b) + 8000 * np.cos(xx / 13.0) + rng.integers(0, 400, (H, W)))
                  for b in range(2)])
    r = (r / 7.0).astype(dt)  # (below 6000)
    r[:, :MARGIN, :] = r[:, -MARGIN:, :] = 0
    r[:, :, :MARGIN] = r[:, :, -MARGIN:] = 0
    # The container stores no nodata value, and the PCM-16 reading of a tile depends on the tile's own minimum and
    # maximum (a float zero comes back as another value): every tile gets a zero (the margin; a hole in the middle
    # tile) and one pixel of the same maximum, so that the zeros of all nine tiles decode to one value, the nodata
    # value of these tests.
    r[:, 90:100, 100:110] = 0
    for row in (30, 94, 128):
        for col in (30, 94, 140):
            r[:, row, col] = 6000
    data = build_streaming(r, TRANSFORM, "EPSG:32633", TILE)
    host = {w: read_window(data, window=w, device=None)[0] for w in WINDOWS}  # the expectation's input, read once
    for a in host.values():
        a.setflags(write=False)
    full = host[WINDOWS[0]]
    nd = float(full[0, 0, 0])
    assert (full[r == 0] == nd).all() and (full[r != 0] != nd).all()
    return data, dt, host, nd


@pytest.mark.parametrize("mode", ("nearest",) + MODES)
def test_container_reads_equal_the_rule_of_the_host_read(container, mode):
    from flac_raster.streaming import read_overview, read_window

    data, dt, host, nd = container
    for wdw in WINDOWS:
        for out_shape in OUT_SHAPES:
            want = resample(host[wdw], out_shape, mode, nodata=nd)
            dev, dw, idx = read_window(data, window=wdw, device=0, out_shape=out_shape, resampling=mode, nodata=nd)
            assert dw == wdw and dev.dtype == dt and _same(dev, want), (wdw, out_shape)
            got, hw, _ = read_window(data, window=wdw, device=None, out_shape=out_shape, resampling=mode, nodata=nd)
            assert hw == wdw and _same(got, want), (wdw, out_shape, "host")
        if mode in ("nearest", "average"):
            for k in (2, 8, 64):
                want = decimate(host[wdw], k, mode, nodata=nd)
                assert _same(read_window(data, window=wdw, device=0, decimate=k, resampling=mode, nodata=nd)[0], want), (wdw, k)
                assert _same(read_window(data, window=wdw, device=None, decimate=k, resampling=mode, nodata=nd)[0], want), (wdw, k)
    full = host[WINDOWS[0]]
    if mode == "average":
        want = decimate(full, 8, mode, nodata=nd)
        assert not _same(want, decimate(full, 8, mode))  # the margin no longer bleeds into the edge blocks
        assert (want == _fill(dt, nd)).any() and (want[:, 3:-3, 3:-3] != _fill(dt, nd)).all()
        for device in (0, None):
            assert _same(read_overview(data, 8, mode, device=device, nodata=nd)[0], want), device
    for device in (0, None):
        assert _same(read_overview(data, out_shape=(37, 53), resampling=mode, device=device, nodata=nd)[0],
                     resample(full, (37, 53), mode, nodata=nd)), device
    assert _ctx().resample_masked_timing() >= 0.0 and len(_ctx().decode_timing()) == 4


def test_container_refusals_counts_and_padding(container):
    from flac_raster.streaming import _window_items, read_window

    data, dt, host, nd = container
    with pytest.raises(ValueError, match="not both"):
        read_window(data, window=WINDOWS[1], device=0, decimate=2, out_shape=(8, 8), nodata=nd)
    with pytest.raises(ValueError, match="nodata"):
        read_window(data, window=WINDOWS[1], device=0, nodata=nd)
    with pytest.raises(ValueError, match="nodata"):
        read_window(data, window=WINDOWS[1], device=0, out_shape=(8, 8), nodata=0.5 if dt.kind != "f" else float("inf"))
    index, win, blob, items = _window_items(data, WINDOWS[1], None)
    assert len(items) == 4
    buf = np.frombuffer(blob, dtype=np.uint8)
    dst = np.full((2, 8, 8), 77, dt)
    ctx = _ctx()
    # items that do not cover the region: the unmasked entries' message, and the destination is left alone
    for mode in ("nearest",) + MODES:
        with pytest.raises(N.NativeError, match="do not cover the region"):
            ctx.decode_device_resampled(buf, items[:3], dst, dt, 2, (64, 8, 1), win, (8, 8), mode, N.DENORM_PCM16, nodata=nd)
    with pytest.raises(N.NativeError, match="do not cover the region"):
        ctx.decode_device_decimated(buf, items[:3], dst, dt, 2, (64, 8, 1), win, 16, "average", N.DENORM_PCM16, nodata=nd)
    assert _same(dst, np.full((2, 8, 8), 77, dt))
    # a padded destination: only the outputs are written; the counts are those of the output
    big = np.full((2, 9, 10), 77, dt)
    filled = np.full(2, 99, np.uint64)
    ctx.decode_device_resampled(buf, items, big, dt, 2, (90, 10, 1), win, (8, 8), "bilinear", N.DENORM_PCM16, nodata=nd,
                                filled=filled)
    want = resample(host[WINDOWS[1]], (8, 8), "bilinear", nodata=nd)
    assert _same(big[:, :8, :8], want) and np.array_equal(filled, _count_fill(want, nd))
    assert _same(big[:, 8, :], np.full((2, 10), 77, dt)) and _same(big[:, :, 8:], np.full((2, 9, 2), 77, dt))
    oh, ow = decimated_shape(win[2], win[3], 16)
    out = np.zeros((2, oh, ow), dt)
    ctx.decode_device_decimated(buf, items, out, dt, 2, (oh * ow, ow, 1), win, 16, "average", N.DENORM_PCM16, nodata=nd,
                                filled=filled)
    assert _same(out, decimate(host[WINDOWS[1]], 16, "average", nodata=nd)) and np.array_equal(filled, _count_fill(out, nd))
    with pytest.raises(ValueError, match="filled"):
        ctx.decode_device_decimated(buf, items, out, dt, 2, (oh * ow, ow, 1), win, 16, "average", N.DENORM_PCM16, nodata=nd,
                                    filled=np.zeros(3, np.uint64))


def test_plan_output_with_nodata_on_device():
    """``tiles.read_window_on_device(nodata=)``: device to device through the plan's frame offsets."""
    from flac_raster.tiles import read_window_on_device

    rng = np.random.default_rng(41)
    B, Hh, Ww = 2, 60, 130
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    r = np.stack([(3000 + 900 * np.sin(yy / 17.0 + b) + 700 * np.cos(xx / 29.0) + rng.integers(0, 60, (Hh, Ww)))
                  for b in range(B)]).astype(np.uint16)
    r[:, :, 40:75] = 0
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
        nd = float(np.bincount(full.ravel().astype(np.int64) + 32768).argmax() - 32768)  # what the zeros decode to
        assert (full == nd).mean() > 0.3
        filled = np.zeros(B, np.uint64)
        for mode in ("nearest",) + MODES:
            read_window_on_device(plan, wdw, dev, out_shape=(19, 50), resampling=mode, nodata=nd, filled=filled)
            got = np.empty((B, 19, 50), np.int16)
            ctx.d2h(got, dev)
            assert np.array_equal(got, resample(full, (19, 50), mode, nodata=nd)), mode
        read_window_on_device(plan, wdw, dev, decimate=4, resampling="average", nodata=nd, filled=filled)
        got = np.empty((B, 11, 20), np.int16)
        ctx.d2h(got, dev)
        assert np.array_equal(got, decimate(full, 4, "average", nodata=nd))
        assert np.array_equal(filled, _count_fill(got, nd)) and filled.all()
        with pytest.raises(ValueError, match="nodata"):
            read_window_on_device(plan, wdw, dev, nodata=nd)
    finally:
        ctx.free(dev)
        plan.close()


# ------------------------------------------------------------------------------- 4. refusals of the C ABI
def test_abi_refusals_reach_last_error():
    L = N.load()
    ctx = _ctx()
    src = np.arange(64, dtype=np.uint8).reshape(1, 8, 8)
    dst = np.full((1, 3, 5), 77, np.uint8)
    filled = np.full(1, 99, np.uint64)
    pf = filled.ctypes.data_as(C.POINTER(C.c_uint64))

    def job(cls, **kw):
        j = cls()
        j.src, j.dtype, j.channels, j.height, j.width = C.c_void_p(src.ctypes.data), N.DTYPE_CODES[src.dtype], 1, 8, 8
        j.src_band_stride, j.src_row_stride, j.src_col_stride = 64, 8, 1
        j.dst, j.dst_band_stride, j.dst_row_stride, j.dst_col_stride = C.c_void_p(dst.ctypes.data), 15, 5, 1
        j.resampling = N.RESAMPLE_AVERAGE
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    def refused(rc, word):
        msg = L.fra_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    rj, dj = job(N.ResampleJob, out_height=3, out_width=5), job(N.DecimateJob, factor=2)
    for nd in (256.0, -1.0, 0.5, float("nan"), float("inf")):  # not a nodata value of uint8
        refused(L.fra_resample_masked(ctx.h, C.byref(rj), nd, pf), "nodata")
        refused(L.fra_decimate_masked(ctx.h, C.byref(dj), nd, pf), "nodata")
    refused(L.fra_resample_masked(ctx.h, None, 0.0, pf), "null")
    refused(L.fra_decimate_masked(ctx.h, None, 0.0, pf), "null")
    refused(L.fra_resample_masked(None, C.byref(rj), 0.0, pf), "null")
    refused(L.fra_decode_device_resampled_masked(ctx.h, None, None, 3, 5, 1, None, 0.0, pf), "null")
    refused(L.fra_decode_device_decimated_masked(ctx.h, None, None, 2, 1, None, 0.0, pf), "null")
    refused(L.fra_resample_masked_timing(None), "null")
    assert filled[0] == 99 and (dst == 77).all()  # nothing ran
    with pytest.raises(ValueError, match="nodata"):  # the same refusal from Python, before the library is called
        ctx.resample(src, (3, 5), "average", nodata=256)
    with pytest.raises(ValueError, match="filled"):
        ctx.resample(src, (3, 5), "average", filled=filled)


# ------------------------------------------------------------------------------- 5. CLI
def test_cli_overview_with_nodata(container, tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app

    data, dt, host, nd = container
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    full = host[WINDOWS[0]]
    out = tmp_path / "ov.tif"
    res = CliRunner().invoke(app, ["overview", str(src), "-o", str(out), "--factor", "8", "--device", "0", "--nodata", repr(nd)])
    assert res.exit_code == 0, res.output
    px, info = read_geotiff(out)
    want = decimate(full, 8, "average", nodata=nd)
    assert _same(px, want) and info.nodata == nd
    share = 100.0 * (want[0] == _fill(dt, nd)).mean()
    assert f"nodata {nd:g}" in res.output and f"band 1 {share:.2f} %" in res.output, res.output
    out2 = tmp_path / "win.tif"
    res = CliRunner().invoke(app, ["window", str(src), "-o", str(out2), "--window", "9,11,97,110", "--device", "0",
                                   "--out-shape", "20,58", "--resampling", "cubic", "--nodata", repr(nd)])
    assert res.exit_code == 0, res.output
    px2, info2 = read_geotiff(out2)
    assert _same(px2, resample(host[WINDOWS[1]], (20, 58), "cubic", nodata=nd)) and info2.nodata == nd
    res = CliRunner().invoke(app, ["overview", str(src), "-o", str(out), "--factor", "8", "--device", "0"])
    assert res.exit_code == 0 and "band 1" not in res.output  # the default remains unmasked, and untagged
    px3, info3 = read_geotiff(out)
    assert _same(px3, decimate(full, 8, "average")) and info3.nodata is None
