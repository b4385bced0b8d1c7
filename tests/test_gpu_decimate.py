"""GPU tests of the decimated reads (``k_decimate`` alone through ``fra_decimate``, and behind the windowed read through
``fra_decode_device_decimated``).

Every comparison is bit-exact (floats: the same NaN positions and the same bits elsewhere, so a lost ``-0.0`` shows).
The expectation is never the kernel: it is ``resample.decimate`` -- the rule in numpy, checked on the CPU against exact
arithmetic -- applied to the host decoder's samples cropped, to numpy's ``denormalize_from_audio`` cropped, to the host
``read_window``, and for the plan path to the oracle's normalised samples.  The shapes are the smallest at which the
thread mapping can go wrong: a single pixel, one block short by a row and long by a column, two and a bit blocks by
three less a bit, rows that are and are not 16-byte aligned (vector and scalar loads), more than one block of lanes.
"""
import numpy as np
import pytest

import oracle as O
from flac_raster import _native as N
from flac_raster.decoder import pcm16_float
from flac_raster.geo import Affine
from flac_raster.normalization import NormalizationParams, denormalize_from_audio
from flac_raster.resample import decimate, decimated_shape
from flac_raster.tiff import read_geotiff

pytestmark = pytest.mark.gpu

SENTINEL = -12345
BS = 16
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
FACTORS = (2, 4, 8, 16, 32, 64)
MODES = ("nearest", "average")


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


# ------------------------------------------------------------------------------- 1. the kernel alone
def _raster(dt, shape, rng):
    """Full-range integers; floats with cancelling magnitudes in most blocks (a wrong summation order shows), and a
    NaN, both infinities and negative zeros (a skipped or reordered special shows)."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        a = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
        a.flat[0] = info.max
        return a
    pick = rng.integers(0, 6, size=shape)
    a = np.choose(pick, [np.full(shape, 1e16), np.full(shape, -1e16), np.ones(shape), rng.normal(0.0, 3.0, size=shape),
                         np.full(shape, -0.0), rng.uniform(0.0, 1e-3, size=shape)]).astype(dt)
    n = a.size
    for v in (np.nan, np.inf, -np.inf, np.inf):  # (two +inf: inf + inf stays inf, inf + -inf is NaN)
        a.flat[int(rng.integers(0, n))] = v
    return a


def _shapes(k):
    s = [(1, 1), (k - 1, k + 1), (2 * k + 1, 3 * k - 1)]
    return s + [(130, 67)] if k == 64 else s


def _padded(a, pad_cols, fill):
    """``a`` (B, h, w) as a view of a larger array: ``pad_cols`` spare columns per row and one spare row per band."""
    B, h, w = a.shape
    big = np.full((B, h + 1, w + pad_cols), fill, a.dtype)
    big[:, :h, :w] = a
    return big, big[:, :h, :w]


def _check_padding(big, h, w, fill):
    assert _same(big[:, h, :], np.full_like(big[:, h, :], fill)) and _same(big[:, :, w:], np.full_like(big[:, :, w:], fill))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_alone_equals_the_numpy_rule(dt, mode):
    dt = np.dtype(dt)
    rng = np.random.default_rng(100 + dt.num)
    ctx = _ctx()
    fill = _sentinel(dt)
    V = 16 // dt.itemsize
    for k in FACTORS:
        for (h, w) in _shapes(k):
            a = _raster(dt, (3, h, w), rng)
            want = decimate(a, k, mode)
            oh, ow = decimated_shape(h, w, k)
            assert want.shape == (3, oh, ow)
            # host source, rows not 16-byte aligned (scalar loads) and aligned (16-byte loads), padded destination
            for pad in (5, -w % V + V):
                sbig, src = _padded(a, pad, fill)
                dbig, dst = _padded(np.full((3, oh, ow), fill, dt), 2, fill)
                assert ctx.decimate(src, k, mode, dst) is dst
                assert _same(dst, want), (k, h, w, pad)
                _check_padding(dbig, oh, ow, fill)
                assert _same(sbig[:, :h, :w], a)
            assert _same(ctx.decimate(a, k, mode), want), (k, h, w)  # contiguous, a new array comes back
            assert ctx.decimate_timing() >= 0.0
        # the largest shape again: pixel-interleaved source, then device-resident source and destination
        inter = np.ascontiguousarray(a.transpose(1, 2, 0))  # (h, w, 3)
        assert _same(ctx.decimate(inter.transpose(2, 0, 1), k, mode), want), (k, "interleaved")
        rs = w + (-w % V)  # aligned rows on the device
        staged = np.full((3, h, rs), fill, dt)
        staged[:, :, :w] = a
        d_src, d_dst = ctx.alloc(staged.nbytes), ctx.alloc(3 * (oh + 1) * (ow + 2) * dt.itemsize)
        try:
            ctx.h2d(d_src, staged)
            dbig = np.full((3, oh + 1, ow + 2), fill, dt)
            ctx.h2d(d_dst, dbig)
            ctx.decimate(d_src, k, mode, d_dst, dtype=dt, shape=(3, h, w), strides=(h * rs, rs, 1),
                         dst_strides=((oh + 1) * (ow + 2), ow + 2, 1))
            ctx.d2h(dbig, d_dst)
        finally:
            ctx.free(d_src)
            ctx.free(d_dst)
        assert _same(dbig[:, :oh, :ow], want), (k, "device")
        _check_padding(dbig, oh, ow, fill)


def test_kernel_order_and_specials_are_seen():
    """The float data above must be able to tell a wrong order or a skipped special from the rule."""
    ctx = _ctx()
    row = np.array([[[1e16, 1.0, -1e16, 1.0]]])
    assert ctx.decimate(row, 4, "average")[0, 0, 0] == 0.0  # the tree; left to right gives 0.25
    col = np.array([[[1e16, 0.0], [1.0, 0.0], [-1e16, 0.0], [1.0, 0.0]]])
    assert ctx.decimate(col, 4, "average")[0, 0, 0] == 0.125  # rows top to bottom
    z = np.full((1, 3, 2), -0.0, np.float32)
    got = ctx.decimate(z, 2, "average")
    assert np.signbit(got[0, 0, 0]) and np.signbit(got[0, 1, 0]) and _same(got, decimate(z, 2, "average"))
    assert not np.signbit(ctx.decimate(z[:, :, :1], 2, "average")[0, 0, 0])  # the +0.0 pad was added
    wide = np.zeros((1, 2, 256), np.float64)  # k = 64 with f64: 32 lanes per block finish the tree
    wide[0, 0, ::2], wide[0, 0, 1::2], wide[0, 1, 5] = 1e16, -1e16, 3.0
    wide[0, 0, 64:128] = np.tile([1e16, 1.0, -1e16, 1.0], 16)
    assert _same(ctx.decimate(wide, 64, "average"), decimate(wide, 64, "average"))
    ties = np.array([[[1, 2, 3, 4, 0, 1], [1, 2, 4, 3, 1, 0]]], np.int16)  # 1.5, 3.5, 0.5: half to even
    assert np.array_equal(ctx.decimate(ties, 2, "average"), [[[2, 4, 0]]])


# ------------------------------------------------------------------------------- 2. decoded path, raw samples
def _smooth(n, ch, bps, rng):
    """Correlated channels (so mid-side occurs) on a random walk."""
    amp = 300 if bps == 16 else 3_000_000
    lim = 32767 if bps == 16 else 2**31 - 1
    walk = np.cumsum(rng.integers(-amp, amp, size=(n, 1)), axis=0)
    x = walk + rng.integers(-amp // 10, amp // 10, size=(n, ch)) + 37 * np.arange(ch)[None]
    return x.clip(-lim - 1, lim).astype(np.int16 if bps == 16 else np.int32)


def _inter(tile, roi):
    r0, c0, h, w = tile
    ra, rb = max(r0, roi[0]), min(r0 + h, roi[0] + roi[2])
    ca, cb = max(c0, roi[1]), min(c0 + w, roi[1] + roi[3])
    return (ra, rb, ca, cb) if ra < rb and ca < cb else None


def _frames(tile, roi, bs):
    """Needed frames of a tile by the header's arithmetic, 0 when the tile misses the region."""
    x = _inter(tile, roi)
    if x is None:
        return 0
    ra, rb, ca, cb = x
    r0, c0, _, w = tile
    p_lo = (ra - r0) * w + (ca - c0)
    p_hi = (rb - 1 - r0) * w + (cb - c0)
    return (p_hi - 1) // bs - p_lo // bs + 1


# 9 x 23 and 9 x 11 pixels: 23 and 11 do not divide 16, so frames straddle rows and every last frame is partial
GRID = [(0, 0, 9, 23), (0, 23, 9, 11), (9, 0, 9, 23), (9, 23, 9, 11)]
ROIS = {
    "whole grid": (0, 0, 18, 34),
    "all four tiles": (7, 20, 4, 8),
    "inside one tile": (2, 5, 3, 10),
    "narrower than k": (6, 22, 7, 1),
}


class Grid:
    """Tile streams of a small raster, the host decoder's samples of every tile placed in the raster, and one blob
    with unaligned starts and gaps between the streams."""

    def __init__(self, tiles, ch, bps, seed):
        rng = np.random.default_rng(seed)
        self.tiles, self.ch = tiles, ch
        self.dtype = np.dtype(np.int16 if bps == 16 else np.int32)
        H = max(r + h for r, _, h, _ in tiles)
        W = max(c + w for _, c, _, w in tiles)
        self.full = np.zeros((ch, H, W), self.dtype)
        blob, self.items = b"\x00" * 5, []
        for (r, c, h, w) in tiles:
            s = O.encode(_smooth(h * w, ch, bps, rng), 44100, level=5, blocksize=BS)
            x, info = N.decode(s)  # the expectation: the host decoder
            assert x.shape == (h * w, ch) and info.blocksize == BS
            self.full[:, r:r + h, c:c + w] = x.reshape(h, w, ch).transpose(2, 0, 1)
            self.items.append({"offset": len(blob), "bytes": len(s), "window": (r, c, h, w)})
            blob += s + b"\x00\x00\x00"
        self.blob = blob
        self.full.setflags(write=False)

    def dst(self, roi, k):
        """A sentinel-filled destination with padding after every row and band, and its strides."""
        oh, ow = decimated_shape(roi[2], roi[3], k)
        row_stride, band_stride = ow + 3, (oh + 1) * (ow + 3) + 5
        return np.full(self.ch * band_stride + 7, SENTINEL, self.dtype), (band_stride, row_stride, 1)

    def read(self, roi, k, mode, items=None):
        items = self.items if items is None else items
        oh, ow = decimated_shape(roi[2], roi[3], k)
        dst, (band_stride, row_stride, _) = self.dst(roi, k)
        infos = _ctx().decode_device_decimated(self.blob, items, dst, self.dtype, self.ch, (band_stride, row_stride, 1),
                                               roi, k, mode)
        bands = dst[:self.ch * band_stride].reshape(self.ch, band_stride)
        body = bands[:, :(oh + 1) * row_stride].reshape(self.ch, oh + 1, row_stride)
        assert (body[:, oh, :] == SENTINEL).all() and (body[:, :, ow:] == SENTINEL).all(), "written outside the output"
        assert (bands[:, (oh + 1) * row_stride:] == SENTINEL).all() and (dst[self.ch * band_stride:] == SENTINEL).all()
        for it, inf in zip(items, infos):  # as the windowed read reports them
            x = _inter(it["window"], roi)
            assert inf.nframes == _frames(it["window"], roi, BS), (it["window"], roi)
            assert inf.nsamples == (0 if x is None else (x[1] - x[0]) * (x[3] - x[2]))
            assert x is None or (inf.channels == self.ch and inf.blocksize == BS)
        return body[:, :oh, :ow].copy()


@pytest.mark.parametrize("bps", [16, 32])
@pytest.mark.parametrize("ch", [1, 2, 4])
def test_grid_regions_equal_decimate_of_the_host_decoder_cropped(ch, bps):
    g = Grid(GRID, ch, bps, seed=10 * ch + bps)
    ctx = _ctx()
    for name, roi in ROIS.items():
        r, c, h, w = roi
        crop = g.full[:, r:r + h, c:c + w]
        for k in (2, 4):
            for mode in MODES:
                assert np.array_equal(g.read(roi, k, mode), decimate(crop, k, mode)), (name, k, mode)
        t = ctx.decode_timing()
        assert len(t) == 4 and t[3] >= 0.0 and ctx.decimate_timing() >= 0.0


# ------------------------------------------------------------------------------- 3. denormalisation
@pytest.mark.parametrize("sem", ["int", "pcm16"])
@pytest.mark.parametrize("dt", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_denormalised_region_equals_decimate_of_numpy_cropped(dt, sem):
    dt = np.dtype(dt)
    rng = np.random.default_rng(31 + dt.itemsize)
    B, h, w = 2, 37, 53
    if dt.kind == "f":
        t = (rng.normal(0.3, 0.2, size=(B, h, w)) * 1000).astype(dt)
        t[0, 3, 4] = np.nan
    else:
        t = rng.integers(300, 60000, size=(B, h, w)).astype(dt)
    bits = 16 if dt.kind != "f" else 24
    audio, mn, mx = O.normalize(t.transpose(1, 2, 0).reshape(-1, B), bits)
    s = O.encode(audio, 44100, level=5)
    ints, _ = N.decode(s)
    p = NormalizationParams(float(mn), float(mx), dt.name, bits, 32767 if bits == 16 else 8388607)
    ints = ints.astype(np.int16) if bits == 16 else ints
    want = denormalize_from_audio(ints if sem == "int" else pcm16_float(ints), p).reshape(h, w, B).transpose(2, 0, 1)
    tile = (100, 200, h, w)  # the tile somewhere in a larger raster
    items = [{"offset": 0, "bytes": len(s), "window": tile, "data_min": float(mn), "data_max": float(mx)}]
    roi = (102, 201, 21, 30)
    crop = np.ascontiguousarray(want[:, 2:23, 1:31])
    for mode in MODES:
        oh, ow = decimated_shape(21, 30, 4)
        got = np.zeros((B, oh, ow), dt)
        _ctx().decode_device_decimated(s, items, got, dt, B, (oh * ow, ow, 1), roi, 4, mode,
                                       N.DENORM_INT if sem == "int" else N.DENORM_PCM16)
        assert _same(got, decimate(crop, 4, mode)), mode


# ------------------------------------------------------------------------------- 4. plan output through offsets
def test_plan_output_decimated_through_frame_offsets():
    from flac_raster.tiles import read_window_on_device

    rng = np.random.default_rng(11)
    B, H, W = 4, 300, 660
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(3000 + 900 * np.sin(yy / 17.0 + b) + 700 * np.cos(xx / 29.0) + rng.integers(0, 60, (H, W)))
                  for b in range(B)]).astype(np.uint16)
    tiles = [(0, 0, 300, 260), (0, 260, 300, 260), (0, 520, 300, 140)]  # the last one ragged
    want = np.zeros((B, H, W), np.int16)
    for (y, x, h, w) in tiles:
        audio, _, _ = O.normalize(r[:, y:y + h, x:x + w].transpose(1, 2, 0).reshape(-1, B), 16)
        want[:, y:y + h, x:x + w] = audio.reshape(h, w, B).transpose(2, 0, 1)
    wins = [(10, 20, 50, 100), (100, 200, 101, 401), (0, 0, 300, 660)]
    ctx = _ctx()
    plan = N.Plan(ctx, r.ctypes.data, False, r.dtype, B, (H * W, W, 1), tiles, 5, 4096, 16, keepalive=r)
    dev = ctx.alloc(B * 150 * 330 * 2)
    try:
        plan.execute()
        plan.sync()
        for wdw in wins:
            y, x, h, w = wdw
            for mode in MODES:
                oh, ow = decimated_shape(h, w, 2)
                ctx.h2d(dev, np.zeros(B * oh * ow, np.int16))
                infos = read_window_on_device(plan, wdw, dev, decimate=2, resampling=mode)
                got = np.empty((B, oh, ow), np.int16)
                ctx.d2h(got, dev)
                assert np.array_equal(got, decimate(want[:, y:y + h, x:x + w], 2, mode)), (wdw, mode)
                assert [i.nframes for i in infos] == [_frames(t, wdw, 4096) for t in tiles]
    finally:
        ctx.free(dev)
        plan.close()


# ------------------------------------------------------------------------------- 5. container and CLI
def test_container_decimated_reads_and_cli(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.streaming import build_streaming, read_overview, read_window

    rng = np.random.default_rng(12)
    H, W = 700, 900
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(20000 + 9000 * np.sin(yy / 41.0 + b) + 8000 * np.cos(xx / 53.0) + rng.integers(0, 400, (H, W)))
                  for b in range(3)]).astype(np.uint16)
    data = build_streaming(r, Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0), "EPSG:32633", 256)
    for wdw in [(200, 200, 120, 130), (400, 700, 300, 200)]:
        for mode in MODES:
            host, hw, _ = read_window(data, window=wdw, device=None, decimate=4, resampling=mode)
            dev, dw, _ = read_window(data, window=wdw, device=0, decimate=4, resampling=mode)
            assert hw == dw == wdw and host.shape == (3,) + decimated_shape(wdw[2], wdw[3], 4)
            assert dev.dtype == np.uint16 and np.array_equal(dev, host), (wdw, mode)
    for sem in ("pcm16", "int"):
        host, _ = read_overview(data, 4, device=None, semantics=sem)
        dev, idx = read_overview(data, 4, device=0, semantics=sem)
        assert host.shape == (3, 175, 225) and len(idx["frames"]) == 12 and np.array_equal(dev, host), sem
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    out = tmp_path / "win.tif"
    res = CliRunner().invoke(app, ["window", str(src), "-o", str(out), "--window", "200,200,120,130", "--device", "0",
                                   "--decimate", "4", "--resampling", "average"])
    assert res.exit_code == 0, res.output
    px, info = read_geotiff(out)
    want, _, _ = read_window(data, window=(200, 200, 120, 130), device=None, decimate=4, resampling="average")
    assert np.array_equal(px, want) and "32633" in str(info.crs)
    assert tuple(info.transform)[:6] == (40.0, 0.0, 502000.0, 0.0, -40.0, 4098000.0)
    out2 = tmp_path / "preview.tif"
    res = CliRunner().invoke(app, ["overview", str(src), "-o", str(out2), "--factor", "8", "--device", "0"])
    assert res.exit_code == 0, res.output
    px2, info2 = read_geotiff(out2)
    assert np.array_equal(px2, read_overview(data, 8, device=None)[0])
    assert tuple(info2.transform)[:6] == (80.0, 0.0, 500000.0, 0.0, -80.0, 4100000.0)


# ------------------------------------------------------------------------------- 6. refusals and damage
class Bits:
    def __init__(self):
        self.b = []

    def put(self, v, n):
        v &= (1 << n) - 1
        self.b.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def bytes(self):
        b = self.b + [0] * (-len(self.b) % 8)
        return bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))


def _message(call):
    with pytest.raises(N.NativeError) as e:
        call()
    return str(e.value)


def test_refusals_and_damage_leave_the_destination_alone():
    ctx = _ctx()
    g = Grid(GRID, 2, 16, seed=23)
    roi = ROIS["all four tiles"]

    # a region with an uncovered corner: the fourth tile is absent from the job
    dst, strides = g.dst(roi, 2)
    msg = _message(lambda: ctx.decode_device_decimated(g.blob, g.items[:3], dst, g.dtype, 2, strides, roi, 2, "average"))
    assert "do not cover the region" in msg and (dst == SENTINEL).all()

    # a flipped byte in a needed frame: the windowed read's message
    rng = np.random.default_rng(41)
    s, fb, _ = O.encode(_smooth(10 * 16, 1, 16, rng), 44100, level=5, blocksize=16, return_info=True)
    pos = 86 + int(fb[:3].sum()) + int(fb[3]) // 2  # inside frame 3 = row 3 of the 10 x 16 tile
    bad = bytearray(s)
    bad[pos] ^= 0x04
    bad = bytes(bad)
    items = [{"offset": 0, "bytes": len(bad), "window": (0, 0, 10, 16)}]
    roi = (2, 0, 4, 16)
    full = np.full((4, 16), SENTINEL, np.int16)
    plain = _message(lambda: ctx.decode_device_window(bad, items, full, np.int16, 1, (64, 16, 1), roi))
    assert "lost sync / corrupt frame at byte" in plain
    dst = np.full(2 * 9 + 3, SENTINEL, np.int16)
    for mode in MODES:  # (nearest needs rows 3 and 5 only, but the whole region is decoded)
        msg = _message(lambda: ctx.decode_device_decimated(bad, items, dst, np.int16, 1, (18, 9, 1), roi, 2, mode))
        assert msg == plain and (dst == SENTINEL).all()
    # the same damage outside the region is not met, and the context decodes afterwards
    good, _ = N.decode(s)
    roi = (5, 0, 4, 16)
    got = np.full((1, 2, 8), SENTINEL, np.int16)
    ctx.decode_device_decimated(bad, items, got, np.int16, 1, (16, 8, 1), roi, 2, "average")
    assert np.array_equal(got, decimate(good.reshape(1, 10, 16)[:, 5:9].astype(np.int16), 2, "average"))

    # a 33-bit side channel (32-bps mid-side): not supported on the device
    mid = rng.integers(-2**31, 2**31, size=16)
    side = np.clip(rng.integers(-2**31, 2**31, size=16) * 2 + 1, -2**32, 2**32 - 1)
    b = Bits()
    b.put(0, 1); b.put(1, 6); b.put(0, 1)
    for v in mid:
        b.put(int(v), 32)
    b.put(0, 1); b.put(1, 6); b.put(0, 1)
    for v in side:
        b.put(int(v), 33)
    fh = bytes([0xFF, 0xF8, 0x69, 0xAE, 0x00, 0x0F])  # 16 samples (8-bit code), 44.1 kHz, mid-side, 32 bps, frame 0
    f = fh + bytes([O.crc8(fh)]) + b.bytes()
    stream = N.stream_header(2, 32, 44100, 16) + f + O.crc16(f).to_bytes(2, "big")
    host, info = N.decode(stream)  # the host decoder accepts it
    assert info.bps == 32 and host.shape == (16, 2)
    items = [{"offset": 0, "bytes": len(stream), "window": (0, 0, 1, 16)}]
    dst = np.full(2 * 8 + 5, SENTINEL, np.int32)
    msg = _message(lambda: ctx.decode_device_decimated(stream, items, dst, np.int32, 2, (8, 8, 1), (0, 0, 1, 16), 2,
                                                       "nearest"))
    assert "not supported on the device" in msg and (dst == SENTINEL).all()
