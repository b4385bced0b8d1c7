"""GPU tests of the windowed read (``fra_decode_device_window``: frame selection, k_dec_parse / k_dec_restore over the
selected frames, the clip of k_dec_scatter).

Every comparison is bit-exact.  The expectation is never the windowed read itself: the host decoder's samples cropped,
numpy's ``denormalize_from_audio`` cropped, the host ``read_window``, and for the plan path the oracle's normalised
samples.  The shapes are the smallest at which the selection, the 64-frame lane groups and the clip can go wrong:
streams are encoded with a block size of 16, so a tile of a few hundred samples has many frames.
"""
import numpy as np
import pytest

import oracle as O
from flac_raster import _native as N
from flac_raster.decoder import pcm16_float
from flac_raster.geo import Affine
from flac_raster.normalization import NormalizationParams, denormalize_from_audio
from flac_raster.tiff import read_geotiff

pytestmark = pytest.mark.gpu

SENTINEL = -12345
BS = 16


def _ctx():
    return N.default_context(0)


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
    """(first, last) needed frame of a tile by the header's arithmetic, None when the tile misses the region."""
    x = _inter(tile, roi)
    if x is None:
        return None
    ra, rb, ca, cb = x
    r0, c0, _, w = tile
    p_lo = (ra - r0) * w + (ca - c0)
    p_hi = (rb - 1 - r0) * w + (cb - c0)
    return p_lo // bs, (p_hi - 1) // bs


class Grid:
    """Tile streams of a small raster, the host decoder's samples of every tile placed in the raster, and one blob
    with unaligned starts and gaps between the streams."""

    def __init__(self, tiles, ch, bps, seed, level=5, bs=BS):
        rng = np.random.default_rng(seed)
        self.tiles, self.ch, self.bs = tiles, ch, bs
        self.dtype = np.int16 if bps == 16 else np.int32
        H = max(r + h for r, _, h, _ in tiles)
        W = max(c + w for _, c, _, w in tiles)
        self.full = np.full((ch, H, W), SENTINEL, np.int32)
        self.streams, blob, self.items = [], b"\x00" * 5, []
        for (r, c, h, w) in tiles:
            s = O.encode(_smooth(h * w, ch, bps, rng), 44100, level=level, blocksize=bs)
            x, info = N.decode(s)  # the expectation: the host decoder
            assert x.shape == (h * w, ch) and info.blocksize == bs
            self.full[:, r:r + h, c:c + w] = x.reshape(h, w, ch).transpose(2, 0, 1)
            self.items.append({"offset": len(blob), "bytes": len(s), "window": (r, c, h, w)})
            self.streams.append(s)
            blob += s + b"\x00\x00\x00"
        self.blob = blob
        self.full.setflags(write=False)

    def read(self, roi, items=None, data=None):
        """One windowed read into a sentinel-filled destination with padding after every row and band; returns the
        (ch, h, w) region and the infos, and checks that nothing outside the intersections was written."""
        items = self.items if items is None else items
        _, _, h, w = roi
        row_stride, band_stride = w + 3, (h + 1) * (w + 3) + 5
        dst = np.full(self.ch * band_stride + 7, SENTINEL, self.dtype)
        infos = _ctx().decode_device_window(self.blob if data is None else data, items, dst, self.dtype, self.ch,
                                            (band_stride, row_stride, 1), roi)
        bands = dst[:self.ch * band_stride].reshape(self.ch, band_stride)
        body = bands[:, :(h + 1) * row_stride].reshape(self.ch, h + 1, row_stride)
        got = body[:, :h, :w].astype(np.int32)
        assert (body[:, h, :] == SENTINEL).all() and (body[:, :, w:] == SENTINEL).all(), "written outside the region"
        assert (bands[:, (h + 1) * row_stride:] == SENTINEL).all() and (dst[self.ch * band_stride:] == SENTINEL).all()
        want = np.full((self.ch, h, w), SENTINEL, np.int32)
        for it, inf in zip(items, infos):
            x = _inter(it["window"], roi)
            fr = _frames(it["window"], roi, self.bs)
            if x is None:
                assert (inf.nframes, inf.nsamples) == (0, 0), it["window"]
                continue
            ra, rb, ca, cb = x
            assert inf.nframes == fr[1] - fr[0] + 1, (it["window"], roi, inf.nframes, fr)
            assert inf.nsamples == (rb - ra) * (cb - ca) and inf.channels == self.ch
            want[:, ra - roi[0]:rb - roi[0], ca - roi[1]:cb - roi[1]] = self.full[:, ra:rb, ca:cb]
        assert np.array_equal(got, want), roi  # (pixels of the region that no item covers keep the sentinel)
        return got, infos


# ------------------------------------------------------------------------------- 1. raw samples on a 2 x 2 grid
# 9 x 23 and 9 x 11 pixels: 23 and 11 do not divide 16, so frames straddle rows and every last frame is partial
GRID = [(0, 0, 9, 23), (0, 23, 9, 11), (9, 0, 9, 23), (9, 23, 9, 11)]


def _last_frame_roi(tile):
    r0, c0, h, w = tile
    s = (h * w - 1) // BS * BS
    assert s // w == h - 1 and h * w % BS
    return (r0 + h - 1, c0 + s % w, 1, w - s % w)


ROIS = {
    "whole grid": (0, 0, 18, 34),
    "single pixel": (13, 25, 1, 1),
    "mid-frame to mid-frame": (2, 5, 3, 10),
    "all four tiles": (7, 20, 4, 8),
    "misses two tiles": (2, 3, 10, 15),
    **{f"last partial frame of tile {k}": _last_frame_roi(t) for k, t in enumerate(GRID)},
}


@pytest.mark.parametrize("bps", [16, 32])
@pytest.mark.parametrize("ch", [1, 2, 4])
def test_grid_regions_equal_the_host_decoder_cropped(ch, bps):
    g = Grid(GRID, ch, bps, seed=10 * ch + bps)
    for name, roi in ROIS.items():
        got, infos = g.read(roi)
        if name == "whole grid":  # must equal the full decode
            full = np.full((ch, 18, 34), SENTINEL, g.dtype)
            _ctx().decode_device(g.blob, g.items, full, g.dtype, ch, (18 * 34, 34, 1))
            assert np.array_equal(got, full.astype(np.int32))
        if name.startswith("last partial"):
            assert sorted(i.nframes for i in infos) == [0, 0, 0, 1]
        if name == "misses two tiles":
            assert [i.nframes > 0 for i in infos] == [True, False, True, False]
    # a region over all four tiles with one of them absent from the job: its pixels keep the caller's values
    got, _ = g.read(ROIS["all four tiles"], items=g.items[:3])
    assert (got[:, 2:, 3:] == SENTINEL).all() and (got[:, :2, :] != SENTINEL).any()


def test_selection_inside_and_across_the_64_frame_lane_group():
    g = Grid([(0, 0, 70, 16)], 2, 16, seed=21)  # 70 frames of 16: the stream crosses the lane group
    _, infos = g.read((60, 0, 9, 16))           # frames 60..68: the selection crosses nothing
    assert infos[0].nframes == 9
    _, infos = g.read((2, 0, 67, 16))           # frames 2..68: 67 selected frames span two groups
    assert infos[0].nframes == 67
    g2 = Grid([(0, 0, 69, 16), (60, 16, 9, 7)], 1, 16, seed=22)  # 63 samples next door: a partial last frame
    _, infos = g2.read((61, 3, 8, 20))
    assert [i.nframes for i in infos] == [8, 4]


def test_pixel_interleaved_destination_and_device_resident_input():
    g = Grid(GRID, 2, 16, seed=23)
    roi = (7, 20, 4, 8)
    want, _ = g.read(roi)
    r, c, h, w = roi
    dst = np.full((h, w + 2, 2), 77, np.int16)  # (row, col, band) with two spare columns per row
    _ctx().decode_device_window(g.blob, g.items, dst, np.int16, 2, (1, (w + 2) * 2, 2), roi)
    assert np.array_equal(dst[:, :w, :].transpose(2, 0, 1).astype(np.int32), want) and (dst[:, w:, :] == 77).all()
    ctx = _ctx()
    buf = np.frombuffer(g.blob, np.uint8)
    dev = ctx.alloc(buf.size)
    try:
        ctx.h2d(dev, buf)
        got, _ = g.read(roi, data=(dev, buf.size))  # no offsets: the library fetches the intersecting streams
    finally:
        ctx.free(dev)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------- 2. a false candidate
class Bits:
    def __init__(self):
        self.b = []

    def put(self, v, n):
        v &= (1 << n) - 1
        self.b.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def bytes(self):
        b = self.b + [0] * (-len(self.b) % 8)
        return bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))


def _frame16(number, body: Bits) -> bytes:
    """A mono 16-bit frame of 16 samples (8-bit block size code) at 44.1 kHz."""
    fh = bytes([0xFF, 0xF8, 0x69, 0x08, number, 0x0F])
    f = fh + bytes([O.crc8(fh)]) + body.bytes()
    return f + O.crc16(f).to_bytes(2, "big")


def test_false_candidates_carrying_the_first_selected_number():
    """Three VERBATIM frames whose samples spell a complete frame header numbered 1 with a valid CRC-8.  A region
    needing frames 1-2 meets such a candidate before the real frame 1: it fails its CRC-16 and the local chain moves
    on."""
    fake = bytes([0xFF, 0xF8, 0x69, 0x08, 0x01, 0x0F])
    fake += bytes([O.crc8(fake)]) + b"\x00"
    smp = [5, -6] + [int.from_bytes(fake[i:i + 2], "big", signed=True) for i in range(0, len(fake), 2)]
    smp += [100, -200, 300, -400, 500, -600, 700, -800, 900, -1000]
    assert len(smp) == 16
    frames = b""
    for k in range(3):
        b = Bits()
        b.put(0, 1); b.put(1, 6); b.put(0, 1)  # VERBATIM
        for v in smp:
            b.put(v, 16)
        frames += _frame16(k, b)
    assert frames.count(fake[:7]) == 4  # frame 1's own header and one copy inside every frame
    stream = N.stream_header(1, 16, 44100, 16) + frames
    want, _ = N.decode(stream)  # the host decoder accepts the stream
    assert want.shape == (48, 1)
    items = [{"offset": 0, "bytes": len(stream), "window": (0, 0, 3, 16)}]
    for roi, nfr in (((1, 0, 2, 16), 2), ((1, 4, 1, 5), 1), ((0, 0, 3, 16), 3)):
        dst = np.full((roi[2], roi[3]), SENTINEL, np.int16)
        infos = _ctx().decode_device_window(stream, items, dst, np.int16, 1, (dst.size, roi[3], 1), roi)
        assert infos[0].nframes == nfr
        assert np.array_equal(dst, want.reshape(3, 16)[roi[0]:roi[0] + roi[2], roi[1]:roi[1] + roi[3]])


# ------------------------------------------------------------------------------- 3. denormalisation
@pytest.mark.parametrize("mode", ["int", "pcm16"])
@pytest.mark.parametrize("dt", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_denormalised_window_equals_numpy_cropped(dt, mode):
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
    ints, info = N.decode(s)
    p = NormalizationParams(float(mn), float(mx), dt.name, bits, 32767 if bits == 16 else 8388607)
    ints = ints.astype(np.int16) if bits == 16 else ints
    want = denormalize_from_audio(ints if mode == "int" else pcm16_float(ints), p).reshape(h, w, B).transpose(2, 0, 1)
    tile = (100, 200, h, w)  # the tile somewhere in a larger raster
    items = [{"offset": 0, "bytes": len(s), "window": tile, "data_min": float(mn), "data_max": float(mx)}]
    roi = (102, 201, 20, 30)  # holds the NaN pixel (103, 204)
    got = np.zeros((B, 20, 30), dt)
    _ctx().decode_device_window(s, items, got, dt, B, (600, 30, 1), roi,
                                N.DENORM_INT if mode == "int" else N.DENORM_PCM16)
    assert np.array_equal(got, want[:, 2:22, 1:31], equal_nan=dt.kind == "f")


# ------------------------------------------------------------------------------- 4. container
def test_container_windows_and_cli(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.streaming import build_streaming, read_window

    rng = np.random.default_rng(12)
    H, W = 700, 900
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(20000 + 9000 * np.sin(yy / 41.0 + b) + 8000 * np.cos(xx / 53.0) + rng.integers(0, 400, (H, W)))
                  for b in range(3)]).astype(np.uint16)
    data = build_streaming(r, Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0), "EPSG:32633", 256)
    # inside a tile, across a corner, across the ragged last column of tiles (and the ragged last row)
    wins = [(300, 300, 100, 120), (200, 200, 120, 130), (400, 700, 300, 200)]
    for sem in ("pcm16", "int"):
        for wdw in wins:
            host, hw, idx = read_window(data, window=wdw, device=None, semantics=sem)
            dev, dw, _ = read_window(data, window=wdw, device=0, semantics=sem)
            assert hw == dw == wdw and len(idx["frames"]) == 12
            assert host.dtype == np.uint16 and np.array_equal(dev, host), (sem, wdw)
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    out = tmp_path / "win.tif"
    res = CliRunner().invoke(app, ["window", str(src), "-o", str(out), "--window", "200,200,120,130", "--device", "0"])
    assert res.exit_code == 0, res.output
    px, info = read_geotiff(out)
    want, _, _ = read_window(data, window=wins[1], device=None)
    assert np.array_equal(px, want) and "32633" in str(info.crs)
    assert tuple(info.transform)[:6] == (10.0, 0.0, 502000.0, 0.0, -10.0, 4098000.0)


# ------------------------------------------------------------------------------- 5. plan output through offsets
def test_plan_output_windows_through_frame_offsets():
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
    wins = [(10, 20, 50, 100), (100, 200, 100, 400), (250, 500, 50, 160)]
    sel0 = [_frames(tiles[0], wdw, 4096) for wdw in wins]  # frames of tile 0 per window
    assert sel0 == [(0, 3), (6, 12), None]
    ctx = _ctx()
    plan = N.Plan(ctx, r.ctypes.data, False, r.dtype, B, (H * W, W, 1), tiles, 5, 4096, 16, keepalive=r)
    dev = ctx.alloc(max(B * h * w * 2 for _, _, h, w in wins))

    def check(wdw):
        y, x, h, w = wdw
        ctx.h2d(dev, np.zeros(B * h * w, np.int16))
        infos = read_window_on_device(plan, wdw, dev)
        got = np.empty((B, h, w), np.int16)
        ctx.d2h(got, dev)
        assert np.array_equal(got, want[:, y:y + h, x:x + w]), wdw
        for t, inf in zip(tiles, infos):
            fr = _frames(t, wdw, 4096)
            assert inf.nframes == (0 if fr is None else fr[1] - fr[0] + 1)

    try:
        plan.execute()
        plan.sync()
        for wdw in wins:
            check(wdw)
        infos, frames = plan.download()
        off = plan.frame_offsets(sum(i.nframes for i in infos))
        ptr, _ = plan.device_output()
        bad = np.frombuffer(frames, np.uint8).copy()
        bad[int(off[16]) + 40] ^= 0x20  # frame 16 of tile 0: no window selects it
        ctx.h2d(ptr, bad)
        for wdw in wins:
            check(wdw)
        bad[int(off[2]) + 40] ^= 0x20  # frame 2 of tile 0: the first window selects it
        ctx.h2d(ptr, bad)
        with pytest.raises(N.NativeError, match=f"corrupt frame at byte {int(off[2]) - infos[0].offset}"):
            read_window_on_device(plan, wins[0], dev)
        check(wins[2])
    finally:
        ctx.free(dev)
        plan.close()


# ------------------------------------------------------------------------------- 6. refusals and short streams
def test_refusals_short_streams_and_damage_on_the_search_path():
    rng = np.random.default_rng(41)
    sig = _smooth(10 * 16, 1, 16, rng)
    s, fb, _ = O.encode(sig, 44100, level=5, blocksize=16, return_info=True)
    want, _ = N.decode(s)
    want = want.reshape(10, 16)
    ctx = _ctx()

    def read(stream, tile, roi):
        dst = np.full((roi[2], roi[3]), SENTINEL, np.int16)
        ctx.decode_device_window(stream, [{"offset": 0, "bytes": len(stream), "window": tile}], dst, np.int16, 1,
                                 (dst.size, roi[3], 1), roi)
        return dst

    # STREAMINFO minimum block size (bytes 8..9) patched to differ from the maximum
    assert s[8:10] == s[10:12] == (16).to_bytes(2, "big")
    with pytest.raises(N.NativeError, match="fixed-blocksize"):
        read(s[:8] + (15).to_bytes(2, "big") + s[10:], (0, 0, 10, 16), (2, 0, 3, 16))
    # the item claims 14 rows, the stream holds 10
    with pytest.raises(N.NativeError, match="ends before the window"):
        read(s, (0, 0, 14, 16), (11, 0, 2, 16))
    with pytest.raises(N.NativeError, match="ends before the window"):
        read(s, (0, 0, 14, 16), (8, 0, 4, 16))
    assert np.array_equal(read(s, (0, 0, 14, 16), (2, 3, 4, 9)), want[2:6, 3:12])
    # a damaged selected frame (frame 3), and the same damage outside the selection
    pos = 86 + int(fb[:3].sum()) + int(fb[3]) // 2
    e = bytearray(s)
    e[pos] ^= 0x04
    with pytest.raises(N.NativeError):
        N.decode(bytes(e))
    with pytest.raises(N.NativeError):
        read(bytes(e), (0, 0, 10, 16), (2, 0, 4, 16))
    assert np.array_equal(read(bytes(e), (0, 0, 10, 16), (5, 0, 4, 16)), want[5:9])
    # (decode_device_window has no concat argument: the flag reaches the entry through the job)
    job, infos, keep = ctx._decode_job(s, [{"offset": 0, "bytes": len(s), "window": (0, 0, 10, 16)}],
                                       np.zeros(160, np.int16), np.int16, N.DENORM_NONE, 1, (160, 16, 1), concat=True)
    with pytest.raises(N.NativeError, match="CONCAT|concat"):
        ctx._decode_run("fra_decode_device_window", job, infos, keep, N._window_ref((0, 0, 2, 16)), infos)
    # the context decodes a good stream afterwards
    assert np.array_equal(read(s, (0, 0, 10, 16), (0, 0, 10, 16)), want)
