"""GPU tests of the device decoder (``fra_decode_device``: k_dec_parse / k_dec_restore / k_dec_scatter).

Every comparison is bit-exact.  The expectation is the host decoder ``fra_decode`` for samples and numpy's
``denormalize_from_audio`` / ``pcm16_float`` for rasters -- never the device path itself.  Every hand-built stream is
accepted (or rejected) by the host decoder first.
"""
import numpy as np
import pytest

import oracle as O
from flac_raster import _native as N
from flac_raster.decoder import decode_flac, pcm16_float
from flac_raster.geo import Affine
from flac_raster.normalization import NormalizationParams, denormalize_from_audio
from flac_raster.tiff import read_geotiff

pytestmark = pytest.mark.gpu


def _ctx():
    return N.default_context(0)


def _hw(n):
    """A window (height, width) of exactly n samples, as square as n's factors allow."""
    h = int(np.sqrt(n))
    while h > 1 and n % h:
        h -= 1
    return max(h, 1), n // max(h, 1)


def _decode_many(streams, dtype, concat=False):
    """One fra_decode_device call over ``streams`` (same channel count): their windows are stacked in a destination
    with padding between rows and bands.  Returns the per-stream ``(N, C)`` arrays cut from the destination, and checks
    that nothing outside the windows was written."""
    host = [N.decode(s, concat=concat) for s in streams]
    C_ = host[0][1].channels
    wins, row = [], 2
    for x, _ in host:
        h, w = _hw(x.shape[0])
        wins.append((row, 3, h, w))
        row += h + 1
    row_stride = max(w for _, _, _, w in wins) + 3 + 7
    band_stride = row * row_stride + 11
    sentinel = -12345
    dst = np.full(C_ * band_stride, sentinel, dtype=dtype)
    blob = b"\x00" * 5 + b"".join(s + b"\x00\x00\x00" for s in streams)  # unaligned starts, gaps between streams
    items, off = [], 5
    for s, wdw in zip(streams, wins):
        items.append({"offset": off, "bytes": len(s), "window": wdw})
        off += len(s) + 3
    infos = _ctx().decode_device(blob, items, dst, dtype, C_, (band_stride, row_stride, 1), N.DENORM_NONE, concat)
    bands = [dst[c * band_stride:c * band_stride + row * row_stride].reshape(row, row_stride) for c in range(C_)]
    mask = np.ones((row, row_stride), bool)
    out = []
    for (r, c, h, w), (x, hi), di in zip(wins, host, infos):
        mask[r:r + h, c:c + w] = False
        out.append(np.stack([b[r:r + h, c:c + w].reshape(-1) for b in bands], axis=1))
        assert (di.channels, di.bps, di.nframes, di.nsamples, di.nstreams) == (
            hi.channels, hi.bps, hi.nframes, hi.nsamples, hi.nstreams)
    for b in bands:
        assert (b[mask] == sentinel).all(), "written outside the windows"
    assert (dst.reshape(C_, band_stride)[:, row * row_stride:] == sentinel).all()
    return out, [x for x, _ in host]


# ------------------------------------------------------------------------------- 1. oracle streams
def _signal(kind, n, ch, bps, rng):
    if kind == "noise":  # full scale: VERBATIM
        if bps == 16:
            return rng.integers(-32768, 32768, size=(n, ch)).astype(np.int16)
        return rng.integers(-2**31, 2**31, size=(n, ch), dtype=np.int64).astype(np.int32)
    if kind == "const":
        return np.full((n, ch), -1234 if bps == 16 else -123456789, np.int16 if bps == 16 else np.int32)
    if kind == "wasted":
        return (rng.integers(-100, 100, size=(n, ch)) * 64).astype(np.int16 if bps == 16 else np.int32)
    if kind == "extreme":
        a = np.where((np.arange(n)[:, None] + np.arange(ch)[None]) % 3 == 0, -32768, 32767)
        return a.astype(np.int16) if bps == 16 else (a.astype(np.int64) * 65536).clip(-2**31, 2**31 - 1).astype(np.int32)
    amp = 300 if bps == 16 else 3_000_000
    lim = 32767 if bps == 16 else 2**31 - 1
    walk = np.cumsum(rng.integers(-amp, amp, size=(n, 1)), axis=0)
    x = walk + rng.integers(-amp // 10, amp // 10, size=(n, ch)) + 37 * np.arange(ch)[None]  # correlated channels
    return x.clip(-lim - 1, lim).astype(np.int16 if bps == 16 else np.int32)


# (level, blocksize, samples, signal): lengths 1, 15, a frame + 1, 70 frames of 16 with a partial last one (crosses
# the 64-frame lane group), 130 frames of 192; every level and block size of the issue
CASES = [
    (0, 16, 1, "smooth"), (2, 16, 15, "smooth"), (5, 16, 69 * 16 + 6, "smooth"), (8, 16, 17, "smooth"),
    (8, 192, 130 * 192, "smooth"), (2, 192, 193, "smooth"), (5, 1152, 1153, "smooth"), (0, 1152, 3000, "smooth"),
    (8, 4096, 4097, "smooth"), (5, 4096, 9000, "smooth"), (2, 4096, 5000, "noise"), (5, 192, 400, "const"),
    (5, 4096, 5000, "wasted"), (8, 1152, 2500, "extreme"), (0, 192, 500, "noise"),
]


@pytest.mark.parametrize("bps", [16, 32])
@pytest.mark.parametrize("ch", [1, 2, 3, 4, 8])
def test_oracle_streams_equal_host_decoder(ch, bps):
    rng = np.random.default_rng(100 * ch + bps)
    streams = [O.encode(_signal(kind, n, ch, bps, rng), 44100, level=lvl, blocksize=bs) for lvl, bs, n, kind in CASES]
    got, want = _decode_many(streams, np.int16 if bps == 16 else np.int32)
    for g, w, case in zip(got, want, CASES):
        assert g.shape == w.shape and np.array_equal(g.astype(np.int32), w), case
    if bps == 16:  # <= 16-bps streams may also go to an int32 destination
        got32, _ = _decode_many(streams[:4], np.int32)
        assert all(np.array_equal(g, w) for g, w in zip(got32, want))


def test_int16_destination_refused_for_32_bps():
    s = O.encode(np.arange(40, dtype=np.int32).reshape(-1, 1) * 100000, 44100)
    dst = np.zeros(40, np.int16)
    with pytest.raises(N.NativeError, match="FRA_I32"):
        _ctx().decode_device(s, [{"offset": 0, "bytes": len(s), "window": (0, 0, 1, 40)}], dst, np.int16, 1,
                             (40, 40, 1))
    with pytest.raises(N.NativeError, match="samples per channel"):
        _ctx().decode_device(s, [{"offset": 0, "bytes": len(s), "window": (0, 0, 1, 39)}], np.zeros(40, np.int32),
                             np.int32, 1, (40, 40, 1))


# ------------------------------------------------------------------------------- 2. libFLAC's own output
def test_libflac_golden_files(golden_dir):
    d = (golden_dir / "sample_rgb.flac").read_bytes()
    want, hinfo = N.decode(d)
    assert (hinfo.nframes, hinfo.channels) == (16, 3)
    got, sr, bps = decode_flac(d, device=0)
    assert (got.dtype, sr, bps) == (np.int16, 44100, 16)
    assert np.array_equal(got.astype(np.int32), want)
    (g2,), _ = _decode_many([d], np.int16)
    assert np.array_equal(g2.astype(np.int32), want)

    dem = (golden_dir / "sample_dem.flac").read_bytes()
    with pytest.raises(N.NativeError, match="lost sync"):
        decode_flac(dem, device=0)
    x, _, bps = decode_flac(dem, concat=True, device=0)
    assert bps == 32 and x.shape == (262144, 1) and not x.any()
    (g3,), (w3,) = _decode_many([dem], np.int32, concat=True)  # (asserts nstreams == the host's 4)
    assert np.array_equal(g3, w3)


# ------------------------------------------------------------------------------- 3. hand-built frames
class Bits:
    def __init__(self):
        self.b = []

    def put(self, v, n):
        v &= (1 << n) - 1
        self.b.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def unary(self, q):
        self.b.extend([0] * q + [1])

    def rice(self, v, k):
        u = (v << 1) if v >= 0 else ((-v << 1) - 1)
        self.unary(u >> k)
        if k:
            self.put(u & ((1 << k) - 1), k)

    def bytes(self):
        b = self.b + [0] * (-len(self.b) % 8)
        return bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))


def _frame(bs, assign, bps, number, body: Bits) -> bytes:
    h = Bits()
    h.put(0xFFF8, 16)
    h.put(12 if bs == 4096 else (6 if bs <= 256 else 7), 4)
    h.put(9, 4)  # 44.1 kHz
    h.put(assign, 4)
    h.put({16: 4, 32: 7}[bps], 3)
    h.put(0, 1)
    assert number < 128
    h.put(number, 8)
    if bs != 4096:
        h.put(bs - 1, 8 if bs <= 256 else 16)
    fh = h.bytes()
    f = fh + bytes([O.crc8(fh)]) + body.bytes()
    return f + O.crc16(f).to_bytes(2, "big")


def _both(stream: bytes):
    """Host decoder first (must accept), then the device; returns (device, host)."""
    want, _ = N.decode(stream)
    got, _, _ = decode_flac(stream, device=0)
    return got.astype(np.int32), want


def test_handbuilt_escaped_partition():
    b = Bits()
    b.put(0, 1); b.put(9, 6); b.put(0, 1)  # FIXED order 1
    b.put(1000, 16)
    b.put(0, 2); b.put(0, 4); b.put(15, 4); b.put(5, 5)  # RICE, partition order 0, escape, raw 5-bit residuals
    res = [3, -4, 15, -16, 0, 7, -7, 1, -1, 2, -2, 9, -9, 5, -5]
    for r in res:
        b.put(r, 5)
    got, want = _both(N.stream_header(1, 16, 44100, 16) + _frame(16, 0, 16, 0, b))
    assert np.array_equal(want[:, 0], 1000 + np.concatenate([[0], np.cumsum(res)]))
    assert np.array_equal(got, want)


def test_handbuilt_rice2_large_parameter():
    rng = np.random.default_rng(7)
    res = rng.integers(-2**26, 2**26, size=32)
    b = Bits()
    b.put(0, 1); b.put(8, 6); b.put(0, 1)  # FIXED order 0, 32 bps
    b.put(1, 2); b.put(1, 4)               # RICE2, partition order 1
    for part, k in ((res[:16], 25), (res[16:], 19)):
        b.put(k, 5)
        for r in part:
            b.rice(int(r), k)
    got, want = _both(N.stream_header(1, 32, 44100, 32) + _frame(32, 0, 32, 0, b))
    assert np.array_equal(want[:, 0], res) and np.array_equal(got, want)


def test_handbuilt_lpc_order_32_precision_15():
    rng = np.random.default_rng(8)
    n, order, shift = 256, 32, 14
    coef = [int(v) for v in rng.integers(-1, 2, size=32)]  # |coefficients| sum to ~1.0 * 2^14: a stable predictor
    coef[0], coef[3], coef[17], coef[31] = 10240, 2048, -2048, -2048
    warm = [int(v) for v in rng.integers(-40, 40, size=order)]
    warm[0] = 0
    res = [int(v) for v in rng.integers(-6, 7, size=n - order)]
    b = Bits()
    b.put(0, 1); b.put(31 + order, 6); b.put(0, 1)
    for w in warm:
        b.put(w, 16)
    b.put(14, 4); b.put(shift, 5)
    for c in coef:
        b.put(c, 15)
    b.put(0, 2); b.put(2, 4)  # RICE, 4 partitions of 64
    i = 0
    for p in range(4):
        cnt = 64 - order if p == 0 else 64
        b.put(3, 4)
        for r in res[i:i + cnt]:
            b.rice(r, 3)
        i += cnt
    # the expected samples, by the format's definition (floored shift)
    s = list(warm)
    for j, r in enumerate(res):
        acc = sum(coef[t] * s[-1 - t] for t in range(order))
        s.append((acc >> shift) + r)
    assert max(abs(v) for v in s) < 32768, "test vector leaves the 16-bit range"
    got, want = _both(N.stream_header(1, 16, 44100, n) + _frame(n, 0, 16, 0, b))
    assert np.array_equal(want[:, 0], s) and np.array_equal(got, want)


def test_handbuilt_partition_order_8():
    rng = np.random.default_rng(9)
    n = 4096
    res = rng.integers(-3, 4, size=n - 1)
    b = Bits()
    b.put(0, 1); b.put(9, 6); b.put(0, 1)  # FIXED order 1
    b.put(-77, 16)
    b.put(0, 2); b.put(8, 4)  # 256 partitions of 16 samples, the first holds 15 residuals
    i = 0
    for p in range(256):
        k = p % 5
        cnt = 15 if p == 0 else 16
        b.put(k, 4)
        for r in res[i:i + cnt]:
            b.rice(int(r), k)
        i += cnt
    got, want = _both(N.stream_header(1, 16, 44100, n) + _frame(n, 0, 16, 0, b))
    assert np.array_equal(want[:, 0], -77 + np.concatenate([[0], np.cumsum(res)]))
    assert np.array_equal(got, want)


def test_handbuilt_false_candidate_inside_a_frame():
    """A VERBATIM frame whose samples spell a complete frame header with a valid CRC-8: the chain steps over it."""
    fake = bytes([0xFF, 0xF8, 0x69, 0x08, 0x00, 0x0F])  # mono 16-bit, 8-bit block size code: 16 samples
    fake += bytes([O.crc8(fake)]) + b"\x00"
    assert len(fake) % 2 == 0
    smp = [int.from_bytes(fake[i:i + 2], "big", signed=True) for i in range(0, len(fake), 2)]
    smp = [5, -6] + smp + [100, -200, 300, -400, 500, -600, 700, -800, 900, -1000]
    assert len(smp) == 16
    frames = b""
    for k in range(3):
        b = Bits()
        b.put(0, 1); b.put(1, 6); b.put(0, 1)  # VERBATIM
        for v in smp:
            b.put(v, 16)
        frames += _frame(16, 0, 16, k, b)
    assert frames.count(fake[:7]) == 4  # frame 0's own header and one copy inside every frame
    got, want = _both(N.stream_header(1, 16, 44100, 16) + frames)
    assert want.shape == (48, 1) and np.array_equal(got, want)


def test_handbuilt_out_of_range_reconstruction_is_rejected():
    b = Bits()
    b.put(0, 1); b.put(9, 6); b.put(0, 1); b.put(32767, 16)
    b.put(0, 2); b.put(0, 4); b.put(15, 4); b.put(17, 5)
    for _ in range(15):
        b.put(65535, 17)
    stream = N.stream_header(1, 16, 44100, 16) + _frame(16, 0, 16, 0, b)
    with pytest.raises(N.NativeError):
        N.decode(stream)
    with pytest.raises(N.NativeError, match="sample range"):
        decode_flac(stream, device=0)


# ------------------------------------------------------------------------------- 4. corruption and truncation
def test_corruption_and_truncation_raise(golden_dir):
    """Each damaged stream ends in an error return because every read and loop of the kernels is bounded."""
    d = bytearray((golden_dir / "sample_rgb.flac").read_bytes())
    for pos in (200, 50000, len(d) - 3):
        e = bytearray(d)
        e[pos] ^= 0x04
        with pytest.raises(N.NativeError):
            N.decode(bytes(e))
        with pytest.raises(N.NativeError):
            decode_flac(bytes(e), device=0)
    with pytest.raises(N.NativeError):
        decode_flac(bytes(d[:-100]), device=0)
    # the context still decodes afterwards
    got, _, _ = decode_flac(bytes(d), device=0)
    assert np.array_equal(got.astype(np.int32), N.decode(bytes(d))[0])


# ------------------------------------------------------------------------------- 5. supplied offsets
def test_plan_output_decoded_through_frame_offsets():
    from flac_raster.tiles import verify_on_device

    rng = np.random.default_rng(11)
    B, H, W = 4, 300, 660
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(3000 + 900 * np.sin(yy / 17.0 + b) + 700 * np.cos(xx / 29.0) + rng.integers(0, 60, (H, W)))
                  for b in range(B)]).astype(np.uint16)
    wins = [(0, 0, 300, 260), (0, 260, 300, 260), (0, 520, 300, 140)]  # the last one ragged
    want = np.zeros((B, H, W), np.int16)
    for (y, x, h, w) in wins:
        audio, _, _ = O.normalize(r[:, y:y + h, x:x + w].transpose(1, 2, 0).reshape(-1, B), 16)
        want[:, y:y + h, x:x + w] = audio.reshape(h, w, B).transpose(2, 0, 1)
    ctx = _ctx()
    plan = N.Plan(ctx, r.ctypes.data, False, r.dtype, B, (H * W, W, 1), wins, 5, 4096, 16, keepalive=r)
    dev = ctx.alloc(want.nbytes)
    try:
        plan.execute()
        plan.sync()
        ctx.h2d(dev, np.zeros_like(want))
        assert verify_on_device(plan, dev) is True
        got = np.empty_like(want)
        ctx.d2h(got, dev)
        assert np.array_equal(got, want)
        # the same bytes as complete streams through the search path
        infos, frames = plan.download()
        blob, items = b"", []
        for inf, wdw in zip(infos, wins):
            s = N.stream_header(inf.channels, inf.bps, inf.sample_rate) + frames[inf.offset:inf.offset + inf.frame_bytes]
            items.append({"offset": len(blob), "bytes": len(s), "window": wdw})
            blob += s
        got2 = np.zeros_like(want)
        ctx.decode_device(blob, items, got2, np.int16, B, (H * W, W, 1))
        assert np.array_equal(got2, want)
        # a damaged frame fails the offsets path with the frame's position
        off = plan.frame_offsets(sum(i.nframes for i in infos))
        ptr, _ = plan.device_output()
        bad = np.frombuffer(frames, np.uint8).copy()
        bad[int(off[3]) + 40] ^= 0x20
        ctx.h2d(ptr, bad)
        with pytest.raises(N.NativeError, match=f"corrupt frame at byte {int(off[3]) - infos[0].offset}"):
            verify_on_device(plan, dev)
    finally:
        ctx.free(dev)
        plan.close()


def test_streams_resident_on_the_device_without_offsets():
    """The search path with the input on the device (the library fetches the bytes for the candidate search) and a
    pixel-interleaved destination (col_stride = channels)."""
    rng = np.random.default_rng(14)
    a = _signal("smooth", 70 * 192 + 5, 3, 16, rng)
    s = O.encode(a, 44100, level=5, blocksize=192)
    want, _ = N.decode(s)
    ctx = _ctx()
    buf = np.frombuffer(b"\x00" * 3 + s, np.uint8)
    dev = ctx.alloc(buf.size)
    try:
        ctx.h2d(dev, buf)
        h, w = _hw(a.shape[0])
        got = np.full((h, w + 2, 3), 77, np.int16)  # (row, col, band) with two spare columns per row
        ctx.decode_device((dev, buf.size), [{"offset": 3, "bytes": len(s), "window": (0, 1, h, w)}], got, np.int16, 3,
                          (1, (w + 2) * 3, 3))
    finally:
        ctx.free(dev)
    assert np.array_equal(got[:, 1:w + 1, :].reshape(-1, 3).astype(np.int32), want)
    assert (got[:, 0, :] == 77).all() and (got[:, w + 1, :] == 77).all()


# ------------------------------------------------------------------------------- 6. denormalisation
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]


def _tile_of(dt, rng, h, w, B):
    dt = np.dtype(dt)
    if dt.kind == "f":
        a = (rng.normal(0.3, 0.2, size=(B, h, w)) * 1000).astype(dt)
        a[0, 3, 4] = np.nan
        return a
    lo, hi = {1: (10, 200), 2: (300, 60000), 4: (1000, 2_000_000_000)}[dt.itemsize]
    if dt.kind == "i":
        lo, hi = -hi // 2, hi // 2
    return rng.integers(lo, hi, size=(B, h, w)).astype(dt)


@pytest.mark.parametrize("mode", ["int", "pcm16"])
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_denormalisation_equals_numpy(dt, mode):
    dt = np.dtype(dt)
    rng = np.random.default_rng(dt.itemsize * 10 + (dt.kind == "f"))
    B, h, w = 2, 37, 53
    tiles = [_tile_of(dt, rng, h, w, B)]
    if dt.kind == "f":
        tiles.append(np.full((B, h, w), 2.5, dt))  # a constant tile: data_max == data_min
    bits = 16 if dt.itemsize <= 2 and dt.kind != "f" else 24
    blob, items, want = b"", [], []
    for k, t in enumerate(tiles):
        audio, mn, mx = O.normalize(t.transpose(1, 2, 0).reshape(-1, B), bits)
        s = O.encode(audio, 44100, level=5)
        ints, info = N.decode(s)
        assert info.bps == (16 if bits == 16 else 32)
        p = NormalizationParams(float(mn), float(mx), dt.name, bits, 32767 if bits == 16 else 8388607)
        ints = ints.astype(np.int16) if bits == 16 else ints
        x = denormalize_from_audio(ints if mode == "int" else pcm16_float(ints), p)
        want.append(x.reshape(h, w, B).transpose(2, 0, 1))
        items.append({"offset": len(blob), "bytes": len(s), "window": (k * h, 0, h, w), "data_min": float(mn),
                      "data_max": float(mx)})
        blob += s
    want = np.concatenate(want, axis=1)
    got = np.zeros((B, len(tiles) * h, w), dt)
    _ctx().decode_device(blob, items, got, dt, B, (got.shape[1] * w, w, 1),
                         N.DENORM_INT if mode == "int" else N.DENORM_PCM16)
    assert got.dtype == want.dtype
    assert np.array_equal(got, want, equal_nan=dt.kind == "f")
    if dt.kind == "f" and mode == "int":
        assert np.isfinite(got).all() and (got[:, h:] == 2.5).all()


# ------------------------------------------------------------------------------- 7. container round trip
def test_container_round_trip_and_cli(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.streaming import build_streaming, streaming_to_raster

    rng = np.random.default_rng(12)
    H, W = 700, 900
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(20000 + 9000 * np.sin(yy / 41.0 + b) + 8000 * np.cos(xx / 53.0) + rng.integers(0, 400, (H, W)))
                  for b in range(3)]).astype(np.uint16)
    data = build_streaming(r, Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0), "EPSG:32633", 256)
    for sem in ("pcm16", "int"):
        host, idx = streaming_to_raster(data, device=None, semantics=sem)
        dev, _ = streaming_to_raster(data, device=0, semantics=sem)
        assert host.dtype == np.uint16 and host.shape == r.shape and len(idx["frames"]) == 12
        assert np.array_equal(dev, host), sem
    pcm, _ = streaming_to_raster(data, device=None)
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    out = tmp_path / "scene.tif"
    res = CliRunner().invoke(app, ["convert", str(src), "-o", str(out)])
    assert res.exit_code == 0, res.output
    px, info = read_geotiff(out)
    assert np.array_equal(px, pcm) and "32633" in str(info.crs)


# ------------------------------------------------------------------------------- 8. a refused stream
def test_32_bps_mid_side_is_decoded_or_refused():
    rng = np.random.default_rng(13)
    mid = rng.integers(-2**31, 2**31, size=16)
    side = rng.integers(-2**31, 2**31, size=16) * 2 + 1  # odd: 33 bits
    side = np.clip(side, -2**32, 2**32 - 1)
    b = Bits()
    b.put(0, 1); b.put(1, 6); b.put(0, 1)
    for v in mid:
        b.put(int(v), 32)
    b.put(0, 1); b.put(1, 6); b.put(0, 1)
    for v in side:
        b.put(int(v), 33)
    stream = N.stream_header(2, 32, 44100, 16) + _frame(16, 10, 32, 0, b)
    want, info = N.decode(stream)  # the host decoder accepts it
    assert info.bps == 32 and want.shape == (16, 2)
    try:
        got, _, _ = decode_flac(stream, device=0)
    except N.NativeError as e:
        assert "not supported on the device" in str(e)
    else:
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------- 9. what the entries' host code keeps
def _verbatim_stream(samples, bps=16):
    """A hand-built stream of VERBATIM frames of 16 samples over ``samples`` (n, channels), n a multiple of 16;
    returns (stream, offsets of the frames and of the stream's end)."""
    x = np.asarray(samples)
    n, ch = x.shape
    assert n % 16 == 0 and ch in (1, 2)
    stream, offs = N.stream_header(ch, bps, 44100, 16), []
    for f in range(n // 16):
        b = Bits()
        for c in range(ch):
            b.put(0, 1); b.put(1, 6); b.put(0, 1)
            for v in x[16 * f:16 * f + 16, c]:
                b.put(int(v), bps)
        offs.append(len(stream))
        stream += _frame(16, ch - 1, bps, f, b)
    return stream, np.array(offs + [len(stream)], np.uint64)


def _out_of_range_stream():
    b = Bits()
    b.put(0, 1); b.put(9, 6); b.put(0, 1); b.put(32767, 16)
    b.put(0, 2); b.put(0, 4); b.put(15, 4); b.put(17, 5)
    for _ in range(15):
        b.put(65535, 17)
    return N.stream_header(1, 16, 44100, 16), _frame(16, 0, 16, 0, b)


def _on_device(ctx, blob, run):
    """run((device pointer, length)) with ``blob`` resident on the device."""
    buf = np.frombuffer(blob, np.uint8)
    dev = ctx.alloc(buf.size)
    try:
        ctx.h2d(dev, buf)
        return run((dev, buf.size))
    finally:
        ctx.free(dev)


def test_out_of_range_frame_of_a_second_item_is_named_by_its_byte():
    """The frame whose reconstruction leaves the sample range, in the second of two items: the full decode names its
    byte in ``data``, the windowed read its byte in the item."""
    good, _ = _verbatim_stream(np.arange(16).reshape(-1, 1))
    head, frame = _out_of_range_stream()
    blob = b"\x00" * 5 + good + b"\x00" * 3 + head + frame
    off = 5 + len(good) + 3
    items = [{"offset": 5, "bytes": len(good), "window": (0, 0, 1, 16)},
             {"offset": off, "bytes": len(head) + len(frame), "window": (1, 0, 1, 16)}]
    ctx = _ctx()
    dst = np.zeros((2, 16), np.int16)
    with pytest.raises(N.NativeError, match=rf"sample range \(frame at byte {off + len(head)}\)"):
        ctx.decode_device(blob, items, dst, np.int16, 1, (32, 16, 1))

    def window(data):
        return ctx.decode_device_window(data, items, dst, np.int16, 1, (32, 16, 1), (0, 0, 2, 16))

    with pytest.raises(N.NativeError, match=rf"sample range \(frame at byte {len(head)}\)"):
        window(blob)
    with pytest.raises(N.NativeError, match=rf"sample range \(frame at byte {len(head)}\)"):
        _on_device(ctx, blob, window)


@pytest.mark.parametrize("interleaved", [False, True], ids=["rows", "interleaved"])
@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
def test_window_over_an_offsets_item_a_searched_item_and_one_outside(resident, interleaved):
    """Three 8 x 8 tiles of four frames: A through frame offsets, B searched, C outside the region and not FLAC."""
    rng = np.random.default_rng(91)
    sa, offs = _verbatim_stream(rng.integers(-3000, 3000, size=(64, 1)))
    sb, _ = _verbatim_stream(rng.integers(-3000, 3000, size=(64, 1)))
    sc = b"these bytes are no FLAC stream " * 3
    full = np.full((16, 16), -12345, np.int32)
    full[:8, :8] = N.decode(sa)[0].reshape(8, 8)
    full[:8, 8:] = N.decode(sb)[0].reshape(8, 8)
    blob = b"\x00" * 5 + sa + b"\x00" * 3 + sb + b"\x00" * 3 + sc
    ob = 5 + len(sa) + 3
    items = [{"offset": 5, "bytes": len(sa), "window": (0, 0, 8, 8), "frame_offsets": offs, "channels": 1, "bps": 16,
              "blocksize": 16},
             {"offset": ob, "bytes": len(sb), "window": (0, 8, 8, 8)},
             {"offset": ob + len(sb) + 3, "bytes": len(sc), "window": (8, 0, 8, 8)}]
    roi = (2, 3, 3, 10)  # tile samples 19..39 of A and 16..36 of B: frames 1 and 2 of each, cut at both ends
    r, c, h, w = roi
    if interleaved:  # (row, col, 2): the column stride is 2, so the destination is staged whole
        dst = np.full((h + 1, w + 2, 2), -12345, np.int16)
        strides, view = (1, (w + 2) * 2, 2), dst[:, :, 0]
    else:
        dst = np.full((h + 1, w + 3), -12345, np.int16)
        strides, view = (dst.size, w + 3, 1), dst
    ctx = _ctx()

    def window(data):
        return ctx.decode_device_window(data, items, dst, np.int16, 1, strides, roi)

    infos = _on_device(ctx, blob, window) if resident else window(blob)
    assert np.array_equal(view[:h, :w], full[r:r + h, c:c + w])
    view[:h, :w] = -12345
    assert (dst == -12345).all(), "written outside the intersections"
    assert [(i.nframes, i.nsamples, i.channels, i.bps, i.blocksize) for i in infos[:2]] == [(2, 15, 1, 16, 16)] * 2
    z = infos[2]
    assert all(getattr(z, name) == 0 for name, _ in N.Decoded._fields_), "infos of an item outside the region"


def test_channel_count_is_refused_before_the_32_bps_destination():
    """A two-channel 32-bps stream into one int16 band breaks two rules: the channel count is named, by both entries."""
    s, _ = _verbatim_stream(np.arange(32).reshape(-1, 2) * 100000, bps=32)
    assert N.decode(s)[1].bps == 32
    items = [{"offset": 0, "bytes": len(s), "window": (0, 0, 1, 16)}]
    dst = np.zeros(16, np.int16)
    with pytest.raises(N.NativeError, match="item 0 has 2 channels, the destination 1"):
        _ctx().decode_device(s, items, dst, np.int16, 1, (16, 16, 1))
    with pytest.raises(N.NativeError, match="item 0 has 2 channels, the destination 1"):
        _ctx().decode_device_window(s, items, dst, np.int16, 1, (16, 16, 1), (0, 0, 1, 16))


def test_capacity_window_too_small_reports_the_samples_needed():
    s, _ = _verbatim_stream(np.arange(48).reshape(-1, 1))
    with pytest.raises(N.OutputTooSmall) as e:
        _ctx().decode_device(s, [{"offset": 0, "bytes": len(s), "window": (0, 0, -40, 1)}], np.zeros(40, np.int16),
                             np.int16, 1, (40, 1, 1))
    assert e.value.needed == 48
