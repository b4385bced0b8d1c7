"""GPU tests of verify mode (``fra_plan_verify``: k_dec_parse / k_dec_restore / k_dec_verify over a plan's own frames).

Every expectation comes from the oracle's ``normalize_to_audio`` with the tile's own min / max as overrides, never
from the device path: ``expected`` is the normalised value the test wrote over a pixel, ``got`` the normalised value
that was encoded.  Rasters are small: 300 rows, tiles of 300 x 260 (19 full frames and a partial one) and a ragged
tile of 140 columns, as ``test_plan_output_decoded_through_frame_offsets`` uses.
"""
import numpy as np
import pytest

import oracle as O
from flac_raster import _native as N
from flac_raster.tiles import encode_tiles, frames_of, mismatch_pixel, norm_bits

pytestmark = pytest.mark.gpu

H, W = 300, 924
WINS = [(0, 0, 300, 260), (0, 260, 300, 260), (0, 520, 300, 140), (0, 660, 300, 260)]  # columns 920..923 uncovered
BS = 4096


def _ctx():
    return N.default_context(0)


def _raster(dtype, B, seed=11, h=H, w=W):
    """Smooth bands + noise; integers span ~3300 counts (so neighbouring values give distinct samples), floats ~0.8."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    r = np.stack([3000 + 900 * np.sin(yy / 17.0 + b) + 700 * np.cos(xx / 29.0) + rng.integers(0, 60, (h, w))
                  for b in range(B)])
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (r / 4000.0).astype(dt)
    if dt.itemsize == 1:
        return (r / 20.0 - (128 if dt.kind == "i" else 0)).astype(dt)
    if dt.kind == "i":
        r = r - 3000
    if dt.itemsize == 4:
        r = r * 50000
    return r.astype(dt)


def _clean(reports, wins, blocksize=BS, ranges=None):
    for k, (rep, w) in enumerate(zip(reports, wins)):
        n = frames_of(w, blocksize)
        if ranges is not None:
            f0, cnt = ranges[k]
            n = n - f0 if cnt < 0 else min(cnt, n - f0)
        assert (rep.mismatches, rep.first_sample, rep.first_channel, rep.expected, rep.got, rep.nframes) == (
            0, -1, 0, 0, 0, n), f"window {k}"


class _Resident:
    """A raster on the device, a plan over it, and pokes of single elements."""

    def __init__(self, r, wins, level, norm=None, strides=None, elem=None, frame_ranges=None, blocksize=BS):
        self.r, self.wins, self.ctx = r, wins, _ctx()
        self.flat = np.ascontiguousarray(r).reshape(-1)
        B = r.shape[0] if elem is None else elem[0]
        self.strides = strides or (r.shape[1] * r.shape[2], r.shape[2], 1)
        self.dev = self.ctx.alloc(self.flat.nbytes)
        self.plan = None
        try:
            self.ctx.h2d(self.dev, self.flat)
            self.plan = N.Plan(self.ctx, self.dev, True, r.dtype, B, self.strides, wins, level, blocksize,
                               norm_bits(r.dtype) if norm is None else norm, frame_ranges=frame_ranges)
        except BaseException:
            self.close()
            raise

    def element(self, band, row, col):
        return band * self.strides[0] + row * self.strides[1] + col * self.strides[2]

    def poke(self, band, row, col, value):
        e = self.element(band, row, col)
        self.ctx.h2d(self.dev + e * self.flat.itemsize, np.array([value], self.flat.dtype))

    def close(self):
        if self.plan is not None:
            self.plan.close()
        self.ctx.free(self.dev)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ------------------------------------------------------------------------------- 1. clean data verifies
def _with_nans(r):
    r = r.copy()
    r[:, 7, 5:40] = np.nan            # a run inside tile 0
    r[0, 100:103, 300:330] = np.nan   # one band of tile 1
    y, x, h, w = WINS[2]
    r[:, y:y + h, x:x + w] = np.nan   # an all-NaN tile
    y, x, h, w = WINS[3]
    r[:, y:y + h, x:x + w] = 0.25     # a constant tile
    return r


CLEAN = [  # dtype, bands, level, norm (None: the dtype's default)
    (np.uint8, 1, 0, None), (np.int8, 2, 5, None), (np.uint16, 4, 5, None), (np.int16, 2, 8, None),
    (np.uint32, 3, 0, None), (np.int32, 1, 5, None), (np.float32, 3, 8, None), (np.float64, 8, 5, None),
    (np.int16, 2, 5, 0), (np.int16, 1, 8, 0), (np.int32, 3, 8, 0), (np.uint16, 2, 8, None),
]


@pytest.mark.parametrize("dtype,B,level,norm", CLEAN,
                         ids=[f"{np.dtype(d).name}-b{b}-l{lv}-n{n}" for d, b, lv, n in CLEAN])
def test_clean_data_verifies(dtype, B, level, norm):
    r = _raster(dtype, B)
    if np.dtype(dtype).kind == "f":
        r = _with_nans(r)
    if norm == 0 and np.dtype(dtype) == np.int16:
        r = (r // 8 * 8).astype(np.int16)  # three wasted bits
        r[:, :, 660:920] = -1234           # a constant tile
    with _Resident(r, WINS, level, norm) as d:
        d.plan.execute()
        d.plan.sync()
        _clean(d.plan.verify(), WINS)
        infos, _ = d.plan.result()
        assert [i.nframes for i in infos] == [frames_of(w) for w in WINS]
        ms = d.ctx.decode_timing()
        assert ms[0] > 0 and ms[2] > 0 and ms[3] >= ms[0]  # parse, verify (slot 2), first kernel to last


# ------------------------------------------------------------------------------- 2. a changed pixel is found
def _tile_minmax(r, win):
    y, x, h, w = win
    return O.minmax(r[:, y:y + h, x:x + w])


def _sample(value, dtype, bps, mn, mx):
    return int(O.normalize(np.array([value], dtype), bps, mn, mx)[0][0])


def _poke_and_check(d, pokes, nan_at=(), extra=(), ranges=None, skip=()):
    """``pokes``: (tile, window-relative pixel, band).  Each is overwritten with another value inside its tile's
    min..max (NaN for those in ``nan_at``); ``extra``: raster (band, row, col) outside every window, overwritten too.
    ``skip``: pokes that lie outside the plan's frame ranges, written but not expected in a report."""
    r, wins = d.r, d.wins
    bps = norm_bits(r.dtype)
    step = 0.1 if r.dtype.kind == "f" else 500
    want = {}
    for pk in list(pokes) + list(skip):
        t, p, band = pk
        row, col, _ = mismatch_pixel(wins[t], p, 0)
        mn, mx = _tile_minmax(r, wins[t])
        old = r[band, row, col]
        new = np.nan if pk in nan_at else (old + step if old + step <= mx else old - step)
        new = np.array([new]).astype(r.dtype)[0]
        e, g = _sample(new, r.dtype, bps, mn, mx), _sample(old, r.dtype, bps, mn, mx)
        assert e != g, "the poke must change the sample"
        if pk in nan_at:
            assert e == 0
        d.poke(band, row, col, new)
        if pk not in skip:
            want.setdefault(t, []).append((p, band, e, g))
    for band, row, col in extra:
        d.poke(band, row, col, r[band, row, col] + (0.1 if r.dtype.kind == "f" else 500))
    reports = d.plan.verify()
    for t, (rep, w) in enumerate(zip(reports, wins)):
        if t not in want:
            _clean([rep], [w], ranges=None if ranges is None else [ranges[t]])
            continue
        p, band, e, g = min(want[t])
        assert (rep.mismatches, rep.first_sample, rep.first_channel, rep.expected, rep.got) == (
            len(want[t]), p, band, e, g), f"tile {t}"
    return reports


POKED = [(np.uint16, 4, 5), (np.float32, 3, 8), (np.uint16, 2, 5)]


@pytest.mark.parametrize("dtype,B,level", POKED, ids=[f"{np.dtype(d).name}-b{b}-l{lv}" for d, b, lv in POKED])
def test_a_changed_pixel_is_found(dtype, B, level):
    r = _raster(dtype, B, seed=12)
    last = 300 * 260 - 1  # the last sample of the partial last frame
    pokes = [(0, 0, 2 % B), (0, 4095, 1), (0, 4096, 3 % B),
             (1, last, B - 1), (1, last, 0),        # one pixel, two bands: the lower band is the first mismatch
             (2, 100 * 140 + 139, 1)]               # the ragged tile's last column
    nan_at = [(0, 4095, 1)] if np.dtype(dtype).kind == "f" else []
    with _Resident(r, WINS, level) as d:
        d.plan.execute()
        d.plan.sync()
        _clean(d.plan.verify(), WINS)
        reports = _poke_and_check(d, pokes, nan_at, extra=[(0, 5, 922)])
        assert reports[3].mismatches == 0
        # the frames themselves are untouched: the same raster again, and the report is clean again
        d.ctx.h2d(d.dev, d.flat)
        _clean(d.plan.verify(), WINS)


# ------------------------------------------------------------------------------- 3. layouts
def test_pixel_interleaved_and_padded_rows():
    B = 3
    r = _raster(np.uint16, B, seed=13)
    pokes = [(0, 4096, 2), (2, 100 * 140 + 139, 0), (3, 300 * 260 - 1, 1)]
    # pixel-interleaved: element (band, row, col) at row * W * B + col * B + band
    inter = np.ascontiguousarray(r.transpose(1, 2, 0))
    d = _Resident(inter[None], WINS, 5, strides=(1, W * B, B), elem=(B,))
    try:
        d.r = r  # (expectations index the band-planar copy)
        d.plan.execute()
        d.plan.sync()
        _clean(d.plan.verify(), WINS)
        _poke_and_check(d, pokes)
    finally:
        d.close()
    # band-planar with padded rows: row_stride > width
    Wp = W + 13
    pad = np.zeros((B, H, Wp), np.uint16)
    pad[:, :, :W] = r
    d = _Resident(pad, WINS, 5, strides=(H * Wp, Wp, 1))
    try:
        d.plan.execute()
        d.plan.sync()
        _clean(d.plan.verify(), WINS)
        _poke_and_check(d, pokes, extra=[(1, 3, W + 5)])
    finally:
        d.close()


# ------------------------------------------------------------------------------- 4. host paths
def test_after_encode_host_the_plans_copy_is_the_reference():
    r = _raster(np.int16, 2, seed=14)
    ctx = _ctx()
    plan = N.Plan(ctx, None, False, r.dtype, 2, (H * W, W, 1), WINS, 5, BS, 16)
    try:
        cap, _ = plan.capacity()
        out = np.empty(cap, np.uint8)
        total = plan.encode_host(r, out)
        assert total > 0
        _clean(plan.verify(), WINS)
        r[:] = 0  # the host raster may change afterwards: the plan's device copy is what is compared
        _clean(plan.verify(), WINS)
    finally:
        plan.close()


def test_after_encode_ring(monkeypatch):
    """A ring smaller than the raster (2048 frames: the host path cuts row bands): after the pass the plan's device
    copy holds the whole raster, and ``verify=True`` compares with it."""
    h, w, tile = 4096, 2048, 512
    r = _raster(np.uint16, 1, seed=15, h=h, w=w)
    wins = [(y, x, tile, tile) for y in range(0, h, tile) for x in range(0, w, tile)]
    seen = []
    real = N.Plan.verify

    def verify(self):
        reports = real(self)
        seen.append(reports)
        return reports

    monkeypatch.setattr(N.Plan, "verify", verify)

    def fill(dst, r0, r1):
        dst[...] = r[:, r0:r1, :]

    infos, frames, R = N.encode_windows_ring(r.shape, r.dtype, wins, fill, 5, BS, 16, verify=True)
    assert R < h and len(seen) == 1
    _clean(seen[0], wins)
    infos2, frames2, _ = N.encode_windows_ring(r.shape, r.dtype, wins, fill, 5, BS, 16)
    assert len(seen) == 1 and bytes(frames) == bytes(frames2)


# ------------------------------------------------------------------------------- 5. ranged plans
def test_ranged_plan_is_verified_over_its_own_frames():
    r = _raster(np.uint16, 4, seed=16)
    ranges = [(1, 2), (0, -1), (2, -1), (18, -1)]
    with _Resident(r, WINS, 5, frame_ranges=ranges) as d:
        d.plan.execute()
        d.plan.sync()
        _clean(d.plan.verify(), WINS, ranges=ranges)
        last = 300 * 260 - 1
        _poke_and_check(d, [(0, 4096, 1), (0, 3 * 4096 - 1, 0), (2, 100 * 140 + 139, 2), (3, last, 3), (3, 18 * 4096, 0)],
                        skip=[(0, 100, 0), (0, 3 * 4096, 2), (2, 0, 1), (3, 18 * 4096 - 1, 1)], ranges=ranges)


# ------------------------------------------------------------------------------- 6. pipelined plans
def test_pipelined_plan_and_a_second_raster():
    h = w = 2048
    tile = 512
    a = _raster(np.uint16, 1, seed=17, h=h, w=w)
    b = a.copy()
    y, x = 512, 1024  # tile 6 differs in 40 of its rows
    b[0, y + 100:y + 140, x:x + tile] += 9
    wins = [(yy, xx, tile, tile) for yy in range(0, h, tile) for xx in range(0, w, tile)]
    ctx = _ctx()
    dev_b = ctx.alloc(b.nbytes)
    try:
        ctx.h2d(dev_b, b)
        with _Resident(a, wins, 5) as d:
            assert d.plan.flags() & 2, "1024 frames: the plan pipelines its executes"
            for _ in range(3):
                d.plan.execute()
            _clean(d.plan.verify(), wins)
            d.plan.set_raster(dev_b, True)
            d.plan.execute()
            _clean(d.plan.verify(), wins)
            # the frames are b's; against raster a, tile 6 differs exactly where b's samples differ from a's
            d.plan.set_raster(d.dev, True)
            reports = d.plan.verify()
            mn, mx = _tile_minmax(b, wins[6])
            sa = O.normalize(a[0, y:y + tile, x:x + tile].reshape(-1, 1), 16, mn, mx)[0].reshape(-1)
            sb = O.normalize(b[0, y:y + tile, x:x + tile].reshape(-1, 1), 16, mn, mx)[0].reshape(-1)
            diff = np.flatnonzero(sa != sb)
            assert diff.size > 1000
            rep = reports[6]
            assert (rep.mismatches, rep.first_sample, rep.first_channel, rep.expected, rep.got) == (
                diff.size, diff[0], 0, sa[diff[0]], sb[diff[0]])
            _clean(reports[:6] + reports[7:], wins[:6] + wins[7:])
    finally:
        ctx.free(dev_b)


# ------------------------------------------------------------------------------- 7. errors
def test_verify_before_execute_and_a_damaged_frame():
    r = _raster(np.uint16, 4, seed=18)
    with _Resident(r, WINS, 5) as d:
        with pytest.raises(N.NativeError, match="error -5.*not executed"):
            d.plan.verify()
        d.plan.execute()
        d.plan.sync()
        infos, frames = d.plan.download()
        off = d.plan.frame_offsets(sum(i.nframes for i in infos))
        ptr, _ = d.plan.device_output()
        bad = np.frombuffer(frames, np.uint8).copy()
        k = infos[0].nframes + 3  # a frame of the second window: the position is relative to that window's frames
        bad[int(off[k]) + 40] ^= 0x20
        d.ctx.h2d(ptr, bad)
        with pytest.raises(N.NativeError, match=f"error -1.*corrupt frame at byte {int(off[k]) - infos[1].offset}$"):
            d.plan.verify()
        d.plan.execute()
        d.plan.sync()
        _clean(d.plan.verify(), WINS)


# ------------------------------------------------------------------------------- 8. wiring
def _count_verifies(monkeypatch):
    seen = []
    real = N.Plan.verify

    def verify(self):
        reports = real(self)
        seen.append(reports)
        return reports

    monkeypatch.setattr(N.Plan, "verify", verify)
    return seen


def test_encode_tiles_verify_returns_the_same_bytes(monkeypatch):
    r = _raster(np.uint16, 3, seed=19)
    seen = _count_verifies(monkeypatch)
    plain = encode_tiles(r, WINS, 5)
    assert not seen
    checked = encode_tiles(r, WINS, 5, verify=True)
    assert len(seen) == 1 and all(rep.mismatches == 0 for rep in seen[0])
    assert [t.data for t in checked] == [t.data for t in plain]
    # a plan over frame ranges, as a rank of the distributed encode holds
    ranges = [(1, 2), (0, -1), (2, -1), (18, -1)]
    part = encode_tiles(r, WINS, 5, frame_ranges=ranges, verify=True)
    assert len(seen) == 2 and [t.data for t in part] == [t.data for t in encode_tiles(r, WINS, 5, frame_ranges=ranges)]


def test_verify_mismatch_carries_raster_coordinates(monkeypatch):
    """A mismatching report of a group that starts below raster row 0 is raised in raster coordinates."""
    r = _raster(np.uint16, 2, seed=20)
    wins = [(40, 0, 200, 260), (40, 260, 200, 260)]
    real = N.Plan.verify

    def verify(self):
        reports = real(self)
        assert all(rep.mismatches == 0 for rep in reports)
        reports[1].mismatches, reports[1].first_sample, reports[1].first_channel = 2, 261, 1
        reports[1].expected, reports[1].got = 5, -6
        return reports

    monkeypatch.setattr(N.Plan, "verify", verify)
    with pytest.raises(N.VerifyMismatch) as ei:
        encode_tiles(r, wins, 5, verify=True)
    e = ei.value
    assert (e.tile, e.pixel, e.expected, e.got, e.mismatches) == (1, (41, 261, 1), 5, -6, 2)


def test_stream_encoder_verify_gives_the_same_stream(monkeypatch, golden_dir):
    from flac_raster.encoder import StreamEncoder

    audio = N.decode((golden_dir / "sample_rgb.flac").read_bytes())[0].astype(np.int16)
    assert audio.shape[1] == 3 and len(audio) > 3 * BS
    seen = _count_verifies(monkeypatch)

    def run(verify):
        calls = []
        enc = StreamEncoder(44100, lambda buf, n, s, f: calls.append((bytes(buf), n, s, f)), compression_level=5,
                            blocksize=BS, verify=verify)
        for lo, hi in [(0, 5000), (5000, 5001), (5001, 3 * BS + 77), (3 * BS + 77, len(audio))]:  # blocks are split
            enc.process(audio[lo:hi])
        enc.finish()
        return calls

    plain = run(False)
    assert not seen
    checked = run(True)
    assert len(seen) >= 3 and all(rep.mismatches == 0 and rep.nframes > 0 for reps in seen for rep in reps)
    assert checked == plain


def test_cli_convert_streaming_verify(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.tiff import write_geotiff

    r = _raster(np.uint16, 3, seed=21, h=300, w=420)
    src = tmp_path / "scene.tif"
    write_geotiff(src, r, transform=(10.0, 0.0, 300000.0, 0.0, -10.0, 5000040.0), crs="EPSG:32633")
    seen = _count_verifies(monkeypatch)
    a, b = tmp_path / "plain_streaming.flac", tmp_path / "verified_streaming.flac"
    res = CliRunner().invoke(app, ["convert", str(src), "-o", str(a), "--streaming", "--tile-size", "128"])
    assert res.exit_code == 0 and not seen, res.output
    res = CliRunner().invoke(app, ["convert", str(src), "-o", str(b), "--streaming", "--tile-size", "128", "--verify"])
    assert res.exit_code == 0 and len(seen) == 1, res.output
    assert a.read_bytes() == b.read_bytes()
    # the single-stream form goes through the same switch
    c = tmp_path / "whole.flac"
    res = CliRunner().invoke(app, ["convert", str(src), "-o", str(c), "--verify"])
    assert res.exit_code == 0 and len(seen) == 2 and c.stat().st_size > 0, res.output
