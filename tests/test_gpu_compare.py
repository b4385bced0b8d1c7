"""GPU tests of the raster comparison (``k_compare`` + ``k_compare_fold`` alone through ``fra_compare``, and behind the
windowed read through ``fra_decode_device_compare``).

The expectation is never the kernel: it is ``compare.compare_arrays`` -- the rule in numpy and Python integers, checked
on the CPU against a brute-force loop -- applied to the rasters themselves, or to the host ``read_window`` and the
reference's crop.  Integers must match exactly, every field.  Floats: the counts, the first pixel, ``max_abs``, the
ranges and ``unordered`` exactly; the two f64 sums within ``n * 2^-53 * sum |term|`` of ``math.fsum`` over the n terms,
the worst case of any summation order.  The shapes are the smallest at which the thread mapping can go wrong: a single
pixel, less than one slot row, a few rows of odd width, and one that needs several workgroups per band (for every
dtype); rows that are and are not 16-byte aligned (vector and element loads), one raster of each, pixel-interleaved.
"""
import json
import math

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.compare import compare_arrays, report_from_bands
from flac_raster.geo import Affine
from flac_raster.tiff import write_geotiff

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
SHAPES = [(1, 1), (7, 19), (33, 67), (130, 517)]  # the last: 3 (one-byte) to 17 (f64) workgroups per band
B = 3


def _ctx():
    return N.default_context(0)


def _same_float(x, y):
    return (x != x and y != y) or x == y


def _float_sums(a, b):
    """math.fsum of |d| and d * d over the pixels where both are numbers, and the bound for any order of that many
    additions; (inf, 0) where a term is infinite."""
    out = []
    for x, y in zip(a.astype(np.float64), b.astype(np.float64)):
        ok = ~(np.isnan(x) | np.isnan(y))
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.where(x == y, 0.0, x - y)[ok]
        rec = []
        for t in (np.abs(d), d * d):
            if np.isinf(t).any():
                rec.append((math.inf, 0.0))
            else:
                s = math.fsum(t.tolist())
                rec.append((s, t.size * 2.0 ** -53 * s))
        out.append(rec)
    return out


def _check(bands, a, b):
    """Native reports against compare_arrays(a, b)."""
    want = compare_arrays(a, b)
    is_float = a.dtype.kind == "f"
    assert len(bands) == a.shape[0]
    sums = _float_sums(a, b) if is_float else None
    for i, (r, w) in enumerate(zip(bands, want["bands"])):
        assert r.count == w["count"] == a.shape[1] * a.shape[2] and r.reserved == 0
        assert r.differing == w["differing"] and r.unordered == w["unordered"], (i, r.differing, w)
        first = [r.first_row, r.first_col] if r.first_row >= 0 else None
        assert first == w["first"] and (first is not None or r.first_col == -1), (i, first, w["first"])
        assert r.max_abs == w["max_diff"], (i, r.max_abs, w["max_diff"])
        for got, exp in ((r.a_min, w["file1_range"][0]), (r.a_max, w["file1_range"][1]), (r.b_min, w["file2_range"][0]),
                         (r.b_max, w["file2_range"][1])):
            assert _same_float(got, exp), (i, got, exp)
        if is_float:
            assert r.sum_abs == 0 and r.sum_sq_lo == 0 and r.sum_sq_hi == 0
            for got, (s, tol) in zip((r.fsum_abs, r.fsum_sq), sums[i]):
                assert abs(got - s) <= tol if math.isfinite(s) else got == s, (i, got, s, tol)
        else:
            assert r.sum_abs == w["sum_abs"] and (r.sum_sq_hi << 64 | r.sum_sq_lo) == w["sum_sq"], (i, w)
            assert r.fsum_abs == 0.0 and r.fsum_sq == 0.0 and r.unordered == 0
    rep = report_from_bands(bands, a.dtype)
    assert rep["arrays_equal"] == want["arrays_equal"] == np.array_equal(a, b, equal_nan=is_float)
    if not is_float:
        assert rep == want  # host and GPU paths print alike
    return want


def _raster(dt, shape, rng):
    """Full-range integers; finite floats of mixed magnitude."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        return rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
    return (rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 6, size=shape)).astype(dt)


def _other(a, rng, frac=0.3):
    """``a`` with a fraction of its pixels replaced."""
    b = _raster(a.dtype, a.shape, rng)
    return np.where(rng.random(a.shape) < frac, b, a).astype(a.dtype)


def _padded(a, pad_cols, fill=77):
    """``a`` (B, h, w) as a view of a larger array: ``pad_cols`` spare columns per row and one spare row per band."""
    nb, h, w = a.shape
    big = np.full((nb, h + 1, w + pad_cols), fill, a.dtype)
    big[:, :h, :w] = a
    return big, big[:, :h, :w]


def _bytes(bands):
    return b"".join(bytes(r) for r in bands)


# ------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_alone_equals_the_numpy_rule(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(200 + dt.num)
    ctx = _ctx()
    V = 16 // dt.itemsize
    for (h, w) in SHAPES:
        a = _raster(dt, (B, h, w), rng)
        b = _other(a, rng)
        if dt.kind == "f" and h * w > 8:  # NaNs on both sides and on one: counted, never summed
            a[0, 0, 1] = b[0, 0, 1] = a[1, h - 1, 2] = b[2, h // 2, w - 1] = np.nan
        _check(ctx.compare(a, b), a, b)  # contiguous
        aligned = -w % V + V
        # rows not 16-byte aligned (element loads), aligned (16-byte loads), and one raster of each
        for pad_a, pad_b in ((5, 5), (aligned, aligned), (aligned, 5), (3, aligned)):
            abig, av = _padded(a, pad_a)
            bbig, bv = _padded(b, pad_b)
            keep = abig.copy(), bbig.copy()
            got = ctx.compare(av, bv)
            _check(got, a, b)
            assert _bytes(ctx.compare(av, bv)) == _bytes(got), "a second call returns other bytes"
            assert abig.tobytes() == keep[0].tobytes() and bbig.tobytes() == keep[1].tobytes()  # nothing is written
            assert ctx.compare_timing() >= 0.0
        # pixel-interleaved, against a planar raster and against an interleaved one
        ai = np.ascontiguousarray(a.transpose(1, 2, 0)).transpose(2, 0, 1)
        bi = np.ascontiguousarray(b.transpose(1, 2, 0)).transpose(2, 0, 1)
        _check(ctx.compare(ai, b), a, b)
        _check(ctx.compare(ai, bi), a, b)
    # the largest shape again, device-resident: aligned rows for a, odd rows for b, then both aligned
    h, w = SHAPES[-1]
    rs_a, rs_b = w + (-w % V), w + 3
    for rs_b in (rs_b, rs_a):
        sa, sb = np.full((B, h, rs_a), 77, dt), np.full((B, h, rs_b), 77, dt)
        sa[:, :, :w], sb[:, :, :w] = a, b
        d_a, d_b = ctx.alloc(sa.nbytes), ctx.alloc(sb.nbytes)
        try:
            ctx.h2d(d_a, sa)
            ctx.h2d(d_b, sb)
            got = ctx.compare(d_a, d_b, dtype=dt, shape=(B, h, w), a_strides=(h * rs_a, rs_a, 1),
                              b_strides=(h * rs_b, rs_b, 1))
            _check(got, a, b)
            back = np.empty_like(sa)
            ctx.d2h(back, d_a)
            assert back.tobytes() == sa.tobytes()
        finally:
            ctx.free(d_a)
            ctx.free(d_b)


# A thread's way from one of its slots to the next, 256 slots on in row-major order, at its two corners.  (3, 4113): more
# than 256 slots per row for every element size (no whole row in a step), the last slot of a row holds 1 element (1 of 2
# for f64).  (5, 511): exactly 256 slots per row for f64 (a step is one row, no slots), 128 for f32 (two rows), and a
# short last slot for every dtype.
CURSOR_SHAPES = [(3, 4113), (5, 511)]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_rows_of_more_than_and_exactly_256_slots(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(250 + dt.num)
    ctx = _ctx()
    for (h, w) in CURSOR_SHAPES:
        a = _raster(dt, (B, h, w), rng)
        b = _other(a, rng)
        if dt.kind == "f":
            a[0, 0, 1] = b[0, 0, 1] = a[1, h - 1, 2] = b[2, h // 2, w - 1] = np.nan
        _check(ctx.compare(a, b), a, b)  # contiguous
        av, bv = _padded(a, 6)[1], _padded(b, 6)[1]  # rows of an odd number of elements: element loads
        assert av.strides[1] % 16 and bv.strides[1] % 16
        _check(ctx.compare(av, bv), a, b)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_identical_single_and_misordered_differences(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(300 + dt.num)
    ctx = _ctx()
    V = 16 // dt.itemsize
    h, w = SHAPES[-1]
    nvec = -(-w // V)
    a = _raster(dt, (B, h, w), rng)
    a.setflags(write=False)

    def bump(b, band, row, col):
        b[band, row, col] = a[band, row, col] + 1 if a[band, row, col] < 100 else a[band, row, col] - 1

    def slot(s):  # first pixel of slot s of a band: thread s % 256 of a workgroup meets it in its pass s // 256
        return s // nvec, (s % nvec) * V

    rep = _check(ctx.compare(a, a.copy()), a, a.copy())
    assert rep["arrays_equal"]
    cases = {
        "first pixel": [(0, 0, 0)],
        "last pixel of the last band": [(B - 1, h - 1, w - 1)],
        # a later thread meets the earlier pixel: slot 256 belongs to thread 0, slot 1 to thread 1
        "thread order against row-major order": [(1,) + slot(256), (1,) + slot(1)],
        "the same across passes": [(2,) + slot(3 * 256 + 5), (2,) + slot(2 * 256 + 200)],
        "inside one slot": [(0, 9, V + V - 1), (0, 9, V + 1)],
        "two workgroups": [(1, h - 1, 0), (1, 0, w - 1)],
    }
    for _ in range(4):
        cases[f"random pair {_}"] = [(int(rng.integers(B)), int(rng.integers(h)), int(rng.integers(w))) for _k in (0, 1)]
    for name, px in cases.items():
        b = a.copy()
        for p in px:
            bump(b, *p)
        for av, bv in ((a, b), (_padded(a, 5)[1], _padded(b, -w % V + V)[1])):
            want = _check(ctx.compare(av, bv), a, b)
            assert want["differing"] == len(set(px)), name
            band = want["bands"][px[0][0]]
            assert band["first"] == list(min(p[1:] for p in px if p[0] == px[0][0])), name


def test_wide_integer_sums_and_extremes():
    ctx = _ctx()
    # sum d^2 = 4900 (2^32 - 1)^2 > 2^64: the carry into the high word
    a, b = np.zeros((2, 70, 70), np.uint32), np.full((2, 70, 70), 2**32 - 1, np.uint32)
    for x, y in ((a, b), (b, a)):
        bands = ctx.compare(x, y)
        want = _check(bands, x, y)
        assert bands[0].sum_sq_hi == (4900 * (2**32 - 1) ** 2) >> 64 > 0 and want["max_difference"] == float(2**32 - 1)
        assert bands[1].sum_abs == 4900 * (2**32 - 1)
    for dt in (np.int32, np.int16, np.int8, np.uint16, np.uint8):
        info = np.iinfo(dt)
        lo, hi = np.full((1, 70, 70), info.min, dt), np.full((1, 70, 70), info.max, dt)
        for x, y in ((lo, hi), (hi, lo)):
            bands = ctx.compare(x, y)
            _check(bands, x, y)
            assert bands[0].max_abs == float(int(info.max) - int(info.min))
            assert (bands[0].a_min, bands[0].b_max) == (float(x[0, 0, 0]), float(y[0, 0, 0]))


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_specials(dt):
    ctx = _ctx()
    nan, inf = np.nan, np.inf
    a = np.array([[[nan, nan, 1.0, -0.0, inf, inf, -inf, 2.0], [3.0, 0.0, 5.0, nan, 1e30, -1.5, 0.25, 7.0]]], dt)
    b = np.array([[[nan, 1.0, nan, 0.0, inf, -inf, -inf, 2.5], [3.0, -0.0, 5.0, nan, 1e30, -1.5, 0.5, 7.0]]], dt)
    r = ctx.compare(a, b)[0]
    _check([r], a, b)
    # inf - -inf = inf propagates by plain IEEE arithmetic; inf against inf and -0.0 against 0.0 are equal
    assert (r.unordered, r.differing, r.first_row, r.first_col) == (4, 5, 0, 1)
    assert r.max_abs == inf and r.fsum_abs == inf and r.fsum_sq == inf
    assert (r.a_min, r.a_max, r.b_min, r.b_max) == (-inf, inf, -inf, inf)
    a[0, 0, 5] = -inf
    r = ctx.compare(a, b)[0]
    _check([r], a, b)
    assert (r.differing, r.max_abs, r.fsum_abs, r.fsum_sq) == (4, 0.5, 0.75, 0.3125)  # exact: few terms, powers of two
    # a band without a number on one side, and on both
    c = np.full((2, 5, 9), nan, dt)
    d = c.copy()
    d[1] = 1.5
    got = ctx.compare(c, d)
    _check(got, c, d)
    assert got[0].differing == 0 and got[0].unordered == 45 and math.isnan(got[0].a_min) and math.isnan(got[0].b_max)
    assert got[1].differing == 45 and got[1].first_row == 0 and math.isnan(got[1].a_max) and got[1].b_min == 1.5
    assert got[1].max_abs == 0.0 and got[1].fsum_abs == 0.0
    # the largest finite f32 squared fits f64; the largest f64 squared does not
    big = np.full((1, 3, 3), np.finfo(dt).max, dt)
    r = ctx.compare(big, -big)[0]
    _check([r], big, -big)
    assert r.fsum_sq == inf if dt == np.float64 else math.isfinite(r.fsum_sq)


# ------------------------------------------------------------------------------- 2. behind the decoder
H, W, TILE = 300, 420, 128  # 3 x 4 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
REGIONS = {"inside one tile": (10, 140, 50, 60), "four tiles": (100, 100, 60, 51), "whole raster": (0, 0, H, W)}


def _scene(dt, bands):
    rng = np.random.default_rng(12 + bands)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(30000 + 20000 * np.sin(yy / 41.0 + b) + 8000 * np.cos(xx / 53.0) + rng.integers(0, 400, (H, W)))
                  for b in range(bands)])
    if np.dtype(dt).kind == "f":
        r = (r / 7.0).astype(dt)
        r[0, 120, 110] = np.nan  # inside the four-tile region: the container holds a number there
        return r
    return r.astype(dt)


@pytest.fixture(scope="module", params=[(np.uint16, 3), (np.float32, 1), (np.float32, 2)],
                ids=["uint16x3", "float32x1", "float32x2"])
def scene(request):
    from flac_raster.streaming import build_streaming

    dt, bands = request.param
    src = _scene(dt, bands)
    data = build_streaming(src, TRANSFORM, "EPSG:32633", TILE)
    src.setflags(write=False)
    return data, src


def _float_close(rep, want, a, b):
    """A GPU report of floats against the host's: everything but the sums exactly, the sums within the bound."""
    sums = _float_sums(a, b)
    for i, (g, w) in enumerate(zip(rep["bands"], want["bands"])):
        for key in ("count", "differing", "unordered", "first", "max_diff", "equal"):
            assert g[key] == w[key], (key, g, w)
        for key in ("file1_range", "file2_range"):
            assert all(_same_float(p, q) for p, q in zip(g[key], w[key]))
        for key, (s, tol) in zip(("sum_abs", "sum_sq"), sums[i]):
            assert abs(g[key] - s) <= tol and abs(w[key] - s) <= tol, (key, g[key], w[key], s, tol)


@pytest.mark.parametrize("sem", ["pcm16", "int"])
def test_regions_against_the_source_raster(scene, sem):
    from flac_raster.streaming import _tile_items, read_window

    data, src = scene
    nb, dt = src.shape[0], src.dtype
    ctx = _ctx()
    index, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    denorm = N.DENORM_PCM16 if sem == "pcm16" else N.DENORM_INT
    for name, win in REGIONS.items():
        r, c, h, w = win
        host = read_window(data, window=win, device=None, semantics=sem)[0]
        plain = np.zeros((nb, h, w), dt)
        want_infos = ctx.decode_device_window(blob, items, plain, dt, nb, (h * w, w, 1), win, denorm)
        inside = src.copy()
        px = (nb - 1, r + h // 2, c + w - 1)
        inside[px] = host[nb - 1, h // 2, w - 1] + 9  # differs from the decoded pixel whatever the source held
        outside = src.copy()
        if name != "whole raster":
            for p in ((0, r - 1, c), (0, r, c - 1), (nb - 1, r + h, c + w - 1), (0, r + h - 1, c + w)):
                outside[p] = outside[p] + 11
        for ref_full in (src, inside, outside):
            ref = ref_full[:, r:r + h, c:c + w]  # a view: what lies outside the region is staged and never compared
            bands, infos = ctx.decode_device_compare(blob, items, ref, dt, nb, win, denorm)
            crop = np.ascontiguousarray(ref)
            want = _check(bands, host, crop)  # = compare_arrays(host read_window, ref crop)
            for g, e in zip(infos, want_infos):
                assert (g.nframes, g.nsamples, g.channels, g.bps, g.blocksize, g.sample_rate) == (
                    e.nframes, e.nsamples, e.channels, e.bps, e.blocksize, e.sample_rate)
            if ref_full is inside:
                assert bands[-1].differing >= 1 and bands[-1].first_row >= 0, "the changed pixel was not seen"
            if ref_full is outside:
                assert _bytes(bands) == base, "a pixel outside the region was seen"
            if ref_full is src:
                base = _bytes(bands)
                # a device-resident reference gives the same bytes
                d_ref = ctx.alloc(crop.nbytes)
                try:
                    ctx.h2d(d_ref, crop)
                    dev_bands, _ = ctx.decode_device_compare(blob, items, d_ref, dt, nb, win, denorm)
                finally:
                    ctx.free(d_ref)
                _check(dev_bands, host, crop)
                assert [(b.differing, b.first_row, b.first_col, b.max_abs, b.sum_abs, b.unordered) for b in dev_bands] == \
                       [(b.differing, b.first_row, b.first_col, b.max_abs, b.sum_abs, b.unordered) for b in bands]
        t = ctx.decode_timing()
        assert len(t) == 4 and t[3] >= 0.0 and ctx.compare_timing() >= 0.0
    if dt.kind == "f":  # the NaN of the source is a number in the container: one-sided, seen in the four-tile region
        win = REGIONS["four tiles"]
        bands, _ = ctx.decode_device_compare(blob, items, src[:, 100:160, 100:151], dt, nb, win, denorm)
        assert bands[0].unordered == 1 and bands[0].differing >= 1


def test_uncovered_region_is_refused_and_the_context_goes_on(scene):
    from flac_raster.streaming import _tile_items

    data, src = scene
    nb, dt = src.shape[0], src.dtype
    ctx = _ctx()
    _, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    win = REGIONS["four tiles"]
    ref = np.ascontiguousarray(src[:, 100:160, 100:151])
    hit = [k for k, it in enumerate(items) if it["window"][0] < 160 and it["window"][0] + it["window"][2] > 100
           and it["window"][1] < 151 and it["window"][1] + it["window"][3] > 100]
    assert len(hit) == 4
    with pytest.raises(N.NativeError, match="do not cover the region"):
        ctx.decode_device_compare(blob, [it for k, it in enumerate(items) if k != hit[-1]], ref, dt, nb, win,
                                  N.DENORM_PCM16)
    with pytest.raises(ValueError):
        ctx.decode_device_compare(blob, items, ref[:, :-1], dt, nb, win, N.DENORM_PCM16)
    bands, _ = ctx.decode_device_compare(blob, [items[k] for k in hit], ref, dt, nb, win, N.DENORM_PCM16)
    assert bands[0].count == 60 * 51


def test_compare_with_raster_and_check_cli_on_the_device(scene, tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.streaming import compare_with_raster, read_window, streaming_to_raster

    data, src = scene
    is_float = src.dtype.kind == "f"
    for win in (None, REGIONS["four tiles"]):
        host, hw, _ = compare_with_raster(data, src, window=win, device=None)
        dev, dw, idx = compare_with_raster(data, src, window=win, device=0)
        assert hw == dw == (win or (0, 0, H, W)) and len(idx["frames"]) == 12 and dev["origin"] == list(hw[:2])
        if is_float:
            r, c, h, w = hw
            _float_close(dev, host, read_window(data, window=hw, device=None)[0], src[:, r:r + h, c:c + w])
        else:
            assert dev == host
    flac = tmp_path / "scene_streaming.flac"
    flac.write_bytes(data)
    t = tuple(TRANSFORM)[:6]
    srcf, backf, out = tmp_path / "src.tif", tmp_path / "back.tif", tmp_path / "report.json"
    write_geotiff(srcf, src, transform=t, crs="EPSG:32633")
    write_geotiff(backf, streaming_to_raster(data, device=None)[0], transform=t, crs="EPSG:32633")
    run = lambda *args: CliRunner().invoke(app, ["check", *[str(a) for a in args], "--device", "0"])  # noqa: E731
    res = run(backf, flac, "--export", out)
    assert res.exit_code == 0, res.output
    assert json.loads(out.read_text())["passed"] is True
    res = run(srcf, flac, "--window", "100,100,60,51", "--export", out)
    assert res.exit_code == 1, res.output
    rep = json.loads(out.read_text())
    assert rep["window"] == [100, 100, 60, 51] and rep["differing"] == host["differing"] and not rep["passed"]
    assert rep["max_difference"] == host["max_difference"]
    # within a tolerance, unless a NaN stands on one side only (the float scene's source holds one in this window)
    res = run(srcf, flac, "--window", "100,100,60,51", "--max-diff", host["max_difference"], "--export", out)
    assert res.exit_code == (1 if is_float else 0), res.output
    assert json.loads(out.read_text())["one_sided_nan"] == (1 if is_float else 0)
    assert run(srcf, flac, "--window", "10,140,50,60", "--max-diff", "1e9").exit_code == 0  # no NaN in this window
