"""CPU tests of the band statistics (no GPU needed).

* the new C ABI names are declared, exported and bound; ``fra_stats_band`` is 160 bytes in the documented order;
  ``fra_stats`` and ``fra_decode_device_stats`` refuse every bad argument before any GPU work.
* ``stats.stats_arrays`` is the rule: against a brute-force Python loop (Python ints, ``fractions.Fraction``,
  ``math.fsum``) on tiny arrays of all eight dtypes with NaN, +-inf, -0.0 and nodata; sums past 64 bits; the exact
  histograms against ``np.bincount``; ``percentile`` against ``sorted(x)[k - 1]``.
* ``container_stats(device=None)`` and the ``stats`` command on the host path, on a small container.
"""
import ctypes as C
import json
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.stats import exact_range, percentile, report_from_bands, stats_arrays
from flac_raster.streaming import assemble_streaming, container_stats, read_window, streaming_to_raster
from flac_raster.tiff import write_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
NEW = ("fra_stats", "fra_decode_device_stats", "fra_stats_timing")
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TILE = 150, 200, 64  # 3 x 4 tiles, ragged right and bottom


# ------------------------------------------------------------------------------- 1. names and refusals
def test_new_names_exported_declared_and_bound():
    hdr = (ROOT / "include" / "flac_raster_amd.h").read_text()
    decl = set(re.findall(r"FRA_API\s+[^;(]*?\b(fra_\w+)\s*\(", hdr))
    L = N.load()
    for name in NEW:
        assert name in decl and name in N.EXPORTS and hasattr(L, name), name
    for name in ("fra_stats_band", "fra_stats_job", "fra_stats_opts", "FRA_STATS_AUTO_RANGE 1", "FRA_STATS_NODATA 2"):
        assert name in hdr, name
    assert C.sizeof(N.StatsBand) == 160
    assert [f[0] for f in N.StatsBand._fields_] == [
        "count", "valid", "nan", "nodata", "below", "above", "sum_lo", "sum_hi", "sq_lo", "sq_hi", "min", "max",
        "fin_min", "fin_max", "fsum", "mean", "fm2", "hist_lo", "hist_hi", "hist_scale"]
    assert [t for _, t in N.StatsBand._fields_[:10]] == [C.c_uint64] * 7 + [C.c_int64] + [C.c_uint64] * 2
    assert all(t is C.c_double for _, t in N.StatsBand._fields_[10:])
    assert [f[0] for f in N.StatsOpts._fields_] == ["bins", "flags", "hist_lo", "hist_hi", "nodata"]
    assert (N.STATS_AUTO_RANGE, N.STATS_NODATA) == (1, 2)
    assert L.fra_abi_version() == 3 and re.search(r"#define\s+FRA_ABI_VERSION\s+3\b", hdr)
    for name in ("stats", "decode_device_stats", "stats_timing"):
        assert hasattr(N.Context, name), name
    assert C.sizeof(N.DecodeJob) == 88 and C.sizeof(N.DecodeItem) == 72  # the decode structures keep their layouts


def _stats_job():
    a = (C.c_int32 * 64)()
    job = N.StatsJob()
    job.src, job.dtype = C.cast(a, C.c_void_p), N.DTYPE_CODES[np.dtype(np.int32)]
    job.channels, job.height, job.width = 1, 8, 8
    job.band_stride, job.row_stride, job.col_stride = 64, 8, 1
    return job, a


BAD_OPTS = [  # (bins, flags, lo, hi), a word of the message
    ((-1, 0, 0.0, 1.0), b"bins"), ((65537, 0, 0.0, 1.0), b"bins"), ((0, 4, 0.0, 0.0), b"flags"),
    ((4, 8 | 1, 0.0, 1.0), b"flags"), ((4, 0, 2.0, 1.0), b"range"), ((4, 0, math.nan, 1.0), b"range"),
    ((4, 0, 0.0, math.inf), b"range"), ((4, 2, -math.inf, 0.0), b"range"),
]


def test_stats_entry_refuses_before_any_gpu_work():
    """Every call returns FRA_E_INVALID before the context is looked at, so a stand-in pointer serves."""
    L = N.load()
    ctx = C.c_void_p(16)
    bands = (N.StatsBand * 1)()
    hist = (C.c_uint64 * 8)()
    job, _keep = _stats_job()
    assert L.fra_stats(None, C.byref(job), bands, hist) == -1 and b"null" in L.fra_last_error()
    assert L.fra_stats(ctx, None, bands, hist) == -1 and b"null" in L.fra_last_error()
    assert L.fra_stats(ctx, C.byref(job), None, hist) == -1 and b"null" in L.fra_last_error()
    job.src = None
    assert L.fra_stats(ctx, C.byref(job), bands, hist) == -1 and b"null" in L.fra_last_error()
    for dt in (-1, 8):
        job, _keep = _stats_job()
        job.dtype = dt
        assert L.fra_stats(ctx, C.byref(job), bands, hist) == -1 and b"dtype" in L.fra_last_error(), dt
    for field, v in (("channels", 0), ("height", 0), ("width", 0), ("width", -3), ("band_stride", -1),
                     ("row_stride", -8), ("col_stride", -1)):
        job, _keep = _stats_job()
        setattr(job, field, v)
        assert L.fra_stats(ctx, C.byref(job), bands, hist) == -1 and b"layout" in L.fra_last_error(), field
    job, _keep = _stats_job()
    job.height, job.width = 65537, 65536  # 2^32 + 2^16 pixels
    assert L.fra_stats(ctx, C.byref(job), bands, hist) == -1 and b"2^32 pixels" in L.fra_last_error()
    for (b, f, lo, hi), word in BAD_OPTS:
        job, _keep = _stats_job()
        job.opts.bins, job.opts.flags, job.opts.hist_lo, job.opts.hist_hi = b, f, lo, hi
        assert L.fra_stats(ctx, C.byref(job), bands, hist) == -1 and word in L.fra_last_error(), (b, f, lo, hi)
    job, _keep = _stats_job()
    job.opts.bins, job.opts.hist_lo, job.opts.hist_hi = 8, 0.0, 1.0
    assert L.fra_stats(ctx, C.byref(job), bands, None) == -1 and b"null histogram" in L.fra_last_error()
    assert L.fra_stats_timing(None) == -1 and b"null" in L.fra_last_error()


def _decode_job():
    data = (C.c_uint8 * 64)()
    item = N.DecodeItem()
    item.offset, item.bytes, item.window = 0, 64, N.Window(0, 0, 4, 8)
    job = N.DecodeJob()
    job.data, job.len, job.items, job.nitems = C.cast(data, C.c_void_p), 64, C.pointer(item), 1
    job.dst, job.dst_dtype, job.channels = None, N.DTYPE_CODES[np.dtype(np.int32)], 1  # dst and its strides are ignored
    return job, item, data


def test_stats_of_a_decode_refuses_before_any_gpu_work():
    L = N.load()
    ctx = C.c_void_p(16)
    job, item, _keep = _decode_job()
    infos = (N.Decoded * 1)()
    bands = (N.StatsBand * 1)()
    hist = (C.c_uint64 * 8)()
    roi = N.Window(0, 0, 4, 8)
    opts = N.StatsOpts()

    def call(ctx=ctx, job=job, roi=roi, opts=opts, bands=bands, hist=hist, infos=infos):
        return L.fra_decode_device_stats(ctx, C.byref(job) if job is not None else None,
                                         C.byref(roi) if roi is not None else None,
                                         C.byref(opts) if opts is not None else None, bands, hist, infos)

    for kw in ({"ctx": None}, {"job": None}, {"roi": None}, {"opts": None}, {"bands": None}, {"infos": None}):
        assert call(**kw) == -1 and b"null" in L.fra_last_error(), kw
    for (b, f, lo, hi), word in BAD_OPTS:
        o = N.StatsOpts()
        o.bins, o.flags, o.hist_lo, o.hist_hi = b, f, lo, hi
        assert call(opts=o) == -1 and word in L.fra_last_error(), (b, f, lo, hi)
    o = N.StatsOpts()
    o.bins, o.flags = 8, N.STATS_AUTO_RANGE
    assert call(opts=o, hist=None) == -1 and b"null histogram" in L.fra_last_error()
    for dt in (-1, 8):
        job.dst_dtype = dt
        assert call() == -1 and b"dtype" in L.fra_last_error(), dt
    job.dst_dtype = N.DTYPE_CODES[np.dtype(np.int32)]
    for ch in (0, 9):
        job.channels = ch
        assert call() == -1 and b"layout" in L.fra_last_error(), ch
    job.channels = 1
    # the job's own strides are ignored, whatever they hold
    job.band_stride, job.row_stride, job.col_stride = -5, -5, -5
    assert call(roi=N.Window(0, 0, 5, 8)) == -1 and b"do not cover the region" in L.fra_last_error()
    job.band_stride, job.row_stride, job.col_stride = 0, 0, 0
    item.window = N.Window(0, 0, 4, 7)  # an uncovered column
    assert call() == -1 and b"do not cover the region" in L.fra_last_error()
    job.nitems = 0
    assert call() == -1 and b"do not cover the region" in L.fra_last_error()
    job.nitems = 1
    item.window = N.Window(0, 0, 4, 8)
    assert call(roi=N.Window(0, 0, 65537, 65536)) == -1 and b"2^32 pixels" in L.fra_last_error()
    # what the windowed read refuses is refused in its words
    assert call(roi=N.Window(0, 0, 0, 8)) == -1 and b"region of interest" in L.fra_last_error()
    job.flags = N.DECODE_CONCAT
    assert call() == -1 and b"CONCAT" in L.fra_last_error()
    job.flags = 0
    job.denorm = 3
    assert call() == -1 and b"denorm" in L.fra_last_error()


# ------------------------------------------------------------------------------- 2. the numpy rule
def _brute(a, bins, rng, nodata):
    """One band by a Python loop: integers with Python ints and Fractions, floats with math.fsum."""
    is_float = a.dtype.kind == "f"
    vals, r = [], {"nan": 0, "nodata": 0}
    for v in a.ravel().tolist():
        x = float(v)
        if x != x:
            r["nan"] += 1
        elif nodata is not None and x == nodata:
            r["nodata"] += 1
        else:
            vals.append(v)
    n = r["valid"] = len(vals)
    fin = [v for v in vals if math.isfinite(v)]
    r["min"], r["max"] = (float(min(vals)), float(max(vals))) if vals else (None, None)
    r["fin_min"], r["fin_max"] = (float(min(fin)), float(max(fin))) if fin else (None, None)
    if is_float:
        r["sum_terms"] = vals
    else:
        r["sum"], r["sum_sq"] = sum(vals), sum(v * v for v in vals)
        r["mean"] = float(Fraction(r["sum"], n)) if n else math.nan
        r["variance"] = float(Fraction(sum((v * n - r["sum"]) ** 2 for v in vals), n ** 3)) if n else math.nan
    if rng == "auto":
        rng = (r["fin_min"], r["fin_max"]) if fin else None
    r["hist_range"] = list(rng) if rng is not None and bins else None
    r["below"] = r["above"] = 0
    r["histogram"] = [0] * bins if bins else None
    if bins and rng is not None:
        lo, hi = rng
        scale = bins / (hi - lo) if hi > lo and hi - lo != math.inf else 0.0
        if not math.isfinite(scale):
            scale = 0.0
        for v in vals:
            x = float(v)
            if x < lo:
                r["below"] += 1
            elif x > hi:
                r["above"] += 1
            else:
                r["histogram"][0 if scale == 0.0 else min(bins - 1, math.floor((x - lo) * scale))] += 1
    return r


def _same(x, y):
    return (x is None and y is None) or (x is not None and y is not None and ((x != x and y != y) or x == y))


def _check_against_brute(a, bins=0, rng=None, nodata=None):
    rep = stats_arrays(a, bins, rng, nodata)
    is_float = a.dtype.kind == "f"
    assert len(rep) == a.shape[0]
    for band, x in zip(rep, a):
        want = _brute(x, bins, "auto" if (rng is None and bins) else rng, nodata)
        assert band["count"] == x.size == band["valid"] + band["nan"] + band["nodata"]
        for key in ("valid", "nan", "nodata", "below", "above", "histogram", "hist_range"):
            assert band[key] == want[key], (key, band[key], want[key])
        for key in ("min", "max", "fin_min", "fin_max"):
            assert _same(band[key], want[key]), (key, band[key], want[key])
        n = want["valid"]
        if is_float:
            terms = want["sum_terms"]
            if n == 0:
                assert band["sum"] == 0.0 and band["fm2"] == 0.0 and math.isnan(band["mean"])
            elif all(map(math.isfinite, terms)):
                s = math.fsum(terms)
                assert abs(band["sum"] - s) <= n * 2.0 ** -53 * math.fsum(map(abs, terms))
                assert band["mean"] == band["sum"] / n
                sq = [(t - band["mean"]) * (t - band["mean"]) for t in terms]
                assert abs(band["fm2"] - math.fsum(sq)) <= n * 2.0 ** -53 * math.fsum(sq)
                assert band["variance"] == band["fm2"] / n and band["std"] == math.sqrt(band["variance"])
            else:  # plain IEEE: an infinity propagates
                assert not math.isfinite(band["sum"]) and not math.isfinite(band["fm2"])
        else:
            assert isinstance(band["sum"], int) and band["sum"] == want["sum"] and band["sum_sq"] == want["sum_sq"]
            assert _same(band["mean"], want["mean"]) and _same(band["variance"], want["variance"])
            if n:
                assert band["std"] == math.sqrt(want["variance"])
    return rep


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_stats_arrays_equals_the_brute_force_loop(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(17 + dt.num)
    for shape in ((1, 1, 1), (2, 3, 5), (3, 7, 4)):
        if dt.kind == "f":
            a = (rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 6, size=shape)).astype(dt)
            lo, hi = -50.0, 120.5
        else:
            info = np.iinfo(dt)
            a = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
            lo, hi = info.min * 0.5 + 3, info.max * 0.75
        nd = float(a[0, 0, 0])  # a value that occurs
        for bins, r in ((0, None), (1, "auto"), (7, "auto"), (7, (lo, hi)), (256, (lo, hi)), (5, (lo, lo))):
            _check_against_brute(a, bins, r)
            rep = _check_against_brute(a, bins, r, nodata=nd)
            assert rep[0]["nodata"] >= 1
        _check_against_brute(a, 4, None)  # None with bins: the automatic range
        assert stats_arrays(a[0], 3, "auto") == stats_arrays(a[:1], 3, "auto")  # the (h, w) form
    c = np.full((1, 3, 3), a[0, 0, 0], dt)  # a constant band: lo == hi, everything in bin 0
    rep = _check_against_brute(c, 5, "auto")
    assert rep[0]["histogram"] == [9, 0, 0, 0, 0] and rep[0]["hist_scale"] == 0.0 and rep[0]["variance"] == 0.0
    rep = _check_against_brute(c, 5, "auto", nodata=float(c[0, 0, 0]))  # a band of nodata only
    assert rep[0]["valid"] == 0 and rep[0]["min"] is None and rep[0]["hist_range"] is None
    assert rep[0]["histogram"] == [0] * 5 and math.isnan(rep[0]["mean"])


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_stats_arrays_nan_inf_and_negative_zero(dt):
    nan, inf = np.nan, np.inf
    a = np.array([[[nan, -0.0, 1.0, 0.0, inf, 2.5, -inf, 2.0], [3.0, 0.0, 5.0, nan, 1e30, -1.5, 0.25, 7.0]]], dt)
    rep = _check_against_brute(a, 8, "auto")[0]
    assert (rep["nan"], rep["valid"], rep["below"], rep["above"]) == (2, 14, 1, 1)
    assert (rep["min"], rep["max"], rep["fin_min"], rep["fin_max"]) == (-inf, inf, -1.5, float(dt(1e30)))
    assert math.isnan(rep["sum"]) and math.isnan(rep["mean"]) and sum(rep["histogram"]) == 12
    a[0, 0, 6] = 4.0
    rep = _check_against_brute(a, 8, (-2.0, 8.0))[0]
    assert rep["sum"] == inf and rep["mean"] == inf and rep["above"] == 2 and rep["below"] == 0
    # nodata 0.0 takes -0.0 too; a NaN nodata matches nothing
    rep = _check_against_brute(a, 0, None, nodata=0.0)[0]
    assert rep["nodata"] == 3
    assert _check_against_brute(a, 0, None, nodata=nan)[0]["nodata"] == 0
    # a band without a number
    rep = _check_against_brute(np.full((1, 2, 2), nan, dt), 4, "auto")[0]
    assert rep["valid"] == 0 and rep["nan"] == 4 and rep["min"] is None and rep["hist_range"] is None
    assert rep["sum"] == 0.0 and rep["fm2"] == 0.0 and math.isnan(rep["mean"])
    # only infinities: valid, but no automatic range
    rep = _check_against_brute(np.array([[[inf, -inf]]], dt), 4, "auto")[0]
    assert rep["valid"] == 2 and rep["fin_min"] is None and rep["histogram"] == [0] * 4 and rep["below"] == 0


def test_sums_past_64_bits_and_native_reports():
    a = np.full((1, 70, 70), 2**32 - 1, np.uint32)
    rep = stats_arrays(a)[0]
    assert rep["sum"] == 4900 * (2**32 - 1) and rep["sum_sq"] == 4900 * (2**32 - 1) ** 2 > 2**64
    assert rep["mean"] == float(2**32 - 1) and rep["variance"] == 0.0
    rng = np.random.default_rng(3)
    big = rng.integers(2**31, 2**32, size=(1, 1 << 11, 1 << 11), dtype=np.int64).astype(np.uint32)  # sum > 2^53
    rep = stats_arrays(big)[0]
    assert rep["sum"] == int(big.astype(np.uint64).sum()) and rep["sum_sq"] > 2**64
    assert rep["sum_sq"] == sum(int(v) for v in (big.astype(np.uint64)[0] ** 2 >> np.uint64(32)).sum(axis=1)) * 2**32 + \
        sum(int(v) for v in (big.astype(np.uint64)[0] ** 2 & np.uint64(0xFFFFFFFF)).sum(axis=1))
    neg = np.full((1, 1 << 11, 1 << 11), -2**31, np.int32)
    rep = stats_arrays(neg)[0]
    assert rep["sum"] == -(2**31) * (1 << 22) and rep["sum_sq"] == 2**62 * (1 << 22) > 2**64
    # the native record of the same band gives the same dict: a negative 128-bit sum, a square past 64 bits
    r = N.StatsBand()
    r.count = r.valid = 1 << 22
    r.sum_lo, r.sum_hi = rep["sum"] & (2**64 - 1), rep["sum"] >> 64
    r.sq_lo, r.sq_hi = rep["sum_sq"] & (2**64 - 1), rep["sum_sq"] >> 64
    r.min = r.max = r.fin_min = r.fin_max = float(-2**31)
    assert r.sum_hi == -1
    assert report_from_bands([r], None, np.int32) == [rep]
    with pytest.raises(TypeError):
        stats_arrays(np.zeros((1, 2, 2), np.int64))
    for bad in ({"bins": -1}, {"bins": 65537}, {"bins": 4, "hist_range": (2.0, 1.0)},
                {"bins": 4, "hist_range": (0.0, math.inf)}):
        with pytest.raises(ValueError):
            stats_arrays(np.zeros((1, 2, 2), np.int16), **bad)


@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.uint16, np.int16], ids=lambda d: np.dtype(d).name)
def test_exact_range_histograms_equal_bincount_and_percentiles_the_sorted_values(dt):
    dt = np.dtype(dt)
    info = np.iinfo(dt)
    rng = np.random.default_rng(40 + dt.num)
    lo, hi, bins = exact_range(dt)
    assert (lo, hi, bins) == (float(info.min), float(info.max) + 1.0, 2 ** (8 * dt.itemsize))
    a = rng.integers(info.min, int(info.max) + 1, size=(2, 37, 53), dtype=np.int64).astype(dt)
    a[1] = (a[1] // 7).astype(dt)  # a narrower band with ties
    a[0, 0, :2] = info.min, info.max
    for band, x in zip(stats_arrays(a, bins, (lo, hi)), a):
        assert band["hist_scale"] == 1.0 and band["below"] == band["above"] == 0
        assert band["histogram"] == np.bincount(x.ravel().astype(np.int64) - int(info.min), minlength=bins).tolist()
        s = sorted(x.ravel().tolist())
        for q in (0, 2, 2.5, 50, 98, 99.99, 100, Fraction(1, 3)):
            k = max(1, math.ceil(Fraction(str(q)) * len(s) / 100))
            assert percentile(band, q) == s[k - 1], q
    # with a nodata value the percentiles are over what remains
    band = stats_arrays(a[:1], bins, (lo, hi), nodata=float(a[0, 3, 3]))[0]
    s = sorted(v for v in a[0].ravel().tolist() if v != a[0, 3, 3])
    assert percentile(band, 50) == s[max(1, math.ceil(len(s) / 2)) - 1] and len(s) == band["valid"]
    # wider bins: the bin's nominal edges
    band = stats_arrays(a[:1], 16, (lo, hi))[0]
    e = percentile(band, 50)
    s = sorted(a[0].ravel().tolist())
    assert isinstance(e, tuple) and e[0] <= s[math.ceil(len(s) / 2) - 1] < e[1] and e[1] - e[0] == (hi - lo) / 16
    assert percentile(stats_arrays(a[:1])[0], 50) is None  # no histogram
    with pytest.raises(ValueError):
        exact_range(np.uint32)
    with pytest.raises(ValueError):
        percentile(band, 101)


# ------------------------------------------------------------------------------- 3. the container on the host
@pytest.fixture(scope="module")
def container():
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (30000 + 20000 * np.sin(yy / 23.0) + 8000 * np.cos(xx / 31.0)).astype(np.int64)  # a wide range per tile
    r = np.stack([base + b * 7 + rng.integers(0, 50, size=(H, W)) for b in range(2)]).astype(np.uint16)
    tiles = calculate_tiles(H, W, TILE)
    streams = oracle_encode_tiles(r, tiles, level=5)
    data = assemble_streaming(tiles, streams, r.shape, r.dtype, TRANSFORM, "EPSG:32633", TILE)
    full = {sem: streaming_to_raster(data, device=None, semantics=sem)[0] for sem in ("pcm16", "int")}
    return data, r, full


def test_host_container_stats(container):
    data, src, full = container
    lo, hi, bins = exact_range(np.uint16)
    for sem in ("pcm16", "int"):
        rep, win, index = container_stats(data, device=None, semantics=sem, bins=bins, hist_range=(lo, hi))
        assert win == (0, 0, H, W) and index["height"] == H
        assert rep == stats_arrays(full[sem], bins, (lo, hi))
        assert rep[1]["histogram"] == np.bincount(full[sem][1].ravel(), minlength=65536).tolist()
        assert percentile(rep[0], 50) == sorted(full[sem][0].ravel().tolist())[H * W // 2 - 1]
    wdw = (40, 50, 60, 70)
    nd = float(full["pcm16"][0, 45, 60])
    rep, win, _ = container_stats(data, window=wdw, device=None, bins=7, nodata=nd)
    assert win == wdw and rep == stats_arrays(read_window(data, window=wdw)[0], 7, "auto", nd)
    assert rep[0]["nodata"] >= 1 and rep[0]["count"] == 60 * 70
    rep, win, _ = container_stats(data, bbox=(500500.0, 4099000.0, 501200.0, 4099600.0), device=None)
    assert win == wdw and rep == stats_arrays(full["pcm16"][:, 40:100, 50:120])
    with pytest.raises(ValueError):
        container_stats(data, device=None, semantics="float")
    with pytest.raises(ValueError):
        container_stats(data, device=None, bins=70000)


def test_stats_cli_on_the_host(container, tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli

    data, src, full = container
    flac = tmp_path / "scene_streaming.flac"
    flac.write_bytes(data)
    monkeypatch.setattr(cli, "_gpu_present", lambda: False)  # the host path, wherever this runs
    run = lambda *args: CliRunner().invoke(cli.app, ["stats", *[str(a) for a in args]])  # noqa: E731
    out = tmp_path / "stats.json"
    res = run(flac, "--export", out)
    assert res.exit_code == 0, res.output
    assert "p50" in res.output and "Std" in res.output
    rep = json.loads(out.read_text())
    lo, hi, bins = exact_range(np.uint16)
    want = stats_arrays(full["pcm16"], bins, (lo, hi))  # the exact histogram is the default for uint16
    assert rep["dtype"] == "uint16" and rep["window"] == [0, 0, H, W] and rep["device"] is None
    for got, w in zip(rep["bands"], want):
        s = sorted(full["pcm16"][w["band"] - 1].ravel().tolist())
        assert got["percentiles"] == {str(q): float(s[max(1, math.ceil(q * len(s) / 100)) - 1]) for q in (2, 50, 98)}
        del got["percentiles"]
        assert got == w
    res = run(flac, "--window", "40,50,60,70", "--bins", "16", "--range", "20000,50000", "--percentiles", "50",
              "--semantics", "int", "--export", out)
    assert res.exit_code == 0, res.output
    rep = json.loads(out.read_text())
    want = stats_arrays(full["int"][:, 40:100, 50:120], 16, (20000.0, 50000.0))
    assert [b["histogram"] for b in rep["bands"]] == [b["histogram"] for b in want] and rep["semantics"] == "int"
    assert rep["bands"][0]["percentiles"]["50"] == list(percentile(want[0], 50))
    # a GeoTIFF, with its own nodata tag and with one given
    tif = tmp_path / "src.tif"
    write_geotiff(tif, src, transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    nd = float(src[1, 10, 10])
    res = run(tif, "--nodata", nd, "--export", out)
    assert res.exit_code == 0, res.output
    rep = json.loads(out.read_text())
    want = stats_arrays(src, bins, (lo, hi), nd)
    assert [{k: b[k] for k in w} for b, w in zip(rep["bands"], want)] == want and rep["bands"][1]["nodata"] >= 1
    assert run(tif, "--window", "0,0,8,8", "--bbox", "500500.0,4099000.0,501200.0,4099600.0").exit_code == 1
    assert run(tmp_path / "absent.tif").exit_code == 1
    assert run(flac, "--bins", "70000").exit_code == 1
    assert run(flac, "--semantics", "float").exit_code == 1
