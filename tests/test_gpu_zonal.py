"""GPU tests of the zonal statistics (``k_zonal`` and its small kernels alone through ``fra_zonal``, and behind the
windowed read through ``fra_decode_device_zonal``).

The expectation is never the kernel: it is ``zonal.zonal_arrays`` -- the rule in numpy, Python integers and fractions,
checked on the CPU against a brute-force loop -- applied to the raster itself or to the host ``read_window``.  Integers
must match exactly, every field of every record and ``outside``.  Floats: the counts, the extremes and ``outside``
exactly; ``mean == fsum / valid`` bit for bit; ``fsum`` within ``n * 2^-53 * sum |x|`` of ``math.fsum`` and ``fm2`` within
``n * 2^-53 * sum term`` of ``math.fsum`` of the terms ``(x - mean)^2`` formed with the GPU's mean, per zone with ``n``
that zone's valid count: the worst case of any order of n additions, as ``test_gpu_stats.py`` derives it (the unit adds
with f64 atomics, so no order is fixed).  The shapes are the smallest at which the thread mapping can go wrong, as in
``test_gpu_stats.py``; the zone counts straddle the LDS windows of both passes.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.zonal import REC_DTYPE, report_from_recs, zonal_arrays

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
ZDTYPES = [np.uint8, np.int16, np.int32]       # on every shape but the largest
ZDTYPES_REST = [np.int8, np.uint16, np.uint32]  # on one shape
SHAPES = [(1, 1), (7, 19), (33, 67), (130, 517)]  # the last: 3 (one-byte) to 17 (f64) workgroups per band
B = 3
LDS_ZONES = 512    # kLdsZones of fra_zonal.hip: the zones a workgroup of the first pass keeps in LDS; a chunk of rows
#                    whose zones span more takes one launch per window of that size
LDS_ZONES2 = 2048  # kLdsZones2: the same for the floats' second pass
NZONES = [1, 2, 255, LDS_ZONES, LDS_ZONES + 1, 65536]
PATTERNS = ["const", "random", "blocks", "mixed"]


def _ctx():
    return N.default_context(0)


def same(x, y):
    """Equality of reports in which a NaN equals a NaN."""
    if isinstance(x, dict) and isinstance(y, dict):
        return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)) and isinstance(y, (list, tuple)):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    if isinstance(x, float) and isinstance(y, float) and x != x and y != y:
        return True
    return type(x) is type(y) and x == y


def _raster(dt, shape, rng):
    """Full-range integers; finite floats of mixed magnitude."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        return rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
    return (rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 6, size=shape)).astype(dt)


def _zones(pattern, shape, zdt, rng):
    """``(zones, zone_lo, nzones, ignore)`` of a pattern: one zone (the worst case of equal addresses), a label per
    pixel at random (no runs), blocks of 5 x 11 (runs that cross slot and row boundaries), and labels below zone_lo,
    above the range and an ignored one."""
    h, w = shape
    zdt = np.dtype(zdt)
    lo = 3 if zdt.kind == "u" else -4
    if pattern == "const":
        return np.full(shape, lo + 2, zdt), lo, 5, None
    if pattern == "random":
        return rng.integers(lo, lo + 40, shape).astype(zdt), lo, 40, None
    if pattern == "blocks":
        yy, xx = np.mgrid[0:h, 0:w]
        return ((yy // 5 * ((w + 10) // 11) + xx // 11) % 100 + lo).astype(zdt), lo, 100, None
    return rng.integers(lo - 3, lo + 23, shape).astype(zdt), lo, 16, lo + 5


def _valid_by_zone(band, zones, zone_lo, nzones, nodata, ignore):
    """label -> the band's valid pixels of that zone as f64."""
    z = zones.astype(np.int64).ravel()
    x = band.astype(np.float64).ravel()
    ok = (z >= zone_lo) & (z < zone_lo + nzones) & ~np.isnan(x)
    if ignore is not None:
        ok &= z != ignore
    if nodata is not None:
        ok &= x != nodata
    z, x = z[ok], x[ok]
    order = np.argsort(z, kind="stable")
    z, x = z[order], x[order]
    labels, starts = np.unique(z, return_index=True)
    return {int(k): v for k, v in zip(labels, np.split(x, starts[1:]))}


def _check(got, a, zones, zone_lo, nzones, nodata=None, ignore=None, want=None):
    """Native records and the outside count against zonal_arrays."""
    recs, outside = got
    a = a if a.ndim == 3 else a[None]
    is_float = a.dtype.kind == "f"
    if want is None:
        want = zonal_arrays(a, zones, zone_lo, nzones, nodata, ignore)
    assert recs.shape == (a.shape[0], nzones) and recs.dtype == REC_DTYPE
    assert outside == want[0]["outside"]
    assert not recs["reserved"].any() and np.array_equal(recs["count"], recs["valid"] + recs["nan"] + recs["nodata"])
    for b in range(a.shape[0]):  # count is the number of pixels of the zone, whatever the band
        assert np.array_equal(recs["count"][b], recs["count"][0])
    assert int(recs["count"][0].sum()) + outside == a.shape[1] * a.shape[2]
    none = recs[recs["valid"] == 0]  # zones without a valid pixel: NaN extremes, no sums
    assert np.isnan(none["min"]).all() and np.isnan(none["max"]).all()
    for f in ("sum_lo", "sum_hi", "sq_lo", "sq_hi", "fsum", "fm2"):
        assert not none[f].any(), f
    assert np.isnan(none["mean"]).all() if is_float else not none["mean"].any()
    rep = report_from_recs(recs, outside, a.dtype, zone_lo)
    if not is_float:
        assert not recs["fsum"].any() and not recs["mean"].any() and not recs["fm2"].any()
        assert same(rep, want)  # every field exact; host and GPU paths print alike
        return
    for f in ("sum_lo", "sum_hi", "sq_lo", "sq_hi"):
        assert not recs[f].any(), f
    for b, (g, w) in enumerate(zip(rep, want)):
        assert [r["zone"] for r in g["zones"]] == [r["zone"] for r in w["zones"]]
        vals = _valid_by_zone(a[b], zones, zone_lo, nzones, nodata, ignore)
        for r, e in zip(g["zones"], w["zones"]):
            assert (r["count"], r["valid"], r["nan"], r["nodata"]) == (e["count"], e["valid"], e["nan"], e["nodata"]), (b, r, e)
            assert same(r["min"], e["min"]) and same(r["max"], e["max"]), (b, r, e)
            n = r["valid"]
            if n == 0:
                assert r["sum"] == 0.0 and r["fm2"] == 0.0 and math.isnan(r["mean"])
                continue
            v = vals[r["zone"]]
            assert v.size == n
            with np.errstate(all="ignore"):
                assert same(r["mean"], float(np.float64(r["sum"]) / np.float64(n)))  # bit for bit
            if not np.isfinite(v).all():
                assert not math.isfinite(r["sum"]) and not math.isfinite(r["fm2"])
                continue
            s, sabs = math.fsum(v.tolist()), math.fsum(np.abs(v).tolist())
            assert abs(r["sum"] - s) <= n * 2.0 ** -53 * sabs, (b, r["zone"], r["sum"], s)
            with np.errstate(over="ignore"):
                d = v - np.float64(r["mean"])
                terms = d * d  # the GPU's terms: only the order of the additions differs
            if np.isfinite(terms).all():
                t = math.fsum(terms.tolist())
                assert abs(r["fm2"] - t) <= n * 2.0 ** -53 * t, (b, r["zone"], r["fm2"], t)
            else:
                assert r["fm2"] == math.inf


# ------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_alone_equals_the_numpy_rule(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(700 + dt.num)
    ctx = _ctx()
    for si, shape in enumerate(SHAPES):
        h, w = shape
        a = _raster(dt, (B,) + shape, rng)
        if dt.kind == "f" and h * w > 8:
            a[0, 0, 1] = a[1, h - 1, 2] = a[2, h // 2, w - 1] = np.nan
        nd = float(a[1, h // 2, w // 3])
        if nd != nd:
            nd = 1.5
        zdts = ZDTYPES + (ZDTYPES_REST if shape == (33, 67) else [])
        if si == 3:
            zdts = [ZDTYPES[DTYPES.index(dt.type) % 3]]
        for zdt in zdts:
            for pattern in PATTERNS:
                zones, lo, nz, ignore = _zones(pattern, shape, zdt, rng)
                nodata = nd if pattern in ("mixed", "blocks") else None
                got = ctx.zonal(a, zones, lo, nz, nodata, ignore)
                _check(got, a, zones, lo, nz, nodata, ignore)
                assert ctx.zonal_timing() >= 0.0


# Rows of many slots, at the two corners of the chunk arithmetic that the units over a raster share.  (3, 4113): more
# than 256 slots per row for every element size, the last slot of a row holds 1 element (1 of 2 for f64).  (5, 511):
# exactly 256 slots per row for f64, 128 for f32, and a short last slot for every dtype.  One value dtype per element
# size (both of four bytes).
CURSOR_SHAPES = [(3, 4113), (5, 511)]


@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.int32, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_rows_of_more_than_and_exactly_256_slots(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(750 + dt.num)
    ctx = _ctx()
    lo, nz = -2, 7
    for shape in CURSOR_SHAPES:
        h, w = shape
        a = _raster(dt, (B,) + shape, rng)
        if dt.kind == "f":
            a[0, 0, 1] = a[1, h - 1, 2] = a[2, h // 2, w - 1] = np.nan
        nd = float(a[1, h // 2, w // 3])  # (not one of the NaNs)
        zones = rng.integers(lo - 1, lo + nz + 1, shape).astype(np.int16)  # a label below and one above the zones
        zones[:, w // 2:w // 2 + 300] = lo + 3                              # and a run over many slots of every row
        want = zonal_arrays(a, zones, lo, nz, nd, lo + 5)
        _check(ctx.zonal(a, zones, lo, nz, nd, lo + 5), a, zones, lo, nz, nd, lo + 5, want)  # contiguous
        av, zv = _padded(a, 6, 77)[1], _padded(zones, 3, lo + 2)[1]  # rows of both that are not 16-byte aligned
        assert av.strides[1] % 16 and zv.strides[0] % 16
        _check(ctx.zonal(av, zv, lo, nz, nd, lo + 5), a, zones, lo, nz, nd, lo + 5, want)


@pytest.mark.parametrize("nz", NZONES)
def test_zone_counts_across_the_windows(nz):
    """Zone counts on both sides of the LDS window of the first pass (integers), the populated zones in every window,
    with labels below and above the range."""
    ctx = _ctx()
    rng = np.random.default_rng(nz)
    shape = (130, 517) if nz == 65536 else (33, 67)
    a = _raster(np.uint16, (B,) + shape, rng)
    lo = -7
    zones = rng.integers(lo - 2, lo + nz + 2, shape).astype(np.int32)
    _check(ctx.zonal(a, zones, lo, nz), a, zones, lo, nz)
    if nz >= 255:  # ... and in the last window only: a window that is skipped must not be this one
        last = rng.integers(lo + nz - 100, lo + nz, shape).astype(np.int32)
        got = ctx.zonal(a, last, lo, nz, None, lo + nz - 50)
        _check(got, a, last, lo, nz, None, lo + nz - 50)
        assert not got[0]["count"][:, :nz - 100].any() and got[0]["count"][:, nz - 100:].any()


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_windows_follow_the_chunks_of_rows(dt):
    """A workgroup's window of zones starts at the smallest zone of its own chunk of rows: zones that follow the rows
    (more of them than one window holds, few per chunk), the same with one far label in every chunk (its span then
    takes several windows, from a base that is no multiple of the window), and chunks that lie outside altogether."""
    ctx = _ctx()
    rng = np.random.default_rng(5)
    h, w = 130, 517
    a = _raster(dt, (2, h, w), rng)
    yy, xx = np.mgrid[0:h, 0:w]
    rows = (yy * 9 + xx // 64 + 3).astype(np.int32)  # 1181 zones, 9 per row
    nz = int(rows.max()) + 1
    _check(ctx.zonal(a, rows, 0, nz), a, rows, 0, nz)
    far = rows.copy()
    far[:, 100] = (yy[:, 100] * 9 + 1100) % nz
    _check(ctx.zonal(a, far, 0, nz), a, far, 0, nz)
    part = rows.copy()
    part[40:90] = -5      # whole chunks without a zone
    part[100:, ::2] = nz  # ... and above the range
    _check(ctx.zonal(a, part, 0, nz, None, 3), a, part, 0, nz, None, 3)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_zone_counts_across_both_windows(dt):
    """The floats' second pass keeps a window of its own size: zone counts on both sides of either window."""
    ctx = _ctx()
    rng = np.random.default_rng(77)
    shape = (33, 67)
    a = _raster(dt, (2,) + shape, rng)
    a[0, 5, 5] = a[1, 20, 60] = np.nan
    for nz in (LDS_ZONES, LDS_ZONES + 1, LDS_ZONES2, LDS_ZONES2 + 1):
        zones = rng.integers(0, nz + 3, shape).astype(np.uint16)
        _check(ctx.zonal(a, zones, 1, nz), a, zones, 1, nz)
        last = rng.integers(nz - 40, nz + 1, shape).astype(np.uint16)
        _check(ctx.zonal(a, last, 1, nz), a, last, 1, nz)


# ------------------------------------------------------------------------------- 2. specials
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_specials(dt):
    ctx = _ctx()
    nan, inf = np.nan, np.inf
    h, w = 33, 67
    rng = np.random.default_rng(9)
    a = _raster(dt, (2, h, w), rng)
    zones = np.repeat(np.arange(h, dtype=np.int16)[:, None] // 3, w, axis=1)  # 11 zones of three rows
    a[:, 0:3] = nan                                    # zone 0: all NaN
    a[:, 3:6] = -7.5                                   # zone 1: all nodata (without the nodata value: a constant zone)
    a[0, 7, 5], a[0, 8, 66] = inf, -inf                # zone 2: inf + -inf
    a[1, 6, 0] = inf                                   # ... and +inf alone
    a[0, 10, 4] = a[0, 11, 60] = -7.5                  # zone 3: the nodata value occurs
    a[0, 12, 5], a[0, 12, 6] = -0.0, 0.0               # zone 4
    for nodata in (None, -7.5, nan, 0.0):
        got = ctx.zonal(a, zones, 0, 12, nodata)
        _check(got, a, zones, 0, 12, nodata)
        recs, outside = got
        assert outside == 0 and recs["count"][0, 11] == 0 and math.isnan(recs["mean"][0, 11])  # an empty zone
        z0 = recs[0, 0]
        assert (z0["valid"], z0["nan"], z0["fm2"], z0["fsum"]) == (0, 3 * w, 0.0, 0.0) and math.isnan(z0["mean"])
        assert math.isnan(z0["min"]) and math.isnan(z0["max"])
        z2 = recs[0, 2]
        assert (z2["min"], z2["max"]) == (-inf, inf) and math.isnan(z2["fsum"]) and math.isnan(z2["mean"])
        assert not math.isfinite(z2["fm2"])
        assert recs[1, 2]["fsum"] == inf and recs[1, 2]["mean"] == inf and math.isnan(recs[1, 2]["fm2"])
        if nodata == -7.5:
            assert (recs[0, 1]["valid"], recs[0, 1]["nodata"], recs[0, 3]["nodata"]) == (0, 3 * w, 2)
            assert math.isnan(recs[0, 1]["mean"]) and recs[0, 1]["fsum"] == 0.0
        elif nodata is None or nodata != nodata:
            assert recs[0, 1]["fm2"] == 0.0 and recs[0, 1]["mean"] == -7.5 and recs[0, 1]["min"] == recs[0, 1]["max"] == -7.5
        if nodata == 0.0:
            assert recs[0, 4]["nodata"] == 2  # -0.0 too


def test_integer_specials():
    ctx = _ctx()
    # 70 x 70 of 2^32 - 1 in one zone: the sum of squares carries into the high word
    a = np.full((2, 70, 70), 2**32 - 1, np.uint32)
    a[1] = 0
    zones = np.zeros((70, 70), np.uint8)
    zones[:, 69] = 1
    for nodata in (None, 0.0, float(2**32 - 1)):
        got = ctx.zonal(a, zones, 0, 2, nodata)
        _check(got, a, zones, 0, 2, nodata)
        if nodata is None:
            r = got[0][0, 0]
            assert r["sq_hi"] == (4830 * (2**32 - 1) ** 2) >> 64 > 0 and r["sum_lo"] == 4830 * (2**32 - 1)
    # negative sums: the high word of the 128-bit sum is signed
    for dt in (np.int32, np.int16, np.int8):
        info = np.iinfo(dt)
        lo = np.full((1, 70, 70), info.min, dt)
        lo[0, 5, 5] = info.max
        for nodata in (None, float(info.max), 0.5, float(info.max) + 1.0):  # the last two match nothing
            got = ctx.zonal(lo, zones, 0, 2, nodata)
            _check(got, lo, zones, 0, 2, nodata)
            assert got[0][0, 0]["sum_hi"] == -1 and got[0][0, 0]["nodata"] == (1 if nodata == float(info.max) else 0)
    # zone_lo and the ignored label at the ends of int64, labels at the ends of their dtype
    z32 = np.array([[-2**31, 2**31 - 1, 0, 5]], np.int32)
    v = np.array([[[1, 2, 3, 4]]], np.int16)
    for zl, nz, ig in ((-2**31, 1, None), (2**31 - 1, 1, None), (-2**63, 1, None), (2**63 - 1, 1, None),
                       (-2**31, 65536, -2**31), (0, 6, 2**63 - 1), (2**31 - 65536, 65536, -2**63)):
        _check(ctx.zonal(v, z32, zl, nz, None, ig), v, z32, zl, nz, None, ig)


# ------------------------------------------------------------------------------- 3. layouts
def _padded(a, pad_cols, fill):
    """``a`` (..., h, w) as a view of a larger array: ``pad_cols`` spare columns per row and one spare row."""
    *lead, h, w = a.shape
    big = np.full(tuple(lead) + (h + 1, w + pad_cols), fill, a.dtype)
    big[..., :h, :w] = a
    return big, big[..., :h, :w]


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.int32, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_layouts(dt):
    dt = np.dtype(dt)
    ctx = _ctx()
    rng = np.random.default_rng(40 + dt.num)
    V = 16 // dt.itemsize
    for shape in ((7, 19), (33, 67)):
        h, w = shape
        a = _raster(dt, (B,) + shape, rng)
        for zdt in (np.uint8, np.int32):
            zones, lo, nz, ignore = _zones("mixed", shape, zdt, rng)
            zones[h // 2, :] = lo + 1  # a run across a whole row
            want = zonal_arrays(a, zones, lo, nz, None, ignore)
            chk = lambda got: _check(got, a, zones, lo, nz, None, ignore, want)  # noqa: E731
            sentinel = lo + 2  # a label inside the range: counted, it would show
            # host views: rows that are not / are 16-byte aligned, a pixel-interleaved raster, a zone column stride of 2
            abig5, av5 = _padded(a, 5, 77)
            abig16, av16 = _padded(a, -w % V + V, 77)
            zbig3, zv3 = _padded(zones, 3, sentinel)
            zbig16, zv16 = _padded(zones, -w % 16 + 16, sentinel)
            ai = np.ascontiguousarray(a.transpose(1, 2, 0)).transpose(2, 0, 1)
            z2big = np.full((h, 2 * w), sentinel, zones.dtype)
            z2big[:, ::2] = zones
            keep = [x.tobytes() for x in (abig5, abig16, zbig3, zbig16, ai, z2big)]
            for av, zv in ((av5, zv3), (av16, zv16), (av16, zv3), (av5, zv16), (ai, zones), (a, z2big[:, ::2]),
                           (ai, z2big[:, ::2])):
                chk(ctx.zonal(av, zv, lo, nz, None, ignore))
            assert [x.tobytes() for x in (abig5, abig16, zbig3, zbig16, ai, z2big)] == keep  # neither raster is written
            # device pointers, the bases offset by one element or not: both, either or neither raster takes vector loads
            rs, zrs = w + (-w % V) + V, w + (-w % 16) + 16
            sa = np.full((B, h, rs), 77, dt)
            sa[:, :, :w] = a
            sz = np.full((h, zrs), sentinel, zones.dtype)
            sz[:, :w] = zones
            abuf = np.full(sa.size + 1, 77, dt)
            zbuf = np.full(sz.size + 1, sentinel, zones.dtype)
            d_a, d_z = ctx.alloc(abuf.nbytes), ctx.alloc(zbuf.nbytes)
            try:
                for off_a in (0, 1):
                    abuf[:] = 77
                    abuf[off_a:off_a + sa.size] = sa.ravel()
                    ctx.h2d(d_a, abuf)
                    for off_z in (0, 1):
                        zbuf[:] = sentinel
                        zbuf[off_z:off_z + sz.size] = sz.ravel()
                        ctx.h2d(d_z, zbuf)
                        chk(ctx.zonal(d_a + off_a * dt.itemsize, d_z + off_z * zones.dtype.itemsize, lo, nz, None, ignore,
                                      dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1), zone_dtype=zones.dtype,
                                      zone_strides=(zrs, 1)))
                        back_a, back_z = np.empty_like(abuf), np.empty_like(zbuf)
                        ctx.d2h(back_a, d_a)
                        ctx.d2h(back_z, d_z)
                        assert back_a.tobytes() == abuf.tobytes() and back_z.tobytes() == zbuf.tobytes()
                # a host value raster with device zones, and the other way round
                chk(ctx.zonal(a, d_z + zones.dtype.itemsize, lo, nz, None, ignore, zone_dtype=zones.dtype, zone_strides=(zrs, 1)))
                chk(ctx.zonal(d_a + dt.itemsize, zones, lo, nz, None, ignore, dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1)))
            finally:
                ctx.free(d_a)
                ctx.free(d_z)


def test_two_calls_return_the_same_bytes():
    ctx = _ctx()
    rng = np.random.default_rng(3)
    for dt in (np.uint8, np.int16, np.uint32):
        a = _raster(dt, (B, 130, 517), rng)
        for pattern in ("const", "random"):
            zones, lo, nz, ignore = _zones(pattern, (130, 517), np.int16, rng)
            first = ctx.zonal(a, zones, lo, nz, None, ignore)
            second = ctx.zonal(a, zones, lo, nz, None, ignore)
            assert first[0].tobytes() == second[0].tobytes() and first[1] == second[1]


# ------------------------------------------------------------------------------- 4. refusals
def _job(ctx, a, zones, nzones=4):
    job = N.ZonalJob()
    job.src, job.src_on_device, job.dtype = a.ctypes.data, 0, N.DTYPE_CODES[a.dtype]
    job.channels, job.height, job.width = a.shape
    job.band_stride, job.row_stride, job.col_stride = a.shape[1] * a.shape[2], a.shape[2], 1
    job.zones, job.zones_on_device, job.zone_dtype = zones.ctypes.data, 0, N.DTYPE_CODES[zones.dtype]
    job.zone_row_stride, job.zone_col_stride = zones.shape[1], 1
    job.opts.nzones = nzones
    return job


REFUSALS = [
    ("dtype", 8, "bad dtype"), ("dtype", -1, "bad dtype"), ("width", 0, "bad raster layout"),
    ("channels", 0, "bad raster layout"), ("row_stride", -8, "bad raster layout"), ("zone_dtype", 6, "bad zone dtype"),
    ("zone_dtype", 7, "bad zone dtype"), ("zone_dtype", 8, "bad zone dtype"), ("zone_dtype", -1, "bad zone dtype"),
    ("zone_row_stride", -8, "bad zone layout"), ("zone_col_stride", -1, "bad zone layout"), ("nzones", 0, "nzones"),
    ("nzones", 65537, "nzones"), ("flags", 4, "unknown zonal flags"), ("height+width", (65537, 65536), "2^32 pixels"),
    ("channels+nzones", (257, 65536), "2^24 records"),
    ("src", None, "null argument"), ("zones", None, "null argument"), ("recs", None, "null argument"),
    ("outside", None, "null argument"),
]


@pytest.mark.parametrize("field,value,message", REFUSALS, ids=[f"{f}={v}" for f, v, _ in REFUSALS])
def test_refusals(field, value, message):
    """Every refusal returns FRA_E_INVALID with a message before any GPU work; one call per case."""
    ctx = _ctx()
    a = np.arange(64, dtype=np.int32).reshape(1, 8, 8)
    zones = np.zeros((8, 8), np.uint16)
    job = _job(ctx, a, zones)
    recs = np.zeros((1, 4), REC_DTYPE)
    outside = C.c_uint64()
    rp, op = C.c_void_p(recs.ctypes.data), C.byref(outside)
    if field == "height+width":
        job.height, job.width = value
    elif field == "channels+nzones":
        job.channels, job.opts.nzones = value
    elif field in ("nzones", "flags"):
        setattr(job.opts, field, value)
    elif field == "recs":
        rp = None
    elif field == "outside":
        op = None
    else:
        setattr(job, field, value)
    rc = N.load().fra_zonal(ctx.h, C.byref(job), rp, op)
    assert rc == -1 and message in N.load().fra_last_error().decode()
    assert not recs["count"].any()


def test_python_layer_refusals():
    ctx = _ctx()
    a = np.zeros((1, 8, 8), np.int16)
    with pytest.raises(ValueError):
        ctx.zonal(a, np.zeros((8, 9), np.uint8), 0, 4)
    with pytest.raises(TypeError):
        ctx.zonal(a, np.zeros((8, 8), np.int64), 0, 4)
    with pytest.raises(N.NativeError, match="bad zone dtype"):
        ctx.zonal(a, np.zeros((8, 8), np.float32), 0, 4)
    with pytest.raises(N.NativeError, match="bad zone layout"):
        ctx.zonal(a, np.zeros((8, 8), np.uint8)[:, ::-1], 0, 4)
    with pytest.raises(N.NativeError, match="nzones"):
        ctx.zonal(a, np.zeros((8, 8), np.uint8), 0, 70000)
    recs, outside = ctx.zonal(a, np.zeros((8, 8), np.uint8), 0, 4)  # the context goes on
    assert recs["count"][0].tolist() == [64, 0, 0, 0] and outside == 0


# ------------------------------------------------------------------------------- 5. behind the decoder
H, W, TILE = 150, 200, 64  # 3 x 4 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
REGIONS = {"inside one tile": (10, 70, 40, 50), "four tiles": (40, 40, 60, 51), "whole raster": (0, 0, H, W)}


def _scene(dt, bands):
    rng = np.random.default_rng(12 + bands)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(30000 + 20000 * np.sin(yy / 41.0 + b) + 8000 * np.cos(xx / 53.0) + rng.integers(0, 400, (H, W)))
                  for b in range(bands)])
    if np.dtype(dt).kind == "f":
        r = (r / 7.0).astype(dt)
        r[0, 60, 55] = np.nan
        return r
    return r.astype(dt)


def _scene_zones():
    yy, xx = np.mgrid[0:H, 0:W]
    z = ((yy // 23) * 10 + xx // 31 + 100).astype(np.uint16)  # blocks that cross the tile borders
    z[50:70, 60:80] = 999                                      # a label far above the others
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _container(dt, bands):
    from flac_raster.streaming import build_streaming

    src = _scene(dt, bands)
    data = build_streaming(src, TRANSFORM, "EPSG:32633", TILE)
    src.setflags(write=False)
    return data, src


@pytest.fixture(scope="module", params=[(np.uint16, 3), (np.float32, 1)], ids=["uint16x3", "float32x1"])
def scene(request):
    return _container(*request.param)


def test_regions_against_the_host_read(scene):
    from flac_raster.streaming import _tile_items, read_window

    data, src = scene
    nb, dt = src.shape[0], src.dtype
    ctx = _ctx()
    index, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    zones = _scene_zones()
    for sem, denorm in (("pcm16", N.DENORM_PCM16), ("int", N.DENORM_INT)):
        for name, win in REGIONS.items():
            r, c, h, w = win
            host = read_window(data, window=win, device=None, semantics=sem)[0]
            nd = float(host[0, h // 2, w // 2])
            crop = zones[r:r + h, c:c + w]  # a strided crop of a larger array: addressed relative to the region
            assert not crop.flags.c_contiguous or win == REGIONS["whole raster"]
            for lo, nz, nodata, ignore in ((100, 70, None, None), (95, 1000, nd, 999), (110, 20, None, 112)):
                recs, outside, infos = ctx.decode_device_zonal(blob, items, crop, dt, nb, win, denorm, lo, nz, nodata,
                                                               ignore)
                _check((recs, outside), host, crop, lo, nz, nodata, ignore)
                assert len(infos) == len(items)
            t = ctx.decode_timing()
            assert len(t) == 4 and t[3] >= 0.0 and ctx.zonal_timing() >= 0.0
    # device-resident zones of the whole raster, addressed from the region's first pixel
    d_z = ctx.alloc(zones.nbytes)
    try:
        ctx.h2d(d_z, np.ascontiguousarray(zones))
        r, c, h, w = REGIONS["four tiles"]
        host = read_window(data, window=(r, c, h, w), device=None)[0]
        recs, outside, _ = ctx.decode_device_zonal(blob, items, d_z + (r * W + c) * 2, dt, nb, (r, c, h, w),
                                                   N.DENORM_PCM16, 100, 70, zone_dtype=np.uint16, zone_strides=(W, 1))
        _check((recs, outside), host, zones[r:r + h, c:c + w], 100, 70)
    finally:
        ctx.free(d_z)


def test_uncovered_region_is_refused_and_the_context_goes_on(scene):
    from flac_raster.streaming import _tile_items

    data, src = scene
    nb, dt = src.shape[0], src.dtype
    ctx = _ctx()
    _, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    r, c, h, w = win = REGIONS["four tiles"]
    crop = _scene_zones()[r:r + h, c:c + w]
    hit = [k for k, it in enumerate(items) if it["window"][0] < r + h and it["window"][0] + it["window"][2] > r
           and it["window"][1] < c + w and it["window"][1] + it["window"][3] > c]
    assert len(hit) == 4
    with pytest.raises(N.NativeError, match="do not cover the region"):
        ctx.decode_device_zonal(blob, [it for k, it in enumerate(items) if k != hit[-1]], crop, dt, nb, win,
                                N.DENORM_PCM16, 100, 70)
    with pytest.raises(N.NativeError, match="bad zone dtype"):
        ctx.decode_device_zonal(blob, items, crop.astype(np.float64), dt, nb, win, N.DENORM_PCM16, 100, 70)
    recs, outside, _ = ctx.decode_device_zonal(blob, [items[k] for k in hit], crop, dt, nb, win, N.DENORM_PCM16, 100, 70)
    assert int(recs["count"][0].sum()) + outside == h * w


def test_container_zonal_on_the_device():
    from flac_raster.streaming import container_zonal

    data, src = _container(np.uint16, 3)
    zones = _scene_zones()
    wide = zones.astype(np.int32) * 100000  # labels spread too far for one call: relabelled on the way
    for win in (None, REGIONS["four tiles"]):
        for z, kw in ((zones, {}), (zones, {"nodata": float(src[0, 60, 60]), "ignore": 999}), (wide, {"ignore": 99900000}),
                      (zones.astype(np.int64), {"ignore": 999})):
            host, hw, _ = container_zonal(data, z, window=win, device=None, **kw)
            dev, dw, idx = container_zonal(data, z, window=win, device=0, **kw)
            assert hw == dw == (win or (0, 0, H, W)) and len(idx["frames"]) == 12
            assert same(dev, host)
