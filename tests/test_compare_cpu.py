"""CPU tests of the container-against-raster comparison (no GPU needed).

* the new C ABI names are declared, exported and bound; ``fra_compare_band`` is 128 bytes; ``fra_compare`` and
  ``fra_decode_device_compare`` refuse a null argument, a bad dtype, a bad layout, more than 2^32 pixels per band and
  items that do not cover the region before any GPU work.
* ``compare.compare_arrays`` is the rule: against a brute-force Python loop on tiny arrays of all eight dtypes --
  integers with Python ints, floats with ``math.fsum`` (NaN on one side and on both, +-inf, -0.0).
* ``compare_with_raster(device=None)`` and the ``check`` command on the host path, on a small container.
"""
import ctypes as C
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.compare import compare_arrays, report_from_bands
from flac_raster.geo import Affine
from flac_raster.streaming import (assemble_streaming, check_against_tiff, compare_with_raster, read_window,
                                   streaming_to_raster)
from flac_raster.tiff import write_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
NEW = ("fra_compare", "fra_decode_device_compare", "fra_compare_timing")
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
    assert "fra_compare_band" in hdr and "fra_compare_job" in hdr
    assert C.sizeof(N.CompareBand) == 128
    names = [f[0] for f in N.CompareBand._fields_]
    assert names == ["count", "differing", "unordered", "first_row", "first_col", "sum_abs", "sum_sq_lo", "sum_sq_hi",
                     "max_abs", "fsum_abs", "fsum_sq", "a_min", "a_max", "b_min", "b_max", "reserved"]
    assert [N.CompareBand._fields_[i][1] for i in (3, 4)] == [C.c_int64, C.c_int64]
    assert all(t is C.c_double for _, t in N.CompareBand._fields_[8:15])
    assert L.fra_abi_version() == 3 and re.search(r"#define\s+FRA_ABI_VERSION\s+3\b", hdr)
    assert hasattr(N.Context, "compare") and hasattr(N.Context, "decode_device_compare")
    assert C.sizeof(N.DecodeJob) == 88 and C.sizeof(N.DecodeItem) == 72  # the decode structures keep their layouts


def _compare_job():
    a = (C.c_int32 * 64)()
    b = (C.c_int32 * 64)()
    job = N.CompareJob()
    job.a, job.b, job.dtype = C.cast(a, C.c_void_p), C.cast(b, C.c_void_p), N.DTYPE_CODES[np.dtype(np.int32)]
    job.channels, job.height, job.width = 1, 8, 8
    job.a_band_stride, job.a_row_stride, job.a_col_stride = 64, 8, 1
    job.b_band_stride, job.b_row_stride, job.b_col_stride = 64, 8, 1
    return job, (a, b)


def test_compare_entry_refuses_before_any_gpu_work():
    """Every call returns FRA_E_INVALID before the context is looked at, so a stand-in pointer serves."""
    L = N.load()
    ctx = C.c_void_p(16)
    bands = (N.CompareBand * 1)()
    job, _keep = _compare_job()
    assert L.fra_compare(None, C.byref(job), bands) == -1 and b"null" in L.fra_last_error()
    assert L.fra_compare(ctx, None, bands) == -1 and b"null" in L.fra_last_error()
    assert L.fra_compare(ctx, C.byref(job), None) == -1 and b"null" in L.fra_last_error()
    for side in ("a", "b"):
        job, _keep = _compare_job()
        setattr(job, side, None)
        assert L.fra_compare(ctx, C.byref(job), bands) == -1 and b"null" in L.fra_last_error(), side
    for dt in (-1, 8):
        job, _keep = _compare_job()
        job.dtype = dt
        assert L.fra_compare(ctx, C.byref(job), bands) == -1 and b"dtype" in L.fra_last_error(), dt
    for field, v in (("channels", 0), ("height", 0), ("width", 0), ("width", -3), ("a_band_stride", -1),
                     ("a_row_stride", -1), ("a_col_stride", -1), ("b_band_stride", -1), ("b_row_stride", -8),
                     ("b_col_stride", -1)):
        job, _keep = _compare_job()
        setattr(job, field, v)
        assert L.fra_compare(ctx, C.byref(job), bands) == -1 and b"layout" in L.fra_last_error(), field
    job, _keep = _compare_job()
    job.height, job.width = 65537, 65536  # 2^32 + 2^16 pixels
    assert L.fra_compare(ctx, C.byref(job), bands) == -1 and b"2^32 pixels" in L.fra_last_error()
    assert L.fra_compare_timing(None) == -1 and b"null" in L.fra_last_error()


def _decode_job():
    data = (C.c_uint8 * 64)()
    item = N.DecodeItem()
    item.offset, item.bytes, item.window = 0, 64, N.Window(0, 0, 4, 8)
    job = N.DecodeJob()
    job.data, job.len, job.items, job.nitems = C.cast(data, C.c_void_p), 64, C.pointer(item), 1
    job.dst, job.dst_dtype, job.channels = None, N.DTYPE_CODES[np.dtype(np.int32)], 1  # dst and its strides are ignored
    return job, item, data


def test_compared_decode_refuses_before_any_gpu_work():
    L = N.load()
    ctx = C.c_void_p(16)
    job, item, _keep = _decode_job()
    infos = (N.Decoded * 1)()
    bands = (N.CompareBand * 1)()
    ref = (C.c_int32 * 64)()
    roi = N.Window(0, 0, 4, 8)

    def call(ctx=ctx, job=job, roi=roi, ref=ref, strides=(32, 8, 1), bands=bands, infos=infos):
        return L.fra_decode_device_compare(ctx, C.byref(job) if job is not None else None,
                                           C.byref(roi) if roi is not None else None,
                                           C.cast(ref, C.c_void_p) if ref is not None else None, 0, *strides, bands, infos)

    for kw in ({"ctx": None}, {"job": None}, {"roi": None}, {"ref": None}, {"bands": None}, {"infos": None}):
        assert call(**kw) == -1 and b"null" in L.fra_last_error(), kw
    for strides in ((-1, 8, 1), (32, -8, 1), (32, 8, -1)):
        assert call(strides=strides) == -1 and b"layout" in L.fra_last_error(), strides
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
    # the item covers rows 0..3 of columns 0..7; a region one row taller has an uncovered strip
    assert call(roi=N.Window(0, 0, 5, 8)) == -1 and b"do not cover the region" in L.fra_last_error()
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
def _brute(a, b):
    """One band by a Python loop: integers with Python ints, floats with math.fsum."""
    h, w = a.shape
    is_float = a.dtype.kind == "f"
    r = {"differing": 0, "unordered": 0, "one_sided_nan": 0, "first": None, "max_abs": 0.0}
    abs_terms, sq_terms, av, bv = [], [], [], []
    for i in range(h):
        for j in range(w):
            if is_float:
                x, y = float(a[i, j]), float(b[i, j])
                xn, yn = math.isnan(x), math.isnan(y)
                if not xn:
                    av.append(x)
                if not yn:
                    bv.append(y)
                if xn or yn:
                    r["unordered"] += 1
                    if xn != yn:
                        r["one_sided_nan"] += 1
                        r["differing"] += 1
                        r["first"] = r["first"] or [i, j]
                    continue
                d = 0.0 if x == y else x - y
                abs_terms.append(abs(d))
                sq_terms.append(d * d)
            else:
                x, y = int(a[i, j]), int(b[i, j])
                av.append(x)
                bv.append(y)
                d = x - y
                abs_terms.append(abs(d))
                sq_terms.append(d * d)
            if d != 0:
                r["differing"] += 1
                r["first"] = r["first"] or [i, j]
            r["max_abs"] = max(r["max_abs"], float(abs(d)))
    if is_float:
        r["sum_abs"] = math.fsum(abs_terms) if not any(map(math.isinf, abs_terms)) else math.inf
        r["sum_sq"] = math.fsum(sq_terms) if not any(map(math.isinf, sq_terms)) else math.inf
        r["tol_abs"] = len(abs_terms) * 2.0 ** -53 * r["sum_abs"]  # any order of n additions of non-negative terms
        r["tol_sq"] = len(sq_terms) * 2.0 ** -53 * r["sum_sq"]
    else:
        r["sum_abs"], r["sum_sq"] = sum(abs_terms), sum(sq_terms)
    r["a_range"] = [float(min(av)), float(max(av))] if av else [math.nan, math.nan]
    r["b_range"] = [float(min(bv)), float(max(bv))] if bv else [math.nan, math.nan]
    return r


def _same_float(x, y):
    return (x != x and y != y) or x == y


def _check_against_brute(a, b):
    rep = compare_arrays(a, b)
    is_float = a.dtype.kind == "f"
    assert rep["arrays_equal"] == np.array_equal(a, b, equal_nan=is_float)
    total_abs, total_sq, count = 0, 0, 0
    for band, x, y in zip(rep["bands"], a, b):
        want = _brute(x, y)
        for key in ("differing", "unordered", "one_sided_nan", "first"):
            assert band[key] == want[key], (key, band, want)
        assert band["count"] == x.size and band["equal"] == (want["differing"] == 0)
        assert band["max_diff"] == want["max_abs"]
        assert all(_same_float(p, q) for p, q in zip(band["file1_range"], want["a_range"])), (band, want)
        assert all(_same_float(p, q) for p, q in zip(band["file2_range"], want["b_range"])), (band, want)
        if is_float:
            for key, tol in (("sum_abs", "tol_abs"), ("sum_sq", "tol_sq")):
                if math.isinf(want[key]):
                    assert band[key] == math.inf
                else:
                    assert abs(band[key] - want[key]) <= want[tol], (key, band[key], want[key])
            assert _same_float(band["mean_diff"], band["sum_abs"] / x.size)
        else:
            assert band["sum_abs"] == want["sum_abs"] and band["sum_sq"] == want["sum_sq"]
            assert isinstance(band["sum_abs"], int) and isinstance(band["sum_sq"], int)
            assert band["mean_diff"] == want["sum_abs"] / x.size  # from the exact sums, rounded once
            assert band["rmse"] == math.sqrt(want["sum_sq"] / x.size)
            total_abs, total_sq, count = total_abs + want["sum_abs"], total_sq + want["sum_sq"], count + x.size
    if not is_float:
        assert rep["mean_difference"] == total_abs / count and rep["rmse"] == math.sqrt(total_sq / count)
    assert rep["max_difference"] == max(bd["max_diff"] for bd in rep["bands"])
    assert rep["differing"] == sum(bd["differing"] for bd in rep["bands"])
    return rep


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_compare_arrays_equals_the_brute_force_loop(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(7 + dt.num)
    for shape in ((1, 1, 1), (2, 3, 5), (3, 7, 4)):
        if dt.kind == "f":
            a = (rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 6, size=shape)).astype(dt)
            b = np.where(rng.random(shape) < 0.5, a, a + rng.normal(0.0, 1.0, size=shape).astype(dt)).astype(dt)
        else:
            info = np.iinfo(dt)
            a = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
            b = np.where(rng.random(shape) < 0.5, a,
                         rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)).astype(dt)
        _check_against_brute(a, b)
        rep = _check_against_brute(a, a.copy())
        assert rep["arrays_equal"] and rep["max_difference"] == 0.0 and rep["bands"][0]["first"] is None
    if dt.kind != "f":  # the extremes against each other: nothing wraps
        info = np.iinfo(dt)
        a, b = np.full((1, 2, 3), info.min, dt), np.full((1, 2, 3), info.max, dt)
        span = int(info.max) - int(info.min)
        for x, y in ((a, b), (b, a)):
            rep = _check_against_brute(x, y)
            assert rep["max_difference"] == float(span) and rep["bands"][0]["sum_sq"] == 6 * span * span
    assert compare_arrays(a[0], b[0])["bands"] == compare_arrays(a[:1], b[:1])["bands"]  # the (h, w) form


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_compare_arrays_nan_inf_and_negative_zero(dt):
    nan, inf = np.nan, np.inf
    a = np.array([[[nan, nan, 1.0, -0.0, inf, inf, -inf, 2.0], [3.0, 0.0, 5.0, nan, 1e30, -1.5, 0.25, 7.0]]], dt)
    b = np.array([[[nan, 1.0, nan, 0.0, inf, -inf, -inf, 2.5], [3.0, -0.0, 5.0, nan, 1e30, -1.5, 0.5, 7.0]]], dt)
    rep = _check_against_brute(a, b)
    band = rep["bands"][0]
    # both NaN x 2: unordered only; one NaN x 2: unordered and differing; -0.0 == 0.0; inf == inf; inf - -inf = inf
    assert (band["unordered"], band["one_sided_nan"], band["differing"], band["first"]) == (4, 2, 5, [0, 1])
    assert band["max_diff"] == inf and band["sum_abs"] == inf and band["sum_sq"] == inf and not rep["arrays_equal"]
    # without the infinite difference the sums are finite and exact here
    a[0, 0, 5] = -inf
    band = _check_against_brute(a, b)["bands"][0]
    assert band["differing"] == 4 and band["max_diff"] == 0.5 and band["sum_abs"] == 0.75 and band["sum_sq"] == 0.3125
    # a band without a number: NaN ranges; both NaN everywhere is equal
    c = np.full((1, 2, 2), nan, dt)
    rep = _check_against_brute(c, c.copy())
    assert rep["arrays_equal"] and rep["bands"][0]["unordered"] == 4 and math.isnan(rep["file1_min"])
    assert math.isnan(rep["bands"][0]["file2_range"][1])
    # equal apart from the zero's sign
    z = np.array([[[0.0, -0.0]]], dt)
    assert compare_arrays(z, -z)["arrays_equal"]


def test_compare_arrays_refuses_mismatches_and_builds_from_native_reports():
    with pytest.raises(ValueError):
        compare_arrays(np.zeros((1, 2, 2), np.int16), np.zeros((1, 2, 3), np.int16))
    with pytest.raises(ValueError):
        compare_arrays(np.zeros((1, 2, 2), np.int16), np.zeros((1, 2, 2), np.uint16))
    with pytest.raises(TypeError):
        compare_arrays(np.zeros((1, 2, 2), np.int64), np.zeros((1, 2, 2), np.int64))
    # the uint32 wrap of compare_tiffs' arithmetic is not repeated: 0 against 2^32 - 1
    a, b = np.zeros((1, 70, 70), np.uint32), np.full((1, 70, 70), 2**32 - 1, np.uint32)
    rep = compare_arrays(a, b)
    assert rep["max_difference"] == float(2**32 - 1) and rep["bands"][0]["sum_sq"] == 4900 * (2**32 - 1) ** 2 > 2**64
    # a native report of the same comparison gives the same dict
    r = N.CompareBand()
    r.count, r.differing, r.first_row, r.first_col = 4900, 4900, 0, 0
    r.sum_abs = 4900 * (2**32 - 1)
    r.sum_sq_lo, r.sum_sq_hi = (4900 * (2**32 - 1) ** 2) & (2**64 - 1), (4900 * (2**32 - 1) ** 2) >> 64
    r.max_abs, r.a_min, r.a_max, r.b_min, r.b_max = float(2**32 - 1), 0.0, 0.0, float(2**32 - 1), float(2**32 - 1)
    assert report_from_bands([r], np.uint32) == rep == report_from_bands([r])
    f = N.CompareBand()
    f.count, f.differing, f.unordered, f.first_row, f.first_col = 6, 2, 1, 1, 2
    f.max_abs, f.fsum_abs, f.fsum_sq, f.a_min, f.a_max, f.b_min, f.b_max = 0.5, 0.75, 0.3125, -1.0, 2.0, -1.0, 2.5
    rep = report_from_bands([f], np.float32)
    assert rep["bands"][0]["first"] == [1, 2] and rep["mean_difference"] == 0.125 and rep["one_sided_nan"] is None
    assert rep["rmse"] == math.sqrt(0.3125 / 6) and not rep["arrays_equal"]


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
    r.setflags(write=False)
    for a in full.values():
        a.setflags(write=False)
    return data, r, full


def test_host_compare_with_raster(container):
    data, src, full = container
    for sem in ("pcm16", "int"):
        rep, win, index = compare_with_raster(data, full[sem], device=None, semantics=sem)
        assert rep["arrays_equal"] and win == (0, 0, H, W) and index["height"] == H and rep["origin"] == [0, 0]
        # against the source raster the report is compare_arrays of the two
        rep, _, _ = compare_with_raster(data, src, device=None, semantics=sem)
        want = compare_arrays(full[sem], src)
        want["origin"] = [0, 0]
        assert rep == want
    assert not np.array_equal(full["pcm16"], src)  # 32767 against 32768: pcm16 does not give the integers back
    # a window: one changed pixel inside is found, relative to the window; one outside is not seen
    wdw = (40, 50, 60, 70)
    ref = full["pcm16"].copy()
    ref[1, 45, 119] += 3
    ref[0, 39, 50] += 1
    ref[0, 100, 60] += 1
    rep, win, _ = compare_with_raster(data, ref, window=wdw, device=None)
    assert win == wdw and rep["origin"] == [40, 50] and rep["differing"] == 1 and rep["max_difference"] == 3.0
    assert rep["bands"][0]["equal"] and rep["bands"][1]["first"] == [5, 69]
    assert rep == dict(compare_arrays(read_window(data, window=wdw)[0], ref[:, 40:100, 50:120]), origin=[40, 50])
    rep, win, _ = compare_with_raster(data, ref, bbox=(500500.0, 4099000.0, 501200.0, 4099600.0), device=None)
    assert win == wdw and rep["differing"] == 1
    with pytest.raises(ValueError):
        compare_with_raster(data, full["pcm16"].astype(np.int16), device=None)
    with pytest.raises(ValueError):
        compare_with_raster(data, full["pcm16"][:, :-1], device=None)
    with pytest.raises(ValueError):
        compare_with_raster(data, full["pcm16"][0], device=None)
    with pytest.raises(ValueError):
        compare_with_raster(data, full["pcm16"], device=None, semantics="float")


def test_check_cli_on_the_host(container, tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli

    data, src, full = container
    flac = tmp_path / "scene_streaming.flac"
    flac.write_bytes(data)
    monkeypatch.setattr(cli, "_gpu_present", lambda: False)  # the host path, wherever this runs
    run = lambda *args: CliRunner().invoke(cli.app, ["check", *[str(a) for a in args]])  # noqa: E731
    t = tuple(TRANSFORM)[:6]

    same = tmp_path / "same.tif"
    write_geotiff(same, full["pcm16"], transform=t, crs="EPSG:32633")
    res = run(same, flac)
    assert res.exit_code == 0, res.output
    assert "Arrays Equal" in res.output and "YES" in res.output
    assert run(same, flac, "--semantics", "int").exit_code == 1  # the other semantics give other pixels
    same_int = tmp_path / "same_int.tif"
    write_geotiff(same_int, full["int"], transform=t, crs="EPSG:32633")
    assert run(same_int, flac, "--semantics", "int").exit_code == 0

    changed = full["pcm16"].copy()
    changed[1, 45, 119] += 3
    one = tmp_path / "one.tif"
    write_geotiff(one, changed, transform=t, crs="EPSG:32633")
    out = tmp_path / "report.json"
    res = run(one, flac, "--export", out)
    assert res.exit_code == 1, res.output
    assert re.search(r"Band 2: 1 of 30000 pixels differ, the first at row\s+45, column\s+119", res.output), res.output
    rep = json.loads(out.read_text())
    assert rep["differing"] == 1 and rep["max_difference"] == 3.0 and rep["passed"] is False
    assert rep["bands"][1]["first"] == [45, 119] and rep["bands"][0]["equal"] and rep["file2"] == "one.tif"
    assert rep["file1_shape"] == [2, H, W] and rep["semantics"] == "pcm16" and rep["window"] == [0, 0, H, W]
    # either side of the actual maximum
    assert run(one, flac, "--max-diff", "3").exit_code == 0
    assert run(one, flac, "--max-diff", "2.5").exit_code == 1
    # a window that holds the pixel names it in raster coordinates, one that does not passes
    res = run(one, flac, "--window", "40,50,60,70")
    assert res.exit_code == 1 and re.search(r"row\s+45, column\s+119", res.output), res.output
    assert run(one, flac, "--window", "0,0,40,200").exit_code == 0
    assert run(one, flac, "--bbox", "500500.0,4099000.0,501200.0,4099600.0").exit_code == 1
    # the source raster itself: pcm16 is off by the 32767 / 32768 scale, within a count or two
    srcf = tmp_path / "src.tif"
    write_geotiff(srcf, src, transform=t, crs="EPSG:32633")
    rep, _, _ = check_against_tiff(flac, srcf, device=None)
    assert not rep["arrays_equal"] and rep == dict(compare_arrays(full["pcm16"], src), **{k: rep[k] for k in (
        "file1", "file2", "shape_match", "dtype_match", "crs_match", "file1_shape", "file2_shape", "file1_dtype",
        "file2_dtype", "file1_crs", "file2_crs", "origin", "window", "semantics")})
    assert rep["crs_match"] and rep["file1_dtype"] == "uint16"
    assert run(srcf, flac).exit_code == 1
    assert run(srcf, flac, "--max-diff", rep["max_difference"]).exit_code == 0
    # errors: a dtype or shape that is not the container's, a missing file, both region options
    write_geotiff(tmp_path / "i16.tif", full["pcm16"].astype(np.int16), transform=t, crs="EPSG:32633")
    write_geotiff(tmp_path / "short.tif", full["pcm16"][:, :-1], transform=t, crs="EPSG:32633")
    for name in ("i16.tif", "short.tif"):
        with pytest.raises(ValueError):
            check_against_tiff(flac, tmp_path / name, device=None)
        assert run(tmp_path / name, flac).exit_code == 1
    assert run(tmp_path / "absent.tif", flac).exit_code == 1
    assert run(same, flac, "--window", "0,0,8,8", "--bbox", "500500.0,4099000.0,501200.0,4099600.0").exit_code == 1
    assert run(same, flac, "--semantics", "float").exit_code == 1
