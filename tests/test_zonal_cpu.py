"""CPU tests of the zonal statistics (no GPU needed).

* the new C ABI names are declared, exported and bound; ``fra_zonal_rec`` is 112 bytes in the documented order.
* ``zonal.zonal_arrays`` is the rule: against a brute-force Python loop per pixel (Python ints, ``fractions.Fraction``,
  ``math.fsum``) on small arrays of all eight dtypes with NaN, +-inf, nodata and an ignored label, negative labels, an
  empty zone inside the range and pixels below and above it; integer sums past 64 bits.
* ``dense_zones``: the no-copy case, the relabel case, the refusal, and the labels' round trip through
  ``report_from_recs``.
* ``container_zonal(device=None)`` on a small container (tiles encoded by the oracle stand-in, as the other CPU tests
  build theirs: the package's own encoder needs a GPU), ``zonal_with_tiff`` and the ``zonal`` command on the host path.
* ``make hostcheck`` with the refusals of both entries in it.
"""
import ctypes as C
import json
import math
import re
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import zonal as Z
from flac_raster.geo import Affine
from flac_raster.streaming import (assemble_streaming, container_zonal, read_window, resolve_window, tiff_zonal,
                                   zonal_with_tiff)
from flac_raster.tiff import read_geotiff, write_geotiff
from flac_raster.tiles import calculate_tiles
from flac_raster.zonal import dense_zones, report_from_recs, zonal_arrays
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
NEW = ("fra_zonal", "fra_decode_device_zonal", "fra_zonal_timing")
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TILE = 150, 200, 64  # 3 x 4 tiles, ragged right and bottom


def same(x, y):
    """Equality of reports in which a NaN equals a NaN."""
    if isinstance(x, dict) and isinstance(y, dict):
        return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)) and isinstance(y, (list, tuple)):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    if isinstance(x, float) and isinstance(y, float) and x != x and y != y:
        return True
    return type(x) is type(y) and x == y


# ------------------------------------------------------------------------------- 1. names and layout
def test_new_names_exported_declared_and_bound():
    hdr = (ROOT / "include" / "flac_raster_amd.h").read_text()
    decl = set(re.findall(r"FRA_API\s+[^;(]*?\b(fra_\w+)\s*\(", hdr))
    L = N.load()
    for name in NEW:
        assert name in decl and name in N.EXPORTS and hasattr(L, name), name
    for name in ("fra_zonal_rec", "fra_zonal_job", "fra_zonal_opts", "FRA_ZONAL_NODATA 1", "FRA_ZONAL_IGNORE 2"):
        assert name in hdr, name
    assert C.sizeof(N.ZonalRec) == 112 == Z.REC_DTYPE.itemsize and C.sizeof(N.ZonalOpts) == 32
    names = [f[0] for f in N.ZonalRec._fields_]
    assert names == ["count", "valid", "nan", "nodata", "sum_lo", "sum_hi", "sq_lo", "sq_hi", "min", "max", "fsum",
                     "mean", "fm2", "reserved"] == list(Z.REC_DTYPE.names)
    assert [N.ZonalRec.__dict__[n].offset for n in names] == [Z.REC_DTYPE.fields[n][1] for n in names]
    assert (N.ZonalJob.zones.offset, N.ZonalJob.zone_row_stride.offset, N.ZonalJob.opts.offset) == (56, 72, 88)
    assert (N.ZONAL_NODATA, N.ZONAL_IGNORE) == (Z.NODATA, Z.IGNORE) == (1, 2) and L.fra_abi_version() == 3
    for name in ("zonal", "decode_device_zonal", "zonal_timing"):
        assert hasattr(N.Context, name)
    assert L.fra_zonal_timing(None) == -1  # FRA_E_INVALID, no context needed


# ------------------------------------------------------------------------------- 2. the rule against a loop
def brute(values, zones, zone_lo, nzones, nodata=None, ignore=None):
    """The rule, pixel by pixel."""
    a = values if values.ndim == 3 else values[None]
    is_float = a.dtype.kind == "f"
    out = []
    for b in range(a.shape[0]):
        acc, outside = {}, 0
        for r in range(a.shape[1]):
            for c in range(a.shape[2]):
                z = int(zones[r, c])
                k = z - zone_lo
                if (ignore is not None and z == ignore) or not 0 <= k < nzones:
                    outside += 1
                    continue
                rec = acc.setdefault(z, {"count": 0, "nan": 0, "nodata": 0, "x": []})
                rec["count"] += 1
                x = float(a[b, r, c])
                if x != x:
                    rec["nan"] += 1
                elif nodata is not None and x == nodata:
                    rec["nodata"] += 1
                else:
                    rec["x"].append(a[b, r, c])
        zs = []
        for z in sorted(acc):
            rec = acc[z]
            xs = rec.pop("x")
            n = len(xs)
            rec.update(zone=z, valid=n, min=float(min(xs)) if n else None, max=float(max(xs)) if n else None)
            if is_float:
                f = [float(x) for x in xs]
                rec["sum_exact"] = math.fsum(f) if all(map(math.isfinite, f)) else None
                rec["abs"] = math.fsum(map(abs, f)) if rec["sum_exact"] is not None else None
                rec["x"] = f
            else:
                s, q = sum(int(x) for x in xs), sum(int(x) ** 2 for x in xs)
                rec.update(sum=s, sum_sq=q, fm2=0.0, mean=float(Fraction(s, n)) if n else math.nan,
                           variance=float(Fraction(n * q - s * s, n * n)) if n else math.nan)
                v = rec["variance"]
                rec["std"] = math.sqrt(v) if v == v else math.nan
            zs.append(rec)
        out.append({"band": b + 1, "outside": outside, "zones": zs})
    return out


def check_against_brute(got, want, is_float):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["band"], g["outside"]) == (w["band"], w["outside"])
        assert [r["zone"] for r in g["zones"]] == [r["zone"] for r in w["zones"]]
        for r, e in zip(g["zones"], w["zones"]):
            assert set(r) == set(Z.FIELDS)
            for k in ("count", "valid", "nan", "nodata"):
                assert r[k] == e[k], (k, r, e)
            assert r["count"] == r["valid"] + r["nan"] + r["nodata"]
            assert same(r["min"], e["min"]) and same(r["max"], e["max"])
            if not is_float:
                assert same({k: r[k] for k in ("sum", "sum_sq", "mean", "variance", "std", "fm2")},
                            {k: e[k] for k in ("sum", "sum_sq", "mean", "variance", "std", "fm2")}), (r, e)
                continue
            n = r["valid"]
            assert r["sum_sq"] == 0
            if n == 0:
                assert r["sum"] == 0.0 and r["fm2"] == 0.0 and math.isnan(r["mean"]) and math.isnan(r["variance"])
                continue
            with np.errstate(all="ignore"):
                assert same(r["mean"], float(np.float64(r["sum"]) / np.float64(n)))
                assert same(r["variance"], float(np.float64(r["fm2"]) / np.float64(n)))
            if e["sum_exact"] is None:
                assert not math.isfinite(r["sum"]) and not math.isfinite(r["fm2"])
                continue
            assert abs(r["sum"] - e["sum_exact"]) <= n * 2.0 ** -53 * e["abs"]
            terms = [(x - r["mean"]) ** 2 for x in e["x"]]
            t = math.fsum(terms)
            assert abs(r["fm2"] - t) <= n * 2.0 ** -53 * t


def small_case(dt, rng, h=11, w=13):
    dt = np.dtype(dt)
    if dt.kind == "f":
        a = (rng.normal(0, 1, (2, h, w)) * 10.0 ** rng.integers(-2, 4, (2, h, w))).astype(dt)
        a[0, 0, 1] = a[1, 3, 3] = np.nan
        a[0, 2, 2], a[1, 5, 6] = np.inf, -np.inf
        a[0, 4, 4] = a[0, 7, 7] = a[1, 8, 2] = -7.5
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, int(info.max) + 1, (2, h, w), dtype=np.int64).astype(dt)
        a[0, 4, 4] = a[0, 7, 7] = a[1, 8, 2] = 5
    return a


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_zonal_arrays_against_a_loop(dt):
    rng = np.random.default_rng(np.dtype(dt).num)
    a = small_case(dt, rng)
    nd = -7.5 if a.dtype.kind == "f" else 5.0
    zones = rng.integers(-4, 6, a.shape[1:]).astype(np.int16)  # negative labels
    zones[zones == 1] = 2                                       # an empty zone inside the range
    zones[0, :3] = -9                                           # below the range
    zones[1, :2] = 40                                           # above it
    zones[5, :] = 3                                             # a zone of one row: the NaN / nodata pixels aside
    for nodata in (None, nd, math.nan):
        for ignore in (None, 0):
            got = zonal_arrays(a, zones, -4, 10, nodata, ignore)
            want = brute(a, zones, -4, 10, nodata, ignore)
            check_against_brute(got, want, a.dtype.kind == "f")
            assert got[0]["outside"] == 5 + (int((zones == 0).sum()) if ignore == 0 else 0)
            assert 1 not in [r["zone"] for r in got[0]["zones"]]
    # every zone listed: the empty ones with their empty record
    full = zonal_arrays(a, zones, -4, 10, all_zones=True)
    assert [r["zone"] for r in full[0]["zones"]] == list(range(-4, 6))
    e = full[0]["zones"][5]
    assert (e["zone"], e["count"], e["valid"], e["min"], e["max"], e["sum"], e["sum_sq"]) == (1, 0, 0, None, None, 0, 0)
    assert math.isnan(e["mean"]) and math.isnan(e["std"])
    # the default range: from the smallest to the largest label that is not ignored
    d = zonal_arrays(a, zones, ignore=-9)
    assert same(d, zonal_arrays(a, zones, -4, 45, ignore=-9)) and d[0]["outside"] == 3
    # a single band given as (h, w); a zone raster of another shape or kind
    assert same(zonal_arrays(a[0], zones, -4, 10), zonal_arrays(a[:1], zones, -4, 10))
    with pytest.raises(ValueError):
        zonal_arrays(a, zones[:-1])
    with pytest.raises(TypeError):
        zonal_arrays(a, zones.astype(np.float32))
    with pytest.raises(ValueError):
        zonal_arrays(a, zones, 0, 0)


def test_all_nan_and_all_nodata_zones():
    a = np.arange(24, dtype=np.float64).reshape(1, 4, 6)
    zones = np.repeat(np.arange(4, dtype=np.uint8), 6).reshape(4, 6)
    a[0, 1] = np.nan
    a[0, 2] = 3.25
    rep = zonal_arrays(a, zones, nodata=3.25)[0]["zones"]
    assert (rep[1]["valid"], rep[1]["nan"], rep[1]["fm2"], rep[1]["sum"], rep[1]["min"]) == (0, 6, 0.0, 0.0, None)
    assert math.isnan(rep[1]["mean"]) and (rep[2]["valid"], rep[2]["nodata"]) == (0, 6) and rep[3]["mean"] == 20.5
    assert rep[0]["fm2"] == 17.5 and rep[0]["std"] == math.sqrt(17.5 / 6)


@pytest.mark.parametrize("dt", [np.uint32, np.int32], ids=lambda d: np.dtype(d).name)
def test_integer_sums_past_64_bits(dt):
    info = np.iinfo(dt)
    a = np.full((1, 70, 70), info.max, dt)  # 4900 x (2^32 - 1)^2 > 2^64
    a[0, :, 35:] = info.min
    zones = np.zeros((70, 70), np.int8)
    zones[:, 60:] = 1
    rep = zonal_arrays(a, zones)[0]["zones"]
    lo, hi = int(info.min), int(info.max)
    assert rep[0]["sum"] == 70 * 35 * hi + 70 * 25 * lo and rep[0]["sum_sq"] == 70 * 35 * hi * hi + 70 * 25 * lo * lo
    assert rep[1]["sum"] == 700 * lo and rep[1]["sum_sq"] == 700 * lo * lo
    assert rep[0]["sum_sq"] >= 1 << 64  # a 64-bit sum of squares would have wrapped
    assert rep[0]["mean"] == float(Fraction(rep[0]["sum"], 4200)) and rep[1]["variance"] == 0.0
    # ... and through the native record's 128-bit encoding
    recs = np.zeros((1, 2), Z.REC_DTYPE)
    for k, r in enumerate(rep):
        q = recs[0, k]
        q["count"] = q["valid"] = r["count"]
        s = r["sum"] & ((1 << 128) - 1)
        q["sum_lo"], q["sum_hi"] = s & ((1 << 64) - 1), (s >> 64) - (1 << 64 if s >> 127 else 0)
        q["sq_lo"], q["sq_hi"] = r["sum_sq"] & ((1 << 64) - 1), r["sum_sq"] >> 64
        q["min"], q["max"] = r["min"], r["max"]
    assert same(report_from_recs(recs, 0, dt), zonal_arrays(a, zones))


# ------------------------------------------------------------------------------- 3. dense_zones
def test_dense_zones():
    rng = np.random.default_rng(4)
    z = rng.integers(-300, 900, (20, 30)).astype(np.int32)
    got, lo, n, labels = dense_zones(z)
    assert got is z and (lo, n, labels) == (int(z.min()), int(z.max()) - int(z.min()) + 1, None)  # no copy
    zi = z.copy()
    zi[0, 0] = 10**9  # an ignored label far away does not widen the range
    got, lo, n, labels = dense_zones(zi, ignore=10**9)
    assert got is zi and labels is None and lo == int(zi.ravel()[1:].min()) and n <= 1200
    # labels spread over more than 2^16: dense ids and the label table
    wide = (z.astype(np.int64) * 100000).astype(np.int32)
    wide[3, 3] = 77
    got, lo, n, labels = dense_zones(wide, ignore=77)
    assert got.dtype == np.int32 and lo == 0 and n == labels.size == np.unique(wide[wide != 77]).size
    assert got[3, 3] == -1 and np.array_equal(labels[got[got >= 0]], wide[wide != 77])
    # the round trip of the labels through the native records
    a = rng.integers(0, 50000, (2, 20, 30)).astype(np.uint16)
    want = zonal_arrays(a, wide, ignore=77, zone_lo=int(wide.min()), nzones=int(wide.max()) - int(wide.min()) + 1)
    dense = zonal_arrays(a, got, 0, n, all_zones=True)
    recs = np.zeros((2, n), Z.REC_DTYPE)
    for b in range(2):
        for k, r in enumerate(dense[b]["zones"]):
            q = recs[b, k]
            q["count"], q["valid"], q["sum_lo"], q["sq_lo"] = r["count"], r["valid"], r["sum"], r["sum_sq"]
            q["min"], q["max"] = r["min"], r["max"]
    assert same(report_from_recs(recs, dense[0]["outside"], np.uint16, 0, labels), want)
    assert same(Z.relabel(zonal_arrays(a, got, 0, n), labels), want)
    # more than 65536 distinct labels
    many = (np.arange(70000, dtype=np.int32) * 3).reshape(350, 200)
    with pytest.raises(ValueError, match="65536"):
        dense_zones(many)
    exactly = (np.arange(65536, dtype=np.int32) * 3).reshape(256, 256)
    assert dense_zones(exactly)[2] == 65536
    # nothing but the ignored label
    assert dense_zones(np.full((2, 2), 5, np.uint8), ignore=5)[1:] == (0, 1, None)
    with pytest.raises(TypeError):
        dense_zones(np.zeros((2, 2), np.float32))


# ------------------------------------------------------------------------------- 4. containers and TIFFs on the host
@pytest.fixture(scope="module")
def container():
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(30000 + 20000 * np.sin(yy / 41.0 + b) + 8000 * np.cos(xx / 53.0) + rng.integers(0, 400, (H, W)))
                  for b in range(3)]).astype(np.uint16)
    tiles = calculate_tiles(H, W, TILE)
    streams = oracle_encode_tiles(r, tiles, level=5)
    data = assemble_streaming(tiles, streams, r.shape, r.dtype, TRANSFORM, "EPSG:32633", TILE)
    zones = ((yy // 23) * 10 + xx // 31).astype(np.uint16)  # blocks that cross the tile borders
    zones[40:60, 90:130] = 999                               # ... and a label to ignore
    r.setflags(write=False)
    zones.setflags(write=False)
    return data, r, zones


def test_host_container_zonal(container):
    data, src, zones = container
    bbox = (500500.0, 4099000.0, 501200.0, 4099600.0)
    for sem in ("pcm16", "int"):
        for kw in ({}, {"window": (50, 40, 40, 100)}, {"window": (-5, 190, 30, 40)}, {"bbox": bbox}):
            host, win, index = read_window(data, device=None, semantics=sem, **(kw or {"window": (0, 0, H, W)}))
            r, c, h, w = win
            for nodata, ignore in ((None, None), (float(host[1, h // 2, w // 2]), 999)):
                rep, got, idx = container_zonal(data, zones, nodata=nodata, ignore=ignore, device=None, semantics=sem, **kw)
                assert got == win and idx["height"] == H
                assert same(rep, zonal_arrays(host, zones[r:r + h, c:c + w], nodata=nodata, ignore=ignore))
                assert rep[0]["outside"] == (int((zones[r:r + h, c:c + w] == 999).sum()) if ignore else 0)
    assert resolve_window(index, bbox=bbox) == container_zonal(data, zones, bbox=bbox)[1]
    with pytest.raises(ValueError, match="zone raster"):
        container_zonal(data, zones[:-1])
    with pytest.raises(TypeError):
        container_zonal(data, zones.astype(np.float64))
    with pytest.raises(ValueError):
        container_zonal(data, zones, semantics="float")
    with pytest.raises(LookupError):
        container_zonal(data, zones, window=(0, W, 5, 5))


def test_zonal_with_tiff_and_the_command_on_the_host(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app

    tif = ROOT / "tests" / "golden" / "sample_multispectral.tif"
    src, meta = read_geotiff(tif)
    nb, h, w = src.shape
    yy, xx = np.mgrid[0:h, 0:w]
    zones = ((yy // 7) * 100 + xx // 9).astype(np.int32)
    zones[:3] = -1
    ztif = tmp_path / "zones.tif"
    write_geotiff(ztif, zones[None], transform=tuple(meta.transform)[:6], crs=str(meta.crs), nodata=-1)
    nd = None if meta.nodata is None else float(meta.nodata)
    want = zonal_arrays(src, zones, nodata=nd, ignore=-1)
    rep, win, info = zonal_with_tiff(tif, ztif, device=None)
    assert win == (0, 0, h, w) and info.count == nb and same(rep, want) and rep[0]["outside"] == 3 * w
    assert same(tiff_zonal(tif, zones, ignore=-1)[0], want)
    sub = (5, 4, min(20, h - 5), min(17, w - 4))
    rep, win, _ = zonal_with_tiff(tif, ztif, window=sub, ignore=zones[6, 5], nodata=7.0, device=None)
    r, c, hh, ww = sub
    assert win == sub and same(rep, zonal_arrays(src[:, r:r + hh, c:c + ww], zones[r:r + hh, c:c + ww], nodata=7.0,
                                                 ignore=int(zones[6, 5])))

    def run(*args):
        return CliRunner().invoke(app, ["zonal"] + [str(a) for a in args])

    out_json, out_csv = tmp_path / "zonal.json", tmp_path / "zonal.csv"
    res = run(tif, "--zones", ztif, "--cpu", "--export", out_json)
    assert res.exit_code == 0, res.output
    assert "Zonal statistics" in res.output or "zones.tif" in res.output
    got = json.loads(out_json.read_text())
    assert got["device"] is None and got["window"] == [0, 0, h, w] and same(got["bands"], json.loads(json.dumps(want)))
    res = run(tif, "--zones", ztif, "--cpu", "--window", ",".join(map(str, sub)), "--nodata", "7", "--ignore",
              int(zones[6, 5]), "--export", out_csv)
    assert res.exit_code == 0, res.output
    assert same(Z.read_csv_report(out_csv), rep)
    assert run(tif, "--zones", tmp_path / "absent.tif", "--cpu").exit_code == 1
    assert run(tif, "--zones", ztif, "--cpu", "--export", tmp_path / "zonal.txt").exit_code == 1
    assert run(tif, "--zones", ztif, "--cpu", "--window", "0,0,8,8", "--bbox", "0,0,1,1").exit_code == 1
    assert run(tif, "--zones", tif, "--cpu").exit_code == 1  # a zones TIFF of several bands


def test_command_on_a_container(tmp_path, container):
    from typer.testing import CliRunner

    from flac_raster.cli import app

    data, src, zones = container
    flac, ztif, out = tmp_path / "scene_streaming.flac", tmp_path / "zones.tif", tmp_path / "z.json"
    flac.write_bytes(data)
    write_geotiff(ztif, zones[None], transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    res = CliRunner().invoke(app, ["zonal", str(flac), "--zones", str(ztif), "--cpu", "--window", "50,40,40,100",
                                   "--ignore", "999", "--export", str(out)])
    assert res.exit_code == 0, res.output
    want, win, _ = container_zonal(data, zones, window=(50, 40, 40, 100), ignore=999, device=None)
    got = json.loads(out.read_text())
    assert got["window"] == list(win) and same(got["bands"], json.loads(json.dumps(want)))
    assert "more zones" not in res.output or len(want[0]["zones"]) > 50


# ------------------------------------------------------------------------------- 5. the stand-alone check program
def test_hostcheck_covers_the_zonal_refusals():
    """make hostcheck: the argument validation of the two zonal entries in the stand-alone program under
    AddressSanitizer + UBSan; no GPU."""
    csrc = ROOT / "flac-raster_amd" / "csrc"
    if not shutil.which("make") or not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("no make / hipcc")
    text = (ROOT / "tools" / "decode_host_check.cpp").read_text()
    for name in ("fra_zonal(", "fra_decode_device_zonal", "fra_zonal_timing", "bad zone dtype", "bad zone layout",
                 "nzones", "unknown zonal flags"):
        assert name in text, name
    assert "fra_zonal.hip" in (csrc / "Makefile").read_text()
    subprocess.run(["make", "-C", str(csrc), "hostcheck"], check=True, capture_output=True)
    run = subprocess.run([str(csrc / "build" / "decode_host_check"), str(ROOT / "tests" / "golden" / "sample_rgb.flac")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "argument validation checked" in run.stdout and "host check ok" in run.stdout, \
        run.stdout[-4000:] + run.stderr[-4000:]
