"""CPU tests of the polygon rasterizer (no GPU needed).

* the new C ABI names are declared, exported and bound; ``fra_rasterize_job`` is 128 bytes.
* ``rasterize.rasterize_arrays`` is the rule: against a brute-force Python loop that does the same operations in the
  same order per pixel, feature and edge; the half-open square; a jittered triangulation covers every pixel exactly
  once; invariance under ring reversal and the start vertex; painter's order; offsets equal the crop; no feature;
  every refusal.
* ``read_geojson`` and ``to_pixel``; ``zonal_with_polygons(device=None)`` and the ``rasterize`` / ``zonal`` commands on
  the host path.
"""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

import rasterize_cases as RC
from flac_raster import _native as N
from flac_raster import rasterize as RZ
from flac_raster.geo import Affine
from flac_raster.rasterize import edge_table, rasterize_arrays, read_geojson, to_pixel
from flac_raster.tiff import read_geotiff
from flac_raster.zonal import zonal_arrays

ROOT = Path(__file__).resolve().parents[1]
TIF = ROOT / "tests" / "golden" / "sample_multispectral.tif"
FIELDS = ROOT / "tests" / "golden" / "fields.geojson"
SHAPES = [(1, 1), (7, 19), (33, 67)]


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
    for name in ("fra_rasterize", "fra_rasterize_timing"):
        assert name in decl and name in N.EXPORTS and hasattr(L, name), name
    assert "fra_rasterize_job" in hdr and C.sizeof(N.RasterizeJob) == 128
    assert (N.RasterizeJob.values.offset, N.RasterizeJob.row_off.offset, N.RasterizeJob.fill.offset,
            N.RasterizeJob.dst.offset, N.RasterizeJob.col_stride.offset) == (48, 64, 88, 96, 120)
    for name in ("rasterize", "rasterize_timing"):
        assert hasattr(N.Context, name)
    assert L.fra_rasterize_timing(None) == -1  # FRA_E_INVALID, no context needed


# ------------------------------------------------------------------------------- 2. the rule
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_rasterize_arrays_against_a_loop(shape):
    h, w = shape
    for features, values in ((RC.triangle(h, w), None), (RC.basic_set(h, w), [5, -3, 9, 2, 7, 11, 13]),
                             (RC.outside_set(h, w), None)):
        got = rasterize_arrays(features, shape, values, fill=-1, dtype=np.int16)
        want = RC.brute(features, shape, values, fill=-1, dtype=np.int16)
        assert got[0].dtype == np.int16 and np.array_equal(got[0], want[0]) and got[1] == want[1]
    if shape == (33, 67):
        assert want[1] > 0 and (want[0] == -1).any()


def test_half_open_square():
    sq = [[[(2.5, 2.5), (10.5, 2.5), (10.5, 8.5), (2.5, 8.5)]]]
    out, burned = rasterize_arrays(sq, (12, 14))
    want = np.zeros((12, 14), np.int32)
    want[2:8, 2:10] = 1
    assert np.array_equal(out, want) and burned == 48


def test_a_triangulation_covers_every_pixel_once():
    h, w = 33, 67
    tris = RC.triangulation(h, w)
    count = np.zeros((h, w), np.int32)
    for t in tris:
        count += rasterize_arrays([t], (h, w))[0]
    assert (count == 1).all()
    out, burned = rasterize_arrays(tris, (h, w))
    assert burned == h * w and out.min() >= 1
    # two triangles split along a diagonal that passes through the pixel centres
    a = [[(0.0, 0.0), (8.0, 0.0), (8.0, 8.0)]]
    b = [[(0.0, 0.0), (8.0, 8.0), (0.0, 8.0)]]
    assert (rasterize_arrays([a], (8, 8))[0] + rasterize_arrays([b], (8, 8))[0] == 1).all()


def test_ring_orientation_and_start_vertex_do_not_matter():
    h, w = 33, 67
    base = RC.basic_set(h, w)
    want = rasterize_arrays(base, (h, w))
    turned = [[list(reversed(ring)) for ring in f] for f in base]
    rolled = [[ring[2:] + ring[:2] for ring in f] for f in base]
    closed = [[ring + ring[:1] for ring in f] for f in base]  # a repeated closing vertex
    for other in (turned, rolled, closed):
        got = rasterize_arrays(other, (h, w))
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    x0, y0, x1, y1, feat = edge_table(base)
    assert (y0 < y1).all() and (np.diff(feat) >= 0).all() and feat.dtype == np.int32
    tx0, ty0, tx1, ty1, _ = edge_table(turned)
    key = lambda *a: sorted(zip(*[v.tolist() for v in a]))  # noqa: E731
    assert key(x0, y0, x1, y1) == key(tx0, ty0, tx1, ty1)  # the same canonical edges, whatever the orientation
    assert edge_table(closed)[0].size == x0.size             # the edge of no length is dropped


def test_painters_order():
    sq = lambda a, b: [[(a, a), (b, a), (b, b), (a, b)]]  # noqa: E731
    out, burned = rasterize_arrays([sq(0, 6), sq(2, 8), sq(4, 10)], (10, 10), [7, 8, 9], fill=1, dtype=np.uint8)
    want = np.full((10, 10), 1, np.uint8)
    want[0:6, 0:6], want[2:8, 2:8], want[4:10, 4:10] = 7, 8, 9
    assert np.array_equal(out, want) and burned == 36 + 36 + 36 - 16 - 16


def test_offsets_equal_the_crop():
    h, w = 33, 67
    feats = RC.basic_set(h, w) + RC.triangulation(h, w)[:20]
    full, _ = rasterize_arrays(feats, (h, w))
    for win in ((5, 9, 20, 31), (16, 0, 17, 67), (32, 66, 1, 1)):
        r, c, hh, ww = win
        got, burned = rasterize_arrays(feats, win)
        assert np.array_equal(got, full[r:r + hh, c:c + ww]) and burned == np.count_nonzero(got)
    # a window at negative offsets (one of the features reaches there)
    got, burned = rasterize_arrays(feats, (-3, -2, 10, 12))
    want = RC.brute(feats, (-3, -2, 10, 12))
    assert np.array_equal(got[3:, 2:], full[:7, :10]) and np.array_equal(got, want[0]) and burned == want[1]


def test_no_feature():
    out, burned = rasterize_arrays([], (7, 19), fill=-5, dtype=np.int8)
    assert out.dtype == np.int8 and (out == -5).all() and burned == 0


def test_refusals():
    tri = RC.triangle(7, 19)
    for kw in (dict(dtype=np.float32), dict(dtype=np.int64), dict(fill=256, dtype=np.uint8), dict(values=[-1], dtype=np.uint16),
               dict(values=[1, 2]), dict(values=[1.5]), dict(fill=2**31, dtype=np.int32)):
        with pytest.raises(ValueError):
            rasterize_arrays(tri, (7, 19), **kw)
    for shape in ((0, 5), (5, 0), (65537, 1), (1, 65537), (1, 2, 3)):
        with pytest.raises(ValueError):
            rasterize_arrays(tri, shape)
    for bad in ([[[(0, 0), (1, 1)]]], [[[(0, 0), (1, np.nan), (2, 2)]]], [[[(0, 0), (np.inf, 1), (2, 2)]]],
                [[[(0, 0), (2.0**52 * 2, 1), (2, 2)]]], [[[(0, 0, 0), (1, 1, 1), (2, 2, 2)]]]):
        with pytest.raises(ValueError):
            rasterize_arrays(bad, (7, 19))
    assert rasterize_arrays([[[(0, 0), (2.0**52, 1), (2, 2)]]], (3, 3))[1] >= 0  # 2^52 itself is taken


# ------------------------------------------------------------------------------- 3. GeoJSON and the transform
def test_read_geojson():
    doc = json.loads(FIELDS.read_text())
    feats, vals = read_geojson(FIELDS)
    assert vals == [1, 2, 3] and [len(f) for f in feats] == [2, 3, 1]
    assert feats[0][0].shape == (5, 2) and feats[1][2].shape == (3, 2) and feats[0][0].dtype == np.float64
    assert feats[1][1][0].tolist() == [-74.98893, 34.98877]
    assert read_geojson(doc, "field")[1] == [7, 300, 12]
    one = read_geojson(doc["features"][1])  # a Feature, a MultiPolygon with a hole
    assert one[1] == [1] and len(one[0][0]) == 3
    bare = read_geojson(doc["features"][0]["geometry"])
    assert bare[1] == [1] and len(bare[0][0]) == 2
    with pytest.raises(ValueError, match="LineString"):
        read_geojson({"type": "LineString", "coordinates": [[0, 0], [1, 1]]})
    with pytest.raises(ValueError, match="Point"):
        read_geojson({"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {},
                                                                 "geometry": {"type": "Point", "coordinates": [0, 0]}}]})
    with pytest.raises(ValueError, match="area_ha"):
        read_geojson(doc, "area_ha")
    with pytest.raises(ValueError, match="name"):
        read_geojson(doc, "name")
    with pytest.raises(ValueError, match="absent"):
        read_geojson(doc, "absent")
    assert read_geojson({"type": "FeatureCollection", "features": []}) == ([], [])


def test_to_pixel():
    t = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
    world = [[[(500000.0, 4100000.0), (500025.0, 4099990.0), (500100.0, 4099875.0)]]]
    assert to_pixel(world, t)[0][0].tolist() == [[0.0, 0.0], [2.5, 1.0], [10.0, 12.5]]
    # with rotation terms: x = 2 col + row + 10, y = col - 3 row + 20; (col, row) = (3, 4) -> (20, 11)
    assert to_pixel([[[(20.0, 11.0), (10.0, 20.0), (12.0, 21.0)]]], (2.0, 1.0, 10.0, 1.0, -3.0, 20.0))[0][0].tolist() == \
        [[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]]
    with pytest.raises(ValueError):
        to_pixel(world, (1.0, 2.0, 0.0, 2.0, 4.0, 0.0))


# ------------------------------------------------------------------------------- 4. zonal statistics over polygons
def test_zonal_with_polygons_on_the_host():
    from flac_raster.streaming import rasterize_like, zonal_with_polygons

    src, meta = read_geotiff(TIF)
    _, h, w = src.shape
    feats, vals = read_geojson(FIELDS, "field")
    pix = to_pixel(feats, Affine(*tuple(meta.transform)[:6]))
    zones, burned = rasterize_arrays(pix, (h, w), vals, 0, np.uint16)
    assert set(np.unique(zones).tolist()) == {0, 7, 12, 300} and burned == np.count_nonzero(zones)
    want = zonal_arrays(src, zones, nodata=None, ignore=0)
    rep, win, info = zonal_with_polygons(TIF, FIELDS, "field", device=None)
    assert win == (0, 0, h, w) and info.count == src.shape[0] and same(rep, want)
    assert [r["zone"] for r in rep[0]["zones"]] == [7, 12, 300] and rep[0]["outside"] == h * w - burned
    sub = (40, 30, 90, 101)
    r, c, hh, ww = sub
    rep, win, _ = zonal_with_polygons(TIF, FIELDS, "field", window=sub, nodata=7.0, device=None)
    assert win == sub and same(rep, zonal_arrays(src[:, r:r + hh, c:c + ww], zones[r:r + hh, c:c + ww], nodata=7.0, ignore=0))
    # without an attribute: feature i is zone i + 1
    plain, _ = rasterize_arrays(pix, (h, w))
    assert same(zonal_with_polygons(TIF, FIELDS, device=None)[0], zonal_arrays(src, plain, ignore=0))
    # labels spread too far for one call are burned as dense ids and come back as labels
    doc = json.loads(FIELDS.read_text())
    for f, v in zip(doc["features"], (5, 7_000_000_000, -90_000)):
        f["properties"]["field"] = v
    rep = zonal_with_polygons(TIF, doc, "field", device=None)[0]
    assert [r["zone"] for r in rep[0]["zones"]] == [-90_000, 5, 7_000_000_000]
    by_label = {r["zone"]: r for r in rep[0]["zones"]}
    for label, first in ((5, 1), (7_000_000_000, 2), (-90_000, 3)):
        assert by_label[label]["count"] == int(np.count_nonzero(plain == first))
    doc["features"][0]["properties"]["field"] = 0
    with pytest.raises(ValueError, match="label of 0"):
        zonal_with_polygons(TIF, doc, "field", device=None)
    # the raster alone
    raster, win, transform, crs = rasterize_like(TIF, FIELDS, "field", window=sub, device=None)
    assert raster.dtype == np.uint16 and np.array_equal(raster, zones[r:r + hh, c:c + ww]) and crs == "EPSG:4326"
    assert transform == pytest.approx((0.0001, 0.0, -75.0 + 30 * 0.0001, 0.0, -0.0001, 35.0 - 40 * 0.0001))


def test_commands_on_the_host(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.streaming import zonal_with_polygons

    src, meta = read_geotiff(TIF)
    _, h, w = src.shape
    feats, vals = read_geojson(FIELDS, "field")
    pix = to_pixel(feats, Affine(*tuple(meta.transform)[:6]))
    run = lambda *args: CliRunner().invoke(app, [str(a) for a in args])  # noqa: E731
    out = tmp_path / "zones.tif"
    res = run("rasterize", FIELDS, "-o", out, "--like", TIF, "--attribute", "field", "--cpu")
    assert res.exit_code == 0, res.output
    zones, burned = rasterize_arrays(pix, (h, w), vals, 0, np.uint16)
    back, info = read_geotiff(out)
    assert back.dtype == np.uint16 and np.array_equal(back[0], zones) and float(info.nodata) == 0.0
    assert tuple(info.transform)[:6] == tuple(meta.transform)[:6] and f"burned: {burned} pixels" in res.output
    res = run("rasterize", FIELDS, "-o", out, "--like", TIF, "--burn", "1", "--fill", "255", "--dtype", "uint8", "--cpu",
              "--window", "40,30,90,101")
    assert res.exit_code == 0, res.output
    back, info = read_geotiff(out)
    mask = rasterize_arrays(pix, (40, 30, 90, 101), [1, 1, 1], 255, np.uint8)[0]
    assert back.dtype == np.uint8 and np.array_equal(back[0], mask) and float(info.nodata) == 255.0
    assert run("rasterize", FIELDS, "-o", out, "--like", TIF, "--burn", "1", "--attribute", "field", "--cpu").exit_code == 1
    assert run("rasterize", FIELDS, "-o", out, "--like", TIF, "--attribute", "field", "--dtype", "uint8", "--cpu").exit_code == 1
    assert run("rasterize", tmp_path / "absent.geojson", "-o", out, "--like", TIF, "--cpu").exit_code == 1
    # the zonal command with polygons
    exported = tmp_path / "zonal.json"
    res = run("zonal", TIF, "--zones", FIELDS, "--attribute", "field", "--cpu", "--export", exported)
    assert res.exit_code == 0, res.output
    want = zonal_with_polygons(TIF, FIELDS, "field", device=None)[0]
    got = json.loads(exported.read_text())
    assert got["window"] == [0, 0, h, w] and same(got["bands"], json.loads(json.dumps(want)))
    assert run("zonal", TIF, "--zones", FIELDS, "--ignore", "7", "--cpu").exit_code == 1
    assert run("zonal", TIF, "--zones", out, "--attribute", "field", "--cpu").exit_code == 1
