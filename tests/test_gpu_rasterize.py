"""GPU tests of the polygon rasterizer (``k_rasterize`` through ``fra_rasterize``) and of the zonal statistics over
polygons, whose label raster is burned on the device and handed to ``k_zonal`` there.

The expectation is never the kernel: it is ``rasterize.rasterize_arrays`` -- the rule in numpy, checked on the CPU
against a brute-force loop -- compared byte for byte, together with ``burned``.  The shapes are those of
``test_gpu_zonal.py``: one pixel, less than a tile, several tiles with ragged edges, and (130, 517) with 9 bands of rows
and 9 tiles across.  The feature sets make the band lists empty, shorter and longer than a chunk of the kernel, and put
a feature's parity and the boundary between two features on a chunk boundary.
"""
import ctypes as C
import json

import numpy as np
import pytest

import rasterize_cases as RC
from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.rasterize import edge_table, flatten, rasterize_arrays

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32]
SMALL = [(1, 1), (7, 19), (33, 67)]
LARGE = (130, 517)
CHUNK = 128  # kChunk of fra_rasterize.hip: the edges of a band's list the workgroup takes at a time


def _ctx():
    return N.default_context(0)


def _values(n, dt, rng):
    """Burn values over the dtype's whole range, its ends among them."""
    info = np.iinfo(dt)
    v = rng.integers(info.min, int(info.max) + 1, size=n, dtype=np.int64)
    if n >= 2:
        v[0], v[-1] = info.min, info.max
    return v.tolist()


def _check(ctx, feats, window, values=None, fill=0, dt=np.int32):
    want, wburned = rasterize_arrays(feats, window, values, fill, dt)
    got, burned = ctx.rasterize(feats, window, values, fill, dt)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
    assert burned == wburned
    return want, wburned


def _band_entries(feats, row_off, band):
    """The edges of the list of one band of 16 rows: those whose [y0, y1) holds one of its row centres."""
    _, y0, _, y1, _ = edge_table(feats)
    yc = row_off + 16 * band + np.arange(16) + 0.5
    return int(((y0[:, None] <= yc[None, :]) & (yc[None, :] < y1[:, None])).any(axis=1).sum())


# ------------------------------------------------------------------------------- 1. the kernel against the rule
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_equals_the_numpy_rule(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(900 + dt.num)
    ctx = _ctx()
    shapes = SMALL + ([LARGE] if dt in (np.dtype(np.uint8), np.dtype(np.int16), np.dtype(np.uint32)) else [])
    fill = int(np.iinfo(dt).max) - 3
    for shape in shapes:
        h, w = shape
        for feats in ([], RC.triangle(h, w), RC.basic_set(h, w), RC.outside_set(h, w), RC.triangulation(h, w),
                      RC.random_quads(h, w)):
            vals = _values(len(feats), dt, rng)
            want, burned = _check(ctx, feats, shape, vals, fill, dt)
            if not feats:
                assert burned == 0 and (want == fill).all()
        assert ctx.rasterize_timing() > 0.0
    # the lists of the random quads run over a chunk on the largest shape
    if len(shapes) > 3:
        assert max(_band_entries(RC.random_quads(*LARGE), 0, b) for b in range(9)) > CHUNK
    # the triangulation: every pixel is covered
    assert ctx.rasterize(RC.triangulation(33, 67), (33, 67), None, 0, dt)[1] == 33 * 67


@pytest.mark.parametrize("nedges", [CHUNK + 7, 3 * CHUNK + 1], ids=["chunk+7", "3chunks+1"])
def test_one_features_parity_across_chunks(nedges):
    """One feature with more edges in one band's list than a chunk holds: its parity straddles the chunk boundaries."""
    ctx = _ctx()
    for shape, cy in (((16, 130), 8.0), ((33, 67), 24.0), ((40, 517), 8.0)):
        h, w = shape
        st = [RC.star(nedges, 0.5 * w, cy, 0.6 * w, 0.2, 0.1)]
        assert _band_entries(st, 0, int(cy) // 16) > nedges - 8  # chunk + 7: two chunks; 3 chunks + 1: three or four
        _check(ctx, st, shape, [77], 5, np.uint8)
        cb = [RC.comb((nedges - 1) // 2, 1.25, w - 0.75, 1.0, 14.0)]  # nedges - 1 teeth edges and 2 short ones, all in band 0
        assert _band_entries(cb, 0, 0) == (nedges - 1) // 2 * 2 + 2
        _check(ctx, cb, shape, [-9], 0, np.int16)
        _check(ctx, [RC.triangle(h, w)[0], st[0], cb[0], RC.triangle(h, w)[0]], shape, [1, 2, 3, 4], 9, np.int32)


def test_a_chunk_boundary_between_two_features():
    """The first feature fills a chunk exactly (and one edge less, and one more): the boundary between the features
    falls on, before and after the chunk boundary."""
    ctx = _ctx()
    for shape in ((16, 130), (40, 517)):
        h, w = shape
        for teeth in (CHUNK // 2 - 1, CHUNK // 2, 3 * CHUNK // 2 - 1):  # 2 teeth + 2 entries: a chunk, 2 more, 3 chunks
            first = RC.comb(teeth, 0.75, w - 1.25, 0.25, 13.75)
            assert _band_entries([first], 0, 0) == 2 * teeth + 2
            second = RC.comb(teeth + 3, 2.3, w - 0.2, 2.0, 12.0)
            for feats in ([first, second], [first, RC.triangle(h, w)[0], second, first]):
                _check(ctx, feats, shape, list(range(3, 3 + len(feats))), 0, np.uint16)


def test_vertices_on_pixel_centres_and_shared_edges():
    ctx = _ctx()
    h, w = 33, 67
    on = [[[(2.5, 2.5), (60.5, 2.5), (60.5, 30.5), (30.5, 16.5), (2.5, 30.5)]],     # vertices on centres, level edges
          [[(10.5, 5.5), (20.5, 15.5), (10.5, 25.5), (0.5, 15.5)]],                  # diagonals through centres
          [[(0.0, 0.0), (8.0, 0.0), (8.0, 8.0)]], [[(0.0, 0.0), (8.0, 8.0), (0.0, 8.0)]]]
    want, _ = _check(ctx, on, (h, w), [1, 2, 3, 4], 0, np.uint8)
    assert (want[2:8, 2:8] > 0).all()
    sq = [[[(2.5, 2.5), (10.5, 2.5), (10.5, 8.5), (2.5, 8.5)]]]
    got, burned = ctx.rasterize(sq, (12, 14))
    assert burned == 48 and (got[2:8, 2:10] == 1).all() and np.count_nonzero(got) == 48  # half-open on both axes
    tris = RC.triangulation(h, w, seed=5)
    count = np.zeros((h, w), np.int64)
    for t in tris[::3] + tris[1::3] + tris[2::3]:
        count += ctx.rasterize([t], (h, w))[0]
    assert (count == 1).all()  # a partition: no pixel twice, none missed


def test_offsets_crops_and_large_coordinates():
    ctx = _ctx()
    h, w = LARGE
    feats = RC.basic_set(h, w) + RC.random_quads(h, w, 60, seed=8)
    full, _ = _check(ctx, feats, LARGE, None, 0, np.uint16)
    for win in ((5, 9, 20, 31), (16, 64, 17, 67), (129, 516, 1, 1), (50, 3, 80, 514), (-3, -2, 40, 70)):
        r, c, hh, ww = win
        got, burned = ctx.rasterize(feats, win, None, 0, np.uint16)
        want, wburned = rasterize_arrays(feats, win, None, 0, np.uint16)
        assert got.tobytes() == want.tobytes() and burned == wburned == np.count_nonzero(got)
        if r >= 0:
            assert np.array_equal(got, full[r:r + hh, c:c + ww])
    # the same geometry moved by 2^40 pixels along both axes, with the window's offsets to match: the centres are exact
    # there, the coordinates keep 12 fractional bits
    big = float(2**40)
    moved = [[[(np.round(x * 4096) / 4096 + big, np.round(y * 4096) / 4096 + big) for x, y in ring] for ring in f]
             for f in RC.basic_set(33, 67) + RC.triangulation(33, 67)]
    _check(ctx, moved, (2**40, 2**40, 33, 67), None, 0, np.int32)
    _check(ctx, moved, (2**40 + 7, 2**40 - 5, 40, 90), None, -1, np.int16)


# ------------------------------------------------------------------------------- 2. destinations
def test_strided_host_destinations_keep_their_other_elements():
    ctx = _ctx()
    rng = np.random.default_rng(4)
    for shape in ((7, 19), (33, 67), (130, 517)):
        h, w = shape
        feats = RC.basic_set(h, w)
        for dt in (np.uint8, np.int16, np.uint32):
            want, wburned = rasterize_arrays(feats, shape, None, 0, dt)
            for pad, step in ((5, 1), (-w % 4 + 4, 1), (3, 2)):  # rows off / on the vector store's alignment; column stride 2
                big = rng.integers(1, 100, (h + 1, step * w + pad)).astype(dt)
                keep = big.copy()
                view = big[:h, :step * w:step]
                ret, burned = ctx.rasterize(feats, shape, None, 0, dt, dst=view)
                assert ret is view and burned == wburned and np.array_equal(view, want)
                mask = np.ones(big.shape, bool)
                mask[:h, :step * w:step] = False
                assert np.array_equal(big[mask], keep[mask])
    with pytest.raises(ValueError):
        ctx.rasterize(feats, (7, 19), dst=np.zeros((7, 18), np.int32))
    with pytest.raises(ValueError):
        ctx.rasterize(feats, (7, 19), dst=np.zeros((7, 19), np.int16))


def test_device_destinations_equal_the_host_one():
    """Device pointers as destinations (buffers of the context, as any framework's tensor memory would be given): tight
    rows, padded rows, and a base that rules out vector stores; what lies between and after the rows is kept."""
    ctx = _ctx()
    h, w = LARGE
    feats = RC.random_quads(h, w, 80, seed=3)
    for dt in (np.uint8, np.int16, np.int32):
        dt = np.dtype(dt)
        want, wburned = ctx.rasterize(feats, LARGE, None, 7, dt)
        assert want.tobytes() == rasterize_arrays(feats, LARGE, None, 7, dt)[0].tobytes()
        # a device buffer of the context: rows of w + 3 elements from an offset of one element (no vector stores), and tight
        for off, rs in ((1, w + 3), (0, w), (0, w + 3)):
            buf = np.full(off + h * rs, 99, dt)
            d = ctx.alloc(buf.nbytes)
            try:
                ctx.h2d(d, buf)
                ret, burned = ctx.rasterize(feats, LARGE, None, 7, dt, dst=d + off * dt.itemsize, dst_strides=(rs, 1))
                back = np.empty_like(buf)
                ctx.d2h(back, d)
            finally:
                ctx.free(d)
            assert ret is None and burned == wburned
            rows = back[off:].reshape(h, rs)
            assert np.array_equal(rows[:, :w], want) and (rows[:, w:] == 99).all() and (back[:off] == 99).all()


# ------------------------------------------------------------------------------- 3. refusals
def _job(feats, out, values, fill=0):
    xy, rs, fs = flatten(feats)
    vals = np.asarray(values, np.int64)
    job = N.RasterizeJob()
    job.xy, job.nverts, job.ring_start, job.nrings = xy.ctypes.data, xy.shape[0], rs.ctypes.data, rs.size - 1
    job.feature_ring_start, job.nfeatures, job.values = fs.ctypes.data, fs.size - 1, vals.ctypes.data
    job.dtype, job.height, job.width, job.fill = N.DTYPE_CODES[out.dtype], out.shape[0], out.shape[1], fill
    job.dst, job.dst_on_device, job.row_stride, job.col_stride = out.ctypes.data, 0, out.shape[1], 1
    return job, (xy, rs, fs, vals)


REFUSALS = [
    ("dst", None, "null argument"), ("xy", None, "null argument"), ("values", None, "null argument"),
    ("ring_start", None, "null argument"), ("feature_ring_start", None, "null argument"),
    ("dtype", 6, "bad output dtype"), ("dtype", 7, "bad output dtype"), ("dtype", -1, "bad output dtype"),
    ("height", 0, "output size"), ("width", 65537, "output size"), ("row_stride", -19, "bad output layout"),
    ("col_stride", -1, "bad output layout"), ("nfeatures", -1, "bad geometry tables"), ("nrings", 1, "feature_ring_start"),
    ("nverts", 5, "ring_start"), ("ring", 2, "has 2 vertices"), ("coordinate", np.nan, "coordinate 3"),
    ("coordinate", np.inf, "coordinate 3"), ("coordinate", 2.0**53, "coordinate 3"), ("value", 32768, "burn value 32768"),
    ("fill", -32769, "fill -32769"), ("nverts", 2**28 + 1, "2^28"),
]


@pytest.mark.parametrize("field,value,message", REFUSALS, ids=[f"{f}={v}" for f, v, _ in REFUSALS])
def test_refusals(field, value, message):
    """Every refusal returns FRA_E_INVALID with a message before any GPU work, and dst is not touched."""
    ctx = _ctx()
    out = np.full((7, 19), 55, np.int16)
    feats = [RC.triangle(7, 19)[0], [[(1.0, 1.0), (5.0, 1.5), (3.0, 6.0)]]]
    job, keep = _job(feats, out, [4, 5])
    if field == "ring":
        keep[1][1] = 2  # rings of 2 and 4 vertices
    elif field == "coordinate":
        keep[0][1, 1] = value
    elif field == "value":
        keep[3][1] = value
    else:
        setattr(job, field, value)
    burned = C.c_uint64(123)
    rc = N.load().fra_rasterize(ctx.h, C.byref(job), C.byref(burned))
    assert rc == -1 and message in N.load().fra_last_error().decode()
    assert (out == 55).all() and burned.value == 123
    got, n = ctx.rasterize(feats, (7, 19), [4, 5], 0, np.int16)  # the context goes on
    assert n == np.count_nonzero(got) > 0
    assert N.load().fra_rasterize(ctx.h, C.byref(_job(feats, out, [4, 5])[0]), None) == 0 and (out != 55).any()  # burned may be NULL


def test_python_layer_refusals():
    ctx = _ctx()
    tri = RC.triangle(7, 19)
    for kw in (dict(dtype=np.float32), dict(values=[300], dtype=np.uint8), dict(fill=-1, dtype=np.uint16)):
        with pytest.raises(ValueError):
            ctx.rasterize(tri, (7, 19), **kw)
    with pytest.raises(ValueError):
        ctx.rasterize([[[(0, 0), (1, 1)]]], (7, 19))
    with pytest.raises(ValueError):
        ctx.rasterize(tri, (0, 19))


# ------------------------------------------------------------------------------- 4. zonal statistics over polygons
H, W, TILE = 150, 200, 64  # 3 x 4 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)


def same(x, y):
    """Equality of reports in which a NaN equals a NaN."""
    if isinstance(x, dict) and isinstance(y, dict):
        return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)) and isinstance(y, (list, tuple)):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    if isinstance(x, float) and isinstance(y, float) and x != x and y != y:
        return True
    return type(x) is type(y) and x == y


def _world(feats, labels):
    """Pixel-coordinate features of the scene's grid as a GeoJSON FeatureCollection in its CRS."""
    out = []
    for f, label in zip(feats, labels):
        rings = [[[500000.0 + 10.0 * x, 4100000.0 - 10.0 * y] for x, y in ring] for ring in f]
        out.append({"type": "Feature", "properties": {"zone": label},
                    "geometry": {"type": "MultiPolygon", "coordinates": [[r] for r in rings]}})
    return {"type": "FeatureCollection", "features": out}


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from flac_raster.streaming import build_streaming

    rng = np.random.default_rng(15)
    yy, xx = np.mgrid[0:H, 0:W]
    src = np.stack([(30000 + 20000 * np.sin(yy / 41.0 + b) + 8000 * np.cos(xx / 53.0) + rng.integers(0, 400, (H, W)))
                    for b in range(3)]).astype(np.uint16)
    path = tmp_path_factory.mktemp("rasterize") / "scene_streaming.flac"
    path.write_bytes(build_streaming(src, TRANSFORM, "EPSG:32633", TILE))
    feats = RC.triangulation(H, W, 5, 4, seed=9)[:30] + RC.random_quads(H, W, 12, seed=10)
    return path, feats


@pytest.mark.parametrize("window", [None, (40, 40, 60, 51)], ids=["whole", "window"])
def test_zonal_with_polygons_on_a_container(scene, window):
    from flac_raster.streaming import zonal_with_polygons

    path, feats = scene
    near = _world(feats, [3 + (7 * i) % 40 for i in range(len(feats))])            # labels that go as they are, some shared
    far = _world(feats, [(-1) ** i * (1 + i) * 100000 for i in range(len(feats))])  # spread too far: dense ids
    for doc, attribute, nodata in ((near, "zone", None), (near, None, 30500.0), (far, "zone", None)):
        host, hw, _ = zonal_with_polygons(path, doc, attribute, window=window, nodata=nodata, device=None)
        dev, dw, idx = zonal_with_polygons(path, doc, attribute, window=window, nodata=nodata, device=0)
        assert hw == dw == (window or (0, 0, H, W)) and len(idx["frames"]) == 12
        assert same(dev, host) and len(dev[0]["zones"]) > 5


@pytest.mark.parametrize("window", [None, (40, 30, 90, 101)], ids=["whole", "window"])
def test_zonal_with_polygons_on_a_tiff(window):
    from pathlib import Path

    from flac_raster.streaming import rasterize_like, zonal_with_polygons

    root = Path(__file__).resolve().parents[1] / "tests" / "golden"
    tif, fields = root / "sample_multispectral.tif", root / "fields.geojson"
    for attribute in (None, "field"):
        host = zonal_with_polygons(tif, fields, attribute, window=window, device=None)
        dev = zonal_with_polygons(tif, fields, attribute, window=window, device=0)
        assert host[1] == dev[1] and same(dev[0], host[0]) and len(dev[0][0]["zones"]) == 3
    a = rasterize_like(tif, fields, "field", window=window, device=None)
    b = rasterize_like(tif, fields, "field", window=window, device=0)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]


def test_the_zonal_command_with_polygons(scene, tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.streaming import zonal_with_polygons

    path, feats = scene
    shapes, out = tmp_path / "fields.geojson", tmp_path / "zonal.json"
    shapes.write_text(json.dumps(_world(feats, [3 + (7 * i) % 40 for i in range(len(feats))])))
    res = CliRunner().invoke(app, ["zonal", str(path), "--zones", str(shapes), "--attribute", "zone", "--device", "0",
                                   "--export", str(out)])
    assert res.exit_code == 0, res.output
    want = zonal_with_polygons(path, shapes, "zone", device=None)[0]
    got = json.loads(out.read_text())
    assert got["device"] == 0 and len(got["bands"][0]["zones"]) == len(want[0]["zones"])
    assert same(got["bands"], json.loads(json.dumps(want)))
    tif = tmp_path / "zones.tif"
    res = CliRunner().invoke(app, ["rasterize", str(shapes), "-o", str(tif), "--like", str(path), "--device", "0"])
    assert res.exit_code == 0 and "burned:" in res.output, res.output
