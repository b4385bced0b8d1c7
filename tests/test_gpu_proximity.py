"""GPU tests of the proximity unit (``k_prox_mask`` / ``k_prox_carry`` / ``k_prox_cols`` and ``k_prox_rows`` through
``fra_proximity`` and ``fra_decode_device_proximity``).

The expectation is never the kernel: it is ``proximity.proximity_arrays`` -- the separable rule in numpy, which the CPU
tests hold against the all-pairs definition -- or ``proximity.proximity_direct`` itself where stated, compared byte for
byte in ``dist`` and ``alloc``, together with the three counts.  The shapes are the project's: one pixel, less than a
chunk, several column blocks with ragged edges; (200, 70) puts several 64-row chunks and a ragged one under the column
phase, (5, 1100) rows wider than a workgroup under the row phase (a workgroup solves four rows up to 512 columns, one
row above), and (3, 32768) / (32768, 3) stand at the size limit, where the row phase needs 130 KiB of LDS.
"""
import ctypes as C
import dataclasses
from pathlib import Path

import numpy as np
import pytest

import proximity_cases as PC
from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.proximity import MAX_SIDE, Options, distance, proximity_arrays, proximity_direct

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _ctx():
    return N.default_context(0)


def _same(got, want):
    for g, w, name in zip(got[:2], want[:2], ("dist", "alloc")):
        assert (g is None) == (w is None), name
        if w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, name
            bits = f"u{g.dtype.itemsize}"
            assert g.tobytes() == w.tobytes(), (name, np.argwhere(np.ascontiguousarray(g).view(bits) != w.view(bits))[:5])
    assert [int(v) for v in got[2]] == [int(v) for v in want[2]], "counts"


def _check(ctx, a, opts=Options(), win=None, ddt="float32", ref=proximity_arrays):
    want = ref(a, opts, win, ddt)
    _same(ctx.proximity(a, opts, ddt, out_window=win), want)
    return want


# ------------------------------------------------------------------------------- 1. the kernels against the rule
@pytest.mark.parametrize("dt", PC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernels_equal_the_numpy_rule(dt):
    dt = np.dtype(dt)
    ctx = _ctx()
    shapes = PC.SMALL + ([PC.LARGE] if dt in (np.dtype(np.uint8), np.dtype(np.int16), np.dtype(np.float32)) else [])
    for shape in shapes:
        for density in PC.DENSITIES:
            a = PC.raster(shape, density, dt, seed=3)
            want = _check(ctx, a, Options(alloc_fill=-7.0))
            n = int(want[2][0])
            assert n == {"none": 0, "one": 1, "all": a.size}.get(density, n) and int(want[2][1]) == (a.size if n else 0)
    ms = ctx.proximity_timing()
    assert len(ms) == 2 and all(np.isfinite(t) and t >= 0.0 for t in ms)


@pytest.mark.parametrize("name,a", PC.seam_rasters(), ids=[n for n, _ in PC.seam_rasters()])
def test_distances_carried_across_chunks(name, a):
    """(200, 70): targets in the first row, in the last row, and on the boundaries of the 64-row chunks only."""
    ctx = _ctx()
    want = _check(ctx, a)
    assert int(want[2][0]) >= 9
    if name in ("first row", "last row"):
        assert float(want[0].max()) > 192.0   # a distance carried over three chunks
    _check(ctx, a, Options(max_dist=70.0), (60, 3, 75, 60), "uint16")


@pytest.mark.parametrize("density", ["one", "1%", "30%"])
def test_rows_wider_than_a_workgroup(density):
    ctx = _ctx()
    a = PC.raster((5, 1100), density, np.int16, seed=5)
    _check(ctx, a)
    _check(ctx, a, Options(max_dist=40.0), (1, 37, 3, 1001))
    b = PC.raster((9, 513), density, np.uint8, seed=6)   # the first width one row per workgroup takes
    _check(ctx, b)
    _check(ctx, b[:, :, :512])                             # ... and the last one of four rows per workgroup


@pytest.mark.parametrize("shape", [(3, MAX_SIDE), (MAX_SIDE, 3)], ids=["3x32768", "32768x3"])
def test_the_size_limit(shape):
    """At most 64 targets, the four ends among them, against the all-pairs definition."""
    h, w = shape
    rng = np.random.default_rng(h)
    a = np.zeros((1, h, w), np.uint16)
    rr, cc = rng.integers(0, h, 60), rng.integers(0, w, 60)
    a[0, rr, cc] = rng.integers(1, 65536, 60)
    a[0, 0, 0], a[0, h - 1, w - 1], a[0, 0, w - 1], a[0, h - 1, 0] = 1, 2, 3, 4
    ctx = _ctx()
    want = _check(ctx, a, ref=proximity_direct)
    assert int(want[2][0]) <= 64
    b = np.zeros((1, h, w), np.uint8)                       # one target at an end: the other end is 32767 away
    b[0, h - 1, w - 1] = 9
    want = _check(ctx, b, ddt="float64", ref=proximity_direct)
    assert float(want[0].max()) == float(distance(32767 ** 2 + 2 ** 2, 1.0)) and (want[1] == 9).all()


@pytest.mark.parametrize("shape", [(1, MAX_SIDE + 1), (MAX_SIDE + 1, 1)], ids=["1x32769", "32769x1"])
def test_one_over_the_limit_is_refused(shape):
    with pytest.raises(N.NativeError, match="1 .. 32768"):
        _ctx().proximity(np.ones((1,) + shape, np.uint8))


@pytest.mark.parametrize("name,a,pixel,nearest", PC.ties(), ids=[t[0] for t in PC.ties()])
def test_ties(name, a, pixel, nearest):
    ctx = _ctx()
    want = _check(ctx, a[None])
    got = ctx.proximity(a[None])
    assert got[1][0][pixel] == a[nearest] == want[1][0][pixel]
    _check(ctx, a[None], ref=proximity_direct)


# ------------------------------------------------------------------------------- 2. options and outputs
def test_outputs_alone_and_together():
    ctx = _ctx()
    a = PC.raster((33, 67), "1%", np.int32, seed=8)
    want = proximity_arrays(a, Options(), None, "float32")
    d, al, counts = ctx.proximity(a, alloc=False)
    assert al is None and d.tobytes() == want[0].tobytes() and [int(v) for v in counts] == [int(v) for v in want[2]]
    d, al, counts = ctx.proximity(a, dist=False)
    assert d is None and al.tobytes() == want[1].tobytes() and [int(v) for v in counts] == [int(v) for v in want[2]]
    _same(ctx.proximity(a), want)
    with pytest.raises(N.NativeError, match="neither dist nor alloc"):
        ctx.proximity(a, dist=False, alloc=False)


@pytest.mark.parametrize("ddt", ["float32", "float64", "uint8", "uint16"])
def test_output_dtypes(ddt):
    ctx = _ctx()
    a = PC.raster(PC.LARGE, "one", np.uint8, seed=9)
    want = _check(ctx, a, Options(scale=30.0), None, ddt)
    if ddt == "uint8":
        assert (want[0] == 255).any() and (want[0] < 255).any()   # saturated far away
    _check(ctx, PC.raster((33, 67), "none", np.uint8), Options(), None, ddt)  # the default fill: NaN, or the maximum
    _check(ctx, a, Options(scale=0.1, max_dist=7.0, fill=-3.0, alloc_fill=300.0), None, ddt)


def test_max_dist_on_a_boundary_and_fixed():
    ctx = _ctx()
    a = np.zeros((1, 40, 60), np.uint16)
    a[0, 20, 30], a[0, 3, 4] = 500, 600
    for scale in (1.0, 0.1, 10.0, 30.0):
        for d2 in (25, 50, 169, 170):
            md = float(distance(d2, scale))   # exactly a representable distance: within reach, and the next d2 is not
            want = _check(ctx, a, Options(max_dist=md, scale=scale), None, "float64")
            reached = ~np.isnan(want[0][0])
            rr, cc = np.mgrid[0:40, 0:60]
            true_d2 = np.minimum((rr - 20) ** 2 + (cc - 30) ** 2, (rr - 3) ** 2 + (cc - 4) ** 2)
            assert np.array_equal(reached, true_d2 <= d2)
    want = _check(ctx, a, Options(max_dist=5.0, fixed=1.0, fill=0.0), None, "uint8")
    assert want[0][0, 20, 30] == 1 and want[0][0, 20, 35] == 1 and want[0][0, 20, 36] == 0
    _check(ctx, a, Options(max_dist=0.0, fixed=7.5), None, "float32")
    _check(ctx, a, Options(values=(600.0, 12.0)), None, "float32")
    f = PC.raster((33, 67), "30%", np.float32, seed=2)
    assert np.isnan(f).any() and (np.signbit(f) & (f == 0)).any()
    _check(ctx, f)                                         # NaN is never a target, -0.0 is zero
    _check(ctx, f, Options(values=(0.0,)))                 # ... and -0.0 equals the value 0


def test_output_window_into_strided_destinations():
    ctx = _ctx()
    rng = np.random.default_rng(12)
    a = PC.raster(PC.LARGE, "1%", np.uint16, seed=12, bands=2)
    win = (17, 29, 90, 333)
    opts = Options(max_dist=25.0)
    want = proximity_arrays(a, opts, win, "float32")
    whole = proximity_arrays(a, opts, None, "float32")
    assert want[0].tobytes() == whole[0][:, 17:107, 29:362].tobytes()
    bigd = rng.uniform(1, 2, (2, 91, 2 * 333 + 5)).astype(np.float32)
    biga = rng.integers(1, 9, (2, 95, 333 + 3)).astype(np.uint16)
    keepd, keepa = bigd.copy(), biga.copy()
    vd, va = bigd[:, :90, :2 * 333:2], biga[:, 2:92, 3:]
    d, al, counts = ctx.proximity(a, opts, "float32", vd, va, out_window=win)
    assert d is vd and al is va
    _same((vd, va, counts), want)
    md, ma = np.ones(bigd.shape, bool), np.ones(biga.shape, bool)
    md[:, :90, :2 * 333:2], ma[:, 2:92, 3:] = False, False
    assert np.array_equal(bigd[md], keepd[md]) and np.array_equal(biga[ma], keepa[ma])
    with pytest.raises(N.NativeError, match="output window"):
        ctx.proximity(a, opts, out_window=(100, 0, 31, 10))


def test_device_sources_and_destinations():
    """Buffers of the library's own context as the source and as both destinations, with padded rows."""
    ctx = _ctx()
    h, w = PC.LARGE
    a = PC.raster(PC.LARGE, "1%", np.int16, seed=14)
    win = (5, 7, 120, 500)
    opts = Options(max_dist=60.0, alloc_fill=-1.0)
    want = proximity_arrays(a, opts, win, "float32")
    srs, drs, ars = w + 6, 500 + 3, 500
    src = np.zeros((h, srs), np.int16)
    src[:, :w] = a[0]
    dbuf, abuf = np.full(120 * drs, 99.0, np.float32), np.full(120 * ars, 99, np.int16)
    ds, dd, da = ctx.alloc(src.nbytes), ctx.alloc(dbuf.nbytes), ctx.alloc(abuf.nbytes)
    try:
        ctx.h2d(ds, src), ctx.h2d(dd, dbuf), ctx.h2d(da, abuf)
        d, al, counts = ctx.proximity(ds, opts, "float32", dd, da, out_window=win, dtype=np.int16, shape=(1, h, w),
                                      strides=(0, srs, 1), dist_strides=(0, drs, 1), alloc_strides=(0, ars, 1))
        ctx.d2h(dbuf, dd), ctx.d2h(abuf, da)
    finally:
        ctx.free(ds), ctx.free(dd), ctx.free(da)
    rows = dbuf.reshape(120, drs)
    assert rows[:, :500].tobytes() == want[0][0].tobytes() and (rows[:, 500:] == 99.0).all()
    assert abuf.reshape(120, ars).tobytes() == want[1][0].tobytes()
    assert [int(v) for v in counts] == [int(v) for v in want[2]]


def test_bands_are_handled_on_their_own():
    ctx = _ctx()
    a = np.concatenate([PC.raster((33, 67), d, np.uint8, seed=s) for s, d in enumerate(("1%", "none", "30%"))])
    want = _check(ctx, a, Options(max_dist=9.0))
    total = np.zeros(3, np.uint64)
    for b in range(3):
        one = ctx.proximity(a[b:b + 1], Options(max_dist=9.0))
        assert one[0].tobytes() == want[0][b:b + 1].tobytes() and one[1].tobytes() == want[1][b:b + 1].tobytes()
        total += one[2]
    assert [int(v) for v in total] == [int(v) for v in want[2]]


# ------------------------------------------------------------------------------- 3. refusals through ctypes
def _job(a, dist, alloc):
    job = N.ProximityJob()
    job.src, job.src_on_device, job.dtype = a.ctypes.data, 0, N.DTYPE_CODES[a.dtype]
    job.channels, job.height, job.width = a.shape
    job.band_stride, job.row_stride, job.col_stride = a.shape[1] * a.shape[2], a.shape[2], 1
    o = job.opts
    o.scale, o.out_height, o.out_width = 1.0, a.shape[1], a.shape[2]
    for dst, arr in ((o.dist, dist), (o.alloc, alloc)):
        dst.dst, dst.dtype = arr.ctypes.data, N.DTYPE_CODES[arr.dtype]
        dst.band_stride, dst.row_stride, dst.col_stride = arr.shape[1] * arr.shape[2], arr.shape[2], 1
    return job


def test_refusals_leave_the_outputs_alone():
    ctx = _ctx()
    a = PC.raster((7, 19), "30%", np.uint8, seed=1)
    dist, alloc = np.full(a.shape, 5.0, np.float32), np.full(a.shape, 5, np.uint8)
    counts = (C.c_uint64 * 3)(7, 7, 7)
    for field, value, message in (("height", 0, "1 .. 32768"), ("nvalues", 17, "nvalues"), ("scale", 0.0, "scale"),
                                  ("max_dist", -1.0, "max_dist"), ("out_width", 20, "output window")):
        job = _job(a, dist, alloc)
        job.opts.has_max_dist = 1
        setattr(job if field == "height" else job.opts, field, value)
        assert N.load().fra_proximity(ctx.h, C.byref(job), counts) == -1
        assert message in N.load().fra_last_error().decode()
        assert (dist == 5.0).all() and (alloc == 5).all() and list(counts) == [7, 7, 7]
    assert N.load().fra_proximity(ctx.h, C.byref(_job(a, dist, alloc)), None) == 0   # counts may be NULL
    assert dist.tobytes() == proximity_arrays(a)[0].tobytes()


# ------------------------------------------------------------------------------- 4. containers and polygons
H, W, TILE = 100, 120, 64  # 2 x 2 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from flac_raster.streaming import build_streaming, read_window

    rng = np.random.default_rng(21)
    src = np.zeros((2, H, W), np.uint16)
    for b in range(2):
        rr, cc = rng.integers(0, H, 40), rng.integers(0, W, 40)
        src[b, rr, cc] = rng.choice([20000, 40000, 65535], 40)
    src[0, 0, 0], src[1, H - 1, W - 1] = 65535, 65535
    path = tmp_path_factory.mktemp("proximity") / "scene_streaming.flac"
    path.write_bytes(build_streaming(src, TRANSFORM, "EPSG:32633", TILE))
    plain = read_window(path, window=(0, 0, H, W), device=None)[0]
    # the 16-bit round trip moves the values, the zeros included: the targets are the values of the plain read but its least
    vals = tuple(float(v) for v in np.unique(plain)[1:])
    assert 1 <= len(vals) <= 3 and 0 < np.isin(plain, vals).sum() < plain.size // 4
    plain.setflags(write=False)
    return path, plain, vals


def test_decode_device_proximity_on_a_container(scene):
    from flac_raster.streaming import proximity_window

    path, plain, vals = scene
    for opts, units in ((Options(vals), "pixel"), (Options(vals, max_dist=150.0, alloc_fill=9.0), "geo")):
        used = dataclasses.replace(opts, scale=10.0 if units == "geo" else 1.0)
        want = proximity_arrays(plain, used, None, "float32")
        dist, alloc, counts, win, index = proximity_window(path, opts, units=units, want_alloc=True, device=0)
        assert win == (0, 0, H, W) and len(index["frames"]) == 4
        _same((dist, alloc, counts), want)
        host = proximity_window(path, opts, units=units, want_alloc=True, device=None)
        _same(host[:3], want)
    # a window under a max_dist: the crop of the whole, from the grown region alone
    opts = Options(vals, max_dist=12.0)
    whole = proximity_arrays(plain, opts, None, "float32")
    for window in ((30, 40, 50, 60), (0, 0, 20, 30), (70, 90, 30, 30)):
        r, c, h, w = window
        dist, alloc, counts, win, _ = proximity_window(path, opts, window=window, want_alloc=True, device=0)
        assert win == window
        assert dist.tobytes() == whole[0][:, r:r + h, c:c + w].tobytes()
        assert alloc.tobytes() == whole[1][:, r:r + h, c:c + w].tobytes()
        assert int(counts[1]) == int((~np.isnan(dist)).sum()) and int(counts[1] + counts[2]) == dist.size
    dist, _, _, _, _ = proximity_window(path, Options(vals), window=(30, 40, 50, 60), device=0)   # no max_dist: the whole raster
    assert dist.tobytes() == proximity_arrays(plain, Options(vals))[0][:, 30:80, 40:100].tobytes()


def test_proximity_of_polygons():
    from flac_raster.rasterize import rasterize_arrays, read_geojson, to_pixel
    from flac_raster.streaming import proximity_of_polygons
    from flac_raster.tiff import read_geotiff

    tif, fields = ROOT / "tests" / "golden" / "sample_multispectral.tif", ROOT / "tests" / "golden" / "fields.geojson"
    _, meta = read_geotiff(tif)
    feats, values = read_geojson(fields, "field")
    pix = to_pixel(feats, Affine(*list(meta.transform)[:6]))
    labels, _ = rasterize_arrays(pix, (meta.height, meta.width), values, 0, np.uint8 if max(values) < 256 else np.int32)
    for opts in (Options(), Options(max_dist=6.0)):
        want = proximity_arrays(labels, opts, None, "float32")
        dev = proximity_of_polygons(tif, fields, "field", opts, device=0)
        host = proximity_of_polygons(tif, fields, "field", opts, device=None)
        assert dev[3] == host[3] == (0, 0, meta.height, meta.width)
        assert dev[0].tobytes() == want[0].tobytes() == host[0].tobytes()
        assert np.array_equal(dev[1], want[1]) and np.array_equal(host[1], want[1])
        assert [int(v) for v in dev[2]] == [int(v) for v in want[2]]
        assert set(np.unique(dev[1]).tolist()) <= set(int(v) for v in values) | {0}
    win = (4, 5, 20, 17)
    dev = proximity_of_polygons(tif, fields, "field", Options(max_dist=6.0), window=win, device=0)
    assert dev[0].tobytes() == want[0][:, 4:24, 5:22].tobytes() and np.array_equal(dev[1], want[1][:, 4:24, 5:22])
