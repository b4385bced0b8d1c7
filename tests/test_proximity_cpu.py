"""CPU tests of the proximity feature: the rule in numpy and everything around the kernels that needs no GPU.

* ``proximity_arrays`` (columns, then rows) against ``proximity_direct`` (all pairs) in the bytes of ``dist`` and of
  ``alloc``, over the shapes and target densities the issue names; hand-made ties that pin the nearest target.
* The options: the value list against the non-zero default, NaN and -0.0, ``max_dist`` on a representable distance,
  ``fixed``, integer ``dist`` dtypes, the output window under a ``max_dist``.
* Every refusal of ``fra_proximity`` through ctypes, in the header's order, with a context that is never dereferenced.
* ``proximity_window`` over a container (tiles encoded by the oracle stand-in, as the other CPU tests build theirs),
  ``proximity_tiff``, ``proximity_of_polygons`` and the ``proximity`` command on the host path.
* ``make hostcheck`` with the refusals, the reach threshold and the launch plan in it.
"""
import ctypes as C
import dataclasses
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import proximity_cases as PC
from flac_raster import _native as N
from flac_raster import proximity as P
from flac_raster.geo import Affine
from flac_raster.proximity import Options, distance, proximity_arrays, proximity_direct
from flac_raster.streaming import (assemble_streaming, proximity_of_polygons, proximity_tiff, proximity_to_tiff,
                                   proximity_window, read_window)
from flac_raster.tiff import read_geotiff, write_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
NEW = ("fra_proximity", "fra_decode_device_proximity", "fra_proximity_timing")
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TILE = 100, 120, 64  # 2 x 2 tiles, ragged right and bottom


def _equal(x, y):
    assert x[0].dtype == y[0].dtype and x[0].tobytes() == y[0].tobytes(), "dist"
    assert x[1].dtype == y[1].dtype and x[1].tobytes() == y[1].tobytes(), "alloc"
    assert [int(v) for v in x[2]] == [int(v) for v in y[2]], "counts"


# ------------------------------------------------------------------------------- 1. names and layout
def test_new_names_exported_declared_and_bound():
    hdr = (ROOT / "include" / "flac_raster_amd.h").read_text()
    decl = set(re.findall(r"FRA_API\s+[^;(]*?\b(fra_\w+)\s*\(", hdr))
    L = N.load()
    for name in NEW:
        assert name in decl and name in N.EXPORTS and hasattr(L, name), name
    assert "fra_proximity_opts" in hdr and "fra_proximity_job" in hdr
    assert C.sizeof(N.ProximityOpts) == 280 and N.ProximityOpts.values.offset == 32 and N.ProximityOpts.dist.offset == 200


# ------------------------------------------------------------------------------- 2. the two forms of the rule
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (7, 19), (33, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("density", PC.DENSITIES)
def test_the_separable_form_equals_the_definition(shape, density):
    for dt in (np.uint8, np.int16, np.float32):
        a = PC.raster(shape, density, dt, seed=1, bands=2)
        for opts in (Options(), Options(max_dist=4.0, alloc_fill=-1.0), Options(scale=30.0, max_dist=100.0)):
            _equal(proximity_arrays(a, opts, None, "float64"), proximity_direct(a, opts, None, "float64"))


@pytest.mark.parametrize("name,a,pixel,nearest", PC.ties(), ids=[t[0] for t in PC.ties()])
def test_ties(name, a, pixel, nearest):
    for f in (proximity_direct, proximity_arrays):
        dist, alloc, _ = f(a)
        assert alloc[0][pixel] == a[nearest], (f.__name__, alloc[0][pixel])
        d2 = (pixel[0] - nearest[0]) ** 2 + (pixel[1] - nearest[1]) ** 2
        assert dist[0][pixel] == np.float32(np.sqrt(float(d2)))
    # the tie is a tie: another target of the raster lies at the same distance
    rr, cc = np.nonzero(a)
    assert ((rr - pixel[0]) ** 2 + (cc - pixel[1]) ** 2 == d2).sum() >= 2


def test_values_nan_and_negative_zero():
    a = np.array([[[0.0, -0.0, np.nan, 2.0, 0.0, 0.0, 7.0, np.nan, 0.0]]], np.float32)
    for f in (proximity_direct, proximity_arrays):
        dist, alloc, counts = f(a)                       # non-zero and not NaN: columns 3 and 6
        assert counts.tolist() == [2, 9, 0]
        assert dist[0, 0].tolist() == [3, 2, 1, 0, 1, 1, 0, 1, 2] and alloc[0, 0].tolist() == [2, 2, 2, 2, 2, 7, 7, 7, 7]
        dist, alloc, counts = f(a, Options(values=(7.0,)))
        assert counts[0] == 1 and dist[0, 0].tolist() == [6, 5, 4, 3, 2, 1, 0, 1, 2]
        dist, alloc, counts = f(a, Options(values=(0.0, 2.0)))   # -0.0 == 0.0; NaN equals nothing
        assert counts[0] == 6 and dist[0, 0].tolist() == [0, 0, 1, 0, 0, 0, 1, 1, 0]
        assert np.signbit(alloc[0, 0, 1]) and alloc[0, 0, 2] == 0.0 and not np.signbit(alloc[0, 0, 7])  # bits copied
        dist, alloc, counts = f(np.full((1, 3, 3), np.nan))
        assert counts.tolist() == [0, 0, 9] and np.isnan(dist).all() and (alloc == 0).all()
    i = np.array([[[0, 5, 0, -5, 0]]], np.int8)
    assert proximity_arrays(i, Options(values=(-5.0,)))[0][0, 0].tolist() == [3, 2, 1, 0, 1]
    assert proximity_arrays(i, Options(values=(5.5,)))[2][0] == 0


def test_max_dist_on_a_representable_distance():
    a = np.zeros((1, 40, 60), np.uint8)
    a[0, 20, 30] = 1
    rr, cc = np.mgrid[0:40, 0:60]
    true_d2 = (rr - 20) ** 2 + (cc - 30) ** 2
    for scale in (1.0, 0.1, 10.0, 30.0):
        for d2 in (1, 25, 50, 169, 170, 400):
            md = float(distance(d2, scale))
            opts = Options(max_dist=md, scale=scale)
            assert P.reach_threshold(opts) == d2
            for f in (proximity_direct, proximity_arrays):
                dist, _, counts = f(a, opts, None, "float64")
                assert np.array_equal(~np.isnan(dist[0]), true_d2 <= d2) and int(counts[1]) == int((true_d2 <= d2).sum())
            assert P.reach_threshold(Options(max_dist=float(np.nextafter(md, 0.0)), scale=scale)) == d2 - 1
    assert P.reach_threshold(Options()) == P.MAX_D2 == P.reach_threshold(Options(max_dist=float("inf")))
    assert P.halo(Options(max_dist=5.0)) == 5 and P.halo(Options(max_dist=5.5)) == 6 and P.halo(Options(max_dist=0.0)) == 0
    assert P.halo(Options(max_dist=100.0, scale=30.0)) == 4 and P.halo(Options()) is None


def test_fixed_fill_and_integer_outputs():
    a = np.zeros((1, 9, 400), np.uint16)
    a[0, 4, 10] = 777
    for f in (proximity_direct, proximity_arrays):
        dist, alloc, counts = f(a, Options(max_dist=3.0, fixed=1.0, fill=0.0, alloc_fill=5.0), None, "uint8")
        assert dist[0, 4, 10] == 1 and dist[0, 4, 13] == 1 and dist[0, 4, 14] == 0 and dist[0, 1, 10] == 1 and dist[0, 0, 10] == 0
        assert alloc[0, 4, 13] == 777 and alloc[0, 4, 14] == 5 and int(counts[1]) == int((dist == 1).sum()) == 29
        dist = f(a, Options(), None, "uint8")[0]            # to_out: half to even, saturated
        assert dist[0, 4, 399] == 255 and dist[0, 4, 265] == 255 and dist[0, 4, 264] == 254 and dist[0, 3, 11] == 1
        assert dist[0, 2, 12] == 3 and dist[0, 6, 12] == 3   # sqrt(8) = 2.83 -> 3
        assert f(a, Options(scale=0.5), None, "int16")[0][0, 4, 15] == 2       # 2.5 -> 2
        assert f(a, Options(scale=0.5), None, "int16")[0][0, 4, 17] == 4       # 3.5 -> 4
        none = f(np.zeros((1, 2, 2), np.uint8), Options(), None, "uint16")
        assert (none[0] == 65535).all() and (none[1] == 0).all()               # the default fill: the dtype's maximum
        assert np.isnan(f(np.zeros((1, 2, 2), np.uint8))[0]).all()              # ... NaN for a float output
        assert (f(np.zeros((1, 2, 2), np.int8), Options(alloc_fill=-200.0))[1] == -128).all()


@pytest.mark.parametrize("window", [(0, 0, 20, 31), (40, 50, 33, 41), (100, 440, 30, 77)], ids=["corner", "middle", "far corner"])
def test_a_grown_window_is_the_crop_of_the_whole(window):
    a = PC.raster(PC.LARGE, "1%", np.uint16, seed=4)
    Hh, Ww = PC.LARGE
    for opts in (Options(max_dist=9.0), Options(max_dist=250.0, scale=30.0), Options(max_dist=0.0)):
        whole = proximity_arrays(a, opts, None, "float32")
        k = P.halo(opts)
        assert k == int(np.ceil(opts.max_dist / opts.scale))
        r, c, h, w = window
        r0, c0, r1, c1 = max(r - k, 0), max(c - k, 0), min(r + h + k, Hh), min(c + w + k, Ww)
        part = proximity_arrays(a[:, r0:r1, c0:c1], opts, (r - r0, c - c0, h, w), "float32")
        assert part[0].tobytes() == whole[0][:, r:r + h, c:c + w].tobytes()
        assert part[1].tobytes() == whole[1][:, r:r + h, c:c + w].tobytes()
        _equal(proximity_arrays(a, opts, window, "float32")[:2] + (part[2][1:],),
               (part[0], part[1], proximity_direct(a, opts, window, "float32")[2][1:]))


def test_python_layer_refusals():
    a = np.ones((1, 3, 3), np.uint8)
    for opts in (Options(values=tuple(range(17))), Options(values=(float("nan"),)), Options(scale=0.0),
                 Options(scale=float("inf")), Options(max_dist=-1.0), Options(max_dist=float("nan"))):
        with pytest.raises(ValueError):
            proximity_arrays(a, opts)
    for win in ((0, 0, 0, 3), (1, 1, 3, 3), (-1, 0, 2, 2)):
        with pytest.raises(ValueError, match="output window"):
            proximity_direct(a, Options(), win)
    with pytest.raises(ValueError):
        proximity_arrays(np.ones((3,), np.uint8))
    assert P.scale_of(None, "pixel") == 1.0 and P.scale_of(list(TRANSFORM)[:6], "geo") == 10.0
    with pytest.raises(ValueError, match="rotated"):
        P.scale_of([10.0, 1.0, 0.0, 0.0, -10.0, 0.0], "geo")
    with pytest.raises(ValueError, match="anisotropic"):
        P.scale_of([10.0, 0.0, 0.0, 0.0, -20.0, 0.0], "geo")
    with pytest.raises(ValueError):
        P.scale_of(None, "geo")
    with pytest.raises(ValueError):
        P.scale_of(list(TRANSFORM)[:6], "metres")


# ------------------------------------------------------------------------------- 3. the library's refusals, without a GPU
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


# (what to break, the message): in the header's order; each later entry is also broken in every earlier case's job
REFUSALS = [
    (lambda j: setattr(j, "src", None), "null argument"),
    (lambda j: setattr(j, "dtype", 8), "bad dtype 8"),
    (lambda j: setattr(j, "channels", 256), "more than 255"),
    (lambda j: setattr(j.opts.dist, "dtype", -1), "bad dist dtype"),
    (lambda j: setattr(j.opts.dist, "row_stride", -1), "bad dist layout"),
    (lambda j: setattr(j.opts.alloc, "col_stride", -1), "bad alloc layout"),
    (lambda j: setattr(j, "height", 32769), "1 .. 32768"),
    (lambda j: setattr(j.opts, "nvalues", 17), "nvalues"),
    (lambda j: (setattr(j.opts, "nvalues", 1), j.opts.values.__setitem__(0, float("inf"))), "target value 0 is not finite"),
    (lambda j: setattr(j.opts, "scale", float("nan")), "scale"),
    (lambda j: (setattr(j.opts, "has_max_dist", 1), setattr(j.opts, "max_dist", -0.25)), "max_dist"),
    (lambda j: setattr(j.opts, "out_width", 20), "output window"),
    (lambda j: (setattr(j.opts.dist, "dst", None), setattr(j.opts.alloc, "dst", None)), "neither dist nor alloc"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[m for _, m in REFUSALS])
def test_refusals_in_the_stated_order(k):
    """FRA_E_INVALID with its message before any GPU work (the context is never dereferenced); a job that breaks this
    rule and every later one gets this rule's message."""
    L = N.load()
    ctx = C.c_void_p(16)
    a = np.ones((2, 7, 19), np.uint8)
    dist, alloc = np.full(a.shape, 5.0, np.float32), np.full(a.shape, 5, np.uint8)
    counts = (C.c_uint64 * 3)(7, 7, 7)
    for later in (False, True):
        job = _job(a, dist, alloc)
        if later:
            outputs = REFUSALS[k][1] in ("bad dist dtype", "bad dist layout", "bad alloc layout")
            for brk, _ in REFUSALS[k + 1:len(REFUSALS) - outputs]:  # (an output is looked at only when it is given)
                brk(job)
        REFUSALS[k][0](job)
        assert L.fra_proximity(ctx, C.byref(job), counts) == -1
        assert REFUSALS[k][1] in L.fra_last_error().decode(), (later, L.fra_last_error())
    assert (dist == 5.0).all() and (alloc == 5).all() and list(counts) == [7, 7, 7]
    assert L.fra_proximity(None, C.byref(_job(a, dist, alloc)), counts) == -1
    assert L.fra_proximity(ctx, None, counts) == -1 and L.fra_proximity_timing(None) == -1
    ms = (C.c_float * 2)(-1.0, -1.0)
    assert L.fra_proximity_timing(ms) == 0 and ms[0] >= 0.0 and ms[1] >= 0.0


def test_the_read_refers_to_the_windowed_read():
    L = N.load()
    ctx = N.Context.__new__(N.Context)
    ctx.h = C.c_void_p(16)
    try:
        o = N.ProximityOpts()
        o.scale, o.out_height, o.out_width = 1.0, 4, 8
        out = np.zeros((1, 5, 8), np.float32)
        o.dist.dst, o.dist.dtype, o.dist.band_stride, o.dist.row_stride, o.dist.col_stride = out.ctypes.data, N.DTYPE_CODES[out.dtype], 40, 8, 1
        items = [{"offset": 0, "bytes": 10, "window": (0, 0, 4, 8)}]
        job, infos, keep = ctx._decode_job(b"\0" * 10, items, None, np.int32, N.DENORM_NONE, 1, (0, 0, 0))
        counts = (C.c_uint64 * 3)()
        rc = L.fra_decode_device_proximity(ctx.h, C.byref(job), C.byref(N.Window(0, 0, 4, 0)), C.byref(o), infos, counts)
        assert rc == -1 and "region of interest" in L.fra_last_error().decode()
        assert L.fra_decode_device_proximity(ctx.h, C.byref(job), C.byref(N.Window(0, 0, 4, 8)), None, infos, counts) == -1
        o.scale = -1.0
        rc = L.fra_decode_device_proximity(ctx.h, C.byref(job), C.byref(N.Window(0, 0, 4, 8)), C.byref(o), infos, counts)
        assert rc == -1 and "scale" in L.fra_last_error().decode()
        o.scale, o.out_height = 1.0, 5
        rc = L.fra_decode_device_proximity(ctx.h, C.byref(job), C.byref(N.Window(0, 0, 5, 8)), C.byref(o), infos, counts)
        assert rc == -1 and "do not cover" in L.fra_last_error().decode()
    finally:
        ctx.h = None


# ------------------------------------------------------------------------------- 4. containers, TIFFs, polygons, the command
@pytest.fixture(scope="module")
def container():
    rng = np.random.default_rng(21)
    src = np.zeros((2, H, W), np.uint16)
    for b in range(2):
        rr, cc = rng.integers(0, H, 40), rng.integers(0, W, 40)
        src[b, rr, cc] = rng.choice([20000, 40000, 65535], 40)
    src[0, 0, 0], src[1, H - 1, W - 1] = 65535, 65535
    tiles = calculate_tiles(H, W, TILE)
    data = assemble_streaming(tiles, oracle_encode_tiles(src, tiles, level=5), src.shape, src.dtype, TRANSFORM, "EPSG:32633", TILE)
    plain = read_window(data, window=(0, 0, H, W), device=None)[0]
    # the 16-bit round trip moves the values, the zeros included: the targets are the values of the plain read but its least
    vals = tuple(float(v) for v in np.unique(plain)[1:])
    assert 1 <= len(vals) <= 3 and 0 < np.isin(plain, vals).sum() < plain.size // 4
    plain.setflags(write=False)
    return data, plain, vals


def test_proximity_window_on_the_host(container):
    data, plain, vals = container
    for opts, units, scale in ((Options(vals), "pixel", 1.0), (Options(vals, max_dist=150.0, alloc_fill=9.0), "geo", 10.0)):
        want = proximity_arrays(plain, dataclasses.replace(opts, scale=scale), None, "float32")
        dist, alloc, counts, win, index = proximity_window(data, opts, units=units, want_alloc=True, device=None)
        assert win == (0, 0, H, W) and len(index["frames"]) == 4
        _equal((dist, alloc, counts), want)
    opts = Options(vals, max_dist=12.0)
    whole = proximity_arrays(plain, opts, None, "uint16")
    for window in ((30, 40, 50, 60), (0, 0, 20, 30), (70, 90, 30, 30)):
        r, c, h, w = window
        dist, alloc, counts, win, _ = proximity_window(data, opts, window=window, dist_dtype="uint16", want_alloc=True)
        assert win == window and dist.tobytes() == whole[0][:, r:r + h, c:c + w].tobytes()
        assert alloc.tobytes() == whole[1][:, r:r + h, c:c + w].tobytes()
    dist, alloc, _, _, _ = proximity_window(data, Options(vals), window=(30, 40, 50, 60))   # no max_dist: the whole raster is read
    assert alloc is None and dist.tobytes() == proximity_arrays(plain, Options(vals))[0][:, 30:80, 40:100].tobytes()
    with pytest.raises(ValueError):
        proximity_window(data, Options(), semantics="float")


def test_tiffs_polygons_and_the_command_on_the_host(tmp_path, container):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.rasterize import rasterize_arrays, read_geojson, to_pixel

    data, plain, vals = container
    tif = tmp_path / "targets.tif"
    write_geotiff(tif, plain, transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    opts = Options(vals, max_dist=80.0, fill=-1.0)
    want = proximity_arrays(plain, dataclasses.replace(opts, scale=10.0), None, "float32")
    dist, alloc, counts, win, info, used = proximity_tiff(tif, opts, units="geo", want_alloc=True)
    assert used.scale == 10.0 and win == (0, 0, H, W)
    _equal((dist, alloc, counts), want)
    sub = (10, 20, 40, 50)
    d2 = proximity_tiff(tif, opts, window=sub, units="geo")[0]
    assert d2.tobytes() == want[0][:, 10:50, 20:70].tobytes()

    flac, out, out_alloc = tmp_path / "scene_streaming.flac", tmp_path / "dist.tif", tmp_path / "nearest.tif"
    flac.write_bytes(data)

    def run(*args):
        return CliRunner().invoke(app, ["proximity"] + [str(a) for a in args])

    for source in (flac, tif):
        res = run(source, "-o", out, "--values", ",".join(str(v) for v in vals), "--max-dist", 80, "--units", "geo", "--fill", -1, "--alloc", out_alloc, "--cpu")
        assert res.exit_code == 0 and "targets:" in res.output and "within reach" in res.output, res.output
        got, meta = read_geotiff(out)
        assert got.tobytes() == want[0].tobytes() and float(meta.nodata) == -1.0
        assert read_geotiff(out_alloc)[0].tobytes() == want[1].tobytes()
    res = run(flac, "-o", out, "--values", str(vals[-1]), "--dtype", "uint16", "--window", "10,20,40,50", "--cpu")
    assert res.exit_code == 0, res.output
    got, meta = read_geotiff(out)
    assert got.tobytes() == proximity_arrays(plain, Options(values=vals[-1:]), sub, "uint16")[0].tobytes()
    assert int(meta.nodata) == 65535   # the default fill of an integer output is its maximum, and the nodata tag
    res = run(flac, "-o", out, "--fixed", 1, "--max-dist", 3, "--fill", 0, "--dtype", "uint8", "--cpu")  # every pixel is non-zero
    assert res.exit_code == 0 and read_geotiff(out)[0].tobytes() == proximity_arrays(
        plain, Options(max_dist=3.0, fixed=1.0, fill=0.0), None, "uint8")[0].tobytes()
    assert run(flac, "-o", out, "--window", "0,0,8,8", "--bbox", "0,0,1,1", "--cpu").exit_code == 1
    assert run(tmp_path / "absent.tif", "-o", out, "--cpu").exit_code == 1
    assert run(flac, "-o", out, "--units", "metres", "--cpu").exit_code == 1
    assert run(flac, "-o", out, "--attribute", "field", "--cpu").exit_code == 1
    assert run(flac, "-o", out, "--max-dist", -1, "--cpu").exit_code == 1

    # polygons: the distance to the nearest polygon and its label
    grid, fields = ROOT / "tests" / "golden" / "sample_multispectral.tif", ROOT / "tests" / "golden" / "fields.geojson"
    _, meta = read_geotiff(grid)
    feats, values = read_geojson(fields, "field")
    labels, _ = rasterize_arrays(to_pixel(feats, Affine(*list(meta.transform)[:6])), (meta.height, meta.width), values, 0, np.uint16)
    want = proximity_arrays(labels, Options(max_dist=6.0), None, "float32")
    dist, alloc, counts, win, transform, crs = proximity_of_polygons(grid, fields, "field", Options(max_dist=6.0))
    assert win == (0, 0, meta.height, meta.width) and transform == tuple(meta.transform)[:6]
    assert dist.tobytes() == want[0].tobytes() and np.array_equal(alloc, want[1]) and counts.tolist() == want[2].tolist()
    assert set(np.unique(alloc).tolist()) <= set(values) | {0} and len(np.unique(alloc)) > 2
    part = proximity_of_polygons(grid, fields, "field", Options(max_dist=6.0), window=(4, 5, 20, 17))
    assert part[0].tobytes() == want[0][:, 4:24, 5:22].tobytes()
    res = run(fields, "--like", grid, "--attribute", "field", "-o", out, "--alloc", out_alloc, "--max-dist", 6, "--cpu")
    assert res.exit_code == 0, res.output
    assert read_geotiff(out)[0].tobytes() == want[0].tobytes() and np.array_equal(read_geotiff(out_alloc)[0], want[1])
    doc = json.loads(fields.read_text())
    doc["features"][0]["properties"]["field"] = 0
    with pytest.raises(ValueError, match="label of 0"):
        proximity_of_polygons(grid, doc, "field")


# ------------------------------------------------------------------------------- 5. the stand-alone check program
def test_hostcheck_covers_the_proximity_unit():
    """make hostcheck: the refusals of both entries in their order, the reach threshold against the f64 predicate and
    the launch plan's arithmetic in the stand-alone program under AddressSanitizer + UBSan; no GPU."""
    csrc = ROOT / "flac-raster_amd" / "csrc"
    if not shutil.which("make") or not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("no make / hipcc")
    text = (ROOT / "tools" / "decode_host_check.cpp").read_text()
    for name in ("fra_proximity(", "fra_decode_device_proximity", "fra_proximity_timing", "reach_threshold", "make_plan",
                 "neither dist nor alloc", "output window"):
        assert name in text, name
    mk = (csrc / "Makefile").read_text()
    assert mk.count("fra_proximity.hip") == 1 and mk.count("fra_proximity.h ") >= 2 and " fra_proximity " in mk
    subprocess.run(["make", "-C", str(csrc), "hostcheck"], check=True, capture_output=True)
    run = subprocess.run([str(csrc / "build" / "decode_host_check"), str(ROOT / "tests" / "golden" / "sample_rgb.flac")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "argument validation checked" in run.stdout and "host check ok" in run.stdout, \
        run.stdout[-4000:] + run.stderr[-4000:]
