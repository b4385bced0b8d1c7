"""CPU tests of the regions feature: the rule in numpy and everything around the kernels that needs no GPU.

* ``regions_arrays`` (run-based union-find) against ``regions_direct`` (a flood fill per component) in the bytes of
  ``labels``, ``area`` and ``sieved``, the table records and the counts, over the small shapes and every content, for 4 and
  8, by value and not, ``min_size`` 1, 2 and 50; against ``scipy.ndimage.label`` where it imports.
* What the rule promises: one spiral, exact checker counts, the table's areas against the counts, dense labels in
  first-pixel order, ``sieved`` against the removed components.
* ``validate`` and every refusal of ``fra_regions`` through ctypes, with a context that is never dereferenced.
* ``regions_window`` over a container (tiles encoded by the oracle stand-in), ``regions_tiff``, ``zonal_of_regions`` and
  the ``regions``, ``sieve`` and ``zonal --zones-regions`` commands on the host path.
* ``make hostcheck`` with the refusals, the FRA_E_SPACE decisions and the launch plan in it.
"""
import csv
import ctypes as C
import itertools
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import regions_cases as RC
from flac_raster import _native as N
from flac_raster import regions as R
from flac_raster.geo import Affine
from flac_raster.regions import Options, regions_arrays, regions_direct
from flac_raster.streaming import assemble_streaming, read_window, regions_tiff, regions_window, zonal_of_regions
from flac_raster.tiff import read_geotiff, write_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
NEW = ("fra_regions", "fra_decode_device_regions", "fra_regions_timing")
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TSIZE = 100, 120, 64  # 2 x 2 tiles, ragged right and bottom
T = RC.T


def _equal(x, y):
    for u, v, name in zip(x[:3], y[:3], ("labels", "area", "sieved")):
        assert (u is None) == (v is None), name
        if u is not None:
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes(), name
    assert len(x[3]) == len(y[3]) and all(p.tobytes() == q.tobytes() for p, q in zip(x[3], y[3])), "tables"
    assert x[4].tolist() == y[4].tolist(), "counts"


def _properties(a, opts, res):
    """What the rule promises about its own result."""
    labels, area, sieved, tables, counts = res
    for b in range(a.shape[0]):
        t, (fg, ncomp, n, px) = tables[b], counts[b].tolist()
        assert t.size == n <= ncomp and int(t["area"].sum()) == px <= fg
        assert (t["area"] >= opts.min_size).all() and (np.diff(t["first"].astype(np.int64)) > 0).all()
        assert set(np.unique(labels[b]).tolist()) == set(range(1, n + 1)) | ({0} if (labels[b] == 0).any() else set())
        lab = labels[b].ravel()
        firsts = np.full(n + 1, lab.size, np.int64)
        np.minimum.at(firsts, lab, np.arange(lab.size))
        assert firsts[1:].tolist() == t["first"].tolist()       # dense, and in the order of the first pixels
        assert np.array_equal(np.bincount(lab, minlength=n + 1)[1:], t["area"])
        fgm = R.foreground_of(a[b], opts)
        removed = fgm & (labels[b] == 0)
        assert int(fgm.sum()) == fg and not labels[b][~fgm].any()
        diff = sieved[b].view(f"u{a.itemsize}") != a[b].view(f"u{a.itemsize}")
        assert not diff[~removed].any()
        if opts.sieve_fill == -3.0 and a.dtype.kind != "u":
            assert (sieved[b][removed] == -3).all()
        if area is not None:
            assert np.array_equal(area[b], np.where(labels[b] > 0, np.concatenate([[0], t["area"]])[labels[b]], 0))


# ------------------------------------------------------------------------------- 1. the two forms of the rule
@pytest.mark.parametrize("name,m", RC.small_cases(), ids=[n for n, _ in RC.small_cases()])
def test_arrays_equal_the_definition(name, m):
    for k, (conn, by_value) in enumerate(itertools.product((4, 8), (False, True))):
        dt = np.dtype([np.uint8, np.int16, np.uint32, np.float32, np.float64][(k + len(name)) % 5])
        a = m[None].astype(dt)
        for min_size in (1, 2, 50):
            opts = Options(connectivity=conn, by_value=by_value, min_size=min_size, sieve_fill=-3.0)
            res = regions_arrays(a, opts, "int32", "uint32")
            _equal(res, regions_direct(a, opts, "int32", "uint32"))
            _properties(a, opts, res)


def test_float_classes():
    a = RC.float_classes((T + 1, T + 3))[None]
    for conn in (4, 8):
        for opts in (Options((1.5,), invert=True, by_value=True, connectivity=conn),
                     Options((0.0, 2.5), by_value=True, connectivity=conn, min_size=3, sieve_fill=float("nan")),
                     Options(connectivity=conn, by_value=True), Options(invert=True, connectivity=conn)):
            res = regions_arrays(a, opts, "uint16", "float32")
            _equal(res, regions_direct(a, opts, "uint16", "float32"))
            assert not res[0][0][np.isnan(a[0])].any()
    # the two zeros are one class: a band of -0.0 and 0.0 alone is one component by value
    z = np.where(RC.mask((9, 9), "checker") > 0, -0.0, 0.0).astype(np.float32)[None]
    assert regions_arrays(z, Options((0.0,), by_value=True))[4].tolist() == [[81, 1, 1, 81]]


def test_labels_equal_scipy_for_binary_unsieved_masks():
    ndimage = pytest.importorskip("scipy.ndimage")
    four, eight = ndimage.generate_binary_structure(2, 1), ndimage.generate_binary_structure(2, 2)
    for name, m in RC.small_cases() + RC.large_cases()[1:3]:
        for conn, st in ((4, four), (8, eight)):
            want, n = ndimage.label(m > 0, structure=st)
            got = regions_arrays(m[None], Options(connectivity=conn))
            assert int(got[4][0, 2]) == n and np.array_equal(got[0][0], want), (name, conn)


def test_spiral_checker_and_hand_made_cases():
    for shape in ((T + 1, T + 1), RC.SEAMS, RC.LARGE):
        m = RC.mask(shape, "spiral")
        for conn in (4, 8):
            res = regions_arrays(m[None], Options(connectivity=conn))
            assert res[4].tolist() == [[int(m.sum())] + [1, 1] + [int(m.sum())]] and int(res[3][0]["area"][0]) == int(m.sum())
        assert int(m.sum()) > m.size // 3 and m[0].all() and m[:, -1].all()   # it does go through every tile
        c = RC.mask(shape, "checker")
        n = int(c.sum())
        assert n == (shape[0] * shape[1] + 1) // 2
        assert regions_arrays(c[None], Options(connectivity=4))[4].tolist() == [[n, n, n, n]]
        assert regions_arrays(c[None], Options(connectivity=8))[4].tolist() == [[n, 1, 1, n]]
        assert regions_arrays(c[None], Options(connectivity=4, min_size=2))[4].tolist() == [[n, n, 0, 0]]
    d = RC.diagonals()[None]
    assert regions_arrays(d, Options(connectivity=8))[4].tolist() == [[16, 2, 2, 16]]
    assert regions_arrays(d, Options(connectivity=4))[4].tolist() == [[16, 16, 16, 16]]
    for m in (RC.seam_row(), RC.seam_col()):
        res = regions_arrays(m[None], Options(connectivity=4))
        assert res[4].tolist() == [[int(m.sum()), 1, 1, int(m.sum())]]
    comb = RC.mask(RC.SEAMS, "comb")
    res = regions_arrays(comb[None], Options())
    assert res[4][0, 1] == 1 and res[3][0][0].tolist() == (0, int(comb.sum()), 0, 0, RC.SEAMS[0] - 1, RC.SEAMS[1] - 1)


def test_bands_label_dtypes_and_the_export_rows():
    a = np.stack([RC.mask(RC.SEAMS, c) for c in ("r5", "none", "blocks3")]).astype(np.int16)
    opts = Options(by_value=True, connectivity=8)
    res = regions_arrays(a, opts, "uint16", "float64")
    for b in range(3):
        _equal(regions_arrays(a[b:b + 1], opts, "uint16", "float64"), tuple(x[b:b + 1] for x in res))
    assert res[4][1].tolist() == [0, 0, 0, 0] and res[0].dtype == np.uint16 and res[1].dtype == np.float64
    with pytest.raises(ValueError, match="more than the labels dtype holds"):
        regions_arrays(RC.mask((T, T), "checker")[None], Options(), "uint8")
    rows = R.export_rows(a, res[3], tuple(TRANSFORM)[:6])
    assert len(rows) == int(res[4][:, 2].sum()) and rows[0]["band"] == 1 and rows[-1]["band"] == 3
    last = rows[-1]
    assert last["value"] == int(a[2, last["first_row"], last["first_col"]]) and last["label"] == int(res[4][2, 2])
    assert last["x_min"] == 500000.0 + 10.0 * last["col_min"] and last["y_max"] == 4100000.0 - 10.0 * last["row_min"]
    assert last["x_max"] == 500000.0 + 10.0 * (last["col_max"] + 1) and last["y_min"] == 4100000.0 - 10.0 * (last["row_max"] + 1)


# ------------------------------------------------------------------------------- 2. refusals
def test_validate_refuses_what_the_header_refuses():
    for opts, message in ((Options(values=tuple(range(17))), "nvalues"), (Options(values=(1.0, float("inf"))), "value 1 is not finite"),
                          (Options(values=(float("nan"),)), "value 0 is not finite"), (Options(connectivity=6), "connectivity"),
                          (Options(min_size=0), "min_size"), (Options(values=tuple(range(17)), connectivity=5), "nvalues"),
                          (Options(connectivity=5, min_size=0), "connectivity")):
        with pytest.raises(ValueError, match=message):
            R.validate(opts)
        with pytest.raises(ValueError, match=message):
            regions_arrays(np.ones((1, 3, 3), np.uint8), opts)
    R.validate(Options(values=tuple(range(16)), connectivity=8, min_size=2 ** 31 - 1))
    for bad in ("float32", "int64"):
        with pytest.raises(ValueError, match="bad labels dtype"):
            regions_arrays(np.ones((1, 3, 3), np.uint8), Options(), bad)
    with pytest.raises(ValueError, match="1 .. 32768"):
        R.check_region(0, 5)
    with pytest.raises(ValueError, match="1 .. 32768"):
        R.check_region(5, 32769)


def _job(a, lab):
    job = N.RegionsJob()
    job.src, job.src_on_device, job.dtype = a.ctypes.data, 0, N.DTYPE_CODES[a.dtype]
    job.channels, job.height, job.width = a.shape
    job.band_stride, job.row_stride, job.col_stride = a.shape[1] * a.shape[2], a.shape[2], 1
    o = job.opts
    o.connectivity, o.min_size = 4, 1
    o.labels.dst, o.labels.dtype = lab.ctypes.data, N.DTYPE_CODES[lab.dtype]
    o.labels.band_stride, o.labels.row_stride, o.labels.col_stride = lab.shape[1] * lab.shape[2], lab.shape[2], 1
    return job


def test_the_library_refuses_before_any_gpu_work():
    """Through ctypes with a context that is never dereferenced: every refusal comes before the first GPU call."""
    L = N.load()
    for name in NEW:
        assert hasattr(L, name), name
    a = np.ones((1, 6, 7), np.uint8)
    lab = np.full(a.shape, 5, np.int32)
    fake = C.c_void_p(0x10)
    counts = (C.c_uint64 * 4)(7, 7, 7, 7)

    def refused(change, message):
        job = _job(a, lab)
        change(job)
        assert L.fra_regions(fake, C.byref(job), counts) == -1
        assert message in L.fra_last_error().decode(), (message, L.fra_last_error())
        assert (lab == 5).all() and list(counts) == [7, 7, 7, 7]

    refused(lambda j: setattr(j, "src", None), "null argument")
    refused(lambda j: setattr(j, "dtype", 8), "bad dtype")
    refused(lambda j: setattr(j, "channels", 256), "more than 255")
    refused(lambda j: setattr(j, "row_stride", -1), "bad raster layout")
    refused(lambda j: setattr(j.opts.labels, "dtype", N.DTYPE_CODES[np.dtype(np.float32)]), "bad labels dtype")
    refused(lambda j: setattr(j.opts.labels, "col_stride", -1), "bad labels layout")
    refused(lambda j: (setattr(j.opts.area, "dst", lab.ctypes.data), setattr(j.opts.area, "dtype", 9)), "bad area dtype")
    refused(lambda j: (setattr(j.opts.sieved, "dst", lab.ctypes.data), setattr(j.opts.sieved, "row_stride", -2)), "bad sieved layout")
    refused(lambda j: setattr(j, "height", 0), "1 .. 32768")
    refused(lambda j: setattr(j, "width", 32769), "1 .. 32768")
    refused(lambda j: setattr(j.opts, "nvalues", 17), "nvalues")
    refused(lambda j: (setattr(j.opts, "nvalues", 1), j.opts.values.__setitem__(0, float("nan"))), "value 0 is not finite")
    refused(lambda j: setattr(j.opts, "connectivity", 0), "connectivity")
    refused(lambda j: setattr(j.opts, "min_size", 0), "min_size")
    refused(lambda j: setattr(j.opts, "table_cap", -1), "table_cap")
    refused(lambda j: setattr(j.opts.labels, "dst", None), "none of labels, area, sieved and table")
    # the order: the first rule that is broken speaks
    refused(lambda j: (setattr(j, "dtype", 8), setattr(j, "height", 0)), "bad dtype")
    refused(lambda j: (setattr(j, "height", 0), setattr(j.opts, "min_size", 0)), "1 .. 32768")
    refused(lambda j: (setattr(j.opts, "connectivity", 5), setattr(j.opts, "min_size", 0)), "connectivity")
    assert L.fra_regions_timing(None) == -1
    assert C.sizeof(N.RegionsOpts) == 296 and R.REC.itemsize == 24 and R.TILE == 64


# ------------------------------------------------------------------------------- 3. containers, TIFFs, zones, the commands
@pytest.fixture(scope="module")
def container():
    rng = np.random.default_rng(31)
    classes = np.array([0, 20000, 40000, 65535], np.uint16)
    src = classes[(rng.random((2, H, W)) < 0.55) * rng.integers(1, 4, (2, H, W))]
    tiles = calculate_tiles(H, W, TSIZE)
    data = assemble_streaming(tiles, oracle_encode_tiles(src, tiles, level=5), src.shape, src.dtype, TRANSFORM, "EPSG:32633", TSIZE)
    plain = read_window(data, window=(0, 0, H, W), device=None)[0]
    # the 16-bit round trip moves the values, the zeros included: the foreground is every value of the plain read but its least
    vals = tuple(float(v) for v in np.unique(plain)[1:])
    assert 1 <= len(vals) <= 16 and 0 < np.isin(plain, vals).sum() < plain.size
    plain.setflags(write=False)
    return data, plain, vals


def test_regions_window_and_tiff_on_the_host(tmp_path, container):
    data, plain, vals = container
    opts = Options(vals, by_value=True, connectivity=8, min_size=3, sieve_fill=1.0)
    for window in (None, (30, 40, 50, 60)):
        r, c, h, w = window or (0, 0, H, W)
        want = regions_arrays(plain[:, r:r + h, c:c + w], opts, "int32", "uint32")
        got = regions_window(data, opts, window=window, want_area=True, want_sieved=True)
        assert got[5] == (r, c, h, w) and len(got[6]["frames"]) == 4
        _equal(got[:5], want)
    lab, area, sieved, _, _, _, _ = regions_window(data, opts)
    assert area is None and sieved is None and lab.dtype == np.int32
    tif = tmp_path / "classes.tif"
    write_geotiff(tif, plain, transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    got = regions_tiff(tif, opts, window=(30, 40, 50, 60), label_dtype="uint16", want_area=True, want_sieved=True)
    _equal(got[:5], regions_arrays(plain[:, 30:80, 40:100], opts, "uint16", "uint32"))
    with pytest.raises(ValueError):
        regions_window(data, opts, semantics="float")
    with pytest.raises(ValueError, match="bad labels dtype"):
        regions_window(data, opts, label_dtype="float32")


def test_zonal_of_regions_on_the_host(tmp_path, container):
    from flac_raster.zonal import zonal_arrays

    data, plain, _ = container
    flac, mask_tif = tmp_path / "scene_streaming.flac", tmp_path / "mask.tif"
    flac.write_bytes(data)
    mask = (RC.mask((H, W), "perc4") * 3).astype(np.uint8)
    write_geotiff(mask_tif, mask[None], transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    opts = Options(min_size=4)
    labels, _, _, _, counts = regions_arrays(mask[None], opts, np.int32, None)
    want = zonal_arrays(plain, labels[0], 1, int(counts[0, 2]), ignore=0)
    rep, win, _, got_counts = zonal_of_regions(flac, mask_tif, opts)
    assert rep == want and win == (0, 0, H, W) and got_counts.tolist() == counts.tolist()
    assert len(rep[0]["zones"]) == int(counts[0, 2])
    two = tmp_path / "two.tif"
    write_geotiff(two, np.stack([mask, mask]), transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    with pytest.raises(ValueError, match="single-band"):
        zonal_of_regions(flac, two, opts)
    big = tmp_path / "checker.tif"
    write_geotiff(big, RC.mask((400, 400), "checker")[None], transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    with pytest.raises(ValueError, match="80000 components.*min_size"):
        zonal_of_regions(big, big, Options())


def test_the_commands_on_the_host(tmp_path, container):
    from typer.testing import CliRunner

    from flac_raster.cli import app

    data, plain, vals = container
    flac, tif = tmp_path / "scene_streaming.flac", tmp_path / "classes.tif"
    flac.write_bytes(data)
    write_geotiff(tif, plain, transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    out, out_area, out_sieved = tmp_path / "labels.tif", tmp_path / "area.tif", tmp_path / "sieved.tif"

    def run(*args):
        return CliRunner().invoke(app, [str(a) for a in args])

    vs = ",".join(str(v) for v in vals)
    opts = Options(vals, by_value=True, connectivity=8, min_size=3)
    want = regions_arrays(plain, opts, "uint16", "uint32")
    for source in (flac, tif):
        for export in (tmp_path / "comps.json", tmp_path / "comps.csv"):
            res = run("regions", source, "-o", out, "--values", vs, "--by-value", "--connectivity", 8, "--min-size", 3,
                      "--area", out_area, "--export", export, "--dtype", "uint16", "--cpu")
            assert res.exit_code == 0, res.output
            for b in range(2):
                fg, ncomp, n, px = want[4][b].tolist()
                assert f"band {b + 1}: {fg} foreground pixels, {ncomp} components, {n} kept with {px} pixels" in res.output
            got, meta = read_geotiff(out)
            assert got.dtype == np.uint16 and got.tobytes() == want[0].tobytes() and int(meta.nodata) == 0
            assert read_geotiff(out_area)[0].tobytes() == want[1].tobytes()
            rows = (json.loads(export.read_text())["components"] if export.suffix == ".json"
                    else list(csv.DictReader(open(export, newline=""))))
            ref = R.export_rows(plain, want[3], tuple(TRANSFORM)[:6])
            assert len(rows) == len(ref)
            for got_row, ref_row in zip(rows, ref):
                assert {k: float(v) for k, v in got_row.items()} == {k: float(v) for k, v in ref_row.items()}
    res = run("regions", flac, "-o", out, "--values", vals[0], "--invert", "--window", "10,20,40,50", "--cpu")
    assert res.exit_code == 0, res.output
    assert read_geotiff(out)[0].tobytes() == regions_arrays(plain[:, 10:50, 20:70], Options(vals[:1], invert=True))[0].tobytes()
    # the sieve: regions of one value by default, the fill is the nodata tag
    sopts = Options((), False, True, 4, 5, 7.0)
    res = run("sieve", flac, "-o", out_sieved, "--min-size", 5, "--fill", 7, "--cpu")
    assert res.exit_code == 0, res.output
    got, meta = read_geotiff(out_sieved)
    assert got.tobytes() == regions_arrays(plain, sopts)[2].tobytes() and int(meta.nodata) == 7
    res = run("sieve", tif, "-o", out_sieved, "--min-size", 5, "--any-value", "--connectivity", 8, "--cpu")
    assert res.exit_code == 0 and read_geotiff(out_sieved)[0].tobytes() == regions_arrays(plain, Options(connectivity=8, min_size=5))[2].tobytes()
    # zones from the components of a mask
    mask_tif = tmp_path / "mask.tif"
    mask = RC.mask((H, W), "perc8")
    write_geotiff(mask_tif, mask[None], transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    rep_path = tmp_path / "zonal.json"
    res = run("zonal", flac, "--zones", mask_tif, "--zones-regions", "--connectivity", 8, "--min-size", 10, "--export", rep_path, "--cpu")
    assert res.exit_code == 0, res.output
    n = int(regions_arrays(mask[None], Options(connectivity=8, min_size=10))[4][0, 2])
    assert f"zones: {n} components" in res.output and rep_path.exists()
    # refusals
    assert run("regions", flac, "-o", out, "--connectivity", 6, "--cpu").exit_code == 1
    assert run("regions", flac, "-o", out, "--min-size", 0, "--cpu").exit_code == 1
    assert run("regions", flac, "-o", out, "--export", tmp_path / "x.txt", "--cpu").exit_code == 1
    assert run("regions", tmp_path / "absent.tif", "-o", out, "--cpu").exit_code == 1
    assert run("regions", flac, "-o", out, "--dtype", "float32", "--cpu").exit_code == 1
    assert run("sieve", flac, "-o", out, "--min-size", 0, "--cpu").exit_code == 1
    assert run("zonal", flac, "--zones", mask_tif, "--zones-regions", "--ignore", 3, "--cpu").exit_code == 1


# ------------------------------------------------------------------------------- 4. the stand-alone check program
def test_hostcheck_covers_the_regions_unit():
    """make hostcheck: the refusals of both entries in their order, the FRA_E_SPACE decisions and the launch plan's
    arithmetic in the stand-alone program under AddressSanitizer + UBSan; no GPU."""
    csrc = ROOT / "flac-raster_amd" / "csrc"
    if not shutil.which("make") or not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("no make / hipcc")
    text = (ROOT / "tools" / "decode_host_check.cpp").read_text()
    for name in ("fra_regions(", "fra_decode_device_regions", "fra_regions_timing", "check_space", "may_lack_space", "make_plan",
                 "bad labels dtype", "none of labels, area, sieved and table", "more than the table holds"):
        assert name in text, name
    mk = (csrc / "Makefile").read_text()
    assert mk.count("fra_regions.hip") == 1 and mk.count("fra_regions.h ") >= 2 and " fra_regions " in mk
    subprocess.run(["make", "-C", str(csrc), "hostcheck"], check=True, capture_output=True)
    run = subprocess.run([str(csrc / "build" / "decode_host_check"), str(ROOT / "tests" / "golden" / "sample_rgb.flac")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "argument validation checked" in run.stdout and "host check ok" in run.stdout, \
        run.stdout[-4000:] + run.stderr[-4000:]
