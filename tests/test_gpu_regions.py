"""GPU tests of the regions unit (``k_reg_links``, ``k_reg_tile``, ``k_reg_seam`` and the kernels after them, through
``fra_regions`` and ``fra_decode_device_regions``).

The expectation is never the kernel: it is ``regions.regions_arrays`` -- the run-based union-find in numpy, which the
CPU tests hold against the flood-fill definition -- or ``regions.regions_direct`` itself where stated, compared byte for
byte in ``labels``, ``area`` and ``sieved``, record for record in the table, together with the four counts per band.
Everything is integer work, so there is no tolerance anywhere.  The shapes stand around the tile side T = 64: one pixel,
one row, one column, exactly a tile, a tile and one, four-tile corners with ragged edges, a row of 18 tiles, and
(520, 520), whose 81 tiles put workgroups on every XCD.
"""
import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest

import regions_cases as RC
from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.regions import MAX_SIDE, REC, Options, regions_arrays, regions_direct

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SRC_DTYPES = [np.uint8, np.int16, np.uint32, np.float32, np.float64]
COMBOS = list(itertools.product((4, 8), (False, True), (1, 50)))   # connectivity, by_value, min_size


def _ctx():
    return N.default_context(0)


def _same(got, want):
    """got: (labels, area, sieved, table (B, cap), counts) of the GPU; want: the rule's."""
    for g, w, name in zip(got[:3], want[:3], ("labels", "area", "sieved")):
        assert (g is None) == (w is None), name
        if w is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, name
            bits = f"u{g.dtype.itemsize}"
            assert g.tobytes() == w.tobytes(), (name, np.argwhere(np.ascontiguousarray(g).view(bits) != w.view(bits))[:5])
    assert got[4].tolist() == want[4].tolist(), ("counts", got[4].tolist(), want[4].tolist())
    if got[3] is not None:
        for b, t in enumerate(want[3]):
            assert got[3][b, :t.size].tobytes() == t.tobytes(), ("table", b)
            assert not got[3][b, t.size:].view(np.uint8).any(), ("records past N were written", b)


def _label_dtype(n, k):
    """uint8 where N fits, else uint16 where it fits, else int32; k picks among those that fit."""
    fits = [dt for dt in (np.uint8, np.uint16, np.int32) if n <= np.iinfo(dt).max]
    return np.dtype(fits[k % len(fits)])


def _check(ctx, a, opts=Options(), k=0, adt="uint32", ref=regions_arrays):
    """ctx.regions over ``a`` with every output against the rule; the labels dtype is picked by N and ``k``."""
    n = int(ref(a, opts, np.int32, None)[4][:, 2].max())
    ldt = _label_dtype(n, k)
    want = ref(a, opts, ldt, adt)
    got = ctx.regions(a, opts, ldt, adt, labels=None, area=None, sieved=None, table=n + 2)
    _same(got, want)
    return want


# ------------------------------------------------------------------------------- 1. the kernels against the rule
@pytest.mark.parametrize("name,m", RC.small_cases(), ids=[n for n, _ in RC.small_cases()])
def test_small_cases_equal_the_numpy_rule(name, m):
    ctx = _ctx()
    for k, (conn, by_value, min_size) in enumerate(COMBOS):
        dt = np.dtype(SRC_DTYPES[(k + len(name)) % len(SRC_DTYPES)])
        a = m[None].astype(dt)
        _check(ctx, a, Options(connectivity=conn, by_value=by_value, min_size=min_size, sieve_fill=-3.0), k)


@pytest.mark.parametrize("name,m", RC.large_cases(), ids=[n for n, _ in RC.large_cases()])
def test_large_cases_equal_the_numpy_rule(name, m):
    ctx = _ctx()
    for k, (conn, by_value, min_size) in enumerate(COMBOS):
        dt = np.dtype(SRC_DTYPES[k % len(SRC_DTYPES)])
        want = _check(ctx, m[None].astype(dt), Options(connectivity=conn, by_value=by_value, min_size=min_size, sieve_fill=7.0), k)
        if name.endswith("spiral"):
            assert want[4][0].tolist()[1:3] == [1, 1] and int(want[3][0]["area"][0]) == int(m.sum())
        if name.endswith("checker") and min_size == 1:
            assert int(want[4][0, 1]) == (int(m.sum()) if conn == 4 else 1)


def test_float_classes_with_both_zeros_and_nan():
    """-0.0 and 0.0 are one class under ==; a NaN is background, inverted or not."""
    ctx = _ctx()
    for dt in (np.float32, np.float64):
        a = RC.float_classes(dt=dt)[None]
        for conn in (4, 8):
            for opts in (Options((1.5,), invert=True, by_value=True, connectivity=conn),
                         Options((0.0, 2.5), by_value=True, connectivity=conn, min_size=3, sieve_fill=float("nan")),
                         Options(connectivity=conn, by_value=True), Options(invert=True, connectivity=conn)):
                want = _check(ctx, a, opts, 2, "float32")
                assert not want[0][0][np.isnan(a[0])].any()


@pytest.mark.parametrize("adt", ["uint8", "int16", "float32", "float64"])
def test_area_dtypes_saturate_as_the_band_math_does(adt):
    a = RC.mask((RC.T + 1, RC.T + 1), "perc4")[None]      # areas past 255
    want = _check(_ctx(), a, Options(connectivity=8), 0, adt)
    assert int(want[3][0]["area"].max()) > 255


def test_determinism():
    ctx = _ctx()
    for content, conn in (("perc4", 4), ("perc8", 8), ("spiral", 4)):
        a = RC.mask(RC.LARGE, content)[None]
        opts = Options(connectivity=conn, min_size=2)
        one = ctx.regions(a, opts, labels=None, area=None, sieved=None, table=70000)
        two = ctx.regions(a, opts, labels=None, area=None, sieved=None, table=70000)
        for x, y in zip(one, two):
            assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------- 2. layouts and buffers
def test_outputs_alone_and_together():
    ctx = _ctx()
    a = RC.mask(RC.SEAMS, "r5")[None].astype(np.int16)
    opts = Options(connectivity=8, min_size=2, sieve_fill=-1.0)
    want = regions_arrays(a, opts, "uint16", "uint32")
    n = int(want[4][0, 2])
    for labels, area, sieved, table in ((None, False, False, None), (False, None, False, None), (False, False, None, None),
                                        (False, False, False, n), (None, None, None, n)):
        got = ctx.regions(a, opts, "uint16", "uint32", labels=labels, area=area, sieved=sieved, table=table)
        full = (want[0] if labels is None else None, want[1] if area is None else None,
                want[2] if sieved is None else None, want[3], want[4])
        _same(got, full)
    with pytest.raises(N.NativeError, match="none of labels, area, sieved and table"):
        ctx.regions(a, opts, labels=False)


def test_strided_sources_and_destinations():
    """A pixel-interleaved source seen band by band, outputs that are views with gaps, rows and columns: the elements
    between the outputs keep their values."""
    ctx = _ctx()
    h, w = RC.SEAMS
    inter = np.stack([RC.mask(RC.SEAMS, c) for c in ("perc4", "random3", "comb")], axis=-1).astype(np.uint16)  # (h, w, 3)
    a = inter.transpose(2, 0, 1)
    assert not a.flags.c_contiguous
    opts = Options(by_value=True, min_size=4, sieve_fill=9.0)
    want = regions_arrays(a, opts, "int32", "float32")
    lab = np.full((3, h + 2, 2 * w + 1), -5, np.int32)
    area = np.full((h, w, 3), -5.0, np.float32)
    sieved = np.full((3, h, w + 3), 77, np.uint16)
    got = ctx.regions(a, opts, "int32", "float32", labels=lab[:, 1:h + 1, 1:2 * w + 1:2], area=area.transpose(2, 0, 1),
                      sieved=sieved[:, :, :w], table=int(want[4][:, 2].max()))
    _same((np.ascontiguousarray(got[0]), np.ascontiguousarray(got[1]), np.ascontiguousarray(got[2]), got[3], got[4]), want)
    assert (lab[:, 0] == -5).all() and (lab[:, -1] == -5).all() and (lab[:, :, ::2] == -5).all()
    assert (sieved[:, :, w:] == 77).all()
    col = RC.mask((70, 1), "perc4")[None]
    _same(ctx.regions(np.asfortranarray(col), Options(), table=40, area=None, sieved=None), regions_arrays(col))


def test_device_sources_and_destinations():
    """Buffers of the library's own context as the source, the three rasters and the table, with padded rows."""
    ctx = _ctx()
    h, w = RC.SEAMS
    a = RC.mask(RC.SEAMS, "perc8")[None].astype(np.int16)
    opts = Options(connectivity=8, min_size=3, sieve_fill=-2.0)
    want = regions_arrays(a, opts, "uint16", "uint32")
    n = int(want[4][0, 2])
    srs, lrs, ars, vrs = w + 6, w + 3, w, w + 1
    src = np.zeros((h, srs), np.int16)
    src[:, :w] = a[0]
    lbuf, abuf, vbuf = np.full(h * lrs, 99, np.uint16), np.full(h * ars, 99, np.uint32), np.full(h * vrs, 99, np.int16)
    tbuf = np.zeros(n + 3, REC)
    tbuf["area"] = 99
    bufs = [ctx.alloc(x.nbytes) for x in (src, lbuf, abuf, vbuf, tbuf)]
    try:
        for d, x in zip(bufs, (src, lbuf, abuf, vbuf, tbuf)):
            ctx.h2d(d, x)
        got = ctx.regions(bufs[0], opts, "uint16", "uint32", labels=bufs[1], area=bufs[2], sieved=bufs[3],
                          table=(bufs[4], n + 3), dtype=np.int16, shape=(1, h, w), strides=(0, srs, 1),
                          out_strides={"labels": (0, lrs, 1), "area": (0, ars, 1), "sieved": (0, vrs, 1)})
        for d, x in zip(bufs[1:], (lbuf, abuf, vbuf, tbuf)):
            ctx.d2h(x, d)
    finally:
        for d in bufs:
            ctx.free(d)
    rows = lbuf.reshape(h, lrs)
    assert rows[:, :w].tobytes() == want[0][0].tobytes() and (rows[:, w:] == 99).all()
    assert abuf.reshape(h, ars).tobytes() == want[1][0].tobytes()
    rows = vbuf.reshape(h, vrs)
    assert rows[:, :w].tobytes() == want[2][0].tobytes() and (rows[:, w:] == 99).all()
    assert tbuf[:n].tobytes() == want[3][0].tobytes() and (tbuf["area"][n:] == 99).all()
    assert got[4].tolist() == want[4].tolist()


def test_bands_are_handled_on_their_own():
    """Three bands, with labels narrow enough that every band is counted before any is written."""
    ctx = _ctx()
    a = np.stack([RC.mask(RC.SEAMS, c) for c in ("r5", "none", "spiral")]).astype(np.uint8)
    opts = Options(connectivity=8, min_size=2)
    want = regions_arrays(a, opts, "uint8", "uint32")
    cap = int(want[4][:, 2].max())
    _same(ctx.regions(a, opts, "uint8", "uint32", area=None, sieved=None, table=cap), want)
    _same(ctx.regions(a, opts, "uint8", "uint32", area=None, sieved=None, table=None)[:3] + (None, want[4]), want)
    for b in range(3):
        one = ctx.regions(a[b:b + 1], opts, "uint8", "uint32", area=None, sieved=None, table=cap)
        _same(one, (want[0][b:b + 1], want[1][b:b + 1], want[2][b:b + 1], want[3][b:b + 1], want[4][b:b + 1]))


# ------------------------------------------------------------------------------- 3. refusals
def _prefilled(shape, ldt):
    return (np.full(shape, 0x5a, ldt), np.full(shape, 0x5a5a5a5a, np.uint32), np.full(shape, 0x5a, np.uint8))


def test_no_space_in_the_labels_dtype():
    """The checker under 4-connectivity has a component per foreground pixel: uint8 labels cannot number them."""
    ctx = _ctx()
    m = RC.mask((RC.T + 1, RC.T + 1), "checker")
    a = np.stack([RC.mask((RC.T + 1, RC.T + 1), "one"), m])   # the band that fits comes first
    for src in (a[1:], a):
        lab, area, sieved = _prefilled(src.shape, np.uint8)
        table = np.zeros((src.shape[0], 3000), REC)
        table["first"] = 0x5a5a5a5a
        with pytest.raises(N.RegionsNoSpace, match=f"band {src.shape[0] - 1} has {int(m.sum())} components.*255") as e:
            ctx.regions(src, Options(), "uint8", "uint32", labels=lab, area=area, sieved=sieved, table=table)
        assert e.value.counts.tolist() == regions_arrays(src, Options(), "int32")[4].tolist()
        assert (lab == 0x5a).all() and (area == 0x5a5a5a5a).all() and (sieved == 0x5a).all()
        assert (table["first"] == 0x5a5a5a5a).all() and not table["area"].any()
    _check(ctx, a[1:], Options(connectivity=8))   # one component under 8: uint8 holds it


def test_no_space_in_the_table():
    ctx = _ctx()
    a = RC.mask(RC.SEAMS, "perc4")[None]
    opts = Options(min_size=3)
    want = regions_arrays(a, opts, "int32", "uint32")
    n = int(want[4][0, 2])
    lab, area, sieved = _prefilled(a.shape, np.int32)
    table = np.zeros((1, n - 1), REC)
    with pytest.raises(N.RegionsNoSpace, match=f"band 0 has {n} components.*table holds \\({n - 1}\\)") as e:
        ctx.regions(a, opts, "int32", "uint32", labels=lab, area=area, sieved=sieved, table=table)
    assert e.value.counts.tolist() == want[4].tolist()
    assert (lab == 0x5a).all() and (area == 0x5a5a5a5a).all() and (sieved == 0x5a).all() and not table.view(np.uint8).any()
    _same(ctx.regions(a, opts, "int32", "uint32", labels=lab, area=area, sieved=sieved, table=n), want)   # N itself fits


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


def test_refusals_leave_the_outputs_alone():
    ctx = _ctx()
    a = RC.mask((1, 70), "perc4")[None]
    lab = np.full(a.shape, 5, np.int32)
    counts = (C.c_uint64 * 4)(7, 7, 7, 7)
    for field, value, message in (("height", 0, "1 .. 32768"), ("nvalues", 17, "nvalues"), ("connectivity", 6, "connectivity"),
                                  ("min_size", 0, "min_size"), ("table_cap", -1, "table_cap")):
        job = _job(a, lab)
        setattr(job if field == "height" else job.opts, field, value)
        assert N.load().fra_regions(ctx.h, C.byref(job), counts) == -1
        assert message in N.load().fra_last_error().decode()
        assert (lab == 5).all() and list(counts) == [7, 7, 7, 7]
    job = _job(a, lab)
    job.opts.labels.dtype = N.DTYPE_CODES[np.dtype(np.float32)]
    assert N.load().fra_regions(ctx.h, C.byref(job), counts) == -1 and "bad labels dtype" in N.load().fra_last_error().decode()
    assert N.load().fra_regions(ctx.h, C.byref(_job(a, lab)), None) == 0   # counts may be NULL
    assert lab.tobytes() == regions_arrays(a)[0].tobytes()


@pytest.mark.parametrize("shape", [(3, MAX_SIDE), (MAX_SIDE, 3)], ids=["3x32768", "32768x3"])
def test_the_size_limit(shape):
    """A few dozen pixels, the four ends and a pair across every kind of seam among them, against the definition."""
    h, w = shape
    rng = np.random.default_rng(h)
    a = np.zeros((1, h, w), np.uint16)
    rr, cc = rng.integers(0, h, 40), rng.integers(0, w, 40)
    a[0, rr, cc] = 1
    a[0, 0, 0] = a[0, h - 1, w - 1] = a[0, 0, w - 1] = a[0, h - 1, 0] = 1
    if w > h:
        a[0, 1, 32700:32768] = 1            # a run over the last seam, up to the last pixel index
        a[0, 0, 63], a[0, 1, 64] = 1, 1    # a diagonal across the first seam
    else:
        a[0, 32700:32768, 1] = 1
        a[0, 63, 0], a[0, 64, 1] = 1, 1
    ctx = _ctx()
    for conn in (4, 8):
        want = _check(ctx, a, Options(connectivity=conn), 1, ref=regions_direct)
        assert int(want[3][0]["area"].max()) >= 68


@pytest.mark.parametrize("shape", [(1, MAX_SIDE + 1), (MAX_SIDE + 1, 1)], ids=["1x32769", "32769x1"])
def test_one_over_the_limit_is_refused(shape):
    with pytest.raises(N.NativeError, match="1 .. 32768"):
        _ctx().regions(np.ones((1,) + shape, np.uint8))


def test_timing():
    ctx = _ctx()
    ctx.regions(RC.mask(RC.SEAMS, "perc4")[None])
    ms = ctx.regions_timing()
    assert len(ms) == 4 and all(np.isfinite(t) and t >= 0.0 for t in ms)


# ------------------------------------------------------------------------------- 4. containers and zones
H, W, TSIZE = 100, 120, 64  # 2 x 2 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from flac_raster.streaming import build_streaming, read_window
    from flac_raster.tiff import write_geotiff

    rng = np.random.default_rng(31)
    classes = np.array([0, 20000, 40000, 65535], np.uint16)
    src = classes[(rng.random((2, H, W)) < 0.55) * rng.integers(1, 4, (2, H, W))]
    d = tmp_path_factory.mktemp("regions")
    path = d / "scene_streaming.flac"
    path.write_bytes(build_streaming(src, TRANSFORM, "EPSG:32633", TSIZE))
    plain = read_window(path, window=(0, 0, H, W), device=None)[0]
    # the 16-bit round trip moves the values, the zeros included: the foreground is every value of the plain read but its least
    vals = tuple(float(v) for v in np.unique(plain)[1:])
    assert 1 <= len(vals) <= 16
    mask_tif = d / "mask.tif"
    mask = (RC.mask((H, W), "perc4") * 3).astype(np.uint8)
    write_geotiff(mask_tif, mask[None], transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    plain.setflags(write=False)
    return path, plain, vals, mask_tif, mask


def test_decode_device_regions_on_a_container(scene):
    from flac_raster.streaming import regions_window

    path, plain, vals, _, _ = scene
    for opts in (Options(vals), Options(vals, by_value=True, connectivity=8, min_size=3, sieve_fill=1.0)):
        for window in (None, (30, 40, 50, 60), (70, 90, 30, 30)):
            r, c, h, w = window or (0, 0, H, W)
            want = regions_arrays(plain[:, r:r + h, c:c + w], opts, "int32", "uint32")
            got = regions_window(path, opts, window=window, want_area=True, want_sieved=True, device=0)
            assert got[5] == (r, c, h, w)
            host = regions_window(path, opts, window=window, want_area=True, want_sieved=True, device=None)
            for res in (got, host):
                for g, x in zip(res[:3], want[:3]):
                    assert g.tobytes() == x.tobytes()
                assert all(g.tobytes() == x.tobytes() for g, x in zip(res[3], want[3])) and len(res[3]) == 2
                assert res[4].tolist() == want[4].tolist()
    # the first table holds fewer records than a band has components: the call is repeated with the N it was told
    import flac_raster.streaming as S
    guess, S._TABLE_GUESS = S._TABLE_GUESS, 5
    try:
        got = regions_window(path, Options(vals), device=0)
    finally:
        S._TABLE_GUESS = guess
    want = regions_arrays(plain, Options(vals), "int32", None)
    assert int(want[4][:, 2].min()) > 5 and all(g.tobytes() == x.tobytes() for g, x in zip(got[3], want[3]))


def test_zonal_of_regions(scene):
    from flac_raster.streaming import zonal_of_regions
    from flac_raster.zonal import zonal_arrays

    path, plain, _, mask_tif, mask = scene
    for opts in (Options(min_size=4), Options(connectivity=8)):
        labels, _, _, _, counts = regions_arrays(mask[None], opts, np.int32, None)
        want = zonal_arrays(plain, labels[0], 1, max(int(counts[0, 2]), 1), ignore=0)
        dev = zonal_of_regions(path, mask_tif, opts, device=0)
        host = zonal_of_regions(path, mask_tif, opts, device=None)
        assert dev[0] == want and host[0] == want
        assert dev[3].tolist() == counts.tolist() == host[3].tolist()
    r, c, h, w = win = (10, 20, 70, 64)
    labels, _, _, _, counts = regions_arrays(mask[None, r:r + h, c:c + w], Options(), np.int32, None)
    want = zonal_arrays(plain[:, r:r + h, c:c + w], labels[0], 1, int(counts[0, 2]), ignore=0)
    assert zonal_of_regions(path, mask_tif, Options(), window=win, device=0)[0] == want


def test_more_than_65536_components_are_refused(tmp_path):
    from flac_raster.streaming import zonal_of_regions
    from flac_raster.tiff import write_geotiff

    m = RC.mask((400, 400), "checker")
    assert int(m.sum()) == 80000
    write_geotiff(tmp_path / "checker.tif", m[None], transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    with pytest.raises(ValueError, match="80000 components.*min_size"):
        zonal_of_regions(tmp_path / "checker.tif", tmp_path / "checker.tif", Options(), device=0)
    rep = zonal_of_regions(tmp_path / "checker.tif", tmp_path / "checker.tif", Options(connectivity=8), device=0)
    assert rep[3].tolist() == [[80000, 1, 1, 80000]]
