"""GPU tests of the focal operations (``k_focal`` alone through ``fra_focal``, and behind the windowed read through
``fra_decode_device_focal``).

The expectation is never the kernel: it is ``focal.focal_arrays`` -- the rule in numpy, checked on the CPU against a
per-pixel loop -- applied to the raster itself or to the host ``read_window``.  The comparison is bit for bit for every
output dtype, floats included: every step is one IEEE f64 operation in a fixed order and the rule fixes the NaN a float
output holds, so there is no tolerance to choose.  The shapes are those of ``test_gpu_calc.py``: (1, 1), (7, 19) and
(33, 67) are the smallest at which a halo larger than the raster, a ragged slot and a one-workgroup grid can go wrong
(the tile is 16 x 64 pixels), (130, 517) has several tiles and a ragged tail in both axes.  A reference is computed once
(``focal.focal_values``) and converted for every output dtype (``focal.finish``).
"""
import functools

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import focal
from flac_raster.focal import Spec, finish, focal_arrays, focal_values, hillshade_params, slope_params
from flac_raster.geo import Affine

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
ODTS = [np.float32, np.float64, np.uint8, np.int16, np.int32]
SHAPES = [(1, 1), (7, 19), (33, 67), (130, 517)]
WINDOWS = [(3, 3), (1, 15), (15, 1), (15, 15)]
B = 4
HS = hillshade_params(315.0, 45.0, 0.01, 10.0, 20.0, 255.0)
SL = slope_params(0.01, 10.0, 20.0, 100.0)


def _ctx():
    return N.default_context(0)


def _raster(dt, shape, rng):
    """Half small values (ties for the extremes and the median, 7 = the nodata of the tests), half the full range;
    floats with NaN, +-inf and -0.0 sprinkled in."""
    dt = np.dtype(dt)
    small = rng.integers(0, 9, size=shape)
    if dt.kind != "f":
        info = np.iinfo(dt)
        full = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64)
        return np.where(rng.random(shape) < 0.5, small, full).astype(dt)
    full = rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 6, size=shape)
    a = np.where(rng.random(shape) < 0.5, small.astype(np.float64), full).astype(dt)
    flat = a.reshape(-1)
    if flat.size > 16:
        k = rng.choice(flat.size, size=max(4, flat.size // 50), replace=False)
        flat[k] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], dt), size=k.size)
    return a


def _padded(a, pad_cols, fill=77):
    """``a`` (B, h, w) as a view of a larger array: ``pad_cols`` spare columns per row and one spare row per band."""
    nb, h, w = a.shape
    big = np.full((nb, h + 1, w + pad_cols), fill, a.dtype)
    big[:, :h, :w] = a
    return big, big[:, :h, :w]


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ, first at {i}: got {got[i]!r} "
                             f"({int(g[i]):#x}), want {want[i]!r} ({int(w[i]):#x})")


def _weights(size, rng):
    w = rng.integers(-3, 4, size=size).astype(np.float64)
    w[size[0] // 2, size[1] // 2] = 0.3  # products and sums that round
    return w


def _specs(size, edge, rng, nodata=None, **kw):
    """Every op that takes the window ``size``."""
    out = [Spec(op, size, edge, nodata, **kw) for op in ("sum", "mean", "min", "max", "count")]
    w = _weights(size, rng)
    out += [Spec("convolve", size, edge, nodata, weights=w, **kw), Spec("convolve", size, edge, nodata, weights=w, normalize=True, **kw)]
    if size[0] * size[1] <= 25:
        out.append(Spec("median", size, edge, nodata, **kw))
    if size == (3, 3):
        out += [Spec("slope", 3, edge, nodata, params=SL, **kw), Spec("hillshade", 3, edge, nodata, params=HS, **kw)]
    return out


def _name(s):
    return f"{focal.OPS[s.op]} {s.kh}x{s.kw} {focal.EDGES[s.edge]}{' normalize' if s.normalize else ''}{' keep' if s.keep_mask else ''}"


def _check(ctx, a, spec, odts, what, win=None, whole=None):
    """``ctx.focal`` against the rule for every dtype of ``odts``; ``whole``: the rule's (values, filled) over the whole
    raster, of which the rectangle ``win`` must be the crop."""
    values, filled = focal_values(a, spec, win)
    if whole is not None:
        sl = (slice(None), slice(win[0], win[0] + win[2]), slice(win[1], win[1] + win[3]))
        _same(values, whole[0][sl], f"{what}: the rule's rectangle is not the crop")
        assert np.array_equal(filled, whole[1][sl])
    for odt in odts:
        want, wleft = finish(values, filled, spec, odt)
        got, left = ctx.focal(a, spec, odt, out_window=win)
        _same(got, want, f"{_name(spec)} {a.dtype} {a.shape[1:]} {win} -> {np.dtype(odt)} {what}")
        assert left.tolist() == wleft.tolist(), (what, _name(spec), left, wleft)
    return got, left


# ------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_op_for_every_source_and_output_dtype(dt):
    rng = np.random.default_rng(900 + np.dtype(dt).num)
    ctx = _ctx()
    a = _raster(dt, (B, 33, 67), rng)
    seen = set()
    for size, edge in (((3, 3), "skip"), ((5, 5), "clamp")):
        for spec in _specs(size, edge, rng):
            _check(ctx, a, spec, ODTS, "")
            seen.add(spec.op)
    assert seen == set(range(len(focal.OPS)))
    assert ctx.focal_timing() >= 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_windows_edge_modes_and_shapes(dt, shape):
    rng = np.random.default_rng(300 + np.dtype(dt).num + shape[1])
    ctx = _ctx()
    a = _raster(dt, (B,) + shape, rng)
    big = shape[0] * shape[1] > 10000  # the rule takes 0.3 s per 15 x 15 op there: two ops per edge mode
    for size in WINDOWS + [(5, 5)]:
        for edge in ("skip", "clamp"):
            specs = _specs(size, edge, rng)
            if big and size == (15, 15):
                specs = [s for s in specs if s.op == focal.MEAN or s.normalize]
            for spec in specs:
                _check(ctx, a, spec, [np.float32] if spec.op != focal.MEAN else [np.float32, np.int16], "")


# ------------------------------------------------------------------------------- 2. nodata, counts, determinism
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_nodata_and_counts(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(40 + dt.num)
    ctx = _ctx()
    for (h, w) in SHAPES[1:]:
        a = _raster(dt, (B, h, w), rng)
        nd, absent = 7.0, 9.0
        a[a == dt.type(absent)] = 8
        a[rng.random(a.shape) < 0.05] = dt.type(nd)   # about 5 % of the pixels of every band
        if dt.kind == "f":
            a[1, 0, 1] = a[3, h - 1, w - 1] = np.nan
        wide = (15, 15) if h * w < 10000 else (15, 1)
        for nodata, fill in ((nd, None), (absent, None), (nd, 42.5), (float("nan"), None)):
            specs = [Spec("mean", 3, "skip", nodata, fill), Spec("count", 3, "clamp", nodata, fill, keep_mask=True),
                     Spec("median", 5, "skip", nodata, fill, keep_mask=True), Spec("max", wide, "clamp", nodata, fill),
                     Spec("convolve", (1, 15), "skip", nodata, fill, normalize=True, weights=_weights((1, 15), rng)),
                     Spec("hillshade", 3, "clamp", nodata, fill, params=HS), Spec("slope", 3, "skip", nodata, fill, params=SL)]
            for spec in specs:
                got, left = _check(ctx, a, spec, [np.float32, np.uint8], f"nodata {nodata} fill {fill}")
                again, left2 = ctx.focal(a, spec, np.uint8)
                assert again.tobytes() == got.tobytes() and left2.tolist() == left.tolist()
                if nodata == nd and spec.keep_mask:
                    assert (left > 0).all()
        if dt.kind == "f":  # NaN taps are left out with and without a nodata value
            nans = np.count_nonzero(np.isnan(a), axis=(1, 2))
            assert nans[1] > 0
            assert ctx.focal(a, Spec("sum", 1), np.float32)[1].tolist() == nans.tolist()
            assert ctx.focal(a, Spec("sum", 1, nodata=float("nan")), np.float32)[1].tolist() == nans.tolist()


# ------------------------------------------------------------------------------- 3. output rectangles
@pytest.mark.parametrize("dt", [np.uint16, np.float64], ids=lambda d: np.dtype(d).name)
def test_output_rectangles_are_crops(dt):
    rng = np.random.default_rng(17 + np.dtype(dt).num)
    ctx = _ctx()
    for (h, w), rects in (((33, 67), {"corner": (24, 46, 9, 21), "interior": (5, 7, 17, 41)}),
                          ((130, 517), {"corner": (0, 430, 23, 87), "interior": (9, 66, 100, 333), "one pixel": (64, 129, 1, 1)})):
        a = _raster(dt, (B, h, w), rng)
        a[rng.random(a.shape) < 0.05] = 7
        for spec in (Spec("mean", (3, 3), "skip", 7.0), Spec("min", (15, 15), "clamp", 7.0), Spec("median", (5, 5), "skip", 7.0, keep_mask=True),
                     Spec("convolve", (15, 1), "clamp", weights=_weights((15, 1), rng)), Spec("hillshade", 3, "skip", 7.0, params=HS)):
            whole = focal_values(a, spec)
            for name, win in rects.items():
                _check(ctx, a, spec, [np.float32, np.int32], name, win, whole)


# ------------------------------------------------------------------------------- 4. layouts
@pytest.mark.parametrize("dt,odt", [(np.uint16, np.float32), (np.uint8, np.uint8), (np.float64, np.int16),
                                    (np.float32, np.float64), (np.int32, np.uint16)],
                         ids=lambda d: np.dtype(d).name)
def test_layouts(dt, odt):
    dt, odt = np.dtype(dt), np.dtype(odt)
    rng = np.random.default_rng(70 + dt.num + odt.num)
    ctx = _ctx()
    for (h, w) in SHAPES:
        a = _raster(dt, (B, h, w), rng)
        for spec in (Spec("mean", 3, "clamp", 7.0), Spec("max", (1, 15), "skip"), Spec("median", 5, "skip", 7.0)):
            want, wleft = focal_arrays(a, spec, odt)
            V, OV = 16 // dt.itemsize, 16 // odt.itemsize
            abig16, av16 = _padded(a, -w % V + V)   # rows 16-byte aligned: vector loads
            abig5, av5 = _padded(a, 5)              # rows not 16-byte aligned: element loads
            wide = np.full((B, h, 2 * w), 77, dt)
            wide[:, :, ::2] = a
            keep = abig16.tobytes(), abig5.tobytes(), wide.tobytes()
            for view in (av16, av5, wide[:, :, ::2]):
                got, left = ctx.focal(view, spec, odt)
                _same(got, want, f"{_name(spec)} source view {view.strides}")
                assert left.tolist() == wleft.tolist()
            assert (abig16.tobytes(), abig5.tobytes(), wide.tobytes()) == keep  # nothing is written to the source
            # host destinations: the caller's values between the outputs stay
            for pad in (-w % OV + OV, 5):
                obig = np.full((B, h + 1, w + pad), 77, odt)
                ctx.focal(a, spec, odt, dst=obig[:, :h, :w])
                _same(obig[:, :h, :w], want, f"{_name(spec)} padded destination {pad}")
                assert (obig[:, h] == 77).all() and (obig[:, :, w:] == 77).all()
            owide = np.full((B, h, 2 * w), 77, odt)
            ctx.focal(av5, spec, odt, dst=owide[:, :, ::2])
            _same(owide[:, :, ::2], want, f"{_name(spec)} column stride 2")
            assert (owide[:, :, 1::2] == 77).all()
            # device source and destination
            rs, ors = w + (-w % V), w + (-w % OV) + OV
            sa = np.full((B, h, rs), 77, dt)
            sa[:, :, :w] = a
            so = np.full((B, h, ors), 77, odt)
            d_a, d_o = ctx.alloc(sa.nbytes), ctx.alloc(so.nbytes)
            try:
                ctx.h2d(d_a, sa)
                ctx.h2d(d_o, so)
                ctx.focal(d_a, spec, odt, dst=d_o, dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1),
                          dst_strides=(h * ors, ors, 1))
                back = np.empty_like(so)
                ctx.d2h(back, d_o)
                _same(back[:, :, :w], want, f"{_name(spec)} device to device")
                assert (back[:, :, w:] == 77).all()
                got, _ = ctx.focal(d_a, spec, odt, dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1))
                _same(got, want, f"{_name(spec)} device to host")
                src_back = np.empty_like(sa)
                ctx.d2h(src_back, d_a)
                assert src_back.tobytes() == sa.tobytes()
            finally:
                ctx.free(d_a)
                ctx.free(d_o)


# ------------------------------------------------------------------------------- 5. refusals reach Python
def _bad_dtype_job(ctx, d):
    """``fra_focal`` with a destination dtype outside ``fra_dtype``."""
    import ctypes as C

    job = N.FocalJob()
    job.src, job.src_on_device, job.dtype, job.channels, job.height, job.width = C.c_void_p(int(d)), 1, 2, 4, 1, 1
    job.band_stride, job.row_stride, job.col_stride = 1, 1, 1
    job.rect = N.Window(0, 0, 1, 1)
    job.spec = N.focal_spec(Spec("mean"))
    job.out.dst, job.out.dst_on_device, job.out.dtype = C.c_void_p(int(d)), 1, 8
    job.out.band_stride, job.out.row_stride, job.out.col_stride = 1, 1, 1
    return N.load().fra_focal(ctx.h, C.byref(job), None)


def test_refusals_leave_everything_untouched_and_the_context_goes_on():
    ctx = _ctx()
    a = np.arange(4 * 7 * 19, dtype=np.uint16).reshape(4, 7, 19)
    ctx.focal(a, Spec("mean"), np.float32)
    before = ctx.focal_timing()
    bad = {
        "op: unknown focal op 9": Spec(9),
        "edge: unknown edge mode 3": Spec("mean", edge=3),
        "flags: unknown focal flags 0x10": Spec("mean", flags=16),
        "kh: window height 4": Spec("sum", (4, 3)),
        "kw: window width 17": Spec("sum", (3, 17)),
        "a median of 5 x 7 taps": Spec("median", (5, 7)),
        "take a 3 x 3 window": Spec("hillshade", 5),
        "FRA_FOCAL_NORMALIZE goes with": Spec("max", normalize=True),
    }
    for msg, spec in bad.items():
        dst = np.full((4, 7, 19), 5, np.float32)
        with pytest.raises(N.NativeError, match=msg) as e:
            ctx.focal(a, spec, np.float32, dst=dst)
        assert "error -1" in str(e.value)  # FRA_E_INVALID
        assert (dst == 5).all() and ctx.focal_timing() == before
        with pytest.raises(ValueError, match=msg):
            focal.validate(spec)
    for win in ((0, 0, 0, 19), (0, 0, 8, 19), (3, 10, 4, 10), (-1, 0, 2, 2)):
        dst = np.full((4, max(win[2], 1), win[3]), 5, np.float32)
        with pytest.raises(N.NativeError, match="the output rectangle"):
            ctx.focal(a, Spec("mean"), np.float32, dst=dst if win[2] else None, out_window=win)
        assert (dst == 5).all() and ctx.focal_timing() == before
    d = ctx.alloc(16)
    try:
        with pytest.raises(N.NativeError, match="bad raster layout"):
            ctx.focal(a, Spec("mean"), np.float32, dst=d, dst_strides=(0, -1, 1))
        with pytest.raises(N.NativeError, match="bad dtype"):
            N._check(_bad_dtype_job(ctx, d))
    finally:
        ctx.free(d)
    assert ctx.focal_timing() == before
    got, _ = ctx.focal(a, Spec("mean"), np.float32)  # the context goes on
    _same(got, focal_arrays(a, Spec("mean"), np.float32)[0])


# ------------------------------------------------------------------------------- 6. behind the decoder
H, W, TILE = 100, 130, 64  # 2 x 3 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -20.0, 4100000.0)
REGIONS = {"whole raster": (0, 0, H, W), "four tiles": (50, 50, 30, 30), "one pixel": (64, 64, 1, 1)}


def _scene(dt):
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(3000 + 2000 * np.sin(yy / 17.0 + b) + 800 * np.cos(xx / 23.0) + rng.integers(0, 40, (H, W)))
                  for b in range(B)])
    return (r / 7.0).astype(dt) if np.dtype(dt).kind == "f" else r.astype(dt)


@functools.lru_cache(maxsize=None)
def _container(dt):
    from flac_raster.streaming import build_streaming, read_window

    src = _scene(dt)
    data = build_streaming(src, TRANSFORM, "EPSG:32633", TILE)
    host = read_window(data, window=(0, 0, H, W), device=None)[0]  # what the container holds: the source of the rule
    host.setflags(write=False)
    return data, host


@pytest.mark.parametrize("dt", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_regions_are_crops_of_the_whole_result(dt):
    from flac_raster.streaming import focal_window

    data, host = _container(dt)
    ctx = _ctx()
    nd = float(host[2, 60, 70])
    rng = np.random.default_rng(4)
    terrain = {"hillshade": lambda dx, dy: Spec("hillshade", 3, "clamp", params=hillshade_params(315.0, 45.0, 1.0, dx, dy)),
               "slope": lambda dx, dy: Spec("slope", 3, "skip", nd, params=slope_params(1.0, dx, dy, 100.0))}
    cases = [(Spec("mean", 3, "skip", nd), np.float32), (Spec("median", 5, "clamp", nd, keep_mask=True), np.uint16),
             (Spec("max", (15, 15), "skip"), np.float64), (Spec("convolve", (1, 15), "clamp", nd, normalize=True, weights=_weights((1, 15), rng)), np.int16),
             (terrain["hillshade"], np.uint8), (terrain["slope"], np.float32)]
    for make, odt in cases:
        spec = make(10.0, 20.0) if callable(make) else make  # dx = |a|, dy = |e| of the transform
        whole, wleft = focal_arrays(host, spec, odt)
        for name, win in REGIONS.items():
            r, c, h, w = win
            dev, left, dwin, idx = focal_window(data, make, window=win, out_dtype=odt, device=0)
            _same(dev, whole[:, r:r + h, c:c + w], f"{name} {_name(spec)} -> {np.dtype(odt)}")  # the halo is there
            assert tuple(dwin) == win and len(idx["frames"]) == 6
            if win == (0, 0, H, W):
                assert left.tolist() == wleft.tolist()
            cpu, cleft, cwin, _ = focal_window(data, make, window=win, out_dtype=odt, device=None)
            _same(cpu, dev, f"{name} {_name(spec)}: host path")
            assert cleft.tolist() == left.tolist() and tuple(cwin) == win
        t = ctx.decode_timing()
        assert len(t) == 4 and t[3] >= 0.0 and ctx.focal_timing() >= 0.0
    res, _, win, _ = focal_window(data, Spec("mean"), device=0)
    assert tuple(win) == (0, 0, H, W) and res.shape == (B, H, W) and res.dtype == np.float32


def test_uncovered_region_and_bad_rectangles_are_refused_and_the_context_goes_on():
    from flac_raster.streaming import _tile_items

    data, host = _container(np.uint16)
    ctx = _ctx()
    _, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    roi, inner = (49, 49, 32, 32), (1, 1, 30, 30)
    spec = Spec("mean")
    hit = [k for k, it in enumerate(items) if it["window"][0] < 81 and it["window"][0] + it["window"][2] > 49
           and it["window"][1] < 81 and it["window"][1] + it["window"][3] > 49]
    assert len(hit) == 4
    with pytest.raises(N.NativeError, match="do not cover the region"):
        ctx.decode_device_focal(blob, [it for k, it in enumerate(items) if k != hit[-1]], host.dtype, B, roi, spec, inner,
                                denorm=N.DENORM_PCM16)
    with pytest.raises(N.NativeError, match="the inner rectangle"):
        ctx.decode_device_focal(blob, items, host.dtype, B, roi, spec, (1, 1, 32, 30), denorm=N.DENORM_PCM16)
    with pytest.raises(N.NativeError, match="kh: window height"):
        ctx.decode_device_focal(blob, items, host.dtype, B, roi, Spec("mean", (2, 3)), inner, denorm=N.DENORM_PCM16)
    d = ctx.alloc(64)
    try:
        with pytest.raises(N.NativeError, match="region of interest"):
            ctx.decode_device_focal(blob, items, host.dtype, B, (0, 0, 0, 5), spec, (0, 0, 1, 1), dst=d, denorm=N.DENORM_PCM16)
    finally:
        ctx.free(d)
    got, left, _ = ctx.decode_device_focal(blob, [items[k] for k in hit], host.dtype, B, roi, spec, inner, denorm=N.DENORM_PCM16)
    _same(got, focal_arrays(host, spec, np.float32, (50, 50, 30, 30))[0], "after the refusals")
    assert left.tolist() == [0] * B


def test_focal_cli_on_the_device(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.tiff import read_geotiff, write_geotiff

    data, host = _container(np.uint16)
    flac = tmp_path / "scene_streaming.flac"
    flac.write_bytes(data)
    out = tmp_path / "out.tif"
    res = CliRunner().invoke(app, ["focal", str(flac), "-o", str(out), "--op", "mean", "--size", "5", "--window", "50,50,30,30",
                                   "--device", "0"])
    assert res.exit_code == 0 and "GPU 0" in res.output, res.output
    got, info = read_geotiff(out)
    _same(got, focal_arrays(host, Spec("mean", 5), np.float32, (50, 50, 30, 30))[0], "cli, container")
    assert tuple(info.transform)[:6] == (10.0, 0.0, 500500.0, 0.0, -20.0, 4099000.0)
    tif = tmp_path / "scene.tif"
    write_geotiff(tif, np.asarray(host), transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    res = CliRunner().invoke(app, ["hillshade", str(tif), "-o", str(out), "--nodata", str(int(host[0, 10, 10])), "--fill", "255",
                                   "--device", "0"])
    assert res.exit_code == 0 and "left out" in res.output, res.output
    got, info = read_geotiff(out)
    spec = Spec("hillshade", 3, "skip", float(host[0, 10, 10]), 255.0, params=hillshade_params(315.0, 45.0, 1.0, 10.0, 20.0, 255.0))
    want, left = focal_arrays(host, spec, np.uint8)
    _same(got, want, "cli, tiff")
    assert left[0] > 0 and info.nodata == 255
