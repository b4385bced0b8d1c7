"""GPU tests of the band math (``k_calc`` alone through ``fra_calc``, and behind the windowed read through
``fra_decode_device_calc``).

The expectation is never the kernel: it is ``calc.calc_arrays`` -- the rule in numpy, checked on the CPU against a
brute-force per-pixel loop -- applied to the raster itself or to the host ``read_window``.  The comparison is bit for
bit for every output dtype, floats included: every op is one IEEE f64 operation and the rule fixes the NaN a float
output holds, so there is no tolerance to choose.  The shapes are those of ``test_gpu_stats.py``: the smallest at which
the thread mapping can go wrong, the last one with several workgroups and a ragged tail.
"""
import functools

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import calc
from flac_raster.calc import Program, calc_arrays, compile_exprs
from flac_raster.geo import Affine

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
SHAPES = [(1, 1), (7, 19), (33, 67), (130, 517)]
B = 4
NDVI = "(b4 - b3) / (b4 + b3)"
STRETCH = ["clamp((b3 - 3) * 255 / 90, 0, 255)", "clamp((b2 - 3) * 255 / 90, 0, 255)", "clamp((b1 - 3) * 255 / 90, 0, 255)"]
SCENE_STRETCH = [f"clamp((b{k} - {lo}) * 255 / {span}, 0, 255)" for k, lo, span in ((3, 1000, 5000), (2, 150, 700), (1, 0, 6000))]
DEPTH8 = "b1 - (b2 * (b3 + (b4 / (b1 - (b2 * (b3 + b4))))))"
DEPTH4 = "b1 - (b2 * (b3 + b4))"  # the first depth at which k_calc evaluates 4 pixels of a lane per word, not 8
LONG = " + ".join(["b1", "b2"] * 32)  # 64 operands: 64 BAND + 63 ADD + STORE = 128 words


def _ctx():
    return N.default_context(0)


def _raster(dt, shape, rng):
    """Half small values (zeros and ties for the comparisons, the logic and the divisions), half the full range; floats
    with NaN, +-inf and -0.0 sprinkled in."""
    dt = np.dtype(dt)
    small = rng.integers(0, 4, size=shape)
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


def _op_programs():
    """Every op alone: its operands are bands, the result is stored."""
    progs = {"CONST": Program([calc.CONST, calc.STORE], [-2.5], 1)}
    for name in ("NEG", "ABS", "SQRT", "FLOOR", "NOT"):
        progs[name] = Program([calc.BAND, getattr(calc, name), calc.STORE], [], 1)
    for name in ("ADD", "SUB", "MUL", "DIV", "MIN", "MAX", "LT", "LE", "GT", "GE", "EQ", "NE", "AND", "OR"):
        progs[name] = Program([calc.BAND, calc.BAND | 1 << 8, getattr(calc, name), calc.STORE], [], 1)
    progs["SELECT"] = Program([calc.BAND, calc.BAND | 1 << 8, calc.BAND | 2 << 8, calc.SELECT, calc.STORE], [], 1)
    assert set(progs) | {"BAND", "STORE"} == set(calc.OPS)
    return progs


# ------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_op_alone_for_every_output_dtype(dt):
    rng = np.random.default_rng(900 + np.dtype(dt).num)
    ctx = _ctx()
    a = _raster(dt, (B, 33, 67), rng)
    for name, prog in _op_programs().items():
        for odt in DTYPES:
            want, _ = calc_arrays(a, prog, odt)
            got, left = ctx.calc(a, prog, odt)
            _same(got, want, f"{name} {np.dtype(dt)} -> {np.dtype(odt)}")
            assert left.tolist() == [0]


PROGRAMS = {"ndvi": [NDVI], "long": [LONG], "depth8": [DEPTH8], "depth4": [DEPTH4], "stretch": STRETCH, "band2": ["b2 * 2"],
            "logic": ["where(b1 > b2 and not b3 == 0 or b4 <= 1, floor(sqrt(abs(b1))), -min(b2, max(b3, 0.5)))"]}


@functools.lru_cache(maxsize=None)
def _program(name):
    p = compile_exprs(PROGRAMS[name], B)
    if name == "long":
        assert p.code.size == 128
    if name in ("depth8", "depth4", "ndvi"):  # depth 3 and 4: either side of the kernel's choice of instance
        assert calc.validate(p, B) == {"depth8": 8, "depth4": 4, "ndvi": 3}[name]
    return p


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_programs_shapes_and_output_dtypes(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(300 + dt.num)
    ctx = _ctx()
    for (h, w) in SHAPES:
        a = _raster(dt, (B, h, w), rng)
        for name in PROGRAMS:
            prog = _program(name)
            for odt in DTYPES:
                want, _ = calc_arrays(a, prog, odt)
                got, _ = ctx.calc(a, prog, odt)
                _same(got, want, f"{name} {dt} {(h, w)} -> {np.dtype(odt)}")
        assert ctx.calc_timing() >= 0.0


# A thread's way from one of its slots to the next, 256 slots on in row-major order, at its two corners.  (3, 4113): more
# than 256 slots of 8 pixels per row (no whole row in a step), the last slot of a row holds 1 pixel.  (5, 511): 64 slots
# per row (a step is four rows, no slots) and a short last slot.
CURSOR_SHAPES = [(3, 4113), (5, 511)]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_rows_of_more_than_256_slots_and_whole_row_steps(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(350 + dt.num)
    ctx = _ctx()
    prog = compile_exprs(["b1", "b1 + b2"], B)
    for (h, w) in CURSOR_SHAPES:
        a = _raster(dt, (B, h, w), rng)
        av = _padded(a, 6)[1]  # rows of an odd number of elements: element loads
        assert av.strides[1] % 16
        for odt in (dt, np.float64):
            want, _ = calc_arrays(a, prog, odt)
            _same(ctx.calc(a, prog, odt)[0], want, f"{dt} {(h, w)} -> {np.dtype(odt)}")  # contiguous
            _same(ctx.calc(av, prog, odt)[0], want, f"{dt} {(h, w)} padded -> {np.dtype(odt)}")


def test_ndvi_with_zero_denominators():
    ctx = _ctx()
    rng = np.random.default_rng(5)
    a = rng.integers(-2, 3, size=(B, 33, 67)).astype(np.int16)  # b4 + b3 == 0 often: 0 / 0 and x / 0
    prog = _program("ndvi")
    f, _ = calc_arrays(a, prog, np.float32)
    assert np.isnan(f).any() and np.isinf(f).any()
    for odt in DTYPES:
        want, _ = calc_arrays(a, prog, odt)
        got, _ = ctx.calc(a, prog, odt)
        _same(got, want, f"ndvi -> {np.dtype(odt)}")
    i, _ = ctx.calc(a, prog, np.int16)
    assert i[0][np.isnan(f[0])].tolist() == [0] * int(np.isnan(f).sum())
    big = compile_exprs(["b1 * 1e30 / b2"], B)  # saturates the integers, overflows float32
    for odt in DTYPES:
        _same(ctx.calc(a, big, odt)[0], calc_arrays(a, big, odt)[0], f"saturation -> {np.dtype(odt)}")


# ------------------------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("dt,odt", [(np.uint16, np.float32), (np.uint8, np.uint8), (np.float64, np.int16),
                                    (np.float32, np.float64), (np.int32, np.uint16)],
                         ids=lambda d: np.dtype(d).name)
def test_layouts(dt, odt):
    dt, odt = np.dtype(dt), np.dtype(odt)
    rng = np.random.default_rng(70 + dt.num + odt.num)
    ctx = _ctx()
    for (h, w) in SHAPES:
        a = _raster(dt, (B, h, w), rng)
        for name in ("ndvi", "stretch", "depth4"):
            prog = _program(name)
            nout = prog.nout
            want, _ = calc_arrays(a, prog, odt)
            V, OV = 16 // dt.itemsize, 16 // odt.itemsize
            abig16, av16 = _padded(a, -w % V + V)   # rows 16-byte aligned: vector loads
            abig5, av5 = _padded(a, 5)              # rows not 16-byte aligned: element loads
            wide = np.full((B, h, 2 * w), 77, dt)
            wide[:, :, ::2] = a
            keep = abig16.tobytes(), abig5.tobytes(), wide.tobytes()
            for view in (av16, av5, wide[:, :, ::2]):
                _same(ctx.calc(view, prog, odt)[0], want, f"{name} source view {view.strides}")
            assert (abig16.tobytes(), abig5.tobytes(), wide.tobytes()) == keep  # nothing is written to the source
            # host destinations: the caller's values between the outputs stay
            for pad in (-w % OV + OV, 5):
                obig = np.full((nout, h + 1, w + pad), 77, odt)
                ret, _ = ctx.calc(a, prog, odt, dst=obig[:, :h, :w])
                _same(obig[:, :h, :w], want, f"{name} padded destination {pad}")
                assert (obig[:, h] == 77).all() and (obig[:, :, w:] == 77).all()
            owide = np.full((nout, h, 2 * w), 77, odt)
            ctx.calc(av5, prog, odt, dst=owide[:, :, ::2])
            _same(owide[:, :, ::2], want, f"{name} column stride 2")
            assert (owide[:, :, 1::2] == 77).all()
            # device source and destination
            rs, ors = w + (-w % V), w + (-w % OV) + OV
            sa = np.full((B, h, rs), 77, dt)
            sa[:, :, :w] = a
            so = np.full((nout, h, ors), 77, odt)
            d_a, d_o = ctx.alloc(sa.nbytes), ctx.alloc(so.nbytes)
            try:
                ctx.h2d(d_a, sa)
                ctx.h2d(d_o, so)
                ctx.calc(d_a, prog, odt, dst=d_o, dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1),
                         dst_strides=(h * ors, ors, 1))
                back = np.empty_like(so)
                ctx.d2h(back, d_o)
                _same(back[:, :, :w], want, f"{name} device to device")
                assert (back[:, :, w:] == 77).all()
                got, _ = ctx.calc(d_a, prog, odt, dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1))
                _same(got, want, f"{name} device to host")
                src_back = np.empty_like(sa)
                ctx.d2h(src_back, d_a)
                assert src_back.tobytes() == sa.tobytes()
            finally:
                ctx.free(d_a)
                ctx.free(d_o)


# ------------------------------------------------------------------------------- 3. nodata
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
        cases = [(nd, None), (absent, None), (nd, 42.5), (float("nan"), None)]
        for name in ("ndvi", "band2", "stretch", "depth4"):
            prog = _program(name)
            for nodata, fill in cases:
                for odt in (np.float32, np.uint8, np.int32, np.float64):
                    f = calc.default_fill(odt) if fill is None else fill
                    want, wleft = calc_arrays(a, prog, odt, nodata, f)
                    got, left = ctx.calc(a, prog, odt, nodata=nodata, fill=fill)
                    _same(got, want, f"{name} {dt} {(h, w)} nodata {nodata} fill {fill} -> {np.dtype(odt)}")
                    assert left.tolist() == wleft.tolist()
                    again, left2 = ctx.calc(a, prog, odt, nodata=nodata, fill=fill)
                    assert again.tobytes() == got.tobytes() and left2.tolist() == left.tolist()
        # a program that reads band 2 alone ignores the other bands' nodata
        only2 = np.count_nonzero((a[1].astype(np.float64) == nd) | np.isnan(a[1].astype(np.float64)))
        _, left = ctx.calc(a, _program("band2"), np.float32, nodata=nd)
        assert left.tolist() == [only2]
        if dt.kind == "f":  # NaN pixels are left out whatever the nodata value is, and only with one
            nans = np.count_nonzero(np.isnan(a[1]))
            assert nans > 0
            assert ctx.calc(a, _program("band2"), np.float32, nodata=float("nan"))[1].tolist() == [nans]
            assert ctx.calc(a, _program("band2"), np.float32)[1].tolist() == [0]


# ------------------------------------------------------------------------------- 4. refusals reach Python
def _bad_dtype_job(ctx, d):
    """``fra_calc`` with a destination dtype outside ``fra_dtype``."""
    import ctypes as C

    job = N.CalcJob()
    job.src, job.src_on_device, job.dtype, job.channels, job.height, job.width = C.c_void_p(int(d)), 1, 2, 4, 1, 1
    job.band_stride, job.row_stride, job.col_stride = 1, 1, 1
    job.program = N.calc_program(_program("ndvi"))
    job.out.dst, job.out.dst_on_device, job.out.dtype = C.c_void_p(int(d)), 1, 8
    job.out.band_stride, job.out.row_stride, job.out.col_stride = 1, 1, 1
    return N.load().fra_calc(ctx.h, C.byref(job), None)


def test_an_invalid_program_is_refused_before_any_launch():
    ctx = _ctx()
    a = np.arange(4 * 7 * 19, dtype=np.uint16).reshape(4, 7, 19)
    ctx.calc(a, _program("ndvi"), np.float32)
    before = ctx.calc_timing()
    bad = {
        "word 1: band 4 of 4": Program([calc.BAND, calc.BAND | 4 << 8, calc.ADD, calc.STORE], [], 1),
        "word 2: stack underflow": Program([calc.BAND, calc.NEG, calc.ADD, calc.STORE], [], 1),
        "word 0: unknown op 23": Program([23, calc.STORE], [], 1),
        "word 0: constant 0 of 0": Program([calc.CONST, calc.STORE], [], 1),
        "word 3: output 0 stored twice": Program([calc.BAND, calc.STORE, calc.BAND, calc.STORE], [], 1),
        "word 1: output 1 is never stored": Program([calc.BAND, calc.STORE], [], 2),
        "word 8: stack deeper than 8": Program([calc.BAND] * 9 + [calc.ADD] * 8 + [calc.STORE], [], 1),
        "word 2: 1 values left": Program([calc.BAND, calc.BAND, calc.STORE], [], 1),
    }
    for msg, prog in bad.items():
        dst = np.full((prog.nout, 7, 19), 5, np.float32)
        with pytest.raises(N.NativeError, match=msg) as e:
            ctx.calc(a, prog, np.float32, dst=dst)
        assert "error -1" in str(e.value)  # FRA_E_INVALID
        assert (dst == 5).all() and ctx.calc_timing() == before
        with pytest.raises(ValueError, match=msg):
            calc.validate(prog, 4)
    d = ctx.alloc(16)
    try:
        with pytest.raises(N.NativeError, match="bad raster layout"):
            ctx.calc(a, _program("ndvi"), np.float32, dst=d, dst_strides=(0, -1, 1))
        with pytest.raises(N.NativeError, match="bad dtype"):
            N._check(_bad_dtype_job(ctx, d))
    finally:
        ctx.free(d)
    got, _ = ctx.calc(a, _program("ndvi"), np.float32)  # the context goes on
    _same(got, calc_arrays(a, _program("ndvi"), np.float32)[0])


# ------------------------------------------------------------------------------- 5. behind the decoder
H, W, TILE = 100, 130, 64  # 2 x 3 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
REGIONS = {"whole raster": (0, 0, H, W), "four tiles": (50, 50, 30, 30), "one pixel": (70, 100, 1, 1)}


def _scene(dt):
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(3000 + 2000 * np.sin(yy / 17.0 + b) + 800 * np.cos(xx / 23.0) + rng.integers(0, 40, (H, W)))
                  for b in range(B)])
    return (r / 7.0).astype(dt) if np.dtype(dt).kind == "f" else r.astype(dt)


@functools.lru_cache(maxsize=None)
def _container(dt):
    from flac_raster.streaming import build_streaming

    src = _scene(dt)
    data = build_streaming(src, TRANSFORM, "EPSG:32633", TILE)
    src.setflags(write=False)
    return data, src


@pytest.mark.parametrize("dt", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_regions_against_the_host_read(dt):
    from flac_raster.streaming import calc_window, read_window

    data, src = _container(dt)
    ctx = _ctx()
    for name, win in REGIONS.items():
        host = read_window(data, window=win, device=None)[0]
        nd = float(host[2, win[2] // 2, win[3] // 2])
        for exprs, odt, nodata in (([NDVI], np.float32, None), (SCENE_STRETCH, np.uint8, None), ([NDVI, "b2"], np.float64, nd),
                                   ([NDVI], np.int16, nd)):
            prog = compile_exprs(exprs, B)
            want, wleft = calc_arrays(host, prog, odt, nodata, calc.default_fill(odt))
            dev, left, dwin, idx = calc_window(data, exprs, window=win, out_dtype=odt, nodata=nodata, device=0)
            _same(dev, want, f"{name} {exprs} -> {np.dtype(odt)}")
            assert left.tolist() == wleft.tolist() and tuple(dwin) == win and len(idx["frames"]) == 6
            cpu, cleft, cwin, _ = calc_window(data, exprs, window=win, out_dtype=odt, nodata=nodata, device=None)
            _same(cpu, dev, f"{name}: host path")
            assert cleft.tolist() == left.tolist() and tuple(cwin) == win
        t = ctx.decode_timing()
        assert len(t) == 4 and t[3] >= 0.0 and ctx.calc_timing() >= 0.0
    whole, _, win, _ = calc_window(data, [NDVI], device=0)
    assert tuple(win) == (0, 0, H, W) and whole.shape == (1, H, W) and whole.dtype == np.float32


def test_uncovered_region_and_bad_roi_are_refused_and_the_context_goes_on():
    from flac_raster.streaming import _tile_items

    data, src = _container(np.uint16)
    ctx = _ctx()
    _, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    win = REGIONS["four tiles"]
    prog = _program("ndvi")
    hit = [k for k, it in enumerate(items) if it["window"][0] < 80 and it["window"][0] + it["window"][2] > 50
           and it["window"][1] < 80 and it["window"][1] + it["window"][3] > 50]
    assert len(hit) == 4
    with pytest.raises(N.NativeError, match="do not cover the region"):
        ctx.decode_device_calc(blob, [it for k, it in enumerate(items) if k != hit[-1]], src.dtype, B, win, prog,
                               denorm=N.DENORM_PCM16)
    d = ctx.alloc(64)
    try:
        with pytest.raises(N.NativeError, match="region of interest"):
            ctx.decode_device_calc(blob, items, src.dtype, B, (0, 0, 0, 5), prog, dst=d, denorm=N.DENORM_PCM16)
    finally:
        ctx.free(d)
    with pytest.raises(N.NativeError, match="word 0: band 3 of 3"):
        ctx.decode_device_calc(blob, items, src.dtype, 3, win, prog, denorm=N.DENORM_PCM16)
    got, left, _ = ctx.decode_device_calc(blob, [items[k] for k in hit], src.dtype, B, win, prog, denorm=N.DENORM_PCM16)
    assert got.shape == (1, 30, 30) and left.tolist() == [0]


def test_calc_cli_on_the_device(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.streaming import read_window
    from flac_raster.tiff import read_geotiff, write_geotiff

    data, src = _container(np.uint16)
    flac = tmp_path / "scene_streaming.flac"
    flac.write_bytes(data)
    out = tmp_path / "ndvi.tif"
    res = CliRunner().invoke(app, ["calc", str(flac), "-o", str(out), "--expr", NDVI, "--window", "50,50,30,30",
                                   "--device", "0"])
    assert res.exit_code == 0, res.output
    got, info = read_geotiff(out)
    host = read_window(data, window=(50, 50, 30, 30), device=None)[0]
    _same(got, calc_arrays(host, compile_exprs([NDVI], B), np.float32)[0], "cli, container")
    assert info.nodata is None and tuple(info.transform)[:6] == (10.0, 0.0, 500500.0, 0.0, -10.0, 4099500.0)
    # a GeoTIFF source, three 8-bit outputs, nodata: the tag is the fill
    tif = tmp_path / "scene.tif"
    write_geotiff(tif, np.asarray(src), transform=tuple(TRANSFORM)[:6], crs="EPSG:32633")
    out2 = tmp_path / "rgb.tif"
    nd = float(src[0, 10, 10])
    args = ["calc", str(tif), "-o", str(out2), "--dtype", "uint8", "--nodata", str(nd), "--fill", "255", "--device", "0"]
    for e in SCENE_STRETCH:
        args += ["--expr", e]
    res = CliRunner().invoke(app, args)
    assert res.exit_code == 0, res.output
    assert "left out" in res.output
    got, info = read_geotiff(out2)
    want, left = calc_arrays(np.asarray(src), compile_exprs(SCENE_STRETCH, B), np.uint8, nd, 255.0)
    _same(got, want, "cli, tiff")
    assert left[0] > 0 and info.nodata == 255.0
    res = CliRunner().invoke(app, ["calc", str(tif), "-o", str(out2), "--expr", "b9 ** 2", "--device", "0"])
    assert res.exit_code == 1 and "Error" in res.output
