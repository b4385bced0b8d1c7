"""CPU tests of the focal operations: the numpy rule (``focal.focal_arrays``) against a per-pixel loop written straight
from the rule in ``include/flac_raster_amd.h``, the validators, the ABI, the command line with ``--cpu`` and the
stand-alone host check.  No GPU.

The comparison is bit for bit: every step of the rule is one IEEE f64 operation, numpy's f64 scalars and arrays do the
same operations, and the rule fixes the order of the taps and the NaN a float output holds.
"""
import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import calc, focal
from flac_raster.focal import Spec, focal_arrays, hillshade_params, slope_params

ROOT = Path(__file__).resolve().parents[1]
F = np.float64


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


def _raster(dt, shape, rng):
    """Small values with ties, 7 (the nodata of the tests) here and there; floats with NaN, +-inf and -0.0."""
    dt = np.dtype(dt)
    a = rng.integers(-3, 12, size=shape).astype(dt) if dt.kind != "u" else rng.integers(0, 12, size=shape).astype(dt)
    if dt.kind == "f":
        a = (a * dt.type(0.37)).astype(dt)
        a[rng.random(shape) < 0.15] = dt.type(7)
        flat = a.reshape(-1)
        for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, -0.0)):
            flat[(3 + 5 * k) % flat.size] = v
    return a


def _taps(a, b, i, j, spec, win):
    """The taps of output pixel (i, j) of band b in row-major order: (value as f64, valid)."""
    _, h, w = a.shape
    ry, rx = spec.kh // 2, spec.kw // 2
    taps = []
    for dy in range(spec.kh):
        for dx in range(spec.kw):
            y, x = win[0] + i + dy - ry, win[1] + j + dx - rx
            if not (0 <= y < h and 0 <= x < w):
                if spec.edge == focal.EDGE_SKIP:
                    taps.append((F(0.0), False))
                    continue
                y, x = min(max(y, 0), h - 1), min(max(x, 0), w - 1)
            v = F(a[b, y, x])
            left_out = bool(np.isnan(v)) or (spec.nodata is not None and bool(v == F(spec.nodata)))
            taps.append((v, not left_out))
    return taps


def _pixel(taps, spec):
    """One output pixel by the rule: (the f64 result, whether it gets fill instead)."""
    valid = [v for v, ok in taps if ok]
    n = len(valid)
    centre_out = not taps[(spec.kh // 2) * spec.kw + spec.kw // 2][1]
    got_fill, r = False, F(0.0)
    op = spec.op
    if op in (focal.SLOPE, focal.HILLSHADE):
        if n < 9:
            got_fill = True
        else:
            a, b, c, d, _, f, g, h, i = (v for v, _ in taps)
            zx = ((c + (f + f)) + i) - ((a + (d + d)) + g)
            zy = ((a + (b + b)) + c) - ((g + (h + h)) + i)
            P = [F(v) for v in spec.params]
            p, q = zx * P[0], zy * P[1]
            if op == focal.SLOPE:
                r = np.sqrt(p * p + q * q) * P[2]
            else:
                s = ((P[4] - p * P[2]) - q * P[3]) / np.sqrt((F(1.0) + p * p) + q * q)
                s = s if s > 0 else F(0.0)
                r = s * P[5]
    elif op == focal.COUNT:
        r = F(n)
    elif n == 0:
        got_fill = True
    elif op in (focal.SUM, focal.MEAN):
        r = valid[0]
        for v in valid[1:]:
            r = r + v
        if op == focal.MEAN:
            r = r / F(n)
    elif op == focal.MIN:
        r = valid[0]
        for v in valid[1:]:
            r = v if v < r else r
    elif op == focal.MAX:
        r = valid[0]
        for v in valid[1:]:
            r = v if v > r else r
    elif op == focal.MEDIAN:
        r = sorted(valid)[(n - 1) // 2]  # a stable sort: equal values stay in tap order
    elif op == focal.CONVOLVE:
        ws = [F(wt) for (v, ok), wt in zip(taps, spec.weights.reshape(-1)) if ok]
        r, s = valid[0] * ws[0], ws[0]
        for v, wt in zip(valid[1:], ws[1:]):
            r = r + v * wt
            s = s + wt
        if spec.normalize:
            if s == 0.0:
                got_fill = True
            else:
                r = r / s
    if spec.keep_mask and centre_out:
        got_fill = True
    return r, got_fill


def _brute(a, specs, odts, win=None):
    """Every spec of ``specs`` (which share window, edge mode and nodata) by the per-pixel loop: per spec, the result in
    every dtype of ``odts`` and the per-band count of pixels that got fill."""
    B, h, w = a.shape
    win = win or (0, 0, h, w)
    outs = [np.zeros((B, win[2], win[3]), F) for _ in specs]
    filled = [np.zeros((B, win[2], win[3]), bool) for _ in specs]
    with np.errstate(all="ignore"):
        for b in range(B):
            for i in range(win[2]):
                for j in range(win[3]):
                    taps = _taps(a, b, i, j, specs[0], win)
                    for k, s in enumerate(specs):
                        outs[k][b, i, j], filled[k][b, i, j] = _pixel(taps, s)
    res = []
    for s, o, f in zip(specs, outs, filled):
        fills = [F(calc.default_fill(odt) if s.fill is None else s.fill) for odt in odts]
        res.append(([calc.convert(np.where(f, fill, o), odt) for odt, fill in zip(odts, fills)], f.sum(axis=(1, 2)).astype(np.uint64)))
    return res


def _specs(size, edge, nodata, rng):
    """Every op that takes the window ``size``, with and without KEEP_MASK and NORMALIZE."""
    kh, kw = size
    out = []
    for op in ("sum", "mean", "min", "max", "count"):
        out.append(Spec(op, size, edge, nodata, keep_mask=op in ("mean", "count")))
    out.append(Spec("sum", size, edge, nodata, fill=-5.5))
    if kh * kw <= 25:
        out.append(Spec("median", size, edge, nodata))
        out.append(Spec("median", size, edge, nodata, keep_mask=True))
    wts = rng.integers(-2, 3, size=size).astype(F)
    wts[kh // 2, kw // 2] = 0.25
    for norm in (False, True):
        out.append(Spec("convolve", size, edge, nodata, normalize=norm, weights=wts, keep_mask=norm))
    if kh * kw > 1:
        zero = np.zeros(size)
        zero.reshape(-1)[:2] = 1.0, -1.0  # the weights of the valid taps often add up to 0
        out.append(Spec("convolve", size, edge, nodata, normalize=True, weights=zero))
    if size == (3, 3):
        out.append(Spec("slope", 3, edge, nodata, params=slope_params(2.0, 10.0, 20.0, 100.0)))
        out.append(Spec("hillshade", 3, edge, nodata, keep_mask=True, params=hillshade_params(315.0, 45.0, 1.0, 3.0, 2.0)))
        out.append(Spec("hillshade", 3, edge, nodata, params=hillshade_params(100.0, 10.0, 5.0, 1.0, 1.0, 1.0)))
    return out


SIZES = [(1, 1), (3, 3), (3, 7), (5, 5), (15, 15)]


@pytest.mark.parametrize("dt", [np.int16, np.float32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_focal_arrays_equals_the_per_pixel_loop(dt, size):
    rng = np.random.default_rng(11 + size[0] * 16 + size[1] + np.dtype(dt).num)
    seen_fill = 0
    for shape in ((1, 1), (2, 5), (9, 13)):
        a = _raster(dt, (2,) + shape, rng)
        for edge in ("skip", "clamp"):
            for nodata in (None, 7.0, math.nan):
                specs = _specs(size, edge, nodata, rng)
                odts = (np.float64, np.int16)
                for s, (wants, left) in zip(specs, _brute(a, specs, odts)):
                    for odt, want in zip(odts, wants):
                        got, gleft = focal_arrays(a, s, odt)
                        _same(got, want, (focal.OPS[s.op], size, shape, edge, nodata, np.dtype(odt).name, s.keep_mask, s.normalize))
                        assert gleft.tolist() == left.tolist() and gleft.dtype == np.uint64
                    seen_fill += int(left.sum())
    assert seen_fill > 0 or size == (1, 1) and np.dtype(dt).kind != "f"


def test_an_output_rectangle_is_the_crop_of_the_whole_result():
    rng = np.random.default_rng(3)
    a = _raster(np.float32, (2, 9, 13), rng)
    for size in ((3, 3), (3, 7), (5, 5)):
        for edge in ("skip", "clamp"):
            for s in _specs(size, edge, 7.0, rng):
                whole, _ = focal_arrays(a, s, np.float32)
                for win in ((0, 0, 4, 5), (5, 8, 4, 5), (3, 4, 2, 3), (8, 12, 1, 1)):
                    part, left = focal_arrays(a, s, np.float32, win)
                    _same(part, whole[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]], (focal.OPS[s.op], size, edge, win))
                    (want,), wleft = _brute(a, [s], (np.float32,), win)[0]
                    _same(part, want, "rectangle by the loop")
                    assert left.tolist() == wleft.tolist()
    for win in ((0, 0, 0, 3), (0, 0, 10, 3), (-1, 0, 2, 2), (0, 12, 1, 2)):
        with pytest.raises(ValueError, match="output rectangle"):
            focal_arrays(a, Spec("mean"), np.float32, win)


# ------------------------------------------------------------------------------- the validators
def _bad_specs():
    w33 = np.ones((3, 3))
    return {
        "op: unknown focal op 9": Spec(9),
        "op: unknown focal op -1": Spec(-1),
        "edge: unknown edge mode 2": Spec("mean", edge=2),
        "flags: unknown focal flags 0x8": Spec("mean", flags=8),
        "kh: window height 4 is not odd and in 1 ... 15": Spec("mean", (4, 3)),
        "kh: window height 17 is not odd and in 1 ... 15": Spec("mean", (17, 3)),
        "kw: window width 0 is not odd and in 1 ... 15": Spec("mean", (3, 0)),
        "kw: window width 2 is not odd and in 1 ... 15": Spec("max", (1, 2)),
        "kh, kw: a median of 5 x 7 taps, more than 25": Spec("median", (5, 7)),
        "kh, kw: a median of 3 x 9 taps, more than 25": Spec("median", (3, 9)),
        "kh, kw: slope and hillshade take a 3 x 3 window, not 5 x 5": Spec("slope", 5),
        "kh, kw: slope and hillshade take a 3 x 3 window, not 3 x 1": Spec("hillshade", (3, 1)),
        r"flags: FRA_FOCAL_NORMALIZE goes with FRA_FOCAL_CONVOLVE alone \(op 1\)": Spec("mean", normalize=True),
        r"flags: FRA_FOCAL_NORMALIZE goes with FRA_FOCAL_CONVOLVE alone \(op 7\)": Spec("slope", normalize=True),
        # the first rule broken names the refusal
        "op: unknown focal op 12": Spec(12, (4, 4), edge=5),
        "edge: unknown edge mode 5": Spec("convolve", (4, 4), edge=5, weights=np.ones((4, 4))),
        "kh: window height 2 is not odd and in 1 ... 15": Spec("median", (2, 2), normalize=True),
        "a median of 7 x 7 taps": Spec("median", 7, normalize=True),
        "_ok": [Spec("mean", 15), Spec("median", 5), Spec("median", (1, 15)), Spec("median", (3, 7), keep_mask=True),
                Spec("convolve", 3, normalize=True, weights=w33, nodata=math.nan, fill=math.inf), Spec("count", (15, 1), "clamp"),
                Spec("slope", params=slope_params()), Spec("hillshade", params=hillshade_params())],
    }


def test_every_refusal_of_the_spec_validator_reaches_python():
    bad = _bad_specs()
    for s in bad.pop("_ok"):
        focal.validate(s)
        N.focal_check(s)
    for msg, s in bad.items():
        with pytest.raises(ValueError, match=msg):
            focal.validate(s)
        with pytest.raises(N.NativeError, match=msg) as e:
            N.focal_check(s)
        assert "error -1" in str(e.value)  # FRA_E_INVALID
        with pytest.raises(ValueError, match=msg):
            focal_arrays(np.zeros((1, 4, 4), np.int16), s, np.float32)
    assert N.load().fra_focal_check(None) == -1
    with pytest.raises(ValueError, match="unknown focal op"):
        Spec("mode")
    with pytest.raises(ValueError, match="unknown edge mode"):
        Spec("mean", edge="wrap")
    with pytest.raises(ValueError, match="weights"):
        Spec("convolve", 3, weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="weights"):
        focal.validate(Spec("convolve", 3))


def test_abi_names_and_layout():
    header = (ROOT / "include" / "flac_raster_amd.h").read_text()
    for name in ("fra_focal_check", "fra_focal", "fra_decode_device_focal", "fra_focal_timing"):
        assert name in N.EXPORTS and re.search(rf"FRA_API int {name}\(", header), name
        assert hasattr(N.load(), name)
    for name in ("fra_focal_spec", "fra_focal_job", "FRA_FOCAL_NODATA 1", "FRA_FOCAL_NORMALIZE 2", "FRA_FOCAL_KEEP_MASK 4",
                 "FRA_FOCAL_EDGE_SKIP = 0", "FRA_FOCAL_EDGE_CLAMP = 1", "#define FRA_ABI_VERSION 3"):
        assert name in header, name
    assert N.load().fra_abi_version() == 3
    assert C.sizeof(N.FocalSpec) == 1904 and N.FocalSpec.nodata.offset == 24 and N.FocalSpec.params.offset == 40
    assert N.FocalSpec.weights.offset == 104
    assert N.FocalJob.rect.offset == 56 and N.FocalJob.spec.offset == 72 and N.FocalJob.out.offset == 72 + 1904
    assert C.sizeof(N.FocalJob) == 72 + 1904 + 40
    for k, name in enumerate(focal.OPS):  # the op numbers of the header are those of focal.py
        assert re.search(rf"FRA_FOCAL_{name.upper()} = {k}\b", header), name
    assert (focal.MAX_SIZE, focal.MAX_MEDIAN) == (15, 25)
    assert (focal.FLAG_NODATA, focal.FLAG_NORMALIZE, focal.FLAG_KEEP_MASK) == (1, 2, 4)
    ms = C.c_float(-1.0)
    assert N.load().fra_focal_timing(C.byref(ms)) == 0 and ms.value >= 0.0
    assert N.load().fra_focal_timing(None) == -1
    csrc = ROOT / "flac-raster_amd" / "csrc"
    make = (csrc / "Makefile").read_text()
    assert re.search(r"^UNITS = [^#]*\bfra_focal\b", make, re.M | re.S) and re.search(r"^HOSTCHECK_UNITS = [^#]*fra_focal\.hip", make, re.M | re.S)


# ------------------------------------------------------------------------------- terrain
def test_a_north_facing_slope_is_brighter_lit_from_the_north():
    yy = np.mgrid[0:12, 0:15][0].astype(np.float32)
    dem = (100.0 + 3.0 * yy)[None]  # row 0 is north: the ground rises to the south, the slope faces north
    lit = {az: focal_arrays(dem, Spec("hillshade", params=hillshade_params(az, 45.0, 1.0, 10.0, 10.0, 255.0)), np.float64)[0]
           for az in (0.0, 180.0, 90.0, 270.0)}
    inner = (slice(None), slice(1, -1), slice(1, -1))
    assert (lit[0.0][inner] > lit[180.0][inner]).all() and (lit[180.0][inner] >= 0).all()
    np.testing.assert_allclose(lit[90.0][inner], lit[270.0][inner], rtol=1e-12)  # neither east nor west is favoured
    flat = focal_arrays(np.full((1, 5, 5), 9, np.int16), Spec("hillshade", params=hillshade_params(315.0, 30.0)), np.float64)[0]
    np.testing.assert_allclose(flat[0, 1:-1, 1:-1], 255.0 * math.sin(math.radians(30.0)), rtol=1e-12)
    assert np.isnan(flat[0, 0]).all()  # a tap outside the raster: fill
    s = focal_arrays(dem, Spec("slope", params=slope_params(1.0, 10.0, 10.0, 100.0)), np.float64)[0]
    np.testing.assert_allclose(s[inner], 30.0, rtol=1e-12)  # 3 up per 10 along: 30 percent
    u8, left = focal_arrays(dem, Spec("hillshade", edge="clamp", params=hillshade_params()), np.uint8)
    assert u8.dtype == np.uint8 and left.tolist() == [0] and u8.min() > 0


# ------------------------------------------------------------------------------- the command line
H, W, TILE = 40, 52, 32
TRANSFORM = (10.0, 0.0, 500000.0, 0.0, -20.0, 4100000.0)


def _dem():
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([1000 + 60 * np.sin(yy / 5.0) + 40 * np.cos(xx / 7.0) + rng.integers(0, 5, (H, W)),
                  500 + 3 * yy + 2 * xx + rng.integers(0, 9, (H, W))]).astype(np.uint16)
    a[0, 10:12, 20:23] = 0
    return a


def test_cli_writes_the_rule(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli
    from flac_raster.geo import Affine
    from flac_raster.streaming import assemble_streaming, focal_window, read_window
    from flac_raster.tiles import calculate_tiles
    from oracle_tiles import oracle_encode_tiles
    from flac_raster.tiff import read_geotiff, write_geotiff

    a = _dem()
    tif = tmp_path / "dem.tif"
    write_geotiff(tif, a, transform=TRANSFORM, crs="EPSG:32633")
    flac = tmp_path / "dem_streaming.flac"
    tiles = calculate_tiles(H, W, TILE)
    data = assemble_streaming(tiles, oracle_encode_tiles(a, tiles, level=5), a.shape, a.dtype, Affine(*TRANSFORM), "EPSG:32633", TILE)
    flac.write_bytes(data)
    decoded = read_window(data, window=(0, 0, H, W), device=None)[0]
    monkeypatch.setattr(cli, "_gpu_present", lambda: False)
    app, run = cli.app, CliRunner()
    for src, ref in ((tif, a), (flac, decoded)):
        out = tmp_path / "out.tif"
        res = run.invoke(app, ["focal", str(src), "-o", str(out), "--op", "mean", "--size", "3x7", "--nodata", "0", "--cpu"])
        assert res.exit_code == 0 and "left out" in res.output, res.output
        got, info = read_geotiff(out)
        _same(got, focal_arrays(ref, Spec("mean", (3, 7), nodata=0.0), np.float32)[0], f"mean, {src.name}")
        assert info.nodata is not None and math.isnan(info.nodata) and tuple(info.transform)[:6] == TRANSFORM
        res = run.invoke(app, ["focal", str(src), "-o", str(out), "--op", "median", "--size", "5", "--window", "8,30,20,22",
                               "--edge", "clamp", "--dtype", "uint16", "--keep-mask", "--nodata", "0", "--fill", "9", "--cpu"])
        assert res.exit_code == 0, res.output
        got, info = read_geotiff(out)
        want = focal_arrays(ref, Spec("median", 5, "clamp", 0.0, 9.0, keep_mask=True), np.uint16)[0]
        _same(got, want[:, 8:28, 30:52], f"median window, {src.name}")  # a window is the crop of the whole result
        assert info.nodata == 9 and tuple(info.transform)[:6] == (10.0, 0.0, 500300.0, 0.0, -20.0, 4099840.0)
        res = run.invoke(app, ["focal", str(src), "-o", str(out), "--kernel", "0,-1,0;-1,4,-1;0,-1,0", "--cpu"])
        assert res.exit_code == 0, res.output
        lap = Spec("convolve", weights=[[0, -1, 0], [-1, 4, -1], [0, -1, 0]])
        _same(read_geotiff(out)[0], focal_arrays(ref, lap, np.float32)[0], f"kernel, {src.name}")
        res = run.invoke(app, ["focal", str(src), "-o", str(out), "--kernel", "1,2,1", "--normalize", "--cpu"])
        assert res.exit_code == 0, res.output
        _same(read_geotiff(out)[0], focal_arrays(ref, Spec("convolve", weights=[[1, 2, 1]], normalize=True), np.float32)[0],
              f"1 x 3 kernel, {src.name}")
        res = run.invoke(app, ["hillshade", str(src), "-o", str(out), "--azimuth", "300", "--altitude", "40", "--z-factor", "2",
                               "--cpu"])
        assert res.exit_code == 0, res.output
        got, _ = read_geotiff(out)
        hs = Spec("hillshade", params=hillshade_params(300.0, 40.0, 2.0, 10.0, 20.0, 255.0))  # dx = |a|, dy = |e|
        _same(got, focal_arrays(ref, hs, np.uint8)[0], f"hillshade, {src.name}")
        assert got.dtype == np.uint8 and got[:, 1:-1, 1:-1].max() > 100
        res = run.invoke(app, ["slope", str(src), "-o", str(out), "--percent", "--scale-xy", "0.5", "--cpu"])
        assert res.exit_code == 0, res.output
        _same(read_geotiff(out)[0], focal_arrays(ref, Spec("slope", params=slope_params(1.0, 5.0, 10.0, 100.0)), np.float32)[0],
              f"slope, {src.name}")
    for args in (["focal", str(tif), "-o", str(out), "--cpu"], ["focal", str(tif), "-o", str(out), "--op", "mode", "--cpu"],
                 ["focal", str(tif), "-o", str(out), "--op", "mean", "--size", "4", "--cpu"],
                 ["focal", str(tif), "-o", str(out), "--op", "median", "--size", "7", "--cpu"],
                 ["focal", str(tif), "-o", str(out), "--op", "mean", "--kernel", "1,1,1", "--cpu"]):
        res = run.invoke(app, args)
        assert res.exit_code == 1 and "Error" in res.output, (args, res.output)
    # the streaming layer: a window of the container is the crop, whatever tiles it touches
    whole = focal_arrays(decoded, Spec("max", (5, 3), nodata=0.0), np.uint16)[0]
    for win in ((0, 0, H, W), (30, 30, 5, 5), (31, 31, 1, 1)):
        got, left, gwin, index = focal_window(data, Spec("max", (5, 3), nodata=0.0), window=win, out_dtype=np.uint16)
        _same(got, whole[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]], f"focal_window {win}")
        assert tuple(gwin) == win and left.shape == (2,)
    rot = tmp_path / "rot.tif"
    write_geotiff(rot, a, transform=(10.0, 1.0, 0.0, 1.0, -10.0, 0.0), crs="EPSG:32633")
    res = run.invoke(app, ["slope", str(rot), "-o", str(out), "--cpu"])
    assert res.exit_code == 1 and "rotation" in res.output
    res = run.invoke(app, ["focal", str(rot), "-o", str(out), "--op", "sum", "--cpu"])  # no pixel size is needed
    assert res.exit_code == 0, res.output


def test_hostcheck_covers_the_focal_refusals():
    """make hostcheck: the argument validation of the two focal entries and their spec validator in the stand-alone
    program under AddressSanitizer + UBSan; no GPU."""
    csrc = ROOT / "flac-raster_amd" / "csrc"
    if not shutil.which("make") or not (shutil.which("hipcc") or Path("/opt/rocm/bin/hipcc").exists()):
        pytest.skip("no make / hipcc")
    text = (ROOT / "tools" / "decode_host_check.cpp").read_text()
    for name in ("fra_focal_check", "fra_focal(", "fra_decode_device_focal", "fra_focal_timing"):
        assert name in text, name
    subprocess.run(["make", "-C", str(csrc), "hostcheck"], check=True, capture_output=True)
    run = subprocess.run([str(csrc / "build" / "decode_host_check"), str(ROOT / "tests" / "golden" / "sample_rgb.flac")],
                         capture_output=True, text=True)
    assert run.returncode == 0 and "argument validation checked" in run.stdout and "host check ok" in run.stdout, \
        run.stdout[-4000:] + run.stderr[-4000:]
