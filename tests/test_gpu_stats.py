"""GPU tests of the band statistics (``k_stats`` and its folds alone through ``fra_stats``, and behind the windowed read
through ``fra_decode_device_stats``).

The expectation is never the kernel: it is ``stats.stats_arrays`` -- the rule in numpy, Python integers and fractions,
checked on the CPU against a brute-force loop -- applied to the raster itself or to the host ``read_window``.  Integers
must match exactly, every field and every bin.  Floats: the counts, the extremes, ``below`` / ``above`` and every bin
exactly (the bin index is the same f64 operation sequence); ``mean == fsum / valid`` bit for bit; ``fsum`` within
``n * 2^-53 * sum |x|`` of ``math.fsum`` and ``fm2`` within ``n * 2^-53 * sum term`` of ``math.fsum`` of the terms
``(x - mean)^2`` formed with the GPU's mean: the worst case of any order of n additions.  The shapes are the smallest
at which the thread mapping can go wrong, as in ``test_gpu_compare.py``; the bin counts straddle the LDS cap.
"""
import functools
import json
import math

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.stats import exact_range, percentile, report_from_bands, stats_arrays

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
SHAPES = [(1, 1), (7, 19), (33, 67), (130, 517)]  # the last: 3 (one-byte) to 17 (f64) workgroups per band
B = 3
LDS_CAP = 8192  # kLdsBins of fra_stats.hip: the bins a launch counts in LDS; more take one launch per window of that size
BINS = [0, 1, 7, 256, LDS_CAP, LDS_CAP + 1, 65536]


def _ctx():
    return N.default_context(0)


def _same_float(x, y):
    return (x != x and y != y) or x == y


def _opt(v):
    return math.nan if v is None else v


def _raster(dt, shape, rng):
    """Full-range integers; finite floats of mixed magnitude."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        return rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
    return (rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 6, size=shape)).astype(dt)


def _padded(a, pad_cols, fill=77):
    """``a`` (B, h, w) as a view of a larger array: ``pad_cols`` spare columns per row and one spare row per band."""
    nb, h, w = a.shape
    big = np.full((nb, h + 1, w + pad_cols), fill, a.dtype)
    big[:, :h, :w] = a
    return big, big[:, :h, :w]


def _bytes(bands, hist):
    return b"".join(bytes(r) for r in bands) + (hist.tobytes() if hist is not None else b"")


class Want:
    """``stats_arrays`` of a raster and, for floats, what the sums are measured against: computed once per case."""

    def __init__(self, a, bins, rng, nodata=None):
        self.a, self.bins, self.rng, self.nodata = a, bins, rng, nodata
        self.rep = stats_arrays(a, bins, rng, nodata)
        self.valid = None
        self.terms = {}  # (band, the GPU's mean) -> math.fsum of its (x - mean)^2, None when one is infinite
        if a.dtype.kind == "f":
            self.valid = []
            for x in a.astype(np.float64):
                ok = ~np.isnan(x)
                if nodata is not None:
                    ok &= x != nodata
                v = x[ok]
                fin = bool(np.isfinite(v).all())
                self.valid.append((v, fin, math.fsum(v.tolist()) if fin else None,
                                   math.fsum(np.abs(v).tolist()) if fin else None))


def _check(got, want: Want, printed_alike=True):
    """Native reports and histogram against stats_arrays."""
    bands, hist = got
    a, rep = want.a, want.rep
    is_float = a.dtype.kind == "f"
    assert len(bands) == a.shape[0]
    assert (hist is None) == (want.bins == 0) and (hist is None or hist.shape == (a.shape[0], want.bins))
    for i, (r, w) in enumerate(zip(bands, rep)):
        assert r.count == w["count"] == a.shape[1] * a.shape[2] == r.valid + r.nan + r.nodata
        assert (r.valid, r.nan, r.nodata, r.below, r.above) == (w["valid"], w["nan"], w["nodata"], w["below"],
                                                                 w["above"]), (i, w["band"], want.bins, want.rng)
        for g, e in ((r.min, w["min"]), (r.max, w["max"]), (r.fin_min, w["fin_min"]), (r.fin_max, w["fin_max"])):
            assert _same_float(g, _opt(e)), (i, g, e)
        if want.bins:
            assert hist[i].tolist() == w["histogram"], (i, want.bins, want.rng)
            lo, hi = w["hist_range"] if w["hist_range"] is not None else (math.nan, math.nan)
            assert _same_float(r.hist_lo, lo) and _same_float(r.hist_hi, hi) and r.hist_scale == w["hist_scale"]
        else:
            assert (r.hist_lo, r.hist_hi, r.hist_scale) == (0.0, 0.0, 0.0)
        if is_float:
            assert (r.sum_lo, r.sum_hi, r.sq_lo, r.sq_hi) == (0, 0, 0, 0)
            v, fin, s, sabs = want.valid[i]
            n = v.size
            if n == 0:
                assert r.fsum == 0.0 and r.fm2 == 0.0 and math.isnan(r.mean)
                continue
            with np.errstate(all="ignore"):
                assert _same_float(r.mean, float(np.float64(r.fsum) / np.float64(n)))  # bit for bit
            if fin:
                assert abs(r.fsum - s) <= n * 2.0 ** -53 * sabs, (i, r.fsum, s)
                if (i, r.mean) not in want.terms:
                    with np.errstate(over="ignore"):
                        d = v - np.float64(r.mean)
                        terms = d * d  # the GPU's terms: only the order of the additions differs
                    want.terms[(i, r.mean)] = math.fsum(terms.tolist()) if np.isfinite(terms).all() else None
                t = want.terms[(i, r.mean)]
                if t is not None:
                    assert abs(r.fm2 - t) <= n * 2.0 ** -53 * t, (i, r.fm2, t)
                else:
                    assert r.fm2 == math.inf
            else:
                assert not math.isfinite(r.fsum) and not math.isfinite(r.fm2)
        else:
            assert (int(r.sum_hi) << 64) + int(r.sum_lo) == w["sum"] and (int(r.sq_hi) << 64 | int(r.sq_lo)) == w["sum_sq"]
            assert (r.fsum, r.mean, r.fm2) == (0.0, 0.0, 0.0)
    if not is_float and printed_alike:
        assert report_from_bands(bands, hist, a.dtype) == rep  # host and GPU paths print alike


def _ranges(a, bins):
    """The three range modes of a case: explicit with pixels below and above, automatic, unit bins."""
    dt = a.dtype
    lo, hi = np.nanpercentile(a.astype(np.float64), [20, 85])
    out = [(bins, (float(lo), float(hi))), (bins, "auto")]
    if dt.kind in "iu" and dt.itemsize <= 2:
        elo, ehi, ebins = exact_range(dt)
        out.append((ebins, (elo, ehi)))
    else:  # unit bins from the band's neighbourhood of zero
        out.append((bins, (-3.0, -3.0 + bins)))
    return out


# ------------------------------------------------------------------------------- 1. the kernel alone
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernel_alone_equals_the_numpy_rule(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(500 + dt.num)
    ctx = _ctx()
    V = 16 // dt.itemsize
    for (h, w) in SHAPES:
        a = _raster(dt, (B, h, w), rng)
        if dt.kind == "f" and h * w > 8:
            a[0, 0, 1] = a[1, h - 1, 2] = a[2, h // 2, w - 1] = np.nan
        aligned = -w % V + V
        abig5, av5 = _padded(a, 5)        # rows not 16-byte aligned: element loads
        abig16, av16 = _padded(a, aligned)  # rows 16-byte aligned: 16-byte loads
        ai = np.ascontiguousarray(a.transpose(1, 2, 0)).transpose(2, 0, 1)  # pixel-interleaved
        rs = w + (-w % V)
        sa = np.full((B, h, rs), 77, dt)
        sa[:, :, :w] = a
        d_a = ctx.alloc(sa.nbytes)
        try:
            ctx.h2d(d_a, sa)
            cases = [(0, None)]
            for bins in BINS[1:]:
                cases += _ranges(a, bins)
            for bins, r in dict.fromkeys(cases):
                want = Want(a, bins, r)
                first = ctx.stats(a, bins, r)  # contiguous
                _check(first, want)
                assert ctx.stats_timing() >= 0.0
                keep = abig5.tobytes(), abig16.tobytes()
                for view in (av5, av16, ai):
                    got = ctx.stats(view, bins, r)
                    _check(got, want, printed_alike=False)
                    assert _bytes(*ctx.stats(view, bins, r)) == _bytes(*got), "a second call returns other bytes"
                assert (abig5.tobytes(), abig16.tobytes()) == keep  # nothing is written to the source
                got = ctx.stats(d_a, bins, r, dtype=dt, shape=(B, h, w), strides=(h * rs, rs, 1))  # device-resident
                _check(got, want, printed_alike=False)
            back = np.empty_like(sa)
            ctx.d2h(back, d_a)
            assert back.tobytes() == sa.tobytes()
        finally:
            ctx.free(d_a)


# A thread's way from one of its slots to the next, 256 slots on in row-major order, at its two corners.  (3, 4113): more
# than 256 slots per row for every element size (no whole row in a step), the last slot of a row holds 1 element (1 of 2
# for f64).  (5, 511): exactly 256 slots per row for f64 (a step is one row, no slots), 128 for f32 (two rows), and a
# short last slot for every dtype.
CURSOR_SHAPES = [(3, 4113), (5, 511)]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_rows_of_more_than_and_exactly_256_slots(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(550 + dt.num)
    ctx = _ctx()
    for (h, w) in CURSOR_SHAPES:
        a = _raster(dt, (B, h, w), rng)
        if dt.kind == "f":
            a[0, 0, 1] = a[1, h - 1, 2] = a[2, h // 2, w - 1] = np.nan
        av = _padded(a, 6)[1]  # rows of an odd number of elements: element loads
        assert av.strides[1] % 16
        for bins, r in [(0, None)] + _ranges(a, 256)[:2]:  # no histogram; 256 bins over an explicit and the automatic range
            want = Want(a, bins, r)
            _check(ctx.stats(a, bins, r), want)  # contiguous
            _check(ctx.stats(av, bins, r), want, printed_alike=False)


# ------------------------------------------------------------------------------- 2. specials
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_float_specials(dt):
    ctx = _ctx()
    nan, inf = np.nan, np.inf
    h, w = 33, 67
    rng = np.random.default_rng(9)
    a = _raster(dt, (4, h, w), rng)
    a[0] = nan                      # a band of all NaN
    a[1] = -7.5                     # a band of all nodata (and, without the nodata value, a constant band)
    a[2, 3, 5], a[2, 30, 66], a[2, 0, 0] = inf, -inf, nan  # +-inf under AUTO: below / above, outside fin_min / fin_max
    a[3, 4, 4] = a[3, 20, 60] = -7.5                       # the nodata value occurs
    a[3, 5, 5], a[3, 6, 6] = -0.0, 0.0
    for bins in (0, 7, 256, LDS_CAP + 1):
        for nodata in (None, -7.5, nan, 0.0):
            want = Want(a, bins, "auto" if bins else None, nodata)
            got = ctx.stats(a, bins, "auto", nodata)
            _check(got, want)
            bands, hist = got
            assert bands[0].valid == 0 and bands[0].nan == h * w and math.isnan(bands[0].min)
            assert bands[2].min == -inf and bands[2].max == inf and math.isfinite(bands[2].fin_min)
            assert not math.isfinite(bands[2].fsum) and math.isnan(bands[2].mean)  # inf + -inf
            if bins:
                assert (bands[2].below, bands[2].above) == (1, 1) and math.isnan(bands[0].hist_lo)
                assert int(hist[0].sum()) == 0 and bands[0].hist_scale == 0.0
            if nodata == -7.5:
                assert bands[1].valid == 0 and bands[1].nodata == h * w and bands[3].nodata == 2
                assert math.isnan(bands[1].mean) and bands[1].fsum == 0.0
            elif bins:  # the constant band: lo == hi, everything in bin 0
                assert hist[1, 0] == h * w and bands[1].hist_lo == bands[1].hist_hi == -7.5 and bands[1].fm2 == 0.0
            if nodata == 0.0:
                assert bands[3].nodata == 2  # -0.0 too
    # an explicit range with the infinities and an overflowing square
    big = np.full((1, 3, 3), np.finfo(dt).max / 16, dt)  # (the sum stays finite)
    big[0, 1, 1] = -np.finfo(dt).max / 16
    want = Want(big, 4, (-1.0, 1.0))
    got = ctx.stats(big, 4, (-1.0, 1.0))
    _check(got, want)
    assert (got[0][0].below, got[0][0].above) == (1, 8)
    assert got[0][0].fm2 == inf if dt == np.float64 else math.isfinite(got[0][0].fm2)


def test_integer_specials():
    ctx = _ctx()
    # 70 x 70 of 2^32 - 1: the sum of squares carries into the high word
    a = np.full((2, 70, 70), 2**32 - 1, np.uint32)
    a[1] = 0
    for bins, r, nodata in ((0, None, None), (256, "auto", None), (256, (0.0, 2.0**32), None), (7, "auto", 0.0),
                            (LDS_CAP + 1, "auto", float(2**32 - 1))):
        got = ctx.stats(a, bins, r, nodata)
        _check(got, Want(a, bins, r, nodata))
        bands, hist = got
        if nodata is None:
            assert bands[0].sq_hi == (4900 * (2**32 - 1) ** 2) >> 64 > 0 and bands[0].sum_lo == 4900 * (2**32 - 1)
        if bins and r == "auto" and nodata is None:  # constant bands: everything in bin 0
            assert hist[0, 0] == hist[1, 0] == 4900 and bands[0].hist_scale == 0.0
        if nodata == 0.0:  # a band of nodata only
            assert bands[1].valid == 0 and bands[1].nodata == 4900 and math.isnan(bands[1].min)
            assert math.isnan(bands[1].hist_lo) and int(hist[1].sum()) == 0
    # negative sums: the high word of the 128-bit sum is signed
    for dt in (np.int32, np.int16, np.int8):
        info = np.iinfo(dt)
        lo = np.full((1, 70, 70), info.min, dt)
        lo[0, 5, 5] = info.max
        for nodata in (None, float(info.max), 0.5, float(info.max) + 1.0):  # the last two match nothing
            got = ctx.stats(lo, 16, "auto", nodata)
            _check(got, Want(lo, 16, "auto", nodata))
            assert got[0][0].sum_hi == -1 and got[0][0].nodata == (1 if nodata == float(info.max) else 0)
    # exact order statistics of a 16-bit band
    rng = np.random.default_rng(2)
    x = rng.integers(-2000, 3000, size=(1, 130, 517), dtype=np.int64).astype(np.int16)
    elo, ehi, ebins = exact_range(np.int16)
    bands, hist = ctx.stats(x, ebins, (elo, ehi))
    rep = report_from_bands(bands, hist, np.int16)
    s = sorted(x.ravel().tolist())
    for q in (2, 50, 98):
        assert percentile(rep[0], q) == s[max(1, math.ceil(q * len(s) / 100)) - 1]


# ------------------------------------------------------------------------------- 3. behind the decoder
H, W, TILE = 300, 420, 128  # 3 x 4 tiles, ragged right and bottom
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
REGIONS = {"inside one tile": (10, 140, 50, 60), "four tiles": (100, 100, 60, 51), "whole raster": (0, 0, H, W)}


def _scene(dt, bands):
    rng = np.random.default_rng(12 + bands)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(30000 + 20000 * np.sin(yy / 41.0 + b) + 8000 * np.cos(xx / 53.0) + rng.integers(0, 400, (H, W)))
                  for b in range(bands)])
    if np.dtype(dt).kind == "f":
        r = (r / 7.0).astype(dt)
        r[0, 120, 110] = np.nan
        return r
    return r.astype(dt)


@functools.lru_cache(maxsize=None)
def _container(dt, bands):
    from flac_raster.streaming import build_streaming

    src = _scene(dt, bands)
    data = build_streaming(src, TRANSFORM, "EPSG:32633", TILE)
    src.setflags(write=False)
    return data, src


@pytest.fixture(scope="module", params=[(np.uint16, 3), (np.float32, 1)], ids=["uint16x3", "float32x1"])
def scene(request):
    return _container(*request.param)


def test_regions_against_the_host_read(scene):
    from flac_raster.streaming import _tile_items, read_window

    data, src = scene
    nb, dt = src.shape[0], src.dtype
    ctx = _ctx()
    index, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    for sem, denorm in (("pcm16", N.DENORM_PCM16), ("int", N.DENORM_INT)):
        for name, win in REGIONS.items():
            r, c, h, w = win
            host = read_window(data, window=win, device=None, semantics=sem)[0]
            plain = np.zeros((nb, h, w), dt)
            want_infos = ctx.decode_device_window(blob, items, plain, dt, nb, (h * w, w, 1), win, denorm)
            nd = float(host[0, h // 2, w // 2])
            cases = [(0, None, None), (256, "auto", None), (LDS_CAP + 1, "auto", nd)]
            if dt.kind != "f":
                elo, ehi, ebins = exact_range(dt)
                cases.append((ebins, (elo, ehi), None))
            else:
                cases.append((64, (3000.0, 6000.0), None))
            for bins, rng, nodata in cases:
                bands, hist, infos = ctx.decode_device_stats(blob, items, dt, nb, win, denorm, bins, rng, nodata)
                _check((bands, hist), Want(host, bins, rng, nodata))
                for g, e in zip(infos, want_infos):
                    assert (g.nframes, g.nsamples, g.channels, g.bps, g.blocksize, g.sample_rate) == (
                        e.nframes, e.nsamples, e.channels, e.bps, e.blocksize, e.sample_rate)
                again = ctx.decode_device_stats(blob, items, dt, nb, win, denorm, bins, rng, nodata)
                assert _bytes(*again[:2]) == _bytes(bands, hist)
            t = ctx.decode_timing()
            assert len(t) == 4 and t[3] >= 0.0 and ctx.stats_timing() >= 0.0


def test_uncovered_region_is_refused_and_the_context_goes_on(scene):
    from flac_raster.streaming import _tile_items

    data, src = scene
    nb, dt = src.shape[0], src.dtype
    ctx = _ctx()
    _, items = _tile_items(data)
    blob = np.frombuffer(data, dtype=np.uint8)
    win = REGIONS["four tiles"]
    hit = [k for k, it in enumerate(items) if it["window"][0] < 160 and it["window"][0] + it["window"][2] > 100
           and it["window"][1] < 151 and it["window"][1] + it["window"][3] > 100]
    assert len(hit) == 4
    with pytest.raises(N.NativeError, match="do not cover the region"):
        ctx.decode_device_stats(blob, [it for k, it in enumerate(items) if k != hit[-1]], dt, nb, win, N.DENORM_PCM16)
    with pytest.raises(ValueError):
        ctx.decode_device_stats(blob, items, dt, nb, win, N.DENORM_PCM16, bins=70000)
    bands, hist, _ = ctx.decode_device_stats(blob, [items[k] for k in hit], dt, nb, win, N.DENORM_PCM16, 16)
    assert bands[0].count == 60 * 51 and int(hist[0].sum()) == bands[0].valid


def test_container_stats_and_stats_cli_on_the_device(tmp_path):
    from typer.testing import CliRunner

    from flac_raster.cli import app
    from flac_raster.streaming import container_stats

    data, src = _container(np.uint16, 3)
    elo, ehi, ebins = exact_range(src.dtype)
    for win in (None, REGIONS["four tiles"]):
        for kw in ({}, {"bins": 256}, {"bins": ebins, "hist_range": (elo, ehi), "nodata": float(src[0, 150, 120])}):
            host, hw, _ = container_stats(data, window=win, device=None, **kw)
            dev, dw, idx = container_stats(data, window=win, device=0, **kw)
            assert hw == dw == (win or (0, 0, H, W)) and len(idx["frames"]) == 12
            assert dev == host
    flac = tmp_path / "scene_streaming.flac"
    flac.write_bytes(data)
    out = tmp_path / "stats.json"
    res = CliRunner().invoke(app, ["stats", str(flac), "--window", "100,100,60,51", "--device", "0", "--export", str(out)])
    assert res.exit_code == 0, res.output
    rep = json.loads(out.read_text())
    host, _, _ = container_stats(data, window=REGIONS["four tiles"], device=None, bins=ebins, hist_range=(elo, ehi))
    assert rep["device"] == 0 and rep["window"] == [100, 100, 60, 51]
    for got, w in zip(rep["bands"], host):
        assert got["percentiles"] == {str(q): percentile(w, q) for q in (2, 50, 98)}
        del got["percentiles"]
        assert got == w
