"""CPU tests of the resampled reads (no GPU needed).

* the new C ABI names are declared, exported and bound; ``fra_resample`` and ``fra_decode_device_resampled`` refuse a
  null argument, a bad dtype or layout, an output size outside 1 .. 65536, an unknown code, the two overflow bounds of
  the average and items that do not cover the region before any GPU work.
* ``resample.resample`` is the rule: it equals, bit for bit, a per-pixel loop that takes every coordinate from
  ``fractions.Fraction``, integer sums as Python ints and float sums in the stated order, for 8 dtypes x 4 modes x the
  shape pairs; identity at equal size; equality with ``decimate``; the error bounds of bilinear and float average
  against exact rational values; the visible summation order; the clamp of cubic on integers.
* host ``read_window(out_shape=)`` / ``read_overview(out_shape= | max_size=)`` and the ``window --out-shape`` /
  ``overview --size`` CLI commands on the host path.
"""
import ctypes as C
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import resample as RS
from flac_raster.geo import Affine
from flac_raster.resample import decimate, resample, resampled_transform
from flac_raster.streaming import assemble_streaming, read_overview, read_window, streaming_to_raster
from flac_raster.tiff import read_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
MODES = ("nearest", "average", "bilinear", "cubic")
# (h, w) -> (oh, ow): the smallest at which the mapping can go wrong
PAIRS = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((5, 7), (3, 4)), ((5, 7), (11, 13)), ((9, 6), (9, 6)),
         ((13, 17), (2, 1)), ((2, 3), (7, 1)), ((300, 5), (2, 3)), ((3, 4100), (2, 1025)), ((3, 4100), (2, 37))]
NEW = ("fra_resample", "fra_decode_device_resampled", "fra_resample_timing")


def _same(got, want):
    """Bit-exact equality; NaNs need only be NaNs at the same places."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(np.ascontiguousarray(got).view(u)[~gn],
                                                     np.ascontiguousarray(want).view(u)[~wn])


def _raster(dt, shape, rng):
    """Full-range integers; floats with cancelling magnitudes (a wrong order shows) and, where there is room, a NaN,
    both infinities and negative zeros (a skipped or reordered special shows)."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        a = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
        a.flat[0] = info.max
        return a
    pick = rng.integers(0, 6, size=shape)
    a = np.choose(pick, [np.full(shape, 1e16), np.full(shape, -1e16), np.ones(shape), rng.normal(0.0, 3.0, size=shape),
                         np.full(shape, -0.0), rng.uniform(0.0, 1e-3, size=shape)]).astype(dt)
    if a.size >= 30:
        for v in (np.nan, np.inf, -np.inf, np.inf):
            a.flat[int(rng.integers(0, a.size))] = v
    return a


# ------------------------------------------------------------------------------- the per-pixel loop
def _axis(n_in, n_out):
    """Per output index, from exact rational coordinates: the nearest index, (i0, t), and the area taps [(i, v)]."""
    scale = Fraction(n_in, n_out)
    unit = n_out // math.gcd(n_in, n_out)  # area weights are counted in 1 / unit of a source pixel
    out = []
    for c in range(n_out):
        centre = Fraction(2 * c + 1, 2) * scale - Fraction(1, 2)
        near = min(math.floor(Fraction(2 * c + 1, 2) * scale), n_in - 1)
        i0 = math.floor(centre)
        frac = centre - i0
        t = frac.numerator / frac.denominator  # int / int: correctly rounded
        lo, hi = c * scale, (c + 1) * scale
        taps = []
        for i in range(math.floor(lo), math.ceil(hi)):
            v = (min(Fraction(i + 1), hi) - max(Fraction(i), lo)) * unit
            assert v.denominator == 1 and v > 0
            taps.append((i, int(v)))
        assert sum(v for _, v in taps) == n_in // math.gcd(n_in, n_out)
        out.append((near, i0, t, taps))
    return out


def _weights(t, mode):
    if mode == "bilinear":
        return 0, [1.0 - t, t]
    return -1, [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
                ((0.5 * t - 0.5) * t) * t]


def _to_dtype(v, dt):
    if dt.kind == "f":
        with np.errstate(over="ignore"):
            return dt.type(v)
    info = np.iinfo(dt)
    return dt.type(min(max(round(v), info.min), info.max))  # round(): half to even


def _loop(x, out_shape, mode):
    """The rule one pixel at a time over a (h, w) raster."""
    h, w = x.shape
    oh, ow = out_shape
    dt = x.dtype
    if (oh, ow) == (h, w):
        return x.copy()
    ys, xs = _axis(h, oh), _axis(w, ow)
    n = (h // math.gcd(h, oh)) * (w // math.gcd(w, ow))
    out = np.zeros((oh, ow), dt)
    item = (lambda j, i: float(x[j, i])) if dt.kind == "f" or mode in ("bilinear", "cubic") else (lambda j, i: int(x[j, i]))
    for R, (ny, i0y, ty, tapsy) in enumerate(ys):
        for Cc, (nx, i0x, tx, tapsx) in enumerate(xs):
            if mode == "nearest":
                out[R, Cc] = x[ny, nx]
            elif mode == "average":
                if dt.kind == "f":
                    acc = None
                    for i, vx in tapsx:
                        c = None
                        for j, vy in tapsy:
                            p = float(vy) * item(j, i)
                            c = p if c is None else c + p
                        p = float(vx) * c
                        acc = p if acc is None else acc + p
                    out[R, Cc] = _to_dtype(acc / float(n), dt)
                else:
                    S = sum(vy * vx * item(j, i) for j, vy in tapsy for i, vx in tapsx)
                    out[R, Cc] = dt.type(round(float(S) / float(n)))
            else:
                off, wy = _weights(ty, mode)
                _, wx = _weights(tx, mode)
                v = None
                for k, wxi in enumerate(wx):
                    i = min(max(i0x + off + k, 0), w - 1)
                    c = None
                    for m, wyj in enumerate(wy):
                        p = item(min(max(i0y + off + m, 0), h - 1), i) * wyj
                        c = p if c is None else c + p
                    p = c * wxi
                    v = p if v is None else v + p
                out[R, Cc] = _to_dtype(v, dt)
    return out


# ------------------------------------------------------------------------------- 1. names and refusals
def test_new_names_exported_declared_and_bound():
    hdr = (ROOT / "include" / "flac_raster_amd.h").read_text()
    decl = set(re.findall(r"FRA_API\s+[^;(]*?\b(fra_\w+)\s*\(", hdr))
    L = N.load()
    for name in NEW:
        assert name in decl and name in N.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+FRA_RESAMPLE_BILINEAR\s+2\b", hdr) and re.search(r"#define\s+FRA_RESAMPLE_CUBIC\s+3\b", hdr)
    assert "fra_resample_job" in hdr and (N.RESAMPLE_BILINEAR, N.RESAMPLE_CUBIC) == (2, 3)
    assert RS.RESAMPLING_ANY == {"nearest": 0, "average": 1, "bilinear": 2, "cubic": 3}
    assert RS.RESAMPLING == {"nearest": 0, "average": 1}  # the decimate path keeps its two
    for name in ("resample", "decode_device_resampled", "resample_timing"):
        assert hasattr(N.Context, name)
    import inspect

    from flac_raster import streaming, tiles

    for fn in (streaming.read_window, streaming.window_to_tiff, tiles.read_window_on_device, streaming.read_overview):
        assert inspect.signature(fn).parameters["out_shape"].default is None, fn
    assert inspect.signature(streaming.read_overview).parameters["max_size"].default is None


def _resample_job():
    src = (C.c_int32 * 64)()
    dst = (C.c_int32 * 64)()
    job = N.ResampleJob()
    job.src, job.dst, job.dtype = C.cast(src, C.c_void_p), C.cast(dst, C.c_void_p), N.DTYPE_CODES[np.dtype(np.int32)]
    job.channels, job.height, job.width = 1, 8, 8
    job.src_band_stride, job.src_row_stride, job.src_col_stride = 64, 8, 1
    job.dst_band_stride, job.dst_row_stride, job.dst_col_stride = 15, 5, 1
    job.out_height, job.out_width, job.resampling = 3, 5, 1
    return job, (src, dst)


def test_resample_entry_refuses_before_any_gpu_work():
    """Every call returns FRA_E_INVALID before the context is looked at, so a stand-in pointer serves."""
    L = N.load()
    ctx = C.c_void_p(16)
    job, (src, dst) = _resample_job()

    def refused(word):
        return L.fra_resample(ctx, C.byref(job)) == -1 and word in L.fra_last_error()

    assert L.fra_resample(None, C.byref(job)) == -1 and b"null" in L.fra_last_error()
    assert L.fra_resample(ctx, None) == -1 and b"null" in L.fra_last_error()
    job.src = None
    assert refused(b"null")
    job.src, job.dst = C.cast(src, C.c_void_p), None
    assert refused(b"null")
    job.dst = C.cast(dst, C.c_void_p)
    for oh, ow in ((0, 5), (3, 0), (-1, 5), (65537, 5), (3, 65537)):
        job.out_height, job.out_width = oh, ow
        assert refused(b"output size"), (oh, ow)
    job.out_height, job.out_width = 3, 5
    for mode in (4, -1):
        job.resampling = mode
        assert refused(b"resampling")
    job.resampling, job.dtype = 1, 8
    assert refused(b"dtype")
    job.dtype, job.width = 5, 0
    assert refused(b"layout")
    job.width, job.src_row_stride = 8, -1
    assert refused(b"layout")
    job.src_row_stride = 8
    # the overflow bounds of the average: n = h' w' with n 2^(8 itemsize) > 2^63 (integers), n > 2^53 (floats)
    job.height, job.width, job.out_height, job.out_width = 65537, 65537, 1, 1  # n = 2^32 + 2^17 + 1 > 2^31
    assert refused(b"average")
    for dt, hw in ((np.uint8, (2**28 + 1, 2**27 + 1)), (np.float64, (2**27 + 1, 2**26 + 1)),
                   (np.float32, (2**27 + 1, 2**26 + 1))):  # odd sizes to (2, 2): nothing to reduce
        job.dtype, (job.height, job.width) = N.DTYPE_CODES[np.dtype(dt)], hw
        job.out_height, job.out_width = 2, 2
        assert refused(b"average"), dt
    assert L.fra_resample_timing(None) == -1
    # the same bounds in Python, before anything is touched (a broadcast view holds no memory)
    with pytest.raises(ValueError, match="average"):
        resample(np.broadcast_to(np.zeros(1, np.int32), (1, 65537, 65537)), (1, 1), "average")
    assert RS.check_average_size(65536, 32768, 1, 1, np.int32) == 2**31
    assert RS.check_average_size(65536, 32768, 1, 1, np.uint32) == 2**31
    with pytest.raises(ValueError):
        RS.check_average_size(65536, 32769, 1, 1, np.int32)
    assert RS.check_average_size(2**28, 2**27, 1, 1, np.uint8) == 2**55
    with pytest.raises(ValueError):
        RS.check_average_size(2**28 + 1, 2**27, 1, 1, np.int8)
    assert RS.check_average_size(2**27, 2**26, 1, 1, np.float32) == 2**53
    with pytest.raises(ValueError):
        RS.check_average_size(2**27 + 1, 2**26, 1, 1, np.float64)
    assert RS.check_average_size(2**30, 2**30, 2**15, 2**15, np.int32) == 2**30  # n is of the reduced sizes
    for bad in ((0, 4), (4, 65537), (2.5, 4), (4,), None):
        with pytest.raises(ValueError):
            resample(np.zeros((2, 2), np.uint8), bad)
    with pytest.raises(ValueError):
        resample(np.zeros((2, 2), np.uint8), (3, 3), "lanczos")
    with pytest.raises(TypeError):
        resample(np.zeros((2, 2), np.int64), (3, 3))


def test_resampled_decode_refuses_before_any_gpu_work():
    L = N.load()
    ctx = C.c_void_p(16)
    data = (C.c_uint8 * 64)()
    dst = (C.c_int32 * 64)()
    item = N.DecodeItem()
    item.offset, item.bytes, item.window = 0, 64, N.Window(0, 0, 4, 8)
    job = N.DecodeJob()
    job.data, job.len, job.items, job.nitems = C.cast(data, C.c_void_p), 64, C.pointer(item), 1
    job.dst, job.dst_dtype, job.channels = C.cast(dst, C.c_void_p), N.DTYPE_CODES[np.dtype(np.int32)], 1
    job.band_stride, job.row_stride, job.col_stride = 15, 5, 1
    infos = (N.Decoded * 1)()
    roi = N.Window(0, 0, 4, 8)

    def call(ctx=ctx, job=job, roi=roi, oh=3, ow=5, mode=1, infos=infos):
        return L.fra_decode_device_resampled(ctx, C.byref(job) if job is not None else None,
                                             C.byref(roi) if roi is not None else None, oh, ow, mode, infos)

    for kw in ({"ctx": None}, {"job": None}, {"roi": None}, {"infos": None}):
        assert call(**kw) == -1 and b"null" in L.fra_last_error(), kw
    for oh, ow in ((0, 5), (3, 65537), (-3, 5)):
        assert call(oh=oh, ow=ow) == -1 and b"output size" in L.fra_last_error()
    for mode in (4, -1):
        assert call(mode=mode) == -1 and b"resampling" in L.fra_last_error()
    assert call(roi=N.Window(0, 0, 5, 8)) == -1 and b"do not cover the region" in L.fra_last_error()
    item.window = N.Window(0, 0, 4, 7)
    for mode in range(4):  # (nearest would not read the missing column, but every pixel must be covered)
        assert call(mode=mode) == -1 and b"do not cover the region" in L.fra_last_error()
    item.window = N.Window(0, 0, 4, 8)
    # what the windowed read refuses is refused in its words
    assert call(roi=N.Window(0, 0, 0, 8)) == -1 and b"region of interest" in L.fra_last_error()
    job.flags = N.DECODE_CONCAT
    assert call() == -1 and b"CONCAT" in L.fra_last_error()
    job.flags = 0
    # the decimate entries still know two codes only
    assert L.fra_decode_device_decimated(ctx, C.byref(job), C.byref(roi), 2, 2, infos) == -1
    assert b"resampling" in L.fra_last_error()


# ------------------------------------------------------------------------------- 2. the numpy rule
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_numpy_rule_equals_the_per_pixel_loop(dt, mode):
    dt = np.dtype(dt)
    rng = np.random.default_rng(7 + dt.num)
    for (h, w), out_shape in PAIRS:
        a = _raster(dt, (2, h, w), rng)
        got = resample(a, out_shape, mode)
        assert got.shape == (2,) + out_shape and got.dtype == dt and got.flags.c_contiguous
        assert _same(got[1], _loop(a[1], out_shape, mode)), (h, w, out_shape)
        assert _same(resample(a[0], out_shape, mode), got[0])  # the (h, w) form


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_identity_and_equality_with_decimate(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(40 + dt.num)
    a = _raster(dt, (2, 9, 6), rng)
    for mode in MODES:  # the input itself, specials included (a zero weight beside an infinity would give a NaN)
        assert _same(resample(a, (9, 6), mode), a), mode
    for k in (2, 4):
        for h, w in ((k, k), (3 * k, 5 * k), (8 * k, 2 * k)):
            a = _raster(dt, (2, h, w), rng)
            assert _same(resample(a, (h // k, w // k), "nearest"), decimate(a, k, "nearest")), (k, h, w)
            if dt.kind != "f":
                assert _same(resample(a, (h // k, w // k), "average"), decimate(a, k, "average")), (k, h, w)


def _exact(x, out_shape, mode):
    """The value of every output pixel in exact rational arithmetic (bilinear with exact weights, or the area
    average), and the largest |tap| of each."""
    h, w = x.shape
    ys, xs = _axis(h, out_shape[0]), _axis(w, out_shape[1])
    n = (h // math.gcd(h, out_shape[0])) * (w // math.gcd(w, out_shape[1]))
    val = np.empty(out_shape, object)
    big = np.empty(out_shape, object)
    for R, (_, i0y, _, tapsy) in enumerate(ys):
        for Cc, (_, i0x, _, tapsx) in enumerate(xs):
            if mode == "bilinear":
                fy = Fraction(2 * R + 1, 2) * Fraction(h, out_shape[0]) - Fraction(1, 2) - i0y
                fx = Fraction(2 * Cc + 1, 2) * Fraction(w, out_shape[1]) - Fraction(1, 2) - i0x
                ty_ = [(min(max(i0y + m, 0), h - 1), wt) for m, wt in enumerate((1 - fy, fy))]
                tx_ = [(min(max(i0x + m, 0), w - 1), wt) for m, wt in enumerate((1 - fx, fx))]
                scale = 1
            else:
                ty_, tx_, scale = tapsy, tapsx, n
            val[R, Cc] = sum(wy * wx * Fraction(float(x[j, i])) for j, wy in ty_ for i, wx in tx_) / scale
            big[R, Cc] = max(abs(Fraction(float(x[j, i]))) for j, _ in ty_ for i, _ in tx_)
    return val, big


def test_bilinear_and_float_average_are_within_their_bounds():
    """Both use non-negative weights.  Bilinear: two taps per axis, within 8 * 2^-53 * max|tap| of the exact value.
    Average on positive data: every term is positive, so each of the roundings on an output's longest path (one per
    product and one per addition of the vertical sum over my taps: my; the same horizontally: mx; the division: 1)
    changes the partial result by a relative 2^-53 at most, k = my + mx + 1 roundings in all, and the result lies
    within gamma_k = k u / (1 - k u), u = 2^-53, of the exact weighted mean."""
    rng = np.random.default_rng(3)
    u = 2.0 ** -53
    for (h, w), out_shape in PAIRS[:8]:
        x = rng.uniform(-1000.0, 1000.0, size=(h, w))
        got = resample(x, out_shape, "bilinear")
        if (h, w) != out_shape:
            val, big = _exact(x, out_shape, "bilinear")
            for idx in np.ndindex(*out_shape):
                assert abs(Fraction(float(got[idx])) - val[idx]) <= 8 * Fraction(u) * big[idx], (h, w, out_shape, idx)
        x = rng.uniform(0.5, 1000.0, size=(h, w))
        got = resample(x, out_shape, "average")
        if (h, w) != out_shape:
            val, _ = _exact(x, out_shape, "average")
            my = max(len(t[3]) for t in _axis(h, out_shape[0]))
            mx = max(len(t[3]) for t in _axis(w, out_shape[1]))
            k = my + mx + 1
            gamma = Fraction(k) * Fraction(u) / (1 - Fraction(k) * Fraction(u))
            for idx in np.ndindex(*out_shape):
                assert abs(Fraction(float(got[idx])) - val[idx]) <= gamma * val[idx], (h, w, out_shape, idx)


def test_order_is_visible_and_cubic_clamps():
    col = np.array([[1e16], [1.0], [-1e16], [1.0]])
    assert ((1e16 + 1.0) + -1e16) + 1.0 == 1.0 and (1e16 + 1.0) + (-1e16 + 1.0) == 0.0
    assert resample(col, (1, 1), "average")[0, 0] == 0.25  # top to bottom; a pairwise tree would give 0.0
    assert resample(col.T.copy(), (1, 1), "average")[0, 0] == 0.25  # and left to right
    # vertically first: the column sums (1e16 + -1e16 = 0, 1 + 1 = 2) and then 0 + 2; horizontally first would be
    # (1e16 + 1 = 1e16, -1e16 + 1 = -1e16) and then 0
    sq = np.array([[1e16, 1.0], [-1e16, 1.0]])
    assert resample(sq, (1, 1), "average")[0, 0] == 0.5
    # plain IEEE: NaN and infinities propagate, -0.0 survives
    a = np.ones((2, 4), np.float32)
    a[0, 1], a[1, 2] = np.nan, np.inf
    got = resample(a, (1, 2), "average")
    assert np.isnan(got[0, 0]) and got[0, 1] == np.inf
    assert np.signbit(resample(np.full((2, 2), -0.0), (1, 1), "average")[0, 0])
    ties = np.array([[1, 2, 3, 4, 0, 1], [1, 2, 4, 3, 1, 0]], np.int16)  # 1.5, 3.5, 0.5: half to even
    assert np.array_equal(resample(ties, (1, 3), "average"), [[2, 4, 0]])
    # cubic overshoots and is clamped on integers
    step = np.array([[0, 0, 255, 255, 0, 0]], np.uint8)
    up = resample(step, (1, 24), "cubic")
    exact = resample(step.astype(np.float64), (1, 24), "cubic")
    assert up.dtype == np.uint8 and exact.max() > 255.0 and exact.min() < 0.0
    assert np.array_equal(up, np.clip(np.rint(exact), 0, 255).astype(np.uint8))
    assert up.max() == 255 and up.min() == 0
    lo = resample(np.array([[-128, -128, 127, 127, -128, -128]], np.int8), (1, 24), "cubic")
    assert lo.min() == -128 and lo.max() == 127
    bil = resample(step, (1, 24), "bilinear")  # bilinear cannot overshoot
    assert np.array_equal(bil, np.rint(resample(step.astype(np.float64), (1, 24), "bilinear")).astype(np.uint8))


def test_transform_and_max_size():
    t = (10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
    assert resampled_transform(t, (100, 230, 60, 50), (15, 25)) == (20.0, 0.0, 502300.0, 0.0, -40.0, 4099000.0)
    for k in (2, 8):  # at sx = sy = k: decimated_transform
        assert resampled_transform(t, (100, 230, 64, 48), (64 // k, 48 // k)) == RS.decimated_transform(t, (100, 230), k)
    r = (2.0, 0.5, 7.0, -0.25, -3.0, 11.0)  # rotation terms scale and shift too; upsampling shrinks the pixel
    assert resampled_transform(r, (3, 5, 10, 20), (40, 40)) == (1.0, 0.125, 7.0 + 5 * 2.0 + 3 * 0.5, -0.125, -0.75,
                                                                11.0 + 5 * -0.25 + 3 * -3.0)
    with pytest.raises(ValueError):
        resampled_transform(t, (0, 0, 4, 4), (0, 4))
    assert RS.max_size_shape(300, 420, 100) == (71, 100) and RS.max_size_shape(420, 300, 100) == (100, 71)
    assert RS.max_size_shape(5, 5, 64) == (64, 64) and RS.max_size_shape(1, 5000, 10) == (1, 10)
    assert RS.max_size_shape(10980, 10980, 1024) == (1024, 1024)
    for bad in (0, 65537, 2.5):
        with pytest.raises(ValueError):
            RS.max_size_shape(10, 10, bad)


# ------------------------------------------------------------------------------- 3. the container on the host
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TILE = 150, 210, 64  # 3 x 4 tiles, ragged right and bottom


@pytest.fixture(scope="module")
def container():
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (1000 + 60 * np.sin(yy / 23.0) + 40 * np.cos(xx / 31.0)).astype(np.int64)
    r = np.stack([base + b * 7 + rng.integers(0, 50, size=(H, W)) for b in range(3)]).astype(np.uint16)
    tiles = calculate_tiles(H, W, TILE)
    streams = oracle_encode_tiles(r, tiles, level=5)
    data = assemble_streaming(tiles, streams, r.shape, r.dtype, TRANSFORM, "EPSG:32633", TILE)
    full = streaming_to_raster(data, device=None)[0]
    full.setflags(write=False)
    return data, full


def test_host_reads_resampled(container):
    data, full = container
    for asked, (r, c, h, w) in (((10, 70, 50, 60), (10, 70, 50, 60)), ((120, 190, 100, 100), (120, 190, 30, 20))):
        for mode in MODES:
            for out_shape in ((37, 53), (7, 5)):
                got, win, index = read_window(data, window=asked, device=None, out_shape=out_shape, resampling=mode)
                assert tuple(win) == (r, c, h, w) and index["height"] == H and got.dtype == np.uint16
                assert np.array_equal(got, resample(full[:, r:r + h, c:c + w], out_shape, mode)), (asked, mode)
    got, index = read_overview(data, out_shape=(40, 30), resampling="cubic")
    assert index["width"] == W and np.array_equal(got, resample(full, (40, 30), "cubic"))
    got, _ = read_overview(data, max_size=64)  # average by default
    assert got.shape == (3, 46, 64) and np.array_equal(got, resample(full, (46, 64), "average"))
    assert np.array_equal(read_overview(data, 2)[0], decimate(full, 2, "average"))  # as before
    with pytest.raises(ValueError, match="not both"):
        read_window(data, window=(0, 0, 8, 8), decimate=2, out_shape=(4, 4))
    with pytest.raises(ValueError):
        read_window(data, window=(0, 0, 8, 8), out_shape=(4, 4), resampling="lanczos")
    with pytest.raises(ValueError):
        read_window(data, window=(0, 0, 8, 8), out_shape=(0, 4))
    with pytest.raises(ValueError):
        read_window(data, window=(0, 0, 8, 8), decimate=2, resampling="cubic")  # the decimate path keeps its two
    for kw in ({}, {"factor": 2, "max_size": 8}, {"out_shape": (4, 4), "max_size": 8}):
        with pytest.raises(ValueError):
            read_overview(data, **kw)


def test_cli_on_the_host(container, tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli

    data, full = container
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    monkeypatch.setattr(cli, "_gpu_present", lambda: False)  # the host path, wherever this runs
    out = tmp_path / "win.tif"
    res = CliRunner().invoke(cli.app, ["window", str(src), "-o", str(out), "--window", "10,70,50,60", "--out-shape",
                                       "25,40", "--resampling", "bilinear"])
    assert res.exit_code == 0, res.output
    px, info = read_geotiff(out)
    assert px.shape == (3, 25, 40) and np.array_equal(px, resample(full[:, 10:60, 70:130], (25, 40), "bilinear"))
    assert tuple(info.transform)[:6] == (15.0, 0.0, 500700.0, 0.0, -20.0, 4099900.0) and "32633" in str(info.crs)
    out2 = tmp_path / "preview.tif"
    res = CliRunner().invoke(cli.app, ["overview", str(src), "-o", str(out2), "--size", "70"])
    assert res.exit_code == 0, res.output
    px2, info2 = read_geotiff(out2)
    assert px2.shape == (3, 50, 70) and np.array_equal(px2, resample(full, (50, 70), "average"))
    assert tuple(info2.transform)[:6] == (30.0, 0.0, 500000.0, 0.0, -30.0, 4100000.0)
    run = lambda *a: CliRunner().invoke(cli.app, list(a)).exit_code  # noqa: E731
    assert run("window", str(src), "-o", str(tmp_path / "x.tif"), "--window", "0,0,8,8", "--out-shape", "4,4",
               "--decimate", "2") == 1
    assert run("window", str(src), "-o", str(tmp_path / "x.tif"), "--window", "0,0,8,8", "--out-shape", "4,4",
               "--resampling", "lanczos") == 1
    assert run("overview", str(src), "-o", str(tmp_path / "x.tif"), "--size", "8", "--factor", "2") == 1
    assert run("overview", str(src), "-o", str(tmp_path / "x.tif")) == 1
