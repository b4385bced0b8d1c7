"""The nodata-aware rule of ``flac_raster.resample`` (``resample(..., nodata=)``, ``decimate(..., nodata=)``) on the CPU.

The expectation is a per-pixel loop that follows the rule's text: Python integers and ``Fraction`` for the coordinates
and for the exact integer sums and weights, Python floats, in the stated order, for the float operations.  Every
comparison is bit-exact (floats: the same NaN positions and the same bits elsewhere).
"""
from fractions import Fraction
from math import floor, gcd, isnan

import numpy as np
import pytest

from flac_raster.resample import FACTORS, check_nodata, decimate, resample

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
IDS = [np.dtype(d).name for d in DTYPES]
PAIRS = [((1, 1), (3, 2)), ((5, 7), (3, 4)), ((5, 7), (11, 13)), ((13, 17), (2, 1)), ((2, 3), (7, 1)), ((6, 9), (4, 5))]


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    u = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(np.ascontiguousarray(got).view(u)[~gn],
                                                     np.ascontiguousarray(want).view(u)[~wn])


def _nodata_of(dt):
    dt = np.dtype(dt)
    return -9999.0 if dt.kind == "f" else float({1: 7, 2: 1000, 4: 100000}[dt.itemsize])


def _raster(dt, shape, rng, nd, share=0.3, specials=True):
    """Full-range integers / floats with cancelling magnitudes, ``share`` of the pixels set to ``nd``; floats hold NaN,
    both infinities and negative zeros as well where there is room."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        info = np.iinfo(dt)
        a = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dt)
        a[a == dt.type(int(nd))] = dt.type(int(nd) + 1)
    else:
        pick = rng.integers(0, 6, size=shape)
        a = np.choose(pick, [np.full(shape, 1e16), np.full(shape, -1e16), np.ones(shape), rng.normal(0.0, 3.0, size=shape),
                             np.full(shape, -0.0), rng.uniform(0.0, 1e-3, size=shape)]).astype(dt)
        if specials and a.size >= 30:
            for v in (np.nan, np.inf, -np.inf, np.inf):
                a.flat[int(rng.integers(0, a.size))] = v
    if share:
        a[rng.random(shape) < share] = dt.type(nd) if dt.kind == "f" else dt.type(int(nd))
    return a


# ------------------------------------------------------------------------------- the rule, pixel by pixel
def _is_invalid(x, nd):
    return x == nd or (isinstance(x, float) and isnan(x))


def _area_taps(n_in, n_out):
    g = gcd(n_in, n_out)
    ni, no = n_in // g, n_out // g
    taps = []
    for C in range(n_out):
        lo, hi = C * ni, (C + 1) * ni
        taps.append([(i, min((i + 1) * no, hi) - max(i * no, lo)) for i in range(lo // no, -(-hi // no))])
    return taps


def _block_taps(n, k):
    return [[(i, 1) for i in range(C * k, min(C * k + k, n))] for C in range(-(-n // k))]


def _brute_average(a, taps_y, taps_x, nd):
    dt = a.dtype
    is_float = dt.kind == "f"
    px = a.astype(np.float64).tolist() if is_float else a.astype(np.int64).tolist()
    fill = dt.type(nd) if is_float else dt.type(int(nd))
    out = np.empty((len(taps_y), len(taps_x)), dt)
    for R, ty in enumerate(taps_y):
        for C, tx in enumerate(taps_x):
            S, W = None, 0
            for i, vx in tx:
                c, u = None, 0
                for j, vy in ty:
                    x = px[j][i]
                    if _is_invalid(x, nd):
                        continue
                    term = float(vy) * x if is_float else vy * x
                    c = term if c is None else c + term
                    u += vy
                if u == 0:
                    continue
                term = float(vx) * c if is_float else vx * c
                S = term if S is None else S + term
                W += vx * u
            if W == 0:
                out[R, C] = fill
            elif is_float:
                with np.errstate(over="ignore"):
                    out[R, C] = dt.type(S / float(W))
            else:
                out[R, C] = round(float(S) / float(W))  # half to even
    return out


def _centre(C, n_in, n_out):
    g = gcd(n_in, n_out)
    ni, no = n_in // g, n_out // g
    num, den = (2 * C + 1) * ni - no, 2 * no
    i0 = floor(Fraction(num, den))
    return i0, float(num - i0 * den) / float(den)


def _weights(t, mode):
    if mode == "bilinear":
        return [1.0 - t, t]
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
            ((0.5 * t - 0.5) * t) * t]


def _to_dtype(q, dt):
    if dt.kind == "f":
        with np.errstate(over="ignore"):
            return dt.type(q)
    info = np.iinfo(dt)
    return dt.type(min(max(round(q), info.min), info.max))


def _brute_taps(a, oh, ow, mode, nd):
    dt = a.dtype
    h, w = a.shape
    px = a.astype(np.float64).tolist()
    fill = dt.type(nd) if dt.kind == "f" else dt.type(int(nd))
    off, nt = (0, 2) if mode == "bilinear" else (-1, 4)
    out = np.empty((oh, ow), dt)
    for R in range(oh):
        i0y, ty = _centre(R, h, oh)
        for C in range(ow):
            i0x, tx = _centre(C, w, ow)
            rows = [min(max(i0y + off + k, 0), h - 1) for k in range(nt)]
            cols = [min(max(i0x + off + k, 0), w - 1) for k in range(nt)]
            if not any(_is_invalid(px[j][i], nd) for j in rows for i in cols):
                wy, wx = _weights(ty, mode), _weights(tx, mode)
                v = None
                for k, i in enumerate(cols):
                    c = None
                    for m, j in enumerate(rows):
                        term = px[j][i] * wy[m]
                        c = term if c is None else c + term
                    v = c * wx[k] if v is None else v + c * wx[k]
                out[R, C] = _to_dtype(v, dt)
                continue
            wy, wx = [1.0 - ty, ty], [1.0 - tx, tx]
            v = wt = None
            for k in range(2):
                i = min(max(i0x + k, 0), w - 1)
                c = u = None
                for m in range(2):
                    x = px[min(max(i0y + m, 0), h - 1)][i]
                    if _is_invalid(x, nd):
                        continue
                    c = x * wy[m] if c is None else c + x * wy[m]
                    u = wy[m] if u is None else u + wy[m]
                if c is None:
                    continue
                v = c * wx[k] if v is None else v + c * wx[k]
                wt = u * wx[k] if wt is None else wt + u * wx[k]
            out[R, C] = fill if v is None or wt <= 0.0 else _to_dtype(v / wt, dt)
    return out


@pytest.mark.parametrize("mode", ("average", "bilinear", "cubic"))
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_rule_equals_the_pixel_loop(dt, mode):
    dt = np.dtype(dt)
    rng = np.random.default_rng(500 + dt.num)
    nd = _nodata_of(dt)
    seen_fill = seen_partial = False
    for (h, w), (oh, ow) in PAIRS:
        a = _raster(dt, (2, h, w), rng, nd)
        got = resample(a, (oh, ow), mode, nodata=nd)
        assert got.shape == (2, oh, ow) and got.dtype == dt
        for b in range(2):
            if mode == "average":
                want = _brute_average(a[b], _area_taps(h, oh), _area_taps(w, ow), nd)
            else:
                want = _brute_taps(a[b], oh, ow, mode, nd)
            assert _same(got[b], want), (h, w, oh, ow, b)
        seen_fill |= bool((got == dt.type(nd)).any())
        seen_partial |= not _same(got, resample(a, (oh, ow), mode))
    assert seen_fill and seen_partial  # the data made the rule fill some outputs and renormalise others


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_decimate_equals_the_pixel_loop(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(600 + dt.num)
    nd = _nodata_of(dt)
    for k in FACTORS:
        for h, w in ((13, 17), (70, 67)):
            a = _raster(dt, (h, w), rng, nd)
            assert _same(decimate(a, k, "average", nodata=nd), _brute_average(a, _block_taps(h, k), _block_taps(w, k), nd)), (k, h, w)
            assert _same(decimate(a, k, "nearest", nodata=nd), decimate(a, k, "nearest"))


# ------------------------------------------------------------------------------- the rule's consequences
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_identities(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(700 + dt.num)
    nd = _nodata_of(dt)
    # no invalid pixel: the unmasked resampling in every mode and dtype (floats: -0.0 and both infinities included;
    # a NaN would be invalid)
    for (h, w), out_shape in PAIRS:
        a = _raster(dt, (2, h, w), rng, nd, share=0.0)
        if dt.kind == "f":
            a[np.isnan(a)] = -0.0
        for mode in ("nearest", "average", "bilinear", "cubic"):
            assert _same(resample(a, out_shape, mode, nodata=nd), resample(a, out_shape, mode)), (h, w, out_shape, mode)
    z = np.full((1, 4, 4), -0.0, dt) if dt.kind == "f" else None
    if z is not None:
        assert np.signbit(resample(z, (2, 2), "average", nodata=nd)).all()
        assert np.signbit(decimate(z, 2, "average", nodata=nd)).all()
    for k in FACTORS:
        # k divides h and w: the decimation is the resampling to (h / k, w / k), invalid pixels or not
        a = _raster(dt, (2, 2 * k, 3 * k), rng, nd)
        assert _same(decimate(a, k, "average", nodata=nd), resample(a, (2, 3), "average", nodata=nd)), k
        # no invalid pixel: the unmasked decimation, for integers (the float tree sums in another order)
        if dt.kind != "f":
            c = _raster(dt, (2, 2 * k + 3, 3 * k + 1), rng, nd, share=0.0)
            assert _same(decimate(c, k, "average", nodata=nd), decimate(c, k, "average")), k
    # nearest picks its pixel, invalid or not; the identity size returns the input
    a = _raster(dt, (2, 9, 6), rng, nd)
    assert _same(resample(a, (4, 5), "nearest", nodata=nd), resample(a, (4, 5), "nearest"))
    for mode in ("nearest", "average", "bilinear", "cubic"):
        assert _same(resample(a, (9, 6), mode, nodata=nd), a)


def test_float_decimation_order_is_the_rule_not_the_tree():
    row = np.array([[1e16, 1.0, -1e16, 1.0]])
    assert decimate(row, 4, "average")[0, 0] == 0.0  # (1e16 + 1) + (-1e16 + 1) in the tree
    assert decimate(row, 4, "average", nodata=-9999.0)[0, 0] == 0.25  # left to right


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_all_invalid_one_valid_and_nan(dt):
    dt = np.dtype(dt)
    nd = _nodata_of(dt)
    fill = dt.type(nd) if dt.kind == "f" else dt.type(int(nd))
    a = np.full((1, 8, 12), fill, dt)
    for mode in ("average", "bilinear", "cubic"):
        for out_shape in ((2, 3), (3, 5), (11, 17)):
            assert _same(resample(a, out_shape, mode, nodata=nd), np.full((1,) + out_shape, fill, dt)), (mode, out_shape)
    assert _same(decimate(a, 4, "average", nodata=nd), np.full((1, 2, 3), fill, dt))
    # one valid pixel in a block gives that pixel
    a[0, 5, 2] = dt.type(42)
    want = np.full((1, 2, 3), fill, dt)
    want[0, 1, 0] = dt.type(42)
    assert _same(decimate(a, 4, "average", nodata=nd), want)
    assert _same(resample(a, (2, 3), "average", nodata=nd), want)
    got = resample(a, (4, 6), "bilinear", nodata=nd)  # an output with the pixel as its only valid tap gives it back
    assert set(np.unique(got).tolist()) == {fill.item(), 42}
    if dt.kind == "f":
        # a NaN pixel is skipped whatever nd is; nd = NaN works
        b = np.array([[[1.0, np.nan], [3.0, nd]]], dt)
        assert resample(b, (1, 1), "average", nodata=nd)[0, 0, 0] == 2.0
        assert resample(b, (1, 1), "bilinear", nodata=nd)[0, 0, 0] == 2.0
        b[0, 1, 1] = 5.0
        assert resample(b, (1, 1), "average", nodata=np.nan)[0, 0, 0] == 3.0
        assert decimate(b, 2, "average", nodata=np.nan)[0, 0, 0] == 3.0
        allnan = np.full((1, 4, 4), np.nan, dt)
        assert np.isnan(resample(allnan, (2, 2), "average", nodata=np.nan)).all()
        assert (resample(allnan, (2, 2), "cubic", nodata=nd) == fill).all()
        inf = np.array([[[np.inf, nd], [1.0, 1.0]]], dt)  # +-inf are valid and propagate
        assert resample(inf, (1, 1), "average", nodata=nd)[0, 0, 0] == np.inf


def test_a_lone_valid_tap_of_weight_zero_gives_the_fill():
    # 3 columns into 1: the centre is column 1 exactly (t = 0), so column 2 weighs 0.0
    for dt in (np.int16, np.float64):
        a = np.array([[5, -7, 9]], dt)
        assert resample(a, (1, 1), "bilinear", nodata=-7)[0, 0] == -7  # column 1 invalid, column 2 valid but weightless
        assert resample(a, (1, 1), "bilinear", nodata=9)[0, 0] == -7  # column 1 alone
        assert resample(a, (1, 1), "cubic", nodata=5)[0, 0] == -7  # a tap of the cubic is invalid: the masked bilinear


def test_an_average_that_lands_on_nodata_is_written_as_it_is():
    a = np.array([[99, 101]], np.uint8)
    assert resample(a, (1, 1), "average", nodata=100)[0, 0] == 100
    assert decimate(a, 2, "average", nodata=100)[0, 0] == 100
    assert resample(a.astype(np.float32), (1, 1), "average", nodata=100.0)[0, 0] == 100.0


def test_refused_nodata_values():
    for dt, bad in ((np.uint8, 256), (np.uint8, -1), (np.int8, 128), (np.int16, -32769), (np.uint16, 65536),
                    (np.int32, 2**31), (np.uint32, 2**32), (np.uint16, 0.5), (np.int32, 1.5), (np.float32, 0.1),
                    (np.float32, 16777217.0), (np.float32, 1e300), (np.float32, np.inf), (np.float64, -np.inf),
                    (np.uint8, np.inf), (np.uint8, np.nan), (np.int32, "x")):
        with pytest.raises(ValueError):
            check_nodata(bad, dt)
        a = np.zeros((2, 2), dt)
        with pytest.raises(ValueError):
            resample(a, (1, 1), "average", nodata=bad)
        with pytest.raises(ValueError):
            resample(a, (1, 1), "nearest", nodata=bad)
        with pytest.raises(ValueError):
            decimate(a, 2, "average", nodata=bad)
    for dt, good in ((np.uint8, 255), (np.int8, -128), (np.uint32, 2**32 - 1), (np.float32, 0.5), (np.float32, np.nan),
                     (np.float64, 0.1), (np.float64, np.nan), (np.float32, -9999)):
        nd = check_nodata(good, dt)
        assert isinstance(nd, float) and (nd == good or (nd != nd and good != good))
