"""Decimation of a raster by a power-of-two factor: the rule of the decimated reads, stated in numpy.

This is the host path of ``streaming.read_window(decimate=k)`` / ``read_overview`` and the expectation the GPU kernel
(``k_decimate``, ``include/flac_raster_amd.h``) is tested against, bit for bit.

A region of ``h x w`` pixels is cut into ``k x k`` blocks anchored at its origin; block ``(R, C)`` covers rows
``[R k, min(R k + k, h))`` and columns ``[C k, min(C k + k, w))`` and holds ``n`` = rows x columns pixels (edge blocks
are smaller).  The output is ``ceil(h / k) x ceil(w / k)`` in the input's dtype.

``nearest``   ``out[R, C] = in[min(R k + k/2, h - 1), min(C k + k/2, w - 1)]``
``average``   integer dtypes: ``S`` = the exact integer sum of the block, ``out = rint(float64(S) / float64(n))``,
              round half to even.  Float dtypes: every element as float64; each block row is padded with ``+0.0`` to
              ``k`` elements and summed by the adjacent-pair tree (``(x0 + x1), (x2 + x3), ...`` then pairs of those,
              ``log2 k`` levels); the row sums are accumulated top to bottom (``acc = row_0; acc += row_1; ...``; rows
              the block does not have are not added); ``out = dtype(acc / float64(n))``.  Plain IEEE arithmetic: NaN
              and infinities propagate, nothing is skipped.

Resampling to any output size (``resample``, ``k_resample``): ``(B, h, w) -> (B, oh, ow)``, ``1 <= oh, ow <= 65536``,
larger or smaller than the input, same dtype.  Each axis is handled alone and the same way (columns below); with
``g = gcd(w, ow)``, ``w' = w / g`` and ``ow' = ow / g`` (rows: ``h'``, ``oh'``).  Every coordinate is an integer, every
value operation an IEEE float64 operation rounded on its own; NaN and infinities propagate, there is no nodata.

The centre of output column ``C`` lies at source coordinate ``(C + 1/2) w / ow - 1/2``: ``num = (2 C + 1) w' - ow'``,
``den = 2 ow'``, ``i0 = floor(num / den)``, ``t = float64(num - i0 den) / float64(den)``.

``nearest``   ``out[R, C] = in[min(((2 R + 1) h') // (2 oh'), h - 1), min(((2 C + 1) w') // (2 ow'), w - 1)]``
``bilinear``  taps ``i0, i0 + 1`` with weights ``[1.0 - t, t]``
``cubic``     taps ``i0 - 1 .. i0 + 2`` (Catmull-Rom, a = -1/2) with weights ``((-0.5 t + 1.0) t - 0.5) t``,
              ``((1.5 t - 2.5) t) t + 1.0``, ``((-1.5 t + 2.0) t + 0.5) t``, ``((0.5 t - 0.5) t) t``.
              Both: every tap index is clamped to the raster; vertically first, ``c_i = sum_j float64(x[j][i]) wy_j``
              for every tap column, top to bottom (``acc = p0; acc += p1; ...``), then ``v = sum_i c_i wx_i`` left to
              right.  Float dtypes: ``dtype(v)``; integer dtypes: ``rint(v)`` (half to even) clamped to the dtype.
``average``   area weights in units of ``1 / ow'`` of a source pixel: output column ``C`` covers ``[C w', (C + 1) w')``,
              source column ``i`` covers ``[i ow', (i + 1) ow')``, ``vx_i`` = the length of their intersection where
              positive (they sum to ``w'``); ``vy_j`` likewise; ``n = h' w'``.  Integer dtypes: ``S = sum_j sum_i vy_j
              vx_i x[j][i]`` exact in int64, ``out = rint(float64(S) / float64(n))``; refused when ``n 2^(8 itemsize)
              > 2^63``.  Float dtypes: ``c_i = sum_j float64(vy_j) float64(x[j][i])`` top to bottom, ``acc = sum_i
              float64(vx_i) c_i`` left to right, ``out = dtype(acc / float64(n))``; refused when ``n > 2^53``.
When the output has the input's size every mode returns the input.

Nodata-aware reads (``resample(..., nodata=nd)``, ``decimate(..., nodata=nd)``, ``k_resample_masked``; the same words as
``include/flac_raster_amd.h``):

 A nodata value nd is a double.
   For integer dtypes nd must be an integer inside the dtype's range.
   For float32 / float64 nd must be NaN, or finite and exactly representable in the dtype.
   Anything else is refused before any GPU work: ValueError in Python, FRA_E_INVALID in the C ABI.  An infinite nd
   is refused too.
   A pixel x is invalid when (double)x == nd, the same test as the statistics.  In float dtypes a NaN pixel is also
   invalid, whatever nd is.  +-inf are valid and propagate by IEEE arithmetic.  The fill is (T)nd.
 Coordinates, taps, weights, g, h', w', i0 and t are exactly those of the unmasked rule.  Only the value arithmetic
 below is new.  Every f64 operation is rounded on its own.
   nearest   unchanged: it picks one pixel, invalid or not.
   average   (resample)  Down the output row's source rows j, top to bottom, for every source column i:
             integer dtypes: c_i = the sum of vy_j x[j][i] over the valid pixels, exact in int64; float dtypes: the
             first valid term initialises c_i and later valid terms are added (c_i = term; c_i += term; ...).
             u_i = the integer sum of vy_j over the valid pixels.
             Then over the output's source columns i, left to right, skipping the columns with u_i == 0:
             S = sum_i vx_i c_i (floats: acc = (double)vx_i * c_i, the first non-skipped column initialising) and
             W = sum_i vx_i u_i, exact in int64, 1 <= W <= n.  W == 0 gives the fill.  Otherwise integers give
             rint((double)S / (double)W), half to even (between the valid extremes: no clamp), and floats give
             (T)(acc / (double)W).  The two overflow bounds of the unmasked average apply unchanged.
             With no invalid pixel the result equals the unmasked resampling bit for bit in every dtype, -0.0
             included.  An average of valid pixels that happens to land on nd is written as it is (possible only
             when nd lies strictly inside the data's range); nothing is nudged.
   average   (decimate, factor k)  The same arithmetic with h' = w' = k and oh' = ow' = 1: every weight is 1, the tap
             ranges are clipped at the raster's edge, the output is ceil(h / k) x ceil(w / k), and edge blocks need
             no special case because the divisor is W, the count of valid pixels.  The float summation order is the
             one above, not the adjacent-pair tree of the unmasked decimation.  So for k dividing h and w the
             decimation equals the resampling to (h / k, w / k) bit for bit in every dtype, and with no invalid
             pixel it equals the unmasked decimation for integer dtypes only.
   bilinear, cubic   If all taps of the output (4 or 16, after clamping) are valid, the result is the unmasked
             formula exactly, with no division.  Otherwise the result is the masked bilinear of the same centre,
             whichever of the two modes was asked for (a cubic kernel's negative weights cannot be renormalised
             safely): taps i0, i0 + 1 per axis, clamped, weights wy = [1.0 - ty, ty] and wx likewise.  Vertically
             c_i = the sum of (double)x[j][i] * wy_j over the valid j in ascending order, the first valid term
             initialising, and u_i = the sum of wy_j over the valid j.  Horizontally, over the columns with at
             least one valid tap, v = sum_i c_i * wx_i and Wt = sum_i u_i * wx_i in ascending order, the first such
             column initialising both.  No valid tap, or Wt <= 0.0 (a lone valid tap with weight exactly 0), gives
             the fill.  Otherwise q = v / Wt; floats give (T)q, integers rint(q) clamped to the dtype.
   When (oh, ow) = (h, w) every mode of the resampling returns the input.
"""

from __future__ import annotations

from math import gcd
from typing import Sequence, Tuple

import numpy as np

FACTORS = (2, 4, 8, 16, 32, 64)
RESAMPLING = {"nearest": 0, "average": 1}
RESAMPLING_ANY = {"nearest": 0, "average": 1, "bilinear": 2, "cubic": 3}  # of resample(); decimate() knows the first two
MAX_OUT = 65536
_DTYPES = tuple(np.dtype(t) for t in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32,
                                      np.float64))


def check_factor(factor) -> int:
    k = int(factor)
    if k not in FACTORS or k != factor:
        raise ValueError(f"the decimation factor must be one of {FACTORS}, got {factor!r}")
    return k


def resampling_code(resampling) -> int:
    if resampling not in RESAMPLING:
        raise ValueError(f"resampling must be 'nearest' or 'average', got {resampling!r}")
    return RESAMPLING[resampling]


def decimated_shape(h: int, w: int, k: int) -> Tuple[int, int]:
    """``(ceil(h / k), ceil(w / k))``."""
    k = check_factor(k)
    return -(-int(h) // k), -(-int(w) // k)


def decimated_transform(transform: Sequence[float], window: Sequence[int], k: int) -> Tuple[float, ...]:
    """The geotransform ``(a, b, c, d, e, f)`` of a region decimated by ``k``: ``window`` = (row_off, col_off, ...) is
    the region in the raster ``transform`` belongs to.  ``k = 1`` is the plain shift to the region's origin."""
    a, b, c, d, e, f = (float(v) for v in tuple(transform)[:6])
    row, col = int(window[0]), int(window[1])
    return a * k, b * k, c + col * a + row * b, d * k, e * k, f + col * d + row * e


def decimate(raster: np.ndarray, factor: int, resampling: str = "nearest", nodata=None) -> np.ndarray:
    """``raster`` ``(B, h, w)`` or ``(h, w)`` at ``1 / factor`` resolution (the module's rule), same dtype.  With
    ``nodata`` the average leaves that value (and NaN) out: the nodata-aware rule."""
    k = check_factor(factor)
    mode = resampling_code(resampling)
    a = np.asarray(raster)
    if a.ndim == 2:
        return decimate(a[None], k, resampling, nodata)[0]
    if a.ndim != 3 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"expected a (B, h, w) or (h, w) raster with h, w >= 1, got shape {a.shape}")
    if a.dtype.newbyteorder("=") not in _DTYPES:
        raise TypeError(f"unsupported dtype {a.dtype}")
    B, h, w = a.shape
    oh, ow = decimated_shape(h, w, k)
    if nodata is not None:
        nd = check_nodata(nodata, a.dtype)
        if mode == 1:
            return _masked_area(a, *_block_taps(h, k), *_block_taps(w, k), nd)
    if mode == 0:
        rows = np.minimum(np.arange(oh) * k + k // 2, h - 1)
        cols = np.minimum(np.arange(ow) * k + k // 2, w - 1)
        return np.ascontiguousarray(a[:, rows[:, None], cols[None, :]])
    is_float = a.dtype.kind == "f"
    acc_t = np.float64 if is_float else np.int64
    # the blocks as (B, oh, k, ow, k); what the raster does not have is +0.0 / 0
    x = np.zeros((B, oh * k, ow * k), dtype=acc_t)
    x[:, :h, :w] = a
    x = x.reshape(B, oh, k, ow, k)
    with np.errstate(invalid="ignore", over="ignore"):
        while x.shape[-1] > 1:  # the adjacent-pair tree along a block row
            x = x[..., 0::2] + x[..., 1::2]
        rows = x[..., 0]  # (B, oh, k, ow): the row sums of every block
        nrows = np.minimum(k, h - np.arange(oh) * k)  # rows of the blocks of block row R
        ncols = np.minimum(k, w - np.arange(ow) * k)
        acc = rows[:, :, 0, :].copy()
        for j in range(1, k):  # top to bottom; rows a block does not have are not added
            have = (j < nrows)[None, :, None]
            acc = np.where(have, acc + rows[:, :, j, :], acc)
        n = (nrows[:, None] * ncols[None, :]).astype(np.float64)
        if is_float:
            return (acc / n).astype(a.dtype)
        return np.rint(acc.astype(np.float64) / n).astype(a.dtype)


# ------------------------------------------------------------------------------- any output size
def resampling_any_code(resampling) -> int:
    if resampling not in RESAMPLING_ANY:
        raise ValueError(f"resampling must be one of {tuple(RESAMPLING_ANY)}, got {resampling!r}")
    return RESAMPLING_ANY[resampling]


def check_out_shape(out_shape) -> Tuple[int, int]:
    try:
        oh, ow = out_shape
        ok = int(oh) == oh and int(ow) == ow and 1 <= oh <= MAX_OUT and 1 <= ow <= MAX_OUT
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"out_shape must be (height, width) with 1 <= height, width <= {MAX_OUT}, got {out_shape!r}")
    return int(oh), int(ow)


def max_size_shape(h: int, w: int, max_size: int) -> Tuple[int, int]:
    """The output shape whose longest side is ``max_size``; the other is ``max(1, round(side max_size / longest))``."""
    n, longest = int(max_size), max(int(h), int(w))
    if n != max_size or not 1 <= n <= MAX_OUT:
        raise ValueError(f"max_size must be an integer in 1 .. {MAX_OUT}, got {max_size!r}")
    other = max(1, round(min(int(h), int(w)) * n / longest))
    return (n, other) if h >= w else (other, n)


def check_average_size(h: int, w: int, oh: int, ow: int, dtype) -> int:
    """``n = h' w'`` of the area average, refused where the rule's arithmetic would no longer be exact."""
    n = (h // gcd(h, oh)) * (w // gcd(w, ow))
    dt = np.dtype(dtype)
    if dt.kind == "f":
        if n > 2**53:
            raise ValueError(f"average: {h} x {w} -> {oh} x {ow} has n = {n} > 2^53 weights per output pixel")
    elif n * 2**(8 * dt.itemsize) > 2**63:
        raise ValueError(f"average: {h} x {w} -> {oh} x {ow} with n = {n} overflows the 64-bit sum of {dt.name}")
    return n


def resampled_transform(transform: Sequence[float], window: Sequence[int],
                        out_shape: Sequence[int]) -> Tuple[float, ...]:
    """The geotransform ``(a, b, c, d, e, f)`` of a region ``window`` = (row_off, col_off, height, width) of the raster
    ``transform`` belongs to, resampled to ``out_shape``.  At ``height / oh = width / ow = k`` this is
    ``decimated_transform``."""
    a, b, c, d, e, f = (float(v) for v in tuple(transform)[:6])
    row, col, h, w = (int(v) for v in tuple(window)[:4])
    oh, ow = check_out_shape(out_shape)
    sx, sy = w / ow, h / oh
    return a * sx, b * sy, c + col * a + row * b, d * sx, e * sy, f + col * d + row * e


def _centres(n_in: int, n_out: int):
    """``(i0, t)`` of every output index along one axis."""
    g = gcd(n_in, n_out)
    ni, no = n_in // g, n_out // g
    num = (2 * np.arange(n_out, dtype=np.int64) + 1) * ni - no
    den = 2 * no
    i0 = num // den
    return i0, (num - i0 * den).astype(np.float64) / np.float64(den)


def _tap_weights(t: np.ndarray, mode: int):
    if mode == 2:
        return [1.0 - t, t]
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
            ((0.5 * t - 0.5) * t) * t]


def _area_taps(n_in: int, n_out: int):
    """``(first, weights)`` along one axis: ``weights[k, C]`` is the integer weight of source index ``first[C] + k``
    for output ``C`` (0 past its last tap)."""
    g = gcd(n_in, n_out)
    ni, no = n_in // g, n_out // g
    C = np.arange(n_out, dtype=np.int64)
    first = (C * ni) // no
    taps = int((-(-(C + 1) * ni // no) - first).max())
    i = first[None, :] + np.arange(taps, dtype=np.int64)[:, None]
    wts = np.minimum((i + 1) * no, ((C + 1) * ni)[None, :]) - np.maximum(i * no, (C * ni)[None, :])
    return first, np.maximum(wts, 0)


def _tap_filter(x: np.ndarray, oh: int, ow: int, mode: int) -> np.ndarray:
    """The bilinear (2) or cubic (3) combination of ``x`` (B, h, w) float64, before the conversion to the dtype."""
    h, w = x.shape[1:]
    i0y, ty = _centres(h, oh)
    i0x, tx = _centres(w, ow)
    off = 0 if mode == 2 else -1
    cols = None  # (B, oh, w): every source column combined vertically for output row R
    for k, wy in enumerate(_tap_weights(ty, mode)):
        term = x[:, np.clip(i0y + off + k, 0, h - 1), :] * wy[None, :, None]
        cols = term if k == 0 else cols + term
    v = None
    for k, wx in enumerate(_tap_weights(tx, mode)):
        term = cols[:, :, np.clip(i0x + off + k, 0, w - 1)] * wx[None, None, :]
        v = term if k == 0 else v + term
    return v


# ------------------------------------------------------------------------------- nodata-aware
def check_nodata(nodata, dtype) -> float:
    """``nodata`` as the float the rule admits for ``dtype``: an integer inside an integer dtype's range; for floats
    NaN, or finite and exactly representable.  ``ValueError`` otherwise."""
    dt = np.dtype(dtype).newbyteorder("=")
    if dt not in _DTYPES:
        raise TypeError(f"unsupported dtype {dt}")
    try:
        nd = float(nodata)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"nodata must be a number, got {nodata!r}") from None
    if dt.kind == "f":
        with np.errstate(over="ignore"):
            ok = nd != nd or (abs(nd) != float("inf") and float(dt.type(nd)) == nd)
    else:
        info = np.iinfo(dt)
        ok = nd == nd and abs(nd) != float("inf") and nd == int(nd) and info.min <= nd <= info.max
    if not ok:
        raise ValueError(f"nodata {nodata!r} is not a value of {dt.name}: an integer in range; for floats NaN, or "
                         "finite and exact")
    return nd


def fill_value(nodata: float, dtype):
    """The fill ``(T)nd`` of a checked nodata value."""
    dt = np.dtype(dtype)
    return dt.type(nodata) if dt.kind == "f" else dt.type(int(nodata))


def valid_mask(a: np.ndarray, nodata: float) -> np.ndarray:
    """The pixels that are neither ``nodata`` nor, in a float dtype, NaN."""
    if a.dtype.kind == "f":
        return ~(a == fill_value(nodata, a.dtype)) & ~np.isnan(a)
    return a != fill_value(nodata, a.dtype)


def _block_taps(n: int, k: int):
    """``(first, weights)`` of the decimation by ``k`` along one axis, as ``_area_taps`` gives them: block ``C`` starts
    at ``C k`` and every index it has inside the raster weighs 1."""
    first = np.arange(-(-n // k), dtype=np.int64) * k
    return first, ((first[None, :] + np.arange(k, dtype=np.int64)[:, None]) < n).astype(np.int64)


def _masked_area(a: np.ndarray, firsty, vy, firstx, vx, nd: float) -> np.ndarray:
    """The nodata-aware average of ``a`` (B, h, w) over the integer taps of the two axes."""
    B, h, w = a.shape
    dt = a.dtype
    is_float = dt.kind == "f"
    acc_t = np.float64 if is_float else np.int64
    valid = valid_mask(a, nd)
    x = a.astype(acc_t)
    oh, ow = len(firsty), len(firstx)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = np.zeros((B, oh, w), acc_t)  # every source column summed down the valid rows of output row R
        u = np.zeros((B, oh, w), np.int64)  # ... and the weights of those rows
        for k in range(vy.shape[0]):
            rows = np.minimum(firsty + k, h - 1)
            ok = valid[:, rows, :] & (vy[k] > 0)[None, :, None]
            term = vy[k].astype(acc_t)[None, :, None] * x[:, rows, :]
            c = np.where(ok, np.where(u > 0, c + term, term), c) if is_float else c + np.where(ok, term, 0)
            u = u + np.where(ok, vy[k][None, :, None], 0)
        S = np.zeros((B, oh, ow), acc_t)
        W = np.zeros((B, oh, ow), np.int64)
        for k in range(vx.shape[0]):
            cols = np.minimum(firstx + k, w - 1)
            uu = u[:, :, cols]
            ok = (uu > 0) & (vx[k] > 0)[None, None, :]  # a column without a valid pixel is skipped
            term = vx[k].astype(acc_t)[None, None, :] * c[:, :, cols]
            S = np.where(ok, np.where(W > 0, S + term, term), S) if is_float else S + np.where(ok, term, 0)
            W = W + np.where(ok, vx[k][None, None, :] * uu, 0)
        div = np.where(W > 0, W, 1).astype(np.float64)
        q = S / div if is_float else np.rint(S.astype(np.float64) / div)
        return np.where(W > 0, q.astype(dt), fill_value(nd, dt)).astype(dt, order="C")


def _masked_taps(a: np.ndarray, oh: int, ow: int, mode: int, nd: float) -> np.ndarray:
    """The nodata-aware bilinear (2) or cubic (3) of ``a`` (B, h, w)."""
    B, h, w = a.shape
    dt = a.dtype
    valid = valid_mask(a, nd)
    x = a.astype(np.float64)
    i0y, ty = _centres(h, oh)
    i0x, tx = _centres(w, ow)
    off, nt = (0, 2) if mode == 2 else (-1, 4)
    whole = _tap_filter(x, oh, ow, mode)  # what the outputs whose taps are all valid get
    rows_ok = np.ones((B, oh, w), bool)
    for k in range(nt):
        rows_ok &= valid[:, np.clip(i0y + off + k, 0, h - 1), :]
    all_ok = np.ones((B, oh, ow), bool)
    for k in range(nt):
        all_ok &= rows_ok[:, :, np.clip(i0x + off + k, 0, w - 1)]
    # the masked bilinear of every centre
    c = np.zeros((B, oh, w))
    u = np.zeros((B, oh, w))
    have = np.zeros((B, oh, w), bool)
    for k, wy in enumerate((1.0 - ty, ty)):
        rows = np.clip(i0y + k, 0, h - 1)
        ok = valid[:, rows, :]
        term = x[:, rows, :] * wy[None, :, None]
        wk = np.broadcast_to(wy[None, :, None], term.shape)
        c = np.where(ok, np.where(have, c + term, term), c)
        u = np.where(ok, np.where(have, u + wk, wk), u)
        have = have | ok
    v = np.zeros((B, oh, ow))
    wt = np.zeros((B, oh, ow))
    seen = np.zeros((B, oh, ow), bool)
    for k, wx in enumerate((1.0 - tx, tx)):
        cols = np.clip(i0x + k, 0, w - 1)
        ok = have[:, :, cols]
        tc = c[:, :, cols] * wx[None, None, :]
        tu = u[:, :, cols] * wx[None, None, :]
        v = np.where(ok, np.where(seen, v + tc, tc), v)
        wt = np.where(ok, np.where(seen, wt + tu, tu), wt)
        seen = seen | ok
    fill = ~all_ok & (~seen | (wt <= 0.0))
    q = np.where(all_ok, whole, v / np.where(wt > 0.0, wt, 1.0))
    if dt.kind == "f":
        out = q.astype(dt, order="C")
    else:
        info = np.iinfo(dt)
        out = np.clip(np.rint(np.where(fill, 0.0, q)), np.float64(info.min), np.float64(info.max)).astype(dt, order="C")
    out[fill] = fill_value(nd, dt)
    return out


def resample(raster: np.ndarray, out_shape: Sequence[int], resampling: str = "nearest", nodata=None) -> np.ndarray:
    """``raster`` ``(B, h, w)`` or ``(h, w)`` resampled to ``out_shape`` = (oh, ow) (the module's rule), same dtype.
    With ``nodata`` the average, the bilinear and the cubic leave that value (and NaN) out: the nodata-aware rule."""
    mode = resampling_any_code(resampling)
    oh, ow = check_out_shape(out_shape)
    a = np.asarray(raster)
    if a.ndim == 2:
        return resample(a[None], (oh, ow), resampling, nodata)[0]
    if a.ndim != 3 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"expected a (B, h, w) or (h, w) raster with h, w >= 1, got shape {a.shape}")
    if a.dtype.newbyteorder("=") not in _DTYPES:
        raise TypeError(f"unsupported dtype {a.dtype}")
    B, h, w = a.shape
    dt = a.dtype
    is_float = dt.kind == "f"
    nd = None if nodata is None else check_nodata(nodata, dt)
    if (oh, ow) == (h, w):
        return np.array(a, order="C")
    if nd is not None and mode != 0:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if mode == 1:
                check_average_size(h, w, oh, ow, dt)
                return _masked_area(a, *_area_taps(h, oh), *_area_taps(w, ow), nd)
            return _masked_taps(a, oh, ow, mode, nd)
    if mode == 0:
        gh, gw = gcd(h, oh), gcd(w, ow)
        rows = np.minimum(((2 * np.arange(oh, dtype=np.int64) + 1) * (h // gh)) // (2 * (oh // gh)), h - 1)
        cols = np.minimum(((2 * np.arange(ow, dtype=np.int64) + 1) * (w // gw)) // (2 * (ow // gw)), w - 1)
        return np.ascontiguousarray(a[:, rows[:, None], cols[None, :]])
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 1:
            n = check_average_size(h, w, oh, ow, dt)
            acc_t = np.float64 if is_float else np.int64
            x = a.astype(acc_t)
            firsty, vy = _area_taps(h, oh)
            firstx, vx = _area_taps(w, ow)
            cols = None  # (B, oh, w): every source column summed down the rows of output row R
            for k in range(vy.shape[0]):
                term = vy[k].astype(acc_t)[None, :, None] * x[:, np.minimum(firsty + k, h - 1), :]
                cols = term if k == 0 else np.where((vy[k] > 0)[None, :, None], cols + term, cols)
            acc = None
            for k in range(vx.shape[0]):
                term = vx[k].astype(acc_t)[None, None, :] * cols[:, :, np.minimum(firstx + k, w - 1)]
                acc = term if k == 0 else np.where((vx[k] > 0)[None, None, :], acc + term, acc)
            if is_float:
                return (acc / np.float64(n)).astype(dt, order="C")
            return np.rint(acc.astype(np.float64) / np.float64(n)).astype(dt, order="C")
        v = _tap_filter(a.astype(np.float64), oh, ow, mode)
        if is_float:
            return v.astype(dt, order="C")
        info = np.iinfo(dt)
        return np.clip(np.rint(v), np.float64(info.min), np.float64(info.max)).astype(dt, order="C")
