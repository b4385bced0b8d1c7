"""Proximity: the exact Euclidean distance of every pixel to the nearest target pixel, and nearest-target allocation.

The rule of ``fra_proximity`` (``include/flac_raster_amd.h``, "Proximity") restated in numpy, twice:

* :func:`proximity_direct` is the definition: every output pixel against every target, in chunks;
* :func:`proximity_arrays` is the separable form the kernels use: per column the vertical distance ``g`` to the nearest
  target (above wins a tie), then per row ``min over c' of g[c']^2 + (c - c')^2`` with the leftmost ``c'`` winning.

Both give, per band of a ``(B, h, w)`` raster: the integer squared distance ``d2`` to the nearest target, that target
(smallest column, then smallest row among the nearest), ``d = sqrt(float64(d2)) * scale``, the reach ``d <= max_dist`` and
the two outputs ``dist`` and ``alloc``.  The GPU results equal them byte for byte.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from .calc import convert

MAX_SIDE = 32768
MAX_D2 = 2 * 32767 * 32767   # the greatest squared distance inside a region, below 2^31
MAX_VALUES = 16
_FAR = np.int64(1) << 40     # no distance: above every d2


@dataclass(frozen=True)
class Options:
    """What a proximity call is asked for.

    ``values``: the target values (at most 16); empty: every pixel that is non-zero and not NaN.  ``max_dist``: the
    reach in the units of ``scale`` (``None``: no limit).  ``scale``: the size of a pixel (1: pixel units).  ``fixed``: a
    value every pixel within reach gets instead of its distance, the targets included.  ``fill``: what the other pixels
    of ``dist`` get (``None``: :func:`default_fill` of the output dtype); ``alloc_fill``: what they get in ``alloc``."""

    values: Tuple[float, ...] = ()
    max_dist: Optional[float] = None
    scale: float = 1.0
    fixed: Optional[float] = None
    fill: Optional[float] = None
    alloc_fill: float = 0.0


def default_fill(out_dtype) -> float:
    """NaN for a float ``dist``, the dtype's maximum for an integer one."""
    dt = np.dtype(out_dtype)
    return float("nan") if dt.kind == "f" else float(np.iinfo(dt).max)


def validate(opts: Options) -> None:
    """``ValueError`` for options the rule refuses, in the library's order."""
    if len(opts.values) > MAX_VALUES:
        raise ValueError(f"values: {len(opts.values)} target values (0 .. {MAX_VALUES})")
    for i, v in enumerate(opts.values):
        if not math.isfinite(float(v)):
            raise ValueError(f"values: target value {i} is not finite")
    if not math.isfinite(float(opts.scale)) or not float(opts.scale) > 0.0:
        raise ValueError(f"scale: {opts.scale} is not finite and positive")
    if opts.max_dist is not None and not float(opts.max_dist) >= 0.0:
        raise ValueError(f"max_dist: {opts.max_dist} is NaN or negative")


def check_region(h: int, w: int, out_window) -> Tuple[int, int, int, int]:
    """The output window (default: the whole region) of an ``h x w`` region, checked as the library checks it."""
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"the region must be 1 .. {MAX_SIDE} in each dimension (got {h} x {w})")
    r0, c0, oh, ow = (0, 0, h, w) if out_window is None else (int(v) for v in out_window)
    if oh < 1 or ow < 1 or r0 < 0 or c0 < 0 or r0 + oh > h or c0 + ow > w:
        raise ValueError(f"the output window ({r0}, {c0}, {oh} x {ow}) is empty or not inside the region ({h} x {w})")
    return r0, c0, oh, ow


def distance(d2, scale: float) -> np.ndarray:
    """``sqrt(float64(d2)) * scale``, each operation rounded on its own."""
    return np.sqrt(np.asarray(d2).astype(np.float64)) * np.float64(scale)


def reach_threshold(opts: Options) -> int:
    """The greatest ``d2`` in ``0 .. MAX_D2`` with ``distance(d2) <= max_dist``: the predicate is monotone in ``d2`` and
    holds at 0, so a bisection finds it."""
    if opts.max_dist is None:
        return MAX_D2
    md = np.float64(opts.max_dist)
    if distance(MAX_D2, opts.scale) <= md:
        return MAX_D2
    lo, hi = 0, MAX_D2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if distance(mid, opts.scale) <= md:
            lo = mid
        else:
            hi = mid
    return lo


def halo(opts: Options) -> Optional[int]:
    """The pixels a window must be grown by for its result to be the crop of the whole: ``ceil(max_dist / scale)``, no
    more than a region holds; ``None`` without a ``max_dist`` (the whole raster is needed)."""
    if opts.max_dist is None:
        return None
    return math.isqrt(reach_threshold(opts) - 1) + 1 if reach_threshold(opts) > 0 else 0


def targets_of(band: np.ndarray, values: Sequence[float]) -> np.ndarray:
    """The target mask of one band."""
    if len(values) == 0:
        m = band != 0
        return m & ~np.isnan(band) if band.dtype.kind == "f" else m
    x = band.astype(np.float64)
    m = np.zeros(band.shape, dtype=bool)
    for v in values:
        m |= x == np.float64(v)
    return m


def _as_bands(raster) -> np.ndarray:
    a = np.asarray(raster)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("raster must be (B, h, w) or (h, w)")
    return a


def _finish(band, d2, tr, tc, opts: Options, dist_dtype):
    """``(dist, alloc, pixels within reach)`` of one band's output window from ``d2`` (``_FAR``: none) and the nearest
    target's row and column."""
    has = d2 < _FAR
    d = distance(np.where(has, d2, 0), opts.scale)
    reach = has if opts.max_dist is None else has & (d <= np.float64(opts.max_dist))
    dist = None
    if dist_dtype is not None:
        fill = default_fill(dist_dtype) if opts.fill is None else float(opts.fill)
        v = np.where(reach, d if opts.fixed is None else np.float64(opts.fixed), np.float64(fill))
        dist = convert(v, dist_dtype)
    af = convert(np.array([float(opts.alloc_fill)]), band.dtype)[0]
    alloc = np.where(reach, band[np.where(reach, tr, 0), np.where(reach, tc, 0)], af).astype(band.dtype)
    return dist, alloc, int(reach.sum())


def _run(raster, opts: Options, out_window, dist_dtype, nearest):
    a = _as_bands(raster)
    validate(opts)
    B, h, w = a.shape
    win = check_region(h, w, out_window)
    dists, allocs, counts = [], [], np.zeros(3, np.uint64)
    for b in range(B):
        mask = targets_of(a[b], opts.values)
        d2, tr, tc = nearest(mask, win, reach_threshold(opts))
        dist, alloc, reached = _finish(a[b], d2, tr, tc, opts, dist_dtype)
        dists.append(dist), allocs.append(alloc)
        counts += np.array([int(mask.sum()), reached, win[2] * win[3] - reached], np.uint64)
    return (None if dist_dtype is None else np.stack(dists)), np.stack(allocs), counts


def _nearest_direct(mask, win, t2, chunk: int = 1 << 22):
    r0, c0, oh, ow = win
    tr, tc = (v.astype(np.int64) for v in np.nonzero(mask))
    d2 = np.full((oh, ow), _FAR, np.int64)
    nr, nc = np.zeros((oh, ow), np.int64), np.zeros((oh, ow), np.int64)
    if tr.size == 0:
        return d2, nr, nc
    rr, cc = np.divmod(np.arange(oh * ow, dtype=np.int64), ow)
    rr, cc = rr + r0, cc + c0
    step = max(1, chunk // tr.size)
    d2f, nrf, ncf = d2.reshape(-1), nr.reshape(-1), nc.reshape(-1)
    for s in range(0, oh * ow, step):
        e = min(oh * ow, s + step)
        dd = (rr[s:e, None] - tr[None, :]) ** 2 + (cc[s:e, None] - tc[None, :]) ** 2
        # the least d2, then the least column, then the least row: one key (d2 < 2^31, columns and rows < 2^15)
        k = np.argmin((dd << 30) | (tc[None, :] << 15) | tr[None, :], axis=1)
        d2f[s:e], nrf[s:e], ncf[s:e] = dd[np.arange(e - s), k], tr[k], tc[k]
    return d2, nr, nc


def column_pass(mask: np.ndarray, win, t2: int):
    """Per pixel of the output window's rows (all columns of the region): the vertical distance ``g`` to the nearest
    target of its column (``-1``: none, or beyond the reach) and whether that target lies below (above wins a tie)."""
    h, w = mask.shape
    r0, _, oh, _ = win
    rows = np.arange(h, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(mask, rows, -1), axis=0)                       # the last target at or above
    dn = np.minimum.accumulate(np.where(mask, rows, _FAR)[::-1], axis=0)[::-1]          # the first one at or below
    ga = np.where(up >= 0, rows - up, _FAR)[r0:r0 + oh]
    gb = np.where(dn < _FAR, dn - rows, _FAR)[r0:r0 + oh]
    g, below = np.minimum(ga, gb), gb < ga
    return np.where(g > math.isqrt(t2), -1, g), below


def _nearest_separable(mask, win, t2):
    r0, c0, oh, ow = win
    h, w = mask.shape
    g, below = column_pass(mask, win, t2)
    g2 = np.where(g >= 0, g * g, _FAR)
    best = np.full((oh, ow), _FAR, np.int64)
    bj = np.zeros((oh, ow), np.int64)
    live = (g >= 0).any(axis=1)  # rows with a candidate at all: the others never get a d2
    reach = min(w - 1, math.isqrt(t2))
    for dx in range(0, reach + 1 if live.any() else 0):
        if dx * dx > int(best[live].max()):  # no closer candidate is left for any pixel
            break
        for sgn in ((-1, 1) if dx else (1,)):
            # the candidates j = c + sgn * dx of the output pixels c = c0 .. c0 + ow - 1, inside the region
            ca, cb = max(c0, -sgn * dx), min(c0 + ow, w - sgn * dx)
            if ca >= cb:
                continue
            cand = g2[:, ca + sgn * dx:cb + sgn * dx] + dx * dx
            cur = best[:, ca - c0:cb - c0]
            better = (cand <= cur) & (cand < _FAR) if sgn < 0 else cand < cur  # a smaller column wins a tie
            best[:, ca - c0:cb - c0] = np.where(better, cand, cur)
            bj[:, ca - c0:cb - c0] = np.where(better, np.arange(ca, cb)[None, :] + sgn * dx, bj[:, ca - c0:cb - c0])
    best = np.where(best >= _FAR, _FAR, best)
    rr = np.arange(r0, r0 + oh, dtype=np.int64)[:, None]
    gj = np.take_along_axis(np.where(g >= 0, g, 0), bj, axis=1)
    bl = np.take_along_axis(below, bj, axis=1)
    return best, np.where(bl, rr + gj, rr - gj), bj


def proximity_direct(raster, opts: Options = Options(), out_window=None, dist_dtype="float32"):
    """The definition, all pairs in chunks: ``(dist (B, oh, ow) in dist_dtype or None, alloc (B, oh, ow) in the
    raster's dtype, counts = [targets, output pixels within reach, output pixels filled] (uint64))``.
    ``out_window`` = (row_off, col_off, oh, ow) inside the raster, default all of it; ``dist_dtype=None``: no ``dist``."""
    return _run(raster, opts, out_window, dist_dtype, _nearest_direct)


def proximity_arrays(raster, opts: Options = Options(), out_window=None, dist_dtype="float32"):
    """The separable form (columns, then rows); arguments and result as :func:`proximity_direct`, which it equals."""
    return _run(raster, opts, out_window, dist_dtype, _nearest_separable)


def scale_of(transform, units: str) -> float:
    """The ``scale`` of a call: 1 for ``units='pixel'``; for ``'geo'`` the pixel size of an axis-aligned transform with
    square pixels.  Non-square pixels would need anisotropic distances, which the transform here does not do."""
    if units == "pixel":
        return 1.0
    if units != "geo":
        raise ValueError("units must be 'pixel' or 'geo'")
    if not transform:
        raise ValueError("geo units need a transform (the pixel size)")
    a, b, _, d, e, _ = (float(v) for v in list(transform)[:6])
    if b != 0.0 or d != 0.0:
        raise ValueError("geo units need an axis-aligned transform: a rotated grid is not supported")
    if abs(a) != abs(e) or a == 0.0:
        raise ValueError(f"geo units need square pixels (|a| = {abs(a)}, |e| = {abs(e)}): anisotropic distances are not supported")
    return abs(a)
