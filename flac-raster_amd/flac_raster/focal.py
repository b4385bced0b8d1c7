"""Focal operations: a ``kh x kw`` window around every pixel of every band of a raster.

The rule of ``fra_focal`` / ``fra_decode_device_focal`` (the normative text is in ``include/flac_raster_amd.h``), in
numpy: the GPU is checked against :func:`focal_arrays` bit for bit, never against itself.

Every band of a ``(B, h, w)`` raster is processed on its own; the result covers an output rectangle inside the source,
and neighbours inside the source but outside the rectangle are read, so a rectangle of the result is the crop of the
whole-raster result.  Every element is taken as f64 and every arithmetic step is one IEEE f64 operation; the taps of a
window are visited in row-major order.  A tap is left out when it is NaN, when a nodata value is given and ``float(x) ==
nodata`` (a NaN nodata matches nothing), and when it lies outside the source and the edge mode is ``"skip"``; with
``"clamp"`` a tap outside the source is the nearest source pixel.  ``n`` is the number of valid taps.

``sum``: the valid taps added in tap order, starting from the first valid one; ``mean``: that sum ``/ n``; ``min`` /
``max``: ``m = x < m ? x : m`` (``>``) in tap order from the first valid tap; ``count``: ``n``; ``median``: the lower
median (rank ``(n - 1) // 2`` by value, equal values by tap order), at most 25 taps; ``convolve``: the rounded products
``x * w`` added in tap order, with ``normalize`` divided by the valid taps' weights added the same way (a sum of 0 gives
``fill``); ``slope`` / ``hillshade``: Horn's 3 x 3 gradient, see :func:`focal_arrays`.  A pixel gets ``fill`` when no tap
is valid (``count`` gives 0), when an op says so, and with ``keep_mask`` when the centre pixel itself is left out.  The
conversion to the output dtype is the band math's (``calc.convert``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np

from .calc import DTYPES, convert, default_fill

OPS = ("sum", "mean", "min", "max", "count", "median", "convolve", "slope", "hillshade")
SUM, MEAN, MIN, MAX, COUNT, MEDIAN, CONVOLVE, SLOPE, HILLSHADE = range(len(OPS))
EDGES = ("skip", "clamp")
EDGE_SKIP, EDGE_CLAMP = 0, 1
FLAG_NODATA, FLAG_NORMALIZE, FLAG_KEEP_MASK = 1, 2, 4
MAX_SIZE, MAX_MEDIAN = 15, 25


@dataclass
class Spec:
    """A focal operation: ``op`` (a name of ``OPS`` or its number), the window ``size`` = (kh, kw) or one odd number
    (default: the shape of 2-D ``weights``, else 3), ``edge`` (``"skip"`` / ``"clamp"`` or its number), ``nodata``
    (``None``: nothing but NaN is masked), ``fill`` (``None``: the default of the output dtype), ``normalize`` and
    ``keep_mask``, the ``weights`` of ``convolve`` (kh x kw, row-major) and the ``params`` of ``slope`` / ``hillshade``
    (:func:`slope_params`, :func:`hillshade_params`).  ``flags``: further flag bits, passed on as they are (the
    validators refuse unknown ones)."""

    op: object
    size: object = None
    edge: object = "skip"
    nodata: Optional[float] = None
    fill: Optional[float] = None
    normalize: bool = False
    keep_mask: bool = False
    weights: Optional[Sequence[float]] = None
    params: Sequence[float] = field(default_factory=tuple)
    flags: int = 0

    def __post_init__(self):
        if isinstance(self.op, str):
            if self.op.lower() not in OPS:
                raise ValueError(f"op: unknown focal op {self.op!r} (one of {', '.join(OPS)})")
            self.op = OPS.index(self.op.lower())
        self.op = int(self.op)
        if isinstance(self.edge, str):
            if self.edge.lower() not in EDGES:
                raise ValueError(f"edge: unknown edge mode {self.edge!r} (skip or clamp)")
            self.edge = EDGES.index(self.edge.lower())
        self.edge = int(self.edge)
        if self.weights is not None:
            self.weights = np.asarray(self.weights, dtype=np.float64)
            if self.size is None and self.weights.ndim == 2:
                self.size = self.weights.shape
        if self.size is None:
            self.size = 3
        if np.ndim(self.size) == 0:
            self.size = (int(self.size), int(self.size))
        self.size = (int(self.size[0]), int(self.size[1]))
        if self.weights is not None:
            if self.weights.size != self.size[0] * self.size[1] or self.weights.size > MAX_SIZE * MAX_SIZE:
                raise ValueError(f"weights: {self.weights.size} weights for a {self.size[0]} x {self.size[1]} window")
            self.weights = self.weights.reshape(self.size)
        self.params = tuple(float(v) for v in self.params)
        if len(self.params) > 8:
            raise ValueError("params: more than 8 parameters")

    @property
    def kh(self) -> int:
        return self.size[0]

    @property
    def kw(self) -> int:
        return self.size[1]

    def flag_bits(self) -> int:
        return (int(self.flags) | (FLAG_NODATA if self.nodata is not None else 0)
                | (FLAG_NORMALIZE if self.normalize else 0) | (FLAG_KEEP_MASK if self.keep_mask else 0))


def validate(spec: Spec) -> None:
    """The Python twin of the C validator (``fra_focal_check``): ``ValueError`` naming the field for whatever it
    refuses, in its order."""
    flags = spec.flag_bits()
    if not SUM <= spec.op <= HILLSHADE:
        raise ValueError(f"op: unknown focal op {spec.op}")
    if spec.edge not in (EDGE_SKIP, EDGE_CLAMP):
        raise ValueError(f"edge: unknown edge mode {spec.edge}")
    if flags & ~(FLAG_NODATA | FLAG_NORMALIZE | FLAG_KEEP_MASK):
        raise ValueError(f"flags: unknown focal flags {flags:#x}")
    if not 1 <= spec.kh <= MAX_SIZE or not spec.kh & 1:
        raise ValueError(f"kh: window height {spec.kh} is not odd and in 1 ... {MAX_SIZE}")
    if not 1 <= spec.kw <= MAX_SIZE or not spec.kw & 1:
        raise ValueError(f"kw: window width {spec.kw} is not odd and in 1 ... {MAX_SIZE}")
    if spec.op == MEDIAN and spec.kh * spec.kw > MAX_MEDIAN:
        raise ValueError(f"kh, kw: a median of {spec.kh} x {spec.kw} taps, more than {MAX_MEDIAN}")
    if spec.op in (SLOPE, HILLSHADE) and (spec.kh, spec.kw) != (3, 3):
        raise ValueError(f"kh, kw: slope and hillshade take a 3 x 3 window, not {spec.kh} x {spec.kw}")
    if flags & FLAG_NORMALIZE and spec.op != CONVOLVE:
        raise ValueError(f"flags: FRA_FOCAL_NORMALIZE goes with FRA_FOCAL_CONVOLVE alone (op {spec.op})")
    if spec.op == CONVOLVE and spec.weights is None:
        raise ValueError("weights: convolve needs its weights")


def slope_params(zfactor: float = 1.0, dx: float = 1.0, dy: float = 1.0, scale: float = 1.0) -> Tuple[float, ...]:
    """The ``params`` of ``slope``: ``zfactor / (8 dx)``, ``zfactor / (8 dy)`` and the scale (1: rise / run, 100:
    percent)."""
    return (float(zfactor) / (8.0 * float(dx)), float(zfactor) / (8.0 * float(dy)), float(scale)) + (0.0,) * 5


def hillshade_params(azimuth: float = 315.0, altitude: float = 45.0, zfactor: float = 1.0, dx: float = 1.0,
                     dy: float = 1.0, scale: float = 255.0) -> Tuple[float, ...]:
    """The ``params`` of ``hillshade``: the gradient factors of :func:`slope_params`, the unit vector towards the light
    (east, north, up) for an azimuth clockwise from north and an altitude above the horizon, both in degrees, and the
    scale of the result.  The trigonometry happens here, once, on the host: the kernel and the numpy rule take the same
    doubles."""
    az, alt = math.radians(float(azimuth)), math.radians(float(altitude))
    return (float(zfactor) / (8.0 * float(dx)), float(zfactor) / (8.0 * float(dy)), math.sin(az) * math.cos(alt),
            math.cos(az) * math.cos(alt), math.sin(alt), float(scale), 0.0, 0.0)


def _window_of(out_window, h: int, w: int) -> Tuple[int, int, int, int]:
    if out_window is None:
        return 0, 0, h, w
    r, c, oh, ow = (int(v) for v in out_window)
    if oh < 1 or ow < 1 or r < 0 or c < 0 or r + oh > h or c + ow > w:
        raise ValueError(f"the output rectangle ({r}, {c}, {oh} x {ow}) is empty or not inside the source ({h} x {w})")
    return r, c, oh, ow


def focal_values(raster: np.ndarray, spec: Spec, out_window=None) -> Tuple[np.ndarray, np.ndarray]:
    """``spec`` over a ``(B, h, w)`` raster up to the conversion: ``(the f64 results (B, out_h, out_w), which pixels get
    fill instead)``.  :func:`finish` turns them into the output; :func:`focal_arrays` is the two in one.

    A sum starts at -0.0, which is ``x`` for every first ``x`` (``-0.0 + x == x`` bit for bit, ``x = +-0.0`` included),
    a minimum at +inf and a maximum at -inf likewise: the rule's "starting from the first valid tap" without a case."""
    a = np.asarray(raster)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("raster must be (B, h, w) or (h, w)")
    validate(spec)
    B, h, w = a.shape
    r0, c0, oh, ow = _window_of(out_window, h, w)
    kh, kw = spec.kh, spec.kw
    ry, rx = kh // 2, kw // 2
    x = a.astype(np.float64)
    ok = ~np.isnan(x)
    if spec.nodata is not None:
        ok &= ~(x == np.float64(spec.nodata))
    pad = ((0, 0), (ry, ry), (rx, rx))
    if spec.edge == EDGE_CLAMP:
        xp, okp = np.pad(x, pad, mode="edge"), np.pad(ok, pad, mode="edge")
    else:
        xp, okp = np.pad(x, pad, mode="constant"), np.pad(ok, pad, mode="constant", constant_values=False)

    def tap(dy, dx):
        sl = (slice(None), slice(r0 + dy, r0 + dy + oh), slice(c0 + dx, c0 + dx + ow))
        return xp[sl], okp[sl]

    shape = (B, oh, ow)
    n = np.zeros(shape, np.int64)
    filled = np.zeros(shape, bool)
    params = tuple(np.float64(v) for v in spec.params) + (np.float64(0.0),) * (8 - len(spec.params))
    with np.errstate(all="ignore"):
        if spec.op in (SLOPE, HILLSHADE):
            z = []
            for dy in range(3):
                for dx in range(3):
                    v, m = tap(dy, dx)
                    z.append(v)
                    filled |= ~m
            za, zb, zc, zd, _, zf, zg, zh, zi = z
            zx = ((zc + (zf + zf)) + zi) - ((za + (zd + zd)) + zg)
            zy = ((za + (zb + zb)) + zc) - ((zg + (zh + zh)) + zi)
            p, q = zx * params[0], zy * params[1]
            if spec.op == SLOPE:
                res = np.sqrt(p * p + q * q) * params[2]
            else:
                s = ((params[4] - p * params[2]) - q * params[3]) / np.sqrt((np.float64(1.0) + p * p) + q * q)
                res = np.where(s > 0.0, s, np.float64(0.0)) * params[5]
        elif spec.op == MEDIAN:
            vals = np.empty((kh * kw,) + shape, np.float64)
            for dy in range(kh):
                for dx in range(kw):
                    v, m = tap(dy, dx)
                    vals[dy * kw + dx] = np.where(m, v, np.inf)  # sorts last; a valid +inf beside it is the same value
                    n += m
            vals = np.sort(vals, axis=0, kind="stable")  # equal values (-0.0 == 0.0) stay in tap order
            rank = np.where(n > 0, (n - 1) // 2, 0)
            res = np.take_along_axis(vals, rank[None], axis=0)[0]
            filled = n == 0
        else:
            start = {MIN: np.inf, MAX: -np.inf}.get(spec.op, -0.0)
            acc = np.full(shape, start, np.float64)
            ws = np.full(shape, -0.0, np.float64)
            for dy in range(kh):
                for dx in range(kw):
                    v, m = tap(dy, dx)
                    if spec.op in (SUM, MEAN):
                        acc = np.where(m, acc + v, acc)
                    elif spec.op == MIN:
                        acc = np.where(m & (v < acc), v, acc)
                    elif spec.op == MAX:
                        acc = np.where(m & (v > acc), v, acc)
                    elif spec.op == CONVOLVE:
                        wt = np.float64(spec.weights[dy, dx])
                        acc = np.where(m, acc + v * wt, acc)
                        ws = np.where(m, ws + wt, ws)
                    n += m
            filled = n == 0
            if spec.op == MEAN:
                res = acc / n.astype(np.float64)
            elif spec.op == COUNT:
                res = n.astype(np.float64)
                filled = np.zeros(shape, bool)
            elif spec.op == CONVOLVE and spec.normalize:
                res = acc / ws
                filled = filled | (ws == 0.0)
            else:
                res = acc
        if spec.keep_mask:
            filled = filled | ~tap(ry, rx)[1]
    return res, filled


def finish(values: np.ndarray, filled: np.ndarray, spec: Spec, out_dtype) -> Tuple[np.ndarray, np.ndarray]:
    """The output of :func:`focal_values`' results: ``fill`` (default: that of ``out_dtype``) where ``filled``, the
    rule's conversion, and the per-band count of pixels that got fill (uint64)."""
    dt = np.dtype(out_dtype)
    if dt.name not in DTYPES:
        raise TypeError(f"unsupported output dtype {dt}")
    fill = np.float64(default_fill(dt) if spec.fill is None else spec.fill)
    return convert(np.where(filled, fill, values), dt), np.count_nonzero(filled, axis=(1, 2)).astype(np.uint64)


def focal_arrays(raster: np.ndarray, spec: Spec, out_dtype, out_window=None) -> Tuple[np.ndarray, np.ndarray]:
    """``spec`` over a ``(B, h, w)`` raster, tap by tap on f64 arrays in the rule's order: ``(the (B, out_h, out_w)
    result in out_dtype, the per-band count of pixels that got fill (uint64))``.  ``out_window`` = (row_off, col_off,
    out_h, out_w) inside the raster, default all of it.

    ``slope`` and ``hillshade`` take the taps ``a b c / d e f / g h i`` (row 0 to the north): ``zx = ((c + (f + f)) + i) -
    ((a + (d + d)) + g)``, ``zy = ((a + (b + b)) + c) - ((g + (h + h)) + i)``, ``p = zx * params[0]``, ``q = zy *
    params[1]``; slope is ``sqrt(p * p + q * q) * params[2]``, hillshade ``s = ((lz - p * lx) - q * ly) / sqrt((1.0 + p * p)
    + q * q)`` with ``(lx, ly, lz) = params[2:5]``, negative ``s`` (and NaN) to 0, times ``params[5]``; any of the nine
    taps left out gives ``fill``."""
    if np.dtype(out_dtype).name not in DTYPES:
        raise TypeError(f"unsupported output dtype {np.dtype(out_dtype)}")
    values, filled = focal_values(raster, spec, out_window)
    return finish(values, filled, spec, out_dtype)
