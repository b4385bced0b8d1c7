"""Warped reads: a raster onto an output grid of its own -- the rule of ``k_warp``, stated in numpy.

``warp_arrays`` is the host path of ``streaming.warp_window(cpu=True)`` and the expectation the GPU kernel
(``fra_warp``, ``fra_decode_device_warped``; ``include/flac_raster_amd.h``, "Warped reads") is tested against, bit for
bit.  ``warp_pixel`` says the same in a scalar loop over Python floats and is what ``warp_arrays`` is checked against.

All coordinate and value arithmetic is IEEE float64, each operation rounded on its own.  Pixel ``(row r, col c)``
covers ``[c, c + 1) x [r, r + 1)``; its centre is ``(c + 0.5, r + 0.5)``.

Maps.  For output pixel ``(R, C)``: ``u = float(C) + 0.5``, ``v = float(R) + 0.5``.

``affine``  six floats ``a .. f``: ``x = (a*u + b*v) + c``, ``y = (d*u + e*v) + f``, in exactly this order.
``grid``    ``step >= 1``, ``gw = ceil(ow / step) + 1``, ``gh = ceil(oh / step) + 1`` and two float64 planes ``gx, gy`` of
            shape ``(gh, gw)``: the source coordinates of the output-grid points ``(j*step, i*step)`` (pixel corners).
            ``cj = min(C // step, gw - 2)``, ``ci = min(R // step, gh - 2)``, ``fx = (u - float(cj*step)) /
            float(step)``, ``fy`` likewise; per plane ``top = g[ci][cj] + (g[ci][cj+1] - g[ci][cj]) * fx``, ``bot`` the
            same on row ``ci + 1``, value ``top + (bot - top) * fy``.

Inside.  ``x >= 0 and x < W and y >= 0 and y < H`` (a NaN coordinate fails).  An outside pixel is written as ``fill``
and counted.

Sampling an inside pixel.  ``nearest``: ``in[floor(y)][floor(x)]``.  ``bilinear`` / ``cubic``: ``px = x - 0.5``, ``i0 =
floor(px)``, ``t = px - i0``, rows likewise; taps, weights, clamping of the tap indices, the order (vertically first, top
to bottom, then left to right) and the conversion are those of ``resample.resample``, except that a NaN result is written
as the canonical quiet NaN (positive, no payload), so that a float output is fixed to the last bit on every machine.  With ``nodata`` the validity of a
value and the renormalisation are those of the nodata-aware resampling: all taps valid gives the unmasked formula,
otherwise the masked bilinear of the same centre; no valid tap, or ``Wt <= 0``, gives ``fill`` and the pixel is counted;
the nearest picks its pixel, invalid or not, and counts it when it is invalid.  ``average`` is refused: a warp that
shrinks takes point samples (read an overview first, then warp that).

Consequences: under the identity map the nearest returns the input bit for bit and the bilinear and the cubic every
finite value; an integer translation is a shifted copy with fill; an axis-aligned map with power-of-two scales and zero
offsets equals ``resample.resample`` (nearest, bilinear, cubic) of that size bit for bit.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from .resample import (MAX_OUT, _DTYPES, _tap_weights, check_nodata, check_out_shape, fill_value, valid_mask)

AFFINE, GRID = 0, 1
RESAMPLING = {"nearest": 0, "bilinear": 2, "cubic": 3}
MARGIN = 3  # pixels the decoded source window grows by per side
FLAG_NODATA = 1


@dataclass(frozen=True)
class Map:
    """An affine map (``affine`` = (a, b, c, d, e, f)) or a coordinate grid (``step``, ``gx``, ``gy``)."""

    kind: int
    affine: Tuple[float, ...] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    step: int = 0
    gx: Optional[np.ndarray] = None
    gy: Optional[np.ndarray] = None


def resampling_code(resampling) -> int:
    if resampling == "average":
        raise ValueError("a warp takes point samples: the average is not offered (read an overview, then warp it)")
    if resampling not in RESAMPLING:
        raise ValueError(f"resampling must be one of {tuple(RESAMPLING)}, got {resampling!r}")
    return RESAMPLING[resampling]


def grid_shape(out_shape, step: int) -> Tuple[int, int]:
    """``(gh, gw)`` of a coordinate grid for ``out_shape`` at ``step``."""
    oh, ow = check_out_shape(out_shape)
    if int(step) != step or step < 1:
        raise ValueError(f"the grid step must be an integer >= 1, got {step!r}")
    return -(-oh // int(step)) + 1, -(-ow // int(step)) + 1


def affine_coefficients(coeffs) -> Map:
    """The affine map of six finite floats ``(a, b, c, d, e, f)``: output pixel coordinates -> source pixel coordinates."""
    k = tuple(float(v) for v in tuple(coeffs)[:6])
    if len(k) != 6 or not all(math.isfinite(v) for v in k):
        raise ValueError(f"an affine map takes six finite coefficients, got {coeffs!r}")
    return Map(AFFINE, k)


def affine_map(dst_transform, src_transform) -> Map:
    """The map of an output grid with geotransform ``dst_transform`` onto a source with ``src_transform`` (both
    ``geo.Affine`` or six floats, in one CRS): the composition ``src^-1 o dst`` as six floats."""
    da, db, dc, dd, de, df = (float(v) for v in tuple(dst_transform)[:6])
    sa, sb, sc, sd, se, sf = (float(v) for v in tuple(src_transform)[:6])
    det = sa * se - sb * sd
    if det == 0.0 or not math.isfinite(det):
        raise ValueError(f"the source transform {tuple(src_transform)[:6]} has no inverse")
    ia, ib, id_, ie = se / det, -sb / det, -sd / det, sa / det  # the inverse's linear part
    ic, if_ = -(ia * sc + ib * sf), -(id_ * sc + ie * sf)
    return affine_coefficients((ia * da + ib * dd, ia * db + ib * de, ia * dc + ib * df + ic,
                                id_ * da + ie * dd, id_ * db + ie * de, id_ * dc + ie * df + if_))


def grid_map(coords: Callable, out_shape, step: int) -> Map:
    """The coordinate grid of ``coords(cols, rows) -> (src_x, src_y)`` (any callable over float64 arrays of output pixel
    coordinates) for ``out_shape`` at ``step``: ``coords`` at the grid points ``(j*step, i*step)``."""
    gh, gw = grid_shape(out_shape, step)
    cols, rows = np.meshgrid(np.arange(gw, dtype=np.float64) * float(step), np.arange(gh, dtype=np.float64) * float(step))
    sx, sy = coords(cols, rows)
    gx = np.ascontiguousarray(np.broadcast_to(np.asarray(sx, dtype=np.float64), (gh, gw)))
    gy = np.ascontiguousarray(np.broadcast_to(np.asarray(sy, dtype=np.float64), (gh, gw)))
    return Map(GRID, step=int(step), gx=gx, gy=gy)


def centre_error(m: Map, coords: Callable) -> float:
    """The largest distance, in source pixels, between the grid's interpolated coordinates and ``coords`` at the cell
    centres (cells where either is not finite are left out; 0.0 when none is left)."""
    gh, gw = m.gx.shape
    step = float(m.step)
    cols, rows = np.meshgrid((np.arange(gw - 1, dtype=np.float64) + 0.5) * step, (np.arange(gh - 1, dtype=np.float64) + 0.5) * step)
    tx, ty = coords(cols, rows)
    with np.errstate(invalid="ignore", over="ignore"):
        def mid(g):
            top = g[:-1, :-1] + (g[:-1, 1:] - g[:-1, :-1]) * 0.5
            bot = g[1:, :-1] + (g[1:, 1:] - g[1:, :-1]) * 0.5
            return top + (bot - top) * 0.5
        d = np.hypot(mid(m.gx) - np.asarray(tx, np.float64), mid(m.gy) - np.asarray(ty, np.float64))
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


def fit_grid(coords: Callable, out_shape, max_error: float = 0.125, first_step: int = 16) -> Tuple[Map, float]:
    """The coarsest grid, from step 16 down by halving, whose interpolated coordinates at the cell centres lie within
    ``max_error`` source pixels of ``coords`` (step 1 is taken as it is); returns ``(map, error reached)``.  0.125 px is
    GDAL's default error threshold: a parameter, not a finding."""
    step = int(first_step)
    while True:
        m = grid_map(coords, out_shape, step)
        err = centre_error(m, coords)
        if err <= max_error or step == 1:
            return m, err
        step //= 2


def check_map(m: Map, out_shape) -> Tuple[int, int]:
    oh, ow = check_out_shape(out_shape)
    if m.kind == AFFINE:
        if len(m.affine) != 6 or not all(math.isfinite(v) for v in m.affine):
            raise ValueError("an affine map takes six finite coefficients")
    elif m.kind == GRID:
        want = grid_shape((oh, ow), m.step)
        for g in (m.gx, m.gy):
            if not (isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == want and g.flags.c_contiguous):
                raise ValueError(f"a {oh} x {ow} output at step {m.step} takes contiguous float64 planes of {want}")
    else:
        raise ValueError(f"unknown map kind {m.kind!r}")
    return oh, ow


def map_coords(m: Map, out_shape, out_window=None) -> Tuple[np.ndarray, np.ndarray]:
    """``(x, y)``, each ``(oh, ow)`` float64: the source coordinates of every output pixel, by the rule's operations;
    with ``out_window`` = (row, col, height, width) those of that rectangle of the output only."""
    oh, ow = check_map(m, out_shape)
    R0, C0, wh, ww = (0, 0, oh, ow) if out_window is None else (int(v) for v in out_window)
    if R0 < 0 or C0 < 0 or wh < 1 or ww < 1 or R0 + wh > oh or C0 + ww > ow:
        raise ValueError(f"the output window {out_window!r} is empty or not inside the {oh} x {ow} output")
    u = np.arange(C0, C0 + ww, dtype=np.float64) + 0.5
    v = np.arange(R0, R0 + wh, dtype=np.float64) + 0.5
    with np.errstate(invalid="ignore", over="ignore"):
        if m.kind == AFFINE:
            a, b, c, d, e, f = (np.float64(k) for k in m.affine)
            return (a * u[None, :] + b * v[:, None]) + c, (d * u[None, :] + e * v[:, None]) + f
        gh, gw = m.gx.shape
        cj = np.minimum(np.arange(C0, C0 + ww, dtype=np.int64) // m.step, gw - 2)
        ci = np.minimum(np.arange(R0, R0 + wh, dtype=np.int64) // m.step, gh - 2)
        fx = ((u - (cj * m.step).astype(np.float64)) / np.float64(m.step))[None, :]
        fy = ((v - (ci * m.step).astype(np.float64)) / np.float64(m.step))[:, None]
        out = []
        for g in (m.gx, m.gy):
            g00, g01 = g[ci[:, None], cj[None, :]], g[ci[:, None], cj[None, :] + 1]
            g10, g11 = g[ci[:, None] + 1, cj[None, :]], g[ci[:, None] + 1, cj[None, :] + 1]
            top = g00 + (g01 - g00) * fx
            bot = g10 + (g11 - g10) * fx
            out.append(top + (bot - top) * fy)
        return out[0], out[1]


def source_window(m: Map, raster_shape, out_shape):
    """The source window ``(row_off, col_off, height, width)`` the warped read decodes, or ``None`` when the map's
    footprint misses the raster: the hull of the coordinates (affine: of the four corner pixel centres; grid: of the nodes
    where both planes are finite), ``floor(min) - 3 .. floor(max) + 3`` per axis, clipped to the raster; ``None`` when the
    hull misses ``[0, W) x [0, H)`` by more than a pixel.  The same arithmetic as ``fra_warp_source_window``."""
    oh, ow = check_map(m, out_shape)
    H, W = (int(v) for v in tuple(raster_shape)[-2:])
    if m.kind == AFFINE:
        a, b, c, d, e, f = m.affine
        pts = [((a * u + b * v) + c, (d * u + e * v) + f) for v in (0.5, float(oh) - 0.5) for u in (0.5, float(ow) - 0.5)]
        xs, ys = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    else:
        xs, ys = m.gx.reshape(-1), m.gy.reshape(-1)
    ok = np.isfinite(xs) & np.isfinite(ys)
    if not ok.any():
        return None
    xmin, xmax, ymin, ymax = xs[ok].min(), xs[ok].max(), ys[ok].min(), ys[ok].max()
    if not (xmax >= -1.0 and xmin < W + 1.0 and ymax >= -1.0 and ymin < H + 1.0):
        return None
    c0, c1 = max(math.floor(xmin) - MARGIN, 0), min(math.floor(xmax) + MARGIN, W - 1)
    r0, r1 = max(math.floor(ymin) - MARGIN, 0), min(math.floor(ymax) + MARGIN, H - 1)
    return int(r0), int(c0), int(r1 - r0 + 1), int(c1 - c0 + 1)


def check_values(dtype, nodata, fill) -> Tuple[Optional[float], float]:
    """``(nodata, fill)`` as the floats the rule admits for ``dtype`` (``ValueError`` otherwise).  ``fill=None``: the
    nodata value, or without one NaN for floats and 0 for integers."""
    from .calc import default_fill

    nd = None if nodata is None else check_nodata(nodata, dtype)
    if fill is None:
        return nd, (nd if nd is not None else default_fill(dtype))
    try:
        return nd, check_nodata(fill, dtype)
    except ValueError as e:
        raise ValueError(str(e).replace("nodata", "fill", 1)) from None


def _convert(v: np.ndarray, dt) -> np.ndarray:
    if dt.kind == "f":
        return np.where(v != v, np.float64("nan"), v).astype(dt)  # a NaN result: the canonical quiet NaN
    info = np.iinfo(dt)
    return np.clip(np.rint(v), np.float64(info.min), np.float64(info.max)).astype(dt)


def _sample(a: np.ndarray, x: np.ndarray, y: np.ndarray, mode: int, nd, fillv, place):
    """The values ``(B, n)`` of the ``n`` inside pixels at ``(x, y)`` and which of them are counted ``(B, n)``.
    ``place`` = (r0, c0, H, W): ``a`` is the window at (r0, c0) of an H x W raster; tap indices are clamped to the raster
    and then taken relative to the window, which must hold them."""
    r0, c0, H, W = place
    dt = a.dtype

    def rel(i, n, off, length, what):
        k = np.clip(i, 0, n - 1) - off
        if k.min() < 0 or k.max() >= length:
            raise ValueError(f"the window at ({r0}, {c0}) of {a.shape[1]} x {a.shape[2]} does not hold the {what} the map "
                             f"needs ({int(k.min()) + off} .. {int(k.max()) + off})")
        return k

    if mode == 0:
        out = a[:, rel(np.floor(y).astype(np.int64), H, r0, a.shape[1], "rows"),
                rel(np.floor(x).astype(np.int64), W, c0, a.shape[2], "columns")]
        return out, (~valid_mask(out, nd) if nd is not None else np.zeros(out.shape, bool))
    px, py = x - 0.5, y - 0.5
    fx, fy = np.floor(px), np.floor(py)
    tx, ty = px - fx, py - fy
    i0x, i0y = fx.astype(np.int64), fy.astype(np.int64)
    off, nt = (0, 2) if mode == 2 else (-1, 4)
    rows = [rel(i0y + off + k, H, r0, a.shape[1], "rows") for k in range(nt)]
    cols = [rel(i0x + off + k, W, c0, a.shape[2], "columns") for k in range(nt)]
    xf = a.astype(np.float64)
    wy, wx = _tap_weights(ty, mode), _tap_weights(tx, mode)
    v = None
    for i in range(nt):
        c = None
        for j in range(nt):  # vertically first, top to bottom
            term = xf[:, rows[j], cols[i]] * wy[j][None, :]
            c = term if j == 0 else c + term
        term = c * wx[i][None, :]  # then left to right
        v = term if i == 0 else v + term
    if nd is None:
        return _convert(v, dt), np.zeros(v.shape, bool)
    valid = valid_mask(a, nd)
    all_ok = np.ones(v.shape, bool)
    for j in range(nt):
        for i in range(nt):
            all_ok &= valid[:, rows[j], cols[i]]
    # the masked bilinear of the same centre
    brows = [rel(i0y + k, H, r0, a.shape[1], "rows") for k in range(2)]
    bcols = [rel(i0x + k, W, c0, a.shape[2], "columns") for k in range(2)]
    bwy, bwx = (1.0 - ty, ty), (1.0 - tx, tx)
    vm, wt, seen = np.zeros(v.shape), np.zeros(v.shape), np.zeros(v.shape, bool)
    for i in range(2):
        c, u, have = np.zeros(v.shape), np.zeros(v.shape), np.zeros(v.shape, bool)
        for j in range(2):
            ok = valid[:, brows[j], bcols[i]]
            term = xf[:, brows[j], bcols[i]] * bwy[j][None, :]
            wk = np.broadcast_to(bwy[j][None, :], term.shape)
            c = np.where(ok, np.where(have, c + term, term), c)
            u = np.where(ok, np.where(have, u + wk, wk), u)
            have = have | ok
        tc, tu = c * bwx[i][None, :], u * bwx[i][None, :]
        vm = np.where(have, np.where(seen, vm + tc, tc), vm)
        wt = np.where(have, np.where(seen, wt + tu, tu), wt)
        seen = seen | have
    filled = ~all_ok & (~seen | (wt <= 0.0))
    q = np.where(all_ok, v, vm / np.where(wt > 0.0, wt, 1.0))
    out = _convert(np.where(filled, 0.0, q), dt)
    out[filled] = fillv
    return out, filled


def _check_raster(raster) -> np.ndarray:
    a = np.asarray(raster)
    if a.ndim != 3 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"expected a (B, h, w) raster with h, w >= 1, got shape {a.shape}")
    if a.dtype.newbyteorder("=") not in _DTYPES:
        raise TypeError(f"unsupported dtype {a.dtype}")
    return a


def warp_arrays(raster: np.ndarray, out_shape, m: Map, resampling: str = "bilinear", nodata=None, fill=None,
                origin: Sequence[int] = (0, 0), raster_shape=None, out_window=None):
    """``raster`` ``(B, h, w)`` warped onto ``out_shape`` = (oh, ow) through ``m`` (the module's rule): ``(out, filled)``,
    the ``(B, oh, ow)`` output in the input's dtype and per band the number of pixels counted (``uint64``).

    ``origin`` / ``raster_shape``: ``raster`` is the window at ``origin`` = (row, col) of a whole raster of
    ``raster_shape`` = (H, W) that holds every tap the map needs (``source_window``); the result is that of the whole
    raster.  ``out_window`` = (row, col, height, width): that rectangle of the output only (its crop, and its counts)."""
    a = _check_raster(raster)
    mode = resampling_code(resampling)
    oh, ow = check_map(m, out_shape)
    dt = a.dtype
    nd, fl = check_values(dt, nodata, fill)
    fillv = fill_value(fl, dt)
    B, h, w = a.shape
    r0, c0 = (int(v) for v in origin)
    H, W = (int(v) for v in raster_shape) if raster_shape is not None else (r0 + h, c0 + w)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x, y = map_coords(m, (oh, ow), out_window)
        oh, ow = x.shape
        out = np.full((B, oh * ow), fillv, dt)
        counted = np.ones((B, oh * ow), bool)
        x, y = x.reshape(-1), y.reshape(-1)
        inside = (x >= 0.0) & (x < np.float64(W)) & (y >= 0.0) & (y < np.float64(H))
        idx = np.flatnonzero(inside)
        if idx.size:
            vals, cnt = _sample(a, x[idx], y[idx], mode, nd, fillv, (r0, c0, H, W))
            out[:, idx] = vals
            counted[:, idx] = cnt
    return out.reshape(B, oh, ow), counted.sum(axis=1).astype(np.uint64)


def warp_pixel(raster: np.ndarray, out_shape, m: Map, resampling: str = "bilinear", nodata=None, fill=None):
    """The same as ``warp_arrays``, pixel by pixel over Python floats: the check of the vectorised rule, nothing else."""
    a = _check_raster(raster)
    mode = resampling_code(resampling)
    oh, ow = check_map(m, out_shape)
    dt = a.dtype
    nd, fl = check_values(dt, nodata, fill)
    fillv = fill_value(fl, dt)
    B, H, W = a.shape
    is_float = dt.kind == "f"
    ndv = None if nd is None else fill_value(nd, dt)

    def bad(p):
        return nd is not None and (bool(p == ndv) or (is_float and bool(p != p)))

    def conv(v):
        if is_float:
            with np.errstate(over="ignore", invalid="ignore"):
                return dt.type(math.nan if v != v else v)
        info = np.iinfo(dt)
        return dt.type(min(max(round(v), info.min), info.max))

    def weights(t):
        if mode == 2:
            return [1.0 - t, t]
        return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
                ((0.5 * t - 0.5) * t) * t]

    def coords(R, C):
        u, v = float(C) + 0.5, float(R) + 0.5
        if m.kind == AFFINE:
            ka, kb, kc, kd, ke, kf = m.affine
            return (ka * u + kb * v) + kc, (kd * u + ke * v) + kf
        gh, gw = m.gx.shape
        cj, ci = min(C // m.step, gw - 2), min(R // m.step, gh - 2)
        fx, fy = (u - float(cj * m.step)) / float(m.step), (v - float(ci * m.step)) / float(m.step)
        res = []
        for g in (m.gx, m.gy):
            g00, g01, g10, g11 = float(g[ci, cj]), float(g[ci, cj + 1]), float(g[ci + 1, cj]), float(g[ci + 1, cj + 1])
            top = g00 + (g01 - g00) * fx
            bot = g10 + (g11 - g10) * fx
            res.append(top + (bot - top) * fy)
        return res[0], res[1]

    out = np.empty((B, oh, ow), dt)
    filled = np.zeros(B, np.uint64)
    with np.errstate(invalid="ignore", over="ignore"):
        for R in range(oh):
            for C in range(ow):
                x, y = coords(R, C)
                if not (x >= 0.0 and x < float(W) and y >= 0.0 and y < float(H)):
                    out[:, R, C] = fillv
                    filled += np.uint64(1)
                    continue
                if mode == 0:
                    r, c = math.floor(y), math.floor(x)
                    for b in range(B):
                        out[b, R, C] = a[b, r, c]
                        if bad(a[b, r, c]):
                            filled[b] += np.uint64(1)
                    continue
                px, py = x - 0.5, y - 0.5
                i0x, i0y = math.floor(px), math.floor(py)
                tx, ty = px - float(i0x), py - float(i0y)
                off, nt = (0, 2) if mode == 2 else (-1, 4)
                rows = [min(max(i0y + off + k, 0), H - 1) for k in range(nt)]
                cols = [min(max(i0x + off + k, 0), W - 1) for k in range(nt)]
                wy, wx = weights(ty), weights(tx)
                for b in range(B):
                    taps = [[a[b, r, c] for c in cols] for r in rows]
                    if not any(bad(p) for row in taps for p in row):
                        v = None
                        for i in range(nt):
                            c_ = None
                            for j in range(nt):
                                term = float(taps[j][i]) * wy[j]
                                c_ = term if j == 0 else c_ + term
                            term = c_ * wx[i]
                            v = term if i == 0 else v + term
                        out[b, R, C] = conv(v)
                        continue
                    br = [min(max(i0y + k, 0), H - 1) for k in range(2)]
                    bc = [min(max(i0x + k, 0), W - 1) for k in range(2)]
                    bwy, bwx = [1.0 - ty, ty], [1.0 - tx, tx]
                    v = wt = None
                    for i in range(2):
                        c_ = u_ = None
                        for j in range(2):
                            p = a[b, br[j], bc[i]]
                            if bad(p):
                                continue
                            term = float(p) * bwy[j]
                            c_ = term if c_ is None else c_ + term
                            u_ = bwy[j] if u_ is None else u_ + bwy[j]
                        if c_ is None:
                            continue
                        cv, cu = c_ * bwx[i], u_ * bwx[i]
                        v = cv if v is None else v + cv
                        wt = cu if wt is None else wt + cu
                    if v is None or wt <= 0.0:
                        out[b, R, C] = fillv
                        filled[b] += np.uint64(1)
                    else:
                        out[b, R, C] = conv(v / wt)
    return out, filled
