"""Rasterizing polygons: the rule of ``fra_rasterize`` (include/flac_raster_amd.h) in numpy, and the GeoJSON reader.

All arithmetic is IEEE f64, every operation rounded on its own.

* A feature is a list of rings, a ring a list of at least 3 vertices ``(x, y)`` in pixel coordinates of the raster the
  output window belongs to (x along columns, y along rows).  Exterior rings, holes and the parts of a multipolygon are
  not told apart.  Every feature carries an integer burn value.
* Pixel ``(r, c)`` of the window ``(row_off, col_off, h, w)`` has the centre ``xc = (col_off + c) + 0.5``,
  ``yc = (row_off + r) + 0.5``.
* Edges: a ring is closed implicitly (last -> first); an edge with ``y0 == y1`` is dropped; every other edge is
  oriented so that ``y0 < y1``, its endpoints swapped if need be before any arithmetic (two features that share an
  edge then compute the same numbers for it).
* An edge crosses the scanline of ``yc`` when ``y0 <= yc < y1``; then ``t = (yc - y0) / (y1 - y0)``,
  ``xi = x0 + t * (x1 - x0)``, and the edge counts for the pixel when ``xi > xc``.
* A feature covers the pixel when an odd number of its edges count, over all its rings together (even-odd).
* The pixel's value is the burn value of the covering feature with the highest index (painter's order); without one
  it is ``fill``.  ``burned`` is the number of pixels covered by at least one feature.
* The output dtype is one of the six zone dtypes of the zonal statistics; every burn value and ``fill`` must be
  representable in it.
"""

from __future__ import annotations

import json
import math
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .zonal import ZONE_DTYPES

MAX_SIDE = 65536         # of the output window, per axis
MAX_FEATURES = 1 << 24
MAX_VERTS = 1 << 28
MAX_COORD = float(1 << 52)
BAND_ROWS = 16           # rows per band of the native edge lists (and of the numpy rule's working set)


def window_of(window_or_shape) -> Tuple[int, int, int, int]:
    """``(row_off, col_off, h, w)`` of a window, or of a shape ``(h, w)`` at the origin."""
    v = [int(x) for x in window_or_shape]
    if len(v) == 2:
        v = [0, 0] + v
    if len(v) != 4:
        raise ValueError("give a shape (h, w) or a window (row_off, col_off, h, w)")
    if not (1 <= v[2] <= MAX_SIDE and 1 <= v[3] <= MAX_SIDE):
        raise ValueError(f"the output size must be 1 .. {MAX_SIDE} in each dimension (got {v[2]} x {v[3]})")
    return v[0], v[1], v[2], v[3]


def flatten(features):
    """The features as the three arrays ``fra_rasterize`` takes: ``(xy (nverts, 2) f64, ring_start (nrings + 1) i64,
    feature_ring_start (nfeatures + 1) i64)``.  Refuses a ring of fewer than 3 vertices, a coordinate that is not
    finite or of magnitude above 2^52, and more features or vertices than the entry takes."""
    rings, ring_start, feat_start = [], [0], [0]
    for f, feature in enumerate(features):
        for ring in feature:
            a = np.asarray(ring, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != 2:
                raise ValueError(f"feature {f}: a ring must be (n, 2) coordinates, got {a.shape}")
            if a.shape[0] < 3:
                raise ValueError(f"feature {f}: a ring of {a.shape[0]} vertices (at least 3 are needed)")
            if not np.isfinite(a).all() or (np.abs(a) > MAX_COORD).any():
                raise ValueError(f"feature {f}: a coordinate is not finite or above 2^52 in magnitude")
            rings.append(a)
            ring_start.append(ring_start[-1] + a.shape[0])
        feat_start.append(len(rings))
    if len(feat_start) - 1 > MAX_FEATURES:
        raise ValueError(f"{len(feat_start) - 1} features: at most 2^24 go into one call")
    if ring_start[-1] > MAX_VERTS:
        raise ValueError(f"{ring_start[-1]} vertices: at most 2^28 go into one call")
    xy = np.concatenate(rings) if rings else np.zeros((0, 2), np.float64)
    return np.ascontiguousarray(xy), np.asarray(ring_start, np.int64), np.asarray(feat_start, np.int64)


def burn_values(values, nfeatures: int, fill, dtype) -> Tuple[np.ndarray, int, np.dtype]:
    """``(values (nfeatures) i64, fill, dtype)`` checked: the dtype is one of the six, and holds every value and the
    fill.  ``values=None``: feature ``i`` burns ``i + 1``."""
    dt = np.dtype(dtype)
    if dt not in ZONE_DTYPES:
        raise ValueError(f"the output dtype must be one of {', '.join(t.name for t in ZONE_DTYPES)}, got {dt}")
    vals = [i + 1 for i in range(nfeatures)] if values is None else [_integer(v, "burn value") for v in values]
    if len(vals) != nfeatures:
        raise ValueError(f"{len(vals)} burn values for {nfeatures} features")
    fill = _integer(fill, "fill")
    info = np.iinfo(dt)
    for what, v in [("fill", fill)] + [("burn value", v) for v in vals]:
        if not info.min <= v <= info.max:
            raise ValueError(f"{what} {v} is not a value of {dt}")
    return np.asarray(vals, np.int64).reshape(nfeatures), fill, dt


def _integer(v, what: str) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        if isinstance(v, (float, np.floating)) and float(v) == int(v):
            return int(v)
        raise ValueError(f"{what} {v!r} is not an integer")
    return int(v)


def edge_table(features):
    """The canonical edges of the features, in feature, ring and vertex order: ``(x0, y0, x1, y1, feature)`` arrays
    (f64, and int32 for the feature index) with ``y0 < y1`` everywhere."""
    xy, ring_start, feat_start = flatten(features)
    return _edges(xy, ring_start, feat_start)


def _edges(xy, ring_start, feat_start):
    n = xy.shape[0]
    nxt = np.arange(1, n + 1, dtype=np.int64)
    nxt[ring_start[1:] - 1] = ring_start[:-1]  # the last vertex of a ring goes back to its first
    ring_of = np.repeat(np.arange(ring_start.size - 1), np.diff(ring_start))
    feat_of_ring = np.repeat(np.arange(feat_start.size - 1), np.diff(feat_start))
    feat = feat_of_ring[ring_of].astype(np.int32) if n else np.zeros(0, np.int32)
    ax, ay, bx, by = xy[:, 0], xy[:, 1], xy[nxt, 0], xy[nxt, 1]
    keep = ay != by
    swap = ay > by
    x0, y0 = np.where(swap, bx, ax), np.where(swap, by, ay)
    x1, y1 = np.where(swap, ax, bx), np.where(swap, ay, by)
    return x0[keep], y0[keep], x1[keep], y1[keep], feat[keep]


def rasterize_arrays(features, window_or_shape, values=None, fill=0, dtype=np.int32):
    """The rule above -> ``(raster (h, w) of dtype, burned)``.

    ``features``: a list of features, each a list of rings, each ``(n, 2)`` pixel coordinates.  ``window_or_shape``:
    ``(h, w)`` or ``(row_off, col_off, h, w)``.  ``values``: one integer per feature (default ``i + 1``)."""
    row_off, col_off, h, w = window_of(window_or_shape)
    features = list(features)
    vals, fill, dt = burn_values(values, len(features), fill, dtype)
    x0, y0, x1, y1, feat = edge_table(features)
    out = np.full((h, w), fill, dtype=dt)
    burned = 0
    xc = (np.arange(w, dtype=np.int64) + col_off).astype(np.float64) + 0.5
    for r0 in range(0, h, BAND_ROWS):
        r1 = min(r0 + BAND_ROWS, h)
        yc = (np.arange(r0, r1, dtype=np.int64) + row_off).astype(np.float64) + 0.5
        hit = (y0 <= yc[-1]) & (yc[0] < y1)
        if not hit.any():
            continue
        ex0, ey0, ex1, ey1, ef = x0[hit], y0[hit], x1[hit], y1[hit], feat[hit]
        cross = (ey0[None, :] <= yc[:, None]) & (yc[:, None] < ey1[None, :])
        t = (yc[:, None] - ey0[None, :]) / (ey1 - ey0)[None, :]
        xi = ex0[None, :] + t * (ex1 - ex0)[None, :]
        # the edge counts for the pixels with xc < xi: the first k of the row, k the number of centres below xi
        k = np.searchsorted(xc, xi.ravel(), side="left").reshape(xi.shape)
        present, slot = np.unique(ef, return_inverse=True)
        rows, edges = np.nonzero(cross & (k > 0))
        if rows.size == 0:
            continue
        hist = np.zeros((r1 - r0, present.size, w + 1), np.int32)
        np.add.at(hist, (rows, slot[edges], k[rows, edges]), 1)
        # pixel c is counted by the crossings with k > c
        count = hist[:, :, ::-1].cumsum(axis=2)[:, :, ::-1][:, :, 1:]
        cover = (count & 1).astype(bool)
        any_cover = cover.any(axis=1)
        last = present.size - 1 - np.argmax(cover[:, ::-1, :], axis=1)  # the covering feature with the highest index
        band = out[r0:r1]
        band[any_cover] = vals[present[last[any_cover]]].astype(dt)
        burned += int(np.count_nonzero(any_cover))
    return out, burned


# ------------------------------------------------------------------------------------------ GeoJSON
def _polygon_rings(coords, where: str) -> List[np.ndarray]:
    rings = []
    for ring in coords:
        a = np.asarray([p[:2] for p in ring], dtype=np.float64)
        if a.ndim != 2 or a.shape[0] < 3:
            raise ValueError(f"{where}: a ring of fewer than 3 positions")
        rings.append(a)
    return rings


def _geometry_rings(geom, where: str) -> List[np.ndarray]:
    kind = geom.get("type") if isinstance(geom, dict) else None
    if kind == "Polygon":
        return _polygon_rings(geom["coordinates"], where)
    if kind == "MultiPolygon":
        return [r for poly in geom["coordinates"] for r in _polygon_rings(poly, where)]
    raise ValueError(f"{where}: geometry type {kind!r} is not rasterized (Polygon and MultiPolygon are)")


def read_geojson(path_or_dict, attribute: Optional[str] = None):
    """A GeoJSON ``FeatureCollection``, ``Feature``, ``Polygon`` or ``MultiPolygon`` (a path or the parsed object) ->
    ``(features in the file's coordinates, values)``.  Without ``attribute`` feature ``i`` gets ``i + 1``; with it the
    property of that name, which must be an integer for every feature.  Any other geometry type raises
    ``ValueError`` naming it."""
    doc = path_or_dict if isinstance(path_or_dict, dict) else json.loads(Path(path_or_dict).read_text())
    kind = doc.get("type")
    if kind == "FeatureCollection":
        items = list(doc.get("features") or [])
    elif kind == "Feature":
        items = [doc]
    else:
        items = [{"type": "Feature", "geometry": doc, "properties": {}}]
    features, values = [], []
    for i, item in enumerate(items):
        where = f"feature {i}"
        if not isinstance(item, dict) or item.get("type") != "Feature":
            raise ValueError(f"{where}: not a GeoJSON Feature")
        features.append(_geometry_rings(item.get("geometry"), where))
        if attribute is None:
            values.append(i + 1)
            continue
        v = (item.get("properties") or {}).get(attribute)
        if isinstance(v, bool) or not (isinstance(v, int) or (isinstance(v, float) and math.isfinite(v) and v == int(v))):
            raise ValueError(f"{where}: property {attribute!r} is {v!r}, not an integer")
        values.append(int(v))
    return features, values


def to_pixel(features, transform):
    """World coordinates -> pixel coordinates through the inverse of a ``geo.Affine`` (or its six coefficients), in
    numpy f64: ``col = (e dx - b dy) / det``, ``row = (a dy - d dx) / det`` with ``dx = x - c``, ``dy = y - f``,
    ``det = a e - b d``.  The host rule and the GPU entry are given these same numbers."""
    a, b, c, d, e, f = (float(v) for v in tuple(transform)[:6])
    det = a * e - b * d
    if det == 0.0 or not math.isfinite(det):
        raise ValueError("the transform cannot be inverted")
    out = []
    for feature in features:
        rings = []
        for ring in feature:
            p = np.asarray(ring, dtype=np.float64)
            dx, dy = p[:, 0] - c, p[:, 1] - f
            rings.append(np.stack([(e * dx - b * dy) / det, (a * dy - d * dx) / det], axis=1))
        out.append(rings)
    return out
