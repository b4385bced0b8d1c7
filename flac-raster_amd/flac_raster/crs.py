"""Coordinate transforms between the three CRS families the warped reads know without a dependency: geographic WGS84
(``EPSG:4326``, x = longitude, y = latitude in degrees), Web Mercator (``EPSG:3857``) and WGS84 UTM (``EPSG:326zz``
north, ``EPSG:327zz`` south, zz = 01 .. 60).

``transformer(src, dst)`` composes the inverse formula of ``src`` and the forward formula of ``dst`` through geographic
WGS84.  UTM is the transverse Mercator by Krueger's series in the third flattening n, to n^4 with four harmonics
(Karney 2011, eqs. 7-36: truncation below 1e-7 m inside a zone).  Web Mercator is the sphere of radius a.  Datum shifts
do not exist here: every CRS is on WGS84.  Any other CRS raises ``ValueError``; pass ``coords=`` then.

``suggested_grid`` is the output grid a reprojection gets when none is asked for, after GDAL's
``GDALSuggestedWarpOutput``: the bounds of 21 points per source edge, and the resolution at which the source's
corner-to-corner diagonal keeps its pixel count.
"""

from __future__ import annotations

import math
import re
from typing import Callable, Tuple

import numpy as np

from .geo import Affine

A_WGS84 = 6378137.0
F_WGS84 = 1.0 / 298.257223563
K0, E0, N0_SOUTH = 0.9996, 500000.0, 10000000.0

_N = F_WGS84 / (2.0 - F_WGS84)
_E = math.sqrt(F_WGS84 * (2.0 - F_WGS84))
_A = A_WGS84 / (1.0 + _N) * (1.0 + _N**2 / 4.0 + _N**4 / 64.0)
_ALPHA = (_N / 2.0 - 2.0 / 3.0 * _N**2 + 5.0 / 16.0 * _N**3 + 41.0 / 180.0 * _N**4,
          13.0 / 48.0 * _N**2 - 3.0 / 5.0 * _N**3 + 557.0 / 1440.0 * _N**4,
          61.0 / 240.0 * _N**3 - 103.0 / 140.0 * _N**4,
          49561.0 / 161280.0 * _N**4)
_BETA = (_N / 2.0 - 2.0 / 3.0 * _N**2 + 37.0 / 96.0 * _N**3 - 1.0 / 360.0 * _N**4,
         1.0 / 48.0 * _N**2 + 1.0 / 15.0 * _N**3 - 437.0 / 1440.0 * _N**4,
         17.0 / 480.0 * _N**3 - 37.0 / 840.0 * _N**4,
         4397.0 / 161280.0 * _N**4)

UNKNOWN = ("{crs!r} is not one of EPSG:4326, EPSG:3857 and WGS84 UTM (EPSG:326zz / 327zz): pass coords= (for example "
           "a pyproj Transformer.transform from the output CRS to the source CRS), or use --like / --transform within "
           "one CRS")


def _f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float64) for a in arrays)


def utm_forward(lon, lat, zone: int, south: bool = False):
    """Longitude / latitude in degrees -> UTM easting / northing in metres of ``zone``."""
    lon, lat = _f64(lon, lat)
    lam = np.radians(lon - (6.0 * zone - 183.0))
    phi = np.radians(lat)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.sin(phi)
        t = np.sinh(np.arctanh(s) - _E * np.arctanh(_E * s))  # the tangent of the conformal latitude
        xi = np.arctan2(t, np.cos(lam))
        eta = np.arcsinh(np.sin(lam) / np.hypot(t, np.cos(lam)))
        x, y = xi, eta
        for j, a in enumerate(_ALPHA, start=1):
            x = x + a * np.sin(2.0 * j * xi) * np.cosh(2.0 * j * eta)
            y = y + a * np.cos(2.0 * j * xi) * np.sinh(2.0 * j * eta)
        return E0 + K0 * _A * y, (N0_SOUTH if south else 0.0) + K0 * _A * x


def utm_inverse(easting, northing, zone: int, south: bool = False):
    """UTM easting / northing in metres of ``zone`` -> longitude / latitude in degrees."""
    easting, northing = _f64(easting, northing)
    xi = (northing - (N0_SOUTH if south else 0.0)) / (K0 * _A)
    eta = (easting - E0) / (K0 * _A)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x, y = xi, eta
        for j, b in enumerate(_BETA, start=1):
            x = x - b * np.sin(2.0 * j * xi) * np.cosh(2.0 * j * eta)
            y = y - b * np.cos(2.0 * j * xi) * np.sinh(2.0 * j * eta)
        lam = np.arctan2(np.sinh(y), np.cos(x))
        tp = np.sin(x) / np.hypot(np.sinh(y), np.cos(x))  # the tangent of the conformal latitude
        tau = tp.copy() if isinstance(tp, np.ndarray) else np.float64(tp)
        e2 = _E * _E
        for _ in range(5):  # Newton on tau = tan(phi) (Karney 2011, eqs. 19-21); quadratic, two steps suffice
            sig = np.sinh(_E * np.arctanh(_E * tau / np.hypot(1.0, tau)))
            ti = tau * np.hypot(1.0, sig) - sig * np.hypot(1.0, tau)
            tau = tau + (tp - ti) / np.hypot(1.0, ti) * (1.0 + (1.0 - e2) * tau * tau) / ((1.0 - e2) * np.hypot(1.0, tau))
        return np.degrees(lam) + (6.0 * zone - 183.0), np.degrees(np.arctan(tau))


def mercator_forward(lon, lat):
    lon, lat = _f64(lon, lat)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return A_WGS84 * np.radians(lon), A_WGS84 * np.arcsinh(np.tan(np.radians(lat)))


def mercator_inverse(x, y):
    x, y = _f64(x, y)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.degrees(x / A_WGS84), np.degrees(np.arctan(np.sinh(y / A_WGS84)))


def _parse(crs) -> Tuple[str, int, bool]:
    """``("geographic" | "mercator" | "utm", zone, south)`` of a CRS string; ``ValueError`` for any other."""
    m = re.fullmatch(r"\s*EPSG:(\d+)\s*", str(crs), re.I)
    code = int(m.group(1)) if m else -1
    if code == 4326:
        return "geographic", 0, False
    if code == 3857:
        return "mercator", 0, False
    if 32601 <= code <= 32660 or 32701 <= code <= 32760:
        return "utm", code % 100, code >= 32700
    raise ValueError(UNKNOWN.format(crs=str(crs)))


def transformer(src_crs, dst_crs) -> Callable:
    """``f(x, y) -> (x', y')`` over arrays: coordinates of ``src_crs`` to coordinates of ``dst_crs``."""
    s, d = _parse(src_crs), _parse(dst_crs)

    def to_geographic(x, y):
        if s[0] == "utm":
            return utm_inverse(x, y, s[1], s[2])
        return mercator_inverse(x, y) if s[0] == "mercator" else _f64(x, y)

    def f(x, y):
        if s == d:
            return _f64(x, y)
        lon, lat = to_geographic(x, y)
        if d[0] == "utm":
            return utm_forward(lon, lat, d[1], d[2])
        return mercator_forward(lon, lat) if d[0] == "mercator" else (lon, lat)

    return f


def suggested_grid(src_transform, src_shape, coords_to_dst: Callable, edge_points: int = 21):
    """``(transform, (height, width))`` of the output grid a reprojection of a ``src_shape`` = (h, w) raster with
    ``src_transform`` gets: north-up, square pixels, covering the bounds of ``edge_points`` points per source edge
    under ``coords_to_dst`` (source CRS -> output CRS), at the resolution that keeps the pixel count of the source's
    diagonal."""
    h, w = (int(v) for v in tuple(src_shape)[-2:])
    t = Affine(*tuple(src_transform)[:6])
    s = np.linspace(0.0, 1.0, int(edge_points))
    cols = np.concatenate([s * w, np.full_like(s, w), s * w, np.zeros_like(s)])
    rows = np.concatenate([np.zeros_like(s), s * h, np.full_like(s, h), s * h])
    x, y = coords_to_dst(t.a * cols + t.b * rows + t.c, t.d * cols + t.e * rows + t.f)
    x, y = _f64(x, y)
    ok = np.isfinite(x) & np.isfinite(y)
    if not ok.any():
        raise ValueError("no point of the source's edge has coordinates in the output CRS")
    xmin, xmax, ymin, ymax = float(x[ok].min()), float(x[ok].max()), float(y[ok].min()), float(y[ok].max())
    res = math.hypot(xmax - xmin, ymax - ymin) / math.hypot(w, h)
    ow, oh = max(1, int((xmax - xmin) / res + 0.5)), max(1, int((ymax - ymin) / res + 0.5))
    return Affine(res, 0.0, xmin, 0.0, -res, ymax), (oh, ow)
