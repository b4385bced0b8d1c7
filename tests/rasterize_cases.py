"""Feature sets the CPU and the GPU tests of the rasterizer share (pixel coordinates; a feature is a list of rings)."""
import math

import numpy as np


def brute(features, window, values=None, fill=0, dtype=np.int32):
    """The rule of ``rasterize.rasterize_arrays`` pixel by pixel, feature by feature and edge by edge, in the same
    operations and the same order -> ``(raster, burned)``."""
    if len(window) == 2:
        window = (0, 0) + tuple(window)
    row_off, col_off, h, w = window
    values = [i + 1 for i in range(len(features))] if values is None else list(values)
    edges = []
    for feature in features:
        mine = []
        for ring in feature:
            pts = [(np.float64(p[0]), np.float64(p[1])) for p in ring]
            for i, (ax, ay) in enumerate(pts):
                bx, by = pts[(i + 1) % len(pts)]
                if ay == by:
                    continue
                mine.append((ax, ay, bx, by) if ay < by else (bx, by, ax, ay))
        edges.append(mine)
    out = np.full((h, w), fill, dtype)
    burned = 0
    for r in range(h):
        yc = np.float64(row_off + r) + np.float64(0.5)
        for c in range(w):
            xc = np.float64(col_off + c) + np.float64(0.5)
            hit = False
            for f, mine in enumerate(edges):
                n = 0
                for x0, y0, x1, y1 in mine:
                    if y0 <= yc and yc < y1:
                        t = (yc - y0) / (y1 - y0)
                        xi = x0 + t * (x1 - x0)
                        n += bool(xi > xc)
                if n & 1:
                    out[r, c] = values[f]
                    hit = True
            burned += hit
    return out, burned


def triangle(h, w):
    return [[[(0.3 * w, 0.1 * h), (0.95 * w, 0.6 * h), (0.1 * w, 0.9 * h)]]]


def basic_set(h, w):
    """A triangle, a polygon with a hole, a multipolygon, a self-overlapping bow-tie, and features partly and wholly
    outside a window of (h, w) at the origin."""
    return [
        [[(0.05 * w, 0.1 * h), (0.9 * w, 0.2 * h), (0.4 * w, 0.95 * h)]],
        [[(0.2 * w, 0.2 * h), (0.8 * w, 0.25 * h), (0.85 * w, 0.8 * h), (0.15 * w, 0.7 * h)],
         [(0.4 * w, 0.4 * h), (0.6 * w, 0.4 * h), (0.6 * w, 0.6 * h), (0.4 * w, 0.6 * h)]],
        [[(0.0, 0.0), (0.3 * w, 0.05 * h), (0.1 * w, 0.4 * h)], [(0.7 * w, 0.6 * h), (w + 3.0, 0.7 * h), (0.8 * w, h + 2.0)]],
        [[(0.1 * w, 0.5 * h), (0.9 * w, 0.9 * h), (0.9 * w, 0.5 * h), (0.1 * w, 0.9 * h)]],
        [[(-5.0, -4.0), (0.5 * w, -2.0), (0.25 * w, 0.5 * h)]],
        [[(w + 1.0, 0.0), (w + 9.0, 1.0), (w + 4.0, h + 0.0)]],
        [[(0.0, h + 0.75), (w + 0.0, h + 0.75), (0.5 * w, h + 8.0)]],
    ]


def outside_set(h, w):
    """A feature wholly left of, right of, above and below the window, then one that covers a part of it."""
    return [
        [[(-9.0, 0.0), (-1.0, 0.5 * h), (-7.0, h + 0.0)]],
        [[(w + 1.0, -3.0), (w + 70.0, 0.5 * h), (w + 4.0, h + 2.0)]],
        [[(0.0, -8.0), (w + 0.0, -6.0), (0.5 * w, -0.25)]],
        [[(0.0, h + 0.75), (w + 0.0, h + 3.0), (0.5 * w, h + 9.0)]],
        [[(0.25 * w, 0.25 * h), (0.75 * w, 0.3 * h), (0.5 * w, 0.8 * h)]],
    ]


def triangulation(h, w, nx=8, ny=6, seed=1):
    """A jittered nx x ny grid of quads over the window, its border on the window's, each quad split into two
    triangles: a partition of the window."""
    rng = np.random.default_rng(seed)
    gx = np.linspace(0.0, w, nx + 1)[None, :].repeat(ny + 1, 0)
    gy = np.linspace(0.0, h, ny + 1)[:, None].repeat(nx + 1, 1)
    gx[:, 1:-1] += rng.uniform(-0.3, 0.3, (ny + 1, nx - 1)) * w / nx
    gy[1:-1, :] += rng.uniform(-0.3, 0.3, (ny - 1, nx + 1)) * h / ny
    out = []
    for i in range(ny):
        for j in range(nx):
            a, b, c, d = [(gx[p], gy[p]) for p in ((i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j))]
            out += ([[[a, b, c]], [[a, c, d]]] if (i + j) & 1 else [[[a, b, d]], [[b, c, d]]])
    return out


def random_quads(h, w, n=300, seed=2):
    """n small quads in painter's order, some reaching past the window."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cx, cy = rng.uniform(-4.0, w + 4.0), rng.uniform(-4.0, h + 4.0)
        rx, ry = rng.uniform(1.0, 0.2 * w + 2.0), rng.uniform(1.0, 0.35 * h + 2.0)
        ang = np.sort(rng.uniform(0.0, 2.0 * math.pi, 4))
        out.append([[(cx + rx * math.cos(t), cy + ry * math.sin(t)) for t in ang]])
    return out


def star(nedges, cx, cy, r_out, r_in, phase=0.0):
    """One star polygon of ``nedges`` edges about (cx, cy): every edge crosses the rows near cy's band."""
    pts = []
    for k in range(nedges):
        t = phase + 2.0 * math.pi * k / nedges
        r = r_out if k % 2 == 0 else r_in
        pts.append((cx + r * math.cos(t), cy + r * math.sin(t)))
    return [pts]


def comb(nteeth, x0, x1, y_top, y_bot):
    """A comb of ``nteeth`` teeth between x0 and x1: 2 * nteeth + 1 edges (one level edge aside) that all cross every
    row between y_top and y_bot, so one feature's parity runs over many chunks of one band's list."""
    xs = np.linspace(x0, x1, 2 * nteeth + 1)
    pts = [(float(x), y_bot if k % 2 == 0 else y_top) for k, x in enumerate(xs)]
    return [pts + [(float(x1), y_bot + 1.0), (float(x0), y_bot + 1.0)]]
