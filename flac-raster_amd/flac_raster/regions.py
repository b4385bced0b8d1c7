"""Regions: the connected components of a raster's foreground, their areas and boxes, and a sieve.

The rule of ``fra_regions`` (``include/flac_raster_amd.h``, "Regions") restated in numpy, twice:

* :func:`regions_direct` is the definition: a flood fill from each unvisited foreground pixel in raster order;
* :func:`regions_arrays` is a run-based union-find: the runs of every row, united across the links between rows.

The rule, per band of a ``(B, h, w)`` raster with ``1 <= h, w <= 32768``:

* **Foreground**: the targets of the proximity rule (:func:`flac_raster.proximity.targets_of`): without ``values`` a
  pixel that is non-zero and not NaN, with 1 .. 16 ``values`` one that equals one of them as float64.  ``invert`` swaps
  foreground and background after that test; a NaN stays background.
* **Links**: ``connectivity`` 4 or 8.  Two neighbouring foreground pixels are linked; with ``by_value`` only if their
  values are equal under ``==`` in the source dtype.  A component is a class of the transitive closure of the links.
  Pixels outside the raster do not exist, so a window of a raster labels the window: a component is cut at its edge.
* A component's **first pixel** is its pixel with the smallest ``r * w + c``, its **area** its pixel count, its **box**
  the minimum and maximum of its rows and of its columns.
* **Sieve**: a component is kept when ``area >= min_size`` (``min_size >= 1``; 1 keeps everything).
* **Numbering**: the kept components are numbered 1 .. N in the order of their first pixels; background pixels and the
  pixels of removed components have label 0.
* **Outputs**: ``labels`` (an integer dtype); ``area`` (any dtype): the area of the pixel's kept component, 0 elsewhere,
  converted as the band math converts a result; ``sieved`` (the source's dtype): the source, except that the pixels of
  removed components get ``sieve_fill``; a table per band, record ``i - 1`` for component ``i``; and per band the
  counts ``[foreground pixels, components before the sieve, kept components, pixels of kept components]``.

The GPU results equal both functions byte for byte.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from .calc import convert
from .proximity import targets_of

MAX_SIDE = 32768
MAX_VALUES = 16
TILE = 64           # the side of the tile a workgroup labels (csrc/fra_regions.h: kTile)
MAX_ZONES = 65536   # the most components `zonal` takes as zones in one call
REC = np.dtype([("first", "<u4"), ("area", "<u4"), ("rmin", "<i4"), ("cmin", "<i4"), ("rmax", "<i4"), ("cmax", "<i4")])
assert REC.itemsize == 24


@dataclass(frozen=True)
class Options:
    """What a regions call is asked for.

    ``values``: the foreground values (at most 16); empty: every pixel that is non-zero and not NaN.  ``invert``: swap
    foreground and background (a NaN stays background).  ``by_value``: link only equal neighbours.  ``connectivity``: 4
    or 8.  ``min_size``: the smallest area a component is kept at.  ``sieve_fill``: what the pixels of removed components
    get in ``sieved``."""

    values: Tuple[float, ...] = ()
    invert: bool = False
    by_value: bool = False
    connectivity: int = 4
    min_size: int = 1
    sieve_fill: float = 0.0


def validate(opts: Options) -> None:
    """``ValueError`` for options the rule refuses, in the library's order."""
    if len(opts.values) > MAX_VALUES:
        raise ValueError(f"nvalues: {len(opts.values)} foreground values (0 .. {MAX_VALUES})")
    for i, v in enumerate(opts.values):
        if not math.isfinite(float(v)):
            raise ValueError(f"values: foreground value {i} is not finite")
    if opts.connectivity not in (4, 8):
        raise ValueError(f"connectivity: {opts.connectivity} is neither 4 nor 8")
    if int(opts.min_size) < 1:
        raise ValueError(f"min_size: {opts.min_size} is below 1")


def check_region(h: int, w: int) -> None:
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"the region must be 1 .. {MAX_SIDE} in each dimension (got {h} x {w})")


def check_label_dtype(label_dtype) -> np.dtype:
    dt = np.dtype(label_dtype)
    if dt.kind not in "iu" or dt.itemsize > 4:
        raise ValueError(f"bad labels dtype {dt} (an integer dtype is needed)")
    return dt


def foreground_of(band: np.ndarray, opts: Options) -> np.ndarray:
    """The foreground mask of one band."""
    m = targets_of(band, opts.values)
    if opts.invert:
        m = ~m
        if band.dtype.kind == "f":
            m &= ~np.isnan(band)
    return m


def links_of(band: np.ndarray, fg: np.ndarray, opts: Options):
    """``(W, N, NW, NE)``: whether a pixel is linked to its neighbour in that direction (the other four follow)."""
    h, w = fg.shape

    def link(dr: int, dc: int) -> np.ndarray:
        out = np.zeros((h, w), bool)
        # the pixel (r, c) and its neighbour (r - dr, c + dc)
        r0, c0, c1 = dr, max(0, -dc), w - max(0, dc)
        if r0 >= h or c0 >= c1:
            return out
        a = (slice(r0, h), slice(c0, c1))
        b = (slice(r0 - dr, h - dr), slice(c0 + dc, c1 + dc))
        m = fg[a] & fg[b]
        if opts.by_value:
            with np.errstate(invalid="ignore"):
                m &= band[a] == band[b]
        out[a] = m
        return out

    none = np.zeros((h, w), bool)
    eight = opts.connectivity == 8
    return link(0, -1), link(1, 0), (link(1, -1) if eight else none), (link(1, 1) if eight else none)


def _as_bands(raster) -> np.ndarray:
    a = np.asarray(raster)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("raster must be (B, h, w) or (h, w)")
    return a


def _components_runs(band, fg, opts: Options) -> np.ndarray:
    """Per pixel the index of its component in the order of the first pixels, -1 for background: the runs of every row
    united across the links between rows."""
    h, w = fg.shape
    lw, ln, lnw, lne = links_of(band, fg, opts)
    start = (fg & ~lw).ravel()
    nruns = int(start.sum())
    run = np.where(fg.ravel(), np.cumsum(start) - 1, -1)  # runs do not span rows: column 0 has no W link
    pairs = []
    for m, back in ((ln, w), (lnw, w + 1), (lne, w - 1)):
        p = np.flatnonzero(m.ravel())
        if p.size:
            pairs.append(np.stack([run[p], run[p - back]], axis=1))
    parent = list(range(nruns))
    if pairs:
        uniq = np.unique(np.concatenate(pairs), axis=0)
        for a, b in uniq.tolist():
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            while parent[b] != b:
                parent[b] = parent[parent[b]]
                b = parent[b]
            if a != b:  # the larger root goes below the smaller: a root is the run of the component's first pixel
                if a < b:
                    parent[b] = a
                else:
                    parent[a] = b
    par = np.asarray(parent, dtype=np.int64)
    while True:
        nxt = par[par] if nruns else par
        if np.array_equal(nxt, par):
            break
        par = nxt
    # run ids follow their first pixels, so the roots in increasing order are the components in the rule's order
    is_root = par == np.arange(nruns)
    comp_of_run = (np.cumsum(is_root) - 1)[par] if nruns else par
    return np.where(fg.ravel(), comp_of_run[np.maximum(run, 0)] if nruns else -1, -1).reshape(h, w)


def _components_fill(band, fg, opts: Options) -> np.ndarray:
    """The same by the definition: a flood fill from each unvisited foreground pixel in raster order."""
    h, w = fg.shape
    comp = np.full((h, w), -1, np.int64)
    steps = [(0, -1), (0, 1), (-1, 0), (1, 0)]
    if opts.connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    fgl, vals = fg.tolist(), band.tolist()
    compl = [[-1] * w for _ in range(h)]
    n = 0
    for r in range(h):
        for c in range(w):
            if not fgl[r][c] or compl[r][c] >= 0:
                continue
            compl[r][c] = n
            stack = [(r, c)]
            while stack:
                y, x = stack.pop()
                v = vals[y][x]
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and fgl[yy][xx] and compl[yy][xx] < 0 and \
                            (not opts.by_value or vals[yy][xx] == v):
                        compl[yy][xx] = n
                        stack.append((yy, xx))
            n += 1
    comp[:] = np.asarray(compl, dtype=np.int64).reshape(h, w)
    return comp


def _finish(band, comp, opts: Options, label_dtype, area_dtype):
    """``(labels, area, sieved, table, counts)`` of one band from the component index of every pixel."""
    h, w = comp.shape
    flat = comp.ravel()
    fgi = np.flatnonzero(flat >= 0)
    ci = flat[fgi]
    ncomp = int(ci.max()) + 1 if ci.size else 0
    area = np.bincount(ci, minlength=ncomp).astype(np.int64)
    first = np.full(ncomp, h * w, np.int64)
    np.minimum.at(first, ci, fgi)
    rows, cols = fgi // w, fgi % w
    rmin, cmin = np.full(ncomp, 1 << 40, np.int64), np.full(ncomp, 1 << 40, np.int64)
    rmax, cmax = np.full(ncomp, -1, np.int64), np.full(ncomp, -1, np.int64)
    np.minimum.at(rmin, ci, rows), np.minimum.at(cmin, ci, cols)
    np.maximum.at(rmax, ci, rows), np.maximum.at(cmax, ci, cols)
    kept = area >= int(opts.min_size)
    number = np.where(kept, np.cumsum(kept), 0)
    n = int(kept.sum())
    ldt = np.dtype(label_dtype)
    if n > np.iinfo(ldt).max:
        raise ValueError(f"{n} components, more than the labels dtype holds ({np.iinfo(ldt).max})")
    num_px = np.where(flat >= 0, number[np.maximum(flat, 0)] if ncomp else 0, 0)
    labels = num_px.astype(ldt).reshape(h, w)
    area_px = np.where(num_px > 0, area[np.maximum(flat, 0)] if ncomp else 0, 0).astype(np.float64)
    area_out = None if area_dtype is None else convert(area_px, area_dtype).reshape(h, w)
    fill = convert(np.array([float(opts.sieve_fill)]), band.dtype)[0]
    removed = ((flat >= 0) & (num_px == 0)).reshape(h, w)
    sieved = band.copy()
    sieved[removed] = fill
    table = np.zeros(n, REC)
    for name, v in (("first", first), ("area", area), ("rmin", rmin), ("cmin", cmin), ("rmax", rmax), ("cmax", cmax)):
        table[name] = v[kept]
    counts = np.array([fgi.size, ncomp, n, int(area[kept].sum())], np.uint64)
    return labels, area_out, sieved, table, counts


def _run(raster, opts: Options, label_dtype, area_dtype, components):
    a = _as_bands(raster)
    validate(opts)
    check_label_dtype(label_dtype)
    B, h, w = a.shape
    check_region(h, w)
    labels, areas, sieved, tables, counts = [], [], [], [], []
    for b in range(B):
        fg = foreground_of(a[b], opts)
        res = _finish(a[b], components(a[b], fg, opts), opts, label_dtype, area_dtype)
        for lst, v in zip((labels, areas, sieved, tables, counts), res):
            lst.append(v)
    return (np.stack(labels), None if area_dtype is None else np.stack(areas), np.stack(sieved), tables,
            np.stack(counts))


def regions_arrays(raster, opts: Options = Options(), label_dtype="int32", area_dtype="uint32"):
    """The run-based union-find: ``(labels (B, h, w), area (B, h, w) or None, sieved (B, h, w), tables (a list of B
    arrays of :data:`REC`), counts (B, 4) uint64)``.  ``ValueError`` when a band's N does not fit ``label_dtype``."""
    return _run(raster, opts, label_dtype, area_dtype, _components_runs)


def regions_direct(raster, opts: Options = Options(), label_dtype="int32", area_dtype="uint32"):
    """The definition, a flood fill per component; arguments and result as :func:`regions_arrays`, which it equals."""
    return _run(raster, opts, label_dtype, area_dtype, _components_fill)


def component_values(band: np.ndarray, table: np.ndarray) -> np.ndarray:
    """The value of every component of a band's table: the source at its first pixel."""
    return np.asarray(band).ravel()[table["first"].astype(np.int64)]


def export_rows(bands: np.ndarray, tables: List[np.ndarray], transform=None) -> List[dict]:
    """Per band and component: label, value, area, the box in pixels and (with an affine ``transform`` ``(a, b, c, d, e,
    f)``: x = a col + b row + c, y = d col + e row + f) in map coordinates, and the first pixel."""
    a = _as_bands(bands)
    w = a.shape[2]
    rows = []
    for b, table in enumerate(tables):
        vals = component_values(a[b], table)
        for i, rec in enumerate(table):
            row = {"band": b + 1, "label": i + 1, "value": vals[i].item(), "area": int(rec["area"]),
                   "row_min": int(rec["rmin"]), "col_min": int(rec["cmin"]), "row_max": int(rec["rmax"]),
                   "col_max": int(rec["cmax"]), "first_row": int(rec["first"]) // w, "first_col": int(rec["first"]) % w}
            if transform:
                ta, tb, tc, td, te, tf = (float(v) for v in list(transform)[:6])
                xs, ys = [], []
                for cc in (row["col_min"], row["col_max"] + 1):
                    for rr in (row["row_min"], row["row_max"] + 1):
                        xs.append(ta * cc + tb * rr + tc), ys.append(td * cc + te * rr + tf)
                row.update(x_min=min(xs), y_min=min(ys), x_max=max(xs), y_max=max(ys))
            rows.append(row)
    return rows
