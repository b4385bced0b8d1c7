"""Zonal statistics: the rule of ``fra_zonal`` (include/flac_raster_amd.h) in numpy, Python integers and ``fractions``.

A value raster ``(B, h, w)`` of one of the eight raster dtypes and a zone raster ``(h, w)`` of an integer dtype:

* a pixel with label ``z`` belongs to zone ``k = z - zone_lo`` when ``0 <= k < nzones`` and ``z`` is not the ignored
  label; every other pixel is *outside* (one count per call, not per band);
* one record per (band, zone) over the zone's pixels, with the meanings of ``stats``: ``count = valid + nan + nodata``
  (every element taken as f64, a NaN nodata matches nothing, +-inf are valid), ``min`` / ``max`` over the valid pixels
  (``None`` where there is none);
* integer dtypes: ``sum`` and ``sum_sq`` are exact Python integers, ``mean`` and ``variance`` (population) the exact
  rationals rounded once, ``std`` the square root of that variance;
* f32 / f64: ``sum`` is an f64 sum (no order implied), ``mean = sum / valid``, ``fm2 = sum (x - mean)^2`` with that
  zone's mean, ``variance = fm2 / valid``.  Plain IEEE arithmetic: +-inf propagate; a zone without a valid pixel has
  ``mean = NaN`` and ``fm2 = 0``.
"""

from __future__ import annotations

import csv
import json
import math
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np

from .stats import _check_raster, _finish

NODATA, IGNORE = 1, 2  # fra_zonal_opts.flags
MAX_ZONES = 65536
ZONE_DTYPES = tuple(np.dtype(t) for t in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32))
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1

# fra_zonal_rec (112 bytes)
REC_DTYPE = np.dtype([("count", "<u8"), ("valid", "<u8"), ("nan", "<u8"), ("nodata", "<u8"), ("sum_lo", "<u8"),
                      ("sum_hi", "<i8"), ("sq_lo", "<u8"), ("sq_hi", "<u8"), ("min", "<f8"), ("max", "<f8"),
                      ("fsum", "<f8"), ("mean", "<f8"), ("fm2", "<f8"), ("reserved", "<u8")])
assert REC_DTYPE.itemsize == 112

FIELDS = ("zone", "count", "valid", "nan", "nodata", "min", "max", "sum", "sum_sq", "mean", "variance", "std", "fm2")


def _check_zones(zones, shape) -> np.ndarray:
    z = np.asarray(zones)
    if z.dtype.kind not in "iu":
        raise TypeError(f"the zone raster must have an integer dtype, got {z.dtype}")
    if z.shape != tuple(shape):
        raise ValueError(f"the zone raster must be {tuple(shape)} like the values, got {z.shape}")
    return z


def _label_range(z: np.ndarray, ignore):
    """``(min, max)`` of the labels that are not ignored, as Python integers; ``None`` when there is none."""
    if ignore is not None:
        z = z[z != ignore] if _I64_MIN <= int(ignore) <= _I64_MAX else z.ravel()
    if z.size == 0:
        return None
    return int(z.min()), int(z.max())


def _empty_record(label: int, is_float: bool) -> dict:
    rec = {"zone": label, "count": 0, "valid": 0, "nan": 0, "nodata": 0, "min": None, "max": None,
           "sum": 0.0 if is_float else 0, "sum_sq": 0}
    if is_float:
        rec["mean"], rec["fm2"] = math.nan, 0.0
    return _finish(rec, is_float)


def zonal_arrays(values, zones, zone_lo: Optional[int] = None, nzones: Optional[int] = None, nodata=None, ignore=None,
                 all_zones: bool = False) -> List[dict]:
    """The zonal statistics of ``values`` ``(B, h, w)`` (or ``(h, w)``) over ``zones`` ``(h, w)``: one dict per band,
    ``{"band", "outside", "zones": [record, ...]}`` with the records in zone order, each ``{"zone": label, "count",
    "valid", "nan", "nodata", "min", "max", "sum", "sum_sq", "mean", "variance", "std", "fm2"}`` (the rule above).

    ``zone_lo`` / ``nzones``: the range of labels that are zones (default: from the smallest to the largest label that
    is not ignored).  ``ignore``: a label whose pixels are outside.  ``nodata`` as ``stats.stats_arrays``.  Only the
    zones with ``count > 0`` are listed, unless ``all_zones``."""
    a = _check_raster(values)
    B, h, w = a.shape
    z = _check_zones(zones, (h, w)).ravel()
    is_float = a.dtype.kind == "f"
    nodata = None if nodata is None else float(nodata)
    ignore = None if ignore is None else int(ignore)
    if zone_lo is None or nzones is None:
        rng = _label_range(z, ignore)
        lo = int(zone_lo) if zone_lo is not None else (rng[0] if rng else 0)
        nzones = int(nzones) if nzones is not None else (max(1, rng[1] - lo + 1) if rng else 1)
        zone_lo = lo
    zone_lo, nzones = int(zone_lo), int(nzones)
    if nzones < 1:
        raise ValueError(f"nzones must be at least 1, got {nzones}")
    z = z.astype(np.int64)
    inside = np.ones(z.shape, bool)
    if ignore is not None and _I64_MIN <= ignore <= _I64_MAX:
        inside &= z != ignore
    zone_hi = zone_lo + nzones - 1
    if zone_hi < _I64_MIN or zone_lo > _I64_MAX:
        inside[:] = False
    else:
        lo_c, hi_c = max(zone_lo, _I64_MIN), min(zone_hi, _I64_MAX)
        inside &= (z >= lo_c) & (z <= hi_c)
    outside = int(z.size - np.count_nonzero(inside))
    k = (z[inside] - max(zone_lo, _I64_MIN)) + (max(zone_lo, _I64_MIN) - zone_lo) if inside.any() else np.zeros(0, np.int64)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    present, starts = np.unique(ks, return_index=True)
    sizes = np.diff(np.append(starts, ks.size))
    group = np.repeat(np.arange(present.size), sizes)  # of every sorted pixel
    out = []
    for b in range(B):
        raw = a[b].ravel()[inside][order]
        recs = _zone_records(raw, present, starts, sizes, group, is_float, nodata) if present.size else []
        for rec in recs:
            rec["zone"] = zone_lo + rec["zone"]
        if all_zones:
            have = {rec["zone"]: rec for rec in recs}
            recs = [have.get(zone_lo + i) or _empty_record(zone_lo + i, is_float) for i in range(nzones)]
        out.append({"band": b + 1, "outside": outside, "zones": recs})
    return out


def _zone_records(raw, present, starts, sizes, group, is_float: bool, nodata) -> List[dict]:
    """The records of the zones ``present`` of one band: ``raw`` holds the band's pixels sorted by zone, zone ``i``
    being ``raw[starts[i]:starts[i] + sizes[i]]``."""
    x = raw.astype(np.float64)
    isn = np.isnan(x) if is_float else np.zeros(x.shape, bool)
    isnd = (~isn & (x == nodata)) if nodata is not None else np.zeros(x.shape, bool)  # a NaN nodata: never
    ok = ~(isn | isnd)
    seg = lambda v, op=np.add: op.reduceat(v, starts)  # noqa: E731
    n_nan, n_nd, n_ok = seg(isn.astype(np.int64)), seg(isnd.astype(np.int64)), seg(ok.astype(np.int64))
    with np.errstate(all="ignore"):
        mins = seg(np.where(ok, x, np.inf), np.minimum)
        maxs = seg(np.where(ok, x, -np.inf), np.maximum)
        if is_float:
            fsum = seg(np.where(ok, x, 0.0))
            mean = fsum / n_ok.astype(np.float64)  # 0 / 0 = NaN
            d = np.where(ok, x - mean[group], 0.0)
            fm2 = seg(d * d)
        else:
            v = np.where(ok, raw.astype(np.int64), 0)
            # a zone's |sum| stays below 2^63 and the halves of its squares below 2^64 for fewer than 2^32 pixels
            s_pos = seg(np.where(v > 0, v, 0).astype(np.uint64))
            s_neg = seg(np.where(v < 0, -v, 0).astype(np.uint64))
            ax = np.abs(v).astype(np.uint64)
            sq = ax * ax  # < 2^64; summed in two 32-bit halves so that nothing wraps
            sq_hi, sq_lo = seg(sq >> np.uint64(32)), seg(sq & np.uint64(0xFFFFFFFF))
    recs = []
    for i in range(present.size):
        n = int(n_ok[i])
        rec = {"zone": int(present[i]), "count": int(sizes[i]), "valid": n, "nan": int(n_nan[i]), "nodata": int(n_nd[i]),
               "min": float(mins[i]) if n else None, "max": float(maxs[i]) if n else None}
        if is_float:
            rec["sum"], rec["sum_sq"] = float(fsum[i]), 0
            rec["mean"], rec["fm2"] = float(mean[i]), float(fm2[i])
        else:
            rec["sum"] = int(s_pos[i]) - int(s_neg[i])
            rec["sum_sq"] = (int(sq_hi[i]) << 32) + int(sq_lo[i])
        recs.append(_finish(rec, is_float))
    return recs


def dense_zones(zones, ignore=None):
    """How the labels of a zone raster reach the kernel -> ``(zones, zone_lo, nzones, labels)``.

    Labels that span fewer than 65536 values (the ignored label aside) go as they are: the same array, no copy, with
    ``zone_lo`` the smallest label and ``labels = None``.  Otherwise they are relabelled through ``np.unique`` to dense
    ids ``0 ... n - 1`` (an int32 raster, ``zone_lo = 0``) and ``labels[id]`` is the label of zone ``id``; the pixels of
    the ignored label then carry id -1, which lies outside the range, so no ignore label goes with the dense raster.
    More than 65536 distinct labels raise ``ValueError``."""
    z = np.asarray(zones)
    if z.dtype.kind not in "iu":
        raise TypeError(f"the zone raster must have an integer dtype, got {z.dtype}")
    ignore = None if ignore is None else int(ignore)
    rng = _label_range(z, ignore)
    if rng is None:
        return zones, 0, 1, None
    if rng[1] - rng[0] < MAX_ZONES:
        return zones, rng[0], rng[1] - rng[0] + 1, None
    keep = z != ignore if ignore is not None and _I64_MIN <= ignore <= _I64_MAX else np.ones(z.shape, bool)
    labels = np.unique(z[keep])
    if labels.size > MAX_ZONES:
        raise ValueError(f"{labels.size} distinct zone labels: at most {MAX_ZONES} zones go into one call")
    dense = np.where(keep, np.searchsorted(labels, z), -1).astype(np.int32)
    return dense, 0, int(labels.size), labels


def records_array(recs) -> np.ndarray:
    """The native records (a ctypes array of ``_native.ZonalRec`` or bytes) as a numpy array of :data:`REC_DTYPE`."""
    if isinstance(recs, np.ndarray) and recs.dtype == REC_DTYPE:
        return recs
    return np.frombuffer(recs, dtype=REC_DTYPE)


def report_from_recs(recs, outside: int, dtype, zone_lo: int = 0, labels=None, all_zones: bool = False) -> List[dict]:
    """The dicts of :func:`zonal_arrays` from the native records of ``Context.zonal`` /
    ``Context.decode_device_zonal`` -- ``(B, nzones)`` of :data:`REC_DTYPE` -- of a value raster of ``dtype``, so that
    host and GPU paths print alike.  Zone ``k`` carries the label ``labels[k]`` (:func:`dense_zones`) or
    ``zone_lo + k``."""
    r = records_array(recs)
    if r.ndim != 2:
        raise ValueError("the records must be (bands, nzones)")
    is_float = np.dtype(dtype).kind == "f"
    out = []
    for b in range(r.shape[0]):
        rows = r[b]
        ks = np.arange(rows.size) if all_zones else np.flatnonzero(rows["count"])
        zs = []
        for k in ks:
            q = rows[k]
            n = int(q["valid"])
            label = int(labels[k]) if labels is not None else int(zone_lo) + int(k)
            rec = {"zone": label, "count": int(q["count"]), "valid": n, "nan": int(q["nan"]), "nodata": int(q["nodata"]),
                   "min": float(q["min"]) if n else None, "max": float(q["max"]) if n else None}
            if is_float:
                rec["sum"], rec["sum_sq"] = float(q["fsum"]), 0
                rec["mean"], rec["fm2"] = float(q["mean"]), float(q["fm2"])
            else:
                rec["sum"] = (int(q["sum_hi"]) << 64) + int(q["sum_lo"])  # two's complement: the high word is signed
                rec["sum_sq"] = (int(q["sq_hi"]) << 64) | int(q["sq_lo"])
            zs.append(_finish(rec, is_float))
        out.append({"band": b + 1, "outside": int(outside), "zones": zs})
    return out


def relabel(report: List[dict], labels) -> List[dict]:
    """``report`` of a dense raster of :func:`dense_zones` with the zones' own labels."""
    if labels is not None:
        for band in report:
            for rec in band["zones"]:
                rec["zone"] = int(labels[rec["zone"]])
    return report


def flags_of(nodata, ignore) -> int:
    return (NODATA if nodata is not None else 0) | (IGNORE if ignore is not None else 0)


# ------------------------------------------------------------------------------------------ printing and export
def display_zonal_table(report: Sequence[dict], title: str = "Zonal statistics", limit: int = 50):
    from rich.console import Console
    from rich.table import Table

    t = Table(title=title, show_header=True)
    for name in ("Zone", "Band", "Valid", "Min", "Max", "Mean", "Std"):
        t.add_column(name)
    fmt = lambda v: "-" if v is None or v != v else f"{v:.6g}"  # noqa: E731
    labels = sorted({rec["zone"] for band in report for rec in band["zones"]})
    shown = set(labels[:limit])
    by_band = [{rec["zone"]: rec for rec in band["zones"]} for band in report]
    for label in labels[:limit]:
        for band, recs in zip(report, by_band):
            rec = recs.get(label)
            if rec is not None:
                t.add_row(str(label), str(band["band"]), str(rec["valid"]), fmt(rec["min"]), fmt(rec["max"]),
                          fmt(rec["mean"]), fmt(rec["std"]))
    con = Console()
    con.print(t)
    if len(labels) > len(shown):
        con.print(f"... and {len(labels) - len(shown)} more zones")
    if report:
        con.print(f"{report[0]['outside']} pixels outside every zone")


def export_report(path: Path, report: Sequence[dict], header: Optional[dict] = None):
    """The full report as JSON (``.json``: ``header`` plus ``"bands"``) or CSV (``.csv``: one row per (band, zone),
    floats written so that they read back exactly, an empty cell for a missing value)."""
    path = Path(path)
    if path.suffix.lower() == ".csv":
        with open(path, "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(("band", "outside") + FIELDS)
            for band in report:
                for rec in band["zones"]:
                    wr.writerow([band["band"], band["outside"]] +
                                ["" if rec[k] is None else repr(rec[k]) for k in FIELDS])
    elif path.suffix.lower() == ".json":
        path.write_text(json.dumps(dict(header or {}, bands=list(report)), indent=2))
    else:
        raise ValueError("the export goes to a .json or a .csv file")


def read_csv_report(path: Path) -> List[dict]:
    """The report a CSV of :func:`export_report` holds."""
    ints = {"zone", "count", "valid", "nan", "nodata", "sum_sq"}
    bands = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            rec = {}
            for k in FIELDS:
                v = row[k]
                if v == "":
                    rec[k] = None
                elif k in ints or (k == "sum" and not any(c in v for c in ".einfa")):
                    rec[k] = int(v)
                else:
                    rec[k] = float(v)
            band = bands.setdefault(int(row["band"]), {"band": int(row["band"]), "outside": int(row["outside"]), "zones": []})
            band["zones"].append(rec)
    return [bands[b] for b in sorted(bands)]
