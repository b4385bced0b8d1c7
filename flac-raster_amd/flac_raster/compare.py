"""TIFF comparison report (``compare.py`` of the reference: ``compare_tiffs`` +
``display_comparison_table``), on the in-package GeoTIFF reader."""

from __future__ import annotations

import logging
from pathlib import Path

import numpy as np
from rich.console import Console
from rich.table import Table

from .tiff import GeoTIFF

console = Console()
logger = logging.getLogger("flac_raster.compare")


def compare_tiffs(file1_path: Path, file2_path: Path, show_bands: bool = True) -> dict:
    p1, p2 = Path(file1_path), Path(file2_path)
    g1, g2 = GeoTIFF(p1), GeoTIFF(p2)
    d1, d2 = g1.read(), g2.read()
    r = {
        "file1": p1.name, "file2": p2.name,
        "shape_match": d1.shape == d2.shape,
        "dtype_match": d1.dtype == d2.dtype,
        "crs_match": g1.info.crs == g2.info.crs,
        "file1_shape": d1.shape, "file2_shape": d2.shape,
        "file1_dtype": str(d1.dtype), "file2_dtype": str(d2.dtype),
        "file1_crs": str(g1.info.crs), "file2_crs": str(g2.info.crs),
    }
    if r["shape_match"]:
        diff = np.abs(d1 - d2)  # same (possibly wrapping) arithmetic as the reference
        r["arrays_equal"] = bool(np.array_equal(d1, d2))
        r["max_difference"] = float(np.max(diff))
        r["mean_difference"] = float(np.mean(diff))
        r["rmse"] = float(np.sqrt(np.mean((d1 - d2) ** 2)))
        r["file1_min"], r["file1_max"] = float(np.min(d1)), float(np.max(d1))
        r["file2_min"], r["file2_max"] = float(np.min(d2)), float(np.max(d2))
        if show_bands and d1.ndim == 3:
            r["bands"] = [{
                "band": i + 1,
                "equal": bool(np.array_equal(d1[i], d2[i])),
                "max_diff": float(np.max(np.abs(d1[i] - d2[i]))),
                "mean_diff": float(np.mean(np.abs(d1[i] - d2[i]))),
                "file1_range": [float(d1[i].min()), float(d1[i].max())],
                "file2_range": [float(d2[i].min()), float(d2[i].max())],
            } for i in range(d1.shape[0])]
    return r


# ------------------------------------------------------------------------------------------ the exact comparison
# The rule of ``fra_compare`` (include/flac_raster_amd.h) in numpy and Python integers.  Two rasters ``a``, ``b`` of one
# dtype and shape ``(B, h, w)``, one record per band:
#   integer dtypes  d = int64(a) - int64(b), never wrapping.  differing = pixels with d != 0, first = the first of them
#                   in row-major order, max_abs = max |d|, sum_abs = sum |d| and sum_sq = sum d^2 as Python integers,
#                   the minima and maxima of a and b: all exact.  unordered = 0.
#   f32 / f64       every element as f64.  Both non-NaN: equal iff a == b (-0.0 equals +0.0), d = 0.0 when equal else
#                   a - b (+-inf propagates), |d| goes to max_abs and sum_abs, d * d to sum_sq (f64 sums, no order
#                   implied).  Both NaN: unordered only.  One NaN: unordered and differing, eligible for first, nothing
#                   else.  Minima and maxima skip NaN (NaN when the band holds no number).
#                   differing == 0 is np.array_equal(a, b, equal_nan=True).
_CHUNK = 1 << 22  # pixels per step: bounds the temporaries of a band


def _band_record(a: np.ndarray, b: np.ndarray) -> dict:
    h, w = a.shape
    is_float = a.dtype.kind == "f"
    rec = {"count": h * w, "differing": 0, "unordered": 0, "one_sided_nan": 0, "first": None, "max_abs": 0.0,
           "sum_abs": 0.0 if is_float else 0, "sum_sq": 0.0 if is_float else 0, "is_float": is_float}
    mins = {"a_min": [], "a_max": [], "b_min": [], "b_max": []}
    step = max(1, _CHUNK // w)
    for r0 in range(0, h, step):
        x, y = a[r0:r0 + step], b[r0:r0 + step]
        if is_float:
            x, y = x.astype(np.float64), y.astype(np.float64)
            xn, yn = np.isnan(x), np.isnan(y)
            un = xn | yn
            eq = x == y
            with np.errstate(invalid="ignore", over="ignore"):
                d = np.where(un | eq, 0.0, x - y)
            ad = np.abs(d)
            diff = (xn != yn) | (~un & ~eq)
            rec["unordered"] += int(np.count_nonzero(un))
            rec["one_sided_nan"] += int(np.count_nonzero(xn != yn))
            rec["max_abs"] = max(rec["max_abs"], float(ad.max()))
            with np.errstate(over="ignore"):
                rec["sum_abs"] += float(ad.sum())
                rec["sum_sq"] += float((d * d).sum())
            for key, v, nan in (("a", x, xn), ("b", y, yn)):
                if not nan.all():
                    mins[key + "_min"].append(float(np.nanmin(v)))
                    mins[key + "_max"].append(float(np.nanmax(v)))
        else:
            ad = np.abs(x.astype(np.int64) - y.astype(np.int64)).astype(np.uint64)  # <= 2^32 - 1
            diff = ad != 0
            rec["max_abs"] = max(rec["max_abs"], float(ad.max()))
            rec["sum_abs"] += int(ad.sum(dtype=np.uint64))  # < 2^22 * 2^32
            sq = ad * ad  # < 2^64; summed in two 32-bit halves so that nothing wraps
            rec["sum_sq"] += (int((sq >> np.uint64(32)).sum(dtype=np.uint64)) << 32) + int(
                (sq & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))
            for key, v in (("a", x), ("b", y)):
                mins[key + "_min"].append(float(v.min()))
                mins[key + "_max"].append(float(v.max()))
        n = int(np.count_nonzero(diff))
        if n and rec["first"] is None:
            at = int(np.argmax(diff.ravel()))
            rec["first"] = (r0 + at // w, at % w)
        rec["differing"] += n
    for key, vals in mins.items():
        rec[key] = (min(vals) if key.endswith("min") else max(vals)) if vals else float("nan")
    return rec


def _record_of_native(r, is_float=None) -> dict:
    """A ``_native.CompareBand`` as the record ``_band_record`` gives (``is_float`` None: told from the report, whose
    integer sums are 0 for a float dtype and whose float sums are 0 for an integer one)."""
    if is_float is None:
        is_float = not (r.sum_abs or r.sum_sq_lo or r.sum_sq_hi) and bool(r.fsum_abs or r.fsum_sq or r.unordered)
    # pixels with a NaN on one side only are both unordered and differing; the two counts settle their number only
    # when one of them is 0 (None: not known from this report)
    return {"count": int(r.count), "differing": int(r.differing), "unordered": int(r.unordered),
            "one_sided_nan": 0 if not (r.unordered and r.differing) else None,
            "first": (int(r.first_row), int(r.first_col)) if r.first_row >= 0 else None, "max_abs": float(r.max_abs),
            "sum_abs": float(r.fsum_abs) if is_float else int(r.sum_abs),
            "sum_sq": float(r.fsum_sq) if is_float else (int(r.sum_sq_hi) << 64) | int(r.sum_sq_lo),
            "a_min": float(r.a_min), "a_max": float(r.a_max), "b_min": float(r.b_min), "b_max": float(r.b_max),
            "is_float": is_float}


def _nan_extreme(vals, fn):
    vals = [v for v in vals if v == v]
    return fn(vals) if vals else float("nan")


def _report(records) -> dict:
    count = sum(r["count"] for r in records)
    sum_abs = sum(r["sum_abs"] for r in records)
    sum_sq = sum(r["sum_sq"] for r in records)
    bands = []
    for i, r in enumerate(records):
        bands.append({
            "band": i + 1, "equal": r["differing"] == 0, "count": r["count"], "differing": r["differing"],
            "unordered": r["unordered"], "one_sided_nan": r["one_sided_nan"],
            "first": list(r["first"]) if r["first"] is not None else None,
            "max_diff": r["max_abs"], "mean_diff": r["sum_abs"] / r["count"],
            "rmse": float(np.sqrt(r["sum_sq"] / r["count"])),
            "sum_abs": r["sum_abs"], "sum_sq": r["sum_sq"],
            "file1_range": [r["a_min"], r["a_max"]], "file2_range": [r["b_min"], r["b_max"]],
        })
    return {
        "arrays_equal": all(r["differing"] == 0 for r in records),
        "differing": sum(r["differing"] for r in records), "unordered": sum(r["unordered"] for r in records),
        "one_sided_nan": (None if any(r["one_sided_nan"] is None for r in records)
                          else sum(r["one_sided_nan"] for r in records)),
        "max_difference": max(r["max_abs"] for r in records),
        "mean_difference": sum_abs / count, "rmse": float(np.sqrt(sum_sq / count)),
        "file1_min": _nan_extreme([r["a_min"] for r in records], min),
        "file1_max": _nan_extreme([r["a_max"] for r in records], max),
        "file2_min": _nan_extreme([r["b_min"] for r in records], min),
        "file2_max": _nan_extreme([r["b_max"] for r in records], max),
        "bands": bands,
    }


def compare_arrays(a: np.ndarray, b: np.ndarray) -> dict:
    """The exact comparison of two rasters ``(B, h, w)`` (or ``(h, w)``) of one dtype and shape (the rule above).

    Returns ``arrays_equal`` (no differing pixel: ``np.array_equal(a, b, equal_nan=True)``), ``differing``,
    ``unordered``, ``max_difference``, ``mean_difference``, ``rmse``, ``file1_min`` / ``_max`` (of ``a``), ``file2_min`` /
    ``_max`` (of ``b``) and ``bands``: per band ``equal``, ``count``, ``differing``, ``first`` ([row, col] of the first
    differing pixel in row-major order, or ``None``), ``max_diff``, ``mean_diff``, ``rmse``, ``unordered``, the ranges,
    and the sums the means come from, ``sum_abs`` and ``sum_sq`` (exact Python integers for integer dtypes, f64 sums
    for floats).  Integer differences never wrap, whatever the dtype."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError(f"the rasters differ in shape or dtype: {a.shape} of {a.dtype}, {b.shape} of {b.dtype}")
    if a.dtype.kind not in "iuf" or a.dtype.itemsize > (8 if a.dtype.kind == "f" else 4):
        raise TypeError(f"unsupported dtype {a.dtype}")
    if a.ndim == 2:
        a, b = a[None], b[None]
    if a.ndim != 3 or a.size == 0:
        raise ValueError("rasters must be (B, h, w) or (h, w) with at least one pixel")
    return _report([_band_record(a[i], b[i]) for i in range(a.shape[0])])


def report_from_bands(bands, dtype=None) -> dict:
    """The dict of :func:`compare_arrays` from the native reports of ``Context.compare`` /
    ``Context.decode_device_compare`` (``_native.CompareBand``) of rasters of ``dtype``, so that host and GPU paths
    print alike.  ``one_sided_nan`` is ``None`` where a band has both unordered and differing pixels: the native
    report does not say how many pixels are both."""
    is_float = None if dtype is None else np.dtype(dtype).kind == "f"
    return _report([_record_of_native(r, is_float) for r in bands])


def display_first_differences(results: dict):
    """The first differing pixel of every band that has one (``compare_arrays`` / ``report_from_bands`` results;
    ``results["origin"]`` = (row, col) of the compared region in the raster, default (0, 0))."""
    r0, c0 = results.get("origin", (0, 0))
    for x in results.get("bands", []):
        if x.get("first") is not None:
            row, col = x["first"]
            note = f", {x['unordered']} pixel(s) with a NaN" if x.get("unordered") else ""
            console.print(f"Band {x['band']}: {x['differing']} of {x['count']} pixels differ, the first at row "
                          f"{r0 + row}, column {c0 + col}{note}")


def display_comparison_table(results: dict):
    t = Table(title="TIFF Comparison Results", show_header=True)
    t.add_column("Property", style="cyan")
    t.add_column(results["file1"], style="green")
    t.add_column(results["file2"], style="yellow")
    t.add_column("Match", style="bold")
    yn = lambda b: "YES" if b else "NO"  # noqa: E731
    t.add_row("Shape", str(results["file1_shape"]), str(results["file2_shape"]), yn(results["shape_match"]))
    t.add_row("Data Type", results["file1_dtype"], results["file2_dtype"], yn(results["dtype_match"]))
    t.add_row("CRS", results["file1_crs"], results["file2_crs"], yn(results["crs_match"]))
    console.print(t)
    if not results.get("shape_match"):
        console.print("[red]Cannot compute detailed statistics - shapes don't match![/red]")
        return
    s = Table(title="Statistical Comparison", show_header=True)
    s.add_column("Metric", style="cyan")
    s.add_column("Value", style="bold")
    s.add_row("Arrays Equal", yn(results["arrays_equal"]))
    s.add_row("Max Difference", f"{results['max_difference']:.6f}")
    s.add_row("Mean Difference", f"{results['mean_difference']:.6f}")
    s.add_row("RMSE", f"{results['rmse']:.6f}")
    console.print(s)
    rg = Table(title="Data Ranges", show_header=True)
    rg.add_column("File", style="cyan")
    rg.add_column("Min", style="blue")
    rg.add_column("Max", style="red")
    rg.add_row(results["file1"], f"{results['file1_min']:.2f}", f"{results['file1_max']:.2f}")
    rg.add_row(results["file2"], f"{results['file2_min']:.2f}", f"{results['file2_max']:.2f}")
    console.print(rg)
    if "bands" in results:
        b = Table(title="Per-Band Statistics", show_header=True)
        for name, style in (("Band", "cyan"), ("Equal", "bold"), ("Max Diff", "yellow"), ("Mean Diff", "yellow"),
                            (f"{results['file1']} Range", "green"), (f"{results['file2']} Range", "blue")):
            b.add_column(name, style=style)
        for x in results["bands"]:
            b.add_row(str(x["band"]), yn(x["equal"]), f"{x['max_diff']:.3f}", f"{x['mean_diff']:.6f}",
                      f"[{x['file1_range'][0]:.1f}, {x['file1_range'][1]:.1f}]",
                      f"[{x['file2_range'][0]:.1f}, {x['file2_range'][1]:.1f}]")
        console.print(b)
