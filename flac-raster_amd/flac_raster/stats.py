"""Band statistics and histograms of a raster: the rule of ``fra_stats`` (include/flac_raster_amd.h) in numpy, Python
integers and ``fractions``.

One record per band of a raster ``(B, h, w)`` of one of the eight raster dtypes, every element taken as f64:

* ``nan`` counts the NaN pixels (floats), ``nodata`` those with ``float64(x) == nodata`` (when a nodata value is given; a
  NaN nodata matches nothing), ``valid`` the rest; only valid pixels enter anything else.  +-inf are valid numbers.
* ``min`` / ``max`` over the valid pixels, ``fin_min`` / ``fin_max`` over the finite valid ones (``None`` where there is
  none).
* integer dtypes: ``sum`` and ``sum_sq`` are exact Python integers; ``mean`` and ``variance`` (population) are the exact
  rationals rounded once to a double, ``std`` the square root of that variance.
* f32 / f64: ``sum`` is an f64 sum (no order implied), ``mean = sum / valid``, ``fm2 = sum (x - mean)^2`` with that mean,
  ``variance = fm2 / valid``.  Plain IEEE arithmetic: +-inf propagate.
* histogram: ``bins`` bins over ``[lo, hi]`` -- explicit, or ``"auto"`` = ``[fin_min, fin_max]`` of the band --,
  ``scale = bins / (hi - lo)`` if ``hi > lo`` else 0.0 (also when that quotient is not finite); a valid pixel with
  ``x < lo`` counts in ``below``, one with ``x > hi`` in ``above``, any other goes to bin
  ``min(bins - 1, floor((x - lo) * scale))`` (bin 0 when the scale is 0): separate f64 operations.  When
  ``hi - lo == bins`` the scale is exactly 1.0 and bin ``i`` holds exactly the pixels of value ``lo + i``
  (:func:`exact_range`), which gives exact order statistics (:func:`percentile`).
"""

from __future__ import annotations

import math
from fractions import Fraction
from typing import List, Optional, Sequence

import numpy as np

AUTO_RANGE, NODATA = 1, 2  # fra_stats_opts.flags
MAX_BINS = 65536
_CHUNK = 1 << 22  # pixels per step: bounds the temporaries of a band


def exact_range(dtype):
    """``(lo, hi, bins)`` with unit bins for a dtype of at most 16 bits: bin ``i`` holds exactly the value ``lo + i``."""
    dt = np.dtype(dtype)
    if dt.kind not in "iu" or dt.itemsize > 2:
        raise ValueError(f"no exact histogram range for {dt}: integer dtypes of at most 16 bits only")
    info = np.iinfo(dt)
    bins = int(info.max) - int(info.min) + 1
    return float(info.min), float(info.min) + bins, bins


def _scale(lo: float, hi: float, bins: int) -> float:
    with np.errstate(over="ignore", divide="ignore"):
        scale = float(np.float64(bins) / (np.float64(hi) - np.float64(lo))) if hi > lo else 0.0
    return scale if math.isfinite(scale) else 0.0


def check_options(bins: int, hist_range, nodata):
    """``(bins, range mode, nodata)`` of a request: the mode is ``None`` (no histogram), ``"auto"`` or ``(lo, hi)``."""
    bins = int(bins)
    if bins < 0 or bins > MAX_BINS:
        raise ValueError(f"bins must be 0 ... {MAX_BINS}, got {bins}")
    if bins == 0:
        mode = None
    elif hist_range is None or (isinstance(hist_range, str) and hist_range == "auto"):
        mode = "auto"
    else:
        lo, hi = (float(v) for v in hist_range)
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            raise ValueError(f"the histogram range needs finite bounds with lo <= hi, got ({lo}, {hi})")
        mode = (lo, hi)
    return bins, mode, (None if nodata is None else float(nodata))


def _none_if_nan(v: float) -> Optional[float]:
    return None if v != v else float(v)


def _finish(rec: dict, is_float: bool) -> dict:
    """mean / variance / std of a record that holds the counts and the sums."""
    n = rec["valid"]
    if is_float:
        with np.errstate(all="ignore"):
            rec["variance"] = float(np.float64(rec["fm2"]) / np.float64(n)) if n else math.nan
    else:
        rec["mean"] = float(Fraction(rec["sum"], n)) if n else math.nan
        rec["variance"] = float(Fraction(n * rec["sum_sq"] - rec["sum"] ** 2, n * n)) if n else math.nan
        rec["fm2"] = 0.0
    v = rec["variance"]
    rec["std"] = math.sqrt(v) if v == v and v >= 0.0 else math.nan
    return rec


def _band_record(a: np.ndarray, bins: int, mode, nodata: Optional[float]) -> dict:
    h, w = a.shape
    is_float = a.dtype.kind == "f"
    step = max(1, _CHUNK // w)

    def chunks():
        for r0 in range(0, h, step):
            x = a[r0:r0 + step].astype(np.float64).ravel()
            raw = a[r0:r0 + step].ravel()
            isn = np.isnan(x) if is_float else np.zeros(x.shape, bool)
            isnd = (~isn & (x == nodata)) if nodata is not None else np.zeros(x.shape, bool)  # a NaN nodata: never
            ok = ~(isn | isnd)
            yield x[ok], raw[ok], int(np.count_nonzero(isn)), int(np.count_nonzero(isnd))

    rec = {"count": h * w, "valid": 0, "nan": 0, "nodata": 0, "sum": 0.0 if is_float else 0, "sum_sq": 0}
    mins, maxs, fmins, fmaxs = [], [], [], []
    for x, raw, n_nan, n_nd in chunks():
        rec["valid"] += x.size
        rec["nan"] += n_nan
        rec["nodata"] += n_nd
        if not x.size:
            continue
        mins.append(float(x.min()))
        maxs.append(float(x.max()))
        fin = x[np.isfinite(x)] if is_float else x
        if fin.size:
            fmins.append(float(fin.min()))
            fmaxs.append(float(fin.max()))
        if is_float:
            with np.errstate(all="ignore"):
                rec["sum"] = float(np.float64(rec["sum"]) + x.sum())
        else:
            v = raw.astype(np.int64)
            rec["sum"] += int(v.sum())  # |x| <= 2^31 over 2^22 pixels
            ax = np.abs(v).astype(np.uint64)
            sq = ax * ax  # < 2^64; summed in two 32-bit halves so that nothing wraps
            rec["sum_sq"] += (int((sq >> np.uint64(32)).sum(dtype=np.uint64)) << 32) + int(
                (sq & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))
    rec["min"], rec["max"] = (min(mins), max(maxs)) if mins else (None, None)
    rec["fin_min"], rec["fin_max"] = (min(fmins), max(fmaxs)) if fmins else (None, None)
    n = rec["valid"]
    if is_float:
        with np.errstate(all="ignore"):
            mean = float(np.float64(rec["sum"]) / np.float64(n)) if n else math.nan
        rec["mean"] = mean
        rec["sum_sq"] = 0
    # the second pass: fm2 with the first pass's mean, and the histogram
    rng = None
    if mode == "auto":
        rng = (rec["fin_min"], rec["fin_max"]) if rec["fin_min"] is not None else None
    elif mode is not None:
        rng = mode
    hist = np.zeros(bins, np.uint64) if bins else None
    below = above = 0
    fm2 = 0.0
    scale = _scale(rng[0], rng[1], bins) if rng is not None else 0.0
    if is_float or rng is not None:
        for x, _, _, _ in chunks():
            if not x.size:
                continue
            with np.errstate(all="ignore"):
                if is_float:
                    d = x - np.float64(rec["mean"])
                    fm2 = float(np.float64(fm2) + (d * d).sum())
                if rng is not None:
                    lo, hi = np.float64(rng[0]), np.float64(rng[1])
                    lt, gt = x < lo, x > hi
                    below += int(np.count_nonzero(lt))
                    above += int(np.count_nonzero(gt))
                    y = x[~(lt | gt)]
                    if scale == 0.0:
                        idx = np.zeros(y.shape, np.int64)
                    else:
                        d = y - lo
                        t = d * np.float64(scale)
                        idx = np.minimum(np.float64(bins - 1), np.floor(t)).astype(np.int64)
                    hist += np.bincount(idx, minlength=bins).astype(np.uint64)
    if is_float:
        rec["fm2"] = fm2
    rec.update({"bins": bins, "histogram": [int(v) for v in hist] if hist is not None else None, "below": below,
                "above": above, "hist_range": [float(rng[0]), float(rng[1])] if rng is not None else None,
                "hist_scale": scale})
    return _finish(rec, is_float)


def _check_raster(a):
    a = np.asarray(a)
    if a.dtype.kind not in "iuf" or a.dtype.itemsize > (8 if a.dtype.kind == "f" else 4) or a.dtype == np.float16:
        raise TypeError(f"unsupported dtype {a.dtype}")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.size == 0:
        raise ValueError("the raster must be (B, h, w) or (h, w) with at least one pixel")
    return a


def stats_arrays(a, bins: int = 0, hist_range=None, nodata=None) -> List[dict]:
    """The statistics of a raster ``(B, h, w)`` (or ``(h, w)``): one dict per band (the rule above) with ``band``,
    ``count``, ``valid``, ``nan``, ``nodata``, ``min``, ``max``, ``fin_min``, ``fin_max``, ``sum``, ``sum_sq``, ``fm2``,
    ``mean``, ``variance``, ``std`` (population), ``bins``, ``histogram`` (a list of ints, ``None`` without bins),
    ``below``, ``above``, ``hist_range`` ([lo, hi] used, ``None`` where the band has none) and ``hist_scale``.

    ``hist_range``: ``(lo, hi)``, or ``"auto"`` / ``None`` for ``[fin_min, fin_max]`` of each band."""
    a = _check_raster(a)
    bins, mode, nodata = check_options(bins, hist_range, nodata)
    out = []
    for i in range(a.shape[0]):
        rec = _band_record(a[i], bins, mode, nodata)
        out.append(dict(band=i + 1, **rec))
    return out


def report_from_bands(bands, hist, dtype) -> List[dict]:
    """The dicts of :func:`stats_arrays` from the native records of ``Context.stats`` /
    ``Context.decode_device_stats`` (``_native.StatsBand``) and their histogram (``(B, bins)`` uint64 or ``None``) of a
    raster of ``dtype``, so that host and GPU paths print alike."""
    is_float = np.dtype(dtype).kind == "f"
    out = []
    for i, r in enumerate(bands):
        bins = 0 if hist is None else int(np.asarray(hist).shape[1])
        rec = {"count": int(r.count), "valid": int(r.valid), "nan": int(r.nan), "nodata": int(r.nodata)}
        if is_float:
            rec["sum"], rec["sum_sq"] = float(r.fsum), 0
        else:
            rec["sum"] = (int(r.sum_hi) << 64) + int(r.sum_lo)  # two's complement: the high word is signed
            rec["sum_sq"] = (int(r.sq_hi) << 64) | int(r.sq_lo)
        rec["min"], rec["max"] = _none_if_nan(r.min), _none_if_nan(r.max)
        rec["fin_min"], rec["fin_max"] = _none_if_nan(r.fin_min), _none_if_nan(r.fin_max)
        if is_float:
            rec["mean"], rec["fm2"] = float(r.mean), float(r.fm2)
        has_range = bins > 0 and r.hist_lo == r.hist_lo
        rec.update({"bins": bins, "histogram": [int(v) for v in np.asarray(hist)[i]] if bins else None,
                    "below": int(r.below), "above": int(r.above),
                    "hist_range": [float(r.hist_lo), float(r.hist_hi)] if has_range else None,
                    "hist_scale": float(r.hist_scale)})
        out.append(dict(band=i + 1, **_finish(rec, is_float)))
    return out


def percentile(band: dict, q):
    """The nearest-rank ``q``-th percentile over the binned pixels of a band's dict: with ``n`` of them,
    ``k = max(1, ceil(q n / 100))`` in exact rational arithmetic, and the result is the bin that holds the ``k``-th
    smallest.  Unit bins (``hi - lo == bins``): the exact value ``lo + j``; otherwise the bin's nominal edges
    ``(lo + j (hi - lo) / bins, lo + (j + 1) (hi - lo) / bins)``.  ``None`` when nothing is binned."""
    hist = band.get("histogram")
    if not hist or band.get("hist_range") is None:
        return None
    qf = Fraction(q) if isinstance(q, (int, Fraction)) else Fraction(str(q))
    if not 0 <= qf <= 100:
        raise ValueError("a percentile lies in 0 ... 100")
    n = sum(hist)
    if n == 0:
        return None
    k = max(1, math.ceil(qf * n / 100))
    seen = 0
    for j, c in enumerate(hist):
        seen += c
        if seen >= k:
            break
    lo, hi = band["hist_range"]
    bins = len(hist)
    if hi - lo == bins:
        return lo + j
    return lo + j * (hi - lo) / bins, lo + (j + 1) * (hi - lo) / bins


def flags_of(mode, nodata) -> int:
    return (AUTO_RANGE if mode == "auto" else 0) | (NODATA if nodata is not None else 0)


def display_stats_table(bands: Sequence[dict], percentiles: Sequence[float] = (), title: str = "Band statistics"):
    from rich.console import Console
    from rich.table import Table

    t = Table(title=title, show_header=True)
    for name in ["Band", "Valid", "NaN", "Nodata", "Min", "Max", "Mean", "Std"] + [f"p{q:g}" for q in percentiles]:
        t.add_column(name)
    fmt = lambda v: "-" if v is None or v != v else f"{v:.6g}"  # noqa: E731
    for b in bands:
        cells = [str(b["band"]), str(b["valid"]), str(b["nan"]), str(b["nodata"]), fmt(b["min"]), fmt(b["max"]),
                 fmt(b["mean"]), fmt(b["std"])]
        for q in percentiles:
            p = percentile(b, q)
            cells.append("-" if p is None else (fmt(p) if not isinstance(p, tuple) else f"[{p[0]:.6g}, {p[1]:.6g})"))
        t.add_row(*cells)
    Console().print(t)
