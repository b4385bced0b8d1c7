#!/usr/bin/env python3
"""Decode benchmark: the device decoder (``fra_decode_device``) against the host decoder (``fra_decode``).

A synthetic C4-like scene (``fra_synth_raster`` kind 4: 10980 x 10980 x 4 uint16, tile 1024, level 5) is encoded
once by a plan on the GPU; ``--tiles N`` keeps the first N tiles (default: all 121).  Per step, over ``--warmup`` +
``--steps`` steps, one JSON line reports:

  host_decode_ms    fra_decode on every tile's stream, one tile after the other; each call uses at most 16 threads
                    (the library caps its pool at 16, it is not sized by the machine's core count)
  device_ms         HIP events, first decode kernel to last: the plan's frames resident on the device, frame offsets
                    supplied (no candidate search), samples into a device raster
  device_search_ms  wall time of the same decode without offsets: complete streams in page-locked host memory, so it
                    includes their H2D copy, the candidate search, the frame-table copy and the chain
  e2e_ms            wall time, host container bytes -> host raster (``streaming_to_raster(device=0)``)
  samples_per_s     of each of the above, and each kernel's share of device_ms (``kernels``)

    python tools/bench_decode.py --tiles 121 --steps 3 --warmup 1

``--window [r,c,h,w]`` (default: 2048 x 2048 at the scene's centre) times a windowed read
(``fra_decode_device_window``) against the full decode of the same run -- what a user of the full decode has to do to
get the same pixels -- on both paths: frames resident with offsets (``window_ms`` against ``device_ms``, HIP events,
and the wall times) and complete streams in page-locked host memory, searched (``window_search_ms`` against
``device_search_ms``, wall).  The window's pixels must equal the crop of the full decode.  The host-decoder and
container legs are skipped.

    python tools/bench_decode.py --window --steps 5 --warmup 2

``--verify`` times verify mode (``fra_plan_verify``: the plan's frames decoded and compared with its raster on the
GPU, nothing stored) beside the plain decode of the same frames in the same run: ``verify_wall_ms`` / ``verify_ms``
(HIP events, first kernel to last) and its three kernel times against ``device_wall_ms`` / ``device_ms`` and the
decode's.  The plan's encode time (``encode_ms``, wall, one execute + sync) is reported for scale.  A pixel of the
raster is then overwritten and must be the one reported.  The other legs are skipped.

    python tools/bench_decode.py --verify --steps 5 --warmup 2

``--decimate K`` (``--resampling`` nearest | average, default average) times the decimated read of the whole raster
(``fra_decode_device_decimated``) in three legs: the full decode to a device destination as above (``device_ms``); the
decimated decode of the same resident frames (``kernels_decimated``: parse, restore, scatter and ``k_decimate`` by HIP
events, ``decimated_wall_ms``; ``k_decimate_TBps`` = (bytes read + written) / its event time;
``peak_device_bytes_of_call`` = the drop of free device memory sampled beside one call); and container bytes -> host
raster, ``read_overview(device=0)`` against ``streaming_to_raster(device=0)`` alternating in this process
(``e2e_overview_ms`` / ``e2e_full_ms``).  The result must equal ``resample.decimate`` of the full decode on the rows
checked.  The other legs are skipped.

    python tools/bench_decode.py --decimate 8 --steps 5 --warmup 2

``--resample H,W`` (``--resampling`` nearest | average | bilinear | cubic, default average; ``--region r,c,h,w``, default
the whole raster) times the read of the region resampled to H x W (``fra_decode_device_resampled``) in the same three
legs as ``--decimate``: the full decode (``device_ms``); the resampled decode of the same resident frames
(``kernels_resampled`` with ``k_resample_ms``, ``resampled_wall_ms``; ``k_resample_TBps`` = ``k_resample_bytes`` / its
event time, the bytes being the region once plus the output for ``average`` and at most the taps of every output
otherwise); and container bytes -> host raster, ``read_overview(out_shape=)`` against ``streaming_to_raster`` (with
``--region``: ``read_window(out_shape=)`` against the plain ``read_window``), alternating (``e2e_resampled_ms`` /
``e2e_full_ms``).  Band 0 of the result must equal ``resample.resample`` of band 0 of the full
decode (an output row of an arbitrary size depends on the whole raster's height, so the band is checked whole).

    python tools/bench_decode.py --resample 1373,1373 --steps 5 --warmup 2

``--nodata X`` with ``--decimate`` or ``--resample`` times the nodata-aware read instead (``k_resample_masked`` through the
``_masked`` entries; the same JSON keys, the kernel's time from ``fra_resample_masked_timing``) and checks it against
the rule with that value.  X is a value of the decoded int16 samples, or ``corner``: what pixel (0, 0) decodes to, the
value of the scene's corner of zeros; 32767 is a value the scene does not hold.  ``nodata_share_band0`` reports how much
of band 0 is X.

    python tools/bench_decode.py --resample 1373,1373 --nodata corner --steps 5 --warmup 2

``--compare`` times the comparison of the scene's container with its own synthetic raster, resident on the device
(``fra_decode_device_compare``: the whole raster decoded with ``pcm16`` semantics to uint16 and compared there, only the
reports come back), against the plain windowed read of the same region to a device destination in the same run
(``plain_wall_ms`` / ``plain_ms`` against ``compare_wall_ms`` / the inner read + ``k_compare_ms``).  ``k_compare_ms`` is
the HIP-event time of ``k_compare`` + ``k_compare_fold`` and ``k_compare_TBps`` = (bytes of both rasters read) / that
time.  The synthetic raster's rows (10980 uint16) are not 16-byte aligned, so that call reads element by element;
``aligned`` repeats it against a copy of the raster with rows padded to 16 bytes (16-byte loads).  Both must give the
same reports, and band 0 must equal ``compare.compare_arrays`` of the plain read and the raster.  The other legs are
skipped.

    python tools/bench_decode.py --compare --steps 5 --warmup 2

``--calc EXPR`` times band math over the same container (``fra_decode_device_calc``: the whole raster decoded into a
per-call buffer, then ``k_calc``) beside the plain read and beside ``k_stats`` without a histogram -- a streaming kernel's
achieved bandwidth in the same session.  One expression per output band separated by ``;``, optionally ``:dtype``
(default ``--dtype``); ``--calc`` may be repeated, each one a leg of the same run; ``--nodata corner`` masks with what
pixel (0, 0) decodes to.  Per leg ``calc_wall_ms``, the inner read, ``k_calc_ms`` (HIP events), the bytes read (the bands
the program reads, once) and written, and ``k_calc_TBps``.  It exits non-zero unless the first and last 256 rows equal
``calc.calc_arrays`` of the plain read byte for byte.

    python tools/bench_decode.py --calc "(b4-b3)/(b4+b3)" --calc "b1" --steps 5 --warmup 2

``--focal OP[:SIZE]`` times a focal operation over the same container (``fra_decode_device_focal``: the whole raster
decoded into a per-call buffer, then ``k_focal`` over all four bands) in the same run, beside the plain read and the
``--calc`` legs: with ``--calc b1`` every focal leg also reports ``over_calc_copy_per_band``, its time per band over
``k_calc``'s one-band copy, which moves the same bytes per band and shares nothing between pixels.  It exits non-zero
unless the top left and the bottom right 1024-column corners of the result equal ``focal.focal_arrays`` of the plain read
byte for byte.  ``--dem`` runs the focal legs over a synthetic 16384 x 16384 int16 DEM on the device instead
(``fra_focal``: ``k_focal`` alone).

    python tools/bench_decode.py --focal mean:3 --focal mean:15 --focal median:5 --calc b1 --steps 5 --warmup 2
    python tools/bench_decode.py --focal hillshade --dtype uint8 --dem --steps 5 --warmup 2

``--warp KIND`` times a warped read of the same container onto a grid of the scene's own size
(``fra_decode_device_warped``: the source window decoded into a per-call buffer, then ``k_warp`` over all four bands) in the
same run, beside the plain read and the ``--calc`` legs, once per mode of ``--warp-resampling``: ``rotate:DEG`` about the
centre, ``shift:DX,DY``, or ``mercator`` (UTM 33 N to EPSG:3857 through ``warp.fit_grid``).  Per leg ``k_warp_ms`` (HIP
events), the bytes read and written, the ``staged`` / ``gathered`` workgroups and, with ``--calc b1:uint16``,
``over_calc_copy_per_band``.  It exits non-zero unless three 64 x 512 rectangles of the result equal ``warp.warp_arrays``
of the plain read byte for byte.  With ``--nodata X`` (a value of the scene's uint16, or ``corner``) the legs run the
masked ``k_warp`` and are checked against ``warp_arrays`` with that value.  ``FRA_LIB_PATH`` set to the ``warpgather`` diagnostic build times the kernel without its
staged path.

    python tools/bench_decode.py --warp shift:0.5,0.5 --warp rotate:10 --warp mercator --calc b1:uint16 --steps 5 --warmup 2

``--stats`` times the band statistics of the same container (``fra_decode_device_stats``: the whole raster decoded
with ``pcm16`` semantics to uint16 and described there, only the reports and the histogram come back) in five legs: the
plain read to a device destination, ``bins = 0`` (one pass), 256 bins over the automatic range (two passes), the exact
65536-bin histogram (one pass, and one more per further window of 8192 bins that a band's values reach), and the kernels alone (``fra_stats``) on a
constant raster on the device, with 256 bins and with 65536 -- the worst case for same-address atomics.  Per leg ``stats_wall_ms``, the
inner read, ``k_stats_ms`` (HIP events over both passes and folds) and ``k_stats_TBps`` = bytes read by the passes /
that time; ``band_reads`` counts them: a band is read once per pass and once more per further window of 8192 bins that
its values reach (the launches of the other windows leave without reading).  It exits non-zero unless band 0 of every leg equals ``stats.stats_arrays`` of the plain read.

    python tools/bench_decode.py --stats --steps 5 --warmup 2

``--rasterize KIND`` times the polygon rasterizer (``fra_rasterize``: the edge table and band lists on the host, then
``k_rasterize`` and its fold) over the scene's grid into a device-resident uint16 raster, ``--rasterize`` may be repeated.
``blocks:N`` burns the N x N squares of ``--zonal blocks:N`` as four-edge polygons (feature i burns zone i) and exits
non-zero unless the result equals that pattern's block raster exactly; ``circle:V`` burns one V-gon inscribed in the scene
-- every band then holds edges of one feature, over several chunks of the kernel -- and is checked on three 64 x 512
rectangles against ``rasterize.rasterize_arrays``.  Per leg ``k_rasterize_ms`` (``fra_rasterize_timing``), the call's wall
time (host binning and uploads included), the features, the edges of the band lists and the longest list.  Beside them,
in the same session, the plain read, ``k_calc``'s one-band uint16 copy and, with ``--zonal blocks:N``, ``k_zonal_ms`` of
``fra_decode_device_zonal`` over the labels just burned, which never leave the device.

    python tools/bench_decode.py --rasterize blocks:256 --zonal blocks:256 --rasterize circle:100000 --steps 5 --warmup 2

``--proximity KIND[:MAXDIST]`` times the proximity unit (``fra_proximity``) over the scene's grid, from a device-resident
uint16 target raster into a device-resident float32 ``dist``, and may be repeated: ``blocks:N`` (the outlines of the N x N
squares the rasterize benchmark burns), ``single`` (one target pixel in the centre), ``random:P`` (a share P of the pixels),
``all`` and ``none``; a further ``:MAXDIST`` limits the reach in pixels.  Per leg the two phase times (``cols_ms``,
``rows_ms``: ``fra_proximity_timing``), their sum against the floor of 10 bytes per pixel (``floor_gb_per_s``) and against
``k_calc``'s one-band uint16 -> float32 copy of the same run.  It exits non-zero unless a 64 x 512 rectangle through the
centre equals ``proximity.proximity_arrays`` wherever the nearest target lies within 160 pixels.  No container is built.

    python tools/bench_decode.py --proximity blocks:256 --proximity single --proximity random:0.01 --proximity all --proximity none --steps 5 --warmup 2

``--regions KIND`` times the regions unit (``fra_regions``) over the scene's grid, from a device-resident uint16 mask
into device-resident uint32 labels: ``none``, ``all``, ``blocks:N``, ``checker``, ``random:P[:4|8]`` or ``spiral``.  Per
kind: the four phase times (``fra_regions_timing``: links, tiles, seams, and everything after them), their sum against
the floor of 16 bytes per pixel and against a one-band ``k_calc`` copy uint16 -> uint16 of the same run.  The counts are
checked where the kind fixes them, the labels against the mask, and a corner crop against ``regions.regions_arrays``.

    python tools/bench_decode.py --regions none --regions all --regions blocks:256 --regions checker --regions random:0.59:4 --regions spiral --steps 5 --warmup 2

``--zonal PATTERN`` times the zonal statistics of the same container (``fra_decode_device_zonal``: the whole raster
decoded to uint16 and reduced per zone there, only the records come back) over a uint16 zone raster synthesised on the
host and resident on the device: ``blocks:N`` (squares of N x N pixels, ``blocks:256`` = 43 x 43 = 1849 zones),
``const`` (one zone: every update to one address) or ``random:N`` (a label in 0 ... N - 1 per pixel: no runs).  Beside
it, in the same session, the plain read and ``k_stats`` without a histogram.  ``k_zonal_ms`` is ``fra_zonal_timing``
(HIP events over every launch).  A workgroup's chunk of rows is read once per window of 512 zones between the smallest
and the largest zone that occurs in it: ``launches`` is that count for the widest chunk, ``bytes_moved`` the sum over
the chunks of (the values + the zone raster once per band), plus the zone raster once for the range pass, and
``k_zonal_TBps`` their quotient.  It exits non-zero unless the counts and sums of band 0 equal ``np.bincount`` over the plain read.

    python tools/bench_decode.py --zonal blocks:256 --steps 5 --warmup 2
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "flac-raster_amd"))

from flac_raster import _native as N  # noqa: E402
from flac_raster.compare import compare_arrays, report_from_bands  # noqa: E402
from flac_raster.geo import Affine  # noqa: E402
from flac_raster.resample import FACTORS, RESAMPLING, RESAMPLING_ANY, decimate, decimated_shape, resample  # noqa: E402
from flac_raster.streaming import assemble_streaming, read_overview, read_window, streaming_to_raster  # noqa: E402
from flac_raster.tiles import calculate_tiles, streams_from  # noqa: E402

SEED = 20240607
B, H, W, TILE, LEVEL = 4, 10980, 10980, 1024, 5


def host_decode_all(streams) -> int:
    """fra_decode on every stream (no copy of the samples into numpy); returns the samples decoded."""
    L = N.load()
    total = 0
    for s in streams:
        buf = np.frombuffer(s, dtype=np.uint8)
        info = N.Decoded()
        ptr = C.POINTER(C.c_int32)()
        N._check(L.fra_decode(buf.ctypes.data_as(C.c_void_p), buf.size, 0, C.byref(info), C.byref(ptr)))
        total += info.nsamples * info.channels
        L.fra_free(ptr)
    return total


def focal_spec_of(text, nodata=None):
    """The ``focal.Spec`` of a ``--focal`` leg: ``OP[:SIZE]``; the terrain ops with 10 m pixels."""
    from flac_raster.focal import Spec, hillshade_params, slope_params

    op, _, size = text.partition(":")
    kh, _, kw = (size or "3").lower().partition("x")
    size = (int(kh), int(kw or kh))
    if op == "laplace":
        return Spec("convolve", nodata=nodata, weights=[[0, -1, 0], [-1, 4, -1], [0, -1, 0]])
    if op == "hillshade":
        return Spec(op, 3, nodata=nodata, params=hillshade_params(315.0, 45.0, 1.0, 10.0, 10.0, 255.0))
    if op == "slope":
        return Spec(op, 3, nodata=nodata, params=slope_params(1.0, 10.0, 10.0, 100.0))
    return Spec(op, size, nodata=nodata)


def focal_over_dem(ctx, args):
    """``--focal ... --dem``: k_focal alone (``fra_focal``) over a synthetic DEM resident on the device."""
    from flac_raster.focal import focal_arrays

    n, dt, odt = 16384, np.dtype(np.int16), np.dtype(args.dtype)
    dem = ctx.alloc(n * n * dt.itemsize)
    ctx.synth(3, SEED, 1, n, n, dem)
    out = ctx.alloc(n * n * odt.itemsize)
    rows, cw = 128, 1024
    top = np.empty((rows, n), dt)
    ctx.d2h(top, dem)
    res = {"workload": f"focal over a C3-like {n}x{n}x1 int16 DEM on the device, k_focal alone", "steps": args.steps,
           "warmup": args.warmup, "checked_windows_equal_focal_arrays": True, "legs": []}
    for text in args.focal:
        spec = focal_spec_of(text, None if args.nodata in (None, "corner") else args.nodata)
        kf, wall = [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            _, left = ctx.focal(dem, spec, odt, dst=out, dtype=dt, shape=(1, n, n))
            t1 = time.perf_counter()
            if s >= args.warmup:
                kf.append(ctx.focal_timing())
                wall.append((t1 - t0) * 1e3)
        ry, rx = spec.kh // 2, spec.kw // 2
        want, _ = focal_arrays(top[None, :, :cw + rx], spec, odt, (0, 0, rows - ry, cw))
        got = np.empty((1, rows - ry, cw), odt)
        for r in range(rows - ry):
            ctx.d2h(got[0, r], out + r * n * odt.itemsize)
        if got.tobytes() != want.tobytes():
            raise SystemExit(f"focal {text}: the top left window differs from focal_arrays")
        med = statistics.median
        rd, wr = n * n * dt.itemsize, n * n * odt.itemsize
        res["legs"].append({"focal": text, "window": [spec.kh, spec.kw], "dtype": str(odt), "left_out": int(left[0]),
                            "k_focal_ms": round(med(kf), 4), "focal_wall_ms": round(med(wall), 3),
                            "k_focal_TBps": round((rd + wr) / (med(kf) * 1e-3) / 1e12, 3),
                            "all_ms": {"k_focal": [round(v, 4) for v in kf]}})
    print(json.dumps(res), flush=True)
    ctx.free(out)
    ctx.free(dem)


def proximity_source(kind, arg):
    """The uint16 target raster of a ``--proximity`` kind over the scene's grid."""
    a = np.zeros((H, W), np.uint16)
    if kind == "blocks":
        n = int(arg or 256)
        a[::n, :] = 1 + (np.arange(W) // n % 60000).astype(np.uint16)[None, :]
        a[:, ::n] = 1 + (np.arange(H) // n % 60000).astype(np.uint16)[:, None]
    elif kind == "single":
        a[H // 2, W // 2] = 7
    elif kind == "random":
        rng = np.random.default_rng(SEED)
        m = rng.random((H, W)) < float(arg or 0.01)
        a[m] = rng.integers(1, 65536, int(m.sum()))
    elif kind == "all":
        a[:] = 1 + (np.arange(W) % 60000).astype(np.uint16)[None, :]
    elif kind != "none":
        raise SystemExit("--proximity takes blocks:N, single, random:P, all or none")
    return a


def proximity_over_grid(ctx, args):
    """``--proximity``: the two phases of ``fra_proximity`` per kind, against the 10 B/pixel floor (a uint16 source, the
    16-bit intermediate written and read, a float32 dist) and against a one-band ``k_calc`` copy uint16 -> float32."""
    from flac_raster.calc import compile_exprs
    from flac_raster.proximity import Options, proximity_arrays

    med = statistics.median
    d_src, d_dist = ctx.alloc(H * W * 2), ctx.alloc(H * W * 4)
    copy = compile_exprs(["b1"], 1)
    res = {"workload": f"proximity over the C4-like grid {W}x{H}: uint16 source and float32 dist resident on the device",
           "steps": args.steps, "warmup": args.warmup, "floor_bytes_per_pixel": 10, "legs": []}
    kcopy = []
    for spec in args.proximity:
        parts = spec.split(":")
        kind = parts[0]
        arg = parts[1] if len(parts) > 1 and kind in ("blocks", "random") else None
        rest = parts[2:] if kind in ("blocks", "random") else parts[1:]
        opts = Options(max_dist=float(rest[0])) if rest else Options()
        src = proximity_source(kind, arg)
        ctx.h2d(d_src, src)
        if not kcopy:
            for s in range(args.warmup + args.steps):
                ctx.calc(d_src, copy, np.float32, d_dist, dtype=np.uint16, shape=(1, H, W))
                if s >= args.warmup:
                    kcopy.append(ctx.calc_timing())
            res["k_calc_copy_uint16_to_float32_ms"] = round(med(kcopy), 4)
        wall, cols, rows = [], [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            _, _, counts = ctx.proximity(d_src, opts, np.float32, d_dist, False, dtype=np.uint16, shape=(1, H, W))
            t1 = time.perf_counter()
            if s >= args.warmup:
                ms = ctx.proximity_timing()
                wall.append((t1 - t0) * 1e3), cols.append(ms[0]), rows.append(ms[1])
        # a band of rows through the centre against the numpy rule over the band grown by 160 pixels: wherever the rule finds
        # a target within 160 pixels, that target is the nearest of the whole grid too
        r0, c0, hh, ww, grow = H // 2 - 32, W // 2 - 256, 64, 512, 160
        got = np.empty((hh, W), np.float32)
        ctx.d2h(got, d_dist + r0 * W * 4)
        want = proximity_arrays(src[r0 - grow:r0 + hh + grow, c0 - grow:c0 + ww + grow], opts, (grow, grow, hh, ww))[0][0]
        near = want <= grow
        if not np.array_equal(got[:, c0:c0 + ww][near], want[near]) or (kind != "none" and not near.any()):
            raise SystemExit(f"proximity {spec}: rows {r0} ..., columns {c0} ... differ from proximity_arrays")
        if kind == "none" and not (np.isnan(got).all() and int(counts[0]) == 0):
            raise SystemExit("proximity none: a pixel within reach")
        total = med(cols) + med(rows)
        res["legs"].append({
            "proximity": spec, "targets": int(counts[0]), "within_reach": int(counts[1]),
            "cols_ms": round(med(cols), 4), "rows_ms": round(med(rows), 4), "total_ms": round(total, 4),
            "wall_ms": round(med(wall), 3), "floor_gb_per_s": round(10 * H * W / total / 1e6, 1),
            "total_over_calc_copy": round(total / med(kcopy), 2), "checked_pixels_equal_proximity_arrays": int(near.sum()),
            "all_ms": {"cols": [round(x, 4) for x in cols], "rows": [round(x, 4) for x in rows]}})
    print(json.dumps(res), flush=True)
    ctx.free(d_src)
    ctx.free(d_dist)


def regions_source(kind, arg):
    """The uint16 mask of a ``--regions`` kind over the scene's grid, and what its counts must be (``None``: unknown)."""
    a = np.zeros((H, W), np.uint16)
    expect = None
    if kind == "all":
        a[:] = 1
        expect = [H * W, 1, 1, H * W]
    elif kind == "blocks":
        n = int(arg or 256)
        a[:] = 1
        a[n - 1::n, :] = 0
        a[:, n - 1::n] = 0
        fg = int(a.sum())
        ncomp = ((H + n - 1) // n) * ((W + n - 1) // n) if n > 1 else 0
        expect = [fg, ncomp, ncomp, fg]
    elif kind == "checker":
        a[:] = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0
        fg = int(a.sum())
        expect = [fg, fg, fg, fg]
    elif kind == "random":
        a[:] = np.random.default_rng(SEED).random((H, W)) < float(arg or 0.59)
    elif kind == "spiral":  # one 4-connected path of one pixel's width: the frames at every second inset, each cut
        k = 0               # below its top left corner and joined to the next one
        while k < min(H, W) - k:
            a[k, k:W - k] = a[H - 1 - k, k:W - k] = 1
            a[k:H - k, k] = a[k:H - k, W - 1 - k] = 1
            if k + 2 < min(H, W) - k - 2:
                a[k + 1, k] = 0
                a[k + 2, k + 1] = 1
            k += 2
        fg = int(a.sum())
        expect = [fg, 1, 1, fg]
    elif kind == "none":
        expect = [0, 0, 0, 0]
    else:
        raise SystemExit("--regions takes none, all, blocks:N, checker, random:P[:4|8] or spiral")
    return a, expect


def regions_over_grid(ctx, args):
    """``--regions``: the four phases of ``fra_regions`` per kind -- a resident uint16 mask into resident uint32 labels --
    against the floor of 16 bytes per pixel (the source read, the link byte written and read, the parent written and
    read, the labels written) and against a one-band ``k_calc`` copy uint16 -> uint16 of the same run."""
    from flac_raster.calc import compile_exprs
    from flac_raster.regions import Options, regions_arrays

    med = statistics.median
    d_src, d_lab, d_copy = ctx.alloc(H * W * 2), ctx.alloc(H * W * 4), ctx.alloc(H * W * 2)
    copy = compile_exprs(["b1"], 1)
    res = {"workload": f"regions over the C4-like grid {W}x{H}: uint16 mask and uint32 labels resident on the device",
           "steps": args.steps, "warmup": args.warmup, "floor_bytes_per_pixel": 16, "legs": []}
    kcopy = []
    for spec in args.regions:
        parts = spec.split(":")
        kind = parts[0]
        arg = parts[1] if len(parts) > 1 else None
        conn = int(parts[2]) if len(parts) > 2 else 4
        opts = Options(connectivity=conn)
        src, expect = regions_source(kind, arg)
        ctx.h2d(d_src, src)
        if not kcopy:
            for s in range(args.warmup + args.steps):
                ctx.calc(d_src, copy, np.uint16, d_copy, dtype=np.uint16, shape=(1, H, W))
                if s >= args.warmup:
                    kcopy.append(ctx.calc_timing())
            res["k_calc_copy_uint16_to_uint16_ms"] = round(med(kcopy), 4)
        wall, phases = [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            counts = ctx.regions(d_src, opts, np.uint32, labels=d_lab, dtype=np.uint16, shape=(1, H, W))[4]
            t1 = time.perf_counter()
            if s >= args.warmup:
                wall.append((t1 - t0) * 1e3), phases.append(ctx.regions_timing())
        got = counts[0].tolist()
        if expect is not None and got != expect:
            raise SystemExit(f"regions {spec}: counts {got}, expected {expect}")
        lab = np.empty((H, W), np.uint32)
        ctx.d2h(lab, d_lab)
        if not np.array_equal(lab > 0, src > 0) or int(lab.max()) != got[2] or got[3] != got[0]:
            raise SystemExit(f"regions {spec}: the labels do not cover the mask with 1 .. N")
        # a corner crop: the rule's components of the crop are pieces of the grid's, so each lies in exactly one label
        crop = 512
        piece = regions_arrays(src[None, :crop, :crop], opts, np.int32, None)[0][0]
        pairs = np.unique(np.stack([piece[piece > 0], lab[:crop, :crop][piece > 0].astype(np.int64)], axis=1), axis=0)
        if pairs.shape[0] != int(piece.max()):
            raise SystemExit(f"regions {spec}: a component of the corner crop is split over several labels")
        ph = [med([p[k] for p in phases]) for k in range(4)]
        total = sum(ph)
        worst = max(range(4), key=lambda k: ph[k])
        res["legs"].append({
            "regions": spec, "connectivity": conn, "counts": got,
            "links_ms": round(ph[0], 4), "tiles_ms": round(ph[1], 4), "seams_ms": round(ph[2], 4), "rest_ms": round(ph[3], 4),
            "total_ms": round(total, 4), "wall_ms": round(med(wall), 3), "floor_gb_per_s": round(16 * H * W / total / 1e6, 1),
            "total_over_calc_copy": round(total / med(kcopy), 2), "longest_phase": ("links", "tiles", "seams", "rest")[worst],
            "all_ms": [[round(x, 4) for x in p] for p in phases]})
    print(json.dumps(res), flush=True)
    for d in (d_src, d_lab, d_copy):
        ctx.free(d)


def warp_map_of(text):
    """The ``warp.Map`` of a ``--warp`` leg over the scene at its own size, and a word about it."""
    import math

    from flac_raster import crs
    from flac_raster import warp as WP

    kind, _, arg = text.partition(":")
    if kind == "rotate":
        c, s = math.cos(math.radians(float(arg))), math.sin(math.radians(float(arg)))
        cx, cy = W / 2.0, H / 2.0
        return WP.affine_coefficients((c, -s, cx - (c * cx - s * cy), s, c, cy - (s * cx + c * cy))), f"rotation by {arg} deg"
    if kind == "shift":
        dx, dy = (float(v) for v in arg.split(","))
        return WP.affine_coefficients((1.0, 0.0, dx, 0.0, 1.0, dy)), f"shift by ({dx}, {dy})"
    if kind == "mercator":
        st = (10.0, 0.0, 399960.0, 0.0, -10.0, 4600020.0)  # a Sentinel-2 tile of UTM zone 33 N
        dt_, _ = crs.suggested_grid(st, (H, W), crs.transformer("EPSG:32633", "EPSG:3857"))
        back = crs.transformer("EPSG:3857", "EPSG:32633")

        def pixel(cols, rows):
            x, y = back(dt_.a * cols + dt_.c, dt_.e * rows + dt_.f)
            return (x - st[2]) / st[0], (y - st[5]) / st[4]

        m, err = WP.fit_grid(pixel, (H, W))
        return m, f"UTM 33 N -> EPSG:3857, grid step {m.step}, error {err:.4f} px"
    raise SystemExit(f"--warp {text!r}: rotate:DEG, shift:DX,DY or mercator")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=0, help="first N tiles of the scene (0: all 121)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-steps", type=int, default=1, help="timed passes of the host decoder (it is slow)")
    ap.add_argument("--no-e2e", action="store_true", help="skip the container leg")
    ap.add_argument("--window", nargs="?", const="center", default=None, metavar="r,c,h,w",
                    help="time a windowed read against the full decode (default window: 2048 x 2048 at the centre)")
    ap.add_argument("--verify", action="store_true", help="time fra_plan_verify against the plain decode")
    ap.add_argument("--decimate", type=int, default=0, metavar="K", choices=(0,) + FACTORS,
                    help="time the decimated read of the whole raster at 1/K against the full decode")
    ap.add_argument("--resampling", default="average", choices=tuple(RESAMPLING_ANY),
                    help="with --decimate (nearest or average) or --resample (any)")
    ap.add_argument("--resample", default=None, metavar="H,W",
                    help="time the read of the region resampled to H x W against the full decode")
    ap.add_argument("--region", default=None, metavar="r,c,h,w", help="with --resample: the region (default: all)")
    ap.add_argument("--nodata", default=None, metavar="X",
                    help="with --decimate or --resample: the nodata-aware read with this value of the decoded int16 "
                         "('corner': what pixel (0, 0) decodes to); with --calc, --focal or --warp: of the scene's uint16")
    ap.add_argument("--compare", action="store_true",
                    help="time the comparison of the container with its source raster against the plain read")
    ap.add_argument("--stats", action="store_true",
                    help="time the band statistics and histograms of the container against the plain read")
    ap.add_argument("--zonal", default=None, metavar="PATTERN",
                    help="time fra_decode_device_zonal over a synthetic zone raster: blocks:N, const or random:N")
    ap.add_argument("--rasterize", action="append", default=None, metavar="KIND",
                    help="time fra_rasterize over the scene's grid into a resident uint16 raster: blocks:N (the squares of "
                         "--zonal blocks:N as polygons) or circle:V (one V-gon inscribed in the scene); with --zonal "
                         "blocks:N the zonal statistics then run over the burned labels")
    ap.add_argument("--proximity", action="append", default=None, metavar="KIND[:MAXDIST]",
                    help="time fra_proximity over the scene's grid, a resident uint16 source into a resident float32 dist: "
                         "blocks:N (the outlines of the N x N squares), single (one target pixel), random:P (a share P of "
                         "the pixels), all, none; KIND:...:MAXDIST limits the reach, e.g. blocks:256:64 (repeatable)")
    ap.add_argument("--regions", action="append", default=None, metavar="KIND",
                    help="time fra_regions over the scene's grid, a resident uint16 mask into resident uint32 labels: none, "
                         "all, blocks:N (squares of N x N with a background line between them), checker, random:P[:4|8] (a "
                         "share P of the pixels, 4- or 8-connected) or spiral (repeatable); the k_calc copy of the same run "
                         "is timed beside them, so a --calc leg is not needed")
    ap.add_argument("--calc", action="append", default=None, metavar="EXPR",
                    help="time band math over the container against the plain read: one expression per output band, "
                         "separated by ';', optionally followed by ':dtype'; repeat for further legs of the same run")
    ap.add_argument("--focal", action="append", default=None, metavar="OP[:SIZE]",
                    help="time a focal operation over the container against the plain read (and against the --calc legs "
                         "of the same run): mean, sum, min, max, count, median, laplace (a 3 x 3 convolution), slope or "
                         "hillshade, SIZE one odd number or HxW (default 3); repeat for further legs")
    ap.add_argument("--warp", action="append", default=None, metavar="KIND",
                    help="time a warped read of the container onto a grid of the scene's own size against the plain read "
                         "(and against the --calc legs of the same run): rotate:DEG (about the centre), shift:DX,DY or "
                         "mercator (UTM 33 N -> EPSG:3857 through a fitted coordinate grid); may be repeated")
    ap.add_argument("--warp-resampling", default="bilinear,nearest", help="with --warp: the modes of every leg")
    ap.add_argument("--dem", action="store_true",
                    help="with --focal: k_focal alone over a synthetic 16384 x 16384 int16 DEM on the device instead")
    ap.add_argument("--dtype", default="float32", help="with --calc or --focal: the output dtype of the legs that name none")
    args = ap.parse_args()
    if args.decimate and args.resampling not in RESAMPLING:
        ap.error("--decimate takes --resampling nearest or average")
    if args.nodata is not None and not (args.decimate or args.resample or args.calc or args.focal or args.warp):
        ap.error("--nodata goes with --decimate, --resample, --calc, --focal or --warp")
    if args.dem and not args.focal:
        ap.error("--dem goes with --focal")
    if args.nodata not in (None, "corner"):
        args.nodata = float(args.nodata)

    ctx = N.Context(0)
    if args.dem:
        focal_over_dem(ctx, args)
        return
    if args.proximity:
        proximity_over_grid(ctx, args)
        return
    if args.regions:
        regions_over_grid(ctx, args)
        return
    dt = np.dtype(np.uint16)
    dev_raster = ctx.alloc(B * H * W * dt.itemsize)
    ctx.synth(4, SEED, B, H, W, dev_raster)
    wins = calculate_tiles(H, W, TILE)
    if args.tiles:
        wins = wins[: args.tiles]
    plan = N.Plan(ctx, dev_raster, True, dt, B, (H * W, W, 1), wins, LEVEL, 4096, 16)
    plan.execute()
    plan.sync()
    infos, total = plan.result()
    nfr = sum(i.nframes for i in infos)
    off = plan.frame_offsets(nfr)
    frames_ptr, _ = plan.device_output()
    samples = sum(w[2] * w[3] for w in wins) * B
    dev_out = ctx.alloc(B * H * W * 2)  # int16 samples, laid out like the raster

    # ---- device, offsets supplied, everything resident
    items, f0 = [], 0
    for inf, w in zip(infos, wins):
        items.append({"offset": inf.offset, "bytes": inf.frame_bytes, "window": w,
                      "frame_offsets": off[f0:f0 + inf.nframes + 1] - np.uint64(inf.offset),
                      "channels": inf.channels, "bps": inf.bps, "blocksize": 4096})
        f0 += inf.nframes
    dev_ms, dev_wall, kern = [], [], []
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        ctx.decode_device((frames_ptr, total), items, dev_out, np.int16, B, (H * W, W, 1))
        t1 = time.perf_counter()
        if k >= args.warmup:
            ms = ctx.decode_timing()
            dev_ms.append(ms[3])
            kern.append(ms[:3])
            dev_wall.append((t1 - t0) * 1e3)
    corner = args.nodata == "corner"
    if corner:
        first = np.empty(1, np.int16)
        ctx.d2h(first, dev_out)
        args.nodata = float(first[0])
    nd = {} if args.nodata is None else {"nodata": args.nodata}  # the keyword of the nodata-aware reads and rules

    if args.verify:
        ver_wall, ver_ms, ver_kern = [], [], []
        for k in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            reports = plan.verify()
            t1 = time.perf_counter()
            if any(r.mismatches for r in reports) or sum(r.nframes for r in reports) != nfr:
                raise SystemExit("verify: the plan's frames differ from its raster")
            if k >= args.warmup:
                ms = ctx.decode_timing()
                ver_wall.append((t1 - t0) * 1e3)
                ver_ms.append(ms[3])
                ver_kern.append(ms[:3])
        enc_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            plan.execute()
            plan.sync()
            enc_ms.append((time.perf_counter() - t0) * 1e3)
        # one changed pixel (tile 60, band 2) is the one mismatch reported
        t = min(60, len(wins) - 1)
        r0, c0, _, tw = wins[t]
        px = np.empty(1, dt)
        at = dev_raster + ((2 * H + r0 + 5) * W + c0 + 7) * dt.itemsize
        ctx.d2h(px, at)
        ctx.h2d(at, px ^ 0x10)
        reports = plan.verify()
        bad = [(i, r.mismatches, r.first_sample, r.first_channel) for i, r in enumerate(reports) if r.mismatches]
        if bad != [(t, 1, 5 * tw + 7, 2)]:
            raise SystemExit(f"verify: changed pixel of tile {t} reported as {bad}")
        med = statistics.median
        names = ("k_dec_parse_ms", "k_dec_restore_ms")
        res = {
            "workload": f"verify C4-like {W}x{H}x{B} uint16, tile {TILE}, level {LEVEL}, {len(wins)} tiles",
            "tiles": len(wins), "frames": nfr, "samples": samples, "frame_bytes": total,
            "steps": args.steps, "warmup": args.warmup, "changed_pixel_found": True,
            "encode_ms": round(med(enc_ms), 3),
            "device_ms": round(med(dev_ms), 3), "device_wall_ms": round(med(dev_wall), 3),
            "verify_ms": round(med(ver_ms), 3), "verify_wall_ms": round(med(ver_wall), 3),
            "kernels_decode": dict({n: round(med([k[i] for k in kern]), 3) for i, n in enumerate(names)},
                                   k_dec_scatter_ms=round(med([k[2] for k in kern]), 3)),
            "kernels_verify": dict({n: round(med([k[i] for k in ver_kern]), 3) for i, n in enumerate(names)},
                                   k_dec_verify_ms=round(med([k[2] for k in ver_kern]), 3)),
            "all_ms": {"device": [round(v, 3) for v in dev_ms], "verify": [round(v, 3) for v in ver_ms],
                       "verify_wall": [round(v, 3) for v in ver_wall],
                       "k_dec_scatter": [round(k[2], 3) for k in kern],
                       "k_dec_verify": [round(k[2], 3) for k in ver_kern]},
        }
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    if args.compare:
        if len(wins) != len(calculate_tiles(H, W, TILE)):
            raise SystemExit("--compare needs every tile: the region compared is the whole raster")
        roi = (0, 0, H, W)
        citems = [dict(it, data_min=inf.data_min, data_max=inf.data_max) for it, inf in zip(items, infos)]
        plain_wall, plain_ms = [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ctx.decode_device_window((frames_ptr, total), citems, dev_out, dt, B, (H * W, W, 1), roi, N.DENORM_PCM16)
            t1 = time.perf_counter()
            if s >= args.warmup:
                plain_wall.append((t1 - t0) * 1e3)
                plain_ms.append(ctx.decode_timing()[3])
        raster = np.empty((B, H, W), dt)
        ctx.d2h(raster, dev_raster)
        decoded = np.empty((B, H, W), dt)
        ctx.d2h(decoded, dev_out)
        want = compare_arrays(decoded[:1], raster[:1])["bands"][0]
        del decoded
        rs = -(-W // 8) * 8  # rows on 16-byte boundaries
        padded = np.zeros((B, H, rs), dt)
        padded[:, :, :W] = raster
        del raster
        dev_padded = ctx.alloc(padded.nbytes)
        ctx.h2d(dev_padded, padded)
        del padded
        legs = {}
        for name, ref, strides in (("as_is", dev_raster, (H * W, W, 1)), ("aligned", dev_padded, (H * rs, rs, 1))):
            wall, inner, kc = [], [], []
            for s in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                bands, _ = ctx.decode_device_compare((frames_ptr, total), citems, ref, dt, B, roi, N.DENORM_PCM16,
                                                     ref_strides=strides)
                t1 = time.perf_counter()
                if s >= args.warmup:
                    wall.append((t1 - t0) * 1e3)
                    inner.append(ctx.decode_timing()[3])
                    kc.append(ctx.compare_timing())
            legs[name] = (wall, inner, kc, b"".join(bytes(r) for r in bands), report_from_bands(bands, dt))
        ctx.free(dev_padded)
        if legs["as_is"][3] != legs["aligned"][3]:
            raise SystemExit("compare: element loads and 16-byte loads give different reports")
        rep = legs["as_is"][4]
        if rep["bands"][0] != want:
            raise SystemExit(f"compare: band 0 differs from compare_arrays: {rep['bands'][0]} != {want}")
        med = statistics.median
        moved = 2 * B * H * W * dt.itemsize
        res = {
            "workload": f"compare C4-like {W}x{H}x{B} uint16 (pcm16), tile {TILE}, level {LEVEL}, {len(wins)} tiles, "
                        "whole raster against its source on the device",
            "tiles": len(wins), "frames": nfr, "steps": args.steps, "warmup": args.warmup,
            "band0_equals_compare_arrays": True, "reports_equal_on_both_paths": True,
            "differing": rep["differing"], "max_difference": rep["max_difference"],
            "mean_difference": rep["mean_difference"], "rmse": rep["rmse"],
            "plain_ms": round(med(plain_ms), 3), "plain_wall_ms": round(med(plain_wall), 3),
            "k_compare_bytes": moved, "region_buffer_bytes": B * H * rs * dt.itemsize,
        }
        for name, (wall, inner, kc, _, _) in legs.items():
            res[name] = {"compare_wall_ms": round(med(wall), 3), "inner_read_ms": round(med(inner), 3),
                         "k_compare_ms": round(med(kc), 4), "k_compare_TBps": round(moved / (med(kc) * 1e-3) / 1e12, 3),
                         "wall_over_plain": round(med(wall) / med(plain_wall), 3),
                         "all_ms": {"k_compare": [round(v, 4) for v in kc], "compare_wall": [round(v, 3) for v in wall]}}
        res["all_ms"] = {"plain": [round(v, 3) for v in plain_ms], "plain_wall": [round(v, 3) for v in plain_wall]}
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    if args.stats:
        from flac_raster.stats import exact_range, report_from_bands as stats_report, stats_arrays

        if len(wins) != len(calculate_tiles(H, W, TILE)):
            raise SystemExit("--stats needs every tile: the region described is the whole raster")
        roi = (0, 0, H, W)
        citems = [dict(it, data_min=inf.data_min, data_max=inf.data_max) for it, inf in zip(items, infos)]
        plain_wall, plain_ms = [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ctx.decode_device_window((frames_ptr, total), citems, dev_out, dt, B, (H * W, W, 1), roi, N.DENORM_PCM16)
            t1 = time.perf_counter()
            if s >= args.warmup:
                plain_wall.append((t1 - t0) * 1e3)
                plain_ms.append(ctx.decode_timing()[3])
        decoded = np.empty((B, H, W), dt)
        ctx.d2h(decoded, dev_out)
        elo, ehi, ebins = exact_range(dt)
        med = statistics.median
        once = B * H * W * dt.itemsize
        res = {
            "workload": f"stats C4-like {W}x{H}x{B} uint16 (pcm16), tile {TILE}, level {LEVEL}, {len(wins)} tiles, "
                        "whole raster",
            "tiles": len(wins), "frames": nfr, "steps": args.steps, "warmup": args.warmup,
            "band0_equals_stats_arrays": True,
            "plain_ms": round(med(plain_ms), 3), "plain_wall_ms": round(med(plain_wall), 3), "raster_bytes": once,
        }
        def band_reads(rep, passes):
            """Reads of a band's pixels, summed over the bands: one per pass, one per further window its values reach."""
            n = 0
            for b in rep:
                n += passes
                if b["bins"] > 8192 and b["hist_range"] is not None and b["fin_min"] is not None:
                    lo, hi = b["hist_range"]
                    at = lambda x: 0 if b["hist_scale"] == 0.0 else int(min(b["bins"] - 1, (x - lo) * b["hist_scale"] // 1))  # noqa: E731
                    xa, xb = max(b["fin_min"], lo), min(b["fin_max"], hi)
                    if xa <= xb:
                        n += sum(1 for k in range(1, -(-b["bins"] // 8192)) if at(xb) >= k * 8192 and at(xa) < (k + 1) * 8192)
            return n

        for name, bins, rng, passes in (("bins0", 0, None, 1), ("bins256_auto", 256, "auto", 2),
                                        ("exact65536", ebins, (elo, ehi), 1)):
            want = stats_arrays(decoded[:1], bins, rng)[0]
            wall, inner, ks = [], [], []
            for s in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                bands, hist, _ = ctx.decode_device_stats((frames_ptr, total), citems, dt, B, roi, N.DENORM_PCM16, bins,
                                                         rng)
                t1 = time.perf_counter()
                if s >= args.warmup:
                    wall.append((t1 - t0) * 1e3)
                    inner.append(ctx.decode_timing()[3])
                    ks.append(ctx.stats_timing())
            rep_all = stats_report(bands, hist, dt)
            got = rep_all[0]
            reads = band_reads(rep_all, passes)
            if got != want:
                diff = {k: (got[k], want[k]) for k in want if k != "histogram" and got[k] != want[k]}
                raise SystemExit(f"stats {name}: band 0 differs from stats_arrays: {diff or 'in the histogram'}")
            res[name] = {"stats_wall_ms": round(med(wall), 3), "inner_read_ms": round(med(inner), 3),
                         "k_stats_ms": round(med(ks), 4), "passes": passes, "band_reads": reads,
                         "k_stats_TBps": round(reads * (once // B) / (med(ks) * 1e-3) / 1e12, 3),
                         "wall_over_plain": round(med(wall) / med(plain_wall), 3),
                         "all_ms": {"k_stats": [round(v, 4) for v in ks], "stats_wall": [round(v, 3) for v in wall]}}
        res["band0"] = {k: got[k] for k in ("valid", "min", "max", "mean", "std")}
        del decoded
        # the kernels alone on a constant raster: every pixel of a band in one bin
        const = np.full((B, H, W), 12345, dt)
        ctx.h2d(dev_out, const)
        for name, bins, rng in (("constant_256", 256, (0.0, 65536.0)), ("constant_65536", ebins, (elo, ehi))):
            ks = []
            for s in range(args.warmup + args.steps):
                bands, hist = ctx.stats(dev_out, bins, rng, dtype=dt, shape=(B, H, W), strides=(H * W, W, 1))
                if s >= args.warmup:
                    ks.append(ctx.stats_timing())
            j = 12345 * bins // 65536
            if any(int(hist[b, j]) != H * W or int(hist[b].sum()) != H * W or r.sum_lo != 12345 * H * W
                   for b, r in enumerate(bands)):
                raise SystemExit(f"stats {name}: the constant raster is not counted exactly")
            reads = band_reads(stats_report(bands, hist, dt), 1)  # 12345 lies in the second window of 65536 bins
            res[name] = {"k_stats_ms": round(med(ks), 4), "passes": 1, "band_reads": reads,
                         "k_stats_TBps": round(reads * (once // B) / (med(ks) * 1e-3) / 1e12, 3),
                         "all_ms": {"k_stats": [round(v, 4) for v in ks]}}
        res["all_ms"] = {"plain": [round(v, 3) for v in plain_ms], "plain_wall": [round(v, 3) for v in plain_wall]}
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    if args.rasterize:
        import math

        from flac_raster.calc import compile_exprs, default_fill
        from flac_raster.rasterize import edge_table, rasterize_arrays

        if len(wins) != len(calculate_tiles(H, W, TILE)):
            raise SystemExit("--rasterize needs every tile: the grid is the whole raster's")
        roi = (0, 0, H, W)
        citems = [dict(it, data_min=inf.data_min, data_max=inf.data_max) for it, inf in zip(items, infos)]
        med = statistics.median
        zdt = np.dtype(np.uint16)
        dev_zones = ctx.alloc(H * W * zdt.itemsize)
        plain_ms, kcopy = [], []
        copy = compile_exprs(["b1"], B)
        for s in range(args.warmup + args.steps):
            ctx.decode_device_window((frames_ptr, total), citems, dev_out, dt, B, (H * W, W, 1), roi, N.DENORM_PCM16)
            if s >= args.warmup:
                plain_ms.append(ctx.decode_timing()[3])
            ctx.decode_device_calc((frames_ptr, total), citems, dt, B, roi, copy, zdt, dst=dev_zones, denorm=N.DENORM_PCM16,
                                   nodata=None, fill=default_fill(zdt))
            if s >= args.warmup:
                kcopy.append(ctx.calc_timing())
        res = {
            "workload": f"rasterize onto the C4-like grid {W}x{H}, uint16 labels resident on the device",
            "steps": args.steps, "warmup": args.warmup, "plain_ms": round(med(plain_ms), 3),
            "k_calc_copy_one_band_ms": round(med(kcopy), 4), "label_raster_bytes": H * W * zdt.itemsize, "legs": [],
        }
        got = np.empty((H, W), zdt)
        for spec in args.rasterize:
            kind, _, arg = spec.partition(":")
            if kind == "blocks":
                n = int(arg or 256)
                per_row = -(-W // n)
                feats = [[[(c0, r0), (min(c0 + n, W), r0), (min(c0 + n, W), min(r0 + n, H)), (c0, min(r0 + n, H))]]
                         for r0 in range(0, H, n) for c0 in range(0, W, n)]
                values, fill = list(range(len(feats))), 65535
                if len(feats) > 65535:
                    raise SystemExit(f"--rasterize {spec}: {len(feats)} squares do not fit uint16 labels beside the fill")
            elif kind == "circle":
                v = int(arg or 100000)
                rad = 0.5 * min(H, W) - 1.0
                feats = [[[(0.5 * W + rad * math.cos(2.0 * math.pi * k / v), 0.5 * H + rad * math.sin(2.0 * math.pi * k / v))
                           for k in range(v)]]]
                values, fill = [1], 0
            else:
                raise SystemExit("--rasterize takes blocks:N or circle:V")
            wall, kr = [], []
            for s in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                _, burned = ctx.rasterize(feats, roi, values, fill, zdt, dst=dev_zones)
                t1 = time.perf_counter()
                if s >= args.warmup:
                    wall.append((t1 - t0) * 1e3)
                    kr.append(ctx.rasterize_timing())
            ctx.d2h(got, dev_zones)
            _, y0, _, y1, _ = edge_table(feats)
            first = np.clip(np.ceil(y0 - 0.5), 0, H).astype(np.int64)       # the rows whose centres an edge holds
            last = np.clip(np.ceil(y1 - 0.5) - 1, -1, H - 1).astype(np.int64)
            ok = first <= last
            lists = np.zeros(-(-H // 16) + 1, np.int64)
            np.add.at(lists, first[ok] // 16, 1)
            np.add.at(lists, last[ok] // 16 + 1, -1)
            lists = np.cumsum(lists)[:-1]
            leg = {"rasterize": spec, "features": len(feats), "edges": int(y0.size), "band_list_entries": int(lists.sum()),
                   "longest_band_list": int(lists.max()), "burned": burned, "rasterize_wall_ms": round(med(wall), 3),
                   "k_rasterize_ms": round(med(kr), 4), "k_rasterize_over_calc_copy": round(med(kr) / med(kcopy), 3),
                   "all_ms": {"k_rasterize": [round(x, 4) for x in kr], "rasterize_wall": [round(x, 3) for x in wall]}}
            if kind == "blocks":
                zones = ((np.arange(H, dtype=np.uint32)[:, None] // n) * per_row
                         + np.arange(W, dtype=np.uint32)[None, :] // n).astype(zdt)
                if burned != H * W or got.tobytes() != zones.tobytes():
                    raise SystemExit(f"rasterize {spec}: the result differs from the block raster")
                leg["equals_block_raster"] = True
                if args.zonal == spec:
                    nzones = len(feats)
                    zwall, inner, kz = [], [], []
                    for s in range(args.warmup + args.steps):
                        t0 = time.perf_counter()
                        recs, outside, _ = ctx.decode_device_zonal((frames_ptr, total), citems, dev_zones, dt, B, roi,
                                                                   N.DENORM_PCM16, 0, nzones, zone_dtype=zdt,
                                                                   zone_strides=(W, 1))
                        t1 = time.perf_counter()
                        if s >= args.warmup:
                            zwall.append((t1 - t0) * 1e3)
                            inner.append(ctx.decode_timing()[3])
                            kz.append(ctx.zonal_timing())
                    counts = np.bincount(zones.ravel(), minlength=nzones)
                    if outside != 0 or not np.array_equal(recs["count"][0], counts.astype(np.uint64)):
                        raise SystemExit(f"zonal over the burned {spec}: the zone counts differ from np.bincount")
                    leg.update({"nzones": nzones, "zonal_wall_ms": round(med(zwall), 3), "inner_read_ms": round(med(inner), 3),
                                "k_zonal_ms": round(med(kz), 4), "k_rasterize_over_k_zonal": round(med(kr) / med(kz), 3)})
                    leg["all_ms"]["k_zonal"] = [round(x, 4) for x in kz]
            else:
                for r0, c0 in ((0, W // 2 - 256), (H // 2 - 32, 0), (H - 64 - int(0.146 * H), W - 512 - int(0.146 * W) + 200)):
                    want, _ = rasterize_arrays(feats, (r0, c0, 64, 512), values, fill, zdt)
                    if got[r0:r0 + 64, c0:c0 + 512].tobytes() != want.tobytes():
                        raise SystemExit(f"rasterize {spec}: rows {r0} ..., columns {c0} ... differ from rasterize_arrays")
                leg["checked_rectangles_equal_rasterize_arrays"] = 3
            res["legs"].append(leg)
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_zones)
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    if args.zonal:
        from flac_raster.zonal import report_from_recs

        if len(wins) != len(calculate_tiles(H, W, TILE)):
            raise SystemExit("--zonal needs every tile: the region reduced is the whole raster")
        kind, _, arg = args.zonal.partition(":")
        if kind == "blocks":
            n = int(arg or 256)
            per_row = -(-W // n)
            zones = ((np.arange(H, dtype=np.uint32)[:, None] // n) * per_row + np.arange(W, dtype=np.uint32)[None, :] // n)
            nzones = per_row * -(-H // n)
        elif kind == "const":
            zones, nzones = np.zeros((H, W), np.uint32), 1
        elif kind == "random":
            nzones = int(arg or 16)
            zones = np.random.default_rng(SEED).integers(0, nzones, (H, W), dtype=np.uint32)
        else:
            raise SystemExit("--zonal takes blocks:N, const or random:N")
        if not 1 <= nzones <= 65536:
            raise SystemExit(f"--zonal {args.zonal}: {nzones} zones, 1 ... 65536 go into one call")
        zones = zones.astype(np.uint16)
        dev_zones = ctx.alloc(zones.nbytes)
        ctx.h2d(dev_zones, zones)
        roi = (0, 0, H, W)
        citems = [dict(it, data_min=inf.data_min, data_max=inf.data_max) for it, inf in zip(items, infos)]
        med = statistics.median
        plain_wall, plain_ms, ks = [], [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ctx.decode_device_window((frames_ptr, total), citems, dev_out, dt, B, (H * W, W, 1), roi, N.DENORM_PCM16)
            t1 = time.perf_counter()
            ctx.decode_device_stats((frames_ptr, total), citems, dt, B, roi, N.DENORM_PCM16, 0, None)
            if s >= args.warmup:
                plain_wall.append((t1 - t0) * 1e3)
                plain_ms.append(ctx.decode_timing()[3])
                ks.append(ctx.stats_timing())
        wall, inner, kz = [], [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            recs, outside, _ = ctx.decode_device_zonal((frames_ptr, total), citems, dev_zones, dt, B, roi, N.DENORM_PCM16,
                                                       0, nzones, zone_dtype=np.uint16, zone_strides=(W, 1))
            t1 = time.perf_counter()
            if s >= args.warmup:
                wall.append((t1 - t0) * 1e3)
                inner.append(ctx.decode_timing()[3])
                kz.append(ctx.zonal_timing())
        band0 = np.empty((H, W), dt)
        ctx.d2h(band0, dev_out)
        flat = zones.ravel()
        counts = np.bincount(flat, minlength=nzones)
        sums = np.bincount(flat, weights=band0.ravel().astype(np.float64), minlength=nzones)  # < 2^53: exact
        if (outside != 0 or not np.array_equal(recs["count"][0], counts.astype(np.uint64))
                or not np.array_equal(recs["sum_lo"][0], sums.astype(np.uint64)) or recs["sum_hi"].any()
                or not np.array_equal(recs["valid"], recs["count"])):
            raise SystemExit(f"zonal {args.zonal}: band 0 differs from np.bincount over the plain read")
        first = report_from_recs(recs[:1], outside, dt)[0]["zones"][0]
        once = B * H * W * dt.itemsize
        # the chunks of rows of fra_zonal.hip's launch (8 uint16 per slot, 4096 workgroups aimed at, 1024 slots at least)
        nvec = -(-W // 8)
        rpb = min(H, max(-(-H * B // 4096), -(-1024 // nvec)))
        moved, launches = zones.nbytes, 0
        for r0 in range(0, H, rpb):
            z = zones[r0:r0 + rpb]
            reads = -(-(int(z.max()) - int(z.min()) + 1) // 512)
            launches = max(launches, reads)
            moved += reads * z.shape[0] * W * B * (dt.itemsize + zones.itemsize)
        res = {
            "workload": f"zonal C4-like {W}x{H}x{B} uint16 (pcm16), tile {TILE}, level {LEVEL}, {len(wins)} tiles, whole "
                        f"raster, zones {args.zonal}",
            "tiles": len(wins), "frames": nfr, "steps": args.steps, "warmup": args.warmup, "pattern": args.zonal,
            "nzones": nzones, "band0_counts_and_sums_equal_bincount": True,
            "plain_ms": round(med(plain_ms), 3), "plain_wall_ms": round(med(plain_wall), 3), "raster_bytes": once,
            "zone_raster_bytes": zones.nbytes, "k_stats_ms": round(med(ks), 4),
            "k_stats_TBps": round(once / (med(ks) * 1e-3) / 1e12, 3),
            "zonal_wall_ms": round(med(wall), 3), "inner_read_ms": round(med(inner), 3), "k_zonal_ms": round(med(kz), 4),
            "launches": launches, "chunk_rows": rpb, "bytes_moved": moved, "k_zonal_TBps": round(moved / (med(kz) * 1e-3) / 1e12, 3),
            "k_zonal_over_scaled_k_stats": round(med(kz) / (med(ks) * moved / once), 3),
            "wall_over_plain": round(med(wall) / med(plain_wall), 3),
            "first_zone": {k: first[k] for k in ("zone", "valid", "min", "max", "mean", "std")},
            "all_ms": {"k_zonal": [round(v, 4) for v in kz], "zonal_wall": [round(v, 3) for v in wall],
                       "k_stats": [round(v, 4) for v in ks], "plain": [round(v, 3) for v in plain_ms]},
        }
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_zones)
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    if args.calc or args.focal or args.warp:
        from flac_raster.calc import calc_arrays, compile_exprs, default_fill

        if len(wins) != len(calculate_tiles(H, W, TILE)):
            raise SystemExit("--calc, --focal and --warp need every tile: the region mapped is the whole raster")
        roi = (0, 0, H, W)
        citems = [dict(it, data_min=inf.data_min, data_max=inf.data_max) for it, inf in zip(items, infos)]
        plain_wall, plain_ms = [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ctx.decode_device_window((frames_ptr, total), citems, dev_out, dt, B, (H * W, W, 1), roi, N.DENORM_PCM16)
            t1 = time.perf_counter()
            if s >= args.warmup:
                plain_wall.append((t1 - t0) * 1e3)
                plain_ms.append(ctx.decode_timing()[3])
        rows = 256  # the rows checked against calc_arrays: the first and the last of the raster
        top, bottom = np.empty((B, rows, W), dt), np.empty((B, rows, W), dt)
        for b in range(B):
            ctx.d2h(top[b], dev_out + (b * H * W) * dt.itemsize)
            ctx.d2h(bottom[b], dev_out + (b * H * W + (H - rows) * W) * dt.itemsize)
        nodata = float(top[0, 0, 0]) if corner else args.nodata
        med = statistics.median
        # the streaming kernel of this session: k_stats without a histogram reads every band once
        ks = []
        for s in range(args.warmup + args.steps):
            ctx.decode_device_stats((frames_ptr, total), citems, dt, B, roi, N.DENORM_PCM16, 0, None)
            if s >= args.warmup:
                ks.append(ctx.stats_timing())
        once = B * H * W * dt.itemsize
        res = {
            "workload": f"calc C4-like {W}x{H}x{B} uint16 (pcm16), tile {TILE}, level {LEVEL}, {len(wins)} tiles, "
                        "whole raster",
            "tiles": len(wins), "frames": nfr, "steps": args.steps, "warmup": args.warmup, "nodata": nodata,
            "checked_rows_equal_calc_arrays": bool(args.calc), "checked_windows_equal_focal_arrays": bool(args.focal),
            "plain_ms": round(med(plain_ms), 3), "plain_wall_ms": round(med(plain_wall), 3),
            "k_stats_ms": round(med(ks), 4), "k_stats_TBps": round(once / (med(ks) * 1e-3) / 1e12, 3), "legs": [],
        }
        for spec in args.calc or []:
            text, _, odt = spec.rpartition(":") if ":" in spec else (spec, "", args.dtype)
            exprs = [e.strip() for e in text.split(";") if e.strip()]
            odt = np.dtype(odt)
            prog = compile_exprs(exprs, B)
            fill = default_fill(odt)
            dev_res = ctx.alloc(prog.nout * H * W * odt.itemsize)
            wall, inner, kc = [], [], []
            for s in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                _, left, _ = ctx.decode_device_calc((frames_ptr, total), citems, dt, B, roi, prog, odt, dst=dev_res,
                                                    denorm=N.DENORM_PCM16, nodata=nodata, fill=fill)
                t1 = time.perf_counter()
                if s >= args.warmup:
                    wall.append((t1 - t0) * 1e3)
                    inner.append(ctx.decode_timing()[3])
                    kc.append(ctx.calc_timing())
            for part, r0 in ((top, 0), (bottom, H - rows)):
                want, _ = calc_arrays(part, prog, odt, nodata, fill)
                got = np.empty((prog.nout, rows, W), odt)
                for k in range(prog.nout):
                    ctx.d2h(got[k], dev_res + (k * H * W + r0 * W) * odt.itemsize)
                if got.tobytes() != want.tobytes():
                    raise SystemExit(f"calc {exprs}: rows {r0} ... {r0 + rows} differ from calc_arrays")
            ctx.free(dev_res)
            rd, wr = len(prog.bands_read()) * H * W * dt.itemsize, prog.nout * H * W * odt.itemsize
            res["legs"].append({
                "exprs": exprs, "dtype": str(odt), "words": int(prog.code.size), "left_out": int(left[0]),
                "calc_wall_ms": round(med(wall), 3), "inner_read_ms": round(med(inner), 3),
                "k_calc_ms": round(med(kc), 4), "bytes_read": rd, "bytes_written": wr,
                "k_calc_TBps": round((rd + wr) / (med(kc) * 1e-3) / 1e12, 3),
                "wall_over_plain": round(med(wall) / med(plain_wall), 3),
                "all_ms": {"k_calc": [round(v, 4) for v in kc], "calc_wall": [round(v, 3) for v in wall]}})
        for text in args.focal or []:
            from flac_raster.focal import focal_arrays

            spec = focal_spec_of(text, nodata)
            odt = np.dtype(args.dtype)
            dev_res = ctx.alloc(B * H * W * odt.itemsize)
            wall, inner, kf = [], [], []
            for s in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                _, left, _ = ctx.decode_device_focal((frames_ptr, total), citems, dt, B, roi, spec, roi, odt, dst=dev_res,
                                                     denorm=N.DENORM_PCM16)
                t1 = time.perf_counter()
                if s >= args.warmup:
                    wall.append((t1 - t0) * 1e3)
                    inner.append(ctx.decode_timing()[3])
                    kf.append(ctx.focal_timing())
            # the top left and the bottom right corner of the result against the rule over the rows read back: the
            # windows stay the radius away from the rows and columns that were not
            ry, rx, cw = spec.kh // 2, spec.kw // 2, 1024
            for part, r0, c0, win in ((top[:, :, :cw + rx], 0, 0, (0, 0, rows - ry, cw)),
                                      (bottom[:, :, W - cw - rx:], H - rows + ry, W - cw, (ry, rx, rows - ry, cw))):
                want, _ = focal_arrays(part, spec, odt, win)
                got = np.empty((B, rows - ry, cw), odt)
                for k in range(B):
                    for r in range(rows - ry):
                        ctx.d2h(got[k, r], dev_res + ((k * H + r0 + r) * W + c0) * odt.itemsize)
                if got.tobytes() != want.tobytes():
                    raise SystemExit(f"focal {text}: the window at ({r0}, {c0}) differs from focal_arrays")
            ctx.free(dev_res)
            rd, wr = B * H * W * dt.itemsize, B * H * W * odt.itemsize
            res["legs"].append({
                "focal": text, "window": [spec.kh, spec.kw], "dtype": str(odt), "left_out": [int(v) for v in left],
                "focal_wall_ms": round(med(wall), 3), "inner_read_ms": round(med(inner), 3),
                "k_focal_ms": round(med(kf), 4), "bytes_read": rd, "bytes_written": wr,
                "k_focal_TBps": round((rd + wr) / (med(kf) * 1e-3) / 1e12, 3),
                "wall_over_plain": round(med(wall) / med(plain_wall), 3),
                "all_ms": {"k_focal": [round(v, 4) for v in kf], "focal_wall": [round(v, 3) for v in wall]}})
        for text in args.warp or []:
            from flac_raster import warp as WP

            m, what = warp_map_of(text)
            dev_res = ctx.alloc(B * H * W * dt.itemsize)
            for mode in args.warp_resampling.split(","):
                wall, inner, kw = [], [], []
                for s in range(args.warmup + args.steps):
                    t0 = time.perf_counter()
                    _, filled = ctx.decode_device_warped((frames_ptr, total), citems, dev_res, dt, B, (H * W, W, 1), (H, W), (H, W),
                                                         m, mode, denorm=N.DENORM_PCM16, nodata=nodata)
                    t1 = time.perf_counter()
                    if s >= args.warmup:
                        wall.append((t1 - t0) * 1e3)
                        inner.append(ctx.decode_timing()[3])
                        kw.append(ctx.warp_timing())
                staged, gathered = ctx.warp_paths()
                # two rectangles of the result against the rule over the source pixels they touch, read back from the
                # plain read of this run
                for ow_ in ((0, 0, 64, 512), (H // 2 - 32, W // 2 - 256, 64, 512), (H - 64, W - 512, 64, 512)):
                    x, y = WP.map_coords(m, (H, W), ow_)
                    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                    got = np.empty((B, ow_[2], ow_[3]), dt)
                    for k in range(B):
                        for r in range(ow_[2]):
                            ctx.d2h(got[k, r], dev_res + ((k * H + ow_[0] + r) * W + ow_[1]) * dt.itemsize)
                    if not ok.any():
                        if (got != (0 if nodata is None else nodata)).any():
                            raise SystemExit(f"warp {text} {mode}: a rectangle outside the source is not all fill")
                        continue
                    r0, r1 = max(int(np.floor(y[ok].min())) - 3, 0), min(int(np.floor(y[ok].max())) + 3, H - 1)
                    c0, c1 = max(int(np.floor(x[ok].min())) - 3, 0), min(int(np.floor(x[ok].max())) + 3, W - 1)
                    part = np.empty((B, r1 - r0 + 1, c1 - c0 + 1), dt)
                    for k in range(B):
                        for r in range(part.shape[1]):
                            ctx.d2h(part[k, r], dev_out + ((k * H + r0 + r) * W + c0) * dt.itemsize)
                    want, _ = WP.warp_arrays(part, (H, W), m, mode, nodata=nodata, origin=(r0, c0), raster_shape=(H, W),
                                             out_window=ow_)
                    if got.tobytes() != want.tobytes():
                        raise SystemExit(f"warp {text} {mode}: the rectangle at {ow_[:2]} differs from warp_arrays")
                rd = wr = B * H * W * dt.itemsize
                res["legs"].append({
                    "warp": text, "map": what, "resampling": mode, "nodata": nodata, "filled": [int(v) for v in filled],
                    "source_window": WP.source_window(m, (H, W), (H, W)), "staged": staged, "gathered": gathered,
                    "warp_wall_ms": round(med(wall), 3), "inner_read_ms": round(med(inner), 3),
                    "k_warp_ms": round(med(kw), 4), "bytes_read": rd, "bytes_written": wr,
                    "k_warp_TBps": round((rd + wr) / (med(kw) * 1e-3) / 1e12, 3),
                    "wall_over_plain": round(med(wall) / med(plain_wall), 3),
                    "all_ms": {"k_warp": [round(v, 4) for v in kw], "warp_wall": [round(v, 3) for v in wall]}})
            ctx.free(dev_res)
        copies = [leg["k_calc_ms"] for leg in res["legs"] if leg.get("exprs") == ["b1"]]
        for leg in res["legs"]:
            if "warp" in leg and copies:  # against k_calc's one-band copy of this run, band for band
                leg["over_calc_copy_per_band"] = round(leg["k_warp_ms"] / B / copies[0], 3)
            if "focal" in leg and copies:  # against k_calc's one-band copy of this run, band for band
                leg["over_calc_copy_per_band"] = round(leg["k_focal_ms"] / B / copies[0], 3)
        res["all_ms"] = {"plain": [round(v, 3) for v in plain_ms], "plain_wall": [round(v, 3) for v in plain_wall],
                         "k_stats": [round(v, 4) for v in ks]}
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    _, frames = plan.download()
    streams = streams_from(infos, frames)

    if args.resample:
        oh, ow = (int(v) for v in args.resample.split(","))
        mode = args.resampling
        roi = tuple(int(v) for v in args.region.split(",")) if args.region else (0, 0, H, W)
        r0, c0, h, w = roi
        dev_small = ctx.alloc(B * oh * ow * 2)
        rs_wall, rs_kern, rs_k = [], [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ctx.decode_device_resampled((frames_ptr, total), items, dev_small, np.int16, B, (oh * ow, ow, 1), roi,
                                        (oh, ow), mode, **nd)
            t1 = time.perf_counter()
            if s >= args.warmup:
                rs_wall.append((t1 - t0) * 1e3)
                rs_kern.append(ctx.decode_timing())
                rs_k.append(ctx.resample_masked_timing() if nd else ctx.resample_timing())
        got = np.empty((B, oh, ow), np.int16)
        ctx.d2h(got, dev_small)
        ctx.free(dev_small)
        full = np.empty((B, H, W), np.int16)
        ctx.d2h(full, dev_out)
        if not np.array_equal(got[0], resample(full[0, r0:r0 + h, c0:c0 + w], (oh, ow), mode, **nd)):
            raise SystemExit("the resampled decode differs from resample.resample of the full decode")
        nd_share = float((full[0, r0:r0 + h, c0:c0 + w] == args.nodata).mean()) if nd else None
        del full
        data = assemble_streaming(wins, streams, (B, H, W), dt, Affine(10.0, 0.0, 0.0, 0.0, -10.0, 0.0), "EPSG:32633",
                                  TILE)
        small_ms, full_ms = [], []
        n_e2e = min(1, args.warmup) + min(3, args.steps)
        # (the container reads give the scene's uint16, the decode above its int16 samples)
        e2e_nd = {}
        if nd:
            at00 = read_window(data, window=(0, 0, 1, 1), device=0)[0]
            e2e_nd = {"nodata": float(at00[0, 0, 0]) if corner else min(max(args.nodata + 32768.0, 0.0), 65535.0)}
        for s in range(n_e2e):
            t0 = time.perf_counter()
            if args.region:
                small = read_window(data, window=roi, device=0, out_shape=(oh, ow), resampling=mode, **e2e_nd)[0]
            else:
                small = read_overview(data, out_shape=(oh, ow), resampling=mode, device=0, **e2e_nd)[0]
            t1 = time.perf_counter()
            big = streaming_to_raster(data, device=0)[0] if not args.region else read_window(data, window=roi, device=0)[0]
            t2 = time.perf_counter()
            if s == 0 and not np.array_equal(small[0], resample(big[0], (oh, ow), mode, **e2e_nd)):
                raise SystemExit("the resampled read differs from resample.resample of the plain read")
            del big
            if s >= min(1, args.warmup):
                small_ms.append((t1 - t0) * 1e3)
                full_ms.append((t2 - t1) * 1e3)
        med = statistics.median
        kr = med(rs_k)
        taps = {"nearest": 1, "average": 0, "bilinear": 4, "cubic": 16}[mode]
        moved = (B * h * w * 2 if mode == "average" else min(B * h * w, taps * B * oh * ow) * 2) + B * oh * ow * 2
        names = ("k_dec_parse_ms", "k_dec_restore_ms", "k_dec_scatter_ms")
        res = {
            "workload": f"resample {h}x{w} at ({r0}, {c0}) -> {oh}x{ow} ({mode}) of C4-like {W}x{H}x{B} uint16, tile "
                        f"{TILE}, level {LEVEL}, {len(wins)} tiles",
            "region": list(roi), "output": [B, oh, ow], "resampling": mode, "tiles": len(wins), "frames": nfr,
            "steps": args.steps, "warmup": args.warmup, "band0_equals_numpy_rule": True,
            "nodata": args.nodata, "nodata_share_band0": nd_share,
            "device_ms": round(med(dev_ms), 3), "device_wall_ms": round(med(dev_wall), 3),
            "kernels_full": {n: round(med([q[i] for q in kern]), 3) for i, n in enumerate(names)},
            "resampled_wall_ms": round(med(rs_wall), 3),
            "resampled_events_ms": round(med([q[3] for q in rs_kern]) + kr, 3),
            "kernels_resampled": dict({n: round(med([q[i] for q in rs_kern]), 3) for i, n in enumerate(names)},
                                      k_resample_ms=round(kr, 4)),
            "k_resample_bytes": moved, "k_resample_TBps": round(moved / (kr * 1e-3) / 1e12, 3),
            "e2e_resampled_ms": round(med(small_ms), 2), "e2e_full_ms": round(med(full_ms), 2),
            "e2e_full_over_resampled": round(med(full_ms) / med(small_ms), 2),
            "all_ms": {"k_resample": [round(v, 4) for v in rs_k], "resampled_wall": [round(v, 2) for v in rs_wall],
                       "device": [round(v, 3) for v in dev_ms], "e2e_resampled": [round(v, 2) for v in small_ms],
                       "e2e_full": [round(v, 2) for v in full_ms]},
        }
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    if args.decimate:
        k, mode = args.decimate, args.resampling
        oh, ow = decimated_shape(H, W, k)
        roi = (0, 0, H, W)
        dev_small = ctx.alloc(B * oh * ow * 2)
        dec_wall, dec_kern, dec_k = [], [], []
        for s in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            ctx.decode_device_decimated((frames_ptr, total), items, dev_small, np.int16, B, (oh * ow, ow, 1), roi, k,
                                        mode, **nd)
            t1 = time.perf_counter()
            if s >= args.warmup:
                dec_wall.append((t1 - t0) * 1e3)
                dec_kern.append(ctx.decode_timing())
                dec_k.append(ctx.resample_masked_timing() if nd else ctx.decimate_timing())
        # one more call with the free device memory sampled beside it: the peak of the call
        hip = C.CDLL("libamdhip64.so")
        free, tot = C.c_size_t(), C.c_size_t()
        hip.hipMemGetInfo(C.byref(free), C.byref(tot))
        base, low, stop = free.value, [free.value], threading.Event()

        def sample():
            f, t = C.c_size_t(), C.c_size_t()
            while not stop.is_set():
                if hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0:
                    low[0] = min(low[0], f.value)
                time.sleep(0.0005)

        th = threading.Thread(target=sample, daemon=True)
        th.start()
        ctx.decode_device_decimated((frames_ptr, total), items, dev_small, np.int16, B, (oh * ow, ow, 1), roi, k, mode,
                                    **nd)
        stop.set()
        th.join()
        # the result against the numpy rule over the full decode: the top 2048 rows and the ragged bottom blocks
        got = np.empty((B, oh, ow), np.int16)
        ctx.d2h(got, dev_small)
        full = np.empty((B, H, W), np.int16)
        ctx.d2h(full, dev_out)
        top = 2048 // k
        tail = oh - 4
        if not (np.array_equal(got[:, :top], decimate(full[:, :2048], k, mode, **nd))
                and np.array_equal(got[:, tail:], decimate(full[:, tail * k:], k, mode, **nd))):
            raise SystemExit("the decimated decode differs from resample.decimate of the full decode")
        nd_share = float((full[0] == args.nodata).mean()) if nd else None
        del full
        ctx.free(dev_small)
        # container bytes -> host raster, both ways, alternating
        data = assemble_streaming(wins, streams, (B, H, W), dt, Affine(10.0, 0.0, 0.0, 0.0, -10.0, 0.0), "EPSG:32633",
                                  TILE)
        ov_ms, full_ms = [], []
        n_e2e = min(1, args.warmup) + min(3, args.steps)
        # (the container reads give the scene's uint16, the decode above its int16 samples)
        e2e_nd = {}
        if nd:
            at00 = read_window(data, window=(0, 0, 1, 1), device=0)[0]
            e2e_nd = {"nodata": float(at00[0, 0, 0]) if corner else min(max(args.nodata + 32768.0, 0.0), 65535.0)}
        for s in range(n_e2e):
            t0 = time.perf_counter()
            small, _ = read_overview(data, k, mode, device=0, **e2e_nd)
            t1 = time.perf_counter()
            big, _ = streaming_to_raster(data, device=0)
            t2 = time.perf_counter()
            if s == 0 and not np.array_equal(small[:, :top], decimate(big[:, :2048], k, mode, **e2e_nd)):
                raise SystemExit("read_overview differs from resample.decimate of streaming_to_raster")
            del big
            if s >= min(1, args.warmup):
                ov_ms.append((t1 - t0) * 1e3)
                full_ms.append((t2 - t1) * 1e3)
        med = statistics.median
        kd = med(dec_k)
        # average reads the region once and writes the output; nearest reads one element per output
        moved = (B * H * W * 2 if mode == "average" else B * oh * ow * 2) + B * oh * ow * 2
        names = ("k_dec_parse_ms", "k_dec_restore_ms", "k_dec_scatter_ms")
        res = {
            "workload": f"decimate {k} ({mode}) of C4-like {W}x{H}x{B} uint16, tile {TILE}, level {LEVEL}, "
                        f"{len(wins)} tiles, whole raster",
            "factor": k, "resampling": mode, "output": [B, oh, ow], "tiles": len(wins), "frames": nfr,
            "steps": args.steps, "warmup": args.warmup, "equals_numpy_rule_on_checked_rows": True,
            "nodata": args.nodata, "nodata_share_band0": nd_share,
            "device_ms": round(med(dev_ms), 3), "device_wall_ms": round(med(dev_wall), 3),
            "kernels_full": {n: round(med([q[i] for q in kern]), 3) for i, n in enumerate(names)},
            "decimated_wall_ms": round(med(dec_wall), 3),
            "decimated_events_ms": round(med([q[3] for q in dec_kern]) + kd, 3),
            "kernels_decimated": dict({n: round(med([q[i] for q in dec_kern]), 3) for i, n in enumerate(names)},
                                      k_decimate_ms=round(kd, 4)),
            "k_decimate_bytes": moved, "k_decimate_TBps": round(moved / (kd * 1e-3) / 1e12, 3),
            "peak_device_bytes_of_call": base - low[0],
            "region_buffer_bytes": B * H * (-(-W // 8) * 8) * 2, "output_bytes": B * oh * ow * 2,
            "e2e_overview_ms": round(med(ov_ms), 2), "e2e_full_ms": round(med(full_ms), 2),
            "e2e_full_over_overview": round(med(full_ms) / med(ov_ms), 2),
            "all_ms": {"k_decimate": [round(v, 4) for v in dec_k], "decimated_wall": [round(v, 2) for v in dec_wall],
                       "device": [round(v, 3) for v in dev_ms], "e2e_overview": [round(v, 2) for v in ov_ms],
                       "e2e_full": [round(v, 2) for v in full_ms]},
        }
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    def verify() -> int:
        """The device raster against the host decoder on the first, middle and last tile; then cleared."""
        got = np.empty((B, H, W), np.int16)
        ctx.d2h(got, dev_out)
        picks = sorted({0, len(wins) // 2, len(wins) - 1})
        for i in picks:
            r, c, h, w = wins[i]
            x, _ = N.decode(streams[i].data)
            if not np.array_equal(got[:, r:r + h, c:c + w], x.reshape(h, w, B).transpose(2, 0, 1)):
                raise SystemExit(f"device decode of tile {i} differs from the host decoder")
        got[:] = 0
        ctx.h2d(dev_out, got)
        return len(picks)

    verified = verify()

    # ---- device, search path: complete streams in page-locked host memory
    blob_len = sum(len(ts) for ts in streams)
    blob = N.pinned_empty(blob_len, np.uint8)
    sitems, p = [], 0
    for ts, w in zip(streams, wins):
        d = ts.data
        blob[p:p + len(d)] = np.frombuffer(d, np.uint8)
        sitems.append({"offset": p, "bytes": len(d), "window": w})
        p += len(d)
    search_ms, search_ev = [], []
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        ctx.decode_device(blob, sitems, dev_out, np.int16, B, (H * W, W, 1))
        t1 = time.perf_counter()
        if k >= args.warmup:
            search_ms.append((t1 - t0) * 1e3)
            search_ev.append(ctx.decode_timing()[3])

    if args.window:
        if args.window == "center":
            win = ((H - 2048) // 2, (W - 2048) // 2, 2048, 2048)
        else:
            win = tuple(int(v) for v in args.window.split(","))
        r, c, h, w = win
        full = np.empty((B, H, W), np.int16)
        ctx.d2h(full, dev_out)  # the full decode of the search leg
        want = full[:, r:r + h, c:c + w].copy()
        del full
        dev_win = ctx.alloc(B * h * w * 2)
        got = np.empty((B, h, w), np.int16)
        legs = {}
        for name, data, its in (("window", (frames_ptr, total), items), ("window_search", blob, sitems)):
            wall, evt, ks = [], [], []
            for k in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                out = ctx.decode_device_window(data, its, dev_win, np.int16, B, (h * w, w, 1), win)
                t1 = time.perf_counter()
                if k >= args.warmup:
                    ms = ctx.decode_timing()
                    wall.append((t1 - t0) * 1e3)
                    evt.append(ms[3])
                    ks.append(ms[:3])
            ctx.d2h(got, dev_win)
            if not np.array_equal(got, want):
                raise SystemExit(f"{name}: the window differs from the crop of the full decode")
            ctx.h2d(dev_win, np.zeros_like(got))
            legs[name] = (wall, evt, ks, sum(o.nframes for o in out), sum(1 for o in out if o.nframes))
        ctx.free(dev_win)
        med = statistics.median
        kfull = [med([k[i] for k in kern]) for i in range(3)]
        wwall, wevt, wks, wfr, wtiles = legs["window"]
        swall, sevt, sks, _, _ = legs["window_search"]
        names = ("k_dec_parse_ms", "k_dec_restore_ms", "k_dec_scatter_ms")
        res = {
            "workload": f"window {h}x{w} at ({r}, {c}) of C4-like {W}x{H}x{B} uint16, tile {TILE}, level {LEVEL}, "
                        f"{len(wins)} tiles",
            "window": list(win), "tiles": len(wins), "frames": nfr, "window_tiles": wtiles, "window_frames": wfr,
            "steps": args.steps, "warmup": args.warmup, "window_equals_crop_of_full_decode": True,
            "device_ms": round(med(dev_ms), 3), "device_wall_ms": round(med(dev_wall), 3),
            "window_ms": round(med(wevt), 3), "window_wall_ms": round(med(wwall), 3),
            "device_search_ms": round(med(search_ms), 3), "window_search_ms": round(med(swall), 3),
            "window_search_event_ms": round(med(sevt), 3),
            "full_over_window": {"events": round(med(dev_ms) / med(wevt), 2),
                                 "wall": round(med(dev_wall) / med(wwall), 2),
                                 "search_wall": round(med(search_ms) / med(swall), 2)},
            "area_ratio": round(sum(x[2] * x[3] for x in wins) / (h * w), 2),
            "kernels_full": {n: round(v, 3) for n, v in zip(names, kfull)},
            "kernels_window": {n: round(med([k[i] for k in wks]), 3) for i, n in enumerate(names)},
            "kernels_window_search": {n: round(med([k[i] for k in sks]), 3) for i, n in enumerate(names)},
            "all_ms": {"window": [round(v, 3) for v in wevt], "window_wall": [round(v, 3) for v in wwall],
                       "window_search": [round(v, 2) for v in swall]},
        }
        print(json.dumps(res), flush=True)
        plan.close()
        ctx.free(dev_out)
        ctx.free(dev_raster)
        return

    verified += verify()

    # ---- host decoder, tile by tile
    tile_streams = [ts.data for ts in streams]
    host_decode_all(tile_streams[:1])
    host_ms = []
    for _ in range(max(1, args.host_steps)):
        t0 = time.perf_counter()
        n = host_decode_all(tile_streams)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        assert n == samples

    # ---- host container bytes -> host raster
    e2e_ms = []
    if not args.no_e2e:
        data = assemble_streaming(wins, streams, (B, H, W), dt, Affine(10.0, 0.0, 0.0, 0.0, -10.0, 0.0), "EPSG:32633",
                                  TILE)
        for k in range(min(1, args.warmup) + min(2, args.steps)):
            t0 = time.perf_counter()
            streaming_to_raster(data, device=0)
            if k >= min(1, args.warmup):
                e2e_ms.append((time.perf_counter() - t0) * 1e3)

    med = statistics.median
    d_ms, s_ms, h_ms = med(dev_ms), med(search_ms), med(host_ms)
    kmed = [med([k[i] for k in kern]) for i in range(3)]
    res = {
        "workload": f"decode C4-like {W}x{H}x{B} uint16, tile {TILE}, level {LEVEL}, {len(wins)} tiles",
        "tiles": len(wins), "frames": nfr, "samples": samples, "frame_bytes": total,
        "steps": args.steps, "warmup": args.warmup, "tiles_verified_against_host_decoder": verified,
        "host_decode_ms": round(h_ms, 3), "device_ms": round(d_ms, 3), "device_wall_ms": round(med(dev_wall), 3),
        "device_search_ms": round(s_ms, 3), "device_search_event_ms": round(med(search_ev), 3),
        "e2e_ms": round(med(e2e_ms), 3) if e2e_ms else None,
        "samples_per_s": {"host": round(samples / h_ms * 1e3), "device": round(samples / d_ms * 1e3),
                          "device_search": round(samples / s_ms * 1e3),
                          "e2e": round(samples / med(e2e_ms) * 1e3) if e2e_ms else None},
        "kernels": {"k_dec_parse_ms": round(kmed[0], 3), "k_dec_restore_ms": round(kmed[1], 3),
                    "k_dec_scatter_ms": round(kmed[2], 3),
                    "share": [round(v / d_ms, 3) for v in kmed]},
        "host_over_device": round(h_ms / d_ms, 2), "host_over_device_search": round(h_ms / s_ms, 2),
        "all_ms": {"host": [round(v, 2) for v in host_ms], "device": [round(v, 3) for v in dev_ms],
                   "device_search": [round(v, 2) for v in search_ms], "e2e": [round(v, 2) for v in e2e_ms]},
    }
    print(json.dumps(res), flush=True)
    plan.close()
    ctx.free(dev_out)
    ctx.free(dev_raster)


if __name__ == "__main__":
    main()
