"""ctypes binding of ``libflac_raster_amd.so`` (C ABI: ``include/flac_raster_amd.h``).

This is the only compute path of the package: there is no CPU fallback.  If the library is
missing, or no GPU is visible, every encode call raises :class:`NativeUnavailable` loudly.
The library is built in-tree by ``flac-raster_amd/csrc/Makefile`` (``__graft_entry__.build()``).
"""

from __future__ import annotations

import ctypes as C
import os
import threading
import time
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np

# FRA_LIB_PATH: load another build of the library (same-box A/B experiments, tools/gpu_ab.sh)
_LIB_PATH = Path(os.environ.get("FRA_LIB_PATH") or Path(__file__).resolve().parent / "_lib" / "libflac_raster_amd.so")
_lib = None
_lock = threading.RLock()  # re-entrant: __del__ (cyclic GC) may run while this thread holds it

DTYPE_CODES = {
    np.dtype(np.uint8): 0, np.dtype(np.int8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3,
    np.dtype(np.uint32): 4, np.dtype(np.int32): 5, np.dtype(np.float32): 6, np.dtype(np.float64): 7,
}


class NativeUnavailable(RuntimeError):
    """The HIP extension is not built or no MI355X (gfx950) device is visible."""


class NativeError(RuntimeError):
    pass


class OutputTooSmall(NativeError):
    def __init__(self, needed: int):
        super().__init__(f"output buffer too small: {needed} bytes needed")
        self.needed = needed


class RegionsNoSpace(NativeError):
    """A band of a regions call has more kept components than the labels dtype or the table holds (``FRA_E_SPACE``).
    ``counts``: the complete ``(B, 4)`` counts, ``counts[:, 2]`` the N of every band; nothing has been written."""

    def __init__(self, message: str, counts):
        super().__init__(message)
        self.code = E_SPACE
        self.counts = counts


class VerifyMismatch(NativeError):
    """Verify found decoded samples that differ from the normalised input (``Plan.verify``, ``verify=True``).

    ``tile``: index of the first bad window of the call; ``pixel``: ``(row, col, band)`` of its first mismatch in
    raster coordinates; ``expected`` / ``got``: the normalised input sample and the decoded one there;
    ``mismatches``: differing samples of that tile; ``bad_tiles``: tiles with mismatches."""

    def __init__(self, tile: int, pixel: Tuple[int, int, int], expected: int, got: int, mismatches: int,
                 bad_tiles: int = 1):
        super().__init__(f"verify: tile {tile} differs from its input at pixel (row {pixel[0]}, col {pixel[1]}, "
                         f"band {pixel[2]}): expected sample {expected}, decoded {got}; {mismatches} samples differ "
                         f"in this tile, {bad_tiles} tile(s) differ")
        self.tile, self.pixel, self.expected, self.got = tile, tuple(pixel), expected, got
        self.mismatches, self.bad_tiles = mismatches, bad_tiles


class Window(C.Structure):
    _fields_ = [("row_off", C.c_int32), ("col_off", C.c_int32), ("height", C.c_int32), ("width", C.c_int32)]


class Job(C.Structure):
    _fields_ = [
        ("raster", C.c_void_p), ("raster_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("band_stride", C.c_int64), ("row_stride", C.c_int64), ("col_stride", C.c_int64),
        ("windows", C.POINTER(Window)), ("nwindows", C.c_int32), ("level", C.c_int32), ("blocksize", C.c_int32),
        ("norm", C.c_int32), ("sample_rate", C.c_int32), ("first_frame", C.c_int32),
    ]


class StreamInfo(C.Structure):
    _fields_ = [
        ("offset", C.c_uint64), ("frame_bytes", C.c_uint64), ("data_min", C.c_double), ("data_max", C.c_double),
        ("sample_rate", C.c_int32), ("bps", C.c_int32), ("channels", C.c_int32), ("nframes", C.c_int32),
    ]


class Decoded(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_int32), ("channels", C.c_int32), ("bps", C.c_int32), ("blocksize", C.c_int32),
        ("nframes", C.c_int64), ("nsamples", C.c_uint64), ("nstreams", C.c_int32), ("audio_offset", C.c_uint64),
    ]


class VerifyReport(C.Structure):
    _fields_ = [
        ("mismatches", C.c_uint64), ("first_sample", C.c_int64), ("first_channel", C.c_int32),
        ("expected", C.c_int32), ("got", C.c_int32), ("nframes", C.c_int32),
    ]


class DecimateJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("src_band_stride", C.c_int64), ("src_row_stride", C.c_int64),
        ("src_col_stride", C.c_int64), ("factor", C.c_int32), ("resampling", C.c_int32), ("dst", C.c_void_p),
        ("dst_on_device", C.c_int32), ("dst_band_stride", C.c_int64), ("dst_row_stride", C.c_int64),
        ("dst_col_stride", C.c_int64),
    ]


class ResampleJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("src_band_stride", C.c_int64), ("src_row_stride", C.c_int64),
        ("src_col_stride", C.c_int64), ("out_height", C.c_int32), ("out_width", C.c_int32), ("resampling", C.c_int32),
        ("dst", C.c_void_p), ("dst_on_device", C.c_int32), ("dst_band_stride", C.c_int64),
        ("dst_row_stride", C.c_int64), ("dst_col_stride", C.c_int64),
    ]


class CompareBand(C.Structure):
    """One band's report of ``fra_compare`` / ``fra_decode_device_compare`` (128 bytes; the rule: ``compare.py``)."""

    _fields_ = [
        ("count", C.c_uint64), ("differing", C.c_uint64), ("unordered", C.c_uint64), ("first_row", C.c_int64),
        ("first_col", C.c_int64), ("sum_abs", C.c_uint64), ("sum_sq_lo", C.c_uint64), ("sum_sq_hi", C.c_uint64),
        ("max_abs", C.c_double), ("fsum_abs", C.c_double), ("fsum_sq", C.c_double), ("a_min", C.c_double),
        ("a_max", C.c_double), ("b_min", C.c_double), ("b_max", C.c_double), ("reserved", C.c_uint64),
    ]


class CompareJob(C.Structure):
    _fields_ = [
        ("a", C.c_void_p), ("a_on_device", C.c_int32), ("a_band_stride", C.c_int64), ("a_row_stride", C.c_int64),
        ("a_col_stride", C.c_int64), ("b", C.c_void_p), ("b_on_device", C.c_int32), ("b_band_stride", C.c_int64),
        ("b_row_stride", C.c_int64), ("b_col_stride", C.c_int64), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32),
    ]


class StatsOpts(C.Structure):
    _fields_ = [("bins", C.c_int32), ("flags", C.c_int32), ("hist_lo", C.c_double), ("hist_hi", C.c_double),
                ("nodata", C.c_double)]


class StatsJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("band_stride", C.c_int64), ("row_stride", C.c_int64),
        ("col_stride", C.c_int64), ("opts", StatsOpts),
    ]


class StatsBand(C.Structure):
    """One band's report of ``fra_stats`` / ``fra_decode_device_stats`` (160 bytes; the rule: ``stats.py``)."""

    _fields_ = [
        ("count", C.c_uint64), ("valid", C.c_uint64), ("nan", C.c_uint64), ("nodata", C.c_uint64),
        ("below", C.c_uint64), ("above", C.c_uint64), ("sum_lo", C.c_uint64), ("sum_hi", C.c_int64),
        ("sq_lo", C.c_uint64), ("sq_hi", C.c_uint64), ("min", C.c_double), ("max", C.c_double),
        ("fin_min", C.c_double), ("fin_max", C.c_double), ("fsum", C.c_double), ("mean", C.c_double),
        ("fm2", C.c_double), ("hist_lo", C.c_double), ("hist_hi", C.c_double), ("hist_scale", C.c_double),
    ]


class CalcProgram(C.Structure):
    """``fra_calc_program`` (544 bytes; the rule: ``calc.py``)."""

    _fields_ = [("ncode", C.c_int32), ("nconst", C.c_int32), ("nout", C.c_int32), ("flags", C.c_int32),
                ("nodata", C.c_double), ("fill", C.c_double), ("code", C.c_uint16 * 128), ("consts", C.c_double * 32)]


class CalcDst(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("dst_on_device", C.c_int32), ("dtype", C.c_int32), ("band_stride", C.c_int64),
                ("row_stride", C.c_int64), ("col_stride", C.c_int64)]


class CalcJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("band_stride", C.c_int64), ("row_stride", C.c_int64),
        ("col_stride", C.c_int64), ("program", CalcProgram), ("out", CalcDst),
    ]


class FocalSpec(C.Structure):
    """``fra_focal_spec`` (1904 bytes; the rule: ``focal.py``)."""

    _fields_ = [("op", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("edge", C.c_int32), ("flags", C.c_int32),
                ("nodata", C.c_double), ("fill", C.c_double), ("params", C.c_double * 8), ("weights", C.c_double * 225)]


class FocalJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("band_stride", C.c_int64), ("row_stride", C.c_int64),
        ("col_stride", C.c_int64), ("rect", Window), ("spec", FocalSpec), ("out", CalcDst),
    ]


class WarpMap(C.Structure):
    """``fra_warp_map`` (80 bytes; the rule: ``warp.py``)."""

    _fields_ = [("kind", C.c_int32), ("step", C.c_int32), ("gh", C.c_int32), ("gw", C.c_int32),
                ("affine", C.c_double * 6), ("gx", C.POINTER(C.c_double)), ("gy", C.POINTER(C.c_double))]


class WarpJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("src_band_stride", C.c_int64), ("src_row_stride", C.c_int64),
        ("src_col_stride", C.c_int64), ("out_height", C.c_int32), ("out_width", C.c_int32), ("resampling", C.c_int32),
        ("flags", C.c_int32), ("dst", C.c_void_p), ("dst_on_device", C.c_int32), ("dst_band_stride", C.c_int64),
        ("dst_row_stride", C.c_int64), ("dst_col_stride", C.c_int64), ("nodata", C.c_double), ("fill", C.c_double),
        ("map", WarpMap),
    ]


assert C.sizeof(WarpMap) == 80 and C.sizeof(WarpJob) == 208


class ZonalOpts(C.Structure):
    _fields_ = [("flags", C.c_int32), ("nzones", C.c_int32), ("zone_lo", C.c_int64), ("ignore_zone", C.c_int64),
                ("nodata", C.c_double)]


class ZonalJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("band_stride", C.c_int64), ("row_stride", C.c_int64),
        ("col_stride", C.c_int64), ("zones", C.c_void_p), ("zones_on_device", C.c_int32), ("zone_dtype", C.c_int32),
        ("zone_row_stride", C.c_int64), ("zone_col_stride", C.c_int64), ("opts", ZonalOpts),
    ]


class ZonalRec(C.Structure):
    """One (band, zone) record of ``fra_zonal`` / ``fra_decode_device_zonal`` (112 bytes; the rule: ``zonal.py``)."""

    _fields_ = [
        ("count", C.c_uint64), ("valid", C.c_uint64), ("nan", C.c_uint64), ("nodata", C.c_uint64),
        ("sum_lo", C.c_uint64), ("sum_hi", C.c_int64), ("sq_lo", C.c_uint64), ("sq_hi", C.c_uint64),
        ("min", C.c_double), ("max", C.c_double), ("fsum", C.c_double), ("mean", C.c_double), ("fm2", C.c_double),
        ("reserved", C.c_uint64),
    ]


assert C.sizeof(ZonalRec) == 112 and C.sizeof(ZonalOpts) == 32 and C.sizeof(ZonalJob) == 120


class RasterizeJob(C.Structure):
    """``fra_rasterize_job`` (128 bytes; the rule: ``rasterize.py``)."""

    _fields_ = [
        ("xy", C.c_void_p), ("nverts", C.c_int64), ("ring_start", C.c_void_p), ("nrings", C.c_int64),
        ("feature_ring_start", C.c_void_p), ("nfeatures", C.c_int32), ("values", C.c_void_p), ("dtype", C.c_int32),
        ("row_off", C.c_int64), ("col_off", C.c_int64), ("height", C.c_int32), ("width", C.c_int32),
        ("fill", C.c_int64), ("dst", C.c_void_p), ("dst_on_device", C.c_int32), ("row_stride", C.c_int64),
        ("col_stride", C.c_int64),
    ]


assert C.sizeof(RasterizeJob) == 128


class ProximityOpts(C.Structure):
    """``fra_proximity_opts`` (280 bytes; the rule: ``proximity.py``)."""

    _fields_ = [
        ("nvalues", C.c_int32), ("has_max_dist", C.c_int32), ("has_fixed", C.c_int32), ("out_row_off", C.c_int32),
        ("out_col_off", C.c_int32), ("out_height", C.c_int32), ("out_width", C.c_int32), ("reserved", C.c_int32),
        ("values", C.c_double * 16), ("scale", C.c_double), ("max_dist", C.c_double), ("fixed", C.c_double),
        ("fill", C.c_double), ("alloc_fill", C.c_double), ("dist", CalcDst), ("alloc", CalcDst),
    ]


class ProximityJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("band_stride", C.c_int64), ("row_stride", C.c_int64),
        ("col_stride", C.c_int64), ("opts", ProximityOpts),
    ]


assert C.sizeof(ProximityOpts) == 280 and C.sizeof(ProximityJob) == 336


class RegionsOpts(C.Structure):
    """``fra_regions_opts`` (296 bytes; the rule: ``regions.py``)."""

    _fields_ = [
        ("nvalues", C.c_int32), ("invert", C.c_int32), ("by_value", C.c_int32), ("connectivity", C.c_int32),
        ("min_size", C.c_int32), ("table_cap", C.c_int32), ("table_on_device", C.c_int32), ("reserved", C.c_int32),
        ("values", C.c_double * 16), ("sieve_fill", C.c_double), ("table", C.c_void_p),
        ("labels", CalcDst), ("area", CalcDst), ("sieved", CalcDst),
    ]


class RegionsJob(C.Structure):
    _fields_ = [
        ("src", C.c_void_p), ("src_on_device", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32),
        ("height", C.c_int32), ("width", C.c_int32), ("band_stride", C.c_int64), ("row_stride", C.c_int64),
        ("col_stride", C.c_int64), ("opts", RegionsOpts),
    ]


assert C.sizeof(RegionsOpts) == 296 and C.sizeof(RegionsJob) == 352

STATS_AUTO_RANGE, STATS_NODATA = 1, 2
ZONAL_NODATA, ZONAL_IGNORE = 1, 2
CALC_NODATA = 1
WARP_AFFINE, WARP_GRID = 0, 1
WARP_NODATA = 1
DECODE_CONCAT = 1
RESAMPLE_NEAREST, RESAMPLE_AVERAGE = 0, 1
RESAMPLE_BILINEAR, RESAMPLE_CUBIC = 2, 3
E_SPACE = -6
# fra_plan_flags (Plan.flags)
PLAN_DIRECT_WRITE, PLAN_PIPELINED, PLAN_WAVE, PLAN_KEEP17 = 1, 2, 4, 8
PLAN_LOAD_VEC8, PLAN_MINMAX_VEC16, PLAN_MINMAX_VEC8, PLAN_OFF32 = 16, 32, 64, 128
DENORM_NONE, DENORM_INT, DENORM_PCM16 = 0, 1, 2


class DecodeItem(C.Structure):
    _fields_ = [
        ("offset", C.c_uint64), ("bytes", C.c_uint64), ("window", Window), ("data_min", C.c_double),
        ("data_max", C.c_double), ("frame_offsets", C.POINTER(C.c_uint64)), ("nframes", C.c_int32),
        ("channels", C.c_int32), ("bps", C.c_int32), ("blocksize", C.c_int32),
    ]


class DecodeJob(C.Structure):
    _fields_ = [
        ("data", C.c_void_p), ("len", C.c_uint64), ("data_on_device", C.c_int32), ("items", C.POINTER(DecodeItem)),
        ("nitems", C.c_int32), ("flags", C.c_int32), ("dst", C.c_void_p), ("dst_on_device", C.c_int32),
        ("dst_dtype", C.c_int32), ("denorm", C.c_int32), ("channels", C.c_int32), ("band_stride", C.c_int64),
        ("row_stride", C.c_int64), ("col_stride", C.c_int64),
    ]


class TiffChunk(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64), ("row0", C.c_int32), ("col0", C.c_int32),
                ("rows", C.c_int32), ("cols", C.c_int32), ("plane", C.c_int32), ("pad", C.c_int32)]


class TiffLayout(C.Structure):
    _fields_ = [("compression", C.c_int32), ("predictor", C.c_int32), ("bytes_per_sample", C.c_int32),
                ("samples_per_pixel", C.c_int32), ("is_float", C.c_int32), ("big_endian", C.c_int32),
                ("bands", C.c_int32), ("win_row", C.c_int32), ("win_col", C.c_int32), ("win_h", C.c_int32),
                ("win_w", C.c_int32), ("pad", C.c_int32), ("dst_band_stride", C.c_int64),
                ("dst_row_stride", C.c_int64)]

EXPORTS = [
    "fra_last_error", "fra_abi_version", "fra_device_count", "fra_free", "fra_ctx_create", "fra_ctx_destroy",
    "fra_plan_create", "fra_plan_set_raster", "fra_plan_execute", "fra_plan_sync", "fra_plan_result",
    "fra_plan_download", "fra_plan_device_output", "fra_plan_enable_timing", "fra_plan_timing",
    "fra_plan_destroy", "fra_encode", "fra_stream_header", "fra_synth_raster", "fra_device_alloc",
    "fra_device_free", "fra_memcpy_d2h", "fra_memcpy_h2d", "fra_plan_frame_offsets", "fra_normalize",
    "fra_decode", "fra_plan_encode_host", "fra_plan_capacity", "fra_host_alloc", "fra_host_free",
    "fra_host_register", "fra_host_unregister", "fra_tiff_decode", "fra_plan_set_first_frame",
    "fra_plan_flags", "fra_plan_encode_host_progress", "fra_tiff_compress_bound", "fra_tiff_compress",
    "fra_plan_encode_ring", "fra_plan_host_band_rows", "fra_plan_create_ranged", "fra_decode_device",
    "fra_decode_device_timing", "fra_decode_device_window", "fra_plan_verify", "fra_decimate",
    "fra_decode_device_decimated", "fra_decimate_timing", "fra_compare", "fra_decode_device_compare",
    "fra_compare_timing", "fra_stats", "fra_decode_device_stats", "fra_stats_timing", "fra_resample",
    "fra_decode_device_resampled", "fra_resample_timing", "fra_resample_masked", "fra_decimate_masked",
    "fra_decode_device_resampled_masked", "fra_decode_device_decimated_masked", "fra_resample_masked_timing",
    "fra_calc_check", "fra_calc", "fra_decode_device_calc", "fra_calc_timing",
    "fra_focal_check", "fra_focal", "fra_decode_device_focal", "fra_focal_timing",
    "fra_zonal", "fra_decode_device_zonal", "fra_zonal_timing",
    "fra_warp", "fra_decode_device_warped", "fra_warp_source_window", "fra_warp_timing", "fra_warp_paths",
    "fra_rasterize", "fra_rasterize_timing",
    "fra_proximity", "fra_decode_device_proximity", "fra_proximity_timing",
    "fra_regions", "fra_decode_device_regions", "fra_regions_timing",
]


def library_path() -> Path:
    return _LIB_PATH


def load():
    """Load the shared library (no GPU needed just to load it)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not _LIB_PATH.exists():
            raise NativeUnavailable(
                f"{_LIB_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C flac-raster_amd/csrc)")
        L = C.CDLL(str(_LIB_PATH))
        vp, i32, u64 = C.c_void_p, C.c_int32, C.c_uint64
        L.fra_last_error.restype = C.c_char_p
        L.fra_abi_version.restype = C.c_int
        L.fra_device_count.argtypes = [C.POINTER(C.c_int)]
        L.fra_free.argtypes = [vp]
        L.fra_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.fra_ctx_destroy.argtypes = [vp]
        L.fra_plan_create.argtypes = [vp, C.POINTER(Job), C.POINTER(vp)]
        L.fra_plan_set_raster.argtypes = [vp, vp, i32]
        L.fra_plan_execute.argtypes = [vp]
        L.fra_plan_sync.argtypes = [vp]
        L.fra_plan_result.argtypes = [vp, C.POINTER(StreamInfo), C.POINTER(u64)]
        L.fra_plan_download.argtypes = [vp, vp, u64]
        L.fra_plan_device_output.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
        L.fra_plan_enable_timing.argtypes = [vp, i32]
        L.fra_plan_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(i32)]
        L.fra_plan_destroy.argtypes = [vp]
        L.fra_encode.argtypes = [C.c_int, C.POINTER(Job), C.POINTER(vp), C.POINTER(u64), C.POINTER(StreamInfo)]
        L.fra_stream_header.argtypes = [vp, i32, i32, i32, i32]
        L.fra_synth_raster.argtypes = [vp, i32, u64, i32, i32, i32, vp]
        L.fra_device_alloc.argtypes = [vp, u64, C.POINTER(vp)]
        L.fra_device_free.argtypes = [vp, vp]
        L.fra_memcpy_d2h.argtypes = [vp, vp, vp, u64]
        L.fra_memcpy_h2d.argtypes = [vp, vp, vp, u64]
        L.fra_plan_frame_offsets.argtypes = [vp, C.POINTER(u64), u64]
        pd = C.POINTER(C.c_double)
        L.fra_normalize.argtypes = [vp, vp, i32, i32, u64, i32, pd, pd, vp, pd, pd]
        L.fra_decode.argtypes = [vp, u64, i32, C.POINTER(Decoded), C.POINTER(C.POINTER(C.c_int32))]
        L.fra_plan_encode_host.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
        L.fra_plan_capacity.argtypes = [vp, C.POINTER(u64), C.POINTER(i32)]
        L.fra_plan_set_first_frame.argtypes = [vp, i32]
        L.fra_plan_flags.argtypes = [vp, C.POINTER(i32)]
        L.fra_host_alloc.argtypes = [u64, C.POINTER(vp)]
        L.fra_host_free.argtypes = [vp]
        L.fra_host_register.argtypes = [vp, u64]
        L.fra_host_unregister.argtypes = [vp]
        L.fra_tiff_decode.argtypes = [vp, u64, C.POINTER(TiffLayout), C.POINTER(TiffChunk), i32, vp, i32]
        L.fra_plan_encode_host_progress.argtypes = [vp, vp, vp, u64, C.POINTER(u64), vp]
        if hasattr(L, "fra_plan_create_ranged"):  # (r05; older builds load for same-box A/Bs)
            L.fra_plan_create_ranged.argtypes = [vp, C.POINTER(Job), C.POINTER(C.c_int32), C.POINTER(vp)]
        if hasattr(L, "fra_plan_encode_ring"):
            L.fra_plan_encode_ring.argtypes = [vp, vp, C.c_int64, vp, u64, C.POINTER(u64), vp, vp]
            L.fra_plan_host_band_rows.argtypes = [vp, C.POINTER(C.c_int64)]
        L.fra_decode_device.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Decoded)]
        L.fra_decode_device_timing.argtypes = [C.POINTER(C.c_float)]
        L.fra_decode_device_window.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), C.POINTER(Decoded)]
        if hasattr(L, "fra_plan_verify"):  # (older builds load for same-box A/Bs)
            L.fra_plan_verify.argtypes = [vp, C.POINTER(VerifyReport), C.POINTER(i32)]
        if hasattr(L, "fra_decimate"):
            L.fra_decimate.argtypes = [vp, C.POINTER(DecimateJob)]
            L.fra_decode_device_decimated.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), i32, i32,
                                                      C.POINTER(Decoded)]
            L.fra_decimate_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_compare"):
            L.fra_compare.argtypes = [vp, C.POINTER(CompareJob), C.POINTER(CompareBand)]
            L.fra_decode_device_compare.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), vp, i32, C.c_int64,
                                                    C.c_int64, C.c_int64, C.POINTER(CompareBand), C.POINTER(Decoded)]
            L.fra_compare_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_stats"):
            L.fra_stats.argtypes = [vp, C.POINTER(StatsJob), C.POINTER(StatsBand), C.POINTER(u64)]
            L.fra_decode_device_stats.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), C.POINTER(StatsOpts),
                                                  C.POINTER(StatsBand), C.POINTER(u64), C.POINTER(Decoded)]
            L.fra_stats_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_resample"):
            L.fra_resample.argtypes = [vp, C.POINTER(ResampleJob)]
            L.fra_decode_device_resampled.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), i32, i32, i32,
                                                      C.POINTER(Decoded)]
            L.fra_resample_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_resample_masked"):
            L.fra_resample_masked.argtypes = [vp, C.POINTER(ResampleJob), C.c_double, C.POINTER(u64)]
            L.fra_decimate_masked.argtypes = [vp, C.POINTER(DecimateJob), C.c_double, C.POINTER(u64)]
            L.fra_decode_device_resampled_masked.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), i32, i32, i32,
                                                             C.POINTER(Decoded), C.c_double, C.POINTER(u64)]
            L.fra_decode_device_decimated_masked.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), i32, i32,
                                                             C.POINTER(Decoded), C.c_double, C.POINTER(u64)]
            L.fra_resample_masked_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_calc"):
            L.fra_calc_check.argtypes = [C.POINTER(CalcProgram), i32]
            L.fra_calc.argtypes = [vp, C.POINTER(CalcJob), C.POINTER(u64)]
            L.fra_decode_device_calc.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), C.POINTER(CalcProgram),
                                                 C.POINTER(CalcDst), C.POINTER(u64), C.POINTER(Decoded)]
            L.fra_calc_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_focal"):
            L.fra_focal_check.argtypes = [C.POINTER(FocalSpec)]
            L.fra_focal.argtypes = [vp, C.POINTER(FocalJob), C.POINTER(u64)]
            L.fra_decode_device_focal.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), C.POINTER(FocalSpec),
                                                  C.POINTER(Window), C.POINTER(CalcDst), C.POINTER(u64),
                                                  C.POINTER(Decoded)]
            L.fra_focal_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_zonal"):
            L.fra_zonal.argtypes = [vp, C.POINTER(ZonalJob), vp, C.POINTER(u64)]
            L.fra_decode_device_zonal.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), vp, i32, i32, C.c_int64,
                                                  C.c_int64, C.POINTER(ZonalOpts), vp, C.POINTER(u64),
                                                  C.POINTER(Decoded)]
            L.fra_zonal_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_warp"):
            L.fra_warp.argtypes = [vp, C.POINTER(WarpJob), C.POINTER(u64)]
            L.fra_decode_device_warped.argtypes = [vp, C.POINTER(DecodeJob), i32, i32, C.POINTER(WarpMap), i32, i32, i32,
                                                   i32, C.c_double, C.c_double, C.POINTER(Decoded), C.POINTER(u64)]
            L.fra_warp_source_window.argtypes = [C.POINTER(WarpMap), i32, i32, i32, i32, C.POINTER(Window)]
            L.fra_warp_timing.argtypes = [C.POINTER(C.c_float)]
            L.fra_warp_paths.argtypes = [C.POINTER(u64)]
        if hasattr(L, "fra_rasterize"):
            L.fra_rasterize.argtypes = [vp, C.POINTER(RasterizeJob), C.POINTER(u64)]
            L.fra_rasterize_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_proximity"):
            L.fra_proximity.argtypes = [vp, C.POINTER(ProximityJob), C.POINTER(u64)]
            L.fra_decode_device_proximity.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), C.POINTER(ProximityOpts),
                                                      C.POINTER(Decoded), C.POINTER(u64)]
            L.fra_proximity_timing.argtypes = [C.POINTER(C.c_float)]
        if hasattr(L, "fra_regions"):
            L.fra_regions.argtypes = [vp, C.POINTER(RegionsJob), C.POINTER(u64)]
            L.fra_decode_device_regions.argtypes = [vp, C.POINTER(DecodeJob), C.POINTER(Window), C.POINTER(RegionsOpts),
                                                    C.POINTER(Decoded), C.POINTER(u64)]
            L.fra_regions_timing.argtypes = [C.POINTER(C.c_float)]
        L.fra_tiff_compress_bound.argtypes = [i32, u64]
        L.fra_tiff_compress_bound.restype = u64
        L.fra_tiff_compress.argtypes = [i32, i32, vp, u64, i32, vp, u64, C.POINTER(u64), i32]
        _lib = L
        return L


def _check(rc: int):
    if rc != 0:
        msg = load().fra_last_error()
        raise NativeError(f"flac_raster_amd error {rc}: {msg.decode() if msg else ''}")


def _check_regions(rc: int, counts):
    if rc == E_SPACE:
        msg = load().fra_last_error()
        raise RegionsNoSpace(f"flac_raster_amd error {rc}: {msg.decode() if msg else ''}", counts)
    _check(rc)


def _masked_args(nodata, filled, dtype, channels: int):
    """``(nodata, fill counts pointer)`` of a nodata-aware entry, ``None`` without a nodata value."""
    if nodata is None:
        if filled is not None:
            raise ValueError("filled needs a nodata value")
        return None
    from .resample import check_nodata

    nd = check_nodata(nodata, dtype)
    if filled is None:
        return nd, None
    if not (isinstance(filled, np.ndarray) and filled.dtype == np.uint64 and filled.shape == (int(channels),)
            and filled.flags.c_contiguous and filled.flags.writeable):
        raise ValueError(f"filled must be a writable contiguous uint64 array of {int(channels)}")
    return nd, filled.ctypes.data_as(C.POINTER(C.c_uint64))


def calc_program(program, nodata=None, fill=None, out_dtype=None) -> CalcProgram:
    """The ``fra_calc_program`` of a ``calc.Program`` as it is -- nothing is checked here: the library's validator
    is the one that refuses -- with ``nodata`` (``None``: nothing is masked) and ``fill`` (``None``: the default of
    ``out_dtype``, NaN for floats and 0 for integers)."""
    from .calc import default_fill

    code = np.asarray(program.code, dtype=np.uint16).reshape(-1)
    consts = np.asarray(program.consts, dtype=np.float64).reshape(-1)
    p = CalcProgram()
    p.ncode, p.nconst, p.nout = code.size, consts.size, int(program.nout)
    p.flags = 0 if nodata is None else CALC_NODATA
    p.nodata = 0.0 if nodata is None else float(nodata)
    p.fill = float(fill) if fill is not None else default_fill(out_dtype if out_dtype is not None else np.float64)
    C.memmove(p.code, code.ctypes.data, min(code.size, 128) * 2)
    C.memmove(p.consts, consts.ctypes.data, min(consts.size, 32) * 8)
    return p


def calc_check(program, nbands: int, nodata=None) -> None:
    """``fra_calc_check``: raises :class:`NativeError` with the validator's message for an invalid program.  Pure host
    code: no GPU is needed."""
    p = calc_program(program, nodata)
    _check(load().fra_calc_check(C.byref(p), int(nbands)))


def focal_spec(spec, out_dtype=None) -> FocalSpec:
    """The ``fra_focal_spec`` of a ``focal.Spec`` as it is -- nothing is checked here: the library's validator is the
    one that refuses -- with the default ``fill`` of ``out_dtype`` (NaN for floats, 0 for integers) when the spec has
    none."""
    from .calc import default_fill

    s = FocalSpec()
    s.op, s.kh, s.kw, s.edge, s.flags = int(spec.op), int(spec.kh), int(spec.kw), int(spec.edge), spec.flag_bits()
    s.nodata = 0.0 if spec.nodata is None else float(spec.nodata)
    s.fill = float(spec.fill) if spec.fill is not None else default_fill(out_dtype if out_dtype is not None else np.float64)
    for k, v in enumerate(spec.params):
        s.params[k] = v
    if spec.weights is not None:
        w = np.ascontiguousarray(spec.weights, dtype=np.float64).reshape(-1)
        C.memmove(s.weights, w.ctypes.data, min(w.size, 225) * 8)
    return s


def focal_check(spec) -> None:
    """``fra_focal_check``: raises :class:`NativeError` with the validator's message for an invalid spec.  Pure host
    code: no GPU is needed."""
    s = focal_spec(spec)
    _check(load().fra_focal_check(C.byref(s)))


def warp_map(m) -> Tuple[WarpMap, list]:
    """The ``fra_warp_map`` of a ``warp.Map`` as it is -- nothing is checked here: the library is the one that refuses
    -- and what it points into, which must outlive the call."""
    w = WarpMap()
    w.kind, w.step = int(m.kind), int(m.step)
    for k, v in enumerate(tuple(m.affine)[:6]):
        w.affine[k] = float(v)
    keep = []
    if m.gx is not None and m.gy is not None:
        gx, gy = np.ascontiguousarray(m.gx, dtype=np.float64), np.ascontiguousarray(m.gy, dtype=np.float64)
        keep += [gx, gy]
        w.gh, w.gw = (int(v) for v in gx.shape) if gx.ndim == 2 else (0, 0)
        w.gx, w.gy = gx.ctypes.data_as(C.POINTER(C.c_double)), gy.ctypes.data_as(C.POINTER(C.c_double))
    return w, keep


def warp_source_window(m, raster_shape, out_shape):
    """``fra_warp_source_window``: the source window ``(row_off, col_off, height, width)`` a warped read decodes, or
    ``None`` when the map's footprint misses the raster.  Pure host code: no GPU is needed."""
    w, keep = warp_map(m)
    win = Window()
    rc = load().fra_warp_source_window(C.byref(w), int(raster_shape[0]), int(raster_shape[1]), int(out_shape[0]),
                                       int(out_shape[1]), C.byref(win))
    if rc < 0:
        _check(rc)
    return (win.row_off, win.col_off, win.height, win.width) if rc == 1 else None


def _warp_values(dtype, nodata, fill):
    """``(flags, nodata, fill)`` of a warp entry from the Python arguments (``warp.check_values``)."""
    from .warp import check_values

    nd, fl = check_values(dtype, nodata, fill)
    return (WARP_NODATA if nd is not None else 0), (0.0 if nd is None else nd), fl


def _filled_out(channels: int):
    f = np.zeros(int(channels), np.uint64)
    return f, f.ctypes.data_as(C.POINTER(C.c_uint64))


def _calc_dst(dst, dst_strides, out_dtype, shape) -> Tuple[CalcDst, object]:
    """The ``fra_calc_dst`` for an ``(nout, h, w)`` output: ``None`` (a new array), a numpy array view or a device
    pointer with element ``dst_strides`` (default band-planar); and what the caller returns."""
    dt = np.dtype(out_dtype)
    if dt not in DTYPE_CODES:
        raise TypeError(f"unsupported dtype {dt}")
    nout, h, w = shape
    o = CalcDst()
    o.dtype = DTYPE_CODES[dt]
    ret = dst
    if dst is None:
        ret = dst = np.zeros((max(nout, 0), max(h, 0), max(w, 0)), dtype=dt)
    if isinstance(dst, np.ndarray):
        if dst.shape != (nout, h, w) or dst.dtype != dt:
            raise ValueError(f"dst must be {(nout, h, w)} of {dt}, got {dst.shape} of {dst.dtype}")
        st = _element_strides(dst)
        o.dst, o.dst_on_device = C.c_void_p(dst.ctypes.data), 0
    else:
        st = tuple(int(v) for v in dst_strides) if dst_strides is not None else (h * w, w, 1)
        o.dst, o.dst_on_device = C.c_void_p(int(dst)), 1
    o.band_stride, o.row_stride, o.col_stride = st
    return o, ret


def proximity_opts(opts, out_window, src_dtype, shape, dist, alloc, dist_dtype, dist_strides, alloc_strides):
    """The ``fra_proximity_opts`` of a ``proximity.Options`` over a ``(B, h, w)`` region, and what the caller returns
    as ``(dist, alloc)``.  ``dist`` / ``alloc``: ``False`` (not wanted), ``None`` (a new array), a numpy array view
    ``(B, oh, ow)`` or a device pointer with element strides (default band-planar)."""
    from .proximity import default_fill

    B, h, w = shape
    win = (0, 0, h, w) if out_window is None else tuple(int(v) for v in out_window)
    o = ProximityOpts()
    vals = [float(v) for v in opts.values]
    o.nvalues = len(vals)
    for i, v in enumerate(vals[:16]):
        o.values[i] = v
    o.has_max_dist, o.max_dist = (0, 0.0) if opts.max_dist is None else (1, float(opts.max_dist))
    o.has_fixed, o.fixed = (0, 0.0) if opts.fixed is None else (1, float(opts.fixed))
    o.out_row_off, o.out_col_off, o.out_height, o.out_width = win
    o.scale, o.alloc_fill = float(opts.scale), float(opts.alloc_fill)
    ret_d = ret_a = None
    if dist is not False:
        o.fill = default_fill(dist_dtype) if opts.fill is None else float(opts.fill)
        o.dist, ret_d = _calc_dst(dist, dist_strides, dist_dtype, (B, win[2], win[3]))
    if alloc is not False:
        o.alloc, ret_a = _calc_dst(alloc, alloc_strides, src_dtype, (B, win[2], win[3]))
    return o, ret_d, ret_a


def regions_opts(opts, src_dtype, shape, labels, area, sieved, table, label_dtype, area_dtype, strides):
    """The ``fra_regions_opts`` of a ``regions.Options`` over a ``(B, h, w)`` region, and what the caller returns as
    ``(labels, area, sieved, table)``.  ``labels`` / ``area`` / ``sieved``: ``False`` (not wanted), ``None`` (a new
    array), a numpy array view ``(B, h, w)`` or a device pointer with the element strides ``strides[name]`` (default
    band-planar).  ``table``: ``False`` / ``None`` (none), a number of records per band (a new ``(B, cap)`` array of
    ``regions.REC``), such an array, or ``(device pointer, records per band)``."""
    from .regions import REC

    B, h, w = shape
    o = RegionsOpts()
    vals = [float(v) for v in opts.values]
    o.nvalues = len(vals)
    for i, v in enumerate(vals[:16]):
        o.values[i] = v
    o.invert, o.by_value = int(bool(opts.invert)), int(bool(opts.by_value))
    o.connectivity, o.min_size, o.sieve_fill = int(opts.connectivity), int(opts.min_size), float(opts.sieve_fill)
    strides = strides or {}
    ret_l = ret_a = ret_s = ret_t = None
    if labels is not False:
        o.labels, ret_l = _calc_dst(labels, strides.get("labels"), label_dtype, (B, h, w))
    if area is not False:
        o.area, ret_a = _calc_dst(area, strides.get("area"), area_dtype, (B, h, w))
    if sieved is not False:
        o.sieved, ret_s = _calc_dst(sieved, strides.get("sieved"), src_dtype, (B, h, w))
    if table is not None and table is not False:
        if isinstance(table, tuple):
            o.table, o.table_cap, o.table_on_device = C.c_void_p(int(table[0])), int(table[1]), 1
        else:
            if not isinstance(table, np.ndarray):
                table = np.zeros((B, max(int(table), 0)), REC) if int(table) >= 0 else int(table)
            if isinstance(table, np.ndarray):
                if table.dtype != REC or table.ndim != 2 or table.shape[0] != B or not table.flags.c_contiguous:
                    raise ValueError(f"table must be a C-contiguous ({B}, cap) array of regions.REC")
                ret_t = table
                o.table, o.table_cap = C.c_void_p(table.ctypes.data if table.size else _EMPTY_TABLE.ctypes.data), table.shape[1]
            else:
                o.table, o.table_cap = C.c_void_p(_EMPTY_TABLE.ctypes.data), table  # (a negative cap: the library refuses)
    return o, ret_l, ret_a, ret_s, ret_t


_EMPTY_TABLE = np.zeros(24, np.uint8)  # what a table of no records points at: the pointer says "wanted"


def _window_ref(w):
    """A ``fra_window`` argument from (row_off, col_off, height, width)."""
    return C.byref(Window(*[int(v) for v in w]))


def device_count() -> int:
    n = C.c_int(0)
    load().fra_device_count(C.byref(n))
    return n.value


def stream_header(channels: int, bps: int, sample_rate: int, blocksize: int = 4096) -> bytes:
    buf = (C.c_uint8 * 86)()
    _check(load().fra_stream_header(buf, channels, bps, sample_rate, blocksize))
    return bytes(buf)


_PIN_POOL_BYTES = int(os.environ.get("FRA_PINNED_POOL_MB", "8192")) << 20
_pin_pool: List[Tuple[int, int]] = []  # (capacity, ptr) of released page-locked blocks kept for reuse
_pin_lock = threading.RLock()  # re-entrant, as _lock


class _PinnedBlock:
    """Owner of one page-locked host allocation (``fra_host_alloc``), exposed to numpy.  Released blocks
    go to a small pool (``FRA_PINNED_POOL_MB``, default 8 GiB) because pinning pages costs far more than
    copying through them; the pool reuses a block of at most twice the requested size."""

    def __init__(self, nbytes: int):
        nbytes = max(1, int(nbytes))
        ptr, cap = None, 0
        with _pin_lock:
            best = None
            for k, (c, p) in enumerate(_pin_pool):
                if nbytes <= c <= 2 * nbytes and (best is None or c < _pin_pool[best][0]):
                    best = k
            if best is not None:
                cap, ptr = _pin_pool.pop(best)
        if ptr is None:
            p = C.c_void_p()
            _check(load().fra_host_alloc(nbytes, C.byref(p)))
            ptr, cap = p.value, nbytes
        self.ptr = ptr
        self.capacity = cap
        self.nbytes = nbytes
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            if not self.ptr:
                return
            ptr, self.ptr = self.ptr, None
            with _pin_lock:
                pooled = sum(c for c, _ in _pin_pool)
                if pooled + self.capacity <= _PIN_POOL_BYTES:
                    _pin_pool.append((self.capacity, ptr))
                    return
            load().fra_host_free(C.c_void_p(ptr))
        except Exception:
            pass


def release_pinned_pool():
    """Free every pooled page-locked block."""
    with _pin_lock:
        blocks = list(_pin_pool)
        _pin_pool.clear()
    for _, p in blocks:
        load().fra_host_free(C.c_void_p(p))


def pinned_empty(shape, dtype) -> np.ndarray:
    """``np.empty`` in page-locked host memory (full-rate PCIe DMA; freed with the array).  Needs the
    HIP runtime (a GPU box); raises :class:`NativeError` without one."""
    dt = np.dtype(dtype)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    return np.asarray(_PinnedBlock(n)).view(dt)[: n // dt.itemsize].reshape(shape)


def is_pinned(a: np.ndarray) -> bool:
    base = a
    while base is not None and not isinstance(base, _PinnedBlock):
        base = getattr(base, "base", None)
    return base is not None


class HostRegistration:
    """``hipHostRegister`` of an existing host array for the lifetime of a ``with`` block."""

    def __init__(self, a: np.ndarray):
        self.a = a
        self.ok = False

    def __enter__(self):
        if self.a.nbytes and not is_pinned(self.a):
            _check(load().fra_host_register(C.c_void_p(self.a.ctypes.data), self.a.nbytes))
            self.ok = True
        return self.a

    def __exit__(self, *exc):
        if self.ok:
            load().fra_host_unregister(C.c_void_p(self.a.ctypes.data))
            self.ok = False


def _raster_source(job, src, dtype, shape, strides):
    """Fills ``job.src`` / ``job.src_on_device`` / ``job.dtype`` / ``job.channels`` / ``job.height`` / ``job.width``
    from a raster given as a numpy array ``(B, h, w)`` / ``(h, w)`` or as a device pointer (int) with ``dtype``,
    ``shape`` and element ``strides`` (default band-planar); returns ``(dtype, (B, h, w), element strides)``."""
    if isinstance(src, np.ndarray):
        a = src if src.ndim == 3 else src[None]
        if a.ndim != 3:
            raise ValueError("src must be (B, h, w) or (h, w)")
        dt, (B, h, w), st = a.dtype, a.shape, _element_strides(a)
        job.src, job.src_on_device = C.c_void_p(a.ctypes.data), 0
    else:
        dt, (B, h, w) = np.dtype(dtype), (int(v) for v in shape)
        st = tuple(int(v) for v in strides) if strides is not None else (h * w, w, 1)
        job.src, job.src_on_device = C.c_void_p(int(src)), 1
    if dt not in DTYPE_CODES:
        raise TypeError(f"unsupported dtype {dt}")
    job.dtype, job.channels, job.height, job.width = DTYPE_CODES[dt], B, h, w
    return dt, (B, h, w), st


def _raster_job(job, src, dst, dtype, shape, strides, dst_strides, out_shape):
    """Fills what ``DecimateJob`` and ``ResampleJob`` share: the source (:func:`_raster_source`) and the destination
    ``(B, oh, ow)`` with ``(oh, ow) = out_shape(h, w)`` -- ``None`` (a new array), a numpy array view or a device
    pointer with element ``dst_strides`` (default band-planar).  Returns ``(what the caller returns, dtype, B)``."""
    dt, (B, h, w), sst = _raster_source(job, src, dtype, shape, strides)
    oh, ow = out_shape(h, w)
    ret = dst
    if dst is None:
        ret = dst = np.zeros((B, oh, ow), dtype=dt)
        if isinstance(src, np.ndarray) and src.ndim == 2:
            ret = dst[0]
    if isinstance(dst, np.ndarray):
        d = dst if dst.ndim == 3 else dst[None]
        if d.shape != (B, oh, ow) or d.dtype != dt:
            raise ValueError(f"dst must be {(B, oh, ow)} of {dt}, got {d.shape} of {d.dtype}")
        dstr = _element_strides(d)
        job.dst, job.dst_on_device = C.c_void_p(d.ctypes.data), 0
    else:
        dstr = tuple(int(v) for v in dst_strides) if dst_strides is not None else (oh * ow, ow, 1)
        job.dst, job.dst_on_device = C.c_void_p(int(dst)), 1
    job.src_band_stride, job.src_row_stride, job.src_col_stride = sst
    job.dst_band_stride, job.dst_row_stride, job.dst_col_stride = dstr
    return ret, dt, B


class Context:
    """One HIP device + stream (``fra_ctx``)."""

    def __init__(self, device: int = 0):
        L = load()
        if device_count() == 0:
            raise NativeUnavailable("no HIP device visible: the flac_raster encoder requires an MI355X (gfx950)")
        h = C.c_void_p()
        _check(L.fra_ctx_create(device, C.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            load().fra_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(load().fra_device_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr: int):
        _check(load().fra_device_free(self.h, C.c_void_p(ptr)))

    def h2d(self, dev: int, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        _check(load().fra_memcpy_h2d(self.h, C.c_void_p(dev), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def d2h(self, arr: np.ndarray, dev: int):
        _check(load().fra_memcpy_d2h(self.h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(dev), arr.nbytes))

    def normalize(self, data: np.ndarray, bps: int, data_min=None, data_max=None):
        """normalize_to_audio on this context's GPU (fra_normalize).  Returns (audio, mn, mx)."""
        a = np.ascontiguousarray(data)
        if a.dtype not in DTYPE_CODES:
            raise TypeError(f"unsupported dtype {a.dtype}")
        out = np.empty(a.shape, dtype=np.int16 if bps == 16 else np.int32)
        mn, mx = C.c_double(), C.c_double()
        omin = C.byref(C.c_double(float(data_min))) if data_min is not None else None
        omax = C.byref(C.c_double(float(data_max))) if data_max is not None else None
        _check(load().fra_normalize(self.h, a.ctypes.data_as(C.c_void_p), 0, DTYPE_CODES[a.dtype], a.size, bps, omin,
                                    omax, out.ctypes.data_as(C.c_void_p), C.byref(mn), C.byref(mx)))
        return out, mn.value, mx.value

    def _decode_job(self, data, items, dst, dst_dtype, denorm: int, channels: int, strides, concat: bool = False):
        """The ``DecodeJob`` of a decode call (arguments as :meth:`decode_device`; ``dst`` may be ``None`` for an entry
        that ignores it).  Returns ``(job, infos, keep)``: the per-stream :class:`Decoded` array the entry fills and
        what the job points into, which must outlive the call."""
        keep = []
        job = DecodeJob()
        if isinstance(data, tuple):
            job.data, job.len, job.data_on_device = C.c_void_p(int(data[0])), int(data[1]), 1
        else:
            buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
            if buf.dtype != np.uint8 or not buf.flags.c_contiguous:
                raise TypeError("data must be contiguous uint8")
            keep.append(buf)
            job.data, job.len, job.data_on_device = C.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, 0
        arr = (DecodeItem * max(1, len(items)))()
        for it, d in zip(arr, items):
            it.offset, it.bytes = int(d["offset"]), int(d["bytes"])
            it.window = Window(*[int(v) for v in d["window"]])
            it.data_min, it.data_max = float(d.get("data_min", 0.0)), float(d.get("data_max", 0.0))
            fo = d.get("frame_offsets")
            if fo is not None:
                fo = np.ascontiguousarray(fo, dtype=np.uint64)
                keep.append(fo)
                it.frame_offsets = fo.ctypes.data_as(C.POINTER(C.c_uint64))
                it.nframes = fo.size - 1
                it.channels, it.bps, it.blocksize = int(d["channels"]), int(d["bps"]), int(d["blocksize"])
        job.items, job.nitems = arr, len(items)
        job.flags = DECODE_CONCAT if concat else 0
        if dst is None:
            job.dst, job.dst_on_device = None, 0
        elif isinstance(dst, np.ndarray):
            job.dst, job.dst_on_device = C.c_void_p(dst.ctypes.data), 0
        else:
            job.dst, job.dst_on_device = C.c_void_p(int(dst)), 1
        job.dst_dtype = DTYPE_CODES[np.dtype(dst_dtype)]
        job.denorm = denorm
        job.channels = channels
        job.band_stride, job.row_stride, job.col_stride = (int(v) for v in strides)
        return job, (Decoded * max(1, len(items)))(), keep

    def _decode_run(self, entry: str, job, infos, keep, *args) -> List[Decoded]:
        """``entry(ctx, job, *args)`` of the library for a job of :meth:`_decode_job` (``keep`` is held until the call
        returns); the per-stream infos."""
        rc = getattr(load(), entry)(self.h, C.byref(job), *args)
        if rc == E_SPACE:
            raise OutputTooSmall(max(int(i.nsamples) for i in infos))
        _check(rc)
        return list(infos)[: job.nitems]

    def decode_device(self, data, items, dst, dst_dtype, channels: int, strides: Tuple[int, int, int],
                      denorm: int = DENORM_NONE, concat: bool = False) -> List[Decoded]:
        """Batched FLAC decode on this context's GPU (``fra_decode_device``): tile streams -> raster.

        ``data``: the bytes holding every stream -- bytes-like / uint8 array on the host, or ``(device pointer,
        length)``.  ``items``: one dict per stream with ``offset``, ``bytes``, ``window`` (row_off, col_off, height,
        width) and optionally ``data_min`` / ``data_max`` (denormalisation) and ``frame_offsets`` (uint64 array of
        nframes + 1 offsets relative to ``offset``; then also ``channels``, ``bps``, ``blocksize``: nothing is
        searched).  ``dst``: a numpy array (copied to the device and back, so elements outside the windows keep
        their values) or a device pointer (int); sample p of channel c of a stream lands at element
        ``c * strides[0] + (row_off + p // width) * strides[1] + (col_off + p % width) * strides[2]``.
        Returns the per-stream :class:`Decoded` infos.  Anything the device path does not cover raises
        :class:`NativeError`; there is no fallback to the host decoder."""
        job, infos, keep = self._decode_job(data, items, dst, dst_dtype, denorm, channels, strides, concat)
        return self._decode_run("fra_decode_device", job, infos, keep, infos)

    def decode_device_window(self, data, items, dst, dst_dtype, channels: int, strides: Tuple[int, int, int], roi,
                             denorm: int = DENORM_NONE) -> List[Decoded]:
        """The pixels of ``roi`` (row_off, col_off, height, width) only (``fra_decode_device_window``).

        Arguments as :meth:`decode_device`, except that every item's ``window`` is its tile's window in source-raster
        coordinates, ``roi`` is in the same coordinates, and ``dst`` is addressed relative to the region: raster pixel
        (R, C) of channel c lands at ``c * strides[0] + (R - roi[0]) * strides[1] + (C - roi[1]) * strides[2]``.  Only
        the frames that hold samples of the region are read and decoded; a tile outside it reports 0 frames.  The
        result is bit-identical to cropping the full decode."""
        if roi is None:
            raise ValueError("roi is required")
        job, infos, keep = self._decode_job(data, items, dst, dst_dtype, denorm, channels, strides)
        return self._decode_run("fra_decode_device_window", job, infos, keep, _window_ref(roi), infos)

    def decode_device_decimated(self, data, items, dst, dst_dtype, channels: int, strides: Tuple[int, int, int], roi,
                                factor: int, resampling: str = "nearest", denorm: int = DENORM_NONE, nodata=None,
                                filled=None) -> List[Decoded]:
        """``roi`` at ``1 / factor`` resolution (``fra_decode_device_decimated``): exactly
        ``resample.decimate`` of what :meth:`decode_device_window` would have written, without the full-resolution
        region leaving the GPU.

        Arguments as :meth:`decode_device_window`, except that ``dst`` and ``strides`` address the
        ``resample.decimated_shape(roi[2], roi[3], factor)`` output.  ``factor``: 2, 4, 8, 16, 32 or 64; ``resampling``:
        ``"nearest"`` or ``"average"``.  The items must cover the region.  ``nodata`` / ``filled``: as :meth:`decimate`
        (``fra_decode_device_decimated_masked``)."""
        from .resample import check_factor, resampling_code

        if roi is None:
            raise ValueError("roi is required")
        k, mode = check_factor(factor), resampling_code(resampling)
        masked = _masked_args(nodata, filled, dst_dtype, channels)
        job, infos, keep = self._decode_job(data, items, dst, dst_dtype, denorm, channels, strides)
        if masked is not None:
            return self._decode_run("fra_decode_device_decimated_masked", job, infos, keep, _window_ref(roi), k, mode,
                                    infos, float(masked[0]), masked[1])
        return self._decode_run("fra_decode_device_decimated", job, infos, keep, _window_ref(roi), k, mode, infos)

    def decimate(self, src, factor: int, resampling: str = "nearest", dst=None, *, dtype=None, shape=None,
                 strides=None, dst_strides=None, nodata=None, filled=None):
        """A raster at ``1 / factor`` resolution on this context's GPU (``fra_decimate``, the rule of
        ``flac_raster.resample``).

        ``src``: a numpy array ``(B, h, w)`` / ``(h, w)`` of one of the eight raster dtypes with any non-negative
        strides (a view is fine: it is copied to the device from its first element to its last), or a device pointer
        (int) with ``dtype``, ``shape`` = (B, h, w) and element ``strides`` (default band-planar).  ``dst``: ``None``
        (a new array is returned), a numpy array view ``(B, oh, ow)`` (the elements between its outputs keep their
        values), or a device pointer with element ``dst_strides`` (default band-planar).  Returns ``dst``.

        ``nodata``: the nodata-aware rule (``fra_decimate_masked``; ``ValueError`` for a value the dtype does not
        admit); ``filled``, then, an optional ``uint64`` array of ``B`` that receives per band the number of output
        pixels no valid pixel reached.  ``None`` is the unmasked kernel."""
        from .resample import check_factor, decimated_shape, resampling_code

        k, mode = check_factor(factor), resampling_code(resampling)
        job = DecimateJob()
        ret, dt, B = _raster_job(job, src, dst, dtype, shape, strides, dst_strides,
                                 lambda h, w: decimated_shape(h, w, k))
        job.factor, job.resampling = k, mode
        masked = _masked_args(nodata, filled, dt, B)
        if masked is not None:
            _check(load().fra_decimate_masked(self.h, C.byref(job), *masked))
        else:
            _check(load().fra_decimate(self.h, C.byref(job)))
        return ret

    def decimate_timing(self) -> float:
        """HIP-event ms of this thread's last ``k_decimate`` (:meth:`decimate` / :meth:`decode_device_decimated`)."""
        ms = C.c_float()
        _check(load().fra_decimate_timing(C.byref(ms)))
        return ms.value

    def decode_device_resampled(self, data, items, dst, dst_dtype, channels: int, strides: Tuple[int, int, int], roi,
                                out_shape, resampling: str = "nearest", denorm: int = DENORM_NONE, nodata=None,
                                filled=None) -> List[Decoded]:
        """``roi`` at ``out_shape`` = (oh, ow) (``fra_decode_device_resampled``): exactly ``resample.resample`` of what
        :meth:`decode_device_window` would have written, without the full-resolution region leaving the GPU.

        Arguments as :meth:`decode_device_window`, except that ``dst`` and ``strides`` address the ``(oh, ow)``
        output.  ``resampling``: ``"nearest"``, ``"average"``, ``"bilinear"`` or ``"cubic"``.  The items must cover
        the region.  ``nodata`` / ``filled``: as :meth:`decimate` (``fra_decode_device_resampled_masked``)."""
        from .resample import check_average_size, check_out_shape, resampling_any_code

        if roi is None:
            raise ValueError("roi is required")
        oh, ow = check_out_shape(out_shape)
        mode = resampling_any_code(resampling)
        if mode == RESAMPLE_AVERAGE and int(roi[2]) > 0 and int(roi[3]) > 0:
            check_average_size(int(roi[2]), int(roi[3]), oh, ow, dst_dtype)
        masked = _masked_args(nodata, filled, dst_dtype, channels)
        job, infos, keep = self._decode_job(data, items, dst, dst_dtype, denorm, channels, strides)
        if masked is not None:
            return self._decode_run("fra_decode_device_resampled_masked", job, infos, keep, _window_ref(roi), oh, ow,
                                    mode, infos, float(masked[0]), masked[1])
        return self._decode_run("fra_decode_device_resampled", job, infos, keep, _window_ref(roi), oh, ow, mode, infos)

    def resample(self, src, out_shape, resampling: str = "nearest", dst=None, *, dtype=None, shape=None,
                 strides=None, dst_strides=None, nodata=None, filled=None):
        """A raster at ``out_shape`` = (oh, ow) on this context's GPU (``fra_resample``, the rule of
        ``flac_raster.resample.resample``).

        ``src``, ``dst`` and the keyword arguments as :meth:`decimate`; ``dst`` is ``(B, oh, ow)``.  ``resampling``:
        ``"nearest"``, ``"average"``, ``"bilinear"`` or ``"cubic"``.  Returns ``dst``.  ``nodata`` / ``filled``: as
        :meth:`decimate` (``fra_resample_masked``)."""
        from .resample import check_out_shape, resampling_any_code

        (oh, ow), mode = check_out_shape(out_shape), resampling_any_code(resampling)
        job = ResampleJob()
        ret, dt, B = _raster_job(job, src, dst, dtype, shape, strides, dst_strides, lambda h, w: (oh, ow))
        job.out_height, job.out_width, job.resampling = oh, ow, mode
        masked = _masked_args(nodata, filled, dt, B)
        if masked is not None:
            _check(load().fra_resample_masked(self.h, C.byref(job), *masked))
        else:
            _check(load().fra_resample(self.h, C.byref(job)))
        return ret

    def resample_timing(self) -> float:
        """HIP-event ms of this thread's last ``k_resample`` (:meth:`resample` / :meth:`decode_device_resampled`)."""
        ms = C.c_float()
        _check(load().fra_resample_timing(C.byref(ms)))
        return ms.value

    def resample_masked_timing(self) -> float:
        """HIP-event ms of this thread's last ``k_resample_masked`` (any read with ``nodata``)."""
        ms = C.c_float()
        _check(load().fra_resample_masked_timing(C.byref(ms)))
        return ms.value

    def decode_device_compare(self, data, items, ref, dst_dtype, channels: int, roi, denorm: int = DENORM_NONE,
                              ref_strides=None) -> Tuple[List[CompareBand], List[Decoded]]:
        """``roi`` of the tile streams compared with a reference raster (``fra_decode_device_compare``): the reports of
        ``compare.compare_arrays(what decode_device_window would have written, ref)``, one per band, without the
        decoded region leaving the GPU.

        ``data``, ``items``, ``roi``, ``denorm`` as :meth:`decode_device_window`.  ``ref``: a numpy array ``(channels, h,
        w)`` of ``dst_dtype`` addressed relative to the region (a view with any non-negative strides is fine: it is
        copied to the device from its first element to its last), or a device pointer (int) with element
        ``ref_strides`` (default band-planar).  The items must cover the region.  Returns ``(reports, infos)``;
        ``first_row`` / ``first_col`` are relative to the region."""
        if roi is None:
            raise ValueError("roi is required")
        dt = np.dtype(dst_dtype)
        h, w = int(roi[2]), int(roi[3])
        if isinstance(ref, np.ndarray):
            if ref.shape != (channels, h, w) or ref.dtype != dt:
                raise ValueError(f"ref must be {(channels, h, w)} of {dt}, got {ref.shape} of {ref.dtype}")
            ptr, on_device, rst = ref.ctypes.data, 0, _element_strides(ref)
        else:
            ptr, on_device = int(ref), 1
            rst = tuple(int(v) for v in ref_strides) if ref_strides is not None else (h * w, w, 1)
        bands = (CompareBand * max(1, channels))()
        job, infos, keep = self._decode_job(data, items, None, dt, denorm, channels, (0, 0, 0))
        infos = self._decode_run("fra_decode_device_compare", job, infos, keep, _window_ref(roi), C.c_void_p(ptr),
                                 on_device, int(rst[0]), int(rst[1]), int(rst[2]), bands, infos)
        return list(bands)[:channels], infos

    def compare(self, a, b, *, dtype=None, shape=None, a_strides=None, b_strides=None) -> List[CompareBand]:
        """Two rasters compared on this context's GPU (``fra_compare``, the rule of ``flac_raster.compare``): one
        :class:`CompareBand` per band.

        ``a``, ``b``: numpy arrays ``(B, h, w)`` / ``(h, w)`` of one of the eight raster dtypes with any non-negative
        strides (views are fine: each is copied to the device from its first element to its last), or device pointers
        (int) with ``dtype``, ``shape`` = (B, h, w) and element strides (default band-planar).  Neither is written."""
        job = CompareJob()
        shp, dt = None, None
        sides = []
        for x, st in ((a, a_strides), (b, b_strides)):
            if isinstance(x, np.ndarray):
                v = x if x.ndim == 3 else x[None]
                if v.ndim != 3:
                    raise ValueError("rasters must be (B, h, w) or (h, w)")
                if (shp is not None and v.shape != shp) or (dt is not None and v.dtype != dt):
                    raise ValueError(f"the rasters differ in shape or dtype: {shp} of {dt}, {v.shape} of {v.dtype}")
                shp, dt = tuple(v.shape), v.dtype
                sides.append((v.ctypes.data, 0, _element_strides(v), v))
            else:
                sides.append((int(x), 1, st, None))
        if shp is None:
            shp, dt = tuple(int(v) for v in shape), np.dtype(dtype)
        elif (shape is not None and tuple(shape) != shp) or (dtype is not None and np.dtype(dtype) != dt):
            raise ValueError("shape / dtype disagree with the array given")
        if dt not in DTYPE_CODES:
            raise TypeError(f"unsupported dtype {dt}")
        B, h, w = shp
        sides = [(p, dev, tuple(int(v) for v in st) if st is not None else (h * w, w, 1), keep)
                 for p, dev, st, keep in sides]
        (job.a, job.a_on_device, ast, _), (job.b, job.b_on_device, bst, _) = sides
        job.a_band_stride, job.a_row_stride, job.a_col_stride = ast
        job.b_band_stride, job.b_row_stride, job.b_col_stride = bst
        job.dtype, job.channels, job.height, job.width = DTYPE_CODES[dt], B, h, w
        bands = (CompareBand * max(1, B))()
        _check(load().fra_compare(self.h, C.byref(job), bands))
        return list(bands)[:B]

    def compare_timing(self) -> float:
        """HIP-event ms of this thread's last ``k_compare`` + fold (:meth:`compare` / :meth:`decode_device_compare`)."""
        ms = C.c_float()
        _check(load().fra_compare_timing(C.byref(ms)))
        return ms.value

    @staticmethod
    def _stats_opts(bins, hist_range, nodata):
        """The ``StatsOpts`` of a request (checked by ``stats.check_options``)."""
        from .stats import check_options, flags_of

        bins, mode, nodata = check_options(bins, hist_range, nodata)
        o = StatsOpts()
        o.bins, o.flags = bins, flags_of(mode, nodata)
        if isinstance(mode, tuple):
            o.hist_lo, o.hist_hi = mode
        o.nodata = 0.0 if nodata is None else nodata
        return o

    def decode_device_stats(self, data, items, dst_dtype, channels: int, roi, denorm: int = DENORM_NONE, bins: int = 0,
                            hist_range=None, nodata=None):
        """The statistics of ``roi`` of the tile streams (``fra_decode_device_stats``): the records of
        ``stats.stats_arrays(what decode_device_window would have written, bins, hist_range, nodata)``, one per band,
        without the decoded region leaving the GPU.

        ``data``, ``items``, ``roi``, ``denorm`` as :meth:`decode_device_window`; ``bins``, ``hist_range``, ``nodata``
        as ``stats.stats_arrays``.  The items must cover the region.  Returns ``(reports, histogram (channels, bins)
        uint64 or None, infos)``."""
        if roi is None:
            raise ValueError("roi is required")
        o = self._stats_opts(bins, hist_range, nodata)
        bands = (StatsBand * max(1, channels))()
        hist = np.zeros((channels, o.bins), np.uint64) if o.bins else None
        hp = hist.ctypes.data_as(C.POINTER(C.c_uint64)) if hist is not None else None
        job, infos, keep = self._decode_job(data, items, None, np.dtype(dst_dtype), denorm, channels, (0, 0, 0))
        infos = self._decode_run("fra_decode_device_stats", job, infos, keep, _window_ref(roi), C.byref(o), bands, hp,
                                 infos)
        return list(bands)[:channels], hist, infos

    def stats(self, src, bins: int = 0, hist_range=None, nodata=None, *, dtype=None, shape=None, strides=None):
        """Band statistics and histograms of a raster on this context's GPU (``fra_stats``, the rule of
        ``flac_raster.stats``): ``(one StatsBand per band, histogram (B, bins) uint64 or None)``.

        ``src``: a numpy array ``(B, h, w)`` / ``(h, w)`` of one of the eight raster dtypes with any non-negative
        strides (a view is fine: it is copied to the device from its first element to its last), or a device pointer
        (int) with ``dtype``, ``shape`` = (B, h, w) and element ``strides`` (default band-planar).  It is not written.
        ``bins``, ``hist_range`` (``(lo, hi)``, ``"auto"`` / ``None``), ``nodata`` as ``stats.stats_arrays``."""
        job = StatsJob()
        _, (B, _, _), st = _raster_source(job, src, dtype, shape, strides)
        job.band_stride, job.row_stride, job.col_stride = st
        job.opts = self._stats_opts(bins, hist_range, nodata)
        bands = (StatsBand * max(1, B))()
        hist = np.zeros((B, job.opts.bins), np.uint64) if job.opts.bins else None
        hp = hist.ctypes.data_as(C.POINTER(C.c_uint64)) if hist is not None else None
        _check(load().fra_stats(self.h, C.byref(job), bands, hp))
        return list(bands)[:B], hist

    def stats_timing(self) -> float:
        """HIP-event ms of this thread's last statistics kernels (:meth:`stats` / :meth:`decode_device_stats`)."""
        ms = C.c_float()
        _check(load().fra_stats_timing(C.byref(ms)))
        return ms.value

    @staticmethod
    def _zonal_opts(zone_lo, nzones, nodata, ignore):
        from .zonal import flags_of

        o = ZonalOpts()
        o.flags, o.nzones, o.zone_lo = flags_of(nodata, ignore), int(nzones), int(zone_lo)
        o.ignore_zone = 0 if ignore is None else int(ignore)
        o.nodata = 0.0 if nodata is None else float(nodata)
        return o

    @staticmethod
    def _zone_raster(zones, zone_dtype, zone_strides, h: int, w: int):
        """``(pointer, on_device, dtype code, row stride, column stride, keepalive)`` of a zone raster given as a
        numpy array ``(h, w)`` of an integer dtype (any non-negative strides) or as a device pointer (int) with
        ``zone_dtype`` and element ``zone_strides`` = (row, column), default ``(w, 1)``."""
        if isinstance(zones, np.ndarray):
            if zones.shape != (h, w):
                raise ValueError(f"the zone raster must be {(h, w)}, got {zones.shape}")
            zdt = zones.dtype
            if any(st % zdt.itemsize for st in zones.strides):
                raise ValueError("the zone raster's strides must be whole elements")
            ptr, on_device, zst = zones.ctypes.data, 0, tuple(st // zdt.itemsize for st in zones.strides)
        else:
            zdt = np.dtype(zone_dtype)
            ptr, on_device = int(zones), 1
            zst = tuple(int(v) for v in zone_strides) if zone_strides is not None else (w, 1)
        if zdt not in DTYPE_CODES:
            raise TypeError(f"unsupported zone dtype {zdt}")
        return C.c_void_p(ptr), on_device, DTYPE_CODES[zdt], int(zst[0]), int(zst[1]), zones

    def zonal(self, src, zones, zone_lo: int = 0, nzones: int = 1, nodata=None, ignore=None, *, dtype=None, shape=None,
              strides=None, zone_dtype=None, zone_strides=None):
        """Zonal statistics of a raster on this context's GPU (``fra_zonal``, the rule of ``flac_raster.zonal``):
        ``(records (B, nzones) of zonal.REC_DTYPE, outside)``.

        ``src``: a numpy array ``(B, h, w)`` / ``(h, w)`` of one of the eight raster dtypes with any non-negative
        strides, or a device pointer (int) with ``dtype``, ``shape`` = (B, h, w) and element ``strides`` (default
        band-planar).  ``zones``: a numpy array ``(h, w)`` of an integer dtype of at most 32 bits with any
        non-negative strides, or a device pointer with ``zone_dtype`` and element ``zone_strides`` = (row, column).
        Neither is written.  ``zone_lo``, ``nzones``, ``nodata``, ``ignore`` as ``zonal.zonal_arrays``."""
        from .zonal import REC_DTYPE

        job = ZonalJob()
        _, (B, h, w), st = _raster_source(job, src, dtype, shape, strides)
        job.band_stride, job.row_stride, job.col_stride = st
        (job.zones, job.zones_on_device, job.zone_dtype, job.zone_row_stride, job.zone_col_stride,
         _keep) = self._zone_raster(zones, zone_dtype, zone_strides, h, w)
        job.opts = self._zonal_opts(zone_lo, nzones, nodata, ignore)
        recs = np.zeros((max(1, B), max(1, min(int(nzones), 65536))), REC_DTYPE)
        outside = C.c_uint64()
        _check(load().fra_zonal(self.h, C.byref(job), C.c_void_p(recs.ctypes.data), C.byref(outside)))
        return recs[:B], int(outside.value)

    def decode_device_zonal(self, data, items, zones, dst_dtype, channels: int, roi, denorm: int = DENORM_NONE,
                            zone_lo: int = 0, nzones: int = 1, nodata=None, ignore=None, *, zone_dtype=None,
                            zone_strides=None):
        """The zonal statistics of ``roi`` of the tile streams (``fra_decode_device_zonal``): the records of
        ``zonal.zonal_arrays(what decode_device_window would have written, zones, ...)`` without the decoded region
        leaving the GPU.

        ``data``, ``items``, ``roi``, ``denorm`` as :meth:`decode_device_window`.  ``zones`` is addressed relative to
        the region: a numpy array ``(h, w)`` of the region's size (a strided crop of a larger array is fine: it is
        copied to the device from its first element to its last), or a device pointer with ``zone_dtype`` and
        ``zone_strides``.  The items must cover the region.  Returns ``(records (channels, nzones), outside,
        infos)``."""
        from .zonal import REC_DTYPE

        if roi is None:
            raise ValueError("roi is required")
        h, w = int(roi[2]), int(roi[3])
        zp, z_on_device, zcode, zrs, zcs, _keep = self._zone_raster(zones, zone_dtype, zone_strides, h, w)
        o = self._zonal_opts(zone_lo, nzones, nodata, ignore)
        recs = np.zeros((max(1, channels), max(1, min(int(nzones), 65536))), REC_DTYPE)
        outside = C.c_uint64()
        job, infos, keep = self._decode_job(data, items, None, np.dtype(dst_dtype), denorm, channels, (0, 0, 0))
        infos = self._decode_run("fra_decode_device_zonal", job, infos, keep, _window_ref(roi), zp, z_on_device, zcode,
                                 zrs, zcs, C.byref(o), C.c_void_p(recs.ctypes.data), C.byref(outside), infos)
        return recs[:channels], int(outside.value), infos

    def zonal_timing(self) -> float:
        """HIP-event ms of this thread's last zonal kernels (:meth:`zonal` / :meth:`decode_device_zonal`)."""
        ms = C.c_float()
        _check(load().fra_zonal_timing(C.byref(ms)))
        return ms.value

    def calc(self, src, program, out_dtype="float32", dst=None, *, nodata=None, fill=None, dtype=None, shape=None,
             strides=None, dst_strides=None):
        """Band math over a raster on this context's GPU (``fra_calc``, the rule of ``flac_raster.calc``): ``(the
        (nout, h, w) result, the per-output count of left-out pixels)``.

        ``src``: as :meth:`stats`.  ``program``: a ``calc.Program`` (``calc.compile_exprs``); an invalid one is refused
        by the library before anything is launched.  ``dst``: ``None`` (a new array is returned), a numpy array view
        ``(nout, h, w)`` of ``out_dtype`` (the elements between its outputs keep their values) or a device pointer with
        element ``dst_strides`` (default band-planar).  ``nodata`` / ``fill``: as ``calc.calc_arrays``; the default
        ``fill`` is NaN for float outputs and 0 for integer ones."""
        job = CalcJob()
        _, (B, h, w), st = _raster_source(job, src, dtype, shape, strides)
        job.band_stride, job.row_stride, job.col_stride = st
        job.program = calc_program(program, nodata, fill, out_dtype)
        job.out, ret = _calc_dst(dst, dst_strides, out_dtype, (int(program.nout), h, w))
        left = np.zeros(max(1, int(program.nout)), np.uint64)
        _check(load().fra_calc(self.h, C.byref(job), left.ctypes.data_as(C.POINTER(C.c_uint64))))
        return ret, left[: int(program.nout)]

    def decode_device_calc(self, data, items, dst_dtype, channels: int, roi, program, out_dtype="float32", dst=None, *,
                           denorm: int = DENORM_NONE, nodata=None, fill=None, dst_strides=None):
        """Band math over ``roi`` of the tile streams (``fra_decode_device_calc``): ``calc.calc_arrays`` of what
        :meth:`decode_device_window` would have written in ``dst_dtype``, without the decoded region leaving the GPU.

        ``data``, ``items``, ``roi``, ``denorm`` as :meth:`decode_device_window`; ``program``, ``out_dtype``, ``dst``,
        ``nodata``, ``fill`` as :meth:`calc`.  The items must cover the region.  Returns ``(result, left-out counts,
        infos)``."""
        if roi is None:
            raise ValueError("roi is required")
        p = calc_program(program, nodata, fill, out_dtype)
        o, ret = _calc_dst(dst, dst_strides, out_dtype, (int(program.nout), int(roi[2]), int(roi[3])))
        left = np.zeros(max(1, int(program.nout)), np.uint64)
        job, infos, keep = self._decode_job(data, items, None, np.dtype(dst_dtype), denorm, channels, (0, 0, 0))
        infos = self._decode_run("fra_decode_device_calc", job, infos, keep, _window_ref(roi), C.byref(p), C.byref(o),
                                 left.ctypes.data_as(C.POINTER(C.c_uint64)), infos)
        return ret, left[: int(program.nout)], infos

    def calc_timing(self) -> float:
        """HIP-event ms of this thread's last ``k_calc`` (:meth:`calc` / :meth:`decode_device_calc`)."""
        ms = C.c_float()
        _check(load().fra_calc_timing(C.byref(ms)))
        return ms.value

    def focal(self, src, spec, out_dtype="float32", dst=None, *, out_window=None, dtype=None, shape=None, strides=None,
              dst_strides=None):
        """A focal operation over a raster on this context's GPU (``fra_focal``, the rule of ``flac_raster.focal``):
        ``(the (B, out_h, out_w) result, the per-band count of pixels that got fill)``.

        ``src``, ``dst``, ``dst_strides``: as :meth:`calc`.  ``spec``: a ``focal.Spec``; an invalid one is refused by the
        library before anything is launched.  ``out_window`` = (row_off, col_off, out_h, out_w) inside the source,
        default all of it: neighbours outside it are read."""
        job = FocalJob()
        _, (B, h, w), st = _raster_source(job, src, dtype, shape, strides)
        job.band_stride, job.row_stride, job.col_stride = st
        win = (0, 0, h, w) if out_window is None else tuple(int(v) for v in out_window)
        job.rect = Window(*win)
        job.spec = focal_spec(spec, out_dtype)
        job.out, ret = _calc_dst(dst, dst_strides, out_dtype, (B, win[2], win[3]))
        left = np.zeros(max(1, B), np.uint64)
        _check(load().fra_focal(self.h, C.byref(job), left.ctypes.data_as(C.POINTER(C.c_uint64))))
        return ret, left[:B]

    def decode_device_focal(self, data, items, dst_dtype, channels: int, roi, spec, inner, out_dtype="float32", dst=None,
                            *, denorm: int = DENORM_NONE, dst_strides=None):
        """A focal operation over the tile streams (``fra_decode_device_focal``): ``focal.focal_arrays`` of what
        :meth:`decode_device_window` would have written for ``roi`` in ``dst_dtype``, over the rectangle ``inner`` of
        it, without the decoded region leaving the GPU.

        ``data``, ``items``, ``roi``, ``denorm`` as :meth:`decode_device_window`; ``roi`` is the wanted rectangle grown
        by the window's radius and clipped to the raster, ``inner`` = (row_off, col_off, h, w) the wanted rectangle
        relative to it.  ``spec``, ``out_dtype``, ``dst`` as :meth:`focal`.  The items must cover ``roi``.  Returns
        ``(result, fill counts, infos)``."""
        if roi is None or inner is None:
            raise ValueError("roi and inner are required")
        s = focal_spec(spec, out_dtype)
        o, ret = _calc_dst(dst, dst_strides, out_dtype, (int(channels), int(inner[2]), int(inner[3])))
        left = np.zeros(max(1, int(channels)), np.uint64)
        job, infos, keep = self._decode_job(data, items, None, np.dtype(dst_dtype), denorm, channels, (0, 0, 0))
        infos = self._decode_run("fra_decode_device_focal", job, infos, keep, _window_ref(roi), C.byref(s),
                                 _window_ref(inner), C.byref(o), left.ctypes.data_as(C.POINTER(C.c_uint64)), infos)
        return ret, left[: int(channels)], infos

    def focal_timing(self) -> float:
        """HIP-event ms of this thread's last ``k_focal`` (:meth:`focal` / :meth:`decode_device_focal`)."""
        ms = C.c_float()
        _check(load().fra_focal_timing(C.byref(ms)))
        return ms.value

    def warp(self, src, out_shape, m, resampling: str = "bilinear", dst=None, *, nodata=None, fill=None, dtype=None,
             shape=None, strides=None, dst_strides=None):
        """A raster warped onto ``out_shape`` = (oh, ow) through the ``warp.Map`` ``m`` on this context's GPU
        (``fra_warp``, the rule of ``flac_raster.warp.warp_arrays``).

        ``src``, ``dst`` and the layout arguments as :meth:`resample`.  ``resampling``: ``"nearest"``, ``"bilinear"`` or
        ``"cubic"``.  ``nodata``: the nodata-aware sampling; ``fill``: what an outside pixel gets (``None``: the nodata
        value, else NaN for floats and 0 for integers).  Returns ``(dst, filled)``: per band the number of pixels
        written as the fill."""
        from .resample import check_out_shape
        from .warp import resampling_code

        (oh, ow), mode = check_out_shape(out_shape), resampling_code(resampling)
        job = WarpJob()
        ret, dt, B = _raster_job(job, src, dst, dtype, shape, strides, dst_strides, lambda h, w: (oh, ow))
        job.out_height, job.out_width, job.resampling = oh, ow, mode
        job.flags, job.nodata, job.fill = _warp_values(dt, nodata, fill)
        job.map, keep = warp_map(m)
        filled, fp = _filled_out(B)
        _check(load().fra_warp(self.h, C.byref(job), fp))
        del keep
        return ret, filled

    def decode_device_warped(self, data, items, dst, dst_dtype, channels: int, strides: Tuple[int, int, int],
                             raster_shape, out_shape, m, resampling: str = "bilinear", denorm: int = DENORM_NONE,
                             nodata=None, fill=None):
        """The tile streams' raster of ``raster_shape`` = (H, W) warped onto ``out_shape`` through ``m``
        (``fra_decode_device_warped``): exactly ``warp.warp_arrays`` of the full decode, with only the source window
        the map touches (``warp.source_window``) decoded and nothing but the output leaving the GPU.

        ``data``, ``items``, ``denorm`` as :meth:`decode_device_window` (the items must cover the source window);
        ``dst`` and ``strides`` address the ``(channels, oh, ow)`` output.  Returns ``(infos, filled)``."""
        from .resample import check_out_shape
        from .warp import resampling_code

        (oh, ow), mode = check_out_shape(out_shape), resampling_code(resampling)
        flags, nd, fl = _warp_values(dst_dtype, nodata, fill)
        w, keep_map = warp_map(m)
        job, infos, keep = self._decode_job(data, items, dst, dst_dtype, denorm, channels, strides)
        filled, fp = _filled_out(channels)
        infos = self._decode_run("fra_decode_device_warped", job, infos, keep, int(raster_shape[0]), int(raster_shape[1]),
                                 C.byref(w), oh, ow, mode, flags, nd, fl, infos, fp)
        del keep_map
        return infos, filled

    def warp_timing(self) -> float:
        """HIP-event ms of this thread's last ``k_warp`` (:meth:`warp` / :meth:`decode_device_warped`)."""
        ms = C.c_float()
        _check(load().fra_warp_timing(C.byref(ms)))
        return ms.value

    def warp_paths(self) -> Tuple[int, int]:
        """The workgroups of this thread's last ``k_warp`` that staged their footprint in LDS, and that gathered it."""
        counts = (C.c_uint64 * 2)()
        _check(load().fra_warp_paths(counts))
        return int(counts[0]), int(counts[1])

    def rasterize(self, features, window_or_shape, values=None, fill=0, dtype=np.int32, dst=None, *, dst_strides=None):
        """Polygon features burned into an integer raster on this context's GPU (``fra_rasterize``, the rule of
        ``flac_raster.rasterize.rasterize_arrays``).

        ``features``: a list of features, each a list of rings, each ``(n, 2)`` pixel coordinates.
        ``window_or_shape``: ``(h, w)`` or ``(row_off, col_off, h, w)``.  ``values``: an integer per feature (default
        ``i + 1``).  ``dst``: ``None`` (a new array), a numpy array ``(h, w)`` of ``dtype`` with any non-negative
        strides, or a device pointer (int) with element ``dst_strides`` = (row, column), default ``(w, 1)``.  Returns
        ``(raster, burned)``, the raster ``None`` for a device pointer."""
        from .rasterize import burn_values, flatten, window_of

        row_off, col_off, h, w = window_of(window_or_shape)
        features = list(features)
        xy, ring_start, feat_start = flatten(features)
        vals, fill, dt = burn_values(values, len(features), fill, dtype)
        job = RasterizeJob()
        job.xy, job.nverts = C.c_void_p(xy.ctypes.data), xy.shape[0]
        job.ring_start, job.nrings = C.c_void_p(ring_start.ctypes.data), ring_start.size - 1
        job.feature_ring_start, job.nfeatures = C.c_void_p(feat_start.ctypes.data), feat_start.size - 1
        job.values, job.dtype = C.c_void_p(vals.ctypes.data), DTYPE_CODES[dt]
        job.row_off, job.col_off, job.height, job.width, job.fill = row_off, col_off, h, w, fill
        ret = dst
        if dst is None:
            ret = dst = np.zeros((h, w), dtype=dt)
        if isinstance(dst, np.ndarray):
            if dst.shape != (h, w) or dst.dtype != dt:
                raise ValueError(f"dst must be {(h, w)} of {dt}, got {dst.shape} of {dst.dtype}")
            if any(st % dt.itemsize for st in dst.strides):
                raise ValueError("dst's strides must be whole elements")
            job.dst, job.dst_on_device = C.c_void_p(dst.ctypes.data), 0
            job.row_stride, job.col_stride = (st // dt.itemsize for st in dst.strides)
        else:
            job.dst, job.dst_on_device, ret = C.c_void_p(int(dst)), 1, None
            job.row_stride, job.col_stride = (int(v) for v in dst_strides) if dst_strides is not None else (w, 1)
        burned = C.c_uint64()
        _check(load().fra_rasterize(self.h, C.byref(job), C.byref(burned)))
        return ret, int(burned.value)

    def rasterize_timing(self) -> float:
        """HIP-event ms of this thread's last ``k_rasterize`` (:meth:`rasterize`)."""
        ms = C.c_float()
        _check(load().fra_rasterize_timing(C.byref(ms)))
        return ms.value

    def proximity(self, src, opts=None, dist_dtype="float32", dist=None, alloc=None, *, out_window=None, dtype=None,
                  shape=None, strides=None, dist_strides=None, alloc_strides=None):
        """Distance to the nearest target pixel and nearest-target allocation over a raster on this context's GPU
        (``fra_proximity``, the rule of ``flac_raster.proximity.proximity_arrays``): ``(dist, alloc, counts)``.

        ``src``: as :meth:`stats`.  ``opts``: a ``proximity.Options``.  ``dist`` / ``alloc``: ``None`` (a new array is
        returned), ``False`` (not wanted), a numpy array view ``(B, oh, ow)`` -- of ``dist_dtype`` and of the source's
        dtype -- whose elements between the outputs keep their values, or a device pointer with element
        ``dist_strides`` / ``alloc_strides`` (default band-planar).  ``out_window`` = (row_off, col_off, oh, ow) inside
        the source, default all of it: targets outside it count.  ``counts``: targets, output pixels within reach,
        output pixels filled, over all bands."""
        from .proximity import Options

        job = ProximityJob()
        dt, (B, h, w), st = _raster_source(job, src, dtype, shape, strides)
        job.band_stride, job.row_stride, job.col_stride = st
        job.opts, ret_d, ret_a = proximity_opts(opts or Options(), out_window, dt, (B, h, w), dist, alloc, dist_dtype,
                                                dist_strides, alloc_strides)
        counts = np.zeros(3, np.uint64)
        _check(load().fra_proximity(self.h, C.byref(job), counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        return ret_d, ret_a, counts

    def decode_device_proximity(self, data, items, dst_dtype, channels: int, roi, opts=None, dist_dtype="float32",
                                dist=None, alloc=None, *, out_window=None, denorm: int = DENORM_NONE,
                                dist_strides=None, alloc_strides=None):
        """:meth:`proximity` over ``roi`` of the tile streams (``fra_decode_device_proximity``): ``roi`` is the region
        -- the wanted window grown by the halo of ``max_dist`` and clipped to the raster -- and ``out_window`` the wanted
        window relative to it.  The decoded region never leaves the GPU.  ``data``, ``items``, ``roi``, ``denorm`` as
        :meth:`decode_device_window`; the items must cover ``roi``.  Returns ``(dist, alloc, counts, infos)``."""
        from .proximity import Options

        if roi is None:
            raise ValueError("roi is required")
        o, ret_d, ret_a = proximity_opts(opts or Options(), out_window, np.dtype(dst_dtype),
                                         (int(channels), int(roi[2]), int(roi[3])), dist, alloc, dist_dtype,
                                         dist_strides, alloc_strides)
        counts = np.zeros(3, np.uint64)
        job, infos, keep = self._decode_job(data, items, None, np.dtype(dst_dtype), denorm, channels, (0, 0, 0))
        infos = self._decode_run("fra_decode_device_proximity", job, infos, keep, _window_ref(roi), C.byref(o), infos,
                                 counts.ctypes.data_as(C.POINTER(C.c_uint64)))
        return ret_d, ret_a, counts, infos

    def proximity_timing(self) -> Tuple[float, float]:
        """HIP-event ms of the two phases (columns, rows) of this thread's last proximity call."""
        ms = (C.c_float * 2)()
        _check(load().fra_proximity_timing(ms))
        return float(ms[0]), float(ms[1])

    def regions(self, src, opts=None, label_dtype="int32", area_dtype="uint32", labels=None, area=False, sieved=False,
                table=None, *, dtype=None, shape=None, strides=None, out_strides=None):
        """Connected components, their areas and the sieve over a raster on this context's GPU (``fra_regions``, the
        rule of ``flac_raster.regions.regions_arrays``): ``(labels, area, sieved, table, counts)``.

        ``src``: as :meth:`stats`.  ``opts``: a ``regions.Options``.  ``labels`` / ``area`` / ``sieved``: ``None`` (a new
        array is returned), ``False`` (not wanted), a numpy array view ``(B, h, w)`` -- of ``label_dtype``, ``area_dtype``
        and the source's dtype -- whose elements between the outputs keep their values, or a device pointer with the
        element strides ``out_strides[name]`` (default band-planar).  ``table``: ``None`` (none), a number of records
        per band, a ``(B, cap)`` array of ``regions.REC`` or ``(device pointer, cap)``.  ``counts``: ``(B, 4)``:
        foreground pixels, components, kept components N, their pixels.  A band whose N does not fit ``label_dtype`` or
        the table raises :class:`RegionsNoSpace` with the complete ``counts`` as ``.counts``; nothing has been
        written then."""
        from .regions import Options

        job = RegionsJob()
        dt, (B, h, w), st = _raster_source(job, src, dtype, shape, strides)
        job.band_stride, job.row_stride, job.col_stride = st
        job.opts, ret_l, ret_a, ret_s, ret_t = regions_opts(opts or Options(), dt, (B, h, w), labels, area, sieved, table,
                                                            label_dtype, area_dtype, out_strides)
        counts = np.zeros((max(B, 0), 4), np.uint64)
        _check_regions(load().fra_regions(self.h, C.byref(job), counts.ctypes.data_as(C.POINTER(C.c_uint64))), counts)
        return ret_l, ret_a, ret_s, ret_t, counts

    def decode_device_regions(self, data, items, dst_dtype, channels: int, roi, opts=None, label_dtype="int32",
                              area_dtype="uint32", labels=None, area=False, sieved=False, table=None, *,
                              denorm: int = DENORM_NONE, out_strides=None):
        """:meth:`regions` over ``roi`` of the tile streams (``fra_decode_device_regions``): the decoded region never
        leaves the GPU.  ``data``, ``items``, ``roi``, ``denorm`` as :meth:`decode_device_window`; the items must cover
        ``roi``.  Returns ``(labels, area, sieved, table, counts, infos)``."""
        from .regions import Options

        if roi is None:
            raise ValueError("roi is required")
        B = int(channels)
        o, ret_l, ret_a, ret_s, ret_t = regions_opts(opts or Options(), np.dtype(dst_dtype), (B, int(roi[2]), int(roi[3])),
                                                     labels, area, sieved, table, label_dtype, area_dtype, out_strides)
        counts = np.zeros((max(B, 0), 4), np.uint64)
        job, infos, keep = self._decode_job(data, items, None, np.dtype(dst_dtype), denorm, channels, (0, 0, 0))
        rc = load().fra_decode_device_regions(self.h, C.byref(job), _window_ref(roi), C.byref(o), infos,
                                              counts.ctypes.data_as(C.POINTER(C.c_uint64)))
        del keep
        _check_regions(rc, counts)
        return ret_l, ret_a, ret_s, ret_t, counts, list(infos)[: job.nitems]

    def regions_timing(self) -> Tuple[float, float, float, float]:
        """HIP-event ms of the four phases (links, tiles, seams, the rest) of this thread's last regions call."""
        ms = (C.c_float * 4)()
        _check(load().fra_regions_timing(ms))
        return tuple(float(v) for v in ms)

    def decode_timing(self) -> List[float]:
        """HIP-event ms of this thread's last ``decode_device`` / ``decode_device_window``: parse, restore, scatter,
        first kernel to last."""
        ms = (C.c_float * 4)()
        _check(load().fra_decode_device_timing(ms))
        return list(ms)

    def synth(self, kind: int, seed: int, bands: int, height: int, width: int, dev_out: int):
        _check(load().fra_synth_raster(self.h, kind, seed, bands, height, width, C.c_void_p(dev_out)))


class Plan:
    """Device workspace for one job (``fra_plan``): windows of one raster -> FLAC frame streams."""

    def __init__(self, ctx: Context, raster_ptr: Optional[int], on_device: bool, dtype: np.dtype, channels: int,
                 strides: Tuple[int, int, int], windows: Sequence[Tuple[int, int, int, int]], level: int = 5,
                 blocksize: int = 4096, norm: int = 16, sample_rate: int = 0, keepalive=None,
                 frame_ranges: Optional[Sequence[Tuple[int, int]]] = None):
        """``frame_ranges``: per window (first frame, count; count -1 = to the end) -- the plan encodes only
        those frames of each window's stream (``fra_plan_create_ranged``; normalisation over the whole
        window, frame numbers of the whole stream)."""
        L = load()
        self.ctx = ctx
        self.nwin = len(windows)
        self.windows = [tuple(int(v) for v in w) for w in windows]
        self.strides = tuple(int(v) for v in strides)
        self.blocksize = blocksize
        self._wins = (Window * max(1, self.nwin))(*[Window(*w) for w in windows])
        self._keep = keepalive
        job = Job()
        job.raster = C.c_void_p(raster_ptr) if raster_ptr else None
        job.raster_on_device = 1 if on_device else 0
        job.dtype = DTYPE_CODES[np.dtype(dtype)]
        job.channels = channels
        job.band_stride, job.row_stride, job.col_stride = strides
        job.windows = self._wins
        job.nwindows = self.nwin
        job.level = level
        job.blocksize = blocksize
        job.norm = norm
        job.sample_rate = sample_rate
        h = C.c_void_p()
        if frame_ranges is None:
            _check(L.fra_plan_create(ctx.h, C.byref(job), C.byref(h)))
        else:
            if len(frame_ranges) != self.nwin:
                raise ValueError("one (first, count) frame range per window")
            self._ranges = (C.c_int32 * max(2, 2 * self.nwin))(*[int(v) for fr in frame_ranges for v in fr])
            _check(L.fra_plan_create_ranged(ctx.h, C.byref(job), self._ranges, C.byref(h)))
        self.h = h

    def set_raster(self, ptr: int, on_device: bool, keepalive=None):
        self._keep = keepalive
        _check(load().fra_plan_set_raster(self.h, C.c_void_p(ptr), 1 if on_device else 0))

    def execute(self):
        _check(load().fra_plan_execute(self.h))

    def sync(self):
        _check(load().fra_plan_sync(self.h))

    def result(self) -> Tuple[List[StreamInfo], int]:
        infos = (StreamInfo * max(1, self.nwin))()
        total = C.c_uint64()
        _check(load().fra_plan_result(self.h, infos, C.byref(total)))
        return list(infos)[: self.nwin], total.value

    def download(self) -> Tuple[List[StreamInfo], bytes]:
        infos, total = self.result()
        buf = np.empty(max(1, total), dtype=np.uint8)
        _check(load().fra_plan_download(self.h, buf.ctypes.data_as(C.c_void_p), total))
        return infos, buf[:total].tobytes()

    def set_first_frame(self, n: int):
        """FLAC frame number of every stream's first frame for the next execute (pyflac shim)."""
        _check(load().fra_plan_set_first_frame(self.h, int(n)))

    def flags(self) -> int:
        """``FRA_PLAN_*`` bits: 2 cross-execute pipelined, 4 full frames on the per-wave analysis kernel, 8 (with 4)
        its next execute keeps residuals up to 17 bits (else 16; picked per execute from an earlier one's count of
        waves that needed bit 16); 1, direct write, is never set since r03.  The load paths of the next execute for
        the current raster pointer: 16 (``PLAN_LOAD_VEC8``) the analysis loads 8-byte sample vectors, 32 / 64
        (``PLAN_MINMAX_VEC16`` / ``PLAN_MINMAX_VEC8``) the min/max pass loads 16- / 8-byte vectors, 128
        (``PLAN_OFF32``) 32-bit lane offsets."""
        f = C.c_int32()
        _check(load().fra_plan_flags(self.h, C.byref(f)))
        return f.value

    def capacity(self) -> Tuple[int, int]:
        """(upper bound of the output bytes, number of host-pipeline row bands)."""
        cap, nb = C.c_uint64(), C.c_int32()
        _check(load().fra_plan_capacity(self.h, C.byref(cap), C.byref(nb)))
        return cap.value, nb.value

    def encode_host(self, raster: np.ndarray, out: np.ndarray) -> int:
        """Pipelined host raster -> host frames (``fra_plan_encode_host``): row bands of the raster go
        H2D while earlier bands are analysed, and each band's frames come back D2H as soon as they are
        assembled.  ``raster`` must have the plan's dtype/strides; ``out`` is a uint8 buffer (page-locked
        for full rate).  Returns the total frame bytes; raises :class:`OutputTooSmall` (with ``.needed``)
        if ``out`` is too small -- the frames then stay on the device (``download``)."""
        total = C.c_uint64()
        self._keep = raster
        rc = load().fra_plan_encode_host(self.h, C.c_void_p(raster.ctypes.data), C.c_void_p(out.ctypes.data),
                                         out.nbytes, C.byref(total))
        if rc == E_SPACE:
            raise OutputTooSmall(total.value)
        _check(rc)
        return total.value

    def encode_host_progress(self, raster: np.ndarray, out: np.ndarray, rows_ready: np.ndarray) -> int:
        """:meth:`encode_host` over a raster still being produced (``fra_plan_encode_host_progress``): a
        producer thread fills ``raster`` top to bottom and publishes the rows done in ``rows_ready[0]``
        (int64; -1 = failed); each row band's H2D copy waits for its rows."""
        if rows_ready.dtype != np.int64 or rows_ready.size < 1:
            raise ValueError("rows_ready must be an int64 array of >= 1 element")
        total = C.c_uint64()
        self._keep = raster
        rc = load().fra_plan_encode_host_progress(self.h, C.c_void_p(raster.ctypes.data),
                                                  C.c_void_p(out.ctypes.data), out.nbytes, C.byref(total),
                                                  C.c_void_p(rows_ready.ctypes.data))
        if rc == E_SPACE:
            raise OutputTooSmall(total.value)
        _check(rc)
        return total.value

    def host_band_rows(self) -> int:
        """Rows of the tallest host row band (``fra_plan_host_band_rows``)."""
        m = C.c_int64()
        _check(load().fra_plan_host_band_rows(self.h, C.byref(m)))
        return m.value

    def encode_ring(self, ring: np.ndarray, out: np.ndarray, rows_ready: np.ndarray, rows_done: np.ndarray) -> int:
        """:meth:`encode_host_progress` with bounded host memory (``fra_plan_encode_ring``): ``ring`` is
        ``(B, ring_rows, W)`` and holds image row r at ring row ``r % ring_rows``; the call publishes in
        ``rows_done[0]`` the rows whose H2D copy completed (the producer may then reuse their ring rows)."""
        for a in (rows_ready, rows_done):
            if a.dtype != np.int64 or a.size < 1:
                raise ValueError("rows_ready / rows_done must be int64 arrays of >= 1 element")
        total = C.c_uint64()
        self._keep = ring
        rc = load().fra_plan_encode_ring(self.h, C.c_void_p(ring.ctypes.data), ring.shape[1],
                                         C.c_void_p(out.ctypes.data), out.nbytes, C.byref(total),
                                         C.c_void_p(rows_ready.ctypes.data), C.c_void_p(rows_done.ctypes.data))
        if rc == E_SPACE:
            raise OutputTooSmall(total.value)
        _check(rc)
        return total.value

    def frame_offsets(self, nframes: int) -> np.ndarray:
        """Byte offset of every frame in the concatenated output (+ total at the end)."""
        off = np.empty(nframes + 1, dtype=np.uint64)
        _check(load().fra_plan_frame_offsets(self.h, off.ctypes.data_as(C.POINTER(C.c_uint64)), nframes + 1))
        return off

    def device_output(self) -> Tuple[int, int]:
        p, cap = C.c_void_p(), C.c_uint64()
        _check(load().fra_plan_device_output(self.h, C.byref(p), C.byref(cap)))
        return p.value, cap.value

    def verify(self) -> List[VerifyReport]:
        """libFLAC's verify mode for this plan (``fra_plan_verify``): decode the frames of the last execute /
        ``encode_host`` / ``encode_ring`` on the GPU and compare every sample with the plan's current raster,
        normalised anew.  One :class:`VerifyReport` per window (``mismatches == 0`` and ``first_sample == -1`` when
        clean); a frame that does not parse or fails its CRC-16 raises :class:`NativeError`.  No second raster is
        allocated.  :func:`raise_on_mismatch` turns the reports into :class:`VerifyMismatch`."""
        reports = (VerifyReport * max(1, self.nwin))()
        bad = C.c_int32()
        _check(load().fra_plan_verify(self.h, reports, C.byref(bad)))
        return list(reports)[: self.nwin]

    def enable_timing(self, on: bool = True):
        _check(load().fra_plan_enable_timing(self.h, 1 if on else 0))

    def timing(self) -> Tuple[List[float], int]:
        ms = (C.c_float * 4)()
        n = C.c_int32()
        _check(load().fra_plan_timing(self.h, ms, C.byref(n)))
        return list(ms), n.value

    def close(self):
        if getattr(self, "h", None):
            load().fra_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mismatch_pixel(window, first_sample: int, first_channel: int) -> Tuple[int, int, int]:
    """``(row, col, band)`` in raster coordinates of sample ``first_sample`` (window-relative pixel index, row-major)
    of channel ``first_channel`` of ``window`` (row_off, col_off, height, width)."""
    r0, c0, _, w = (int(v) for v in window)
    return r0 + int(first_sample) // w, c0 + int(first_sample) % w, int(first_channel)


def raise_on_mismatch(reports: Sequence[VerifyReport], windows):
    """Raise :class:`VerifyMismatch` for the first report with mismatches (``windows``: the plan's windows)."""
    bad = [k for k, r in enumerate(reports) if r.mismatches]
    if not bad:
        return
    k = bad[0]
    r = reports[k]
    pixel = mismatch_pixel(windows[k], r.first_sample, r.first_channel)
    raise VerifyMismatch(k, pixel, int(r.expected), int(r.got), int(r.mismatches), len(bad))


_default_ctx = {}

# Process-wide pool of idle plans keyed by job shape: the reference creates one encoder per tile
# (spatial_encoder.py:291-304), and tiles of one raster share a few shapes, so a released plan (with its
# page-locked output buffer) is handed to the next encoder of the same shape instead of rebuilding the
# device workspace (~20 ms of allocations and table uploads).  Plans are used by one owner at a time.
_PLAN_POOL_MAX = int(os.environ.get("FRA_PLAN_POOL", "16"))
_plan_pool: "dict" = {}
_plan_pool_n = 0


def acquire_plan(key, factory):
    """An idle pooled plan entry for ``key`` or a new one from ``factory()``; the caller owns it until
    :func:`release_plan`."""
    global _plan_pool_n
    with _lock:
        lst = _plan_pool.get(key)
        if lst:
            _plan_pool_n -= 1
            return lst.pop()
    return factory()


def release_plan(key, entry):
    """Return a plan entry ``(plan, ...)`` to the pool (closed instead when the pool is full)."""
    global _plan_pool_n
    with _lock:
        if _plan_pool_n < _PLAN_POOL_MAX:
            _plan_pool.setdefault(key, []).append(entry)
            _plan_pool_n += 1
            return
    entry[0].close()


def default_context(device: int = 0) -> Context:
    with _lock:
        ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = Context(device)
        with _lock:
            _default_ctx[device] = ctx
    return ctx


def _element_strides(a: np.ndarray) -> Tuple[int, int, int]:
    es = a.dtype.itemsize
    if any(st < 0 or st % es for st in a.strides):
        raise ValueError("raster strides must be non-negative multiples of the item size")
    return tuple(st // es for st in a.strides)


def encode_windows_buffer(raster: np.ndarray, windows, level: int = 5, blocksize: int = 4096, norm: int = 16,
                          sample_rate: int = 0, device: int = 0, pinned: bool = True,
                          rows_ready: Optional[np.ndarray] = None, frame_ranges=None, verify: bool = False):
    """Encode windows of a band-planar host raster ``(B, H, W)`` (any non-negative strides, e.g. a row
    band view of a larger raster) through the pipelined host path (``fra_plan_encode_host``).

    Returns ``(infos, frames)``: ``frames`` is a uint8 array (page-locked unless ``pinned=False``) with
    every window's FLAC frames concatenated in window order; ``infos[i].offset/.frame_bytes`` slice it.
    ``rows_ready``: the raster is still being filled by a producer thread that publishes the rows done
    in ``rows_ready[0]`` (``fra_plan_encode_host_progress``).  ``frame_ranges``: (first frame, count) per
    window (``fra_plan_create_ranged``).  ``verify``: decode the plan's frames on the GPU and compare them with the
    plan's copy of the raster before the plan is closed (:meth:`Plan.verify`); raises :class:`VerifyMismatch`.
    """
    a = np.asarray(raster)
    if a.ndim == 2:
        a = a[None]
    if a.dtype not in DTYPE_CODES:
        raise TypeError(f"unsupported dtype {a.dtype}")
    if not a.dtype.isnative:
        a = a.astype(a.dtype.newbyteorder("="))
    B = a.shape[0]
    ctx = default_context(device)
    plan = Plan(ctx, None, False, a.dtype, B, _element_strides(a), windows, level, blocksize, norm, sample_rate,
                frame_ranges=frame_ranges)
    try:
        cap, _ = plan.capacity()
        out = pinned_empty(cap, np.uint8) if pinned else np.empty(cap, np.uint8)
        total = plan.encode_host(a, out) if rows_ready is None else plan.encode_host_progress(a, out, rows_ready)
        if verify:
            raise_on_mismatch(plan.verify(), plan.windows)
        infos, _ = plan.result()
        return infos, out[:total]
    finally:
        plan.close()


def ring_rows_for(band_rows: int, step: int, height: int) -> int:
    """Ring height for :func:`encode_windows_ring`: two host bands + one producer step (so the producer
    decodes band b+1 while band b is copied; band + step is the minimum that cannot deadlock), in whole
    producer steps, capped at the raster height."""
    step = max(1, step)
    rows = -(-(2 * band_rows + step) // step) * step
    return int(min(height, rows))


def encode_windows_ring(shape, dtype, windows, fill, level: int = 5, blocksize: int = 4096, norm: int = 16,
                        sample_rate: int = 0, device: int = 0, step: int = 0, ring_rows: int = 0,
                        verify: bool = False):
    """Encode windows of a band-planar raster of ``shape`` ``(B, H, W)`` that never exists whole in host
    memory (``fra_plan_encode_ring``): a producer thread calls ``fill(dst, r0, r1)`` to write image rows
    ``[r0, r1)`` of every band into ``dst`` (a ``(B, r1 - r0, W)`` view of a page-locked ring), in steps of
    ``step`` rows (default: the tallest host band), top to bottom; each step waits until the encoder's H2D
    copies have released its ring rows.  Host memory: the ring (``ring_rows`` rows, default
    :func:`ring_rows_for`) + the frames (a lazily committed buffer: only the written bytes are resident).

    ``verify``: as :func:`encode_windows_buffer` (the plan's device copy holds the whole raster after the pass).

    Returns ``(infos, frames, ring_rows)`` as :func:`encode_windows_buffer` (``frames`` not page-locked)."""
    B, H, W = shape
    dt = np.dtype(dtype)
    if dt not in DTYPE_CODES:
        raise TypeError(f"unsupported dtype {dt}")
    ctx = default_context(device)
    plan = Plan(ctx, None, False, dt, B, (H * W, W, 1), windows, level, blocksize, norm, sample_rate)
    th = None
    rows_ready = np.zeros(1, np.int64)
    rows_done = np.zeros(1, np.int64)
    stop = []
    try:
        band = max(1, plan.host_band_rows())
        step = int(step) if step and step > 0 else band
        R = int(ring_rows) if ring_rows else ring_rows_for(band, step, H)
        if R < min(H, band + step):
            raise ValueError(f"ring of {R} rows < band {band} + step {step}")
        ring = pinned_empty((B, R, W), dt)
        cap, _ = plan.capacity()
        out = np.empty(cap, np.uint8)  # pages are committed as the frames land
        errors: list = []

        def produce():
            try:
                r0 = 0
                while r0 < H:
                    r1 = min(H, r0 + step)
                    while rows_done[0] < r1 - R:  # the encoder still copies these ring rows
                        if stop:
                            return
                        time.sleep(0.0002)
                    r = r0
                    while r < r1:  # split where the ring wraps
                        rr = r % R
                        n = min(r1 - r, R - rr)
                        fill(ring[:, rr:rr + n, :], r, r + n)
                        r += n
                    rows_ready[0] = r1
                    r0 = r1
            except BaseException as e:  # reported to the encoder (rows_ready = -1), re-raised below
                errors.append(e)
                rows_ready[0] = -1

        th = threading.Thread(target=produce, name="ring-producer", daemon=True)
        th.start()
        try:
            total = plan.encode_ring(ring, out, rows_ready, rows_done)
        except BaseException:
            stop.append(1)
            th.join()
            if errors:
                raise errors[0]
            raise
        th.join()
        if errors:
            raise errors[0]
        if verify:
            raise_on_mismatch(plan.verify(), plan.windows)
        infos, _ = plan.result()
        return infos, out[:total], R
    finally:
        plan.close()


def encode_windows(raster: np.ndarray, windows, level: int = 5, blocksize: int = 4096, norm: int = 16,
                   sample_rate: int = 0, device: int = 0, path: str = "host"):
    """Encode windows of a band-planar host raster ``(B, H, W)`` (or ``(H, W)``).

    Returns ``(infos, frames_bytes)``: ``frames_bytes`` holds every window's FLAC frames
    concatenated in window order; ``infos[i].offset/.frame_bytes`` slice it.  ``path="host"`` is the
    pipelined host path (``fra_plan_encode_host``); ``path="device"`` copies the whole raster first and
    runs ``fra_plan_execute`` (frame groups per ``FRA_GROUPS``) then ``fra_plan_download``.
    """
    if path == "host":
        infos, buf = encode_windows_buffer(raster, windows, level, blocksize, norm, sample_rate, device)
        return infos, buf.tobytes()
    a = np.ascontiguousarray(raster)
    if a.ndim == 2:
        a = a[None]
    B, H, W = a.shape
    ctx = default_context(device)
    plan = Plan(ctx, a.ctypes.data, False, a.dtype, B, (H * W, W, 1), windows, level, blocksize, norm,
                sample_rate, keepalive=a)
    try:
        plan.execute()
        plan.sync()
        return plan.download()
    finally:
        plan.close()


def encode_interleaved(samples: np.ndarray, sample_rate: int, level: int = 5, blocksize: int = 4096,
                       device: int = 0, return_offsets: bool = False):
    """pyflac ``StreamEncoder.process(samples); finish()`` semantics: samples (N, C) int16/int32
    already in the audio domain; bps = itemsize*8.  Returns (info, frames) or, with
    ``return_offsets``, (info, frames, per-frame byte offsets + total)."""
    s = np.asarray(samples)
    if s.ndim == 1:
        s = s.reshape(-1, 1)
    if s.dtype not in (np.int16, np.int32):
        s = s.astype(np.int32)
    s = np.ascontiguousarray(s)
    N, Ch = s.shape
    ctx = default_context(device)
    # treat the (N, C) array as one raster row of N pixels with C interleaved bands
    plan = Plan(ctx, s.ctypes.data, False, s.dtype, Ch, (1, N * Ch, Ch), [(0, 0, 1, N)] if N else [(0, 0, 0, 0)],
                level, blocksize, 0, sample_rate, keepalive=s)
    try:
        plan.execute()
        plan.sync()
        infos, data = plan.download()
        if return_offsets:
            return infos[0], data, plan.frame_offsets(infos[0].nframes)
        return infos[0], data
    finally:
        plan.close()

def decode(data: bytes, concat: bool = False) -> Tuple[np.ndarray, Decoded]:
    """Native FLAC decode (fra_decode; host code, no GPU needed).  Returns ((N, C) int32, info)."""
    L = load()
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, np.uint8)
    info = Decoded()
    ptr = C.POINTER(C.c_int32)()
    _check(L.fra_decode(buf.ctypes.data_as(C.c_void_p), len(data), DECODE_CONCAT if concat else 0, C.byref(info),
                        C.byref(ptr)))
    try:
        n = info.nsamples * info.channels
        out = np.ctypeslib.as_array(ptr, shape=(max(1, n),))[:n].copy() if n else np.zeros(0, np.int32)
    finally:
        L.fra_free(ptr)
    return out.reshape(-1, info.channels), info


def decode_on_device(data: bytes, concat: bool = False, device: int = 0) -> Tuple[np.ndarray, Decoded]:
    """:func:`decode` on the GPU (``fra_decode_device``, ``FRA_DENORM_NONE``) -> ((N, C) int16 for streams of
    <= 16 bps / int32 otherwise, info).  The sample count is only known after the frames are parsed: the call is made
    with room for STREAMINFO's total (or a guess from the size) and repeated once with the count the library reports
    when that was too small."""
    from . import flac_meta

    data = bytes(data)
    at = 0
    if data[:3] == b"ID3" and len(data) >= 10:
        at = 10 + ((data[6] & 0x7F) << 21 | (data[7] & 0x7F) << 14 | (data[8] & 0x7F) << 7 | (data[9] & 0x7F))
    try:
        f = flac_meta.FLACFile(data[at:])
    except Exception as e:  # (damaged metadata: the same verdict as the decoders')
        raise NativeError(f"not a FLAC stream: {e}") from e
    ch, bps = f.channels, f.bits_per_sample
    dt = np.dtype(np.int16 if bps <= 16 else np.int32)
    buf = np.frombuffer(data, dtype=np.uint8)
    ctx = default_context(device)
    room = int(f.total_samples) if f.total_samples and not concat else max(4096, min(1 << 24, 2 * len(data) // ch))
    for attempt in (0, 1):
        out = np.zeros((room, ch), dtype=dt)
        job_items = [{"offset": 0, "bytes": buf.size, "window": (0, 0, -room, 1)}]
        try:
            info = ctx.decode_device(buf, job_items, out, dt, ch, (1, ch, 0), DENORM_NONE, concat)[0]
            return out[:info.nsamples], info
        except OutputTooSmall as e:
            if attempt:
                raise
            room = e.needed
    raise AssertionError("unreachable")


def tiff_compress(compression: int, chunks: np.ndarray, level: int = 6, threads: int = 0):
    """Compress equal-size raw TIFF chunks (``chunks``: uint8 array (nchunks, chunk_bytes), file layout,
    predictor already applied) with LZW (5) or deflate (8) on the native thread pool
    (``fra_tiff_compress``).  Returns a list of ``bytes``, one per chunk."""
    chunks = np.ascontiguousarray(chunks, dtype=np.uint8)
    n, cb = chunks.shape
    L = load()
    stride = int(L.fra_tiff_compress_bound(int(compression), int(cb)))
    dst = np.empty(max(1, n) * stride, np.uint8)
    sizes = np.zeros(max(1, n), np.uint64)
    _check(L.fra_tiff_compress(int(compression), int(level), C.c_void_p(chunks.ctypes.data), int(cb), int(n),
                               C.c_void_p(dst.ctypes.data), stride, sizes.ctypes.data_as(C.POINTER(C.c_uint64)),
                               int(threads)))
    return [dst[i * stride:i * stride + int(sizes[i])].tobytes() for i in range(n)]
