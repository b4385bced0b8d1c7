"""Tile geometry and the batched GPU tile encoder shared by the streaming / spatial / standard paths.

The reference encodes its units one at a time (``cli.py:553-622``: temp GeoTIFF per tile,
``converter.tiff_to_flac``, mutagen; ``spatial_encoder.py:196-245``: ``_encode_tile_to_flac`` per
tile).  Here every unit of a raster is one window of ONE plan (``fra_plan_*``): per-window
nanmin/nanmax, normalisation, analysis, bit packing and CRCs run as a handful of kernel launches
over all tiles at once.  With several devices, the tiles are split into contiguous runs of
near-equal pixel count (so each device receives only the rows its tiles cover) and the devices
run concurrently from host threads (ctypes releases the GIL); there is no exchange between
devices.  Output is identical for any device count.
"""

from __future__ import annotations

import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native

BLOCKSIZE = 4096  # converter.py:143, spatial_encoder.py:295


def calculate_tiles(height: int, width: int, tile_size: int) -> List[Tuple[int, int, int, int]]:
    """Row-major ``(row_off, col_off, h, w)`` with clipped edge tiles (``spatial_encoder.py:110-121``,
    ``cli.py:553-556``)."""
    if tile_size <= 0:
        raise ValueError("tile_size must be positive")
    return [(r, c, min(tile_size, height - r), min(tile_size, width - c))
            for r in range(0, height, tile_size) for c in range(0, width, tile_size)]


def split_contiguous(weights: Sequence[int], parts: int) -> List[Tuple[int, int]]:
    """Split ``range(len(weights))`` into ``parts`` contiguous runs of near-equal total weight."""
    n = len(weights)
    parts = max(1, min(parts, n)) if n else 1
    total = float(sum(weights))
    out, start, acc = [], 0, 0.0
    for p in range(parts - 1):
        target = total * (p + 1) / parts
        end = start
        while end < n - (parts - 1 - p) and (acc + weights[end] <= target or end == start):
            acc += weights[end]
            end += 1
        out.append((start, end))
        start = end
    out.append((start, n))
    return out


def frames_of(tile: Tuple[int, int, int, int], blocksize: int = 4096) -> int:
    """FLAC frames of one tile's stream."""
    return -(-(tile[2] * tile[3]) // blocksize)


# What holding partial last frames (n < blocksize) costs a rank, in full frames: those subframes run as ONE separate,
# latency-bound k_analyze launch per execute beside the per-wave analysis of the full frames, whatever their number.
# Measured on the C4 8-way split (r06, profiles/r06_shards_partial_cost.txt): the one rank holding the scene's only
# partial frame (the 740^2 corner tile) stepped ~0.012 ms (~6 %, about 240 frames of analysis) slower than the others;
# after FRA-1 3.5b made the frames cheaper the same launch weighs ~500 frames (256 -> 512: slowest 8-way share 0.200 ->
# 0.190 ms, profiles/r06_shards_final.txt).
PARTIAL_FRAME_COST = 512


def frame_split(tiles: Sequence[Tuple[int, int, int, int]], parts: int,
                blocksize: int = 4096, stride: int = 1,
                partial_cost: int = PARTIAL_FRAME_COST) -> List[List[Tuple[int, int, int]]]:
    """Work items of equal cost for ``parts`` ranks ((tile, frame range) items): the frames of all
    tiles in tile order, cut into ``parts`` contiguous runs; part k gets a list of (tile index, first frame, frame
    count) -- whole tiles, plus at most a partial tile at each end.  The frames of one tile, concatenated over the
    parts in order, are that tile's stream.  A part's cost is its frame count, plus ``partial_cost`` if it holds a
    tile's partial last frame (0: equal frame counts); the cuts are refined over a few passes (the parts holding
    partial frames depend on the cuts) and the pass with the smallest largest cost is kept.

    ``stride`` > 1 visits the tiles as i = 0, s, 2s, ..., then 1, 1 + s, ... (tile index mod s first), so each
    part's run samples the whole scene instead of one band of it: content that varies across the scene (a
    no-data corner, water, cloud) spreads over the parts, while the costs stay equal."""
    counts = [frames_of(t, blocksize) for t in tiles]
    order = sorted(range(len(tiles)), key=lambda j: (j % max(1, stride), j))
    total = sum(counts)
    # the global frame index of every partial last frame, in visiting order
    partial_at, pos = [], 0
    for i in order:
        pos += counts[i]
        if (tiles[i][2] * tiles[i][3]) % blocksize:
            partial_at.append(pos - 1)
    # (bounded by a quarter part's frames: no part can be left empty)
    pc = max(0, min(partial_cost, total // (4 * max(1, parts))))

    def cut(holds):  # cuts giving part k a frame count of (total + pc |P|) / parts - pc [k in P]
        t = total + pc * sum(holds)
        c, acc = [0], 0
        for k in range(parts):
            acc += (t * (k + 1) // parts - t * k // parts) - pc * holds[k]
            c.append(min(total, max(c[-1], acc)))
        c[-1] = total
        return c

    def holders(c):
        return [int(any(c[k] <= f < c[k + 1] for f in partial_at)) for k in range(parts)]

    def worst(c):  # the largest part cost of cuts c
        h = holders(c)
        return max(c[k + 1] - c[k] + pc * h[k] for k in range(parts))

    cuts = [total * k // parts for k in range(parts + 1)]
    if pc and partial_at:
        cands = [cuts]
        for _ in range(4):  # a cut next to a partial frame can flip its holder: keep the best of the passes
            cands.append(cut(holders(cands[-1])))
            if cands[-1] == cands[-2]:
                break
        cuts = min(cands, key=worst)
    out: List[List[Tuple[int, int, int]]] = [[] for _ in range(parts)]
    base = 0
    for i in order:
        n = counts[i]
        for k in range(parts):
            a, b = max(base, cuts[k]), min(base + n, cuts[k + 1])
            if b > a:
                out[k].append((i, a - base, b - a))
        base += n
    return out


def lpt_assign(weights: Sequence[int], parts: int) -> List[List[int]]:
    """Longest-processing-time assignment (used when data already lives on every device)."""
    order = sorted(range(len(weights)), key=lambda i: (-weights[i], i))
    loads = [0] * parts
    groups: List[List[int]] = [[] for _ in range(parts)]
    for i in order:
        g = min(range(parts), key=lambda k: (loads[k], k))
        groups[g].append(i)
        loads[g] += weights[i]
    return [sorted(g) for g in groups]


@dataclass
class TileStream:
    """One encoded unit: a complete FLAC stream (86-byte header + frames) + its normalisation.

    ``header`` is the 86-byte libFLAC-layout header, ``body`` the frames -- a zero-copy view into the
    page-locked output of the pipelined encode (``_native.encode_windows_buffer``); ``data`` joins them."""

    header: bytes
    body: object  # bytes-like (memoryview / bytes)
    data_min: float
    data_max: float
    sample_rate: int
    bps: int        # FLAC bits per sample (16, or 32 for int32 audio: SURVEY.md F3)
    channels: int
    nframes: int

    @property
    def data(self) -> bytes:
        return self.header + bytes(self.body)

    def __len__(self) -> int:
        return len(self.header) + len(self.body)

    def __getstate__(self):  # pickling (multi-process gather) materialises the view
        st = dict(self.__dict__)
        st["body"] = bytes(self.body)
        return st


def norm_bits(dtype) -> int:
    """calculate_audio_params' bit depth: 16 for <=16-bit integers, else 24 (int32 audio)."""
    return 16 if np.dtype(dtype) in (np.uint8, np.int8, np.uint16, np.int16) else 24


def mismatch_pixel(window: Tuple[int, int, int, int], first_sample: int, first_channel: int) -> Tuple[int, int, int]:
    """``(row, col, band)`` in raster coordinates of a verify report's first mismatch: ``first_sample`` is the
    window-relative pixel index (row-major over the window's own width, ragged edge tiles included) and
    ``first_channel`` the band; ``window`` is (row_off, col_off, height, width)."""
    return _native.mismatch_pixel(window, first_sample, first_channel)


def _encode_group(raster: np.ndarray, tiles: Sequence[Tuple[int, int, int, int]], level: int, device: int,
                  norm: int, out: list, errors: list, slot: int, rows_ready=None, frame_ranges=None,
                  verify: bool = False, tile0: int = 0):
    r0 = 0
    try:
        r0 = min(t[0] for t in tiles)
        r1 = max(t[0] + t[2] for t in tiles)
        sub = raster[:, r0:r1, :]  # a view: the plan copies only these rows, band by band
        wins = [(t[0] - r0, t[1], t[2], t[3]) for t in tiles]
        if rows_ready is not None and r0 != 0:
            raise ValueError("rows_ready needs the group to start at raster row 0")
        infos, frames = _native.encode_windows_buffer(sub, wins, level=level, blocksize=BLOCKSIZE, norm=norm,
                                                      device=device, rows_ready=rows_ready,
                                                      frame_ranges=frame_ranges, verify=verify)
        out[slot] = streams_from(infos, frames)
    except _native.VerifyMismatch as e:  # from the group's rows and tiles to the raster's
        errors.append(_native.VerifyMismatch(tile0 + e.tile, (e.pixel[0] + r0, e.pixel[1], e.pixel[2]), e.expected,
                                             e.got, e.mismatches, e.bad_tiles))
    except BaseException as e:  # re-raised on the calling thread
        errors.append(e)


def streams_from(infos, frames) -> List[TileStream]:
    """TileStreams over one plan's output: zero-copy views of ``frames`` at each window's offset."""
    res = []
    mv = memoryview(frames)
    for inf in infos:
        hdr = _native.stream_header(inf.channels, inf.bps, inf.sample_rate, BLOCKSIZE)
        res.append(TileStream(hdr, mv[inf.offset:inf.offset + inf.frame_bytes], float(inf.data_min),
                              float(inf.data_max), inf.sample_rate, inf.bps, inf.channels, inf.nframes))
    return res


def encode_tiles_ring(shape, dtype, tiles: Sequence[Tuple[int, int, int, int]], fill, level: int = 5,
                      device: int = 0, step: int = 0, ring_rows: int = 0,
                      verify: bool = False) -> Tuple[List[TileStream], int]:
    """:func:`encode_tiles` for a raster that is produced row band by row band and never held whole
    (``_native.encode_windows_ring``): ``fill(dst, r0, r1)`` writes image rows ``[r0, r1)`` of every band
    into ``dst``.  The reference reads each tile's window the same way (``cli.py:553-559``).  ``verify``: as
    :func:`encode_tiles`.  Returns the streams and the ring's height in rows."""
    if not tiles:
        return [], 0
    infos, frames, R = _native.encode_windows_ring(shape, dtype, tiles, fill, level=level, blocksize=BLOCKSIZE,
                                                   norm=norm_bits(dtype), device=device, step=step,
                                                   ring_rows=ring_rows, verify=verify)
    return streams_from(infos, frames), R


def encode_tiles(raster: np.ndarray, tiles: Sequence[Tuple[int, int, int, int]], level: int = 5,
                 devices: Optional[Sequence[int]] = None, rows_ready=None,
                 producer: Optional[threading.Thread] = None, frame_ranges=None,
                 verify: bool = False) -> List[TileStream]:
    """Encode every tile of a band-planar ``(B, H, W)`` raster as its own FLAC stream on the GPU(s).

    Each stream equals what ``normalize_to_audio`` + ``pyflac.StreamEncoder(blocksize=4096)``
    produce for ``raster[:, r:r+h, c:c+w]`` interleaved pixel-major (``cli.py:557-597``).
    ``rows_ready`` / ``producer``: the raster is still being decoded by ``producer``, which publishes the
    rows done in ``rows_ready[0]``; one device encodes as the rows land, several wait for the producer.
    ``frame_ranges``: (first frame, count) per tile -- only those frames of each stream (one device; the
    multi-GPU work items of ``frame_split``); the TileStream's body then holds just those frames.
    ``verify``: libFLAC's verify mode -- every plan's frames are decoded on its GPU and compared with its copy of the
    raster, normalised anew, before the plan is closed (``_native.Plan.verify``); a difference raises
    ``_native.VerifyMismatch`` with the tile, the pixel and both samples, a frame that does not decode ``NativeError``.
    """
    a = np.asarray(raster)
    if a.ndim == 2:
        a = a[None]
    if not a.dtype.isnative:
        a = a.astype(a.dtype.newbyteorder("="))
    if a.dtype not in _native.DTYPE_CODES:
        raise TypeError(f"unsupported raster dtype {a.dtype}")
    if not tiles:
        return []
    devs = list(devices) if devices else [0]
    norm = norm_bits(a.dtype)
    runs = split_contiguous([t[2] * t[3] for t in tiles], len(devs))
    out: list = [None] * len(runs)
    errors: list = []
    if rows_ready is not None and (len(runs) > 1 or min(t[0] for t in tiles) != 0):
        if producer is not None:
            producer.join()
        if rows_ready[0] < 0:
            raise RuntimeError("raster decode failed")
        rows_ready = None
    if frame_ranges is not None:
        if len(devs) != 1:
            raise ValueError("frame_ranges: one device per call (one rank per GPU)")
        _encode_group(a, tiles, level, devs[0], norm, out, errors, 0, rows_ready, frame_ranges, verify)
    elif len(runs) == 1:
        _encode_group(a, tiles, level, devs[0], norm, out, errors, 0, rows_ready, None, verify)
    else:
        th = [threading.Thread(target=_encode_group,
                               args=(a, tiles[s:e], level, devs[k], norm, out, errors, k, None, None, verify, s))
              for k, (s, e) in enumerate(runs)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    if errors:
        raise errors[0]
    return [ts for grp in out for ts in grp]


def _plan_items(plan: "_native.Plan"):
    """An executed plan's device output as ``decode_device`` input: (stream infos, (pointer, length), one item per
    window addressed through the plan's frame offsets)."""
    infos, total = plan.result()
    nfr = sum(i.nframes for i in infos)
    off = plan.frame_offsets(nfr)
    ptr, _ = plan.device_output()
    items, f0 = [], 0
    for inf, w in zip(infos, plan.windows):
        fo = off[f0:f0 + inf.nframes + 1] - np.uint64(inf.offset)
        items.append({"offset": inf.offset, "bytes": inf.frame_bytes, "window": w, "frame_offsets": fo,
                      "channels": inf.channels, "bps": inf.bps, "blocksize": plan.blocksize})
        f0 += inf.nframes
    return infos, (ptr, total), items


def verify_on_device(plan: "_native.Plan", raster_ptr: int,
                     strides: Optional[Tuple[int, int, int]] = None) -> bool:
    """Decode an executed plan's device output on its GPU into ``raster_ptr`` (a device buffer of int16 for 16-bps
    plans / int32 otherwise, laid out like the plan's raster, or with other element ``strides``) without copying the
    frames to the host: the frames are addressed through ``fra_plan_frame_offsets``, nothing is searched.  Returns True
    when every frame parsed with a matching CRC-16 (a corrupt frame raises ``NativeError``).  The library offers the
    decode; comparing the samples with the expectation stays with the caller -- or with ``Plan.verify``
    (``fra_plan_verify``), which decodes the same way and compares on the GPU with the plan's own raster, without a
    destination buffer."""
    infos, data, items = _plan_items(plan)
    if not items:
        return True
    dt = np.int16 if all(i.bps <= 16 for i in infos) else np.int32
    out = plan.ctx.decode_device(data, items, int(raster_ptr), dt, infos[0].channels,
                                 strides or plan.strides)
    return all(o.nframes == i.nframes for o, i in zip(out, infos))


def read_window_on_device(plan: "_native.Plan", window: Tuple[int, int, int, int], raster_ptr: int,
                          strides: Optional[Tuple[int, int, int]] = None, decimate: int = 1,
                          resampling: str = "nearest", out_shape: Optional[Tuple[int, int]] = None, nodata=None,
                          filled=None):
    """The windowed counterpart of :func:`verify_on_device`: decode the pixels ``window`` (row_off, col_off, height,
    width, in the plan's raster coordinates) of an executed plan's device output into ``raster_ptr``, a device buffer
    of int16 (16-bps plans) / int32 whose element 0 is the window's first pixel (default ``strides``: band-planar
    ``(height * width, width, 1)`` of the window).  Only the frames that hold samples of the window are parsed,
    through ``fra_plan_frame_offsets``; nothing is searched and nothing is copied to the host.  Returns the per-tile
    :class:`Decoded` infos (0 frames for a tile outside the window); a corrupt selected frame raises ``NativeError``.

    ``decimate`` = 2 .. 64: the window at that fraction of the resolution (``resample.decimate`` of the above with
    ``resampling``, ``fra_decode_device_decimated``); ``raster_ptr`` and the default ``strides`` then address the
    ``resample.decimated_shape(height, width, decimate)`` output, and the plan's tiles must cover the window.

    ``out_shape`` = (oh, ow), not together with ``decimate``: the window resampled to that size
    (``resample.resample`` with ``resampling``, any of its four; ``fra_decode_device_resampled``); ``raster_ptr`` and
    the default ``strides`` then address the ``(oh, ow)`` output.

    ``nodata`` (with ``decimate`` or ``out_shape``): the nodata-aware rule of ``resample`` in the decoded samples'
    dtype (the ``_masked`` entries); ``filled``: an optional ``uint64`` array of one word per channel that receives the
    number of output pixels no valid pixel reached."""
    if out_shape is not None and decimate != 1:
        raise ValueError("give decimate or out_shape, not both")
    if out_shape is None and decimate == 1 and (nodata is not None or filled is not None):
        raise ValueError("nodata needs decimate or out_shape")
    infos, data, items = _plan_items(plan)
    if not items:
        return []
    _, _, h, w = (int(v) for v in window)
    dt = np.int16 if all(i.bps <= 16 for i in infos) else np.int32
    if out_shape is not None:
        from .resample import check_out_shape

        oh, ow = check_out_shape(out_shape)
        return plan.ctx.decode_device_resampled(data, items, int(raster_ptr), dt, infos[0].channels,
                                                strides or (oh * ow, ow, 1), window, (oh, ow), resampling,
                                                nodata=nodata, filled=filled)
    if decimate != 1:
        from .resample import decimated_shape

        oh, ow = decimated_shape(h, w, decimate)
        return plan.ctx.decode_device_decimated(data, items, int(raster_ptr), dt, infos[0].channels,
                                                strides or (oh * ow, ow, 1), window, decimate, resampling,
                                                nodata=nodata, filled=filled)
    return plan.ctx.decode_device_window(data, items, int(raster_ptr), dt, infos[0].channels,
                                         strides or (h * w, w, 1), window)
