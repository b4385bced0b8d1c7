"""``--streaming`` container: ``[u32 BE index length][compact JSON index][tile FLAC streams]``.

Writer = ``cli._create_streaming_flac`` (``cli.py:521-639``), the north-star path: per tile the
reference writes a temp GeoTIFF, runs ``tiff_to_flac`` on it (normalise, pyflac, mutagen tags of
the TILE: its size, transform, bounds, min/max) and appends the bytes.  Here all tiles are encoded
by one batched GPU plan per device (``tiles.encode_tiles``), and the per-tile tag rewrite is the
same host byte assembly (``flac_meta``) with the values the temp GeoTIFF would have carried:
the window transform (rasterio ``windows.transform`` arithmetic), no nodata, the source CRS.

Reader = the index parse + byte-range slicing of ``cli.extract`` (``cli.py:238-313``); ``streaming_to_raster`` decodes
the whole container, ``read_window`` a pixel window of it (only the byte ranges of the tiles it intersects are read,
and on the GPU only the frames that hold its rows are decoded), at full resolution, decimated by 2 .. 64
(``decimate=``) or resampled to any size (``out_shape=``), and ``read_overview`` the whole raster decimated or resampled
(``resample`` states the rules).

Every windowed operation below is written once over a source (``source``: a container or a GeoTIFF behind one surface);
the public ``X_window`` / ``X_tiff`` / ``X_to_tiff`` functions pick the source and shape the return tuple.
"""

from __future__ import annotations

import json
import struct
import threading
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import flac_meta, resample
from .converter import raster_metadata, raster_tags
from .geo import Affine, window_transform
from .source import ContainerSource, TiffSource, _decode_window_on_host, denorm_code, normal_crs, open_source
from .tiff import GeoTIFF
from .tiles import TileStream, calculate_tiles, encode_tiles, encode_tiles_ring


def tile_flac_parts(ts: TileStream, transform: Affine, crs: Optional[str], row_off: int, col_off: int, height: int,
                    width: int, dtype):
    """One tile's file as ``converter.tiff_to_flac(temp_tile.tif)`` would write it, as (tagged metadata
    bytes, frames view, window transform): the frames are not copied."""
    tt = window_transform(transform, col_off, row_off)
    md = raster_metadata(width, height, ts.channels, dtype, crs, tt, ts.data_min, ts.data_max, None,
                         32767 if ts.bps == 16 else 8388607)
    return flac_meta.rewrite_header_parts(ts.header, len(ts.body), raster_tags(md)), ts.body, tt


def tile_flac_bytes(ts: TileStream, transform: Affine, crs: Optional[str], row_off: int, col_off: int, height: int,
                    width: int, dtype) -> Tuple[bytes, Affine]:
    head, body, tt = tile_flac_parts(ts, transform, crs, row_off, col_off, height, width, dtype)
    return head + bytes(body), tt


def streaming_parts(tiles: Sequence[Tuple[int, int, int, int]], streams: Sequence[TileStream], shape, dtype,
                    transform: Affine, crs: Optional[str], tile_size: int) -> List:
    """The container as a list of bytes-like parts (index first); frames stay zero-copy views."""
    B, H, W = shape
    index: Dict = {"crs": str(crs), "transform": list(transform), "width": W, "height": H, "bands": B,
                   "dtype": str(np.dtype(dtype)), "tile_size": tile_size, "frames": []}
    parts: List = []
    total = 0
    for fid, ((r, c, h, w), ts) in enumerate(zip(tiles, streams)):
        head, body, tt = tile_flac_parts(ts, transform, crs, r, c, h, w, dtype)
        size = len(head) + len(body)
        xmin, ymax = tt.c, tt.f
        index["frames"].append({
            "frame_id": fid,
            "bbox": [xmin, ymax + h * tt.e, xmin + w * tt.a, ymax],
            "window": {"col_off": c, "row_off": r, "width": w, "height": h},
            "byte_offset": total,
            "byte_size": size,
        })
        parts += [head, body]
        total += size
    head = json.dumps(index, separators=(",", ":")).encode("utf-8")
    return [len(head).to_bytes(4, "big") + head] + parts


def assemble_streaming(tiles: Sequence[Tuple[int, int, int, int]], streams: Sequence[TileStream], shape,
                       dtype, transform: Affine, crs: Optional[str], tile_size: int) -> bytes:
    """Container bytes from encoded tile streams (tile order = ``calculate_tiles`` order)."""
    return b"".join(bytes(p) if isinstance(p, memoryview) else p
                    for p in streaming_parts(tiles, streams, shape, dtype, transform, crs, tile_size))


def build_streaming(raster: np.ndarray, transform: Affine, crs: Optional[str], tile_size: int,
                    compression_level: int = 5, devices: Optional[Sequence[int]] = None,
                    verify: bool = False) -> bytes:
    """Container bytes for a band-planar ``(B, H, W)`` raster (all tiles on the GPU(s)); ``verify`` as
    ``tiles.encode_tiles``."""
    a = raster if raster.ndim == 3 else raster[None]
    tiles = calculate_tiles(a.shape[1], a.shape[2], tile_size)
    streams = encode_tiles(a, tiles, compression_level, devices, verify=verify)
    return assemble_streaming(tiles, streams, a.shape, a.dtype, transform, crs, tile_size)


def decode_while_encoding(g: GeoTIFF, tile_size: int):
    """Start decoding a GeoTIFF into page-locked memory on a producer thread, top to bottom in row bands
    (one tile row, rounded up to whole TIFF strips/tiles): returns ``(raster, rows_ready, thread)``;
    ``rows_ready[0]`` = rows decoded so far (-1 on failure).  The encoder's host pipeline copies a band
    H2D as soon as its rows are published (``fra_plan_encode_host_progress``), so the decode of band b+1
    overlaps the PCIe copies and kernels of band b."""
    from .tiff import _alloc

    info = g.info
    raster = _alloc((info.count, info.height, info.width), info.dtype, True)
    rows_ready = np.zeros(1, np.int64)
    step = decode_step(g, tile_size)
    errors: list = []

    def run():
        try:
            for r0 in range(0, info.height, step):
                r1 = min(info.height, r0 + step)
                g.read_window_into(raster[:, r0:r1, :], r0, 0, r1 - r0, info.width)
                rows_ready[0] = r1
        except BaseException as e:  # reported to the encoder (rows_ready = -1) and re-raised by the caller
            errors.append(e)
            rows_ready[0] = -1

    th = threading.Thread(target=run, name="geotiff-decode", daemon=True)
    th.errors = errors  # type: ignore[attr-defined]
    th.start()
    return raster, rows_ready, th


def decode_step(g: GeoTIFF, tile_size: int) -> int:
    """Rows per producer step: one tile row, rounded up to whole TIFF strips / tiles."""
    info = g.info
    step = max(tile_size, g.ch)
    return ((step + g.ch - 1) // g.ch) * g.ch if g.ch < info.height else info.height


def encode_geotiff_ring(g: GeoTIFF, tiles, compression_level: int = 5, device: int = 0, tile_size: int = 512,
                        ring_rows: int = 0, verify: bool = False):
    """GeoTIFF -> tile streams with bounded host memory: the file's row bands are decoded into a
    page-locked ring (``tiles.encode_tiles_ring``) that the pipelined encoder copies from and recycles, so
    the raster is never held whole -- as the reference, which reads one tile window at a time
    (``cli.py:553-559``).  Returns ``(streams, ring_rows)``."""
    info = g.info

    def fill(dst, r0, r1):
        g.read_window_into(dst, r0, 0, r1 - r0, info.width)

    return encode_tiles_ring((info.count, info.height, info.width), info.dtype, tiles, fill, compression_level,
                             device, step=decode_step(g, tile_size), ring_rows=ring_rows, verify=verify)


def encode_geotiff_streaming(input_path: Path, tile_size: int = 512, compression_level: int = 5,
                             devices: Optional[Sequence[int]] = None, ring: bool = True, verify: bool = False):
    """GeoTIFF file -> (tiles, streams, raster info): decode and encode overlapped.  One device: through
    the bounded ring (``encode_geotiff_ring``); several: the whole raster is decoded into page-locked
    memory (``decode_while_encoding``) and split over the devices."""
    g = GeoTIFF(input_path)
    if ring and (not devices or len(devices) == 1):
        try:
            info = g.info
            tiles = calculate_tiles(info.height, info.width, tile_size)
            streams, _ = encode_geotiff_ring(g, tiles, compression_level, devices[0] if devices else 0, tile_size,
                                             verify=verify)
            return tiles, streams, (info.count, info.height, info.width), np.dtype(info.dtype), info
        finally:
            g.close()
    raster, rows_ready, th = decode_while_encoding(g, tile_size)
    try:
        tiles = calculate_tiles(raster.shape[1], raster.shape[2], tile_size)
        try:
            streams = encode_tiles(raster, tiles, compression_level, devices, rows_ready=rows_ready, producer=th,
                                   verify=verify)
        finally:
            th.join()
        if th.errors:  # type: ignore[attr-defined]
            raise th.errors[0]  # type: ignore[attr-defined]
        return tiles, streams, raster.shape, raster.dtype, g.info
    finally:
        g.close()


def create_streaming_flac(input_path: Path, output_path: Path, tile_size: int = 512, compression_level: int = 5,
                          devices: Optional[Sequence[int]] = None, verify: bool = False) -> Dict:
    """Write the streaming container for a GeoTIFF; returns the index.

    The raster is decoded into page-locked memory by a producer thread, row band by row band, while the
    pipelined host path encodes the bands already decoded (H2D, kernels and D2H of band b overlap the
    decode of band b+1); the container is written from zero-copy views of the page-locked frames.  ``verify``:
    every plan's frames are decoded on the GPU and compared with the raster before anything is written
    (``tiles.encode_tiles``; raises ``VerifyMismatch``)."""
    tiles, streams, shape, dtype, info = encode_geotiff_streaming(input_path, tile_size, compression_level, devices,
                                                                  verify=verify)
    parts = streaming_parts(tiles, streams, shape, dtype, Affine(*info.transform), info.crs, tile_size)
    with open(output_path, "wb") as f:
        for p in parts:
            f.write(p)
    n = struct.unpack(">I", parts[0][:4])[0]
    return json.loads(parts[0][4:4 + n].decode("utf-8"))


@dataclass
class StreamingFile:
    """Parsed container: index + absolute byte range of every tile."""

    index: Dict
    header_size: int

    def tile_range(self, frame: Dict) -> Tuple[int, int]:
        start = self.header_size + frame["byte_offset"]
        return start, start + frame["byte_size"]


def read_index_bytes(data: bytes) -> Tuple[Dict, int]:
    n = struct.unpack(">I", data[:4])[0]
    return json.loads(data[4:4 + n].decode("utf-8")), 4 + n


def open_streaming(path: Path) -> StreamingFile:
    with open(path, "rb") as f:
        n = struct.unpack(">I", f.read(4))[0]
        idx = json.loads(f.read(n).decode("utf-8"))
    return StreamingFile(idx, 4 + n)


def select_frame(frames: List[Dict], tile_id: Optional[int] = None, bbox: Optional[Sequence[float]] = None,
                 center: bool = False, last: bool = False) -> Dict:
    """Tile choice of ``cli.extract`` (``cli.py:245-296``)."""
    if tile_id is not None:
        fr = next((f for f in frames if f["frame_id"] == tile_id), None)
        if fr is None:
            raise KeyError(f"Tile ID {tile_id} not found")
        return fr
    if last:
        return max(frames, key=lambda f: f["frame_id"])
    if center:
        boxes = [f["bbox"] for f in frames]
        cx = (min(b[0] for b in boxes) + max(b[2] for b in boxes)) / 2
        cy = (min(b[1] for b in boxes) + max(b[3] for b in boxes)) / 2
        return min(frames, key=lambda f: ((f["bbox"][0] + f["bbox"][2]) / 2 - cx) ** 2
                   + ((f["bbox"][1] + f["bbox"][3]) / 2 - cy) ** 2)
    if bbox is not None:
        if len(bbox) != 4:
            raise ValueError("Bbox must have 4 coordinates")
        hit = [f for f in frames if bbox[0] < f["bbox"][2] and bbox[2] > f["bbox"][0] and bbox[1] < f["bbox"][3]
               and bbox[3] > f["bbox"][1]]
        if not hit:
            raise LookupError("No tiles intersect bbox")
        return hit[0]
    raise ValueError("Specify tile_id, bbox, center or last")


def read_tile_bytes(path: Path, frame: Dict, header_size: int) -> bytes:
    with open(path, "rb") as f:
        f.seek(header_size + frame["byte_offset"])
        return f.read(frame["byte_size"])


# ------------------------------------------------------------------------------------------ container -> raster
def is_streaming_container(path: Path) -> bool:
    """A ``.flac`` file that starts with neither ``fLaC`` nor an ID3v2 tag: the ``--streaming`` container."""
    with open(path, "rb") as f:
        head = f.read(4)
    return head[:4] != b"fLaC" and head[:3] != b"ID3"


def _tile_items(data: bytes):
    """The index and, per tile, the ``decode_device`` item: byte range, window and the tile's own min / max tags."""
    s = ContainerSource(data)
    return s.meta, s.whole()[1]


def _to_raster(s: ContainerSource, device: Optional[int], semantics: str):
    """:func:`streaming_to_raster` of a source."""
    from . import _native

    denorm = denorm_code(semantics)
    data, items = s.whole()  # to the device as they are
    H, W = s.height, s.width
    out = np.zeros((s.bands, H, W), dtype=s.dtype)
    if device is not None:
        ctx = _native.default_context(int(device))
        ctx.decode_device(np.frombuffer(data, dtype=np.uint8), items, out, s.dtype, s.bands, (H * W, W, 1), denorm)
    else:
        _decode_window_on_host(data, items, s.window(), out, semantics)
    return out, s.meta


def streaming_to_raster(src, device: Optional[int] = None, semantics: str = "pcm16"):
    """Streaming container (path or bytes) -> ``(raster (B, H, W) in the index's dtype, index)``.

    Every tile is denormalised with its own ``GEOSPATIAL_DATA_MIN`` / ``_MAX`` tags into its window of the index.
    ``semantics="pcm16"`` gives what ``flac_to_tiff`` / ``extract`` give per tile (PCM_16 floats),
    ``"int"`` denormalises the exact integer samples.  ``device=None`` is the host implementation (``fra_decode`` per
    tile + ``denormalize_from_audio``, no GPU needed); an integer runs one ``fra_decode_device`` call over all tiles
    on that GPU."""
    return _to_raster(ContainerSource(src), device, semantics)


def _to_tiff(tiff_path: Path, raster: np.ndarray, s, win=None, transform=None, crs=None, nodata=None):
    """A result raster of the source ``s`` -> GeoTIFF with the source's CRS (``crs``: the grid's, after a warp), the
    transform at the origin of the window ``win`` (``transform``: the one of a read that resampled or warped) and
    ``nodata`` as its nodata tag."""
    from .tiff import write_geotiff

    write_geotiff(Path(tiff_path), raster, transform=s.window_transform(win) if transform is None else transform,
                  crs=s.crs if crs is None else normal_crs(crs), nodata=nodata)


def _fill_tag(fill, dtype):
    """A fill as the output dtype holds it (``calc.convert``), as a GeoTIFF nodata tag."""
    from .calc import convert

    v = convert(np.array([float(fill)]), dtype)[0]
    return float(v) if np.dtype(dtype).kind == "f" else int(v)


def _nodata(s, nodata):
    """``nodata=None`` takes the source's own nodata tag, when it has one."""
    return s.nodata if nodata is None else nodata


def streaming_to_tiff(path: Path, tiff_path: Path, device: Optional[int] = None) -> Dict:
    """Streaming container -> GeoTIFF with the index's transform and CRS (``flac_to_tiff`` semantics per tile);
    returns the index."""
    s = ContainerSource(Path(path))
    raster, index = _to_raster(s, device, "pcm16")
    _to_tiff(tiff_path, raster, s, transform=s.transform)
    return index


# ------------------------------------------------------------------------------------------ container -> window
def resolve_window(index: Dict, window: Optional[Sequence[int]] = None,
                   bbox: Optional[Sequence[float]] = None) -> Tuple[int, int, int, int]:
    """The pixel window ``(row_off, col_off, height, width)`` of a request, clipped to the index's raster.

    ``bbox`` = (xmin, ymin, xmax, ymax) in the index's CRS goes through the index's transform: floor of the minimum
    pixel edge, ceil of the maximum.  A transform with rotation terms raises ``ValueError``, an empty result
    ``LookupError``."""
    if (window is None) == (bbox is None):
        raise ValueError("Specify exactly one of window and bbox")
    H, W = int(index["height"]), int(index["width"])
    if bbox is not None:
        if len(bbox) != 4:
            raise ValueError("Bbox must have 4 coordinates")
        t = index.get("transform")
        if not t:
            raise ValueError("the index has no transform")
        a, b, c, d, e, f = (float(v) for v in t[:6])
        if b != 0.0 or d != 0.0 or a == 0.0 or e == 0.0:
            raise ValueError("a bbox needs an axis-aligned transform (no rotation terms)")
        cols = sorted(((float(bbox[0]) - c) / a, (float(bbox[2]) - c) / a))
        rows = sorted(((float(bbox[1]) - f) / e, (float(bbox[3]) - f) / e))
        r0, r1 = int(np.floor(rows[0])), int(np.ceil(rows[1]))
        c0, c1 = int(np.floor(cols[0])), int(np.ceil(cols[1]))
    else:
        if len(window) != 4:
            raise ValueError("Window must be (row_off, col_off, height, width)")
        r0, c0, h, w = (int(v) for v in window)
        r1, c1 = r0 + h, c0 + w
    r0, c0, r1, c1 = max(r0, 0), max(c0, 0), min(r1, H), min(c1, W)
    if r1 <= r0 or c1 <= c0:
        raise LookupError("The window does not intersect the raster")
    return r0, c0, r1 - r0, c1 - c0


def _read_window(s: ContainerSource, window, bbox, device, semantics, decimate, resampling, out_shape, nodata):
    """:func:`read_window` of a source."""
    from . import _native

    k = 1
    if out_shape is not None:
        if decimate != 1:
            raise ValueError("give decimate or out_shape, not both")
        out_shape = resample.check_out_shape(out_shape)
        resample.resampling_any_code(resampling)
    elif decimate != 1:
        k = resample.check_factor(decimate)
        resample.resampling_code(resampling)
    win = resolve_window(s.meta, window, bbox)  # a read names its window: no whole-raster default here
    reg = s.region(win, semantics)
    index, dt, B = s.meta, s.dtype, s.bands
    h, w = win[2], win[3]
    if nodata is not None:
        if out_shape is None and k == 1:
            raise ValueError("nodata needs decimate or out_shape")
        nodata = resample.check_nodata(nodata, dt)
    if device is None:
        out = reg.host()
        if out_shape is not None:
            out = resample.resample(out, out_shape, resampling, nodata)
        elif k > 1:
            out = resample.decimate(out, k, resampling, nodata)
        return out, win, index
    ctx = _native.default_context(int(device))
    data, items = reg.decode_args()[:2]
    if out_shape is not None:
        oh, ow = out_shape
        out = np.zeros((B, oh, ow), dtype=dt)
        ctx.decode_device_resampled(data, items, out, dt, B, (oh * ow, ow, 1), win, out_shape, resampling, reg.denorm,
                                    nodata=nodata)
    elif k > 1:
        oh, ow = resample.decimated_shape(h, w, k)
        out = np.zeros((B, oh, ow), dtype=dt)
        ctx.decode_device_decimated(data, items, out, dt, B, (oh * ow, ow, 1), win, k, resampling, reg.denorm,
                                    nodata=nodata)
    else:
        out = np.zeros((B, h, w), dtype=dt)
        ctx.decode_device_window(data, items, out, dt, B, (h * w, w, 1), win, reg.denorm)
    return out, win, index


def read_window(src, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                device: Optional[int] = None, semantics: str = "pcm16", decimate: int = 1,
                resampling: str = "nearest", out_shape: Optional[Sequence[int]] = None, nodata=None):
    """A pixel window of a streaming container (path or bytes) -> ``(raster (B, h, w) in the index's dtype, window,
    index)``, bit-identical to cropping :func:`streaming_to_raster`.

    ``decimate`` = 2, 4, 8, 16, 32 or 64 returns the window at that fraction of the resolution instead:
    ``resample.decimate(window's raster, decimate, resampling)``, shape ``(B, ceil(h / k), ceil(w / k))``; the returned
    window is still the clipped full-resolution one (``resample.decimated_transform`` gives the result's transform).
    On the host the window is read as below and decimated with numpy; on a GPU one ``fra_decode_device_decimated``
    call decodes and decimates it there and only the small result comes back.

    ``out_shape`` = (oh, ow), not together with ``decimate``: the window resampled to that size, larger or smaller,
    ``resample.resample(window's raster, out_shape, resampling)`` with ``resampling`` one of ``nearest``, ``average``,
    ``bilinear``, ``cubic`` (``resample.resampled_transform`` gives the result's transform).  On the host the window
    is read and resampled with numpy; on a GPU one ``fra_decode_device_resampled`` call does both there.

    ``nodata`` (with ``decimate`` or ``out_shape``): the nodata-aware rule of ``resample``: pixels of that value, and
    NaN, are left out of every result, and an output no valid pixel reaches holds the value.  The container stores no
    nodata value, so it is always the caller's; ``None`` is the unmasked read.  On a GPU the ``_masked`` entries.

    ``window`` = (row_off, col_off, height, width) or ``bbox`` = (xmin, ymin, xmax, ymax), see :func:`resolve_window`;
    the returned window is the clipped one.  Of a file only the index and the byte ranges of the intersecting tiles
    are read (seek + read).  ``device=None`` decodes those tiles on the host and crops; an integer makes one
    ``fra_decode_device_window`` call on that GPU, which decodes only the frames that hold the window's rows."""
    return _read_window(ContainerSource(src), window, bbox, device, semantics, decimate, resampling, out_shape, nodata)


def _window_items(src, window, bbox):
    """The index of a container (path or bytes), the clipped window of a request, and the bytes and ``decode_device``
    items of the tiles that intersect it (of a file only the index and those byte ranges are read)."""
    s = ContainerSource(src)
    reg = s.region(resolve_window(s.meta, window, bbox))
    return s.meta, reg.win, reg.blob, reg.items


# ------------------------------------------------------------------------------------------ container against raster
def _compare_window(reg, ref: np.ndarray, device: Optional[int], count_one_sided_nans: bool = False) -> Dict:
    """The region ``reg`` of a container against ``ref`` (B, h, w): on the host the window is decoded and compared with
    numpy; on a GPU one ``fra_decode_device_compare`` call returns the reports."""
    from . import _native
    from .compare import compare_arrays, report_from_bands

    r, c, h, w = reg.win
    if device is None:
        report = compare_arrays(reg.host(), ref)
    else:
        ctx = _native.default_context(int(device))
        data, items, dt, B, win = reg.decode_args()
        bands, _ = ctx.decode_device_compare(data, items, ref, dt, B, win, reg.denorm)
        report = report_from_bands(bands, dt)
        if count_one_sided_nans and report["one_sided_nan"] is None:
            out = np.zeros((B, h, w), dtype=dt)
            ctx.decode_device_window(data, items, out, dt, B, (h * w, w, 1), win, reg.denorm)
            for i, band in enumerate(report["bands"]):
                band["one_sided_nan"] = int(np.count_nonzero(np.isnan(out[i]) != np.isnan(ref[i])))
            report["one_sided_nan"] = sum(band["one_sided_nan"] for band in report["bands"])
    report["origin"] = [r, c]
    return report


def compare_with_raster(src, raster: np.ndarray, window: Optional[Sequence[int]] = None,
                        bbox: Optional[Sequence[float]] = None, device: Optional[int] = None,
                        semantics: str = "pcm16"):
    """Does this container (path or bytes) give ``raster`` back, and if not, by how much -> ``(report, window,
    index)``: ``compare.compare_arrays(read_window(src, ...)[0], raster cropped to the window)``, the container's
    pixels being ``file1`` / ``a`` and the raster's ``file2`` / ``b``.

    ``raster`` is the whole source raster ``(B, H, W)`` of the index's dtype and shape (``ValueError`` otherwise);
    ``window`` / ``bbox`` restrict the comparison as in :func:`read_window` (default: the whole raster); the positions
    in the report are relative to the returned (clipped) window, whose origin is ``report["origin"]``.
    ``device=None`` reads the window on the host and compares with numpy; an integer makes one
    ``fra_decode_device_compare`` call on that GPU: the decoded pixels never leave the device, the raster's window goes
    there, and only the reports come back (``one_sided_nan`` is then ``None`` where a band has both unordered and
    differing pixels, see ``compare.report_from_bands``)."""
    s = ContainerSource(src)
    win = s.window(window, bbox)
    reg = s.region(win, semantics)
    shape, dt = (s.bands, s.height, s.width), s.dtype
    raster = np.asarray(raster)
    if raster.shape != shape or raster.dtype != dt:
        raise ValueError(f"the raster must be {shape} of {dt} as the container's index says, got {raster.shape} of "
                         f"{raster.dtype}")
    r, c, h, w = win
    ref = raster[:, r:r + h, c:c + w]
    if any(st < 0 or st % dt.itemsize for st in ref.strides) or not ref.dtype.isnative:
        ref = np.ascontiguousarray(ref, dtype=dt.newbyteorder("="))
    return _compare_window(reg, ref, device), win, s.meta


def check_against_tiff(container: Path, tiff: Path, window: Optional[Sequence[int]] = None,
                       bbox: Optional[Sequence[float]] = None, device: Optional[int] = None,
                       semantics: str = "pcm16", count_one_sided_nans: bool = False):
    """:func:`compare_with_raster` of a streaming container against the GeoTIFF it was made from -> ``(report, window,
    index)``; the report also carries what ``compare.display_comparison_table`` prints (names, shapes, dtypes, CRS).
    With a window only that window of the TIFF is read (in-package reader).  A TIFF whose shape or dtype is not the
    index's raises ``ValueError``.

    ``count_one_sided_nans``: a GPU report leaves ``one_sided_nan`` open (``None``) when a band has both unordered and
    differing pixels; the window is then read once more (``fra_decode_device_window``) and the pixels with a NaN on
    one side only are counted on the host.  The host path always counts them."""
    container, tiff = Path(container), Path(tiff)
    s, t = ContainerSource(container), TiffSource(tiff)
    shape, tshape = (s.bands, s.height, s.width), (t.bands, t.height, t.width)
    if tshape != shape or t.dtype != s.dtype:
        raise ValueError(f"{tiff.name} is {tshape} of {t.dtype}, the container holds {shape} of {s.dtype}")
    win = s.window(window, bbox)
    reg = s.region(win, semantics)
    report = _compare_window(reg, t.region(win).host(), device, count_one_sided_nans)
    crs, tcrs = str(s.meta.get("crs")), str(t.meta.crs)  # as they are stored, "None" for none
    report.update({
        "file1": container.name, "file2": tiff.name, "shape_match": True, "dtype_match": True,
        "crs_match": crs == tcrs, "file1_shape": shape, "file2_shape": tshape,
        "file1_dtype": str(s.dtype), "file2_dtype": str(t.dtype), "file1_crs": crs, "file2_crs": tcrs,
        "window": list(win), "semantics": semantics,
    })
    return report, win, s.meta


# ------------------------------------------------------------------------------------------ statistics
def _stats(s, window, bbox, bins, hist_range, nodata, device, semantics=None):
    """Band statistics of a source -> ``(report, window)``."""
    from . import _native
    from .stats import check_options, report_from_bands, stats_arrays

    check_options(bins, hist_range, nodata)
    win = s.window(window, bbox)
    nodata = _nodata(s, nodata)
    reg = s.region(win, semantics)
    if device is None:
        return stats_arrays(reg.host(), bins, hist_range, nodata), win
    ctx = _native.default_context(int(device))
    if reg.encoded:
        bands, hist, _ = ctx.decode_device_stats(*reg.decode_args(), reg.denorm, bins, hist_range, nodata)
    else:
        bands, hist = ctx.stats(reg.host(), bins, hist_range, nodata)
    return report_from_bands(bands, hist, s.dtype), win


def container_stats(src, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                    bins: int = 0, hist_range=None, nodata: Optional[float] = None, device: Optional[int] = None,
                    semantics: str = "pcm16"):
    """Band statistics and histograms of a streaming container (path or bytes), or of a window of it -> ``(report,
    window, index)``: ``stats.stats_arrays(read_window(src, ...)[0], bins, hist_range, nodata)``, one dict per band.

    ``window`` / ``bbox`` as in :func:`read_window` (default: the whole raster); ``bins``, ``hist_range`` (``(lo, hi)``,
    ``"auto"`` / ``None``) and ``nodata`` as ``stats.stats_arrays``.  ``device=None`` reads the window on the host and
    applies the numpy rule; an integer makes one ``fra_decode_device_stats`` call on that GPU: the decoded pixels never
    leave the device and only the reports and the histogram come back."""
    s = ContainerSource(src)
    return _stats(s, window, bbox, bins, hist_range, nodata, device, semantics) + (s.meta,)


def tiff_stats(path: Path, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
               bins: int = 0, hist_range=None, nodata: Optional[float] = None, device: Optional[int] = None):
    """Band statistics and histograms of a GeoTIFF, or of a window of it -> ``(report, window, info)``.  The window is
    read with the in-package reader; an integer ``device`` hands it to ``fra_stats`` on that GPU, ``None`` to the numpy
    rule.  ``nodata=None`` takes the TIFF's own nodata tag, when it has one."""
    s = TiffSource(path)
    return _stats(s, window, bbox, bins, hist_range, nodata, device) + (s.meta,)


# ------------------------------------------------------------------------------------------ zonal statistics
def _zone_crop(zones, shape, win) -> np.ndarray:
    """The whole zone raster ``(H, W)`` checked against the raster's shape and cropped to ``win`` (a view)."""
    zones = np.asarray(zones)
    if zones.dtype.kind not in "iu":
        raise TypeError(f"the zone raster must have an integer dtype, got {zones.dtype}")
    if zones.shape != tuple(shape):
        raise ValueError(f"the zone raster must be {tuple(shape)} like the raster, got {zones.shape}")
    r, c, h, w = win
    return zones[r:r + h, c:c + w]


def _zonal_on_device(run, crop: np.ndarray, dt, nodata, ignore):
    """The report of one GPU call over the cropped zone raster: ``run(zones, zone_lo, nzones, ignore)`` returns the
    records and the outside count.  Labels spread too far for one call are relabelled first (``zonal.dense_zones``),
    and 64-bit labels go as int32 offsets from the smallest."""
    from .zonal import ZONE_DTYPES, dense_zones, report_from_recs

    zones, zone_lo, nzones, labels = dense_zones(crop, ignore)
    if labels is not None:
        ignore = None  # the ignored pixels carry id -1, outside the range
    first = zone_lo  # the label of zone 0 when there is no label table
    if zones.dtype not in ZONE_DTYPES:
        with np.errstate(over="ignore"):
            k = (zones - zones.dtype.type(zone_lo)).astype(np.int64)  # (an ignored label may wrap: it is replaced)
        zones = (k if ignore is None else np.where(zones == ignore, -1, k)).astype(np.int32)
        zone_lo, ignore = 0, None
    elif not zones.dtype.isnative or any(st < 0 for st in zones.strides):
        zones = np.ascontiguousarray(zones, dtype=zones.dtype.newbyteorder("="))
    recs, outside = run(zones, zone_lo, nzones, ignore)
    return report_from_recs(recs, outside, dt, first, labels)


def _zonal(s, win, crop: np.ndarray, nodata, ignore, device, semantics):
    """The report of the window ``win`` of a source over ``crop``, the zones of that window."""
    from . import _native
    from .zonal import zonal_arrays

    nodata = _nodata(s, nodata)
    reg = s.region(win, semantics)
    if device is None:
        return zonal_arrays(reg.host(), crop, nodata=nodata, ignore=ignore)
    ctx = _native.default_context(int(device))
    if reg.encoded:
        data, items, dt, B, _ = reg.decode_args()

        def run(z, zone_lo, nzones, ign):
            recs, outside, _ = ctx.decode_device_zonal(data, items, z, dt, B, win, reg.denorm, zone_lo, nzones, nodata, ign)
            return recs, outside
    else:
        a = reg.host()

        def run(z, zone_lo, nzones, ign):
            return ctx.zonal(a, z, zone_lo, nzones, nodata, ign)

    return _zonal_on_device(run, crop, s.dtype, nodata, ignore)


def _zonal_over_array(s, zones, window, bbox, nodata, ignore, device, semantics=None):
    """Zonal statistics of a source over the whole ``(H, W)`` zone raster ``zones`` -> ``(report, window, meta)``."""
    win = s.window(window, bbox)
    crop = _zone_crop(zones, (s.height, s.width), win)
    return _zonal(s, win, crop, nodata, ignore, device, semantics), win, s.meta


def container_zonal(src, zones, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                    nodata: Optional[float] = None, ignore: Optional[int] = None, device: Optional[int] = None,
                    semantics: str = "pcm16"):
    """Zonal statistics of a streaming container (path or bytes), or of a window of it -> ``(report, window, index)``:
    ``zonal.zonal_arrays(read_window(src, ...)[0], zones cropped to the window, nodata=nodata, ignore=ignore)``.

    ``zones`` is the whole ``(H, W)`` zone raster of the container's raster (``ValueError`` otherwise), of an integer
    dtype; ``window`` / ``bbox`` as in :func:`read_window` (default: the whole raster).  ``device=None`` reads the
    window on the host and applies the numpy rule; an integer makes one ``fra_decode_device_zonal`` call on that GPU:
    the decoded pixels never leave the device, the cropped zone raster goes there, and only the records come back."""
    return _zonal_over_array(ContainerSource(src), zones, window, bbox, nodata, ignore, device, semantics)


def tiff_zonal(path: Path, zones, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
               nodata: Optional[float] = None, ignore: Optional[int] = None, device: Optional[int] = None):
    """Zonal statistics of a GeoTIFF, or of a window of it, over the whole ``(H, W)`` zone raster ``zones`` ->
    ``(report, window, info)``.  The window is read with the in-package reader; an integer ``device`` hands it to
    ``fra_zonal`` on that GPU, ``None`` to the numpy rule.  ``nodata=None`` takes the TIFF's own nodata tag, when it
    has one."""
    return _zonal_over_array(TiffSource(path), zones, window, bbox, nodata, ignore, device)


def zonal_with_tiff(source: Path, zones_tiff: Path, window: Optional[Sequence[int]] = None,
                    bbox: Optional[Sequence[float]] = None, nodata: Optional[float] = None,
                    ignore: Optional[int] = None, device: Optional[int] = None, semantics: str = "pcm16"):
    """Zonal statistics of ``source`` -- a streaming container or a GeoTIFF -- over the zones of a single-band integer
    GeoTIFF of the same shape -> ``(report, window, index or info)``.  Only the window of the zones TIFF is read
    (in-package reader).  ``ignore=None`` takes the zones TIFF's nodata tag, when it has one; ``nodata=None`` a source
    TIFF's."""
    source, zones_tiff = Path(source), Path(zones_tiff)
    s = open_source(source)
    win = s.window(window, bbox)
    z = TiffSource(zones_tiff)
    if z.bands != 1 or z.dtype.kind not in "iu":
        raise ValueError(f"{zones_tiff.name} must be a single-band integer raster, it has {z.bands} band(s) of {z.dtype}")
    if (z.height, z.width) != (s.height, s.width):
        raise ValueError(f"{zones_tiff.name} is {(z.height, z.width)}, {source.name} is {(s.height, s.width)}")
    if ignore is None and z.nodata is not None and z.nodata == int(z.nodata):
        ignore = int(z.nodata)
    crop = z.region(win).host()[0]
    return _zonal(s, win, crop, nodata, ignore, device, semantics), win, s.meta


# ------------------------------------------------------------------------------------------ polygons
def _label_dtype(values, fill) -> np.dtype:
    """The narrowest of the six label dtypes that holds every burn value and the fill."""
    lo, hi = min([int(fill)] + [int(v) for v in values]), max([int(fill)] + [int(v) for v in values])
    for t in ((np.uint8, np.uint16, np.uint32) if lo >= 0 else (np.int8, np.int16, np.int32)):
        if np.iinfo(t).min <= lo and hi <= np.iinfo(t).max:
            return np.dtype(t)
    raise ValueError(f"burn values {lo} .. {hi} do not fit an integer dtype of 32 bits")


def _pixel_features(geojson, attribute, transform):
    """The polygons of a GeoJSON file in pixel coordinates of a grid, and their values."""
    from .rasterize import read_geojson, to_pixel

    if not transform:
        raise ValueError("the source has no transform: polygons cannot be placed on its grid")
    features, values = read_geojson(geojson, attribute)
    return to_pixel(features, Affine(*list(transform)[:6])), values


def _burn(pix, win, values, fill, dt, device):
    """``(raster, burned)`` of the window on the host (``device=None``) or on a GPU."""
    from . import _native
    from .rasterize import rasterize_arrays

    if device is None:
        return rasterize_arrays(pix, win, values, fill, dt)
    return _native.default_context(int(device)).rasterize(pix, win, values, fill, dt)


def _rasterize_like(source, geojson, attribute, burn, window, bbox, fill, dtype, device):
    """:func:`rasterize_like` with ``burn`` (one value for every feature, or ``None``) -> ``(raster, window, burned
    count, the source)``."""
    if burn is not None and attribute is not None:
        raise ValueError("give at most one of an attribute and a burn value")
    s = open_source(source)
    pix, values = _pixel_features(geojson, attribute, s.transform)
    if burn is not None:
        values = [int(burn)] * len(pix)
    win = s.window(window, bbox)
    dt = _label_dtype(values, fill) if dtype is None else np.dtype(dtype)
    raster, burned = _burn(pix, win, values, fill, dt, device)
    return raster, win, burned, s


def rasterize_like(source, geojson, attribute: Optional[str] = None, window: Optional[Sequence[int]] = None,
                   bbox: Optional[Sequence[float]] = None, fill: int = 0, dtype=None, device: Optional[int] = None):
    """The polygons of a GeoJSON file (a path or the parsed object; its coordinates are taken to be in the source's
    CRS) burned onto the grid of ``source`` -- a streaming container or a GeoTIFF -- or onto a window of it ->
    ``(raster (h, w), window, transform of the window, crs)``.

    Feature ``i`` burns ``i + 1``, or its integer property ``attribute``; ``fill`` elsewhere.  ``dtype=None`` picks the
    narrowest of the six label dtypes that holds them.  ``device=None`` applies ``rasterize.rasterize_arrays``, an
    integer makes one ``fra_rasterize`` call on that GPU; both are given the same pixel coordinates."""
    raster, win, _, s = _rasterize_like(source, geojson, attribute, None, window, bbox, fill, dtype, device)
    return raster, win, s.window_transform(win), s.crs


def rasterize_to_tiff(source, geojson, tiff_path: Path, attribute: Optional[str] = None, burn: Optional[int] = None,
                      window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None, fill: int = 0,
                      dtype=None, device: Optional[int] = None):
    """:func:`rasterize_like` into a single-band GeoTIFF on the source's grid with the fill as its nodata tag; ``burn``:
    one value for every feature instead of ``i + 1`` or an attribute.  Returns ``(window, burned, dtype)``."""
    raster, win, burned, s = _rasterize_like(source, geojson, attribute, burn, window, bbox, fill, dtype, device)
    _to_tiff(tiff_path, raster[None], s, win, nodata=int(fill))
    return win, burned, raster.dtype


def zonal_with_polygons(source, geojson, attribute: Optional[str] = None, window: Optional[Sequence[int]] = None,
                        bbox: Optional[Sequence[float]] = None, nodata: Optional[float] = None,
                        device: Optional[int] = None, semantics: str = "pcm16"):
    """Zonal statistics of ``source`` -- a streaming container or a GeoTIFF -- over the polygons of a GeoJSON file ->
    ``(report, window, index or info)``.  Feature ``i`` is zone ``i + 1``, or the zone of its integer property
    ``attribute`` (features may share one); 0 is the fill and no zone, so a label of 0 is refused.

    The labels are burned for the window only.  ``device=None``: ``zonal.zonal_arrays`` over
    ``rasterize.rasterize_arrays``.  On a GPU ``fra_rasterize`` burns them into a device buffer that goes to
    ``fra_decode_device_zonal`` / ``fra_zonal`` as it is: the label raster never visits the host.  Labels spread over
    more than 65536 values are burned as dense ids (``zonal.dense_zones``) and the report carries the labels."""
    from . import _native
    from .zonal import dense_zones, report_from_recs, zonal_arrays

    s = open_source(Path(source))
    win = s.window(window, bbox)
    nodata = _nodata(s, nodata)
    reg = s.region(win, semantics)
    pix, values = _pixel_features(geojson, attribute, s.transform)
    if any(int(v) == 0 for v in values):
        raise ValueError("a zone label of 0 is not possible: 0 is what the pixels outside every polygon get")
    if values:
        _, zone_lo, nzones, labels = dense_zones(np.asarray(values, dtype=np.int64))
    else:
        zone_lo, nzones, labels = 1, 1, None
    if labels is None and values and not -2**31 <= min(values) <= max(values) <= 2**31 - 1:
        labels = np.unique(np.asarray(values, dtype=np.int64))  # close together, but past 32 bits
    if labels is not None:  # dense ids 1 ... n stand for the labels
        values, zone_lo, nzones = (np.searchsorted(labels, np.asarray(values, dtype=np.int64)) + 1).tolist(), 1, labels.size
    zdt = _label_dtype(values, 0)
    h, w = win[2], win[3]
    if device is None:
        zones, _ = _burn(pix, win, values, 0, zdt, None)
        rep = zonal_arrays(reg.host(), zones, zone_lo, nzones, nodata=nodata, ignore=0)
        if labels is not None:
            for band in rep:
                for rec in band["zones"]:
                    rec["zone"] = int(labels[rec["zone"] - 1])
        return rep, win, s.meta
    ctx = _native.default_context(int(device))
    d_zones = ctx.alloc(h * w * zdt.itemsize)
    try:
        ctx.rasterize(pix, win, values, 0, zdt, dst=d_zones)
        if reg.encoded:
            data, items, dt, B, _ = reg.decode_args()
            recs, outside, _ = ctx.decode_device_zonal(data, items, d_zones, dt, B, win, reg.denorm, zone_lo, nzones,
                                                       nodata, 0, zone_dtype=zdt, zone_strides=(w, 1))
        else:
            recs, outside = ctx.zonal(reg.host(), d_zones, zone_lo, nzones, nodata, 0, zone_dtype=zdt, zone_strides=(w, 1))
    finally:
        ctx.free(d_zones)
    return report_from_recs(recs, outside, s.dtype, zone_lo, labels), win, s.meta


# ------------------------------------------------------------------------------------------ proximity
def _proximity_opts(opts, transform, units: str):
    """``opts`` (default: none) with the scale of ``units``: 1 for pixels, the pixel size for map units."""
    import dataclasses

    from .proximity import Options, scale_of, validate

    opts = dataclasses.replace(opts or Options(), scale=scale_of(transform, units))
    validate(opts)
    return opts


def _proximity_region(win, opts, H: int, W: int):
    """The region a window's result needs, and the window relative to it: the window grown by the halo of ``max_dist``
    and clipped to the ``H x W`` raster; the whole raster without a ``max_dist``, when any target may be the nearest."""
    from .proximity import halo

    k = halo(opts)
    if k is None:
        return (0, 0, H, W), tuple(win)
    r, c, h, w = win
    r0, c0, r1, c1 = max(r - k, 0), max(c - k, 0), min(r + h + k, H), min(c + w + k, W)
    return (r0, c0, r1 - r0, c1 - c0), (r - r0, c - c0, h, w)


def _proximity(s, opts, window, bbox, units, dist_dtype, want_alloc, device, semantics=None):
    """Proximity over a source -> ``(dist, alloc or None, counts, window, the options used)``."""
    from . import _native
    from .proximity import proximity_arrays

    opts = _proximity_opts(opts, s.transform, units)
    win = s.window(window, bbox)
    region, inner = _proximity_region(win, opts, s.height, s.width)
    reg = s.region(region, semantics)
    odt = np.dtype(dist_dtype)
    if device is None:
        dist, alloc, counts = proximity_arrays(reg.host(), opts, inner, odt)
        return dist, alloc if want_alloc else None, counts, win, opts
    ctx = _native.default_context(int(device))
    if reg.encoded:
        dist, alloc, counts, _ = ctx.decode_device_proximity(*reg.decode_args(), opts, odt,
                                                             alloc=None if want_alloc else False, out_window=inner,
                                                             denorm=reg.denorm)
    else:
        dist, alloc, counts = ctx.proximity(reg.host(), opts, odt, alloc=None if want_alloc else False, out_window=inner)
    return dist, alloc, counts, win, opts


def proximity_window(src, opts=None, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                     units: str = "pixel", dist_dtype="float32", want_alloc: bool = False, device: Optional[int] = None,
                     semantics: str = "pcm16"):
    """The distance of every pixel of a streaming container (path or bytes), or of a window of it, to the nearest
    target pixel -> ``(dist (B, h, w) in dist_dtype, alloc (B, h, w) in the container's dtype or None, counts, window,
    index)``: the crop of ``proximity.proximity_arrays`` over the whole raster.

    ``opts``: a ``proximity.Options`` whose ``max_dist`` is in ``units`` -- ``'pixel'``, or ``'geo'`` for the map units
    of the container's transform (square, axis-aligned pixels; anything else is refused).  With a ``window`` / ``bbox``
    and a ``max_dist`` the decoded region is the window grown by ``ceil(max_dist / scale)`` pixels and clipped to the
    raster; without a ``max_dist`` it is the whole raster.  ``device=None`` reads the region on the host and applies the
    numpy rule; an integer makes one ``fra_decode_device_proximity`` call on that GPU: the decoded pixels never leave
    the device."""
    s = ContainerSource(src)
    return _proximity(s, opts, window, bbox, units, dist_dtype, want_alloc, device, semantics)[:4] + (s.meta,)


def proximity_tiff(path: Path, opts=None, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                   units: str = "pixel", dist_dtype="float32", want_alloc: bool = False, device: Optional[int] = None):
    """:func:`proximity_window` for a GeoTIFF source -> ``(dist, alloc, counts, window, info, the options used)``.  The
    region is read with the in-package reader; an integer ``device`` hands it to ``fra_proximity`` on that GPU, ``None``
    to the numpy rule."""
    s = TiffSource(path)
    dist, alloc, counts, win, opts = _proximity(s, opts, window, bbox, units, dist_dtype, want_alloc, device)
    return dist, alloc, counts, win, s.meta, opts


def _proximity_to_tiff(s, win, opts, tiff_path, dist, alloc_path, alloc):
    """The distances, and with ``alloc_path`` the nearest targets' values, as GeoTIFFs on the window's grid with the
    fills of ``opts`` as their nodata tags."""
    from .proximity import default_fill

    fill = default_fill(dist.dtype) if opts.fill is None else opts.fill
    _to_tiff(tiff_path, dist, s, win, nodata=_fill_tag(fill, dist.dtype))
    if alloc_path is not None:
        _to_tiff(alloc_path, alloc, s, win, nodata=_fill_tag(opts.alloc_fill, alloc.dtype))


def proximity_to_tiff(path: Path, tiff_path: Path, opts=None, window: Optional[Sequence[int]] = None,
                      bbox: Optional[Sequence[float]] = None, units: str = "pixel", dist_dtype="float32",
                      alloc_path: Optional[Path] = None, device: Optional[int] = None, semantics: str = "pcm16"):
    """Proximity over a streaming container or a GeoTIFF (told apart by their first bytes) -> a GeoTIFF of the distances
    with the source's CRS, the transform shifted to the window's origin and the fill as its nodata tag; ``alloc_path``:
    a second GeoTIFF of the nearest targets' values, ``alloc_fill`` as its nodata tag.  Returns ``(window, counts)``."""
    s = open_source(Path(path))
    dist, alloc, counts, win, opts = _proximity(s, opts, window, bbox, units, dist_dtype, alloc_path is not None, device,
                                                semantics)
    _proximity_to_tiff(s, win, opts, tiff_path, dist, alloc_path, alloc)
    return win, counts


def _proximity_of_polygons(s, geojson, attribute, opts, window, bbox, units, dist_dtype, device):
    """:func:`proximity_of_polygons` over the grid of a source -> ``(dist, alloc, counts, window, the options used)``."""
    from . import _native
    from .proximity import proximity_arrays

    pix, values = _pixel_features(geojson, attribute, s.transform)
    if any(int(v) == 0 for v in values):
        raise ValueError("a label of 0 is not possible: 0 is what the pixels outside every polygon get")
    opts = _proximity_opts(opts, s.transform, units)
    win = s.window(window, bbox)
    region, inner = _proximity_region(win, opts, s.height, s.width)
    zdt, odt = _label_dtype(values, 0), np.dtype(dist_dtype)
    if device is None:
        labels, _ = _burn(pix, region, values, 0, zdt, None)
        dist, alloc, counts = proximity_arrays(labels, opts, inner, odt)
    else:
        ctx = _native.default_context(int(device))
        d_labels = ctx.alloc(region[2] * region[3] * zdt.itemsize)
        try:
            ctx.rasterize(pix, region, values, 0, zdt, dst=d_labels)
            dist, alloc, counts = ctx.proximity(d_labels, opts, odt, out_window=inner, dtype=zdt,
                                                shape=(1, region[2], region[3]))
        finally:
            ctx.free(d_labels)
    return dist, alloc, counts, win, opts


def proximity_of_polygons(source, geojson, attribute: Optional[str] = None, opts=None,
                          window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                          units: str = "pixel", dist_dtype="float32", device: Optional[int] = None):
    """The distance of every pixel of the grid of ``source`` -- a streaming container or a GeoTIFF, whose pixels are not
    read -- to the nearest polygon of a GeoJSON file, and that polygon's label -> ``(dist (1, h, w), alloc (1, h, w),
    counts, window, transform of the window, crs)``.  Feature ``i`` has the label ``i + 1``, or its integer property
    ``attribute``; 0 is what a pixel outside every polygon is burned with, so a label of 0 is refused.

    ``device=None``: ``proximity.proximity_arrays`` over ``rasterize.rasterize_arrays``.  On a GPU ``fra_rasterize``
    burns the labels of the region into a device buffer that goes to ``fra_proximity`` as it is: the label raster never
    visits the host."""
    s = open_source(source)
    dist, alloc, counts, win, _ = _proximity_of_polygons(s, geojson, attribute, opts, window, bbox, units, dist_dtype,
                                                         device)
    return dist, alloc, counts, win, s.window_transform(win), s.crs


def proximity_of_polygons_to_tiff(source, geojson, tiff_path: Path, attribute: Optional[str] = None, opts=None,
                                  window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                                  units: str = "pixel", dist_dtype="float32", alloc_path: Optional[Path] = None,
                                  device: Optional[int] = None):
    """:func:`proximity_of_polygons` into GeoTIFFs as :func:`proximity_to_tiff` writes them: the distances, and with
    ``alloc_path`` the nearest polygons' labels.  Returns ``(window, counts)``."""
    s = open_source(source)
    dist, alloc, counts, win, opts = _proximity_of_polygons(s, geojson, attribute, opts, window, bbox, units, dist_dtype,
                                                            device)
    _proximity_to_tiff(s, win, opts, tiff_path, dist, alloc_path, alloc)
    return win, counts


# ------------------------------------------------------------------------------------------ regions
_TABLE_GUESS = 4096  # records per band the first GPU call has room for; the library says how many it takes


def _regions_on_device(ctx, reg, opts, label_dtype, area_dtype, labels, area, sieved, want_table, out_strides=None):
    """One regions call over a region on a GPU, repeated once with the table the library asked for ->
    ``(labels, area, sieved, tables or None, counts)``."""
    from . import _native

    def call(cap):
        kw = dict(label_dtype=label_dtype, area_dtype=area_dtype, labels=labels, area=area, sieved=sieved,
                  table=cap if want_table else None, out_strides=out_strides)
        if reg.encoded:
            return ctx.decode_device_regions(*reg.decode_args(), opts, denorm=reg.denorm, **kw)[:5]
        return ctx.regions(reg.host(), opts, **kw)

    try:
        got = call(_TABLE_GUESS)
    except _native.RegionsNoSpace as e:
        n = int(e.counts[:, 2].max())
        if not want_table or n <= _TABLE_GUESS:
            raise  # the labels dtype is what does not hold them
        got = call(n)
    lab, ar, sv, table, counts = got
    tables = None if table is None else [table[b, :int(counts[b, 2])].copy() for b in range(table.shape[0])]
    return lab, ar, sv, tables, counts


def _regions(s, opts, window, bbox, label_dtype, area_dtype, want_area, want_sieved, device, semantics=None):
    """Regions over a source -> ``(labels, area or None, sieved or None, tables, counts, window)``."""
    from . import _native
    from .regions import Options, check_label_dtype, regions_arrays, validate

    opts = opts or Options()
    validate(opts)
    ldt = check_label_dtype(label_dtype)
    win = s.window(window, bbox)
    reg = s.region(win, semantics)
    if device is None:
        lab, ar, sv, tables, counts = regions_arrays(reg.host(), opts, ldt, area_dtype if want_area else None)
        return lab, ar, sv if want_sieved else None, tables, counts, win
    ctx = _native.default_context(int(device))
    return _regions_on_device(ctx, reg, opts, ldt, area_dtype, None, None if want_area else False,
                              None if want_sieved else False, True) + (win,)


def regions_window(src, opts=None, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                   label_dtype="int32", area_dtype="uint32", want_area: bool = False, want_sieved: bool = False,
                   device: Optional[int] = None, semantics: str = "pcm16"):
    """The connected components of a streaming container (path or bytes), or of a window of it -> ``(labels (B, h, w),
    area or None, sieved or None, tables (a list of B arrays of regions.REC), counts (B, 4), window, index)``:
    ``regions.regions_arrays(read_window(src, ...)[0], opts)``.  A window of a raster labels the window: a component is
    cut at its edge.  ``device=None`` reads the window on the host and applies the numpy rule; an integer makes one
    ``fra_decode_device_regions`` call on that GPU -- the decoded pixels never leave the device -- and a second one when
    a band has more components than the first table holds."""
    s = ContainerSource(src)
    return _regions(s, opts, window, bbox, label_dtype, area_dtype, want_area, want_sieved, device, semantics) + (s.meta,)


def regions_tiff(path: Path, opts=None, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                 label_dtype="int32", area_dtype="uint32", want_area: bool = False, want_sieved: bool = False,
                 device: Optional[int] = None):
    """:func:`regions_window` for a GeoTIFF source (``fra_regions`` on a GPU); the last element is its info."""
    s = TiffSource(path)
    return _regions(s, opts, window, bbox, label_dtype, area_dtype, want_area, want_sieved, device) + (s.meta,)


def export_components(path: Path, rows: List[dict]):
    """The rows of ``regions.export_rows`` as JSON (``.json``) or CSV (anything else)."""
    path = Path(path)
    if path.suffix.lower() == ".json":
        path.write_text(json.dumps({"components": rows}, indent=1))
        return
    import csv

    with open(path, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0].keys()) if rows else ["band", "label"])
        wr.writeheader()
        wr.writerows(rows)


def regions_to_tiff(path: Path, tiff_path: Path, opts=None, window: Optional[Sequence[int]] = None,
                    bbox: Optional[Sequence[float]] = None, label_dtype="int32", area_path: Optional[Path] = None,
                    sieved_path: Optional[Path] = None, export_path: Optional[Path] = None, area_dtype="uint32",
                    device: Optional[int] = None, semantics: str = "pcm16"):
    """Regions over a streaming container or a GeoTIFF (told apart by their first bytes) -> a GeoTIFF of the labels on
    the window's grid with nodata 0; ``area_path``: a GeoTIFF of the areas (nodata 0); ``sieved_path``: the source with
    the removed components filled (``sieve_fill`` as its nodata tag); ``export_path``: a ``.json`` or ``.csv`` with a row
    per band and component (``regions.export_rows``).  Returns ``(window, counts)``."""
    from .regions import Options, export_rows

    opts = opts or Options()
    s = open_source(Path(path))
    # a kept component's pixels keep the source's bits in `sieved`: the export takes the components' values from it
    want_sieved = sieved_path is not None or export_path is not None
    lab, ar, sv, tables, counts, win = _regions(s, opts, window, bbox, label_dtype, area_dtype, area_path is not None,
                                                want_sieved, device, semantics)
    _to_tiff(tiff_path, lab, s, win, nodata=0)
    if area_path is not None:
        _to_tiff(area_path, ar, s, win, nodata=0)
    if sieved_path is not None:
        _to_tiff(sieved_path, sv, s, win, nodata=_fill_tag(opts.sieve_fill, sv.dtype))
    if export_path is not None:
        export_components(export_path, export_rows(sv, tables, s.window_transform(win)))
    return win, counts


def sieve_to_tiff(path: Path, tiff_path: Path, min_size: int, connectivity: int = 4, by_value: bool = True,
                  values: Sequence[float] = (), invert: bool = False, fill: float = 0.0,
                  window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                  device: Optional[int] = None, semantics: str = "pcm16"):
    """The source with every component of fewer than ``min_size`` pixels replaced by ``fill`` -> a GeoTIFF with ``fill`` as
    its nodata tag.  Components are regions of one value by default (``by_value``), as ``gdal_sieve`` sees them; the
    removed ones are filled and not merged into a neighbour.  Returns ``(window, counts)``."""
    from .regions import Options

    opts = Options(tuple(values), invert, by_value, connectivity, min_size, fill)
    s = open_source(Path(path))
    _, _, sv, _, counts, win = _regions(s, opts, window, bbox, "int32", "uint32", False, True, device, semantics)
    _to_tiff(tiff_path, sv, s, win, nodata=_fill_tag(fill, sv.dtype))
    return win, counts


def zonal_of_regions(source, mask_source, opts=None, window: Optional[Sequence[int]] = None,
                     bbox: Optional[Sequence[float]] = None, nodata: Optional[float] = None,
                     device: Optional[int] = None, semantics: str = "pcm16"):
    """Zonal statistics of ``source`` over the connected components of ``mask_source``, a single-band raster on the same
    grid (each a streaming container or a GeoTIFF) -> ``(report, window, index or info of the source, counts of the
    components)``.  Component ``i`` of the window is zone ``i``.

    ``device=None``: ``zonal.zonal_arrays`` over the labels of ``regions.regions_arrays``.  On a GPU the labels are born
    in a device buffer that goes to ``fra_decode_device_zonal`` / ``fra_zonal`` as it is: the label raster never visits
    the host.  More than 65536 kept components are refused: raise ``min_size``."""
    from . import _native
    from .regions import MAX_ZONES, Options, regions_arrays, validate
    from .zonal import report_from_recs, zonal_arrays

    opts = opts or Options()
    validate(opts)
    s, m = open_source(source), open_source(mask_source)
    if m.bands != 1:
        raise ValueError(f"the mask must be a single-band raster, it has {m.bands} bands")
    if (m.height, m.width) != (s.height, s.width):
        raise ValueError(f"the mask is {(m.height, m.width)}, the source is {(s.height, s.width)}")
    win = s.window(window, bbox)
    nodata = _nodata(s, nodata)
    reg, mreg = s.region(win, semantics), m.region(win, semantics)
    h, w = win[2], win[3]

    def check(n):
        if n > MAX_ZONES:
            raise ValueError(f"{n} components are more than the {MAX_ZONES} zones of one call: drop the small ones with "
                             f"min_size (it is {opts.min_size})")
        return max(n, 1)

    if device is None:
        lab, _, _, _, counts = regions_arrays(mreg.host(), opts, np.int32, None)
        nzones = check(int(counts[0, 2]))
        return zonal_arrays(reg.host(), lab[0], 1, nzones, nodata=nodata, ignore=0), win, s.meta, counts
    ctx = _native.default_context(int(device))
    zdt = np.dtype(np.int32)
    d_zones = ctx.alloc(h * w * zdt.itemsize)
    try:
        counts = _regions_on_device(ctx, mreg, opts, zdt, "uint32", d_zones, False, False, False)[4]
        nzones = check(int(counts[0, 2]))
        if reg.encoded:
            data, items, dt, B, _ = reg.decode_args()
            recs, outside, _ = ctx.decode_device_zonal(data, items, d_zones, dt, B, win, reg.denorm, 1, nzones, nodata, 0,
                                                       zone_dtype=zdt, zone_strides=(w, 1))
        else:
            recs, outside = ctx.zonal(reg.host(), d_zones, 1, nzones, nodata, 0, zone_dtype=zdt, zone_strides=(w, 1))
    finally:
        ctx.free(d_zones)
    return report_from_recs(recs, outside, s.dtype, 1), win, s.meta, counts


# ------------------------------------------------------------------------------------------ band math
def _calc_fill(fill, out_dtype):
    from .calc import default_fill

    return default_fill(out_dtype) if fill is None else float(fill)


def _calc(s, exprs, window, bbox, out_dtype, nodata, fill, device, semantics=None):
    """Band math over a source -> ``(raster, left-out pixels, window, the nodata used)``."""
    from . import _native
    from .calc import calc_arrays, compile_exprs

    program = compile_exprs(exprs, s.bands)
    win = s.window(window, bbox)
    nodata = _nodata(s, nodata)
    odt = np.dtype(out_dtype)
    fill = _calc_fill(fill, odt)
    reg = s.region(win, semantics)
    if device is None:
        res, left = calc_arrays(reg.host(), program, odt, nodata, fill)
    elif reg.encoded:
        res, left, _ = _native.default_context(int(device)).decode_device_calc(
            *reg.decode_args(), program, odt, denorm=reg.denorm, nodata=nodata, fill=fill)
    else:
        res, left = _native.default_context(int(device)).calc(reg.host(), program, odt, nodata=nodata, fill=fill)
    return res, left, win, nodata


def calc_window(src, exprs, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                out_dtype="float32", nodata: Optional[float] = None, fill: Optional[float] = None,
                device: Optional[int] = None, semantics: str = "pcm16"):
    """Band math over a streaming container (path or bytes), or over a window of it -> ``(raster (nout, h, w) in
    out_dtype, left-out pixels per output band, window, index)``: ``calc.calc_arrays(read_window(src, ...)[0],
    calc.compile_exprs(exprs, bands), out_dtype, nodata, fill)``.

    ``exprs``: one expression per output band over ``b1 ... bN`` (``calc.compile_exprs``); ``window`` / ``bbox`` as in
    :func:`read_window` (default: the whole raster); ``nodata`` / ``fill`` as ``calc.calc_arrays``, the default ``fill``
    being NaN for float outputs and 0 for integer ones.  ``device=None`` reads the window on the host and applies the
    numpy rule; an integer makes one ``fra_decode_device_calc`` call on that GPU: the decoded pixels never leave the
    device and only the result comes back."""
    s = ContainerSource(src)
    return _calc(s, exprs, window, bbox, out_dtype, nodata, fill, device, semantics)[:3] + (s.meta,)


def calc_tiff(path: Path, exprs, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
              out_dtype="float32", nodata: Optional[float] = None, fill: Optional[float] = None,
              device: Optional[int] = None):
    """:func:`calc_window` for a GeoTIFF source -> ``(raster, left-out pixels, window, info, the nodata used)``.  The
    window is read with the in-package reader; an integer ``device`` hands it to ``fra_calc`` on that GPU, ``None`` to
    the numpy rule.  ``nodata=None`` takes the TIFF's own nodata tag, when it has one."""
    s = TiffSource(path)
    res, left, win, nodata = _calc(s, exprs, window, bbox, out_dtype, nodata, fill, device)
    return res, left, win, s.meta, nodata


def calc_to_tiff(path: Path, tiff_path: Path, exprs, window: Optional[Sequence[int]] = None,
                 bbox: Optional[Sequence[float]] = None, out_dtype="float32", nodata: Optional[float] = None,
                 fill: Optional[float] = None, device: Optional[int] = None, semantics: str = "pcm16"):
    """Band math over a streaming container or a GeoTIFF (told apart by their first bytes) -> GeoTIFF with the
    source's CRS and the transform shifted to the window's origin.  When a nodata value was given (or the source TIFF
    carries one) the result's nodata tag is ``fill`` as the output dtype holds it.  Returns ``(window, left-out pixels
    per output band, pixels per band)``."""
    s = open_source(Path(path))
    res, left, win, nodata = _calc(s, exprs, window, bbox, out_dtype, nodata, fill, device, semantics)
    tag = _fill_tag(_calc_fill(fill, res.dtype), res.dtype) if nodata is not None else None
    _to_tiff(tiff_path, res, s, win, nodata=tag)
    return win, left, int(win[2]) * int(win[3])


# ------------------------------------------------------------------------------------------ focal operations
def _pixel_sizes(transform) -> Tuple[float, float]:
    """``(dx, dy)`` = ``(|a|, |e|)`` of a transform; ``ValueError`` without one or with rotation terms."""
    if not transform:
        raise ValueError("the terrain ops need a transform (the pixel sizes)")
    a, b, _, d, e, _ = (float(v) for v in list(transform)[:6])
    if b != 0.0 or d != 0.0 or a == 0.0 or e == 0.0:
        raise ValueError("the terrain ops need an axis-aligned transform (no rotation terms)")
    return abs(a), abs(e)


def _focal_spec(spec, transform):
    """``spec`` itself, or ``spec(dx, dy)`` for a function of the pixel sizes (the terrain ops)."""
    return spec(*_pixel_sizes(transform)) if callable(spec) else spec


def _grown(win, spec, H: int, W: int):
    """``win`` grown by the radius of ``spec``'s window and clipped to an ``H x W`` raster, and ``win`` relative to it."""
    r, c, h, w = win
    ry, rx = spec.kh // 2, spec.kw // 2
    r0, c0, r1, c1 = max(r - ry, 0), max(c - rx, 0), min(r + h + ry, H), min(c + w + rx, W)
    return (r0, c0, r1 - r0, c1 - c0), (r - r0, c - c0, h, w)


def _focal(s, spec, window, bbox, out_dtype, device, semantics=None):
    """A focal operation over a source -> ``(raster, pixels that got fill, window, the spec used)``."""
    import dataclasses

    from . import _native
    from .focal import focal_arrays, validate

    spec = _focal_spec(spec, s.transform)
    if spec.nodata is None and s.nodata is not None:
        spec = dataclasses.replace(spec, nodata=s.nodata)
    validate(spec)
    win = s.window(window, bbox)
    grown, inner = _grown(win, spec, s.height, s.width)
    reg = s.region(grown, semantics)
    odt = np.dtype(out_dtype)
    if device is None:
        res, left = focal_arrays(reg.host(), spec, odt, inner)
    elif reg.encoded:
        res, left, _ = _native.default_context(int(device)).decode_device_focal(*reg.decode_args(), spec, inner, odt,
                                                                                denorm=reg.denorm)
    else:
        res, left = _native.default_context(int(device)).focal(reg.host(), spec, odt, out_window=inner)
    return res, left, win, spec


def focal_window(src, spec, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
                 out_dtype="float32", device: Optional[int] = None, semantics: str = "pcm16"):
    """A focal operation over a streaming container (path or bytes), or over a window of it -> ``(raster (B, h, w) in
    out_dtype, pixels that got fill per band, window, index)``: the crop of ``focal.focal_arrays`` over the whole
    raster.

    ``spec``: a ``focal.Spec``, or a function ``(dx, dy) -> Spec`` that receives the pixel sizes ``|a|`` and ``|e|`` of
    the container's transform (the terrain ops; a transform with rotation terms is then refused).  ``window`` / ``bbox``
    as in :func:`read_window` (default: the whole raster).  The window is grown by the radius of the spec's window and
    clipped to the raster, and the tiles of the grown window are selected: ``device=None`` reads it on the host and
    applies the numpy rule; an integer makes one ``fra_decode_device_focal`` call on that GPU: the decoded pixels never
    leave the device and only the result comes back."""
    s = ContainerSource(src)
    return _focal(s, spec, window, bbox, out_dtype, device, semantics)[:3] + (s.meta,)


def focal_tiff(path: Path, spec, window: Optional[Sequence[int]] = None, bbox: Optional[Sequence[float]] = None,
               out_dtype="float32", device: Optional[int] = None):
    """:func:`focal_window` for a GeoTIFF source -> ``(raster, pixels that got fill, window, info, the spec used)``.
    The grown window is read with the in-package reader; an integer ``device`` hands it to ``fra_focal`` on that GPU,
    ``None`` to the numpy rule.  A spec without a nodata value takes the TIFF's own nodata tag, when it has one."""
    s = TiffSource(path)
    res, left, win, spec = _focal(s, spec, window, bbox, out_dtype, device)
    return res, left, win, s.meta, spec


def focal_to_tiff(path: Path, tiff_path: Path, spec, window: Optional[Sequence[int]] = None,
                  bbox: Optional[Sequence[float]] = None, out_dtype="float32", device: Optional[int] = None,
                  semantics: str = "pcm16"):
    """A focal operation over a streaming container or a GeoTIFF (told apart by their first bytes) -> GeoTIFF with the
    source's CRS and the transform shifted to the window's origin.  When the spec used has a nodata value (its own or
    the source TIFF's) the result's nodata tag is ``fill`` as the output dtype holds it.  Returns ``(window, pixels that
    got fill per band, pixels per band)``."""
    s = open_source(Path(path))
    res, left, win, spec = _focal(s, spec, window, bbox, out_dtype, device, semantics)
    tag = _fill_tag(_calc_fill(spec.fill, res.dtype), res.dtype) if spec.nodata is not None else None
    _to_tiff(tiff_path, res, s, win, nodata=tag)
    return win, left, int(win[2]) * int(win[3])


# ------------------------------------------------------------------------------------------ warped reads
def _warp_map(src_transform, src_crs, dst_transform, out_shape, dst_crs, coords, grid_step, max_error):
    """The ``warp.Map`` of an output grid onto a source: an affine map within one CRS, else a coordinate grid fitted to
    ``coords`` (output CRS -> source CRS over arrays; default ``crs.transformer``).  Returns ``(map, step, error)``."""
    from . import warp
    from .crs import transformer

    if not src_transform:
        raise ValueError("the source has no transform")
    same = dst_crs is None or not src_crs or str(dst_crs).strip().upper() == str(src_crs).strip().upper()
    if coords is None and same:
        return warp.affine_map(dst_transform, src_transform), 0, 0.0
    if coords is None:
        coords = transformer(dst_crs, src_crs)
    da, db, dc, dd, de, df = (float(v) for v in tuple(dst_transform)[:6])
    inv = warp.affine_map((1.0, 0.0, 0.0, 0.0, 1.0, 0.0), src_transform).affine  # source CRS -> source pixels

    def pixel(cols, rows):
        x, y = coords(da * cols + db * rows + dc, dd * cols + de * rows + df)
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return (inv[0] * x + inv[1] * y) + inv[2], (inv[3] * x + inv[4] * y) + inv[5]

    if grid_step is not None:
        m = warp.grid_map(pixel, out_shape, int(grid_step))
        return m, m.step, warp.centre_error(m, pixel)
    m, err = warp.fit_grid(pixel, out_shape, max_error)
    return m, m.step, err


def _warp(s, dst_transform, out_shape, dst_crs, coords, resampling, nodata, fill, device, cpu, grid_step, max_error,
          semantics="pcm16"):
    """A source read onto another grid -> ``(raster, output transform, output CRS, info, the nodata used)``."""
    from . import _native, warp

    denorm = denorm_code(semantics)
    oh, ow = resample.check_out_shape(out_shape)
    warp.resampling_code(resampling)
    nodata = _nodata(s, nodata)
    H, W, B, dt = s.height, s.width, s.bands, s.dtype
    m, step, err = _warp_map(s.transform, s.crs, dst_transform, (oh, ow), dst_crs, coords, grid_step, max_error)
    warp.check_values(dt, nodata, fill)
    win = warp.source_window(m, (H, W), (oh, ow))
    # of a container only the window the map touches is decoded (none when the map misses the raster); a GeoTIFF is read
    # whole, as fra_warp takes it
    read = win if s.encoded else s.window()
    reg = s.region(read, semantics) if read is not None else None
    if cpu or device is None:
        region, origin = (np.zeros((B, 1, 1), dt), (0, 0)) if reg is None else (reg.host(), read[:2])
        out, filled = warp.warp_arrays(region, (oh, ow), m, resampling, nodata, fill, origin=origin, raster_shape=(H, W))
    elif s.encoded:
        data, items = (np.zeros(0, np.uint8), []) if reg is None else reg.decode_args()[:2]
        out = np.zeros((B, oh, ow), dtype=dt)
        _, filled = _native.default_context(int(device)).decode_device_warped(
            data, items, out, dt, B, (oh * ow, ow, 1), (H, W), (oh, ow), m, resampling, denorm, nodata=nodata, fill=fill)
    else:
        out, filled = _native.default_context(int(device)).warp(reg.host(), (oh, ow), m, resampling, nodata=nodata,
                                                                fill=fill)
    n = oh * ow
    info = {"map": m, "grid_step": step, "grid_error": err, "source_window": win, "filled": filled,
            "shares": [int(v) / n for v in filled], "index": s.meta if s.encoded else None}
    return out, tuple(float(v) for v in tuple(dst_transform)[:6]), (dst_crs or s.crs), info, nodata


def warp_window(src, dst_transform, out_shape, dst_crs=None, coords=None, resampling: str = "bilinear", nodata=None,
                fill=None, device: Optional[int] = None, cpu: bool = False, semantics: str = "pcm16",
                grid_step: Optional[int] = None, max_error: float = 0.125):
    """A streaming container (path or bytes) read onto another grid -> ``(raster (B, oh, ow) in the index's dtype,
    output transform, output CRS, info)``: ``warp.warp_arrays`` of the whole raster.

    The output grid is ``dst_transform`` (``geo.Affine`` or six floats) and ``out_shape`` in ``dst_crs`` (default: the
    container's CRS, where the map is the affine ``src^-1 o dst``).  Across CRSs the map is a coordinate grid fitted to
    ``coords`` (output CRS -> source CRS over arrays, e.g. a pyproj ``Transformer.transform``; default
    ``crs.transformer``) by ``warp.fit_grid(max_error)``, or built at ``grid_step``.  Only the source window the map
    touches (``warp.source_window``) is read.  An integer ``device`` makes one ``fra_decode_device_warped`` call on that
    GPU: the decoded window never leaves it and only the output comes back; ``cpu=True`` (or ``device=None``) decodes the
    window on the host and applies the numpy rule.  ``info``: the map, the grid step and the error reached, the source
    window (``None``: the map misses the raster), the pixels written as fill per band and their shares."""
    return _warp(ContainerSource(src), dst_transform, out_shape, dst_crs, coords, resampling, nodata, fill, device, cpu,
                 grid_step, max_error, semantics)[:4]


def warp_tiff(path: Path, dst_transform, out_shape, dst_crs=None, coords=None, resampling: str = "bilinear", nodata=None,
              fill=None, device: Optional[int] = None, cpu: bool = False, grid_step: Optional[int] = None,
              max_error: float = 0.125):
    """:func:`warp_window` for a GeoTIFF source, read whole with the in-package reader: ``fra_warp`` on the GPU
    ``device``, the numpy rule with ``cpu=True`` (or ``device=None``).  Without ``nodata`` the TIFF's own tag is used."""
    out, t, crs, info, nodata = _warp(TiffSource(path), dst_transform, out_shape, dst_crs, coords, resampling, nodata,
                                      fill, device, cpu, grid_step, max_error)
    info["nodata"] = nodata
    return out, t, crs, info


def warp_to_tiff(path: Path, tiff_path: Path, dst_transform, out_shape, dst_crs=None, coords=None,
                 resampling: str = "bilinear", nodata=None, fill=None, device: Optional[int] = None, cpu: bool = False,
                 semantics: str = "pcm16", grid_step: Optional[int] = None, max_error: float = 0.125):
    """A streaming container or a GeoTIFF (told apart by their first bytes) warped onto a grid -> GeoTIFF with the
    grid's transform and CRS; with a nodata value (the caller's or the source TIFF's) the nodata tag is the fill.
    Returns the ``info`` of :func:`warp_window`."""
    from . import warp

    s = open_source(Path(path))
    out, t, crs, info, nodata = _warp(s, dst_transform, out_shape, dst_crs, coords, resampling, nodata, fill, device,
                                      cpu, grid_step, max_error, semantics)
    if not s.encoded:
        info["nodata"] = nodata
    tag = None
    if nodata is not None:  # not _fill_tag: the warp's fill defaults to the nodata value (warp.check_values)
        v = warp.check_values(out.dtype, nodata, fill)[1]
        tag = float(v) if out.dtype.kind == "f" else int(v)
    _to_tiff(tiff_path, out, s, transform=t, crs=crs, nodata=tag)
    return info


def _read_overview(s: ContainerSource, factor, resampling, device, semantics, out_shape, max_size, nodata):
    """:func:`read_overview` of a source."""
    from . import _native

    if (factor is not None) + (out_shape is not None) + (max_size is not None) != 1:
        raise ValueError("give exactly one of factor, out_shape and max_size")
    H, W = s.height, s.width
    if max_size is not None:
        out_shape = resample.max_size_shape(H, W, max_size)
    if device is None:
        out, _, index = _read_window(s, s.window(), None, None, semantics,
                                     1 if factor is None else resample.check_factor(factor), resampling, out_shape, nodata)
        return out, index
    denorm = denorm_code(semantics)
    if factor is None:
        oh, ow = resample.check_out_shape(out_shape)
        resample.resampling_any_code(resampling)
    else:
        k = resample.check_factor(factor)
        resample.resampling_code(resampling)
        oh, ow = resample.decimated_shape(H, W, k)
    data, items = s.whole()  # to the device as they are
    out = np.zeros((s.bands, oh, ow), dtype=s.dtype)
    ctx = _native.default_context(int(device))
    args = np.frombuffer(data, dtype=np.uint8), items, out, s.dtype, s.bands, (oh * ow, ow, 1), s.window()
    if factor is None:
        ctx.decode_device_resampled(*args, (oh, ow), resampling, denorm, nodata=nodata)
    else:
        ctx.decode_device_decimated(*args, k, resampling, denorm, nodata=nodata)
    return out, s.meta


def read_overview(src, factor: Optional[int] = None, resampling: str = "average", device: Optional[int] = None,
                  semantics: str = "pcm16", out_shape: Optional[Sequence[int]] = None,
                  max_size: Optional[int] = None, nodata=None):
    """The whole raster of a streaming container (path or bytes) at ``1 / factor`` resolution -> ``(raster (B,
    ceil(H / k), ceil(W / k)) in the index's dtype, index)``: ``resample.decimate(streaming_to_raster(src)[0], factor,
    resampling)``.  ``device=None`` reads the raster on the host and decimates it with numpy; an integer makes one
    ``fra_decode_device_decimated`` call on that GPU: the full-resolution raster exists only in device memory and the
    overview alone is copied back (the container's bytes go to the device as they are, as in
    :func:`streaming_to_raster`).

    Instead of ``factor``: ``out_shape`` = (oh, ow), the whole raster resampled to that size
    (``resample.resample``, ``resampling`` any of its four; on a GPU one ``fra_decode_device_resampled`` call), or
    ``max_size`` = N, the output shape whose longest side is N (``resample.max_size_shape``).  ``nodata``: as
    :func:`read_window`."""
    return _read_overview(ContainerSource(src), factor, resampling, device, semantics, out_shape, max_size, nodata)


def _tiff_nodata(nodata, dtype):
    """A nodata value as the TIFF tag writes it: an integer for an integer dtype."""
    if nodata is None:
        return None
    nd = resample.check_nodata(nodata, dtype)
    return nd if np.dtype(dtype).kind == "f" else int(nd)


def nodata_share(raster: np.ndarray, nodata) -> list:
    """Per band of ``raster`` (B, h, w), the share of pixels that are ``nodata`` or, in a float dtype, NaN."""
    nd = resample.check_nodata(nodata, raster.dtype)
    return [float(1.0 - resample.valid_mask(band, nd).mean()) for band in raster]


def window_to_tiff(path: Path, tiff_path: Path, window: Optional[Sequence[int]] = None,
                   bbox: Optional[Sequence[float]] = None, device: Optional[int] = None, decimate: int = 1,
                   resampling: str = "nearest", out_shape: Optional[Sequence[int]] = None, nodata=None,
                   shares: Optional[list] = None):
    """A pixel window of a streaming container -> GeoTIFF with the index's CRS and the transform shifted to the
    window's origin (``decimate`` > 1: the window at that fraction of the resolution, ``out_shape``: the window
    resampled to that size; pixel size scaled to match; ``nodata``: as :func:`read_window`, and the TIFF carries the
    value in its nodata tag; ``shares``, a list, then receives :func:`nodata_share` of what was written); returns
    ``(window, index)``."""
    s = ContainerSource(Path(path))
    raster, win, index = _read_window(s, window, bbox, device, "pcm16", decimate, resampling, out_shape, nodata)
    transform = None  # the window's own
    if s.transform and out_shape is not None:
        transform = resample.resampled_transform(s.transform, win, out_shape)
    elif s.transform and decimate != 1:
        transform = resample.decimated_transform(s.transform, win, decimate)
    _to_tiff(tiff_path, raster, s, win, transform, nodata=_tiff_nodata(nodata, raster.dtype))
    if nodata is not None and shares is not None:
        shares.extend(nodata_share(raster, nodata))
    return win, index


def overview_to_tiff(path: Path, tiff_path: Path, factor: Optional[int] = None, resampling: str = "average",
                     device: Optional[int] = None, max_size: Optional[int] = None, nodata=None,
                     shares: Optional[list] = None):
    """The whole raster of a streaming container at ``1 / factor`` resolution, or with its longest side ``max_size``
    pixels -> GeoTIFF with the index's CRS and the pixel size scaled to match (``nodata``: as :func:`read_window`, and
    the TIFF carries the value in its nodata tag; ``shares`` as :func:`window_to_tiff`); returns ``(raster shape,
    index)``."""
    s = ContainerSource(Path(path))
    raster, index = _read_overview(s, factor, resampling, device, "pcm16", None, max_size, nodata)
    transform = None
    if s.transform and max_size is not None:
        transform = resample.resampled_transform(s.transform, s.window(), raster.shape[1:])
    elif s.transform:
        transform = resample.decimated_transform(s.transform, (0, 0), factor)
    _to_tiff(tiff_path, raster, s, transform=transform, nodata=_tiff_nodata(nodata, raster.dtype))
    if nodata is not None and shares is not None:
        shares.extend(nodata_share(raster, nodata))
    return raster.shape, index
