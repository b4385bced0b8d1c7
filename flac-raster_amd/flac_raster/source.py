"""Where the pixels of a windowed operation come from: a streaming container (a path or its bytes) or a GeoTIFF.

The two sources have one surface -- the grid (``height``, ``width``, ``bands``, ``dtype``), the georeferencing
(``transform``: six floats or ``None``, ``crs``: a string or ``None``), ``nodata`` (a GeoTIFF's tag; a container stores
none), ``meta`` (the index dict or the ``RasterInfo``), ``window(window, bbox)``, ``window_transform(win)`` and
``region(win, semantics)`` -- so that ``streaming`` writes each operation once.  A region's ``host()`` is the ``(B, h,
w)`` array.  A container's region also has ``decode_args()``, what every ``Context.decode_device_*`` call starts with,
and ``denorm``: the operations hand its tiles to the device undecoded.  That is the one place where they branch on
``region.encoded``, because the C ABI has two entries per unit.

``open_source`` tells the two apart by their first bytes and is the only place that looks at them.  The ``semantics``
check, the ``DENORM_*`` mapping, the CRS normalisation, the item of a tile and the host decode live here, once each.
"""

from __future__ import annotations

from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

from . import flac_meta
from .geo import Affine, window_transform
from .tiff import GeoTIFF

_TIFF_MAGIC = (b"II*\x00", b"MM\x00*", b"II+\x00", b"MM\x00+")


def denorm_code(semantics: str) -> int:
    """The ``FRA_DENORM_*`` code of ``semantics``: ``'pcm16'`` (what ``flac_to_tiff`` gives) or ``'int'``."""
    from . import _native

    if semantics not in ("pcm16", "int"):
        raise ValueError("semantics must be 'pcm16' or 'int'")
    return _native.DENORM_PCM16 if semantics == "pcm16" else _native.DENORM_INT


def normal_crs(crs) -> Optional[str]:
    """A CRS as a string, or ``None`` for none: an index stores ``str(None)`` for a raster without one."""
    crs = None if crs is None else str(crs)
    return crs if crs and crs != "None" else None


def _item(offset: int, tile: bytes, frame: dict) -> dict:
    """The ``decode_device`` item of one tile at ``offset`` of the bytes handed over: its byte range, its window and
    its own min / max tags."""
    tags = flac_meta.FLACFile(tile).tags
    w = frame["window"]
    return {"offset": offset, "bytes": frame["byte_size"],
            "window": (w["row_off"], w["col_off"], w["height"], w["width"]),
            "data_min": float(tags["GEOSPATIAL_DATA_MIN"][0]), "data_max": float(tags["GEOSPATIAL_DATA_MAX"][0])}


def _decode_window_on_host(blob, items, win, out: np.ndarray, semantics: str):
    """The tiles ``items`` of ``blob`` decoded on the host, denormalised and cropped into ``out`` (B, h, w), the window
    ``win`` of the raster."""
    from .decoder import decode_flac, pcm16_float
    from .normalization import NormalizationParams, denormalize_from_audio

    R, C_, h, w = win
    B, dt = out.shape[0], out.dtype
    for it in items:
        r, c, th, tw = it["window"]
        samples, _, bps = decode_flac(bytes(blob[it["offset"]:it["offset"] + it["bytes"]]))
        if samples.shape != (th * tw, B):
            raise ValueError(f"tile at ({r}, {c}) decodes to {samples.shape}, expected {(th * tw, B)}")
        params = NormalizationParams(it["data_min"], it["data_max"], str(dt), 16 if bps <= 16 else 24,
                                     32767 if bps <= 16 else 8388607)
        audio = pcm16_float(samples) if semantics == "pcm16" else samples
        tile = denormalize_from_audio(audio, params).reshape(th, tw, B).transpose(2, 0, 1)
        ra, rb, ca, cb = max(r, R), min(r + th, R + h), max(c, C_), min(c + tw, C_ + w)
        out[:, ra - R:rb - R, ca - C_:cb - C_] = tile[:, ra - r:rb - r, ca - c:cb - c]


class _Source:
    """What the two sources share: the window of a request and its transform."""

    encoded = False
    nodata: Optional[float] = None

    def window(self, window: Optional[Sequence[int]] = None,
               bbox: Optional[Sequence[float]] = None) -> Tuple[int, int, int, int]:
        """The clipped window of a request (``streaming.resolve_window``); the whole raster when both are ``None``."""
        from .streaming import resolve_window

        if window is None and bbox is None:
            return 0, 0, self.height, self.width
        return resolve_window({"height": self.height, "width": self.width, "transform": self.transform}, window, bbox)

    def window_transform(self, win):
        """The transform at the origin of ``win``; ``None`` when the source has none."""
        if not self.transform:
            return None
        return tuple(window_transform(Affine(*self.transform), win[1], win[0])[:6])


class ArrayRegion:
    """A region in host memory."""

    encoded = False

    def __init__(self, array: np.ndarray, win):
        self.array, self.win = array, tuple(win)

    def host(self) -> np.ndarray:
        return self.array


class TiffSource(_Source):
    """A GeoTIFF file, read with the in-package reader: opened for its tags here and once more for a region's pixels,
    so that nothing stays mapped between the two."""

    def __init__(self, path):
        self.path = Path(path)
        g = GeoTIFF(self.path)
        try:
            info = g.info
        finally:
            g.close()
        self.meta = info
        self.height, self.width, self.bands, self.dtype = info.height, info.width, int(info.count), np.dtype(info.dtype)
        self.transform = tuple(info.transform)[:6] if info.transform is not None else None
        self.crs = normal_crs(info.crs)
        self.nodata = float(info.nodata) if info.nodata is not None else None

    def region(self, win, semantics: Optional[str] = None) -> ArrayRegion:
        """The window ``win`` read into a fresh array (a GeoTIFF holds its pixels as they are: no ``semantics``)."""
        a = np.zeros((self.bands, win[2], win[3]), dtype=self.dtype)
        g = GeoTIFF(self.path)
        try:
            g.read_window_into(a, *win)
        finally:
            g.close()
        return ArrayRegion(a, win)


class ContainerRegion:
    """The tiles of a container that intersect a window, undecoded: ``blob`` holds their bytes back to back and
    ``items`` their ``decode_device`` items."""

    encoded = True

    def __init__(self, source: "ContainerSource", win, blob: bytearray, items: list, semantics: str):
        self.win, self.blob, self.items, self.semantics = tuple(win), blob, items, semantics
        self.denorm = denorm_code(semantics)
        self._dtype, self._bands = source.dtype, source.bands

    def host(self) -> np.ndarray:
        out = np.zeros((self._bands, self.win[2], self.win[3]), dtype=self._dtype)
        _decode_window_on_host(self.blob, self.items, self.win, out, self.semantics)
        return out

    def decode_args(self):
        """``data, items, dtype, bands, win``."""
        return np.frombuffer(self.blob, dtype=np.uint8), self.items, self._dtype, self._bands, self.win


class ContainerSource(_Source):
    """A streaming container, a path or its bytes (``bytes``, ``bytearray``, ``memoryview``).  The index is parsed here,
    once; of a file nothing else is read until a region is asked for, and then only the byte ranges of its tiles."""

    encoded = True

    def __init__(self, src):
        import struct

        from .streaming import open_streaming, read_index_bytes

        self._src = src
        if isinstance(src, (bytes, bytearray, memoryview)):
            self._path, view = None, memoryview(src)
            index, self._header = read_index_bytes(bytes(view[:4 + struct.unpack(">I", view[:4])[0]]))
        else:
            self._path = Path(src)
            sf = open_streaming(self._path)
            index, self._header = sf.index, sf.header_size
        self.meta = index
        self.height, self.width, self.bands = int(index["height"]), int(index["width"]), int(index["bands"])
        self.dtype = np.dtype(index["dtype"])
        t = index.get("transform")
        self.transform = tuple(t[:6]) if t else None
        self.crs = normal_crs(index.get("crs"))

    def _ranges(self, frames, size: int):
        """``(frame, start, end)`` of each of ``frames`` in a container of ``size`` bytes."""
        for fr in frames:
            a = self._header + fr["byte_offset"]
            b = a + fr["byte_size"]
            if b > size:
                raise ValueError(f"tile {fr['frame_id']} runs past the end of the container")
            yield fr, a, b

    def whole(self):
        """``(data, items)``: the container's bytes as they are and an item per tile, for the whole-container reads."""
        data = bytes(self._src) if self._path is None else self._path.read_bytes()
        return data, [_item(a, data[a:b], fr) for fr, a, b in self._ranges(self.meta["frames"], len(data))]

    def region(self, win, semantics: str = "pcm16") -> ContainerRegion:
        """The tiles that intersect ``win``; ``LookupError`` when none does."""
        R, C_, h, w = win

        def intersects(fw):
            return (fw["row_off"] < R + h and fw["row_off"] + fw["height"] > R and fw["col_off"] < C_ + w
                    and fw["col_off"] + fw["width"] > C_)

        frames = [fr for fr in self.meta["frames"] if intersects(fr["window"])]
        blob, items = bytearray(), []
        view = memoryview(self._src) if self._path is None else None
        fh = open(self._path, "rb") if self._path is not None else None
        try:
            for fr, a, b in self._ranges(frames, len(view) if fh is None else self._path.stat().st_size):
                if fh is None:
                    tile = bytes(view[a:b])
                else:
                    fh.seek(a)
                    tile = fh.read(b - a)
                items.append(_item(len(blob), tile, fr))
                blob += tile
        finally:
            if fh is not None:
                fh.close()
        if not items:
            raise LookupError("No tiles intersect the window")
        return ContainerRegion(self, win, blob, items, semantics)


def open_source(src):
    """The source of ``src``: container bytes, or the path of a streaming container or of a GeoTIFF."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        return ContainerSource(src)
    with open(src, "rb") as f:
        head = f.read(4)
    if head in _TIFF_MAGIC:
        return TiffSource(src)
    if head[:4] == b"fLaC" or head[:3] == b"ID3":  # a plain FLAC file (``streaming.is_streaming_container``)
        raise ValueError("a streaming FLAC file (convert --streaming) or a GeoTIFF is needed")
    return ContainerSource(src)
