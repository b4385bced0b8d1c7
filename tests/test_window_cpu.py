"""CPU tests of the windowed read (no GPU needed).

* the new C ABI names are declared, exported and bound; ``fra_decode_device_window`` refuses a null / zero-size
  region, ``FRA_DECODE_CONCAT`` and the capacity window before any GPU work.
* host ``read_window`` equals the crop of the host ``streaming_to_raster`` (which ``test_decode_cpu`` checks against
  the oracle's decoder), bit for bit, for both semantics; the bbox form; only the byte ranges of the intersecting
  tiles are read; the ``window`` CLI command on the host path.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster.geo import Affine
from flac_raster.streaming import (assemble_streaming, read_index_bytes, read_window, resolve_window,
                                   streaming_to_raster)
from flac_raster.tiff import read_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
H, W, TILE = 300, 420, 128  # 3 x 4 tiles, ragged right (36 columns) and bottom (44 rows)

# (row_off, col_off, height, width) as asked -> the same clipped to the raster
WINDOWS = {
    "inside one tile": ((10, 140, 50, 60), (10, 140, 50, 60)),
    "four-tile corner": ((100, 230, 60, 50), (100, 230, 60, 50)),
    "single pixel": ((299, 419, 1, 1), (299, 419, 1, 1)),
    "full row band": ((120, 0, 20, 420), (120, 0, 20, 420)),
    "whole raster": ((0, 0, 300, 420), (0, 0, 300, 420)),
    "over the edge": ((250, 380, 100, 100), (250, 380, 50, 40)),
}


@pytest.fixture(scope="module")
def container():
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (1000 + 60 * np.sin(yy / 23.0) + 40 * np.cos(xx / 31.0)).astype(np.int64)
    r = np.stack([base + b * 7 + rng.integers(0, 50, size=(H, W)) for b in range(3)]).astype(np.uint16)
    tiles = calculate_tiles(H, W, TILE)
    streams = oracle_encode_tiles(r, tiles, level=5)
    data = assemble_streaming(tiles, streams, r.shape, r.dtype, TRANSFORM, "EPSG:32633", TILE)
    full = {sem: streaming_to_raster(data, device=None, semantics=sem)[0] for sem in ("pcm16", "int")}
    for a in full.values():
        a.setflags(write=False)
    return data, full


def test_new_names_exported_and_declared():
    hdr = (ROOT / "include" / "flac_raster_amd.h").read_text()
    decl = set(re.findall(r"FRA_API\s+[^;(]*?\b(fra_\w+)\s*\(", hdr))
    L = N.load()
    assert "fra_decode_device_window" in decl and "fra_decode_device_window" in N.EXPORTS
    assert hasattr(L, "fra_decode_device_window") and hasattr(N.Context, "decode_device_window")
    assert L.fra_abi_version() == 3
    from flac_raster import tiles
    assert callable(tiles.read_window_on_device)


def test_window_entry_validates_arguments_without_a_gpu():
    """Every call returns FRA_E_INVALID before the context is looked at, so a stand-in pointer serves."""
    L = N.load()
    ctx = C.c_void_p(16)
    data = (C.c_uint8 * 64)()
    dst = (C.c_int32 * 64)()
    item = N.DecodeItem()
    item.offset, item.bytes, item.window = 0, 64, N.Window(0, 0, 1, 8)
    job = N.DecodeJob()
    job.data, job.len, job.items, job.nitems = C.cast(data, C.c_void_p), 64, C.pointer(item), 1
    job.dst, job.dst_dtype, job.channels = C.cast(dst, C.c_void_p), N.DTYPE_CODES[np.dtype(np.int32)], 1
    job.band_stride, job.row_stride, job.col_stride = 64, 8, 1
    infos = (N.Decoded * 1)()
    roi = N.Window(0, 0, 1, 8)

    def call(r):
        return L.fra_decode_device_window(ctx, C.byref(job), C.byref(r) if r is not None else None, infos)

    assert call(None) == -1 and b"null" in L.fra_last_error()
    assert L.fra_decode_device_window(None, C.byref(job), C.byref(roi), infos) == -1
    for bad in (N.Window(0, 0, 0, 8), N.Window(0, 0, 1, 0), N.Window(0, 0, -1, 8)):
        assert call(bad) == -1 and b"region of interest" in L.fra_last_error()
    job.flags = N.DECODE_CONCAT
    assert call(roi) == -1 and b"CONCAT" in L.fra_last_error()
    job.flags = 0
    item.window = N.Window(0, 0, -8, 1)
    assert call(roi) == -1 and b"capacity" in L.fra_last_error()
    item.window = N.Window(50, 50, 1, 8)  # outside the region, but the item must still lie inside the data
    item.offset = 60
    assert call(roi) == -1 and b"outside the data" in L.fra_last_error()


@pytest.mark.parametrize("sem", ["pcm16", "int"])
@pytest.mark.parametrize("name", list(WINDOWS))
def test_host_read_window_equals_the_crop(container, name, sem):
    data, full = container
    asked, (r, c, h, w) = WINDOWS[name]
    got, win, index = read_window(data, window=asked, device=None, semantics=sem)
    assert tuple(win) == (r, c, h, w) and index["height"] == H
    assert got.dtype == np.uint16 and got.shape == (3, h, w)
    assert np.array_equal(got, full[sem][:, r:r + h, c:c + w])


def test_bbox_form_rotation_and_empty_requests(container):
    data, full = container
    index, _ = read_index_bytes(data)
    # x 501403.5 .. 501999 -> columns floor(140.35) .. ceil(199.9); y 4099400.1 .. 4099899 -> rows floor(10.1) .. ceil(59.99)
    bbox = (501403.5, 4099400.1, 501999.0, 4099899.0)
    assert resolve_window(index, bbox=bbox) == (10, 140, 50, 60)
    got, win, _ = read_window(data, bbox=bbox)
    want, _, _ = read_window(data, window=(10, 140, 50, 60))
    assert win == (10, 140, 50, 60) and np.array_equal(got, want)
    assert np.array_equal(got, full["pcm16"][:, 10:60, 140:200])
    # a bbox hanging over the raster's corner is clipped
    assert resolve_window(index, bbox=(499000.0, 4099900.0, 500025.0, 4200000.0)) == (0, 0, 10, 3)
    with pytest.raises(ValueError):
        read_window(data)
    with pytest.raises(ValueError):
        read_window(data, window=(0, 0, 5, 5), bbox=bbox)
    with pytest.raises(ValueError):
        read_window(data, bbox=bbox[:3])
    with pytest.raises(ValueError):
        read_window(data, window=(0, 0, 5, 5), semantics="float")
    with pytest.raises(LookupError):
        read_window(data, window=(300, 0, 10, 10))
    with pytest.raises(LookupError):
        read_window(data, window=(10, 10, 0, 10))
    with pytest.raises(LookupError):
        read_window(data, bbox=(0.0, 0.0, 100.0, 100.0))
    rotated = dict(index, transform=[10.0, 0.5, 500000.0, 0.0, -10.0, 4100000.0, 0.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="rotation"):
        resolve_window(rotated, bbox=bbox)
    assert resolve_window(rotated, window=(1, 2, 3, 4)) == (1, 2, 3, 4)  # a pixel window needs no transform


def test_only_the_intersecting_tiles_are_read(container, tmp_path):
    data, full = container
    index, hs = read_index_bytes(data)
    r, c, h, w = 100, 230, 60, 50  # tiles (0, 1), (0, 2), (1, 1), (1, 2) of the 3 x 4 grid
    bad = bytearray(data)
    hit = []
    for fr in index["frames"]:
        fw = fr["window"]
        inside = (fw["row_off"] < r + h and fw["row_off"] + fw["height"] > r and fw["col_off"] < c + w
                  and fw["col_off"] + fw["width"] > c)
        a = hs + fr["byte_offset"]
        if inside:
            hit.append((a, fr["byte_size"]))
        else:
            bad[a:a + fr["byte_size"]] = b"\xa5" * fr["byte_size"]
    assert len(hit) == 4
    path = tmp_path / "garbled_streaming.flac"
    path.write_bytes(bad)
    got, win, _ = read_window(path, window=(r, c, h, w))
    assert win == (r, c, h, w) and np.array_equal(got, full["pcm16"][:, r:r + h, c:c + w])
    with pytest.raises(Exception):  # the whole-container read does meet the garbage
        streaming_to_raster(path, device=None)
    a, n = hit[2]
    bad[a + n // 2] ^= 0x10
    path.write_bytes(bad)
    with pytest.raises(N.NativeError):
        read_window(path, window=(r, c, h, w))


def test_window_cli_on_the_host(container, tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli

    data, full = container
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    monkeypatch.setattr(cli, "_gpu_present", lambda: False)  # the host path, wherever this runs
    out = tmp_path / "win.tif"
    res = CliRunner().invoke(cli.app, ["window", str(src), "-o", str(out), "--window", "100,230,60,50"])
    assert res.exit_code == 0, res.output
    px, info = read_geotiff(out)
    assert np.array_equal(px, full["pcm16"][:, 100:160, 230:280]) and "32633" in str(info.crs)
    t = tuple(info.transform)[:6]
    assert t == (10.0, 0.0, 500000.0 + 230 * 10.0, 0.0, -10.0, 4100000.0 - 100 * 10.0)
    out2 = tmp_path / "box.tif"
    res = CliRunner().invoke(cli.app, ["window", str(src), "-o", str(out2), "--bbox",
                                       "501403.5,4099400.1,501999.0,4099899.0"])
    assert res.exit_code == 0, res.output
    px2, info2 = read_geotiff(out2)
    assert np.array_equal(px2, full["pcm16"][:, 10:60, 140:200])
    assert tuple(info2.transform)[:6] == (10.0, 0.0, 501400.0, 0.0, -10.0, 4099900.0)
    # exactly one of the two forms
    assert CliRunner().invoke(cli.app, ["window", str(src), "-o", str(tmp_path / "x.tif")]).exit_code == 1
    assert CliRunner().invoke(cli.app, ["window", str(src), "-o", str(tmp_path / "x.tif"), "--window", "0,0,4,4",
                                        "--bbox", "0,0,1,1"]).exit_code == 1
