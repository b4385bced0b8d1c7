"""CPU tests of the read side added with the device decoder (no GPU needed).

* ``streaming_to_raster(device=None)``: the host implementation (``fra_decode`` per tile + ``denormalize_from_audio``)
  on a container assembled from oracle-encoded tiles; the expectation is built from the oracle's own decoder.
* ``convert container.flac -o scene.tif`` through the CLI.
* the new C ABI names are declared, exported and bound; the ctypes structures mirror the header's layout.
* ``decode_flac(device=None)`` is unchanged on the libFLAC golden file.
"""
import ctypes as C
import hashlib
import json
import re
from pathlib import Path

import numpy as np
import pytest

import oracle as O
from flac_raster import _native as N
from flac_raster.decoder import decode_flac, pcm16_float
from flac_raster.geo import Affine
from flac_raster.normalization import NormalizationParams, denormalize_from_audio
from flac_raster.streaming import assemble_streaming, is_streaming_container, streaming_to_raster, streaming_to_tiff
from flac_raster.tiff import read_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

ROOT = Path(__file__).resolve().parents[1]
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)


def _scene(B=3, H=300, W=420, seed=3):
    """uint16, a range of 200 per tile at most: the 16-bit mapping is lossless (one raster unit = 327 audio steps)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (1000 + 60 * np.sin(yy / 23.0) + 40 * np.cos(xx / 31.0)).astype(np.int64)
    r = np.stack([base + b * 7 + rng.integers(0, 50, size=(H, W)) for b in range(B)]).astype(np.uint16)
    return r


@pytest.fixture(scope="module")
def container():
    r = _scene()
    tiles = calculate_tiles(r.shape[1], r.shape[2], 128)  # ragged right and bottom tiles
    streams = oracle_encode_tiles(r, tiles, level=5)
    return r, tiles, streams, assemble_streaming(tiles, streams, r.shape, r.dtype, TRANSFORM, "EPSG:32633", 128)


def _expected_pcm16(r, tiles, streams):
    """flac_to_tiff per tile, from the ORACLE's decoder: PCM_16 floats, denormalised with the tile's min / max."""
    out = np.zeros_like(r)
    for (y, x, h, w), ts in zip(tiles, streams):
        dec, _, bps, _ = O.decode(ts.data)
        assert bps == 16
        p = NormalizationParams(ts.data_min, ts.data_max, str(r.dtype), 16, 32767)
        out[:, y:y + h, x:x + w] = denormalize_from_audio(pcm16_float(dec.astype(np.int16)), p).reshape(
            h, w, r.shape[0]).transpose(2, 0, 1)
    return out


def test_streaming_to_raster_host(container):
    r, tiles, streams, data = container
    got, index = streaming_to_raster(data, device=None, semantics="int")
    assert got.dtype == r.dtype and got.shape == r.shape
    assert np.array_equal(got, r)  # lossless for this range
    assert len(index["frames"]) == len(tiles) and index["tile_size"] == 128
    got16, _ = streaming_to_raster(data)  # default: flac_to_tiff's PCM_16 semantics
    assert np.array_equal(got16, _expected_pcm16(r, tiles, streams))
    with pytest.raises(ValueError):
        streaming_to_raster(data, semantics="float")


def test_streaming_to_raster_rejects_a_damaged_tile(container):
    _, _, _, data = container
    bad = bytearray(data)
    bad[len(bad) - 40] ^= 0x10
    with pytest.raises(N.NativeError):
        streaming_to_raster(bytes(bad), device=None)
    with pytest.raises(ValueError):
        streaming_to_raster(data[:-500], device=None)


def test_streaming_to_tiff_and_cli_convert_on_the_host(container, tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from flac_raster import cli

    r, tiles, streams, data = container
    src = tmp_path / "scene_streaming.flac"
    src.write_bytes(data)
    assert is_streaming_container(src)
    (tmp_path / "plain.flac").write_bytes(streams[0].data)
    assert not is_streaming_container(tmp_path / "plain.flac")
    want = _expected_pcm16(r, tiles, streams)

    out = tmp_path / "direct.tif"
    streaming_to_tiff(src, out, device=None)
    px, info = read_geotiff(out)
    assert np.array_equal(px, want)
    assert tuple(info.transform)[:6] == tuple(TRANSFORM)[:6] and "32633" in str(info.crs)

    monkeypatch.setattr(cli, "_gpu_present", lambda: False)  # the host path, wherever this runs
    out2 = tmp_path / "scene.tif"
    res = CliRunner().invoke(cli.app, ["convert", str(src), "-o", str(out2)])
    assert res.exit_code == 0, res.output
    px2, _ = read_geotiff(out2)
    assert np.array_equal(px2, want)
    # an existing output is still refused without --force
    res = CliRunner().invoke(cli.app, ["convert", str(src), "-o", str(out2)])
    assert res.exit_code == 1


def test_new_names_exported_and_declared():
    hdr = (ROOT / "include" / "flac_raster_amd.h").read_text()
    decl = set(re.findall(r"FRA_API\s+[^;(]*?\b(fra_\w+)\s*\(", hdr))
    L = N.load()
    for name in ("fra_decode_device", "fra_decode_device_timing"):
        assert name in decl and name in N.EXPORTS and hasattr(L, name)
    for macro, val in (("FRA_DENORM_NONE", N.DENORM_NONE), ("FRA_DENORM_INT", N.DENORM_INT),
                       ("FRA_DENORM_PCM16", N.DENORM_PCM16)):
        assert int(re.search(rf"#define {macro} (\d+)", hdr).group(1)) == val
    assert L.fra_abi_version() == 3
    # layout of the ctypes mirrors (LP64): the header's field order and natural alignment
    assert C.sizeof(N.DecodeItem) == 72 and N.DecodeItem.frame_offsets.offset == 48
    assert N.DecodeItem.window.offset == 16 and N.DecodeItem.nframes.offset == 56
    assert C.sizeof(N.DecodeJob) == 88 and N.DecodeJob.dst.offset == 40 and N.DecodeJob.band_stride.offset == 64
    assert hasattr(N.Context, "decode_device")


def test_decode_device_validates_arguments_without_a_gpu():
    """fra_decode_device checks its job before it touches the GPU: these fail the same way on any machine."""
    L = N.load()
    job = N.DecodeJob()
    infos = (N.Decoded * 1)()
    assert L.fra_decode_device(None, C.byref(job), infos) == -1
    assert b"null" in L.fra_last_error()


def test_decode_flac_host_unchanged(golden_dir):
    g = json.loads((golden_dir / "golden.json").read_text())
    data = (golden_dir / "sample_rgb.flac").read_bytes()
    x, sr, bps = decode_flac(data)
    assert (x.dtype, x.shape, sr, bps) == (np.int16, (65536, 3), 44100, 16)
    assert hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() == g["tiffs"]["sample_rgb.tif"]["audio_sha256"]
    y, _, _ = decode_flac(data, concat=False, device=None)
    assert np.array_equal(x, y)
    if N.device_count() == 0:
        with pytest.raises(N.NativeUnavailable):  # no silent host decode when a device is asked for
            decode_flac(data, device=0)
