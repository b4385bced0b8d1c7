"""What the source tests share (``test_sources_cpu.py``, ``test_gpu_sources.py``): one small raster as a streaming
container (a file and its bytes) and as the GeoTIFF written from the host read of that container, and every windowed
operation run over both.  A source is a source: the container function and the GeoTIFF function of an operation return
the same bytes, dtypes, shapes, reports and windows."""
import math
from types import SimpleNamespace

import numpy as np

from flac_raster.focal import Spec, slope_params
from flac_raster.geo import Affine
from flac_raster.proximity import Options
from flac_raster import streaming as S
from flac_raster.tiff import write_geotiff
from flac_raster.tiles import calculate_tiles
from oracle_tiles import oracle_encode_tiles

B, H, W, TILE = 3, 96, 130, 64  # 2 x 3 tiles, ragged right (2 columns) and bottom (32 rows)
TRANSFORM = Affine(10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
CRS = "EPSG:32633"
# no window, a window across the tile corners (64, 64) and (64, 128), and a bbox that hangs over the right edge: columns
# floor(30.3) .. ceil(140.2) clipped to 130, rows floor(20.5) .. ceil(79.6)
REQUESTS = {
    "whole": ({}, (0, 0, H, W)),
    "window": ({"window": (20, 30, 60, 90)}, (20, 30, 60, 90)),
    "bbox": ({"bbox": (500303.0, 4099204.0, 501402.0, 4099795.0)}, (20, 30, 60, 100)),
}
EXPRS = ["(b1-b2)/(b1+b2)", "b3*2+b1"]
FOCAL = Spec("mean", (3, 5))
# the output grid of the warp: the source's, turned by 20 degrees about a point inside it, at 1.25 times the pixel size
_c, _s = 12.5 * math.cos(math.radians(20.0)), 12.5 * math.sin(math.radians(20.0))
WARP_GRID = (_c, _s, 500200.0, _s, -_c, 4099900.0)
WARP_SHAPE = (61, 83)

# every (operation, case) that ``results`` runs
CASES = [(name, f"{rname}, {kind}") for name in ("calc", "focal", "focal of the pixel sizes", "stats", "zonal", "proximity")
         for rname in REQUESTS for kind in ("path", "bytes")]
CASES += [("warp", "whole, path"), ("warp", "whole, bytes")]
CASES += [(name, "the TIFF's nodata tag") for name in ("calc", "focal", "focal of the pixel sizes", "stats", "zonal", "warp")]


def terrain(dx, dy):
    """A focal spec as a function of the pixel sizes, as the terrain commands pass it."""
    return Spec("slope", 3, params=slope_params(1.0, dx, dy))


def build(tmp):
    """The fixture, its files under the directory ``tmp``."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.stack([(2000 + 90 * np.sin(yy / 9.0 + b) + 70 * np.cos(xx / 13.0) + rng.integers(0, 40, (H, W)))
                  for b in range(B)]).astype(np.uint16)
    r[2] = rng.choice([0, 500, 30000, 65535], (H, W), p=[0.88, 0.04, 0.04, 0.04])  # a few repeated values
    tiles = calculate_tiles(H, W, TILE)
    data = S.assemble_streaming(tiles, oracle_encode_tiles(r, tiles, level=5), r.shape, r.dtype, TRANSFORM, CRS, TILE)
    path = tmp / "scene_streaming.flac"
    path.write_bytes(data)
    plain, _ = S.streaming_to_raster(data, device=None)
    # the 16-bit round trip moves the values: the nodata value and the targets are taken from what the container gives
    vals, counts = np.unique(plain[2], return_counts=True)
    nodata = float(vals[np.argmax(counts)])
    targets = tuple(float(v) for v in vals[np.argsort(counts)][:3])
    tiff, tagged = tmp / "scene.tif", tmp / "scene_nodata.tif"
    write_geotiff(tiff, plain, transform=tuple(TRANSFORM)[:6], crs=CRS)
    write_geotiff(tagged, plain, transform=tuple(TRANSFORM)[:6], crs=CRS, nodata=int(nodata))
    zones = ((yy // 17) * 10 + xx // 23).astype(np.int32)
    plain.setflags(write=False)
    return SimpleNamespace(data=data, path=path, tiff=tiff, tagged=tagged, plain=plain, nodata=nodata, targets=targets,
                           zones=zones)


def same(a, b, where=""):
    """Exact equality of two results: arrays by dtype, shape and bytes, containers by element, numbers by value."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray), where
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{where}[{i}]")
    elif isinstance(a, float) and a != a:
        assert isinstance(b, float) and b != b, where
    else:
        assert type(a) is type(b) and a == b, f"{where}: {a!r} != {b!r}"


# One entry per operation: (what the container function returns, what the GeoTIFF function returns), each cut down to
# the part the two share -- the result, the report and the window, without the index or the RasterInfo.
def _calc(src, tiff, req, device, nodata):
    return (S.calc_window(src, EXPRS, nodata=nodata[0], device=device, **req)[:3],
            S.calc_tiff(tiff, EXPRS, nodata=nodata[1], device=device, **req)[:3])


def _focal(spec):
    def run(src, tiff, req, device, nodata):
        import dataclasses

        given = spec
        if nodata[0] is not None:  # the container stores no nodata value: its spec carries the tag's
            given = (lambda dx, dy: dataclasses.replace(spec(dx, dy), nodata=nodata[0])) if callable(spec) \
                else dataclasses.replace(spec, nodata=nodata[0])
        return (S.focal_window(src, given, device=device, **req)[:3], S.focal_tiff(tiff, spec, device=device, **req)[:3])
    return run


def _stats(src, tiff, req, device, nodata):
    return (S.container_stats(src, bins=32, hist_range=(0.0, 65536.0), nodata=nodata[0], device=device, **req)[:2],
            S.tiff_stats(tiff, bins=32, hist_range=(0.0, 65536.0), nodata=nodata[1], device=device, **req)[:2])


def _zonal(zones):
    def run(src, tiff, req, device, nodata):
        return (S.container_zonal(src, zones, nodata=nodata[0], device=device, **req)[:2],
                S.tiff_zonal(tiff, zones, nodata=nodata[1], device=device, **req)[:2])
    return run


def _proximity(targets):
    opts = Options(targets, max_dist=120.0, alloc_fill=7.0)

    def run(src, tiff, req, device, nodata):
        return (S.proximity_window(src, opts, units="geo", want_alloc=True, device=device, **req)[:4],
                S.proximity_tiff(tiff, opts, units="geo", want_alloc=True, device=device, **req)[:4])
    return run


def _warp(src, tiff, req, device, nodata):
    a = S.warp_window(src, WARP_GRID, WARP_SHAPE, resampling="cubic", nodata=nodata[0], device=device)
    b = S.warp_tiff(tiff, WARP_GRID, WARP_SHAPE, resampling="cubic", nodata=nodata[1], device=device)
    keys = ("grid_step", "grid_error", "source_window", "filled", "shares")
    return (a[:3] + ({k: a[3][k] for k in keys},), b[:3] + ({k: b[3][k] for k in keys},))


def operations(fix):
    """``name -> (run(src, tiff, request, device, (container nodata, tiff nodata)), takes a window, has the nodata
    default)``."""
    return {
        "calc": (_calc, True, True),
        "focal": (_focal(FOCAL), True, True),
        "focal of the pixel sizes": (_focal(terrain), True, True),
        "stats": (_stats, True, True),
        "zonal": (_zonal(fix.zones), True, True),
        "proximity": (_proximity(fix.targets), True, False),
        "warp": (_warp, False, True),
    }


def results(fix, device):
    """Every case once on ``device`` -> ``{(operation, case): (container result, GeoTIFF result)}``.  The cases: each
    request with the container as a path and as bytes, both given the same nodata value (the warp) or none; and, where
    an operation has the default, the GeoTIFF with a nodata tag called without a value against the container called
    with the tag's."""
    out = {}
    for name, (run, windowed, default) in operations(fix).items():
        explicit = (fix.nodata, fix.nodata) if name == "warp" else (None, None)
        for rname, (req, _) in REQUESTS.items():
            if not windowed and rname != "whole":
                continue
            for kind, src in (("path", fix.path), ("bytes", fix.data)):
                out[name, f"{rname}, {kind}"] = run(src, fix.tiff, req if windowed else {}, device, explicit)
        if default:
            req = REQUESTS["window"][0] if windowed else {}
            out[name, "the TIFF's nodata tag"] = run(fix.path, fix.tagged, req, device, (fix.nodata, None))
    return out


def check_windows(res):
    """The returned windows are the clipped requests (the warp returns none)."""
    for (name, case), (a, _) in res.items():
        if name != "warp":
            rname = case.split(",")[0] if "," in case else "window"
            assert tuple(a[-1]) == REQUESTS[rname][1], (name, case)
