"""``flac-raster`` command line (commands and options of the reference's ``cli.py``).

convert / info / extract / query / compare keep the reference's arguments (``cli.py:51-444``);
``convert`` adds ``--devices`` (comma-separated GPU ids) for the multi-GPU tile split.  Remote
inputs (http/s3/az/gs) are out of scope for this build and are rejected with a clear message.
"""

from __future__ import annotations

import json
import logging
import tempfile
from contextlib import contextmanager
from pathlib import Path
from typing import List, Optional

import typer
from rich.console import Console
from rich.logging import RichHandler
from rich.table import Table

from ._native import VerifyMismatch
from .compare import compare_tiffs, display_comparison_table
from .converter import RasterFLACConverter

app = typer.Typer(name="flac-raster",
                  help="Convert GeoTIFF raster data to/from FLAC format with spatial streaming support (MI355X).",
                  add_completion=False, no_args_is_help=True)
console = Console()
logging.basicConfig(level=logging.INFO, format="%(message)s", datefmt="[%X]",
                    handlers=[RichHandler(console=console, rich_tracebacks=True)])
logger = logging.getLogger("flac_raster")

_REMOTE = ("http://", "https://", "s3://", "az://", "gs://")


def _local(path: str) -> Path:
    if path.startswith(_REMOTE):
        raise typer.BadParameter("remote URLs are not supported by this build; download the file first")
    return Path(path)


def _devices(spec: Optional[str]) -> Optional[List[int]]:
    if not spec:
        return None
    return [int(x) for x in spec.split(",") if x.strip()]


def _gpu_present() -> bool:
    from . import _native

    try:
        return _native.device_count() > 0
    except Exception:
        return False


def _pick_device(device: Optional[int], cpu: bool = False) -> Optional[int]:
    """The given device, else device 0 when a GPU is present, else the host path; ``cpu``: the host path."""
    if cpu:
        return None
    return device if device is not None else (0 if _gpu_present() else None)


def _request_window(bbox: Optional[str], pixels: Optional[str]):
    """``(window, bbox)`` of ``--window`` and ``--bbox``, of which at most one may be given."""
    if bbox is not None and pixels is not None:
        console.print("[red]Error: give at most one of --bbox and --window[/red]")
        raise typer.Exit(1)
    box = [float(x.strip()) for x in bbox.split(",")] if bbox else None
    win = [int(x.strip()) for x in pixels.split(",")] if pixels else None
    return win, box


def _existing(*paths: Path):
    for p in paths:
        if not p.exists():
            console.print(f"[red]File not found: {p}[/red]")
            raise typer.Exit(1)


@contextmanager
def _failing(what: str):
    """The frame of a command: an exit passes; anything else is logged as ``what``, printed, and exits with 1."""
    try:
        yield
    except typer.Exit:
        raise
    except VerifyMismatch as e:  # convert --verify: reported by its first differing sample, without a traceback
        console.print(f"[red]Verify failed: tile {e.tile}, pixel row {e.pixel[0]} col {e.pixel[1]} band {e.pixel[2]}: "
                      f"expected sample {e.expected}, decoded {e.got} ({e.mismatches} samples differ in this tile, "
                      f"{e.bad_tiles} tile(s) differ)[/red]")
        raise typer.Exit(1)
    except Exception as e:
        logger.exception(what)
        console.print(f"[red]Error: {e}[/red]")
        raise typer.Exit(1)


@app.command()
def convert(
    input_file: str = typer.Argument(..., help="Input file (TIFF or FLAC)"),
    output_file: Optional[Path] = typer.Option(None, "--output", "-o", help="Output file path"),
    compression_level: int = typer.Option(5, "--compression", "-c", min=0, max=8, help="FLAC compression level"),
    spatial: bool = typer.Option(False, "--spatial", "-s", help="Enable spatial tiling for streaming"),
    tile_size: int = typer.Option(512, "--tile-size", "-t", help="Tile size in pixels (default: 512)"),
    streaming: bool = typer.Option(False, "--streaming", help="Streaming format (each tile is a complete FLAC)"),
    force: bool = typer.Option(False, "--force", "-f", help="Overwrite existing output file"),
    verbose: bool = typer.Option(False, "--verbose", "-v", help="Enable verbose logging"),
    devices: Optional[str] = typer.Option(None, "--devices", help="GPU ids to split tiles over, e.g. 0,1,2,3"),
    verify: bool = typer.Option(False, "--verify", help="TIFF to FLAC: decode every frame on the GPU and compare it "
                                                        "with the input before the output is written"),
):
    """Convert between TIFF and FLAC formats."""
    if verbose:
        logging.getLogger("flac_raster").setLevel(logging.DEBUG)
    with _failing("Conversion failed"):
        src = _local(input_file)
        if not src.exists():
            console.print(f"[red]Error: Input file does not exist: {src}[/red]")
            raise typer.Exit(1)
        suffix = src.suffix.lower()
        if suffix in (".tif", ".tiff"):
            direction, default_suffix = "tiff_to_flac", ".flac"
        elif suffix == ".flac":
            direction, default_suffix = "flac_to_tiff", ".tif"
        else:
            console.print(f"[red]Error: Unsupported format: {suffix}[/red]")
            raise typer.Exit(1)
        if output_file is None:
            output_file = (src.with_name(f"{src.stem}_streaming{default_suffix}") if streaming
                           else src.with_suffix(default_suffix))
        if output_file.exists() and not force:
            console.print(f"[red]Error: Output exists: {output_file}[/red]")
            raise typer.Exit(1)
        devs = _devices(devices)
        if verify and direction != "tiff_to_flac":
            console.print("[red]Error: --verify applies to TIFF -> FLAC conversions[/red]")
            raise typer.Exit(1)
        if streaming and direction == "tiff_to_flac":
            from .streaming import create_streaming_flac

            idx = create_streaming_flac(src, output_file, tile_size, compression_level, devs, verify=verify)
            console.print(f"[green]Created streaming FLAC: {output_file} ({len(idx['frames'])} tiles, "
                          f"{output_file.stat().st_size / 1024 / 1024:.2f} MB)[/green]")
            return
        if direction == "flac_to_tiff":
            from .streaming import is_streaming_container, streaming_to_tiff

            if is_streaming_container(src):
                dev = _pick_device(devs[0] if devs else None)  # the first of --devices
                idx = streaming_to_tiff(src, output_file, device=dev)
                console.print(f"[green]SUCCESS: Converted {len(idx['frames'])} tiles to TIFF: {output_file}[/green]")
                return
        conv = RasterFLACConverter(devices=devs)
        if direction == "tiff_to_flac":
            res = conv.tiff_to_flac(src, output_file, compression_level, spatial, tile_size, verify=verify)
            if spatial and res:
                console.print(f"[green]Created {len(res.frames)} spatial tiles[/green]")
        else:
            conv.flac_to_tiff(src, output_file)


@app.command()
def info(file_path: str = typer.Argument(..., help="File to inspect")):
    """Display information about a FLAC or TIFF file."""
    with _failing("Info failed"):
        p = _local(file_path)
        if not p.exists():
            console.print(f"[red]Error: File not found: {p}[/red]")
            raise typer.Exit(1)
        s = p.suffix.lower()
        if s in (".tif", ".tiff"):
            _show_tiff_info(p)
        elif s == ".flac":
            _show_flac_info(p)
        else:
            console.print(f"[red]Unsupported format: {s}[/red]")
            raise typer.Exit(1)


@app.command()
def extract(
    flac_file: str = typer.Argument(..., help="Streaming FLAC file"),
    output: Path = typer.Option(..., "--output", "-o", help="Output TIFF file path"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="Bounding box: 'xmin,ymin,xmax,ymax'"),
    tile_id: Optional[int] = typer.Option(None, "--tile-id", help="Extract specific tile by ID"),
    center: bool = typer.Option(False, "--center", help="Extract center tile"),
    last: bool = typer.Option(False, "--last", help="Extract last tile"),
):
    """Extract one tile of a streaming FLAC file to GeoTIFF."""
    from .streaming import open_streaming, read_tile_bytes, select_frame

    with _failing("Extraction failed"):
        path = _local(flac_file)
        sf = open_streaming(path)
        frames = sf.index["frames"]
        console.print(f"[green]Found {len(frames)} tiles[/green]")
        coords = [float(x.strip()) for x in bbox.split(",")] if bbox else None
        fr = select_frame(frames, tile_id=tile_id, bbox=coords, center=center, last=last)
        data = read_tile_bytes(path, fr, sf.header_size)
        with tempfile.NamedTemporaryFile(suffix=".flac", delete=False) as tmp:
            tmp.write(data)
            tmp_path = Path(tmp.name)
        try:
            RasterFLACConverter().flac_to_tiff(tmp_path, output)
        finally:
            tmp_path.unlink()
        total = sum(f["byte_size"] for f in frames)
        console.print(f"[green]Saved to: {output}[/green]")
        console.print(f"[blue]Bandwidth: {fr['byte_size'] / 1024:.1f} KB "
                      f"(saved {(1 - fr['byte_size'] / total) * 100:.1f}%)[/blue]")


def _print_nodata_shares(nodata, shares):
    """The share of output pixels that are nodata, per band (after a read with ``--nodata``)."""
    if nodata is not None:
        console.print(f"nodata {nodata:g}: " + ", ".join(f"band {b + 1} {100.0 * s:.2f} %" for b, s in enumerate(shares)))


@app.command()
def window(
    flac_file: str = typer.Argument(..., help="Streaming FLAC file"),
    output: Path = typer.Option(..., "--output", "-o", help="Output TIFF file path"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="Bounding box: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="Pixel window: 'row,col,height,width'"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
    decimate: int = typer.Option(1, "--decimate", help="Write the window at 1/K resolution: K = 2, 4, 8, 16, 32 or 64"),
    resampling: str = typer.Option("nearest", "--resampling", help="With --decimate: nearest or average; with "
                                   "--out-shape: nearest, average, bilinear or cubic"),
    out_shape: Optional[str] = typer.Option(None, "--out-shape", help="Write the window resampled to 'H,W' pixels"),
    nodata: Optional[float] = typer.Option(None, "--nodata", help="With --decimate or --out-shape: leave pixels of this "
                                           "value (and NaN) out of every result and tag the TIFF with it"),
):
    """Read a pixel window of a streaming FLAC file to GeoTIFF (only the tiles and frames it needs)."""
    from .streaming import window_to_tiff

    with _failing("Window read failed"):
        if (bbox is None) == (pixels is None):
            console.print("[red]Error: give exactly one of --bbox and --window[/red]")
            raise typer.Exit(1)
        win, box = _request_window(bbox, pixels)
        path = _local(flac_file)
        dev = _pick_device(device)
        shape = tuple(int(x.strip()) for x in out_shape.split(",")) if out_shape else None
        shares: list = []
        got, idx = window_to_tiff(path, output, window=win, bbox=box, device=dev, decimate=decimate,
                                  resampling=resampling, out_shape=shape, nodata=nodata, shares=shares)
        scale = f" at 1/{decimate} resolution ({resampling})" if decimate != 1 else ""
        if shape:
            scale = f" as {shape[0]} x {shape[1]} ({resampling})"
        console.print(f"[green]Saved rows {got[0]}..{got[0] + got[2]}, columns {got[1]}..{got[1] + got[3]} of "
                      f"{idx['height']} x {idx['width']}{scale} to: {output}[/green]")
        _print_nodata_shares(nodata, shares)


@app.command()
def overview(
    flac_file: str = typer.Argument(..., help="Streaming FLAC file"),
    output: Path = typer.Option(..., "--output", "-o", help="Output TIFF file path"),
    factor: Optional[int] = typer.Option(None, "--factor", help="Write the raster at 1/K resolution: K = 2, 4, 8, 16, "
                                         "32 or 64"),
    resampling: str = typer.Option("average", "--resampling", help="nearest or average; with --size also bilinear "
                                   "or cubic"),
    size: Optional[int] = typer.Option(None, "--size", help="Write the raster with its longest side N pixels"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
    nodata: Optional[float] = typer.Option(None, "--nodata", help="Leave pixels of this value (and NaN) out of every "
                                           "result and tag the TIFF with it"),
):
    """Write a reduced-resolution preview of a whole streaming FLAC file to GeoTIFF."""
    from .streaming import overview_to_tiff

    with _failing("Overview failed"):
        path = _local(flac_file)
        dev = _pick_device(device)
        if (factor is None) == (size is None):
            console.print("[red]Error: give exactly one of --factor and --size[/red]")
            raise typer.Exit(1)
        shares: list = []
        shape, idx = overview_to_tiff(path, output, factor, resampling, device=dev, max_size=size, nodata=nodata,
                                      shares=shares)
        how = f"at 1/{factor} resolution" if size is None else f"with longest side {size}"
        console.print(f"[green]Saved {idx['height']} x {idx['width']} {how} ({resampling}) as "
                      f"{shape[1]} x {shape[2]} to: {output}[/green]")
        _print_nodata_shares(nodata, shares)


@app.command()
def query(
    flac_file: str = typer.Argument(..., help="Spatial FLAC file"),
    bbox: str = typer.Option(..., "--bbox", "-b", help="Bounding box: 'xmin,ymin,xmax,ymax'"),
    output: Optional[Path] = typer.Option(None, "--output", "-o", help="Save byte ranges to JSON file"),
):
    """Byte ranges of the tiles of a spatial FLAC file that intersect a bbox."""
    from .spatial_encoder import SpatialFLACStreamer

    with _failing("Query failed"):
        coords = tuple(float(x.strip()) for x in bbox.split(","))
        if len(coords) != 4:
            console.print("[red]Bbox must have 4 coordinates[/red]")
            raise typer.Exit(1)
        ranges = SpatialFLACStreamer(_local(flac_file)).get_byte_ranges_for_bbox(coords)
        total = sum(e - s + 1 for s, e in ranges)
        t = Table(title=f"Byte Ranges for bbox {bbox}")
        for name, style in (("#", "cyan"), ("Start", "green"), ("End", "yellow"), ("Size", "blue"),
                            ("Range Header", "magenta")):
            t.add_column(name, style=style)
        for i, (s, e) in enumerate(ranges, 1):
            t.add_row(str(i), f"{s:,}", f"{e:,}", f"{e - s + 1:,}", f"bytes={s}-{e}")
        console.print(t)
        console.print(f"[bold]Total: {total:,} bytes ({len(ranges)} ranges)[/bold]")
        if output:
            output.write_text(json.dumps({"bbox": list(coords), "ranges": [{"start": s, "end": e} for s, e in ranges],
                                          "total_bytes": total}, indent=2))


@app.command()
def compare(
    file1: Path = typer.Argument(..., help="First TIFF file"),
    file2: Path = typer.Argument(..., help="Second TIFF file"),
    show_bands: bool = typer.Option(True, "--show-bands/--no-bands", help="Show per-band statistics"),
    export_json: Optional[Path] = typer.Option(None, "--export", "-e", help="Export comparison to JSON"),
):
    """Compare two TIFF files."""
    for f in (file1, file2):
        if not f.exists():
            console.print(f"[red]File not found: {f}[/red]")
            raise typer.Exit(1)
        if f.suffix.lower() not in (".tif", ".tiff"):
            console.print(f"[red]Not a TIFF file: {f}[/red]")
            raise typer.Exit(1)
    res = compare_tiffs(file1, file2, show_bands)
    display_comparison_table(res)
    if export_json:
        export_json.write_text(json.dumps(res, indent=2, default=list))


@app.command()
def check(
    source: Path = typer.Argument(..., help="Source TIFF file"),
    flac_file: str = typer.Argument(..., help="Streaming FLAC file made from it"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="Compare this bounding box only: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="Compare this pixel window only: 'row,col,height,width'"),
    semantics: str = typer.Option("pcm16", "--semantics", help="pcm16 (what convert back to TIFF gives) or int"),
    max_diff: Optional[float] = typer.Option(None, "--max-diff", help="Accept differences up to this absolute value"),
    export_json: Optional[Path] = typer.Option(None, "--export", "-e", help="Export the comparison to JSON"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """Does a streaming FLAC file give its source TIFF back, and if not, by how much (exit 0: it does)."""
    from .compare import display_first_differences
    from .streaming import check_against_tiff

    with _failing("Check failed"):
        win, box = _request_window(bbox, pixels)
        _existing(source)
        path = _local(flac_file)
        dev = _pick_device(device)
        res, got, _ = check_against_tiff(path, source, window=win, bbox=box, device=dev, semantics=semantics,
                                         count_one_sided_nans=max_diff is not None)
        display_comparison_table(res)
        display_first_differences(res)
        if max_diff is None:
            ok = res["arrays_equal"]
        else:  # a pixel with a NaN on one side only differs by no number: it is never within a tolerance
            ok = res["max_difference"] <= max_diff and res["one_sided_nan"] == 0
        res["max_diff_allowed"], res["passed"] = max_diff, bool(ok)
        if export_json:
            export_json.write_text(json.dumps(res, indent=2, default=list))
        where = f"rows {got[0]}..{got[0] + got[2]}, columns {got[1]}..{got[1] + got[3]}"
        if ok:
            console.print(f"[green]{path.name} gives {source.name} back ({where}, {semantics}"
                          + (f", differences up to {res['max_difference']:g} <= {max_diff:g}" if max_diff is not None
                             and not res["arrays_equal"] else "") + ")[/green]")
        else:
            console.print(f"[red]{path.name} differs from {source.name} in {res['differing']} pixel values ({where}, "
                          f"{semantics}, largest difference {res['max_difference']:g})[/red]")
            raise typer.Exit(1)


@app.command()
def stats(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="This bounding box only: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="This pixel window only: 'row,col,height,width'"),
    bins: Optional[int] = typer.Option(None, "--bins", help="Histogram bins, 0 ... 65536 (default: the exact value "
                                       "histogram for dtypes of at most 16 bits, else 256)"),
    hist_range: Optional[str] = typer.Option(None, "--range", help="Histogram range 'lo,hi' (default: each band's finite "
                                             "minimum and maximum)"),
    nodata: Optional[float] = typer.Option(None, "--nodata", help="Nodata value (default: the TIFF's own tag)"),
    percentiles: str = typer.Option("2,50,98", "--percentiles", help="Percentiles to print, from the histogram"),
    semantics: str = typer.Option("pcm16", "--semantics", help="Container pixels: pcm16 (what convert back gives) or int"),
    export_json: Optional[Path] = typer.Option(None, "--export", "-e", help="Export the full report to JSON"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """Band statistics, histogram and percentiles of a streaming FLAC file or a GeoTIFF."""
    from .stats import display_stats_table, exact_range, percentile
    from .source import open_source
    from .streaming import container_stats, tiff_stats

    with _failing("Statistics failed"):
        win, box = _request_window(bbox, pixels)
        path = _local(file_path)
        _existing(path)
        qs = [float(x.strip()) for x in percentiles.split(",") if x.strip()]
        try:
            src = open_source(path)
        except ValueError as e:  # neither a container nor a GeoTIFF: a refusal, not a failure to log
            console.print(f"[red]Error: {e}[/red]")
            raise typer.Exit(1)
        dt = src.dtype
        rng = tuple(float(x.strip()) for x in hist_range.split(",")) if hist_range else None
        if rng is not None and len(rng) != 2:
            console.print("[red]Error: --range takes 'lo,hi'[/red]")
            raise typer.Exit(1)
        if bins is None and rng is None and dt.kind in "iu" and dt.itemsize <= 2:
            lo, hi, bins = exact_range(dt)  # bin i holds exactly the value lo + i: exact percentiles
            rng = (lo, hi)
        elif bins is None:
            bins = 256
        dev = _pick_device(device)
        if src.encoded:
            bands, got, _ = container_stats(path, window=win, bbox=box, bins=bins, hist_range=rng, nodata=nodata,
                                            device=dev, semantics=semantics)
        else:
            bands, got, _ = tiff_stats(path, window=win, bbox=box, bins=bins, hist_range=rng, nodata=nodata, device=dev)
        display_stats_table(bands, qs, title=f"{path.name}: rows {got[0]}..{got[0] + got[2]}, columns "
                                             f"{got[1]}..{got[1] + got[3]} ({dt})")
        if export_json:
            for b in bands:
                b["percentiles"] = {f"{q:g}": percentile(b, q) for q in qs}
            export_json.write_text(json.dumps({"file": path.name, "dtype": str(dt), "window": list(got),
                                               "semantics": semantics if src.encoded else None,
                                               "device": dev, "bands": bands}, indent=2))


@app.command()
def zonal(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF"),
    zones: Path = typer.Option(..., "--zones", "-z", help="Single-band integer GeoTIFF of the same shape: the zones; or "
                               "a GeoJSON file (.geojson, .json) of polygons in the source's CRS"),
    attribute: Optional[str] = typer.Option(None, "--attribute", "-a", help="With GeoJSON zones: the integer property "
                                            "that names a feature's zone (default: feature i is zone i + 1)"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="This bounding box only: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="This pixel window only: 'row,col,height,width'"),
    nodata: Optional[float] = typer.Option(None, "--nodata", help="Nodata value (default: a source TIFF's own tag)"),
    ignore: Optional[int] = typer.Option(None, "--ignore", help="Zone label to leave out (default: the zones TIFF's "
                                         "nodata tag)"),
    zones_regions: bool = typer.Option(False, "--zones-regions", help="The zones are the connected components of --zones, "
                                       "a single-band raster on the same grid (a streaming FLAC file or a GeoTIFF)"),
    connectivity: int = typer.Option(4, "--connectivity", help="With --zones-regions: 4 or 8"),
    min_size: int = typer.Option(1, "--min-size", help="With --zones-regions: drop components of fewer pixels"),
    values: Optional[str] = typer.Option(None, "--values", help="With --zones-regions: the foreground values, e.g. '1,2' "
                                         "(default: every pixel that is non-zero and not NaN)"),
    invert: bool = typer.Option(False, "--invert", help="With --zones-regions: swap foreground and background"),
    by_value: bool = typer.Option(False, "--by-value", help="With --zones-regions: link only neighbours of equal value"),
    semantics: str = typer.Option("pcm16", "--semantics", help="Container pixels: pcm16 (what convert back gives) or int"),
    export: Optional[Path] = typer.Option(None, "--export", "-e", help="Export the full report to .json or .csv"),
    cpu: bool = typer.Option(False, "--cpu", help="Decode and reduce on the host (numpy)"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """Per-zone band statistics of a streaming FLAC file or a GeoTIFF over the zones of a GeoTIFF, the polygons of a
    GeoJSON file or the connected components of a mask."""
    from .streaming import zonal_of_regions, zonal_with_polygons, zonal_with_tiff
    from .zonal import display_zonal_table, export_report

    with _failing("Zonal statistics failed"):
        win, box = _request_window(bbox, pixels)
        path = _local(file_path)
        _existing(path, zones)
        if export is not None and export.suffix.lower() not in (".json", ".csv"):
            console.print("[red]Error: --export takes a .json or a .csv file[/red]")
            raise typer.Exit(1)
        dev = _pick_device(device, cpu)
        if zones_regions:
            from .regions import Options as RegionOptions

            if ignore is not None or attribute is not None:
                console.print("[red]Error: --ignore and --attribute do not go with --zones-regions[/red]")
                raise typer.Exit(1)
            ropts = RegionOptions(_float_list(values), invert, by_value, connectivity, min_size)
            report, got, _, rcounts = zonal_of_regions(path, zones, ropts, window=win, bbox=box, nodata=nodata, device=dev,
                                                       semantics=semantics)
            console.print(f"zones: {int(rcounts[0, 2])} components of {zones.name} ({int(rcounts[0, 1])} before the sieve)")
        elif zones.suffix.lower() in (".geojson", ".json"):
            if ignore is not None:
                console.print("[red]Error: --ignore goes with a zones GeoTIFF: polygons leave the pixels outside them "
                              "out already[/red]")
                raise typer.Exit(1)
            report, got, _ = zonal_with_polygons(path, zones, attribute=attribute, window=win, bbox=box, nodata=nodata,
                                                 device=dev, semantics=semantics)
        else:
            if attribute is not None:
                console.print("[red]Error: --attribute goes with GeoJSON zones[/red]")
                raise typer.Exit(1)
            report, got, _ = zonal_with_tiff(path, zones, window=win, bbox=box, nodata=nodata, ignore=ignore, device=dev,
                                             semantics=semantics)
        display_zonal_table(report, title=f"{path.name} by {zones.name}: rows {got[0]}..{got[0] + got[2]}, columns "
                                          f"{got[1]}..{got[1] + got[3]}")
        if export is not None:
            export_report(export, report, {"file": path.name, "zones": zones.name, "window": list(got), "device": dev})


@app.command()
def rasterize(
    shapes: Path = typer.Argument(..., help="GeoJSON file of polygons, in the CRS of --like"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF (one band)"),
    like: Path = typer.Option(..., "--like", help="Streaming FLAC file or GeoTIFF whose grid the output takes"),
    attribute: Optional[str] = typer.Option(None, "--attribute", "-a", help="Burn this integer property of every feature "
                                            "(default: feature i burns i + 1)"),
    burn: Optional[int] = typer.Option(None, "--burn", help="Burn this value for every feature"),
    fill: int = typer.Option(0, "--fill", help="What a pixel outside every polygon gets; the output's nodata tag"),
    dtype: Optional[str] = typer.Option(None, "--dtype", help="uint8, int8, uint16, int16, uint32 or int32 (default: the "
                                        "narrowest that holds the values)"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="This bounding box only: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="This pixel window only: 'row,col,height,width'"),
    cpu: bool = typer.Option(False, "--cpu", help="Rasterize with numpy on the host"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """Polygons of a GeoJSON file burned onto the grid of a streaming FLAC file or a GeoTIFF -> GeoTIFF."""
    from .streaming import rasterize_to_tiff

    with _failing("Rasterizing failed"):
        win, box = _request_window(bbox, pixels)
        if attribute is not None and burn is not None:
            console.print("[red]Error: give at most one of --attribute and --burn[/red]")
            raise typer.Exit(1)
        _existing(shapes, like)
        dev = _pick_device(device, cpu)
        got, burned, dt = rasterize_to_tiff(like, shapes, output_path, attribute=attribute, burn=burn, window=win, bbox=box,
                                            fill=fill, dtype=dtype, device=dev)
        console.print(f"[green]{output_path}[/green]: {dt}, rows {got[0]}..{got[0] + got[2]}, columns {got[1]}.."
                      f"{got[1] + got[3]}" + (f" (GPU {dev})" if dev is not None else " (host)"))
        console.print(f"burned: {burned} pixels, {100.0 * burned / (got[2] * got[3]):.2f}% of the window")


@app.command()
def proximity(
    file_path: str = typer.Argument(..., help="Streaming FLAC file, GeoTIFF, or (with --like) a GeoJSON file of polygons"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF of the distances"),
    values: Optional[str] = typer.Option(None, "--values", help="Target pixel values, e.g. '1,2' (default: every pixel "
                                         "that is non-zero and not NaN)"),
    max_dist: Optional[float] = typer.Option(None, "--max-dist", help="Pixels farther than this get the fill, in --units"),
    units: str = typer.Option("pixel", "--units", help="pixel, or geo: the map units of the source's transform"),
    fixed: Optional[float] = typer.Option(None, "--fixed", help="Write this value instead of the distance to every pixel "
                                          "within reach, the targets included (a buffer)"),
    fill: Optional[float] = typer.Option(None, "--fill", help="What a pixel out of reach gets, and the nodata tag "
                                         "(default: NaN for float outputs, the maximum for integer ones)"),
    dtype: str = typer.Option("float32", "--dtype", help="Output dtype of the distances"),
    alloc: Optional[Path] = typer.Option(None, "--alloc", help="Also write the value of the nearest target to this GeoTIFF"),
    alloc_fill: float = typer.Option(0.0, "--alloc-fill", help="What a pixel out of reach gets in --alloc"),
    like: Optional[Path] = typer.Option(None, "--like", help="With a GeoJSON source: the streaming FLAC file or GeoTIFF "
                                        "whose grid the polygons are burned on"),
    attribute: Optional[str] = typer.Option(None, "--attribute", "-a", help="With --like: this integer property is a "
                                            "polygon's label (default: feature i has i + 1)"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="This bounding box only: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="This pixel window only: 'row,col,height,width' "
                                         "(targets outside it still count)"),
    cpu: bool = typer.Option(False, "--cpu", help="Evaluate with numpy on the host"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """Distance of every pixel to the nearest target pixel (or polygon), and the nearest target's value -> GeoTIFF."""
    import numpy as np

    from .proximity import Options
    from .streaming import proximity_of_polygons_to_tiff, proximity_to_tiff

    with _failing("Proximity failed"):
        win, box = _request_window(bbox, pixels)
        if attribute is not None and like is None:
            console.print("[red]Error: --attribute goes with a GeoJSON source and --like[/red]")
            raise typer.Exit(1)
        path = _local(file_path)
        _existing(path)
        if like is not None:
            _existing(like)
        vals = tuple(float(x.strip()) for x in values.split(",")) if values else ()
        dev = _pick_device(device, cpu)
        odt = np.dtype(dtype)
        opts = Options(values=vals, max_dist=max_dist, fixed=fixed, fill=fill, alloc_fill=alloc_fill)
        if like is not None:
            got, counts = proximity_of_polygons_to_tiff(like, path, output_path, attribute, opts, window=win, bbox=box,
                                                        units=units, dist_dtype=odt, alloc_path=alloc, device=dev)
        else:
            got, counts = proximity_to_tiff(path, output_path, opts, window=win, bbox=box, units=units, dist_dtype=odt,
                                            alloc_path=alloc, device=dev)
        n = int(counts[1]) + int(counts[2])
        console.print(f"[green]{output_path}[/green]: {odt}, rows {got[0]}..{got[0] + got[2]}, columns {got[1]}.."
                      f"{got[1] + got[3]}" + (f" (GPU {dev})" if dev is not None else " (host)"))
        console.print(f"targets: {int(counts[0])}; within reach: {100.0 * int(counts[1]) / max(1, n):.2f}% of the pixels")


def _float_list(values: Optional[str]):
    return tuple(float(x.strip()) for x in values.split(",")) if values else ()


def _print_region_counts(counts):
    for b, (fg, ncomp, kept, px) in enumerate(counts.tolist()):
        console.print(f"band {b + 1}: {fg} foreground pixels, {ncomp} components, {kept} kept with {px} pixels")


@app.command()
def regions(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF of the labels (nodata 0)"),
    values: Optional[str] = typer.Option(None, "--values", help="Foreground pixel values, e.g. '1,2' (default: every "
                                         "pixel that is non-zero and not NaN)"),
    invert: bool = typer.Option(False, "--invert", help="Swap foreground and background (a NaN stays background)"),
    by_value: bool = typer.Option(False, "--by-value", help="Link only neighbours of equal value: regions of one class"),
    connectivity: int = typer.Option(4, "--connectivity", help="4 or 8"),
    min_size: int = typer.Option(1, "--min-size", help="Drop components of fewer pixels"),
    area: Optional[Path] = typer.Option(None, "--area", help="Also write every pixel's component area to this GeoTIFF"),
    export: Optional[Path] = typer.Option(None, "--export", "-e", help="Export a row per band and component (label, "
                                          "value, area, box, first pixel) to .json or .csv"),
    dtype: str = typer.Option("int32", "--dtype", help="Dtype of the labels: uint8, int8, uint16, int16, uint32 or int32"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="This bounding box only: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="This pixel window only: 'row,col,height,width' "
                                         "(a component is cut at the window's edge)"),
    semantics: str = typer.Option("pcm16", "--semantics", help="Container pixels: pcm16 (what convert back gives) or int"),
    cpu: bool = typer.Option(False, "--cpu", help="Label with numpy on the host"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """Connected components of a streaming FLAC file or a GeoTIFF -> a GeoTIFF of labels, numbered in the order of the
    components' first pixels."""
    from .regions import Options
    from .streaming import regions_to_tiff

    with _failing("Regions failed"):
        win, box = _request_window(bbox, pixels)
        path = _local(file_path)
        _existing(path)
        if export is not None and export.suffix.lower() not in (".json", ".csv"):
            console.print("[red]Error: --export takes a .json or a .csv file[/red]")
            raise typer.Exit(1)
        dev = _pick_device(device, cpu)
        opts = Options(_float_list(values), invert, by_value, connectivity, min_size)
        got, counts = regions_to_tiff(path, output_path, opts, window=win, bbox=box, label_dtype=dtype, area_path=area,
                                      export_path=export, device=dev, semantics=semantics)
        console.print(f"[green]{output_path}[/green]: {dtype}, rows {got[0]}..{got[0] + got[2]}, columns {got[1]}.."
                      f"{got[1] + got[3]}" + (f" (GPU {dev})" if dev is not None else " (host)"))
        _print_region_counts(counts)


@app.command()
def sieve(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF: the source without its small components"),
    min_size: int = typer.Option(..., "--min-size", help="Components of fewer pixels are replaced by --fill"),
    connectivity: int = typer.Option(4, "--connectivity", help="4 or 8"),
    any_value: bool = typer.Option(False, "--any-value", help="Link neighbouring foreground pixels whatever their values "
                                   "(default: only equal values, regions of one class)"),
    values: Optional[str] = typer.Option(None, "--values", help="Foreground pixel values (default: non-zero, not NaN)"),
    invert: bool = typer.Option(False, "--invert", help="Swap foreground and background"),
    fill: float = typer.Option(0.0, "--fill", help="What the pixels of removed components get; the output's nodata tag"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="This bounding box only: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="This pixel window only: 'row,col,height,width'"),
    semantics: str = typer.Option("pcm16", "--semantics", help="Container pixels: pcm16 (what convert back gives) or int"),
    cpu: bool = typer.Option(False, "--cpu", help="Label with numpy on the host"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """Remove the connected components of fewer than --min-size pixels (filled, not merged into a neighbour)."""
    from .streaming import sieve_to_tiff

    with _failing("Sieve failed"):
        win, box = _request_window(bbox, pixels)
        path = _local(file_path)
        _existing(path)
        dev = _pick_device(device, cpu)
        got, counts = sieve_to_tiff(path, output_path, min_size, connectivity, not any_value, _float_list(values), invert,
                                    fill, window=win, bbox=box, device=dev, semantics=semantics)
        console.print(f"[green]{output_path}[/green]: rows {got[0]}..{got[0] + got[2]}, columns {got[1]}.."
                      f"{got[1] + got[3]}" + (f" (GPU {dev})" if dev is not None else " (host)"))
        _print_region_counts(counts)


@app.command()
def calc(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF"),
    expr: List[str] = typer.Option(..., "--expr", "-e", help="Expression over b1 ... bN, e.g. '(b4-b3)/(b4+b3)'; "
                                   "one per output band"),
    bbox: Optional[str] = typer.Option(None, "--bbox", "-b", help="This bounding box only: 'xmin,ymin,xmax,ymax'"),
    pixels: Optional[str] = typer.Option(None, "--window", "-w", help="This pixel window only: 'row,col,height,width'"),
    dtype: str = typer.Option("float32", "--dtype", help="Output dtype"),
    nodata: Optional[float] = typer.Option(None, "--nodata", help="Nodata value of the source (default: the TIFF's own "
                                           "tag): pixels that hold it in a band the expressions read are left out"),
    fill: Optional[float] = typer.Option(None, "--fill", help="What a left-out pixel gets (default: NaN for float "
                                         "outputs, 0 for integer ones)"),
    cpu: bool = typer.Option(False, "--cpu", help="Evaluate with numpy on the host"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """Band math: per-pixel expressions over the bands of a streaming FLAC file or a GeoTIFF -> GeoTIFF."""
    import numpy as np

    from .streaming import calc_to_tiff

    with _failing("Band math failed"):
        win, box = _request_window(bbox, pixels)
        path = _local(file_path)
        _existing(path)
        dev = _pick_device(device, cpu)
        got, left, n = calc_to_tiff(path, output_path, list(expr), window=win, bbox=box, out_dtype=np.dtype(dtype),
                                    nodata=nodata, fill=fill, device=dev)
        console.print(f"[green]{output_path}[/green]: {len(expr)} band(s) of {np.dtype(dtype)}, rows {got[0]}.."
                      f"{got[0] + got[2]}, columns {got[1]}..{got[1] + got[3]}"
                      + (f" (GPU {dev})" if dev is not None else " (host)"))
        if nodata is not None or int(left[0]):
            console.print("left out: " + ", ".join(f"band {k + 1}: {100.0 * int(v) / max(1, n):.2f}%"
                                                   for k, v in enumerate(left)))


def _run_focal(what: str, file_path: str, output_path: Path, spec, bbox, pixels, dtype: str, cpu: bool, device):
    """The three focal commands from their spec (a ``focal.Spec`` or a function of the pixel sizes) on."""
    import numpy as np

    from .streaming import focal_to_tiff

    with _failing("Focal operation failed"):
        win, box = _request_window(bbox, pixels)
        path = _local(file_path)
        _existing(path)
        dev = _pick_device(device, cpu)
        got, left, n = focal_to_tiff(path, output_path, spec(), window=win, bbox=box, out_dtype=np.dtype(dtype), device=dev)
        console.print(f"[green]{output_path}[/green]: {what}, {len(left)} band(s) of {np.dtype(dtype)}, rows {got[0]}.."
                      f"{got[0] + got[2]}, columns {got[1]}..{got[1] + got[3]}"
                      + (f" (GPU {dev})" if dev is not None else " (host)"))
        console.print("left out: " + ", ".join(f"band {k + 1}: {100.0 * int(v) / max(1, n):.2f}%"
                                               for k, v in enumerate(left)))


_F_BBOX = typer.Option(None, "--bbox", "-b", help="This bounding box only: 'xmin,ymin,xmax,ymax'")
_F_WINDOW = typer.Option(None, "--window", "-w", help="This pixel window only: 'row,col,height,width' (neighbours "
                         "outside it are still read)")
_F_EDGE = typer.Option("skip", "--edge", help="Taps outside the raster: skip (left out) or clamp (the nearest pixel)")
_F_NODATA = typer.Option(None, "--nodata", help="Nodata value of the source (default: the TIFF's own tag): taps that "
                         "hold it are left out")
_F_FILL = typer.Option(None, "--fill", help="What a pixel without a result gets (default: NaN for float outputs, 0 for "
                       "integer ones)")
_F_KEEP = typer.Option(False, "--keep-mask", help="A pixel that is itself nodata or NaN gets the fill")
_F_CPU = typer.Option(False, "--cpu", help="Evaluate with numpy on the host")
_F_DEVICE = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)")


@app.command()
def focal(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF"),
    op: Optional[str] = typer.Option(None, "--op", help="mean, sum, min, max, count or median over the window"),
    size: str = typer.Option("3", "--size", help="Window: one odd number 1 ... 15, or 'HEIGHTxWIDTH' (median: at most "
                             "25 pixels)"),
    kernel: Optional[str] = typer.Option(None, "--kernel", help="Convolution weights, rows separated by ';': "
                                         "'0,-1,0;-1,4,-1;0,-1,0'"),
    normalize: bool = typer.Option(False, "--normalize", help="Divide a convolution by the sum of the weights used"),
    bbox: Optional[str] = _F_BBOX, pixels: Optional[str] = _F_WINDOW, edge: str = _F_EDGE,
    nodata: Optional[float] = _F_NODATA, fill: Optional[float] = _F_FILL, keep_mask: bool = _F_KEEP,
    dtype: str = typer.Option("float32", "--dtype", help="Output dtype"),
    cpu: bool = _F_CPU, device: Optional[int] = _F_DEVICE,
):
    """Focal statistics (--op) or a convolution (--kernel) over a streaming FLAC file or a GeoTIFF -> GeoTIFF."""
    from .focal import Spec

    def spec():
        if (op is None) == (kernel is None):
            raise ValueError("give exactly one of --op and --kernel")
        if kernel is not None:
            rows = [[float(v) for v in row.split(",")] for row in kernel.split(";")]
            if len({len(r) for r in rows}) != 1:
                raise ValueError("--kernel: every row needs the same number of weights")
            return Spec("convolve", (len(rows), len(rows[0])), edge, nodata, fill, normalize, keep_mask, rows)
        if op.lower() not in ("mean", "sum", "min", "max", "count", "median"):
            raise ValueError(f"--op: {op!r} is none of mean, sum, min, max, count, median")
        kh, _, kw = size.lower().partition("x")
        return Spec(op, (int(kh), int(kw or kh)), edge, nodata, fill, normalize, keep_mask)

    _run_focal(f"{op or 'convolution'} {size if kernel is None else ''}".strip(), file_path, output_path, spec, bbox,
               pixels, dtype, cpu, device)


@app.command()
def hillshade(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF holding elevations"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF"),
    azimuth: float = typer.Option(315.0, "--azimuth", help="Direction of the light, degrees clockwise from north"),
    altitude: float = typer.Option(45.0, "--altitude", help="Height of the light above the horizon, degrees"),
    z_factor: float = typer.Option(1.0, "--z-factor", help="Vertical exaggeration"),
    scale_xy: float = typer.Option(1.0, "--scale-xy", help="Ground units per elevation unit (111120 for degrees and "
                                   "metres)"),
    scale: float = typer.Option(255.0, "--scale", help="Value of a fully lit pixel"),
    bbox: Optional[str] = _F_BBOX, pixels: Optional[str] = _F_WINDOW, edge: str = _F_EDGE,
    nodata: Optional[float] = _F_NODATA, fill: Optional[float] = _F_FILL, keep_mask: bool = _F_KEEP,
    dtype: str = typer.Option("uint8", "--dtype", help="Output dtype"),
    cpu: bool = _F_CPU, device: Optional[int] = _F_DEVICE,
):
    """Hillshade (Horn's gradient) of a streaming FLAC file or a GeoTIFF -> GeoTIFF."""
    from .focal import Spec, hillshade_params

    def spec():
        return lambda dx, dy: Spec("hillshade", 3, edge, nodata, fill, False, keep_mask, None,
                                   hillshade_params(azimuth, altitude, z_factor, dx * scale_xy, dy * scale_xy, scale))

    _run_focal("hillshade", file_path, output_path, spec, bbox, pixels, dtype, cpu, device)


@app.command()
def slope(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF holding elevations"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF"),
    percent: bool = typer.Option(False, "--percent", help="Percent instead of rise over run"),
    z_factor: float = typer.Option(1.0, "--z-factor", help="Vertical exaggeration"),
    scale_xy: float = typer.Option(1.0, "--scale-xy", help="Ground units per elevation unit"),
    bbox: Optional[str] = _F_BBOX, pixels: Optional[str] = _F_WINDOW, edge: str = _F_EDGE,
    nodata: Optional[float] = _F_NODATA, fill: Optional[float] = _F_FILL, keep_mask: bool = _F_KEEP,
    dtype: str = typer.Option("float32", "--dtype", help="Output dtype"),
    cpu: bool = _F_CPU, device: Optional[int] = _F_DEVICE,
):
    """Slope (Horn's gradient, rise over run or percent) of a streaming FLAC file or a GeoTIFF -> GeoTIFF."""
    from .focal import Spec, slope_params

    def spec():
        return lambda dx, dy: Spec("slope", 3, edge, nodata, fill, False, keep_mask, None,
                                   slope_params(z_factor, dx * scale_xy, dy * scale_xy, 100.0 if percent else 1.0))

    _run_focal("slope", file_path, output_path, spec, bbox, pixels, dtype, cpu, device)


def _numbers(text: str, n: int, what: str, kind=float):
    try:
        vals = [kind(x.strip()) for x in text.split(",")]
    except ValueError:
        vals = []
    if len(vals) != n:
        raise ValueError(f"{what} takes {n} comma-separated numbers, got {text!r}")
    return vals


@app.command()
def warp(
    file_path: str = typer.Argument(..., help="Streaming FLAC file or GeoTIFF"),
    output_path: Path = typer.Option(..., "--output", "-o", help="Output GeoTIFF"),
    dst_crs: Optional[str] = typer.Option(None, "--dst-crs", help="Reproject to this CRS (EPSG:4326, EPSG:3857, WGS84 UTM)"),
    res: Optional[float] = typer.Option(None, "--res", help="With --dst-crs: the output pixel size"),
    size: Optional[str] = typer.Option(None, "--size", help="With --dst-crs: the output size 'HEIGHT,WIDTH'"),
    bounds: Optional[str] = typer.Option(None, "--bounds", help="With --dst-crs: 'xmin,ymin,xmax,ymax' in that CRS"),
    like: Optional[Path] = typer.Option(None, "--like", help="Onto the grid of this GeoTIFF: its transform, shape and CRS"),
    transform: Optional[str] = typer.Option(None, "--transform", help="Onto this geotransform 'a,b,c,d,e,f' in the "
                                            "source's CRS, with --out-shape"),
    out_shape: Optional[str] = typer.Option(None, "--out-shape", help="With --transform: 'HEIGHT,WIDTH'"),
    resampling: str = typer.Option("bilinear", "--resampling", help="nearest, bilinear or cubic"),
    nodata: Optional[float] = typer.Option(None, "--nodata", help="Nodata value of the source (default: the TIFF's own "
                                           "tag): pixels that hold it are left out of every sample"),
    fill: Optional[float] = typer.Option(None, "--fill", help="What a pixel outside the source gets (default: the "
                                         "nodata value, else NaN for floats and 0 for integers)"),
    grid_step: Optional[int] = typer.Option(None, "--grid-step", help="Across CRSs: the coordinate grid's step in output "
                                            "pixels (default: from 16 down until the error is within 0.125 px)"),
    cpu: bool = typer.Option(False, "--cpu", help="Evaluate with numpy on the host"),
    device: Optional[int] = typer.Option(None, "--device", help="GPU id (default: 0 when a GPU is present)"),
):
    """A streaming FLAC file or a GeoTIFF onto another grid (another CRS, another raster's grid, any transform) -> GeoTIFF."""
    from .crs import suggested_grid, transformer
    from .geo import Affine
    from .source import open_source
    from .streaming import warp_to_tiff

    with _failing("Warp failed"):
        if sum(x is not None for x in (dst_crs, like, transform)) != 1:
            console.print("[red]Error: give exactly one of --dst-crs, --like and --transform[/red]")
            raise typer.Exit(1)
        if (transform is None) != (out_shape is None):
            console.print("[red]Error: --transform and --out-shape go together[/red]")
            raise typer.Exit(1)
        if dst_crs is None and (res is not None or size is not None or bounds is not None):
            console.print("[red]Error: --res, --size and --bounds go with --dst-crs[/red]")
            raise typer.Exit(1)
        if res is not None and size is not None:
            console.print("[red]Error: give at most one of --res and --size[/red]")
            raise typer.Exit(1)
        path = _local(file_path)
        _existing(path)
        if like is not None:
            grid = open_source(like)
            t, shape, crs = grid.transform, (grid.height, grid.width), grid.crs
            if t is None:
                raise ValueError(f"{like} has no transform")
        elif transform is not None:
            t, shape, crs = _numbers(transform, 6, "--transform"), tuple(_numbers(out_shape, 2, "--out-shape", int)), None
        else:
            grid = open_source(path)
            st, sshape, scrs = grid.transform, (grid.height, grid.width), grid.crs
            if st is None or scrs is None:
                raise ValueError("--dst-crs needs a source with a transform and a CRS")
            crs = dst_crs
            t, shape = suggested_grid(st, sshape, transformer(scrs, dst_crs))
            if bounds is not None or res is not None or size is not None:
                xmin, ymax = t[2], t[5]
                xmax, ymin = xmin + t[0] * shape[1], ymax + t[4] * shape[0]
                if bounds is not None:
                    xmin, ymin, xmax, ymax = _numbers(bounds, 4, "--bounds")
                if size is not None:
                    shape = tuple(_numbers(size, 2, "--size", int))
                else:
                    r = float(res) if res is not None else t[0]
                    shape = (max(1, int((ymax - ymin) / r + 0.5)), max(1, int((xmax - xmin) / r + 0.5)))
                if size is not None:
                    t = Affine((xmax - xmin) / shape[1], 0.0, xmin, 0.0, -(ymax - ymin) / shape[0], ymax)
                else:
                    t = Affine(r, 0.0, xmin, 0.0, -r, ymax)
        dev = _pick_device(device, cpu)
        info = warp_to_tiff(path, output_path, tuple(t)[:6], shape, crs, None, resampling, nodata, fill, dev, cpu,
                            grid_step=grid_step)
        console.print(f"[green]{output_path}[/green]: {len(info['filled'])} band(s) of {shape[0]} x {shape[1]}, {resampling}"
                      + (f" (GPU {dev})" if dev is not None else " (host)"))
        if info["grid_step"]:
            console.print(f"coordinate grid: step {info['grid_step']}, error {info['grid_error']:.4f} px at the cell centres")
        w = info["source_window"]
        console.print("source window: " + (f"rows {w[0]}..{w[0] + w[2]}, columns {w[1]}..{w[1] + w[3]}" if w else
                                           "none (the grid misses the source)"))
        console.print("filled: " + ", ".join(f"band {k + 1}: {100.0 * v:.2f}%" for k, v in enumerate(info["shares"])))


def _show_tiff_info(path: Path):
    from .tiff import GeoTIFF

    info = GeoTIFF(path).info
    from .geo import Affine, bounds

    l, b, r, t = bounds(Affine(*info.transform), info.width, info.height)
    tab = Table(title=f"TIFF: {path.name}")
    tab.add_column("Property", style="cyan")
    tab.add_column("Value", style="green")
    tab.add_row("Dimensions", f"{info.width} x {info.height}")
    tab.add_row("Bands", str(info.count))
    tab.add_row("Data Type", str(info.dtype))
    tab.add_row("CRS", str(info.crs))
    tab.add_row("Bounds", f"({l:.6f}, {b:.6f}, {r:.6f}, {t:.6f})")
    tab.add_row("File Size", f"{path.stat().st_size / 1024 / 1024:.2f} MB")
    console.print(tab)


def _show_flac_info(path: Path):
    from . import flac_meta

    f = flac_meta.FLACFile(path)
    tab = Table(title=f"FLAC: {path.name}")
    tab.add_column("Property", style="cyan")
    tab.add_column("Value", style="green")
    tab.add_row("Sample Rate", f"{f.sample_rate} Hz")
    tab.add_row("Channels", str(f.channels))
    tab.add_row("Bits per Sample", str(f.bits_per_sample))
    tab.add_row("File Size", f"{path.stat().st_size / 1024 / 1024:.2f} MB")
    console.print(tab)
    if "GEOSPATIAL_CRS" in f:
        g = Table(title="Geospatial Metadata")
        g.add_column("Property", style="cyan")
        g.add_column("Value", style="green")
        get = lambda k, d="?": f.get(k, [d])[0]  # noqa: E731
        g.add_row("Dimensions", f"{get('GEOSPATIAL_WIDTH')} x {get('GEOSPATIAL_HEIGHT')}")
        g.add_row("Bands", get("GEOSPATIAL_COUNT"))
        g.add_row("Original Type", get("GEOSPATIAL_DTYPE"))
        g.add_row("CRS", get("GEOSPATIAL_CRS"))
        g.add_row("Data Range", f"[{get('GEOSPATIAL_DATA_MIN')}, {get('GEOSPATIAL_DATA_MAX')}]")
        g.add_row("Spatial Tiling", get("GEOSPATIAL_SPATIAL_TILING", "false"))
        console.print(g)


def main():
    app()


if __name__ == "__main__":
    main()
