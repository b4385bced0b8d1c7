"""GPU parity across raster layouts and load paths: every way the encoder can read its raster -- 16- and 8-byte
vector min/max, the scalar min/max, 8-byte sample vectors, element strides, the wave kernel's loader, 32- and 64-bit
offsets, both row-wrap classes of every loader, the host row copies -- against the CPU oracle, byte for byte.

Every case declares the load paths it must take (``fra_plan_flags``: ``PLAN_LOAD_VEC8``, ``PLAN_MINMAX_VEC16`` /
``_VEC8``, ``PLAN_OFF32``, ``PLAN_WAVE``) and asserts them before it compares, so no layout passes on the baseline
path.  The declared flags are worked out by hand from the rule in ``fra_layout.h`` (V = vector bytes / itemsize; every
window start, width, row stride and -- with more than one band -- band stride a multiple of V; col_stride 1; the raster
pointer aligned to the vector), as in ``tools/plan_layout_check.cpp``.

The expectation of a window is built from the flat array alone: its elements gathered by index arithmetic
(``base + c*bs + (r0+i)*rs + (c0+j)*cs``), normalised and encoded by the oracle.  All comparisons are exact.
"""
import hashlib

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

import oracle as O
from flac_raster import _native as N
from flac_raster.synth import synth_window

pytestmark = pytest.mark.gpu

WAVE, VEC8, MM16, MM8, OFF32 = N.PLAN_WAVE, N.PLAN_LOAD_VEC8, N.PLAN_MINMAX_VEC16, N.PLAN_MINMAX_VEC8, N.PLAN_OFF32
PATH_BITS = WAVE | VEC8 | MM16 | MM8 | OFF32
# vector classes of a layout: 16-byte min/max + 8-byte sample vectors, 8-byte both, sample vectors only, scalar
CLS = {"v16": VEC8 | MM16, "v8": VEC8 | MM8, "ld": VEC8, "s": 0}

H, W = 72, 264  # 19,008 samples per band: four full frames and a partial one, every frame crossing rows
ALIGNED = [(0, 0, 72, 264), (8, 16, 40, 128)]
UNALIGNED = [(3, 5, 33, 131), (0, 0, 1, 1)]  # (one unaligned window sends the whole plan to the scalar paths)


def _names(f):
    return "|".join(n for n, b in (("WAVE", WAVE), ("VEC8", VEC8), ("MM16", MM16), ("MM8", MM8), ("OFF32", OFF32))
                    if f & b) or "0"


def _diag(got: bytes, exp: bytes, fb):
    n = min(len(got), len(exp))
    i = next((k for k in range(n) if got[k] != exp[k]), n)
    f, acc = 0, 0
    for f, b in enumerate(fb):
        if acc + b > i:
            break
        acc += b
    return f"len got {len(got)} exp {len(exp)}; first diff byte {i} (frame {f}, +{i - acc})"


def gather(flat, base, B, strides, win):
    """The window's samples as ``(h*w, B)``, read from the flat array by index arithmetic alone."""
    bs, rs, cs = strides
    r0, c0, h, w = win
    i = np.arange(h, dtype=np.int64)[:, None, None]
    j = np.arange(w, dtype=np.int64)[None, :, None]
    c = np.arange(B, dtype=np.int64)[None, None, :]
    return flat[(base + c * bs + (r0 + i) * rs + (c0 + j) * cs).reshape(h * w, B)]


_oracle_cache = {}


def oracle_stream(inter, level, norm, blocksize):
    """(frames, frame sizes, audio, mn, mx, sample rate, stream bps) of the oracle for one window's samples.  Memoised
    on the samples themselves: layouts that hold the same pixels share one oracle encode."""
    key = (hashlib.sha1(inter.tobytes()).digest(), inter.dtype.str, inter.shape, level, norm, blocksize)
    hit = _oracle_cache.get(key)
    if hit is None:
        if norm:
            audio, mn, mx = O.normalize(inter, 16 if norm == 16 else 24)
            bps = 16 if norm == 16 else 32
        else:  # raw samples: int16 -> 16 bps, int32 -> 32 bps
            audio, mn, mx = inter, 0.0, 0.0
            bps = 16 if inter.dtype == np.int16 else 32
        sr = O.sample_rate_for_pixels(inter.shape[0])
        exp, fb, _ = O.encode(audio, sr, level=level, blocksize=blocksize, with_header=False, return_info=True)
        hit = _oracle_cache[key] = (exp, fb, audio, mn, mx, sr, bps)
    return hit


def check_streams(inters, windows, level, norm, blocksize, infos, frames):
    """Every stream of a plan against the oracle's encoding of its gathered samples: bytes, min / max, round trip."""
    assert len(infos) == len(inters)
    end = 0
    for win, inter, info in zip(windows, inters, infos):
        exp, fb, audio, mn, mx, sr, bps = oracle_stream(inter, level, norm, blocksize)
        assert info.sample_rate == sr and info.bps == bps and info.channels == inter.shape[1]
        assert np.array_equal(np.array([info.data_min, info.data_max]), np.array([mn, mx]), equal_nan=True), (
            f"window {win}: min/max {info.data_min!r}, {info.data_max!r}, oracle {mn!r}, {mx!r}")
        assert info.offset == end
        got = bytes(frames[info.offset: info.offset + info.frame_bytes])
        assert got == exp, f"window {win} level {level} norm {norm}: " + _diag(got, exp, fb)
        dec, _, _, _ = O.decode(O.stream_header(inter.shape[1], bps, sr, blocksize) + got)
        assert np.array_equal(dec, audio.astype(np.int32)), f"window {win}: decoded samples"
        end += len(got)
    assert end == len(frames)


def check_layout(flat, dtype, B, strides, windows, level, norm, flags, blocksize=4096, offset=0):
    """Encode ``windows`` of the device-resident raster ``flat[offset:]`` with element ``strides`` (band, row, col),
    assert the load paths the plan reports and compare every stream with the oracle.  Returns the frames."""
    ctx = N.default_context(0)
    flat = np.ascontiguousarray(flat, dtype=dtype).reshape(-1)
    dev = ctx.alloc(flat.nbytes)
    plan = None
    try:
        ctx.h2d(dev, flat)
        plan = N.Plan(ctx, dev + offset * flat.itemsize, True, flat.dtype, B, strides, windows, level, blocksize, norm)
        got = plan.flags() & PATH_BITS
        assert got == flags, f"load paths {_names(got)}, expected {_names(flags)}"
        plan.execute()
        plan.sync()
        infos, frames = plan.download()
    finally:
        if plan is not None:
            plan.close()
        ctx.free(dev)
    check_streams([gather(flat, offset, B, strides, w) for w in windows], windows, level, norm, blocksize, infos,
                  frames)
    return frames


# ------------------------------------------------------------------------------------------- 3a. layout matrix
class Cfg:
    def __init__(self, name, dtype, B, level, norm, wave):
        self.name, self.dtype, self.B, self.level, self.norm, self.wave = name, np.dtype(dtype), B, level, norm, wave

    def flags(self, cls):
        """The declared paths of a layout of vector class ``cls``: raw samples (norm 0) have no min/max pass, and the
        wave kernel takes the full frames of this configuration whenever its sample vectors are possible."""
        f = CLS[cls] | OFF32
        if self.norm == 0:
            f &= ~(MM16 | MM8)
        if self.wave and f & VEC8:
            f |= WAVE
        return f


CONFIGS = [
    Cfg("u16-l5", np.uint16, 3, 5, 16, True),     # the wave kernel
    Cfg("u16-l8", np.uint16, 3, 8, 16, False),    # the workgroup kernel, normalisation table
    Cfg("u8-l5", np.uint8, 2, 5, 16, True),       # 8-bit table and mid-side (levels 3..6: the wave kernel too)
    Cfg("f32-l8", np.float32, 2, 8, 24, False),
    Cfg("i16-raw", np.int16, 2, 5, 0, False),     # raw samples (load_raw_int), no min/max pass
]
F64 = Cfg("f64-l5", np.float64, 1, 5, 24, False)  # never a vector path: every layout is class "s"

_data_cache = {}


def _data(dtype, B):
    """A smooth synthetic ``(B, H, W)`` raster of ``dtype`` (computed once, never written)."""
    dt = np.dtype(dtype)
    key = (dt.str, B)
    if key not in _data_cache:
        if dt == np.uint16:
            r = synth_window(4, 41, B, H, W)
        elif dt == np.int16:
            r = synth_window(3, 42, B, H, W)
        elif dt == np.uint8:
            r = synth_window(4, 43, B, H, W).astype(np.float64)
            r = (r / r.max() * 255.0).astype(np.uint8)
        elif dt == np.float32:
            r = synth_window(5, 44, B, H, W).astype(np.float32)
        else:  # float64 values that float32 cannot hold
            r = synth_window(5, 45, B, H, W).astype(np.float64) * (1.0 + 2.0 ** -40) + 2.0 ** -30
        r.setflags(write=False)
        _data_cache[key] = r
    return _data_cache[key]


def _filler(n, dtype):
    """Padding elements: the type's extremes in turn, so that a load that strays into padding moves the min / max."""
    dt = np.dtype(dtype)
    lo, hi = (-3.0e38, 3.0e38) if dt.kind == "f" else (np.iinfo(dt).min, np.iinfo(dt).max)
    out = np.empty(n, dt)
    out[0::2] = hi
    out[1::2] = lo
    return out


def _padded(data, row_pad, band_pad):
    """Band-planar with ``row_pad`` elements after every row and ``band_pad`` after every band."""
    B = data.shape[0]
    rs = W + row_pad
    bs = H * rs + band_pad
    flat = _filler(B * bs, data.dtype)
    for b in range(B):
        flat[b * bs: b * bs + H * rs].reshape(H, rs)[:, :W] = data[b]
    return flat, (bs, rs, 1)


# name -> (builder(data, itemsize) -> (flat, B, strides, pointer offset in elements), vector class of the ALIGNED
# windows per itemsize).  V = 16 / itemsize for the 16-byte class, 8 / itemsize for the 8-byte one.  The aligned
# windows start at elements 0 and 8 rs + 16 and are 264 and 128 wide: uint8 (V = 16) never has 16-byte vectors here
# because 264 % 16 == 8, so its best class is "v8".
def _planar(d, es):
    return d.reshape(-1), d.shape[0], (H * W, W, 1), 0


def _rows16(d, es):
    flat, st = _padded(d, 16 // es, 0)
    return flat, d.shape[0], st, 0


def _rows8(d, es):
    flat, st = _padded(d, 8 // es, 0)
    return flat, d.shape[0], st, 0


def _rows13(d, es):
    flat, st = _padded(d, 13, 0)
    return flat, d.shape[0], st, 0


def _bands8(d, es):
    flat, st = _padded(d, 0, 8 // es)
    return flat, d.shape[0], st, 0


def _bands1(d, es):
    flat, st = _padded(d, 0, 1)
    return flat, d.shape[0], st, 0


def _pixel(d, es):
    B = d.shape[0]
    return d.transpose(1, 2, 0).reshape(-1), B, (1, W * B, B), 0


def _line(d, es):  # band-planar inside each row: band_stride < row_stride
    B = d.shape[0]
    return d.transpose(1, 0, 2).reshape(-1), B, (W, B * W, 1), 0


def _ptr1(d, es):
    return np.concatenate([_filler(1, d.dtype), d.reshape(-1)]), d.shape[0], (H * W, W, 1), 1


def _ptr8(d, es):
    return np.concatenate([_filler(8 // es, d.dtype), d.reshape(-1)]), d.shape[0], (H * W, W, 1), 8 // es


def _band0(d, es):  # two identical bands: the side channel is all zero
    return d[0].reshape(-1), 2, (0, W, 1), 0


def _row0(d, es):  # every row is row 0
    return d[:, 0, :].reshape(-1), d.shape[0], (W, 0, 1), 0


def _row8(d, es):  # rows overlap: row r starts 8 elements after row r - 1
    n = (H - 1) * 8 + W
    return np.concatenate([d[b].reshape(-1)[:n] for b in range(d.shape[0])]), d.shape[0], (n, 8, 1), 0


SAME_AS_PLANAR = {1: "v8", 2: "v16", 4: "v16"}
SCALAR = {1: "s", 2: "s", 4: "s"}
LAYOUTS = {
    # 264, 19008 and 8*264+16 are multiples of 8 (and of 16 / itemsize for itemsize 2 and 4)
    "planar": (_planar, SAME_AS_PLANAR),
    # rows of 264 + 16 / itemsize elements: 280 % 8 == 0 (uint8), 272 % 8 == 0 (16-bit), 268 % 4 == 0 (32-bit)
    "rows+16B": (_rows16, SAME_AS_PLANAR),
    # rows of 264 + 8 / itemsize: 268 % 8 == 4 and 266 % 4 == 2 leave 8-byte vectors only; uint8 rows of 272 allow
    # 16, its widths do not
    "rows+8B": (_rows8, {1: "v8", 2: "v8", 4: "v8"}),
    "rows+13": (_rows13, SCALAR),  # 277 is odd
    # bands of 19008 + 8 / itemsize elements: % (16 / itemsize) != 0
    "bands+8B": (_bands8, {1: "v8", 2: "v8", 4: "v8"}),
    "bands+1": (_bands1, SCALAR),  # 19009 is odd (every configuration here has two or three bands)
    "pixel": (_pixel, SCALAR),     # col_stride = B
    # rows of B * 264, bands 264 apart: multiples of 8 / 8 / 4 elements
    "line": (_line, SAME_AS_PLANAR),
    "ptr+1": (_ptr1, SCALAR),      # the pointer is a multiple of neither 8 nor 16
    # pointer % 16 == 8: 8-byte sample vectors; a 16-byte min/max layout does not fall back to 8-byte vectors but to
    # the scalar kernel (fra_plan.h minmax_vec), the uint8 layout's 8-byte min/max stays
    "ptr+8B": (_ptr8, {1: "v8", 2: "ld", 4: "ld"}),
    "band0": (_band0, SAME_AS_PLANAR),   # 0 is a multiple of every V
    "row0": (_row0, SAME_AS_PLANAR),     # bands 264 apart, window starts 0 and 16
    "row8": (_row8, SAME_AS_PLANAR),     # bands 832 apart, window starts 0 and 8*8+16 = 80, rows 8 apart
}


def _run_layout(cfg, layout, monkeypatch):
    build, classes = LAYOUTS[layout]
    es = cfg.dtype.itemsize
    flat, B, strides, offset = build(_data(cfg.dtype, cfg.B), es)
    cls = "s" if es == 8 else classes[es]
    out = []
    for wins, f in ((ALIGNED, cfg.flags(cls)), (UNALIGNED, cfg.flags("s"))):
        out.append(check_layout(flat, cfg.dtype, B, strides, wins, cfg.level, cfg.norm, f, offset=offset))
        if f & WAVE:  # the same layout through the workgroup kernel's loaders
            monkeypatch.setenv("FRA_ANALYZE_WG", "1")
            wg = check_layout(flat, cfg.dtype, B, strides, wins, cfg.level, cfg.norm, f & ~WAVE, offset=offset)
            monkeypatch.delenv("FRA_ANALYZE_WG")
            assert wg == out[-1]
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cfg", CONFIGS, ids=[c.name for c in CONFIGS])
def test_layout_matrix(monkeypatch, cfg, layout):
    """Every layout in every configuration, aligned and unaligned windows in plans of their own, against the oracle;
    a plan on the wave kernel runs again on the workgroup kernel (FRA_ANALYZE_WG=1)."""
    monkeypatch.delenv("FRA_ANALYZE_WG", raising=False)
    got = _run_layout(cfg, layout, monkeypatch)
    if layout in ("ptr+1", "ptr+8B"):  # the same pixels behind a moved pointer: the baseline's bytes
        assert got == _run_layout(cfg, "planar", monkeypatch)


@pytest.mark.parametrize("layout", ["planar", "rows+16B", "pixel"])
def test_layout_float64(monkeypatch, layout):
    """float64 has no vector path: whatever the layout, the flags report element loads and 32-bit offsets only."""
    monkeypatch.delenv("FRA_ANALYZE_WG", raising=False)
    assert F64.flags("s") == OFF32
    _run_layout(F64, layout, monkeypatch)


# ------------------------------------------------------------------------------------------- 3b. width classes
RW = 4104  # raster columns


def _stacked(widths):
    """Windows of the given widths, each the fewest rows that hold two full frames and a partial one, stacked
    vertically at column 0."""
    wins, r = [], 0
    for w in widths:
        h = -(-9000 // w)
        wins.append((r, 0, h, w))
        r += h
    return wins, r


def _ramp_noise(shape, dtype, seed, cols=None):
    """Cheap smooth-plus-noise data over ``shape`` = (..., rows, columns); columns >= ``cols`` stay zero."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    out = np.zeros(shape, dt)
    n = shape[-1] if cols is None else cols
    part = shape[:-1] + (n,)
    r = np.arange(shape[-2], dtype=np.int64)[:, None]
    c = np.arange(n, dtype=np.int64)[None, :]
    v = 3 * r + 2 * c + rng.integers(0, 24, size=part)
    if dt.kind == "f":
        out[..., :n] = (v / 977.0).astype(dt)
    elif dt.itemsize == 1:
        out[..., :n] = (v // 16 % 256).astype(dt)
    else:
        out[..., :n] = (v % 60000).astype(dt)
    return out


WIDTHS = [
    # uint16: V = 4; the workgroup loader steps 1,024 columns, the wave loader 256.  Widths are multiples of 4 but not
    # all of 8, rows of 4104 = 8 * 513 elements: 8-byte vectors in both passes
    ("u16", np.uint16, 2, 16, [4, 252, 256, 260, 1020, 1024, 1028, 4096, 4100], (5, 8), True),
    # uint8: V = 8; steps 2,048 / 512; 4104 % 16 == 8
    ("u8", np.uint8, 2, 16, [8, 504, 512, 520, 2040, 2048, 2056], (5, 8), True),
    # float32: V = 2; step 512; width 2 is no multiple of 4
    ("f32", np.float32, 2, 24, [2, 510, 512, 514], (8,), False),
]


@pytest.mark.parametrize("name,dtype,B,norm,widths,levels,wave", WIDTHS, ids=[w[0] for w in WIDTHS])
def test_width_classes_vector_loaders(monkeypatch, name, dtype, B, norm, widths, levels, wave):
    """Windows narrower than, equal to and wider than each vector loader's step (one subtraction per row wrap when
    the width reaches the step, a division below it), and one vector wide."""
    monkeypatch.delenv("FRA_ANALYZE_WG", raising=False)
    wins, rows = _stacked(widths)
    flat = _ramp_noise((B, rows, RW), dtype, 7, cols=max(widths)).reshape(-1)
    for level in levels:
        f = VEC8 | MM8 | OFF32 | (WAVE if wave and level == 5 else 0)
        check_layout(flat, dtype, B, (rows * RW, RW, 1), wins, level, norm, f)


def test_width_classes_scalar_loader(monkeypatch):
    """The element-stride loader (256 samples per step) on a pixel-interleaved uint16 raster with col_stride 2:
    widths 1, 255, 256 and 257."""
    monkeypatch.delenv("FRA_ANALYZE_WG", raising=False)
    wins, rows = _stacked([1, 255, 256, 257])
    flat = _ramp_noise((rows, RW * 2), np.uint16, 8, cols=2 * 257).reshape(-1)  # (row, column, band)
    for level in (5, 8):
        check_layout(flat, np.uint16, 2, (1, RW * 2, 2), wins, level, 16, OFF32)


# ------------------------------------------------------------------------------------------- 3c. wide 32-bit ranges
def _wide_range_raster(dtype):
    """Five 64 x 96 blocks, two bands, stacked vertically; block k spans exactly [mn, mx] of ``RANGES[k]`` in each of
    its windows: the extremes sit in columns 9 and 10 (inside the 4-column window at column 8 and the window at
    column 3), further planted values in columns 3..11."""
    dt = np.dtype(dtype)
    if dt == np.uint32:
        ranges = [(0, 2**32 - 1),            # R = 2^32 - 1
                  (0, 2**31),                # 2^31
                  (2**31, 2**32 - 1),        # 2^31 - 1, every value >= 2^31
                  (2**31 - 2**23, 2**31 + 2**23 + 1),  # 2^24 + 1 across 2^31
                  (0, 4294967291)]           # the prime 2^32 - 5
        plant = [0, 1, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1]
    else:
        ranges = [(-2**31, 2**31 - 1), (-2**31, 0), (-2**31 + 1, 0), (-2**23, 2**23 + 1), (-2**31, 2**31 - 5)]
        plant = [-2**31, -2**31 + 1, -1, 0, 2**31 - 1]
    yy, xx = np.mgrid[0:64, 0:96]
    blocks = []
    for k, (mn, mx) in enumerate(ranges):
        bands = []
        for b in range(2):
            f = 0.5 + 0.3 * np.sin(yy / 9.0 + b) + 0.15 * np.cos(xx / 7.0 + k)  # in [0.05, 0.95]
            v = mn + (f * float(mx - mn)).astype(np.int64)
            v[5, 9], v[40, 10] = mn, mx
            inside = [p for p in plant if mn <= p <= mx]
            for n, p in enumerate(inside):
                v[10 + 3 * n, 8 + (n + b) % 4] = p   # columns 8..11
                v[11 + 3 * n, 3 + n] = p             # columns 3..8
            assert v.min() == mn and v.max() == mx
            bands.append(v)
        blocks.append(np.stack(bands))
    return np.concatenate(blocks, axis=1).astype(dt), [mx - mn for mn, mx in ranges]


@pytest.mark.parametrize("dtype", [np.uint32, np.int32], ids=["uint32", "int32"])
@pytest.mark.parametrize("norm", [24, 16])
def test_wide_range_32bit_integers(dtype, norm):
    """Ranges up to 2^32 - 1 and values on both sides of 2^31 through the integer normalisation: the vectorised
    min/max with its 32-bit keys (16-byte aligned windows 4 and 96 wide) and the scalar one (a window at column 3)."""
    r, R = _wide_range_raster(dtype)
    assert R == [2**32 - 1, 2**31, 2**31 - 1, 2**24 + 1, 4294967291]
    flat, st = r.reshape(-1), (320 * 96, 96, 1)
    aligned = [w for k in range(5) for w in ((64 * k, 0, 64, 96), (64 * k, 8, 64, 4))]
    check_layout(flat, dtype, 2, st, aligned, 5, norm, VEC8 | MM16 | OFF32)  # (32-bit types never take the wave kernel)
    check_layout(flat, dtype, 2, st, [(64 * k, 3, 64, 90) for k in range(5)], 5, norm, OFF32)


# ------------------------------------------------------------------------------------------- 3d. 64-bit offsets
def test_row_stride_beyond_32bit_offsets():
    """Rows 2^29 uint16 elements (1 GiB) apart: a frame's two rows span 2^31 + 16384 bytes, so the sample loads take
    64-bit addresses (no OFF32, hence no WAVE) while the min/max pass (2 rows * 2^30 bytes < 2^32) stays on 16-byte
    vectors.  One 2.0 GiB allocation of which only the three window rows are written and read."""
    rs, width = 1 << 29, 8192
    rows = _ramp_noise((3, width), np.uint16, 9)
    ctx = N.default_context(0)
    dev = ctx.alloc((2 * rs + width) * 2)
    plan = None
    try:
        for r in range(3):
            ctx.h2d(dev + r * rs * 2, rows[r])
        wins = [(0, 0, 3, width)]
        plan = N.Plan(ctx, dev, True, np.uint16, 1, (0, rs, 1), wins, 5, 4096, 16)
        got = plan.flags() & PATH_BITS
        assert got == VEC8 | MM16, f"load paths {_names(got)}"
        plan.execute()
        plan.sync()
        infos, frames = plan.download()
    finally:
        if plan is not None:
            plan.close()
        ctx.free(dev)
    check_streams([rows.reshape(-1, 1)], wins, 5, 16, 4096, infos, frames)


# ------------------------------------------------------------------------------------------- 3e. host paths
def _view_layout(view, base):
    """(flat base array, element offset of the view's first element, element strides) of a view of ``base``."""
    off = view.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    assert off >= 0 and off % base.itemsize == 0
    return base.reshape(-1), off // base.itemsize, N._element_strides(view)


def check_host_view(view, base, windows, level, norm, flags):
    """``encode_windows_buffer`` (fra_plan_encode_host) of a strided host view against the oracle's encoding of the
    windows gathered from the base array; the flags are those of a host plan of the view's strides (its device copy
    is aligned)."""
    flat, off, strides = _view_layout(view, base)
    B = view.shape[0]
    plan = N.Plan(N.default_context(0), None, False, view.dtype, B, strides, windows, level, 4096, norm)
    try:
        got = plan.flags() & PATH_BITS
    finally:
        plan.close()
    assert got == flags, f"load paths {_names(got)}, expected {_names(flags)}"
    infos, frames = N.encode_windows_buffer(view, windows, level=level, norm=norm, pinned=False)
    check_streams([gather(flat, off, B, strides, w) for w in windows], windows, level, norm, 4096, infos, frames)


def test_host_path_strided_views():
    """Views of larger arrays through the host pipeline's row copies.  The job's pointer is the view's first element
    and the plan's device copy starts there, aligned: the load paths depend on the strides and windows alone."""
    d = _data(np.uint16, 3)
    big = _ramp_noise((3, H + 9, W + 16), np.uint16, 10)  # rows of 280 elements, bands of 81 * 280: multiples of 8
    full = VEC8 | MM16 | OFF32 | WAVE
    # column offset 8 (a 16-byte aligned host pointer) and 3 (an odd one): padded rows, the same paths
    check_host_view(big[:, 5:5 + H, 8:8 + W], big, ALIGNED, 5, 16, full)
    check_host_view(big[:, 5:5 + H, 3:3 + W], big, ALIGNED, 5, 16, full)
    check_host_view(big[:, 5:5 + H, 3:3 + W], big, UNALIGNED, 5, 16, OFF32)
    # the (B, H, W) view of a pixel-interleaved array (one run of all bands per row band), and of a line-interleaved one
    pix = np.ascontiguousarray(d.transpose(1, 2, 0))
    check_host_view(pix.transpose(2, 0, 1), pix, ALIGNED, 5, 16, OFF32)
    check_host_view(pix.transpose(2, 0, 1), pix, UNALIGNED, 5, 16, OFF32)
    lin = np.ascontiguousarray(d.transpose(1, 0, 2))
    check_host_view(lin.transpose(1, 0, 2), lin, ALIGNED, 5, 16, full)
    check_host_view(lin.transpose(1, 0, 2), lin, ALIGNED, 8, 16, full & ~WAVE)


def test_host_path_several_bands_column_offset_view():
    """A plan of 2,304 frames (36 tiles of 512 x 512, uint16, one band) goes through the host pipeline in several
    row bands, its raster a column-offset view of a wider array: bytes and stream table equal the device path's on a
    contiguous copy, and three windows equal the oracle's."""
    S = 3072
    rng = np.random.default_rng(12)
    big = np.empty((1, S, S + 24), np.uint16)
    big[0] = (30000 + np.cumsum(rng.integers(-20, 21, size=(S, S + 24)), axis=1)).astype(np.uint16)
    view = big[:, :, 8:8 + S]
    wins = [(r, c, 512, 512) for r in range(0, S, 512) for c in range(0, S, 512)]
    flat, off, strides = _view_layout(view, big)
    plan = N.Plan(N.default_context(0), None, False, view.dtype, 1, strides, wins, 5, 4096, 16)
    try:
        assert plan.capacity()[1] > 1, "one host band only"
        assert plan.flags() & PATH_BITS == VEC8 | MM16 | OFF32 | WAVE
    finally:
        plan.close()
    ih, fh = N.encode_windows_buffer(view, wins, level=5, norm=16, pinned=False)
    idv, fd = N.encode_windows(np.ascontiguousarray(view), wins, level=5, norm=16, path="device")
    assert bytes(fh) == bytes(fd)
    table = [(a.offset, a.frame_bytes, a.nframes, a.data_min, a.data_max) for a in ih]
    assert table == [(a.offset, a.frame_bytes, a.nframes, a.data_min, a.data_max) for a in idv]
    for k in (0, len(wins) // 2 + 2, len(wins) - 1):
        exp, fb, _, mn, mx, _, _ = oracle_stream(gather(flat, off, 1, strides, wins[k]), 5, 16, 4096)
        got = bytes(fh[ih[k].offset: ih[k].offset + ih[k].frame_bytes])
        assert got == exp, f"window {wins[k]}: " + _diag(got, exp, fb)
        assert (ih[k].data_min, ih[k].data_max) == (mn, mx)


def _oracle_or_refusal(view, base, windows):
    """A host encode of rows that overlap: the oracle's bytes, or FRA_E_INVALID naming the layout -- never success
    with other bytes."""
    flat, off, strides = _view_layout(view, base)
    try:
        infos, frames = N.encode_windows_buffer(view, windows, level=5, norm=16, pinned=False)
    except N.NativeError as e:
        assert "error -1:" in str(e) and "layout" in str(e) and "row_stride" in str(e), str(e)
        return "refused"
    check_streams([gather(flat, off, view.shape[0], strides, w) for w in windows], windows, 5, 16, 4096, infos, frames)
    return "encoded"


def test_host_path_zero_and_overlapping_row_strides():
    d = _data(np.uint16, 3)
    row = np.ascontiguousarray(d[:, :1, :])              # (3, 1, W)
    bcast = np.broadcast_to(row, (3, H, W))              # row stride 0
    assert N._element_strides(bcast)[1] == 0
    n = (H - 1) * 8 + W
    src = np.ascontiguousarray(d.reshape(3, -1)[:, :n])  # (3, 832)
    slide = as_strided(src, shape=(3, H, W), strides=(src.strides[0], 8 * 2, 2), writeable=False)  # row stride 8
    outcomes = {"broadcast": _oracle_or_refusal(bcast, row, ALIGNED + UNALIGNED),
                "sliding": _oracle_or_refusal(slide, src, ALIGNED + UNALIGNED)}
    assert outcomes == {"broadcast": "refused", "sliding": "refused"}  # the documented contract of the host entries
    # a raster of one row has no rows to overlap: whatever its row stride, it is encoded
    one = as_strided(src, shape=(3, 1, W), strides=(src.strides[0], 0, 2), writeable=False)
    assert N._element_strides(one)[1] == 0
    assert _oracle_or_refusal(one, src, [(0, 0, 1, W), (0, 3, 1, 131)]) == "encoded"
    # the producer-driven entries refuse the same job before they wait for a row or touch the ring
    ctx = N.default_context(0)
    plan = N.Plan(ctx, None, False, np.uint16, 3, (n, 8, 1), ALIGNED, 5, 4096, 16)
    try:
        out = np.empty(plan.capacity()[0], np.uint8)
        ready, done = np.array([H], np.int64), np.zeros(1, np.int64)
        with pytest.raises(N.NativeError, match="layout"):
            plan.encode_host_progress(src, out, ready)
        ring = np.zeros((3, H, W), np.uint16)
        with pytest.raises(N.NativeError, match="layout"):
            plan.encode_ring(ring, out, ready, done)
        assert done[0] == 0
    finally:
        plan.close()
    # the device-resident path encodes both layouts (test_layout_matrix: row0, row8)
