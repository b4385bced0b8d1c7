"""Inputs the proximity tests share (``test_proximity_cpu.py``, ``test_gpu_proximity.py``): rasters of every source
dtype at the target densities the issue names, and the hand-made ties that pin the nearest-target rule."""
import numpy as np

DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]
DENSITIES = ["none", "one", "1%", "30%", "all"]
SMALL = [(1, 1), (7, 19), (33, 67)]
LARGE = (130, 517)


def _values(rng, shape, dt):
    """Non-zero values of the dtype, its ends among them: what an allocation copies must be told apart."""
    dt = np.dtype(dt)
    if dt.kind == "f":
        v = rng.uniform(-1000.0, 1000.0, shape).astype(dt)
        v[v == 0] = 1.5
        return v
    info = np.iinfo(dt)
    v = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64)
    v[v == 0] = info.max
    v.reshape(-1)[0] = info.min if info.min else info.max
    return v.astype(dt)


def raster(shape, density, dt=np.uint8, seed=0, bands=1):
    """A ``(bands, h, w)`` raster whose non-zero pixels are the targets.  A float raster carries NaN and -0.0 among the
    pixels that are no targets."""
    dt = np.dtype(dt)
    h, w = shape
    rng = np.random.default_rng(1000 * seed + 17 * h + w + dt.num)
    mask = np.zeros((bands, h, w), bool)
    for b in range(bands):
        if density == "one":
            mask[b, rng.integers(0, h), rng.integers(0, w)] = True
        elif density == "all":
            mask[b] = True
        elif density != "none":
            mask[b] = rng.random((h, w)) < (0.01 if density == "1%" else 0.3)
    a = np.where(mask, _values(rng, (bands, h, w), dt), 0).astype(dt)
    if dt.kind == "f" and density not in ("all",):
        odd = ~mask & (rng.random((bands, h, w)) < 0.2)
        a[odd] = np.where(rng.random(int(odd.sum())) < 0.5, np.nan, -0.0).astype(dt)
    return a


def ties():
    """``(name, raster (h, w) uint8, pixel (r, c), the nearest target (r, c))``: the smallest column wins, then the
    smallest row."""
    out = []
    a = np.zeros((5, 9), np.uint8)
    a[2, 1], a[2, 7] = 11, 22
    out.append(("left and right", a, (2, 4), (2, 1)))
    a = np.zeros((9, 5), np.uint8)
    a[1, 2], a[7, 2] = 11, 22
    out.append(("above and below", a, (4, 2), (1, 2)))
    a = np.zeros((7, 7), np.uint8)
    a[1, 1], a[1, 5], a[5, 1], a[5, 5] = 11, 22, 33, 44
    out.append(("four diagonals", a, (3, 3), (1, 1)))
    a = np.zeros((11, 11), np.uint8)
    a[4, 2], a[1, 6], a[9, 6] = 33, 11, 22   # (5, 6): the pair at d2 = 16, the single target (4, 2) at 1 + 16 = 17
    out.append(("a pair in one column", a, (5, 6), (1, 6)))
    a = np.zeros((11, 11), np.uint8)
    a[2, 6], a[8, 6], a[5, 3] = 11, 22, 33   # (5, 6): the pair in column 6 at d2 = 9, the single target in column 3 at 9
    out.append(("a pair against a smaller column", a, (5, 6), (5, 3)))
    return out


def seam_rasters():
    """(200, 70): four chunks of 64 rows, the last one ragged.  Targets in the first row only, in the last row only, and
    on the chunk boundaries only, so that a distance is carried across more than one chunk."""
    out = []
    for name, rows in (("first row", [0]), ("last row", [199]), ("chunk boundaries", [63, 64, 191, 192]),
                       ("one chunk end", [127])):
        a = np.zeros((1, 200, 70), np.uint16)
        rng = np.random.default_rng(len(name))
        for r in rows:
            cols = rng.choice(70, 9, replace=False)
            a[0, r, cols] = rng.integers(1, 60000, 9)
        out.append((name, a))
    return out
