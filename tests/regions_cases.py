"""Inputs the regions tests share (``test_regions_cpu.py``, ``test_gpu_regions.py``): masks and class rasters at the
shapes around the kernel's tile side T, and the hand-made ones that pin the seams."""
import functools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "flac-raster_amd"))
from flac_raster.regions import TILE as T  # noqa: E402

SMALL = [(1, 1), (1, 70), (70, 1), (T, T), (T + 1, T + 1), (2 * T + 2, 3 * T - 1), (5, 1100)]
LARGE = (520, 520)   # 81 tiles of 64: workgroups on every XCD
SEAMS = (2 * T + 2, 3 * T - 1)
CONTENTS = ["none", "one", "all", "r5", "perc4", "perc8", "checker", "spiral", "comb", "blocks3", "random3"]
LARGE_CONTENTS = ["all", "perc4", "perc8", "checker", "spiral", "random3"]


def spiral(h, w):
    """A one-pixel-wide 4-connected path from (0, 0) inwards: one component whose area is its pixel count."""
    a = np.zeros((h, w), bool)
    r = c = 0
    dr, dc = 0, 1
    a[0, 0] = True
    al = a.tolist()

    def free(nr, nc, r, c):
        if not (0 <= nr < h and 0 <= nc < w) or al[nr][nc]:
            return False
        for ar, ac in ((nr - 1, nc), (nr + 1, nc), (nr, nc - 1), (nr, nc + 1)):
            if (ar, ac) != (r, c) and 0 <= ar < h and 0 <= ac < w and al[ar][ac]:
                return False
        return True

    while True:
        if free(r + dr, c + dc, r, c):
            r, c = r + dr, c + dc
        else:
            dr, dc = dc, -dr  # turn right
            if not free(r + dr, c + dc, r, c):
                break
            r, c = r + dr, c + dc
        al[r][c] = True
    return np.asarray(al, bool).reshape(h, w)


@functools.lru_cache(maxsize=None)
def _content(shape, content):
    h, w = shape
    rng = np.random.default_rng(17 * h + w + 1000 * CONTENTS.index(content))
    a = np.zeros((h, w), np.uint8)
    if content == "one":
        a[rng.integers(0, h), rng.integers(0, w)] = 1
    elif content == "all":
        a[:] = 1
    elif content in ("r5", "perc4", "perc8"):
        a[:] = rng.random((h, w)) < {"r5": 0.05, "perc4": 0.59, "perc8": 0.41}[content]
    elif content == "checker":
        a[:] = (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0
    elif content == "spiral":
        a[:] = spiral(h, w)
    elif content == "comb":       # the teeth join only in the last row: a first pixel far from where it is united
        a[:, ::2] = 1
        a[h - 1, :] = 1
    elif content == "blocks3":    # three classes in blocks of 24 x 40, no background
        a[:] = (np.add.outer(np.arange(h) // 24, np.arange(w) // 40) % 3) + 1
    elif content == "random3":    # background and three classes at random
        a[:] = rng.integers(0, 4, (h, w))
    a.setflags(write=False)
    return a


def mask(shape, content):
    """The (h, w) uint8 raster of a content (read-only, shared)."""
    return _content(tuple(shape), content)


def diagonals():
    """Two diagonals that cross a four-tile corner exactly at (T-1, T-1)-(T, T) and at (T-1, 2T)-(T, 2T-1): one component
    each under 8-connectivity, eight apart under 4."""
    a = np.zeros(SEAMS, np.uint8)
    for k in range(-4, 4):
        a[T + k, T + k] = 1
        a[T + k, 2 * T - 1 - k] = 1
    return a


def seam_row():
    """Two blocks that touch only along the seam between the rows T-1 and T."""
    a = np.zeros(SEAMS, np.uint8)
    a[T - 10:T, 5:21] = 1
    a[T:T + 10, 20:40] = 1
    return a


def seam_col():
    """Two blocks that touch only along the seam between the columns T-1 and T."""
    a = np.zeros(SEAMS, np.uint8)
    a[5:21, T - 10:T] = 1
    a[20:40, T:T + 10] = 1
    return a


def float_classes(shape=SEAMS, dt=np.float32):
    """A float band of -0.0, 0.0, NaN, 1.5 and 2.5 at random: under ``==`` the two zeros are one class and a NaN is
    background whatever the options say."""
    rng = np.random.default_rng(99)
    vals = np.array([-0.0, 0.0, np.nan, 1.5, 2.5], dt)
    return vals[rng.integers(0, 5, shape)]


def hand_made():
    return [("diagonals", diagonals()), ("seam_row", seam_row()), ("seam_col", seam_col())]


def small_cases():
    """(id, (h, w) uint8 raster) for every small shape and content, then the hand-made ones."""
    out = [(f"{h}x{w}-{c}", mask((h, w), c)) for (h, w) in SMALL for c in CONTENTS]
    return out + hand_made()


def large_cases():
    return [(f"{LARGE[0]}x{LARGE[1]}-{c}", mask(LARGE, c)) for c in LARGE_CONTENTS]
