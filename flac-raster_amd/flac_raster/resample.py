"""Decimation of a raster by a power-of-two factor: the rule of the decimated reads, stated in numpy.

This is the host path of ``streaming.read_window(decimate=k)`` / ``read_overview`` and the expectation the GPU kernel
(``k_decimate``, ``include/flac_raster_amd.h``) is tested against, bit for bit.

A region of ``h x w`` pixels is cut into ``k x k`` blocks anchored at its origin; block ``(R, C)`` covers rows
``[R k, min(R k + k, h))`` and columns ``[C k, min(C k + k, w))`` and holds ``n`` = rows x columns pixels (edge blocks
are smaller).  The output is ``ceil(h / k) x ceil(w / k)`` in the input's dtype.

``nearest``   ``out[R, C] = in[min(R k + k/2, h - 1), min(C k + k/2, w - 1)]``
``average``   integer dtypes: ``S`` = the exact integer sum of the block, ``out = rint(float64(S) / float64(n))``,
              round half to even.  Float dtypes: every element as float64; each block row is padded with ``+0.0`` to
              ``k`` elements and summed by the adjacent-pair tree (``(x0 + x1), (x2 + x3), ...`` then pairs of those,
              ``log2 k`` levels); the row sums are accumulated top to bottom (``acc = row_0; acc += row_1; ...``; rows
              the block does not have are not added); ``out = dtype(acc / float64(n))``.  Plain IEEE arithmetic: NaN
              and infinities propagate, nothing is skipped.
"""

from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

FACTORS = (2, 4, 8, 16, 32, 64)
RESAMPLING = {"nearest": 0, "average": 1}
_DTYPES = tuple(np.dtype(t) for t in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32,
                                      np.float64))


def check_factor(factor) -> int:
    k = int(factor)
    if k not in FACTORS or k != factor:
        raise ValueError(f"the decimation factor must be one of {FACTORS}, got {factor!r}")
    return k


def resampling_code(resampling) -> int:
    if resampling not in RESAMPLING:
        raise ValueError(f"resampling must be 'nearest' or 'average', got {resampling!r}")
    return RESAMPLING[resampling]


def decimated_shape(h: int, w: int, k: int) -> Tuple[int, int]:
    """``(ceil(h / k), ceil(w / k))``."""
    k = check_factor(k)
    return -(-int(h) // k), -(-int(w) // k)


def decimated_transform(transform: Sequence[float], window: Sequence[int], k: int) -> Tuple[float, ...]:
    """The geotransform ``(a, b, c, d, e, f)`` of a region decimated by ``k``: ``window`` = (row_off, col_off, ...) is
    the region in the raster ``transform`` belongs to.  ``k = 1`` is the plain shift to the region's origin."""
    a, b, c, d, e, f = (float(v) for v in tuple(transform)[:6])
    row, col = int(window[0]), int(window[1])
    return a * k, b * k, c + col * a + row * b, d * k, e * k, f + col * d + row * e


def decimate(raster: np.ndarray, factor: int, resampling: str = "nearest") -> np.ndarray:
    """``raster`` ``(B, h, w)`` or ``(h, w)`` at ``1 / factor`` resolution (the module's rule), same dtype."""
    k = check_factor(factor)
    mode = resampling_code(resampling)
    a = np.asarray(raster)
    if a.ndim == 2:
        return decimate(a[None], k, resampling)[0]
    if a.ndim != 3 or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"expected a (B, h, w) or (h, w) raster with h, w >= 1, got shape {a.shape}")
    if a.dtype.newbyteorder("=") not in _DTYPES:
        raise TypeError(f"unsupported dtype {a.dtype}")
    B, h, w = a.shape
    oh, ow = decimated_shape(h, w, k)
    if mode == 0:
        rows = np.minimum(np.arange(oh) * k + k // 2, h - 1)
        cols = np.minimum(np.arange(ow) * k + k // 2, w - 1)
        return np.ascontiguousarray(a[:, rows[:, None], cols[None, :]])
    is_float = a.dtype.kind == "f"
    acc_t = np.float64 if is_float else np.int64
    # the blocks as (B, oh, k, ow, k); what the raster does not have is +0.0 / 0
    x = np.zeros((B, oh * k, ow * k), dtype=acc_t)
    x[:, :h, :w] = a
    x = x.reshape(B, oh, k, ow, k)
    with np.errstate(invalid="ignore", over="ignore"):
        while x.shape[-1] > 1:  # the adjacent-pair tree along a block row
            x = x[..., 0::2] + x[..., 1::2]
        rows = x[..., 0]  # (B, oh, k, ow): the row sums of every block
        nrows = np.minimum(k, h - np.arange(oh) * k)  # rows of the blocks of block row R
        ncols = np.minimum(k, w - np.arange(ow) * k)
        acc = rows[:, :, 0, :].copy()
        for j in range(1, k):  # top to bottom; rows a block does not have are not added
            have = (j < nrows)[None, :, None]
            acc = np.where(have, acc + rows[:, :, j, :], acc)
        n = (nrows[:, None] * ncols[None, :]).astype(np.float64)
        if is_float:
            return (acc / n).astype(a.dtype)
        return np.rint(acc.astype(np.float64) / n).astype(a.dtype)
