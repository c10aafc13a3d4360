"""The numpy oracle of half, quarter and eighth-size delivery (include/dsv2_hip.h, DSV2HIP_SCALE_*), written from the header's
formula and from nothing else: with n = 1 << s, a plane P of pw x ph becomes ceil(pw / n) x ceil(ph / n), and

    out(x, y) = (SUM j<n, i<n  P(min(x*n + i, pw-1), min(y*n + j, ph-1))  +  (1 << (2*s - 1))) >> (2*s)

-- a box average with one rounding over the whole footprint; a footprint across the right or bottom edge repeats the edge pixel.
"""
import numpy as np


def reduced_size(v, s):
    return (v + (1 << s) - 1) >> s


def reduce(plane, s):
    """plane: uint8 [ph, pw]; s: the shift, 0 .. 3.  Returns the reduced plane, uint8 [ceil(ph / n), ceil(pw / n)]."""
    plane = np.asarray(plane)
    assert plane.dtype == np.uint8 and plane.ndim == 2 and 0 <= s <= 3
    if s == 0:
        return plane.copy()
    n = 1 << s
    ph, pw = plane.shape
    oh, ow = reduced_size(ph, s), reduced_size(pw, s)
    ys = np.minimum(np.arange(oh * n), ph - 1)  # the clamp of the formula, as an index list
    xs = np.minimum(np.arange(ow * n), pw - 1)
    wide = plane[np.ix_(ys, xs)].astype(np.int64)
    total = wide.reshape(oh, n, ow, n).sum(axis=(1, 3))
    assert total.max() <= 64 * 255
    out = (total + (1 << (2 * s - 1))) >> (2 * s)
    return out.astype(np.uint8)


def reduce_picture(y, u, v, s):
    """each plane on its own"""
    return [reduce(p, s) for p in (y, u, v)]


def interleave(u, v):
    """the semiplanar chroma plane: rows U0 V0 U1 V1 ..."""
    out = np.empty((u.shape[0], 2 * u.shape[1]), dtype=np.uint8)
    out[:, 0::2], out[:, 1::2] = u, v
    return out
