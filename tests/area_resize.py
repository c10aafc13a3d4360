"""The numpy oracle of delivery at any smaller size (include/dsv2_hip.h, dsv2hip_dec_batch_surface_sized), written from the header's
formula and from nothing else: a plane P of pw x ph becomes ow x oh; with g = gcd(pw, ow), a = pw / g, b = ow / g, source pixel i
covers [i*b, (i+1)*b), output sample x covers [x*a, (x+1)*a),

    wx(x, i) = max(0, min((i+1)*b, (x+1)*a) - max(i*b, x*a))

and the same vertically (c, d, wy); with D = a * c

    out(x, y) = (SUM_j SUM_i wy(y,j) * wx(x,i) * P(i, j)  +  D // 2) // D

-- the direct double sum, as a product of two weight matrices, in exact integers.
"""
from math import gcd

import numpy as np

MAX_D = 1 << 24
MAX_SIDE = 32768
# the plane sizes (pw, ph, ow, oh) that the sweeps of tools/egress_resize_check.cpp and tools/ingest_resize_check.cpp must hold
SWEEP_SHAPES = [(48, 32, 32, 24), (50, 38, 33, 21), (25, 19, 17, 11), (64, 48, 9, 7), (64, 48, 64, 6), (64, 48, 8, 48), (16, 16, 16, 16),
                (16, 16, 2, 2), (64, 48, 32, 24), (64, 48, 16, 12), (97, 61, 13, 8), (131, 67, 130, 66)]


def ratio(src, dst):
    """(a, b): src / dst in lowest terms"""
    g = gcd(src, dst)
    return src // g, dst // g


def weights(src, dst):
    """int64 [dst, src]: row x holds wx(x, i) for every source pixel i"""
    a, b = ratio(src, dst)
    x = np.arange(dst, dtype=np.int64)[:, None]
    i = np.arange(src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * b, (x + 1) * a) - np.maximum(i * b, x * a))


def allowed(pw, ph, ow, oh):
    """the bounds of the call for one plane"""
    if not (0 < ow <= pw <= 8 * ow and 0 < oh <= ph <= 8 * oh and pw <= MAX_SIDE and ph <= MAX_SIDE):
        return False
    return ratio(pw, ow)[0] * ratio(ph, oh)[0] <= MAX_D


def resize(plane, ow, oh):
    """plane: uint8 [ph, pw].  Returns the resampled plane, uint8 [oh, ow]."""
    plane = np.asarray(plane)
    assert plane.dtype == np.uint8 and plane.ndim == 2
    ph, pw = plane.shape
    assert allowed(pw, ph, ow, oh), (pw, ph, ow, oh)
    D = ratio(pw, ow)[0] * ratio(ph, oh)[0]
    total = weights(ph, oh) @ plane.astype(np.int64) @ weights(pw, ow).T
    assert total.max() <= 255 * D
    return ((total + D // 2) // D).astype(np.uint8)


def plane_sizes(out_w, out_h, hs, vs):
    """[(w, h)] * 3 of the delivered picture: dsv_mk_frame's for out_w x out_h with chroma shifts hs, vs"""
    cw, ch = (out_w + (1 << hs) - 1) >> hs, (out_h + (1 << vs) - 1) >> vs
    return [(out_w, out_h), (cw, ch), (cw, ch)]


def resize_picture(y, u, v, out_w, out_h, hs, vs):
    """each plane on its own, by its own ratio"""
    return [resize(p, w, h) for p, (w, h) in zip((y, u, v), plane_sizes(out_w, out_h, hs, vs))]
