"""The YUV -> RGB conversion of include/dsv2_hip.h (packed BGRA / RGBA surfaces as decoder output) in numpy: the oracle of
tests/test_gpu_dec_rgb.py, pinned to the kernel's text and to the C restatement by tests/test_egress_rgb_cpu.py.  The counterpart
of tests/rgb_csc.py, whose layout constants it shares.

C = ky * (Y - ybase),  D = U - 128,  E = V - 128
R = clamp((C + rv*E + 128) >> 8),  G = clamp((C + gu*D + gv*E + 128) >> 8),  B = clamp((C + bu*D + 128) >> 8)     (>> floors)
The chroma of pixel (x, y) is the sample (x >> hs, y >> vs).
"""
import numpy as np

from rgb_csc import BGRA, BT601, BT709, CSC, FULL, RGBA  # noqa: F401  (the layout constants are the encoder's)

#                 ky ybase   rv    gu    gv   bu
COEFS = {BT601: (298, 16, 409, -100, -208, 516),
         BT709: (298, 16, 459, -55, -136, 541),
         BT601 | FULL: (256, 0, 359, -88, -183, 454),
         BT709 | FULL: (256, 0, 403, -48, -120, 475)}


def sums(csc, y, u, v):
    """the three sums before their shift (R, G, B), int64, for samples of equal shape"""
    ky, ybase, rv, gu, gv, bu = COEFS[csc]
    c = ky * (y.astype(np.int64) - ybase)
    d, e = u.astype(np.int64) - 128, v.astype(np.int64) - 128
    return c + rv * e + 128, c + gu * d + gv * e + 128, c + bu * d + 128


def rgb(csc, y, u, v):
    """R, G, B (uint8) of samples of equal shape"""
    return tuple(np.clip(s >> 8, 0, 255).astype(np.uint8) for s in sums(csc, y, u, v))


def upsample(plane, hs, vs, w, h):
    """chroma sample (x >> hs, y >> vs) for every pixel of the w x h picture"""
    return np.repeat(np.repeat(plane, 1 << vs, axis=0), 1 << hs, axis=1)[:h, :w]


def convert(y, u, v, layout, hs, vs):
    """y: h x w, u, v: ch x cw uint8 planes; layout: BGRA / RGBA or-ed with CSC bits.  Returns h x w x 4 uint8 in the surface's byte order."""
    order, csc = layout & ~0x300, layout & 0x300
    assert order in (BGRA, RGBA) and y.dtype == u.dtype == v.dtype == np.uint8
    h, w = y.shape
    assert u.shape == v.shape == ((h + (1 << vs) - 1) >> vs, (w + (1 << hs) - 1) >> hs)
    r, g, b = rgb(csc, y, upsample(u, hs, vs, w, h), upsample(v, hs, vs, w, h))
    alpha = np.full_like(r, 255)
    return np.stack([b, g, r, alpha] if order == BGRA else [r, g, b, alpha], axis=-1)
