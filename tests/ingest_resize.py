"""The numpy oracle of ingest at any larger size (include/dsv2_hip.h, dsv2hip_enc_batch_surface_sized), written from the header's
text alone.  An encoder of W x H reads a source of src_w x src_h, W <= src_w <= 8 W and H <= src_h <= 8 H:

YUV surfaces: each SOURCE plane on its own through the header's resampling (tests/area_resize.py) to the encoder's plane; a
semiplanar chroma plane is de-interleaved first.

RGB surfaces: the packed picture is resampled as RGB and the matrix is applied to the weighted sums, one rounding per sample.
With w = wy * wx the weights of src_w x src_h -> ow x oh (W x H for luma, cw x ch for chroma), D = a * c of that resampling and
S_R = SUM w * R, S_G, S_B:
    Y'(x,y)   = (yr*S_R + yg*S_G + yb*S_B + (128 + 256*ybase) * D) // (256 * D)
    U'(cx,cy) = min(255, (ur*S_R + ug*S_G + ub*S_B + 32896 * Dc) // (256 * Dc)),   V' likewise
in exact (Python / int64) integers.
"""
import numpy as np

import area_resize as AR
import rgb_csc as R
from ingest_scale import PLANAR, SEMI, deinterleave, packed, source_dims, split_planar, up  # noqa: F401  (shared shapes)

RGB_MAX_D = 65535


def D_of(pw, ph, ow, oh):
    return AR.ratio(pw, ow)[0] * AR.ratio(ph, oh)[0]


def enc_planes(w, h, hs, vs):
    """[(w, h)] * 3 of the encoder's planes"""
    return AR.plane_sizes(w, h, hs, vs)


def allowed(src_w, src_h, w, h, hs, vs, rgb):
    """the bounds of a sized entry: per plane the resampling's (YUV); for RGB the luma resampling's, D <= 65 535 for the luma and for
    the chroma resampling of the packed picture, whose ratio may reach 8 << hs by 8 << vs"""
    if min(src_w, src_h, w, h) <= 0:
        return False
    (_, _), (cw, ch), _ = enc_planes(w, h, hs, vs)
    if rgb:
        return (AR.allowed(src_w, src_h, w, h) and D_of(src_w, src_h, w, h) <= RGB_MAX_D and
                cw <= src_w and ch <= src_h and D_of(src_w, src_h, cw, ch) <= RGB_MAX_D)
    scw, sch = up(src_w, hs), up(src_h, vs)
    return AR.allowed(src_w, src_h, w, h) and AR.allowed(scw, sch, cw, ch)


def resize_yuv(planes, w, h, hs, vs):
    """planes: Y, U, V of the source, or Y and the interleaved UV plane.  Returns the encoder's Y, U, V."""
    if len(planes) == 2:
        u, v = deinterleave(np.asarray(planes[1]))
        planes = [planes[0], np.ascontiguousarray(u), np.ascontiguousarray(v)]
    return [AR.resize(np.ascontiguousarray(p), ow, oh) for p, (ow, oh) in zip(planes, enc_planes(w, h, hs, vs))]


def weighted_sums(channel, ow, oh):
    """int64 [oh, ow]: SUM wy * wx * channel"""
    ph, pw = channel.shape
    return AR.weights(ph, oh) @ channel.astype(np.int64) @ AR.weights(pw, ow).T


def convert_sized(pixels, layout, w, h, hs, vs):
    """pixels: src_h x src_w x 4 uint8 in the surface's byte order; layout: BGRA / RGBA or-ed with CSC bits.  Returns the encoder's
    Y, U, V.  Every numerator is asserted non-negative and below 2^32, every divisor below 2^24."""
    order, csc = layout & ~0x300, layout & 0x300
    assert order in (R.BGRA, R.RGBA) and pixels.ndim == 3 and pixels.shape[2] == 4 and pixels.dtype == np.uint8
    sh, sw = pixels.shape[:2]
    assert allowed(sw, sh, w, h, hs, vs, True), (sw, sh, w, h)
    rgb = (pixels[..., 2 if order == R.BGRA else 0], pixels[..., 1], pixels[..., 0 if order == R.BGRA else 2])
    m = R.MATRIX[csc]
    out = []
    for c, (ow, oh) in enumerate(enc_planes(w, h, hs, vs)):
        D = D_of(sw, sh, ow, oh)
        s = [weighted_sums(ch, ow, oh) for ch in rgb]
        num = m[c][0] * s[0] + m[c][1] * s[1] + m[c][2] * s[2] + ((128 + 256 * R.ybase(csc)) if c == 0 else 32896) * D
        assert num.min() >= 0 and num.max() < 1 << 32 and 256 * D < 1 << 24
        v = num // (256 * D)
        out.append((v if c == 0 else np.minimum(v, 255)).astype(np.uint8))
        assert c != 0 or v.max() <= 255
    return out
