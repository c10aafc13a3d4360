"""The numpy oracle of half, quarter and eighth-size ingest (include/dsv2_hip.h, dsv2hip_enc_batch_surface_scaled), written from
the header's text alone.  With s the shift and n = 1 << s, a source of src_w x src_h feeds an encoder of ceil(src_w / n) x
ceil(src_h / n):

YUV surfaces: each SOURCE plane on its own through the decoder's reduction (tests/box_reduce.py); a semiplanar chroma plane is
de-interleaved first.

RGB surfaces: the plain conversion (tests/rgb_csc.py) with every footprint enlarged by the scale and one rounding per sample:
    Y'(x,y)   = (SUM n x n of (yr*R + yg*G + yb*B) + ((128 + 256*ybase) << 2s)) >> (8 + 2s)
    U'(cx,cy) = min(255, (SUM (n << hs) x (n << vs) of (ur*R + ug*G + ub*B) + (32896 << (hs + vs + 2s))) >> (8 + hs + vs + 2s))
footprints from (x*n, y*n) / (cx << (hs + s), cy << (vs + s)), source coordinates clamped to src_w - 1, src_h - 1.
"""
import numpy as np

import box_reduce as B
import rgb_csc as R

PLANAR, SEMI = 0, 1
SCALE = (0, 0x1000, 0x2000, 0x3000)


def up(v, s):
    return (v + (1 << s) - 1) >> s


def source_dims(src_w, src_h, hs, vs, kind):
    """[(row bytes, rows)] of the source planes; kind: PLANAR, SEMI or "rgb" """
    scw, sch = up(src_w, hs), up(src_h, vs)
    if kind == "rgb":
        return [(4 * src_w, src_h)]
    if kind == SEMI:
        return [(src_w, src_h), (2 * scw, sch)]
    return [(src_w, src_h), (scw, sch), (scw, sch)]


def split_planar(frame, src_w, src_h, hs, vs):
    """a packed planar picture (bytes) as its three uint8 planes"""
    flat = np.frombuffer(frame, dtype=np.uint8)
    out, at = [], 0
    for rb, rows in source_dims(src_w, src_h, hs, vs, PLANAR):
        out.append(flat[at:at + rb * rows].reshape(rows, rb))
        at += rb * rows
    assert at == flat.size
    return out


def deinterleave(uv):
    return uv[:, 0::2], uv[:, 1::2]


def reduce_yuv(planes, s):
    """planes: Y, U, V of the source, or Y and the interleaved UV plane.  Returns the encoder's Y, U, V."""
    if len(planes) == 2:
        u, v = deinterleave(np.asarray(planes[1]))
        planes = [planes[0], np.ascontiguousarray(u), np.ascontiguousarray(v)]
    return [B.reduce(np.ascontiguousarray(p), s) for p in planes]


def footprint_sum(t, fw_log2, fh_log2):
    """t: int64 [h, w]; sums over footprints of (1 << fw_log2) x (1 << fh_log2) from (cx << fw_log2, cy << fh_log2), coordinates clamped"""
    h, w = t.shape
    ow, oh = up(w, fw_log2), up(h, fh_log2)
    t = np.pad(t, ((0, (oh << fh_log2) - h), (0, (ow << fw_log2) - w)), mode="edge")
    return t.reshape(oh, 1 << fh_log2, ow, 1 << fw_log2).sum(axis=(1, 3))


def convert_scaled(pixels, layout, hs, vs, s):
    """pixels: src_h x src_w x 4 uint8 in the surface's byte order; layout: BGRA / RGBA or-ed with CSC bits (no scale value).
    Returns the encoder's Y, U, V."""
    order, csc = layout & ~0x300, layout & 0x300
    assert order in (R.BGRA, R.RGBA) and pixels.ndim == 3 and pixels.shape[2] == 4 and pixels.dtype == np.uint8 and 0 <= s <= 3
    r, g, b = (pixels[..., 2 if order == R.BGRA else 0], pixels[..., 1], pixels[..., 0 if order == R.BGRA else 2])
    m = R.MATRIX[csc]
    ysum = footprint_sum(R.weighted(m[0], r, g, b), s, s)
    out = [((ysum + ((128 + 256 * R.ybase(csc)) << (2 * s))) >> (8 + 2 * s)).astype(np.uint8)]
    for row in m[1:]:
        t = footprint_sum(R.weighted(row, r, g, b), hs + s, vs + s)
        assert t.min() + (32896 << (hs + vs + 2 * s)) >= 0 and np.abs(t).max() <= 1024 * 255 * 128
        out.append(R.chroma_sum(t, hs + vs + 2 * s).astype(np.uint8))
    return out


def packed(planes):
    return b"".join(np.ascontiguousarray(p).tobytes() for p in planes)
