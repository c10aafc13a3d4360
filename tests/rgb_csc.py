"""The RGB -> YUV conversion of include/dsv2_hip.h (packed BGRA / RGBA surfaces as encoder input) in numpy: the oracle of
tests/test_gpu_enc_rgb.py, pinned to the kernel's text and to the C restatement by tests/test_ingest_rgb_cpu.py.

Y(x,y)   = (yr*R + yg*G + yb*B + 128 + 256*ybase) >> 8
U(cx,cy) = min(255, (SUM over the footprint of (ur*R + ug*G + ub*B) + N*32896) >> (8 + hs + vs)),  N = 1 << (hs + vs); V likewise
The footprint of (cx, cy) is (1 << hs) x (1 << vs) pixels from (cx << hs, cy << vs), coordinates clamped to w - 1 and h - 1.
"""
import numpy as np

BGRA, RGBA = 0x10, 0x11
BT601, BT709, FULL = 0x000, 0x100, 0x200
CSC = (BT601, BT709, BT601 | FULL, BT709 | FULL)

#          yr   yg  yb     ur   ug   ub     vr    vg   vb
MATRIX = {BT601: ((66, 129, 25), (-38, -74, 112), (112, -94, -18)),
          BT709: ((47, 157, 16), (-26, -86, 112), (112, -102, -10)),
          BT601 | FULL: ((77, 150, 29), (-43, -85, 128), (128, -107, -21)),
          BT709 | FULL: ((54, 183, 19), (-29, -99, 128), (128, -116, -12))}


def ybase(csc):
    return 0 if csc & FULL else 16


def weighted(row, r, g, b):
    return row[0] * r.astype(np.int64) + row[1] * g.astype(np.int64) + row[2] * b.astype(np.int64)


def luma(csc, r, g, b):
    return (weighted(MATRIX[csc][0], r, g, b) + 128 + 256 * ybase(csc)) >> 8


def chroma_sum(total, n_log2):
    """a chroma sample from the sum of its footprint's weighted colours (1 << n_log2 pixels)"""
    return np.minimum(255, (total + (32896 << n_log2)) >> (8 + n_log2))


def convert(pixels, layout, hs, vs):
    """pixels: h x w x 4 uint8 in the surface's byte order; layout: BGRA / RGBA or-ed with CSC bits.  Returns Y (h x w), U, V (ch x cw)."""
    order, csc = layout & ~0x300, layout & 0x300
    assert order in (BGRA, RGBA) and pixels.ndim == 3 and pixels.shape[2] == 4 and pixels.dtype == np.uint8
    h, w = pixels.shape[:2]
    r, g, b = (pixels[..., 2 if order == BGRA else 0], pixels[..., 1], pixels[..., 0 if order == BGRA else 2])
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    out = [luma(csc, r, g, b).astype(np.uint8)]
    for row in MATRIX[csc][1:]:
        t = np.pad(weighted(row, r, g, b), ((0, (ch << vs) - h), (0, (cw << hs) - w)), mode="edge")  # the clamp: edge pixels again
        t = t.reshape(ch, 1 << vs, cw, 1 << hs).sum(axis=(1, 3))
        assert t.min() + (32896 << (hs + vs)) >= 0
        out.append(chroma_sum(t, hs + vs).astype(np.uint8))
    return out


def planar_bytes(pixels, layout, hs, vs):
    """the packed planar picture (Y, U, V back to back) dsv_enc takes"""
    return b"".join(p.tobytes() for p in convert(pixels, layout, hs, vs))
