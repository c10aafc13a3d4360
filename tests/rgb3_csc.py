"""Three-byte and planar RGB surfaces (DSV2HIP_SURFACE_BGR / _RGB / _RGBP of include/dsv2_hip.h) in numpy: the oracle of
tests/test_gpu_enc_rgb3.py and tests/test_ingest_rgb3_cpu.py.  There is no conversion of its own here: the picture is widened to
four bytes a pixel -- an alpha channel appended to h x w x 3, the planes of 3 x h x w stacked -- and handed to tests/rgb_csc.py,
which is what the header promises ("exactly the packets that the same pixels give as an RGBA surface with any alpha").
"""
import numpy as np

import rgb_csc as R

BGR, RGB, RGBP = 0x20, 0x21, 0x22
ORDER = {"bgr": BGR, "rgb": RGB, "rgbp": RGBP}


def order_of(layout):
    return layout & ~0x300


def widen(pixels, layout, alpha=0):
    """the picture as h x w x 4 uint8 and the four-byte layout that names the same colours.  pixels: h x w x 3 in the surface's byte
    order (BGR / RGB) or 3 x h x w as R, G, B (RGBP); alpha: a value or an h x w array"""
    order, csc = order_of(layout), layout & 0x300
    assert pixels.dtype == np.uint8 and pixels.ndim == 3
    if order == RGBP:
        assert pixels.shape[0] == 3
        colours = np.stack([pixels[0], pixels[1], pixels[2]], axis=-1)
    else:
        assert order in (BGR, RGB) and pixels.shape[2] == 3
        colours = pixels
    h, w = colours.shape[:2]
    a = np.broadcast_to(np.asarray(alpha, dtype=np.uint8), (h, w))
    return np.concatenate([colours, a[..., None]], axis=-1), (R.BGRA if order == BGR else R.RGBA) | csc


def convert(pixels, layout, hs, vs):
    """Y (h x w), U, V (ch x cw) of the surface"""
    return R.convert(*widen(pixels, layout), hs, vs)


def planar_bytes(pixels, layout, hs, vs):
    """the packed planar picture (Y, U, V back to back) dsv_enc takes"""
    return b"".join(p.tobytes() for p in convert(pixels, layout, hs, vs))


def from_rgba(rgba, layout):
    """the surface of `layout` that holds the colours of an h x w x 4 R G B A picture"""
    order = order_of(layout)
    if order == RGBP:
        return np.ascontiguousarray(rgba[..., :3].transpose(2, 0, 1))
    return np.ascontiguousarray(rgba[..., 2::-1] if order == BGR else rgba[..., :3])
