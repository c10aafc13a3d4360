"""Planar RGB tensors as decoder output (dsv2hip_out_tensor of include/dsv2_hip.h) in numpy: the oracle of
tests/test_gpu_dec_tensor.py, pinned to the kernel's text and to the C restatement by tests/test_egress_rgb_cpu.py.  Built on
tests/yuv_rgb.py (THE CONVERSION) and tests/area_resize.py (THE RESAMPLING); what is its own is the float contract:

    f = fl32(fl32(float(v) * scale[c]) + bias[c])       two binary32 operations, not fused
    F32 stores f, F16 f rounded to binary16 (nearest even, subnormals kept, overflow to infinity), BF16 f rounded to bfloat16
    (nearest even: (bits + 0x7fff + ((bits >> 16) & 1)) >> 16)

Planes come back as uint8 (U8) or as the elements' bit patterns, uint16 (F16, BF16) / uint32 (F32).
"""
import numpy as np

import area_resize as R
import yuv_rgb as Q

U8, F16, BF16, F32 = 0, 1, 2, 3
DTYPES = (U8, F16, BF16, F32)
NAMES = {U8: "u8", F16: "f16", BF16: "bf16", F32: "f32"}
ELEM = {U8: 1, F16: 2, BF16: 2, F32: 4}
BITS = {U8: np.uint8, F16: np.uint16, BF16: np.uint16, F32: np.uint32}

UNIT = ((1 / 255,) * 3, (0.0,) * 3)
IMAGENET = (tuple(1 / (255 * s) for s in (0.229, 0.224, 0.225)), tuple(-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))))
TINY = ((1e-7,) * 3, (0.0,) * 3)      # binary16 subnormals and zeros
HUGE = ((300.0,) * 3, (-5.0,) * 3)    # binary16 overflow to infinity


def elements(v, dtype, scale, bias):
    """the bit patterns plane elements hold for the bytes v (any shape) under one plane's constants"""
    v = np.asarray(v)
    assert v.dtype == np.uint8
    if dtype == U8:
        return v.copy()
    with np.errstate(over="ignore"):
        f = v.astype(np.float32) * np.float32(scale) + np.float32(bias)
        assert f.dtype == np.float32
        if dtype == F32:
            return f.view(np.uint32).copy()
        if dtype == F16:
            return f.astype(np.float16).view(np.uint16).copy()
    bits = f.view(np.uint32).astype(np.uint64)
    return ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def tensor(y, u, v, csc, hs, vs, dtype, scale=UNIT[0], bias=UNIT[1], size=None):
    """y: h x w, u, v: ch x cw uint8 planes of the picture as the decoder delivers it at full size; csc: Q.CSC bits; size: (out_w,
    out_h) or None.  Returns [R, G, B], each out_h x out_w of BITS[dtype]."""
    h, w = y.shape
    if size is not None and tuple(size) != (w, h):
        y, u, v = R.resize_picture(y, u, v, size[0], size[1], hs, vs)
        h, w = y.shape
    rgb = Q.rgb(csc, y, Q.upsample(u, hs, vs, w, h), Q.upsample(v, hs, vs, w, h))
    return [elements(p, dtype, scale[c], bias[c]) for c, p in enumerate(rgb)]
