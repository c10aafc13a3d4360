"""The dsv2hip_* ABI of include/dsv2_hip.h as the GPU tests call it, declared once: the ctypes structures, the constants that go
into a layout word, one bind() with the prototype of every dsv2hip_* function the delivery / ingest tests call, and the small
readers (statistics, plane sizes) with their reset-everything helpers.  The dsv_* codec API and its structures are tests/dsvabi.py's."""
import ctypes as C

import dsvabi as A
from rgb3_csc import BGR, RGB, RGBP  # noqa: F401  DSV2HIP_SURFACE_BGR, _RGB, _RGBP, as the oracle of that conversion names them
from rgb_csc import BGRA, BT601, BT709, CSC, FULL, RGBA  # noqa: F401  DSV2HIP_SURFACE_BGRA, _RGBA and DSV2HIP_CSC_*, likewise

PLANAR, SEMI = 0, 1  # DSV2HIP_SURFACE_PLANAR, _SEMIPLANAR
HALF, QUARTER, EIGHTH = 0x1000, 0x2000, 0x3000  # DSV2HIP_SCALE_*
SCALE = {0: 0, 1: HALF, 2: QUARTER, 3: EIGHTH}  # by shift
NO_FN = 0xFFFFFFFF  # fn[k] of a DSV_DEC_OK that delivered nothing
GUARD = 0xA5        # what the tests fill around every plane they hand over
LEAD = 64           # guard bytes in front of and behind every plane
# (the decoder's return codes are dsvabi's DEC_*; a call refused as a whole returns -1, which the tests write as such)


class SURFACE(C.Structure):  # dsv2hip_surface
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("layout", C.c_int)]


class OUTSURF(C.Structure):  # dsv2hip_out_surface
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("cap", C.c_size_t * 3), ("layout", C.c_int)]


class OUTTENSOR(C.Structure):  # dsv2hip_out_tensor
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("cap", C.c_size_t * 3), ("dtype", C.c_int), ("csc", C.c_int), ("out_w", C.c_int),
                ("out_h", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


def _prototypes():
    P = C.POINTER
    i, sz, vp = C.c_int, C.c_size_t, C.c_void_p
    ENC, DEC, BUF = P(A.ENCODER), P(A.DECODER), P(A.BUF)
    ints, sizes, fns, stats = P(i), P(sz), P(C.c_uint32), [P(C.c_ulonglong), i]
    # name: (argtypes, restype); a restype the tests have never declared is not in the tuple
    return {
        # encoder
        "dsv2hip_enc_device_frame": ([ENC, vp, BUF], i),
        "dsv2hip_enc_batch": ([i, P(ENC), P(vp), BUF, ints], i),
        "dsv2hip_enc_batch_host": ([i, P(ENC), P(vp), P(vp), BUF, ints], i),
        "dsv2hip_enc_batch_surface": ([i, P(ENC), P(SURFACE), BUF, ints], i),
        "dsv2hip_enc_surface_frame": ([ENC, P(SURFACE), BUF], i),
        "dsv2hip_enc_batch_surface_scaled": ([i, P(ENC), P(SURFACE), ints, ints, BUF, ints], i),
        "dsv2hip_enc_surface_frame_scaled": ([ENC, P(SURFACE), i, i, BUF], i),
        "dsv2hip_enc_scaled_dims": ([i, i, i, i, ints, ints, sizes, ints], i),
        "dsv2hip_enc_batch_surface_sized": ([i, P(ENC), P(SURFACE), ints, ints, BUF, ints], i),
        "dsv2hip_enc_surface_frame_sized": ([ENC, P(SURFACE), i, i, BUF], i),
        "dsv2hip_enc_sized_dims": ([i, i, i, i, i, i, sizes, ints], i),
        "dsv2hip_enc_set_uyvy_input": ([ENC, i], i),
        "dsv2hip_enc_surface_stats": (stats, None),
        "dsv2hip_enc_rgb_stats": (stats, None),
        "dsv2hip_enc_rgb3_stats": (stats, None),
        "dsv2hip_enc_scale_stats": (stats, None),
        "dsv2hip_enc_resize_stats": (stats, None),
        "dsv2hip_enc_list_growths": (None, C.c_long),
        "dsv2hip_enc_ent_flag_count": ([i], C.c_long),
        "dsv2hip_seam_set_gpu_entropy": ([i], i),
        "dsv2hip_seam_set_field": ([ENC, vp, i, i, i, i, C.c_uint], i),
        "dsv2hip_enc_side_flag_count": ([], C.c_long),
        "dsv2hip_host_alloc": ([sz], vp),
        "dsv2hip_host_free": ([vp],),
        # decoder
        "dsv2hip_dec_set_out420p": ([DEC, i], i),
        "dsv2hip_dec_set_postsharp": ([DEC, i], i),
        "dsv2hip_dec_set_parse_mode": ([i], i),
        "dsv2hip_dec_batch": ([i, P(DEC), BUF, P(P(A.FRAME)), fns, ints], i),
        "dsv2hip_dec_picture_bytes": ([DEC], sz),
        "dsv2hip_dec_batch_device": ([i, P(DEC), BUF, P(vp), sizes, fns, ints], i),
        "dsv2hip_dec_device_frame": ([DEC, BUF, vp, sz, fns], i),
        "dsv2hip_dec_surface_dims": ([DEC, i, sizes, ints], i),
        "dsv2hip_dec_batch_surface": ([i, P(DEC), BUF, P(OUTSURF), fns, ints], i),
        "dsv2hip_dec_surface_frame": ([DEC, BUF, P(OUTSURF), fns], i),
        "dsv2hip_dec_sized_dims": ([DEC, i, i, i, sizes, ints], i),
        "dsv2hip_dec_batch_surface_sized": ([i, P(DEC), BUF, P(OUTSURF), ints, ints, fns, ints], i),
        "dsv2hip_dec_surface_frame_sized": ([DEC, BUF, P(OUTSURF), i, i, fns], i),
        "dsv2hip_dec_tensor_dims": ([DEC, i, i, i, sizes, ints], i),
        "dsv2hip_dec_batch_tensor": ([i, P(DEC), BUF, P(OUTTENSOR), fns, ints], i),
        "dsv2hip_dec_tensor_frame": ([DEC, BUF, P(OUTTENSOR), fns], i),
        "dsv2hip_dec_surface_stats": (stats, None),
        "dsv2hip_dec_rgb_stats": (stats, None),
        "dsv2hip_dec_scale_stats": (stats, None),
        "dsv2hip_dec_resize_stats": (stats, None),
        "dsv2hip_dec_tensor_stats": (stats, None),
        "dsv2hip_dec_queue_stats": (stats, None),
    }


def bind(hip):
    """argtypes and restype of every dsv2hip_* function the GPU tests call; idempotent; returns hip"""
    for name, proto in _prototypes().items():
        f = getattr(hip, name)
        if proto[0] is not None:
            f.argtypes = proto[0]
        if len(proto) > 1:
            f.restype = proto[1]
    return hip


PARSE_IDS = {0: "host-parse", 1: "P-on-device", 2: "device-parse"}


class parse_mode:
    """dsv2hip_dec_set_parse_mode for the pictures handed over inside the block"""

    def __init__(self, mode):
        self.hip, self.mode = bind(A.load_hip()), mode

    def __enter__(self):
        if self.mode is not None:
            assert self.hip.dsv2hip_dec_set_parse_mode(self.mode) == self.mode
        return self.hip

    def __exit__(self, *a):
        self.hip.dsv2hip_dec_set_parse_mode(-1)


def mk_buf(hip, buf, pk):
    """buf: a DSV_BUF that owns a copy of packet pk (the decoder frees it)"""
    hip.dsv_mk_buf(C.byref(buf), len(pk) + 64)
    C.memmove(buf.data, pk, len(pk))


# ---- the statistics: (wide, general) rounds or steps since the last reset; four counters where the header says out4 ----------------
def _forms(name, n):
    def forms(hip, reset=False):
        out = (C.c_ulonglong * n)()
        getattr(hip, name)(out, int(reset))
        return tuple(out)
    forms.__doc__ = "%s as a tuple of %d" % (name, n)
    return forms


dec_uv_forms = _forms("dsv2hip_dec_surface_stats", 2)
dec_rgb_forms = _forms("dsv2hip_dec_rgb_stats", 2)
dec_scale_forms = _forms("dsv2hip_dec_scale_stats", 2)
dec_resize_forms = _forms("dsv2hip_dec_resize_stats", 2)
dec_tensor_forms = _forms("dsv2hip_dec_tensor_stats", 2)
enc_yuv_forms = _forms("dsv2hip_enc_surface_stats", 2)
enc_rgb_forms = _forms("dsv2hip_enc_rgb_stats", 2)
enc_rgb3_forms = _forms("dsv2hip_enc_rgb3_stats", 4)
enc_scale_forms = _forms("dsv2hip_enc_scale_stats", 4)
enc_resize_forms = _forms("dsv2hip_enc_resize_stats", 4)


def reset_dec_forms(hip):
    """every statistic of the decoder's deliveries back to zero"""
    for forms in (dec_uv_forms, dec_rgb_forms, dec_scale_forms, dec_resize_forms, dec_tensor_forms):
        forms(hip, reset=True)


def reset_enc_forms(hip):
    """every statistic of the encoder's ingests back to zero"""
    for forms in (enc_yuv_forms, enc_rgb_forms, enc_rgb3_forms, enc_scale_forms, enc_resize_forms):
        forms(hip, reset=True)


# ---- the plane sizes the decoder reports ------------------------------------------------------------------------------------------
def surface_dims(hip, dec, layout):
    """[(row bytes, rows)] of the planes of `layout` as the decoder reports them, or None (no metadata yet, or no such layout)"""
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    if hip.dsv2hip_dec_surface_dims(C.byref(dec), layout, rb, rows) != 0:
        return None
    return [(rb[c], rows[c]) for c in range(3)]


def sized_dims(hip, dec, layout, ow, oh):
    """the same for a sized entry of out_w x out_h"""
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    if hip.dsv2hip_dec_sized_dims(C.byref(dec), layout, ow, oh, rb, rows) != 0:
        return None
    return [(rb[c], rows[c]) for c in range(3)]


def tensor_dims(hip, dec, dtype, ow=0, oh=0):
    """(row bytes, rows) of one plane of a tensor as the decoder reports them, or None"""
    rb, rows = C.c_size_t(0), C.c_int(0)
    if hip.dsv2hip_dec_tensor_dims(C.byref(dec) if dec is not None else None, dtype, ow, oh, C.byref(rb), C.byref(rows)) != 0:
        return None
    return rb.value, rows.value
