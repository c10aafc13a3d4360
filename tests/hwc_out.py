"""Interleaved RGB tensors as decoder output (dsv2hip_out_hwc of include/dsv2_hip.h): the ctypes structure and prototypes on top of
hipabi.bind, the numpy oracle, a holder with guard bytes and the target description that plugs into dec_out.decode_steps.

The oracle is tests/tensor_out.py's, interleaved: element k of a pixel is the channel the order puts there (R G B, or B G R), and the
constants belong to memory positions, so a BGR tensor's scale[k] / bias[k] are those of channel (B, G, R)[k].  Pictures come back as
h x w x 3 arrays of the elements' bit patterns (tensor_out.BITS)."""
import ctypes as C

import numpy as np
import torch

import dsvabi as A
import tensor_out as T
from codec_run import FMT
from dec_out import TORCH_INT, Surfaces
from hipabi import GUARD, LEAD, bind as bind_abi

BGR, RGB = 0x20, 0x21  # DSV2HIP_SURFACE_BGR, _RGB: the element orders
ORDERS = (RGB, BGR)
ORDER_NAMES = {RGB: "rgb", BGR: "bgr"}


class OUTHWC(C.Structure):  # dsv2hip_out_hwc
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_size_t), ("cap", C.c_size_t), ("dtype", C.c_int), ("order", C.c_int), ("csc", C.c_int),
                ("out_w", C.c_int), ("out_h", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


def bind(hip):
    """hipabi.bind plus the prototypes of the interleaved tensor calls; idempotent; returns hip"""
    bind_abi(hip)
    P = C.POINTER
    i, sz = C.c_int, C.c_size_t
    DEC, BUF = P(A.DECODER), P(A.BUF)
    protos = {
        "dsv2hip_dec_hwc_dims": ([DEC, i, i, i, P(sz), P(i)], i),
        "dsv2hip_dec_batch_hwc": ([i, P(DEC), BUF, P(OUTHWC), P(C.c_uint32), P(i)], i),
        "dsv2hip_dec_hwc_frame": ([DEC, BUF, P(OUTHWC), P(C.c_uint32)], i),
        "dsv2hip_dec_hwc_stats": ([P(C.c_ulonglong), i], None),
    }
    for name, (args, res) in protos.items():
        f = getattr(hip, name)
        f.argtypes, f.restype = args, res
    return hip


def hwc_forms(hip, reset=False):
    """dsv2hip_dec_hwc_stats as a tuple of 2: (wide, general) rounds since the last reset"""
    out = (C.c_ulonglong * 2)()
    hip.dsv2hip_dec_hwc_stats(out, int(reset))
    return tuple(out)


def hwc_dims(hip, dec, dtype, ow=0, oh=0):
    """(row bytes, rows) of an interleaved tensor as the decoder reports them, or None"""
    rb, rows = C.c_size_t(0), C.c_int(0)
    if hip.dsv2hip_dec_hwc_dims(C.byref(dec) if dec is not None else None, dtype, ow, oh, C.byref(rb), C.byref(rows)) != 0:
        return None
    return rb.value, rows.value


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
def channel_of(order):
    """the channel (0 R, 1 G, 2 B) of element k, k = 0, 1, 2"""
    return (0, 1, 2) if order == RGB else (2, 1, 0)


def hwc(y, u, v, csc, hs, vs, dtype, order, scale=T.UNIT[0], bias=T.UNIT[1], size=None):
    """the interleaved tensor of a picture delivered as planes y, u, v at full size: out_h x out_w x 3 of tensor_out.BITS[dtype]; scale /
    bias per ELEMENT position"""
    ch = channel_of(order)
    by_channel = [None] * 3
    for k in range(3):
        by_channel[ch[k]] = k
    planes = T.tensor(y, u, v, csc, hs, vs, dtype, [scale[by_channel[c]] for c in range(3)], [bias[by_channel[c]] for c in range(3)], size)
    return np.stack([planes[ch[k]] for k in range(3)], axis=-1)


def hwc_expected(results, fmt, sp):
    """planar results [(code, fn, [Y, U, V] or None)] as the interleaved tensor of spec sp"""
    _, hs, vs = FMT[fmt]
    return [(code, fn if pl is not None else None,
             None if pl is None else hwc(pl[0], pl[1], pl[2], sp["csc"], hs, vs, sp["dtype"], sp["order"], sp["consts"][0], sp["consts"][1], sp["size"]))
            for code, fn, pl in results]


def spec(dtype, order=RGB, csc=0, pitch=None, offset=0, consts=T.UNIT, size=None):
    """an interleaved tensor: element type, order, CSC bits, pitch as a function of (row bytes, element size) -- dec_out's policies;
    None: tight --, pointer offset in ELEMENTS behind a 16-byte boundary, (scale[3], bias[3]) by element position, size or None"""
    return dict(dtype=dtype, order=order, csc=csc, pitch=pitch or (lambda rb, elem=1: rb), offset=offset, consts=consts, size=size)


# ---- the holder -----------------------------------------------------------------------------------------------------------------------
class OutHwc:
    """One decoder's interleaved tensor: LEAD guard bytes, `offset` elements more, the rows pitch apart (the last one without padding),
    LEAD guard bytes; cap is exactly what the rows need."""

    def __init__(self, dims, dtype, order, csc, pitch, offset, consts, size):
        rb, rows = dims
        self.dtype, self.elem, self.rb, self.rows = dtype, T.ELEM[dtype], rb, rows
        self.p = pitch(rb, self.elem)
        need = (rows - 1) * self.p + rb
        self.start = LEAD + offset * self.elem
        self.t = torch.empty(self.start + need + LEAD, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.inside = np.zeros(self.t.numel(), dtype=bool)
        for y in range(rows):
            self.inside[self.start + y * self.p:self.start + y * self.p + rb] = True
        self.c = OUTHWC()
        self.c.data, self.c.pitch, self.c.cap = self.t.data_ptr() + self.start, self.p, need
        self.c.dtype, self.c.order, self.c.csc = dtype, order, csc
        self.c.out_w, self.c.out_h = size or (0, 0)
        for k in range(3):
            self.c.scale[k], self.c.bias[k] = consts[0][k], consts[1][k]

    def wide(self):
        """include/dsv2_hip.h at dsv2hip_dec_hwc_stats: data and pitch multiples of four elements, width of 4"""
        return self.start % (4 * self.elem) == 0 and self.p % (4 * self.elem) == 0 and (self.rb // (3 * self.elem)) % 4 == 0

    def arm(self):
        self.t.fill_(GUARD)

    def planes(self):
        """the picture, rows x w x 3 bit patterns read back through torch as integers of the element's width; asserts that every byte
        outside the rows -- in front, in the padding, behind the last row -- still holds the guard"""
        a = self.t.cpu().numpy()
        assert np.all(a[~self.inside] == GUARD), "bytes outside the rows were written"
        rows = torch.as_strided(self.t, (self.rows, self.rb), (self.p, 1), self.start).contiguous()
        return rows.view(TORCH_INT[self.elem]).cpu().numpy().view(T.BITS[self.dtype]).reshape(self.rows, -1, 3)

    def untouched(self):
        return bool(torch.all(self.t == GUARD))


# ---- the target description -----------------------------------------------------------------------------------------------------------
class Hwc(Surfaces):
    """dsv2hip_dec_batch_hwc / dsv2hip_dec_hwc_frame: spec() per stream"""
    batch, frame = "dsv2hip_dec_batch_hwc", "dsv2hip_dec_hwc_frame"

    def arrays(self, m):
        return ((OUTHWC * m)(),)

    def dims(self, hip, dec, k):
        return hwc_dims(bind(hip), dec, self.specs[k]["dtype"], *(self.specs[k]["size"] or (0, 0)))

    def expected(self, hip, dec, k, out420p):
        ow, oh = self.specs[k]["size"] or (dec.vidmeta.width, dec.vidmeta.height)
        return 3 * ow * T.ELEM[self.specs[k]["dtype"]], oh

    def make(self, dims, dec, k, out420p):
        return OutHwc(dims, **self.specs[k])


def same(want, got, what=""):
    """return codes, frame numbers and every element of every picture, the first differing one named"""
    assert [r[:2] for r in want] == [r[:2] for r in got], what
    for (_, fn, pw), (_, _, pg) in zip(want, got):
        assert (pw is None) == (pg is None), what
        if pw is None:
            continue
        assert pw.dtype == pg.dtype and pw.shape == pg.shape, (what, pw.dtype, pg.dtype, pw.shape, pg.shape)
        bad = np.argwhere(pw != pg)
        assert bad.size == 0, "%s frame %d: element %d of pixel (x=%d, y=%d) is %#x, the oracle gives %#x (%d differ)" % (
            what, fn, bad[0][2], bad[0][1], bad[0][0], pg[tuple(bad[0])], pw[tuple(bad[0])], len(bad))
