"""Interleaved RGB float tensors as encoder input (dsv2hip_in_hwc of include/dsv2_hip.h): the numpy oracle of the contract, built on
tests/tensor_in.py's (picture, tensor_near, interleaved by the order), the ctypes descriptor with the three prototypes, a source
class that holds one tensor in device memory with guard bytes and padding around its rows, a wrapper for torch tensors read in place,
and the lockstep driver over dsv2hip_enc_batch_hwc.  Pinned to the kernel's text and to the C restatement by
tests/test_ingest_hwc_cpu.py; the GPU side is tests/test_gpu_enc_hwc.py.

    element k (k = 0, 1, 2 in memory order) of a pixel is the channel the order puts there: RGB R G B, BGR B G R
    g = fl32(fl32(e * scale[k]) + bias[k])              constants by MEMORY POSITION, as tests/hwc_out.py has them
    v = 0 where g is a NaN, else rint(min(max(g, 0), 255)), ties to even

Tensors travel as h x w x 3 arrays of the elements' bit patterns (tensor_out.BITS), as tests/hwc_out.py delivers them.
"""
import ctypes as C

import numpy as np

import dsvabi as A
import tensor_in as T
from tensor_in import BF16, BITS, ELEM, F16, F32, FLOATS, GUARD, LEAD, U8  # noqa: F401

BGR, RGB = 0x20, 0x21  # DSV2HIP_SURFACE_BGR, _RGB: the element orders (tests/hwc_out.py's)
ORDERS = (RGB, BGR)
ORDER_NAMES = {RGB: "rgb", BGR: "bgr"}


def channel_of(order):
    """the channel (0 R, 1 G, 2 B) of element k, k = 0, 1, 2"""
    return (0, 1, 2) if order == RGB else (2, 1, 0)


def by_position(per_channel, order):
    """a triple given per channel R, G, B as the triple per element position of `order` (its own inverse: both orders are involutions)"""
    return tuple(per_channel[c] for c in channel_of(order))


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def interleave(planes, order):
    """[R, G, B] planes (h x w each) as the h x w x 3 tensor of `order`"""
    return np.ascontiguousarray(np.stack([planes[c] for c in channel_of(order)], axis=-1))


def planes_of(hwc, order):
    """the other way: the h x w x 3 tensor's [R, G, B] planes"""
    ch = channel_of(order)
    out = [None] * 3
    for k in range(3):
        out[ch[k]] = np.ascontiguousarray(hwc[..., k])
    return out


def picture(hwc, dtype, order, scale, bias):
    """hwc: h x w x 3 bit patterns (uint8 for U8); scale, bias by POSITION.  Returns the h x w x 4 uint8 picture (R, G, B, alpha 0)
    whose RGBA | csc surface gives the tensor's packets: tensor_in.picture on the de-interleaved planes under the permuted constants."""
    return T.picture(planes_of(hwc, order), dtype, by_position(scale, order), by_position(bias, order))


def tensor_near(px4, dtype, order, scale, bias, seed):
    """an h x w x 3 tensor of `order` near the colour bytes of an h x w x 4 picture, for constants by POSITION"""
    return interleave(T.tensor_near(px4, dtype, by_position(scale, order), by_position(bias, order), seed), order)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
class INHWC(C.Structure):  # dsv2hip_in_hwc
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_size_t), ("dtype", C.c_int), ("order", C.c_int), ("csc", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


def bind(hip):
    """argtypes and restype of the three interleaved tensor entry points; idempotent; returns hip"""
    P = C.POINTER
    hip.dsv2hip_enc_batch_hwc.argtypes = [C.c_int, P(P(A.ENCODER)), P(INHWC), P(A.BUF), P(C.c_int)]
    hip.dsv2hip_enc_batch_hwc.restype = C.c_int
    hip.dsv2hip_enc_hwc_frame.argtypes = [P(A.ENCODER), P(INHWC), P(A.BUF)]
    hip.dsv2hip_enc_hwc_frame.restype = C.c_int
    hip.dsv2hip_enc_hwc_stats.argtypes = [P(C.c_ulonglong), C.c_int]
    hip.dsv2hip_enc_hwc_stats.restype = None
    return hip


def hwc_forms(hip, reset=False):
    """dsv2hip_enc_hwc_stats as a tuple of 2: steps in the wide / in the general form"""
    out = (C.c_ulonglong * 2)()
    hip.dsv2hip_enc_hwc_stats(out, int(reset))
    return tuple(out)


def descriptor(ptr, pitch, dtype, order, csc, scale, bias):
    c = INHWC()
    c.data, c.pitch, c.dtype, c.order, c.csc = ptr, pitch, dtype, order, csc
    for k in range(3):
        c.scale[k], c.bias[k] = scale[k], bias[k]
    return c


def copy_of(c):
    d = INHWC()
    C.memmove(C.byref(d), C.byref(c), C.sizeof(c))
    return d


# ---- sources in device memory (torch is imported where a GPU test asks for one) -------------------------------------------------------
class HwcIn:
    """an h x w x 3 tensor (bit patterns) as one device allocation: LEAD guard bytes, `offset` ELEMENTS more, h rows `pitch` bytes apart
    (the last one without padding), LEAD guard bytes; guard and padding hold `fill` (None: noise).  `check_untouched` compares every
    byte with what was put there."""

    def __init__(self, hwc, dtype, order, csc, scale, bias, pitch, offset=0, fill=GUARD):
        import torch
        elem = ELEM[dtype]
        h, w, three = hwc.shape
        rb = 3 * w * elem
        assert three == 3 and pitch >= rb and hwc.dtype == BITS[dtype]
        start = LEAD + offset * elem
        size = start + (h - 1) * pitch + rb + LEAD
        if fill is None:
            t = torch.from_numpy(np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8)).cuda()
        else:
            t = torch.full((size,), fill, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        rows = np.ascontiguousarray(hwc).view(np.uint8).reshape(h, rb)
        torch.as_strided(t, (h, rb), (pitch, 1), start).copy_(torch.from_numpy(rows).cuda())
        self.t, self.was = t, t.clone()
        self.c = descriptor(t.data_ptr() + start, pitch, dtype, order, csc, scale, bias)

    def check_untouched(self):
        import torch
        assert torch.equal(self.t, self.was), "the encoder wrote into a tensor"


class TorchIn:
    """a torch [h, w, 3] tensor or view (element strides (row, 3, 1)) read in place; `check_untouched` compares every byte of the tensor
    the view belongs to"""

    def __init__(self, view, whole, dtype, order, csc, scale, bias):
        assert view.shape[2] == 3 and view.stride(2) == 1 and view.stride(1) == 3 and view.element_size() == ELEM[dtype]
        self.whole, self.was = whole, whole.clone()
        self.c = descriptor(view.data_ptr(), view.stride(0) * ELEM[dtype], dtype, order, csc, scale, bias)

    def check_untouched(self):
        import torch
        assert torch.equal(self.whole.view(torch.uint8), self.was.view(torch.uint8)), "the encoder wrote into a tensor"


def wide_pitch(w, dtype):
    """the pointer on a 16-byte boundary, the pitch a multiple of 16 above the row"""
    return dict(pitch=((3 * w * ELEM[dtype] + 15) & ~15) + 16)


def general_pitch(w, dtype, k=0):
    """the pitch the row's bytes plus one, two or three elements, the pointer 1, 2 or 3 elements behind a 16-byte boundary"""
    e = ELEM[dtype]
    return dict(pitch=3 * w * e + (1 + k % 3) * e, offset=1 + (k + 1) % 3)


def encode_hwc_steps(hip, encs, make, nfr, expect=0):
    """nfr lockstep steps over encs through dsv2hip_enc_batch_hwc, which returns `expect`; make(k, t) is stream k's source of step t
    (anything with .c and .check_untouched()).  Every source is compared with what was put there after every step.  Returns the
    packets per stream."""
    import torch
    from enc_in import take_packets
    n = len(encs)
    encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
    bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)()
    got = [[] for _ in range(n)]
    for t in range(nfr):
        made = [make(k, t) for k in range(n)]
        arr = (INHWC * n)(*[m.c for m in made])
        torch.cuda.synchronize()  # (the tensors are built on torch's stream, the encoder runs on its own)
        assert hip.dsv2hip_enc_batch_hwc(n, encp, arr, bufs, nbufs) == expect
        take_packets(hip, bufs, nbufs, got)
        for m in made:
            m.check_untouched()
    return got
