"""Planar RGB float tensors as encoder input (dsv2hip_in_tensor of include/dsv2_hip.h): the numpy oracle of the contract, a float
element generator, the ctypes descriptor with the three prototypes, a source class that holds one tensor in device memory with guard
bytes and padding around its rows, and the lockstep driver over dsv2hip_enc_batch_tensor.  Pinned to the kernel's text and to the C
restatement by tests/test_ingest_tensor_cpu.py; the GPU side is tests/test_gpu_enc_tensor.py.

    g = fl32(fl32(e * scale[c]) + bias[c])              e widened exactly to binary32; two operations, not fused
    v = 0 where g is a NaN, else rint(min(max(g, 0), 255)), ties to even

Elements travel as bit patterns: uint16 (F16, BF16) / uint32 (F32), as tests/tensor_out.py has them.
"""
import ctypes as C

import numpy as np

import dsvabi as A
from tensor_out import BF16, BITS, ELEM, F16, F32, IMAGENET, NAMES, U8, UNIT  # noqa: F401  (the decoder's constants; the element types are one enum)

FLOATS = (F16, BF16, F32)
GUARD, LEAD = 0xA5, 64  # (tests/hipabi.py's)


def inverse(constants):
    """the encoder-side constants that undo the decoder's (scale, bias): scale' = 1 / scale, bias' = -bias / scale, folded in double
    precision and handed over as binary32"""
    scale, bias = constants
    return (tuple(float(np.float32(1.0 / s)) for s in scale), tuple(float(np.float32(-b / s)) for s, b in zip(scale, bias)))


UNIT_INV = inverse(UNIT)  # 255, 0
IMAGENET_INV = ((255 * 0.229, 255 * 0.224, 255 * 0.225), (255 * 0.485, 255 * 0.456, 255 * 0.406))  # 255 * std, 255 * mean
IDENTITY = ((1.0,) * 3, (0.0,) * 3)


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def widen(bits, dtype):
    """the elements' bit patterns as the binary32 values they stand for, exactly"""
    bits = np.asarray(bits)
    assert bits.dtype == BITS[dtype] and dtype in FLOATS
    if dtype == F32:
        return bits.view(np.float32)
    if dtype == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def plane_bytes(bits, dtype, scale, bias):
    """the bytes the encoder makes of one plane's elements under that plane's constants"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = widen(bits, dtype) * np.float32(scale)
        g = p + np.float32(bias)
        assert p.dtype == np.float32 and g.dtype == np.float32
        g = np.where(np.isnan(g), np.float32(0), g)
        return np.rint(np.clip(g, 0, 255)).astype(np.uint8)


def picture(planes, dtype, scale, bias):
    """planes: [R, G, B] bit patterns, each h x w.  Returns the h x w x 4 uint8 picture (alpha 0) whose RGBA | csc surface gives the
    tensor's packets."""
    h, w = planes[0].shape
    px = np.zeros((h, w, 4), dtype=np.uint8)
    for c in range(3):
        px[..., c] = planes[c] if dtype == U8 else plane_bytes(planes[c], dtype, scale[c], bias[c])
    return px


# ---- elements -----------------------------------------------------------------------------------------------------------------------
def narrow(f, dtype):
    """binary32 values rounded to the element type, as bit patterns (bfloat16: the decoder oracle's rounding)"""
    f = np.asarray(f, dtype=np.float32)
    if dtype == F32:
        return f.view(np.uint32).copy()
    if dtype == F16:
        with np.errstate(over="ignore"):
            return f.astype(np.float16).view(np.uint16).copy()
    b = f.view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def elements_near(values, dtype, scale, bias, rng):
    """float elements of one plane that a producer under (scale, bias) might hold for a picture whose bytes are about `values` (h x w
    uint8): (values + a fraction in -0.45 .. 0.45 - bias) / scale, rounded to the element type.  What bytes they ARE is plane_bytes'
    business, not this function's: a bfloat16 element has 8 significant bits."""
    v = values.astype(np.float64) + rng.uniform(-0.45, 0.45, values.shape)
    return narrow(((v - bias) / scale).astype(np.float32), dtype)


def tensor_near(px4, dtype, scale, bias, seed):
    """[R, G, B] element planes near the colour bytes of an h x w x 4 picture (tests/enc_in.py's rgb_content)"""
    rng = np.random.default_rng(seed)
    return [px4[..., c].copy() if dtype == U8 else elements_near(px4[..., c], dtype, scale[c], bias[c], rng) for c in range(3)]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
class INTENSOR(C.Structure):  # dsv2hip_in_tensor
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("dtype", C.c_int), ("csc", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


def bind(hip):
    """argtypes and restype of the three tensor entry points; idempotent; returns hip"""
    P = C.POINTER
    hip.dsv2hip_enc_batch_tensor.argtypes = [C.c_int, P(P(A.ENCODER)), P(INTENSOR), P(A.BUF), P(C.c_int)]
    hip.dsv2hip_enc_batch_tensor.restype = C.c_int
    hip.dsv2hip_enc_tensor_frame.argtypes = [P(A.ENCODER), P(INTENSOR), P(A.BUF)]
    hip.dsv2hip_enc_tensor_frame.restype = C.c_int
    hip.dsv2hip_enc_tensor_stats.argtypes = [P(C.c_ulonglong), C.c_int]
    hip.dsv2hip_enc_tensor_stats.restype = None
    return hip


def tensor_forms(hip, reset=False):
    """dsv2hip_enc_tensor_stats as a tuple of 2: steps in the wide / in the general form"""
    out = (C.c_ulonglong * 2)()
    hip.dsv2hip_enc_tensor_stats(out, int(reset))
    return tuple(out)


def descriptor(ptrs, pitches, dtype, csc, scale, bias):
    c = INTENSOR()
    c.dtype, c.csc = dtype, csc
    for k in range(3):
        c.plane[k], c.pitch[k], c.scale[k], c.bias[k] = ptrs[k], pitches[k], scale[k], bias[k]
    return c


def copy_of(c):
    d = INTENSOR()
    C.memmove(C.byref(d), C.byref(c), C.sizeof(c))
    return d


# ---- sources in device memory (torch is imported where a GPU test asks for one) -------------------------------------------------------
class TensorIn:
    """[R, G, B] element planes (bit patterns, h x w) as three device allocations: LEAD guard bytes, `offsets[c]` ELEMENTS more, h rows
    `pitches[c]` bytes apart (the last one without padding), LEAD guard bytes; guard and padding hold `fill` (None: noise).
    `check_untouched` compares every byte with what was put there."""

    def __init__(self, planes, dtype, csc, scale, bias, pitches, offsets=(0, 0, 0), fill=GUARD):
        import torch
        elem = ELEM[dtype]
        self.t, self.was, ptrs = [], [], []
        for c, pl in enumerate(planes):
            h, w = pl.shape
            rb, pitch = w * elem, pitches[c]
            assert pitch >= rb and pl.dtype == BITS[dtype]
            start = LEAD + offsets[c] * elem
            size = start + (h - 1) * pitch + rb + LEAD
            if fill is None:
                t = torch.from_numpy(np.random.default_rng(size + c).integers(0, 256, size, dtype=np.uint8)).cuda()
            else:
                t = torch.full((size,), fill, dtype=torch.uint8, device="cuda")
            assert t.data_ptr() % 16 == 0
            rows = np.ascontiguousarray(pl).view(np.uint8).reshape(h, rb)
            torch.as_strided(t, (h, rb), (pitch, 1), start).copy_(torch.from_numpy(rows).cuda())
            self.t.append(t)
            self.was.append(t.clone())
            ptrs.append(t.data_ptr() + start)
        self.c = descriptor(ptrs, pitches, dtype, csc, scale, bias)

    def check_untouched(self):
        import torch
        for t, was in zip(self.t, self.was):
            assert torch.equal(t, was), "the encoder wrote into a tensor"


class TorchIn:
    """a torch [3, h, w] tensor (or view: any plane and row stride, element stride 1) read in place; order: which plane of the view is
    handed over as R, G, B; `check_untouched` compares every byte of the tensor the view belongs to"""

    def __init__(self, view, whole, dtype, csc, scale, bias, order=(0, 1, 2)):
        assert view.shape[0] == 3 and view.stride(2) == 1 and view.element_size() == ELEM[dtype]
        self.whole, self.was = whole, whole.clone()
        self.c = descriptor([view[k].data_ptr() for k in order], [view.stride(1) * ELEM[dtype]] * 3, dtype, csc, scale, bias)

    def check_untouched(self):
        import torch
        assert torch.equal(self.whole.view(torch.uint8), self.was.view(torch.uint8)), "the encoder wrote into a tensor"


def wide_pitches(w, dtype):
    """pointers on a 16-byte boundary, pitches multiples of 16 that differ per plane"""
    p = ((w * ELEM[dtype] + 15) & ~15) + 16
    return dict(pitches=(p, p + 16, p + 32))


def general_pitches(w, dtype, k=0):
    """pitches the row's bytes plus one, two, three elements, pointers 1, 2, 3 elements behind a 16-byte boundary (odd ones among them,
    another one per plane)"""
    e = ELEM[dtype]
    return dict(pitches=tuple(w * e + (1 + c) * e for c in range(3)), offsets=tuple(1 + (k + c) % 3 for c in range(3)))


def encode_tensor_steps(hip, encs, make, nfr, expect=0):
    """nfr lockstep steps over encs through dsv2hip_enc_batch_tensor, which returns `expect`; make(k, t) is stream k's source of step t
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
        arr = (INTENSOR * n)(*[m.c for m in made])
        torch.cuda.synchronize()  # (the tensors are built on torch's stream, the encoder runs on its own)
        assert hip.dsv2hip_enc_batch_tensor(n, encp, arr, bufs, nbufs) == expect
        take_packets(hip, bufs, nbufs, got)
        for m in made:
            m.check_untouched()
    return got
