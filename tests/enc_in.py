"""What the encoder reads in the GPU tests, and the one lockstep driver over every batch call that takes surfaces.

Sources (Surface, RgbSurface, Rgb3Surface, TensorSurface) hold one picture in device memory with guard bytes and padding around
the rows, and compare every byte with what was put there after the encoder has read them.  The pictures, and the reference
encoder's packets on the planes that the header's conversions define, are made once here, shared and never changed."""
import ctypes as C
import functools

import numpy as np
import torch

import dsvabi as A
import ingest_scale as S
import rgb3_csc as R3
import rgb_csc as R
from codec_run import FMT, configure_encoder, decode_stream, encode_stream, frames as plain_frames
from edge_cases import packet_bound_holds
from hipabi import GUARD, LEAD, PLANAR, SCALE, SEMI, SURFACE

CFG = dict(qp=60, gop=12)
LOSSLESS = dict(qp=100, gop=12)
CSC_IDS = ["bt601", "bt709", "bt601_full", "bt709_full"]
CIF_PLANAR = dict(layout=PLANAR, pitches=(512, 256, 256))  # 352x288 4:2:0, aligned pointers and pitches: the wide forms
CIF_NV12 = dict(layout=SEMI, pitches=(512, 512))


def is_rgb(layout):
    return (layout & 0xff) in (R.BGRA, R.RGBA)


def kind_of(layout):
    """which oracle a layout's pictures come from: the YUV content for both YUV layouts, the RGB content through the layout's conversion"""
    return layout if is_rgb(layout) else "yuv"


# ---- pictures and the reference's packets on them ------------------------------------------------------------------------------
def dims(w, h, name):
    """(format code, [(row bytes, rows)] of Y, U, V)"""
    code, hs, vs = FMT[name]
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    return code, [(w, h), (cw, ch), (cw, ch)]


@functools.lru_cache(maxsize=None)
def content(w, h, name, nfr, seed):
    _, hs, vs = FMT[name]
    return tuple(plain_frames(w, h, hs, vs, nfr, seed))


@functools.lru_cache(maxsize=None)
def reference(w, h, name, nfr, seed):
    return tuple(encode_stream(A.load_ref(), list(content(w, h, name, nfr, seed)), w, h, FMT[name][0], eos=False, **CFG)[0])


@functools.lru_cache(maxsize=None)
def rgb_content(w, h, nfr, seed):
    """nfr pictures, h x w x 4 uint8: smooth moving gradients in the three colour bytes plus noise, the alpha byte random"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for t in range(nfr):
        c = [(np.sin((xx + 3 * t) / 17.0) + np.cos((yy + 2 * t) / 11.0)) * 50 + 128,
             np.sin((xx - 2 * t + yy) / 23.0) * 90 + 128,
             np.cos((yy + 4 * t) / 19.0) * 70 + np.sin(xx / 31.0) * 40 + 120]
        px = np.stack(c + [np.zeros((h, w))], axis=-1) + rng.integers(-3, 4, (h, w, 4))
        px = px.clip(0, 255).astype(np.uint8)
        px[..., 3] = rng.integers(0, 256, (h, w))
        px.setflags(write=False)
        out.append(px)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def saturated_pictures():
    """64x48: the 8 corners of the colour cube in 8x8 tiles, 16 rows of noise, a sweep 0..255 of each primary (12 rows), 12 rows
    of noise; the second picture has other noise"""
    out = []
    for t in range(2):
        rng = np.random.default_rng(70 + t)
        px = rng.integers(0, 256, (48, 64, 4), dtype=np.uint8)
        for k in range(8):
            px[0:8, 8 * k:8 * k + 8, 0:3] = [255 * (k & 1), 255 * ((k >> 1) & 1), 255 * ((k >> 2) & 1)]
        sweep = np.zeros((768, 3), dtype=np.uint8)
        for c in range(3):
            sweep[256 * c:256 * c + 256, c] = np.arange(256)
        px[24:36, :, 0:3] = sweep.reshape(12, 64, 3)
        px.setflags(write=False)
        out.append(px)
    return tuple(out)


def oracle_frames(pictures, layout, name):
    _, hs, vs = FMT[name]
    return [R.planar_bytes(p, layout, hs, vs) for p in pictures]


def rgb_ref_packets(pictures, layout, name, cfg):
    """the real reference encoder on the planar pictures the conversion defines"""
    h, w = pictures[0].shape[:2]
    return encode_stream(A.load_ref(), oracle_frames(pictures, layout, name), w, h, FMT[name][0], eos=False, **cfg)[0]


@functools.lru_cache(maxsize=None)
def rgb_reference(w, h, name, nfr, seed, layout, lossless=False):
    return tuple(rgb_ref_packets(rgb_content(w, h, nfr, seed), layout, name, LOSSLESS if lossless else CFG))


def conditions(packets, w, h, name):
    """both conditions of a scaled or sized case: the packets stay inside the bound within which the reference is defined, and I and P
    pictures both occur.  (4:1:1 and "4:1:0": the reference gives their packets the buffer of 4:2:0, dsv_encoder.c:1062-1066.)"""
    packet_bound_holds(packets, w, h, FMT[name][0] if name in ("444", "422", "420") else A.SUBSAMP_420)
    kinds = {pk[5] & 1 for pk in packets if pk[5] & 0x04}  # (dsv.h: packet type at byte 5, picture = 0x04, bit 0 = predicted)
    assert kinds == {0, 1}, "broken test case: I and P pictures do not both occur"


def ref_packets(pictures, w, h, name, cfg):
    """the reference encoder's packets on packed planar pictures, checked for conditions()"""
    packets = tuple(encode_stream(A.load_ref(), list(pictures), w, h, FMT[name][0], eos=False, **cfg)[0])
    conditions(packets, w, h, name)
    return packets


# the scaled and sized ingests' cases: four pictures with seed 5 in GOPs of 4, so that I and P pictures occur in every stream
LADDER_CFG, LADDER_LOSSLESS, LADDER_NFR, LADDER_SEED = dict(qp=60, gop=4), dict(qp=100, gop=4), 4, 5


@functools.lru_cache(maxsize=None)
def scaled_pictures(sw, sh, name, s, kind):
    """the pictures (packed planar bytes) of an encoder that reads the content made at the SOURCE size at the scale of shift s (the
    oracle tests/ingest_scale.py)"""
    _, hs, vs = FMT[name]
    if kind == "yuv":
        return tuple(S.packed(S.reduce_yuv(S.split_planar(f, sw, sh, hs, vs), s)) for f in content(sw, sh, name, LADDER_NFR, LADDER_SEED))
    return tuple(S.packed(S.convert_scaled(px, kind, hs, vs, s)) for px in rgb_content(sw, sh, LADDER_NFR, LADDER_SEED))


@functools.lru_cache(maxsize=None)
def scaled_reference(sw, sh, name, s, kind):
    return ref_packets(scaled_pictures(sw, sh, name, s, kind), S.up(sw, s), S.up(sh, s), name, LADDER_CFG)


def planes_equal_oracle(packets, pictures, layout, name):
    """the product's packets through the REFERENCE decoder: with a lossless stream its pictures are the oracle's planes, sample for sample"""
    _, hs, vs = FMT[name]
    dec = decode_stream(A.load_ref(), packets)
    assert len(dec) == len(pictures)
    for t, (fn, *planes) in enumerate(dec):
        for c, (got, want) in enumerate(zip(planes, R.convert(pictures[t], layout, hs, vs))):
            assert got.shape == want.shape
            bad = np.argwhere(got != want)
            assert bad.size == 0, "frame %d plane %d: sample (x=%d, y=%d) is %d, the conversion gives %d" % (
                t, c, bad[0][1], bad[0][0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- sources ---------------------------------------------------------------------------------------------------------------------
def guarded(rows, rb, pitch, offset, fill, seed=0):
    """a device tensor of LEAD guard bytes, `offset` more, `rows` rows of rb bytes `pitch` apart (the last one without padding) and LEAD
    guard bytes, everything holding `fill` (None: noise seeded by the size + seed); returns (tensor, the index of the first row)"""
    assert pitch >= rb
    start = LEAD + offset
    size = start + (rows - 1) * pitch + rb + LEAD
    if fill is None:
        t = torch.from_numpy(np.random.default_rng(size + seed).integers(0, 256, size, dtype=np.uint8)).cuda()
    else:
        t = torch.full((size,), fill, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t, start


class Planes:
    """Source planes as device tensors, one per plane (guarded()); `check_untouched` compares every byte with what was put."""

    def __init__(self, planes, layout, pitches, offsets, fill):
        self.t, self.was = [], []
        self.c = SURFACE()
        self.c.layout = layout
        for i, pl in enumerate(planes):
            rows, rb = pl.shape
            t, start = guarded(rows, rb, pitches[i], offsets[i], fill, seed=i)
            torch.as_strided(t, (rows, rb), (pitches[i], 1), start).copy_(torch.from_numpy(pl.copy()).cuda())
            self.t.append(t)
            self.was.append(t.clone())
            self.c.plane[i] = t.data_ptr() + start
            self.c.pitch[i] = pitches[i]

    def check_untouched(self):
        for t, was in zip(self.t, self.was):
            assert torch.equal(t, was), "the encoder wrote into a surface"


class Surface(Planes):
    """One packed planar picture as a planar or semiplanar surface: a tensor per source plane, rows `pitches[i]` apart, `offsets[i]`
    bytes behind a 16-byte boundary; guard and padding hold `fill`."""

    def __init__(self, frame, w, h, name, layout, pitches, offsets=(0, 0, 0), fill=GUARD):
        _, d = dims(w, h, name)
        flat = np.frombuffer(frame, dtype=np.uint8)
        planes, at = [], 0
        for pw, ph in d:
            planes.append(flat[at:at + pw * ph].reshape(ph, pw))
            at += pw * ph
        assert at == flat.size
        if layout == SEMI:
            planes = [planes[0], np.stack([planes[1], planes[2]], axis=-1).reshape(d[1][1], 2 * d[1][0])]
        super().__init__(planes, layout, pitches, offsets, fill)


class RgbSurface(Planes):
    """One h x w x 4 picture as a four-byte RGB surface: rows of 4 * w bytes `pitch` apart.  Guard and padding hold `fill` (None:
    noise); `alpha` (not None) replaces the picture's alpha bytes.  plane[1..2] and pitch[1..2] stay NULL / 0: an RGB surface has none."""

    def __init__(self, pixels, layout, pitch, offset=0, fill=GUARD, alpha=None):
        h, w = pixels.shape[:2]
        if alpha is not None:
            pixels = pixels.copy()
            pixels[..., 3] = alpha
        super().__init__([pixels.reshape(h, 4 * w)], layout, (pitch,), (offset,), fill)


def pixels_of(px4, layout):
    """bytes 0..2 of an h x w x 4 picture as a three-byte surface of `layout` holds them: in memory order (BGR / RGB), or as three planes
    that are R, G, B (RGBP)"""
    if R3.order_of(layout) == R3.RGBP:
        return np.ascontiguousarray(px4[..., :3].transpose(2, 0, 1))
    return np.ascontiguousarray(px4[..., :3])


class Rgb3Surface(Planes):
    """Bytes 0..2 of an h x w x 4 picture as a three-byte or planar RGB surface: one tensor (BGR / RGB) or three (RGBP).  Guard and
    padding hold `fill` (None: noise).  pitch / offset: a value, or one per plane.  plane[1..2] and pitch[1..2] of a packed surface stay
    NULL / 0."""

    def __init__(self, px4, layout, pitch, offset=0, fill=GUARD):
        pixels = pixels_of(px4, layout)
        planes = list(pixels) if R3.order_of(layout) == R3.RGBP else [pixels.reshape(pixels.shape[0], -1)]
        pitches = pitch if isinstance(pitch, tuple) else (pitch,) * len(planes)
        offsets = offset if isinstance(offset, tuple) else (offset,) * len(planes)
        super().__init__(planes, layout, pitches, offsets, fill)


class TensorSurface:
    """a view of a torch uint8 tensor as a surface, read in place: h x w x 3 (element strides (pitch, 3, 1)) or 3 x h x w (strides
    (plane, pitch, 1)); `check_untouched` compares every byte of the tensor the view belongs to"""

    def __init__(self, view, whole, layout):
        self.whole, self.was = whole, whole.clone()
        self.c = SURFACE()
        self.c.layout = layout
        if R3.order_of(layout) == R3.RGBP:
            assert view.shape[0] == 3 and view.stride(2) == 1
            for c in range(3):
                self.c.plane[c] = view[c].data_ptr()
                self.c.pitch[c] = view.stride(1)
        else:
            assert view.shape[2] == 3 and view.stride(2) == 1 and view.stride(1) == 3
            self.c.plane[0] = view.data_ptr()
            self.c.pitch[0] = view.stride(0)

    def check_untouched(self):
        assert torch.equal(self.whole, self.was), "the encoder wrote into a tensor"


def pitch_of(rb, variant):
    return {"tight": rb, "plus1": rb + 1, "aligned": ((rb + 15) & ~15) + 16}[variant]


def offset_of(variant):
    return 1 if variant == "plus1" else 0


def yuv_source(frame, sw, sh, name, layout, s, variant, offset=None):
    """a packed planar picture of sw x sh as a planar / semiplanar device surface whose layout says the scale of shift s"""
    _, hs, vs = FMT[name]
    rbs = [rb for rb, _ in S.source_dims(sw, sh, hs, vs, layout)]
    off = offset_of(variant) if offset is None else offset
    sf = Surface(frame, sw, sh, name, layout, tuple(pitch_of(rb, variant) for rb in rbs), offsets=(off, off, off))
    sf.c.layout = layout | SCALE[s]
    return sf


def rgb_source(pixels, layout, s, variant, offset=None):
    sw = pixels.shape[1]
    return RgbSurface(pixels, layout | SCALE[s], pitch_of(4 * sw, variant), offset=offset_of(variant) if offset is None else offset)


# ---- encoders and the lockstep driver ----------------------------------------------------------------------------------------------
def encoders(hip, w, h, name, n, cfg=CFG):
    meta = A.mk_meta(w, h, FMT[name][0])
    encs = [A.ENCODER() for _ in range(n)]
    for e in encs:
        configure_encoder(hip, e, meta, **cfg)
    return encs


def take_packets(hip, bufs, nbufs, got):
    for s in range(len(got)):
        assert 0 <= nbufs[s] <= 4
        for i in range(nbufs[s]):
            b = bufs[4 * s + i]
            got[s].append(bytes(C.string_at(b.data, b.len)))
            hip.dsv_buf_free(C.byref(b))


def encode_steps(hip, encs, make, nfr, expect=0, call="dsv2hip_enc_batch_surface"):
    """nfr lockstep steps over encs through the batch call `call`, which returns `expect`; make(k, t) is stream k's source of step t --
    for the scaled and the sized call (source, src_w, src_h).  Every source, its guard and its padding bytes are compared with what
    was put there after every step.  Returns the packets per stream."""
    n = len(encs)
    encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
    bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)()
    got = [[] for _ in range(n)]
    for t in range(nfr):
        made = [make(k, t) for k in range(n)]
        made = [m if isinstance(m, tuple) else (m,) for m in made]
        arr = (SURFACE * n)(*[m[0].c for m in made])
        sizes = [(C.c_int * n)(*column) for column in zip(*[m[1:] for m in made])]
        torch.cuda.synchronize()  # (the tensors are built on torch's stream, the encoder runs on its own)
        assert getattr(hip, call)(n, encp, arr, *sizes, bufs, nbufs) == expect
        take_packets(hip, bufs, nbufs, got)
        for m in made:
            m[0].check_untouched()
    return got


def packed_batch(hip, w, h, name, frames):
    """dsv2hip_enc_batch on the packed picture, one stream"""
    enc = encoders(hip, w, h, name, 1)[0]
    encp = (C.POINTER(A.ENCODER) * 1)(C.pointer(enc))
    bufs, nbufs = (A.BUF * 4)(), (C.c_int * 1)()
    got = [[]]
    for fb in frames:
        dev = torch.from_numpy(np.frombuffer(fb, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        assert hip.dsv2hip_enc_batch(1, encp, (C.c_void_p * 1)(dev.data_ptr()), bufs, nbufs) == 0
        take_packets(hip, bufs, nbufs, got)
    hip.dsv_enc_free(C.byref(enc))
    return got[0]


def same_packets(want, got, what=""):
    assert len(want) == len(got), "%s: %d packets, the reference has %d" % (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(want, got)):
        assert a == b, "%s: packet %d differs" % (what, i)


def copy_of(c):
    d = SURFACE()
    C.memmove(C.byref(d), C.byref(c), C.sizeof(c))
    return d


def refused(hip, encs, cs, single=True):
    """the plain batch call on surfaces cs returns -1 and leaves nbufs alone; the one-frame call on each pair returns 0"""
    n = len(encs)
    encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
    bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)(*[77 + k for k in range(n)])
    state = [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs]
    assert hip.dsv2hip_enc_batch_surface(n, encp, (SURFACE * n)(*cs), bufs, nbufs) == -1
    assert list(nbufs) == [77 + k for k in range(n)]
    if single:
        assert sum(hip.dsv2hip_enc_surface_frame(C.byref(e), C.byref(c), bufs) for e, c in zip(encs, cs)) == 0
    assert [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs] == state
    return encp, bufs, nbufs
