"""Three-byte and planar RGB device surfaces (DSV2HIP_SURFACE_BGR / _RGB / _RGBP, or-ed with DSV2HIP_CSC_*) as encoder input: the
packets are the reference encoder's on the planar picture that the conversion of include/dsv2_hip.h defines (tests/rgb3_csc.py:
tests/rgb_csc.py on the picture widened to four bytes) -- both forms of both kinds of k_ingest_rgb3, both byte orders, the four
presets, the five chroma formats, the smallest pictures and footprints half outside them (lossless, so every LSB of the conversion
reaches the packets), saturated colours, rows of several passes, torch tensors read in place, every kind of surface mixed in one
step; padding is never a pixel, the surface is never written, a refused call touches nothing.  The shapes are those of
tests/test_gpu_enc_rgb.py; the pictures, encoders and references of both are tests/enc_in.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsvabi as A
import rgb3_csc as R3
import rgb_csc as R
from edge_cases import stream_inverse_is_undefined
from codec_run import FMT
from dec_out import OutSurf, aligned as aligned_out, format_stream, planar_oracle
from enc_in import (CFG, CIF_NV12, CSC_IDS, LOSSLESS, Rgb3Surface, RgbSurface, Surface, TensorSurface, content, copy_of, encode_steps, encoders, oracle_frames,
                    packed_batch, pixels_of, planes_equal_oracle, reference, refused, rgb_content, rgb_ref_packets as ref_packets, rgb_reference, same_packets,
                    saturated_pictures)
from hipabi import (OUTSURF, PLANAR, SURFACE, bind, enc_rgb3_forms as rgb3_forms, enc_rgb_forms as rgb_forms, enc_yuv_forms as yuv_forms, mk_buf,
                    reset_enc_forms as reset_all, surface_dims)

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

BGR, RGB, RGBP = R3.BGR, R3.RGB, R3.RGBP
ORDERS = ["bgr", "rgb", "rgbp"]


def counts(layout, wide, steps=3):
    """dsv2hip_enc_rgb3_stats after `steps` steps of surfaces of `layout` alone"""
    at = 2 * (R3.order_of(layout) == RGBP) + (0 if wide else 1)
    return tuple(steps if i == at else 0 for i in range(4))


def four(layout):
    """the four-byte layout that names the colours of rgb_content's bytes 0..2 read as a surface of `layout`"""
    return (R.BGRA if R3.order_of(layout) == BGR else R.RGBA) | (layout & 0x300)


def expected(pictures4, layout, name):
    """the real reference encoder on the planar pictures of the oracle (tests/rgb3_csc.py)"""
    _, hs, vs = FMT[name]
    h, w = pictures4[0].shape[:2]
    frames = [R3.planar_bytes(pixels_of(p, layout), layout, hs, vs) for p in pictures4]
    assert frames == oracle_frames(pictures4, four(layout), name)  # (so rgb_reference below is this very encode, made once for both files)
    return frames


def reference3(w, h, name, nfr, seed, layout, lossless=False):
    expected(rgb_content(w, h, nfr, seed), layout, name)
    return rgb_reference(w, h, name, nfr, seed, four(layout), lossless)


def row_bytes(w, layout):
    return w if R3.order_of(layout) == RGBP else 3 * w


def wide_spec(w, layout):
    """pointers on a 16-byte boundary, pitches multiples of 16 (the planes' differ)"""
    p = ((row_bytes(w, layout) + 15) & ~15) + 16
    return dict(pitch=(p, p + 16, p + 32)) if R3.order_of(layout) == RGBP else dict(pitch=p)


def general_spec(w, layout, k=0):
    """pitches the row's bytes + 3 made odd, pointers 1, 2, 3 bytes behind a 16-byte boundary (RGBP: another one per plane)"""
    p = (row_bytes(w, layout) + 3) | 1
    if R3.order_of(layout) == RGBP:
        return dict(pitch=(p, p + 2, p + 4), offset=tuple(1 + (k + c) % 3 for c in range(3)))
    return dict(pitch=p, offset=1 + k % 3)


def encode_rgb3(hip, pictures4, layout, name, cfg=CFG, **surface):
    """one encoder over `pictures4`, each in an Rgb3Surface(**surface); frees the encoder"""
    h, w = pictures4[0].shape[:2]
    encs = encoders(hip, w, h, name, 1, cfg)
    got = encode_steps(hip, encs, lambda s, t: Rgb3Surface(pictures4[t], layout, **surface), len(pictures4))
    hip.dsv_enc_free(C.byref(encs[0]))
    return got[0]


def lossless_planes_equal_oracle(packets, pictures4, layout, name):
    planes_equal_oracle(packets, pictures4, four(layout), name)
    _, hs, vs = FMT[name]
    for a, b in zip(R3.convert(pixels_of(pictures4[0], layout), layout, hs, vs), R.convert(pictures4[0], four(layout), hs, vs)):
        assert np.array_equal(a, b)


# ---- 1. wide forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_wide_form_equals_reference(order):
    """352x288 4:2:0, pitches multiples of 16, aligned: one 12-byte load a row (BGR, RGB), a dword a plane a row (RGBP); the counters
    of the four-byte and the YUV surfaces do not move."""
    hip = bind(A.load_hip())
    reset_all(hip)
    layout = R3.ORDER[order]
    got = encode_rgb3(hip, rgb_content(352, 288, 3, 5), layout, "420", **wide_spec(352, layout))
    same_packets(reference3(352, 288, "420", 3, 5, layout), got)
    assert rgb3_forms(hip) == counts(layout, wide=True) == ((0, 0, 3, 0) if order == "rgbp" else (3, 0, 0, 0))
    assert rgb_forms(hip) == (0, 0) and yuv_forms(hip) == (0, 0)


# ---- 2. general forms, every format ------------------------------------------------------------------------------------------------
GENERAL = [(354, 290, "420")] + [(176, 144, name) for name in sorted(FMT)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k,w,h,name", [(k,) + g for k, g in enumerate(GENERAL)], ids=["%dx%d-%s" % g for g in GENERAL])
def test_general_form_equals_reference(k, w, h, name, order):
    """Odd pitches and pointers 1, 2 and 3 bytes behind a 16-byte boundary (RGBP: another offset and pitch per plane); a 354-pixel row is
    more than one pass of the workgroup (256 pixels), its last pass partial, and its last thread holds two pixels of four."""
    hip = bind(A.load_hip())
    reset_all(hip)
    turn = k + ORDERS.index(order)
    layout = R3.ORDER[order] | R.CSC[turn % 4]
    got = encode_rgb3(hip, rgb_content(w, h, 3, 5), layout, name, **general_spec(w, layout, turn))
    same_packets(reference3(w, h, name, 3, 5, layout), got)
    assert rgb3_forms(hip) == counts(layout, wide=False)
    assert rgb_forms(hip) == (0, 0) and yuv_forms(hip) == (0, 0)


# ---- 3. smallest pictures, clamped footprints: lossless -------------------------------------------------------------------------------
SMALL = ([(16, 16, name, form) for name in sorted(FMT) for form in ("wide", "general")] +
         [(22, 22, "411", "general"), (22, 22, "410", "general"), (22, 18, "420", "general")])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("w,h,name,form", SMALL, ids=["%dx%d-%s-%s" % s for s in SMALL])
def test_smallest_pictures_lossless(w, h, name, form, order):
    """16x16 in both forms; 22x22 in 4:1:1 and "4:1:0" and 22x18 in 4:2:0 (footprints half outside the picture), which only the general
    forms take -- the sizes of tests/test_gpu_enc_rgb.py, which says why 18x18 is left to the CPU side.  qp 100: the packets carry every
    bit of the planes, and the reference decoder gives them back to be compared with the conversion directly."""
    assert not stream_inverse_is_undefined(w, h, FMT[name][0], LOSSLESS)
    hip = bind(A.load_hip())
    reset_all(hip)
    k = SMALL.index((w, h, name, form))
    layout = R3.ORDER[order] | R.CSC[(k >> 1) % 4]  # (that file's preset of the case; the REFERENCE decoder refuses the reference encoder's own
    #                                                  lossless 16x16 "4:1:0" packets of these pictures under BT709 | FULL: "plane length was strange")
    pictures = rgb_content(w, h, 3, 9)
    surface = wide_spec(w, layout) if form == "wide" else general_spec(w, layout, k + ORDERS.index(order))
    got = encode_rgb3(hip, pictures, layout, name, cfg=LOSSLESS, **surface)
    assert rgb3_forms(hip) == counts(layout, wide=form == "wide")
    lossless_planes_equal_oracle(got, pictures, layout, name)
    same_packets(reference3(w, h, name, 3, 9, layout, lossless=True), got)


# ---- 4. presets and saturation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["444", "420"])
@pytest.mark.parametrize("csc", R.CSC, ids=CSC_IDS)
def test_presets_and_saturation_lossless(csc, name):
    """the cube-corner / sweep pictures of tests/test_gpu_enc_rgb.py in every layout: Y, U and V reach the ends of their ranges"""
    hip = bind(A.load_hip())
    pictures = saturated_pictures()
    want = {}
    for order in ORDERS:
        layout = R3.ORDER[order] | csc
        y, u, v = R3.convert(pixels_of(pictures[0], layout), layout, 0, 0)
        if csc & R.FULL:  # (U, V = 255 is the clamped 256)
            assert (y.min(), y.max()) == (0, 255) and (u.min(), u.max()) == (1, 255) and (v.min(), v.max()) == (1, 255)
        else:
            assert (y.min(), y.max()) == (16, 235) and (u.min(), u.max()) == (16, 240) and (v.min(), v.max()) == (16, 240)
        got = encode_rgb3(hip, pictures, layout, name, cfg=LOSSLESS, **wide_spec(64, layout))
        lossless_planes_equal_oracle(got, pictures, layout, name)
        if four(layout) not in want:
            want[four(layout)] = ref_packets(pictures, four(layout), name, LOSSLESS)
        same_packets(want[four(layout)], got, order)


# ---- 5. padding is never a pixel; the surface is never written -------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["rgb", "rgbp"])
@pytest.mark.parametrize("w,h,form", [(352, 288, "wide"), (354, 290, "general")], ids=["wide", "general"])
def test_padding_is_never_a_pixel_and_nothing_is_written(w, h, form, order):
    """The same colours with the pitch padding and the bytes around the planes holding 0x00, then 0xFF, then noise: identical packets,
    the reference's; every byte of the tensors is afterwards what the test put there (encode_steps)."""
    hip = bind(A.load_hip())
    layout = R3.ORDER[order]
    pictures = rgb_content(w, h, 3, 5)
    surface = wide_spec(w, layout) if form == "wide" else general_spec(w, layout, 2)
    runs = [encode_rgb3(hip, pictures, layout, "420", fill=fill, **surface) for fill in (0x00, 0xFF, None)]
    assert runs[0] == runs[1] == runs[2]
    same_packets(reference3(w, h, "420", 3, 5, layout), runs[0])


# ---- 6. straight from torch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [False, True], ids=["contiguous", "crop"])
@pytest.mark.parametrize("order", ["bgr", "rgbp"], ids=["hwc", "chw"])
def test_straight_from_torch(order, crop):
    """A contiguous uint8[h, w, 3] / uint8[3, h, w] tensor (pitch 3 * w / w, nothing around it) and a 354x290 crop at (7, 5) of a
    370x300 tensor of each kind (the parent's pitch, an offset pointer, w no multiple of 4): read in place, the reference's packets on the
    cropped pixels."""
    hip = bind(A.load_hip())
    reset_all(hip)
    layout = R3.ORDER[order] | R.BT709
    w, h = (354, 290) if crop else (352, 288)
    pictures = rgb_content(w, h, 3, 5)

    def make(s, t):
        pixels = torch.from_numpy(pixels_of(pictures[t], layout))
        if not crop:
            whole = pixels.cuda().contiguous()
            return TensorSurface(whole, whole, layout)
        if order == "rgbp":
            whole = torch.randint(0, 256, (3, 300, 370), dtype=torch.uint8, device="cuda")
            view = whole[:, 5:5 + h, 7:7 + w]
        else:
            whole = torch.randint(0, 256, (300, 370, 3), dtype=torch.uint8, device="cuda")
            view = whole[5:5 + h, 7:7 + w, :]
        view.copy_(pixels.cuda())
        assert not view.is_contiguous()
        return TensorSurface(view, whole, layout)

    encs = encoders(hip, w, h, "420", 1, CFG)
    got = encode_steps(hip, encs, make, 3)
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(reference3(w, h, "420", 3, 5, layout), got[0])
    assert rgb3_forms(hip) == counts(layout, wide=not crop)


# ---- 7. rows of several passes in the wide form -------------------------------------------------------------------------------------
def test_1920_wide_rows_take_several_passes():
    """1920x32 4:2:0 RGB with a 6144-byte pitch: 7.5 passes of the workgroup per row, two steps in the 12-byte form.  As
    tests/test_gpu_enc_rgb.py has it: of the reference's packets only those up to the first P picture are comparable where its inverse
    is undefined at this size; both pictures' ingest is checked against the library's own packed path on the conversion's planes."""
    hip = bind(A.load_hip())
    reset_all(hip)
    w, h, layout = 1920, 32, RGB | R.BT709
    pictures = rgb_content(w, h, 2, 5)
    got = encode_rgb3(hip, pictures, layout, "420", pitch=6144)
    assert rgb3_forms(hip) == (2, 0, 0, 0)
    want = reference3(w, h, "420", 2, 5, layout)
    if stream_inverse_is_undefined(w, h, FMT["420"][0], CFG):
        assert len(got) == len(want)
        same_packets(want[:2], got[:2])
    else:
        same_packets(want, got)
    assert got == packed_batch(hip, w, h, "420", expected(pictures, layout, "420"))


# ---- 8. one step: every kind of surface ------------------------------------------------------------------------------------------------
def test_mixed_step():
    """Six encoders at 352x288 4:2:0 in one call per frame: packed as a surface, NV12, BGRA, BGR-709 (aligned), RGB-601-full one byte
    off alignment and RGBP (aligned).  Each stream's packets are its own reference's, and every counter moves by its own kind: the
    three-byte launch is general because ONE of its two surfaces is, the planar launch and the others stay wide."""
    hip = bind(A.load_hip())
    w, h, name, nfr = 352, 288, "420", 3
    yuv = [dict(layout=PLANAR, pitches=(352, 176, 176)), CIF_NV12]
    rgb3 = [(BGR | R.BT709, wide_spec(w, BGR)), (RGB | R.FULL, dict(pitch=1072, offset=1)), (RGBP, wide_spec(w, RGBP))]

    def make(s, t):
        if s < 2:
            return Surface(content(w, h, name, nfr, 40 + s)[t], w, h, name, **yuv[s])
        if s == 2:
            return RgbSurface(rgb_content(w, h, nfr, 42)[t], R.BGRA, pitch=1536)
        return Rgb3Surface(rgb_content(w, h, nfr, 40 + s)[t], rgb3[s - 3][0], **rgb3[s - 3][1])

    encs = encoders(hip, w, h, name, 6, CFG)
    reset_all(hip)
    got = encode_steps(hip, encs, make, nfr)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    assert rgb3_forms(hip) == (0, 3, 3, 0)
    assert rgb_forms(hip) == (3, 0) and yuv_forms(hip) == (3, 0)
    for s in range(2):
        same_packets(reference(w, h, name, nfr, 40 + s), got[s], "stream %d" % s)
    same_packets(rgb_reference(w, h, name, nfr, 42, R.BGRA), got[2], "stream 2")
    for s in range(3, 6):
        same_packets(reference3(w, h, name, nfr, 40 + s, rgb3[s - 3][0]), got[s], "stream %d" % s)


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
def short_pitch(plane):
    def f(c, w):
        c.pitch[plane] = row_bytes(w, c.layout) - 1
    return f


def null_plane(plane):
    def f(c, w):
        c.plane[plane] = None
    return f


def layout_value(value):
    def f(c, w):
        c.layout = value
    return f


def scale_bit(c, w):
    c.layout |= 0x1000


REFUSALS = ([("rgb", "pitch_short", short_pitch(0)), ("bgr", "null_plane", null_plane(0)), ("rgb", "scale_half", scale_bit), ("bgr", "layout_0x4000", layout_value(0x4000)),
             ("rgb", "layout_0x4021", layout_value(0x4021)), ("bgr", "layout_0x23", layout_value(0x23)), ("rgbp", "scale_half", scale_bit),
             ("rgbp", "layout_0x422", layout_value(0x422))] +
            [("rgbp", "pitch_short_%d" % p, short_pitch(p)) for p in range(3)] + [("rgbp", "null_plane_%d" % p, null_plane(p)) for p in range(3)])


def steps_equal_reference(hip, encs, w, h, name, layouts, seeds):
    got = encode_steps(hip, encs, lambda s, t: Rgb3Surface(rgb_content(w, h, 3, seeds[s])[t], layouts[s], **wide_spec(w, layouts[s])), 3)
    for s in range(len(encs)):
        same_packets(reference3(w, h, name, 3, seeds[s], layouts[s]), got[s], "stream %d" % s)


@pytest.mark.parametrize("order,what,spoil", REFUSALS, ids=["%s-%s" % r[:2] for r in REFUSALS])
def test_refused_surface_touches_nothing(order, what, spoil):
    """Two encoders, the second one's surface spoiled: -1 (0 from the one-frame call), nbufs as the test set it, the encoders' bytes
    -- frame counters included -- unchanged; the same encoders then give the reference's packets from frame 0 on."""
    hip = bind(A.load_hip())
    w, h, name = 352, 288, "420"
    layouts = [BGR | R.FULL, R3.ORDER[order] | R.BT709]
    encs = encoders(hip, w, h, name, 2, CFG)
    good = [Rgb3Surface(rgb_content(w, h, 3, 5 + s)[0], layouts[s], **wide_spec(w, layouts[s])) for s in range(2)]
    bad = copy_of(good[1].c)
    spoil(bad, w)
    torch.cuda.synchronize()
    refused(hip, encs, [good[0].c, bad], single=False)
    state = bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1])))
    assert hip.dsv2hip_enc_surface_frame(C.byref(encs[1]), C.byref(bad), (A.BUF * 4)()) == 0
    assert bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1]))) == state
    steps_equal_reference(hip, encs, w, h, name, layouts, [5, 6])
    for e in encs:
        hip.dsv_enc_free(C.byref(e))


@pytest.mark.parametrize("order", ["rgb", "rgbp"])
def test_refused_on_a_uyvy_encoder(order):
    """An encoder whose packed input is interleaved UYVY takes none of the layouts; with the switch off again it encodes from frame 0."""
    hip = bind(A.load_hip())
    w, h, name = 176, 144, "422"
    layout = R3.ORDER[order]
    encs = encoders(hip, w, h, name, 1, CFG)
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 1) == 0
    sf = Rgb3Surface(rgb_content(w, h, 3, 5)[0], layout, **wide_spec(w, layout))
    torch.cuda.synchronize()
    refused(hip, encs, [sf.c])
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 0) == 0
    steps_equal_reference(hip, encs, w, h, name, [layout], [5])
    hip.dsv_enc_free(C.byref(encs[0]))


@pytest.mark.parametrize("order", ORDERS)
def test_refused_by_the_scaled_and_sized_calls_at_the_encoders_own_size(order):
    """dsv2hip_enc_batch_surface_scaled / _sized and their one-frame calls know nothing of the layouts, also where the surface holds
    exactly the encoder's picture (where a BGRA surface is the plain call's job): -1 / 0, nothing touched; the plain call then encodes
    the same surface from frame 0."""
    hip = bind(A.load_hip())
    w, h, name = 352, 288, "420"
    layout = R3.ORDER[order] | R.BT709
    encs = encoders(hip, w, h, name, 1, CFG)
    sf = Rgb3Surface(rgb_content(w, h, 3, 5)[0], layout, **wide_spec(w, layout))
    torch.cuda.synchronize()
    encp, arr = (C.POINTER(A.ENCODER) * 1)(C.pointer(encs[0])), (SURFACE * 1)(sf.c)
    bufs, nbufs, sws, shs = (A.BUF * 4)(), (C.c_int * 1)(77), (C.c_int * 1)(w), (C.c_int * 1)(h)
    state = bytes(C.string_at(C.byref(encs[0]), C.sizeof(encs[0])))
    assert hip.dsv2hip_enc_batch_surface_scaled(1, encp, arr, sws, shs, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_surface_sized(1, encp, arr, sws, shs, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_surface_frame_scaled(C.byref(encs[0]), C.byref(sf.c), w, h, bufs) == 0
    assert hip.dsv2hip_enc_surface_frame_sized(C.byref(encs[0]), C.byref(sf.c), w, h, bufs) == 0
    assert nbufs[0] == 77 and bytes(C.string_at(C.byref(encs[0]), C.sizeof(encs[0]))) == state
    sf.check_untouched()
    steps_equal_reference(hip, encs, w, h, name, [layout], [5])
    hip.dsv_enc_free(C.byref(encs[0]))


def test_refused_by_the_decoder():
    """Delivery into the three layouts is not done: dsv2hip_dec_surface_dims / _sized_dims know none of them, and dsv2hip_dec_batch_surface
    / dsv2hip_dec_surface_frame refuse a surface that names one -- here a 4:4:4 stream's PLANAR surface, three planes of w x h bytes,
    which has room for each of them -- with the packet, the decoder, fn / ret and the surface as they were; the same packets then
    decode into that surface as PLANAR."""
    hip = bind(A.load_hip())
    packets = format_stream("444", 34, 18, 3)
    want = planar_oracle(packets)
    dec = A.DECODER()
    decp = (C.POINTER(A.DECODER) * 1)(C.pointer(dec))
    bufs, arr, fns, rets = (A.BUF * 1)(), (OUTSURF * 1)(), (C.c_uint32 * 1)(), (C.c_int * 1)()
    mk_buf(hip, bufs[0], packets[0])
    assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, arr, fns, rets) == 1 and rets[0] == A.DEC_GOT_META
    dims = surface_dims(hip, dec, PLANAR)
    assert dims == [(34, 18)] * 3
    sf = OutSurf(dims, PLANAR, aligned_out)
    sf.arm()
    torch.cuda.synchronize()
    mk_buf(hip, bufs[0], packets[1])
    data, length = C.cast(bufs[0].data, C.c_void_p).value, bufs[0].len
    state = bytes(C.string_at(C.byref(dec), C.sizeof(dec)))
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    for order in (BGR, RGB, RGBP):
        for csc in R.CSC:
            layout = order | csc
            assert hip.dsv2hip_dec_surface_dims(C.byref(dec), layout, rb, rows) == -1, hex(layout)
            assert hip.dsv2hip_dec_sized_dims(C.byref(dec), layout, 34, 18, rb, rows) == -1, hex(layout)
            assert hip.dsv2hip_dec_sized_dims(C.byref(dec), layout, 17, 9, rb, rows) == -1, hex(layout)
            C.memmove(C.byref(arr[0]), C.byref(sf.c), C.sizeof(OUTSURF))
            arr[0].layout = layout
            fns[0], rets[0] = 77, -5
            assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, arr, fns, rets) == -1, hex(layout)
            one_fn = C.c_uint32(77)
            assert hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(bufs[0]), C.byref(arr[0]), C.byref(one_fn)) == -1, hex(layout)
            assert one_fn.value == 77 and fns[0] == 77 and rets[0] == -5
            assert C.cast(bufs[0].data, C.c_void_p).value == data and bufs[0].len == length
            assert bytes(C.string_at(bufs[0].data, len(packets[1]))) == packets[1]
            assert bytes(C.string_at(C.byref(dec), C.sizeof(dec))) == state
            assert sf.untouched()
    arr[0] = sf.c
    for t in range(1, len(packets)):
        if t > 1:
            mk_buf(hip, bufs[0], packets[t])
            sf.arm()
            torch.cuda.synchronize()
        assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, arr, fns, rets) == 1
        assert rets[0] == want[t][0]
        if want[t][2] is not None:
            assert fns[0] == want[t][1]
            for got, exp in zip(sf.planes(), want[t][2]):
                assert np.array_equal(got, exp)
    hip.dsv_dec_free(C.byref(dec))
