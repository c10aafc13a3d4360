"""Decoded pictures delivered at half, quarter and eighth size (DSV2HIP_SCALE_* or-ed into the layout of an out surface, through
dsv2hip_dec_batch_surface / dsv2hip_dec_surface_frame / dsv2hip_dec_surface_dims): the surface holds exactly the box reduction of
include/dsv2_hip.h (tests/box_reduce.py, numpy) -- then the chroma interleave, or the header's RGB conversion (tests/yuv_rgb.py) -- of
the planar picture that a second decoder of the library delivers from the same packets, under the same switches, into a full-size
PLANAR surface: a delivery the existing tests pin to the reference decoder.  Every shift into every kind of layout at the smallest
pictures, partial footprints, rows of more than one pass and planes of more than one workgroup, both forms of k_egress_scale, the
five chroma formats, saturated content, draw_info and postsharp in front of the reduction, layouts, scales and geometries mixed in
one step with either parser; no byte outside the reduced rows is written, a refused call consumes nothing, and a half-size NV12
surface feeds an encoder of the reduced geometry without the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import box_reduce as B
import dsvabi as A
import yuv_rgb as Q
from codec_run import configure_encoder, encode_stream
from edge_cases import packet_bound_holds
from codec_run import FMT
from dec_out import (OutSurf, Surfaces, aligned, base_of, content_stream, decode_steps, expected_dims, format_stream, in_layout, is_rgb, npics, planar_oracle, plus1,
                     same_results, shift_of, stream, tight)
from hipabi import (EIGHTH, HALF, OUTSURF, PLANAR, QUARTER, SCALE, SEMI, SURFACE, bind, dec_rgb_forms as rgb_forms, dec_scale_forms as scale_forms,
                    dec_uv_forms as uv_forms, mk_buf, reset_dec_forms as reset_all, surface_dims)

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

BGRA709, RGBAFULL = Q.BGRA | Q.BT709, Q.RGBA | Q.FULL
LAYOUTS = [PLANAR, SEMI, BGRA709, RGBAFULL]
LAYOUT_IDS = ["planar", "semiplanar", "bgra709", "rgba601full"]


def documented_wide(dims, layout, pitch, offset):
    """include/dsv2_hip.h at dsv2hip_dec_scale_stats: every reduced plane that goes straight into the caller's surface (PLANAR: all
    three, SEMIPLANAR: luma, RGB: none) has pointer and pitch multiples of 8 and a width that is a multiple of 16 >> s"""
    s, base = shift_of(layout), base_of(layout)
    straight = [] if is_rgb(base) else dims[:1] if base == SEMI else dims
    return all(offset % 8 == 0 and pitch(rb) % 8 == 0 and rb % (16 >> s) == 0 for rb, _ in straight)


def equals_oracle(hip, packets, fmt, layout, pitch, offset=0, mode=0, sharp=False):
    got = decode_steps(hip, [packets], Surfaces([dict(layout=layout, pitch=pitch, offset=offset)]), modes=[mode], sharp=[sharp])[0]
    want = planar_oracle(packets, mode, sharp)
    same_results(in_layout(want, layout, fmt), got)
    return want, got


def first_dims(got):
    return next([(pl_c.shape[1], pl_c.shape[0]) for pl_c in pl] for _, _, pl in got if pl is not None)


# ---- 1. every shift into every kind of layout, at the smallest pictures ----------------------------------------------------------------
# 16x16: luma 2x2 and chroma 1x1 at an eighth; 18x16: a partial footprint at a quarter and an eighth; 130x16: a second pass of the
# row loop (128 source bytes a pass) at the smallest height; GOPs of 2: I and P pictures in every stream
SIZES = [(16, 16), (18, 16), (34, 18), (66, 34), (130, 16)]
VARIANTS = [(tight, 0), (plus1, 1), (aligned, 0)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % g for g in SIZES])
def test_equals_the_reduction_of_the_planar_delivery(w, h, s, layout):
    hip = bind(A.load_hip())
    # (34x18: the synthetic video's pictures are all coded as intra pictures at this size; the plain frames give I P P P)
    packets = format_stream("420", w, h, 4) if (w, h) == (34, 18) else stream(w, h, "420", 4, 2)
    packet_bound_holds(packets, w, h, A.SUBSAMP_420)  # (the condition under which the reference encoder is defined at this size)
    kinds = {pk[5] & 1 for pk in packets if pk[5] & 0x04}  # (dsv.h: packet type at byte 5, picture = 0x04, bit 0 = predicted)
    assert kinds == {0, 1}  # I and P pictures both occur
    for pitch, offset in VARIANTS:
        reset_all(hip)
        want, got = equals_oracle(hip, packets, "420", layout | SCALE[s], pitch, offset)
        assert npics(want) == npics(got) == 4
        dims = first_dims(got)
        assert dims[0] == ((4 if is_rgb(layout) else 1) * B.reduced_size(w, s), B.reduced_size(h, s))
        wide = documented_wide(dims, layout | SCALE[s], pitch, offset)
        assert scale_forms(hip) == ((4, 0) if wide else (0, 4))
        assert sum(rgb_forms(hip)) == (4 if is_rgb(layout) else 0) and sum(uv_forms(hip)) == (4 if layout == SEMI else 0)


def test_both_forms_are_reached_by_the_cases_above():
    """the documented rule, applied to the cases of test 1 -- and to the planar surfaces of test 2 --, picks either form somewhere"""
    seen = set()
    for w, h in SIZES + [(64, 48)]:
        for s in (1, 2, 3):
            for layout in LAYOUTS:
                md = A.mk_meta(w, h, A.SUBSAMP_420)
                dims = [d for d in expected_dims(md, layout | SCALE[s]) if d[1]]
                for pitch, offset in VARIANTS:
                    seen.add((layout, documented_wide(dims, layout | SCALE[s], pitch, offset)))
    assert seen == {(layout, wide) for layout in LAYOUTS for wide in (True, False)} - {(BGRA709, False), (RGBAFULL, False)}


# ---- 2. the wide form into planar surfaces; planes of more than one workgroup ------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3])
def test_wide_form_into_planar_surfaces(s):
    """64x48: reduced widths 32 / 16 / 8 (luma) and 16 / 8 / 4 (chroma), multiples of 8 / 4 / 2 at their shift"""
    hip = bind(A.load_hip())
    packets = stream(64, 48, "420", 4, 2)
    reset_all(hip)
    equals_oracle(hip, packets, "420", PLANAR | SCALE[s], aligned)
    assert scale_forms(hip) == (4, 0)
    equals_oracle(hip, packets, "420", PLANAR | SCALE[s], aligned, offset=4)  # (a pointer that is a multiple of 4 only)
    assert scale_forms(hip) == (4, 4)


@pytest.mark.parametrize("layout", [PLANAR, BGRA709], ids=["planar", "bgra709"])
def test_tall_picture_takes_more_than_one_workgroup(layout):
    """130x258: 129 / 65 / 33 reduced rows against the 32 of a workgroup, two passes of the row loop, partial footprints both ways"""
    hip = bind(A.load_hip())
    packets = stream(130, 258, "420", 2, 2)
    for s in (1, 2, 3):
        equals_oracle(hip, packets, "420", layout | SCALE[s], plus1, offset=1)


# ---- 3. the five chroma formats -----------------------------------------------------------------------------------------------------
# 34x18; 4:1:1 and "4:1:0" at 38x22: the reference encoder, which makes the streams, divides by zero at 34x18 and at 34x22 there
FORMAT_SIZE = {"444": (34, 18), "422": (34, 18), "420": (34, 18), "411": (38, 22), "410": (38, 22)}


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("fmt", sorted(FMT))
def test_every_chroma_format(fmt, s):
    hip = bind(A.load_hip())
    w, h = FORMAT_SIZE[fmt]
    packets = format_stream(fmt, w, h, 3)
    for k, layout in enumerate(LAYOUTS):
        pitch, offset = VARIANTS[(k + s) % 3]
        want, _ = equals_oracle(hip, packets, fmt, layout | SCALE[s], pitch, offset)
        assert npics(want) == 3


# ---- 4. saturated content -------------------------------------------------------------------------------------------------------------
# white and black lossless; the checkerboard at 66x34 and quantiser 30: finer, or smaller, the reference encoder's packets of this
# content leave the bound inside which it is defined (tests/edge_cases.py)
CONTENT = [("white", 16, 16, 100), ("white", 34, 18, 100), ("black", 16, 16, 100), ("black", 34, 18, 100), ("checker", 66, 34, 30)]


@pytest.mark.parametrize("kind,w,h,qp", CONTENT, ids=["%s-%dx%d" % c[:3] for c in CONTENT])
def test_saturated_content(kind, w, h, qp):
    """255 stays 255 and 0 stays 0 through every shift: the rounding never carries a constant plane out of its value"""
    hip = bind(A.load_hip())
    packets = content_stream(kind, w, h, qp)
    full = planar_oracle(packets)
    assert npics(full) == 3
    if kind != "checker":
        value = 255 if kind == "white" else 0
        assert all(np.all(p == value) for _, _, pl in full if pl is not None for p in pl)  # (lossless: the decoded picture is the constant)
    for s in (1, 2, 3):
        _, got = equals_oracle(hip, packets, "420", PLANAR | SCALE[s], plus1, offset=1)
        if kind != "checker":
            assert all(np.all(p == value) for _, _, pl in got if pl is not None for p in pl)
        equals_oracle(hip, packets, "420", RGBAFULL | SCALE[s], tight)
        equals_oracle(hip, packets, "420", SEMI | SCALE[s], aligned)


# ---- 5. draw_info and postsharp act in front of the reduction --------------------------------------------------------------------------
@pytest.mark.parametrize("mode,sharp", [(7, False), (0, True), (7, True)], ids=["draw_info", "postsharp", "both"])
@pytest.mark.parametrize("layout", [SEMI, BGRA709], ids=["nv12", "bgra709"])
def test_draw_info_and_postsharp(layout, mode, sharp):
    """The reduced picture is the reduction of the drawn-on / sharpened full-size picture; that picture differs from the plain one in
    every picture, in luma only, and so does its reduction.  With the switches on for the first picture alone, every later picture
    -- the P picture that predicts from it first of all -- is the plain one: the picture predicted from is never touched."""
    hip = bind(A.load_hip())
    packets = stream(66, 34, "420", 4, 4)
    lay = layout | HALF
    want, got = equals_oracle(hip, packets, "420", lay, plus1, offset=1, mode=mode, sharp=sharp)
    plain = planar_oracle(packets)
    same_results(plain, want, planes=(1, 2))
    red_plain, red_want = in_layout(plain, PLANAR | HALF, "420"), in_layout(want, PLANAR | HALF, "420")
    assert all(not np.array_equal(a[2][0], b[2][0]) for a, b in zip(red_plain, red_want) if a[2] is not None)  # visible at half size
    assert npics(got) == 4
    first = next(i for i, r in enumerate(plain) if r[2] is not None)
    once = decode_steps(hip, [packets], Surfaces([dict(layout=lay, pitch=aligned, offset=0)]), modes=[lambda t: mode if t <= first else 0],
                        sharp=[lambda t: sharp and t <= first])[0]
    mixed = [w_ if i <= first else p for i, (w_, p) in enumerate(zip(want, plain))]
    same_results(in_layout(mixed, lay, "420"), once)


# ---- 6. one mixed step ---------------------------------------------------------------------------------------------------------------
def mixed_step(hip):
    a, b = stream(66, 34, "420", 4, 2), format_stream("444", 34, 18, 3)
    streams = [a, a, a, b, a]
    fmts = ["420", "420", "420", "444", "420"]
    specs = [dict(layout=SEMI, pitch=aligned, offset=0),                 # full-size NV12
             dict(layout=PLANAR | HALF, pitch=plus1, offset=1),
             dict(layout=BGRA709 | QUARTER, pitch=aligned, offset=0),
             dict(layout=PLANAR | EIGHTH, pitch=tight, offset=0),          # the second geometry, packed: a round of its own
             dict(layout=SEMI | QUARTER, pitch=tight, offset=0)]           # joins two steps late: no metadata beside decoders with pictures
    delay = [0, 0, 0, 0, 2]
    reset_all(hip)
    got = decode_steps(hip, streams, Surfaces(specs), delay=delay)
    assert scale_forms(hip)[1] >= 4  # (the half-size planar surface at an odd address forces its rounds' general form)
    for k, (pk, spec, fmt) in enumerate(zip(streams, specs, fmts)):
        alone = decode_steps(hip, [pk], Surfaces([spec]))[0]
        same_results(alone, got[k])  # every output equals its single-decoder result
        same_results(in_layout(planar_oracle(pk), spec["layout"], fmt), got[k])


def test_mixed_scales_layouts_and_geometries_in_one_step():
    """Five decoders in one step sequence: 66x34 as full-size NV12, half-size planar at an odd address, quarter-size BGRA and -- two
    steps late -- quarter-size NV12, and 34x18 4:4:4 at an eighth, packed: two geometries, so two rounds a step."""
    mixed_step(bind(A.load_hip()))


def test_mixed_scales_layouts_and_geometries_in_one_step_device_parser():
    hip = bind(A.load_hip())
    try:
        assert hip.dsv2hip_dec_set_parse_mode(2) == 2
        mixed_step(hip)
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)


# ---- 7. sizes ------------------------------------------------------------------------------------------------------------------------
def decoder_with_metadata(hip, packets):
    dec = A.DECODER()
    buf, fn = A.BUF(), C.c_uint32(0)
    mk_buf(hip, buf, packets[0])
    assert hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(buf), C.byref(OUTSURF()), C.byref(fn)) == A.DEC_GOT_META
    return dec


ALL_BASES = [PLANAR, SEMI] + [order | csc for order in (Q.BGRA, Q.RGBA) for csc in Q.CSC]
# include/dsv2_hip.h: 0x1010 (BGRA, default matrix and range, at half size) was "no layout" before the scale values existed
# (tests/test_gpu_dec_rgb.py pins that) and stays refused; every other preset and RGBA deliver at half size
HELD_BACK = Q.BGRA | HALF


def test_half_size_bgra_next_to_the_value_held_back():
    hip = bind(A.load_hip())
    packets = stream(66, 34, "420", 4, 2)
    for layout in (Q.BGRA | Q.BT709 | HALF, Q.BGRA | Q.FULL | HALF, Q.BGRA | Q.BT709 | Q.FULL | HALF, Q.RGBA | HALF, Q.BGRA | QUARTER, Q.BGRA | EIGHTH):
        want, _ = equals_oracle(hip, packets, "420", layout, plus1, offset=1)
        assert npics(want) == 4
    dec = decoder_with_metadata(hip, packets)
    sf = OutSurf(surface_dims(hip, dec, Q.RGBA | HALF), HELD_BACK, aligned)
    sf.arm()
    torch.cuda.synchronize()
    buf, fn = A.BUF(), C.c_uint32(77)
    mk_buf(hip, buf, packets[1])
    assert hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(buf), C.byref(sf.c), C.byref(fn)) == -1
    assert fn.value == 77 and bytes(C.string_at(buf.data, len(packets[1]))) == packets[1] and sf.untouched()
    sf.c.layout = Q.RGBA | HALF
    assert hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(buf), C.byref(sf.c), C.byref(fn)) == A.DEC_OK
    hip.dsv_dec_free(C.byref(dec))


@pytest.mark.parametrize("fmt,w,h", [("420", 34, 18), ("444", 34, 18), ("411", 38, 22), ("420", 130, 258)])
def test_surface_dims_of_every_layout_and_scale(fmt, w, h):
    hip = bind(A.load_hip())
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    fresh = A.DECODER()
    for base in ALL_BASES:
        for s in range(4):
            assert hip.dsv2hip_dec_surface_dims(None, base | SCALE[s], rb, rows) == -1
            assert hip.dsv2hip_dec_surface_dims(C.byref(fresh), base | SCALE[s], rb, rows) == -1  # no metadata yet
    dec = decoder_with_metadata(hip, format_stream(fmt, w, h, 3) if fmt != "420" else stream(w, h, "420", 2, 2))
    _, hs, vs = FMT[fmt]
    for s in range(4):
        ww, hh = (w + (1 << s) - 1) >> s, (h + (1 << s) - 1) >> s
        cw, ch = (ww + (1 << hs) - 1) >> hs, (hh + (1 << vs) - 1) >> vs
        assert surface_dims(hip, dec, PLANAR | SCALE[s]) == [(ww, hh), (cw, ch), (cw, ch)]
        assert surface_dims(hip, dec, SEMI | SCALE[s]) == [(ww, hh), (2 * cw, ch), (0, 0)]
        for base in ALL_BASES[2:]:
            if base | SCALE[s] == HELD_BACK:
                assert surface_dims(hip, dec, HELD_BACK) is None
                continue
            assert surface_dims(hip, dec, base | SCALE[s]) == [(4 * ww, hh), (0, 0), (0, 0)]
    for layout in (0x4000, 0x4000 | PLANAR | HALF, 0x5000, 0x1012, 0x3012, 0x8000 | SEMI, HALF | PLANAR | Q.BT709, EIGHTH | SEMI | Q.FULL, 0x10000 | HALF,
                   -1):
        assert surface_dims(hip, dec, layout) is None, hex(layout)
    # reducing behind the 4:2:0 conversion is out of scope
    assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 1) == 0
    for base in ALL_BASES:
        for s in (1, 2, 3):
            assert surface_dims(hip, dec, base | SCALE[s]) is None
    assert surface_dims(hip, dec, PLANAR) == [(w, h), ((w + 1) >> 1, (h + 1) >> 1), ((w + 1) >> 1, (h + 1) >> 1)]  # (unscaled: as before)
    assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 0) == 0
    assert surface_dims(hip, dec, PLANAR | EIGHTH) is not None
    hip.dsv_dec_free(C.byref(dec))
    hip.dsv_dec_free(C.byref(fresh))


# ---- 8. refusals consume nothing --------------------------------------------------------------------------------------------------------
def spoil_bits(c, rb):
    c.layout |= 0x4000


def spoil_cap(plane):
    def f(c, rb):
        c.cap[plane] -= 1
    return f


def spoil_pitch(plane):
    def f(c, rb):
        c.pitch[plane] = rb[plane] - 1
    return f


REFUSALS = [("bits_0x4000", spoil_bits)] + [("cap_short_%d" % p, spoil_cap(p)) for p in range(3)] + [("pitch_short_%d" % p, spoil_pitch(p)) for p in range(3)]


@pytest.mark.parametrize("layout", [PLANAR | HALF, SEMI | QUARTER, RGBAFULL | EIGHTH], ids=["planar_half", "nv12_quarter", "rgba_eighth"])
def test_refused_calls_consume_nothing(layout):
    """Bits outside the layout, a cap one byte short of the reduced need, a pitch one byte below the reduced row, and a scaled layout
    on an -out420p decoder: -1 from the batch and the one-decoder call, with the packet, the decoder, fn / ret and the surfaces as they
    were -- as the second decoder of a step whose first one is in order; the same packets then decode to the reduction's pictures."""
    hip = bind(A.load_hip())
    w, h = 66, 34
    packets = stream(w, h, "420", 4, 2)
    want = in_layout(planar_oracle(packets), layout, "420")
    decs = [A.DECODER(), A.DECODER()]
    decp = (C.POINTER(A.DECODER) * 2)(*[C.pointer(d) for d in decs])
    fns, rets = (C.c_uint32 * 2)(), (C.c_int * 2)()
    bufs, arr = (A.BUF * 2)(), (OUTSURF * 2)()
    for i in range(2):  # no metadata yet: all-zero entries are allowed, the metadata packets are consumed
        mk_buf(hip, bufs[i], packets[0])
    assert hip.dsv2hip_dec_batch_surface(2, decp, bufs, arr, fns, rets) == 2
    assert list(rets) == [A.DEC_GOT_META] * 2
    dims = surface_dims(hip, decs[0], layout)
    assert dims == expected_dims(decs[0].vidmeta, layout)
    rb = [d[0] for d in dims]
    surfs = [OutSurf(dims, layout, aligned) for _ in decs]
    nplanes = len(surfs[0].t)
    for sf in surfs:
        sf.arm()
    torch.cuda.synchronize()
    for i in range(2):
        mk_buf(hip, bufs[i], packets[1])
    data, lens = [C.cast(bufs[i].data, C.c_void_p).value for i in range(2)], [bufs[i].len for i in range(2)]
    state = [bytes(C.string_at(C.byref(d), C.sizeof(d))) for d in decs]

    def refused(what):
        for i in range(2):
            fns[i], rets[i] = 77, -5
        assert hip.dsv2hip_dec_batch_surface(2, decp, bufs, arr, fns, rets) == -1, what
        one_fn = C.c_uint32(77)
        assert hip.dsv2hip_dec_surface_frame(C.byref(decs[1]), C.byref(bufs[1]), C.byref(arr[1]), C.byref(one_fn)) == -1, what
        assert one_fn.value == 77
        for i in range(2):
            assert C.cast(bufs[i].data, C.c_void_p).value == data[i] and bufs[i].len == lens[i]
            assert bytes(C.string_at(bufs[i].data, len(packets[1]))) == packets[1]
            assert bytes(C.string_at(C.byref(decs[i]), C.sizeof(decs[i]))) == state[i]
            assert fns[i] == 77 and rets[i] == -5
        assert all(sf.untouched() for sf in surfs)

    arr[0] = surfs[0].c
    for what, spoil in REFUSALS:
        if what[-1].isdigit() and int(what[-1]) >= nplanes:
            continue
        C.memmove(C.byref(arr[1]), C.byref(surfs[1].c), C.sizeof(OUTSURF))
        spoil(arr[1], rb)
        refused(what)
    # an -out420p decoder takes no scaled surface; the switch off again, it does
    arr[1] = surfs[1].c
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 1) == 0
    state[1] = bytes(C.string_at(C.byref(decs[1]), C.sizeof(decs[1])))  # (the switch may have made the decoder's private part)
    refused("out420p")
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 0) == 0
    got = [[(A.DEC_GOT_META, None, None)] for _ in range(2)]
    for t in range(1, len(packets)):
        if t > 1:
            for i in range(2):
                mk_buf(hip, bufs[i], packets[t])
                surfs[i].arm()
            torch.cuda.synchronize()
        had_meta = [d.got_metadata for d in decs]
        assert hip.dsv2hip_dec_batch_surface(2, decp, bufs, arr, fns, rets) == 2
        for i in range(2):
            pic = rets[i] == A.DEC_OK and had_meta[i]
            got[i].append((rets[i], fns[i] if pic else None, surfs[i].planes() if pic else None))
    for i in range(2):
        same_results(want, got[i])
        hip.dsv_dec_free(C.byref(decs[i]))


def test_the_encoder_still_refuses_a_scaled_layout():
    """dsv2hip_enc_surface_frame / _batch_surface know no scale: such a layout is an unknown value, refused with the encoder untouched"""
    hip = bind(A.load_hip())
    w, h = 32, 24
    enc = A.ENCODER()
    configure_encoder(hip, enc, A.mk_meta(w, h, A.SUBSAMP_420), qp=50, gop=48)
    t = torch.zeros(w * h * 2, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    encp = (C.POINTER(A.ENCODER) * 1)(C.pointer(enc))
    for base in (PLANAR, SEMI, Q.BGRA, RGBAFULL):
        for s in (1, 2, 3):
            src = SURFACE()
            src.layout = base | SCALE[s]
            for c in range(3):
                src.plane[c], src.pitch[c] = t.data_ptr() + c * w * h // 2, 4 * w
            obufs, nbufs = (A.BUF * 4)(), (C.c_int * 1)()
            assert hip.dsv2hip_enc_surface_frame(C.byref(enc), C.byref(src), obufs) == 0
            assert hip.dsv2hip_enc_batch_surface(1, encp, (SURFACE * 1)(src), obufs, nbufs) == -1
    hip.dsv_enc_free(C.byref(enc))


# ---- 9. a proxy ladder without the host ------------------------------------------------------------------------------------------------
def test_half_size_nv12_goes_straight_into_an_encoder_of_the_reduced_geometry():
    """A 64x48 4:2:0 stream decoded at half size into a pitched NV12 device surface whose pointers and pitches go straight to
    dsv2hip_enc_surface_frame of a 32x24 encoder: the packets are the reference encoder's on the host copy of the same reduced
    planes."""
    ref, hip = A.load_ref(), bind(A.load_hip())
    w, h, layout = 64, 48, SEMI | HALF
    packets = stream(w, h, "420", 4, 4)
    reduced = [B.reduce_picture(pl[0], pl[1], pl[2], 1) for _, _, pl in planar_oracle(packets) if pl is not None]
    assert len(reduced) == 4 and [p.shape for p in reduced[0]] == [(24, 32), (12, 16), (12, 16)]
    want = encode_stream(ref, [b"".join(p.tobytes() for p in pic) for pic in reduced], 32, 24, A.SUBSAMP_420, eos=False, qp=50, gop=48)[0]
    packet_bound_holds(want, 32, 24, A.SUBSAMP_420)
    enc, dec = A.ENCODER(), A.DECODER()
    configure_encoder(hip, enc, A.mk_meta(32, 24, A.SUBSAMP_420), qp=50, gop=48)
    sf = OutSurf([(32, 24), (32, 12), (0, 0)], layout, aligned)
    sf.arm()
    torch.cuda.synchronize()
    src = SURFACE()
    src.layout = SEMI
    for c in range(2):
        src.plane[c], src.pitch[c] = sf.c.plane[c], sf.c.pitch[c]
    got, seen = [], 0
    for pk in packets:
        buf, fn = A.BUF(), C.c_uint32(0)
        mk_buf(hip, buf, pk)
        had_meta = dec.got_metadata
        code = hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(buf), C.byref(sf.c), C.byref(fn))
        if code == A.DEC_EOS:
            break
        if code != A.DEC_OK or not had_meta:
            continue
        obufs = (A.BUF * 4)()
        n = hip.dsv2hip_enc_surface_frame(C.byref(enc), C.byref(src), obufs)
        assert 1 <= n <= 4
        for q in range(n):
            got.append(bytes(C.string_at(obufs[q].data, obufs[q].len)))
            hip.dsv_buf_free(C.byref(obufs[q]))
        y, uv = sf.planes()  # (and the encoder wrote nothing into the surface)
        assert np.array_equal(y, reduced[seen][0]) and np.array_equal(uv, B.interleave(reduced[seen][1], reduced[seen][2]))
        seen += 1
    hip.dsv_enc_free(C.byref(enc))
    hip.dsv_dec_free(C.byref(dec))
    assert seen == 4 and len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a == b, "packet %d differs" % i
