"""Decoded pictures delivered into packed four-byte RGB device surfaces (DSV2HIP_SURFACE_BGRA / _RGBA, or-ed with DSV2HIP_CSC_*,
through dsv2hip_dec_batch_surface / dsv2hip_dec_surface_frame): the surface holds exactly the conversion of include/dsv2_hip.h
(tests/yuv_rgb.py, numpy) of the planar picture that a second decoder of the library delivers from the same packets, under the same
switches, into a PLANAR surface -- a delivery the existing tests pin to the reference decoder.  Both forms of k_egress_rgb, both
byte orders, the four presets, the five chroma formats, the smallest pictures, saturated content that reaches both clamps, rows of
several passes, draw_info and postsharp, RGB and YUV surfaces and two geometries mixed in one step with either parser; every alpha
byte is 255, no byte outside the rows is written, a refused call consumes nothing, and the surface feeds
dsv2hip_enc_surface_frame without a host copy."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsvabi as A
import rgb_csc as R
import yuv_rgb as Q
from codec_run import configure_encoder, encode_stream
from edge_cases import packet_bound_holds
from codec_run import FMT
from dec_out import (OutSurf, Surfaces, aligned, decode_steps, fixed, format_stream, in_layout as as_rgb, is_rgb, npics, packets_of, planar_oracle, plus1,
                     same_results, same_rgb, saturated_stream, stream, tight)
from hipabi import OUTSURF, PLANAR, SEMI, SURFACE, bind, dec_rgb_forms as rgb_forms, dec_uv_forms as uv_forms, mk_buf, reset_dec_forms as reset_forms, surface_dims

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

ORDER = {"bgra": Q.BGRA, "rgba": Q.RGBA}
CSC_IDS = ["bt601", "bt709", "bt601_full", "bt709_full"]


def rgb_equals_oracle(hip, packets, fmt, layout, pitch, offset=0, mode=0, sharp=False):
    got = decode_steps(hip, [packets], Surfaces([dict(layout=layout, pitch=pitch, offset=offset)]), modes=[mode], sharp=[sharp])[0]
    want = planar_oracle(packets, mode, sharp)
    same_rgb(as_rgb(want, layout, fmt), got)
    return want, got


# ---- 1. wide form ------------------------------------------------------------------------------------------------------------
def test_wide_form_equals_the_conversion_of_the_planar_delivery():
    """352x288 4:2:0, 9 pictures in GOPs of 4 (I and P pictures), BGRA at pitch 1536 on an aligned pointer: the 16-byte form in
    every round; the chroma interleave's counts do not move."""
    hip = bind(A.load_hip())
    packets = stream(352, 288, "420", 9, 4)
    assert len(packets) > 9 + 2
    reset_forms(hip)
    want, _ = rgb_equals_oracle(hip, packets, "420", Q.BGRA, fixed(1536))
    assert npics(want) == 9
    assert rgb_forms(hip) == (9, 0)
    assert uv_forms(hip) == (0, 0)


# ---- 2. general form, every format, both byte orders -----------------------------------------------------------------------------
def test_general_form_odd_pitch_and_pointer():
    """354x290 4:2:0 at pitch 4 * w + 1 (every row at another alignment) three bytes behind a 16-byte boundary: rows of more than one
    pass of the workgroup, the last pass partial, the last thread with two pixels of four"""
    hip = bind(A.load_hip())
    reset_forms(hip)
    rgb_equals_oracle(hip, packets_of(354, 290, "420", 3), "420", Q.RGBA | Q.BT709, plus1, offset=3)
    assert rgb_forms(hip) == (0, 3)


@pytest.mark.parametrize("order", sorted(ORDER))
@pytest.mark.parametrize("k,fmt", list(enumerate(sorted(FMT))), ids=sorted(FMT))
def test_general_form_every_format(k, fmt, order):
    hip = bind(A.load_hip())
    reset_forms(hip)
    layout = ORDER[order] | Q.CSC[(k + (order == "rgba")) % 4]
    rgb_equals_oracle(hip, packets_of(176, 144, fmt, 3), fmt, layout, plus1, offset=1 + (k + (order == "rgba")) % 3)
    assert rgb_forms(hip) == (0, 3)
    assert uv_forms(hip) == (0, 0)


# ---- 3. smallest pictures ----------------------------------------------------------------------------------------------------
# 16x16 in every format and both forms; the smallest odd sizes of tests/edge_cases.py (GEOMETRIES), and 22x22 for 4:1:1 / "4:1:0":
# the reference encoder, which makes the streams, divides by zero at 18x18 there (tests/test_gpu_enc_rgb.py)
SMALL = ([(16, 16, fmt, form) for fmt in sorted(FMT) for form in ("wide", "general")] +
         [(18, 16, "420", "general"), (16, 18, "420", "general"), (34, 18, "420", "general"), (30, 22, "422", "general"),
          (22, 22, "411", "general"), (22, 22, "410", "general")])


@pytest.mark.parametrize("w,h,fmt,form", SMALL, ids=["%dx%d-%s-%s" % s for s in SMALL])
def test_smallest_pictures(w, h, fmt, form):
    hip = bind(A.load_hip())
    k = SMALL.index((w, h, fmt, form))
    packets = format_stream(fmt, w, h, 3)
    if FMT[fmt][0] in (A.SUBSAMP_420, A.SUBSAMP_422, A.SUBSAMP_444):
        packet_bound_holds(packets, w, h, FMT[fmt][0])  # (the condition under which the reference encoder is defined at this size)
    layout = (Q.BGRA, Q.RGBA)[k & 1] | Q.CSC[(k >> 1) % 4]
    reset_forms(hip)
    want, _ = rgb_equals_oracle(hip, packets, fmt, layout, aligned if form == "wide" else plus1, offset=0 if form == "wide" else 1 + k % 3)
    assert npics(want) == 3
    assert rgb_forms(hip) == ((3, 0) if form == "wide" else (0, 3))


# ---- 4. saturation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["444", "420"])
@pytest.mark.parametrize("csc", Q.CSC, ids=CSC_IDS)
def test_saturation_reaches_both_clamps(csc, fmt):
    hip = bind(A.load_hip())
    _, hs, vs = FMT[fmt]
    packets, planes = saturated_stream(fmt)
    layout = (Q.RGBA if csc & Q.BT709 else Q.BGRA) | csc
    want, _ = rgb_equals_oracle(hip, packets, fmt, layout, fixed(256))
    pics = [pl for _, _, pl in want if pl is not None]
    assert len(pics) == 2
    for pl in pics:
        assert all(np.array_equal(a, b) for a, b in zip(pl, planes))  # (lossless: the decoded picture is the synthetic one)
    y, u, v = planes
    raw = [s >> 8 for s in Q.sums(csc, y, Q.upsample(u, hs, vs, 64, 48), Q.upsample(v, hs, vs, 64, 48))]
    out = Q.convert(y, u, v, Q.RGBA | csc, hs, vs)
    for c in range(3):
        below, above = raw[c] < 0, raw[c] > 255
        assert below.any() and above.any()  # both clamps are at work in every channel
        assert np.all(out[..., c][below] == 0) and np.all(out[..., c][above] == 255)
        inside = ~below & ~above
        assert np.array_equal(out[..., c][inside], raw[c][inside])


# ---- 5. nothing else is written ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["wide", "general"])
def test_only_the_rows_are_written_and_alpha_is_255(form):
    """The surface is 0xA5 throughout before every step.  Afterwards the 64 bytes in front of plane[0], the padding between the rows
    and the 64 bytes behind the last row -- which has no padding of its own -- still are (OutSurf.planes, after every step), every
    alpha byte is 255 and no colour byte kept the fill by accident of not being written: the picture equals the conversion."""
    hip = bind(A.load_hip())
    w, h = (352, 288) if form == "wide" else (354, 290)
    spec = dict(layout=Q.RGBA | Q.FULL, pitch=aligned if form == "wide" else plus1, offset=0 if form == "wide" else 3)
    packets = packets_of(w, h, "420", 3)
    got = decode_steps(hip, [packets], Surfaces([spec]))[0]
    same_rgb(as_rgb(planar_oracle(packets), spec["layout"], "420"), got)
    pics = [pl[0] for _, _, pl in got if pl is not None]
    assert len(pics) == 3 and all(p.shape == (h, 4 * w) and np.all(p[:, 3::4] == 255) for p in pics)


# ---- 6. rows of several passes -----------------------------------------------------------------------------------------------
def test_1920_wide_rows_take_several_passes():
    """1920x32 4:2:0 with an 8192-byte pitch: 7.5 passes of the workgroup's 256 pixels per row, in the 16-byte form"""
    hip = bind(A.load_hip())
    reset_forms(hip)
    want, _ = rgb_equals_oracle(hip, packets_of(1920, 32, "420", 2), "420", Q.BGRA | Q.BT709, fixed(8192))
    assert npics(want) == 2
    assert rgb_forms(hip) == (2, 0)


# ---- 7. one mixed step -------------------------------------------------------------------------------------------------------
def mixed_step(hip):
    cif, c444 = stream(352, 288, "420", 9, 4), stream(354, 290, "444", 3, 48)
    rgb601, rgb709f = Q.BGRA | Q.BT601, Q.RGBA | Q.BT709 | Q.FULL
    streams = [cif, cif, cif, cif, cif, c444, c444]
    fmts = ["420"] * 5 + ["444"] * 2
    specs = [dict(layout=PLANAR, pitch=tight, offset=0),            # packed: the planar surface with pitch {w, cw, cw}
             dict(layout=PLANAR, pitch=aligned, offset=0),
             dict(layout=SEMI, pitch=aligned, offset=0),            # NV12
             dict(layout=rgb601, pitch=fixed(1536), offset=0),
             dict(layout=rgb709f, pitch=aligned, offset=0),
             dict(layout=rgb709f, pitch=plus1, offset=1),           # the second geometry: a round of its own, in the general form
             dict(layout=PLANAR, pitch=tight, offset=0)]
    reset_forms(hip)
    got = decode_steps(hip, streams, Surfaces(specs))
    # CIF: 9 rounds with two aligned RGB surfaces each; 354x290: 3 rounds with an RGB surface at an odd address
    assert rgb_forms(hip) == (9, 3)
    assert uv_forms(hip)[0] == 9
    for k, (pk, spec, fmt) in enumerate(zip(streams, specs, fmts)):
        alone = decode_steps(hip, [pk], Surfaces([spec]))[0]
        planes = range(len(alone[1][2]))
        same_results(alone, got[k], planes=planes)  # every output equals its single-decoder result
        want = planar_oracle(pk)
        if is_rgb(spec["layout"]):
            same_rgb(as_rgb(want, spec["layout"], fmt), got[k])
        elif spec["layout"] == PLANAR:
            same_results(want, got[k])


def test_mixed_layouts_and_geometries_in_one_step():
    """Seven decoders in one step sequence: CIF packed, planar pitched, NV12, BGRA-601 and RGBA-709-full, and 354x290 4:4:4 as
    RGBA-709-full at an odd address and packed -- two geometries, so two rounds a step, each picking its own form."""
    mixed_step(bind(A.load_hip()))


def test_mixed_layouts_and_geometries_in_one_step_device_parser():
    hip = bind(A.load_hip())
    try:
        assert hip.dsv2hip_dec_set_parse_mode(2) == 2
        mixed_step(hip)
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)


# ---- 8. draw_info and postsharp ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,sharp", [(7, False), (0, True), (7, True)], ids=["draw_info", "postsharp", "both"])
@pytest.mark.parametrize("form", ["wide", "general"])
def test_draw_info_and_postsharp(mode, sharp, form):
    """Both act on the luma the conversion reads, exactly as on the luma plane of the PLANAR delivery under the same switches;
    that delivery differs from the plain one in every picture (the switches are at work), and in luma only."""
    hip = bind(A.load_hip())
    packets = stream(352, 288, "420", 9, 4)
    layout = Q.BGRA | Q.BT709 if form == "wide" else Q.RGBA | Q.FULL
    want, got = rgb_equals_oracle(hip, packets, "420", layout, fixed(1536) if form == "wide" else plus1, offset=0 if form == "wide" else 2,
                                  mode=mode, sharp=sharp)
    plain = planar_oracle(packets)
    same_results(plain, want, planes=(1, 2))
    assert all(not np.array_equal(a[2][0], b[2][0]) for a, b in zip(plain, want) if a[2] is not None)
    assert npics(got) == 9
    # the next decode of the same stream without the switches is the plain one: nothing of them stays in the library
    rgb_equals_oracle(hip, packets, "420", layout, fixed(1536))


# ---- 9. refusals consume nothing ---------------------------------------------------------------------------------------------
def spoil_pitch(c, w):
    c.pitch[0] = 4 * w - 1


def spoil_plane(c, w):
    c.plane[0] = None


def spoil_cap(c, w):
    c.cap[0] -= 1


def spoil_layout(value):
    def f(c, w):
        c.layout = value
    return f


RGB_REFUSALS = [("pitch_short", spoil_pitch), ("null_plane", spoil_plane), ("cap_short", spoil_cap), ("layout_0x12", spoil_layout(0x12)),
                ("layout_0x13", spoil_layout(0x13)), ("layout_0x410", spoil_layout(0x410)), ("layout_0x1010", spoil_layout(0x1010))]


def test_surface_dims_of_rgb_layouts():
    hip = bind(A.load_hip())
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    dec = A.DECODER()
    assert hip.dsv2hip_dec_surface_dims(None, Q.BGRA, rb, rows) == -1
    assert hip.dsv2hip_dec_surface_dims(C.byref(dec), Q.BGRA, rb, rows) == -1  # no metadata yet
    buf, fn = A.BUF(), C.c_uint32(0)
    mk_buf(hip, buf, packets_of(354, 290, "444", 3)[0])
    assert hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(buf), C.byref(OUTSURF()), C.byref(fn)) == A.DEC_GOT_META
    for layout in [order | csc for order in (Q.BGRA, Q.RGBA) for csc in Q.CSC]:
        assert surface_dims(hip, dec, layout) == [(4 * 354, 290), (0, 0), (0, 0)]
    for layout in (0x12, 0x13, 0x410, 0x1010, 0x0F, PLANAR | Q.BT709, SEMI | Q.FULL, PLANAR | Q.BT709 | Q.FULL, -1):
        assert surface_dims(hip, dec, layout) is None, hex(layout)
    assert surface_dims(hip, dec, PLANAR) == [(354, 290)] * 3  # (the YUV layouts as before)
    # an RGB picture has no chroma planes to subsample
    assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 1) == 0
    assert surface_dims(hip, dec, Q.BGRA) is None and surface_dims(hip, dec, Q.RGBA | Q.FULL) is None
    assert surface_dims(hip, dec, PLANAR) == [(354, 290), (177, 145), (177, 145)]
    assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 0) == 0
    assert surface_dims(hip, dec, Q.BGRA) == [(4 * 354, 290), (0, 0), (0, 0)]
    hip.dsv_dec_free(C.byref(dec))


def test_refused_calls_consume_nothing():
    """Every spoiled RGB surface, a CSC bit on PLANAR and on SEMIPLANAR, and an RGB layout on an -out420p decoder: -1 from the batch
    and the one-decoder call, with the packet, the decoder, fn / ret and the surface as they were -- also as the second decoder of a
    step whose first one is in order; the same packets then decode to the conversion's pictures."""
    hip = bind(A.load_hip())
    w, h = 352, 288
    packets = stream(w, h, "420", 9, 4)
    layout = Q.BGRA | Q.BT709
    want = as_rgb(planar_oracle(packets), layout, "420")
    decs = [A.DECODER(), A.DECODER()]
    decp = (C.POINTER(A.DECODER) * 2)(*[C.pointer(d) for d in decs])
    fns, rets = (C.c_uint32 * 2)(), (C.c_int * 2)()
    bufs, arr = (A.BUF * 2)(), (OUTSURF * 2)()
    for i in range(2):  # no metadata yet: all-zero entries are allowed, the metadata packets are consumed
        mk_buf(hip, bufs[i], packets[0])
    assert hip.dsv2hip_dec_batch_surface(2, decp, bufs, arr, fns, rets) == 2
    assert list(rets) == [A.DEC_GOT_META] * 2
    surfs = [OutSurf(surface_dims(hip, d, layout), layout, fixed(1536)) for d in decs]
    yuv = {lay: OutSurf(surface_dims(hip, decs[1], lay), lay, aligned) for lay in (PLANAR, SEMI)}
    for sf in surfs + list(yuv.values()):
        sf.arm()
    torch.cuda.synchronize()
    for i in range(2):
        mk_buf(hip, bufs[i], packets[1])
    data, lens = [C.cast(bufs[i].data, C.c_void_p).value for i in range(2)], [bufs[i].len for i in range(2)]
    state = [bytes(C.string_at(C.byref(d), C.sizeof(d))) for d in decs]

    def nothing_happened():
        for i in range(2):
            assert C.cast(bufs[i].data, C.c_void_p).value == data[i] and bufs[i].len == lens[i]
            assert bytes(C.string_at(bufs[i].data, len(packets[1]))) == packets[1]
            assert bytes(C.string_at(C.byref(decs[i]), C.sizeof(decs[i]))) == state[i]
            assert fns[i] == 77 and rets[i] == -5
        assert all(sf.untouched() for sf in surfs + list(yuv.values()))

    def refused(what):
        for i in range(2):
            fns[i], rets[i] = 77, -5
        assert hip.dsv2hip_dec_batch_surface(2, decp, bufs, arr, fns, rets) == -1, what
        one_fn = C.c_uint32(77)
        assert hip.dsv2hip_dec_surface_frame(C.byref(decs[1]), C.byref(bufs[1]), C.byref(arr[1]), C.byref(one_fn)) == -1, what
        assert one_fn.value == 77
        nothing_happened()

    arr[0] = surfs[0].c
    for what, spoil in RGB_REFUSALS:
        C.memmove(C.byref(arr[1]), C.byref(surfs[1].c), C.sizeof(OUTSURF))
        spoil(arr[1], w)
        refused(what)
    for lay, bit in ((PLANAR, Q.BT709), (SEMI, Q.FULL)):  # a CSC bit on a YUV layout is no layout
        C.memmove(C.byref(arr[1]), C.byref(yuv[lay].c), C.sizeof(OUTSURF))
        arr[1].layout |= bit
        refused("csc_bit_on_%d" % lay)
    # an -out420p decoder takes no RGB surface; the switch off again, it does
    arr[1] = surfs[1].c
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 1) == 0
    state[1] = bytes(C.string_at(C.byref(decs[1]), C.sizeof(decs[1])))  # (the switch may have made the decoder's private part)
    refused("out420p")
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 0) == 0
    # the same packets, the good surfaces: decoded as if nothing had happened, and on to the end of the stream
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
        same_rgb(want, got[i])
        hip.dsv_dec_free(C.byref(decs[i]))


# ---- 10. decode -> RGB -> encode without the host ----------------------------------------------------------------------------
def test_rgba_surface_goes_straight_into_the_encoder():
    """A CIF stream decoded into a pitched RGBA device surface whose pointer and pitch go straight to dsv2hip_enc_surface_frame
    with the same layout: the packets are the reference encoder's on the planar pictures that the encoder's conversion
    (tests/rgb_csc.py) defines on this conversion's pixels."""
    ref, hip = A.load_ref(), bind(A.load_hip())
    w, h, layout = 352, 288, Q.RGBA | Q.BT709
    packets = stream(w, h, "420", 5, 4)
    pixels = [pl[0].reshape(h, w, 4) for _, _, pl in as_rgb(planar_oracle(packets), layout, "420") if pl is not None]
    assert len(pixels) == 5
    want = encode_stream(ref, [R.planar_bytes(p, layout, 1, 1) for p in pixels], w, h, A.SUBSAMP_420, eos=False, qp=50, gop=48)[0]
    enc, dec = A.ENCODER(), A.DECODER()
    configure_encoder(hip, enc, A.mk_meta(w, h, A.SUBSAMP_420), qp=50, gop=48)
    sf = OutSurf([(4 * w, h), (0, 0), (0, 0)], layout, fixed(1536))
    sf.arm()
    torch.cuda.synchronize()
    src = SURFACE()
    src.layout, src.plane[0], src.pitch[0] = layout, sf.c.plane[0], sf.c.pitch[0]
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
        assert np.array_equal(sf.planes()[0].reshape(h, w, 4), pixels[seen])  # (and the encoder wrote nothing into the surface)
        seen += 1
    hip.dsv_enc_free(C.byref(enc))
    hip.dsv_dec_free(C.byref(dec))
    assert seen == 5 and len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a == b, "packet %d differs" % i
