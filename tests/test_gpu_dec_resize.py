"""Decoded pictures delivered at any smaller size (dsv2hip_dec_batch_surface_sized / dsv2hip_dec_surface_frame_sized /
dsv2hip_dec_sized_dims): the surface holds exactly the area average of include/dsv2_hip.h (tests/area_resize.py, numpy) -- then the
chroma interleave, or the header's RGB conversion (tests/yuv_rgb.py) -- of the planar picture that a second decoder of the library
delivers from the same packets, under the same switches, into a full-size PLANAR surface: a delivery the existing tests pin to the
reference decoder.  Ratios of two and nine taps, one axis only, exact ratios, the identity, planes of more than one workgroup, both
forms of k_egress_resize, the five chroma formats, saturated content, draw_info and postsharp in front of the resampling, sized, scaled
and plain entries mixed in one step with either parser, the staging picture growing on one decoder; no byte outside the sized rows is
written, a refused call consumes nothing, and a sized NV12 surface feeds an encoder of that geometry without the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import area_resize as R
import box_reduce as B
import dsvabi as A
import yuv_rgb as Q
from codec_run import configure_encoder, encode_stream
from edge_cases import packet_bound_holds
from codec_run import FMT, meta_packet
from dec_out import (OutSurf, Sized, Surfaces, aligned, content_stream, decode_steps, expected_dims, format_stream, in_layout, is_rgb, npics, planar_oracle,
                     plus1, same_results, stream, tight)
from hipabi import (EIGHTH, HALF, OUTSURF, PLANAR, QUARTER, SEMI, SURFACE, bind, dec_resize_forms as resize_forms, dec_rgb_forms as rgb_forms,
                    dec_scale_forms as scale_forms, dec_uv_forms as uv_forms, mk_buf, reset_dec_forms as reset_every, sized_dims)

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

DECP = C.POINTER(A.DECODER)
BGRA709, RGBAFULL = Q.BGRA | Q.BT709, Q.RGBA | Q.FULL
LAYOUTS = [PLANAR, SEMI, BGRA709, RGBAFULL]
LAYOUT_IDS = ["planar", "semiplanar", "bgra709", "rgba601full"]


def documented_wide(dims, layout, pitch, offset):
    """include/dsv2_hip.h at dsv2hip_dec_resize_stats: every resampled plane that goes straight into the caller's surface (PLANAR: all
    three, SEMIPLANAR: luma, RGB: none) has pointer and pitch multiples of 4 and a width that is a multiple of 4"""
    straight = [] if is_rgb(layout) else dims[:1] if layout == SEMI else dims
    return all(offset % 4 == 0 and pitch(rb) % 4 == 0 and rb % 4 == 0 for rb, _ in straight)


def equals_oracle(hip, packets, fmt, layout, size, pitch, offset=0, mode=0, sharp=False):
    got = decode_steps(hip, [packets], Sized([dict(layout=layout, pitch=pitch, offset=offset, size=size)]), modes=[mode], sharp=[sharp])[0]
    want = planar_oracle(packets, mode, sharp)
    same_results(in_layout(want, layout, fmt, size), got)
    return want, got


# ---- 1. sizes x layouts ------------------------------------------------------------------------------------------------------------------
# two taps an axis; both sizes odd (luma 50x38 -> 33x21, chroma 25x19 -> 17x11); ratios near 8 (8 - 9 taps); one axis only, each; an
# exact ratio of 8; the identity; 176x144 -> 117x96: more than one workgroup per plane (24 of 4 rows) -- a workgroup covers 256 samples
# of a row, so a row of more than one takes a width beyond what a test of a few seconds decodes: tools/egress_resize_check.cpp runs
# those.  GOPs of 2: I and P pictures in every stream
CASES = [(48, 32, 32, 24), (50, 38, 33, 21), (64, 48, 9, 7), (64, 48, 64, 6), (64, 48, 8, 48), (16, 16, 2, 2), (16, 16, 16, 16), (176, 144, 117, 96)]
VARIANTS = [(aligned, 0), (plus1, 1)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("w,h,ow,oh", CASES, ids=["%dx%d-%dx%d" % g for g in CASES])
def test_equals_the_area_average_of_the_planar_delivery(w, h, ow, oh, layout):
    hip = bind(A.load_hip())
    packets = stream(w, h, "420", 4, 2)
    packet_bound_holds(packets, w, h, A.SUBSAMP_420)  # (the condition under which the reference encoder is defined at this size)
    kinds = {pk[5] & 1 for pk in packets if pk[5] & 0x04}  # (dsv.h: packet type at byte 5, picture = 0x04, bit 0 = predicted)
    assert kinds == {0, 1}  # I and P pictures both occur
    for pitch, offset in VARIANTS:
        reset_every(hip)
        want, got = equals_oracle(hip, packets, "420", layout, (ow, oh), pitch, offset)
        assert npics(want) == npics(got) == 4
        dims = [(pl.shape[1], pl.shape[0]) for pl in next(pl for _, _, pl in got if pl is not None)]
        assert dims[0] == ((4 if is_rgb(layout) else 1) * ow, oh)
        if (ow, oh) == (w, h):
            assert resize_forms(hip) == (0, 0)  # the picture's own size is the plain delivery
        else:
            assert resize_forms(hip) == ((4, 0) if documented_wide(dims, layout, pitch, offset) else (0, 4))
        assert scale_forms(hip) == (0, 0)  # a sized picture counts in the resize statistic only
        assert sum(rgb_forms(hip)) == (4 if is_rgb(layout) else 0) and sum(uv_forms(hip)) == (4 if layout == SEMI else 0)


def test_both_forms_are_reached_by_the_cases_above():
    seen = set()
    for w, h, ow, oh in CASES:
        for layout in LAYOUTS:
            dims = [d for d in expected_dims(A.mk_meta(w, h, A.SUBSAMP_420), layout, (ow, oh)) if d[1]]
            for pitch, offset in VARIANTS:
                seen.add((layout, documented_wide(dims, layout, pitch, offset)))
    assert seen == {(layout, wide) for layout in LAYOUTS for wide in (True, False)} - {(BGRA709, False), (RGBAFULL, False)}


def test_a_pointer_that_is_a_multiple_of_4_only_keeps_the_wide_form():
    """64x48 -> 32x24 planar: widths 32 and 16; wide at offset 4, general at offset 2"""
    hip = bind(A.load_hip())
    packets = stream(64, 48, "420", 4, 2)
    reset_every(hip)
    equals_oracle(hip, packets, "420", PLANAR, (32, 24), aligned, offset=4)
    assert resize_forms(hip) == (4, 0)
    equals_oracle(hip, packets, "420", PLANAR, (32, 24), aligned, offset=2)
    assert resize_forms(hip) == (4, 4)
    assert scale_forms(hip) == (0, 0) and sum(rgb_forms(hip)) == 0 and sum(uv_forms(hip)) == 0


# ---- 2. the five chroma formats ------------------------------------------------------------------------------------------------------
# 50x38 -> 33x21.  4:1:1 and "4:1:0" at 54x38 -> 33x21: the reference encoder, which makes the streams, divides by zero at 50x38 in
# these two formats (as at the sizes tests/test_gpu_dec_scale.py names); chroma there 14x38 -> 9x21 and 14x19 -> 9x11, odd ratios too
FORMAT_SIZE = {"444": (50, 38), "422": (50, 38), "420": (50, 38), "411": (54, 38), "410": (54, 38)}


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_every_chroma_format(fmt):
    hip = bind(A.load_hip())
    w, h = FORMAT_SIZE[fmt]
    packets = format_stream(fmt, w, h, 3)
    for k, layout in enumerate(LAYOUTS):
        pitch, offset = VARIANTS[k % 2]
        want, _ = equals_oracle(hip, packets, fmt, layout, (33, 21), pitch, offset)
        assert npics(want) == 3


# ---- 3. saturated content -------------------------------------------------------------------------------------------------------------
# 64x48 -> 9x7; white and black lossless; the checkerboard at quantiser 30 (tests/test_gpu_dec_scale.py: finer, the reference encoder's
# packets of this content leave the bound inside which it is defined)
@pytest.mark.parametrize("kind,qp", [("white", 100), ("black", 100), ("checker", 30)], ids=["white", "black", "checker"])
def test_saturated_content(kind, qp):
    """255 stays 255 and 0 stays 0 at a ratio of 64 / 9 by 48 / 7 (D = 64 * 48): the rounding never carries a constant plane out of
    its value"""
    hip = bind(A.load_hip())
    packets = content_stream(kind, 64, 48, qp)
    full = planar_oracle(packets)
    assert npics(full) == 3
    if kind != "checker":
        value = 255 if kind == "white" else 0
        assert all(np.all(p == value) for _, _, pl in full if pl is not None for p in pl)  # (lossless: the decoded picture is the constant)
    _, got = equals_oracle(hip, packets, "420", PLANAR, (9, 7), plus1, offset=1)
    if kind != "checker":
        assert all(np.all(p == value) for _, _, pl in got if pl is not None for p in pl)
    equals_oracle(hip, packets, "420", RGBAFULL, (9, 7), tight)
    equals_oracle(hip, packets, "420", SEMI, (9, 7), aligned)


# ---- 4. draw_info and postsharp act in front of the resampling ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,sharp", [(1, False), (2, False), (4, False), (8, False), (0, True), (7, True)],
                         ids=["draw1", "draw2", "draw4", "draw8", "postsharp", "both"])
@pytest.mark.parametrize("layout", [PLANAR, BGRA709], ids=["planar", "bgra709"])
def test_draw_info_and_postsharp(layout, mode, sharp):
    """The sized picture is the resampling of the drawn-on / sharpened full-size picture (the staged-luma paths); chroma is the plain
    picture's.  With the switches on for the first picture alone, every later picture -- the P picture that predicts from it first of
    all -- is the plain one: the picture predicted from is never touched."""
    hip = bind(A.load_hip())
    packets = stream(66, 34, "420", 4, 4)
    size = (44, 23)
    want, got = equals_oracle(hip, packets, "420", layout, size, plus1, offset=1, mode=mode, sharp=sharp)
    plain = planar_oracle(packets)
    same_results(plain, want, planes=(1, 2))
    if mode in (0, 7, 8):  # (the grid and the sharpening show in every picture; dashes, vectors and marks only where the stream has them)
        assert all(not np.array_equal(a[2][0], b[2][0]) for a, b in zip(plain, want) if a[2] is not None)
    assert npics(got) == 4
    first = next(i for i, r in enumerate(plain) if r[2] is not None)
    once = decode_steps(hip, [packets], Sized([dict(layout=layout, pitch=aligned, offset=0, size=size)]), modes=[lambda t: mode if t <= first else 0],
                        sharp=[lambda t: sharp and t <= first])[0]
    mixed = [w_ if i <= first else p for i, (w_, p) in enumerate(zip(want, plain))]
    same_results(in_layout(mixed, layout, "420", size), once)


# ---- 5. one mixed step ---------------------------------------------------------------------------------------------------------------
def mixed_step(hip):
    a, b = stream(66, 34, "420", 4, 2), format_stream("444", 50, 38, 3)
    streams = [a, a, a, b, a]
    fmts = ["420", "420", "420", "444", "420"]
    specs = [dict(layout=SEMI, pitch=aligned, offset=0, size=None),               # full-size NV12, not sized
             dict(layout=BGRA709 | QUARTER, pitch=aligned, offset=0, size=None),  # quarter-size BGRA, not sized
             dict(layout=PLANAR, pitch=plus1, offset=1, size=(44, 23)),           # sized planar of the same stream, the same round
             dict(layout=SEMI, pitch=tight, offset=0, size=(33, 21)),             # the second geometry: a round of its own
             dict(layout=RGBAFULL, pitch=tight, offset=0, size=(9, 5))]           # joins two steps late: no metadata beside decoders with pictures
    delay = [0, 0, 0, 0, 2]
    reset_every(hip)
    got = decode_steps(hip, streams, Sized(specs), delay=delay)
    assert resize_forms(hip)[1] >= 4 and sum(scale_forms(hip)) >= 4  # (the sized planar surface at an odd address: its rounds' general form)
    for k, (pk, spec, fmt) in enumerate(zip(streams, specs, fmts)):
        same_results(in_layout(planar_oracle(pk), spec["layout"], fmt, spec["size"]), got[k])
        if spec["size"] is None:  # byte-identical to the plain call's
            same_results(decode_steps(hip, [pk], Surfaces([dict(layout=spec["layout"], pitch=spec["pitch"], offset=spec["offset"])]))[0], got[k])
        else:
            same_results(decode_steps(hip, [pk], Sized([spec]), single=True)[0], got[k])  # ... to the one-decoder call's


def test_sized_scaled_and_plain_entries_in_one_step():
    """Five decoders in one step sequence: 66x34 as full-size NV12 and as quarter-size BGRA (not sized), sized planar 44x23 at an odd
    address and -- two steps late -- sized RGBA 9x5, and 50x38 4:4:4 sized to NV24 33x21: two geometries, so two rounds a step."""
    mixed_step(bind(A.load_hip()))


def test_sized_scaled_and_plain_entries_in_one_step_device_parser():
    hip = bind(A.load_hip())
    try:
        assert hip.dsv2hip_dec_set_parse_mode(2) == 2
        mixed_step(hip)
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)


# ---- 6. the picture's own size; the one-decoder call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_own_size_is_the_plain_delivery_and_frame_sized_is_the_batch_call(layout):
    hip = bind(A.load_hip())
    packets = stream(50, 38, "420", 4, 2)
    plain = decode_steps(hip, [packets], Surfaces([dict(layout=layout, pitch=plus1, offset=1)]), modes=[7], sharp=[True])[0]
    reset_every(hip)
    own = decode_steps(hip, [packets], Sized([dict(layout=layout, pitch=plus1, offset=1, size=(50, 38))]), modes=[7], sharp=[True])[0]
    assert resize_forms(hip) == (0, 0)
    same_results(plain, own)
    batch = decode_steps(hip, [packets], Sized([dict(layout=layout, pitch=plus1, offset=1, size=(33, 21))]), modes=[7], sharp=[True])[0]
    one = decode_steps(hip, [packets], Sized([dict(layout=layout, pitch=plus1, offset=1, size=(33, 21))]), modes=[7], sharp=[True], single=True)[0]
    assert npics(batch) == 4
    same_results(batch, one)


# ---- 7. the staging picture grows on one decoder -------------------------------------------------------------------------------------------
def test_the_staging_picture_grows_on_one_decoder():
    """ONE decoder of a 64x48 stream: half-size NV12 first (the staging picture at half size), then sized NV12 at 63x47 (chroma 32x24 of
    32x24: the staging picture at the planes' own size), then eighth-size BGRA (the grown staging, reduced planes in its top left)"""
    hip = bind(A.load_hip())
    packets = stream(64, 48, "420", 3, 3)
    oracle = planar_oracle(packets)
    assert npics(oracle) == 3
    plan = [(SEMI | HALF, None), (SEMI, (63, 47)), (BGRA709 | EIGHTH, None)]
    dec = A.DECODER()
    seen = 0
    for i, pk in enumerate(packets):
        buf, fn = A.BUF(), C.c_uint32(0)
        mk_buf(hip, buf, pk)
        if not dec.got_metadata:
            assert hip.dsv2hip_dec_surface_frame_sized(C.byref(dec), C.byref(buf), C.byref(OUTSURF()), 0, 0, C.byref(fn)) == A.DEC_GOT_META
            continue
        layout, size = plan[min(seen, 2)]
        ow, oh = size or (0, 0)
        sf = OutSurf(sized_dims(hip, dec, layout, ow, oh), layout, aligned)
        sf.arm()
        torch.cuda.synchronize()
        code = hip.dsv2hip_dec_surface_frame_sized(C.byref(dec), C.byref(buf), C.byref(sf.c), ow, oh, C.byref(fn))
        assert code == oracle[i][0]
        if oracle[i][2] is None:
            assert sf.untouched()
            continue
        want = in_layout([oracle[i]], layout, "420", size)[0]
        assert fn.value == want[1]
        for a, b in zip(want[2], sf.planes()):
            assert np.array_equal(a, b), "picture %d" % seen
        seen += 1
    assert seen == 3
    hip.dsv_dec_free(C.byref(dec))


# ---- 8. refusals consume nothing --------------------------------------------------------------------------------------------------------
def test_sized_dims_of_a_null_and_a_fresh_decoder():
    hip = bind(A.load_hip())
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    fresh = A.DECODER()
    for layout in LAYOUTS:
        assert hip.dsv2hip_dec_sized_dims(None, layout, 8, 8, rb, rows) == -1
        assert hip.dsv2hip_dec_sized_dims(C.byref(fresh), layout, 8, 8, rb, rows) == -1  # no metadata yet
        assert hip.dsv2hip_dec_sized_dims(C.byref(fresh), layout, 0, 0, rb, rows) == -1
    hip.dsv_dec_free(C.byref(fresh))


# (what, bits or-ed into the layout -- None: the value 0x12, no layout --, out_w, out_h) on a 66x34 stream; 8 * 8 = 64 < 66 and 8 * 4 = 32 < 34
BAD_SIZES = [("w_zero", 0, 0, 20), ("h_zero", 0, 40, 0), ("w_negative", 0, -40, 20), ("h_negative", 0, 40, -20), ("both_negative", 0, -1, -1),
             ("w_above", 0, 67, 34), ("h_above", 0, 66, 35), ("w_below_an_eighth", 0, 8, 20), ("h_below_an_eighth", 0, 40, 4),
             ("half_and_size", HALF, 33, 17), ("quarter_and_own_size", QUARTER, 66, 34), ("eighth_and_size", EIGHTH, 40, 20),
             ("bits_0x4000", 0x4000, 40, 20), ("no_layout_0x12", None, 40, 20)]


def spoil_cap(plane):
    def f(c, rb):
        c.cap[plane] -= 1
    return f


def spoil_pitch(plane):
    def f(c, rb):
        c.pitch[plane] = rb[plane] - 1
    return f


def spoil_plane(c, rb):
    c.plane[0] = None


@pytest.mark.parametrize("layout", [PLANAR, SEMI, RGBAFULL], ids=["planar", "nv12", "rgba"])
def test_refused_calls_consume_nothing(layout):
    """Every refusal of include/dsv2_hip.h: -1 from the batch and the one-decoder call and from dsv2hip_dec_sized_dims, with the packet,
    the decoder, fn / ret and the surfaces as they were -- as the second decoder of a step whose first one is in order; the same
    packets then decode to the resampling's pictures."""
    hip = bind(A.load_hip())
    w, h, size = 66, 34, (40, 20)
    packets = stream(w, h, "420", 4, 2)
    want = in_layout(planar_oracle(packets), layout, "420", size)
    decs = [A.DECODER(), A.DECODER()]
    decp = (DECP * 2)(*[C.pointer(d) for d in decs])
    fns, rets = (C.c_uint32 * 2)(), (C.c_int * 2)()
    bufs, arr = (A.BUF * 2)(), (OUTSURF * 2)()
    ows, ohs = (C.c_int * 2)(-7, 1000), (C.c_int * 2)(0, -3)
    for i in range(2):  # no metadata yet: all-zero entries and any sizes are allowed, the metadata packets are consumed
        mk_buf(hip, bufs[i], packets[0])
    assert hip.dsv2hip_dec_batch_surface_sized(2, decp, bufs, arr, ows, ohs, fns, rets) == 2
    assert list(rets) == [A.DEC_GOT_META] * 2
    dims = sized_dims(hip, decs[0], layout, *size)
    assert dims == expected_dims(decs[0].vidmeta, layout, size)
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

    def refused(what, pw, ph):
        for i in range(2):
            fns[i], rets[i] = 77, -5
        assert hip.dsv2hip_dec_batch_surface_sized(2, decp, bufs, arr, pw, ph, fns, rets) == -1, what
        one_fn = C.c_uint32(77)
        one_w, one_h = (pw[1], ph[1]) if pw and ph else (size[0], size[1])
        if pw and ph:
            assert hip.dsv2hip_dec_surface_frame_sized(C.byref(decs[1]), C.byref(bufs[1]), C.byref(arr[1]), one_w, one_h, C.byref(one_fn)) == -1, what
        assert one_fn.value == 77
        for i in range(2):
            assert C.cast(bufs[i].data, C.c_void_p).value == data[i] and bufs[i].len == lens[i]
            assert bytes(C.string_at(bufs[i].data, len(packets[1]))) == packets[1]
            assert bytes(C.string_at(C.byref(decs[i]), C.sizeof(decs[i]))) == state[i]
            assert fns[i] == 77 and rets[i] == -5
        assert all(sf.untouched() for sf in surfs)

    def sizes(ow, oh):
        return (C.c_int * 2)(size[0], ow), (C.c_int * 2)(size[1], oh)

    arr[0], arr[1] = surfs[0].c, surfs[1].c
    none = C.POINTER(C.c_int)()
    good_w, good_h = sizes(*size)
    refused("null out_w", none, good_h)
    refused("null out_h", good_w, none)
    for what, bits, ow, oh in BAD_SIZES:
        C.memmove(C.byref(arr[1]), C.byref(surfs[1].c), C.sizeof(OUTSURF))
        arr[1].layout = 0x12 if bits is None else layout | bits
        assert sized_dims(hip, decs[1], arr[1].layout, ow, oh) is None, what
        refused(what, *sizes(ow, oh))
    spoils = [("cap_short_%d" % p, spoil_cap(p)) for p in range(nplanes)] + [("pitch_short_%d" % p, spoil_pitch(p)) for p in range(nplanes)]
    for what, spoil in spoils + [("null_plane", spoil_plane)]:  # everything the plain call refuses, against the sized rows
        C.memmove(C.byref(arr[1]), C.byref(surfs[1].c), C.sizeof(OUTSURF))
        spoil(arr[1], rb)
        refused(what, good_w, good_h)
    # an -out420p decoder takes no sized entry, at its own size neither; the switch off again, it does
    arr[1] = surfs[1].c
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 1) == 0
    state[1] = bytes(C.string_at(C.byref(decs[1]), C.sizeof(decs[1])))  # (the switch may have made the decoder's private part)
    assert sized_dims(hip, decs[1], layout, *size) is None and sized_dims(hip, decs[1], layout, w, h) is None
    refused("out420p", good_w, good_h)
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 0) == 0
    got = [[(A.DEC_GOT_META, None, None)] for _ in range(2)]
    for t in range(1, len(packets)):
        if t > 1:
            for i in range(2):
                mk_buf(hip, bufs[i], packets[t])
                surfs[i].arm()
            torch.cuda.synchronize()
        had_meta = [d.got_metadata for d in decs]
        assert hip.dsv2hip_dec_batch_surface_sized(2, decp, bufs, arr, good_w, good_h, fns, rets) == 2
        for i in range(2):
            pic = rets[i] == A.DEC_OK and had_meta[i]
            got[i].append((rets[i], fns[i] if pic else None, surfs[i].planes() if pic else None))
    for i in range(2):
        same_results(want, got[i])
        hip.dsv_dec_free(C.byref(decs[i]))


# (w, h, out_w, out_h, accepted) for a 4:2:0 decoder whose metadata says w x h.  4100^2 > 2^24: the luma's D; a gcd of 2 halves a and c.
# 8194 -> 4097 is 2 : 1 for the luma (D = 4) and 4097 -> 2049 in lowest terms for the chroma: 4097^2 > 2^24, the chroma's D alone; with
# one axis at its own size the chroma's D is 4097
BIG = [(4100, 4100, 4099, 4099, False), (4100, 4100, 4098, 4098, True), (4100, 4100, 4099, 4100, True),
       (8194, 8194, 4097, 4097, False), (8194, 8194, 4097, 8194, True), (8194, 8194, 8194, 4097, True)]


@pytest.mark.parametrize("w,h", [(4100, 4100), (8194, 8194)], ids=["luma_4100", "chroma_8194"])
def test_sizes_beyond_what_32_bit_sums_hold_are_refused(w, h):
    """D > 2^24, for the luma and for the chroma alone: a decoder that has read a metadata packet of such a size -- nothing is allocated
    for a geometry before its first picture -- answers -1 from dsv2hip_dec_sized_dims, the batch call and the one-decoder call, with the
    packet, the decoder, fn / ret and the surface as they were; the accepted neighbours get their plane sizes.  (A plane side above
    32 768 cannot be reached through a packet, the decoder taking metadata of up to 16 384 a side: tests/test_egress_resize_cpu.py
    pins that bound, as every other, on the rule the calls refuse by.)"""
    hip = bind(A.load_hip())
    dec = A.DECODER()
    buf, fn = A.BUF(), C.c_uint32(0)
    mk_buf(hip, buf, meta_packet((w, h, A.SUBSAMP_420, 30, 1, 1, 1, 1)))
    assert hip.dsv2hip_dec_surface_frame_sized(C.byref(dec), C.byref(buf), C.byref(OUTSURF()), 0, 0, C.byref(fn)) == A.DEC_GOT_META
    assert (dec.vidmeta.width, dec.vidmeta.height, dec.vidmeta.subsamp) == (w, h, A.SUBSAMP_420)
    picture = stream(64, 48, "420", 4, 2)[1]
    sf = OutSurf([(64, 8), (32, 4), (32, 4)], PLANAR, aligned)  # (refused before a plane is looked at)
    sf.arm()
    torch.cuda.synchronize()
    mk_buf(hip, buf, picture)
    data, length = C.cast(buf.data, C.c_void_p).value, buf.len
    state = bytes(C.string_at(C.byref(dec), C.sizeof(dec)))
    decp = (DECP * 1)(C.pointer(dec))
    seen = set()
    for pw, ph, ow, oh, accepted in BIG:
        if (pw, ph) != (w, h):
            continue
        luma, chroma = R.allowed(pw, ph, ow, oh), R.allowed((pw + 1) // 2, (ph + 1) // 2, (ow + 1) // 2, (oh + 1) // 2)
        assert accepted == (luma and chroma) and (accepted or luma == (w == 8194))  # (refused by the luma's D at 4100, by the chroma's alone at 8194)
        seen.add(accepted)
        for layout in LAYOUTS:
            dims = sized_dims(hip, dec, layout, ow, oh)
            if accepted:
                assert dims == expected_dims(dec.vidmeta, layout, (ow, oh)), (layout, ow, oh)
                continue
            assert dims is None, (layout, ow, oh)
            sf.c.layout = layout
            fns, rets = (C.c_uint32 * 1)(77), (C.c_int * 1)(-5)
            assert hip.dsv2hip_dec_batch_surface_sized(1, decp, buf, (OUTSURF * 1)(sf.c), (C.c_int * 1)(ow), (C.c_int * 1)(oh), fns, rets) == -1
            one_fn = C.c_uint32(77)
            assert hip.dsv2hip_dec_surface_frame_sized(C.byref(dec), C.byref(buf), C.byref(sf.c), ow, oh, C.byref(one_fn)) == -1
            assert fns[0] == 77 and rets[0] == -5 and one_fn.value == 77
            assert C.cast(buf.data, C.c_void_p).value == data and buf.len == length and bytes(C.string_at(buf.data, len(picture))) == picture
            assert bytes(C.string_at(C.byref(dec), C.sizeof(dec))) == state and sf.untouched()
    assert seen == {True, False}
    hip.dsv_buf_free(C.byref(buf))
    hip.dsv_dec_free(C.byref(dec))


# ---- 9. a rendition ladder without the host ----------------------------------------------------------------------------------------------
def test_sized_nv12_goes_straight_into_an_encoder_of_that_geometry():
    """A 64x48 4:2:0 stream delivered sized to 48x32 into a pitched NV12 device surface whose pointers and pitches go straight to
    dsv2hip_enc_surface_frame of a 48x32 encoder: the packets are the reference encoder's on the oracle's planes."""
    ref, hip = A.load_ref(), bind(A.load_hip())
    w, h, size = 64, 48, (48, 32)
    packets = stream(w, h, "420", 4, 4)
    sized = [R.resize_picture(pl[0], pl[1], pl[2], size[0], size[1], 1, 1) for _, _, pl in planar_oracle(packets) if pl is not None]
    assert len(sized) == 4 and [p.shape for p in sized[0]] == [(32, 48), (16, 24), (16, 24)]
    want = encode_stream(ref, [b"".join(p.tobytes() for p in pic) for pic in sized], 48, 32, A.SUBSAMP_420, eos=False, qp=50, gop=48)[0]
    packet_bound_holds(want, 48, 32, A.SUBSAMP_420)
    enc, dec = A.ENCODER(), A.DECODER()
    configure_encoder(hip, enc, A.mk_meta(48, 32, A.SUBSAMP_420), qp=50, gop=48)
    sf = OutSurf([(48, 32), (48, 16), (0, 0)], SEMI, aligned)
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
        code = hip.dsv2hip_dec_surface_frame_sized(C.byref(dec), C.byref(buf), C.byref(sf.c), size[0], size[1], C.byref(fn))
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
        assert np.array_equal(y, sized[seen][0]) and np.array_equal(uv, B.interleave(sized[seen][1], sized[seen][2]))
        seen += 1
    hip.dsv_enc_free(C.byref(enc))
    hip.dsv_dec_free(C.byref(dec))
    assert seen == 4 and len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a == b, "packet %d differs" % i
