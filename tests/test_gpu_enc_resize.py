"""Ingest at any larger size (dsv2hip_enc_batch_surface_sized, dsv2hip_enc_surface_frame_sized): an encoder of W x H reads a planar,
NV12, BGRA or RGBA device surface of src_w x src_h, W <= src_w <= 8 W and H <= src_h <= 8 H, and its packets are the reference
encoder's on the planes that include/dsv2_hip.h defines (tests/ingest_resize.py, numpy) -- both forms of both kernels, two to
thirty taps a sample, one axis only, exact ratios, the five chroma formats, an output row of more than one workgroup, saturated
content, plain, scaled and sized surfaces mixed in one step; the surface is never written, a refused call touches nothing, and a
picture decoded at full size and encoded through the sized call gives the packets of the same picture decoded at that size and
encoded through the plain call.

The reference streams and the cases are tests/enc_resize_cases.py's; tests/test_ingest_resize_ref.py checks each stream's two
conditions without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import area_resize as AR
import dsvabi as A
import enc_in as EI
import enc_resize_cases as K
import ingest_resize as IR
import rgb_csc as R
from codec_run import FMT, configure_encoder, encode_stream
from edge_cases import packet_bound_holds
from dec_out import OutSurf, aligned as aligned_out, planar_oracle, stream
from enc_in import content, copy_of, encode_steps, encoders, is_rgb, kind_of, rgb_content, same_packets, take_packets
from hipabi import (HALF, PLANAR, SEMI, SURFACE, bind, enc_resize_forms as resize_forms, enc_rgb_forms as rgb_forms, enc_scale_forms as scale_forms,
                    enc_yuv_forms as yuv_forms, mk_buf, reset_enc_forms as reset_all)

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

CFG, NFR, SEED = K.CFG, K.NFR, K.SEED
BGRA709, RGBAFULL, LAYOUTS, LAYOUT_IDS, VARIANTS = K.BGRA709, K.RGBAFULL, K.LAYOUTS, K.LAYOUT_IDS, K.VARIANTS


sized_steps = functools.partial(encode_steps, nfr=NFR, call="dsv2hip_enc_batch_surface_sized")


def source(sw, sh, name, layout, variant, t, offset=None, s=0):
    """picture t of the content made at sw x sh as a device surface; s: the scale value of its layout (0: a sized or plain entry)"""
    if is_rgb(layout):
        return EI.rgb_source(rgb_content(sw, sh, NFR, SEED)[t], layout, s, variant, offset)
    return EI.yuv_source(content(sw, sh, name, NFR, SEED)[t], sw, sh, name, layout, s, variant, offset)


def documented_wide(sw, sh, name, layout, variant, offset=None):
    """include/dsv2_hip.h at dsv2hip_enc_resize_stats: YUV -- every sized source plane's pointer, pitch and SOURCE row bytes are
    multiples of 4; RGB -- pointer and pitch multiples of 4.  (The tensors start 16-byte aligned and the guard in front is 64 bytes.)"""
    _, hs, vs = FMT[name]
    off = EI.offset_of(variant) if offset is None else offset
    if is_rgb(layout):
        return off % 4 == 0 and EI.pitch_of(4 * sw, variant) % 4 == 0
    return all(off % 4 == 0 and EI.pitch_of(rb, variant) % 4 == 0 and rb % 4 == 0 for rb, _ in IR.source_dims(sw, sh, hs, vs, layout))


def encode_sized(hip, sw, sh, w, h, name, layout, variant, offset=None, cfg=CFG, s=0):
    encs = encoders(hip, w, h, name, 1, cfg)
    got = sized_steps(hip, encs, lambda k, t: (source(sw, sh, name, layout, variant, t, offset, s), sw, sh))
    hip.dsv_enc_free(C.byref(encs[0]))
    return got[0]


def parity_case(sw, sh, w, h, name, layout, variant, offset=None):
    """the packets are the reference's, and the step ran in the form the documented rule names"""
    hip = bind(A.load_hip())
    reset_all(hip)
    want = K.reference(sw, sh, w, h, name, kind_of(layout))
    got = encode_sized(hip, sw, sh, w, h, name, layout, variant, offset)
    same_packets(want, got)
    wide = documented_wide(sw, sh, name, layout, variant, offset)
    at = (2 if is_rgb(layout) else 0) + (0 if wide else 1)
    assert resize_forms(hip) == tuple(NFR if i == at else 0 for i in range(4))
    assert scale_forms(hip) == (0, 0, 0, 0) and rgb_forms(hip) == (0, 0) and yuv_forms(hip) == (0, 0)  # (sized entries count here only)


# ---- 1. every 4:2:0 source x layout x pitch / alignment ------------------------------------------------------------------------------
CASES_1 = [c + (layout, variant) for c in K.SOURCES_420 for layout in LAYOUTS for variant in VARIANTS]


@pytest.mark.parametrize("sw,sh,w,h,layout,variant", CASES_1, ids=["%dx%d-%dx%d-%s-%s" % (c[0], c[1], c[2], c[3], LAYOUT_IDS[c[4]], c[5]) for c in CASES_1])
def test_equals_the_reference_on_the_oracles_planes(sw, sh, w, h, layout, variant):
    parity_case(sw, sh, w, h, "420", layout, variant)


def test_the_rule_picks_both_forms_among_the_cases_above():
    for rgb in (False, True):
        picked = {documented_wide(sw, sh, "420", layout, variant) for sw, sh, w, h, layout, variant in CASES_1 if is_rgb(layout) == rgb}
        assert picked == {False, True}


# ---- 2. every chroma format ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=[LAYOUT_IDS[l] for l in LAYOUTS])
@pytest.mark.parametrize("name,sw,sh,w,h", K.FORMAT_SOURCES, ids=["%s-%dx%d-%dx%d" % c for c in K.FORMAT_SOURCES])
def test_every_chroma_format(name, sw, sh, w, h, layout):
    k = K.FORMAT_SOURCES.index((name, sw, sh, w, h)) + LAYOUTS.index(layout)
    parity_case(sw, sh, w, h, name, layout, VARIANTS[k % 3])


# ---- 3. saturated content -------------------------------------------------------------------------------------------------------------
def constant_yuv(sw, sh, value):
    return b"".join(np.full((rows, rb), value, dtype=np.uint8).tobytes() for rb, rows in IR.source_dims(sw, sh, 1, 1, PLANAR))


def steps_of_one_picture(hip, make, w, h, cfg, name="420"):
    encs = encoders(hip, w, h, name, 1, cfg)
    got = sized_steps(hip, encs, lambda k, t: make())
    hip.dsv_enc_free(C.byref(encs[0]))
    return got[0]


@pytest.mark.parametrize("sw,sh", K.CONSTANT_SOURCES, ids=["%dx%d" % c for c in K.CONSTANT_SOURCES])
@pytest.mark.parametrize("value", [255, 0], ids=["white", "black"])
def test_constant_sources_lossless(value, sw, sh):
    """A white and a black source into 16x16, lossless: 255 stays 255 and 0 stays 0 through the resampling, an RGB footprint of equal
    pixels gives what one pixel gives, and the packets are those of the constant picture."""
    hip = bind(A.load_hip())
    want = K.constant_reference(value, value)
    for layout in (PLANAR, SEMI):
        frame = constant_yuv(sw, sh, value)
        got = steps_of_one_picture(hip, lambda: (EI.yuv_source(frame, sw, sh, "420", layout, 0, "plus1"), sw, sh), 16, 16, K.LOSSLESS)
        same_packets(want, got, LAYOUT_IDS[layout])
    px = np.full((sh, sw, 4), value, dtype=np.uint8)
    px[..., 3] = 77
    for layout in (BGRA709, RGBAFULL):
        one = R.convert(px[:1, :1], layout, 0, 0)
        flat = [np.full((16, 16), one[0][0, 0], dtype=np.uint8)] + [np.full((8, 8), 128, dtype=np.uint8)] * 2
        assert one[1][0, 0] == 128 and one[2][0, 0] == 128
        assert all(np.array_equal(a, b) for a, b in zip(IR.convert_sized(px, layout, 16, 16, 1, 1), flat))
        got = steps_of_one_picture(hip, lambda: (EI.rgb_source(px, layout, 0, "tight"), sw, sh), 16, 16, K.LOSSLESS)
        same_packets(K.constant_reference(int(one[0][0, 0]), 128), got, LAYOUT_IDS[layout])


def test_checkerboard_99x51_into_66x34():
    """the checkerboard of tests/edge_cases.py at the source size, quantiser 30: planar, and the same board as grey RGB pixels"""
    hip = bind(A.load_hip())
    sw, sh, w, h = K.CHECKER
    frame = IR.packed(K.checker_planes())
    got = steps_of_one_picture(hip, lambda: (EI.yuv_source(frame, sw, sh, "420", PLANAR, 0, "plus1"), sw, sh), w, h, K.CHECKER_CFG)
    same_packets(K.checker_reference("yuv"), got, "planar")
    px = K.checker_pixels()
    got = steps_of_one_picture(hip, lambda: (EI.rgb_source(px, BGRA709, 0, "aligned"), sw, sh), w, h, K.CHECKER_CFG)
    same_packets(K.checker_reference(BGRA709), got, "bgra709")


# ---- 4. one step: plain, scaled and sized surfaces, YUV and RGB ----------------------------------------------------------------------------
def test_mixed_step():
    """Five 34x18 encoders in one call per picture: plain planar, NV12 with SCALE_HALF from 67x35, sized BGRA-709 from 51x27, sized
    planar from 35x19, and a sized RGBA entry at the encoder's own size.  Each equals its own reference stream; every counter counts
    its own kind."""
    hip = bind(A.load_hip())
    encs = encoders(hip, 34, 18, "420", len(K.MIXED), CFG)
    reset_all(hip)

    def make(k, t):
        layout, sw, sh, how = K.MIXED[k]
        return (source(sw, sh, "420", layout, "aligned", t, None, 1 if how == "half" else 0), sw, sh)

    got = sized_steps(hip, encs, make)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    assert yuv_forms(hip) == (0, NFR) and rgb_forms(hip) == (0, NFR)  # (rows of 34 bytes / 34 pixels: the plain general forms)
    assert scale_forms(hip) == (0, NFR, 0, 0)
    assert resize_forms(hip) == (0, NFR, NFR, 0)  # (35-byte rows: general; an aligned BGRA surface: wide)
    for k, (layout, sw, sh, how) in enumerate(K.MIXED):
        if how == "half":
            want = EI.scaled_reference(sw, sh, "420", 1, kind_of(layout))
        else:
            want = K.reference(sw, sh, 34, 18, "420", kind_of(layout))
        same_packets(want, got[k], "stream %d" % k)


# ---- 5. the encoder's own size: the plain calls' step --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [SEMI, RGBAFULL], ids=["nv12", "rgbafull"])
def test_own_size_gives_the_packets_and_counters_of_the_plain_calls(layout):
    hip = bind(A.load_hip())
    w, h = 34, 18
    plain = encoders(hip, w, h, "420", 1, CFG)
    encp = (C.POINTER(A.ENCODER) * 1)(C.pointer(plain[0]))
    bufs, nbufs, want = (A.BUF * 4)(), (C.c_int * 1)(), [[]]
    for t in range(NFR):
        sf = source(w, h, "420", layout, "plus1", t)
        torch.cuda.synchronize()
        assert hip.dsv2hip_enc_batch_surface(1, encp, (SURFACE * 1)(sf.c), bufs, nbufs) == 0
        take_packets(hip, bufs, nbufs, want)
    hip.dsv_enc_free(C.byref(plain[0]))
    reset_all(hip)
    got = encode_sized(hip, w, h, w, h, "420", layout, "plus1")
    same_packets(want[0], got)
    same_packets(K.reference(w, h, w, h, "420", kind_of(layout)), got)
    assert resize_forms(hip) == (0, 0, 0, 0) and scale_forms(hip) == (0, 0, 0, 0)
    assert (rgb_forms(hip), yuv_forms(hip)) == (((0, NFR), (0, 0)) if is_rgb(layout) else ((0, 0), (0, NFR)))


def test_the_one_frame_call_equals_the_batch_call():
    hip = bind(A.load_hip())
    sw, sh, w, h = 51, 27, 34, 18
    for layout in (BGRA709, SEMI):
        encs = encoders(hip, w, h, "420", 1, CFG)
        got, bufs = [[]], (A.BUF * 4)()
        for t in range(NFR):
            sf = source(sw, sh, "420", layout, "plus1", t)
            torch.cuda.synchronize()
            nb = (C.c_int * 1)(hip.dsv2hip_enc_surface_frame_sized(C.byref(encs[0]), C.byref(sf.c), sw, sh, bufs))
            take_packets(hip, bufs, nb, got)
            sf.check_untouched()
        hip.dsv_enc_free(C.byref(encs[0]))
        same_packets(K.reference(sw, sh, w, h, "420", kind_of(layout)), got[0])


# ---- 6. exact ratios: the scaled call's result ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=[LAYOUT_IDS[l] for l in LAYOUTS])
def test_twice_the_encoders_size_equals_scale_half(layout):
    """68x36 -> 34x18: the sized entry, the same entry with DSV2HIP_SCALE_HALF through the sized call, and the scaled call's reference"""
    hip = bind(A.load_hip())
    sw, sh, w, h = 68, 36, 34, 18
    reset_all(hip)
    sized = encode_sized(hip, sw, sh, w, h, "420", layout, "aligned")
    assert sum(resize_forms(hip)) == NFR and sum(scale_forms(hip)) == 0
    half = encode_sized(hip, sw, sh, w, h, "420", layout, "aligned", s=1)
    assert sum(resize_forms(hip)) == NFR and sum(scale_forms(hip)) == NFR  # (a scale value: the scaled call's entry and counters)
    want = EI.scaled_reference(sw, sh, "420", 1, kind_of(layout))
    same_packets(want, half, "SCALE_HALF through the sized call")
    same_packets(want, sized, "sized")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def set_layout(value):
    def f(c, size):
        c.layout = value
    return f


def set_size(sw, sh):
    def f(c, size):
        size[0], size[1] = sw, sh
    return f


def short_pitch(plane, row_bytes):
    def f(c, size):
        c.pitch[plane] = row_bytes - 1
    return f


def null_plane(plane):
    def f(c, size):
        c.plane[plane] = None
    return f


# (a 34x18 4:2:0 encoder and a 51x27 source: rows of 51 / 26 / 26 bytes planar, 51 / 52 NV12, 204 RGB; a size alone is spoiled
# without the surface being read: the call refuses before it looks at a byte)
REFUSALS = ([("source_8w_plus_1", PLANAR, set_size(8 * 34 + 1, 27)), ("source_w_minus_1", SEMI, set_size(33, 27)), ("source_h_minus_1", BGRA709, set_size(51, 17)),
             ("src_w_0", SEMI, set_size(0, 27)), ("src_h_0", BGRA709, set_size(51, 0)), ("src_w_negative", PLANAR, set_size(-51, 27)),
             ("src_h_negative", RGBAFULL, set_size(51, -27)),
             ("layout_0x4000", PLANAR, lambda c, size: setattr(c, "layout", c.layout | 0x4000)), ("layout_0x1010", R.RGBA, set_layout(0x1010)),
             ("planar_bt709", PLANAR, set_layout(PLANAR | R.BT709)), ("layout_2", PLANAR, set_layout(2)),
             ("half_of_another_size", SEMI, set_layout(SEMI | HALF))] +
            [("pitch_short_planar_%d" % p, PLANAR, short_pitch(p, (51, 26, 26)[p])) for p in range(3)] +
            [("pitch_short_semiplanar_%d" % p, SEMI, short_pitch(p, (51, 52)[p])) for p in range(2)] +
            [("pitch_short_rgb", BGRA709, short_pitch(0, 204))] +
            [("null_planar_%d" % p, PLANAR, null_plane(p)) for p in range(3)] + [("null_semiplanar_%d" % p, SEMI, null_plane(p)) for p in range(2)] +
            [("null_rgb", RGBAFULL, null_plane(0))])


def refused(hip, encs, cs, sizes):
    """the batch call returns -1 and leaves nbufs and the encoders' bytes alone"""
    n = len(encs)
    encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
    bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)(*[77 + k for k in range(n)])
    state = [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs]
    sws, shs = (C.c_int * n)(*[z[0] for z in sizes]), (C.c_int * n)(*[z[1] for z in sizes])
    assert hip.dsv2hip_enc_batch_surface_sized(n, encp, (SURFACE * n)(*cs), sws, shs, bufs, nbufs) == -1
    assert list(nbufs) == [77 + k for k in range(n)]
    assert [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs] == state


@pytest.mark.parametrize("what,layout,spoil", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_source_touches_nothing(what, layout, spoil):
    """Two 34x18 encoders, the second one's source spoiled: -1 (0 from the one-frame call), nbufs, the encoders' bytes and the
    counters as they were; the same encoders then give the reference's packets from frame 0 on."""
    hip = bind(A.load_hip())
    sw, sh, w, h = 51, 27, 34, 18
    encs = encoders(hip, w, h, "420", 2, CFG)
    good = [source(sw, sh, "420", PLANAR, "aligned", 0), source(sw, sh, "420", layout, "aligned", 0)]
    bad, size = copy_of(good[1].c), [sw, sh]
    spoil(bad, size)
    torch.cuda.synchronize()
    reset_all(hip)
    refused(hip, encs, [good[0].c, bad], [(sw, sh), tuple(size)])
    state = bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1])))
    assert hip.dsv2hip_enc_surface_frame_sized(C.byref(encs[1]), C.byref(bad), size[0], size[1], (A.BUF * 4)()) == 0
    assert bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1]))) == state
    assert resize_forms(hip) == (0, 0, 0, 0) and scale_forms(hip) == (0, 0, 0, 0)
    for g in good:
        g.check_untouched()
    layouts = [PLANAR, layout]
    got = sized_steps(hip, encs, lambda k, t: (source(sw, sh, "420", layouts[k], "aligned", t), sw, sh))
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    for k in range(2):
        same_packets(K.reference(sw, sh, w, h, "420", kind_of(layouts[k])), got[k], "stream %d" % k)


def test_refused_by_the_bounds_on_D():
    """No surface is read before every entry has passed, so the sources here need not exist.  Two encoders a step, the first entry a
    planar source of the encoder's own size, the second spoiled.  4099x4099 -> 4098x4098: D = 4099^2 > 2^24, refused for YUV.
    514x514 -> 512x512 (4:4:4 encoders): D = 257^2 = 66 049 > 65 535, refused for RGB; the same sizes pass as YUV in
    dsv2hip_enc_sized_dims, as 1920x1080 -> 1918x1078 does, which RGB refuses."""
    hip = bind(A.load_hip())
    one = source(51, 27, "420", PLANAR, "aligned", 0)
    torch.cuda.synchronize()
    for w, sw, name, layout in [(4098, 4099, "420", PLANAR), (512, 514, "444", BGRA709)]:
        encs = encoders(hip, w, w, name, 2, CFG)
        good, bad = copy_of(one.c), copy_of(one.c)
        bad.layout = layout
        for c in range(3):
            good.pitch[c] = bad.pitch[c] = 1 << 20
        refused(hip, encs, [good, bad], [(w, w), (sw, sw)])
        assert hip.dsv2hip_enc_surface_frame_sized(C.byref(encs[1]), C.byref(bad), sw, sw, (A.BUF * 4)()) == 0
        for e in encs:
            hip.dsv_enc_free(C.byref(e))
    one.check_untouched()
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    assert hip.dsv2hip_enc_sized_dims(514, 514, 512, 512, A.SUBSAMP_444, PLANAR, rb, rows) == 0
    assert hip.dsv2hip_enc_sized_dims(514, 514, 512, 512, A.SUBSAMP_444, BGRA709, rb, rows) == -1
    assert hip.dsv2hip_enc_sized_dims(1920, 1080, 1918, 1078, A.SUBSAMP_420, SEMI, rb, rows) == 0
    assert hip.dsv2hip_enc_sized_dims(1920, 1080, 1918, 1078, A.SUBSAMP_420, RGBAFULL, rb, rows) == -1
    assert hip.dsv2hip_enc_sized_dims(4099, 4099, 4098, 4098, A.SUBSAMP_420, PLANAR, rb, rows) == -1


def test_refused_arguments():
    hip = bind(A.load_hip())
    sw, sh, w, h = 51, 27, 34, 18
    encs = encoders(hip, w, h, "420", 1, CFG)
    sf = source(sw, sh, "420", SEMI, "aligned", 0)
    torch.cuda.synchronize()
    encp, bufs, nbufs = (C.POINTER(A.ENCODER) * 1)(C.pointer(encs[0])), (A.BUF * 4)(), (C.c_int * 1)(77)
    arr, sws, shs = (SURFACE * 1)(sf.c), (C.c_int * 1)(sw), (C.c_int * 1)(sh)
    call = hip.dsv2hip_enc_batch_surface_sized
    assert call(0, encp, arr, sws, shs, bufs, nbufs) == -1 and call(-1, encp, arr, sws, shs, bufs, nbufs) == -1
    assert call(1, None, arr, sws, shs, bufs, nbufs) == -1 and call(1, encp, None, sws, shs, bufs, nbufs) == -1
    assert call(1, encp, arr, None, shs, bufs, nbufs) == -1 and call(1, encp, arr, sws, None, bufs, nbufs) == -1  # NULL size arrays
    assert call(1, encp, arr, sws, shs, None, nbufs) == -1 and call(1, encp, arr, sws, shs, bufs, None) == -1
    assert call(1, (C.POINTER(A.ENCODER) * 1)(), arr, sws, shs, bufs, nbufs) == -1
    one = hip.dsv2hip_enc_surface_frame_sized
    assert one(None, arr, sw, sh, bufs) == 0 and one(C.byref(encs[0]), None, sw, sh, bufs) == 0 and one(C.byref(encs[0]), arr, sw, sh, None) == 0
    assert nbufs[0] == 77
    # the scaled call with s = 0 and another source size stays refused
    assert hip.dsv2hip_enc_batch_surface_scaled(1, encp, arr, sws, shs, bufs, nbufs) == -1 and nbufs[0] == 77
    got = sized_steps(hip, encs, lambda k, t: (source(sw, sh, "420", SEMI, "aligned", t), sw, sh))
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(K.reference(sw, sh, w, h, "420", "yuv"), got[0])


def test_refused_on_a_uyvy_encoder():
    """An encoder whose packed input is interleaved UYVY takes no sized source; with the switch off again it encodes NV16 from 51x27
    from frame 0."""
    hip = bind(A.load_hip())
    sw, sh, w, h, name = 51, 27, 34, 18, "422"
    encs = encoders(hip, w, h, name, 1, CFG)
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 1) == 0
    sf = source(sw, sh, name, SEMI, "aligned", 0)
    torch.cuda.synchronize()
    refused(hip, encs, [sf.c], [(sw, sh)])
    assert hip.dsv2hip_enc_surface_frame_sized(C.byref(encs[0]), C.byref(sf.c), sw, sh, (A.BUF * 4)()) == 0
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 0) == 0
    got = sized_steps(hip, encs, lambda k, t: (source(sw, sh, name, SEMI, "aligned", t), sw, sh))
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(K.reference(sw, sh, w, h, name, "yuv"), got[0])


# ---- 8. the ladder identity ----------------------------------------------------------------------------------------------------------------
def test_full_size_decode_into_the_sized_call_equals_sized_decode_into_the_plain_call():
    """A 64x48 4:2:0 stream decoded at FULL size into a pitched NV12 device surface that goes to dsv2hip_enc_surface_frame_sized of a
    42x30 encoder, against the same stream decoded at 42x30 into a PLANAR surface (dsv2hip_dec_surface_frame_sized) that goes to the
    plain call, and against the reference encoder on the host's resampling of the decoded planes."""
    ref, hip = A.load_ref(), bind(A.load_hip())
    w, h, ow, oh, cfg = 64, 48, 42, 30, dict(qp=50, gop=48)
    packets = stream(w, h, "420", 4, 4)
    full = [pl for _, _, pl in planar_oracle(packets) if pl is not None]
    small = [AR.resize_picture(pl[0], pl[1], pl[2], ow, oh, 1, 1) for pl in full]
    assert len(small) == 4 and [p.shape for p in small[0]] == [(30, 42), (15, 21), (15, 21)]
    want = encode_stream(ref, [IR.packed(pic) for pic in small], ow, oh, A.SUBSAMP_420, eos=False, **cfg)[0]
    packet_bound_holds(want, ow, oh, A.SUBSAMP_420)

    def run(sized_decode):
        enc, dec = A.ENCODER(), A.DECODER()
        configure_encoder(hip, enc, A.mk_meta(ow, oh, A.SUBSAMP_420), **cfg)
        if sized_decode:
            sf = OutSurf([(ow, oh), (21, 15), (21, 15)], PLANAR, aligned_out)
        else:
            sf = OutSurf([(64, 48), (64, 24), (0, 0)], SEMI, aligned_out)
        sf.arm()
        torch.cuda.synchronize()
        got, seen = [], 0
        for pk in packets:
            buf, fn = A.BUF(), C.c_uint32(0)
            mk_buf(hip, buf, pk)
            had_meta = dec.got_metadata
            if sized_decode:
                code = hip.dsv2hip_dec_surface_frame_sized(C.byref(dec), C.byref(buf), C.byref(sf.c), ow, oh, C.byref(fn))
            else:
                code = hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(buf), C.byref(sf.c), C.byref(fn))
            if code == A.DEC_EOS:
                break
            if code != A.DEC_OK or not had_meta:
                continue
            src = SURFACE()
            for c in range(3):
                src.plane[c], src.pitch[c] = sf.c.plane[c], sf.c.pitch[c]
            src.layout = PLANAR if sized_decode else SEMI
            obufs = (A.BUF * 4)()
            if sized_decode:
                n = hip.dsv2hip_enc_surface_frame(C.byref(enc), C.byref(src), obufs)
            else:
                n = hip.dsv2hip_enc_surface_frame_sized(C.byref(enc), C.byref(src), 64, 48, obufs)
            assert 1 <= n <= 4
            for q in range(n):
                got.append(bytes(C.string_at(obufs[q].data, obufs[q].len)))
                hip.dsv_buf_free(C.byref(obufs[q]))
            seen += 1
        hip.dsv_enc_free(C.byref(enc))
        hip.dsv_dec_free(C.byref(dec))
        assert seen == 4
        return got

    same_packets(want, run(True), "decode at 42x30, plain encode")
    same_packets(want, run(False), "decode at full size, sized encode")


# ---- 9. dsv2hip_enc_sized_dims ------------------------------------------------------------------------------------------------------------
def sized_dims(hip, sw, sh, w, h, subsamp, layout):
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    r = hip.dsv2hip_enc_sized_dims(sw, sh, w, h, subsamp, layout, rb, rows)
    return r, list(zip(rb, rows))


def test_sized_dims_are_the_oracles_shapes_and_refuse_what_the_calls_refuse():
    hip = bind(A.load_hip())
    for name, sw, sh, w, h in [("420",) + c for c in K.SOURCES_420] + K.FORMAT_SOURCES:
        code, hs, vs = FMT[name]
        for layout in LAYOUTS:
            dims = IR.source_dims(sw, sh, hs, vs, "rgb" if is_rgb(layout) else layout)
            r, got = sized_dims(hip, sw, sh, w, h, code, layout)
            assert r == 0 and got == dims + [(0, 0)] * (3 - len(dims))
            assert IR.allowed(sw, sh, w, h, hs, vs, is_rgb(layout))
            planes = K.oracle_pictures(sw, sh, w, h, name, kind_of(layout))[0]
            assert len(planes) == sum(rb * rows for rb, rows in IR.source_dims(w, h, hs, vs, PLANAR))
    for sw, sh, w, h in [(273, 27, 34, 18), (33, 27, 34, 18), (51, 145, 34, 18), (51, 17, 34, 18), (0, 27, 34, 18), (51, -1, 34, 18), (51, 27, 0, 18),
                         (272, 144, 34, 18), (34, 18, 34, 18), (514, 514, 512, 512)]:
        for layout in LAYOUTS:
            assert (sized_dims(hip, sw, sh, w, h, A.SUBSAMP_420, layout)[0] == 0) == IR.allowed(sw, sh, w, h, 1, 1, is_rgb(layout)), (sw, sh, w, h, layout)
    for layout in (0x4000, 0x1010, 0x1012, PLANAR | R.BT709, 0x2):
        assert sized_dims(hip, 51, 27, 34, 18, A.SUBSAMP_420, layout)[0] == -1
    # a scale value: the scaled call's rule
    assert sized_dims(hip, 67, 35, 34, 18, A.SUBSAMP_420, SEMI | HALF)[0] == 0 and sized_dims(hip, 51, 27, 34, 18, A.SUBSAMP_420, SEMI | HALF)[0] == -1
