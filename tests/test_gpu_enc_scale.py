"""Half, quarter and eighth-size ingest (dsv2hip_enc_batch_surface_scaled, dsv2hip_enc_surface_frame_scaled): an encoder of
ceil(src_w / n) x ceil(src_h / n) reads a planar, NV12, BGRA or RGBA device surface of src_w x src_h, and its packets are the
reference encoder's on the planes that include/dsv2_hip.h defines (tests/ingest_scale.py, numpy) -- both forms of both kernels,
every shift, the five chroma formats, sources whose last footprints lie half outside them, more than one workgroup of rows,
saturated content, scaled and plain surfaces mixed in one step; the surface is never written, a refused call touches nothing,
and a picture decoded at full size and encoded through the scaled call gives the packets of the same picture decoded at that
scale and encoded through the plain call.

Every reference stream is checked for the two conditions of a case before it is compared with: its packets stay inside the bound
within which the reference is defined (edge_cases.packet_bound_holds), and I and P pictures both occur."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import box_reduce as B
import dsvabi as A
import ingest_scale as S
import rgb_csc as R
from codec_run import configure_encoder, encode_stream
from edge_cases import content_planes, packet_bound_holds
from codec_run import FMT
from dec_out import OutSurf, aligned as aligned_out, planar_oracle, stream
from enc_in import (LADDER_CFG, LADDER_LOSSLESS, LADDER_NFR, LADDER_SEED, content, copy_of, encode_steps, encoders, is_rgb, kind_of, offset_of, pitch_of,
                    ref_packets, rgb_content, rgb_source, same_packets, scaled_pictures as oracle_pictures, scaled_reference as reference, take_packets,
                    yuv_source)
from hipabi import (PLANAR, SEMI, SURFACE, bind, enc_rgb_forms as rgb_forms, enc_scale_forms as scale_forms, enc_yuv_forms as yuv_forms, mk_buf,
                    reset_enc_forms as reset_all)

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

CFG, LOSSLESS, NFR, SEED = LADDER_CFG, LADDER_LOSSLESS, LADDER_NFR, LADDER_SEED
SCALE = S.SCALE
BGRA709, RGBAFULL = R.BGRA | R.BT709, R.RGBA | R.FULL
LAYOUTS = [PLANAR, SEMI, BGRA709, RGBAFULL]
LAYOUT_IDS = {PLANAR: "planar", SEMI: "semiplanar", BGRA709: "bgra709", RGBAFULL: "rgbafull"}
VARIANTS = ["tight", "plus1", "aligned"]


# ---- sources ----------------------------------------------------------------------------------------------------------------------
scaled_steps = functools.partial(encode_steps, nfr=NFR, call="dsv2hip_enc_batch_surface_scaled")


def source(sw, sh, name, layout, s, variant, t, offset=None):
    if is_rgb(layout):
        return rgb_source(rgb_content(sw, sh, NFR, SEED)[t], layout, s, variant, offset)
    return yuv_source(content(sw, sh, name, NFR, SEED)[t], sw, sh, name, layout, s, variant, offset)


def documented_wide(sw, sh, name, layout, variant, offset=None):
    """include/dsv2_hip.h at dsv2hip_enc_scale_stats: YUV -- every source plane's pointer, pitch and SOURCE row bytes are multiples of
    16; RGB -- pointer and pitch multiples of 16, src_w of 4.  (The tensors start 16-byte aligned and the guard in front is 64 bytes.)"""
    _, hs, vs = FMT[name]
    off = offset_of(variant) if offset is None else offset
    if is_rgb(layout):
        return off % 16 == 0 and pitch_of(4 * sw, variant) % 16 == 0 and sw % 4 == 0
    return all(off % 16 == 0 and pitch_of(rb, variant) % 16 == 0 and rb % 16 == 0 for rb, _ in S.source_dims(sw, sh, hs, vs, layout))


def encode_scaled(hip, sw, sh, name, layout, s, variant, offset=None, cfg=CFG):
    """one encoder of the reduced geometry over the NFR source pictures; frees the encoder"""
    encs = encoders(hip, S.up(sw, s), S.up(sh, s), name, 1, cfg)
    got = scaled_steps(hip, encs, lambda k, t: (source(sw, sh, name, layout, s, variant, t, offset), sw, sh))
    hip.dsv_enc_free(C.byref(encs[0]))
    return got[0]


def parity_case(sw, sh, name, layout, s, variant, offset=None):
    """the packets are the reference's, and the step ran in the form the documented rule names"""
    hip = bind(A.load_hip())
    reset_all(hip)
    want = reference(sw, sh, name, s, kind_of(layout))
    got = encode_scaled(hip, sw, sh, name, layout, s, variant, offset)
    same_packets(want, got)
    wide = documented_wide(sw, sh, name, layout, variant, offset)
    at = (2 if is_rgb(layout) else 0) + (0 if wide else 1)
    assert scale_forms(hip) == tuple(NFR if i == at else 0 for i in range(4))
    assert rgb_forms(hip) == (0, 0) and yuv_forms(hip) == (0, 0)  # (the plain surfaces' counters count plain surfaces only)


# ---- 1. every 4:2:0 source x layout x pitch / alignment ------------------------------------------------------------------------------
SOURCES_420 = [(31, 31, 1), (32, 32, 1), (61, 62, 2), (121, 125, 3),  # -> 16x16
               (137, 121, 3),                                          # -> 18x16
               (67, 35, 1), (133, 69, 2),                              # -> 34x18
               (131, 67, 1), (263, 135, 2), (521, 265, 3)]             # -> 66x34
CASES_1 = [(sw, sh, s, layout, variant) for sw, sh, s in SOURCES_420 for layout in LAYOUTS for variant in VARIANTS]


@pytest.mark.parametrize("sw,sh,s,layout,variant", CASES_1, ids=["%dx%d-s%d-%s-%s" % (c[0], c[1], c[2], LAYOUT_IDS[c[3]], c[4]) for c in CASES_1])
def test_equals_the_reference_on_the_oracles_planes(sw, sh, s, layout, variant):
    assert (S.up(sw, s), S.up(sh, s)) in ((16, 16), (18, 16), (34, 18), (66, 34))
    parity_case(sw, sh, "420", layout, s, variant)


def test_the_rule_picks_both_forms_among_the_cases_above():
    for rgb in (False, True):
        picked = {documented_wide(sw, sh, "420", layout, variant) for sw, sh, s, layout, variant in CASES_1 if is_rgb(layout) == rgb}
        assert picked == {False, True}


# ---- 2. the wide form at every shift; a pointer that is a multiple of 4 only --------------------------------------------------------
SOURCES_64x48 = [(128, 96, 1), (256, 192, 2), (512, 384, 3)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=[LAYOUT_IDS[l] for l in LAYOUTS])
@pytest.mark.parametrize("sw,sh,s", SOURCES_64x48, ids=["s%d" % c[2] for c in SOURCES_64x48])
@pytest.mark.parametrize("offset", [0, 4], ids=["wide", "pointer_multiple_of_4"])
def test_aligned_surfaces_into_64x48(offset, sw, sh, s, layout):
    assert documented_wide(sw, sh, "420", layout, "aligned", offset) == (offset == 0)
    parity_case(sw, sh, "420", layout, s, "aligned", offset)


# ---- 3. more than one workgroup of rows, partial footprints both ways -----------------------------------------------------------------
@pytest.mark.parametrize("layout,variant", [(PLANAR, "plus1"), (BGRA709, "aligned")], ids=["planar", "bgra709"])
def test_tall_source_takes_more_than_one_workgroup(layout, variant):
    """259x515 -> 130x258: 65 workgroups of four output rows, the last column and the last row half outside the source"""
    parity_case(259, 515, "420", layout, 1, variant)


# ---- 4. every chroma format --------------------------------------------------------------------------------------------------------
FORMAT_SOURCES = ([(name, 67, 35, 1) for name in ("444", "422")] + [(name, 269, 141, 3) for name in ("444", "422")] +  # -> 34x18
                  [(name, 75, 43, 1) for name in ("411", "410")] + [(name, 297, 169, 3) for name in ("411", "410")])   # -> 38x22


@pytest.mark.parametrize("layout", LAYOUTS, ids=[LAYOUT_IDS[l] for l in LAYOUTS])
@pytest.mark.parametrize("name,sw,sh,s", FORMAT_SOURCES, ids=["%s-%dx%d-s%d" % c for c in FORMAT_SOURCES])
def test_every_chroma_format(name, sw, sh, s, layout):
    k = FORMAT_SOURCES.index((name, sw, sh, s)) + LAYOUTS.index(layout)
    parity_case(sw, sh, name, layout, s, VARIANTS[k % 3])


# ---- 5. saturated content ------------------------------------------------------------------------------------------------------------
def constant_yuv(sw, sh, value):
    return b"".join(np.full((rows, rb), value, dtype=np.uint8).tobytes() for rb, rows in S.source_dims(sw, sh, 1, 1, PLANAR))


def steps_of_one_picture(hip, make, w, h, cfg, name="420"):
    encs = encoders(hip, w, h, name, 1, cfg)
    got = scaled_steps(hip, encs, lambda k, t: make())
    hip.dsv_enc_free(C.byref(encs[0]))
    return got[0]


@pytest.mark.parametrize("sw,sh,s", SOURCES_420[:1] + SOURCES_420[2:4], ids=["s1", "s2", "s3"])
@pytest.mark.parametrize("value", [255, 0], ids=["white", "black"])
def test_constant_sources_lossless(value, sw, sh, s):
    """A white and a black source into 16x16, lossless: 255 stays 255 and 0 stays 0 through the reduction, an RGB footprint of equal
    pixels gives what one pixel gives, and the packets are those of the constant picture."""
    hip = bind(A.load_hip())
    assert (S.up(sw, s), S.up(sh, s)) == (16, 16)
    flat = [np.full((16, 16), value, dtype=np.uint8)] + [np.full((8, 8), value, dtype=np.uint8)] * 2
    want = ref_packets([S.packed(flat)] * NFR, 16, 16, "420", LOSSLESS)
    for layout in (PLANAR, SEMI):
        frame = constant_yuv(sw, sh, value)
        got = steps_of_one_picture(hip, lambda: (yuv_source(frame, sw, sh, "420", layout, s, "plus1"), sw, sh), 16, 16, LOSSLESS)
        same_packets(want, got, LAYOUT_IDS[layout])
    px = np.full((sh, sw, 4), value, dtype=np.uint8)
    px[..., 3] = 77
    for layout in (BGRA709, RGBAFULL):
        one = R.convert(px[:1, :1], layout, 0, 0)
        flat = [np.full((16, 16), one[0][0, 0], dtype=np.uint8)] + [np.full((8, 8), 128, dtype=np.uint8)] * 2
        assert one[1][0, 0] == 128 and one[2][0, 0] == 128
        assert all(np.array_equal(a, b) for a, b in zip(S.convert_scaled(px, layout, 1, 1, s), flat))
        want_rgb = ref_packets([S.packed(flat)] * NFR, 16, 16, "420", LOSSLESS)
        got = steps_of_one_picture(hip, lambda: (rgb_source(px, layout, s, "tight"), sw, sh), 16, 16, LOSSLESS)
        same_packets(want_rgb, got, LAYOUT_IDS[layout])


def test_checkerboard_131x67_into_66x34():
    """the checkerboard of tests/edge_cases.py at the source size, quantiser 30: planar, and the same board as grey RGB pixels"""
    hip = bind(A.load_hip())
    sw, sh, s, cfg = 131, 67, 1, dict(qp=30, gop=4)
    planes = content_planes("checker", A.SUBSAMP_420, sw, sh)
    frame = S.packed(planes)
    want = ref_packets([S.packed(S.reduce_yuv(list(planes), s))] * NFR, 66, 34, "420", cfg)
    got = steps_of_one_picture(hip, lambda: (yuv_source(frame, sw, sh, "420", PLANAR, s, "plus1"), sw, sh), 66, 34, cfg)
    same_packets(want, got, "planar")
    px = np.repeat(planes[0][:, :, None], 4, axis=2).copy()
    want = ref_packets([S.packed(S.convert_scaled(px, BGRA709, 1, 1, s))] * NFR, 66, 34, "420", cfg)
    got = steps_of_one_picture(hip, lambda: (rgb_source(px, BGRA709, s, "aligned"), sw, sh), 66, 34, cfg)
    same_packets(want, got, "bgra709")


# ---- 6. one step: scaled and plain surfaces, YUV and RGB ---------------------------------------------------------------------------------
MIXED = [(PLANAR, 34, 18, 0), (SEMI, 67, 35, 1), (BGRA709, 133, 69, 2), (RGBAFULL, 269, 141, 3), (R.RGBA, 34, 18, 0)]


def test_mixed_step():
    """Five 34x18 encoders in one call per picture: plain planar, NV12 at half size from 67x35, BGRA-709 at a quarter from 133x69,
    RGBA-full at an eighth from 269x141, plain RGBA.  Each equals its own reference stream; the plain surfaces' counters count the
    plain ones, the scaled counters the scaled ones."""
    hip = bind(A.load_hip())
    encs = encoders(hip, 34, 18, "420", len(MIXED), CFG)
    reset_all(hip)
    got = scaled_steps(hip, encs, lambda k, t: (source(MIXED[k][1], MIXED[k][2], "420", MIXED[k][0], MIXED[k][3], "aligned", t),) + MIXED[k][1:3])
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    assert yuv_forms(hip) == (0, NFR) and rgb_forms(hip) == (0, NFR)  # (rows of 34 bytes / 34 pixels: the general forms)
    assert scale_forms(hip) == (0, NFR, 0, NFR)
    for k, (layout, sw, sh, s) in enumerate(MIXED):
        same_packets(reference(sw, sh, "420", s, kind_of(layout)), got[k], "stream %d" % k)


# ---- 7. no scale value: the plain calls' step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [SEMI, RGBAFULL], ids=["nv12", "rgbafull"])
def test_shift_0_gives_the_packets_of_the_plain_calls(layout):
    hip = bind(A.load_hip())
    w, h = 34, 18
    plain = encoders(hip, w, h, "420", 1, CFG)
    encp = (C.POINTER(A.ENCODER) * 1)(C.pointer(plain[0]))
    bufs, nbufs, want = (A.BUF * 4)(), (C.c_int * 1)(), [[]]
    for t in range(NFR):
        sf = source(w, h, "420", layout, 0, "plus1", t)
        torch.cuda.synchronize()
        assert hip.dsv2hip_enc_batch_surface(1, encp, (SURFACE * 1)(sf.c), bufs, nbufs) == 0
        take_packets(hip, bufs, nbufs, want)
    hip.dsv_enc_free(C.byref(plain[0]))
    reset_all(hip)
    got = encode_scaled(hip, w, h, "420", layout, 0, "plus1")
    same_packets(want[0], got)
    same_packets(reference(w, h, "420", 0, kind_of(layout)), got)
    assert scale_forms(hip) == (0, 0, 0, 0)
    assert (rgb_forms(hip), yuv_forms(hip)) == (((0, NFR), (0, 0)) if is_rgb(layout) else ((0, 0), (0, NFR)))
    # ... and a source size that is not the encoder's is refused there too
    encs = encoders(hip, w, h, "420", 1, CFG)
    sf = source(w, h, "420", layout, 0, "aligned", 0)
    torch.cuda.synchronize()
    assert hip.dsv2hip_enc_surface_frame_scaled(C.byref(encs[0]), C.byref(sf.c), w - 1, h, (A.BUF * 4)()) == 0
    hip.dsv_enc_free(C.byref(encs[0]))


def test_the_one_frame_call_equals_the_batch_call():
    hip = bind(A.load_hip())
    sw, sh, s = 133, 69, 2
    encs = encoders(hip, 34, 18, "420", 1, CFG)
    got, bufs = [[]], (A.BUF * 4)()
    for t in range(NFR):
        sf = source(sw, sh, "420", BGRA709, s, "plus1", t)
        torch.cuda.synchronize()
        nb = (C.c_int * 1)(hip.dsv2hip_enc_surface_frame_scaled(C.byref(encs[0]), C.byref(sf.c), sw, sh, bufs))
        take_packets(hip, bufs, nb, got)
        sf.check_untouched()
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(reference(sw, sh, "420", s, BGRA709), got[0])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
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


# (a 34x18 4:2:0 encoder and a 67x35 source at half size: rows of 67 / 34 / 34 bytes planar, 67 / 68 NV12, 268 RGB)
REFUSALS = ([("layout_0x4000", PLANAR, lambda c, size: setattr(c, "layout", c.layout | 0x4000)), ("layout_0x1010", R.RGBA, set_layout(0x1010)),
             ("planar_half_bt709", PLANAR, set_layout(PLANAR | SCALE[1] | R.BT709)), ("source_69x35", PLANAR, set_size(69, 35)),
             ("src_w_0", SEMI, set_size(0, 35))] +
            [("pitch_short_planar_%d" % p, PLANAR, short_pitch(p, (67, 34, 34)[p])) for p in range(3)] +
            [("pitch_short_semiplanar_%d" % p, SEMI, short_pitch(p, (67, 68)[p])) for p in range(2)] +
            [("pitch_short_rgb", BGRA709, short_pitch(0, 268))] +
            [("null_planar_%d" % p, PLANAR, null_plane(p)) for p in range(3)] + [("null_semiplanar_%d" % p, SEMI, null_plane(p)) for p in range(2)] +
            [("null_rgb", RGBAFULL, null_plane(0))])


def refused(hip, encs, cs, sizes):
    """the batch call returns -1 and leaves nbufs and the encoders' bytes alone"""
    n = len(encs)
    encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
    bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)(*[77 + k for k in range(n)])
    state = [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs]
    sws, shs = (C.c_int * n)(*[z[0] for z in sizes]), (C.c_int * n)(*[z[1] for z in sizes])
    assert hip.dsv2hip_enc_batch_surface_scaled(n, encp, (SURFACE * n)(*cs), sws, shs, bufs, nbufs) == -1
    assert list(nbufs) == [77 + k for k in range(n)]
    assert [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs] == state


@pytest.mark.parametrize("what,layout,spoil", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_source_touches_nothing(what, layout, spoil):
    """Two 34x18 encoders, the second one's source spoiled: -1 (0 from the one-frame call), nbufs and the encoders' bytes as they
    were; the same encoders then give the reference's packets from frame 0 on."""
    hip = bind(A.load_hip())
    sw, sh, s = 67, 35, 1
    encs = encoders(hip, 34, 18, "420", 2, CFG)
    good = [source(sw, sh, "420", PLANAR, s, "aligned", 0), source(sw, sh, "420", layout, s, "aligned", 0)]
    bad, size = copy_of(good[1].c), [sw, sh]
    spoil(bad, size)
    torch.cuda.synchronize()
    refused(hip, encs, [good[0].c, bad], [(sw, sh), tuple(size)])
    state = bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1])))
    assert hip.dsv2hip_enc_surface_frame_scaled(C.byref(encs[1]), C.byref(bad), size[0], size[1], (A.BUF * 4)()) == 0
    assert bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1]))) == state
    layouts = [PLANAR, layout]
    got = scaled_steps(hip, encs, lambda k, t: (source(sw, sh, "420", layouts[k], s, "aligned", t), sw, sh))
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    for k in range(2):
        same_packets(reference(sw, sh, "420", s, kind_of(layouts[k])), got[k], "stream %d" % k)


def test_refused_arguments():
    hip = bind(A.load_hip())
    sw, sh, s = 67, 35, 1
    encs = encoders(hip, 34, 18, "420", 1, CFG)
    sf = source(sw, sh, "420", SEMI, s, "aligned", 0)
    torch.cuda.synchronize()
    encp, bufs, nbufs = (C.POINTER(A.ENCODER) * 1)(C.pointer(encs[0])), (A.BUF * 4)(), (C.c_int * 1)(77)
    arr, sws, shs = (SURFACE * 1)(sf.c), (C.c_int * 1)(sw), (C.c_int * 1)(sh)
    call = hip.dsv2hip_enc_batch_surface_scaled
    assert call(0, encp, arr, sws, shs, bufs, nbufs) == -1 and call(-1, encp, arr, sws, shs, bufs, nbufs) == -1
    assert call(1, None, arr, sws, shs, bufs, nbufs) == -1 and call(1, encp, None, sws, shs, bufs, nbufs) == -1
    assert call(1, encp, arr, None, shs, bufs, nbufs) == -1 and call(1, encp, arr, sws, None, bufs, nbufs) == -1
    assert call(1, encp, arr, sws, shs, None, nbufs) == -1 and call(1, encp, arr, sws, shs, bufs, None) == -1
    assert call(1, (C.POINTER(A.ENCODER) * 1)(), arr, sws, shs, bufs, nbufs) == -1
    one = hip.dsv2hip_enc_surface_frame_scaled
    assert one(None, arr, sw, sh, bufs) == 0 and one(C.byref(encs[0]), None, sw, sh, bufs) == 0 and one(C.byref(encs[0]), arr, sw, sh, None) == 0
    assert nbufs[0] == 77
    got = scaled_steps(hip, encs, lambda k, t: (source(sw, sh, "420", SEMI, s, "aligned", t), sw, sh))
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(reference(sw, sh, "420", s, "yuv"), got[0])


def test_refused_on_a_uyvy_encoder():
    """An encoder whose packed input is interleaved UYVY takes no scaled source; with the switch off again it encodes NV16 at half
    size from frame 0."""
    hip = bind(A.load_hip())
    sw, sh, s, name = 67, 35, 1, "422"
    encs = encoders(hip, 34, 18, name, 1, CFG)
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 1) == 0
    sf = source(sw, sh, name, SEMI, s, "aligned", 0)
    torch.cuda.synchronize()
    refused(hip, encs, [sf.c], [(sw, sh)])
    assert hip.dsv2hip_enc_surface_frame_scaled(C.byref(encs[0]), C.byref(sf.c), sw, sh, (A.BUF * 4)()) == 0
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 0) == 0
    got = scaled_steps(hip, encs, lambda k, t: (source(sw, sh, name, SEMI, s, "aligned", t), sw, sh))
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(reference(sw, sh, name, s, "yuv"), got[0])


def test_refused_with_an_encoder_of_another_geometry():
    """34x18 from 67x35 and 16x16 from 31x31 in one call: -1; each then encodes its source on its own from frame 0."""
    hip = bind(A.load_hip())
    geo = [(67, 35), (31, 31)]
    encs = [encoders(hip, S.up(sw, 1), S.up(sh, 1), "420", 1, CFG)[0] for sw, sh in geo]
    first = [source(sw, sh, "420", BGRA709, 1, "aligned", 0) for sw, sh in geo]
    torch.cuda.synchronize()
    refused(hip, encs, [sf.c for sf in first], geo)
    for k, (sw, sh) in enumerate(geo):
        got = scaled_steps(hip, [encs[k]], lambda _, t: (source(sw, sh, "420", BGRA709, 1, "aligned", t), sw, sh))
        hip.dsv_enc_free(C.byref(encs[k]))
        same_packets(reference(sw, sh, "420", 1, BGRA709), got[0], "%dx%d" % (sw, sh))


# ---- 10. the ladder identity ----------------------------------------------------------------------------------------------------------------
def test_full_size_decode_into_the_scaled_call_equals_half_size_decode_into_the_plain_call():
    """A 64x48 4:2:0 stream decoded at FULL size into a pitched NV12 device surface that goes to dsv2hip_enc_surface_frame_scaled of a
    32x24 encoder at half size: the packets of test_gpu_dec_scale.test_half_size_nv12_goes_straight_into_an_encoder_of_the_reduced_
    geometry (decode at half size, plain encode) and of the reference encoder on the host copy of the reduced planes."""
    ref, hip = A.load_ref(), bind(A.load_hip())
    w, h, cfg = 64, 48, dict(qp=50, gop=48)
    packets = stream(w, h, "420", 4, 4)
    full = [pl for _, _, pl in planar_oracle(packets) if pl is not None]
    reduced = [B.reduce_picture(pl[0], pl[1], pl[2], 1) for pl in full]
    assert len(reduced) == 4 and [p.shape for p in reduced[0]] == [(24, 32), (12, 16), (12, 16)]
    want = encode_stream(ref, [S.packed(pic) for pic in reduced], 32, 24, A.SUBSAMP_420, eos=False, **cfg)[0]
    packet_bound_holds(want, 32, 24, A.SUBSAMP_420)

    def run(decode_layout, encode):
        """decode every packet into one NV12 surface of decode_layout, hand each delivered picture to encode(enc, surface, bufs)"""
        enc, dec = A.ENCODER(), A.DECODER()
        configure_encoder(hip, enc, A.mk_meta(32, 24, A.SUBSAMP_420), **cfg)
        half = bool(decode_layout & SCALE[1])
        sf = OutSurf([(32, 24), (32, 12), (0, 0)] if half else [(64, 48), (64, 24), (0, 0)], decode_layout, aligned_out)
        sf.arm()
        torch.cuda.synchronize()
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
            src = SURFACE()
            for c in range(2):
                src.plane[c], src.pitch[c] = sf.c.plane[c], sf.c.pitch[c]
            obufs = (A.BUF * 4)()
            n = encode(enc, src, obufs)
            assert 1 <= n <= 4
            for q in range(n):
                got.append(bytes(C.string_at(obufs[q].data, obufs[q].len)))
                hip.dsv_buf_free(C.byref(obufs[q]))
            y, uv = sf.planes()  # (and the encoder wrote nothing into the surface)
            pic = reduced[seen] if half else full[seen]
            assert np.array_equal(y, pic[0]) and np.array_equal(uv, B.interleave(pic[1], pic[2]))
            seen += 1
        hip.dsv_enc_free(C.byref(enc))
        hip.dsv_dec_free(C.byref(dec))
        assert seen == 4
        return got

    def plain(enc, src, obufs):
        src.layout = SEMI
        return hip.dsv2hip_enc_surface_frame(C.byref(enc), C.byref(src), obufs)

    def scaled(enc, src, obufs):
        src.layout = SEMI | SCALE[1]
        return hip.dsv2hip_enc_surface_frame_scaled(C.byref(enc), C.byref(src), 64, 48, obufs)

    existing = run(SEMI | SCALE[1], plain)
    ladder = run(SEMI, scaled)
    same_packets(want, existing, "decode at half size, plain encode")
    same_packets(want, ladder, "decode at full size, scaled encode")


# ---- 11. dsv2hip_enc_scaled_dims ----------------------------------------------------------------------------------------------------------
def scaled_dims(hip, sw, sh, subsamp, layout):
    ew, eh, rb, rows = C.c_int(-7), C.c_int(-7), (C.c_size_t * 3)(), (C.c_int * 3)()
    r = hip.dsv2hip_enc_scaled_dims(sw, sh, subsamp, layout, C.byref(ew), C.byref(eh), rb, rows)
    return r, (ew.value, eh.value), list(zip(rb, rows))


def test_scaled_dims_are_the_oracles_shapes_and_refuse_what_the_calls_refuse():
    hip = bind(A.load_hip())
    for name, sw, sh, s in [("420", c[0], c[1], c[2]) for c in SOURCES_420] + FORMAT_SOURCES:
        code, hs, vs = FMT[name]
        for layout in LAYOUTS:
            kind = "rgb" if is_rgb(layout) else layout
            dims = S.source_dims(sw, sh, hs, vs, kind)
            r, enc, got = scaled_dims(hip, sw, sh, code, layout | SCALE[s])
            assert r == 0 and got == dims + [(0, 0)] * (3 - len(dims))
            planes = oracle_pictures(sw, sh, name, s, kind_of(layout))[0]
            assert enc == (S.up(sw, s), S.up(sh, s)) and len(planes) == sum(rb * rows for rb, rows in S.source_dims(enc[0], enc[1], hs, vs, PLANAR))
    for layout in (0x4000, 0x1010, 0x1012, PLANAR | SCALE[1] | R.BT709, SEMI | SCALE[2] | R.FULL, 0x2):
        assert scaled_dims(hip, 67, 35, A.SUBSAMP_420, layout)[0] == -1
    assert scaled_dims(hip, 0, 35, A.SUBSAMP_420, SCALE[1])[0] == -1 and scaled_dims(hip, 67, -1, A.SUBSAMP_420, SCALE[1])[0] == -1
