"""Packed four-byte RGB device surfaces (DSV2HIP_SURFACE_BGRA / _RGBA, or-ed with DSV2HIP_CSC_*) as encoder input: the packets
are the reference encoder's on the planar picture that the conversion of include/dsv2_hip.h defines (tests/rgb_csc.py, numpy) --
both forms of k_ingest_rgb, both byte orders, the four presets, the five chroma formats, the smallest pictures and footprints
half outside them (lossless, so every LSB of the conversion reaches the packets), saturated colours, rows of several passes, RGB
and YUV surfaces mixed in one step; alpha and padding are never pixels, the surface is never written, a refused call touches
nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsvabi as A
import rgb_csc as R
from codec_run import FMT
from edge_cases import stream_inverse_is_undefined
from enc_in import (CFG, CIF_NV12, CIF_PLANAR, CSC_IDS, LOSSLESS, RgbSurface, Surface, content, copy_of, encode_steps, encoders, oracle_frames, packed_batch, planes_equal_oracle,
                    reference, refused, rgb_content, rgb_ref_packets as ref_packets, rgb_reference, same_packets, saturated_pictures)
from hipabi import PLANAR, bind, enc_rgb_forms as rgb_forms, enc_yuv_forms as yuv_forms, reset_enc_forms as reset_forms

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

ORDER = {"bgra": R.BGRA, "rgba": R.RGBA}


def encode_rgb(hip, pictures, layout, name, cfg=CFG, **surface):
    """one encoder over `pictures`, each in an RgbSurface(**surface); frees the encoder"""
    h, w = pictures[0].shape[:2]
    encs = encoders(hip, w, h, name, 1, cfg)
    got = encode_steps(hip, encs, lambda s, t: RgbSurface(pictures[t], layout, **surface), len(pictures))
    hip.dsv_enc_free(C.byref(encs[0]))
    return got[0]


def odd_pitch(w):
    return (4 * w + 3) | 1


def aligned_pitch(w):
    return ((4 * w + 15) & ~15) + 16


# ---- 1. wide form -------------------------------------------------------------------------------------------------------
def test_wide_form_equals_reference():
    """352x288 4:2:0 BGRA, pitch 1536, aligned: the 16-byte form; the YUV surface counts do not move."""
    hip = bind(A.load_hip())
    reset_forms(hip)
    got = encode_rgb(hip, rgb_content(352, 288, 3, 5), R.BGRA, "420", pitch=1536)
    same_packets(rgb_reference(352, 288, "420", 3, 5, R.BGRA), got)
    assert rgb_forms(hip) == (3, 0)
    assert yuv_forms(hip) == (0, 0)


# ---- 2. general form, every format ------------------------------------------------------------------------------------------
GENERAL = [(354, 290, "420")] + [(176, 144, name) for name in sorted(FMT)]


@pytest.mark.parametrize("order", sorted(ORDER))
@pytest.mark.parametrize("k,w,h,name", [(k,) + g for k, g in enumerate(GENERAL)], ids=["%dx%d-%s" % g for g in GENERAL])
def test_general_form_equals_reference(k, w, h, name, order):
    """Odd pitches (4 * w + 3, made odd) and pointers 1, 2 and 3 bytes behind a 16-byte boundary; a 354-pixel row is more than one
    pass of the workgroup (256 pixels), its last pass partial, and its last thread holds two pixels of four."""
    hip = bind(A.load_hip())
    reset_forms(hip)
    layout = ORDER[order] | R.CSC[(k + (order == "rgba")) % 4]
    got = encode_rgb(hip, rgb_content(w, h, 3, 5), layout, name, pitch=odd_pitch(w), offset=1 + (k + (order == "rgba")) % 3)
    same_packets(rgb_reference(w, h, name, 3, 5, layout), got)
    assert rgb_forms(hip) == (0, 3)
    assert yuv_forms(hip) == (0, 0)


# ---- 3. smallest pictures, clamped footprints: lossless --------------------------------------------------------------------
SMALL = ([(16, 16, name, form) for name in sorted(FMT) for form in ("wide", "general")] +
         [(22, 22, "411", "general"), (22, 22, "410", "general"), (22, 18, "420", "general")])


@pytest.mark.parametrize("w,h,name,form", SMALL, ids=["%dx%d-%s-%s" % s for s in SMALL])
def test_smallest_pictures_lossless(w, h, name, form):
    """16x16 in both forms; 22x22 in 4:1:1 and "4:1:0" (cw = 6, ch = 6: the last footprint is half outside the picture both ways)
    and 22x18 in 4:2:0, which only the general form takes.  qp 100: the packets carry every bit of the planes, and the reference
    decoder gives them back to be compared with the conversion directly.

    22x22 and not 18x18 for the quarter-width formats: the REFERENCE encoder cannot encode 18x18 in 4:1:1 or "4:1:0" -- its block
    analysis averages the chroma of a block over (bw >> hs) * (bh >> vs) samples (hme.c:771, c_average), the last block of an
    18-pixel row is 2 pixels wide, 2 >> 2 = 0, and it dies of the integer division (measured: SIGFPE inside dsv_enc on the first
    picture, at any qp, also with 18 rows in "4:1:0"); so there are no reference packets to expect, and the library's block
    analysis, which restates that average, has no defined result there either.  22 = 16 + 6 is the smallest size with a
    footprint half outside that the reference encodes.  The 18x18 planes themselves (cw = 5, ch = 5) are covered where no
    encoder is needed: tools/ingest_rgb_check.cpp sweeps the kernel's text over them in every format, and
    tests/test_ingest_rgb_cpu.py compares its 18x18 4:1:1 and "4:1:0" dumps with the numpy oracle."""
    assert not stream_inverse_is_undefined(w, h, FMT[name][0], LOSSLESS)
    hip = bind(A.load_hip())
    reset_forms(hip)
    k = SMALL.index((w, h, name, form))
    layout = (R.BGRA, R.RGBA)[k & 1] | R.CSC[(k >> 1) % 4]
    pictures = rgb_content(w, h, 3, 9)
    surface = dict(pitch=aligned_pitch(w)) if form == "wide" else dict(pitch=odd_pitch(w), offset=1 + k % 3)
    got = encode_rgb(hip, pictures, layout, name, cfg=LOSSLESS, **surface)
    assert rgb_forms(hip) == ((3, 0) if form == "wide" else (0, 3))
    planes_equal_oracle(got, pictures, layout, name)
    same_packets(rgb_reference(w, h, name, 3, 9, layout, lossless=True), got)


# ---- 4. presets and saturation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["444", "420"])
@pytest.mark.parametrize("csc", R.CSC, ids=CSC_IDS)
def test_presets_and_saturation_lossless(csc, name):
    hip = bind(A.load_hip())
    layout = (R.RGBA if csc & R.BT709 else R.BGRA) | csc
    pictures = saturated_pictures()
    y, u, v = R.convert(pictures[0], layout, 0, 0)
    if csc & R.FULL:  # (U, V = 255 is the clamped 256)
        assert (y.min(), y.max()) == (0, 255) and (u.min(), u.max()) == (1, 255) and (v.min(), v.max()) == (1, 255)
    else:
        assert (y.min(), y.max()) == (16, 235) and (u.min(), u.max()) == (16, 240) and (v.min(), v.max()) == (16, 240)
    got = encode_rgb(hip, pictures, layout, name, cfg=LOSSLESS, pitch=256)
    planes_equal_oracle(got, pictures, layout, name)
    same_packets(ref_packets(pictures, layout, name, LOSSLESS), got)


# ---- 5. alpha and padding are not pixels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,surface", [(352, 288, dict(pitch=1536)), (354, 290, dict(pitch=odd_pitch(354), offset=3))], ids=["wide", "general"])
def test_alpha_and_padding_are_never_pixels(w, h, surface):
    """The same colours with alpha, pitch padding and the bytes around the surface holding 0x00, then 0xFF, then noise: identical
    packets, the reference's; every byte of the tensors is afterwards what the test put there (encode_steps)."""
    hip = bind(A.load_hip())
    pictures = rgb_content(w, h, 3, 5)
    noise = np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8)
    runs = [encode_rgb(hip, pictures, R.RGBA, "420", fill=fill, alpha=alpha, **surface) for fill, alpha in ((0x00, 0x00), (0xFF, 0xFF), (None, noise))]
    assert runs[0] == runs[1] == runs[2]
    same_packets(rgb_reference(w, h, "420", 3, 5, R.RGBA), runs[0])


# ---- 6. rows of several passes in the wide form ------------------------------------------------------------------------------
def test_1920_wide_rows_take_several_passes():
    """1920x32 4:2:0 RGBA with an 8192-byte pitch: 7.5 passes of the workgroup per row, two steps in the 16-byte form.  The
    reference cannot invert a 960x16 chroma plane as a function of its input (tests/edge_cases.py, stream_inverse_is_undefined), so
    of ITS packets only those up to the first P picture are comparable, as tests/test_gpu_edges.py has it; both pictures' ingest
    is checked against the library's own packed path on the conversion's planes, which is deterministic."""
    hip = bind(A.load_hip())
    reset_forms(hip)
    w, h, layout = 1920, 32, R.RGBA | R.BT709
    pictures = rgb_content(w, h, 2, 5)
    got = encode_rgb(hip, pictures, layout, "420", pitch=8192)
    assert rgb_forms(hip) == (2, 0)
    want = rgb_reference(w, h, "420", 2, 5, layout)
    if stream_inverse_is_undefined(w, h, FMT["420"][0], CFG):
        assert len(got) == len(want)
        same_packets(want[:2], got[:2])
    else:
        same_packets(want, got)
    assert got == packed_batch(hip, w, h, "420", oracle_frames(pictures, layout, "420"))


# ---- 7. one step: RGB and YUV surfaces mixed -----------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [False, True], ids=["general_rgb", "wide_rgb"])
def test_mixed_step(aligned):
    """Six encoders at 352x288 4:2:0 in one call per frame: packed as a surface, planar pitched, NV12, BGRA-601, RGBA-709-full and
    a BGRA surface one byte off alignment (`aligned`: on it).  Each form is chosen over its own kind of job: the three YUV
    surfaces are aligned and stay wide whatever the RGB surfaces do."""
    hip = bind(A.load_hip())
    w, h, name, nfr = 352, 288, "420", 3
    yuv = [dict(layout=PLANAR, pitches=(352, 176, 176)), CIF_PLANAR, CIF_NV12]
    rgb = [(R.BGRA | R.BT601, dict(pitch=1536)), (R.RGBA | R.BT709 | R.FULL, dict(pitch=1408)),
           (R.BGRA | R.FULL, dict(pitch=1424) if aligned else dict(pitch=1536, offset=1))]

    def make(s, t):
        if s < 3:
            return Surface(content(w, h, name, nfr, 40 + s)[t], w, h, name, **yuv[s])
        return RgbSurface(rgb_content(w, h, nfr, 40 + s)[t], rgb[s - 3][0], **rgb[s - 3][1])

    encs = encoders(hip, w, h, name, 6, CFG)
    reset_forms(hip)
    got = encode_steps(hip, encs, make, nfr)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    assert rgb_forms(hip) == ((3, 0) if aligned else (0, 3))
    assert yuv_forms(hip) == (3, 0)
    for s in range(3):
        same_packets(reference(w, h, name, nfr, 40 + s), got[s], "stream %d" % s)
    for s in range(3, 6):
        same_packets(rgb_reference(w, h, name, nfr, 40 + s, rgb[s - 3][0]), got[s], "stream %d" % s)


# ---- 8. equivalence with the packed path --------------------------------------------------------------------------------------
def test_equals_the_packed_path_on_the_converted_planes():
    """the stream of test 1 is what dsv2hip_enc_batch gives on the conversion's packed planes uploaded to the device"""
    hip = bind(A.load_hip())
    pictures = rgb_content(352, 288, 3, 5)
    got = encode_rgb(hip, pictures, R.BGRA, "420", pitch=1536)
    assert got == packed_batch(hip, 352, 288, "420", oracle_frames(pictures, R.BGRA, "420"))


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def spoil_pitch(c, w):
    c.pitch[0] = 4 * w - 1


def spoil_plane(c, w):
    c.plane[0] = None


def spoil_layout(value):
    def f(c, w):
        c.layout = value
    return f


RGB_REFUSALS = [("pitch_short", spoil_pitch), ("null_plane", spoil_plane), ("layout_0x12", spoil_layout(0x12)),
                ("layout_0x13", spoil_layout(0x13)), ("layout_0x410", spoil_layout(0x410))]


def rgb_steps_equal_reference(hip, encs, w, h, name, layouts, seeds, **surface):
    got = encode_steps(hip, encs, lambda s, t: RgbSurface(rgb_content(w, h, 3, seeds[s])[t], layouts[s], **surface), 3)
    for s in range(len(encs)):
        same_packets(rgb_reference(w, h, name, 3, seeds[s], layouts[s]), got[s], "stream %d" % s)


@pytest.mark.parametrize("what,spoil", RGB_REFUSALS, ids=[r[0] for r in RGB_REFUSALS])
def test_refused_rgb_surface_touches_nothing(what, spoil):
    """Two encoders, the second one's RGB surface spoiled: -1 (0 from the one-frame call), nbufs as the test set it, the encoders'
    bytes unchanged; the same encoders then give the reference's packets from frame 0 on."""
    hip = bind(A.load_hip())
    w, h, name = 352, 288, "420"
    layouts = [R.BGRA, R.RGBA | R.BT709]
    encs = encoders(hip, w, h, name, 2, CFG)
    good = [RgbSurface(rgb_content(w, h, 3, 5 + s)[0], layouts[s], pitch=1536) for s in range(2)]
    bad = copy_of(good[1].c)
    spoil(bad, w)
    torch.cuda.synchronize()
    refused(hip, encs, [good[0].c, bad], single=False)
    state = bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1])))
    assert hip.dsv2hip_enc_surface_frame(C.byref(encs[1]), C.byref(bad), (A.BUF * 4)()) == 0
    assert bytes(C.string_at(C.byref(encs[1]), C.sizeof(encs[1]))) == state
    rgb_steps_equal_reference(hip, encs, w, h, name, layouts, [5, 6], pitch=1536)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))


@pytest.mark.parametrize("spec,bit", [(CIF_PLANAR, R.BT709), (CIF_NV12, R.FULL)], ids=["planar_bt709", "semiplanar_full_range"])
def test_refused_csc_bit_on_a_yuv_surface(spec, bit):
    """PLANAR | DSV2HIP_CSC_BT709 and SEMIPLANAR | DSV2HIP_CSC_FULL_RANGE are no layouts; the encoder then takes the surface without the bit"""
    hip = bind(A.load_hip())
    w, h, name = 352, 288, "420"
    encs = encoders(hip, w, h, name, 1, CFG)
    sf = Surface(content(w, h, name, 3, 5)[0], w, h, name, **spec)
    bad = copy_of(sf.c)
    bad.layout |= bit
    torch.cuda.synchronize()
    refused(hip, encs, [bad])
    got = encode_steps(hip, encs, lambda s, t: Surface(content(w, h, name, 3, 5)[t], w, h, name, **spec), 3)
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(reference(w, h, name, 3, 5), got[0])


def test_refused_on_a_uyvy_encoder():
    """An encoder whose packed input is interleaved UYVY takes no RGB surface; with the switch off again it encodes it from frame 0."""
    hip = bind(A.load_hip())
    w, h, name = 176, 144, "422"
    encs = encoders(hip, w, h, name, 1, CFG)
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 1) == 0
    sf = RgbSurface(rgb_content(w, h, 3, 5)[0], R.RGBA, pitch=768)
    torch.cuda.synchronize()
    refused(hip, encs, [sf.c])
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 0) == 0
    rgb_steps_equal_reference(hip, encs, w, h, name, [R.RGBA], [5], pitch=768)
    hip.dsv_enc_free(C.byref(encs[0]))


def test_refused_with_an_encoder_of_another_geometry():
    """352x288 and 176x144 in one call: -1; each then encodes its RGB surfaces on its own from frame 0."""
    hip = bind(A.load_hip())
    geo = [(352, 288), (176, 144)]
    encs = [encoders(hip, w, h, "420", 1, CFG)[0] for w, h in geo]
    first = [RgbSurface(rgb_content(w, h, 3, 5)[0], R.BGRA, pitch=aligned_pitch(w)) for w, h in geo]
    torch.cuda.synchronize()
    refused(hip, encs, [sf.c for sf in first], single=False)
    for k, (w, h) in enumerate(geo):
        rgb_steps_equal_reference(hip, [encs[k]], w, h, "420", [R.BGRA], [5], pitch=aligned_pitch(w))
        hip.dsv_enc_free(C.byref(encs[k]))
