"""Pitched device surfaces as encoder input (dsv2hip_enc_batch_surface, dsv2hip_enc_surface_frame): planar and semi-planar
(NV12 / NV16 / NV24) surfaces of any pitch and alignment give the reference encoder's packets on the same pixels -- both forms
of the ingest kernel, rows wider than one workgroup pass, mixed surfaces in one step -- padding is never read as pixels, the
surface is never written, and a refused call touches nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsvabi as A
from codec_run import FMT
from enc_in import CIF_NV12, CIF_PLANAR, Surface, content, copy_of, dims, encode_steps, encoders, packed_batch, reference, refused, same_packets, take_packets
from hipabi import BGR, BGRA, BT709, HALF, PLANAR, RGBA, RGBP, SEMI, SURFACE, bind, enc_yuv_forms as forms

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def row_bytes(w, h, name, layout):
    """bytes of a row of each source plane of the layout"""
    _, d = dims(w, h, name)
    return [d[0][0], 2 * d[1][0]] if layout == SEMI else [p[0] for p in d]


def encode_with(hip, w, h, name, specs, nfr=3, seed0=5):
    """One encoder per spec = dict(layout, pitches, offsets, fill), stream s encoding content(seed0 + s); frees the encoders."""
    code = dims(w, h, name)[0]
    assert code == FMT[name][0]
    encs = encoders(hip, w, h, name, len(specs))
    got = encode_steps(hip, encs, lambda s, t: Surface(content(w, h, name, nfr, seed0 + s)[t], w, h, name, **specs[s]), nfr)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    return got


def odd_pitch(rb):
    return (rb + 3) | 1


# ---- 1. parity, wide form ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("spec", [CIF_PLANAR, CIF_NV12], ids=["planar", "nv12"])
def test_wide_form_equals_reference(spec):
    """352x288 4:2:0 (chroma rows of 176 bytes, NV12 rows of 352), aligned pointers and pitches: the 16-byte form."""
    hip = bind(A.load_hip())
    forms(hip, reset=True)
    got = encode_with(hip, 352, 288, "420", [spec])
    same_packets(reference(352, 288, "420", 3, 5), got[0])
    assert forms(hip) == (3, 0)


# ---- 2. parity, general form ------------------------------------------------------------------------------------------
GENERAL = [(354, 290, "420")] + [(176, 144, name) for name in sorted(FMT)]


@pytest.mark.parametrize("layout", [PLANAR, SEMI], ids=["planar", "semiplanar"])
@pytest.mark.parametrize("w,h,name", GENERAL)
def test_general_form_equals_reference(w, h, name, layout):
    """Odd pitches (row bytes + 3, made odd) and plane pointers 1, 2 and 3 bytes behind a 16-byte boundary; 354x290 has
    177-sample chroma rows (NV12 rows of 354 bytes: the last U V pair of a row is half a dword)."""
    hip = bind(A.load_hip())
    forms(hip, reset=True)
    spec = dict(layout=layout, pitches=tuple(odd_pitch(rb) for rb in row_bytes(w, h, name, layout)), offsets=(1, 2, 3))
    got = encode_with(hip, w, h, name, [spec])
    same_packets(reference(w, h, name, 3, 5), got[0])
    assert forms(hip) == (0, 3)


# ---- 3. rows wider than 2048 bytes in the wide form ---------------------------------------------------------------------
def test_2160p_nv12_takes_the_wide_form():
    """3840x2160 NV12 with a 4096-byte pitch: every row is several passes of the workgroup (1024 bytes each); the counter of
    dsv2hip_enc_surface_stats shows that both steps ran the 16-byte form."""
    hip = bind(A.load_hip())
    forms(hip, reset=True)
    got = encode_with(hip, 3840, 2160, "420", [dict(layout=SEMI, pitches=(4096, 4096))], nfr=2)
    same_packets(reference(3840, 2160, "420", 2, 5), got[0])
    assert forms(hip) == (2, 0)


# ---- 4. padding is not pixels; the surface is not written ----------------------------------------------------------------
@pytest.mark.parametrize("w,h,spec", [(352, 288, CIF_NV12),
                                      (354, 290, dict(layout=PLANAR, pitches=(357, 181, 181), offsets=(1, 2, 3)))],
                         ids=["nv12_wide", "planar_general"])
def test_padding_is_never_read_and_nothing_is_written(w, h, spec):
    """The same pixels with the pitch padding and the bytes around the planes holding 0x00, then 0xFF: identical packets, the
    reference's; every byte of the tensors is afterwards what the test put there (checked after each step: encode_steps)."""
    hip = bind(A.load_hip())
    zero = encode_with(hip, w, h, "420", [dict(spec, fill=0x00)])[0]
    ones = encode_with(hip, w, h, "420", [dict(spec, fill=0xFF)])[0]
    assert zero == ones
    same_packets(reference(w, h, "420", 3, 5), zero)


# ---- 5. one step, mixed surfaces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [False, True], ids=["general_step", "wide_step"])
def test_mixed_surfaces_in_one_step(aligned):
    """Five encoders with different content in one call per frame: packed as a surface (pitch = width), planar pitched, NV12,
    NV12 one byte off a 16-byte boundary and planar with odd pitches -- the last two force the step's general form; with
    `aligned` they are aligned surfaces of other pitches and the whole step is wide."""
    hip = bind(A.load_hip())
    w, h = 352, 288
    specs = [dict(layout=PLANAR, pitches=(352, 176, 176)), CIF_PLANAR, CIF_NV12,
             dict(layout=SEMI, pitches=(384, 368)) if aligned else dict(layout=SEMI, pitches=(512, 512), offsets=(1, 1, 0)),
             dict(layout=PLANAR, pitches=(368, 192, 208)) if aligned else dict(layout=PLANAR, pitches=(355, 179, 181))]
    forms(hip, reset=True)
    got = encode_with(hip, w, h, "420", specs, seed0=40)
    assert forms(hip) == ((3, 0) if aligned else (0, 3))
    for s in range(len(specs)):
        same_packets(reference(w, h, "420", 3, 40 + s), got[s], "stream %d" % s)
    assert got[0] == packed_batch(hip, w, h, "420", content(w, h, "420", 3, 40))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def break_pitch(layout, plane):
    def f(c, w, h, name):
        c.pitch[plane] = row_bytes(w, h, name, layout)[plane] - 1
    return f


def null_plane(plane):
    def f(c, w, h, name):
        c.plane[plane] = None
    return f


def bad_layout(c, w, h, name):
    c.layout = 2


REFUSALS = ([("pitch_short_planar_%d" % p, PLANAR, break_pitch(PLANAR, p)) for p in range(3)] +
            [("pitch_short_semiplanar_%d" % p, SEMI, break_pitch(SEMI, p)) for p in range(2)] +
            [("null_planar_%d" % p, PLANAR, null_plane(p)) for p in range(3)] +
            [("null_semiplanar_%d" % p, SEMI, null_plane(p)) for p in range(2)] +
            [("layout_2_planar", PLANAR, bad_layout), ("layout_2_semiplanar", SEMI, bad_layout)])


@pytest.mark.parametrize("what,layout,spoil", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_surface_touches_nothing(what, layout, spoil):
    """Two encoders, the second one's surface spoiled: -1 (0 from the one-frame call), nbufs as the test set it; the same
    encoders then give the reference's packets from frame 0 on."""
    hip = bind(A.load_hip())
    w, h, name = 352, 288, "420"
    spec = CIF_NV12 if layout == SEMI else CIF_PLANAR
    encs = encoders(hip, w, h, name, 2)
    good = [Surface(content(w, h, name, 3, 5 + s)[0], w, h, name, **spec) for s in range(2)]
    bad = copy_of(good[1].c)
    spoil(bad, w, h, name)
    torch.cuda.synchronize()
    refused(hip, encs, [good[0].c, bad], single=False)
    bufs = (A.BUF * 4)()
    assert hip.dsv2hip_enc_surface_frame(C.byref(encs[1]), C.byref(bad), bufs) == 0
    got = encode_steps(hip, encs, lambda s, t: Surface(content(w, h, name, 3, 5 + s)[t], w, h, name, **spec), 3)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    for s in range(2):
        same_packets(reference(w, h, name, 3, 5 + s), got[s], "stream %d" % s)


def test_refused_arguments():
    """n <= 0, NULL arrays, a NULL encoder, a NULL surface: refused, and the encoder still starts at frame 0"""
    hip = bind(A.load_hip())
    w, h, name = 352, 288, "420"
    encs = encoders(hip, w, h, name, 1)
    sf = Surface(content(w, h, name, 3, 5)[0], w, h, name, **CIF_NV12)
    torch.cuda.synchronize()
    encp, bufs, nbufs = (C.POINTER(A.ENCODER) * 1)(C.pointer(encs[0])), (A.BUF * 4)(), (C.c_int * 1)(77)
    arr = (SURFACE * 1)(sf.c)
    assert hip.dsv2hip_enc_batch_surface(0, encp, arr, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_surface(-1, encp, arr, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_surface(1, None, arr, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_surface(1, encp, None, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_batch_surface(1, encp, arr, None, nbufs) == -1
    assert hip.dsv2hip_enc_batch_surface(1, encp, arr, bufs, None) == -1
    assert hip.dsv2hip_enc_batch_surface(1, (C.POINTER(A.ENCODER) * 1)(), arr, bufs, nbufs) == -1
    assert hip.dsv2hip_enc_surface_frame(None, arr, bufs) == 0
    assert hip.dsv2hip_enc_surface_frame(C.byref(encs[0]), None, bufs) == 0
    assert hip.dsv2hip_enc_surface_frame(C.byref(encs[0]), arr, None) == 0
    assert nbufs[0] == 77
    # the one-frame call, frame by frame, from frame 0
    got = [[]]
    for t in range(3):
        s = Surface(content(w, h, name, 3, 5)[t], w, h, name, **CIF_NV12)
        torch.cuda.synchronize()
        nb = (C.c_int * 1)(hip.dsv2hip_enc_surface_frame(C.byref(encs[0]), C.byref(s.c), bufs))
        take_packets(hip, bufs, nb, got)
        s.check_untouched()
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(reference(w, h, name, 3, 5), got[0])


def test_refused_on_a_uyvy_encoder():
    """An encoder whose packed input is interleaved UYVY takes no surface; with the switch off again it encodes NV16 from
    frame 0."""
    hip = bind(A.load_hip())
    w, h, name = 176, 144, "422"
    encs = encoders(hip, w, h, name, 1)
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 1) == 0
    spec = dict(layout=SEMI, pitches=(256, 256))
    sf = Surface(content(w, h, name, 3, 5)[0], w, h, name, **spec)
    torch.cuda.synchronize()
    refused(hip, encs, [sf.c])
    assert hip.dsv2hip_enc_set_uyvy_input(C.byref(encs[0]), 0) == 0
    got = encode_steps(hip, encs, lambda s, t: Surface(content(w, h, name, 3, 5)[t], w, h, name, **spec), 3)
    hip.dsv_enc_free(C.byref(encs[0]))
    same_packets(reference(w, h, name, 3, 5), got[0])


def test_refused_with_an_encoder_of_another_geometry():
    """352x288 and 176x144 in one call: -1; each then encodes on its own from frame 0."""
    hip = bind(A.load_hip())
    geo = [(352, 288), (176, 144)]
    encs = [encoders(hip, w, h, "420", 1)[0] for w, h in geo]
    spec = [CIF_NV12, dict(layout=SEMI, pitches=(256, 256))]
    first = [Surface(content(w, h, "420", 3, 5)[0], w, h, "420", **spec[k]) for k, (w, h) in enumerate(geo)]
    torch.cuda.synchronize()
    refused(hip, encs, [sf.c for sf in first], single=False)
    for k, (w, h) in enumerate(geo):
        got = encode_steps(hip, [encs[k]], lambda s, t: Surface(content(w, h, "420", 3, 5)[t], w, h, "420", **spec[k]), 3)
        hip.dsv_enc_free(C.byref(encs[k]))
        same_packets(reference(w, h, "420", 3, 5), got[0], "%dx%d" % (w, h))


# ---- 7. every way in, side by side ---------------------------------------------------------------------------------------------
# (call, layout, the picture in the surface, its planes as (row bytes, rows)) for nine 34x18 4:2:0 encoders
WAYS_IN = [("plain", PLANAR, (34, 18), [(34, 18), (17, 9), (17, 9)]),
           ("plain", SEMI, (34, 18), [(34, 18), (34, 9)]),
           ("plain", BGRA, (34, 18), [(136, 18)]),
           ("plain", BGR, (34, 18), [(102, 18)]),
           ("plain", RGBP, (34, 18), [(34, 18)] * 3),
           ("scaled", SEMI | HALF, (67, 35), [(67, 35), (68, 18)]),
           ("scaled", RGBA | HALF, (67, 35), [(268, 35)]),
           ("sized", PLANAR, (35, 19), [(35, 19), (18, 10), (18, 10)]),
           ("sized", BGRA | BT709, (51, 27), [(204, 27)])]


def all_forms(hip, reset=False):
    got = {}
    for name, n in (("surface", 2), ("rgb", 2), ("scale", 4), ("resize", 4), ("rgb3", 4)):
        out = (C.c_ulonglong * n)()
        getattr(hip, "dsv2hip_enc_%s_stats" % name)(out, int(reset))
        got[name] = tuple(out)
    return got


def test_every_ingest_in_one_session():
    """Nine 34x18 4:2:0 encoders, three frames (I P P); per frame the plain call with planar, NV12, BGRA, BGR and RGBP, the scaled call
    with NV12 and RGBA at half size from 67x35 and the sized call with planar from 35x19 and BGRA-709 from 51x27.  Every stream's packets
    are those of a fresh encoder fed the same surfaces alone through the matching one-frame call, and each of the five form counters
    counts its own kind and no other: tight pitches and 16-byte aligned planes, so only the sized RGB ingest (pitch 204) is wide."""
    hip = bind(A.load_hip())
    w, h, nfr = 34, 18, 3
    rng = np.random.RandomState(34)
    surfs = []  # [stream][frame]: (SURFACE, its tensors)
    for s, (_, layout, _, planes) in enumerate(WAYS_IN):
        per_frame = []
        for t in range(nfr):
            c, keep = SURFACE(), []
            c.layout = layout
            for i, (rb, rows) in enumerate(planes):
                y, x = np.mgrid[0:rows, 0:rb]
                pl = ((3 * x + 5 * y + 11 * s + 2 * t) % 200 + rng.randint(0, 9, size=(rows, rb))).astype(np.uint8)
                keep.append(torch.from_numpy(pl).cuda())
                assert keep[-1].data_ptr() % 16 == 0
                c.plane[i], c.pitch[i] = keep[-1].data_ptr(), rb
            per_frame.append((c, keep))
        surfs.append(per_frame)
    torch.cuda.synchronize()
    groups = {call: [s for s, way in enumerate(WAYS_IN) if way[0] == call] for call in ("plain", "scaled", "sized")}
    encs = encoders(hip, w, h, "420", len(WAYS_IN))
    got = [[] for _ in WAYS_IN]
    all_forms(hip, reset=True)
    for t in range(nfr):
        for call, ids in groups.items():
            n = len(ids)
            encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(encs[s]) for s in ids])
            arr = (SURFACE * n)(*[surfs[s][t][0] for s in ids])
            sw, sh = (C.c_int * n)(*[WAYS_IN[s][2][0] for s in ids]), (C.c_int * n)(*[WAYS_IN[s][2][1] for s in ids])
            bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)()
            if call == "plain":
                assert hip.dsv2hip_enc_batch_surface(n, encp, arr, bufs, nbufs) == 0
            else:
                assert getattr(hip, "dsv2hip_enc_batch_surface_" + call)(n, encp, arr, sw, sh, bufs, nbufs) == 0
            part = [[] for _ in ids]
            take_packets(hip, bufs, nbufs, part)
            for k, s in enumerate(ids):
                got[s] += part[k]
    counted = all_forms(hip)
    assert counted == dict(surface=(0, 3), rgb=(0, 3), scale=(0, 3, 0, 3), resize=(0, 3, 3, 0), rgb3=(0, 3, 0, 3)), counted
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    for s, (call, _, (sw, sh), _) in enumerate(WAYS_IN):
        enc = encoders(hip, w, h, "420", 1)[0]
        alone, bufs = [[]], (A.BUF * 4)()
        for t in range(nfr):
            c = surfs[s][t][0]
            if call == "plain":
                nb = hip.dsv2hip_enc_surface_frame(C.byref(enc), C.byref(c), bufs)
            else:
                nb = getattr(hip, "dsv2hip_enc_surface_frame_" + call)(C.byref(enc), C.byref(c), sw, sh, bufs)
            assert nb > 0, "stream %d, frame %d: no packets" % (s, t)
            take_packets(hip, bufs, (C.c_int * 1)(nb), alone)
        hip.dsv_enc_free(C.byref(enc))
        same_packets(alone[0], got[s], "stream %d (%s call, layout %#x)" % (s, call, WAYS_IN[s][1]))
