"""Decoded pictures delivered into pitched device surfaces (dsv2hip_dec_batch_surface, dsv2hip_dec_surface_frame,
dsv2hip_dec_surface_dims): planar and semiplanar (NV12 / NV16 / NV24) surfaces of any pitch and alignment hold the reference
decoder's pictures, bit for bit -- both forms of the chroma interleave, every chroma format, -out420p fused into the interleave,
draw_info and postsharp, both parsers, mixed surfaces and geometries in one step -- no byte outside the rows is written, a
refused call consumes nothing, and the surfaces feed dsv2hip_enc_batch_surface without a host copy."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsvabi as A
from codec_run import configure_encoder, encode_stream
import dec_out as D
import yuv_rgb as Q
from codec_run import FMT as FMT5
from dec_out import (OutSurf, Surfaces, aligned, chroma_dims, decode, decode_steps, device_decode, expected_dims, expected_sharp, frame_decode, in_layout,
                     npics, packets_of, plus1, same_results, stream, tight)
from hipabi import EIGHTH, HALF, OUTSURF, PLANAR, QUARTER, SEMI, SURFACE, bind, dec_uv_forms as forms, mk_buf, surface_dims

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

PITCH = {"tight": tight, "align256": lambda rb: (rb + 255) // 256 * 256, "plus3": lambda rb: rb + 3}


def dims_of(subsamp, w, h, layout):
    """the plane sizes of a picture of the format: dsv_mk_frame's"""
    return expected_dims(A.mk_meta(w, h, subsamp), layout)


def named(specs):
    """Surfaces over spec = dict(layout, pitch, offset) per stream, the pitch by its name in PITCH"""
    return Surfaces([dict(sp, pitch=PITCH[sp["pitch"]]) for sp in specs])


def same(want, got, layout):
    same_results(in_layout(want, layout), got)


def reference(w, h, fmt, nfr, gop=48, to420=False):
    """the reference decoder's results on the stream (dec_out.reference: shared, never modified); to420: chroma through the oracle's
    -out420p chain"""
    want = D.reference(packets_of(w, h, fmt, nfr, gop), to420=(FMT5[fmt][0], w, h) if to420 else None)
    assert npics(want) == nfr and want[0][0] == A.DEC_GOT_META and want[-1][0] == A.DEC_EOS
    return want


def is_wide(row_bytes, pitch, offset):
    """the documented rule for an interleaved plane: pointer and pitch multiples of 16, cw of 8"""
    return row_bytes % 16 == 0 and PITCH[pitch](row_bytes) % 16 == 0 and offset % 16 == 0


# ---- 1. equals the reference and writes nothing else ------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,fmt,nfr,gop", [(352, 288, "420", 9, 4), (354, 290, "420", 3, 48), (354, 290, "444", 3, 48)])
@pytest.mark.parametrize("layout", [PLANAR, SEMI], ids=["planar", "semiplanar"])
@pytest.mark.parametrize("pitch", ["tight", "align256", "plus3"])
@pytest.mark.parametrize("offset", [0, 1])
def test_equals_reference_and_writes_nothing_else(w, h, fmt, nfr, gop, layout, pitch, offset):
    """352x288 NV12 on aligned pointers and pitches: the wide form of the interleave; 354x290 (rows of 354 / 708 bytes: a ragged
    last dword), pitch + 3 or an odd pointer: the general form; planar surfaces: no interleave at all.  The bytes around the rows
    are checked after every step (Surf.planes)."""
    hip = bind(A.load_hip())
    packets = packets_of(w, h, fmt, nfr, gop)
    if gop == 4:
        assert len(packets) > nfr + 2  # (a metadata packet per GOP: I and P pictures both occur)
    forms(hip, reset=True)
    got = decode_steps(hip, [packets], named([dict(layout=layout, pitch=pitch, offset=offset)]))[0]
    same(reference(w, h, fmt, nfr, gop), got, layout)
    if layout == PLANAR:
        assert forms(hip) == (0, 0)
    else:
        wide = is_wide(2 * chroma_dims(FMT5[fmt][0], w, h)[0], pitch, offset)
        if (w, offset) == (352, 0) and pitch != "plus3":
            assert wide
        if offset == 1 or pitch == "plus3" or w == 354:
            assert not wide
        assert forms(hip) == ((nfr, 0) if wide else (0, nfr))


# ---- 2. other chroma formats -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [PLANAR, SEMI], ids=["planar", "semiplanar"])
@pytest.mark.parametrize("fmt", ["422", "411", "410"])
def test_other_chroma_formats(fmt, layout):
    hip = bind(A.load_hip())
    got = decode_steps(hip, [packets_of(330, 250, fmt, 3)], named([dict(layout=layout, pitch="plus3", offset=0)]))[0]
    same(reference(330, 250, fmt, 3), got, layout)


# ---- 3. -out420p into NV12 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", ["tight", "plus3"])
@pytest.mark.parametrize("w,h,fmt", [(354, 290, "444"), (330, 250, "422"), (330, 250, "411"), (330, 250, "410")])
def test_out420p_into_nv12(w, h, fmt, pitch):
    """The conversion fused with the interleave, edge clamps included: every source plane here has an odd width or height or
    both (354 -> 177 pairs from 354 samples, 330x250 -> 165 x 125 from 165 / 83 wide, 250 / 63 tall planes)."""
    hip = bind(A.load_hip())
    forms(hip, reset=True)
    got = decode_steps(hip, [packets_of(w, h, fmt, 3)], named([dict(layout=SEMI, pitch=pitch, offset=0)]), out420p=[True])[0]
    same(reference(w, h, fmt, 3, to420=True), got, SEMI)
    assert got[1][2][1].shape == ((h + 1) // 2, 2 * ((w + 1) // 2))
    assert forms(hip) == (0, 3)  # (odd row bytes / 2: 354 and 330 are no multiples of 16)


# ---- 4. draw_info and postsharp ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [True, False], ids=["every_picture", "odd_packets_only"])
def test_draw_info_and_postsharp_into_pitched_nv12(every):
    """draw_info = 7 and postsharp: the overlay and the sharpening land in the delivered luma only -- the chroma is the undrawn
    decode's, and with both switched on for the odd packets only, the pictures in between (P pictures predicted from drawn-on,
    sharpened ones) are the plain reference's."""
    ref, hip = A.load_ref(), bind(A.load_hip())
    packets = stream(352, 288, "420", 9, 4)
    mode = 7 if every else (lambda k: 7 * (k & 1))
    sharp = True if every else (lambda k: k % 2 == 1)
    want = expected_sharp(ref, packets, mode=mode, sharp=sharp)
    plain = reference(352, 288, "420", 9, 4)
    got = decode_steps(hip, [packets], named([dict(layout=SEMI, pitch="align256", offset=0)]), modes=[mode], sharp=[sharp])[0]
    same(want, got, SEMI)
    same_results(in_layout(plain, SEMI), got, planes=(1,))  # chroma: the undrawn decode's
    touched = [k for k, (a, b) in enumerate(zip(plain, got)) if a[2] is not None and not np.array_equal(a[2][0], b[2][0])]
    pics = [k for k, a in enumerate(plain) if a[2] is not None]
    assert touched == (pics if every else [k for k in pics if k % 2 == 1])
    assert any(plain[k][0] == A.DEC_OK and k % 2 == 0 for k in pics[1:])  # (untouched pictures behind touched ones exist)


# ---- 5. one step, mixed ------------------------------------------------------------------------------------------------------
def mixed_step(hip):
    cif, c444, hd = stream(352, 288, "420", 9, 4), stream(354, 290, "444", 3, 48), stream(1280, 720, "420", 3, 48)
    specs = [dict(layout=PLANAR, pitch="tight", offset=0), dict(layout=SEMI, pitch="align256", offset=0),
             dict(layout=SEMI, pitch="plus3", offset=1), dict(layout=PLANAR, pitch="align256", offset=0)]
    got = decode_steps(hip, [cif, cif, c444, hd], named(specs), out420p=[False, False, True, False])
    same(reference(352, 288, "420", 9, 4), got[0], PLANAR)
    same(reference(352, 288, "420", 9, 4), got[1], SEMI)
    same(reference(354, 290, "444", 3, to420=True), got[2], SEMI)
    same(reference(1280, 720, "420", 3), got[3], PLANAR)
    assert got[2][1][2][1].shape == (145, 354)


def test_mixed_surfaces_and_geometries_in_one_step():
    """Four decoders in one step sequence: CIF planar tight, CIF NV12 aligned, 354x290 4:4:4 with -out420p into NV12 at an odd
    address, 1280x720 planar padded."""
    mixed_step(bind(A.load_hip()))


def test_mixed_surfaces_and_geometries_in_one_step_device_parser():
    hip = bind(A.load_hip())
    try:
        assert hip.dsv2hip_dec_set_parse_mode(2) == 2
        mixed_step(hip)
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)


# ---- 6. packed equals planar-tight -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,fmt,out420p", [(352, 288, "420", False), (354, 290, "444", False), (354, 290, "444", True)])
def test_packed_equals_planar_tight(w, h, fmt, out420p):
    """dsv2hip_dec_batch_device and dsv2hip_dec_batch_surface with pitch {w, cw, cw} on the same packets; the sizes
    dsv2hip_dec_surface_dims reports add up to dsv2hip_dec_picture_bytes."""
    hip = bind(A.load_hip())
    packets = packets_of(w, h, fmt, 3)
    packed = device_decode(hip, [packets], out420p=[out420p])[0]
    got = decode_steps(hip, [packets], named([dict(layout=PLANAR, pitch="tight", offset=0)]), out420p=[out420p])[0]
    assert npics(packed) == 3
    same_results(packed, got)
    dec = A.DECODER()
    if out420p:
        assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 1) == 0
    buf = A.BUF()
    mk_buf(hip, buf, packets[0])
    fn = C.c_uint32(0)
    assert hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(buf), C.byref(OUTSURF()), C.byref(fn)) == A.DEC_GOT_META
    pb = hip.dsv2hip_dec_picture_bytes(C.byref(dec))
    for layout in (PLANAR, SEMI):
        dims = surface_dims(hip, dec, layout)
        assert dims == dims_of(A.SUBSAMP_420 if out420p else FMT5[fmt][0], w, h, layout)
        assert sum(rb * rows for rb, rows in dims) == pb > 0
    hip.dsv_dec_free(C.byref(dec))


# ---- 7. refusals consume nothing ---------------------------------------------------------------------------------------------
def spoil_layout(c, dims):
    c.layout = 2


def spoil_plane(p):
    def f(c, dims):
        c.plane[p] = None
    return f


def spoil_pitch(p):
    def f(c, dims):
        c.pitch[p] = dims[p][0] - 1
    return f


def spoil_cap(p):
    def f(c, dims):
        c.cap[p] -= 1
    return f


REFUSALS = ([("layout_%s" % name, lay, spoil_layout) for name, lay in (("planar", PLANAR), ("semiplanar", SEMI))] +
            [("null_planar_%d" % p, PLANAR, spoil_plane(p)) for p in range(3)] + [("null_semiplanar_%d" % p, SEMI, spoil_plane(p)) for p in range(2)] +
            [("pitch_planar_%d" % p, PLANAR, spoil_pitch(p)) for p in range(3)] + [("pitch_semiplanar_%d" % p, SEMI, spoil_pitch(p)) for p in range(2)] +
            [("cap_planar_%d" % p, PLANAR, spoil_cap(p)) for p in range(3)] + [("cap_semiplanar_%d" % p, SEMI, spoil_cap(p)) for p in range(2)])


def test_dims_before_metadata_and_for_null():
    hip = bind(A.load_hip())
    rb, rows = (C.c_size_t * 3)(), (C.c_int * 3)()
    dec = A.DECODER()
    assert hip.dsv2hip_dec_surface_dims(None, PLANAR, rb, rows) == -1
    assert hip.dsv2hip_dec_surface_dims(C.byref(dec), PLANAR, rb, rows) == -1
    assert hip.dsv2hip_dec_surface_dims(C.byref(dec), SEMI, rb, rows) == -1


@pytest.mark.parametrize("layout", [PLANAR, SEMI], ids=["planar", "semiplanar"])
def test_refused_calls_consume_nothing(layout):
    """Every spoiled surface of the layout, n = 0 and NULL arrays: -1, the packet, the decoder and the surface as they were; the
    same packet with the good surface then decodes to the reference's picture."""
    hip = bind(A.load_hip())
    packets = stream(352, 288, "420", 9, 4)
    want = reference(352, 288, "420", 9, 4)
    dec = A.DECODER()
    decp = (C.POINTER(A.DECODER) * 1)(C.pointer(dec))
    fns, rets = (C.c_uint32 * 1)(), (C.c_int * 1)()
    bufs, arr = (A.BUF * 1)(), (OUTSURF * 1)()
    # no metadata yet: an all-zero entry is allowed, the metadata packet is consumed
    mk_buf(hip, bufs[0], packets[0])
    assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, arr, fns, rets) == 1
    assert rets[0] == A.DEC_GOT_META and dec.got_metadata == 1
    dims = surface_dims(hip, dec, layout)
    assert dims == dims_of(A.SUBSAMP_420, 352, 288, layout)
    surf = OutSurf(dims, layout, PITCH["align256"], 0)
    surf.arm()
    torch.cuda.synchronize()
    mk_buf(hip, bufs[0], packets[1])
    data, length = C.cast(bufs[0].data, C.c_void_p).value, bufs[0].len
    state = bytes(C.string_at(C.byref(dec), C.sizeof(dec)))

    def nothing_happened():
        assert C.cast(bufs[0].data, C.c_void_p).value == data and bufs[0].len == length
        assert bytes(C.string_at(bufs[0].data, len(packets[1]))) == packets[1]
        assert bytes(C.string_at(C.byref(dec), C.sizeof(dec))) == state
        assert surf.untouched()

    tried = 0
    for what, lay, spoil in REFUSALS:
        if lay != layout:
            continue
        C.memmove(C.byref(arr[0]), C.byref(surf.c), C.sizeof(OUTSURF))
        spoil(arr[0], dims)
        assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, arr, fns, rets) == -1, what
        assert hip.dsv2hip_dec_surface_frame(C.byref(dec), bufs, arr, fns) == -1, what
        nothing_happened()
        tried += 1
    assert tried == (10 if layout == PLANAR else 7)
    arr[0] = surf.c
    assert hip.dsv2hip_dec_batch_surface(0, decp, bufs, arr, fns, rets) == -1
    assert hip.dsv2hip_dec_batch_surface(1, None, bufs, arr, fns, rets) == -1
    assert hip.dsv2hip_dec_batch_surface(1, decp, None, arr, fns, rets) == -1
    assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, None, fns, rets) == -1
    assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, arr, None, rets) == -1
    assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, arr, fns, None) == -1
    assert hip.dsv2hip_dec_batch_surface(1, (C.POINTER(A.DECODER) * 1)(), bufs, arr, fns, rets) == -1
    assert hip.dsv2hip_dec_surface_frame(C.byref(dec), bufs, None, fns) == -1
    nothing_happened()
    # the same packet with the good surface: decoded as if nothing had happened
    assert hip.dsv2hip_dec_batch_surface(1, decp, bufs, arr, fns, rets) == 1
    assert rets[0] == A.DEC_OK and fns[0] == want[1][1]
    same_results(in_layout([want[1]], layout), [(rets[0], fns[0], surf.planes())], planes=(0, 1) if layout == SEMI else (0, 1, 2))
    hip.dsv_dec_free(C.byref(dec))


# ---- 8. transcode through surfaces without the host --------------------------------------------------------------------------
def test_transcode_through_surfaces_without_the_host():
    """Two CIF streams decoded into pitched NV12 surfaces whose pointers and pitches go straight to dsv2hip_enc_batch_surface: the
    packets are the reference encoder's on the reference decoder's pictures.  dsv2hip_dec_surface_frame gives the batch call's
    pictures."""
    ref, hip = A.load_ref(), bind(A.load_hip())
    w, h, ns = 352, 288, 2
    streams = [stream(w, h, "420", 5, 4, seed=70 + s) for s in range(ns)]
    refpics = [[r for r in decode(ref, pk, 0) if r[2] is not None] for pk in streams]
    want = [encode_stream(ref, [b"".join(p.tobytes() for p in r[2]) for r in pics], w, h, A.SUBSAMP_420, eos=False, qp=50, gop=48)[0]
            for pics in refpics]
    meta = A.mk_meta(w, h, A.SUBSAMP_420)
    encs, decs = [A.ENCODER() for _ in range(ns)], [A.DECODER() for _ in range(ns)]
    for e in encs:
        configure_encoder(hip, e, meta, qp=50, gop=48)
    surfs = [OutSurf(dims_of(A.SUBSAMP_420, w, h, SEMI), SEMI, PITCH["align256"], 0) for _ in range(ns)]

    def as_input(sf):
        c = SURFACE()
        c.layout = sf.c.layout
        for i in range(3):
            c.plane[i], c.pitch[i] = sf.c.plane[i], sf.c.pitch[i]
        return c

    for sf in surfs:
        sf.arm()
    torch.cuda.synchronize()
    got, pics = [[] for _ in range(ns)], [[] for _ in range(ns)]
    for t in range(max(len(s) for s in streams)):
        live = [k for k in range(ns) if t < len(streams[k])]
        m = len(live)
        decp = (C.POINTER(A.DECODER) * m)(*[C.pointer(decs[k]) for k in live])
        bufs = (A.BUF * m)()
        for i, k in enumerate(live):
            mk_buf(hip, bufs[i], streams[k][t])
        arr = (OUTSURF * m)(*[surfs[k].c for k in live])
        fns, rets = (C.c_uint32 * m)(), (C.c_int * m)()
        had_meta = [decs[k].got_metadata for k in live]
        assert hip.dsv2hip_dec_batch_surface(m, decp, bufs, arr, fns, rets) == m
        ready = [k for i, k in enumerate(live) if rets[i] == A.DEC_OK and had_meta[i]]
        if not ready:
            continue
        r = len(ready)
        encp = (C.POINTER(A.ENCODER) * r)(*[C.pointer(encs[k]) for k in ready])
        src = (SURFACE * r)(*[as_input(surfs[k]) for k in ready])
        obufs, nbufs = (A.BUF * (4 * r))(), (C.c_int * r)()
        assert hip.dsv2hip_enc_batch_surface(r, encp, src, obufs, nbufs) == 0
        for i, k in enumerate(ready):
            pics[k].append(surfs[k].planes())
            for q in range(nbufs[i]):
                b = obufs[4 * i + q]
                got[k].append(bytes(C.string_at(b.data, b.len)))
                hip.dsv_buf_free(C.byref(b))
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    for d in decs:
        hip.dsv_dec_free(C.byref(d))
    for s in range(ns):
        assert len(pics[s]) == 5
        assert len(want[s]) == len(got[s])
        for i, (a, b) in enumerate(zip(want[s], got[s])):
            assert a == b, "stream %d packet %d differs" % (s, i)
    # one decoder, one call per packet
    dec = A.DECODER()
    one = []
    sf = OutSurf(dims_of(A.SUBSAMP_420, w, h, SEMI), SEMI, PITCH["align256"], 0)
    sf.arm()
    torch.cuda.synchronize()
    for pk in streams[0]:
        buf = A.BUF()
        mk_buf(hip, buf, pk)
        fn = C.c_uint32(0)
        had_meta = dec.got_metadata
        code = hip.dsv2hip_dec_surface_frame(C.byref(dec), C.byref(buf), C.byref(sf.c), C.byref(fn))
        if code == A.DEC_OK and had_meta:
            one.append((fn.value, sf.planes()))
        if code == A.DEC_EOS:
            break
    hip.dsv_dec_free(C.byref(dec))
    assert code == A.DEC_EOS and [f for f, _ in one] == [r[1] for r in refpics[0]]
    for (_, a), b in zip(one, pics[0]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 9. every way out side by side -------------------------------------------------------------------------------------------
def test_every_delivery_in_one_round():
    """Ten decoders of one geometry (66x34 4:2:0) on the same I P P stream, one lockstep step per picture, each with another way out:
    pinned frames (plain, sharpened, drawn on and sharpened), the packed device buffer, a planar surface at an odd pitch and address,
    NV12, half-size NV12 drawn on and sharpened, BGRA BT.709, sharpened quarter-size RGBA, eighth-size planar.  Every decoder
    delivers, byte for byte -- the helpers check the guard bytes around every plane after every step --, what a decoder with its
    settings delivers alone, which the tests above and those of the other ways out pin to the reference.  The ABI has one entry
    point per kind of destination, so a step is three calls: the three pinned frames share a round, the six surfaces share one,
    and the packed buffer has its own.  This guards the packing of several pictures' jobs into one round's tables."""
    hip = bind(A.load_hip())
    packets = stream(66, 34, "420", 3, 48, seed=71)
    assert [pk[5] & 1 for pk in packets if pk[5] & 0x04] == [0, 1, 1]  # (dsv.h: packet type at byte 5, picture = 0x04, bit 0 = predicted)
    frames = [(0, False), (0, True), (7, True)]  # (draw_info, postsharp)
    surfaces = [(dict(layout=PLANAR, pitch=plus1, offset=1), 0, False),
                (dict(layout=SEMI, pitch=aligned, offset=0), 0, False),
                (dict(layout=SEMI | HALF, pitch=tight, offset=0), 7, True),
                (dict(layout=Q.BGRA | Q.BT709, pitch=aligned, offset=0), 0, False),
                (dict(layout=Q.RGBA | QUARTER, pitch=tight, offset=0), 0, True),
                (dict(layout=PLANAR | EIGHTH, pitch=tight, offset=0), 0, False)]

    def steps(fr, packed, sf):
        """the three calls of a step sequence over the chosen decoders of each kind"""
        return (frame_decode(hip, [packets] * len(fr), [m for m, _ in fr], [s for _, s in fr]) if fr else [],
                device_decode(hip, [packets]) if packed else [],
                decode_steps(hip, [packets] * len(sf), Surfaces([spec for spec, _, _ in sf]), modes=[m for _, m, _ in sf], sharp=[s for _, _, s in sf]) if sf else [])

    got_frames, got_packed, got_surfaces = steps(frames, True, surfaces)
    assert all(npics(r) == 3 for r in got_frames + got_packed + got_surfaces)
    for k, f in enumerate(frames):
        same_results(steps([f], False, [])[0][0], got_frames[k])
    same_results(steps([], True, [])[1][0], got_packed[0])
    for k, s in enumerate(surfaces):
        alone = steps([], False, [s])[2][0]
        same_results(alone, got_surfaces[k], planes=range(len(alone[1][2])))
    # (the settings take effect: the drawn-on, sharpened pictures differ from the plain ones)
    assert not np.array_equal(got_frames[0][1][2][0], got_frames[1][1][2][0]) and not np.array_equal(got_frames[1][1][2][0], got_frames[2][1][2][0])
