"""Decoded pictures delivered into packed four-byte RGB device surfaces (DSV2HIP_SURFACE_BGRA / _RGBA, or-ed with DSV2HIP_CSC_*,
through dsv2hip_dec_batch_surface / dsv2hip_dec_surface_frame): the surface holds exactly the conversion of include/dsv2_hip.h
(tests/yuv_rgb.py, numpy) of the planar picture that a second decoder of the library delivers from the same packets, under the same
switches, into a PLANAR surface -- a delivery the existing tests pin to the reference decoder.  Both forms of k_egress_rgb, both
byte orders, the four presets, the five chroma formats, the smallest pictures, saturated content that reaches both clamps, rows of
several passes, draw_info and postsharp, RGB and YUV surfaces and two geometries mixed in one step with either parser; every alpha
byte is 255, no byte outside the rows is written, a refused call consumes nothing, and the surface feeds
dsv2hip_enc_surface_frame without a host copy."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dsvabi as A
import rgb_csc as R
import yuv_rgb as Q
from codec_run import configure_encoder, encode_stream
from edge_cases import packet_bound_holds
from test_gpu_dec_device_out import format_stream, mk_buf, npics, same_results
from test_gpu_dec_drawinfo import stream
from test_gpu_dec_surface import GUARD, LEAD, NO_FN, OUTSURF, PLANAR, SEMI, packets_of, surface_decode, surface_dims
from test_gpu_dec_surface import bind as bind_surface
from test_gpu_dec_surface import forms as uv_forms
from test_gpu_enc_rgb import bind as bind_enc
from test_gpu_enc_surface import SURFACE
from test_gpu_formats import FMT

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

ORDER = {"bgra": Q.BGRA, "rgba": Q.RGBA}
CSC_IDS = ["bt601", "bt709", "bt601_full", "bt709_full"]


def bind(hip):
    bind_surface(hip)
    hip.dsv2hip_dec_rgb_stats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    hip.dsv2hip_dec_rgb_stats.restype = None
    return hip


def rgb_forms(hip, reset=False):
    out = (C.c_ulonglong * 2)()
    hip.dsv2hip_dec_rgb_stats(out, int(reset))
    return out[0], out[1]


def reset_forms(hip):
    rgb_forms(hip, reset=True)
    uv_forms(hip, reset=True)


def is_rgb(layout):
    return (layout & ~0x300) in (Q.BGRA, Q.RGBA)


def tight(rb):
    return rb


def plus1(rb):
    return rb + 1


def aligned(rb):
    return (rb + 15) // 16 * 16 + 16


def fixed(pitch):
    return lambda rb: pitch


class OutSurf:
    """One decoder's surface of any layout: per plane a tensor of LEAD guard bytes, `offset` more, rows pitch(row bytes) apart (the
    last one without padding), LEAD guard bytes; cap[c] is exactly what the rows need.  (test_gpu_dec_surface.Surf with the pitch
    as a function.)"""

    def __init__(self, dims, layout, pitch, offset=0):
        self.layout, self.dims = layout, [d for d in dims if d[1]]
        self.c = OUTSURF()
        self.c.layout = layout
        self.t, self.inside, self.start, self.pitches = [], [], LEAD + offset, []
        for i, (rb, rows) in enumerate(self.dims):
            p = pitch(rb)
            need = (rows - 1) * p + rb
            t = torch.empty(self.start + need + LEAD, dtype=torch.uint8, device="cuda")
            assert t.data_ptr() % 16 == 0
            mask = np.zeros(t.numel(), dtype=bool)
            for y in range(rows):
                mask[self.start + y * p:self.start + y * p + rb] = True
            self.t.append(t)
            self.inside.append(mask)
            self.pitches.append(p)
            self.c.plane[i], self.c.pitch[i], self.c.cap[i] = t.data_ptr() + self.start, p, need

    def arm(self):
        for t in self.t:
            t.fill_(GUARD)

    def planes(self):
        """the delivered planes; asserts that every byte outside the rows -- in front of plane[0], between the rows, behind the last
        row -- still holds the guard value"""
        out = []
        for t, mask, (rb, rows), p in zip(self.t, self.inside, self.dims, self.pitches):
            a = t.cpu().numpy()
            assert np.all(a[~mask] == GUARD), "bytes outside the rows were written"
            out.append(np.stack([a[self.start + y * p:self.start + y * p + rb] for y in range(rows)]))
        return out

    def untouched(self):
        return all(bool(torch.all(t == GUARD)) for t in self.t)


def expected_dims(md, layout):
    if is_rgb(layout):
        return [(4 * md.width, md.height), (0, 0), (0, 0)]
    hs, vs = A.format_shifts(md.subsamp)
    cw, ch = (md.width + (1 << hs) - 1) >> hs, (md.height + (1 << vs) - 1) >> vs
    return [(md.width, md.height), (2 * cw, ch), (0, 0)] if layout == SEMI else [(md.width, md.height), (cw, ch), (cw, ch)]


def decode_steps(hip, streams, specs, modes=None, sharp=None):
    """Lockstep steps over one decoder per stream, pictures delivered into surfaces: spec = dict(layout, pitch, offset) per stream,
    any layout.  Per stream: [(return code, frame number or None, planes or None)] per packet (test_gpu_dec_surface.surface_decode);
    an RGB surface's planes are [h x 4w bytes].  The guards are checked after every step."""
    bind(hip)
    n = len(streams)
    modes, sharp = modes or [0] * n, sharp or [False] * n
    decs = [A.DECODER() for _ in range(n)]
    surfs = [None] * n
    res = [[] for _ in range(n)]
    done = [False] * n
    for t in range(max(len(s) for s in streams)):
        live = [k for k in range(n) if t < len(streams[k]) and not done[k]]
        m = len(live)
        decp = (C.POINTER(A.DECODER) * m)(*[C.pointer(decs[k]) for k in live])
        bufs, arr, had_meta = (A.BUF * m)(), (OUTSURF * m)(), []
        for i, k in enumerate(live):
            decs[k].draw_info = modes[k]
            assert hip.dsv2hip_dec_set_postsharp(C.byref(decs[k]), int(sharp[k])) == 0
            mk_buf(hip, bufs[i], streams[k][t])
            dims = surface_dims(hip, decs[k], specs[k]["layout"])
            had_meta.append(dims is not None)
            if dims is None:
                assert decs[k].got_metadata == 0  # (its entry stays all zeros)
                continue
            assert dims == expected_dims(decs[k].vidmeta, specs[k]["layout"])
            if surfs[k] is None:
                surfs[k] = OutSurf(dims, **specs[k])
            surfs[k].arm()
            arr[i] = surfs[k].c
        fns, rets = (C.c_uint32 * m)(), (C.c_int * m)()
        torch.cuda.synchronize()  # (the guard fills run on torch's stream, the decoder on its own)
        assert hip.dsv2hip_dec_batch_surface(m, decp, bufs, arr, fns, rets) == m
        for i, k in enumerate(live):
            planes = None
            if surfs[k] is not None and had_meta[i]:
                if rets[i] == A.DEC_OK:
                    planes = surfs[k].planes()
                else:
                    assert surfs[k].untouched()
            if planes is None and rets[i] == A.DEC_OK:
                assert fns[i] == NO_FN
            res[k].append((rets[i], fns[i] if planes is not None else None, planes))
            done[k] = rets[i] == A.DEC_EOS
    for d in decs:
        hip.dsv_dec_free(C.byref(d))
    return res


@functools.lru_cache(maxsize=None)
def planar_oracle(packets, mode=0, sharp=False):
    """the same packets through another decoder of the library into a tight PLANAR surface, under the same switches (shared, never
    modified): [(return code, frame number, [Y, U, V])]"""
    got = surface_decode(A.load_hip(), [packets], [dict(layout=PLANAR, pitch="tight", offset=0)], modes=[mode], sharp=[sharp])[0]
    for _, _, pl in got:
        for p in pl or ():
            p.setflags(write=False)
    return tuple(got)


def as_rgb(results, layout, fmt):
    """planar results as the surface's one plane of h x 4w bytes"""
    _, hs, vs = FMT[fmt]
    out = []
    for code, fn, pl in results:
        if pl is not None:
            h, w = pl[0].shape
            pl = [Q.convert(pl[0], pl[1], pl[2], layout, hs, vs).reshape(h, 4 * w)]
        out.append((code, fn, pl))
    return out


def same_rgb(want, got):
    """test_gpu_dec_device_out.same_results on the one plane, with the first differing byte named; alpha is part of the comparison"""
    assert [r[:2] for r in want] == [r[:2] for r in got]
    for (_, fn, pw), (_, _, pg) in zip(want, got):
        assert (pw is None) == (pg is None)
        if pw is not None:
            assert pw[0].shape == pg[0].shape
            bad = np.argwhere(pw[0] != pg[0])
            assert bad.size == 0, "frame %d: byte %d of pixel (x=%d, y=%d) is %d, the conversion gives %d (%d bytes differ)" % (
                fn, bad[0][1] % 4, bad[0][1] // 4, bad[0][0], pg[0][tuple(bad[0])], pw[0][tuple(bad[0])], len(bad))
            assert np.all(pg[0][:, 3::4] == 255)


def rgb_equals_oracle(hip, packets, fmt, layout, pitch, offset=0, mode=0, sharp=False):
    got = decode_steps(hip, [packets], [dict(layout=layout, pitch=pitch, offset=offset)], modes=[mode], sharp=[sharp])[0]
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
@functools.lru_cache(maxsize=None)
def saturated_planes():
    """64x48 at full resolution (Y, U, V each 48 x 64): the eight corners of the YUV cube in 8x8 tiles; a ramp 0..255 of each of Y, U
    and V against the extremes of the other two (3 x 8 rows); the limited-range extremes 16 / 235 (Y) and 16 / 240 (U, V) in 8x8
    tiles; 8 rows of a smooth gradient"""
    y, u, v = (np.full((48, 64), 128, dtype=np.uint8) for _ in range(3))
    for k in range(8):
        sl = (slice(0, 8), slice(8 * k, 8 * k + 8))
        y[sl], u[sl], v[sl] = 255 * (k & 1), 255 * ((k >> 1) & 1), 255 * ((k >> 2) & 1)
        sl = (slice(32, 40), slice(8 * k, 8 * k + 8))
        y[sl], u[sl], v[sl] = (16, 235)[k & 1], (16, 240)[(k >> 1) & 1], (16, 240)[(k >> 2) & 1]
    ramp = np.arange(64) * 255 // 63
    for c, pl in enumerate((y, u, v)):
        rows = slice(8 + 8 * c, 16 + 8 * c)
        for other in (y, u, v):
            other[rows, :32], other[rows, 32:] = 0, 255
        pl[rows] = ramp
    y[40:] = np.arange(64) * 3 + 20
    u[40:] = (np.arange(8) * 20 + 30)[:, None]
    v[40:] = 220 - np.arange(64) * 3
    return y, u, v


@functools.lru_cache(maxsize=None)
def saturated_stream(fmt):
    """the picture twice (an I and a P picture), lossless, by the reference encoder; returns (packets, the planes in the format)"""
    code, hs, vs = FMT[fmt]
    y, u, v = saturated_planes()
    planes = (y, np.ascontiguousarray(u[::1 << vs, ::1 << hs]), np.ascontiguousarray(v[::1 << vs, ::1 << hs]))
    frame = b"".join(p.tobytes() for p in planes)
    packets = tuple(encode_stream(A.load_ref(), [frame, frame], 64, 48, code, eos=True, qp=100, gop=12)[0])
    packet_bound_holds(packets, 64, 48, code)
    return packets, planes


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
    got = decode_steps(hip, [packets], [spec])[0]
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
    got = decode_steps(hip, streams, specs)
    # CIF: 9 rounds with two aligned RGB surfaces each; 354x290: 3 rounds with an RGB surface at an odd address
    assert rgb_forms(hip) == (9, 3)
    assert uv_forms(hip)[0] == 9
    for k, (pk, spec, fmt) in enumerate(zip(streams, specs, fmts)):
        alone = decode_steps(hip, [pk], [spec])[0]
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
    ref, hip = A.load_ref(), bind_enc(bind(A.load_hip()))
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
