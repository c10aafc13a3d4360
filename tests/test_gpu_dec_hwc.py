"""Decoded pictures delivered as interleaved [h, w, 3] RGB / BGR tensors (dsv2hip_dec_batch_hwc / dsv2hip_dec_hwc_frame /
dsv2hip_dec_hwc_dims): uint8, binary16, bfloat16 and binary32 elements hold exactly the oracle tests/hwc_out.py -- THE CONVERSION, THE
RESAMPLING and the float contract of include/dsv2_hip.h in numpy, interleaved -- of the library's own PLANAR delivery of the same packets
under the same switches (which the existing tests pin to the reference decoder), bit for bit: both forms of k_egress_hwc, both orders,
the five chroma formats, rows of several passes, content that reaches both clamps, sized tensors, draw_info and postsharp, types,
orders, sizes, constants and geometries mixed in one step with either parser; no byte outside the rows is written, a refused call
touches nothing, the statistics count what the header says, the library's BGRA / RGBA surfaces and planar tensors say the same, and a
uint8 BGR tensor feeds the encoder as a DSV2HIP_SURFACE_BGR surface without a host copy."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsvabi as A
import rgb3_csc as R3
import tensor_out as T
import yuv_rgb as Q
from codec_run import FMT, configure_encoder, encode_stream
from dec_out import (Surfaces, Tensors, aligned, decode_steps, format_stream, npics, planar_oracle, plus1, reference, saturated_stream, stream,
                     tensor_expected, tight)
from hipabi import (SURFACE, dec_resize_forms as resize_forms, dec_rgb_forms as rgb_forms, dec_tensor_forms as tensor_forms, mk_buf,
                    reset_dec_forms)
from hwc_out import BGR, ORDER_NAMES, ORDERS, OUTHWC, RGB, Hwc, OutHwc, bind, hwc_dims, hwc_expected as expected, hwc_forms, same, spec

pytestmark = [pytest.mark.gpu]

DECP = C.POINTER(A.DECODER)
CONSTS = {T.U8: T.UNIT, T.F16: T.IMAGENET, T.BF16: T.IMAGENET, T.F32: T.IMAGENET}


def reset_forms(hip):
    reset_dec_forms(hip)
    hwc_forms(hip, reset=True)


def lib():
    return bind(A.load_hip())


def equals_oracle(hip, packets, fmt, specs, mode=0, sharp=False, single=False, against_reference=False):
    """one decoder per spec, all on the same packets, in one step sequence, against the library's planar delivery (and the reference
    decoder's pictures where asked)"""
    n = len(specs)
    to = Hwc(specs)
    got = decode_steps(hip, [packets] * n, to, modes=[mode] * n, sharp=[sharp] * n, single=single)
    own = planar_oracle(packets, mode, sharp)
    for k, sp in enumerate(specs):
        what = "%s %s %s" % (T.NAMES[sp["dtype"]], ORDER_NAMES[sp["order"]], fmt)
        same(expected(own, fmt, sp), got[k], what)
        if against_reference:
            same(expected(reference(packets, mode, sharp), fmt, sp), got[k], what + " (reference)")
    return own, got, to.held


# ---- 1. both forms, every element type, both orders, every format ---------------------------------------------------------------------
# wide at 16x16 and 36x20, general at 34x18 with a pitch of one element more and the pointer one element off; 4:1:1 and "4:1:0" at 38x22,
# where the reference encoder that makes the streams does not divide by zero (tests/test_gpu_dec_tensor.py)
GENERAL_SIZE = {"444": (34, 18), "422": (34, 18), "420": (34, 18), "411": (38, 22), "410": (38, 22)}


@pytest.mark.parametrize("order", ORDERS, ids=[ORDER_NAMES[o] for o in ORDERS])
@pytest.mark.parametrize("form", ["wide16x16", "wide36x20", "general"])
@pytest.mark.parametrize("k,fmt", list(enumerate(sorted(FMT))), ids=sorted(FMT))
def test_every_element_type_order_and_format(k, fmt, form, order):
    """four decoders in lockstep on one stream (I and P pictures), one per element type, each preset in turn"""
    hip = lib()
    w, h = {"wide16x16": (16, 16), "wide36x20": (36, 20)}.get(form, GENERAL_SIZE[fmt])
    packets = format_stream(fmt, w, h, 3)
    wide = form != "general"
    specs = [spec(dt, order, Q.CSC[(k + dt) % 4], aligned if wide and dt & 1 else tight if wide else plus1, 0 if wide else 1, CONSTS[dt])
             for dt in T.DTYPES]
    reset_forms(hip)
    own, got, held = equals_oracle(hip, packets, fmt, specs)
    assert npics(own) == 3 and all(npics(g) == 3 for g in got)
    assert all(t.wide() == wide for t in held)
    assert hwc_forms(hip) == ((3, 0) if wide else (0, 3))
    assert tensor_forms(hip) == (0, 0) and rgb_forms(hip) == (0, 0) and resize_forms(hip) == (0, 0)


# ---- 2. a row longer than one pass of the workgroup -----------------------------------------------------------------------------------
def test_rows_of_more_than_one_pass():
    """516x130 (two full passes of 256 pixels and a third of four; h % 4 == 2) in every element type, wide and general (a pitch of
    one element more), against the library's planar delivery and the reference decoder"""
    hip = lib()
    packets = format_stream("420", 516, 130, 2)
    reset_forms(hip)
    equals_oracle(hip, packets, "420", [spec(dt, RGB if dt & 1 else BGR, Q.BT709, tight, 0, CONSTS[dt]) for dt in T.DTYPES], against_reference=True)
    assert hwc_forms(hip) == (2, 0)
    equals_oracle(hip, packets, "420", [spec(dt, BGR if dt & 1 else RGB, Q.FULL, plus1, 0, CONSTS[dt]) for dt in T.DTYPES], against_reference=True)
    assert hwc_forms(hip) == (2, 2)


# ---- 3. saturation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["444", "420"])
def test_saturated_content_reaches_both_clamps(fmt):
    hip = lib()
    packets, planes = saturated_stream(fmt)
    specs = [spec(T.U8, ORDERS[i % 2], csc) for i, csc in enumerate(Q.CSC)] + [
        spec(T.F16, BGR, Q.BT601, consts=T.HUGE), spec(T.F16, RGB, Q.FULL, consts=T.TINY), spec(T.F32, BGR, Q.BT709, consts=T.IMAGENET)]
    own, got, _ = equals_oracle(hip, packets, fmt, specs, against_reference=True)
    assert all(np.array_equal(a, b) for _, _, pl in own if pl is not None for a, b in zip(pl, planes))  # (lossless: the synthetic picture)
    for k in range(4):  # both clamps are at work in every channel under every preset
        assert all(p[..., e].min() == 0 and p[..., e].max() == 255 for _, _, p in got[k] if p is not None for e in range(3))
    assert any(np.any(p == 0x7c00) for _, _, p in got[4] if p is not None)  # binary16 infinity
    assert any(np.any((p > 0) & (p < 0x0400)) for _, _, p in got[5] if p is not None)  # binary16 subnormals


# ---- 4. sized tensors -----------------------------------------------------------------------------------------------------------------
SIZED = [(34, 18, 17, 9), (34, 18, 33, 17), (34, 18, 5, 3), (64, 48, 24, 24)]


@pytest.mark.parametrize("w,h,ow,oh", SIZED, ids=["%dx%d-%dx%d" % s for s in SIZED])
def test_sized_tensors(w, h, ow, oh):
    """THE CONVERSION of the planes resampled by THE RESAMPLING, u8 and f16 in both orders; the resampling counts as any sized picture's"""
    hip = lib()
    packets = format_stream("420", w, h, 3)
    specs = [spec(T.U8, BGR, Q.BT709, plus1, 1, size=(ow, oh)), spec(T.U8, RGB, Q.BT601, tight, 0, size=(ow, oh)),
             spec(T.F16, RGB, Q.FULL, aligned if ow % 4 == 0 else tight, 0, T.IMAGENET, size=(ow, oh)),
             spec(T.F16, BGR, Q.BT709 | Q.FULL, plus1, 0, T.IMAGENET, size=(ow, oh))]
    reset_forms(hip)
    own, got, _ = equals_oracle(hip, packets, "420", specs)
    assert npics(own) == 3 and all(p.shape == (oh, ow, 3) for g in got for _, _, p in g if p is not None)
    assert sum(resize_forms(hip)) == 3 and sum(hwc_forms(hip)) == 3 and rgb_forms(hip) == (0, 0) and tensor_forms(hip) == (0, 0)


def test_own_size_is_the_plain_delivery():
    """a sized entry at the picture's own size equals the plain one and counts in no resize statistic; dsv2hip_dec_hwc_frame is the
    batch call for one decoder"""
    hip = lib()
    packets = format_stream("420", 34, 18, 3)
    reset_forms(hip)
    _, got, _ = equals_oracle(hip, packets, "420", [spec(T.F32, BGR, Q.BT709, consts=T.IMAGENET), spec(T.F32, BGR, Q.BT709, consts=T.IMAGENET, size=(34, 18))])
    same(got[0], got[1])
    assert resize_forms(hip) == (0, 0) and sum(hwc_forms(hip)) == 3
    _, one, _ = equals_oracle(hip, packets, "420", [spec(T.F32, BGR, Q.BT709, consts=T.IMAGENET, size=(34, 18))], single=True)
    same(got[0], one[0])
    assert resize_forms(hip) == (0, 0) and tensor_forms(hip) == (0, 0)


# ---- 5. draw_info and postsharp -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [None, (44, 23)], ids=["full", "sized"])
@pytest.mark.parametrize("mode,sharp", [(7, False), (0, True), (7, True)], ids=["draw_info", "postsharp", "both"])
def test_draw_info_and_postsharp(mode, sharp, size):
    """both act on the full-size luma before everything else, as on the planar picture of the same decoder settings"""
    hip = lib()
    packets = stream(66, 34, "420", 4, 4)
    specs = [spec(T.U8, BGR, Q.BT601, plus1, 1, size=size), spec(T.BF16, RGB, Q.BT709 | Q.FULL, tight, 0, T.IMAGENET, size=size)]
    own, got, _ = equals_oracle(hip, packets, "420", specs, mode=mode, sharp=sharp)
    plain = planar_oracle(packets)
    assert npics(own) == 4
    assert all(not np.array_equal(a[2][0], b[2][0]) for a, b in zip(plain, own) if a[2] is not None)  # (the switches are at work)
    _, again, _ = equals_oracle(hip, packets, "420", specs)  # nothing of the switches stays in the library
    assert any(not np.array_equal(a[2], b[2]) for a, b in zip(got[0], again[0]) if a[2] is not None)


# ---- 6. only the rows are written -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES, ids=[T.NAMES[d] for d in T.DTYPES])
def test_only_the_rows_are_written(dtype):
    """The allocation is 0xA5 throughout before every step.  Afterwards the bytes in front of data, the padding of every row and the
    bytes behind the last row still are (OutHwc.planes, after every step), in the general form (a pitch of one element more, one
    element off) and in the wide one (an aligned pitch with padding)."""
    hip = lib()
    packets = format_stream("420", 36, 20, 2)
    _, got, held = equals_oracle(hip, packets, "420", [spec(dtype, BGR, Q.FULL, plus1, 1, CONSTS[dtype]), spec(dtype, RGB, Q.FULL, aligned, 0, CONSTS[dtype])])
    assert [t.wide() for t in held] == [False, True]
    assert [t.p > t.rb for t in held] == [True, True]
    assert all(p.shape == (20, 36, 3) for g in got for _, _, p in g if p is not None)


# ---- 7. the library's own paths say the same --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["wide", "general"])
def test_equals_the_four_byte_surfaces_and_the_planar_tensors(geometry):
    """U8 BGR / RGB are bytes 0..2 of the BGRA / RGBA surface of the same packets; every element type is the planar tensor of the same
    packets, constants and size, transposed, the constants permuted with the order"""
    hip = lib()
    w, h, pitch, off = (36, 20, aligned, 0) if geometry == "wide" else (34, 18, plus1, 1)
    packets = format_stream("420", w, h, 3)
    csc = Q.BT709
    hw = decode_steps(hip, [packets] * 2, Hwc([spec(T.U8, BGR, csc, pitch, off), spec(T.U8, RGB, csc, pitch, off)]))
    four = decode_steps(hip, [packets] * 2, Surfaces([dict(layout=Q.BGRA | csc, pitch=tight, offset=0), dict(layout=Q.RGBA | csc, pitch=tight, offset=0)]))
    for k in range(2):
        assert npics(hw[k]) == 3 and [r[:2] for r in hw[k]] == [r[:2] for r in four[k]]
        for (_, _, p), (_, _, s) in zip(hw[k], four[k]):
            if p is not None:
                assert np.array_equal(p, s[0].reshape(h, w, 4)[..., :3])
    consts = T.IMAGENET
    for dt in T.DTYPES:
        for order in ORDERS:
            ch = (0, 1, 2) if order == RGB else (2, 1, 0)
            mine = [None] * 3
            for e in range(3):
                mine[e] = (consts[0][ch[e]], consts[1][ch[e]])
            by_pos = (tuple(m[0] for m in mine), tuple(m[1] for m in mine))
            size = (17, 9) if dt == T.F16 else None
            got = decode_steps(hip, [packets], Hwc([spec(dt, order, csc, pitch, off, by_pos, size=size)]))[0]
            planar = decode_steps(hip, [packets], Tensors([dict(dtype=dt, csc=csc, pitch=tight, offset=0, consts=consts, size=size)]))[0]
            assert [r[:2] for r in got] == [r[:2] for r in planar]
            for (_, _, p), (_, _, q) in zip(got, planar):
                if p is not None:
                    assert np.array_equal(p, np.stack([q[ch[e]] for e in range(3)], axis=-1)), (T.NAMES[dt], ORDER_NAMES[order])


# ---- 8. torch tensors written in place --------------------------------------------------------------------------------------------------
def test_torch_tensors_are_written_in_place():
    """contiguous uint8 [h, w, 3] in both orders, bfloat16 [h, w, 3] and a float32 [1, 3, h, w] tensor in channels_last, read back
    through torch as integers of the element's width"""
    hip = lib()
    w, h = 36, 20
    packets = format_stream("420", w, h, 2)
    own = planar_oracle(packets)
    cases = [(T.U8, BGR, torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda"), torch.uint8),
             (T.U8, RGB, torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda"), torch.uint8),
             (T.BF16, RGB, torch.zeros((h, w, 3), dtype=torch.bfloat16, device="cuda"), torch.int16),
             (T.F32, RGB, torch.zeros((1, 3, h, w), dtype=torch.float32, device="cuda").to(memory_format=torch.channels_last), torch.int32)]
    reset_forms(hip)
    for dt, order, t, itype in cases:
        assert t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)
        c = OUTHWC()
        c.data, c.pitch, c.cap = t.data_ptr(), 3 * w * T.ELEM[dt], t.numel() * t.element_size()
        c.dtype, c.order, c.csc = dt, order, Q.BT709
        for k in range(3):
            c.scale[k], c.bias[k] = T.IMAGENET[0][k], T.IMAGENET[1][k]
        torch.cuda.synchronize()
        dec, last = A.DECODER(), None
        for pk in packets:
            buf, fn = A.BUF(), C.c_uint32(0)
            mk_buf(hip, buf, pk)
            had_meta = dec.got_metadata
            code = hip.dsv2hip_dec_hwc_frame(C.byref(dec), C.byref(buf), C.byref(c), C.byref(fn))
            if code == A.DEC_OK and had_meta:
                last = fn.value
        hip.dsv_dec_free(C.byref(dec))
        pl = next(p for code, fn, p in own if p is not None and fn == last)
        want = expected([(A.DEC_OK, last, pl)], "420", spec(dt, order, Q.BT709, consts=T.IMAGENET))[0][2]
        if t.dim() == 4:  # channels_last [1, 3, h, w]: [h, w, 3] in memory, read as such through torch
            got = t.permute(0, 2, 3, 1)[0].contiguous().view(itype).cpu().numpy().view(T.BITS[dt])
        else:
            got = t.view(itype).cpu().numpy().view(T.BITS[dt])
        assert np.array_equal(got, want), (T.NAMES[dt], ORDER_NAMES[order])
        if dt != T.U8:
            assert torch.isfinite(t.float()).all() and float(t.float().abs().max()) < 3.0
    assert hwc_forms(hip) == (2 * len(cases), 0)  # (two pictures each, one decoder a round)


# ---- 9. one mixed step ----------------------------------------------------------------------------------------------------------------
def mixed_step(hip):
    a, b = format_stream("420", 34, 18, 3), format_stream("444", 36, 20, 3)
    streams = [a, a, a, b, b, a]
    fmts = ["420", "420", "420", "444", "444", "420"]
    specs = [spec(T.U8, BGR, Q.BT601, plus1, 1),
             spec(T.F16, RGB, Q.BT709, tight, 0, T.IMAGENET),
             spec(T.BF16, BGR, Q.FULL, aligned, 0, T.HUGE, size=(17, 9)),
             spec(T.F32, RGB, Q.BT709 | Q.FULL, tight, 0, T.IMAGENET),   # the second geometry: a round of its own, in the wide form
             spec(T.F16, BGR, Q.BT601, aligned, 0, T.TINY, size=(24, 12)),
             spec(T.F32, BGR, Q.BT709, plus1, 3, T.UNIT)]                # a late joiner
    delay = [0, 0, 0, 0, 0, 2]
    reset_forms(hip)
    got = decode_steps(hip, streams, Hwc(specs), delay=delay)
    assert hwc_forms(hip)[0] == 3  # 36x20: three rounds of aligned tensors; 34x18 (w % 4 == 2): always the general form
    assert hwc_forms(hip)[1] >= 3 and tensor_forms(hip) == (0, 0) and rgb_forms(hip) == (0, 0)
    for k, (pk, sp, fmt) in enumerate(zip(streams, specs, fmts)):
        same(expected(planar_oracle(pk), fmt, sp), got[k], "decoder %d" % k)
        alone = decode_steps(hip, [pk], Hwc([sp]))
        same(alone[0], got[k], "decoder %d alone" % k)


def test_mixed_types_orders_sizes_constants_and_geometries_in_one_step():
    mixed_step(lib())


def test_mixed_types_orders_sizes_constants_and_geometries_in_one_step_device_parser():
    hip = lib()
    try:
        assert hip.dsv2hip_dec_set_parse_mode(2) == 2
        mixed_step(hip)
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)


# ---- 10. dsv2hip_dec_hwc_dims ---------------------------------------------------------------------------------------------------------
def test_hwc_dims():
    hip = lib()
    assert hwc_dims(hip, None, T.U8) is None
    dec = A.DECODER()
    assert hwc_dims(hip, dec, T.F32) is None  # no metadata yet
    buf, fn = A.BUF(), C.c_uint32(0)
    mk_buf(hip, buf, format_stream("420", 34, 18, 3)[0])
    assert hip.dsv2hip_dec_hwc_frame(C.byref(dec), C.byref(buf), C.byref(OUTHWC()), C.byref(fn)) == A.DEC_GOT_META
    for dt in T.DTYPES:
        e = T.ELEM[dt]
        assert hwc_dims(hip, dec, dt) == (3 * 34 * e, 18)
        for ow, oh in [(17, 9), (33, 17), (5, 3), (34, 18), (34, 3), (5, 18)]:
            assert hwc_dims(hip, dec, dt, ow, oh) == (3 * ow * e, oh)
        for ow, oh in [(17, 0), (0, 9), (35, 18), (34, 19), (4, 3), (5, 2), (-17, 9)]:
            assert hwc_dims(hip, dec, dt, ow, oh) is None, (ow, oh)
    for dt in (-1, 4, 0x20):
        assert hwc_dims(hip, dec, dt) is None
    rb, rows = C.c_size_t(0), C.c_int(0)
    assert hip.dsv2hip_dec_hwc_dims(C.byref(dec), T.U8, 0, 0, None, C.byref(rows)) == -1
    assert hip.dsv2hip_dec_hwc_dims(C.byref(dec), T.U8, 0, 0, C.byref(rb), None) == -1
    assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 1) == 0
    assert hwc_dims(hip, dec, T.U8) is None and hwc_dims(hip, dec, T.F16, 17, 9) is None
    assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 0) == 0
    assert hwc_dims(hip, dec, T.U8) == (3 * 34, 18)
    hip.dsv_dec_free(C.byref(dec))


# ---- 11. refusals touch nothing -------------------------------------------------------------------------------------------------------
def set_field(name, value):
    def f(c):
        setattr(c, name, value(getattr(c, name)) if callable(value) else value)
    return f


def set_item(name, k, value):
    def f(c):
        getattr(c, name)[k] = value
    return f


ROW = 3 * 34 * 4  # the row bytes of the refused tensor: binary32, 34 pixels
REFUSALS = [("unknown_dtype", set_field("dtype", 4)),
            ("negative_dtype", set_field("dtype", -1)),
            ("order_rgbp", set_field("order", 0x22)),
            ("order_bgra", set_field("order", 0x10)),
            ("order_rgba", set_field("order", 0x11)),
            ("order_with_csc_bits", set_field("order", 0x20 | 0x100)),
            ("order_zero", set_field("order", 0)),
            ("csc_bit_outside", set_field("csc", 0x400)),
            ("csc_layout_bits", set_field("csc", 0x100 | 0x21)),
            ("null_data", set_field("data", None)),
            ("data_off_the_element", set_field("data", lambda p: p + 2)),
            ("pitch_off_the_element", lambda c: (set_field("pitch", lambda p: p + 2)(c), set_field("cap", lambda v: v + 2 * 17)(c))),  # (cap holds the rows)
            ("pitch_short", set_field("pitch", ROW - 4)),
            ("pitch_beyond_int", lambda c: (set_field("pitch", (1 << 31) + 4)(c), set_field("cap", 1 << 40)(c))),
            ("cap_short", set_field("cap", lambda v: v - 1)),
            ("scale_infinite", set_item("scale", 0, float("inf"))),
            ("scale_nan", set_item("scale", 2, float("nan"))),
            ("bias_infinite", set_item("bias", 1, float("-inf"))),
            ("bias_nan", set_item("bias", 0, float("nan"))),
            ("one_size_zero_w", set_field("out_w", 17)),
            ("one_size_zero_h", set_field("out_h", 9)),
            ("enlargement", lambda c: (setattr(c, "out_w", 35), setattr(c, "out_h", 18))),
            ("below_an_eighth", lambda c: (setattr(c, "out_w", 4), setattr(c, "out_h", 3))),
            ("negative_size", lambda c: (setattr(c, "out_w", -17), setattr(c, "out_h", 9)))]


def test_refused_calls_touch_nothing():
    """Every refusal of the header, one case each, the spoiled entry SECOND in a step of two: -1 from the batch and the one-decoder
    call, with the packets, the decoders' bytes, fn / ret and the tensors as they were; the same packets then decode to the oracle's
    pictures."""
    hip = lib()
    packets = format_stream("420", 34, 18, 3)
    sp = spec(T.F32, BGR, Q.BT709, plus1, 0, T.IMAGENET)
    want = expected(planar_oracle(packets), "420", sp)
    decs = [A.DECODER(), A.DECODER()]
    decp = (DECP * 2)(*[C.pointer(d) for d in decs])
    fns, rets = (C.c_uint32 * 2)(), (C.c_int * 2)()
    bufs, arr = (A.BUF * 2)(), (OUTHWC * 2)()
    for i in range(2):  # no metadata yet: anything may be passed (here: entries that are all zeros but for an unknown dtype)
        mk_buf(hip, bufs[i], packets[0])
        arr[i].dtype = 99
    assert hip.dsv2hip_dec_batch_hwc(2, decp, bufs, arr, fns, rets) == 2
    assert list(rets) == [A.DEC_GOT_META] * 2
    held = [OutHwc(hwc_dims(hip, d, T.F32), **sp) for d in decs]
    assert held[1].rb == ROW
    for t in held:
        t.arm()
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
        assert all(t.untouched() for t in held)

    def refused(what):
        for i in range(2):
            fns[i], rets[i] = 77, -5
        assert hip.dsv2hip_dec_batch_hwc(2, decp, bufs, arr, fns, rets) == -1, what
        one_fn = C.c_uint32(77)
        assert hip.dsv2hip_dec_hwc_frame(C.byref(decs[1]), C.byref(bufs[1]), C.byref(arr[1]), C.byref(one_fn)) == -1, what
        assert one_fn.value == 77
        nothing_happened()

    arr[0] = held[0].c
    for what, spoil in REFUSALS:
        C.memmove(C.byref(arr[1]), C.byref(held[1].c), C.sizeof(OUTHWC))
        spoil(arr[1])
        refused(what)
    # an -out420p decoder takes no interleaved tensor; the switch off again, it does
    arr[1] = held[1].c
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 1) == 0
    state[1] = bytes(C.string_at(C.byref(decs[1]), C.sizeof(decs[1])))  # (the switch may have made the decoder's private part)
    refused("out420p")
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 0) == 0
    for bad in (dict(n=0), dict(decs=None), dict(bufs=None), dict(t=None), dict(fn=None), dict(ret=None)):
        args = dict(n=2, decs=decp, bufs=bufs, t=arr, fn=fns, ret=rets)
        args.update(bad)
        for i in range(2):
            fns[i], rets[i] = 77, -5
        assert hip.dsv2hip_dec_batch_hwc(args["n"], args["decs"], args["bufs"], args["t"], args["fn"], args["ret"]) == -1, bad
        nothing_happened()
    # the same packets, the good tensors: decoded as if nothing had happened, and on to the end of the stream
    got = [[(A.DEC_GOT_META, None, None)] for _ in range(2)]
    for t in range(1, len(packets)):
        if t > 1:
            for i in range(2):
                mk_buf(hip, bufs[i], packets[t])
                held[i].arm()
            torch.cuda.synchronize()
        had_meta = [d.got_metadata for d in decs]
        assert hip.dsv2hip_dec_batch_hwc(2, decp, bufs, arr, fns, rets) == 2
        for i in range(2):
            pic = rets[i] == A.DEC_OK and had_meta[i]
            got[i].append((rets[i], fns[i] if pic else None, held[i].planes() if pic else None))
    for i in range(2):
        same(want, got[i])
        hip.dsv_dec_free(C.byref(decs[i]))


# ---- 12. uint8 ignores the constants ----------------------------------------------------------------------------------------------------
def test_uint8_tensors_ignore_the_constants():
    hip = lib()
    packets = format_stream("420", 34, 18, 3)
    junk = ((float("nan"), float("inf"), -1e30), (float("-inf"), float("nan"), 7.0))
    _, got, _ = equals_oracle(hip, packets, "420", [spec(T.U8, BGR, Q.BT709, consts=junk), spec(T.U8, BGR, Q.BT709)])
    same(got[0], got[1])


# ---- 13. the statistics ---------------------------------------------------------------------------------------------------------------
def test_statistics_count_rounds_by_form():
    hip = lib()
    packets = format_stream("420", 36, 20, 3)
    reset_forms(hip)
    equals_oracle(hip, packets, "420", [spec(T.F32, RGB, consts=T.IMAGENET), spec(T.U8, BGR)])  # two aligned tensors a round: one wide round each
    assert hwc_forms(hip) == (3, 0)
    equals_oracle(hip, packets, "420", [spec(T.F32, RGB, consts=T.IMAGENET), spec(T.U8, BGR, offset=1)])  # one of them off the grid: the round is general
    assert hwc_forms(hip) == (3, 3)
    assert rgb_forms(hip) == (0, 0) and tensor_forms(hip) == (0, 0) and resize_forms(hip) == (0, 0)
    equals_oracle(hip, packets, "420", [spec(T.F16, BGR, size=(18, 10))])
    assert hwc_forms(hip) == (3, 6) and sum(resize_forms(hip)) == 3  # (18 % 4 == 2: general; the resampling counts as any sized picture's)
    assert rgb_forms(hip) == (0, 0) and tensor_forms(hip) == (0, 0)
    assert hwc_forms(hip, reset=True) == (3, 6) and hwc_forms(hip) == (0, 0)
    hip.dsv2hip_dec_hwc_stats(None, 0)


# ---- 14. decode -> uint8 BGR tensor -> encode without the host ---------------------------------------------------------------------------
def test_uint8_bgr_tensor_goes_straight_into_the_encoder():
    """A CIF 4:2:0 stream decoded into a pitched uint8 BGR tensor whose pointer and pitch go straight to dsv2hip_enc_surface_frame as a
    DSV2HIP_SURFACE_BGR surface: the packets are the reference encoder's on the planar pictures that the encoder's conversion
    (tests/rgb3_csc.py) defines on the oracle's bytes."""
    ref, hip = A.load_ref(), lib()
    w, h, csc = 352, 288, Q.BT709
    packets = stream(w, h, "420", 3, 3)
    sp = spec(T.U8, BGR, csc, aligned, 0)
    pictures = [p for _, _, p in expected(planar_oracle(packets), "420", sp) if p is not None]
    assert len(pictures) == 3
    want = encode_stream(ref, [R3.planar_bytes(p, R3.BGR | csc, 1, 1) for p in pictures], w, h, A.SUBSAMP_420, eos=False, qp=50, gop=48)[0]
    enc, dec = A.ENCODER(), A.DECODER()
    configure_encoder(hip, enc, A.mk_meta(w, h, A.SUBSAMP_420), qp=50, gop=48)
    tn = OutHwc((3 * w, h), **sp)
    assert tn.p > 3 * w
    tn.arm()
    torch.cuda.synchronize()
    src = SURFACE()
    src.layout = R3.BGR | csc
    src.plane[0], src.pitch[0] = tn.c.data, tn.c.pitch
    got, seen = [], 0
    for pk in packets:
        buf, fn = A.BUF(), C.c_uint32(0)
        mk_buf(hip, buf, pk)
        had_meta = dec.got_metadata
        code = hip.dsv2hip_dec_hwc_frame(C.byref(dec), C.byref(buf), C.byref(tn.c), C.byref(fn))
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
        assert np.array_equal(tn.planes(), pictures[seen])  # (and the encoder wrote nothing into the tensor)
        seen += 1
    hip.dsv_enc_free(C.byref(enc))
    hip.dsv_dec_free(C.byref(dec))
    assert seen == 3 and len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a == b, "packet %d differs" % i
