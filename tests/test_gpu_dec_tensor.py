"""Decoded pictures delivered as planar RGB tensors (dsv2hip_dec_batch_tensor / dsv2hip_dec_tensor_frame / dsv2hip_dec_tensor_dims):
uint8, binary16, bfloat16 and binary32 planes R, G, B hold exactly the oracle tests/tensor_out.py -- THE CONVERSION, THE RESAMPLING
and the float contract of include/dsv2_hip.h in numpy -- of the REFERENCE decoder's planar pictures, bit for bit: both forms of
k_egress_tensor, the five chroma formats, the smallest picture, rows of several passes, content that reaches both clamps, sized
tensors, draw_info and postsharp, element types, sizes, constants and geometries mixed in one step with either parser; no byte outside
the rows is written, a refused call touches nothing, the statistics count what the header says, and a uint8 tensor feeds the encoder as
a DSV2HIP_SURFACE_RGBP surface without a host copy.  Float planes are read back through torch as integers of the element's width and
compared as bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsvabi as A
import rgb3_csc as R3
import tensor_out as T
import yuv_rgb as Q
from codec_run import FMT, configure_encoder, encode_stream
from edge_cases import stream_inverse_is_undefined
from dec_out import (OutTensor, Tensors, aligned, decode_steps, format_stream, npics, planar_oracle, plus1, reference, saturated_stream, stream,
                     tensor_expected as expected, tight)
from hipabi import (OUTTENSOR, SURFACE, bind, dec_resize_forms as resize_forms, dec_rgb_forms as rgb_forms, dec_tensor_forms as tensor_forms, mk_buf,
                    reset_dec_forms as reset_forms, sized_dims, tensor_dims)

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

DECP = C.POINTER(A.DECODER)


def spec(dtype, csc=0, pitch=tight, offset=0, consts=T.UNIT, size=None):
    """a tensor: element type, CSC bits, pitch as a function of (row bytes, element size), pointer offset in ELEMENTS behind a 16-byte
    boundary, (scale[3], bias[3]), delivered size or None"""
    return dict(dtype=dtype, csc=csc, pitch=pitch, offset=offset, consts=consts, size=size)


def same(want, got, what=""):
    assert [r[:2] for r in want] == [r[:2] for r in got], what
    for (_, fn, pw), (_, _, pg) in zip(want, got):
        assert (pw is None) == (pg is None)
        if pw is None:
            continue
        for c in range(3):
            assert pw[c].dtype == pg[c].dtype and pw[c].shape == pg[c].shape, what
            bad = np.argwhere(pw[c] != pg[c])
            assert bad.size == 0, "%s frame %d plane %d: element (x=%d, y=%d) is %#x, the oracle gives %#x (%d differ)" % (
                what, fn, c, bad[0][1], bad[0][0], pg[c][tuple(bad[0])], pw[c][tuple(bad[0])], len(bad))


def equals_reference(hip, packets, fmt, specs, mode=0, sharp=False, single=False):
    """one decoder per spec, all on the same packets, in one step sequence"""
    n = len(specs)
    to = Tensors(specs)
    got = decode_steps(hip, [packets] * n, to, modes=[mode] * n, sharp=[sharp] * n, single=single)
    ref = reference(packets, mode, sharp)
    for k, sp in enumerate(specs):
        same(expected(ref, fmt, sp), got[k], "%s %s" % (T.NAMES[sp["dtype"]], fmt))
    return ref, got, to.held


CONSTS = {T.U8: T.UNIT, T.F16: T.IMAGENET, T.BF16: T.IMAGENET, T.F32: T.IMAGENET}
# (ImageNet's pairs: a bias and scale = 1 / (255 * 0.229), which tell the two roundings of the contract from a fused multiply-add)


# ---- 1. both forms, every element type, every format --------------------------------------------------------------------------------
# wide at 16x16 and 36x20, general at 34x18 with a pitch of one element more and the pointer one element off.  4:1:1 and "4:1:0" take
# the general form at 38x22: the reference encoder, which makes the streams, divides by zero at 34x18 there (tests/test_gpu_dec_scale.py);
# w % 4 == 2 and h % 4 == 2 hold at both sizes.
GENERAL_SIZE = {"444": (34, 18), "422": (34, 18), "420": (34, 18), "411": (38, 22), "410": (38, 22)}


@pytest.mark.parametrize("form", ["wide16x16", "wide36x20", "general"])
@pytest.mark.parametrize("k,fmt", list(enumerate(sorted(FMT))), ids=sorted(FMT))
def test_every_element_type_and_format(k, fmt, form):
    """four decoders in lockstep on one stream (I and P pictures), one per element type, each preset in turn"""
    hip = bind(A.load_hip())
    w, h = {"wide16x16": (16, 16), "wide36x20": (36, 20)}.get(form, GENERAL_SIZE[fmt])
    packets = format_stream(fmt, w, h, 3)
    wide = form != "general"
    specs = [spec(dt, Q.CSC[(k + dt) % 4], aligned if wide and dt & 1 else tight if wide else plus1, 0 if wide else 1, CONSTS[dt]) for dt in T.DTYPES]
    reset_forms(hip)
    ref, got, tens = equals_reference(hip, packets, fmt, specs)
    assert npics(ref) == 3 and all(npics(g) == 3 for g in got)
    assert all(t.wide() == wide for t in tens)
    assert tensor_forms(hip) == ((3, 0) if wide else (0, 3))
    assert rgb_forms(hip) == (0, 0) and resize_forms(hip) == (0, 0)


# ---- 2. a row longer than one pass of the workgroup ---------------------------------------------------------------------------------
# 516 wide: two full passes of 256 pixels and a third of four.  At 516x16 the reference decoder's pictures are not a function of the
# packets (its inverse transform of the 8-row chroma planes reads stale scratch: tests/edge_cases.py, stream_inverse_is_undefined --
# measured here: 5228 of 8256 red samples one off), so the reference pins 516x130, the smallest such height at which it is defined
# (h % 4 == 2: the last thread rows lie half below the picture), and 516x16 is pinned to the oracle on the planar pictures the library
# itself delivers from the same packets, which the existing tests pin.
def test_rows_of_more_than_one_pass():
    """516x130 against the reference, in every element type, wide and (a pitch of one element more) general"""
    hip = bind(A.load_hip())
    assert stream_inverse_is_undefined(516, 16, A.SUBSAMP_420, dict(qp=60)) and not stream_inverse_is_undefined(516, 130, A.SUBSAMP_420, dict(qp=60))
    packets = format_stream("420", 516, 130, 2)
    reset_forms(hip)
    equals_reference(hip, packets, "420", [spec(dt, Q.BT709, tight, 0, CONSTS[dt]) for dt in T.DTYPES])
    assert tensor_forms(hip) == (2, 0)
    equals_reference(hip, packets, "420", [spec(dt, Q.FULL, plus1, 0, CONSTS[dt]) for dt in T.DTYPES])
    assert tensor_forms(hip) == (2, 2)


def test_rows_of_more_than_one_pass_one_block_high():
    """516x16 against the oracle on the library's own planar delivery"""
    hip = bind(A.load_hip())
    packets = format_stream("420", 516, 16, 2)
    own = planar_oracle(packets)
    for pitch in (tight, plus1):
        specs = [spec(dt, Q.BT709, pitch, 0, CONSTS[dt]) for dt in T.DTYPES]
        got = decode_steps(hip, [packets] * 4, Tensors(specs))
        for k, sp in enumerate(specs):
            same(expected(own, "420", sp), got[k], T.NAMES[sp["dtype"]])


# ---- 3. saturation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["444", "420"])
def test_saturated_content_reaches_both_clamps(fmt):
    hip = bind(A.load_hip())
    packets, planes = saturated_stream(fmt)
    specs = [spec(T.U8, csc) for csc in Q.CSC] + [spec(T.F16, Q.BT601, consts=T.HUGE), spec(T.F16, Q.FULL, consts=T.TINY), spec(T.F32, Q.BT709, consts=T.IMAGENET)]
    ref, got, _ = equals_reference(hip, packets, fmt, specs)
    assert all(np.array_equal(a, b) for _, _, pl in ref if pl is not None for a, b in zip(pl, planes))  # (lossless: the synthetic picture)
    for k in range(4):  # both clamps are at work in every channel under every preset
        assert all(p.min() == 0 and p.max() == 255 for _, _, pl in got[k] if pl is not None for p in pl)
    assert any(np.any(p == 0x7c00) for _, _, pl in got[4] if pl is not None for p in pl)  # binary16 infinity
    assert any(np.any((p > 0) & (p < 0x0400)) for _, _, pl in got[5] if pl is not None for p in pl)  # binary16 subnormals


# ---- 4. sized tensors ---------------------------------------------------------------------------------------------------------------
SIZED = [(34, 18, 17, 9), (34, 18, 33, 17), (34, 18, 5, 3), (64, 48, 24, 24)]


@pytest.mark.parametrize("w,h,ow,oh", SIZED, ids=["%dx%d-%dx%d" % s for s in SIZED])
def test_sized_tensors(w, h, ow, oh):
    """THE CONVERSION of the planes resampled by THE RESAMPLING, in u8 and f16; the resampling counts as any sized picture's"""
    hip = bind(A.load_hip())
    packets = format_stream("420", w, h, 3)
    specs = [spec(T.U8, Q.BT709, plus1, 1, size=(ow, oh)), spec(T.F16, Q.FULL, aligned if ow % 4 == 0 else tight, 0, T.IMAGENET, size=(ow, oh))]
    reset_forms(hip)
    ref, got, tens = equals_reference(hip, packets, "420", specs)
    assert npics(ref) == 3 and all(pl[0].shape == (oh, ow) for _, _, pl in got[0] if pl is not None)
    assert sum(resize_forms(hip)) == 3 and sum(tensor_forms(hip)) == 3 and rgb_forms(hip) == (0, 0)


def test_own_size_is_the_plain_delivery():
    """a sized entry at the picture's own size equals the plain one and counts in no resize statistic; dsv2hip_dec_tensor_frame is the
    batch call for one decoder"""
    hip = bind(A.load_hip())
    packets = format_stream("420", 34, 18, 3)
    reset_forms(hip)
    _, got, _ = equals_reference(hip, packets, "420", [spec(T.F32, Q.BT709, consts=T.IMAGENET), spec(T.F32, Q.BT709, consts=T.IMAGENET, size=(34, 18))])
    same(got[0], got[1])
    assert resize_forms(hip) == (0, 0) and sum(tensor_forms(hip)) == 3
    _, one, _ = equals_reference(hip, packets, "420", [spec(T.F32, Q.BT709, consts=T.IMAGENET, size=(34, 18))], single=True)
    same(got[0], one[0])
    assert resize_forms(hip) == (0, 0)


# ---- 5. draw_info and postsharp -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [None, (44, 23)], ids=["full", "sized"])
@pytest.mark.parametrize("mode,sharp", [(7, False), (0, True), (7, True)], ids=["draw_info", "postsharp", "both"])
def test_draw_info_and_postsharp(mode, sharp, size):
    """both act on the full-size luma before everything else, exactly as the reference draws and sharpens its own picture"""
    hip = bind(A.load_hip())
    packets = stream(66, 34, "420", 4, 4)
    specs = [spec(T.U8, Q.BT601, plus1, 1, size=size), spec(T.BF16, Q.BT709 | Q.FULL, tight, 0, T.IMAGENET, size=size)]
    ref, got, _ = equals_reference(hip, packets, "420", specs, mode=mode, sharp=sharp)
    plain = reference(packets)
    assert npics(ref) == 4
    assert all(not np.array_equal(a[2][0], b[2][0]) for a, b in zip(plain, ref) if a[2] is not None)  # (the switches are at work)
    assert all(np.array_equal(a[2][c], b[2][c]) for a, b in zip(plain, ref) if a[2] is not None for c in (1, 2))  # (in luma only)
    equals_reference(hip, packets, "420", specs)  # nothing of the switches stays in the library


# ---- 6. only the rows are written ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES, ids=[T.NAMES[d] for d in T.DTYPES])
def test_only_the_rows_are_written(dtype):
    """The allocation is 0xA5 throughout before every step.  Afterwards the bytes in front of plane[0], the padding of every row, the
    bytes between the planes and behind the last row -- which has no padding of its own -- still are (OutTensor.planes, after every
    step), in the general form (a pitch of one element more, one element off) and in the wide one (an aligned pitch with padding)."""
    hip = bind(A.load_hip())
    packets = format_stream("420", 36, 20, 2)
    _, got, tens = equals_reference(hip, packets, "420", [spec(dtype, Q.FULL, plus1, 1, CONSTS[dtype]), spec(dtype, Q.FULL, aligned, 0, CONSTS[dtype])])
    assert [t.wide() for t in tens] == [False, True]
    assert all(p.shape == (20, 36) for g in got for _, _, pl in g if pl is not None for p in pl)


def test_contiguous_torch_tensors_are_written_in_place():
    """torch [3, h, w] tensors of the four element types, planes named by pointer -- B, G, R order for one of them -- and read back as
    integers of the element's width"""
    hip = bind(A.load_hip())
    w, h = 36, 20
    packets = format_stream("420", w, h, 2)
    ref = reference(packets)
    kinds = {T.U8: (torch.uint8, torch.uint8), T.F16: (torch.float16, torch.int16), T.BF16: (torch.bfloat16, torch.int16), T.F32: (torch.float32, torch.int32)}
    reset_forms(hip)
    for dt, (ttype, itype) in kinds.items():
        t = torch.zeros((3, h, w), dtype=ttype, device="cuda")
        order = (2, 1, 0) if dt == T.F16 else (0, 1, 2)  # plane[c] = the tensor's channel order[c]
        c = OUTTENSOR()
        c.dtype, c.csc = dt, Q.BT709
        elem = T.ELEM[dt]
        for ch in range(3):
            c.plane[ch], c.pitch[ch], c.cap[ch] = t.data_ptr() + order[ch] * h * w * elem, w * elem, h * w * elem
            c.scale[ch], c.bias[ch] = T.IMAGENET[0][ch], T.IMAGENET[1][ch]
        torch.cuda.synchronize()
        dec, last = A.DECODER(), None
        for pk in packets:
            buf, fn = A.BUF(), C.c_uint32(0)
            mk_buf(hip, buf, pk)
            had_meta = dec.got_metadata
            code = hip.dsv2hip_dec_tensor_frame(C.byref(dec), C.byref(buf), C.byref(c), C.byref(fn))
            if code == A.DEC_OK and had_meta:
                last = fn.value
        hip.dsv_dec_free(C.byref(dec))
        pl = next(p for code, fn, p in ref if p is not None and fn == last)
        want = T.tensor(pl[0], pl[1], pl[2], Q.BT709, 1, 1, dt, *T.IMAGENET)
        got = t.view(itype).cpu().numpy().view(T.BITS[dt])
        for ch in range(3):
            assert np.array_equal(got[order[ch]], want[ch]), (T.NAMES[dt], ch)
        if dt != T.U8:  # the values are the normalised picture, as torch reads them
            assert torch.isfinite(t).all() and float(t.float().abs().max()) < 3.0
    assert tensor_forms(hip) == (8, 0)


# ---- 7. one mixed step --------------------------------------------------------------------------------------------------------------
def mixed_step(hip):
    a, b = format_stream("420", 34, 18, 3), format_stream("444", 36, 20, 3)
    streams = [a, a, a, b, b, a]
    fmts = ["420", "420", "420", "444", "444", "420"]
    specs = [spec(T.U8, Q.BT601, plus1, 1),
             spec(T.F16, Q.BT709, tight, 0, T.IMAGENET),
             spec(T.BF16, Q.FULL, aligned, 0, T.HUGE, size=(17, 9)),
             spec(T.F32, Q.BT709 | Q.FULL, tight, 0, T.IMAGENET),   # the second geometry: a round of its own, in the wide form
             spec(T.F16, Q.BT601, aligned, 0, T.TINY, size=(24, 12)),
             spec(T.F32, Q.BT709, plus1, 3, T.UNIT)]                # a late joiner
    delay = [0, 0, 0, 0, 0, 2]
    reset_forms(hip)
    got = decode_steps(hip, streams, Tensors(specs), delay=delay)
    assert tensor_forms(hip)[0] == 3  # 36x20: three rounds of aligned tensors; 34x18 (w % 4 == 2): always the general form
    assert tensor_forms(hip)[1] >= 3 and rgb_forms(hip) == (0, 0)
    for k, (pk, sp, fmt) in enumerate(zip(streams, specs, fmts)):
        same(expected(reference(pk), fmt, sp), got[k], "decoder %d" % k)
        alone = decode_steps(hip, [pk], Tensors([sp]))
        same(alone[0], got[k], "decoder %d alone" % k)


def test_mixed_types_sizes_constants_and_geometries_in_one_step():
    mixed_step(bind(A.load_hip()))


def test_mixed_types_sizes_constants_and_geometries_in_one_step_device_parser():
    hip = bind(A.load_hip())
    try:
        assert hip.dsv2hip_dec_set_parse_mode(2) == 2
        mixed_step(hip)
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)


# ---- 8. dsv2hip_dec_tensor_dims -----------------------------------------------------------------------------------------------------
def test_tensor_dims():
    hip = bind(A.load_hip())
    assert tensor_dims(hip, None, T.U8) is None
    dec = A.DECODER()
    assert tensor_dims(hip, dec, T.F32) is None  # no metadata yet
    buf, fn = A.BUF(), C.c_uint32(0)
    mk_buf(hip, buf, format_stream("420", 34, 18, 3)[0])
    assert hip.dsv2hip_dec_tensor_frame(C.byref(dec), C.byref(buf), C.byref(OUTTENSOR()), C.byref(fn)) == A.DEC_GOT_META
    for dt in T.DTYPES:
        e = T.ELEM[dt]
        assert tensor_dims(hip, dec, dt) == (34 * e, 18)
        for ow, oh in [(17, 9), (33, 17), (5, 3), (34, 18), (34, 3), (5, 18)]:
            assert tensor_dims(hip, dec, dt, ow, oh) == (ow * e, oh)
            assert sized_dims(hip, dec, Q.RGBA, ow, oh) == [(4 * ow, oh), (0, 0), (0, 0)]  # (the RGB surface's sizes, as the header says)
        for ow, oh in [(17, 0), (0, 9), (35, 18), (34, 19), (4, 3), (5, 2), (-17, 9)]:
            assert tensor_dims(hip, dec, dt, ow, oh) is None, (ow, oh)
    for dt in (-1, 4, 0x22):
        assert tensor_dims(hip, dec, dt) is None
    rb, rows = C.c_size_t(0), C.c_int(0)
    assert hip.dsv2hip_dec_tensor_dims(C.byref(dec), T.U8, 0, 0, None, C.byref(rows)) == -1
    assert hip.dsv2hip_dec_tensor_dims(C.byref(dec), T.U8, 0, 0, C.byref(rb), None) == -1
    assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 1) == 0  # an RGB picture has no chroma planes to subsample
    assert tensor_dims(hip, dec, T.U8) is None and tensor_dims(hip, dec, T.F16, 17, 9) is None
    assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 0) == 0
    assert tensor_dims(hip, dec, T.U8) == (34, 18)
    hip.dsv_dec_free(C.byref(dec))


# ---- 9. refusals touch nothing ------------------------------------------------------------------------------------------------------
def set_field(name, value):
    def f(c):
        setattr(c, name, value)
    return f


def set_item(name, k, value):
    def f(c):
        getattr(c, name)[k] = value(getattr(c, name)[k]) if callable(value) else value
    return f


REFUSALS = [("unknown_dtype", set_field("dtype", 4)),
            ("negative_dtype", set_field("dtype", -1)),
            ("csc_bit_outside", set_field("csc", 0x400)),
            ("csc_layout_bits", set_field("csc", 0x100 | 0x11)),
            ("null_plane", set_item("plane", 1, None)),
            ("plane_off_the_element", set_item("plane", 2, lambda p: p + 1)),
            ("pitch_off_the_element", lambda c: (set_item("pitch", 0, lambda p: p + 2)(c), set_item("cap", 0, lambda v: v + 2 * 17)(c))),  # (cap holds the rows)
            ("pitch_short", set_item("pitch", 1, lambda p: 34 * 4 - 4)),
            ("pitch_beyond_int", lambda c: (set_item("pitch", 0, (1 << 31) + 4)(c), set_item("cap", 0, 1 << 40)(c))),
            ("cap_short", set_item("cap", 2, lambda v: v - 1)),
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
    hip = bind(A.load_hip())
    packets = format_stream("420", 34, 18, 3)
    sp = spec(T.F32, Q.BT709, plus1, 0, T.IMAGENET)
    want = expected(reference(packets), "420", sp)
    decs = [A.DECODER(), A.DECODER()]
    decp = (DECP * 2)(*[C.pointer(d) for d in decs])
    fns, rets = (C.c_uint32 * 2)(), (C.c_int * 2)()
    bufs, arr = (A.BUF * 2)(), (OUTTENSOR * 2)()
    for i in range(2):  # no metadata yet: anything may be passed (here: entries that are all zeros but for an unknown dtype)
        mk_buf(hip, bufs[i], packets[0])
        arr[i].dtype = 99
    assert hip.dsv2hip_dec_batch_tensor(2, decp, bufs, arr, fns, rets) == 2
    assert list(rets) == [A.DEC_GOT_META] * 2
    tens = [OutTensor(tensor_dims(hip, d, T.F32), **sp) for d in decs]
    for t in tens:
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
        assert all(t.untouched() for t in tens)

    def refused(what):
        for i in range(2):
            fns[i], rets[i] = 77, -5
        assert hip.dsv2hip_dec_batch_tensor(2, decp, bufs, arr, fns, rets) == -1, what
        one_fn = C.c_uint32(77)
        assert hip.dsv2hip_dec_tensor_frame(C.byref(decs[1]), C.byref(bufs[1]), C.byref(arr[1]), C.byref(one_fn)) == -1, what
        assert one_fn.value == 77
        nothing_happened()

    arr[0] = tens[0].c
    for what, spoil in REFUSALS:
        C.memmove(C.byref(arr[1]), C.byref(tens[1].c), C.sizeof(OUTTENSOR))
        spoil(arr[1])
        refused(what)
    # an -out420p decoder takes no tensor; the switch off again, it does
    arr[1] = tens[1].c
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 1) == 0
    state[1] = bytes(C.string_at(C.byref(decs[1]), C.sizeof(decs[1])))  # (the switch may have made the decoder's private part)
    refused("out420p")
    assert hip.dsv2hip_dec_set_out420p(C.byref(decs[1]), 0) == 0
    for bad in (dict(n=0), dict(decs=None), dict(bufs=None), dict(t=None), dict(fn=None), dict(ret=None)):
        args = dict(n=2, decs=decp, bufs=bufs, t=arr, fn=fns, ret=rets)
        args.update(bad)
        for i in range(2):
            fns[i], rets[i] = 77, -5
        assert hip.dsv2hip_dec_batch_tensor(args["n"], args["decs"], args["bufs"], args["t"], args["fn"], args["ret"]) == -1, bad
        nothing_happened()
    # the same packets, the good tensors: decoded as if nothing had happened, and on to the end of the stream
    got = [[(A.DEC_GOT_META, None, None)] for _ in range(2)]
    for t in range(1, len(packets)):
        if t > 1:
            for i in range(2):
                mk_buf(hip, bufs[i], packets[t])
                tens[i].arm()
            torch.cuda.synchronize()
        had_meta = [d.got_metadata for d in decs]
        assert hip.dsv2hip_dec_batch_tensor(2, decp, bufs, arr, fns, rets) == 2
        for i in range(2):
            pic = rets[i] == A.DEC_OK and had_meta[i]
            got[i].append((rets[i], fns[i] if pic else None, tens[i].planes() if pic else None))
    for i in range(2):
        same(want, got[i])
        hip.dsv_dec_free(C.byref(decs[i]))


def test_uint8_tensors_ignore_the_constants():
    hip = bind(A.load_hip())
    packets = format_stream("420", 34, 18, 3)
    junk = ((float("nan"), float("inf"), -1e30), (float("-inf"), float("nan"), 7.0))
    _, got, _ = equals_reference(hip, packets, "420", [spec(T.U8, Q.BT709, consts=junk), spec(T.U8, Q.BT709)])
    same(got[0], got[1])


# ---- 10. the statistics -------------------------------------------------------------------------------------------------------------
def test_statistics_count_rounds_by_form():
    hip = bind(A.load_hip())
    packets = format_stream("420", 36, 20, 3)
    reset_forms(hip)
    equals_reference(hip, packets, "420", [spec(T.F32, consts=T.IMAGENET), spec(T.U8)])  # two aligned tensors a round: one wide round each
    assert tensor_forms(hip) == (3, 0)
    equals_reference(hip, packets, "420", [spec(T.F32, consts=T.IMAGENET), spec(T.U8, offset=1)])  # one of them off the grid: the round is general
    assert tensor_forms(hip) == (3, 3)
    assert rgb_forms(hip) == (0, 0) and resize_forms(hip) == (0, 0)
    equals_reference(hip, packets, "420", [spec(T.F16, size=(18, 10))])
    assert tensor_forms(hip) == (3, 6) and sum(resize_forms(hip)) == 3  # (18 % 4 == 2: general; the resampling counts as any sized picture's)
    assert tensor_forms(hip, reset=True) == (3, 6) and tensor_forms(hip) == (0, 0)
    hip.dsv2hip_dec_tensor_stats(None, 0)


# ---- 11. decode -> uint8 tensor -> encode without the host --------------------------------------------------------------------------
def test_uint8_tensor_goes_straight_into_the_encoder_as_rgbp():
    """A stream decoded into a pitched uint8 tensor whose plane pointers and pitches go straight to dsv2hip_enc_surface_frame as a
    DSV2HIP_SURFACE_RGBP surface: the packets are the reference encoder's on the planar picture that the encoder's conversion
    (tests/rgb3_csc.py) defines on the oracle's bytes."""
    ref, hip = A.load_ref(), bind(A.load_hip())
    w, h, csc = 64, 48, Q.BT709
    packets = stream(w, h, "420", 4, 4)
    sp = spec(T.U8, csc, aligned, 0)
    pictures = [np.stack(pl) for _, _, pl in expected(reference(packets), "420", sp) if pl is not None]
    assert len(pictures) == 4
    want = encode_stream(ref, [R3.planar_bytes(p, R3.RGBP | csc, 1, 1) for p in pictures], w, h, A.SUBSAMP_420, eos=False, qp=50, gop=48)[0]
    enc, dec = A.ENCODER(), A.DECODER()
    configure_encoder(hip, enc, A.mk_meta(w, h, A.SUBSAMP_420), qp=50, gop=48)
    tn = OutTensor((w, h), **sp)
    tn.arm()
    torch.cuda.synchronize()
    src = SURFACE()
    src.layout = R3.RGBP | csc
    for c in range(3):
        src.plane[c], src.pitch[c] = tn.c.plane[c], tn.c.pitch[c]
    got, seen = [], 0
    for pk in packets:
        buf, fn = A.BUF(), C.c_uint32(0)
        mk_buf(hip, buf, pk)
        had_meta = dec.got_metadata
        code = hip.dsv2hip_dec_tensor_frame(C.byref(dec), C.byref(buf), C.byref(tn.c), C.byref(fn))
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
        assert np.array_equal(np.stack(tn.planes()), pictures[seen])  # (and the encoder wrote nothing into the tensor)
        seen += 1
    hip.dsv_enc_free(C.byref(enc))
    hip.dsv_dec_free(C.byref(dec))
    assert seen == 4 and len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a == b, "packet %d differs" % i
