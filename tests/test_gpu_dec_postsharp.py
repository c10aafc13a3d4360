"""dsv2hip_dec_set_postsharp: the reference CLI's -postsharp (dsv_post_process, bmc.c:340, on the luma of the frame dsv_dec
returned) inside the decoder.  The luma of every picture handed out -- by dsv_dec, dsv2hip_dec_batch and the device deliveries --
equals the reference decoder's luma put through the reference's own dsv_post_process; chroma equals the unsharpened reference;
the picture later P pictures predict from is never sharpened; -out420p and draw_info come first, the sharpening last."""
import ctypes as C
import functools

import numpy as np
import pytest

import dsvabi as A
from dec_out import decode, device_decode, expected_sharp as expected, frame_decode, planes_of, same_results, stream
from hipabi import bind, mk_buf

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def host_decode(hip, packets, mode=0, sharp=True, out420p=False):
    """dec_out.decode through dsv_dec with the postsharp switch set before every call"""
    bind(hip)
    dec = A.DECODER()
    if out420p:
        assert hip.dsv2hip_dec_set_out420p(C.byref(dec), 1) == 0
    out = []
    for k, pk in enumerate(packets):
        dec.draw_info = mode
        assert hip.dsv2hip_dec_set_postsharp(C.byref(dec), int(sharp(k) if callable(sharp) else sharp)) == 0
        buf = A.BUF()
        mk_buf(hip, buf, pk)
        fp = C.POINTER(A.FRAME)()
        fn = C.c_uint32(0)
        code = hip.dsv_dec(C.byref(dec), C.byref(buf), C.byref(fp), C.byref(fn))
        planes = None
        if code == A.DEC_OK and fp:
            planes = planes_of(fp)
            hip.dsv_frame_ref_dec(fp)
        out.append((code, fn.value if planes is not None else None, planes))
        if code == A.DEC_EOS:
            break
    hip.dsv_dec_free(C.byref(dec))
    return out


CASES = [(352, 288, "420", 9, 4), (354, 290, "444", 3, 48), (354, 290, "420", 3, 48)]


@functools.lru_cache(maxsize=None)
def want_sharp(w, h, fmt, nfr, gop):
    return expected(A.load_ref(), stream(w, h, fmt, nfr, gop))


@pytest.mark.parametrize("w,h,fmt,nfr,gop", CASES)
def test_dsv_dec(w, h, fmt, nfr, gop):
    same_results(want_sharp(w, h, fmt, nfr, gop), host_decode(A.load_hip(), stream(w, h, fmt, nfr, gop)))


def test_dec_batch_sharpens_per_decoder():
    """the three streams in one step sequence (two geometries, three formats), plus an unsharpened decoder on the first"""
    ref, hip = A.load_ref(), A.load_hip()
    streams = [stream(*c) for c in CASES] + [stream(*CASES[0])]
    got = frame_decode(hip, streams, [0] * 4, [True, True, True, False])
    for c, g in zip(CASES, got):
        same_results(want_sharp(*c), g)
    same_results(decode(ref, streams[3], 0), got[3])


@pytest.mark.parametrize("offset", [0, 1])
def test_device_delivery(offset):
    """offset 0: CIF through the wide form; offset 1: every stream through the general form, odd destination addresses"""
    ref, hip = A.load_ref(), A.load_hip()
    streams = [stream(*c) for c in CASES] + [stream(*CASES[0])]
    got = device_decode(hip, streams, sharp=[True, True, True, False], offset=offset)
    for c, g in zip(CASES, got):
        same_results(want_sharp(*c), g)
    same_results(decode(ref, streams[3], 0), got[3])


def test_switch_toggled_from_packet_to_packet():
    """exactly the pictures handed out while the switch is on are sharpened; what they are predicted from never is"""
    ref, hip = A.load_ref(), A.load_hip()
    packets = stream(352, 288, "420", 9, 4)
    for toggle in (lambda k: k % 2 == 1, lambda k: k % 2 == 0):
        want = expected(ref, packets, sharp=toggle)
        same_results(want, host_decode(hip, packets, sharp=toggle))
        same_results(want, device_decode(hip, [packets], sharp=[toggle])[0])


def test_out420p_then_sharpen():
    ref, hip = A.load_ref(), A.load_hip()
    packets = stream(354, 290, "444", 3, 48)
    want = expected(ref, packets, to420=(A.SUBSAMP_444, 354, 290))
    assert want[1][2][1].shape == (145, 177)
    same_results(want, host_decode(hip, packets, out420p=True))
    same_results(want, device_decode(hip, [packets], out420p=[True], sharp=[True])[0])
    same_results(want, device_decode(hip, [packets], out420p=[True], sharp=[True], offset=1)[0])


def test_draw_info_then_sharpen():
    ref, hip = A.load_ref(), A.load_hip()
    packets = stream(352, 288, "420", 9, 4)
    want = expected(ref, packets, mode=3)
    plain = want_sharp(352, 288, "420", 9, 4)
    assert any(not np.array_equal(a[2][0], b[2][0]) for a, b in zip(want, plain) if a[2] is not None)  # the overlay is there
    same_results(want, host_decode(hip, packets, mode=3))
    same_results(want, device_decode(hip, [packets], modes=[3], sharp=[True])[0])
