"""dsv2hip_dec_set_postsharp: the reference CLI's -postsharp (dsv_post_process, bmc.c:340, on the luma of the frame dsv_dec
returned) inside the decoder.  The luma of every picture handed out -- by dsv_dec, dsv2hip_dec_batch and the device deliveries --
equals the reference decoder's luma put through the reference's own dsv_post_process; chroma equals the unsharpened reference;
the picture later P pictures predict from is never sharpened; -out420p and draw_info come first, the sharpening last."""
import ctypes as C
import functools

import numpy as np
import pytest

import dsvabi as A
from test_gpu_dec_batch import bind as bind_batch, planes_of
from test_gpu_dec_device_out import bind, device_decode, mk_buf, same_results
from test_gpu_dec_drawinfo import decode, stream
from test_oracle_fmt import orc_to420

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

MIN_CHANGED = 1000  # a compared picture in which sharpening changes fewer luma samples than this shows nothing


def ref_sharpen(ref, y):
    """the reference's dsv_post_process on a copy of the plane, in an unbordered frame of the reference's own making"""
    h, w = y.shape
    fp = ref.dsv_mk_frame(A.SUBSAMP_420, w, h, 0)
    p = fp.contents.planes[0]
    assert p.w == w and p.h == h
    a = np.ctypeslib.as_array(p.data, shape=(p.h * p.stride,)).reshape(p.h, p.stride)
    a[:, :w] = y
    ref.dsv_post_process.argtypes = [C.POINTER(A.PLANE)]
    ref.dsv_post_process.restype = None
    ref.dsv_post_process(C.byref(p))
    out = a[:, :w].copy()
    ref.dsv_frame_ref_dec(fp)
    return out


def expected(ref, packets, mode=0, sharp=True, to420=None):
    """Reference results per packet with the luma of the pictures picked by `sharp` (True, or a function of the packet's index)
    sharpened by the reference; to420 = (subsamp, w, h): chroma through the oracle's -out420p conversion.  Asserts that the
    sharpening changes at least MIN_CHANGED samples of each such picture and leaves the cells the reference skips alone."""
    orc = A.load_oracle() if to420 else None
    out = []
    for k, (code, fn, pl) in enumerate(decode(ref, packets, mode)):
        if pl is not None:
            pl = list(pl)
            if to420:
                pl[1:] = [orc_to420(orc, np.ascontiguousarray(c), *to420) for c in pl[1:]]
            if sharp(k) if callable(sharp) else sharp:
                y = ref_sharpen(ref, pl[0])
                h, w = y.shape
                assert int(np.sum(y != pl[0])) >= MIN_CHANGED
                # the last cell column / row -- partial at 354x290, whole but skipped by the reference's >= at 352x288 -- is a copy
                assert np.array_equal(y[:, (w - 1) // 4 * 4:], pl[0][:, (w - 1) // 4 * 4:])
                assert np.array_equal(y[(h - 1) // 4 * 4:], pl[0][(h - 1) // 4 * 4:])
                pl[0] = y
        out.append((code, fn, pl))
    return out


def host_decode(hip, packets, mode=0, sharp=True, out420p=False):
    """test_gpu_dec_drawinfo.decode through dsv_dec with the postsharp switch set before every call"""
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


def host_batch_decode(hip, streams, sharp):
    """dsv2hip_dec_batch over one decoder per stream, postsharp per decoder"""
    bind(hip)
    bind_batch(hip)
    n = len(streams)
    decs = [A.DECODER() for _ in range(n)]
    for d, s in zip(decs, sharp):
        assert hip.dsv2hip_dec_set_postsharp(C.byref(d), int(s)) == 0
    res = [[] for _ in range(n)]
    for t in range(max(len(s) for s in streams)):
        live = [k for k in range(n) if t < len(streams[k])]
        m = len(live)
        decp = (C.POINTER(A.DECODER) * m)(*[C.pointer(decs[k]) for k in live])
        bufs = (A.BUF * m)()
        for i, k in enumerate(live):
            mk_buf(hip, bufs[i], streams[k][t])
        outs = (C.POINTER(A.FRAME) * m)()
        fns = (C.c_uint32 * m)()
        rets = (C.c_int * m)()
        assert hip.dsv2hip_dec_batch(m, decp, bufs, outs, fns, rets) == m
        for i, k in enumerate(live):
            planes = None
            if rets[i] == A.DEC_OK and outs[i]:
                planes = planes_of(outs[i])
                hip.dsv_frame_ref_dec(outs[i])
            res[k].append((rets[i], fns[i] if planes is not None else None, planes))
    for d in decs:
        hip.dsv_dec_free(C.byref(d))
    return res


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
    got = host_batch_decode(hip, streams, [True, True, True, False])
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
