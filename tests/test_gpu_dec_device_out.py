"""Decoded pictures delivered to device memory (dsv2hip_dec_batch_device, dsv2hip_dec_device_frame, dsv2hip_dec_picture_bytes):
every picture, frame number and return code equals the reference decoder's -- both forms of the egress kernel (16-byte rows /
any width and alignment), every chroma format, draw_info and -out420p, both parsers, two geometries in one step -- no byte outside
[dev_out, dev_out + picture_bytes) is written, a refused call consumes nothing, and the device buffers feed dsv2hip_enc_batch
without a host copy."""
import ctypes as C

import numpy as np
import pytest
import torch

import dsvabi as A
from codec_run import configure_encoder, encode_stream
from dec_out import DevOut, decode, device_decode, format_stream, npics, orc_to420, out_dims, same_results, split_planes, stream
from hipabi import GUARD, bind, mk_buf

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def test_picture_bytes_of_a_null_and_a_fresh_decoder():
    hip = bind(A.load_hip())
    assert hip.dsv2hip_dec_picture_bytes(None) == 0
    dec = A.DECODER()
    assert hip.dsv2hip_dec_picture_bytes(C.byref(dec)) == 0
    assert hip.dsv2hip_dec_set_postsharp(None, 1) == -1


@pytest.mark.parametrize("w,h,fmt,nfr,gop", [(352, 288, "420", 9, 4), (354, 290, "420", 3, 48), (354, 290, "444", 3, 48)])
@pytest.mark.parametrize("offset", [0, 1])
def test_equals_reference_and_writes_nothing_else(w, h, fmt, nfr, gop, offset):
    """offset 0: 352x288 takes the wide form, 354x290 (177-wide chroma in 4:2:0) the general one; offset 1: the general form on
    an odd destination address at every size.  The bytes around the picture are checked after every step (DevOut.picture)."""
    ref, hip = A.load_ref(), A.load_hip()
    packets = stream(w, h, fmt, nfr, gop)
    want = decode(ref, packets, 0)
    assert npics(want) == nfr and want[0][0] == A.DEC_GOT_META and want[-1][0] == A.DEC_EOS
    if gop == 4:
        assert len(packets) > nfr + 2  # (a metadata packet per GOP: I and P pictures both occur)
    same_results(want, device_decode(hip, [packets], offset=offset)[0])


@pytest.mark.parametrize("name", ["422", "411", "410"])
def test_other_chroma_formats(name):
    ref, hip = A.load_ref(), A.load_hip()
    packets = format_stream(name, 330, 250, 3)
    want = decode(ref, packets, 0)
    assert npics(want) == 3
    same_results(want, device_decode(hip, [packets])[0])


def mixed_batch(ref, hip):
    cif, c444, hd = stream(352, 288, "420", 9, 4), stream(354, 290, "444", 3, 48), stream(1280, 720, "420", 3, 48)
    got = device_decode(hip, [cif, cif, c444, hd], modes=[0, 7, 0, 0], out420p=[False, False, True, False])
    same_results(decode(ref, cif, 0), got[0])
    same_results(decode(ref, cif, 7), got[1])
    same_results(decode(ref, hd, 0), got[3])
    orc = A.load_oracle()
    want = []
    for code, fn, pl in decode(ref, c444, 0):
        if pl is not None:
            pl = [pl[0]] + [orc_to420(orc, np.ascontiguousarray(pl[c]), A.SUBSAMP_444, 354, 290) for c in (1, 2)]
        want.append((code, fn, pl))
    same_results(want, got[2])
    assert got[2][1][2][1].shape == (145, 177)
    assert not np.array_equal(got[0][1][2][0], got[1][1][2][0])  # the overlay is there


def test_batch_with_mixed_geometries_and_options():
    """Four decoders in one step sequence: CIF plain, CIF with draw_info = 7, 354x290 4:4:4 with -out420p, 1280x720."""
    mixed_batch(A.load_ref(), A.load_hip())


def test_batch_with_mixed_geometries_and_options_device_parser():
    ref, hip = A.load_ref(), bind(A.load_hip())
    try:
        assert hip.dsv2hip_dec_set_parse_mode(2) == 2
        mixed_batch(ref, hip)
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)


def test_refused_calls_consume_nothing():
    ref, hip = A.load_ref(), bind(A.load_hip())
    packets = stream(352, 288, "420", 9, 4)
    want = decode(ref, packets, 0)
    dec = A.DECODER()
    decp = (C.POINTER(A.DECODER) * 1)(C.pointer(dec))
    fns, rets = (C.c_uint32 * 1)(), (C.c_int * 1)()
    ptrs, caps = (C.c_void_p * 1)(), (C.c_size_t * 1)()
    bufs = (A.BUF * 1)()
    # no metadata yet: NULL is allowed, the metadata packet is consumed
    mk_buf(hip, bufs[0], packets[0])
    ptrs[0], caps[0] = None, 0
    assert hip.dsv2hip_dec_batch_device(1, decp, bufs, ptrs, caps, fns, rets) == 1
    assert rets[0] == A.DEC_GOT_META and dec.got_metadata == 1
    pb = hip.dsv2hip_dec_picture_bytes(C.byref(dec))
    assert pb == 352 * 288 * 3 // 2
    out = DevOut(pb, 0)
    out.arm()
    torch.cuda.synchronize()
    mk_buf(hip, bufs[0], packets[1])
    data, length = C.cast(bufs[0].data, C.c_void_p).value, bufs[0].len
    state = bytes(C.string_at(C.byref(dec), C.sizeof(dec)))
    for p, cap in ((out.ptr(), pb - 1), (None, pb)):
        ptrs[0], caps[0] = p, cap
        assert hip.dsv2hip_dec_batch_device(1, decp, bufs, ptrs, caps, fns, rets) == -1
        assert C.cast(bufs[0].data, C.c_void_p).value == data and bufs[0].len == length
        assert bytes(C.string_at(bufs[0].data, len(packets[1]))) == packets[1]
        assert bytes(C.string_at(C.byref(dec), C.sizeof(dec))) == state
        assert np.all(out.t.cpu().numpy() == GUARD)
    assert hip.dsv2hip_dec_device_frame(C.byref(dec), bufs, out.ptr(), pb - 1, fns) == -1
    assert hip.dsv2hip_dec_batch_device(0, decp, bufs, ptrs, caps, fns, rets) == -1
    assert hip.dsv2hip_dec_batch_device(1, decp, bufs, None, caps, fns, rets) == -1
    assert bytes(C.string_at(bufs[0].data, len(packets[1]))) == packets[1]
    # the same packet with a buffer that holds the picture: decoded as if nothing had happened
    ptrs[0], caps[0] = out.ptr(), pb
    assert hip.dsv2hip_dec_batch_device(1, decp, bufs, ptrs, caps, fns, rets) == 1
    assert rets[0] == A.DEC_OK and fns[0] == want[1][1]
    got = split_planes(out.picture(), out_dims(dec, False))
    for c in range(3):
        assert np.array_equal(got[c], want[1][2][c])
    hip.dsv_dec_free(C.byref(dec))


def test_transcode_without_the_host():
    """Two CIF streams decoded into device buffers whose pointers go straight to dsv2hip_enc_batch: the packets are the
    reference encoder's on the reference decoder's pictures.  dsv2hip_dec_device_frame gives the batch call's pictures."""
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
    pb = w * h * 3 // 2
    dev = [torch.zeros(pb, dtype=torch.uint8, device="cuda") for _ in range(ns)]
    torch.cuda.synchronize()
    got, pics = [[] for _ in range(ns)], [[] for _ in range(ns)]
    for t in range(max(len(s) for s in streams)):
        live = [k for k in range(ns) if t < len(streams[k])]
        m = len(live)
        decp = (C.POINTER(A.DECODER) * m)(*[C.pointer(decs[k]) for k in live])
        bufs = (A.BUF * m)()
        for i, k in enumerate(live):
            mk_buf(hip, bufs[i], streams[k][t])
        ptrs = (C.c_void_p * m)(*[dev[k].data_ptr() for k in live])
        caps = (C.c_size_t * m)(*[pb] * m)
        fns, rets = (C.c_uint32 * m)(), (C.c_int * m)()
        had_meta = [decs[k].got_metadata for k in live]
        assert hip.dsv2hip_dec_batch_device(m, decp, bufs, ptrs, caps, fns, rets) == m
        ready = [k for i, k in enumerate(live) if rets[i] == A.DEC_OK and had_meta[i]]
        if not ready:
            continue
        r = len(ready)
        encp = (C.POINTER(A.ENCODER) * r)(*[C.pointer(encs[k]) for k in ready])
        src = (C.c_void_p * r)(*[dev[k].data_ptr() for k in ready])
        obufs, nbufs = (A.BUF * (4 * r))(), (C.c_int * r)()
        assert hip.dsv2hip_enc_batch(r, encp, src, obufs, nbufs) == 0
        for i, k in enumerate(ready):
            pics[k].append(dev[k].cpu().numpy().copy())
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
    out = torch.zeros(pb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for pk in streams[0]:
        buf = A.BUF()
        mk_buf(hip, buf, pk)
        fn = C.c_uint32(0)
        had_meta = dec.got_metadata
        code = hip.dsv2hip_dec_device_frame(C.byref(dec), C.byref(buf), out.data_ptr(), pb, C.byref(fn))
        if code == A.DEC_OK and had_meta:
            one.append((fn.value, out.cpu().numpy().copy()))
        if code == A.DEC_EOS:
            break
    hip.dsv_dec_free(C.byref(dec))
    assert code == A.DEC_EOS and [f for f, _ in one] == [r[1] for r in refpics[0]]
    for (_, a), b in zip(one, pics[0]):
        assert np.array_equal(a, b)
