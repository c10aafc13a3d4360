"""Decoded pictures delivered to device memory (dsv2hip_dec_batch_device, dsv2hip_dec_device_frame, dsv2hip_dec_picture_bytes):
every picture, frame number and return code equals the reference decoder's -- both forms of the egress kernel (16-byte rows /
any width and alignment), every chroma format, draw_info and -out420p, both parsers, two geometries in one step -- no byte outside
[dev_out, dev_out + picture_bytes) is written, a refused call consumes nothing, and the device buffers feed dsv2hip_enc_batch
without a host copy."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dsvabi as A
from codec_run import configure_encoder, encode_stream
from test_gpu_dec_drawinfo import decode, stream
from test_gpu_formats import FMT as FMT5, frames as plain_frames
from test_oracle_fmt import chroma_dims, orc_to420

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

GUARD = 0xA5
NO_FN = 0xFFFFFFFF


def bind(hip):
    P = C.POINTER
    hip.dsv2hip_dec_picture_bytes.argtypes = [P(A.DECODER)]
    hip.dsv2hip_dec_picture_bytes.restype = C.c_size_t
    hip.dsv2hip_dec_batch_device.argtypes = [C.c_int, P(P(A.DECODER)), P(A.BUF), P(C.c_void_p), P(C.c_size_t), P(C.c_uint32), P(C.c_int)]
    hip.dsv2hip_dec_batch_device.restype = C.c_int
    hip.dsv2hip_dec_device_frame.argtypes = [P(A.DECODER), P(A.BUF), C.c_void_p, C.c_size_t, P(C.c_uint32)]
    hip.dsv2hip_dec_device_frame.restype = C.c_int
    hip.dsv2hip_dec_set_out420p.argtypes = [P(A.DECODER), C.c_int]
    hip.dsv2hip_dec_set_postsharp.argtypes = [P(A.DECODER), C.c_int]
    hip.dsv2hip_dec_set_postsharp.restype = C.c_int
    hip.dsv2hip_dec_set_parse_mode.argtypes = [C.c_int]
    hip.dsv2hip_dec_set_parse_mode.restype = C.c_int
    return hip


def mk_buf(hip, buf, pk):
    hip.dsv_mk_buf(C.byref(buf), len(pk) + 64)
    C.memmove(buf.data, pk, len(pk))


def out_dims(dec, out420p):
    """[(w, h)] of the three planes of the picture as delivered (dsv_mk_frame's plane sizes)"""
    m = dec.vidmeta
    cw, ch = chroma_dims(A.SUBSAMP_420 if out420p else m.subsamp, m.width, m.height)
    return [(m.width, m.height), (cw, ch), (cw, ch)]


def split_planes(flat, dims):
    out, at = [], 0
    for w, h in dims:
        out.append(flat[at:at + w * h].reshape(h, w).copy())
        at += w * h
    assert at == flat.size
    return out


class DevOut:
    """One decoder's device buffer: picture_bytes + 64 bytes of 0xA5, handed over at base + offset."""

    def __init__(self, nbytes, offset):
        self.nbytes, self.offset = nbytes, offset
        self.t = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0

    def arm(self):
        self.t.fill_(GUARD)

    def ptr(self):
        return self.t.data_ptr() + self.offset

    def picture(self):
        """the delivered bytes; asserts that every byte around them still holds the guard value"""
        a = self.t.cpu().numpy()
        assert np.all(a[:self.offset] == GUARD), "bytes before the picture were written"
        assert np.all(a[self.offset + self.nbytes:] == GUARD), "bytes behind the picture were written"
        return a[self.offset:self.offset + self.nbytes]


def lockstep(streams, schedule=None, delay=None):
    """the steps of a run, each the ordered [(decoder, packet index)] it feeds: packet t (t - delay[k]) of every stream that has
    one, or the caller's schedule -- in which a step holds whichever decoders and packets it names, each decoder's in order"""
    if schedule is not None:
        at = [0] * len(streams)
        for step in schedule:
            for k, p in step:
                assert p == at[k] < len(streams[k]), "the schedule feeds decoder %d packet %d, its next one is %d" % (k, p, at[k])
                at[k] += 1
        return [list(step) for step in schedule if step]
    delay = delay or [0] * len(streams)
    return [[(k, t - delay[k]) for k in range(len(streams)) if 0 <= t - delay[k] < len(streams[k])]
            for t in range(max(len(s) + d for s, d in zip(streams, delay)))]


def device_decode(hip, streams, modes=None, out420p=None, sharp=None, offset=0, schedule=None, single=False):
    """Lockstep steps over one decoder per stream, pictures delivered to device memory.  Per stream: [(return code, frame number
    or None, [Y, U, V] or None)] per packet, as test_gpu_dec_drawinfo.decode gives for dsv_dec.  modes / out420p / sharp: per
    stream; a mode or sharp entry may be a function of the packet's index (set before every step).  schedule: lockstep()'s;
    single: one dsv2hip_dec_device_frame per packet in place of the step's batch call."""
    bind(hip)
    n = len(streams)
    modes = modes or [0] * n
    out420p = out420p or [False] * n
    sharp = sharp or [False] * n
    decs = [A.DECODER() for _ in range(n)]
    for d, o in zip(decs, out420p):
        if o:
            assert hip.dsv2hip_dec_set_out420p(C.byref(d), 1) == 0
    outs = [None] * n
    res = [[] for _ in range(n)]
    done = [False] * n
    for step in lockstep(streams, schedule):
        at = {k: t for k, t in step if not done[k]}
        live = list(at)
        m = len(live)
        decp = (C.POINTER(A.DECODER) * m)(*[C.pointer(decs[k]) for k in live])
        bufs = (A.BUF * m)()
        ptrs, caps, had_meta = (C.c_void_p * m)(), (C.c_size_t * m)(), []
        for i, k in enumerate(live):
            t = at[k]
            decs[k].draw_info = modes[k](t) if callable(modes[k]) else modes[k]
            assert hip.dsv2hip_dec_set_postsharp(C.byref(decs[k]), int(sharp[k](t) if callable(sharp[k]) else sharp[k])) == 0
            mk_buf(hip, bufs[i], streams[k][t])
            pb = hip.dsv2hip_dec_picture_bytes(C.byref(decs[k]))
            had_meta.append(pb > 0)
            if pb:
                dims = out_dims(decs[k], out420p[k])
                assert pb == sum(w * h for w, h in dims)
                if outs[k] is None or outs[k].nbytes != pb:
                    outs[k] = DevOut(pb, offset)
                outs[k].arm()
                ptrs[i], caps[i] = outs[k].ptr(), pb
            else:
                assert decs[k].got_metadata == 0
                ptrs[i], caps[i] = None, 0
        fns = (C.c_uint32 * m)()
        rets = (C.c_int * m)()
        torch.cuda.synchronize()  # (the guard fills run on torch's stream, the decoder on its own)
        if single:
            for i in range(m):
                fn = C.c_uint32(0)
                rets[i] = hip.dsv2hip_dec_device_frame(decp[i], C.byref(bufs[i]), ptrs[i], caps[i], C.byref(fn))
                fns[i] = fn.value
        else:
            assert hip.dsv2hip_dec_batch_device(m, decp, bufs, ptrs, caps, fns, rets) == m
        for i, k in enumerate(live):
            planes = None
            if outs[k] is not None and had_meta[i]:
                flat = outs[k].picture()  # (guards checked after every step, picture or not)
                if rets[i] == A.DEC_OK:
                    planes = split_planes(flat, out_dims(decs[k], out420p[k]))
                else:
                    assert np.all(flat == GUARD)
            if planes is None and rets[i] == A.DEC_OK:
                assert fns[i] == NO_FN
            res[k].append((rets[i], fns[i] if planes is not None else None, planes))
            done[k] = rets[i] == A.DEC_EOS
    for d in decs:
        hip.dsv_dec_free(C.byref(d))
    return res


def same_results(want, got, planes=(0, 1, 2)):
    assert [r[0] for r in want] == [r[0] for r in got]
    assert [r[1] for r in want] == [r[1] for r in got]
    for (_, fn, pw), (_, _, pg) in zip(want, got):
        assert (pw is None) == (pg is None)
        if pw is not None:
            for c in planes:
                assert pw[c].shape == pg[c].shape
                assert np.array_equal(pw[c], pg[c]), "frame %d plane %d differs in %d samples" % (fn, c, int(np.sum(pw[c] != pg[c])))


@functools.lru_cache(maxsize=None)
def format_stream(name, w, h, nfr):
    code, hs, vs = FMT5[name]
    return tuple(encode_stream(A.load_ref(), plain_frames(w, h, hs, vs, nfr, 5), w, h, code, eos=True, qp=60, gop=12)[0])


def npics(results):
    return sum(1 for r in results if r[2] is not None)


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
    hip.dsv2hip_enc_batch.argtypes = [C.c_int, C.POINTER(C.POINTER(A.ENCODER)), C.POINTER(C.c_void_p), C.POINTER(A.BUF), C.POINTER(C.c_int)]
    hip.dsv2hip_enc_batch.restype = C.c_int
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
