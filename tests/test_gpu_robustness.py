"""Damaged picture packets: the GPU decoder returns the same codes and the same pictures as the reference
decoder (planes that fail to parse stay zero, dsv_decoder.c:516-523; truncated symbol lists, hzcc.c:525-529)."""
import ctypes as C
import os

import numpy as np
import pytest

import dsvabi as A
from codec_run import encode_stream, meta_packet as _meta_packet
from conftest import load_pkg

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def decode_all(lib, packets):
    """Like codec_run.decode_stream but keeps going after DSV_DEC_ERROR and records every return code."""
    dec = A.DECODER()
    out = []
    for pk in packets:
        buf = A.BUF()
        lib.dsv_mk_buf(C.byref(buf), len(pk) + 64)
        C.memmove(buf.data, pk, len(pk))
        fp = C.POINTER(A.FRAME)()
        fn = C.c_uint32(0)
        code = lib.dsv_dec(C.byref(dec), C.byref(buf), C.byref(fp), C.byref(fn))
        planes = None
        if code == A.DEC_OK and fp:
            f = fp.contents
            planes = []
            for c in range(3):
                p = f.planes[c]
                a = np.ctypeslib.as_array(p.data, shape=(p.h * p.stride,))
                planes.append(a.reshape(-1, p.stride)[:p.h, :p.w].copy())
            lib.dsv_frame_ref_dec(fp)
        out.append((code, fn.value if code == A.DEC_OK else None, planes))
        if code == A.DEC_EOS:
            break
    lib.dsv_dec_free(C.byref(dec))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_damaged_plane_data(seed):
    ref, hip = A.load_ref(), A.load_hip()
    ref.dsv_set_log_level(0)  # the reference reports every damaged plane on stderr
    pkg = load_pkg()
    w, h = 352, 288
    v = pkg.synth.SynthVideo(w, h, "420", seed=11)
    frames = [v.frame_bytes(t) for t in range(5)]
    packets, _ = encode_stream(ref, frames, w, h, A.SUBSAMP_420, eos=True, qp=60, gop=4)
    rng = np.random.default_rng(seed)
    damaged = []
    for pk in packets:
        b = bytearray(pk)
        if len(b) > 400:  # a picture packet: damage bytes in the second half (coefficient data of some plane)
            for _ in range(1 + seed % 3):
                i = int(rng.integers(len(b) // 2, len(b) - 8))
                b[i] ^= int(rng.integers(1, 256))
        damaged.append(bytes(b))
    want, got = decode_all(ref, damaged), decode_all(hip, damaged)
    assert [x[0] for x in want] == [x[0] for x in got]
    for (cw, fw, pw), (cg, fg, pg) in zip(want, got):
        assert fw == fg
        if pw is not None:
            for c in range(3):
                assert np.array_equal(pw[c], pg[c])


def _feed(hip, dec, pk):
    buf = A.BUF()
    hip.dsv_mk_buf(C.byref(buf), len(pk))  # exactly as long as the packet: nothing readable behind it
    C.memmove(buf.data, pk, len(pk))
    fp = C.POINTER(A.FRAME)()
    fn = C.c_uint32(0)
    code = hip.dsv_dec(C.byref(dec), C.byref(buf), C.byref(fp), C.byref(fn))
    if code == A.DEC_OK and fp:
        hip.dsv_frame_ref_dec(fp)
    return code


def test_hostile_packets_return_errors_not_crashes():
    """The product only (the reference reads out of bounds on such input): truncated packets, absurd sub-stream and
    plane lengths, metadata the device pipeline cannot allocate -- every call returns a decoder code, the process
    survives and a clean stream decodes correctly afterwards on the same library."""
    ref, hip = A.load_ref(), A.load_hip()
    pkg = load_pkg()
    w, h = 352, 288
    v = pkg.synth.SynthVideo(w, h, "420", seed=12)
    frames = [v.frame_bytes(t) for t in range(3)]
    packets, _ = encode_stream(ref, frames, w, h, A.SUBSAMP_420, eos=False, qp=60, gop=48)
    meta, pic_i, pic_p = packets[0], packets[1], packets[2]
    rng = np.random.default_rng(5)
    codes = set()
    # (1) truncation at every kind of place
    for pk in (pic_i, pic_p):
        for cut in [15, 18, 20, 24, 30, 40, 64, 100, 200, len(pk) // 3, len(pk) // 2, len(pk) - 1]:
            dec = A.DECODER()
            assert _feed(hip, dec, meta) == A.DEC_GOT_META
            if pk is pic_p:
                assert _feed(hip, dec, pic_i) == A.DEC_OK
            codes.add(_feed(hip, dec, pk[:cut]))
            hip.dsv_dec_free(C.byref(dec))
    # (2) random garbage behind a valid picture header, and 0xff runs (huge exp-Golomb lengths)
    for k in range(24):
        dec = A.DECODER()
        assert _feed(hip, dec, meta) == A.DEC_GOT_META
        junk = bytes(rng.integers(0, 256, size=int(rng.integers(1, 4000)), dtype=np.uint8)) if k % 3 else bytes([0]) * 64 + bytes([0xff]) * 64
        codes.add(_feed(hip, dec, pic_i[:22 + k] + junk))
        hip.dsv_dec_free(C.byref(dec))
    # (3) metadata that must be refused: zero / odd / enormous sizes, unknown subsampling
    for fields in [(0, 288, 5, 30, 1, 1, 1, 1), (352, 0, 5, 30, 1, 1, 1, 1), (353, 288, 5, 30, 1, 1, 1, 1), (1 << 20, 1 << 20, 5, 30, 1, 1, 1, 1),
                   (352, 288, 3, 30, 1, 1, 1, 1), (352, 288, 0x3f, 30, 1, 1, 1, 1)]:
        dec = A.DECODER()
        assert _feed(hip, dec, _meta_packet(fields)) == A.DEC_GOT_META
        assert _feed(hip, dec, pic_i) == A.DEC_ERROR
        hip.dsv_dec_free(C.byref(dec))
    assert codes <= {A.DEC_OK, A.DEC_ERROR}
    # the library is still healthy
    from codec_run import decode_stream
    good = decode_stream(hip, packets)
    want = decode_stream(ref, packets)
    assert len(good) == len(want) == 3
    for a, b in zip(good, want):
        for c in (1, 2, 3):
            assert np.array_equal(a[c], b[c])


@pytest.mark.parametrize("w,h", [(15, 16), (16, 8), (33, 32), (32, 31)])
def test_unsupported_picture_sizes_fail_the_call_not_the_process(w, h):
    """odd or tiny pictures (the reference CLI rejects them, dsv_main.c:621): dsv_enc returns no packets and releases the frame, the
    batch entry point returns -1 -- the process lives (round 4: the library called abort())"""
    from codec_run import configure_encoder
    hip = A.load_hip()
    meta = A.mk_meta(w, h, A.SUBSAMP_420)
    enc = A.ENCODER()
    configure_encoder(hip, enc, meta, qp=60, gop=4)
    hip.dsv_mk_frame.restype = C.POINTER(A.FRAME)
    fr = hip.dsv_mk_frame(A.SUBSAMP_420, w, h, 1)
    bufs = (A.BUF * 4)()
    hip.dsv_enc.restype = C.c_int
    assert hip.dsv_enc(C.byref(enc), fr, bufs) == 0
    hip.dsv2hip_enc_batch_host.argtypes = [C.c_int, C.POINTER(C.POINTER(A.ENCODER)), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(A.BUF), C.POINTER(C.c_int)]
    hip.dsv2hip_enc_batch_host.restype = C.c_int
    pic = np.zeros(w * h * 3, dtype=np.uint8)
    ptrs = (C.c_void_p * 1)(pic.ctypes.data)
    nb = (C.c_int * 1)()
    assert hip.dsv2hip_enc_batch_host(1, (C.POINTER(A.ENCODER) * 1)(C.pointer(enc)), ptrs, None, bufs, nb) == -1
    hip.dsv_enc_free(C.byref(enc))


def test_mixed_geometries_in_one_batch_are_refused_and_arenas_hold_their_instances():
    from codec_run import configure_encoder
    hip = A.load_hip()
    encs = [A.ENCODER(), A.ENCODER()]
    for e, (w, h) in zip(encs, ((64, 48), (96, 48))):
        configure_encoder(hip, e, A.mk_meta(w, h, A.SUBSAMP_420), qp=60, gop=4)
    hip.dsv2hip_enc_batch_host.argtypes = [C.c_int, C.POINTER(C.POINTER(A.ENCODER)), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(A.BUF), C.POINTER(C.c_int)]
    hip.dsv2hip_enc_batch_host.restype = C.c_int
    pics = [np.zeros(96 * 48 * 3 // 2, dtype=np.uint8) for _ in range(2)]
    bufs = (A.BUF * 8)()
    nb = (C.c_int * 2)()
    gp = (C.POINTER(A.ENCODER) * 2)(*[C.pointer(e) for e in encs])
    assert hip.dsv2hip_enc_batch_host(2, gp, (C.c_void_p * 2)(*[p.ctypes.data for p in pics]), None, bufs, nb) == -1
    # each on its own is fine -- and every device buffer of an instance fitted its one-block arena (the size is an estimate
    # kept in step with the allocations by hand: a drift would show here, not as a silent extra hipMalloc)
    for k in range(2):
        g1 = (C.POINTER(A.ENCODER) * 1)(C.pointer(encs[k]))
        assert hip.dsv2hip_enc_batch_host(1, g1, (C.c_void_p * 1)(pics[k].ctypes.data), None, bufs, nb) == 0 and nb[0] >= 1
        for i in range(nb[0]):
            hip.dsv_buf_free(C.byref(bufs[i]))
    hip.dsv2hip_arena_fallbacks.restype = C.c_long
    assert hip.dsv2hip_arena_fallbacks() == 0
    for e in encs:
        hip.dsv_enc_free(C.byref(e))


@pytest.mark.parametrize("how", [1, 2])
def test_a_failed_step_fails_its_calls_and_nothing_else(how):
    """advisor finding (round 5): the StepFailed path had no test, the batch calls returned 0 after a failed step and the step's
    job tables went back to the pool with work still enqueued on its stream.  The hook fails ONE step (how = 1: a search without
    counters, how = 2: the token never came, with the step's first kernels still enqueued): the batch call returns -1 with no
    packets, the encoders of that step are dead (later calls: -1 / 0 packets), a fresh encoder of the same geometry -- which
    takes the same scratch, tables and streams -- then encodes exactly what the reference encodes."""
    from codec_run import configure_encoder, encode_stream
    ref, hip = A.load_ref(), A.load_hip()
    pkg = load_pkg()
    w, h = 352, 288
    v = pkg.synth.SynthVideo(w, h, "420", seed=21)
    frames = [v.frame_bytes(t) for t in range(3)]
    hip.dsv2hip_enc_batch_host.argtypes = [C.c_int, C.POINTER(C.POINTER(A.ENCODER)), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(A.BUF), C.POINTER(C.c_int)]
    hip.dsv2hip_enc_batch_host.restype = C.c_int
    hip.dsv2hip_test_fail_next_step.argtypes = [C.c_int]
    encs = [A.ENCODER(), A.ENCODER()]
    for e in encs:
        configure_encoder(hip, e, A.mk_meta(w, h, A.SUBSAMP_420), qp=60, gop=48)
    gp = (C.POINTER(A.ENCODER) * 2)(*[C.pointer(e) for e in encs])
    bufs = (A.BUF * 8)()
    nb = (C.c_int * 2)()
    pics = [np.frombuffer(f, dtype=np.uint8).copy() for f in frames]

    def step(t):
        nb[0] = nb[1] = 7
        return hip.dsv2hip_enc_batch_host(2, gp, (C.c_void_p * 2)(pics[t].ctypes.data, pics[t].ctypes.data), None, bufs, nb)

    assert step(0) == 0 and nb[0] >= 1 and nb[1] >= 1  # the intra picture
    for k in range(2):
        for i in range(nb[k]):
            hip.dsv_buf_free(C.byref(bufs[4 * k + i]))
    hip.dsv2hip_test_fail_next_step(how)
    assert step(1) == -1 and nb[0] == 0 and nb[1] == 0  # the failed step (a P picture: it searches)
    assert step(2) == -1                                 # dead encoders are refused
    hip.dsv_mk_frame.restype = C.POINTER(A.FRAME)
    hip.dsv_enc.restype = C.c_int
    fr = hip.dsv_mk_frame(A.SUBSAMP_420, w, h, 1)
    assert hip.dsv_enc(C.byref(encs[0]), fr, bufs) == 0
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    # the library is healthy: same scratch, same streams, same geometry
    want, _ = encode_stream(ref, frames, w, h, A.SUBSAMP_420, eos=False, qp=60, gop=48)
    got, _ = encode_stream(hip, frames, w, h, A.SUBSAMP_420, eos=False, qp=60, gop=48)
    assert want == got
