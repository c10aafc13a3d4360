"""Lockstep batch decoding (dsv2hip_dec_batch): n packets per step == n independent reference decodes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dsvabi as A
from codec_run import decode_stream, encode_stream, frames
from conftest import load_pkg
from dec_out import Surfaces, batch_decode, check, decode_steps, expected_sharp, in_layout, pictures, same_results
from hipabi import PLANAR, SEMI, bind

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def test_dec_batch_mixed_streams():
    """Four streams in lockstep: two CIF IP streams of different length, one intra-only CIF stream, and a
    720p stream (second geometry in the same step); metadata / picture / end-of-stream packets interleave."""
    ref, hip = A.load_ref(), A.load_hip()
    bind(hip)
    pkg = load_pkg()
    spec = [(352, 288, 9, dict(qp=60, gop=4)), (352, 288, 5, dict(qp=40, gop=12)), (352, 288, 4, dict(qp=85, gop=0)),
            (1280, 720, 3, dict(qp=60, gop=48))]
    streams = []
    for s, (w, h, nfr, cfg) in enumerate(spec):
        v = pkg.synth.SynthVideo(w, h, "420", seed=70 + s)
        frames = [v.frame_bytes(t) for t in range(nfr)]
        streams.append(encode_stream(ref, frames, w, h, A.SUBSAMP_420, eos=True, **cfg)[0])
    want = [decode_stream(ref, pk) for pk in streams]
    got = batch_decode(hip, streams)
    for s in range(len(spec)):
        check(want[s], got[s])


def test_dec_batch_444_lossless_and_single_call_agree():
    ref, hip = A.load_ref(), A.load_hip()
    bind(hip)
    pkg = load_pkg()
    streams = []
    for s in range(2):
        v = pkg.synth.SynthVideo(354, 290, "444", seed=90 + s)
        frames = [v.frame_bytes(t) for t in range(3)]
        streams.append(encode_stream(ref, frames, 354, 290, A.SUBSAMP_444, eos=True, qp=100 if s else 70, gop=48)[0])
    want = [decode_stream(ref, pk) for pk in streams]
    got = batch_decode(hip, streams)
    single = [decode_stream(hip, pk) for pk in streams]
    for s in range(2):
        check(want[s], got[s])
        check(want[s], single[s])


def test_lossless_round_trip_1080p_through_both_batch_engines():
    """Size-independent property at the full BASELINE picture size: lossless (-qp=100) batch encode followed by
    batch decode returns the input pictures bit for bit (no reference needed)."""
    import torch
    from codec_run import configure_encoder
    hip = A.load_hip()
    bind(hip)
    pkg = load_pkg()
    w, h, ns, nf = 1920, 1080, 2, 3
    vids = [pkg.synth.SynthVideo(w, h, "420", seed=40 + s) for s in range(ns)]
    frames = [[v.frame_bytes(t) for t in range(nf)] for v in vids]
    meta = A.mk_meta(w, h, A.SUBSAMP_420)
    encs = [A.ENCODER() for _ in range(ns)]
    for e in encs:
        configure_encoder(hip, e, meta, qp=100, gop=48)
    encp = (C.POINTER(A.ENCODER) * ns)(*[C.pointer(e) for e in encs])
    bufs = (A.BUF * (4 * ns))()
    nbufs = (C.c_int * ns)()
    streams = [[] for _ in range(ns)]
    for t in range(nf):
        dev = [torch.from_numpy(np.frombuffer(frames[s][t], dtype=np.uint8).copy()).cuda() for s in range(ns)]
        torch.cuda.synchronize()
        ptrs = (C.c_void_p * ns)(*[d.data_ptr() for d in dev])
        assert hip.dsv2hip_enc_batch(ns, encp, ptrs, bufs, nbufs) == 0
        for s in range(ns):
            for i in range(nbufs[s]):
                b = bufs[4 * s + i]
                streams[s].append(bytes(C.string_at(b.data, b.len)))
                hip.dsv_buf_free(C.byref(b))
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    got = batch_decode(hip, streams)
    for s in range(ns):
        assert len(got[s]) == nf
        for t, (fn, y, u, v) in enumerate(got[s]):
            raw = np.frombuffer(frames[s][t], dtype=np.uint8)
            assert np.array_equal(y.ravel(), raw[:w * h])
            assert np.array_equal(u.ravel(), raw[w * h:w * h + w * h // 4])
            assert np.array_equal(v.ravel(), raw[w * h + w * h // 4:])


# ---- one round of every kind -------------------------------------------------------------------------------------------------
# Ten 4:2:2 streams of three pictures: eight of 80x48 (five by three blocks, width no multiple of 32) and two of 72x40 (a second
# round in every step; luma width no multiple of 16).  (gop, qp, offset): gop 0 = intra only, qp 100 = lossless; an offset stream
# starts with a one-picture closed GOP, so its I picture shares a step with the others' P pictures; an intra-only stream has a
# metadata packet before every picture.  Step 3 holds a picture of every stream: all four (frame type, lossless) classes at 80x48,
# a lossy P and a lossless I picture at 72x40.
KINDS = [(80, 48, 48, 60, False), (80, 48, 48, 60, False), (80, 48, 0, 60, False), (80, 48, 48, 100, False), (80, 48, 48, 60, True),
         (80, 48, 0, 100, False), (80, 48, 48, 100, True), (80, 48, 48, 60, False), (72, 40, 48, 60, False), (72, 40, 0, 100, False)]
DRAW_ALL = 7  # DSV_DRAW_STABHQ | DSV_DRAW_MOVECS | DSV_DRAW_IBLOCK
SUBSAMP_422 = 0x4
# leg A, per stream: (draw_info, postsharp, out420p); the draw_info decoders are 80x48 ones: the reference stores intra marks
# without a bounds check, so it is compared on block-aligned pictures only (test_gpu_dec_drawinfo.py)
HOST_OPTS = [(DRAW_ALL, False, False), (0, True, False), (DRAW_ALL, True, False), (0, False, True), (0, True, True)] + [(0, False, False)] * 5
# leg B: planar and semiplanar surfaces alternate; pitches: row bytes rounded up to 64, one odd (83 / 43 for rows of 80 / 40 bytes)
SURF_OPTS = [(0, k == 2, k == 3) for k in range(10)]


@functools.lru_cache(maxsize=None)
def kind_stream(k):
    w, h, gop, qp, offset = KINDS[k]
    fr = frames(w, h, 1, 0, 3, 30 + k)
    enc = lambda f, eos: encode_stream(A.load_ref(), f, w, h, SUBSAMP_422, eos=eos, qp=qp, gop=gop)[0]
    return tuple(enc(fr[:1], False) + enc(fr[1:], True)) if offset else tuple(enc(fr, True))


@functools.lru_cache(maxsize=None)
def kind_want(k, mode, sharp, to420):
    """the reference decode of stream k with the post-steps applied by the reference / the oracle (shared, never modified)"""
    w, h = KINDS[k][:2]
    want = expected_sharp(A.load_ref(), kind_stream(k), mode=mode, sharp=sharp, to420=(SUBSAMP_422, w, h) if to420 else None)
    assert sum(1 for r in want if r[2] is not None) == 3
    return tuple(want)


@pytest.mark.parametrize("parse_mode", [0, 1], ids=["host-parse", "P-on-device"])
def test_one_round_of_every_kind(parse_mode):
    """Every job table of a device round filled in the same round: I and P, lossy and lossless pictures, host- and (mode 1:
    the P pictures) device-parsed sections, whole-frame copies, 4:2:0 conversion, egress with and without sharpening, chroma
    interleave with and without conversion, overlay, overlay + sharpening -- through dsv2hip_dec_batch into host frames (leg A)
    and through dsv2hip_dec_batch_surface into planar and semiplanar surfaces (leg B).  Every delivered picture equals the
    reference decode of its stream with the same post-steps.  (No stream carries a damaged plane section: the damaged packets
    of test_gpu_robustness.py are drawn at random inside its test, so the zfail table stays empty here.)"""
    hip = bind(A.load_hip())
    assert A.block_geometry(80, 48)[2:] == (5, 3) and 80 % A.block_geometry(80, 48)[0] == 0 and 48 % A.block_geometry(80, 48)[1] == 0
    streams = [kind_stream(k) for k in range(len(KINDS))]
    kinds = [[r[0] for r in kind_want(k, 0, False, False)] for k in range(len(KINDS))]
    assert all(k[3] == A.DEC_OK for k in kinds) and len(streams[4]) == len(streams[0]) + 1  # (step 3; an offset stream is one packet longer)
    specs = [dict(layout=SEMI if k % 2 else PLANAR, pitch=(lambda rb: rb + 3) if k == 5 else (lambda rb: (rb + 63) // 64 * 64), offset=0) for k in range(len(KINDS))]
    try:
        assert hip.dsv2hip_dec_set_parse_mode(parse_mode) == parse_mode
        got = batch_decode(hip, streams, *zip(*HOST_OPTS))
        for k, opts in enumerate(HOST_OPTS):
            check(pictures(kind_want(k, *opts)), got[k])
        modes, sharp, out420p = zip(*SURF_OPTS)
        got = decode_steps(hip, streams, Surfaces(specs), modes=modes, sharp=sharp, out420p=out420p)
        for k, opts in enumerate(SURF_OPTS):
            same_results(in_layout(kind_want(k, *opts), specs[k]["layout"]), got[k])
    finally:
        hip.dsv2hip_dec_set_parse_mode(-1)
