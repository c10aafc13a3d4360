"""libdsv2hip.so against the real reference at the edges (tests/edge_cases.py), bit for bit: every stage of the C ABI seam over
geometries x contents, then tiny whole streams through the plain API and both batch engines.  tests/test_oracle_edges.py runs
the same inputs through the reference on the CPU and has to pass first: it shows that the reference survives them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dsvabi as A
from codec_run import configure_encoder, decode_stream, encode_stream
from edge_cases import (BATCH_CFG, BATCH_GEOMETRIES, BATCH_STREAMS, CONTENTS, GEOM_IDS, GEOM_IDS_420, GEOMETRIES, GEOMETRIES_420,
                        STREAM_CASES, STREAM_FRAMES, STREAM_SEED, TIE_SCENES, TIE_SIZES, content_frame, inverse_reads_stale_scratch,
                        packet_bound_holds, stream_frames, stream_inverse_is_undefined, tie_scene_planes)
from hme_common import Scene, assert_fields_equal
from test_gpu_dec_batch import batch_decode, bind, check
from test_gpu_quant import decode_plane
from test_gpu_sbt import hip_fwd, hip_inv
from test_oracle_bmc import clone, rand_motion
from test_oracle_edges import content_scene, filter_can_act, intra_filter_input
from test_oracle_hzcc import rand_mvs, ref_encode_plane
from test_oracle_intra import ref_intra_flags
from test_oracle_sbt import ref_fwd, ref_inv

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)

geometries = pytest.mark.parametrize("w,h,subsamp", GEOMETRIES, ids=GEOM_IDS)


@geometries
@pytest.mark.parametrize("isP,lossless", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_sbt(w, h, subsamp, isP, lossless):
    ref, hip = A.load_ref(), A.load_hip()
    meta = A.mk_meta(w, h, subsamp)
    params = A.mk_params(meta, w, h, isP, lossless)
    nb = params.nblocks_h * params.nblocks_v
    blockdata = np.random.RandomState(w * 7 + h + isP).randint(0, 128, size=nb).astype(np.uint8)
    cdims = A.coef_dims(subsamp, w, h)
    for kind in CONTENTS:
        frame = content_frame(kind, subsamp, w, h)
        for plane in range(3):
            cw, ch = cdims[plane]
            want = ref_fwd(ref, frame, plane, isP, lossless, blockdata, params, cdims)
            got = hip_fwd(hip, frame, plane, isP, blockdata, params, cdims)
            assert np.array_equal(want, got), "%s: fwd plane %d" % (kind, plane)
            q = 1 if lossless else 200
            coefs = want.copy() if lossless else (want // 24) * 24
            got_px = hip_inv(hip, coefs, plane, isP, q, blockdata, params, cdims, subsamp, w, h)
            if lossless:
                assert np.array_equal(got_px, frame.plane(plane)), "%s: lossless plane %d" % (kind, plane)
            elif inverse_reads_stale_scratch(cw, ch, plane, isP, lossless):
                continue  # the reference's output depends on the calls before this one
            want_px = ref_inv(ref, coefs, plane, isP, lossless, q, blockdata, params, cdims, subsamp, w, h)
            assert np.array_equal(want_px, got_px), "%s: inv plane %d" % (kind, plane)


@geometries
@pytest.mark.parametrize("isP,lossless,q,do_psy", [(0, 0, 180, 0xff), (1, 0, 172, 0xff), (0, 0, 40, 0), (1, 0, 900, 0x1),
                                                    (0, 1, 1, 0xff), (1, 1, 1, 0xff), (0, 0, 900, 1)])
def test_encode_decode_plane(w, h, subsamp, isP, lossless, q, do_psy):
    ref, hip = A.load_ref(), A.load_hip()
    meta = A.mk_meta(w, h, subsamp)
    params = A.mk_params(meta, w, h, isP, lossless, do_psy=do_psy)
    nb = params.nblocks_h * params.nblocks_v
    rng = np.random.RandomState(w + 3 * h + isP + q)
    blockdata = rng.randint(0, 128, size=nb).astype(np.uint8)
    mvs = rand_mvs(rng, nb)
    cdims = A.coef_dims(subsamp, w, h)
    for kind in CONTENTS:
        frame = content_frame(kind, subsamp, w, h, seed=1)
        for plane in range(3):
            cw, ch = cdims[plane]
            coefs = ref_fwd(ref, frame, plane, isP, lossless, blockdata, params, cdims)
            want_bytes, want_coefs = ref_encode_plane(ref, coefs, cw, ch, q, plane, isP, params, blockdata, mvs)
            got_bytes, got_coefs = ref_encode_plane(hip, coefs, cw, ch, q, plane, isP, params, blockdata, mvs)
            assert np.array_equal(want_coefs, got_coefs), "%s: dequantised coefficients, plane %d" % (kind, plane)
            assert np.array_equal(want_bytes, got_bytes), "%s: plane bitstream, plane %d" % (kind, plane)
            ok_r, dec_r, pos_r = decode_plane(ref, want_bytes, cw, ch, q, plane, isP, params, blockdata)
            ok_h, dec_h, pos_h = decode_plane(hip, want_bytes, cw, ch, q, plane, isP, params, blockdata)
            # (the reference's decoder refuses a plane of 8 bytes a coefficient or more, hzcc.c:627, which its encoder does write for
            # the smallest planes of saturated content: both libraries then return 0 and leave position and coefficients alike)
            fits = len(want_bytes) - 4 < cw * ch * 8
            assert ok_r == int(fits) and ok_h == int(fits) and pos_r == pos_h, "%s: plane %d" % (kind, plane)
            assert np.array_equal(dec_r, dec_h), "%s: decoded coefficients, plane %d" % (kind, plane)


@geometries
@pytest.mark.parametrize("lossless,tmc,do_filter,q", [(0, 0, 1, 700), (0, 1, 1, 172), (0, 1, 0, 2500), (1, 0, 1, 1)])
def test_motion_compensation_and_filters(w, h, subsamp, lossless, tmc, do_filter, q):
    ref, hip = A.load_ref(), A.load_hip()
    meta = A.mk_meta(w, h, subsamp, inter_sharpen=1)
    params = A.mk_params(meta, w, h, 1, lossless, temporal_mc=tmc)
    rng = np.random.RandomState(w + h + q + tmc)
    mvs = rand_motion(rng, params, big=(q == 700))
    mvp = C.cast(mvs.ctypes.data, C.POINTER(A.MV))
    fm = A.FMETA()
    fm.params = C.pointer(params)
    fm.isP = 1
    for kind in CONTENTS:
        refframe = content_frame(kind, subsamp, w, h, seed=3)
        ref.dsv_extend_frame(refframe.ptr())
        src = content_frame(kind, subsamp, w, h, seed=4)
        ref.dsv_extend_frame(src.ptr())

        pred_r, resd_r = A.HostFrame(subsamp, w, h), clone(src)
        pred_h, resd_h = A.HostFrame(subsamp, w, h), clone(src)
        ref.dsv_sub_pred(mvp, C.byref(params), pred_r.ptr(), resd_r.ptr(), refframe.ptr())
        hip.dsv_sub_pred(mvp, C.byref(params), pred_h.ptr(), resd_h.ptr(), refframe.ptr())
        for c in range(3):
            assert np.array_equal(pred_r.full[c], pred_h.full[c]), "%s: prediction plane %d" % (kind, c)
            assert np.array_equal(resd_r.full[c], resd_h.full[c]), "%s: residual plane %d" % (kind, c)

        ref.dsv_add_res(mvp, C.byref(fm), q, resd_r.ptr(), pred_r.ptr(), do_filter)
        hip.dsv_add_res(mvp, C.byref(fm), q, resd_h.ptr(), pred_h.ptr(), do_filter)
        for c in range(3):
            assert np.array_equal(resd_r.full[c], resd_h.full[c]), "%s: add_res plane %d" % (kind, c)

        resd = content_frame(kind, subsamp, w, h, seed=9)
        out_r, out_h = A.HostFrame(subsamp, w, h), A.HostFrame(subsamp, w, h)
        ref.dsv_add_pred(mvp, C.byref(fm), q, resd.ptr(), out_r.ptr(), refframe.ptr(), do_filter)
        hip.dsv_add_pred(mvp, C.byref(fm), q, resd.ptr(), out_h.ptr(), refframe.ptr(), do_filter)
        for c in range(3):
            assert np.array_equal(out_r.full[c], out_h.full[c]), "%s: add_pred plane %d" % (kind, c)


@geometries
@pytest.mark.parametrize("q", [60, 400, 3000])
def test_intra_filter(w, h, subsamp, q):
    ref, hip = A.load_ref(), A.load_hip()
    meta = A.mk_meta(w, h, subsamp)
    params = A.mk_params(meta, w, h, 0, 0)
    nb = params.nblocks_h * params.nblocks_v
    bd = np.random.RandomState(q + w).choice([0, 1, 2, 3, 8, 9, 10], size=nb).astype(np.uint8)
    fm = A.FMETA()
    fm.params = C.pointer(params)
    fm.blockdata = A.np_ptr(bd, C.c_uint8)
    for kind in CONTENTS:
        a = intra_filter_input(kind, subsamp, w, h)
        before = a.plane(0).copy()
        b = clone(a)
        ref.dsv_intra_filter(q, C.byref(params), C.byref(fm), 0, a.plane_ptr(0), 1)
        hip.dsv_intra_filter(q, C.byref(params), C.byref(fm), 0, b.plane_ptr(0), 1)
        assert np.array_equal(a.plane(0), b.plane(0)), kind
        if kind == "smooth" and q != 60 and filter_can_act(params):
            assert not np.array_equal(a.plane(0), before), "the case does not exercise the filter"


@geometries
@pytest.mark.parametrize("do_psy", [0xff, 0x1, 0x10, 0x0])
def test_intra_analysis(w, h, subsamp, do_psy):
    ref, hip = A.load_ref(), A.load_hip()
    meta = A.mk_meta(w, h, subsamp)
    params = A.mk_params(meta, w, h, 0, 0, do_psy=do_psy)
    for kind in CONTENTS:
        frame = content_frame(kind, subsamp, w, h, seed=2)
        ref.dsv_extend_frame(frame.ptr())
        assert np.array_equal(ref_intra_flags(ref, frame, params), ref_intra_flags(hip, frame, params)), kind


def check_hme(ref, hip, sc, quant, effort, what):
    want, ipct_r, scb_r, err_r = sc.run_reference(ref, quant, effort)
    got, ipct_h, scb_h, err_h = sc.run_reference(hip, quant, effort)  # same call, the product library
    for l in range(sc.levels, -1, -1):
        assert_fields_equal(want[l], got[l], "%s level %d" % (what, l))
    assert (ipct_r, scb_r, err_r) == (ipct_h, scb_h, err_h), what


@geometries
@pytest.mark.parametrize("quant,effort,prev", [(172, 10, True), (900, 7, False)])
def test_hme(w, h, subsamp, quant, effort, prev):
    ref, hip = A.load_ref(), A.load_hip()
    for kind in CONTENTS:
        check_hme(ref, hip, content_scene(ref, kind, w, h, subsamp, prev), quant, effort, kind)


@pytest.mark.parametrize("w,h", TIE_SIZES, ids=["%dx%d" % s for s in TIE_SIZES])
@pytest.mark.parametrize("prev", [True, False], ids=["prev-mvs", "no-prev-mvs"])
@pytest.mark.parametrize("effort", [10, 7])
def test_hme_ties(w, h, prev, effort):
    """flat and periodic pictures: every candidate, or every candidate a period apart, has the same SAD, and the winner is the
    one the reference's scan order meets first -- whatever order the kernels reduce in"""
    ref, hip = A.load_ref(), A.load_hip()
    for name in TIE_SCENES:
        sc = Scene(ref, w, h, A.SUBSAMP_420, 11, with_prev_mvs=prev, planes=tie_scene_planes(name, w, h))
        check_hme(ref, hip, sc, 172, effort, name)


@geometries
def test_extend_and_ds2x(w, h, subsamp):
    """border extension and the 2x decimation pyramid three levels deep (dsv_encoder.c:494-516): down to 2 x 2 inside a 32-pixel border"""
    ref, hip = A.load_ref(), A.load_hip()
    for kind in CONTENTS:
        a = content_frame(kind, subsamp, w, h, seed=5)
        b = clone(a)
        ref.dsv_extend_frame(a.ptr())
        hip.dsv_extend_frame(b.ptr())
        for c in range(3):
            assert np.array_equal(a.full[c], b.full[c]), "%s: extend plane %d" % (kind, c)
        pa, pb = a, b
        for lvl in range(1, 4):
            dw, dh = (w + (1 << lvl) - 1) >> lvl, (h + (1 << lvl) - 1) >> lvl
            na, nb_ = A.HostFrame(subsamp, dw, dh, border=True), A.HostFrame(subsamp, dw, dh, border=True)
            ref.dsv_ds2x_frame_luma(na.ptr(), pa.ptr())
            hip.dsv_ds2x_frame_luma(nb_.ptr(), pb.ptr())
            assert np.array_equal(na.plane(0), nb_.plane(0)), "%s: ds2x level %d" % (kind, lvl)
            ref.dsv_extend_frame_luma(na.ptr())
            hip.dsv_extend_frame_luma(nb_.ptr())
            assert np.array_equal(na.full[0], nb_.full[0]), "%s: extend luma level %d" % (kind, lvl)
            pa, pb = na, nb_


@pytest.mark.parametrize("w,h,subsamp", GEOMETRIES_420, ids=GEOM_IDS_420)
def test_post_process(w, h, subsamp):
    ref, hip = A.load_ref(), A.load_hip()
    ref.dsv_post_process.argtypes = [C.POINTER(A.PLANE)]
    hip.dsv_post_process.argtypes = [C.POINTER(A.PLANE)]
    for kind in ("white", "checker", "smooth"):
        a = content_frame(kind, subsamp, w, h, seed=11)
        b = clone(a)
        ref.dsv_post_process(a.plane_ptr(0))
        hip.dsv_post_process(b.plane_ptr(0))
        assert np.array_equal(a.full[0], b.full[0]), kind


# ---- tiny whole streams (the measured packet sizes and the rule they obey: tests/edge_cases.py) ------------------------------

def assert_packets_equal(pk_r, pk_h):
    assert len(pk_r) == len(pk_h)
    for i, (a, b) in enumerate(zip(pk_r, pk_h)):
        assert len(a) == len(b), "packet %d length %d vs %d" % (i, len(a), len(b))
        if a != b:
            d = next(k for k in range(len(a)) if a[k] != b[k])
            raise AssertionError("packet %d differs at byte %d of %d" % (i, d, len(a)))


@pytest.mark.parametrize("name,w,h,subsamp,content,cfg", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_tiny_stream_bit_exact(name, w, h, subsamp, content, cfg):
    ref, hip = A.load_ref(), A.load_hip()
    frames = stream_frames(w, h, subsamp, content)
    pk_r, st_r = encode_stream(ref, frames, w, h, subsamp, **cfg)
    packet_bound_holds(pk_r, w, h, subsamp)
    pk_h, st_h = encode_stream(hip, frames, w, h, subsamp, **cfg)
    dec_h = decode_stream(hip, pk_h)
    assert len(dec_h) == STREAM_FRAMES
    if stream_inverse_is_undefined(w, h, subsamp, cfg):
        # the reference's reconstruction is not a function of its input here: its packets count up to the first P picture
        # (metadata and the first intra picture; every packet of an intra-only stream), its decoded pictures not at all
        n = len(pk_r) if cfg["gop"] == 0 else 2
        assert len(pk_r) == len(pk_h)
        assert_packets_equal(pk_r[:n], pk_h[:n])
    else:
        assert_packets_equal(pk_r, pk_h)
        assert st_r == st_h
        dec_r = decode_stream(ref, pk_r)
        assert len(dec_r) == STREAM_FRAMES
        check(dec_r, dec_h)
    if cfg["qp"] == 100:
        for t, (fn, y, u, v) in enumerate(dec_h):
            assert y.tobytes() + u.tobytes() + v.tobytes() == frames[t], "lossless frame %d" % t


def batch_encode(hip, w, h, inputs, cfg):
    """every stream's pictures through dsv2hip_enc_batch_host, one launch a step for all of them"""
    hip.dsv2hip_enc_batch_host.argtypes = [C.c_int, C.POINTER(C.POINTER(A.ENCODER)), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.POINTER(A.BUF), C.POINTER(C.c_int)]
    hip.dsv2hip_enc_batch_host.restype = C.c_int
    hip.dsv2hip_host_alloc.argtypes = [C.c_size_t]
    hip.dsv2hip_host_alloc.restype = C.c_void_p
    hip.dsv2hip_host_free.argtypes = [C.c_void_p]
    n, nf, P = len(inputs), len(inputs[0]), len(inputs[0][0])
    pinned = []
    for fr in inputs:
        p = hip.dsv2hip_host_alloc(P * nf)
        assert p
        for t in range(nf):
            C.memmove(p + t * P, fr[t], P)
        pinned.append(p)
    meta = A.mk_meta(w, h, A.SUBSAMP_420)
    encs = [A.ENCODER() for _ in range(n)]
    for e in encs:
        configure_encoder(hip, e, meta, **cfg)
    got = [[] for _ in range(n)]
    gp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
    for t in range(nf):
        gb = (A.BUF * (4 * n))()
        gn = (C.c_int * n)()
        cur = (C.c_void_p * n)(*[p + t * P for p in pinned])
        nxt = (C.c_void_p * n)(*[(p + (t + 1) * P) if t + 1 < nf else None for p in pinned])
        assert hip.dsv2hip_enc_batch_host(n, gp, cur, nxt, gb, gn) == 0
        for s in range(n):
            for b in range(gn[s]):
                buf = gb[4 * s + b]
                got[s].append(bytes(C.string_at(buf.data, buf.len)))
                hip.dsv_buf_free(C.byref(buf))
    for e in encs:
        hip.dsv_enc_free(C.byref(e))
    for p in pinned:
        hip.dsv2hip_host_free(p)
    return got


@pytest.mark.parametrize("w,h", BATCH_GEOMETRIES, ids=["%dx%d" % g for g in BATCH_GEOMETRIES])
def test_tiny_batches(w, h):
    """eight streams of one tiny geometry through the lockstep encode engine in one launch a step, their packets through the
    lockstep decode engine -- with the plane sections parsed where DSV2_DEC_DEVICE_PARSE says (test_tiny_batches_device_parse)"""
    ref, hip = A.load_ref(), A.load_hip()
    bind(hip)
    inputs = [stream_frames(w, h, A.SUBSAMP_420, "synth", seed=STREAM_SEED + s) for s in range(BATCH_STREAMS)]
    want = [encode_stream(ref, fr, w, h, A.SUBSAMP_420, eos=False, **BATCH_CFG)[0] for fr in inputs]
    for pk in want:
        packet_bound_holds(pk, w, h, A.SUBSAMP_420)
    got = batch_encode(hip, w, h, inputs, BATCH_CFG)
    for s in range(BATCH_STREAMS):
        assert_packets_equal(want[s], got[s])
    pictures = batch_decode(hip, got)
    for s in range(BATCH_STREAMS):
        check(decode_stream(ref, want[s]), pictures[s])


@pytest.mark.parametrize("env", [{"DSV2_DEC_DEVICE_PARSE": "2"}, {"DSV2_DEC_DEVICE_PARSE": "2", "DSV2_DEC_LANE_ROUNDS": "0"},
                                 {"DSV2_DEC_DEVICE_PARSE": "0"}],
                         ids=["all-on-device", "all-on-device-serial-step", "all-on-host"])
def test_tiny_batches_device_parse(env):
    """the switch is read when the library loads (tests/test_gpu_dec_device_parse.py): each setting is a process of its own.
    Sections of a few bytes, planes of 8 x 8 coefficients"""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_edges.py",
                        "-k", "test_tiny_batches and not device_parse"], cwd=A.ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert " passed" in r.stdout
