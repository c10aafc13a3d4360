"""The oracle against the real reference at the edges (tests/edge_cases.py): every stage over geometries x contents.  Besides
checking the restatement, this file shows that every input of tests/test_gpu_edges.py is one the reference survives with a roomy
bitstream buffer; it has to pass before those run."""
import ctypes as C
import os

import numpy as np
import pytest

import dsvabi as A
import orcabi as O
from codec_run import decode_stream, encode_stream
from edge_cases import (BATCH_CFG, BATCH_GEOMETRIES, BATCH_STREAMS, CONTENTS, GEOM_IDS, GEOMETRIES, STREAM_CASES, STREAM_FRAMES,
                        STREAM_SEED, TIE_SCENES, TIE_SIZES, content_frame, content_planes, degrade, inverse_reads_stale_scratch,
                        packet_bound, packet_bound_holds, stream_frames, tie_scene_planes)
from hme_common import Scene, assert_fields_equal
from test_oracle_bmc import clone, rand_motion
from test_oracle_hzcc import orc_encode_plane, rand_mvs, ref_encode_plane
from test_oracle_intra import ref_intra_flags
from test_oracle_sbt import ref_fwd, ref_inv

pytestmark = pytest.mark.skipif(not os.path.exists(A.REF_SO), reason="oracle/_ref not built")

geometries = pytest.mark.parametrize("w,h,subsamp", GEOMETRIES, ids=GEOM_IDS)


def filter_can_act(params):
    """the intra filter smooths 4 x 4 cells across and down, the last column and row of cells excepted: in a picture one block
    wide or high the few cells left need not hold one with the texture it looks for"""
    return params.nblocks_h > 1 and params.nblocks_v > 1


@geometries
@pytest.mark.parametrize("isP,lossless", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_sbt(w, h, subsamp, isP, lossless):
    ref, orc = A.load_ref(), A.load_oracle()
    meta = A.mk_meta(w, h, subsamp)
    params = A.mk_params(meta, w, h, isP, lossless)
    nb = params.nblocks_h * params.nblocks_v
    blockdata = np.random.RandomState(w * 7 + h + isP).randint(0, 128, size=nb).astype(np.uint8)
    cdims = A.coef_dims(subsamp, w, h)
    peak = 0
    for kind in CONTENTS:
        frame = content_frame(kind, subsamp, w, h)
        for plane in range(3):
            cw, ch = cdims[plane]
            pw, ph = frame.dims[plane]
            want = ref_fwd(ref, frame, plane, isP, lossless, blockdata, params, cdims)
            peak = max(peak, int(np.abs(want).max()))
            got = np.zeros(cw * ch, dtype=np.int32)
            orc.orc_fwd_sbt(frame.c.planes[plane].data, frame.strides[plane], pw, ph, A.np_ptr(got, C.c_int32), cw, ch, plane, isP,
                            lossless, A.np_ptr(blockdata, C.c_uint8), params.nblocks_h, params.nblocks_v)
            assert np.array_equal(want, got), "%s: fwd plane %d" % (kind, plane)
            if inverse_reads_stale_scratch(cw, ch, plane, isP, lossless) and not lossless:
                continue  # the reference's output depends on the calls before this one
            q = 1 if lossless else 200
            coefs = want.copy() if lossless else (want // 24) * 24
            want_px = ref_inv(ref, coefs, plane, isP, lossless, q, blockdata, params, cdims, subsamp, w, h)
            out = A.HostFrame(subsamp, w, h, border=True)
            orc.orc_inv_sbt(out.c.planes[plane].data, out.strides[plane], pw, ph, A.np_ptr(coefs, C.c_int32), cw, ch, q, plane, isP,
                            lossless, A.np_ptr(blockdata, C.c_uint8), params.nblocks_h, params.nblocks_v)
            assert np.array_equal(want_px, out.plane(plane)), "%s: inv plane %d" % (kind, plane)
            if lossless:
                assert np.array_equal(out.plane(plane), frame.plane(plane)), "%s: lossless plane %d" % (kind, plane)
    if (w, h) == (16, 16) and not isP and not lossless:
        assert peak >= 8160, "the saturated contents do not reach the top of the coefficient range"


@geometries
@pytest.mark.parametrize("isP,lossless,q,do_psy", [(0, 0, 180, 0xff), (1, 0, 172, 0xff), (0, 0, 40, 0), (1, 0, 900, 0x1),
                                                    (0, 1, 1, 0xff), (1, 1, 1, 0xff), (0, 0, 900, 1)])
def test_encode_plane(w, h, subsamp, isP, lossless, q, do_psy):
    ref, orc = A.load_ref(), A.load_oracle()
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
            got_bytes, got_coefs = orc_encode_plane(orc, coefs, cw, ch, q, plane, isP, params, subsamp, blockdata, mvs)
            assert np.array_equal(want_coefs, got_coefs), "%s: dequantised coefficients, plane %d" % (kind, plane)
            assert np.array_equal(want_bytes, got_bytes), "%s: plane bitstream, plane %d" % (kind, plane)


@geometries
@pytest.mark.parametrize("lossless,tmc,do_filter,q", [(0, 0, 1, 700), (0, 1, 1, 172), (0, 1, 0, 2500), (1, 0, 1, 1)])
def test_motion_compensation_and_filters(w, h, subsamp, lossless, tmc, do_filter, q):
    ref, orc = A.load_ref(), A.load_oracle()
    meta = A.mk_meta(w, h, subsamp, inter_sharpen=1)
    params = A.mk_params(meta, w, h, 1, lossless, temporal_mc=tmc)
    rng = np.random.RandomState(w + h + q + tmc)
    mvs = rand_motion(rng, params, big=(q == 700))
    mvp = C.cast(mvs.ctypes.data, C.POINTER(A.MV))
    op = O.orc_params(params, meta)
    fm = A.FMETA()
    fm.params = C.pointer(params)
    fm.isP = 1
    for kind in CONTENTS:
        refframe = content_frame(kind, subsamp, w, h, seed=3)
        ref.dsv_extend_frame(refframe.ptr())
        src = content_frame(kind, subsamp, w, h, seed=4)
        ref.dsv_extend_frame(src.ptr())

        pred_r, resd_r = A.HostFrame(subsamp, w, h), clone(src)
        pred_o, resd_o = A.HostFrame(subsamp, w, h), clone(src)
        ref.dsv_sub_pred(mvp, C.byref(params), pred_r.ptr(), resd_r.ptr(), refframe.ptr())
        orc.orc_sub_pred(C.c_void_p(mvs.ctypes.data), C.byref(op), C.byref(O.oframe(pred_o)), C.byref(O.oframe(resd_o)),
                         C.byref(O.oframe(refframe)))
        for c in range(3):
            assert np.array_equal(pred_r.full[c], pred_o.full[c]), "%s: prediction plane %d" % (kind, c)
            assert np.array_equal(resd_r.full[c], resd_o.full[c]), "%s: residual plane %d" % (kind, c)

        ref.dsv_add_res(mvp, C.byref(fm), q, resd_r.ptr(), pred_r.ptr(), do_filter)
        orc.orc_add_res(C.c_void_p(mvs.ctypes.data), C.byref(op), q, C.byref(O.oframe(resd_o)), C.byref(O.oframe(pred_o)), do_filter)
        for c in range(3):
            assert np.array_equal(resd_r.full[c], resd_o.full[c]), "%s: add_res plane %d" % (kind, c)

        resd = content_frame(kind, subsamp, w, h, seed=9)
        out_r, out_o = A.HostFrame(subsamp, w, h), A.HostFrame(subsamp, w, h)
        ref.dsv_add_pred(mvp, C.byref(fm), q, resd.ptr(), out_r.ptr(), refframe.ptr(), do_filter)
        orc.orc_add_pred(C.c_void_p(mvs.ctypes.data), C.byref(op), q, C.byref(O.oframe(resd)), C.byref(O.oframe(out_o)),
                         C.byref(O.oframe(refframe)), do_filter)
        for c in range(3):
            assert np.array_equal(out_r.full[c], out_o.full[c]), "%s: add_pred plane %d" % (kind, c)


def intra_filter_input(kind, subsamp, w, h):
    a = content_frame(kind, subsamp, w, h, seed=21)
    if kind == "smooth":  # smoother still, so that the texture window (8 < max(sh,sv) < 256) is hit often
        a.plane(0)[:, :] = (a.plane(0).astype(np.int32) // 8 + 100).astype(np.uint8)
    return a


@geometries
@pytest.mark.parametrize("q", [60, 400, 3000])
def test_intra_filter(w, h, subsamp, q):
    ref, orc = A.load_ref(), A.load_oracle()
    meta = A.mk_meta(w, h, subsamp)
    params = A.mk_params(meta, w, h, 0, 0)
    nb = params.nblocks_h * params.nblocks_v
    bd = np.random.RandomState(q + w).choice([0, 1, 2, 3, 8, 9, 10], size=nb).astype(np.uint8)
    fm = A.FMETA()
    fm.params = C.pointer(params)
    fm.blockdata = A.np_ptr(bd, C.c_uint8)
    op = O.orc_params(params, meta)
    for kind in CONTENTS:
        a = intra_filter_input(kind, subsamp, w, h)
        before = a.plane(0).copy()
        b = clone(a)
        ref.dsv_intra_filter(q, C.byref(params), C.byref(fm), 0, a.plane_ptr(0), 1)
        orc.orc_intra_filter(b.c.planes[0].data, b.strides[0], w, h, C.byref(op), A.np_ptr(bd, C.c_uint8), q, 1)
        assert np.array_equal(a.full[0], b.full[0]), kind
        if kind == "smooth" and q != 60 and filter_can_act(params):
            assert not np.array_equal(a.plane(0), before), "the case does not exercise the filter"


@geometries
@pytest.mark.parametrize("do_psy", [0xff, 0x1, 0x10, 0x0])
def test_intra_analysis(w, h, subsamp, do_psy):
    ref, orc = A.load_ref(), A.load_oracle()
    meta = A.mk_meta(w, h, subsamp)
    params = A.mk_params(meta, w, h, 0, 0, do_psy=do_psy)
    nb = params.nblocks_h * params.nblocks_v
    for kind in CONTENTS:
        frame = content_frame(kind, subsamp, w, h, seed=2)
        ref.dsv_extend_frame(frame.ptr())
        want = ref_intra_flags(ref, frame, params)
        got = np.zeros(nb, dtype=A.MV_DTYPE)
        planes = (C.POINTER(C.c_uint8) * 3)(*[frame.c.planes[c].data for c in range(3)])
        strides = (C.c_int * 3)(*frame.strides)
        orc.orc_intra_analysis(planes, strides, C.byref(O.orc_params(params, meta)), C.c_void_p(got.ctypes.data))
        assert np.array_equal(want, got["flags"]), kind


def content_scene(ref, kind, w, h, subsamp, prev):
    """the current picture and the previous one are the same content with another seed: a one-pixel shift of the checkerboard and
    the stripes, other noise, another phase of the smooth picture"""
    before = content_planes(kind, subsamp, w, h, seed=1)
    return Scene(ref, w, h, subsamp, 7, with_prev_mvs=prev, planes=(content_planes(kind, subsamp, w, h, seed=0), before, degrade(before, 7)))


def check_hme(ref, orc, sc, quant, effort, what):
    want, ipct_r, scb_r, err_r = sc.run_reference(ref, quant, effort)
    got, ipct_o, scb_o, err_o = sc.run_oracle(orc, quant, effort)
    for l in range(sc.levels, -1, -1):
        assert_fields_equal(want[l], got[l], "%s level %d" % (what, l))
    assert (ipct_r, scb_r, err_r) == (ipct_o, scb_o, err_o), what


@geometries
@pytest.mark.parametrize("quant,effort,prev", [(172, 10, True), (900, 7, False)])
def test_hme(w, h, subsamp, quant, effort, prev):
    ref, orc = A.load_ref(), A.load_oracle()
    for kind in CONTENTS:
        check_hme(ref, orc, content_scene(ref, kind, w, h, subsamp, prev), quant, effort, kind)


@pytest.mark.parametrize("w,h", TIE_SIZES, ids=["%dx%d" % s for s in TIE_SIZES])
@pytest.mark.parametrize("prev", [True, False], ids=["prev-mvs", "no-prev-mvs"])
@pytest.mark.parametrize("effort", [10, 7])
def test_hme_ties(w, h, prev, effort):
    """flat and periodic pictures: every candidate, or every candidate a period apart, has the same SAD, and the winner is the
    one the reference's scan order meets first"""
    ref, orc = A.load_ref(), A.load_oracle()
    for name in TIE_SCENES:
        sc = Scene(ref, w, h, A.SUBSAMP_420, 11, with_prev_mvs=prev, planes=tie_scene_planes(name, w, h))
        check_hme(ref, orc, sc, 172, effort, name)


@pytest.mark.parametrize("name,w,h,subsamp,content,cfg", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_stream_cases_stay_inside_the_reference_packet_bound(name, w, h, subsamp, content, cfg):
    """every tiny stream of tests/test_gpu_edges.py is one the reference encodes without outgrowing its packet buffer, and
    decodes"""
    ref = A.load_ref()
    packets, _ = encode_stream(ref, stream_frames(w, h, subsamp, content), w, h, subsamp, **cfg)
    print("largest packet %d of %d" % (max(len(p) for p in packets), packet_bound(w, h, subsamp)))
    packet_bound_holds(packets, w, h, subsamp)
    assert len(decode_stream(ref, packets)) == STREAM_FRAMES


@pytest.mark.parametrize("w,h", BATCH_GEOMETRIES)
def test_batch_streams_stay_inside_the_reference_packet_bound(w, h):
    ref = A.load_ref()
    for s in range(BATCH_STREAMS):
        frames = stream_frames(w, h, A.SUBSAMP_420, "synth", seed=STREAM_SEED + s)
        packet_bound_holds(encode_stream(ref, frames, w, h, A.SUBSAMP_420, **BATCH_CFG)[0], w, h, A.SUBSAMP_420)
