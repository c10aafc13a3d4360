"""Lockstep encoder steps whose streams differ in everything a step need not share (tests/mixed_steps.py: the cases, the
driver; tests/test_mixed_steps_ref.py: the cases are what they claim).  Every stream's packets and final stats must be exactly the
reference encoder's on that stream alone -- whatever its neighbours in the step are, whichever slot it has, whichever group,
scratch and entry point its pictures come through.  Every assertion is equality; there are no tolerances."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import dsvabi as A
import mixed_steps as M
from codec_run import configure_encoder

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def streams_of(specs):
    return [M.build(sp) for sp in specs]


def device(t):
    return "device"


def check(specs, schedule, entry=device, what="", **kw):
    streams = streams_of(specs)
    got = M.run_schedule(A.load_hip(), streams, schedule, entry, **kw)
    M.assert_same(M.reference_packets(streams), got, what)


# ---- a, b: one step, every option mixed --------------------------------------------------------------------------------------
def test_everything_a_step_need_not_share():
    """14 streams (one entropy chain), each another row of the table: in list order, reversed, and rotated by t at step t -- a
    result that depends on the slot is the bug this hunts"""
    specs = M.everything()
    sched = M.together(specs)
    check(specs, sched, what="in order:")
    check(specs, [ids[::-1] for ids in sched], what="reversed:")
    check(specs, [ids[t % len(ids):] + ids[:t % len(ids)] for t, ids in enumerate(sched)], what="rotated:")


def test_small_step_mixed():
    """the first 5 rows: n < 12, the entropy coding of a small step"""
    specs = M.everything(5)
    sched = M.together(specs)
    check(specs, sched)
    check(specs, [ids[t % len(ids):] + ids[:t % len(ids)] for t, ids in enumerate(sched)], what="rotated:")


# ---- c: joins, leaves, a stream that sits out ---------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["device", "host"])
def test_staggered_joins_and_leaves(entry):
    """frame-number parity, GOP phase and the ping-pong indices differ across every step; in the host run the prefetched picture
    of the stream that sits out waits two steps in its stage buffer, and stream 8's caller announces one picture and brings
    another (the one brought is encoded)"""
    specs, sched = M.staggered()
    check(specs, sched, lambda t: entry)


# ---- d: encoders move between groups ------------------------------------------------------------------------------------------
def test_regrouping():
    """two threads, each running lockstep steps on its half of 12 encoders; the halves are re-dealt after every second step (the
    threads are joined in between: this is about state carried across batch scratches, not about racing one encoder)"""
    specs, sched = M.regrouping()
    streams = streams_of(specs)
    run = M.Runner(A.load_hip(), streams)
    errors = []

    def work(group_steps):
        try:
            for ids in group_steps:
                run.step(ids, "device")
        except BaseException as e:  # noqa: B902 (reported by the main thread)
            errors.append(e)

    for t in range(0, len(sched), 2):
        ths = [threading.Thread(target=work, args=([sched[u][g] for u in range(t, min(t + 2, len(sched)))],)) for g in range(2)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors
    M.assert_same(M.reference_packets(streams), run.finish())


# ---- e: entry points alternate on one encoder -----------------------------------------------------------------------------------
def test_entry_points_alternate_on_one_encoder():
    """device, host, surface, single, frame, device ... on the same 6 encoders; stream 5 joins at step 1 with symbol lists of 1000
    entries (its first intra picture is redone beside neighbours that are not); the two surface steps run the wide and the
    general form of both surface ingests"""
    hip = M.bind(A.load_hip())
    specs, sched = M.alternating()
    streams = streams_of(specs)
    run = M.Runner(hip, streams)
    yuv, rgb = (C.c_ulonglong * 2)(), (C.c_ulonglong * 2)()
    hip.dsv2hip_enc_surface_stats(yuv, 1)
    hip.dsv2hip_enc_rgb_stats(rgb, 1)
    for t, ids in enumerate(sched):
        before = hip.dsv2hip_enc_list_growths()
        with M.env(**(dict(DSV2_COMPACT_CAP=1000) if t == 1 else {})):
            run.step(ids, M.ENTRY_CYCLE[t % len(M.ENTRY_CYCLE)])
        assert hip.dsv2hip_enc_list_growths() - before == (1 if t == 1 else 0), "step %d" % t
    hip.dsv2hip_enc_surface_stats(yuv, 0)
    hip.dsv2hip_enc_rgb_stats(rgb, 0)
    M.assert_same(M.reference_packets(streams), run.finish())
    assert list(yuv) == [1, 1] and list(rgb) == [1, 1], "surface steps by form: YUV %r, RGB %r" % (list(yuv), list(rgb))


# ---- f: other step keys ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.KEY_CASES))
def test_other_step_keys(name):
    specs = M.key_case(name)
    sched = M.together(specs)
    check(specs, [ids[t % len(ids):] + ids[:t % len(ids)] for t, ids in enumerate(sched)])


# ---- g: threads of plain dsv_enc ----------------------------------------------------------------------------------------------
def _enc_thread(hip, st, out, idx, start):
    """tests/test_gpu_api_threads.py's caller, with the stream's own metadata and settings"""
    sp = st["spec"]
    enc = A.ENCODER()
    configure_encoder(hip, enc, A.mk_meta(**st["meta_kw"]), **st["cfg"])
    bufs, pk = (A.BUF * 4)(), []
    start.wait()
    for fb in st["frames"]:
        arr = np.frombuffer(fb, dtype=np.uint8).copy()
        fr = hip.dsv_load_planar_frame(M.FMT[sp.fmt][0], arr.ctypes.data, sp.w, sp.h)
        for i in range(hip.dsv_enc(C.byref(enc), fr, bufs)):
            pk.append(bytes(C.string_at(bufs[i].data, bufs[i].len)))
            hip.dsv_buf_free(C.byref(bufs[i]))
    stats = {k: getattr(enc.stats, k) for k in M.STAT_KEYS}
    hip.dsv_enc_free(C.byref(enc))
    out[idx] = (pk, stats)


def test_threads_of_plain_dsv_enc_with_different_settings():
    """8 threads loop plain dsv_enc, each with another row: the submit queue merges them into steps by step key alone"""
    hip = A.load_hip()
    streams = streams_of(M.everything(8))
    out = [None] * len(streams)
    start = threading.Barrier(len(streams))
    ths = [threading.Thread(target=_enc_thread, args=(hip, st, out, s, start)) for s, st in enumerate(streams)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert all(o is not None for o in out), "a caller died: %r" % [o is not None for o in out]
    M.assert_same(M.reference_packets(streams), ([o[0] for o in out], [o[1] for o in out]))


# ---- h: what a step must share ----------------------------------------------------------------------------------------------------
REFUSED = [("do_psy", M.W, M.H, dict(do_psy=0)), ("block_size_override_x", M.W, M.H, dict(block_size_override_x=1)),
           ("pyramid_levels", 352, 288, dict(pyramid_levels=3))]  # (352x288 resolves to 4 levels; 176x144 to 3)


@pytest.mark.parametrize("what,w,h,over", REFUSED, ids=[r[0] for r in REFUSED])
def test_different_step_keys_are_refused_and_touch_nothing(what, w, h, over):
    """two started encoders that differ in one member of the step key: the three batch calls return -1 with nbufs, the
    DSV_ENCODER bytes (next_fnum among them) and the input buffers as they were; each encoder then encodes its stream alone"""
    hip = M.bind(A.load_hip())
    specs = [M.table_stream(2, nframes=4, seed0=800, cut=False, w=w, h=h), M.table_stream(2, nframes=4, seed0=801, cut=False, w=w, h=h, over=over)]
    streams = streams_of(specs)
    run = M.Runner(hip, streams)
    encs = [run.encoder(s) for s in range(2)]
    encp = (C.POINTER(A.ENCODER) * 2)(*[C.pointer(e) for e in encs])
    state = [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs]
    bufs = (A.BUF * 8)()
    dev = [torch.from_numpy(np.frombuffer(st["frames"][0], dtype=np.uint8).copy()).cuda() for st in streams]
    was = [d.clone() for d in dev]
    surf = [M.make_surface(st, 1, 0, False) for st in streams]  # (kind 1: pitched planar)
    host = (C.c_void_p * 2)(*[run.host_picture(s, 0) for s in range(2)])
    nxt = (C.c_void_p * 2)(*[run.host_picture(s, 1) for s in range(2)])
    torch.cuda.synchronize()
    calls = [lambda nb: hip.dsv2hip_enc_batch(2, encp, (C.c_void_p * 2)(*[d.data_ptr() for d in dev]), bufs, nb),
             lambda nb: hip.dsv2hip_enc_batch_host(2, encp, host, nxt, bufs, nb),
             lambda nb: hip.dsv2hip_enc_batch_surface(2, encp, (M.SURFACE * 2)(*[M.SURFACE.from_buffer_copy(sf.c) for sf in surf]), bufs, nb)]
    for k, call in enumerate(calls):
        nbufs = (C.c_int * 2)(77, 78)
        assert call(nbufs) == -1, "call %d was not refused" % k
        assert list(nbufs) == [77, 78]
        assert [bytes(C.string_at(C.byref(e), C.sizeof(e))) for e in encs] == state, "call %d changed an encoder" % k
        assert [e.next_fnum for e in encs] == [0, 0]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dev, was))
    for sf in surf:
        sf.check_untouched()
    for s, st in enumerate(streams):
        assert bytes(C.string_at(run.host_picture(s, 0), len(st["frames"][0]))) == st["frames"][0]
    for t in range(specs[0].nframes):  # alone, through the three entry points in turn
        for s in range(2):
            run.step([s], ("device", "host", "surface")[(t + s) % 3])
    M.assert_same(M.reference_packets(streams), run.finish())
