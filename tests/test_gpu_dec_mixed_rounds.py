"""Lockstep decoder rounds whose streams differ in everything a round need not share (tests/dec_mixed_rounds.py: the cases, the
driver; tests/test_dec_mixed_rounds_ref.py: the cases are what they claim).  Every decoder is judged on its own: per packet, its
return code, its frame number and every byte it delivers -- the helpers check the guard bytes around every plane after every step
-- must be exactly the reference decoder's on that decoder's packets alone, whatever its neighbours in the round are, whichever
slot it has, whichever parser reads its sections and whichever way its pictures go out.  Every assertion is equality; there are no
tolerances."""
import ctypes as C

import numpy as np
import pytest
import torch

import dec_mixed_rounds as D
import dsvabi as A
from dec_out import DevOut, OutSurf, out_dims, split_planes
from hipabi import OUTSURF, PARSE_IDS, bind, mk_buf, parse_mode, surface_dims

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def run_and_check(cs, mode=None, single=False):
    with parse_mode(mode) as hip:
        D.check(cs, D.run(hip, cs, single=single))


# ---- one round, every option mixed ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2], ids=PARSE_IDS.get)
@pytest.mark.parametrize("order", D.ORDERS)
@pytest.mark.parametrize("name", ["everything", "small"])
def test_everything_a_round_need_not_share(name, order, mode):
    """the 14 rows of the table (the first 5), one step per packet index: in list order, reversed, and rotated by one slot a step -- a
    picture that depends on its slot, or on the first record of its slice, is the bug this hunts; mode 1 mixes host- and device-parsed
    pictures inside the rounds"""
    run_and_check(D.case(name, order), mode)


# ---- joins, leaves, a decoder that sits out --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True], ids=["batch", "single-calls"])
@pytest.mark.parametrize("entry", ["frame", "device", "surface"])
def test_staggered_joins_and_leaves(entry, single):
    """frame-number parity and GOP phase differ across every round; decoder 2 keeps its reference picture over the two steps it sits
    out; through the three batch calls and through dsv_dec / dsv2hip_dec_device_frame / dsv2hip_dec_surface_frame"""
    run_and_check(D.through(D.case("staggered"), entry), single=single)


# ---- damaged neighbours ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2], ids=PARSE_IDS.get)
@pytest.mark.parametrize("entry", ["frame", "surface"])
def test_damaged_neighbours(entry, mode):
    """decoders 2 and 6 of 8 carry damaged plane sections in I and P pictures (refused planes among them: the host's zfail table,
    the device parser's fail flags and zcond table are filled for some slots of a round and not for others): they equal the
    reference's decode of the same damaged packets, return codes included, the six clean neighbours their clean decode"""
    run_and_check(D.through(D.case("damaged"), entry), mode)


# ---- every way out, each on a stream of its own ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=PARSE_IDS.get)
def test_every_way_out_on_its_own_stream(mode):
    """ten decoders, ten deliveries, ten streams, the same steps; expected is the reference decode of each stream with the post-steps
    of the CPU models (the reference's overlay and dsv_post_process, tests/box_reduce.py, tests/yuv_rgb.py) -- not the same decoder
    alone"""
    run_and_check(D.case("ways"), mode)


# ---- other round keys -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=PARSE_IDS.get)
@pytest.mark.parametrize("entry", ["frame", "surface"])
@pytest.mark.parametrize("key", D.KEYS)
def test_other_round_keys(key, entry, mode):
    """five mixed streams at a clipped size, in 4:4:4 and 4:2:2, with 32 x 16 and 32 x 32 blocks and at 64 x 48 (four transform
    levels), rotated by one slot a step; the surfaces alternate planar (odd pitch and address) and semiplanar (NV12 / NV16 / NV24)"""
    run_and_check(D.through(D.case("key_" + key), entry), mode)


def test_two_rounds_of_one_size():
    """three decoders with 16 x 16 and three with 32 x 32 blocks at 176 x 144, interleaved slot by slot: every step splits into two
    rounds by the block size alone"""
    run_and_check(D.case("two_rounds"))
    run_and_check(D.case("two_rounds"), 2)


@pytest.mark.parametrize("entry", ["frame", "device"])
def test_parameters_change_under_a_decoder(entry):
    """picture size, block size, chroma format and the metadata's inter_sharpen / fps change under four decoders, at different steps,
    while their neighbours are mid-GOP: a decoder is rebuilt in phase A of a step and moves to another round"""
    run_and_check(D.through(D.case("change"), entry))


# ---- threads of plain dsv_dec -----------------------------------------------------------------------------------------------------------
def test_threads_of_plain_dsv_dec_with_different_streams():
    """8 threads loop plain dsv_dec, each on another row: the submit queue forms the steps"""
    hip = bind(A.load_hip())
    cs = D.case("threads")
    D.run(hip, cs._replace(feeds=cs.feeds[:1], opts=cs.opts[:1], schedule=D.together(cs.feeds[:1])))  # (binds every prototype before the threads start)
    hip.dsv2hip_dec_queue_stats(None, 1)
    D.check(cs, D.run_threads(hip, cs))
    st = (C.c_ulonglong * 4)()
    hip.dsv2hip_dec_queue_stats(st, 0)
    assert st[0] == sum(len(D.packets(fd)) for fd in cs.feeds)
    assert st[1] < st[0] and st[2] >= 2, "the queue did not merge concurrent dsv_dec callers: %s" % list(st)


# ---- refusals stay whole ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=PARSE_IDS.get)
@pytest.mark.parametrize("entry", ["frame", "device", "surface"])
def test_a_picture_without_its_reference_fails_alone(entry, mode):
    """DSV_DEC_ERROR for the one decoder whose P picture comes before its reference picture -- nothing is delivered for it, its
    destination stays untouched --, the five neighbours of the step deliver the reference's pictures, and the decoder goes on"""
    run_and_check(D.through(D.case("orphan"), entry), mode)


class Destinations:
    """the destinations of dsv2hip_dec_batch_device / dsv2hip_dec_batch_surface for the decoders of a case, made when a decoder has
    its metadata, armed before every call"""

    def __init__(self, hip, cs, decs):
        self.hip, self.cs, self.decs, self.out = hip, cs, decs, [None] * len(decs)
        self.surface = cs.opts[0].way[0] == "surface"

    def arm(self, ids):
        """(the call's destination arguments, which of the decoders can deliver)"""
        hip, m = self.hip, len(ids)
        ptrs, caps, arr, ready = (C.c_void_p * m)(), (C.c_size_t * m)(), (OUTSURF * m)(), []
        for i, k in enumerate(ids):
            way = self.cs.opts[k].way
            if self.surface:
                dims = surface_dims(hip, self.decs[k], way[1])
                if dims is not None and self.out[k] is None:
                    self.out[k] = OutSurf(dims, way[1], D.pitch_of(way[2]), way[3])
            else:
                pb = hip.dsv2hip_dec_picture_bytes(C.byref(self.decs[k]))
                if pb and self.out[k] is None:
                    self.out[k] = DevOut(pb, 0)
            ready.append(self.out[k] is not None)
            if ready[i]:
                self.out[k].arm()
                if self.surface:
                    arr[i] = self.out[k].c
                else:
                    ptrs[i], caps[i] = self.out[k].ptr(), self.out[k].nbytes
        torch.cuda.synchronize()
        return (arr,) if self.surface else (ptrs, caps), ready

    def untouched(self, k):
        return self.out[k] is None or (self.out[k].untouched() if self.surface else bool(np.all(self.out[k].picture() == 0xA5)))

    def planes(self, k):
        return self.out[k].planes() if self.surface else split_planes(self.out[k].picture(), out_dims(self.decs[k], False))


@pytest.mark.parametrize("entry", ["device", "surface"])
def test_refused_calls_consume_nothing_among_mixed_neighbours(entry):
    """in the step in which the five decoders hand in P pictures and metadata, the call is refused for a NULL decoder in slot 3 and for a
    destination of decoder 0 that is one byte short (device: or NULL): -1, every packet, every decoder and every destination as it
    was -- as test_refused_calls_consume_nothing defines it for one decoder --, and the same buffers then decode to the reference's
    pictures, as do all the steps behind"""
    hip = bind(A.load_hip())
    cs = D.through(D.case("small"), entry)
    n = len(cs.feeds)
    streams = [D.packets(fd) for fd in cs.feeds]
    decs = [A.DECODER() for _ in range(n)]
    dest = Destinations(hip, cs, decs)
    call = hip.dsv2hip_dec_batch_surface if entry == "surface" else hip.dsv2hip_dec_batch_device
    got, refused = [[] for _ in range(n)], 0
    for t, step in enumerate(cs.schedule):
        ids = [k for k, _ in step]
        m = len(ids)
        decp = (C.POINTER(A.DECODER) * m)(*[C.pointer(decs[k]) for k in ids])
        bufs, fns, rets = (A.BUF * m)(), (C.c_uint32 * m)(), (C.c_int * m)()
        for i, (k, p) in enumerate(step):
            mk_buf(hip, bufs[i], streams[k][p])
        args, ready = dest.arm(ids)
        if t == 2:
            assert m == n and ready[0] and {D.kind(streams[k][p]) for k, p in step} == {"P", "M"}
            state = [bytes(C.string_at(C.byref(d), C.sizeof(d))) for d in decs]
            where = [(C.cast(b.data, C.c_void_p).value, b.len) for b in bufs]

            def nothing_happened(what):
                assert [(C.cast(b.data, C.c_void_p).value, b.len) for b in bufs] == where, what
                assert all(bytes(C.string_at(bufs[i].data, len(streams[k][p]))) == streams[k][p] for i, (k, p) in enumerate(step)), what
                assert [bytes(C.string_at(C.byref(d), C.sizeof(d))) for d in decs] == state, what
                assert all(dest.untouched(k) for k in ids), what

            null = (C.POINTER(A.DECODER) * m)(*decp)
            null[3] = None
            assert call(m, null, bufs, *args, fns, rets) == -1
            nothing_happened("a NULL decoder in slot 3")
            refused += 1
            if entry == "surface":
                args[0][0].cap[0] -= 1
                assert call(m, decp, bufs, *args, fns, rets) == -1
                args[0][0].cap[0] += 1
            else:
                args[1][0] -= 1
                assert call(m, decp, bufs, *args, fns, rets) == -1
                args[1][0] += 1
                nothing_happened("a buffer that is too small in slot 0")
                refused += 1
                keep, args[0][0] = args[0][0], None
                assert call(m, decp, bufs, *args, fns, rets) == -1
                args[0][0] = keep
            nothing_happened("a destination that cannot hold the picture in slot 0")
            refused += 1
        assert call(m, decp, bufs, *args, fns, rets) == m
        for i, k in enumerate(ids):
            planes = dest.planes(k) if ready[i] and rets[i] == A.DEC_OK else None
            if planes is None:
                assert dest.untouched(k)
            got[k].append((rets[i], fns[i] if planes is not None else None, planes))
    for d in decs:
        hip.dsv_dec_free(C.byref(d))
    assert refused == (2 if entry == "surface" else 3)
    D.check(cs, dict(enumerate(got)))
