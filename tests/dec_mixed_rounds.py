"""Lockstep decoder rounds whose streams differ: the cases and the driver shared by tests/test_dec_mixed_rounds_ref.py (CPU: the
cases are what they claim, shown on the reference alone) and tests/test_gpu_dec_mixed_rounds.py (the library against the reference).

A round (csrc/decoder.cpp: dec_device_round) only has to agree on picture size, chroma format and block size.  The quantiser, the
filter switch, the metadata's inter_sharpen, lossless or not, I or P, the frame-number parity, the parser, the symbol-list lengths,
the damaged planes and the way out are per picture and reach the kernels through the round's job tables.  A decoder here is a Feed
(the reference encoder's packets of one or more mixed_steps.Specs, some of them damaged), a case is a list of Feeds, a schedule --
schedule[t] is the ordered [(decoder, packet index)] of step t; it counts PACKETS, so metadata and end-of-stream packets share steps
with the neighbours' pictures -- and the options of each decoder: draw_info, postsharp, out420p and its way out."""
import collections
import ctypes as C
import functools

import numpy as np

import dsvabi as A
import mixed_steps as M

# parts: the Specs whose packets follow one another (no end-of-stream packet in between); damage: None, or (seed, the ordinals of the
# pictures that are damaged); eos: an end-of-stream packet behind the last part; pick: None, or the indices of the packets that are
# handed in, in that order (a P picture in front of its reference picture)
Feed = collections.namedtuple("Feed", "parts damage eos pick")
# way: ("frame",) a pinned DSV_FRAME; ("packed",) the packed device buffer; ("surface", layout, pitch name, offset)
Opt = collections.namedtuple("Opt", "draw sharp out420p way")
Case = collections.namedtuple("Case", "name feeds schedule opts")

FRAME, PACKED = ("frame",), ("packed",)
PLAIN = Opt(0, False, False, FRAME)
DRAW_ALL = 7  # DSV_DRAW_STABHQ | DSV_DRAW_MOVECS | DSV_DRAW_IBLOCK
PLANAR, SEMI, HALF, QUARTER, EIGHTH = 0, 1, 0x1000, 0x2000, 0x3000  # include/dsv2_hip.h: DSV2HIP_SURFACE_*, DSV2HIP_SCALE_*


def feed(*parts, damage=None, eos=True, pick=None):
    return Feed(tuple(parts), damage, eos, pick)


# ---- packets -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eos_packet():
    """the reference encoder's end-of-stream packet (it carries nothing of the stream)"""
    from codec_run import configure_encoder
    ref, enc, bufs = A.load_ref(), A.ENCODER(), (A.BUF * 4)()
    configure_encoder(ref, enc, A.mk_meta(M.W, M.H, A.SUBSAMP_420))
    ref.dsv_enc_end_of_stream(C.byref(enc), bufs)
    pk = bytes(C.string_at(bufs[0].data, bufs[0].len))
    ref.dsv_buf_free(C.byref(bufs[0]))
    ref.dsv_enc_free(C.byref(enc))
    assert pk[5] == 0x10  # dsv.h: DSV_PT_EOS
    return pk


def kind(pk):
    """'M' metadata, 'I' / 'P' picture, 'E' end of stream (dsv.h: the packet type at byte 5, DSV_PT_PIC = 4, bit 0 = has_ref)"""
    return ("P" if pk[5] & 1 else "I") if pk[5] & 4 else "E" if pk[5] == 0x10 else "M"


def damaged(pk, rng, count):
    """the recipe of tests/test_gpu_robustness.py::test_damaged_plane_data: bytes altered in the second half of a picture packet"""
    b = bytearray(pk)
    for _ in range(count):
        i = int(rng.integers(len(b) // 2, len(b) - 8))
        b[i] ^= int(rng.integers(1, 256))
    return bytes(b)


@functools.lru_cache(maxsize=None)
def clean_packets(fd):
    out = [pk for sp in fd.parts for pk in M._reference(sp)[0]]
    return tuple(out + [eos_packet()] if fd.eos else out)


@functools.lru_cache(maxsize=None)
def packets(fd):
    """the packets a decoder is fed (shared, never modified)"""
    out = list(clean_packets(fd))
    if fd.damage is not None:
        seed, which = fd.damage
        rng = np.random.default_rng(seed)
        pics = [i for i, pk in enumerate(out) if pk[5] & 4]
        for n in which:
            out[pics[n]] = damaged(out[pics[n]], rng, 1 + (seed + n) % 3)
    return tuple(out if fd.pick is None else [out[i] for i in fd.pick])


class Bits:
    def __init__(self, data, at):
        self.data, self.at = data, 8 * at

    def bit(self):
        b = (self.data[self.at >> 3] >> (7 - (self.at & 7))) & 1
        self.at += 1
        return b

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def ueg(self):  # the interleaved exp-Golomb code (bs.c:132)
        v = 1
        while not self.bit():
            v = (v << 1) | self.bit()
        return v - 1

    def align(self):
        self.at = (self.at + 7) & ~7


def picture_header(pk):
    """dict(type, fno, blk_w, blk_h, do_filter, quant, lossless) of a picture packet (dsv_decoder.c:393-470): 14 bytes of packet
    header, the frame number, the block-size exponents, three statistics bits, the filter switch, the quantiser"""
    assert pk[:4] == b"DSV2" and pk[5] & 4
    br = Bits(pk, 14)
    fno = br.bits(32)
    ew, eh = br.ueg(), br.ueg()
    br.align()
    br.bits(3)
    do_filter, quant = br.bit(), br.bits(12)  # dsv.h: DSV_MAX_QP_BITS
    return dict(type=kind(pk), fno=fno, blk_w=16 << ew, blk_h=16 << eh, do_filter=do_filter, quant=quant, lossless=int(quant == 1))


# ---- the reference -------------------------------------------------------------------------------------------------------------
def geometry(fd):
    """(w, h, fmt) of the feed's first part"""
    return fd.parts[0].w, fd.parts[0].h, fd.parts[0].fmt


@functools.lru_cache(maxsize=None)
def reference(fd, draw=0, sharp=False):
    """the reference decoder's [(return code, frame number or None, [Y, U, V] or None)] per packet of the feed, with the reference's
    own overlay and -- tests/dec_out.py: expected_sharp -- its own dsv_post_process on the luma (shared, never modified)"""
    from dec_out import decode
    A.load_ref().dsv_set_log_level(0)  # (the reference reports every damaged plane)
    if sharp:
        from dec_out import expected_sharp
        res = expected_sharp(A.load_ref(), packets(fd), mode=draw, sharp=True)
    else:
        res = decode(A.load_ref(), packets(fd), draw)
    for _, _, pl in res:
        for p in pl or ():
            p.setflags(write=False)
    return tuple(res)


def digest(results):
    """the results as plain data: [[return code, frame number, sha1 of the planes or None]]"""
    import hashlib
    return [[code, fn, None if pl is None else hashlib.sha1(b"".join(p.tobytes() for p in pl)).hexdigest()] for code, fn, pl in results]


def child_report(fd):
    """for a fresh child process, on stdout: the reference's own log (level ERROR: "decoding error in plane N" for every plane its plane
    decoder refuses, dsv_decoder.c:516-523) with a line "packet N" in front of every packet, then "result " and the digest of
    reference(fd) as JSON"""
    import json
    import os
    from dec_out import decode
    ref, libc = A.load_ref(), C.CDLL(None)
    ref.dsv_set_log_level(1)
    dec = A.DECODER()
    for i, pk in enumerate(packets(fd)):
        libc.fflush(None)  # (the log goes through C's buffered stdout)
        os.write(1, b"\npacket %d\n" % i)
        buf, fp, fn = A.BUF(), C.POINTER(A.FRAME)(), C.c_uint32(0)
        ref.dsv_mk_buf(C.byref(buf), len(pk) + 64)
        C.memmove(buf.data, pk, len(pk))
        code = ref.dsv_dec(C.byref(dec), C.byref(buf), C.byref(fp), C.byref(fn))
        if code == A.DEC_OK and fp:
            ref.dsv_frame_ref_dec(fp)
    ref.dsv_dec_free(C.byref(dec))
    libc.fflush(None)
    ref.dsv_set_log_level(0)
    os.write(1, b"\nresult " + json.dumps(digest(decode(ref, packets(fd), 0))).encode() + b"\n")


def refused_planes(log):
    """{packet index: [planes refused]} from child_report's log"""
    out, at = {}, None
    for line in log.splitlines():
        if line.startswith("packet "):
            at = int(line.split()[1])
        elif "decoding error in plane" in line:
            out.setdefault(at, []).append(int(line.split("decoding error in plane")[1].split()[0]))
    return out


def wanted(fd, opt):
    """what decoder (fd, opt) must deliver, per packet: the reference's decode with the post-steps of the existing CPU models, as the
    planes of the way out.  -out420p on a 4:2:0 stream changes nothing (dsv_main.c:1030-1048 converts no 4:2:0 picture), and these
    cases switch it on for 4:2:0 streams only."""
    want = reference(fd, opt.draw, opt.sharp)
    if opt.out420p:
        assert all(sp.fmt == "420" for sp in fd.parts)
    if opt.way[0] == "surface":
        from dec_out import in_layout
        assert len(set(sp.fmt for sp in fd.parts)) == 1
        return in_layout(want, opt.way[1], geometry(fd)[2])
    return want


def assert_same(name, k, fd, want, got):
    """per packet: the return code, the frame number and every delivered plane (the helpers have checked the guard bytes)"""
    pk = packets(fd)
    assert len(want) == len(got), "%s decoder %d: %d results, the reference has %d" % (name, k, len(got), len(want))
    for i, ((cw, fw, pw), (cg, fg, pg)) in enumerate(zip(want, got)):
        what = "%s decoder %d packet %d (%s)" % (name, k, i, kind(pk[i]))
        assert cw == cg, "%s: return code %d, the reference gives %d" % (what, cg, cw)
        assert (pw is None) == (pg is None), "%s: %s, the reference has %s" % (what, *("no picture" if p is None else "a picture" for p in (pg, pw)))
        if pw is None:
            continue
        assert fw == fg, "%s: frame number %r, the reference gives %r" % (what, fg, fw)
        assert len(pw) == len(pg), "%s: %d planes, %d expected" % (what, len(pg), len(pw))
        for c, (a, b) in enumerate(zip(pw, pg)):
            assert a.shape == b.shape, "%s plane %d: shape %r, expected %r" % (what, c, b.shape, a.shape)
            if not np.array_equal(a, b):
                y, x = np.argwhere(a != b)[0]
                raise AssertionError("%s plane %d differs in %d of %d bytes, first at row %d byte %d" % (what, c, int(np.sum(a != b)), a.size, y, x))


def check(case, got):
    assert sorted(got) == list(range(len(case.feeds)))
    for k, (fd, opt) in enumerate(zip(case.feeds, case.opts)):
        assert_same(case.name, k, fd, wanted(fd, opt), got[k])


# ---- schedules -----------------------------------------------------------------------------------------------------------------
def together(feeds, order="order"):
    """packet t of every decoder that still has one in step t: in list order, reversed, or rotated by one slot a step"""
    n, lens = len(feeds), [len(packets(fd)) for fd in feeds]
    out = []
    for t in range(max(lens)):
        ids = list(range(n))
        ids = ids[::-1] if order == "reversed" else ids[t % n:] + ids[:t % n] if order == "rotated" else ids
        out.append(tuple((k, t) for k in ids if t < lens[k]))
    return tuple(out)


def staggered_schedule(feeds):
    """decoder s joins at step s (8, the ninth, at step 1) and hands in a packet a step until it has none left -- 1 and 4 are short
    and leave early; 2 sits out steps 5 and 6; every second step is reversed"""
    lens, at, out, t = [len(packets(fd)) for fd in feeds], [0] * len(feeds), [], 0
    while any(a < n for a, n in zip(at, lens)):
        ids = [s for s in range(len(feeds)) if t >= (1 if s == 8 else s) and at[s] < lens[s] and not (s == 2 and t in (5, 6))]
        step = [(s, at[s]) for s in (ids[::-1] if t % 2 else ids)]
        for s in ids:
            at[s] += 1
        out.append(tuple(step))
        t += 1
    return tuple(out)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
ORDERS = ("order", "reversed", "rotated")
# damaged neighbours: decoder -> (seed, the pictures damaged).  Row 2 is I P P ..., row 6 (lossless) I P P P P I P P P P: each damages
# I and P pictures, and every picture behind the first damaged one is decoded on top of a damaged reference picture.  The seeds are
# chosen, on the CPU (tests/test_dec_mixed_rounds_ref.py asserts it), so that the reference's plane decoder REFUSES luma and chroma
# planes, in I and in P pictures, and every damaged picture differs from its clean decode.
DAMAGE = {2: (3, (0, 3, 4)), 6: (5, (2, 5, 7))}
CHANGE_POINTS = ((3, 4, 3), (4, 4, 3), (5, 5), (2, 8))


def retuned(sp, **meta):
    return sp._replace(meta=tuple(sorted(dict(dict(sp.meta), **meta).items())))


def change_feeds():
    """four decoders whose stream parameters change under them (csrc/decoder.cpp: dec_parse rebuilds the device instance), at points
    that differ per decoder, and two plain neighbours"""
    bs = dict(block_size_override_x=1, block_size_override_y=1)
    a, b, c, d = CHANGE_POINTS
    part = lambda row, n, k, **kw: M.table_stream(row, nframes=n, seed0=1000 + 20 * k, cut=False, **kw)
    size = feed(part(1, a[0], 0), part(1, a[1], 1, w=178, h=146), part(1, a[2], 2), eos=True)
    block = feed(part(2, b[0], 3), part(2, b[1], 4, over=bs), part(2, b[2], 5))
    fmt = feed(part(11, c[0], 6), part(11, c[1], 7, fmt="422"))
    meta = feed(retuned(part(0, d[0], 8), inter_sharpen=0, fps=(30, 1)), retuned(part(0, d[1], 9), inter_sharpen=1, fps=(25, 1)))
    return [size, feed(part(6, 10, 10)), block, fmt, feed(part(7, 10, 11)), meta]


def ways_out():
    """ten deliveries (tests/test_gpu_dec_surface.py: test_every_delivery_in_one_round), each on a stream of its own"""
    import yuv_rgb as Q
    return [PLAIN, Opt(DRAW_ALL, True, False, FRAME), Opt(0, False, True, FRAME), Opt(0, False, False, PACKED),
            Opt(0, False, False, ("surface", PLANAR, "plus1", 1)), Opt(0, False, False, ("surface", SEMI, "aligned", 0)),
            Opt(0, True, False, ("surface", SEMI | HALF, "tight", 0)), Opt(0, False, False, ("surface", Q.BGRA | Q.BT709, "aligned", 0)),
            Opt(0, False, False, ("surface", Q.RGBA | QUARTER, "tight", 0)), Opt(0, False, False, ("surface", PLANAR | EIGHTH, "tight", 0))]


@functools.lru_cache(maxsize=None)
def case(name, order="order"):
    if name in ("everything", "small"):
        feeds = [feed(sp) for sp in M.everything(M.NROWS if name == "everything" else 5)]
        return Case("%s/%s" % (name, order), feeds, together(feeds, order), [PLAIN] * len(feeds))
    if name == "staggered":
        feeds = [feed(sp) for sp in M.staggered()[0]]
        return Case(name, feeds, staggered_schedule(feeds), [PLAIN] * len(feeds))
    if name == "damaged":
        feeds = [feed(sp, damage=DAMAGE.get(s)) for s, sp in enumerate(M.everything(8))]
        return Case(name, feeds, together(feeds), [PLAIN] * len(feeds))
    if name == "ways":
        bw, bh, _, _ = A.block_geometry(M.W, M.H)
        assert M.W % bw == 0 and M.H % bh == 0  # block-aligned: the reference's unchecked intra marks stay inside the luma plane (tests/test_gpu_dec_batch.py)
        feeds = [feed(M.table_stream(s, nframes=6, seed0=900, cut=False)) for s in range(10)]
        return Case(name, feeds, together(feeds), ways_out())
    if name.startswith("key_"):
        feeds = [feed(sp) for sp in M.key_case(name[4:])]
        return Case(name, feeds, together(feeds, "rotated"), [PLAIN] * len(feeds))
    if name == "two_rounds":
        bs = dict(block_size_override_x=1, block_size_override_y=1)
        feeds = [feed(M.table_stream(s, nframes=6, seed0=950, cut=False, over=bs if k % 2 else {})) for k, s in enumerate((0, 2, 6, 12, 1, 11))]
        return Case(name, feeds, together(feeds), [PLAIN] * len(feeds))
    if name == "change":
        feeds = change_feeds()
        return Case(name, feeds, together(feeds), [PLAIN] * len(feeds))
    if name == "orphan":  # the first five rows and, in slot 2, a decoder that gets metadata, a P picture (no reference yet: DSV_DEC_ERROR), then the stream
        late = feed(M.table_stream(1, seed0=960, cut=False), pick=(0, 2) + tuple(range(1, 12)))
        feeds = [feed(sp) for sp in M.everything(5)]
        feeds.insert(2, late)
        return Case(name, feeds, together(feeds), [PLAIN] * len(feeds))
    if name == "threads":
        feeds = [feed(sp) for sp in M.everything(8)]
        return Case(name, feeds, (), [PLAIN] * len(feeds))
    raise ValueError(name)


KEYS = ("178x146_420", "444", "422", "352x288_bsx1", "bsx1_bsy1", "64x48_pyr3")
NAMES = ("everything", "small", "staggered", "damaged", "ways", "two_rounds", "change", "orphan", "threads") + tuple("key_" + k for k in KEYS)


def through(cs, entry):
    """the case with every decoder's way out replaced: "frame" (dsv2hip_dec_batch), "device" (dsv2hip_dec_batch_device) or "surface"
    (dsv2hip_dec_batch_surface: planar at an odd pitch and address and NV12 on the 16-byte grid alternate)"""
    way = {"frame": lambda k: FRAME, "device": lambda k: PACKED,
           "surface": lambda k: ("surface", SEMI, "aligned", 0) if k % 2 else ("surface", PLANAR, "plus1", 1)}[entry]
    return cs._replace(name="%s/%s" % (cs.name, entry), opts=[o._replace(way=way(k)) for k, o in enumerate(cs.opts)])


# ---- what a step holds (for the CPU module) ------------------------------------------------------------------------------------------
def step_table(cs):
    """per step: [dict(k, packet, kind, and for a picture the header's fields plus inter_sharpen)] in slot order"""
    sharpen = []
    for fd in cs.feeds:
        per = []
        for sp in fd.parts:
            per += [dict(sp.meta).get("inter_sharpen", 1)] * len(M._reference(sp)[0])
        sharpen.append(per + [None] * fd.eos)
    out = []
    for step in cs.schedule:
        row = []
        for k, p in step:
            pk = packets(cs.feeds[k])[p]
            e = dict(k=k, packet=p, kind=kind(pk))
            if pk[5] & 4:
                e.update(picture_header(clean_packets(cs.feeds[k])[p]), inter_sharpen=sharpen[k][p])
            row.append(e)
        out.append(row)
    return out


def slices(row):
    """the pictures of a step as round_sort (csrc/decoder.cpp) orders them: [(class, [entries])], classes P-lossless, P, I-lossless, I"""
    pics = [e for e in row if e["kind"] in "IP"]
    cls = lambda e: 2 * (e["kind"] == "P") + e["lossless"]
    return [(c, [e for e in pics if cls(e) == c]) for c in (3, 2, 1, 0) if any(cls(e) == c for e in pics)]


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def pitch_of(name):
    import dec_out as G
    return {"tight": G.tight, "plus1": G.plus1, "aligned": G.aligned}[name]


def run(hip, cs, single=False):
    """Feeds the case's schedule to one decoder per feed.  A step is one call per kind of destination that occurs in it (the ABI has
    an entry point per kind): dsv2hip_dec_batch for the pinned frames, dsv2hip_dec_batch_device for the packed buffers,
    dsv2hip_dec_batch_surface for the surfaces -- or, single, one dsv_dec / dsv2hip_dec_device_frame / dsv2hip_dec_surface_frame per
    packet.  The decoders of one kind run their whole schedule before the next kind's, as in test_every_delivery_in_one_round.
    Returns {decoder: [(return code, frame number or None, planes or None)] per packet}."""
    from dec_out import Surfaces, decode_steps, device_decode, frame_decode
    got = {}
    for what in ("frame", "packed", "surface"):
        ids = [k for k, o in enumerate(cs.opts) if o.way[0] == what]
        if not ids:
            continue
        local = {k: i for i, k in enumerate(ids)}
        sched = [[(local[k], p) for k, p in step if k in local] for step in cs.schedule]
        streams, opts = [packets(cs.feeds[k]) for k in ids], [cs.opts[k] for k in ids]
        kw = dict(modes=[o.draw for o in opts], sharp=[o.sharp for o in opts], schedule=sched, single=single)
        if what == "frame":
            res = frame_decode(hip, streams, out420p=[o.out420p for o in opts], **kw)
        elif what == "packed":
            res = device_decode(hip, streams, out420p=[o.out420p for o in opts], **kw)
        else:
            assert not any(o.out420p for o in opts)
            res = decode_steps(hip, streams, Surfaces([dict(layout=o.way[1], pitch=pitch_of(o.way[2]), offset=o.way[3]) for o in opts]), **kw)
        got.update({k: res[local[k]] for k in ids})
    return got


def run_threads(hip, cs):
    """one thread per decoder, each looping plain dsv_dec over its own packets: the submit queue (csrc/decoder.cpp: g_dec_queue) forms
    the steps"""
    import threading
    from dec_out import frame_decode
    got, errors, start = {}, [], threading.Barrier(len(cs.feeds))

    def work(k):
        try:
            start.wait()
            got[k] = frame_decode(hip, [packets(cs.feeds[k])], [cs.opts[k].draw], [cs.opts[k].sharp], single=True)[0]
        except BaseException as e:  # noqa: B902 (reported by the main thread)
            errors.append((k, e))

    ths = [threading.Thread(target=work, args=(k,)) for k in range(len(cs.feeds))]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors
    return got
