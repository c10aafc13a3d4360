"""Lockstep encoder steps whose streams differ: the cases and the driver shared by tests/test_mixed_steps_ref.py (CPU: the cases
are what they claim, shown on the reference alone) and tests/test_gpu_enc_mixed_steps.py (the library against the reference).

A step only has to agree on what step_key() hashes (csrc/encoder.cpp): picture size, chroma format, block-size overrides, resolved
pyramid depth and do_psy.  Everything else -- quality, effort, rate control, GOP phase, frame-number parity, filters, thresholds,
the metadata's fps and inter_sharpen, the entry point a picture came through -- is per picture.  A stream here is a Spec (hashable:
the reference's packets are computed once per Spec and shared), a case is a list of Specs plus a schedule: schedule[t] is the
ordered list of the streams that take part in step t."""
import collections
import ctypes as C
import functools
import os

import numpy as np

import dsvabi as A
import rgb_csc as R
from codec_run import configure_encoder, encode_stream
from conftest import load_pkg
from hipabi import PLANAR, SEMI, SURFACE, bind

FMT = {"444": (A.SUBSAMP_444, 0, 0), "422": (A.SUBSAMP_422, 1, 0), "420": (A.SUBSAMP_420, 1, 1)}
W, H = 176, 144  # the smallest size at which noise and scene cuts stay inside the reference's packet bound
STAT_KEYS = ("inum", "pnum", "isize", "psize", "eprm", "skip", "mbI", "mbP", "qpx", "hpx")

# w, h, fmt: geometry; seed, nframes: SynthVideo content; cut: index of the frame that is inverted (a scene cut), or None;
# layout: None, or the RGB surface layout that DEFINES the stream's pictures (tests/rgb_csc.py); lie: indices of the frames in front
# of which a host step announces another pointer than the one it then brings; cfg, meta: sorted item tuples of configure_encoder's
# keywords and of mk_meta's fps / inter_sharpen
Spec = collections.namedtuple("Spec", "w h fmt seed nframes cut layout lie cfg meta")


def spec(seed, nframes, cfg, meta=None, w=W, h=H, fmt="420", cut=None, layout=None, lie=()):
    return Spec(w, h, fmt, seed, nframes, cut, layout, tuple(lie), tuple(sorted(cfg.items())), tuple(sorted((meta or {}).items())))


# ---- the configuration table ----------------------------------------------------------------------------------------------
QP = (25, 40, 55, 60, 70, 85, 100)  # 100: lossless
EFFORT = (1, 3, 5, 7, 10)
RC = (0, 1, 2)  # CRF, ABR, CQP
GOP = (0, 1, 2, 3, 5, 12)
SKIP = (-1, 0, 8)
INTER_FILTER = (-1, 0, 1)  # (-1, the default, is "on" with the automatic strength)
FPS = ((30, 1), (25, 1), (60000, 1001))
SCENE_PCT = (85, 60, 40)
INTRA_PCT = (90, 50)
ABR_BITRATE = 150000  # (tests/test_mixed_steps_ref.py: the quantiser of the ABR streams moves at this rate)
NROWS = 14
CUTS = {0: 5, 7: 4, 12: 6}  # row -> the frame that is inverted; P for that row's GOP (tests/test_mixed_steps_ref.py); 12 is lossless
ABR_ROW = 1                 # the ABR row whose quantiser is shown to move against its CRF twin


def pick(vals, s, a, b=0):
    """value of an option for row s: stride a over the values, moved on by one every full turn, so that options with the same
    number of values do not march together"""
    n = len(vals)
    return vals[(a * s + b + s // n) % n]


def row(s):
    """(cfg, meta) of row s of the table"""
    cfg = dict(qp=pick(QP, s, 1), effort=pick(EFFORT, s, 2), rc_mode=pick(RC, s, 1), gop=pick(GOP, s, 1, 3),
               skip_block_thresh=pick(SKIP, s, 2, 1), do_inter_filter=pick(INTER_FILTER, s, 1, 2), do_intra_filter=(s >> 1) & 1,
               do_temporal_aq=s & 1, do_dark_intra_boost=(s >> 2) & 1, do_scd=int(s % 5 != 1), variable_i_interval=int(s % 3 != 2),
               scene_change_pct=pick(SCENE_PCT, s, 2), intra_pct_thresh=pick(INTRA_PCT, s, 1, 1))
    if cfg["rc_mode"] == 1:
        cfg["bitrate"] = ABR_BITRATE
    meta = dict(fps=pick(FPS, s, 1, 1), inter_sharpen=(s >> 3) & 1 ^ (s & 1))
    return cfg, meta


def table_stream(s, nframes=10, seed0=500, cut=True, **kw):
    """row s as a stream; over: configuration keywords that replace the row's (a step key's, a GOP)"""
    cfg, meta = row(s)
    cfg.update(kw.pop("over", {}))
    return spec(seed0 + s, nframes, cfg, meta, cut=CUTS.get(s) if cut else None, **kw)


def everything(n=NROWS):
    return [table_stream(s) for s in range(n)]


def together(streams):
    """every stream in every step, in list order, until its frames run out"""
    T = max(sp.nframes for sp in streams)
    return [[s for s, sp in enumerate(streams) if t < sp.nframes] for t in range(T)]


# ---- staggered joins and leaves --------------------------------------------------------------------------------------------
STAGGER_STEPS = 10


def staggered():
    """8 streams with gop 3: stream s joins at step s; 1 and 4 leave after 4 frames; 2 sits out steps 5 and 6.  A ninth joins at
    step 1 and is the one whose caller breaks the host_next promise (frames 2 and 5)."""
    sched = [[] for _ in range(STAGGER_STEPS)]
    for s in range(8):
        steps = list(range(s, STAGGER_STEPS))
        if s in (1, 4):
            steps = steps[:4]
        if s == 2:
            steps = [t for t in steps if t not in (5, 6)]
        for t in steps:
            sched[t].append(s)
    for t in range(1, STAGGER_STEPS):
        sched[t].append(8)
    for t in range(1, STAGGER_STEPS, 2):  # (slot order is not stream order)
        sched[t].reverse()
    count = [sum(s in step for step in sched) for s in range(9)]
    streams = [table_stream(s, nframes=count[s], seed0=600, cut=False, over=dict(gop=3), lie=(2, 5) if s == 8 else ()) for s in range(9)]
    return streams, sched


# ---- regrouping, alternating entry points -------------------------------------------------------------------------------------
def deal(d, n=12):
    """the two groups of deal d: the streams, rotated by 3 * d, cut in halves; every other deal lists them backwards (slot 0 is
    another stream's each time)"""
    order = [(k + 3 * d) % n for k in range(n)][::-1 if d % 2 else 1]
    return order[:n // 2], order[n // 2:]


def regrouping():
    """12 streams in two groups that are re-dealt after every second step"""
    streams = everything(12)
    return streams, [deal(t // 2) for t in range(streams[0].nframes)]


ENTRY_CYCLE = ("device", "host", "surface", "single", "frame", "device")
SHORT_LIST = 5  # the stream of alternating() that starts with symbol lists too short for its first picture


def alternating():
    """6 streams; streams 3 and 4 are defined by their RGB pictures; stream 5 joins at step 1, one frame short.  352x288: chroma
    rows of 176 bytes -- at 176x144 they have 88, no multiple of 16, and no step with a planar surface could take the wide form of
    the surface ingest (csrc/io_jobs.h: surface_job_wide)."""
    streams = [table_stream(s, nframes=9 if s == SHORT_LIST else 10, layout=RGB_LAYOUTS.get(s % 5), w=352, h=288) for s in range(6)]
    return streams, [[s for s in ((k + t) % 6 for k in range(6)) if s != SHORT_LIST or t >= 1] for t in range(10)]  # (rotated by one slot a step)


# ---- other step keys ---------------------------------------------------------------------------------------------------------
KEY_ROWS = (0, 6, 2, 12, 4)  # rows 6 and 12 are lossless
KEY_CASES = {
    "178x146_420": dict(w=178, h=146),
    "444": dict(fmt="444"),
    "422": dict(fmt="422"),
    "352x288_bsx1": dict(w=352, h=288, over=dict(block_size_override_x=1)),
    "bsx1_bsy1": dict(over=dict(block_size_override_x=1, block_size_override_y=1)),
    "psy0": dict(over=dict(do_psy=0)),
    "64x48_pyr3": dict(w=64, h=48, over=dict(pyramid_levels=3)),
}


def key_case(name):
    kw = dict(KEY_CASES[name])
    over = kw.pop("over", {})
    return [table_stream(s, nframes=6, seed0=700, cut=False, over=dict(over), **kw) for s in KEY_ROWS]


def cases():
    """name -> (streams, [schedule[t] = the groups of step t, each an ordered list of stream ids])"""
    out = {"everything": (everything(), [[ids] for ids in together(everything())]),
           "small": (everything(5), [[ids] for ids in together(everything(5))]),
           "staggered": (staggered()[0], [[ids] for ids in staggered()[1]]),
           "regrouping": (regrouping()[0], [list(groups) for groups in regrouping()[1]]),
           "alternating": (alternating()[0], [[ids] for ids in alternating()[1]]),
           "threads": (everything(8), [[[s] for s in ids] for ids in together(everything(8))])}
    for name in KEY_CASES:
        out["key_" + name] = (key_case(name), [[ids] for ids in together(key_case(name))])
    return out


# ---- content ---------------------------------------------------------------------------------------------------------------
def chroma_dims(w, h, fmt):
    _, hs, vs = FMT[fmt]
    return (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs


@functools.lru_cache(maxsize=None)
def build(sp):
    """the stream of a Spec: dict(frames, meta_kw, cfg, spec, rgb).  rgb: None, or the h x w x 4 pictures whose conversion the
    frames are"""
    code, hs, vs = FMT[sp.fmt]
    v = load_pkg().synth.SynthVideo(sp.w, sp.h, "420" if sp.fmt == "420" else "444", seed=sp.seed)
    frames, rgb = [], None
    if sp.layout is None:
        for t in range(sp.nframes):
            y, u, vv = v.frame(t)
            if sp.fmt == "422":
                u, vv = u[:, ::2], vv[:, ::2]
            fb = y.tobytes() + u.tobytes() + vv.tobytes()
            frames.append(bytes(255 - b for b in fb) if t == sp.cut else fb)
    else:  # colours from a 4:4:4 picture of the same generator: its Y, U, V planes are the R, G, B bytes; alpha is noise
        v4 = load_pkg().synth.SynthVideo(sp.w, sp.h, "444", seed=sp.seed)
        rgb = []
        for t in range(sp.nframes):
            px = np.stack(list(v4.frame(t)) + [np.random.default_rng(sp.seed + t).integers(0, 256, (sp.h, sp.w), dtype=np.uint8)], axis=-1)
            if t == sp.cut:
                px[..., :3] = 255 - px[..., :3]
            px.setflags(write=False)
            rgb.append(px)
            frames.append(R.planar_bytes(px, sp.layout, hs, vs))
    cw, ch = chroma_dims(sp.w, sp.h, sp.fmt)
    assert all(len(f) == sp.w * sp.h + 2 * cw * ch for f in frames)
    return dict(frames=frames, meta_kw=dict(dict(sp.meta), w=sp.w, h=sp.h, subsamp=code), cfg=dict(sp.cfg), spec=sp, rgb=rgb)


# ---- the reference ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(sp):
    st = build(sp)
    pk, stats = encode_stream(A.load_ref(), st["frames"], sp.w, sp.h, FMT[sp.fmt][0], eos=False, meta=A.mk_meta(**st["meta_kw"]), **st["cfg"])
    return tuple(pk), stats


def reference_packets(streams):
    """[(packets, stats)] of the reference encoder on each stream alone"""
    return [_reference(st["spec"]) for st in streams]


@functools.lru_cache(maxsize=None)
def reference_quants(sp):
    """enc.prev_quant behind every picture of the reference's encode: the quantiser the NEXT picture's search is given"""
    ref, st = A.load_ref(), build(sp)
    enc = A.ENCODER()
    configure_encoder(ref, enc, A.mk_meta(**st["meta_kw"]), **st["cfg"])
    bufs, out = (A.BUF * 4)(), []
    for fb in st["frames"]:
        arr = np.frombuffer(fb, dtype=np.uint8).copy()
        for i in range(ref.dsv_enc(C.byref(enc), ref.dsv_load_planar_frame(FMT[sp.fmt][0], arr.ctypes.data, sp.w, sp.h), bufs)):
            ref.dsv_buf_free(C.byref(bufs[i]))
        out.append(enc.prev_quant)
    ref.dsv_enc_free(C.byref(enc))
    return tuple(out)


def picture_types(packets):
    """'I' / 'P' of each picture packet, from the header's type byte (dsv.h: DSV_PT_PIC = 4, bit 0 = has_ref)"""
    return ["P" if p[5] & 1 else "I" for p in packets if p[5] & 4]


def types_per_step(streams, schedule):
    """[[(stream, 'I' / 'P', lossless)]] per step, from the reference's packets"""
    types = [picture_types(_reference(sp)[0]) for sp in streams]
    pos = [0] * len(streams)
    out = []
    for ids in schedule:
        out.append([(s, types[s][pos[s]], dict(streams[s].cfg)["qp"] == 100) for s in ids])
        for s in ids:
            pos[s] += 1
    assert pos == [sp.nframes for sp in streams], "the schedule does not use up every stream"
    return out


def assert_same(want, got, what=""):
    """want: reference_packets(); got: (packets per stream, stats per stream)"""
    assert len(want) == len(got[0]) == len(got[1]) > 0
    for s, ((wp, ws), gp, gs) in enumerate(zip(want, got[0], got[1])):
        assert len(wp) == len(gp), "%s stream %d: %d packets, the reference has %d" % (what, s, len(gp), len(wp))
        for i, (a, b) in enumerate(zip(wp, gp)):
            assert len(a) == len(b), "%s stream %d packet %d: %d bytes, the reference has %d" % (what, s, i, len(b), len(a))
            if a != b:
                d = next(k for k in range(len(a)) if a[k] != b[k])
                raise AssertionError("%s stream %d packet %d (%s) differs at byte %d of %d" % (what, s, i, "P" if a[5] & 1 else "I", d, len(a)))
        assert ws == gs, "%s stream %d: stats %r, the reference has %r" % (what, s, gs, ws)


# ---- the driver ------------------------------------------------------------------------------------------------------------
class env:
    """os.environ with some variables set, as tests/test_gpu_compact_lists.py has it"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


SURFACE_KINDS = ("packed", "planar", "semiplanar", "bgra601", "rgba709full")
RGB_LAYOUTS = {3: R.BGRA | R.BT601, 4: R.RGBA | R.BT709 | R.FULL}  # stream index % 5 -> the layout that defines its pictures


def slot(bufs, k):
    """the four DSV_BUFs of the step's k-th stream"""
    return C.cast(C.addressof(bufs) + 4 * k * C.sizeof(A.BUF), C.POINTER(A.BUF))


def up16(x):
    return (x + 15) & ~15


def make_surface(st, s, t, general):
    """stream index s's picture t as the device surface of kind s % 5; general: off the 16-byte grid (the ingests' general forms)"""
    from enc_in import RgbSurface, Surface
    sp, kind = st["spec"], s % 5
    w, h = sp.w, sp.h
    cw, _ = chroma_dims(w, h, sp.fmt)
    if kind in RGB_LAYOUTS:
        assert sp.layout == RGB_LAYOUTS[kind], "stream %d goes in as an RGB surface: its Spec must carry that layout" % s
        if general:
            return RgbSurface(st["rgb"][t], sp.layout, pitch=(4 * w + 3) | 1, offset=1 + s % 3)
        return RgbSurface(st["rgb"][t], sp.layout, pitch=up16(4 * w) + 16)
    fb = st["frames"][t]
    if kind == 0:
        return Surface(fb, w, h, sp.fmt, layout=PLANAR, pitches=(w, cw, cw))
    rows = (w, 2 * cw) if kind == 2 else (w, cw, cw)
    if general:
        return Surface(fb, w, h, sp.fmt, layout=SEMI if kind == 2 else PLANAR, pitches=tuple((rb + 3) | 1 for rb in rows), offsets=(1, 2, 3))
    return Surface(fb, w, h, sp.fmt, layout=SEMI if kind == 2 else PLANAR, pitches=tuple(up16(rb) + 16 for rb in rows))


class Runner:
    """One encoder per stream, made when the stream first takes part in a step; step(ids, kind) runs one lockstep step (or one
    call per stream for "single" / "frame") over the listed streams' next pictures.  Per-stream state only: steps over disjoint
    sets of streams may run on different threads."""

    def __init__(self, hip, streams):
        self.hip, self.streams = bind(hip), streams
        n = len(streams)
        self.encs, self.pos, self.got = [None] * n, [0] * n, [[] for _ in range(n)]
        self.pinned, self.decoy = [None] * n, [None] * n
        self.surface_steps = 0

    def encoder(self, s):
        if self.encs[s] is None:
            self.encs[s] = A.ENCODER()
            configure_encoder(self.hip, self.encs[s], A.mk_meta(**self.streams[s]["meta_kw"]), **self.streams[s]["cfg"])
        return self.encs[s]

    def host_picture(self, s, t, announced=False):
        """pinned address of stream s's picture t; announced: what host_next says of it -- for a picture the caller lies about,
        another block that holds the inverted picture"""
        st = self.streams[s]
        P, lie = len(st["frames"][0]), st["spec"].lie
        if self.pinned[s] is None:
            self.pinned[s] = self.hip.dsv2hip_host_alloc(P * (len(st["frames"]) + len(lie)))
            assert self.pinned[s]
            for k, fb in enumerate(st["frames"]):
                C.memmove(self.pinned[s] + k * P, fb, P)
            for k, f in enumerate(lie):
                C.memmove(self.pinned[s] + (len(st["frames"]) + k) * P, bytes(255 - b for b in st["frames"][f]), P)
        if announced and t in lie:
            return self.pinned[s] + (len(st["frames"]) + lie.index(t)) * P
        return self.pinned[s] + t * P

    def step(self, ids, kind):
        import torch
        hip, n = self.hip, len(ids)
        encs = [self.encoder(s) for s in ids]
        fr = [self.streams[s]["frames"][self.pos[s]] for s in ids]
        encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
        bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)()
        if kind in ("device", "single"):
            dev = [torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() for f in fr]
            torch.cuda.synchronize()  # (the tensors are built on torch's stream, the encoder runs on its own)
            if kind == "device":
                assert hip.dsv2hip_enc_batch(n, encp, (C.c_void_p * n)(*[d.data_ptr() for d in dev]), bufs, nbufs) == 0
            else:
                for k in range(n):
                    nbufs[k] = hip.dsv2hip_enc_device_frame(C.byref(encs[k]), dev[k].data_ptr(), slot(bufs, k))
        elif kind == "host":
            cur = (C.c_void_p * n)(*[self.host_picture(s, self.pos[s]) for s in ids])
            nxt = (C.c_void_p * n)(*[self.host_picture(s, self.pos[s] + 1, announced=True) if self.pos[s] + 1 < len(self.streams[s]["frames"]) else None
                                     for s in ids])
            assert hip.dsv2hip_enc_batch_host(n, encp, cur, nxt, bufs, nbufs) == 0
        elif kind == "surface":
            general = self.surface_steps % 2 == 1
            self.surface_steps += 1
            surfs = [make_surface(self.streams[s], s, self.pos[s], general) for s in ids]
            torch.cuda.synchronize()
            assert hip.dsv2hip_enc_batch_surface(n, encp, (SURFACE * n)(*[sf.c for sf in surfs]), bufs, nbufs) == 0
            for sf in surfs:
                sf.check_untouched()
        elif kind == "frame":
            for k, s in enumerate(ids):
                sp = self.streams[s]["spec"]
                arr = np.frombuffer(fr[k], dtype=np.uint8).copy()
                f = hip.dsv_load_planar_frame(FMT[sp.fmt][0], arr.ctypes.data, sp.w, sp.h)
                nbufs[k] = hip.dsv_enc(C.byref(encs[k]), f, slot(bufs, k))
        else:
            raise ValueError(kind)
        for k, s in enumerate(ids):
            assert 1 <= nbufs[k] <= 4, "stream %d: %d packets from a %s step" % (s, nbufs[k], kind)
            for i in range(nbufs[k]):
                b = bufs[4 * k + i]
                self.got[s].append(bytes(C.string_at(b.data, b.len)))
                hip.dsv_buf_free(C.byref(b))
            self.pos[s] += 1

    def finish(self):
        """(packets per stream, stats per stream); frees the encoders and the pinned pictures"""
        stats = []
        for s, e in enumerate(self.encs):
            stats.append(None if e is None else {k: getattr(e.stats, k) for k in STAT_KEYS})
            if e is not None:
                self.hip.dsv_enc_free(C.byref(e))
            if self.pinned[s]:
                self.hip.dsv2hip_host_free(self.pinned[s])
        self.encs = [None] * len(self.encs)
        return self.got, stats


def run_schedule(hip, streams, schedule, entry, step_env=None):
    """schedule[t]: the ordered stream ids of step t; entry(t): "device" (dsv2hip_enc_batch), "host" (dsv2hip_enc_batch_host on
    pinned pictures, host_next = each stream's next picture, whichever step that comes in), "surface" (dsv2hip_enc_batch_surface;
    the layout cycles over the stream index through SURFACE_KINDS, every other surface step off the 16-byte grid), "single" (one
    dsv2hip_enc_device_frame per stream) or "frame" (one dsv_enc per stream); step_env(t): None, or the environment variables set
    while step t runs (an encoder is made in the first step that lists it).  Returns (packets per stream, stats per stream)."""
    run = Runner(hip, streams)
    for t, ids in enumerate(schedule):
        if not ids:
            continue
        with env(**((step_env(t) if step_env else None) or {})):
            run.step(ids, entry(t))
    return run.finish()
