"""Long motion: pictures that pan by 20 - 57 pixels a frame, so that the level-0 search works with vectors beyond +-31 px, with
candidates that point off the padded picture and with refinement walks that stop at its border.  The cases and helpers shared by
tests/test_long_motion_ref.py (CPU: the oracle against the reference, and the cases are what they claim, shown on the reference
alone) and tests/test_gpu_long_motion.py (the library against the reference).

A scene is a window of a canvas of low-passed hash noise (the texture of the package's SynthVideo, with a coarser band, which the
search can follow down the pyramid without a previous field, and more fine detail); the previous picture is the window moved by
the pan, so the true vector of every block is -pan.  A fifth of the picture (band_columns) is the same in both frames: zero and
skipped vectors sit beside the long ones."""
import collections
import ctypes as C
import functools

import numpy as np

import dsvabi as A
from codec_run import encode_stream
from conftest import load_pkg
from edge_cases import degrade
from hme_common import Scene

PANS = [(24, 0), (0, -20), (-40, 28), (57, -45), (-33, -33)]
FAST_PANS = [(-40, 28), (57, -45), (-33, -33)]  # every one has a component beyond 32 px
PREV_KINDS = (None, "long", "limit")
# (effort, quant, skip_block_thresh): the search branches at efforts 4, 6 and 8
CONFIGS = [(10, 172, 0), (5, 61, 8), (7, 900, -1), (3, 300, 0)]

FLAG_INTRA, FLAG_SKIP = 1 << 0, 1 << 3  # dsv_internal.h: DSV_MODE_INTRA, DSV_IS_SKIP (as tests/test_oracle_bmc.py sets them)


def blocks(w, h, bw, bh):
    return (bw, bh, (w + bw - 1) // bw, (h + bh - 1) // bh)


# name -> (w, h, subsamp, blk or None for the encoder's own rule): each reaches another routine of the search
GEOMETRIES = collections.OrderedDict([
    ("352x288", (352, 288, A.SUBSAMP_420, None)),                             # fast 16 x 16
    ("354x290", (354, 290, A.SUBSAMP_420, None)),                             # the general routine on the clipped edge
    ("352x288-444", (352, 288, A.SUBSAMP_444, None)),                         # fast
    ("640x360-422", (640, 360, A.SUBSAMP_422, None)),                         # general at level 0
    ("352x288-b32x16", (352, 288, A.SUBSAMP_420, blocks(352, 288, 32, 16))),  # hme_fast32.h, two quadrants
    ("352x288-b32x32", (352, 288, A.SUBSAMP_420, blocks(352, 288, 32, 32))),  # hme_fast32.h, four quadrants
    ("352x288-b16x32", (352, 288, A.SUBSAMP_420, blocks(352, 288, 16, 32))),  # the general routine
    ("336x280-b32x16", (336, 280, A.SUBSAMP_420, blocks(336, 280, 32, 16))),  # last column 16 wide, last row 8 high: still fast 32 x 16
    ("178x146", (178, 146, A.SUBSAMP_420, None)),                             # three pyramid levels
])
FULL_SIZES = collections.OrderedDict([  # their natural block sizes: 32 x 16 and 32 x 32
    ("1920x800", (1920, 800, A.SUBSAMP_420, None)),
    ("2560x1440", (2560, 1440, A.SUBSAMP_420, None)),
])

Case = collections.namedtuple("Case", "geom pan prev effort quant skip")


def case_id(c):
    return "%s-pan%+d%+d-%s-e%d-q%d-s%d" % (c.geom, c.pan[0], c.pan[1], c.prev or "noprev", c.effort, c.quant, c.skip)


def stage_cases():
    """every small geometry x every pan x every kind of previous field; the configuration moves on by one from case to case, so
    every geometry meets all four; then one case at each full size"""
    out = []
    for g, name in enumerate(GEOMETRIES):
        for p, pan in enumerate(PANS):
            for k, prev in enumerate(PREV_KINDS):
                out.append(Case(name, pan, prev, *CONFIGS[(g + p + k) % len(CONFIGS)]))
    out.append(Case("1920x800", (57, -45), "long", *CONFIGS[0]))
    out.append(Case("2560x1440", (-40, 28), "limit", *CONFIGS[1]))
    return out


STAGE_CASES = stage_cases()
ALT_FORM_CASES = [c for c in STAGE_CASES if c.geom in ("352x288", "352x288-b32x32")]  # run under the library's other forms


def find_case(geom, pan, prev):
    return next(c for c in STAGE_CASES if (c.geom, c.pan, c.prev) == (geom, pan, prev))


BMC_CASES = [find_case("352x288", (57, -45), "long"), find_case("352x288-b32x16", (-40, 28), "limit"), find_case("640x360-422", (-33, -33), None)]


# ---- content ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def canvas(ch, cw, seed, fine=False):
    """ch x cw bytes of hash noise in three bands, box means of radius 16, 6 and 1; fine: in two, of radius 4 and 1 -- a texture
    that the search loses at 33 pixels a frame without a previous field to start from"""
    synth = load_pkg().synth
    n = (synth._hash2d(ch, cw, seed) >> np.uint32(24)).astype(np.int32)
    band = lambda r: synth._box_blur(n, r) - 128
    a = np.clip(128 + (band(4) * 6 if fine else band(16) * 16 + band(6) * 6) + band(1) // 2, 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a


def window(w, h, off, pad, seed, fine=False):
    """(Y, U, V) at full resolution: the w x h window of the three canvases whose corner is `off` from the padded origin"""
    x, y = pad + off[0], pad + off[1]
    assert 0 <= x and 0 <= y
    return [canvas(h + 2 * pad, w + 2 * pad, seed + 101 * c, fine)[y:y + h, x:x + w] for c in range(3)]


def decimate(full, subsamp):
    hs, vs = A.format_shifts(subsamp)
    return (full[0].copy(), full[1][::1 << vs, ::1 << hs].copy(), full[2][::1 << vs, ::1 << hs].copy())


def band_columns(w, pan):
    """the static band: a fifth of the picture's columns, at the left edge -- at the right one where the pan uncovers the left"""
    return slice(w - w // 5, w) if pan[0] > 0 else slice(0, w // 5)


def pan_planes(w, h, subsamp, pan, seed):
    """(current, previous, degraded previous) pictures on the format's chroma grid; current(x, y) = previous(x - pan) outside the
    static band"""
    pad = max(abs(pan[0]), abs(pan[1]))
    cur = [p.copy() for p in window(w, h, (0, 0), pad, seed)]
    prev = [p.copy() for p in window(w, h, pan, pad, seed)]
    # The strip of the current picture that the pan uncovers has no counterpart in the previous one.  In the upper half of a
    # vertical strip and the left half of a horizontal one it shows a smear: the previous picture's edge sample, which is what the
    # border extension puts there.  Those blocks are predicted best from wholly outside the picture, by the pan's own vector.
    yy, xx = np.mgrid[0:h, 0:w]
    sx, sy = xx - pan[0], yy - pan[1]
    smear = (((sx < 0) | (sx >= w)) & (yy < h // 2)) | (((sy < 0) | (sy >= h)) & (xx < w // 2))
    band = band_columns(w, pan)
    for c in range(3):
        cur[c][smear] = prev[c][np.clip(sy, 0, h - 1)[smear], np.clip(sx, 0, w - 1)[smear]]
        prev[c][:, band] = cur[c][:, band]
    cur, prev = decimate(cur, subsamp), decimate(prev, subsamp)
    return cur, prev, degrade(prev, seed)


def block_origins(params):
    nbh, nbv = params.nblocks_h, params.nblocks_v
    bx = np.tile(np.arange(nbh) * params.blk_w, nbv)
    by = np.repeat(np.arange(nbv) * params.blk_h, nbh)
    return bx, by


def block_dims(params, w, h):
    bx, by = block_origins(params)
    return np.minimum(params.blk_w, w - bx), np.minimum(params.blk_h, h - by)


LIMIT_REACH = 112  # a block's "limit" component is the extreme towards the nearer border where that is at most this many pixels long


def prev_field(kind, params, w, h, pan, seed):
    """the previous frame's level-0 field.  "long": what a stream that has panned all along hands on.  "limit": the extremes a
    real previous field can hold -- a block's own prediction stays inside the padded picture (32 px), so its x lies in
    -4 (bx + 32) .. 4 (w + 32 - bx - bw) - 1 and y likewise.  On each axis for itself, a block takes the extreme towards the nearer
    border (less 0 - 7 quarter-pels) where that is at most LIMIT_REACH pixels long, and the "long" component elsewhere.  As the
    candidate of a NEIGHBOUR nearer to the border such a vector is invalid: this is how invalid candidates arise in real streams.
    "limit-full": either extreme for every block, whatever its place -- vectors up to 400 pixels apart side by side, with which
    the reference's find_inliers overflows (inlier_sum_overflows): no parity case, kept to show why "limit" stops at a reach."""
    if kind is None:
        return None
    nb = params.nblocks_h * params.nblocks_v
    rng = np.random.RandomState(seed + 7)
    m = np.zeros(nb, dtype=A.MV_DTYPE)
    long_x = -4 * pan[0] + rng.randint(-8, 9, size=nb)
    long_y = -4 * pan[1] + rng.randint(-8, 9, size=nb)
    if kind == "long":
        m["x"], m["y"] = long_x, long_y
        return m
    assert kind in ("limit", "limit-full")
    bx, by = block_origins(params)
    bw, bh = block_dims(params, w, h)
    lo_x, hi_x = -4 * (bx + A.BORDER), 4 * (w + A.BORDER - bx - bw) - 1
    lo_y, hi_y = -4 * (by + A.BORDER), 4 * (h + A.BORDER - by - bh) - 1
    jx, jy = rng.randint(0, 8, size=nb), rng.randint(0, 8, size=nb)
    if kind == "limit-full":
        m["x"] = np.where(rng.randint(0, 2, size=nb) == 1, hi_x - jx, lo_x + jx)
        m["y"] = np.where(rng.randint(0, 2, size=nb) == 1, hi_y - jy, lo_y + jy)
    else:
        m["x"] = np.where(np.minimum(-lo_x, hi_x) > 4 * LIMIT_REACH, np.clip(long_x, lo_x, hi_x), np.where(-lo_x <= hi_x, lo_x + jx, hi_x - jx))
        m["y"] = np.where(np.minimum(-lo_y, hi_y) > 4 * LIMIT_REACH, np.clip(long_y, lo_y, hi_y), np.where(-lo_y <= hi_y, lo_y + jy, hi_y - jy))
    assert np.all((m["x"] >= lo_x) & (m["x"] <= hi_x) & (m["y"] >= lo_y) & (m["y"] <= hi_y))
    return m


def geometry(name):
    return (GEOMETRIES.get(name) or FULL_SIZES[name])


SEED0 = 401  # (the final vectors at the picture's edge hang on ties: tests/test_long_motion_ref.py asserts that every case has an off-picture block)


def case_seed(c):
    if c.geom in GEOMETRIES:
        return SEED0 + list(GEOMETRIES).index(c.geom) * len(PANS) + PANS.index(c.pan)
    return SEED0 + 90 + list(FULL_SIZES).index(c.geom)


def scene(ref_lib, c):
    w, h, subsamp, blk = geometry(c.geom)
    seed = case_seed(c)
    sc = Scene(ref_lib, w, h, subsamp, seed, with_prev_mvs=False, planes=pan_planes(w, h, subsamp, c.pan, seed), blk=blk)
    sc.prev_mvs = prev_field(c.prev, sc.params, w, h, c.pan, seed)
    return sc


@functools.lru_cache(maxsize=None)
def reference_result(c):
    """(fields of every level, (intra share, scene-change blocks, average error)) of the reference's dsv_hme on a case; shared by
    the tests of a module and never written to"""
    ref = A.load_ref()
    fields, ipct, scb, aerr = scene(ref, c).run_reference(ref, c.quant, c.effort, c.skip)
    for f in fields:
        f.setflags(write=False)
    return tuple(fields), (ipct, scb, aerr)


# ---- what a level-0 field holds -----------------------------------------------------------------------------------------------
Stats = collections.namedtuple("Stats", "nblocks ge16 ge32 off_picture intra skip band_skips max_qpel")


def field_stats(field, params, w, h, pan):
    """of a level-0 field: the share of inter blocks with a component of 16 px (32 px) or more; the number of inter blocks whose
    prediction lies more than 16 px outside the picture; the intra and the skip share of all blocks; the skipped blocks that lie
    wholly in the static band; the largest component in quarter-pels"""
    bx, by = block_origins(params)
    bw, bh = block_dims(params, w, h)
    x, y, flags = field["x"].astype(np.int32), field["y"].astype(np.int32), field["flags"]
    intra, skip = (flags & FLAG_INTRA) != 0, (flags & FLAG_SKIP) != 0
    inter = ~intra
    comp = np.maximum(np.abs(x), np.abs(y))
    n_inter = max(1, int(inter.sum()))
    px, py = bx + (x >> 2), by + (y >> 2)
    band = band_columns(w, pan)
    off = inter & ((px < -16) | (py < -16) | (px + bw > w + 16) | (py + bh > h + 16))
    return Stats(len(field), float((inter & (comp >= 64)).sum()) / n_inter, float((inter & (comp >= 128)).sum()) / n_inter, int(off.sum()),
                 float(intra.sum()) / len(field), float(skip.sum()) / len(field), int((skip & (bx >= band.start) & (bx + bw <= band.stop)).sum()),
                 int(comp[inter].max()) if inter.any() else 0)


# ---- whole streams ------------------------------------------------------------------------------------------------------------
STREAM_W, STREAM_H, STREAM_FRAMES = 352, 288, 8
VELOCITIES = [(24, 0), (0, -20), (57, -45), (-33, -33)]
# The reference's picture types, the same under the three settings (tests/test_long_motion_ref.py).  Every I but the first is a P
# picture that the search's own sums flipped: (57, -45) is flipped every frame, (-33, -33) until the previous field carries the pan.
# Which fast pan ends up which way hangs on the texture; the seeds below are picked for this outcome.
PICTURE_TYPES = {(24, 0): "IPPPPPPP", (0, -20): "IPPPPPPP", (57, -45): "IIIIIIII", (-33, -33): "IIIPPPPP"}
STREAM_SEEDS = {(24, 0): 40, (0, -20): 41, (57, -45): 40, (-33, -33): 69}
SETTINGS = collections.OrderedDict([("qp60-e10", dict(qp=60, effort=10)), ("qp40-e5", dict(qp=40, effort=5)),
                                    ("lossless-e7", dict(qp=100, effort=7))])

Stream = collections.namedtuple("Stream", "w h fmt vel setting scd lie")  # (w, h, fmt, lie: what tests/mixed_steps.py's Runner reads)


def stream_id(s):
    return "vel%+d%+d-%s%s" % (s.vel[0], s.vel[1], s.setting, "" if s.scd else "-noscd")


# every velocity under every setting; the two fast ones once more without scene-change detection, so that they stay P
STREAMS = [Stream(STREAM_W, STREAM_H, "420", v, name, 1, ()) for name in SETTINGS for v in VELOCITIES] + \
          [Stream(STREAM_W, STREAM_H, "420", v, name, 0, ()) for name in SETTINGS for v in VELOCITIES[2:]]


def stream_cfg(s):
    cfg = dict(SETTINGS[s.setting], gop=48)
    if not s.scd:
        cfg["do_scd"] = 0
    return cfg


@functools.lru_cache(maxsize=None)
def stream_frames(vel, w=STREAM_W, h=STREAM_H, n=STREAM_FRAMES):
    """n pictures (packed planar 4:2:0 bytes) that pan at `vel` pixels a frame: picture t is the window at t * vel"""
    pad = (n - 1) * max(abs(vel[0]), abs(vel[1]))
    seed = STREAM_SEEDS[vel]
    out = []
    for t in range(n):  # picture t-1 is picture t's window moved by the pan: the search finds -vel, as in the stage scenes
        planes = decimate(window(w, h, (-t * vel[0], -t * vel[1]), pad, seed, fine=True), A.SUBSAMP_420)
        out.append(b"".join(p.tobytes() for p in planes))
    return tuple(out)


def built(s):
    """the stream as tests/mixed_steps.py's Runner takes it"""
    return dict(frames=list(stream_frames(s.vel)), meta_kw=dict(w=s.w, h=s.h, subsamp=A.SUBSAMP_420), cfg=stream_cfg(s), spec=s, rgb=None)


@functools.lru_cache(maxsize=None)
def reference_stream(s):
    """(packets, final stats) of the reference encoder on the stream alone"""
    pk, stats = encode_stream(A.load_ref(), list(stream_frames(s.vel)), s.w, s.h, A.SUBSAMP_420, eos=False, **stream_cfg(s))
    return tuple(pk), stats


def decode_packets(lib, packets):
    """[(return code, frame number, Y, U, V or None)] per packet: every packet's outcome, not only the pictures"""
    dec = A.DECODER()
    out = []
    for pk in packets:
        buf = A.BUF()
        lib.dsv_mk_buf(C.byref(buf), len(pk) + 64)
        C.memmove(buf.data, pk, len(pk))
        fp, fn = C.POINTER(A.FRAME)(), C.c_uint32(0)
        code = lib.dsv_dec(C.byref(dec), C.byref(buf), C.byref(fp), C.byref(fn))
        planes = None
        if code == A.DEC_OK and fp:
            planes = []
            for c in range(3):
                p = fp.contents.planes[c]
                planes.append(np.ctypeslib.as_array(p.data, shape=(p.h * p.stride,)).reshape(-1, p.stride)[:p.h, :p.w].copy())
            lib.dsv_frame_ref_dec(fp)
        out.append((code, fn.value if planes is not None else None, planes))
    lib.dsv_dec_free(C.byref(dec))
    return out


@functools.lru_cache(maxsize=None)
def reference_decode(s):
    return decode_packets(A.load_ref(), reference_stream(s)[0])


def assert_decodes_equal(want, got, what=""):
    assert len(want) == len(got)
    for i, ((cw, fw, pw), (cg, fg, pg)) in enumerate(zip(want, got)):
        assert (cw, fw) == (cg, fg), "%s packet %d: return code / frame number %r, the reference has %r" % (what, i, (cg, fg), (cw, fw))
        assert (pw is None) == (pg is None), "%s packet %d" % (what, i)
        for c in range(3 if pw is not None else 0):
            assert np.array_equal(pw[c], pg[c]), "%s packet %d: plane %d differs" % (what, i, c)


# ---- where the reference is defined ---------------------------------------------------------------------------------------------
_PARENT_POINTS = ((0, 0), (-2, 0), (2, 0), (0, -2), (0, 2), (-2, -2), (2, 2), (2, -2), (-2, 2))  # hme.c:1484


def inlier_sum_overflows(fields, nxb, nyb):
    """the blocks, over all levels, at which find_inliers (hme.c:1260) sums squares past INT_MAX.  It squares the distance of each
    of up to nine parent vectors from their mean, takes the deviation of that from its average and squares again, in `int`: with
    parents some 200 pixels apart the sum overflows, which is undefined in C -- measured: the reference built at -O3 (gcc
    reasons from "a sum of squares is not negative") and the same source built with -fwrapv, at -O1 or with -fno-inline return
    different fields from there on.  A parity case has to stay clear of it; this recomputes the sums from the reference's own
    fields, exactly."""
    count = 0
    for level in range(len(fields) - 2, -1, -1):
        step = 1 << level
        px, py = (fields[level + 1][k].astype(np.int64).reshape(nyb, nxb) for k in ("x", "y"))
        jj, ii = np.mgrid[0:nyb:step, 0:nxb:step]
        pi, pj = ii & ~(2 * step - 1), jj & ~(2 * step - 1)
        vx, vy, ok = [], [], []
        for ox, oy in _PARENT_POINTS:
            x, y = pi + ox * step, pj + oy * step
            inside = (x >= 0) & (x < nxb) & (y >= 0) & (y < nyb)
            xc, yc = np.clip(x, 0, nxb - 1), np.clip(y, 0, nyb - 1)
            vx.append(np.where(inside, px[yc, xc], 0))
            vy.append(np.where(inside, py[yc, xc], 0))
            ok.append(inside)
        vx, vy, ok = np.array(vx), np.array(vy), np.array(ok)
        n = ok.sum(0)  # (the block's own parent is always inside)
        trunc = lambda a, b: np.sign(a) * (np.abs(a) // b)
        ax, ay = trunc(vx.sum(0), n), trunc(vy.sum(0), n)
        dist = np.where(ok, (vx - ax) ** 2 + (vy - ay) ** 2, 0)
        avgd = dist.sum(0) // n
        ssd = np.where(ok, (dist - avgd) ** 2, 0).sum(0)
        count += int((ssd > 0x7fffffff).sum()) + int((dist.max(0) > 0x7fffffff).sum())
    return count


# ---- a motion sub-stream that outgrows the side-information coder's image -------------------------------------------------------
# csrc/sideinfo.hip codes the x and y vector differences of a P picture into LDS images of SIDE_MV_CAP bytes each and hands a
# picture that needs more to the host.  2560 x 1440 with 16 x 16 blocks forced (14 400 blocks), every tile of a picture the
# previous picture's moved by its own random offset of up to SIDE_JITTER pixels: about 1.2 bytes a block and axis.
SIDE_MV_CAP = 16384
SIDE_W, SIDE_H, SIDE_FRAMES, SIDE_JITTER, SIDE_SEED = 2560, 1440, 3, 28, 77
SIDE_CFG = dict(qp=60, effort=10, gop=48, do_scd=0, block_size_override_x=0, block_size_override_y=0)


@functools.lru_cache(maxsize=None)
def jitter_frames():
    w, h, tile = SIDE_W, SIDE_H, 16
    y = canvas(h, w, SIDE_SEED)
    cur = [y, y[::-1], y[:, ::-1]]  # (chroma: the same texture mirrored -- one canvas of this size is enough work)
    rng = np.random.RandomState(SIDE_SEED)
    yy, xx = (a.astype(np.int32) for a in np.mgrid[0:h, 0:w])
    out = []
    for t in range(SIDE_FRAMES):
        if t:
            ox, oy = (np.repeat(np.repeat(rng.randint(-SIDE_JITTER, SIDE_JITTER + 1, size=(h // tile, w // tile)).astype(np.int32), tile, 0), tile, 1)
                      for _ in range(2))
            at = np.clip(yy + oy, 0, h - 1) * w + np.clip(xx + ox, 0, w - 1)
            cur = [np.take(np.ascontiguousarray(p).ravel(), at) for p in cur]
        out.append(b"".join(p.tobytes() for p in decimate(cur, A.SUBSAMP_420)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_jitter_stream():
    pk, stats = encode_stream(A.load_ref(), list(jitter_frames()), SIDE_W, SIDE_H, A.SUBSAMP_420, eos=False, **SIDE_CFG)
    return tuple(pk), stats


class _Bits:
    """the reference's bit reader (bs.c): most significant bit first"""

    def __init__(self, data, byte):
        self.d, self.pos = data, 8 * byte

    def bit(self):
        b = (self.d[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def align(self):
        self.pos = (self.pos + 7) & ~7

    def ueg(self):  # interleaved exp-Golomb (bs.c: dsv_bs_get_ueg)
        v = 1
        while not self.bit():
            v = (v << 1) | self.bit()
        return v - 1

    def section(self):  # a byte count, then that many bytes, both aligned
        self.align()
        n = self.ueg()
        self.align()
        self.pos += 8 * n
        return n


def side_substream_lengths(packet):
    """(blk_w, blk_h, (stable, mode, EPRM inversion bits), [bytes of the stability, mode, x, y, sub-block-mask and EPRM
    sub-streams]) of a P picture packet, read as the reference's decoder reads it (dsv_decoder.c: the picture header, the
    stability section, decode_motion)"""
    assert packet[5] & 4 and packet[5] & 1, "no P picture"
    bs = _Bits(packet, 14)  # DSV_PACKET_HDR_SIZE
    bs.bits(32)             # frame number
    bs.align()
    bw, bh = 16 << bs.ueg(), 16 << bs.ueg()
    bs.align()
    inv = (bs.bit(), bs.bit(), bs.bit())  # the three statistics bits
    bs.bits(1 + 12)         # the filter flag, the quantiser
    if bs.bit():
        bs.bits(15)
    bs.align()
    return bw, bh, inv, [bs.section() for _ in range(6)]


def motion_substream_lengths(packet):
    """(blk_w, blk_h, [bytes of the mode, x, y, sub-block-mask and EPRM sub-streams]) of a P picture packet"""
    bw, bh, _, lengths = side_substream_lengths(packet)
    return bw, bh, lengths[1:]
