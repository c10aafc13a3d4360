"""Geometries and contents at the edges of what the library accepts: the smallest pictures (16 x 16, one block), planes with 2 - 5
transform levels, a dimension that collapses to one row or column while the other still has many levels to go, and content that
drives the coefficients to the top of their range.  Shared by tests/test_oracle_edges.py (CPU: oracle against reference, which
also shows that the reference survives every input) and tests/test_gpu_edges.py (the library against the reference)."""
import numpy as np

import dsvabi as A
from test_oracle_sbt import rand_frame

SUBSAMP_411, SUBSAMP_410 = 0x8, 0xA

GEOMETRIES = [
    # (w, h, subsamp)
    (16, 16, A.SUBSAMP_420),       # one block; chroma 8 x 8
    (18, 16, A.SUBSAMP_420),       # two blocks wide, the second 2 pixels; odd chroma width (9 -> coefficient plane of 10)
    (16, 18, A.SUBSAMP_420),
    (32, 32, A.SUBSAMP_420),
    (34, 18, A.SUBSAMP_420),
    (48, 16, A.SUBSAMP_420),       # one block high
    (64, 48, A.SUBSAMP_420),
    (66, 34, A.SUBSAMP_420),
    (130, 258, A.SUBSAMP_420),
    (16384, 16, A.SUBSAMP_420),    # the height collapses to 1 while the width has nine levels to go
    (16, 4096, A.SUBSAMP_420),
    (16, 16, A.SUBSAMP_444),
    (4098, 18, A.SUBSAMP_444),
    (16, 16, SUBSAMP_410),         # chroma 4 x 4
    (16, 16, SUBSAMP_411),         # chroma 4 x 16
    (30, 22, A.SUBSAMP_422),
]
GEOM_IDS = ["%dx%d-%x" % g for g in GEOMETRIES]
GEOMETRIES_420 = [g for g in GEOMETRIES if g[2] == A.SUBSAMP_420]
GEOM_IDS_420 = ["%dx%d-%x" % g for g in GEOMETRIES_420]

CONTENTS = ("black", "white", "checker", "stripes", "noise", "impulses", "smooth")


def plane_bitstream_bytes(cw, ch):
    """Room for one coded plane.  The reference writes up to 19 bytes a coefficient on the smallest planes (a 16 x 16 lossless
    checkerboard: 5951 bytes); the largest plane measured, 16384 x 16 of lossless 0/255 noise, takes 324 959."""
    return cw * ch * 64 + 65536


def inverse_reads_stale_scratch(cw, ch, plane, isP, lossless):
    """True where the reference's inverse transform of a cw x ch coefficient plane is not a function of its input.  At a level
    whose picture is one row high, a lifting filter's update step reads the row under it (sbt.c:200, 222: v[0] -= v[s] >> 1 with
    n = 1).  The forward transform finds there the high-pass output of the level that was two rows high, which is also the
    coefficient below in the plane; the inverse finds what the call before it left in the static scratch image (sbt.c:60) --
    measured: up to 5 grey levels of difference in 16384 x 16 intra chroma, any difference in lossless planes, between two
    calls on the same coefficients.  Only straight after the forward transform of the same plane, unquantised, is it the
    coefficient below, which is what the library reads.  (A collapsed width reads the plane itself in both directions.)"""
    lvls = (max(cw, ch) - 1).bit_length()
    for l in range(1, lvls + 1):
        if lossless or plane:
            lifting = 1 <= l <= lvls - 2 and (lossless or not isP)
        else:
            lifting = l == 4 or (not isP and l in (1, 2))
        if lifting and (ch + (1 << (l - 1)) - 1) >> (l - 1) == 1:
            return True
    return False


def content_plane(kind, pw, ph, seed=0):
    """One pw x ph plane of the named content (every kind but 'smooth', which is a whole-frame generator)"""
    yy, xx = np.mgrid[0:ph, 0:pw]
    if kind == "black":
        a = np.zeros((ph, pw))
    elif kind == "white":
        a = np.full((ph, pw), 255)
    elif kind == "checker":
        a = ((xx + yy + seed) & 1) * 255
    elif kind == "stripes":
        a = ((xx + seed) & 1) * 255 + 0 * yy
    elif kind == "noise":
        a = np.random.RandomState(1000 + seed).randint(0, 2, size=(ph, pw)) * 255
    elif kind == "impulses":
        a = np.zeros((ph, pw))
        a[ph // 2, pw // 2] = a[0, 0] = a[ph - 1, pw - 1] = 255
    else:
        raise ValueError(kind)
    return a.astype(np.uint8)


def content_frame(kind, subsamp, w, h, seed=0):
    """A bordered frame of the named content; the border holds random bytes, as rand_frame's does"""
    if kind == "smooth":
        return rand_frame(subsamp, w, h, seed=w + h + seed)
    f = A.HostFrame(subsamp, w, h, border=True)
    f.buf[:] = np.random.RandomState(seed + 5).randint(0, 256, size=f.buf.shape, dtype=np.uint8)
    for c in range(3):
        pw, ph = f.dims[c]
        f.plane(c)[:, :] = content_plane(kind, pw, ph, seed)
    return f


def content_planes(kind, subsamp, w, h, seed=0):
    f = content_frame(kind, subsamp, w, h, seed)
    return tuple(f.plane(c).copy() for c in range(3))


def degrade(planes, seed):
    """the stand-in for a reconstruction that hme_common.Scene uses"""
    rng = np.random.RandomState(seed)
    return tuple(np.clip((p.astype(np.int32) // 6) * 6 + 3 + rng.randint(-1, 2, size=p.shape), 0, 255).astype(np.uint8) for p in planes)


def striped_planes(subsamp, w, h, period, shift):
    """vertical stripes of the given period in every plane, moved `shift` pixels to the right"""
    f = A.HostFrame(subsamp, w, h, border=True)
    out = []
    for c in range(3):
        pw, ph = f.dims[c]
        yy, xx = np.mgrid[0:ph, 0:pw]
        out.append(((((xx - shift) % period) < period // 2) * 255 + 0 * yy).astype(np.uint8))
    return tuple(out)


def const_planes(subsamp, w, h, value):
    f = A.HostFrame(subsamp, w, h, border=True)
    return tuple(np.full((f.dims[c][1], f.dims[c][0]), value, dtype=np.uint8) for c in range(3))


TIE_SIZES = [(16, 16), (34, 18), (64, 48), (130, 258)]
TIE_SCENES = ("constant", "constant-vs-checker", "stripes2", "stripes4", "stripes8", "noise")


def tie_scene_planes(name, w, h, subsamp=A.SUBSAMP_420):
    """(cur, prev, degraded prev) of the motion-search scenes in which many candidates tie exactly.  The degraded picture is the
    previous one itself where the scene is about ties (a degradation with noise would break them)."""
    if name == "constant":
        p = const_planes(subsamp, w, h, 128)
        return p, p, p
    if name == "constant-vs-checker":
        prev = content_planes("checker", subsamp, w, h)
        return const_planes(subsamp, w, h, 128), prev, prev
    if name.startswith("stripes"):
        period = int(name[7:])
        prev = striped_planes(subsamp, w, h, period, 0)
        return striped_planes(subsamp, w, h, period, 1), prev, prev
    if name == "noise":
        prev = content_planes("noise", subsamp, w, h, seed=1)
        return content_planes("noise", subsamp, w, h, seed=2), prev, degrade(prev, 3)
    raise ValueError(name)


# ---- tiny whole streams ---------------------------------------------------------------------------------------------------
# The reference encoder gives a picture's packet w * h * 2 bytes in 4:2:0 (w * h * 4 in 4:2:2, w * h * 6 in 4:4:4:
# dsv_encoder.c:1053-1072) and does not check it.  Below about 96 x 80 a packet can outgrow that: the reference then corrupts its
# heap (34 x 18 at qp 85 aborts).  A stream is a parity case only where every reference packet stays within 3/4 of the bound;
# packet_bound_holds asserts that condition (tests/test_oracle_edges.py runs it on the CPU for every case below).
# Largest reference packet in bytes, SynthVideo(seed=7), 5 frames (re-measure when either changes):
#
#   size      qp 30   qp 60   qp 85 (gop 0)   qp 100   bound
#   16x16        62      66      104             126      512
#   18x16       113     189      570             535      576
#   32x32       403     917     1903            1906     2048
#   34x18       287     553     abort           abort    1224
#   48x32       490    1111     2187            2236     3072
#   64x48       703    1677     3147            3676     6144
#   66x34       710    1553     2823            2986     4488
#   128x16      443    1053     2223            2185     4096
#   16x128      411     996     2075            2194     4096
STREAM_SEED, STREAM_FRAMES = 7, 5
STREAM_SIZES = [(16, 16), (18, 16), (32, 32), (34, 18), (48, 32), (64, 48), (66, 34), (128, 16), (16, 128)]
STREAM_SIZES_ALL_QP = [(16, 16), (48, 32), (64, 48), (66, 34), (128, 16), (16, 128)]  # qp 85 and qp 100 stay inside 3/4 of the bound
STREAM_CASES = (
    [("%dx%d-qp%d" % (w, h, qp), w, h, A.SUBSAMP_420, "synth", dict(qp=qp, gop=4)) for (w, h) in STREAM_SIZES for qp in (30, 60)]
    + [("%dx%d-qp85-intra" % (w, h), w, h, A.SUBSAMP_420, "synth", dict(qp=85, gop=0)) for (w, h) in STREAM_SIZES_ALL_QP]
    + [("%dx%d-lossless" % (w, h), w, h, A.SUBSAMP_420, "synth", dict(qp=100, gop=4)) for (w, h) in STREAM_SIZES_ALL_QP]
    + [("16x16-444-lossless", 16, 16, A.SUBSAMP_444, "synth", dict(qp=100, gop=4)),
       ("130x258-qp60", 130, 258, A.SUBSAMP_420, "synth", dict(qp=60, gop=4))]
    # the "static" content class at the smallest sizes: identical frames, every block of every P picture skipped
    + [("%dx%d-%s" % (w, h, kind), w, h, A.SUBSAMP_420, kind, dict(qp=60, gop=4)) for (w, h) in ((16, 16), (64, 48)) for kind in ("black", "white")]
)
BATCH_GEOMETRIES = [(16, 16), (34, 18)]
BATCH_STREAMS, BATCH_CFG = 8, dict(qp=60, gop=4)


def stream_frames(w, h, subsamp, content, seed=STREAM_SEED, n=STREAM_FRAMES):
    """the pictures of a stream case as packed planar bytes"""
    if content == "synth":
        from conftest import load_pkg
        v = load_pkg().synth.SynthVideo(w, h, "420" if subsamp == A.SUBSAMP_420 else "444", seed=seed)
        return [v.frame_bytes(t) for t in range(n)]
    return [b"".join(p.tobytes() for p in content_planes(content, subsamp, w, h))] * n


def packet_bound(w, h, subsamp):
    return w * h * {A.SUBSAMP_420: 2, A.SUBSAMP_422: 4, A.SUBSAMP_444: 6}[subsamp]


def packet_bound_holds(packets, w, h, subsamp):
    """the condition of a stream case, not a tolerance: beyond its bound the reference is undefined"""
    worst = max(len(p) for p in packets)
    assert 4 * worst <= 3 * packet_bound(w, h, subsamp), "broken test case: a reference packet of %d bytes against a bound of %d" % (
        worst, packet_bound(w, h, subsamp))


def stream_inverse_is_undefined(w, h, subsamp, cfg):
    """True for a stream some plane of which the reference cannot invert as a function of its input (inverse_reads_stale_scratch):
    128 x 16 here.  Measured: the reference decodes its own lossless 128 x 16 stream to pictures that differ from the source and
    from its own second decode of the same packets.  Its intra packets depend on the forward transform alone and stay comparable;
    its reconstructions, so every P packet after them, and its decoded pictures do not."""
    lossless = int(cfg["qp"] == 100)
    return any(inverse_reads_stale_scratch(cw, ch, plane, isP, lossless)
               for plane, (cw, ch) in enumerate(A.coef_dims(subsamp, w, h)) for isP in (0, 1))
