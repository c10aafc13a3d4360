"""Crafted motion fields: what the side-information coder (csrc/sideinfo.hip: k_side_info) and the controller's sums
(csrc/hme.hip: k_block_stats_b) are given when a test, not the search, chooses the field.  The cases and helpers shared by
tests/test_field_cases_ref.py (CPU: every label below is checked against the reference alone) and tests/test_gpu_field_cases.py
(the library against the reference).

Both encoders get the same field in place of their search's: the reference through oracle/_ref/libdsv2ref_field.so
(oracle/field_hook/field_hook.c: its dsv_hme hands out a queued field), the library through dsv2hip_seam_set_field.  With the
field go the four integers the search would have returned its three results from: nintra, ndiff, eligible, total_err
(intra_pct = nintra * 100 / nb, scblocks = ndiff * 100 / max(eligible, 1), avg_err = total_err / nb).

THE DOMAIN OF A LEGAL RECORD is what the reference's dsv_hme can store at level 0 (hme.c:1640-1821):
  skipped   x = y = 0, err = 0, submask = 0, dc = 0; flags: SKIP, and any of MAINTAIN, EPRM (hme.c:1670, :1723-1727, :1812-1816)
  inter     any vector; submask = 0, dc = 0; flags: any of EPRM, MAINTAIN, NOXMITY, NOXMITC, SIMCMPLX, but never SIMCMPLX with EPRM
            (hme.c:1818); err = the block's mean absolute difference, 0 under NOXMITY (hme.c:1790)
  intra     a FULL-PEL vector (hme.c:1809); submask 1 .. 15; dc = 0, or an average | DSV_SRC_DC_PRED (hme.c:977-982); flags: INTRA and
            any of EPRM, MAINTAIN, NOXMITY, NOXMITC; never SIMCMPLX, never SKIP (the skip test leaves before the intra tests)
  RINGING is a flag of intra pictures' analysis only.  Vectors stay within +-800 quarter-pels (tests/test_gpu_long_motion.py).
Two families step outside it on purpose, because the coders have arithmetic of their own for them -- intra blocks with sub-pel
vectors (DSV_SAR on the vector, DSV_SAR_R on the predictor) and skipped blocks with a non-zero raw vector (k_block_stats_b
reads the RAW neighbour, k_side_info the FINAL one): OUTSIDE lists them, and tests/test_field_cases_ref.py shows the reference
deterministic on each over two fresh processes.  SKIP and INTRA both set is in no case.

The labels of a field -- the bit length of each of the six sub-streams, the header's three inversion bits, k_side_info's verdict
-- are computed here.  labels() restates what decides a length: finalisation, the median predictor (with DSV_SAR on an intra
vector and DSV_SAR_R on its predictor), the three votes and the zero runs of each plane; the codes themselves enter by their
lengths only (ueg: 2 * floor(log2(v + 1)) + 1 bits, seg: one more for a non-zero value, an intra record 2 / 6 / 10 / 14 bits).  It
writes no bit and is no second coder; tests/test_field_cases_ref.py checks every label against the reference's packets."""
import collections
import ctypes as C
import functools

import numpy as np

import dsvabi as A
from codec_run import configure_encoder

INTRA, EPRM, MAINTAIN, SKIP, RINGING, NOXMITY, NOXMITC, SIMCMPLX = (1 << b for b in range(8))  # dsv.h:184-191
ALL_INTRA, DC_PRED = 15, 0x100
STAT_KEYS = [n for n, _ in A.STATS._fields_ if n != "mbsubs"]

# k_side_info's published rule (csrc/sideinfo.hip): image sizes in bytes, the slack of each test, the block-count gate
CAP_RLE, CAP_MV, CAP_SBIM = 2048, 16384, 8192
GATE_BLOCKS = 8 * (CAP_RLE - 8)
THREADS = 256
SUBS = ("stable", "mode", "mvx", "mvy", "sbim", "eprm")  # in packet order

# name -> (w, h, block_size_override_x, _y): the smallest pictures that reach each seam of the two-pass coder
GEOMS = collections.OrderedDict([
    ("16x16", (16, 16, 0, 0)),           # one block
    ("48x16", (48, 16, 0, 0)),           # one row: no top neighbour anywhere
    ("16x48", (16, 48, 0, 0)),           # one column: no left neighbour anywhere
    ("176x144", (176, 144, 0, 0)),       # 99 blocks, 157 empty threads
    ("256x256", (256, 256, 0, 0)),       # 256 blocks, one a thread
    ("272x256", (272, 256, 0, 0)),       # 272 blocks, two a thread, 120 empty threads
    ("272x272", (272, 272, 0, 0)),       # 289 blocks: the last busy thread's run is one block short
    ("352x288", (352, 288, 0, 0)),       # 396 blocks
    ("352x288-b32x16", (352, 288, 1, 0)),
    ("178x146", (178, 146, 0, 0)),       # clipped last row and column
    ("1920x1080", (1920, 1080, 0, 0)),   # 8 160 blocks: the smallest here at which the MV and SBIM caps can be crossed
    ("2560x1440", (2560, 1440, 0, 0)),   # 14 400 blocks: the RLE cap
    ("2320x1808", (2320, 1808, 0, 0)),   # 16 385 blocks: just above the nblk > 16 320 gate
])


def grid(geom):
    """(w, h, blk_w, blk_h, nbh, nbv)"""
    w, h, ox, oy = GEOMS[geom]
    bw, bh = 16 << ox, 16 << oy
    return w, h, bw, bh, (w + bw - 1) // bw, (h + bh - 1) // bh


def nblocks(geom):
    g = grid(geom)
    return g[4] * g[5]


def run_of_thread(nblk):
    """blocks per thread of k_side_info's walk"""
    return (nblk + THREADS - 1) // THREADS


# ---- content ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def pictures(w, h, n):
    """n packed planar 4:2:0 pictures, smooth and of low contrast, so that a wrong vector costs little and packets stay small"""
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:ch, 0:cw]
    out = []
    for t in range(n):
        y = 120 + 14 * np.sin((xx + 5 * t) / 61.0) + 10 * np.cos((yy - 3 * t) / 43.0)
        u = 128 + 6 * np.sin((cx + cy + 2 * t) / 37.0)
        v = 128 + 6 * np.cos((cx - cy - 3 * t) / 29.0)
        out.append(b"".join(np.clip(np.rint(p), 0, 255).astype(np.uint8).tobytes() for p in (y, u, v)))
    return tuple(out)


@functools.lru_cache(maxsize=4)
def textured_pictures(w, h, n):
    """n pictures of fine texture (noise, lightly low-passed, moving by (2, 1) pixels a picture): every block has a residual that
    survives the quantiser, so the flag byte k_side_info forms for it shows in the packet"""
    rng = np.random.RandomState(7)
    pad = 2 * n
    planes = []
    for c, (pw, ph) in enumerate(((w, h), ((w + 1) >> 1, (h + 1) >> 1), ((w + 1) >> 1, (h + 1) >> 1))):
        a = rng.randint(0, 256, size=(ph + pad + 2, pw + pad + 2)).astype(np.int32)
        a = (a[:-1, :-1] + a[1:, :-1] + a[:-1, 1:] + a[1:, 1:]) // 4
        planes.append(np.clip(128 + (a - 128) * (3 if c == 0 else 1) // 4, 0, 255).astype(np.uint8))
    out = []
    for t in range(n):
        out.append(b"".join(np.ascontiguousarray(planes[c][(t >> (c > 0)):(t >> (c > 0)) + ph, (2 * t >> (c > 0)):(2 * t >> (c > 0)) + pw]).tobytes()
                            for c, (pw, ph) in enumerate(((w, h), ((w + 1) >> 1, (h + 1) >> 1), ((w + 1) >> 1, (h + 1) >> 1)))))
    return tuple(out)


def pictures_of(case, n):
    w, h = GEOMS[case.geom][:2]
    return textured_pictures(w, h, n) if case.family.endswith("-textured") else pictures(w, h, n)


# ---- fields ----------------------------------------------------------------------------------------------------------------
def blank(nb):
    """nb inter blocks with the zero vector"""
    return np.zeros(nb, dtype=A.MV_DTYPE)


def set_intra(f, at, submask=ALL_INTRA, dc=0):
    f["flags"][at] |= INTRA
    f["submask"][at] = submask
    f["dc"][at] = dc


def set_skip(f, at):
    f["flags"][at] |= SKIP
    f["x"][at] = f["y"][at] = 0
    f["err"][at] = 0


def legal(f):
    """the field lies in the domain written down at the top of this module"""
    fl = f["flags"].astype(np.int64)
    skip, intra = (fl & SKIP) != 0, (fl & INTRA) != 0
    inter = ~skip & ~intra
    ok = (fl & ~0xff) == 0
    ok &= (fl & RINGING) == 0
    ok &= ~(skip & intra)
    ok &= ~skip | ((f["x"] == 0) & (f["y"] == 0) & (f["err"] == 0) & (f["submask"] == 0) & (f["dc"] == 0) & ((fl & ~(SKIP | MAINTAIN | EPRM)) == 0))
    ok &= ~inter | ((f["submask"] == 0) & (f["dc"] == 0) & ~(((fl & SIMCMPLX) != 0) & ((fl & EPRM) != 0)))
    ok &= ~(inter & ((fl & NOXMITY) != 0)) | (f["err"] == 0)
    ok &= ~intra | ((f["x"] % 4 == 0) & (f["y"] % 4 == 0) & (f["submask"] >= 1) & (f["submask"] <= 15) & ((fl & SIMCMPLX) == 0) &
                    ((f["dc"] == 0) | ((f["dc"] & 0xff00) == DC_PRED)))
    ok &= (np.abs(f["x"].astype(np.int32)) <= 800) & (np.abs(f["y"].astype(np.int32)) <= 800)
    return bool(ok.all())


def random_field(geom, seed, p_skip=0.3, p_intra=0.25, reach=60, p_flag=0.3):
    """a legal field with every kind of record side by side"""
    nb = nblocks(geom)
    rng = np.random.RandomState(seed)
    f = blank(nb)
    kind = rng.choice(3, size=nb, p=[1 - p_skip - p_intra, p_skip, p_intra])  # inter, skipped, intra
    f["x"], f["y"] = rng.randint(-reach, reach + 1, size=nb), rng.randint(-reach, reach + 1, size=nb)
    f["err"] = rng.randint(0, 64, size=nb)
    flag = lambda: rng.rand(nb) < p_flag
    fl = np.where(flag(), EPRM, 0) | np.where(flag(), MAINTAIN, 0)
    body = np.where(flag(), NOXMITY, 0) | np.where(flag(), NOXMITC, 0)
    sim = np.where(flag() & ((fl & EPRM) == 0), SIMCMPLX, 0)
    intra, skip = kind == 2, kind == 1
    f["flags"] = np.where(skip, fl | SKIP, np.where(intra, fl | body | INTRA, fl | body | sim))
    f["submask"] = np.where(intra, rng.randint(1, 16, size=nb), 0)
    f["dc"] = np.where(intra & (rng.rand(nb) < 0.5), DC_PRED | rng.randint(0, 256, size=nb), 0)
    f["x"] = np.where(skip, 0, np.where(intra, f["x"] & ~3, f["x"]))
    f["y"] = np.where(skip, 0, np.where(intra, f["y"] & ~3, f["y"]))
    f["err"] = np.where(skip | ((f["flags"] & NOXMITY) != 0), 0, f["err"])
    return f


# ---- labels: code lengths ------------------------------------------------------------------------------------------------------
def ueg_len(v):
    """bits of the interleaved exp-Golomb code of v >= 0 (scalar or array)"""
    return 2 * (np.frexp(np.asarray(v, dtype=np.int64) + 1)[1] - 1) + 1


def seg_len(v):
    v = np.asarray(v, dtype=np.int64)
    return ueg_len(np.abs(v)) + (v != 0)


def rle_len(ones):
    """(bits in front of the closing code, bits of the closing code) of a zero-run-length plane whose emitted bits are `ones`"""
    at = np.flatnonzero(ones)
    if len(at) == 0:
        return 0, int(ueg_len(len(ones)))
    runs = np.diff(np.concatenate(([-1], at))) - 1
    return int(ueg_len(runs).sum()), int(ueg_len(len(ones) - 1 - at[-1]))


def pred1(l, t, tl):  # dsv.c:324
    dif = l + t - tl
    return np.where(np.abs(dif - l) < np.abs(dif - t), l, t)


def finalised(f):
    """the vectors a field finally transmits: zero for a skipped block, full-pel (rounded down) for an intra one"""
    fl = f["flags"]
    x, y = f["x"].astype(np.int64), f["y"].astype(np.int64)
    skip, intra = (fl & SKIP) != 0, (fl & INTRA) != 0
    return np.where(skip, 0, np.where(intra, (x >> 2) * 4, x)), np.where(skip, 0, np.where(intra, (y >> 2) * 4, y))


Labels = collections.namedtuple("Labels", "bits inv verdict rle_pre")  # bits: of the six sub-streams; inv: (stable, mode, eprm)


def labels(f, geom):
    nbh, nbv = grid(geom)[4:]
    fl = f["flags"].astype(np.int64)
    skip, intra, eprm = (fl & SKIP) != 0, (fl & INTRA) != 0, (fl & EPRM) != 0
    stable = skip & ~intra
    coded = ~skip
    vote = lambda v, among: int(np.where(v[among], 1, -1).sum()) > 0  # gather_stats; a tie leaves the plane as it is
    inv = (vote(stable, np.ones(len(f), bool)), vote(intra, coded), vote(eprm, coded))
    planes = [rle_len(stable != inv[0]), rle_len(intra[coded] != inv[1]), rle_len(eprm[coded] != inv[2])]
    fx, fy = (a.reshape(nbv, nbh) for a in finalised(f))
    mvbits = []
    for fin, raw in ((fx, f["x"]), (fy, f["y"])):
        p = np.zeros((nbv + 1, nbh + 1), dtype=np.int64)
        p[1:, 1:] = fin
        pr = pred1(p[1:, :-1], p[:-1, 1:], p[:-1, :-1]).ravel()
        cv = np.where(intra, raw.astype(np.int64) >> 2, fin.ravel())
        pr = np.where(intra, (pr + 2) >> 2, pr)
        mvbits.append(int(seg_len(cv - pr)[coded].sum()))
    sb = np.where(f["submask"] == ALL_INTRA, 1, 5) + np.where((f["dc"] & DC_PRED) != 0, 9, 1)
    sbim = int(sb[intra & coded].sum())
    bits = (sum(planes[0]), sum(planes[1]), mvbits[0], mvbits[1], sbim, sum(planes[2]))
    pre = tuple(p[0] for p in planes)
    bad = len(f) > GATE_BLOCKS or any((b + 32) // 8 + 8 > CAP_RLE for b in pre) or any((b + 40) // 8 + 8 > CAP_MV for b in mvbits) or \
        (sbim + 40) // 8 + 8 > CAP_SBIM
    return Labels(bits, tuple(int(b) for b in inv), int(bad), pre)


# ---- cases -----------------------------------------------------------------------------------------------------------------
BASE_CFG = dict(qp=60, effort=10, gop=48, do_scd=0, intra_pct_thresh=1000)

# name, family, geom; fields: one per P picture (the stream is I and then these); ints: per field (nintra, ndiff, eligible,
# total_err) or None for the field's own counts; cfg: configure_encoder's keywords; types: the pictures' types
Case = collections.namedtuple("Case", "name family geom make ints cfg types")


def own_ints(f):
    fl = f["flags"]
    return (int((((fl & INTRA) != 0) & ((fl & SKIP) == 0)).sum()), 0, len(f), int(f["err"].astype(np.int64).sum()))


def fields_of(case):
    return _fields(case.name)


@functools.lru_cache(maxsize=64)
def _fields(name):
    case = BY_NAME[name]
    out = tuple(case.make())
    for f in out:
        assert len(f) == nblocks(case.geom)
        assert legal(f) or case.family in OUTSIDE, case.name
        f.setflags(write=False)
    return out


def ints_of(case):
    return [own_ints(f) if case.ints is None else case.ints[k] for k, f in enumerate(fields_of(case))]


def case_cfg(case):
    _, _, ox, oy = GEOMS[case.geom]
    return dict(BASE_CFG, block_size_override_x=ox, block_size_override_y=oy, **dict(case.cfg))


def mk(name, family, geom, make, ints=None, cfg=(), types=None):
    return Case(name, family, geom, make, ints, tuple(sorted(dict(cfg).items())), types)


OUTSIDE = ("intra-subpel", "skip-raw")  # families outside the domain (see the top of this module)


# -- runs: one plane at a time.  A pattern is the plane's VALUE per block (stable / intra / EPRM); its complement is the same
# pattern with the vote going the other way (the majority is what becomes zeros), so both are cases.
def run_patterns(nblk):
    bpt = run_of_thread(nblk)
    used = (nblk + bpt - 1) // bpt  # busy threads
    z = lambda: np.zeros(nblk, bool)
    pats = collections.OrderedDict()
    pats["none"] = z()
    for name, at in (("first", [0]), ("last", [nblk - 1]), ("before-seam", [3 * bpt - 1]), ("after-seam", [3 * bpt]), ("both-sides", [3 * bpt - 1, 3 * bpt]),
                     ("gap3", [bpt, 5 * bpt]), ("gap-to-end", [2 * bpt - 1, nblk - 1]), ("gap-most", [0, nblk - 1])):
        if max(at) < nblk and len(set(at)) == len(at):
            p = z()
            p[at] = True
            pats[name] = p
    p = z()
    p[(used - 1) * bpt:] = True  # ones only in the last busy thread's run (a partial run where nblk is no multiple of the run)
    pats["last-thread"] = p
    p = z()
    p[::2] = True
    pats["alternating"] = p     # a tie where nblk is even
    p = z()
    p[:nblk // 2] = True
    pats["half"] = p            # a tie where nblk is even: the plane goes out as it is
    p = z()
    p[:(nblk + 1) // 2 + (nblk % 2 == 0)] = True
    pats["half-plus-one"] = p   # one past the tie: inverted
    return pats


def run_field(plane, value):
    f = blank(len(value))
    if plane == "stable":
        set_skip(f, value)
    elif plane == "mode":
        set_intra(f, value)
    else:
        f["flags"][value] |= EPRM
    return f


RUN_GEOMS = ("16x16", "48x16", "16x48", "176x144", "256x256", "272x256", "272x272", "352x288-b32x16")


def run_cases():
    out = []
    for geom in RUN_GEOMS:
        for plane in ("stable", "mode", "eprm"):
            for pname, p in run_patterns(nblocks(geom)).items():
                for sense, v in (("", p), ("-not", ~p)):
                    out.append(mk("runs-%s-%s-%s%s" % (geom, plane, pname, sense), "runs-" + plane, geom,
                                  functools.partial(lambda plane, v: [run_field(plane, v)], plane, v)))
    return out


# -- predictor and finalisation.  A block at an odd column and an odd row has its left, top and top-left neighbours to itself
# (none of them is left, top or top-left of another such block), so every such block is an experiment of its own.
def odd_cells(geom):
    nbh, nbv = grid(geom)[4:]
    return [(i, j) for j in range(1, nbv, 2) for i in range(1, nbh, 2)], nbh


def intra_subpel_field(geom, seed):
    """intra blocks with every sub-pel phase of x and y, of both signs, beside inter neighbours that make pred1 choose the
    left one (top = top-left), the top one (left = top-left), and tie (left = top)"""
    cells, nbh = odd_cells(geom)
    rng = np.random.RandomState(seed)
    f = blank(nblocks(geom))
    for n, (i, j) in enumerate(cells):
        at = j * nbh + i
        px, py, sign = n & 3, (n >> 2) & 3, -1 if (n >> 4) & 1 else 1
        f["x"][at], f["y"][at] = sign * (4 * rng.randint(0, 30) + px), sign * (4 * rng.randint(0, 30) + py)
        set_intra(f, at, submask=1 + n % 15, dc=(DC_PRED | (n * 37 & 255)) if n & 1 else 0)
        a, b = rng.randint(-200, 201, size=2), rng.randint(-200, 201, size=2)
        l, t, tl = [(a, b, b), (b, a, b), (a, a, b)][(n >> 5) % 3]
        for (ci, cj), v in (((i - 1, j), l), ((i, j - 1), t), ((i - 1, j - 1), tl)):
            f["x"][cj * nbh + ci], f["y"][cj * nbh + ci] = v
    return f


def kinds_field(geom, seed, raw_skip):
    """the left, top and top-left neighbour of a block each in turn inter, skipped or intra (absent: the first row and column
    of every field); the block itself inter, then intra.  raw_skip: skipped neighbours keep a non-zero raw vector"""
    cells, nbh = odd_cells(geom)
    rng = np.random.RandomState(seed)
    f = blank(nblocks(geom))
    for n, (i, j) in enumerate(cells):
        at = j * nbh + i
        f["x"][at], f["y"][at] = rng.randint(-40, 41) * 4, rng.randint(-40, 41) * 4
        if (n // 27) & 1:
            set_intra(f, at, submask=1 + n % 15)
        for k, (ci, cj) in enumerate(((i - 1, j), (i, j - 1), (i - 1, j - 1))):
            c, kind = cj * nbh + ci, (n // 3 ** k) % 3
            f["x"][c], f["y"][c] = rng.randint(-40, 41) * 4 + 2, rng.randint(-40, 41) * 4 - 4
            if kind == 1:
                if raw_skip:
                    f["flags"][c] |= SKIP
                else:
                    set_skip(f, c)
            elif kind == 2:
                f["x"][c] &= ~3
                set_intra(f, c, submask=1 + (n + k) % 15)
    return f


# -- neighbour difference: nd = (|lx - x| + |ly - y| + |tx - x| + |ty - y|) / 3 against 8 (k_side_info), |lx - x| + |ly - y| and
# |tx - x| + |ty - y| against 4 (k_block_stats_b), and the exemption of a vector with both components below 2
DEVIATIONS = [(12, 0), (0, 12), (13, 0), (6, 7), (14, 0), (7, 7), (-12, 0), (-6, -8), (2, 0), (0, 2), (1, 1), (2, 1), (3, 2), (0, 4), (0, 5), (-4, 0), (-5, 0)]
TINY = [(1, 1), (-1, 1), (1, 0), (0, 0), (2, 0), (0, 2), (-2, 1), (1, -2), (-1, -1), (0, -2)]


def neighbourdif_field(geom, base, own):
    """every odd cell differs from its neighbours (all `base`) by the next entry of DEVIATIONS: sums of 24, 26 (nd = 8) and 28
    (nd = 9) inside the picture; along the first row only the left neighbour counts, and 27 (nd = 9) is reached too.
    own: the odd cells hold the entries of TINY themselves (the exemption at 1 and 2)"""
    nbh, nbv = grid(geom)[4:]
    f = blank(nblocks(geom))
    f["x"], f["y"] = base
    n = 0
    for j in list(range(1, nbv, 2)) + [0]:
        for i in range(1, nbh, 2):
            d = (TINY if own else DEVIATIONS + [(27, 0), (13, 14), (26, 0), (24, 0), (25, 0)])
            dx, dy = d[n % len(d)]
            f["x"][j * nbh + i], f["y"][j * nbh + i] = (dx, dy) if own else (base[0] + dx, base[1] + dy)
            n += 1
    return f


def intra_records_field(geom):
    """every sub-mask 1 .. 15 (15: ALL_INTRA), with and without a source DC (0, 255 and another), EPRM set and clear; every third
    block stays inter.  (Sub-mask 0 with INTRA set is outside the domain: hme.c:977.)"""
    nb = nblocks(geom)
    f = blank(nb)
    n = 0
    for at in range(nb):
        if at % 3 == 2:
            f["x"][at], f["y"][at] = (at * 7) % 23 - 11, (at * 5) % 19 - 9
            continue
        dc = [0, DC_PRED | 0, DC_PRED | 255, DC_PRED | 77][(n // 15) % 4]
        set_intra(f, at, submask=1 + n % 15, dc=dc)
        f["x"][at], f["y"][at] = 4 * ((n * 3) % 9 - 4), 4 * ((n * 5) % 7 - 3)
        if (n // 60) & 1:
            f["flags"][at] |= EPRM
        n += 1
    return f


def finalisation_cases():
    out = []
    for geom in ("352x288", "178x146", "352x288-b32x16"):
        out.append(mk("intra-subpel-%s" % geom, "intra-subpel", geom, functools.partial(lambda g: [intra_subpel_field(g, 11)], geom)))
        out.append(mk("kinds-%s" % geom, "kinds", geom, functools.partial(lambda g: [kinds_field(g, 12, False)], geom)))
        out.append(mk("skip-raw-%s" % geom, "skip-raw", geom, functools.partial(lambda g: [kinds_field(g, 13, True)], geom)))
        out.append(mk("nd-%s" % geom, "neighbour-dif", geom, functools.partial(lambda g: [neighbourdif_field(g, (40, -24), False)], geom)))
        out.append(mk("nd-tiny-%s" % geom, "neighbour-dif", geom, functools.partial(lambda g: [neighbourdif_field(g, (40, -24), True)], geom)))
        # the same two fields on textured pictures, where the flag byte (STABLE by nd > 8) reaches the quantiser of a residual
        out.append(mk("nd-textured-%s" % geom, "neighbour-dif-textured", geom, functools.partial(lambda g: [neighbourdif_field(g, (40, -24), False)], geom)))
        out.append(mk("nd-tiny-textured-%s" % geom, "neighbour-dif-textured", geom, functools.partial(lambda g: [neighbourdif_field(g, (40, -24), True)], geom)))
        out.append(mk("intra-records-%s" % geom, "intra-records", geom, functools.partial(lambda g: [intra_records_field(g)], geom)))
    for geom in ("16x16", "48x16", "16x48", "176x144", "256x256", "272x256", "272x272", "352x288", "352x288-b32x16", "178x146"):
        out.append(mk("random-%s" % geom, "random", geom, functools.partial(lambda g: [random_field(g, 21)], geom)))
    return out


# -- the sums of k_block_stats_b: each kind of block alone, all at once, under the three rate-control modes (the complexity term
# differs per mode); err against avg_err = total_err / nb takes both signs
def uniform_field(geom, kind):
    nb = nblocks(geom)
    f = blank(nb)
    f["err"] = 20 + np.arange(nb) % 25
    if kind == "skip":
        set_skip(f, np.ones(nb, bool))
    elif kind.startswith("phase"):
        f["x"], f["y"] = 8 + int(kind[5]), -12 + int(kind[6])
    elif kind == "intra-all":
        set_intra(f, np.ones(nb, bool))
    elif kind == "intra-sub-dc":
        set_intra(f, np.ones(nb, bool), submask=1 + np.arange(nb) % 14, dc=DC_PRED | 90)
    elif kind == "eprm":
        f["flags"] |= EPRM
    elif kind == "maintain-noxmity":
        f["flags"] |= MAINTAIN | NOXMITY
        f["err"] = 0
    elif kind == "chaos":
        f["x"], f["y"] = np.where(np.arange(nb) % 2 == 0, 30, -30), 9
    else:
        raise ValueError(kind)
    return f


SUM_KINDS = ("skip", "phase00", "phase20", "phase12", "phase33", "phase01", "intra-all", "intra-sub-dc", "eprm", "maintain-noxmity", "chaos")
RC = collections.OrderedDict([("crf", dict(rc_mode=0)), ("abr", dict(rc_mode=1, bitrate=150000)), ("cqp", dict(rc_mode=2))])


def sum_cases():
    out = []
    geom = "176x144"
    nb = nblocks(geom)
    for rc, cfg in RC.items():
        for kind in SUM_KINDS:
            out.append(mk("sums-%s-%s" % (rc, kind), "sums-" + rc, geom, functools.partial(lambda k: [uniform_field("176x144", k)], kind), cfg=cfg))
        for name, total in (("err-above", 10 * nb), ("err-below", 60 * nb), ("err-zero", 0)):  # avg_err 10 / 60 / 0 against err 0 .. 63
            out.append(mk("sums-%s-all-%s" % (rc, name), "sums-" + rc, geom, functools.partial(lambda: [random_field("176x144", 31)]),
                          ints=[(20, 3, nb, total)], cfg=cfg))
    return out


# -- the running intra map (scene_change_detection's second test): I P P P, a field a picture; MAINTAIN and NOXMITY on blocks
# that are, and are not, in the map.  With the default intra_pct_thresh the accumulated share flips a picture to intra.
def map_fields(geom, seed, share):
    nb = nblocks(geom)
    rng = np.random.RandomState(seed)
    out = []
    for t in range(3):
        f = blank(nb)
        pick = rng.rand(nb) < share
        set_intra(f, pick, submask=np.where(rng.rand(nb) < 0.5, ALL_INTRA, 5)[pick])
        rest = ~pick
        f["flags"][rest & (rng.rand(nb) < 0.5)] |= MAINTAIN
        f["flags"][rest & (rng.rand(nb) < 0.5)] |= NOXMITY
        moving = rest & (rng.rand(nb) < 0.3)
        f["x"][moving] = 4
        set_skip(f, rest & ~moving & (rng.rand(nb) < 0.3))
        f["flags"][(f["flags"] & SKIP) != 0] &= ~np.uint32(NOXMITY)
        out.append(f)
    return out


def map_cases():
    out = []
    for geom in ("176x144", "352x288"):
        for share, types in ((0.1, "IPPP"), (0.3, "IPIP"), (0.45, "IIPI")):  # (what the reference does: tests/test_field_cases_ref.py)
            out.append(mk("map-%s-%d" % (geom, int(share * 100)), "intra-map", geom, functools.partial(map_fields, geom, 41, share),
                          cfg=dict(intra_pct_thresh=90), types=types))
    return out


# -- scene change by field: do_scd = 1 (every other case runs with 0), intra_pct_thresh out of reach, so that scene_change_detection's
# `sc` alone decides -- blks against 120 and against scene_change_pct, from the four integers (scblocks, avg_err) and from the
# avg_motion / chaos / complexity sums of k_block_stats_b.  The pairs were found by search on the reference through the hook
# library (all k in 0 .. 74 under ndiff 70 .. 95 and total_err 40 nb, 60 nb; all ndiff in 0 .. nb under k 0, 10, 20); the CPU module
# asserts the types.
def scene_field(geom, k):
    """a random legal field whose first k plain inter blocks are made wholly intra"""
    f = random_field(geom, 51, p_skip=0.2, p_intra=0.1)
    plain = np.flatnonzero((f["flags"] & (SKIP | INTRA)) == 0)[:k]
    f["x"][plain] &= ~3
    f["y"][plain] &= ~3
    f["flags"][plain] &= ~np.uint32(SIMCMPLX)
    set_intra(f, plain)
    return f


def scene_cases():
    geom = "176x144"
    nb = nblocks(geom)
    out = []
    # (k, ndiff, the second picture's type): one block apart at k 21 | 22 and, where the sums move `shift` back, at 48 | 49;
    # one ndiff apart, the field the same, at 82 | 83
    for k, ndiff, t in ((21, 80, "P"), (22, 80, "I"), (48, 80, "I"), (49, 80, "P"), (20, 82, "P"), (20, 83, "I")):
        out.append(mk("scene-k%d-ndiff%d" % (k, ndiff), "scene", geom, functools.partial(lambda k: [scene_field("176x144", k)], k),
                      ints=[(20, ndiff, nb, 40 * nb)], cfg=dict(do_scd=1), types="I" + t))
    return out


# -- the caps.  A field on each side of k_side_info's rule, as near as the code lengths allow, and one far beyond.
def checker_x(geom, strong, axis="x"):
    """x = +-64 in a chequerboard, +-128 on the first `strong` blocks: every difference against the median predictor is twice
    the amplitude (16 bits; 18 among the strong ones)"""
    nbh, nbv = grid(geom)[4:]
    s = np.where((np.arange(nbh)[None, :] + np.arange(nbv)[:, None]) % 2 == 0, 1, -1).ravel()
    f = blank(nbh * nbv)
    f[axis] = s * np.where(np.arange(nbh * nbv) < strong, 128, 64)
    return f


def plane_alternating(geom, plane):
    """every other block wholly intra (plane "mode") or EPRM: 3 bits a pair in that plane, a tie of its vote"""
    f = blank(nblocks(geom))
    return run_field(plane, np.arange(len(f)) % 2 == 1)


def sbim_field(geom, n14, n2=0):
    """the first n14 blocks intra with a partial mask and a source DC (14 bits), the next n2 wholly intra without one (2)"""
    f = blank(nblocks(geom))
    at = np.arange(len(f))
    set_intra(f, at < n14, submask=5, dc=DC_PRED | 128)
    set_intra(f, (at >= n14) & (at < n14 + n2))
    return f


def stable_alternating(geom, pairs, singles=0):
    """inter and skipped blocks in turn over the first 2 * pairs blocks (3 bits a pair in the stability plane), then `singles`
    more skipped ones (1 bit each), inter behind"""
    f = blank(nblocks(geom))
    at = np.arange(len(f))
    set_skip(f, ((at < 2 * pairs) & (at % 2 == 1)) | ((at >= 2 * pairs) & (at < 2 * pairs + singles)))
    return f


def threshold(make, lo, hi, geom):
    """the smallest n in (lo, hi] for which make(n) is handed to the host by the kernel's rule (make(lo) is not, make(hi) is)"""
    assert not labels(make(lo), geom).verdict and labels(make(hi), geom).verdict
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if labels(make(mid), geom).verdict:
            hi = mid
        else:
            lo = mid
    return hi


@functools.lru_cache(maxsize=None)
def cap_threshold(which):
    if which == "mv":
        return threshold(lambda n: checker_x("1920x1080", n), 0, 8160, "1920x1080")
    if which == "sbim":
        return threshold(lambda n: sbim_field("1920x1080", n), 0, 8160, "1920x1080")
    return threshold(lambda n: stable_alternating("2560x1440", n), 0, 7200, "2560x1440")


CAP_MAKERS = {"mv": ("1920x1080", checker_x), "sbim": ("1920x1080", sbim_field), "rle": ("2560x1440", stable_alternating)}
CAP_FAR = {"mv": 8160, "sbim": 8160, "rle": 7200}
CAP_FINE = {"mv": None, "sbim": 2, "rle": 1}  # bits of the finer code each maker's second argument adds


def cap_margin_of(which, f):
    """how many bits the capped sub-stream of field f lies from the smallest count the kernel hands to the host
    (off + slack >= 8 * (cap - 8 + 1)): >= 0 is over"""
    lab = labels(f, CAP_MAKERS[which][0])
    if which == "rle":
        return lab.rle_pre[0] + 32 - 8 * (CAP_RLE - 7)
    if which == "mv":
        return lab.bits[2] + 40 - 8 * (CAP_MV - 7)
    return lab.bits[4] + 40 - 8 * (CAP_SBIM - 7)


@functools.lru_cache(maxsize=None)
def cap_field_args(which, side):
    """the coarse threshold by bisection; then the finer code, where the maker has one, brings each side as near as it goes"""
    geom, make = CAP_MAKERS[which]
    if side == "far":
        return (CAP_FAR[which],)
    n = cap_threshold(which)
    fine = CAP_FINE[which]
    if fine is None:
        return (n - 1,) if side == "below" else (n,)
    short = -cap_margin_of(which, make(geom, n - 1))  # > 0
    k = (short + fine - 1) // fine                    # the fewest fine codes that cross
    return (n - 1, k - 1) if side == "below" else (n - 1, k)


def cap_field(which, side):
    geom, make = CAP_MAKERS[which]
    return make(geom, *cap_field_args(which, side))


def cap_margin(which, side):
    return cap_margin_of(which, cap_field(which, side))


def cap_cases():
    out = []
    for which, (geom, _) in CAP_MAKERS.items():
        for side in ("below", "above", "far"):
            out.append(mk("cap-%s-%s" % (which, side), "caps", geom, functools.partial(lambda w, s: [cap_field(w, s)], which, side)))
    # the other scan lanes of the same rules, far beyond: y vectors (k == 1), the mode and the EPRM plane (tid 1, 2)
    out.append(mk("cap-mvy-far", "caps", "1920x1080", lambda: [checker_x("1920x1080", 8160, "y")]))
    out.append(mk("cap-rle-mode-far", "caps", "2560x1440", lambda: [plane_alternating("2560x1440", "mode")]))
    out.append(mk("cap-rle-eprm-far", "caps", "2560x1440", lambda: [plane_alternating("2560x1440", "eprm")]))
    out.append(mk("gate-2320x1808", "caps", "2320x1808", lambda: [blank(nblocks("2320x1808"))]))
    return out


SMALL_CASES = run_cases() + finalisation_cases() + sum_cases() + map_cases() + scene_cases()
CAP_CASES = cap_cases()
CASES = SMALL_CASES + CAP_CASES
BY_NAME = collections.OrderedDict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)
FAMILIES = list(collections.OrderedDict.fromkeys((c.family, c.geom) for c in SMALL_CASES))


def family_id(fg):
    return "%s-%s" % fg


def family_cases(fg):
    return [c for c in SMALL_CASES if (c.family, c.geom) == fg]


# ---- encoding a case ------------------------------------------------------------------------------------------------------------
FIELD_SO = A.REF_SO.replace("libdsv2ref.so", "libdsv2ref_field.so")


def load_field_ref():
    lib = A.bind_codec_api(A.load(FIELD_SO))
    lib.dsv2ref_set_field.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint]
    lib.dsv2ref_set_field.restype = C.c_int
    return lib


def ref_setter(lib):
    return lambda enc, f, ints: lib.dsv2ref_set_field(f.ctypes.data, len(f), *ints)


def hip_setter(hip):
    return lambda enc, f, ints: hip.dsv2hip_seam_set_field(C.byref(enc), f.ctypes.data, len(f), *ints)


def encode_case(lib, setter, case):
    """(packets, every counter of the encoder's final stats) of the case through dsv_enc, its fields queued picture by picture"""
    w, h = GEOMS[case.geom][:2]
    fields, ints = fields_of(case), ints_of(case)
    enc = A.ENCODER()
    configure_encoder(lib, enc, A.mk_meta(w, h, A.SUBSAMP_420), **case_cfg(case))
    bufs, packets = (A.BUF * 4)(), []
    for t, fb in enumerate(pictures_of(case, len(fields) + 1)):
        if t:
            f = np.ascontiguousarray(fields[t - 1])
            assert setter(enc, f, ints[t - 1]) == 0
        arr = np.frombuffer(fb, dtype=np.uint8).copy()
        n = lib.dsv_enc(C.byref(enc), lib.dsv_load_planar_frame(A.SUBSAMP_420, arr.ctypes.data, w, h), bufs)
        for i in range(n):
            packets.append(bytes(C.string_at(bufs[i].data, bufs[i].len)))
            lib.dsv_buf_free(C.byref(bufs[i]))
    stats = {k: getattr(enc.stats, k) for k in STAT_KEYS}
    stats["mbsubs"] = tuple(enc.stats.mbsubs)
    lib.dsv_enc_free(C.byref(enc))
    return packets, stats


@functools.lru_cache(maxsize=None)
def reference_case(name):
    """the reference's (packets, stats) of a case; shared by the tests of a module and never written to"""
    lib = load_field_ref()
    pk, stats = encode_case(lib, ref_setter(lib), BY_NAME[name])
    return tuple(pk), stats


def expected_types(case):
    return case.types or "I" + "P" * len(fields_of(case))


def expected_flags(case):
    """how often k_side_info itself hands a picture of the case to the host: its verdict on every field that stays a P picture"""
    return sum(labels(f, case.geom).verdict for f, t in zip(fields_of(case), expected_types(case)[1:]) if t == "P")


def digest(packets, stats):
    """what two runs of a case are compared by across processes"""
    import hashlib
    h = hashlib.sha256()
    for p in packets:
        h.update(len(p).to_bytes(4, "little") + p)
    return h.hexdigest() + " " + repr(sorted(stats.items()))


# ---- lockstep steps ---------------------------------------------------------------------------------------------------------
STEP_SIX = ("random-352x288", "intra-subpel-352x288", "kinds-352x288", "nd-352x288", "intra-records-352x288", "skip-raw-352x288")
STEP_1080 = ("cap-mv-below", "cap-mv-far", "cap-sbim-below")  # the middle one overflows


def encode_step(hip, names):
    """the cases `names` (one geometry, two pictures each) in one dsv2hip_enc_batch_host step a picture, slot k = names[k];
    returns [(packets, stats)] in that order"""
    cases = [BY_NAME[n] for n in names]
    w, h = GEOMS[cases[0].geom][:2]
    assert all(GEOMS[c.geom] == GEOMS[cases[0].geom] and len(fields_of(c)) == 1 for c in cases)
    n, pics = len(cases), pictures(w, h, 2)
    encs = [A.ENCODER() for _ in cases]
    for e, c in zip(encs, cases):
        configure_encoder(hip, e, A.mk_meta(w, h, A.SUBSAMP_420), **case_cfg(c))
    P = len(pics[0])
    pinned = hip.dsv2hip_host_alloc(2 * P)
    assert pinned
    got = [[] for _ in cases]
    try:
        for t in range(2):  # (both up front: the step prefetches what host_next announces)
            C.memmove(pinned + t * P, pics[t], P)
        for t in range(2):
            if t:
                for e, c in zip(encs, cases):
                    assert hip_setter(hip)(e, np.ascontiguousarray(fields_of(c)[0]), ints_of(c)[0]) == 0
            encp = (C.POINTER(A.ENCODER) * n)(*[C.pointer(e) for e in encs])
            bufs, nbufs = (A.BUF * (4 * n))(), (C.c_int * n)()
            cur = (C.c_void_p * n)(*[pinned + t * P] * n)
            nxt = (C.c_void_p * n)(*[pinned + P if t == 0 else None] * n)
            assert hip.dsv2hip_enc_batch_host(n, encp, cur, nxt, bufs, nbufs) == 0
            for k in range(n):
                for i in range(nbufs[k]):
                    b = bufs[4 * k + i]
                    got[k].append(bytes(C.string_at(b.data, b.len)))
                    hip.dsv_buf_free(C.byref(b))
        out = []
        for k, e in enumerate(encs):
            stats = {s: getattr(e.stats, s) for s in STAT_KEYS}
            stats["mbsubs"] = tuple(e.stats.mbsubs)
            out.append((got[k], stats))
    finally:
        for e in encs:
            hip.dsv_enc_free(C.byref(e))
        hip.dsv2hip_host_free(pinned)
    return out
