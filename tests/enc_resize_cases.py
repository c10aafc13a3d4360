"""The cases of tests/test_gpu_enc_resize.py and the reference streams it compares with, apart from the GPU: the oracle's pictures
(tests/ingest_resize.py on the content of the surface tests) and the reference encoder's packets on them, made once, shared and
never changed.  tests/test_ingest_resize_ref.py builds every one of them on a machine without a GPU and checks the two conditions
of a case there."""
import functools

import numpy as np

import dsvabi as A
import ingest_resize as IR
import rgb_csc as R
from codec_run import FMT
from edge_cases import content_planes
from enc_in import LADDER_CFG, LADDER_LOSSLESS, LADDER_NFR, LADDER_SEED, content, ref_packets, rgb_content
from hipabi import PLANAR, SEMI

CFG, LOSSLESS = LADDER_CFG, LADDER_LOSSLESS
CHECKER_CFG = dict(qp=30, gop=4)
NFR, SEED = LADDER_NFR, LADDER_SEED
BGRA709, RGBAFULL = R.BGRA | R.BT709, R.RGBA | R.FULL
LAYOUTS = [PLANAR, SEMI, BGRA709, RGBAFULL]
LAYOUT_IDS = {PLANAR: "planar", SEMI: "semiplanar", BGRA709: "bgra709", RGBAFULL: "rgbafull"}
VARIANTS = ["tight", "plus1", "aligned"]

# (src_w, src_h, W, H): two taps, anamorphic, a ratio just above 1, 3 : 2, nine taps, exact, one axis only, a row of 352 samples (two workgroups)
SOURCES_420 = [(24, 24, 16, 16), (27, 19, 18, 16), (35, 19, 34, 18), (51, 27, 34, 18), (127, 121, 16, 16), (128, 128, 16, 16), (48, 32, 48, 16),
               (440, 360, 352, 288)]
# every chroma format at the encoder sizes of test_gpu_enc_scale.py: 34x18 and 38x22
FORMAT_SOURCES = [("444", 51, 27, 34, 18), ("422", 51, 27, 34, 18), ("420", 43, 20, 34, 18), ("411", 57, 33, 38, 22), ("410", 57, 33, 38, 22),
                  ("410", 297, 169, 38, 22)]
# one step of five 34x18 encoders: (layout, src_w, src_h, "plain" | "half" | "sized")
MIXED = [(PLANAR, 34, 18, "plain"), (SEMI, 67, 35, "half"), (BGRA709, 51, 27, "sized"), (PLANAR, 35, 19, "sized"), (RGBAFULL, 34, 18, "sized")]
CONSTANT_SOURCES = [(24, 24), (127, 121)]  # -> 16x16
CHECKER = (99, 51, 66, 34)


@functools.lru_cache(maxsize=None)
def oracle_pictures(sw, sh, w, h, name, kind):
    """the encoder's pictures (packed planar bytes) for the content made at the SOURCE size with seed 5"""
    _, hs, vs = FMT[name]
    if kind == "yuv":
        return tuple(IR.packed(IR.resize_yuv(IR.split_planar(f, sw, sh, hs, vs), w, h, hs, vs)) for f in content(sw, sh, name, NFR, SEED))
    return tuple(IR.packed(IR.convert_sized(px, kind, w, h, hs, vs)) for px in rgb_content(sw, sh, NFR, SEED))


@functools.lru_cache(maxsize=None)
def reference(sw, sh, w, h, name, kind):
    return ref_packets(oracle_pictures(sw, sh, w, h, name, kind), w, h, name, CFG)


@functools.lru_cache(maxsize=None)
def constant_reference(y, c):
    flat = [np.full((16, 16), y, dtype=np.uint8)] + [np.full((8, 8), c, dtype=np.uint8)] * 2
    return ref_packets([IR.packed(flat)] * NFR, 16, 16, "420", LOSSLESS)


def checker_planes():
    sw, sh, _, _ = CHECKER
    return content_planes("checker", A.SUBSAMP_420, sw, sh)


@functools.lru_cache(maxsize=None)
def checker_reference(kind):
    sw, sh, w, h = CHECKER
    planes = checker_planes()
    if kind == "yuv":
        pic = IR.packed(IR.resize_yuv(list(planes), w, h, 1, 1))
    else:
        pic = IR.packed(IR.convert_sized(checker_pixels(), kind, w, h, 1, 1))
    return ref_packets([pic] * NFR, w, h, "420", CHECKER_CFG)


def checker_pixels():
    return np.repeat(checker_planes()[0][:, :, None], 4, axis=2).copy()


def every_reference():
    """(what, thunk) for every reference stream tests/test_gpu_enc_resize.py compares with (the mixed step's scaled stream and the
    ladder's are test_gpu_enc_scale.py's and the decoder's, built there)"""
    out = []
    for sw, sh, w, h in SOURCES_420 + [(sw, sh, 34, 18) for _, sw, sh, how in MIXED if how == "sized"]:
        for kind in ("yuv", BGRA709, RGBAFULL):
            out.append(("%dx%d->%dx%d 420 %s" % (sw, sh, w, h, kind), functools.partial(reference, sw, sh, w, h, "420", kind)))
    for name, sw, sh, w, h in FORMAT_SOURCES:
        for kind in ("yuv", BGRA709, RGBAFULL):
            out.append(("%dx%d->%dx%d %s %s" % (sw, sh, w, h, name, kind), functools.partial(reference, sw, sh, w, h, name, kind)))
    for kind in ("yuv", RGBAFULL):  # the encoder's own size
        out.append(("34x18->34x18 420 %s" % kind, functools.partial(reference, 34, 18, 34, 18, "420", kind)))
    out.append(("51x27->34x18 420 rgba601", functools.partial(reference, 51, 27, 34, 18, "420", R.RGBA)))
    for value in (0, 255):
        out.append(("constant %d" % value, functools.partial(constant_reference, value, value)))
        for layout in (BGRA709, RGBAFULL):
            px = np.full((1, 1, 4), value, dtype=np.uint8)
            y = int(R.convert(px, layout, 0, 0)[0][0, 0])
            out.append(("constant rgb %d %s" % (value, LAYOUT_IDS[layout]), functools.partial(constant_reference, y, 128)))
    for kind in ("yuv", BGRA709):
        out.append(("checker %s" % kind, functools.partial(checker_reference, kind)))
    return out
