"""Half, quarter and eighth-size delivery without a GPU: the thread body of k_egress_scale (csrc/egress_scale.h) compiled for the host
and swept under AddressSanitizer + UndefinedBehaviorSanitizer by tools/egress_scale_check.cpp (a stand-alone program: nothing
sanitized is loaded into Python), its dumped planes against the numpy oracle tests/box_reduce.py -- which pins the kernel's text, the
program's C restatement and the oracle of tests/test_gpu_dec_scale.py to one another -- and what include/dsv2_hip.h says of the
reduction: half size is the reference's dsv_ds2x_frame_luma, constants stay, and the reduced picture has dsv_mk_frame's plane sizes.
"""
import os
import re

import numpy as np
import pytest

import box_reduce as B
import dsvabi as A
from sanitized_tool import build_and_run

FORMATS = [0x0, 0x4, 0x5, 0x8, 0xA]  # DSV_SUBSAMP_444, _422, _420, _411, _410


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    """builds tools/egress_scale_check.cpp with the sanitizers, runs its whole sweep and returns the directory of its dumped cases"""
    out, dump = build_and_run("tools/egress_scale_check.cpp", tmp_path_factory.mktemp("egress_scale"), ["--dump", "{dump}"])
    assert "in the wide form" in out
    return dump


def test_kernel_body_sweep_is_clean_and_equals_the_numpy_oracle(dump_dir):
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".src"))
    assert len(names) >= 10
    seen, odd = set(), set()
    for name in names:
        m = re.fullmatch(r"s([123])_(wide|general)_(\d+)x(\d+)", name)
        assert m, name
        s, form, w, h = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        src = np.fromfile(os.path.join(dump_dir, name + ".src"), dtype=np.uint8)
        assert src.size == w * h, name
        want = B.reduce(src.reshape(h, w), s)
        got = np.fromfile(os.path.join(dump_dir, name + ".out"), dtype=np.uint8)
        assert got.size == want.size, name
        bad = np.flatnonzero(got != want.reshape(-1))
        assert bad.size == 0, "%s: sample %d is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want.reshape(-1)[bad[0]])
        seen.add((s, form))
        n = 1 << s
        odd |= {"w"} if w % n else set()
        odd |= {"h"} if h % n else set()
    assert seen == {(s, form) for s in (1, 2, 3) for form in ("wide", "general")}  # every shift in both forms
    assert odd == {"w", "h"}  # partial footprints in both directions


# ---- the oracle's own properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(16, 16), (34, 18), (130, 66), (352, 288)])
def test_half_size_is_the_references_ds2x(w, h):
    """s = 1 on an even-sized luma plane of random content equals dsv_ds2x_frame_luma (frame.c:211) of the reference library"""
    ref = A.load_ref()
    rng = np.random.default_rng(w * 1000 + h)
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    src, dst = A.HostFrame(A.SUBSAMP_420, w, h, border=True), A.HostFrame(A.SUBSAMP_420, w // 2, h // 2, border=True)
    src.plane(0)[:, :] = y
    ref.dsv_ds2x_frame_luma(dst.ptr(), src.ptr())
    assert np.array_equal(B.reduce(y, 1), dst.plane(0))


@pytest.mark.parametrize("s", [1, 2, 3])
def test_constants_stay_and_a_checkerboard_is_128(s):
    for w, h in ((16, 16), (17, 19), (5, 3), (1, 1)):
        for value in (0, 1, 254, 255):
            out = B.reduce(np.full((h, w), value, dtype=np.uint8), s)
            assert out.shape == (B.reduced_size(h, s), B.reduced_size(w, s)) and np.all(out == value)
    yy, xx = np.mgrid[0:24, 0:40]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    assert np.all(B.reduce(board, s) == 128)  # (n * n / 2 * 255 + n * n / 2) >> 2s = 127.5 + 0.5


def test_one_rounding_over_the_footprint_not_pairwise():
    """a quarter-size sample whose iterated pairwise average differs: the contract is the single rounding"""
    p = np.zeros((4, 4), dtype=np.uint8)
    p[0, 0] = p[2, 2] = 2  # each 2 x 2 block: (2 + 2) >> 2 = 1 twice, then (1 + 0 + 0 + 1 + 2) >> 2 = 1; in one go (4 + 8) >> 4 = 0
    assert B.reduce(p, 2)[0, 0] == 0
    assert B.reduce(B.reduce(p, 1), 1)[0, 0] == 1


def test_edge_footprints_repeat_the_edge_pixel():
    p = np.arange(15, dtype=np.uint8).reshape(3, 5) * 17
    for s in (1, 2, 3):
        n = 1 << s
        out = B.reduce(p, s)
        for y in range(out.shape[0]):
            for x in range(out.shape[1]):
                total = sum(int(p[min(y * n + j, 2), min(x * n + i, 4)]) for j in range(n) for i in range(n))
                assert out[y, x] == (total + (1 << (2 * s - 1))) >> (2 * s)


@pytest.mark.parametrize("fmt", FORMATS, ids=["444", "422", "420", "411", "410"])
def test_reduced_plane_sizes_are_mk_frames(fmt):
    """each plane reduced on its own has exactly dsv_mk_frame's sizes for (ceil(w / n), ceil(h / n)): nested round-ups commute"""
    ref = A.load_ref()
    hs, vs = A.format_shifts(fmt)
    cache = {}

    def mk_dims(w, h):
        if (w, h) not in cache:
            f = ref.dsv_mk_frame(fmt, w, h, 1)
            cache[(w, h)] = [(f.contents.planes[c].w, f.contents.planes[c].h) for c in range(3)]
            ref.dsv_frame_ref_dec(f)
        return cache[(w, h)]

    for w in range(16, 81):
        for h in range(16, 81):
            cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
            for s in (1, 2, 3):
                each = [(B.reduced_size(pw, s), B.reduced_size(ph, s)) for pw, ph in ((w, h), (cw, ch), (cw, ch))]
                assert each == mk_dims(B.reduced_size(w, s), B.reduced_size(h, s)), (w, h, s)
    y, u, v = (np.zeros((d[1], d[0]), dtype=np.uint8) for d in mk_dims(34, 18))
    assert [p.shape[::-1] for p in B.reduce_picture(y, u, v, 3)] == mk_dims(5, 3)
