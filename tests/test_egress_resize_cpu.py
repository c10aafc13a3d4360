"""Delivery at any smaller size without a GPU: the thread body of k_egress_resize (csrc/egress_resize.h) compiled for the host and swept
under AddressSanitizer + UndefinedBehaviorSanitizer by tools/egress_resize_check.cpp (a stand-alone program: nothing sanitized is
loaded into Python), its dumped planes against the numpy oracle tests/area_resize.py -- which pins the kernel's text, the program's C
restatement and the oracle of tests/test_gpu_dec_resize.py to one another -- and what include/dsv2_hip.h says of the resampling: the
weights sum to a, exact ratios of 2, 4, 8 are the existing reduction, constants stay, the sums fit 32 bits, and the delivered picture
has dsv_mk_frame's plane sizes.
"""
import os
import re
import signal
import subprocess
import sys

import numpy as np
import pytest

import area_resize as R
import box_reduce as B
import dsvabi as A
from sanitized_tool import build_and_run

FORMATS = [0x0, 0x4, 0x5, 0x8, 0xA]  # DSV_SUBSAMP_444, _422, _420, _411, _410
SHAPES = R.SWEEP_SHAPES


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    """builds tools/egress_resize_check.cpp with the sanitizers, runs its whole sweep and returns the directory of its dumped cases"""
    out, dump = build_and_run("tools/egress_resize_check.cpp", tmp_path_factory.mktemp("egress_resize"), ["--dump", "{dump}"])
    assert "in the wide form" in out and "quotients of the division helper" in out
    return dump


def test_kernel_body_sweep_is_clean_and_equals_the_numpy_oracle(dump_dir):
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".src"))
    seen = set()
    for name in names:
        m = re.fullmatch(r"(wide|general)_(\d+)x(\d+)_(\d+)x(\d+)(?:_c(\d+))?", name)
        assert m, name
        form = m.group(1)
        pw, ph, ow, oh = (int(g) for g in m.group(2, 3, 4, 5))
        src = np.fromfile(os.path.join(dump_dir, name + ".src"), dtype=np.uint8)
        assert src.size == pw * ph, name
        src = src.reshape(ph, pw)
        if m.group(6) is not None:
            assert np.all(src == int(m.group(6))), name
        want = R.resize(src, ow, oh)
        got = np.fromfile(os.path.join(dump_dir, name + ".out"), dtype=np.uint8)
        assert got.size == want.size, name
        bad = np.flatnonzero(got != want.reshape(-1))
        assert bad.size == 0, "%s: sample %d is %d, the oracle says %d" % (name, bad[0], got[bad[0]], want.reshape(-1)[bad[0]])
        if m.group(6) is not None:
            assert np.all(got == int(m.group(6))), name  # constant planes stay constant
        if (pw, ph) == (ow, oh):
            assert np.array_equal(got.reshape(oh, ow), src), name  # the identity
        for s in (1, 2, 3):
            if (pw, ph) == (ow << s, oh << s):
                assert np.array_equal(got.reshape(oh, ow), B.reduce(src, s)), name  # the existing reduction
        seen.add((form, (pw, ph, ow, oh), m.group(6)))
    for shape in SHAPES:
        for const in (None, "0", "1", "254", "255"):
            for form in ("wide", "general"):  # (every destination list of the program holds aligned and offset destinations)
                assert (form, shape, const) in seen, (form, shape, const)


def test_the_bounds_of_the_call_equal_the_oracles(dump_dir):
    """resize_allowed (io_jobs.h), which the three sized calls refuse by, at and around every bound -- ratio 8 and 1 per axis, sizes that are
    not positive, a side of 32 768, D = 2^24 -- against the oracle's restatement; both verdicts occur, for each kind of bound"""
    rows = [[int(v) for v in line.split()] for line in open(os.path.join(dump_dir, "allowed.txt"))]
    assert len(rows) >= 40
    for pw, ph, ow, oh, verdict in rows:
        assert bool(verdict) == R.allowed(pw, ph, ow, oh), (pw, ph, ow, oh)
    verdicts = {(pw, ph, ow, oh): bool(v) for pw, ph, ow, oh, v in rows}
    assert verdicts[(4096, 4096, 4095, 4095)] and verdicts[(4093, 4099, 4092, 4098)] and verdicts[(4100, 4100, 4098, 4098)]  # D <= 2^24
    assert not verdicts[(4097, 4097, 4096, 4096)] and not verdicts[(4100, 4100, 4099, 4099)] and not verdicts[(4097, 4097, 2049, 2049)]  # D > 2^24
    assert verdicts[(32768, 16, 32767, 16)] and not verdicts[(32769, 16, 32768, 16)] and not verdicts[(16, 32769, 16, 32768)]  # a side
    assert verdicts[(64, 48, 8, 6)] and not verdicts[(64, 48, 7, 6)] and not verdicts[(64, 48, 65, 48)] and not verdicts[(64, 48, 0, 0)]


# ---- the oracle's own properties ----------------------------------------------------------------------------------------------------
def test_weights_sum_to_a_and_cover_every_source_pixel_b_times():
    pairs = [(src, dst) for src in range(1, 90) for dst in range((src + 7) // 8, src + 1)]
    for src, dst in pairs + [(1080, 720), (1079, 719), (1920, 1280), (1919, 1279), (1920, 240), (1919, 240)]:
        a, b = R.ratio(src, dst)
        w = R.weights(src, dst)
        assert np.all(w.sum(axis=1) == a) and np.all(w.sum(axis=0) == b), (src, dst)
        assert np.count_nonzero(w, axis=1).max() <= 9, (src, dst)  # a footprint spans at most 9 source pixels


def test_exact_ratios_are_the_existing_reduction():
    """pw = n * ow and ph = n * oh for n = 2, 4, 8: exactly box_reduce.reduce, for all exactly divisible (w, h, s) with w, h in 16 .. 80"""
    rng = np.random.default_rng(7)
    full = rng.integers(0, 256, (80, 80), dtype=np.uint8)
    full[rng.random((80, 80)) < 0.2] = 255
    count = 0
    for s in (1, 2, 3):
        n = 1 << s
        for w in range(16, 81):
            for h in range(16, 81):
                if w % n == 0 and h % n == 0:
                    p = full[:h, :w]
                    assert np.array_equal(R.resize(p, w // n, h // n), B.reduce(p, s)), (w, h, s)
                    count += 1
    assert count > 1000
    assert np.array_equal(R.resize(full, 80, 80), full)  # the identity


def test_an_odd_width_at_half_size_differs_from_scale_half():
    """DSV2HIP_SCALE_HALF repeats the edge pixel; the sized delivery to ceil(w / 2) spreads the ratio over the row"""
    p = (np.arange(5, dtype=np.uint8) * 50)[None, :]
    assert B.reduce(p, 1).tolist() == [[25, 125, 200]]  # the last footprint is pixel 4 twice
    # 5 -> 3: a = 5, b = 3; sample 2 covers [10, 15): pixel 3 from 10 to 12 and pixel 4 whole: (2 * 150 + 3 * 200 + 2) // 5
    assert R.resize(p, 3, 1).tolist() == [[(3 * 0 + 2 * 50 + 2) // 5, (1 * 50 + 3 * 100 + 1 * 150 + 2) // 5, (2 * 150 + 3 * 200 + 2) // 5]]


def test_constants_stay_and_the_sums_fit_32_bits():
    for pw, ph, ow, oh in SHAPES:
        for value in (0, 1, 254, 255):
            assert np.all(R.resize(np.full((ph, pw), value, dtype=np.uint8), ow, oh) == value)
    assert 255 * R.MAX_D + R.MAX_D // 2 < 1 << 32
    a, c = R.ratio(1919, 1279)[0], R.ratio(1079, 719)[0]
    assert a * c == 2070601
    assert R.ratio(1920, 1280) == (3, 2) and R.ratio(1080, 720) == (3, 2)
    assert not R.allowed(4099, 4099, 4098, 4098) and R.allowed(4093, 4099, 4092, 4098)  # D just above / below 2^24
    assert not R.allowed(64, 48, 7, 48) and not R.allowed(64, 48, 65, 48) and not R.allowed(64, 48, 64, 5) and not R.allowed(64, 48, 0, 0)


@pytest.mark.parametrize("fmt", FORMATS, ids=["444", "422", "420", "411", "410"])
def test_sized_plane_sizes_are_mk_frames(fmt):
    """the delivered picture has exactly dsv_mk_frame's plane sizes for every allowed (out_w, out_h), and every chroma plane is inside the
    bounds that the luma's bounds imply"""
    ref = A.load_ref()
    hs, vs = A.format_shifts(fmt)
    cache = {}

    def mk_dims(w, h):
        if (w, h) not in cache:
            f = ref.dsv_mk_frame(fmt, w, h, 1)
            cache[(w, h)] = [(f.contents.planes[c].w, f.contents.planes[c].h) for c in range(3)]
            ref.dsv_frame_ref_dec(f)
        return cache[(w, h)]

    for w, h in ((34, 18), (50, 38), (64, 48)):
        full = mk_dims(w, h)
        for ow in range((w + 7) // 8, w + 1):
            for oh in range((h + 7) // 8, h + 1):
                sizes = R.plane_sizes(ow, oh, hs, vs)
                assert sizes == mk_dims(ow, oh), (w, h, ow, oh)
                for (pw, ph), (sw, sh) in zip(full, sizes):
                    assert R.allowed(pw, ph, sw, sh), (w, h, ow, oh)
    y, u, v = (np.zeros((d[1], d[0]), dtype=np.uint8) for d in mk_dims(50, 38))
    assert [p.shape[::-1] for p in R.resize_picture(y, u, v, 33, 21, hs, vs)] == mk_dims(33, 21)


# ---- why tests/test_gpu_dec_resize.py takes its 4:1:1 and "4:1:0" streams from 54x38 ---------------------------------------------------
def reference_stream(fmt, w, h):
    """the return code of a child process that has the reference encoder make tests/dec_out.format_stream(fmt, w, h, 3)
    (a child: where the encoder is not defined it ends the process that calls it)"""
    code = "from test_gpu_dec_device_out import format_stream; assert len(format_stream(%r, %d, %d, 3)) >= 4" % (fmt, w, h)
    env = dict(os.environ, PYTHONPATH=os.path.join(A.ROOT, "tests"))
    return subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120).returncode


@pytest.mark.parametrize("fmt", ["411", "410"])
def test_the_reference_encoder_makes_no_411_or_410_stream_at_50x38(fmt):
    """The reference encoder divides by zero at 50x38 in these two formats, so the five-format test of the sized delivery takes their
    streams from 54x38, where it is defined (and from 50x38 for the three other formats)."""
    A.load_ref()
    assert reference_stream(fmt, 50, 38) == -signal.SIGFPE
    assert reference_stream(fmt, 54, 38) == 0
