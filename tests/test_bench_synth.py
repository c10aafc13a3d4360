"""bench.py makes the headline's pictures with benchparts/synth_gpu.py (torch, on the GPU in a plain run); they must be the bytes of
the package's own generator (synth.py), which the golden fixtures and the --full legs use.  torch on the CPU runs the same integer
arithmetic, so no GPU is needed here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from benchparts.synth_gpu import DeviceVideo  # noqa: E402
from conftest import load_pkg  # noqa: E402


@pytest.mark.parametrize("w,h,fmt,seed,n", [(1920, 1080, "420", 1, 3), (1280, 720, "420", 101, 2), (640, 360, "444", 201, 2),
                                            (1920, 800, "420", 401, 2), (352, 288, "420", 96, 70), (354, 290, "420", 7, 4)])
def test_device_video_equals_synth(w, h, fmt, seed, n):
    torch = pytest.importorskip("torch")
    v = load_pkg().synth.SynthVideo(w, h, fmt, seed=seed)
    want = np.stack([np.frombuffer(v.frame_bytes(t), dtype=np.uint8) for t in range(n)])
    dv = DeviceVideo(w, h, fmt, seed, n, dev="cpu")
    assert len(dv) == n and dv.P == v.frame_size()
    got = dv.generate(torch).numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want)
