"""The reference's own CLI linked against libdsv2hip.so (oracle/_ref/dsv2_dropin): `d -drawinfo=7` writes the pictures the pure
reference build (oracle/_ref/dsv2_ref) writes -- grid, dashes, vectors and intra marks included."""
import os

import pytest

import dsvabi as A
from conftest import load_pkg
from test_gpu_cli import DROPIN, md5, run

pytestmark = [pytest.mark.gpu]  # (a GPU box without oracle/_ref FAILS these tests: conftest.py)


def test_cli_drawinfo_pictures_identical(tmp_path):
    for exe in (A.REF_CLI, DROPIN):
        assert os.path.exists(exe), "oracle/_ref is not built (%s)" % os.path.relpath(exe, A.ROOT)
    pkg = load_pkg()
    w, h, n = 352, 288, 14
    v = pkg.synth.SynthVideo(w, h, "420", seed=11)
    y4m, dsv = str(tmp_path / "in.y4m"), str(tmp_path / "in.dsv")
    pkg.synth.write_y4m(y4m, v, n)
    run([A.REF_CLI, "e", "-inp=" + y4m, "-out=" + dsv, "-y4m=1", "-y", "-nfr=%d" % n, "-qp=60", "-gop=6", "-effort=10"])
    out = {}
    for name, exe, flags in (("ref", A.REF_CLI, ["-drawinfo=7"]), ("hip", DROPIN, ["-drawinfo=7"]), ("plain", A.REF_CLI, [])):
        yuv = str(tmp_path / (name + ".yuv"))
        run([exe, "d", "-inp=" + dsv, "-out=" + yuv, "-y"] + flags)
        assert os.path.getsize(yuv) == n * v.frame_size()
        out[name] = md5(yuv)
    assert out["ref"] != out["plain"], "-drawinfo=7 draws nothing"
    assert out["ref"] == out["hip"], "drawn pictures differ"
