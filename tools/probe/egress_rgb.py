#!/usr/bin/env python3
"""Decode steps delivering device-resident pictures three ways (experiments), the counterpart of tools/probe/ingest_rgb.py:
tools/probe/egress_rgb.py [packed] [bgra] [bgra_general]   (default: all three)
1080p 4:2:0, 64 decoders in one lockstep group, 12 timed steps behind the warm-up steps, on the same streams:
  packed        dsv2hip_dec_batch_device: packed planar pictures (k_egress<16>: 1.5 P bytes in, 1.5 P out)
  bgra          dsv2hip_dec_batch_surface, BGRA (BT.601, limited range), pitch 7680 (k_egress_rgb<packed, wide>: 1.5 P bytes in, 4 P out)
  bgra_general  the same one byte off alignment at pitch 7681 (k_egress_rgb<packed, general>)
The legs are interleaved step by step in one process -- leg A's step t, leg B's step t, leg C's step t, then step t + 1 -- each with
decoders and destinations of its own, so clock and load drift hit them alike.  Prints per leg the median and the minimum wall
time of a step, and of the span of its last stage (border extension + the picture's way out: dsv2hip_prof_read entry 7) per step
and per picture.  The kernels' own times: rocprofv3 --kernel-trace --stats -- python tools/probe/egress_rgb.py."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, S, WARM, STEPS, NVID = 1920, 1080, 64, 3, 12, 4
BGRA = 0x10


class OUTSURF(C.Structure):  # dsv2hip_out_surface
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("cap", C.c_size_t * 3), ("layout", C.c_int)]


def main():
    legs = sys.argv[1:] or ["packed", "bgra", "bgra_general"]
    import torch
    import dsvabi as A
    from codec_run import encode_stream
    from conftest import load_pkg
    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0
    P = C.POINTER
    hip.dsv2hip_dec_batch_device.argtypes = [C.c_int, P(P(A.DECODER)), P(A.BUF), P(C.c_void_p), P(C.c_size_t), P(C.c_uint32), P(C.c_int)]
    hip.dsv2hip_dec_batch_surface.argtypes = [C.c_int, P(P(A.DECODER)), P(A.BUF), P(OUTSURF), P(C.c_uint32), P(C.c_int)]
    hip.dsv2hip_prof_enable.argtypes = [C.c_int]
    hip.dsv2hip_prof_read.argtypes = [P(C.c_double), P(C.c_longlong), P(C.c_longlong)]
    nfr = WARM + STEPS
    vids = []
    for k in range(NVID):  # the packets come from the library's own encoder (identical to the reference's, and quick)
        v = load_pkg().synth.SynthVideo(W, H, "420", seed=501 + k)
        vids.append(encode_stream(hip, [v.frame_bytes(t) for t in range(nfr)], W, H, A.SUBSAMP_420, eos=False, qp=60, gop=48)[0])
    npk = len(vids[0])
    assert all(len(v) == npk for v in vids) and npk == nfr + 1  # metadata, then one packet a picture
    pic_bytes = W * H * 3 // 2

    class Leg:
        def __init__(self, name):
            self.name = name
            self.decs = [A.DECODER() for _ in range(S)]
            self.decp = (P(A.DECODER) * S)(*[C.pointer(d) for d in self.decs])
            self.fns, self.rets = (C.c_uint32 * S)(), (C.c_int * S)()
            self.wall, self.stage = [], []
            if name == "packed":
                self.keep = [torch.empty(pic_bytes, dtype=torch.uint8, device="cuda") for _ in range(S)]
                self.ptrs = (C.c_void_p * S)(*[t.data_ptr() for t in self.keep])
                self.caps = (C.c_size_t * S)(*[pic_bytes] * S)
            else:
                off, pitch = (1, 4 * W + 1) if name == "bgra_general" else (0, 4 * W)
                self.keep = [torch.empty(off + pitch * H, dtype=torch.uint8, device="cuda") for _ in range(S)]
                self.surfs = (OUTSURF * S)()
                for c, t in zip(self.surfs, self.keep):
                    assert t.data_ptr() % 16 == 0
                    c.layout, c.plane[0], c.pitch[0], c.cap[0] = BGRA, t.data_ptr() + off, pitch, pitch * H

        def step(self, t):
            bufs = (A.BUF * S)()
            for s in range(S):
                pk = vids[s % NVID][t]
                hip.dsv_mk_buf(C.byref(bufs[s]), len(pk) + 64)
                C.memmove(bufs[s].data, pk, len(pk))
            ms, ln, fr = (C.c_double * 9)(), (C.c_longlong * 9)(), C.c_longlong(0)
            hip.dsv2hip_prof_enable(1)  # (resets the totals: what is read below is this call's)
            t0 = time.perf_counter()
            if self.name == "packed":
                assert hip.dsv2hip_dec_batch_device(S, self.decp, bufs, self.ptrs, self.caps, self.fns, self.rets) == S
            else:
                assert hip.dsv2hip_dec_batch_surface(S, self.decp, bufs, self.surfs, self.fns, self.rets) == S
            el = time.perf_counter() - t0
            hip.dsv2hip_prof_read(ms, ln, C.byref(fr))
            hip.dsv2hip_prof_enable(0)
            if t > WARM:
                assert all(r == A.DEC_OK for r in self.rets)
                self.wall.append(1e3 * el)
                self.stage.append(ms[7])

    run = [Leg(name) for name in legs]
    torch.cuda.synchronize()
    for t in range(npk):
        for leg in run:
            leg.step(t)
    for leg in run:
        print("%-13s %dx%d %d decoders, %d steps: step %.2f ms median (%.2f min); last stage %.3f ms median (%.3f min) = %.2f us a picture"
              % (leg.name, W, H, S, len(leg.wall), statistics.median(leg.wall), min(leg.wall), statistics.median(leg.stage), min(leg.stage),
                 1e3 * statistics.median(leg.stage) / S), flush=True)
        for d in leg.decs:
            hip.dsv_dec_free(C.byref(d))


if __name__ == "__main__":
    main()
