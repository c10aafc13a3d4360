#!/usr/bin/env python3
"""Decode steps delivering device-resident pictures as planar RGB tensors and, for comparison, as a BGRA surface (experiments;
DESIGN 5.21), the counterpart of tools/probe/egress_rgb.py:
tools/probe/egress_tensor.py [bgra] [u8] [f16] [bf16] [f32]   (default: all five, in this order)
1080p 4:2:0, 64 decoders in one lockstep group, 8 timed steps behind the warm-up steps, on the same streams:
  bgra          dsv2hip_dec_batch_surface, BGRA (BT.601, limited range), pitch 7680 (k_egress_rgb<packed, wide>: 1.5 P bytes in, 4 P out)
  u8 .. f32     dsv2hip_dec_batch_tensor into contiguous [3, h, w] tensors of the element type, ImageNet's constants folded
                (k_egress_rgb<planar, wide>: 1.5 P bytes in, 3 / 6 / 6 / 12 P out)
The legs are interleaved step by step in one process -- leg A's step t, leg B's step t, ... then step t + 1 -- each with decoders and
destinations of its own, so clock and load drift hit them alike; every launch of the planar layout in a kernel trace (k_egress_rgb<1, ...>;
k_egress_tensor before DESIGN 5.25) is then leg
(launch index mod number of tensor legs).  Prints per leg the median and the minimum wall time of a step, and of the span of its last
stage (border extension + the picture's way out: dsv2hip_prof_read entry 7) per step and per picture.  The kernels' own times:
rocprofv3 --kernel-trace -- python tools/probe/egress_tensor.py."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, S, WARM, STEPS, NVID = 1920, 1080, 64, 3, 8, 4
BGRA = 0x10
DTYPE = {"u8": 0, "f16": 1, "bf16": 2, "f32": 3}
ELEM = {"u8": 1, "f16": 2, "bf16": 2, "f32": 4}
SCALE = [1 / (255 * s) for s in (0.229, 0.224, 0.225)]
BIAS = [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]


class OUTSURF(C.Structure):  # dsv2hip_out_surface
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("cap", C.c_size_t * 3), ("layout", C.c_int)]


class OUTTENSOR(C.Structure):  # dsv2hip_out_tensor
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("cap", C.c_size_t * 3), ("dtype", C.c_int), ("csc", C.c_int), ("out_w", C.c_int),
                ("out_h", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]

def main():
    legs = sys.argv[1:] or ["bgra", "u8", "f16", "bf16", "f32"]
    import torch
    import dsvabi as A
    from codec_run import encode_stream
    from conftest import load_pkg
    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0
    P = C.POINTER
    hip.dsv2hip_dec_batch_tensor.argtypes = [C.c_int, P(P(A.DECODER)), P(A.BUF), P(OUTTENSOR), P(C.c_uint32), P(C.c_int)]
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

    class Leg:
        def __init__(self, name):
            self.name = name
            self.decs = [A.DECODER() for _ in range(S)]
            self.decp = (P(A.DECODER) * S)(*[C.pointer(d) for d in self.decs])
            self.fns, self.rets = (C.c_uint32 * S)(), (C.c_int * S)()
            self.wall, self.stage = [], []
            if name == "bgra":
                pitch = 4 * W
                self.keep = [torch.empty(pitch * H, dtype=torch.uint8, device="cuda") for _ in range(S)]
                self.surfs = (OUTSURF * S)()
                for c, t in zip(self.surfs, self.keep):
                    assert t.data_ptr() % 16 == 0
                    c.layout, c.plane[0], c.pitch[0], c.cap[0] = BGRA, t.data_ptr(), pitch, pitch * H
            else:
                e = ELEM[name]
                self.keep = [torch.empty(3 * H * W * e, dtype=torch.uint8, device="cuda") for _ in range(S)]  # a contiguous [3, h, w] tensor
                self.tens = (OUTTENSOR * S)()
                for c, t in zip(self.tens, self.keep):
                    assert t.data_ptr() % 16 == 0
                    c.dtype = DTYPE[name]
                    for ch in range(3):
                        c.plane[ch], c.pitch[ch], c.cap[ch] = t.data_ptr() + ch * H * W * e, W * e, H * W * e
                        c.scale[ch], c.bias[ch] = SCALE[ch], BIAS[ch]

        def step(self, t):
            bufs = (A.BUF * S)()
            for s in range(S):
                pk = vids[s % NVID][t]
                hip.dsv_mk_buf(C.byref(bufs[s]), len(pk) + 64)
                C.memmove(bufs[s].data, pk, len(pk))
            ms, ln, fr = (C.c_double * 9)(), (C.c_longlong * 9)(), C.c_longlong(0)
            hip.dsv2hip_prof_enable(1)  # (resets the totals: what is read below is this call's)
            t0 = time.perf_counter()
            if self.name == "bgra":
                assert hip.dsv2hip_dec_batch_surface(S, self.decp, bufs, self.surfs, self.fns, self.rets) == S
            else:
                assert hip.dsv2hip_dec_batch_tensor(S, self.decp, bufs, self.tens, self.fns, self.rets) == S
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
