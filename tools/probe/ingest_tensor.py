#!/usr/bin/env python3
"""Encode steps reading device-resident pictures as planar RGB float tensors and, for comparison, as a planar RGB surface (experiments;
DESIGN 5.22), the counterpart of tools/probe/egress_tensor.py:
tools/probe/ingest_tensor.py [rgbp] [f16] [bf16] [f32]   (default: all four, in this order)
tools/probe/ingest_tensor.py --summarise KERNEL_TRACE.csv [legs ...]
1080p 4:2:0, 192 encoders in one lockstep group, 8 timed steps behind 2 warm-up steps, on the same pixels:
  rgbp          dsv2hip_enc_batch_surface, RGBP (BT.709, limited range), three planes of pitch 1920 (k_ingest_rgb3<planar, wide>: 3 P
                bytes in, 1.5 P out)
  f16 .. f32    dsv2hip_enc_batch_tensor from contiguous [3, h, w] tensors of the element type that hold byte / 255, encoded under scale
                255, bias 0 (k_ingest_tensor<wide>: 6 / 6 / 12 P bytes in, 1.5 P out)
The legs are interleaved step by step in one process and take turns on ONE set of encoders -- leg A's step t, leg B's step t, ... then
step t + 1, every stream reading memory of its own -- so clock and load drift hit them alike; every launch of k_ingest_tensor in a
kernel trace is then leg (launch index mod number of tensor legs).  Prints per leg the median and the minimum wall time of a step.
The kernels' own times: rocprofv3 --kernel-trace --output-format csv -- python tools/probe/ingest_tensor.py, then --summarise on the
trace: per leg the launches behind the warm-up ones, mean, min - max and sigma in microseconds."""
import csv
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, S, WARM, STEPS = 1920, 1080, 192, 2, 8
RGBP, BT709 = 0x22, 0x100
DTYPE = {"f16": 1, "bf16": 2, "f32": 3}
ELEM = {"f16": 2, "bf16": 2, "f32": 4}
ALL = ["rgbp", "f16", "bf16", "f32"]


class SURFACE(C.Structure):  # dsv2hip_surface
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("layout", C.c_int)]


class INTENSOR(C.Structure):  # dsv2hip_in_tensor
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("dtype", C.c_int), ("csc", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


def summarise(path, legs):
    tensor_legs = [name for name in legs if name != "rgbp"]
    per = {name: [] for name in legs}
    nt = 0
    for r in csv.DictReader(open(path)):
        k, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "k_ingest_tensor" in k:
            per[tensor_legs[nt % len(tensor_legs)]].append(us)
            nt += 1
        elif "k_ingest_rgb3" in k and "rgbp" in per:
            per["rgbp"].append(us)
    for name in legs:
        v = per[name][WARM:]
        print("%-5s %d launches behind %d warm-up ones: mean %.1f us, %.1f - %.1f, sigma %.1f" % (name, len(v), WARM, statistics.mean(v), min(v), max(v), statistics.pstdev(v)))


def main():
    if sys.argv[1:2] == ["--summarise"]:
        return summarise(sys.argv[2], sys.argv[3:] or ALL)
    legs = sys.argv[1:] or ALL
    import torch
    import dsvabi as A
    from codec_run import configure_encoder
    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0
    P = C.POINTER
    hip.dsv2hip_enc_batch_tensor.argtypes = [C.c_int, P(P(A.ENCODER)), P(INTENSOR), P(A.BUF), P(C.c_int)]
    hip.dsv2hip_enc_batch_surface.argtypes = [C.c_int, P(P(A.ENCODER)), P(SURFACE), P(A.BUF), P(C.c_int)]
    hip.dsv2hip_enc_tensor_stats.argtypes = [P(C.c_ulonglong), C.c_int]
    meta = A.mk_meta(W, H, A.SUBSAMP_420)
    encs = [A.ENCODER() for _ in range(S)]
    for e in encs:
        configure_encoder(hip, e, meta, qp=60, gop=48)
    encp = (P(A.ENCODER) * S)(*[C.pointer(e) for e in encs])
    # the pixels: a smooth picture per stream, uint8 [3, h, w] on the device; every leg holds them in its own form and memory
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    keep, descs = {name: [] for name in legs}, {}
    for name in legs:
        descs[name] = (SURFACE * S)() if name == "rgbp" else (INTENSOR * S)()
    for s in range(S):
        px = torch.stack([128 + 100 * torch.sin((xx + 3 * s) / 37.0) * torch.cos(yy / 29.0), 128 + 90 * torch.sin((xx + yy + s) / 53.0), 120 + 80 * torch.cos((yy - 2 * s) / 41.0)])
        px = px.round().clamp(0, 255).to(torch.uint8)
        for name in legs:
            c = descs[name][s]
            if name == "rgbp":
                t = px.clone()
                c.layout = RGBP | BT709
                for ch in range(3):
                    c.plane[ch], c.pitch[ch] = t.data_ptr() + ch * H * W, W
            else:
                t = (px.to(torch.float32) / 255).to({"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]).contiguous()
                c.dtype, c.csc = DTYPE[name], BT709
                for ch in range(3):
                    c.plane[ch], c.pitch[ch], c.scale[ch], c.bias[ch] = t.data_ptr() + ch * H * W * ELEM[name], W * ELEM[name], 255.0, 0.0
            assert t.data_ptr() % 16 == 0
            keep[name].append(t)
    torch.cuda.synchronize()
    bufs, nbufs = (A.BUF * (4 * S))(), (C.c_int * S)()
    wall = {name: [] for name in legs}
    for t in range(WARM + STEPS):
        for name in legs:
            t0 = time.perf_counter()
            if name == "rgbp":
                assert hip.dsv2hip_enc_batch_surface(S, encp, descs[name], bufs, nbufs) == 0
            else:
                assert hip.dsv2hip_enc_batch_tensor(S, encp, descs[name], bufs, nbufs) == 0
            el = time.perf_counter() - t0
            for s in range(S):
                for i in range(nbufs[s]):
                    hip.dsv_buf_free(C.byref(bufs[4 * s + i]))
            if t >= WARM:
                wall[name].append(1e3 * el)
    forms = (C.c_ulonglong * 2)()
    hip.dsv2hip_enc_tensor_stats(forms, 0)
    assert forms[1] == 0, "a tensor step ran in the general form"
    for name in legs:
        print("%-5s %dx%d %d encoders, %d steps: step %.2f ms median (%.2f min)" % (name, W, H, S, len(wall[name]), statistics.median(wall[name]), min(wall[name])), flush=True)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))


if __name__ == "__main__":
    main()
