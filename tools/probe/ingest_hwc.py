#!/usr/bin/env python3
"""Encode steps reading device-resident pictures as interleaved [h, w, 3] float tensors and, for comparison, as planar tensors and as
what a caller without the interleaved calls does (experiments), the counterpart of tools/probe/egress_hwc.py:
tools/probe/ingest_hwc.py [f16] [bf16] [f32]   (default: all three, in this order)
tools/probe/ingest_hwc.py --summarise KERNEL_TRACE.csv [types ...]
1080p 4:2:0, 192 encoders in one lockstep group, 8 timed steps behind 2 warm-up steps, on the same pixels (every float holds byte / 255,
encoded under scale 255, bias 0; BT.709, limited range); per element type four legs:
  planar    dsv2hip_enc_batch_tensor from a contiguous [192, 3, h, w] tensor (k_ingest_tensor<wide>)
  hwc_rgb   dsv2hip_enc_batch_hwc from a contiguous [192, h, w, 3] tensor, order R G B (k_ingest_hwc<wide>)
  hwc_bgr   the same from a tensor that holds B G R
  permute   the caller's alternative: ONE batched permute(0, 3, 1, 2) of the 192 R G B pictures into a contiguous [192, 3, h, w] tensor
            (torch's copy kernel), then dsv2hip_enc_batch_tensor on that
The legs are interleaved step by step in one process and take turns on ONE set of encoders -- type by type, leg by leg, then the next
step; every leg reads memory of its own -- so clock and load drift hit them alike.  In a kernel trace the launches of k_ingest_tensor
then alternate planar, permute and those of k_ingest_hwc rgb, bgr, type by type; the only kernels of torch's between the first and the
last ingest launch are the permutes' copies.  Prints per leg the median and the minimum wall time of a step.
The kernels' own times: rocprofv3 --kernel-trace --output-format csv -- python tools/probe/ingest_hwc.py, then --summarise on the
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
BGR, RGB, BT709 = 0x20, 0x21, 0x100
DTYPE = {"f16": 1, "bf16": 2, "f32": 3}
ELEM = {"f16": 2, "bf16": 2, "f32": 4}
ALL = ["f16", "bf16", "f32"]
LEGS = ["planar", "hwc_rgb", "hwc_bgr", "permute"]


class INTENSOR(C.Structure):  # dsv2hip_in_tensor
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("dtype", C.c_int), ("csc", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class INHWC(C.Structure):  # dsv2hip_in_hwc
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_size_t), ("dtype", C.c_int), ("order", C.c_int), ("csc", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


def line(name, v):
    print("%-16s %d launches behind %d warm-up ones: mean %.1f us, %.1f - %.1f, sigma %.1f" % (name, len(v), WARM, statistics.mean(v), min(v), max(v), statistics.pstdev(v)))


def summarise(path, types):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ingest = [i for i, r in enumerate(rows) if "k_ingest_tensor" in r["Kernel_Name"] or "k_ingest_hwc" in r["Kernel_Name"]]
    per = {(t, leg): [] for t in types for leg in LEGS + ["permute_copy"]}
    nt = nh = 0
    pending, pieces = 0.0, 0  # torch's kernels since the last ingest launch: a permute's copy, in as many pieces as torch split it into
    for r in rows[ingest[0]:ingest[-1] + 1]:
        k, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "k_ingest_tensor" in k:
            t = types[(nt // 2) % len(types)]
            per[(t, "planar" if nt % 2 == 0 else "permute")].append(us)
            if nt % 2:
                assert pieces >= 1, "no copy in front of a permute leg's ingest"
                per[(t, "permute_copy")].append(pending)
            else:
                assert pieces == 0, "a torch kernel in front of a planar leg's ingest"
            pending, pieces = 0.0, 0
            nt += 1
        elif "k_ingest_hwc" in k:
            assert pieces == 0, "a torch kernel in front of an interleaved leg's ingest"
            per[(types[(nh // 2) % len(types)], "hwc_rgb" if nh % 2 == 0 else "hwc_bgr")].append(us)
            nh += 1
        elif "at::native" in k:  # (torch's kernels: between the first and the last ingest launch only the permutes' copies)
            pending, pieces = pending + us, pieces + 1
    steps = WARM + STEPS
    assert nt == 2 * steps * len(types) and nh == 2 * steps * len(types), (nt, nh)
    for t in types:
        for leg in LEGS[:3]:
            line("%s %s" % (t, leg), per[(t, leg)][WARM:])
        line("%s permute copy" % t, per[(t, "permute_copy")][WARM:])
        line("%s permute ingest" % t, per[(t, "permute")][WARM:])
        line("%s permute both" % t, [a + b for a, b in zip(per[(t, "permute_copy")][WARM:], per[(t, "permute")][WARM:])])


def main():
    if sys.argv[1:2] == ["--summarise"]:
        return summarise(sys.argv[2], sys.argv[3:] or ALL)
    types = sys.argv[1:] or ALL
    import torch
    import dsvabi as A
    from codec_run import configure_encoder
    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0
    P = C.POINTER
    hip.dsv2hip_enc_batch_tensor.argtypes = [C.c_int, P(P(A.ENCODER)), P(INTENSOR), P(A.BUF), P(C.c_int)]
    hip.dsv2hip_enc_batch_hwc.argtypes = [C.c_int, P(P(A.ENCODER)), P(INHWC), P(A.BUF), P(C.c_int)]
    hip.dsv2hip_enc_tensor_stats.argtypes = [P(C.c_ulonglong), C.c_int]
    hip.dsv2hip_enc_hwc_stats.argtypes = [P(C.c_ulonglong), C.c_int]
    meta = A.mk_meta(W, H, A.SUBSAMP_420)
    encs = [A.ENCODER() for _ in range(S)]
    for e in encs:
        configure_encoder(hip, e, meta, qp=60, gop=48)
    encp = (P(A.ENCODER) * S)(*[C.pointer(e) for e in encs])
    # the pixels: a smooth picture per stream, uint8 [S, 3, h, w] on the device; every leg holds them in its own form and memory
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    px = torch.empty((S, 3, H, W), dtype=torch.uint8, device="cuda")
    for s in range(S):
        one = torch.stack([128 + 100 * torch.sin((xx + 3 * s) / 37.0) * torch.cos(yy / 29.0), 128 + 90 * torch.sin((xx + yy + s) / 53.0), 120 + 80 * torch.cos((yy - 2 * s) / 41.0)])
        px[s] = one.round().clamp(0, 255).to(torch.uint8)
    keep, descs = {}, {}

    def planar_descs(t, name):
        d = (INTENSOR * S)()
        for s in range(S):
            d[s].dtype, d[s].csc = DTYPE[name], BT709
            for ch in range(3):
                d[s].plane[ch], d[s].pitch[ch], d[s].scale[ch], d[s].bias[ch] = t[s, ch].data_ptr(), W * ELEM[name], 255.0, 0.0
        return d

    def hwc_descs(t, name, order):
        d = (INHWC * S)()
        for s in range(S):
            d[s].data, d[s].pitch, d[s].dtype, d[s].order, d[s].csc = t[s].data_ptr(), 3 * W * ELEM[name], DTYPE[name], order, BT709
            for k in range(3):
                d[s].scale[k], d[s].bias[k] = 255.0, 0.0
        return d

    for name in types:
        dt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[name]
        planar = torch.empty((S, 3, H, W), dtype=dt, device="cuda")
        for s in range(S):  # (picture by picture: no float32 copy of the whole batch)
            planar[s] = (px[s].to(torch.float32) / 255).to(dt)
        rgb = planar.permute(0, 2, 3, 1).contiguous()           # [S, h, w, 3], R G B
        bgr = planar.flip(1).permute(0, 2, 3, 1).contiguous()   # ... B G R
        permuted = torch.empty_like(planar)                     # what the permute leg writes and then encodes from
        for t in (planar, rgb, bgr, permuted):
            assert t.is_contiguous() and t.data_ptr() % 16 == 0
        keep[name] = (planar, rgb, bgr, permuted)
        descs[name] = {"planar": planar_descs(planar, name), "hwc_rgb": hwc_descs(rgb, name, RGB), "hwc_bgr": hwc_descs(bgr, name, BGR), "permute": planar_descs(permuted, name)}
    del px
    torch.cuda.synchronize()
    bufs, nbufs = (A.BUF * (4 * S))(), (C.c_int * S)()
    wall = {(name, leg): [] for name in types for leg in LEGS}
    for t in range(WARM + STEPS):
        for name in types:
            for leg in LEGS:
                t0 = time.perf_counter()
                if leg == "permute":
                    keep[name][3].copy_(keep[name][1].permute(0, 3, 1, 2))  # (= permute(0, 3, 1, 2).contiguous() into memory that stays put)
                    torch.cuda.synchronize()  # (torch's stream; the encoder runs on its own)
                if leg.startswith("hwc"):
                    assert hip.dsv2hip_enc_batch_hwc(S, encp, descs[name][leg], bufs, nbufs) == 0
                else:
                    assert hip.dsv2hip_enc_batch_tensor(S, encp, descs[name][leg], bufs, nbufs) == 0
                el = time.perf_counter() - t0
                for s in range(S):
                    for i in range(nbufs[s]):
                        hip.dsv_buf_free(C.byref(bufs[4 * s + i]))
                if t >= WARM:
                    wall[(name, leg)].append(1e3 * el)
    forms = (C.c_ulonglong * 2)()
    hip.dsv2hip_enc_tensor_stats(forms, 0)
    assert forms[1] == 0, "a planar tensor step ran in the general form"
    hip.dsv2hip_enc_hwc_stats(forms, 0)
    assert forms[1] == 0 and forms[0] == 2 * (WARM + STEPS) * len(types), "an interleaved tensor step ran in the general form"
    for name in types:
        assert torch.equal(keep[name][3].view(torch.uint8), keep[name][0].view(torch.uint8))  # (the permute leg encoded the planar leg's elements)
        for leg in LEGS:
            v = wall[(name, leg)]
            print("%-5s %-8s %dx%d %d encoders, %d steps: step %.2f ms median (%.2f min)" % (name, leg, W, H, S, len(v), statistics.median(v), min(v)), flush=True)
    for e in encs:
        hip.dsv_enc_free(C.byref(e))


if __name__ == "__main__":
    main()
