#!/usr/bin/env python3
"""Decode steps delivering device-resident pictures as interleaved [h, w, 3] tensors and, for comparison, as a BGRA surface, as planar
[3, h, w] tensors and as planar tensors permuted to [h, w, 3] by torch afterwards -- what a caller does without the interleaved calls
(experiments), the counterpart of tools/probe/egress_tensor.py:
tools/probe/egress_hwc.py [legs ...]                      (default: all seventeen, in the order below)
tools/probe/egress_hwc.py --summarise KERNEL_TRACE.csv    (the same legs as the traced run)
1080p 4:2:0, 64 decoders in one lockstep group, 8 timed steps behind 3 warm-up steps, on the same streams, ImageNet's constants folded
(in B, G, R order for a BGR tensor):
  bgra            dsv2hip_dec_batch_surface, BGRA (BT.601, limited range), pitch 7680 (k_egress_rgb<packed, wide>: 1.5 P bytes in, 4 P out)
  ten_DT          dsv2hip_dec_batch_tensor into one [64, 3, h, w] tensor of element type DT (k_egress_rgb<planar, wide>: 3 / 6 / 6 / 12 P out)
  hwc_DT_rgb/bgr  dsv2hip_dec_batch_hwc into one [64, h, w, 3] tensor (k_egress_rgb<interleaved, wide>: the same bytes in and out as ten_DT)
  perm_DT         ten_DT, then torch's permute(0, 2, 3, 1).contiguous() of the whole batch -- one copy kernel for the 64 pictures,
                  the cheapest form of the caller's permute(1, 2, 0).contiguous() per picture
                  DT: u8, f16, bf16, f32
The legs are interleaved step by step in one process -- leg A's step t, leg B's step t, ... then step t + 1 -- each with decoders and
destinations of its own, so clock and load drift hit them alike.  Prints per leg the median and the minimum wall time of a step, and
checks on the last step that every hwc leg holds its type's planar tensor transposed, element for element.  The kernels' own times:
rocprofv3 --kernel-trace --output-format csv -- python tools/probe/egress_hwc.py, then --summarise on the trace: per leg the launches
behind the warm-up ones (a launch of the planar layout belongs to leg (its index mod the number of ten and perm legs), likewise the
interleaved layout and the copy kernel), mean, min - max and sigma in microseconds, and per element type the comparisons of DESIGN 5.24.
Launches are told apart by layout, so the traces of builds before the layouts shared k_egress_rgb read alike."""
import csv
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, S, WARM, STEPS, NVID = 1920, 1080, 64, 3, 8, 4
BGRA, RGB, BGR = 0x10, 0x21, 0x20
DTS = ["u8", "f16", "bf16", "f32"]
DTYPE = {"u8": 0, "f16": 1, "bf16": 2, "f32": 3}
ELEM = {"u8": 1, "f16": 2, "bf16": 2, "f32": 4}
SCALE = [1 / (255 * s) for s in (0.229, 0.224, 0.225)]
BIAS = [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
ALL = ["bgra"] + ["ten_" + d for d in DTS] + ["hwc_%s_%s" % (d, o) for d in DTS for o in ("rgb", "bgr")] + ["perm_" + d for d in DTS]


class OUTSURF(C.Structure):  # dsv2hip_out_surface
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("cap", C.c_size_t * 3), ("layout", C.c_int)]


class OUTTENSOR(C.Structure):  # dsv2hip_out_tensor
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_size_t * 3), ("cap", C.c_size_t * 3), ("dtype", C.c_int), ("csc", C.c_int), ("out_w", C.c_int),
                ("out_h", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class OUTHWC(C.Structure):  # dsv2hip_out_hwc
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_size_t), ("cap", C.c_size_t), ("dtype", C.c_int), ("order", C.c_int), ("csc", C.c_int),
                ("out_w", C.c_int), ("out_h", C.c_int), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


def layout_of(kernel):
    """the layout an egress conversion kernel writes -- k_egress_rgb<0 / 1 / 2, WIDE>, or before DESIGN 5.25 k_egress_rgb<WIDE>,
    k_egress_tensor<WIDE>, k_egress_hwc<WIDE> -- or None for any other kernel"""
    for name, layout in (("k_egress_tensor<", "planar"), ("k_egress_hwc<", "interleaved"), ("k_egress_rgb<0,", "packed"), ("k_egress_rgb<1,", "planar"),
                         ("k_egress_rgb<2,", "interleaved"), ("k_egress_rgb<true>", "packed"), ("k_egress_rgb<false>", "packed")):
        if name in kernel.replace(", ", ","):
            return layout
    return None


def summarise(path, legs):
    rows = list(csv.DictReader(open(path)))
    if rows and "Dispatch_Id" in rows[0]:
        rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    planar = [n for n in legs if n.startswith(("ten_", "perm_"))]
    hwc = [n for n in legs if n.startswith("hwc_")]
    perm = [n for n in legs if n.startswith("perm_")]
    per = {n: [] for n in legs}
    copies = {n: [] for n in perm}
    nt = nh = nc = 0
    for r in rows:
        k, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        layout = layout_of(k)
        if layout == "planar" and planar:
            per[planar[nt % len(planar)]].append(us)
            nt += 1
        elif layout == "interleaved" and hwc:
            per[hwc[nh % len(hwc)]].append(us)
            nh += 1
        elif layout == "packed" and "bgra" in per:
            per["bgra"].append(us)
        elif "dsv2" not in k and perm and nt and ("elementwise" in k or "copy" in k.lower()):
            copies[perm[nc % len(perm)]].append(us)
            nc += 1
    stats = {}

    def show(name, v):
        v = v[WARM:WARM + STEPS]
        stats[name] = (statistics.mean(v), statistics.pstdev(v))
        print("%-16s %d launches behind %d warm-up ones: mean %.1f us, %.1f - %.1f, sigma %.1f" % (name, len(v), WARM, statistics.mean(v), min(v), max(v),
                                                                                                statistics.pstdev(v)))
    for name in legs:
        show(name, per[name])
        if name in copies:
            show(name + " copy", copies[name])
    for d in DTS:
        if "ten_" + d not in stats:
            continue
        ten, sd = stats["ten_" + d]
        alt = stats["perm_" + d][0] + stats["perm_%s copy" % d][0] if "perm_" + d in stats else None
        for o in ("rgb", "bgr"):
            name = "hwc_%s_%s" % (d, o)
            if name not in stats:
                continue
            m = stats[name][0]
            margin = max(0.05 * ten, 2 * max(sd, stats[name][1]))
            print("%-16s %.1f us = %.3f x ten_%s (%.1f); within max(5 %%, 2 sigma) = %.1f us: %s; below planar + permute (%s us): %s" % (
                name, m, m / ten, d, ten, margin, "yes" if abs(m - ten) <= margin else "NO", "%.1f" % alt if alt else "-",
                ("yes" if m < alt else "NO") if alt else "-"))


def main():
    if sys.argv[1:2] == ["--summarise"]:
        return summarise(sys.argv[2], sys.argv[3:] or ALL)
    legs = sys.argv[1:] or ALL
    import torch
    import dsvabi as A
    from codec_run import encode_stream
    from conftest import load_pkg
    tdt = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
    tint = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
    hip = A.load_hip()
    assert hip.dsv2hip_device_ok() == 0
    P = C.POINTER
    hip.dsv2hip_dec_batch_tensor.argtypes = [C.c_int, P(P(A.DECODER)), P(A.BUF), P(OUTTENSOR), P(C.c_uint32), P(C.c_int)]
    hip.dsv2hip_dec_batch_surface.argtypes = [C.c_int, P(P(A.DECODER)), P(A.BUF), P(OUTSURF), P(C.c_uint32), P(C.c_int)]
    hip.dsv2hip_dec_batch_hwc.argtypes = [C.c_int, P(P(A.DECODER)), P(A.BUF), P(OUTHWC), P(C.c_uint32), P(C.c_int)]
    hip.dsv2hip_dec_hwc_stats.argtypes = [P(C.c_ulonglong), C.c_int]
    hip.dsv2hip_dec_hwc_stats.restype = None
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
            self.wall = []
            if name == "bgra":
                pitch = 4 * W
                self.keep = torch.empty((S, H, pitch), dtype=torch.uint8, device="cuda")
                self.out = (OUTSURF * S)()
                for s, c in enumerate(self.out):
                    c.layout, c.plane[0], c.pitch[0], c.cap[0] = BGRA, self.keep[s].data_ptr(), pitch, pitch * H
                self.call = hip.dsv2hip_dec_batch_surface
                return
            d = name.split("_")[1]
            e = ELEM[d]
            if name.startswith("hwc_"):
                bgr = name.endswith("_bgr")
                self.keep = torch.empty((S, H, W, 3), dtype=tdt[d], device="cuda")
                self.out = (OUTHWC * S)()
                for s, c in enumerate(self.out):
                    c.data, c.pitch, c.cap, c.dtype, c.order = self.keep[s].data_ptr(), 3 * W * e, 3 * W * H * e, DTYPE[d], BGR if bgr else RGB
                    for k in range(3):
                        c.scale[k], c.bias[k] = SCALE[2 - k if bgr else k], BIAS[2 - k if bgr else k]
                self.call = hip.dsv2hip_dec_batch_hwc
            else:
                self.keep = torch.empty((S, 3, H, W), dtype=tdt[d], device="cuda")
                self.out = (OUTTENSOR * S)()
                for s, c in enumerate(self.out):
                    c.dtype = DTYPE[d]
                    for ch in range(3):
                        c.plane[ch], c.pitch[ch], c.cap[ch] = self.keep[s, ch].data_ptr(), W * e, H * W * e
                        c.scale[ch], c.bias[ch] = SCALE[ch], BIAS[ch]
                self.call = hip.dsv2hip_dec_batch_tensor
            assert self.keep.data_ptr() % 256 == 0
            self.permuted = None

        def step(self, t):
            bufs = (A.BUF * S)()
            for s in range(S):
                pk = vids[s % NVID][t]
                hip.dsv_mk_buf(C.byref(bufs[s]), len(pk) + 64)
                C.memmove(bufs[s].data, pk, len(pk))
            t0 = time.perf_counter()
            assert self.call(S, self.decp, bufs, self.out, self.fns, self.rets) == S
            if self.name.startswith("perm_") and t > 0:  # (the round ends with its stream drained: the pictures are there)
                self.permuted = self.keep.permute(0, 2, 3, 1).contiguous()
                torch.cuda.synchronize()
            el = time.perf_counter() - t0
            if t > WARM:
                assert all(r == A.DEC_OK for r in self.rets)
                self.wall.append(1e3 * el)

    run = [Leg(name) for name in legs]
    hip.dsv2hip_dec_hwc_stats((C.c_ulonglong * 2)(), 1)
    torch.cuda.synchronize()
    for t in range(npk):
        for leg in run:
            leg.step(t)
    forms = (C.c_ulonglong * 2)()
    hip.dsv2hip_dec_hwc_stats(forms, 0)
    for leg in run:
        print("%-16s %dx%d %d decoders, %d steps: step %.2f ms median (%.2f min)" % (leg.name, W, H, S, len(leg.wall), statistics.median(leg.wall), min(leg.wall)),
              flush=True)
    print("hwc rounds: %d wide, %d general" % (forms[0], forms[1]))
    by = {leg.name: leg for leg in run}
    for leg in run:  # the last step's pictures: every hwc leg is its type's planar tensor transposed (BGR: the channels reversed)
        if leg.name.startswith("hwc_") and "ten_" + leg.name.split("_")[1] in by:
            d = leg.name.split("_")[1]
            want = by["ten_" + d].keep.permute(0, 2, 3, 1)
            if leg.name.endswith("_bgr"):
                want = want.flip(-1)
            e = ELEM[d]
            same = torch.equal(want.contiguous().view(tint[e]), leg.keep.view(tint[e]))
            print("%-16s equals ten_%s transposed: %s" % (leg.name, d, same), flush=True)
            assert same
    for leg in run:
        for d in leg.decs:
            hip.dsv_dec_free(C.byref(d))


if __name__ == "__main__":
    main()
