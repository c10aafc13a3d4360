// dec_plan_check.cpp -- the decoder's delivery planner (csrc/dec_delivery.h) swept on the CPU for tensor targets, planar
// (dsv2hip_dec_batch_tensor) and interleaved (dsv2hip_dec_batch_hwc): chroma format x picture size x element type x order x sized or not x
// postsharp x draw_info x pointer offset x pitch, over FAKE addresses as tools/dec_delivery_check.cpp does -- the reconstruction, the two
// staging areas and the target are disjoint ranges of one synthetic address space, and nothing is ever dereferenced.  Meant to be built
// with AddressSanitizer and UndefinedBehaviorSanitizer (the planner is handed no staging area it says it does not need: a look at one
// faults).
//   tensors   target_tensor / target_hwc take a tensor that holds the rows exactly and refuse one a byte short, a pitch or a pointer off
//             the element grid, a pitch below the row or beyond an int, a constant that is not finite (uint8: the constants are not looked
//             at) and, interleaved, an order that is not exactly RGB or BGR; the predicates ask for the staged luma exactly for a
//             sharpened or drawn-on picture and for the staged (full-size) scaled picture exactly for a sized one; the plan holds one
//             conversion job of the target's layout behind the luma's egress job and the three resampling jobs, reading what they
//             staged, writing the tensor's rows, with the preset's coefficients, the element type, the order and the constants; rgb_wide
//             is rgb_out_job_wide of the job.  One line per case goes to stdout for tests/test_dec_plan_cpu.py to compare with its own
//             restatement of the rules:
//               R fmt w h dtype ow oh sharp draw offset pitch_kind : n_eg n_rsz n_rgb n_overlay sharpen_overlaid wide luma scaled full
//               H fmt w h dtype bgr ow oh sharp draw offset pitch_kind : (the same nine) hwc (the job's members)
//             (R: planar, H: interleaved.)  The test compares the digests of the H lines with tests/golden/dec_hwc_plans_parent.json.
//   existing  for FRAME, PLANAR, SEMI and RGB targets -- every scale, size, out420p, sharp, draw, offset and pitch the older sweeps use --
//             the predicates' answers and every member a DeliveryPlan had before tensors ("P case : members"); for planar tensor targets
//             the same and the tensor job and facts ("T case : members").  The test compares their digests with
//             tests/golden/dec_plans_parent.json and dec_tensor_plans_parent.json.  A plan of such a target holds no interleaved job.
// The three golden files are the record of what the planners of earlier commits planned (their "what" fields name them): the lines
// are printed from today's record -- one RgbOutJob with a layout word -- in the words those planners' records had, and must hash
// equal.
// tests/test_dec_plan_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/dec_plan_check.cpp -o dec_plan_check
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>

#include "dec_delivery.h"

using namespace dsv2;

namespace {

typedef unsigned long long U64;
constexpr U64 kReconAt = 0x10000000ull, kLumaAt = 0x20000000ull, kScaledAt = 0x30000000ull, kTargetAt = 0x40000000ull, kPlaneApart = 0x08000000ull;

[[noreturn]] void fail(const std::string &what, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "FAILED [%s]: ", what.c_str());
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}

int cdiv(int v, int shift) { return (v + (1 << shift) - 1) >> shift; }
U64 at(const void *q) { return (U64) (uintptr_t) q; }

// a bordered frame as frame.c:63-113 lays it out (32-pixel borders, strides rounded up to 16, plane behind plane), restated
DFrame fake_frame(U64 where, int format, int w, int h)
{
    DFrame f;
    f.format = format, f.w = w, f.h = h;
    f.alloc = (uint8_t *) (uintptr_t) where;
    size_t off = 0;
    for (int c = 0; c < 3; c++) {
        const int pw = c ? cdiv(w, DSV_FORMAT_H_SHIFT(format)) : w, ph = c ? cdiv(h, DSV_FORMAT_V_SHIFT(format)) : h;
        const int stride = (pw + 64 + 15) & ~15;
        f.plane_off[c] = off, f.plane_len[c] = (size_t) stride * (size_t) (ph + 64);
        f.p[c] = DPlane{f.alloc + off + (size_t) stride * 32 + 32, stride, pw, ph};
        off += f.plane_len[c];
    }
    f.bytes = off;
    return f;
}

struct Staging { // the decoder's staging areas: the luma w x h, the scaled picture at the planes' own sizes; 16-byte strides
    DFrame recon;
    DPlane luma, scaled[3];
    Staging(int fmt, int w, int h) : recon(fake_frame(kReconAt, fmt, w, h))
    {
        luma = DPlane{(uint8_t *) (uintptr_t) kLumaAt, (w + 15) & ~15, w, h};
        U64 where = kScaledAt;
        for (int k = 0; k < 3; k++) {
            scaled[k] = DPlane{(uint8_t *) (uintptr_t) where, (recon.p[k].w + 15) & ~15, recon.p[k].w, recon.p[k].h};
            where += (U64) scaled[k].stride * (U64) recon.p[k].h;
        }
    }
};

const int kCoef[4][6] = {{298, 16, 409, -100, -208, 516}, {298, 16, 459, -55, -136, 541}, {256, 0, 359, -88, -183, 454}, {256, 0, 403, -48, -120, 475}};
static const DPlane kNone = {nullptr, 0, 0, 0};

// ---- tensor targets, planar and interleaved ---------------------------------------------------------------------------------------------
struct Case {
    int fmt, w, h, dtype;
    bool hwc; // interleaved, else planar
    int bgr, ow, oh; // bgr: interleaved only; ow x oh: 0 x 0 = not sized
    bool sharp;
    int draw, offset, pitch_kind; // offset: elements behind a 256-byte boundary; pitch: tight, + 1 element, rounded up to 256
    std::string name() const
    {
        char s[160];
        snprintf(s, sizeof s, "%s fmt=%#x %dx%d dtype=%d bgr=%d -> %dx%d sharp=%d draw=%d offset=%d pitch=%d", hwc ? "hwc" : "tensor", fmt, w, h, dtype, bgr, ow, oh,
                 (int) sharp, draw, offset, pitch_kind);
        return s;
    }
};

long g_cases[2] = {0, 0}, g_wide[2] = {0, 0}; // planar, interleaved

// the planar tensor of a case, and what target_tensor refuses of it, one spoiled field each
dsv2hip_out_tensor planar_target(const Case &c, size_t rb, size_t pitch, int dh, delivery::OutTarget *t)
{
    using namespace delivery;
    const int elem = tensor_elem(c.dtype);
    dsv2hip_out_tensor tn = {};
    tn.dtype = c.dtype, tn.csc = ((c.w + c.offset) & 1 ? DSV2HIP_CSC_FULL_RANGE : 0) | (c.pitch_kind & 1 ? DSV2HIP_CSC_BT709 : 0);
    tn.out_w = c.ow, tn.out_h = c.oh;
    for (int k = 0; k < 3; k++) {
        tn.plane[k] = (void *) (uintptr_t) (kTargetAt + (U64) k * kPlaneApart + 256 + (U64) c.offset * (U64) elem);
        tn.pitch[k] = pitch, tn.cap[k] = (size_t) (dh - 1) * pitch + rb;
        tn.scale[k] = 0.25f * (float) (k + 1), tn.bias[k] = -1.5f * (float) k;
    }
    if (!target_tensor(tn, rb, dh, t)) {
        fail(c.name(), "target_tensor refused a tensor that holds the rows exactly");
    }
    OutTarget none_t;
    dsv2hip_out_tensor bad = tn;
    bad.cap[2]--;
    bool refused = !target_tensor(bad, rb, dh, &none_t);
    bad = tn, bad.plane[1] = nullptr;
    refused = refused && !target_tensor(bad, rb, dh, &none_t);
    bad = tn, bad.pitch[0] = rb - 1;
    refused = refused && !target_tensor(bad, rb, dh, &none_t);
    bad = tn, bad.pitch[0] = (size_t) INT32_MAX + 1 + (size_t) elem, bad.cap[0] = ~(size_t) 0;
    refused = refused && !target_tensor(bad, rb, dh, &none_t);
    if (elem > 1) {
        bad = tn, bad.plane[0] = (char *) tn.plane[0] + 1, bad.cap[0] += 8;
        refused = refused && !target_tensor(bad, rb, dh, &none_t);
        bad = tn, bad.pitch[1] = pitch + 1, bad.cap[1] = (size_t) dh * (pitch + 1);
        refused = refused && !target_tensor(bad, rb, dh, &none_t);
        bad = tn, bad.scale[2] = std::numeric_limits<float>::infinity();
        refused = refused && !target_tensor(bad, rb, dh, &none_t);
        bad = tn, bad.bias[0] = std::numeric_limits<float>::quiet_NaN();
        refused = refused && !target_tensor(bad, rb, dh, &none_t);
    } else { // uint8: the constants are not looked at
        bad = tn, bad.scale[2] = std::numeric_limits<float>::infinity(), bad.bias[0] = std::numeric_limits<float>::quiet_NaN();
        refused = refused && target_tensor(bad, rb, dh, &none_t);
    }
    if (!refused) {
        fail(c.name(), "target_tensor accepted a spoiled tensor (or refused constants a uint8 tensor ignores)");
    }
    return tn;
}

// the interleaved tensor of a case, and what target_hwc refuses of it, one spoiled field each
dsv2hip_out_hwc hwc_target(const Case &c, size_t rb, size_t pitch, int dh, delivery::OutTarget *t)
{
    using namespace delivery;
    const int elem = tensor_elem(c.dtype);
    dsv2hip_out_hwc hw = {};
    hw.dtype = c.dtype, hw.order = c.bgr ? DSV2HIP_SURFACE_BGR : DSV2HIP_SURFACE_RGB;
    hw.csc = ((c.w + c.offset) & 1 ? DSV2HIP_CSC_FULL_RANGE : 0) | (c.pitch_kind & 1 ? DSV2HIP_CSC_BT709 : 0);
    hw.out_w = c.ow, hw.out_h = c.oh;
    hw.data = (void *) (uintptr_t) (kTargetAt + 256 + (U64) c.offset * (U64) elem);
    hw.pitch = pitch, hw.cap = (size_t) (dh - 1) * pitch + rb;
    for (int k = 0; k < 3; k++) {
        hw.scale[k] = 0.25f * (float) (k + 1), hw.bias[k] = -1.5f * (float) k;
    }
    if (!target_hwc(hw, rb, dh, t)) {
        fail(c.name(), "target_hwc refused a tensor that holds the rows exactly");
    }
    OutTarget none_t;
    dsv2hip_out_hwc bad = hw;
    bad.cap--;
    bool refused = !target_hwc(bad, rb, dh, &none_t);
    bad = hw, bad.data = nullptr;
    refused = refused && !target_hwc(bad, rb, dh, &none_t);
    bad = hw, bad.pitch = rb - 1;
    refused = refused && !target_hwc(bad, rb, dh, &none_t);
    bad = hw, bad.pitch = (size_t) INT32_MAX + 1 + (size_t) elem, bad.cap = ~(size_t) 0;
    refused = refused && !target_hwc(bad, rb, dh, &none_t);
    for (int order : {0, 0x22, 0x10, 0x11, hw.order | DSV2HIP_CSC_BT709, hw.order | DSV2HIP_CSC_FULL_RANGE}) {
        bad = hw, bad.order = order;
        refused = refused && !target_hwc(bad, rb, dh, &none_t);
    }
    if (elem > 1) {
        bad = hw, bad.data = (char *) hw.data + 1, bad.cap += 8;
        refused = refused && !target_hwc(bad, rb, dh, &none_t);
        bad = hw, bad.pitch = pitch + 1, bad.cap = (size_t) dh * (pitch + 1);
        refused = refused && !target_hwc(bad, rb, dh, &none_t);
        bad = hw, bad.scale[2] = std::numeric_limits<float>::infinity();
        refused = refused && !target_hwc(bad, rb, dh, &none_t);
        bad = hw, bad.bias[0] = std::numeric_limits<float>::quiet_NaN();
        refused = refused && !target_hwc(bad, rb, dh, &none_t);
        bad = hw, bad.scale[1] = -std::numeric_limits<float>::infinity();
        refused = refused && !target_hwc(bad, rb, dh, &none_t);
    } else { // uint8: the constants are not looked at
        bad = hw, bad.scale[2] = std::numeric_limits<float>::infinity(), bad.bias[0] = std::numeric_limits<float>::quiet_NaN();
        refused = refused && target_hwc(bad, rb, dh, &none_t);
    }
    if (!refused) {
        fail(c.name(), "target_hwc accepted a spoiled tensor (or refused constants a uint8 tensor ignores)");
    }
    return hw;
}

void check_tensor(const Case &c)
{
    using namespace delivery;
    const Staging S(c.fmt, c.w, c.h);
    const int elem = tensor_elem(c.dtype), dw = c.ow ? c.ow : c.w, dh = c.oh ? c.oh : c.h;
    const size_t rb = (c.hwc ? 3 : 1) * (size_t) dw * (size_t) elem;
    const size_t pitch = c.pitch_kind == 0 ? rb : c.pitch_kind == 1 ? rb + (size_t) elem : (rb + 255) / 256 * 256;
    OutTarget t;
    // what the job must hold: the target's planes (interleaved: one), its order and its constants
    uint8_t *dst[3] = {nullptr, nullptr, nullptr};
    float scale[3], bias[3];
    int csc;
    if (c.hwc) {
        const dsv2hip_out_hwc hw = hwc_target(c, rb, pitch, dh, &t);
        dst[0] = (uint8_t *) hw.data, csc = hw.csc;
        memcpy(scale, hw.scale, sizeof scale), memcpy(bias, hw.bias, sizeof bias);
    } else {
        const dsv2hip_out_tensor tn = planar_target(c, rb, pitch, dh, &t);
        for (int k = 0; k < 3; k++) {
            dst[k] = (uint8_t *) tn.plane[k];
        }
        csc = tn.csc;
        memcpy(scale, tn.scale, sizeof scale), memcpy(bias, tn.bias, sizeof bias);
    }
    t.ow = c.ow, t.oh = c.oh;
    const bool sized = c.ow != 0, staged_luma = c.sharp || c.draw;
    if (!t.converted() || t.sized() != sized || needs_staged_luma(t, c.sharp, c.draw) != staged_luma || needs_staged_scaled(t) != sized ||
        needs_staged_full(t) != sized) {
        fail(c.name(), "the staging predicates disagree with the rules");
    }
    const DeliveryPlan p = plan_delivery(S.recon, c.fmt, t, c.sharp, c.draw, staged_luma ? S.luma : kNone, sized ? S.scaled : nullptr);
    g_cases[c.hwc]++;
    if (p.n_copy || p.n_to420 || p.n_scl || p.n_uv || p.n_rgb != 1 || p.n_rsz != (sized ? 3 : 0) || p.n_eg != (int) staged_luma || p.n_overlay != (int) (c.draw != 0) ||
        p.sharpen_overlaid != (c.draw && c.sharp)) {
        fail(c.name(), "jobs copy %d to420 %d egress %d scale %d resize %d uv %d rgb %d overlay %d sharpen %d", p.n_copy, p.n_to420, p.n_eg, p.n_scl, p.n_rsz, p.n_uv,
             p.n_rgb, p.n_overlay, (int) p.sharpen_overlaid);
    }
    if (staged_luma) {
        const EgressJob &e = p.eg[0];
        if (e.src.data != S.recon.p[0].data || e.src.w != c.w || e.src.h != c.h || e.dst != S.luma.data || e.dstride != S.luma.stride ||
            (e.sharp != 0) != (c.sharp && !c.draw)) {
            fail(c.name(), "the egress job does not stage the luma");
        }
    }
    if (c.draw && (p.overlay[0].data != S.luma.data || p.overlay[0].stride != S.luma.stride || p.overlay[0].w != c.w || p.overlay[0].h != c.h)) {
        fail(c.name(), "the overlay is not on the staged luma");
    }
    const int hs = DSV_FORMAT_H_SHIFT(c.fmt), vs = DSV_FORMAT_V_SHIFT(c.fmt);
    DPlane src[3];
    for (int k = 0; k < 3; k++) {
        src[k] = (k == 0 && staged_luma) ? S.luma : S.recon.p[k];
        if (sized) {
            const ResizeOutJob &j = p.rsz[k];
            const int sw = k ? cdiv(c.ow, hs) : c.ow, sh = k ? cdiv(c.oh, vs) : c.oh;
            if (j.src != src[k].data || j.sstride != src[k].stride || j.pw != S.recon.p[k].w || j.ph != S.recon.p[k].h || j.ow != sw || j.oh != sh ||
                j.dst != S.scaled[k].data || j.dpitch != S.scaled[k].stride || sw > S.scaled[k].stride || sh > S.scaled[k].h) {
                fail(c.name(), "resampling job %d does not stage plane %d at %dx%d", k, k, sw, sh);
            }
            src[k] = DPlane{S.scaled[k].data, S.scaled[k].stride, sw, sh};
        }
    }
    const RgbOutJob &j = p.rgb[0];
    const int *co = kCoef[((csc & DSV2HIP_CSC_FULL_RANGE) ? 2 : 0) + ((csc & DSV2HIP_CSC_BT709) ? 1 : 0)];
    bool ok = j.layout == (c.hwc ? kRgbOutInterleaved : kRgbOutPlanar) && j.sy == src[0].data && j.su == src[1].data && j.sv == src[2].data &&
              j.ystride == src[0].stride && j.cstride == src[1].stride && j.w == dw && j.h == dh && j.hs == hs && j.vs == vs && j.dtype == c.dtype &&
              (j.bgra != 0) == (c.hwc && c.bgr) && j.csc.ky == co[0] && j.csc.ybase == co[1] && j.csc.rv == co[2] && j.csc.gu == co[3] && j.csc.gv == co[4] &&
              j.csc.bu == co[5];
    for (int k = 0; k < 3; k++) {
        ok = ok && j.dst[k] == dst[k] && (size_t) j.dpitch[k] == (dst[k] ? pitch : 0);
        ok = ok && (elem == 1 || (j.scale[k] == scale[k] && j.bias[k] == bias[k]));
    }
    if (!ok) {
        fail(c.name(), "the conversion job does not read what was staged, or does not write the tensor's rows with its layout, order and constants");
    }
    const bool wide = ((kTargetAt + 256 + (U64) c.offset * (U64) elem) | (U64) pitch) % (U64) (4 * elem) == 0 && dw % 4 == 0; // (kPlaneApart: a multiple of 16)
    if (p.rgb_wide != wide || rgb_out_job_wide(j) != wide) {
        fail(c.name(), "rgb_wide is %d, the rule says %d", (int) p.rgb_wide, (int) wide);
    }
    g_wide[c.hwc] += wide;
    if (c.hwc) {
        printf("H %d %d %d %d %d %d %d %d %d %d %d :", c.fmt, c.w, c.h, c.dtype, c.bgr, c.ow, c.oh, (int) c.sharp, c.draw, c.offset, c.pitch_kind);
    } else {
        printf("R %d %d %d %d %d %d %d %d %d %d :", c.fmt, c.w, c.h, c.dtype, c.ow, c.oh, (int) c.sharp, c.draw, c.offset, c.pitch_kind);
    }
    printf(" %d %d %d %d %d %d %d %d %d", p.n_eg, p.n_rsz, p.n_rgb, p.n_overlay, (int) p.sharpen_overlaid, (int) p.rgb_wide, (int) needs_staged_luma(t, c.sharp, c.draw),
           (int) needs_staged_scaled(t), (int) needs_staged_full(t));
    if (c.hwc) { // the job's members, in the order of the interleaved tensor's own record before the layouts shared one
        printf(" hwc %llx %llx %llx %llx %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", at(j.sy), at(j.su), at(j.sv), at(j.dst[0]), j.ystride, j.cstride, j.dpitch[0], j.w,
               j.h, j.hs, j.vs, j.csc.ky, j.csc.ybase, j.csc.rv, j.csc.gu, j.csc.gv, j.csc.bu, j.bgra, j.dtype);
        for (int k = 0; k < 3; k++) {
            printf(" %a %a", (double) j.scale[k], (double) j.bias[k]);
        }
    }
    printf("\n");
}

// ---- the targets of the older sweeps --------------------------------------------------------------------------------------------------------
long g_existing = 0, g_tensor = 0;
struct Old { // a target of a kind that existed before the interleaved tensor
    int fmt, w, h, kind, shift, ow, oh; // kind: 0 FRAME, 1 PLANAR, 2 SEMI, 3 RGB, 4 TENSOR (shift: the element type)
    bool out420p, sharp;
    int draw, offset, pitch_kind;
    std::string name() const
    {
        char s[200];
        snprintf(s, sizeof s, "parent fmt=%#x %dx%d kind=%d shift=%d -> %dx%d out420p=%d sharp=%d draw=%d offset=%d pitch=%d", fmt, w, h, kind, shift, ow, oh, (int) out420p,
                 (int) sharp, draw, offset, pitch_kind);
        return s;
    }
};

delivery::OutTarget make_target(const Old &c)
{
    using namespace delivery;
    if (c.kind == 4) {
        const Case tc{c.fmt, c.w, c.h, c.shift, false, 0, c.ow, c.oh, c.sharp, c.draw, c.offset, c.pitch_kind};
        const int elem = tensor_elem(c.shift), dh = c.oh ? c.oh : c.h;
        const size_t rb = (size_t) (c.ow ? c.ow : c.w) * (size_t) elem;
        const size_t pitch = c.pitch_kind == 0 ? rb : c.pitch_kind == 1 ? rb + (size_t) elem : (rb + 255) / 256 * 256;
        OutTarget t;
        planar_target(tc, rb, pitch, dh, &t);
        t.ow = c.ow, t.oh = c.oh;
        return t;
    }
    const int out_format = c.out420p ? DSV_SUBSAMP_420 : c.fmt;
    if (c.kind == 0) {
        const DFrame fr = fake_frame(kTargetAt, out_format, c.w, c.h);
        DSV_FRAME f = {};
        f.alloc = fr.alloc;
        for (int k = 0; k < 3; k++) {
            f.planes[k].data = fr.p[k].data, f.planes[k].stride = fr.p[k].stride, f.planes[k].w = fr.p[k].w, f.planes[k].h = fr.p[k].h;
        }
        return target_frame(&f);
    }
    const int rw = c.ow ? c.ow : cdiv(c.w, c.shift), rh = c.oh ? c.oh : cdiv(c.h, c.shift);
    const int cw = cdiv(rw, DSV_FORMAT_H_SHIFT(out_format)), ch = cdiv(rh, DSV_FORMAT_V_SHIFT(out_format));
    size_t rb[3] = {(size_t) rw, (size_t) cw, (size_t) cw};
    int rows[3] = {rh, ch, ch}, nplanes = 3;
    if (c.kind == 2) {
        rb[1] = 2 * (size_t) cw, rb[2] = 0, rows[2] = 0, nplanes = 2;
    } else if (c.kind == 3) {
        rb[0] = 4 * (size_t) rw, rb[1] = rb[2] = 0, rows[1] = rows[2] = 0, nplanes = 1;
    }
    dsv2hip_out_surface sf = {};
    const int base = c.kind == 1 ? DSV2HIP_SURFACE_PLANAR : c.kind == 2 ? DSV2HIP_SURFACE_SEMIPLANAR
                   : (c.w + c.offset) & 1 ? (DSV2HIP_SURFACE_RGBA | DSV2HIP_CSC_FULL_RANGE) : (DSV2HIP_SURFACE_BGRA | DSV2HIP_CSC_BT709);
    sf.layout = base | (c.shift << 12);
    for (int k = 0; k < nplanes; k++) {
        const size_t pitch = c.pitch_kind == 0 ? rb[k] : c.pitch_kind == 1 ? rb[k] + 1 : (rb[k] + 255) / 256 * 256;
        sf.plane[k] = (void *) (uintptr_t) (kTargetAt + (U64) k * kPlaneApart + 256 + (U64) c.offset);
        sf.pitch[k] = pitch, sf.cap[k] = (size_t) (rows[k] - 1) * pitch + rb[k];
    }
    OutTarget t;
    if (!target_surface(sf, rb, rows, &t)) {
        fail(c.name(), "target_surface refused a surface that holds the picture exactly");
    }
    t.ow = c.ow, t.oh = c.oh;
    return t;
}

// the predicates' answers and the members a DeliveryPlan had before tensors, as text (addresses are the synthetic ones) -- "P" lines;
// a TENSOR target's "T" line adds its tensor job and facts.  The words of the records of that time: the RGB surface's job and wide flag
// (n_rgb, rgb_wide) are the packed layout's, the tensor's (n_ten, ten_wide) the planar layout's
void print_plan(const Old &c, const delivery::DeliveryPlan &p, bool luma, bool scaled, bool full)
{
    const int layout = p.n_rgb ? p.rgb[0].layout : -1;
    const int n_packed = layout == kRgbOutPacked ? p.n_rgb : 0, n_planar = layout == kRgbOutPlanar ? p.n_rgb : 0;
    printf("%c %d %d %d %d %d %d %d %d %d %d %d %d :", c.kind == 4 ? 'T' : 'P', c.fmt, c.w, c.h, c.kind, c.shift, c.ow, c.oh, (int) c.out420p, (int) c.sharp, c.draw,
           c.offset, c.pitch_kind);
    printf(" %d%d%d n %d %d %d %d %d %d %d %d f %d %d %d %d %d %d %d %d %d %d %d %d", (int) luma, (int) scaled, (int) full, p.n_copy, p.n_to420, p.n_eg, p.n_scl, p.n_rsz, p.n_uv,
           n_packed, p.n_overlay, (int) p.sharpen_overlaid, (int) p.eg_wide, (int) p.eg_sharp, (int) p.scl_wide, p.scl_rows, (int) p.rsz_wide, p.rsz_rows, p.rsz_cols,
           (int) p.uv_wide, (int) p.uv_conv, p.uv_rows, (int) (n_packed ? p.rgb_wide : true));
    for (int i = 0; i < p.n_copy; i++) {
        printf(" copy %llx %llx %zu", at(p.copy[i].src), at(p.copy[i].dst), p.copy[i].bytes);
    }
    for (int i = 0; i < p.n_to420; i++) {
        const To420Job &j = p.to420[i];
        printf(" to420 %llx %d %d %d %llx %d %d %d %d", at(j.src.data), j.src.stride, j.src.w, j.src.h, at(j.dst.data), j.dst.stride, j.dst.w, j.dst.h, j.mode);
    }
    for (int i = 0; i < p.n_eg; i++) {
        const EgressJob &j = p.eg[i];
        printf(" eg %llx %d %d %d %llx %d %d", at(j.src.data), j.src.stride, j.src.w, j.src.h, at(j.dst), j.dstride, j.sharp);
    }
    for (int i = 0; i < p.n_scl; i++) {
        const ScaleOutJob &j = p.scl[i];
        printf(" scl %llx %llx %d %d %d %d %d", at(j.src), at(j.dst), j.sstride, j.pw, j.ph, j.dpitch, j.shift);
    }
    for (int i = 0; i < p.n_rsz; i++) {
        const ResizeOutJob &j = p.rsz[i];
        printf(" rsz %llx %llx %d %d %d %d %d %d %d %d %d %d %u %u %u %u", at(j.src), at(j.dst), j.sstride, j.dpitch, j.pw, j.ph, j.ow, j.oh, j.a, j.b, j.c, j.d, j.D, j.rD, j.rb, j.rd);
    }
    for (int i = 0; i < p.n_uv; i++) {
        const UvEgressJob &j = p.uv[i];
        printf(" uv %llx %llx %llx %d %d %d %d %d %d %d", at(j.su), at(j.sv), at(j.dst), j.dpitch, j.sstride, j.sw, j.sh, j.cw, j.ch, j.mode);
    }
    for (int i = 0; i < n_packed; i++) {
        const RgbOutJob &j = p.rgb[i];
        printf(" rgb %llx %llx %llx %llx %d %d %d %d %d %d %d %d %d %d %d %d %d %d", at(j.sy), at(j.su), at(j.sv), at(j.dst[0]), j.ystride, j.cstride, j.dpitch[0], j.w, j.h, j.hs,
               j.vs, j.csc.ky, j.csc.ybase, j.csc.rv, j.csc.gu, j.csc.gv, j.csc.bu, j.bgra);
    }
    for (int i = 0; i < p.n_overlay; i++) {
        printf(" ov %llx %d %d %d", at(p.overlay[i].data), p.overlay[i].stride, p.overlay[i].w, p.overlay[i].h);
    }
    if (c.kind == 4) {
        printf(" ten %d %d", n_planar, (int) (n_planar ? p.rgb_wide : true));
        for (int i = 0; i < n_planar; i++) {
            const RgbOutJob &j = p.rgb[i];
            printf(" %llx %llx %llx %d %d %d %d %d %d %d %d %d %d %d %d %d", at(j.sy), at(j.su), at(j.sv), j.ystride, j.cstride, j.w, j.h, j.hs, j.vs, j.csc.ky, j.csc.ybase,
                   j.csc.rv, j.csc.gu, j.csc.gv, j.csc.bu, j.dtype);
            for (int k = 0; k < 3; k++) {
                printf(" %llx %d %a %a", at(j.dst[k]), j.dpitch[k], (double) j.scale[k], (double) j.bias[k]);
            }
        }
    }
    printf("\n");
}

void check_existing(const Old &c)
{
    using namespace delivery;
    const Staging S(c.fmt, c.w, c.h);
    Staging H(c.fmt, c.w, c.h); // (a target with a shift alone: the scaled picture is laid out for half size, as the older sweep has it)
    if (c.shift && c.kind != 4) {
        U64 where = kScaledAt;
        for (int k = 0; k < 3; k++) {
            const int sw = (S.recon.p[k].w + 1) >> 1, sh = (S.recon.p[k].h + 1) >> 1;
            H.scaled[k] = DPlane{(uint8_t *) (uintptr_t) where, (sw + 15) & ~15, sw, sh};
            where += (U64) H.scaled[k].stride * (U64) sh;
        }
    }
    const OutTarget t = make_target(c);
    const bool luma = needs_staged_luma(t, c.sharp, c.draw), scaled = needs_staged_scaled(t), full = needs_staged_full(t);
    if (t.converted() != (c.kind >= 3)) {
        fail(c.name(), "converted() is wrong");
    }
    const int out_format = c.out420p ? DSV_SUBSAMP_420 : c.fmt;
    const DeliveryPlan p = plan_delivery(S.recon, out_format, t, c.sharp, c.draw, luma ? S.luma : kNone, scaled ? H.scaled : nullptr);
    (c.kind == 4 ? g_tensor : g_existing)++;
    const int want = c.kind == 3 ? kRgbOutPacked : c.kind == 4 ? kRgbOutPlanar : -1; // (the others: no conversion job)
    if (p.n_rgb != (want >= 0) || (p.n_rgb && p.rgb[0].layout != want) || (!p.n_rgb && !p.rgb_wide)) {
        fail(c.name(), "the conversion job or fact is not of the target's layout");
    }
    print_plan(c, p, luma, scaled, full);
}

} // namespace

int main()
{
    static const int formats[] = {DSV_SUBSAMP_444, DSV_SUBSAMP_422, DSV_SUBSAMP_420, DSV_SUBSAMP_411, DSV_SUBSAMP_410};
    static const int sizes[][2] = {{16, 16}, {34, 18}, {64, 48}, {352, 288}, {1919, 1079}};
    static const int offsets[] = {0, 1, 2, 4};
    for (int fmt : formats) {
        for (const int *wh : sizes) {
            const int w = wh[0], h = wh[1];
            const int outs[][2] = {{0, 0}, {(w + 1) / 2, (h + 1) / 2}, {(3 * w / 4) & ~3, (3 * h / 4) & ~3}, {w - 1, h}};
            for (int dtype = 0; dtype < 4; dtype++) {
                for (const int *o : outs) {
                    for (int sd = 0; sd < 4; sd++) {
                        const bool sharp = (sd & 1) != 0;
                        const int draw = (sd & 2) ? 7 : 0;
                        for (int offset : offsets) {
                            for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                                check_tensor(Case{fmt, w, h, dtype, false, 0, o[0], o[1], sharp, draw, offset, pitch_kind});
                                for (int bgr = 0; bgr < 2; bgr++) {
                                    check_tensor(Case{fmt, w, h, dtype, true, bgr, o[0], o[1], sharp, draw, offset, pitch_kind});
                                }
                                check_existing(Old{fmt, w, h, 4, dtype, o[0], o[1], false, sharp, draw, offset, pitch_kind});
                            }
                        }
                    }
                }
            }
            const int old_outs[][2] = {{0, 0}, {(2 * w + 2) / 3, (2 * h + 2) / 3}, {(w + 7) / 8, (h + 7) / 8}, {w, h - 1}};
            for (int kind = 0; kind <= 3; kind++) {
                for (int shift = 0; shift <= (kind == 0 ? 0 : 3); shift++) {
                    for (const int *o : old_outs) {
                        if (o[0] && (kind == 0 || shift)) { // (a size: device targets without a scale value)
                            continue;
                        }
                        for (int out420p = 0; out420p <= (shift || o[0] || kind == 3 ? 0 : 1); out420p++) { // (the surface calls refuse the pairs)
                            for (int sd = 0; sd < 4; sd++) {
                                for (int offset : {0, 1, 16}) {
                                    for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                                        check_existing(Old{fmt, w, h, kind, shift, o[0], o[1], out420p != 0, (sd & 1) != 0, (sd & 2) ? 7 : 0, offset, pitch_kind});
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    for (int l = 0; l < 2; l++) {
        if (g_wide[l] == 0 || g_wide[l] == g_cases[l]) {
            fprintf(stderr, "FAILED: the sweep holds only one form of the %s conversion\n", l ? "interleaved" : "planar");
            return 1;
        }
    }
    printf("dec_plan_check: %ld planar tensor cases (%ld in the wide form) and %ld interleaved (%ld): target, staging, jobs and form hold; %ld plans of the "
           "other targets and %ld of tensor targets printed\n",
           g_cases[0], g_wide[0], g_cases[1], g_wide[1], g_existing, g_tensor);
    return 0;
}
