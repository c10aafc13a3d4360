// dec_hwc_plan_check.cpp -- the decoder's delivery planner (csrc/dec_delivery.h) swept on the CPU for HWC targets
// (dsv2hip_dec_batch_hwc): chroma format x picture size x element type x order x sized or not x postsharp x draw_info x pointer offset x
// pitch, over FAKE addresses as tools/dec_tensor_plan_check.cpp does -- the reconstruction, the two staging areas and the target are
// disjoint ranges of one synthetic address space, and nothing is ever dereferenced.  Meant to be built with AddressSanitizer and
// UndefinedBehaviorSanitizer (the planner is handed no staging area it says it does not need: a look at one faults).
//   hwc       target_hwc takes a tensor that holds the rows exactly and refuses one a byte short, a pitch or a pointer off the element
//             grid, a pitch below the row or beyond an int, an order that is not exactly RGB or BGR, and a constant that is not finite
//             (uint8: the constants are not looked at); the predicates ask for the staged luma exactly for a sharpened or drawn-on
//             picture and for the staged (full-size) scaled picture exactly for a sized one; the plan holds one HWC job behind the luma's
//             egress job and the three resampling jobs, reading what they staged, writing the tensor's rows, with the preset's
//             coefficients, the element type, the order and the constants; hwc_wide is hwc_job_wide of the job.  One line per case goes
//             to stdout for tests/test_dec_hwc_plan_cpu.py to compare with its own restatement of the rules:
//               H fmt w h dtype bgr ow oh sharp draw offset pitch_kind : n_eg n_rsz n_hwc n_overlay sharpen_overlaid wide luma scaled full
//   existing  for FRAME, PLANAR, SEMI and RGB targets -- the sweep of tools/dec_tensor_plan_check.cpp -- the predicates' answers and
//             every member a DeliveryPlan had before tensors go to stdout as that tool prints them ("P case : members"); the test
//             compares their digests with tests/golden/dec_plans_parent.json.  For TENSOR targets -- that tool's tensor sweep -- the
//             same and the tensor job and facts ("T case : members"); the test compares their digests with
//             tests/golden/dec_tensor_plans_parent.json.  A plan of such a target holds no HWC job or fact.
//   parent    how tests/golden/dec_tensor_plans_parent.json was recorded, and a check of its own: with -DPARENT_HEADER="file" (the text
//             of the parent commit's dec_delivery.h, the last one without HWC targets -- git show PARENT:digital-subband-video-2_amd/
//             csrc/dec_delivery.h -- with `namespace delivery {` replaced by `namespace delivery_parent { using namespace delivery;`,
//             in a directory of its own) both planners run side by side in this one program, every member and predicate of the P and
//             T cases compares equal, and the lines printed are the PARENT planner's; the golden file holds sha256 over the T lines
//             per chroma format and picture size ("fmt WxH"), as dec_plans_parent.json does over the P lines.
// tests/test_dec_hwc_plan_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/dec_hwc_plan_check.cpp -o dec_hwc_plan_check
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>

#include "dec_delivery.h"
#ifdef PARENT_HEADER
#include PARENT_HEADER
#endif

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

// a bordered frame as frame.c:63-113 lays it out (32-pixel borders, strides rounded up to 16, plane behind plane), restated
DFrame fake_frame(U64 at, int format, int w, int h)
{
    DFrame f;
    f.format = format, f.w = w, f.h = h;
    f.alloc = (uint8_t *) (uintptr_t) at;
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
        U64 at = kScaledAt;
        for (int k = 0; k < 3; k++) {
            scaled[k] = DPlane{(uint8_t *) (uintptr_t) at, (recon.p[k].w + 15) & ~15, recon.p[k].w, recon.p[k].h};
            at += (U64) scaled[k].stride * (U64) recon.p[k].h;
        }
    }
};

const int kCoef[4][6] = {{298, 16, 409, -100, -208, 516}, {298, 16, 459, -55, -136, 541}, {256, 0, 359, -88, -183, 454}, {256, 0, 403, -48, -120, 475}};
static const DPlane kNone = {nullptr, 0, 0, 0};

// ---- HWC targets ------------------------------------------------------------------------------------------------------------------------
struct Case {
    int fmt, w, h, dtype, bgr, ow, oh; // ow x oh: 0 x 0 = not sized
    bool sharp;
    int draw, offset, pitch_kind; // offset: elements behind a 256-byte boundary; pitch: tight, + 1 element, rounded up to 256
    std::string name() const
    {
        char s[160];
        snprintf(s, sizeof s, "hwc fmt=%#x %dx%d dtype=%d bgr=%d -> %dx%d sharp=%d draw=%d offset=%d pitch=%d", fmt, w, h, dtype, bgr, ow, oh, (int) sharp, draw, offset,
                 pitch_kind);
        return s;
    }
};

long g_hwc = 0, g_wide = 0;

void check_hwc(const Case &c)
{
    using namespace delivery;
    const Staging S(c.fmt, c.w, c.h);
    const int elem = tensor_elem(c.dtype), dw = c.ow ? c.ow : c.w, dh = c.oh ? c.oh : c.h;
    const size_t rb = 3 * (size_t) dw * (size_t) elem;
    const size_t pitch = c.pitch_kind == 0 ? rb : c.pitch_kind == 1 ? rb + (size_t) elem : (rb + 255) / 256 * 256;
    dsv2hip_out_hwc hw = {};
    hw.dtype = c.dtype, hw.order = c.bgr ? DSV2HIP_SURFACE_BGR : DSV2HIP_SURFACE_RGB;
    hw.csc = ((c.w + c.offset) & 1 ? DSV2HIP_CSC_FULL_RANGE : 0) | (c.pitch_kind & 1 ? DSV2HIP_CSC_BT709 : 0);
    hw.out_w = c.ow, hw.out_h = c.oh;
    hw.data = (void *) (uintptr_t) (kTargetAt + 256 + (U64) c.offset * (U64) elem);
    hw.pitch = pitch, hw.cap = (size_t) (dh - 1) * pitch + rb;
    for (int k = 0; k < 3; k++) {
        hw.scale[k] = 0.25f * (float) (k + 1), hw.bias[k] = -1.5f * (float) k;
    }
    OutTarget t, none_t;
    if (!target_hwc(hw, rb, dh, &t)) {
        fail(c.name(), "target_hwc refused a tensor that holds the rows exactly");
    }
    // what target_hwc refuses, one spoiled field each
    {
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
    }
    t.ow = c.ow, t.oh = c.oh;
    const bool sized = c.ow != 0, staged_luma = c.sharp || c.draw;
    if (!t.converted() || t.sized() != sized || needs_staged_luma(t, c.sharp, c.draw) != staged_luma || needs_staged_scaled(t) != sized ||
        needs_staged_full(t) != sized) {
        fail(c.name(), "the staging predicates disagree with the rules");
    }
    const DeliveryPlan p = plan_delivery(S.recon, c.fmt, t, c.sharp, c.draw, staged_luma ? S.luma : kNone, sized ? S.scaled : nullptr);
    g_hwc++;
    if (p.n_copy || p.n_to420 || p.n_scl || p.n_uv || p.n_rgb || p.n_ten || p.n_hwc != 1 || p.n_rsz != (sized ? 3 : 0) || p.n_eg != (int) staged_luma ||
        p.n_overlay != (int) (c.draw != 0) || p.sharpen_overlaid != (c.draw && c.sharp)) {
        fail(c.name(), "jobs copy %d to420 %d egress %d scale %d resize %d uv %d rgb %d tensor %d hwc %d overlay %d sharpen %d", p.n_copy, p.n_to420, p.n_eg,
             p.n_scl, p.n_rsz, p.n_uv, p.n_rgb, p.n_ten, p.n_hwc, p.n_overlay, (int) p.sharpen_overlaid);
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
    const HwcOutJob &j = p.hwc[0];
    const int *co = kCoef[((hw.csc & DSV2HIP_CSC_FULL_RANGE) ? 2 : 0) + ((hw.csc & DSV2HIP_CSC_BT709) ? 1 : 0)];
    bool ok = j.sy == src[0].data && j.su == src[1].data && j.sv == src[2].data && j.ystride == src[0].stride && j.cstride == src[1].stride && j.w == dw && j.h == dh &&
              j.hs == hs && j.vs == vs && j.dtype == c.dtype && (j.bgra != 0) == (c.bgr != 0) && j.csc.ky == co[0] && j.csc.ybase == co[1] && j.csc.rv == co[2] &&
              j.csc.gu == co[3] && j.csc.gv == co[4] && j.csc.bu == co[5] && j.dst == hw.data && (size_t) j.dpitch == pitch;
    for (int k = 0; k < 3; k++) {
        ok = ok && (elem == 1 || (j.scale[k] == hw.scale[k] && j.bias[k] == hw.bias[k]));
    }
    if (!ok) {
        fail(c.name(), "the HWC job does not read what was staged, or does not write the tensor's rows with its order and constants");
    }
    const bool wide = ((kTargetAt + 256 + (U64) c.offset * (U64) elem) | (U64) pitch) % (U64) (4 * elem) == 0 && dw % 4 == 0;
    if (p.hwc_wide != wide || hwc_job_wide(j) != wide || !p.ten_wide || !p.rgb_wide) {
        fail(c.name(), "hwc_wide is %d, the rule says %d", (int) p.hwc_wide, (int) wide);
    }
    g_wide += wide;
    printf("H %d %d %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d %d %d %d\n", c.fmt, c.w, c.h, c.dtype, c.bgr, c.ow, c.oh, (int) c.sharp, c.draw, c.offset, c.pitch_kind,
           p.n_eg, p.n_rsz, p.n_hwc, p.n_overlay, (int) p.sharpen_overlaid, (int) p.hwc_wide, (int) needs_staged_luma(t, c.sharp, c.draw), (int) needs_staged_scaled(t),
           (int) needs_staged_full(t));
}

// ---- the targets that existed before: both planners side by side --------------------------------------------------------------------------
long g_existing = 0, g_tensor = 0;
struct Old { // a target of a kind that existed before
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

// the target in one planner's terms: its OutTarget made by its own target_frame / target_surface / target_tensor (tools/
// dec_tensor_plan_check.cpp's targets, the same synthetic addresses)
template <class Target, class MakeFrame, class MakeSurface, class MakeTensor>
Target make_target(const Old &c, MakeFrame target_frame, MakeSurface target_surface, MakeTensor target_tensor)
{
    if (c.kind == 4) {
        const int dtype = c.shift, elem = tensor_elem(dtype), dw = c.ow ? c.ow : c.w, dh = c.oh ? c.oh : c.h;
        const size_t rb = (size_t) dw * (size_t) elem;
        const size_t pitch = c.pitch_kind == 0 ? rb : c.pitch_kind == 1 ? rb + (size_t) elem : (rb + 255) / 256 * 256;
        dsv2hip_out_tensor tn = {};
        tn.dtype = dtype, tn.csc = ((c.w + c.offset) & 1 ? DSV2HIP_CSC_FULL_RANGE : 0) | (c.pitch_kind & 1 ? DSV2HIP_CSC_BT709 : 0);
        tn.out_w = c.ow, tn.out_h = c.oh;
        for (int k = 0; k < 3; k++) {
            tn.plane[k] = (void *) (uintptr_t) (kTargetAt + (U64) k * kPlaneApart + 256 + (U64) c.offset * (U64) elem);
            tn.pitch[k] = pitch, tn.cap[k] = (size_t) (dh - 1) * pitch + rb;
            tn.scale[k] = 0.25f * (float) (k + 1), tn.bias[k] = -1.5f * (float) k;
        }
        Target t;
        if (!target_tensor(tn, rb, dh, &t)) {
            fail(c.name(), "target_tensor refused a tensor that holds the rows exactly");
        }
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
    Target t;
    if (!target_surface(sf, rb, rows, &t)) {
        fail(c.name(), "target_surface refused a surface that holds the picture exactly");
    }
    t.ow = c.ow, t.oh = c.oh;
    return t;
}

// the predicates' answers and the members a DeliveryPlan had before tensors, as text (addresses are the synthetic ones) -- "P" lines
// exactly as tools/dec_tensor_plan_check.cpp prints them; a TENSOR target's "T" line adds its tensor job and facts
template <class Plan> void print_plan(const Old &c, const Plan &p, bool luma, bool scaled, bool full)
{
    printf("%c %d %d %d %d %d %d %d %d %d %d %d %d :", c.kind == 4 ? 'T' : 'P', c.fmt, c.w, c.h, c.kind, c.shift, c.ow, c.oh, (int) c.out420p, (int) c.sharp, c.draw,
           c.offset, c.pitch_kind);
    printf(" %d%d%d n %d %d %d %d %d %d %d %d f %d %d %d %d %d %d %d %d %d %d %d %d", (int) luma, (int) scaled, (int) full, p.n_copy, p.n_to420, p.n_eg, p.n_scl, p.n_rsz, p.n_uv,
           p.n_rgb, p.n_overlay, (int) p.sharpen_overlaid, (int) p.eg_wide, (int) p.eg_sharp, (int) p.scl_wide, p.scl_rows, (int) p.rsz_wide, p.rsz_rows, p.rsz_cols,
           (int) p.uv_wide, (int) p.uv_conv, p.uv_rows, (int) p.rgb_wide);
    auto at = [](const void *q) { return (U64) (uintptr_t) q; };
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
    for (int i = 0; i < p.n_rgb; i++) {
        const RgbOutJob &j = p.rgb[i];
        printf(" rgb %llx %llx %llx %llx %d %d %d %d %d %d %d %d %d %d %d %d %d %d", at(j.sy), at(j.su), at(j.sv), at(j.dst), j.ystride, j.cstride, j.dpitch, j.w, j.h, j.hs, j.vs, j.csc.ky,
               j.csc.ybase, j.csc.rv, j.csc.gu, j.csc.gv, j.csc.bu, j.bgra);
    }
    for (int i = 0; i < p.n_overlay; i++) {
        printf(" ov %llx %d %d %d", at(p.overlay[i].data), p.overlay[i].stride, p.overlay[i].w, p.overlay[i].h);
    }
    if (c.kind == 4) {
        printf(" ten %d %d", p.n_ten, (int) p.ten_wide);
        for (int i = 0; i < p.n_ten; i++) {
            const TensorOutJob &j = p.ten[i];
            printf(" %llx %llx %llx %d %d %d %d %d %d %d %d %d %d %d %d %d", at(j.sy), at(j.su), at(j.sv), j.ystride, j.cstride, j.w, j.h, j.hs, j.vs, j.csc.ky, j.csc.ybase,
                   j.csc.rv, j.csc.gu, j.csc.gv, j.csc.bu, j.dtype);
            for (int k = 0; k < 3; k++) {
                printf(" %llx %d %a %a", at(j.dst[k]), j.dpitch[k], (double) j.scale[k], (double) j.bias[k]);
            }
        }
    }
    printf("\n");
}

#ifdef PARENT_HEADER
bool same(const DPlane &a, const DPlane &b) { return a.data == b.data && a.stride == b.stride && a.w == b.w && a.h == b.h; }
bool same(const CopyJob &a, const CopyJob &b) { return a.src == b.src && a.dst == b.dst && a.bytes == b.bytes; }
bool same(const To420Job &a, const To420Job &b) { return same(a.src, b.src) && same(a.dst, b.dst) && a.mode == b.mode; }
bool same(const EgressJob &a, const EgressJob &b) { return same(a.src, b.src) && a.dst == b.dst && a.dstride == b.dstride && a.sharp == b.sharp; }
bool same(const ScaleOutJob &a, const ScaleOutJob &b)
{
    return a.src == b.src && a.dst == b.dst && a.sstride == b.sstride && a.pw == b.pw && a.ph == b.ph && a.dpitch == b.dpitch && a.shift == b.shift;
}
bool same(const ResizeOutJob &a, const ResizeOutJob &b)
{
    return a.src == b.src && a.dst == b.dst && a.sstride == b.sstride && a.dpitch == b.dpitch && a.pw == b.pw && a.ph == b.ph && a.ow == b.ow && a.oh == b.oh && a.a == b.a &&
           a.b == b.b && a.c == b.c && a.d == b.d && a.D == b.D && a.rD == b.rD && a.rb == b.rb && a.rd == b.rd;
}
bool same(const UvEgressJob &a, const UvEgressJob &b)
{
    return a.su == b.su && a.sv == b.sv && a.dst == b.dst && a.dpitch == b.dpitch && a.sstride == b.sstride && a.sw == b.sw && a.sh == b.sh && a.cw == b.cw && a.ch == b.ch &&
           a.mode == b.mode;
}
bool same(const RgbOutCoefs &a, const RgbOutCoefs &b) { return a.ky == b.ky && a.ybase == b.ybase && a.rv == b.rv && a.gu == b.gu && a.gv == b.gv && a.bu == b.bu; }
bool same(const RgbOutJob &a, const RgbOutJob &b)
{
    return a.sy == b.sy && a.su == b.su && a.sv == b.sv && a.dst == b.dst && a.ystride == b.ystride && a.cstride == b.cstride && a.dpitch == b.dpitch && a.w == b.w &&
           a.h == b.h && a.hs == b.hs && a.vs == b.vs && same(a.csc, b.csc) && a.bgra == b.bgra;
}
bool same(const TensorOutJob &a, const TensorOutJob &b)
{
    bool ok = a.sy == b.sy && a.su == b.su && a.sv == b.sv && a.ystride == b.ystride && a.cstride == b.cstride && a.w == b.w && a.h == b.h && a.hs == b.hs && a.vs == b.vs &&
              same(a.csc, b.csc) && a.dtype == b.dtype;
    for (int k = 0; k < 3; k++) { // (the constants as bits: a NaN would not equal itself)
        ok = ok && a.dst[k] == b.dst[k] && a.dpitch[k] == b.dpitch[k] && memcmp(&a.scale[k], &b.scale[k], 4) == 0 && memcmp(&a.bias[k], &b.bias[k], 4) == 0;
    }
    return ok;
}
template <class T> bool same_jobs(const T *a, int na, const T *b, int nb)
{
    if (na != nb) {
        return false;
    }
    for (int i = 0; i < na; i++) {
        if (!same(a[i], b[i])) {
            return false;
        }
    }
    return true;
}
#endif

void check_existing(const Old &c)
{
    namespace N = delivery;
    const Staging S(c.fmt, c.w, c.h);
    Staging H(c.fmt, c.w, c.h); // (a target with a shift alone: the scaled picture is laid out for half size, as the older sweep has it)
    if (c.shift && c.kind != 4) {
        U64 at = kScaledAt;
        for (int k = 0; k < 3; k++) {
            const int sw = (S.recon.p[k].w + 1) >> 1, sh = (S.recon.p[k].h + 1) >> 1;
            H.scaled[k] = DPlane{(uint8_t *) (uintptr_t) at, (sw + 15) & ~15, sw, sh};
            at += (U64) H.scaled[k].stride * (U64) sh;
        }
    }
    const N::OutTarget tn = make_target<N::OutTarget>(c, N::target_frame, N::target_surface, N::target_tensor);
    const bool luma = N::needs_staged_luma(tn, c.sharp, c.draw), scaled = N::needs_staged_scaled(tn), full = N::needs_staged_full(tn);
    if (tn.converted() != (c.kind >= 3)) {
        fail(c.name(), "converted() is wrong");
    }
    const int out_format = c.out420p ? DSV_SUBSAMP_420 : c.fmt;
    const N::DeliveryPlan a = N::plan_delivery(S.recon, out_format, tn, c.sharp, c.draw, luma ? S.luma : kNone, scaled ? H.scaled : nullptr);
    (c.kind == 4 ? g_tensor : g_existing)++;
    if (a.n_hwc || !a.hwc_wide) {
        fail(c.name(), "a target that is no HWC tensor has an HWC job or fact");
    }
#ifdef PARENT_HEADER
    namespace P = delivery_parent;
    const P::OutTarget tp = make_target<P::OutTarget>(c, P::target_frame, P::target_surface, P::target_tensor);
    if (luma != P::needs_staged_luma(tp, c.sharp, c.draw) || scaled != P::needs_staged_scaled(tp) || full != P::needs_staged_full(tp)) {
        fail(c.name(), "the staging predicates changed");
    }
    const P::DeliveryPlan b = P::plan_delivery(S.recon, out_format, tp, c.sharp, c.draw, luma ? S.luma : kNone, scaled ? H.scaled : nullptr);
    const bool jobs = same_jobs(a.copy, a.n_copy, b.copy, b.n_copy) && same_jobs(a.to420, a.n_to420, b.to420, b.n_to420) && same_jobs(a.eg, a.n_eg, b.eg, b.n_eg) &&
                      same_jobs(a.scl, a.n_scl, b.scl, b.n_scl) && same_jobs(a.rsz, a.n_rsz, b.rsz, b.n_rsz) && same_jobs(a.uv, a.n_uv, b.uv, b.n_uv) &&
                      same_jobs(a.rgb, a.n_rgb, b.rgb, b.n_rgb) && same_jobs(a.overlay, a.n_overlay, b.overlay, b.n_overlay) && same_jobs(a.ten, a.n_ten, b.ten, b.n_ten);
    const bool facts = a.sharpen_overlaid == b.sharpen_overlaid && a.eg_wide == b.eg_wide && a.eg_sharp == b.eg_sharp && a.scl_wide == b.scl_wide && a.scl_rows == b.scl_rows &&
                       a.rsz_wide == b.rsz_wide && a.rsz_rows == b.rsz_rows && a.rsz_cols == b.rsz_cols && a.uv_wide == b.uv_wide && a.uv_conv == b.uv_conv &&
                       a.uv_rows == b.uv_rows && a.rgb_wide == b.rgb_wide && a.ten_wide == b.ten_wide;
    if (!jobs || !facts) {
        fail(c.name(), "the plan differs from the parent planner's (%s)", jobs ? "facts" : "jobs");
    }
    print_plan(c, b, P::needs_staged_luma(tp, c.sharp, c.draw), P::needs_staged_scaled(tp), P::needs_staged_full(tp));
#else
    print_plan(c, a, luma, scaled, full);
#endif
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
                        for (int offset : offsets) {
                            for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                                for (int bgr = 0; bgr < 2; bgr++) {
                                    check_hwc(Case{fmt, w, h, dtype, bgr, o[0], o[1], (sd & 1) != 0, (sd & 2) ? 7 : 0, offset, pitch_kind});
                                }
                                // the TENSOR case of tools/dec_tensor_plan_check.cpp (the element type in `shift`)
                                check_existing(Old{fmt, w, h, 4, dtype, o[0], o[1], false, (sd & 1) != 0, (sd & 2) ? 7 : 0, offset, pitch_kind});
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
    if (g_wide == 0 || g_wide == g_hwc) {
        fprintf(stderr, "FAILED: the sweep holds only one form of the HWC conversion\n");
        return 1;
    }
    printf("dec_hwc_plan_check: %ld hwc cases (%ld in the wide form): target, staging, jobs and form hold; %ld plans of the other targets and %ld of tensor targets "
           "printed%s\n",
           g_hwc, g_wide, g_existing, g_tensor,
#ifdef PARENT_HEADER
           " from the PARENT planner, each equal to this tree's"
#else
           ""
#endif
    );
    return 0;
}
