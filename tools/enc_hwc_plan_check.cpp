// enc_hwc_plan_check.cpp -- the encoder's acceptance rule and ingest planner (csrc/enc_ingest.h) swept on the CPU for HWC sources
// (dsv2hip_enc_batch_hwc): chroma format x picture size x element type x element order x pointer offset x pitch, over FAKE addresses
// as tools/enc_tensor_plan_check.cpp does -- nothing is ever dereferenced or launched.  Meant to be built with AddressSanitizer and
// UndefinedBehaviorSanitizer.
//   hwc       accept_hwc takes a tensor whose rows hold the picture and refuses, one spoiled field each, an unknown dtype, an order that
//             is not exactly RGB or BGR (RGBP, the four-byte layouts, 0, CSC bits inside it), a csc bit outside the two, a NULL data, a
//             pointer or a pitch off the element grid, pitch / elem < 3 * w, a constant that is not finite (float types; a uint8
//             tensor's are not looked at), an encoder with UYVY input on and a format outside the five; a float tensor's plan holds ONE
//             HwcInJob in the class behind TENSOR_IN and none of another class, reading exactly h rows of 3 * w elements, writing the
//             encoder's three planes, with the preset's quads in MEMORY order, the element type and the constants by position; its wide
//             fact is hwc_in_job_wide of the job.  A uint8 tensor gives, member for member, the source and the plan of the
//             DSV2HIP_SURFACE_RGB / _BGR | csc surface.  One line per case goes to stdout for tests/test_enc_hwc_plan_cpu.py to compare
//             with its own restatement of the rules:
//               H fmt w h dtype order offset pitch_kind : n_hwc n_rgb3_packed wide
//   existing  for every surface kind, call and route tools/enc_ingest_check.cpp sweeps, every member an IngestPlan had before the
//             header knew tensors goes to stdout ("P case : members", the lines of tools/enc_tensor_plan_check.cpp); the test compares
//             their digests with tests/golden/enc_plans_parent.json.  For every planar tensor case of that program's sweep the whole plan
//             goes to stdout, tensor job and constants included ("T case : members"); their digests are
//             tests/golden/enc_tensor_plans_parent.json.  Neither kind of plan holds an HWC job, and its HWC class is planned wide (the
//             neutral value).
//   parent    how the second file was recorded, and a check of its own: with -DPARENT_HEADER="file" (the text of the parent commit's
//             enc_ingest.h -- git show PARENT:digital-subband-video-2_amd/csrc/enc_ingest.h -- with `namespace enc_ingest {` replaced
//             by `namespace enc_ingest_parent {`) both planners run side by side in this one program, acceptance and every one of those
//             members compare equal, and the P and T lines printed are the PARENT planner's.
// tests/test_enc_hwc_plan_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/enc_hwc_plan_check.cpp -o enc_hwc_plan_check
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>

#include "enc_ingest.h"
#ifdef PARENT_HEADER
#include PARENT_HEADER
#endif

using namespace dsv2;

namespace {

typedef unsigned long long U64;
constexpr U64 kFrameAt = 0x10000000ull, kSourceAt = 0x100000000ull, kPlaneApart = 0x40000000ull;

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
DFrame fake_frame(U64 base, int format, int w, int h)
{
    DFrame f;
    f.format = format, f.w = w, f.h = h;
    f.alloc = (uint8_t *) (uintptr_t) base;
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

// ---- HWC sources ------------------------------------------------------------------------------------------------------------------
const int kQuads[4][9] = {{66, 129, 25, -38, -74, 112, 112, -94, -18},
                          {47, 157, 16, -26, -86, 112, 112, -102, -10},
                          {77, 150, 29, -43, -85, 128, 128, -107, -21},
                          {54, 183, 19, -29, -99, 128, 128, -116, -12}};
// the row's coefficients of R, G, B at the byte the order gives each (B G R: blue is byte 0): the positive parts, or the magnitudes of
// the negative ones
uint32_t quad(const int *row, bool negative, bool b_first)
{
    uint32_t q = 0;
    for (int c = 0; c < 3; c++) {
        if ((row[c] < 0) == negative) {
            q |= (uint32_t) (row[c] < 0 ? -row[c] : row[c]) << (8 * (b_first ? 2 - c : c));
        }
    }
    return q;
}

struct Case {
    int fmt, w, h, dtype, order, offset, pitch_kind; // offset: elements behind a 256-byte boundary; pitch: tight, + 1 element, rounded up to 256
    std::string name() const
    {
        char s[160];
        snprintf(s, sizeof s, "hwc fmt=%#x %dx%d dtype=%d order=%#x offset=%d pitch=%d", fmt, w, h, dtype, order, offset, pitch_kind);
        return s;
    }
};
long g_hwc = 0, g_wide = 0;

void check_hwc(const Case &c)
{
    using namespace enc_ingest;
    const int elem = tensor_elem(c.dtype), hs = DSV_FORMAT_H_SHIFT(c.fmt), vs = DSV_FORMAT_V_SHIFT(c.fmt);
    const size_t rb = 3 * (size_t) c.w * (size_t) elem;
    const size_t pitch = c.pitch_kind == 0 ? rb : c.pitch_kind == 1 ? rb + (size_t) elem : (rb + 255) / 256 * 256;
    dsv2hip_in_hwc tn = {};
    tn.dtype = c.dtype, tn.order = c.order, tn.csc = ((c.w + c.offset) & 1 ? DSV2HIP_CSC_FULL_RANGE : 0) | (c.pitch_kind & 1 ? DSV2HIP_CSC_BT709 : 0);
    tn.data = (const void *) (uintptr_t) (kSourceAt + 256 + (U64) c.offset * (U64) elem);
    tn.pitch = pitch;
    for (int k = 0; k < 3; k++) {
        tn.scale[k] = 0.25f * (float) (k + 1), tn.bias[k] = -1.5f * (float) k;
    }
    Source s, never;
    if (!accept_hwc(c.w, c.h, c.fmt, false, tn, &s)) {
        fail(c.name(), "accept_hwc refused a tensor whose rows hold the picture");
    }
    // what accept_hwc refuses, one spoiled field each
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        dsv2hip_in_hwc bad = tn;
        bool refused = !accept_hwc(c.w, c.h, c.fmt, true, tn, &never) && !accept_hwc(c.w, c.h, DSV_SUBSAMP_UYVY, false, tn, &never);
        bad.dtype = 4;
        refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.dtype = -1;
        refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        for (int order : {0, 1, (int) DSV2HIP_SURFACE_BGRA, (int) DSV2HIP_SURFACE_RGBA, (int) DSV2HIP_SURFACE_RGBP, 0x23, c.order | DSV2HIP_CSC_BT709, c.order | DSV2HIP_CSC_FULL_RANGE, c.order | 0x1000}) {
            bad = tn, bad.order = order;
            refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        }
        bad = tn, bad.csc |= 0x400;
        refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.csc |= DSV2HIP_SURFACE_RGB;
        refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.data = nullptr;
        refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.pitch = rb - (size_t) elem;
        refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.pitch = (size_t) c.w * (size_t) elem; // (a planar tensor's row)
        refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        if (elem > 1) {
            bad = tn, bad.data = (const char *) tn.data + 1;
            refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.pitch = pitch + 1;
            refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.scale[2] = inf;
            refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.scale[0] = nan;
            refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.bias[1] = -inf;
            refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.bias[0] = nan;
            refused = refused && !accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        } else { // uint8: the constants are not looked at
            bad = tn, bad.scale[2] = inf, bad.bias[0] = nan;
            refused = refused && accept_hwc(c.w, c.h, c.fmt, false, bad, &never);
        }
        if (!refused) {
            fail(c.name(), "accept_hwc took a spoiled tensor (or refused constants a uint8 tensor ignores)");
        }
    }
    const DFrame f = fake_frame(kFrameAt, c.fmt, c.w, c.h);
    const IngestPlan p = plan_ingest(f, s);
    g_hwc++;
    const bool wide = c.offset % 4 == 0 && c.w % 4 == 0 && pitch % (size_t) (4 * elem) == 0;
    if (c.dtype == kTensorU8) { // the three-byte surface, member for member
        const dsv2hip_surface sf{{tn.data, nullptr, nullptr}, {tn.pitch, 0, 0}, c.order | tn.csc};
        Source q;
        if (!accept(CALL_PLAIN, c.w, c.h, c.fmt, false, sf, 0, 0, &q) || memcmp(&q, &s, sizeof q) != 0 || s.kind != Source::RGB3) {
            fail(c.name(), "a uint8 tensor is not the three-byte surface's source");
        }
        const IngestPlan ps = plan_ingest(f, q);
        const Rgb3Job &a = p.rgb3[0], &b = ps.rgb3[0];
        bool same = p.scaled_row_bytes == ps.scaled_row_bytes && p.scaled_rgb_sw == ps.scaled_rgb_sw && a.kind == b.kind && a.kind == kRgb3Packed && a.ystride == b.ystride &&
                    a.cstride == b.cstride && a.w == b.w && a.h == b.h && a.hs == b.hs && a.vs == b.vs && memcmp(&a.csc, &b.csc, sizeof a.csc) == 0;
        for (int k = 0; k < 3; k++) {
            same = same && a.src[k] == b.src[k] && a.pitch[k] == b.pitch[k] && a.dst[k] == b.dst[k];
        }
        for (int cl = 0; cl < kClasses; cl++) {
            same = same && p.n[cl] == ps.n[cl] && p.wide[cl] == ps.wide[cl];
            if (p.n[cl] != (cl == RGB3_PACKED) || p.wide[cl] != (cl == RGB3_PACKED ? wide : true)) {
                fail(c.name(), "a uint8 tensor's plan: %d records of class %d, planned %s", p.n[cl], cl, p.wide[cl] ? "wide" : "general");
            }
        }
        if (!same) {
            fail(c.name(), "a uint8 tensor's plan is not the three-byte surface's");
        }
    } else {
        if (s.kind != Source::HWC || s.route != Source::PLAIN || !s.surface() || !s.rgb() || s.layout != (c.order | tn.csc)) {
            fail(c.name(), "the source record says kind %d, route %d, layout %#x", (int) s.kind, (int) s.route, s.layout);
        }
        for (int cl = 0; cl < kClasses; cl++) {
            if (p.n[cl] != (cl == HWC_IN) || p.wide[cl] != (cl == HWC_IN ? wide : true)) {
                fail(c.name(), "%d records of class %d, planned %s", p.n[cl], cl, p.wide[cl] ? "wide" : "general");
            }
        }
        const HwcInJob &j = p.hwc[0];
        const int preset = ((tn.csc & DSV2HIP_CSC_FULL_RANGE) ? 2 : 0) + ((tn.csc & DSV2HIP_CSC_BT709) ? 1 : 0);
        const int *m = kQuads[preset];
        const bool bf = c.order == DSV2HIP_SURFACE_BGR;
        bool ok = j.ystride == f.p[0].stride && j.cstride == f.p[1].stride && j.w == c.w && j.h == c.h && j.hs == hs && j.vs == vs && j.dtype == c.dtype &&
                  j.csc.ycoef == quad(m, false, bf) && j.csc.upos == quad(m + 3, false, bf) && j.csc.uneg == quad(m + 3, true, bf) && j.csc.vpos == quad(m + 6, false, bf) &&
                  j.csc.vneg == quad(m + 6, true, bf) && j.csc.yoff == 128u + (preset >= 2 ? 0u : 4096u) && quad(m, true, bf) == 0;
        ok = ok && j.src == tn.data && j.pitch == tn.pitch;
        // reads: h rows of 3 * w elements, the last one ending where the caller's last row ends
        ok = ok && at(j.src) + (U64) (j.h - 1) * j.pitch + 3 * (U64) j.w * (U64) elem == at(tn.data) + (U64) (c.h - 1) * tn.pitch + rb;
        for (int k = 0; k < 3; k++) {
            ok = ok && j.dst[k] == f.p[k].data && j.scale[k] == tn.scale[k] && j.bias[k] == tn.bias[k]; // (by position, whatever the order)
        }
        if (!ok || hwc_in_job_wide(j) != wide) {
            fail(c.name(), "the job does not read the tensor's rows with its constants, write the encoder's planes or say its form");
        }
    }
    g_wide += wide;
    printf("H %d %d %d %d %d %d %d : %d %d %d\n", c.fmt, c.w, c.h, c.dtype, c.order, c.offset, c.pitch_kind, p.n[enc_ingest::HWC_IN], p.n[enc_ingest::RGB3_PACKED], (int) wide);
}

// ---- the sources that existed before: both planners side by side -------------------------------------------------------------------
long g_existing = 0, g_taken = 0, g_tensor = 0;
struct Old {
    int fmt, w, h, kind, way, offset, pitch_kind; // kind: Source::PLANAR .. RGBP; way: tools/enc_ingest_check.cpp's twelve
};
struct Way {
    int call, shift, size; // size: 0 own, 1 one column more, 2 3 : 2, 3 8 : 1
};
const Way kWays[12] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 2, 0}, {1, 3, 0}, {2, 0, 0}, {2, 0, 1}, {2, 0, 2}, {2, 0, 3}, {2, 1, 0}, {2, 2, 0}, {2, 3, 0}};

void print_ratio(const SizedRatio &q) { printf(" %u %u %u %u %u %u %u %u", q.a, q.b, q.c, q.d, q.D, q.rD, q.rb, q.rd); }
template <class J> void print_quads(const J &j) { printf(" %x %x %x %x %x %x", j.csc.ycoef, j.csc.upos, j.csc.uneg, j.csc.vpos, j.csc.vneg, j.csc.yoff); }
// the members an IngestPlan had before tensors, as text (addresses are the synthetic ones): tools/enc_tensor_plan_check.cpp's words
template <class Plan> void print_plan(const Plan &p)
{
    for (int cl = 0; cl < 8; cl++) {
        printf(" %d%d", p.n[cl], (int) p.wide[cl]);
    }
    printf(" %d %d", p.scaled_row_bytes, p.scaled_rgb_sw);
    for (int i = 0; i < p.n[0]; i++) {
        const SurfaceJob &j = p.surf[i];
        printf(" surf %llx %zu %llx %llx %d %d %d", at(j.src), j.pitch, at(j.dst), at(j.dst2), j.dstride, j.w, j.h);
    }
    for (int i = 0; i < p.n[1]; i++) {
        const RgbJob &j = p.rgb[i];
        printf(" rgb %llx %zu %llx %llx %llx %d %d %d %d %d %d", at(j.src), j.pitch, at(j.dst[0]), at(j.dst[1]), at(j.dst[2]), j.ystride, j.cstride, j.w, j.h, j.hs, j.vs);
        print_quads(j);
    }
    for (int i = 0; i < p.n[2]; i++) {
        const ScaledSurfaceJob &j = p.scaled_surf[i];
        printf(" ssurf %llx %zu %llx %llx %d %d %d %d", at(j.src), j.pitch, at(j.dst), at(j.dst2), j.dstride, j.pw, j.ph, j.shift);
    }
    for (int i = 0; i < p.n[3]; i++) {
        const ScaledRgbJob &j = p.scaled_rgb[i];
        printf(" srgb %llx %zu %llx %llx %llx %d %d %d %d %d %d %d", at(j.src), j.pitch, at(j.dst[0]), at(j.dst[1]), at(j.dst[2]), j.ystride, j.cstride, j.sw, j.sh, j.hs, j.vs,
               j.shift);
        print_quads(j);
    }
    for (int i = 0; i < p.n[4]; i++) {
        const SizedSurfaceJob &j = p.sized_surf[i];
        printf(" zsurf %llx %zu %llx %d %d %d %u %u", at(j.src), j.pitch, at(j.dst), j.dstride, j.ow, j.oh, j.step, j.off);
        print_ratio(j.q);
    }
    for (int i = 0; i < p.n[5]; i++) {
        const SizedRgbJob &j = p.sized_rgb[i];
        printf(" zrgb %llx %zu %llx %llx %llx %d %d %d %d %d %d", at(j.src), j.pitch, at(j.dst[0]), at(j.dst[1]), at(j.dst[2]), j.ystride, j.cstride, j.ow, j.oh, j.cw, j.ch);
        print_ratio(j.ql), print_ratio(j.qc), print_quads(j);
    }
    for (int i = 0; i < p.n[6] + p.n[7]; i++) {
        const Rgb3Job &j = p.rgb3[i];
        printf(" rgb3 %llx %llx %llx %zu %zu %zu %llx %llx %llx %d %d %d %d %d %d %d", at(j.src[0]), at(j.src[1]), at(j.src[2]), j.pitch[0], j.pitch[1], j.pitch[2], at(j.dst[0]),
               at(j.dst[1]), at(j.dst[2]), j.ystride, j.cstride, j.w, j.h, j.hs, j.vs, j.kind);
        print_quads(j);
    }
}
// ... and what DESIGN 5.22 added: the tensor class and its job, constants as bit patterns
template <class Plan> void print_tensor_part(const Plan &p)
{
    printf(" t %d%d", p.n[8], (int) p.wide[8]);
    for (int i = 0; i < p.n[8]; i++) {
        const TensorInJob &j = p.tensor[i];
        printf(" ten %llx %llx %llx %zu %zu %zu %llx %llx %llx %d %d %d %d %d %d %d", at(j.src[0]), at(j.src[1]), at(j.src[2]), j.pitch[0], j.pitch[1], j.pitch[2], at(j.dst[0]),
               at(j.dst[1]), at(j.dst[2]), j.ystride, j.cstride, j.w, j.h, j.hs, j.vs, j.dtype);
        print_quads(j);
        for (int k = 0; k < 3; k++) {
            uint32_t sb, bb;
            memcpy(&sb, &j.scale[k], 4), memcpy(&bb, &j.bias[k], 4);
            printf(" %x %x", sb, bb);
        }
    }
}

// a planner's acceptance rules and plan_ingest under one name each
struct ThisTree {
    typedef enc_ingest::Source Source;
    typedef enc_ingest::IngestPlan IngestPlan;
    static bool accept(int call, int w, int h, int fmt, bool uyvy, const dsv2hip_surface &sf, int sw, int sh, Source *out)
    {
        return enc_ingest::accept((enc_ingest::Call) call, w, h, fmt, uyvy, sf, sw, sh, out);
    }
    static bool accept_tensor(int w, int h, int fmt, bool uyvy, const dsv2hip_in_tensor &t, Source *out) { return enc_ingest::accept_tensor(w, h, fmt, uyvy, t, out); }
    static IngestPlan plan(const DFrame &f, const Source &s) { return enc_ingest::plan_ingest(f, s); }
};
#ifdef PARENT_HEADER
struct ParentTree {
    typedef enc_ingest_parent::Source Source;
    typedef enc_ingest_parent::IngestPlan IngestPlan;
    static bool accept(int call, int w, int h, int fmt, bool uyvy, const dsv2hip_surface &sf, int sw, int sh, Source *out)
    {
        return enc_ingest_parent::accept((enc_ingest_parent::Call) call, w, h, fmt, uyvy, sf, sw, sh, out);
    }
    static bool accept_tensor(int w, int h, int fmt, bool uyvy, const dsv2hip_in_tensor &t, Source *out)
    {
        return enc_ingest_parent::accept_tensor(w, h, fmt, uyvy, t, out);
    }
    static IngestPlan plan(const DFrame &f, const Source &s) { return enc_ingest_parent::plan_ingest(f, s); }
};
#endif

// what `print` writes to stdout, as a string (so that the side-by-side build can compare the two planners' lines as text)
template <class F> std::string printed(F print)
{
    char *buf = nullptr;
    size_t len = 0;
    FILE *mem = open_memstream(&buf, &len), *was = stdout;
    stdout = mem;
    print();
    stdout = was;
    fclose(mem);
    std::string out(buf, len);
    free(buf);
    return out;
}

// the case's line as planner T gives it: its verdict and, where it takes the surface, its source record and its plan
template <class T> std::string line_of(const Old &c, const dsv2hip_surface &sf, int sw, int sh, const DFrame &f, bool *taken)
{
    typename T::Source s, never;
    *taken = T::accept(kWays[c.way].call, c.w, c.h, c.fmt, false, sf, sw, sh, &s);
    if (T::accept(kWays[c.way].call, c.w, c.h, c.fmt, true, sf, sw, sh, &never)) {
        fail("existing", "taken by an encoder with UYVY input on");
    }
    return printed([&] {
        printf("P %d %d %d %d %d %d %d : %d", c.fmt, c.w, c.h, c.kind, c.way, c.offset, c.pitch_kind, (int) *taken);
        if (*taken) {
            printf(" s %d %d %d %d %d %x", (int) s.kind, (int) s.route, s.src_w, s.src_h, s.shift, s.layout);
            const typename T::IngestPlan p = T::plan(f, s);
            print_plan(p);
        }
        printf("\n");
    });
}

void check_existing(const Old &c, long turn)
{
    const Way &way = kWays[c.way];
    const int s = way.shift, hs = DSV_FORMAT_H_SHIFT(c.fmt), vs = DSV_FORMAT_V_SHIFT(c.fmt);
    const int sw = s ? (c.w << s) - 1 : way.size == 1 ? c.w + 1 : way.size == 2 ? c.w * 3 / 2 : way.size == 3 ? 8 * c.w : c.w;
    const int sh = s ? c.h << s : way.size == 2 ? c.h * 3 / 2 : way.size == 3 ? 8 * c.h : c.h;
    const int csc = (int) ((turn >> 1) & 3) << 8, scw = cdiv(sw, hs), sch = cdiv(sh, vs);
    (void) sch;
    using enc_ingest::Source;
    int layout = c.kind == Source::PLANAR ? DSV2HIP_SURFACE_PLANAR
                 : c.kind == Source::SEMI ? DSV2HIP_SURFACE_SEMIPLANAR
                 : c.kind == Source::RGBP ? DSV2HIP_SURFACE_RGBP | csc
                                          : ((c.kind == Source::RGB4 ? DSV2HIP_SURFACE_BGRA : DSV2HIP_SURFACE_BGR) + (int) (turn & 1)) | csc;
    layout |= s << 12;
    if (layout == 0x1010) { // (the value the grammar holds back)
        layout |= DSV2HIP_CSC_BT709;
    }
    long row_bytes[3] = {sw, scw, scw};
    int nplanes = 3;
    if (c.kind == Source::SEMI) {
        nplanes = 2, row_bytes[1] = 2L * scw;
    } else if (c.kind == Source::RGBP) {
        row_bytes[1] = row_bytes[2] = sw;
    } else if (c.kind != Source::PLANAR) {
        nplanes = 1, row_bytes[0] = (c.kind == Source::RGB4 ? 4L : 3L) * sw;
    }
    dsv2hip_surface sf{};
    sf.layout = layout;
    for (int p = 0; p < nplanes; p++) {
        sf.plane[p] = (const void *) (uintptr_t) (kSourceAt + (U64) p * kPlaneApart + (U64) c.offset);
        sf.pitch[p] = c.pitch_kind == 0 ? (size_t) row_bytes[p] : c.pitch_kind == 1 ? (size_t) row_bytes[p] + 1 : ((size_t) row_bytes[p] + 255) & ~(size_t) 255;
    }
    const DFrame f = fake_frame(kFrameAt, c.fmt, c.w, c.h);
    bool taken;
    const std::string mine = line_of<ThisTree>(c, sf, sw, sh, f, &taken);
    g_existing++, g_taken += taken;
    if (taken) { // a plan of a surface holds no HWC job, and its HWC class keeps the neutral value
        enc_ingest::Source src;
        enc_ingest::accept((enc_ingest::Call) way.call, c.w, c.h, c.fmt, false, sf, sw, sh, &src);
        const enc_ingest::IngestPlan p = enc_ingest::plan_ingest(f, src);
        if (p.n[enc_ingest::HWC_IN] || !p.wide[enc_ingest::HWC_IN] || src.kind == Source::HWC) {
            fail("existing", "a surface has an HWC job or fact");
        }
    }
#ifdef PARENT_HEADER
    bool parent_taken;
    const std::string parents = line_of<ParentTree>(c, sf, sw, sh, f, &parent_taken);
    if (parents != mine) {
        fail("existing", "the plan differs from the parent planner's:\n%s%s", parents.c_str(), mine.c_str());
    }
    fputs(parents.c_str(), stdout);
#else
    fputs(mine.c_str(), stdout);
#endif
}

// ---- DESIGN 5.22's planar tensor cases: tools/enc_tensor_plan_check.cpp's sweep and tensors, the whole plan printed -------------------
struct TensorCase {
    int fmt, w, h, dtype, offset, pitch_kind;
};
template <class T> std::string tensor_line_of(const TensorCase &c, const dsv2hip_in_tensor &tn, const DFrame &f)
{
    typename T::Source s;
    const bool taken = T::accept_tensor(c.w, c.h, c.fmt, false, tn, &s);
    return printed([&] {
        printf("T %d %d %d %d %d %d : %d", c.fmt, c.w, c.h, c.dtype, c.offset, c.pitch_kind, (int) taken);
        if (taken) {
            printf(" s %d %d %d %d %d %x %d", (int) s.kind, (int) s.route, s.src_w, s.src_h, s.shift, s.layout, s.dtype);
            const typename T::IngestPlan p = T::plan(f, s);
            print_plan(p), print_tensor_part(p);
        }
        printf("\n");
    });
}
void check_tensor(const TensorCase &c)
{
    const int elem = tensor_elem(c.dtype);
    const size_t rb = (size_t) c.w * (size_t) elem;
    const size_t pitch = c.pitch_kind == 0 ? rb : c.pitch_kind == 1 ? rb + (size_t) elem : (rb + 255) / 256 * 256;
    dsv2hip_in_tensor tn = {};
    tn.dtype = c.dtype, tn.csc = ((c.w + c.offset) & 1 ? DSV2HIP_CSC_FULL_RANGE : 0) | (c.pitch_kind & 1 ? DSV2HIP_CSC_BT709 : 0);
    for (int k = 0; k < 3; k++) {
        tn.plane[k] = (const void *) (uintptr_t) (kSourceAt + (U64) k * kPlaneApart + 256 + (U64) c.offset * (U64) elem);
        tn.pitch[k] = pitch + (size_t) (16 * k * (c.pitch_kind == 2));
        tn.scale[k] = 0.25f * (float) (k + 1), tn.bias[k] = -1.5f * (float) k;
    }
    const DFrame f = fake_frame(kFrameAt, c.fmt, c.w, c.h);
    const std::string mine = tensor_line_of<ThisTree>(c, tn, f);
    g_tensor++;
    enc_ingest::Source src;
    if (!enc_ingest::accept_tensor(c.w, c.h, c.fmt, false, tn, &src)) {
        fail("tensor", "a planar tensor whose rows hold the picture is refused");
    }
    const enc_ingest::IngestPlan p = enc_ingest::plan_ingest(f, src);
    if (p.n[enc_ingest::HWC_IN] || !p.wide[enc_ingest::HWC_IN] || src.kind == enc_ingest::Source::HWC) {
        fail("tensor", "a planar tensor has an HWC job or fact");
    }
#ifdef PARENT_HEADER
    const std::string parents = tensor_line_of<ParentTree>(c, tn, f);
    if (parents != mine) {
        fail("tensor", "the plan differs from the parent planner's:\n%s%s", parents.c_str(), mine.c_str());
    }
    fputs(parents.c_str(), stdout);
#else
    fputs(mine.c_str(), stdout);
#endif
}

} // namespace

int main()
{
    static const int formats[] = {DSV_SUBSAMP_444, DSV_SUBSAMP_422, DSV_SUBSAMP_420, DSV_SUBSAMP_411, DSV_SUBSAMP_410};
    static const int sizes[][2] = {{16, 16}, {34, 18}, {66, 34}, {352, 288}, {1920, 1080}};
    static const int offsets[] = {0, 1, 2, 4};
    long turn = 0;
    for (int fmt : formats) {
        for (const int *wh : sizes) {
            for (int dtype = 0; dtype < 4; dtype++) {
                for (int offset : offsets) {
                    for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                        for (int order : {(int) DSV2HIP_SURFACE_RGB, (int) DSV2HIP_SURFACE_BGR}) {
                            check_hwc(Case{fmt, wh[0], wh[1], dtype, order, offset, pitch_kind});
                        }
                        check_tensor(TensorCase{fmt, wh[0], wh[1], dtype, offset, pitch_kind});
                    }
                }
            }
            for (int kind = enc_ingest::Source::PLANAR; kind <= enc_ingest::Source::RGBP; kind++) {
                for (int way = 0; way < 12; way++) {
                    for (int offset : {0, 1, 4, 16}) {
                        for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++, turn++) {
                            check_existing(Old{fmt, wh[0], wh[1], kind, way, offset, pitch_kind}, turn);
                        }
                    }
                }
            }
        }
    }
    if (g_wide == 0 || g_wide == g_hwc) {
        fprintf(stderr, "FAILED: the sweep holds only one form of the HWC ingest\n");
        return 1;
    }
    printf("enc_hwc_plan_check: %ld hwc cases (%ld in the wide form): acceptance, refusals, job and form hold; %ld planar tensor cases and %ld cases of the other sources "
           "(%ld taken) printed%s\n",
           g_hwc, g_wide, g_tensor, g_existing, g_taken,
#ifdef PARENT_HEADER
           " from the PARENT planner, each equal to this tree's"
#else
           ""
#endif
    );
    return 0;
}
