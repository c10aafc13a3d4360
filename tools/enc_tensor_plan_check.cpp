// enc_tensor_plan_check.cpp -- the encoder's acceptance rule and ingest planner (csrc/enc_ingest.h) swept on the CPU for TENSOR sources
// (dsv2hip_enc_batch_tensor): chroma format x picture size x element type x pointer offset x pitch, over FAKE addresses as
// tools/enc_ingest_check.cpp does -- nothing is ever dereferenced or launched.  Meant to be built with AddressSanitizer and
// UndefinedBehaviorSanitizer.
//   tensor    accept_tensor takes a tensor whose rows hold the picture and refuses, one spoiled field each, an unknown dtype, a csc bit
//             outside the two, a NULL plane, a pointer or a pitch off the element grid, a pitch below w * elem, a constant that is not
//             finite (float types; a uint8 tensor's are not looked at), an encoder with UYVY input on and a format outside the five; a
//             float tensor's plan holds ONE TensorInJob in the class behind RGB3_PLANAR and none of another class, reading exactly h rows
//             of w elements of each plane, writing the encoder's three planes, with the preset's planar quads, the element type and the
//             constants; its wide fact is tensor_in_job_wide of the job.  A uint8 tensor gives, member for member, the source and the
//             plan of the DSV2HIP_SURFACE_RGBP | csc surface.  One line per case goes to stdout for tests/test_enc_tensor_plan_cpu.py to
//             compare with its own restatement of the rules:
//               T fmt w h dtype offset pitch_kind : n_tensor n_rgb3_planar wide
//   existing  for every surface kind, call and route tools/enc_ingest_check.cpp sweeps, every member an IngestPlan had before this
//             header knew tensors goes to stdout, one line a case ("P case : members"); the test compares their digests with
//             tests/golden/enc_plans_parent.json, which was recorded from the PARENT commit's enc_ingest.h.  Such a plan holds no tensor
//             job, and its tensor class is planned wide (the neutral value).
//   parent    how that file was recorded, and a check of its own: with -DPARENT_HEADER="file" (the text of the parent commit's
//             enc_ingest.h -- git show PARENT:digital-subband-video-2_amd/csrc/enc_ingest.h -- with `namespace enc_ingest {` replaced
//             by `namespace enc_ingest_parent {`) both planners run side by side in this one program, acceptance and every one of those
//             members compare equal, and the lines printed are the PARENT planner's.
// tests/test_enc_tensor_plan_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/enc_tensor_plan_check.cpp -o enc_tensor_plan_check
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

// ---- tensor sources ---------------------------------------------------------------------------------------------------------------
const int kQuads[4][9] = {{66, 129, 25, -38, -74, 112, 112, -94, -18},
                          {47, 157, 16, -26, -86, 112, 112, -102, -10},
                          {77, 150, 29, -43, -85, 128, 128, -107, -21},
                          {54, 183, 19, -29, -99, 128, 128, -116, -12}};
uint32_t quad(const int *row, bool negative) // R G B in bytes 0..2: the positive parts, or the magnitudes of the negative ones
{
    uint32_t q = 0;
    for (int c = 0; c < 3; c++) {
        if ((row[c] < 0) == negative) {
            q |= (uint32_t) (row[c] < 0 ? -row[c] : row[c]) << (8 * c);
        }
    }
    return q;
}

struct Case {
    int fmt, w, h, dtype, offset, pitch_kind; // offset: elements behind a 256-byte boundary; pitch: tight, + 1 element, rounded up to 256
    std::string name() const
    {
        char s[160];
        snprintf(s, sizeof s, "tensor fmt=%#x %dx%d dtype=%d offset=%d pitch=%d", fmt, w, h, dtype, offset, pitch_kind);
        return s;
    }
};
long g_tensor = 0, g_wide = 0;

void check_tensor(const Case &c)
{
    using namespace enc_ingest;
    const int elem = tensor_elem(c.dtype), hs = DSV_FORMAT_H_SHIFT(c.fmt), vs = DSV_FORMAT_V_SHIFT(c.fmt);
    const size_t rb = (size_t) c.w * (size_t) elem;
    const size_t pitch = c.pitch_kind == 0 ? rb : c.pitch_kind == 1 ? rb + (size_t) elem : (rb + 255) / 256 * 256;
    dsv2hip_in_tensor tn = {};
    tn.dtype = c.dtype, tn.csc = ((c.w + c.offset) & 1 ? DSV2HIP_CSC_FULL_RANGE : 0) | (c.pitch_kind & 1 ? DSV2HIP_CSC_BT709 : 0);
    for (int k = 0; k < 3; k++) {
        tn.plane[k] = (const void *) (uintptr_t) (kSourceAt + (U64) k * kPlaneApart + 256 + (U64) c.offset * (U64) elem);
        tn.pitch[k] = pitch + (size_t) (16 * k * (c.pitch_kind == 2)); // (the planes' pitches may differ)
        tn.scale[k] = 0.25f * (float) (k + 1), tn.bias[k] = -1.5f * (float) k;
    }
    Source s, never;
    if (!accept_tensor(c.w, c.h, c.fmt, false, tn, &s)) {
        fail(c.name(), "accept_tensor refused a tensor whose rows hold the picture");
    }
    // what accept_tensor refuses, one spoiled field each
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        dsv2hip_in_tensor bad = tn;
        bool refused = !accept_tensor(c.w, c.h, c.fmt, true, tn, &never) && !accept_tensor(c.w, c.h, DSV_SUBSAMP_UYVY, false, tn, &never);
        bad.dtype = 4;
        refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.dtype = -1;
        refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.csc |= 0x400;
        refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.csc |= DSV2HIP_SURFACE_RGBP;
        refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.plane[1] = nullptr;
        refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
        bad = tn, bad.pitch[2] = rb - (size_t) elem;
        refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
        if (elem > 1) {
            bad = tn, bad.plane[0] = (const char *) tn.plane[0] + 1;
            refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.pitch[1] = pitch + 1;
            refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.scale[2] = inf;
            refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.scale[0] = nan;
            refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.bias[1] = -inf;
            refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
            bad = tn, bad.bias[0] = nan;
            refused = refused && !accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
        } else { // uint8: the constants are not looked at
            bad = tn, bad.scale[2] = inf, bad.bias[0] = nan;
            refused = refused && accept_tensor(c.w, c.h, c.fmt, false, bad, &never);
        }
        if (!refused) {
            fail(c.name(), "accept_tensor took a spoiled tensor (or refused constants a uint8 tensor ignores)");
        }
    }
    const DFrame f = fake_frame(kFrameAt, c.fmt, c.w, c.h);
    const IngestPlan p = plan_ingest(f, s);
    g_tensor++;
    const bool grid = (c.offset * elem) % (4 * elem) == 0 && c.w % 4 == 0;
    bool wide = grid;
    for (int k = 0; k < 3; k++) {
        wide = wide && tn.pitch[k] % (size_t) (4 * elem) == 0;
    }
    if (c.dtype == kTensorU8) { // the planar RGB surface, member for member
        const dsv2hip_surface sf{{tn.plane[0], tn.plane[1], tn.plane[2]}, {tn.pitch[0], tn.pitch[1], tn.pitch[2]}, DSV2HIP_SURFACE_RGBP | tn.csc};
        Source q;
        if (!accept(CALL_PLAIN, c.w, c.h, c.fmt, false, sf, 0, 0, &q) || memcmp(&q, &s, sizeof q) != 0 || s.kind != Source::RGBP) {
            fail(c.name(), "a uint8 tensor is not the planar RGB surface's source");
        }
        for (int cl = 0; cl < kClasses; cl++) {
            if (p.n[cl] != (cl == RGB3_PLANAR) || p.wide[cl] != (cl == RGB3_PLANAR ? wide : true)) {
                fail(c.name(), "a uint8 tensor's plan: %d records of class %d, planned %s", p.n[cl], cl, p.wide[cl] ? "wide" : "general");
            }
        }
    } else {
        if (s.kind != Source::TENSOR || s.route != Source::PLAIN || !s.surface() || !s.rgb()) {
            fail(c.name(), "the source record says kind %d, route %d", (int) s.kind, (int) s.route);
        }
        for (int cl = 0; cl < kClasses; cl++) {
            if (p.n[cl] != (cl == TENSOR_IN) || p.wide[cl] != (cl == TENSOR_IN ? wide : true)) {
                fail(c.name(), "%d records of class %d, planned %s", p.n[cl], cl, p.wide[cl] ? "wide" : "general");
            }
        }
        const TensorInJob &j = p.tensor[0];
        const int preset = ((tn.csc & DSV2HIP_CSC_FULL_RANGE) ? 2 : 0) + ((tn.csc & DSV2HIP_CSC_BT709) ? 1 : 0);
        const int *m = kQuads[preset];
        bool ok = j.ystride == f.p[0].stride && j.cstride == f.p[1].stride && j.w == c.w && j.h == c.h && j.hs == hs && j.vs == vs && j.dtype == c.dtype &&
                  j.csc.ycoef == quad(m, false) && j.csc.upos == quad(m + 3, false) && j.csc.uneg == quad(m + 3, true) && j.csc.vpos == quad(m + 6, false) && j.csc.vneg == quad(m + 6, true) &&
                  j.csc.yoff == 128u + (preset >= 2 ? 0u : 4096u) && quad(m, true) == 0;
        for (int k = 0; k < 3; k++) {
            ok = ok && j.src[k] == tn.plane[k] && j.pitch[k] == tn.pitch[k] && j.dst[k] == f.p[k].data && j.scale[k] == tn.scale[k] && j.bias[k] == tn.bias[k];
            // reads: h rows of w elements, the last one ending inside what the caller described
            ok = ok && at(j.src[k]) + (U64) (j.h - 1) * j.pitch[k] + (U64) j.w * (U64) elem <= at(tn.plane[k]) + (U64) (c.h - 1) * tn.pitch[k] + rb;
        }
        if (!ok || tensor_in_job_wide(j) != wide) {
            fail(c.name(), "the tensor job does not read the tensor's rows with its constants, write the encoder's planes or say its form");
        }
    }
    g_wide += wide;
    printf("T %d %d %d %d %d %d : %d %d %d\n", c.fmt, c.w, c.h, c.dtype, c.offset, c.pitch_kind, p.n[enc_ingest::TENSOR_IN], p.n[enc_ingest::RGB3_PLANAR], (int) wide);
}

// ---- the sources that existed before: both planners side by side -------------------------------------------------------------------
long g_existing = 0, g_taken = 0;
struct Old {
    int fmt, w, h, kind, way, offset, pitch_kind; // kind: Source::PLANAR .. RGBP; way: tools/enc_ingest_check.cpp's twelve
};
struct Way {
    int call, shift, size; // size: 0 own, 1 one column more, 2 3 : 2, 3 8 : 1
};
const Way kWays[12] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 2, 0}, {1, 3, 0}, {2, 0, 0}, {2, 0, 1}, {2, 0, 2}, {2, 0, 3}, {2, 1, 0}, {2, 2, 0}, {2, 3, 0}};

void print_ratio(const SizedRatio &q) { printf(" %u %u %u %u %u %u %u %u", q.a, q.b, q.c, q.d, q.D, q.rD, q.rb, q.rd); }
template <class J> void print_quads(const J &j) { printf(" %x %x %x %x %x %x", j.csc.ycoef, j.csc.upos, j.csc.uneg, j.csc.vpos, j.csc.vneg, j.csc.yoff); }
// the members an IngestPlan had before tensors, as text (addresses are the synthetic ones)
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

// a planner's acceptance rule and plan_ingest under one name each
struct ThisTree {
    typedef enc_ingest::Source Source;
    typedef enc_ingest::IngestPlan IngestPlan;
    static bool accept(int call, int w, int h, int fmt, bool uyvy, const dsv2hip_surface &sf, int sw, int sh, Source *out)
    {
        return enc_ingest::accept((enc_ingest::Call) call, w, h, fmt, uyvy, sf, sw, sh, out);
    }
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
    static IngestPlan plan(const DFrame &f, const Source &s) { return enc_ingest_parent::plan_ingest(f, s); }
};
#endif

// the case's line as planner T gives it: its verdict and, where it takes the surface, its source record and its plan (printed into a
// memory stream, so that the side-by-side build can compare the two planners' lines as text)
template <class T> std::string line_of(const Old &c, const dsv2hip_surface &sf, int sw, int sh, const DFrame &f, bool *taken)
{
    typename T::Source s, never;
    *taken = T::accept(kWays[c.way].call, c.w, c.h, c.fmt, false, sf, sw, sh, &s);
    if (T::accept(kWays[c.way].call, c.w, c.h, c.fmt, true, sf, sw, sh, &never)) {
        fail("existing", "taken by an encoder with UYVY input on");
    }
    char *buf = nullptr;
    size_t len = 0;
    FILE *mem = open_memstream(&buf, &len), *was = stdout;
    stdout = mem;
    printf("P %d %d %d %d %d %d %d : %d", c.fmt, c.w, c.h, c.kind, c.way, c.offset, c.pitch_kind, (int) *taken);
    if (*taken) {
        printf(" s %d %d %d %d %d %x", (int) s.kind, (int) s.route, s.src_w, s.src_h, s.shift, s.layout);
        const typename T::IngestPlan p = T::plan(f, s);
        print_plan(p);
    }
    printf("\n");
    stdout = was;
    fclose(mem);
    std::string out(buf, len);
    free(buf);
    return out;
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
    if (taken) { // a plan of a source that is no tensor holds no tensor job, and its tensor class keeps the neutral value
        enc_ingest::Source src;
        enc_ingest::accept((enc_ingest::Call) way.call, c.w, c.h, c.fmt, false, sf, sw, sh, &src);
        const enc_ingest::IngestPlan p = enc_ingest::plan_ingest(f, src);
        if (p.n[enc_ingest::TENSOR_IN] || !p.wide[enc_ingest::TENSOR_IN] || src.kind == Source::TENSOR) {
            fail("existing", "a surface has a tensor job or fact");
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
                        check_tensor(Case{fmt, wh[0], wh[1], dtype, offset, pitch_kind});
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
    if (g_wide == 0 || g_wide == g_tensor) {
        fprintf(stderr, "FAILED: the sweep holds only one form of the tensor ingest\n");
        return 1;
    }
    printf("enc_tensor_plan_check: %ld tensor cases (%ld in the wide form): acceptance, refusals, job and form hold; %ld cases of the other sources (%ld taken) printed%s\n",
           g_tensor, g_wide, g_existing, g_taken,
#ifdef PARENT_HEADER
           " from the PARENT planner, each equal to this tree's"
#else
           ""
#endif
    );
    return 0;
}
