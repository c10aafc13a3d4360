// enc_ingest_check.cpp -- the encoder's acceptance rule and ingest planner (csrc/enc_ingest.h) swept on the CPU: chroma format x encoder
// size x source kind x (call, route) x pointer offset x pitch, over FAKE addresses -- the encoder's source planes and the planes of the
// caller's surface are disjoint ranges of one synthetic address space, and nothing is ever dereferenced or launched.  Meant to be built
// with AddressSanitizer and UndefinedBehaviorSanitizer.  For every case the program works out, by its own interval arithmetic over the
// footprints io_jobs.h documents for each job record,
//   acceptance  the call takes or refuses the surface as the table below says (and refuses it on an encoder with UYVY input on);
//   counts      a taken picture brings the records of ONE launch class, as many as the second table says (restated as data);
//   coverage    the visible w x h of each of the encoder's three source planes is written by exactly one record, and nothing else is;
//   reads       what a record reads is exactly the samples that feed the plane(s) it writes -- the whole rows of a plane, the pairs of an
//               interleaved plane, or its U or its V bytes alone, of the SOURCE's size -- and lies inside (rows - 1) * pitch + row_bytes
//               of a plane the layout has;
//   form        the plan's wide flags, the scaled class's largest row bytes and source width are io_jobs.h's *_job_wide predicates and the
//               extents of its records.
// tests/test_enc_ingest_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/enc_ingest_check.cpp -o enc_ingest_check && ./enc_ingest_check
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "enc_ingest.h"

using namespace dsv2;
using namespace dsv2::enc_ingest;

namespace {

typedef unsigned long long U64;
constexpr U64 kFrameAt = 0x10000000ull, kSourceAt = 0x100000000ull, kPlaneApart = 0x40000000ull;

// ---- the sweep's axes -------------------------------------------------------------------------------------------------------------------
const int kFormats[6] = {DSV_SUBSAMP_444, DSV_SUBSAMP_422, DSV_SUBSAMP_420, DSV_SUBSAMP_411, DSV_SUBSAMP_410, DSV_SUBSAMP_UYVY}; // (UYVY: the YUV kinds alone)
const int kSizes[5][2] = {{16, 16}, {34, 18}, {66, 34}, {352, 288}, {1920, 1080}};
const int kOffsets[4] = {0, 1, 4, 16};
enum Pitch { TIGHT, PLUS_ONE, ROUNDED_256, kPitches };
const char *const kKindName[6] = {"packed", "planar", "semiplanar", "rgb4", "rgb3", "rgbp"};
enum Size { OWN, PLUS_PIXEL, THREE_HALVES, EIGHTFOLD };
struct Way { // a call, and what the caller says of the surface
    Call call;
    int shift; // the layout's scale value
    Size size; // of the picture in the surface, against the encoder's (a scale: what the scale makes of it)
    const char *name;
    Source::Route route() const { return shift ? Source::REDUCED : size != OWN ? Source::SIZED : Source::PLAIN; }
};
const Way kWays[12] = {{CALL_PLAIN, 0, OWN, "plain call"},
                       {CALL_SCALED, 0, OWN, "scaled call, no scale"},
                       {CALL_SCALED, 1, OWN, "scaled call, half"},
                       {CALL_SCALED, 2, OWN, "scaled call, quarter"},
                       {CALL_SCALED, 3, OWN, "scaled call, eighth"},
                       {CALL_SIZED, 0, OWN, "sized call, own size"},
                       {CALL_SIZED, 0, PLUS_PIXEL, "sized call, one column more"},
                       {CALL_SIZED, 0, THREE_HALVES, "sized call, 3 : 2"},
                       {CALL_SIZED, 0, EIGHTFOLD, "sized call, 8 : 1"},
                       {CALL_SIZED, 1, OWN, "sized call, half"},
                       {CALL_SIZED, 2, OWN, "sized call, quarter"},
                       {CALL_SIZED, 3, OWN, "sized call, eighth"}};

// ---- the two tables ---------------------------------------------------------------------------------------------------------------------
// acceptance: call x kind x route.  Three-byte and planar RGB are the plain call's alone; four-byte RGB is resampled only where both its
// resamplings keep D = a * c within 65535 (include/dsv2_hip.h); everything else the sweep holds is taken
enum Verdict { REFUSED, TAKEN, TAKEN_IF_D };
Verdict verdict(const Way &w, int kind)
{
    if (kind == Source::RGB3 || kind == Source::RGBP) {
        return w.call == CALL_PLAIN ? TAKEN : REFUSED;
    }
    return kind == Source::RGB4 && w.route() == Source::SIZED ? TAKEN_IF_D : TAKEN;
}
// counts: kind x route -> the one class a picture brings records of, and how many
struct CountRow {
    int kind, route, cl, n;
    const char *name;
    long hits;
};
CountRow g_counts[11] = {{Source::PLANAR, Source::PLAIN, SURF, 3, "planar, plain: 3 SurfaceJob", 0},
                         {Source::SEMI, Source::PLAIN, SURF, 2, "semiplanar, plain: 2 SurfaceJob", 0},
                         {Source::RGB4, Source::PLAIN, RGB, 1, "four-byte RGB, plain: 1 RgbJob", 0},
                         {Source::RGB3, Source::PLAIN, RGB3_PACKED, 1, "three-byte RGB, plain: 1 Rgb3Job, packed", 0},
                         {Source::RGBP, Source::PLAIN, RGB3_PLANAR, 1, "planar RGB, plain: 1 Rgb3Job, planar", 0},
                         {Source::PLANAR, Source::REDUCED, SCALED_SURF, 3, "planar, reduced: 3 ScaledSurfaceJob", 0},
                         {Source::SEMI, Source::REDUCED, SCALED_SURF, 2, "semiplanar, reduced: 2 ScaledSurfaceJob", 0},
                         {Source::RGB4, Source::REDUCED, SCALED_RGB, 1, "four-byte RGB, reduced: 1 ScaledRgbJob", 0},
                         {Source::PLANAR, Source::SIZED, SIZED_SURF, 3, "planar, sized: 3 SizedSurfaceJob", 0},
                         {Source::SEMI, Source::SIZED, SIZED_SURF, 3, "semiplanar, sized: 3 SizedSurfaceJob", 0},
                         {Source::RGB4, Source::SIZED, SIZED_RGB, 1, "four-byte RGB, sized: 1 SizedRgbJob", 0}};
long g_accept_hits[12][6][2]; // [way][kind][taken]

struct Case {
    int fmt, w, h, kind, way, offset, pitch_kind, layout, sw, sh;
    std::string name() const
    {
        char s[200];
        snprintf(s, sizeof s, "fmt=%#x %dx%d %s, %s: layout %#x, source %dx%d, offset=%d pitch=%d", fmt, w, h, kKindName[kind], kWays[way].name, layout, sw, sh,
                 offset, pitch_kind);
        return s;
    }
};
[[noreturn]] void fail(const Case &c, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "FAILED [%s]: ", c.name().c_str());
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}

// ---- footprints -------------------------------------------------------------------------------------------------------------------------
struct Foot { // `rows` rows `pitch` apart, each `count` bytes `step` apart from `base` on
    U64 base, pitch;
    long step, count;
    int rows;
    bool operator==(const Foot &o) const { return base == o.base && pitch == o.pitch && step == o.step && count == o.count && rows == o.rows; }
    U64 end() const { return base + (U64) (rows - 1) * pitch + (U64) ((count - 1) * step + 1); }
};
Foot foot(const void *p, U64 pitch, long step, long count, int rows) { return Foot{(U64) (uintptr_t) p, pitch, step, count, rows}; }
struct Access { // what one record reads and writes
    std::vector<Foot> reads, writes;
};
int cdiv(int v, int shift) { return (v + (1 << shift) - 1) >> shift; }
long gcd_of(long x, long y) { return y ? gcd_of(y, x % y) : x; }

// the footprints io_jobs.h documents, record type by record type
Access access_of(const SurfaceJob &j)
{
    Access a{{foot(j.src, j.pitch, 1, j.dst2 ? 2 * j.w : j.w, j.h)}, {foot(j.dst, (U64) j.dstride, 1, j.w, j.h)}};
    if (j.dst2) {
        a.writes.push_back(foot(j.dst2, (U64) j.dstride, 1, j.w, j.h));
    }
    return a;
}
template <class J> std::vector<Foot> yuv_writes(const J &j, int ow, int oh, int hs, int vs)
{
    const int cw = cdiv(ow, hs), ch = cdiv(oh, vs);
    return {foot(j.dst[0], (U64) j.ystride, 1, ow, oh), foot(j.dst[1], (U64) j.cstride, 1, cw, ch), foot(j.dst[2], (U64) j.cstride, 1, cw, ch)};
}
Access access_of(const RgbJob &j) { return Access{{foot(j.src, j.pitch, 1, 4L * j.w, j.h)}, yuv_writes(j, j.w, j.h, j.hs, j.vs)}; }
Access access_of(const Rgb3Job &j)
{
    Access a{{}, yuv_writes(j, j.w, j.h, j.hs, j.vs)};
    if (j.kind == kRgb3Planar) {
        for (int c = 0; c < 3; c++) {
            a.reads.push_back(foot(j.src[c], j.pitch[c], 1, j.w, j.h));
        }
    } else {
        a.reads.push_back(foot(j.src[0], j.pitch[0], 1, 3L * j.w, j.h));
    }
    return a;
}
Access access_of(const ScaledSurfaceJob &j)
{
    const int ow = cdiv(j.pw, j.shift), oh = cdiv(j.ph, j.shift);
    Access a{{foot(j.src, j.pitch, 1, j.dst2 ? 2 * j.pw : j.pw, j.ph)}, {foot(j.dst, (U64) j.dstride, 1, ow, oh)}};
    if (j.dst2) {
        a.writes.push_back(foot(j.dst2, (U64) j.dstride, 1, ow, oh));
    }
    return a;
}
Access access_of(const ScaledRgbJob &j)
{
    return Access{{foot(j.src, j.pitch, 1, 4L * j.sw, j.sh)}, yuv_writes(j, cdiv(j.sw, j.shift), cdiv(j.sh, j.shift), j.hs, j.vs)};
}
// (a sized record names its source plane's size through its ratio alone: pw = ow * a / b, ph = oh * c / d)
Access access_of(const SizedSurfaceJob &j)
{
    const long pw = (long) j.ow * j.q.a / j.q.b, ph = (long) j.oh * j.q.c / j.q.d;
    return Access{{foot(j.src + j.off, j.pitch, j.step, pw, (int) ph)}, {foot(j.dst, (U64) j.dstride, 1, j.ow, j.oh)}};
}
Access access_of(const SizedRgbJob &j, const Case &c)
{
    const long sw = (long) j.ow * j.ql.a / j.ql.b, sh = (long) j.oh * j.ql.c / j.ql.d;
    if ((long) j.cw * j.qc.a / j.qc.b != sw || (long) j.ch * j.qc.c / j.qc.d != sh) {
        fail(c, "the two ratios of a sized RGB record name two source sizes");
    }
    return Access{{foot(j.src, j.pitch, 1, 4 * sw, (int) sh)},
                  {foot(j.dst[0], (U64) j.ystride, 1, j.ow, j.oh), foot(j.dst[1], (U64) j.cstride, 1, j.cw, j.ch), foot(j.dst[2], (U64) j.cstride, 1, j.cw, j.ch)}};
}

// ---- the synthetic pictures -------------------------------------------------------------------------------------------------------------
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

struct SourcePlanes { // the caller's surface as include/dsv2_hip.h documents its kinds, restated: planes, row bytes and rows of a picture of sw x sh
    int n;
    U64 base[3], pitch[3];
    long row_bytes[3];
    int rows[3];
};
SourcePlanes source_planes(const Case &c)
{
    const int hs = DSV_FORMAT_H_SHIFT(c.fmt), vs = DSV_FORMAT_V_SHIFT(c.fmt), scw = cdiv(c.sw, hs), sch = cdiv(c.sh, vs);
    SourcePlanes s{};
    switch (c.kind) {
    case Source::PLANAR:
        s.n = 3, s.row_bytes[0] = c.sw, s.row_bytes[1] = s.row_bytes[2] = scw, s.rows[0] = c.sh, s.rows[1] = s.rows[2] = sch;
        break;
    case Source::SEMI:
        s.n = 2, s.row_bytes[0] = c.sw, s.row_bytes[1] = 2L * scw, s.rows[0] = c.sh, s.rows[1] = sch;
        break;
    case Source::RGBP:
        s.n = 3, s.row_bytes[0] = s.row_bytes[1] = s.row_bytes[2] = c.sw, s.rows[0] = s.rows[1] = s.rows[2] = c.sh;
        break;
    default:
        s.n = 1, s.row_bytes[0] = (c.kind == Source::RGB4 ? 4L : 3L) * c.sw, s.rows[0] = c.sh;
    }
    for (int p = 0; p < s.n; p++) {
        s.base[p] = kSourceAt + (U64) p * kPlaneApart + (U64) c.offset;
        s.pitch[p] = c.pitch_kind == TIGHT ? (U64) s.row_bytes[p] : c.pitch_kind == PLUS_ONE ? (U64) s.row_bytes[p] + 1 : ((U64) s.row_bytes[p] + 255) & ~255ull;
    }
    return s;
}

// what feeds the encoder's planes in `mask` (bit c: plane c) when ONE record writes them
std::vector<Foot> expected_reads(const Case &c, const SourcePlanes &s, int mask)
{
    const int hs = DSV_FORMAT_H_SHIFT(c.fmt), vs = DSV_FORMAT_V_SHIFT(c.fmt), scw = cdiv(c.sw, hs), sch = cdiv(c.sh, vs);
    if (c.kind == Source::PLANAR || c.kind == Source::SEMI) {
        if (mask == 1) {
            return {Foot{s.base[0], s.pitch[0], 1, c.sw, c.sh}};
        }
        if (c.kind == Source::PLANAR && (mask == 2 || mask == 4)) {
            const int p = mask == 2 ? 1 : 2;
            return {Foot{s.base[p], s.pitch[p], 1, scw, sch}};
        }
        if (c.kind == Source::SEMI && mask == 6) { // the pairs, whole
            return {Foot{s.base[1], s.pitch[1], 1, 2L * scw, sch}};
        }
        if (c.kind == Source::SEMI && (mask == 2 || mask == 4)) { // the U bytes, or the V bytes
            return {Foot{s.base[1] + (mask == 4 ? 1 : 0), s.pitch[1], 2, scw, sch}};
        }
    } else if (mask == 7) {
        std::vector<Foot> v;
        for (int p = 0; p < s.n; p++) {
            v.push_back(Foot{s.base[p], s.pitch[p], 1, s.row_bytes[p], c.sh});
        }
        return v;
    }
    fail(c, "one record writes the planes of mask %d, which nothing of this source feeds together", mask);
}

long g_cases = 0, g_taken = 0;

// every record of the plan, checked against the case; returns nothing: a miss ends the program
void check_plan(const Case &c, const DFrame &f, const SourcePlanes &s, const IngestPlan &p)
{
    const Way &way = kWays[c.way];
    // counts
    const CountRow *row = nullptr;
    for (CountRow &r : g_counts) {
        if (r.kind == c.kind && r.route == way.route()) {
            row = &r;
            r.hits++;
        }
    }
    if (!row) {
        fail(c, "a picture was taken that the table of counts does not know");
    }
    for (int cl = 0; cl < kClasses; cl++) {
        if (p.n[cl] != (cl == row->cl ? row->n : 0)) {
            fail(c, "%d records of class %d; the table says %d of class %d alone", p.n[cl], cl, row->n, row->cl);
        }
    }
    // the records' footprints, and the form facts restated from io_jobs.h's predicates
    std::vector<Access> acc;
    bool wide = true;
    int row_bytes = 0, rgb_sw = 0;
    for (int i = 0; i < row->n; i++) {
        switch (row->cl) {
        case SURF:
            acc.push_back(access_of(p.surf[i])), wide = wide && surface_job_wide(p.surf[i]);
            break;
        case RGB:
            acc.push_back(access_of(p.rgb[i])), wide = wide && rgb_job_wide(p.rgb[i]);
            break;
        case SCALED_SURF:
            acc.push_back(access_of(p.scaled_surf[i])), wide = wide && scaled_surface_job_wide(p.scaled_surf[i]);
            row_bytes = std::max(row_bytes, (int) acc.back().reads[0].count);
            if (p.scaled_surf[i].shift != way.shift) {
                fail(c, "a scaled record's shift is %d", p.scaled_surf[i].shift);
            }
            break;
        case SCALED_RGB:
            acc.push_back(access_of(p.scaled_rgb[i])), wide = wide && scaled_rgb_job_wide(p.scaled_rgb[i]);
            rgb_sw = p.scaled_rgb[i].sw;
            if (p.scaled_rgb[i].shift != way.shift) {
                fail(c, "a scaled RGB record's shift is %d", p.scaled_rgb[i].shift);
            }
            break;
        case SIZED_SURF:
            acc.push_back(access_of(p.sized_surf[i]));
            wide = wide && sized_job_wide(p.sized_surf[i], (size_t) (acc.back().reads[0].step * acc.back().reads[0].count)); // (the rows of the whole plane)
            break;
        case SIZED_RGB:
            acc.push_back(access_of(p.sized_rgb[i], c)), wide = wide && sized_rgb_job_wide(p.sized_rgb[i]);
            break;
        default:
            acc.push_back(access_of(p.rgb3[i])), wide = wide && rgb3_job_wide(p.rgb3[i]);
            if (p.rgb3[i].kind != row->cl - RGB3_PACKED) {
                fail(c, "an Rgb3Job of kind %d in class %d", p.rgb3[i].kind, row->cl);
            }
        }
    }
    for (int cl = 0; cl < kClasses; cl++) {
        if (p.wide[cl] != (cl == row->cl ? wide : true)) {
            fail(c, "form: class %d is planned %s; its records' predicates say otherwise", cl, p.wide[cl] ? "wide" : "general");
        }
    }
    if (p.scaled_row_bytes != row_bytes || p.scaled_rgb_sw != rgb_sw) {
        fail(c, "form: the scaled class's largest row is planned as %d bytes (the records': %d), the scaled RGB source as %d wide (%d)", p.scaled_row_bytes,
             row_bytes, p.scaled_rgb_sw, rgb_sw);
    }
    // coverage and reads
    int written[3] = {0, 0, 0};
    for (const Access &a : acc) {
        int mask = 0;
        for (const Foot &w : a.writes) {
            int at = -1;
            for (int pl = 0; pl < 3; pl++) {
                if (w == foot(f.p[pl].data, (U64) f.p[pl].stride, 1, f.p[pl].w, f.p[pl].h) && !(mask & (1 << pl))) {
                    at = pl;
                    break;
                }
            }
            if (at < 0) {
                fail(c, "coverage: a record writes %ld x %d bytes at %#llx, pitch %llu: not the visible samples of a source plane of the encoder", w.count, w.rows,
                     w.base, w.pitch);
            }
            mask |= 1 << at;
            written[at]++;
        }
        const std::vector<Foot> want = expected_reads(c, s, mask);
        if (!(a.reads == want)) {
            const Foot &g = a.reads[0], &e = want[0];
            fail(c, "reads: the record that writes the planes of mask %d reads %ld bytes %ld apart in %d rows from %#llx, pitch %llu; what feeds them is %ld bytes "
                    "%ld apart in %d rows from %#llx, pitch %llu", mask, g.count, g.step, g.rows, g.base, g.pitch, e.count, e.step, e.rows, e.base, e.pitch);
        }
        for (const Foot &r : a.reads) {
            bool inside = false;
            for (int pl = 0; pl < s.n; pl++) {
                inside = inside || (r.base >= s.base[pl] && r.pitch == s.pitch[pl] && r.end() <= s.base[pl] + (U64) (s.rows[pl] - 1) * s.pitch[pl] + (U64) s.row_bytes[pl]);
            }
            if (!inside) {
                fail(c, "reads: %#llx .. %#llx lies in no plane the layout has", r.base, r.end());
            }
        }
    }
    for (int pl = 0; pl < 3; pl++) {
        if (written[pl] != 1) {
            fail(c, "coverage: plane %d of the encoder is written by %d records", pl, written[pl]);
        }
    }
}

// both resamplings of a four-byte RGB source keep D within 65535 (restated: own gcd)
bool rgb_d_fits(const Case &c)
{
    const int cw = cdiv(c.w, DSV_FORMAT_H_SHIFT(c.fmt)), ch = cdiv(c.h, DSV_FORMAT_V_SHIFT(c.fmt));
    const long Dl = (c.sw / gcd_of(c.sw, c.w)) * (c.sh / gcd_of(c.sh, c.h)), Dc = (c.sw / gcd_of(c.sw, cw)) * (c.sh / gcd_of(c.sh, ch));
    return Dl <= 65535 && Dc <= 65535;
}

void run_case(Case c, long turn)
{
    const Way &way = kWays[c.way];
    const int s = way.shift;
    // the picture in the surface: a scale's source has an odd width that still reduces to the encoder's, and its exact height
    c.sw = s ? (c.w << s) - 1 : way.size == PLUS_PIXEL ? c.w + 1 : way.size == THREE_HALVES ? c.w * 3 / 2 : way.size == EIGHTFOLD ? 8 * c.w : c.w;
    c.sh = s ? c.h << s : way.size == THREE_HALVES ? c.h * 3 / 2 : way.size == EIGHTFOLD ? 8 * c.h : c.h;
    const int csc = (int) ((turn >> 1) & 3) << 8;
    c.layout = c.kind == Source::PLANAR ? DSV2HIP_SURFACE_PLANAR
               : c.kind == Source::SEMI ? DSV2HIP_SURFACE_SEMIPLANAR
               : c.kind == Source::RGBP ? DSV2HIP_SURFACE_RGBP | csc
                                        : ((c.kind == Source::RGB4 ? DSV2HIP_SURFACE_BGRA : DSV2HIP_SURFACE_BGR) + (int) (turn & 1)) | csc;
    c.layout |= s << 12;
    if (c.layout == 0x1010) { // (the value the grammar holds back)
        c.layout |= DSV2HIP_CSC_BT709;
    }
    const DFrame f = fake_frame(kFrameAt, c.fmt, c.w, c.h);
    const SourcePlanes sp = source_planes(c);
    dsv2hip_surface sf{};
    sf.layout = c.layout;
    for (int p = 0; p < sp.n; p++) {
        sf.plane[p] = (const void *) (uintptr_t) sp.base[p], sf.pitch[p] = (size_t) sp.pitch[p];
    }
    Source src;
    const bool taken = accept(way.call, c.w, c.h, c.fmt, false, sf, c.sw, c.sh, &src);
    const Verdict v = verdict(way, c.kind);
    if (taken != (v == TAKEN || (v == TAKEN_IF_D && rgb_d_fits(c)))) {
        fail(c, "acceptance: %s, the table says otherwise", taken ? "taken" : "refused");
    }
    Source never;
    if (accept(way.call, c.w, c.h, c.fmt, true, sf, c.sw, c.sh, &never)) {
        fail(c, "acceptance: taken by an encoder with UYVY input on");
    }
    g_cases++;
    g_accept_hits[c.way][c.kind][taken]++;
    if (taken) {
        g_taken++;
        if (src.kind != c.kind || src.route != way.route()) {
            fail(c, "the source record says kind %d, route %d", (int) src.kind, (int) src.route);
        }
        check_plan(c, f, sp, plan_ingest(f, src));
    }
}

} // namespace

int main()
{
    long turn = 0;
    for (int fi = 0; fi < 6; fi++) {
        for (const auto &size : kSizes) {
            for (int kind = Source::PLANAR; kind <= Source::RGBP; kind++) {
                if (kFormats[fi] == DSV_SUBSAMP_UYVY && kind != Source::PLANAR && kind != Source::SEMI) {
                    continue;
                }
                for (int way = 0; way < 12; way++) {
                    for (int offset : kOffsets) {
                        for (int pitch_kind = 0; pitch_kind < kPitches; pitch_kind++, turn++) {
                            run_case(Case{kFormats[fi], size[0], size[1], kind, way, offset, pitch_kind, 0, 0, 0}, turn);
                        }
                    }
                }
            }
        }
    }
    printf("enc_ingest_check: %ld cases, %ld of them taken: acceptance, counts, coverage, reads and form hold\n", g_cases, g_taken);
    for (const CountRow &r : g_counts) {
        printf("  %6ld cases  %s\n", r.hits, r.name);
    }
    for (int way = 0; way < 12; way++) {
        for (int kind = Source::PLANAR; kind <= Source::RGBP; kind++) {
            const long *h = g_accept_hits[way][kind];
            const Verdict v = verdict(kWays[way], kind);
            printf("  %6ld cases  %s, %s: %s\n", h[0] + h[1], kWays[way].name, kKindName[kind],
                   v == REFUSED ? "refused" : v == TAKEN ? "taken" : "taken where both resamplings keep D within 65535");
            if (v == TAKEN_IF_D) {
                printf("                (%ld taken, %ld refused)\n", h[1], h[0]);
            }
        }
    }
    return 0;
}
