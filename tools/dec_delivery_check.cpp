// dec_delivery_check.cpp -- the decoder's delivery planner (csrc/dec_delivery.h) swept on the CPU: chroma format x picture size x target
// kind x scale x out420p x postsharp x draw_info x pointer offset x pitch, over FAKE addresses -- the reconstruction, the two staging
// areas and the target are disjoint ranges of one synthetic address space, and nothing is ever dereferenced.  Meant to be built with
// AddressSanitizer and UndefinedBehaviorSanitizer (the planner is handed no staging area it says it does not need: a look at one faults).
// For every case the program works out, by its own interval arithmetic over the footprints io_jobs.h documents for each job record,
//   coverage  the bytes written by the jobs whose destination is the target are exactly the visible rows of the target's planes as
//             dsv2hip_dec_surface_dims documents them (a pinned frame: its planes' rows, or under the whole-frame copy its block), no
//             byte twice, nothing else outside the staging areas -- where a row may be written up to its stride;
//   order     every byte read from a staging area was written by a job of a strictly earlier launch class (whole-frame copy, 4:2:0
//             conversion, egress, overlay, sharpening in place, reduction, chroma interleave, RGB conversion); overlay and sharpening touch
//             a staged plane only between the egress that fills it and the reduction / conversion that reads it;
//   form      the plan's wide / sharp / conv / rows facts are those of io_jobs.h's *_job_wide predicates applied to its jobs;
//   counts    the job counts are those of the table below (restated as data), every row of which some case must hit;
//   sources   the reconstruction is never written, and the luma is read from it -- or from the staged copy if and only if the picture
//             is sharpened or drawn on and leaves reduced or as RGB.
// tests/test_dec_delivery_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/dec_delivery_check.cpp -o dec_delivery_check && ./dec_delivery_check
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dec_delivery.h"

using namespace dsv2;
using namespace dsv2::delivery;

namespace {

typedef unsigned long long U64;
constexpr U64 kReconAt = 0x10000000ull, kLumaAt = 0x20000000ull, kScaledAt = 0x30000000ull, kTargetAt = 0x40000000ull, kPlaneApart = 0x08000000ull;
enum Region { NOWHERE, RECON, LUMA, SCALED, TARGET };
enum Class { COPY = 1, TO420, EGRESS, OVERLAY, SHARPEN, SCALE, UV, RGBOUT }; // the launch order of a round
enum Kind { FRAME, PLANAR, SEMI, RGB };

struct Case {
    int fmt, w, h, kind, shift;
    bool out420p, sharp;
    int draw, offset, pitch_kind;
    bool conv() const { return out420p && fmt != DSV_SUBSAMP_420; }
    bool sharp_out() const { return sharp && !draw; }
    bool device() const { return kind != FRAME; }
    bool via_staging() const { return device() && (shift || kind == RGB); } // the "scaled or RGB target" of the rules
    bool staged_luma() const { return via_staging() && (sharp || draw); }
    std::string name() const
    {
        static const char *kinds[] = {"frame", "planar", "semiplanar", "rgb"};
        char s[160];
        snprintf(s, sizeof s, "fmt=%#x %dx%d %s shift=%d out420p=%d sharp=%d draw=%d offset=%d pitch=%d", fmt, w, h, kinds[kind], shift, (int) out420p,
                 (int) sharp, draw, offset, pitch_kind);
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

// ---- interval arithmetic ----------------------------------------------------------------------------------------------------------------
struct Span {
    U64 a, b; // [a, b)
};
struct Rows { // `rows` rows of `bytes` bytes, `pitch` apart
    U64 base;
    long pitch, bytes;
    int rows;
    U64 last() const { return base + (U64) (rows - 1) * (U64) pitch + (U64) bytes; }
};
Rows rows_of(const void *p, long pitch, long bytes, int rows) { return Rows{(U64) (uintptr_t) p, pitch, bytes, rows}; }
Rows rows_of(const DPlane &p) { return rows_of(p.data, p.stride, p.w, p.h); }
void add_spans(std::vector<Span> &v, const Rows &r)
{
    for (int y = 0; y < r.rows; y++) {
        v.push_back(Span{r.base + (U64) y * (U64) r.pitch, r.base + (U64) y * (U64) r.pitch + (U64) r.bytes});
    }
}
// sorted, touching spans merged; *twice: some byte lies in two of them
std::vector<Span> normal(std::vector<Span> v, bool *twice = nullptr)
{
    std::sort(v.begin(), v.end(), [](const Span &x, const Span &y) { return x.a < y.a; });
    std::vector<Span> out;
    for (const Span &s : v) {
        if (s.a == s.b) {
            continue;
        }
        if (!out.empty() && s.a < out.back().b && twice) {
            *twice = true;
        }
        if (!out.empty() && s.a <= out.back().b) {
            out.back().b = std::max(out.back().b, s.b);
        } else {
            out.push_back(s);
        }
    }
    return out;
}
bool covers(const std::vector<Span> &norm, const Rows &r)
{
    for (int y = 0; y < r.rows; y++) {
        const U64 a = r.base + (U64) y * (U64) r.pitch, b = a + (U64) r.bytes;
        auto it = std::upper_bound(norm.begin(), norm.end(), a, [](U64 v, const Span &s) { return v < s.a; });
        if (it == norm.begin() || (it - 1)->b < b) {
            return false;
        }
    }
    return true;
}

// ---- the synthetic pictures -------------------------------------------------------------------------------------------------------------
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

struct World { // one case's address space
    DFrame recon, frame; // frame: the pinned target
    DPlane luma, scaled[3];
    Rows want[3]; // the target's planes as documented: base, pitch, row bytes, rows
    int nplanes = 0;
    OutTarget target;
};

long pitch_of(long rb, int pitch_kind) { return pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + 1 : (rb + 255) / 256 * 256; }

World make_world(const Case &c)
{
    World W;
    W.recon = fake_frame(kReconAt, c.fmt, c.w, c.h);
    // the decoder's staging areas (decoder.cpp: DecImpl): the luma w x h, the scaled picture sized for half size; 16-byte strides
    W.luma = DPlane{(uint8_t *) (uintptr_t) kLumaAt, (c.w + 15) & ~15, c.w, c.h};
    U64 at = kScaledAt;
    for (int k = 0; k < 3; k++) {
        const int sw = (W.recon.p[k].w + 1) >> 1, sh = (W.recon.p[k].h + 1) >> 1;
        W.scaled[k] = DPlane{(uint8_t *) (uintptr_t) at, (sw + 15) & ~15, sw, sh};
        at += (U64) W.scaled[k].stride * (U64) sh;
    }
    const int out_format = c.out420p ? DSV_SUBSAMP_420 : c.fmt;
    if (c.kind == FRAME) {
        W.frame = fake_frame(kTargetAt, out_format, c.w, c.h);
        DSV_FRAME f = {};
        f.alloc = W.frame.alloc;
        for (int k = 0; k < 3; k++) {
            f.planes[k].data = W.frame.p[k].data, f.planes[k].stride = W.frame.p[k].stride;
            f.planes[k].w = W.frame.p[k].w, f.planes[k].h = W.frame.p[k].h;
            W.want[k] = rows_of(W.frame.p[k]);
        }
        W.nplanes = 3;
        W.target = target_frame(&f);
        return W;
    }
    // include/dsv2_hip.h at dsv2hip_dec_surface_dims: dsv_mk_frame's plane sizes for ceil(w / n) x ceil(h / n); RGB: one plane of 4 bytes a pixel
    const int rw = cdiv(c.w, c.shift), rh = cdiv(c.h, c.shift);
    const int cw = cdiv(rw, DSV_FORMAT_H_SHIFT(out_format)), ch = cdiv(rh, DSV_FORMAT_V_SHIFT(out_format));
    size_t rb[3] = {(size_t) rw, (size_t) cw, (size_t) cw};
    int rows[3] = {rh, ch, ch};
    W.nplanes = 3;
    if (c.kind == SEMI) {
        rb[1] = 2 * (size_t) cw, rb[2] = 0, rows[2] = 0, W.nplanes = 2;
    } else if (c.kind == RGB) {
        rb[0] = 4 * (size_t) rw, rb[1] = rb[2] = 0, rows[1] = rows[2] = 0, W.nplanes = 1;
    }
    if (c.kind == PLANAR && c.shift == 0 && c.pitch_kind == 0) { // the packed buffer of dsv2hip_dec_batch_device
        U64 p = kTargetAt + 256 + (U64) c.offset;
        W.target = target_packed((void *) (uintptr_t) p, rb, rows);
        for (int k = 0; k < 3; k++) {
            W.want[k] = Rows{p, (long) rb[k], (long) rb[k], rows[k]};
            p += rb[k] * (U64) rows[k];
        }
        return W;
    }
    dsv2hip_out_surface sf = {};
    const int base = c.kind == PLANAR ? DSV2HIP_SURFACE_PLANAR : c.kind == SEMI ? DSV2HIP_SURFACE_SEMIPLANAR
                   : (c.w + c.offset) & 1 ? (DSV2HIP_SURFACE_RGBA | DSV2HIP_CSC_FULL_RANGE) : (DSV2HIP_SURFACE_BGRA | DSV2HIP_CSC_BT709);
    sf.layout = base | (c.shift << 12);
    for (int k = 0; k < W.nplanes; k++) {
        W.want[k] = Rows{kTargetAt + (U64) k * kPlaneApart + 256 + (U64) c.offset, pitch_of((long) rb[k], c.pitch_kind), (long) rb[k], rows[k]};
        sf.plane[k] = (void *) (uintptr_t) W.want[k].base;
        sf.pitch[k] = (size_t) W.want[k].pitch;
        sf.cap[k] = (size_t) (W.want[k].last() - W.want[k].base);
    }
    if (!target_surface(sf, rb, rows, &W.target)) {
        fail(c, "target_surface refused a surface that holds the picture exactly");
    }
    sf.cap[W.nplanes - 1]--;
    OutTarget none;
    if (target_surface(sf, rb, rows, &none)) {
        fail(c, "target_surface accepted a plane one byte short");
    }
    return W;
}

Region region_of(const Case &c, const World &W, const Rows &r)
{
    auto inside = [&](U64 a, U64 b) { return r.rows > 0 && r.base >= a && r.last() <= b; };
    if (inside(kReconAt, kReconAt + W.recon.bytes + 4096)) {
        return RECON;
    }
    if (inside(kLumaAt, kLumaAt + (U64) W.luma.stride * (U64) W.luma.h)) {
        return LUMA;
    }
    if (inside(kScaledAt, (U64) (uintptr_t) W.scaled[2].data + (U64) W.scaled[2].stride * (U64) W.scaled[2].h)) {
        return SCALED;
    }
    if (c.kind == FRAME) {
        return inside(kTargetAt, kTargetAt + W.frame.bytes) ? TARGET : NOWHERE;
    }
    for (int k = 0; k < W.nplanes; k++) {
        if (inside(W.want[k].base, W.want[k].last())) {
            return TARGET;
        }
    }
    return NOWHERE;
}

// ---- a plan's jobs with the footprints io_jobs.h documents ----------------------------------------------------------------------------------
struct Access {
    int cls;
    const char *what;
    std::vector<Rows> reads;
    Rows write;
};

std::vector<Access> accesses_of(const DeliveryPlan &p)
{
    std::vector<Access> v;
    for (int i = 0; i < p.n_copy; i++) {
        const CopyJob &j = p.copy[i];
        v.push_back(Access{COPY, "whole-frame copy", {rows_of(j.src, (long) j.bytes, (long) j.bytes, 1)}, rows_of(j.dst, (long) j.bytes, (long) j.bytes, 1)});
    }
    for (int i = 0; i < p.n_to420; i++) {
        v.push_back(Access{TO420, "4:2:0 conversion", {rows_of(p.to420[i].src)}, rows_of(p.to420[i].dst)});
    }
    for (int i = 0; i < p.n_eg; i++) {
        const EgressJob &j = p.eg[i];
        v.push_back(Access{EGRESS, "egress", {rows_of(j.src)}, rows_of(j.dst, j.dstride, j.src.w, j.src.h)});
    }
    for (int i = 0; i < p.n_overlay; i++) {
        v.push_back(Access{OVERLAY, "overlay", {}, rows_of(p.overlay[i])});
        if (p.sharpen_overlaid) {
            v.push_back(Access{SHARPEN, "sharpening in place", {}, rows_of(p.overlay[i])});
        }
    }
    for (int i = 0; i < p.n_scl; i++) {
        const ScaleOutJob &j = p.scl[i];
        v.push_back(Access{SCALE, "reduction", {rows_of(j.src, j.sstride, j.pw, j.ph)}, rows_of(j.dst, j.dpitch, cdiv(j.pw, j.shift), cdiv(j.ph, j.shift))});
    }
    for (int i = 0; i < p.n_uv; i++) {
        const UvEgressJob &j = p.uv[i];
        v.push_back(Access{UV, "chroma interleave", {rows_of(j.su, j.sstride, j.sw, j.sh), rows_of(j.sv, j.sstride, j.sw, j.sh)},
                           rows_of(j.dst, j.dpitch, 2 * (long) j.cw, j.ch)});
    }
    for (int i = 0; i < p.n_rgb; i++) {
        const RgbOutJob &j = p.rgb[i];
        const int cw = cdiv(j.w, j.hs), ch = cdiv(j.h, j.vs);
        v.push_back(Access{RGBOUT, "RGB conversion", {rows_of(j.sy, j.ystride, j.w, j.h), rows_of(j.su, j.cstride, cw, ch), rows_of(j.sv, j.cstride, cw, ch)},
                           rows_of(j.dst[0], j.dpitch[0], 4 * (long) j.w, j.h)});
    }
    return v;
}

// ---- the table of DESIGN 5.15, as data --------------------------------------------------------------------------------------------------
struct Counts {
    int copy = 0, to420 = 0, eg = 0, scl = 0, uv = 0, rgb = 0, overlay = 0, sharpen = 0;
    int total() const { return copy + to420 + eg + scl + uv + rgb + overlay + sharpen; }
};
bool per_plane(const Case &c) { return !c.via_staging() && !(c.kind == FRAME && !c.conv() && !c.sharp_out()); }
int planes_to420(const Case &c) // planes of the per-plane case that go through the 4:2:0 conversion
{
    int n = 0;
    for (int k = 0; k < 3; k++) {
        n += !(k && c.kind == SEMI) && c.conv() && (k || (c.kind == FRAME && !c.sharp_out()));
    }
    return n;
}
struct TableRow {
    const char *name;
    void (*add)(const Case &c, Counts &n); // what the row contributes to a case's counts (nothing: the row does not apply)
    long hits;
};
TableRow g_table[] = {
    {"device target, shift > 0, sharp or draw: luma staged through one egress job", [](const Case &c, Counts &n) { n.eg += c.device() && c.shift && c.staged_luma(); }, 0},
    {"device target, shift > 0: three scale jobs", [](const Case &c, Counts &n) { n.scl += c.device() && c.shift ? 3 : 0; }, 0},
    {"semiplanar, shift > 0: one uv job on the reduced geometry", [](const Case &c, Counts &n) { n.uv += c.kind == SEMI && c.shift; }, 0},
    {"RGB, shift > 0: one rgb job on the reduced geometry", [](const Case &c, Counts &n) { n.rgb += c.kind == RGB && c.shift; }, 0},
    {"RGB, shift 0, sharp or draw: luma staged through one egress job", [](const Case &c, Counts &n) { n.eg += c.kind == RGB && !c.shift && c.staged_luma(); }, 0},
    {"RGB, shift 0: one rgb job", [](const Case &c, Counts &n) { n.rgb += c.kind == RGB && !c.shift; }, 0},
    {"pinned frame, not converted, not sharpened on the way: one whole-frame copy",
     [](const Case &c, Counts &n) { n.copy += c.kind == FRAME && !c.conv() && !c.sharp_out(); }, 0},
    {"per plane, semiplanar chroma: one uv job for both planes", [](const Case &c, Counts &n) { n.uv += per_plane(c) && c.kind == SEMI; }, 0},
    {"per plane, converted chroma (and the luma of a pinned frame): to420 jobs", [](const Case &c, Counts &n) { n.to420 += per_plane(c) ? planes_to420(c) : 0; }, 0},
    {"per plane, otherwise: egress jobs", [](const Case &c, Counts &n) { n.eg += per_plane(c) ? (c.kind == SEMI ? 1 : 3) - planes_to420(c) : 0; }, 0},
    {"draw_info: overlay on the delivered or the staged luma", [](const Case &c, Counts &n) { n.overlay += c.draw != 0; }, 0},
    {"draw_info and postsharp: that plane sharpened in place", [](const Case &c, Counts &n) { n.sharpen += c.draw && c.sharp; }, 0},
};

Counts expected_counts(const Case &c)
{
    Counts n;
    for (TableRow &row : g_table) {
        const int before = n.total();
        row.add(c, n);
        row.hits += n.total() > before;
    }
    return n;
}

// ---- one case ---------------------------------------------------------------------------------------------------------------------------
long g_cases = 0;

void check(const Case &c)
{
    const World W = make_world(c);
    const int out_format = c.out420p ? DSV_SUBSAMP_420 : c.fmt;
    static const DPlane none = {nullptr, 0, 0, 0};
    if (needs_staged_luma(W.target, c.sharp, c.draw) != c.staged_luma() || needs_staged_scaled(W.target) != (c.device() && c.shift && c.kind != PLANAR)) {
        fail(c, "the staging predicates disagree with the rules");
    }
    const DeliveryPlan p = plan_delivery(W.recon, out_format, W.target, c.sharp, c.draw, c.staged_luma() ? W.luma : none,
                                         needs_staged_scaled(W.target) ? W.scaled : nullptr);
    g_cases++;
    // counts, and what the table says of the jobs' modes and flags
    const Counts n = expected_counts(c);
    if (p.n_copy != n.copy || p.n_to420 != n.to420 || p.n_eg != n.eg || p.n_scl != n.scl || p.n_uv != n.uv || p.n_rgb != n.rgb || p.n_overlay != n.overlay ||
        p.sharpen_overlaid != (n.sharpen != 0)) {
        fail(c, "jobs copy %d to420 %d egress %d scale %d uv %d rgb %d overlay %d sharpen %d, the table says %d %d %d %d %d %d %d %d", p.n_copy, p.n_to420,
             p.n_eg, p.n_scl, p.n_uv, p.n_rgb, p.n_overlay, (int) p.sharpen_overlaid, n.copy, n.to420, n.eg, n.scl, n.uv, n.rgb, n.overlay, n.sharpen);
    }
    const int hs = DSV_FORMAT_H_SHIFT(c.fmt), vs = DSV_FORMAT_V_SHIFT(c.fmt);
    const int mode420 = (hs == 0 && vs == 0) ? 1 : (hs == 1 && vs == 0) ? 2 : (hs == 2 && vs == 0) ? 3 : 4;
    for (int i = 0; i < p.n_eg; i++) {
        const bool luma = p.eg[i].src.data == W.recon.p[0].data;
        if ((p.eg[i].sharp != 0) != (luma && c.sharp_out())) {
            fail(c, "egress job %d sharpens = %d", i, p.eg[i].sharp);
        }
    }
    for (int i = 0; i < p.n_uv; i++) {
        if (p.uv[i].mode != (c.conv() && !c.shift ? mode420 : 0)) {
            fail(c, "uv job in mode %d", p.uv[i].mode);
        }
    }
    for (int i = 0; i < p.n_to420; i++) {
        const bool luma = p.to420[i].src.data == W.recon.p[0].data;
        if (p.to420[i].mode != (luma ? 0 : mode420)) {
            fail(c, "to420 job %d in mode %d", i, p.to420[i].mode);
        }
    }
    for (int i = 0; i < p.n_scl; i++) {
        if (p.scl[i].shift != c.shift) {
            fail(c, "scale job %d has shift %d", i, p.scl[i].shift);
        }
    }
    for (int i = 0; i < p.n_rgb; i++) {
        const RgbOutJob &j = p.rgb[i];
        const bool bgra = ((c.w + c.offset) & 1) == 0;
        if (j.layout != kRgbOutPacked || j.hs != hs || j.vs != vs || (j.bgra != 0) != bgra || j.csc.ky != (bgra ? 298 : 256) || j.w != cdiv(c.w, c.shift) || j.h != cdiv(c.h, c.shift)) {
            fail(c, "rgb job: hs %d vs %d bgra %d ky %d %dx%d", j.hs, j.vs, j.bgra, j.csc.ky, j.w, j.h);
        }
    }
    // sources and destinations by region
    const std::vector<Access> acc = accesses_of(p);
    const Rows recon_luma = rows_of(W.recon.alloc + W.recon.plane_off[0], (long) W.recon.plane_len[0], (long) W.recon.plane_len[0], 1);
    const std::vector<Span> recon_luma_span = {Span{recon_luma.base, recon_luma.last()}};
    std::vector<Span> terminal, early_terminal;
    for (const Access &a : acc) {
        for (const Rows &r : a.reads) {
            const Region g = region_of(c, W, r);
            if (g != RECON && g != LUMA && g != SCALED) {
                fail(c, "%s reads %#llx, which is neither the reconstruction nor a staging area", a.what, r.base);
            }
            if (g == LUMA && !c.staged_luma()) {
                fail(c, "%s reads the staged luma of a picture that has none", a.what);
            }
            if (c.staged_luma() && a.cls != EGRESS && covers(recon_luma_span, r)) {
                fail(c, "%s reads the reconstruction's luma where the staged copy holds the picture's", a.what);
            }
        }
        const Region g = region_of(c, W, a.write);
        if (g != TARGET && g != LUMA && g != SCALED) {
            fail(c, "%s writes %#llx: %s", a.what, a.write.base, g == RECON ? "the reconstruction" : "outside everything");
        }
        if (g == TARGET && a.cls != OVERLAY && a.cls != SHARPEN) {
            add_spans(terminal, a.write);
            if (a.cls < OVERLAY) {
                add_spans(early_terminal, a.write);
            }
        }
        if (g != TARGET) { // a staging plane: from its origin, rows up to its stride, no more rows than it has
            const DPlane *pl = a.write.base == kLumaAt ? &W.luma : nullptr;
            for (int k = 0; k < 3; k++) {
                pl = a.write.base == (U64) (uintptr_t) W.scaled[k].data ? &W.scaled[k] : pl;
            }
            if (!pl || a.write.pitch != pl->stride || a.write.bytes > pl->stride || a.write.rows > pl->h) {
                fail(c, "%s writes %d rows of %ld bytes, %ld apart, at %#llx: no staging plane holds them", a.what, a.write.rows, a.write.bytes, a.write.pitch,
                     a.write.base);
            }
        }
    }
    // coverage
    std::vector<Span> want;
    if (c.kind == FRAME && n.copy) {
        want.push_back(Span{kTargetAt, kTargetAt + W.frame.bytes});
    } else {
        for (int k = 0; k < W.nplanes; k++) {
            add_spans(want, W.want[k]);
        }
    }
    bool twice = false;
    const std::vector<Span> got = normal(terminal, &twice), exact = normal(want);
    if (twice) {
        fail(c, "a byte of the target is written twice");
    }
    if (got.size() != exact.size() || !std::equal(got.begin(), got.end(), exact.begin(), [](const Span &x, const Span &y) { return x.a == y.a && x.b == y.b; })) {
        size_t i = 0;
        while (i < got.size() && i < exact.size() && got[i].a == exact[i].a && got[i].b == exact[i].b) {
            i++;
        }
        fail(c, "the target's bytes written differ from its visible rows at span %zu: written [%#llx, %#llx), rows [%#llx, %#llx)", i,
             i < got.size() ? got[i].a : 0, i < got.size() ? got[i].b : 0, i < exact.size() ? exact[i].a : 0, i < exact.size() ? exact[i].b : 0);
    }
    // order
    const std::vector<Span> early = normal(early_terminal);
    for (const Access &a : acc) {
        for (const Rows &r : a.reads) {
            if (region_of(c, W, r) == RECON) {
                continue;
            }
            std::vector<Span> before;
            for (const Access &b : acc) {
                if (b.cls < a.cls && b.cls != OVERLAY && b.cls != SHARPEN && region_of(c, W, b.write) != TARGET) {
                    add_spans(before, b.write);
                }
            }
            if (!covers(normal(before), r)) {
                fail(c, "%s reads staged bytes at %#llx that no earlier launch wrote", a.what, r.base);
            }
        }
        if (a.cls == OVERLAY || a.cls == SHARPEN) {
            if (region_of(c, W, a.write) == TARGET) { // the delivered luma plane, whole, filled before the overlay
                const Rows &y = W.want[0];
                if (c.via_staging() || a.write.base != y.base || a.write.pitch != y.pitch || a.write.bytes != y.bytes || a.write.rows != y.rows ||
                    !covers(early, a.write)) {
                    fail(c, "the %s is not on the delivered luma plane as an earlier launch filled it", a.what);
                }
            } else { // the staged luma: behind the egress that fills it, in front of the job that reads it
                bool filled = false, read_later = false;
                for (const Access &b : acc) {
                    filled = filled || (b.cls == EGRESS && b.write.base == a.write.base && b.write.bytes == a.write.bytes && b.write.rows == a.write.rows);
                    for (const Rows &r : b.reads) {
                        read_later = read_later || (b.cls > SHARPEN && r.base == a.write.base && r.bytes == a.write.bytes && r.rows == a.write.rows);
                    }
                }
                if (!c.staged_luma() || a.write.base != kLumaAt || !filled || !read_later) {
                    fail(c, "the %s touches a staged plane that is not filled before it and read behind it", a.what);
                }
            }
        }
    }
    // form: io_jobs.h's predicates over the jobs
    bool eg_wide = true, eg_sharp = false, scl_wide = true, uv_wide = true, uv_conv = false, rgb_wide = true;
    int scl_rows = 0, uv_rows = 0;
    for (int i = 0; i < p.n_eg; i++) {
        eg_wide = eg_wide && egress_job_wide(p.eg[i], p.eg[i].src.w);
        eg_sharp = eg_sharp || p.eg[i].sharp;
    }
    for (int i = 0; i < p.n_scl; i++) {
        const Rows w = rows_of(p.scl[i].dst, p.scl[i].dpitch, cdiv(p.scl[i].pw, c.shift), cdiv(p.scl[i].ph, c.shift));
        scl_wide = scl_wide && scale_job_wide(p.scl[i], region_of(c, W, w) == SCALED ? p.scl[i].dpitch : (int) w.bytes);
        scl_rows = std::max(scl_rows, w.rows);
    }
    for (int i = 0; i < p.n_uv; i++) {
        uv_wide = uv_wide && uv_job_wide(p.uv[i]);
        uv_conv = uv_conv || p.uv[i].mode != 0;
        uv_rows = std::max(uv_rows, p.uv[i].ch);
    }
    for (int i = 0; i < p.n_rgb; i++) {
        rgb_wide = rgb_wide && rgb_out_job_wide(p.rgb[i]);
    }
    if (p.eg_wide != eg_wide || p.eg_sharp != eg_sharp || p.scl_wide != scl_wide || p.scl_rows != scl_rows || p.uv_wide != uv_wide || p.uv_conv != uv_conv ||
        p.uv_rows != uv_rows || p.rgb_wide != rgb_wide) {
        fail(c, "the plan's facts (eg wide %d sharp %d, scale wide %d rows %d, uv wide %d conv %d rows %d, rgb wide %d) are not its jobs' (%d %d, %d %d, %d %d %d, %d)",
             (int) p.eg_wide, (int) p.eg_sharp, (int) p.scl_wide, p.scl_rows, (int) p.uv_wide, (int) p.uv_conv, p.uv_rows, (int) p.rgb_wide, (int) eg_wide,
             (int) eg_sharp, (int) scl_wide, scl_rows, (int) uv_wide, (int) uv_conv, uv_rows, (int) rgb_wide);
    }
    if (c.staged_luma() && p.eg_wide != (c.w % 16 == 0)) { // (16-byte aligned origin and stride: the width decides)
        fail(c, "staged luma: egress wide = %d at width %d", (int) p.eg_wide, c.w);
    }
}

} // namespace

int main()
{
    static const int formats[] = {DSV_SUBSAMP_444, DSV_SUBSAMP_422, DSV_SUBSAMP_420, DSV_SUBSAMP_411, DSV_SUBSAMP_410};
    static const int sizes[][2] = {{16, 16}, {34, 18}, {38, 22}, {66, 34}, {352, 288}, {1920, 1080}};
    static const int offsets[] = {0, 1, 16};
    for (int fmt : formats) {
        for (const int *wh : sizes) {
            for (int kind = FRAME; kind <= RGB; kind++) {
                for (int shift = 0; shift <= (kind == FRAME ? 0 : 3); shift++) {
                    for (int out420p = 0; out420p <= (shift || kind == RGB ? 0 : 1); out420p++) { // (the surface call refuses the pairs)
                        for (int sd = 0; sd < 4; sd++) {
                            for (int offset : offsets) {
                                for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                                    if (kind == FRAME && (offset || pitch_kind)) { // (a pinned frame has one layout)
                                        continue;
                                    }
                                    check(Case{fmt, wh[0], wh[1], kind, shift, out420p != 0, (sd & 1) != 0, (sd & 2) ? 7 : 0, offset, pitch_kind});
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    printf("dec_delivery_check: %ld cases: coverage, order, form, counts and sources hold\n", g_cases);
    bool all = true;
    for (const TableRow &row : g_table) {
        printf("  %8ld cases  %s\n", row.hits, row.name);
        all = all && row.hits > 0;
    }
    if (!all) {
        fprintf(stderr, "FAILED: a row of the table was hit by no case\n");
        return 1;
    }
    return 0;
}
