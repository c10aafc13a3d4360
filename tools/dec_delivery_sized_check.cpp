// dec_delivery_sized_check.cpp -- the decoder's delivery planner (csrc/dec_delivery.h) swept on the CPU for SIZED targets
// (dsv2hip_dec_batch_surface_sized): chroma format x picture size x delivered size x target kind x postsharp x draw_info x pointer
// offset x pitch, over FAKE addresses as tools/dec_delivery_check.cpp does -- the reconstruction, the two staging areas and the target
// are disjoint ranges of one synthetic address space, and nothing is ever dereferenced.  Meant to be built with AddressSanitizer and
// UndefinedBehaviorSanitizer (the planner is handed no staging area it says it does not need: a look at one faults).  For every case:
//   staging   the predicates ask for the staged luma exactly for a sharpened or drawn-on picture, for the staged scaled picture exactly
//             for a semiplanar or RGB target, and for it at full size exactly then;
//   jobs      three resampling jobs and no reduction job; each reads the reconstruction's plane (the luma: the staged copy where there is
//             one), carries the ratio in lowest terms, D and the reciprocals, and delivers dsv_mk_frame's plane size for the named size;
//   ranges    every job's destination lies inside the target's plane as dsv2hip_dec_sized_dims documents it -- its rows exactly -- or
//             inside the staging plane it was given (from its origin, rows up to its stride, no more rows than it has), and the
//             interleave / the conversion read exactly what the resampling staged and write the target's rows exactly;
//   form      the plan's wide / rows / samples-a-row facts are those of resize_job_wide applied to its jobs;
//   not sized target_surface makes no sized target; for one that is not sized, with or without a shift, the predicates answer as they
//             did for a shift alone, never ask for the full-size staging, and the plan holds no resampling job, the resampling facts at
//             their defaults and three reduction jobs exactly under a shift.  (The rest of such a plan is what the unchanged
//             tools/dec_delivery_check.cpp checks.)
// tests/test_dec_delivery_sized_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/dec_delivery_sized_check.cpp -o dec_delivery_sized_check && ./dec_delivery_sized_check
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "dec_delivery.h"

using namespace dsv2;
using namespace dsv2::delivery;

namespace {

typedef unsigned long long U64;
constexpr U64 kReconAt = 0x10000000ull, kLumaAt = 0x20000000ull, kScaledAt = 0x30000000ull, kTargetAt = 0x40000000ull, kPlaneApart = 0x08000000ull;
enum Kind { PLANAR = 1, SEMI, RGB };

struct Case {
    int fmt, w, h, ow, oh, kind;
    bool sharp;
    int draw, offset, pitch_kind;
    bool staged_luma() const { return sharp || draw; }
    bool staged(int c) const { return kind == RGB || (kind == SEMI && c); } // plane c goes through the staged scaled picture
    std::string name() const
    {
        static const char *kinds[] = {"", "planar", "semiplanar", "rgb"};
        char s[160];
        snprintf(s, sizeof s, "fmt=%#x %dx%d -> %dx%d %s sharp=%d draw=%d offset=%d pitch=%d", fmt, w, h, ow, oh, kinds[kind], (int) sharp, draw, offset, pitch_kind);
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

int cdiv(int v, int shift) { return (v + (1 << shift) - 1) >> shift; }
int gcd_of(int x, int y) { return y ? gcd_of(y, x % y) : x; }

struct Rows { // `rows` rows of `bytes` bytes, `pitch` apart
    U64 base;
    long pitch, bytes;
    int rows;
    bool same(const void *p, long pitch_, long bytes_, int rows_) const { return base == (U64) (uintptr_t) p && pitch == pitch_ && bytes == bytes_ && rows == rows_; }
};

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

long pitch_of(long rb, int pitch_kind) { return pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + 1 : (rb + 255) / 256 * 256; }

struct World {
    DFrame recon;
    DPlane luma, scaled[3]; // the decoder's staging areas: the luma w x h, the scaled picture at the planes' own sizes (a sized target's); 16-byte strides
    Rows want[3];           // the target's planes as documented
    int nplanes = 0;
    int pw[3], ph[3], sw[3], sh[3]; // the planes of the picture and of the delivered one
    dsv2hip_out_surface sf = {};
    size_t rb[3];
    int rows[3];
};

// shift: a DSV2HIP_SCALE_* shift for the not-sized comparison (the delivered size is then the reduced one); ow x oh else
World make_world(const Case &c, int shift)
{
    World W;
    W.recon = fake_frame(kReconAt, c.fmt, c.w, c.h);
    W.luma = DPlane{(uint8_t *) (uintptr_t) kLumaAt, (c.w + 15) & ~15, c.w, c.h};
    U64 at = kScaledAt;
    const int hs = DSV_FORMAT_H_SHIFT(c.fmt), vs = DSV_FORMAT_V_SHIFT(c.fmt);
    const int dw = shift >= 0 ? cdiv(c.w, shift) : c.ow, dh = shift >= 0 ? cdiv(c.h, shift) : c.oh;
    for (int k = 0; k < 3; k++) {
        W.pw[k] = W.recon.p[k].w, W.ph[k] = W.recon.p[k].h;
        W.sw[k] = k ? cdiv(dw, hs) : dw, W.sh[k] = k ? cdiv(dh, vs) : dh;
        W.scaled[k] = DPlane{(uint8_t *) (uintptr_t) at, (W.pw[k] + 15) & ~15, W.pw[k], W.ph[k]};
        at += (U64) W.scaled[k].stride * (U64) W.ph[k];
    }
    W.rb[0] = (size_t) dw, W.rb[1] = W.rb[2] = (size_t) W.sw[1];
    W.rows[0] = dh, W.rows[1] = W.rows[2] = W.sh[1];
    W.nplanes = 3;
    if (c.kind == SEMI) {
        W.rb[1] = 2 * (size_t) W.sw[1], W.rb[2] = 0, W.rows[2] = 0, W.nplanes = 2;
    } else if (c.kind == RGB) {
        W.rb[0] = 4 * (size_t) dw, W.rb[1] = W.rb[2] = 0, W.rows[1] = W.rows[2] = 0, W.nplanes = 1;
    }
    const int base = c.kind == PLANAR ? DSV2HIP_SURFACE_PLANAR : c.kind == SEMI ? DSV2HIP_SURFACE_SEMIPLANAR
                   : (c.w + c.offset) & 1 ? (DSV2HIP_SURFACE_RGBA | DSV2HIP_CSC_FULL_RANGE) : (DSV2HIP_SURFACE_BGRA | DSV2HIP_CSC_BT709);
    W.sf.layout = base | ((shift > 0 ? shift : 0) << 12);
    for (int k = 0; k < W.nplanes; k++) {
        W.want[k] = Rows{kTargetAt + (U64) k * kPlaneApart + 256 + (U64) c.offset, pitch_of((long) W.rb[k], c.pitch_kind), (long) W.rb[k], W.rows[k]};
        W.sf.plane[k] = (void *) (uintptr_t) W.want[k].base;
        W.sf.pitch[k] = (size_t) W.want[k].pitch;
        W.sf.cap[k] = (size_t) (W.rows[k] - 1) * W.sf.pitch[k] + W.rb[k];
    }
    return W;
}

long g_cases = 0, g_wide = 0, g_plain = 0;

void check(const Case &c)
{
    World W = make_world(c, -1);
    OutTarget t;
    if (!target_surface(W.sf, W.rb, W.rows, &t)) {
        fail(c, "target_surface refused a surface that holds the sized picture exactly");
    }
    W.sf.cap[W.nplanes - 1]--;
    OutTarget none_t;
    if (target_surface(W.sf, W.rb, W.rows, &none_t)) {
        fail(c, "target_surface accepted a plane one byte short of the sized rows");
    }
    t.ow = c.ow, t.oh = c.oh;
    // staging
    if (!t.sized() || needs_staged_luma(t, c.sharp, c.draw) != c.staged_luma() || needs_staged_scaled(t) != (c.kind != PLANAR) ||
        needs_staged_full(t) != (c.kind != PLANAR)) {
        fail(c, "the staging predicates disagree with the rules");
    }
    static const DPlane none = {nullptr, 0, 0, 0};
    const DeliveryPlan p = plan_delivery(W.recon, c.fmt, t, c.sharp, c.draw, c.staged_luma() ? W.luma : none, needs_staged_scaled(t) ? W.scaled : nullptr);
    g_cases++;
    if (p.n_copy || p.n_to420 || p.n_scl || p.n_rsz != 3 || p.n_eg != (int) c.staged_luma() || p.n_uv != (int) (c.kind == SEMI) || p.n_rgb != (int) (c.kind == RGB) ||
        p.n_overlay != (int) (c.draw != 0) || p.sharpen_overlaid != (c.draw && c.sharp)) {
        fail(c, "jobs copy %d to420 %d egress %d scale %d resize %d uv %d rgb %d overlay %d sharpen %d", p.n_copy, p.n_to420, p.n_eg, p.n_scl, p.n_rsz, p.n_uv,
             p.n_rgb, p.n_overlay, (int) p.sharpen_overlaid);
    }
    // the staged luma: filled by one egress job from the reconstruction, drawn on and sharpened there
    if (c.staged_luma()) {
        const EgressJob &e = p.eg[0];
        if (e.src.data != W.recon.p[0].data || e.src.w != c.w || e.src.h != c.h || e.dst != W.luma.data || e.dstride != W.luma.stride ||
            (e.sharp != 0) != (c.sharp && !c.draw)) {
            fail(c, "the egress job does not stage the luma");
        }
    }
    if (c.draw && (p.overlay[0].data != W.luma.data || p.overlay[0].stride != W.luma.stride || p.overlay[0].w != c.w || p.overlay[0].h != c.h)) {
        fail(c, "the overlay is not on the staged luma");
    }
    // jobs and ranges
    bool wide = true;
    int max_rows = 0, max_cols = 0;
    for (int k = 0; k < 3; k++) {
        const ResizeOutJob &j = p.rsz[k];
        const DPlane &src = (k == 0 && c.staged_luma()) ? W.luma : W.recon.p[k];
        if (j.src != src.data || j.sstride != src.stride || j.pw != W.pw[k] || j.ph != W.ph[k] || j.ow != W.sw[k] || j.oh != W.sh[k]) {
            fail(c, "resampling job %d: %dx%d -> %dx%d from %p", k, j.pw, j.ph, j.ow, j.oh, (const void *) j.src);
        }
        const int gx = gcd_of(j.pw, j.ow), gy = gcd_of(j.ph, j.oh);
        if (j.a != j.pw / gx || j.b != j.ow / gx || j.c != j.ph / gy || j.d != j.oh / gy || (U64) j.D != (U64) j.a * (U64) j.c || j.D > (1u << 24) ||
            j.rD != resize_recip(j.D) || j.rb != resize_recip((uint32_t) j.b) || j.rd != resize_recip((uint32_t) j.d) || !resize_allowed(j.pw, j.ph, j.ow, j.oh)) {
            fail(c, "resampling job %d: a %d b %d c %d d %d D %u", k, j.a, j.b, j.c, j.d, j.D);
        }
        int room;
        if (c.staged(k)) { // from the staging plane's origin, rows up to its stride, no more rows than it has
            const DPlane &st = W.scaled[k];
            if (j.dst != st.data || j.dpitch != st.stride || j.ow > st.stride || j.oh > st.h) {
                fail(c, "resampling job %d writes %d rows of %d bytes, %d apart, at %p: its staging plane does not hold them", k, j.oh, j.ow, j.dpitch, (void *) j.dst);
            }
            room = st.stride;
        } else {
            if (!W.want[k].same(j.dst, j.dpitch, j.ow, j.oh)) {
                fail(c, "resampling job %d does not write the target's plane as documented", k);
            }
            room = j.ow;
        }
        wide = wide && resize_job_wide(j, room);
        max_rows = std::max(max_rows, j.oh), max_cols = std::max(max_cols, j.ow);
    }
    if (p.rsz_wide != wide || p.rsz_rows != max_rows || p.rsz_cols != max_cols) {
        fail(c, "the plan's facts (wide %d rows %d samples %d) are not its jobs' (%d %d %d)", (int) p.rsz_wide, p.rsz_rows, p.rsz_cols, (int) wide, max_rows, max_cols);
    }
    g_wide += wide;
    if (c.kind == SEMI) {
        const UvEgressJob &u = p.uv[0];
        if (u.su != W.scaled[1].data || u.sv != W.scaled[2].data || u.sstride != W.scaled[1].stride || u.sw != W.sw[1] || u.sh != W.sh[1] || u.cw != W.sw[1] ||
            u.ch != W.sh[1] || u.mode != 0 || !W.want[1].same(u.dst, u.dpitch, 2 * (long) u.cw, u.ch) || p.uv_rows != u.ch || p.uv_wide != uv_job_wide(u) || p.uv_conv) {
            fail(c, "the interleave does not read what the resampling staged, or does not write the target's rows");
        }
    }
    if (c.kind == RGB) {
        const RgbOutJob &r = p.rgb[0];
        const bool bgra = ((c.w + c.offset) & 1) == 0;
        if (r.sy != W.scaled[0].data || r.su != W.scaled[1].data || r.sv != W.scaled[2].data || r.ystride != W.scaled[0].stride || r.cstride != W.scaled[1].stride ||
            r.w != c.ow || r.h != c.oh || r.hs != DSV_FORMAT_H_SHIFT(c.fmt) || r.vs != DSV_FORMAT_V_SHIFT(c.fmt) || (r.bgra != 0) != bgra ||
            r.csc.ky != (bgra ? 298 : 256) || r.layout != kRgbOutPacked || !W.want[0].same(r.dst[0], r.dpitch[0], 4 * (long) r.w, r.h) || p.rgb_wide != rgb_out_job_wide(r)) {
            fail(c, "the conversion does not read what the resampling staged, or does not write the target's rows");
        }
    }
}

// ---- a target that is not sized: nothing of the resampling --------------------------------------------------------------------------------
// (what such a plan DOES hold is pinned by tools/dec_delivery_check.cpp, which knows nothing of a size and passes unchanged)

void check_plain(const Case &c, int shift)
{
    World W = make_world(c, shift);
    OutTarget t;
    if (!target_surface(W.sf, W.rb, W.rows, &t)) {
        fail(c, "target_surface refused the plain surface (shift %d)", shift);
    }
    if (t.ow || t.oh || t.sized()) {
        fail(c, "target_surface made a sized target");
    }
    const bool luma = needs_staged_luma(t, c.sharp, c.draw), scaled = needs_staged_scaled(t);
    if (luma != ((shift || c.kind == RGB) && c.staged_luma()) || scaled != (shift && c.kind != PLANAR) || needs_staged_full(t)) {
        fail(c, "the staging predicates changed for a target that is not sized (shift %d)", shift);
    }
    static const DPlane none = {nullptr, 0, 0, 0};
    const DeliveryPlan p = plan_delivery(W.recon, c.fmt, t, c.sharp, c.draw, luma ? W.luma : none, scaled ? W.scaled : nullptr);
    g_plain++;
    if (p.n_rsz || !p.rsz_wide || p.rsz_rows || p.rsz_cols || p.n_scl != (shift ? 3 : 0)) {
        fail(c, "a target that is not sized has resampling jobs or facts (shift %d)", shift);
    }
}

} // namespace

int main()
{
    static const int formats[] = {DSV_SUBSAMP_444, DSV_SUBSAMP_422, DSV_SUBSAMP_420, DSV_SUBSAMP_411, DSV_SUBSAMP_410};
    static const int sizes[][2] = {{16, 16}, {34, 18}, {50, 38}, {64, 48}, {352, 288}, {1920, 1080}, {1919, 1079}};
    static const int offsets[] = {0, 1, 16};
    for (int fmt : formats) {
        for (const int *wh : sizes) {
            const int w = wh[0], h = wh[1];
            // two thirds, an eighth, one less on one axis each, half, a multiple of 4 near three quarters, one axis only
            const int outs[][2] = {{(2 * w + 2) / 3, (2 * h + 2) / 3}, {(w + 7) / 8, (h + 7) / 8}, {w, h - 1}, {w - 1, h}, {(w + 1) / 2, (h + 1) / 2},
                                   {(3 * w / 4) & ~3, (3 * h / 4) & ~3},   {w, (h + 7) / 8},           {(w + 7) / 8, h}};
            for (const int *o : outs) {
                for (int kind = PLANAR; kind <= RGB; kind++) {
                    for (int sd = 0; sd < 4; sd++) {
                        for (int offset : offsets) {
                            for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                                const Case c{fmt, w, h, o[0], o[1], kind, (sd & 1) != 0, (sd & 2) ? 7 : 0, offset, pitch_kind};
                                check(c);
                                if (o == outs[0]) {
                                    for (int shift = 0; shift <= 3; shift++) {
                                        check_plain(c, shift);
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    if (g_wide == 0 || g_wide == g_cases) {
        fprintf(stderr, "FAILED: the sweep holds only one form of the resampling\n");
        return 1;
    }
    printf("dec_delivery_sized_check: %ld sized cases (%ld in the wide form): staging, jobs, ranges and form hold; %ld plans of targets that are not sized hold "
           "nothing of the resampling\n",
           g_cases, g_wide, g_plain);
    return 0;
}
