// ingest_rgb3_check.cpp -- the body of k_ingest_rgb3 (csrc/ingest_rgb3.h) run as plain C++ on the CPU, thread by thread, over a sweep
// of kinds (packed three-byte, planar), forms, byte orders, presets, chroma formats, widths 1 .. 40 and 354, heights, pitches and
// pointer offsets 0 .. 3; meant to be built with AddressSanitizer and UndefinedBehaviorSanitizer, which see every read outside a
// source plane's allocation (an exact-size heap block: the last row has nothing behind it), every write outside a destination
// plane's and every misaligned word access.  The program itself compares the three planes
//   - with the conversion of include/dsv2_hip.h restated here sample by sample (nothing shared with the kernel's text), and
//   - with what the body of k_ingest_rgb (csrc/ingest_rgb.h) makes of the same pixels as an RGBA surface with noise for alpha,
// and checks that no byte outside the planes' w x h / cw x ch changed and that the surface is as it was.
// The job records the bodies run on are the library's own: csrc/enc_ingest.h accepts each surface and plans them (tools/ingest_plan.h).
// tests/test_ingest_rgb3_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/ingest_rgb3_check.cpp -o ingest_rgb3_check && ./ingest_rgb3_check [--dump DIR]
// --dump DIR writes, for a few named cases, NAME.src (packed: h rows of 3 * w bytes; planar: the planes R, G, B of h rows of w bytes,
// back to back) and NAME.yuv (the converted planes, packed).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ingest_plan.h"
#include "ingest_rgb3.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::expect_chroma;
using support::expect_luma;
using support::kGuard;
using support::Picture;
enum Order { BGR = 0, RGB = 1, RGBP = 2 };
const char *const kOrderName[3] = {"bgr", "rgb", "rgbp"};

// (the conversion, restated one sample at a time: check_support.h)

// ---- planes as dframe_alloc lays them out: 32-pixel border, stride a multiple of 16, 16-byte aligned origin ---------------------
struct Plane : support::GuardedPlane {
    Plane(int w_, int h_) : support::GuardedPlane(w_, h_, kBorder, 0) {}
};

// a source plane: `offset` bytes, then h rows of rb bytes `pitch` apart, and not one byte more
struct Source {
    uint8_t *alloc, *org;
    size_t bytes, pitch, rb;
    std::vector<uint8_t> was;
    Source(int h, size_t rb_, size_t pitch_, int offset, unsigned &seed) : pitch(pitch_), rb(rb_)
    {
        bytes = (size_t) offset + (size_t) (h - 1) * pitch + rb;
        if (posix_memalign((void **) &alloc, 16, bytes) != 0) {
            abort();
        }
        org = alloc + offset;
        for (size_t i = 0; i < bytes; i++) { // (padding holds noise too)
            seed = seed * 1664525u + 1013904223u;
            alloc[i] = (uint8_t) (seed >> 24);
        }
    }
    void keep() { was.assign(alloc, alloc + bytes); }
    bool untouched() const { return memcmp(was.data(), alloc, bytes) == 0; }
    ~Source() { free(alloc); }
};

template <class F> void run_grid(int h, F thread)
{
    const int blocks = (h + 15) / 16;
    for (int bx = 0; bx < blocks; bx++) {
        for (int ty = 0; ty < 4; ty++) {
            const int y0 = (bx * 4 + ty) * 4;
            if (y0 >= h) {
                continue;
            }
            for (int tx = 0; tx < 64; tx++) {
                thread(y0, tx * 4, 64 * 4);
            }
        }
    }
}

using support::kHs;
using support::kVs;
const int kSubsamp[5] = {DSV_SUBSAMP_444, DSV_SUBSAMP_422, DSV_SUBSAMP_420, DSV_SUBSAMP_411, DSV_SUBSAMP_410};
using support::kFmtName;
long g_cases = 0, g_wide[2] = {0, 0};
const char *g_dump = nullptr;

size_t pitch_of(size_t rb, int pitch_kind) { return pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + 1 : pitch_kind == 2 ? rb + 3 : ((rb + 15) & ~(size_t) 15) + 16; }

// offset: of plane[0]; the other planes of a planar surface get offset + 1, + 2 (mod 4) unless it is 0
// force_general: run the general form even where the wide one would be picked (a step takes it when ANY of its surfaces needs it)
void check(int w, int h, int fmt, int csc, Order order, int pitch_kind, int offset, bool force_general, const char *dump_name = nullptr)
{
    const int hs = kHs[fmt], vs = kVs[fmt];
    const int cw = (w + (1 << hs) - 1) >> hs, ch = (h + (1 << vs) - 1) >> vs;
    const bool planar = order == RGBP;
    const int nsrc = planar ? 3 : 1;
    unsigned seed = 977u * (unsigned) w + 31u * (unsigned) h + (unsigned) (fmt + 5 * pitch_kind + 20 * offset + 80 * (int) order);
    std::vector<Source *> src;
    for (int c = 0; c < nsrc; c++) {
        const size_t rb = planar ? (size_t) w : 3 * (size_t) w;
        const size_t pitch = pitch_of(rb, pitch_kind) + (pitch_kind == 3 ? 16 * (size_t) c : 0); // (planar: the planes' pitches differ)
        src.push_back(new Source(h, rb, pitch, offset ? (offset + c) & 3 : 0, seed));
    }
    Picture pic{w, h, std::vector<int>(3 * (size_t) w * h)};
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            uint8_t *p[3]; // R, G, B of the pixel
            for (int c = 0; c < 3; c++) {
                p[c] = planar ? src[(size_t) c]->org + (size_t) y * src[(size_t) c]->pitch + x
                              : src[0]->org + (size_t) y * src[0]->pitch + 3 * (size_t) x + (order == BGR ? 2 - c : c);
            }
            seed = seed * 1664525u + 1013904223u;
            if ((seed >> 29) == 0) { // an eighth of the pixels: a corner of the colour cube, where the sums are extreme
                *p[0] = (seed & 0x10000) ? 255 : 0, *p[1] = (seed & 0x20000) ? 255 : 0, *p[2] = (seed & 0x40000) ? 255 : 0;
            }
            int *c = &pic.rgb[3 * ((size_t) y * w + x)];
            c[0] = *p[0], c[1] = *p[1], c[2] = *p[2];
        }
    }
    for (Source *s : src) {
        s->keep();
    }
    Plane Y(w, h), U(cw, ch), V(cw, ch);
    dsv2hip_surface sf{};
    sf.layout = (DSV2HIP_SURFACE_BGR + (int) order) | csc;
    for (int c = 0; c < nsrc; c++) {
        sf.plane[c] = src[(size_t) c]->org, sf.pitch[c] = src[(size_t) c]->pitch;
    }
    const int cl = planar ? enc_ingest::RGB3_PLANAR : enc_ingest::RGB3_PACKED;
    const enc_ingest::IngestPlan plan = planned(enc_ingest::CALL_PLAIN, kSubsamp[fmt], Y, U, V, sf, w, h);
    expect_records(plan, cl, 1);
    const Rgb3Job &j = plan.rgb3[0];
    const bool wide = plan.wide[cl] && !force_general;
    if (planar) {
        wide ? run_grid(h, [&](int y0, int x, int step) { ingest_rgb3_rows<kRgb3Planar, true>(j, y0, x, step); })
             : run_grid(h, [&](int y0, int x, int step) { ingest_rgb3_rows<kRgb3Planar, false>(j, y0, x, step); });
    } else {
        wide ? run_grid(h, [&](int y0, int x, int step) { ingest_rgb3_rows<kRgb3Packed, true>(j, y0, x, step); })
             : run_grid(h, [&](int y0, int x, int step) { ingest_rgb3_rows<kRgb3Packed, false>(j, y0, x, step); });
    }
    g_cases++;
    g_wide[planar] += wide;
    char what[160];
    snprintf(what, sizeof what, "%dx%d %s csc=0x%x %s pitch=%zu offset=%d wide=%d", w, h, kFmtName[fmt], csc, kOrderName[order], src[0]->pitch, offset, (int) wide);
    for (Source *s : src) {
        if (!s->untouched()) {
            fprintf(stderr, "the surface was written: %s\n", what);
            exit(1);
        }
    }
    const Plane *pl[3] = {&Y, &U, &V};
    for (int c = 0; c < 3; c++) {
        std::vector<uint8_t> want(pl[c]->bytes, kGuard);
        for (int y = 0; y < pl[c]->h; y++) {
            for (int x = 0; x < pl[c]->w; x++) {
                want[(size_t) (y + kBorder) * pl[c]->stride + kBorder + x] =
                    (uint8_t) (c == 0 ? expect_luma(pic, csc, x, y) : expect_chroma(pic, csc, c, hs, vs, x, y));
            }
        }
        if (memcmp(want.data(), pl[c]->alloc, pl[c]->bytes) != 0) {
            size_t i = 0;
            while (want[i] == pl[c]->alloc[i]) {
                i++;
            }
            const long row = (long) (i / pl[c]->stride) - kBorder, col = (long) (i % pl[c]->stride) - kBorder;
            fprintf(stderr, "MISMATCH %s: plane %d row %ld column %ld is %02x, expected %02x\n", what, c, row, col, pl[c]->alloc[i], want[i]);
            exit(1);
        }
    }
    // the same pixels as an RGBA surface with noise for alpha, through the four-byte body: identical planes, borders and all
    {
        std::vector<uint8_t> rgba(4 * (size_t) w * h);
        for (size_t i = 0; i < (size_t) w * h; i++) {
            seed = seed * 1664525u + 1013904223u;
            rgba[4 * i] = (uint8_t) pic.rgb[3 * i], rgba[4 * i + 1] = (uint8_t) pic.rgb[3 * i + 1], rgba[4 * i + 2] = (uint8_t) pic.rgb[3 * i + 2];
            rgba[4 * i + 3] = (uint8_t) (seed >> 24);
        }
        Plane Y4(w, h), U4(cw, ch), V4(cw, ch);
        const dsv2hip_surface sf4{{rgba.data(), nullptr, nullptr}, {4 * (size_t) w, 0, 0}, DSV2HIP_SURFACE_RGBA | csc};
        const enc_ingest::IngestPlan plan4 = planned(enc_ingest::CALL_PLAIN, kSubsamp[fmt], Y4, U4, V4, sf4, w, h);
        expect_records(plan4, enc_ingest::RGB, 1);
        const RgbJob &j4 = plan4.rgb[0];
        run_grid(h, [&](int y0, int x, int step) { ingest_rgb_rows<4>(j4, y0, x, step); });
        const Plane *p4[3] = {&Y4, &U4, &V4};
        for (int c = 0; c < 3; c++) {
            if (memcmp(p4[c]->alloc, pl[c]->alloc, pl[c]->bytes) != 0) {
                fprintf(stderr, "plane %d differs from the RGBA surface's of the same pixels: %s\n", c, what);
                exit(1);
            }
        }
    }
    if (dump_name && g_dump) {
        FILE *fs = fopen((std::string(g_dump) + "/" + dump_name + ".src").c_str(), "wb");
        FILE *fy = fopen((std::string(g_dump) + "/" + dump_name + ".yuv").c_str(), "wb");
        if (!fs || !fy) {
            fprintf(stderr, "cannot write into %s\n", g_dump);
            exit(1);
        }
        for (Source *s : src) {
            for (int y = 0; y < h; y++) {
                fwrite(s->org + (size_t) y * s->pitch, 1, s->rb, fs);
            }
        }
        for (int c = 0; c < 3; c++) {
            for (int y = 0; y < pl[c]->h; y++) {
                fwrite(pl[c]->org + (size_t) y * pl[c]->stride, 1, (size_t) pl[c]->w, fy);
            }
        }
        fclose(fs);
        fclose(fy);
    }
    for (Source *s : src) {
        delete s;
    }
}

} // namespace

int main(int argc, char **argv)
{
    if (!support::dump_option(argc, argv, &g_dump)) {
        return 2;
    }
    static const int cscs[4] = {0x000, 0x100, 0x200, 0x300};
    static const Order orders[3] = {BGR, RGB, RGBP};
    // every width 1 .. 40 and 354 (more than one pass of the 64 lanes, the last one partial) with every layout, format, pitch kind and
    // offset, in both forms where the wide one applies; heights and presets take turns
    static const int hts[10] = {16, 1, 17, 2, 18, 3, 19, 5, 22, 4};
    long turn = 0;
    for (int wi = 1; wi <= 41; wi++) {
        const int w = wi <= 40 ? wi : 354;
        for (int fmt = 0; fmt < 5; fmt++) {
            for (Order order : orders) {
                for (int pitch_kind = 0; pitch_kind < 4; pitch_kind++) {
                    for (int offset = 0; offset < 4; offset++, turn++) {
                        check(w, hts[turn % 10], fmt, cscs[(turn / 10) & 3], order, pitch_kind, offset, false);
                    }
                }
                check(w, hts[turn % 10], fmt, cscs[turn & 3], order, 3, 0, true); // general on an aligned surface
                check(w, hts[(turn + 1) % 10], fmt, cscs[(turn + 1) & 3], order, 0, 0, false); // pitch = the row's bytes: wide where w % 4 == 0
            }
        }
    }
    // every height 1 .. 38 at the smallest pictures and at footprints half outside them, every preset with every layout
    for (int w : {16, 18, 22}) {
        for (int h = 1; h <= 38; h++) {
            for (int fmt = 0; fmt < 5; fmt++) {
                for (int csc : cscs) {
                    for (Order order : orders) {
                        turn++;
                        check(w, h, fmt, csc, order, 3, 0, false);                            // wide where w allows
                        check(w, h, fmt, csc, order, (int) (turn % 3), (int) (turn & 3), false); // general
                    }
                }
            }
        }
    }
    check(1920, 18, 2, 0x100, RGB, 3, 0, false); // (rows of several passes in the wide form)
    check(1920, 16, 4, 0x200, RGBP, 3, 0, false);
    check(22, 18, 2, 0x000, BGR, 2, 1, false, "bgr_000_420_22x18");
    check(18, 18, 4, 0x300, RGB, 1, 3, false, "rgb_300_410_18x18");
    check(18, 18, 3, 0x100, RGBP, 2, 2, false, "rgbp_100_411_18x18");
    check(18, 18, 4, 0x000, RGBP, 1, 1, false, "rgbp_000_410_18x18");
    check(18, 18, 3, 0x200, BGR, 2, 3, false, "bgr_200_411_18x18");
    check(17, 16, 0, 0x200, BGR, 0, 0, false, "bgr_200_444_17x16");
    check(68, 38, 1, 0x000, RGB, 3, 0, false, "rgb_000_422_68x38");
    check(68, 38, 1, 0x300, RGBP, 3, 0, false, "rgbp_300_422_68x38");
    check(40, 21, 0, 0x100, RGBP, 0, 0, false, "rgbp_100_444_40x21");
    check(1920, 16, 2, 0x300, BGR, 3, 0, false, "bgr_300_420_1920x16");
    printf("ingest_rgb3_check: %ld cases (%ld packed and %ld planar ones in the wide form) equal the sample-by-sample conversion and the RGBA "
           "surface's planes; no byte outside the planes changed, the surfaces are as they were\n",
           g_cases, g_wide[0], g_wide[1]);
    return 0;
}
