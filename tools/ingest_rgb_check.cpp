// ingest_rgb_check.cpp -- the body of k_ingest_rgb (csrc/ingest_rgb.h) run as plain C++ on the CPU, thread by thread, over a sweep of
// forms, byte orders, presets, chroma formats, widths, heights, pitches and pointer offsets; meant to be built with
// AddressSanitizer and UndefinedBehaviorSanitizer, which see every read outside the surface's allocation (an exact-size heap block:
// the last row has nothing behind it), every write outside a plane's and every misaligned word access.  The program itself compares
// the three planes with the conversion of include/dsv2_hip.h restated here sample by sample (nothing shared with the kernel's
// text), and checks that no byte outside the planes' w x h / cw x ch changed.
// The job records the bodies run on are the library's own: csrc/enc_ingest.h accepts each surface and plans them (tools/ingest_plan.h).
// tests/test_ingest_rgb_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/ingest_rgb_check.cpp -o ingest_rgb_check && ./ingest_rgb_check [--dump DIR]
// --dump DIR writes, for a few named cases, NAME.src (the pixels, h rows of 4 * w bytes) and NAME.yuv (the converted planes, packed).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ingest_plan.h"
#include "ingest_rgb.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::expect_chroma;
using support::expect_luma;
using support::kGuard;
using support::Picture;

// (the conversion, restated one sample at a time: check_support.h)

// ---- planes as dframe_alloc lays them out: 32-pixel border, stride a multiple of 16, 16-byte aligned origin ---------------------
struct Plane : support::GuardedPlane {
    Plane(int w_, int h_) : support::GuardedPlane(w_, h_, kBorder, 0) {}
};

template <int VEC> void run_grid(const RgbJob &j)
{
    const int blocks = (j.h + 15) / 16;
    for (int bx = 0; bx < blocks; bx++) {
        for (int ty = 0; ty < 4; ty++) {
            const int y0 = (bx * 4 + ty) * 4;
            if (y0 >= j.h) {
                continue;
            }
            for (int tx = 0; tx < 64; tx++) {
                ingest_rgb_rows<VEC>(j, y0, tx * 4, 64 * 4);
            }
        }
    }
}

using support::kHs;
using support::kVs;
const int kSubsamp[5] = {DSV_SUBSAMP_444, DSV_SUBSAMP_422, DSV_SUBSAMP_420, DSV_SUBSAMP_411, DSV_SUBSAMP_410};
using support::kFmtName;
long g_cases = 0, g_wide = 0;
const char *g_dump = nullptr;

// force_general: run the general form even where the wide one would be picked (a step takes it when ANY of its surfaces needs it)
void check(int w, int h, int fmt, int csc, bool bgra, int pitch_kind, int offset, bool force_general, const char *dump_name = nullptr)
{
    const int hs = kHs[fmt], vs = kVs[fmt];
    const int cw = (w + (1 << hs) - 1) >> hs, ch = (h + (1 << vs) - 1) >> vs;
    const size_t rb = 4 * (size_t) w;
    const size_t pitch = pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + 1 : pitch_kind == 2 ? rb + 3 : ((rb + 15) & ~(size_t) 15) + 16;
    const size_t bytes = (size_t) offset + (size_t) (h - 1) * pitch + rb; // not one byte more: the last row has no padding behind it
    uint8_t *alloc = nullptr;
    if (posix_memalign((void **) &alloc, 16, bytes) != 0) {
        abort();
    }
    uint8_t *src = alloc + offset;
    unsigned seed = 977u * (unsigned) w + 31u * (unsigned) h + (unsigned) (fmt + 5 * pitch_kind + 20 * offset);
    for (size_t i = 0; i < bytes; i++) { // (padding and alpha hold noise too)
        seed = seed * 1664525u + 1013904223u;
        alloc[i] = (uint8_t) (seed >> 24);
    }
    Picture pic{w, h, std::vector<int>(3 * (size_t) w * h)};
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            uint8_t *p = src + (size_t) y * pitch + 4 * (size_t) x;
            seed = seed * 1664525u + 1013904223u;
            if ((seed >> 29) == 0) { // an eighth of the pixels: a corner of the colour cube, where the sums are extreme
                p[0] = (seed & 0x10000) ? 255 : 0, p[1] = (seed & 0x20000) ? 255 : 0, p[2] = (seed & 0x40000) ? 255 : 0;
            }
            int *c = &pic.rgb[3 * ((size_t) y * w + x)];
            c[0] = bgra ? p[2] : p[0], c[1] = p[1], c[2] = bgra ? p[0] : p[2];
        }
    }
    std::vector<uint8_t> was(alloc, alloc + bytes);
    Plane Y(w, h), U(cw, ch), V(cw, ch);
    const dsv2hip_surface sf{{src, nullptr, nullptr}, {pitch, 0, 0}, (bgra ? DSV2HIP_SURFACE_BGRA : DSV2HIP_SURFACE_RGBA) | csc};
    const enc_ingest::IngestPlan plan = planned(enc_ingest::CALL_PLAIN, kSubsamp[fmt], Y, U, V, sf, w, h);
    expect_records(plan, enc_ingest::RGB, 1);
    const RgbJob &j = plan.rgb[0];
    const bool wide = plan.wide[enc_ingest::RGB] && !force_general;
    wide ? run_grid<16>(j) : run_grid<4>(j);
    g_cases++;
    g_wide += wide;
    bool ok = memcmp(was.data(), alloc, bytes) == 0; // the surface is only read
    const Plane *pl[3] = {&Y, &U, &V};
    for (int c = 0; c < 3 && ok; c++) {
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
            fprintf(stderr, "MISMATCH %dx%d %s csc=0x%x %s pitch=%zu offset=%d wide=%d: plane %d row %ld column %ld is %02x, expected %02x\n", w, h,
                    kFmtName[fmt], csc, bgra ? "bgra" : "rgba", pitch, offset, (int) wide, c, row, col, pl[c]->alloc[i], want[i]);
            exit(1);
        }
    }
    if (!ok) {
        fprintf(stderr, "the surface was written: %dx%d %s pitch=%zu offset=%d\n", w, h, kFmtName[fmt], pitch, offset);
        exit(1);
    }
    if (dump_name && g_dump) {
        FILE *fs = fopen((std::string(g_dump) + "/" + dump_name + ".src").c_str(), "wb");
        FILE *fy = fopen((std::string(g_dump) + "/" + dump_name + ".yuv").c_str(), "wb");
        if (!fs || !fy) {
            fprintf(stderr, "cannot write into %s\n", g_dump);
            exit(1);
        }
        for (int y = 0; y < h; y++) {
            fwrite(src + (size_t) y * pitch, 1, rb, fs);
        }
        for (int c = 0; c < 3; c++) {
            for (int y = 0; y < pl[c]->h; y++) {
                fwrite(pl[c]->org + (size_t) y * pl[c]->stride, 1, (size_t) pl[c]->w, fy);
            }
        }
        fclose(fs);
        fclose(fy);
    }
    free(alloc);
}

} // namespace

int main(int argc, char **argv)
{
    if (!support::dump_option(argc, argv, &g_dump)) {
        return 2;
    }
    static const int cscs[4] = {0x000, 0x100, 0x200, 0x300};
    // every combination of byte order, preset, format, pitch kind and offset, in both forms where the wide one applies, at the
    // smallest pictures and at footprints half outside them
    for (int w : {16, 17, 18, 19, 22}) {
        for (int h : {16, 17, 18, 19}) {
            for (int fmt = 0; fmt < 5; fmt++) {
                for (int csc : cscs) {
                    for (int bgra = 0; bgra < 2; bgra++) {
                        for (int pitch_kind = 0; pitch_kind < 4; pitch_kind++) {
                            for (int offset = 0; offset < 4; offset++) {
                                check(w, h, fmt, csc, bgra != 0, pitch_kind, offset, false);
                            }
                        }
                        check(w, h, fmt, csc, bgra != 0, 3, 0, true);
                    }
                }
            }
        }
    }
    // every width, height and format; byte order, preset, pitch and offset take turns
    std::vector<int> ws;
    for (int w = 16; w <= 70; w++) {
        ws.push_back(w);
    }
    ws.push_back(1920); // (rows of several passes of the 64 lanes)
    long turn = 0;
    for (int w : ws) {
        for (int h = 16; h <= 38; h++) {
            if (w == 1920 && h != 16 && h != 18 && h != 37) {
                continue;
            }
            for (int fmt = 0; fmt < 5; fmt++, turn++) {
                const int csc = cscs[turn & 3];
                const bool bgra = ((turn >> 2) & 1) != 0;
                check(w, h, fmt, csc, bgra, 3, 0, false);                                                  // wide where w allows
                check(w, h, fmt, cscs[(turn + 1) & 3], !bgra, (int) (turn % 3), (int) ((turn / 3) & 3), false); // general
                check(w, h, fmt, cscs[(turn + 2) & 3], bgra, 3, 0, true);                                  // general on an aligned surface
            }
        }
    }
    check(22, 18, 2, 0x000, true, 2, 1, false, "bgra_000_420_22x18");
    check(18, 18, 4, 0x300, false, 1, 3, false, "rgba_300_410_18x18");
    check(18, 18, 3, 0x100, false, 2, 2, false, "rgba_100_411_18x18");
    check(17, 16, 0, 0x200, true, 0, 0, false, "bgra_200_444_17x16");
    check(68, 38, 1, 0x000, false, 3, 0, false, "rgba_000_422_68x38");
    check(1920, 16, 2, 0x300, true, 3, 0, false, "bgra_300_420_1920x16");
    printf("ingest_rgb_check: %ld cases (%ld in the wide form) equal the sample-by-sample conversion; no byte outside the planes changed, "
           "the surfaces are as they were\n",
           g_cases, g_wide);
    return 0;
}
