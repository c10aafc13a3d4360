// egress_rgb_check.cpp -- the body of k_egress_rgb (csrc/egress_rgb.h) run as plain C++ on the CPU, thread by thread, over a sweep of
// forms, byte orders, presets, chroma formats, widths, heights, pitches and pointer offsets; meant to be built with
// AddressSanitizer and UndefinedBehaviorSanitizer, which see every read outside the source planes' allocations (exact-size heap
// blocks: planes as dframe_alloc lays them out, and the luma also as the decoder stages it for drawn-on / sharpened pictures -- no
// border, nothing behind the last row's stride), every write outside the surface's and every misaligned word access.  The program
// itself compares the surface with the conversion of include/dsv2_hip.h restated here pixel by pixel (nothing shared with the
// kernel's text), and checks that every alpha byte is 255, that no byte outside the h rows of 4 * w bytes changed -- guard bytes in
// front, padding between the rows, guard bytes behind -- and that the source planes are as they were.
// tests/test_egress_rgb_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/egress_rgb_check.cpp -o egress_rgb_check && ./egress_rgb_check [--dump DIR]
// --dump DIR writes, for a few named cases, NAME.yuv (the source planes, packed) and NAME.rgb (the pixels, h rows of 4 * w bytes).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "egress_rgb.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::kFmtName;
using support::kGuard;
using support::kHs;
using support::kLead; // guard bytes in front of and behind the surface
using support::kPreset;
using support::preset_of;
using support::kVs;

// ---- the conversion, restated: one pixel at a time, in the header's own terms ---------------------------------------------------
void expect_pixel(int csc, bool bgra, int Y, int U, int V, uint8_t out[4])
{
    uint8_t rgb[3];
    support::expect_pixel(csc, Y, U, V, rgb);
    out[0] = rgb[bgra ? 2 : 0], out[1] = rgb[1], out[2] = rgb[bgra ? 0 : 2], out[3] = 255;
}

// ---- source planes: an exact-size heap block each ---------------------------------------------------------------------------------
struct Plane : support::Plane {
    // bordered: as dframe_alloc lays a plane out (32-pixel border, stride a multiple of 16, 16-byte aligned origin); else as the
    // decoder stages a luma plane: no border, stride = w rounded up to 16, h rows
    Plane(int w_, int h_, bool bordered, unsigned seed) : support::Plane(w_, h_, bordered ? kBorder : 0, seed, support::noise_range_ends) {}
};

template <bool WIDE> void run_grid(const RgbOutJob &j)
{
    const int blocks = (j.h + 15) / 16;
    for (int bx = 0; bx < blocks; bx++) {
        for (int ty = 0; ty < 4; ty++) {
            const int y0 = (bx * 4 + ty) * 4;
            if (y0 >= j.h) {
                continue;
            }
            for (int tx = 0; tx < 64; tx++) {
                egress_rgb_rows<WIDE>(j, y0, tx * 4, 64 * 4);
            }
        }
    }
}

long g_cases = 0, g_wide = 0;
const char *g_dump = nullptr;

size_t pitch_of(int w, int pitch_kind)
{
    const size_t rb = 4 * (size_t) w, up = (rb + 15) & ~(size_t) 15;
    return pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + 1 : pitch_kind == 2 ? up + 16 : up + 4096;
}

// force_general: run the general form even where the wide one would be picked (a round takes it when ANY of its surfaces needs it)
void check(const Plane &Y, const Plane &U, const Plane &V, int fmt, int csc, bool bgra, int pitch_kind, int offset, bool force_general,
           const char *dump_name = nullptr)
{
    const int w = Y.w, h = Y.h, hs = kHs[fmt], vs = kVs[fmt];
    const size_t rb = 4 * (size_t) w, pitch = pitch_of(w, pitch_kind);
    const size_t start = (size_t) kLead + (size_t) offset;
    const size_t bytes = start + (size_t) (h - 1) * pitch + rb + kLead;
    uint8_t *alloc = nullptr;
    if (posix_memalign((void **) &alloc, 16, bytes) != 0) {
        abort();
    }
    memset(alloc, kGuard, bytes);
    uint8_t *dst = alloc + start;
    const long *p = kPreset[preset_of(csc)];
    const RgbOutJob j{Y.org, U.org, V.org, dst, Y.stride, U.stride, (int) pitch, w, h, hs, vs, {(int) p[0], (int) p[1], (int) p[2], (int) p[3], (int) p[4], (int) p[5]}, bgra};
    const bool wide = rgb_out_job_wide(j) && !force_general;
    wide ? run_grid<true>(j) : run_grid<false>(j);
    g_cases++;
    g_wide += wide;
    std::vector<uint8_t> want(bytes, kGuard);
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            expect_pixel(csc, bgra, Y.at(x, y), U.at(x >> hs, y >> vs), V.at(x >> hs, y >> vs), &want[start + (size_t) y * pitch + 4 * (size_t) x]);
        }
    }
    if (memcmp(want.data(), alloc, bytes) != 0) {
        size_t i = 0;
        while (want[i] == alloc[i]) {
            i++;
        }
        const long rel = (long) i - (long) start;
        fprintf(stderr, "MISMATCH %dx%d %s csc=0x%x %s pitch=%zu offset=%d wide=%d: byte %ld of the surface (row %ld, byte %ld of it) is %02x, expected %02x\n", w,
                h, kFmtName[fmt], csc, bgra ? "bgra" : "rgba", pitch, offset, (int) wide, rel, rel >= 0 ? rel / (long) pitch : -1L,
                rel >= 0 ? rel % (long) pitch : rel, alloc[i], want[i]);
        exit(1);
    }
    for (int y = 0; y < h; y++) { // (what the comparison above already implies, said on its own)
        for (int x = 0; x < w; x++) {
            if (dst[(size_t) y * pitch + 4 * (size_t) x + 3] != 255) {
                fprintf(stderr, "alpha of pixel (%d, %d) is not 255\n", x, y);
                exit(1);
            }
        }
    }
    if (!Y.unchanged() || !U.unchanged() || !V.unchanged()) {
        fprintf(stderr, "a source plane was written: %dx%d %s pitch=%zu offset=%d\n", w, h, kFmtName[fmt], pitch, offset);
        exit(1);
    }
    if (dump_name && g_dump) {
        FILE *fy = fopen((std::string(g_dump) + "/" + dump_name + ".yuv").c_str(), "wb");
        FILE *fr = fopen((std::string(g_dump) + "/" + dump_name + ".rgb").c_str(), "wb");
        if (!fy || !fr) {
            fprintf(stderr, "cannot write into %s\n", g_dump);
            exit(1);
        }
        const Plane *pl[3] = {&Y, &U, &V};
        for (int c = 0; c < 3; c++) {
            for (int y = 0; y < pl[c]->h; y++) {
                fwrite(pl[c]->org + (size_t) y * pl[c]->stride, 1, (size_t) pl[c]->w, fy);
            }
        }
        for (int y = 0; y < h; y++) {
            fwrite(dst + (size_t) y * pitch, 1, rb, fr);
        }
        fclose(fy);
        fclose(fr);
    }
    free(alloc);
}

struct Source { // the three planes of a w x h picture of format fmt; staged: the luma as the decoder stages it
    Plane Y, U, V;
    Source(int w, int h, int fmt, bool staged)
        : Y(w, h, !staged, 977u * (unsigned) w + 31u * (unsigned) h + (unsigned) fmt),
          U((w + (1 << kHs[fmt]) - 1) >> kHs[fmt], (h + (1 << kVs[fmt]) - 1) >> kVs[fmt], true, 7919u * (unsigned) w + 13u * (unsigned) h + (unsigned) fmt),
          V((w + (1 << kHs[fmt]) - 1) >> kHs[fmt], (h + (1 << kVs[fmt]) - 1) >> kVs[fmt], true, 104729u * (unsigned) w + 7u * (unsigned) h + (unsigned) fmt)
    {
    }
};

void named(int w, int h, int fmt, int csc, bool bgra, int pitch_kind, int offset, const char *name)
{
    Source s(w, h, fmt, false);
    check(s.Y, s.U, s.V, fmt, csc, bgra, pitch_kind, offset, false, name);
}

} // namespace

int main(int argc, char **argv)
{
    if (!support::dump_option(argc, argv, &g_dump)) {
        return 2;
    }
    static const int cscs[4] = {0x000, 0x100, 0x200, 0x300};
    std::vector<int> ws;
    for (int w = 1; w <= 40; w++) {
        ws.push_back(w);
    }
    ws.push_back(1920); // (rows of several passes of the 64 lanes)
    long turn = 0;
    for (int w : ws) {
        for (int h = 1; h <= 9; h++) {
            for (int fmt = 0; fmt < 5; fmt++) {
                const Source s(w, h, fmt, false), staged(w, h, fmt, true);
                for (int csc : cscs) {
                    for (int bgra = 0; bgra < 2; bgra++) {
                        for (int pitch_kind = 0; pitch_kind < 4; pitch_kind++) {
                            for (int offset = 0; offset < 4; offset++, turn++) {
                                if (w == 1920 && (turn + h) % 8 != 0) { // (the long rows: an eighth of the combinations, taking turns)
                                    continue;
                                }
                                const Source &src = (turn & 1) ? staged : s;
                                check(src.Y, src.U, src.V, fmt, csc, bgra != 0, pitch_kind, offset, false); // wide where everything allows
                                if (offset == 0 && w % 4 == 0 && pitch_of(w, pitch_kind) % 16 == 0) {
                                    check(src.Y, src.U, src.V, fmt, csc, bgra != 0, pitch_kind, offset, true); // general on an aligned surface
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    named(22, 18, 2, 0x000, true, 1, 1, "bgra_000_420_22x18");
    named(18, 18, 4, 0x300, false, 1, 3, "rgba_300_410_18x18");
    named(18, 18, 3, 0x100, false, 0, 2, "rgba_100_411_18x18");
    named(17, 16, 0, 0x200, true, 0, 0, "bgra_200_444_17x16");
    named(68, 38, 1, 0x000, false, 2, 0, "rgba_000_422_68x38");
    named(1920, 16, 2, 0x300, true, 3, 0, "bgra_300_420_1920x16");
    printf("egress_rgb_check: %ld cases (%ld in the wide form) equal the pixel-by-pixel conversion; every alpha byte is 255, no byte outside "
           "the rows changed, the source planes are as they were\n",
           g_cases, g_wide);
    return 0;
}
