// egress_scale_check.cpp -- the body of k_egress_scale (csrc/egress_scale.h) run as plain C++ on the CPU, thread by thread, over a sweep
// of shifts, forms, plane widths and heights, pitches and pointer offsets; meant to be built with AddressSanitizer and
// UndefinedBehaviorSanitizer, which see every read outside the source plane's allocation (an exact-size heap block: a plane as
// dframe_alloc lays it out, or the luma as the decoder stages it for drawn-on / sharpened pictures -- no border, nothing behind the
// last row's stride), every write outside the destination's and every misaligned word access.  The program itself compares the
// destination with the reduction of include/dsv2_hip.h restated here sample by sample (nothing shared with the kernel's text), and
// checks that no byte outside the oh rows of ow bytes changed -- guard bytes in front, padding between the rows, guard bytes behind --
// and that the source plane is as it was.  A destination may also be the decoder's staging picture: rows of a 16-byte stride, which
// the wide form may write up to the stride, nothing in front of the first or behind the last row.
// tests/test_egress_scale_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/egress_scale_check.cpp -o egress_scale_check && ./egress_scale_check [--dump DIR]
// --dump DIR writes, for a few named cases, NAME.src (the source plane, packed) and NAME.out (the reduced plane, packed).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "egress_scale.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::kGuard;
using support::kLead;                    // guard bytes in front of and behind the destination
constexpr int kLanes = 8, kRows = 32;  // k_egress_scale's workgroup (egress.hip): threads along a row, output rows

struct Plane : support::Plane {
    // bordered: as dframe_alloc lays a plane out (32-pixel border, stride a multiple of 16, 16-byte aligned origin); else as the
    // decoder stages a luma plane: no border, stride = w rounded up to 16, h rows
    Plane(int w_, int h_, bool bordered, unsigned seed) : support::Plane(w_, h_, bordered ? kBorder : 0, seed, support::noise_extremes) {}
};

// ---- the reduction, restated: one sample at a time, in the header's own terms -------------------------------------------------------
uint8_t expect_sample(const Plane &p, int s, int x, int y)
{
    const int n = 1 << s;
    long sum = 0;
    for (int j = 0; j < n; j++) {
        for (int i = 0; i < n; i++) {
            const int sx = x * n + i < p.w - 1 ? x * n + i : p.w - 1, sy = y * n + j < p.h - 1 ? y * n + j : p.h - 1;
            sum += p.at(sx, sy);
        }
    }
    return (uint8_t) ((sum + (1L << (2 * s - 1))) >> (2 * s));
}

template <bool WIDE> void run_grid(const ScaleOutJob &j)
{
    const int oh = (j.ph + (1 << j.shift) - 1) >> j.shift;
    for (int bx = 0; bx < (oh + kRows - 1) / kRows; bx++) {
        for (int ty = 0; ty < kRows; ty++) {
            const int oy = bx * kRows + ty;
            if (oy >= oh) {
                continue;
            }
            for (int tx = 0; tx < kLanes; tx++) {
                egress_scale_row<WIDE>(j, bx * kRows, ty, tx, kLanes);
            }
        }
    }
}

long g_cases = 0, g_wide = 0;
const char *g_dump = nullptr;

// pitch kinds 0 .. 2: a caller's plane, tight / + 1 / aligned with room; 3: the decoder's staging picture (stride = ow rounded up to 16)
size_t pitch_of(int ow, int pitch_kind)
{
    const size_t up = ((size_t) ow + 15) & ~(size_t) 15;
    return pitch_kind == 0 ? (size_t) ow : pitch_kind == 1 ? (size_t) ow + 1 : pitch_kind == 2 ? up + 16 : up;
}

// force_general: run the general form even where the wide one would be picked (a round takes it when ANY of its jobs needs it)
void check(const Plane &P, int s, int pitch_kind, int offset, bool force_general, const char *dump_name = nullptr)
{
    const int n = 1 << s, ow = (P.w + n - 1) >> s, oh = (P.h + n - 1) >> s;
    const bool staging = pitch_kind == 3;
    const size_t pitch = pitch_of(ow, pitch_kind), row_room = staging ? pitch : (size_t) ow;
    const size_t start = (size_t) kLead + (size_t) offset;
    const size_t bytes = start + (size_t) (oh - 1) * pitch + row_room + kLead;
    uint8_t *alloc = nullptr;
    if (posix_memalign((void **) &alloc, 16, bytes) != 0) {
        abort();
    }
    memset(alloc, kGuard, bytes);
    uint8_t *dst = alloc + start;
    const ScaleOutJob j{P.org, dst, P.stride, P.w, P.h, (int) pitch, s};
    const bool wide = scale_job_wide(j, (int) row_room) && !force_general;
    wide ? run_grid<true>(j) : run_grid<false>(j);
    g_cases++;
    g_wide += wide;
    std::vector<uint8_t> want(bytes, kGuard);
    for (int y = 0; y < oh; y++) {
        for (int x = 0; x < ow; x++) {
            want[start + (size_t) y * pitch + (size_t) x] = expect_sample(P, s, x, y);
        }
        if (staging) { // (the bytes between the row and its stride are the staging picture's own: written or not)
            memcpy(&want[start + (size_t) y * pitch + (size_t) ow], dst + (size_t) y * pitch + (size_t) ow, row_room - (size_t) ow);
        }
    }
    if (memcmp(want.data(), alloc, bytes) != 0) {
        size_t i = 0;
        while (want[i] == alloc[i]) {
            i++;
        }
        const long rel = (long) i - (long) start;
        fprintf(stderr, "MISMATCH %dx%d shift=%d pitch=%zu offset=%d wide=%d staging=%d: byte %ld of the destination (row %ld, byte %ld of it) is %02x, expected %02x\n",
                P.w, P.h, s, pitch, offset, (int) wide, (int) staging, rel, rel >= 0 ? rel / (long) pitch : -1L, rel >= 0 ? rel % (long) pitch : rel, alloc[i],
                want[i]);
        exit(1);
    }
    if (!P.unchanged()) {
        fprintf(stderr, "the source plane was written: %dx%d shift=%d pitch=%zu offset=%d\n", P.w, P.h, s, pitch, offset);
        exit(1);
    }
    if (dump_name && g_dump) {
        FILE *fs = fopen((std::string(g_dump) + "/" + dump_name + ".src").c_str(), "wb");
        FILE *fo = fopen((std::string(g_dump) + "/" + dump_name + ".out").c_str(), "wb");
        if (!fs || !fo) {
            fprintf(stderr, "cannot write into %s\n", g_dump);
            exit(1);
        }
        for (int y = 0; y < P.h; y++) {
            fwrite(P.org + (size_t) y * P.stride, 1, (size_t) P.w, fs);
        }
        for (int y = 0; y < oh; y++) {
            fwrite(dst + (size_t) y * pitch, 1, (size_t) ow, fo);
        }
        fclose(fs);
        fclose(fo);
    }
    free(alloc);
}

// NAME = s<shift>_<form>_<w>x<h>
void named(int w, int h, int s, int pitch_kind, int offset, bool force_general, bool bordered)
{
    const Plane p(w, h, bordered, 48271u * (unsigned) w + 16807u * (unsigned) h + (unsigned) s);
    const int ow = (w + (1 << s) - 1) >> s;
    const size_t pitch = pitch_of(ow, pitch_kind);
    const bool wide = !force_general && offset % 8 == 0 && pitch % 8 == 0 && (pitch_kind == 3 ? pitch : (size_t) ow) % (size_t) (16 >> s) == 0;
    char name[64];
    snprintf(name, sizeof name, "s%d_%s_%dx%d", s, wide ? "wide" : "general", w, h);
    check(p, s, pitch_kind, offset, force_general, name);
}

} // namespace

int main(int argc, char **argv)
{
    if (!support::dump_option(argc, argv, &g_dump)) {
        return 2;
    }
    std::vector<int> ws;
    for (int w = 1; w <= 40; w++) {
        ws.push_back(w);
    }
    for (int w = 63; w <= 66; w++) {
        ws.push_back(w);
    }
    ws.push_back(130); // (a second pass of two bytes: a pass of the eight lanes is 128 source bytes)
    ws.push_back(300); // (three passes, the last one partial)
    long turn = 0;
    for (int w : ws) {
        for (int h = 1; h <= 18; h++) {
            const Plane bordered(w, h, true, 977u * (unsigned) w + 31u * (unsigned) h), staged(w, h, false, 7919u * (unsigned) w + 13u * (unsigned) h);
            for (int s = 1; s <= 3; s++) {
                for (int pitch_kind = 0; pitch_kind < 4; pitch_kind++) {
                    for (int offset = 0; offset < 4; offset++, turn++) {
                        if (pitch_kind == 3 && offset) { // (the staging picture is 16-byte aligned)
                            continue;
                        }
                        const Plane &src = (turn & 1) ? staged : bordered;
                        check(src, s, pitch_kind, offset, false); // wide where everything allows
                        const int ow = (w + (1 << s) - 1) >> s;
                        if (scale_job_wide(ScaleOutJob{nullptr, nullptr, 0, w, h, (int) pitch_of(ow, pitch_kind), s}, pitch_kind == 3 ? (int) pitch_of(ow, 3) : ow) &&
                            offset == 0) {
                            check(src, s, pitch_kind, offset, true); // general on a destination that allows the wide form
                        }
                    }
                }
            }
        }
    }
    // a plane taller than a workgroup's 32 output rows
    for (int s = 1; s <= 3; s++) {
        const Plane tall(18, 33 * (1 << s) + 1, true, 5u + (unsigned) s);
        check(tall, s, 1, 1, false);
        check(tall, s, 3, 0, false);
    }
    //    w    h  s  pitch offset general bordered
    named(32, 16, 1, 2, 0, false, true);
    named(34, 18, 1, 1, 1, false, true);
    named(33, 17, 1, 0, 3, false, false);
    named(64, 16, 2, 2, 0, false, true);
    named(35, 17, 2, 1, 2, false, true);
    named(18, 16, 2, 0, 0, true, false);
    named(64, 32, 3, 2, 0, false, true);
    named(18, 16, 3, 3, 0, false, true); // (the staging picture: wide at any width)
    named(37, 19, 3, 1, 3, false, false);
    named(130, 9, 3, 0, 1, false, true);
    named(300, 7, 1, 1, 0, false, true);
    named(304, 8, 2, 2, 0, false, true);
    printf("egress_scale_check: %ld cases (%ld in the wide form) equal the sample-by-sample reduction; no byte outside the rows changed, "
           "the source planes are as they were\n",
           g_cases, g_wide);
    return 0;
}
