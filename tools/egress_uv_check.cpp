// egress_uv_check.cpp -- the body of k_egress_uv (csrc/egress_uv.h) run as plain C++ on the CPU, thread by thread, over a sweep
// of widths, heights, pitches, pointer offsets and modes; meant to be built with AddressSanitizer and
// UndefinedBehaviorSanitizer, which see every read outside a source plane's allocation, every write outside the destination's
// and every misaligned word access.  The program itself checks the delivered bytes against the conversions written out
// sample by sample, and that no byte outside the rows changed.  A development aid, not part of the test suite:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/egress_uv_check.cpp -o egress_uv_check && ./egress_uv_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "egress_uv.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::kGuard;

struct Plane : support::Plane { // as dframe_alloc lays one out: 32-pixel border, stride a multiple of 16, 16-byte aligned origin
    Plane(int w_, int h_, unsigned seed) : support::Plane(w_, h_, kBorder, seed, support::noise_plain) {}
};

int imin(int a, int b) { return a < b ? a : b; }

// util.c:79-153 of the reference CLI, sample by sample (k_to420, frame.hip)
int expect(const Plane &s, int mode, int x, int y)
{
    const int y0 = 2 * y, y1 = imin(y0 + 1, s.h - 1);
    switch (mode) {
    case 0:
        return s.at(x, y);
    case 1: {
        const int x0 = 2 * x, x1 = imin(x0 + 1, s.w - 1);
        const int a = (s.at(x0, y0) + s.at(x1, y0) + 1) >> 1, b = (s.at(x0, y1) + s.at(x1, y1) + 1) >> 1;
        return (a + b + 1) >> 1;
    }
    case 2:
        return (s.at(x, y0) + s.at(x, y1) + 1) >> 1;
    case 3:
        return (s.at(imin(x >> 1, s.w - 1), y0) + s.at(imin(x >> 1, s.w - 1), y1) + 1) >> 1;
    default:
        return s.at(imin(x >> 1, s.w - 1), imin(y >> 1, s.h - 1));
    }
}

template <int VEC, bool CONV> void run_grid(const UvEgressJob &j)
{
    const int blocks = (j.ch + 15) / 16; // (the launch's grid: sized by the delivered rows)
    for (int bx = 0; bx < blocks; bx++) {
        for (int ty = 0; ty < 4; ty++) {
            const int y0 = (bx * 4 + ty) * 4;
            if (y0 >= j.ch) {
                continue;
            }
            for (int tx = 0; tx < 64; tx++) {
                egress_uv_rows<VEC, CONV>(j, y0, tx * VEC, 64 * VEC);
            }
        }
    }
}

long g_cases = 0, g_wide = 0;

void check(int w, int h, int mode, int pitch_kind, int offset, bool conv_kernel)
{
    // luma w x h; source chroma by the stream's format, delivered chroma 4:2:0 (mode 0: the source's own size, any w x h)
    static const int shs[5] = {0, 0, 1, 2, 2}, svs[5] = {0, 0, 0, 0, 2};
    const int sw = mode ? (w + (1 << shs[mode]) - 1) >> shs[mode] : w, sh = mode ? (h + (1 << svs[mode]) - 1) >> svs[mode] : h;
    const int cw = mode ? (w + 1) >> 1 : w, ch = mode ? (h + 1) >> 1 : h;
    Plane U(sw, sh, 17u * (unsigned) w + (unsigned) h), V(sw, sh, 31u * (unsigned) w + (unsigned) h + 7u);
    const int rb = 2 * cw;
    const int pitch = pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + 1 : pitch_kind == 2 ? rb + 3 : ((rb + 15) & ~15) + 16;
    const size_t bytes = (size_t) offset + (size_t) (ch - 1) * pitch + rb; // not one byte more: the last row has no padding behind it
    uint8_t *alloc = (uint8_t *) aligned_alloc(16, (bytes + 15) & ~(size_t) 15);
    // (aligned_alloc rounds the size up: what lies behind `bytes` is compared below instead)
    const size_t whole = (bytes + 15) & ~(size_t) 15;
    memset(alloc, kGuard, whole);
    UvEgressJob j{U.org, V.org, alloc + offset, pitch, U.stride, sw, sh, cw, ch, mode};
    const bool wide = uv_job_wide(j);
    if (wide) {
        conv_kernel ? run_grid<8, true>(j) : run_grid<8, false>(j);
        g_wide++;
    } else {
        conv_kernel ? run_grid<4, true>(j) : run_grid<4, false>(j);
    }
    g_cases++;
    std::vector<uint8_t> want(whole, kGuard);
    for (int y = 0; y < ch; y++) {
        for (int x = 0; x < cw; x++) {
            want[(size_t) offset + (size_t) y * pitch + 2 * x] = (uint8_t) expect(U, mode, x, y);
            want[(size_t) offset + (size_t) y * pitch + 2 * x + 1] = (uint8_t) expect(V, mode, x, y);
        }
    }
    if (memcmp(want.data(), alloc, whole) != 0) {
        size_t i = 0;
        while (want[i] == alloc[i]) {
            i++;
        }
        fprintf(stderr, "MISMATCH w=%d h=%d mode=%d pitch=%d offset=%d conv_kernel=%d wide=%d at byte %zu: %02x, expected %02x\n", w, h, mode, pitch,
                offset, (int) conv_kernel, (int) wide, i, alloc[i], want[i]);
        exit(1);
    }
    free(alloc);
}

} // namespace

int main()
{
    std::vector<int> ws, hs;
    for (int w = 1; w <= 40; w++) {
        ws.push_back(w);
    }
    for (int w : {63, 64, 65, 176, 177, 330, 354, 511, 512, 513, 1031, 1040, 2080}) { // (rows of more than one pass of the 64 lanes in either form)
        ws.push_back(w);
    }
    for (int h = 1; h <= 10; h++) {
        hs.push_back(h);
    }
    for (int h : {15, 16, 17, 33, 67}) {
        hs.push_back(h);
    }
    for (int w : ws) {
        for (int h : hs) {
            for (int mode = 0; mode <= 4; mode++) {
                for (int pitch_kind = 0; pitch_kind < 4; pitch_kind++) {
                    for (int offset : {0, 1, 2, 3, 16}) {
                        check(w, h, mode, pitch_kind, offset, true); // the converting instantiation serves every mode
                        if (mode == 0) {
                            check(w, h, mode, pitch_kind, offset, false);
                        }
                    }
                }
            }
        }
    }
    printf("egress_uv_check: %ld cases (%ld in the wide form) equal the sample-by-sample conversions; no byte outside the rows changed\n", g_cases,
           g_wide);
    return 0;
}
