// egress_resize_check.cpp -- the body of k_egress_resize (csrc/egress_resize.h) run as plain C++ on the CPU, thread by thread, over a
// sweep of sizes, forms, pitches and pointer offsets; meant to be built with AddressSanitizer and UndefinedBehaviorSanitizer, which see
// every read outside the source plane's allocation (an exact-size heap block: a plane as dframe_alloc lays it out, or the luma as the
// decoder stages it -- no border, nothing behind the last row's stride), every write outside the destination's and every misaligned
// word access.  The program itself compares the destination with the area average of include/dsv2_hip.h restated here sample by
// sample in 64-bit arithmetic with plain divisions (nothing shared with the kernel's text), and checks that no byte outside the oh
// rows of ow bytes changed -- guard bytes in front, padding between the rows, guard bytes behind -- and that the source plane is as it
// was.  A destination may also be the decoder's staging picture: rows of a 16-byte stride, which the wide form may write up to the
// stride, nothing in front of the first or behind the last row.  The division helper is checked on its own against `/`.
// tests/test_egress_resize_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/egress_resize_check.cpp -o egress_resize_check && ./egress_resize_check [--dump DIR]
// --dump DIR writes, for the named cases, NAME.src (the source plane, packed) and NAME.out (the resampled plane, packed), and
// allowed.txt: resize_allowed's verdict (io_jobs.h: the bounds of the call) on sizes at and around every bound, refused ones included, a
// line "pw ph ow oh verdict" each, which the test compares with the oracle's restatement of the bounds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "egress_resize.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::kGuard;
using support::kLead; // guard bytes in front of and behind the destination

struct Plane : support::Plane {
    // bordered: as dframe_alloc lays a plane out (32-pixel border, stride a multiple of 16, 16-byte aligned origin); else as the
    // decoder stages a luma plane: no border, stride = w rounded up to 16, h rows.  constant >= 0: the visible pixels hold that value
    // (border and padding keep their noise)
    Plane(int w_, int h_, bool bordered, unsigned seed, int constant = -1)
        : support::Plane(w_, h_, bordered ? kBorder : 0, seed, support::noise_extremes, constant)
    {
    }
};

long long gcd_of(long long x, long long y) { return y ? gcd_of(y, x % y) : x; }

// ---- the area average, restated: one sample at a time, in the header's own terms ------------------------------------------------------
uint8_t expect_sample(const Plane &p, int ow, int oh, int x, int y)
{
    const long long gx = gcd_of(p.w, ow), gy = gcd_of(p.h, oh);
    const long long a = p.w / gx, b = ow / gx, c = p.h / gy, d = oh / gy, D = a * c;
    long long sum = 0;
    for (long long j = y * c / d; j * d < (y + 1) * c; j++) {
        const long long wy = std::min((j + 1) * d, (y + 1) * c) - std::max(j * d, y * c);
        for (long long i = x * a / b; i * b < (x + 1) * a; i++) {
            const long long wx = std::min((i + 1) * b, (x + 1) * a) - std::max(i * b, x * a);
            if (wx <= 0 || wy <= 0 || i >= p.w || j >= p.h) {
                fprintf(stderr, "the restated formula left the plane: %dx%d -> %dx%d at (%d, %d)\n", p.w, p.h, ow, oh, x, y);
                exit(1);
            }
            sum += wy * wx * p.at((int) i, (int) j);
        }
    }
    return (uint8_t) ((sum + D / 2) / D);
}

// the kernel's grid (egress.hip): a thread per four samples of a row, threads past the plane return
template <bool WIDE> void run_grid(const ResizeOutJob &j)
{
    for (int y = 0; y < ((j.oh + 3) & ~3); y++) {
        for (int x0 = 0; x0 < ((j.ow + 255) & ~255); x0 += 4) {
            if (y >= j.oh || x0 >= j.ow) {
                continue;
            }
            egress_resize_quad<WIDE>(j, y, x0);
        }
    }
}

long g_cases = 0, g_wide = 0;
const char *g_dump = nullptr;

// pitch kinds 0 .. 2: a caller's plane, tight / + 1 / a multiple of 16 with room; 3: the decoder's staging picture (stride = ow rounded up to 16)
size_t pitch_of(int ow, int pitch_kind)
{
    const size_t up = ((size_t) ow + 15) & ~(size_t) 15;
    return pitch_kind == 0 ? (size_t) ow : pitch_kind == 1 ? (size_t) ow + 1 : pitch_kind == 2 ? up + 16 : up;
}

// force_general: run the general form even where the wide one would be picked (a round takes it when ANY of its jobs needs it).
// Returns whether the wide form ran.
bool check(const Plane &P, int ow, int oh, int pitch_kind, int offset, bool force_general, const char *dump_name = nullptr)
{
    if (!resize_allowed(P.w, P.h, ow, oh)) {
        fprintf(stderr, "not a size of the contract: %dx%d -> %dx%d\n", P.w, P.h, ow, oh);
        exit(1);
    }
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
    const ResizeOutJob j = resize_job(P.org, P.stride, P.w, P.h, dst, (int) pitch, ow, oh);
    const bool wide = resize_job_wide(j, (int) row_room) && !force_general;
    wide ? run_grid<true>(j) : run_grid<false>(j);
    g_cases++;
    g_wide += wide;
    std::vector<uint8_t> want(bytes, kGuard);
    for (int y = 0; y < oh; y++) {
        for (int x = 0; x < ow; x++) {
            want[start + (size_t) y * pitch + (size_t) x] = expect_sample(P, ow, oh, x, y);
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
        fprintf(stderr, "MISMATCH %dx%d -> %dx%d pitch=%zu offset=%d wide=%d staging=%d: byte %ld of the destination (row %ld, byte %ld of it) is %02x, expected %02x\n",
                P.w, P.h, ow, oh, pitch, offset, (int) wide, (int) staging, rel, rel >= 0 ? rel / (long) pitch : -1L, rel >= 0 ? rel % (long) pitch : rel,
                alloc[i], want[i]);
        exit(1);
    }
    if (!P.unchanged()) {
        fprintf(stderr, "the source plane was written: %dx%d -> %dx%d pitch=%zu offset=%d\n", P.w, P.h, ow, oh, pitch, offset);
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
    return wide;
}

// every destination for one plane and size: offsets 0 .. 3 with pitches ow, ow + 1 and a multiple of 16, the
// staging picture, and the general form wherever the wide one was picked.  Dumps NAME = <form>_<pw>x<ph>_<ow>x<oh>[_c<value>], once
// per form that occurs.
void shape(int pw, int ph, int ow, int oh, int constant = -1)
{
    const unsigned seed = 48271u * (unsigned) pw + 16807u * (unsigned) ph + 31u * (unsigned) ow + (unsigned) oh;
    const Plane bordered(pw, ph, true, seed, constant), staged(pw, ph, false, seed + 1, constant);
    bool dumped[2] = {false, false};
    int turn = 0;
    auto one = [&](int pitch_kind, int offset, bool force_general) {
        const Plane &src = (turn++ & 1) ? staged : bordered;
        char name[2][96];
        for (int f = 0; f < 2; f++) {
            const int n = snprintf(name[f], sizeof name[f], "%s_%dx%d_%dx%d", f ? "general" : "wide", pw, ph, ow, oh);
            if (constant >= 0) {
                snprintf(name[f] + n, sizeof name[f] - (size_t) n, "_c%d", constant);
            }
        }
        // (which form runs is known only inside: dump under the name of the form that has not been dumped yet, if this is it)
        const ResizeOutJob probe = resize_job(nullptr, 0, pw, ph, (uint8_t *) (uintptr_t) offset, (int) pitch_of(ow, pitch_kind), ow, oh);
        const bool wide = !force_general && resize_job_wide(probe, pitch_kind == 3 ? (int) pitch_of(ow, 3) : ow);
        const int f = wide ? 0 : 1;
        const bool ran_wide = check(src, ow, oh, pitch_kind, offset, force_general, dumped[f] ? nullptr : name[f]);
        if (ran_wide != wide) {
            fprintf(stderr, "form mismatch %dx%d -> %dx%d\n", pw, ph, ow, oh);
            exit(1);
        }
        dumped[f] = true;
        return wide;
    };
    for (int pitch_kind = 0; pitch_kind < 4; pitch_kind++) {
        for (int offset = 0; offset < (pitch_kind == 3 ? 1 : 4); offset++) { // (the staging picture is 16-byte aligned)
            if (one(pitch_kind, offset, false)) {
                one(pitch_kind, offset, true);
            }
        }
    }
}

// resize_div against `/`
void check_div(uint32_t n, uint32_t den)
{
    const uint32_t got = resize_div(n, den, resize_recip(den));
    if (got != n / den) {
        fprintf(stderr, "resize_div(%u, %u) = %u, not %u\n", n, den, got, n / den);
        exit(1);
    }
}

long check_divisions()
{
    long count = 0;
    const uint32_t Ds[] = {1, 2, 3, 9, 12, 64, 475, 1900, 5917, 2070601, (1u << 24) - 3, 1u << 24};
    const uint64_t ks[] = {0, 1, 2, 127, 128, 254, 255};
    for (uint32_t D : Ds) {
        const uint64_t top = 255ull * D + D / 2; // the largest sum the kernel divides
        for (uint64_t k : ks) {
            for (int e = -1; e <= 1; e++) {
                const int64_t s = (int64_t) (k * D) + e;
                if (s >= 0 && (uint64_t) s <= top) {
                    check_div((uint32_t) s, D);
                    count++;
                }
            }
        }
        check_div((uint32_t) top, D);
        count++;
        uint32_t seed = D;
        for (int i = 0; i < 20000; i++) {
            seed = seed * 1664525u + 1013904223u;
            check_div((uint32_t) ((uint64_t) seed % (top + 1)), D);
            count++;
        }
    }
    // the coordinate quotients: any denominator up to a plane's side, numerators up to 2^31 and the 32-bit extremes
    for (uint32_t den = 1; den <= 32768; den = den < 70 ? den + 1 : den * 2 - 3) {
        uint32_t seed = den * 2654435761u;
        for (int i = 0; i < 2000; i++) {
            seed = seed * 1664525u + 1013904223u;
            check_div(seed >> 1, den);
            check_div(seed, den);
            count += 2;
        }
        for (uint32_t k = 0; k < 300; k++) {
            check_div(k * den, den);
            check_div(k * den + den - 1, den);
            count += 2;
        }
        check_div(0xffffffffu, den);
        check_div(0x80000000u, den);
        count += 2;
    }
    return count;
}

// resize_allowed at and around every bound of the call: the ratio of 8 and of 1 per axis, sizes that are not positive, a side of
// 32 768 and beyond, D at and around 2^24 (4096^2 exactly; 4093 * 4099 just below; 4097^2, 4100^2 above; reached by one axis alone)
long dump_allowed()
{
    static const int cases[][4] = {
        {64, 48, 8, 6},         {64, 48, 7, 6},         {64, 48, 8, 5},         {64, 48, 64, 48},       {64, 48, 65, 48},       {64, 48, 64, 49},
        {65, 49, 9, 7},         {65, 49, 8, 7},         {65, 49, 9, 6},         {64, 48, 0, 0},         {64, 48, 0, 24},        {64, 48, 32, 0},
        {64, 48, -32, 24},      {64, 48, 32, -24},      {64, 48, -1, -1},       {1, 1, 1, 1},           {32768, 16, 32767, 16}, {32768, 16, 4096, 2},
        {32769, 16, 32768, 16}, {16, 32769, 16, 32768}, {16, 32768, 16, 32767}, {40000, 40000, 40000, 40000},
        {4096, 4096, 4095, 4095}, {4097, 4097, 4096, 4096}, {4093, 4099, 4092, 4098}, {4099, 4099, 4098, 4098}, {4100, 4100, 4099, 4099},
        {4100, 4100, 4098, 4098}, {4097, 4097, 2049, 2049}, {4097, 4097, 2049, 4097}, {4097, 4097, 4097, 2049}, {32768, 32768, 32767, 32768},
        {32768, 32768, 32767, 32766}, {32768, 513, 32767, 512}, {32768, 512, 32767, 511}, {32749, 521, 32748, 520}, {16384, 16384, 16383, 16383},
        {8194, 8194, 4097, 4097}, {8190, 8190, 4095, 4095}, {1919, 1079, 1279, 719}, {1920, 1080, 1280, 720}};
    if (!g_dump) {
        return 0;
    }
    FILE *f = fopen((std::string(g_dump) + "/allowed.txt").c_str(), "w");
    if (!f) {
        fprintf(stderr, "cannot write into %s\n", g_dump);
        exit(1);
    }
    long n = 0;
    for (const int(&c)[4] : cases) {
        fprintf(f, "%d %d %d %d %d\n", c[0], c[1], c[2], c[3], (int) resize_allowed(c[0], c[1], c[2], c[3]));
        n++;
    }
    fclose(f);
    return n;
}

} // namespace

int main(int argc, char **argv)
{
    if (!support::dump_option(argc, argv, &g_dump)) {
        return 2;
    }
    const long divisions = check_divisions();
    dump_allowed();
    // every size a small plane can take, one destination each (the kinds and offsets in turn)
    long turn = 0;
    for (int pw = 1; pw <= 20; pw++) {
        for (int ph = 1; ph <= 9; ph++) {
            const Plane bordered(pw, ph, true, 977u * (unsigned) pw + 31u * (unsigned) ph), staged(pw, ph, false, 7919u * (unsigned) pw + 13u * (unsigned) ph);
            for (int ow = (pw + 7) / 8; ow <= pw; ow++) {
                for (int oh = (ph + 7) / 8; oh <= ph; oh++, turn++) {
                    const int pitch_kind = (int) (turn % 4), offset = pitch_kind == 3 ? 0 : (int) ((turn / 4) % 4);
                    if (check((turn & 8) ? staged : bordered, ow, oh, pitch_kind, offset, false)) {
                        check((turn & 8) ? staged : bordered, ow, oh, pitch_kind, offset, true);
                    }
                }
            }
        }
    }
    static const int shapes[][4] = {{48, 32, 32, 24},  {50, 38, 33, 21},  {25, 19, 17, 11}, {64, 48, 9, 7},   {64, 48, 64, 6},   {64, 48, 8, 48},
                                    {16, 16, 16, 16},  {16, 16, 2, 2},    {64, 48, 32, 24}, {64, 48, 16, 12}, {97, 61, 13, 8},   {131, 67, 130, 66},
                                    {300, 9, 260, 5},  {1030, 5, 1028, 3}}; // (the last two: more than one workgroup along a row)
    for (const int(&s)[4] : shapes) {
        shape(s[0], s[1], s[2], s[3]);
        for (int constant : {0, 1, 254, 255}) {
            shape(s[0], s[1], s[2], s[3], constant);
        }
    }
    printf("egress_resize_check: %ld cases (%ld in the wide form) equal the sample-by-sample area average; no byte outside the rows changed, "
           "the source planes are as they were; %ld quotients of the division helper equal those of `/`\n",
           g_cases, g_wide, divisions);
    return 0;
}
