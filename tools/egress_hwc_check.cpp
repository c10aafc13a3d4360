// egress_hwc_check.cpp -- the body of k_egress_hwc (csrc/egress_hwc.h) run as plain C++ on the CPU, thread by thread, over a sweep of
// forms, element types, orders, presets, chroma formats, widths, heights, pitches, pointer offsets and constants; meant to be built with
// AddressSanitizer and UndefinedBehaviorSanitizer, which see every read outside the source planes' allocations (exact-size heap blocks:
// planes as dframe_alloc lays them out, and the luma also as the decoder stages it), every write outside the tensor's and every
// misaligned word access.  The program itself compares the tensor with the conversion and the float contract of include/dsv2_hip.h
// restated here element by element (nothing shared with the kernel's text: the binary16 rounding is done in integers), checks that no
// byte outside the h rows of 3 * w elements changed -- guard bytes in front, padding between the rows, guard bytes behind -- and that
// the source planes are as they were; and it runs egress_tensor.h's planar body on the same source with the constants permuted into
// channel order, and checks that the interleaved tensor is the planar one transposed.
// tests/test_egress_hwc_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/egress_hwc_check.cpp -o egress_hwc_check && ./egress_hwc_check [--dump DIR]
// --dump DIR writes, for a few named cases, NAME.yuv (the source planes, packed), NAME.const (scale[3], bias[3] by element position, as
// binary32) and NAME.hwc (h rows of 3 * w elements).  NAME = dtype_order_csc_format_WxH[_ramp], order "rgb" or "bgr".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "egress_hwc.h"
#include "egress_tensor.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::expect_pixel;
using support::kFmtName;
using support::kGuard;
using support::kHs;
using support::kLead; // guard bytes in front of and behind the tensor
using support::kPreset;
using support::kVs;
using support::preset_of;

// ---- the contract, restated: one element at a time, in the header's own terms ---------------------------------------------------
uint32_t bits_of(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

// binary32 bits to binary16 bits, round to nearest even, subnormals kept, overflow to infinity (finite or infinite input)
uint32_t half_of(uint32_t b)
{
    const uint32_t sign = (b >> 16) & 0x8000u, mag = b & 0x7fffffffu;
    if (mag >= 0x7f800000u) {
        return sign | 0x7c00u;
    }
    const int e = (int) (mag >> 23) - 127;
    if (e < -25) {
        return sign;
    }
    uint64_t m = (mag & 0x7fffffu) | 0x800000u;
    int drop;
    uint32_t base;
    if (e < -14) {
        drop = 13 + (-14 - e), base = 0;
    } else {
        drop = 13, base = (uint32_t) (e + 15 - 1) << 10;
    }
    const uint64_t q = m >> drop, rest = m & ((1ull << drop) - 1), half = 1ull << (drop - 1);
    uint32_t r = base + (uint32_t) q;
    if (rest > half || (rest == half && (q & 1))) {
        r++;
    }
    return sign | (r > 0x7c00u ? 0x7c00u : r);
}

uint32_t expect_elem(int dtype, uint8_t v, float scale, float bias)
{
    volatile float p = (float) v * scale; // (two operations, each rounded on its own)
    volatile float f = p + bias;
    const uint32_t b = bits_of(f);
    return dtype == kTensorF32 ? b : dtype == kTensorF16 ? half_of(b) : (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}

// element k of a pixel: channel kChannel[bgr][k] of R (0), G (1), B (2)
const int kChannel[2][3] = {{0, 1, 2}, {2, 1, 0}};

// ---- source planes: an exact-size heap block each ---------------------------------------------------------------------------------
struct Plane : support::Plane {
    Plane(int w_, int h_, bool bordered, unsigned seed) : support::Plane(w_, h_, bordered ? kBorder : 0, seed, support::noise_range_ends) {}
};

template <bool WIDE> void run_grid(const HwcOutJob &j)
{
    const int blocks = (j.h + 15) / 16;
    for (int bx = 0; bx < blocks; bx++) {
        for (int ty = 0; ty < 4; ty++) {
            const int y0 = (bx * 4 + ty) * 4;
            if (y0 >= j.h) {
                continue;
            }
            for (int tx = 0; tx < 64; tx++) {
                egress_hwc_rows<WIDE>(j, y0, tx * 4, 64 * 4);
            }
        }
    }
}

template <bool WIDE> void run_planar(const TensorOutJob &j)
{
    for (int y0 = 0; y0 < j.h; y0 += 4) {
        for (int tx = 0; tx < 64; tx++) {
            egress_tensor_rows<WIDE>(j, y0, tx * 4, 64 * 4);
        }
    }
}

const char *const kTypeName[4] = {"u8", "f16", "bf16", "f32"};
const char *const kOrderName[2] = {"rgb", "bgr"};
long g_cases = 0, g_wide = 0, g_planar = 0;
const char *g_dump = nullptr;

// scale[3], bias[3] by element position: tests/tensor_out.py's UNIT, IMAGENET, TINY (binary16 subnormals and zeros), HUGE (binary16
// overflow to infinity), and the three mixed
const float kConst[5][6] = {
    {(float) (1.0 / 255.0), (float) (1.0 / 255.0), (float) (1.0 / 255.0), 0.0f, 0.0f, 0.0f},
    {(float) (1.0 / (255.0 * 0.229)), (float) (1.0 / (255.0 * 0.224)), (float) (1.0 / (255.0 * 0.225)), (float) (-0.485 / 0.229), (float) (-0.456 / 0.224),
     (float) (-0.406 / 0.225)},
    {1e-7f, 1e-7f, 1e-7f, 0.0f, 0.0f, 0.0f},
    {300.0f, 300.0f, 300.0f, -5.0f, -5.0f, -5.0f},
    {1e-7f, (float) (1.0 / (255.0 * 0.224)), 300.0f, 0.0f, (float) (-0.456 / 0.224), -5.0f}};

size_t pitch_of(int w, int elem, int pitch_kind)
{
    const size_t rb = 3 * (size_t) w * (size_t) elem, up = (rb + 255) & ~(size_t) 255;
    return pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + (size_t) elem : up;
}

[[noreturn]] void mismatch(const char *what, int w, int h, int dtype, int bgr, int fmt, int csc, size_t pitch, int offset, int konst, bool wide, long rel, uint8_t got,
                           uint8_t want)
{
    fprintf(stderr, "MISMATCH (%s) %dx%d %s %s %s csc=0x%x pitch=%zu offset=%d consts=%d wide=%d: byte %ld (row %ld, byte %ld of it) is %02x, expected %02x\n", what,
            w, h, kTypeName[dtype], kOrderName[bgr], kFmtName[fmt], csc, pitch, offset, konst, (int) wide, rel, rel >= 0 ? rel / (long) pitch : -1L,
            rel >= 0 ? rel % (long) pitch : rel, got, want);
    exit(1);
}

// offset: elements behind a 16-byte boundary; force_general: run the general form even where the wide one would be picked (a round
// takes it when ANY of its tensors needs it)
void check(const Plane &Y, const Plane &U, const Plane &V, int fmt, int csc, int dtype, int bgr, int pitch_kind, int offset, int konst, bool force_general,
           const char *dump_name = nullptr)
{
    const int w = Y.w, h = Y.h, hs = kHs[fmt], vs = kVs[fmt], elem = tensor_elem(dtype);
    const size_t rb = 3 * (size_t) w * (size_t) elem, pitch = pitch_of(w, elem, pitch_kind);
    const size_t start = (size_t) kLead + (size_t) offset * (size_t) elem;
    const size_t bytes = start + (size_t) (h - 1) * pitch + rb + kLead;
    const long *p = kPreset[preset_of(csc)];
    const float *k = kConst[konst];
    const int *ch = kChannel[bgr];
    uint8_t *alloc;
    if (posix_memalign((void **) &alloc, 16, bytes) != 0) {
        abort();
    }
    memset(alloc, kGuard, bytes);
    HwcOutJob j{};
    j.sy = Y.org, j.su = U.org, j.sv = V.org, j.ystride = Y.stride, j.cstride = U.stride, j.w = w, j.h = h, j.hs = hs, j.vs = vs;
    j.csc = RgbOutCoefs{(int) p[0], (int) p[1], (int) p[2], (int) p[3], (int) p[4], (int) p[5]}, j.dtype = dtype, j.bgra = bgr;
    j.dst = alloc + start, j.dpitch = (int) pitch;
    for (int e = 0; e < 3; e++) {
        j.scale[e] = k[e], j.bias[e] = k[3 + e];
    }
    const bool wide = hwc_job_wide(j) && !force_general;
    wide ? run_grid<true>(j) : run_grid<false>(j);
    g_cases++;
    g_wide += wide;
    // the contract, element by element, guard bytes everywhere else
    std::vector<uint8_t> want(bytes, kGuard);
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            uint8_t px[3];
            expect_pixel(csc, Y.at(x, y), U.at(x >> hs, y >> vs), V.at(x >> hs, y >> vs), px);
            for (int e = 0; e < 3; e++) {
                uint8_t *at = &want[start + (size_t) y * pitch + (size_t) (3 * x + e) * (size_t) elem];
                if (dtype == kTensorU8) {
                    at[0] = px[ch[e]];
                } else {
                    const uint32_t v = expect_elem(dtype, px[ch[e]], k[e], k[3 + e]);
                    memcpy(at, &v, (size_t) elem); // (little endian)
                }
            }
        }
    }
    if (memcmp(want.data(), alloc, bytes) != 0) {
        size_t i = 0;
        while (want[i] == alloc[i]) {
            i++;
        }
        mismatch("contract", w, h, dtype, bgr, fmt, csc, pitch, offset, konst, wide, (long) i - (long) start, alloc[i], want[i]);
    }
    if (!Y.unchanged() || !U.unchanged() || !V.unchanged()) {
        fprintf(stderr, "a source plane was written: %dx%d %s %s pitch=%zu offset=%d\n", w, h, kTypeName[dtype], kFmtName[fmt], pitch, offset);
        exit(1);
    }
    // egress_tensor.h's planar output of the same source, the constants of channel c those of the element it lands in, transposed
    {
        const size_t prb = (size_t) w * (size_t) elem;
        std::vector<uint8_t> planes(3 * prb * (size_t) h + 16);
        uint8_t *base = (uint8_t *) (((uintptr_t) planes.data() + 15) & ~(uintptr_t) 15);
        TensorOutJob t{};
        t.sy = Y.org, t.su = U.org, t.sv = V.org, t.ystride = Y.stride, t.cstride = U.stride, t.w = w, t.h = h, t.hs = hs, t.vs = vs;
        t.csc = j.csc, t.dtype = dtype;
        for (int e = 0; e < 3; e++) {
            t.dst[ch[e]] = base + (size_t) ch[e] * prb * (size_t) h, t.dpitch[ch[e]] = (int) prb;
            t.scale[ch[e]] = k[e], t.bias[ch[e]] = k[3 + e];
        }
        tensor_job_wide(t) ? run_planar<true>(t) : run_planar<false>(t);
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                for (int e = 0; e < 3; e++) {
                    const uint8_t *a = j.dst + (size_t) y * pitch + (size_t) (3 * x + e) * (size_t) elem;
                    const uint8_t *b = t.dst[ch[e]] + (size_t) y * prb + (size_t) x * (size_t) elem;
                    if (memcmp(a, b, (size_t) elem) != 0) {
                        mismatch("planar transposed", w, h, dtype, bgr, fmt, csc, pitch, offset, konst, wide, (long) (a - j.dst), a[0], b[0]);
                    }
                }
            }
        }
        g_planar++;
    }
    if (dump_name && g_dump) {
        FILE *fy = support::dump_open(g_dump, dump_name, ".yuv"), *fc = support::dump_open(g_dump, dump_name, ".const"),
             *fh = support::dump_open(g_dump, dump_name, ".hwc");
        const Plane *pl[3] = {&Y, &U, &V};
        for (int c = 0; c < 3; c++) {
            support::dump_rows(fy, pl[c]->org, (size_t) pl[c]->stride, (size_t) pl[c]->w, pl[c]->h);
        }
        fwrite(k, sizeof(float), 6, fc);
        support::dump_rows(fh, j.dst, pitch, rb, h);
        fclose(fy);
        fclose(fc);
        fclose(fh);
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

void named(int w, int h, int fmt, int csc, int dtype, int bgr, int pitch_kind, int offset, int konst)
{
    Source s(w, h, fmt, false);
    char name[96];
    snprintf(name, sizeof name, "%s_%s_%03x_%s_%dx%d", kTypeName[dtype], kOrderName[bgr], csc, kFmtName[fmt], w, h);
    check(s.Y, s.U, s.V, fmt, csc, dtype, bgr, pitch_kind, offset, konst, false, name);
}

// full range, U = V = 128, Y a ramp over 32 x 8 pixels: R = G = B = Y, so all 256 byte values occur in every element
void grey_ramp(int dtype, int bgr, int konst)
{
    Source s(32, 8, 2, false);
    s.Y.fill([](int x, int y) { return (32 * y + x) & 255; });
    s.U.fill([](int, int) { return 128; });
    s.V.fill([](int, int) { return 128; });
    char name[96];
    snprintf(name, sizeof name, "%s_%s_200_420_32x8_ramp", kTypeName[dtype], kOrderName[bgr]);
    check(s.Y, s.U, s.V, 2, 0x200, dtype, bgr, 0, 0, konst, false, name);
    check(s.Y, s.U, s.V, 2, 0x200, dtype, bgr, 1, 1, konst, false);
}

} // namespace

int main(int argc, char **argv)
{
    if (!support::dump_option(argc, argv, &g_dump)) {
        return 2;
    }
    static const int cscs[4] = {0x000, 0x100, 0x200, 0x300};
    static const int ws[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 255, 256, 257, 260}, hts[] = {1, 2, 3, 4, 5, 16, 17};
    long turn = 0;
    for (int w : ws) {
        for (int h : hts) {
            for (int fmt = 0; fmt < 5; fmt++) {
                const Source s(w, h, fmt, false), staged(w, h, fmt, true);
                for (int csc : cscs) {
                    for (int dtype = 0; dtype < 4; dtype++) {
                        for (int bgr = 0; bgr < 2; bgr++) {
                            for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                                for (int offset = 0; offset < 4; offset++, turn++) {
                                    const Source &src = (turn & 1) ? staged : s;
                                    const int konst = (int) (turn % 5);
                                    check(src.Y, src.U, src.V, fmt, csc, dtype, bgr, pitch_kind, offset, konst, false); // wide where everything allows
                                    if (offset == 0 && w % 4 == 0 && pitch_of(w, tensor_elem(dtype), pitch_kind) % (size_t) (4 * tensor_elem(dtype)) == 0) {
                                        check(src.Y, src.U, src.V, fmt, csc, dtype, bgr, pitch_kind, offset, konst, true); // general on an aligned tensor
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
        fprintf(stderr, "FAILED: the sweep holds only one form\n");
        return 1;
    }
    for (int dtype = 0; dtype < 4; dtype++) {
        for (int bgr = 0; bgr < 2; bgr++) {
            for (int konst = 0; konst < 5; konst++) {
                grey_ramp(dtype, bgr, konst); // (dumped once per element type and order: the last constants stay in the file)
            }
        }
    }
    named(22, 18, 2, 0x000, kTensorU8, 1, 1, 1, 0);
    named(18, 18, 4, 0x300, kTensorU8, 0, 1, 3, 0);
    named(18, 18, 3, 0x100, kTensorF16, 1, 0, 2, 1);
    named(17, 16, 0, 0x200, kTensorBF16, 0, 0, 0, 1);
    named(68, 38, 1, 0x000, kTensorF32, 1, 2, 0, 1);
    named(260, 16, 2, 0x300, kTensorF16, 0, 2, 0, 2);  // binary16 subnormals and zeros
    named(36, 20, 2, 0x100, kTensorF16, 1, 2, 0, 3);   // binary16 overflow to infinity
    named(34, 18, 1, 0x200, kTensorBF16, 1, 1, 1, 4);
    named(34, 18, 0, 0x300, kTensorF32, 0, 1, 1, 4);
    named(516, 16, 2, 0x000, kTensorU8, 0, 2, 0, 0);   // a row of more than one pass
    named(20, 17, 0, 0x100, kTensorF32, 1, 0, 0, 0);
    printf("egress_hwc_check: %ld cases (%ld in the wide form) equal the element-by-element contract and the planar tensor transposed "
           "(%ld); no byte outside the rows changed, the source planes are as they were\n",
           g_cases, g_wide, g_planar);
    return 0;
}
