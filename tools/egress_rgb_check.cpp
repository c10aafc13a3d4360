// egress_rgb_check.cpp -- the body of k_egress_rgb (csrc/egress_rgb.h) run as plain C++ on the CPU, thread by thread, for its three
// layouts -- packed four-byte surfaces, planar and interleaved tensors -- over a sweep of forms, byte / element orders, element types,
// presets, chroma formats, widths, heights, pitches, pointer offsets and constants; meant to be built with AddressSanitizer and
// UndefinedBehaviorSanitizer, which see every read outside the source planes' allocations (exact-size heap blocks: planes as dframe_alloc
// lays them out, and the luma also as the decoder stages it for drawn-on / sharpened pictures -- no border, nothing behind the last
// row's stride), every write outside a destination's and every misaligned word access.
// THE CONTRACT, restated here once and shared with nothing of the kernel's text: every pixel converted by include/dsv2_hip.h's integer
// formulas (support::expect_pixel) into R, G, B; a packed pixel is the bytes B G R or R G B in the surface's order and 255; a tensor
// element is the byte (uint8) or fl32(fl32(byte * scale) + bias) rounded to the element type -- binary16 rounded in integers here --
// with the constants of its plane (planar) or of its position in the pixel (interleaved, R G B or B G R).  The program compares every
// destination with it byte for byte, guard bytes in front, padding between the rows and guard bytes behind included (no byte outside the
// h rows changed), checks that the source planes are as they were, and runs every interleaved case again as a planar one, the constants
// permuted into channel order, and checks that the interleaved tensor is the planar one transposed.
// tests/test_egress_rgb_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/egress_rgb_check.cpp -o egress_rgb_check && ./egress_rgb_check [--dump DIR]
// --dump DIR writes, for a few named cases, into DIR/packed, DIR/planar and DIR/interleaved: NAME.yuv (the source planes, packed) and
//   packed       NAME.rgb (h rows of 4 * w bytes); NAME = order_csc_format_WxH, order "bgra" or "rgba";
//   planar       NAME.const (scale[3], bias[3] as binary32) and NAME.ten (the planes R, G, B, h rows of w elements each);
//                NAME = dtype_csc_format_WxH[_ramp];
//   interleaved  NAME.const (by element position) and NAME.hwc (h rows of 3 * w elements); NAME = dtype_order_csc_format_WxH[_ramp],
//                order "rgb" or "bgr".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <string>
#include <vector>

#include "egress_rgb.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::kFmtName;
using support::kGuard;
using support::kHs;
using support::kLead; // guard bytes in front of and behind every destination
using support::kPreset;
using support::kVs;
using support::preset_of;

const char *const kLayoutName[kRgbOutLayouts] = {"packed", "planar", "interleaved"};
const char *const kTypeName[4] = {"u8", "f16", "bf16", "f32"};
const char *const kOrderName[2][2] = {{"rgba", "bgra"}, {"rgb", "bgr"}}; // packed; interleaved
const int kChannel[2][3] = {{0, 1, 2}, {2, 1, 0}};                        // byte / element k of a pixel: channel kChannel[bgr][k] of R, G, B

// ---- the contract, restated: one element at a time ----------------------------------------------------------------------------------
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
    const int e = (int) (mag >> 23) - 127; // unbiased exponent (zero and binary32 subnormals: -127, far below binary16's range)
    if (e < -25) {
        return sign; // below half of the smallest subnormal
    }
    uint64_t m = (mag & 0x7fffffu) | 0x800000u; // 1.23
    int drop;                                   // bits of m that go
    uint32_t base;
    if (e < -14) {
        drop = 13 + (-14 - e), base = 0; // subnormal: the value is m * 2^(e - 23), in units of 2^-24
    } else {
        drop = 13, base = (uint32_t) (e + 15 - 1) << 10; // the hidden bit adds the last exponent step
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
    if (dtype == kTensorU8) {
        return v;
    }
    volatile float p = (float) v * scale; // (two operations, each rounded on its own)
    volatile float f = p + bias;
    const uint32_t b = bits_of(f);
    return dtype == kTensorF32 ? b : dtype == kTensorF16 ? half_of(b) : (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}

// ---- source planes: an exact-size heap block each ---------------------------------------------------------------------------------
struct Plane : support::Plane {
    // bordered: as dframe_alloc lays a plane out (32-pixel border, stride a multiple of 16, 16-byte aligned origin); else as the
    // decoder stages a luma plane: no border, stride = w rounded up to 16, h rows
    Plane(int w_, int h_, bool bordered, unsigned seed) : support::Plane(w_, h_, bordered ? kBorder : 0, seed, support::noise_range_ends) {}
};

struct Source { // the three planes of a w x h picture of format fmt; staged: the luma as the decoder stages it
    Plane Y, U, V;
    Source(int w, int h, int fmt, bool staged)
        : Y(w, h, !staged, 977u * (unsigned) w + 31u * (unsigned) h + (unsigned) fmt),
          U((w + (1 << kHs[fmt]) - 1) >> kHs[fmt], (h + (1 << kVs[fmt]) - 1) >> kVs[fmt], true, 7919u * (unsigned) w + 13u * (unsigned) h + (unsigned) fmt),
          V((w + (1 << kHs[fmt]) - 1) >> kHs[fmt], (h + (1 << kVs[fmt]) - 1) >> kVs[fmt], true, 104729u * (unsigned) w + 7u * (unsigned) h + (unsigned) fmt)
    {
    }
};

// the kernel's grid: 16 rows a workgroup, 64 x 4 threads
template <int LAYOUT, bool WIDE> void run_grid(const RgbOutJob &j)
{
    const int blocks = (j.h + 15) / 16;
    for (int bx = 0; bx < blocks; bx++) {
        for (int ty = 0; ty < 4; ty++) {
            const int y0 = (bx * 4 + ty) * 4;
            if (y0 >= j.h) {
                continue;
            }
            for (int tx = 0; tx < 64; tx++) {
                egress_rgb_rows<LAYOUT, WIDE>(j, y0, tx * 4, 64 * 4);
            }
        }
    }
}
template <int LAYOUT> void run(const RgbOutJob &j, bool wide) { wide ? run_grid<LAYOUT, true>(j) : run_grid<LAYOUT, false>(j); }
void run(const RgbOutJob &j, bool wide)
{
    j.layout == kRgbOutPacked ? run<kRgbOutPacked>(j, wide) : j.layout == kRgbOutPlanar ? run<kRgbOutPlanar>(j, wide) : run<kRgbOutInterleaved>(j, wide);
}

long g_cases[kRgbOutLayouts] = {}, g_wide[kRgbOutLayouts] = {}, g_transposed = 0;
const char *g_dump = nullptr;

// scale[3], bias[3]: 1 / 255; ImageNet's Normalize folded (scale = 1 / (255 * std), bias = -mean / std); binary16 subnormals and zeros;
// binary16 overflow to infinity; the three mixed (tests/tensor_out.py's UNIT, IMAGENET, TINY, HUGE)
const float kConst[5][6] = {
    {(float) (1.0 / 255.0), (float) (1.0 / 255.0), (float) (1.0 / 255.0), 0.0f, 0.0f, 0.0f},
    {(float) (1.0 / (255.0 * 0.229)), (float) (1.0 / (255.0 * 0.224)), (float) (1.0 / (255.0 * 0.225)), (float) (-0.485 / 0.229), (float) (-0.456 / 0.224),
     (float) (-0.406 / 0.225)},
    {1e-7f, 1e-7f, 1e-7f, 0.0f, 0.0f, 0.0f},
    {300.0f, 300.0f, 300.0f, -5.0f, -5.0f, -5.0f},
    {1e-7f, (float) (1.0 / (255.0 * 0.224)), 300.0f, 0.0f, (float) (-0.456 / 0.224), -5.0f}};

int elems_per_pixel(int layout) { return layout == kRgbOutPacked ? 4 : layout == kRgbOutInterleaved ? 3 : 1; } // of a destination row
int elem_of(int layout, int dtype) { return layout == kRgbOutPacked ? 1 : tensor_elem(dtype); }

// each sweep's pitches: packed tight, + 1, 16 bytes behind the row rounded up to 16, 4 KiB behind it; planar tight, + 1 element, 16
// bytes behind the row rounded up to 16; interleaved tight, + 1 element, rounded up to 256
size_t pitch_of(int layout, int w, int dtype, int pitch_kind)
{
    const size_t elem = (size_t) elem_of(layout, dtype), rb = (size_t) elems_per_pixel(layout) * (size_t) w * elem, up = (rb + 15) & ~(size_t) 15;
    if (layout == kRgbOutPacked) {
        return pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + 1 : pitch_kind == 2 ? up + 16 : up + 4096;
    }
    return pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + elem : layout == kRgbOutPlanar ? up + 16 : (rb + 255) & ~(size_t) 255;
}

// one case: offset in elements behind a 16-byte boundary (packed: bytes); force_general: run the general form even where the wide one
// would be picked (a round takes it when ANY of its destinations needs it)
void check(const Source &src, int fmt, int csc, int layout, int dtype, int bgr, int pitch_kind, int offset, int konst, bool force_general,
           const char *dump_name = nullptr)
{
    const Plane &Y = src.Y, &U = src.U, &V = src.V;
    const int w = Y.w, h = Y.h, hs = kHs[fmt], vs = kVs[fmt], elem = elem_of(layout, dtype), E = elems_per_pixel(layout);
    const int nbuf = layout == kRgbOutPlanar ? 3 : 1;
    const size_t rb = (size_t) E * (size_t) w * (size_t) elem, pitch = pitch_of(layout, w, dtype, pitch_kind);
    const size_t start = (size_t) kLead + (size_t) offset * (size_t) elem;
    const size_t bytes = start + (size_t) (h - 1) * pitch + rb + kLead;
    const long *p = kPreset[preset_of(csc)];
    const float *k = kConst[konst];
    const int *ch = kChannel[bgr];
    RgbOutJob j{};
    j.sy = Y.org, j.su = U.org, j.sv = V.org, j.ystride = Y.stride, j.cstride = U.stride, j.w = w, j.h = h, j.hs = hs, j.vs = vs;
    j.csc = RgbOutCoefs{(int) p[0], (int) p[1], (int) p[2], (int) p[3], (int) p[4], (int) p[5]};
    j.bgra = bgr, j.layout = layout, j.dtype = layout == kRgbOutPacked ? kTensorU8 : dtype;
    uint8_t *alloc[3] = {nullptr, nullptr, nullptr};
    for (int b = 0; b < nbuf; b++) {
        if (posix_memalign((void **) &alloc[b], 16, bytes) != 0) {
            abort();
        }
        memset(alloc[b], kGuard, bytes);
        j.dst[b] = alloc[b] + start, j.dpitch[b] = (int) pitch;
    }
    for (int c = 0; c < 3; c++) {
        j.scale[c] = k[c], j.bias[c] = k[3 + c];
    }
    const bool wide = rgb_out_job_wide(j) && !force_general;
    run(j, wide);
    g_cases[layout]++;
    g_wide[layout] += wide;
    // the contract, element by element, guard bytes everywhere else
    std::vector<uint8_t> want[3];
    for (int b = 0; b < nbuf; b++) {
        want[b].assign(bytes, kGuard);
    }
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            uint8_t px[3];
            support::expect_pixel(csc, Y.at(x, y), U.at(x >> hs, y >> vs), V.at(x >> hs, y >> vs), px);
            for (int b = 0; b < nbuf; b++) {
                for (int e = 0; e < E; e++) {
                    const int c = layout == kRgbOutPlanar ? b : e < 3 ? ch[e] : -1, kk = layout == kRgbOutPlanar ? b : e; // channel; constants
                    const uint32_t v = c < 0 ? 255 : expect_elem(j.dtype, px[c], k[kk], k[3 + kk]);
                    memcpy(&want[b][start + (size_t) y * pitch + (size_t) (E * x + e) * (size_t) elem], &v, (size_t) elem); // (little endian)
                }
            }
        }
    }
    for (int b = 0; b < nbuf; b++) {
        if (memcmp(want[b].data(), alloc[b], bytes) != 0) {
            size_t i = 0;
            while (want[b][i] == alloc[b][i]) {
                i++;
            }
            const long rel = (long) i - (long) start;
            fprintf(stderr, "MISMATCH %s %dx%d %s %s order=%d csc=0x%x pitch=%zu offset=%d consts=%d wide=%d: byte %ld of destination %d (row %ld, byte %ld of it) is %02x, "
                    "expected %02x\n",
                    kLayoutName[layout], w, h, kTypeName[j.dtype], kFmtName[fmt], bgr, csc, pitch, offset, konst, (int) wide, rel, b, rel >= 0 ? rel / (long) pitch : -1L,
                    rel >= 0 ? rel % (long) pitch : rel, alloc[b][i], want[b][i]);
            exit(1);
        }
    }
    if (layout == kRgbOutPacked) { // (what the comparison above already implies, said on its own)
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                if (j.dst[0][(size_t) y * pitch + 4 * (size_t) x + 3] != 255) {
                    fprintf(stderr, "alpha of pixel (%d, %d) is not 255\n", x, y);
                    exit(1);
                }
            }
        }
    }
    if (!Y.unchanged() || !U.unchanged() || !V.unchanged()) {
        fprintf(stderr, "a source plane was written: %s %dx%d %s %s pitch=%zu offset=%d\n", kLayoutName[layout], w, h, kTypeName[j.dtype], kFmtName[fmt], pitch, offset);
        exit(1);
    }
    if (layout == kRgbOutInterleaved) { // the planar layout's output of the same source, the constants of channel c those of the element it lands in, transposed
        const size_t prb = (size_t) w * (size_t) elem;
        std::vector<uint8_t> planes(3 * prb * (size_t) h + 16);
        uint8_t *base = (uint8_t *) (((uintptr_t) planes.data() + 15) & ~(uintptr_t) 15);
        RgbOutJob t = j;
        t.layout = kRgbOutPlanar, t.bgra = 0;
        for (int e = 0; e < 3; e++) {
            t.dst[ch[e]] = base + (size_t) ch[e] * prb * (size_t) h, t.dpitch[ch[e]] = (int) prb;
            t.scale[ch[e]] = k[e], t.bias[ch[e]] = k[3 + e];
        }
        run(t, rgb_out_job_wide(t));
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                for (int e = 0; e < 3; e++) {
                    const uint8_t *a = j.dst[0] + (size_t) y * pitch + (size_t) (3 * x + e) * (size_t) elem;
                    const uint8_t *b = t.dst[ch[e]] + (size_t) y * prb + (size_t) x * (size_t) elem;
                    if (memcmp(a, b, (size_t) elem) != 0) {
                        fprintf(stderr, "MISMATCH (planar transposed) %dx%d %s %s %s csc=0x%x pitch=%zu offset=%d consts=%d wide=%d: element %d of pixel (%d, %d)\n", w, h,
                                kTypeName[dtype], kOrderName[1][bgr], kFmtName[fmt], csc, pitch, offset, konst, (int) wide, e, x, y);
                        exit(1);
                    }
                }
            }
        }
        g_transposed++;
    }
    if (dump_name && g_dump) {
        const std::string dir = std::string(g_dump) + "/" + kLayoutName[layout];
        FILE *fy = support::dump_open(dir.c_str(), dump_name, ".yuv");
        const Plane *pl[3] = {&Y, &U, &V};
        for (int c = 0; c < 3; c++) {
            support::dump_rows(fy, pl[c]->org, (size_t) pl[c]->stride, (size_t) pl[c]->w, pl[c]->h);
        }
        fclose(fy);
        if (layout != kRgbOutPacked) {
            FILE *fc = support::dump_open(dir.c_str(), dump_name, ".const");
            fwrite(k, sizeof(float), 6, fc);
            fclose(fc);
        }
        FILE *fo = support::dump_open(dir.c_str(), dump_name, layout == kRgbOutPacked ? ".rgb" : layout == kRgbOutPlanar ? ".ten" : ".hwc");
        for (int b = 0; b < nbuf; b++) {
            support::dump_rows(fo, j.dst[b], pitch, rb, h);
        }
        fclose(fo);
    }
    for (int b = 0; b < nbuf; b++) {
        free(alloc[b]);
    }
}

// a named case, dumped: packed with konst 0 (unused)
void named(int layout, int w, int h, int fmt, int csc, int dtype, int bgr, int pitch_kind, int offset, int konst)
{
    Source s(w, h, fmt, false);
    char name[96];
    if (layout == kRgbOutPacked) {
        snprintf(name, sizeof name, "%s_%03x_%s_%dx%d", kOrderName[0][bgr], csc, kFmtName[fmt], w, h);
    } else if (layout == kRgbOutPlanar) {
        snprintf(name, sizeof name, "%s_%03x_%s_%dx%d", kTypeName[dtype], csc, kFmtName[fmt], w, h);
    } else {
        snprintf(name, sizeof name, "%s_%s_%03x_%s_%dx%d", kTypeName[dtype], kOrderName[1][bgr], csc, kFmtName[fmt], w, h);
    }
    check(s, fmt, csc, layout, dtype, bgr, pitch_kind, offset, konst, false, name);
}

// full range, U = V = 128, Y a ramp over 32 x 8 pixels: R = G = B = Y, so all 256 byte values occur in every channel
void grey_ramp(int layout, int dtype, int bgr, int konst)
{
    Source s(32, 8, 2, false);
    s.Y.fill([](int x, int y) { return (32 * y + x) & 255; });
    s.U.fill([](int, int) { return 128; });
    s.V.fill([](int, int) { return 128; });
    char name[96];
    if (layout == kRgbOutPlanar) {
        snprintf(name, sizeof name, "%s_200_420_32x8_ramp", kTypeName[dtype]);
    } else {
        snprintf(name, sizeof name, "%s_%s_200_420_32x8_ramp", kTypeName[dtype], kOrderName[1][bgr]);
    }
    check(s, 2, 0x200, layout, dtype, bgr, 0, 0, konst, false, name);
    check(s, 2, 0x200, layout, dtype, bgr, 1, 1, konst, false);
}

} // namespace

int main(int argc, char **argv)
{
    if (!support::dump_option(argc, argv, &g_dump)) {
        return 2;
    }
    if (g_dump) {
        for (const char *l : kLayoutName) {
            mkdir((std::string(g_dump) + "/" + l).c_str(), 0755);
        }
    }
    static const int cscs[4] = {0x000, 0x100, 0x200, 0x300};
    // packed: every width to 40 and one of several passes of the 64 lanes, heights to 9, both byte orders, four pitches, four offsets
    std::vector<int> ws;
    for (int w = 1; w <= 40; w++) {
        ws.push_back(w);
    }
    ws.push_back(1920);
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
                                check(src, fmt, csc, kRgbOutPacked, kTensorU8, bgra, pitch_kind, offset, 0, false); // wide where everything allows
                                if (offset == 0 && w % 4 == 0 && pitch_of(kRgbOutPacked, w, kTensorU8, pitch_kind) % 16 == 0) {
                                    check(src, fmt, csc, kRgbOutPacked, kTensorU8, bgra, pitch_kind, offset, 0, true); // general on an aligned surface
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    // tensors: widths and heights around the quad and the pass, four element types, interleaved in both orders, three pitches, four offsets
    static const int tws[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 255, 256, 257, 260}, hts[] = {1, 2, 3, 4, 5, 16, 17};
    for (int layout : {kRgbOutPlanar, kRgbOutInterleaved}) {
        turn = 0;
        for (int w : tws) {
            for (int h : hts) {
                for (int fmt = 0; fmt < 5; fmt++) {
                    const Source s(w, h, fmt, false), staged(w, h, fmt, true);
                    for (int csc : cscs) {
                        for (int dtype = 0; dtype < 4; dtype++) {
                            for (int bgr = 0; bgr < (layout == kRgbOutInterleaved ? 2 : 1); bgr++) {
                                for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                                    for (int offset = 0; offset < 4; offset++, turn++) {
                                        const Source &src = (turn & 1) ? staged : s;
                                        const int konst = (int) (turn % 5);
                                        check(src, fmt, csc, layout, dtype, bgr, pitch_kind, offset, konst, false); // wide where everything allows
                                        if (offset == 0 && w % 4 == 0 && pitch_of(layout, w, dtype, pitch_kind) % (size_t) (4 * tensor_elem(dtype)) == 0) {
                                            check(src, fmt, csc, layout, dtype, bgr, pitch_kind, offset, konst, true); // general on an aligned tensor
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    for (int l = 0; l < kRgbOutLayouts; l++) {
        if (g_wide[l] == 0 || g_wide[l] == g_cases[l]) {
            fprintf(stderr, "FAILED: the %s sweep holds only one form\n", kLayoutName[l]);
            return 1;
        }
    }
    for (int dtype = 0; dtype < 4; dtype++) {
        for (int konst = 0; konst < 5; konst++) { // (dumped once per element type and order: the last constants stay in the file)
            grey_ramp(kRgbOutPlanar, dtype, 0, konst);
            grey_ramp(kRgbOutInterleaved, dtype, 0, konst);
            grey_ramp(kRgbOutInterleaved, dtype, 1, konst);
        }
    }
    named(kRgbOutPacked, 22, 18, 2, 0x000, kTensorU8, 1, 1, 1, 0);
    named(kRgbOutPacked, 18, 18, 4, 0x300, kTensorU8, 0, 1, 3, 0);
    named(kRgbOutPacked, 18, 18, 3, 0x100, kTensorU8, 0, 0, 2, 0);
    named(kRgbOutPacked, 17, 16, 0, 0x200, kTensorU8, 1, 0, 0, 0);
    named(kRgbOutPacked, 68, 38, 1, 0x000, kTensorU8, 0, 2, 0, 0);
    named(kRgbOutPacked, 1920, 16, 2, 0x300, kTensorU8, 1, 3, 0, 0);
    named(kRgbOutPlanar, 22, 18, 2, 0x000, kTensorU8, 0, 1, 1, 0);
    named(kRgbOutPlanar, 18, 18, 4, 0x300, kTensorU8, 0, 1, 3, 0);
    named(kRgbOutPlanar, 18, 18, 3, 0x100, kTensorF16, 0, 0, 2, 1);
    named(kRgbOutPlanar, 17, 16, 0, 0x200, kTensorBF16, 0, 0, 0, 1);
    named(kRgbOutPlanar, 68, 38, 1, 0x000, kTensorF32, 0, 2, 0, 1);
    named(kRgbOutPlanar, 260, 16, 2, 0x300, kTensorF16, 0, 2, 0, 2); // binary16 subnormals and zeros
    named(kRgbOutPlanar, 36, 20, 2, 0x100, kTensorF16, 0, 2, 0, 3);  // binary16 overflow to infinity
    named(kRgbOutPlanar, 34, 18, 1, 0x200, kTensorBF16, 0, 1, 1, 4);
    named(kRgbOutPlanar, 34, 18, 0, 0x300, kTensorF32, 0, 1, 1, 4);
    named(kRgbOutPlanar, 516, 16, 2, 0x000, kTensorU8, 0, 2, 0, 0); // a row of more than one pass
    named(kRgbOutPlanar, 20, 17, 0, 0x100, kTensorF32, 0, 0, 0, 0);
    named(kRgbOutInterleaved, 22, 18, 2, 0x000, kTensorU8, 1, 1, 1, 0);
    named(kRgbOutInterleaved, 18, 18, 4, 0x300, kTensorU8, 0, 1, 3, 0);
    named(kRgbOutInterleaved, 18, 18, 3, 0x100, kTensorF16, 1, 0, 2, 1);
    named(kRgbOutInterleaved, 17, 16, 0, 0x200, kTensorBF16, 0, 0, 0, 1);
    named(kRgbOutInterleaved, 68, 38, 1, 0x000, kTensorF32, 1, 2, 0, 1);
    named(kRgbOutInterleaved, 260, 16, 2, 0x300, kTensorF16, 0, 2, 0, 2); // binary16 subnormals and zeros
    named(kRgbOutInterleaved, 36, 20, 2, 0x100, kTensorF16, 1, 2, 0, 3);  // binary16 overflow to infinity
    named(kRgbOutInterleaved, 34, 18, 1, 0x200, kTensorBF16, 1, 1, 1, 4);
    named(kRgbOutInterleaved, 34, 18, 0, 0x300, kTensorF32, 0, 1, 1, 4);
    named(kRgbOutInterleaved, 516, 16, 2, 0x000, kTensorU8, 0, 2, 0, 0); // a row of more than one pass
    named(kRgbOutInterleaved, 20, 17, 0, 0x100, kTensorF32, 1, 0, 0, 0);
    printf("egress_rgb_check: packed %ld cases (%ld in the wide form) equal the pixel-by-pixel conversion, every alpha byte is 255; planar %ld cases (%ld in the "
           "wide form) equal the element-by-element contract; interleaved %ld cases (%ld in the wide form) equal the element-by-element contract and the planar "
           "tensor transposed (%ld); no byte outside the rows changed, the source planes are as they were\n",
           g_cases[kRgbOutPacked], g_wide[kRgbOutPacked], g_cases[kRgbOutPlanar], g_wide[kRgbOutPlanar], g_cases[kRgbOutInterleaved], g_wide[kRgbOutInterleaved],
           g_transposed);
    return 0;
}
