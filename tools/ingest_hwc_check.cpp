// ingest_hwc_check.cpp -- the body of k_ingest_hwc (csrc/ingest_hwc.h) run as plain C++ on the CPU, thread by thread, over a sweep of
// forms, element types (binary16, bfloat16, binary32), element orders (R G B, B G R), presets, chroma formats, widths 1 .. 9, 12, 16,
// 17, 255, 256, 257, 260, heights 1 .. 5, 16, 17, three pitches (tight, + 1 element, rounded to 256), pointer offsets 0 .. 3 elements
// and six sets of constants, each with three DIFFERENT constants per element position; meant to be built with AddressSanitizer and
// UndefinedBehaviorSanitizer, which see every write outside a destination plane's allocation, every misaligned vector access and every
// read outside a source ROW: the tensor is an exact-size heap block (the last row has nothing behind it) whose padding between the
// rows is poisoned while the body runs.  Every case is compared
//   - with the contract of include/dsv2_hip.h restated here (the affine step as two rounded operations, widening, clamp and rounding
//     in integers on the elements' bit patterns; constants by MEMORY POSITION, channels by the order; nothing shared with the kernel's
//     text) followed by the conversion restated sample by sample (check_support.h), guard bytes around every destination row;
//   - with ingest_tensor.h's planar body on the same picture de-interleaved, the constants permuted by the order: the same destination
//     planes, byte for byte.
// The job records the bodies run on are the library's own: csrc/enc_ingest.h accepts each tensor and plans it.
// tests/test_ingest_hwc_cpu.py builds and runs it:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I digital-subband-video-2_amd/csrc tools/ingest_hwc_check.cpp -o ingest_hwc_check && ./ingest_hwc_check [--dump DIR]
// Two deliberate breaks of the body, each of which must fail this program (DESIGN 5.26 records that they do; no build sets them):
//   -DINGEST_HWC_CHECK_BREAK_LOAD   the general form loads one element further on: a read past the last row's end, and wrong bytes
//   -DINGEST_HWC_CHECK_BREAK_SCALE  scale / bias indexed by channel instead of by memory position under B G R
// --dump DIR writes, for a few named cases, NAME.hwc (h rows of 3 * w elements, packed), NAME.const (scale[3], bias[3] as binary32, by
// position) and NAME.yuv (the converted planes, packed); NAME = dtype_order_csc_format_WxH.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#endif
#endif
#ifndef POISON
#define POISON(p, n) ((void) (p), (void) (n))
#define UNPOISON(p, n) ((void) (p), (void) (n))
#endif

#include "ingest_plan.h"
#include "ingest_hwc.h"

#include "check_support.h"

using namespace dsv2;

namespace {

using support::expect_chroma;
using support::expect_luma;
using support::kFmtName;
using support::kHs;
using support::kVs;
using support::Picture;

// ---- the contract, restated (tools/ingest_tensor_check.cpp's restatement, written out again: the programs share no text) ------------
uint32_t bits_of(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}
float float_of(uint32_t b)
{
    float f;
    memcpy(&f, &b, 4);
    return f;
}
uint32_t widen_half(uint32_t h) // binary16 bits to the binary32 bits of the same value, in integers
{
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu;
    uint32_t m = h & 0x3ffu;
    if (e == 0x1f) {
        return sign | 0x7f800000u | (m << 13);
    }
    if (e == 0) {
        if (m == 0) {
            return sign;
        }
        int ex = 127 - 15 + 1; // the value is m * 2^-24: normalise
        while (!(m & 0x400u)) {
            m <<= 1, ex--;
        }
        return sign | ((uint32_t) ex << 23) | ((m & 0x3ffu) << 13);
    }
    return sign | ((e + 127 - 15) << 23) | (m << 13);
}
uint32_t widen(int dtype, uint32_t e) { return dtype == kTensorF32 ? e : dtype == kTensorBF16 ? e << 16 : widen_half(e); }
uint8_t byte_of(uint32_t b) // binary32 bits of g to the byte: 0 for a NaN, else rint(min(max(g, 0), 255)), ties to even
{
    const uint32_t ex = (b >> 23) & 0xffu, man = b & 0x7fffffu;
    if ((b >> 31) || (ex == 0xff && man) || ex < 126) { // negative, -0, -inf; NaN; below a half
        return 0;
    }
    if (ex >= 135) { // 256 and above, +inf
        return 255;
    }
    const uint32_t m = man | 0x800000u, shift = 150 - ex; // the value is m * 2^-shift, shift 16 .. 24
    uint32_t q = m >> shift;
    const uint32_t rest = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rest > half || (rest == half && (q & 1))) {
        q++;
    }
    return (uint8_t) (q > 255 ? 255 : q);
}
uint8_t expect_byte(int dtype, uint32_t e, float scale, float bias)
{
    volatile float p = float_of(widen(dtype, e)) * scale; // (two operations, each rounded on its own)
    volatile float g = p + bias;
    return byte_of(bits_of(g));
}

// ---- constants: scale[3], bias[3] BY ELEMENT POSITION, three different ones in every set, so that a swapped index shows --------------
// near identity; near the inverse of 1 / 255; the inverse of ImageNet's Normalize folded (255 * std, 255 * mean); integers to ties and
// near them; subnormals to 1 and 2 (2^127; binary16's own: 2^23); mixed, with a negative scale
constexpr int kConsts = 6;
const float kConst[kConsts][6] = {{1.0f, 0.5f, 2.0f, 0.0f, 1.0f, -1.0f},
                                  {255.0f, 254.0f, 256.0f, 0.0f, 0.25f, -0.25f},
                                  {(float) (255.0 * 0.229), (float) (255.0 * 0.224), (float) (255.0 * 0.225), (float) (255.0 * 0.485), (float) (255.0 * 0.456), (float) (255.0 * 0.406)},
                                  {1.0f, 1.0f, 1.0f, 0.5f, 1.5f, -0.5f},
                                  {0x1p127f, 0x1p126f, 0x1p23f, 0.0f, 0.5f, 1.0f},
                                  {-255.0f, (float) (255.0 * 0.224), 0x1p23f, 255.0f, (float) (255.0 * 0.456), 0.25f}};
const char *const kTypeName[4] = {"u8", "f16", "bf16", "f32"};
const int kOrder[2] = {DSV2HIP_SURFACE_RGB, DSV2HIP_SURFACE_BGR};
const char *const kOrderName[2] = {"rgb", "bgr"};

unsigned lcg(unsigned &s) { return s = s * 1664525u + 1013904223u; }

uint32_t narrow(int dtype, float f) // binary32 bits to the element type's (the generator only needs SOME element near the value)
{
    if (dtype == kTensorF32) {
        return bits_of(f);
    }
    if (dtype == kTensorBF16) {
        return bits_of(f) >> 16;
    }
    const _Float16 h = (_Float16) f;
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}
// an element for constants (scale, bias): mostly values whose g lies in -20 .. 280 on a grid of quarters (so ties occur), an eighth of
// them special patterns
uint32_t element(int dtype, float scale, float bias, unsigned &seed)
{
    static const uint32_t special32[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00001u, 0x7f800001u, 0x00400000u, 0x00600000u, 0x80400000u,
                                         0x00000001u, 0x3f000000u, 0x3fc00000u, 0x40200000u, 0x437e8000u, 0x437f8000u, 0x7f7fffffu, 0xff7fffffu, 0x43800000u, 0xc3800000u};
    static const uint32_t special16[] = {0x0000u, 0x8000u, 0x7c00u, 0xfc00u, 0x7e00u, 0xfe01u, 0x7c01u, 0x0001u, 0x0002u, 0x0003u, 0x8001u, 0x03ffu, 0x3800u, 0x3e00u, 0x4100u,
                                         0x5bf4u, 0x5bfcu, 0x7bffu, 0xfbffu, 0x5c00u};
    const unsigned r = lcg(seed);
    if ((r >> 29) == 0) {
        const unsigned k = (r >> 8) % 20;
        return dtype == kTensorF32 ? special32[k] : dtype == kTensorF16 ? special16[k] : special32[k] >> 16;
    }
    const float target = (float) ((r >> 8) % 1201u) * 0.25f - 20.0f;
    return narrow(dtype, (target - bias) / scale);
}

// ---- planes -----------------------------------------------------------------------------------------------------------------------
struct Plane : support::GuardedPlane { // as dframe_alloc lays one out: 32-pixel border, stride a multiple of 16, 16-byte aligned origin
    Plane(int w_, int h_) : support::GuardedPlane(w_, h_, kBorder, 0) {}
};

// a source: `offset` bytes, then h rows of rb bytes `pitch` apart, and not one byte more; armed: the padding between the rows and the
// bytes in front are poisoned, so that a read outside a row faults also where it stays inside the block
struct Source {
    uint8_t *alloc, *org;
    size_t bytes, pitch, rb;
    int h;
    std::vector<uint8_t> was;
    Source(int h_, size_t rb_, size_t pitch_, size_t offset) : pitch(pitch_), rb(rb_), h(h_)
    {
        bytes = offset + (size_t) (h - 1) * pitch + rb;
        if (posix_memalign((void **) &alloc, 64, bytes) != 0) { // (exact size: one byte behind the last row is outside the block)
            abort();
        }
        org = alloc + offset;
        memset(alloc, 0x7f, bytes); // (padding: NaN-ish patterns in every element type)
    }
    void arm(bool on)
    {
        if (on) {
            was.assign(alloc, alloc + bytes);
        }
        for (int y = 0; y + 1 < h && pitch > rb; y++) {
            on ? POISON(org + (size_t) y * pitch + rb, pitch - rb) : UNPOISON(org + (size_t) y * pitch + rb, pitch - rb);
        }
        if (org > alloc) {
            on ? POISON(alloc, (size_t) (org - alloc)) : UNPOISON(alloc, (size_t) (org - alloc));
        }
    }
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

const int kSubsamp[5] = {DSV_SUBSAMP_444, DSV_SUBSAMP_422, DSV_SUBSAMP_420, DSV_SUBSAMP_411, DSV_SUBSAMP_410};
long g_cases = 0, g_wide = 0, g_seen[4][2][2][5][4]; // [dtype][wide][order][format][preset]
const char *g_dump = nullptr;

// pitch_kind: tight; one element more; rounded up to 256 bytes
size_t pitch_of(size_t rb, int elem, int pitch_kind) { return pitch_kind == 0 ? rb : pitch_kind == 1 ? rb + (size_t) elem : (rb + 255) / 256 * 256; }

// offset: elements behind a 64-byte boundary
void check(int w, int h, int fmt, int csc, int dtype, int oi, int pitch_kind, int offset, int cset, bool force_general, const char *dump_name = nullptr)
{
    const int hs = kHs[fmt], vs = kVs[fmt], elem = tensor_elem(dtype), order = kOrder[oi];
    const int cw = (w + (1 << hs) - 1) >> hs, ch = (h + (1 << vs) - 1) >> vs;
    unsigned seed = 977u * (unsigned) w + 31u * (unsigned) h + (unsigned) (fmt + 5 * pitch_kind + 20 * offset + 80 * dtype + 400 * cset + 2400 * oi);
    const float *k = kConst[cset];
    const size_t rb = 3 * (size_t) w * (size_t) elem;
    Source src(h, rb, pitch_of(rb, elem, pitch_kind), (size_t) offset * (size_t) elem);
    // the planar counterpart: plane c holds channel c, which is element position (order == BGR ? 2 - c : c) of every pixel
    std::vector<uint8_t> planar[3];
    Picture pic{w, h, std::vector<int>(3 * (size_t) w * h)};
    dsv2hip_in_hwc tn{};
    dsv2hip_in_tensor pt{};
    tn.data = src.org, tn.pitch = src.pitch, tn.dtype = pt.dtype = dtype, tn.order = order, tn.csc = pt.csc = csc;
    for (int c = 0; c < 3; c++) {
        planar[c].resize((size_t) w * h * elem);
    }
    for (int y = 0; y < h; y++) {
        for (int x = 0; x < w; x++) {
            for (int pos = 0; pos < 3; pos++) {
                const int c = order == DSV2HIP_SURFACE_BGR ? 2 - pos : pos; // the channel at this position
                const uint32_t e = element(dtype, k[pos], k[3 + pos], seed);
                memcpy(src.org + (size_t) y * src.pitch + (3 * (size_t) x + pos) * (size_t) elem, &e, (size_t) elem); // (little endian: the low bytes)
                memcpy(planar[c].data() + ((size_t) y * w + x) * (size_t) elem, &e, (size_t) elem);
                pic.rgb[3 * ((size_t) y * w + x) + (size_t) c] = expect_byte(dtype, e, k[pos], k[3 + pos]);
            }
        }
    }
    for (int pos = 0; pos < 3; pos++) {
        const int c = order == DSV2HIP_SURFACE_BGR ? 2 - pos : pos;
        tn.scale[pos] = k[pos], tn.bias[pos] = k[3 + pos];
        pt.plane[c] = planar[c].data(), pt.pitch[c] = (size_t) w * elem, pt.scale[c] = k[pos], pt.bias[c] = k[3 + pos];
    }
    Plane Y(w, h), U(cw, ch), V(cw, ch), PY(w, h), PU(cw, ch), PV(cw, ch);
    enc_ingest::Source accepted, accepted_planar;
    if (!enc_ingest::accept_hwc(w, h, kSubsamp[fmt], false, tn, &accepted) || !enc_ingest::accept_tensor(w, h, kSubsamp[fmt], false, pt, &accepted_planar)) {
        fprintf(stderr, "REFUSED: a %s tensor of %dx%d, pitch kind %d, offset %d\n", kTypeName[dtype], w, h, pitch_kind, offset);
        exit(1);
    }
    const enc_ingest::IngestPlan plan = planned_from(kSubsamp[fmt], Y, U, V, accepted);
    expect_records(plan, enc_ingest::HWC_IN, 1);
    const HwcInJob &j = plan.hwc[0];
    const bool wide = plan.wide[enc_ingest::HWC_IN] && !force_general;
    src.arm(true);
    wide ? run_grid(h, [&](int y0, int x, int step) { ingest_hwc_rows<true>(j, y0, x, step); })
         : run_grid(h, [&](int y0, int x, int step) { ingest_hwc_rows<false>(j, y0, x, step); });
    src.arm(false);
    g_cases++, g_wide += wide;
    g_seen[dtype][wide][oi][fmt][csc >> 8]++;
    char what[240];
    snprintf(what, sizeof what, "%dx%d %s csc=0x%x %s %s pitch=%zu offset=%d constants=%d wide=%d", w, h, kFmtName[fmt], csc, kTypeName[dtype], kOrderName[oi], src.pitch,
             offset, cset, (int) wide);
    if (!src.untouched()) {
        fprintf(stderr, "the tensor was written: %s\n", what);
        exit(1);
    }
    const Plane *pl[3] = {&Y, &U, &V};
    for (int c = 0; c < 3; c++) {
        long bx, by;
        int got, exp;
        if (!pl[c]->equals([&](int x, int y) { return c == 0 ? expect_luma(pic, csc, x, y) : expect_chroma(pic, csc, c, hs, vs, x, y); }, &bx, &by, &got, &exp)) {
            fprintf(stderr, "MISMATCH %s: plane %d row %ld column %ld is %02x, expected %02x\n", what, c, by, bx, got, exp);
            exit(1);
        }
    }
    // the planar body on the picture de-interleaved, the constants permuted: the same allocation contents, guard bytes and all
    const enc_ingest::IngestPlan pplan = planned_from(kSubsamp[fmt], PY, PU, PV, accepted_planar);
    expect_records(pplan, enc_ingest::TENSOR_IN, 1);
    const TensorInJob &pj = pplan.tensor[0];
    pplan.wide[enc_ingest::TENSOR_IN] ? run_grid(h, [&](int y0, int x, int step) { ingest_tensor_rows<true>(pj, y0, x, step); })
                                      : run_grid(h, [&](int y0, int x, int step) { ingest_tensor_rows<false>(pj, y0, x, step); });
    const Plane *ppl[3] = {&PY, &PU, &PV};
    for (int c = 0; c < 3; c++) {
        if (pl[c]->bytes != ppl[c]->bytes || memcmp(pl[c]->alloc, ppl[c]->alloc, pl[c]->bytes) != 0) {
            fprintf(stderr, "PLANAR %s: plane %d differs from k_ingest_tensor's body on the de-interleaved picture\n", what, c);
            exit(1);
        }
    }
    if (dump_name && g_dump) {
        FILE *ft = support::dump_open(g_dump, dump_name, ".hwc"), *fc = support::dump_open(g_dump, dump_name, ".const"), *fy = support::dump_open(g_dump, dump_name, ".yuv");
        support::dump_rows(ft, src.org, src.pitch, src.rb, h);
        fwrite(k, 4, 6, fc);
        for (int c = 0; c < 3; c++) {
            support::dump_rows(fy, pl[c]->org, (size_t) pl[c]->stride, (size_t) pl[c]->w, pl[c]->h);
        }
        fclose(ft), fclose(fc), fclose(fy);
    }
}

// what the contract says in so many words, through the fetch: a row of four pixels whose twelve elements are named values, three
// constant pairs by position
void named_values()
{
    HwcInJob j{};
    const float scale[3] = {1.0f, 0x1p127f, 1.0f + 0x1p-12f}, bias[3] = {0.0f, 0.0f, -256.0f};
    for (int k = 0; k < 3; k++) {
        j.scale[k] = scale[k], j.bias[k] = bias[k];
    }
    // position 0: ties; position 1: 2^-127, 1.5 * 2^-127, a NaN, +inf; position 2: the element whose product exceeds a tie by less than
    // half an ulp (0 unfused, 1 fused), -inf, 257 / (1 + 2^-12) or so, -0
    const uint32_t e[12] = {bits_of(0.5f),   0x00400000u, 0x438037fdu, bits_of(1.5f),   0x00600000u, 0xff800000u,
                            bits_of(2.5f),   0x7fc00000u, bits_of(258.0f), bits_of(254.5f), 0x7f800000u, 0x80000000u};
    const int want[12] = {0, 1, 0, 2, 2, 0, 2, 0, 2, 254, 255, 0};
    HwcInRaw<kTensorF32> raw;
    memcpy(raw.d, e, sizeof e);
    uint32_t px[4];
    hwc_in_pixels<kTensorF32>(j, raw, px);
    for (int i = 0; i < 12; i++) {
        const int got = (int) ((px[i / 3] >> (8 * (i % 3))) & 0xffu), restated = expect_byte(kTensorF32, e[i], scale[i % 3], bias[i % 3]);
        if (got != want[i] || restated != want[i] || (px[i / 3] >> 24)) {
            fprintf(stderr, "NAMED: element %d (%#x): the fetch gives %d, the restatement %d, the contract %d\n", i, e[i], got, restated, want[i]);
            exit(1);
        }
    }
}

} // namespace

int main(int argc, char **argv)
{
    if (!support::dump_option(argc, argv, &g_dump)) {
        return 2;
    }
    named_values();
    static const int cscs[4] = {0x000, 0x100, 0x200, 0x300};
    static const int widths[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 255, 256, 257, 260, 12};
    static const int hts[7] = {1, 2, 3, 4, 5, 16, 17};
    static const int dtypes[3] = {kTensorF16, kTensorBF16, kTensorF32};
    // every width with every element type, order, format, pitch kind and offset, in both forms where the wide one applies; heights,
    // presets and constants take turns (with periods 7, 4 and 6 against an inner loop of 12: every combination comes round)
    long turn = 0;
    for (int w : widths) {
        for (int dtype : dtypes) {
            for (int oi = 0; oi < 2; oi++) {
                for (int fmt = 0; fmt < 5; fmt++) {
                    for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++) {
                        for (int offset = 0; offset < 4; offset++, turn++) {
                            check(w, hts[turn % 7], fmt, cscs[(turn / 7) & 3], dtype, oi, pitch_kind, offset, (int) (turn % kConsts), false);
                        }
                    }
                    check(w, hts[turn % 7], fmt, cscs[turn & 3], dtype, oi, 2, 0, (int) (turn % kConsts), true); // general on an aligned tensor
                    check(w, hts[(turn + 1) % 7], fmt, cscs[(turn + 1) & 3], dtype, oi, 0, 0, (int) ((turn + 1) % kConsts), false); // tight: wide where w % 4 == 0
                    turn++;
                }
            }
        }
    }
    // every height with every format, preset, element type and order at the smallest pictures and at footprints half outside them
    for (int w : {16, 18, 22}) {
        for (int h : hts) {
            for (int fmt = 0; fmt < 5; fmt++) {
                for (int csc : cscs) {
                    for (int dtype : dtypes) {
                        for (int oi = 0; oi < 2; oi++) {
                            turn++;
                            check(w, h, fmt, csc, dtype, oi, 2, 0, (int) (turn % kConsts), false);                                          // wide where w allows
                            check(w, h, fmt, csc, dtype, oi, (int) (turn % 3), 1 + (int) (turn % 3), (int) ((turn / 3) % kConsts), false); // general
                        }
                    }
                }
            }
        }
    }
    for (int dtype = 1; dtype < 4; dtype++) {
        for (int wide = 0; wide < 2; wide++) {
            for (int oi = 0; oi < 2; oi++) {
                for (int fmt = 0; fmt < 5; fmt++) {
                    for (int p = 0; p < 4; p++) {
                        if (!g_seen[dtype][wide][oi][fmt][p]) {
                            fprintf(stderr, "FAILED: the sweep holds no %s %s case in the %s form, format %s, preset %d\n", kTypeName[dtype], kOrderName[oi],
                                    wide ? "wide" : "general", kFmtName[fmt], p);
                            return 1;
                        }
                    }
                }
            }
        }
    }
    check(1920, 18, 2, 0x100, kTensorF32, 0, 2, 0, 2, false); // (rows of several passes in the wide form)
    check(1920, 16, 4, 0x200, kTensorF16, 1, 0, 0, 1, false);
    check(22, 18, 2, 0x000, kTensorF16, 0, 1, 1, 1, false, "f16_rgb_000_420_22x18");
    check(18, 18, 4, 0x300, kTensorBF16, 1, 1, 3, 2, false, "bf16_bgr_300_410_18x18");
    check(18, 18, 3, 0x100, kTensorF32, 1, 2, 2, 2, false, "f32_bgr_100_411_18x18");
    check(17, 16, 0, 0x200, kTensorF32, 0, 0, 0, 5, false, "f32_rgb_200_444_17x16");
    check(68, 38, 1, 0x000, kTensorBF16, 0, 2, 0, 0, false, "bf16_rgb_000_422_68x38");
    check(68, 38, 1, 0x300, kTensorF16, 1, 2, 0, 4, false, "f16_bgr_300_422_68x38");
    check(40, 21, 0, 0x100, kTensorF32, 1, 0, 0, 3, false, "f32_bgr_100_444_40x21");
    check(260, 17, 2, 0x300, kTensorF16, 0, 2, 0, 5, false, "f16_rgb_300_420_260x17");
    check(256, 16, 2, 0x200, kTensorBF16, 1, 0, 0, 3, false, "bf16_bgr_200_420_256x16");
    check(1920, 16, 2, 0x300, kTensorF32, 0, 2, 0, 1, false, "f32_rgb_300_420_1920x16");
    printf("ingest_hwc_check: %ld cases (%ld in the wide form) equal the contract and the conversion restated and the planar body on the picture de-interleaved; "
           "no byte outside the planes changed, no byte outside a tensor's rows was read, the tensors are as they were\n",
           g_cases, g_wide);
    return 0;
}
