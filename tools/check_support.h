// check_support.h -- what the stand-alone check programs tools/*_check.cpp share: the guard constants, the source plane in an
// exact-size heap block, the guarded destination plane, the chroma format tables, the --dump option and the two conversions of include/dsv2_hip.h restated.
//
// This header includes nothing from csrc/: no egress_*.h, no ingest_*.h.  The programs exist to compare a kernel's thread body with a
// restatement that shares no text with it, so whatever is restated here -- the conversion's constants and rounding above all -- is
// written from the public header alone and must stay that way.  (The border width of a decoder plane is csrc's kBorder: a program
// passes it in.)
#ifndef DSV2_TOOLS_CHECK_SUPPORT_H
#define DSV2_TOOLS_CHECK_SUPPORT_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

namespace support {

constexpr uint8_t kGuard = 0xA5; // what a destination holds before the kernel body runs
constexpr int kLead = 64;        // guard bytes in front of and behind a destination

// DSV_SUBSAMP_444, _422, _420, _411 and the reference's "4:1:0": chroma shifts and names, by the programs' format index
const int kHs[5] = {0, 1, 1, 2, 2}, kVs[5] = {0, 0, 1, 0, 2};
const char *const kFmtName[5] = {"444", "422", "420", "411", "410"};

// ---- noise: one byte from a state of the programs' linear congruential generator; each program keeps its own recipe ----------------
inline uint8_t noise_plain(unsigned s) { return (uint8_t) (s >> 24); }
// an eighth of the samples 0 or 255, a sixteenth 16 or 235 (the ends of both ranges of the conversion)
inline uint8_t noise_range_ends(unsigned s)
{
    return (s >> 29) == 0 ? ((s & 0x10000) ? 255 : 0) : (s >> 28) == 2 ? ((s & 0x10000) ? 235 : 16) : (uint8_t) (s >> 20);
}
// a quarter of the samples 0 or 255
inline uint8_t noise_extremes(unsigned s) { return (s >> 30) == 0 ? ((s & 0x10000) ? 255 : 0) : (uint8_t) (s >> 20); }

// ---- a source plane: an exact-size heap block, so that the sanitizer sees every read outside it ------------------------------------
struct Plane {
    uint8_t *alloc, *org;
    size_t bytes;
    int stride, w, h;
    std::vector<uint8_t> was;
    // border > 0: as dframe_alloc lays a plane out (a border all round, stride a multiple of 16, 16-byte aligned origin); 0: as the
    // decoder stages a luma plane: stride = w rounded up to 16, h rows.  Border and padding hold noise too.  constant >= 0: the
    // visible samples hold that value.
    Plane(int w_, int h_, int border, unsigned seed, uint8_t (*noise)(unsigned), int constant = -1) : w(w_), h(h_)
    {
        stride = (w + 2 * border + 15) & ~15;
        bytes = (size_t) stride * (size_t) (h + 2 * border);
        alloc = (uint8_t *) aligned_alloc(16, bytes);
        for (size_t i = 0; i < bytes; i++) {
            seed = seed * 1664525u + 1013904223u;
            alloc[i] = noise(seed);
        }
        org = alloc + (size_t) border * stride + border;
        if (constant >= 0) {
            for (int y = 0; y < h; y++) {
                memset(org + (size_t) y * stride, constant, (size_t) w);
            }
        }
        was.assign(alloc, alloc + bytes);
    }
    ~Plane() { free(alloc); }
    Plane(const Plane &) = delete;
    int at(int x, int y) const { return org[(size_t) y * stride + x]; }
    bool unchanged() const { return memcmp(was.data(), alloc, bytes) == 0; }
    void fill(int (*f)(int, int)) // the visible samples, for a case with chosen content
    {
        for (int y = 0; y < h; y++) {
            for (int x = 0; x < w; x++) {
                org[(size_t) y * stride + x] = (uint8_t) f(x, y);
            }
        }
        was.assign(alloc, alloc + bytes);
    }
};

// ---- a destination plane as dframe_alloc lays one out (a border all round, stride a multiple of 16, 16-byte aligned origin) with `lead`
// guard bytes in front of and behind it, every byte holding the guard value ------------------------------------------------------------
struct GuardedPlane {
    uint8_t *alloc, *first, *org;
    size_t bytes;
    int stride, w, h, border, lead;
    GuardedPlane(int w_, int h_, int border_, int lead_) : w(w_), h(h_), border(border_), lead(lead_)
    {
        stride = (w + 2 * border + 15) & ~15;
        bytes = (size_t) stride * (size_t) (h + 2 * border) + 2 * (size_t) lead;
        alloc = (uint8_t *) aligned_alloc(16, (bytes + 15) & ~(size_t) 15);
        memset(alloc, kGuard, bytes);
        first = alloc + lead;
        org = first + (size_t) border * stride + border;
    }
    ~GuardedPlane() { free(alloc); }
    GuardedPlane(const GuardedPlane &) = delete;
    // every byte is the guard value except the w x h samples, which are want(x, y): nothing outside the rows changed
    template <class F> bool equals(F want, long *bad_x, long *bad_y, int *got, int *expected) const
    {
        for (size_t i = 0; i < bytes; i++) {
            const long at = (long) i - lead;
            long y = at >= 0 ? at / stride - border : -1000, x = at >= 0 ? at % stride - border : -1000;
            const bool inside = at >= 0 && x >= 0 && x < w && y >= 0 && y < h;
            const int e = inside ? want((int) x, (int) y) : kGuard;
            if (alloc[i] != e) {
                *bad_x = x, *bad_y = y, *got = alloc[i], *expected = e;
                return false;
            }
        }
        return true;
    }
};

inline int ceil_shift(int v, int s) { return (v + (1 << s) - 1) >> s; }

// ---- dumps: `rows` rows of rb bytes `pitch` apart, packed; a file NAME + ext in the --dump directory ----------------------------------
inline void dump_rows(FILE *f, const uint8_t *p, size_t pitch, size_t rb, int rows)
{
    for (int y = 0; y < rows; y++) {
        fwrite(p + (size_t) y * pitch, 1, rb, f);
    }
}
inline FILE *dump_open(const char *dir, const char *name, const char *ext)
{
    FILE *f = fopen((std::string(dir) + "/" + name + ext).c_str(), "wb");
    if (!f) {
        fprintf(stderr, "cannot write into %s\n", dir);
        exit(1);
    }
    return f;
}

// ---- [--dump DIR]: the directory, or nullptr; false for any other command line (usage is printed) -----------------------------------
inline bool dump_option(int argc, char **argv, const char **dir)
{
    *dir = nullptr;
    if (argc == 3 && strcmp(argv[1], "--dump") == 0) {
        *dir = argv[2];
    } else if (argc != 1) {
        fprintf(stderr, "usage: %s [--dump DIR]\n", argv[0]);
        return false;
    }
    return true;
}

// ---- THE CONVERSION of include/dsv2_hip.h, YUV -> RGB, restated: one pixel at a time, in the header's own terms ---------------------
const long kPreset[4][6] = {{298, 16, 409, -100, -208, 516}, {298, 16, 459, -55, -136, 541}, {256, 0, 359, -88, -183, 454}, {256, 0, 403, -48, -120, 475}};
inline int preset_of(int csc) { return ((csc & 0x200) ? 2 : 0) + ((csc & 0x100) ? 1 : 0); }
inline long floor_shift8(long v) { return v >= 0 ? v / 256 : -((-v + 255) / 256); }
inline uint8_t clamp255(long v) { return (uint8_t) (v < 0 ? 0 : v > 255 ? 255 : v); }

inline void expect_pixel(int csc, int Y, int U, int V, uint8_t out[3]) // R, G, B
{
    const long *p = kPreset[preset_of(csc)];
    const long C = p[0] * (Y - p[1]), D = U - 128, E = V - 128;
    out[0] = clamp255(floor_shift8(C + p[2] * E + 128));
    out[1] = clamp255(floor_shift8(C + p[3] * D + p[4] * E + 128));
    out[2] = clamp255(floor_shift8(C + p[5] * D + 128));
}

// ---- THE CONVERSION of include/dsv2_hip.h, RGB -> YUV, restated: one sample at a time, signed arithmetic, coordinates clamped ---------
const int kMatrix[4][9] = {{66, 129, 25, -38, -74, 112, 112, -94, -18},
                           {47, 157, 16, -26, -86, 112, 112, -102, -10},
                           {77, 150, 29, -43, -85, 128, 128, -107, -21},
                           {54, 183, 19, -29, -99, 128, 128, -116, -12}};

struct Picture { // a surface's pixels as R, G, B triples, whatever its byte order, layout and pitch
    int w, h;
    std::vector<int> rgb;
    const int *at(int x, int y) const
    {
        x = x < w - 1 ? x : w - 1;
        y = y < h - 1 ? y : h - 1;
        return &rgb[3 * ((size_t) y * w + x)];
    }
};

inline int expect_luma(const Picture &p, int csc, int x, int y)
{
    const int *m = kMatrix[preset_of(csc)], *c = p.at(x, y);
    const int ybase = (csc & 0x200) ? 0 : 16;
    return (m[0] * c[0] + m[1] * c[1] + m[2] * c[2] + 128 + 256 * ybase) >> 8;
}

inline int expect_chroma(const Picture &p, int csc, int row, int hs, int vs, int cx, int cy)
{
    const int *m = kMatrix[preset_of(csc)] + 3 * row;
    long sum = 0;
    for (int dy = 0; dy < 1 << vs; dy++) {
        for (int dx = 0; dx < 1 << hs; dx++) {
            const int *c = p.at((cx << hs) + dx, (cy << vs) + dy);
            sum += m[0] * c[0] + m[1] * c[1] + m[2] * c[2];
        }
    }
    const long v = (sum + (32896L << (hs + vs))) >> (8 + hs + vs);
    return (int) (v < 255 ? v : 255);
}

} // namespace support

#endif
