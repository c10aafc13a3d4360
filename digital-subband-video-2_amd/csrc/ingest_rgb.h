// ingest_rgb.h -- what one thread of k_ingest_rgb (ingest.hip) does, as a function that also compiles for the host (the pattern of
// egress_uv.h): the kernel is this function behind blockIdx / threadIdx, and tools/ingest_rgb_check.cpp sweeps the very same code
// on the CPU under AddressSanitizer -- forms, byte orders, presets, formats, widths, pitches and offsets -- before it runs on a GPU.
//
// One RgbJob (io_jobs.h) = one packed four-byte RGB surface (dsv2hip_surface, layout BGRA / RGBA) on its way into the three bordered
// source planes, converted on the way by the integer formulas of include/dsv2_hip.h (the contract; restated at rgb_chroma below).
// A thread owns FOUR pixels of FOUR consecutive rows -- a whole number of chroma footprints of every format (the widest is 4 pixels,
// the tallest 4 rows), so neither LDS nor another lane is needed; rows below h and pixels right of w are read again from the last
// row / pixel (the clamp of the contract) and never stored; every load is issued before the first store.
//   VEC = 16, the wide form: source pointer and pitch multiples of 16 and w a multiple of 4 in every job of the launch (the host
//             picks it per step, rgb_job_wide): one 16-byte load per row; luma leaves as one dword per row, chroma as a dword
//             (4:4:4), two bytes (4:2:2, 4:2:0) or one byte (4:1:1, "4:1:0") per chroma row -- what four pixels hold of it.
//   VEC = 4, the general form: any w, pitch and alignment.  A pixel is read as one dword where the surface's pointer and pitch are
//             multiples of 4 (the dword always lies whole inside the row), else as its three colour bytes; no word that holds no
//             byte of the row is touched.
//             Destination bytes are written dword- or pair-wise where the piece is whole, else byte by byte inside w x h (luma) and
//             cw x ch (chroma): the border is k_extend's.
// The coefficients arrive as byte quads in the surface's channel order with 0 for alpha, so BGRA and RGBA differ only in the
// job's data, and a weighted sum over a pixel is ONE v_dot4_u32_u8 against the pixel dword; chroma rows, whose coefficients have
// both signs, are two quads (positive parts, magnitudes of the negative parts) and two dot products, accumulated over the footprint
// and subtracted once.  Every sum is non-negative before its shift (checked over all colours by tests/test_ingest_rgb_cpu.py).
#pragma once

#include "egress_uv.h" // perm_b32

namespace dsv2 {

// Every address below is a base all lanes share (a row of a plane: scalar registers) plus a 32-bit lane offset, and says that it
// is device memory: global_load / global_store instead of the flat_ forms a pointer of unknown kind gets (which also count against
// the LDS counter); the 64-bit sum lives for the one access only.
#if defined(__HIP_DEVICE_COMPILE__)
#define DSV2_GLOBAL __attribute__((address_space(1)))
#else
#define DSV2_GLOBAL
#endif
template <class T> __host__ __device__ __forceinline__ T ld_global(const uint8_t *base, uint32_t off) { return *(const DSV2_GLOBAL T *) (base + off); }
template <class T> __host__ __device__ __forceinline__ void st_global(uint8_t *base, uint32_t off, T v) { *(DSV2_GLOBAL T *) (base + off) = v; }
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// The row loop's pixel index, handed on as a value the compiler knows nothing about: it otherwise turns every address of the loop
// body into a 64-bit per-lane induction variable of its own (twelve of them, 24 VGPRs, in the first build of this file).
__host__ __device__ __forceinline__ int lane_offset(int x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}

// c + sum over the four bytes of a * b
__host__ __device__ __forceinline__ uint32_t dot4_u8(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int i = 0; i < 4; i++) {
        c += ((a >> (8 * i)) & 0xffu) * ((b >> (8 * i)) & 0xffu);
    }
    return c;
#endif
}

// pixel at byte offset `off` (a multiple of 4) of a row (general form): its dword where the row is 4-byte aligned (the dword always
// lies whole inside the row), else its colour bytes (alpha, byte 3 in both orders, weighs 0)
__host__ __device__ __forceinline__ uint32_t rgb_pixel(const uint8_t *row, uint32_t off, bool aligned)
{
    if (aligned) {
        return ld_global<uint32_t>(row, off);
    }
    return (uint32_t) ld_global<uint8_t>(row, off) | ((uint32_t) ld_global<uint8_t>(row, off + 1) << 8) | ((uint32_t) ld_global<uint8_t>(row, off + 2) << 16);
}

// One chroma plane's samples of the thread's 4 x 4 pixels px[row][pixel] (top-left pixel (x, y0)):
//   C(cx, cy) = min(255, (SUM over the footprint of (cr * R + cg * G + cb * B) + N * 32896) >> (8 + HS + VS)),  N = 1 << (HS + VS)
// pos / neg: the row's positive coefficients / the magnitudes of its negative ones.  WIDE: w is a multiple of 4.
template <int HS, int VS, bool WIDE>
__host__ __device__ __forceinline__ void rgb_chroma(const RgbJob &j, const uint32_t (&px)[4][4], int x, int y0, uint8_t *plane, uint32_t pos,
                                                    uint32_t neg)
{
    constexpr int NX = 4 >> HS, NY = 4 >> VS; // samples per row, rows of samples
    const int cw = (j.w + (1 << HS) - 1) >> HS, cx0 = x >> HS;
#pragma unroll
    for (int cy = 0; cy < NY; cy++) {
        if (y0 + (cy << VS) >= j.h) { // (= the chroma row lies below ch)
            break;
        }
        uint32_t o = 0;
#pragma unroll
        for (int cx = 0; cx < NX; cx++) {
            uint32_t p = 32896u << (HS + VS), n = 0;
#pragma unroll
            for (int r = 0; r < 1 << VS; r++) {
#pragma unroll
                for (int i = 0; i < 1 << HS; i++) {
                    const uint32_t q = px[(cy << VS) + r][(cx << HS) + i];
                    p = dot4_u8(q, pos, p);
                    n = dot4_u8(q, neg, n);
                }
            }
            const uint32_t v = (p - n) >> (8 + HS + VS);
            o |= (v < 255u ? v : 255u) << (8 * cx);
        }
        uint8_t *crow = plane + (size_t) ((y0 >> VS) + cy) * (size_t) j.cstride;
        if constexpr (NX == 4) {
            if (WIDE || cx0 + 4 <= cw) {
                st_global<uint32_t>(crow, cx0, o); // (x is a multiple of 4, the plane's origin and stride of 16)
            } else {
                for (int i = 0; cx0 + i < cw; i++) {
                    st_global<uint8_t>(crow, cx0 + i, (uint8_t) (o >> (8 * i)));
                }
            }
        } else if constexpr (NX == 2) {
            if (WIDE || cx0 + 2 <= cw) {
                st_global<uint16_t>(crow, cx0, (uint16_t) o);
            } else {
                st_global<uint8_t>(crow, cx0, (uint8_t) o);
            }
        } else {
            st_global<uint8_t>(crow, cx0, (uint8_t) o);
        }
    }
}

// luma, U and V of the thread's 4 x 4 pixels px[row][pixel] (top-left pixel (x, y0), x and y0 multiples of 4), stored: all that follows
// the fetch, shared with ingest_rgb3.h.  WIDE: w is a multiple of 4.
template <int HS, int VS, bool WIDE> __host__ __device__ __forceinline__ void rgb_emit(const RgbJob &j, const uint32_t (&px)[4][4], int x, int y0)
{
    const int w = j.w, h = j.h;
    // Y(x, y) = (yr * R + yg * G + yb * B + 128 + 256 * ybase) >> 8: byte 1 of the sum, which is below 65 536
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (y0 + r >= h) {
            break;
        }
        const uint32_t y01 = perm_b32(dot4_u8(px[r][1], j.csc.ycoef, j.csc.yoff), dot4_u8(px[r][0], j.csc.ycoef, j.csc.yoff), 0x00000501u);
        const uint32_t y23 = perm_b32(dot4_u8(px[r][3], j.csc.ycoef, j.csc.yoff), dot4_u8(px[r][2], j.csc.ycoef, j.csc.yoff), 0x00000501u);
        const uint32_t o = perm_b32(y23, y01, 0x05040100u);
        uint8_t *yrow = j.dst[0] + (size_t) (y0 + r) * (size_t) j.ystride;
        if (WIDE || x + 4 <= w) {
            st_global<uint32_t>(yrow, x, o); // (x is a multiple of 4, the plane's origin and stride of 16)
        } else {
            for (int i = 0; x + i < w; i++) {
                st_global<uint8_t>(yrow, x + i, (uint8_t) (o >> (8 * i)));
            }
        }
    }
    rgb_chroma<HS, VS, WIDE>(j, px, x, y0, j.dst[1], j.csc.upos, j.csc.uneg);
    rgb_chroma<HS, VS, WIDE>(j, px, x, y0, j.dst[2], j.csc.vpos, j.csc.vneg);
}

// rows y0 .. y0 + 3 (y0 a multiple of 4, below h) of job j, pixels x_first .. x_first + 3 (a multiple of 4) and on in steps of x_step,
// for a stream with chroma shifts HS, VS
template <int VEC, int HS, int VS> __host__ __device__ __forceinline__ void ingest_rgb_rows_fmt(const RgbJob &j, int y0, int x_first, int x_step)
{
    static_assert(VEC == 16 || VEC == 4, "wide or general form");
    constexpr bool WIDE = VEC == 16;
    const int w = j.w, h = j.h;
    // general form: pixels are dwords where every row of the surface starts 4-byte aligned -- one decision for the job, as any surface
    // a renderer made has it; on a surface with a pointer or pitch off that grid every pixel goes byte by byte, the rows that happen
    // to be aligned too
    const bool aligned = ((((uintptr_t) j.src) | j.pitch) & 3) == 0;
    (void) aligned;
    for (int xi = x_first; xi < w; xi += x_step) {
        const int x = lane_offset(xi);
        uint32_t px[4][4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = y0 + r < h ? y0 + r : h - 1; // (rows below the picture: read again from its last row, never stored)
            const uint8_t *row = j.src + (size_t) y * j.pitch;
            if constexpr (WIDE) {
                const u32x4 q = ld_global<u32x4>(row, 4 * (uint32_t) x);
                px[r][0] = q[0], px[r][1] = q[1], px[r][2] = q[2], px[r][3] = q[3];
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int xc = x + i < w ? x + i : w - 1; // (pixels right of the picture: its last pixel again)
                    px[r][i] = rgb_pixel(row, 4 * (uint32_t) xc, aligned);
                }
            }
        }
        rgb_emit<HS, VS, WIDE>(j, px, x, y0);
    }
}

// The stream's format (DSV_SUBSAMP_*) is one value for the whole launch, so the switch stands outside the row loop: each format's
// loop keeps only its own row bases in scalar registers (one loop with the switch inside held all five formats' and spilled some).
template <int VEC> __host__ __device__ __forceinline__ void ingest_rgb_rows(const RgbJob &j, int y0, int x_first, int x_step)
{
    switch (4 * j.hs + j.vs) {
    case 0x0:
        ingest_rgb_rows_fmt<VEC, 0, 0>(j, y0, x_first, x_step);
        break;
    case 0x4:
        ingest_rgb_rows_fmt<VEC, 1, 0>(j, y0, x_first, x_step);
        break;
    case 0x5:
        ingest_rgb_rows_fmt<VEC, 1, 1>(j, y0, x_first, x_step);
        break;
    case 0x8:
        ingest_rgb_rows_fmt<VEC, 2, 0>(j, y0, x_first, x_step);
        break;
    default: // 0xA, "4:1:0" (the host lets no other format through)
        ingest_rgb_rows_fmt<VEC, 2, 2>(j, y0, x_first, x_step);
        break;
    }
}

} // namespace dsv2
