// ingest_rgb3.h -- what one thread of k_ingest_rgb3 (ingest.hip) does, as a function that also compiles for the host (the pattern of
// ingest_rgb.h): the kernel is this function behind blockIdx / threadIdx, and tools/ingest_rgb3_check.cpp sweeps the very same code
// on the CPU under AddressSanitizer -- kinds, forms, byte orders, presets, formats, widths, pitches and offsets -- before it runs on a GPU.
//
// One Rgb3Job (io_jobs.h) = one RGB surface WITHOUT a fourth byte (dsv2hip_surface) on its way into the three bordered source planes:
//   kRgb3Packed: BGR / RGB, three bytes a pixel in one plane (OpenCV's Mat, a numpy / torch uint8[h, w, 3]);
//   kRgb3Planar: RGBP, one plane per colour (torch's uint8[3, h, w]).
// The decomposition is k_ingest_rgb's: a thread owns FOUR pixels of FOUR consecutive rows, rows below h and pixels right of w are
// read again from the last row / pixel and never stored, every load is issued before the first store.  Only the fetch is new: once
// the thread holds its px[4][4] pixel dwords with the colour bytes in bytes 0..2, luma, chroma and the stores are ingest_rgb.h's
// rgb_emit, text and all.  Byte 3 of a pixel dword weighs 0 in every coefficient quad, so it holds whatever the fetch left there.
//   wide, packed:  pointer and pitch multiples of 4 and w of 4 in every such job of the launch (rgb3_job_wide): the thread's 4 pixels
//                  are the 12 bytes at 3 * x, dword-aligned as x is a multiple of 4 -- one 12-byte load d0 d1 d2 per row, the
//                  pixels d0, alignbyte(d1 : d0, 3), alignbyte(d2 : d1, 2), d2 >> 8.  The last dword ends where the row ends.
//   wide, planar:  the three pointers and pitches multiples of 4 and w of 4: one dword per plane per row, zipped into the four
//                  pixel dwords by six v_perm_b32 (R G pairs first, then B into each pixel).
//   general:       any w, pitch and alignment: the colour bytes one by one, coordinates clamped to w - 1 / h - 1.
// The coefficient quads are RgbJob's, in the order the colour bytes take in the pixel dword: memory order for the packed kind (so
// BGR and RGB differ only in the job's data), R G B for the planar kind (the planes are named by pointer).
#pragma once

#include "ingest_rgb.h"

namespace dsv2 {

// bytes n .. n + 3 of the eight bytes hi : lo
__host__ __device__ __forceinline__ uint32_t alignbyte_b32(uint32_t hi, uint32_t lo, uint32_t n)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, n);
#else
    return (uint32_t) ((((uint64_t) hi << 32) | lo) >> (8 * n));
#endif
}

// rows y0 .. y0 + 3 (y0 a multiple of 4, below h) of job j, pixels x_first .. x_first + 3 (a multiple of 4) and on in steps of x_step,
// for a stream with chroma shifts HS, VS
template <int KIND, bool WIDE, int HS, int VS> __host__ __device__ __forceinline__ void ingest_rgb3_rows_fmt(const Rgb3Job &j, int y0, int x_first, int x_step)
{
    static_assert(KIND == kRgb3Packed || KIND == kRgb3Planar, "packed or planar");
    constexpr bool PLANAR = KIND == kRgb3Planar;
    const int w = j.w, h = j.h;
    // what rgb_emit reads of a job: destination, geometry, coefficients
    const RgbJob o{nullptr, 0, {j.dst[0], j.dst[1], j.dst[2]}, j.ystride, j.cstride, w, h, j.hs, j.vs, j.csc};
    for (int xi = x_first; xi < w; xi += x_step) {
        const int x = lane_offset(xi);
        uint32_t px[4][4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = y0 + r < h ? y0 + r : h - 1; // (rows below the picture: read again from its last row, never stored)
            // colour byte c of pixel x of this row: packed, row0[3 * x + c]; planar, rowc[x]
            const uint8_t *row0 = j.src[0] + (size_t) y * j.pitch[0];
            const uint8_t *row1 = PLANAR ? j.src[1] + (size_t) y * j.pitch[1] : row0 + 1;
            const uint8_t *row2 = PLANAR ? j.src[2] + (size_t) y * j.pitch[2] : row0 + 2;
            if constexpr (WIDE && !PLANAR) {
                // 12 bytes at 3 * x, a multiple of 12, and 3 * x + 12 <= 3 * w as x + 4 <= w; three dwords off ONE address, which is what
                // lets the compiler see that they are consecutive and make them one global_load_dwordx3
                const DSV2_GLOBAL uint32_t *q = (const DSV2_GLOBAL uint32_t *) (row0 + 3 * (uint32_t) x);
                const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
                px[r][0] = d0, px[r][1] = alignbyte_b32(d1, d0, 3), px[r][2] = alignbyte_b32(d2, d1, 2), px[r][3] = d2 >> 8;
            } else if constexpr (WIDE) {
                const uint32_t cr = ld_global<uint32_t>(row0, (uint32_t) x), cg = ld_global<uint32_t>(row1, (uint32_t) x), cb = ld_global<uint32_t>(row2, (uint32_t) x);
                const uint32_t rg01 = perm_b32(cg, cr, kZipLo), rg23 = perm_b32(cg, cr, kZipHi); // R0 G0 R1 G1, R2 G2 R3 G3
                px[r][0] = perm_b32(cb, rg01, 0x00040100u), px[r][1] = perm_b32(cb, rg01, 0x00050302u);
                px[r][2] = perm_b32(cb, rg23, 0x00060100u), px[r][3] = perm_b32(cb, rg23, 0x00070302u);
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int xc = x + i < w ? x + i : w - 1; // (pixels right of the picture: its last pixel again)
                    const uint32_t at = (PLANAR ? 1u : 3u) * (uint32_t) xc;
                    px[r][i] = (uint32_t) ld_global<uint8_t>(row0, at) | ((uint32_t) ld_global<uint8_t>(row1, at) << 8) | ((uint32_t) ld_global<uint8_t>(row2, at) << 16);
                }
            }
        }
        rgb_emit<HS, VS, WIDE>(o, px, x, y0);
    }
}

// The stream's format is one value for the whole launch, so the switch stands outside the row loop (ingest_rgb.h).
template <int KIND, bool WIDE> __host__ __device__ __forceinline__ void ingest_rgb3_rows(const Rgb3Job &j, int y0, int x_first, int x_step)
{
    switch (4 * j.hs + j.vs) {
    case 0x0:
        ingest_rgb3_rows_fmt<KIND, WIDE, 0, 0>(j, y0, x_first, x_step);
        break;
    case 0x4:
        ingest_rgb3_rows_fmt<KIND, WIDE, 1, 0>(j, y0, x_first, x_step);
        break;
    case 0x5:
        ingest_rgb3_rows_fmt<KIND, WIDE, 1, 1>(j, y0, x_first, x_step);
        break;
    case 0x8:
        ingest_rgb3_rows_fmt<KIND, WIDE, 2, 0>(j, y0, x_first, x_step);
        break;
    default: // 0xA, "4:1:0" (the host lets no other format through)
        ingest_rgb3_rows_fmt<KIND, WIDE, 2, 2>(j, y0, x_first, x_step);
        break;
    }
}

} // namespace dsv2
