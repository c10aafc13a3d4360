// egress_uv.h -- what one thread of k_egress_uv (egress.hip) does, as a function that also compiles for the host: the kernel is
// this function behind blockIdx / threadIdx, and tools/egress_uv_check.cpp sweeps the very same code on the CPU under
// AddressSanitizer -- widths, pitches, offsets and modes -- before it ever runs on a GPU.
//
// One UvEgressJob (io_jobs.h) = the two chroma planes of one decoded picture on their way into the interleaved plane of a
// semiplanar surface (NV12 / NV16 / NV24: rows U0 V0 U1 V1 ...).  A thread owns VEC (U, V) pairs -- 2 * VEC destination bytes -- of
// FOUR consecutive rows; every load is issued before the first store.
//   VEC = 8, the wide form: destination pointer and pitch multiples of 16 and cw a multiple of 8 in every job of the launch (the
//            host picks it per round): 8 bytes of U and 8 of V per row, zipped by four v_perm_b32 into one 16-byte store -- the
//            inverse of k_ingest_surface's split (ingest.hip).
//   VEC = 4, the general form: any cw, pitch and alignment.  Whole dwords are read from the sources (x is a multiple of 4 and
//            the planes' origins and strides of 16; the up to three bytes past the row lie in the 32-pixel border); a destination
//            dword is stored as one only where it is aligned and lies whole inside the row, else byte by byte inside the row:
//            no byte outside the ch row pieces of 2 * cw bytes is ever written.
//   CONV:    the samples are the reference CLI's -out420p conversions (util.c:79-153, mode 1..4 as k_to420, frame.hip, computes
//            them: rounded pair averages, the second operand clamped at the plane edge) of the source planes, gathered byte
//            by byte at coordinates clamped into the source plane -- no 4:2:0 planar picture exists in between.  j.mode is a
//            run-time switch inside this one instantiation (it also serves mode 0 jobs of a round that mixes converted and
//            unconverted pictures): four more instantiations per form would each keep three dead conversions out of a kernel
//            whose cost is its byte loads, not its branches, and the switch is uniform over the launch's workgroup.
#pragma once

#include "io_jobs.h"

namespace dsv2 {

constexpr uint32_t kZipLo = 0x05010400u, kZipHi = 0x07030602u; // bytes 0, 1 / 2, 3 of the second and of the first operand of v_perm_b32, alternating

__host__ __device__ __forceinline__ uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t) hi << 32) | lo; // (selectors 0..7 only: all this file uses)
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        r |= (uint32_t) ((v >> (8 * ((sel >> (8 * i)) & 7))) & 0xffu) << (8 * i);
    }
    return r;
#endif
}

// sample (x, y) of the delivered chroma plane from source plane s; x < j.cw, y < j.ch
__host__ __device__ __forceinline__ uint32_t uv_sample(const uint8_t *s, const UvEgressJob &j, int x, int y)
{
    const int sw = j.sw, sh = j.sh;
    const size_t st = (size_t) j.sstride;
    if (j.mode == 0) {
        return s[(size_t) y * st + x];
    }
    if (j.mode == 4) { // "4:1:0": conv410to420
        const int sx = x >> 1 < sw - 1 ? x >> 1 : sw - 1, sy = y >> 1 < sh - 1 ? y >> 1 : sh - 1;
        return s[(size_t) sy * st + sx];
    }
    const int y0 = 2 * y, y1 = y0 < sh - 1 ? y0 + 1 : sh - 1;
    const uint8_t *r0 = s + (size_t) y0 * st, *r1 = s + (size_t) y1 * st;
    if (j.mode == 1) { // 4:4:4: conv444to422 then conv422to420
        const int x0 = 2 * x, x1 = x0 < sw - 1 ? x0 + 1 : sw - 1;
        const uint32_t a = ((uint32_t) r0[x0] + r0[x1] + 1) >> 1, b = ((uint32_t) r1[x0] + r1[x1] + 1) >> 1;
        return (a + b + 1) >> 1;
    }
    const int sx = j.mode == 2 ? x : (x >> 1 < sw - 1 ? x >> 1 : sw - 1); // 4:2:2: conv422to420; 4:1:1: conv411to420
    return ((uint32_t) r0[sx] + r1[sx] + 1) >> 1;
}

// rows y0 .. y0 + 3 of job j, pairs x_first .. x_first + VEC - 1 and on in steps of x_step
template <int VEC, bool CONV> __host__ __device__ __forceinline__ void egress_uv_rows(const UvEgressJob &j, int y0, int x_first, int x_step)
{
    static_assert(VEC == 8 || VEC == 4, "wide or general form");
    constexpr int NS = VEC / 4; // source dwords of each plane per row
    constexpr int NW = VEC / 2; // destination dwords per row
    const int cw = j.cw, ch = j.ch;
    for (int x = x_first; x < cw; x += x_step) {
        uint32_t ru[4][NS], rv[4][NS], o[4][NW];
        (void) ru, (void) rv; // (CONV gathers straight into o)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = y0 + r < ch ? y0 + r : ch - 1; // (rows below the plane: read again from its last row, never stored)
            if constexpr (CONV) {
#pragma unroll
                for (int k = 0; k < NW; k++) {
                    const int xa = x + 2 * k < cw ? x + 2 * k : cw - 1, xb = x + 2 * k + 1 < cw ? x + 2 * k + 1 : cw - 1; // (pairs past the row: never stored)
                    o[r][k] = uv_sample(j.su, j, xa, y) | (uv_sample(j.sv, j, xa, y) << 8) | (uv_sample(j.su, j, xb, y) << 16) |
                              (uv_sample(j.sv, j, xb, y) << 24);
                }
            } else {
                const size_t off = (size_t) y * (size_t) j.sstride + (size_t) x;
                if constexpr (VEC == 8) {
                    const uint2 u = *(const uint2 *) (j.su + off), v = *(const uint2 *) (j.sv + off);
                    ru[r][0] = u.x, ru[r][1] = u.y, rv[r][0] = v.x, rv[r][1] = v.y;
                } else {
                    ru[r][0] = *(const uint32_t *) (j.su + off);
                    rv[r][0] = *(const uint32_t *) (j.sv + off);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (y0 + r >= ch) {
                break;
            }
            if constexpr (!CONV) {
#pragma unroll
                for (int k = 0; k < NS; k++) {
                    o[r][2 * k] = perm_b32(rv[r][k], ru[r][k], kZipLo);     // U0 V0 U1 V1
                    o[r][2 * k + 1] = perm_b32(rv[r][k], ru[r][k], kZipHi); // U2 V2 U3 V3
                }
            }
            uint8_t *dp = j.dst + (size_t) (y0 + r) * (size_t) j.dpitch + 2 * (size_t) x;
            if constexpr (VEC == 8) {
                *(uint4 *) dp = make_uint4(o[r][0], o[r][1], o[r][2], o[r][3]);
            } else {
#pragma unroll
                for (int k = 0; k < NW; k++) {
                    uint8_t *q = dp + 4 * k;
                    if (x + 2 * k + 2 <= cw && (((uintptr_t) q) & 3) == 0) {
                        *(uint32_t *) q = o[r][k];
                    } else {
                        for (int i = 0; i < 4 && 2 * (x + 2 * k) + i < 2 * cw; i++) {
                            q[i] = (uint8_t) (o[r][k] >> (8 * i));
                        }
                    }
                }
            }
        }
    }
}

} // namespace dsv2
