// egress_rgb.h -- what one thread of k_egress_rgb (egress.hip) does, as a function that also compiles for the host (the pattern of
// egress_uv.h and ingest_rgb.h): the kernel is this function behind blockIdx / threadIdx, and tools/egress_rgb_check.cpp sweeps the
// very same code on the CPU under AddressSanitizer -- forms, byte orders, presets, formats, widths, pitches and offsets -- before it
// runs on a GPU.
//
// One RgbOutJob (io_jobs.h) = one decoded picture on its way into a packed four-byte RGB surface (dsv2hip_out_surface, layout BGRA /
// RGBA), converted on the way by the integer formulas of include/dsv2_hip.h (the contract; restated at rgb_terms below).  The
// mirror image of ingest_rgb.h: a thread owns FOUR pixels of FOUR consecutive rows -- a whole number of chroma footprints of every
// format, so a chroma sample is read and its three products formed once for all the pixels it covers; rows below h are read again
// from the last row and never stored; every load is issued before the first store, and a row leaves as 16 bytes.
//   Sources: luma is one aligned dword per row (x is a multiple of 4, the plane's origin and stride of 16; the up to three bytes
//            past the row lie in the plane's border, or inside the stride of the decoder's staged luma).  What four pixels hold of
//            chroma is a dword (4:4:4), an aligned pair of bytes (4:2:2, 4:2:0: x >> 1 is even) or one byte (4:1:1, "4:1:0") per
//            chroma row -- never an unaligned word; a sample right of cw is border, and belongs to pixels that are not stored.
//   WIDE:    destination pointer and pitch multiples of 16 and w a multiple of 4 in every job of the launch (the host picks it per
//            round, rgb_out_job_wide): one unconditional 16-byte store per row.
//   general: any w, pitch and alignment.  A pixel is stored only where x < w: as one dword where its address is a multiple of 4,
//            else as its four bytes -- no byte outside the h row pieces of 4 * w bytes is ever written.
// The byte order is data: the job says which of R and B is byte 0, and the two outer bytes' coefficient pairs are picked from it
// once, in scalar registers; every byte of a pixel is then the same multiply-add chain, and alpha is the constant 255.
#pragma once

#include "ingest_rgb.h" // ld_global, st_global, u32x4, lane_offset

namespace dsv2 {

// a * b + c for |a|, |b| < 2^23: v_mad_i32_i24 (every product of the conversion has a coefficient below 1024 and a sample below 256)
__host__ __device__ __forceinline__ int mad24(int a, int b, int c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b) + c;
#else
    return a * b + c;
#endif
}

// clamp(v >> 8, 0, 255) is byte 1 of clamp(v, 0, 65535): the sum is clamped FIRST (one v_med3_i32) and its byte 1 picked by the
// v_perm_b32 that packs the pixel -- no shift, and not the shape "shift, clamp to a byte, pack two" that hipcc turns into
// v_ashr_pk_u8_i32: it then ORs that instruction's result as if its upper 16 bits were zero, and on an MI355X byte 2 of 4 % of the
// pixels came out with stray bits set (the first build of this file)
__host__ __device__ __forceinline__ uint32_t rgb_sum16(int v) { return (uint32_t) (v < 0 ? 0 : v > 65535 ? 65535 : v); }

struct RgbTerms { // a job's conversion, per byte of the pixel: byte k = clamp((ky * Y + cu[k] * U + cv[k] * V + off[k]) >> 8, 0, 255)
    int ky, cu[3], cv[3], off[3];
};
// With C = ky * (Y - ybase), D = U - 128, E = V - 128 (include/dsv2_hip.h):
//   R = clamp((C + rv * E + 128) >> 8),  G = clamp((C + gu * D + gv * E + 128) >> 8),  B = clamp((C + bu * D + 128) >> 8)
// multiplied out, the constants gathered: off = 128 - ky * ybase - 128 * (cu + cv).  Integer arithmetic: the same sum bit for bit.
__host__ __device__ __forceinline__ RgbTerms rgb_terms(const RgbOutJob &j)
{
    RgbTerms t;
    t.ky = j.csc.ky;
    t.cu[0] = j.bgra ? j.csc.bu : 0, t.cv[0] = j.bgra ? 0 : j.csc.rv; // byte 0: B or R
    t.cu[1] = j.csc.gu, t.cv[1] = j.csc.gv;
    t.cu[2] = j.bgra ? 0 : j.csc.bu, t.cv[2] = j.bgra ? j.csc.rv : 0; // byte 2: R or B
    for (int k = 0; k < 3; k++) {
        t.off[k] = 128 - j.csc.ky * j.csc.ybase - 128 * (t.cu[k] + t.cv[k]);
    }
    return t;
}

// rows y0 .. y0 + 3 (y0 a multiple of 4, below h) of job j, pixels x_first .. x_first + 3 (a multiple of 4) and on in steps of x_step,
// for a stream with chroma shifts HS, VS
template <bool WIDE, int HS, int VS> __host__ __device__ __forceinline__ void egress_rgb_rows_fmt(const RgbOutJob &j, int y0, int x_first, int x_step)
{
    constexpr int NX = 4 >> HS, NY = 4 >> VS; // chroma samples per row, chroma rows of the thread's 4 x 4 pixels
    const int w = j.w, h = j.h;
    const RgbTerms t = rgb_terms(j);
    for (int xi = x_first; xi < w; xi += x_step) {
        const int x = lane_offset(xi);
        uint32_t ly[4], cu[NY], cv[NY];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = y0 + r < h ? y0 + r : h - 1; // (rows below the picture: read again from its last row, never stored)
            ly[r] = ld_global<uint32_t>(j.sy + (size_t) y * (size_t) j.ystride, (uint32_t) x);
        }
#pragma unroll
        for (int k = 0; k < NY; k++) {
            const int y = y0 + (k << VS) < h ? y0 + (k << VS) : h - 1; // (the 1 << VS rows of a footprint clamp to the same chroma row)
            const size_t off = (size_t) (y >> VS) * (size_t) j.cstride;
            const uint32_t cx = (uint32_t) x >> HS;
            if constexpr (HS == 0) {
                cu[k] = ld_global<uint32_t>(j.su + off, cx), cv[k] = ld_global<uint32_t>(j.sv + off, cx);
            } else if constexpr (HS == 1) {
                cu[k] = ld_global<uint16_t>(j.su + off, cx), cv[k] = ld_global<uint16_t>(j.sv + off, cx);
            } else {
                cu[k] = ld_global<uint8_t>(j.su + off, cx), cv[k] = ld_global<uint8_t>(j.sv + off, cx);
            }
        }
#pragma unroll
        for (int k = 0; k < NY; k++) {
            int c[NX][3]; // what the chroma sample adds to each byte of its pixels
#pragma unroll
            for (int s = 0; s < NX; s++) {
                const int u = (int) ((cu[k] >> (8 * s)) & 0xffu), v = (int) ((cv[k] >> (8 * s)) & 0xffu);
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    c[s][b] = mad24(t.cu[b], u, mad24(t.cv[b], v, t.off[b]));
                }
            }
#pragma unroll
            for (int r = k << VS; r < (k + 1) << VS; r++) {
                if (y0 + r >= h) {
                    break;
                }
                uint32_t o[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int yv = (int) ((ly[r] >> (8 * i)) & 0xffu);
                    const int *cs = c[i >> HS];
                    const uint32_t b0 = rgb_sum16(mad24(t.ky, yv, cs[0])), b1 = rgb_sum16(mad24(t.ky, yv, cs[1])), b2 = rgb_sum16(mad24(t.ky, yv, cs[2]));
                    // byte 1 of each clamped sum: b0 and b1 into bytes 0 and 1, then b2 into byte 2 (its byte 3 is zero)
                    o[i] = perm_b32(b2, perm_b32(b1, b0, 0x00000501u), 0x07050100u) | 0xff000000u;
                }
                uint8_t *drow = j.dst + (size_t) (y0 + r) * (size_t) j.dpitch;
                if constexpr (WIDE) {
                    st_global<u32x4>(drow, 4 * (uint32_t) x, u32x4{o[0], o[1], o[2], o[3]});
                } else {
                    const bool aligned = (((uintptr_t) drow) & 3) == 0;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        if (x + i >= w) {
                            break;
                        }
                        const uint32_t at = 4 * (uint32_t) (x + i);
                        if (aligned) {
                            st_global<uint32_t>(drow, at, o[i]);
                        } else {
                            for (int b = 0; b < 4; b++) {
                                st_global<uint8_t>(drow, at + (uint32_t) b, (uint8_t) (o[i] >> (8 * b)));
                            }
                        }
                    }
                }
            }
        }
    }
}

// The stream's format is one value for the whole launch, so the switch stands outside the row loop (ingest_rgb.h).
template <bool WIDE> __host__ __device__ __forceinline__ void egress_rgb_rows(const RgbOutJob &j, int y0, int x_first, int x_step)
{
    switch (4 * j.hs + j.vs) {
    case 0x0:
        egress_rgb_rows_fmt<WIDE, 0, 0>(j, y0, x_first, x_step);
        break;
    case 0x4:
        egress_rgb_rows_fmt<WIDE, 1, 0>(j, y0, x_first, x_step);
        break;
    case 0x5:
        egress_rgb_rows_fmt<WIDE, 1, 1>(j, y0, x_first, x_step);
        break;
    case 0x8:
        egress_rgb_rows_fmt<WIDE, 2, 0>(j, y0, x_first, x_step);
        break;
    default: // 0xA, "4:1:0" (the host lets no other format through)
        egress_rgb_rows_fmt<WIDE, 2, 2>(j, y0, x_first, x_step);
        break;
    }
}

} // namespace dsv2
