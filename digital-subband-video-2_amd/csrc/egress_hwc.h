// egress_hwc.h -- what one thread of k_egress_hwc (egress.hip) does, as a function that also compiles for the host (the pattern of
// egress_rgb.h and egress_tensor.h): the kernel is this function behind blockIdx / threadIdx, and tools/egress_hwc_check.cpp sweeps the
// very same code on the CPU under AddressSanitizer -- forms, element types, orders, presets, formats, widths, pitches and offsets --
// before it runs on a GPU.
//
// One HwcOutJob (io_jobs.h) = one decoded picture on its way into an interleaved [h, w, 3] tensor (dsv2hip_out_hwc), converted on the
// way by the integer formulas of include/dsv2_hip.h (egress_rgb.h's rgb_terms, mad24 and rgb_sum16 with the job's element order) and,
// for a float element type, taken through the job's per-element scale and bias (tensor_num.h).  k_egress_rgb's shape: a thread owns
// FOUR pixels of FOUR consecutive rows -- a whole number of chroma footprints of every format; rows below h are read again from the
// last row and never stored; every load is issued before the first store.  What is new: a row of the thread's four pixels is TWELVE
// consecutive elements, and it leaves as whole vector stores -- three dwords (uint8: 12 bytes), three 8-byte stores (binary16,
// bfloat16: 24 bytes) or three 16-byte stores (binary32: 48 bytes) -- so a wavefront writes 768 B / 1.5 KiB / 3 KiB of one contiguous
// row, where k_egress_tensor wrote three streams a quarter that size.
//   WIDE:    pointer and pitch a multiple of four elements and w a multiple of 4 in every job of the launch (the host picks it per round,
//            hwc_job_wide): unconditional vector stores.
//   general: any element-aligned pointer and pitch, any w.  The twelve elements leave as the wide form's vectors where the row's address
//            is aligned for them and all four pixels lie inside the row, else element by element where the pixel lies inside it -- no
//            byte outside the h row pieces of 3 * w elements is ever written.
// The element type is data of the job, one value for the whole workgroup: the switch on it stands outside the loops, around the switch
// on the stream's format.  THE FLOAT CONTRACT is egress_tensor.h's, with the constants of element k of a pixel in place of a plane's.
#pragma once

#include "egress_rgb.h"
#include "tensor_num.h"

namespace dsv2 {

// the conversion's terms with element 0 = B (order B G R) or R (order R G B): the RGB surface's byte order word
__host__ __device__ __forceinline__ RgbTerms hwc_terms(const HwcOutJob &j)
{
    RgbOutJob r{};
    r.csc = j.csc, r.bgra = j.bgra;
    return rgb_terms(r);
}

// bytes 1 of four clamped 16-bit sums into one dword, a's in byte 0 (egress_rgb.h: no shift, clamp and pack)
__host__ __device__ __forceinline__ uint32_t hwc_pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    return perm_b32(perm_b32(d, c, 0x00000501u), perm_b32(b, a, 0x00000501u), 0x05040100u);
}

// one row of the thread's four pixels -- s[n], n = 3 * i + k: element k of pixel x + i as a clamped 16-bit sum whose byte 1 is the
// sample -- into row `drow` at pixel x (a multiple of 4)
template <bool WIDE, int DT>
__host__ __device__ __forceinline__ void hwc_store(uint8_t *drow, int x, int w, const uint32_t (&s)[12], const float (&scale)[3], const float (&bias)[3])
{
    constexpr uint32_t ELEM = DT == kTensorU8 ? 1 : DT == kTensorF32 ? 4 : 2;
    const uint32_t at = 3 * ELEM * (uint32_t) x;
    const bool whole = WIDE || ((((uintptr_t) drow) & (4 * ELEM - 1)) == 0 && x + 4 <= w);
    const int n_in = WIDE ? 12 : 3 * (w - x < 4 ? w - x : 4); // elements of the twelve that lie inside the row
    if constexpr (DT == kTensorU8) {
        const uint32_t o[3] = {hwc_pack4(s[0], s[1], s[2], s[3]), hwc_pack4(s[4], s[5], s[6], s[7]), hwc_pack4(s[8], s[9], s[10], s[11])};
        if (whole) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                st_global<uint32_t>(drow, at + 4 * (uint32_t) q, o[q]);
            }
        } else {
#pragma unroll
            for (int n = 0; n < 12; n++) {
                if (n < n_in) {
                    st_global<uint8_t>(drow, at + (uint32_t) n, (uint8_t) (o[n >> 2] >> (8 * (n & 3))));
                }
            }
        }
    } else {
        uint32_t e[12];
        if constexpr (DT == kTensorF16) {
#pragma unroll
            for (int n = 0; n < 12; n += 2) {
                const float f0 = tensor_affine((float) ((s[n] >> 8) & 0xffu), scale[n % 3], bias[n % 3]);
                const float f1 = tensor_affine((float) ((s[n + 1] >> 8) & 0xffu), scale[(n + 1) % 3], bias[(n + 1) % 3]);
                const uint32_t p = tensor_f16_pair(f0, f1);
                e[n] = p & 0xffffu, e[n + 1] = p >> 16;
            }
        } else {
#pragma unroll
            for (int n = 0; n < 12; n++) {
                const float f = tensor_affine((float) ((s[n] >> 8) & 0xffu), scale[n % 3], bias[n % 3]);
                e[n] = DT == kTensorF32 ? tensor_f32_bits(f) : tensor_bf16_bits(f);
            }
        }
        if constexpr (DT == kTensorF32) {
            if (whole) {
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    st_global<u32x4>(drow, at + 16 * (uint32_t) q, u32x4{e[4 * q], e[4 * q + 1], e[4 * q + 2], e[4 * q + 3]});
                }
            } else {
#pragma unroll
                for (int n = 0; n < 12; n++) {
                    if (n < n_in) {
                        st_global<uint32_t>(drow, at + 4 * (uint32_t) n, e[n]);
                    }
                }
            }
        } else {
            if (whole) {
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    st_global<u32x2>(drow, at + 8 * (uint32_t) q, u32x2{e[4 * q] | (e[4 * q + 1] << 16), e[4 * q + 2] | (e[4 * q + 3] << 16)});
                }
            } else {
#pragma unroll
                for (int n = 0; n < 12; n++) {
                    if (n < n_in) {
                        st_global<uint16_t>(drow, at + 2 * (uint32_t) n, (uint16_t) e[n]);
                    }
                }
            }
        }
    }
}

// rows y0 .. y0 + 3 (y0 a multiple of 4, below h) of job j, pixels x_first .. x_first + 3 (a multiple of 4) and on in steps of x_step,
// for element type DT and a stream with chroma shifts HS, VS
template <bool WIDE, int DT, int HS, int VS>
__host__ __device__ __forceinline__ void egress_hwc_rows_fmt(const HwcOutJob &j, int y0, int x_first, int x_step)
{
    constexpr int NX = 4 >> HS, NY = 4 >> VS; // chroma samples per row, chroma rows of the thread's 4 x 4 pixels
    const int w = j.w, h = j.h;
    const RgbTerms t = hwc_terms(j);
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
            const size_t off = (size_t) row_number(y >> VS) * (size_t) j.cstride;
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
            int c[NX][3]; // what the chroma sample adds to elements 0, 1, 2 of its pixels
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
                uint32_t s[12]; // the row's twelve elements in memory order
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int yv = (int) ((ly[r] >> (8 * i)) & 0xffu);
#pragma unroll
                    for (int b = 0; b < 3; b++) {
                        s[3 * i + b] = rgb_sum16(mad24(t.ky, yv, c[i >> HS][b]));
                    }
                }
                hwc_store<WIDE, DT>(j.dst + (size_t) row_number(y0 + r) * (size_t) j.dpitch, x, w, s, j.scale, j.bias);
            }
        }
    }
}

// The stream's format is one value for the whole launch, so the switch stands outside the row loop (egress_rgb.h) ...
template <bool WIDE, int DT> __host__ __device__ __forceinline__ void egress_hwc_rows_dt(const HwcOutJob &j, int y0, int x_first, int x_step)
{
    switch (4 * j.hs + j.vs) {
    case 0x0:
        egress_hwc_rows_fmt<WIDE, DT, 0, 0>(j, y0, x_first, x_step);
        break;
    case 0x4:
        egress_hwc_rows_fmt<WIDE, DT, 1, 0>(j, y0, x_first, x_step);
        break;
    case 0x5:
        egress_hwc_rows_fmt<WIDE, DT, 1, 1>(j, y0, x_first, x_step);
        break;
    case 0x8:
        egress_hwc_rows_fmt<WIDE, DT, 2, 0>(j, y0, x_first, x_step);
        break;
    default: // 0xA, "4:1:0" (the host lets no other format through)
        egress_hwc_rows_fmt<WIDE, DT, 2, 2>(j, y0, x_first, x_step);
        break;
    }
}

// ... and so does the one on the job's element type, one value for the whole workgroup.
template <bool WIDE> __host__ __device__ __forceinline__ void egress_hwc_rows(const HwcOutJob &j, int y0, int x_first, int x_step)
{
    switch (j.dtype) {
    case kTensorU8:
        egress_hwc_rows_dt<WIDE, kTensorU8>(j, y0, x_first, x_step);
        break;
    case kTensorF16:
        egress_hwc_rows_dt<WIDE, kTensorF16>(j, y0, x_first, x_step);
        break;
    case kTensorBF16:
        egress_hwc_rows_dt<WIDE, kTensorBF16>(j, y0, x_first, x_step);
        break;
    default: // kTensorF32 (the host lets no other element type through)
        egress_hwc_rows_dt<WIDE, kTensorF32>(j, y0, x_first, x_step);
        break;
    }
}

} // namespace dsv2
