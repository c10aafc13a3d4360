// ingest_hwc.h -- what one thread of k_ingest_hwc (ingest.hip) does, as a function that also compiles for the host (the pattern of
// ingest_tensor.h): the kernel is this function behind blockIdx / threadIdx, and tools/ingest_hwc_check.cpp sweeps the very same code
// on the CPU under AddressSanitizer -- forms, element types, orders, presets, formats, widths, pitches, offsets and constants -- before
// it runs on a GPU.
//
// One HwcInJob (io_jobs.h) = one picture that is a caller's interleaved [h, w, 3] float tensor (dsv2hip_in_hwc: binary16, bfloat16 or
// binary32 elements, R G B or B G R) on its way into the three bordered source planes.  The decomposition is k_ingest_rgb3's: a thread
// owns FOUR pixels of FOUR consecutive rows, rows below h and pixels right of w are read again from the last row / pixel and never
// stored.  Only the fetch is new: a thread's row is TWELVE consecutive elements at 3 * x * elem, and element 3 * i + k goes through
// ingest_tensor.h's tensor_in_pack into byte k of pixel dword i under scale[k], bias[k] -- the constants belong to memory positions,
// and memory order is byte order, so B G R and R G B differ only in the job's coefficient quads, as for a packed Rgb3Job.  Luma, chroma
// and the stores are ingest_rgb.h's rgb_emit, text and all.
//   WIDE:    pointer and pitch multiples of four elements and w a multiple of 4 in every job of the launch (the host picks it per
//            step, hwc_in_job_wide): the twelve elements are three loads off ONE address, 8 bytes each for the half types (24 bytes,
//            8-byte aligned as x is a multiple of 4), 16 bytes each for binary32 (48 bytes, 16-byte aligned).  A wavefront reads 1.5 /
//            3 KiB of one contiguous row, but each of the three instructions has its lanes 24 / 48 bytes apart.
//   general: any element-aligned pointer and pitch, any w: element by element, the pixel's coordinates clamped to w - 1 / h - 1.
// A binary16 / bfloat16 dword now pairs elements of DIFFERENT channels, and at odd positions of different pixels: dword m holds
// elements 2 m and 2 m + 1 of the twelve, whatever pixel and channel those are.
// Loads in flight, as ingest_tensor.h reasons: the half types issue all twelve loads of a pass (four rows of three) before the first
// conversion, 24 registers of raw data; binary32 takes its rows TWO at a time (24 registers), with the scheduling barrier between
// the pairs.  Row bases are formed where they are used (row_number).  Element type and stream format are switched outside the loops.
// THE FLOAT CONTRACT is ingest_tensor.h's, word for word (tensor_num.h's tensor_affine: two binary32 operations, not fused).
#pragma once

#include "ingest_tensor.h"

namespace dsv2 {

template <int DT> struct HwcInRaw { // a thread's twelve elements of one row as loaded: 6 dwords (pairs, lo first) or 12
    static constexpr int N = DT == kTensorF32 ? 12 : 6;
    uint32_t d[N];
};

// the twelve elements of pixels x .. x + 3 (x a multiple of 4) of a row
template <bool WIDE, int DT> __host__ __device__ __forceinline__ HwcInRaw<DT> hwc_in_load(const uint8_t *row, int x, int w)
{
    HwcInRaw<DT> q;
    if constexpr (WIDE && DT == kTensorF32) {
        // 48 bytes at 12 * x, a multiple of 48, and x + 4 <= w; three vectors off ONE address, so that the compiler sees them consecutive
        const DSV2_GLOBAL u32x4 *p = (const DSV2_GLOBAL u32x4 *) (row + 12 * (uint32_t) x);
        const u32x4 a = p[0], b = p[1], c = p[2];
        q.d[0] = a[0], q.d[1] = a[1], q.d[2] = a[2], q.d[3] = a[3];
        q.d[4] = b[0], q.d[5] = b[1], q.d[6] = b[2], q.d[7] = b[3];
        q.d[8] = c[0], q.d[9] = c[1], q.d[10] = c[2], q.d[11] = c[3];
    } else if constexpr (WIDE) {
        const DSV2_GLOBAL u32x2 *p = (const DSV2_GLOBAL u32x2 *) (row + 6 * (uint32_t) x); // 24 bytes at 6 * x, a multiple of 24
        const u32x2 a = p[0], b = p[1], c = p[2];
        q.d[0] = a[0], q.d[1] = a[1], q.d[2] = b[0], q.d[3] = b[1], q.d[4] = c[0], q.d[5] = c[1];
    } else {
        uint32_t e[12];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t xc = (uint32_t) (x + i < w ? x + i : w - 1); // (pixels right of the picture: its last pixel again)
#pragma unroll
            for (int k = 0; k < 3; k++) {
#if defined(INGEST_HWC_CHECK_BREAK_LOAD) // (tools/ingest_hwc_check.cpp's deliberate break: one element past the row; never set in a build)
                const uint32_t at = 3 * xc + (uint32_t) k + 1;
#else
                const uint32_t at = 3 * xc + (uint32_t) k;
#endif
                if constexpr (DT == kTensorF32) {
                    e[3 * i + k] = ld_global<uint32_t>(row, 4 * at);
                } else {
                    e[3 * i + k] = ld_global<uint16_t>(row, 2 * at);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < HwcInRaw<DT>::N; m++) {
            q.d[m] = DT == kTensorF32 ? e[m] : e[2 * m] | (e[2 * m + 1] << 16);
        }
    }
    return q;
}

// a row's twelve elements as loaded into its four pixel dwords: element k of pixel i in byte k, byte 3 zero
template <int DT> __host__ __device__ __forceinline__ void hwc_in_pixels(const HwcInJob &j, const HwcInRaw<DT> &raw, uint32_t (&px)[4])
{
    float e[12];
    if constexpr (DT == kTensorF32) {
#pragma unroll
        for (int i = 0; i < 12; i++) {
            e[i] = tensor_f32_of(raw.d[i]);
        }
    } else if constexpr (DT == kTensorF16) {
#pragma unroll
        for (int m = 0; m < 6; m++) {
            const tensor_f32x2 a = tensor_f16_widen(raw.d[m]);
            e[2 * m] = a[0], e[2 * m + 1] = a[1];
        }
    } else {
#pragma unroll
        for (int m = 0; m < 6; m++) {
            e[2 * m] = tensor_bf16_widen(raw.d[m]), e[2 * m + 1] = tensor_f32_of(raw.d[m] & 0xffff0000u);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        px[i] = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
#if defined(INGEST_HWC_CHECK_BREAK_SCALE) // (the check program's other deliberate break: the constants by CHANNEL under B G R; never set in a build)
            const int at = (j.csc.ycoef & 0xffu) < ((j.csc.ycoef >> 16) & 0xffu) ? 2 - k : k; // (blue weighs least in luma: blue first)
#else
            const int at = k;
#endif
            px[i] = tensor_in_pack(px[i], k, e[3 * i + k], j.scale[at], j.bias[at]);
        }
    }
}

// rows y0 .. y0 + 3 (y0 a multiple of 4, below h) of job j, pixels x_first .. x_first + 3 (a multiple of 4) and on in steps of x_step,
// for element type DT and a stream with chroma shifts HS, VS
template <bool WIDE, int DT, int HS, int VS>
__host__ __device__ __forceinline__ void ingest_hwc_rows_fmt(const HwcInJob &j, int y0, int x_first, int x_step)
{
    constexpr int ROWS = !WIDE ? 1 : DT == kTensorF32 ? 2 : 4; // rows whose loads are in flight together
    const int w = j.w, h = j.h;
    // what rgb_emit reads of a job: destination, geometry, coefficients
    const RgbJob o{nullptr, 0, {j.dst[0], j.dst[1], j.dst[2]}, j.ystride, j.cstride, w, h, j.hs, j.vs, j.csc};
    for (int xi = x_first; xi < w; xi += x_step) {
        const int x = lane_offset(xi);
        uint32_t px[4][4];
#pragma unroll
        for (int r0 = 0; r0 < 4; r0 += ROWS) {
            HwcInRaw<DT> raw[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int y = y0 + r0 + r < h ? y0 + r0 + r : h - 1; // (rows below the picture: read again from its last row, never stored)
                raw[r] = hwc_in_load<WIDE, DT>(j.src + (size_t) row_number(y) * j.pitch, x, w);
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                hwc_in_pixels<DT>(j, raw[r], px[r0 + r]);
            }
#if defined(__HIP_DEVICE_COMPILE__)
            if constexpr (ROWS < 4) {
                __builtin_amdgcn_sched_barrier(0); // (the next group's loads stay behind this group's conversion)
            }
#endif
        }
        rgb_emit<HS, VS, WIDE>(o, px, x, y0);
    }
}

// The stream's format is one value for the whole launch, so the switch stands outside the row loop (ingest_rgb.h) ...
template <bool WIDE, int DT> __host__ __device__ __forceinline__ void ingest_hwc_rows_dt(const HwcInJob &j, int y0, int x_first, int x_step)
{
    switch (4 * j.hs + j.vs) {
    case 0x0:
        ingest_hwc_rows_fmt<WIDE, DT, 0, 0>(j, y0, x_first, x_step);
        break;
    case 0x4:
        ingest_hwc_rows_fmt<WIDE, DT, 1, 0>(j, y0, x_first, x_step);
        break;
    case 0x5:
        ingest_hwc_rows_fmt<WIDE, DT, 1, 1>(j, y0, x_first, x_step);
        break;
    case 0x8:
        ingest_hwc_rows_fmt<WIDE, DT, 2, 0>(j, y0, x_first, x_step);
        break;
    default: // 0xA, "4:1:0" (the host lets no other format through)
        ingest_hwc_rows_fmt<WIDE, DT, 2, 2>(j, y0, x_first, x_step);
        break;
    }
}

// ... and so does the one on the job's element type, one value for the whole workgroup.
template <bool WIDE> __host__ __device__ __forceinline__ void ingest_hwc_rows(const HwcInJob &j, int y0, int x_first, int x_step)
{
    switch (j.dtype) {
    case kTensorF16:
        ingest_hwc_rows_dt<WIDE, kTensorF16>(j, y0, x_first, x_step);
        break;
    case kTensorBF16:
        ingest_hwc_rows_dt<WIDE, kTensorBF16>(j, y0, x_first, x_step);
        break;
    default: // kTensorF32 (the host lets no other element type through: a uint8 one is a three-byte surface's Rgb3Job)
        ingest_hwc_rows_dt<WIDE, kTensorF32>(j, y0, x_first, x_step);
        break;
    }
}

} // namespace dsv2
