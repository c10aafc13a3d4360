// ingest_tensor.h -- what one thread of k_ingest_tensor (ingest.hip) does, as a function that also compiles for the host (the pattern of
// ingest_rgb3.h): the kernel is this function behind blockIdx / threadIdx, and tools/ingest_tensor_check.cpp sweeps the very same code
// on the CPU under AddressSanitizer -- forms, element types, presets, formats, widths, pitches, offsets and constants -- before it runs
// on a GPU.
//
// One TensorInJob (io_jobs.h) = one picture that is the three planes R, G, B of a caller's float tensor (dsv2hip_in_tensor: binary16,
// bfloat16 or binary32 elements) on its way into the three bordered source planes.  The decomposition is k_ingest_rgb3's: a thread
// owns FOUR pixels of FOUR consecutive rows, rows below h and pixels right of w are read again from the last row / pixel and never
// stored.  Only the fetch is new -- load, widen, scale and bias, clamp, round, pack: once the thread holds its px[4][4] pixel dwords
// with R, G, B in bytes 0..2, luma, chroma and the stores are ingest_rgb.h's rgb_emit, text and all, under the planar kind's
// coefficient quads.
//   WIDE:    every plane pointer and pitch a multiple of four elements and w a multiple of 4 in every job of the launch (the host picks
//            it per step, tensor_in_job_wide): a row of a plane is ONE load, 8 bytes (binary16, bfloat16) or 16 bytes (binary32), so a
//            wavefront reads 512 B / 1 KiB of consecutive bytes per row and plane, whole 128-byte lines.
//   general: any element-aligned pointer and pitch, any w: element by element, coordinates clamped to w - 1 / h - 1.
// Loads in flight: the half types issue all twelve of a pass (four rows of three planes, 24 registers of raw data) before the first
// conversion, as every ingest here does; binary32 would hold 48 registers of raw data that way and takes its rows TWO at a time
// (24 registers), the first pair converted to its eight pixel dwords before the second pair is asked for.
// The element type is data of the job, one value for the whole workgroup: the switch on it stands outside the loops, around the
// switch on the stream's format (egress_rgb.h).
// THE FLOAT CONTRACT (include/dsv2_hip.h): g = fl32(fl32(e * scale) + bias), two IEEE binary32 operations, NOT fused (tensor_num.h's
// tensor_affine, shared with the decoder's side); the byte is 0 for a NaN, else rint(min(max(g, 0), 255)) with ties to even.  The clamp
// stands BEFORE the conversion to an integer, which is undefined outside the integer's range on the host and need not saturate alike
// on both sides; a NaN fails the first comparison and leaves as +0, and so does -0.  Widening is exact: bfloat16 is bits << 16,
// binary16 the hardware's / the host's conversion, subnormals with their value.
#pragma once

#include "ingest_rgb.h"
#include "tensor_num.h"

namespace dsv2 {

// element e (widened) of plane c under its constants, as a byte in byte c of pixel dword px (which holds 0 there)
__host__ __device__ __forceinline__ uint32_t tensor_in_pack(uint32_t px, int c, float e, float scale, float bias)
{
    const float g = tensor_affine(e, scale, bias);
    const float lo = g > 0.0f ? g : 0.0f;                          // (false for a NaN and for -0)
    const float v = __builtin_rintf(lo < 255.0f ? lo : 255.0f); // an integer 0 .. 255: v_rndne_f32
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_cvt_pk_u8_f32(v, (uint32_t) c, px); // convert and place in one instruction (exact: v is an integer in range)
#else
    return px | ((uint32_t) (int) v << (8 * c));
#endif
}

template <int DT> struct TensorInRaw { // a thread's four elements of one row of one plane as loaded: 2 dwords (pairs, lo first) or 4
    static constexpr int N = DT == kTensorF32 ? 4 : 2;
    uint32_t d[N];
};

// the four elements at pixels x .. x + 3 (x a multiple of 4) of a plane's row
template <bool WIDE, int DT> __host__ __device__ __forceinline__ TensorInRaw<DT> tensor_in_load(const uint8_t *row, int x, int w)
{
    TensorInRaw<DT> q;
    if constexpr (WIDE && DT == kTensorF32) {
        const u32x4 v = ld_global<u32x4>(row, 4 * (uint32_t) x);
        q.d[0] = v[0], q.d[1] = v[1], q.d[2] = v[2], q.d[3] = v[3];
    } else if constexpr (WIDE) {
        const u32x2 v = ld_global<u32x2>(row, 2 * (uint32_t) x);
        q.d[0] = v[0], q.d[1] = v[1];
    } else {
        uint32_t e[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t xc = (uint32_t) (x + i < w ? x + i : w - 1); // (pixels right of the picture: its last pixel again)
            if constexpr (DT == kTensorF32) {
                e[i] = ld_global<uint32_t>(row, 4 * xc);
            } else {
                e[i] = ld_global<uint16_t>(row, 2 * xc);
            }
        }
        if constexpr (DT == kTensorF32) {
            q.d[0] = e[0], q.d[1] = e[1], q.d[2] = e[2], q.d[3] = e[3];
        } else {
            q.d[0] = e[0] | (e[1] << 16), q.d[1] = e[2] | (e[3] << 16);
        }
    }
    return q;
}

// a row's three planes as loaded into its four pixel dwords: R, G, B in bytes 0..2, byte 3 zero
template <int DT> __host__ __device__ __forceinline__ void tensor_in_pixels(const TensorInJob &j, const TensorInRaw<DT> (&raw)[3], uint32_t (&px)[4])
{
    px[0] = px[1] = px[2] = px[3] = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float e[4];
        if constexpr (DT == kTensorF32) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                e[i] = tensor_f32_of(raw[c].d[i]);
            }
        } else if constexpr (DT == kTensorF16) {
            const tensor_f32x2 a = tensor_f16_widen(raw[c].d[0]), b = tensor_f16_widen(raw[c].d[1]);
            e[0] = a[0], e[1] = a[1], e[2] = b[0], e[3] = b[1];
        } else {
            e[0] = tensor_bf16_widen(raw[c].d[0]), e[1] = tensor_f32_of(raw[c].d[0] & 0xffff0000u);
            e[2] = tensor_bf16_widen(raw[c].d[1]), e[3] = tensor_f32_of(raw[c].d[1] & 0xffff0000u);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            px[i] = tensor_in_pack(px[i], c, e[i], j.scale[c], j.bias[c]);
        }
    }
}

// rows y0 .. y0 + 3 (y0 a multiple of 4, below h) of job j, pixels x_first .. x_first + 3 (a multiple of 4) and on in steps of x_step,
// for element type DT and a stream with chroma shifts HS, VS
template <bool WIDE, int DT, int HS, int VS>
__host__ __device__ __forceinline__ void ingest_tensor_rows_fmt(const TensorInJob &j, int y0, int x_first, int x_step)
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
            TensorInRaw<DT> raw[ROWS][3];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int y = y0 + r0 + r < h ? y0 + r0 + r : h - 1; // (rows below the picture: read again from its last row, never stored)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    raw[r][c] = tensor_in_load<WIDE, DT>(j.src[c] + (size_t) row_number(y) * j.pitch[c], x, w);
                }
            }
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                tensor_in_pixels<DT>(j, raw[r], px[r0 + r]);
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
template <bool WIDE, int DT> __host__ __device__ __forceinline__ void ingest_tensor_rows_dt(const TensorInJob &j, int y0, int x_first, int x_step)
{
    switch (4 * j.hs + j.vs) {
    case 0x0:
        ingest_tensor_rows_fmt<WIDE, DT, 0, 0>(j, y0, x_first, x_step);
        break;
    case 0x4:
        ingest_tensor_rows_fmt<WIDE, DT, 1, 0>(j, y0, x_first, x_step);
        break;
    case 0x5:
        ingest_tensor_rows_fmt<WIDE, DT, 1, 1>(j, y0, x_first, x_step);
        break;
    case 0x8:
        ingest_tensor_rows_fmt<WIDE, DT, 2, 0>(j, y0, x_first, x_step);
        break;
    default: // 0xA, "4:1:0" (the host lets no other format through)
        ingest_tensor_rows_fmt<WIDE, DT, 2, 2>(j, y0, x_first, x_step);
        break;
    }
}

// ... and so does the one on the job's element type, one value for the whole workgroup.
template <bool WIDE> __host__ __device__ __forceinline__ void ingest_tensor_rows(const TensorInJob &j, int y0, int x_first, int x_step)
{
    switch (j.dtype) {
    case kTensorF16:
        ingest_tensor_rows_dt<WIDE, kTensorF16>(j, y0, x_first, x_step);
        break;
    case kTensorBF16:
        ingest_tensor_rows_dt<WIDE, kTensorBF16>(j, y0, x_first, x_step);
        break;
    default: // kTensorF32 (the host lets no other element type through: a uint8 tensor is a planar RGB surface's Rgb3Job)
        ingest_tensor_rows_dt<WIDE, kTensorF32>(j, y0, x_first, x_step);
        break;
    }
}

} // namespace dsv2
