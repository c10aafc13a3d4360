// egress_tensor.h -- what one thread of k_egress_tensor (egress.hip) does, as a function that also compiles for the host (the pattern of
// egress_rgb.h): the kernel is this function behind blockIdx / threadIdx, and tools/egress_tensor_check.cpp sweeps the very same code
// on the CPU under AddressSanitizer -- forms, element types, presets, formats, widths, pitches and offsets -- before it runs on a GPU.
//
// One TensorOutJob (io_jobs.h) = one decoded picture on its way into the three planes R, G, B of a caller's tensor (dsv2hip_out_tensor),
// converted on the way by the integer formulas of include/dsv2_hip.h (egress_rgb.h's rgb_terms, mad24 and rgb_sum16 with the byte
// order fixed to R, G, B) and, for a float element type, taken through the job's per-plane scale and bias.  k_egress_rgb's shape: a
// thread owns FOUR pixels of FOUR consecutive rows -- a whole number of chroma footprints of every format; rows below h are read again
// from the last row and never stored; every load is issued before the first store.  What is new: a row of a channel leaves as ONE
// store per plane -- a dword (uint8), 8 bytes (binary16, bfloat16) or 16 bytes (binary32) -- so a wavefront writes 256 B / 512 B /
// 1 KiB of consecutive bytes per row and plane, whole 128-byte lines; rows are converted and stored one by one, so no more than one
// row's four elements of one channel are alive as floats.
//   WIDE:    every plane pointer and pitch a multiple of four elements and w a multiple of 4 in every job of the launch (the host
//            picks it per round, tensor_job_wide): unconditional vector stores.
//   general: any element-aligned pointer and pitch, any w.  A sample is stored only where x < w: the four as one vector where the
//            row's address is aligned for it and all four lie inside the row, else element by element -- no byte outside the h row
//            pieces of w elements is ever written.
// The element type is data of the job, one value for the whole workgroup: the switch on it stands outside the loops, around the
// switch on the stream's format.
// THE FLOAT CONTRACT (include/dsv2_hip.h): f = fl32(fl32((float) byte * scale) + bias), two IEEE binary32 operations, NOT fused --
// tensor_affine switches contraction off by pragma, without which hipcc makes one v_fma_f32 (v_fma_mixlo_f16 in front of a half
// store) of the pair.  binary16: round to nearest even, subnormals kept, overflow to infinity (the hardware's / the host's conversion);
// bfloat16: (bits + 0x7fff + ((bits >> 16) & 1)) >> 16, in integers on both sides (f is never a NaN: the constants are finite).
#pragma once

#include "egress_rgb.h"
#include "tensor_num.h"

namespace dsv2 {

// (tensor_affine, tensor_f32_bits, tensor_f16_pair, tensor_bf16_bits and u32x2: tensor_num.h, shared with ingest_tensor.h)

// (row_number: tensor_num.h -- the twelve destination rows of a pass are addressed where they are stored; the first build of this
// file kept them in 24 scalar registers across the loop next to the job's 34 and spilled them)

// the conversion's terms with byte 0 = R, byte 1 = G, byte 2 = B
__host__ __device__ __forceinline__ RgbTerms tensor_terms(const TensorOutJob &j)
{
    RgbOutJob r{};
    r.csc = j.csc, r.bgra = 0;
    return rgb_terms(r);
}

// one channel's four samples of a row -- s[i]: the clamped 16-bit sums, whose byte 1 is the sample -- into row `drow` of its plane at
// pixel x (a multiple of 4)
template <bool WIDE, int DT>
__host__ __device__ __forceinline__ void tensor_store(uint8_t *drow, int x, int w, const uint32_t (&s)[4], float scale, float bias)
{
    constexpr uint32_t ELEM = DT == kTensorU8 ? 1 : DT == kTensorF32 ? 4 : 2;
    const uint32_t at = ELEM * (uint32_t) x;
    const bool whole = WIDE || ((((uintptr_t) drow) & (4 * ELEM - 1)) == 0 && x + 4 <= w);
    if constexpr (DT == kTensorU8) {
        // byte 1 of each sum: picked by the v_perm_b32 that packs them (egress_rgb.h: no shift, clamp and pack)
        const uint32_t o = perm_b32(perm_b32(s[3], s[2], 0x00000501u), perm_b32(s[1], s[0], 0x00000501u), 0x05040100u);
        if (whole) {
            st_global<uint32_t>(drow, at, o);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (x + i < w) {
                    st_global<uint8_t>(drow, at + (uint32_t) i, (uint8_t) (o >> (8 * i)));
                }
            }
        }
    } else {
        uint32_t e[4];
        if constexpr (DT == kTensorF16) {
            float f[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                f[i] = tensor_affine((float) ((s[i] >> 8) & 0xffu), scale, bias);
            }
            const uint32_t p01 = tensor_f16_pair(f[0], f[1]), p23 = tensor_f16_pair(f[2], f[3]);
            e[0] = p01 & 0xffffu, e[1] = p01 >> 16, e[2] = p23 & 0xffffu, e[3] = p23 >> 16;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float f = tensor_affine((float) ((s[i] >> 8) & 0xffu), scale, bias);
                e[i] = DT == kTensorF32 ? tensor_f32_bits(f) : tensor_bf16_bits(f);
            }
        }
        if constexpr (DT == kTensorF32) {
            if (whole) {
                st_global<u32x4>(drow, at, u32x4{e[0], e[1], e[2], e[3]});
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (x + i < w) {
                        st_global<uint32_t>(drow, at + 4 * (uint32_t) i, e[i]);
                    }
                }
            }
        } else {
            if (whole) {
                st_global<u32x2>(drow, at, u32x2{e[0] | (e[1] << 16), e[2] | (e[3] << 16)});
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    if (x + i < w) {
                        st_global<uint16_t>(drow, at + 2 * (uint32_t) i, (uint16_t) e[i]);
                    }
                }
            }
        }
    }
}

// rows y0 .. y0 + 3 (y0 a multiple of 4, below h) of job j, pixels x_first .. x_first + 3 (a multiple of 4) and on in steps of x_step,
// for element type DT and a stream with chroma shifts HS, VS
template <bool WIDE, int DT, int HS, int VS>
__host__ __device__ __forceinline__ void egress_tensor_rows_fmt(const TensorOutJob &j, int y0, int x_first, int x_step)
{
    constexpr int NX = 4 >> HS, NY = 4 >> VS; // chroma samples per row, chroma rows of the thread's 4 x 4 pixels
    const int w = j.w, h = j.h;
    const RgbTerms t = tensor_terms(j);
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
            int c[NX][3]; // what the chroma sample adds to R, G, B of its pixels
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
#pragma unroll
                for (int b = 0; b < 3; b++) { // a channel of the row at a time: converted, packed and stored before the next
                    uint32_t s[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        s[i] = rgb_sum16(mad24(t.ky, (int) ((ly[r] >> (8 * i)) & 0xffu), c[i >> HS][b]));
                    }
                    tensor_store<WIDE, DT>(j.dst[b] + (size_t) row_number(y0 + r) * (size_t) j.dpitch[b], x, w, s, j.scale[b], j.bias[b]);
                }
            }
        }
    }
}

// The stream's format is one value for the whole launch, so the switch stands outside the row loop (egress_rgb.h) ...
template <bool WIDE, int DT> __host__ __device__ __forceinline__ void egress_tensor_rows_dt(const TensorOutJob &j, int y0, int x_first, int x_step)
{
    switch (4 * j.hs + j.vs) {
    case 0x0:
        egress_tensor_rows_fmt<WIDE, DT, 0, 0>(j, y0, x_first, x_step);
        break;
    case 0x4:
        egress_tensor_rows_fmt<WIDE, DT, 1, 0>(j, y0, x_first, x_step);
        break;
    case 0x5:
        egress_tensor_rows_fmt<WIDE, DT, 1, 1>(j, y0, x_first, x_step);
        break;
    case 0x8:
        egress_tensor_rows_fmt<WIDE, DT, 2, 0>(j, y0, x_first, x_step);
        break;
    default: // 0xA, "4:1:0" (the host lets no other format through)
        egress_tensor_rows_fmt<WIDE, DT, 2, 2>(j, y0, x_first, x_step);
        break;
    }
}

// ... and so does the one on the job's element type, one value for the whole workgroup.
template <bool WIDE> __host__ __device__ __forceinline__ void egress_tensor_rows(const TensorOutJob &j, int y0, int x_first, int x_step)
{
    switch (j.dtype) {
    case kTensorU8:
        egress_tensor_rows_dt<WIDE, kTensorU8>(j, y0, x_first, x_step);
        break;
    case kTensorF16:
        egress_tensor_rows_dt<WIDE, kTensorF16>(j, y0, x_first, x_step);
        break;
    case kTensorBF16:
        egress_tensor_rows_dt<WIDE, kTensorBF16>(j, y0, x_first, x_step);
        break;
    default: // kTensorF32 (the host lets no other element type through)
        egress_tensor_rows_dt<WIDE, kTensorF32>(j, y0, x_first, x_step);
        break;
    }
}

} // namespace dsv2
