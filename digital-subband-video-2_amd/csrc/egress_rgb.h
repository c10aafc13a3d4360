// egress_rgb.h -- what one thread of k_egress_rgb (egress.hip) does, as a function that also compiles for the host (the pattern of
// egress_uv.h and ingest_rgb.h): the kernel is this function behind blockIdx / threadIdx, and tools/egress_rgb_check.cpp sweeps the
// very same code on the CPU under AddressSanitizer -- layouts, forms, element types, orders, presets, formats, widths, pitches, offsets
// and constants -- before it runs on a GPU.
//
// One RgbOutJob (io_jobs.h) = one decoded picture on its way out as RGB, converted on the way by the integer formulas of
// include/dsv2_hip.h (the contract; restated at rgb_terms below) into one of three layouts: a packed four-byte surface
// (dsv2hip_out_surface, BGRA / RGBA), the three planes R, G, B of a tensor (dsv2hip_out_tensor) or an interleaved [h, w, 3] tensor
// (dsv2hip_out_hwc), the tensors of uint8, binary16, bfloat16 or binary32 elements.  The mirror image of ingest_rgb.h: a thread owns
// FOUR pixels of FOUR consecutive rows -- a whole number of chroma footprints of every format, so a chroma sample is read and its three
// products formed once for all the pixels it covers; rows below h are read again from the last row and never stored; every load is
// issued before the first store.  All of that is written once (egress_rgb_rows_fmt); only the store of a row differs by layout:
//   packed       the row's four pixels as dwords, one 16-byte store (in the walk itself);
//   planar       a channel at a time, one store per plane of 4 / 8 / 8 / 16 bytes -- a wavefront writes whole 128-byte lines of a plane,
//                and no more than one row's four elements of one channel are alive as floats (rgb_emit_planar, tensor_store);
//   interleaved  the row's TWELVE consecutive elements as three vector stores of 4 / 8 / 8 / 16 bytes (rgb_emit_interleaved, hwc_store).
//   Sources: luma is one aligned dword per row (x is a multiple of 4, the plane's origin and stride of 16; the up to three bytes
//            past the row lie in the plane's border, or inside the stride of the decoder's staged luma).  What four pixels hold of
//            chroma is a dword (4:4:4), an aligned pair of bytes (4:2:2, 4:2:0: x >> 1 is even) or one byte (4:1:1, "4:1:0") per
//            chroma row -- never an unaligned word; a sample right of cw is border, and belongs to pixels that are not stored.
//   WIDE:    rgb_out_job_wide of every job of the launch (the host picks it per round): unconditional vector stores.
//   general: any w, pitch and alignment (tensors: element aligned).  A pixel is stored only where x < w -- packed: as one dword where
//            its address is a multiple of 4, else as its four bytes; tensors: the wide form's vectors where the row's address is
//            aligned for them and all four pixels lie inside the row, else element by element -- no byte outside the h rows of the
//            picture is ever written.
// The byte order is data: the job says which of R and B is byte (element) 0, and the two outer bytes' coefficient pairs are picked from
// it once, in scalar registers; every byte of a pixel is then the same multiply-add chain, and packed alpha is the constant 255.  The
// element type is data of the job, one value for the whole workgroup: the switch on it stands outside the loops, around the switch on
// the stream's format.
// THE FLOAT CONTRACT (include/dsv2_hip.h): f = fl32(fl32((float) byte * scale) + bias), two IEEE binary32 operations, NOT fused --
// tensor_affine switches contraction off by pragma, without which hipcc makes one v_fma_f32 (v_fma_mixlo_f16 in front of a half
// store) of the pair.  binary16: round to nearest even, subnormals kept, overflow to infinity (the hardware's / the host's conversion);
// bfloat16: (bits + 0x7fff + ((bits >> 16) & 1)) >> 16, in integers on both sides (f is never a NaN: the constants are finite).
#pragma once

#include "ingest_rgb.h" // ld_global, st_global, u32x4, lane_offset
#include "tensor_num.h" // tensor_affine, the element bits, u32x2, row_number

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
// bgra: byte 0 is B, else R (planar passes 0: the planes are R, G, B)
__host__ __device__ __forceinline__ RgbTerms rgb_terms(const RgbOutCoefs &csc, int bgra)
{
    RgbTerms t;
    t.ky = csc.ky;
    t.cu[0] = bgra ? csc.bu : 0, t.cv[0] = bgra ? 0 : csc.rv; // byte 0: B or R
    t.cu[1] = csc.gu, t.cv[1] = csc.gv;
    t.cu[2] = bgra ? 0 : csc.bu, t.cv[2] = bgra ? csc.rv : 0; // byte 2: R or B
    for (int k = 0; k < 3; k++) {
        t.off[k] = 128 - csc.ky * csc.ybase - 128 * (t.cu[k] + t.cv[k]);
    }
    return t;
}

// ---- the tensors' row stores: row y of the thread's four pixels at x (a multiple of 4), w the picture's -- ly: their luma bytes, c[s][b]:
// what chroma sample s adds to element b of its pixels.  (The packed surface's store stands in the walk itself: as a function of its own,
// its general form took 28 to 37 VGPRs in every form tried, against 27 there) ----------------------------------------------

// one channel's four samples of a row -- s[i]: the clamped 16-bit sums, whose byte 1 is the sample -- into row `drow` of its plane at
// pixel x (a multiple of 4)
template <bool WIDE, int DT>
__host__ __device__ __forceinline__ void tensor_store(uint8_t *drow, int x, int w, const uint32_t (&s)[4], float scale, float bias)
{
    constexpr uint32_t ELEM = DT == kTensorU8 ? 1 : DT == kTensorF32 ? 4 : 2;
    const uint32_t at = ELEM * (uint32_t) x;
    const bool whole = WIDE || ((((uintptr_t) drow) & (4 * ELEM - 1)) == 0 && x + 4 <= w);
    if constexpr (DT == kTensorU8) {
        // byte 1 of each sum: picked by the v_perm_b32 that packs them (rgb_sum16: no shift, clamp and pack)
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

// planar: a channel of the row at a time, converted, packed and stored before the next -- not all twelve sums first, which keeps fewer
// floats alive.  (row_number, tensor_num.h: the twelve destination rows of a pass are addressed where they are stored; the first build of
// this path kept them in 24 scalar registers across the loop next to the job's and spilled them)
template <bool WIDE, int DT, int HS>
__host__ __device__ __forceinline__ void rgb_emit_planar(const RgbOutJob &j, int ky, uint32_t ly, const int (&c)[4 >> HS][3], int y, int x, int w)
{
#pragma unroll
    for (int b = 0; b < 3; b++) {
        uint32_t s[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s[i] = rgb_sum16(mad24(ky, (int) ((ly >> (8 * i)) & 0xffu), c[i >> HS][b]));
        }
        tensor_store<WIDE, DT>(j.dst[b] + (size_t) row_number(y) * (size_t) j.dpitch[b], x, w, s, j.scale[b], j.bias[b]);
    }
}

// bytes 1 of four clamped 16-bit sums into one dword, a's in byte 0 (rgb_sum16: no shift, clamp and pack)
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

// interleaved: the row's twelve sums in memory order, then hwc_store
template <bool WIDE, int DT, int HS>
__host__ __device__ __forceinline__ void rgb_emit_interleaved(const RgbOutJob &j, int ky, uint32_t ly, const int (&c)[4 >> HS][3], int y, int x, int w)
{
    uint32_t s[12];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int yv = (int) ((ly >> (8 * i)) & 0xffu);
#pragma unroll
        for (int b = 0; b < 3; b++) {
            s[3 * i + b] = rgb_sum16(mad24(ky, yv, c[i >> HS][b]));
        }
    }
    hwc_store<WIDE, DT>(j.dst[0] + (size_t) row_number(y) * (size_t) j.dpitch[0], x, w, s, j.scale, j.bias);
}

// ---- the walk, written once ---------------------------------------------------------------------------------------------------------
// rows y0 .. y0 + 3 (y0 a multiple of 4, below h) of job j, pixels x_first .. x_first + 3 (a multiple of 4) and on in steps of x_step,
// for layout LAYOUT, element type DT and a stream with chroma shifts HS, VS
template <int LAYOUT, bool WIDE, int DT, int HS, int VS>
__host__ __device__ __forceinline__ void egress_rgb_rows_fmt(const RgbOutJob &j, int y0, int x_first, int x_step)
{
    constexpr int NX = 4 >> HS, NY = 4 >> VS; // chroma samples per row, chroma rows of the thread's 4 x 4 pixels
    const int w = j.w, h = j.h;
    const RgbTerms t = rgb_terms(j.csc, LAYOUT == kRgbOutPlanar ? 0 : j.bgra);
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
            size_t off;
            if constexpr (LAYOUT == kRgbOutPacked) {
                off = (size_t) (y >> VS) * (size_t) j.cstride;
            } else {
                off = (size_t) row_number(y >> VS) * (size_t) j.cstride;
            }
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
            int c[NX][3]; // what the chroma sample adds to each byte (element) of its pixels
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
                if constexpr (LAYOUT == kRgbOutPlanar) {
                    rgb_emit_planar<WIDE, DT, HS>(j, t.ky, ly[r], c, y0 + r, x, w);
                } else if constexpr (LAYOUT == kRgbOutInterleaved) {
                    rgb_emit_interleaved<WIDE, DT, HS>(j, t.ky, ly[r], c, y0 + r, x, w);
                } else { // packed: four pixel dwords, then one 16-byte store (general: per pixel, a dword or its four bytes)
                    uint32_t o[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int yv = (int) ((ly[r] >> (8 * i)) & 0xffu);
                        const int *cs = c[i >> HS];
                        const uint32_t b0 = rgb_sum16(mad24(t.ky, yv, cs[0])), b1 = rgb_sum16(mad24(t.ky, yv, cs[1])), b2 = rgb_sum16(mad24(t.ky, yv, cs[2]));
                        // byte 1 of each clamped sum: b0 and b1 into bytes 0 and 1, then b2 into byte 2 (its byte 3 is zero)
                        o[i] = perm_b32(b2, perm_b32(b1, b0, 0x00000501u), 0x07050100u) | 0xff000000u;
                    }
                    uint8_t *drow = j.dst[0] + (size_t) (y0 + r) * (size_t) j.dpitch[0];
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
}

// The stream's format is one value for the whole launch, so the switch stands outside the row loop (ingest_rgb.h) ...
template <int LAYOUT, bool WIDE, int DT> __host__ __device__ __forceinline__ void egress_rgb_rows_dt(const RgbOutJob &j, int y0, int x_first, int x_step)
{
    switch (4 * j.hs + j.vs) {
    case 0x0:
        egress_rgb_rows_fmt<LAYOUT, WIDE, DT, 0, 0>(j, y0, x_first, x_step);
        break;
    case 0x4:
        egress_rgb_rows_fmt<LAYOUT, WIDE, DT, 1, 0>(j, y0, x_first, x_step);
        break;
    case 0x5:
        egress_rgb_rows_fmt<LAYOUT, WIDE, DT, 1, 1>(j, y0, x_first, x_step);
        break;
    case 0x8:
        egress_rgb_rows_fmt<LAYOUT, WIDE, DT, 2, 0>(j, y0, x_first, x_step);
        break;
    default: // 0xA, "4:1:0" (the host lets no other format through)
        egress_rgb_rows_fmt<LAYOUT, WIDE, DT, 2, 2>(j, y0, x_first, x_step);
        break;
    }
}

// ... and so does the one on a tensor's element type, one value for the whole workgroup (a packed surface holds bytes).
template <int LAYOUT, bool WIDE> __host__ __device__ __forceinline__ void egress_rgb_rows(const RgbOutJob &j, int y0, int x_first, int x_step)
{
    if constexpr (LAYOUT == kRgbOutPacked) {
        egress_rgb_rows_dt<LAYOUT, WIDE, kTensorU8>(j, y0, x_first, x_step);
    } else {
        switch (j.dtype) {
        case kTensorU8:
            egress_rgb_rows_dt<LAYOUT, WIDE, kTensorU8>(j, y0, x_first, x_step);
            break;
        case kTensorF16:
            egress_rgb_rows_dt<LAYOUT, WIDE, kTensorF16>(j, y0, x_first, x_step);
            break;
        case kTensorBF16:
            egress_rgb_rows_dt<LAYOUT, WIDE, kTensorBF16>(j, y0, x_first, x_step);
            break;
        default: // kTensorF32 (the host lets no other element type through)
            egress_rgb_rows_dt<LAYOUT, WIDE, kTensorF32>(j, y0, x_first, x_step);
            break;
        }
    }
}

} // namespace dsv2
