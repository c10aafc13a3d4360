// ingest_resize.h -- ingest at any larger size (dsv2hip_enc_batch_surface_sized): what one thread of k_ingest_sized and
// k_ingest_rgb_sized (ingest.hip) does, as functions that also compile for the host (the pattern of ingest_scale.h and
// egress_resize.h), and the device-free rule that says which source an encoder takes (ingest_resize::plan_sized_source,
// sized_surface_fits).  tools/ingest_resize_check.cpp sweeps the very same code on the CPU under AddressSanitizer -- ratios, forms,
// layouts, pitches and offsets -- before it runs on a GPU.
//
// The contract is include/dsv2_hip.h's.  A source plane of pw x ph becomes the encoder's plane of ow x oh by the exact area average
// of egress_resize.h: pw / ow = a / b and ph / oh = c / d in lowest terms, D = a * c,
//   YUV: out(x, y) = (SUM j SUM i  wy(y,j) * wx(x,i) * P(i, j)  +  D / 2) / D        each source plane on its own
//   RGB: S_ch = SUM SUM wy * wx * ch(i, j) for the three colour bytes of the packed picture, src_w x src_h -> W x H for luma and
//        -> cw x ch for chroma, then the matrix ONCE on the sums:
//          Y' = (yr*S_R + yg*S_G + yb*S_B + (128 + 256*ybase) * D) / (256 * D)
//          U' = min(255, (ur*S_R + ug*S_G + ub*S_B + 32896 * Dc) / (256 * Dc)),  V' likewise
// No coordinate outside the plane exists in the formula, and none is read.
//
// SHAPE.  A thread owns four consecutive samples of ONE output row and stores one dword; 64 x 4 threads a workgroup, the grid covers
// rows, jobs and 256-sample groups -- no loop over a row or over rows.
//   YUV (ingest_sized_quad): ONE body for the three kinds of source, parametrised on the byte step between samples and the byte
//        offset of the first: 1 / 0 a planar plane, 2 / 0 and 2 / 1 the U and the V of an interleaved plane.  The horizontal sum of
//        a sample over one source row is a DIFFERENCE OF TWO PREFIX SUMS: with F(t) = b * SUM i<q P(i) + r * P(q), q = t / b,
//        r = t % b, SUM i wx(x,i) P(i) = F((x+1)*a) - F(x*a).  The thread's four samples share five boundaries, so it walks the
//        dwords of its span of the row ONCE -- at most 4*a/b + 2 samples: 8 bytes at 3 : 2, 34 at 8 : 1 -- sums each dword's samples
//        with one v_dot4_u32_u8 against the kind's pattern of ones, and takes F at a boundary from the running sum, one masked dot
//        product and one byte of the dword it falls into.  Masks, shifts and remainders of the five boundaries depend on x alone and
//        are worked out once, before the rows.  One load per 4 source bytes, where k_egress_resize issues one per tap.
//        A boundary with r = 0 (k >= 1) is taken at the sample before it with the whole weight b, so the last boundary of a row,
//        t = pw * b, needs no sample pw.
//     wide:    every sized source plane of the step has pointer, pitch and source row bytes multiples of 4 (sized_job_wide): the span's
//              dwords are aligned loads, and a dword that holds a sample of the row lies whole inside the row.
//     general: any pointer, pitch and width: the same walk, each dword put together from byte loads of exactly the samples between
//              the thread's first and last boundary sample.
//   RGB (ingest_sized_rgb_quad): the sample step is a pixel, 4 bytes; three channel sums a tap and the matrix at the end.  Rows
//        0 .. H-1 of the grid are luma rows, rows H .. H+ch-1 chroma rows (U and V of four samples); a plain loop over the taps of a
//        sample -- up to 9 x 9 for luma, 33 x 33 for chroma at "4:1:0" and a ratio of 8.
//     wide:    pointer and pitch multiples of 4 (sized_rgb_job_wide): a pixel is one dword load.
//     general: rgb_pixel (ingest_rgb.h): the dword where this surface's rows are aligned, else the three colour bytes.
// Destinations are dframe_alloc's planes (16-byte aligned origin and stride): only ow x oh are written, as a dword where the four
// samples lie inside the row, else byte by byte; the border is k_extend's.
//
// RANGES.  xs = x * a <= pw * b <= 2^30.  F <= b * 255 * 40 < 2^29 (b <= 32768).  A row's horizontal sum <= 255 * a, the whole sum
// <= 255 * D, D <= 2^24 (YUV) -- egress_resize.h's.  RGB: D <= 65535 for both ratios, so a channel sum <= 255 * 65535, a matrix row
// times the sums <= 256 * 255 * D, with the bias <= 65536 * D < 2^32, and the divisor 256 * D < 2^24 (include/dsv2_hip.h).
#pragma once

#include "egress_resize.h" // resize_div, mulhi_u32
#include "ingest_scale.h"  // ingest_scale::plan_source, surface_fits; dot4_u8, rgb_pixel

namespace dsv2 {

// x * y for x, y below 2^24 (the low 32 bits of the product: v_mul_u32_u24, full rate where v_mul_lo_u32 is a quarter)
__host__ __device__ __forceinline__ uint32_t mul24_u32(uint32_t x, uint32_t y)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(x, y);
#else
    return (x & 0xffffffu) * (y & 0xffffffu); // (what the instruction does: an operand of 2^24 or more shows in the CPU sweep)
#endif
}

// ---- YUV: four samples of one row of one source plane ----------------------------------------------------------------------------
// dword m of a row as the walk sees it.  general: only the samples first .. last (byte offsets, (at - first) a multiple of step)
template <bool WIDE>
__host__ __device__ __forceinline__ uint32_t sized_span_dword(const uint8_t *row, uint32_t m, uint32_t first, uint32_t last, uint32_t step)
{
    if constexpr (WIDE) {
        return ld_global<uint32_t>(row, 4 * m);
    } else {
        uint32_t dw = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t at = 4 * m + i;
            if (at >= first && at <= last && ((at - first) & (step - 1)) == 0) {
                dw |= (uint32_t) ld_global<uint8_t>(row, at) << (8 * i);
            }
        }
        return dw;
    }
}

// samples x0 .. x0 + 3 (x0 a multiple of 4, below ow) of output row y (below oh) of job j
template <bool WIDE> __host__ __device__ __forceinline__ void ingest_sized_quad(const SizedSurfaceJob &j, int y, int x0)
{
    const uint32_t a = j.q.a, b = j.q.b, c = j.q.c, d = j.q.d, step = j.step, off = j.off;
    const int ow = j.ow;
    const uint32_t pattern = step == 1 ? 0x01010101u : 0x00010001u << (8 * off);
    uint32_t dwi[5], sh[5], msk[5], rem[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const uint32_t x = (uint32_t) (x0 + k < ow ? x0 + k : ow); // (boundaries behind the row: the row's end, an empty sample)
        const uint32_t xs = x * a;
        uint32_t q = resize_div(xs, b, j.q.rb), r = xs - q * b;
        if (k && r == 0) { // the whole of the sample before
            q -= 1, r = b;
        }
        const uint32_t p = off + step * q;
        dwi[k] = p >> 2, sh[k] = 8 * (p & 3), msk[k] = pattern & ((1u << sh[k]) - 1u), rem[k] = r;
    }
    const uint32_t first = 4 * dwi[0] + (sh[0] >> 3), last = 4 * dwi[4] + (sh[4] >> 3);
    const uint32_t ys = (uint32_t) y * c, ye = ys + c; // the sample row's interval, in units of 1 / d of a source row
    const uint32_t j0 = resize_div(ys, d, j.q.rd);
    const uint8_t *row = j.src + (size_t) j0 * j.pitch;
    uint32_t acc[4] = {0, 0, 0, 0};
    for (uint32_t lo_y = j0 * d; lo_y < ye; lo_y += d, row += j.pitch) { // (at most 9 rows)
        const uint32_t top = lo_y > ys ? lo_y : ys, bot = lo_y + d < ye ? lo_y + d : ye, wy = bot - top;
        // (the walk only picks: the prefix sum and the dword at each boundary; the multiplications wait until it is over, and all
        // their operands are below 2^24 -- b, rem, wy <= 32768, a prefix <= 255 * 40, a row's sum <= 255 * 32768 -- v_mul_u32_u24)
        uint32_t pre[5] = {0, 0, 0, 0, 0}, at[5] = {0, 0, 0, 0, 0}, run = 0;
        for (uint32_t m = dwi[0]; m <= dwi[4]; m++) {
            const uint32_t dw = sized_span_dword<WIDE>(row, m, first, last, step);
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const bool here = m == dwi[k];
                pre[k] = here ? dot4_u8(dw, msk[k], run) : pre[k];
                at[k] = here ? dw : at[k];
            }
            run = dot4_u8(dw, pattern, run);
        }
        uint32_t F[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            F[k] = mul24_u32(b, pre[k]) + mul24_u32(rem[k], (at[k] >> sh[k]) & 0xffu);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            acc[k] += mul24_u32(wy, F[k + 1] - F[k]);
        }
    }
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        w |= resize_div(acc[k] + (j.q.D >> 1), j.q.D, j.q.rD) << (8 * k);
    }
    uint8_t *drow = j.dst + (size_t) y * (size_t) j.dstride;
    if (x0 + 4 <= ow) {
        st_global<uint32_t>(drow, (uint32_t) x0, w); // (x0 is a multiple of 4, the plane's origin and stride of 16)
    } else {
        for (int k = 0; x0 + k < ow; k++) {
            st_global<uint8_t>(drow, (uint32_t) (x0 + k), (uint8_t) (w >> (8 * k)));
        }
    }
}

// ---- RGB: four luma samples, or four U and four V samples, of one row ------------------------------------------------------------
// the three channel sums S[byte] of sample (x, y) of the picture resampled by ratio q
template <bool WIDE>
__host__ __device__ __forceinline__ void sized_rgb_sums(const SizedRgbJob &j, const SizedRatio &q, int y, int x, bool aligned, uint32_t (&S)[3])
{
    const uint32_t a = q.a, b = q.b, c = q.c, d = q.d;
    const uint32_t ys = (uint32_t) y * c, ye = ys + c, xs = (uint32_t) x * a, xe = xs + a;
    const uint32_t j0 = resize_div(ys, d, q.rd), i0 = resize_div(xs, b, q.rb);
    const uint8_t *row = j.src + (size_t) j0 * j.pitch;
    S[0] = S[1] = S[2] = 0;
    (void) aligned;
    for (uint32_t lo_y = j0 * d; lo_y < ye; lo_y += d, row += j.pitch) {
        const uint32_t top = lo_y > ys ? lo_y : ys, bot = lo_y + d < ye ? lo_y + d : ye, wy = bot - top;
        uint32_t h0 = 0, h1 = 0, h2 = 0, i = i0;
        for (uint32_t lo = i0 * b; lo < xe; lo += b, i++) {
            const uint32_t left = lo > xs ? lo : xs, right = lo + b < xe ? lo + b : xe, wx = right - left;
            const uint32_t px = WIDE ? ld_global<uint32_t>(row, 4 * i) : rgb_pixel(row, 4 * i, aligned);
            h0 += wx * (px & 0xffu), h1 += wx * ((px >> 8) & 0xffu), h2 += wx * ((px >> 16) & 0xffu);
        }
        S[0] += wy * h0, S[1] += wy * h1, S[2] += wy * h2;
    }
}
// a coefficient quad (bytes in the surface's channel order, 0 for alpha) times the channel sums
__host__ __device__ __forceinline__ uint32_t sized_rgb_weigh(uint32_t quad, const uint32_t (&S)[3])
{
    return (quad & 0xffu) * S[0] + ((quad >> 8) & 0xffu) * S[1] + ((quad >> 16) & 0xffu) * S[2];
}
__host__ __device__ __forceinline__ void sized_store_quad(uint8_t *drow, int x0, int ow, uint32_t w)
{
    if (x0 + 4 <= ow) {
        st_global<uint32_t>(drow, (uint32_t) x0, w);
    } else {
        for (int k = 0; x0 + k < ow; k++) {
            st_global<uint8_t>(drow, (uint32_t) (x0 + k), (uint8_t) (w >> (8 * k)));
        }
    }
}

// grid row gy: below oh the luma row gy, from oh on the chroma row gy - oh (below ch); samples x0 .. x0 + 3 of it (x0 a multiple of 4,
// below ow / cw)
template <bool WIDE> __host__ __device__ __forceinline__ void ingest_sized_rgb_quad(const SizedRgbJob &j, int gy, int x0)
{
    const bool aligned = ((((uintptr_t) j.src) | j.pitch) & 3) == 0;
    uint32_t S[3];
    if (gy < j.oh) {
        uint32_t w = 0;
        for (int k = 0; k < 4 && x0 + k < j.ow; k++) {
            sized_rgb_sums<WIDE>(j, j.ql, gy, x0 + k, aligned, S);
            w |= resize_div(sized_rgb_weigh(j.csc.ycoef, S) + j.csc.yoff * j.ql.D, j.ql.D << 8, j.ql.rD) << (8 * k);
        }
        sized_store_quad(j.dst[0] + (size_t) gy * (size_t) j.ystride, x0, j.ow, w);
    } else {
        const int cy = gy - j.oh;
        uint32_t wu = 0, wv = 0;
        for (int k = 0; k < 4 && x0 + k < j.cw; k++) {
            sized_rgb_sums<WIDE>(j, j.qc, cy, x0 + k, aligned, S);
            const uint32_t bias = 32896u * j.qc.D;
            const uint32_t u = resize_div(sized_rgb_weigh(j.csc.upos, S) + bias - sized_rgb_weigh(j.csc.uneg, S), j.qc.D << 8, j.qc.rD);
            const uint32_t v = resize_div(sized_rgb_weigh(j.csc.vpos, S) + bias - sized_rgb_weigh(j.csc.vneg, S), j.qc.D << 8, j.qc.rD);
            wu |= (u < 255u ? u : 255u) << (8 * k), wv |= (v < 255u ? v : 255u) << (8 * k);
        }
        sized_store_quad(j.dst[1] + (size_t) cy * (size_t) j.cstride, x0, j.cw, wu);
        sized_store_quad(j.dst[2] + (size_t) cy * (size_t) j.cstride, x0, j.cw, wv);
    }
}

// ---- which source an encoder takes (device-free: swept on the CPU by tools/ingest_resize_check.cpp) -----------------------------
namespace ingest_resize {

constexpr uint32_t kRgbMaxD = 65535; // 256 * D < 2^24 and 65536 * D < 2^32

struct Sized {
    ingest_scale::Source src;  // kind, plain layout, the source planes; shift != 0: the scaled call's entry, nothing below is set
    bool sized = false;        // the source is resampled by the sized kernels (false: a scaled entry, or the encoder's own size)
    int nres = 0;              // resamplings: YUV 3 (Y, U, V), RGB 2 (luma, chroma)
    int pw[3] = {0, 0, 0}, ph[3] = {0, 0, 0}, ow[3] = {0, 0, 0}, oh[3] = {0, 0, 0};
};

// the ratio record of pw x ph -> ow x oh; rgb: the final divisor is 256 * D
inline SizedRatio sized_ratio(int pw, int ph, int ow, int oh, bool rgb)
{
    const int gx = resize_gcd(pw, ow), gy = resize_gcd(ph, oh);
    SizedRatio q{(uint16_t) (pw / gx), (uint16_t) (ow / gx), (uint16_t) (ph / gy), (uint16_t) (oh / gy), 0, 0, 0, 0};
    q.D = (uint32_t) q.a * (uint32_t) q.c;
    q.rD = resize_recip(rgb ? q.D << 8 : q.D), q.rb = resize_recip(q.b), q.rd = resize_recip(q.d);
    return q;
}

// the chroma of an RGB source: src_w x src_h -> cw x ch, a ratio of up to 8 << hs by 8 << vs (the luma ratio has passed resize_allowed)
inline bool rgb_chroma_allowed(int pw, int ph, int cw, int ch)
{
    if (cw <= 0 || ch <= 0 || cw > pw || ch > ph) {
        return false;
    }
    return (uint64_t) (pw / resize_gcd(pw, cw)) * (uint64_t) (ph / resize_gcd(ph, ch)) <= kRgbMaxD;
}

// An entry of dsv2hip_enc_batch_surface_sized for an encoder of enc_w x enc_h in format subsamp.  A layout with a scale value: the
// scaled call's entry (ingest_scale::plan_source, and the reduction must be the encoder's geometry).  Without one: any source with
// enc <= src <= 8 * enc per axis whose planes pass resize_allowed one by one (RGB: the luma resampling passes it, and both its
// resamplings have D <= 65535); a source of the encoder's own size is the plain ingest's business (sized = false).
inline bool plan_sized_source(int src_w, int src_h, int enc_w, int enc_h, int subsamp, int layout, Sized *out)
{
    Sized z;
    if (enc_w <= 0 || enc_h <= 0 || !ingest_scale::plan_source(src_w, src_h, subsamp, layout, &z.src)) {
        return false;
    }
    if (z.src.shift) {
        if (z.src.enc_w != enc_w || z.src.enc_h != enc_h) {
            return false;
        }
        *out = z;
        return true;
    }
    z.src.enc_w = enc_w, z.src.enc_h = enc_h;
    const int hs = DSV_FORMAT_H_SHIFT(subsamp), vs = DSV_FORMAT_V_SHIFT(subsamp);
    const int cw = (int) (((size_t) enc_w + ((size_t) 1 << hs) - 1) >> hs), ch = (int) (((size_t) enc_h + ((size_t) 1 << vs) - 1) >> vs);
    if (z.src.kind == ingest_scale::Source::RGB) {
        z.nres = 2;
        z.pw[0] = z.pw[1] = src_w, z.ph[0] = z.ph[1] = src_h;
        z.ow[0] = enc_w, z.oh[0] = enc_h, z.ow[1] = cw, z.oh[1] = ch;
        if (!resize_allowed(src_w, src_h, enc_w, enc_h) || !rgb_chroma_allowed(src_w, src_h, cw, ch) ||
            (uint64_t) (src_w / resize_gcd(src_w, enc_w)) * (uint64_t) (src_h / resize_gcd(src_h, enc_h)) > kRgbMaxD) {
            return false;
        }
    } else {
        z.nres = 3;
        const int scw = (int) (((size_t) src_w + ((size_t) 1 << hs) - 1) >> hs), sch = (int) (((size_t) src_h + ((size_t) 1 << vs) - 1) >> vs);
        for (int p = 0; p < 3; p++) {
            z.pw[p] = p ? scw : src_w, z.ph[p] = p ? sch : src_h, z.ow[p] = p ? cw : enc_w, z.oh[p] = p ? ch : enc_h;
            if (!resize_allowed(z.pw[p], z.ph[p], z.ow[p], z.oh[p])) {
                return false;
            }
        }
    }
    z.sized = src_w != enc_w || src_h != enc_h;
    *out = z;
    return true;
}

// every plane the layout has is there with a pitch of at least its SOURCE row's bytes (a scaled entry: surface_fits, the same)
inline bool sized_surface_fits(const Sized &z, const dsv2hip_surface &sf)
{
    return ingest_scale::surface_fits(z.src, sf, z.src.enc_w, z.src.enc_h);
}

} // namespace ingest_resize
} // namespace dsv2
