// ingest_scale.h -- half, quarter and eighth-size ingest (dsv2hip_enc_batch_surface_scaled): what the threads of
// k_ingest_surface_scaled and k_ingest_rgb_scaled (ingest.hip) do, as functions that also compile for the host (the pattern of
// ingest_rgb.h and egress_scale.h), and the device-free rule that says which source an encoder takes (ingest_scale::plan_source, surface_fits).
// tools/ingest_scale_check.cpp sweeps the very same code on the CPU under AddressSanitizer -- shifts, forms, formats, byte orders,
// presets, widths, heights, pitches and offsets -- before it runs on a GPU.
//
// With s the shift and n = 1 << s, a source of src_w x src_h feeds an encoder of W' = ceil(src_w / n) by H' = ceil(src_h / n); the
// contract is include/dsv2_hip.h's:
//   YUV: each SOURCE plane P (pw x ph) on its own, the decoder's REDUCTION
//          out(x, y) = (SUM j<n, i<n  P(min(x*n + i, pw-1), min(y*n + j, ph-1))  +  (1 << (2*s - 1))) >> (2*s)
//        (an interleaved plane: the reduced U and V of the de-interleaved one);
//   RGB: the conversion of the plain RGB ingest with every footprint enlarged by the scale and ONE rounding per sample
//          Y'(x, y)   = (SUM n x n of (yr*R + yg*G + yb*B) + ((128 + 256*ybase) << 2s)) >> (8 + 2s)
//          U'(cx, cy) = min(255, (SUM (n << hs) x (n << vs) of (ur*R + ug*G + ub*B) + (32896 << (hs + vs + 2s))) >> (8 + hs + vs + 2s))
//        footprints from (x*n, y*n) / (cx << (hs + s), cy << (vs + s)), source coordinates clamped to src_w - 1, src_h - 1.
//
// SHAPE.  A thread does ONE chunk: 16 source bytes (the wide form: one 16-byte load per row, neighbouring lanes neighbouring
// vectors) of the n source rows of one output row, summed in the lane -- at most 8 rows, 32 registers of loads.  The passes over a
// row are workgroups of the grid, not a loop (k_egress_scale's 15 dependent passes a row were its cost); the loop
// that remains runs again only for rows wider than the grid covers.  Horizontal byte sums are v_dot4_u32_u8 against ones (YUV) or
// against the coefficient quads (RGB).
//   YUV: 16 bytes hold a whole number of footprints at every shift (planar 16 samples, interleaved 8 pairs), so no lane needs
//        another; U and V of an interleaved dword are two dot products with 0x00010001 / 0x01000100.
//   RGB: 16 bytes are 4 pixels.  A wavefront owns one row of chroma samples over 256 source pixels: 1 << vs strips of n source
//        rows, each strip one luma row.  Footprints wider than a lane's 4 pixels -- luma at an eighth (2 lanes), chroma over
//        n << hs pixels (up to 8 lanes) -- are summed across an aligned group of lanes; chroma taller than a strip accumulates in
//        the lane over the strips (up to 4 of 8 rows at "4:1:0" and an eighth).  The cross-lane step is a PHASE: the body is
//        written over WaveLanes, which on the device is the one lane with __shfl_xor for the group sum and on the host the 64
//        lanes of a wavefront in a loop, phase by phase -- so the text the check program runs is the kernel's.
//   wide:    the existing predicates on the SOURCE (YUV: pointer, pitch, source row bytes multiples of 16; RGB: pointer and pitch
//            multiples of 16, src_w of 4), chosen per step over all its scaled jobs of the kind.
//   general: any size, pitch and alignment: a dword is read where it is aligned and lies whole inside the row, else the row's
//            bytes one by one, clamped -- no word is touched that holds no byte of a source row.
// Destinations are dframe_alloc's planes (16-byte aligned origin and stride): only W' x H' / cw' x ch' are written, the border is
// k_extend's.
#pragma once

#include "ingest_rgb.h" // ld_global, st_global, u32x4, lane_offset, dot4_u8, rgb_pixel
#include "surface_layout.h"

namespace dsv2 {

typedef uint32_t u32x2_in __attribute__((ext_vector_type(2)));

// NB samples, a byte each in o[], to row[x ..]: x is a multiple of NB and the row's origin of 16, so the piece is one aligned store
// where it lies whole inside the ow samples of the row (WHOLE: it always does), else its bytes below ow
template <int NB, bool WHOLE> __host__ __device__ __forceinline__ void st_samples(uint8_t *row, int x, const uint32_t *o, int ow)
{
    if (WHOLE || x + NB <= ow) {
        if constexpr (NB == 8) {
            st_global<u32x2_in>(row, (uint32_t) x,
                                u32x2_in{o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24), o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24)});
        } else if constexpr (NB == 4) {
            st_global<uint32_t>(row, (uint32_t) x, o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24));
        } else if constexpr (NB == 2) {
            st_global<uint16_t>(row, (uint32_t) x, (uint16_t) (o[0] | (o[1] << 8)));
        } else {
            st_global<uint8_t>(row, (uint32_t) x, (uint8_t) o[0]);
        }
    } else {
        for (int i = 0; i < NB && x + i < ow; i++) {
            st_global<uint8_t>(row, (uint32_t) (x + i), (uint8_t) o[i]);
        }
    }
}

// ---- YUV: one source plane ------------------------------------------------------------------------------------------------------
// the dword at byte `off` (a multiple of 4) of a source row of sb bytes, general form: bytes behind the row are the row's last
// sample again (UV: the last pair's byte of the same kind), and are never read
template <bool UV> __host__ __device__ __forceinline__ uint32_t scaled_src_dword(const uint8_t *row, int off, int sb)
{
    if (off + 4 <= sb && (((uintptr_t) (row + off)) & 3) == 0) {
        return ld_global<uint32_t>(row, (uint32_t) off);
    }
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int at = off + i;
        if (at >= sb) {
            at = UV ? sb - 2 + (i & 1) : sb - 1;
        }
        d |= (uint32_t) ld_global<uint8_t>(row, (uint32_t) at) << (8 * i);
    }
    return d;
}

// output row oy (below ceil(ph / n)) of job j at shift S: source vectors t_first, t_first + t_step ... of its n rows
template <bool WIDE, int S, bool UV>
__host__ __device__ __forceinline__ void ingest_scaled_row_s(const ScaledSurfaceJob &j, int oy, int t_first, int t_step)
{
    constexpr int N = 1 << S;
    constexpr uint32_t kRound = 1u << (2 * S - 1);
    const int pw = j.pw, ph = j.ph, sb = UV ? 2 * pw : pw, ow = (pw + N - 1) >> S;
    const size_t drow = (size_t) oy * (size_t) j.dstride;
    for (int ti = t_first; 16 * ti < sb; ti += t_step) {
        const int t = lane_offset(ti);
        uint32_t v[N][4];
#pragma unroll
        for (int r = 0; r < N; r++) {
            const int y = oy * N + r < ph ? oy * N + r : ph - 1; // (rows below the plane: its last row again)
            const uint8_t *row = j.src + (size_t) y * j.pitch;
            if constexpr (WIDE) { // (the row's bytes are a multiple of 16: no vector is partial)
                const u32x4 q = ld_global<u32x4>(row, 16 * (uint32_t) t);
                v[r][0] = q[0], v[r][1] = q[1], v[r][2] = q[2], v[r][3] = q[3];
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    v[r][k] = scaled_src_dword<UV>(row, 16 * t + 4 * k, sb);
                }
            }
        }
        if constexpr (!UV) {
            constexpr int NOUT = 16 >> S; // 8, 4, 2 samples
            uint32_t o[NOUT];
#pragma unroll
            for (int i = 0; i < NOUT; i++) {
                uint32_t sum = kRound;
#pragma unroll
                for (int r = 0; r < N; r++) {
                    if constexpr (S == 1) {
                        sum = dot4_u8(v[r][i >> 1], (i & 1) ? 0x01010000u : 0x00000101u, sum);
                    } else if constexpr (S == 2) {
                        sum = dot4_u8(v[r][i], 0x01010101u, sum);
                    } else {
                        sum = dot4_u8(v[r][2 * i + 1], 0x01010101u, dot4_u8(v[r][2 * i], 0x01010101u, sum));
                    }
                }
                o[i] = sum >> (2 * S);
            }
            st_samples<NOUT, WIDE>(j.dst + drow, t * NOUT, o, ow);
        } else {
            constexpr int NOUT = 8 >> S, DPO = 4 / NOUT; // 4, 2, 1 samples of each kind; dwords (two pairs each) per sample
            uint32_t ou[NOUT], ov[NOUT];
#pragma unroll
            for (int i = 0; i < NOUT; i++) {
                uint32_t su = kRound, sv = kRound;
#pragma unroll
                for (int r = 0; r < N; r++) {
#pragma unroll
                    for (int m = 0; m < DPO; m++) {
                        su = dot4_u8(v[r][i * DPO + m], 0x00010001u, su);
                        sv = dot4_u8(v[r][i * DPO + m], 0x01000100u, sv);
                    }
                }
                ou[i] = su >> (2 * S), ov[i] = sv >> (2 * S);
            }
            st_samples<NOUT, WIDE>(j.dst + drow, t * NOUT, ou, ow);
            st_samples<NOUT, WIDE>(j.dst2 + drow, t * NOUT, ov, ow);
        }
    }
}

// The shift and the plane's kind are one value for the whole job, so the switch stands outside the row loop (egress_scale.h).
template <bool WIDE> __host__ __device__ __forceinline__ void ingest_scaled_row(const ScaledSurfaceJob &j, int oy, int t_first, int t_step)
{
    const bool uv = j.dst2 != nullptr;
    switch (2 * j.shift + (uv ? 1 : 0)) {
    case 2:
        ingest_scaled_row_s<WIDE, 1, false>(j, oy, t_first, t_step);
        break;
    case 3:
        ingest_scaled_row_s<WIDE, 1, true>(j, oy, t_first, t_step);
        break;
    case 4:
        ingest_scaled_row_s<WIDE, 2, false>(j, oy, t_first, t_step);
        break;
    case 5:
        ingest_scaled_row_s<WIDE, 2, true>(j, oy, t_first, t_step);
        break;
    case 6:
        ingest_scaled_row_s<WIDE, 3, false>(j, oy, t_first, t_step);
        break;
    default: // 7 (the host lets no other shift through)
        ingest_scaled_row_s<WIDE, 3, true>(j, oy, t_first, t_step);
        break;
    }
}

// ---- RGB: the lanes of a wavefront ------------------------------------------------------------------------------------------------
// What is per lane lives in arrays of WaveLanes::N entries.  On the device N = 1: the lane itself, each() runs its function once and
// group_sum() is a butterfly of __shfl_xor over an aligned group of g lanes (every lane of the wavefront is active: the loops around
// the phases depend on nothing a lane owns).  On the host N = 64: each() is a loop over the lanes, group_sum() adds up each aligned
// group -- phase by phase, what the wavefront does in lockstep.
#if defined(__HIP_DEVICE_COMPILE__)
struct WaveLanes {
    static constexpr int N = 1;
    template <class F> __device__ __forceinline__ void each(F &&f) const { f(0, (int) threadIdx.x); }
    __device__ __forceinline__ void group_sum(uint32_t (&v)[N], int g) const
    {
        for (int m = 1; m < g; m <<= 1) {
            v[0] += (uint32_t) __shfl_xor((int) v[0], m);
        }
    }
};
#else
struct WaveLanes {
    static constexpr int N = 64;
    template <class F> void each(F &&f) const
    {
        for (int lane = 0; lane < N; lane++) {
            f(lane, lane);
        }
    }
    void group_sum(uint32_t (&v)[N], int g) const
    {
        for (int first = 0; first < N; first += g) {
            uint32_t sum = 0;
            for (int i = 0; i < g; i++) {
                sum += v[first + i];
            }
            for (int i = 0; i < g; i++) {
                v[first + i] = sum;
            }
        }
    }
};
#endif
constexpr int kRgbScaledSpan = 256; // source pixels a wavefront covers in one go: 64 lanes of 4

// chroma row cy (below ch') of job j at shift S: the spans of 256 source pixels from xb_first on in steps of xb_step (multiples of
// 256), all 64 lanes of the wavefront together
template <bool WIDE, int S> __host__ __device__ __forceinline__ void ingest_rgb_scaled_band_s(const ScaledRgbJob &j, int cy, int xb_first, int xb_step)
{
    constexpr int N = 1 << S, L = WaveLanes::N;
    const WaveLanes lanes;
    const int sw = j.sw, sh = j.sh, hs = j.hs, vs = j.vs;
    const int ow = (sw + N - 1) >> S, oh = (sh + N - 1) >> S, cw = (ow + (1 << hs) - 1) >> hs;
    const int cshift = hs + S;                               // a chroma footprint is 1 << cshift source pixels wide: 2 .. 32
    const int gc = cshift >= 2 ? 1 << (cshift - 2) : 1;      // ... that many lanes; 2 pixels wide: two footprints in a lane
    const uint32_t cbias = 32896u << (hs + vs + 2 * S);
    const int cdown = 8 + hs + vs + 2 * S;
    // general form: pixels are dwords where every row of the surface starts 4-byte aligned (ingest_rgb.h)
    const bool aligned = ((((uintptr_t) j.src) | j.pitch) & 3) == 0;
    (void) aligned;
    for (int xb = xb_first; xb < sw; xb += xb_step) {
        uint32_t up0[L], un0[L], vp0[L], vn0[L], up1[L], un1[L], vp1[L], vn1[L]; // chroma sums of the lane: footprint 0, and 1 where it has two
        lanes.each([&](int li, int) { up0[li] = un0[li] = vp0[li] = vn0[li] = up1[li] = un1[li] = vp1[li] = vn1[li] = 0; });
        for (int strip = 0; strip < 1 << vs; strip++) {
            const int oy = (cy << vs) + strip; // the luma row of the strip (at or below H': its source rows are the last one again, for chroma alone)
            uint32_t ys0[L], ys1[L];
            // phase 1: load the strip's n rows, sum them in the lane
            lanes.each([&](int li, int lane) {
                const int x = lane_offset(xb + 4 * lane);
                uint32_t px[N][4];
#pragma unroll
                for (int r = 0; r < N; r++) {
                    const int y = oy * N + r < sh ? oy * N + r : sh - 1; // (rows below the picture: its last row again)
                    const uint8_t *row = j.src + (size_t) y * j.pitch;
                    if constexpr (WIDE) { // (sw is a multiple of 4: a vector lies inside the row or behind it, where it is the last pixel four times)
                        const u32x4 q = ld_global<u32x4>(row, 4 * (uint32_t) (x < sw ? x : sw - 4));
                        const bool in = x < sw;
                        px[r][0] = in ? q[0] : q[3], px[r][1] = in ? q[1] : q[3], px[r][2] = in ? q[2] : q[3], px[r][3] = q[3];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int xc = x + i < sw ? x + i : sw - 1; // (pixels right of the picture: its last pixel again)
                            px[r][i] = rgb_pixel(row, 4 * (uint32_t) xc, aligned);
                        }
                    }
                }
                uint32_t a = 0, b = 0; // luma: pixels 0, 1 / 2, 3
#pragma unroll
                for (int r = 0; r < N; r++) {
                    a = dot4_u8(px[r][1], j.csc.ycoef, dot4_u8(px[r][0], j.csc.ycoef, a));
                    b = dot4_u8(px[r][3], j.csc.ycoef, dot4_u8(px[r][2], j.csc.ycoef, b));
                }
                ys0[li] = S == 1 ? a : a + b, ys1[li] = b;
                uint32_t p0 = 0, n0 = 0, p1 = 0, n1 = 0, q0 = 0, m0 = 0, q1 = 0, m1 = 0; // U pos / neg, V pos / neg of pixels 0, 1 and of 2, 3
#pragma unroll
                for (int r = 0; r < N; r++) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        p0 = dot4_u8(px[r][i], j.csc.upos, p0), n0 = dot4_u8(px[r][i], j.csc.uneg, n0);
                        q0 = dot4_u8(px[r][i], j.csc.vpos, q0), m0 = dot4_u8(px[r][i], j.csc.vneg, m0);
                        p1 = dot4_u8(px[r][2 + i], j.csc.upos, p1), n1 = dot4_u8(px[r][2 + i], j.csc.uneg, n1);
                        q1 = dot4_u8(px[r][2 + i], j.csc.vpos, q1), m1 = dot4_u8(px[r][2 + i], j.csc.vneg, m1);
                    }
                }
                if (cshift >= 2) {
                    up0[li] += p0 + p1, un0[li] += n0 + n1, vp0[li] += q0 + q1, vn0[li] += m0 + m1;
                } else {
                    up0[li] += p0, un0[li] += n0, vp0[li] += q0, vn0[li] += m0;
                    up1[li] += p1, un1[li] += n1, vp1[li] += q1, vn1[li] += m1;
                }
            });
            // phase 2: a luma footprint of 8 pixels is two lanes
            if constexpr (S == 3) {
                lanes.group_sum(ys0, 2);
            }
            // phase 3: the strip's luma samples
            if (oy < oh) {
                lanes.each([&](int li, int lane) {
                    const int x = xb + 4 * lane;
                    uint8_t *yrow = j.dst[0] + (size_t) oy * (size_t) j.ystride;
                    const uint32_t yoff = j.csc.yoff << (2 * S);
                    if constexpr (S == 1) {
                        const uint32_t o[2] = {(ys0[li] + yoff) >> (8 + 2 * S), (ys1[li] + yoff) >> (8 + 2 * S)};
                        st_samples<2, false>(yrow, x >> 1, o, ow);
                    } else {
                        const uint32_t o[1] = {(ys0[li] + yoff) >> (8 + 2 * S)};
                        if (S == 2 || (lane & 1) == 0) {
                            st_samples<1, false>(yrow, x >> S, o, ow);
                        }
                    }
                });
            }
        }
        // phase 4: a chroma footprint wider than 4 pixels is gc lanes
        if (gc > 1) {
            lanes.group_sum(up0, gc);
            lanes.group_sum(un0, gc);
            lanes.group_sum(vp0, gc);
            lanes.group_sum(vn0, gc);
        }
        // phase 5: the chroma samples, from the first lane of each group
        lanes.each([&](int li, int lane) {
            const int x = xb + 4 * lane;
            const size_t crow = (size_t) cy * (size_t) j.cstride;
            if (cshift >= 2) {
                if ((lane & (gc - 1)) == 0) {
                    const uint32_t u = (up0[li] + cbias - un0[li]) >> cdown, v = (vp0[li] + cbias - vn0[li]) >> cdown;
                    const uint32_t o_u[1] = {u < 255u ? u : 255u}, o_v[1] = {v < 255u ? v : 255u};
                    st_samples<1, false>(j.dst[1] + crow, x >> cshift, o_u, cw);
                    st_samples<1, false>(j.dst[2] + crow, x >> cshift, o_v, cw);
                }
            } else {
                const uint32_t u0 = (up0[li] + cbias - un0[li]) >> cdown, u1 = (up1[li] + cbias - un1[li]) >> cdown;
                const uint32_t v0 = (vp0[li] + cbias - vn0[li]) >> cdown, v1 = (vp1[li] + cbias - vn1[li]) >> cdown;
                const uint32_t o_u[2] = {u0 < 255u ? u0 : 255u, u1 < 255u ? u1 : 255u}, o_v[2] = {v0 < 255u ? v0 : 255u, v1 < 255u ? v1 : 255u};
                st_samples<2, false>(j.dst[1] + crow, x >> 1, o_u, cw);
                st_samples<2, false>(j.dst[2] + crow, x >> 1, o_v, cw);
            }
        });
    }
}

// The shift is one value for the whole job, so the switch stands outside the loops.
template <bool WIDE> __host__ __device__ __forceinline__ void ingest_rgb_scaled_band(const ScaledRgbJob &j, int cy, int xb_first, int xb_step)
{
    switch (j.shift) {
    case 1:
        ingest_rgb_scaled_band_s<WIDE, 1>(j, cy, xb_first, xb_step);
        break;
    case 2:
        ingest_rgb_scaled_band_s<WIDE, 2>(j, cy, xb_first, xb_step);
        break;
    default: // 3 (the host lets no other shift through)
        ingest_rgb_scaled_band_s<WIDE, 3>(j, cy, xb_first, xb_step);
        break;
    }
}

// ---- which source an encoder takes (device-free: swept on the CPU by tools/ingest_scale_check.cpp) ---------------------------
namespace ingest_scale {

struct Source {
    enum Kind { PLANAR, SEMI, RGB } kind = PLANAR;
    int shift = 0;            // 0: the plain ingest's business
    int plain_layout = 0;     // the layout without its scale value
    int enc_w = 0, enc_h = 0; // what the encoder must be
    int nplanes = 0;          // source planes the layout has
    size_t row_bytes[3] = {0, 0, 0};
    int rows[3] = {0, 0, 0};
};

inline bool rgb_format(int subsamp)
{
    return subsamp == DSV_SUBSAMP_444 || subsamp == DSV_SUBSAMP_422 || subsamp == DSV_SUBSAMP_420 || subsamp == DSV_SUBSAMP_411 ||
           subsamp == DSV_SUBSAMP_410;
}

// The layout grammar is the out surfaces' (surface_layout.h: one grammar for both directions, 0x1010 held back here too); the source
// planes are dsv_mk_frame's for src_w x src_h in the format.  false for a layout outside the grammar, a size <= 0, a format that is
// none of the six (RGB: of the five).
inline bool plan_source(int src_w, int src_h, int subsamp, int layout, Source *out)
{
    Source s;
    s.shift = delivery::layout_shift(layout);
    s.plain_layout = delivery::layout_unscaled(layout);
    if (delivery::is_rgb_layout(layout)) {
        s.kind = Source::RGB;
    } else if (s.plain_layout == DSV2HIP_SURFACE_PLANAR) {
        s.kind = Source::PLANAR;
    } else if (s.plain_layout == DSV2HIP_SURFACE_SEMIPLANAR) {
        s.kind = Source::SEMI;
    } else {
        return false;
    }
    if (src_w <= 0 || src_h <= 0 || !(rgb_format(subsamp) || (subsamp == DSV_SUBSAMP_UYVY && s.kind != Source::RGB))) {
        return false;
    }
    const int hs = DSV_FORMAT_H_SHIFT(subsamp), vs = DSV_FORMAT_V_SHIFT(subsamp), up = (1 << s.shift) - 1;
    const size_t w = (size_t) src_w, scw = (w + ((size_t) 1 << hs) - 1) >> hs;
    const int sch = (int) (((size_t) src_h + ((size_t) 1 << vs) - 1) >> vs);
    s.enc_w = (int) ((w + (size_t) up) >> s.shift);
    s.enc_h = (int) (((size_t) src_h + (size_t) up) >> s.shift);
    if (s.kind == Source::RGB) {
        s.nplanes = 1, s.row_bytes[0] = 4 * w, s.rows[0] = src_h;
    } else if (s.kind == Source::SEMI) {
        s.nplanes = 2, s.row_bytes[0] = w, s.row_bytes[1] = 2 * scw, s.rows[0] = src_h, s.rows[1] = sch;
    } else {
        s.nplanes = 3, s.row_bytes[0] = w, s.row_bytes[1] = s.row_bytes[2] = scw, s.rows[0] = src_h, s.rows[1] = s.rows[2] = sch;
    }
    *out = s;
    return true;
}

// A surface of that source for an encoder of enc_w x enc_h: every plane the layout has is there with a pitch of at least its SOURCE
// row's bytes, and the reduction of the source is the encoder's geometry (nested round-ups commute, so each reduced source plane
// then has exactly the encoder's plane size).
inline bool surface_fits(const Source &s, const dsv2hip_surface &sf, int enc_w, int enc_h)
{
    if (s.enc_w != enc_w || s.enc_h != enc_h) {
        return false;
    }
    for (int c = 0; c < s.nplanes; c++) {
        if (!sf.plane[c] || sf.pitch[c] < s.row_bytes[c]) {
            return false;
        }
    }
    return true;
}

// (the forms: scaled_surface_job_wide / scaled_rgb_job_wide in io_jobs.h, the existing wide predicates applied to the SOURCE)

} // namespace ingest_scale
} // namespace dsv2
