// io_jobs.h -- the job records of the kernels a picture enters the encoder (ingest.hip) and leaves the decoder (egress.hip) through,
// with the predicates that pick a kernel's form, the resize arithmetic the records carry, and the launch functions' prototypes.
// The planners fill the records (enc_ingest.h, dec_delivery.h), the body headers (ingest_*.h, egress_*.h) read them, on the device
// and in the CPU check programs alike.  Every record is a trivially copyable aggregate of whole dwords: a kernel fetches it by
// value and pins it to scalar registers with pin() (dev.h).  The byte layouts are pinned at the end of this file.
#pragma once

#include <stddef.h>

#include "dev.h"

namespace dsv2 {

// The RGB -> YUV conversion of include/dsv2_hip.h as the ingest kernels take it: each row of the matrix as byte quads in the order the
// colour bytes take in a pixel dword, 0 for a fourth byte -- the byte order lives in these quads and nowhere else.  Chroma rows:
// positive coefficients / magnitudes of the negative ones.  (enc_ingest::rgb_job_coefs)
struct RgbInCoefs {
    uint32_t ycoef, upos, uneg, vpos, vneg;
    uint32_t yoff; // 128 + 256 * ybase
};
// The YUV -> RGB conversion of include/dsv2_hip.h as the egress kernels take it (delivery::rgb_out_coefs)
struct RgbOutCoefs {
    int ky, ybase, rv, gu, gv, bu;
};

struct SurfaceJob { // one SOURCE plane of a caller's surface (dsv2hip_surface) on its way into the bordered source planes (ingest.hip:
                    // k_ingest_surface); 48 bytes
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch
    size_t pitch;
    uint8_t *dst, *dst2; // plane(s) from dframe_alloc; dst2 != null: the source rows are U0 V0 U1 V1 ..., U goes to dst, V to dst2
    int dstride;         // of dst and dst2 (the two chroma planes of a frame share their geometry)
    int w, h;            // visible pixels of each destination plane: the source row holds w bytes (2 * w with dst2)
};
struct RgbJob { // one packed four-byte RGB surface (dsv2hip_surface, BGRA / RGBA) on its way into the three bordered source planes, converted
                // on the way (ingest_rgb.h, ingest.hip: k_ingest_rgb); 88 bytes
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch, w pixels of 4 bytes
    size_t pitch;
    uint8_t *dst[3];      // Y, U, V planes from dframe_alloc
    int ystride, cstride; // of dst[0]; of dst[1] and dst[2] (the two chroma planes of a frame share their geometry)
    int w, h;             // of the picture
    int hs, vs;           // the stream's chroma shifts
    RgbInCoefs csc;       // the quads in the surface's channel order
};
constexpr int kRgb3Packed = 0, kRgb3Planar = 1; // Rgb3Job::kind
struct Rgb3Job { // one RGB surface without a fourth byte (dsv2hip_surface: BGR / RGB, three bytes a pixel; RGBP, a plane per colour) on its way
                 // into the three bordered source planes, converted on the way (ingest_rgb3.h, ingest.hip: k_ingest_rgb3); 128 bytes
    const uint8_t *src[3]; // device memory, any alignment.  Packed: row y at src[0] + y * pitch[0], w pixels of 3 bytes, src[1..2] and
    size_t pitch[3];       // pitch[1..2] unused.  Planar: row y of R, G, B at src[c] + y * pitch[c], w bytes
    uint8_t *dst[3];       // Y, U, V planes from dframe_alloc
    int ystride, cstride;  // RgbJob's, as all that follows but `kind`
    int w, h;
    int hs, vs;
    int kind;              // kRgb3Packed, kRgb3Planar; one launch takes jobs of one kind
    RgbInCoefs csc;        // the quads in the order the colour bytes take in a pixel dword: memory order (packed), R G B (planar)
};
struct EgressJob { // one plane of a decoded picture on its way into the picture the caller receives (egress.hip: k_egress); 40 bytes
    DPlane src;   // reconstruction plane (dframe_alloc: bordered, 16-byte aligned origin and stride)
    uint8_t *dst; // the same w x h pixels: device memory (packed, dstride = w) or a plane of a pinned host frame
    int dstride;
    int sharp;    // luma under -postsharp: dsv_post_process (bmc.c:340) applied in registers on the way
};
// w: the plane's width (the decoder's staged luma, 16-byte aligned origin and stride: w % 16 == 0 decides)
inline bool egress_job_wide(const EgressJob &j, int w) { return ((((uintptr_t) j.dst) | (uintptr_t) j.dstride) & 15) == 0 && w % 16 == 0; }
struct UvEgressJob { // both chroma planes of a decoded picture on their way into ONE interleaved plane of a caller's surface (dsv2hip_out_surface,
                     // SEMIPLANAR: rows U0 V0 U1 V1 ...), converted to 4:2:0 on the way or not (egress.hip: k_egress_uv); 56 bytes.  The two
                     // source planes of a frame share their geometry.
    const uint8_t *su, *sv; // pixel (0,0) of the reconstruction's U and V planes (dframe_alloc: bordered, 16-byte aligned origin and stride)
    uint8_t *dst;           // device memory, any alignment: row y at dst + y * dpitch, 2 * cw bytes of it written
    int dpitch;
    int sstride, sw, sh;    // of both source planes
    int cw, ch;             // chroma samples per row / rows of the delivered picture (= sw x sh with mode 0)
    int mode;               // To420Job's: 0 as decoded, 1 from 4:4:4, 2 from 4:2:2, 3 from 4:1:1, 4 from "4:1:0"
};
inline bool uv_job_wide(const UvEgressJob &j) { return ((((uintptr_t) j.dst) | (uintptr_t) j.dpitch) & 15) == 0 && j.cw % 8 == 0; }
constexpr int kTensorU8 = 0, kTensorF16 = 1, kTensorBF16 = 2, kTensorF32 = 3; // RgbOutJob::dtype, TensorInJob::dtype (DSV2HIP_TENSOR_*)
inline int tensor_elem(int dtype) { return dtype == kTensorU8 ? 1 : dtype == kTensorF32 ? 4 : 2; } // bytes of an element
// RgbOutJob::layout: where the converted picture goes -- a packed four-byte RGB surface (dsv2hip_out_surface, BGRA / RGBA), the three
// planes R, G, B of a tensor (dsv2hip_out_tensor) or an interleaved [h, w, 3] tensor (dsv2hip_out_hwc); one launch takes one layout
constexpr int kRgbOutPacked = 0, kRgbOutPlanar = 1, kRgbOutInterleaved = 2, kRgbOutLayouts = 3;
struct RgbOutJob { // one decoded picture on its way out as RGB, converted on the way (egress_rgb.h, egress.hip: k_egress_rgb); 144 bytes.
                   // What every layout reads comes first, the tensors' element type and constants last.
    const uint8_t *sy, *su, *sv; // pixel (0,0) of the luma and the chroma planes: 16-byte aligned origin and stride, rows readable up to the
                                 // next multiple of 4 bytes (dframe_alloc's border; the decoder's staged luma: its stride)
    int ystride, cstride;        // of sy; of su and sv (the two chroma planes of a frame share their geometry)
    int w, h;                    // of the picture
    int hs, vs;                  // the stream's chroma shifts
    RgbOutCoefs csc;
    int bgra;                    // packed: the byte order, non-zero B G R A, zero R G B A; interleaved: the element order, non-zero B G R,
                                 // zero R G B (which of R and B is byte / element 0); planar: 0 (the planes are R, G, B)
    int layout;                  // kRgbOut*
    uint8_t *dst[3];             // device memory.  Packed: any alignment, row y at dst[0] + y * dpitch[0], 4 * w bytes of it written.
    int dpitch[3];               // Planar: element aligned, row y of R, G, B at dst[c] + y * dpitch[c], w elements of it written.
                                 // Interleaved: element aligned, pixel x of row y at dst[0] + y * dpitch[0] + 3 * x * elem, 3 * w elements
                                 // written.  Pitches in bytes, multiples of the element size.  Only planar uses dst[1..2], dpitch[1..2]
    int dtype;                   // tensors: kTensor*; packed: kTensorU8
    float scale[3], bias[3];     // float dtypes: plane c (planar) / element k of every pixel in memory order (interleaved) holds
                                 // fl32(fl32(byte * scale) + bias), rounded to the element type
};
// Which launches may take the wide form: the destination pointers and pitches of the layout -- packed: multiples of 16 bytes; tensors:
// of four elements, every plane's where planar -- and w a multiple of 4.  A thread's row then leaves as whole vector stores.
inline bool rgb_out_job_wide(const RgbOutJob &j)
{
    uintptr_t bits = 0;
    for (int c = 0; c < (j.layout == kRgbOutPlanar ? 3 : 1); c++) {
        bits |= ((uintptr_t) j.dst[c]) | (uintptr_t) j.dpitch[c];
    }
    const uintptr_t grain = j.layout == kRgbOutPacked ? 16 : (uintptr_t) (4 * tensor_elem(j.dtype));
    return (bits & (grain - 1)) == 0 && (j.w & 3) == 0;
}
struct TensorInJob { // one picture that is three planes R, G, B of a caller's float tensor (dsv2hip_in_tensor: binary16, bfloat16 or binary32
                     // elements) on its way into the three bordered source planes: taken through the job's per-plane scale and bias, clamped and
                     // rounded to bytes, then converted as a planar RGB surface is (ingest_tensor.h, ingest.hip: k_ingest_tensor); 152 bytes.
                     // It shares Rgb3Job's destination side.  (A uint8 tensor is an Rgb3Job.)
    const uint8_t *src[3]; // device memory, element aligned: row y of R, G, B at src[c] + y * pitch[c], w elements of it read
    size_t pitch[3];       // bytes, multiples of the element size
    uint8_t *dst[3];       // Y, U, V planes from dframe_alloc
    int ystride, cstride;  // RgbJob's, as w, h, hs, vs and the quads
    int w, h;
    int hs, vs;
    int dtype;             // kTensorF16, kTensorBF16, kTensorF32
    RgbInCoefs csc;        // the planar kind's: R G B in bytes 0..2 of a pixel dword
    float scale[3], bias[3]; // the byte of element e of plane c is rint(min(max(fl32(fl32(e * scale[c]) + bias[c]), 0), 255)), 0 for a NaN
};
// every plane's pointer and pitch multiples of four elements and w of 4: a thread's four elements of a row arrive as one vector load
inline bool tensor_in_job_wide(const TensorInJob &j)
{
    uintptr_t bits = 0;
    for (int c = 0; c < 3; c++) {
        bits |= ((uintptr_t) j.src[c]) | (uintptr_t) j.pitch[c];
    }
    return (bits & (uintptr_t) (4 * tensor_elem(j.dtype) - 1)) == 0 && (j.w & 3) == 0;
}
struct HwcInJob { // one picture that is a caller's interleaved [h, w, 3] float tensor (dsv2hip_in_hwc: binary16, bfloat16 or binary32 elements,
                  // R G B or B G R) on its way into the three bordered source planes: element k of a pixel taken through the job's
                  // scale[k] and bias[k], clamped and rounded to byte k of the pixel's dword, then converted as a three-byte surface is
                  // (ingest_hwc.h, ingest.hip: k_ingest_hwc); 120 bytes.  It shares Rgb3Job's destination side.  (A uint8 one is an Rgb3Job.)
    const uint8_t *src;    // device memory, element aligned: pixel x of row y at src + y * pitch + 3 * x * elem, 3 * w elements of a row read
    size_t pitch;          // bytes, a multiple of the element size
    uint8_t *dst[3];       // Y, U, V planes from dframe_alloc
    int ystride, cstride;  // RgbJob's, as w, h, hs, vs and the quads
    int w, h;
    int hs, vs;
    int dtype;             // kTensorF16, kTensorBF16, kTensorF32
    RgbInCoefs csc;        // the packed kind's: memory order is byte order, so B G R and R G B differ only in these quads
    float scale[3], bias[3]; // of element k of every pixel, in memory order: TensorInJob's formula with k for c
};
// pointer and pitch multiples of four elements and w of 4: a thread's twelve elements of a row arrive as three vector loads
inline bool hwc_in_job_wide(const HwcInJob &j)
{
    return ((((uintptr_t) j.src) | (uintptr_t) j.pitch) & (uintptr_t) (4 * tensor_elem(j.dtype) - 1)) == 0 && (j.w & 3) == 0;
}
struct ScaleOutJob { // one plane of a decoded picture on its way out at half, quarter or eighth size (dsv2hip_out_surface, DSV2HIP_SCALE_*): the box
                     // average of include/dsv2_hip.h (egress_scale.h, egress.hip: k_egress_scale) into a plane of the caller's surface, or into the
                     // decoder's staging picture that k_egress_uv / k_egress_rgb then read; 40 bytes
    const uint8_t *src; // pixel (0,0) of the source plane: 16-byte aligned origin and stride, rows readable up to the next multiple of 16 bytes
                        // (dframe_alloc's border; the decoder's staged luma: its stride)
    uint8_t *dst;       // device memory, any alignment: row y at dst + y * dpitch, ceil(pw / n) bytes of it written, ceil(ph / n) rows
    int sstride;
    int pw, ph;         // of the source plane
    int dpitch;
    int shift;          // 1, 2, 3: n = 1 << shift
};
// row_room: bytes of a destination row that may be written (a caller's surface: the reduced width; the staging picture: its stride)
inline bool scale_job_wide(const ScaleOutJob &j, int row_room)
{
    return ((((uintptr_t) j.dst) | (uintptr_t) j.dpitch) & 7) == 0 && row_room % (16 >> j.shift) == 0;
}
struct ResizeOutJob { // one plane of a decoded picture on its way out at a size the caller names (dsv2hip_dec_batch_surface_sized): the exact area
                      // average of include/dsv2_hip.h (egress_resize.h, egress.hip: k_egress_resize) into a plane of the caller's surface, or into
                      // the decoder's staging picture that k_egress_uv / k_egress_rgb then read; 72 bytes
    const uint8_t *src; // pixel (0,0) of the source plane; nothing outside [0, pw) x [0, ph) is read
    uint8_t *dst;       // device memory, any alignment: row y at dst + y * dpitch, ow bytes of it written, oh rows
    int sstride, dpitch;
    int pw, ph, ow, oh; // of the source plane; of the delivered one: ow <= pw <= 8 * ow, oh <= ph <= 8 * oh
    int a, b, c, d;     // pw / ow = a / b and ph / oh = c / d in lowest terms
    uint32_t D;         // a * c, at most 2^24
    uint32_t rD, rb, rd; // resize_recip of D, b, d: a quotient by one of them is mulhi(n, r) or one more (egress_resize.h: resize_div)
};
inline uint32_t resize_recip(uint32_t den) { return den <= 1 ? 0xffffffffu : (uint32_t) ((1ull << 32) / den); } // min(floor(2^32 / den), 2^32 - 1)
constexpr uint32_t kResizeMaxD = 1u << 24;
constexpr int kResizeMaxSide = 32768;
inline int resize_gcd(int x, int y)
{
    while (y) {
        const int t = x % y;
        x = y, y = t;
    }
    return x;
}
// a plane of pw x ph to ow x oh: inside the bounds of the contract (reduction only, down to an eighth, D and the sides within what
// 32-bit sums and coordinates hold)
inline bool resize_allowed(int pw, int ph, int ow, int oh)
{
    if (ow <= 0 || oh <= 0 || ow > pw || oh > ph || pw > kResizeMaxSide || ph > kResizeMaxSide || (int64_t) 8 * ow < pw || (int64_t) 8 * oh < ph) {
        return false;
    }
    return (uint64_t) (pw / resize_gcd(pw, ow)) * (uint64_t) (ph / resize_gcd(ph, oh)) <= kResizeMaxD;
}
inline ResizeOutJob resize_job(const uint8_t *src, int sstride, int pw, int ph, uint8_t *dst, int dpitch, int ow, int oh)
{
    const int gx = resize_gcd(pw, ow), gy = resize_gcd(ph, oh);
    ResizeOutJob j{src, dst, sstride, dpitch, pw, ph, ow, oh, pw / gx, ow / gx, ph / gy, oh / gy, 0, 0, 0, 0};
    j.D = (uint32_t) j.a * (uint32_t) j.c;
    j.rD = resize_recip(j.D), j.rb = resize_recip((uint32_t) j.b), j.rd = resize_recip((uint32_t) j.d);
    return j;
}
// row_room: bytes of a destination row that may be written (a caller's surface: ow; the staging picture: its stride)
inline bool resize_job_wide(const ResizeOutJob &j, int row_room) { return ((((uintptr_t) j.dst) | (uintptr_t) j.dpitch) & 3) == 0 && row_room % 4 == 0; }

// ---- ingest.hip: the launches --------------------------------------------------------------------------------------------------------
// n source planes of at most max_h rows; wide: every job's source row bytes, pointer and pitch are multiples of 16 (surface_job_wide)
void ingest_surface_batch(hipStream_t s, const SurfaceJob *d_jobs, int n, int max_h, bool wide);
inline bool surface_job_wide(const SurfaceJob &j)
{
    return ((((uintptr_t) j.src) | j.pitch | (size_t) (j.dst2 ? 2 * j.w : j.w)) & 15) == 0;
}
// n RGB surfaces of h rows; wide: every job's source pointer and pitch are multiples of 16 and w of 4 (rgb_job_wide)
void ingest_rgb_batch(hipStream_t s, const RgbJob *d_jobs, int n, int h, bool wide);
inline bool rgb_job_wide(const RgbJob &j) { return ((((uintptr_t) j.src) | j.pitch) & 15) == 0 && (j.w & 3) == 0; }
// n three-byte or planar RGB surfaces of h rows, all of one kind (planar: Rgb3Job::kind of every job is kRgb3Planar); wide: every
// job's source pointers and pitches -- those its kind uses -- and w are multiples of 4 (rgb3_job_wide)
void ingest_rgb3_batch(hipStream_t s, const Rgb3Job *d_jobs, int n, int h, bool planar, bool wide);
inline bool rgb3_job_wide(const Rgb3Job &j)
{
    uintptr_t m = (uintptr_t) j.src[0] | j.pitch[0] | (uintptr_t) j.w;
    if (j.kind == kRgb3Planar) {
        m |= (uintptr_t) j.src[1] | j.pitch[1] | (uintptr_t) j.src[2] | j.pitch[2];
    }
    return (m & 3) == 0;
}
// n float tensors of h rows (TensorInJob above; the element types may differ from job to job); wide: every job's plane pointers and
// pitches are multiples of four elements and w of 4 (tensor_in_job_wide)
void ingest_tensor_batch(hipStream_t s, const TensorInJob *d_jobs, int n, int h, bool wide);
// n interleaved float tensors of h rows (HwcInJob above; element types and orders may differ from job to job); wide: every job's
// pointer and pitch are multiples of four elements and w of 4 (hwc_in_job_wide)
void ingest_hwc_batch(hipStream_t s, const HwcInJob *d_jobs, int n, int h, bool wide);
// Half, quarter and eighth-size ingest (dsv2hip_enc_batch_surface_scaled): the records of k_ingest_surface_scaled and
// k_ingest_rgb_scaled (ingest.hip, ingest_scale.h), in tables of their own behind the two above.
struct ScaledSurfaceJob { // one SOURCE plane of a caller's surface, box-averaged (the decoder's REDUCTION, include/dsv2_hip.h) on its way into a
                          // bordered source plane of the reduced geometry; 48 bytes
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch
    size_t pitch;
    uint8_t *dst, *dst2; // plane(s) from dframe_alloc; dst2 != null: the source rows are U0 V0 U1 V1 ..., reduced U goes to dst, V to dst2
    int dstride;         // of dst and dst2
    int pw, ph;          // samples per row and rows of the SOURCE plane (with dst2: U V pairs per row, the row holds 2 * pw bytes)
    int shift;           // 1, 2, 3: n = 1 << shift; the destination holds ceil(pw / n) x ceil(ph / n)
};
struct ScaledRgbJob { // one packed four-byte RGB surface, converted and reduced with one rounding per sample on its way into the three bordered
                      // source planes of the reduced geometry; 96 bytes
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch, sw pixels of 4 bytes
    size_t pitch;
    uint8_t *dst[3];      // Y, U, V planes from dframe_alloc
    int ystride, cstride; // of dst[0]; of dst[1] and dst[2]
    int sw, sh;           // of the picture IN THE SURFACE; the encoder's is ceil(sw / n) x ceil(sh / n)
    int hs, vs;           // the stream's chroma shifts
    int shift;            // 1, 2, 3
    RgbInCoefs csc;       // RgbJob's quads
};
// n source planes, the widest source row max_row_bytes, the most reduced rows max_rows; wide: the predicate of surface_job_wide on the SOURCE
void ingest_surface_scaled_batch(hipStream_t s, const ScaledSurfaceJob *d_jobs, int n, int max_row_bytes, int max_rows, bool wide);
inline bool scaled_surface_job_wide(const ScaledSurfaceJob &j)
{
    return ((((uintptr_t) j.src) | j.pitch | (size_t) (j.dst2 ? 2 * j.pw : j.pw)) & 15) == 0;
}
// n RGB surfaces, the widest max_sw pixels, the most chroma rows of the reduced picture max_crows; wide: rgb_job_wide's predicate on the SOURCE
void ingest_rgb_scaled_batch(hipStream_t s, const ScaledRgbJob *d_jobs, int n, int max_sw, int max_crows, bool wide);
inline bool scaled_rgb_job_wide(const ScaledRgbJob &j) { return ((((uintptr_t) j.src) | j.pitch) & 15) == 0 && (j.sw & 3) == 0; }
// Ingest at any larger size (dsv2hip_enc_batch_surface_sized): the records of k_ingest_sized and k_ingest_rgb_sized
// (ingest.hip, ingest_resize.h), in tables of their own behind the scaled ones.
struct SizedRatio { // pw x ph -> ow x oh, the exact area average of include/dsv2_hip.h (ResizeOutJob's arithmetic); 24 bytes
    uint16_t a, b, c, d; // pw / ow = a / b and ph / oh = c / d in lowest terms (a, c <= 32768)
    uint32_t D;          // a * c
    uint32_t rD, rb, rd; // resize_recip of the final divisor (YUV: D, RGB: 256 * D), of b, of d
};
struct SizedSurfaceJob { // one source plane -- or the U or the V half of an interleaved one -- resampled into a bordered source plane of the
                         // encoder; 64 bytes
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch, sample i at byte off + step * i of it
    size_t pitch;
    uint8_t *dst; // plane from dframe_alloc
    int dstride;
    int ow, oh; // of dst
    SizedRatio q;
    uint16_t step, off; // 1, 0: a planar plane; 2, 0 / 2, 1: U / V of an interleaved plane
};
struct SizedRgbJob { // one packed four-byte RGB surface, resampled as RGB and converted with one rounding per sample into the three bordered
                     // source planes of the encoder; 136 bytes
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch, pixels of 4 bytes
    size_t pitch;
    uint8_t *dst[3];      // Y, U, V planes from dframe_alloc
    int ystride, cstride; // of dst[0]; of dst[1] and dst[2]
    int ow, oh, cw, ch;   // of dst[0]; of dst[1] and dst[2]
    SizedRatio ql, qc;    // the surface's picture -> ow x oh; -> cw x ch
    RgbInCoefs csc;       // RgbJob's quads
};
// n jobs, the widest destination row max_ow samples, the most destination rows max_oh; wide: sized_job_wide of every job
void ingest_sized_batch(hipStream_t s, const SizedSurfaceJob *d_jobs, int n, int max_ow, int max_oh, bool wide);
// row_bytes: of the SOURCE plane's rows (an interleaved plane: of both halves together)
inline bool sized_job_wide(const SizedSurfaceJob &j, size_t row_bytes) { return ((((uintptr_t) j.src) | j.pitch | row_bytes) & 3) == 0; }
// n RGB surfaces, the widest luma row max_ow, the most luma plus chroma rows max_rows; wide: sized_rgb_job_wide of every job
void ingest_rgb_sized_batch(hipStream_t s, const SizedRgbJob *d_jobs, int n, int max_ow, int max_rows, bool wide);
inline bool sized_rgb_job_wide(const SizedRgbJob &j) { return ((((uintptr_t) j.src) | j.pitch) & 3) == 0; }

// ---- egress.hip: the launches --------------------------------------------------------------------------------------------------------
// decoder egress: n planes (device table) copied out of the reconstruction into the delivered picture, the sharpened ones
// through dsv_post_process on the way.  wide: every job's width is a multiple of 16 and its destination and destination
// stride are 16-byte aligned (16-byte loads and stores); else any width and alignment.  any_sharp: some job has `sharp` set.
// max_h: the tallest plane.
void egress_batch(hipStream_t s, const EgressJob *d_jobs, int n, int max_h, bool wide, bool any_sharp);
// ... into a semiplanar surface: n pictures' chroma (device table), U and V interleaved into one plane, converted to 4:2:0 on
// the way where the job's mode says so.  wide: every job's destination and pitch are multiples of 16 and its cw of 8
// (uv_job_wide); any_conv: some job has mode != 0.  max_ch: the most rows delivered.
void egress_uv_batch(hipStream_t s, const UvEgressJob *d_jobs, int n, int max_ch, bool wide, bool any_conv);
// ... as RGB, converted on the way (egress_rgb.h): n pictures of at most h rows (device table), every job of the given layout
// (kRgbOut*: packed four-byte surfaces, planar or interleaved tensors).  wide: rgb_out_job_wide of every job.
void egress_rgb_batch(hipStream_t s, const RgbOutJob *d_jobs, int n, int h, int layout, bool wide);
// ... at half, quarter or eighth size: n planes (device table) box-averaged on the way (egress_scale.h) into a caller's plane or the
// decoder's staging picture.  wide: every job's destination and pitch are multiples of 8 and its row is writable up to a multiple of
// 16 >> shift bytes (scale_job_wide).  max_oh: the most rows delivered.
void egress_scale_batch(hipStream_t s, const ScaleOutJob *d_jobs, int n, int max_oh, bool wide);
// ... at a size the caller names: n planes (device table) area-averaged on the way (egress_resize.h) into a caller's plane or the
// decoder's staging picture.  wide: every job's destination and pitch are multiples of 4 and its row is writable up to a multiple of
// 4 bytes (resize_job_wide).  max_ow, max_oh: the most samples a row and the most rows delivered.
void egress_resize_batch(hipStream_t s, const ResizeOutJob *d_jobs, int n, int max_ow, int max_oh, bool wide);

// ---- the byte layouts: what the host writes into a table is what pin() reads back, dword for dword ----------------------------------------
#define DSV2_IO_RECORD(T, bytes) static_assert(sizeof(T) == (bytes) && sizeof(T) % 4 == 0 && __is_trivially_copyable(T), #T)
DSV2_IO_RECORD(SurfaceJob, 48);
DSV2_IO_RECORD(RgbJob, 88);
DSV2_IO_RECORD(Rgb3Job, 128);
DSV2_IO_RECORD(TensorInJob, 152);
DSV2_IO_RECORD(HwcInJob, 120);
DSV2_IO_RECORD(ScaledSurfaceJob, 48);
DSV2_IO_RECORD(ScaledRgbJob, 96);
DSV2_IO_RECORD(SizedSurfaceJob, 64);
DSV2_IO_RECORD(SizedRgbJob, 136);
DSV2_IO_RECORD(EgressJob, 40);
DSV2_IO_RECORD(UvEgressJob, 56);
DSV2_IO_RECORD(RgbOutJob, 144);
DSV2_IO_RECORD(ScaleOutJob, 40);
DSV2_IO_RECORD(ResizeOutJob, 72);
#undef DSV2_IO_RECORD
static_assert(offsetof(RgbJob, csc) == 64 && offsetof(Rgb3Job, csc) == 100 && offsetof(TensorInJob, csc) == 100 && offsetof(HwcInJob, csc) == 68 &&
                  offsetof(ScaledRgbJob, csc) == 68 &&
                  offsetof(SizedRgbJob, csc) == 112,
              "the ingest quads stay where the six words were (HwcInJob: new with DESIGN 5.26)");
static_assert(offsetof(RgbOutJob, layout) + 4 == offsetof(RgbOutJob, dst) && offsetof(RgbOutJob, dtype) == 116,
              "what every layout reads first, the tensors' words behind it");

} // namespace dsv2
