// dev.h -- device-side plumbing shared by every kernel group of libdsv2hip.
//
// Data layout in HBM (DESIGN.md "Data layout"):
//   * pictures: planar u8, every plane surrounded by a 32-pixel border, row stride
//     rounded up to 16 bytes -- byte-identical to the reference's host layout
//     (frame.c:63-113) so that block reads that run into the border see the same bytes;
//   * coefficient planes: int32, row stride = plane width, Mallat layout (frame.c:30-60);
//   * motion vectors: 16-byte DSV_MV records, raster order; blockdata: one flag byte per block.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/dsv2_hip.h"

namespace dsv2 {

[[noreturn]] void fatal(const char *what, const char *file, int line);

#define HIPCHK(expr)                                                   \
    do {                                                               \
        hipError_t e__ = (expr);                                       \
        if (e__ != hipSuccess) {                                       \
            fprintf(stderr, "[dsv2hip] HIP error %d (%s) ", (int) e__, \
                    hipGetErrorString(e__));                           \
            dsv2::fatal(#expr, __FILE__, __LINE__);                    \
        }                                                              \
    } while (0)

// every kernel launch goes through this macro so that the stage profile can report launch counts
extern thread_local long long t_launch_count;
#define DSV2_LAUNCH(...)                \
    do {                                \
        hipLaunchKernelGGL(__VA_ARGS__); \
        dsv2::t_launch_count++;         \
    } while (0)

constexpr int kBorder = 32; // dsv_internal.h:38
constexpr int kBlockP = 14; // dsv_internal.h:127

struct DPlane {
    uint8_t *data; // device pointer to pixel (0,0)
    int stride;
    int w, h;
};

// A launch's job record: entry i of a device table the host wrote before the launch (nothing writes it during) --
// for the small records (planes, plane pairs, the compaction's job) fetched BY VALUE, THROUGH THE SCALAR CACHE, into scalar
// registers: the record's pointers and strides then live in scalar registers, and every address the kernel forms from them is a
// scalar base plus a 32-bit lane offset.  The 144-byte PlaneJob with its arrays ends up in scratch when copied this way; the
// transform and quantiser kernels bind a reference into the `const __restrict__` table instead.
#ifdef __HIPCC__
// a value / pointer every lane holds alike, told to the compiler as such: it moves to scalar registers and what is computed from it
// (addresses above all) to the scalar unit
template <class T> __device__ __forceinline__ T *uni_ptr(T *p)
{
    unsigned long long v = (unsigned long long) p;
    unsigned lo = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) v);
    unsigned hi = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) (v >> 32));
    return (T *) (((unsigned long long) hi << 32) | lo);
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni(float v) { return __builtin_bit_cast(float, uni(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ DPlane uni(const DPlane &p) { return DPlane{uni_ptr(p.data), uni(p.stride), uni(p.w), uni(p.h)}; }

template <class T> __device__ __forceinline__ T job_of(const T *tab, unsigned i)
{
    T j;
    __builtin_memcpy(&j, (const __attribute__((address_space(4))) void *) (tab + i), sizeof(T));
    return j;
}
#endif

struct DFrame {
    uint8_t *alloc = nullptr;
    size_t bytes = 0;
    DPlane p[3];
    size_t plane_off[3]; // byte offset of each plane's storage (incl. border) inside alloc
    size_t plane_len[3];
    int format = 0, w = 0, h = 0;
};

struct DCoefs {
    int32_t *data;
    int w, h;
};

void dev_zero(void *p, size_t bytes); // synchronous zero fill of device memory (nothing inside an arena scope: the arena is zeroed once)
// One device allocation per codec instance (round 4).  Inside an arena scope (DevArenaScope on the calling thread) dev_alloc
// hands out 256-byte aligned pieces of ONE hipMalloc'd block -- an encoder instance made ~75 allocations, each a driver call
// when it is made and a device-synchronising one when it is freed: what a short-lived process (one CLI process per closed-GOP
// segment) pays before its first packet and again on its way out.  A request the block cannot hold falls back to hipMalloc;
// dev_release frees only what does not lie inside a live arena (the block itself is freed by its owner).
struct DevArena {
    uint8_t *base = nullptr;
    size_t cap = 0, used = 0;
    void create(size_t bytes); // hipMalloc + zero fill + registration
    void destroy();
};
struct DevArenaScope {
    DevArenaScope(DevArena *a);
    ~DevArenaScope();
    DevArena *prev;
};
hipError_t dev_alloc(void **p, size_t bytes);
long arena_fallbacks(); // allocations an instance arena could not hold so far (0 unless CodecDev::init's estimate has drifted)
void dev_release(void *p);
size_t dframe_bytes(int format, int w, int h); // device bytes dframe_alloc asks for
void event_wait(hipEvent_t ev);        // ... for a recorded event
void set_wait_fine(bool fine);         // this thread's waits poll at 20 us (steps of one stream) instead of up to 120 us
void stream_wait(hipStream_t s);       // host wait for the stream to drain: sleeps between completion queries (dev.cpp: 10 - 120 us apart), no busy spin
// pinned host blocks the GPU may write (hostutil.cpp): recycled through dsv_free
void *pinned_pool_take(size_t bytes);
bool pinned_pool_release(void *p);
DSV_FRAME *mk_frame_pinned(int format, int width, int height);
void dframe_alloc(DFrame *f, int format, int w, int h);
void dframe_free(DFrame *f);
// copy between a host DSV_FRAME (any stride, bordered or not) and a device frame: visible pixels only
void dframe_upload(DFrame *d, const DSV_FRAME *h, hipStream_t s);
void dframe_download(const DFrame *d, DSV_FRAME *h, hipStream_t s);
// whole storage including borders (host frame must be bordered with the reference layout)
void dframe_upload_full(DFrame *d, const DSV_FRAME *h, hipStream_t s);
void dframe_download_full(const DFrame *d, DSV_FRAME *h, hipStream_t s);

void coef_dims(int format, int w, int h, int cw[3], int ch[3]);

// scratch images for the transform: three int32 planes of the luma coefficient size
struct SbtScratch {
    int32_t *t[3] = {nullptr, nullptr, nullptr};
    size_t elems = 0, elems_ll = 0;
    // t[2] (row-pass temporary) holds a whole plane: n elements.  t[0] / t[1] only ever hold LL images of level >= 1, stored
    // with the plane's row stride: (ceil(h / 2) + 1) rows of it suffice -- n_ll elements (0: as large as t[2]).
    void ensure(size_t n, size_t n_ll = 0);
    void release();
    // the three images laid out in memory the caller owns (base: 16-byte aligned, scratch_elems(n, n_ll) int32): t[2], t[0], t[1]
    bool borrowed = false;
    void borrow(int32_t *base, size_t n, size_t n_ll);
    static size_t scratch_elems(size_t n, size_t n_ll) { return ((n + 3) & ~(size_t) 3) + 2 * ((n_ll + 3) & ~(size_t) 3); }
};
inline size_t sbt_ll_elems(int cw, int ch) { return (size_t) cw * (size_t) ((ch + 1) / 2 + 1); }

// One plane of one stream as the transform and the quantiser see it.  A device table of these
// (one per stream and plane of a lockstep batch) lets a single launch serve every stream.
struct PlaneJob {
    DPlane pic;        // working picture plane: residual in (forward level 1), reconstruction out (inverse level 1)
    int32_t *coefs;    // coefficient plane
    int32_t *t[3];     // scratch images with the plane's row stride: t[2] a whole plane, t[0] / t[1] the LL images (half the rows)
    const uint8_t *bd; // per-block flag bytes
    int32_t *qv;       // dense quantised values of this plane, scan order
    const DSV_MV *mvs; // motion field (P frames)
    int q;             // frame quantiser
    int qll;           // LL step size
    int qp[3][3];      // detail step sizes [level][subband - 1]
    int *tile_count;   // quantiser: per-1024-position nonzero counts of the stream's symbol list
    unsigned qv_base;  // scan position of this plane's first value within that list
};

// --- subband transform (sbt.hip) ------------------------------------------------
// forward: u8 plane -> coefs (cw x ch).  inverse: coefs -> u8 plane (coefs preserved).
// n jobs of identical geometry (cw x ch coefficient plane); have_bd: the jobs carry block flag bytes (the adaptive filters need them)
void sbt_forward_jobs(hipStream_t s, const PlaneJob *d_jobs, int n, int cw, int ch, int plane_idx, int isP, int lossless, int nbh,
                      int nbv, bool have_bd);
void sbt_inverse_jobs(hipStream_t s, const PlaneJob *d_jobs, int n, int cw, int ch, int plane_idx, int isP, int lossless, int nbh,
                      int nbv, bool have_bd);

// --- picture helpers (frame.hip) ---------------------------------------------------
// one launch works through a device-resident table of jobs
struct PlanePair {
    DPlane src, dst;
};
struct CopyJob {
    const void *src;
    void *dst;
    size_t bytes;
};
struct IngestJob {
    const uint8_t *src; // packed planar picture in HBM
    DPlane dst[3];
};
struct SurfaceJob { // one SOURCE plane of a caller's surface (dsv2hip_surface) on its way into the bordered source planes (frame.hip:
                    // k_ingest_surface); 48 bytes, fetched by value through the scalar cache like EgressJob
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch
    size_t pitch;
    uint8_t *dst, *dst2; // plane(s) from dframe_alloc; dst2 != null: the source rows are U0 V0 U1 V1 ..., U goes to dst, V to dst2
    int dstride;         // of dst and dst2 (the two chroma planes of a frame share their geometry)
    int w, h;            // visible pixels of each destination plane: the source row holds w bytes (2 * w with dst2)
};
struct RgbJob { // one packed four-byte RGB surface (dsv2hip_surface, BGRA / RGBA) on its way into the three bordered source planes, converted
                // on the way (ingest_rgb.h, frame.hip: k_ingest_rgb); 88 bytes, fetched by value through the scalar cache like SurfaceJob
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch, w pixels of 4 bytes
    size_t pitch;
    uint8_t *dst[3];      // Y, U, V planes from dframe_alloc
    int ystride, cstride; // of dst[0]; of dst[1] and dst[2] (the two chroma planes of a frame share their geometry)
    int w, h;             // of the picture
    int hs, vs;           // the stream's chroma shifts
    // The conversion's coefficients as byte quads in the surface's channel order, 0 for alpha -- the byte order lives in these
    // quads and nowhere else.  Chroma rows: positive coefficients / magnitudes of the negative ones.
    uint32_t ycoef, upos, uneg, vpos, vneg;
    uint32_t yoff; // 128 + 256 * ybase
};
constexpr int kRgb3Packed = 0, kRgb3Planar = 1; // Rgb3Job::kind
struct Rgb3Job { // one RGB surface without a fourth byte (dsv2hip_surface: BGR / RGB, three bytes a pixel; RGBP, a plane per colour) on its way
                 // into the three bordered source planes, converted on the way (ingest_rgb3.h, frame.hip: k_ingest_rgb3); 128 bytes, fetched
                 // by value through the scalar cache like RgbJob
    const uint8_t *src[3]; // device memory, any alignment.  Packed: row y at src[0] + y * pitch[0], w pixels of 3 bytes, src[1..2] and
    size_t pitch[3];       // pitch[1..2] unused.  Planar: row y of R, G, B at src[c] + y * pitch[c], w bytes
    uint8_t *dst[3];       // Y, U, V planes from dframe_alloc
    int ystride, cstride;  // RgbJob's, as all that follows but `kind`
    int w, h;
    int hs, vs;
    int kind;              // kRgb3Packed, kRgb3Planar; one launch takes jobs of one kind
    // the quads in the order the colour bytes take in a pixel dword: memory order (packed), R G B (planar)
    uint32_t ycoef, upos, uneg, vpos, vneg;
    uint32_t yoff;
};
struct PlaneOutJob {
    DPlane src;
    uint8_t *dst; // pinned host memory, w * h bytes
};
struct To420Job { // one plane of a decoded picture on its way into a 4:2:0 output frame (frame.hip: k_to420)
    DPlane src, dst;
    int mode; // 0 copy, 1 from 4:4:4, 2 from 4:2:2, 3 from 4:1:1, 4 from "4:1:0"
};
struct EgressJob { // one plane of a decoded picture on its way into the picture the caller receives (bmc.hip: k_egress)
    DPlane src;   // reconstruction plane (dframe_alloc: bordered, 16-byte aligned origin and stride)
    uint8_t *dst; // the same w x h pixels: device memory (packed, dstride = w) or a plane of a pinned host frame
    int dstride;
    int sharp;    // luma under -postsharp: dsv_post_process (bmc.c:340) applied in registers on the way
};
// w: the plane's width (the decoder's staged luma, 16-byte aligned origin and stride: w % 16 == 0 decides)
inline bool egress_job_wide(const EgressJob &j, int w) { return ((((uintptr_t) j.dst) | (uintptr_t) j.dstride) & 15) == 0 && w % 16 == 0; }
struct UvEgressJob { // both chroma planes of a decoded picture on their way into ONE interleaved plane of a caller's surface (dsv2hip_out_surface,
                     // SEMIPLANAR: rows U0 V0 U1 V1 ...), converted to 4:2:0 on the way or not (bmc.hip: k_egress_uv); 56 bytes, fetched by
                     // value through the scalar cache like EgressJob.  The two source planes of a frame share their geometry.
    const uint8_t *su, *sv; // pixel (0,0) of the reconstruction's U and V planes (dframe_alloc: bordered, 16-byte aligned origin and stride)
    uint8_t *dst;           // device memory, any alignment: row y at dst + y * dpitch, 2 * cw bytes of it written
    int dpitch;
    int sstride, sw, sh;    // of both source planes
    int cw, ch;             // chroma samples per row / rows of the delivered picture (= sw x sh with mode 0)
    int mode;               // To420Job's: 0 as decoded, 1 from 4:4:4, 2 from 4:2:2, 3 from 4:1:1, 4 from "4:1:0"
};
inline bool uv_job_wide(const UvEgressJob &j) { return ((((uintptr_t) j.dst) | (uintptr_t) j.dpitch) & 15) == 0 && j.cw % 8 == 0; }
struct RgbOutJob { // one decoded picture on its way into a packed four-byte RGB surface (dsv2hip_out_surface, BGRA / RGBA), converted on the
                   // way (egress_rgb.h, bmc.hip: k_egress_rgb); 88 bytes, fetched by value through the scalar cache like UvEgressJob
    const uint8_t *sy, *su, *sv; // pixel (0,0) of the luma and the chroma planes: 16-byte aligned origin and stride, rows readable up to the
                                 // next multiple of 4 bytes (dframe_alloc's border; the decoder's staged luma: its stride)
    uint8_t *dst;                // device memory, any alignment: row y at dst + y * dpitch, 4 * w bytes of it written
    int ystride, cstride;        // of sy; of su and sv (the two chroma planes of a frame share their geometry)
    int dpitch;
    int w, h;                    // of the picture
    int hs, vs;                  // the stream's chroma shifts
    int ky, ybase, rv, gu, gv, bu; // the conversion of include/dsv2_hip.h
    int bgra;                    // the surface's byte order: non-zero B G R A, zero R G B A
};
inline bool rgb_out_job_wide(const RgbOutJob &j) { return ((((uintptr_t) j.dst) | (uintptr_t) j.dpitch) & 15) == 0 && (j.w & 3) == 0; }
constexpr int kTensorU8 = 0, kTensorF16 = 1, kTensorBF16 = 2, kTensorF32 = 3; // TensorOutJob::dtype (DSV2HIP_TENSOR_*)
inline int tensor_elem(int dtype) { return dtype == kTensorU8 ? 1 : dtype == kTensorF32 ? 4 : 2; } // bytes of an element
struct TensorOutJob { // one decoded picture on its way into three planes R, G, B of a caller's tensor (dsv2hip_out_tensor: uint8, binary16, bfloat16
                      // or binary32 elements), converted on the way (egress_tensor.h, bmc.hip: k_egress_tensor); 136 bytes, fetched by value
                      // through the scalar cache like RgbOutJob, whose source side it shares
    const uint8_t *sy, *su, *sv; // RgbOutJob's
    uint8_t *dst[3];             // device memory, element aligned: row y of R, G, B at dst[c] + y * dpitch[c], w elements of it written
    int ystride, cstride;
    int dpitch[3];               // bytes, multiples of the element size
    int w, h;                    // of the picture
    int hs, vs;                  // the stream's chroma shifts
    int ky, ybase, rv, gu, gv, bu; // the conversion of include/dsv2_hip.h
    int dtype;                   // kTensor*
    float scale[3], bias[3];     // float dtypes: plane c holds fl32(fl32(byte * scale[c]) + bias[c]), rounded to the element type
};
// every plane's pointer and pitch multiples of four elements and w of 4: a thread's four samples of a row leave as one vector store
inline bool tensor_job_wide(const TensorOutJob &j)
{
    uintptr_t bits = 0;
    for (int c = 0; c < 3; c++) {
        bits |= ((uintptr_t) j.dst[c]) | (uintptr_t) j.dpitch[c];
    }
    return (bits & (uintptr_t) (4 * tensor_elem(j.dtype) - 1)) == 0 && (j.w & 3) == 0;
}
struct TensorInJob { // one picture that is three planes R, G, B of a caller's float tensor (dsv2hip_in_tensor: binary16, bfloat16 or binary32
                     // elements) on its way into the three bordered source planes: taken through the job's per-plane scale and bias, clamped and
                     // rounded to bytes, then converted as a planar RGB surface is (ingest_tensor.h, frame.hip: k_ingest_tensor); 152 bytes,
                     // fetched by value through the scalar cache like Rgb3Job, whose destination side it shares.  (A uint8 tensor is an Rgb3Job.)
    const uint8_t *src[3]; // device memory, element aligned: row y of R, G, B at src[c] + y * pitch[c], w elements of it read
    size_t pitch[3];       // bytes, multiples of the element size
    uint8_t *dst[3];       // Y, U, V planes from dframe_alloc
    int ystride, cstride;  // RgbJob's, as w, h, hs, vs and the quads
    int w, h;
    int hs, vs;
    int dtype;             // kTensorF16, kTensorBF16, kTensorF32
    uint32_t ycoef, upos, uneg, vpos, vneg; // the planar kind's: R G B in bytes 0..2 of a pixel dword
    uint32_t yoff;
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
struct ScaleOutJob { // one plane of a decoded picture on its way out at half, quarter or eighth size (dsv2hip_out_surface, DSV2HIP_SCALE_*): the box
                     // average of include/dsv2_hip.h (egress_scale.h, bmc.hip: k_egress_scale) into a plane of the caller's surface, or into the
                     // decoder's staging picture that k_egress_uv / k_egress_rgb then read; 40 bytes, fetched by value through the scalar cache
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
                      // average of include/dsv2_hip.h (egress_resize.h, bmc.hip: k_egress_resize) into a plane of the caller's surface, or into
                      // the decoder's staging picture that k_egress_uv / k_egress_rgb then read; 72 bytes, fetched by value through the scalar cache
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
void to420_batch(hipStream_t s, const To420Job *d_jobs, int n, int max_w, int max_h);
void ingest_uyvy_batch(hipStream_t s, const IngestJob *d_jobs, int n, int w, int h); // src = interleaved UYVY rows
void planes_to_host_batch(hipStream_t s, const PlaneOutJob *d_jobs, int n, int h);
void extend_planes(hipStream_t s, const DPlane *d_planes, int n, int max_w, int max_h);
void ds2x_planes4(hipStream_t s, const PlanePair *d_pairs, int n, int dst_w, int dst_h); // planes from dframe_alloc: 4 samples per thread
void copy_linear_batch(hipStream_t s, const CopyJob *d_jobs, int n, size_t max_bytes);
void zero_linear_batch(hipStream_t s, const CopyJob *d_jobs, int n, size_t max_bytes); // dst, bytes of each job
void copy_planes_batch(hipStream_t s, const PlanePair *d_pairs, int n, int w, int h);  // visible pixels, same-size planes
void ingest_batch(hipStream_t s, const IngestJob *d_jobs, int n, int w, int total_rows);
void ingest_batch16(hipStream_t s, const IngestJob *d_jobs, int n, int total_rows); // all plane widths % 16 == 0, <= 2048, 16-byte aligned sources
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
// Half, quarter and eighth-size ingest (dsv2hip_enc_batch_surface_scaled): the records of k_ingest_surface_scaled and
// k_ingest_rgb_scaled (frame.hip, ingest_scale.h), in tables of their own behind the two above.
struct ScaledSurfaceJob { // one SOURCE plane of a caller's surface, box-averaged (the decoder's REDUCTION, include/dsv2_hip.h) on its way into a
                          // bordered source plane of the reduced geometry; 56 bytes, fetched by value through the scalar cache
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch
    size_t pitch;
    uint8_t *dst, *dst2; // plane(s) from dframe_alloc; dst2 != null: the source rows are U0 V0 U1 V1 ..., reduced U goes to dst, V to dst2
    int dstride;         // of dst and dst2
    int pw, ph;          // samples per row and rows of the SOURCE plane (with dst2: U V pairs per row, the row holds 2 * pw bytes)
    int shift;           // 1, 2, 3: n = 1 << shift; the destination holds ceil(pw / n) x ceil(ph / n)
};
struct ScaledRgbJob { // one packed four-byte RGB surface, converted and reduced with one rounding per sample on its way into the three bordered
                      // source planes of the reduced geometry; 96 bytes, fetched by value through the scalar cache
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch, sw pixels of 4 bytes
    size_t pitch;
    uint8_t *dst[3];      // Y, U, V planes from dframe_alloc
    int ystride, cstride; // of dst[0]; of dst[1] and dst[2]
    int sw, sh;           // of the picture IN THE SURFACE; the encoder's is ceil(sw / n) x ceil(sh / n)
    int hs, vs;           // the stream's chroma shifts
    int shift;            // 1, 2, 3
    uint32_t ycoef, upos, uneg, vpos, vneg; // RgbJob's quads
    uint32_t yoff;                          // 128 + 256 * ybase
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
// (frame.hip, ingest_resize.h), in tables of their own behind the scaled ones.
struct SizedRatio { // pw x ph -> ow x oh, the exact area average of include/dsv2_hip.h (ResizeOutJob's arithmetic); 24 bytes
    uint16_t a, b, c, d; // pw / ow = a / b and ph / oh = c / d in lowest terms (a, c <= 32768)
    uint32_t D;          // a * c
    uint32_t rD, rb, rd; // resize_recip of the final divisor (YUV: D, RGB: 256 * D), of b, of d
};
struct SizedSurfaceJob { // one source plane -- or the U or the V half of an interleaved one -- resampled into a bordered source plane of the
                         // encoder; 64 bytes, fetched by value through the scalar cache
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch, sample i at byte off + step * i of it
    size_t pitch;
    uint8_t *dst; // plane from dframe_alloc
    int dstride;
    int ow, oh; // of dst
    SizedRatio q;
    uint16_t step, off; // 1, 0: a planar plane; 2, 0 / 2, 1: U / V of an interleaved plane
};
struct SizedRgbJob { // one packed four-byte RGB surface, resampled as RGB and converted with one rounding per sample into the three bordered
                     // source planes of the encoder; 136 bytes, fetched by value through the scalar cache
    const uint8_t *src; // device memory, any alignment: row y at src + y * pitch, pixels of 4 bytes
    size_t pitch;
    uint8_t *dst[3];      // Y, U, V planes from dframe_alloc
    int ystride, cstride; // of dst[0]; of dst[1] and dst[2]
    int ow, oh, cw, ch;   // of dst[0]; of dst[1] and dst[2]
    SizedRatio ql, qc;    // the surface's picture -> ow x oh; -> cw x ch
    uint32_t ycoef, upos, uneg, vpos, vneg; // RgbJob's quads
    uint32_t yoff;                          // 128 + 256 * ybase
};
// n jobs, the widest destination row max_ow samples, the most destination rows max_oh; wide: sized_job_wide of every job
void ingest_sized_batch(hipStream_t s, const SizedSurfaceJob *d_jobs, int n, int max_ow, int max_oh, bool wide);
// row_bytes: of the SOURCE plane's rows (an interleaved plane: of both halves together)
inline bool sized_job_wide(const SizedSurfaceJob &j, size_t row_bytes) { return ((((uintptr_t) j.src) | j.pitch | row_bytes) & 3) == 0; }
// n RGB surfaces, the widest luma row max_ow, the most luma plus chroma rows max_rows; wide: sized_rgb_job_wide of every job
void ingest_rgb_sized_batch(hipStream_t s, const SizedRgbJob *d_jobs, int n, int max_ow, int max_rows, bool wide);
inline bool sized_rgb_job_wide(const SizedRgbJob &j) { return ((((uintptr_t) j.src) | j.pitch) & 3) == 0; }

void ensure_device();
void set_default_device(int ordinal);
void bind_device(); // ensure_device + hipSetDevice(default ordinal) for the calling thread
int trace_mode();                    // DSV2_TRACE: bit 0 start-up marks, bit 1 wall-clock split of the lockstep steps (bit 2: absolute times, bit 3: every step)
void startup_mark(const char *what); // DSV2_TRACE=1
int device_status(); // 0 = usable HIP device present
bool device_arch_is(const char *prefix); // the default device's gcnArchName starts with `prefix`

} // namespace dsv2
