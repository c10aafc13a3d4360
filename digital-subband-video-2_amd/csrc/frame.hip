// frame.hip -- picture helpers that feed motion estimation / compensation and therefore
// the bitstream: border extension, 2x luma decimation, plane copies.
//
// Replaces reference src/frame.c: extend_plane (:358, with downsample_strip :251),
// dsv_ds2x_frame_luma (:211), dsv_frame_copy (:186).
//
// Border extension is NOT edge replication: each side strip is the rounded mean of
// groups of 4 edge pixels ((a+b+c+d+2)>>2, a trailing partial group takes a plain
// truncating mean), replicated across the 32-pixel border; corners average the two
// adjacent strip ends (frame.c:377-380).
#include "dev.h"
#include "ingest_rgb.h"
#include "ingest_rgb3.h"
#include "ingest_tensor.h"
#include "ingest_scale.h"
#include "ingest_resize.h"
#include "prio.h"

namespace dsv2 {

// mean of edge group k taken along a line of `n` pixels starting at p with pixel step `step`
__device__ __forceinline__ int strip_value(const uint8_t *p, int step, int n, int k)
{
    int full = n >> 2;
    if (k < 0) {
        return 0; // a line of fewer than 4 pixels has no last full group: the corners then take the byte in front of the reference's
                  // zero-initialised strip (frame.c:378-380, index n / 4 - 1), which is zero
    }
    if (k < full) {
        const uint8_t *q = p + (size_t) (4 * k) * step;
        return (q[0] + q[step] + q[2 * step] + q[3 * step] + 2) >> 2;
    }
    int rem = n & 3, sum = 0;
    if (rem == 0) {
        return 0; // the reference's zero-initialised strip entry past the last group
    }
    const uint8_t *q = p + (size_t) (4 * full) * step;
    for (int i = 0; i < rem; i++) {
        sum += q[i * step];
    }
    return sum / rem;
}

// One work item per 4-byte piece of border.  Roles by linear id:
//   [0, 16h)                   : row y, side, piece -> the 32-pixel runs left and right of the row
//   [.., + 64 * ngx)           : border row, side, column group -> the 32 rows above / below
//   [.., + 4 * 32 * 8)         : the four corners
__device__ __forceinline__ void put4(uint8_t *dst, int v, int n)
{
    if (n == 4 && (((uintptr_t) dst) & 3) == 0) {
        *(uint32_t *) dst = (uint32_t) v * 0x01010101u;
    } else {
        for (int i = 0; i < n; i++) {
            dst[i] = (uint8_t) v;
        }
    }
}

__device__ __forceinline__ void extend_item(const DPlane &pl, int id)
{
    uint8_t *base = pl.data;
    int stride = pl.stride, w = pl.w, h = pl.h;
    int ngx = (w + 3) >> 2;
    if (id < 16 * h) {
        int y = id >> 4, side = (id >> 3) & 1, piece = id & 7;
        int v = strip_value(side ? base + (w - 1) : base, stride, h, y >> 2);
        uint8_t *row = base + (size_t) y * stride;
        put4(side ? row + w + 4 * piece : row - kBorder + 4 * piece, v, 4);
        return;
    }
    id -= 16 * h;
    if (id < 2 * kBorder * ngx) {
        int k = id % ngx, j = (id / ngx) % kBorder, side = id / (ngx * kBorder);
        int v = strip_value(side ? base + (size_t) (h - 1) * stride : base, 1, w, k);
        uint8_t *line = side ? base + (size_t) (h + j) * stride : base - (size_t) (j + 1) * stride;
        put4(line + 4 * k, v, min(4, w - 4 * k));
        return;
    }
    id -= 2 * kBorder * ngx;
    if (id < 4 * kBorder * 8) {
        int piece = id & 7, j = (id >> 3) % kBorder, corner = id / (8 * kBorder);
        int lastx = (w >> 2) - 1, lasty = (h >> 2) - 1;
        int v;
        uint8_t *dst;
        if (corner == 0) { // top-left
            v = (strip_value(base, 1, w, 0) + strip_value(base, stride, h, 0) + 1) >> 1;
            dst = base - (size_t) (j + 1) * stride - kBorder;
        } else if (corner == 1) { // top-right
            v = (strip_value(base, 1, w, lastx) + strip_value(base + (w - 1), stride, h, 0) + 1) >> 1;
            dst = base - (size_t) (j + 1) * stride + w;
        } else if (corner == 2) { // bottom-left
            v = (strip_value(base, stride, h, lasty) + strip_value(base + (size_t) (h - 1) * stride, 1, w, 0) + 1) >> 1;
            dst = base + (size_t) (h + j) * stride - kBorder;
        } else { // bottom-right
            v = (strip_value(base + (size_t) (h - 1) * stride, 1, w, lastx) + strip_value(base + (w - 1), stride, h, lasty) + 1) >> 1;
            dst = base + (size_t) (h + j) * stride + w;
        }
        put4(dst + 4 * piece, v, 4);
    }
}

static int extend_items(int w, int h) { return 16 * h + 2 * kBorder * ((w + 3) >> 2) + 4 * kBorder * 8; }

// blockIdx.y indexes a device table of planes
__global__ __launch_bounds__(256) void k_extend(const DPlane *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const DPlane pl = job_of(tab, blockIdx.y);
    extend_item(pl, blockIdx.x * blockDim.x + threadIdx.x);
}

// n planes (device table d_planes); max_w / max_h bound the largest of them
void extend_planes(hipStream_t s, const DPlane *d_planes, int n, int max_w, int max_h)
{
    if (n <= 0) {
        return;
    }
    DSV2_LAUNCH(k_extend, dim3((extend_items(max_w, max_h) + 255) / 256, n), dim3(256), 0, s, d_planes);
}

// 2x2 rounded mean decimation of the luma plane (frame.c:211-234), four output samples per thread: two 8-byte loads (rows 2y,
// 2y + 1), byte-lane sums, one dword store.  Needs 16-byte aligned plane origins and strides (every plane made by dframe_alloc);
// the last partial group of a row goes sample by sample.
constexpr int kDsRows = 4; // output rows per thread (y, y + 4, ...): all eight 8-byte loads issued before the first average
__global__ __launch_bounds__(256) void k_ds2x4(const PlanePair *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const PlanePair pp = job_of(tab, blockIdx.z);
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int y0 = blockIdx.y * (4 * kDsRows) + threadIdx.y;
    if (x >= pp.dst.w || y0 >= pp.dst.h) {
        return;
    }
    const int sstride = pp.src.stride;
    const bool whole = x + 4 <= pp.dst.w;
    uint2 a[kDsRows], b[kDsRows];
#pragma unroll
    for (int r = 0; r < kDsRows; r++) {
        const int y = y0 + 4 * r < pp.dst.h ? y0 + 4 * r : y0;
        const uint8_t *sp = pp.src.data + (size_t) (2 * y) * sstride + 2 * x;
        a[r] = whole ? *(const uint2 *) sp : make_uint2(0u, 0u);
        b[r] = whole ? *(const uint2 *) (sp + sstride) : make_uint2(0u, 0u);
    }
#pragma unroll
    for (int r = 0; r < kDsRows; r++) {
        const int y = y0 + 4 * r;
        if (y >= pp.dst.h) {
            break;
        }
        const uint8_t *sp = pp.src.data + (size_t) (2 * y) * sstride + 2 * x;
        uint8_t *dp = pp.dst.data + (size_t) y * pp.dst.stride + x;
        if (whole) {
            const uint32_t m = 0x00ff00ffu;
            // per 32-bit word: bytes (p0 p1 p2 p3) -> 16-bit fields (p0 + p1, p2 + p3)
            uint32_t lo = (a[r].x & m) + ((a[r].x >> 8) & m) + (b[r].x & m) + ((b[r].x >> 8) & m) + 0x00020002u;
            uint32_t hi = (a[r].y & m) + ((a[r].y >> 8) & m) + (b[r].y & m) + ((b[r].y >> 8) & m) + 0x00020002u;
            lo = (lo >> 2) & m; // outputs 0, 1 in bytes 0 and 2
            hi = (hi >> 2) & m; // outputs 2, 3
            *(uint32_t *) dp = (lo & 0xffu) | ((lo >> 8) & 0xff00u) | ((hi & 0xffu) << 16) | ((hi >> 16) << 24);
        } else {
            for (int i = 0; x + i < pp.dst.w; i++) {
                const uint8_t *q = sp + 2 * i;
                dp[i] = (uint8_t) ((q[0] + q[1] + q[sstride] + q[sstride + 1] + 2) >> 2);
            }
        }
    }
}

// all planes of the table come from dframe_alloc (16-byte aligned origins and strides): four samples per thread
void ds2x_planes4(hipStream_t s, const PlanePair *d_pairs, int n, int dst_w, int dst_h)
{
    if (n <= 0) {
        return;
    }
    DSV2_LAUNCH(k_ds2x4, dim3((dst_w + 255) / 256, (dst_h + 4 * kDsRows - 1) / (4 * kDsRows), n), dim3(64, 4), 0, s, d_pairs);
}

// ---- batched copies: blockIdx.y indexes a device table --------------------------------------------
// linear copy of `bytes` (multiple of 16, 16-byte aligned both sides)
__global__ __launch_bounds__(256) void k_copy_linear(const CopyJob *__restrict__ tab)
{
    const CopyJob &j = tab[blockIdx.y];
    const uint4 *sp = (const uint4 *) j.src;
    uint4 *dp = (uint4 *) j.dst;
    size_t n = j.bytes >> 4;
    for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t) gridDim.x * 256) {
        dp[i] = sp[i];
    }
}

// zero fill of `bytes` (multiple of 16) at dst; src is ignored
__global__ __launch_bounds__(256) void k_zero_linear(const CopyJob *__restrict__ tab)
{
    const CopyJob &j = tab[blockIdx.y];
    uint4 *dp = (uint4 *) j.dst;
    size_t n = j.bytes >> 4;
    const uint4 z = {0, 0, 0, 0};
    for (size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t) gridDim.x * 256) {
        dp[i] = z;
    }
}

void zero_linear_batch(hipStream_t s, const CopyJob *d_jobs, int n, size_t max_bytes)
{
    if (n <= 0) {
        return;
    }
    size_t vecs = max_bytes >> 4;
    int gx = (int) ((vecs + 256 * 8 - 1) / (256 * 8));
    DSV2_LAUNCH(k_zero_linear, dim3(gx < 1 ? 1 : gx, n), dim3(256), 0, s, d_jobs);
}

// visible pixels of one plane to another plane of the same size (both 4-byte aligned rows)
__global__ __launch_bounds__(256) void k_copy_plane(const PlanePair *__restrict__ tab)
{
    const PlanePair &pp = tab[blockIdx.z];
    int x = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
    if (y >= pp.dst.h || x >= pp.dst.w) {
        return;
    }
    const uint8_t *sp = pp.src.data + (size_t) y * pp.src.stride + x;
    uint8_t *dp = pp.dst.data + (size_t) y * pp.dst.stride + x;
    if (x + 4 <= pp.dst.w) {
        *(uint32_t *) dp = *(const uint32_t *) sp;
    } else {
        for (int i = 0; x + i < pp.dst.w; i++) {
            dp[i] = sp[i];
        }
    }
}

void copy_planes_batch(hipStream_t s, const PlanePair *d_pairs, int n, int w, int h)
{
    if (n > 0) {
        DSV2_LAUNCH(k_copy_plane, dim3((w + 1023) / 1024, h, n), dim3(256), 0, s, d_pairs);
    }
}

void copy_linear_batch(hipStream_t s, const CopyJob *d_jobs, int n, size_t max_bytes)
{
    if (n <= 0) {
        return;
    }
    size_t vecs = max_bytes >> 4;
    int gx = (int) ((vecs + 256 * 8 - 1) / (256 * 8));
    DSV2_LAUNCH(k_copy_linear, dim3(gx < 1 ? 1 : gx, n), dim3(256), 0, s, d_jobs);
}

// packed planar picture (rows of exactly w bytes, planes back to back) -> the three padded planes
__global__ __launch_bounds__(256) void k_ingest(const IngestJob *__restrict__ tab)
{
    const IngestJob &j = tab[blockIdx.z];
    int y = blockIdx.y;
    const uint8_t *sp = j.src;
    int c = 0;
    while (c < 2 && y >= j.dst[c].h) { // plane of this row
        sp += (size_t) j.dst[c].w * j.dst[c].h;
        y -= j.dst[c].h;
        c++;
    }
    const DPlane &pl = j.dst[c];
    if (y >= pl.h) {
        return;
    }
    int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= pl.w) {
        return;
    }
    const uint8_t *srow = sp + (size_t) y * pl.w + x;
    uint8_t *drow = pl.data + (size_t) y * pl.stride + x;
    if (x + 4 <= pl.w && ((((uintptr_t) srow) | ((uintptr_t) drow)) & 3) == 0) {
        *(uint32_t *) drow = *(const uint32_t *) srow;
    } else {
        for (int i = 0; i < 4 && x + i < pl.w; i++) {
            drow[i] = srow[i];
        }
    }
}

// the same for pictures whose rows are multiples of 16 bytes in every plane (all the usual sizes): 16 bytes per thread and
// load, four rows per workgroup -- an eighth of the workgroups and a quarter of the memory instructions of k_ingest
__global__ __launch_bounds__(128) void k_ingest16(const IngestJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const IngestJob &j = tab[blockIdx.y];
    const int x = (int) threadIdx.x * 16;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int y = (int) blockIdx.x * 4 + r;
        const uint8_t *sp = j.src;
        int c = 0;
        while (c < 2 && y >= j.dst[c].h) { // plane of this row
            sp += (size_t) j.dst[c].w * j.dst[c].h;
            y -= j.dst[c].h;
            c++;
        }
        const DPlane &pl = j.dst[c];
        if (y < pl.h && x < pl.w) {
            *(uint4 *) (pl.data + (size_t) y * pl.stride + x) = *(const uint4 *) (sp + (size_t) y * pl.w + x);
        }
    }
}

// interleaved UYVY 4:2:2 picture (rows of 2 * w bytes: U0 Y0 V0 Y1 ...) -> the three padded planes; the
// de-interleave of dsv_yuv_read (dsv.c:177-205) done while the picture is ingested.  One thread per 4 luma pixels
// (8 source bytes -> 4 Y, 2 U, 2 V).
__global__ __launch_bounds__(256) void k_ingest_uyvy(const IngestJob *__restrict__ tab)
{
    const IngestJob &j = tab[blockIdx.z];
    const int y = blockIdx.y, w = j.dst[0].w;
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (y >= j.dst[0].h || x >= w) {
        return;
    }
    const uint8_t *s = j.src + (size_t) y * (size_t) (2 * w) + (size_t) 2 * x;
    uint8_t *dy = j.dst[0].data + (size_t) y * j.dst[0].stride + x;
    uint8_t *du = j.dst[1].data + (size_t) y * j.dst[1].stride + (x >> 1);
    uint8_t *dv = j.dst[2].data + (size_t) y * j.dst[2].stride + (x >> 1);
    if (x + 4 <= w && (((uintptr_t) s) & 7) == 0) {
        uint2 q = *(const uint2 *) s; // U0 Y0 V0 Y1 | U1 Y2 V1 Y3
        uint32_t yy = ((q.x >> 8) & 0xffu) | ((q.x >> 16) & 0xff00u) | ((q.y << 8) & 0xff0000u) | (q.y & 0xff000000u);
        *(uint32_t *) dy = yy; // x is a multiple of 4 and the plane origin is 16-byte aligned
        *(uint16_t *) du = (uint16_t) ((q.x & 0xffu) | ((q.y & 0xffu) << 8));
        *(uint16_t *) dv = (uint16_t) (((q.x >> 16) & 0xffu) | (((q.y >> 16) & 0xffu) << 8));
    } else {
        for (int i = 0; i < 4 && x + i < w; i += 2) { // (w is even for this format)
            du[i >> 1] = s[2 * i];
            dy[i] = s[2 * i + 1];
            dv[i >> 1] = s[2 * i + 2];
            dy[i + 1] = s[2 * i + 3];
        }
    }
}

// ---- pitched surfaces (dsv2hip_surface): planar, or luma + one interleaved UV plane (NV12 / NV16 / NV24) ----------------
// One job per SOURCE plane (SurfaceJob, dev.h), fetched by value through the scalar cache; an interleaved plane's job names
// both chroma planes.  As k_egress (bmc.hip), the other way round: a thread moves VEC source bytes of FOUR consecutive rows, a
// workgroup (64 x 4 threads) 16 rows over the whole row width, every load issued before the first store.  VEC = 16, the wide
// form: the source row's bytes, the source pointer and its pitch are multiples of 16 in every job of the launch (the host
// picks it per step); a lane's 16 interleaved bytes leave as 8 U + 8 V, two aligned 8-byte stores.  VEC = 4, the general form:
// any width, pitch and alignment -- a dword is read where it is aligned and lies whole inside the row, single bytes of the
// row otherwise (no word is touched that holds no byte of the row), and stored dword-wise (2 + 2 bytes for an interleaved
// piece) where it is whole, else byte by byte inside the plane's w x h: the border is k_extend's.
constexpr int kSurfaceRows = 16; // source rows per workgroup
constexpr uint32_t kPermEven = 0x06040200u, kPermOdd = 0x07050301u; // bytes 0, 2 / 1, 3 of (second, first) operand of v_perm_b32
template <int VEC> __global__ __launch_bounds__(256) void k_ingest_surface(const SurfaceJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    // the record and the wavefront's row (64 x 4 threads: threadIdx.y is one value per wavefront) are the same in every lane, and
    // said so: the row bases below are scalar, a lane adds its 32-bit sx
    const SurfaceJob jl = job_of(tab, blockIdx.y);
    const SurfaceJob j{uni_ptr(jl.src), ((size_t) (unsigned) uni((int) (jl.pitch >> 32)) << 32) | (unsigned) uni((int) jl.pitch), uni_ptr(jl.dst),
                       uni_ptr(jl.dst2), uni(jl.dstride), uni(jl.w), uni(jl.h)};
    const int w = j.w, h = j.h;
    const int y0 = ((int) blockIdx.x * 4 + uni((int) threadIdx.y)) * 4;
    if (y0 >= h) {
        return;
    }
    const bool uv = j.dst2 != nullptr;
    const int sbytes = uv ? 2 * w : w; // of a source row
    constexpr int NW = VEC / 4;
    for (int sx = (int) threadIdx.x * VEC; sx < sbytes; sx += 64 * VEC) {
        uint32_t v[4][NW];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = y0 + r < h ? y0 + r : h - 1; // (rows below the plane: read again from its last row, never stored)
            const uint8_t *sp = j.src + (size_t) y * j.pitch + sx;
            if constexpr (VEC == 16) {
                const uint4 q = *(const uint4 *) sp;
                v[r][0] = q.x, v[r][1] = q.y, v[r][2] = q.z, v[r][3] = q.w;
            } else if (sx + 4 <= sbytes && (((uintptr_t) sp) & 3) == 0) {
                v[r][0] = *(const uint32_t *) sp;
            } else {
                v[r][0] = 0;
                for (int i = 0; i < 4 && sx + i < sbytes; i++) {
                    v[r][0] |= (uint32_t) sp[i] << (8 * i);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (y0 + r >= h) {
                break;
            }
            const size_t row = (size_t) (y0 + r) * j.dstride;
            if (!uv) {
                uint8_t *dp = j.dst + row + sx;
                if constexpr (VEC == 16) {
                    *(uint4 *) dp = make_uint4(v[r][0], v[r][1], v[r][2], v[r][3]);
                } else if (sx + 4 <= w) {
                    *(uint32_t *) dp = v[r][0]; // (sx is a multiple of 4, the plane's origin and stride of 16)
                } else {
                    for (int i = 0; sx + i < w; i++) {
                        dp[i] = (uint8_t) (v[r][0] >> (8 * i));
                    }
                }
            } else {
                uint8_t *du = j.dst + row + (sx >> 1), *dv = j.dst2 + row + (sx >> 1);
                if constexpr (VEC == 16) {
                    *(uint2 *) du = make_uint2(__builtin_amdgcn_perm(v[r][1], v[r][0], kPermEven), __builtin_amdgcn_perm(v[r][3], v[r][2], kPermEven));
                    *(uint2 *) dv = make_uint2(__builtin_amdgcn_perm(v[r][1], v[r][0], kPermOdd), __builtin_amdgcn_perm(v[r][3], v[r][2], kPermOdd));
                } else if (sx + 4 <= sbytes) { // U0 V0 U1 V1
                    const uint32_t q = __builtin_amdgcn_perm(0u, v[r][0], 0x03010200u); // U0 U1 V0 V1
                    *(uint16_t *) du = (uint16_t) q;
                    *(uint16_t *) dv = (uint16_t) (q >> 16);
                } else { // the last U V pair of an odd-width plane
                    du[0] = (uint8_t) v[r][0];
                    dv[0] = (uint8_t) (v[r][0] >> 8);
                }
            }
        }
    }
}

void ingest_surface_batch(hipStream_t s, const SurfaceJob *d_jobs, int n, int max_h, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((max_h + kSurfaceRows - 1) / kSurfaceRows, n), block(64, 4);
    if (wide) {
        DSV2_LAUNCH(k_ingest_surface<16>, grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH(k_ingest_surface<4>, grid, block, 0, s, d_jobs);
    }
}

// ---- packed four-byte RGB surfaces (dsv2hip_surface, BGRA / RGBA), converted on the way in ------------------------------------
// One RgbJob per surface, fetched by value and pinned to scalar registers as above; the thread's work is ingest_rgb.h's
// ingest_rgb_rows (which tools/ingest_rgb_check.cpp runs on the CPU): 64 x 4 threads cover 16 rows -- every vertical chroma footprint,
// up to 4 rows, lies inside one thread -- and walk the row in passes of 256 pixels.
template <int VEC> __global__ __launch_bounds__(256) void k_ingest_rgb(const RgbJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const RgbJob jl = job_of(tab, blockIdx.y);
    const RgbJob j{uni_ptr(jl.src),
                   ((size_t) (unsigned) uni((int) (jl.pitch >> 32)) << 32) | (unsigned) uni((int) jl.pitch),
                   {uni_ptr(jl.dst[0]), uni_ptr(jl.dst[1]), uni_ptr(jl.dst[2])},
                   uni(jl.ystride),
                   uni(jl.cstride),
                   uni(jl.w),
                   uni(jl.h),
                   uni(jl.hs),
                   uni(jl.vs),
                   (uint32_t) uni((int) jl.ycoef),
                   (uint32_t) uni((int) jl.upos),
                   (uint32_t) uni((int) jl.uneg),
                   (uint32_t) uni((int) jl.vpos),
                   (uint32_t) uni((int) jl.vneg),
                   (uint32_t) uni((int) jl.yoff)};
    const int y0 = ((int) blockIdx.x * 4 + uni((int) threadIdx.y)) * 4;
    if (y0 >= j.h) {
        return;
    }
    ingest_rgb_rows<VEC>(j, y0, (int) threadIdx.x * 4, 64 * 4);
}

void ingest_rgb_batch(hipStream_t s, const RgbJob *d_jobs, int n, int h, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((h + kSurfaceRows - 1) / kSurfaceRows, n), block(64, 4);
    if (wide) {
        DSV2_LAUNCH(k_ingest_rgb<16>, grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH(k_ingest_rgb<4>, grid, block, 0, s, d_jobs);
    }
}

// ---- RGB surfaces without a fourth byte (dsv2hip_surface, BGR / RGB / RGBP), converted on the way in ----------------------------
// One Rgb3Job per surface, fetched by value and pinned to scalar registers as above; the thread's work is ingest_rgb3.h's
// ingest_rgb3_rows (which tools/ingest_rgb3_check.cpp runs on the CPU), k_ingest_rgb's decomposition with another fetch.  A launch
// takes jobs of ONE kind: the packed kernels never look at src[1..2] and pitch[1..2].
template <int KIND, bool WIDE> __global__ __launch_bounds__(256) void k_ingest_rgb3(const Rgb3Job *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const Rgb3Job jl = job_of(tab, blockIdx.y);
    constexpr bool PLANAR = KIND == kRgb3Planar;
    const auto uni_pitch = [](size_t p) { return ((size_t) (unsigned) uni((int) (p >> 32)) << 32) | (unsigned) uni((int) p); };
    const Rgb3Job j{{uni_ptr(jl.src[0]), PLANAR ? uni_ptr(jl.src[1]) : nullptr, PLANAR ? uni_ptr(jl.src[2]) : nullptr},
                    {uni_pitch(jl.pitch[0]), PLANAR ? uni_pitch(jl.pitch[1]) : 0, PLANAR ? uni_pitch(jl.pitch[2]) : 0},
                    {uni_ptr(jl.dst[0]), uni_ptr(jl.dst[1]), uni_ptr(jl.dst[2])},
                    uni(jl.ystride),
                    uni(jl.cstride),
                    uni(jl.w),
                    uni(jl.h),
                    uni(jl.hs),
                    uni(jl.vs),
                    KIND,
                    (uint32_t) uni((int) jl.ycoef),
                    (uint32_t) uni((int) jl.upos),
                    (uint32_t) uni((int) jl.uneg),
                    (uint32_t) uni((int) jl.vpos),
                    (uint32_t) uni((int) jl.vneg),
                    (uint32_t) uni((int) jl.yoff)};
    const int y0 = ((int) blockIdx.x * 4 + uni((int) threadIdx.y)) * 4;
    if (y0 >= j.h) {
        return;
    }
    ingest_rgb3_rows<KIND, WIDE>(j, y0, (int) threadIdx.x * 4, 64 * 4);
}

void ingest_rgb3_batch(hipStream_t s, const Rgb3Job *d_jobs, int n, int h, bool planar, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((h + kSurfaceRows - 1) / kSurfaceRows, n), block(64, 4);
    if (planar && wide) {
        DSV2_LAUNCH((k_ingest_rgb3<kRgb3Planar, true>), grid, block, 0, s, d_jobs);
    } else if (planar) {
        DSV2_LAUNCH((k_ingest_rgb3<kRgb3Planar, false>), grid, block, 0, s, d_jobs);
    } else if (wide) {
        DSV2_LAUNCH((k_ingest_rgb3<kRgb3Packed, true>), grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH((k_ingest_rgb3<kRgb3Packed, false>), grid, block, 0, s, d_jobs);
    }
}

// ---- planar RGB float tensors (dsv2hip_in_tensor: binary16, bfloat16, binary32), taken to bytes and converted on the way in -----
// One TensorInJob per picture, fetched by value and pinned to scalar registers as above -- the six constants too; the thread's work
// is ingest_tensor.h's ingest_tensor_rows (which tools/ingest_tensor_check.cpp runs on the CPU), k_ingest_rgb3's decomposition with
// another fetch.  The job's element type is uniform over the workgroup; a launch may hold jobs of all three.
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_tensor(const TensorInJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const TensorInJob jl = job_of(tab, blockIdx.y);
    const auto uni_pitch = [](size_t p) { return ((size_t) (unsigned) uni((int) (p >> 32)) << 32) | (unsigned) uni((int) p); };
    const TensorInJob j{{uni_ptr(jl.src[0]), uni_ptr(jl.src[1]), uni_ptr(jl.src[2])},
                        {uni_pitch(jl.pitch[0]), uni_pitch(jl.pitch[1]), uni_pitch(jl.pitch[2])},
                        {uni_ptr(jl.dst[0]), uni_ptr(jl.dst[1]), uni_ptr(jl.dst[2])},
                        uni(jl.ystride),
                        uni(jl.cstride),
                        uni(jl.w),
                        uni(jl.h),
                        uni(jl.hs),
                        uni(jl.vs),
                        uni(jl.dtype),
                        (uint32_t) uni((int) jl.ycoef),
                        (uint32_t) uni((int) jl.upos),
                        (uint32_t) uni((int) jl.uneg),
                        (uint32_t) uni((int) jl.vpos),
                        (uint32_t) uni((int) jl.vneg),
                        (uint32_t) uni((int) jl.yoff),
                        {uni(jl.scale[0]), uni(jl.scale[1]), uni(jl.scale[2])},
                        {uni(jl.bias[0]), uni(jl.bias[1]), uni(jl.bias[2])}};
    const int y0 = ((int) blockIdx.x * 4 + uni((int) threadIdx.y)) * 4;
    if (y0 >= j.h) {
        return;
    }
    ingest_tensor_rows<WIDE>(j, y0, (int) threadIdx.x * 4, 64 * 4);
}

void ingest_tensor_batch(hipStream_t s, const TensorInJob *d_jobs, int n, int h, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((h + kSurfaceRows - 1) / kSurfaceRows, n), block(64, 4);
    if (wide) {
        DSV2_LAUNCH(k_ingest_tensor<true>, grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH(k_ingest_tensor<false>, grid, block, 0, s, d_jobs);
    }
}

// ---- half, quarter and eighth-size ingest (dsv2hip_enc_batch_surface_scaled) ---------------------------------------------------
// The threads' work is ingest_scale.h's (which tools/ingest_scale_check.cpp runs on the CPU); the records are fetched by value and
// pinned to scalar registers as above.  The passes over a row are workgroups, not a loop: blockIdx.x names the 1024 source bytes
// (RGB: 256 source pixels) a wavefront takes, and the loop inside the bodies runs again only for rows beyond kScaledGridX of them.
constexpr int kScaledGridX = 64;
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_surface_scaled(const ScaledSurfaceJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const ScaledSurfaceJob jl = job_of(tab, blockIdx.z);
    const ScaledSurfaceJob j{uni_ptr(jl.src), ((size_t) (unsigned) uni((int) (jl.pitch >> 32)) << 32) | (unsigned) uni((int) jl.pitch), uni_ptr(jl.dst),
                             uni_ptr(jl.dst2), uni(jl.dstride), uni(jl.pw), uni(jl.ph), uni(jl.shift)};
    const int oy = (int) blockIdx.y * 4 + uni((int) threadIdx.y); // one output row per wavefront
    if (oy >= (j.ph + (1 << j.shift) - 1) >> j.shift) {
        return;
    }
    ingest_scaled_row<WIDE>(j, oy, (int) blockIdx.x * 64 + (int) threadIdx.x, (int) gridDim.x * 64);
}

void ingest_surface_scaled_batch(hipStream_t s, const ScaledSurfaceJob *d_jobs, int n, int max_row_bytes, int max_rows, bool wide)
{
    if (n <= 0) {
        return;
    }
    const int gx = (max_row_bytes + 1023) / 1024;
    const dim3 grid(gx < kScaledGridX ? gx : kScaledGridX, (max_rows + 3) / 4, n), block(64, 4);
    if (wide) {
        DSV2_LAUNCH(k_ingest_surface_scaled<true>, grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH(k_ingest_surface_scaled<false>, grid, block, 0, s, d_jobs);
    }
}

// a wavefront: one row of chroma samples of the reduced picture over a span of 256 source pixels -- (1 << vs) strips of n source rows
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_rgb_scaled(const ScaledRgbJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const ScaledRgbJob jl = job_of(tab, blockIdx.z);
    const ScaledRgbJob j{uni_ptr(jl.src),
                         ((size_t) (unsigned) uni((int) (jl.pitch >> 32)) << 32) | (unsigned) uni((int) jl.pitch),
                         {uni_ptr(jl.dst[0]), uni_ptr(jl.dst[1]), uni_ptr(jl.dst[2])},
                         uni(jl.ystride),
                         uni(jl.cstride),
                         uni(jl.sw),
                         uni(jl.sh),
                         uni(jl.hs),
                         uni(jl.vs),
                         uni(jl.shift),
                         (uint32_t) uni((int) jl.ycoef),
                         (uint32_t) uni((int) jl.upos),
                         (uint32_t) uni((int) jl.uneg),
                         (uint32_t) uni((int) jl.vpos),
                         (uint32_t) uni((int) jl.vneg),
                         (uint32_t) uni((int) jl.yoff)};
    const int cy = (int) blockIdx.y * 4 + uni((int) threadIdx.y);
    const int up = (1 << (j.shift + j.vs)) - 1;
    if (cy >= (j.sh + up) >> (j.shift + j.vs)) { // (= ch' of the reduced picture; the whole wavefront leaves or stays)
        return;
    }
    ingest_rgb_scaled_band<WIDE>(j, cy, (int) blockIdx.x * kRgbScaledSpan, (int) gridDim.x * kRgbScaledSpan);
}

void ingest_rgb_scaled_batch(hipStream_t s, const ScaledRgbJob *d_jobs, int n, int max_sw, int max_crows, bool wide)
{
    if (n <= 0) {
        return;
    }
    const int gx = (max_sw + kRgbScaledSpan - 1) / kRgbScaledSpan;
    const dim3 grid(gx < kScaledGridX ? gx : kScaledGridX, (max_crows + 3) / 4, n), block(64, 4);
    if (wide) {
        DSV2_LAUNCH(k_ingest_rgb_scaled<true>, grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH(k_ingest_rgb_scaled<false>, grid, block, 0, s, d_jobs);
    }
}

// ---- ingest at any larger size (dsv2hip_enc_batch_surface_sized) ----------------------------------------------------------------
// The threads' work is ingest_resize.h's (which tools/ingest_resize_check.cpp runs on the CPU); the records are fetched by value and
// pinned to scalar registers as above.  A thread: four samples of one destination row; a wavefront: 256 samples of one row; the grid:
// 256-sample groups, groups of four rows, jobs -- no loop over a row or over rows.
__device__ __forceinline__ SizedRatio uni_ratio(const SizedRatio &q)
{
    return SizedRatio{(uint16_t) uni((int) q.a), (uint16_t) uni((int) q.b), (uint16_t) uni((int) q.c), (uint16_t) uni((int) q.d),
                      (uint32_t) uni((int) q.D), (uint32_t) uni((int) q.rD), (uint32_t) uni((int) q.rb), (uint32_t) uni((int) q.rd)};
}

template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_sized(const SizedSurfaceJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const SizedSurfaceJob jl = job_of(tab, blockIdx.z);
    const SizedSurfaceJob j{uni_ptr(jl.src), ((size_t) (unsigned) uni((int) (jl.pitch >> 32)) << 32) | (unsigned) uni((int) jl.pitch), uni_ptr(jl.dst),
                            uni(jl.dstride), uni(jl.ow), uni(jl.oh), uni_ratio(jl.q), (uint16_t) uni((int) jl.step), (uint16_t) uni((int) jl.off)};
    const int y = (int) blockIdx.y * 4 + uni((int) threadIdx.y); // one destination row per wavefront
    const int x0 = ((int) blockIdx.x * 64 + (int) threadIdx.x) * 4;
    if (y >= j.oh || x0 >= j.ow) {
        return;
    }
    ingest_sized_quad<WIDE>(j, y, x0);
}

void ingest_sized_batch(hipStream_t s, const SizedSurfaceJob *d_jobs, int n, int max_ow, int max_oh, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((max_ow + 255) / 256, (max_oh + 3) / 4, n), block(64, 4);
    if (wide) {
        DSV2_LAUNCH(k_ingest_sized<true>, grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH(k_ingest_sized<false>, grid, block, 0, s, d_jobs);
    }
}

// grid rows 0 .. oh - 1: luma rows; oh .. oh + ch - 1: chroma rows (U and V)
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_rgb_sized(const SizedRgbJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const SizedRgbJob jl = job_of(tab, blockIdx.z);
    const SizedRgbJob j{uni_ptr(jl.src),
                        ((size_t) (unsigned) uni((int) (jl.pitch >> 32)) << 32) | (unsigned) uni((int) jl.pitch),
                        {uni_ptr(jl.dst[0]), uni_ptr(jl.dst[1]), uni_ptr(jl.dst[2])},
                        uni(jl.ystride),
                        uni(jl.cstride),
                        uni(jl.ow),
                        uni(jl.oh),
                        uni(jl.cw),
                        uni(jl.ch),
                        uni_ratio(jl.ql),
                        uni_ratio(jl.qc),
                        (uint32_t) uni((int) jl.ycoef),
                        (uint32_t) uni((int) jl.upos),
                        (uint32_t) uni((int) jl.uneg),
                        (uint32_t) uni((int) jl.vpos),
                        (uint32_t) uni((int) jl.vneg),
                        (uint32_t) uni((int) jl.yoff)};
    const int gy = (int) blockIdx.y * 4 + uni((int) threadIdx.y);
    const int x0 = ((int) blockIdx.x * 64 + (int) threadIdx.x) * 4;
    if (gy >= j.oh + j.ch || x0 >= (gy < j.oh ? j.ow : j.cw)) {
        return;
    }
    ingest_sized_rgb_quad<WIDE>(j, gy, x0);
}

void ingest_rgb_sized_batch(hipStream_t s, const SizedRgbJob *d_jobs, int n, int max_ow, int max_rows, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((max_ow + 255) / 256, (max_rows + 3) / 4, n), block(64, 4);
    if (wide) {
        DSV2_LAUNCH(k_ingest_rgb_sized<true>, grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH(k_ingest_rgb_sized<false>, grid, block, 0, s, d_jobs);
    }
}

// ---- decoder egress: chroma planes of a decoded picture converted to 4:2:0 -----------------------------------
// util.c:79-153 of the reference CLI (-out420p): 4:4:4 -> 4:2:2 -> 4:2:0 (two rounded pair averages, the second
// operand clamped at the plane edge), 4:2:2 -> 4:2:0, 4:1:1 -> 4:2:0, 4:1:0 -> 4:2:0; one thread per output sample,
// both steps of the 4:4:4 chain fused (the intermediate 4:2:2 sample is recomputed, never stored).
__device__ __forceinline__ int px(const DPlane &p, int x, int y) { return p.data[(size_t) y * p.stride + x]; }

__global__ __launch_bounds__(256) void k_to420(const To420Job *__restrict__ tab)
{
    const To420Job &j = tab[blockIdx.z];
    const DPlane &s = j.src, &d = j.dst;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= d.w || y >= d.h) {
        return;
    }
    int v;
    if (j.mode == 0) { // luma (and chroma that is 4:2:0 already): copy
        v = px(s, x, y);
    } else if (j.mode == 1) { // 4:4:4: conv444to422 then conv422to420
        int x0 = 2 * x, x1 = x0 < s.w - 1 ? x0 + 1 : s.w - 1;
        int y0 = 2 * y, y1 = y0 < s.h - 1 ? y0 + 1 : s.h - 1;
        int a = (px(s, x0, y0) + px(s, x1, y0) + 1) >> 1, b = (px(s, x0, y1) + px(s, x1, y1) + 1) >> 1;
        v = (a + b + 1) >> 1;
    } else if (j.mode == 2) { // 4:2:2: conv422to420
        int y0 = 2 * y, y1 = y0 < s.h - 1 ? y0 + 1 : s.h - 1;
        v = (px(s, x, y0) + px(s, x, y1) + 1) >> 1;
    } else if (j.mode == 3) { // 4:1:1: conv411to420
        int y0 = 2 * y, y1 = y0 < s.h - 1 ? y0 + 1 : s.h - 1;
        int sx = min(x >> 1, s.w - 1);
        v = (px(s, sx, y0) + px(s, sx, y1) + 1) >> 1;
    } else { // "4:1:0": conv410to420
        v = px(s, min(x >> 1, s.w - 1), min(y >> 1, s.h - 1));
    }
    d.data[(size_t) y * d.stride + x] = (uint8_t) v;
}

// small planes (the coarsest pyramid level) packed row after row into pinned host memory
__global__ __launch_bounds__(64) void k_plane_to_host(const PlaneOutJob *__restrict__ tab)
{
    const PlaneOutJob &j = tab[blockIdx.y];
    int y = blockIdx.x;
    if (y >= j.src.h) {
        return;
    }
    for (int x = threadIdx.x; x < j.src.w; x += 64) {
        j.dst[(size_t) y * j.src.w + x] = j.src.data[(size_t) y * j.src.stride + x];
    }
}

void planes_to_host_batch(hipStream_t s, const PlaneOutJob *d_jobs, int n, int h)
{
    if (n > 0) {
        DSV2_LAUNCH(k_plane_to_host, dim3(h, n), dim3(64), 0, s, d_jobs);
    }
}

void ingest_batch(hipStream_t s, const IngestJob *d_jobs, int n, int w, int total_rows)
{
    if (n <= 0) {
        return;
    }
    DSV2_LAUNCH(k_ingest, dim3((w + 1023) / 1024, total_rows, n), dim3(256), 0, s, d_jobs);
}

// every plane's width a multiple of 16 (and at most 2048), sources 16-byte aligned: the wide form
void ingest_batch16(hipStream_t s, const IngestJob *d_jobs, int n, int total_rows)
{
    if (n <= 0) {
        return;
    }
    DSV2_LAUNCH(k_ingest16, dim3((total_rows + 3) / 4, n), dim3(128), 0, s, d_jobs);
}

void ingest_uyvy_batch(hipStream_t s, const IngestJob *d_jobs, int n, int w, int h)
{
    if (n <= 0) {
        return;
    }
    DSV2_LAUNCH(k_ingest_uyvy, dim3((w + 1023) / 1024, h, n), dim3(256), 0, s, d_jobs);
}

void to420_batch(hipStream_t s, const To420Job *d_jobs, int n, int max_w, int max_h)
{
    if (n <= 0) {
        return;
    }
    DSV2_LAUNCH(k_to420, dim3((max_w + 255) / 256, max_h, n), dim3(256), 0, s, d_jobs);
}

} // namespace dsv2
