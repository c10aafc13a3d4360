// egress.hip -- the kernels a decoded picture leaves the decoder through: the visible pixels of the reconstruction into the picture
// the caller receives (sharpened on the way under -postsharp), chroma interleaved into a semiplanar surface, RGB surfaces and
// tensors converted on the way out, planes at half / quarter / eighth size or at a size the caller names.  The records are
// io_jobs.h's, planned per picture by dec_delivery.h; what a thread does is in the body headers egress_*.h, which the check programs
// under tools/ run on the CPU.  (The 4:2:0 conversion into a host frame is frame.hip's k_to420, the sharpening in place bmc.hip's
// k_post_process.)
#include "io_jobs.h"
#include "degrad.h"
#include "egress_rgb.h"
#include "egress_resize.h"
#include "egress_scale.h"
#include "egress_uv.h"
#include "prio.h"

namespace dsv2 {

// ---- decoder egress: visible pixels of a reconstruction plane into the picture the caller receives ---------------------
// One job per plane (EgressJob, io_jobs.h), fetched by value through the scalar cache.  A thread moves VEC bytes of FOUR
// consecutive rows -- one row of 4x4 cells -- and a workgroup (64 x 4 threads) 16 rows of the plane, every load issued before
// the first store.  VEC = 16, the wide form: the plane's width a multiple of 16, destination and its stride 16-byte aligned
// (the host picks it per round); VEC = 4, the general form: any width, any destination alignment -- whole dwords are read
// from the source (its 32-pixel border covers the up to three bytes past the row), the destination is written dword-wise
// only where the dword is whole and aligned, else byte by byte inside the row: nothing outside [dst, dst + h * dstride) row
// pieces of w bytes is ever touched.  With `sharp` (luma under dsv2hip_dec_set_postsharp) each cell the reference's
// dsv_post_process visits -- x + 4 < w and y + 4 < h (bmc.c:350,355) -- goes through degrad16 in registers on the way: the
// cells are independent and read only their own 16 samples, so this equals the in-place pass over the delivered plane, and
// the reconstruction the next P picture predicts from stays unsharpened.  SHARP = false is the kernel of rounds without
// such a job: the copy alone, a third of the registers.
constexpr int kEgressRows = 16; // plane rows per workgroup
template <int VEC, bool SHARP> __global__ __launch_bounds__(256) void k_egress(const EgressJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const EgressJob j = job_of(tab, blockIdx.y);
    const int w = j.src.w, h = j.src.h;
    const int y0 = ((int) blockIdx.x * 4 + (int) threadIdx.y) * 4;
    if (y0 >= h) {
        return;
    }
    constexpr int NW = VEC / 4;
    const bool sharp_row = SHARP && j.sharp && y0 + 4 < h;
    for (int x = (int) threadIdx.x * VEC; x < w; x += 64 * VEC) {
        uint32_t v[4][NW];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = y0 + r < h ? y0 + r : h - 1; // (rows below the plane: read again from its last row, never stored)
            const uint8_t *sp = j.src.data + (size_t) y * j.src.stride + x;
            if constexpr (VEC == 16) {
                const uint4 q = *(const uint4 *) sp;
                v[r][0] = q.x, v[r][1] = q.y, v[r][2] = q.z, v[r][3] = q.w;
            } else {
                v[r][0] = *(const uint32_t *) sp;
            }
        }
        if (sharp_row) {
#pragma unroll
            for (int k = 0; k < NW; k++) {
                if (x + 4 * k + 4 < w) {
                    int px[16];
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        px[i] = (int) ((v[i >> 2][k] >> (8 * (i & 3))) & 0xffu);
                    }
                    if (degrad16(px)) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            v[r][k] = (uint32_t) px[4 * r] | ((uint32_t) px[4 * r + 1] << 8) | ((uint32_t) px[4 * r + 2] << 16) |
                                      ((uint32_t) px[4 * r + 3] << 24);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (y0 + r >= h) {
                break;
            }
            uint8_t *dp = j.dst + (size_t) (y0 + r) * j.dstride + x;
            if constexpr (VEC == 16) {
                *(uint4 *) dp = make_uint4(v[r][0], v[r][1], v[r][2], v[r][3]);
            } else {
                if (x + 4 <= w && (((uintptr_t) dp) & 3) == 0) {
                    *(uint32_t *) dp = v[r][0];
                } else {
                    for (int i = 0; i < 4 && x + i < w; i++) {
                        dp[i] = (uint8_t) (v[r][0] >> (8 * i));
                    }
                }
            }
        }
    }
}

void egress_batch(hipStream_t s, const EgressJob *d_jobs, int n, int max_h, bool wide, bool any_sharp)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((max_h + kEgressRows - 1) / kEgressRows, n), block(64, 4);
    if (any_sharp) {
        DSV2_LAUNCH_FORM(wide, (k_egress<16, true>), (k_egress<4, true>), grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH_FORM(wide, (k_egress<16, false>), (k_egress<4, false>), grid, block, 0, s, d_jobs);
    }
}

// ---- decoder egress into a semiplanar surface: U and V of a decoded picture interleaved into one plane ---------------------
// One job per picture (UvEgressJob, io_jobs.h), fetched by value through the scalar cache.  k_egress's shape: a workgroup (64 x 4
// threads) covers 16 rows of the delivered chroma, a thread VEC (U, V) pairs of four consecutive rows, all loads before the
// first store.  What a thread does -- both forms, the fused -out420p conversions, the bounds argument -- is egress_uv.h.
template <int VEC, bool CONV> __global__ __launch_bounds__(256) void k_egress_uv(const UvEgressJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const UvEgressJob j = job_of(tab, blockIdx.y);
    const int y0 = ((int) blockIdx.x * 4 + (int) threadIdx.y) * 4;
    if (y0 >= j.ch) {
        return;
    }
    egress_uv_rows<VEC, CONV>(j, y0, (int) threadIdx.x * VEC, 64 * VEC);
}

void egress_uv_batch(hipStream_t s, const UvEgressJob *d_jobs, int n, int max_ch, bool wide, bool any_conv)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((max_ch + kEgressRows - 1) / kEgressRows, n), block(64, 4);
    if (any_conv) {
        DSV2_LAUNCH_FORM(wide, (k_egress_uv<8, true>), (k_egress_uv<4, true>), grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH_FORM(wide, (k_egress_uv<8, false>), (k_egress_uv<4, false>), grid, block, 0, s, d_jobs);
    }
}

// ---- decoder egress as RGB, converted on the way out: packed four-byte surfaces (BGRA / RGBA), planar or interleaved tensors -------------
// One job per picture (RgbOutJob, io_jobs.h), fetched by value and pinned to scalar registers (dev.h: job_of, pin) as k_ingest_rgb
// (ingest.hip) does, whose shape this mirrors: 64 x 4 threads cover 16 rows -- every vertical chroma footprint, up to 4 rows, lies
// inside one thread -- and walk the row in passes of 256 pixels.  The thread's work is egress_rgb.h's egress_rgb_rows (which
// tools/egress_rgb_check.cpp runs on the CPU); the layout is the kernel's, the job's element type is uniform over the workgroup.
template <int LAYOUT, bool WIDE> __global__ __launch_bounds__(256) void k_egress_rgb(const RgbOutJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const RgbOutJob j = pin(job_of(tab, blockIdx.y));
    const int y0 = ((int) blockIdx.x * 4 + uni((int) threadIdx.y)) * 4;
    if (y0 >= j.h) {
        return;
    }
    egress_rgb_rows<LAYOUT, WIDE>(j, y0, (int) threadIdx.x * 4, 64 * 4);
}

template <int LAYOUT> static void egress_rgb_launch(hipStream_t s, const RgbOutJob *d_jobs, int n, int h, bool wide)
{
    const dim3 grid((h + kEgressRows - 1) / kEgressRows, n), block(64, 4);
    DSV2_LAUNCH_FORM(wide, (k_egress_rgb<LAYOUT, true>), (k_egress_rgb<LAYOUT, false>), grid, block, 0, s, d_jobs);
}

void egress_rgb_batch(hipStream_t s, const RgbOutJob *d_jobs, int n, int h, int layout, bool wide)
{
    if (n <= 0) {
        return;
    }
    if (layout == kRgbOutPacked) {
        egress_rgb_launch<kRgbOutPacked>(s, d_jobs, n, h, wide);
    } else if (layout == kRgbOutPlanar) {
        egress_rgb_launch<kRgbOutPlanar>(s, d_jobs, n, h, wide);
    } else {
        egress_rgb_launch<kRgbOutInterleaved>(s, d_jobs, n, h, wide);
    }
}

// ---- decoder egress at half, quarter or eighth size: the box average of include/dsv2_hip.h ------------------------------------------
// One job per plane (ScaleOutJob, io_jobs.h), fetched by value and pinned to scalar registers as above.  A workgroup of 8 x 32 threads
// covers 32 OUTPUT rows, a thread one output row: it walks the source rows of its footprint in passes of 8 x 16 = 128 source bytes,
// so a wavefront's load is eight whole 128-byte lines, one per output row.  The thread's work is egress_scale.h's egress_scale_row
// (which tools/egress_scale_check.cpp runs on the CPU).
constexpr int kScaleRows = 32, kScaleLanes = 8; // output rows per workgroup; threads along a row
template <bool WIDE> __global__ __launch_bounds__(256) void k_egress_scale(const ScaleOutJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const ScaleOutJob j = pin(job_of(tab, blockIdx.y));
    const int oy0 = uni((int) blockIdx.x * kScaleRows);
    if (oy0 + (int) threadIdx.y >= (j.ph + (1 << j.shift) - 1) >> j.shift) {
        return;
    }
    egress_scale_row<WIDE>(j, oy0, (int) threadIdx.y, (int) threadIdx.x, kScaleLanes);
}

void egress_scale_batch(hipStream_t s, const ScaleOutJob *d_jobs, int n, int max_oh, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((max_oh + kScaleRows - 1) / kScaleRows, n), block(kScaleLanes, kScaleRows);
    DSV2_LAUNCH_FORM(wide, k_egress_scale<true>, k_egress_scale<false>, grid, block, 0, s, d_jobs);
}

// ---- decoder egress at a size the caller names: the exact area average of include/dsv2_hip.h ------------------------------------------
// One job per plane (ResizeOutJob, io_jobs.h), fetched by value and pinned to scalar registers as above.  A workgroup of 64 x 4 threads
// covers 256 samples of 4 OUTPUT rows, a thread four samples of one row, and the grid covers the largest plane of the launch: no loop
// over a row or over rows.  The thread's work is egress_resize.h's egress_resize_quad (which tools/egress_resize_check.cpp runs on the
// CPU).
constexpr int kResizeRows = 4, kResizeLanes = 64; // output rows per workgroup; threads along a row, four samples each
template <bool WIDE> __global__ __launch_bounds__(256) void k_egress_resize(const ResizeOutJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const ResizeOutJob j = pin(job_of(tab, blockIdx.y));
    const int y = (int) blockIdx.x * kResizeRows + (int) threadIdx.y;
    const int x0 = 4 * ((int) blockIdx.z * kResizeLanes + (int) threadIdx.x);
    if (y >= j.oh || x0 >= j.ow) {
        return;
    }
    egress_resize_quad<WIDE>(j, y, x0);
}

void egress_resize_batch(hipStream_t s, const ResizeOutJob *d_jobs, int n, int max_ow, int max_oh, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((max_oh + kResizeRows - 1) / kResizeRows, n, (max_ow + 4 * kResizeLanes - 1) / (4 * kResizeLanes)), block(kResizeLanes, kResizeRows);
    DSV2_LAUNCH_FORM(wide, k_egress_resize<true>, k_egress_resize<false>, grid, block, 0, s, d_jobs);
}

} // namespace dsv2
