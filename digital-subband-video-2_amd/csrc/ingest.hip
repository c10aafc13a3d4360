// ingest.hip -- the kernels a caller's device picture enters the encoder through: pitched planar / semiplanar surfaces, packed and
// planar RGB surfaces and planar and interleaved float tensors converted on the way in, each at the encoder's size, at half / quarter / eighth size or
// at any larger size.  The records are io_jobs.h's, planned per picture by enc_ingest.h; what a thread does is in the body headers
// ingest_*.h, which the check programs under tools/ run on the CPU.  (The packed and the UYVY pictures of the host path enter
// through frame.hip.)
//
// Every kernel here fetches its record by value and pins it to scalar registers (dev.h: job_of, pin); the wavefront's row
// (64 x 4 threads: threadIdx.y is one value per wavefront) is said to be uniform the same way.
#include "io_jobs.h"
#include "ingest_rgb.h"
#include "ingest_rgb3.h"
#include "ingest_tensor.h"
#include "ingest_hwc.h"
#include "ingest_scale.h"
#include "ingest_resize.h"
#include "prio.h"

namespace dsv2 {

// ---- pitched surfaces (dsv2hip_surface): planar, or luma + one interleaved UV plane (NV12 / NV16 / NV24) ----------------
// One job per SOURCE plane (SurfaceJob, io_jobs.h), fetched by value through the scalar cache; an interleaved plane's job names
// both chroma planes.  As k_egress (egress.hip), the other way round: a thread moves VEC source bytes of FOUR consecutive rows, a
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
    // the record and the wavefront's row are the same in every lane, and said so: the row bases below are scalar, a lane adds its
    // 32-bit sx
    const SurfaceJob j = pin(job_of(tab, blockIdx.y));
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
    DSV2_LAUNCH_FORM(wide, k_ingest_surface<16>, k_ingest_surface<4>, grid, block, 0, s, d_jobs);
}

// ---- packed four-byte RGB surfaces (dsv2hip_surface, BGRA / RGBA), converted on the way in ------------------------------------
// One RgbJob per surface, fetched by value and pinned to scalar registers as above; the thread's work is ingest_rgb.h's
// ingest_rgb_rows (which tools/ingest_rgb_check.cpp runs on the CPU): 64 x 4 threads cover 16 rows -- every vertical chroma footprint,
// up to 4 rows, lies inside one thread -- and walk the row in passes of 256 pixels.
template <int VEC> __global__ __launch_bounds__(256) void k_ingest_rgb(const RgbJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const RgbJob j = pin(job_of(tab, blockIdx.y));
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
    DSV2_LAUNCH_FORM(wide, k_ingest_rgb<16>, k_ingest_rgb<4>, grid, block, 0, s, d_jobs);
}

// ---- RGB surfaces without a fourth byte (dsv2hip_surface, BGR / RGB / RGBP), converted on the way in ----------------------------
// One Rgb3Job per surface, fetched by value and pinned to scalar registers as above; the thread's work is ingest_rgb3.h's
// ingest_rgb3_rows (which tools/ingest_rgb3_check.cpp runs on the CPU), k_ingest_rgb's decomposition with another fetch.  A launch
// takes jobs of ONE kind: the packed kernels never look at src[1..2] and pitch[1..2] (null and 0 in a packed record).
template <int KIND, bool WIDE> __global__ __launch_bounds__(256) void k_ingest_rgb3(const Rgb3Job *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const Rgb3Job j = pin(job_of(tab, blockIdx.y));
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
    if (planar) {
        DSV2_LAUNCH_FORM(wide, (k_ingest_rgb3<kRgb3Planar, true>), (k_ingest_rgb3<kRgb3Planar, false>), grid, block, 0, s, d_jobs);
    } else {
        DSV2_LAUNCH_FORM(wide, (k_ingest_rgb3<kRgb3Packed, true>), (k_ingest_rgb3<kRgb3Packed, false>), grid, block, 0, s, d_jobs);
    }
}

// ---- planar RGB float tensors (dsv2hip_in_tensor: binary16, bfloat16, binary32), taken to bytes and converted on the way in -----
// One TensorInJob per picture, fetched by value and pinned to scalar registers as above -- the six constants too; the thread's work
// is ingest_tensor.h's ingest_tensor_rows (which tools/ingest_tensor_check.cpp runs on the CPU), k_ingest_rgb3's decomposition with
// another fetch.  The job's element type is uniform over the workgroup; a launch may hold jobs of all three.
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_tensor(const TensorInJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const TensorInJob j = pin(job_of(tab, blockIdx.y));
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
    DSV2_LAUNCH_FORM(wide, k_ingest_tensor<true>, k_ingest_tensor<false>, grid, block, 0, s, d_jobs);
}

// ---- interleaved RGB float tensors (dsv2hip_in_hwc: [h, w, 3] of binary16, bfloat16, binary32; R G B or B G R) --------------------
// One HwcInJob per picture, fetched by value and pinned to scalar registers as above -- the six constants too; the thread's work is
// ingest_hwc.h's ingest_hwc_rows (which tools/ingest_hwc_check.cpp runs on the CPU), k_ingest_rgb3's decomposition with another
// fetch.  Element type and order are data of the job; a launch may hold jobs of all of them.
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_hwc(const HwcInJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const HwcInJob j = pin(job_of(tab, blockIdx.y));
    const int y0 = ((int) blockIdx.x * 4 + uni((int) threadIdx.y)) * 4;
    if (y0 >= j.h) {
        return;
    }
    ingest_hwc_rows<WIDE>(j, y0, (int) threadIdx.x * 4, 64 * 4);
}

void ingest_hwc_batch(hipStream_t s, const HwcInJob *d_jobs, int n, int h, bool wide)
{
    if (n <= 0) {
        return;
    }
    const dim3 grid((h + kSurfaceRows - 1) / kSurfaceRows, n), block(64, 4);
    DSV2_LAUNCH_FORM(wide, k_ingest_hwc<true>, k_ingest_hwc<false>, grid, block, 0, s, d_jobs);
}

// ---- half, quarter and eighth-size ingest (dsv2hip_enc_batch_surface_scaled) ---------------------------------------------------
// The threads' work is ingest_scale.h's (which tools/ingest_scale_check.cpp runs on the CPU); the records are fetched by value and
// pinned to scalar registers as above.  The passes over a row are workgroups, not a loop: blockIdx.x names the 1024 source bytes
// (RGB: 256 source pixels) a wavefront takes, and the loop inside the bodies runs again only for rows beyond kScaledGridX of them.
constexpr int kScaledGridX = 64;
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_surface_scaled(const ScaledSurfaceJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const ScaledSurfaceJob j = pin(job_of(tab, blockIdx.z));
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
    DSV2_LAUNCH_FORM(wide, k_ingest_surface_scaled<true>, k_ingest_surface_scaled<false>, grid, block, 0, s, d_jobs);
}

// a wavefront: one row of chroma samples of the reduced picture over a span of 256 source pixels -- (1 << vs) strips of n source rows
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_rgb_scaled(const ScaledRgbJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const ScaledRgbJob j = pin(job_of(tab, blockIdx.z));
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
    DSV2_LAUNCH_FORM(wide, k_ingest_rgb_scaled<true>, k_ingest_rgb_scaled<false>, grid, block, 0, s, d_jobs);
}

// ---- ingest at any larger size (dsv2hip_enc_batch_surface_sized) ----------------------------------------------------------------
// The threads' work is ingest_resize.h's (which tools/ingest_resize_check.cpp runs on the CPU); the records are fetched by value and
// pinned to scalar registers as above.  A thread: four samples of one destination row; a wavefront: 256 samples of one row; the grid:
// 256-sample groups, groups of four rows, jobs -- no loop over a row or over rows.
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_sized(const SizedSurfaceJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const SizedSurfaceJob j = pin(job_of(tab, blockIdx.z));
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
    DSV2_LAUNCH_FORM(wide, k_ingest_sized<true>, k_ingest_sized<false>, grid, block, 0, s, d_jobs);
}

// grid rows 0 .. oh - 1: luma rows; oh .. oh + ch - 1: chroma rows (U and V)
template <bool WIDE> __global__ __launch_bounds__(256) void k_ingest_rgb_sized(const SizedRgbJob *__restrict__ tab)
{
    DSV2_KERNEL_PRIO();
    const SizedRgbJob j = pin(job_of(tab, blockIdx.z));
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
    DSV2_LAUNCH_FORM(wide, k_ingest_rgb_sized<true>, k_ingest_rgb_sized<false>, grid, block, 0, s, d_jobs);
}

} // namespace dsv2
