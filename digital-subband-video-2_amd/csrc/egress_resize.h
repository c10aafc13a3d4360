// egress_resize.h -- what one thread of k_egress_resize (egress.hip) does, as a function that also compiles for the host (the pattern of
// egress_scale.h): the kernel is this function behind blockIdx / threadIdx, and tools/egress_resize_check.cpp sweeps the very same
// code on the CPU under AddressSanitizer -- ratios, forms, pitches and offsets -- before it runs on a GPU.
//
// One ResizeOutJob (io_jobs.h) = one plane of a decoded picture on its way out at a size the caller names.  A plane of pw x ph becomes
// ow x oh by the exact area average of include/dsv2_hip.h: with pw / ow = a / b and ph / oh = c / d in lowest terms, source pixel i
// covers [i*b, (i+1)*b), output sample x covers [x*a, (x+1)*a), wx(x, i) is the length of their overlap (and wy(y, j) likewise), and
//   out(x, y) = (SUM j SUM i  wy(y,j) * wx(x,i) * P(i, j)  +  D / 2) / D,   D = a * c
// one rounding, an exact integer division.  The last sample's interval ends at pw * b: no coordinate outside the plane exists in the
// formula, and none is read -- byte loads, no vector that could reach past a row.
// A thread owns four consecutive samples of ONE output row, and there is no loop over a row or over rows: the grid has a workgroup
// for every 256 samples of a row and every 4 rows (the finding of DESIGN 5.14).  It walks the source rows its sample rows overlap
// (at most 9) and, for each sample, the source pixels that overlap it (at most 9); the horizontal sum of one source row is at most
// 255 * a, the whole sum at most 255 * D + D / 2 < 2^32 for D <= 2^24.  The three quotients a thread needs -- its first source row,
// its samples' first source pixels, the final one by D -- are a multiply-high by a reciprocal the host computed and one correction
// (resize_div), exact for every 32-bit numerator.
//   WIDE:    destination pointer and pitch multiples of 4 and the row writable up to a multiple of 4 bytes in every job of the launch
//            (a caller's plane: ow such a multiple; the staging picture: always) -- the host picks it per round, resize_job_wide:
//            one unconditional dword store.  Samples from ow on (the staging picture's slack) repeat sample ow - 1.
//   general: any ow, pitch and alignment.  The four samples go out as one dword where they lie whole inside the row at an address
//            that is a multiple of 4, else byte by byte where x < ow -- no byte outside the oh row pieces of ow bytes is ever written.
#pragma once

#include "ingest_rgb.h" // ld_global, st_global

namespace dsv2 {

__host__ __device__ __forceinline__ uint32_t mulhi_u32(uint32_t x, uint32_t y)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(x, y);
#else
    return (uint32_t) (((uint64_t) x * (uint64_t) y) >> 32);
#endif
}
// n / den for any 32-bit n, with r = resize_recip(den) (io_jobs.h): n * r / 2^32 lies below n / den by less than n / 2^32 < 1, so its
// integer part is the quotient or one less
__host__ __device__ __forceinline__ uint32_t resize_div(uint32_t n, uint32_t den, uint32_t r)
{
    const uint32_t q = mulhi_u32(n, r);
    return q + (n - q * den >= den ? 1u : 0u);
}

// samples x0 .. x0 + 3 (x0 a multiple of 4, below ow) of output row y (below oh) of job j
template <bool WIDE> __host__ __device__ __forceinline__ void egress_resize_quad(const ResizeOutJob &j, int y, int x0)
{
    const uint32_t a = (uint32_t) j.a, b = (uint32_t) j.b, c = (uint32_t) j.c, d = (uint32_t) j.d;
    const int ow = j.ow;
    const uint32_t ys = (uint32_t) y * c, ye = ys + c; // the sample row's interval, in units of 1 / d of a source row
    const uint32_t j0 = resize_div(ys, d, j.rd);
    uint32_t xs[4], i0[4], acc[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = x0 + k < ow ? x0 + k : ow - 1;
        xs[k] = (uint32_t) x * a;
        i0[k] = resize_div(xs[k], b, j.rb);
        acc[k] = 0;
    }
    const uint8_t *srow = j.src + (size_t) j0 * (size_t) j.sstride;
    uint32_t roff = 0; // (at most 8 strides)
    for (uint32_t lo_y = j0 * d; lo_y < ye; lo_y += d, roff += (uint32_t) j.sstride) {
        const uint32_t top = lo_y > ys ? lo_y : ys, bot = lo_y + d < ye ? lo_y + d : ye, wy = bot - top;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t xe = xs[k] + a;
            uint32_t hsum = 0, i = i0[k];
            for (uint32_t lo = i * b; lo < xe; lo += b, i++) {
                const uint32_t left = lo > xs[k] ? lo : xs[k], right = lo + b < xe ? lo + b : xe;
                hsum += (right - left) * (uint32_t) ld_global<uint8_t>(srow, roff + i);
            }
            acc[k] += wy * hsum;
        }
    }
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        w |= resize_div(acc[k] + (j.D >> 1), j.D, j.rD) << (8 * k);
    }
    uint8_t *drow = j.dst + (size_t) y * (size_t) j.dpitch;
    if (WIDE || (x0 + 4 <= ow && (((uintptr_t) (drow + x0)) & 3) == 0)) {
        st_global<uint32_t>(drow, (uint32_t) x0, w);
    } else {
        for (int k = 0; k < 4 && x0 + k < ow; k++) {
            st_global<uint8_t>(drow, (uint32_t) (x0 + k), (uint8_t) (w >> (8 * k)));
        }
    }
}

} // namespace dsv2
