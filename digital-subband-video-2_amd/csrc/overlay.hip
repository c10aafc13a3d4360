// overlay.hip -- the decoder's draw_info overlay (reference src/dsv_decoder.c: drawvec :243, draw_info :280).
//
// The reference draws block after block in raster order: grid row (once per block row), column line, horizontal dash
// (skip / stable blocks), vertical dash (maintain blocks), motion vector, intra sub-block marks.  Everything it stores is 255
// except the even pixels of a dash, which are 0 -- so the serial order shows only where a vector crosses such a pixel: the
// vector of an earlier block was drawn before the dash and loses, the block's own vector and every later block's win.
// Nothing is ever read back from the picture, which makes the order a rule on coordinates:
//   k_overlay_marks    grid rows, column lines, dashes, intra marks -- pairwise disjoint or equal in value (the dashes lie
//                      strictly inside their block, the marks at its quarter points);
//   k_overlay_vectors  one lane per block steps the reference's line loop and stores 255, except on a zero pixel of a dash
//                      that exists in this mode and belongs to a block of greater raster index.
// The second kernel runs behind the first on the same stream.  Plain vector stores only; the destination is the pinned
// luma plane the caller receives.
//
// One deliberate difference: the reference stores the four intra marks without a bounds check (:326-346), which in a clipped
// last block row / column lands outside the luma plane.  Here a mark outside the plane is dropped.
#include "overlay.h"

namespace dsv2 {

constexpr int kOvRows = 4; // picture rows per workgroup of k_overlay_marks

// One wavefront per workgroup: lane = block column, the row loop and everything derived from the row are scalar.
__global__ __launch_bounds__(64) void k_overlay_marks(const OverlayJob *__restrict__ tab)
{
    const OverlayJob j = job_of(tab, blockIdx.z);
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= j.nbh) {
        return;
    }
    const int w = j.dst.w, h = j.dst.h, bw = j.blk_w, bh = j.blk_h;
    const int lbh = __builtin_ctz(bh);
    const int x = i * bw;
    for (int rr = 0; rr < kOvRows; rr++) {
        const int y = blockIdx.y * kOvRows + rr;
        if (y >= h) {
            break;
        }
        const int r = y & (bh - 1), blk = (y >> lbh) * j.nbh + i;
        uint8_t *row = j.dst.data + (size_t) y * j.dst.stride;
        if (r == 0) { // grid row: this block's share of it, 16 bytes a store
            for (int k = 0; k < bw; k += 16) {
                uint8_t *p = row + x + k;
                if (x + k + 16 <= w && (((uintptr_t) p) & 15) == 0) {
                    *(uint4 *) p = make_uint4(~0u, ~0u, ~0u, ~0u);
                } else {
                    for (int b = 0; b < 16 && x + k + b < w; b++) {
                        p[b] = 255;
                    }
                }
            }
        } else { // column line
            row[x] = 255;
        }
        const int k = r - bh / 2;
        if ((j.mode & DSV_DRAW_STABHQ) && k >= -(bh / 4) && k <= bh / 4) {
            const int f = j.bd[blk], a = x + bw / 2;
            if (k == 0 && (f & (DSV_IS_SKIP | DSV_IS_STABLE))) {
                for (int t = -(bw / 4); t <= bw / 4; t++) {
                    if (a + t < w) {
                        row[a + t] = (uint8_t) ((t & 1) * 255);
                    }
                }
            }
            if ((f & DSV_IS_MAINTAIN) && a < w) {
                row[a] = (uint8_t) ((k & 1) * 255);
            }
        }
        if (j.isP && (j.mode & DSV_DRAW_IBLOCK) && (r == bh / 4 || r == 3 * bh / 4)) {
            // DSV_MASK_INTRA00 / 01 in the upper row of marks, INTRA10 / 11 in the lower one
            const int sm = r == bh / 4 ? j.mvs[blk].submask : j.mvs[blk].submask >> 2;
            if ((sm & 1) && x + bw / 4 < w) {
                row[x + bw / 4] = 255;
            }
            if ((sm & 2) && x + 3 * bw / 4 < w) {
                row[x + 3 * bw / 4] = 255;
            }
        }
    }
}

// drawvec's line, one lane per block.  The loop is the reference's, error update included, so the pixel set is the same; its
// length is bounded by the int16 range of the vector (at most 2^17 steps).
__global__ __launch_bounds__(64) void k_overlay_vectors(const OverlayJob *__restrict__ tab)
{
    const OverlayJob j = job_of(tab, blockIdx.y);
    if (!j.isP || !(j.mode & DSV_DRAW_MOVECS)) {
        return;
    }
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= j.nbh * j.nbv || (j.bd[b] & DSV_IS_SKIP)) {
        return;
    }
    const int w = j.dst.w, h = j.dst.h, bw = j.blk_w, bh = j.blk_h;
    const int lbw = __builtin_ctz(bw), lbh = __builtin_ctz(bh);
    const bool dashes = (j.mode & DSV_DRAW_STABHQ) != 0;
    const int32_t v = j.mvs[b].u.all;
    int x0 = (b % j.nbh) * bw + bw / 2, y0 = (b / j.nbh) * bh + bh / 2;
    const int x1 = x0 + (int16_t) (v & 0xffff), y1 = y0 + (int16_t) (v >> 16);
    const int dx = abs(x1 - x0), dy = abs(y1 - y0);
    const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
    int err = dx - dy;
    auto plot = [&](int px, int py) {
        if ((unsigned) px >= (unsigned) w || (unsigned) py >= (unsigned) h) {
            return;
        }
        if (dashes) {
            const int owner = (py >> lbh) * j.nbh + (px >> lbw);
            if (owner > b) { // that block's dashes are drawn after this vector: their zero pixels stay
                const int lx = (px & (bw - 1)) - bw / 2, ly = (py & (bh - 1)) - bh / 2;
                const bool hz = ly == 0 && abs(lx) <= bw / 4 && !(lx & 1);
                const bool vz = lx == 0 && abs(ly) <= bh / 4 && !(ly & 1);
                if (hz || vz) {
                    const int f = j.bd[owner];
                    if ((hz && (f & (DSV_IS_SKIP | DSV_IS_STABLE))) || (vz && (f & DSV_IS_MAINTAIN))) {
                        return;
                    }
                }
            }
        }
        j.dst.data[(size_t) py * j.dst.stride + px] = 255;
    };
    plot(x0, y0);
    while (x0 != x1 || y0 != y1) {
        plot(x0, y0);
        const int e2 = 2 * err;
        if (e2 > -dy) {
            err -= dy;
            x0 += sx;
        }
        if (e2 < dx) {
            err += dx;
            y0 += sy;
        }
    }
}

void overlay_batch(hipStream_t s, const OverlayJob *d_jobs, int n, int h, int nbh, int nbv, bool any_vectors)
{
    if (n <= 0) {
        return;
    }
    DSV2_LAUNCH(k_overlay_marks, dim3((nbh + 63) / 64, (h + kOvRows - 1) / kOvRows, n), dim3(64), 0, s, d_jobs);
    if (any_vectors) {
        DSV2_LAUNCH(k_overlay_vectors, dim3((nbh * nbv + 63) / 64, n), dim3(64), 0, s, d_jobs);
    }
}

} // namespace dsv2
