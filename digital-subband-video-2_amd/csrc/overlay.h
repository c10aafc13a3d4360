// overlay.h -- DSV_DECODER.draw_info: the block grid, skip / stable / maintain dashes, motion vectors and intra sub-block
// marks the reference decoder draws on the luma of the pictures it hands out (dsv_decoder.c:240-350).
#pragma once

#include "dev.h"

namespace dsv2 {

// One picture of a decoder round that asked for the overlay.  The record is the same for every lane of a workgroup: the
// kernels fetch it by value through the scalar cache (job_of, dev.h).
struct OverlayJob {
    DPlane dst;        // luma plane of the frame the caller receives (pinned host memory, written only)
    const DSV_MV *mvs; // the picture's motion field (read for P pictures only)
    const uint8_t *bd; // the picture's per-block flag bytes
    int nbh, nbv;      // blocks per row / column
    int blk_w, blk_h;  // block size: 16 << k each
    int mode;          // the decoder's draw_info word (DSV_DRAW_*), non-zero
    int isP;
};

// n jobs of one picture geometry (w x h luma, nbh x nbv blocks); any_vectors: some job is a P picture with DSV_DRAW_MOVECS
void overlay_batch(hipStream_t s, const OverlayJob *d_jobs, int n, int h, int nbh, int nbv, bool any_vectors);

} // namespace dsv2
