// ingest_plan.h -- how the ingest check programs come by their job records: from the library's own acceptance rule and planner
// (csrc/enc_ingest.h), given the guarded planes they made as the encoder's source planes and their exact-size source blocks as a
// caller's surface.  The records the kernels' bodies then run on are the ones encoder.cpp would have built.
#pragma once

#include <stdio.h>
#include <stdlib.h>

#include "enc_ingest.h"

// PlaneT: org (pixel (0,0)), stride, w, h
template <class PlaneT>
dsv2::enc_ingest::IngestPlan planned_from(int subsamp, const PlaneT &Y, const PlaneT &U, const PlaneT &V, const dsv2::enc_ingest::Source &src)
{
    dsv2::DFrame f;
    f.format = subsamp, f.w = Y.w, f.h = Y.h;
    const PlaneT *pl[3] = {&Y, &U, &V};
    for (int c = 0; c < 3; c++) {
        f.p[c] = dsv2::DPlane{pl[c]->org, pl[c]->stride, pl[c]->w, pl[c]->h};
    }
    return dsv2::enc_ingest::plan_ingest(f, src);
}
// A surface the rule refuses ends the program: the sweeps hold only what a caller may bring.
template <class PlaneT>
dsv2::enc_ingest::IngestPlan planned(dsv2::enc_ingest::Call call, int subsamp, const PlaneT &Y, const PlaneT &U, const PlaneT &V,
                                     const dsv2hip_surface &sf, int src_w, int src_h)
{
    dsv2::enc_ingest::Source src;
    if (!dsv2::enc_ingest::accept(call, Y.w, Y.h, subsamp, false, sf, src_w, src_h, &src)) {
        fprintf(stderr, "REFUSED: layout 0x%x, %dx%d for an encoder of %dx%d in format %d, call %d\n", sf.layout, src_w, src_h, Y.w, Y.h, subsamp, (int) call);
        exit(1);
    }
    return planned_from(subsamp, Y, U, V, src);
}
// the plan holds `want` records of class `cl` and none of another
inline void expect_records(const dsv2::enc_ingest::IngestPlan &p, int cl, int want)
{
    for (int c = 0; c < dsv2::enc_ingest::kClasses; c++) {
        if (p.n[c] != (c == cl ? want : 0)) {
            fprintf(stderr, "PLAN: %d records of class %d where %d of class %d alone were expected\n", p.n[c], c, want, cl);
            exit(1);
        }
    }
}
