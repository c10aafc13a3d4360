// dec_delivery.h -- which kernels a decoded picture leaves through, reading and writing what: planned per picture, free of any device
// call and of any allocation.  decoder.cpp plans every picture of a round with it before it sizes and fills the round's job
// tables; tools/dec_delivery_check.cpp compiles it for the host under AddressSanitizer + UndefinedBehaviorSanitizer and sweeps
// target kind x scale x out420p x postsharp x draw_info x alignment over synthetic addresses (tests/test_dec_delivery_cpu.py);
// tools/dec_delivery_sized_check.cpp does the same for sized targets (tests/test_dec_delivery_sized_cpu.py), tools/dec_plan_check.cpp
// for planar and interleaved tensor targets (tests/test_dec_plan_cpu.py).
#pragma once

#include <math.h>
#include <stddef.h>

#include "io_jobs.h"
#include "surface_layout.h"

namespace dsv2 {
namespace delivery {

// ---- the layout word of a dsv2hip_out_surface -------------------------------------------------------------------------------------------
// layout_shift, layout_unscaled, is_rgb_layout: surface_layout.h (shared with the encoder's scaled ingest, ingest_scale.h)

// ---- where a picture goes ---------------------------------------------------------------------------------------------------------------
struct OutTarget {
    enum Kind {
        FRAME,  // a bordered frame on pinned memory the device writes directly: plane[] / pitch[] are its planes, frame_alloc its block
        PLANAR, // the caller's device planes Y, U, V (a packed buffer: pitch {w, cw, cw})
        SEMI,   // ... Y and one plane of interleaved U V rows (plane[2] unused)
        RGB,    // ... one plane of four-byte pixels, plane[0], converted on the way out (plane[1..2] unused)
        TENSOR, // ... the planes R, G, B of a tensor (dsv2hip_out_tensor), converted on the way out; pitches in bytes
        HWC     // ... one interleaved [h, w, 3] tensor (dsv2hip_out_hwc), plane[0], converted on the way out (plane[1..2] unused)
    } kind = FRAME;
    uint8_t *plane[3] = {nullptr, nullptr, nullptr};
    int pitch[3] = {0, 0, 0};
    int fw[3] = {0, 0, 0}, fh[3] = {0, 0, 0}; // FRAME: the planes' sizes (a device target's follow from the picture's and the shift)
    void *frame_alloc = nullptr;
    int shift = 0;  // device targets: every plane at 1 / 2^shift of its size, box-averaged on the way out (egress_scale.h); 0 .. 3
    int ow = 0, oh = 0; // device targets: the picture at this size, every plane area-averaged on the way out (egress_resize.h); 0 x 0: not
                        // sized.  Never together with a shift
    int csc = 0;    // RGB, TENSOR, HWC: the DSV2HIP_CSC_* bits
    bool bgra = false; // RGB: bytes in memory B G R A, else R G B A; HWC: elements B G R, else R G B
    int dtype = 0;  // TENSOR, HWC: DSV2HIP_TENSOR_*
    float scale[3] = {0, 0, 0}, bias[3] = {0, 0, 0}; // TENSOR, HWC, float element types: the per-plane / per-element constants
    bool device() const { return kind != FRAME; }
    bool converted() const { return kind == RGB || kind == TENSOR || kind == HWC; } // leaves through a YUV -> RGB conversion, which reads every plane in place
    bool sized() const { return ow != 0; }
    bool reduced() const { return shift != 0 || sized(); } // leaves through the reduction or the resampling
};

inline OutTarget target_frame(const DSV_FRAME *f)
{
    OutTarget t;
    t.frame_alloc = f->alloc;
    for (int c = 0; c < 3; c++) {
        t.plane[c] = f->planes[c].data, t.pitch[c] = f->planes[c].stride;
        t.fw[c] = f->planes[c].w, t.fh[c] = f->planes[c].h;
    }
    return t;
}

// A caller's surface, whose layout dsv2hip_dec_surface_dims accepted with these rows: false for a plane that is missing, whose pitch is
// below its row bytes or beyond an int (the kernels carry a pitch as an int) or whose capacity does not hold the rows.
inline bool target_surface(const dsv2hip_out_surface &sf, const size_t row_bytes[3], const int rows[3], OutTarget *out)
{
    OutTarget t;
    const int plain = layout_unscaled(sf.layout);
    t.shift = layout_shift(sf.layout);
    t.kind = is_rgb_layout(sf.layout) ? OutTarget::RGB : plain == DSV2HIP_SURFACE_SEMIPLANAR ? OutTarget::SEMI : OutTarget::PLANAR;
    if (t.kind == OutTarget::RGB) {
        t.csc = plain & (DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE);
        t.bgra = (plain & 0xff) == DSV2HIP_SURFACE_BGRA;
    }
    for (int c = 0; c < (t.kind == OutTarget::RGB ? 1 : t.kind == OutTarget::SEMI ? 2 : 3); c++) {
        if (!sf.plane[c] || sf.pitch[c] < row_bytes[c] || sf.pitch[c] > (size_t) INT32_MAX ||
            sf.cap[c] < (size_t) (rows[c] - 1) * sf.pitch[c] + row_bytes[c]) {
            return false;
        }
        t.plane[c] = (uint8_t *) sf.plane[c];
        t.pitch[c] = (int) sf.pitch[c];
    }
    *out = t;
    return true;
}

// A caller's tensor whose element type, CSC bits and size dsv2hip_dec_tensor_dims accepted with these rows (the three planes are
// alike): false for a plane that is missing or not aligned to its element, a pitch that is no multiple of the element, below the
// row's bytes or beyond an int, a capacity that does not hold the rows, or (float element types) a constant that is not finite.
inline bool target_tensor(const dsv2hip_out_tensor &tn, size_t row_bytes, int rows, OutTarget *out)
{
    OutTarget t;
    t.kind = OutTarget::TENSOR;
    t.dtype = tn.dtype, t.csc = tn.csc;
    const size_t elem = (size_t) tensor_elem(tn.dtype);
    for (int c = 0; c < 3; c++) {
        if (!tn.plane[c] || ((uintptr_t) tn.plane[c]) % elem || tn.pitch[c] % elem || tn.pitch[c] < row_bytes || tn.pitch[c] > (size_t) INT32_MAX ||
            tn.cap[c] < (size_t) (rows - 1) * tn.pitch[c] + row_bytes) {
            return false;
        }
        if (tn.dtype != DSV2HIP_TENSOR_U8) {
            if (!isfinite(tn.scale[c]) || !isfinite(tn.bias[c])) {
                return false;
            }
            t.scale[c] = tn.scale[c], t.bias[c] = tn.bias[c];
        }
        t.plane[c] = (uint8_t *) tn.plane[c];
        t.pitch[c] = (int) tn.pitch[c];
    }
    *out = t;
    return true;
}

// A caller's interleaved tensor whose element type, CSC bits and size dsv2hip_dec_hwc_dims accepted with these rows: false for an order
// that is not exactly DSV2HIP_SURFACE_RGB or _BGR, a NULL pointer or one not aligned to its element, a pitch that is no multiple of the
// element, below the row's bytes or beyond an int, a capacity that does not hold the rows, or (float element types) a constant that is
// not finite.
inline bool target_hwc(const dsv2hip_out_hwc &hw, size_t row_bytes, int rows, OutTarget *out)
{
    OutTarget t;
    t.kind = OutTarget::HWC;
    t.dtype = hw.dtype, t.csc = hw.csc;
    const size_t elem = (size_t) tensor_elem(hw.dtype);
    if ((hw.order != DSV2HIP_SURFACE_RGB && hw.order != DSV2HIP_SURFACE_BGR) || !hw.data || ((uintptr_t) hw.data) % elem || hw.pitch % elem ||
        hw.pitch < row_bytes || hw.pitch > (size_t) INT32_MAX || hw.cap < (size_t) (rows - 1) * hw.pitch + row_bytes) {
        return false;
    }
    t.bgra = hw.order == DSV2HIP_SURFACE_BGR;
    if (hw.dtype != DSV2HIP_TENSOR_U8) {
        for (int k = 0; k < 3; k++) {
            if (!isfinite(hw.scale[k]) || !isfinite(hw.bias[k])) {
                return false;
            }
            t.scale[k] = hw.scale[k], t.bias[k] = hw.bias[k];
        }
    }
    t.plane[0] = (uint8_t *) hw.data;
    t.pitch[0] = (int) hw.pitch;
    *out = t;
    return true;
}

// the packed buffer of dsv2hip_dec_batch_device: the planar surface with pitch {w, cw, cw}, plane behind plane
inline OutTarget target_packed(void *buf, const size_t row_bytes[3], const int rows[3])
{
    OutTarget t;
    t.kind = OutTarget::PLANAR;
    uint8_t *at = (uint8_t *) buf;
    for (int c = 0; c < 3; c++) {
        t.plane[c] = at;
        t.pitch[c] = (int) row_bytes[c];
        at += row_bytes[c] * (size_t) rows[c];
    }
    return t;
}

// the YUV -> RGB conversion of include/dsv2_hip.h for a layout's DSV2HIP_CSC_* bits: ky, ybase, rv, gu, gv, bu
inline RgbOutCoefs rgb_out_coefs(int csc)
{
    static const int preset[4][6] = {{298, 16, 409, -100, -208, 516},  // BT601 (limited)
                                     {298, 16, 459, -55, -136, 541},   // BT709 (limited)
                                     {256, 0, 359, -88, -183, 454},    // BT601 | FULL
                                     {256, 0, 403, -48, -120, 475}};   // BT709 | FULL
    const int *p = preset[((csc & DSV2HIP_CSC_FULL_RANGE) ? 2 : 0) + ((csc & DSV2HIP_CSC_BT709) ? 1 : 0)];
    return RgbOutCoefs{p[0], p[1], p[2], p[3], p[4], p[5]};
}

// ---- what one picture contributes to a round --------------------------------------------------------------------------------------------
// The jobs by launch class, in the order the round launches the classes: whole-frame copy, 4:2:0 conversion, egress, overlay, sharpening
// in place, reduction, resampling, chroma interleave, RGB conversion (one launch per layout: packed, planar, interleaved).  A job of a
// later class may read what a job of an earlier one wrote -- the decoder's two staging areas -- and nothing else is shared between them.
struct DeliveryPlan {
    CopyJob copy[1];
    To420Job to420[3];
    EgressJob eg[3];
    ScaleOutJob scl[3];
    ResizeOutJob rsz[3];
    UvEgressJob uv[1];
    RgbOutJob rgb[1];
    DPlane overlay[1]; // the luma plane the draw_info overlay goes onto: the delivered one, or the staged one
    int n_copy = 0, n_to420 = 0, n_eg = 0, n_scl = 0, n_rsz = 0, n_uv = 0, n_rgb = 0, n_overlay = 0;
    bool sharpen_overlaid = false; // that plane is also sharpened in place, behind the overlay (a drawn-on picture under postsharp)
    // what the round needs to pick its kernels' forms
    bool eg_wide = true, eg_sharp = false; // every egress job allows the 16-byte form / some egress job sharpens (egress.hip: k_egress)
    bool scl_wide = true;                  // every reduction job allows the unconditional vector store (egress.hip: k_egress_scale)
    int scl_rows = 0;                      // the most rows a reduction job delivers
    bool rsz_wide = true;                  // every resampling job allows the unconditional dword store (egress.hip: k_egress_resize)
    int rsz_rows = 0, rsz_cols = 0;        // the most rows / samples a row a resampling job delivers
    bool uv_wide = true, uv_conv = false;  // the interleave job allows the 16-byte form / converts to 4:2:0 (egress.hip: k_egress_uv)
    int uv_rows = 0;                       // the chroma rows it delivers ("4:1:0" to 4:2:0: more than the source has)
    bool rgb_wide = true;                  // the RGB job allows the wide form (egress.hip: k_egress_rgb; its layout: rgb[0].layout)
};

// A sharpened and / or drawn-on picture that leaves reduced, as RGB or as a tensor (planar or interleaved) has no delivered full-size luma plane for the overlay and the
// sharpening to act on: its luma goes through the egress kernel into DecImpl's staged luma plane (w x h, 16-byte aligned origin and stride)
inline bool needs_staged_luma(const OutTarget &t, bool sharp, int draw)
{
    return t.device() && (t.reduced() || t.converted()) && (sharp || draw);
}
// the reduced planes that k_egress_uv / k_egress_rgb then read go into DecImpl's staged scaled picture (16-byte aligned origins and strides)
inline bool needs_staged_scaled(const OutTarget &t) { return t.device() && t.reduced() && t.kind != OutTarget::PLANAR; }
// ... which a sized picture needs at up to the picture's own size, a shifted one at half size
inline bool needs_staged_full(const OutTarget &t) { return needs_staged_scaled(t) && t.sized(); }

// recon: the picture as decoded (read only; its format is the stream's); out_format: the delivered picture's, the stream's or 4:2:0 under
// out420p; staged_luma / staged_scaled: the staging areas' planes, looked at only where the predicates above hold
inline DeliveryPlan plan_delivery(const DFrame &recon, int out_format, const OutTarget &t, bool sharp, int draw, const DPlane &staged_luma,
                                  const DPlane *staged_scaled)
{
    DeliveryPlan p{};
    const int hs = DSV_FORMAT_H_SHIFT(recon.format), vs = DSV_FORMAT_V_SHIFT(recon.format);
    const bool conv = out_format != recon.format; // converted on the way out (dsv_main.c:1030-1048): chroma through the reference's pair averages
    const bool sharp_out = sharp && !draw;        // luma sharpened in registers on its way out (a drawn one: in place, behind the overlay)
    // the planes of the delivered picture: those of the pinned frame, or the caller's device planes (semiplanar: op[1] is the interleaved
    // plane, w (U, V) pairs a row; op[2] is not a plane)
    DPlane op[3];
    if (t.device()) {
        const int ohs = DSV_FORMAT_H_SHIFT(out_format), ovs = DSV_FORMAT_V_SHIFT(out_format);
        const int ocw = (recon.w + (1 << ohs) - 1) >> ohs, och = (recon.h + (1 << ovs) - 1) >> ovs; // dsv_mk_frame's plane sizes (frame.c:63-113)
        const bool semi = t.kind == OutTarget::SEMI;
        op[0] = DPlane{t.plane[0], t.pitch[0], recon.w, recon.h};
        op[1] = DPlane{t.plane[1], t.pitch[1], ocw, och};
        op[2] = DPlane{semi ? nullptr : t.plane[2], semi ? 0 : t.pitch[2], ocw, och};
    } else {
        for (int c = 0; c < 3; c++) {
            op[c] = DPlane{t.plane[c], t.pitch[c], t.fw[c], t.fh[c]};
        }
    }
    auto egress = [&](const DPlane &src, const DPlane &dst, bool sharpen) {
        const EgressJob &j = p.eg[p.n_eg++] = EgressJob{src, dst.data, dst.stride, sharpen};
        p.eg_sharp = p.eg_sharp || sharpen;
        p.eg_wide = p.eg_wide && egress_job_wide(j, dst.w);
    };
    if (t.device() && (t.reduced() || t.converted())) {
        // Every plane is read in place by the reduction (egress_scale.h) and / or the RGB conversion.  A sharpened and / or drawn-on
        // picture: its full-size luma is staged first, stands in for the delivered luma plane below (overlay, sharpening behind the
        // overlay) and is what the reduction or the conversion then reads.  (No 4:2:0 conversion here: the surface call refuses the pair.)
        DPlane src[3] = {recon.p[0], recon.p[1], recon.p[2]};
        if (needs_staged_luma(t, sharp, draw)) {
            src[0] = op[0] = staged_luma;
            egress(recon.p[0], staged_luma, sharp_out);
        }
        if (t.shift) {
            // PLANAR, and the luma of SEMIPLANAR, straight into the caller's planes; what the interleave or the conversion has yet to read,
            // into the staged scaled picture, from which the unchanged k_egress_uv (mode 0) / k_egress_rgb run on the reduced geometry
            const int s = t.shift, up = (1 << s) - 1;
            for (int c = 0; c < 3; c++) {
                const bool staged = t.converted() || (t.kind == OutTarget::SEMI && c);
                DPlane red = staged ? staged_scaled[c] : DPlane{t.plane[c], t.pitch[c], 0, 0};
                red.w = (src[c].w + up) >> s, red.h = (src[c].h + up) >> s;
                const ScaleOutJob &sj = p.scl[p.n_scl++] = ScaleOutJob{src[c].data, red.data, src[c].stride, src[c].w, src[c].h, red.stride, s};
                p.scl_wide = p.scl_wide && scale_job_wide(sj, staged ? red.stride : red.w);
                p.scl_rows = red.h > p.scl_rows ? red.h : p.scl_rows;
                src[c] = red;
            }
        } else if (t.sized()) {
            // the same routes at the size the caller names: luma ow x oh, chroma dsv_mk_frame's planes for that picture, each plane by
            // its own ratio (egress_resize.h)
            for (int c = 0; c < 3; c++) {
                const bool staged = t.converted() || (t.kind == OutTarget::SEMI && c);
                DPlane red = staged ? staged_scaled[c] : DPlane{t.plane[c], t.pitch[c], 0, 0};
                red.w = c ? (t.ow + (1 << hs) - 1) >> hs : t.ow, red.h = c ? (t.oh + (1 << vs) - 1) >> vs : t.oh;
                const ResizeOutJob &rj = p.rsz[p.n_rsz++] = resize_job(src[c].data, src[c].stride, src[c].w, src[c].h, red.data, red.stride, red.w, red.h);
                p.rsz_wide = p.rsz_wide && resize_job_wide(rj, staged ? red.stride : red.w);
                p.rsz_rows = red.h > p.rsz_rows ? red.h : p.rsz_rows;
                p.rsz_cols = red.w > p.rsz_cols ? red.w : p.rsz_cols;
                src[c] = red;
            }
        }
        if (t.kind == OutTarget::SEMI) {
            const UvEgressJob &uj = p.uv[p.n_uv++] =
                UvEgressJob{src[1].data, src[2].data, t.plane[1], t.pitch[1], src[1].stride, src[1].w, src[1].h, src[1].w, src[1].h, 0};
            p.uv_wide = uv_job_wide(uj);
            p.uv_rows = src[1].h;
        } else if (t.converted()) { // one conversion job, its layout the target's (plane[1..2] and pitch[1..2]: null / 0 but for TENSOR)
            const int layout = t.kind == OutTarget::RGB ? kRgbOutPacked : t.kind == OutTarget::TENSOR ? kRgbOutPlanar : kRgbOutInterleaved;
            const RgbOutJob &rj = p.rgb[p.n_rgb++] = RgbOutJob{src[0].data,
                                                               src[1].data,
                                                               src[2].data,
                                                               src[0].stride,
                                                               src[1].stride,
                                                               src[0].w,
                                                               src[0].h,
                                                               hs,
                                                               vs,
                                                               rgb_out_coefs(t.csc),
                                                               t.bgra,
                                                               layout,
                                                               {t.plane[0], t.plane[1], t.plane[2]},
                                                               {t.pitch[0], t.pitch[1], t.pitch[2]},
                                                               t.dtype,
                                                               {t.scale[0], t.scale[1], t.scale[2]},
                                                               {t.bias[0], t.bias[1], t.bias[2]}};
            p.rgb_wide = rgb_out_job_wide(rj);
        }
    } else if (!conv && !t.device() && !sharp_out) {
        p.copy[p.n_copy++] = CopyJob{recon.alloc, t.frame_alloc, recon.bytes};
    } else {
        const int mode = (hs == 0 && vs == 0) ? 1 : (hs == 1 && vs == 0) ? 2 : (hs == 2 && vs == 0) ? 3 : 4;
        for (int c = 0; c < 3; c++) {
            if (c && t.kind == OutTarget::SEMI) { // both chroma planes through one job, converted on the way or not
                if (c == 1) {
                    const DPlane &su = recon.p[1];
                    const UvEgressJob &uj = p.uv[p.n_uv++] =
                        UvEgressJob{su.data, recon.p[2].data, op[1].data, op[1].stride, su.stride, su.w, su.h, op[1].w, op[1].h, conv ? mode : 0};
                    p.uv_wide = uv_job_wide(uj);
                    p.uv_conv = conv;
                    p.uv_rows = op[1].h;
                }
            } else if (conv && (c || (!t.device() && !sharp_out))) {
                p.to420[p.n_to420++] = To420Job{recon.p[c], op[c], c ? mode : 0};
            } else {
                egress(recon.p[c], op[c], c == 0 && sharp_out);
            }
        }
    }
    if (draw) { // on the picture the caller receives only: the reconstruction, which the next P picture reads, stays as decoded (dsv_decoder.c:555-561)
        p.overlay[p.n_overlay++] = op[0];
        p.sharpen_overlaid = sharp;
    }
    return p;
}

} // namespace delivery
} // namespace dsv2
