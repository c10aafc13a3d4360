// enc_ingest.h -- which kernels a picture enters the encoder through, reading and writing what: accepted per call and planned per
// picture, free of any device call and of any allocation (the decoder's counterpart is dec_delivery.h).  encoder.cpp
// passes every surface of the three surface calls through accept(), every tensor of the tensor calls through accept_tensor() (DESIGN
// 5.22; tools/enc_tensor_plan_check.cpp sweeps those), every interleaved tensor of the hwc calls through accept_hwc() (DESIGN 5.26;
// tools/enc_hwc_plan_check.cpp), and plans every picture of a step with plan_ingest() before it sizes
// and fills the step's job tables.  tools/enc_ingest_check.cpp compiles this header for the host under AddressSanitizer +
// UndefinedBehaviorSanitizer and sweeps format x size x kind x route x offset x pitch over synthetic addresses
// (tests/test_enc_ingest_cpu.py); the four tools/ingest_*_check.cpp run the kernels' bodies on the records planned here.
#pragma once

#include "ingest_resize.h" // ingest_resize::plan_sized_source, sized_ratio; ingest_scale::plan_source, surface_fits

namespace dsv2 {
namespace enc_ingest {

enum Call { CALL_PLAIN, CALL_SCALED, CALL_SIZED }; // dsv2hip_enc_batch_surface / _surface_scaled / _surface_sized and their one-frame calls

// ---- where a picture comes from ---------------------------------------------------------------------------------------------------------
struct Source { // (an aggregate without initialisers: it lives in the encoder's Job, which is cleared as bytes -- all zero is PACKED)
    enum Kind {
        PACKED, // no surface: a packed picture in HBM (planar, or UYVY rows), as uploaded from the host or not, or a host DSV_FRAME -- the
                // step's own business, no record of the plan
        PLANAR, // the caller's device planes Y, U, V
        SEMI,   // ... Y and one plane of interleaved U V rows (plane[2] unused)
        RGB4,   // ... one plane of four-byte pixels, BGRA / RGBA (plane[1..2] unused)
        RGB3,   // ... one plane of three-byte pixels, BGR / RGB
        RGBP,   // ... a plane per colour: R, G, B
        TENSOR, // ... a plane per colour of binary16, bfloat16 or binary32 elements under per-plane constants (dsv2hip_in_tensor; the plain
                // route alone).  A uint8 tensor is an RGBP.
        HWC     // ... one plane of three such elements a pixel, R G B or B G R, under per-position constants (dsv2hip_in_hwc; the plain
                // route alone; plane[0] / pitch[0]).  A uint8 one is an RGB3.
    } kind;
    enum Route {
        PLAIN,   // the picture in the surface has the encoder's size
        REDUCED, // it is src_w x src_h and box-averaged by 1 << shift on the way in (ingest_scale.h)
        SIZED    // it is src_w x src_h, larger than the encoder's, and area-averaged on the way in (ingest_resize.h)
    } route;
    const uint8_t *plane[3]; // by value: the caller's dsv2hip_surface may go once the call has been accepted
    size_t pitch[3];
    int src_w, src_h; // of the picture IN THE SURFACE
    int shift;        // REDUCED: 1 .. 3
    int layout;       // the RGB kinds: the layout without its scale value -- byte order and DSV2HIP_CSC_* bits (TENSOR: the bits alone; HWC: the
                      // element order, DSV2HIP_SURFACE_RGB or _BGR, and the bits)
    int dtype;        // TENSOR, HWC: DSV2HIP_TENSOR_F16, _BF16 or _F32
    float scale[3], bias[3]; // TENSOR: of plane[c]; HWC: of element k of every pixel
    bool surface() const { return kind != PACKED; }
    bool rgb() const { return kind == RGB4 || kind == RGB3 || kind == RGBP || kind == TENSOR || kind == HWC; }
};

// One rule for the three calls: may an encoder of enc_w x enc_h in format subsamp take surface sf, which the caller says holds a picture
// of src_w x src_h (CALL_PLAIN: not looked at, the encoder's own size)?  Fills *out where it may.  The scaled and the sized call start
// from ingest_scale::plan_source / ingest_resize::plan_sized_source (layout grammar with the value held back, formats, size relation,
// planes and pitches of the SOURCE); an entry of theirs that carries no scale and has the encoder's size must pass the plain call's
// rule, and is the plain call's picture.  Refused: every surface on an encoder with UYVY input on; a layout outside the grammar (a CSC bit
// on PLANAR / SEMIPLANAR among them); an RGB layout on a format that is none of the five; three-byte and planar RGB through the scaled
// and the sized call; a missing plane; a pitch below its row's bytes.
inline bool accept(Call call, int enc_w, int enc_h, int subsamp, bool uyvy_input, const dsv2hip_surface &sf, int src_w, int src_h, Source *out)
{
    if (uyvy_input) {
        return false;
    }
    Source s{};
    s.layout = sf.layout, s.src_w = enc_w, s.src_h = enc_h;
    int nplanes = 0;
    if (call != CALL_PLAIN) {
        ingest_resize::Sized z;
        if (call == CALL_SCALED ? !ingest_scale::plan_source(src_w, src_h, subsamp, sf.layout, &z.src) || !ingest_scale::surface_fits(z.src, sf, enc_w, enc_h)
                                : !ingest_resize::plan_sized_source(src_w, src_h, enc_w, enc_h, subsamp, sf.layout, &z) || !ingest_resize::sized_surface_fits(z, sf)) {
            return false;
        }
        if (z.src.shift || z.sized) {
            s.route = z.src.shift ? Source::REDUCED : Source::SIZED;
            s.kind = z.src.kind == ingest_scale::Source::RGB ? Source::RGB4 : z.src.kind == ingest_scale::Source::SEMI ? Source::SEMI : Source::PLANAR;
            s.layout = z.src.plain_layout, s.shift = z.src.shift, s.src_w = src_w, s.src_h = src_h;
            nplanes = z.src.nplanes;
        }
    }
    if (s.route == Source::PLAIN) { // every pitch at least its row's bytes, every plane the layout has
        const int order = sf.layout & ~(DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE), hs = DSV_FORMAT_H_SHIFT(subsamp);
        const size_t w = (size_t) enc_w, cw = (w + ((size_t) 1 << hs) - 1) >> hs;
        size_t row_bytes[3] = {w, cw, cw};
        if (sf.layout == DSV2HIP_SURFACE_PLANAR) {
            s.kind = Source::PLANAR, nplanes = 3;
        } else if (sf.layout == DSV2HIP_SURFACE_SEMIPLANAR) {
            s.kind = Source::SEMI, nplanes = 2, row_bytes[1] = 2 * cw;
        } else if (!ingest_scale::rgb_format(subsamp)) { // (a stream format outside the five the conversion knows: the RGB kernels have no code for it)
            return false;
        } else if (order == DSV2HIP_SURFACE_BGRA || order == DSV2HIP_SURFACE_RGBA) {
            s.kind = Source::RGB4, nplanes = 1, row_bytes[0] = 4 * w;
        } else if (order == DSV2HIP_SURFACE_BGR || order == DSV2HIP_SURFACE_RGB) {
            s.kind = Source::RGB3, nplanes = 1, row_bytes[0] = 3 * w;
        } else if (order == DSV2HIP_SURFACE_RGBP) {
            s.kind = Source::RGBP, nplanes = 3, row_bytes[1] = row_bytes[2] = w;
        } else {
            return false;
        }
        for (int c = 0; c < nplanes; c++) {
            if (!sf.plane[c] || sf.pitch[c] < row_bytes[c]) {
                return false;
            }
        }
    }
    for (int c = 0; c < nplanes; c++) {
        s.plane[c] = (const uint8_t *) sf.plane[c], s.pitch[c] = sf.pitch[c];
    }
    *out = s;
    return true;
}

// The same rule for a tensor (dsv2hip_enc_batch_tensor / _tensor_frame; always the plain route: the picture has the encoder's size).
// Refused: what accept() refuses for an RGB layout (UYVY input on, a stream format outside the five); an unknown dtype; a csc bit outside
// the two; a NULL plane; a plane pointer or a pitch that is not a multiple of the element size; a pitch below w * elem; for a float dtype
// a scale[c] or bias[c] that is not finite.  A uint8 tensor IS the planar RGB surface: it leaves as an RGBP source, constants unread.
inline bool accept_tensor(int enc_w, int enc_h, int subsamp, bool uyvy_input, const dsv2hip_in_tensor &t, Source *out)
{
    if (t.csc & ~(DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE)) {
        return false;
    }
    if (t.dtype == DSV2HIP_TENSOR_U8) {
        const dsv2hip_surface sf{{t.plane[0], t.plane[1], t.plane[2]}, {t.pitch[0], t.pitch[1], t.pitch[2]}, DSV2HIP_SURFACE_RGBP | t.csc};
        return accept(CALL_PLAIN, enc_w, enc_h, subsamp, uyvy_input, sf, 0, 0, out);
    }
    if (uyvy_input || !ingest_scale::rgb_format(subsamp) || (t.dtype != DSV2HIP_TENSOR_F16 && t.dtype != DSV2HIP_TENSOR_BF16 && t.dtype != DSV2HIP_TENSOR_F32)) {
        return false;
    }
    Source s{};
    s.kind = Source::TENSOR, s.route = Source::PLAIN, s.layout = t.csc, s.src_w = enc_w, s.src_h = enc_h, s.dtype = t.dtype;
    const size_t elem = (size_t) tensor_elem(t.dtype);
    for (int c = 0; c < 3; c++) {
        // (finite: x - x is 0 for every finite x and a NaN for the infinities and the NaNs)
        if (!t.plane[c] || ((uintptr_t) t.plane[c] | t.pitch[c]) % elem != 0 || t.pitch[c] / elem < (size_t) enc_w || t.scale[c] - t.scale[c] != 0.0f ||
            t.bias[c] - t.bias[c] != 0.0f) {
            return false;
        }
        s.plane[c] = (const uint8_t *) t.plane[c], s.pitch[c] = t.pitch[c];
        s.scale[c] = t.scale[c], s.bias[c] = t.bias[c];
    }
    *out = s;
    return true;
}

// The same rule for an interleaved tensor (dsv2hip_enc_batch_hwc / _hwc_frame; always the plain route).  Refused: what accept_tensor
// refuses, read for one pointer and pitch (the row holds 3 * w elements); an order that is not exactly DSV2HIP_SURFACE_RGB or
// DSV2HIP_SURFACE_BGR.  A uint8 one IS the three-byte surface: it leaves as an RGB3 source, constants unread.
inline bool accept_hwc(int enc_w, int enc_h, int subsamp, bool uyvy_input, const dsv2hip_in_hwc &t, Source *out)
{
    if ((t.csc & ~(DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE)) || (t.order != DSV2HIP_SURFACE_RGB && t.order != DSV2HIP_SURFACE_BGR)) {
        return false;
    }
    if (t.dtype == DSV2HIP_TENSOR_U8) {
        const dsv2hip_surface sf{{t.data, nullptr, nullptr}, {t.pitch, 0, 0}, t.order | t.csc};
        return accept(CALL_PLAIN, enc_w, enc_h, subsamp, uyvy_input, sf, 0, 0, out);
    }
    if (uyvy_input || !ingest_scale::rgb_format(subsamp) || (t.dtype != DSV2HIP_TENSOR_F16 && t.dtype != DSV2HIP_TENSOR_BF16 && t.dtype != DSV2HIP_TENSOR_F32)) {
        return false;
    }
    const size_t elem = (size_t) tensor_elem(t.dtype);
    if (!t.data || ((uintptr_t) t.data | t.pitch) % elem != 0 || t.pitch / elem < 3 * (size_t) enc_w) {
        return false;
    }
    Source s{};
    s.kind = Source::HWC, s.route = Source::PLAIN, s.layout = t.order | t.csc, s.src_w = enc_w, s.src_h = enc_h, s.dtype = t.dtype;
    s.plane[0] = (const uint8_t *) t.data, s.pitch[0] = t.pitch;
    for (int k = 0; k < 3; k++) {
        if (t.scale[k] - t.scale[k] != 0.0f || t.bias[k] - t.bias[k] != 0.0f) { // (finite: accept_tensor's test)
            return false;
        }
        s.scale[k] = t.scale[k], s.bias[k] = t.bias[k];
    }
    *out = s;
    return true;
}

// The conversion of include/dsv2_hip.h for an RGB surface of `layout` as the RGB ingest kernels take it: each row of the preset's matrix as
// byte quads in the surface's channel order (a fourth byte weighs 0), chroma rows split into positive parts and magnitudes of negative ones
inline RgbInCoefs rgb_job_coefs(int layout)
{
    static const int presets[4][9] = {{66, 129, 25, -38, -74, 112, 112, -94, -18},   // BT601 (limited)
                                      {47, 157, 16, -26, -86, 112, 112, -102, -10},  // BT709 (limited)
                                      {77, 150, 29, -43, -85, 128, 128, -107, -21},  // BT601 | FULL
                                      {54, 183, 19, -29, -99, 128, 128, -116, -12}}; // BT709 | FULL
    const bool full = (layout & DSV2HIP_CSC_FULL_RANGE) != 0;
    const int *m = presets[(full ? 2 : 0) + ((layout & DSV2HIP_CSC_BT709) ? 1 : 0)];
    const int order = layout & ~(DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE);
    const bool b_first = order == DSV2HIP_SURFACE_BGRA || order == DSV2HIP_SURFACE_BGR; // blue is byte 0 of a pixel
    uint32_t q[3][2];
    for (int row = 0; row < 3; row++) {
        q[row][0] = q[row][1] = 0;
        for (int c = 0; c < 3; c++) { // R, G, B
            const int v = m[3 * row + c], at = 8 * (b_first ? 2 - c : c);
            q[row][v < 0] |= (uint32_t) (v < 0 ? -v : v) << at;
        }
    }
    return RgbInCoefs{q[0][0], q[1][0], q[1][1], q[2][0], q[2][1], 128u + (full ? 0u : 256u * 16u)};
}

// ---- what one picture contributes to a step ---------------------------------------------------------------------------------------------
// The launch classes, in the order the step launches them (behind the packed and the UYVY pictures' launches); a class has a job table
// of its own in the step, a form counter pair, and one launch for all the step's records of it.
enum Class { SURF, RGB, SCALED_SURF, SCALED_RGB, SIZED_SURF, SIZED_RGB, RGB3_PACKED, RGB3_PLANAR, TENSOR_IN, HWC_IN, kClasses };

struct IngestPlan {
    SurfaceJob surf[3];
    RgbJob rgb[1];
    ScaledSurfaceJob scaled_surf[3];
    ScaledRgbJob scaled_rgb[1];
    SizedSurfaceJob sized_surf[3];
    SizedRgbJob sized_rgb[1];
    Rgb3Job rgb3[1];                         // of RGB3_PACKED or of RGB3_PLANAR, by its kind
    TensorInJob tensor[1];
    int n[kClasses] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // records per class: a surface brings those of ONE class, a PACKED picture none
    // what the step needs to pick its kernels' forms and grids
    bool wide[kClasses] = {true, true, true, true, true, true, true, true, true, true}; // every record of the class allows the wide form (io_jobs.h: *_job_wide)
    int scaled_row_bytes = 0; // SCALED_SURF: the most bytes a source row of a record holds
    int scaled_rgb_sw = 0;    // SCALED_RGB: the source's width
    HwcInJob hwc[1];          // (behind every member a plan had before it)
};
// the room a picture's records take in the step's table arena at most: they are some of its plan's arrays
constexpr size_t kPlanRecordBytes = 3 * sizeof(SurfaceJob) + sizeof(RgbJob) + 3 * sizeof(ScaledSurfaceJob) + sizeof(ScaledRgbJob) +
                                    3 * sizeof(SizedSurfaceJob) + sizeof(SizedRgbJob) + sizeof(Rgb3Job) + sizeof(TensorInJob) + sizeof(HwcInJob);

// f: the encoder's bordered source planes (dframe_alloc's: its format and plane sizes are the encoder's), which the records write; s: an
// accepted source
inline IngestPlan plan_ingest(const DFrame &f, const Source &s)
{
    IngestPlan p;
    if (!s.surface()) {
        return p;
    }
    const DPlane *dp = f.p;
    const int hs = DSV_FORMAT_H_SHIFT(f.format), vs = DSV_FORMAT_V_SHIFT(f.format);
    const bool semi = s.kind == Source::SEMI;
    const int scw = (s.src_w + (1 << hs) - 1) >> hs, sch = (s.src_h + (1 << vs) - 1) >> vs; // dsv_mk_frame's chroma planes, of the SOURCE
    if (s.kind == Source::HWC) { // (the plain route alone)
        HwcInJob &j = p.hwc[p.n[HWC_IN]++];
        j = HwcInJob{s.plane[0], s.pitch[0], {dp[0].data, dp[1].data, dp[2].data}, dp[0].stride, dp[1].stride, dp[0].w, dp[0].h, hs, vs, s.dtype,
                     rgb_job_coefs(s.layout), // (memory order is byte order, as for a packed Rgb3Job)
                     {s.scale[0], s.scale[1], s.scale[2]}, {s.bias[0], s.bias[1], s.bias[2]}};
        p.wide[HWC_IN] = hwc_in_job_wide(j);
    } else if (s.kind == Source::TENSOR) { // (the plain route alone)
        TensorInJob &j = p.tensor[p.n[TENSOR_IN]++];
        j = TensorInJob{{s.plane[0], s.plane[1], s.plane[2]}, {s.pitch[0], s.pitch[1], s.pitch[2]}, {dp[0].data, dp[1].data, dp[2].data}, dp[0].stride, dp[1].stride,
                        dp[0].w, dp[0].h, hs, vs, s.dtype,
                        rgb_job_coefs(DSV2HIP_SURFACE_RGBA | (s.layout & 0x300)), // (R is byte 0 of a pixel dword, as for the planar kind)
                        {s.scale[0], s.scale[1], s.scale[2]}, {s.bias[0], s.bias[1], s.bias[2]}};
        p.wide[TENSOR_IN] = tensor_in_job_wide(j);
    } else if (s.kind == Source::RGB3 || s.kind == Source::RGBP) { // (the plain route alone)
        const int kind = s.kind == Source::RGBP ? kRgb3Planar : kRgb3Packed, cl = RGB3_PACKED + kind;
        Rgb3Job &j = p.rgb3[p.n[cl]++];
        j = Rgb3Job{{s.plane[0], nullptr, nullptr}, {s.pitch[0], 0, 0}, {dp[0].data, dp[1].data, dp[2].data}, dp[0].stride, dp[1].stride,
                    dp[0].w, dp[0].h, hs, vs, kind,
                    rgb_job_coefs(kind == kRgb3Planar ? DSV2HIP_SURFACE_RGBA | (s.layout & 0x300) : s.layout)}; // (planar: R is byte 0 of a pixel dword)
        for (int c = 1; c < 3 && kind == kRgb3Planar; c++) {
            j.src[c] = s.plane[c], j.pitch[c] = s.pitch[c];
        }
        p.wide[cl] = rgb3_job_wide(j);
    } else if (s.kind == Source::RGB4 && s.route == Source::SIZED) {
        SizedRgbJob &j = p.sized_rgb[p.n[SIZED_RGB]++];
        j = SizedRgbJob{s.plane[0], s.pitch[0], {dp[0].data, dp[1].data, dp[2].data}, dp[0].stride, dp[1].stride, dp[0].w, dp[0].h, dp[1].w, dp[1].h,
                        ingest_resize::sized_ratio(s.src_w, s.src_h, dp[0].w, dp[0].h, true),
                        ingest_resize::sized_ratio(s.src_w, s.src_h, dp[1].w, dp[1].h, true), rgb_job_coefs(s.layout)};
        p.wide[SIZED_RGB] = sized_rgb_job_wide(j);
    } else if (s.kind == Source::RGB4 && s.route == Source::REDUCED) {
        ScaledRgbJob &j = p.scaled_rgb[p.n[SCALED_RGB]++];
        j = ScaledRgbJob{s.plane[0], s.pitch[0], {dp[0].data, dp[1].data, dp[2].data}, dp[0].stride, dp[1].stride, s.src_w, s.src_h, hs, vs, s.shift,
                         rgb_job_coefs(s.layout)};
        p.wide[SCALED_RGB] = scaled_rgb_job_wide(j);
        p.scaled_rgb_sw = s.src_w;
    } else if (s.kind == Source::RGB4) {
        RgbJob &j = p.rgb[p.n[RGB]++];
        j = RgbJob{s.plane[0], s.pitch[0], {dp[0].data, dp[1].data, dp[2].data}, dp[0].stride, dp[1].stride, dp[0].w, dp[0].h, hs, vs, rgb_job_coefs(s.layout)};
        p.wide[RGB] = rgb_job_wide(j);
    } else if (s.route == Source::SIZED) {
        for (int c = 0; c < 3; c++) { // (an interleaved plane: two records, its U and its V half)
            const int sp = semi && c == 2 ? 1 : c, pw = c ? scw : s.src_w, ph = c ? sch : s.src_h;
            SizedSurfaceJob &j = p.sized_surf[p.n[SIZED_SURF]++];
            j = SizedSurfaceJob{s.plane[sp], s.pitch[sp], dp[c].data, dp[c].stride, dp[c].w, dp[c].h, ingest_resize::sized_ratio(pw, ph, dp[c].w, dp[c].h, false),
                                (uint16_t) (semi && c ? 2 : 1), (uint16_t) (semi && c == 2 ? 1 : 0)};
            p.wide[SIZED_SURF] = p.wide[SIZED_SURF] && sized_job_wide(j, (size_t) (semi && c ? 2 * pw : pw));
        }
    } else if (s.route == Source::REDUCED) {
        for (int c = 0; c < (semi ? 2 : 3); c++) { // (an interleaved plane: one record, which writes both chroma planes)
            const bool uv = semi && c == 1;
            ScaledSurfaceJob &j = p.scaled_surf[p.n[SCALED_SURF]++];
            j = ScaledSurfaceJob{s.plane[c], s.pitch[c], dp[c].data, uv ? dp[2].data : nullptr, dp[c].stride, c ? scw : s.src_w, c ? sch : s.src_h, s.shift};
            p.wide[SCALED_SURF] = p.wide[SCALED_SURF] && scaled_surface_job_wide(j);
            const int row_bytes = uv ? 2 * j.pw : j.pw;
            p.scaled_row_bytes = row_bytes > p.scaled_row_bytes ? row_bytes : p.scaled_row_bytes;
        }
    } else {
        for (int c = 0; c < (semi ? 2 : 3); c++) {
            const bool uv = semi && c == 1;
            SurfaceJob &j = p.surf[p.n[SURF]++];
            j = SurfaceJob{s.plane[c], s.pitch[c], dp[c].data, uv ? dp[2].data : nullptr, dp[c].stride, dp[c].w, dp[c].h};
            p.wide[SURF] = p.wide[SURF] && surface_job_wide(j);
        }
    }
    return p;
}

} // namespace enc_ingest
} // namespace dsv2
