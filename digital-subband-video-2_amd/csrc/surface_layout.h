// surface_layout.h -- the layout word of a surface that carries a scale (include/dsv2_hip.h, DSV2HIP_SCALE_*): ONE grammar for the
// decoder's out surfaces (dec_delivery.h) and for the encoder's scaled in surfaces (ingest_scale.h).  Free of any device call.
#pragma once

#include "../../include/dsv2_hip.h"

namespace dsv2 {
namespace delivery {

// the shift of a layout: 0, or 1 .. 3 for DSV2HIP_SCALE_HALF / _QUARTER / _EIGHTH; the layout without it
constexpr int kScaleMask = DSV2HIP_SCALE_EIGHTH; // (the three values are 1, 2, 3 << 12)
inline int layout_shift(int layout) { return (layout & kScaleMask) >> 12; }
inline int layout_unscaled(int layout) { return layout & ~kScaleMask; }

// an RGB layout: BGRA / RGBA or-ed with any subset of the DSV2HIP_CSC_* bits (the bits on PLANAR / SEMIPLANAR are no layout) and at
// most one DSV2HIP_SCALE_* value.  One value is held back: 0x1010, which reads as BGRA | BT601 | limited range | HALF, was refused as
// "no layout" before the scale values existed, callers and the RGB surface tests probe with it and rely on the refusal, and it stays
// refused (include/dsv2_hip.h): half-size BGRA takes any other preset (0x1110, 0x1210, 0x1310), or RGBA (0x1011).
inline bool is_rgb_layout(int layout)
{
    if (layout == (DSV2HIP_SURFACE_BGRA | DSV2HIP_SCALE_HALF)) {
        return false;
    }
    const int order = layout_unscaled(layout) & ~(DSV2HIP_CSC_BT709 | DSV2HIP_CSC_FULL_RANGE);
    return order == DSV2HIP_SURFACE_BGRA || order == DSV2HIP_SURFACE_RGBA;
}

} // namespace delivery
} // namespace dsv2
