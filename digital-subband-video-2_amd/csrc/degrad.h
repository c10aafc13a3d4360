// degrad.h -- the de-gradient sharpening of one 4x4 cell in registers (reference src/bmc.c: degrad4x4, :277), shared by the in-loop
// filters and the decoder's post-processing (bmc.hip) and by the sharpening egress (egress.hip: k_egress).  Device code only.
#pragma once

#include "dev.h"

namespace dsv2 {

// n / d for 0 <= n < 2^12, 1 <= d <= 16 (sums of at most 16 pixels over their count): reciprocal estimate + one correction
__device__ __forceinline__ int div_small(int n, int d)
{
    int q = (int) ((float) n * __builtin_amdgcn_rcpf((float) d));
    int r = n - q * d;
    return r < 0 ? q - 1 : (r >= d ? q + 1 : q);
}

// one pixel of the de-gradient step (bmc.c:318-330), without branches: pulled towards the mean of the darkest / brightest
// bin by count / 16 (C division: towards zero; |count * difference| < 2^12, a 24-bit multiply)
__device__ __forceinline__ int degrad_px(int os, int t, int nlo, int alo, int nhi, int ahi)
{
    bool lt = os < t;
    int v = __mul24(lt ? nlo : nhi, (lt ? alo : ahi) - os);
    int adj = (v + ((v >> 31) & 15)) >> 4;
    return os == t ? os : (os + adj) & 0xff;
}

// de-gradient sharpening of 16 pixels px[y * 4 + x] in place (bmc.c:276); returns true when it changed them
__device__ __forceinline__ bool degrad16(int (&px)[16])
{
    int lo = 16, hi = -1;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        lo = min(lo, px[k] >> 4);
        hi = max(hi, px[k] >> 4);
    }
    if (lo >= hi) {
        return false;
    }
    int nlo = 0, nhi = 0, slo = 0, shi = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        int b = px[k] >> 4;
        if (b == lo) {
            nlo++;
            slo += px[k];
        }
        if (b == hi) {
            nhi++;
            shi += px[k];
        }
    }
    int alo = div_small(slo, nlo), ahi = div_small(shi, nhi);
    if (alo == 0) {
        alo = 1;
    }
    if (ahi == 0) {
        ahi = 1;
    }
    int t = (alo + ahi + 1) >> 1;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        px[k] = degrad_px(px[k], t, nlo, alo, nhi, ahi);
    }
    return true;
}

} // namespace dsv2
