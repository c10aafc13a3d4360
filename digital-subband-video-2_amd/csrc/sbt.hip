// sbt.hip -- multi-level integer subband transform on gfx950, forward and inverse.
//
// Replaces reference src/sbt.c: dsv_fwd_sbt (:848) / dsv_inv_sbt (:890) and the
// filters they dispatch to (Haar fwd/inv/inv_simple :547/:686/:616, LLI/LLP :279-338,
// CC :341-356, adaptive L2 :359-382, ASF93 L1 :390-429, lossless 5/3 :432-447).
//
// Decomposition (proved bit-exact on the CPU by oracle/orc_sbt.c):
//   * every 1-D lifting filter is evaluated in closed form from the unmodified input
//     vector (a lifting step only reads samples of the other parity), so each output
//     pair is an independent work item: no serial in-place loops;
//   * the shrinking LL band ping-pongs between two scratch images; the three high
//     bands of each level are stored once, directly at their final Mallat position;
//   * level 1 reads the u8 picture directly (fused "p2sbc", sbt.c:799) and the last
//     inverse level stores clamped u8 pixels (fused "sbc2p", sbt.c:817).
// Work mapping: threadIdx.x runs along image x (coalesced rows), 64 x 4 threads per
// workgroup = 4 wavefronts; grids are >> 256 workgroups on the full-resolution levels.
#include "dev.h"
#include "prio.h"

namespace dsv2 {

enum { F_HAAR = 0, F_LLI, F_LLP, F_CC, F_L2A, F_L1, F_LOSSLESS };

static inline int host_lb2(unsigned n)
{
    unsigned i = 1;
    int l = 0;
    while (i < n) {
        i <<= 1;
        l++;
    }
    return l;
}

static inline int rshift_up(int x, int s) { return (x + (1 << s) - 1) >> s; }

static int pick_filter(int plane, int isP, int lossless, int l, int lvls) // sbt.c:22-29, 862-885
{
    if (lossless) {
        return (l >= 1 && l <= lvls - 2) ? F_LOSSLESS : F_HAAR;
    }
    if (plane == 0) {
        if (l == 4) {
            return isP ? F_LLP : F_LLI;
        }
        if (!isP && l == 2) {
            return F_L2A;
        }
        if (!isP && l == 1) {
            return F_L1;
        }
        return F_HAAR;
    }
    if (!isP && l >= 1 && l <= lvls - 2) {
        return F_CC;
    }
    return F_HAAR;
}

__device__ __forceinline__ int sar(int v, int s) { return v >> s; } // arithmetic on AMDGPU
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int reflect_idx(int i, int nm1)
{
    if (i < 0) {
        i = -i;
    }
    if (i >= nm1) {
        i = nm1 + nm1 - i;
    }
    return i;
}

// ---- input vector views -------------------------------------------------------
struct VecI { // strided int32 vector
    const int32_t *p;
    int s, n;
    // n == 1 (a dimension that has collapsed while the other still has levels to go): what the reference's update step
    // v[0] += v[s] >> 1 (sbt.c:200, 222) reads next to the vector -- the previous level's high band at its final place in the
    // coefficient plane, beside a row, below a column (for a column the reference finds it in row 1 of its scratch image, left
    // there by the level that was two rows high)
    const int32_t *past;
    __device__ __forceinline__ int operator()(int i) const { return p[i * s]; }
    __device__ __forceinline__ int beyond() const { return *past; }
};
struct VecU8 { // row of the u8 picture, centred on zero; rows below the picture are zero
    const uint8_t *p;
    int n;
    bool live;
    __device__ __forceinline__ int operator()(int i) const { return live ? (int) p[i] - 128 : 0; }
    __device__ __forceinline__ int beyond() const { return 0; } // (level 1 is never one sample long)
};

// adaptive tap selection walk (sbt.c:227-238, 392-405): flag byte of walk index t
struct Ring {
    const uint8_t *sb;
    int delta2, sbs;
    __device__ __forceinline__ bool at(int t) const
    {
        return (sb[((t * delta2) >> kBlockP) * sbs] & DSV_IS_RINGING) != 0;
    }
};

// ---- 1-D analysis, closed form --------------------------------------------------
template <class V> __device__ __forceinline__ int hi3(const V &v, int i)
{
    if (i < v.n - 1) {
        return v(i) - ((v(i - 1) + v(i + 1) + 1) >> 1);
    }
    return v(i) - v(i - 1);
}

// the high-pass sample that the first update step reads
template <class V> __device__ __forceinline__ int first_hi(const V &v) { return v.n > 1 ? hi3(v, 1) : v.beyond(); }

template <class V> __device__ __forceinline__ int lo3(const V &v, int i)
{
    int even_n = v.n & ~1;
    if (i == 0) {
        return v(0) + (first_hi(v) >> 1);
    }
    if (i >= even_n) {
        return v(i);
    }
    return v(i) + ((hi3(v, i - 1) + hi3(v, i + 1) + 2) >> 2);
}

template <class V> __device__ __forceinline__ int lo5(const V &v, int i, int c0, int ca, int cs)
{
    int even_n = v.n & ~1, nm1 = v.n - 1;
    if (i == 0) {
        return v(0) + (first_hi(v) >> 1);
    }
    if (i >= even_n) {
        return v(i);
    }
    return v(i) + ((-hi3(v, reflect_idx(i - 3, nm1)) + c0 * (hi3(v, i - 1) + hi3(v, i + 1)) -
                    hi3(v, reflect_idx(i + 3, nm1)) + ca) >> cs);
}

template <class V> __device__ __forceinline__ int rgx(const V &v, int i) { return v(reflect_idx(i, v.n - 1)); }

template <class V> __device__ __forceinline__ void l1_pair(const V &v, const Ring &r, int k, int &L, int &H)
{
    int n = v.n, i = 2 * k;
    if (k == 0) {
        int h = hi3(v, 1);
        L = 2 * (v(0) + (h >> 1));
        H = 4 * h;
        return;
    }
    if (i == n - 2) {
        int h0 = hi3(v, n - 3), h1 = hi3(v, n - 1);
        L = 2 * (v(n - 2) + ((h0 + h1 + 2) >> 2));
        H = 4 * h1;
        return;
    }
    int x0 = rgx(v, i), a1 = rgx(v, i - 1) + rgx(v, i + 1), a2 = rgx(v, i - 2) + rgx(v, i + 2);
    int a3 = rgx(v, i - 3) + rgx(v, i + 3), a4 = rgx(v, i - 4) + rgx(v, i + 4);
    int lo = r.at(k) ? (46 * x0 + 20 * a1 - 9 * a2 - 4 * a3 + 2 * a4) : (46 * x0 + 19 * a1 - 8 * a2 - 3 * a3 + a4);
    int hi = 32 * rgx(v, i + 1) - 16 * (x0 + rgx(v, i + 2));
    L = (lo + 16) >> 5;
    H = (hi + 4) >> 3;
}

template <int F, class V> __device__ __forceinline__ void analysis_pair(const V &v, const Ring &r, int k, int &L, int &H)
{
    int i = 2 * k;
    if (F == F_L1) {
        l1_pair(v, r, k, L, H);
        return;
    }
    int hi = ((i + 1) < v.n) ? hi3(v, i + 1) : 0;
    int lo;
    if (F == F_LLI) {
        lo = lo3(v, i) * 5 / 2;
        hi *= 4;
    } else if (F == F_LLP) {
        lo = lo3(v, i) * 5 / 2;
        hi *= 2;
    } else if (F == F_CC) {
        lo = lo5(v, i, 3, 8, 4) * 2;
    } else if (F == F_L2A) {
        bool ring = (i >= 2 && i < (v.n & ~1)) ? r.at(k - 1) : false;
        lo = (ring ? lo5(v, i, 3, 4, 3) : lo5(v, i, 9, 16, 5)) * 2;
        hi *= 3;
        hi = hi - sar(hi, 3);
    } else {
        lo = lo3(v, i);
    }
    L = lo;
    H = hi;
}

// ---- 1-D synthesis, closed form -------------------------------------------------
struct Syn {
    const int32_t *lo; // low(k)  = lo[k * s]
    const int32_t *hi; // high(k) = hi[k * s]
    int s, n;
    // n == 1: what out[0] -= out[s] >> 1 reads, unscaled: the coefficient beside a row, below a column (see VecI.  For a column
    // the reference reads its scratch image, which holds that coefficient only straight after the forward transform of the same
    // plane and anything otherwise: tests/edge_cases.py, inverse_reads_stale_scratch)
    const int32_t *past;
};

template <int F> __device__ __forceinline__ int even_raw(const Syn &v, int k)
{
    int a = v.lo[k * v.s];
    if (F == F_LLI || F == F_LLP) {
        return a * 2 / 5;
    }
    if (F == F_CC || F == F_L2A || F == F_L1) {
        return a / 2;
    }
    return a;
}

template <int F> __device__ __forceinline__ int odd_raw(const Syn &v, int k)
{
    int a = v.hi[k * v.s];
    if (F == F_LLI || F == F_L1) {
        return a / 4;
    }
    if (F == F_LLP) {
        return a / 2;
    }
    if (F == F_L2A) {
        a = a / 3;
        return a + sar(a, 3);
    }
    return a;
}

template <int F> __device__ __forceinline__ int syn_even(const Syn &v, const Ring &r, int k)
{
    int i = 2 * k, n = v.n, even_n = n & ~1, nm1 = n - 1;
    int e = even_raw<F>(v, k);
    if (i == 0) {
        return e - ((n > 1 ? odd_raw<F>(v, 0) : *v.past) >> 1);
    }
    if (i >= even_n) {
        return e;
    }
    if (F == F_CC || F == F_L2A) {
        int c0 = 3, ca = 8, cs = 4;
        if (F == F_L2A) {
            if (r.at(k - 1)) {
                c0 = 3, ca = 4, cs = 3;
            } else {
                c0 = 9, ca = 16, cs = 5;
            }
        }
        return e - ((-odd_raw<F>(v, reflect_idx(i - 3, nm1) >> 1) + c0 * (odd_raw<F>(v, k - 1) + odd_raw<F>(v, k)) -
                     odd_raw<F>(v, reflect_idx(i + 3, nm1) >> 1) + ca) >> cs);
    }
    return e - ((odd_raw<F>(v, k - 1) + odd_raw<F>(v, k) + 2) >> 2);
}

// both samples of output pair k: x[2k] and (if it exists) x[2k+1]
template <int F> __device__ __forceinline__ void synthesis_pair(const Syn &v, const Ring &r, int k, int &xe, int &xo)
{
    int n = v.n, i = 2 * k + 1;
    int e0 = syn_even<F>(v, r, k);
    xe = e0;
    xo = 0;
    if (i >= n) {
        return;
    }
    int o = odd_raw<F>(v, k);
    if (i < n - 1) {
        if (F == F_L1 && (n & 1) && i == n - 2) {
            xo = o; // sbt.c:205-213 never updates it for odd n
        } else {
            xo = o + ((e0 + syn_even<F>(v, r, k + 1) + 1) >> 1);
        }
    } else {
        xo = o + e0;
    }
}

// ---- kernels ----------------------------------------------------------------------
// Every kernel works through PlaneJob records: blockIdx.z indexes a device table (one entry per stream
// and plane of a lockstep batch; all entries share the geometry `g`).  Images are named by selector: 0..2 = the job's scratch images, 3 = its
// coefficient plane.
struct LevelGeom {
    int w;      // row stride of every int32 image (= coefficient plane width)
    int sw, sh; // size of the LL image being analysed / synthesised at this level
    int hw, hh; // ceil halves
    int use_bd; // adaptive filter: consult the job's block flag bytes
    int nbh;
    int dbx, dby;
};

enum { IMG_COEFS = 3 };

__device__ __forceinline__ int32_t *img(const PlaneJob &J, int sel) { return sel == IMG_COEFS ? J.coefs : J.t[sel]; }

template <int F, bool U8>
__global__ __launch_bounds__(256) void k_fwd_rows(const PlaneJob *__restrict__ tab, LevelGeom g, int s_sel)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    int k = blockIdx.x * 64 + threadIdx.x;
    int j = blockIdx.y * 4 + threadIdx.y;
    if (k >= g.hw || j >= g.sh) {
        return;
    }
    int32_t *R = J.t[2];
    Ring r{g.use_bd ? J.bd + ((j * g.dby) >> kBlockP) * g.nbh : nullptr, 2 * g.dbx, 1};
    int L, H;
    if (U8) {
        VecU8 v{J.pic.data + (size_t) j * J.pic.stride, g.sw, j < J.pic.h};
        analysis_pair<F>(v, r, k, L, H);
    } else {
        VecI v{img(J, s_sel) + (size_t) j * g.w, 1, g.sw, J.coefs + (size_t) j * g.w + 1};
        analysis_pair<F>(v, r, k, L, H);
    }
    R[(size_t) j * g.w + k] = L;
    if (2 * k + 1 < g.sw) {
        R[(size_t) j * g.w + g.hw + k] = H;
    }
}

template <int F>
__global__ __launch_bounds__(256) void k_fwd_cols(const PlaneJob *__restrict__ tab, LevelGeom g, int d_sel)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    int i = blockIdx.x * 64 + threadIdx.x;
    int k = blockIdx.y * 4 + threadIdx.y;
    if (i >= g.sw || k >= g.hh) {
        return;
    }
    int32_t *D = img(J, d_sel), *C = J.coefs;
    Ring r{g.use_bd ? J.bd + ((i * g.dbx) >> kBlockP) : nullptr, 2 * g.dby, g.nbh};
    VecI v{J.t[2] + i, g.w, g.sh, C + g.w + i};
    int L, H;
    analysis_pair<F>(v, r, k, L, H);
    if (i < g.hw) {
        D[(size_t) k * g.w + i] = L;
    } else {
        C[(size_t) k * g.w + i] = L;
    }
    if (2 * k + 1 < g.sh) {
        C[(size_t) (g.hh + k) * g.w + i] = H;
    }
}

template <bool U8>
__device__ __forceinline__ void fwd_haar_quad(const PlaneJob &J, const LevelGeom &g, int idx, int jy, int s_sel, int d_sel, int ovf)
{
    int32_t *D = img(J, d_sel), *C = J.coefs;
    int x = 2 * idx, y = 2 * jy;
    bool hasx = (x + 1) < g.sw, hasy = (y + 1) < g.sh;
    int x0, x1 = 0, x2 = 0, x3 = 0;
    if (U8) {
        int ustride = J.pic.stride, ph = J.pic.h;
        const uint8_t *r0 = J.pic.data + (size_t) y * ustride + x;
        const uint8_t *r1 = r0 + ustride;
        bool l0 = y < ph, l1 = (y + 1) < ph;
        x0 = l0 ? (int) r0[0] - 128 : 0;
        if (hasx) {
            x1 = l0 ? (int) r0[1] - 128 : 0;
        }
        if (hasy) {
            x2 = l1 ? (int) r1[0] - 128 : 0;
            if (hasx) {
                x3 = l1 ? (int) r1[1] - 128 : 0;
            }
        }
    } else {
        const int32_t *r0 = img(J, s_sel) + (size_t) y * g.w + x;
        x0 = r0[0];
        if (hasx) {
            x1 = r0[1];
        }
        if (hasy) {
            x2 = r0[g.w];
            if (hasx) {
                x3 = r0[g.w + 1];
            }
        }
    }
    int dv = ovf ? 2 : 1;
    size_t oLL = (size_t) jy * g.w + idx, oHL = (size_t) (g.hh + jy) * g.w + idx;
    if (hasx && hasy) {
        D[oLL] = (x0 + x1 + x2 + x3) / dv;
        C[oLL + g.hw] = x0 - x1 + x2 - x3;
        C[oHL] = x0 + x1 - x2 - x3;
        C[oHL + g.hw] = x0 - x1 - x2 + x3;
    } else if (hasy) {
        D[oLL] = 2 * (x0 + x2) / dv;
        C[oHL] = 2 * (x0 - x2);
    } else if (hasx) {
        D[oLL] = 2 * (x0 + x1) / dv;
        C[oLL + g.hw] = 2 * (x0 - x1);
    } else {
        D[oLL] = (x0 * 4) / dv;
    }
}

template <bool U8>
__global__ __launch_bounds__(256) void k_fwd_haar(const PlaneJob *__restrict__ tab, LevelGeom g, int s_sel,
                                                  int d_sel, int ovf)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    int idx = blockIdx.x * 64 + threadIdx.x;
    int jy = blockIdx.y * 4 + threadIdx.y;
    if (idx >= g.hw || jy >= g.hh) {
        return;
    }
    fwd_haar_quad<U8>(J, g, idx, jy, s_sel, d_sel, ovf);
}

// levels above 1, four quads per thread (round 6): the int32 image's two rows as four 16-byte loads, one 16-byte store per band,
// two quad rows per thread with every load issued up front.  The quad-per-thread kernel above moved 4 bytes per lane and load:
// at a third of level 1's work the levels 2 .. 3 took as long under load.  Launched when the level's half width and the row
// stride are multiples of four; edge threads and unaligned jobs go quad by quad.
constexpr int kHaarRowsI = 1;
__global__ __launch_bounds__(256) void k_fwd_haar_i32x4(const PlaneJob *__restrict__ tab, LevelGeom g, int s_sel, int d_sel, int ovf)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    const int idx = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int jy0 = blockIdx.y * (4 * kHaarRowsI) + threadIdx.y;
    if (idx >= g.hw || jy0 >= g.hh) {
        return;
    }
    int32_t *D = img(J, d_sel), *C = J.coefs;
    const int32_t *S = img(J, s_sel);
    const int x = 2 * idx;
    const bool fastx = x + 8 <= g.sw && ((((uintptr_t) D) | ((uintptr_t) C) | ((uintptr_t) S)) & 15) == 0;
    int4 a0[kHaarRowsI], a1[kHaarRowsI], b0[kHaarRowsI], b1[kHaarRowsI];
    const int4 z4 = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < kHaarRowsI; r++) {
        const int jy = jy0 + 4 * r, y = 2 * jy;
        const bool f = fastx && jy < g.hh && y + 2 <= g.sh;
        const int32_t *r0 = S + (size_t) (f ? y : 0) * g.w + x;
        a0[r] = f ? *(const int4 *) r0 : z4;
        a1[r] = f ? *(const int4 *) (r0 + 4) : z4;
        b0[r] = f ? *(const int4 *) (r0 + g.w) : z4;
        b1[r] = f ? *(const int4 *) (r0 + g.w + 4) : z4;
    }
#pragma unroll
    for (int r = 0; r < kHaarRowsI; r++) {
        const int jy = jy0 + 4 * r, y = 2 * jy;
        if (jy >= g.hh) {
            // (nothing: past the level's last quad row)
        } else if (!(fastx && y + 2 <= g.sh)) {
            for (int q = 0; q < 4 && idx + q < g.hw; q++) {
                fwd_haar_quad<false>(J, g, idx + q, jy, s_sel, d_sel, ovf);
            }
        } else {
        const int ta[8] = {a0[r].x, a0[r].y, a0[r].z, a0[r].w, a1[r].x, a1[r].y, a1[r].z, a1[r].w};
        const int tb[8] = {b0[r].x, b0[r].y, b0[r].z, b0[r].w, b1[r].x, b1[r].y, b1[r].z, b1[r].w};
        int ll[4], lh[4], hl[4], hh[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int x0 = ta[2 * q], x1 = ta[2 * q + 1], x2 = tb[2 * q], x3 = tb[2 * q + 1];
            ll[q] = ovf ? (x0 + x1 + x2 + x3) / 2 : (x0 + x1 + x2 + x3);
            lh[q] = x0 - x1 + x2 - x3;
            hl[q] = x0 + x1 - x2 - x3;
            hh[q] = x0 - x1 - x2 + x3;
        }
        const size_t oLL = (size_t) jy * g.w + idx, oHL = (size_t) (g.hh + jy) * g.w + idx;
        *(int4 *) (D + oLL) = make_int4(ll[0], ll[1], ll[2], ll[3]);
        *(int4 *) (C + oLL + g.hw) = make_int4(lh[0], lh[1], lh[2], lh[3]);
        *(int4 *) (C + oHL) = make_int4(hl[0], hl[1], hl[2], hl[3]);
        *(int4 *) (C + oHL + g.hw) = make_int4(hh[0], hh[1], hh[2], hh[3]);
        }
    }
}

// level 1 from the 8-bit picture, four 2x2 quads (eight pixels of two rows) per thread: two 8-byte loads, four 16-byte
// stores (one per band).  Launched when the level's half width and the row stride are multiples of four; threads at the
// picture's right / bottom edge, and jobs whose images are not 16-byte aligned, go quad by quad.
constexpr int kHaarRows = 2; // output rows per thread (jy, jy + 4): both row pairs' loads are issued before the first is used (four rows: 60 registers, a wavefront per SIMD fewer under load, no faster)
__global__ __launch_bounds__(256) void k_fwd_haar_u8x4(const PlaneJob *__restrict__ tab, LevelGeom g, int d_sel, int ovf)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    const int idx = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int jy0 = blockIdx.y * (4 * kHaarRows) + threadIdx.y;
    if (idx >= g.hw || jy0 >= g.hh) {
        return;
    }
    int32_t *D = img(J, d_sel), *C = J.coefs;
    const int x = 2 * idx;
    const bool fastx = x + 8 <= min(g.sw, J.pic.w) && ((((uintptr_t) D) | ((uintptr_t) C)) & 15) == 0 &&
                       (((uintptr_t) J.pic.data | (uintptr_t) J.pic.stride) & 7) == 0;
    uint2 a[kHaarRows], b[kHaarRows];
    bool fast[kHaarRows];
#pragma unroll
    for (int r = 0; r < kHaarRows; r++) {
        const int jy = jy0 + 4 * r, y = 2 * jy;
        fast[r] = fastx && jy < g.hh && y + 2 <= min(g.sh, J.pic.h);
        const uint8_t *r0 = J.pic.data + (size_t) (fast[r] ? y : 2 * jy0) * J.pic.stride + x;
        a[r] = fastx ? *(const uint2 *) r0 : make_uint2(0u, 0u);
        b[r] = fast[r] ? *(const uint2 *) (r0 + J.pic.stride) : make_uint2(0u, 0u);
    }
#pragma unroll
    for (int r = 0; r < kHaarRows; r++) {
        const int jy = jy0 + 4 * r;
        if (jy >= g.hh) {
            break;
        }
        if (!fast[r]) {
            for (int q = 0; q < 4 && idx + q < g.hw; q++) {
                fwd_haar_quad<true>(J, g, idx + q, jy, 0, d_sel, ovf);
            }
            continue;
        }
        const uint32_t aw[2] = {a[r].x, a[r].y}, bw[2] = {b[r].x, b[r].y};
        int ll[4], lh[4], hl[4], hh[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t wa = aw[q >> 1] >> (16 * (q & 1)), wb = bw[q >> 1] >> (16 * (q & 1));
            const int x0 = (int) (wa & 0xffu) - 128, x1 = (int) ((wa >> 8) & 0xffu) - 128;
            const int x2 = (int) (wb & 0xffu) - 128, x3 = (int) ((wb >> 8) & 0xffu) - 128;
            ll[q] = ovf ? (x0 + x1 + x2 + x3) / 2 : (x0 + x1 + x2 + x3);
            lh[q] = x0 - x1 + x2 - x3;
            hl[q] = x0 + x1 - x2 - x3;
            hh[q] = x0 - x1 - x2 + x3;
        }
        const size_t oLL = (size_t) jy * g.w + idx, oHL = (size_t) (g.hh + jy) * g.w + idx;
        *(int4 *) (D + oLL) = make_int4(ll[0], ll[1], ll[2], ll[3]);
        *(int4 *) (C + oLL + g.hw) = make_int4(lh[0], lh[1], lh[2], lh[3]);
        *(int4 *) (C + oHL) = make_int4(hl[0], hl[1], hl[2], hl[3]);
        *(int4 *) (C + oHL + g.hw) = make_int4(hh[0], hh[1], hh[2], hh[3]);
    }
}

// (v + (v < 0 ? -1 : 1)) / 2 and (v + (v < 0 ? -2 : 2)) / 4 with C's truncating division (sbt.c:94-104), as three instructions
// each: for v < 0 the truncated quotient of v - r is the floored quotient of v + r - 1
__device__ __forceinline__ int round2(int v) { return (v + 1 + (v >> 31)) >> 1; }
__device__ __forceinline__ int round4(int v) { return (v + 2 + (v >> 31)) >> 2; }

__device__ __forceinline__ int nudge(int LL, int lp, int ln, int band, int hqp) // sbt.c:723-741
{
    int mx = LL - ln, mn = lp - LL;
    if (mn > mx) {
        int t = mn;
        mn = mx;
        mx = t;
    }
    mx = min(mx, 0);
    mn = max(mn, 0);
    if (mx != mn) {
        int t = round4(lp - ln);
        int nd = round2(clampi(t, mx, mn) - band * 2);
        band += clampi(nd, -hqp, hqp);
    }
    return band;
}

// v * (1 << ovf) (sbt.c:717: the LL band's overflow guard) as a shift: a 32-bit vector multiply is a quarter-rate instruction, and the
// four-quad kernels scale fourteen values per thread
__device__ __forceinline__ int shl_ovf(int v, int ovf) { return (int) ((unsigned) v << ovf); }

__device__ __forceinline__ uint8_t to_px(int v) { return (uint8_t) clampi(v + 128, 0, 255); }

// ll_sel: image holding the LL quadrant of this level; the coefficient plane holds the high bands.
// hdiv: the smoothing clamp is the job's quantiser / hdiv (sbt.c:903)
template <bool OUT_U8>
__device__ __forceinline__ void inv_haar_quad(const PlaneJob &J, const LevelGeom &g, int idx, int jy, int ll_sel, int d_sel, int ovf,
                                              int filtered, int hdiv)
{
    const int32_t *LLp = img(J, ll_sel), *C = J.coefs;
    int hqp = J.q / hdiv;
    int x = 2 * idx, y = 2 * jy;
    bool hasx = (x + 1) < g.sw, hasy = (y + 1) < g.sh;
    size_t oLL = (size_t) jy * g.w + idx, oHL = (size_t) (g.hh + jy) * g.w + idx;
    int LL = LLp[oLL] * (1 << ovf);
    int v00, v01 = 0, v10 = 0, v11 = 0;
    if (hasx && hasy) {
        int LH = C[oLL + g.hw], HL = C[oHL], HH = C[oHL + g.hw];
        if (filtered) {
            if (idx > 0) {
                int lp = LLp[oLL - 1] * (1 << ovf);
                // the reference reads one past the LL row for the last pair (sbt.c:715,725): that is
                // the first LH coefficient of the row when the level width is even
                int ln = ((idx + 1 < g.hw) ? LLp[oLL + 1] : C[oLL + 1]) * (1 << ovf);
                LH = nudge(LL, lp, ln, LH, hqp);
            }
            if (jy > 0) {
                int lp = LLp[oLL - g.w] * (1 << ovf);
                int ln = ((jy + 1 < g.hh) ? LLp[oLL + g.w] : C[oLL + g.w]) * (1 << ovf);
                HL = nudge(LL, lp, ln, HL, hqp);
            }
        }
        v00 = (LL + LH + HL + HH) / 4;
        v01 = (LL - LH + HL - HH) / 4;
        v10 = (LL + LH - HL - HH) / 4;
        v11 = (LL - LH - HL + HH) / 4;
    } else if (hasy) {
        int HL = C[oHL];
        v00 = (LL + HL) / 4;
        v10 = (LL - HL) / 4;
    } else if (hasx) {
        int LH = C[oLL + g.hw];
        v00 = (LL + LH) / 4;
        v01 = (LL - LH) / 4;
    } else {
        v00 = LL / 4;
    }
    if (OUT_U8) {
        int ustride = J.pic.stride, pw = J.pic.w, ph = J.pic.h;
        uint8_t *r0 = J.pic.data + (size_t) y * ustride + x;
        if (y < ph) {
            if (x < pw) {
                r0[0] = to_px(v00);
            }
            if (hasx && x + 1 < pw) {
                r0[1] = to_px(v01);
            }
        }
        if (hasy && y + 1 < ph) {
            if (x < pw) {
                r0[ustride] = to_px(v10);
            }
            if (hasx && x + 1 < pw) {
                r0[ustride + 1] = to_px(v11);
            }
        }
    } else {
        int32_t *r0 = J.t[d_sel] + (size_t) y * g.w + x;
        r0[0] = v00;
        if (hasx) {
            r0[1] = v01;
        }
        if (hasy) {
            r0[g.w] = v10;
            if (hasx) {
                r0[g.w + 1] = v11;
            }
        }
    }
}

template <bool OUT_U8>
__global__ __launch_bounds__(256) void k_inv_haar(const PlaneJob *__restrict__ tab, LevelGeom g, int ll_sel,
                                                  int d_sel, int ovf, int filtered, int hdiv)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    int idx = blockIdx.x * 64 + threadIdx.x;
    int jy = blockIdx.y * 4 + threadIdx.y;
    if (idx >= g.hw || jy >= g.hh) {
        return;
    }
    inv_haar_quad<OUT_U8>(J, g, idx, jy, ll_sel, d_sel, ovf, filtered, hdiv);
}

// level 1 to the 8-bit picture, four quads per thread: 16-byte loads of the four bands (and of the LL rows above and
// below for the smoothing), two 8-byte pixel stores.  Interior threads only; the rest goes quad by quad.
__global__ __launch_bounds__(256) void k_inv_haar_u8x4(const PlaneJob *__restrict__ tab, LevelGeom g, int ll_sel, int ovf,
                                                       int filtered, int hdiv)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    const int idx = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int jy = blockIdx.y * 4 + threadIdx.y;
    if (idx >= g.hw || jy >= g.hh) {
        return;
    }
    const int32_t *LLp = img(J, ll_sel), *C = J.coefs;
    const int x = 2 * idx, y = 2 * jy;
    const bool fast = idx > 0 && idx + 4 < g.hw && jy > 0 && jy + 1 < g.hh && x + 8 <= min(g.sw, J.pic.w) && y + 2 <= min(g.sh, J.pic.h) &&
                      ((((uintptr_t) LLp) | ((uintptr_t) C)) & 15) == 0 && (((uintptr_t) J.pic.data | (uintptr_t) J.pic.stride) & 7) == 0;
    if (!fast) {
        for (int q = 0; q < 4 && idx + q < g.hw; q++) {
            inv_haar_quad<true>(J, g, idx + q, jy, ll_sel, 0, ovf, filtered, hdiv);
        }
        return;
    }
    const int hqp = J.q / hdiv;
    const size_t oLL = (size_t) jy * g.w + idx, oHL = (size_t) (g.hh + jy) * g.w + idx;
    const int4 l4 = *(const int4 *) (LLp + oLL), lh4 = *(const int4 *) (C + oLL + g.hw), hl4 = *(const int4 *) (C + oHL),
               hh4 = *(const int4 *) (C + oHL + g.hw);
    const int L[6] = {filtered ? shl_ovf(LLp[oLL - 1], ovf) : 0, shl_ovf(l4.x, ovf), shl_ovf(l4.y, ovf), shl_ovf(l4.z, ovf), shl_ovf(l4.w, ovf),
                      filtered ? shl_ovf(LLp[oLL + 4], ovf) : 0};
    int LH[4] = {lh4.x, lh4.y, lh4.z, lh4.w}, HL[4] = {hl4.x, hl4.y, hl4.z, hl4.w};
    const int HH[4] = {hh4.x, hh4.y, hh4.z, hh4.w};
    if (filtered) {
        const int4 u4 = *(const int4 *) (LLp + oLL - g.w), d4 = *(const int4 *) (LLp + oLL + g.w);
        const int U[4] = {shl_ovf(u4.x, ovf), shl_ovf(u4.y, ovf), shl_ovf(u4.z, ovf), shl_ovf(u4.w, ovf)};
        const int Dn[4] = {shl_ovf(d4.x, ovf), shl_ovf(d4.y, ovf), shl_ovf(d4.z, ovf), shl_ovf(d4.w, ovf)};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            LH[q] = nudge(L[q + 1], L[q], L[q + 2], LH[q], hqp);
            HL[q] = nudge(L[q + 1], U[q], Dn[q], HL[q], hqp);
        }
    }
    uint32_t r0w[2] = {0, 0}, r1w[2] = {0, 0};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int LL = L[q + 1];
        const uint32_t v00 = to_px((LL + LH[q] + HL[q] + HH[q]) / 4), v01 = to_px((LL - LH[q] + HL[q] - HH[q]) / 4);
        const uint32_t v10 = to_px((LL + LH[q] - HL[q] - HH[q]) / 4), v11 = to_px((LL - LH[q] - HL[q] + HH[q]) / 4);
        r0w[q >> 1] |= (v00 | (v01 << 8)) << (16 * (q & 1));
        r1w[q >> 1] |= (v10 | (v11 << 8)) << (16 * (q & 1));
    }
    uint8_t *r0 = J.pic.data + (size_t) y * J.pic.stride + x;
    *(uint2 *) r0 = make_uint2(r0w[0], r0w[1]);
    *(uint2 *) (r0 + J.pic.stride) = make_uint2(r1w[0], r1w[1]);
}

// levels above 1, four quads per thread to the int32 image (round 6): k_inv_haar_u8x4's loads, four 16-byte stores.  Interior
// threads only; the rest goes quad by quad.
__global__ __launch_bounds__(256) void k_inv_haar_i32x4(const PlaneJob *__restrict__ tab, LevelGeom g, int ll_sel, int d_sel, int ovf,
                                                        int filtered, int hdiv)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    const int idx = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int jy = blockIdx.y * 4 + threadIdx.y;
    if (idx >= g.hw || jy >= g.hh) {
        return;
    }
    const int32_t *LLp = img(J, ll_sel), *C = J.coefs;
    int32_t *O = J.t[d_sel];
    const int x = 2 * idx, y = 2 * jy;
    const bool fast = idx > 0 && idx + 4 < g.hw && jy > 0 && jy + 1 < g.hh && x + 8 <= g.sw && y + 2 <= g.sh &&
                      ((((uintptr_t) LLp) | ((uintptr_t) C) | ((uintptr_t) O)) & 15) == 0;
    if (!fast) {
        for (int q = 0; q < 4 && idx + q < g.hw; q++) {
            inv_haar_quad<false>(J, g, idx + q, jy, ll_sel, d_sel, ovf, filtered, hdiv);
        }
        return;
    }
    const int hqp = J.q / hdiv;
    const size_t oLL = (size_t) jy * g.w + idx, oHL = (size_t) (g.hh + jy) * g.w + idx;
    const int4 l4 = *(const int4 *) (LLp + oLL), lh4 = *(const int4 *) (C + oLL + g.hw), hl4 = *(const int4 *) (C + oHL),
               hh4 = *(const int4 *) (C + oHL + g.hw);
    const int L[6] = {filtered ? shl_ovf(LLp[oLL - 1], ovf) : 0, shl_ovf(l4.x, ovf), shl_ovf(l4.y, ovf), shl_ovf(l4.z, ovf), shl_ovf(l4.w, ovf),
                      filtered ? shl_ovf(LLp[oLL + 4], ovf) : 0};
    int LH[4] = {lh4.x, lh4.y, lh4.z, lh4.w}, HL[4] = {hl4.x, hl4.y, hl4.z, hl4.w};
    const int HH[4] = {hh4.x, hh4.y, hh4.z, hh4.w};
    if (filtered) {
        const int4 u4 = *(const int4 *) (LLp + oLL - g.w), d4 = *(const int4 *) (LLp + oLL + g.w);
        const int U[4] = {shl_ovf(u4.x, ovf), shl_ovf(u4.y, ovf), shl_ovf(u4.z, ovf), shl_ovf(u4.w, ovf)};
        const int Dn[4] = {shl_ovf(d4.x, ovf), shl_ovf(d4.y, ovf), shl_ovf(d4.z, ovf), shl_ovf(d4.w, ovf)};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            LH[q] = nudge(L[q + 1], L[q], L[q + 2], LH[q], hqp);
            HL[q] = nudge(L[q + 1], U[q], Dn[q], HL[q], hqp);
        }
    }
    int r0v[8], r1v[8];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int LL = L[q + 1];
        r0v[2 * q] = (LL + LH[q] + HL[q] + HH[q]) / 4;
        r0v[2 * q + 1] = (LL - LH[q] + HL[q] - HH[q]) / 4;
        r1v[2 * q] = (LL + LH[q] - HL[q] - HH[q]) / 4;
        r1v[2 * q + 1] = (LL - LH[q] - HL[q] + HH[q]) / 4;
    }
    int32_t *r0 = O + (size_t) y * g.w + x;
    *(int4 *) r0 = make_int4(r0v[0], r0v[1], r0v[2], r0v[3]);
    *(int4 *) (r0 + 4) = make_int4(r0v[4], r0v[5], r0v[6], r0v[7]);
    *(int4 *) (r0 + g.w) = make_int4(r1v[0], r1v[1], r1v[2], r1v[3]);
    *(int4 *) (r0 + g.w + 4) = make_int4(r1v[4], r1v[5], r1v[6], r1v[7]);
}

// ---- the Haar tail of a plane in ONE launch --------------------------------------------------------------------
// From the level whose LL output fits in LDS down to the 1x1 top every level is Haar (pick_filter) and tiny: ten
// launches of ~15 us per direction and plane kind.  One workgroup per job walks them all, the LL images ping-ponging
// between two LDS buffers; the detail bands go to / come from the coefficient plane exactly as in the per-level kernels.
__device__ __forceinline__ LevelGeom tail_geom(int cw, int ch, int l)
{
    LevelGeom g;
    g.w = cw;
    g.sw = (cw + (1 << (l - 1)) - 1) >> (l - 1);
    g.sh = (ch + (1 << (l - 1)) - 1) >> (l - 1);
    g.hw = (g.sw + 1) / 2;
    g.hh = (g.sh + 1) / 2;
    g.use_bd = 0;
    g.nbh = g.dbx = g.dby = 0;
    return g;
}

// one forward quad: source image (src, ss), LL destination (dll, ds), detail bands into the coefficient plane C
__device__ __forceinline__ void fwd_haar_quad_p(const int32_t *src, int ss, int32_t *dll, int ds, int32_t *C, const LevelGeom &g, int idx, int jy,
                                                int ovf)
{
    const int x = 2 * idx, y = 2 * jy;
    const bool hasx = (x + 1) < g.sw, hasy = (y + 1) < g.sh;
    const int32_t *r0 = src + (size_t) y * ss + x;
    const int x0 = r0[0], x1 = hasx ? r0[1] : 0, x2 = hasy ? r0[ss] : 0, x3 = (hasx && hasy) ? r0[ss + 1] : 0;
    const int dv = ovf ? 2 : 1;
    const size_t oLL = (size_t) jy * g.w + idx, oHL = (size_t) (g.hh + jy) * g.w + idx;
    int32_t *d = dll + (size_t) jy * ds + idx;
    if (hasx && hasy) {
        *d = (x0 + x1 + x2 + x3) / dv;
        C[oLL + g.hw] = x0 - x1 + x2 - x3;
        C[oHL] = x0 + x1 - x2 - x3;
        C[oHL + g.hw] = x0 - x1 - x2 + x3;
    } else if (hasy) {
        *d = 2 * (x0 + x2) / dv;
        C[oHL] = 2 * (x0 - x2);
    } else if (hasx) {
        *d = 2 * (x0 + x1) / dv;
        C[oLL + g.hw] = 2 * (x0 - x1);
    } else {
        *d = (x0 * 4) / dv;
    }
}

__global__ __launch_bounds__(256) void k_fwd_haar_tail(const PlaneJob *__restrict__ tab, int cw, int ch, int l0, int lvls, int lossless,
                                                       int cap_a)
{
    DSV2_KERNEL_PRIO();
    extern __shared__ int32_t tail_lds[];
    const PlaneJob &J = tab[blockIdx.z];
    int32_t *C = J.coefs;
    const int32_t *src = img(J, l0 & 1); // written by level l0 - 1
    int ss = cw;
    for (int l = l0; l <= lvls; l++) {
        const LevelGeom g = tail_geom(cw, ch, l);
        const int ovf = (l >= 6 && l >= (lvls - 3) && !lossless); // sbt.c:29
        int32_t *dll = l == lvls ? C : (((l - l0) & 1) ? tail_lds + cap_a : tail_lds);
        const int ds = l == lvls ? cw : g.hw;
        const int nq = g.hw * g.hh;
        for (int t = threadIdx.x; t < nq; t += 256) {
            const int jy = t / g.hw, idx = t - jy * g.hw;
            fwd_haar_quad_p(src, ss, dll, ds, C, g, idx, jy, ovf);
        }
        __syncthreads();
        src = dll;
        ss = ds;
    }
}

// one inverse quad: LL image (LLp, ls), detail bands from C, output image (out, os)
__device__ __forceinline__ void inv_haar_quad_p(const int32_t *LLp, int ls, const int32_t *C, int32_t *out, int os, const LevelGeom &g, int idx,
                                                int jy, int ovf, int filtered, int hqp)
{
    const int x = 2 * idx, y = 2 * jy;
    const bool hasx = (x + 1) < g.sw, hasy = (y + 1) < g.sh;
    const size_t oC = (size_t) jy * g.w + idx, oHL = (size_t) (g.hh + jy) * g.w + idx;
    const int32_t *lp0 = LLp + (size_t) jy * ls + idx;
    const int sc = 1 << ovf;
    const int LL = lp0[0] * sc;
    int v00, v01 = 0, v10 = 0, v11 = 0;
    if (hasx && hasy) {
        int LH = C[oC + g.hw], HL = C[oHL], HH = C[oHL + g.hw];
        if (filtered) {
            if (idx > 0) { // (one past the LL row is the row's first LH coefficient: sbt.c:715,725)
                const int lp = lp0[-1] * sc, ln = ((idx + 1 < g.hw) ? lp0[1] : C[oC + 1]) * sc;
                LH = nudge(LL, lp, ln, LH, hqp);
            }
            if (jy > 0) {
                const int lp = lp0[-ls] * sc, ln = ((jy + 1 < g.hh) ? lp0[ls] : C[oC + g.w]) * sc;
                HL = nudge(LL, lp, ln, HL, hqp);
            }
        }
        v00 = (LL + LH + HL + HH) / 4;
        v01 = (LL - LH + HL - HH) / 4;
        v10 = (LL + LH - HL - HH) / 4;
        v11 = (LL - LH - HL + HH) / 4;
    } else if (hasy) {
        const int HL = C[oHL];
        v00 = (LL + HL) / 4;
        v10 = (LL - HL) / 4;
    } else if (hasx) {
        const int LH = C[oC + g.hw];
        v00 = (LL + LH) / 4;
        v01 = (LL - LH) / 4;
    } else {
        v00 = LL / 4;
    }
    int32_t *r0 = out + (size_t) y * os + x;
    r0[0] = v00;
    if (hasx) {
        r0[1] = v01;
    }
    if (hasy) {
        r0[os] = v10;
        if (hasx) {
            r0[os + 1] = v11;
        }
    }
}

__global__ __launch_bounds__(256) void k_inv_haar_tail(const PlaneJob *__restrict__ tab, int cw, int ch, int l0, int lvls, int lossless,
                                                       int plane_idx, int isP, int cap_a)
{
    DSV2_KERNEL_PRIO();
    extern __shared__ int32_t tail_lds[];
    const PlaneJob &J = tab[blockIdx.z];
    const int32_t *C = J.coefs;
    const int32_t *LLp = C;
    int ls = cw;
    const int filtered = !lossless && (plane_idx == 0 || !isP); // sbt.c:925
    for (int l = lvls; l >= l0; l--) {
        const LevelGeom g = tail_geom(cw, ch, l);
        const int ovf = (l >= 6 && l >= (lvls - 3) && !lossless);
        const int hdiv = (plane_idx == 0) ? (isP ? 14 : (l > 4 ? 2 : 8)) : 2; // sbt.c:903
        const int hqp = J.q / hdiv;
        // level l0's output is the picture the next (per-level) launch reads: scratch image (lvls - l0) & 1, as the level loop
        // would have left it; the others alternate between the LDS buffers, the larger one holding level l0 + 1's
        int32_t *out = l == l0 ? J.t[(lvls - l0) & 1] : (((l - l0) & 1) ? tail_lds : tail_lds + cap_a);
        const int os = l == l0 ? cw : g.sw;
        const int nq = g.hw * g.hh;
        for (int t = threadIdx.x; t < nq; t += 256) {
            const int jy = t / g.hw, idx = t - jy * g.hw;
            inv_haar_quad_p(LLp, ls, C, out, os, g, idx, jy, ovf, filtered, hqp);
        }
        __syncthreads();
        LLp = out;
        ls = os;
    }
}

// columns first (sbt.c:467-469): packed column i of the Mallat image -> full column in scratch image 2
template <int F>
__global__ __launch_bounds__(256) void k_inv_cols(const PlaneJob *__restrict__ tab, LevelGeom g, int ll_sel)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    int i = blockIdx.x * 64 + threadIdx.x;
    int k = blockIdx.y * 4 + threadIdx.y;
    if (i >= g.sw || k >= g.hh) {
        return;
    }
    const int32_t *LLp = img(J, ll_sel), *C = J.coefs;
    int32_t *R = J.t[2];
    Ring r{g.use_bd ? J.bd + ((i * g.dbx) >> kBlockP) : nullptr, 2 * g.dby, g.nbh};
    Syn v{(i < g.hw) ? LLp + i : C + i, C + (size_t) g.hh * g.w + i, g.w, g.sh, C + g.w + i};
    int xe, xo;
    synthesis_pair<F>(v, r, k, xe, xo);
    R[(size_t) (2 * k) * g.w + i] = xe;
    if (2 * k + 1 < g.sh) {
        R[(size_t) (2 * k + 1) * g.w + i] = xo;
    }
}

template <int F, bool OUT_U8>
__global__ __launch_bounds__(256) void k_inv_rows(const PlaneJob *__restrict__ tab, LevelGeom g, int d_sel)
{
    DSV2_KERNEL_PRIO();
    const PlaneJob &J = tab[blockIdx.z];
    int k = blockIdx.x * 64 + threadIdx.x;
    int j = blockIdx.y * 4 + threadIdx.y;
    if (k >= g.hw || j >= g.sh) {
        return;
    }
    const int32_t *R = J.t[2];
    Ring r{g.use_bd ? J.bd + ((j * g.dby) >> kBlockP) * g.nbh : nullptr, 2 * g.dbx, 1};
    Syn v{R + (size_t) j * g.w, R + (size_t) j * g.w + g.hw, 1, g.sw, J.coefs + (size_t) j * g.w + 1};
    int xe, xo;
    synthesis_pair<F>(v, r, k, xe, xo);
    if (OUT_U8) {
        int pw = J.pic.w;
        if (j < J.pic.h) {
            uint8_t *o = J.pic.data + (size_t) j * J.pic.stride + 2 * k;
            if (2 * k < pw) {
                o[0] = to_px(xe);
            }
            if (2 * k + 1 < g.sw && 2 * k + 1 < pw) {
                o[1] = to_px(xo);
            }
        }
    } else {
        int32_t *o = J.t[d_sel] + (size_t) j * g.w + 2 * k;
        o[0] = xe;
        if (2 * k + 1 < g.sw) {
            o[1] = xo;
        }
    }
}

// ---- host drivers -------------------------------------------------------------------
struct Batch { // what a launch iterates over: a device table of n jobs
    const PlaneJob *tab;
    int n;
};
static dim3 grid3(int nx, int ny, const Batch &b) { return dim3((nx + 63) / 64, (ny + 3) / 4, b.n); }
static const dim3 kBlk(64, 4);

template <int F> static void launch_fwd_sep(hipStream_t s, const Batch &b, bool u8, const LevelGeom &g, int s_sel, int d_sel)
{
    if (u8) {
        DSV2_LAUNCH((k_fwd_rows<F, true>), grid3(g.hw, g.sh, b), kBlk, 0, s, b.tab, g, s_sel);
    } else {
        DSV2_LAUNCH((k_fwd_rows<F, false>), grid3(g.hw, g.sh, b), kBlk, 0, s, b.tab, g, s_sel);
    }
    DSV2_LAUNCH((k_fwd_cols<F>), grid3(g.sw, g.hh, b), kBlk, 0, s, b.tab, g, d_sel);
}

template <int F> static void launch_inv_sep(hipStream_t s, const Batch &b, bool u8, const LevelGeom &g, int ll_sel, int d_sel)
{
    DSV2_LAUNCH((k_inv_cols<F>), grid3(g.sw, g.hh, b), kBlk, 0, s, b.tab, g, ll_sel);
    if (u8) {
        DSV2_LAUNCH((k_inv_rows<F, true>), grid3(g.hw, g.sh, b), kBlk, 0, s, b.tab, g, d_sel);
    } else {
        DSV2_LAUNCH((k_inv_rows<F, false>), grid3(g.hw, g.sh, b), kBlk, 0, s, b.tab, g, d_sel);
    }
}

static LevelGeom level_geom(int cw, int ch, int l, int filter, int nbh, int nbv, bool have_bd, bool forward)
{
    LevelGeom g;
    g.w = cw;
    g.sw = rshift_up(cw, l - 1);
    g.sh = rshift_up(ch, l - 1);
    g.hw = (g.sw + 1) / 2;
    g.hh = (g.sh + 1) / 2;
    g.use_bd = 0;
    g.nbh = nbh;
    g.dbx = g.dby = 0;
    if (filter == F_L2A || (filter == F_L1 && forward)) {
        if (!have_bd) {
            fatal("adaptive subband filter needs blockdata", __FILE__, __LINE__);
        }
        g.use_bd = 1;
        g.dbx = (nbh << kBlockP) / g.sw;
        g.dby = (nbv << kBlockP) / g.sh;
    }
    return g;
}

// first level of the fused Haar tail (lvls + 1: none): every level from it up is Haar, its LL output and the next one fit in
// 48 KB of LDS, and at least two levels are fused.
constexpr int kTailLdsInts = 12 * 1024;
static int tail_first_level(int cw, int ch, int plane_idx, int isP, int lossless, int lvls, int *cap_a)
{
    int l0 = lvls + 1;
    *cap_a = 0;
    for (int l = lvls; l >= 2; l--) { // (level 1 reads / writes the 8-bit picture: never part of the tail)
        int hw = (rshift_up(cw, l - 1) + 1) / 2, hh = (rshift_up(ch, l - 1) + 1) / 2;
        int hw2 = (hw + 1) / 2, hh2 = (hh + 1) / 2;
        if (pick_filter(plane_idx, isP, lossless, l, lvls) != F_HAAR || hw * hh + hw2 * hh2 > kTailLdsInts) {
            break;
        }
        l0 = l;
        *cap_a = hw * hh;
    }
    return l0 < lvls ? l0 : lvls + 1;
}

static void fwd_levels(hipStream_t s, const Batch &b, int cw, int ch, int plane_idx, int isP, int lossless, int nbh, int nbv,
                       bool have_bd)
{
    int lvls = host_lb2((unsigned) (cw > ch ? cw : ch));
    int cap_a = 0;
    const int tail0 = tail_first_level(cw, ch, plane_idx, isP, lossless, lvls, &cap_a);
    for (int l = 1; l <= lvls; l++) {
        if (l == tail0) {
            DSV2_LAUNCH(k_fwd_haar_tail, dim3(1, 1, b.n), dim3(256), (size_t) kTailLdsInts * sizeof(int32_t), s, b.tab, cw, ch, tail0,
                        lvls, lossless, cap_a);
            break;
        }
        // level l reads the LL image written by level l-1 and writes its own LL to the other scratch
        int s_sel = l & 1;
        int d_sel = (l == lvls) ? IMG_COEFS : ((l - 1) & 1);
        int filter = pick_filter(plane_idx, isP, lossless, l, lvls);
        LevelGeom g = level_geom(cw, ch, l, filter, nbh, nbv, have_bd, true);
        int ovf = (l >= 6 && l >= (lvls - 3) && !lossless); // sbt.c:29
        bool u8 = (l == 1);
        switch (filter) {
            case F_HAAR:
                if (u8 && (g.hw & 3) == 0 && (g.w & 3) == 0) {
                    DSV2_LAUNCH(k_fwd_haar_u8x4, grid3(g.hw / 4, (g.hh + kHaarRows - 1) / kHaarRows, b), kBlk, 0, s, b.tab, g, d_sel, ovf);
                } else if (u8) {
                    DSV2_LAUNCH((k_fwd_haar<true>), grid3(g.hw, g.hh, b), kBlk, 0, s, b.tab, g, s_sel, d_sel, ovf);
                } else if ((g.hw & 3) == 0 && (g.w & 3) == 0) {
                    DSV2_LAUNCH(k_fwd_haar_i32x4, grid3(g.hw / 4, (g.hh + kHaarRowsI - 1) / kHaarRowsI, b), kBlk, 0, s, b.tab, g, s_sel, d_sel, ovf);
                } else {
                    DSV2_LAUNCH((k_fwd_haar<false>), grid3(g.hw, g.hh, b), kBlk, 0, s, b.tab, g, s_sel, d_sel, ovf);
                }
                break;
            case F_LLI: launch_fwd_sep<F_LLI>(s, b, u8, g, s_sel, d_sel); break;
            case F_LLP: launch_fwd_sep<F_LLP>(s, b, u8, g, s_sel, d_sel); break;
            case F_CC: launch_fwd_sep<F_CC>(s, b, u8, g, s_sel, d_sel); break;
            case F_L2A: launch_fwd_sep<F_L2A>(s, b, u8, g, s_sel, d_sel); break;
            case F_L1: launch_fwd_sep<F_L1>(s, b, u8, g, s_sel, d_sel); break;
            default: launch_fwd_sep<F_LOSSLESS>(s, b, u8, g, s_sel, d_sel); break;
        }
    }
    HIPCHK(hipGetLastError());
}

static void inv_levels(hipStream_t s, const Batch &b, int cw, int ch, int plane_idx, int isP, int lossless, int nbh, int nbv,
                       bool have_bd)
{
    int lvls = host_lb2((unsigned) (cw > ch ? cw : ch));
    int ll_sel = IMG_COEFS, d_sel = 0;
    int cap_a = 0, top = lvls;
    const int tail0 = tail_first_level(cw, ch, plane_idx, isP, lossless, lvls, &cap_a);
    if (tail0 <= lvls) {
        DSV2_LAUNCH(k_inv_haar_tail, dim3(1, 1, b.n), dim3(256), (size_t) kTailLdsInts * sizeof(int32_t), s, b.tab, cw, ch, tail0, lvls,
                    lossless, plane_idx, isP, cap_a);
        ll_sel = (lvls - tail0) & 1; // where the level loop would have left level tail0's picture
        d_sel = ll_sel ^ 1;
        top = tail0 - 1;
    }
    for (int l = top; l > 0; l--) {
        int filter = pick_filter(plane_idx, isP, lossless, l, lvls);
        LevelGeom g = level_geom(cw, ch, l, filter, nbh, nbv, have_bd, false);
        int ovf = (l >= 6 && l >= (lvls - 3) && !lossless);
        bool u8 = (l == 1);
        switch (filter) {
            case F_HAAR: {
                int hdiv = (plane_idx == 0) ? (isP ? 14 : (l > 4 ? 2 : 8)) : 2;   // sbt.c:903
                int filtered = !lossless && (plane_idx == 0 || !isP);               // sbt.c:925
                if (u8 && (g.hw & 3) == 0 && (g.w & 3) == 0) {
                    DSV2_LAUNCH(k_inv_haar_u8x4, grid3(g.hw / 4, g.hh, b), kBlk, 0, s, b.tab, g, ll_sel, ovf, filtered, hdiv);
                } else if (u8) {
                    DSV2_LAUNCH((k_inv_haar<true>), grid3(g.hw, g.hh, b), kBlk, 0, s, b.tab, g, ll_sel, d_sel, ovf,
                                       filtered, hdiv);
                } else if ((g.hw & 3) == 0 && (g.w & 3) == 0) {
                    DSV2_LAUNCH(k_inv_haar_i32x4, grid3(g.hw / 4, g.hh, b), kBlk, 0, s, b.tab, g, ll_sel, d_sel, ovf, filtered, hdiv);
                } else {
                    DSV2_LAUNCH((k_inv_haar<false>), grid3(g.hw, g.hh, b), kBlk, 0, s, b.tab, g, ll_sel, d_sel, ovf,
                                       filtered, hdiv);
                }
                break;
            }
            case F_LLI: launch_inv_sep<F_LLI>(s, b, u8, g, ll_sel, d_sel); break;
            case F_LLP: launch_inv_sep<F_LLP>(s, b, u8, g, ll_sel, d_sel); break;
            case F_CC: launch_inv_sep<F_CC>(s, b, u8, g, ll_sel, d_sel); break;
            case F_L2A: launch_inv_sep<F_L2A>(s, b, u8, g, ll_sel, d_sel); break;
            case F_L1: launch_inv_sep<F_L1>(s, b, u8, g, ll_sel, d_sel); break;
            default: launch_inv_sep<F_LOSSLESS>(s, b, u8, g, ll_sel, d_sel); break;
        }
        ll_sel = d_sel;
        d_sel ^= 1;
    }
    HIPCHK(hipGetLastError());
}

void sbt_forward_jobs(hipStream_t s, const PlaneJob *d_jobs, int n, int cw, int ch, int plane_idx, int isP, int lossless, int nbh,
                      int nbv, bool have_bd)
{
    if (n > 0) {
        fwd_levels(s, Batch{d_jobs, n}, cw, ch, plane_idx, isP, lossless, nbh, nbv, have_bd);
    }
}

void sbt_inverse_jobs(hipStream_t s, const PlaneJob *d_jobs, int n, int cw, int ch, int plane_idx, int isP, int lossless, int nbh,
                      int nbv, bool have_bd)
{
    if (n > 0) {
        inv_levels(s, Batch{d_jobs, n}, cw, ch, plane_idx, isP, lossless, nbh, nbv, have_bd);
    }
}

} // namespace dsv2
