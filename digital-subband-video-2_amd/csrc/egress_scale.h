// egress_scale.h -- what one thread of k_egress_scale (egress.hip) does, as a function that also compiles for the host (the pattern of
// egress_uv.h and egress_rgb.h): the kernel is this function behind blockIdx / threadIdx, and tools/egress_scale_check.cpp sweeps the
// very same code on the CPU under AddressSanitizer -- shifts, forms, widths, heights, pitches and offsets -- before it runs on a GPU.
//
// One ScaleOutJob (io_jobs.h) = one plane of a decoded picture on its way out at half, quarter or eighth size.  With s = j.shift and
// n = 1 << s, a plane of pw x ph becomes ow = ceil(pw / n) by oh = ceil(ph / n), and (include/dsv2_hip.h, the contract)
//   out(x, y) = (SUM j<n, i<n  P(min(x*n + i, pw-1), min(y*n + j, ph-1))  +  (1 << (2*s - 1))) >> (2*s)
// one rounding over the whole footprint; a footprint across the right or bottom edge repeats the edge pixel.
// A thread owns 16 source bytes -- 16 >> s consecutive output samples (8, 4, 2) -- of ONE output row: its n source rows are read as
// one aligned 16-byte vector each (the plane's origin and stride are multiples of 16; the up to 15 bytes past the row lie in the
// plane's border, or inside the stride of the decoder's staged luma), rows below ph again from the last row, every load issued
// before the first store.  Only the vector that holds the row's last byte can be partial: its bytes from pw on are replaced by byte
// pw - 1 before anything is summed, so the sums know no edge.  A horizontal sum of bytes is one v_dot4_u32_u8 of a dword against
// ones (two bytes of it at half size); the sum of a footprint is at most 64 * 255 = 16 320.
//   WIDE:    destination pointer and pitch multiples of 8 and the row writable up to a multiple of 16 >> s bytes in every job of the
//            launch (a caller's plane: ow such a multiple; the staging picture: always) -- the host picks it per round,
//            scale_job_wide: one unconditional store of 8, 4 or 2 bytes.
//   general: any ow, pitch and alignment.  A sample is stored only where x < ow: four of them as one dword where they lie whole
//            inside the row at an address that is a multiple of 4 (an eighth: the two as one 16-bit word, a multiple of 2), else byte
//            by byte -- no byte outside the oh row pieces of ow bytes is ever written.
#pragma once

#include "ingest_rgb.h" // ld_global, st_global, u32x4, lane_offset, dot4_u8

namespace dsv2 {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// A row's last vector, `valid` (1 .. 15) bytes of which lie inside the row: the others become the row's last byte.  Straight-line
// code: what depends on `valid` alone -- which bits of each dword stay, where the last byte sits -- is the same for every row of the
// footprint, and a row costs four masked ORs, a shift, a multiply and four bit-field inserts.
struct ScaleEdge {
    uint32_t keep[4]; // bits of dword k that lie inside the row
    uint32_t pick[4]; // all ones for the dword that holds the row's last byte
    int sh;           // bit position of that byte
};
__host__ __device__ __forceinline__ ScaleEdge scale_edge_of(int valid)
{
    ScaleEdge e;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int nv = valid - 4 * k; // bytes of dword k inside the row
        e.keep[k] = nv >= 4 ? 0xffffffffu : nv <= 0 ? 0u : (1u << (8 * (nv & 3))) - 1u;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        e.pick[k] = ((valid - 1) >> 2) == k ? 0xffffffffu : 0u;
    }
    e.sh = 8 * ((valid - 1) & 3);
    return e;
}
__host__ __device__ __forceinline__ void scale_edge(u32x4 &q, const ScaleEdge &e)
{
    const uint32_t d = (q[0] & e.pick[0]) | (q[1] & e.pick[1]) | (q[2] & e.pick[2]) | (q[3] & e.pick[3]);
    const uint32_t edge = ((d >> e.sh) & 0xffu) * 0x01010101u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        q[k] = (q[k] & e.keep[k]) | (edge & ~e.keep[k]);
    }
}

// output row oy0 + ry (below oh) of job j at shift S: source vectors t_first, t_first + t_step ... of its rows.  oy0 is the first row
// of the workgroup, the same in every lane: a source address is then a base all lanes share plus a 32-bit lane offset of at most
// 32 * 8 rows (a destination row keeps its 64-bit address: its pitch may be anything up to INT_MAX)
template <bool WIDE, int S> __host__ __device__ __forceinline__ void egress_scale_row_s(const ScaleOutJob &j, int oy0, int ry, int t_first, int t_step)
{
    constexpr int N = 1 << S, NOUT = 16 >> S; // source rows and columns of a footprint; output samples of a thread
    constexpr uint32_t kRound = 1u << (2 * S - 1);
    const int pw = j.pw, ph = j.ph, ow = (pw + N - 1) >> S;
    const int oy = oy0 + ry, below = ph - 1 - oy * N; // rows of the footprint below its first one that lie inside the plane (or more)
    const uint8_t *sbase = j.src + (size_t) (oy0 * N) * (size_t) j.sstride;
    uint8_t *drow = j.dst + (size_t) oy * (size_t) j.dpitch;
    for (int ti = t_first; 16 * ti < pw; ti += t_step) {
        const int t = lane_offset(ti);
        u32x4 v[N];
#pragma unroll
        for (int r = 0; r < N; r++) {
            const int rr = r < below ? r : below; // (rows below the plane: its last row again)
            v[r] = ld_global<u32x4>(sbase, (uint32_t) (ry * N + rr) * (uint32_t) j.sstride + 16 * (uint32_t) t);
        }
        const int valid = pw - 16 * t;
        if (valid < 16) {
            const ScaleEdge e = scale_edge_of(valid);
#pragma unroll
            for (int r = 0; r < N; r++) {
                scale_edge(v[r], e);
            }
        }
        uint32_t o[NOUT]; // the samples, a byte each
#pragma unroll
        for (int i = 0; i < NOUT; i++) {
            uint32_t sum = kRound;
#pragma unroll
            for (int r = 0; r < N; r++) {
                if constexpr (S == 1) {
                    sum = dot4_u8(v[r][i >> 1], (i & 1) ? 0x01010000u : 0x00000101u, sum);
                } else if constexpr (S == 2) {
                    sum = dot4_u8(v[r][i], 0x01010101u, sum);
                } else {
                    sum = dot4_u8(v[r][2 * i + 1], 0x01010101u, dot4_u8(v[r][2 * i], 0x01010101u, sum));
                }
            }
            o[i] = sum >> (2 * S);
        }
        const int x = t * NOUT;
        if constexpr (S == 3) {
            const uint32_t pair = o[0] | (o[1] << 8);
            if (WIDE || (x + 2 <= ow && (((uintptr_t) (drow + x)) & 1) == 0)) {
                st_global<uint16_t>(drow, (uint32_t) x, (uint16_t) pair);
            } else {
                for (int i = 0; i < 2 && x + i < ow; i++) {
                    st_global<uint8_t>(drow, (uint32_t) (x + i), (uint8_t) o[i]);
                }
            }
        } else {
            uint32_t w[NOUT / 4];
#pragma unroll
            for (int k = 0; k < NOUT / 4; k++) {
                w[k] = o[4 * k] | (o[4 * k + 1] << 8) | (o[4 * k + 2] << 16) | (o[4 * k + 3] << 24);
            }
            if constexpr (WIDE) {
                if constexpr (S == 1) {
                    st_global<u32x2>(drow, (uint32_t) x, u32x2{w[0], w[1]});
                } else {
                    st_global<uint32_t>(drow, (uint32_t) x, w[0]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < NOUT / 4; k++) {
                    const int xk = x + 4 * k;
                    if (xk + 4 <= ow && (((uintptr_t) (drow + xk)) & 3) == 0) {
                        st_global<uint32_t>(drow, (uint32_t) xk, w[k]);
                    } else {
                        for (int i = 0; i < 4 && xk + i < ow; i++) {
                            st_global<uint8_t>(drow, (uint32_t) (xk + i), (uint8_t) (w[k] >> (8 * i)));
                        }
                    }
                }
            }
        }
    }
}

// The shift is one value for the whole job, so the switch stands outside the row loop (egress_rgb.h).
template <bool WIDE> __host__ __device__ __forceinline__ void egress_scale_row(const ScaleOutJob &j, int oy0, int ry, int t_first, int t_step)
{
    switch (j.shift) {
    case 1:
        egress_scale_row_s<WIDE, 1>(j, oy0, ry, t_first, t_step);
        break;
    case 2:
        egress_scale_row_s<WIDE, 2>(j, oy0, ry, t_first, t_step);
        break;
    default: // 3 (the host lets no other shift through)
        egress_scale_row_s<WIDE, 3>(j, oy0, ry, t_first, t_step);
        break;
    }
}

} // namespace dsv2
