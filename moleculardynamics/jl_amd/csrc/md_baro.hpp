// md_baro.hpp -- gfx950 device code of md_scale_cell: the whole frame of a live handle is scaled isotropically about the
// origin of its own unwrapped frame, x -> mu x, v -> vscale v, together with the reference positions x0 (list build) and
// x1 (last prune) of the Verlet rows -- so that the rows stay the rows of the scaled frame and only the displacement
// budget changes.
//
// New relative to the reference, which has no barostat.  The arithmetic is one product per component, rounded once, no
// fma: numpy's mu * x reproduces positions and velocities bit for bit.  Nothing is wrapped (the wrap is lazy, md_kernels.hpp
// k_export; a wrap here would invalidate the shift codes of the rows) and image counts are not touched, so frac + img is
// kept up to the rounding of the products.
//
// One streaming pass in slot order, one thread per record, as k_set_cell: 32-byte position records, the planes of x0, x1
// and v coalesced.  The pass also decides, on the values it has in registers, whether the kept rows still cover the frame:
// the squared displacement from the scaled x0 and from the scaled x1 (the fma chain of k_max_disp0 / k_kickdrift) against
// the limits the step loop will use, a wave maximum, and -- only from a wave that holds a particle beyond a limit -- one
// integer atomicMax on the double's bits (non-negative doubles order as their bits, as Scalars::max_disp2_bits).  A frame
// inside its limits, the usual case, issues no atomic at all (an unconditional maximum would queue one atomic per wave,
// 16 k of them at N = 2^20, on one address).  No floating-point atomics.
#pragma once
#include "md_kernels.hpp"

#define MD_SCALE_NOUT 3 // dmax: bits of max |x - x0|^2 and max |x - x1|^2 beyond their limits (0: none), bits of the new d1^2

// d1 = max |x1 - x0| (Scalars::d1max2_bits holds its square) after a scale by mu, rounded up: sqrt, product and square
// each err by at most half an ulp, a factor (1 + 2^-50) covers them.  The host forms the limits from the same value.
__device__ __forceinline__ double scaled_d1sq(double d1sq, double mu)
{
#pragma clang fp contract(off)
    double r = mu * sqrt(d1sq);
    return (r * r) * (1.0 + 0x1p-50);
}

// npos >= n records of s.pos are scaled (the owned particles and, behind them, the real ghost records of the list);
// x0, v of the n owned ones; x1 only when the inner rows are valid (has_x1: s.x1 aliases x0 otherwise).
// half_skin, half_inner: the displacement limits after the scale (k_kickdrift's rule: within half_skin of x0, and with
// inner rows within min(half_inner, half_skin - d1) of x1); INFINITY when no rows are kept.  sc is only read: the new
// d1^2 goes to dmax[2] (k_scale_commit stores it), so that every block sees the old one whenever it runs.
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_scale_cell(int n, int npos, DevState s, double mu, double vscale, int has_x1, double half_skin, double half_inner,
                 const Scalars *__restrict__ sc, unsigned long long *__restrict__ dmax)
{
#pragma clang fp contract(off)
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    double d0 = 0.0, d1 = 0.0;
    if (k < npos) {
        double4 p = s.pos[k];
        p.x = mu * p.x;
        p.y = mu * p.y;
        if constexpr (D == 3) p.z = mu * p.z;
        s.pos[k] = p;
        if (k < n) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                double xc = pos_get(p, c);
                double a = mu * s.x0[c][k];
                s.x0[c][k] = a;
                double d = xc - a;
                d0 = __builtin_fma(d, d, d0);
                if (has_x1) {
                    double b = mu * s.x1[c][k];
                    s.x1[c][k] = b;
                    double e = xc - b;
                    d1 = __builtin_fma(e, e, d1);
                }
                s.v[c][k] = vscale * s.v[c][k];
            }
        }
    }
    if (blockIdx.x * blockDim.x >= n) return; // (a block of ghost records only: uniform per block)
    double lim0 = half_skin * half_skin, lim1 = INFINITY;
    if (has_x1) {
        double d1sq = scaled_d1sq(__longlong_as_double((long long)sc->d1max2_bits), mu);
        if (k == 0) dmax[2] = (unsigned long long)__double_as_longlong(d1sq);
        double thr = fmin(half_inner, half_skin - sqrt(d1sq));
        lim1 = thr > 0.0 ? thr * thr : -1.0;
    }
    double w0 = wave_max_d(d0), w1 = wave_max_d(d1);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long b0 = (unsigned long long)__double_as_longlong(w0);
        unsigned long long b1 = (unsigned long long)__double_as_longlong(w1);
        if (w0 > lim0 && b0 > dmax[0]) atomicMax(&dmax[0], b0);
        if (w1 > lim1 && b1 > dmax[1]) atomicMax(&dmax[1], b1);
    }
}

__global__ void k_scale_commit(Scalars *sc, const unsigned long long *__restrict__ dmax) { sc->d1max2_bits = dmax[2]; }
