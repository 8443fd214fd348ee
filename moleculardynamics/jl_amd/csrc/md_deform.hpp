// md_deform.hpp -- gfx950 device code of md_deform_cell: the whole frame of a live handle is mapped by a deformation
// gradient F about the origin of its own unwrapped frame, x -> F x, v -> G v, together with the reference positions x0 (list
// build) and x1 (last prune) of the Verlet rows -- so that the rows stay the rows of the mapped frame and only the
// displacement budget changes.  md_baro.hpp's k_scale_cell is the special case F = mu 1.
//
// New relative to the reference, which fixes its cell at initialisation (src/initialization.jl:7-18).  The arithmetic is
// that of k_set_cell's general branch (md_cell.hpp cell_cart): row times vector, left to right, every product and every sum
// rounded on its own, no fma -- numpy reproduces positions, x0, x1 and velocities bit for bit.  Nothing is wrapped (the wrap
// is lazy; a wrap here would invalidate the shift codes of the rows) and image counts are not touched: every lattice vector
// is mapped with the frame, so frac + img is kept up to the rounding of the products.
//
// One streaming pass in slot order, one thread per record, as k_scale_cell, and the same verdict in the same pass: the
// squared displacement from the mapped x0 and x1 (the fma chain of k_kickdrift) against the limits the step loop will use, a
// wave maximum, and -- only from a wave that holds a particle beyond a limit -- one integer atomicMax on the double's bits.
// No floating-point atomics, no LDS.  F and G are kernel arguments: they live in scalar registers.
#pragma once
#include "md_baro.hpp"

struct DeformMap {
    double F[9], G[9]; // row-major 3 x 3 (a 2-D map uses the upper left 2 x 2)
};

// o = M x in cell_cart's arithmetic
template <int D>
__device__ __forceinline__ void deform_apply(const double *m, double x, double y, double z, double *o)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double t = m[r * 3 + 0] * x + m[r * 3 + 1] * y;
        if constexpr (D == 3) t = t + m[r * 3 + 2] * z;
        o[r] = t;
    }
}

// npos >= n records of s.pos are mapped (the owned particles and, behind them, the real ghost records of the list); x0 of
// the n owned ones; x1 only when the inner rows are valid (has_x1: s.x1 aliases x0 otherwise); v only with has_g.
// half_skin, half_inner: the displacement limits after the map, as in k_scale_cell; smax >= sigma_max(F) scales d1 (rounded
// up, scaled_d1sq).  sc is only read: the new d1^2 goes to dmax[2] (k_scale_commit stores it).
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_deform_cell(int n, int npos, DevState s, DeformMap m, int has_g, int has_x1, double half_skin, double half_inner,
                  double smax, const Scalars *__restrict__ sc, unsigned long long *__restrict__ dmax)
{
#pragma clang fp contract(off)
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    double d0 = 0.0, d1 = 0.0;
    if (k < npos) {
        double4 p = s.pos[k];
        double x[3] = {0.0, 0.0, 0.0};
        deform_apply<D>(m.F, p.x, p.y, p.z, x);
        p.x = x[0];
        p.y = x[1];
        if constexpr (D == 3) p.z = x[2];
        s.pos[k] = p;
        if (k < n) {
            double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
            deform_apply<D>(m.F, s.x0[0][k], s.x0[1][k], D == 3 ? s.x0[2][k] : 0.0, a);
#pragma unroll
            for (int c = 0; c < D; ++c) {
                s.x0[c][k] = a[c];
                double d = x[c] - a[c];
                d0 = __builtin_fma(d, d, d0);
            }
            if (has_x1) {
                deform_apply<D>(m.F, s.x1[0][k], s.x1[1][k], D == 3 ? s.x1[2][k] : 0.0, b);
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    s.x1[c][k] = b[c];
                    double e = x[c] - b[c];
                    d1 = __builtin_fma(e, e, d1);
                }
            }
            if (has_g) {
                double w[3] = {0.0, 0.0, 0.0};
                deform_apply<D>(m.G, s.v[0][k], s.v[1][k], D == 3 ? s.v[2][k] : 0.0, w);
#pragma unroll
                for (int c = 0; c < D; ++c) s.v[c][k] = w[c];
            }
        }
    }
    if (blockIdx.x * blockDim.x >= n) return; // (a block of ghost records only: uniform per block)
    double lim0 = half_skin * half_skin, lim1 = INFINITY;
    if (has_x1) {
        double d1sq = scaled_d1sq(__longlong_as_double((long long)sc->d1max2_bits), smax);
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
