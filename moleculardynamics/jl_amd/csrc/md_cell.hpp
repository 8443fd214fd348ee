// md_cell.hpp -- gfx950 device code of md_set_cell and md_nonaffine_*: the cell of a live handle changes and the
// particles go along, either at fixed fractional coordinates (MD_CELL_AFFINE) or at fixed Cartesian positions in a cell
// that generates the same lattice (MD_CELL_LATTICE); and the displacement since a mark, in the current cell, with the
// affine part taken out.
//
// Reference behaviour restated here: wrap_to_box, src/boundary.jl:7-17 (x -> U (U^-1 x - floor.(U^-1 x))), in the
// operation order of oracle/md_oracle.c wrap1 / wrap_tric: every product and every sum rounded on its own, left to right,
// no fma.  The reference has no cell change of its own; an affine one is that wrap with the OLD inverse and the NEW matrix.
//
// Every kernel is one streaming pass over the state records in slot order (slot k holds particle id[k], as k_import /
// k_export read them); what is kept by particle id (the mark) is reached through id[k], one thread per particle, so no two
// threads share a word.  No floating-point atomics: sums are fixed-order block partials finished by k_naff_finish.
#pragma once
#include "md_kernels.hpp"

#define MD_CELL_AFFINE_MODE 0
#define MD_CELL_LATTICE_MODE 1
#define MD_NAFF_NSUM 5 // block partials of md_nonaffine: sum u_x, u_y, u_z, |u|^2, |u|^4

// What k_set_cell needs of the two cells.  Matrices are row-major 3 x 3 with the lattice vectors in the columns, as
// DevState::cellA; a diagonal cell (tric == 0) uses only the diagonal, inv[c * 3 + c] = 1 / L_c being BoxGrid::invL.
struct CellMap {
    int tric_old, tric_new;
    double inv_old[9];         // U_old^-1 (MD_CELL_AFFINE)
    double a_new[9], inv_new[9];
    long long minv[9];         // M^-1, M = U_old^-1 U_new, integer and unimodular (MD_CELL_LATTICE)
};

// frac = U^-1 x in the wrap's arithmetic: invL * x per component, or row times vector
template <int D>
__device__ __forceinline__ void cell_frac(const double4 &p, int tric, const double *inv, double *fr)
{
#pragma clang fp contract(off)
    if (tric) {
        frac_of<D>(p.x, p.y, p.z, inv, fr);
    } else {
        fr[0] = inv[0] * p.x;
        fr[1] = inv[4] * p.y;
        fr[2] = D == 3 ? inv[8] * p.z : 0.0;
    }
}

// x = U d in the wrap's arithmetic: L * d per component, or row times vector
template <int D>
__device__ __forceinline__ void cell_cart(const double *d, int tric, const double *a, double *o)
{
#pragma clang fp contract(off)
    o[2] = 0.0;
    if (tric) {
#pragma unroll
        for (int r = 0; r < D; ++r) {
            double t = a[r * 3 + 0] * d[0] + a[r * 3 + 1] * d[1];
            if constexpr (D == 3) t = t + a[r * 3 + 2] * d[2];
            o[r] = t;
        }
    } else {
#pragma unroll
        for (int r = 0; r < D; ++r) o[r] = a[r * 3 + r] * d[r];
    }
}

// One pass over the n state records.  commit == 0 (MD_CELL_LATTICE only): nothing is written but *range_error, set when an
// image count of the state or of the mark would leave int32 -- the host refuses then, with the handle untouched.
//
// MD_CELL_AFFINE: frac = U_old^-1 x, n = floor(frac), img += n, x = U_new (frac - n).  v and f are not touched (the forces
// are those of the old cell until the next evaluation).  frac + img is kept exactly, so a mark needs no change.
// MD_CELL_LATTICE: img' = M^-1 img in integers; x is wrapped into the new cell as k_export wraps (only a coordinate outside
// [0, 1) moves) and the wrap's shift goes to img'.  The mark of particle id[k] (mfrac, mimg: n x D by id, or null) becomes
// M^-1 frac0, M^-1 img0: frac0 + img0 is the same lattice-frame vector in the new basis.
template <int D, int MODE>
__global__ void __launch_bounds__(MD_BLOCK)
    k_set_cell(int n, DevState s, CellMap m, int commit, int *__restrict__ range_error, double *__restrict__ mfrac,
               int32_t *__restrict__ mimg)
{
#pragma clang fp contract(off)
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double4 p = s.pos[k];
    if constexpr (MODE == MD_CELL_AFFINE_MODE) {
        double fr[3], fm[3] = {0.0, 0.0, 0.0}, o[3];
        cell_frac<D>(p, m.tric_old, m.inv_old, fr);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            double nn = floor(fr[c]);
            fm[c] = fr[c] - nn;
            s.img[c][k] += (int32_t)nn;
        }
        cell_cart<D>(fm, m.tric_new, m.a_new, o);
        p.x = o[0];
        p.y = o[1];
        if constexpr (D == 3) p.z = o[2];
        s.pos[k] = p;
    } else {
        long long im[3] = {0, 0, 0}, jm[3];
#pragma unroll
        for (int c = 0; c < D; ++c) im[c] = s.img[c][k];
#pragma unroll
        for (int r = 0; r < D; ++r) jm[r] = m.minv[r * 3 + 0] * im[0] + m.minv[r * 3 + 1] * im[1] + m.minv[r * 3 + 2] * im[2];
        int32_t dn[3] = {0, 0, 0};
        bool moved = false;
        if (m.tric_new) {
            moved = wrap_general<D>(p.x, p.y, p.z, m.a_new, m.inv_new, dn);
        } else {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                double xc = pos_get(p, c), Lc = m.a_new[c * 3 + c];
                if (xc < 0.0 || xc >= Lc) {
                    double frac = m.inv_new[c * 3 + c] * xc;
                    double nn = floor(frac);
                    dn[c] = (int32_t)nn;
                    pos_set(p, c, Lc * (frac - nn));
                    moved = true;
                }
            }
        }
        bool bad = false;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            jm[c] += dn[c];
            bad = bad || jm[c] > 2147483647ll || jm[c] < -2147483648ll;
        }
        long long i0[3] = {0, 0, 0}, j0[3] = {0, 0, 0};
        double f0[3] = {0.0, 0.0, 0.0}, g0[3] = {0.0, 0.0, 0.0};
        size_t o = 0;
        if (mfrac) {
            o = (size_t)s.id[k] * D;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                i0[c] = mimg[o + c];
                f0[c] = mfrac[o + c];
            }
#pragma unroll
            for (int r = 0; r < D; ++r) {
                j0[r] = m.minv[r * 3 + 0] * i0[0] + m.minv[r * 3 + 1] * i0[1] + m.minv[r * 3 + 2] * i0[2];
                double t = (double)m.minv[r * 3 + 0] * f0[0] + (double)m.minv[r * 3 + 1] * f0[1];
                if constexpr (D == 3) t = t + (double)m.minv[r * 3 + 2] * f0[2];
                g0[r] = t;
                bad = bad || j0[r] > 2147483647ll || j0[r] < -2147483648ll;
            }
        }
        if (bad) *range_error = 1; // (every writer stores the same value)
        if (!commit) return;
#pragma unroll
        for (int c = 0; c < D; ++c) s.img[c][k] = (int32_t)jm[c];
        if (moved) s.pos[k] = p;
        if (mfrac) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                mimg[o + c] = (int32_t)j0[c];
                mfrac[o + c] = g0[c];
            }
        }
    }
}

struct NaffCell {
    int tric;
    double a[9], inv[9];
};

// md_nonaffine_mark: fractional coordinate (as stored: not reduced to [0, 1), the wrap is lazy) and image count of every
// particle, by particle id
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_naff_mark(int n, DevState s, NaffCell cell, double *__restrict__ mfrac, int32_t *__restrict__ mimg)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double fr[3];
    cell_frac<D>(s.pos[k], cell.tric, cell.inv, fr);
    size_t o = (size_t)s.id[k] * D;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        mfrac[o + c] = fr[c];
        mimg[o + c] = s.img[c][k];
    }
}

// md_nonaffine, first pass: u = U ((frac - frac0) + (img - img0)) per particle (the image difference exact), written by
// id when uo is given; per block the sums of u, |u|^2, |u|^4 in a fixed order (xor-shuffle tree per wave, the four waves
// left to right), the block's largest |u|^2 with the lowest id attaining it, and the global maximum through an integer
// atomicMax on the double's bits (non-negative doubles order as their bits, as Scalars::max_disp2_bits).
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_naff(int n, DevState s, NaffCell cell, const double *__restrict__ mfrac, const int32_t *__restrict__ mimg,
           double *__restrict__ uo, double *__restrict__ part, unsigned long long *__restrict__ pmax,
           int32_t *__restrict__ pid, unsigned long long *__restrict__ gmax)
{
#pragma clang fp contract(off)
    __shared__ double sh[MD_NAFF_NSUM][MD_BLOCK / 64];
    __shared__ unsigned long long shb[MD_BLOCK / 64];
    __shared__ int32_t shi[MD_BLOCK / 64];
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    double u[3] = {0.0, 0.0, 0.0}, u2 = 0.0;
    int32_t id = 0x7fffffff;
    if (k < n) {
        id = s.id[k];
        size_t o = (size_t)id * D;
        double fr[3], d[3] = {0.0, 0.0, 0.0};
        cell_frac<D>(s.pos[k], cell.tric, cell.inv, fr);
#pragma unroll
        for (int c = 0; c < D; ++c) {
            // (the int32 difference in 64 bits: exact; as a double exact as well)
            long long di = (long long)s.img[c][k] - (long long)mimg[o + c];
            d[c] = (fr[c] - mfrac[o + c]) + (double)di;
        }
        cell_cart<D>(d, cell.tric, cell.a, u);
        u2 = d2_ref<D>(u[0], u[1], u[2]);
        if (uo) {
#pragma unroll
            for (int c = 0; c < D; ++c) uo[o + c] = u[c];
        }
    }
    double v[MD_NAFF_NSUM] = {u[0], u[1], u[2], u2, u2 * u2};
    unsigned long long bits = (unsigned long long)__double_as_longlong(u2);
    if (k >= n) bits = 0ull;
    unsigned long long wb = bits;
    int32_t wi = id;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long ob = __shfl_xor(wb, off);
        int32_t oi = __shfl_xor(wi, off);
        if (ob > wb || (ob == wb && oi < wi)) {
            wb = ob;
            wi = oi;
        }
    }
#pragma unroll
    for (int q = 0; q < MD_NAFF_NSUM; ++q) v[q] = wave_sum(v[q]);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < MD_NAFF_NSUM; ++q) sh[q][w] = v[q];
        shb[w] = wb;
        shi[w] = wi;
        if (wb > *gmax) atomicMax(gmax, wb);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < MD_NAFF_NSUM; ++q) {
            double a = sh[q][0];
            for (int j = 1; j < MD_BLOCK / 64; ++j) a = a + sh[q][j];
            part[(size_t)q * gridDim.x + blockIdx.x] = a;
        }
        unsigned long long b = shb[0];
        int32_t bi = shi[0];
        for (int j = 1; j < MD_BLOCK / 64; ++j)
            if (shb[j] > b || (shb[j] == b && shi[j] < bi)) {
                b = shb[j];
                bi = shi[j];
            }
        pmax[blockIdx.x] = b;
        pid[blockIdx.x] = bi;
    }
}

// md_nonaffine, second pass, MD_NAFF_NSUM + 1 blocks: block q < MD_NAFF_NSUM finishes sum q -- thread t adds the partials of
// blocks t, t + 256, ... in that order, an LDS tree adds the threads -- and the last block finds the id: the lowest one
// among the blocks that attain the global maximum.
// out: sum u_x, u_y, u_z, sum |u|^2, sum |u|^4, max |u|^2, the id attaining it, n.
__global__ void __launch_bounds__(MD_BLOCK)
    k_naff_finish(int nblk, int n, const double *__restrict__ part, const unsigned long long *__restrict__ pmax,
                  const int32_t *__restrict__ pid, const unsigned long long *__restrict__ gmax, double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double sh[MD_BLOCK];
    __shared__ int32_t si[MD_BLOCK];
    const int t = threadIdx.x, q = blockIdx.x;
    if (q < MD_NAFF_NSUM) {
        double a = 0.0;
        for (int b = t; b < nblk; b += MD_BLOCK) a = a + part[(size_t)q * nblk + b];
        sh[t] = a;
        __syncthreads();
        for (int h = MD_BLOCK / 2; h > 0; h >>= 1) {
            if (t < h) sh[t] = sh[t] + sh[t + h];
            __syncthreads();
        }
        if (t == 0) out[q] = sh[0];
        return;
    }
    const unsigned long long g = *gmax;
    int32_t best = 0x7fffffff;
    for (int b = t; b < nblk; b += MD_BLOCK)
        if (pmax[b] == g) best = min(best, pid[b]);
    si[t] = best;
    __syncthreads();
    for (int h = MD_BLOCK / 2; h > 0; h >>= 1) {
        if (t < h) si[t] = min(si[t], si[t + h]);
        __syncthreads();
    }
    if (t == 0) {
        out[5] = __longlong_as_double((long long)g);
        out[6] = (double)si[0];
        out[7] = (double)n;
    }
}
