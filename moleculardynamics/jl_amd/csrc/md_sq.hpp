// md_sq.hpp -- collective structure sampled on the device (md_sq_* in include/mdhip.h): the density modes
// rho(q) = sum_j exp(+i q.x_j) of the current frame on a set of wave vectors commensurate with the cell, the static
// accumulator sum |rho|^2 behind S(q), and the correlations Re(rho(t) rho*(t0)) against stored origins behind the coherent
// intermediate scattering function F(q, t).
//
// A wave vector is an integer tuple n, q_n = 2 pi U^-T n, so q_n.x = 2 pi n.f with f = U^-1 x: the phase needs only the
// wrapped coordinates (an image shift changes n.f by an integer).  One md_sq_sample call = one k_export of the current
// frame (what md_download returns), then
//   k_sq_frac    f of every particle, id order, one array per axis (x_c / L_c for a diagonal cell, U^-1 x otherwise)
//   k_sq_rho     grid = (blocks of MD_SQ_BLOCK * MD_SQ_PPT particle ids) x (tiles of MD_SQ_TILE wave vectors): particles
//                across lanes, the tile's vectors wave-uniform (scalar loads), 2 * MD_SQ_TILE fp64 accumulators per thread,
//                no LDS in the walk; block partials in a fixed tree, written per (vector, component, block)
//   k_sq_reduce  one wave per vector: the block partials in a fixed tree -> rho; then lane 0 adds |rho|^2 to s2, the
//                correlations of this call to their rows and stores the origin, in that order
// The particle walk and the partial tree are written once, here, for the three wave-vector samplers (md_sq, md_chi4,
// md_cur): mode_walk<D, TILE, MASKED, Term> is the body of k_sq_rho, k_chi4_modes and k_cur_modes, sq_row_sum the
// opening of k_sq_reduce, k_chi4_reduce and k_cur_reduce.
//
// Exactness contract: t = (n_0 f_0 + n_1 f_1) + n_2 f_2 with every operation rounded on its own,
// r = t - rint(t) (exact), the term is (cos 2 pi r, sin 2 pi r) from two polynomials in r^2 for sin / cos of the half angle
// pi r and the double-angle identities (a few units of 2^-53 of absolute error).  No fp32 in the phase.  The
// sum over particles is a tree fixed by N alone -- thread: MD_SQ_PPT ids in order; wave: shuffle tree; block: the four
// waves in order; k_sq_reduce: lane l sums the blocks l, l + 64, ... in order, then a shuffle tree -- with no
// floating-point atomics, so rho is a function of the frame only.  Longest chain of dependent additions:
// MD_SQ_PPT + 6 + 3 + ceil(nblk / 64) + 6 = 47 at N = 2^22.  s2 and corr are no-fma expressions of the rho values.
#pragma once
#include "md_kernels.hpp"

#define MD_SQ_BLOCK 256
#define MD_SQ_PPT 16              // particle ids per thread: one block covers MD_SQ_BLOCK * MD_SQ_PPT ids
#define MD_SQ_TILE 8              // wave vectors per block
#define MD_SQ_MAX_VEC 16384
#define MD_SQ_MAX_N 32767         // |n_c|
#define MD_SQ_MAX_SLOTS 64
#define MD_SQ_MAX_BATCH 64        // correlations per k_sq_reduce launch
#define MD_SQ_REDUCE_BLOCK 256

struct SqBatch {
    int count;
    int slot[MD_SQ_MAX_BATCH];
    int row[MD_SQ_MAX_BATCH];
};

__device__ __forceinline__ double sq_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v; // (lane 0)
}

// f = U^-1 x per particle, written one array per axis (fr[c * n + i]) so k_sq_rho reads it coalesced.
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_sq_frac(int n, BoxGrid g, const double *__restrict__ x, double *__restrict__ fr)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double p[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < D; ++c) p[c] = x[(size_t)i * D + c];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double f;
        if (g.tric) {
            f = g.Ainv[c * 3 + 0] * p[0] + g.Ainv[c * 3 + 1] * p[1];
            if constexpr (D == 3) f = f + g.Ainv[c * 3 + 2] * p[2];
        } else
            f = p[c] / g.L[c];
        fr[(size_t)c * n + i] = f;
    }
}

// (cos 2 pi r, sin 2 pi r) for |r| <= 1/2 from the half angle h = pi r, |h| <= pi / 2: two polynomials in w = r^2 on
// [0, 1/4], near-minimax fits of 2 sin(pi r) / r and cos(pi r) (error with the rounded coefficients 0.28 and 0.89 units of
// 2^-53 before the Horner roundings), then sin 2h = (2 sin h) cos h and cos 2h = 1 - (2 sin h)^2 / 2.  No quadrant fold,
// no integer work: every instruction of a term is an fp64 one.  The doubling costs a few units of 2^-53 of absolute error
// (|d cos 2h| <= 4 |sin h| |d sin h|), inside the 128 the contract leaves per particle.
__device__ __forceinline__ void sq_cossin(double r, double &c, double &s)
{
    const double w = r * r;
    double ps = 0x1.9d462020fcc78p-20;
    ps = fma(ps, w, -0x1.6f7acdb8f6580p-15);
    ps = fma(ps, w, 0x1.e8f3675ee37ddp-11);
    ps = fma(ps, w, -0x1.e3074dfaf87afp-7);
    ps = fma(ps, w, 0x1.5078348551854p-3);
    ps = fma(ps, w, -0x1.32d2cce627c86p+0);
    ps = fma(ps, w, 0x1.466bc6775aa7dp+2);
    ps = fma(ps, w, -0x1.4abbce625be52p+3);
    ps = fma(ps, w, 0x1.921fb54442d18p+2);
    const double s2 = ps * r;                    // 2 sin h
    double pc = 0x1.1678f9078a9b3p-18;
    pc = fma(pc, w, -0x1.b6957b54dd389p-14);
    pc = fma(pc, w, 0x1.f9d254582ac30p-10);
    pc = fma(pc, w, -0x1.a6d1efc8c38bep-6);
    pc = fma(pc, w, 0x1.e1f506813a321p-3);
    pc = fma(pc, w, -0x1.55d3c7e3bfbf5p+0);
    pc = fma(pc, w, 0x1.03c1f081b5992p+2);
    pc = fma(pc, w, -0x1.3bd3cc9be45dbp+2);
    pc = fma(pc, w, 1.0);                        // cos h
    s = s2 * pc;
    c = fma(s2 * s2, -0.5, 1.0);
}

// What a particle adds to the accumulators of one wave vector -- the term policy of mode_walk: NPV accumulators per
// vector, load(aux, n, i) fetches what particle i brings besides f, add(c, s, acc) adds its term to acc[0..NPV).  Here
// (rho, W) the term is (c, s) itself, a plain add each; CurTerm (md_cur.hpp) is the other one.
struct SqTerm {
    static constexpr int NPV = 2; // Re, Im
    __device__ __forceinline__ void load(const double *, int, int) {}
    __device__ __forceinline__ void add(double c, double s, double *acc) const
    {
#pragma clang fp contract(off)
        acc[0] += c;
        acc[1] += s;
    }
};

// The walk of the wave-vector samplers (k_sq_rho, k_chi4_modes, k_cur_modes): particle block pblk (MD_SQ_BLOCK *
// MD_SQ_PPT ids) against the TILE vectors from v0.  nd: the wave vectors as doubles, 3 per vector (the third 0 in 2-D),
// padded with zero vectors to a multiple of MD_SQ_TILE; aux: what Term::load reads (nullptr for SqTerm).  The tile's
// vectors are wave-uniform (scalar loads), a thread walks its MD_SQ_PPT ids in order with NPV * TILE fp64 accumulators and
// no LDS; then the fixed tree -- a shuffle tree per accumulator, the four wave sums in order -- and one partial per
// (vector, accumulator, block): part[((v0 + j) * NPV + k) * nblk + pblk].
// MASKED (md_chi4.hpp): the same walk over the particles whose bit is set in mask (bit l of word k = particle id
// 64 k + l, nwords words).  The 64 ids of a wave in one iteration are consecutive from a multiple of 64, so they share one
// word: it is loaded once per wave and iteration through a wave-uniform address, a zero word skips the iteration, and a
// particle whose bit is clear adds nothing -- the tree of the sum is the unmasked one.
template <int D, int TILE, bool MASKED, class Term>
__device__ __forceinline__ void mode_walk(int n, int nblk, int pblk, int v0, const double *__restrict__ fr,
                                          const double *__restrict__ aux, const double *__restrict__ nd,
                                          double *__restrict__ part, const unsigned long long *__restrict__ mask, int nwords)
{
#pragma clang fp contract(off)
    constexpr int NPV = Term::NPV, NACC = NPV * TILE;
    __shared__ double wsum[MD_SQ_BLOCK / 64][NACC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double nv[TILE][3];
#pragma unroll
    for (int j = 0; j < TILE; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) nv[j][c] = nd[(size_t)(v0 + j) * 3 + c]; // (uniform: scalar loads)
    double acc[NACC];             // [j * NPV + k]
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    const int base = pblk * (MD_SQ_BLOCK * MD_SQ_PPT) + threadIdx.x;
    for (int m = 0; m < MD_SQ_PPT; ++m) {
        const int i = base + m * MD_SQ_BLOCK;
        bool on = i < n;
        if constexpr (MASKED) {
            const int k = __builtin_amdgcn_readfirstlane(i) >> 6; // (the wave's first id: a multiple of 64)
            const unsigned long long word = k < nwords ? mask[k] : 0ull;
            if (word == 0ull) continue; // (the whole wave)
            on = on && ((word >> lane) & 1ull);
        }
        if (on) {
            const double f0 = fr[i], f1 = fr[(size_t)n + i];
            double f2 = 0.0;
            if constexpr (D == 3) f2 = fr[2 * (size_t)n + i];
            Term term;
            term.load(aux, n, i);
#pragma unroll
            for (int j = 0; j < TILE; ++j) {
                double t = nv[j][0] * f0 + nv[j][1] * f1;
                if constexpr (D == 3) t = t + nv[j][2] * f2;
                const double r = t - rint(t);
                double c, s;
                sq_cossin(r, c, s);
                term.add(c, s, acc + j * NPV);
            }
        }
    }
    // fixed tree: shuffle within the wave, then the waves in order
#pragma unroll
    for (int j = 0; j < TILE; ++j) {
        double w[NPV];
#pragma unroll
        for (int k = 0; k < NPV; ++k) w[k] = sq_wave_sum(acc[j * NPV + k]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NPV; ++k) wsum[wave][j * NPV + k] = w[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        const int k = threadIdx.x;
        double s = wsum[0][k];
#pragma unroll
        for (int w = 1; w < MD_SQ_BLOCK / 64; ++w) s = s + wsum[w][k];
        part[((size_t)v0 * NPV + k) * nblk + pblk] = s;
    }
}

template <int D>
__global__ void __launch_bounds__(MD_SQ_BLOCK)
    k_sq_rho(int n, int nblk, const double *__restrict__ fr, const double *__restrict__ nd, double *__restrict__ part)
{
    mode_walk<D, MD_SQ_TILE, false, SqTerm>(n, nblk, blockIdx.x, blockIdx.y * MD_SQ_TILE, fr, nullptr, nd, part, nullptr, 0);
}

// W of md_chi4.hpp: the walk over the slow particles of one (origin, current frame) pair.
template <int D>
__global__ void __launch_bounds__(MD_SQ_BLOCK)
    k_chi4_modes(int n, int nblk, const double *__restrict__ fr, const double *__restrict__ nd, double *__restrict__ part,
                 const unsigned long long *__restrict__ mask, int nwords)
{
    mode_walk<D, MD_SQ_TILE, true, SqTerm>(n, nblk, blockIdx.x, blockIdx.y * MD_SQ_TILE, fr, nullptr, nd, part, mask, nwords);
}

// The partial tree of k_sq_reduce, k_chi4_reduce and k_cur_reduce: lane 0 of the calling wave gets the sums (a, b) of one
// (Re, Im) pair of partial rows, p[block] and p[nblk + block] -- lane l adds the blocks l, l + 64, ... in order, then a
// shuffle tree.
__device__ __forceinline__ void sq_row_sum(const double *__restrict__ p, int nblk, int lane, double &a, double &b)
{
#pragma clang fp contract(off)
    double x = 0.0, y = 0.0;
    for (int k = lane; k < nblk; k += 64) {
        x += p[k];
        y += p[nblk + k];
    }
    a = sq_wave_sum(x);
    b = sq_wave_sum(y);
}

// One wave per vector.  reduce != 0: rho[v] from the block partials (and |rho|^2 into s2 if add_static); otherwise rho[v]
// is read back (a later batch of the same call).  Then the batch's correlations in call order, then the origin store.
__global__ void __launch_bounds__(MD_SQ_REDUCE_BLOCK)
    k_sq_reduce(int nvec, int nblk, int reduce, int add_static, SqBatch B, int origin_slot,
                const double *__restrict__ part, double *__restrict__ rho, double *__restrict__ s2,
                double *__restrict__ corr, double *__restrict__ org)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * (MD_SQ_REDUCE_BLOCK / 64) + (threadIdx.x >> 6);
    if (v >= nvec) return; // (the whole wave)
    double a, b;
    if (reduce) sq_row_sum(part + (size_t)v * 2 * nblk, nblk, lane, a, b);
    if (lane != 0) return;
    if (reduce) {
        rho[2 * v] = a;
        rho[2 * v + 1] = b;
        if (add_static) s2[v] = s2[v] + (a * a + b * b);
    } else {
        a = rho[2 * v];
        b = rho[2 * v + 1];
    }
    for (int i = 0; i < B.count; ++i) {
        const double *o = org + ((size_t)B.slot[i] * nvec + v) * 2;
        double *r = corr + (size_t)B.row[i] * nvec + v;
        *r = *r + (a * o[0] + b * o[1]);
    }
    if (origin_slot >= 0) {
        double *o = org + ((size_t)origin_slot * nvec + v) * 2;
        o[0] = a;
        o[1] = b;
    }
}
