// md_elas.hpp -- elastic moduli of a minimum on the device (md_elas_* in include/mdhip.h).
//
//   ElasAffineLane<D, POT>     one lane per particle walks its OUTER row through the md_rowwalk.hpp kernel pair: the affine
//                              force field Xi_i (nc D doubles), its half of the nc stress sums and of the 15 (3-D) or 5
//                              (2-D) Born sums, and whether the particle has a bond at all
//   k_elas_affine_finish       the block partials in block order, times 0.5 (exact) and 1/V
//   k_elas_*                   column-wise conjugate gradients for H u_c = -Xi_c, c = 0 .. nc-1 at once, everything resident
//                              in the apply's slot-major layout [slot][M][D], M = hess_block(nc): the masked translation
//                              projection, the dot products (chunk partials, then a fixed-order finish that also forms
//                              alpha_c and beta_c), the two updates, the true residual and the contraction Xi_s . u_t
//
// Per accepted pair (hess_sep: the pairs and the separation of md_hess_*), with t = U'/r, k = U'', c = (k - t) / d2,
// del = x_j(+translation) - x_i and p_ab = del_a del_b (rounded first):
//   sigma_ab  += t p_ab                                          fma(t, p_ab, .)
//   CB_abcd   += c p_ab p_cd        (a <= b <= c <= d)           fma(c p_ab, p_cd, .)
//   Xi_{c;ab} -= c p_ab del_c + t (delta_ac del_b + delta_bc del_a)      . - fma(c p_ab, del_c, t del_x)
// each lane in row order, fp64, no atomics.  Every operation is odd or even in del, and both members of a pair hold the same
// del bits with opposite signs: their Xi terms are exact negatives of each other, their sigma and CB terms equal.
//
// Components: 3-D xx, yy, zz, xy, xz, yz (nc = 6); 2-D xx, yy, xy (nc = 3) -- the stress sampler's order.  The unique Born
// entries are numbered by the loops a <= b <= c <= d (elas_born_index below, host and device).
//
// The vector kernels give one thread one (slot, vector) PAIR, D contiguous doubles: thread g of a block serves the pairs
// base + i * MD_BLOCK + g, so its vector v = g % M never changes (M divides MD_BLOCK) and consecutive threads read
// consecutive memory.  A per-vector sum is then wave shuffles over the lanes of equal g % M, the waves in order
// (col_block_sum), one partial per (vector, chunk), and a finish kernel adds the chunks in chunk order.
#pragma once
#include "md_hess.hpp"

#define MD_ELAS_PER 4                           // pairs per thread of a vector kernel
#define MD_ELAS_CHUNK (MD_BLOCK * MD_ELAS_PER)  // pairs per block
#define MD_ELAS_MAX_NQ 22                       // affine sums: 6 stress + 15 Born + the bonded count (3-D)

#define MD_ELAS_ST_ACTIVE 0
#define MD_ELAS_ST_CONVERGED 1
#define MD_ELAS_ST_INDEFINITE 2

template <int D>
struct ElasShape {
    static constexpr int NC = (D == 3) ? 6 : 3;   // strain components
    static constexpr int NB = (D == 3) ? 15 : 5;  // unique Born entries
    static constexpr int NQ = NC + NB + 1;        // block sums of the affine pass (the last: bonded particles)
    static constexpr int M = (D == 3) ? 8 : 4;    // hess_block(NC)
};

// component s -> (a, b), a <= b, and back
__host__ __device__ constexpr int elas_ca(int D, int s) { return s < D ? s : (D == 3 ? (s == 5 ? 1 : 0) : 0); }
__host__ __device__ constexpr int elas_cb(int D, int s) { return s < D ? s : (D == 3 ? (s == 3 ? 1 : 2) : 1); }
__host__ __device__ constexpr int elas_comp(int D, int a, int b) { return a == b ? a : (D == 3 ? a + b + 2 : 2); }

// the number of the unique Born entry of four sorted indices a <= b <= c <= d
inline int elas_born_index(int D, int a, int b, int c, int d)
{
    int q = 0;
    for (int i = 0; i < D; ++i)
        for (int j = i; j < D; ++j)
            for (int k = j; k < D; ++k)
                for (int l = k; l < D; ++l, ++q)
                    if (i == a && j == b && k == c && l == d) return q;
    return -1;
}

// ---- the affine pass ---------------------------------------------------------------------------------------------------
struct ElasAffineArgs {
    HessPairArgs P;
    double *xi;        // [slot][M][D], vectors nc .. M-1 zero
    int32_t *bonded;   // [slot]: 1 when some accepted pair has t != 0 or k != 0 (the particle's row of H is not zero)
    double *partials;  // [NQ][nblk]
    int nblk;
};

template <int D, int POT>
struct ElasAffineLane {
    typedef ElasAffineArgs Args;
    static constexpr int NC = ElasShape<D>::NC, NB = ElasShape<D>::NB, M = ElasShape<D>::M;
    double xi[NC * D], sg[NC], cb[NB];
    double4 pi;
    int kk, bonded;
    __device__ __forceinline__ void begin(const Args &, const DevState &, int, int kk_, bool, const double4 &pi_)
    {
        kk = kk_;
        pi = pi_;
        bonded = 0;
#pragma unroll
        for (int q = 0; q < NC * D; ++q) xi[q] = 0.0;
#pragma unroll
        for (int q = 0; q < NC; ++q) sg[q] = 0.0;
#pragma unroll
        for (int q = 0; q < NB; ++q) cb[q] = 0.0;
    }
    __device__ __forceinline__ void visit(const Args &A, const DevState &s, bool hit, double dx, double dy, double dz, double d2,
                                          uint32_t own)
    {
#pragma clang fp contract(off)
        if (!hit) return;
        double t, k;
        if (!hess_sep<D, POT>(A.P, s, kk, pi, dx, dy, dz, d2, own, t, k)) return;
        const double c = (k - t) * md_rcp(d2);
        const double del[3] = {dx, dy, dz};
        if (t != 0.0 || k != 0.0) bonded = 1;
        double p[NC], cp[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            p[q] = del[elas_ca(D, q)] * del[elas_cb(D, q)];
            cp[q] = c * p[q];
            sg[q] = __builtin_fma(t, p[q], sg[q]);
        }
        {
            int q = 0;
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = a; b < D; ++b)
#pragma unroll
                    for (int e = b; e < D; ++e)
#pragma unroll
                        for (int f = e; f < D; ++f, ++q) cb[q] = __builtin_fma(cp[elas_comp(D, a, b)], p[elas_comp(D, e, f)], cb[q]);
        }
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int a = elas_ca(D, q), b = elas_cb(D, q);
#pragma unroll
            for (int e = 0; e < D; ++e) {
                double tt = 0.0;
                if (a == b) {
                    if (e == a) tt = (2.0 * t) * del[a];
                } else {
                    if (e == a) tt = t * del[b];
                    if (e == b) tt = t * del[a];
                }
                xi[q * D + e] = xi[q * D + e] - __builtin_fma(cp[q], del[e], tt);
            }
        }
    }
    __device__ __forceinline__ void end(const Args &A, int k, bool active, int bid)
    {
        __shared__ double red[16];
        if (active) {
            double *o = A.xi + (size_t)k * (M * D);
#pragma unroll
            for (int q = 0; q < M * D; ++q) o[q] = (q < NC * D) ? xi[q] : 0.0;
            A.bonded[k] = bonded;
        } else {
            bonded = 0;
#pragma unroll
            for (int q = 0; q < NC; ++q) sg[q] = 0.0;
#pragma unroll
            for (int q = 0; q < NB; ++q) cb[q] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            double t = block_sum(sg[q], red);
            if (threadIdx.x == 0) A.partials[(size_t)q * A.nblk + bid] = t;
        }
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            double t = block_sum(cb[q], red);
            if (threadIdx.x == 0) A.partials[(size_t)(NC + q) * A.nblk + bid] = t;
        }
        double t = block_sum((double)bonded, red);
        if (threadIdx.x == 0) A.partials[(size_t)(NC + NB) * A.nblk + bid] = t;
    }
};

// One block per sum: the block partials in block order (strided_sum + block_sum).  out[q] = (sum * 0.5) * inv_v for the
// stress and Born sums (every pair was evaluated from both ends), out[nq - 1] = the bonded count as it is.
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_affine_finish(int nblk, int nq, const double *__restrict__ partials, double inv_v, double *__restrict__ out)
{
    __shared__ double red[16];
    const int q = blockIdx.x;
    double a = strided_sum<4>(partials + (size_t)q * nblk, nblk);
    a = block_sum(a, red);
    if (threadIdx.x != 0) return;
    out[q] = (q == nq - 1) ? a : (a * 0.5) * inv_v;
}

// ---- per-vector sums over the interleaved layout -------------------------------------------------------------------------
// The sum of v over the threads of equal threadIdx.x % M: valid in threads 0 .. M-1 (thread g holds vector g).  Shuffles
// with strides that are multiples of M, then the waves in order: fixed.  Contains barriers.
template <int M>
__device__ __forceinline__ double col_block_sum(double v, double *lds /* >= 4 * M doubles */)
{
#pragma unroll
    for (int off = 32; off >= M; off >>= 1) v = v + __shfl_xor(v, off);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane < M) lds[w * M + lane] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < M)
        for (int i = 0; i < MD_BLOCK / 64; ++i) r += lds[i * M + threadIdx.x];
    return r;
}

// The solver's scalars, one set per vector
struct ElasScal {
    double rr[MD_HESS_MAX_M];     // r . r of the recurrence
    double rr0[MD_HESS_MAX_M];    // |projected Xi_c|^2
    double thr2[MD_HESS_MAX_M];   // tol^2 rr0
    double php[MD_HESS_MAX_M];    // the last p . H p
    double alpha[MD_HESS_MAX_M], beta[MD_HESS_MAX_M];
    long long iters[MD_HESS_MAX_M];
    int state[MD_HESS_MAX_M];     // MD_ELAS_ST_*
    int nactive;                  // vectors still iterating
    int pad;
};

struct ElasVecs {
    size_t npair;              // n M
    const int32_t *bonded;     // [slot]
    const double *xi;          // the right-hand sides as the affine pass left them
    double *x, *r, *p, *hp;    // [slot][M][D]
    double *partials;          // [.][nchunk]
    ElasScal *sc;
    const double *mean;        // [M][D]: masked translation component
};

// partials[(v D + a) nchunk + chunk] = sum over the chunk's slots of src[slot][v][a]  (the translation component; a
// particle without bonds holds exact zeros and is not part of the translation the solver projects against)
template <int D, int M>
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_colsum(size_t npair, const double *__restrict__ src, double *__restrict__ partials)
{
    __shared__ double red[4 * M];
    const int nchunk = gridDim.x;
    const size_t g0 = (size_t)blockIdx.x * MD_ELAS_CHUNK + threadIdx.x;
    double a[D];
#pragma unroll
    for (int e = 0; e < D; ++e) a[e] = 0.0;
#pragma unroll
    for (int i = 0; i < MD_ELAS_PER; ++i) {
        const size_t g = g0 + (size_t)i * MD_BLOCK;
        if (g < npair) {
#pragma unroll
            for (int e = 0; e < D; ++e) a[e] = a[e] + src[g * D + e];
        }
    }
#pragma unroll
    for (int e = 0; e < D; ++e) {
        double t = col_block_sum<M>(a[e], red);
        if (threadIdx.x < M) partials[((size_t)threadIdx.x * D + e) * nchunk + blockIdx.x] = t;
    }
}

// One block per (v, a): mean[q] = (the chunk partials in chunk order) / (bonded particles), 0 when nobody is bonded
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_mean_finish(int nchunk, const double *__restrict__ partials, const double *__restrict__ nbonded, double *__restrict__ mean)
{
    __shared__ double red[16];
    const int q = blockIdx.x;
    double a = strided_sum<4>(partials + (size_t)q * nchunk, nchunk);
    a = block_sum(a, red);
    if (threadIdx.x != 0) return;
    mean[q] = nbonded[0] > 0.0 ? a / nbonded[0] : 0.0;
}

// x = 0, r = p = -(Xi - mean) on bonded particles and exactly 0 on the others; partials[v nchunk + chunk] = the chunk's r . r
template <int D, int M>
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_init(ElasVecs V)
{
    __shared__ double red[4 * M];
    const int nchunk = gridDim.x;
    const size_t g0 = (size_t)blockIdx.x * MD_ELAS_CHUNK + threadIdx.x;
    const int v = threadIdx.x % M;
    double m[D];
#pragma unroll
    for (int e = 0; e < D; ++e) m[e] = V.mean[v * D + e];
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < MD_ELAS_PER; ++i) {
        const size_t g = g0 + (size_t)i * MD_BLOCK;
        if (g < V.npair) {
            const bool b = V.bonded[g / M] != 0;
#pragma unroll
            for (int e = 0; e < D; ++e) {
                double r = b ? -(V.xi[g * D + e] - m[e]) : 0.0;
                V.x[g * D + e] = 0.0;
                V.r[g * D + e] = r;
                V.p[g * D + e] = r;
                a = __builtin_fma(r, r, a);
            }
        }
    }
    double t = col_block_sum<M>(a, red);
    if (threadIdx.x < M) V.partials[(size_t)threadIdx.x * nchunk + blockIdx.x] = t;
}

// partials[v nchunk + chunk] = the chunk's p . H p
template <int D, int M>
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_php(ElasVecs V)
{
    __shared__ double red[4 * M];
    const int nchunk = gridDim.x;
    const size_t g0 = (size_t)blockIdx.x * MD_ELAS_CHUNK + threadIdx.x;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < MD_ELAS_PER; ++i) {
        const size_t g = g0 + (size_t)i * MD_BLOCK;
        if (g < V.npair) {
#pragma unroll
            for (int e = 0; e < D; ++e) a = __builtin_fma(V.p[g * D + e], V.hp[g * D + e], a);
        }
    }
    double t = col_block_sum<M>(a, red);
    if (threadIdx.x < M) V.partials[(size_t)threadIdx.x * nchunk + blockIdx.x] = t;
}

// x += alpha p, r -= alpha H p; partials[v nchunk + chunk] = the chunk's new r . r.  A frozen vector has alpha = 0: its x
// and r keep their bits.
template <int D, int M>
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_update(ElasVecs V)
{
    __shared__ double red[4 * M];
    const int nchunk = gridDim.x;
    const size_t g0 = (size_t)blockIdx.x * MD_ELAS_CHUNK + threadIdx.x;
    const double al = V.sc->alpha[threadIdx.x % M];
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < MD_ELAS_PER; ++i) {
        const size_t g = g0 + (size_t)i * MD_BLOCK;
        if (g < V.npair) {
#pragma unroll
            for (int e = 0; e < D; ++e) {
                const size_t q = g * D + e;
                V.x[q] = __builtin_fma(al, V.p[q], V.x[q]);
                double r = __builtin_fma(-al, V.hp[q], V.r[q]);
                V.r[q] = r;
                a = __builtin_fma(r, r, a);
            }
        }
    }
    double t = col_block_sum<M>(a, red);
    if (threadIdx.x < M) V.partials[(size_t)threadIdx.x * nchunk + blockIdx.x] = t;
}

// p = r + beta p
template <int D, int M>
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_direction(ElasVecs V)
{
    const size_t g0 = (size_t)blockIdx.x * MD_ELAS_CHUNK + threadIdx.x;
    const double be = V.sc->beta[threadIdx.x % M];
#pragma unroll
    for (int i = 0; i < MD_ELAS_PER; ++i) {
        const size_t g = g0 + (size_t)i * MD_BLOCK;
        if (g < V.npair) {
#pragma unroll
            for (int e = 0; e < D; ++e) {
                const size_t q = g * D + e;
                V.p[q] = __builtin_fma(be, V.p[q], V.r[q]);
            }
        }
    }
}

// x -= mean on bonded particles (the solution's masked translation component, once, after the loop)
template <int D, int M>
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_project(ElasVecs V)
{
    const size_t g0 = (size_t)blockIdx.x * MD_ELAS_CHUNK + threadIdx.x;
    const int v = threadIdx.x % M;
#pragma unroll
    for (int i = 0; i < MD_ELAS_PER; ++i) {
        const size_t g = g0 + (size_t)i * MD_BLOCK;
        if (g < V.npair && V.bonded[g / M] != 0) {
#pragma unroll
            for (int e = 0; e < D; ++e) V.x[g * D + e] = V.x[g * D + e] - V.mean[v * D + e];
        }
    }
}

// partials[v nchunk + chunk] = the chunk's |H x + Xi|^2 (hp holds H x): the TRUE residual against the unprojected Xi
template <int D, int M>
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_resid(ElasVecs V)
{
    __shared__ double red[4 * M];
    const int nchunk = gridDim.x;
    const size_t g0 = (size_t)blockIdx.x * MD_ELAS_CHUNK + threadIdx.x;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < MD_ELAS_PER; ++i) {
        const size_t g = g0 + (size_t)i * MD_BLOCK;
        if (g < V.npair) {
#pragma unroll
            for (int e = 0; e < D; ++e) {
                double r = V.hp[g * D + e] + V.xi[g * D + e];
                a = __builtin_fma(r, r, a);
            }
        }
    }
    double t = col_block_sum<M>(a, red);
    if (threadIdx.x < M) V.partials[(size_t)threadIdx.x * nchunk + blockIdx.x] = t;
}

// The three finishes of the loop, one block each: the M per-vector sums in chunk order (strided_sum + block_sum), then
// thread 0 forms the scalars.
//   mode 0 (after k_elas_init):   rr = rr0 = sum, thr2 = tol^2 rr0; a vector with rr <= thr2 (a zero right-hand side, the
//                                 padding vectors) is converged at 0 iterations; nactive
//   mode 1 (after k_elas_php):    php = sum; alpha = rr / php, or -- p . H p <= 0 (or not finite) -- the vector is frozen
//                                 as indefinite; alpha = 0 for every frozen vector
//   mode 2 (after k_elas_update): beta = sum / rr, rr = sum, iters += 1; rr <= thr2 freezes the vector as converged;
//                                 beta = 0 for every frozen vector; nactive
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_scalars(int nchunk, int M, int mode, double tol, const double *__restrict__ partials, ElasScal *__restrict__ sc)
{
    __shared__ double red[16];
    double s[MD_HESS_MAX_M];
    for (int v = 0; v < M; ++v) {
        double a = strided_sum<4>(partials + (size_t)v * nchunk, nchunk);
        s[v] = block_sum(a, red);
    }
    if (threadIdx.x != 0) return;
    int nactive = 0;
    for (int v = 0; v < M; ++v) {
        if (mode == 0) {
            sc->rr[v] = s[v];
            sc->rr0[v] = s[v];
            sc->thr2[v] = (tol * tol) * s[v];
            sc->php[v] = 0.0;
            sc->alpha[v] = 0.0;
            sc->beta[v] = 0.0;
            sc->iters[v] = 0;
            sc->state[v] = (s[v] <= sc->thr2[v]) ? MD_ELAS_ST_CONVERGED : MD_ELAS_ST_ACTIVE;
        } else if (sc->state[v] != MD_ELAS_ST_ACTIVE) {
            sc->alpha[v] = 0.0;
            sc->beta[v] = 0.0;
        } else if (mode == 1) {
            sc->php[v] = s[v];
            if (s[v] > 0.0 && s[v] <= 1.7976931348623157e308) {
                sc->alpha[v] = sc->rr[v] / s[v];
            } else {
                sc->state[v] = MD_ELAS_ST_INDEFINITE;
                sc->alpha[v] = 0.0;
                sc->beta[v] = 0.0;
            }
        } else {
            sc->beta[v] = s[v] / sc->rr[v];
            sc->rr[v] = s[v];
            sc->iters[v] = sc->iters[v] + 1;
            if (!(s[v] > sc->thr2[v])) {
                sc->state[v] = (s[v] <= sc->thr2[v]) ? MD_ELAS_ST_CONVERGED : MD_ELAS_ST_INDEFINITE; // (NaN: give up)
                sc->beta[v] = 0.0;
            }
        }
        if (sc->state[v] == MD_ELAS_ST_ACTIVE) ++nactive;
    }
    sc->nactive = nactive;
}

// One block per sum: out[q] = scale * (the chunk partials in chunk order), or its square root (root != 0)
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_sum_finish(int nchunk, const double *__restrict__ partials, double scale, int root, double *__restrict__ out)
{
    __shared__ double red[16];
    const int q = blockIdx.x;
    double a = strided_sum<4>(partials + (size_t)q * nchunk, nchunk);
    a = block_sum(a, red);
    if (threadIdx.x != 0) return;
    out[q] = root ? sqrt(a) : a * scale;
}

// ---- the contraction -----------------------------------------------------------------------------------------------------
// partials[(s nc + t) nblk + block] = sum over the block's slots of Xi_s[slot] . u_t[slot]: one thread per slot, the D
// products in component order, then block_sum.  Not symmetrised: the asymmetry measures the solve's error.
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_elas_contract(int n, const double *__restrict__ xi, const double *__restrict__ u, double *__restrict__ partials)
{
    constexpr int NC = ElasShape<D>::NC, M = ElasShape<D>::M;
    __shared__ double red[16];
    const int nblk = gridDim.x;
    const int k = blockIdx.x * MD_BLOCK + threadIdx.x;
    double a[NC * D], b[NC * D];
#pragma unroll
    for (int q = 0; q < NC * D; ++q) {
        a[q] = (k < n) ? xi[(size_t)k * (M * D) + q] : 0.0;
        b[q] = (k < n) ? u[(size_t)k * (M * D) + q] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < NC; ++s)
#pragma unroll
        for (int t = 0; t < NC; ++t) {
            double v = 0.0;
#pragma unroll
            for (int e = 0; e < D; ++e) v = __builtin_fma(a[s * D + e], b[t * D + e], v);
            double w = block_sum(v, red);
            if (threadIdx.x == 0) partials[(size_t)(s * NC + t) * nblk + blockIdx.x] = w;
        }
}
