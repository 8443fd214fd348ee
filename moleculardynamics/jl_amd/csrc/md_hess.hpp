// md_hess.hpp -- the Hessian of the pair energy on the device (md_hess_* in include/mdhip.h).
//
//   HessApplyLane<D, POT, M>   Y = H X for a block of M vectors: one lane per particle walks its OUTER row through the
//                              md_rowwalk.hpp kernel pair, forms the pair's D x D block once and applies it to all M vectors
//   HessDiagLane<D, POT>       the diagonal blocks H_ii = sum_j h_ij
//   k_hess_*                   what the Lanczos iteration around the apply needs: the start vector, the dot products of one
//                              Gram-Schmidt pass (block partials, then a fixed-order finish), the update, the scaling, V S
//
// The pair block.  With t = U'/r, k = U'' (pair_eval2), del = x_j(+translation) - x_i and c = (k - t) / d2:
//   h_ab = fma(c, del_a del_b, t delta_ab)            (del_a del_b rounded first: h_ab == h_ba bit for bit)
//   (H X)_i = sum_j h (X_i - X_j),                    the difference formed before anything is multiplied, fma in b order,
// each lane in row order, fp64, no atomics of any kind: every pair is evaluated from both of its members.
//
// One separation for both members.  Across a periodic face the row walk hands the two members different roundings of the
// same separation.  Here a lane that finds del != fl(x_j - x_i) recovers the lattice translation
// (signs s = rint(U^-1 (del - (x_j - x_i))), vector as shift_xyz forms it) and both members use the form of the LOWER
// slot, fl(fl(x_hi + T) - x_lo), the higher slot negated: d2, t, k and every del_a del_b are then the same bits from either
// member, and the acceptance d2 < pp.c2 is re-decided on that value.  (A pair whose two walk values straddle pp.c2 -- the
// window of section 5 -- is taken by the member whose walk value is inside only if the shared value is inside too.)
#pragma once
#include "md_rowwalk.hpp"

#define MD_HESS_MAX_M 8       // vectors per launch: 2 M D doubles of lane state (48 at M = 8, D = 3)
#define MD_HESS_CHUNK 1024    // elements per block of the dot-product kernel
#define MD_HESS_QPB 8         // vectors of a Gram-Schmidt pass per block of the dot-product kernel

struct HessPairArgs {
    PotParams pp;
    double Ainv[9]; // U^-1, row-major (the handle's), for the lattice signs of a translated neighbour
};

// The separation both members of a pair share (see above), and t = U'/r, k = U'' at it: false when the pair contributes
// nothing.  dx, dy, dz, d2 come in as the walk formed them and go out as the shared form.  (md_elas.hpp uses it too.)
template <int D, int POT>
__device__ __forceinline__ bool hess_sep(const HessPairArgs &P, const DevState &s, int kk, const double4 &pi, double &dx, double &dy,
                                         double &dz, double &d2, uint32_t own, double &t, double &k)
{
#pragma clang fp contract(off)
    if ((int)own == kk) return false; // (a particle's own periodic image: U does not depend on x_i through it)
    const double4 pj = s.pos[own];
    const double tx = dx - (pj.x - pi.x);
    const double ty = dy - (pj.y - pi.y);
    const double tz = (D == 3) ? dz - (pj.z - pi.z) : 0.0;
    if (tx != 0.0 || ty != 0.0 || tz != 0.0) {
        const double *Ai = P.Ainv, *A = s.cellA;
        double s0 = rint((Ai[0] * tx + Ai[1] * ty) + Ai[2] * tz);
        double s1 = rint((Ai[3] * tx + Ai[4] * ty) + Ai[5] * tz);
        double s2 = (D == 3) ? rint((Ai[6] * tx + Ai[7] * ty) + Ai[8] * tz) : 0.0;
        double vx = (s0 * A[0] + s1 * A[1]) + s2 * A[2];
        double vy = (s0 * A[3] + s1 * A[4]) + s2 * A[5];
        double vz = (s0 * A[6] + s1 * A[7]) + s2 * A[8];
        if (kk < (int)own) {
            dx = (pj.x + vx) - pi.x;
            dy = (pj.y + vy) - pi.y;
            if constexpr (D == 3) dz = (pj.z + vz) - pi.z;
        } else {
            dx = -((pi.x - vx) - pj.x);
            dy = -((pi.y - vy) - pj.y);
            if constexpr (D == 3) dz = -((pi.z - vz) - pj.z);
        }
        d2 = d2_ref<D>(dx, dy, dz);
        if (!(d2 < P.pp.c2)) return false;
    }
    pair_eval2<POT>(d2, pi.w, pj.w, P.pp, t, k);
    return true;
}

// The block of one row entry that the walk accepted (hit): false when the pair contributes nothing.
template <int D, int POT>
__device__ __forceinline__ bool hess_pair(const HessPairArgs &P, const DevState &s, int kk, const double4 &pi, double dx, double dy,
                                          double dz, double d2, uint32_t own, double (&h)[D][D])
{
#pragma clang fp contract(off)
    double t, k;
    if (!hess_sep<D, POT>(P, s, kk, pi, dx, dy, dz, d2, own, t, k)) return false;
    const double c = (k - t) * md_rcp(d2);
    const double del[3] = {dx, dy, dz};
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a; b < D; ++b) {
            double p = del[a] * del[b];
            double v = __builtin_fma(c, p, (a == b) ? t : 0.0);
            h[a][b] = v;
            h[b][a] = v;
        }
    return true;
}

// ---- Y = H X ----------------------------------------------------------------------------------------------------------
// X, Y: slot-major, the M D entries of a slot contiguous: [slot][vector][component].
struct HessApplyArgs {
    HessPairArgs P;
    const double *X;
    double *Y;
};

template <int D, int POT, int M>
struct HessApplyLane {
    typedef HessApplyArgs Args;
    double xi[M * D], acc[M * D];
    double4 pi;
    int kk;
    __device__ __forceinline__ void begin(const Args &A, const DevState &, int, int kk_, bool, const double4 &pi_)
    {
        kk = kk_;
        pi = pi_;
        const double *x = A.X + (size_t)kk * (M * D);
#pragma unroll
        for (int q = 0; q < M * D; ++q) {
            xi[q] = x[q];
            acc[q] = 0.0;
        }
    }
    __device__ __forceinline__ void visit(const Args &A, const DevState &s, bool hit, double dx, double dy, double dz, double d2,
                                          uint32_t own)
    {
        if (!hit) return;
        double h[D][D];
        if (!hess_pair<D, POT>(A.P, s, kk, pi, dx, dy, dz, d2, own, h)) return;
        const double *xj = A.X + (size_t)own * (M * D);
#pragma unroll
        for (int v = 0; v < M; ++v) {
            double e[D];
#pragma unroll
            for (int b = 0; b < D; ++b) e[b] = xi[v * D + b] - xj[v * D + b];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) acc[v * D + a] = __builtin_fma(h[a][b], e[b], acc[v * D + a]);
        }
    }
    __device__ __forceinline__ void end(const Args &A, int k, bool active, int)
    {
        if (!active) return;
        double *y = A.Y + (size_t)k * (M * D);
#pragma unroll
        for (int q = 0; q < M * D; ++q) y[q] = acc[q];
    }
};

// ---- the diagonal blocks ----------------------------------------------------------------------------------------------
struct HessDiagArgs {
    HessPairArgs P;
    double *diag; // [slot][a][b]
};

template <int D, int POT>
struct HessDiagLane {
    typedef HessDiagArgs Args;
    double acc[D][D];
    double4 pi;
    int kk;
    __device__ __forceinline__ void begin(const Args &, const DevState &, int, int kk_, bool, const double4 &pi_)
    {
        kk = kk_;
        pi = pi_;
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b) acc[a][b] = 0.0;
    }
    __device__ __forceinline__ void visit(const Args &A, const DevState &s, bool hit, double dx, double dy, double dz, double d2,
                                          uint32_t own)
    {
        if (!hit) return;
        double h[D][D];
        if (!hess_pair<D, POT>(A.P, s, kk, pi, dx, dy, dz, d2, own, h)) return;
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b) acc[a][b] = acc[a][b] + h[a][b];
    }
    __device__ __forceinline__ void end(const Args &A, int k, bool active, int)
    {
        if (!active) return;
        double *o = A.diag + (size_t)k * (D * D);
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b) o[a * D + b] = acc[a][b];
    }
};

// ---- between particle-id order (host arrays) and slot order (the resident vectors) --------------------------------------
// in: [m][n][D] by particle id; out: [slot][M][D], vectors m .. M-1 zero.
__global__ void __launch_bounds__(MD_BLOCK)
    k_hess_import(int n, const int32_t *__restrict__ id, int D, int m, int M, const double *__restrict__ in, double *__restrict__ out)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t i = (size_t)id[k];
    for (int v = 0; v < M; ++v)
        for (int a = 0; a < D; ++a)
            out[((size_t)k * M + v) * D + a] = (v < m) ? in[((size_t)v * n + i) * D + a] : 0.0;
}

// in: [slot][M][D] (per = M D) or any [slot][per] block; out: [m][n][per / M] by particle id (m = M: a plain permutation).
__global__ void __launch_bounds__(MD_BLOCK)
    k_hess_export(int n, const int32_t *__restrict__ id, int D, int m, int M, const double *__restrict__ in, double *__restrict__ out)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t i = (size_t)id[k];
    for (int v = 0; v < m; ++v)
        for (int a = 0; a < D; ++a) out[((size_t)v * n + i) * D + a] = in[((size_t)k * M + v) * D + a];
}

// ---- Lanczos with full reorthogonalisation, everything resident ---------------------------------------------------------
// Vectors are [slot][D] (the apply's layout at M = 1), nd = n D elements.  The vectors a pass projects against are numbered
// q = 0 .. D-1: the uniform translations (1/sqrt(n) in component q of every particle), q = D + i: basis vector i.
__device__ __forceinline__ double hess_q_elem(int q, size_t e, int D, double rsn, const double *__restrict__ V, size_t nd)
{
    if (q < D) return ((int)(e % (size_t)D) == q) ? rsn : 0.0;
    return V[(size_t)(q - D) * nd + e];
}

// Start vector: Philox words keyed by (seed, particle id), component a = 2 u_a - 1.
__global__ void __launch_bounds__(MD_BLOCK)
    k_hess_start(int n, const int32_t *__restrict__ id, int D, unsigned long long seed, double *__restrict__ w)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t r[4];
    philox4x32_10((uint32_t)id[k], 0x48455353u /* "HESS" */, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    for (int a = 0; a < D; ++a) {
        double u = ((double)r[a] + 0.5) * 2.3283064365386963e-10;
        w[(size_t)k * D + a] = 2.0 * u - 1.0;
    }
}

// partials[q * nchunk + chunk] = sum over the chunk's elements of w[e] * Q_q[e], q = q0 .. q0 + nq - 1 (self != 0: the
// one "vector" is w itself, partials[chunk] = sum w^2).  Thread order, then block_sum's tree: fixed.
__global__ void __launch_bounds__(MD_BLOCK)
    k_hess_dots(size_t nd, int D, double rsn, const double *__restrict__ V, const double *__restrict__ w, int q0, int nq, int self,
                double *__restrict__ partials)
{
    __shared__ double red[16];
    const int nchunk = gridDim.x;
    const size_t e0 = (size_t)blockIdx.x * MD_HESS_CHUNK;
    constexpr int PER = MD_HESS_CHUNK / MD_BLOCK;
    double wv[PER];
    size_t ev[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        ev[i] = e0 + (size_t)i * MD_BLOCK + threadIdx.x;
        wv[i] = (ev[i] < nd) ? w[ev[i]] : 0.0;
    }
    // (blockIdx.y: MD_HESS_QPB vectors per block, so a long pass over a short vector still fills the device)
    const int qlo = blockIdx.y * MD_HESS_QPB, qhi = min(nq, qlo + MD_HESS_QPB);
    for (int qi = qlo; qi < qhi; ++qi) {
        const int q = q0 + qi;
        double a = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            double qv = 0.0;
            if (ev[i] < nd) qv = self ? wv[i] : hess_q_elem(q, ev[i], D, rsn, V, nd);
            a = __builtin_fma(wv[i], qv, a);
        }
        double t = block_sum(a, red);
        if (threadIdx.x == 0) partials[(size_t)qi * nchunk + blockIdx.x] = t;
    }
}

// One block per q: coef[q] = the chunk partials in chunk order (strided_sum + block_sum).  mode 0: plain.  mode 1: also
// alpha[0] = coef of q == qa (first pass).  mode 2: alpha[0] += coef of q == qa (second pass).  mode 3: coef[0] =
// beta[0] = sqrt(sum) (the norm).
__global__ void __launch_bounds__(MD_BLOCK)
    k_hess_dots_finish(int nchunk, const double *__restrict__ partials, double *__restrict__ coef, int mode, int qa,
                       double *__restrict__ out)
{
    __shared__ double red[16];
    const int q = blockIdx.x;
    double a = strided_sum<4>(partials + (size_t)q * nchunk, nchunk);
    a = block_sum(a, red);
    if (threadIdx.x != 0) return;
    if (mode == 3) {
        a = sqrt(a);
        out[0] = a;
    } else if (q == qa) {
        if (mode == 1) out[0] = a;
        if (mode == 2) out[0] = out[0] + a;
    }
    coef[q] = a;
}

// w -= sum_q coef[q] Q_q, q = 0 .. nq-1 in that order
__global__ void __launch_bounds__(MD_BLOCK)
    k_hess_update(size_t nd, int D, double rsn, const double *__restrict__ V, const double *__restrict__ coef, int nq,
                  double *__restrict__ w)
{
    size_t e = (size_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    if (e >= nd) return;
    double a = w[e];
    for (int q = 0; q < nq; ++q) a = __builtin_fma(-coef[q], hess_q_elem(q, e, D, rsn, V, nd), a);
    w[e] = a;
}

// out = w / beta[0]
__global__ void __launch_bounds__(MD_BLOCK)
    k_hess_scale(size_t nd, const double *__restrict__ w, const double *__restrict__ beta, double *__restrict__ out)
{
    size_t e = (size_t)blockIdx.x * MD_BLOCK + threadIdx.x;
    if (e >= nd) return;
    out[e] = w[e] / beta[0];
}

// Y[slot][c][a] = sum_j V_j[slot][a] S[j][c0 + c], c = 0 .. M-1 (columns past nvec: zero), j in order.  S is k x nvec.
__global__ void __launch_bounds__(MD_BLOCK)
    k_hess_combine(int n, int D, size_t nd, int ksteps, int nvec, int c0, int M, const double *__restrict__ V,
                   const double *__restrict__ S, double *__restrict__ Y)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    for (int c = 0; c < M; ++c)
        for (int a = 0; a < D; ++a) {
            double y = 0.0;
            if (c0 + c < nvec)
                for (int j = 0; j < ksteps; ++j)
                    y = __builtin_fma(V[(size_t)j * nd + (size_t)k * D + a], S[(size_t)j * nvec + c0 + c], y);
            Y[((size_t)k * M + c) * D + a] = y;
        }
}
