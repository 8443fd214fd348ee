// md_boo.hpp -- bond-orientational order, sampled on the device (md_boo_* in include/mdhip.h): Steinhardt q_l (l = 4, 6)
// and its neighbour-averaged form in 3-D, the k-fold psi_k in 2-D, ten Wolde's solid-bond count.
//
// One sample = three launches on the handle's stream, no host wait; the first two are md_rowwalk.hpp's kernel pair
// (k_rows_tile / k_rows: one lane per particle walks its OUTER row) with the lanes below:
//   BooQlmLane     pass 1: accumulates sum_j Y_lm(u_ij) for m = 0..l and n_i, writes q_lm, its 2-norm and n_i per slot
//   BooAvgLane     pass 2: the same walk and the same acceptance test; every hit gathers the neighbour's q_lm by OWNER
//                  slot (orientations are translation invariant: a ghost's q_lm is its owner's), accumulates Q_lm and
//                  the bond coherence s_ij; q, qbar, c per slot, the histograms, per-block partials
//   k_boo_finish   one block: the partials in block order, the frame vector, the running sums, the series
//
// Arithmetic contract: del = x_j(+translation) - x_i as the force kernels form it, j is a neighbour
// iff d2_ref(del) < rn2, everything fp64.  Y_lm(u) = c_lm D_l^m(u_z) (u_x + i u_y)^m with D_l^m = d^m P_l / dz^m a
// polynomial and c_lm = (-1)^m sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!): no atan2, acos or sincos.  The lane sums the
// unnormalised D_l^m (u_x + i u_y)^m in row order and applies c_lm / n_i once.  Reductions: block_sum, then one block over
// the partials in block order -- no floating-point atomics; the histograms are integer atomics.
#pragma once
#include "md_rowwalk.hpp"

#define MD_BOO_MAX_BINS 8192
#define MD_BOO_MAX_SERIES (1 << 20)
#define MD_BOO_NCLAMP 32   // n_i and c_i are histogrammed in 0..32, the last bin holding everything above
#define MD_BOO_LDS_BINS 1024 // up to this many bins the q / qbar histograms are gathered per block in LDS first
#define MD_BOO_NFR 8

// Per-order constants, formed on the host: coef[m] = c_lm (2-D: coef[0] = 1), pref = 4 pi / (2l + 1) (2-D: 1).
struct BooCoef {
    double coef[7];
    double pref;
};

template <int D, int L>
struct BooShape {
    static constexpr int NM = (D == 3) ? L + 1 : 1;
    static constexpr int NC = 2 * NM;           // real components per particle
    static constexpr int NPART = 7 + NC;        // block partials: 6 sums, the solid count, sum n_i q_lm
};

// 1 / sqrt(a): v_rsq_f64 seed and two Newton steps (full fp64 accuracy for normal-range a)
__device__ __forceinline__ double boo_rsqrt(double a)
{
    double y = __builtin_amdgcn_rsq(a);
    double h = 0.5 * a;
    y = y * __builtin_fma(-h * y, y, 1.5);
    y = y * __builtin_fma(-h * y, y, 1.5);
    return y;
}

// D_l^m(z) = d^m P_l / dz^m
template <int L>
__device__ __forceinline__ void boo_legendre(double z, double (&d)[L + 1])
{
    static_assert(L == 4 || L == 6, "only l = 4 and l = 6 are tabulated");
    const double z2 = z * z;
    if constexpr (L == 4) {
        d[0] = __builtin_fma(__builtin_fma(35.0, z2, -30.0), z2, 3.0) * 0.125;
        d[1] = __builtin_fma(35.0, z2, -15.0) * z * 0.5;
        d[2] = __builtin_fma(105.0, z2, -15.0) * 0.5;
        d[3] = 105.0 * z;
        d[4] = 105.0;
    } else {
        d[0] = __builtin_fma(__builtin_fma(__builtin_fma(231.0, z2, -315.0), z2, 105.0), z2, -5.0) * 0.0625;
        d[1] = __builtin_fma(__builtin_fma(693.0, z2, -630.0), z2, 105.0) * z * 0.125;
        d[2] = __builtin_fma(__builtin_fma(3465.0, z2, -1890.0), z2, 105.0) * 0.125;
        d[3] = __builtin_fma(3465.0, z2, -945.0) * z * 0.5;
        d[4] = __builtin_fma(10395.0, z2, -945.0) * 0.5;
        d[5] = 10395.0 * z;
        d[6] = 10395.0;
    }
}

// One candidate of pass 1: a[2m], a[2m+1] += Re, Im of D_l^m(u_z) (u_x + i u_y)^m (3-D) or of (u_x + i u_y)^k (2-D).
// A rejected candidate adds exact zeros: its unit vector and the zeroth power are replaced by 0.
template <int D, int L, int NC>
__device__ __forceinline__ void boo_add(double (&a)[NC], bool hit, double dx, double dy, double dz,
                                        double d2, int korder)
{
    static_assert(NC == BooShape<D, L>::NC, "one accumulator pair per stored m");
    const double rinv = boo_rsqrt(hit ? d2 : 1.0);
    const double er = hit ? dx * rinv : 0.0;
    const double ei = hit ? dy * rinv : 0.0;
    double pr = hit ? 1.0 : 0.0, pim = 0.0;
    if constexpr (D == 3) {
        const double z = hit ? dz * rinv : 0.0;
        double d[L + 1];
        boo_legendre<L>(z, d);
        a[0] = __builtin_fma(d[0], pr, a[0]);
#pragma unroll
        for (int m = 1; m <= L; ++m) {
            const double tr = __builtin_fma(pr, er, -(pim * ei));
            const double ti = __builtin_fma(pr, ei, pim * er);
            pr = tr;
            pim = ti;
            a[2 * m] = __builtin_fma(d[m], pr, a[2 * m]);
            a[2 * m + 1] = __builtin_fma(d[m], pim, a[2 * m + 1]);
        }
    } else {
        for (int m = 0; m < korder; ++m) {
            const double tr = __builtin_fma(pr, er, -(pim * ei));
            const double ti = __builtin_fma(pr, ei, pim * er);
            pr = tr;
            pim = ti;
        }
        a[0] += pr;
        a[1] += pim;
    }
}

// |q|^2 over all m = -l..l from the stored half: |q_0|^2 + 2 sum_{m>0} |q_m|^2, in this order
template <int NC>
__device__ __forceinline__ double boo_norm2(const double (&q)[NC])
{
    double s = 0.0;
#pragma unroll
    for (int m = NC / 2 - 1; m >= 1; --m) s += __builtin_fma(q[2 * m], q[2 * m], q[2 * m + 1] * q[2 * m + 1]);
    return __builtin_fma(2.0, s, __builtin_fma(q[0], q[0], q[1] * q[1]));
}

// ------------------------------------------------------------------------------------------
// Pass 1: q_lm, its norm and n_i per slot.  qlm[c * cap + slot], c = 2 m (+ 1 for the imaginary part).
// ------------------------------------------------------------------------------------------
struct BooQlmArgs {
    int korder, cap;
    BooCoef bc;
    double *qlm, *norm;
    int32_t *nnb;
};

template <int D, int L>
struct BooQlmLane {
    using Args = BooQlmArgs;
    static constexpr int NC = BooShape<D, L>::NC;
    double a[NC];
    int nn;
    __device__ __forceinline__ void begin(const Args &, const DevState &, int, int, bool, const double4 &)
    {
#pragma unroll
        for (int c = 0; c < NC; ++c) a[c] = 0.0;
        nn = 0;
    }
    __device__ __forceinline__ void visit(const Args &A, const DevState &, bool hit, double dx, double dy, double dz,
                                          double d2, uint32_t)
    {
        boo_add<D, L>(a, hit, dx, dy, dz, d2, A.korder);
        nn += hit ? 1 : 0;
    }
    __device__ __forceinline__ void end(const Args &A, int k, bool active, int)
    {
        if (!active) return;
        const double inv = nn > 0 ? 1.0 / (double)nn : 0.0;
        double q[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            q[c] = (A.bc.coef[c >> 1] * a[c]) * inv;
            A.qlm[(size_t)c * A.cap + k] = q[c];
        }
        A.norm[k] = sqrt(boo_norm2<NC>(q));
        A.nnb[k] = nn;
    }
};

// ------------------------------------------------------------------------------------------
// Pass 2: Q_lm, s_ij, q, qbar and c per slot; the histograms; the block partials
//   partials[c * nblk + bid], c = 0..5: sum q, q^2, qbar, qbar^2, n, c;  6: solid particles;  7 + c: sum n_i q_lm component c
// hist: [nbins q][nbins qbar][33 n_i][33 c_i]
// ------------------------------------------------------------------------------------------
struct BooAvgArgs {
    double threshold;
    int min_conn, nbins, cap, nblk;
    BooCoef bc;
    const double *qlm, *norm;
    const int32_t *nnb;
    double *q, *qbar;
    int32_t *nconn;
    unsigned long long *hist;
    double *partials;
};

template <int D, int L>
struct BooAvgLane {
    using Args = BooAvgArgs;
    static constexpr int NC = BooShape<D, L>::NC;
    double qi[NC], Q[NC];
    double ni_norm;
    int conn;
    __device__ __forceinline__ void begin(const Args &A, const DevState &, int, int kk, bool, const double4 &)
    {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            qi[c] = A.qlm[(size_t)c * A.cap + kk];
            Q[c] = 0.0;
        }
        ni_norm = A.norm[kk];
        conn = 0;
    }
    __device__ __forceinline__ void visit(const Args &A, const DevState &, bool hit, double, double, double, double,
                                          uint32_t own)
    {
        if (!hit) return;
        double qj[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) qj[c] = A.qlm[(size_t)c * A.cap + own];
        const double nj = A.norm[own];
#pragma unroll
        for (int c = 0; c < NC; ++c) Q[c] += qj[c];
        // Re sum_m q_m(i) conj(q_m(j)), the m > 0 half doubled
        double t = 0.0;
#pragma unroll
        for (int m = NC / 2 - 1; m >= 1; --m) t += __builtin_fma(qi[2 * m], qj[2 * m], qi[2 * m + 1] * qj[2 * m + 1]);
        const double dot = __builtin_fma(2.0, t, __builtin_fma(qi[0], qj[0], qi[1] * qj[1]));
        const double den = ni_norm * nj;
        const double sij = den > 0.0 ? dot / den : 0.0;
        conn += sij > A.threshold ? 1 : 0;
    }
    __device__ __forceinline__ void end(const Args &A, int k, bool active, int bid)
    {
        __shared__ double red[16];
        __shared__ unsigned hl[2 * MD_BOO_LDS_BINS + 2 * (MD_BOO_NCLAMP + 1)];
        const bool lds_hist = A.nbins <= MD_BOO_LDS_BINS;
        const int nh = (lds_hist ? 2 * A.nbins : 0) + 2 * (MD_BOO_NCLAMP + 1);
        for (int i = threadIdx.x; i < nh; i += blockDim.x) hl[i] = 0u;
        __syncthreads();
        unsigned *hl_small = hl + (lds_hist ? 2 * A.nbins : 0);
        double v[BooShape<D, L>::NPART];
#pragma unroll
        for (int c = 0; c < BooShape<D, L>::NPART; ++c) v[c] = 0.0;
        if (active) {
            const int nn = A.nnb[k];
            const double invn1 = 1.0 / (double)(nn + 1);
            double Qa[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) Qa[c] = (qi[c] + Q[c]) * invn1;
            const double q = sqrt(A.bc.pref * boo_norm2<NC>(qi));
            const double qb = sqrt(A.bc.pref * boo_norm2<NC>(Qa));
            A.q[k] = q;
            A.qbar[k] = qb;
            A.nconn[k] = conn;
            const bool solid = conn >= A.min_conn;
            v[0] = q;
            v[1] = q * q;
            v[2] = qb;
            v[3] = qb * qb;
            v[4] = (double)nn;
            v[5] = (double)conn;
            v[6] = solid ? 1.0 : 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) v[7 + c] = (double)nn * qi[c];
            int bq = (int)(q * (double)A.nbins);
            int bb = (int)(qb * (double)A.nbins);
            bq = bq < 0 ? 0 : (bq > A.nbins - 1 ? A.nbins - 1 : bq);
            bb = bb < 0 ? 0 : (bb > A.nbins - 1 ? A.nbins - 1 : bb);
            if (lds_hist) {
                atomicAdd(&hl[bq], 1u);
                atomicAdd(&hl[A.nbins + bb], 1u);
            } else {
                atomicAdd(&A.hist[bq], 1ull);
                atomicAdd(&A.hist[A.nbins + bb], 1ull);
            }
            atomicAdd(&hl_small[nn > MD_BOO_NCLAMP ? MD_BOO_NCLAMP : nn], 1u);
            atomicAdd(&hl_small[(MD_BOO_NCLAMP + 1) + (conn > MD_BOO_NCLAMP ? MD_BOO_NCLAMP : conn)], 1u);
        }
        __syncthreads();
        // (the LDS bins follow the global layout: q, qbar when gathered here, then n_i, c_i)
        const int goff = lds_hist ? 0 : 2 * A.nbins;
        for (int i = threadIdx.x; i < nh; i += blockDim.x) {
            unsigned cnt = hl[i];
            if (cnt) atomicAdd(&A.hist[goff + i], (unsigned long long)cnt);
        }
#pragma unroll
        for (int c = 0; c < BooShape<D, L>::NPART; ++c) {
            double t = block_sum(v[c], red);
            if (threadIdx.x == 0) A.partials[(size_t)c * A.nblk + bid] = t;
        }
    }
};

// ------------------------------------------------------------------------------------------
// One block: the frame vector fr (k_stress_finish's tree over the partials, in block order)
//   fr[0..5] = sum q, q^2, qbar, qbar^2, n, c;  fr[6] = solid particles;
//   fr[7] = sqrt(pref (|G_0|^2 + 2 sum_{m>0} |G_m|^2)),  G_m = sum_i n_i q_lm(i) / sum_i n_i  (0 when nobody has a neighbour)
// sum_fr += fr, series[m] = fr when m < nseries; m = samples since setup / reset, counted by the host.
// ------------------------------------------------------------------------------------------
template <int D, int L>
__global__ void __launch_bounds__(1024)
    k_boo_finish(int nblk, const double *__restrict__ partials, BooCoef bc, long long m, long long nseries,
                 double *__restrict__ sum_fr, double *__restrict__ series)
{
    constexpr int NC = BooShape<D, L>::NC;
    constexpr int NP = BooShape<D, L>::NPART;
    __shared__ double red[16];
    double t[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        double a = strided_sum<4>(partials + (size_t)c * nblk, nblk);
        t[c] = block_sum(a, red);
    }
    if (threadIdx.x != 0) return;
    double fr[MD_BOO_NFR];
#pragma unroll
    for (int c = 0; c < 7; ++c) fr[c] = t[c];
    double G[NC];
    const double invn = t[4] > 0.0 ? 1.0 / t[4] : 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) G[c] = t[7 + c] * invn;
    fr[7] = sqrt(bc.pref * boo_norm2<NC>(G));
#pragma unroll
    for (int c = 0; c < MD_BOO_NFR; ++c) {
        sum_fr[c] = sum_fr[c] + fr[c];
        if (m < nseries) series[(size_t)m * MD_BOO_NFR + c] = fr[c];
    }
}

// ------------------------------------------------------------------------------------------
// Slot order -> particle-id order (k_export's permutation) for md_boo_particles and md_boo_qlm; any output may be null.
// `id` is the sampler's copy of the permutation taken with the sample: the handle's own changes at every list build.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MD_BLOCK)
    k_boo_export(int n, const int32_t *__restrict__ id, int cap, int nm, const int32_t *__restrict__ nnb,
                 const double *__restrict__ q, const double *__restrict__ qbar, const int32_t *__restrict__ nconn,
                 const double *__restrict__ qlm, int32_t *__restrict__ o_nnb, double *__restrict__ o_q,
                 double *__restrict__ o_qbar, int32_t *__restrict__ o_nconn, double *__restrict__ o_qlm)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    size_t o = (size_t)id[k];
    if (o_nnb) o_nnb[o] = nnb[k];
    if (o_q) o_q[o] = q[k];
    if (o_qbar) o_qbar[o] = qbar[k];
    if (o_nconn) o_nconn[o] = nconn[k];
    if (o_qlm)
        for (int c = 0; c < 2 * nm; ++c) o_qlm[o * 2 * nm + c] = qlm[(size_t)c * cap + k];
}
