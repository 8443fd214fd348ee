// md_boo.hpp -- bond-orientational order, sampled on the device (md_boo_* in include/mdhip.h): Steinhardt q_l (l = 4, 6)
// and its neighbour-averaged form in 3-D, the k-fold psi_k in 2-D, ten Wolde's solid-bond count.
//
// One sample = three launches on the handle's stream, no host wait:
//   k_boo_qlm_tile / k_boo_qlm   pass 1: one lane per particle walks its OUTER row (k_stress_tile's walk), accumulates
//                                sum_j Y_lm(u_ij) for m = 0..l and n_i, writes q_lm, its 2-norm and n_i per slot
//   k_boo_avg_tile / k_boo_avg   pass 2: the same walk and the same acceptance test; every hit gathers the neighbour's
//                                q_lm by OWNER slot (orientations are translation invariant: a ghost's q_lm is its
//                                owner's), accumulates Q_lm and the bond coherence s_ij; q, qbar, c per slot, the
//                                histograms, per-block partials
//   k_boo_finish                 one block: the partials in block order, the frame vector, the running sums, the series
//
// Arithmetic contract: del = x_j(+translation) - x_i as the force kernels form it, j is a neighbour
// iff d2_ref(del) < rn2, everything fp64.  Y_lm(u) = c_lm D_l^m(u_z) (u_x + i u_y)^m with D_l^m = d^m P_l / dz^m a
// polynomial and c_lm = (-1)^m sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!): no atan2, acos or sincos.  The lane sums the
// unnormalised D_l^m (u_x + i u_y)^m in row order and applies c_lm / n_i once.  Reductions: block_sum, then one block over
// the partials in block order -- no floating-point atomics; the histograms are integer atomics.
#pragma once
#include "md_kernels.hpp"

#define MD_BOO_MAX_BINS 8192
#define MD_BOO_MAX_SERIES (1 << 20)
#define MD_BOO_NCLAMP 32   // n_i and c_i are histogrammed in 0..32, the last bin holding everything above
#define MD_BOO_LDS_BINS 1024 // up to this many bins the q / qbar histograms are gathered per block in LDS first
#define MD_BOO_NFR 8
// The rows address the force kernel's LDS image with 16-bit byte offsets: the list builders accept a tile only if
// (H + 1) * stride <= MD_BOO_ROW_OFFSET_MAX, stride 24 or 32 (md_boo_sample checks exactly that on the handle).  The
// sampler's own image, 32 bytes per record, then stays below the dynamic LDS the force kernel itself may use.
#define MD_BOO_ROW_OFFSET_MAX 65535
#define MD_BOO_LDS_LIMIT (150 * 1024)
static_assert((MD_BOO_ROW_OFFSET_MAX / 24) * 32 + 16 <= MD_BOO_LDS_LIMIT && (MD_BOO_ROW_OFFSET_MAX / 32) * 32 + 16 <= MD_BOO_LDS_LIMIT,
              "the sampler's 32-byte image of any tile the builders accept must fit the force kernel's LDS limit");

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
// The two walks.  f(hit, dx, dy, dz, d2, owner) is called once per row entry, in row order.
// ------------------------------------------------------------------------------------------

// Stage the tile's halo (k_stress_tile's prologue) as 32-byte records {x, y, z, owner slot}: the owner is the halo word's
// low 26 bits, resolved through gowner for a handle whose ghosts are real slots.  Record H is the sentinel.
template <int D>
__device__ __forceinline__ void boo_stage(unsigned char *smem, int n, const DevState &s, const uint32_t *__restrict__ hl,
                                          int H, const int32_t *__restrict__ gowner)
{
    const double4 *__restrict__ P = s.pos;
    for (int h0 = 0; h0 <= H; h0 += 4 * MD_TILE) {
        uint32_t idx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int h = h0 + i * MD_TILE + threadIdx.x;
            idx[i] = (h < H) ? hl[h] : 0xffffffffu;
        }
        double4 pr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            pr[i] = (idx[i] != 0xffffffffu) ? P[idx[i] & 0x3ffffffu]
                                            : make_double4(MD_SENTINEL_POS, MD_SENTINEL_POS, MD_SENTINEL_POS, 1.0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t code = (idx[i] != 0xffffffffu) ? (idx[i] >> 26) : 0u;
            if (code) shift_xyz(pr[i].x, pr[i].y, pr[i].z, code, s.boxL, s.tric, s.cellA);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int h = h0 + i * MD_TILE + threadIdx.x;
            if (h <= H) {
                uint32_t own = 0u;
                if (idx[i] != 0xffffffffu) {
                    own = idx[i] & 0x3ffffffu;
                    if (own >= (uint32_t)n) own = (uint32_t)gowner[own - (uint32_t)n];
                }
                double *rec = (double *)(smem + (size_t)h * 32);
                rec[0] = pr[i].x;
                rec[1] = pr[i].y;
                rec[2] = (D == 3) ? pr[i].z : 0.0;
                ((uint32_t *)rec)[6] = own;
                ((uint32_t *)rec)[7] = 0u;
            }
        }
    }
    __syncthreads();
}

// The row of one lane: 16-bit byte offsets into the FORCE kernel's image (record stride RS); record index = offset / RS.
template <int D, int RS, class F>
__device__ __forceinline__ void boo_walk_tile(const unsigned char *smem, const ushort4 *row4, int m, const double4 &pi,
                                              double rn2, F &&f)
{
    ushort4 jn = row4[0]; // (m >= 4 or the loop below does not run; entry 0 exists in every allocated row)
    for (int r = 0; r < m; r += 4) {
        const unsigned o[4] = {jn.x, jn.y, jn.z, jn.w};
        const int rg = r + 4;
        jn = row4[(size_t)(((rg < m) ? rg : 0) >> 2) * 64];
        double xj[4], yj[4], zj[4];
        uint32_t own[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned rec = (RS == 32) ? o[q] : (o[q] / (unsigned)RS) * 32u;
            const double *p = (const double *)(smem + rec);
            xj[q] = p[0];
            yj[q] = p[1];
            zj[q] = p[2];
            own[q] = ((const uint32_t *)p)[6];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double dx = xj[q] - pi.x;
            double dy = yj[q] - pi.y;
            double dz = 0.0;
            if constexpr (D == 3) dz = zj[q] - pi.z;
            double d2 = d2_ref<D>(dx, dy, dz);
            f(d2 < rn2, dx, dy, dz, d2, own[q]);
        }
    }
}

// The row of one lane of a handle whose rows are 32-bit global slots (k_stress's walk); the sentinel slot is `cap`.
template <int D, class F>
__device__ __forceinline__ void boo_walk_global(int n, const DevState &s, const uint32_t *row, int m, const double4 &pi,
                                                double rn2, const int32_t *__restrict__ gowner, F &&f)
{
    const double4 *__restrict__ P = s.pos;
    for (int r = 0; r < m; r += 4) {
        uint32_t j[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) j[q] = row[(size_t)(r + q) * 64];
        double4 pj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pj[q] = P[j[q]];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double dx = pj[q].x - pi.x;
            double dy = pj[q].y - pi.y;
            double dz = 0.0;
            if constexpr (D == 3) dz = pj[q].z - pi.z;
            double d2 = d2_ref<D>(dx, dy, dz);
            bool hit = d2 < rn2;
            uint32_t own = j[q];
            if (hit && own >= (uint32_t)n) own = (uint32_t)gowner[own - (uint32_t)n]; // (a hit is never the sentinel)
            f(hit, dx, dy, dz, d2, own);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Pass 1: q_lm, its norm and n_i per slot.  qlm[c * cap + slot], c = 2 m (+ 1 for the imaginary part).
// ------------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void boo_qlm_store(int k, bool active, int cap, const double (&a)[NC], int nn,
                                              const BooCoef &bc, double *__restrict__ qlm, double *__restrict__ norm,
                                              int32_t *__restrict__ nnb)
{
    if (!active) return;
    const double inv = nn > 0 ? 1.0 / (double)nn : 0.0;
    double q[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        q[c] = (bc.coef[c >> 1] * a[c]) * inv;
        qlm[(size_t)c * cap + k] = q[c];
    }
    norm[k] = sqrt(boo_norm2<NC>(q));
    nnb[k] = nn;
}

template <int D, int L, int RS>
__global__ void __launch_bounds__(MD_TILE)
    k_boo_qlm_tile(int n, DevState s, double rn2, int korder, BooCoef bc, const uint16_t *__restrict__ nlist16, int maxn,
                   const int32_t *__restrict__ nmax_tile, const uint32_t *__restrict__ halo, int hcap,
                   const int32_t *__restrict__ halo_count, const int32_t *__restrict__ gowner, int cap,
                   double *__restrict__ qlm, double *__restrict__ norm, int32_t *__restrict__ nnb)
{
    constexpr int NC = BooShape<D, L>::NC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int k = bid * MD_TILE + threadIdx.x;
    bool active = k < n;
    int kk = active ? k : n - 1;
    int lane = threadIdx.x & 63;
    int wt = bid * (MD_TILE / 64) + (threadIdx.x >> 6);
    const ushort4 *row4 = (const ushort4 *)(nlist16 + ((size_t)wt * maxn) * 64) + lane;
    const int m = __builtin_amdgcn_readfirstlane(nmax_tile[wt]);
    double4 pi = s.pos[kk];
    boo_stage<D>(smem, n, s, halo + (size_t)bid * hcap, halo_count[bid], gowner);
    double a[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = 0.0;
    int nn = 0;
    boo_walk_tile<D, RS>(smem, row4, m, pi, rn2, [&](bool hit, double dx, double dy, double dz, double d2, uint32_t) {
        boo_add<D, L>(a, hit, dx, dy, dz, d2, korder);
        nn += hit ? 1 : 0;
    });
    boo_qlm_store(k, active, cap, a, nn, bc, qlm, norm, nnb);
}

template <int D, int L>
__global__ void __launch_bounds__(MD_BLOCK)
    k_boo_qlm(int n, DevState s, double rn2, int korder, BooCoef bc, const uint32_t *__restrict__ nlist, int maxn,
              const int32_t *__restrict__ nmax_tile, const int32_t *__restrict__ gowner, int cap, double *__restrict__ qlm,
              double *__restrict__ norm, int32_t *__restrict__ nnb)
{
    constexpr int NC = BooShape<D, L>::NC;
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int k = bid * MD_BLOCK + threadIdx.x;
    bool active = k < n;
    int kk = active ? k : n - 1;
    int lane = threadIdx.x & 63;
    int tile = kk >> 6;
    const uint32_t *row = nlist + ((size_t)tile * maxn) * 64 + lane;
    int m = nmax_tile[tile];
    double4 pi = s.pos[kk];
    double a[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = 0.0;
    int nn = 0;
    boo_walk_global<D>(n, s, row, m, pi, rn2, gowner, [&](bool hit, double dx, double dy, double dz, double d2, uint32_t) {
        boo_add<D, L>(a, hit, dx, dy, dz, d2, korder);
        nn += hit ? 1 : 0;
    });
    boo_qlm_store(k, active, cap, a, nn, bc, qlm, norm, nnb);
}

// ------------------------------------------------------------------------------------------
// Pass 2: Q_lm, s_ij, q, qbar and c per slot; the histograms; the block partials
//   partials[c * nblk + bid], c = 0..5: sum q, q^2, qbar, qbar^2, n, c;  6: solid particles;  7 + c: sum n_i q_lm component c
// hist: [nbins q][nbins qbar][33 n_i][33 c_i]
// ------------------------------------------------------------------------------------------
struct BooAvgArgs {
    double threshold;
    int min_conn, nbins, cap, nblk;
    const double *qlm, *norm;
    const int32_t *nnb;
    double *q, *qbar;
    int32_t *nconn;
    unsigned long long *hist;
    double *partials;
};

template <int D, int L>
struct BooAvgLane {
    static constexpr int NC = BooShape<D, L>::NC;
    double qi[NC], Q[NC];
    double ni_norm;
    int conn;
    __device__ __forceinline__ void init(int kk, const BooAvgArgs &A)
    {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            qi[c] = A.qlm[(size_t)c * A.cap + kk];
            Q[c] = 0.0;
        }
        ni_norm = A.norm[kk];
        conn = 0;
    }
    __device__ __forceinline__ void hit(uint32_t own, const BooAvgArgs &A)
    {
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
};

template <int D, int L>
__device__ __forceinline__ void boo_avg_epilogue(int k, bool active, BooAvgLane<D, L> &ln, const BooAvgArgs &A,
                                                 const BooCoef &bc, int bid, double *red, unsigned *hl)
{
    constexpr int NC = BooShape<D, L>::NC;
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
        for (int c = 0; c < NC; ++c) Qa[c] = (ln.qi[c] + ln.Q[c]) * invn1;
        const double q = sqrt(bc.pref * boo_norm2<NC>(ln.qi));
        const double qb = sqrt(bc.pref * boo_norm2<NC>(Qa));
        A.q[k] = q;
        A.qbar[k] = qb;
        A.nconn[k] = ln.conn;
        const bool solid = ln.conn >= A.min_conn;
        v[0] = q;
        v[1] = q * q;
        v[2] = qb;
        v[3] = qb * qb;
        v[4] = (double)nn;
        v[5] = (double)ln.conn;
        v[6] = solid ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) v[7 + c] = (double)nn * ln.qi[c];
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
        atomicAdd(&hl_small[(MD_BOO_NCLAMP + 1) + (ln.conn > MD_BOO_NCLAMP ? MD_BOO_NCLAMP : ln.conn)], 1u);
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

template <int D, int L, int RS>
__global__ void __launch_bounds__(MD_TILE)
    k_boo_avg_tile(int n, DevState s, double rn2, BooCoef bc, const uint16_t *__restrict__ nlist16, int maxn,
                   const int32_t *__restrict__ nmax_tile, const uint32_t *__restrict__ halo, int hcap,
                   const int32_t *__restrict__ halo_count, const int32_t *__restrict__ gowner, BooAvgArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double red[16];
    __shared__ unsigned hl[2 * MD_BOO_LDS_BINS + 2 * (MD_BOO_NCLAMP + 1)];
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int k = bid * MD_TILE + threadIdx.x;
    bool active = k < n;
    int kk = active ? k : n - 1;
    int lane = threadIdx.x & 63;
    int wt = bid * (MD_TILE / 64) + (threadIdx.x >> 6);
    const ushort4 *row4 = (const ushort4 *)(nlist16 + ((size_t)wt * maxn) * 64) + lane;
    const int m = __builtin_amdgcn_readfirstlane(nmax_tile[wt]);
    double4 pi = s.pos[kk];
    boo_stage<D>(smem, n, s, halo + (size_t)bid * hcap, halo_count[bid], gowner);
    BooAvgLane<D, L> ln;
    ln.init(kk, A);
    boo_walk_tile<D, RS>(smem, row4, m, pi, rn2, [&](bool hit, double, double, double, double, uint32_t own) {
        if (hit) ln.hit(own, A);
    });
    boo_avg_epilogue<D, L>(k, active, ln, A, bc, bid, red, hl);
}

template <int D, int L>
__global__ void __launch_bounds__(MD_BLOCK)
    k_boo_avg(int n, DevState s, double rn2, BooCoef bc, const uint32_t *__restrict__ nlist, int maxn,
              const int32_t *__restrict__ nmax_tile, const int32_t *__restrict__ gowner, BooAvgArgs A)
{
    __shared__ double red[16];
    __shared__ unsigned hl[2 * MD_BOO_LDS_BINS + 2 * (MD_BOO_NCLAMP + 1)];
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int k = bid * MD_BLOCK + threadIdx.x;
    bool active = k < n;
    int kk = active ? k : n - 1;
    int lane = threadIdx.x & 63;
    int tile = kk >> 6;
    const uint32_t *row = nlist + ((size_t)tile * maxn) * 64 + lane;
    int m = nmax_tile[tile];
    double4 pi = s.pos[kk];
    BooAvgLane<D, L> ln;
    ln.init(kk, A);
    boo_walk_global<D>(n, s, row, m, pi, rn2, gowner, [&](bool hit, double, double, double, double, uint32_t own) {
        if (hit) ln.hit(own, A);
    });
    boo_avg_epilogue<D, L>(k, active, ln, A, bc, bid, red, hl);
}

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
