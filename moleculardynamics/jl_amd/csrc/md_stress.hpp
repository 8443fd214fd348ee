// md_stress.hpp -- the pressure tensor and its Green-Kubo correlations, sampled on the device (md_stress_* in
// include/mdhip.h).
//
// One sample = two launches on the handle's stream, no host wait:
//   k_stress_tile  (tiled handles) or k_stress (global-gather handles): per particle, the nc components of
//                  sum_j (f/r) del_a del_b over its OUTER row and of v_a v_b; per-block partials, 2 nc per block
//   k_stress_finish  one block: the partials in block order (k_finalize's tree), the tensor of the frame, the running
//                  sums, the channel vector into the ring and the lag products
//
// Arithmetic contract: del = x_j(+translation) - x_i as the force kernels form it, the pair is
// accepted iff d2_ref(del) < pp.c2 (the reference's d2 <= list_cutoff^2 and the potential's own cutoff inside pair_eval),
// t = fpr del_a (rounded), W_ab = fma(t, del_b, W_ab) per lane in row order, fp64.  Every pair is seen from both ends:
// the total is multiplied by 0.5 (exact).  K_ab = sum v_a v_b, the product rounded, then added.  Reduction: wave
// shuffles, waves in order, blocks in order -- no floating-point atomics.  Nothing of the handle is written.
#pragma once
#include "md_kernels.hpp"

#define MD_STRESS_MAX_LAGS 65536

template <int D>
struct StressAcc {
    static constexpr int NC = (D == 3) ? 6 : 3;
    double w[NC];
};

// components: 3-D xx, yy, zz, xy, xz, yz; 2-D xx, yy, xy
template <int D>
__device__ __forceinline__ void stress_add(StressAcc<D> &a, double fpr, double dx, double dy, double dz)
{
    double tx = fpr * dx;
    double ty = fpr * dy;
    if constexpr (D == 3) {
        double tz = fpr * dz;
        a.w[0] = __builtin_fma(tx, dx, a.w[0]);
        a.w[1] = __builtin_fma(ty, dy, a.w[1]);
        a.w[2] = __builtin_fma(tz, dz, a.w[2]);
        a.w[3] = __builtin_fma(tx, dy, a.w[3]);
        a.w[4] = __builtin_fma(tx, dz, a.w[4]);
        a.w[5] = __builtin_fma(ty, dz, a.w[5]);
    } else {
        a.w[0] = __builtin_fma(tx, dx, a.w[0]);
        a.w[1] = __builtin_fma(ty, dy, a.w[1]);
        a.w[2] = __builtin_fma(tx, dy, a.w[2]);
    }
}

// Epilogue of both walks: the own particle's v_a v_b, then block sums of the 2 nc components.
// partials[c * nblk + bid] = kinetic component c, partials[(nc + c) * nblk + bid] = virial component c (both ends).
template <int D>
__device__ __forceinline__ void stress_epilogue(const DevState &s, int k, bool active, StressAcc<D> &a, int bid, int nblk,
                                                double *__restrict__ partials, double *red)
{
#pragma clang fp contract(off)
    constexpr int NC = StressAcc<D>::NC;
    double kin[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) kin[c] = 0.0;
    if (active) {
        double vx = s.v[0][k], vy = s.v[1][k];
        if constexpr (D == 3) {
            double vz = s.v[2][k];
            kin[0] = vx * vx;
            kin[1] = vy * vy;
            kin[2] = vz * vz;
            kin[3] = vx * vy;
            kin[4] = vx * vz;
            kin[5] = vy * vz;
        } else {
            kin[0] = vx * vx;
            kin[1] = vy * vy;
            kin[2] = vx * vy;
        }
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) a.w[c] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double tk = block_sum(kin[c], red);
        double tw = block_sum(a.w[c], red);
        if (threadIdx.x == 0) {
            partials[(size_t)c * nblk + bid] = tk;
            partials[(size_t)(NC + c) * nblk + bid] = tw;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Global-gather walk (k_force's): handles whose rows are not tiled.
// ------------------------------------------------------------------------------------------
template <int D, int POT, bool UNIFORM>
__global__ void __launch_bounds__(MD_BLOCK)
    k_stress(int n, DevState s, PotParams pp, const uint32_t *__restrict__ nlist, int maxn,
             const int32_t *__restrict__ nmax_tile, double *__restrict__ partials, int nblk)
{
    __shared__ double red[16];
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int k = bid * MD_BLOCK + threadIdx.x;
    bool active = k < n;
    int kk = active ? k : n - 1;
    int lane = threadIdx.x & 63;
    int tile = kk >> 6;
    const uint32_t *row = nlist + ((size_t)tile * maxn) * 64 + lane;
    int m = nmax_tile[tile];
    const double4 *__restrict__ P = s.pos;
    double4 pi = P[kk];
    StressAcc<D> acc;
#pragma unroll
    for (int c = 0; c < StressAcc<D>::NC; ++c) acc.w[c] = 0.0;
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
            bool hit = d2 < pp.c2;
            double d2m = mask_d2(d2, hit);
            double u = 0.0, fpr;
            pair_eval<POT, UNIFORM, false>(d2m, pi.w, pj[q].w, pp, u, fpr);
            stress_add<D>(acc, fpr, dx, dy, dz);
        }
    }
    stress_epilogue<D>(s, k, active, acc, bid, nblk, partials, red);
}

// ------------------------------------------------------------------------------------------
// Tiled walk (k_force_tile's): the tile's halo staged into the LDS image (virtual ghosts resolved by their shift
// codes while staging), one lane per particle over its row of 16-bit record offsets, 8 candidates per block.
// Dynamic LDS: (H+1) * RS bytes, the force kernel's image.
// ------------------------------------------------------------------------------------------
template <int D, int POT, bool UNIFORM, int NQ>
__device__ __forceinline__ void stress_pair_block(const unsigned char *smem, const unsigned (&o)[NQ], const double4 &pi,
                                                  const PotParams &pp, StressAcc<D> &acc)
{
    double xj[NQ], yj[NQ], zj[NQ], wj[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        // (the reads of tile_pair_block: separate ds_read_b64 for 24-byte records, two ds_read_b128 for 32-byte ones)
        typedef const volatile __attribute__((address_space(3))) double lds_cvd;
        if constexpr (!UNIFORM && D == 3) {
            typedef double md_d2 __attribute__((ext_vector_type(2)));
            typedef const __attribute__((address_space(3))) md_d2 lds_d2;
            lds_d2 *r2 = (lds_d2 *)(smem + o[q]);
            md_d2 a = r2[0], b = r2[1];
            xj[q] = a.x;
            yj[q] = a.y;
            zj[q] = b.x;
            wj[q] = b.y;
        } else {
            lds_cvd *rec = (lds_cvd *)(smem + o[q]);
            xj[q] = rec[0];
            yj[q] = rec[1];
            if constexpr (D == 3) zj[q] = rec[2];
            if constexpr (!UNIFORM) wj[q] = rec[3];
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double dx = xj[q] - pi.x;
        double dy = yj[q] - pi.y;
        double dz = 0.0;
        if constexpr (D == 3) dz = zj[q] - pi.z;
        double d2 = d2_ref<D>(dx, dy, dz);
        bool hit = d2 < pp.c2;
        double d2m = mask_d2(d2, hit);
        double u = 0.0, fpr;
        pair_eval<POT, UNIFORM, false>(d2m, pi.w, UNIFORM ? 0.0 : wj[q], pp, u, fpr);
        stress_add<D>(acc, fpr, dx, dy, dz);
    }
}

template <int D, int POT, bool UNIFORM>
__global__ void __launch_bounds__(MD_TILE)
    k_stress_tile(int n, DevState s, PotParams pp, const uint16_t *__restrict__ nlist16, int maxn,
                  const int32_t *__restrict__ nmax_tile, const uint32_t *__restrict__ halo, int hcap,
                  const int32_t *__restrict__ halo_count, double *__restrict__ partials, int nblk)
{
    constexpr int RS = UNIFORM ? 24 : 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double red[16];
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const double4 *__restrict__ P = s.pos;
    int H = halo_count[bid];
    const uint32_t *hl = halo + (size_t)bid * hcap;
    int k = bid * MD_TILE + threadIdx.x;
    bool active = k < n;
    int kk = active ? k : n - 1;
    int lane = threadIdx.x & 63;
    int wt = bid * (MD_TILE / 64) + (threadIdx.x >> 6);
    const ushort4 *row4 = (const ushort4 *)(nlist16 + ((size_t)wt * maxn) * 64) + lane;
    const int m = __builtin_amdgcn_readfirstlane(nmax_tile[wt]);
    double4 pi = P[kk];
    constexpr int G = MD_UNROLL / 4; // index groups per iteration
    static_assert(G == 2, "the tail handling below assumes two groups per iteration");
    ushort4 jn[G];
#pragma unroll
    for (int g = 0; g < G; ++g) jn[g] = row4[(size_t)((4 * g < m) ? g : 0) * 64];
    // stage the halo (k_force_tile's prologue): a halo entry is a slot (26 bits) plus a periodic shift code (6 bits);
    // with virtual ghosts the slot is the ghost's OWNER and x_owner + translation is formed here
    for (int h0 = 0; h0 <= H; h0 += 8 * MD_TILE) {
        uint32_t idx[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int h = h0 + i * MD_TILE + threadIdx.x;
            idx[i] = (h < H) ? hl[h] : 0xffffffffu;
        }
        double4 pr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            pr[i] = (idx[i] != 0xffffffffu) ? P[idx[i] & 0x3ffffffu]
                                            : make_double4(MD_SENTINEL_POS, MD_SENTINEL_POS, MD_SENTINEL_POS, 1.0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t code = (idx[i] != 0xffffffffu) ? (idx[i] >> 26) : 0u;
            if (code) shift_xyz(pr[i].x, pr[i].y, pr[i].z, code, s.boxL, s.tric, s.cellA);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int h = h0 + i * MD_TILE + threadIdx.x;
            if (h <= H) {
                double *rec = (double *)(smem + (size_t)h * RS);
                rec[0] = pr[i].x;
                rec[1] = pr[i].y;
                rec[2] = (D == 3) ? pr[i].z : 0.0;
                if constexpr (!UNIFORM) rec[3] = pr[i].w;
            }
        }
    }
    __syncthreads();
    StressAcc<D> acc;
#pragma unroll
    for (int c = 0; c < StressAcc<D>::NC; ++c) acc.w[c] = 0.0;
    // the row length is the wave's (rows are padded to the wave maximum, a multiple of 4): full iterations take two
    // index groups, a row of 8 k + 4 entries ends with one 4-candidate block (tile_pair_loop's control)
    int r = 0;
    for (; r + MD_UNROLL <= m; r += MD_UNROLL) {
        unsigned o[MD_UNROLL];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            o[4 * g + 0] = jn[g].x;
            o[4 * g + 1] = jn[g].y;
            o[4 * g + 2] = jn[g].z;
            o[4 * g + 3] = jn[g].w;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            int rg = r + MD_UNROLL + 4 * g; // (past the end: any valid group, never used)
            jn[g] = row4[(size_t)(((rg < m) ? rg : 0) >> 2) * 64];
        }
        stress_pair_block<D, POT, UNIFORM, MD_UNROLL>(smem, o, pi, pp, acc);
    }
    if (r < m) {
        unsigned o[4] = {jn[0].x, jn[0].y, jn[0].z, jn[0].w};
        stress_pair_block<D, POT, UNIFORM, 4>(smem, o, pi, pp, acc);
    }
    stress_epilogue<D>(s, k, active, acc, bid, nblk, partials, red);
}

// ------------------------------------------------------------------------------------------
// One block: the frame's tensor, the running sums, the ring and the lag products.
//   last[0..nc)   = kin_c = sum over blocks, in block order (strided_sum + block_sum, k_finalize's tree)
//   last[nc..2nc) = vir_c = 0.5 * that sum
//   sig_c = kin_c + vir_c; the channel vector ch (see include/mdhip.h) goes to ring[m % nlags];
//   corr[k][ch] += ch(m) * ch(m - k) for k = 0 .. min(m, nlags - 1): product rounded, then added (no fma).
// m = the number of samples since setup / reset, counted by the host.  Thread t owns the lags t, t + 1024, ...: a lag's
// accumulator is touched by one thread of one launch at a time, launches in stream order.
// ------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(1024)
    k_stress_finish(int nblk, const double *__restrict__ partials, long long m, int nlags, double *__restrict__ last,
                    double *__restrict__ sums, double *__restrict__ ring, double *__restrict__ corr)
{
#pragma clang fp contract(off)
    constexpr int NC = (D == 3) ? 6 : 3;
    constexpr int NCH = NC;
    __shared__ double red[16];
    double kin[NC], vir[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double a = strided_sum<4>(partials + (size_t)c * nblk, nblk);
        double b = strided_sum<4>(partials + (size_t)(NC + c) * nblk, nblk);
        kin[c] = block_sum(a, red);
        vir[c] = block_sum(b, red) * 0.5; // every pair was evaluated from both ends
    }
    double sg[NC], ch[NCH];
#pragma unroll
    for (int c = 0; c < NC; ++c) sg[c] = kin[c] + vir[c];
    if constexpr (D == 3) {
        ch[0] = sg[3];
        ch[1] = sg[4];
        ch[2] = sg[5];
        ch[3] = (sg[0] - sg[1]) * 0.5;
        ch[4] = (sg[1] - sg[2]) * 0.5;
        ch[5] = ((sg[0] + sg[1]) + sg[2]) / 3.0;
    } else {
        ch[0] = sg[2];
        ch[1] = (sg[0] - sg[1]) * 0.5;
        ch[2] = (sg[0] + sg[1]) / 2.0;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            last[c] = kin[c];
            last[NC + c] = vir[c];
            sums[c] = sums[c] + kin[c];
            sums[NC + c] = sums[NC + c] + vir[c];
        }
    }
    if (nlags <= 0) return;
    const int slot = (int)(m % nlags);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) ring[(size_t)slot * NCH + c] = ch[c];
    }
    const long long kmax = (m < nlags - 1) ? m : nlags - 1;
    for (long long kl = threadIdx.x; kl <= kmax; kl += blockDim.x) {
        double old[NCH];
        if (kl == 0) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) old[c] = ch[c];
        } else {
            const int so = (int)((m - kl) % nlags); // (kl <= nlags - 1: never this launch's slot)
#pragma unroll
            for (int c = 0; c < NCH; ++c) old[c] = ring[(size_t)so * NCH + c];
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            double p = ch[c] * old[c];
            corr[(size_t)kl * NCH + c] = corr[(size_t)kl * NCH + c] + p;
        }
    }
}
