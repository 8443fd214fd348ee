// md_dyn.hpp -- self dynamics sampled on the device (md_dyn_* in include/mdhip.h): mean-squared displacement, the
// non-Gaussian parameter's fourth moment, the self-intermediate scattering function F_s(q, t) and the self part of the van
// Hove function, between a stored origin frame and the current frame.
//
// A frame is what md_download returns: the wrapped x and the image counts n, in particle-id order, written by the step
// loop's own k_export into buffers the sampler owns.  One md_dyn_sample call = one k_export of the current frame, then per
// batch of up to MD_DYN_MAX_BATCH samples two launches on the handle's stream, no host wait:
//   k_dyn_sample  over particle ids (both frames read coalesced): the displacement, d2, d2*d2 and the nq cosine sums of
//                 every particle; fp64 block partials in a fixed tree; the van Hove bin of d2 counted in LDS (uint32) and
//                 flushed with one 64-bit integer atomic per nonzero bin
//   k_dyn_reduce  one block: every sample's partials summed in block order, the totals added into the sample's row
//
// Exactness contract: dn_c = (double)n_c(t) - (double)n_c(t0) (exact),
// del_c = (x_c(t) - x_c(t0)) + ((U_c0 dn_0 + U_c1 dn_1) + U_c2 dn_2) (2-D: no third term),
// d2 = (del_0 del_0 + del_1 del_1) + del_2 del_2, every operation rounded on its own (no fma); s_i(q) = sum over the axes
// c = 0..d-1, in order, of cos(q del_c).  The sums are reduced over particle ids in a tree fixed by N alone (thread:
// MD_DYN_PPT ids in order; wave: shuffle tree; block: waves in order; k_dyn_reduce: lane l sums the blocks l, l + 64, ...
// in order, then a shuffle tree), with no floating-point atomics, so they are a function of the two frames only.
#pragma once
#include "md_kernels.hpp"

#define MD_DYN_BLOCK 256
#define MD_DYN_PPT 4              // particle ids per thread: one block covers MD_DYN_BLOCK * MD_DYN_PPT ids
#define MD_DYN_MAX_SLOTS 64
#define MD_DYN_MAX_Q 16
#define MD_DYN_MAX_BINS 8192
#define MD_DYN_MAX_BATCH 32       // samples per launch pair
#define MD_DYN_REDUCE_BLOCK 1024

struct DynParams {
    int n, dim, nq, nbins, nblk, nquant; // nquant = 2 + nq sums per sample
    float inv_delta;                     // nbins / r_max: the first guess of a bin, corrected against the table
    double U[9];                         // unit cell, row-major, columns = lattice vectors
    double q[MD_DYN_MAX_Q];
};

struct DynBatch {
    int count;
    int slot[MD_DYN_MAX_BATCH];
    int row[MD_DYN_MAX_BATCH];
};

__device__ __forceinline__ double dyn_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v; // (lane 0)
}

// The displacement of particle id i between the frames (xo, no) and (xc, nc): del_c, c < D, as the contract above forms it
template <int D>
__device__ __forceinline__ void dyn_disp(const DynParams &P, const double *__restrict__ xc, const int32_t *__restrict__ nc,
                                         const double *__restrict__ xo, const int32_t *__restrict__ no, int i,
                                         double (&del)[3])
{
#pragma clang fp contract(off)
    const size_t o = (size_t)i * D;
    double dn[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < D; ++c) dn[c] = (double)nc[o + c] - (double)no[o + c];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double t = P.U[c * 3 + 0] * dn[0] + P.U[c * 3 + 1] * dn[1];
        if constexpr (D == 3) t = t + P.U[c * 3 + 2] * dn[2];
        del[c] = (xc[o + c] - xo[o + c]) + t;
    }
}

// The block's last step of the fixed tree: the wave sums of every quantity (written by lane 0 of each wave, a barrier
// since) added in wave order, part[(smp nquant + j) nblk + block] = the block partial of quantity j
__device__ __forceinline__ void dyn_store_part(const DynParams &P, const double (*wsum)[2 + MD_DYN_MAX_Q], int smp,
                                               double *__restrict__ part)
{
#pragma clang fp contract(off)
    if (threadIdx.x < P.nquant) {
        const int j = threadIdx.x;
        double s = wsum[0][j];
#pragma unroll
        for (int w = 1; w < MD_DYN_BLOCK / 64; ++w) s = s + wsum[w][j];
        part[((size_t)smp * P.nquant + j) * P.nblk + blockIdx.x] = s;
    }
}

// One sample per blockIdx.y.
template <int D>
__global__ void __launch_bounds__(MD_DYN_BLOCK)
    k_dyn_sample(DynParams P, DynBatch B, const double *__restrict__ xc, const int32_t *__restrict__ nc,
                 const double *__restrict__ xo_all, const int32_t *__restrict__ no_all, const double *__restrict__ e2,
                 double *__restrict__ part, unsigned long long *__restrict__ hist)
{
#pragma clang fp contract(off)
    extern __shared__ uint32_t dyn_cnt[];                 // nbins
    __shared__ double wsum[MD_DYN_BLOCK / 64][2 + MD_DYN_MAX_Q];
    const int smp = blockIdx.y;
    const size_t frame = (size_t)P.n * D;
    const double *__restrict__ xo = xo_all + (size_t)B.slot[smp] * frame;
    const int32_t *__restrict__ no = no_all + (size_t)B.slot[smp] * frame;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbins = P.nbins;
    if (nbins > 0) {
        for (int b = threadIdx.x; b < nbins; b += MD_DYN_BLOCK) dyn_cnt[b] = 0u;
        __syncthreads();
    }
    const double e2max = nbins > 0 ? e2[nbins] : 0.0;
    double acc[2 + MD_DYN_MAX_Q];
#pragma unroll
    for (int j = 0; j < 2 + MD_DYN_MAX_Q; ++j) acc[j] = 0.0;
    const int base = blockIdx.x * (MD_DYN_BLOCK * MD_DYN_PPT) + threadIdx.x;
#pragma unroll
    for (int m = 0; m < MD_DYN_PPT; ++m) {
        const int i = base + m * MD_DYN_BLOCK;
        const bool act = i < P.n;
        double d2 = 0.0;
        if (act) {
            double del[3] = {0.0, 0.0, 0.0};
            dyn_disp<D>(P, xc, nc, xo, no, i, del);
            d2 = d2_ref<D>(del[0], del[1], del[2]);
            acc[0] += d2;
            acc[1] += d2 * d2;
#pragma unroll
            for (int j = 0; j < MD_DYN_MAX_Q; ++j) {
                if (j < P.nq) {
                    double s = cos(P.q[j] * del[0]);
#pragma unroll
                    for (int c = 1; c < D; ++c) s = s + cos(P.q[j] * del[c]);
                    acc[2 + j] += s;
                }
            }
        }
        if (nbins > 0 && act && d2 < e2max) {
            // the table decides: e2[k] <= d2 < e2[k + 1]; d2 >= e2[nbins] is not counted
            int k = (int)(sqrtf((float)d2) * P.inv_delta);
            k = k < 0 ? 0 : (k > nbins - 1 ? nbins - 1 : k);
            while (k > 0 && d2 < e2[k]) --k;
            while (k < nbins - 1 && d2 >= e2[k + 1]) ++k;
            atomicAdd(&dyn_cnt[k], 1u);
        }
    }
    // fixed tree: shuffle within the wave, then the waves in order
#pragma unroll
    for (int j = 0; j < 2 + MD_DYN_MAX_Q; ++j) {
        if (j < P.nquant) {
            const double w = dyn_wave_sum(acc[j]);
            if (lane == 0) wsum[wave][j] = w;
        }
    }
    __syncthreads();
    dyn_store_part(P, wsum, smp, part);
    if (nbins > 0) {
        unsigned long long *h = hist + (size_t)B.row[smp] * nbins;
        for (int b = threadIdx.x; b < nbins; b += MD_DYN_BLOCK) {
            const uint32_t v = dyn_cnt[b];
            if (v) atomicAdd(&h[b], (unsigned long long)v);
        }
    }
}

// One block: the totals of every sample of the batch (one wave per (sample, quantity) at a time), then one thread per
// quantity adds them into the rows in sample order -- two samples of one batch on one row are added in call order.
__global__ void __launch_bounds__(MD_DYN_REDUCE_BLOCK)
    k_dyn_reduce(DynParams P, DynBatch B, const double *__restrict__ part, double *__restrict__ sums)
{
#pragma clang fp contract(off)
    __shared__ double tot[MD_DYN_MAX_BATCH * (2 + MD_DYN_MAX_Q)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int items = B.count * P.nquant;
    for (int it = wave; it < items; it += MD_DYN_REDUCE_BLOCK / 64) {
        const double *p = part + (size_t)it * P.nblk;
        double s = 0.0;
        for (int b = lane; b < P.nblk; b += 64) s += p[b];
        s = dyn_wave_sum(s);
        if (lane == 0) tot[it] = s;
    }
    __syncthreads();
    if (threadIdx.x < P.nquant) {
        const int j = threadIdx.x;
        for (int i = 0; i < B.count; ++i) {
            double *r = sums + (size_t)B.row[i] * P.nquant + j;
            *r = *r + tot[i * P.nquant + j];
        }
    }
}
