// md_chi4.hpp -- four-point dynamics sampled on the device (md_chi4_* in include/mdhip.h): the self overlap
// Q(t0, t) = sum_i w_i, w_i = 1 iff particle i moved less than a between the stored origin frame and the current frame,
// its first two moments behind chi4(t) = (<Q^2> - <Q>^2) / N, and the structure factor of the slow particles
// S4(q, t) = <|W(q)|^2> / N, W(q) = sum_i w_i exp(+i q.x_i(t0)), on wave vectors commensurate with the cell.
//
// An origin is md_dyn_origin's frame (wrapped x and image counts by particle id, written by k_export) and, with vectors,
// k_sq_frac's f of that frame.  One md_chi4_sample call = one k_export of the current frame, then per (slot, row) three
// launches on the handle's stream, no host wait:
//   k_chi4_overlap  over particle ids (both frames read coalesced, MD_CHI4_PPT ids per thread): the displacement and d2 of
//                   md_dyn.hpp, w = d2 < a2; the wave's 64 consecutive ids packed by __ballot into one 64-bit word of the
//                   mask (bits past N are 0), written by one lane; Q counted by popcount per wave and one 64-bit integer
//                   atomic per block
//   k_chi4_modes    (md_sq.hpp: mode_walk with MASKED) k_sq_rho's walk over the ORIGIN's f under the mask: one mask word
//                   per wave and iteration, loaded wave-uniformly; a zero word skips the iteration's whole tile of terms
//   k_chi4_reduce   one wave per vector: the block partials in k_sq_reduce's tree (md_sq.hpp: sq_row_sum) -> W; lane 0
//                   adds |W|^2 to the row and stores W; one thread adds Q, Q Q and 1 into the row, keeps Q for
//                   md_chi4_last and zeroes the counter
//
// Exactness contract: del and d2 are section 11's (dyn_disp, d2_ref, no fma), w_i = d2 < a2 with
// a2 = a a formed once on the host; Q and its moments are integers; W is section 12's sum (phase, sq_cossin, the tree
// fixed by N alone) over the slow particles, a fast particle adding nothing; no floating-point atomics, so Q, the mask, W
// and the row are functions of the two frames and the call order only.
#pragma once
#include "md_dyn.hpp"
#include "md_sq.hpp"

#define MD_CHI4_BLOCK 256
#define MD_CHI4_PPT 4             // particle ids per thread of k_chi4_overlap: one block covers 1024 ids = 16 mask words
#define MD_CHI4_MAX_VEC 4096
#define MD_CHI4_MAX_SLOTS 64
#define MD_CHI4_NROW 3            // integers per row: sum Q, sum Q^2, samples

// mask[k] bit l = w of particle id 64 k + l; nwords = ceil(n / 64) words are written, every one of them.  qcur is zero at
// entry (k_chi4_reduce leaves it so).
template <int D>
__global__ void __launch_bounds__(MD_CHI4_BLOCK)
    k_chi4_overlap(DynParams P, double a2, const double *__restrict__ xc, const int32_t *__restrict__ nc,
                   const double *__restrict__ xo, const int32_t *__restrict__ no,
                   unsigned long long *__restrict__ mask, unsigned long long *__restrict__ qcur)
{
#pragma clang fp contract(off)
    __shared__ unsigned int wcnt[MD_CHI4_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = blockIdx.x * (MD_CHI4_BLOCK * MD_CHI4_PPT) + threadIdx.x;
    unsigned int cnt = 0; // (wave-uniform)
#pragma unroll
    for (int m = 0; m < MD_CHI4_PPT; ++m) {
        const int i = base + m * MD_CHI4_BLOCK; // the wave's ids: 64 consecutive ones from a multiple of 64
        bool slow = false;
        if (i < P.n) {
            double del[3] = {0.0, 0.0, 0.0};
            dyn_disp<D>(P, xc, nc, xo, no, i, del);
            slow = d2_ref<D>(del[0], del[1], del[2]) < a2;
        }
        const unsigned long long word = __ballot(slow);
        cnt += (unsigned int)__popcll(word);
        if (lane == 0 && i < P.n) mask[i >> 6] = word;
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int s = wcnt[0];
#pragma unroll
        for (int w = 1; w < MD_CHI4_BLOCK / 64; ++w) s += wcnt[w];
        if (s) atomicAdd(qcur, (unsigned long long)s);
    }
}

// One wave per vector (none when nvec == 0: one block still runs for the integers).  part[(v * 2 + comp) * nblk + block]
// as k_chi4_modes (mode_walk) wrote it; wlast[2 v], wlast[2 v + 1] = W(v) of this sample; s4row = the row's nvec sums of
// |W|^2; irow = the row's MD_CHI4_NROW integers.
__global__ void __launch_bounds__(MD_SQ_REDUCE_BLOCK)
    k_chi4_reduce(int nvec, int nblk, const double *__restrict__ part, double *__restrict__ wlast,
                  double *__restrict__ s4row, unsigned long long *__restrict__ qcur, long long *__restrict__ qlast,
                  long long *__restrict__ irow)
{
#pragma clang fp contract(off)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long q = (long long)*qcur;
        irow[0] += q;
        irow[1] += q * q;
        irow[2] += 1;
        *qlast = q;
        *qcur = 0ull;
    }
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * (MD_SQ_REDUCE_BLOCK / 64) + (threadIdx.x >> 6);
    if (v >= nvec) return; // (the whole wave)
    double a, b;
    sq_row_sum(part + (size_t)v * 2 * nblk, nblk, lane, a, b);
    if (lane != 0) return;
    wlast[2 * v] = a;
    wlast[2 * v + 1] = b;
    s4row[v] = s4row[v] + (a * a + b * b);
}
