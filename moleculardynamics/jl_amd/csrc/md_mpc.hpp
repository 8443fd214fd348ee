// md_mpc.hpp -- marked pair correlations, sampled on the device (md_mpc_* in include/mdhip.h): the orientational
// correlations g6(r) / G_l(r) of the bond-order sampler's q_lm / psi_k, and the spatial correlation of any per-particle
// field a user uploads (C_vv(r), displacement and mobility correlations).
//
// One sample = md_rdf.hpp's pipeline with a mark carried along, on the handle's stream, no host wait:
//   k_rdf_key      (md_rdf.hpp, as it is) wrapped coordinate + cell key of every particle on the sampler's own grid
//   radix sort     (rocPRIM) of the cell digits
//   k_mpc_inv      MD_MPC_BOO only: the inverse of the bond-order frame's slot -> id permutation
//   k_mpc_gather   sorted records, cell ranges, the marks in sorted order (particle-major), self = sum_i I_ii
//   k_mpc_hist     the pairs over the forward half stencil: per workgroup uint32 counts and int64 sums in LDS, flushed
//                  into the per-sample cur_cnt / cur_sum with one integer atomic per nonzero bin
//   k_mpc_finish   the 2^31 check, acc += cur, last = cur, cur = 0
//
// Exactness contract: the pair's distance, translation and bin are md_rdf.hpp's, operation for
// operation.  p_c = a_c(i) a_c(j) (one product: the same whichever end is home), t = the chain acc = fma(w_c, p_c, acc)
// from acc = 0 over c = 0..NC-1, I = llrint(t 2^31 / tmax) with tmax a power of two (the scaling is exact).  Everything
// accumulated is an integer: the result does not depend on the order the pairs are visited in, the grid or the block
// count.  No floating-point atomics.
//
// A term with |t| > tmax (1 + 2^-10) (or not a number) sets bit 0 of range_error and contributes I = 0; a bin with
// cnt >= 2^31 in one sample sets bit 1.  With neither, |I| <= 2^31 (1 + 2^-10) + 1/2 and cnt < 2^31 give
// |sum| < 2^62 (1 + 2^-9) < 2^63: the int64 sums cannot wrap.
//
// The neighbour's marks reach the wave through a per-wave LDS chunk: the marks of the up to 64 particles of a neighbour
// chunk are copied into it, and every lane that accepts the pair reads the NC marks of neighbour jj at one wave-uniform
// address (a broadcast read: no bank conflict, issued only under the exec mask of the accepting lanes).  The
// alternative -- v_readlane as for the coordinates -- costs 2 NC scalar broadcasts per neighbour whether or not any
// lane accepts it (28 at NC = 14, on top of rdf's 6 to 8) and 2 NC scalar registers in a walk that has none to spare.
// The sorted marks are particle-major, smarks[k * NC + c]: a chunk is then one contiguous run of m NC doubles, copied
// with coalesced loads from a single base address (component-major needs NC base addresses in scalar registers).
#pragma once
#include "md_rdf.hpp"

#define MD_MPC_MAX_BINS 4096
#define MD_MPC_MAX_NC 14
#define MD_MPC_ERR_TERM 1  // a term with |t| > tmax (1 + 2^-10)
#define MD_MPC_ERR_COUNT 2 // a bin with cnt >= 2^31 in one sample

struct MpcWeights {
    double w[MD_MPC_MAX_NC];
    double scale; // 2^31 / tmax
    double lim;   // tmax (1 + 2^-10)
};

// t of a pair (or of a particle with itself) -> the integer it contributes; `bad` is raised for a term out of range
template <int NC>
__device__ __forceinline__ long long mpc_term(const double (&a)[NC], const double (&b)[NC], const double (&w)[NC],
                                              double scale, double lim, bool &bad)
{
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double p = a[c] * b[c];
        acc = __builtin_fma(w[c], p, acc);
    }
    const bool ok = fabs(acc) <= lim; // (false for a NaN)
    bad = bad || !ok;
    return ok ? __double2ll_rn(acc * scale) : 0ll;
}

// MD_MPC_BOO: inv[id] = the slot particle `id` had in the bond-order frame
__global__ void __launch_bounds__(MD_BLOCK) k_mpc_inv(int n, const int32_t *__restrict__ ids, int32_t *__restrict__ inv)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    inv[ids[k]] = k;
}

// After the sort: k_rdf_gather's records and cell ranges; the marks of sorted particle k, smarks[k * NC + c]; self.
// The mark of particle `id`, component c, is src[(inv ? inv[id] : id) * stride_i + c * stride_c]:
//   MD_MPC_USER  inv = null, stride_i = NC, stride_c = 1   (marks[i * NC + c] in particle-id order)
//   MD_MPC_BOO   inv = the frame's inverse permutation, stride_i = 1, stride_c = n   (qlm[c * n + slot])
template <int NC>
__global__ void __launch_bounds__(MD_BLOCK)
    k_mpc_gather(int n, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                 const double4 *__restrict__ wrec, const double *__restrict__ src, const int32_t *__restrict__ inv,
                 size_t stride_i, size_t stride_c, MpcWeights W, double4 *__restrict__ srec,
                 double *__restrict__ smarks, int32_t *__restrict__ cell_start, int32_t *__restrict__ cell_end,
                 long long *__restrict__ cur_self, int32_t *__restrict__ range_error)
{
    __shared__ long long red[MD_BLOCK / 64];
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    long long I = 0;
    bool bad = false;
    if (k < n) {
        uint32_t key = keys[k];
        const double4 rec = wrec[vals[k]];
        srec[k] = rec;
        if (k == 0 || keys[k - 1] != key) {
            cell_start[key] = k;
            if (k > 0) cell_end[keys[k - 1]] = k;
        }
        if (k == n - 1) cell_end[key] = n;
        const int id = (int)rec.w;
        const size_t p = (size_t)(inv ? inv[id] : id) * stride_i;
        double a[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            a[c] = src[p + (size_t)c * stride_c];
            smarks[(size_t)k * NC + c] = a[c];
        }
        double w[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) w[c] = W.w[c];
        I = mpc_term<NC>(a, a, w, W.scale, W.lim, bad);
    }
    // integers: the order of the reduction does not matter
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) I += __shfl_xor(I, off);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = I;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
        if (t) atomicAdd((unsigned long long *)cur_self, (unsigned long long)t);
    }
    if (__any(bad) && lane == 0) atomicOr(range_error, MD_MPC_ERR_TERM);
}

// The histogram: k_rdf_hist's walk (a work counter over home cells, 64 home particles per wave, the forward half
// stencil, the coordinates by v_readlane) with the home marks in registers and the neighbour chunk's marks in the
// wave's LDS chunk.  LDS: [waves x 64 x NC marks][16: the weights, scale, lim][e2: nbins + 1][sum: nbins int64]
// [cnt: nbins uint32].  The weights pass through LDS so that they live in vector registers: the walk already uses
// every scalar register (k_rdf_hist: 102), and 2 NC + 4 more would spill.
template <int D, int NC>
__global__ void __launch_bounds__(MD_RDF_BLOCK)
    k_mpc_hist(RdfGrid rg, int nbins, float inv_delta, MpcWeights W, const double *__restrict__ e2g,
               const double4 *__restrict__ srec, const double *__restrict__ smarks,
               const int32_t *__restrict__ cell_start, const int32_t *__restrict__ cell_end, int32_t *__restrict__ work,
               unsigned long long *__restrict__ cur_cnt, unsigned long long *__restrict__ cur_sum,
               int32_t *__restrict__ range_error)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double mpc_lds[];
    constexpr int WAVES = MD_RDF_BLOCK / 64;
    double *chunk = mpc_lds + (size_t)(threadIdx.x >> 6) * 64 * NC;              // this wave's 64 x NC marks
    double *wl = mpc_lds + (size_t)WAVES * 64 * NC;                              // MD_MPC_MAX_NC + 2
    double *e2 = wl + MD_MPC_MAX_NC + 2;                                         // nbins + 1
    unsigned long long *sum = (unsigned long long *)(e2 + nbins + 1);            // nbins (two's complement int64)
    uint32_t *cnt = (uint32_t *)(sum + nbins);                                   // nbins
    for (int b = threadIdx.x; b <= nbins; b += blockDim.x) e2[b] = e2g[b];
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
        cnt[b] = 0u;
        sum[b] = 0ull;
    }
    if (threadIdx.x < MD_MPC_MAX_NC) wl[threadIdx.x] = W.w[threadIdx.x];
    if (threadIdx.x == 0) {
        wl[MD_MPC_MAX_NC] = W.scale;
        wl[MD_MPC_MAX_NC + 1] = W.lim;
    }
    __syncthreads();
    double w[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) w[c] = wl[c];
    const double scale = wl[MD_MPC_MAX_NC], lim = wl[MD_MPC_MAX_NC + 1];
    const double e2max = e2[nbins];
    const int lane = threadIdx.x & 63;
    const int nb1 = nbins - 1;
    constexpr int NS = (D == 3) ? 14 : 5;
    int since_drain = 0; // this lane's LDS increments since the wave last drained (uint32 overflow guard, as in rdf)
    bool bad = false;
    for (;;) {
        int cell = 0;
        if (lane == 0) cell = atomicAdd(work, 1);
        cell = __shfl(cell, 0);
        if (cell >= rg.ncell) break;
        const int cx = cell % rg.nc[0], cy = (cell / rg.nc[0]) % rg.nc[1], cz = cell / (rg.nc[0] * rg.nc[1]);
        const int hs = cell_start[cell], he = cell_end[cell];
        for (int h0 = hs; h0 < he; h0 += 64) {
            const int hi = h0 + lane;
            const bool act = hi < he;
            double4 ph = act ? srec[hi] : make_double4(0.0, 0.0, 0.0, -1.0);
            const int idh = (int)ph.w;
            double ah[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) ah[c] = act ? smarks[(size_t)hi * NC + c] : 0.0;
#pragma nounroll
            for (int sidx = 0; sidx < NS; ++sidx) {
                int o[3] = {0, 0, 0};
                if (sidx > 0) {
                    // 3-D: 9 with dz = +1, 3 with dz = 0 and dy = +1, then (+1, 0, 0); 2-D: 3 with dy = +1, then (+1, 0)
                    int q = sidx - 1;
                    if (D == 3 && q < 9) {
                        o[0] = q % 3 - 1;
                        o[1] = q / 3 - 1;
                        o[2] = 1;
                    } else {
                        if (D == 3) q -= 9;
                        if (q < 3) {
                            o[0] = q - 1;
                            o[1] = 1;
                        } else {
                            o[0] = 1;
                        }
                    }
                }
                int e[3] = {cx + o[0], cy + o[1], cz + o[2]};
                double sh[3] = {0.0, 0.0, 0.0};
                bool shifted = false;
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    if (e[c] < 0) {
                        e[c] += rg.nc[c];
                        sh[c] = -1.0;
                        shifted = true;
                    } else if (e[c] >= rg.nc[c]) {
                        e[c] -= rg.nc[c];
                        sh[c] = 1.0;
                        shifted = true;
                    }
                }
                double t[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int r = 0; r < D; ++r) t[r] = (sh[0] * rg.A[r * 3 + 0] + sh[1] * rg.A[r * 3 + 1]) + sh[2] * rg.A[r * 3 + 2];
                const int ncell_n = (e[2] * rg.nc[1] + e[1]) * rg.nc[0] + e[0];
                const bool self = sidx == 0;
                const int ns = self ? h0 : cell_start[ncell_n];
                const int ne = self ? he : cell_end[ncell_n];
                for (int j0 = ns; j0 < ne; j0 += 64) {
                    const int m = min(64, ne - j0);
                    double4 pn = (lane < m) ? srec[j0 + lane] : make_double4(0.0, 0.0, 0.0, -1.0);
                    // the chunk's marks: m NC consecutive doubles.  LDS operations of one wave execute in order; the
                    // fences keep the compiler from moving a read above the stores (and the next chunk's stores above
                    // these reads)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    {
                        const double *run = smarks + (size_t)j0 * NC;
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            const int i = c * 64 + lane;
                            if (i < m * NC) chunk[i] = run[i];
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (act) {
#pragma nounroll
                        for (int jj = 0; jj < m; ++jj) {
                            const double xn = rdf_readlane(pn.x, jj);
                            const double yn = rdf_readlane(pn.y, jj);
                            const double zn = (D == 3) ? rdf_readlane(pn.z, jj) : 0.0;
                            double dx, dy, dz = 0.0;
                            if (!shifted) {
                                dx = xn - ph.x;
                                dy = yn - ph.y;
                                if constexpr (D == 3) dz = zn - ph.z;
                            } else {
                                // the end with the larger original id is the translated one (md_rdf.hpp)
                                const int idn = (int)rdf_readlane(pn.w, jj);
                                if (idh < idn) {
                                    dx = (xn + t[0]) - ph.x;
                                    dy = (yn + t[1]) - ph.y;
                                    if constexpr (D == 3) dz = (zn + t[2]) - ph.z;
                                } else {
                                    dx = (ph.x - t[0]) - xn;
                                    dy = (ph.y - t[1]) - yn;
                                    if constexpr (D == 3) dz = (ph.z - t[2]) - zn;
                                }
                            }
                            const double d2 = d2_ref<D>(dx, dy, dz);
                            if (d2 < e2max && (!self || j0 + jj > hi)) {
                                int k = (int)(sqrtf((float)d2) * inv_delta);
                                k = k < 0 ? 0 : (k > nb1 ? nb1 : k);
                                // the table decides: e2[k] <= d2 < e2[k + 1]
                                while (k > 0 && d2 < e2[k]) --k;
                                while (k < nb1 && d2 >= e2[k + 1]) ++k;
                                double an[NC];
#pragma unroll
                                for (int c = 0; c < NC; ++c) an[c] = chunk[jj * NC + c];
                                const long long I = mpc_term<NC>(ah, an, w, scale, lim, bad);
                                atomicAdd(&cnt[k], 1u);
                                atomicAdd(&sum[k], (unsigned long long)I);
                                ++since_drain;
                            }
                        }
                    }
                    // uint32 guard (md_rdf.hpp's): a wave that has added more than 2^23 per lane moves the counts and the
                    // sums out; an atomic exchange keeps every concurrent add of the other waves, in either word
                    if (__any(since_drain > (1 << 23))) {
                        for (int b = lane; b < nbins; b += 64) {
                            uint32_t v = atomicExch(&cnt[b], 0u);
                            unsigned long long sv = atomicExch(&sum[b], 0ull);
                            if (v) atomicAdd(&cur_cnt[b], (unsigned long long)v);
                            if (sv) atomicAdd(&cur_sum[b], sv);
                        }
                        since_drain = 0;
                    }
                }
            }
        }
    }
    if (__any(bad) && lane == 0) atomicOr(range_error, MD_MPC_ERR_TERM);
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
        uint32_t v = cnt[b];
        unsigned long long sv = sum[b];
        if (v) atomicAdd(&cur_cnt[b], (unsigned long long)v);
        if (sv) atomicAdd(&cur_sum[b], sv);
    }
}

// One thread per bin: the per-sample words into the accumulators (one conversion and one add per sample, in sample
// order), kept as the last sample, zeroed for the next; thread 0 does the same for self.
__global__ void __launch_bounds__(MD_BLOCK)
    k_mpc_finish(int nbins, unsigned long long *__restrict__ cur_cnt, long long *__restrict__ cur_sum,
                 long long *__restrict__ cur_self, unsigned long long *__restrict__ last_cnt,
                 long long *__restrict__ last_sum, long long *__restrict__ last_self,
                 unsigned long long *__restrict__ acc_cnt, double *__restrict__ acc_sum, double *__restrict__ acc_self,
                 int32_t *__restrict__ range_error)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbins) return;
    const unsigned long long c = cur_cnt[b];
    const long long s = cur_sum[b];
    if (c >= (1ull << 31)) atomicOr(range_error, MD_MPC_ERR_COUNT);
    acc_cnt[b] += c;
    acc_sum[b] = acc_sum[b] + (double)s;
    last_cnt[b] = c;
    last_sum[b] = s;
    cur_cnt[b] = 0ull;
    cur_sum[b] = 0ll;
    if (b == 0) {
        const long long sf = cur_self[0];
        acc_self[0] = acc_self[0] + (double)sf;
        last_self[0] = sf;
        cur_self[0] = 0ll;
    }
}
