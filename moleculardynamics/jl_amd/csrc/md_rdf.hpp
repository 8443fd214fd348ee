// md_rdf.hpp -- the radial distribution function g(r), sampled on the device (md_rdf_* in include/mdhip.h).
//
// One sample = four launches on the handle's stream, no host wait:
//   k_rdf_key     per particle: the coordinate md_download would return (k_export's lazy wrap, recomputed, never
//                 written back), its cell on the rdf grid (cells >= r_max wide, cut in fractional coordinates)
//   radix sort    (rocPRIM) of the cell digits, particle slot as the value
//   k_rdf_gather  sorted records {x, y, z, original id} and every cell's range (the list build's k_gather pattern)
//   k_rdf_hist    the pairs over the forward half of the cell stencil; per-workgroup uint32 counts in LDS, flushed
//                 into the uint64 histogram with one integer atomic per nonzero bin
//
// Exactness contract: the pair {a, b}, a < b ORIGINAL ids, has del = (x_b + t) - x_a with t the
// periodic translation that brings b next to a (t_r = (s0 U_r0 + s1 U_r1) + s2 U_r2, shift_xyz's form; s L for a diagonal
// cell), d2 = (del0 del0 + del1 del1) + del2 del2 with no fma (oracle/md_oracle.c canon_d2 / tric_d2), and it is counted
// in bin k iff e2[k] <= d2 < e2[k+1], e2 being the host's table.  Integer counts: the result does not depend on the
// order in which the pairs are visited.
#pragma once
#include "md_kernels.hpp"

#define MD_RDF_BLOCK 256
#define MD_RDF_MAX_BINS 8192

struct RdfGrid {
    int nc[3];        // cells per lattice direction (>= 3 for a used one, 1 for the unused z of 2-D)
    int ncell;
    double A[9];      // unit cell, row-major, columns = lattice vectors
    double Ainv[9];
};

// Stage 1: wrapped coordinate + cell key of every particle.  The wrap is k_export's, operation for operation, so the
// coordinate is bit-identical to what md_download returns; the state itself is only read.
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_rdf_key(int n, DevState s, BoxGrid g, RdfGrid rg, double4 *__restrict__ wrec, uint32_t *__restrict__ keys,
              uint32_t *__restrict__ vals)
{
#pragma clang fp contract(off)
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double4 p = s.pos[k];
    int32_t dn[3] = {0, 0, 0};
    if (g.tric) wrap_general<D>(p.x, p.y, p.z, g.A, g.Ainv, dn);
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double xc = pos_get(p, c);
        if (!g.tric && (xc < 0.0 || xc >= g.L[c])) {
            double frac = g.invL[c] * xc;
            double nn = floor(frac);
            xc = g.L[c] * (frac - nn);
        }
        pos_set(p, c, xc);
    }
    if constexpr (D == 2) p.z = 0.0;
    double fr[3];
    frac_of<D>(p.x, p.y, p.z, rg.Ainv, fr);
    int cc[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < D; ++c) {
        // L (frac - floor(frac)) can round up to L, and frac_of of a wrapped coordinate can land an ulp outside [0, 1)
        int q = (int)(fr[c] * (double)rg.nc[c]);
        q = q < 0 ? 0 : q;
        cc[c] = q > rg.nc[c] - 1 ? rg.nc[c] - 1 : q;
    }
    p.w = (double)s.id[k]; // exact: ids fit 31 bits
    wrec[k] = p;
    keys[k] = (uint32_t)((cc[2] * rg.nc[1] + cc[1]) * rg.nc[0] + cc[0]);
    vals[k] = (uint32_t)k;
}

// Stage 2 (after the sort): records in cell order, cell ranges [cell_start, cell_end) (both zeroed beforehand).
__global__ void __launch_bounds__(MD_BLOCK)
    k_rdf_gather(int n, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                 const double4 *__restrict__ wrec, double4 *__restrict__ srec, int32_t *__restrict__ cell_start,
                 int32_t *__restrict__ cell_end)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t key = keys[k];
    srec[k] = wrec[vals[k]];
    if (k == 0 || keys[k - 1] != key) {
        cell_start[key] = k;
        if (k > 0) cell_end[keys[k - 1]] = k;
    }
    if (k == n - 1) cell_end[key] = n;
}

__device__ __forceinline__ double rdf_readlane(double v, int l)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// Stage 3: the histogram.  Every wave takes home cells from a work counter; its 64 lanes hold up to 64 home particles,
// and the particles of the home cell and of its forward half-stencil (13 cells in 3-D, 4 in 2-D) are read 64 at a time
// into registers, one per lane, and handed to the whole wave by v_readlane: no LDS staging, no barrier inside the walk.
// LDS holds the edge table e2[0..nbins] and the workgroup's uint32 counts.
template <int D>
__global__ void __launch_bounds__(MD_RDF_BLOCK)
    k_rdf_hist(RdfGrid rg, int nbins, float inv_delta, const double *__restrict__ e2g, const double4 *__restrict__ srec,
               const int32_t *__restrict__ cell_start, const int32_t *__restrict__ cell_end, int32_t *__restrict__ work,
               unsigned long long *__restrict__ hist)
{
#pragma clang fp contract(off)
    extern __shared__ double rdf_lds[];
    double *e2 = rdf_lds;                                    // nbins + 1
    uint32_t *cnt = (uint32_t *)(rdf_lds + nbins + 1);       // nbins
    for (int b = threadIdx.x; b <= nbins; b += blockDim.x) e2[b] = e2g[b];
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) cnt[b] = 0u;
    __syncthreads();
    const double e2max = e2[nbins];
    const int lane = threadIdx.x & 63;
    const int nb1 = nbins - 1;
    // the forward half of the 3^D stencil, home cell first
    constexpr int NS = (D == 3) ? 14 : 5;
    int since_drain = 0; // this lane's LDS increments since the wave last drained the counts (uint32 overflow guard)
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
                // t = the translation of the neighbour cell's particles (shift_xyz's form; exact s L when diagonal)
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
                    if (act) {
                        for (int jj = 0; jj < m; ++jj) {
                            const double xn = rdf_readlane(pn.x, jj);
                            const double yn = rdf_readlane(pn.y, jj);
                            const double zn = (D == 3) ? rdf_readlane(pn.z, jj) : 0.0;
                            double dx, dy, dz = 0.0;
                            if (!shifted) {
                                // t = 0: both orders give the same d2
                                dx = xn - ph.x;
                                dy = yn - ph.y;
                                if constexpr (D == 3) dz = zn - ph.z;
                            } else {
                                // the end with the larger original id is the translated one: (x_nbr + t) - x_home, or
                                // (x_home - t) - x_nbr when the home particle has the larger id
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
                                atomicAdd(&cnt[k], 1u);
                                ++since_drain;
                            }
                        }
                    }
                    // uint32 guard: a wave that has added more than 2^23 per lane moves the counts out (atomic exchange
                    // keeps every concurrent add of the other waves); 4 waves x 2^29 (+ one chunk) stay below 2^32
                    if (__any(since_drain > (1 << 23))) {
                        for (int b = lane; b < nbins; b += 64) {
                            uint32_t v = atomicExch(&cnt[b], 0u);
                            if (v) atomicAdd(&hist[b], (unsigned long long)v);
                        }
                        since_drain = 0;
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
        uint32_t v = cnt[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);
    }
}
