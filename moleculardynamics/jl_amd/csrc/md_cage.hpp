// md_cage.hpp -- cage-relative dynamics and bond breaking, sampled on the device (md_cage_* in include/mdhip.h): the
// displacement of a particle relative to the mean displacement of the neighbours it had at the time origin (its MSD,
// fourth moment and F_s), and the fraction of origin bonds still shorter than a break radius (Yamamoto-Onuki's C_B).
//
// md_cage_origin = one k_export into the slot's frame, then one walk of the OUTER rows (md_rowwalk.hpp's kernel pair):
//   k_rows_tile / k_rows<CageOriginLane>   one lane per particle; every row entry that passes the bond criterion with
//                                          r_neigh appends (id_j, del_ij) to the entry list of particle id_i, in row order,
//                                          up to max_neigh entries; the hits beyond are counted in `overflow`
// md_cage_sample = one k_export of the current frame, then per batch of up to MD_CAGE_MAX_BATCH (slot, row) pairs:
//   k_cage_disp     over particle ids: the displacement Del_i since the slot's origin (md_dyn's dyn_disp), written
//                   component-major by id
//   k_cage_sample   over particle ids: gathers Del_j of the n_i entries by id, the cage-relative displacement, d2, d4 and
//                   the cosine sums; the bond vector at t, b = del_ij + (Del_j - Del_i), against r_break; fp64 block
//                   partials in md_dyn's fixed tree (dyn_store_part), the integers in LDS counters flushed with 64-bit
//                   integer atomics
//   k_dyn_reduce    (md_dyn.hpp, as it is) the partials of every sample summed in block order into the rows
// Nothing waits for the device and nothing of the handle is written.
//
// The table of a slot is keyed by particle id, entry-major: nid[(slot mn + k) N + id], del[((slot mn + k) d + c) N + id],
// so what a list rebuild or an upload does to the slot order does not touch it and the sample's own reads coalesce.
//
// Arithmetic contract: sigma_ij = (sigma_i + sigma_j) / 2.0; a radius r is passed iff
// d2 < (r s) (r s), s = sigma_ij (scaled) or 1.0; d2 = d2_ref of the vector.  Del as in md_dyn.hpp (no fma);
// m_i = (sum_k Del_{j_k}) / n_i in entry order, Del^CR_i = Del_i - m_i, s_i(q) = sum_c cos(q Del^CR_c).
#pragma once
#include "md_rowwalk.hpp"
#include "md_dyn.hpp"

#define MD_CAGE_MAX_NEIGH 32
#define MD_CAGE_MAX_BATCH 8       // (slot, row) pairs per launch triple: the displacements of a batch are kept by id
#define MD_CAGE_NCOUNT 3          // per row: particles with neighbours, sum n_i, surviving bonds
#define MD_CAGE_NHIST (MD_CAGE_MAX_NEIGH + 1)
static_assert(MD_CAGE_MAX_BATCH <= MD_DYN_MAX_BATCH, "k_dyn_reduce sums a batch of the cage sampler");

// One origin slot's part of the table, and the criterion
struct CageOrigin {
    int n, max_neigh, scaled;
    double r_neigh;
    int32_t *nnb;                 // [id]
    int32_t *nid;                 // [k][id]
    double *del;                  // [k][c][id]
    double *sig;                  // [id]
    unsigned long long *overflow;
};

__device__ __forceinline__ bool cage_bonded(double d2, double r, double s)
{
    const double t = r * s;
    return d2 < t * t;
}

template <int D>
struct CageOriginLane {
    using Args = CageOrigin;
    size_t idi;
    double sig_i;
    int hits;
    bool active;
    __device__ __forceinline__ void begin(const Args &, const DevState &s, int, int kk, bool active_, const double4 &pi)
    {
        idi = (size_t)s.id[kk];
        sig_i = pi.w;
        hits = 0;
        active = active_;
    }
    __device__ __forceinline__ void visit(const Args &T, const DevState &s, bool hit, double dx, double dy, double dz,
                                          double d2, uint32_t own)
    {
        if (!hit) return;
        // (own is an owned slot here: the walk resolved it, and the sentinel is never within the list cutoff)
        double sc = 1.0;
        if (T.scaled) sc = (sig_i + s.pos[own].w) / 2.0;
        if (!cage_bonded(d2, T.r_neigh, sc)) return;
        if (active && hits < T.max_neigh) {
            const size_t e = (size_t)hits * T.n;
            T.nid[e + idi] = s.id[own];
            T.del[(e * D) + idi] = dx;
            T.del[(e * D) + (size_t)T.n + idi] = dy;
            if constexpr (D == 3) T.del[(e * D) + 2 * (size_t)T.n + idi] = dz;
        }
        ++hits;
    }
    __device__ __forceinline__ void end(const Args &T, int, bool, int)
    {
        if (!active) return;
        const int kept = hits < T.max_neigh ? hits : T.max_neigh;
        T.nnb[idi] = kept;
        T.sig[idi] = sig_i;
        if (hits > kept) atomicAdd(T.overflow, (unsigned long long)(hits - kept));
    }
};

// ------------------------------------------------------------------------------------------
// Pass 1 of a sample: Del_i of every id against the origin of every slot of the batch (blockIdx.y), md_dyn's dyn_disp: the
// wrapped difference first, the lattice translation of the exact image difference added after, no fma.
// disp[(smp d + c) N + id]
// ------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(MD_DYN_BLOCK)
    k_cage_disp(DynParams P, DynBatch B, const double *__restrict__ xc, const int32_t *__restrict__ nc,
                const double *__restrict__ xo_all, const int32_t *__restrict__ no_all, double *__restrict__ disp)
{
#pragma clang fp contract(off)
    const int smp = blockIdx.y;
    const int i = blockIdx.x * MD_DYN_BLOCK + threadIdx.x;
    if (i >= P.n) return;
    const size_t frame = (size_t)P.n * D;
    const double *__restrict__ xo = xo_all + (size_t)B.slot[smp] * frame;
    const int32_t *__restrict__ no = no_all + (size_t)B.slot[smp] * frame;
    double del[3] = {0.0, 0.0, 0.0};
    dyn_disp<D>(P, xc, nc, xo, no, i, del);
#pragma unroll
    for (int c = 0; c < D; ++c) disp[((size_t)smp * D + c) * P.n + i] = del[c];
}

// ------------------------------------------------------------------------------------------
// Pass 2.  counts[row * 3 + {0, 1, 2}], hist[row * 33 + broken]; the per-particle arrays of batch entry `keep` (or of
// none: -1) are written out by id.
// ------------------------------------------------------------------------------------------
struct CageSample {
    int max_neigh, scaled, keep;
    double r_break;
    const int32_t *nnb, *nid;     // all slots: [slot][id], [slot][k][id]
    const double *del, *sig;      // [slot][k][c][id], [slot][id]
    const double *disp;           // [smp][c][id]
    double *part;
    unsigned long long *counts, *hist;
    int32_t *o_nnb, *o_broken;
    double *o_d2;
};

template <int D>
__global__ void __launch_bounds__(MD_DYN_BLOCK)
    k_cage_sample(DynParams P, DynBatch B, CageSample A)
{
#pragma clang fp contract(off)
    __shared__ double wsum[MD_DYN_BLOCK / 64][2 + MD_DYN_MAX_Q];
    __shared__ uint32_t cnt[MD_CAGE_NCOUNT + MD_CAGE_NHIST];
    const int smp = blockIdx.y;
    const size_t N = (size_t)P.n;
    const size_t slot = (size_t)B.slot[smp];
    const int32_t *__restrict__ nnb = A.nnb + slot * N;
    const int32_t *__restrict__ nid = A.nid + slot * A.max_neigh * N;
    const double *__restrict__ del = A.del + slot * A.max_neigh * D * N;
    const double *__restrict__ sig = A.sig + slot * N;
    const double *__restrict__ disp = A.disp + (size_t)smp * D * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < MD_CAGE_NCOUNT + MD_CAGE_NHIST) cnt[threadIdx.x] = 0u;
    __syncthreads();
    double acc2 = 0.0, acc4 = 0.0;
    double cr[MD_DYN_PPT][3];
    bool has[MD_DYN_PPT];
    const int base = blockIdx.x * (MD_DYN_BLOCK * MD_DYN_PPT) + threadIdx.x;
#pragma unroll
    for (int m = 0; m < MD_DYN_PPT; ++m) {
        const int i = base + m * MD_DYN_BLOCK;
        const bool act = i < P.n;
        int ni = act ? nnb[i] : 0;
        ni = ni < A.max_neigh ? ni : A.max_neigh; // (k < max_neigh whatever the table holds)
        has[m] = ni > 0;
        cr[m][0] = cr[m][1] = cr[m][2] = 0.0;
        double d2 = 0.0;
        int broken = 0;
        if (ni > 0) {
            double di[3] = {0.0, 0.0, 0.0}, sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int c = 0; c < D; ++c) di[c] = disp[c * N + i];
            const double sig_i = A.scaled ? sig[i] : 1.0;
            for (int k = 0; k < ni; ++k) {
                const size_t e = (size_t)k * N;
                uint32_t j = (uint32_t)nid[e + i];
                j = j < (uint32_t)P.n ? j : (uint32_t)P.n - 1u; // (id < N whatever the table holds)
                double b[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < D; ++c) {
                    const double dj = disp[c * N + j];
                    sum[c] = sum[c] + dj;
                    b[c] = del[(e * D) + c * N + i] + (dj - di[c]);
                }
                double sc = 1.0;
                if (A.scaled) sc = (sig_i + sig[j]) / 2.0;
                broken += cage_bonded(d2_ref<D>(b[0], b[1], b[2]), A.r_break, sc) ? 0 : 1;
            }
            const double fn = (double)ni;
#pragma unroll
            for (int c = 0; c < D; ++c) cr[m][c] = di[c] - sum[c] / fn;
            d2 = d2_ref<D>(cr[m][0], cr[m][1], cr[m][2]);
            acc2 += d2;
            acc4 += d2 * d2;
            atomicAdd(&cnt[0], 1u);
            atomicAdd(&cnt[1], (uint32_t)ni);
            atomicAdd(&cnt[2], (uint32_t)(ni - broken));
            atomicAdd(&cnt[MD_CAGE_NCOUNT + broken], 1u);
        }
        if (act && smp == A.keep) {
            A.o_nnb[i] = ni;
            A.o_broken[i] = broken;
            A.o_d2[i] = d2;
        }
    }
    // md_dyn's fixed tree: the thread's ids in order, a shuffle tree within the wave, then the waves in order
    {
        const double w2 = dyn_wave_sum(acc2), w4 = dyn_wave_sum(acc4);
        if (lane == 0) {
            wsum[wave][0] = w2;
            wsum[wave][1] = w4;
        }
    }
#pragma unroll 1
    for (int j = 0; j < P.nq; ++j) {
        const double q = P.q[j];
        double a = 0.0;
#pragma unroll
        for (int m = 0; m < MD_DYN_PPT; ++m) {
            if (has[m]) {
                double sq = cos(q * cr[m][0]);
#pragma unroll
                for (int c = 1; c < D; ++c) sq = sq + cos(q * cr[m][c]);
                a += sq;
            }
        }
        const double w = dyn_wave_sum(a);
        if (lane == 0) wsum[wave][2 + j] = w;
    }
    __syncthreads();
    dyn_store_part(P, wsum, smp, A.part);
    if (threadIdx.x < MD_CAGE_NCOUNT + MD_CAGE_NHIST) {
        const uint32_t v = cnt[threadIdx.x];
        if (v) {
            unsigned long long *dst = threadIdx.x < MD_CAGE_NCOUNT
                                          ? A.counts + (size_t)B.row[smp] * MD_CAGE_NCOUNT + threadIdx.x
                                          : A.hist + (size_t)B.row[smp] * MD_CAGE_NHIST + (threadIdx.x - MD_CAGE_NCOUNT);
            atomicAdd(dst, (unsigned long long)v);
        }
    }
}
