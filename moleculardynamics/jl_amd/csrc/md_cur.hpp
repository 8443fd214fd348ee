// md_cur.hpp -- current correlations and the velocity autocorrelation sampled on the device (md_cur_* in
// include/mdhip.h): the particle current j_a(q) = sum_i v_i,a exp(+i q.x_i) of the current frame on md_sq's wave vectors,
// the static sums |j|^2 and |e.j|^2, their correlations against stored origins (behind the longitudinal and transverse
// current correlation functions C_L(q, t), C_T(q, t)) and Z = sum_i v_i(t).v_i(t0) (behind the VACF).
//
// One md_cur_sample call = one k_export of the current frame (wrapped x and v in particle-id order), then
//   k_sq_frac      md_sq's f = U^-1 x, one array per axis
//   k_cur_vaxis    v, one array per axis (va[a * n + i]), so the walk reads it coalesced
//   k_cur_modes    grid = (tiles of MD_CUR_TILE vectors, fastest) x (blocks of MD_CUR_BLOCK * MD_CUR_PPT ids): md_sq.hpp's
//                  mode_walk with CurTerm -- particles across lanes, the tile's vectors wave-uniform (scalar loads), no
//                  LDS in the walk -- with 2 * D * MD_CUR_TILE fp64 accumulators per thread; block partials per (vector,
//                  component, part, block).  The blocks in flight together share a few particle blocks, so f and v come
//                  from L2
//   k_cur_reduce   one wave per vector: the partials in md_sq's fixed tree (sq_row_sum) -> j; then lane 0 adds the static
//                  sums, the correlations of this call in call order and stores the origin, in that order
//   k_cur_vacf, k_cur_vacf_reduce   (with vacf) Z of every (slot, row) pair over particle ids, md_dyn's tree
//
// Exactness contract: the phase is md_sq's operation for operation (t = (n_0 f_0 + n_1 f_1) + n_2 f_2
// with every operation rounded on its own, r = t - rint(t), sq_cossin); the particle adds fma(v_a, c, Re j_a) and
// fma(v_a, s, Im j_a).  The tree of the sum is md_sq's, fixed by N alone -- thread: MD_CUR_PPT ids in order; wave: shuffle
// tree; block: the four waves in order; k_cur_reduce: lane l sums the blocks l, l + 64, ... in order, then a shuffle tree
// -- so the longest chain of dependent additions is md_sq's 47 at N = 2^22, and j is a function of the frame alone.  The
// accumulators are no-fma expressions of the j values.
#pragma once
#include "md_sq.hpp"

#define MD_CUR_BLOCK 256
#define MD_CUR_PPT 16             // particle ids per thread (md_sq's: the same tree)
#define MD_CUR_TILE 4             // wave vectors per block: 2 * 3 * 4 = 24 fp64 accumulators per thread in 3-D
#define MD_CUR_MAX_BATCH 64       // correlations per k_cur_reduce launch, (slot, row) pairs per k_cur_vacf launch
#define MD_CUR_REDUCE_BLOCK 256
#define MD_CUR_VACF_BLOCK 256
#define MD_CUR_VACF_PPT 4         // md_dyn's MD_DYN_PPT
#define MD_CUR_VACF_REDUCE_BLOCK 1024

static_assert(MD_SQ_TILE % MD_CUR_TILE == 0, "wave_vector_table pads to whole md_sq tiles");
static_assert(MD_CUR_BLOCK == MD_SQ_BLOCK && MD_CUR_PPT == MD_SQ_PPT, "mode_walk's block and its tree are md_sq's");

struct CurBatch {
    int count;
    int slot[MD_CUR_MAX_BATCH];   // (k_cur_vacf: -1 = the current frame itself, the equal-time sample)
    int row[MD_CUR_MAX_BATCH];
};

// v of the exported frame (n x D, particle-id order) written one array per axis, as k_sq_frac writes f
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_cur_vaxis(int n, const double *__restrict__ v, double *__restrict__ va)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int a = 0; a < D; ++a) va[(size_t)a * n + i] = v[(size_t)i * D + a];
}

// mode_walk's term for j: particle i brings v_i (va, one array per axis) and adds fma(v_a, c, Re j_a), fma(v_a, s, Im j_a)
// per axis; acc[a * 2 + {Re, Im}].
template <int D>
struct CurTerm {
    static constexpr int NPV = 2 * D;
    double vel[D];
    __device__ __forceinline__ void load(const double *__restrict__ va, int n, int i)
    {
#pragma unroll
        for (int a = 0; a < D; ++a) vel[a] = va[(size_t)a * n + i];
    }
    __device__ __forceinline__ void add(double c, double s, double *acc) const
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int a = 0; a < D; ++a) {
            acc[a * 2] = fma(vel[a], c, acc[a * 2]);
            acc[a * 2 + 1] = fma(vel[a], s, acc[a * 2 + 1]);
        }
    }
};

// nd: md_sq's table (3 doubles per vector, zero-padded to whole tiles).  part[((v * D + a) * 2 + part) * nblk + block].
// One-dimensional grid of ntiles * nblk blocks, the tile index running fastest: a tile of 4 re-reads f and v (48 B per
// particle) once per tile, twice md_sq's traffic per term, and with the particle block running fastest every tile streamed
// the whole frame (50 MB at N = 2^20) through the Infinity Cache; in this order the resident blocks walk the same few
// particle blocks and the re-reads hit L2.  The sums and their tree do not depend on the order of the blocks.
template <int D>
__global__ void __launch_bounds__(MD_CUR_BLOCK)
    k_cur_modes(int n, int nblk, int ntiles, const double *__restrict__ fr, const double *__restrict__ va,
                const double *__restrict__ nd, double *__restrict__ part)
{
    const int pblk = (int)(blockIdx.x / (unsigned)ntiles);
    const int v0 = (int)(blockIdx.x - (unsigned)pblk * (unsigned)ntiles) * MD_CUR_TILE;
    mode_walk<D, MD_CUR_TILE, false, CurTerm<D>>(n, nblk, pblk, v0, fr, va, nd, part, nullptr, 0);
}

// pL = (e_0 j_0 + e_1 j_1) + e_2 j_2 of one part (Re or Im) of j
template <int D>
__device__ __forceinline__ double cur_long(const double *__restrict__ e, const double (&j)[3])
{
#pragma clang fp contract(off)
    double p = e[0] * j[0] + e[1] * j[1];
    if constexpr (D == 3) p = p + e[2] * j[2];
    return p;
}

// One wave per vector.  reduce != 0: j[v] from the block partials (and the static sums if add_static); otherwise j[v] is
// read back (a later batch of the same call).  Then the batch's correlations in call order, then the origin store.
// jout[(v * D + a) * 2 + part]; e[v * D + a]; org[(slot * nvec + v) * 2 D + a * 2 + part].
template <int D>
__global__ void __launch_bounds__(MD_CUR_REDUCE_BLOCK)
    k_cur_reduce(int nvec, int nblk, int reduce, int add_static, CurBatch B, int origin_slot,
                 const double *__restrict__ part, const double *__restrict__ e, double *__restrict__ jout,
                 double *__restrict__ s_tot, double *__restrict__ s_long, double *__restrict__ c_tot,
                 double *__restrict__ c_long, double *__restrict__ org)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * (MD_CUR_REDUCE_BLOCK / 64) + (threadIdx.x >> 6);
    if (v >= nvec) return; // (the whole wave)
    double re[3] = {0.0, 0.0, 0.0}, im[3] = {0.0, 0.0, 0.0};
    if (reduce) {
#pragma unroll
        for (int a = 0; a < D; ++a) sq_row_sum(part + ((size_t)v * D + a) * 2 * nblk, nblk, lane, re[a], im[a]);
    }
    if (lane != 0) return;
    double *jv = jout + (size_t)v * 2 * D;
    const double *ev = e + (size_t)v * D;
    if (reduce) {
#pragma unroll
        for (int a = 0; a < D; ++a) {
            jv[2 * a] = re[a];
            jv[2 * a + 1] = im[a];
        }
    } else {
#pragma unroll
        for (int a = 0; a < D; ++a) {
            re[a] = jv[2 * a];
            im[a] = jv[2 * a + 1];
        }
    }
    const double lre = cur_long<D>(ev, re), lim = cur_long<D>(ev, im);
    if (reduce && add_static) {
        double t = re[0] * re[0] + im[0] * im[0];
#pragma unroll
        for (int a = 1; a < D; ++a) t = t + (re[a] * re[a] + im[a] * im[a]);
        s_tot[v] = s_tot[v] + t;
        s_long[v] = s_long[v] + (lre * lre + lim * lim);
    }
    for (int i = 0; i < B.count; ++i) {
        const double *o = org + ((size_t)B.slot[i] * nvec + v) * 2 * D;
        double ore[3] = {0.0, 0.0, 0.0}, oim[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < D; ++a) {
            ore[a] = o[2 * a];
            oim[a] = o[2 * a + 1];
        }
        double t = re[0] * ore[0] + im[0] * oim[0];
#pragma unroll
        for (int a = 1; a < D; ++a) t = t + (re[a] * ore[a] + im[a] * oim[a]);
        const double ole = cur_long<D>(ev, ore), oli = cur_long<D>(ev, oim);
        const size_t r = (size_t)B.row[i] * nvec + v;
        c_tot[r] = c_tot[r] + t;
        c_long[r] = c_long[r] + (lre * ole + lim * oli);
    }
    if (origin_slot >= 0) {
        double *o = org + ((size_t)origin_slot * nvec + v) * 2 * D;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            o[2 * a] = re[a];
            o[2 * a + 1] = im[a];
        }
    }
}

// Z of one (slot, row) pair per blockIdx.y: sum over particle ids of (v_0 o_0 + v_1 o_1) + v_2 o_2, no fma; both frames
// n x D in particle-id order (a slot < 0: the current frame against itself).  zpart[pair * nblk + block].
template <int D>
__global__ void __launch_bounds__(MD_CUR_VACF_BLOCK)
    k_cur_vacf(int n, int nblk, CurBatch B, const double *__restrict__ vc, const double *__restrict__ vo_all,
               double *__restrict__ zpart)
{
#pragma clang fp contract(off)
    __shared__ double wsum[MD_CUR_VACF_BLOCK / 64];
    const int smp = blockIdx.y, slot = B.slot[smp];
    const double *__restrict__ vo = slot < 0 ? vc : vo_all + (size_t)slot * n * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    const int base = blockIdx.x * (MD_CUR_VACF_BLOCK * MD_CUR_VACF_PPT) + threadIdx.x;
#pragma unroll
    for (int m = 0; m < MD_CUR_VACF_PPT; ++m) {
        const int i = base + m * MD_CUR_VACF_BLOCK;
        if (i < n) {
            const size_t o = (size_t)i * D;
            double t = vc[o] * vo[o] + vc[o + 1] * vo[o + 1];
            if constexpr (D == 3) t = t + vc[o + 2] * vo[o + 2];
            acc += t;
        }
    }
    const double w = sq_wave_sum(acc);
    if (lane == 0) wsum[wave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
#pragma unroll
        for (int k = 1; k < MD_CUR_VACF_BLOCK / 64; ++k) s = s + wsum[k];
        zpart[(size_t)smp * nblk + blockIdx.x] = s;
    }
}

// One block, the pairs of the batch one after the other: thread t sums the blocks t, t + 1024, ... in order, a shuffle
// tree within each wave, a shuffle tree over the 16 wave sums, and thread 0 adds the total into z[row] -- two pairs of one
// batch on one row are added in call order.  (A template like the other kernels of this file, so that all of them are
// emitted after the kernels the library had before.)
template <int D>
__global__ void __launch_bounds__(MD_CUR_VACF_REDUCE_BLOCK)
    k_cur_vacf_reduce(int nblk, CurBatch B, const double *__restrict__ zpart, double *__restrict__ z)
{
#pragma clang fp contract(off)
    __shared__ double wtot[MD_CUR_VACF_REDUCE_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = 0; i < B.count; ++i) {
        const double *p = zpart + (size_t)i * nblk;
        double s = 0.0;
        for (int b = threadIdx.x; b < nblk; b += MD_CUR_VACF_REDUCE_BLOCK) s += p[b];
        s = sq_wave_sum(s);
        if (lane == 0) wtot[wave] = s;
        __syncthreads();
        if (wave == 0) {
            double t = lane < MD_CUR_VACF_REDUCE_BLOCK / 64 ? wtot[lane] : 0.0;
#pragma unroll
            for (int off = MD_CUR_VACF_REDUCE_BLOCK / 128; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
            if (lane == 0) z[B.row[i]] = z[B.row[i]] + t;
        }
        __syncthreads();
    }
}
