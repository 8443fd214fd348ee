// md_swap.hpp -- swap Monte Carlo on the device (md_swap_* in include/mdhip.h): rounds of diameter
// exchanges attempted in parallel at fixed positions, each round a valid Metropolis move for the diameter assignment.
//
// One round = five launches on the handle's stream, no host wait.  Everything indexed "by id" is indexed by PARTICLE ID, so a
// round is a function of (frame, diameters, seed, round index) and not of the slot order:
//   k_swap_propose   N-wide, elementwise: Philox words of particle i (key = seed, counter = (i, round lo, round hi, 1));
//                    i proposes iff w0 < thr, partner j = (w1 * N) >> 32, void when j == i, key = (w2 << 32) | i;
//                    both members take atomicMin(claim[.], key)
//   k_swap_live      N-wide, elementwise: a proposal that holds the minimum at both members is LIVE -- a particle is a member
//                    of at most one live swap; its two members get the key (livekey) and two consecutive entries of the
//                    compact member list
//   k_swap_walk      the hot path.  Fixed grid; the member count is read on the device.  ONE WAVE PER MEMBER walks that
//                    member's OUTER row, the row's entries split over the 64 lanes (entry r belongs to lane r & 63).  No
//                    LDS image: an entry is decoded as md_listrows.hpp decodes it (16-bit offset -> halo word -> slot + shift
//                    code, or 32-bit slot; a real ghost through gowner) and the distance is formed as the force kernels form
//                    it (shift_xyz, d2_ref).  Every entry with d2 <= list_cutoff^2 other than the partner: a neighbour that
//                    is a member of a live swap with a SMALLER key blocks this one; with d2 < pp.c2 the lane adds
//                    u(r, s_partner, s_k) - u(r, s_self, s_k), s_k = pos[owner].w.  Lane sums in row order, wave_sum's
//                    fixed butterfly; lane 0 writes the member's half of dU and its blocked flag.
//   k_swap_decide    N-wide, elementwise: per live swap blocked -> nothing; |s_i - s_j| > max difference -> filtered; else
//                    accept iff u3 < exp(-dU / kT), u3 = (w3 + 0.5) / 2^32 (a NaN compares false: rejected).  Accepting
//                    exchanges pos[].w of the two owner slots.  Writes partner / status / dU by id, resets claim and livekey
//                    for the next round, counts with integer atomics, block partials of the accepted dU
//   k_swap_finish    one block: the partials in block order onto the running sum; resets the member count
// No LDS atomics, no floating-point atomics.
#pragma once
#include "md_kernels.hpp"

#define MD_SWAP_TAG 1u          // fourth Philox counter word (the Brownian stream uses 0)
#define MD_SWAP_WALK_BLOCKS 1024 // fixed grid of the walk: 4 waves per block, wave-stride loop over the members
#define MD_SWAP_NCOUNT 8        // counter words, indexed by the status codes below

enum { MD_SWAP_NONE = 0, MD_SWAP_VOID = 1, MD_SWAP_LOST = 2, MD_SWAP_BLOCKED = 3, MD_SWAP_FILTERED = 4,
       MD_SWAP_REJECTED = 5, MD_SWAP_ACCEPTED = 6, MD_SWAP_LIVE = 7 /* between k_swap_live and k_swap_decide only */ };

#define MD_SWAP_NOKEY 0xffffffffffffffffull

struct SwapBufs {
    int n;                          // particles = ids
    unsigned long long *claim;      // n, by id
    unsigned long long *livekey;    // n, by id: key of the live swap the particle is a member of, or MD_SWAP_NOKEY
    int32_t *partner, *status;      // n, by proposer id
    int32_t *entry;                 // n, by proposer id: index of the swap's first member entry (live swaps)
    int32_t *members;               // 2 per entry: {self id, partner id}; at most n entries
    double *half;                   // per entry
    int32_t *blocked;               // per entry
    int32_t *nmember;               // 1
    double *du;                     // n, by proposer id
    const int32_t *inv;             // n: id -> slot
    unsigned long long *counts;     // MD_SWAP_NCOUNT
    double *partials, *du_acc;      // blocks of k_swap_decide; 1
};

__device__ __forceinline__ void swap_words(int i, unsigned long long seed, long long round, uint32_t (&w)[4])
{
    philox4x32_10((uint32_t)i, (uint32_t)round, (uint32_t)((unsigned long long)round >> 32), MD_SWAP_TAG, (uint32_t)seed,
                  (uint32_t)(seed >> 32), w);
}

// id -> slot
__global__ void __launch_bounds__(MD_BLOCK) k_swap_inv(int n, const int32_t *__restrict__ id, int32_t *__restrict__ inv)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) inv[id[k]] = k;
}

__global__ void __launch_bounds__(MD_BLOCK) k_swap_propose(SwapBufs B, unsigned long long seed, long long round, uint32_t thr)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    uint32_t w[4];
    swap_words(i, seed, round, w);
    int st = MD_SWAP_NONE, j = -1;
    if (w[0] < thr) {
        j = (int)(((unsigned long long)w[1] * (unsigned long long)B.n) >> 32);
        st = j == i ? MD_SWAP_VOID : MD_SWAP_LOST; // (lost until k_swap_live finds it holding both claims)
        if (j != i) {
            const unsigned long long key = ((unsigned long long)w[2] << 32) | (unsigned long long)(uint32_t)i;
            atomicMin(&B.claim[i], key);
            atomicMin(&B.claim[j], key);
        }
    }
    B.partner[i] = j;
    B.status[i] = st;
}

__global__ void __launch_bounds__(MD_BLOCK) k_swap_live(SwapBufs B, unsigned long long seed, long long round)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    if (B.status[i] != MD_SWAP_LOST) return;
    uint32_t w[4];
    swap_words(i, seed, round, w);
    const int j = B.partner[i];
    const unsigned long long key = ((unsigned long long)w[2] << 32) | (unsigned long long)(uint32_t)i;
    if (B.claim[i] != key || B.claim[j] != key) return;
    // (the minimum at both members: nobody else writes livekey[i] or livekey[j] this round)
    B.livekey[i] = key;
    B.livekey[j] = key;
    const int e = atomicAdd(B.nmember, 2);
    B.members[2 * e] = i;
    B.members[2 * e + 1] = j;
    B.members[2 * e + 2] = j;
    B.members[2 * e + 3] = i;
    B.entry[i] = e;
    B.status[i] = MD_SWAP_LIVE;
}

// The rows as the walk reads them (ListRowsView's fields, md_listrows.hpp)
struct SwapRows {
    int n, nghost;
    long long cap;          // slots of pos[] (the sentinel's index)
    const int32_t *id;
    const uint16_t *rows16; // 16-bit rows, or null: rows32
    const uint32_t *rows32;
    int maxn;
    const int32_t *rowlen;
    int rs;
    const uint32_t *halo;
    int hcap;
    const int32_t *halo_count;
    const int32_t *gowner;
};

template <int D, int POT>
__global__ void __launch_bounds__(MD_BLOCK)
    k_swap_walk(SwapRows V, DevState s, PotParams pp, double c2_inclusive, SwapBufs B)
{
    const int lane = threadIdx.x & 63;
    const int nwaves = gridDim.x * (MD_BLOCK / 64);
    int nm = *B.nmember;
    nm = nm > B.n ? B.n : nm; // (a particle is a member of at most one live swap)
    const double4 *__restrict__ P = s.pos;
    for (int e = blockIdx.x * (MD_BLOCK / 64) + (threadIdx.x >> 6); e < nm; e += nwaves) {
        const int a = B.members[2 * e], b = B.members[2 * e + 1];
        const int k = B.inv[a];
        const unsigned long long mykey = B.livekey[a];
        const double4 pa = P[k];
        const double sa = pa.w, sb = P[B.inv[b]].w;
        const int rl = k & 63, wave = k >> 6, tile = k / MD_TILE;
        const size_t wbase = ((size_t)wave * V.maxn) * 64;
        int m = V.rowlen[wave];
        m = m < 0 ? 0 : (m > V.maxn ? V.maxn : m);
        const int H = V.rows16 ? V.halo_count[tile] : 0;
        const uint32_t *hl = V.rows16 ? V.halo + (size_t)tile * V.hcap : nullptr;
        double acc = 0.0;
        int blk = 0;
        for (int r = lane; r < m; r += 64) {
            uint32_t slot, code = 0u;
            if (V.rows16) {
                const unsigned off = V.rows16[wbase + row_off(r, rl)];
                const unsigned h = off / (unsigned)V.rs;
                if (h >= (unsigned)H || h >= (unsigned)V.hcap) continue; // the sentinel record (padding)
                const uint32_t w = hl[h];
                slot = w & 0x3ffffffu;
                code = w >> 26;
            } else {
                slot = V.rows32[wbase + rl + (size_t)r * 64];
            }
            if ((long long)slot >= V.cap) continue; // the sentinel slot (padding)
            double4 pj = P[slot];
            if (code) shift_xyz(pj.x, pj.y, pj.z, code, s.boxL, s.tric, s.cellA);
            uint32_t own = slot;
            if (own >= (uint32_t)V.n) {
                const uint32_t gi = own - (uint32_t)V.n;
                if (gi >= (uint32_t)V.nghost) continue;
                own = (uint32_t)V.gowner[gi];
                if (own >= (uint32_t)V.n) continue;
            }
            const double dx = pj.x - pa.x;
            const double dy = pj.y - pa.y;
            double dz = 0.0;
            if constexpr (D == 3) dz = pj.z - pa.z;
            const double d2 = d2_ref<D>(dx, dy, dz);
            if (!(d2 <= c2_inclusive)) continue;
            const int kid = V.id[own];
            if (kid == b || kid == a) continue;
            if (B.livekey[kid] < mykey) blk = 1;
            if (d2 < pp.c2) {
                const double sk = P[own].w;
                double un, uo, fpr;
                pair_eval<POT, false, true>(d2, sb, sk, pp, un, fpr);
                pair_eval<POT, false, true>(d2, sa, sk, pp, uo, fpr);
                acc += un - uo;
            }
        }
        acc = wave_sum(acc);
        blk = __any(blk) ? 1 : 0;
        if (lane == 0) {
            B.half[e] = acc;
            B.blocked[e] = blk;
        }
    }
}

__global__ void __launch_bounds__(MD_BLOCK)
    k_swap_decide(SwapBufs B, DevState s, unsigned long long seed, long long round, double ktemp, double max_diff)
{
    __shared__ double red[16];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double dacc = 0.0;
    if (i < B.n) {
        int st = B.status[i];
        double du = 0.0;
        if (st == MD_SWAP_LIVE) {
            const int e = B.entry[i];
            const int j = B.partner[i];
            const int ki = B.inv[i], kj = B.inv[j];
            const double si = s.pos[ki].w, sj = s.pos[kj].w;
            if (B.blocked[e] | B.blocked[e + 1]) {
                st = MD_SWAP_BLOCKED;
            } else if (max_diff > 0.0 && fabs(si - sj) > max_diff) {
                st = MD_SWAP_FILTERED;
            } else {
                uint32_t w[4];
                swap_words(i, seed, round, w);
                du = B.half[e] + B.half[e + 1];
                const double u3 = ((double)w[3] + 0.5) * 2.3283064365386963e-10;
                if (u3 < exp(-du / ktemp)) {
                    st = MD_SWAP_ACCEPTED;
                    s.pos[ki].w = sj;
                    s.pos[kj].w = si;
                    dacc = du;
                } else {
                    st = MD_SWAP_REJECTED;
                }
            }
            B.status[i] = st;
        }
        B.du[i] = du;
    }
    // One counter word per status, gathered per wave by ballot (no LDS atomics), then one integer atomic per block
    const int stf = i < B.n ? B.status[i] : MD_SWAP_NONE;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int c = MD_SWAP_VOID; c <= MD_SWAP_ACCEPTED; ++c) {
        const unsigned long long mask = __ballot(stf == c);
        if (lane == 0 && mask) atomicAdd(&B.counts[c], (unsigned long long)__popcll(mask));
    }
    // the next round starts from empty claims.  (Nobody reads them in this kernel: the live test is k_swap_live's.)
    if (i < B.n) {
        B.claim[i] = MD_SWAP_NOKEY;
        B.livekey[i] = MD_SWAP_NOKEY;
    }
    const double t = block_sum(dacc, red);
    if (threadIdx.x == 0) B.partials[blockIdx.x] = t;
}

__global__ void __launch_bounds__(1024) k_swap_finish(int nblk, SwapBufs B)
{
    __shared__ double red[16];
    double a = strided_sum<4>(B.partials, nblk);
    a = block_sum(a, red);
    if (threadIdx.x == 0) {
        *B.du_acc = *B.du_acc + a;
        *B.nmember = 0;
    }
}

// diameters by particle id
__global__ void __launch_bounds__(MD_BLOCK) k_swap_diameters(int n, DevState s, double *__restrict__ out)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[s.id[k]] = s.pos[k].w;
}
