// md_cluster.hpp -- connected components of the bond graph, sampled on the device (md_cluster_* in include/mdhip.h): the
// cluster of every particle, the cluster-size histogram, the largest (solid) cluster.
//
// One sample = a fixed number of launches on the handle's stream, whatever the frame looks like, no host wait:
//   k_cl_mask                    SOLID only: BOO's per-slot nconn of ITS frame -> a by-particle-id member mask
//   k_cl_init                    parent[slot] = slot for members, CL_NONE otherwise; count = 0, minid = INT_MAX
//   k_rows_tile / k_rows<ClLane> md_rowwalk.hpp's staging, walk and acceptance test; every hit with owner < slot and both
//                                ends members is one union; the lane also counts its degree (block partials)
//   k_cl_flatten                 root[slot] = find(slot); count[root] += 1; minid[root] = min(id)
//   k_cl_stats                   roots only: the size histogram, block partials, the block's top two (size, ~label) keys
//   k_cl_finish                  one block: the partials -> fr, sum_fr += fr, series[m] = fr
//   k_cl_export                  (md_cluster_particles) slot order -> particle-id order
// Every result is an integer and a function of the frame alone: integer sums are exact in any order, a label is the
// smallest particle id of the cluster, not a slot.  No floating-point atomics.
//
// The union (ClLane, cl_union below) is lock-free.  parent[] is a forest over the slots; every edge points to a
// SMALLER slot of the same component, a root points to itself.  Three operations touch it, all agent-scope relaxed atomics
// (__hip_atomic_load / compare_exchange / fetch_min, __HIP_MEMORY_SCOPE_AGENT) -- the kernel has no plain load of
// parent[], because on this chip a CU's vector L1 is never refreshed by another CU's stores and the XCD L2s are not
// coherent with each other; agent-scope atomics are served where all XCDs agree:
//   walk     two walkers start on the two ends of a bond; the one on the larger slot x reads parent[x] and moves there.
//            A value read may be old; an old parent is still a smaller slot of the same component, so the walk only
//            takes longer.  The walkers meet on a common slot iff they are in one tree.
//   hook     parent[x] == x, a root, and the other walker stands on y < x: compare_exchange(parent[x], x, y).  Success
//            makes x a child of a smaller slot of the OTHER end's component: the two trees are one, for good.  Failure
//            returns the parent someone else gave x -- x is no root any more -- and the walker moves there.
//   shorten  parent[b] = min(parent[b], m) (fetch_min) for an end b and the slot m < b its walker ended on: an edge is
//            only ever replaced by an edge to a smaller slot of the same component.  It is issued only for a slot that
//            has been seen with a parent; such a slot never becomes a root again, so a root is written by a hook alone.
// So parents decrease monotonically within a component, nothing is ever split, and correctness rests on that and on the
// value the compare-exchange returns, not on the order or the timing of anything.  No thread waits for another
// workgroup: every step of a union lowers the larger of its two walkers, so a union ends after at most a + b steps
// whatever the others do; a failed hook -- always caused by someone else's SUCCESSFUL hook, of which a frame has at
// most n - 1 -- is one such step.  There is no residency assumption and nothing that can spin for ever.  When the
// kernel has ended every bond's two ends have been through a union that ended on a common slot, so the trees are the
// components; k_cl_flatten, a new launch, sees all of it and only reads parent[].
#pragma once
#include "md_rowwalk.hpp"

#define MD_CL_MAX_SIZE 65536
#define MD_CL_MAX_SERIES (1 << 20)
#define MD_CL_LDS_SIZE 1024 // up to this max_size the size histogram is gathered per block in LDS first
#define MD_CL_NFR 8
#define MD_CL_NPART 6       // block partials of k_cl_stats: members, clusters, sum s^2, singles, top key, second key
#define CL_NONE 0xffffffffu

typedef unsigned long long cl_u64;

__device__ __forceinline__ uint32_t cl_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One union of the components of a and b.  Two walkers climb the forest, u from a and v from b, and the one on the LARGER
// slot moves: to its parent, or -- when it stands on a root -- by hooking that root under the other walker's slot, which
// is smaller and belongs to the other end.  They stop on a common slot.  Two ends that already hang under the same node
// meet there after one load each and never read the root's own word, which finds that run to the root would all end on
// (in a giant component: every union of the frame on one address).  Returns the meeting slot, an ancestor-or-equal of
// a in the united component; b's edge is shortened to it.
__device__ __forceinline__ uint32_t cl_union(uint32_t *parent, uint32_t a, uint32_t b)
{
    uint32_t u = a, v = b;
    uint32_t kb = CL_NONE; // the last value known of parent[b], once it is known not to be a root
    while (u != v) {
        const bool up = u > v;
        const uint32_t x = up ? u : v, y = up ? v : u; // x > y: x moves
        uint32_t p = cl_load(parent + x);
        if (p == x) { // a root: hook it under y; a failure returns the parent someone else gave it
            if (__hip_atomic_compare_exchange_strong(parent + x, &p, y, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                p = y;
        }
        if (!up && x == b) kb = p;
        if (up)
            u = p;
        else
            v = p;
    }
    if (kb != CL_NONE && kb != v) __hip_atomic_fetch_min(parent + b, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return u;
}

// integer block sum (any order gives the same bits); lds: >= 16 words
__device__ __forceinline__ cl_u64 cl_block_sum(cl_u64 v, cl_u64 *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) lds[w] = v;
    __syncthreads();
    cl_u64 r = 0;
    for (int i = 0; i < nw; ++i) r += lds[i];
    return r;
}

// SOLID: BOO's frame (its per-slot nconn and its own slot -> id permutation) -> mask[id] = solid
__global__ void __launch_bounds__(MD_BLOCK)
    k_cl_mask(int n, const int32_t *__restrict__ boo_id, const int32_t *__restrict__ nconn, int min_conn,
              unsigned char *__restrict__ mask)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    mask[boo_id[k]] = nconn[k] >= min_conn ? 1 : 0;
}

// mask == nullptr: everyone is a member
__global__ void __launch_bounds__(MD_BLOCK)
    k_cl_init(int n, const int32_t *__restrict__ id, const unsigned char *__restrict__ mask, uint32_t *__restrict__ parent,
              unsigned char *__restrict__ mem, int32_t *__restrict__ count, int32_t *__restrict__ minid)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const bool m = mask ? mask[id[k]] != 0 : true;
    parent[k] = m ? (uint32_t)k : CL_NONE;
    mem[k] = m ? 1 : 0;
    count[k] = 0;
    minid[k] = 0x7fffffff;
}

// ------------------------------------------------------------------------------------------
// The hooks, a lane of md_rowwalk.hpp's walk.  deg_part[bid] = the block's sum of degrees.
// ------------------------------------------------------------------------------------------
struct ClArgs {
    const unsigned char *mem;
    uint32_t *parent;
    cl_u64 *deg_part;
};

struct ClLane {
    using Args = ClArgs;
    uint32_t kk;
    bool member;
    unsigned deg;
    uint32_t me; // the lowest ancestor of kk this lane has met: the next union starts there
    __device__ __forceinline__ void begin(const Args &A, const DevState &, int, int kk_, bool active, const double4 &)
    {
        kk = (uint32_t)kk_;
        member = active && A.mem[kk_] != 0;
        deg = 0u;
        me = (uint32_t)kk_;
    }
    __device__ __forceinline__ void visit(const Args &A, const DevState &, bool hit, double, double, double, double,
                                          uint32_t own)
    {
        if (!hit || !member || own == kk || !A.mem[own]) return;
        ++deg;
        if (own < kk) me = cl_union(A.parent, me, own);
    }
    __device__ __forceinline__ void end(const Args &A, int, bool, int bid)
    {
        __shared__ cl_u64 red[16];
        // kk's own edge, shortened to what the walk found (me != kk: kk has been seen with a parent, it is no root)
        if (member && me != kk) __hip_atomic_fetch_min(A.parent + kk, me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cl_u64 t = cl_block_sum((cl_u64)deg, red);
        if (threadIdx.x == 0) A.deg_part[bid] = t;
    }
};

// ------------------------------------------------------------------------------------------
// A new launch: every hook is visible.  parent[] is only read here; the roots go to an array of their own.  One global
// atomicAdd / atomicMin per lane on the root's words: in a giant component that is n adds on one word, and this kernel
// is then the most expensive of the sample (13 ms at n = 2^20, DESIGN section 16, which also names the remedy).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MD_BLOCK)
    k_cl_flatten(int n, const int32_t *__restrict__ id, const uint32_t *__restrict__ parent, uint32_t *__restrict__ root,
                 int32_t *__restrict__ count, int32_t *__restrict__ minid)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t x = parent[k];
    if (x == CL_NONE) {
        root[k] = CL_NONE;
        return;
    }
    for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
    root[k] = x;
    atomicAdd(&count[x], 1);
    atomicMin(&minid[x], id[k]);
}

// ------------------------------------------------------------------------------------------
// One lane per slot, roots only.  hist[min(s, max_size)] += 1;  part[c * nblk + bid], c = 0..3: members (the sum of the
// sizes), clusters, sum s^2, size-1 clusters; 4, 5: the block's largest and second-largest key (size << 32 | ~label):
// a larger key is a larger cluster or, at equal size, a smaller label.  Labels differ, so keys differ; 0 = none.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MD_BLOCK)
    k_cl_stats(int n, const uint32_t *__restrict__ root, const int32_t *__restrict__ count, const int32_t *__restrict__ minid,
               int max_size, cl_u64 *__restrict__ hist, int nblk, cl_u64 *__restrict__ part)
{
    __shared__ cl_u64 red[16];
    __shared__ cl_u64 top[2];
    __shared__ unsigned hl[MD_CL_LDS_SIZE + 1];
    const bool lds_hist = max_size <= MD_CL_LDS_SIZE;
    if (lds_hist)
        for (int i = threadIdx.x; i <= max_size; i += blockDim.x) hl[i] = 0u;
    if (threadIdx.x < 2) top[threadIdx.x] = 0ull;
    __syncthreads();
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    cl_u64 size = 0, key = 0;
    if (k < n && root[k] == (uint32_t)k) {
        size = (cl_u64)count[k];
        key = (size << 32) | (cl_u64)(~(uint32_t)minid[k]);
        const int b = size > (cl_u64)max_size ? max_size : (int)size;
        if (lds_hist)
            atomicAdd(&hl[b], 1u);
        else
            atomicAdd(&hist[b], 1ull);
        atomicMax(&top[0], key);
    }
    __syncthreads();
    if (key != 0 && key != top[0]) atomicMax(&top[1], key);
    if (lds_hist)
        for (int i = threadIdx.x; i <= max_size; i += blockDim.x) {
            unsigned c = hl[i];
            if (c) atomicAdd(&hist[i], (cl_u64)c);
        }
    const cl_u64 v[4] = {size, size ? 1ull : 0ull, size * size, size == 1 ? 1ull : 0ull};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        cl_u64 t = cl_block_sum(v[c], red);
        if (threadIdx.x == 0) part[(size_t)c * nblk + blockIdx.x] = t;
    }
    // (cl_block_sum's barriers order the atomicMax on top[1] before this read)
    if (threadIdx.x == 0) {
        part[(size_t)4 * nblk + blockIdx.x] = top[0];
        part[(size_t)5 * nblk + blockIdx.x] = top[1];
    }
}

// ------------------------------------------------------------------------------------------
// One block: fr[0..7] = members, clusters, largest, second largest, directed bonds, sum s^2, label of the largest (-1 if
// none), size-1 clusters.  sum_fr += fr, series[m] = fr when m < nseries; m is counted by the host.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
    k_cl_finish(int nblk, const cl_u64 *__restrict__ part, int ndeg, const cl_u64 *__restrict__ deg_part, long long m,
                long long nseries, long long *__restrict__ sum_fr, long long *__restrict__ series)
{
    __shared__ cl_u64 red[16];
    __shared__ cl_u64 top[2];
    if (threadIdx.x < 2) top[threadIdx.x] = 0ull;
    cl_u64 t[5];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        cl_u64 a = 0;
        for (int i = threadIdx.x; i < nblk; i += blockDim.x) a += part[(size_t)c * nblk + i];
        t[c] = cl_block_sum(a, red);
    }
    {
        cl_u64 a = 0;
        for (int i = threadIdx.x; i < ndeg; i += blockDim.x) a += deg_part[i];
        t[4] = cl_block_sum(a, red);
    }
    // the two largest keys of the 2 nblk block keys: this thread's two, then the block's
    cl_u64 k1 = 0, k2 = 0;
    for (int i = threadIdx.x; i < 2 * nblk; i += blockDim.x) {
        const cl_u64 key = part[(size_t)4 * nblk + i];
        if (key > k1) {
            k2 = k1;
            k1 = key;
        } else if (key > k2) {
            k2 = key;
        }
    }
    if (k1) atomicMax(&top[0], k1);
    __syncthreads();
    const cl_u64 mine = (k1 == top[0]) ? k2 : k1;
    if (mine) atomicMax(&top[1], mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long fr[MD_CL_NFR];
    fr[0] = (long long)t[0];
    fr[1] = (long long)t[1];
    fr[2] = (long long)(top[0] >> 32);
    fr[3] = (long long)(top[1] >> 32);
    fr[4] = (long long)t[4];
    fr[5] = (long long)t[2];
    fr[6] = top[0] ? (long long)(~(uint32_t)top[0]) : -1ll;
    fr[7] = (long long)t[3];
#pragma unroll
    for (int c = 0; c < MD_CL_NFR; ++c) {
        sum_fr[c] = sum_fr[c] + fr[c];
        if (m < nseries) series[(size_t)m * MD_CL_NFR + c] = fr[c];
    }
}

// Slot order -> particle-id order for md_cluster_particles.  `id` is the sampler's copy of the permutation taken with the
// sample: the handle's own changes at every list build.
__global__ void __launch_bounds__(MD_BLOCK)
    k_cl_export(int n, const int32_t *__restrict__ id, const uint32_t *__restrict__ root, const int32_t *__restrict__ count,
                const int32_t *__restrict__ minid, int32_t *__restrict__ o_label, int32_t *__restrict__ o_size)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t o = (size_t)id[k];
    const uint32_t r = root[k];
    o_label[o] = r == CL_NONE ? -1 : minid[r];
    o_size[o] = r == CL_NONE ? 0 : count[r];
}
