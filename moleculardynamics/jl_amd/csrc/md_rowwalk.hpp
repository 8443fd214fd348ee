// md_rowwalk.hpp -- one lane per particle walks its OUTER Verlet row: the kernel pair every neighbour sampler shares (bond
// order passes 1 and 2 in md_boo.hpp, the cluster hooks in md_cluster.hpp, the cage origin in md_cage.hpp).
//
//   k_rows_tile<D, RS, Lane>   tiled handle: stages the tile's halo as 32-byte records {x, y, z, owner slot} (k_stress_tile's
//                              prologue), then every lane walks its row of 16-bit offsets into the force kernel's image
//   k_rows<D, Lane>            handle whose rows are 32-bit global slots (k_stress's walk)
// Both: block bid (XCD-remapped) serves the slots k = bid * 256 + thread.  A lane with k >= n is INACTIVE: it walks the row
// of kk = n - 1 like everyone else (the barriers need it) and must write nothing of its own.
//
// Lane contract.  A pass is a struct Lane with a plain `Args` type (the kernel's third argument, by value) and
//   begin(args, state, k, kk, active, pi)           once, after the staging; pi = state.pos[kk]
//   visit(args, state, hit, dx, dy, dz, d2, own)    once per row entry, in row order, padding and sentinel included:
//                                                   del = x_j(+translation) - x_i as the force kernels form it, d2 =
//                                                   d2_ref(del), hit = d2 < r2 with r2 the pass's own radius.  own is
//                                                   j's OWNER slot (< n; a ghost is resolved through gowner) and means
//                                                   something only when hit
//   end(args, k, active, bid)                       once; EVERY thread of the block calls it, so it may use barriers and
//                                                   static __shared__ storage
// Everything fp64.  The walk itself has no reduction and no atomics; what a lane does with its entries is its own.
#pragma once
#include "md_kernels.hpp"

// The rows address the force kernel's LDS image with 16-bit byte offsets: the list builders accept a tile only if
// (H + 1) * stride <= MD_ROW_OFFSET_MAX, stride 24 or 32 (launch_rows checks exactly that on the handle).  The walk's own
// image, 32 bytes per record, then stays below the dynamic LDS the force kernel itself may use.
#define MD_ROW_OFFSET_MAX 65535
#define MD_ROW_LDS_LIMIT (150 * 1024)
static_assert((MD_ROW_OFFSET_MAX / 24) * 32 + 16 <= MD_ROW_LDS_LIMIT && (MD_ROW_OFFSET_MAX / 32) * 32 + 16 <= MD_ROW_LDS_LIMIT,
              "the walk's 32-byte image of any tile the builders accept must fit the force kernel's LDS limit");

// The image has 32-byte records whatever the force kernel's stride is: (H + 1) * 32 <= 87360 bytes for a 24-byte handle
// and 65536 for a 32-byte one, so it always fits and a tiled handle never needs another walk.
inline size_t row_image_bytes(int max_halo) { return (((size_t)max_halo + 1) * 32 + 15) & ~(size_t)15; }
inline bool row_image_fits(int max_halo) { return row_image_bytes(max_halo) <= (size_t)MD_ROW_LDS_LIMIT; }

// The list as the two kernels read it
struct RowsTile {
    int n;
    DevState s;
    const uint16_t *nlist16;
    int maxn;
    const int32_t *nmax_tile;
    const uint32_t *halo;
    int hcap;
    const int32_t *halo_count, *gowner;
};

struct RowsGlobal {
    int n;
    DevState s;
    const uint32_t *nlist;
    int maxn;
    const int32_t *nmax_tile, *gowner;
};

// ------------------------------------------------------------------------------------------
// The two walks.  f(hit, dx, dy, dz, d2, owner) is called once per row entry, in row order.
// ------------------------------------------------------------------------------------------

// Stage the tile's halo (k_stress_tile's prologue) as 32-byte records {x, y, z, owner slot}: the owner is the halo word's
// low 26 bits, resolved through gowner for a handle whose ghosts are real slots.  Record H is the sentinel.
template <int D>
__device__ __forceinline__ void row_stage(unsigned char *smem, int n, const DevState &s, const uint32_t *__restrict__ hl,
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
__device__ __forceinline__ void row_walk_tile(const unsigned char *smem, const ushort4 *row4, int m, const double4 &pi,
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
__device__ __forceinline__ void row_walk_global(int n, const DevState &s, const uint32_t *row, int m, const double4 &pi,
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
// The two kernels
// ------------------------------------------------------------------------------------------
template <int D, int RS, class Lane>
__global__ void __launch_bounds__(MD_TILE)
    k_rows_tile(RowsTile R, double r2, typename Lane::Args A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int k = bid * MD_TILE + threadIdx.x;
    bool active = k < R.n;
    int kk = active ? k : R.n - 1;
    int lane = threadIdx.x & 63;
    int wt = bid * (MD_TILE / 64) + (threadIdx.x >> 6);
    const ushort4 *row4 = (const ushort4 *)(R.nlist16 + ((size_t)wt * R.maxn) * 64) + lane;
    const int m = __builtin_amdgcn_readfirstlane(R.nmax_tile[wt]);
    double4 pi = R.s.pos[kk];
    row_stage<D>(smem, R.n, R.s, R.halo + (size_t)bid * R.hcap, R.halo_count[bid], R.gowner);
    Lane ln;
    ln.begin(A, R.s, k, kk, active, pi);
    row_walk_tile<D, RS>(smem, row4, m, pi, r2, [&](bool hit, double dx, double dy, double dz, double d2, uint32_t own) {
        ln.visit(A, R.s, hit, dx, dy, dz, d2, own);
    });
    ln.end(A, k, active, bid);
}

template <int D, class Lane>
__global__ void __launch_bounds__(MD_BLOCK)
    k_rows(RowsGlobal R, double r2, typename Lane::Args A)
{
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    int k = bid * MD_BLOCK + threadIdx.x;
    bool active = k < R.n;
    int kk = active ? k : R.n - 1;
    int lane = threadIdx.x & 63;
    int tile = kk >> 6;
    const uint32_t *row = R.nlist + ((size_t)tile * R.maxn) * 64 + lane;
    int m = R.nmax_tile[tile];
    double4 pi = R.s.pos[kk];
    Lane ln;
    ln.begin(A, R.s, k, kk, active, pi);
    row_walk_global<D>(R.n, R.s, row, m, pi, r2, R.gowner, [&](bool hit, double dx, double dy, double dz, double d2, uint32_t own) {
        ln.visit(A, R.s, hit, dx, dy, dz, d2, own);
    });
    ln.end(A, k, active, bid);
}
