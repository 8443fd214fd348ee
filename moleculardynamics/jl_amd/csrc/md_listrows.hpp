// md_listrows.hpp -- read-only read-back of the Verlet rows for md_list_rows (instrumentation): every row entry the force
// kernels would walk, decoded to (id_i, id_j, periodic image) from whatever the build path stored, and x0 / x1 / pos by
// particle id.  Nothing here writes to the handle's state, and no kernel of the product calls into this file.
//
// One thread per owned slot k walks its row r = 0 .. rowlen[k >> 6] - 1 (the wave-padded length the force kernels use):
//   16-bit rows   rows16[wave base + row_off(r, lane)] = byte offset of a record in the tile's LDS image; record number
//                 h = offset / rs indexes the tile's halo list (halo, or halo_in for inner rows written with an inner
//                 halo); h == halo_count[tile] is the sentinel record (padding), not an entry.  A halo word is
//                 slot (26 bits) | shift code (6 bits).
//   32-bit rows   rows32[wave base + lane + r * 64] = global slot; `sentinel32` (the capacity) is padding.
// A slot >= n is a real ghost copy: owner and shift code come from the ghost tables.  The shift code (2 bits per lattice
// direction, 1 = +, 2 = -: shift_xyz) is reported as the image vector n of "the record the pair loop reads is
// x_j + n . A".  What cannot be decoded is still reported, with id_j = -1 (record number past the sentinel or the halo
// capacity, offset that is no multiple of the stride, slot past the ghosts) or an image component of 2 (shift field 3),
// so that a checker sees it: an entry is never dropped silently.
// k_listrows<false> counts a slot's entries, k_listrows<true> writes them at the slot's offset (exclusive scan of the
// counts, in slot order) in row order.
#pragma once
#include "md_kernels.hpp"

struct ListRowsView {
    int n;                 // owned slots
    int nghost;            // real ghost slots [n, n + nghost)
    const int32_t *id;     // slot -> particle id
    const uint16_t *rows16; // 16-bit rows, or null: rows32
    const uint32_t *rows32;
    int maxn;              // row capacity (entries per lane)
    const int32_t *rowlen; // per wave of 64 slots: the padded row length
    int rs;                // LDS record stride of the 16-bit offsets
    const uint32_t *halo;
    int hcap;
    const int32_t *halo_count;
    uint32_t sentinel32;
    const int32_t *gowner;
    const uint32_t *gcode;
};

__device__ __forceinline__ int listrows_image(uint32_t field) { return field == 1u ? 1 : (field == 2u ? -1 : (field == 0u ? 0 : 2)); }

template <bool FILL>
__global__ void __launch_bounds__(MD_BLOCK)
    k_listrows(ListRowsView V, int32_t *__restrict__ counts, const int64_t *__restrict__ offsets, int32_t *__restrict__ out,
               long long cap)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V.n) return;
    const int lane = k & 63, wave = k >> 6, tile = k / MD_TILE;
    const size_t wbase = ((size_t)wave * V.maxn) * 64;
    int m = V.rowlen[wave];
    m = m < 0 ? 0 : (m > V.maxn ? V.maxn : m);
    const int H = V.rows16 ? V.halo_count[tile] : 0;
    const uint32_t *hl = V.rows16 ? V.halo + (size_t)tile * V.hcap : nullptr;
    const int idi = V.id[k];
    long long p = FILL ? (long long)offsets[k] : 0;
    int cnt = 0;
    for (int r = 0; r < m; ++r) {
        uint32_t slot, code = 0u;
        bool bad = false;
        if (V.rows16) {
            const unsigned off = V.rows16[wbase + row_off(r, lane)];
            const unsigned h = off / (unsigned)V.rs;
            if (off == (unsigned)H * (unsigned)V.rs) continue; // the sentinel record: padding
            bad = (off % (unsigned)V.rs) != 0u || h > (unsigned)H || h >= (unsigned)V.hcap;
            const uint32_t w = bad ? 0u : hl[h];
            slot = w & 0x3ffffffu;
            code = w >> 26;
        } else {
            slot = V.rows32[wbase + lane + (size_t)r * 64];
            if (slot == V.sentinel32) continue;
        }
        if (!bad && slot >= (uint32_t)V.n) {
            const uint32_t gi = slot - (uint32_t)V.n;
            bad = gi >= (uint32_t)V.nghost;
            if (!bad) {
                code = V.gcode[gi];
                slot = (uint32_t)V.gowner[gi];
                bad = slot >= (uint32_t)V.n;
            }
        }
        if constexpr (FILL) {
            if (p < cap) {
                int32_t *e = out + (size_t)p * 5;
                e[0] = idi;
                e[1] = bad ? -1 : V.id[slot];
                e[2] = listrows_image(code & 3u);
                e[3] = listrows_image((code >> 2) & 3u);
                e[4] = listrows_image((code >> 4) & 3u);
            }
            ++p;
        }
        ++cnt;
    }
    if constexpr (!FILL) counts[k] = cnt;
}

// x0, x1 and the current positions by particle id, n x D each, in the handle's own unwrapped frame
template <int D>
__global__ void __launch_bounds__(MD_BLOCK)
    k_listrows_positions(int n, DevState s, double *__restrict__ x0, double *__restrict__ x1, double *__restrict__ pos)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t o = (size_t)s.id[k] * D;
    const double4 p = s.pos[k];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        x0[o + c] = s.x0[c][k];
        x1[o + c] = s.x1[c][k];
        pos[o + c] = pos_get(p, c);
    }
}
