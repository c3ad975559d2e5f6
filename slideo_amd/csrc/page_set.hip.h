// page_set.hip.h — kernels that build a page set's search operand from the finalized deck (stage_page_set.hip).
//
// The deck's distinct rows, their duplicate chains (d_grp_next) and their norm order before the tile shuffle are the input; the
// output is what prepare_train_bits (stage_knn.hip) writes for a deck of exactly the selected pages: the set's own chains, its
// distinct rows in norm order (a stable compaction of the deck's), and per operand row its source row, norm and key row id.
#pragma once
#include "common.h"

namespace slideo {

constexpr int PS_BLOCK = 256;
constexpr int PS_SCAN_BLOCK = 1024;

// Mark + regroup.  Per distinct row u of the deck (head row urow[u]; urow null: u itself) walk its chain (rows ascend along it):
// the rows of selected pages (in_set[train_page[row]]) are linked into the set's chain (set_next, which the caller has cleared
// to -1), the first of them becomes the group's head in the set (set_head[u]; -1: no selected row, the group drops out).
__global__ __launch_bounds__(PS_BLOCK) void ps_regroup_kernel(const int32_t* __restrict__ urow, int nu, const int32_t* __restrict__ grp_next,
                                                              const int32_t* __restrict__ train_page, const uint8_t* __restrict__ in_set,
                                                              int32_t* __restrict__ set_head, int32_t* __restrict__ set_next) {
    const int u = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (u >= nu) return;
    int32_t head = -1, prev = -1;
    for (int32_t r = urow ? urow[u] : u; r >= 0; r = grp_next[r]) {
        if (!in_set[train_page[r]]) continue;
        if (prev >= 0) set_next[prev] = r;
        else head = r;
        prev = r;
    }
    set_head[u] = head;
}

// Compaction of the norm order uorder[0 .. nu) to the groups that survive, pass 1: survivors per block (wave ballots).
__global__ __launch_bounds__(PS_BLOCK) void ps_count_kernel(const int32_t* __restrict__ uorder, int nu, const int32_t* __restrict__ set_head,
                                                            uint32_t* __restrict__ block_cnt) {
    __shared__ uint32_t wsum[PS_BLOCK / 64];
    const int i = blockIdx.x * PS_BLOCK + threadIdx.x;
    const bool keep = i < nu && set_head[uorder[i]] >= 0;
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < PS_BLOCK / 64; ++w) t += wsum[w];
        block_cnt[blockIdx.x] = t;
    }
}

// Pass 2 (one block): the block counts [0, n) become exclusive offsets in place; *total = the survivors.
__global__ __launch_bounds__(PS_SCAN_BLOCK) void ps_scan_kernel(uint32_t* __restrict__ cnt, int n, uint32_t* __restrict__ total) {
    __shared__ uint32_t wtot[PS_SCAN_BLOCK / 64];
    __shared__ uint32_t carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += PS_SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < n ? cnt[i] : 0u;
        uint32_t x = v;                                                   // inclusive scan within the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wtot[w] = x;
        __syncthreads();
        uint32_t wofs = 0;
        for (int k = 0; k < w; ++k) wofs += wtot[k];
        const uint32_t c = carry;
        if (i < n) cnt[i] = c + wofs + x - v;
        __syncthreads();                                                  // (every lane has read carry and wtot)
        if (threadIdx.x == PS_SCAN_BLOCK - 1) carry = c + wofs + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// Pass 3: the survivors to cu[block offset + rank], in norm order (ties keep the deck's order).
__global__ __launch_bounds__(PS_BLOCK) void ps_scatter_kernel(const int32_t* __restrict__ uorder, int nu, const int32_t* __restrict__ set_head,
                                                              const uint32_t* __restrict__ block_ofs, int32_t* __restrict__ cu) {
    __shared__ uint32_t wsum[PS_BLOCK / 64];
    const int i = blockIdx.x * PS_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t u = i < nu ? uorder[i] : -1;
    const bool keep = u >= 0 && set_head[u] >= 0;
    const unsigned long long b = __ballot(keep);
    if (lane == 0) wsum[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t ofs = block_ofs[blockIdx.x];
    for (int k = 0; k < w; ++k) ofs += wsum[k];
    if (keep) cu[ofs + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = u;
}

// Lay out: operand row r (< nt_pad) holds position order[r / 32] * 32 + r % 32 of the compacted list (the host's tile shuffle;
// past ns, and past the last tile, a pad row).  perm[r] = its distinct row (the source of the FP4 expansion), the side array
// its norm (f32 bits) and the key row id (the set's head row: a deck row id), pad rows KT_PAD_NORM / -1; nminh per 32-row tile
// half the norm of its first row.  t: the distinct rows, packed [nu][8].
__global__ __launch_bounds__(PS_BLOCK) void ps_layout_kernel(const int32_t* __restrict__ cu, int ns, const int32_t* __restrict__ tile_order,
                                                             int nt_pad, const uint32_t* __restrict__ t, const int32_t* __restrict__ set_head,
                                                             int st_rows, int side_u32, float pad_norm, int32_t* __restrict__ perm,
                                                             uint32_t* __restrict__ side, float* __restrict__ nminh) {
    const int r = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (r >= nt_pad) return;
    int32_t u = -1;
    if (r < (ns + 31) / 32 * 32) {
        const int p = tile_order[r >> 5] * 32 + (r & 31);
        if (p < ns) u = cu[p];
    }
    float nf = pad_norm;
    uint32_t rid = 0xFFFFFFFFu;
    if (u >= 0) {
        const uint4* row = reinterpret_cast<const uint4*>(t + (size_t)u * 8);
        const uint4 a = row[0], c = row[1];
        nf = (float)(__popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(c.x) + __popc(c.y) + __popc(c.z) + __popc(c.w));
        rid = (uint32_t)set_head[u];
    }
    perm[r] = u;
    side[(size_t)(r / st_rows) * side_u32 + (r % st_rows)] = __float_as_uint(nf);
    side[(size_t)(r / st_rows) * side_u32 + st_rows + (r % st_rows)] = rid;
    if ((r & 31) == 0) nminh[r >> 5] = 0.5f * nf;
}

}  // namespace slideo
