// frame_mask.hip.h — kernels of the frame detection mask (stage_orb.hip; include/slideo_amd.h "Frame mask").
//
//   mask_threshold_kernel  one level of the mask pyramid after its resize: threshold(254, THRESH_TOZERO) in place (set time)
//   mask_filter_kernel     per unit, between fast_kernel and threshold_kernel: a (frame, level)'s FAST candidates whose mask byte is 0
//                          leave the candidate list; the level's score histogram and count are rebuilt from the survivors
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geom.h"

namespace slideo {

constexpr int MASK_BLOCK = 256;

// v > 254 ? v : 0 over the w x h bytes of level L of the one-frame mask pyramid.  grid ceil(w * h / 256).
__global__ __launch_bounds__(MASK_BLOCK) void mask_threshold_kernel(uint8_t* __restrict__ pyr, LevelGeom L) {
    const uint32_t i = blockIdx.x * MASK_BLOCK + threadIdx.x;
    if (i >= (uint32_t)L.w * (uint32_t)L.h) return;
    const uint32_t y = i / (uint32_t)L.w, x = i - y * (uint32_t)L.w;
    uint8_t* p = pyr + L.ofs + (size_t)y * L.pitch + x;
    const uint8_t v = *p;
    *p = v > 254 ? v : 0;
}

// grid (nlevels, B), block 256.  The level's candidate list (score << 24 | y << 12 | x, in level coordinates: fast_kernel) is
// walked in chunks of 256: a chunk is read into registers, the mask byte at (y, x) of the mask pyramid (the image pyramid's own
// level layout, one frame) decides, and the survivors are written back IN PLACE behind those of the earlier chunks — a wave-ballot
// prefix, the waves' totals through LDS, the earlier chunks' total carried.  The carried offset never passes the chunk's first
// entry and the barrier between the chunk's reads and its writes orders them, so no entry is overwritten before it was read.  The
// survivors' scores are counted into an LDS histogram, which replaces the level's 256 bins; cand_count becomes the survivors'.
// Nothing returns from a global atomic and nothing is kept per thread beyond one entry.
__global__ __launch_bounds__(MASK_BLOCK) void mask_filter_kernel(PyrGeom g, const uint8_t* __restrict__ mask_pyr, uint32_t* __restrict__ cand,
                                                                 uint32_t* __restrict__ cand_count, uint32_t* __restrict__ hist) {
    __shared__ uint32_t shist[256];
    __shared__ uint32_t wtot[MASK_BLOCK / 64];
    __shared__ uint32_t carry;
    const int l = blockIdx.x, f = blockIdx.y;
    const LevelGeom L = g.lv[l];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t fl = (size_t)f * g.nlevels + l;
    const uint32_t total = cand_count[fl];
    const uint32_t n = min(total, (uint32_t)L.cand_cap);
    uint32_t* clist = cand + (size_t)f * g.cand_per_frame + L.cand_ofs;
    const uint8_t* mlevel = mask_pyr + L.ofs;
    shist[threadIdx.x] = 0;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += MASK_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        uint32_t e = 0;
        bool keep = false;
        if (i < n) {
            e = clist[i];
            const uint32_t x = e & 0xFFFu, y = (e >> 12) & 0xFFFu;
            // (a candidate lies inside the level's keep-region, so (y, x) is inside the level; the test keeps a damaged entry from
            // reading beyond the mask)
            keep = x < (uint32_t)L.w && y < (uint32_t)L.h && mlevel[y * (uint32_t)L.pitch + x] != 0;
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wtot[w] = (uint32_t)__popcll(b);
        __syncthreads();                                               // (the whole chunk is in registers)
        uint32_t ofs = carry, all = 0;
        for (int k = 0; k < MASK_BLOCK / 64; ++k) { if (k < w) ofs += wtot[k]; all += wtot[k]; }
        if (keep) {
            clist[ofs + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = e;
            atomicAdd(&shist[e >> 24], 1u);                            // LDS, nothing returned
        }
        __syncthreads();                                               // (every thread has read carry and wtot)
        if (threadIdx.x == 0) carry += all;
        __syncthreads();
    }
    hist[fl * 256 + threadIdx.x] = shist[threadIdx.x];
    // (a list that overflowed keeps its count: threshold_kernel raises the overflow flag from it)
    if (threadIdx.x == 0 && total <= (uint32_t)L.cand_cap) cand_count[fl] = carry;
}

}  // namespace slideo
