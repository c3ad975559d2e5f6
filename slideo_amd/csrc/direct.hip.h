// direct.hip.h — kernels of the direct page look-up (stage_direct.hip; include/slideo_amd.h "Direct page look-up").  The frames' and
// pages' centred operands and the table of their dot products are the SSD-table engine's (ssd_table.hip.h, stage_ssd_table.hip).
//
//   direct_best_kernel    per frame: ssd(p) = |a'|^2 + |b'|^2 - 2 <a', b'> over the eligible pages, the smallest one and the
//                         lowest page that attains it (the tap: every page's ssd)
//   direct_gate_kernel    one block, behind gate_kernel: the direct frames leave the kept list, the unit's pinned record grows
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slideo {

constexpr int DIRECT_BLOCK = 256;

struct DirectBest { unsigned long long ssd; int32_t page; int32_t _pad; };

// What direct_gate_kernel appends to a gated unit's pinned record (at `rec`, 8-byte aligned behind gate_kernel's): the reduced
// kept count, then per frame the best SSD (u64), its page (i32) and the direct flag (u8; 1 only for a changed frame).
struct DirectHostRec { uint32_t kept, n; };
inline __host__ __device__ size_t direct_rec_ssd_ofs() { return 8; }
inline __host__ __device__ size_t direct_rec_page_ofs(int n) { return 8 + (size_t)n * 8; }
inline __host__ __device__ size_t direct_rec_flag_ofs(int n) { return 8 + (size_t)n * 12; }
inline __host__ __device__ size_t direct_rec_bytes(int n) { return 8 + (size_t)n * 13; }

// Frame blockIdx.x (grid n, block 256): ssd(c) = anorm + bnorm[c] - 2 dot[c] for the class positions c = elig[0 .. ne) (ascending,
// so ascending deck pages = pages[c]); best[frame] = the smallest and the lowest page with it (UINT64_MAX, -1 when ne == 0).
// ssd_out (the tap; null in the gated path): ssd_out[frame * ssd_pitch + pages[c]] = ssd(c).
__global__ __launch_bounds__(DIRECT_BLOCK) void direct_best_kernel(const unsigned long long* __restrict__ dot, int np, const long long* __restrict__ anorm,
                                                                   const long long* __restrict__ bnorm, const int32_t* __restrict__ pages,
                                                                   const int32_t* __restrict__ elig, int ne, DirectBest* __restrict__ best,
                                                                   unsigned long long* __restrict__ ssd_out, int ssd_pitch) {
    __shared__ unsigned long long rs[DIRECT_BLOCK / 64];
    __shared__ int32_t rc[DIRECT_BLOCK / 64];
    const int f = blockIdx.x;
    const long long an = anorm[f];
    unsigned long long bs = ~0ull;
    int32_t bc = 0x7FFFFFFF;
    for (int e = threadIdx.x; e < ne; e += DIRECT_BLOCK) {             // (a thread's own e ascend: < keeps its first minimum)
        const int32_t c = elig[e];
        const unsigned long long s = (unsigned long long)(an + bnorm[c] - 2ll * (long long)dot[(size_t)f * np + c]);
        if (ssd_out) ssd_out[(size_t)f * ssd_pitch + pages[c]] = s;
        if (s < bs) { bs = s; bc = c; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long os = __shfl_xor(bs, d);
        const int32_t oc = __shfl_xor(bc, d);
        if (os < bs || (os == bs && oc < bc)) { bs = os; bc = oc; }
    }
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = bs; rc[threadIdx.x >> 6] = bc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < DIRECT_BLOCK / 64; ++k)
            if (rs[k] < bs || (rs[k] == bs && rc[k] < bc)) { bs = rs[k]; bc = rc[k]; }
        DirectBest r;
        r.ssd = bs; r.page = ne > 0 ? pages[bc] : -1; r._pad = 0;
        best[f] = r;
    }
}

// One block, behind gate_kernel on the unit's stream.  Frame j of the kept list idx[0 .. *count) is DIRECT iff
// best[j].ssd <= thr (slideo_direct_ssd_threshold, in 64-bit integers; thr < 0: never).  The direct frames leave the list in
// place — the rest keeps its ascending order: a wave-ballot prefix scan per chunk of DIRECT_BLOCK entries, the waves' totals
// through LDS, the carry from chunk to chunk; every entry of a chunk is read before any is written, and an entry is written at or
// below where it was read — and *count and the pinned record's list h_idx follow.  rec (pinned, direct_rec_*): the reduced
// count, then best SSD, page and direct flag of all n frames.  Ordinary vector stores throughout.
__global__ __launch_bounds__(DIRECT_BLOCK) void direct_gate_kernel(const DirectBest* __restrict__ best, int n, long long thr,
                                                                   int32_t* __restrict__ idx, uint32_t* __restrict__ count, int32_t* __restrict__ h_idx,
                                                                   uint8_t* __restrict__ rec) {
    __shared__ uint32_t wtot[DIRECT_BLOCK / 64];
    __shared__ uint32_t carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long* h_ssd = reinterpret_cast<unsigned long long*>(rec + direct_rec_ssd_ofs());
    int32_t* h_page = reinterpret_cast<int32_t*>(rec + direct_rec_page_ofs(n));
    uint8_t* h_flag = rec + direct_rec_flag_ofs(n);
    const uint32_t k = *count;
    if (threadIdx.x == 0) carry = 0;
    for (int i = threadIdx.x; i < n; i += DIRECT_BLOCK) {
        const DirectBest b = best[i];
        h_ssd[i] = b.ssd; h_page[i] = b.page; h_flag[i] = 0;
    }
    __syncthreads();                                                   // (count is read by all, the flags are cleared)
    for (uint32_t base = 0; base < k; base += DIRECT_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        int32_t j = -1;
        bool keep = false, direct = false;
        if (i < k) {
            j = idx[i];
            direct = thr >= 0 && best[j].ssd <= (unsigned long long)thr;
            keep = !direct;
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wtot[w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t ofs = carry, all = 0;
        for (int q = 0; q < DIRECT_BLOCK / 64; ++q) { if (q < w) ofs += wtot[q]; all += wtot[q]; }
        if (direct) h_flag[j] = 1;
        if (keep) {
            const uint32_t r = ofs + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            idx[r] = j; h_idx[r] = j;
        }
        __syncthreads();                                               // (every thread has read carry and wtot)
        if (threadIdx.x == 0) carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *count = carry;
        DirectHostRec r{carry, (uint32_t)n};
        *reinterpret_cast<DirectHostRec*>(rec) = r;
    }
}

}  // namespace slideo
