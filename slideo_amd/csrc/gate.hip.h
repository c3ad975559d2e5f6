// gate.hip.h — kernels of the changed-frame gate (stage_gate.hip; include/slideo_amd.h "Changed-frame gate").
//
//   gate_kernel           the unit's n SSDs against the integer threshold T -> flags, the ascending list of kept frames, their count
//   gather_frames_kernel  the kept frames packed back to back (a pure copy)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slideo {

constexpr int GATE_BLOCK = 256;
constexpr int GATHER_BLOCK = 256;

// What a gated unit's host side reads at its mid-submit wait and at collect (pinned, written by gate_kernel): the kept count, then
// n SSDs (u64), n kept indices (i32, the first `count` are valid, ascending) and n flags (u8).
struct GateHostRec { uint32_t count, n; };
inline __host__ __device__ size_t gate_rec_ssd_ofs() { return 8; }
inline __host__ __device__ size_t gate_rec_idx_ofs(int n) { return 8 + (size_t)n * 8; }
inline __host__ __device__ size_t gate_rec_flag_ofs(int n) { return 8 + (size_t)n * 12; }
inline __host__ __device__ size_t gate_rec_bytes(int n) { return 8 + (size_t)n * 13; }

// One block.  changed[i] = force0 && i == 0 (no gate state: video_capture.rs:92) || ssd[i] >= thr, in 64-bit integers
// (thr = slideo_changed_ssd_threshold; INT64_MAX: never).  idx[0 .. count) = the changed frames, ascending: a wave-ballot prefix
// scan, the waves' totals through LDS, chunks of GATE_BLOCK frames carried.  Everything is written twice with ordinary vector
// stores: to device memory (gather_frames_kernel reads idx) and to the slot's pinned record `host`.
__global__ __launch_bounds__(GATE_BLOCK) void gate_kernel(const unsigned long long* __restrict__ ssd, int n, long long thr, int force0,
                                                           uint8_t* __restrict__ flags, int32_t* __restrict__ idx, uint32_t* __restrict__ count,
                                                           uint8_t* __restrict__ host) {
    __shared__ uint32_t wtot[GATE_BLOCK / 64];
    __shared__ uint32_t carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long* h_ssd = reinterpret_cast<unsigned long long*>(host + gate_rec_ssd_ofs());
    int32_t* h_idx = reinterpret_cast<int32_t*>(host + gate_rec_idx_ofs(n));
    uint8_t* h_flag = host + gate_rec_flag_ofs(n);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += GATE_BLOCK) {
        const int i = base + threadIdx.x;
        unsigned long long s = 0;
        bool keep = false;
        if (i < n) {
            s = (force0 && i == 0) ? 0ull : ssd[i];
            keep = (force0 && i == 0) || (long long)s >= thr;          // (an SSD is at most 255^2 * 3 * sw * sh: far inside int64)
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wtot[w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t ofs = carry, all = 0;
        for (int k = 0; k < GATE_BLOCK / 64; ++k) { if (k < w) ofs += wtot[k]; all += wtot[k]; }
        if (i < n) {
            flags[i] = keep ? 1 : 0; h_flag[i] = keep ? 1 : 0;
            h_ssd[i] = s;
            if (keep) {
                const uint32_t r = ofs + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
                idx[r] = i; h_idx[r] = i;
            }
        }
        __syncthreads();                                               // (every thread has read carry and wtot)
        if (threadIdx.x == 0) carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *count = carry;
        GateHostRec r{carry, (uint32_t)n};
        *reinterpret_cast<GateHostRec*>(host) = r;
    }
}

// Frame idx[blockIdx.y] of src (rows `stride` apart, frames `frame_stride` apart: caller memory, any alignment) -> frame blockIdx.y
// of dst, packed: rows row_bytes apart, frames h * row_bytes apart.  The frame is cut into nseg segments of seg_bytes that are
// contiguous on both sides: the whole frame when stride == row_bytes, its rows otherwise.  bps blocks share a segment (gridDim.x is
// a multiple of bps; the groups of bps blocks stride over the segments).  Per segment: bytes up to the destination's first
// 16-byte boundary, 16-byte loads and stores where the source is aligned there too (4-byte ones where it is only 4-byte aligned,
// bytes otherwise), bytes at the ragged end.  No LDS.
__global__ __launch_bounds__(GATHER_BLOCK) void gather_frames_kernel(const uint8_t* __restrict__ src, int64_t frame_stride, int stride,
                                                                     const int32_t* __restrict__ idx, int64_t seg_bytes, int nseg, int bps,
                                                                     uint8_t* __restrict__ dst) {
    const int part = blockIdx.x % bps, seg_step = gridDim.x / bps;
    const uint8_t* sf = src + (int64_t)idx[blockIdx.y] * frame_stride;
    uint8_t* df = dst + (int64_t)blockIdx.y * seg_bytes * nseg;
    const int64_t t = (int64_t)part * GATHER_BLOCK + threadIdx.x, nt = (int64_t)bps * GATHER_BLOCK;
    for (int seg = blockIdx.x / bps; seg < nseg; seg += seg_step) {
        const uint8_t* s = sf + (int64_t)seg * stride;
        uint8_t* d = df + (int64_t)seg * seg_bytes;
        int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15);
        if (head > seg_bytes) head = seg_bytes;
        const uintptr_t sa = reinterpret_cast<uintptr_t>(s + head);
        const int vec = (sa & 15) == 0 ? 16 : (sa & 3) == 0 ? 4 : 1;
        const int64_t body = vec == 1 ? 0 : (seg_bytes - head) / vec;      // vector elements
        const int64_t tail0 = head + body * vec;
        if (vec == 16) {
            const uint4* s4 = reinterpret_cast<const uint4*>(s + head);
            uint4* d4 = reinterpret_cast<uint4*>(d + head);
            for (int64_t i = t; i < body; i += nt) d4[i] = s4[i];
        } else if (vec == 4) {
            const uint32_t* s1 = reinterpret_cast<const uint32_t*>(s + head);
            uint32_t* d1 = reinterpret_cast<uint32_t*>(d + head);
            for (int64_t i = t; i < body; i += nt) d1[i] = s1[i];
        }
        for (int64_t i = t; i < head; i += nt) d[i] = s[i];
        for (int64_t i = tail0 + t; i < seg_bytes; i += nt) d[i] = s[i];
    }
}

}  // namespace slideo
