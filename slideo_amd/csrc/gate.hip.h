// gate.hip.h — kernels of the changed-frame gate (stage_gate.hip; include/slideo_amd.h "Changed-frame gate").
//
//   gate_kernel           the unit's n SSDs against the integer threshold T -> flags, the ascending list of kept frames, their count
//   gather_frames_kernel  the kept frames packed back to back (a pure copy)
// and of the frame mask's GATE scope (include/slideo_amd.h "Frame mask scope"):
//   mask_bgr_kernel       set time: the mask binarised and replicated to three channels, the image to_small_image is run on
//   gate_valid_kernel     set time: that image's small image -> the gate's byte weights and n_valid
//   ssd_masked_kernel     ssd_kernel's contract over the valid small pixels
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

// B of "Frame mask scope": pixel i of the w x h mask (rows `pitch` apart) -> 255, 255, 255 where it is nonzero, 0, 0, 0 elsewhere,
// packed (stride 3w).  grid ceil(w * h / 256).
__global__ __launch_bounds__(GATE_BLOCK) void mask_bgr_kernel(const uint8_t* __restrict__ mask, int pitch, int w, int h, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * GATE_BLOCK + threadIdx.x;
    if (i >= (uint32_t)w * (uint32_t)h) return;
    const uint32_t y = i / (uint32_t)w, x = i - y * (uint32_t)w;
    const uint8_t v = mask[(size_t)y * pitch + x] ? 255 : 0;
    uint8_t* d = out + (size_t)i * 3;
    d[0] = v; d[1] = v; d[2] = v;
}

// One block.  small: S = to_small_image(B), npx pixels of 3 bytes.  Pixel i is valid iff S[3i] == 255; its three weight bytes
// become 0xFF (valid) or 0x00, and the weights are zero-padded to a multiple of 4 bytes (ssd_masked_kernel reads them as dwords).
// n_valid: a wave-ballot count per chunk, the waves' totals summed through LDS at the end, ONE ordinary store.
__global__ __launch_bounds__(GATE_BLOCK) void gate_valid_kernel(const uint8_t* __restrict__ small, int npx, uint8_t* __restrict__ weights,
                                                                 long long* __restrict__ n_valid) {
    __shared__ uint32_t wtot[GATE_BLOCK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t mine = 0;                                                 // (lane 0: the wave's count so far)
    for (int base = 0; base < npx; base += GATE_BLOCK) {
        const int i = base + threadIdx.x;
        const bool valid = i < npx && small[(size_t)i * 3] == 255;
        if (i < npx) {
            const uint8_t v = valid ? 0xFF : 0x00;
            uint8_t* d = weights + (size_t)i * 3;
            d[0] = v; d[1] = v; d[2] = v;
        }
        mine += (uint32_t)__popcll(__ballot(valid));
    }
    const int pad = (4 - (int)(((size_t)npx * 3) & 3)) & 3;
    if ((int)threadIdx.x < pad) weights[(size_t)npx * 3 + threadIdx.x] = 0;
    if (lane == 0) wtot[w] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (int k = 0; k < GATE_BLOCK / 64; ++k) all += wtot[k];
        *n_valid = (long long)all;
    }
}

// ssd_kernel's contract — pair i = (a + i * a_stride, b + i * b_stride), nbytes each, one u64 per pair; grid n, block 256 — with
// the weights of gate_valid_kernel: out[i] = the sum over the bytes j with weights[j] == 0xFF of (a[j] - b[j])^2.
// A small image is 3 sw sh bytes, so a pair's a and b start at ANY byte alignment and at different ones.  Every image is read as
// ALIGNED dwords all the same: dword g of the image at p is bytes s .. s + 3 of the aligned dword pair q[g], q[g + 1], q = p - s,
// s = p & 3 (v_alignbyte_b32); lane t + 1's q[g] is lane t's q[g + 1], so the second load hits the line the first brought.  q[0]
// begins at most 3 bytes in front of the image (inside its allocation: device buffers are 256-byte aligned) and the body stops
// one dword early, so q[g + 1] never passes the image's end; the 4 .. 7 ragged bytes behind the body are read as bytes.
// Per dword: am = a & w, bm = b & w, then sum (am_k - bm_k)^2 = am.am + bm.bm - 2 am.bm as three 4 x u8 dot products (v_dot4_u32_u8),
// exact in integers.  The u32 partial sums take 520 200 per dword at most and are drained into u64 every 4096 dwords.
// weights: 4-byte aligned, zero-padded to whole dwords.  No LDS beyond the four waves' totals.
__global__ __launch_bounds__(256) void ssd_masked_kernel(const uint8_t* __restrict__ a, int64_t a_stride, const uint8_t* __restrict__ b,
                                                         int64_t b_stride, int64_t nbytes, const uint8_t* __restrict__ weights,
                                                         unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[4];
    const uint8_t* pa = a + (int64_t)blockIdx.x * a_stride;
    const uint8_t* pb = b + (int64_t)blockIdx.x * b_stride;
    const uint32_t sa = (uint32_t)(reinterpret_cast<uintptr_t>(pa) & 3), sb = (uint32_t)(reinterpret_cast<uintptr_t>(pb) & 3);
    const uint32_t* qa = reinterpret_cast<const uint32_t*>(pa - sa);
    const uint32_t* qb = reinterpret_cast<const uint32_t*>(pb - sb);
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(weights);
    const int64_t body = nbytes / 4 > 0 ? nbytes / 4 - 1 : 0;          // dwords
    unsigned long long s = 0;
    for (int64_t g0 = 0; g0 < body; g0 += 4096 * 256) {
        const int64_t g1 = g0 + 4096 * 256 < body ? g0 + 4096 * 256 : body;
        uint32_t sq = 0, cr = 0;
        for (int64_t g = g0 + threadIdx.x; g < g1; g += 256) {
            const uint32_t w = qw[g];
            const uint32_t am = __builtin_amdgcn_alignbyte(qa[g + 1], qa[g], sa) & w;
            const uint32_t bm = __builtin_amdgcn_alignbyte(qb[g + 1], qb[g], sb) & w;
            sq = __builtin_amdgcn_udot4(am, am, sq, false);
            sq = __builtin_amdgcn_udot4(bm, bm, sq, false);
            cr = __builtin_amdgcn_udot4(am, bm, cr, false);
        }
        s += (unsigned long long)sq - 2ull * cr;                       // (am.am + bm.bm >= 2 am.bm term by term)
    }
    for (int64_t i = body * 4 + threadIdx.x; i < nbytes; i += 256)
        if (weights[i]) { const int d = (int)pa[i] - (int)pb[i]; s += (unsigned)(d * d); }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

}  // namespace slideo
