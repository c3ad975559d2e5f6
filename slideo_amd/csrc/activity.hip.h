// activity.hip.h — the frame activity map (include/slideo_amd.h "Frame activity map"): per pixel of the analysed image the number of
// consecutive-frame pairs in which it moved, and the mask read out of those counts.
//
//   activity_kernel        one launch per staged block of n frames.  A thread owns 4 consecutive pixels of a row (the decomposition of
//                          reduce2x2_kernel, rectify_kernel and yuv420_to_bgr_desc_kernel) and walks the block's frames in order with the
//                          previous frame's four pixels and its four counts in registers; at the end ONE read-modify-write of its
//                          counts and ONE store of its last 12 bytes into the carried image.  Every count and every carried byte has
//                          exactly one owner: no atomic, no LDS.  A stream: 3 B in per pixel and frame, 4 + 3 B in and out per pixel
//                          once per block.
//   activity_rows_kernel   read-out, pass 1: active = count * 1000000 > max_share_ppm * pairs (u64), OR over [x - grow, x + grow]
//   activity_cols_kernel   read-out, pass 2: OR of pass 1 over [y - grow, y + grow], 0 / 255
//                          (both count through wave ballots, the waves' totals through LDS, one non-returning atomic per block)
//
// Loads of activity_kernel.  Where the frames' rows are dword-aligned (base, stride and frame stride multiples of 4) a thread's 12
// bytes are three aligned dwords at row + 12 tix; otherwise, and in the ragged last 1 - 3 pixels of a row, bytes.  An unaligned
// multi-dword load is split by the texture path (README round 5): the kernel never issues one.  The four 3-byte pixels are taken out
// of the three dwords with the top byte zero (v_and / v_perm_b32 / v_lshrrev), so that ONE v_sad_u8 against the previous frame's
// extracted pixel is |dB| + |dG| + |dR|; the extracted form is what stays in registers.  The frame loop is unrolled by ACT_UNROLL: a
// thread's loads of consecutive frames do not depend on each other and are in flight together.
//
// The per-thread bodies are ACT_HD (host and device): tools/activity_hostcheck.cpp runs them lane by lane on the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ACT_HD __host__ __device__ __forceinline__
#else
#define ACT_HD inline
#endif

namespace slideo {

constexpr int ACT_TX = 64, ACT_TY = 4;
constexpr int ACT_UNROLL = 4;                  // frames whose loads are in flight per thread
constexpr int ACT_MAX_DELTA = 765, ACT_MAX_GROW = 64, ACT_MAX_PPM = 1000000;

struct ActivityArgs {
    const uint8_t* src;          // n BGR8 images of aw x ah, rows of src_stride bytes, frames src_frame_stride apart
    int64_t src_frame_stride;
    int src_stride;
    int aw, ah, n;
    uint32_t delta;              // moved: SAD > delta
    int have_prev;               // the carried image holds the frame in front of frame 0 (0: frame 0 only primes)
    int in4;                     // src + 12 k is dword-aligned in every row of every frame (host-checked: activity_args)
    int own4;                    // aw % 4 == 0: a thread's 12 carried bytes are three aligned dwords, its 4 counts one 16-byte access
    uint8_t* last;               // the carried image: aw x ah, rows of 3 aw bytes
    uint32_t* count;             // [ah][aw]
};

ACT_HD uint32_t act_sad(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, 0u);
#else
    uint32_t s = 0;
    for (int k = 0; k < 32; k += 8) {
        const int d = (int)((a >> k) & 0xFFu) - (int)((b >> k) & 0xFFu);
        s += (uint32_t)(d < 0 ? -d : d);
    }
    return s;
#endif
}

// the four pixels (b | g << 8 | r << 16, top byte zero) of 12 bytes held as three little-endian dwords
ACT_HD void act_extract(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t (&p)[4]) {
    p[0] = d0 & 0x00FFFFFFu;
#if defined(__HIP_DEVICE_COMPILE__)
    p[1] = __builtin_amdgcn_perm(d1, d0, 0x0c050403u);        // {d0.3, d1.0, d1.1, 0}
    p[2] = __builtin_amdgcn_perm(d2, d1, 0x0c040302u);        // {d1.2, d1.3, d2.0, 0}
#else
    p[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
    p[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
#endif
    p[3] = d2 >> 8;
}

// `cnt` pixels at s: three dwords when `dwords` (then cnt == 4 and s is dword-aligned), bytes otherwise
ACT_HD void act_load4(const uint8_t* s, int cnt, bool dwords, uint32_t (&p)[4]) {
    if (dwords) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(s);
        act_extract(q[0], q[1], q[2], p);
        return;
    }
    p[0] = p[1] = p[2] = p[3] = 0;
    for (int i = 0; i < cnt; ++i) p[i] = (uint32_t)s[3 * i] | ((uint32_t)s[3 * i + 1] << 8) | ((uint32_t)s[3 * i + 2] << 16);
}

ACT_HD void act_step(uint32_t (&prev)[4], const uint32_t (&cur)[4], uint32_t delta, uint32_t (&c)[4]) {
    for (int i = 0; i < 4; ++i) {
        c[i] += act_sad(prev[i], cur[i]) > delta ? 1u : 0u;
        prev[i] = cur[i];
    }
}

// The thread that owns pixels 4 tix .. 4 tix + 3 of row y
ACT_HD void activity_thread(const ActivityArgs& a, int tix, int y) {
    const int x0 = tix * 4;
    if (x0 >= a.aw || y >= a.ah || a.n < 1) return;
    const int cnt = a.aw - x0 < 4 ? a.aw - x0 : 4;
    const bool in4 = a.in4 && cnt == 4, own4 = a.own4 != 0;       // (own4: cnt == 4 in every thread)
    const uint8_t* s = a.src + (int64_t)y * a.src_stride + (int64_t)x0 * 3;
    const int64_t fs = a.src_frame_stride;
    uint8_t* lastp = a.last + ((int64_t)y * a.aw + x0) * 3;
    uint32_t* cp = a.count + (int64_t)y * a.aw + x0;
    uint32_t prev[4], c[4] = {0, 0, 0, 0};
    int z = 0;
    if (a.have_prev) act_load4(lastp, cnt, own4, prev);
    else { act_load4(s, cnt, in4, prev); z = 1; }
    for (; z + ACT_UNROLL <= a.n; z += ACT_UNROLL) {
        uint32_t q[ACT_UNROLL][4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < ACT_UNROLL; ++j) act_load4(s + (int64_t)(z + j) * fs, cnt, in4, q[j]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < ACT_UNROLL; ++j) act_step(prev, q[j], a.delta, c);
    }
    for (; z < a.n; ++z) {
        uint32_t q[4];
        act_load4(s + (int64_t)z * fs, cnt, in4, q);
        act_step(prev, q, a.delta, c);
    }
    if (own4) {
#if defined(__HIP_DEVICE_COMPILE__)
        uint4* c4 = reinterpret_cast<uint4*>(cp);
        uint4 v = *c4;
        v.x += c[0]; v.y += c[1]; v.z += c[2]; v.w += c[3];
        *c4 = v;
#else
        for (int i = 0; i < 4; ++i) cp[i] += c[i];
#endif
        uint32_t* q = reinterpret_cast<uint32_t*>(lastp);
        q[0] = prev[0] | (prev[1] << 24);                 // b0 g0 r0 b1
        q[1] = (prev[1] >> 8) | (prev[2] << 16);          // g1 r1 b2 g2
        q[2] = (prev[2] >> 16) | (prev[3] << 8);          // r2 b3 g3 r3
    } else {
        for (int i = 0; i < cnt; ++i) {
            cp[i] += c[i];
            lastp[3 * i] = (uint8_t)prev[i]; lastp[3 * i + 1] = (uint8_t)(prev[i] >> 8); lastp[3 * i + 2] = (uint8_t)(prev[i] >> 16);
        }
    }
}

// The arguments of a launch (host): n images at src into the accumulator (count, last)
inline ActivityArgs activity_args(const uint8_t* src, int64_t src_fs, int stride, int aw, int ah, int n, int delta, bool have_prev, uint8_t* last,
                                  uint32_t* count) {
    ActivityArgs a{};
    a.src = src; a.src_frame_stride = src_fs; a.src_stride = stride;
    a.aw = aw; a.ah = ah; a.n = n;
    a.delta = (uint32_t)delta; a.have_prev = have_prev ? 1 : 0;
    a.in4 = reinterpret_cast<uintptr_t>(src) % 4 == 0 && stride % 4 == 0 && src_fs % 4 == 0;
    a.own4 = aw % 4 == 0 && reinterpret_cast<uintptr_t>(last) % 4 == 0 && reinterpret_cast<uintptr_t>(count) % 16 == 0;
    a.last = last; a.count = count;
    return a;
}

// ---- the mask read-out --------------------------------------------------------------------------------------------------------
struct ActivityMaskArgs {
    const uint32_t* count;       // [ah][aw]
    int aw, ah, grow;
    uint64_t ppm, pairs;         // active: count * 1000000 > ppm * pairs
    uint8_t* rows;               // pass 1: 1 where an active pixel lies within `grow` columns in the same row
    uint8_t* mask;               // pass 2: 0 where pass 1 is set within `grow` rows in the same column, else 255
};

ACT_HD bool act_active(const ActivityMaskArgs& a, int x, int y) {
    return (uint64_t)a.count[(int64_t)y * a.aw + x] * 1000000ull > a.ppm * a.pairs;
}

// pass 1 of pixel (x, y); the return value: the pixel itself is active
ACT_HD bool activity_rows_px(const ActivityMaskArgs& a, int x, int y) {
    const int lo = x - a.grow > 0 ? x - a.grow : 0, hi = x + a.grow < a.aw - 1 ? x + a.grow : a.aw - 1;
    bool any = false;
    for (int k = lo; k <= hi && !any; ++k) any = act_active(a, k, y);
    a.rows[(int64_t)y * a.aw + x] = any ? 1 : 0;
    return act_active(a, x, y);
}

// pass 2 of pixel (x, y); the return value: the pixel is masked (0)
ACT_HD bool activity_cols_px(const ActivityMaskArgs& a, int x, int y) {
    const int lo = y - a.grow > 0 ? y - a.grow : 0, hi = y + a.grow < a.ah - 1 ? y + a.grow : a.ah - 1;
    bool any = false;
    for (int k = lo; k <= hi && !any; ++k) any = a.rows[(int64_t)k * a.aw + x] != 0;
    a.mask[(int64_t)y * a.aw + x] = any ? 0 : 255;
    return any;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(ACT_TX * ACT_TY) void activity_kernel(ActivityArgs a) {
    activity_thread(a, blockIdx.x * ACT_TX + threadIdx.x, blockIdx.y * ACT_TY + threadIdx.y);
}

// the block's number of set predicates added to *total: ballots, the waves' totals through LDS, one non-returning atomic
__device__ __forceinline__ void act_block_count(bool pred, unsigned long long* total) {
    __shared__ uint32_t wave_n[ACT_TY];
    const uint32_t n = (uint32_t)__popcll(__ballot(pred));
    if (threadIdx.x == 0) wave_n[threadIdx.y] = n;       // (a wave is one row of the block: ACT_TX == the wave size)
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        uint32_t s = 0;
        for (int i = 0; i < ACT_TY; ++i) s += wave_n[i];
        if (s) atomicAdd(total, (unsigned long long)s);
    }
}

// grid (ceil(aw / 64), ceil(ah / 4)), block (64, 4): one pixel per thread
__global__ __launch_bounds__(ACT_TX * ACT_TY) void activity_rows_kernel(ActivityMaskArgs a, unsigned long long* n_active) {
    const int x = blockIdx.x * ACT_TX + threadIdx.x, y = blockIdx.y * ACT_TY + threadIdx.y;
    const bool in = x < a.aw && y < a.ah;
    act_block_count(in && activity_rows_px(a, x, y), n_active);
}

__global__ __launch_bounds__(ACT_TX * ACT_TY) void activity_cols_kernel(ActivityMaskArgs a, unsigned long long* n_masked) {
    const int x = blockIdx.x * ACT_TX + threadIdx.x, y = blockIdx.y * ACT_TY + threadIdx.y;
    const bool in = x < a.aw && y < a.ah;
    act_block_count(in && activity_cols_px(a, x, y), n_masked);
}
#endif

}  // namespace slideo
