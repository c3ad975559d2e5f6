// content.hip.h — the frame content box (include/slideo_amd.h "Frame content box"): per pixel of the analysed image the number of
// observed frames in which it is lit, and the row and column fills read out of those counts.
//
//   content_kernel         one launch per staged block of n frames, behind or in place of activity_kernel on the same frames.  A thread
//                          owns 4 consecutive pixels of a row (the decomposition of activity_kernel, reduce2x2_kernel and
//                          yuv420_to_bgr_desc_kernel) and walks the block's frames with its four counts in registers; at the end ONE
//                          read-modify-write of its counts.  Every count has exactly one owner: no atomic, no LDS.  A stream: 3 B in
//                          per pixel and frame, 4 B in and out per pixel once per block.  It carries no previous pixels.
//   content_fill_kernel    read-out: content = lit * 1000000 > min_share_ppm * frames (u64).  A thread owns a column and walks a strip
//                          of CNT_FILL_ROWS rows: a row's count comes from a wave ballot, a column's stays in a register across the
//                          strip; one non-returning integer atomic per row and wave, per column and strip, and per wave and strip for
//                          the total.  Integer sums: exact whatever the order.
//
// Loads of content_kernel.  Where the frames' rows are dword-aligned (base, stride and frame stride multiples of 4) a thread's 12
// bytes are three aligned dwords at row + 12 tix; otherwise, and in the ragged last 1 - 3 pixels of a row, bytes, packed into the
// same three dwords (absent bytes 0, which is never lit).  It never issues an unaligned multi-dword load.  lit is max(B, G, R) >
// level, taken on the three dwords byte by byte; no pixel is extracted.  The frame loop is unrolled by CNT_UNROLL: a thread's loads
// of consecutive frames do not depend on each other and are in flight together.
//
// The per-thread bodies are CNT_HD (host and device): tools/content_hostcheck.cpp runs them lane by lane on the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CNT_HD __host__ __device__ __forceinline__
#else
#define CNT_HD inline
#endif

namespace slideo {

constexpr int CNT_TX = 64, CNT_TY = 4;
constexpr int CNT_UNROLL = 4;                  // frames whose loads are in flight per thread
constexpr int CNT_FILL_TX = 256, CNT_FILL_ROWS = 32;
constexpr int CNT_MAX_LEVEL = 254, CNT_MAX_PPM = 1000000;

struct ContentArgs {
    const uint8_t* src;          // n BGR8 images of aw x ah, rows of src_stride bytes, frames src_frame_stride apart
    int64_t src_frame_stride;
    int src_stride;
    int aw, ah, n;
    uint32_t level;              // lit: max(B, G, R) > level
    int in4;                     // src + 12 k is dword-aligned in every row of every frame (host-checked: content_args)
    int own4;                    // aw % 4 == 0: a thread's 4 counts are one 16-byte access
    uint32_t* lit;               // [ah][aw]
};

CNT_HD uint32_t cnt_byte(uint32_t d, int k) { return (d >> (8 * k)) & 0xFFu; }
CNT_HD uint32_t cnt_max3(uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a > b ? a : b; return m > c ? m : c; }

// `cnt` pixels at s as three little-endian dwords: loaded as such when `dwords` (then cnt == 4 and s is dword-aligned), else from bytes
CNT_HD void cnt_load4(const uint8_t* s, int cnt, bool dwords, uint32_t (&d)[3]) {
    if (dwords) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(s);
        d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
        return;
    }
    d[0] = d[1] = d[2] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 12; ++i)                                   // (constant indices once unrolled: d stays in registers)
        if (i < 3 * cnt) d[i >> 2] |= (uint32_t)s[i] << (8 * (i & 3));
}

// the four pixels b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
CNT_HD void cnt_step(const uint32_t (&d)[3], uint32_t level, uint32_t (&c)[4]) {
    c[0] += cnt_max3(cnt_byte(d[0], 0), cnt_byte(d[0], 1), cnt_byte(d[0], 2)) > level ? 1u : 0u;
    c[1] += cnt_max3(cnt_byte(d[0], 3), cnt_byte(d[1], 0), cnt_byte(d[1], 1)) > level ? 1u : 0u;
    c[2] += cnt_max3(cnt_byte(d[1], 2), cnt_byte(d[1], 3), cnt_byte(d[2], 0)) > level ? 1u : 0u;
    c[3] += cnt_max3(cnt_byte(d[2], 1), cnt_byte(d[2], 2), cnt_byte(d[2], 3)) > level ? 1u : 0u;
}

// The thread that owns pixels 4 tix .. 4 tix + 3 of row y
CNT_HD void content_thread(const ContentArgs& a, int tix, int y) {
    const int x0 = tix * 4;
    if (x0 >= a.aw || y >= a.ah || a.n < 1) return;
    const int cnt = a.aw - x0 < 4 ? a.aw - x0 : 4;
    const bool in4 = a.in4 && cnt == 4;
    const uint8_t* s = a.src + (int64_t)y * a.src_stride + (int64_t)x0 * 3;
    const int64_t fs = a.src_frame_stride;
    uint32_t* cp = a.lit + (int64_t)y * a.aw + x0;
    uint32_t c[4] = {0, 0, 0, 0};
    int z = 0;
    for (; z + CNT_UNROLL <= a.n; z += CNT_UNROLL) {
        uint32_t q[CNT_UNROLL][3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < CNT_UNROLL; ++j) cnt_load4(s + (int64_t)(z + j) * fs, cnt, in4, q[j]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < CNT_UNROLL; ++j) cnt_step(q[j], a.level, c);
    }
    for (; z < a.n; ++z) {
        uint32_t q[3];
        cnt_load4(s + (int64_t)z * fs, cnt, in4, q);
        cnt_step(q, a.level, c);
    }
    if (a.own4) {                                                  // (own4: cnt == 4 in every thread)
#if defined(__HIP_DEVICE_COMPILE__)
        uint4* c4 = reinterpret_cast<uint4*>(cp);
        uint4 v = *c4;
        v.x += c[0]; v.y += c[1]; v.z += c[2]; v.w += c[3];
        *c4 = v;
#else
        for (int i = 0; i < 4; ++i) cp[i] += c[i];
#endif
    } else {
        for (int i = 0; i < cnt; ++i) cp[i] += c[i];
    }
}

// The arguments of a launch (host): n images at src into the counts
inline ContentArgs content_args(const uint8_t* src, int64_t src_fs, int stride, int aw, int ah, int n, int level, uint32_t* lit) {
    ContentArgs a{};
    a.src = src; a.src_frame_stride = src_fs; a.src_stride = stride;
    a.aw = aw; a.ah = ah; a.n = n;
    a.level = (uint32_t)level;
    a.in4 = reinterpret_cast<uintptr_t>(src) % 4 == 0 && stride % 4 == 0 && src_fs % 4 == 0;
    a.own4 = aw % 4 == 0 && reinterpret_cast<uintptr_t>(lit) % 16 == 0;
    a.lit = lit;
    return a;
}

// ---- the read-out -------------------------------------------------------------------------------------------------------------
struct ContentFillArgs {
    const uint32_t* lit;         // [ah][aw]
    int aw, ah;
    uint64_t ppm, frames;        // content: lit * 1000000 > ppm * frames
    uint32_t* row_fill;          // [ah], zeroed
    uint32_t* col_fill;          // [aw], zeroed
    unsigned long long* n_content;   // zeroed
};

// the content test of pixel (x, y), y < ah; a lane beyond the last column holds none
CNT_HD bool content_px(const ContentFillArgs& a, int x, int y) {
    return x < a.aw && (uint64_t)a.lit[(int64_t)y * a.aw + x] * 1000000ull > a.ppm * a.frames;
}

// the rows [y0, y1) of strip `strip`
CNT_HD void content_strip(const ContentFillArgs& a, int strip, int& y0, int& y1) {
    y0 = strip * CNT_FILL_ROWS;
    y1 = y0 + CNT_FILL_ROWS < a.ah ? y0 + CNT_FILL_ROWS : a.ah;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(CNT_TX * CNT_TY) void content_kernel(ContentArgs a) {
    content_thread(a, blockIdx.x * CNT_TX + threadIdx.x, blockIdx.y * CNT_TY + threadIdx.y);
}

// grid (ceil(aw / 256), ceil(ah / 32)), block 256: a thread owns column x of its strip
__global__ __launch_bounds__(CNT_FILL_TX) void content_fill_kernel(ContentFillArgs a) {
    const int x = blockIdx.x * CNT_FILL_TX + threadIdx.x;
    const bool first_lane = (threadIdx.x & 63) == 0;
    int y0, y1;
    content_strip(a, blockIdx.y, y0, y1);
    uint32_t col = 0, wave = 0;
    for (int y = y0; y < y1; ++y) {
        const bool c = content_px(a, x, y);
        const uint32_t n = (uint32_t)__popcll(__ballot(c));
        if (first_lane && n) atomicAdd(a.row_fill + y, n);
        col += c ? 1u : 0u;
        wave += n;
    }
    if (col) atomicAdd(a.col_fill + x, col);                      // (col > 0: x < aw)
    if (first_lane && wave) atomicAdd(a.n_content, (unsigned long long)wave);
}
#endif

}  // namespace slideo
