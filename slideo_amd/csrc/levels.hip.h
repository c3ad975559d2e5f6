// levels.hip.h — the frame levels (include/slideo_amd.h "Frame levels"): the per-channel tone table applied to the unit's BGR image,
// and the per-channel histogram of the analysed images the table is learnt from.
//
//   levels_kernel        out[y][x][c] = lut[c][in[y][x][c]] over a block of n BGR8 images, in place (src == dst) or out of place.  The
//                        thread shape of pixels_to_bgr_kernel: four consecutive pixels of ONE row, block LVL_TX x LVL_TY = 64 threads
//                        along a row x 4 rows.  A thread's 12 bytes in: three aligned dwords where the source's base, row stride and
//                        frame stride (of more than one frame) are multiples of 4, else bytes; out: three dwords where the
//                        destination's are, else bytes; each side chosen by the host on its own (levels_args).  The ragged last 1 - 3
//                        pixels of a row always go byte by byte.  No multi-dword access at an address that is not dword-aligned.  A
//                        thread reads its 12 bytes before it writes them and no other thread touches them: in place is safe.
//                        The 768-byte table sits in LDS, loaded once per block as 192 dwords; 12 byte look-ups per thread.  A look-up
//                        instruction reads ONE channel's 256 bytes in every lane (byte i of a thread is channel i % 3): 64 dwords over
//                        the 32 banks sub-dword reads bank by, so two distinct dwords of a 32-lane half can share a bank and none more:
//                        2-way at worst (noise), a broadcast on the flat areas of a slide.
//   levels_hist_kernel   the histogram.  content_kernel's decomposition: a thread owns 4 pixels of a row and walks the block's n frames;
//                        a block walks row tiles LVH_GY * LVL_TY rows apart, so the number of flushing blocks is bounded.  A static
//                        picture repeats its dwords frame after frame: a thread keeps, per dword, the value and its run length, and
//                        adds the run to the 4 bins of the dword only when the dword changes and at the end of the walk.  n identical
//                        frames cost 12 LDS adds per thread and tile, not 12 n.  Bins: u32 [3][256] in LDS per block; a block counts at
//                        most 1024 px * LVH_MAX_FRAMES * LVH_MAX_TILES = 2^30 samples per channel (static_assert below), which fits.
//                        At the end the block's NONZERO bins go to the global u64 [3][256] with non-returning 64-bit atomics.
//                        Integer sums: exact whatever the order.
//
// The per-thread bodies are LVL_HD (host and device): tools/levels_hostcheck.cpp runs them lane by lane on the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LVL_HD __host__ __device__ __forceinline__
#else
#define LVL_HD inline
#endif

namespace slideo {

constexpr int LVL_TX = 64, LVL_TY = 4;
constexpr int LVH_UNROLL = 4;                  // frames whose loads are in flight per thread
constexpr int LVH_GY = 128;                    // row tiles walked side by side (grid.y) before a block takes more than one
constexpr int LVH_MAX_TILES = 256;             // row tiles per block at most (the host raises grid.y beyond LVH_GY to keep it)
constexpr int LVH_MAX_FRAMES = 4096;           // frames per launch at most (the observe driver's block)
static_assert((uint64_t)LVL_TX * LVL_TY * 4 * LVH_MAX_FRAMES * LVH_MAX_TILES < ((uint64_t)1 << 32), "a block's bins are u32");

// ---- the table ----------------------------------------------------------------------------------------------------------------
struct LevelsArgs {
    const uint8_t* src;          // n BGR8 images of w x h, rows src_stride bytes, frames src_frame_stride apart
    int64_t src_frame_stride;
    int src_stride;
    uint8_t* dst;                // the same geometry with its own strides; src == dst with equal strides: in place
    int64_t dst_frame_stride;
    int dst_stride;
    int w, h;
    int in4, out4;               // dword loads / stores: that side's base, row stride and frame stride are multiples of 4
    const uint8_t* lut;          // [3][256] (B, G, R), device memory, dword-aligned
};

// `cnt` pixels at s as three little-endian dwords: loaded as such when `dwords` (then cnt == 4 and s is dword-aligned), else from bytes
LVL_HD void lvl_load4(const uint8_t* s, int cnt, bool dwords, uint32_t (&d)[3]) {
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

// One thread of the launch grid: pixels 4 tix .. 4 tix + 3 of row `row` of frame z.  lut: the table the look-ups read (LDS on the device)
LVL_HD void levels_thread(const LevelsArgs& a, const uint8_t* lut, int tix, int row, int z) {
    const int x0 = tix * 4;
    if (x0 >= a.w || row >= a.h) return;
    const int cnt = a.w - x0 < 4 ? a.w - x0 : 4;
    const uint8_t* s = a.src + (int64_t)z * a.src_frame_stride + (int64_t)row * a.src_stride + (int64_t)x0 * 3;
    uint8_t* d = a.dst + (int64_t)z * a.dst_frame_stride + (int64_t)row * a.dst_stride + (int64_t)x0 * 3;
    uint32_t q[3], o[3] = {0, 0, 0};
    lvl_load4(s, cnt, a.in4 && cnt == 4, q);
    // byte i of the thread is channel i % 3 (a thread starts at a pixel); absent bytes of a ragged thread are looked up as 0, not stored
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 12; ++i) o[i >> 2] |= (uint32_t)lut[(i % 3) * 256 + ((q[i >> 2] >> (8 * (i & 3))) & 0xFFu)] << (8 * (i & 3));
    if (a.out4 && cnt == 4) {
        uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
        d4[0] = o[0]; d4[1] = o[1]; d4[2] = o[2];
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 12; ++i)
        if (i < 3 * cnt) d[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
}

// The arguments of a launch (host).  A single frame has no frame stride to be aligned.
inline LevelsArgs levels_args(const uint8_t* lut, const uint8_t* src, int64_t src_fs, int src_stride, uint8_t* dst, int64_t dst_fs, int dst_stride,
                              int w, int h, int n) {
    LevelsArgs a{};
    a.src = src; a.src_frame_stride = src_fs; a.src_stride = src_stride;
    a.dst = dst; a.dst_frame_stride = dst_fs; a.dst_stride = dst_stride;
    a.w = w; a.h = h; a.lut = lut;
    a.in4 = ((uint64_t)reinterpret_cast<uintptr_t>(src) | (uint64_t)(n > 1 ? src_fs : 0) | (uint64_t)(int64_t)src_stride) % 4 == 0;
    a.out4 = ((uint64_t)reinterpret_cast<uintptr_t>(dst) | (uint64_t)(n > 1 ? dst_fs : 0) | (uint64_t)(int64_t)dst_stride) % 4 == 0;
    return a;
}

// ---- the histogram ------------------------------------------------------------------------------------------------------------
struct LevelsHistArgs {
    const uint8_t* src;          // n BGR8 images of aw x ah, rows src_stride bytes, frames src_frame_stride apart
    int64_t src_frame_stride;
    int src_stride;
    int aw, ah, n;
    int in4;                     // src + 12 k is dword-aligned in every row of every frame
    unsigned long long* hist;    // [3][256]
};

#if defined(__HIP_DEVICE_COMPILE__)
#define LVH_ADD(p, v) atomicAdd((p), (v))     // (result unused: the non-returning LDS add)
#else
#define LVH_ADD(p, v) (*(p) += (v))
#endif

// a run of `run` equal dwords, dword k of the thread's three: its first `valid` bytes into the bins; byte 4 k + i is channel (4 k + i) % 3
LVL_HD void lvh_flush(uint32_t* bins, uint32_t d, int k, int valid, uint32_t run) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i)
        if (i < valid) LVH_ADD(bins + ((4 * k + i) % 3) * 256 + ((d >> (8 * i)) & 0xFFu), run);
}

// one more frame's three dwords into the thread's runs
LVL_HD void lvh_step(uint32_t* bins, const uint32_t (&q)[3], int nbytes, uint32_t (&cur)[3], uint32_t (&run)[3]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 3; ++k) {
        if (q[k] == cur[k]) { ++run[k]; continue; }               // (run 0: nothing seen yet, cur is 0; flushing a run of 0 adds 0)
        if (run[k]) lvh_flush(bins, cur[k], k, nbytes - 4 * k, run[k]);
        cur[k] = q[k]; run[k] = 1;
    }
}

// The thread that owns pixels 4 tix .. 4 tix + 3 of row y: all n frames into the block's bins
LVL_HD void levels_hist_thread(const LevelsHistArgs& a, uint32_t* bins, int tix, int y) {
    const int x0 = tix * 4;
    if (x0 >= a.aw || y >= a.ah || a.n < 1) return;
    const int cnt = a.aw - x0 < 4 ? a.aw - x0 : 4;
    const bool in4 = a.in4 && cnt == 4;
    const uint8_t* s = a.src + (int64_t)y * a.src_stride + (int64_t)x0 * 3;
    const int64_t fs = a.src_frame_stride;
    uint32_t cur[3] = {0, 0, 0}, run[3] = {0, 0, 0};
    int z = 0;
    for (; z + LVH_UNROLL <= a.n; z += LVH_UNROLL) {
        uint32_t q[LVH_UNROLL][3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < LVH_UNROLL; ++j) lvl_load4(s + (int64_t)(z + j) * fs, cnt, in4, q[j]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < LVH_UNROLL; ++j) lvh_step(bins, q[j], 3 * cnt, cur, run);
    }
    for (; z < a.n; ++z) {
        uint32_t q[3];
        lvl_load4(s + (int64_t)z * fs, cnt, in4, q);
        lvh_step(bins, q, 3 * cnt, cur, run);
    }
    for (int k = 0; k < 3; ++k)
        if (run[k]) lvh_flush(bins, cur[k], k, 3 * cnt - 4 * k, run[k]);
}

// grid.y of a launch over ah rows: LVH_GY tiles side by side, more where a block would walk more than LVH_MAX_TILES
inline int levels_hist_grid_y(int ah) {
    const int tiles = (ah + LVL_TY - 1) / LVL_TY;
    const int gy = tiles < LVH_GY ? tiles : LVH_GY;
    const int need = (tiles + LVH_MAX_TILES - 1) / LVH_MAX_TILES;
    return gy > need ? gy : need;
}

inline LevelsHistArgs levels_hist_args(const uint8_t* src, int64_t src_fs, int stride, int aw, int ah, int n, unsigned long long* hist) {
    LevelsHistArgs a{};
    a.src = src; a.src_frame_stride = src_fs; a.src_stride = stride;
    a.aw = aw; a.ah = ah; a.n = n;
    a.in4 = reinterpret_cast<uintptr_t>(src) % 4 == 0 && stride % 4 == 0 && (n < 2 || src_fs % 4 == 0);
    a.hist = hist;
    return a;
}

#if defined(__HIPCC__)
#if defined(LEVELS_APPLY_KERNEL)
// grid (ceil(ceil(w/4) / LVL_TX), ceil(h / LVL_TY), n), block (LVL_TX, LVL_TY)
__global__ __launch_bounds__(LVL_TX * LVL_TY) void levels_kernel(LevelsArgs a) {
    __shared__ uint32_t s_lut[192];
    const int tid = threadIdx.y * LVL_TX + threadIdx.x;
    if (tid < 192) s_lut[tid] = reinterpret_cast<const uint32_t*>(a.lut)[tid];
    __syncthreads();
    levels_thread(a, reinterpret_cast<const uint8_t*>(s_lut), blockIdx.x * LVL_TX + threadIdx.x, blockIdx.y * LVL_TY + threadIdx.y, blockIdx.z);
}
#endif

#if defined(LEVELS_HIST_KERNEL)
// grid (ceil(ceil(aw/4) / LVL_TX), levels_hist_grid_y(ah)), block (LVL_TX, LVL_TY)
__global__ __launch_bounds__(LVL_TX * LVL_TY) void levels_hist_kernel(LevelsHistArgs a) {
    __shared__ uint32_t s_bins[768];
    const int tid = threadIdx.y * LVL_TX + threadIdx.x;
    for (int b = tid; b < 768; b += LVL_TX * LVL_TY) s_bins[b] = 0;
    __syncthreads();
    const int tix = blockIdx.x * LVL_TX + threadIdx.x;
    for (int y = blockIdx.y * LVL_TY + threadIdx.y; y < a.ah; y += gridDim.y * LVL_TY) levels_hist_thread(a, s_bins, tix, y);
    __syncthreads();
    for (int b = tid; b < 768; b += LVL_TX * LVL_TY) {
        const uint32_t v = s_bins[b];
        if (v) atomicAdd(a.hist + b, (unsigned long long)v);      // (result unused: the non-returning global add)
    }
}
#endif
#endif

}  // namespace slideo
