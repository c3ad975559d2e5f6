// shading.hip.h — the frame shading (include/slideo_amd.h "Frame shading"): the smooth gain field applied to the unit's BGR image,
// in front of the frame levels.
//
//   shading_kernel<LUT>  out[c] = min(255, (in[c] * G + 128) >> 8) over a block of n BGR8 images, in place (src == dst) or out of
//                        place, G the field's Q8.8 gain at the pixel: bilinear between the four nodes of the pixel's cell, in exact
//                        integers.  The thread shape of levels_kernel (levels.hip.h), whose loads, stores and argument rule it
//                        reuses: four consecutive pixels of ONE row, block LVL_TX x LVL_TY, grid.z the frames; dword or byte loads
//                        and stores per side as levels_args chooses; no multi-dword access at an address that is not dword-aligned;
//                        a thread reads its 12 bytes before it writes them: in place is safe.
//                        x0 is a multiple of 4 and the cell a multiple of 16, so a thread's four pixels lie in ONE cell: it fetches
//                        the cell's four nodes once (u16, a handful of distinct addresses per block: cache hits) and interpolates
//                        vertically once (L, R).  Per pixel two 24-bit multiply-adds and a shift give G, then three 24-bit
//                        multiply-adds with a min give the bytes.  Bounds: a gain is below 2^16 and a weight at most 64, so L, R <
//                        2^22 and L (cell - fx) + R fx <= 65535 cell^2 < 2^28; in * G < 2^24: every product's factors fit 24 bits.
//                        LUT false: the plain instance.  LUT true: the fused one — the levels look-up (the 768-byte table in LDS, as
//                        levels_kernel holds it) on the shaded bytes, so a matcher with both settings makes one pass.
//
// The per-thread body is LVL_HD (host and device): tools/shading_hostcheck.cpp runs it lane by lane on the CPU.
#pragma once
#include <stdint.h>

#include "levels.hip.h"

namespace slideo {

struct ShadingArgs {
    LevelsArgs img;              // the images on both sides and the load / store choice (levels_args); img.lut: the fused table, or null
    const uint16_t* gains;       // [gh + 1][gw + 1] Q8.8 nodes, device memory; gw = ceil(img.w / cell), gh = ceil(img.h / cell)
    int pitch;                   // gw + 1
    int shift;                   // log2(cell): 4, 5 or 6
};

#if defined(__HIP_DEVICE_COMPILE__)
#define SHD_MAD24(a, b, c) (__umul24((a), (b)) + (c))      // (v_mad_u32_u24: both factors below 2^24, see the bounds above)
#else
#define SHD_MAD24(a, b, c) ((uint32_t)(a) * (uint32_t)(b) + (uint32_t)(c))
#endif

// One thread of the launch grid: pixels 4 tix .. 4 tix + 3 of row `row` of frame z.  lut: the table the fused look-ups read (LDS on
// the device), unused by the plain instance
template <bool LUT>
LVL_HD void shading_thread(const ShadingArgs& a, const uint8_t* lut, int tix, int row, int z) {
    const LevelsArgs& I = a.img;
    const int x0 = tix * 4;
    if (x0 >= I.w || row >= I.h) return;
    const int cnt = I.w - x0 < 4 ? I.w - x0 : 4;
    const uint8_t* s = I.src + (int64_t)z * I.src_frame_stride + (int64_t)row * I.src_stride + (int64_t)x0 * 3;
    uint8_t* d = I.dst + (int64_t)z * I.dst_frame_stride + (int64_t)row * I.dst_stride + (int64_t)x0 * 3;
    uint32_t q[3], o[3] = {0, 0, 0};
    lvl_load4(s, cnt, I.in4 && cnt == 4, q);
    // the cell (i, j) of all four pixels; its nodes (j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1) exist: i <= gw - 1, j <= gh - 1
    const uint32_t cell = 1u << a.shift, fx0 = (uint32_t)x0 & (cell - 1), fy = (uint32_t)row & (cell - 1);
    const uint16_t* g = a.gains + (int64_t)(row >> a.shift) * a.pitch + (x0 >> a.shift);
    const uint32_t L = SHD_MAD24((uint32_t)g[0], cell - fy, SHD_MAD24((uint32_t)g[a.pitch], fy, 0u));
    const uint32_t R = SHD_MAD24((uint32_t)g[1], cell - fy, SHD_MAD24((uint32_t)g[a.pitch + 1], fy, 0u));
    uint32_t G[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 4; ++k)                               // (fx0 <= cell - 4: fx0 + k stays inside the cell)
        G[k] = SHD_MAD24(L, cell - fx0 - k, SHD_MAD24(R, fx0 + k, cell * cell / 2)) >> (2 * a.shift);
    // byte i of the thread is channel i % 3 of pixel i / 3; absent bytes of a ragged thread are computed from 0, not stored
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 12; ++i) {
        uint32_t v = SHD_MAD24((q[i >> 2] >> (8 * (i & 3))) & 0xFFu, G[i / 3], 128u) >> 8;
        v = v < 255u ? v : 255u;
        if (LUT) v = lut[(i % 3) * 256 + v];
        o[i >> 2] |= v << (8 * (i & 3));
    }
    if (I.out4 && cnt == 4) {
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

// The arguments of a launch (host): levels_args' choice of loads and stores; lut null: the plain instance's.  w x h is the field's
// analysed size (the caller's check), cell 16, 32 or 64
inline ShadingArgs shading_args(const uint16_t* gains, int cell, const uint8_t* lut, const uint8_t* src, int64_t src_fs, int src_stride, uint8_t* dst,
                                int64_t dst_fs, int dst_stride, int w, int h, int n) {
    ShadingArgs a{};
    a.img = levels_args(lut, src, src_fs, src_stride, dst, dst_fs, dst_stride, w, h, n);
    a.gains = gains;
    a.shift = cell == 16 ? 4 : cell == 32 ? 5 : 6;
    a.pitch = ((w + cell - 1) >> a.shift) + 1;
    return a;
}

#if defined(__HIPCC__) && defined(SHADING_APPLY_KERNEL)
// grid (ceil(ceil(w/4) / LVL_TX), ceil(h / LVL_TY), n), block (LVL_TX, LVL_TY)
template <bool LUT>
__global__ __launch_bounds__(LVL_TX * LVL_TY) void shading_kernel(ShadingArgs a) {
    __shared__ uint32_t s_lut[LUT ? 192 : 1];
    if (LUT) {
        const int tid = threadIdx.y * LVL_TX + threadIdx.x;
        if (tid < 192) s_lut[tid] = reinterpret_cast<const uint32_t*>(a.img.lut)[tid];
        __syncthreads();
    }
    shading_thread<LUT>(a, reinterpret_cast<const uint8_t*>(s_lut), blockIdx.x * LVL_TX + threadIdx.x, blockIdx.y * LVL_TY + threadIdx.y, blockIdx.z);
}
#endif

}  // namespace slideo

// ---- the match shading map (include/slideo_amd.h "Match shading map") ---------------------------------------------------------------
//   shading_map_kernel   grid: the unit's frames, block TONE_THREADS; launched by unit_verify behind verdict_kernel and the other
//                        sessions' kernels on the unit's stream, only while a session is open.  Everything up to the sample is the
//                        tone table's, by inclusion (tone.hip.h): the flags word read first, the contributor (tone_frame), phase 1
//                        (tone_votes, the box through LDS min / max), the sample test.  Phase 2: work items of TONE_SEG consecutive
//                        pixels of one small-image row; per item a thread keeps ONE cell index with a run count and two run sums and
//                        issues its three LDS adds (results unused) only when the cell changes and at the item's end — consecutive
//                        small pixels land in the same cell of the analysed image for tens of pixels.  Bins: u32 [3][cells] in
//                        dynamic LDS {cnt | sum_f | sum_p}, at most 48 KB at SHM_MAX_CELLS; row tiles of at most TONE_TILE_PX pixels
//                        (static_assert below); the block's NONZERO bins go to the u64 arrays with 64-bit atomics whose result is
//                        not read.  No returning atomic in a loop, no compare-and-swap, no scratch.
// The per-frame body is host + device functions (tools/shading_hostcheck.cpp runs it on the CPU).  Compiled where SHADING_MAP is defined
// (stage_verify.hip), since it needs the verify stage's records.
#if defined(SHADING_MAP)
#include "tone.hip.h"

namespace slideo {

constexpr int SHM_MAX_CELLS = 4096;                      // cells of a session's grid at most: 48 KB of bins
constexpr int64_t SHM_MAX_FRAMES = (int64_t)1 << 20;     // frames through a session
static_assert((uint64_t)3 * 255 * TONE_TILE_PX < ((uint64_t)1 << 32), "a block's sum bins are u32");

struct ShadingMapArgs {
    ToneArgs t;                          // tone_kernel's arguments (acc unused): the contributor, the hits, the sample test
    int32_t shift, gw, cells;            // log2(cell), the grid's width, gw * gh <= SHM_MAX_CELLS
    unsigned long long* acc;             // {cnt [cells] | sum_f [cells] | sum_p [cells] | frames_counted}
};

// phase 2 of the row tile [j0, j1): thread tid of nt walks its work items; bins: 3 * cells words, zero before the tile
template <class Add>
EV_HD void shading_map_samples(const ShadingMapArgs& a, const ToneFrame& e, const ToneBox& box, int f, int j0, int j1, int tid, int nt, uint32_t* bins,
                               Add&& add) {
    const ToneArgs& t = a.t;
    const PageInfo pi = t.pageinfo[e.page];
    const uint8_t* small = t.page_small + pi.small_ofs;
    const uint8_t* frame = t.frames + (int64_t)f * t.frame_stride;
    const int sw = pi.sw, sh = pi.sh;
    const int nseg = (sw + TONE_SEG - 1) / TONE_SEG;
    const int items = (j1 - j0) * nseg;
    const double* M = e.M;
    for (int it = tid; it < items; it += nt) {
        const int j = j0 + it / nseg, i0 = (it % nseg) * TONE_SEG;
        const double y = tone_centre(j, pi.h, sh);
        if (!((double)box.y0 <= y && y <= (double)box.y1)) continue;
        const int i1 = i0 + TONE_SEG < sw ? i0 + TONE_SEG : sw;
        uint32_t cur = 0, run = 0, rf = 0, rp = 0;
        for (int i = i0; i < i1; ++i) {
            const double x = tone_centre(i, pi.w, sw);
            if (!((double)box.x0 <= x && x <= (double)box.x1)) continue;
            double X = M[0] * x + M[1] * y + M[2], Y = M[3] * x + M[4] * y + M[5];
            if (t.ev.model == 1) {
                const double w = M[6] * x + M[7] * y + M[8];
                if (w == 0.0) continue;
                X /= w; Y /= w;
            }
            const double Xr = __builtin_floor(X + 0.5), Yr = __builtin_floor(Y + 0.5);
            if (!(Xr >= 0.0 && Xr < (double)t.aw && Yr >= 0.0 && Yr < (double)t.ah)) continue;      // (a NaN fails here)
            if (!tone_flat(small, sw, sh, i, j, t.flat)) continue;
            const int Xi = (int)Xr, Yi = (int)Yr;
            const uint8_t* fp = frame + (int64_t)Yi * t.stride + (int64_t)Xi * 3;
            const uint8_t* pp = small + ((size_t)j * sw + i) * 3;
            const uint32_t k = (uint32_t)((Yi >> a.shift) * a.gw + (Xi >> a.shift));      // (< cells: Xi < aw, Yi < ah)
            if (run && k != cur) {
                add(bins + cur, run); add(bins + a.cells + cur, rf); add(bins + 2 * a.cells + cur, rp);
                run = 0; rf = 0; rp = 0;
            }
            cur = k; ++run;
            rf += (uint32_t)fp[0] + fp[1] + fp[2];
            rp += (uint32_t)pp[0] + pp[1] + pp[2];
        }
        if (run) { add(bins + cur, run); add(bins + a.cells + cur, rf); add(bins + 2 * a.cells + cur, rp); }
    }
}

// the tile's nonzero bins to the accumulators: thread tid of nt
template <class Add64>
EV_HD void shading_map_flush(const ShadingMapArgs& a, int tid, int nt, const uint32_t* bins, Add64&& add64) {
    for (int b = tid; b < 3 * a.cells; b += nt) {
        const uint32_t v = bins[b];
        if (v) add64(a.acc + b, (unsigned long long)v);
    }
}

#if defined(__HIPCC__)
// dynamic LDS: (3 * cells + 5) * 4 bytes — the bins, then the hits' count and box
__global__ __launch_bounds__(TONE_THREADS) void shading_map_kernel(ShadingMapArgs a) {
    extern __shared__ uint32_t shm_lds[];
    uint32_t* bins = shm_lds;
    int32_t* s_box = reinterpret_cast<int32_t*>(shm_lds + 3 * a.cells);
    const int f = blockIdx.x, tid = threadIdx.x;
    const ToneFrame e = tone_frame(a.t, f);                // (the flags word first; block-uniform: every thread reads the same words)
    if (e.slot < 0) return;
    if (tid == 0) { const ToneBox z = tone_box_empty(); s_box[0] = 0; s_box[1] = z.x0; s_box[2] = z.y0; s_box[3] = z.x1; s_box[4] = z.y1; }
    __syncthreads();
    const ToneBox mine = tone_votes(a.t, e, tid, TONE_THREADS);
    if (mine.hits) {                                       // (results unused: LDS atomics without a return value, once per thread)
        atomicAdd(&s_box[0], mine.hits);
        atomicMin(&s_box[1], mine.x0); atomicMin(&s_box[2], mine.y0);
        atomicMax(&s_box[3], mine.x1); atomicMax(&s_box[4], mine.y1);
    }
    __syncthreads();
    const ToneBox box{s_box[0], s_box[1], s_box[2], s_box[3], s_box[4]};
    if (box.hits < a.t.min_hits) return;                   // (block-uniform)
    const PageInfo pi = a.t.pageinfo[e.page];
    const int rows = tone_tile_rows(pi.sw);
    for (int j0 = 0; j0 < pi.sh; j0 += rows) {
        for (int b = tid; b < 3 * a.cells; b += TONE_THREADS) bins[b] = 0;
        __syncthreads();
        shading_map_samples(a, e, box, f, j0, j0 + rows < pi.sh ? j0 + rows : pi.sh, tid, TONE_THREADS, bins,
                            [](uint32_t* p, uint32_t v) { atomicAdd(p, v); });
        __syncthreads();
        shading_map_flush(a, tid, TONE_THREADS, bins, [](unsigned long long* p, unsigned long long v) { atomicAdd(p, v); });
        __syncthreads();
    }
    if (tid == 0) atomicAdd(a.acc + 3 * a.cells, 1ull);
}
#endif

}  // namespace slideo
#endif  // SHADING_MAP
