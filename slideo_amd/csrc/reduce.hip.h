// reduce.hip.h — the working-size reduce (include/slideo_amd.h "Working size"): BGR8 frames of sw x sh -> BGR8 frames of dw x dh as
// cv::resize(INTER_AREA) makes them [OCV A.11], in front of the frame pipeline.  A stream: 3 B in per source pixel, 3 B out per
// destination pixel, no LDS.
//
//   reduce2x2_kernel    factor 2 in x and y, ResizeAreaFast's (sum + 2) >> 2, dword loads and stores   (4K -> 1080p, 1440p -> 720p)
//   reduce_int_kernel   any integer factors: integer sum, then saturate(rint((float)sum * (1.f / area))); 2x2 as above.  Bytes: also
//                       what an unaligned 2x2 source takes
//   reduce_area_kernel  any shrink: computeResizeAreaTab weights (geom.h area_taps, both ocv.area variants), f32 accumulate along a
//                       source row, then over the rows — the order of small_image_kernel (verify.hip.h area_pixel)
//
// Every thread owns 4 destination pixels of one row (12 bytes: three dword stores where the destination is dword-aligned); grid
// (ceil(ceil(dw/4) / 64), ceil(dh / 4), n), block (64, 4).  Built with -ffp-contract=off: no product is fused into a sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bgr_store.hip.h"
#include "geom.h"

namespace slideo {

constexpr int RED_TX = 64, RED_TY = 4;

struct ReduceArgs {
    const uint8_t* src;          // BGR8 rows of src_stride bytes, frames src_frame_stride apart
    int64_t src_frame_stride;
    int src_stride;
    uint8_t* dst;                // BGR8, row stride 3 dw, frame stride 3 dw dh
    int sw, sh, dw, dh;
    int ix, iy;                  // integer factors (reduce2x2_kernel: 2, 2; reduce_int_kernel)
    float inv_area;              // 1.f / (float)(ix * iy)
    int out4;                    // dst + 12 k is dword-aligned in every row (host-checked: launch_reduce)
};

// saturate_cast<uchar>(float): cvRound (ties to even), then the clamp
__device__ __forceinline__ uint32_t red_sat_u8(float v) { return (uint32_t)min(max((int)rintf(v), 0), 255); }

// The launch guarantees (launch_reduce): sw == 2 dw, sh == 2 dh, dw % 4 == 0, src / src_stride / src_frame_stride multiples of 8,
// dst dword-aligned.  A thread reads the 8 source pixels under its 4 outputs from both rows as 3 + 3 aligned 8-byte loads (byte
// 24 k of a row) and adds the rows in 16-bit lanes: lo[j] holds bytes 4j and 4j + 2 of the row sum, hi[j] bytes 4j + 1 and 4j + 3.
__global__ __launch_bounds__(RED_TX * RED_TY) void reduce2x2_kernel(ReduceArgs a) {
    const int x0 = (blockIdx.x * RED_TX + threadIdx.x) * 4;
    const int dy = blockIdx.y * RED_TY + threadIdx.y;
    if (x0 >= a.dw || dy >= a.dh) return;
    const uint8_t* s0 = a.src + (int64_t)blockIdx.z * a.src_frame_stride + (int64_t)(2 * dy) * a.src_stride + (int64_t)x0 * 6;
    const uint2* r0 = reinterpret_cast<const uint2*>(s0);
    const uint2* r1 = reinterpret_cast<const uint2*>(s0 + a.src_stride);
    uint32_t lo[6], hi[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint2 u = r0[j], v = r1[j];
        lo[2 * j] = (u.x & 0x00FF00FFu) + (v.x & 0x00FF00FFu);
        hi[2 * j] = ((u.x >> 8) & 0x00FF00FFu) + ((v.x >> 8) & 0x00FF00FFu);
        lo[2 * j + 1] = (u.y & 0x00FF00FFu) + (v.y & 0x00FF00FFu);
        hi[2 * j + 1] = ((u.y >> 8) & 0x00FF00FFu) + ((v.y >> 8) & 0x00FF00FFu);
    }
    // column sum of byte k of the 24 (k is a constant after unrolling)
    auto col = [&](int k) -> uint32_t {
        const uint32_t t = (k & 1) ? hi[k >> 2] : lo[k >> 2];
        return (k & 2) ? t >> 16 : t & 0xFFFFu;
    };
    uint32_t p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t b = (col(6 * i) + col(6 * i + 3) + 2u) >> 2;
        const uint32_t g = (col(6 * i + 1) + col(6 * i + 4) + 2u) >> 2;
        const uint32_t r = (col(6 * i + 2) + col(6 * i + 5) + 2u) >> 2;
        p[i] = b | (g << 8) | (r << 16);
    }
    uint8_t* d = a.dst + ((int64_t)blockIdx.z * a.dh + dy) * a.dw * 3 + (int64_t)x0 * 3;
    bgr_store4(d, p, 4, true);
}

// ResizeAreaFast for any integer factors ix, iy (sw == ix dw, sh == iy dh), bytes.
__global__ __launch_bounds__(RED_TX * RED_TY) void reduce_int_kernel(ReduceArgs a) {
    const int x0 = (blockIdx.x * RED_TX + threadIdx.x) * 4;
    const int dy = blockIdx.y * RED_TY + threadIdx.y;
    if (x0 >= a.dw || dy >= a.dh) return;
    const uint8_t* f = a.src + (int64_t)blockIdx.z * a.src_frame_stride;
    const int cnt = min(4, a.dw - x0);
    const bool two = a.ix == 2 && a.iy == 2;
    uint32_t p[4] = {0, 0, 0, 0};
    for (int i = 0; i < cnt; ++i) {
        int s0 = 0, s1 = 0, s2 = 0;
        for (int yy = 0; yy < a.iy; ++yy) {
            const uint8_t* row = f + (int64_t)min((dy * a.iy + yy), a.sh - 1) * a.src_stride;
            for (int xx = 0; xx < a.ix; ++xx) {
                const uint8_t* s = row + 3 * min((x0 + i) * a.ix + xx, a.sw - 1);
                s0 += s[0]; s1 += s[1]; s2 += s[2];
            }
        }
        if (two) p[i] = (uint32_t)((s0 + 2) >> 2) | ((uint32_t)((s1 + 2) >> 2) << 8) | ((uint32_t)((s2 + 2) >> 2) << 16);
        else p[i] = red_sat_u8((float)s0 * a.inv_area) | (red_sat_u8((float)s1 * a.inv_area) << 8) | (red_sat_u8((float)s2 * a.inv_area) << 16);
    }
    uint8_t* d = a.dst + ((int64_t)blockIdx.z * a.dh + dy) * a.dw * 3 + (int64_t)x0 * 3;
    bgr_store4(d, p, cnt, a.out4 != 0);
}

// ResizeArea_Invoker: taps / idx are the class's own tables (ag's offsets index them), as build_area_geom_to made them.
__global__ __launch_bounds__(RED_TX * RED_TY) void reduce_area_kernel(ReduceArgs a, AreaGeom ag, const AreaTap* __restrict__ taps,
                                                                      const int32_t* __restrict__ idx) {
    const int x0 = (blockIdx.x * RED_TX + threadIdx.x) * 4;
    const int dy = blockIdx.y * RED_TY + threadIdx.y;
    if (x0 >= a.dw || dy >= a.dh) return;
    const uint8_t* f = a.src + (int64_t)blockIdx.z * a.src_frame_stride;
    const int cnt = min(4, a.dw - x0);
    const int yb = idx[ag.yidx_ofs + dy], ye = idx[ag.yidx_ofs + dy + 1];
    uint32_t p[4] = {0, 0, 0, 0};
    for (int i = 0; i < cnt; ++i) {
        const int xb = idx[ag.xidx_ofs + x0 + i], xe = idx[ag.xidx_ofs + x0 + i + 1];
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int j = yb; j < ye; ++j) {
            const AreaTap ty = taps[ag.ytap_ofs + j];
            const uint8_t* row = f + (int64_t)ty.si * a.src_stride;
            float b0 = 0.f, b1 = 0.f, b2 = 0.f;
            for (int k = xb; k < xe; ++k) {
                const AreaTap tx = taps[ag.xtap_ofs + k];
                const uint8_t* s = row + 3 * tx.si;
                b0 = b0 + (float)s[0] * tx.alpha; b1 = b1 + (float)s[1] * tx.alpha; b2 = b2 + (float)s[2] * tx.alpha;
            }
            if (j == yb) { s0 = ty.alpha * b0; s1 = ty.alpha * b1; s2 = ty.alpha * b2; }
            else { s0 += ty.alpha * b0; s1 += ty.alpha * b1; s2 += ty.alpha * b2; }
        }
        p[i] = red_sat_u8(s0) | (red_sat_u8(s1) << 8) | (red_sat_u8(s2) << 16);
    }
    uint8_t* d = a.dst + ((int64_t)blockIdx.z * a.dh + dy) * a.dw * 3 + (int64_t)x0 * 3;
    bgr_store4(d, p, cnt, a.out4 != 0);
}

}  // namespace slideo
