// yuv420.hip.h — decoded YUV 4:2:0 frames (NV12 / NV21 / I420 / YV12) -> the BGR8 image the frame pipeline reads.
//
//   yuv420_to_bgr_kernel   one frame batch, cvtColor(COLOR_YUV2BGR_*) arithmetic   (HBM: 1.5wh in, 3wh out)
//
// [OCV A.14] BT.601 limited range, nearest chroma, fixed point with SHIFT 20 (recalled from color_yuv.simd.hpp,
// include/slideo_amd.h "YUV 4:2:0 frames"):
//   y = max(0, Y - 16) * CY;  R = sat((y + 2^19 + CVR v) >> 20), G = sat((y + 2^19 + CVG v + CUG u) >> 20), B = sat((y + 2^19 + CUB u) >> 20)
// Every coefficient fits a signed 24-bit operand (|c| < 2^23) and so does every factor (Y - 16 in 0..239, u / v in -128..127), and
// every product fits int32 (239 * CY = 2.92e8, 128 * CUB = 2.71e8): v_mul_i32_i24 computes them exactly, at full rate.
// Every sum stays below 2^31 (largest: 2.92e8 + 2^19 + 2.71e8).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slideo {

constexpr int YUV_CY = 1220542, YUV_CUB = 2116026, YUV_CUG = -409993, YUV_CVG = -852492, YUV_CVR = 1673527;
constexpr int YUV_SHIFT = 20, YUV_HALF = 1 << (YUV_SHIFT - 1);
constexpr int YUV_TX = 64, YUV_TY = 4;           // block: 64 threads along a row (4 columns each) x 4 chroma rows (2 luma rows each)

struct Yuv420Args {
    const uint8_t* src;
    int64_t src_frame_stride;
    int64_t c_ofs;           // uv_step 2: the first byte of the interleaved chroma plane (min of u_offset, v_offset); 1: u_offset
    int64_t v_ofs;           // uv_step 1: v_offset
    int y_stride, uv_stride;
    int interleaved;         // uv_step == 2
    int v_first;             // interleaved with V before U (NV21)
    uint8_t* dst;            // BGR8, row stride 3w, frame stride 3wh
    int w, h;
    int fast;                // dword loads / stores are aligned where x % 4 == 0 (host-checked, see launch_yuv420_to_bgr)
};

// sat_u8(v >> 20), clamped BEFORE the shift (same value: v < 0 -> 0, v >= 256 << 20 -> 255).  The shift-then-clamp form of two
// adjacent bytes is selected to v_ashr_pk_u8_i32, and the kernel then wrote wrong bytes on gfx950 (the packed dword's upper half
// was OR-ed in unzeroed: measured against tests/yuv420_ref.py); this form compiles to v_med3_i32 + shifts
__device__ __forceinline__ uint32_t yuv_sat8(int v) { return (uint32_t)min(max(v, 0), (256 << YUV_SHIFT) - 1) >> YUV_SHIFT; }

// chroma terms of one sample (the rounding half folded in)
struct YuvC { int r, g, b; };
__device__ __forceinline__ YuvC yuv_chroma(uint32_t U, uint32_t V) {
    const int u = (int)U - 128, v = (int)V - 128;
    return YuvC{YUV_HALF + __mul24(YUV_CVR, v), YUV_HALF + __mul24(YUV_CVG, v) + __mul24(YUV_CUG, u), YUV_HALF + __mul24(YUV_CUB, u)};
}

// one pixel as b | g << 8 | r << 16
__device__ __forceinline__ uint32_t yuv_px(uint32_t Y, const YuvC& c) {
    const int y = __mul24(max((int)Y - 16, 0), YUV_CY);
    return yuv_sat8(y + c.b) | (yuv_sat8(y + c.g) << 8) | (yuv_sat8(y + c.r) << 16);
}

// 4 pixels (b g r each, 12 bytes) of one row from a luma dword and the two chroma samples they share in pairs, stored as 3 dwords
__device__ __forceinline__ void yuv_row4(uint32_t* __restrict__ d, uint32_t y4, const YuvC& c0, const YuvC& c1) {
    const uint32_t p0 = yuv_px(y4 & 255, c0), p1 = yuv_px((y4 >> 8) & 255, c0);
    const uint32_t p2 = yuv_px((y4 >> 16) & 255, c1), p3 = yuv_px(y4 >> 24, c1);
    d[0] = p0 | (p1 << 24);                       // b0 g0 r0 b1
    d[1] = (p1 >> 8) | (p2 << 16);                // g1 r1 b2 g2
    d[2] = (p2 >> 16) | (p3 << 8);                // r2 b3 g3 r3
}

// grid (ceil(ceil(w/4) / 64), ceil(h/2 / 4), n), block (64, 4).  A thread converts columns x0 .. x0+3 of luma rows 2cy and 2cy+1
// (chroma row cy): two luma dwords and one chroma dword (interleaved) or two chroma u16 (planar) in, two 12-byte BGR runs out.
__global__ __launch_bounds__(YUV_TX * YUV_TY) void yuv420_to_bgr_kernel(Yuv420Args a) {
    const int x0 = (blockIdx.x * YUV_TX + threadIdx.x) * 4;
    const int cy = blockIdx.y * YUV_TY + threadIdx.y;
    if (x0 >= a.w || 2 * cy >= a.h) return;
    const uint8_t* f = a.src + (int64_t)blockIdx.z * a.src_frame_stride;
    const uint8_t* y0 = f + (int64_t)(2 * cy) * a.y_stride;
    const uint8_t* y1 = y0 + a.y_stride;
    const uint8_t* c = f + a.c_ofs + (int64_t)cy * a.uv_stride;
    const uint8_t* cv = f + a.v_ofs + (int64_t)cy * a.uv_stride;          // (planar only)
    uint8_t* d0 = a.dst + (int64_t)blockIdx.z * a.w * a.h * 3 + ((int64_t)(2 * cy) * a.w + x0) * 3;
    uint8_t* d1 = d0 + (int64_t)a.w * 3;
    if (a.fast && x0 + 3 < a.w) {
        uint32_t U0, V0, U1, V1;
        if (a.interleaved) {
            const uint32_t c4 = *reinterpret_cast<const uint32_t*>(c + x0);          // chroma pairs x0/2 and x0/2 + 1
            const uint32_t lo0 = c4 & 255, hi0 = (c4 >> 8) & 255, lo1 = (c4 >> 16) & 255, hi1 = c4 >> 24;
            U0 = a.v_first ? hi0 : lo0; V0 = a.v_first ? lo0 : hi0;
            U1 = a.v_first ? hi1 : lo1; V1 = a.v_first ? lo1 : hi1;
        } else {
            const uint32_t u2 = *reinterpret_cast<const uint16_t*>(c + x0 / 2);
            const uint32_t v2 = *reinterpret_cast<const uint16_t*>(cv + x0 / 2);
            U0 = u2 & 255; U1 = u2 >> 8; V0 = v2 & 255; V1 = v2 >> 8;
        }
        const YuvC k0 = yuv_chroma(U0, V0), k1 = yuv_chroma(U1, V1);
        const uint32_t ya = *reinterpret_cast<const uint32_t*>(y0 + x0);
        const uint32_t yb = *reinterpret_cast<const uint32_t*>(y1 + x0);
        yuv_row4(reinterpret_cast<uint32_t*>(d0), ya, k0, k1);
        yuv_row4(reinterpret_cast<uint32_t*>(d1), yb, k0, k1);
        return;
    }
    // bytes: unaligned layouts, widths that are not a multiple of 4, the last columns of a row
    for (int i = 0; i < 4 && x0 + i < a.w; ++i) {
        const int xc = (x0 + i) >> 1;
        uint32_t U, V;
        if (a.interleaved) {
            const uint8_t* p = c + 2 * xc;
            U = a.v_first ? p[1] : p[0]; V = a.v_first ? p[0] : p[1];
        } else {
            U = c[xc]; V = cv[xc];
        }
        const YuvC k = yuv_chroma(U, V);
        const uint32_t pa = yuv_px(y0[x0 + i], k), pb = yuv_px(y1[x0 + i], k);
        d0[3 * i] = (uint8_t)pa; d0[3 * i + 1] = (uint8_t)(pa >> 8); d0[3 * i + 2] = (uint8_t)(pa >> 16);
        d1[3 * i] = (uint8_t)pb; d1[3 * i + 1] = (uint8_t)(pb >> 8); d1[3 * i + 2] = (uint8_t)(pb >> 16);
    }
}

}  // namespace slideo
