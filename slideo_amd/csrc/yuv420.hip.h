// yuv420.hip.h — decoded YUV 4:2:0 frames (NV12 / NV21 / I420 / YV12) -> the BGR8 image the frame pipeline reads.
//
//   yuv420_to_bgr_kernel              one frame batch, cvtColor(COLOR_YUV2BGR_*) arithmetic   (HBM: 1.5wh in, 3wh out)
//   yuv420_to_bgr_desc_kernel<DEPTH>  the same under a YUV colour description: BT.709, full range, 10-bit samples (below)
//
// [OCV A.14] BT.601 limited range, nearest chroma, fixed point with SHIFT 20 (recalled from color_yuv.simd.hpp,
// include/slideo_amd.h "YUV 4:2:0 frames"):
//   y = max(0, Y - 16) * CY;  R = sat((y + 2^19 + CVR v) >> 20), G = sat((y + 2^19 + CVG v + CUG u) >> 20), B = sat((y + 2^19 + CUB u) >> 20)
// Every coefficient fits a signed 24-bit operand (|c| < 2^23) and so does every factor (Y - 16 in 0..239, u / v in -128..127), and
// every product fits int32 (239 * CY = 2.92e8, 128 * CUB = 2.71e8): v_mul_i32_i24 computes them exactly, at full rate.
// Every sum stays below 2^31 (largest: 2.92e8 + 2^19 + 2.71e8).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace slideo {

constexpr int YUV_CY = 1220542, YUV_CUB = 2116026, YUV_CUG = -409993, YUV_CVG = -852492, YUV_CVR = 1673527;
constexpr int YUV_SHIFT = 20, YUV_HALF = 1 << (YUV_SHIFT - 1);
constexpr int YUV_TX = 64, YUV_TY = 4;           // block: 64 threads along a row (4 columns each) x 4 chroma rows (2 luma rows each)

#if defined(__HIPCC__)      // (the 8-bit BT.601 limited kernel is device code only; a host build reads the description's part below)
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

#endif  // __HIPCC__

// ---- YUV colour description (include/slideo_amd.h "YUV colour description") -----------------------------------------------------
//   yuv420_to_bgr_desc_kernel<DEPTH>   the kernel above with the coefficients as kernel arguments (SGPRs) and the sample loads
//                                      templated on the container: 8-bit, or 16-bit with the value in the top / the low 10 bits
// Launched only under a non-default description (stage_orb.hip launch_yuv420_to_bgr).  Same thread shape, same stores.  Every
// coefficient of the four (matrix, range) pairs is below 2^23 in magnitude (largest: CUB of BT.709 limited, 2215014), every factor
// fits 9 signed bits (Y - y_offset in 0..255, u / v in -128..127), every product fits int32 (255 * 1220945 = 3.11e8,
// 128 * 2215014 = 2.84e8) and every sum stays below 2^31 (largest: 3.11e8 + 2^19 + 2.84e8): the 24-bit multiplies are exact.
// The per-thread arithmetic is a host + device function: tools/yuv_desc_hostcheck.cpp runs it lane by lane on the CPU.
#if defined(__HIPCC__)
#define YUV_HD __host__ __device__ __forceinline__
#else
#define YUV_HD inline
#endif

constexpr int YUV_D8 = 0, YUV_D10_MSB = 1, YUV_D10_LSB = 2;          // = SLIDEO_YUV_DEPTH_*

struct YuvCoef { int cy, cub, cug, cvg, cvr, yofs; };

struct YuvDescArgs {
    const uint8_t* src;
    int64_t src_frame_stride;    // all strides and offsets in BYTES, whatever the container
    int64_t c_ofs;               // interleaved: the first byte of the chroma plane (min of u_offset, v_offset); planar: u_offset
    int64_t v_ofs;               // planar: v_offset
    int y_stride, uv_stride;
    int interleaved, v_first;
    uint8_t* dst;                // BGR8, row stride 3w, frame stride 3wh
    int w, h;
    int wide_y;                  // a thread's 4 luma samples of a row are one aligned load (dword; 8 bytes of 16-bit containers)
    int wide_c;                  // its chroma is aligned for the wide loads of yuv_desc_thread
    int out4;                    // dword stores: dst dword-aligned and w % 4 == 0
};

YUV_HD int yuv_mul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}
// v_perm_b32: byte i of the result is byte sel[i] (0..7) of the 8 bytes hi:lo
YUV_HD uint32_t yuv_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint32_t)((v >> (8 * ((sel >> (8 * i)) & 7))) & 255) << (8 * i);
    return r;
#endif
}
// min(x, 1023) of both u16 halves (v_pk_min_u16)
YUV_HD uint32_t yuv_pkmin1023(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 lim = {1023, 1023};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, x), lim));
#else
    const uint32_t a = x & 0xffffu, b = x >> 16;
    return (a < 1023u ? a : 1023u) | ((b < 1023u ? b : 1023u) << 16);
#endif
}
// the 8-bit value of one sample at p (byte loads: any alignment)
template <int DEPTH>
YUV_HD uint32_t yuv_s8(const uint8_t* p) {
    if (DEPTH == YUV_D8) return p[0];
    if (DEPTH == YUV_D10_MSB) return p[1];                     // (little-endian container: its high byte)
    const uint32_t s = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    return (s < 1023u ? s : 1023u) >> 2;
}
// the 8-bit values of four 16-bit containers (lo: samples 0 1, hi: samples 2 3) as the bytes of one dword: a byte permute picks
// the high bytes (MSB) or, after the packed clamp and one shift per dword, bits 2..9 (LSB)
template <int DEPTH>
YUV_HD uint32_t yuv_pack4(uint32_t lo, uint32_t hi) {
    if (DEPTH == YUV_D10_MSB) return yuv_perm(hi, lo, 0x07050301u);
    return yuv_perm(yuv_pkmin1023(hi) >> 2, yuv_pkmin1023(lo) >> 2, 0x06040200u);
}
YUV_HD uint32_t yuv_ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
// four samples at p as one dword of 8-bit values: one aligned load (dword, or 8 bytes)
template <int DEPTH>
YUV_HD uint32_t yuv_load4(const uint8_t* p) {
    if (DEPTH == YUV_D8) return yuv_ld32(p);
    const uint64_t v = *reinterpret_cast<const uint64_t*>(p);
    return yuv_pack4<DEPTH>((uint32_t)v, (uint32_t)(v >> 32));
}

// sat_u8(v >> 20), clamped BEFORE the shift (yuv_sat8 above says why)
YUV_HD uint32_t yuv_desc_sat8(int v) {
    const int lim = (256 << YUV_SHIFT) - 1;
    const int c = v < 0 ? 0 : (v > lim ? lim : v);
    return (uint32_t)c >> YUV_SHIFT;
}
struct YuvDC { int r, g, b; };
YUV_HD YuvDC yuv_desc_chroma(uint32_t U, uint32_t V, const YuvCoef& k) {
    const int u = (int)U - 128, v = (int)V - 128;
    return YuvDC{YUV_HALF + yuv_mul24(k.cvr, v), YUV_HALF + yuv_mul24(k.cvg, v) + yuv_mul24(k.cug, u), YUV_HALF + yuv_mul24(k.cub, u)};
}
// one pixel as b | g << 8 | r << 16
YUV_HD uint32_t yuv_desc_px(uint32_t Y, const YuvDC& c, const YuvCoef& k) {
    const int d = (int)Y - k.yofs;
    const int y = yuv_mul24(d < 0 ? 0 : d, k.cy);
    return yuv_desc_sat8(y + c.b) | (yuv_desc_sat8(y + c.g) << 8) | (yuv_desc_sat8(y + c.r) << 16);
}

// One thread of the launch grid: columns 4 tix .. 4 tix + 3 of luma rows 2cy and 2cy + 1 of frame z.  Wide loads where the host
// found the layout aligned for them and the thread owns four columns: luma, one dword (8-bit) or one 8-byte load (16-bit) per row;
// chroma, 8-bit: one dword (interleaved) or two u16 (planar), 16-bit: two dwords (interleaved: one per U V pair; planar: U's, V's).
// Else sample by sample with byte loads.  Two 12-byte runs out, as three dwords each (out4) or as bytes.
template <int DEPTH>
YUV_HD void yuv_desc_thread(const YuvDescArgs& a, const YuvCoef& k, int tix, int cy, int z) {
    constexpr int B = DEPTH == YUV_D8 ? 1 : 2;
    const int x0 = tix * 4;
    if (x0 >= a.w || 2 * cy >= a.h) return;
    const uint8_t* f = a.src + (int64_t)z * a.src_frame_stride;
    const uint8_t* y0 = f + (int64_t)(2 * cy) * a.y_stride + (int64_t)x0 * B;
    const uint8_t* y1 = y0 + a.y_stride;
    const int64_t crow = (int64_t)cy * a.uv_stride;
    const int xc = x0 >> 1;
    const bool full = x0 + 3 < a.w;
    const int np = full ? 4 : a.w - x0;              // columns of this thread, and their chroma samples
    const int nc = (np + 1) >> 1;
    uint32_t ya = 0, yb = 0;
    if (full && a.wide_y) { ya = yuv_load4<DEPTH>(y0); yb = yuv_load4<DEPTH>(y1); }
    else
        for (int i = 0; i < np; ++i) {
            ya |= yuv_s8<DEPTH>(y0 + i * B) << (8 * i);
            yb |= yuv_s8<DEPTH>(y1 + i * B) << (8 * i);
        }
    uint32_t U0, V0, U1, V1;
    if (a.interleaved) {
        const uint8_t* p = f + a.c_ofs + crow + (int64_t)xc * 2 * B;
        uint32_t c4 = 0;                             // first0 second0 first1 second1
        if (full && a.wide_c) c4 = DEPTH == YUV_D8 ? yuv_ld32(p) : yuv_pack4<DEPTH>(yuv_ld32(p), yuv_ld32(p + 4));
        else
            for (int j = 0; j < nc; ++j) c4 |= (yuv_s8<DEPTH>(p + 2 * j * B) | (yuv_s8<DEPTH>(p + (2 * j + 1) * B) << 8)) << (16 * j);
        const uint32_t lo0 = c4 & 255, hi0 = (c4 >> 8) & 255, lo1 = (c4 >> 16) & 255, hi1 = c4 >> 24;
        U0 = a.v_first ? hi0 : lo0; V0 = a.v_first ? lo0 : hi0;
        U1 = a.v_first ? hi1 : lo1; V1 = a.v_first ? lo1 : hi1;
    } else {
        const uint8_t* pu = f + a.c_ofs + crow + (int64_t)xc * B;
        const uint8_t* pv = f + a.v_ofs + crow + (int64_t)xc * B;
        uint32_t c4 = 0;                             // U0 U1 V0 V1
        if (full && a.wide_c) {
            if (DEPTH == YUV_D8) c4 = (uint32_t)*reinterpret_cast<const uint16_t*>(pu) | ((uint32_t)*reinterpret_cast<const uint16_t*>(pv) << 16);
            else c4 = yuv_pack4<DEPTH>(yuv_ld32(pu), yuv_ld32(pv));
        } else
            for (int j = 0; j < nc; ++j) c4 |= (yuv_s8<DEPTH>(pu + j * B) << (8 * j)) | (yuv_s8<DEPTH>(pv + j * B) << (16 + 8 * j));
        U0 = c4 & 255; U1 = (c4 >> 8) & 255; V0 = (c4 >> 16) & 255; V1 = c4 >> 24;
    }
    const YuvDC k0 = yuv_desc_chroma(U0, V0, k), k1 = yuv_desc_chroma(U1, V1, k);
    uint8_t* d0 = a.dst + (int64_t)z * a.w * a.h * 3 + ((int64_t)(2 * cy) * a.w + x0) * 3;
    uint8_t* d1 = d0 + (int64_t)a.w * 3;
    if (a.out4) {                                    // (w % 4 == 0: every thread owns four columns)
        for (int r = 0; r < 2; ++r) {
            const uint32_t y4 = r ? yb : ya;
            uint32_t* d = reinterpret_cast<uint32_t*>(r ? d1 : d0);
            const uint32_t p0 = yuv_desc_px(y4 & 255, k0, k), p1 = yuv_desc_px((y4 >> 8) & 255, k0, k);
            const uint32_t p2 = yuv_desc_px((y4 >> 16) & 255, k1, k), p3 = yuv_desc_px(y4 >> 24, k1, k);
            d[0] = p0 | (p1 << 24);                  // b0 g0 r0 b1
            d[1] = (p1 >> 8) | (p2 << 16);           // g1 r1 b2 g2
            d[2] = (p2 >> 16) | (p3 << 8);           // r2 b3 g3 r3
        }
        return;
    }
    for (int i = 0; i < np; ++i) {
        const YuvDC& kc = i < 2 ? k0 : k1;
        const uint32_t pa = yuv_desc_px((ya >> (8 * i)) & 255, kc, k), pb = yuv_desc_px((yb >> (8 * i)) & 255, kc, k);
        d0[3 * i] = (uint8_t)pa; d0[3 * i + 1] = (uint8_t)(pa >> 8); d0[3 * i + 2] = (uint8_t)(pa >> 16);
        d1[3 * i] = (uint8_t)pb; d1[3 * i + 1] = (uint8_t)(pb >> 8); d1[3 * i + 2] = (uint8_t)(pb >> 16);
    }
}

#if defined(__HIPCC__)
// grid and block of yuv420_to_bgr_kernel
template <int DEPTH>
__global__ __launch_bounds__(YUV_TX * YUV_TY) void yuv420_to_bgr_desc_kernel(YuvDescArgs a, YuvCoef k) {
    yuv_desc_thread<DEPTH>(a, k, blockIdx.x * YUV_TX + threadIdx.x, blockIdx.y * YUV_TY + threadIdx.y, blockIdx.z);
}
#endif

}  // namespace slideo
