// yuv420.hip.h — decoded YUV 4:2:0 frames (NV12 / NV21 / I420 / YV12) -> the BGR8 image the frame pipeline reads, and what every
// kernel of the YUV door shares (yuv_sampling.hip.h, yuv_chroma.hip.h and yuv_transfer.hip.h include this file).
//
//   yuv420_to_bgr_desc_kernel<DEPTH>  one frame batch under a YUV colour description (include/slideo_amd.h "YUV colour description"):
//                                     BT.601 / BT.709, limited / full range, 8-bit samples or 16-bit containers with the value in
//                                     the top / the low 10 bits   (HBM, 8-bit: 1.5wh in, 3wh out)
//   YuvArgs, yuv_args                 the ONE argument record of the door's kernels and the one host function that fills it
//
// [OCV A.14] nearest chroma, fixed point with SHIFT 20 (recalled from color_yuv.simd.hpp, include/slideo_amd.h "YUV 4:2:0 frames"):
//   y = max(0, Y - yofs) * CY;  R = sat((y + 2^19 + CVR v) >> 20), G = sat((y + 2^19 + CVG v + CUG u) >> 20), B = sat((y + 2^19 + CUB u) >> 20)
// The coefficients are kernel arguments (SGPRs); under the default description (BT.601, limited, 8) they are cvtColor(COLOR_YUV2BGR_*)'s.
// Every coefficient of the four (matrix, range) pairs is below 2^23 in magnitude (largest: CUB of BT.709 limited, 2215014), every factor
// fits 9 signed bits (Y - yofs in 0..255, u / v in -128..127), every product fits int32 (255 * 1220945 = 3.11e8,
// 128 * 2215014 = 2.84e8) and every sum stays below 2^31 (largest: 3.11e8 + 2^19 + 2.84e8): v_mul_i32_i24 computes them exactly, at full rate.
// The per-thread arithmetic is a host + device function: tools/yuv_desc_hostcheck.cpp runs it lane by lane on the CPU.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "slideo_amd.h"

namespace slideo {

constexpr int YUV_SHIFT = 20, YUV_HALF = 1 << (YUV_SHIFT - 1);
constexpr int YUV_TX = 64, YUV_TY = 4;           // block: 64 threads along a row (4 columns each) x 4 thread rows
constexpr int YUV_S420 = 0, YUV_S422 = 1, YUV_S444 = 2, YUV_S422P = 3;          // = SLIDEO_YUV_SAMPLING_*
constexpr int YUV_D8 = 0, YUV_D10_MSB = 1, YUV_D10_LSB = 2;                     // = SLIDEO_YUV_DEPTH_*

#if defined(__HIPCC__)
#define YUV_HD __host__ __device__ __forceinline__
#else
#define YUV_HD inline
#endif

struct YuvCoef { int cy, cub, cug, cvg, cvr, yofs; };

// What every kernel of the door reads of a frame batch.  wide_y and wide_c say which wide loads the addresses allow, in the
// vocabulary of the kernel family that is launched (yuv_desc_args, yuv_sampled_args, yuv_chroma_args, yuv_transfer_args)
struct YuvArgs {
    const uint8_t* src;
    int64_t src_frame_stride;    // all strides and offsets in BYTES, whatever the container
    int64_t c_ofs;               // interleaved: the first byte of the chroma plane (min of u_offset, v_offset); planar: u_offset
    int64_t v_ofs;               // planar: v_offset
    int y_stride, uv_stride;
    int interleaved, v_first;    // uv_step == 2; and V before U (NV21)
    uint8_t* dst;                // BGR8, row stride 3w, frame stride 3wh
    int w, h;
    int wide_y, wide_c;
    int out4;                    // dword stores: dst dword-aligned and w % 4 == 0
    uint32_t sel_y;              // packed: v_perm selector of Y0 Y1 Y2 Y3 out of a thread's 8 bytes
    uint32_t sel_c;              // v_perm selector of U0 U1 V0 V1 out of the thread's 8 bytes (packed) or its first0 second0 first1 second1
};

// the largest of 8, 4, 2, 1 that divides the address of a plane's every row in every frame
inline int yuv_plane_align(const uint8_t* src, int64_t ofs, int64_t frame_stride, int stride) {
    const uint64_t v = ((uint64_t)(uintptr_t)src + (uint64_t)ofs) | (uint64_t)frame_stride | (uint64_t)(int64_t)stride;
    return v % 8 == 0 ? 8 : v % 4 == 0 ? 4 : v % 2 == 0 ? 2 : 1;
}
// an alignment as a load mode: 8 = 8-byte loads, 4 = dword loads, 0 = bytes
inline int yuv_load_mode(int align) { return align >= 8 ? 8 : align >= 4 ? 4 : 0; }

// The record for n frames in a layout yuv420_validate accepted under `sampling`, all but wide_y and wide_c, and the two alignments
// those are made of: *ay, the luma plane's (packed: the one plane's), *ac, the chroma planes' (planar: the lesser of U's and V's;
// packed: 0).  A single frame has no stride to be aligned.
inline YuvArgs yuv_args(int sampling, const uint8_t* src, int64_t src_fs, const slideo_yuv420_layout& L, int w, int h, int n, uint8_t* dst, int* ay,
                        int* ac) {
    YuvArgs a{};
    a.src = src; a.src_frame_stride = src_fs;
    a.y_stride = L.y_stride; a.uv_stride = L.uv_stride;
    a.dst = dst; a.w = w; a.h = h;
    a.out4 = (uintptr_t)dst % 4 == 0 && w % 4 == 0;
    const int64_t fs = n > 1 ? src_fs : 0;
    *ay = yuv_plane_align(src, 0, fs, L.y_stride);
    *ac = 0;
    if (sampling == SLIDEO_YUV_SAMPLING_422_PACKED) {
        const uint32_t ly = (uint32_t)((L.u_offset & 1) ^ 1), uo = (uint32_t)L.u_offset, vo = (uint32_t)L.v_offset;
        a.sel_y = ly | (ly + 2) << 8 | (ly + 4) << 16 | (ly + 6) << 24;
        a.sel_c = uo | (uo + 4) << 8 | vo << 16 | (vo + 4) << 24;
        return a;
    }
    a.interleaved = L.uv_step == 2;
    a.v_first = a.interleaved && L.v_offset < L.u_offset;
    a.c_ofs = a.interleaved ? (L.u_offset < L.v_offset ? L.u_offset : L.v_offset) : L.u_offset;
    a.v_ofs = L.v_offset;
    a.sel_c = a.v_first ? 0x02000301u : 0x03010200u;
    const int au = yuv_plane_align(src, a.c_ofs, fs, L.uv_stride), av = yuv_plane_align(src, a.v_ofs, fs, L.uv_stride);
    *ac = a.interleaved || au < av ? au : av;
    return a;
}

// yuv_desc_thread's loads.  8-bit samples: dword luma, dword (interleaved) or u16 (planar) chroma; 16-bit containers: 8-byte luma,
// dword chroma.  This family holds the frame stride to the load's size for a single frame too
inline YuvArgs yuv_desc_args(int depth, const uint8_t* src, int64_t src_fs, const slideo_yuv420_layout& L, int w, int h, int n, uint8_t* dst) {
    int ay, ac;
    YuvArgs a = yuv_args(SLIDEO_YUV_SAMPLING_420, src, src_fs, L, w, h, n, dst, &ay, &ac);
    const int B = depth == SLIDEO_YUV_DEPTH_8 ? 1 : 2, need_c = B == 2 || a.interleaved ? 4 : 2;
    a.wide_y = ay >= 4 * B && src_fs % (4 * B) == 0;
    a.wide_c = ac >= need_c && src_fs % need_c == 0;
    return a;
}

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

// sat_u8(v >> 20), clamped BEFORE the shift (same value: v < 0 -> 0, v >= 256 << 20 -> 255).  The shift-then-clamp form of two
// adjacent bytes is selected to v_ashr_pk_u8_i32, and a kernel then wrote wrong bytes on gfx950 (the packed dword's upper half
// was OR-ed in unzeroed: measured against tests/yuv420_ref.py); this form compiles to v_med3_i32 + shifts
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
YUV_HD void yuv_desc_thread(const YuvArgs& a, const YuvCoef& k, int tix, int cy, int z) {
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
// grid (ceil(ceil(w/4) / YUV_TX), ceil(h/2 / YUV_TY), n), block (YUV_TX, YUV_TY)
template <int DEPTH>
__global__ __launch_bounds__(YUV_TX * YUV_TY) void yuv420_to_bgr_desc_kernel(YuvArgs a, YuvCoef k) {
    yuv_desc_thread<DEPTH>(a, k, blockIdx.x * YUV_TX + threadIdx.x, blockIdx.y * YUV_TY + threadIdx.y, blockIdx.z);
}
#endif

}  // namespace slideo
