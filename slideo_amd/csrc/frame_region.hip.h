// frame_region.hip.h — the frame region's rectify (include/slideo_amd.h "Frame region"): BGR8 frames of sw x sh -> the dw x dh
// image cv::warpPerspective(frame, M, Size(dw, dh), INTER_LINEAR | WARP_INVERSE_MAP, BORDER_REPLICATE) makes of them [OCV A.12],
// in front of the frame pipeline.  A stream with a gather: 3 B out per destination pixel, four taps in per destination pixel, no LDS.
//
//   rectify_kernel<RECT_PROJECTIVE>   any accepted M: the coordinate of every destination pixel in float64, one division each
//   rectify_kernel<RECT_AFFINE>       M6 = M7 = 0: W0 = M6*xb + M7*y + M8 is (+-0) + (+-0) + M8 = M8 and W = M8 + M6*x1 = M8, whatever
//                                     x and y are (x + (+-0) == x for x != 0, and M8 != 0 is a set-time rule), so the definition's
//                                     32.0 / W is the ONE correctly rounded quotient 32.0 / M8: the host divides once, the same bits
//   rectify_kernel<RECT_TRANSLATE>    M = [1 0 tx; 0 1 ty; 0 0 1], tx and ty integers: X = 32 (x + tx) exactly, ax = ay = 0, the
//                                     blend is (p00 * 1024 + 512) >> 10 = p00: a clamped copy, three dword loads where the source
//                                     is dword-aligned and the four pixels lie inside the row
//
// Every thread owns 4 destination pixels of one row (12 bytes: three dword stores where the destination is dword-aligned, bytes
// otherwise: the reduce kernels' store pattern); grid (ceil(ceil(dw/4) / 64), ceil(dh / 4), n), block (64, 4).
//
// The taps.  The left and right tap of a source row are 6 contiguous bytes at row + 3 sx, an address of any byte alignment.  An
// unaligned multi-dword load is split by the texture path (README round 5), so the kernel never issues one: it loads the ALIGNED
// dwords that overlap the 6 bytes — two, and a third only when the address is 3 mod 4 — and shifts the bytes out of the 64-bit
// pairs.  Every dword loaded holds at least one byte of the frame, so no load leaves the allocation's last dword.  Where the
// replicate clamp makes both taps the same pixel (sx < 0, sx >= sw - 1) the three bytes are loaded as bytes.
//
// The arithmetic is RECT_HD (host and device): tools/frame_region_hostcheck.cpp runs rectify_thread lane by lane on the CPU.
// Built with -ffp-contract=off, and the coordinate code says so itself: every product and sum is rounded on its own.
#pragma once
#include <stdint.h>

#include <cmath>

#include "bgr_store.hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RECT_HD __host__ __device__ __forceinline__
#else
#define RECT_HD inline
#endif

namespace slideo {

constexpr int RECT_TX = 64, RECT_TY = 4;
constexpr int RECT_PROJECTIVE = 0, RECT_AFFINE = 1, RECT_TRANSLATE = 2;

struct RectifyArgs {
    const uint8_t* src;          // BGR8 rows of src_stride bytes, frames src_frame_stride apart
    int64_t src_frame_stride;
    int src_stride;
    uint8_t* dst;                // BGR8, row stride 3 dw, frame stride 3 dw dh
    int sw, sh, dw, dh;
    int bw0;                     // the column block of warpPerspective's invoker (rect_bw0)
    int out4;                    // dst + 12 k is dword-aligned in every row (host-checked: launch_rectify)
    int in4;                     // RECT_TRANSLATE: src + 3 (x + tx) is dword-aligned at every x % 4 == 0 of every row
    int tx, ty;                  // RECT_TRANSLATE
    double M[9];
    double w_affine;             // RECT_AFFINE: 32.0 / M[8]
};

RECT_HD int rect_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bw0 of WarpPerspectiveInvoker (BLOCK_SZ 32): the x of a block's first column enters the coordinate on its own
RECT_HD int rect_bw0(int dw, int dh) {
    const int bh0 = dh < 16 ? (dh > 1 ? dh : 1) : 16;
    const int b = 1024 / bh0 < dw ? 1024 / bh0 : dw;
    return b > 1 ? b : 1;
}

RECT_HD int rect_round_sat(double v) {
    const double lo = -2147483648.0, hi = 2147483647.0;
    v = v < hi ? v : hi;                 // (v is never NaN: M is finite and W != 0 over the destination, set-time rules)
    v = v > lo ? v : lo;
    return (int)rint(v);
}

// The fixed-point source coordinate (1/32 steps) of destination pixel (xb + x1, y); xb = the first column of the pixel's block
template <int KIND>
RECT_HD void rect_coord(const RectifyArgs& a, int xb, int x1, int y, int& X, int& Y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double* M = a.M;
    const double X0 = M[0] * xb + M[1] * y + M[2], Y0 = M[3] * xb + M[4] * y + M[5];
    double W;
    if (KIND == RECT_AFFINE) {
        W = a.w_affine;
    } else {
        const double W0 = M[6] * xb + M[7] * y + M[8];
        W = W0 + M[6] * x1;
        W = W != 0.0 ? 32.0 / W : 0.0;
    }
    X = rect_round_sat((X0 + M[0] * x1) * W);
    Y = rect_round_sat((Y0 + M[3] * x1) * W);
}

// the taps (xa, xc) of one source row as b | g << 8 | r << 16 each; xc is xa + 1, or xa where the clamp folds them
RECT_HD void rect_row_taps(const uint8_t* row, int xa, int xc, uint32_t& pa, uint32_t& pc) {
    const uint8_t* s = row + 3 * (int64_t)xa;
    if (xc != xa) {
        const uintptr_t ad = reinterpret_cast<uintptr_t>(s);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(ad & ~(uintptr_t)3);
        const unsigned sh = (unsigned)(ad & 3) * 8;
        const uint32_t d0 = q[0], d1 = q[1];
        const uint32_t d2 = sh == 24 ? q[2] : 0u;           // bytes 4, 5 of the six reach the third dword at offset 3 only
        const uint32_t w0 = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
        const uint32_t w1 = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
        pa = w0 & 0x00FFFFFFu;
        pc = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
    } else {
        pa = pc = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
    }
}

// one channel of the bilinear table's blend: the weights at 1/32 steps are exact integers of sum 1024
RECT_HD uint32_t rect_blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, int shift, uint32_t w00, uint32_t w01, uint32_t w10,
                            uint32_t w11) {
    return (((p00 >> shift) & 0xFFu) * w00 + ((p01 >> shift) & 0xFFu) * w01 + ((p10 >> shift) & 0xFFu) * w10 + ((p11 >> shift) & 0xFFu) * w11 +
            512u) >> 10;
}

// The thread that owns destination pixels 4 tix .. 4 tix + 3 of row dy of frame z
template <int KIND>
RECT_HD void rectify_thread(const RectifyArgs& a, int tix, int dy, int z) {
    const int x0 = tix * 4;
    if (x0 >= a.dw || dy >= a.dh) return;
    const uint8_t* f = a.src + (int64_t)z * a.src_frame_stride;
    const int cnt = a.dw - x0 < 4 ? a.dw - x0 : 4;
    uint32_t p[4] = {0, 0, 0, 0};
    if (KIND == RECT_TRANSLATE) {
        const uint8_t* row = f + (int64_t)rect_clamp(dy + a.ty, 0, a.sh - 1) * a.src_stride;
        const int s0 = x0 + a.tx;
        if (a.in4 && cnt == 4 && s0 >= 0 && s0 + 3 <= a.sw - 1) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(row + 3 * (int64_t)s0);
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
            p[0] = d0 & 0x00FFFFFFu; p[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8); p[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16); p[3] = d2 >> 8;
        } else {
            for (int i = 0; i < cnt; ++i) {
                const uint8_t* s = row + 3 * (int64_t)rect_clamp(s0 + i, 0, a.sw - 1);
                p[i] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
            }
        }
    } else {
        int xb = (x0 / a.bw0) * a.bw0, x1 = x0 - xb;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 4; ++i) {
            if (i < cnt) {
                int X, Y;
                rect_coord<KIND>(a, xb, x1, dy, X, Y);
                const int sx = X >> 5, sy = Y >> 5;
                const uint32_t ax = (uint32_t)(X & 31), ay = (uint32_t)(Y & 31);
                const int xa = rect_clamp(sx, 0, a.sw - 1), xc = rect_clamp(sx + 1, 0, a.sw - 1);     // (sx + 1 never wraps: |X| <= 2^31)
                const int ya = rect_clamp(sy, 0, a.sh - 1), yc = rect_clamp(sy + 1, 0, a.sh - 1);
                uint32_t p00, p01, p10, p11;
                rect_row_taps(f + (int64_t)ya * a.src_stride, xa, xc, p00, p01);
                rect_row_taps(f + (int64_t)yc * a.src_stride, xa, xc, p10, p11);
                const uint32_t w00 = (32u - ax) * (32u - ay), w01 = ax * (32u - ay), w10 = (32u - ax) * ay, w11 = ax * ay;
                p[i] = rect_blend(p00, p01, p10, p11, 0, w00, w01, w10, w11) | (rect_blend(p00, p01, p10, p11, 8, w00, w01, w10, w11) << 8) |
                       (rect_blend(p00, p01, p10, p11, 16, w00, w01, w10, w11) << 16);
                if (++x1 == a.bw0) { xb += a.bw0; x1 = 0; }
            }
        }
    }
    uint8_t* d = a.dst + ((int64_t)z * a.dh + dy) * a.dw * 3 + (int64_t)x0 * 3;
    bgr_store4(d, p, cnt, a.out4 != 0);
}

// The instance of a map (host): an integer translation (a copy), an affine map (W constant), or the projective kernel
inline int rect_classify(const double* M, int& tx, int& ty) {
    tx = ty = 0;
    if (M[6] != 0.0 || M[7] != 0.0) return RECT_PROJECTIVE;
    const double lim = 1048576.0;           // (far beyond any frame: the translation travels as int)
    if (M[0] == 1.0 && M[1] == 0.0 && M[3] == 0.0 && M[4] == 1.0 && M[8] == 1.0 && std::fabs(M[2]) <= lim && std::fabs(M[5]) <= lim &&
        M[2] == std::rint(M[2]) && M[5] == std::rint(M[5])) {
        tx = (int)M[2]; ty = (int)M[5];
        return RECT_TRANSLATE;
    }
    return RECT_AFFINE;
}

// The arguments of a launch (host): n frames at src -> dst under M, instance `kind` with its translation
inline RectifyArgs rect_args(const double* M, int kind, int tx, int ty, const uint8_t* src, int64_t src_fs, int stride, int sw, int sh,
                             uint8_t* dst, int dw, int dh) {
    RectifyArgs a{};
    a.src = src; a.src_frame_stride = src_fs; a.src_stride = stride;
    a.dst = dst; a.sw = sw; a.sh = sh; a.dw = dw; a.dh = dh;
    a.bw0 = rect_bw0(dw, dh);
    a.out4 = reinterpret_cast<uintptr_t>(dst) % 4 == 0 && dw % 4 == 0;
    a.tx = tx; a.ty = ty;
    a.in4 = kind == RECT_TRANSLATE && reinterpret_cast<uintptr_t>(src) % 4 == 0 && stride % 4 == 0 && src_fs % 4 == 0 && tx % 4 == 0;
    for (int i = 0; i < 9; ++i) a.M[i] = M[i];
    a.w_affine = M[8] != 0.0 ? 32.0 / M[8] : 0.0;
    return a;
}

#if defined(__HIPCC__)
template <int KIND>
__global__ __launch_bounds__(RECT_TX * RECT_TY) void rectify_kernel(RectifyArgs a) {
    rectify_thread<KIND>(a, blockIdx.x * RECT_TX + threadIdx.x, blockIdx.y * RECT_TY + threadIdx.y, blockIdx.z);
}
#endif

}  // namespace slideo
