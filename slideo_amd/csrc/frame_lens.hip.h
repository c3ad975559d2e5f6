// frame_lens.hip.h — the frame lens's undistortion, fused into the rectify step (include/slideo_amd.h "Frame lens"): BGR8 frames of
// sw x sh -> the dw x dh analysed image whose pixel (x, y) is the bilinear sample of the frame at D(P(x, y)): P the ideal point —
// (x, y) itself, or the region's map M —, D the radial model c + (p - c) (1 + k1 r2 + k2 r2^2), r2 = |p - c|^2 / f^2.  No inversion
// and no iteration: the model runs in the direction the gather needs.  A stream with a gather, as rectify_kernel is: 3 B out per
// destination pixel, four taps in, no LDS, no scratch, no atomics.
//
//   lens_kernel<false>   no region: the ideal point is the destination pixel; no division
//   lens_kernel<true>    the region's M in front: N0, N1, W of the destination pixel in float64, ONE reciprocal per pixel.  Every
//                        accepted M takes this instance — an affine or translating one too: under a lens the region's own three
//                        instances are not used, and the coordinate has no column-block term (frame_region.hip.h bw0)
//
// The thread shape, the taps (aligned dwords shifted out of 64-bit pairs, never an unaligned multi-dword load), the blend and the
// store are frame_region.hip.h's, by include: rect_row_taps, rect_blend, rect_round_sat, bgr_store4.  Every source address is
// clamped to the frame (the replicate border), whatever the coordinate: a saturated or NaN coordinate reads a border pixel.
//
// The arithmetic is RECT_HD (host and device): tools/frame_lens_hostcheck.cpp runs lens_thread lane by lane on the CPU.  Every
// product and sum is rounded on its own (fp contract off), in the order the header writes them.
#pragma once
#include "frame_region.hip.h"

namespace slideo {

struct LensArgs {
    const uint8_t* src;          // BGR8 rows of src_stride bytes, frames src_frame_stride apart
    int64_t src_frame_stride;
    int src_stride;
    uint8_t* dst;                // BGR8, row stride 3 dw, frame stride 3 dw dh
    int sw, sh, dw, dh;
    int out4;                    // dst + 12 k is dword-aligned in every row (host-checked: lens_args)
    double M[9];                 // lens_kernel<true>: the region's map
    double cx, cy, q, k1, k2;    // q = 1.0 / (f * f), the host's
};

// Step 2 of the definition: where the camera sees the ideal point (u, v)
RECT_HD void lens_point(double cx, double cy, double q, double k1, double k2, double u, double v, double& xd, double& yd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dx = u - cx, dy = v - cy;
    const double r2 = (dx * dx + dy * dy) * q;
    double t = r2 * k2;
    t = k1 + t;
    t = r2 * t;
    const double g = 1.0 + t;
    xd = cx + dx * g;
    yd = cy + dy * g;
}

// Steps 1 to 3: the fixed-point source coordinate (1/32 steps) of destination pixel (x, y)
template <bool REGION>
RECT_HD void lens_coord(const LensArgs& a, int x, int y, int& X, int& Y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double u = x, v = y;
    if (REGION) {
        const double* M = a.M;
        const double N0 = (M[0] * x + M[1] * y) + M[2];
        const double N1 = (M[3] * x + M[4] * y) + M[5];
        const double W = (M[6] * x + M[7] * y) + M[8];
        const double Wi = 1.0 / W;
        u = N0 * Wi;
        v = N1 * Wi;
    }
    double xd, yd;
    lens_point(a.cx, a.cy, a.q, a.k1, a.k2, u, v, xd, yd);
    X = rect_round_sat(32.0 * xd);
    Y = rect_round_sat(32.0 * yd);
}

// The thread that owns destination pixels 4 tix .. 4 tix + 3 of row dy of frame z
template <bool REGION>
RECT_HD void lens_thread(const LensArgs& a, int tix, int dy, int z) {
    const int x0 = tix * 4;
    if (x0 >= a.dw || dy >= a.dh) return;
    const uint8_t* f = a.src + (int64_t)z * a.src_frame_stride;
    const int cnt = a.dw - x0 < 4 ? a.dw - x0 : 4;
    uint32_t p[4] = {0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        if (i < cnt) {
            int X, Y;
            lens_coord<REGION>(a, x0 + i, dy, X, Y);
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
        }
    }
    uint8_t* d = a.dst + ((int64_t)z * a.dh + dy) * a.dw * 3 + (int64_t)x0 * 3;
    bgr_store4(d, p, cnt, a.out4 != 0);
}

// The arguments of a launch (host): n frames at src -> dst; M null: no region
inline LensArgs lens_args(const double* M, double cx, double cy, double q, double k1, double k2, const uint8_t* src, int64_t src_fs, int stride,
                          int sw, int sh, uint8_t* dst, int dw, int dh) {
    LensArgs a{};
    a.src = src; a.src_frame_stride = src_fs; a.src_stride = stride;
    a.dst = dst; a.sw = sw; a.sh = sh; a.dw = dw; a.dh = dh;
    a.out4 = reinterpret_cast<uintptr_t>(dst) % 4 == 0 && dw % 4 == 0;
    for (int i = 0; i < 9; ++i) a.M[i] = M ? M[i] : (i % 4 == 0 ? 1.0 : 0.0);
    a.cx = cx; a.cy = cy; a.q = q; a.k1 = k1; a.k2 = k2;
    return a;
}

#if defined(__HIPCC__)
template <bool REGION>
__global__ __launch_bounds__(RECT_TX * RECT_TY) void lens_kernel(LensArgs a) {
    lens_thread<REGION>(a, blockIdx.x * RECT_TX + threadIdx.x, blockIdx.y * RECT_TY + threadIdx.y, blockIdx.z);
}
#endif

}  // namespace slideo
