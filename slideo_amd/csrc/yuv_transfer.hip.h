// yuv_transfer.hip.h — decoded 10-bit HLG / PQ BT.2020 frames (4:2:0, 4:2:2, 4:4:4) -> the SDR BGR8 image the frame pipeline reads
// (include/slideo_amd.h "YUV transfer").
//
//   yuv_transfer_to_bgr_kernel<SAMPLING, DEPTH>   one frame batch under the matcher's transfer, range and depth
//                                                  (HBM: the bytes of the nearest 10-bit kernels: 3wh / 4wh / 6wh in, 3wh out)
// Launched iff the transfer is not SDR (stage_orb.hip launch_yuv420_to_bgr); six instances: 420, 422 and 444 at the two 10-bit
// depths.  Per pixel, in exact integers (the header's steps 1-5): the samples at their full 10 bits, the BT.2020 matrix at SHIFT 18
// (coefficients and the gamut's nine integers as kernel arguments, SGPRs; every operand fits 24 signed bits, every product and sum
// int32: 959 * 306134 = 2.94e8, 512 * 563104 = 2.88e8, their sum + 2^17 = 5.82e8; 27206 * 16383 = 4.46e8), clamp BEFORE the shift
// (yuv420.hip.h yuv_desc_sat8 says why), three reads of LIN (uint16 [1024]), nine 24-bit multiplies, three reads of OUT (uint8 [4096]).
// Both tables live in LDS: the matcher's device copy (LIN then OUT, 6144 bytes = 1536 dwords) is loaded once per block with
// cooperative 16-byte loads and one barrier BEFORE any thread leaves, so every thread of the block reaches the barrier; a block then
// converts YUV_TRK_ROWS thread rows one after the other.  Neighbouring lanes of a slide mostly read the same entries, which the LDS
// broadcasts.
// Thread shapes, loads and stores are the nearest kernels': 2 rows x 4 columns under 4:2:0 (yuv420.hip.h), four pixels of one row
// under 4:2:2 and 4:4:4 (yuv_sampling.hip.h); block YUV_TX x YUV_TY, YUV_TRK_ROWS times.  Loads, each plane's path chosen by the
// host from the addresses (yuv_transfer_args over yuv420.hip.h's yuv_args): 8 = 8-byte loads, 4 = dword loads kept apart (yuv_apart), 0 = sample
// by sample with byte loads — so are the ragged last columns of a row.  No multi-dword load is ever issued at an address that is
// not a multiple of its size.
//   luma                          4 containers, 8 bytes
//   420 / 422 planar chroma       2 containers per plane: one dword (modes 8 and 4)
//   420 / 422 interleaved chroma  2 pairs, 8 bytes
//   444 planar chroma             as luma, per plane
//   444 interleaved chroma        4 pairs, 16 bytes: two 8-byte loads or four dwords
// 12 bytes out per row as three dwords where the destination is dword-aligned and w % 4 == 0, bytes otherwise.
// The full-precision extraction is new (yuv_s10); yuv_pack4 of the other kernels narrows to 8 bits, which this one must not.
// The per-thread body is a host + device function: tools/yuv_transfer_hostcheck.cpp runs it lane by lane on the CPU, the tables a
// plain array argument.
#pragma once
#include "slideo_amd.h"
#include "yuv_sampling.hip.h"

#ifndef YUV_TRANSFER_HIT        // (tools/yuv_transfer_hostcheck.cpp counts the paths a run took)
#define YUV_TRANSFER_HIT(path)
#endif

namespace slideo {

constexpr int YUV_TRK_SHIFT = 18, YUV_TRK_HALF = 1 << (YUV_TRK_SHIFT - 1);
constexpr int YUV_TRK_LIN_BYTES = 2048, YUV_TRK_OUT_BYTES = 4096, YUV_TRK_DWORDS = (YUV_TRK_LIN_BYTES + YUV_TRK_OUT_BYTES) / 4;

// step 2's integers and step 4's, as the kernel takes them
struct YuvTransferCoef { int cy, cub, cug, cvg, cvr, yofs; int g[9]; };

// The kernel's arguments for n frames in a layout yuv420_validate accepted under (sampling, a 10-bit depth): yuv_args' record with
// this family's wide_y and wide_c, each 8 / 4 / 0: the load mode of the table above
inline YuvArgs yuv_transfer_args(int sampling, const uint8_t* src, int64_t src_fs, const slideo_yuv420_layout& L, int w, int h, int n, uint8_t* dst) {
    int ay, ac;
    YuvArgs a = yuv_args(sampling, src, src_fs, L, w, h, n, dst, &ay, &ac);
    a.wide_y = yuv_load_mode(ay);
    a.wide_c = yuv_load_mode(ac);
    return a;
}

// step 1: the 10-bit sample of a 16-bit container
template <int DEPTH>
YUV_HD int yuv_s10(uint32_t c16) {
    if (DEPTH == YUV_D10_MSB) return (int)(c16 >> 6);
    return (int)(c16 < 1023u ? c16 : 1023u);
}
// the container at p (byte loads: any alignment)
YUV_HD uint32_t yuv_c16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
// NDW (2 or 4) dwords at p under load mode 8 (8-byte loads) or 4 (dword loads), every load after the first kept apart from it
template <int NDW>
YUV_HD void yuv_transfer_ld(const uint8_t* p, int mode, uint32_t* q) {
    if (mode == 8) {
        for (int i = 0; i < NDW / 2; ++i) {
            const uint64_t v = yuv_ld64(i ? yuv_apart(p, 8 * i) : p);
            q[2 * i] = (uint32_t)v; q[2 * i + 1] = (uint32_t)(v >> 32);
        }
    } else
        for (int i = 0; i < NDW; ++i) q[i] = yuv_ld32(i ? yuv_apart(p, 4 * i) : p);
}

// clamp(v >> 18, 0, 1023) and clamp(v >> 14, 0, 16383), clamped before the shift (the same values)
YUV_HD int yuv_transfer_code(int v) {
    const int lim = (1024 << YUV_TRK_SHIFT) - 1;
    return (v < 0 ? 0 : (v > lim ? lim : v)) >> YUV_TRK_SHIFT;
}
YUV_HD int yuv_transfer_lin14(int v) {
    const int lim = (16384 << 14) - 1;
    return (v < 0 ? 0 : (v > lim ? lim : v)) >> 14;
}
// chroma terms of one chroma sample (the rounding half folded in)
YUV_HD YuvDC yuv_transfer_chroma(int U10, int V10, const YuvTransferCoef& k) {
    const int u = U10 - 512, v = V10 - 512;
    return YuvDC{YUV_TRK_HALF + yuv_mul24(k.cvr, v), YUV_TRK_HALF + yuv_mul24(k.cvg, v) + yuv_mul24(k.cug, u), YUV_TRK_HALF + yuv_mul24(k.cub, u)};
}
// one pixel as b | g << 8 | r << 16: steps 2-5
YUV_HD uint32_t yuv_transfer_px(int Y10, const YuvDC& c, const YuvTransferCoef& k, const uint16_t* lin, const uint8_t* out) {
    const int d = Y10 - k.yofs;
    const int y = yuv_mul24(d < 0 ? 0 : d, k.cy);
    const int lr = lin[yuv_transfer_code(y + c.r)], lg = lin[yuv_transfer_code(y + c.g)], lb = lin[yuv_transfer_code(y + c.b)];
    const int rnd = 1 << 13;
    const int o_r = yuv_transfer_lin14(yuv_mul24(k.g[0], lr) + yuv_mul24(k.g[1], lg) + yuv_mul24(k.g[2], lb) + rnd);
    const int o_g = yuv_transfer_lin14(yuv_mul24(k.g[3], lr) + yuv_mul24(k.g[4], lg) + yuv_mul24(k.g[5], lb) + rnd);
    const int o_b = yuv_transfer_lin14(yuv_mul24(k.g[6], lr) + yuv_mul24(k.g[7], lg) + yuv_mul24(k.g[8], lb) + rnd);
    const int ir = (o_r + 2) >> 2, ig = (o_g + 2) >> 2, ib = (o_b + 2) >> 2;
    return (uint32_t)out[ib > 4095 ? 4095 : ib] | ((uint32_t)out[ig > 4095 ? 4095 : ig] << 8) | ((uint32_t)out[ir > 4095 ? 4095 : ir] << 16);
}

// One thread of the launch grid: columns 4 tix .. 4 tix + 3 of luma rows 2 row and 2 row + 1 (420) or of luma row `row` (422, 444)
// of frame z.  lin, out: the two tables (device: LDS)
template <int SAMPLING, int DEPTH>
YUV_HD void yuv_transfer_thread(const YuvArgs& a, const YuvTransferCoef& k, const uint16_t* lin, const uint8_t* out, int tix, int row, int z) {
    constexpr bool S420 = SAMPLING == YUV_S420, S444 = SAMPLING == YUV_S444;
    constexpr int NR = S420 ? 2 : 1;                 // luma rows of this thread
    constexpr int NCS = S444 ? 4 : 2;                // chroma samples of a full thread, per plane
    const int x0 = tix * 4, r0 = S420 ? 2 * row : row;
    if (x0 >= a.w || r0 >= a.h) return;
    const uint8_t* f = a.src + (int64_t)z * a.src_frame_stride;
    const bool full = x0 + 3 < a.w;
    const int np = full ? 4 : a.w - x0;              // columns of this thread
    const int nc = S444 ? np : (np + 1) >> 1;        // its chroma samples, per plane
    int Y[NR][4] = {}, U[NCS] = {}, V[NCS] = {};
    const uint8_t* py = f + (int64_t)r0 * a.y_stride + (int64_t)x0 * 2;
    if (full && a.wide_y) {
        if (a.wide_y == 8) YUV_TRANSFER_HIT(y8); else YUV_TRANSFER_HIT(y4);
        for (int r = 0; r < NR; ++r) {
            uint32_t q[2];
            yuv_transfer_ld<2>(py + (int64_t)r * a.y_stride, a.wide_y, q);
            Y[r][0] = yuv_s10<DEPTH>(q[0] & 0xffffu); Y[r][1] = yuv_s10<DEPTH>(q[0] >> 16);
            Y[r][2] = yuv_s10<DEPTH>(q[1] & 0xffffu); Y[r][3] = yuv_s10<DEPTH>(q[1] >> 16);
        }
    } else {
        YUV_TRANSFER_HIT(y_bytes);
        for (int r = 0; r < NR; ++r)
            for (int i = 0; i < 4; ++i) if (i < np) Y[r][i] = yuv_s10<DEPTH>(yuv_c16(py + (int64_t)r * a.y_stride + i * 2));
    }
    const int xc = S444 ? x0 : x0 >> 1;
    const int64_t crow = (int64_t)row * a.uv_stride;         // (420: chroma row `row`; 422, 444: the luma row's)
    if (a.interleaved) {
        const uint8_t* p = f + a.c_ofs + crow + (int64_t)xc * 4;
        int F[NCS] = {}, S[NCS] = {};                // the first and the second sample of every pair
        if (full && a.wide_c) {
            if (a.wide_c == 8) YUV_TRANSFER_HIT(c8); else YUV_TRANSFER_HIT(c4);
            uint32_t q[NCS];
            yuv_transfer_ld<NCS>(p, a.wide_c, q);
            for (int j = 0; j < NCS; ++j) { F[j] = yuv_s10<DEPTH>(q[j] & 0xffffu); S[j] = yuv_s10<DEPTH>(q[j] >> 16); }
        } else {
            YUV_TRANSFER_HIT(c_bytes);
            for (int j = 0; j < NCS; ++j)
                if (j < nc) { F[j] = yuv_s10<DEPTH>(yuv_c16(p + 4 * j)); S[j] = yuv_s10<DEPTH>(yuv_c16(p + 4 * j + 2)); }
        }
        for (int j = 0; j < NCS; ++j) { U[j] = a.v_first ? S[j] : F[j]; V[j] = a.v_first ? F[j] : S[j]; }
    } else {
        const uint8_t* pu = f + a.c_ofs + crow + (int64_t)xc * 2;
        const uint8_t* pv = f + a.v_ofs + crow + (int64_t)xc * 2;
        if (full && a.wide_c) {
            if (a.wide_c == 8) YUV_TRANSFER_HIT(c8); else YUV_TRANSFER_HIT(c4);
            uint32_t qu[2], qv[2];
            if (S444) { yuv_transfer_ld<2>(pu, a.wide_c, qu); yuv_transfer_ld<2>(pv, a.wide_c, qv); }
            else { qu[0] = yuv_ld32(pu); qv[0] = yuv_ld32(pv); qu[1] = qv[1] = 0u; }
            for (int j = 0; j < NCS; ++j) {
                U[j] = yuv_s10<DEPTH>(j & 1 ? qu[j >> 1] >> 16 : qu[j >> 1] & 0xffffu);
                V[j] = yuv_s10<DEPTH>(j & 1 ? qv[j >> 1] >> 16 : qv[j >> 1] & 0xffffu);
            }
        } else {
            YUV_TRANSFER_HIT(c_bytes);
            for (int j = 0; j < NCS; ++j)
                if (j < nc) { U[j] = yuv_s10<DEPTH>(yuv_c16(pu + 2 * j)); V[j] = yuv_s10<DEPTH>(yuv_c16(pv + 2 * j)); }
        }
    }
    YuvDC kc[4];                                     // the chroma terms of the four columns
    if (S444) { for (int i = 0; i < 4; ++i) kc[i] = yuv_transfer_chroma(U[i], V[i], k); }
    else { kc[0] = kc[1] = yuv_transfer_chroma(U[0], V[0], k); kc[2] = kc[3] = yuv_transfer_chroma(U[1], V[1], k); }
    uint8_t* d0 = a.dst + (int64_t)z * a.w * a.h * 3 + ((int64_t)r0 * a.w + x0) * 3;
    for (int r = 0; r < NR; ++r) {
        uint8_t* d = d0 + (int64_t)r * a.w * 3;
        if (a.out4) {                                // (w % 4 == 0: every thread owns four columns)
            if (r == 0) YUV_TRANSFER_HIT(out4);
            const uint32_t p0 = yuv_transfer_px(Y[r][0], kc[0], k, lin, out), p1 = yuv_transfer_px(Y[r][1], kc[1], k, lin, out);
            const uint32_t p2 = yuv_transfer_px(Y[r][2], kc[2], k, lin, out), p3 = yuv_transfer_px(Y[r][3], kc[3], k, lin, out);
            uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
            d4[0] = p0 | (p1 << 24);                 // b0 g0 r0 b1
            d4[1] = (p1 >> 8) | (p2 << 16);          // g1 r1 b2 g2
            d4[2] = (p2 >> 16) | (p3 << 8);          // r2 b3 g3 r3
            continue;
        }
        if (r == 0) YUV_TRANSFER_HIT(out_bytes);
        for (int i = 0; i < 4; ++i)
            if (i < np) {
                const uint32_t px = yuv_transfer_px(Y[r][i], kc[i], k, lin, out);
                d[3 * i] = (uint8_t)px; d[3 * i + 1] = (uint8_t)(px >> 8); d[3 * i + 2] = (uint8_t)(px >> 16);
            }
    }
}

// thread rows a block converts one after the other, so that one fill of the tables serves YUV_TRK_ROWS * 256 threads (at one thread
// row each the fill, 6 KB a block, was as many bytes as the 4 - 6 KB of samples a 4:2:2 / 4:4:4 block reads)
constexpr int YUV_TRK_ROWS = 4;

#if defined(__HIPCC__)
// grid (ceil(ceil(w/4) / YUV_TX), ceil(rows / (YUV_TY * YUV_TRK_ROWS)), n) with rows = h / 2 (420) or h (422, 444), block (YUV_TX,
// YUV_TY).  tab: LIN uint16 [1024] then OUT uint8 [4096], 16-byte aligned (the matcher's d_transfer): 384 16-byte loads a block
template <int SAMPLING, int DEPTH>
__global__ __launch_bounds__(YUV_TX * YUV_TY) void yuv_transfer_to_bgr_kernel(YuvArgs a, YuvTransferCoef k, const uint4* __restrict__ tab) {
    __shared__ uint4 lds[YUV_TRK_DWORDS / 4];
    for (int i = threadIdx.y * YUV_TX + threadIdx.x; i < YUV_TRK_DWORDS / 4; i += YUV_TX * YUV_TY) lds[i] = tab[i];
    __syncthreads();                                 // (before any thread returns: yuv_transfer_thread's first line may)
    const uint16_t* lin = reinterpret_cast<const uint16_t*>(lds);
    const uint8_t* out = reinterpret_cast<const uint8_t*>(lds) + YUV_TRK_LIN_BYTES;
    for (int it = 0; it < YUV_TRK_ROWS; ++it)
        yuv_transfer_thread<SAMPLING, DEPTH>(a, k, lin, out, blockIdx.x * YUV_TX + threadIdx.x, (blockIdx.y * YUV_TRK_ROWS + it) * YUV_TY + threadIdx.y,
                                             blockIdx.z);
}
#endif

}  // namespace slideo
