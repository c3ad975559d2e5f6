// yuv_sampling.hip.h — decoded YUV 4:2:2 (planar, semi-planar, packed) and 4:4:4 frames -> the BGR8 image the frame pipeline reads
// (include/slideo_amd.h "YUV sampling").
//
//   yuv_sampled_to_bgr_kernel<SAMPLING, DEPTH>   one frame batch under the matcher's colour description   (HBM: 2wh / 3wh in per
//                                                 byte of sample, 3wh out)
// Launched iff the sampling is not 4:2:0 (stage_orb.hip launch_yuv420_to_bgr); seven instances: 422 and 444 at three depths, packed
// at 8 bits.  The arithmetic is yuv420.hip.h's description kernel's by inclusion — coefficients as kernel arguments (SGPRs), products
// on the 24-bit multipliers, clamp before shift (yuv_desc_sat8 there says why), the 16-bit narrowing of yuv_s8 / yuv_pack4 / yuv_load4 —
// and so are its bounds: every operand fits 24 signed bits, every product and sum int32.
// Thread shape: four consecutive pixels of ONE row (chroma is not shared between rows, so the 2-row thread of the 4:2:0 kernels
// buys nothing); block YUV_TX x YUV_TY = 64 threads along a row x 4 rows.  12 bytes out as three dwords where the destination is
// dword-aligned and w % 4 == 0, bytes otherwise (the decomposition of the reduce, rectify and content kernels).  No LDS.
// Loads, each path chosen on its own by the host from the addresses (yuv_sampled_args): wide where aligned, else sample by sample
// with byte loads — so are the ragged last 1..3 pixels of a 4:4:4 row and the last 2 of a 4:2:2 row.  No multi-dword load is ever
// issued at an address that is not a multiple of its size.
//   luma                     4 samples: one dword (8-bit) or one 8-byte load (16-bit)
//   422 planar chroma        2 samples per plane: one 2-byte load (8-bit) or one dword (16-bit)
//   422 interleaved chroma   2 pairs: one dword (8-bit) or one 8-byte load (16-bit)
//   444 planar chroma        as luma, per plane
//   444 interleaved chroma   4 pairs: 8 bytes (8-bit) as one 8-byte load where 8-aligned, two dwords where 4-aligned; 16 bytes
//                            (16-bit) as two 8-byte loads where 8-aligned, four dwords where 4-aligned
//   packed                   the thread's two macropixels: one 8-byte load where the rows are 8-aligned, two dwords where
//                            4-aligned; luma and chroma bytes out of the macropixels by v_perm_b32, the selectors from the host
// The per-thread body is a host + device function: tools/yuv_sampling_hostcheck.cpp runs it lane by lane on the CPU.
#pragma once
#include "slideo_amd.h"
#include "yuv420.hip.h"

namespace slideo {

// The kernel's arguments for n frames in a layout yuv420_validate accepted under (sampling, depth): yuv_args' record with this
// family's wide_y and wide_c, by the table above
inline YuvArgs yuv_sampled_args(int sampling, int depth, const uint8_t* src, int64_t src_fs, const slideo_yuv420_layout& L, int w, int h, int n,
                                uint8_t* dst) {
    int ay, ac;
    YuvArgs a = yuv_args(sampling, src, src_fs, L, w, h, n, dst, &ay, &ac);
    const int B = depth == SLIDEO_YUV_DEPTH_8 ? 1 : 2;
    // wide_y: planar luma, 1 = a thread's 4 samples are one aligned load; packed, 8 / 4 = its 8 bytes are one / two.  wide_c: nonzero
    // = the wide load applies; 444 interleaved: 8 / 4, the load's size
    if (sampling == SLIDEO_YUV_SAMPLING_422_PACKED) { a.wide_y = yuv_load_mode(ay); return a; }
    a.wide_y = ay >= 4 * B;
    if (sampling == SLIDEO_YUV_SAMPLING_444) a.wide_c = a.interleaved ? yuv_load_mode(ac) : ac >= 4 * B;
    else a.wide_c = ac >= (a.interleaved ? 4 * B : 2 * B);
    return a;
}

// p + ofs with the offset opaque to the compiler: the load at it is not merged with its neighbour's into one wider load, which would
// sit at an address that is not a multiple of its size (the vectoriser merges adjacent loads whatever their alignment)
YUV_HD const uint8_t* yuv_apart(const uint8_t* p, int ofs) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(ofs));
#endif
    return p + ofs;
}
YUV_HD uint64_t yuv_ld64(const uint8_t* p) { return *reinterpret_cast<const uint64_t*>(p); }
YUV_HD uint32_t yuv_ld16(const uint8_t* p) { return *reinterpret_cast<const uint16_t*>(p); }

// One thread of the launch grid: columns 4 tix .. 4 tix + 3 of row `row` of frame z.
template <int SAMPLING, int DEPTH>
YUV_HD void yuv_sampled_thread(const YuvArgs& a, const YuvCoef& k, int tix, int row, int z) {
    constexpr int B = DEPTH == YUV_D8 ? 1 : 2;
    constexpr bool S444 = SAMPLING == YUV_S444;
    const int x0 = tix * 4;
    if (x0 >= a.w || row >= a.h) return;
    const uint8_t* f = a.src + (int64_t)z * a.src_frame_stride;
    const bool full = x0 + 3 < a.w;
    const int np = full ? 4 : a.w - x0;              // columns of this thread
    // 8-bit values, one per byte: luma of the four columns; chroma per column (444) or per column pair (422: bytes 0 and 1)
    uint32_t y4 = 0, u4 = 0, v4 = 0;
    if (SAMPLING == YUV_S422P) {
        const uint8_t* p = f + (int64_t)row * a.y_stride + (int64_t)x0 * 2;
        if (full && a.wide_y) {
            uint32_t lo, hi;
            if (a.wide_y == 8) { const uint64_t q = yuv_ld64(p); lo = (uint32_t)q; hi = (uint32_t)(q >> 32); }
            else { lo = yuv_ld32(p); hi = yuv_ld32(yuv_apart(p, 4)); }
            y4 = yuv_perm(hi, lo, a.sel_y);
            const uint32_t c4 = yuv_perm(hi, lo, a.sel_c);          // U0 U1 V0 V1
            u4 = c4 & 0xffffu; v4 = c4 >> 16;
        } else {
            const int ly = a.sel_y & 7, uo = a.sel_c & 7, vo = (a.sel_c >> 16) & 7;
            for (int i = 0; i < 4; ++i) if (i < np) y4 |= (uint32_t)p[2 * i + ly] << (8 * i);
            for (int j = 0; j < 2; ++j)
                if (2 * j < np) { u4 |= (uint32_t)p[4 * j + uo] << (8 * j); v4 |= (uint32_t)p[4 * j + vo] << (8 * j); }
        }
    } else {
        const uint8_t* py = f + (int64_t)row * a.y_stride + (int64_t)x0 * B;
        if (full && a.wide_y) y4 = yuv_load4<DEPTH>(py);
        else
            for (int i = 0; i < 4; ++i) if (i < np) y4 |= yuv_s8<DEPTH>(py + i * B) << (8 * i);
        const int xc = S444 ? x0 : x0 >> 1;
        const int nc = S444 ? np : (np + 1) >> 1;    // chroma samples of this thread, per plane
        const int64_t crow = (int64_t)row * a.uv_stride;
        if (a.interleaved) {
            const uint8_t* p = f + a.c_ofs + crow + (int64_t)xc * 2 * B;
            uint32_t f4 = 0, s4 = 0;                 // the first and the second sample of every pair
            if (full && a.wide_c) {
                if (S444) {
                    uint32_t lo, hi;                 // first0 second0 first1 second1, first2 second2 first3 second3
                    if (DEPTH == YUV_D8) {
                        if (a.wide_c == 8) { const uint64_t q = yuv_ld64(p); lo = (uint32_t)q; hi = (uint32_t)(q >> 32); }
                        else { lo = yuv_ld32(p); hi = yuv_ld32(yuv_apart(p, 4)); }
                    } else if (a.wide_c == 8) {
                        const uint64_t q0 = yuv_ld64(p), q1 = yuv_ld64(yuv_apart(p, 8));
                        lo = yuv_pack4<DEPTH>((uint32_t)q0, (uint32_t)(q0 >> 32)); hi = yuv_pack4<DEPTH>((uint32_t)q1, (uint32_t)(q1 >> 32));
                    } else {
                        lo = yuv_pack4<DEPTH>(yuv_ld32(p), yuv_ld32(yuv_apart(p, 4)));
                        hi = yuv_pack4<DEPTH>(yuv_ld32(yuv_apart(p, 8)), yuv_ld32(yuv_apart(p, 12)));
                    }
                    f4 = yuv_perm(hi, lo, 0x06040200u); s4 = yuv_perm(hi, lo, 0x07050301u);
                } else {
                    uint32_t c4;                     // first0 second0 first1 second1
                    if (DEPTH == YUV_D8) c4 = yuv_ld32(p);
                    else { const uint64_t q = yuv_ld64(p); c4 = yuv_pack4<DEPTH>((uint32_t)q, (uint32_t)(q >> 32)); }
                    f4 = yuv_perm(0u, c4, 0x04040200u); s4 = yuv_perm(0u, c4, 0x04040301u);      // (bytes 4..7: the zero operand)
                }
            } else
                for (int j = 0; j < 4; ++j)
                    if (j < nc) { f4 |= yuv_s8<DEPTH>(p + 2 * j * B) << (8 * j); s4 |= yuv_s8<DEPTH>(p + (2 * j + 1) * B) << (8 * j); }
            u4 = a.v_first ? s4 : f4; v4 = a.v_first ? f4 : s4;
        } else {
            const uint8_t* pu = f + a.c_ofs + crow + (int64_t)xc * B;
            const uint8_t* pv = f + a.v_ofs + crow + (int64_t)xc * B;
            if (full && a.wide_c) {
                if (S444) { u4 = yuv_load4<DEPTH>(pu); v4 = yuv_load4<DEPTH>(pv); }
                else if (DEPTH == YUV_D8) { u4 = yuv_ld16(pu); v4 = yuv_ld16(pv); }
                else { const uint32_t c4 = yuv_pack4<DEPTH>(yuv_ld32(pu), yuv_ld32(pv)); u4 = c4 & 0xffffu; v4 = c4 >> 16; }
            } else
                for (int j = 0; j < 4; ++j)
                    if (j < nc) { u4 |= yuv_s8<DEPTH>(pu + j * B) << (8 * j); v4 |= yuv_s8<DEPTH>(pv + j * B) << (8 * j); }
        }
    }
    uint32_t p0, p1, p2, p3;                         // b | g << 8 | r << 16 of the four columns (columns past the row: unused)
    if (S444) {
        p0 = yuv_desc_px(y4 & 255, yuv_desc_chroma(u4 & 255, v4 & 255, k), k);
        p1 = yuv_desc_px((y4 >> 8) & 255, yuv_desc_chroma((u4 >> 8) & 255, (v4 >> 8) & 255, k), k);
        p2 = yuv_desc_px((y4 >> 16) & 255, yuv_desc_chroma((u4 >> 16) & 255, (v4 >> 16) & 255, k), k);
        p3 = yuv_desc_px(y4 >> 24, yuv_desc_chroma(u4 >> 24, v4 >> 24, k), k);
    } else {
        const YuvDC k0 = yuv_desc_chroma(u4 & 255, v4 & 255, k), k1 = yuv_desc_chroma((u4 >> 8) & 255, (v4 >> 8) & 255, k);
        p0 = yuv_desc_px(y4 & 255, k0, k); p1 = yuv_desc_px((y4 >> 8) & 255, k0, k);
        p2 = yuv_desc_px((y4 >> 16) & 255, k1, k); p3 = yuv_desc_px(y4 >> 24, k1, k);
    }
    uint8_t* d = a.dst + (int64_t)z * a.w * a.h * 3 + ((int64_t)row * a.w + x0) * 3;
    if (a.out4) {                                    // (w % 4 == 0: every thread owns four columns)
        uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
        d4[0] = p0 | (p1 << 24);                     // b0 g0 r0 b1
        d4[1] = (p1 >> 8) | (p2 << 16);              // g1 r1 b2 g2
        d4[2] = (p2 >> 16) | (p3 << 8);              // r2 b3 g3 r3
        return;
    }
    const uint32_t px[4] = {p0, p1, p2, p3};
    for (int i = 0; i < 4; ++i)
        if (i < np) { d[3 * i] = (uint8_t)px[i]; d[3 * i + 1] = (uint8_t)(px[i] >> 8); d[3 * i + 2] = (uint8_t)(px[i] >> 16); }
}

#if defined(__HIPCC__)
// grid (ceil(ceil(w/4) / YUV_TX), ceil(h / YUV_TY), n), block (YUV_TX, YUV_TY)
template <int SAMPLING, int DEPTH>
__global__ __launch_bounds__(YUV_TX * YUV_TY) void yuv_sampled_to_bgr_kernel(YuvArgs a, YuvCoef k) {
    yuv_sampled_thread<SAMPLING, DEPTH>(a, k, blockIdx.x * YUV_TX + threadIdx.x, blockIdx.y * YUV_TY + threadIdx.y, blockIdx.z);
}
#endif

}  // namespace slideo
