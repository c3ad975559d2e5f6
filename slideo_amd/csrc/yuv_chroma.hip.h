// yuv_chroma.hip.h — decoded YUV 4:2:0 and 4:2:2 frames -> the BGR8 image the frame pipeline reads, with BILINEAR, SITED chroma
// (include/slideo_amd.h "YUV chroma filter").
//
//   yuv_chroma_to_bgr_kernel<SAMPLING, DEPTH>   one frame batch under the matcher's colour description and chroma filter
//                                                (HBM: the bytes of the nearest kernels: 1.5wh / 2wh in per byte of sample, 3wh out)
// Launched iff the filter is not NEAREST and the sampling is not 4:4:4 (stage_orb.hip launch_yuv420_to_bgr); seven instances: 420 and
// 422 at three depths, packed at 8 bits.  The per-pixel arithmetic is yuv420.hip.h's description kernel's by inclusion (yuv_desc_px,
// yuv_s8, yuv_pack4, yuv_load4: coefficients in SGPRs, 24-bit multiplies, clamp before shift; the chroma terms are yuv_desc_chroma's
// integers, computed per pixel with the - 128 folded into a constant: yuv_chroma_terms), the load helpers are yuv_sampling.hip.h's
// (yuv_apart, yuv_ld64, yuv_ld16).  Only U8 and V8 of a pixel are new.
// Thread shape: four consecutive pixels of two luma rows 2cy, 2cy + 1 (420: the rows that share chroma row cy) or of one row (422);
// block YUV_TX x YUV_TY = 64 threads along a row x 4 thread rows, so a wave is 64 consecutive threads of one thread row.
// The stencil.  The tables of slideo_yuv_chroma_weights have two structural zeros per axis — parity 0 never reaches sample k + 1,
// parity 1 never sample k - 1 — so each axis is a 2-tap filter and the kernel takes the EIGHT weights that can be nonzero (wh and wv
// below).  A thread's pixels 4t .. 4t + 3 sit on chroma columns k0 = 2t and k0 + 1 and need samples k0 - 1 .. k0 + 2 of one chroma
// row (422) or of rows cy - 1, cy, cy + 1 (420; all clamped to the plane).
//   - its OWN samples k0, k0 + 1 of both planes are loaded as the nearest kernels load them — one aligned load per plane or pair
//     plane where the host found the addresses aligned (yuv_chroma_args), else sample by sample with byte loads — and kept as one
//     dword U0 U1 V0 V1;
//   - sample k0 - 1 is the left lane's U1 V1 and sample k0 + 2 the right lane's U0 V0: one exchange of that dword with both
//     neighbours per chroma row (yuv_chroma_exchange: two ds_bpermute_b32, no LDS allocated), the one hook a host build satisfies
//     by computing the neighbour's dword directly;
//   - only the first and the last lane of a wave load a halo sample (byte loads, one branch for both), and at the image's edge the
//     clamp is the lane's own sample: no load;
//   - 420: the row above is loaded only where its weight is nonzero (co-sited vertical siting never reaches it);
//   - every load is issued before the first loaded value is used (luma, own chroma of every row, halo), so that a wave waits for
//     memory once: yuv_chroma_own_load returns what came as it came, yuv_chroma_own makes the dword of it afterwards.
// U and V are filtered TOGETHER, as the two 16-bit halves of one dword (U | V << 16), on the packed 16-bit multiply-adds: vertical
// first (values <= 4 * 255), then horizontal (<= 16 * 255 + 8 < 2^16: no carry between the halves), + 8 >> 4 (420) or + 2 >> 2 (422).
// Integer sums are exact, so the order of the two axes is free; this order needs 16 + 16 multiply-adds per thread instead of 24 + 16.
// No multi-dword load is issued at an address that is not a multiple of its size; no LDS, no scratch.
// The per-thread body is a host + device function: tools/yuv_chroma_hostcheck.cpp runs it lane by lane on the CPU.
#pragma once
#include "slideo_amd.h"
#include "yuv_sampling.hip.h"

#ifndef YUV_CHROMA_HIT          // (tools/yuv_chroma_hostcheck.cpp counts the paths a run took)
#define YUV_CHROMA_HIT(path)
#endif

namespace slideo {

// the EIGHT weights that can be nonzero, each in both 16-bit halves
struct YuvChromaW {
    uint32_t wh[4];              // wh[0][0], wh[0][1], wh[1][1], wh[1][2] of slideo_yuv_chroma_weights
    uint32_t wv[4];              // wv likewise (422: unused)
};

// The kernel's arguments for n frames in a layout yuv420_validate accepted under (sampling, depth), with the twelve integers of
// slideo_yuv_chroma_weights: yuv_args' record with this family's wide_y and wide_c, and the weights.
// false: the table is not one this kernel computes (a structural zero is not zero)
inline bool yuv_chroma_args(int sampling, int depth, const int32_t* w12, const uint8_t* src, int64_t src_fs, const slideo_yuv420_layout& L, int w, int h,
                            int n, uint8_t* dst, YuvArgs* out, YuvChromaW* wt) {
    for (int ax = 0; ax < 2; ++ax) {
        const int32_t* t = w12 + 6 * ax;
        if (t[2] != 0 || t[3] != 0) return false;
        const int32_t four[4] = {t[0], t[1], t[4], t[5]};
        for (int i = 0; i < 4; ++i) {
            if (four[i] < 0 || four[i] > 4) return false;
            (ax ? wt->wv : wt->wh)[i] = (uint32_t)four[i] * 0x00010001u;
        }
    }
    int ay, ac;
    YuvArgs a = yuv_args(sampling, src, src_fs, L, w, h, n, dst, &ay, &ac);
    const int B = depth == SLIDEO_YUV_DEPTH_8 ? 1 : 2;
    // wide_y: planar luma, 1 = a thread's 4 samples of a row are one aligned load; packed, 8 / 4 = its 8 bytes are one / two.
    // wide_c, a thread's own chroma: interleaved 4 B bytes (8-bit: one dword; 16-bit: 8 / 4, one 8-byte load or two dwords), planar
    // 2 B per plane
    if (sampling == SLIDEO_YUV_SAMPLING_422_PACKED) a.wide_y = yuv_load_mode(ay);
    else {
        a.wide_y = ay >= 4 * B;
        if (a.interleaved) a.wide_c = B == 1 ? ac >= 4 : yuv_load_mode(ac);
        else a.wide_c = ac >= 2 * B;
    }
    *out = a;
    return true;
}

// acc + w * p in both 16-bit halves (v_pk_mad_u16); every value here stays below 2^16, so the plain product is the same number
YUV_HD uint32_t yuv_mad2(uint32_t w2, uint32_t p, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, w2) * __builtin_bit_cast(u16x2, p) + __builtin_bit_cast(u16x2, acc)));
#else
    return (w2 & 0xffffu) * p + acc;
#endif
}

// chroma sample k of chroma row crow as U | V << 16, 8-bit values: byte loads, any alignment (halo samples and unaligned layouts).
// _pair: packed macropixels and interleaved planes; _planar: two planes; yuv_chroma_at picks one (a.interleaved is uniform)
template <int SAMPLING, int DEPTH>
YUV_HD uint32_t yuv_chroma_at_pair(const YuvArgs& a, const uint8_t* f, int crow, int k) {
    constexpr int B = DEPTH == YUV_D8 ? 1 : 2;
    if (SAMPLING == YUV_S422P) {
        const uint8_t* p = f + (int64_t)crow * a.y_stride + (int64_t)k * 4;
        return (uint32_t)p[a.sel_c & 7] | (uint32_t)p[(a.sel_c >> 16) & 7] << 16;
    }
    const uint8_t* p = f + a.c_ofs + (int64_t)crow * a.uv_stride + (int64_t)k * 2 * B;
    const uint32_t first = yuv_s8<DEPTH>(p), second = yuv_s8<DEPTH>(p + B);
    return a.v_first ? second | first << 16 : first | second << 16;
}
template <int SAMPLING, int DEPTH>
YUV_HD uint32_t yuv_chroma_at_planar(const YuvArgs& a, const uint8_t* f, int crow, int k) {
    constexpr int B = DEPTH == YUV_D8 ? 1 : 2;
    const int64_t o = (int64_t)crow * a.uv_stride + (int64_t)k * B;
    return yuv_s8<DEPTH>(f + a.c_ofs + o) | yuv_s8<DEPTH>(f + a.v_ofs + o) << 16;
}
template <int SAMPLING, int DEPTH>
YUV_HD uint32_t yuv_chroma_at(const YuvArgs& a, const uint8_t* f, int crow, int k) {
    return SAMPLING == YUV_S422P || a.interleaved ? yuv_chroma_at_pair<SAMPLING, DEPTH>(a, f, crow, k) : yuv_chroma_at_planar<SAMPLING, DEPTH>(a, f, crow, k);
}

// Thread tix's OWN chroma of chroma row crow (samples 2 tix and 2 tix + 1), in two steps so that nothing between them uses a loaded
// value: yuv_chroma_own_load issues the loads and returns what came as it came, yuv_chroma_own turns it into the dword U0 U1 V0 V1
// (a ragged thread, which owns two columns, repeats its one sample: that is the clamp).  Packed: the same bytes hold the row's luma,
// returned through y4 when asked for.  `mine`: the calling thread's own load (a host build's neighbour look-up is not counted)
struct YuvChromaRaw { uint32_t lo, hi; };        // the wide load's dwords (planar: U's, V's); the byte path: lo is the finished dword
template <int SAMPLING, int DEPTH>
YUV_HD YuvChromaRaw yuv_chroma_own_load(const YuvArgs& a, const uint8_t* f, int tix, int crow, uint32_t* y4, bool mine) {
    constexpr int B = DEPTH == YUV_D8 ? 1 : 2;
    const int x0 = tix * 4, k0 = x0 >> 1;
    const bool full = x0 + 3 < a.w;
    (void)mine;
    if (SAMPLING == YUV_S422P) {
        const uint8_t* p = f + (int64_t)crow * a.y_stride + (int64_t)x0 * 2;
        if (full && a.wide_y) {
            if (a.wide_y == 8) { const uint64_t q = yuv_ld64(p); if (mine) YUV_CHROMA_HIT(packed8); return YuvChromaRaw{(uint32_t)q, (uint32_t)(q >> 32)}; }
            if (mine) YUV_CHROMA_HIT(packed4);
            return YuvChromaRaw{yuv_ld32(p), yuv_ld32(yuv_apart(p, 4))};
        }
        if (y4) {
            const int ly = a.sel_y & 7, np = full ? 4 : a.w - x0;
            uint32_t y = 0;
            for (int i = 0; i < 4; ++i) if (i < np) y |= (uint32_t)p[2 * i + ly] << (8 * i);
            *y4 = y;
        }
    } else if (full && a.wide_c) {
        const int64_t ro = (int64_t)crow * a.uv_stride;
        if (a.interleaved) {                         // first0 second0 first1 second1
            const uint8_t* p = f + a.c_ofs + ro + (int64_t)x0 * B;
            if (DEPTH == YUV_D8) { if (mine) YUV_CHROMA_HIT(wide_c4); return YuvChromaRaw{yuv_ld32(p), 0u}; }
            if (a.wide_c == 8) { const uint64_t q = yuv_ld64(p); if (mine) YUV_CHROMA_HIT(wide_c8); return YuvChromaRaw{(uint32_t)q, (uint32_t)(q >> 32)}; }
            if (mine) YUV_CHROMA_HIT(wide_c4);
            return YuvChromaRaw{yuv_ld32(p), yuv_ld32(yuv_apart(p, 4))};
        }
        const uint8_t* pu = f + a.c_ofs + ro + (int64_t)k0 * B;
        const uint8_t* pv = f + a.v_ofs + ro + (int64_t)k0 * B;
        if (DEPTH == YUV_D8) { if (mine) YUV_CHROMA_HIT(wide_c2); return YuvChromaRaw{yuv_ld16(pu), yuv_ld16(pv)}; }
        if (mine) YUV_CHROMA_HIT(wide_c4);
        return YuvChromaRaw{yuv_ld32(pu), yuv_ld32(pv)};
    }
    if (mine) YUV_CHROMA_HIT(bytes_c);
    const uint32_t p0 = yuv_chroma_at<SAMPLING, DEPTH>(a, f, crow, k0);
    const uint32_t p1 = full ? yuv_chroma_at<SAMPLING, DEPTH>(a, f, crow, k0 + 1) : p0;
    return YuvChromaRaw{p0 | p1 << 8, 0u};
}
template <int SAMPLING, int DEPTH>
YUV_HD uint32_t yuv_chroma_own(const YuvArgs& a, int tix, const YuvChromaRaw& raw, uint32_t* y4) {
    const bool full = tix * 4 + 3 < a.w;
    if (SAMPLING == YUV_S422P) {
        if (!(full && a.wide_y)) return raw.lo;
        if (y4) *y4 = yuv_perm(raw.hi, raw.lo, a.sel_y);
        return yuv_perm(raw.hi, raw.lo, a.sel_c);
    }
    if (!(full && a.wide_c)) return raw.lo;
    if (a.interleaved) return yuv_perm(0u, DEPTH == YUV_D8 ? raw.lo : yuv_pack4<DEPTH>(raw.lo, raw.hi), a.sel_c);
    return DEPTH == YUV_D8 ? raw.lo | raw.hi << 16 : yuv_pack4<DEPTH>(raw.lo, raw.hi);
}

// THE cross-lane hook: the own dwords of the lanes to the left and to the right of `lane` (lane = tix % YUV_TX: the wave is one
// thread row of the block).  Device: two ds_bpermute_b32; a lane past the row's end has left, and its slot reads as nothing anybody
// uses.  Host: the neighbour's dword, computed directly.  Lane 0's prev and lane 63's next are never used (yuv_chroma_thread).
template <int SAMPLING, int DEPTH>
YUV_HD void yuv_chroma_exchange(const YuvArgs& a, const uint8_t* f, int tix, int lane, int crow, uint32_t own, uint32_t* prev, uint32_t* next) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)a; (void)f; (void)tix; (void)crow;
    *prev = (uint32_t)__builtin_amdgcn_ds_bpermute((lane - 1) << 2, (int)own);
    *next = (uint32_t)__builtin_amdgcn_ds_bpermute((lane + 1) << 2, (int)own);
#else
    (void)own;
    *prev = lane > 0 ? yuv_chroma_own<SAMPLING, DEPTH>(a, tix - 1, yuv_chroma_own_load<SAMPLING, DEPTH>(a, f, tix - 1, crow, nullptr, false), nullptr) : 0u;
    *next = lane < YUV_TX - 1 && (tix + 1) * 4 < a.w
                ? yuv_chroma_own<SAMPLING, DEPTH>(a, tix + 1, yuv_chroma_own_load<SAMPLING, DEPTH>(a, f, tix + 1, crow, nullptr, false), nullptr) : 0u;
#endif
}

// chroma terms of one pixel from its filtered U8, V8: yuv_desc_chroma's integers with the - 128 folded into the constant
// (half + c (X - 128) = c X + (half - 128 c): every product and sum stays int32 as there), so a pixel costs four multiply-adds
struct YuvChromaK { int r0, g0, b0; };
YUV_HD YuvChromaK yuv_chroma_k(const YuvCoef& k) { return YuvChromaK{YUV_HALF - 128 * k.cvr, YUV_HALF - 128 * (k.cvg + k.cug), YUV_HALF - 128 * k.cub}; }
YUV_HD YuvDC yuv_chroma_terms(uint32_t uv, const YuvCoef& k, const YuvChromaK& c) {      // uv = U8 | V8 << 16
    const int U = (int)(uv & 0xffffu), V = (int)(uv >> 16);
    return YuvDC{yuv_mul24(k.cvr, V) + c.r0, yuv_mul24(k.cvg, V) + yuv_mul24(k.cug, U) + c.g0, yuv_mul24(k.cub, U) + c.b0};
}

// One thread of the launch grid: columns 4 tix .. 4 tix + 3 of luma rows 2 row and 2 row + 1 (420) or of luma row `row` (422) of
// frame z; lane = tix % YUV_TX.  Order: every load is issued before the first value is used — luma, the own chroma of every chroma
// row, then the halo samples of the first and the last lane — so that a wave waits for memory once; then the exchange, the filter
// and the conversion.
template <int SAMPLING, int DEPTH>
YUV_HD void yuv_chroma_thread(const YuvArgs& a, const YuvChromaW& wt, const YuvCoef& k, int tix, int lane, int row, int z) {
    constexpr int B = DEPTH == YUV_D8 ? 1 : 2;
    constexpr bool S420 = SAMPLING == YUV_S420, PACKED = SAMPLING == YUV_S422P;
    constexpr int NR = S420 ? 2 : 1;                 // luma rows of this thread
    constexpr int NC = S420 ? 3 : 1;                 // chroma rows it reads: the thread's own, then (420) the one above and the one below
    const int x0 = tix * 4, r0 = S420 ? 2 * row : row;
    if (x0 >= a.w || r0 >= a.h) return;
    const uint8_t* f = a.src + (int64_t)z * a.src_frame_stride;
    const bool full = x0 + 3 < a.w;
    const int np = full ? 4 : a.w - x0;              // columns of this thread
    const int k0 = tix * 2, cw = a.w >> 1, chh = a.h >> 1;
    uint32_t y4[NR] = {};
    if (!PACKED) {
        const uint8_t* py = f + (int64_t)r0 * a.y_stride + (int64_t)x0 * B;
        if (full && a.wide_y) {
            YUV_CHROMA_HIT(wide_y);
            for (int r = 0; r < NR; ++r) y4[r] = yuv_load4<DEPTH>(py + (int64_t)r * a.y_stride);
        } else {
            YUV_CHROMA_HIT(bytes_y);
            for (int r = 0; r < NR; ++r)
                for (int i = 0; i < 4; ++i) if (i < np) y4[r] |= yuv_s8<DEPTH>(py + (int64_t)r * a.y_stride + i * B) << (8 * i);
        }
    }
    // (uniform: kernel arguments) the row above is read only where its weight is nonzero — co-sited vertical siting never reaches it
    const int crow[3] = {row, row > 0 ? row - 1 : 0, row + 1 < chh ? row + 1 : chh - 1};
    const bool use[3] = {true, S420 && wt.wv[0] != 0, S420 && wt.wv[3] != 0};
    YuvChromaRaw raw[NC] = {};
    uint32_t halo[NC] = {};
    for (int i = 0; i < NC; ++i)
        if (use[i]) raw[i] = yuv_chroma_own_load<SAMPLING, DEPTH>(a, f, tix, crow[i], PACKED ? &y4[0] : nullptr, true);
    // halo samples: k0 - 1 for the first lane of a wave, k0 + 2 for the last, where the row does not end there (there the clamp is
    // the lane's own sample).  One branch for both lanes and no branch between the rows (a row whose weight is zero is read all the
    // same: two lanes of a wave do), so that all their loads are in flight together
    const bool first = lane == 0 && k0 > 0, last = lane == YUV_TX - 1 && k0 + 2 < cw;
    if (first || last) {
        const int kh = first ? k0 - 1 : k0 + 2;
        YUV_CHROMA_HIT(halo);
        if (PACKED || a.interleaved) { for (int i = 0; i < NC; ++i) halo[i] = yuv_chroma_at_pair<SAMPLING, DEPTH>(a, f, crow[i], kh); }
        else { for (int i = 0; i < NC; ++i) halo[i] = yuv_chroma_at_planar<SAMPLING, DEPTH>(a, f, crow[i], kh); }
    }
    uint32_t T[NR][4] = {};                          // per luma row: the vertical sums of chroma columns k0 - 1 .. k0 + 2 (U | V << 16)
    for (int i = 0; i < NC; ++i) {
        if (!use[i]) continue;
        uint32_t prev, next, P[4];
        const uint32_t own = yuv_chroma_own<SAMPLING, DEPTH>(a, tix, raw[i], PACKED ? &y4[0] : nullptr);
        yuv_chroma_exchange<SAMPLING, DEPTH>(a, f, tix, lane, crow[i], own, &prev, &next);
        P[1] = own & 0x00ff00ffu;
        P[2] = (own >> 8) & 0x00ff00ffu;
        if (k0 == 0) { P[0] = P[1]; YUV_CHROMA_HIT(clamp); }
        else if (lane == 0) P[0] = halo[i];
        else { P[0] = (prev >> 8) & 0x00ff00ffu; YUV_CHROMA_HIT(neighbour); }
        if (k0 + 2 >= cw) { P[3] = P[2]; YUV_CHROMA_HIT(clamp); }
        else if (lane == YUV_TX - 1) P[3] = halo[i];
        else { P[3] = next & 0x00ff00ffu; YUV_CHROMA_HIT(neighbour); }
        if (!S420) { for (int j = 0; j < 4; ++j) T[0][j] = P[j]; }
        else if (i == 0) { for (int j = 0; j < 4; ++j) { T[0][j] = yuv_mad2(wt.wv[1], P[j], T[0][j]); T[NR - 1][j] = yuv_mad2(wt.wv[2], P[j], T[NR - 1][j]); } }
        else if (i == 1) { for (int j = 0; j < 4; ++j) T[0][j] = yuv_mad2(wt.wv[0], P[j], T[0][j]); }
        else { for (int j = 0; j < 4; ++j) T[NR - 1][j] = yuv_mad2(wt.wv[3], P[j], T[NR - 1][j]); }
    }
    const uint32_t rnd = S420 ? 0x00080008u : 0x00020002u;
    constexpr int SH = S420 ? 4 : 2;
    const YuvChromaK ck = yuv_chroma_k(k);
    uint8_t* d0 = a.dst + (int64_t)z * a.w * a.h * 3 + ((int64_t)r0 * a.w + x0) * 3;
    for (int r = 0; r < NR; ++r) {
        const uint32_t* V = T[r];
        // columns 0 and 2 have parity 0 (samples k - 1, k), columns 1 and 3 parity 1 (samples k, k + 1)
        const uint32_t c0 = (yuv_mad2(wt.wh[0], V[0], yuv_mad2(wt.wh[1], V[1], rnd)) >> SH) & 0x00ff00ffu;
        const uint32_t c1 = (yuv_mad2(wt.wh[2], V[1], yuv_mad2(wt.wh[3], V[2], rnd)) >> SH) & 0x00ff00ffu;
        const uint32_t c2 = (yuv_mad2(wt.wh[0], V[1], yuv_mad2(wt.wh[1], V[2], rnd)) >> SH) & 0x00ff00ffu;
        const uint32_t c3 = (yuv_mad2(wt.wh[2], V[2], yuv_mad2(wt.wh[3], V[3], rnd)) >> SH) & 0x00ff00ffu;
        const uint32_t p0 = yuv_desc_px(y4[r] & 255, yuv_chroma_terms(c0, k, ck), k);
        const uint32_t p1 = yuv_desc_px((y4[r] >> 8) & 255, yuv_chroma_terms(c1, k, ck), k);
        const uint32_t p2 = yuv_desc_px((y4[r] >> 16) & 255, yuv_chroma_terms(c2, k, ck), k);
        const uint32_t p3 = yuv_desc_px(y4[r] >> 24, yuv_chroma_terms(c3, k, ck), k);
        uint8_t* d = d0 + (int64_t)r * a.w * 3;
        if (a.out4) {                                // (w % 4 == 0: every thread owns four columns)
            if (r == 0) YUV_CHROMA_HIT(out4);
            uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
            d4[0] = p0 | (p1 << 24);                 // b0 g0 r0 b1
            d4[1] = (p1 >> 8) | (p2 << 16);          // g1 r1 b2 g2
            d4[2] = (p2 >> 16) | (p3 << 8);          // r2 b3 g3 r3
            continue;
        }
        if (r == 0) YUV_CHROMA_HIT(out_bytes);
        const uint32_t px[4] = {p0, p1, p2, p3};
        for (int i = 0; i < 4; ++i)
            if (i < np) { d[3 * i] = (uint8_t)px[i]; d[3 * i + 1] = (uint8_t)(px[i] >> 8); d[3 * i + 2] = (uint8_t)(px[i] >> 16); }
    }
}

#if defined(__HIPCC__)
// grid (ceil(ceil(w/4) / YUV_TX), ceil(rows / YUV_TY), n) with rows = h / 2 (420) or h (422), block (YUV_TX, YUV_TY)
template <int SAMPLING, int DEPTH>
__global__ __launch_bounds__(YUV_TX * YUV_TY) void yuv_chroma_to_bgr_kernel(YuvArgs a, YuvChromaW wt, YuvCoef k) {
    yuv_chroma_thread<SAMPLING, DEPTH>(a, wt, k, blockIdx.x * YUV_TX + threadIdx.x, threadIdx.x, blockIdx.y * YUV_TY + threadIdx.y, blockIdx.z);
}
#endif

}  // namespace slideo
