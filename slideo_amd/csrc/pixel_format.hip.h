// pixel_format.hip.h — RGB8, four-byte (BGRA / RGBA / ARGB / ABGR) and planar (RGB / BGR / GBR) frames -> the BGR8 image the frame
// pipeline reads (include/slideo_amd.h "Frame pixel format").
//
//   pixels_to_bgr_kernel<FORM>   one frame batch under the matcher's pixel format   (HBM: 3wh or 4wh in, 3wh out)
// Launched iff the format is not SLIDEO_PIXEL_BGR8 (stage_orb.hip launch_pixels_to_bgr); three instances: PACKED3 (RGB8), PACKED4
// (the four byte orders), PLANAR (the three plane orders).  No arithmetic: bytes move.  Channel positions, plane offsets and the
// v_perm_b32 selectors are kernel arguments the host derives from the format (pixels_args): the kernel holds no per-format branch.
// Thread shape: yuv_sampled_to_bgr_kernel's — four consecutive pixels of ONE row; block YUV_TX x YUV_TY = 64 threads along a row x 4
// rows.  12 bytes out as three dwords where the destination is dword-aligned and w % 4 == 0, bytes otherwise.  No LDS.
// Loads, each path chosen by the host from the addresses (base, row stride, frame stride of more than one frame; planar: every
// plane's): wide where aligned, else byte by byte — so are the ragged last 1..3 pixels of a row.  No multi-byte load is ever issued
// at an address that is not a multiple of its size (yuv_apart keeps adjacent narrow loads from merging into a wider one).
//   PACKED4   the thread's 16 bytes: one 16-byte load where 16-aligned, two 8-byte loads where 8-aligned, four dwords where
//             4-aligned.  Three v_perm_b32 make the three output dwords, each out of two adjacent input dwords.
//   PACKED3   the thread's 12 bytes: three dwords where the rows are dword-aligned.  Four v_perm_b32: the first and the last output
//             dword draw on two input dwords; the middle one draws on all three, through one intermediate.
//   PLANAR    one dword per plane where the plane rows are dword-aligned.  Two v_perm_b32 per output dword (fixed selectors: the
//             plane order is in the plane offsets).
// The per-thread body is a host + device function: tools/pixel_format_hostcheck.cpp runs it lane by lane on the CPU.
#pragma once
#include <algorithm>

#include "frame_settings.h"
#include "slideo_amd.h"
#include "yuv_sampling.hip.h"

namespace slideo {

constexpr int PIX_PACKED3 = 0, PIX_PACKED4 = 1, PIX_PLANAR = 2;

struct PixArgs {
    const uint8_t* src;
    int64_t src_frame_stride;    // bytes
    int64_t ofs_b, ofs_g, ofs_r; // the byte of a pixel's B, G, R past the pixel's first byte: 0..3 (packed), plane * h * stride (planar)
    int stride;                  // source rows (planar: every plane's)
    int px_step;                 // bytes from a pixel to the next of its row: 3, 4, or 1 (planar)
    uint8_t* dst;                // BGR8, row stride 3w, frame stride 3wh
    int w, h;
    int wide;                    // PACKED4: 16 / 8 / 4 = the thread's 16 bytes are one / two / four loads; PACKED3, PLANAR: 4 = dwords; 0: bytes
    int out4;                    // dword stores: dst dword-aligned and w % 4 == 0
    uint32_t sel[4];             // packed: the v_perm selectors (PACKED4: three; PACKED3: four, sel[1] the middle dword's intermediate)
};

inline int pixel_format_form(int format) {
    return format >= SLIDEO_PIXEL_PLANAR_RGB8 ? PIX_PLANAR : format >= SLIDEO_PIXEL_BGRA8 ? PIX_PACKED4 : PIX_PACKED3;
}

// The kernel's arguments for n frames of a layout pixel_format_validate accepted: where the channels lie, the selectors, and which
// wide loads and stores the addresses allow.  A single frame has no stride to be aligned.
inline PixArgs pixels_args(int format, const uint8_t* src, int64_t src_fs, int stride, int w, int h, int n, uint8_t* dst) {
    PixArgs a{};
    a.src = src; a.src_frame_stride = src_fs; a.stride = stride;
    a.dst = dst; a.w = w; a.h = h;
    a.out4 = (uintptr_t)dst % 4 == 0 && w % 4 == 0;
    const int64_t fs = n > 1 ? src_fs : 0;
    int cb, cg, cr;
    pixel_format_channels(format, &cb, &cg, &cr);
    const int form = pixel_format_form(format);
    if (form == PIX_PLANAR) {
        const int64_t plane = (int64_t)h * stride;
        a.ofs_b = cb * plane; a.ofs_g = cg * plane; a.ofs_r = cr * plane;
        a.px_step = 1;
        int al = 8;
        for (int p = 0; p < 3; ++p) al = std::min(al, yuv_plane_align(src, p * plane, fs, stride));
        a.wide = al >= 4 ? 4 : 0;
        return a;
    }
    a.ofs_b = cb; a.ofs_g = cg; a.ofs_r = cr;
    const uint64_t v = (uint64_t)(uintptr_t)src | (uint64_t)fs | (uint64_t)(int64_t)stride;
    const uint32_t b = (uint32_t)cb, g = (uint32_t)cg, r = (uint32_t)cr;
    if (form == PIX_PACKED4) {
        a.px_step = 4;
        a.wide = v % 16 == 0 ? 16 : v % 8 == 0 ? 8 : v % 4 == 0 ? 4 : 0;
        // out of (d[i + 1], d[i]): a selector byte 0..3 is a byte of pixel i, 4..7 of pixel i + 1
        a.sel[0] = b | g << 8 | r << 16 | (4 + b) << 24;              // b0 g0 r0 b1
        a.sel[1] = g | r << 8 | (4 + b) << 16 | (4 + g) << 24;        // g1 r1 b2 g2
        a.sel[2] = r | (4 + b) << 8 | (4 + g) << 16 | (4 + r) << 24;  // r2 b3 g3 r3
        return a;
    }
    a.px_step = 3;
    a.wide = v % 4 == 0 ? 4 : 0;
    // the thread's 12 source bytes s[0..12) in d0, d1, d2; output byte 3i + c is s[3i + pos(c)]
    const uint32_t o[12] = {b, g, r, 3 + b, 3 + g, 3 + r, 6 + b, 6 + g, 6 + r, 9 + b, 9 + g, 9 + r};
    a.sel[0] = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;            // out of (d1, d0): s[0..8)
    // the middle dword: its bytes below s[8] gathered out of (d1, d0) first, then joined with d2's: (d2, intermediate)
    uint32_t mid = 0, fin = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = o[4 + i];
        mid |= (s < 8 ? s : 0u) << (8 * i);
        fin |= (s < 8 ? (uint32_t)i : 4 + (s - 8)) << (8 * i);
    }
    a.sel[1] = mid; a.sel[2] = fin;
    a.sel[3] = (o[8] - 4) | (o[9] - 4) << 8 | (o[10] - 4) << 16 | (o[11] - 4) << 24;     // out of (d2, d1): s[4..12)
    return a;
}

// the 16-byte load of PACKED4 (the host build's sanitizer checks its alignment as it checks the narrower ones')
struct alignas(16) PixQuad { uint32_t x, y, z, w; };

// One thread of the launch grid: columns 4 tix .. 4 tix + 3 of row `row` of frame z.
template <int FORM>
YUV_HD void pixels_thread(const PixArgs& a, int tix, int row, int z) {
    const int x0 = tix * 4;
    if (x0 >= a.w || row >= a.h) return;
    const uint8_t* p = a.src + (int64_t)z * a.src_frame_stride + (int64_t)row * a.stride + (int64_t)x0 * a.px_step;
    const bool full = x0 + 3 < a.w;
    const int np = full ? 4 : a.w - x0;              // columns of this thread
    uint32_t o0, o1, o2;                             // the 12 output bytes: b0 g0 r0 b1, g1 r1 b2 g2, r2 b3 g3 r3
    if (full && a.wide) {
        if (FORM == PIX_PACKED4) {
            uint32_t d0, d1, d2, d3;
            if (a.wide == 16) { const PixQuad q = *reinterpret_cast<const PixQuad*>(p); d0 = q.x; d1 = q.y; d2 = q.z; d3 = q.w; }
            else if (a.wide == 8) {
                const uint64_t q0 = yuv_ld64(p), q1 = yuv_ld64(yuv_apart(p, 8));
                d0 = (uint32_t)q0; d1 = (uint32_t)(q0 >> 32); d2 = (uint32_t)q1; d3 = (uint32_t)(q1 >> 32);
            } else { d0 = yuv_ld32(p); d1 = yuv_ld32(yuv_apart(p, 4)); d2 = yuv_ld32(yuv_apart(p, 8)); d3 = yuv_ld32(yuv_apart(p, 12)); }
            o0 = yuv_perm(d1, d0, a.sel[0]); o1 = yuv_perm(d2, d1, a.sel[1]); o2 = yuv_perm(d3, d2, a.sel[2]);
        } else if (FORM == PIX_PACKED3) {
            const uint32_t d0 = yuv_ld32(p), d1 = yuv_ld32(yuv_apart(p, 4)), d2 = yuv_ld32(yuv_apart(p, 8));
            o0 = yuv_perm(d1, d0, a.sel[0]);
            o1 = yuv_perm(d2, yuv_perm(d1, d0, a.sel[1]), a.sel[2]);
            o2 = yuv_perm(d2, d1, a.sel[3]);
        } else {
            const uint32_t b = yuv_ld32(p + a.ofs_b), g = yuv_ld32(p + a.ofs_g), r = yuv_ld32(p + a.ofs_r);
            o0 = yuv_perm(r, yuv_perm(g, b, 0x01000400u), 0x03040100u);      // b0 g0 . b1 | b0 g0 r0 b1
            o1 = yuv_perm(r, yuv_perm(g, b, 0x06020005u), 0x03020500u);      // g1 . b2 g2 | g1 r1 b2 g2
            o2 = yuv_perm(r, yuv_perm(g, b, 0x00070300u), 0x07020106u);      // . b3 g3 .  | r2 b3 g3 r3
        }
    } else {
        uint32_t px[4] = {0, 0, 0, 0};               // b | g << 8 | r << 16 of the four columns (columns past the row: unused)
        for (int i = 0; i < 4; ++i)
            if (i < np) {
                const uint8_t* q = p + i * a.px_step;
                px[i] = (uint32_t)q[a.ofs_b] | (uint32_t)q[a.ofs_g] << 8 | (uint32_t)q[a.ofs_r] << 16;
            }
        o0 = px[0] | (px[1] << 24); o1 = (px[1] >> 8) | (px[2] << 16); o2 = (px[2] >> 16) | (px[3] << 8);
    }
    uint8_t* d = a.dst + (int64_t)z * a.w * a.h * 3 + ((int64_t)row * a.w + x0) * 3;
    if (a.out4) {                                    // (w % 4 == 0: every thread owns four columns)
        uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
        d4[0] = o0; d4[1] = o1; d4[2] = o2;
        return;
    }
    const uint32_t o[3] = {o0, o1, o2};
    for (int i = 0; i < 12; ++i)
        if (i < 3 * np) d[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
}

#if defined(__HIPCC__)
// grid (ceil(ceil(w/4) / YUV_TX), ceil(h / YUV_TY), n), block (YUV_TX, YUV_TY)
template <int FORM>
__global__ __launch_bounds__(YUV_TX * YUV_TY) void pixels_to_bgr_kernel(PixArgs a) {
    pixels_thread<FORM>(a, blockIdx.x * YUV_TX + threadIdx.x, blockIdx.y * YUV_TY + threadIdx.y, blockIdx.z);
}
#endif

}  // namespace slideo
